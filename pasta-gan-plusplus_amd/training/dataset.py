"""The loaders.  `TrainSet` (at the end of the module) is the training set, the reference's ``UvitonDatasetFull_512`` (training/dataset.py:404-1248);
the rest of this docstring is about the test-time loader.

Test-time loader of try-on pairs (BASELINE config 1): the reference's three test sets, chosen by ``part=`` as test.py's
``--testpart`` chooses them -- 'upper' ``UvitonDatasetFull_512_test_upper`` (training/dataset.py:1952-2728), 'lower'
``UvitonDatasetFull_512_test_lower`` (:2729-3456), 'full' ``UvitonDatasetFull_512_test_full`` (:1251-1951).  Reads the reference's
file formats and produces the 16-tuple every one of them returns (:2702-2726, :3456-3482, :1925-1950) -- uint8 CHW arrays

    image[3,512,512] clothes[3,512,512] pose[3,512,512] clothes_pose[3,512,512] norm_img[30,128,128] norm_img_lower[15,128,128]
    denorm_upper_img[3,512,512] denorm_lower_img[3,512,512] denorm_upper_mask[1,512,512] denorm_lower_mask[1,512,512]
    retain_mask[1,512,512] skin_average[3,512,512] lower_label_map[1,512,512] lower_clothes_upper_bound[1,512,512]
    person_name clothes_name

Directory layout (test.py:109-116): ``image/<name>.jpg`` (RGB JPEG, 320x512), ``parsing/<name>.png`` (L mode, LIP labels
0-19), ``garment_parsing/<name>.png`` (labels in channel 0), ``keypoints/<name>_keypoints.json`` (OpenPose-18:
``people[0].pose_keypoints_2d``, 54 floats) and a pairs file with ``<clothes_name> <person_name>`` per line.

part='outfit' is this package's own fourth mode, not one of the reference's: the top of one clothes image and the trousers or skirt of another on one
person -- 'full' with the lower garment read from a third image.  Its pairs file has ``<upper_clothes_name> <lower_clothes_name> <person_name>`` per
line; its items are 'full''s 16-tuple (with the upper clothes as the clothes) followed by the lower clothes image [3,512,512] and its name.

What is restated and what is not: the label algebra (garment-class resolution, retain / skin / bound maps) follows the
reference statement by statement; the 10-part patch routing runs on this package's kernels (training.patch_routing: HIP on a
GPU, the same arithmetic in NumPy on the CPU).  The reference rasterises the pose map and the palm masks with OpenCV, scikit-image
and pycocotools, none of which exist in this image; `_Raster` below draws the same primitives (thick segments, discs, convex
quadrilaterals, square dilation) with its own pixel-coverage rules, so those two maps are NOT pinned bit for bit against the
reference's libraries (shapes, dtypes, value sets and topology are; DESIGN.md says so).
"""

import collections
import json
import os
import random

import numpy as np
import torch

from . import patch_routing

try:
    import PIL.Image
except ImportError:                                   # pragma: no cover
    PIL = None

KPT_COLORS = [[255, 0, 0], [255, 85, 0], [255, 170, 0], [255, 255, 0], [170, 255, 0], [85, 255, 0], [0, 255, 0], [0, 255, 85], [0, 255, 170],
              [0, 255, 255], [0, 170, 255], [0, 85, 255], [0, 0, 255], [85, 0, 255], [170, 0, 255], [255, 0, 255], [255, 0, 170], [255, 0, 85], [255, 0, 0]]
LIMBS = [[2, 3], [2, 6], [3, 4], [4, 5], [6, 7], [7, 8], [2, 9], [9, 10], [10, 11], [2, 12], [12, 13], [13, 14], [2, 1], [1, 15], [15, 17],
         [1, 16], [16, 18], [3, 17], [6, 18]]
SIDE = 512
PRIMS = len(LIMBS) + 18                               # rows of a pose table (PG_FRONT_PRIMS)
ARMS = ((14, [5, 6, 7]), (15, [2, 3, 4]))             # (hand label, [shoulder, elbow, wrist]) of the palm masks
BAND_K = (35, 28)                                     # dilation of the upper-arm and the fore-arm band (csrc/tryon_front.hip: kBandK)


class _Raster:
    """Minimal rasteriser for the loader's drawings (own coverage rules; see the module docstring)."""

    @staticmethod
    def grid(h, w):
        return np.mgrid[0:h, 0:w]

    @staticmethod
    def segment(canvas, p0, p1, colour, thickness):
        """Pixels within thickness/2 of the segment p0-p1 (x, y)."""
        ys, xs = _Raster.grid(*canvas.shape[:2])
        d = np.array([p1[0] - p0[0], p1[1] - p0[1]], dtype=np.float64)
        ln = float(d @ d)
        t = np.zeros(xs.shape) if ln == 0 else np.clip(((xs - p0[0]) * d[0] + (ys - p0[1]) * d[1]) / ln, 0.0, 1.0)
        dist2 = (xs - (p0[0] + t * d[0])) ** 2 + (ys - (p0[1] + t * d[1])) ** 2
        canvas[dist2 <= (thickness / 2.0) ** 2] = colour

    @staticmethod
    def disc(canvas, centre, radius, colour):
        ys, xs = _Raster.grid(*canvas.shape[:2])
        canvas[(xs - centre[0]) ** 2 + (ys - centre[1]) ** 2 < radius ** 2] = colour

    @staticmethod
    def quad(h, w, pts):
        """Filled convex quadrilateral (4 x (x, y), in order): pixels on the same side of all four edges."""
        ys, xs = _Raster.grid(h, w)
        pts = np.asarray(pts, dtype=np.float64)
        sign = None
        inside = np.ones((h, w), dtype=bool)
        for i in range(4):
            a, b = pts[i], pts[(i + 1) % 4]
            cross = (b[0] - a[0]) * (ys - a[1]) - (b[1] - a[1]) * (xs - a[0])
            if sign is None:
                c = pts[(i + 2) % 4]
                sign = np.sign((b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0])) or 1.0
            inside &= cross * sign >= 0
        return inside

    @staticmethod
    def dilate(mask, k):
        """Square k x k dilation (anchor at the centre, as cv2.dilate with a ones kernel)."""
        h, w = mask.shape
        lo, hi = k // 2, k - 1 - k // 2
        pad = np.zeros((h + k - 1, w + k - 1), dtype=bool)
        pad[lo:lo + h, lo:lo + w] = mask
        out = np.zeros((h, w), dtype=bool)
        for dy in range(k):
            rows = pad[dy:dy + h]
            for dx in range(k):
                out |= rows[:, dx:dx + w]
        return out


def _erode_white(mask_u8, k=8):
    """(cv2.erode(mask, ones(k, k)) == 255)[..., 0:1] with the conventions of this package's paste kernel: window anchored at
    k/2, out-of-image taps ignored."""
    m = mask_u8[:, :, 0] == 255
    h, w = m.shape
    pad = np.ones((h + k, w + k), dtype=bool)
    pad[k // 2:k // 2 + h, k // 2:k // 2 + w] = m
    out = np.ones((h, w), dtype=bool)
    for dy in range(k):
        for dx in range(k):
            out &= pad[dy:dy + h, dx:dx + w]
    return out[:, :, None].astype(np.uint8)


def _bbox(mask):
    """[xmin, ymin, xmax, ymax] of the non-zero pixels, or None (dataset.py:999-1008)."""
    ys, xs = np.nonzero(mask[..., 0] >= 0.5) if mask.ndim == 3 else np.nonzero(mask >= 0.5)
    if ys.size == 0:
        return None
    return [int(xs.min()), int(ys.min()), int(xs.max()), int(ys.max())]


def _pad_square(a, fill):
    """Centre a HxW[xC] array horizontally in a HxH frame (dataset.py:2038-2040: 320 -> 512 columns)."""
    h, w = a.shape[:2]
    left = (h - w) // 2
    widths = ((0, 0), (left, h - w - left)) + ((0, 0),) * (a.ndim - 2)
    return np.pad(a, widths, 'constant', constant_values=fill), left


def _garment_classes(parsing):
    """tops / dresses / pants / skirt masks with the reference's tie-breaking (dataset.py:2083-2111): pants and skirt are merged
    into whichever is larger; a dress is attributed to tops, to the lower garment, or swallows both, by area."""
    is_ = lambda *labels: np.isin(parsing, labels).astype(np.uint8)
    tops, dresses, pants, skirt = is_(5, 7), is_(6), is_(9), is_(12)
    if pants.sum() > skirt.sum():
        pants, skirt = pants + skirt, skirt * 0
    else:
        skirt, pants = skirt + pants, pants * 0
    if dresses.sum() > 0:
        if pants.sum() > 0:
            tops, dresses = tops + dresses, dresses * 0
        elif dresses.sum() > tops.sum() + skirt.sum():
            dresses, tops, skirt = dresses + tops + skirt, tops * 0, skirt * 0
        else:
            if tops.sum() > skirt.sum():
                skirt = skirt + dresses
            else:
                tops = tops + dresses
            dresses = dresses * 0
    return tops, dresses, pants, skirt


def gt_parsing_classes(parsing):
    """The 7-class ground-truth map of a raw parsing image (dataset.py:568-594 and the weighted sum after them): 0 other, 1 tops, 2 pants, 3 skirt,
    4 dresses, 5 neck (label 10), 6 arms / legs (14-17) -> (gt_parsing in the sum's own dtype, the `_garment_classes` masks)."""
    is_ = lambda *labels: np.isin(parsing, labels).astype(np.uint8)
    hand_leg, neck = is_(14, 15, 16, 17), is_(10)
    tops, dresses, pants, skirt = _garment_classes(parsing)
    return tops * 1 + pants * 2 + skirt * 3 + dresses * 4 + neck * 5 + hand_leg * 6, (tops, dresses, pants, skirt)


class TryOnTestSet(torch.utils.data.Dataset):
    """The reference's test sets: transfer the garment(s) of `clothes_name` onto `person_name`.

    part='upper' (default): the clothes' top (``UvitonDatasetFull_512_test_upper``); the person keeps the lower garment.
    part='lower': the clothes' trousers or skirt (``UvitonDatasetFull_512_test_lower``); the person keeps the top.
    part='full': the clothes' whole outfit (``UvitonDatasetFull_512_test_full``).
    part='outfit': the top of one clothes image and the lower garment of another (`_host_outfit`; three names per line of the pairs file).
    use_sleeve_mask reads the garment parsing of the image the upper garment comes from: the clothes' (upper, full, outfit) or the person's (lower)."""

    def __init__(self, path, test_txt='test_pairs.txt', use_sleeve_mask=False, device='cpu', part='upper'):
        if PIL is None:
            raise ImportError('TryOnTestSet needs Pillow')
        if part not in patch_routing.TRYON_MODES:
            raise ValueError(f'part must be one of {sorted(patch_routing.TRYON_MODES)}, not {part!r}')
        self.path, self.use_sleeve_mask, self.device, self.part = path, use_sleeve_mask, device, part
        self.pairs = []                                      # (clothes_name, person_name), in the outfit mode (clothes_name, person_name, lower_name)
        count = 3 if part == 'outfit' else 2
        with open(os.path.join(path, test_txt)) as f:
            for line in f:
                if line.strip():
                    names = line.split()
                    if len(names) != count:
                        raise ValueError(f"{test_txt}: part={part!r} takes {count} names per line ("
                                         f"{'<upper> <lower> <person>' if count == 3 else '<clothes> <person>'}), not {line.strip()!r}")
                    self.pairs.append((names[0], names[-1]) + tuple(names[1:-1]))
        if not self.pairs:
            raise IOError('no pairs listed in ' + test_txt)

    def __len__(self):
        return len(self.pairs)

    # ------------------------------------------------------------------ file readers
    def _image(self, name):
        return np.array(PIL.Image.open(os.path.join(self.path, 'image', name)).convert('RGB'))

    def _labels(self, folder, name):
        a = np.array(PIL.Image.open(os.path.join(self.path, folder, os.path.splitext(name)[0] + '.png')))
        return (a if a.ndim == 2 else a[..., 0])[..., None]           # channel 0, as cv2.imread(...)[..., 0:1] of a grey / label image

    def _keypoints(self, name):
        with open(os.path.join(self.path, 'keypoints', os.path.splitext(name)[0] + '_keypoints.json')) as f:
            people = json.load(f)['people']
        if not people:
            return np.zeros((18, 3))
        return np.array(people[0]['pose_keypoints_2d'], dtype=np.float64).reshape(-1, 3)

    # ------------------------------------------------------------------ drawings
    @staticmethod
    def pose_table(kp, size):
        """The primitives of the coloured skeleton (dataset.py:779-813) in painting order, as int32 [PRIMS, 8] rows of (kind, x0, y0, x1, y1, r, g, b):
        kind 1 = a limb, a 5-pixel segment (x0, y0)-(x1, y1); kind 2 = a joint, a radius-5 disc at (x0, y0); kind 0 = unused row.  Leg joints too
        close to the frame are demoted to confidence 0.01 (the side effect the reference's drawing has on the keypoints).  Returns (table, kp)."""
        h, w = size
        table = np.zeros((PRIMS, 8), dtype=np.int32)
        n = 0
        for i, (a, b) in enumerate(LIMBS):
            pa, pb = kp[a - 1], kp[b - 1]
            if pa[2] < 0.05 or pb[2] < 0.05:
                continue
            table[n] = [1, int(pa[0]), int(pa[1]), int(pb[0]), int(pb[1])] + KPT_COLORS[i]
            n += 1
        for i in range(len(kp)):
            if kp[i][2] < 0.05:
                continue
            if i in (9, 10, 12, 13) and (kp[i][0] <= 0 or kp[i][1] <= 0 or kp[i][0] >= w - 50 or kp[i][1] >= h - 50):
                kp[i][2] = 0.01
                continue
            table[n] = [2, int(kp[i][0]), int(kp[i][1]), 0, 0] + KPT_COLORS[i]
            n += 1
        return table, kp

    @staticmethod
    def draw_pose(table, size):
        """The pose map uint8 [h, w, 3] of a `pose_table`: later rows paint over earlier ones."""
        canvas = np.zeros((size[0], size[1], 3), dtype=np.uint8)
        for kind, x0, y0, x1, y1, r, g, b in table.tolist():
            if kind == 1:
                _Raster.segment(canvas, (x0, y0), (x1, y1), [r, g, b], 5)
            elif kind == 2:
                _Raster.disc(canvas, (x0, y0), 5, [r, g, b])
        return canvas

    @staticmethod
    def pose_map(kp, size):
        """Coloured skeleton (dataset.py:779-813): limbs as 5-pixel segments, joints as radius-5 discs (`pose_table`, drawn)."""
        table, kp = TryOnTestSet.pose_table(kp, size)
        return TryOnTestSet.draw_pose(table, size), kp

    @staticmethod
    def _limb_band(a, b, c, d):
        """Quadrilateral around the limb (a,b)-(c,d), a quarter of its length wide on each side (dataset.py:2250-2275)."""
        ox, oy = (b - d) / 4.0, (c - a) / 4.0
        return [(a + ox, b + oy), (a - ox, b - oy), (c - ox, d - oy), (c + ox, d + oy)]

    @staticmethod
    def _arm_bands(joints):
        """(upper-arm band, fore-arm band) of one arm's (shoulder, elbow, wrist): `_limb_band` corners, or None where a joint is missing."""
        (sx, sy, sc), (ex, ey, ec), (wx, wy, wc) = joints
        upper = TryOnTestSet._limb_band(sx, sy, ex, ey) if sc > 0.1 and ec > 0.1 else None
        lower = TryOnTestSet._limb_band(ex, ey, wx, wy) if ec > 0.1 and wc > 0.1 else None
        return upper, lower

    def _arm_masks(self, joints):
        """The two bands rasterised and dilated; a missing band is all ones (it removes the whole hand label)."""
        bands = TryOnTestSet._arm_bands(joints)
        return tuple(np.ones((SIDE, SIDE), dtype=bool) if band is None else _Raster.dilate(_Raster.quad(SIDE, SIDE, band), k)
                     for band, k in zip(bands, BAND_K))

    def palm_mask(self, kp, parsing):
        """Hand label minus the upper-arm and fore-arm bands = the palms (dataset.py:753-777)."""
        out = np.zeros((SIDE, SIDE), dtype=bool)
        for label, idx in ARMS:
            upper, lower = self._arm_masks(kp[idx])
            out |= (parsing[..., 0] == label) & ~upper & ~lower
        return out[..., None].astype(np.uint8)

    # ------------------------------------------------------------------ one pair
    def _person(self, person_name):
        """The person side every mode shares (dataset.py:2031-2080 = :1330-1375 = :2807-2852), from the files."""
        raw = self._image(person_name)
        assert raw.shape[0] == SIDE, 'images are 512 pixels high (320 x 512 in the reference data)'
        table, kp = self.pose_table(self._keypoints(person_name), raw.shape[:2])       # drawn in the unpadded frame, like the reference
        kp[:, 0] += (SIDE - raw.shape[1]) // 2
        return self._person_maps(raw, table, kp, self._labels('parsing', person_name))

    def _person_maps(self, raw, table, kp, labels):
        """padded image, pose map and keypoints, parsing, retain mask, the three skin medians (NaN where the neck and face hold no pixel) of a
        decoded image [512, W, 3], its pose table, its keypoints (already in the padded frame) and its parsing [512, W, 1]."""
        image, left = _pad_square(raw, 255)
        pose, _ = _pad_square(self.draw_pose(table, raw.shape[:2]), 0)
        parsing, _ = _pad_square(labels, 0)

        is_ = lambda *labels: np.isin(parsing, labels).astype(np.uint8)
        retain_mask = is_(18, 19) + self.palm_mask(kp, parsing) + is_(1, 2, 4, 13)             # shoes + palms + head
        skin = is_(10, 13) * image                                                             # neck + face
        medians = []
        for ch in range(3):
            vals = skin[..., ch].reshape(-1)
            vals = vals[vals > 0]
            medians.append(np.median(vals) if vals.size else np.nan)
        return image, pose, kp, parsing, retain_mask, medians

    @staticmethod
    def _skin_map(medians):
        """skin_average [512, 512, 3] float64: the medians as constant planes (dataset.py:2079)."""
        return np.stack([np.full((SIDE, SIDE), m) for m in medians], axis=2)

    def _clothes(self, clothes_name):
        """The clothes side every mode shares: padded image, pose map and keypoints, parsing."""
        craw = self._image(clothes_name)
        clothes, left = _pad_square(craw, 255)
        clothes_pose, ckp = self.pose_map(self._keypoints(clothes_name), craw.shape[:2])
        clothes_pose, _ = _pad_square(clothes_pose, 0)
        ckp[:, 0] += left
        cparsing, _ = _pad_square(self._labels('parsing', clothes_name), 0)
        return clothes, clothes_pose, ckp, cparsing

    def _lower_clothes(self, lower_name):
        """The outfit mode's second clothes image, as `_clothes` gives the first."""
        return self._clothes(lower_name)

    def _sleeve(self, name):
        return self._sleeve_map(self._labels('garment_parsing', name)) if self.use_sleeve_mask else None

    @staticmethod
    def _sleeve_map(labels):
        gp, _ = _pad_square(labels, 0)
        return np.isin(gp, (10, 11)).astype(np.uint8)

    @staticmethod
    def _hip_top(kp):
        """Start of the lower garment by the hips (the upper mode's rule, `_host_upper`): an int, possibly negative, or None without both hips."""
        lhip, rhip = kp[11], kp[8]
        if lhip[2] > 0.05 and rhip[2] > 0.05:
            return int((lhip[1] + rhip[1]) / 2 - 3 * np.linalg.norm(lhip[0:2] - rhip[0:2]) / 4)
        return None

    def __getitem__(self, idx):
        return getattr(self, '_item_' + self.part)(*self.pairs[idx])

    def unrouted(self, idx):
        """Everything ``__getitem__`` computes except the patch routing and what depends on its result, for a batched route on the GPU
        (training/tryon.py).  A dict of

        upper_img, lower_img, upper_mask, lower_mask  uint8 [512, 512, 3]: the routing inputs of ``patch_routing.normalize_batch``
        sleeve                                         uint8 [512, 512, 1] or None; clothes_kp, person_kp float64 [18, 3]
        image, clothes, pose                           uint8 [512, 512, 3] as read (HWC); retain_mask uint8 [512, 512, 1]
        skin                                           float64 [3]: the skin medians, NaN kept
        label                                          int: 0, 1 or 2
        bound                                          uint8 [512]: the host part of lower_clothes_upper_bound, one value per row (the bound is
                                                       constant along each row in every mode); the upper and full modes finish it from the
                                                       routed canvases (training.tryon.final_bound)
        canvas                                         uint8 [512, 512, 3] or None: the mode's host-computed garment canvas -- the person's eroded
                                                       lower garment (upper) or eroded top (lower); None in the full and outfit modes
        person_name, clothes_name
        lower_kp, lower_clothes, lower_name            outfit mode only: the lower clothes' key points, image (padded with 255, HWC) and name;
                                                       clothes, clothes_kp and clothes_name are the upper clothes'"""
        return self._unrouted(*self.pairs[idx])

    def _unrouted(self, clothes_name, person_name, *lower_name):
        h = getattr(self, '_host_' + self.part)(clothes_name, person_name, *lower_name)
        up, lo, um, lm, sleeve, ckp, kp = h['routing'][:7]
        item = dict(upper_img=up, lower_img=lo, upper_mask=um, lower_mask=lm, sleeve=sleeve, clothes_kp=ckp, person_kp=kp, image=h['image'],
                    clothes=h['clothes'], pose=h['pose'], retain_mask=h['retain_mask'], skin=np.array(h['medians'], dtype=np.float64),
                    label=int(h['label']), bound=np.ascontiguousarray(h['bound'][:, 0, 0]), canvas=h['canvas'], person_name=person_name,
                    clothes_name=clothes_name)
        if lower_name:
            item.update(lower_kp=h['routing'][7], lower_clothes=h['lower_clothes'], lower_name=lower_name[0])
        return item

    def raw(self, idx):
        """File decoding and keypoint arithmetic only -- what ``training.tryon_front.front_batch`` turns into the ``unrouted`` maps on the GPU.
        A dict of

        person_img, clothes_img            uint8 [512, W, 3] as decoded (not padded); person_parsing, clothes_parsing uint8 [512, W]
        garment_parsing                    uint8 [512, W] or None: of the image the sleeve mask is read from (the clothes' in the upper and full modes,
                                           the person's in the lower mode); None without use_sleeve_mask
        person_kp, clothes_kp              float64 [18, 3], as ``unrouted`` returns them (leg joints demoted, x shifted into the padded frame)
        pose_prims                         int32 [PRIMS, 8]: the person's `pose_table`
        bands, band_absent                 float64 [4, 4, 2], int32 [4]: the `_limb_band` corners of the four arm bands (`ARMS` order, upper arm then
                                           fore-arm) in the padded frame; absent = 1 where a joint is missing (the band is then "all ones")
        hip_top                            `_hip_top` of the person: an int or None (read by the upper mode only)
        person_name, clothes_name
        lower_img, lower_parsing, lower_kp, lower_name     outfit mode only: the lower clothes', as clothes_img, clothes_parsing, clothes_kp, clothes_name"""
        clothes_name, person_name = self.pairs[idx][:2]
        person_img, clothes_img = self._image(person_name), self._image(clothes_name)
        assert person_img.shape[0] == SIDE and clothes_img.shape[0] == SIDE, 'images are 512 pixels high (320 x 512 in the reference data)'
        table, kp = self.pose_table(self._keypoints(person_name), person_img.shape[:2])
        kp[:, 0] += (SIDE - person_img.shape[1]) // 2
        _, ckp = self.pose_table(self._keypoints(clothes_name), clothes_img.shape[:2])
        ckp[:, 0] += (SIDE - clothes_img.shape[1]) // 2
        bands, absent = np.zeros((4, 4, 2)), np.zeros(4, dtype=np.int32)
        for arm, (_, idx3) in enumerate(ARMS):
            for j, band in enumerate(self._arm_bands(kp[idx3])):
                if band is None:
                    absent[2 * arm + j] = 1
                else:
                    bands[2 * arm + j] = band
        garment = None
        if self.use_sleeve_mask:
            garment = self._labels('garment_parsing', person_name if self.part == 'lower' else clothes_name)[..., 0]
        item = dict(person_img=person_img, clothes_img=clothes_img, person_parsing=self._labels('parsing', person_name)[..., 0],
                    clothes_parsing=self._labels('parsing', clothes_name)[..., 0], garment_parsing=garment, person_kp=kp, clothes_kp=ckp,
                    pose_prims=table, bands=bands, band_absent=absent, hip_top=self._hip_top(kp), person_name=person_name, clothes_name=clothes_name)
        if self.part == 'outfit':
            lower_name = self.pairs[idx][2]
            lower_img = self._image(lower_name)
            assert lower_img.shape[0] == SIDE, 'images are 512 pixels high (320 x 512 in the reference data)'
            _, lkp = self.pose_table(self._keypoints(lower_name), lower_img.shape[:2])
            lkp[:, 0] += (SIDE - lower_img.shape[1]) // 2
            item.update(lower_img=lower_img, lower_parsing=self._labels('parsing', lower_name)[..., 0], lower_kp=lkp, lower_name=lower_name)
        return item

    # ------------------------------------------------------------------ the three modes: host half (before the routing), then the rest
    def _host_upper(self, clothes_name, person_name):
        """dataset.py:2030-2224 up to the routing, plus what does not depend on it."""
        image, pose, kp, parsing, retain_mask, medians = self._person(person_name)
        tops, dresses, pants, skirt = _garment_classes(parsing)
        lower_mask = skirt + pants
        lower_image = lower_mask * image
        lower_bbox = _bbox(lower_mask.copy())
        bound = np.zeros((SIDE, SIDE, 1), dtype=np.uint8)
        via_kps = self._hip_top(kp)
        if via_kps is not None:                              # start of the lower garment: the hips, or the parsing if that is higher
            top = via_kps if lower_bbox is None else min(lower_bbox[1], via_kps)
            bound[top:] += 255                               # (NumPy slice semantics, negative values included, as in the reference)
        elif lower_bbox is not None:
            bound[lower_bbox[1]:] += 255

        clothes, clothes_pose, ckp, cparsing = self._clothes(clothes_name)
        ctops, cdresses, _, _ = _garment_classes(cparsing)
        upper_mask = ctops + cdresses
        upper_image = upper_mask * clothes
        if cdresses.sum() > 0:                               # a dress replaces the person's lower garment entirely
            lower_mask, pants, skirt, lower_image, bound = lower_mask * 0, pants * 0, skirt * 0, lower_image * 0, bound * 0
        upper_rgb, lower_rgb = np.repeat(upper_mask, 3, axis=2) * 255, np.repeat(lower_mask, 3, axis=2) * 255
        sleeve = self._sleeve(clothes_name)
        routing = (upper_image.astype(np.uint8), lower_image.astype(np.uint8), upper_rgb.astype(np.uint8), lower_rgb.astype(np.uint8), sleeve, ckp, kp)
        denorm_lower = lower_image * _erode_white(lower_rgb.astype(np.uint8))                  # the person's own lower garment, edge eroded
        label = 0.0 if pants.sum() > 0 else (1.0 if skirt.sum() > 0 else (2.0 if cdresses.sum() > 0 else 1.0))
        return dict(routing=routing, image=image, clothes=clothes, pose=pose, clothes_pose=clothes_pose, retain_mask=retain_mask, medians=medians,
                    label=label, bound=bound, canvas=denorm_lower.astype(np.uint8))

    def _item_upper(self, clothes_name, person_name):
        h = self._host_upper(clothes_name, person_name)
        routed = patch_routing.normalize(*h['routing'], 2, device=self.device)
        norm_img, norm_img_lower, denorm_upper, denorm_upper_wo_sleeve, _ = (t.cpu().numpy() for t in routed)
        bound = h['bound']
        upper_bbox = _bbox((denorm_upper_wo_sleeve.sum(axis=2, keepdims=True) > 0).astype(np.uint8))
        if upper_bbox is not None:
            bound[0:upper_bbox[3]] *= 0
        return self._pack(h['image'], h['clothes'], h['pose'], h['clothes_pose'], norm_img, norm_img_lower, denorm_upper, h['canvas'], h['retain_mask'],
                          self._skin_map(h['medians']), h['label'], bound, person_name, clothes_name)

    def _host_lower(self, clothes_name, person_name):
        """dataset.py:2806-2981: the person keeps the top (re-pasted with an 8 x 8 eroded edge), the clothes' lower garment is routed."""
        image, pose, kp, parsing, retain_mask, medians = self._person(person_name)
        tops, dresses, pants, skirt = _garment_classes(parsing)                                # the PERSON's garment classes
        upper_mask = tops + dresses
        upper_image = upper_mask * image
        lower_bbox = _bbox((skirt + pants).copy())
        bound = np.zeros((SIDE, SIDE, 1), dtype=np.uint8)
        if lower_bbox is not None:                           # start of the lower garment: the person's own one (no hip rule here)
            bound[lower_bbox[1]:] += 255
        sleeve = self._sleeve(person_name)                   # the person's garment parsing: the top stays the person's

        clothes, clothes_pose, ckp, cparsing = self._clothes(clothes_name)
        _, _, cpants, cskirt = _garment_classes(cparsing)
        lower_mask = cskirt + cpants
        lower_image = lower_mask * clothes
        if dresses.sum() > 0:                                # a person in a dress keeps it: nothing of the clothes' lower garment is routed
            cskirt, cpants, lower_mask, lower_image, bound = cskirt * 0, cpants * 0, lower_mask * 0, lower_image * 0, bound * 0
        upper_rgb, lower_rgb = np.repeat(upper_mask, 3, axis=2) * 255, np.repeat(lower_mask, 3, axis=2) * 255
        routing = (upper_image.astype(np.uint8), lower_image.astype(np.uint8), upper_rgb.astype(np.uint8), lower_rgb.astype(np.uint8), sleeve, ckp, kp)
        denorm_upper = upper_image * _erode_white(upper_rgb.astype(np.uint8))                  # the person's own top, edge eroded (8 x 8)
        label = 0.0 if cpants.sum() > 0 else (1.0 if cskirt.sum() > 0 else (2.0 if dresses.sum() > 0 else 1.0))
        return dict(routing=routing, image=image, clothes=clothes, pose=pose, clothes_pose=clothes_pose, retain_mask=retain_mask, medians=medians,
                    label=label, bound=bound, canvas=denorm_upper.astype(np.uint8))

    def _item_lower(self, clothes_name, person_name):
        h = self._host_lower(clothes_name, person_name)
        routed = patch_routing.normalize(*h['routing'], 2, device=self.device, part='lower')
        norm_img, norm_img_lower, _, denorm_lower = (t.cpu().numpy() for t in routed)
        return self._pack(h['image'], h['clothes'], h['pose'], h['clothes_pose'], norm_img, norm_img_lower, h['canvas'], denorm_lower, h['retain_mask'],
                          self._skin_map(h['medians']), h['label'], h['bound'], person_name, clothes_name)

    def _host_full(self, clothes_name, person_name):
        """dataset.py:1329-1464: both garments come from the clothes image, the garment classes from the CLOTHES' parsing."""
        image, pose, kp, parsing, retain_mask, medians = self._person(person_name)
        clothes, clothes_pose, ckp, cparsing = self._clothes(clothes_name)
        ctops, cdresses, cpants, cskirt = _garment_classes(cparsing)
        upper_mask, lower_mask = ctops + cdresses, cskirt + cpants
        upper_image, lower_image = upper_mask * clothes, lower_mask * clothes
        upper_rgb, lower_rgb = np.repeat(upper_mask, 3, axis=2) * 255, np.repeat(lower_mask, 3, axis=2) * 255
        sleeve = self._sleeve(clothes_name)
        routing = (upper_image.astype(np.uint8), lower_image.astype(np.uint8), upper_rgb.astype(np.uint8), lower_rgb.astype(np.uint8), sleeve, ckp, kp)
        bound = np.zeros((SIDE, SIDE, 1), dtype=np.uint8)    # start of the lower garment: the routed one's top row (after the routing)
        if cpants.sum() > 0:
            label = 0.0
        elif cskirt.sum() > 0:
            label = 1.0
        elif cdresses.sum() > 0:                             # a dress as the outfit: no lower garment, no bound
            label = 2.0
        else:
            label = 1.0
        return dict(routing=routing, image=image, clothes=clothes, pose=pose, clothes_pose=clothes_pose, retain_mask=retain_mask, medians=medians,
                    label=label, bound=bound, canvas=None)

    def _item_full(self, clothes_name, person_name):
        h = self._host_full(clothes_name, person_name)
        routed = patch_routing.normalize(*h['routing'], 2, device=self.device, part='full')
        norm_img, norm_img_lower, denorm_upper, denorm_lower = (t.cpu().numpy() for t in routed)
        bound = h['bound']
        lower_bbox = _bbox((denorm_lower.sum(axis=2, keepdims=True) > 0).astype(np.uint8))
        if lower_bbox is not None:
            bound[lower_bbox[1]:] += 255
        if h['label'] == 2.0:
            bound = bound * 0
        return self._pack(h['image'], h['clothes'], h['pose'], h['clothes_pose'], norm_img, norm_img_lower, denorm_upper, denorm_lower, h['retain_mask'],
                          self._skin_map(h['medians']), h['label'], bound, person_name, clothes_name)

    def _host_outfit(self, clothes_name, person_name, lower_name):
        """`_host_full`'s statements with the lower-garment quantities taken from a second clothes image: the top (tops + dresses, the sleeve mask, the
        key points that route the upper parts) from `clothes_name`, the trousers or skirt and the key points that route lower parts 0, 6 to 9 from
        `lower_name`.  Nothing is zeroed for a dress: as 'full' routes a clothes image whose parsing holds a dress and pants, both garments are routed."""
        image, pose, kp, parsing, retain_mask, medians = self._person(person_name)
        clothes, clothes_pose, ckp, cparsing = self._clothes(clothes_name)
        lower_clothes, _, lkp, lparsing = self._lower_clothes(lower_name)
        ctops, cdresses, _, _ = _garment_classes(cparsing)
        _, _, cpants, cskirt = _garment_classes(lparsing)
        upper_mask, lower_mask = ctops + cdresses, cskirt + cpants
        upper_image, lower_image = upper_mask * clothes, lower_mask * lower_clothes
        upper_rgb, lower_rgb = np.repeat(upper_mask, 3, axis=2) * 255, np.repeat(lower_mask, 3, axis=2) * 255
        sleeve = self._sleeve(clothes_name)
        routing = (upper_image.astype(np.uint8), lower_image.astype(np.uint8), upper_rgb.astype(np.uint8), lower_rgb.astype(np.uint8), sleeve, ckp, kp, lkp)
        bound = np.zeros((SIDE, SIDE, 1), dtype=np.uint8)    # start of the lower garment: the routed one's top row (after the routing)
        if cpants.sum() > 0:
            label = 0.0
        elif cskirt.sum() > 0:
            label = 1.0
        elif cdresses.sum() > 0:                             # a dress on top and no lower garment: no bound
            label = 2.0
        else:
            label = 1.0
        return dict(routing=routing, image=image, clothes=clothes, pose=pose, clothes_pose=clothes_pose, retain_mask=retain_mask, medians=medians,
                    label=label, bound=bound, canvas=None, lower_clothes=lower_clothes)

    def _item_outfit(self, clothes_name, person_name, lower_name):
        h = self._host_outfit(clothes_name, person_name, lower_name)
        routed = patch_routing.normalize(*h['routing'][:7], 2, device=self.device, part='outfit', lower_keypoints=h['routing'][7])
        norm_img, norm_img_lower, denorm_upper, denorm_lower = (t.cpu().numpy() for t in routed)
        bound = h['bound']
        lower_bbox = _bbox((denorm_lower.sum(axis=2, keepdims=True) > 0).astype(np.uint8))
        if lower_bbox is not None:
            bound[lower_bbox[1]:] += 255
        if h['label'] == 2.0:
            bound = bound * 0
        item = self._pack(h['image'], h['clothes'], h['pose'], h['clothes_pose'], norm_img, norm_img_lower, denorm_upper, denorm_lower, h['retain_mask'],
                          self._skin_map(h['medians']), h['label'], bound, person_name, clothes_name)
        return item + (np.ascontiguousarray(np.transpose(h['lower_clothes'], (2, 0, 1))), lower_name)

    @staticmethod
    def _pack(image, clothes, pose, clothes_pose, norm_img, norm_img_lower, denorm_upper, denorm_lower, retain_mask, skin_average, label, bound,
              person_name, clothes_name):
        """The 16-tuple of ``__getitem__`` (dataset.py:2702-2726)."""
        lower_label_map = np.full((SIDE, SIDE, 1), label / 2.0 * 255)
        chw = lambda a: np.ascontiguousarray(np.transpose(a, (2, 0, 1)))
        denorm_upper, denorm_lower = chw(denorm_upper), chw(denorm_lower.astype(np.uint8))
        return (chw(image), chw(clothes), chw(pose), chw(clothes_pose), chw(norm_img), chw(norm_img_lower), denorm_upper, denorm_lower,
                (denorm_upper.sum(axis=0, keepdims=True) > 0).astype(np.uint8), (denorm_lower.sum(axis=0, keepdims=True) > 0).astype(np.uint8),
                chw(retain_mask), chw(skin_average), chw(lower_label_map), chw(bound), person_name, clothes_name)


def to_generator_inputs(batch, device):
    """The tensor preparation of test.py:126-147: uint8 arrays of `TryOnTestSet` (stacked by a DataLoader) -> the keyword
    arguments of ``GeneratorFull_v20.forward``."""
    (image, clothes, pose, _, norm_img, norm_img_lower, den_up, den_lo, den_up_mask, den_lo_mask, retain_mask, skin_average, lower_label_map,
     lower_bound) = [torch.as_tensor(t).to(device) for t in batch[:14]]
    unit = lambda t: t.to(torch.float32) / 127.5 - 1
    image_t, retain = unit(image), retain_mask.to(torch.float32)
    retain_t = torch.cat([image_t * retain - (1 - retain), unit(skin_average)], dim=1)
    return dict(z=torch.zeros([image.shape[0], 0], device=device), c=torch.cat([unit(norm_img), unit(norm_img_lower)], dim=1), retain=retain_t,
                pose=torch.cat([unit(pose), unit(lower_label_map), unit(lower_bound)], dim=1),
                denorm_upper_input=unit(den_up), denorm_lower_input=unit(den_lo),
                denorm_upper_mask=den_up_mask.to(torch.float32), denorm_lower_mask=den_lo_mask.to(torch.float32))


_NAME_KEYS, _LOWER_NAME_KEYS = ('clothes_kp', 'person_kp', 'person_name', 'clothes_name'), ('lower_kp', 'lower_name')     # the lists of a batch
_UNROUTED_ARRAYS = ('upper_img', 'lower_img', 'upper_mask', 'lower_mask', 'sleeve', 'image', 'clothes', 'pose', 'retain_mask', 'bound', 'canvas')


def collate_unrouted(items, pin=False):
    """Stack ``TryOnTestSet.unrouted`` items into a batch: the uint8 arrays as [N, ...] tensors (pinned with pin=True -- only in the process that
    owns the GPU; a DataLoader with workers pins them itself with ``pin_memory=True``), skin as float32 [N, 3] (the cast
    ``skin_average.to(torch.float32)`` of test.py:133, NaN kept), label as int32 [N]; keypoints and names stay lists.  Keys whose value is None
    (sleeve without the sleeve mask, canvas in the full and outfit modes) stay None.  Outfit items add lower_clothes (after canvas), lower_kp and
    lower_name (at the end); batches of the other modes do not have these keys."""
    outfit = 'lower_clothes' in items[0]
    out = {}
    for k in _UNROUTED_ARRAYS + (('lower_clothes',) if outfit else ()):
        if items[0][k] is None:
            out[k] = None
            continue
        t = torch.from_numpy(np.stack([it[k] for it in items]))
        out[k] = t.pin_memory() if pin else t
    skin = torch.from_numpy(np.stack([it['skin'] for it in items])).to(torch.float32)
    label = torch.tensor([it['label'] for it in items], dtype=torch.int32)
    out['skin'], out['label'] = (skin.pin_memory(), label.pin_memory()) if pin else (skin, label)
    for k in _NAME_KEYS + (_LOWER_NAME_KEYS if outfit else ()):
        out[k] = [it[k] for it in items]
    return out


_RAW_ARRAYS = ('person_img', 'clothes_img', 'person_parsing', 'clothes_parsing', 'garment_parsing', 'pose_prims', 'bands', 'band_absent')
_RAW_LOWER_ARRAYS = ('lower_img', 'lower_parsing')    # outfit batches only
_HIP_CLAMP = 1 << 20                                  # far beyond the frame on either side: the slice ``bound[top:]`` is the same


def collate_raw(items, pin=False):
    """Stack ``TryOnTestSet.raw`` items into a batch: the arrays as [N, ...] tensors (pinned with pin=True, as `collate_unrouted`), garment_parsing None
    without the sleeve mask, hip_top as int32 [N, 2] = (valid, row); keypoints and names stay lists.  Outfit items add lower_img and lower_parsing
    (after band_absent), lower_kp and lower_name (at the end)."""
    outfit = 'lower_img' in items[0]
    out = {}
    for k in _RAW_ARRAYS + (_RAW_LOWER_ARRAYS if outfit else ()):
        out[k] = None if items[0][k] is None else torch.from_numpy(np.stack([it[k] for it in items]))
    out['hip_top'] = torch.tensor([[0, 0] if it['hip_top'] is None else [1, max(-_HIP_CLAMP, min(_HIP_CLAMP, it['hip_top']))] for it in items],
                                  dtype=torch.int32)
    if pin:
        out = {k: (None if v is None else v.pin_memory()) for k, v in out.items()}
    for k in _NAME_KEYS + (_LOWER_NAME_KEYS if outfit else ()):
        out[k] = [it[k] for it in items]
    return out


class _RawPair(TryOnTestSet):
    """One ``raw`` item behind the loader's host code: the readers of `_host_<part>` answer from the decoded arrays instead of the files."""

    def __init__(self, item, part):
        self.item, self.part, self.use_sleeve_mask, self.device = item, part, item['garment_parsing'] is not None, 'cpu'

    def _person(self, person_name):
        it = self.item
        return self._person_maps(it['person_img'], it['pose_prims'], it['person_kp'].copy(), it['person_parsing'][..., None])

    def _clothes(self, clothes_name):
        it = self.item
        clothes, _ = _pad_square(it['clothes_img'], 255)
        cparsing, _ = _pad_square(it['clothes_parsing'][..., None], 0)
        return clothes, None, it['clothes_kp'].copy(), cparsing         # (no clothes pose map: `unrouted` does not carry it)

    def _lower_clothes(self, lower_name):
        it = self.item
        lower, _ = _pad_square(it['lower_img'], 255)
        lparsing, _ = _pad_square(it['lower_parsing'][..., None], 0)
        return lower, None, it['lower_kp'].copy(), lparsing

    def _sleeve(self, name):
        return self._sleeve_map(self.item['garment_parsing'][..., None]) if self.use_sleeve_mask else None


def unrouted_from_raw(item, part):
    """``TryOnTestSet.unrouted`` of a ``raw`` item, through the same host statements (the CPU route of ``training.tryon_front.front_batch``)."""
    return _RawPair(item, part)._unrouted(item['clothes_name'], item['person_name'], *((item['lower_name'],) if part == 'outfit' else ()))


# ------------------------------------------------------------------------------------------------------------- the training set

DATASET_LIST = ['Zalando_512_320_v1', 'Zalando_512_320_v2', 'Zalora_512_320_v1', 'Zalora_512_320_v2', 'Deepfashion_512_320', 'MPV_512_320',
                'ZMO_dresses_512_320', 'Zalando_512_320_v1_flip', 'Zalando_512_320_v2_flip', 'Zalora_512_320_v1_flip', 'Zalora_512_320_v2_flip',
                'Deepfashion_512_320_flip', 'MPV_512_320_flip', 'ZMO_dresses_512_320_flip']                  # dataset.py:415-421
TRAIN_LIST = 'train_pairs_front_list_220508.txt'
ERASE_NONE, ERASE_DROP_PART0, ERASE_BAND = 0, 1, 2            # enum pg_erase_kind (include/pasta_gan_ops.h)

# The random decisions of one training item (dataset.py:1160-1170, :1226), drawn on the host and applied where the routed patches are:
# kind: ERASE_*; rows: with ERASE_DROP_PART0, also erase the top `erase_length` rows of lower parts 1 and 3; u in [0, 1): with ERASE_BAND, rows
# ty : ty + 1 + floor(u * (h - ty)) of lower part 0 (ty = first row of its routed mask); use_random_mask: erase the canvases under the item's random mask.
EraseRecord = collections.namedtuple('EraseRecord', 'kind rows erase_length u use_random_mask')
NO_ERASE = EraseRecord(ERASE_NONE, 0, 0, 0.0, 0)


def sample_record(rng, h=SIDE // 4):
    """One `EraseRecord` from `rng` (a ``random.Random``), with the reference's probabilities: none 0.20, drop_part0 0.8 * 0.6 = 0.48 (its row erase
    0.75, erase_length uniform on 1 ... h // 10), band 0.8 * 0.4 = 0.32; random mask 0.9.  The reference draws from the global ``random`` and only if
    the routed lower mask is non-empty; this draws every field's decision up front, so its stream is not the reference's."""
    kind, rows, erase_length, u = ERASE_NONE, 0, 0, 0.0
    if rng.random() < 0.80:
        if rng.random() < 0.6:
            kind = ERASE_DROP_PART0
            if rng.random() < 0.75:
                rows, erase_length = 1, rng.randint(1, h // 10)
        else:
            kind, u = ERASE_BAND, float(np.float32(rng.random()))
            if u >= 1.0:                                      # (the float32 rounding of a draw within 2**-25 of 1)
                u = float(np.nextafter(np.float32(1), np.float32(0)))
    return EraseRecord(kind, rows, erase_length, u, int(rng.random() < 0.9))


def apply_erase(norm_img_lower, masks_lower, record):
    """``norm_img_lower_for_train`` (dataset.py:1146-1170) of a routed [h, w, 15] uint8 array and its routed masks, for a given record (NumPy)."""
    out = norm_img_lower.copy()
    bbox = _bbox(masks_lower[..., 0:1].copy())
    if bbox is None or record.kind == ERASE_NONE:
        return out
    h = out.shape[0]
    if record.kind == ERASE_DROP_PART0:
        out[..., 0:3] = 0
        if record.rows:
            out[0:record.erase_length, :, 3:6] = 0
            out[0:record.erase_length, :, 9:12] = 0
    else:
        ty = bbox[1]
        by = min(ty + 1 + int(np.floor(np.float32(record.u) * np.float32(h - ty))), h)
        out[ty:by, :, 0:3] = 0
    return out


class TrainSet(torch.utils.data.Dataset):
    """The reference's training set ``UvitonDatasetFull_512`` (dataset.py:404-1248) for its directory layout: ``<path>/<dataset>/{image,keypoints,
    parsing,garment_parsing}/...`` listed by ``<path>/<dataset>/train_pairs_front_list_220508.txt`` (first column; ``_label.png`` parsing names for
    Deepfashion_512_320 and MPV_512_320) and ``<path>/train_random_mask_acgpn/*``.  Sub-datasets of `dataset_list` that are absent are skipped;
    ``train_img_front_vis_512_220414`` is optional (`vis_index` is empty without it).  One person per item, routed through their own key points.

    ``ds[idx]`` is the reference's 19-tuple (:1198-1248), routed on `device` ('cpu' = the NumPy route):

        image[3,512,512] pose[3,512,512] norm_img[30,128,128] norm_img_lower[15,128,128] norm_img_lower_for_train[15,128,128]
        denorm_upper_img_erase[3,512,512] denorm_lower_img_erase[3,512,512] Ms[10,3,3] M_invs[10,3,3] gt_parsing[1,512,512]
        denorm_upper_mask[1,512,512] denorm_lower_mask[1,512,512] norm_clothes_masks[30,128,128] norm_clothes_masks_lower[15,128,128]
        retain_mask[1,512,512] skin_median[3,512,512] lower_label_map[1,512,512] lower_clothes_upper_bound_for_train[1,512,512] ..._for_test[1,512,512]

    (uint8, except Ms / M_invs / skin_median / lower_label_map: float64).  ``ds.unrouted(idx)`` is what the host makes before the routing, for the
    batched GPU route (training/train_fetch.py).  The random decisions come from `sample_record` on a ``random.Random`` seeded by (seed, DataLoader
    worker, index, how often this worker has drawn for the index): reproducible, not the reference's draw-for-draw stream."""

    def __init__(self, path, dataset_list=None, shuffle=True, seed=0, device='cpu'):
        if PIL is None:
            raise ImportError('TrainSet needs Pillow')
        if not os.path.isdir(path):
            raise IOError('Path must point to a directory')
        self.path, self.device, self.seed = path, device, seed
        names = []                                            # (image, keypoints, parsing, garment_parsing), relative to path
        for dataset in (DATASET_LIST if dataset_list is None else dataset_list):
            txt = os.path.join(path, dataset, TRAIN_LIST)
            if not os.path.isfile(txt):
                continue
            label_suffix = '_label.png' if dataset in ('Deepfashion_512_320', 'MPV_512_320') else '.png'
            with open(txt) as f:
                for line in f:
                    if not line.strip():
                        continue
                    person = line.strip().split()[0]
                    names.append((os.path.join(dataset, 'image', person), os.path.join(dataset, 'keypoints', person.replace('.jpg', '_keypoints.json')),
                                  os.path.join(dataset, 'parsing', person.replace('.jpg', label_suffix)),
                                  os.path.join(dataset, 'garment_parsing', person.replace('.jpg', '.png'))))
        if not names:
            raise IOError('No image files found in the specified path')
        if shuffle:
            random.Random(seed).shuffle(names)
        self.names = names
        images = [n[0] for n in names]
        self.vis_index = []
        vis_dir = os.path.join(path, 'train_img_front_vis_512_220414')
        if os.path.isdir(vis_dir):                            # dataset.py:447-461
            for image_name in sorted(os.listdir(vis_dir)):
                for cand in (os.path.join('Zalando_512_320_v1', 'image', image_name), os.path.join('Deepfashion_512_320', 'image', 'train', image_name),
                             os.path.join('Zalora_512_320_v2', 'image', image_name)):
                    if cand in images:
                        self.vis_index.append(images.index(cand))
                        break
        mask_dir = os.path.join(path, 'train_random_mask_acgpn')
        self.random_masks = [os.path.join(mask_dir, m) for m in sorted(os.listdir(mask_dir))] if os.path.isdir(mask_dir) else []
        if not self.random_masks:
            raise IOError('no random masks in ' + mask_dir)
        self._visits = collections.Counter()

    pose_map = staticmethod(TryOnTestSet.pose_map)            # the drawing statements agree with the training class (:698-823)
    _limb_band = staticmethod(TryOnTestSet._limb_band)
    _arm_masks = TryOnTestSet._arm_masks
    palm_mask = TryOnTestSet.palm_mask

    def __len__(self):
        return len(self.names)

    def record(self, idx):
        """The next `EraseRecord` of item `idx` in this process."""
        info = torch.utils.data.get_worker_info()
        visit = self._visits[idx]
        self._visits[idx] += 1
        return sample_record(random.Random(f'{self.seed}/{0 if info is None else info.id}/{int(idx)}/{visit}'))

    def _labels(self, name):
        a = np.array(PIL.Image.open(os.path.join(self.path, name)))
        return (a if a.ndim == 2 else a[..., 0])[..., None]

    def _random_mask(self, idx):
        a = np.array(PIL.Image.open(self.random_masks[idx % len(self.random_masks)]))
        return np.ascontiguousarray((a if a.ndim == 2 else a[..., 0])[..., None])

    def _host(self, idx):
        """``_load_raw_image`` up to the routing (dataset.py:507-632, :644-651)."""
        image_name, kpt_name, parsing_name, garment_name = self.names[idx]
        raw = np.array(PIL.Image.open(os.path.join(self.path, image_name)).convert('RGB'))
        assert raw.shape[0] == SIDE, 'images are 512 pixels high (320 x 512 in the reference data)'
        image, left = _pad_square(raw, 255)
        with open(os.path.join(self.path, kpt_name)) as f:
            people = json.load(f)['people']
        kp = np.array(people[0]['pose_keypoints_2d'], dtype=np.float64).reshape(-1, 3) if people else np.zeros((18, 3))
        pose, kp = self.pose_map(kp, raw.shape[:2])
        pose, _ = _pad_square(pose, 0)
        kp[:, 0] += left
        garment_parsing, _ = _pad_square(self._labels(garment_name), 0)
        sleeve = np.isin(garment_parsing, (10, 11)).astype(np.uint8)
        parsing, _ = _pad_square(self._labels(parsing_name), 0)

        is_ = lambda *labels: np.isin(parsing, labels).astype(np.uint8)
        retain_mask = is_(18, 19) + self.palm_mask(kp, parsing) + is_(1, 2, 4, 13)             # shoes + palms + head
        skin = is_(10, 13) * image
        medians = []
        for ch in range(3):
            vals = skin[..., ch].reshape(-1)
            vals = vals[vals > 0]
            medians.append(np.median(vals) if vals.size else np.nan)
        gt_parsing, (tops, dresses, pants, skirt) = gt_parsing_classes(parsing)               # (also calc_metrics.py's label windows)
        lower_mask, upper_mask = skirt + pants, tops + dresses
        upper_rgb, lower_rgb = np.repeat(upper_mask, 3, axis=2) * 255, np.repeat(lower_mask, 3, axis=2) * 255

        lower_bbox = _bbox(lower_mask.copy())
        bound_train = np.zeros(SIDE, dtype=np.uint8)          # one value per row: the maps are constant along each row
        if lower_bbox is not None:
            bound_train[lower_bbox[1]:] += 255
        bound_test = np.zeros(SIDE, dtype=np.uint8)
        lhip, rhip = kp[11], kp[8]
        if lhip[2] > 0.05 and rhip[2] > 0.05:
            via_kps = int((lhip[1] + rhip[1]) / 2 - np.linalg.norm(lhip[0:2] - rhip[0:2]) / 2)
            top = via_kps if lower_bbox is None else min(lower_bbox[1], via_kps)
            bound_test[top:] += 255                           # (NumPy slice semantics, negative values included, as in the reference)
        elif lower_bbox is not None:
            bound_test[lower_bbox[1]:] += 255
        label = 0 if pants.sum() > 0 else (1 if skirt.sum() > 0 else (2 if dresses.sum() > 0 else 1))
        return dict(upper_img=(upper_mask * image).astype(np.uint8), lower_img=(lower_mask * image).astype(np.uint8), upper_mask=upper_rgb.astype(np.uint8),
                    lower_mask=lower_rgb.astype(np.uint8), sleeve=sleeve, person_kp=kp, image=image, pose=pose, gt_parsing=gt_parsing.astype(np.uint8),
                    retain_mask=retain_mask, skin=np.array(medians, dtype=np.float64), label=label, bound_train=bound_train, bound_test=bound_test,
                    name=image_name)

    def unrouted(self, idx, record=None):
        """Everything the host makes of item `idx`, before the routing: a dict of

        upper_img, lower_img, upper_mask, lower_mask   uint8 [512, 512, 3]: the routing inputs of ``patch_routing.normalize_batch(part='train')``
        sleeve                                         uint8 [512, 512, 1]; person_kp float64 [18, 3]
        image, pose                                    uint8 [512, 512, 3] (HWC); gt_parsing, retain_mask uint8 [512, 512, 1]
        skin                                           float64 [3]: the skin medians, NaN kept; label int: 0, 1 or 2
        bound_train, bound_test                        uint8 [512]: the two bound maps, one value per row
        random_mask                                    uint8 [512, 512, 1], or None when the record does not use it
        record                                         the `EraseRecord` (drawn with ``self.record(idx)`` unless given); name"""
        item = self._host(idx)
        item['record'] = rec = self.record(idx) if record is None else record
        item['random_mask'] = self._random_mask(idx) if rec.use_random_mask else None
        return item

    def __getitem__(self, idx):
        return self.item(idx)

    def item(self, idx, record=None):
        """The 19-tuple of item `idx` under `record` (drawn unless given)."""
        u = self.unrouted(idx, record)
        routed = patch_routing.normalize(u['upper_img'], u['lower_img'], u['upper_mask'], u['lower_mask'], u['sleeve'], u['person_kp'], u['person_kp'], 2,
                                         device=self.device, part='train')
        norm_img, norm_img_lower, denorm_upper, denorm_lower, masks, masks_lower = (t.cpu().numpy() for t in routed)
        for_train = apply_erase(norm_img_lower, masks_lower, u['record'])
        ms, m_invs = patch_routing.crop_matrices(u['person_kp'], SIDE, SIDE, 2)
        chw = lambda a: np.ascontiguousarray(np.transpose(a, (2, 0, 1)))
        random_mask = np.zeros((SIDE, SIDE, 1), dtype=np.uint8)
        if u['random_mask'] is not None:                      # dataset.py:1223-1241
            random_mask += u['random_mask']
        keep = 1 - chw((random_mask > 0).astype(np.uint8))
        upper_erase, lower_erase = chw(denorm_upper) * keep, chw(denorm_lower) * keep
        rows = lambda b: np.ascontiguousarray(np.broadcast_to(b[None, :, None], (1, SIDE, SIDE)))
        return (chw(u['image']), chw(u['pose']), chw(norm_img), chw(norm_img_lower), chw(for_train), upper_erase, lower_erase, ms, m_invs,
                chw(u['gt_parsing']), (np.sum(upper_erase, axis=0, keepdims=True) > 0).astype(np.uint8),
                (np.sum(lower_erase, axis=0, keepdims=True) > 0).astype(np.uint8), chw(masks), chw(masks_lower), chw(u['retain_mask']),
                chw(TryOnTestSet._skin_map(u['skin'])), np.full((1, SIDE, SIDE), u['label'] / 2.0 * 255), rows(u['bound_train']), rows(u['bound_test']))


_TRAIN_ARRAYS = ('upper_img', 'lower_img', 'upper_mask', 'lower_mask', 'sleeve', 'image', 'pose', 'gt_parsing', 'retain_mask', 'bound_train', 'bound_test')


def collate_train(items, pin=False):
    """Stack ``TrainSet.unrouted`` items into a batch: the uint8 arrays as [N, ...] tensors (pinned with pin=True, as `collate_unrouted`), skin as
    float32 [N, 3] (NaN kept), label int32 [N], random_mask uint8 [N, 512, 512, 1] (zeros for an item without one), the records as `erase` int32
    [N, 4] = (kind, rows, erase_length, use_random_mask) and `band_u` float32 [N]; key points, records and names stay lists."""
    out = {k: torch.from_numpy(np.stack([it[k] for it in items])) for k in _TRAIN_ARRAYS}
    zero = np.zeros((SIDE, SIDE, 1), dtype=np.uint8)
    out['random_mask'] = torch.from_numpy(np.stack([zero if it['random_mask'] is None else it['random_mask'] for it in items]))
    out['skin'] = torch.from_numpy(np.stack([it['skin'] for it in items])).to(torch.float32)
    out['label'] = torch.tensor([it['label'] for it in items], dtype=torch.int32)
    out['erase'] = torch.tensor([[r.kind, r.rows, r.erase_length, r.use_random_mask] for r in (it['record'] for it in items)], dtype=torch.int32)
    out['band_u'] = torch.tensor([it['record'].u for it in items], dtype=torch.float32)
    if pin:
        out = {k: v.pin_memory() for k, v in out.items()}
    for k in ('person_kp', 'record', 'name'):
        out[k] = [it[k] for it in items]
    return out

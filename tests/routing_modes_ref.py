"""Test-side restatement of the lower-garment and full-outfit try-on modes' ``normalize`` (TEST INFRASTRUCTURE ONLY).

Written from the reference's statements -- ``UvitonDatasetFull_512_test_full.normalize`` (training/dataset.py:1796-1923) and
``UvitonDatasetFull_512_test_lower.normalize`` (:3313-3454) -- line by line, with the OpenCV calls replaced by the oracle's
primitives only: ``get_crop``, ``warp_perspective_u8`` and ``erode_u8`` of oracle/patch_routing_ref.py.  It does not import the
product.  Parity with OpenCV itself stays unpinned, as for the upper mode.
"""

import numpy as np

from oracle import patch_routing_ref as R


def _flip(a):                                                 # cv2.flip(a, 1)
    return a[:, ::-1]


def _denorm(canvas, part_img, part_mask, m_inv, o_w, o_h, ksize):
    """The de-normalise-and-paste statements of one part (:1860-1866 / :3379-3385): warp back, erode channel 0, paste where it is 255."""
    patch = R.warp_perspective_u8(part_img, m_inv, (o_w, o_h))
    m = R.warp_perspective_u8(part_mask, m_inv, (o_w, o_h))[..., 0:1]
    m = R.erode_u8(m[..., 0], ksize)[..., np.newaxis]
    m = (m == 255).astype(np.uint8)
    return patch * m + canvas * (1 - m)


def _mirror_sleeves(part_imgs, part_clothes_masks):
    """:1889-1918 (full) = :3419-3449 (lower), as written: the bottom-sleeve branches mirror part_imgs[3] / part_imgs[5] themselves."""
    left_top_sleeve_mask = part_clothes_masks[2]
    right_top_sleeve_mask = part_clothes_masks[4]
    left_bottom_sleeve_mask = part_clothes_masks[3]
    right_bottom_sleeve_mask = part_clothes_masks[5]
    if np.sum(left_top_sleeve_mask) == 0 and np.sum(right_top_sleeve_mask) > 0:
        part_imgs[2] = _flip(part_imgs[4])
        part_clothes_masks[2] = _flip(right_top_sleeve_mask)
    elif np.sum(right_top_sleeve_mask) == 0 and np.sum(left_top_sleeve_mask) > 0:
        part_imgs[4] = _flip(part_imgs[2])
        part_clothes_masks[4] = _flip(left_top_sleeve_mask)
    if np.sum(left_bottom_sleeve_mask) == 0 and np.sum(right_bottom_sleeve_mask) > 0:
        part_imgs[3] = _flip(part_imgs[3])
        part_clothes_masks[3] = _flip(right_bottom_sleeve_mask)
    elif np.sum(right_bottom_sleeve_mask) == 0 and np.sum(left_bottom_sleeve_mask) > 0:
        part_imgs[5] = _flip(part_imgs[5])
        part_clothes_masks[5] = _flip(left_bottom_sleeve_mask)


def normalize(part, upper_img, lower_img, upper_clothes_mask, lower_clothes_mask, sleeve_mask, clothes_keypoints, person_keypoints, box_factor):
    """part = 'full' (dataset.py:1796-1923) or 'lower' (:3313-3454) -> (img, img_lower, denorm_upper_img, denorm_lower_img)."""
    assert part in ('full', 'lower')
    h, w = upper_img.shape[:2]
    o_h, o_w = h, w
    h = h // 2 ** box_factor
    w = w // 2 ** box_factor
    wh = np.expand_dims(np.array([w, h]), 0)

    part_imgs, part_imgs_lower, part_clothes_masks, part_clothes_masks_lower = [], [], [], []
    denorm_upper_img = np.zeros_like(upper_img)
    denorm_lower_img = np.zeros_like(upper_img)
    ksize = 5                                                 # kernel = np.ones((5,5)) (:1827, :3345)

    for ii, bpart in enumerate(R.BPARTS):
        ar = 0.5 if ii < 6 else 0.4
        part_img = np.zeros((h, w, 3)).astype(np.uint8)
        part_img_lower = np.zeros((h, w, 3)).astype(np.uint8)
        part_clothes_mask = np.zeros((h, w, 3)).astype(np.uint8)
        part_clothes_mask_lower = np.zeros((h, w, 3)).astype(np.uint8)

        clothes_M, _ = R.get_crop(clothes_keypoints, bpart, wh, o_w, o_h, ar)
        person_M, person_M_inv = R.get_crop(person_keypoints, bpart, wh, o_w, o_h, ar)

        # the upper garment: through the clothes crop in 'full' (:1843-1853), the person crop in 'lower' (:3361-3371)
        upper_M = clothes_M if part == 'full' else person_M
        if upper_M is not None:
            if ii == 2 or ii == 3 or ii == 4 or ii == 5:
                if sleeve_mask is not None:
                    part_img = R.warp_perspective_u8(upper_img * sleeve_mask, upper_M, (w, h))
                    part_clothes_mask = R.warp_perspective_u8(upper_clothes_mask * sleeve_mask, upper_M, (w, h))
                else:
                    part_img = R.warp_perspective_u8(upper_img, upper_M, (w, h))
                    part_clothes_mask = R.warp_perspective_u8(upper_clothes_mask, upper_M, (w, h))
            else:
                if sleeve_mask is not None:
                    part_img = R.warp_perspective_u8(upper_img * (1 - sleeve_mask), upper_M, (w, h))
                    part_clothes_mask = R.warp_perspective_u8(upper_clothes_mask * (1 - sleeve_mask), upper_M, (w, h))
                else:
                    part_img = R.warp_perspective_u8(upper_img, upper_M, (w, h))
                    part_clothes_mask = R.warp_perspective_u8(upper_clothes_mask, upper_M, (w, h))
            if person_M_inv is not None:
                denorm_upper_img = _denorm(denorm_upper_img, part_img, part_clothes_mask, person_M_inv, o_w, o_h, ksize)

        # the lower garment: through the clothes crop in both modes (:1868-1881, :3387-3398)
        if ii == 0 or ii >= 6:
            if clothes_M is not None:
                part_img_lower = R.warp_perspective_u8(lower_img, clothes_M, (w, h))
                part_clothes_mask_lower = R.warp_perspective_u8(lower_clothes_mask, clothes_M, (w, h))
                if person_M_inv is not None:
                    denorm_lower_img = _denorm(denorm_lower_img, part_img_lower, part_clothes_mask_lower, person_M_inv, o_w, o_h, ksize)

        part_imgs.append(part_img)
        part_clothes_masks.append(part_clothes_mask)
        if ii == 0 or ii >= 6:
            part_imgs_lower.append(part_img_lower)
            part_clothes_masks_lower.append(part_clothes_mask_lower)

    if part == 'lower':                                       # :3408-3417 (the full mode has no such step)
        upper_torso_mask = (np.sum(part_clothes_masks[0], axis=2, keepdims=True) > 0).astype(np.uint8)
        upper_left_hip_mask = (np.sum(part_clothes_masks[6], axis=2, keepdims=True) > 0).astype(np.uint8)
        upper_right_hip_mask = (np.sum(part_clothes_masks[8], axis=2, keepdims=True) > 0).astype(np.uint8)
        part_imgs_lower[0] = part_imgs_lower[0] * (1 - upper_torso_mask)
        part_imgs_lower[1] = part_imgs_lower[1] * (1 - upper_left_hip_mask)
        part_imgs_lower[3] = part_imgs_lower[3] * (1 - upper_right_hip_mask)
        part_clothes_masks_lower[0] = part_clothes_masks_lower[0] * (1 - upper_torso_mask)
        part_clothes_masks_lower[1] = part_clothes_masks_lower[1] * (1 - upper_left_hip_mask)
        part_clothes_masks_lower[3] = part_clothes_masks_lower[3] * (1 - upper_right_hip_mask)

    _mirror_sleeves(part_imgs, part_clothes_masks)

    img = np.concatenate(part_imgs, axis=2)
    img_lower = np.concatenate(part_imgs_lower, axis=2)
    return img, img_lower, denorm_upper_img, denorm_lower_img

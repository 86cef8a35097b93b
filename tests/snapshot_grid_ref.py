"""Test-side restatement of the training loop's image snapshots (TEST INFRASTRUCTURE ONLY).

Written from the reference's statements -- ``denorm_clothes`` (training/training_loop_fullbody.py:77-212), ``setup_snapshot_image_grid`` (:214-309),
``save_image_grid`` (:313-340) and the snapshot step (:501-519, :700-719) -- line by line, with the OpenCV calls replaced by the oracle's primitives
only (``warp_perspective_u8``, ``erode_u8`` of oracle/patch_routing_ref.py).  `gnum`, 14 in the reference, is an argument, and `cells` picks which
cells are computed (the NumPy warps take seconds per cell).  It does not import the product.  Parity with OpenCV's own rasterising stays unpinned, as
for every other mode (DESIGN.md sections 6d, 6h).

The reference runs the float conversions on a GPU, where torch computes ``u / 127.5`` as ``u * (1.0f / 127.5f)``; `unit` writes that product out in
float32, as the package's other restatements do (training/train_fetch.py)."""

import numpy as np

from oracle import patch_routing_ref as R

_INV = np.float32(1.0) / np.float32(127.5)


def unit(a):
    return np.asarray(a).astype(np.float32) * _INV - np.float32(1)


def mask_to_bbox(mask):                                       # :66-75
    mask[mask >= 0.5] = 1
    mask[mask < 0.5] = 0
    site = np.where(mask > 0)
    if len(site[0]) > 0 and len(site[1]) > 0:
        return [np.min(site[1]), np.min(site[0]), np.max(site[1]), np.max(site[0])]
    return None


def _warp(img, m, size):
    return R.warp_perspective_u8(np.ascontiguousarray(img), m, size)


def denorm_clothes(norm_patches, norm_patches_lower, norm_clothes_mask, norm_clothes_mask_lower, gt_parsings, lower_label_maps,
                   lower_clothes_upper_bounds_for_test, Ms, M_invs, col, row, gnum):                       # :77-212
    denorm_upper_img = np.zeros((512, 512, 3), dtype=np.uint8)
    denorm_lower_img = np.zeros((512, 512, 3), dtype=np.uint8)
    ksize = 8
    upper_norm_patch_list = []
    lower_norm_patch_list = []
    gap = gnum // 3
    for ii in range(M_invs.shape[1]):
        if row < gap:
            norm_patch = norm_patches[row, ii * 3:(ii + 1) * 3, ...].transpose(1, 2, 0)
            norm_clothes_mask_patch = norm_clothes_mask[row, ii * 3:(ii + 1) * 3, ...].transpose(1, 2, 0)
        else:
            norm_patch = norm_patches[col, ii * 3:(ii + 1) * 3, ...].transpose(1, 2, 0)
            norm_clothes_mask_patch = norm_clothes_mask[col, ii * 3:(ii + 1) * 3, ...].transpose(1, 2, 0)
        if ii == 0:
            who = col if row < 2 * gap else row
            norm_patch_lower = norm_patches_lower[who, ii * 3:(ii + 1) * 3, ...].transpose(1, 2, 0)
            norm_clothes_mask_patch_lower = norm_clothes_mask_lower[who, ii * 3:(ii + 1) * 3, ...].transpose(1, 2, 0)
        if ii >= 6:
            who = col if row < 2 * gap else row
            norm_patch_lower = norm_patches_lower[who, (ii - 6 + 1) * 3:(ii - 6 + 2) * 3, ...].transpose(1, 2, 0)
            norm_clothes_mask_patch_lower = norm_clothes_mask_lower[who, (ii - 6 + 1) * 3:(ii - 6 + 2) * 3, ...].transpose(1, 2, 0)

        M = Ms[row, ii]
        M_inv = M_invs[row, ii]
        if M_inv.sum() == 0:
            upper_norm_patch_list.append(np.zeros_like(norm_patch))
            if ii == 0 or ii >= 6:
                lower_norm_patch_list.append(np.zeros_like(norm_patch_lower))
            continue

        denorm_patch = _warp(norm_patch, M_inv, (512, 512))
        denorm_clothes_mask_patch = _warp(norm_clothes_mask_patch, M_inv, (512, 512))
        denorm_clothes_mask_patch = R.erode_u8(denorm_clothes_mask_patch, ksize)[..., 0:1]
        denorm_clothes_mask_patch = (denorm_clothes_mask_patch == 255).astype(np.uint8)
        denorm_upper_img = denorm_patch * denorm_clothes_mask_patch + denorm_upper_img * (1 - denorm_clothes_mask_patch)

        if ii == 0 or ii >= 6:
            denorm_patch_lower = _warp(norm_patch_lower, M_inv, (512, 512))
            denorm_clothes_mask_patch_lower = _warp(norm_clothes_mask_patch_lower, M_inv, (512, 512))
            denorm_clothes_mask_patch_lower = R.erode_u8(denorm_clothes_mask_patch_lower, ksize)[..., 0:1]
            denorm_clothes_mask_patch_lower = (denorm_clothes_mask_patch_lower == 255).astype(np.uint8)
            denorm_lower_img = denorm_patch_lower * denorm_clothes_mask_patch_lower + denorm_lower_img * (1 - denorm_clothes_mask_patch_lower)

        upper_norm_patch_list.append(norm_patch)
        if ii == 0 or ii >= 6:
            norm_clothes_mask_patch_tmp = norm_clothes_mask_patch[..., 0:1]
            norm_clothes_mask_patch_tmp = (norm_clothes_mask_patch_tmp > 0).astype(np.uint8)
            norm_patch_lower_tmp = norm_patch_lower * (1 - norm_clothes_mask_patch_tmp)
            denorm_patch_tmp = _warp(norm_patch_lower_tmp, M_inv, (512, 512))
            norm_patch_lower_tmp = _warp(denorm_patch_tmp, M, (128, 128))
            lower_norm_patch_list.append(norm_patch_lower_tmp)

    denorm_upper_img = denorm_upper_img.transpose(2, 0, 1)[np.newaxis, ...]
    denorm_lower_img = denorm_lower_img.transpose(2, 0, 1)[np.newaxis, ...]
    denorm_upper_clothes_mask = (np.sum(denorm_upper_img, axis=1, keepdims=True) > 0).astype(np.uint8)
    denorm_lower_clothes_mask = (np.sum(denorm_lower_img, axis=1, keepdims=True) > 0).astype(np.uint8)

    upper_norm_patches = np.concatenate(upper_norm_patch_list, axis=2)
    lower_norm_patches = np.concatenate(lower_norm_patch_list, axis=2)
    upper_lower_norm_patches = np.concatenate([upper_norm_patches, lower_norm_patches], axis=2)
    upper_lower_norm_patches = upper_lower_norm_patches.transpose(2, 0, 1)[np.newaxis, ...]

    if row < gap:
        gt_parsing = gt_parsings[row].transpose(1, 2, 0)
        lower_mask = (gt_parsing == 2).astype(np.uint8) + (gt_parsing == 3).astype(np.uint8)
        lower_clothes_upper_bound = np.zeros_like(gt_parsing)
        bbox = mask_to_bbox(lower_mask.copy())
        if bbox is not None:
            lower_clothes_upper_bound[bbox[1]:, ...] += 255
    elif row < 2 * gap:
        denorm_lower_img_tmp = np.zeros((512, 512, 3), dtype=np.uint8)
        for k, ii in ((0, 0), (1, 6), (3, 8)):
            if np.sum(M_invs[row, ii]) != 0:
                denorm_lower_img_tmp += _warp(lower_norm_patch_list[k], M_invs[row, ii], (512, 512))       # uint8: wraps around
        denorm_lower_mask_tmp = (np.sum(denorm_lower_img_tmp, axis=2, keepdims=True) > 0).astype(np.uint8)
        lower_clothes_upper_bound = np.zeros((512, 512, 1))
        bbox = mask_to_bbox(denorm_lower_mask_tmp.copy())
        if bbox is not None:
            lower_clothes_upper_bound[bbox[1]:, ...] += 255
    else:
        lower_clothes_upper_bound = lower_clothes_upper_bounds_for_test[row].transpose(1, 2, 0).copy()
        denorm_patch_torso = _warp(upper_norm_patch_list[0], M_invs[row, 0], (512, 512))
        denorm_patch_torso_mask = (np.sum(denorm_patch_torso, axis=2, keepdims=True) > 0).astype(np.uint8)
        bbox = mask_to_bbox(denorm_patch_torso_mask)
        if bbox is not None:
            lower_clothes_upper_bound[0:bbox[3], ...] *= 0

    if row < 2 * gap:
        lower_label_map = lower_label_maps[col].transpose(1, 2, 0)
    else:
        lower_label_map = lower_label_maps[row].transpose(1, 2, 0)
    lower_clothes_conditions = np.concatenate([lower_label_map, lower_clothes_upper_bound], axis=2)
    lower_clothes_conditions = lower_clothes_conditions.transpose(2, 0, 1)[np.newaxis, ...]
    return (denorm_upper_img, denorm_lower_img, denorm_upper_clothes_mask, denorm_lower_clothes_mask, upper_lower_norm_patches,
            lower_clothes_conditions)


def setup_snapshot_image_grid(training_set, gnum, cells):                                                 # :214-309
    """-> {cell: dict of the uint8 / float64 arrays of `denorm_clothes` and the seven float32 generator inputs of that cell}."""
    grid_indices = training_set.vis_index[:gnum]
    (images, poses, norm_img, norm_img_lower, _, _, _, Ms, M_invs, gt_parsings, _, _, norm_clothes_mask, norm_clothes_mask_lower, retain_masks, skins,
     lower_label_map, _, bounds_for_test) = (np.array(a) for a in zip(*[training_set[i] for i in grid_indices]))
    out = {}
    for i in cells:
        col, row = i % gnum, i // gnum
        up, lo, up_mask, lo_mask, parts, conditions = denorm_clothes(norm_img, norm_img_lower, norm_clothes_mask, norm_clothes_mask_lower, gt_parsings,
                                                                     lower_label_map, bounds_for_test, Ms, M_invs, col, row, gnum)
        image = unit(images[row])
        retain_mask = retain_masks[row].astype(np.float32)
        retain = np.concatenate([retain_mask * image - (1 - retain_mask), unit(skins[row])], axis=0)
        out[i] = dict(denorm_upper=up[0], denorm_lower=lo[0], upper_mask=up_mask[0], lower_mask=lo_mask[0], parts=parts[0], conditions=conditions[0],
                      inputs=dict(c=unit(parts), retain=retain[None], pose=np.concatenate([unit(poses[row]), unit(conditions[0])], axis=0)[None],
                                  denorm_upper_input=unit(up), denorm_lower_input=unit(lo), denorm_upper_mask=up_mask.astype(np.float32),
                                  denorm_lower_mask=lo_mask.astype(np.float32)))
    return out


def save_image_grid(im_side, im_top, img, drange, grid_size):                                             # :313-334, returning the array it saves
    lo, hi = drange
    img = np.asarray(img, dtype=np.float32)
    img = (img - lo) * (255 / (hi - lo))
    img = np.rint(img).clip(0, 255).astype(np.uint8)

    im_side = np.asarray(im_side, dtype=np.float32)
    im_side = (im_side - lo) * (255 / (hi - lo))
    im_side = np.rint(im_side).clip(0, 255).astype(np.uint8)

    im_top = np.asarray(im_top, dtype=np.float32)
    im_top = (im_top - lo) * (255 / (hi - lo))
    im_top = np.rint(im_top).clip(0, 255).astype(np.uint8)

    gw, gh = grid_size
    _N, C, H, W = img.shape
    img = np.reshape(img, (gh, gw, C, H, W))
    img = img.transpose(0, 3, 1, 4, 2)
    img = img.reshape(gh * H, gw * W, C)
    img = np.concatenate((im_side, img), axis=1)
    img = np.concatenate((im_top, img), axis=0)
    return img


def side_and_top(images, gnum):                                                                           # :501-505; images float32 [gnum, C, H, W]
    _N, C, H, W = images.shape
    source_im = images[:gnum]
    image_side = source_im[:, None].transpose(0, 3, 1, 4, 2).reshape(gnum * H, 1 * W, C)
    image_top = np.concatenate((np.zeros(images[0].shape, dtype=np.float32)[None], source_im), axis=0)
    image_top = image_top[None].transpose(0, 3, 1, 4, 2).reshape(1 * H, (gnum + 1) * W, C)
    return image_side, image_top


def parsing_values(pred_parsing):                                                                         # :709-717; float32 [n, C, H, W] -> [n, 3, H, W]
    x = np.asarray(pred_parsing, dtype=np.float32)
    e = np.exp(x - x.max(axis=1, keepdims=True))
    softmax = e / e.sum(axis=1, keepdims=True)
    parsing_index = np.argmax(softmax, axis=1)[:, None, ...].astype(np.float32)
    parsing_index = np.concatenate([parsing_index, parsing_index, parsing_index], axis=1)
    return parsing_index / 6 * 2 - 1.0

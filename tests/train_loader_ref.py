"""Test-side restatement of the training loader's ``normalize`` and the tail of its ``__getitem__`` (TEST INFRASTRUCTURE ONLY).

Written from the reference's statements -- ``UvitonDatasetFull_512.normalize`` (training/dataset.py:1010-1195) and ``__getitem__`` (:1223-1241) --
line by line, with the OpenCV calls replaced by the oracle's primitives only (``get_crop``, ``warp_perspective_u8``, ``erode_u8`` of
oracle/patch_routing_ref.py; the training class's ``get_crop``, :828-997, is the statements the oracle restates).  The reference draws its random
decisions from ``random`` inside these statements; here they arrive as an argument -- `record` = (kind, rows, erase_length, u, use_random_mask) with
kind 0 none / 1 drop part 0 / 2 band -- so that the product's device-side application of the same record can be compared pixel for pixel.  It does
not import the product.  Parity with OpenCV itself stays unpinned, as for the other modes."""

import numpy as np

from oracle import patch_routing_ref as R


def mask_to_bbox(mask):                                       # :999-1008
    mask = mask.copy()
    site = np.where(mask >= 0.5)
    if len(site[0]) > 0 and len(site[1]) > 0:
        return [np.min(site[1]), np.min(site[0]), np.max(site[1]), np.max(site[0])]
    return None


def normalize(upper_img, lower_img, upper_clothes_mask, lower_clothes_mask, sleeve_mask, keypoints, box_factor, record):
    """-> (img, img_lower, img_lower_for_train, denorm_upper_img, denorm_lower_img, Ms, M_invs, clothes_masks, clothes_masks_lower)"""
    h, w = upper_img.shape[:2]
    o_h, o_w = h, w
    h = h // 2 ** box_factor
    w = w // 2 ** box_factor
    wh = np.expand_dims(np.array([w, h]), 0)

    part_imgs, part_imgs_lower, part_imgs_lower_for_train, part_clothes_masks, part_clothes_masks_lower, M_invs, Ms = [], [], [], [], [], [], []
    denorm_upper_img = np.zeros_like(upper_img)
    denorm_lower_img = np.zeros_like(upper_img)
    ksize = 5

    def paste(canvas, part_img, part_mask, M_inv):
        patch = R.warp_perspective_u8(part_img, M_inv, (o_w, o_h))
        m = R.warp_perspective_u8(part_mask, M_inv, (o_w, o_h))[..., 0:1]
        m = R.erode_u8(m[..., 0], ksize)[..., np.newaxis]
        m = (m == 255).astype(np.uint8)
        return patch * m + canvas * (1 - m)

    for ii, bpart in enumerate(R.BPARTS):
        ar = 0.5 if ii < 6 else 0.4
        part_img = np.zeros((h, w, 3)).astype(np.uint8)
        part_img_lower = np.zeros((h, w, 3)).astype(np.uint8)
        part_clothes_mask = np.zeros((h, w, 3)).astype(np.uint8)
        part_clothes_mask_lower = np.zeros((h, w, 3)).astype(np.uint8)
        M, M_inv = R.get_crop(keypoints, bpart, wh, o_w, o_h, ar)
        if M is not None:
            if ii in (2, 3, 4, 5):
                part_img = R.warp_perspective_u8(upper_img * sleeve_mask, M, (w, h))
                part_clothes_mask = R.warp_perspective_u8(upper_clothes_mask * sleeve_mask, M, (w, h))
            else:
                part_img = R.warp_perspective_u8(upper_img * (1 - sleeve_mask), M, (w, h))
                part_clothes_mask = R.warp_perspective_u8(upper_clothes_mask * (1 - sleeve_mask), M, (w, h))
            denorm_upper_img = paste(denorm_upper_img, part_img, part_clothes_mask, M_inv)
            if ii == 0 or ii >= 6:
                part_img_lower = R.warp_perspective_u8(lower_img, M, (w, h))
                part_clothes_mask_lower = R.warp_perspective_u8(lower_clothes_mask, M, (w, h))
                denorm_lower_img = paste(denorm_lower_img, part_img_lower, part_clothes_mask_lower, M_inv)
            Ms.append(M[np.newaxis, ...])
            M_invs.append(M_inv[np.newaxis, ...])
        else:
            Ms.append(np.zeros((1, 3, 3), dtype=np.float32))
            M_invs.append(np.zeros((1, 3, 3), dtype=np.float32))
        part_imgs.append(part_img)
        part_clothes_masks.append(part_clothes_mask)
        if ii == 0 or ii >= 6:
            part_imgs_lower.append(part_img_lower)
            part_imgs_lower_for_train.append(part_img_lower.copy())
            part_clothes_masks_lower.append(part_clothes_mask_lower)

    flip = lambda a: a[:, ::-1]                                # cv2.flip(a, 1)
    left_top_sleeve_mask, right_top_sleeve_mask = part_clothes_masks[2], part_clothes_masks[4]
    left_bottom_sleeve_mask, right_bottom_sleeve_mask = part_clothes_masks[3], part_clothes_masks[5]
    if np.sum(left_top_sleeve_mask) == 0 and np.sum(right_top_sleeve_mask) > 0:
        part_imgs[2] = flip(part_imgs[4])
        part_clothes_masks[2] = flip(right_top_sleeve_mask)
    elif np.sum(right_top_sleeve_mask) == 0 and np.sum(left_top_sleeve_mask) > 0:
        part_imgs[4] = flip(part_imgs[2])
        part_clothes_masks[4] = flip(left_top_sleeve_mask)
    if np.sum(left_bottom_sleeve_mask) == 0 and np.sum(right_bottom_sleeve_mask) > 0:
        part_imgs[3] = flip(part_imgs[3])                     # as written (:1119-1122): part 3's own image
        part_clothes_masks[3] = flip(right_bottom_sleeve_mask)
    elif np.sum(right_bottom_sleeve_mask) == 0 and np.sum(left_bottom_sleeve_mask) > 0:
        part_imgs[5] = flip(part_imgs[5])
        part_clothes_masks[5] = flip(left_bottom_sleeve_mask)

    kind, rows, erase_length, u, _ = record
    bbox_lower = mask_to_bbox(part_clothes_masks_lower[0][..., 0:1])
    if bbox_lower is not None:                                # :1148-1170, the draws replaced by the record
        if kind == 1:
            part_imgs_lower_for_train[0] = np.zeros((h, w, 3)).astype(np.uint8)
            if rows:
                part_imgs_lower_for_train[1][0:erase_length, ...] *= 0
                part_imgs_lower_for_train[3][0:erase_length, ...] *= 0
        elif kind == 2:
            ty = bbox_lower[1]
            by = min(ty + 1 + int(np.floor(np.float32(u) * np.float32(h - ty))), h)      # randint(ty + 1, h) from the record's u
            part_imgs_lower_for_train[0][ty:by, ...] *= 0

    cat = lambda parts: np.concatenate(parts, axis=2)
    return (cat(part_imgs), cat(part_imgs_lower), cat(part_imgs_lower_for_train), denorm_upper_img, denorm_lower_img, np.concatenate(Ms, axis=0),
            np.concatenate(M_invs, axis=0), cat(part_clothes_masks), cat(part_clothes_masks_lower))


def getitem_tail(denorm_upper_img, denorm_lower_img, random_mask, record):
    """:1223-1241 on CHW canvases; random_mask [512, 512, 1] is the file's channel 0."""
    denorm_random_mask = np.zeros((512, 512, 1), dtype=np.uint8)
    denorm_random_mask_bottom = np.zeros((512, 512, 1), dtype=np.uint8)
    if record[4]:
        denorm_random_mask += random_mask
        denorm_random_mask_bottom += random_mask
    denorm_random_mask = (denorm_random_mask > 0).astype(np.uint8).transpose(2, 0, 1)
    denorm_random_mask_bottom = (denorm_random_mask_bottom > 0).astype(np.uint8).transpose(2, 0, 1)
    denorm_upper_img_erase = denorm_upper_img * (1 - denorm_random_mask)
    denorm_upper_mask = (np.sum(denorm_upper_img_erase, axis=0, keepdims=True) > 0).astype(np.uint8)
    denorm_lower_img_erase = denorm_lower_img * (1 - denorm_random_mask_bottom)
    denorm_lower_mask = (np.sum(denorm_lower_img_erase, axis=0, keepdims=True) > 0).astype(np.uint8)
    return denorm_upper_img_erase, denorm_lower_img_erase, denorm_upper_mask, denorm_lower_mask

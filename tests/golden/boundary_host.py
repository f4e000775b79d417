"""The host statement of cp_boundary_overlaps (include/centerpoly_hip.h) in numpy, written the literal way of the
published Boundary IoU code: surround the mask with one ring of zeros, take d successive 3 x 3 minima, cut the ring
off, subtract -- one value at a time for the id image.  Deliberately NOT the separable form the kernel uses."""
import numpy as np


def erode3(padded):
    """One 3 x 3 minimum of a 0 / 1 array; beyond the array nothing erodes (the ring of zeros is inside it)."""
    p = np.pad(padded, 1, constant_values=1)
    out = p[1:-1, 1:-1].copy()
    for dy in (0, 1, 2):
        for dx in (0, 1, 2):
            np.minimum(out, p[dy:dy + padded.shape[0], dx:dx + padded.shape[1]], out=out)
    return out


def band(mask, d):
    """band(M, d) of a boolean [H, W] array as a boolean array."""
    m = np.asarray(mask).astype(np.uint8)
    e = np.pad(m, 1, constant_values=0)
    for _ in range(int(d)):
        e = erode3(e)
    return (m - e[1:-1, 1:-1]).astype(bool)


def band_of_crop(mask, d):
    """band(mask, d) computed on the set's bounding box grown by one pixel and clipped to the image -- the same literal
    steps on fewer pixels.  Where the crop's edge lies inside the image its outermost line holds no pixel of the set, so
    the ring of zeros beyond it changes nothing; where it is the image's edge the ring is the image's own."""
    m = np.asarray(mask).astype(bool)
    out = np.zeros(m.shape, bool)
    ys, xs = np.flatnonzero(m.any(1)), np.flatnonzero(m.any(0))
    if len(ys):
        y0, y1, x0, x1 = max(ys[0] - 1, 0), ys[-1] + 2, max(xs[0] - 1, 0), xs[-1] + 2
        out[y0:y1, x0:x1] = band(m[y0:y1, x0:x1], d)
    return out


def band_brute(mask, d):
    """The set definition, pixel by pixel: p in M with a q within Chebyshev distance d outside the image or not in M."""
    m = np.asarray(mask).astype(bool)
    H, W = m.shape
    out = np.zeros((H, W), bool)
    for y in range(H):
        for x in range(W):
            if not m[y, x]:
                continue
            for qy in range(y - d, y + d + 1):
                for qx in range(x - d, x + d + 1):
                    if qy < 0 or qy >= H or qx < 0 or qx >= W or not m[qy, qx]:
                        out[y, x] = True
    return out


def clipped(masks, bounds):
    """The masks as sets: non-zero pixels inside the bounds clipped to the image (None: everywhere)."""
    m = np.asarray(masks) != 0
    if bounds is None:
        return m
    n, H, W = m.shape
    out = np.zeros_like(m)
    for i, (x0, y0, x1, y1) in enumerate(np.asarray(bounds).reshape(n, 4)):
        x0, y0, x1, y1 = max(int(x0), 0), max(int(y0), 0), min(int(x1), W - 1), min(int(y1), H - 1)
        if x0 <= x1 and y0 <= y1:
            out[i, y0:y1 + 1, x0:x1 + 1] = m[i, y0:y1 + 1, x0:x1 + 1]
    return out


def gt_band(gt_ids, d):
    """The band image of an id image: the union of band({ids == v}, d) over every value v of the image."""
    ids = np.asarray(gt_ids)
    out = np.zeros(ids.shape, bool)
    for v in np.unique(ids):
        out |= band(ids == v, d)
    return out


def boundary_counts(masks, gt_ids, inst_ids, d, bounds=None):
    """(b_inter int64 [n, G], b_pred [n], b_gt [G], pred_bands uint8 [n, H, W], gt_band uint8 [H, W]) of
    cp_boundary_overlaps."""
    ids = np.asarray(gt_ids)
    sets = clipped(masks, bounds)
    n, G = len(sets), len(inst_ids)
    gband = gt_band(ids, d)
    pbands = np.zeros(sets.shape, bool)
    for i in range(n):
        pbands[i] = band(sets[i], d)
    b_inter, b_gt = np.zeros((n, G), np.int64), np.zeros((G,), np.int64)
    for j, v in enumerate(inst_ids):
        sel = gband & (ids == v) if 0 <= int(v) < 65536 else np.zeros(ids.shape, bool)
        b_gt[j] = sel.sum()
        for i in range(n):
            b_inter[i, j] = (pbands[i] & sel).sum()
    return b_inter, pbands.sum(axis=(1, 2)).astype(np.int64), b_gt, pbands.astype(np.uint8) * 255, \
        gband.astype(np.uint8) * 255


def boundary_tables(masks, gt_ids, inst_ids, d, bounds=None):
    """(b_inter, b_pred, b_gt) alone, for full-size images: every band through band_of_crop, and ground-truth bands of
    the values of interest only (the band of a value depends on no other value's set)."""
    ids = np.asarray(gt_ids)
    sets = clipped(masks, bounds)
    n, G = len(sets), len(inst_ids)
    pbands = [band_of_crop(sets[i], d) for i in range(n)]
    b_inter, b_gt = np.zeros((n, G), np.int64), np.zeros((G,), np.int64)
    for j, v in enumerate(inst_ids):
        if not 0 <= int(v) < 65536:
            continue
        sel = band_of_crop(ids == v, d)
        b_gt[j] = sel.sum()
        for i in range(n):
            b_inter[i, j] = (pbands[i] & sel).sum()
    return b_inter, np.array([p.sum() for p in pbands], np.int64).reshape(n), b_gt

"""Host restatement (numpy) of cp_panoptic_pairs and cp_panoptic_match, written from their definitions in
include/centerpoly_hip.h: the tests compare the device tables with these."""
import numpy as np

MAX_ROWS = 1024


def panoptic_pairs(index, n, gt_ids, id_divisor, id_direct_below, L, label_flags):
    """(seg int64 [R, 4], pairs int64 [R, n + 1]) with R = min(G, 1024) + 1: the rows the device call writes."""
    index = np.asarray(index, np.int64).reshape(-1)
    v = np.asarray(gt_ids, np.int64).reshape(-1)
    flags = np.asarray(label_flags, np.int64)
    g = np.where(v < id_direct_below, v, v // id_divisor)
    void = (g >= L) | ((flags[np.minimum(g, L - 1)] & 1) == 0)
    values = np.unique(v[~void])
    G = len(values)
    kept = values[:MAX_ROWS]
    row = np.zeros(v.shape, np.int64)
    inside = ~void & np.isin(v, kept)
    row[inside] = np.searchsorted(kept, v[inside]) + 1
    counted = void | inside                                   # pixels of a segment past the 1024th count nowhere
    col = np.where(index < n, index, n)
    R = len(kept) + 1
    pairs = np.bincount(row[counted] * (n + 1) + col[counted], minlength=R * (n + 1)).reshape(R, n + 1)
    seg = np.zeros((R, 4), np.int64)
    seg[0] = [G, pairs[0].sum(), 0, 0]
    for r, value in enumerate(kept, 1):
        lab = value if value < id_direct_below else value // id_divisor
        seg[r] = [value, lab, int(value < id_direct_below and (flags[lab] & 2) != 0), pairs[r].sum()]
    return seg, pairs


def panoptic_match(seg, pairs, n, pred_label, L, label_flags, stat=None, iou=None, bad=None):
    """(stat int64 [L, 3], iou float64 [L], bad int64 [2], match int64 [n]): the run-long tables after this image
    (given ones are copied and added to) and the image's match row."""
    seg, pairs = np.asarray(seg, np.int64), np.asarray(pairs, np.int64)
    flags = np.asarray(label_flags, np.int64)
    stat = np.zeros((L, 3), np.int64) if stat is None else np.array(stat, np.int64)
    iou = np.zeros((L,), np.float64) if iou is None else np.array(iou, np.float64)
    bad = np.zeros((2,), np.int64) if bad is None else np.array(bad, np.int64)
    match = np.full((n,), -1, np.int64)
    G = int(seg[0, 0])
    if G > MAX_ROWS:
        bad[0] += 1
        return stat, iou, bad, match
    area_p = pairs[:, :n].sum(0)
    exists = np.zeros((n,), bool)
    for i in range(n):
        lab = int(pred_label[i])
        ok = 0 <= lab < L and bool(flags[lab] & 1)
        if area_p[i] > 0 and not ok:
            bad[1] += 1
        exists[i] = area_p[i] > 0 and ok
    match[exists] = 0
    crowd_row = {}
    for r in range(1, G + 1):
        value, lab, crowd, area_g = (int(x) for x in seg[r])
        if crowd:
            crowd_row[lab] = r                                 # ascending values: the highest stays
            continue
        found = False
        for i in np.flatnonzero(pairs[r, :n]):
            if not exists[i] or int(pred_label[i]) != lab:
                continue
            inter = int(pairs[r, i])
            union = area_g + int(area_p[i]) - inter - int(pairs[0, i])
            if 2 * inter > union:
                stat[lab, 0] += 1
                iou[lab] += float(inter) / float(union)
                match[i] = r
                found = True
        if not found:
            stat[lab, 2] += 1
    for i in range(n):
        if exists[i] and match[i] == 0:
            lab = int(pred_label[i])
            x = int(pairs[0, i]) + (int(pairs[crowd_row[lab], i]) if lab in crowd_row else 0)
            if not 2 * x > int(area_p[i]):
                stat[lab, 1] += 1
    return stat, iou, bad, match

"""cp_pixel_confusion restated in numpy, from the definitions of include/centerpoly_hip.h (section "pixel-level
evaluation") and nothing else: what the kernel is compared with, exactly."""
import numpy as np


def pixel_confusion(pred, pred_label, gt_ids, id_divisor, id_direct_below, L, label_group, inst_ids):
    """pred uint8 [H, W], pred_label uint8 [256], gt_ids uint16 [H, W], label_group int8 [L], inst_ids int [G].
    Returns (conf int64 [L, L], inst int64 [G, 3], bad int64 [2]) of this image alone."""
    pred = np.asarray(pred, np.uint8).reshape(-1)
    v = np.asarray(gt_ids, np.uint16).reshape(-1).astype(np.int64)
    assert pred.shape == v.shape
    group = np.asarray(label_group, np.int64)
    g = np.where(v < id_direct_below, v, v // id_divisor)
    p = np.asarray(pred_label, np.uint8).astype(np.int64)[pred]
    bad_g = g >= L
    bad_p = ~bad_g & (p >= L)
    good = ~bad_g & ~bad_p
    conf = np.bincount(g[good] * L + p[good], minlength=L * L).reshape(L, L).astype(np.int64)
    inst = np.zeros((len(inst_ids), 3), np.int64)
    for j, inst_id in enumerate(inst_ids):
        inst_id = int(inst_id)
        mine = v == inst_id
        inst[j, 0] = mine.sum()
        gl = inst_id if inst_id < id_direct_below else inst_id // id_divisor
        if not 0 <= inst_id < 65536 or gl >= L:
            continue
        ok = mine & (p < L)
        inst[j, 1] = (ok & (p == gl)).sum()
        if group[gl] >= 0:
            inst[j, 2] = (ok & (group[np.minimum(p, L - 1)] == group[gl])).sum()
    return conf, inst, np.array([bad_g.sum(), bad_p.sum()], np.int64)

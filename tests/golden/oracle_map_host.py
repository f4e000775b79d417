"""Host restatement (numpy) of the closed form cp_oracle_map computes (include/centerpoly_hip.h): no flood fill, one
distance table per image.  The fixture oracle_map.npz, recorded from the reference's own breadth-first fill, pins it."""
import numpy as np


def gen_oracle_map_host(feat, ind, w, h):
    """feat [B, M, D] float32, ind [B, M] int64 -> [B, D, h, w] float32."""
    feat, ind = np.asarray(feat, np.float32), np.asarray(ind, np.int64)
    B, M, D = feat.shape
    out = np.zeros((B, D, h, w), np.float32)
    ys, xs = np.mgrid[0:h, 0:w]
    for b in range(B):
        js = np.nonzero((ind[b] > 0) & (ind[b] < h * w))[0]          # seeds, in j order
        if js.size == 0:
            continue
        sx, sy = ind[b, js] % w, ind[b, js] // w
        d = np.abs(xs[None] - sx[:, None, None]) + np.abs(ys[None] - sy[:, None, None])     # [n, h, w]
        k = d.argmin(axis=0)                                          # the first minimum: the lowest j
        zero = d == 0
        last = js.size - 1 - zero[::-1].argmax(axis=0)                # at a seed's own pixel: the highest j
        k = np.where(zero.any(axis=0), last, k)
        out[b] = feat[b, js[k]].transpose(2, 0, 1)
    return out


def tie_counts(ind, w, h):
    """Per image of ind [B, M]: how many pixels have 1, 2, 3, 4+ seeds at the minimal L1 distance."""
    ind = np.asarray(ind, np.int64)
    ys, xs = np.mgrid[0:h, 0:w]
    res = []
    for b in range(ind.shape[0]):
        js = np.nonzero((ind[b] > 0) & (ind[b] < h * w))[0]
        if js.size == 0:
            res.append([0, 0, 0, 0])
            continue
        sx, sy = ind[b, js] % w, ind[b, js] // w
        d = np.abs(xs[None] - sx[:, None, None]) + np.abs(ys[None] - sy[:, None, None])
        n = (d == d.min(axis=0)[None]).sum(axis=0)
        res.append([int((n == 1).sum()), int((n == 2).sum()), int((n == 3).sum()), int((n >= 4).sum())])
    return res

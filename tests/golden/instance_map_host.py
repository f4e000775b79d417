"""cp_instance_map restated on the host in plain numpy, from the definitions of include/centerpoly_hip.h.
TEST INFRASTRUCTURE.

Written the other way round from the kernel: the instances are sorted by `before` and painted back to front, every
cover overwriting what lies behind it (the kernel walks front to back and lets the first cover win)."""
import math

import numpy as np

NONE = 255


def order(n, prio):
    """The indices 0 .. n-1 sorted by `before`: by index without prio; otherwise by prio, ties by index, a NaN after
    every number (NaNs among themselves by index).  -0.0 and 0.0 are equal, as they are to `<`."""
    if prio is None:
        return list(range(n))
    key = []
    for i in range(n):
        p = float(prio[i])
        key.append((1, 0.0, i) if math.isnan(p) else (0, p + 0.0, i))
    return [k[2] for k in sorted(key)]


def instance_map(masks, flags, flag_mask, counts, min_count, label, prio, bounds, multiplier, background):
    """(index uint8 [H, W], ids int32 [H, W], labels int32 [H, W], value int32 [n], visible int32 [n],
    box int32 [n, 4]) of masks uint8 [n, H, W]."""
    masks = np.asarray(masks)
    n, H, W = masks.shape
    flags = np.asarray(flags, np.int64).reshape(n)
    label = np.asarray(label, np.int64).reshape(n)
    live = (flags & flag_mask) != 0
    if counts is not None:
        live &= np.asarray(counts, np.int64).reshape(n) > min_count
    value = np.full(n, -1, np.int64)
    for i in range(n):
        if live[i]:
            value[i] = label[i] * multiplier + sum(1 for j in range(i) if live[j] and label[j] == label[i])
    index = np.full((H, W), NONE, np.uint8)
    for i in reversed(order(n, prio)):
        if not live[i]:
            continue
        x0, y0, x1, y1 = (0, 0, W - 1, H - 1) if bounds is None else (int(v) for v in bounds[i])
        x0, y0, x1, y1 = max(x0, 0), max(y0, 0), min(x1, W - 1), min(y1, H - 1)
        if x1 < x0 or y1 < y0:
            continue
        window = index[y0:y1 + 1, x0:x1 + 1]
        window[masks[i, y0:y1 + 1, x0:x1 + 1] != 0] = i
    won = index != NONE
    lut_value = np.concatenate([value, np.full(256 - n, background)]).astype(np.int64)
    lut_label = np.concatenate([label, np.full(256 - n, background)]).astype(np.int64)
    ids = np.where(won, lut_value[index], background)
    labels = np.where(won, lut_label[index], background)
    visible = np.zeros(n, np.int64)
    box = np.tile(np.array([W, H, -1, -1], np.int64), (n, 1))
    for i in range(n):
        ys, xs = np.nonzero(index == i)
        visible[i] = len(ys)
        if len(ys):
            box[i] = [xs.min(), ys.min(), xs.max(), ys.max()]
    return (index, ids.astype(np.int32), labels.astype(np.int32), value.astype(np.int32), visible.astype(np.int32),
            box.astype(np.int32))

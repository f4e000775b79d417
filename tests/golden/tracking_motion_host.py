"""Host statement (numpy, plain loops) of "instance tracking with motion" in include/centerpoly_hip.h, written from the
definition.  It shares no code with the package; of tracking_host.py it takes what that file already states
(associate, update, T, NONE).  Python integers throughout: no product or quotient can overflow."""
import numpy as np

from tracking_host import NONE, T, associate, update


def clamp(v, lo, hi):
    return lo if v < lo else hi if v > hi else v


def trunc_div(a, b):
    """a / b rounded toward zero, as C divides."""
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def predict(slots, kin, t, H, W):
    """Step 1: int64 [T, 2] = (dx, dy) per slot."""
    shift = np.zeros((T, 2), np.int64)
    for s in range(T):
        if int(slots[s][0]) != 0 and int(kin[s][5]) != 0:
            g = t - int(kin[s][4])
            shift[s, 0] = clamp((int(kin[s][2]) * g + 8) // 16, -W, W)          # // is the floor division
            shift[s, 1] = clamp((int(kin[s][3]) * g + 8) // 16, -H, H)
    return shift


def map_pairs_shifted(a, shift, b, R, n):
    """Step 2: int64 [R + 1, n + 1]."""
    a, b = np.asarray(a), np.asarray(b)
    H, W = a.shape
    pairs = np.zeros((R + 1, n + 1), np.int64)
    area_cur = np.zeros((n + 1,), np.int64)
    for y in range(H):
        for x in range(W):
            c = int(b[y, x])
            area_cur[c if c < n else n] += 1
            s = int(a[y, x])
            if s >= R:
                continue
            qx, qy = x + int(shift[s][0]), y + int(shift[s][1])
            if 0 <= qx < W and 0 <= qy < H:
                c = int(b[qy, qx])
                pairs[s, c if c < n else n] += 1
    for k in range(n + 1):
        pairs[R, k] = area_cur[k] - sum(int(pairs[s, k]) for s in range(R))
    return pairs


def centroid16(S, A):
    return (32 * S + A) // (2 * A)


def kinematics(index, n, inst, slots, t, kin):
    """Step 4 on the tables after the association: the new kin, int64 [T, 6]; `kin` is not changed."""
    index = np.asarray(index)
    kin = np.array(kin, np.int64).reshape(T, 6)
    A, Sx, Sy = [0] * n, [0] * n, [0] * n
    for y in range(index.shape[0]):
        for x in range(index.shape[1]):
            k = int(index[y, x])
            if k < n:
                A[k] += 1
                Sx[k] += x
                Sy[k] += y
    for k in range(n):
        s, is_new = int(inst[k][0]), int(inst[k][4]) != 0
        if s < 0:
            continue
        if A[k] == 0:
            if is_new:
                kin[s] = 0
            continue
        cx, cy = centroid16(Sx[k], A[k]), centroid16(Sy[k], A[k])
        if is_new or int(kin[s, 5]) == 0:
            kin[s] = [cx, cy, 0, 0, t, 1]
        else:
            g = t - int(kin[s, 4])
            kin[s] = [cx, cy, trunc_div(cx - int(kin[s, 0]), g), trunc_div(cy - int(kin[s, 1]), g), t, 1]
    for s in range(T):
        if int(slots[s][0]) == 0:
            kin[s] = 0
    return kin


class Tracker(object):
    def __init__(self, H, W, iou_thresh=0.3, max_age=0, multiplier=1000):
        self.shape, self.iou_thresh, self.max_age, self.multiplier = (H, W), iou_thresh, max_age, multiplier
        self.reset()

    def reset(self):
        self.mem = np.full(self.shape, NONE, np.int64)
        self.slots = np.zeros((T, 5), np.int64)
        self.kin = np.zeros((T, 6), np.int64)
        self.next_id, self.t = 1, 0

    def step(self, index, n, label, live):
        """One frame; returns {"shift", "pairs", "inst", "assigned", "ids"} and leaves mem / slots / kin / next_id / t
        updated.  More than 256 tracks alive: associate's ValueError, nothing changed."""
        H, W = self.shape
        shift = predict(self.slots, self.kin, self.t, H, W)
        pairs = map_pairs_shifted(self.mem, shift, index, T, n)
        slots, next_id, inst, assigned = associate(pairs, n, label, live, self.slots, self.next_id, self.iou_thresh,
                                                   self.max_age, self.t)
        self.kin = kinematics(index, n, inst, slots, self.t, self.kin)
        self.mem, ids = update(self.mem, index, n, label, slots, inst, assigned, self.multiplier)
        self.slots, self.next_id = slots, next_id
        self.t += 1
        return {"shift": shift, "pairs": pairs, "inst": inst, "assigned": assigned, "ids": ids}

"""Host statement (numpy, plain loops) of "instance tracking" in include/centerpoly_hip.h and of the MOTS scoring rule
of centerpoly_amd/datasets/evaluation/tracking.py, written from the definitions.  It shares no code with the package;
the tests compare the device tables with what is computed here."""
from fractions import Fraction

import numpy as np

T = 256
NONE = 0xffff
TOO_MANY = "more than 256 tracks alive"


def map_pairs(a, b, R, n, row_of=None):
    """int64 [R + 1, n + 1]: pixels per (row, column), the none row R and the none column n included."""
    a, b = np.asarray(a).reshape(-1), np.asarray(b).reshape(-1)
    pairs = np.zeros((R + 1, n + 1), np.int64)
    for p in range(a.size):
        r = int(a[p]) if row_of is None else int(row_of[int(a[p])])
        c = int(b[p])
        pairs[r if r < R else R, c if c < n else n] += 1
    return pairs


def associate(pairs, n, label, live, slots, next_id, iou_thresh, max_age, t):
    """Stage 2 on a pair table [T + 1, n + 1].  Returns (slots, next_id, inst [n, 5], assigned [T]) or raises
    ValueError(TOO_MANY); the arguments are not changed."""
    pairs = np.asarray(pairs, np.int64).reshape(T + 1, n + 1)
    slots = np.array(slots, np.int64).reshape(T, 5)
    area_mem, area_cur = pairs.sum(1), pairs.sum(0)
    cands = []
    for s in range(T):
        for k in range(n):
            inter = int(pairs[s, k])
            if slots[s, 0] == 0 or not live[k] or int(slots[s, 1]) != int(label[k]) or inter <= 0:
                continue
            union = int(area_mem[s] + area_cur[k] - inter)
            if float(inter) / float(union) >= float(iou_thresh):
                cands.append((-Fraction(inter, union), int(slots[s, 0]), k, s, inter, union))
    inst = np.zeros((n, 5), np.int64)
    inst[:, 0] = -1
    assigned = np.zeros((T,), np.int64)
    while cands:
        _, tid, k, s, inter, union = min(cands)
        inst[k] = [s, tid, inter, union, 0]
        assigned[s] = 1
        slots[s, 3] = t
        slots[s, 4] += 1
        cands = [c for c in cands if c[2] != k and c[3] != s]
    for k in range(n):
        if live[k] and inst[k, 0] < 0:
            free = [s for s in range(T) if slots[s, 0] == 0]
            if not free:
                raise ValueError(TOO_MANY)
            s = free[0]
            slots[s] = [next_id, int(label[k]), t, t, 1]
            inst[k] = [s, next_id, 0, 0, 1]
            assigned[s] = 1
            next_id += 1
    for s in range(T):
        if slots[s, 0] != 0 and slots[s, 3] < t - max_age:
            slots[s] = 0
    return slots, next_id, inst, assigned


def update(mem, index, n, label, slots, inst, assigned, multiplier):
    """Stage 3: (mem, ids) after the frame."""
    mem, index = np.asarray(mem, np.int64), np.asarray(index, np.int64)
    out, ids = np.full(mem.shape, NONE, np.int64), np.zeros(mem.shape, np.int64)
    for y in range(mem.shape[0]):
        for x in range(mem.shape[1]):
            k, s = int(index[y, x]), int(mem[y, x])
            if k < n and inst[k][0] >= 0:
                out[y, x] = inst[k][0]
                ids[y, x] = int(label[k]) * multiplier + inst[k][1]
            elif s < T and slots[s][0] != 0 and not assigned[s]:
                out[y, x] = s
    return out, ids


class Tracker(object):
    def __init__(self, H, W, iou_thresh=0.3, max_age=0, multiplier=1000):
        self.shape, self.iou_thresh, self.max_age, self.multiplier = (H, W), iou_thresh, max_age, multiplier
        self.reset()

    def reset(self):
        self.mem = np.full(self.shape, NONE, np.int64)
        self.slots = np.zeros((T, 5), np.int64)
        self.next_id, self.t = 1, 0

    def step(self, index, n, label, live):
        """One frame; returns {"pairs", "inst", "assigned", "ids"} and leaves mem / slots / next_id / t updated."""
        pairs = map_pairs(self.mem, index, T, n)
        slots, next_id, inst, assigned = associate(pairs, n, label, live, self.slots, self.next_id, self.iou_thresh,
                                                   self.max_age, self.t)
        self.mem, ids = update(self.mem, index, n, label, slots, inst, assigned, self.multiplier)
        self.slots, self.next_id = slots, next_id
        self.t += 1
        return {"pairs": pairs, "inst": inst, "assigned": assigned, "ids": ids}


class Mots(object):
    """The MOTS measures (Voigtlaender et al., CVPR 2019), per class and for all classes.
    add_frame(sequence key, gt id image, index, n, label, live, track id per instance)."""

    def __init__(self, multiplier, class_labels, ignore_id=10000):
        self.multiplier, self.class_labels, self.ignore_id = multiplier, tuple(class_labels), ignore_id
        self.count = {c: {"tp": 0, "fp": 0, "fn": 0, "ids": 0, "soft_tp": 0.0} for c in self.class_labels}
        self.last = {}                                          # (sequence, object id) -> track id of its last match

    def add_frame(self, seq, gt, index, n, label, live, track_id):
        gt, index = np.asarray(gt, np.int64), np.asarray(index, np.int64)
        ignore = np.zeros(gt.shape, bool)
        objects = set()
        for y in range(gt.shape[0]):
            for x in range(gt.shape[1]):
                v = int(gt[y, x])
                if v == self.ignore_id or (v < self.multiplier and v in self.class_labels):
                    ignore[y, x] = True
                elif v >= self.multiplier and v // self.multiplier in self.class_labels:
                    objects.add(v)
        preds = [k for k in range(n) if live[k] and (index == k).any()]
        for c in self.class_labels:
            cnt = self.count[c]
            matched_pred = set()
            for v in sorted(o for o in objects if o // self.multiplier == c):
                hit = None
                for k in preds:
                    if int(label[k]) != c:
                        continue
                    inter = int(((gt == v) & (index == k)).sum())
                    union = int((gt == v).sum() + (index == k).sum() - inter)
                    if Fraction(inter, union) > Fraction(1, 2):
                        hit = (k, inter, union)
                if hit is None:
                    cnt["fn"] += 1
                    continue
                k, inter, union = hit
                matched_pred.add(k)
                cnt["tp"] += 1
                cnt["soft_tp"] += float(inter) / float(union)
                if (seq, v) in self.last and self.last[(seq, v)] != int(track_id[k]):
                    cnt["ids"] += 1
                self.last[(seq, v)] = int(track_id[k])
            for k in preds:
                if int(label[k]) == c and k not in matched_pred:
                    area = int((index == k).sum())
                    if not 2 * int(((index == k) & ignore).sum()) > area:
                        cnt["fp"] += 1

    @staticmethod
    def measures(cnt):
        m = cnt["tp"] + cnt["fn"]
        nan = float("nan")
        return {"motsa": (cnt["tp"] - cnt["fp"] - cnt["ids"]) / m if m else nan,
                "smotsa": (cnt["soft_tp"] - cnt["fp"] - cnt["ids"]) / m if m else nan,
                "motsp": cnt["soft_tp"] / cnt["tp"] if cnt["tp"] else nan}

    def results(self):
        total = {key: sum(self.count[c][key] for c in self.class_labels) for key in ("tp", "fp", "fn", "ids", "soft_tp")}
        out = {"per_class": {c: dict(self.count[c], **self.measures(self.count[c])) for c in self.class_labels}}
        out["all"] = dict(total, **self.measures(total))
        return out

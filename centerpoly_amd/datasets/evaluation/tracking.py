"""The MOTS measures of Voigtlaender et al. (MOTS: Multi-Object Tracking and Segmentation, CVPR 2019) -- MOTSA,
sMOTSA, MOTSP, TP, FP, FN, IDS -- per class and for all classes, for the tracks of detectors/tracking.py.  Not in the
reference; the rule is stated here and in tests/golden/tracking_host.py.

The ground truth is the per-frame instance-id image the AP is scored against.  Its instance ids must be consistent over
a sequence (the same object keeps its id from frame to frame): that is the user's data -- the Cityscapes `gtFine` ids of
the annotated frames are per image and say nothing about identity; KITTI MOTS style ids do.

Rule, per frame and class:
  * a ground-truth object is an id v >= multiplier, v != ignore_id, whose label v // multiplier is an instance class
  * the ignore region is the pixels with v == ignore_id (10000, KITTI MOTS) and the pixels with v < multiplier where v
    is an instance-class label (Cityscapes crowd groups)
  * a prediction is a live instance that owns at least one pixel (InstanceMaps.index)
  * a prediction matches an object of its class when IoU > 0.5, strictly (decided on integers: 2 inter > union); both
    sides are disjoint, so matches are unique.  A match is a TP and adds its IoU to the soft sum
  * an unmatched prediction is an FP unless more than half of its pixels lie in the ignore region
  * an unmatched object is an FN
  * an IDS is a matched object whose most recent earlier match in the same sequence was to another track id
MOTSA = (TP - FP - IDS) / |M|, sMOTSA = (soft TP - FP - IDS) / |M|, MOTSP = soft TP / TP with |M| = TP + FN the number
of objects; NaN where the denominator is 0.

Per frame the pixel counts come from cp_map_pairs -- the ground-truth ids through a lookup built on the device (ignore
region -> row 0, the frame's objects -> rows 1 .. G, everything else -> none) against the owner map -- and the rule runs
on that small table, read back in one copy."""
import json
import os
import re

import numpy as np

from . import instance_level as il

RESULT_FILE = "resultTracking.json"
MAX_OBJECTS = 1023                                      # objects per frame: rows 1 .. 1023 of cp_map_pairs' 1024
ROWS = 1024
IGNORE_ID = 10000
TRACK_SUFFIX = "_trackIds.png"
DATASET_PROTOCOL = {"cityscapes": "cityscapes", "kitti_poly": "kitti", "IDD": "IDD"}
KEYS = ("tp", "fp", "fn", "ids", "soft_tp")


def sequence_key(file_name):
    """The sequence of a frame: its directory plus, for `<city>_<seq>_<frame>...` names, `<city>_<seq>`."""
    d, base = os.path.split(str(file_name))
    m = re.match(r"^([^_]+_\d+)_\d+", base)
    return d + "/" + (m.group(1) if m else "")


def measures(cnt):
    m, nan = cnt["tp"] + cnt["fn"], float("nan")
    return {"motsa": (cnt["tp"] - cnt["fp"] - cnt["ids"]) / m if m else nan,
            "smotsa": (cnt["soft_tp"] - cnt["fp"] - cnt["ids"]) / m if m else nan,
            "motsp": cnt["soft_tp"] / cnt["tp"] if cnt["tp"] else nan}


class TrackingEvaluator(object):
    """Collects the counts frame by frame (add_frame / add_maps on the device, add_table from a pair table) and scores
    them (results)."""

    def __init__(self, protocol=il.CITYSCAPES, ignore_id=IGNORE_ID, device=None):
        self.protocol, self.ignore_id, self.device = protocol, int(ignore_id), device
        self.multiplier = int(protocol.id_multiplier)
        self.class_labels = tuple(int(l) for l in protocol.label_ids)
        self.names = dict(zip(self.class_labels, protocol.inst_labels))
        self.count = {c: {"tp": 0, "fp": 0, "fn": 0, "ids": 0, "soft_tp": 0.0} for c in self.class_labels}
        self.last = {}                                          # (sequence, object id) -> track id of its last match
        self.frames = 0
        self._dev = None

    def _tables(self, device):
        if self._dev is None:
            import torch
            v = torch.arange(65536, dtype=torch.int64, device=device)
            labels = torch.tensor(self.class_labels, dtype=torch.int64, device=device)
            ignore = (v == self.ignore_id) | ((v < self.multiplier) & torch.isin(v, labels))
            obj = (v >= self.multiplier) & (v != self.ignore_id) & torch.isin(v // self.multiplier, labels)
            self._dev = {"v": v.to(torch.int32), "obj": obj,
                         "base": torch.where(ignore, 0, 0xffff).to(torch.int32)}
            self.device = device
        return self._dev

    def add_frame(self, seq, index_dev, n, label, live, track_id, gt_ids_dev, name=""):
        """One frame on the device: index_dev uint8 [H, W] (a pixel's instance, anything >= n for none), per instance
        label, live flag and track id (host), gt_ids_dev the ground-truth ids (a device tensor of 16-bit integers, or a
        host uint16 array, which is uploaded)."""
        import torch

        from ...detectors import tracking as trk
        what = name or "frame %d" % self.frames
        n = int(n)
        if not 0 <= n <= trk.MAX_COLS:
            raise ValueError("%s: %d instances, more than %d" % (what, n, trk.MAX_COLS))
        gt = il.device_ids(gt_ids_dev, index_dev.device, what)
        if tuple(gt.shape) != tuple(index_dev.shape):
            raise ValueError("%s: the ground truth is %s, the prediction is %s"
                             % (what, tuple(gt.shape), tuple(index_dev.shape)))
        t = self._tables(index_dev.device)
        gt = trk.as_bits16(gt).contiguous()
        values = gt.reshape(-1).to(torch.int64) & 0xffff
        present = torch.bincount(values, minlength=65536) > 0
        is_obj = present & t["obj"]
        rank = torch.cumsum(is_obj, 0, dtype=torch.int32).clamp(max=ROWS)  # an object's row, 1 .. G (1024: none)
        row_of = torch.where(is_obj, rank, t["base"]).to(torch.int16)     # (0xffff keeps its bits)
        out = torch.zeros((ROWS + 1 + (ROWS + 1) * (n + 1),), dtype=torch.int32, device=gt.device)
        head = out[:ROWS + 1]                                             # [0] = G, [r] = the id of row r
        head.scatter_(0, torch.where(is_obj, rank, torch.zeros_like(rank)).long(), t["v"])
        head[0] = rank[-1]
        trk.map_pairs(gt, index_dev.contiguous(), ROWS, n, row_of=row_of, out=out[ROWS + 1:])
        host = out.cpu().numpy()                                          # the one copy
        G = int(host[0])
        if G > MAX_OBJECTS:
            raise ValueError("%s: %d ground-truth objects in one frame, more than %d" % (what, G, MAX_OBJECTS))
        pairs = host[ROWS + 1:].reshape(ROWS + 1, n + 1)
        self.add_table(seq, host[1:G + 1], np.concatenate([pairs[:G + 1], pairs[ROWS:]]), n, label, live, track_id)

    def add_maps(self, seq, maps, tracked, gt_ids_dev, name=""):
        """One frame from its InstanceMaps and the TrackedFrame of InstanceTracker.step."""
        t = maps.table
        return self.add_frame(seq, maps.index, t["n"], t["label"], t["live"], tracked.table["track_id"], gt_ids_dev, name)

    def add_table(self, seq, object_ids, pairs, n, label, live, track_id):
        """One frame from its pair table int [G + 2, n + 1]: row 0 the ignore region, rows 1 .. G the objects
        `object_ids`, the last row everything else; the last column the pixels no instance owns."""
        pairs = np.asarray(pairs, np.int64)
        object_ids = np.asarray(object_ids, np.int64)
        area_gt, area_pred = pairs.sum(1), pairs.sum(0)
        for c in self.class_labels:
            cnt = self.count[c]
            preds = [k for k in range(int(n)) if live[k] and int(label[k]) == c and area_pred[k] > 0]
            matched = set()
            for r in np.flatnonzero(object_ids // self.multiplier == c) + 1:
                hit = None
                for k in preds:
                    inter = int(pairs[r, k])
                    union = int(area_gt[r] + area_pred[k] - inter)
                    if 2 * inter > union:
                        hit = (k, inter, union)
                if hit is None:
                    cnt["fn"] += 1
                    continue
                k, inter, union = hit
                matched.add(k)
                cnt["tp"] += 1
                cnt["soft_tp"] += float(inter) / float(union)
                key = (seq, int(object_ids[r - 1]))
                if key in self.last and self.last[key] != int(track_id[k]):
                    cnt["ids"] += 1
                self.last[key] = int(track_id[k])
            for k in preds:
                if k not in matched and not 2 * int(pairs[0, k]) > int(area_pred[k]):
                    cnt["fp"] += 1
        self.frames += 1

    def results(self):
        """{"per_class": {label id: counts and measures}, "all": the same over the summed counts, "frames"}."""
        total = {key: sum(self.count[c][key] for c in self.class_labels) for key in KEYS}
        out = {"per_class": {c: dict(self.count[c], name=self.names[c], **measures(self.count[c]))
                             for c in self.class_labels}}
        out["all"] = dict(total, **measures(total))
        out["frames"] = self.frames
        return out

    def format_table(self, res=None):
        res = self.results() if res is None else res
        cols = ("sMOTSA", "MOTSA", "MOTSP", "TP", "FP", "FN", "IDS")
        head = "Class".ljust(14) + "| " + "  ".join(h.rjust(6) for h in cols)
        row = lambda name, r: name.ljust(14) + "| " + "  ".join(                                       # noqa: E731
            ["%6.1f" % (100 * r[k]) for k in ("smotsa", "motsa", "motsp")] + ["%6d" % r[k] for k in ("tp", "fp", "fn", "ids")])
        per_class = {int(k): v for k, v in res["per_class"].items()}
        lines = [head] + [row(per_class[c]["name"], per_class[c]) for c in sorted(per_class)]
        lines += ["-" * len(head), row("all", res["all"])]
        return "\n".join(lines)

    def print_table(self, res=None):
        print(self.format_table(res))

    def write_json(self, save_dir, res=None):
        res = self.results() if res is None else res
        os.makedirs(save_dir, exist_ok=True)
        path = os.path.join(save_dir, RESULT_FILE)
        with open(path, "w") as f:
            json.dump(res, f, sort_keys=True, indent=4)
        return path


def index_of_track_png(path, multiplier):
    """A `*_trackIds.png` (v = label * multiplier + track_id, 0 for none) as (index uint8 [H, W], labels, track ids):
    its distinct non-zero values, ascending, become instances 0 .. n-1."""
    ids = il.read_gt_ids(path).astype(np.int64)
    values = np.unique(ids)
    values = values[values != 0]
    if len(values) > 255:
        raise ValueError("%s: %d instances in one frame, more than 255" % (path, len(values)))
    index = np.full(ids.shape, 255, np.uint8)
    inside = ids != 0
    index[inside] = np.searchsorted(values, ids[inside]).astype(np.uint8)
    return index, (values // multiplier).astype(np.int32), (values % multiplier).astype(np.int32)


def evaluate_result_dir(pred_dir, gt_dir, device=None, protocol=il.CITYSCAPES, ignore_id=IGNORE_ID):
    """Scores the `<stem>_trackIds.png` files below pred_dir (demo.py / test.py --track --save_ids, or made anywhere)
    against the ground-truth id images below gt_dir, matched by the protocol's image key; frames in sorted order, the
    sequence of a frame from its ground-truth file's name (sequence_key).  Returns the result dictionary."""
    import torch
    dev = device or torch.device("cuda")
    preds = {}
    for root, _, files in os.walk(pred_dir):
        for f in sorted(files):
            if f.endswith(TRACK_SUFFIX):
                preds[protocol.image_key(os.path.join(root, f[:-len(TRACK_SUFFIX)] + ".png"))] = os.path.join(root, f)
    ev = TrackingEvaluator(protocol, ignore_id, dev)
    for key, gt in sorted(il.find_gt_files(gt_dir, protocol).items()):
        if key not in preds:
            raise ValueError("%s holds no *%s for image %s (ground truth %s)" % (pred_dir, TRACK_SUFFIX, key, gt))
        index, labels, tracks = index_of_track_png(preds[key], int(protocol.id_multiplier))
        ev.add_frame(sequence_key(gt), torch.from_numpy(index).to(dev), len(labels), labels, np.ones(len(labels), bool),
                     tracks, il.read_gt_ids(gt), preds[key])
    return ev.results()

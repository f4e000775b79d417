"""Panoptic quality (PQ / SQ / RQ) of Cityscapes, the protocol of the cityscapesscripts' evalPanopticSemanticLabeling
(pq_compute_single_core, average_pq), written from the algorithm and run on the device.

The ground truth is the `*_gtFine_instanceIds.png` image itself.  createPanopticImgs.py derives its panoptic PNG and
JSON from that file alone: a pixel of an `ignoreInEval` label is VOID, every other distinct value is one segment of
category v < 1000 ? v : v // 1000, and a value below 1000 of a label with instances is a crowd region.  cp_panoptic_pairs
applies exactly that rule on the device, so no panoptic PNG or JSON of the ground truth is read (the fixtures under
tests/golden/ are made by the reference's own converter and evaluator and prove it).

Per image the device path issues two calls and brings nothing back: cp_panoptic_pairs finds the segments and counts
every (segment, prediction) pair, cp_panoptic_match runs the matching and adds to the run-long tables tp / fp / fn
(int64 [L, 3]) and the IoU sums (float64 [L]).  `results()` reads those few hundred bytes once.

The prediction is an 8-bit index image (InstanceMaps.index: the slot of the owning instance, 255 for none) with one label
per slot -- detector.instances() gives every pixel one owner, a panoptic segmentation of the thing classes.
`save_panoptic` / `write_panoptic_json` write it in COCO panoptic format for the official script, and
`evaluate_result_dir` scores such files made anywhere, stuff segments included."""
import ctypes
import json
import os

import numpy as np

from . import instance_level as il
from . import pixel_level

RESULT_FILE = "resultPanopticSemanticLabeling.json"
MAX_ROWS = 1024                                          # ground-truth segments per image (cp_panoptic_pairs)
MAX_SLOTS = 255                                          # predicted segments per image
# data sets test.py scores with --panoptic; the others are refused at parse time with these reasons
DATASETS = ("cityscapes",)
REFUSED = {"kitti_poly": "the reference has no panoptic evaluator for KITTI to pin a protocol against",
           "IDD": "the reference has no panoptic evaluator for IDD to pin a protocol against",
           "synthetic": "the synthetic set has no ground truth"}


class PanopticProtocol(object):
    """The label table as the evaluator's categories: the evaluated labels, `isthing` = has instances.
      flags   uint8 [L] of cp_panoptic_pairs: bit 0 evaluated, bit 1 has instances
      ap      the instance-level protocol of the data set (ground-truth file names and keys)"""

    def __init__(self, name, labels, id_divisor, id_direct_below, ap):
        self.name, self.labels, self.ap = name, tuple(labels), ap
        self.id_divisor, self.id_direct_below = int(id_divisor), int(id_direct_below)
        assert [r[0] for r in self.labels] == list(range(len(self.labels)))
        self.L = len(self.labels)
        self.flags = np.array([(0 if r[4] else 1) | (2 if r[3] else 0) for r in self.labels], np.uint8)
        self.categories = {r[0]: {"id": r[0], "name": r[1], "supercategory": r[2], "isthing": 1 if r[3] else 0}
                           for r in self.labels if not r[4]}


CITYSCAPES = PanopticProtocol("cityscapes", pixel_level.LABELS, 1000, 1000, il.CITYSCAPES)


def _host_ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


class PanopticEvaluator(object):
    """Collects tp / fp / fn and the IoU sums image by image (add_maps / add_index on the device, add_stats from
    tables) and scores them (results)."""

    def __init__(self, protocol=CITYSCAPES, device=None):
        self.protocol, self.device = protocol, device
        self.stat_host = np.zeros((protocol.L, 3), np.int64)              # what add_stats brought
        self.iou_host = np.zeros((protocol.L,), np.float64)
        self.images = 0
        self._dev = None                                                   # the device tables, made at the first image

    def _tables(self, device):
        if self._dev is None:
            import torch

            from ... import _C
            L = self.protocol.L
            nbytes = _C.lib().cp_panoptic_pairs_workspace_bytes()
            self._dev = {"seg": torch.zeros((MAX_ROWS + 1, 4), dtype=torch.int32, device=device),
                         "pairs": torch.zeros(((MAX_ROWS + 1) * (MAX_SLOTS + 1),), dtype=torch.int32, device=device),
                         "stat": torch.zeros((L, 3), dtype=torch.int64, device=device),
                         "iou": torch.zeros((L,), dtype=torch.float64, device=device),
                         "bad": torch.zeros((2,), dtype=torch.int32, device=device),
                         "ws": _C.workspace(nbytes, device), "ws_bytes": nbytes}
            self.device = device
        return self._dev

    def add_stats(self, stat, iou):
        """One image (or a whole run) from its tables: stat int [L, 3] = tp, fp, fn and iou float64 [L]."""
        self.stat_host += np.asarray(stat, np.int64).reshape(self.protocol.L, 3)
        self.iou_host += np.asarray(iou, np.float64).reshape(self.protocol.L)
        self.images += 1

    def add_index(self, index_dev, n, pred_label, gt_ids_dev, name="", match_dev=None):
        """One image on the device: index_dev uint8 [H, W] (a pixel's slot, anything >= n for none), pred_label the n
        slots' labels, gt_ids_dev a device int16 / uint16 tensor [H, W] holding the ids' bits (a host uint16 array is
        uploaded).  Two
        calls, nothing comes back; `match_dev` (device int32 [n]) receives the slots' matched rows if given."""
        import torch

        from ... import _C
        p = self.protocol
        what = name or "image %d" % self.images
        n = int(n)
        if index_dev.dim() != 2 or index_dev.dtype != torch.uint8:
            raise ValueError("%s: the index image must be uint8 [H, W], got %s %s"
                             % (what, index_dev.dtype, tuple(index_dev.shape)))
        if not 0 <= n <= MAX_SLOTS:
            raise ValueError("%s: %d predicted segments, more than %d" % (what, n, MAX_SLOTS))
        labels = np.ascontiguousarray(pred_label, np.int32).reshape(-1)
        if len(labels) < n:
            raise ValueError("%s: %d slot labels for %d slots" % (what, len(labels), n))
        gt_ids_dev = il.device_ids(gt_ids_dev, index_dev.device, what)
        if tuple(gt_ids_dev.shape) != tuple(index_dev.shape):
            raise ValueError("%s: the ground truth is %s, the prediction is %s"
                             % (what, tuple(gt_ids_dev.shape), tuple(index_dev.shape)))
        H, W = (int(v) for v in index_dev.shape)
        t = self._tables(index_dev.device)
        lib, st = _C.lib(), _C.stream()
        index_dev, gt_ids_dev = index_dev.contiguous(), gt_ids_dev.contiguous()
        _C.check(lib.cp_panoptic_pairs(_C.ptr(index_dev), n, _C.ptr(gt_ids_dev), H, W, p.id_divisor, p.id_direct_below,
                                       p.L, _host_ptr(p.flags), _C.ptr(t["seg"]), _C.ptr(t["pairs"]), _C.ptr(t["ws"]),
                                       t["ws_bytes"], st), "cp_panoptic_pairs")
        _C.check(lib.cp_panoptic_match(_C.ptr(t["seg"]), _C.ptr(t["pairs"]), n, _host_ptr(labels) if n else None, p.L,
                                       _host_ptr(p.flags), _C.ptr(t["stat"]), _C.ptr(t["iou"]), _C.ptr(t["bad"]),
                                       _C.ptr(match_dev), st), "cp_panoptic_match")
        self.images += 1

    def add_maps(self, maps, gt_ids_dev, name=""):
        """One image from its InstanceMaps (detector.instances): the segments are the slots of maps.index, a slot's
        category is the table's label; a dead slot owns no pixel and is no segment."""
        return self.add_index(maps.index, int(maps.table["n"]), maps.table["label"], gt_ids_dev, name)

    def tables(self):
        """(stat int64 [L, 3], iou float64 [L], bad int64 [2]): the host sums plus ONE read of the device tables."""
        stat, iou, bad = self.stat_host.copy(), self.iou_host.copy(), np.zeros((2,), np.int64)
        if self._dev is not None:
            stat += self._dev["stat"].cpu().numpy()
            iou += self._dev["iou"].cpu().numpy()
            bad += self._dev["bad"].cpu().numpy()
        return stat, iou, bad

    def results(self):
        """The result dictionary in the layout of the reference's average_pq: "All" / "Things" / "Stuff", each with pq,
        sq, rq (means over the classes of the group that were counted) and n (how many were), and "per_class" keyed
        by label id.  Per class, from the definition: RQ = tp / (tp + fp / 2 + fn / 2), SQ = (sum of matched IoUs) /
        tp, PQ = SQ * RQ = (sum of matched IoUs) / (tp + fp / 2 + fn / 2).  A class nothing was counted for (tp + fp +
        fn == 0) has zeros and is in no mean; a counted class without a match has SQ 0.  A group without a counted
        class has n == 0 and zeros (the reference divides by zero there)."""
        stat, iou, bad = self.tables()
        if bad[0]:
            raise ValueError("%d images hold more than %d ground-truth segments and were not scored" % (bad[0], MAX_ROWS))
        if bad[1]:
            raise ValueError("%d predicted segments carry a label that is not evaluated (unknown category_id)" % bad[1])
        ids = np.array(sorted(self.protocol.categories), np.int64)
        thing = np.array([self.protocol.categories[int(l)]["isthing"] == 1 for l in ids], bool)
        tp, fp, fn = (stat[ids, k].astype(np.float64) for k in range(3))
        matched_iou = iou[ids]
        counted = stat[ids].sum(1) > 0
        found = tp > 0
        weight = tp + (fp + fn) / 2                                        # exact: halves of small integers
        scores = np.zeros((len(ids), 3), np.float64)                       # columns pq, sq, rq
        scores[counted, 0] = matched_iou[counted] / weight[counted]
        scores[found, 1] = matched_iou[found] / tp[found]
        scores[counted, 2] = tp[counted] / weight[counted]
        keys = ("pq", "sq", "rq")
        out = {"per_class": {int(l): dict(zip(keys, (float(v) for v in row))) for l, row in zip(ids, scores)}}
        for group, member in (("All", np.ones(len(ids), bool)), ("Things", thing), ("Stuff", ~thing)):
            rows = scores[member & counted]
            # Python's sum adds class after class in label order, the order the reference accumulates in
            out[group] = {k: (sum(rows[:, j].tolist()) / len(rows) if len(rows) else 0.0) for j, k in enumerate(keys)}
            out[group]["n"] = int(len(rows))
        return out

    def format_table(self, res=None):
        """The table as text, character for character the layout the reference prints: one line per class (name in 14
        columns, then PQ, SQ, RQ in per cent with one decimal), a rule, and All / Things / Stuff with the class count."""
        res = self.results() if res is None else res
        per_class = {int(k): v for k, v in res["per_class"].items()}
        head = lambda first, names: first.ljust(14) + "| " + "  ".join(h.rjust(5) for h in names)       # noqa: E731
        cells = lambda first, r: first.ljust(14) + "| " + "  ".join("%5.1f" % (100 * r[k]) for k in ("pq", "sq", "rq"))  # noqa: E731
        lines = [head("Category", ("PQ", "SQ", "RQ"))]
        lines += [cells(self.protocol.categories[l]["name"], per_class[l]) for l in sorted(per_class)]
        foot = head("", ("PQ", "SQ", "RQ")) + " " + "N".rjust(5)
        lines += ["-" * len(foot), foot]
        lines += [cells(g, res[g]) + " %5d" % res[g]["n"] for g in ("All", "Things", "Stuff")]
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


def image_id_of(stem):
    return stem[:-len("_leftImg8bit")] if stem.endswith("_leftImg8bit") else stem


def save_panoptic(maps, out_dir, stem):
    """--save_panoptic: `<stem>_panoptic.png` in out_dir, RGB = id % 256, id // 256 % 256, id // 65536 with id = maps.ids
    (COCO panoptic format), and the image's annotation entry for write_panoptic_json, which is returned."""
    import torch
    from PIL import Image
    os.makedirs(out_dir, exist_ok=True)
    ids = maps.ids.to(torch.int64)
    rgb = torch.stack([ids % 256, ids // 256 % 256, ids // 65536], 2).to(torch.uint8).cpu().numpy()
    file_name = stem + "_panoptic.png"
    Image.fromarray(rgb).save(os.path.join(out_dir, file_name))
    t = maps.table
    info = []
    for k in range(int(t["n"])):
        if t["live"][k] and int(t["visible"][k]) > 0:
            x0, y0, x1, y1 = (int(v) for v in t["box"][k])
            info.append({"id": int(t["value"][k]), "category_id": int(t["label"][k]), "area": int(t["visible"][k]),
                         "bbox": [x0, y0, x1 - x0 + 1, y1 - y0 + 1], "iscrowd": 0})
    return {"image_id": image_id_of(stem), "file_name": file_name, "segments_info": info}


def write_panoptic_json(out_dir, entries, split="val"):
    """`cityscapes_panoptic_<split>.json` in out_dir with the entries save_panoptic returned."""
    os.makedirs(out_dir, exist_ok=True)
    path = os.path.join(out_dir, "cityscapes_panoptic_%s.json" % split)
    with open(path, "w") as f:
        json.dump({"annotations": list(entries)}, f)
    return path


def index_of_png(path, segments_info, image_id=""):
    """A COCO panoptic PNG as (index uint8 [H, W], labels int32 [n]): its segment ids, ascending, become slots 0 .. n-1,
    id 0 (VOID) becomes 255.  The PNG and the JSON must name the same segments, as the evaluator demands."""
    from PIL import Image
    rgb = np.array(Image.open(path))
    if rgb.ndim != 3 or rgb.shape[2] < 3 or rgb.dtype != np.uint8:
        raise ValueError("%s is not an 8-bit RGB image (shape %s, %s)" % (path, rgb.shape, rgb.dtype))
    rgb = rgb.astype(np.int64)
    ids = rgb[:, :, 0] + 256 * rgb[:, :, 1] + 65536 * rgb[:, :, 2]
    values = np.unique(ids)
    values = values[values != 0]
    category = {int(s["id"]): int(s["category_id"]) for s in segments_info}
    for v in values:
        if int(v) not in category:
            raise ValueError("%s (image %s): segment %d is painted in the PNG but the JSON lists no such segment"
                             % (path, image_id, v))
    missing = sorted(set(category) - set(int(v) for v in values))
    if missing:
        raise ValueError("%s (image %s): the JSON lists segments %s, which own no pixel of the PNG"
                         % (path, image_id, missing))
    if len(values) > MAX_SLOTS:
        raise ValueError("%s: %d segments in one image, more than %d" % (path, len(values), MAX_SLOTS))
    index = np.full(ids.shape, 255, np.uint8)
    inside = ids != 0
    index[inside] = np.searchsorted(values, ids[inside]).astype(np.uint8)
    return index, np.array([category[int(v)] for v in values], np.int32)


def evaluate_result_dir(pred_json, pred_folder, gt_dir, device=None, protocol=CITYSCAPES):
    """Scores COCO panoptic predictions (the JSON's `annotations` and the PNG files in pred_folder) against the
    `*_gtFine_instanceIds.png` files below gt_dir, matched by image_id.  Returns the result dictionary."""
    import torch
    dev = device or torch.device("cuda")
    with open(pred_json) as f:
        annotations = {a["image_id"]: a for a in json.load(f)["annotations"]}
    ev = PanopticEvaluator(protocol, dev)
    for key, gt in sorted(il.find_gt_files(gt_dir, protocol.ap).items()):
        if key not in annotations:
            raise ValueError("%s holds no annotation for image %s (ground truth %s)" % (pred_json, key, gt))
        ann = annotations[key]
        path = os.path.join(pred_folder, ann["file_name"])
        index, labels = index_of_png(path, ann["segments_info"], key)
        ev.add_index(torch.from_numpy(index).to(dev), len(labels), labels, il.read_gt_ids(gt), path)
    return ev.results()

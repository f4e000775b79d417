"""Pixel-level IoU and instance-weighted iIoU of Cityscapes and KITTI (the protocol of the cityscapesscripts' and the
kittiscripts' evalPixelLevelSemanticLabeling, `evalInstLevelScore = True`, `evalPixelAccuracy = False`), written from
the algorithm.

The pixel work -- the confusion matrix over the label table and, per ground-truth instance, its size, its correctly
labelled pixels and its pixels labelled within its category -- is done on the device by cp_pixel_confusion from an
8-bit prediction (a label image, or InstanceMaps.index with the instances' labels as table) and the 16-bit instance-id
image.  The matrix stays on the device for the whole run and is read once; per image one small copy brings the
instance rows back, and this module adds them up in float64 in the order the evaluators loop in (ascending id per
image, image after image), so the weighted sums are the same operations.

The ground-truth label image is derived from the instance-id image by the protocol's id rule (Cityscapes: v < 1000 ?
v : v // 1000; KITTI: v // 256).  For Cityscapes and KITTI ground truth that is exactly `*_gtFine_labelIds.png` /
`semantic/*.png`, which the data sets' own tools write from the same polygons by the same rule, so no second file is
read.  IDD's evaluate_mIoU.py scores level ids, a different protocol, and is not covered.

Per class:    IoU  = tp / (tp + fp + fn) of the matrix, fp counted over rows of labels that are evaluated;
              iIoU = the same with tp and fn replaced by sums over the instances of tp_i * avgClassSize / size_i.
Per category: the same over the labels of a category (iIoU only where every label of the category has instances).
An instance of interest is an id the protocol's rule lets in (Cityscapes v > 1000, KITTI v % 256 > 0) whose label is
evaluated and has instances (an instance id of a label without instances stops the evaluators with a KeyError; here it
is no instance)."""
import json
import math
import os

import numpy as np

from . import instance_level as il

# id, name, category, hasInstances, ignoreInEval of the Cityscapes label table (labels.py; the licence plate, id -1,
# never shows in an image); the kittiscripts use the same table
LABELS = (
    (0, "unlabeled", "void", False, True), (1, "ego vehicle", "void", False, True),
    (2, "rectification border", "void", False, True), (3, "out of roi", "void", False, True),
    (4, "static", "void", False, True), (5, "dynamic", "void", False, True), (6, "ground", "void", False, True),
    (7, "road", "flat", False, False), (8, "sidewalk", "flat", False, False), (9, "parking", "flat", False, True),
    (10, "rail track", "flat", False, True), (11, "building", "construction", False, False),
    (12, "wall", "construction", False, False), (13, "fence", "construction", False, False),
    (14, "guard rail", "construction", False, True), (15, "bridge", "construction", False, True),
    (16, "tunnel", "construction", False, True), (17, "pole", "object", False, False),
    (18, "polegroup", "object", False, True), (19, "traffic light", "object", False, False),
    (20, "traffic sign", "object", False, False), (21, "vegetation", "nature", False, False),
    (22, "terrain", "nature", False, False), (23, "sky", "sky", False, False), (24, "person", "human", True, False),
    (25, "rider", "human", True, False), (26, "car", "vehicle", True, False), (27, "truck", "vehicle", True, False),
    (28, "bus", "vehicle", True, False), (29, "caravan", "vehicle", True, True), (30, "trailer", "vehicle", True, True),
    (31, "train", "vehicle", True, False), (32, "motorcycle", "vehicle", True, False),
    (33, "bicycle", "vehicle", True, False),
)
MAX_INST = 1024                                          # limit of cp_pixel_confusion
RESULT_FILE = "resultPixelLevelSemanticLabeling.json"
AVERAGES = ("averageScoreClasses", "averageScoreInstClasses", "averageScoreCategories", "averageScoreInstCategories")


class PixelProtocol(object):
    """What the two evaluators do not share, and the label table as arrays.
      labels             the table rows (id, name, category, hasInstances, ignoreInEval), ids 0 .. L-1 in order
      avg_class_size     {class name: average instance size in pixels}, the weight of the iIoU
      id_divisor, id_direct_below   the id rule of cp_pixel_confusion
      interest(ids)      which ids the evaluator takes for instances (before the label test)
      ap                 the instance-level protocol of the same data set (ground-truth file names and keys)
      label_group        int8 [L]: index of the label's category among the categories all of whose labels have
                         instances (human, vehicle), -1 for every other label"""

    def __init__(self, name, avg_class_size, id_divisor, id_direct_below, interest, ap, labels=LABELS):
        self.name, self.labels, self.avg_class_size = name, tuple(labels), dict(avg_class_size)
        self.id_divisor, self.id_direct_below, self.interest, self.ap = int(id_divisor), int(id_direct_below), interest, ap
        assert [r[0] for r in self.labels] == list(range(len(self.labels)))
        self.L = len(self.labels)
        self.names = [r[1] for r in self.labels]
        self.has_instances = np.array([r[3] for r in self.labels], bool)
        self.ignore = np.array([r[4] for r in self.labels], bool)
        self.categories = []                                               # in order of first appearance
        for r in self.labels:
            if r[2] not in self.categories:
                self.categories.append(r[2])
        self.category_ids = {c: [r[0] for r in self.labels if r[2] == c] for c in self.categories}
        self.inst_categories = [c for c in self.categories if all(self.has_instances[self.category_ids[c]])]
        self.label_group = np.full((self.L,), -1, np.int8)
        for k, c in enumerate(self.inst_categories):
            self.label_group[self.category_ids[c]] = k

    def label_of(self, ids):
        ids = np.asarray(ids, np.int64)
        return np.where(ids < self.id_direct_below, ids, ids // self.id_divisor)

    def instances_of_interest(self, hist):
        """The ids of one image that get an instance column, ascending, from its id histogram (int [65536])."""
        ids = np.flatnonzero(np.asarray(hist))
        lab = self.label_of(ids)
        ok = self.interest(ids) & (lab < self.L)
        lab = np.minimum(lab, self.L - 1)
        return ids[ok & ~self.ignore[lab] & self.has_instances[lab]].astype(np.int64)


CITYSCAPES = PixelProtocol("cityscapes", {
    "bicycle": 4672.3249222261, "caravan": 36771.8241758242, "motorcycle": 6298.7200839748, "rider": 3930.4788056518,
    "bus": 35732.1511111111, "train": 67583.7075812274, "car": 12794.0202738185, "person": 3462.4756337644,
    "truck": 27855.1264367816, "trailer": 16926.9763313609}, 1000, 1000, lambda ids: ids > 1000, il.CITYSCAPES)
KITTI = PixelProtocol("kitti", {
    "truck": 1801.103394, "person": 1234.262573, "train": 18448.460938, "bicycle": 1244.791260,
    "motorcycle": 695.617676, "bus": 2761.151611, "caravan": 1017.777771, "rider": 1318.393921,
    "trailer": 14457.615234, "car": 3669.255859}, 256, 0, lambda ids: ids % 256 > 0, il.KITTI)
PROTOCOLS = {"cityscapes": CITYSCAPES, "kitti": KITTI}
# data sets test.py scores with --pixel_iou -> protocol; the others are refused at parse time with these reasons
DATASET_PROTOCOL = {"cityscapes": "cityscapes", "kitti_poly": "kitti"}
REFUSED = {"IDD": "IDD's evaluate_mIoU.py scores level ids, a different protocol that is not implemented",
           "synthetic": "the synthetic set has no ground truth and no result writer to draw label maps with"}


def device_confusion(pred_dev, pred_label, gt_dev, protocol, inst_ids, conf_dev):
    """cp_pixel_confusion on a device prediction uint8 [H, W] and device ids [H, W] (16-bit elements), added to
    conf_dev (device int64 [L * L]).  Returns (inst int64 [G, 3], bad int64 [2]) of THIS image, one copy."""
    import ctypes

    import torch

    from ... import _C
    H, W = (int(v) for v in pred_dev.shape)
    G = len(inst_ids)
    dev = pred_dev.device
    pred_label = np.ascontiguousarray(pred_label, np.uint8)
    if pred_label.shape != (256,):
        raise ValueError("pred_label must have 256 entries, got %s" % (pred_label.shape,))
    group = np.ascontiguousarray(protocol.label_group, np.int8)
    ids_dev = torch.tensor([int(v) for v in inst_ids], dtype=torch.int32).to(dev) if G else None
    out = torch.zeros((3 * G + 2,), dtype=torch.int32, device=dev)
    L = _C.lib()
    nbytes = L.cp_pixel_confusion_workspace_bytes(G)
    ws = _C.workspace(nbytes, dev)
    at = lambda o: ctypes.c_void_p(out.data_ptr() + 4 * o)                # noqa: E731
    _C.check(L.cp_pixel_confusion(_C.ptr(pred_dev), pred_label.ctypes.data_as(ctypes.c_void_p), _C.ptr(gt_dev), H, W,
                                  protocol.id_divisor, protocol.id_direct_below, protocol.L,
                                  group.ctypes.data_as(ctypes.c_void_p), _C.ptr(ids_dev), G, _C.ptr(conf_dev),
                                  at(0) if G else None, at(3 * G), _C.ptr(ws), nbytes, _C.stream()),
             "cp_pixel_confusion")
    host = out.cpu().numpy().astype(np.int64)
    return host[:3 * G].reshape(G, 3), host[3 * G:]


class PixelLevelEvaluator(object):
    """Collects the counts image by image (add_image / add_maps on the device, add_counts from tables) and scores them
    (summarize)."""

    def __init__(self, protocol=CITYSCAPES):
        self.protocol = protocol
        self.conf_dev = None                                               # device int64 [L * L], read by summarize
        self.conf_host = np.zeros((protocol.L, protocol.L), np.int64)      # what add_counts brought
        self.pixels = 0
        self.images = 0
        zero = lambda: {"tp": 0.0, "tpWeighted": 0.0, "fn": 0.0, "fnWeighted": 0.0}      # noqa: E731
        self.class_stats = {r[1]: zero() for r in protocol.labels if r[3] and not r[4]}
        self.category_stats = {c: zero() for c in protocol.inst_categories}

    def add_instances(self, rows):
        """The instance rows (id, size, tp, category tp) of one image, ascending id: the evaluators' float64 sums."""
        p = self.protocol
        for inst_id, size, tp, cat_tp in np.asarray(rows, np.int64).reshape(-1, 4):
            label = int(p.label_of(inst_id))
            name, category = p.labels[label][1], p.labels[label][2]
            size, tp, cat_tp = int(size), int(tp), int(cat_tp)
            weight = p.avg_class_size[name] / float(size)
            for stats, t in ((self.class_stats[name], tp), (self.category_stats.get(category), cat_tp)):
                if stats is None:
                    continue
                stats["tp"] += t
                stats["fn"] += size - t
                stats["tpWeighted"] += float(t) * weight
                stats["fnWeighted"] += float(size - t) * weight

    def add_counts(self, conf, rows):
        """One image from its tables: its matrix int [L, L] and its instance rows (id, size, tp, category tp)."""
        conf = np.asarray(conf, np.int64).reshape(self.protocol.L, self.protocol.L)
        self.conf_host += conf
        self.pixels += int(conf.sum())
        self.images += 1
        self.add_instances(rows)

    def add_image(self, pred_dev, pred_label, gt_ids, name=""):
        """One image on the device: pred_dev uint8 [H, W], pred_label uint8 [256] (the label of every prediction
        byte), gt_ids a host uint16 [H, W] array (see read_gt_ids) or a device tensor of 16-bit elements holding those
        bits.  `name` names the image in an error.  Returns the image's instance rows (id, size, tp, category tp)."""
        import torch
        p = self.protocol
        what = name or "image %d" % self.images
        if pred_dev.dim() != 2 or pred_dev.dtype != torch.uint8:
            raise ValueError("%s: the prediction must be uint8 [H, W], got %s %s"
                             % (what, pred_dev.dtype, tuple(pred_dev.shape)))
        gt_ids = il.device_ids(gt_ids, pred_dev.device, what)
        if tuple(gt_ids.shape) != tuple(pred_dev.shape):
            raise ValueError("%s: the ground truth is %s, the prediction is %s"
                             % (what, tuple(gt_ids.shape), tuple(pred_dev.shape)))
        ids = p.instances_of_interest(il.device_histogram(gt_ids))
        if len(ids) > MAX_INST:
            raise ValueError("%s: %d ground-truth instances, more than %d" % (what, len(ids), MAX_INST))
        if self.conf_dev is None:
            self.conf_dev = torch.zeros((p.L * p.L,), dtype=torch.int64, device=pred_dev.device)
        inst, bad = device_confusion(pred_dev.contiguous(), pred_label, gt_ids.contiguous(), p, ids, self.conf_dev)
        if bad[0]:
            raise ValueError("%s: %d ground-truth pixels carry a label outside the table (Unknown label)" % (what, bad[0]))
        if bad[1]:
            raise ValueError("%s: %d predicted pixels carry a label outside the table" % (what, bad[1]))
        rows = np.concatenate([ids[:, None], inst], 1)
        self.pixels += int(pred_dev.numel())
        self.images += 1
        self.add_instances(rows)
        return rows

    def add_maps(self, maps, gt_ids, name=""):
        """One image from its InstanceMaps (detector.instances): the prediction is maps.index, the slot of the owning
        instance, and a slot's label is the table's; 255, no instance, is label 0."""
        pred_label = np.zeros((256,), np.uint8)
        lab = np.where(np.asarray(maps.table["live"], bool), np.asarray(maps.table["label"]), 0)   # a dead slot owns nothing
        if len(lab) and (lab.min() < 0 or lab.max() > 255):
            raise ValueError("%s: instance labels outside 0 .. 255" % (name or "image %d" % self.images))
        pred_label[:len(lab)] = lab
        pred_label[255] = 0
        return self.add_image(maps.index, pred_label, gt_ids, name)

    def conf_matrix(self):
        """int64 [L, L]: rows ground truth, columns prediction (ONE read of the device matrix)."""
        conf = self.conf_host.copy()
        if self.conf_dev is not None:
            conf += self.conf_dev.cpu().numpy().reshape(conf.shape)
        return conf

    def summarize(self):
        """The evaluators' result dictionary: confMatrix, priors, labels, classScores, classInstScores,
        categoryScores, categoryInstScores and the four averageScore*."""
        p = self.protocol
        conf = self.conf_matrix()
        if int(conf.sum()) != self.pixels:
            raise RuntimeError("number of analyzed pixels and entries in the confusion matrix disagree: %d, %d"
                               % (conf.sum(), self.pixels))
        every = list(range(p.L))
        total = float(conf.sum())

        def ratio(tp, fp, fn):
            denom = tp + fp + fn
            return float("nan") if denom == 0 else float(tp) / denom

        class_scores, class_inst = {}, {}
        for l in every:
            name = p.names[l]
            others = [k for k in every if not p.ignore[k] and k != l]
            fp = int(conf[others, l].sum())
            tp = int(conf[l, l])
            class_scores[name] = float("nan") if p.ignore[l] else ratio(tp, fp, int(conf[l, :].sum()) - tp)
            s = self.class_stats.get(name)
            class_inst[name] = float("nan") if p.ignore[l] or s is None else ratio(s["tpWeighted"], fp, s["fnWeighted"])
        cat_scores, cat_inst = {}, {}
        for c in p.categories:
            outside = [k for k in every if not p.ignore[k] and p.labels[k][2] != c]
            ids = [k for k in p.category_ids[c] if not p.ignore[k]]
            if not ids:
                cat_scores[c] = float("nan")
            else:
                tp = int(conf[ids, :][:, ids].sum())
                cat_scores[c] = ratio(tp, int(conf[outside, :][:, ids].sum()), int(conf[ids, :].sum()) - tp)
            s = self.category_stats.get(c)
            if s is None:
                cat_inst[c] = float("nan")
            else:
                cat_inst[c] = ratio(s["tpWeighted"], int(conf[outside, :][:, p.category_ids[c]].sum()), s["fnWeighted"])

        def average(scores):
            valid = [v for v in scores.values() if not math.isnan(v)]
            total_ = 0.0
            for v in valid:
                total_ += v
            return total_ / len(valid) if valid else float("nan")

        return {"confMatrix": conf.tolist(),
                "priors": {p.names[l]: float(conf[l, :].sum()) / total if total else float("nan") for l in every},
                "labels": {p.names[l]: l for l in every},
                "classScores": class_scores, "classInstScores": class_inst,
                "categoryScores": cat_scores, "categoryInstScores": cat_inst,
                "averageScoreClasses": average(class_scores), "averageScoreInstClasses": average(class_inst),
                "averageScoreCategories": average(cat_scores), "averageScoreInstCategories": average(cat_inst)}


def results_json(res):
    """The content of resultPixelLevelSemanticLabeling.json: the result dictionary as it is."""
    return dict(res)


def write_results(res, save_dir):
    os.makedirs(save_dir, exist_ok=True)
    path = os.path.join(save_dir, RESULT_FILE)
    with open(path, "w") as f:
        json.dump(results_json(res), f, indent=4)
    return path


def format_results(res, protocol=CITYSCAPES):
    """The evaluators' class and category tables as text."""
    row = lambda name, a, b: "{:<14}: ".format(name) + "{:>5.3f}".format(a) + "    " + "{:>5.3f}".format(b)   # noqa: E731
    rule = "-" * 32
    lines = ["", "classes          IoU      nIoU", rule]
    for r in protocol.labels:
        if not r[4]:
            lines.append(row(r[1], res["classScores"][r[1]], res["classInstScores"][r[1]]))
    lines += [rule, "Score Average : {:5.3f}    {:5.3f}".format(res["averageScoreClasses"],
                                                             res["averageScoreInstClasses"]), rule, "",
              "categories       IoU      nIoU", rule]
    for c in protocol.categories:
        if not all(protocol.ignore[protocol.category_ids[c]]):
            lines.append(row(c, res["categoryScores"][c], res["categoryInstScores"][c]))
    lines += [rule, "Score Average : {:5.3f}    {:5.3f}".format(res["averageScoreCategories"],
                                                             res["averageScoreInstCategories"]), rule, ""]
    return "\n".join(lines)


def evaluate_result_dir(pred_dir, gt_files, device=None, protocol=CITYSCAPES):
    """Scores the `<stem>_labelIds.png` files below pred_dir, as --save_ids writes them (a pixel is its label id, so
    pred_label is the identity), against the instance-id ground-truth files `gt_files`; a prediction belongs to the
    ground truth whose key its stem gives (Cityscapes: the image prefix, KITTI: the base name)."""
    import torch
    from PIL import Image
    dev = device or torch.device("cuda")
    suffix = "_labelIds.png"
    preds = {}
    for root, _, files in os.walk(pred_dir):
        for f in sorted(files):
            if f.endswith(suffix):
                preds.setdefault(protocol.ap.image_key(f[:-len(suffix)] + ".png"), []).append(os.path.join(root, f))
    ev = PixelLevelEvaluator(protocol)
    identity = np.arange(256, dtype=np.uint8)
    for gt in gt_files:
        root, base = os.path.split(gt)
        key = protocol.ap.gt_key(root, base)
        if key is None:
            key = os.path.splitext(base)[0]
        mine = preds.get(key, [])
        if len(mine) != 1:
            raise FileNotFoundError("%d prediction files *%s for %s below %s (ground truth %s)"
                                    % (len(mine), suffix, key, pred_dir, gt))
        pred = np.array(Image.open(mine[0]))
        if pred.ndim != 2 or pred.dtype != np.uint8:
            raise ValueError("%s is not a single-channel 8-bit label image (shape %s, %s)"
                             % (mine[0], pred.shape, pred.dtype))
        ev.add_image(torch.from_numpy(np.ascontiguousarray(pred)).to(dev), identity, il.read_gt_ids(gt), mine[0])
    return ev.summarize()

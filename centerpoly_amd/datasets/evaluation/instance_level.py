"""Instance-level AP of Cityscapes, KITTI and IDD (the protocol of cityscapesscripts' evalInstanceLevelSemanticLabeling),
written from the algorithm: by default the `distanceAvailable = False` case the reference runs after test.py; with
`InstanceLevelEvaluator(distances=True)` the evaluator's three settings (all, within 100 m, within 50 m: AP 100 m and
AP 50 m of the Cityscapes table), from the per-instance distances of evaluation/distances.py.

The pixel work -- one count per (predicted mask, ground-truth instance) pair, the void overlap, the mask sizes and
the ground-truth table -- is done on the device by cp_instance_overlaps / cp_id_histogram from the masks
cp_instance_masks leaves there and the 16-bit `*_gtFine_instanceIds.png` image.  This module keeps the small count
tables per image and turns them into the AP numbers in float64 on the host.

Per image and per class the protocol holds, for every threshold t in OVERLAPS:
  * ground truths: ids >= 1000 of the class with at least MIN_REGION_SIZE pixels (ids below 1000 are groups); in a
    distance setting (minRegionSize, distanceTh, distanceConf) also medDist <= distanceTh and distConf >= distanceConf,
    and an instance outside the setting is ignored like a small one (a group outside it counts twice);
  * a prediction matches a ground truth when IoU = inter / (gt + pred - inter) > t.  The first match of a ground
    truth is a true positive with the prediction's confidence; every further match makes a false positive that
    carries the lower of the two confidences, the ground truth keeping the higher;
  * a prediction that matches no ground truth of its class (groups and small ones included) is a false positive,
    unless its share of void + group + small-instance pixels exceeds t: then it is dropped;
  * a ground truth nobody matched is a hard false negative.
Precision / recall are taken at the unique scores, AP is the precision weighted by the recall steps of the
[-0.5, 0, 0.5] convolution; 0.0 for a class with ground truth and no prediction, nan for a class without ground truth."""
import fnmatch
import os
import warnings

import numpy as np

INST_LABELS = ("person", "rider", "car", "truck", "bus", "train", "motorcycle", "bicycle")
LABEL_IDS = (24, 25, 26, 27, 28, 31, 32, 33)
# labels with ignoreInEval (-1, the licence plate, never matches a 16-bit pixel)
VOID_IDS = (0, 1, 2, 3, 4, 5, 6, 9, 10, 14, 15, 16, 18, 29, 30, -1)
OVERLAPS = np.arange(0.5, 1.0, 0.05)
MIN_REGION_SIZES = np.array([100, 1000, 1000])          # only the first is used without distances
MIN_REGION_SIZE = 100
# with distances (evaluation/distances.py) the evaluator's three settings: all, within 100 m, within 50 m; a ground
# truth is real in a setting when medDist <= the bound and distConf (its stereo density) >= the density bound
DISTANCE_THS = np.array([np.inf, 100.0, 50.0])
DISTANCE_CONFS = np.array([-np.inf, 0.5, 0.5])
GT_SUFFIX = "_gtFine_instanceIds.png"
MAX_MASKS, MAX_INST = 128, 1024                          # limits of cp_instance_overlaps


class Protocol(object):
    """What the three evaluators of the reference (cityscapesscripts, kittiscripts, IDDscripts) do NOT share; the
    matching and the AP are the same protocol.
      inst_labels / label_ids   the labels with instances, in the evaluator's order
      void_ids                  raw pixel values of the labels its table marks ignoreInEval
      label_of(ids)             label id of an array of instance ids
      gt_filter(ids)            which ids enter the ground-truth table at all (before the label test)
      gt_key(dir, file)         key of a ground-truth file below --gt_dir, None for any other file
      image_key(file_name)      the same key from an image's file name
      pred_match(path, key)     whether the text file at `path` (below the result directory) is the image's
      gt_name(key)              how a missing ground-truth file is named in an error
      id_multiplier             an instance id is label * id_multiplier + k (what label_of undoes for an instance)"""

    def __init__(self, name, inst_labels, label_ids, void_ids, label_of, gt_filter, gt_key, image_key, pred_match,
                 gt_name, id_multiplier=1000):
        self.name, self.inst_labels = name, tuple(inst_labels)
        self.label_ids, self.void_ids = tuple(label_ids), tuple(void_ids)
        self.label_of, self.gt_filter, self.gt_key, self.image_key = label_of, gt_filter, gt_key, image_key
        self.pred_match, self.gt_name = pred_match, gt_name
        self.id_multiplier = id_multiplier


def _thousands(ids):
    return np.where(ids < 1000, ids, ids // 1000)


def _every(ids):
    return np.ones(ids.shape, bool)


def _suffix_key(suffix):
    return lambda root, f: f[:-len(suffix)] if f.endswith(suffix) else None


def _image_prefix(file_name):
    base = os.path.basename(file_name)
    return base[:-len("_leftImg8bit.png")] if base.endswith("_leftImg8bit.png") else os.path.splitext(base)[0]


def _idd_gt_key(root, f):
    return os.path.basename(root) + "/" + f.split("_")[0] if f.endswith(IDD_GT_SUFFIX) else None


def _idd_image_key(file_name):
    return os.path.basename(os.path.dirname(file_name)) + "/" + os.path.basename(file_name).split("_")[0]


IDD_GT_SUFFIX = "_gtFine_instanceids.png"                # lower-case `ids`, one directory per city
CITYSCAPES = Protocol("cityscapes", INST_LABELS, LABEL_IDS, VOID_IDS, _thousands, _every, _suffix_key(GT_SUFFIX),
                      _image_prefix, lambda path, key: fnmatch.fnmatch(os.path.basename(path), key + "*.txt"),
                      lambda key: key + GT_SUFFIX)
# kittiscripts: Cityscapes' label table, ids are label * 256 + k, the ground truth is `<image base name>.png`
KITTI = Protocol("kitti", INST_LABELS, LABEL_IDS, VOID_IDS, lambda ids: ids // 256, _every,
                 lambda root, f: f[:-4] if f.endswith(".png") else None,
                 lambda file_name: os.path.splitext(os.path.basename(file_name))[0],
                 lambda path, key: os.path.basename(path) == key + ".txt", lambda key: key + ".png",
                 id_multiplier=256)
# IDDscripts: the anue label table (levels of 1000 as in Cityscapes); instances2dict lets an id in only when it is
# not 255 and its thousands are a label between 6 and 18, so there are no group ids in its tables
IDD = Protocol("IDD", ("person", "rider", "motorcycle", "bicycle", "autorickshaw", "car", "truck", "bus",
                       "vehicle fallback"), (6, 8, 9, 10, 11, 12, 13, 14, 18),
               (7, 15, 16, 17, 35, 36, 37, 38, 39), _thousands,
               lambda ids: (ids != 255) & (ids // 1000 > 5) & (ids // 1000 < 19), _idd_gt_key, _idd_image_key,
               lambda path, key: fnmatch.fnmatch("/" + path, "*/" + key + "*.txt"), lambda key: key + IDD_GT_SUFFIX)
PROTOCOLS = {"cityscapes": CITYSCAPES, "kitti": KITTI, "IDD": IDD}


def gt_instances(hist, protocol=CITYSCAPES):
    """The ground-truth table of one image from its id histogram (int [65536]): int64 [G, 3] rows
    (instID, labelID, pixelCount) of the ids the protocol lets in whose label has instances, ascending instID."""
    hist = np.asarray(hist)
    ids = np.flatnonzero(hist)
    labels = protocol.label_of(ids)
    keep = np.isin(labels, protocol.label_ids) & protocol.gt_filter(ids)
    return np.stack([ids[keep], labels[keep], hist[ids[keep]]], 1).astype(np.int64).reshape(-1, 3)


def read_gt_ids(path):
    """A `*_gtFine_instanceIds.png` as uint16 [H, W] (PIL hands it over as uint16 or as 32-bit mode I)."""
    from PIL import Image
    arr = np.array(Image.open(path))
    if arr.ndim != 2 or arr.dtype.kind not in "iu":
        raise ValueError("%s is not a single-channel integer id image (shape %s, %s)" % (path, arr.shape, arr.dtype))
    if arr.size and (arr.min() < 0 or arr.max() > 65535):
        raise ValueError("%s holds ids outside 16 bits (%d .. %d)" % (path, arr.min(), arr.max()))
    return np.ascontiguousarray(arr.astype(np.uint16))


def device_ids(gt_ids, device, what=""):
    """The id image as the kernels take it, a device tensor of 16-bit integers: a host uint16 array is uploaded to
    `device` with its bits kept (as int16), a tensor is passed on where it is and only its dtype is checked.  `what`
    names the image in the error.  The shape is the caller's to check."""
    import torch
    what = what and what + ": "
    if torch.is_tensor(gt_ids):
        if gt_ids.dtype not in (torch.int16, getattr(torch, "uint16", torch.int16)):
            raise ValueError("%sthe ground truth is %s: gt_ids must be uint16 (see read_gt_ids) or a device tensor of "
                             "16-bit integers" % (what, gt_ids.dtype))
        return gt_ids
    gt_ids = np.ascontiguousarray(gt_ids)
    if gt_ids.dtype != np.uint16:
        raise ValueError("%sgt_ids must be uint16 (see read_gt_ids), got %s" % (what, gt_ids.dtype))
    return torch.from_numpy(gt_ids.view(np.int16)).to(device)


def find_gt_files(gt_dir, protocol=CITYSCAPES):
    """{image key: path} of every ground-truth file below gt_dir (Cityscapes: *_gtFine_instanceIds.png by image
    prefix; KITTI: *.png by base name; IDD: <city>/<frame>_gtFine_instanceids.png by `<city>/<frame>`)."""
    out = {}
    for root, _, files in os.walk(gt_dir):
        for f in sorted(files):
            key = protocol.gt_key(root, f)
            if key is None:
                continue
            if key in out:
                raise ValueError("two ground-truth files for %s: %s and %s" % (key, out[key], os.path.join(root, f)))
            out[key] = os.path.join(root, f)
    return out


def device_counts(masks_dev, gt_dev, inst_ids, protocol=CITYSCAPES):
    """cp_instance_overlaps on device masks uint8 [n, H, W] and device ids [H, W] (16-bit elements):
    (inter [n, G], void_inter [n], pred_pixels [n]) as host int64 arrays."""
    import torch

    from ... import _C
    n, H, W = masks_dev.shape
    G = len(inst_ids)
    dev = masks_dev.device
    inst = torch.tensor(list(inst_ids), dtype=torch.int32).to(dev)
    void = torch.tensor(protocol.void_ids, dtype=torch.int32).to(dev)
    out = torch.empty((n * G + 2 * n,), dtype=torch.int32, device=dev)
    L = _C.lib()
    nbytes = L.cp_instance_overlaps_workspace_bytes(n, G, H, W)
    ws = _C.workspace(nbytes, dev)
    _C.check(L.cp_instance_overlaps(_C.ptr(masks_dev), n, _C.ptr(gt_dev), H, W, _C.ptr(inst), G, _C.ptr(void),
                                    len(protocol.void_ids), _C.ptr(out[:n * G]), _C.ptr(out[n * G:n * G + n]),
                                    _C.ptr(out[n * G + n:]), _C.ptr(ws), nbytes, _C.stream()), "cp_instance_overlaps")
    host = out.cpu().numpy().astype(np.int64)
    return host[:n * G].reshape(n, G), host[n * G:n * G + n], host[n * G + n:]


def device_histogram(gt_dev):
    """cp_id_histogram of device ids [H, W] (16-bit elements): host int64 [65536]."""
    import torch

    from ... import _C
    H, W = gt_dev.shape
    hist = torch.empty((65536,), dtype=torch.int32, device=gt_dev.device)
    _C.check(_C.lib().cp_id_histogram(_C.ptr(gt_dev), H, W, _C.ptr(hist), _C.stream()), "cp_id_histogram")
    return hist.cpu().numpy().astype(np.int64)


class InstanceLevelEvaluator(object):
    """Collects the count tables image by image (add_image / add_counts) and scores them (summarize)."""

    def __init__(self, protocol=CITYSCAPES, distances=False):
        """distances: score the evaluator's three settings (all, 100 m, 50 m) instead of the first alone; every image
        then comes with its [G, 2] table of (medDist, distConf), see evaluation/distances.py."""
        self.protocol = protocol
        self.distances = bool(distances)
        self.images = []
        self.gt_dists = []                                                # per image [G, 2], or None without distances

    def settings(self):
        """(minRegionSize, distanceTh, distanceConf) of every scored setting: the first alone without distances."""
        k = len(MIN_REGION_SIZES) if self.distances else 1
        return list(zip(MIN_REGION_SIZES[:k].tolist(), DISTANCE_THS[:k].tolist(), DISTANCE_CONFS[:k].tolist()))

    def _note_distances(self, gt_table, gt_dist):
        """The distance table of the image add_counts is about to append, checked against the evaluator's mode."""
        if gt_dist is None:
            if self.distances:
                raise ValueError("this evaluator scores the distance settings: every image needs its gt_dist table "
                                 "(add_counts(..., gt_dist=), add_image(..., disparity=, camera=))")
        else:
            if not self.distances:
                raise ValueError("a distance table was given to an evaluator made with distances=False")
            gt_dist = np.asarray(gt_dist, np.float64)
            if gt_dist.shape != (len(gt_table), 2):
                raise ValueError("gt_dist is %s, the ground-truth table has %d rows: expected [%d, 2] (medDist, "
                                 "distConf)" % (gt_dist.shape, len(gt_table), len(gt_table)))
            if np.isnan(gt_dist).any():
                raise ValueError("gt_dist holds NaN")
        self.gt_dists.append(gt_dist)

    def add_counts(self, gt_table, label_ids, confidences, pred_pixels, void_inter, inter, gt_dist=None):
        """One image from its counts: gt_table [G, 3] as gt_instances returns it; per prediction its label id,
        confidence, pixel count and void overlap; inter [n, G], column j counted against gt_table[j].  Predictions
        with a label without instances or without pixels are skipped, as the protocol skips them.  The order of
        the predictions is the order of the text file's lines: the scores are sorted stably, so it can show in an AP.
        gt_dist: float64 [G, 2] (medDist, distConf) of gt_table's rows, for an evaluator with distances."""
        gt_table = np.asarray(gt_table, np.int64).reshape(-1, 3)
        self._note_distances(gt_table, gt_dist)
        inter = np.asarray(inter, np.int64).reshape(len(label_ids), len(gt_table))
        preds = []
        for i, (lab, conf) in enumerate(zip(label_ids, confidences)):
            if int(lab) not in self.protocol.label_ids or int(pred_pixels[i]) == 0:
                continue
            preds.append((int(lab), float(conf), int(pred_pixels[i]), int(void_inter[i]), inter[i]))
        self.images.append((gt_table, preds))

    def add_image(self, masks_dev, label_ids, confidences, gt_ids, disparity=None, camera=None):
        """One image from device masks uint8 [n, H, W] (any n: the kernel is called on slices of 128) and its id
        image: a host uint16 [H, W] array, or a device tensor of 16-bit elements holding those bits.  For an evaluator
        with distances: the image's disparity (host uint16 [H, W] or device tensor) and camera (baseline, fx)."""
        import torch
        if (disparity is None) != (camera is None):
            raise ValueError("disparity and camera come together")
        if (disparity is not None) != self.distances:
            raise ValueError("this evaluator scores the distance settings: add_image needs disparity and camera"
                             if self.distances else
                             "a disparity was given to an evaluator made with distances=False")
        n = int(masks_dev.shape[0])
        # (an image without predictions still has ground truth to count: on the default device)
        gt_ids = device_ids(gt_ids, masks_dev.device if n else torch.device("cuda"))
        if len(label_ids) != n or len(confidences) != n:
            raise ValueError("%d masks, %d labels, %d confidences" % (n, len(label_ids), len(confidences)))
        if tuple(masks_dev.shape[1:]) != tuple(gt_ids.shape):
            raise ValueError("masks are %s, the id image is %s" % (tuple(masks_dev.shape[1:]), tuple(gt_ids.shape)))
        table = gt_instances(device_histogram(gt_ids), self.protocol)
        G = len(table)
        inter = np.zeros((n, G), np.int64)
        void = np.zeros((n,), np.int64)
        pix = np.zeros((n,), np.int64)
        for a in range(0, n, MAX_MASKS):
            for g in range(0, max(G, 1), MAX_INST):
                i, v, p = device_counts(masks_dev[a:a + MAX_MASKS], gt_ids, table[g:g + MAX_INST, 0], self.protocol)
                inter[a:a + MAX_MASKS, g:g + MAX_INST], void[a:a + MAX_MASKS], pix[a:a + MAX_MASKS] = i, v, p
        gt_dist = None
        if disparity is not None:
            from . import distances
            gt_dist = distances.instance_distances(gt_ids, table[:, 0], disparity, camera)[0]
        self.add_counts(table, label_ids, confidences, pix, void, inter, gt_dist=gt_dist)

    def ap_matrix(self):
        """float64 [settings, labels, 10]: AP per (setting, class, overlap threshold); one setting without
        distances, three (all, 100 m, 50 m) with them."""
        settings = self.settings()
        ap = np.zeros((len(settings), len(self.protocol.label_ids), len(OVERLAPS)), np.float64)
        for di, setting in enumerate(settings):
            for oi, th in enumerate(OVERLAPS):
                for li, lab in enumerate(self.protocol.label_ids):
                    ap[di, li, oi] = self._class_ap(lab, th, setting)
        return ap

    def _overlaps(self, pred, cols, size, inter, hit):
        """The overlap of one prediction (its tuple of add_counts) with the ground truths `cols` of its class, of
        `size` pixels, sharing `inter` pixels, `hit` where inter > 0: the mask IoU.  evaluation/boundary.py overrides it."""
        return np.where(hit, inter / np.maximum(size + pred[2] - inter, 1).astype(np.float64), 0.0)

    def _class_ap(self, lab, th, setting=(MIN_REGION_SIZE, np.inf, -np.inf)):
        min_size, dist_th, dist_conf = setting
        y_true, y_score = [], []
        hard_fn = 0
        have_gt = have_pred = False
        for (table, preds), gt_dist in zip(self.images, self.gt_dists):
            cols = np.flatnonzero(table[:, 1] == lab)                      # every id of the class, groups included
            ids, size = table[cols, 0], table[cols, 2]
            out = size < min_size                                          # outside the setting: small, far or sparse
            if gt_dist is not None:
                out = out | (gt_dist[cols, 0] > dist_th) | (gt_dist[cols, 1] < dist_conf)
            real = (ids >= 1000) & ~out
            ignore = (ids < 1000).astype(np.int64) + out                    # a small group counts twice
            mine = [p for p in preds if p[0] == lab]
            have_gt |= bool(real.any())
            have_pred |= bool(mine)
            best = {}                                                       # ground truth -> score it holds
            for pred in mine:
                _, conf, pix, void, row = pred[:5]
                inter = row[cols]
                hit = inter > 0
                iou = self._overlaps(pred, cols, size, inter, hit)
                over = hit & (iou > th)
                for g in np.flatnonzero(over & real):
                    if g in best:
                        y_true.append(0.0)
                        y_score.append(min(best[g], conf))
                        best[g] = max(best[g], conf)
                    else:
                        best[g] = conf
                if not over.any():
                    if float(void + int((inter * ignore).sum())) / pix <= th:
                        y_true.append(0.0)
                        y_score.append(conf)
            hard_fn += int(real.sum()) - len(best)
            y_true.extend([1.0] * len(best))
            y_score.extend(best.values())
        if not have_gt:
            return float("nan")
        if not have_pred:
            return 0.0
        y_true, y_score = np.array(y_true, np.float64), np.array(y_score, np.float64)
        order = np.argsort(y_score, kind="stable")
        score, true = y_score[order], y_true[order]
        cum = np.append(np.cumsum(true), 0.0)                             # index -1: nothing below the first score
        _, first = np.unique(score, return_index=True)
        n_true = cum[-2] if len(true) else 0.0
        precision = np.zeros(len(first) + 1)
        recall = np.zeros(len(first) + 1)
        for k, idx in enumerate(first):
            below = cum[idx - 1]
            tp = n_true - below
            fp = len(score) - idx - tp
            fn = below + hard_fn
            precision[k] = tp / (tp + fp)
            recall[k] = tp / (tp + fn)
        precision[-1], recall[-1] = 1.0, 0.0
        steps = np.convolve(np.concatenate([recall[:1], recall, [0.0]]), [-0.5, 0, 0.5], "valid")
        return float(np.dot(precision, steps))

    def summarize(self):
        """The evaluator's dictionary (allAp, allAp50%, classes[name][ap | ap50%]) plus "resultApMatrix"; with
        distances also allAp50m, allAp100m, allAp50%50m and per class ap50m, ap100m, ap50%50m."""
        ap = self.ap_matrix()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)             # no ground truth at all: nan, not a warning
            res = {"allAp": float(np.nanmean(ap[0])), "allAp50%": float(np.nanmean(ap[0, :, 0]))}
            if self.distances:                                          # settings 1 and 2: within 100 m, within 50 m
                res.update({"allAp50m": float(np.nanmean(ap[2])), "allAp100m": float(np.nanmean(ap[1])),
                            "allAp50%50m": float(np.nanmean(ap[2, :, 0]))})
        res["classes"] = {}
        for li, name in enumerate(self.protocol.inst_labels):
            res["classes"][name] = {"ap": float(np.average(ap[0, li])), "ap50%": float(ap[0, li, 0])}
            if self.distances:
                res["classes"][name].update({"ap50m": float(np.average(ap[2, li])),
                                             "ap100m": float(np.average(ap[1, li])), "ap50%50m": float(ap[2, li, 0])})
        res["resultApMatrix"] = ap
        return res


def has_distances(res):
    """Whether a summarize() dictionary carries the distance averages."""
    return "allAp100m" in res


def results_json(res, protocol=CITYSCAPES):
    """The dictionary the evaluator writes as resultInstanceLevelSemanticLabeling.json.  With distances it gains the
    evaluator's distanceThresholds and minStereoDensities; JSON has no infinity, so the unbounded first setting is
    written as null (+inf and -inf alike: "no bound")."""
    out = {"averages": {k: v for k, v in res.items() if k != "resultApMatrix"}, "overlaps": OVERLAPS.tolist(),
           "minRegionSizes": MIN_REGION_SIZES.tolist(), "instLabels": list(protocol.inst_labels),
           "resultApMatrix": res["resultApMatrix"].tolist()}
    if has_distances(res):
        finite = lambda a: [float(v) if np.isfinite(v) else None for v in a]   # noqa: E731
        out["distanceThresholds"] = finite(DISTANCE_THS)
        out["minStereoDensities"] = finite(DISTANCE_CONFS)
    return out


DISTANCE_COLUMNS = (("AP_50m", "ap50m", "allAp50m"), ("AP_100m", "ap100m", "allAp100m"),
                    ("AP_50%50m", "ap50%50m", "allAp50%50m"))


def format_results(res, protocol=CITYSCAPES):
    """The evaluator's result table as text: 50 columns wide, 90 with the three distance columns."""
    if has_distances(res):
        lines = ["", "#" * 90, "{:<15}".format("what") + ":" + "{:>15}".format("AP") + "{:>15}".format("AP_50%")
                 + "".join("{:>15}".format(c[0]) for c in DISTANCE_COLUMNS), "#" * 90]
        for name in protocol.inst_labels:
            c = res["classes"][name]
            lines.append("{:<15}".format(name) + ":" + "{:>15.3f}".format(c["ap"]) + "{:>15.3f}".format(c["ap50%"])
                         + "".join("{:>15.3f}".format(c[k[1]]) for k in DISTANCE_COLUMNS))
        lines += ["-" * 90, "{:<15}".format("average") + ":" + "{:>15.3f}".format(res["allAp"])
                  + "{:>15.3f}".format(res["allAp50%"])
                  + "".join("{:>15.3f}".format(res[k[2]]) for k in DISTANCE_COLUMNS), ""]
        return "\n".join(lines)
    lines = ["", "#" * 50, "{:<15}".format("what") + ":" + "{:>15}".format("AP") + "{:>15}".format("AP_50%"), "#" * 50]
    for name in protocol.inst_labels:
        c = res["classes"][name]
        lines.append("{:<15}".format(name) + ":" + "{:>15.3f}".format(c["ap"]) + "{:>15.3f}".format(c["ap50%"]))
    lines += ["-" * 50, "{:<15}".format("average") + ":" + "{:>15.3f}".format(res["allAp"])
              + "{:>15.3f}".format(res["allAp50%"]), ""]
    return "\n".join(lines)


def read_pred_info(txt_path):
    """The lines `relative mask path, label id, confidence` of one result file."""
    out = []
    with open(txt_path) as f:
        for line in f:
            parts = line.split(" ")
            if len(parts) != 3:
                raise ValueError("%s: expected `maskPath labelID confidence`, got %r" % (txt_path, line))
            if os.path.isabs(parts[0]):
                raise ValueError("%s: mask paths must be relative (%s)" % (txt_path, parts[0]))
            out.append((os.path.join(os.path.dirname(txt_path), parts[0]), int(float(parts[1])), float(parts[2])))
    return out


def evaluate_result_dir(pred_dir, gt_files, device=None, protocol=CITYSCAPES, disparity_dir=None, camera_dir=None):
    """Scores a result directory in the protocol's layout (Cityscapes: `<image>*.txt` listing `masks/*.png`; KITTI:
    `<base name>.txt`; IDD: `<city>/<frame>*.txt`, both with the masks next to the text file), searched below pred_dir
    by the key of each ground-truth file.  Masks are uploaded image by image.  With disparity_dir and camera_dir
    (Cityscapes) the three distance settings are scored: every frame needs its disparity and camera file."""
    import torch
    from PIL import Image
    dev = device or torch.device("cuda")
    txts = [os.path.join(r, f) for r, _, files in os.walk(pred_dir) for f in files if f.endswith(".txt")]
    dist_files = None
    if disparity_dir or camera_dir:
        from . import distances
        if not (disparity_dir and camera_dir):
            raise ValueError("disparity_dir and camera_dir come together")
        if protocol is not CITYSCAPES:
            raise ValueError("distances are scored for cityscapes only: %s" % distances.REFUSED.get(
                {"kitti": "kitti_poly"}.get(protocol.name, protocol.name), "no disparity convention"))
        dist_files = distances.find_files(disparity_dir, camera_dir)
        for gt in gt_files:                                                # before anything is scored
            base = os.path.basename(gt)
            distances.frame_files(dist_files, protocol.gt_key("", base) or os.path.splitext(base)[0], base)
    ev = InstanceLevelEvaluator(protocol, distances=dist_files is not None)
    for gt in gt_files:
        root, base = os.path.split(gt)
        key = protocol.gt_key(root, base)
        if key is None:
            key = os.path.splitext(base)[0]
        mine = [t for t in txts if protocol.pred_match(os.path.relpath(t, pred_dir).replace(os.sep, "/"), key)]
        if len(mine) != 1:
            raise FileNotFoundError("%d prediction text files for %s below %s (ground truth %s)"
                                    % (len(mine), key, pred_dir, gt))
        ids = read_gt_ids(gt)
        info = read_pred_info(mine[0])
        info = [p for p in info if p[1] in protocol.label_ids]                      # other labels are never opened
        masks = np.zeros((len(info),) + ids.shape, np.uint8)
        for k, (path, _, _) in enumerate(info):
            m = np.array(Image.open(path).convert("L"))
            if m.shape != ids.shape:
                raise ValueError("%s is %s, the ground truth %s is %s" % (path, m.shape, gt, ids.shape))
            masks[k] = m
        extra = {}
        if dist_files is not None:
            disp_path, cam_path = distances.frame_files(dist_files, key, base)
            disp = distances.read_disparity(disp_path)
            if disp.shape != ids.shape:
                raise ValueError("%s is %s, the ground truth %s is %s" % (disp_path, disp.shape, gt, ids.shape))
            extra = {"disparity": disp, "camera": distances.read_camera(cam_path)}
        ev.add_image(torch.from_numpy(masks).to(dev), [p[1] for p in info], [p[2] for p in info], ids, **extra)
    return ev.summarize()


def evaluate_coco_results(results_json, annot_json, gt_files, device=None, protocol=CITYSCAPES):
    """Scores a COCO segm results file -- a list of {"image_id", "category_id", "score", "segmentation": {"size": [H, W],
    "counts": RLE string or list}}, made here by --save_rle or anywhere else -- with the instance-level AP.  annot_json
    (COCO annotations) gives image_id -> file_name, matched to the ground truth by the protocol's image key, and
    category_id -> name -> the protocol's label id (a category the protocol has no instances of is left out, as
    evaluate_result_dir never opens such masks).  gt_files: find_gt_files' dictionary or a list of paths; every
    ground-truth image is scored, with no prediction when the results name none.  The masks are decoded on the device
    (utils/rle.py); a segmentation whose size is not the ground truth's, or whose counts do not fill it, is a
    ValueError naming the entry."""
    import json

    import torch

    from ...utils import rle
    dev = device or torch.device("cuda")
    with open(annot_json) as f:
        annot = json.load(f)
    with open(results_json) as f:
        results = json.load(f)
    name_of = {int(c["id"]): c["name"] for c in annot.get("categories", [])}
    label_of_name = dict(zip(protocol.inst_labels, protocol.label_ids))
    key_of = {int(im["id"]): protocol.image_key(im["file_name"]) for im in annot.get("images", [])}
    per_key = {}
    for i, r in enumerate(results):
        what = "%s entry %d" % (results_json, i)
        try:
            img, cat, score, seg = int(r["image_id"]), int(r["category_id"]), float(r["score"]), r["segmentation"]
        except (KeyError, TypeError, ValueError):
            raise ValueError("%s: needs image_id, category_id, score and segmentation" % what)
        if img not in key_of:
            raise ValueError("%s: image_id %d is not in %s" % (what, img, annot_json))
        if cat not in name_of:
            raise ValueError("%s: category_id %d is not in %s" % (what, cat, annot_json))
        if name_of[cat] in label_of_name:
            per_key.setdefault(key_of[img], []).append((what, label_of_name[name_of[cat]], score, seg))
    if isinstance(gt_files, dict):
        keyed = sorted(gt_files.items())
    else:
        keyed = []
        for gt in gt_files:
            root, base = os.path.split(gt)
            key = protocol.gt_key(root, base)
            keyed.append((os.path.splitext(base)[0] if key is None else key, gt))
    ev = InstanceLevelEvaluator(protocol)
    for key, gt in keyed:
        ids = read_gt_ids(gt)
        mine = per_key.get(key, [])
        for what, _, _, seg in mine:
            size = seg.get("size") if isinstance(seg, dict) else None
            if size is None or tuple(int(v) for v in size) != tuple(ids.shape):
                raise ValueError("%s: the segmentation's size is %r, the ground truth %s is %s"
                                 % (what, size, gt, list(ids.shape)))
        if mine:
            masks, status = rle.decode([p[3] for p in mine], dev, names=[p[0] for p in mine])
            if status.any():
                raise ValueError("%s: the counts do not add up to the image's %d x %d pixels"
                                 % (mine[int(np.flatnonzero(status)[0])][0], ids.shape[0], ids.shape[1]))
        else:
            masks = torch.zeros((0,) + tuple(ids.shape), dtype=torch.uint8, device=dev)
        ev.add_image(masks, [p[1] for p in mine], [p[2] for p in mine], ids)
    return ev.summarize()

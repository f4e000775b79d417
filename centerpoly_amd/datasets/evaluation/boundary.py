"""Boundary IoU and Boundary AP of instance masks (Cheng et al., "Boundary IoU: Improving Object-Centric Image
Segmentation Evaluation", CVPR 2021), on the count tables of the instance-level protocol (instance_level.py).

Mask IoU hardly moves when the outline of a large object is cut straight across its mirrors and wheels; Boundary IoU is
the IoU of the two masks restricted to the band of width d inside their contours,
    band(M, d) = { p in M : a pixel within Chebyshev distance d of p is outside the image or not in M },
and Boundary AP is the AP protocol with min(mask IoU, boundary IoU) in place of the mask IoU.  Neither is in the
reference tree: the definition is include/centerpoly_hip.h's (cp_boundary_overlaps), the host statement is
tests/golden/boundary_host.py.  The band of a ground-truth instance is taken in the id image, against EVERY other value.

d = max(1, round(ratio * sqrt(H^2 + W^2))).  DEFAULT_RATIO = 0.005 is this project's default for its street-scene
canvases (11 pixels at 2048 x 1024, 6 at 1242 x 375); 0.02 is the value usually used for COCO-sized images.  The
kernel takes d <= 64: a ratio that asks for more on an image is refused with the numbers.

The pixel work -- the bands and three more count tables per image (b_pred, b_gt, b_inter) -- is cp_boundary_overlaps';
everything else is the mask-count protocol unchanged: the region-size filter, the void / group ignore rule on MASK
pixels, the duplicate rule and the precision / recall integration."""
import json
import math
import os
import warnings

import numpy as np

from . import instance_level as il

DEFAULT_RATIO = 0.005
COCO_RATIO = 0.02
MAX_D = 64                                               # cp_boundary_overlaps' limit
RESULT_FILE = "resultBoundaryInstanceLevel.json"
DATASETS = {"cityscapes": "cityscapes", "kitti_poly": "kitti", "IDD": "IDD"}      # --dataset -> AP protocol


def band_width(H, W, ratio=DEFAULT_RATIO):
    """d of an H x W image, in Python floats."""
    return max(1, int(round(ratio * math.sqrt(H * H + W * W))))


def checked_band_width(H, W, ratio):
    d = band_width(H, W, ratio)
    if d > MAX_D:
        raise ValueError("--boundary_ratio %g gives a band of d = %d pixels on a %d x %d image (diagonal %.1f); "
                         "cp_boundary_overlaps takes d <= %d, a ratio of at most %g here"
                         % (ratio, d, W, H, math.hypot(H, W), MAX_D, (MAX_D + 0.49) / math.hypot(H, W)))
    return d


def device_boundary_counts(masks_dev, gt_dev, inst_ids, d, bounds=None, want_bands=False):
    """cp_boundary_overlaps on device masks uint8 [n, H, W] (any n), device ids [H, W] (16-bit elements) and any number
    of ids of interest, on slices of 128 masks x 1024 ids: (b_inter [n, G], b_pred [n], b_gt [G]) as host int64 arrays.
    bounds: device int32 [n, 4] or None.  want_bands: also the device tensors (pred_bands uint8 [n, H, W], gt_band
    uint8 [H, W]), 255 / 0."""
    import ctypes

    import torch

    from ... import _C
    n, H, W = (int(v) for v in masks_dev.shape)
    inst_ids = np.asarray(list(inst_ids), np.int64).reshape(-1)
    G = len(inst_ids)
    dev = gt_dev.device
    L = _C.lib()
    b_inter, b_pred, b_gt = np.zeros((n, G), np.int64), np.zeros((n,), np.int64), np.zeros((G,), np.int64)
    pred_bands = torch.empty((n, H, W), dtype=torch.uint8, device=dev) if want_bands else None
    gt_band = torch.empty((H, W), dtype=torch.uint8, device=dev) if want_bands else None
    inst_dev = torch.from_numpy(inst_ids.astype(np.int32)).to(dev) if G else None
    at = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off) if t is not None and t.numel() else None   # noqa: E731
    for a in range(0, max(n, 1), il.MAX_MASKS):
        na = min(il.MAX_MASKS, n - a)
        for g in range(0, max(G, 1), il.MAX_INST):
            ng = min(il.MAX_INST, G - g)
            out = torch.empty((na * ng + na + ng + 1,), dtype=torch.int32, device=dev)
            nbytes = L.cp_boundary_overlaps_workspace_bytes(na, ng, H, W, d)
            ws = _C.workspace(nbytes, dev)
            _C.check(L.cp_boundary_overlaps(
                _C.ptr(masks_dev[a:a + na]) if na else None, na, _C.ptr(bounds[a:a + na]) if bounds is not None and na else None,
                _C.ptr(gt_dev), H, W, int(d), at(inst_dev, 4 * g) if ng else None, ng, at(out), at(out, 4 * na * ng),
                at(out, 4 * (na * ng + na)), at(pred_bands[a:a + na]) if want_bands and g == 0 and na else None,
                _C.ptr(gt_band) if want_bands and a == 0 and g == 0 else None, _C.ptr(ws), nbytes, _C.stream()),
                "cp_boundary_overlaps")
            host = out.cpu().numpy().astype(np.int64)
            b_inter[a:a + na, g:g + ng] = host[:na * ng].reshape(na, ng)
            b_pred[a:a + na] = host[na * ng:na * ng + na]
            b_gt[g:g + ng] = host[na * ng + na:na * ng + na + ng]
    if want_bands:
        return b_inter, b_pred, b_gt, pred_bands, gt_band
    return b_inter, b_pred, b_gt


def table_words(S, G0):
    """int32 words of the band tables of S masks and G0 ids: b_inter [S, G0], b_pred [S], b_gt [G0]."""
    return S * G0 + S + G0


def enqueue_tables(masks_dev, bounds, gt_dev, d, ids_dev, G0, out, offset):
    """cp_boundary_overlaps for score_instances_device of the writer mixins: the band tables of all S slots against the
    first G0 values of the device int32 tensor `ids_dev` go into the device int32 buffer `out` from word `offset` on
    (table_words(S, G0) words), to come back in the caller's one read."""
    import ctypes

    from ... import _C
    S, H, W = (int(v) for v in masks_dev.shape)
    L = _C.lib()
    at = lambda o: ctypes.c_void_p(out.data_ptr() + 4 * (offset + o))     # noqa: E731
    nbytes = L.cp_boundary_overlaps_workspace_bytes(S, G0, H, W, d)
    ws = _C.workspace(nbytes, masks_dev.device)
    _C.check(L.cp_boundary_overlaps(_C.ptr(masks_dev), S, _C.ptr(bounds), _C.ptr(gt_dev), H, W, int(d),
                                    _C.ptr(ids_dev) if G0 else None, G0, at(0), at(S * G0), at(S * G0 + S), None, None,
                                    _C.ptr(ws), nbytes, _C.stream()), "cp_boundary_overlaps")


def read_tables(host, offset, S, G0, n, masks_dev, bounds, gt_dev, d, gt_table):
    """The tables enqueue_tables left, from the host copy of the buffer: (b_inter int64 [n, G], b_pred [n], b_gt [G])
    of the first n slots; ids beyond the first G0 of gt_table (more than one call takes: rare) are counted here."""
    t = host[offset:offset + table_words(S, G0)].astype(np.int64)
    b_inter, b_pred, b_gt = t[:S * G0].reshape(S, G0)[:n], t[S * G0:S * G0 + S][:n], t[S * G0 + S:]
    if len(gt_table) > G0:
        more = device_boundary_counts(masks_dev, gt_dev, gt_table[G0:, 0], d, bounds)
        b_inter, b_gt = np.concatenate([b_inter, more[0][:n]], axis=1), np.concatenate([b_gt, more[2]])
    return b_inter, b_pred, b_gt


class BoundaryEvaluator(il.InstanceLevelEvaluator):
    """InstanceLevelEvaluator whose overlap of a (prediction, ground truth) pair is min(mask IoU, boundary IoU), with
    boundary IoU = b_inter / max(b_gt + b_pred - b_inter, 1) for a pair that shares a mask pixel.  Per image it keeps
    the three band tables beside the mask tables, so the same counts give the plain AP too."""

    def __init__(self, protocol=il.CITYSCAPES, ratio=DEFAULT_RATIO, distances=False):
        super(BoundaryEvaluator, self).__init__(protocol, distances)
        ratio = float(ratio)
        if not (math.isfinite(ratio) and ratio > 0):
            raise ValueError("the boundary ratio must be finite and > 0, got %r" % ratio)
        self.ratio = ratio
        self.band_widths = {}                                             # (H, W) -> d of every image size seen
        self._plain = False

    def band_width(self, H, W):
        """d of an H x W image (refused beyond the kernel's limit), noted for summarize()."""
        d = checked_band_width(int(H), int(W), self.ratio)
        self.band_widths[(int(H), int(W))] = d
        return d

    def add_counts(self, gt_table, label_ids, confidences, pred_pixels, void_inter, inter, b_pred=None, b_gt=None,
                   b_inter=None, gt_dist=None):
        """InstanceLevelEvaluator.add_counts plus the band tables of the image: b_pred [n], b_gt [G] (the band of
        gt_table[j]'s id), b_inter [n, G].  gt_dist as InstanceLevelEvaluator.add_counts takes it: with distances the
        matrix has the three settings (the printed table shows the first)."""
        if b_pred is None or b_gt is None or b_inter is None:
            raise ValueError("BoundaryEvaluator.add_counts needs b_pred, b_gt and b_inter")
        gt_table = np.asarray(gt_table, np.int64).reshape(-1, 3)
        self._note_distances(gt_table, gt_dist)
        n, G = len(label_ids), len(gt_table)
        inter = np.asarray(inter, np.int64).reshape(n, G)
        b_inter = np.asarray(b_inter, np.int64).reshape(n, G)
        b_gt = np.asarray(b_gt, np.int64).reshape(G)
        preds = []
        for i, (lab, conf) in enumerate(zip(label_ids, confidences)):
            if int(lab) not in self.protocol.label_ids or int(pred_pixels[i]) == 0:
                continue
            preds.append((int(lab), float(conf), int(pred_pixels[i]), int(void_inter[i]), inter[i], int(b_pred[i]),
                          b_inter[i], b_gt))
        self.images.append((gt_table, preds))

    def add_image(self, masks_dev, label_ids, confidences, gt_ids, bounds=None):
        """One image from device masks uint8 [n, H, W] (any n) and its id image, as InstanceLevelEvaluator.add_image
        takes them; bounds: device int32 [n, 4] of the masks, or None."""
        import torch
        n = int(masks_dev.shape[0])
        gt_ids = il.device_ids(gt_ids, masks_dev.device if n else torch.device("cuda"))
        if len(label_ids) != n or len(confidences) != n:
            raise ValueError("%d masks, %d labels, %d confidences" % (n, len(label_ids), len(confidences)))
        if tuple(masks_dev.shape[1:]) != tuple(gt_ids.shape):
            raise ValueError("masks are %s, the id image is %s" % (tuple(masks_dev.shape[1:]), tuple(gt_ids.shape)))
        d = self.band_width(*gt_ids.shape)
        table = il.gt_instances(il.device_histogram(gt_ids), self.protocol)
        G = len(table)
        inter, void, pix = np.zeros((n, G), np.int64), np.zeros((n,), np.int64), np.zeros((n,), np.int64)
        for a in range(0, n, il.MAX_MASKS):
            for g in range(0, max(G, 1), il.MAX_INST):
                i, v, p = il.device_counts(masks_dev[a:a + il.MAX_MASKS], gt_ids, table[g:g + il.MAX_INST, 0],
                                           self.protocol)
                inter[a:a + il.MAX_MASKS, g:g + il.MAX_INST], void[a:a + il.MAX_MASKS], pix[a:a + il.MAX_MASKS] = i, v, p
        b_inter, b_pred, b_gt = device_boundary_counts(masks_dev.to(gt_ids.device), gt_ids, table[:, 0], d, bounds)
        self.add_counts(table, label_ids, confidences, pix, void, inter, b_pred, b_gt, b_inter)

    def _overlaps(self, pred, cols, size, inter, hit):
        iou = super(BoundaryEvaluator, self)._overlaps(pred, cols, size, inter, hit)
        if self._plain:
            return iou
        b_pix, b_row, b_gt = pred[5:8]
        bi = b_row[cols]
        biou = bi / np.maximum(b_gt[cols] + b_pix - bi, 1).astype(np.float64)
        return np.where(hit, np.minimum(iou, biou), 0.0)

    def plain_ap_matrix(self):
        """The AP matrix of the mask IoU alone, from the same counts (InstanceLevelEvaluator's, bit for bit)."""
        self._plain = True
        try:
            return self.ap_matrix()
        finally:
            self._plain = False

    def summarize(self):
        """allBoundaryAp, allBoundaryAp50%, classes[name][bap | bap50% | ap | ap50%], the plain allAp / allAp50% beside
        them, "ratio", "bandWidths" ({"HxW": d} of every image size seen), "resultBoundaryApMatrix" and
        "resultApMatrix"."""
        bap, ap = self.ap_matrix(), self.plain_ap_matrix()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            res = {"allBoundaryAp": float(np.nanmean(bap[0])), "allBoundaryAp50%": float(np.nanmean(bap[0, :, 0])),
                   "allAp": float(np.nanmean(ap[0])), "allAp50%": float(np.nanmean(ap[0, :, 0])), "classes": {}}
        for li, name in enumerate(self.protocol.inst_labels):
            res["classes"][name] = {"bap": float(np.average(bap[0, li])), "bap50%": float(bap[0, li, 0]),
                                    "ap": float(np.average(ap[0, li])), "ap50%": float(ap[0, li, 0])}
        res["ratio"] = self.ratio
        res["bandWidths"] = {"%dx%d" % hw: d for hw, d in sorted(self.band_widths.items())}
        res["resultBoundaryApMatrix"], res["resultApMatrix"] = bap, ap
        return res


def results_json(res, protocol=il.CITYSCAPES):
    """The dictionary write_results writes."""
    matrices = ("resultBoundaryApMatrix", "resultApMatrix")
    out = {"averages": {k: v for k, v in res.items() if k not in matrices}, "overlaps": il.OVERLAPS.tolist(),
           "minRegionSizes": il.MIN_REGION_SIZES.tolist(), "instLabels": list(protocol.inst_labels)}
    for k in matrices:
        out[k] = np.asarray(res[k]).tolist()
    return out


def format_results(res, protocol=il.CITYSCAPES):
    """The Boundary AP table as text, the plain AP beside it."""
    head = "{:<15}".format("what") + ":" + "".join("{:>13}".format(h) for h in ("bAP", "bAP_50%", "AP", "AP_50%"))
    lines = ["", "#" * 68, head, "#" * 68]
    for name in protocol.inst_labels:
        c = res["classes"][name]
        lines.append("{:<15}".format(name) + ":" + "".join("{:>13.3f}".format(c[k]) for k in ("bap", "bap50%", "ap", "ap50%")))
    lines += ["-" * 68, "{:<15}".format("average") + ":" + "".join(
        "{:>13.3f}".format(res[k]) for k in ("allBoundaryAp", "allBoundaryAp50%", "allAp", "allAp50%")),
        "boundary ratio %g: band width %s" % (res["ratio"], ", ".join(
            "%d px at %s" % (d, hw) for hw, d in res["bandWidths"].items()) or "no image seen"), ""]
    return "\n".join(lines)


def write_results(res, out_dir, protocol=il.CITYSCAPES):
    """resultBoundaryInstanceLevel.json in out_dir; returns its path."""
    os.makedirs(out_dir, exist_ok=True)
    path = os.path.join(out_dir, RESULT_FILE)
    with open(path, "w") as f:
        json.dump(results_json(res, protocol), f, indent=4)
    return path


def evaluate_result_dir(pred_dir, gt_files, protocol=il.CITYSCAPES, ratio=DEFAULT_RATIO, device=None):
    """Scores a result directory in the protocol's layout, as instance_level.evaluate_result_dir finds and reads it:
    mask files made anywhere, uploaded image by image.  Returns BoundaryEvaluator.summarize()."""
    import torch
    from PIL import Image
    dev = device or torch.device("cuda")
    txts = [os.path.join(r, f) for r, _, files in os.walk(pred_dir) for f in files if f.endswith(".txt")]
    ev = BoundaryEvaluator(protocol, ratio)
    for gt in gt_files:
        root, base = os.path.split(gt)
        key = protocol.gt_key(root, base)
        if key is None:
            key = os.path.splitext(base)[0]
        mine = [t for t in txts if protocol.pred_match(os.path.relpath(t, pred_dir).replace(os.sep, "/"), key)]
        if len(mine) != 1:
            raise FileNotFoundError("%d prediction text files for %s below %s (ground truth %s)"
                                    % (len(mine), key, pred_dir, gt))
        ids = il.read_gt_ids(gt)
        info = [p for p in il.read_pred_info(mine[0]) if p[1] in protocol.label_ids]
        masks = np.zeros((len(info),) + ids.shape, np.uint8)
        for k, (path, _, _) in enumerate(info):
            m = np.array(Image.open(path).convert("L"))
            if m.shape != ids.shape:
                raise ValueError("%s is %s, the ground truth %s is %s" % (path, m.shape, gt, ids.shape))
            masks[k] = m
        ev.add_image(torch.from_numpy(masks).to(dev), [p[1] for p in info], [p[2] for p in info], ids)
    return ev.summarize()

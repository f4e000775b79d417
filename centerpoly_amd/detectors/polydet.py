"""PolydetDetector (reference: src/lib/detectors/polydet.py:21-100)."""
import time

import numpy as np
import torch

from ..external.nms import MASK_NMS_METHODS, soft_nms
from ..models.decode import polydet_decode
from ..models.utils import flip_tensor
from .. import _C
from ..utils.post_process import _inverse_transforms, polydet_post_process_device
from .base_detector import BaseDetector


class PolydetDetector(BaseDetector):
    # Several test scales or --nms: merge the scales and run soft-nms on the device (merge_outputs_device) instead of
    # copying every scale back for merge_outputs on the host.  The two give the same `results`, bit for bit.  Measured on
    # one MI355X (tools/probe_merge.py, profiles/probe_merge.json; K = 128, rows in two classes) the rows reach the
    # device table in 0.306 ms with it against 0.368 ms without at two scales, 0.489 against 0.529 ms at three.  The
    # classes run side by side on the device: with EVERY row in one class (an untrained network) the host is ahead,
    # 0.349 against 0.364 ms and 0.529 against 0.581 ms.
    device_merge = True
    _slot, _merged = 0, False
    _batch = None                                    # the last run_batch's per-image rows and results (None after run)

    # --mask_nms: the scales always stay on the device and merge_outputs_device calls cp_merge_detections_mask (whole
    # rows, per class, by the IoU of the polygons' masks on the image's canvas) instead of the literal merge; there is no
    # host path for it, and device_merge does not apply.
    mask_nms = False                                 # set by the constructor
    _mask_ws = None                                  # ... its workspace, kept from image to image

    def __init__(self, opt):
        # --mask_nms has no host merge to fall back to: its limits are checked before anything is built
        if getattr(opt, "mask_nms", False) and (len(opt.test_scales) * opt.K > 1024 or opt.num_classes > 64):
            raise ValueError("--mask_nms merges at most 1024 rows of at most 64 classes on the device: %d scales x "
                             "K = %d give %d rows, num_classes = %d"
                             % (len(opt.test_scales), opt.K, len(opt.test_scales) * opt.K, opt.num_classes))
        super(PolydetDetector, self).__init__(opt)
        self.mask_nms = bool(getattr(opt, "mask_nms", False))

    def process(self, images, return_time=False):
        with torch.no_grad():
            output = self.model(images)[-1]
            hm = output["hm"].sigmoid_()             # inference: no clamp (reference :28)
            polys = output["poly"]
            pseudo_depth = output["pseudo_depth"]
            reg = output["reg"] if self.opt.reg_offset else None
            if self.opt.flip_test:
                n = hm.shape[0] // 2                 # all originals, then all flipped copies (run: n = 1)
                hm = (hm[:n] + flip_tensor(hm[n:])) / 2
                reg = reg[:n] if reg is not None else None
                polys, pseudo_depth = polys[:n], pseudo_depth[:n]
            torch.cuda.synchronize()
            forward_time = time.time()
            dets = polydet_decode(hm, polys, pseudo_depth, reg=reg,
                                  cat_spec_poly=self.opt.cat_spec_poly, K=self.opt.K,
                                  rep=self.opt.rep)
        if return_time:
            return output, dets, forward_time
        return output, dets

    def run(self, image_or_path_or_tensor, id=1, meta=None):
        self._slot = 0                               # the scale post_process writes next (device merge)
        self._merged = False
        self._batch = None
        return super(PolydetDetector, self).run(image_or_path_or_tensor, id, meta)

    def run_batch(self, images):
        self._slot = 0
        self._merged = False
        self._batch = None
        return super(PolydetDetector, self).run_batch(images)

    def _merge_on_device(self, K):
        """Several scales or --nms (the settings in which merge_outputs does real work), the switch on and the rows
        within the limits of cp_merge_detections; beyond them merge_outputs on the host remains.  --mask_nms: always
        (one scale included; the constructor has checked its limits)."""
        if self.mask_nms:
            return True
        return (self.device_merge and (len(self.scales) > 1 or self.opt.nms)
                and len(self.scales) * K <= 4096 and self.num_classes <= 64)

    def post_process(self, dets, meta, scale=1, fg=None):
        dets = dets.detach().reshape(1, -1, dets.shape[2])
        if self._merge_on_device(dets.shape[1]):
            # transform_preds + `/ scale` into this scale's slot of one device buffer [S, K, ncols]: no copy back
            dets = dets.contiguous()
            S, (_, K, ncols) = len(self.scales), dets.shape
            if self._slot >= S or self._slot == 0:
                self._slot = 0
                self.scale_rows = torch.empty((S, K, ncols), dtype=torch.float32, device=dets.device)
            if tuple(self.scale_rows.shape) != (S, K, ncols):
                raise ValueError("the test scales differ in the shape of their detections")
            trans = _inverse_transforms([meta["c"]], [meta["s"]], meta["out_height"], meta["out_width"], dets.device)
            _C.check(_C.lib().cp_polydet_post_process(_C.ptr(dets), _C.ptr(trans), float(scale), 1, K, ncols,
                                                      _C.ptr(self.scale_rows[self._slot]), _C.stream()),
                     "cp_polydet_post_process")
            self._slot += 1
            return None                              # merge() reads the buffer
        # transform_preds + `/ scale` on the device, one copy back, class split on the host
        ret, rows, host = polydet_post_process_device(dets, [meta["c"]], [meta["s"]], meta["out_height"],
                                                      meta["out_width"], self.opt.num_classes, scale,
                                                      return_device=True, return_host=True)
        self.rows_dev = rows[0]                      # the same rows, still on the device (see device_rows)
        self.rows_host = host[0]                     # ... and as they were copied back, class column included
        return ret[0]

    def post_process_batch(self, dets, metas, scale=1):
        """post_process for a batch: dets [B, K, ncols], one meta per image.  One cp_polydet_post_process launch with
        the B inverse maps either way.  One scale without --nms: one device -> host copy of [B, K, ncols], the class
        split per image (returns the list of per-image dicts).  Several scales or --nms: the rows go into this
        scale's slot of a [B, S, K, ncols] device buffer, image b's scales contiguous for cp_merge_detections
        (returns None; merge_batch reads the buffer)."""
        dets = dets.detach().contiguous()
        B, K, ncols = dets.shape
        c, s = [m["c"] for m in metas], [m["s"] for m in metas]
        h, w = metas[0]["out_height"], metas[0]["out_width"]
        if self._merge_on_device(K):
            S = len(self.scales)
            if self._slot >= S or self._slot == 0:
                self._slot = 0
                self.scale_rows = torch.empty((B, S, K, ncols), dtype=torch.float32, device=dets.device)
            if tuple(self.scale_rows.shape) != (B, S, K, ncols):
                raise ValueError("the test scales differ in the shape of their detections")
            rows = torch.empty_like(dets)
            trans = _inverse_transforms(c, s, h, w, dets.device)
            _C.check(_C.lib().cp_polydet_post_process(_C.ptr(dets), _C.ptr(trans), float(scale), B, K, ncols,
                                                      _C.ptr(rows), _C.stream()), "cp_polydet_post_process")
            self.scale_rows[:, self._slot].copy_(rows)
            self._slot += 1
            return None
        ret, rows, host = polydet_post_process_device(dets, c, s, h, w, self.opt.num_classes, scale,
                                                      return_device=True, return_host=True)
        self._batch = {"rows_dev": list(rows), "rows_host": list(host), "results": None}
        return ret

    def _image_rows(self, results, image):
        """(rows kept by the last run / run_batch for `image` or None, the results to build them from otherwise)."""
        kept = (len(self.scales) == 1 and not self.opt.nms) or self._merged
        if self._batch is None:
            if image != 0:
                raise IndexError("image %d: the last call was run(), which holds one image" % image)
            return ((self.rows_dev, self.rows_host) if kept else None), results
        if not 0 <= image < len(self._batch["results"]):
            raise IndexError("image %d: the last run_batch held %d images" % (image, len(self._batch["results"])))
        if kept:
            return (self._batch["rows_dev"][image], self._batch["rows_host"][image]), results
        return None, (results if results is not None else self._batch["results"][image])

    def device_rows(self, results=None, image=0):
        """The detections of the last run() as device rows [R, 2N+7] (x1,y1,x2,y2,score,cls,poly,depth), what
        CityscapesWriterMixin.score_instances_device reads.  One scale without --nms: the rows post_process left
        on the device, no copy.  Several scales or --nms: the table merge_outputs_device left there, no copy; where
        merge_outputs ran on the host instead (device_merge off, or beyond its limits), its `results` are uploaded.
        After run_batch: the same for image `image` of the batch (`results` defaults to that image's)."""
        kept, results = self._image_rows(results, image)
        if kept is not None:
            return kept[0]
        rows = [np.concatenate([r[:, :5], np.full((len(r), 1), j - 1, np.float32), r[:, 5:]], axis=1)
                for j, r in sorted(results.items())]
        return torch.from_numpy(np.ascontiguousarray(np.concatenate(rows, axis=0), np.float32)).to(self.opt.device)

    def host_rows(self, results=None, image=0):
        """The rows of device_rows on the host, row for row (the labels of the overlay are made from them)."""
        kept, results = self._image_rows(results, image)
        if kept is not None:
            return kept[1]
        rows = [np.concatenate([r[:, :5], np.full((len(r), 1), j - 1, np.float32), r[:, 5:]], axis=1)
                for j, r in sorted(results.items())]
        return np.ascontiguousarray(np.concatenate(rows, axis=0), np.float32)

    def instances(self, results=None, image=0, thresh=None, canvas=None):
        """The instance maps (detectors/instances.py: who owns each pixel, id and label images, masks, the table) of
        image `image` of the last run() / run_batch(), drawn by the writer of --dataset on `canvas` (width, height; by
        default the size of that image) with the detections above `thresh` (by default --thresh).  Works on
        device_rows, so after several test scales or --nms as well."""
        from ..datasets.dataset_factory import dataset_factory
        from .instances import instance_maps
        rows = self.device_rows(results, image)
        if canvas is None:
            if not 0 <= image < len(self.image_sizes):
                raise IndexError("image %d: the last call held %d images" % (image, len(self.image_sizes)))
            canvas = self.image_sizes[image]
        if self.opt.dataset not in dataset_factory:
            raise KeyError("dataset %r is not registered (have: %s)" % (self.opt.dataset, sorted(dataset_factory)))
        return instance_maps(rows, dataset_factory[self.opt.dataset], canvas,
                             self.opt.thresh if thresh is None else thresh)

    def debug(self, debugger, images, dets, output, scale=1):
        """pred_hm_<scale>: the class heat maps over the network input; out_pred_<scale>: the network input with
        the boxes of the centres above --center_thresh, in network-input coordinates (reference :78-91)."""
        hm_id, out_id = "pred_hm_{:.1f}".format(scale), "out_pred_{:.1f}".format(scale)
        mean, std = self.mean.reshape(3), self.std.reshape(3)
        debugger.add_blend_img(images[0], output["hm"][0], mean, std, img_id=hm_id)
        debugger.add_blend_img(images[0], None, mean, std, img_id=out_id)       # the de-normalised input alone
        rows = dets[0].detach().clone()
        rows[:, :4] *= self.opt.down_ratio
        debugger.add_polydet_detections(rows, rows.cpu().numpy(), self.opt.center_thresh, img_id=out_id,
                                        boxes_only=True)

    def show_results(self, debugger, image, results):
        """The picture `polydet`: box, polygon and label of every detection above --vis_thresh, drawn on the
        device from the rows post_process left there (reference :93-100).  Returns the picture's id."""
        debugger.add_img(image, img_id="polydet")
        debugger.add_polydet_detections(self.device_rows(results), self.host_rows(results), self.opt.vis_thresh,
                                        img_id="polydet")
        return "polydet"

    def merge(self, detections):
        if self._slot > 0:                           # post_process left the scales on the device
            return self.merge_outputs_device()
        return self.merge_outputs(detections)

    def merge_batch(self, detections):
        """One `results` dict per image of the batch: cp_merge_detections on image b's contiguous [S, K, ncols] slice
        where post_process_batch left the scales on the device, merge_outputs on the host otherwise."""
        if self._slot > 0:
            kept = {"rows_dev": [], "rows_host": [], "results": []}
            for b, rows in enumerate(self.scale_rows):
                kept["results"].append(self.merge_outputs_device(rows, image=b))
                kept["rows_dev"].append(self.rows_dev)
                kept["rows_host"].append(self.rows_host)
            self._batch = kept
            return kept["results"]
        results = [self.merge_outputs([d[b] for d in detections]) for b in range(len(detections[0]))]
        if self._batch is None:                      # the host merge of several scales or --nms: nothing kept per image
            self._batch = {"rows_dev": None, "rows_host": None, "results": results}
        self._batch["results"] = results
        return results

    def merge_outputs_device(self, rows=None, image=0):
        """merge_outputs on the rows post_process left on the device (cp_merge_detections: the class split, soft-nms
        and the max_per_image cut, literal behaviour), then ONE device -> host copy of the table and its counts, from
        which the `results` of run() are cut: the same keys, shapes and bits as merge_outputs gives.  The table stays
        on the device for device_rows.  `rows`: one image's [S, K, ncols] slice of a batch (merge_batch).
        --mask_nms: cp_merge_detections_mask instead, on the canvas of image `image` (self.image_sizes): whole rows,
        per class, by the IoU of the polygons' masks (--mask_nms_method; sigma 0.5, Nt 0.5, threshold 0.001)."""
        rows, C = self.scale_rows if rows is None else rows, self.num_classes
        S, K, ncols = rows.shape
        self._slot = 0
        lib = _C.lib()
        blob = torch.empty(S * K * ncols + 1 + C, dtype=torch.float32, device=rows.device)    # the table, then the counts
        out, counts = blob[:S * K * ncols].view(S * K, ncols), blob[S * K * ncols:].view(torch.int32)
        if self.mask_nms:
            W, H = self.image_sizes[image]
            need = lib.cp_merge_detections_mask_workspace_bytes(S, K, ncols, C, H, W)
            if need == 0:
                raise ValueError("--mask_nms cannot merge rows [%d, %d, %d] of %d classes on a %d x %d canvas"
                                 % (S, K, ncols, C, W, H))
            if self._mask_ws is None or self._mask_ws.numel() < need or self._mask_ws.device != rows.device:
                self._mask_ws = _C.workspace(need, rows.device)
            _C.check(lib.cp_merge_detections_mask(_C.ptr(rows), S, K, ncols, C, self.max_per_image, 1, 0.5, 0.5, 0.001,
                                                  MASK_NMS_METHODS[getattr(self.opt, "mask_nms_method", "gaussian")],
                                                  H, W, _C.ptr(out), _C.ptr(counts), _C.ptr(self._mask_ws),
                                                  self._mask_ws.numel(), _C.stream()), "cp_merge_detections_mask")
        else:
            ws = _C.workspace(lib.cp_merge_detections_workspace_bytes(S, K, ncols, C), rows.device)
            _C.check(lib.cp_merge_detections(_C.ptr(rows), S, K, ncols, C, self.max_per_image, 1, 0.5, 0.5, 0.001, 2,
                                             _C.ptr(out), _C.ptr(counts), _C.ptr(ws), ws.numel(), _C.stream()),
                     "cp_merge_detections")
        host = blob.cpu().numpy()
        n = host[S * K * ncols:].view(np.int32)
        table = host[:int(n[0]) * ncols].reshape(-1, ncols)
        self.rows_dev, self.rows_host, self._merged = out[:int(n[0])], table, True
        results, first = {}, 0
        for j in range(1, C + 1):
            r = table[first:first + int(n[j])]
            results[j] = np.concatenate([r[:, :5], r[:, 6:]], axis=1)
            first += int(n[j])
        return results

    def merge_outputs(self, detections):
        results = {}
        for j in range(1, self.num_classes + 1):
            results[j] = np.concatenate([d[j] for d in detections], axis=0).astype(np.float32)
            if len(self.scales) > 1 or self.opt.nms:
                soft_nms(results[j], Nt=0.5, method=2)
        scores = np.hstack([results[j][:, 4] for j in range(1, self.num_classes + 1)])
        if len(scores) > self.max_per_image:
            kth = len(scores) - self.max_per_image
            thresh = np.partition(scores, kth)[kth]
            for j in range(1, self.num_classes + 1):
                results[j] = results[j][results[j][:, 4] >= thresh]
        return results

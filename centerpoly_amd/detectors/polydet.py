"""PolydetDetector (reference: src/lib/detectors/polydet.py:21-100)."""
import time

import numpy as np
import torch

from ..external.nms import soft_nms
from ..models.decode import polydet_decode
from ..models.utils import flip_tensor
from ..utils.post_process import polydet_post_process_device
from .base_detector import BaseDetector


class PolydetDetector(BaseDetector):
    def __init__(self, opt):
        super(PolydetDetector, self).__init__(opt)

    def process(self, images, return_time=False):
        with torch.no_grad():
            output = self.model(images)[-1]
            hm = output["hm"].sigmoid_()             # inference: no clamp (reference :28)
            polys = output["poly"]
            pseudo_depth = output["pseudo_depth"]
            reg = output["reg"] if self.opt.reg_offset else None
            if self.opt.flip_test:
                hm = (hm[0:1] + flip_tensor(hm[1:2])) / 2
                reg = reg[0:1] if reg is not None else None
                polys, pseudo_depth = polys[0:1], pseudo_depth[0:1]
            torch.cuda.synchronize()
            forward_time = time.time()
            dets = polydet_decode(hm, polys, pseudo_depth, reg=reg,
                                  cat_spec_poly=self.opt.cat_spec_poly, K=self.opt.K,
                                  rep=self.opt.rep)
        if return_time:
            return output, dets, forward_time
        return output, dets

    def post_process(self, dets, meta, scale=1, fg=None):
        # transform_preds + `/ scale` on the device, one copy back, class split on the host
        dets = dets.detach().reshape(1, -1, dets.shape[2])
        ret, rows, host = polydet_post_process_device(dets, [meta["c"]], [meta["s"]], meta["out_height"],
                                                      meta["out_width"], self.opt.num_classes, scale,
                                                      return_device=True, return_host=True)
        self.rows_dev = rows[0]                      # the same rows, still on the device (see device_rows)
        self.rows_host = host[0]                     # ... and as they were copied back, class column included
        return ret[0]

    def device_rows(self, results=None):
        """The detections of the last run() as device rows [R, 2N+7] (x1,y1,x2,y2,score,cls,poly,depth), what
        CityscapesWriterMixin.score_instances_device reads.  One scale without --nms: the rows post_process left
        on the device, no copy.  Otherwise merge_outputs ran on the host: its `results` are uploaded."""
        if len(self.scales) == 1 and not self.opt.nms:
            return self.rows_dev
        rows = [np.concatenate([r[:, :5], np.full((len(r), 1), j - 1, np.float32), r[:, 5:]], axis=1)
                for j, r in sorted(results.items())]
        return torch.from_numpy(np.ascontiguousarray(np.concatenate(rows, axis=0), np.float32)).to(self.opt.device)

    def host_rows(self, results=None):
        """The rows of device_rows on the host, row for row (the labels of the overlay are made from them)."""
        if len(self.scales) == 1 and not self.opt.nms:
            return self.rows_host
        rows = [np.concatenate([r[:, :5], np.full((len(r), 1), j - 1, np.float32), r[:, 5:]], axis=1)
                for j, r in sorted(results.items())]
        return np.ascontiguousarray(np.concatenate(rows, axis=0), np.float32)

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

"""Synthetic Cityscapes-shaped polydet dataset: items are regenerated from a counter-based hash
(centerpoly_amd.synth), with the keys PolydetLoss and save_result consume."""
import numpy as np
import torch.utils.data as data

from .. import synth


class SyntheticPolydet(data.Dataset):
    num_classes = 8                                   # cityscapes.py:41-43
    default_resolution = [512, 1024]                  # cityscapes.py:45
    mean = np.array([0.284, 0.323, 0.282], dtype=np.float32).reshape(1, 1, 3)
    std = np.array([0.04, 0.04, 0.04], dtype=np.float32).reshape(1, 1, 3)
    max_objs = 128                                    # cityscapes.py:87

    def __init__(self, opt, split):
        if getattr(opt, "elliptical_gt", False) and not getattr(opt, "device_targets", False):
            raise ValueError("--elliptical_gt on the synthetic dataset needs --device_targets: its host targets "
                             "(synth.train_batch) are UMich Gaussians only")
        self.opt = opt
        self.split = split
        self.num_samples = getattr(opt, "synthetic_samples", 64 if split == "train" else 8)
        print("Loaded synthetic %s split: %d samples" % (split, self.num_samples))

    def __len__(self):
        return self.num_samples

    def _raw_item(self, index):
        """--device_targets: raw annotations + the crop/flip of the reference's sampler
        (sample/polydet.py:88-130), packed for cp_polydet_targets; no target arithmetic here."""
        from ..utils.image import get_affine_transform
        from .sample.polydet import pack_annotations
        opt = self.opt
        tag = "%s/raw/%d" % (self.split, index)
        img_h, img_w = opt.input_h, opt.input_w
        anns = synth.raw_annotations(tag, img_h, img_w, nbr_points=opt.nbr_points, num_classes=self.num_classes)
        c = np.array([img_w / 2.0, img_h / 2.0], dtype=np.float32)
        s = max(img_h, img_w) * 1.0
        flipped = False
        if self.split == "train":
            u = synth.uniform(tag + "/aug", (4,))
            s = s * float(np.arange(0.6, 1.4, 0.1)[int(u[0] * 8) % 8])
            c[0] = np.float32(int(img_w * (0.25 + 0.5 * u[1])))
            c[1] = np.float32(int(img_h * (0.25 + 0.5 * u[2])))
            if u[3] < 0.5:
                flipped = True
                c[0] = img_w - c[0] - 1
        h, w = opt.input_h // opt.down_ratio, opt.input_w // opt.down_ratio
        item = pack_annotations(anns, get_affine_transform(c, s, 0, [w, h]), flipped, img_w,
                                self.max_objs, opt.nbr_points)
        item["input"] = synth.normal(tag + "/input", (3, opt.input_h, opt.input_w))
        if self.split != "train":
            item["meta"] = {"c": c, "s": np.float32(s), "img_id": index, "out_height": h, "out_width": w}
        return item

    def __getitem__(self, index):
        opt = self.opt
        if getattr(opt, "device_targets", False):
            return self._raw_item(index)
        h, w = opt.input_h // opt.down_ratio, opt.input_w // opt.down_ratio
        b = synth.train_batch(1, h, w, nbr_points=opt.nbr_points, num_classes=self.num_classes,
                              max_objs=self.max_objs, rep=opt.rep,
                              stream="%s/%d" % (self.split, index), in_h=opt.input_h, in_w=opt.input_w)
        item = {k: v[0] for k, v in b.items()}
        item["freq_mask"] = np.float32(1.0)
        if self.split != "train":
            item["meta"] = {"c": np.array([opt.input_w / 2.0, opt.input_h / 2.0], dtype=np.float32),
                            "s": np.float32(max(opt.input_h, opt.input_w)), "img_id": index,
                            "out_height": h, "out_width": w}
        return item

    def run_eval(self, results, save_dir):
        """No ground-truth images offline: report the detection count instead of Cityscapes AP
        (reference: cityscapes.py:400-432 runs the vendored evaluator on the real dataset)."""
        n = sum(len(v) for r in results.values() for v in r.values())
        print("synthetic eval: %d images, %d detections (AP needs the real dataset)" % (len(results), n))
        return 0.0

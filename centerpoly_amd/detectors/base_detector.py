"""BaseDetector (reference: src/lib/detectors/base_detector.py:18-191).

Same surface: BaseDetector(opt); .pre_process(image, scale, meta) -> (images, meta);
.run(image_or_path_or_tensor) -> {'results', 'tot','load','pre','net','dec','post','merge'}.
The accelerated path is GPU-only: opt.gpus = [-1] raises instead of silently
running on the host.  cv2 is not required: the 8-bit image is uploaded as is and
the affine warp + normalisation of pre_process run in one HIP kernel with OpenCV's
fixed-point arithmetic (cp_preprocess_warp_normalize), a .npy path or ndarray is
accepted as the image source, and `opt.load_model == ''` keeps the random
initialisation (the reference calls torch.load unconditionally, :27).  An image file
path is read through PIL into cv2.imread's layout (8-bit BGR).

--debug >= 1 (reference :108-109, 145-146, 186-187): run() draws the detections on the
device (utils/debugger.py), writes the pictures into opt.debug_dir and returns the
overlay as ret['vis']; at --debug 0 no Debugger exists and nothing else changes.

Beyond the reference: .run_batch(images) sends a list of images through the network together
(.pre_process_batch: one cp_preprocess_warp_normalize_batch launch for the whole list) and
returns run()'s dict with one `results` entry per image and 'n' (DESIGN 4.26).
"""
import os
import time

import numpy as np
import torch

from ..models.model import create_model, load_model
from ..utils.image import get_affine_transform, warp_affine_normalize, warp_affine_normalize_batch


def read_image_bgr(path):
    """An image file as cv2.imread gives it: 8-bit BGR [H, W, 3] (datasets/dataset/polygons.py reads the same way)."""
    from PIL import Image
    with Image.open(path) as im:
        return np.ascontiguousarray(np.asarray(im.convert("RGB"))[:, :, ::-1])


def load_image(path):
    """What run() makes of a path: a .npy file is the array itself, anything else an image file."""
    return np.load(path) if path.lower().endswith(".npy") else read_image_bgr(path)


def class_names(opt):
    """The names the labels show: the data set's class_name without the background entry (the Cityscapes names for
    a set that has none, c<k> beyond them)."""
    from ..datasets.dataset.polygons import PolygonDataset
    from ..datasets.dataset_factory import dataset_factory
    names = getattr(dataset_factory.get(getattr(opt, "dataset", None)), "class_name", PolygonDataset.class_name)[1:]
    return [names[k] if k < len(names) else "c%d" % k for k in range(opt.num_classes)]


def _resize_bilinear_u8(img_dev, new_w, new_h):
    """cv2.resize stand-in for --test_scales != 1 (device, bilinear, result rounded back to 8 bits;
    OpenCV's fixed-point resize can differ from it by one grey level)."""
    t = img_dev.permute(2, 0, 1)[None].float()
    t = torch.nn.functional.interpolate(t, size=(new_h, new_w), mode="bilinear", align_corners=False)
    return t[0].permute(1, 2, 0).round_().clamp_(0, 255).to(torch.uint8).contiguous()


class BaseDetector(object):
    def __init__(self, opt):
        if getattr(opt, "debug", 0) == 3:
            raise ValueError("--debug 3 shows the pictures with matplotlib, which is not available here: use --debug 1, "
                             "2 or 4 (PNG files in the experiment's debug directory)")
        if opt.gpus[0] < 0:
            raise RuntimeError("centerpoly_amd detectors run on a HIP device only (--gpus -1 "
                               "has no CPU fallback)")
        opt.device = torch.device("cuda")
        print("Creating model...")
        self.model = create_model(opt.arch, opt.heads, opt.head_conv)
        if getattr(opt, "load_model", ""):
            self.model = load_model(self.model, opt.load_model)
        self.model = self.model.to(opt.device)
        self.model.eval()
        if hasattr(self.model, "prepare_inference"):
            self.model.prepare_inference()      # BN folded into convs / the DCN epilogue
        self.mean = np.array(opt.mean, dtype=np.float32).reshape(1, 1, 3)
        self.std = np.array(opt.std, dtype=np.float32).reshape(1, 1, 3)
        self.max_per_image = opt.K
        self.num_classes = opt.num_classes
        self.scales = opt.test_scales
        self.opt = opt
        self.pause = True
        self.debugger = None                                 # made at the first run() with --debug >= 1, then kept
        self.image_sizes = []                                # (width, height) per image of the last run() / run_batch()

    def _input_geometry(self, height, width, scale):
        """(new_height, new_width, inp_height, inp_width, c, s, trans_input) of an image of height x width at a test
        scale (reference :66-83)."""
        new_height, new_width = int(height * scale), int(width * scale)
        if self.opt.fix_res:
            inp_height, inp_width = self.opt.input_h, self.opt.input_w
            c = np.array([new_width / 2.0, new_height / 2.0], dtype=np.float32)
            s = max(height, width) * 1.0
        else:
            inp_height = (new_height | self.opt.pad) + 1
            inp_width = (new_width | self.opt.pad) + 1
            c = np.array([new_width // 2, new_height // 2], dtype=np.float32)
            s = np.array([inp_width, inp_height], dtype=np.float32)
        trans_input = get_affine_transform(c, s, 0, [inp_width, inp_height])
        return new_height, new_width, inp_height, inp_width, c, s, trans_input

    def pre_process(self, image, scale, meta=None):
        height, width = image.shape[0:2]
        new_height, new_width, inp_height, inp_width, c, s, trans_input = self._input_geometry(height, width, scale)
        src = self._upload(image)
        if (new_height, new_width) != (height, width):
            src = _resize_bilinear_u8(src, new_width, new_height)
        images = warp_affine_normalize(src, trans_input, self.mean, self.std, inp_height, inp_width,
                                       flip_copy=bool(self.opt.flip_test))
        meta = {"c": c, "s": s, "out_height": inp_height // self.opt.down_ratio,
                "out_width": inp_width // self.opt.down_ratio}
        return images, meta

    def pre_process_batch(self, images, scale):
        """pre_process for a list of 8-bit images in one launch: ([(1 + flip_test) * B, 3, inp_h, inp_w], [meta per
        image]), all originals first, then all flipped copies.  Every image is uploaded into its slice of one device
        buffer (no host-side concatenation) and warped by cp_preprocess_warp_normalize_batch with its own c, s and
        trans_input, the ones pre_process computes.  The images of a batch must share (inp_height, inp_width): always
        under --fix_res, under --keep_res only for equal source sizes (ValueError otherwise, before any launch)."""
        for image in images:
            self._check_image(image)
        geo = [self._input_geometry(im.shape[0], im.shape[1], scale) for im in images]
        if not geo:
            raise ValueError("pre_process_batch needs at least one image")
        if len(set(g[2:4] for g in geo)) > 1:
            raise ValueError("the images of a batch must give one network input size; sources %s give inputs %s "
                             "(--keep_res batches need equal source sizes)"
                             % ([tuple(im.shape[:2]) for im in images], [g[2:4] for g in geo]))
        inp_height, inp_width = geo[0][2:4]
        hw = np.array([g[0:2] for g in geo], dtype=np.int32)
        sizes = hw[:, 0].astype(np.int64) * hw[:, 1] * 3
        offset = np.cumsum(sizes) - sizes
        flat = torch.empty(int(sizes.sum()), dtype=torch.uint8, device=self.opt.device)
        for image, g, off, n in zip(images, geo, offset, sizes):
            dst = flat[int(off): int(off + n)]
            if tuple(g[0:2]) != tuple(image.shape[0:2]):
                dst.copy_(_resize_bilinear_u8(self._upload(image), g[1], g[0]).view(-1))
            else:
                dst.copy_(torch.from_numpy(np.ascontiguousarray(image).reshape(-1)))
        out = warp_affine_normalize_batch(flat, hw, offset, np.stack([g[6].reshape(6) for g in geo]), self.mean,
                                          self.std, inp_height, inp_width, flip_copy=bool(self.opt.flip_test))
        metas = [{"c": g[4], "s": g[5], "out_height": inp_height // self.opt.down_ratio,
                  "out_width": inp_width // self.opt.down_ratio} for g in geo]
        return out, metas

    @staticmethod
    def _check_image(image):
        if image.dtype != np.uint8 or image.ndim != 3 or image.shape[2] != 3:
            raise TypeError("pre_process needs an 8-bit [H,W,3] image (got %s %s)"
                            % (image.dtype, image.shape))

    def _upload(self, image):
        """8-bit HWC image -> device.  A plain (pageable) copy: measured on MI355X it costs
        0.17 ms for a 2048x1024 image and is steady, while staging through a pinned buffer with
        a non-blocking copy showed periodic ~90 ms stalls (tools/probe_stalls.py)."""
        self._check_image(image)
        return torch.from_numpy(np.ascontiguousarray(image)).to(self.opt.device)

    def process(self, images, return_time=False):
        raise NotImplementedError

    def post_process(self, dets, meta, scale=1, fg=None):
        raise NotImplementedError

    def merge_outputs(self, detections):
        raise NotImplementedError

    def merge(self, detections):
        """What run() makes its `results` with: merge_outputs, unless a detector kept its detections on the device."""
        return self.merge_outputs(detections)

    def post_process_batch(self, dets, metas, scale=1):
        """post_process for the [B, K, ncols] detections of a batch with one meta per image."""
        raise NotImplementedError

    def merge_batch(self, detections):
        """merge for a batch: detections[scale] is what post_process_batch returned; one `results` dict per image."""
        raise NotImplementedError

    def debug(self, debugger, images, dets, output, scale=1):
        raise NotImplementedError

    def show_results(self, debugger, image, results):
        raise NotImplementedError

    def run(self, image_or_path_or_tensor, id=1, meta=None):
        """The same image gives the same detections, bit for bit, with and without --debug: for the duration of the
        call the vendor library is asked for its reproducible convolution algorithms (the previous setting is put
        back).  Only convolutions too small for the MFMA kernel reach it (hourglass: 512 -> 384 at 4 x 8); its
        default choice there sums in an order that changes from launch to launch.  DLA-34 has none."""
        before = torch.backends.cudnn.deterministic
        torch.backends.cudnn.deterministic = True
        try:
            return self._run(image_or_path_or_tensor, id, meta)
        finally:
            torch.backends.cudnn.deterministic = before

    def _run(self, image_or_path_or_tensor, id=1, meta=None):
        load_time = pre_time = net_time = dec_time = post_time = merge_time = 0
        start_time = time.time()
        pre_processed = False
        debug_level = getattr(self.opt, "debug", 0)
        debugger, stem = None, "img%s" % id
        if debug_level >= 1:
            if self.debugger is None:
                from ..utils.debugger import Debugger
                self.debugger = Debugger(class_names(self.opt), theme=getattr(self.opt, "debugger_theme", "white"),
                                         down_ratio=self.opt.down_ratio, device=self.opt.device)
            debugger = self.debugger
            debugger.imgs = {}
        if isinstance(image_or_path_or_tensor, np.ndarray):
            image = image_or_path_or_tensor
        elif isinstance(image_or_path_or_tensor, str):
            image = load_image(image_or_path_or_tensor)
            stem = os.path.splitext(os.path.basename(image_or_path_or_tensor))[0]
        else:
            image = image_or_path_or_tensor["image"][0].numpy()
            pre_processed_images = image_or_path_or_tensor
            pre_processed = True
        loaded_time = time.time()
        load_time += loaded_time - start_time
        self.image_sizes = [(int(image.shape[1]), int(image.shape[0]))]    # (width, height): the default canvas

        detections = []
        for scale in self.scales:
            scale_start_time = time.time()
            if not pre_processed:
                images, meta = self.pre_process(image, scale, meta)
            else:
                images = pre_processed_images["images"][scale][0]
                meta = pre_processed_images["meta"][scale]
                meta = {k: v.numpy()[0] for k, v in meta.items()}
            images = images.to(self.opt.device)
            torch.cuda.synchronize()
            pre_process_time = time.time()
            pre_time += pre_process_time - scale_start_time
            output, dets, forward_time = self.process(images, return_time=True)
            torch.cuda.synchronize()
            net_time += forward_time - pre_process_time
            decode_time = time.time()
            dec_time += decode_time - forward_time
            if debug_level >= 2:
                self.debug(debugger, images, dets, output, scale)
            dets = self.post_process(dets, meta, scale)
            post_process_time = time.time()
            post_time += post_process_time - decode_time
            detections.append(dets)

        results = self.merge(detections)
        end_time = time.time()
        merge_time += end_time - post_process_time
        ret = {"results": results, "tot": end_time - start_time, "load": load_time,
               "pre": pre_time, "net": net_time, "dec": dec_time, "post": post_time,
               "merge": merge_time}
        if debug_level >= 1:
            vis_id = self.show_results(debugger, image, results)
            torch.cuda.synchronize()
            ret["vis"] = debugger.imgs[vis_id]               # the overlay, still on the device
            ret["vis_files"] = debugger.show_all_imgs(pause=self.pause, path=self.opt.debug_dir, prefix=stem + "_")
            ret["vis_time"] = time.time() - end_time
        return ret

    def run_batch(self, images):
        """run() for a list of images (arrays or paths) that go through the network together: {"results": [what run()
        returns as "results", one per image], "n": B, "tot", "load", "pre", "net", "dec", "post", "merge"}, the times
        for the whole batch.  The batch kernels restate the per-image ones bit for bit; the network chooses some K
        splits by its launch size, so its heads agree with a single-image launch to rounding, not in every bit.  The
        debug pictures stay with run(): --debug >= 1 and more than one image is a ValueError."""
        images = list(images)
        if not images:
            raise ValueError("run_batch needs at least one image")
        if getattr(self.opt, "debug", 0) >= 1 and len(images) > 1:
            raise ValueError("run_batch draws no debug pictures: with --debug %d send the images through run() one "
                             "at a time" % self.opt.debug)
        before = torch.backends.cudnn.deterministic
        torch.backends.cudnn.deterministic = True
        try:
            return self._run_batch(images)
        finally:
            torch.backends.cudnn.deterministic = before

    def _run_batch(self, images):
        pre_time = net_time = dec_time = post_time = 0
        start_time = time.time()
        images = [load_image(im) if isinstance(im, str) else im for im in images]
        for im in images:
            if not isinstance(im, np.ndarray):
                raise TypeError("run_batch takes 8-bit [H,W,3] arrays or paths (got %s)" % type(im).__name__)
        loaded_time = time.time()
        self.image_sizes = [(int(im.shape[1]), int(im.shape[0])) for im in images]
        detections = []
        for scale in self.scales:
            scale_start_time = time.time()
            batch, metas = self.pre_process_batch(images, scale)
            torch.cuda.synchronize()
            pre_process_time = time.time()
            pre_time += pre_process_time - scale_start_time
            output, dets, forward_time = self.process(batch, return_time=True)
            torch.cuda.synchronize()
            net_time += forward_time - pre_process_time
            decode_time = time.time()
            dec_time += decode_time - forward_time
            detections.append(self.post_process_batch(dets, metas, scale))
            post_process_time = time.time()
            post_time += post_process_time - decode_time
        results = self.merge_batch(detections)
        end_time = time.time()
        return {"results": results, "n": len(images), "tot": end_time - start_time, "load": loaded_time - start_time,
                "pre": pre_time, "net": net_time, "dec": dec_time, "post": post_time,
                "merge": end_time - post_process_time}

"""Distances of instances from the Cityscapes disparity maps, for the AP 100 m / AP 50 m columns of the instance-level
evaluation (the `medDist` / `distConf` fields of the evaluator's ground-truth instances).

The reference's evaluator carries the two fields and the thresholds (distanceThs = [inf, 100, 50], distanceConfs =
[-inf, 0.5, 0.5]) but none of its public scripts fills them; the benchmark server does.  The definition here is this
project's, from the data set's documented disparity encoding:

  pixel       a disparity pixel p of `disparity/<split>/<city>/<frame>_disparity.png` (16 bit): p == 0 is "no
              measurement"; otherwise d = (p - 1) / 256.0 and distance = (baseline * fx) / d in float64, in exactly this
              order of operations, with `baseline` (extrinsic.baseline) and `fx` (intrinsic.fx) of the frame's
              `camera/<split>/<city>/<frame>_camera.json`.  p == 1 gives +inf.
  medDist     numpy's median of the distances of the instance's measured pixels.  The distance falls as p rises, so
              it is 0.5 * (distance(v_lo) + distance(v_hi)) of the two middle order statistics of p; +inf for an
              instance without a measured pixel (it is outside both finite settings).
  distConf    measured pixels / pixels, the stereo density (the evaluator's JSON key `minStereoDensities`).

The per-instance order statistics are cp_segment_medians' (csrc/segment_median.hip): one call per image on the id
image the device already holds, whatever the number of instances; this module does the float64 mapping on the
[G, 4] integers that come back.  Any id image works: the ground truth's, or a prediction's `ids` map
(detector.instances)."""
import json
import math
import os

import numpy as np

DISPARITY_SUFFIX = "_disparity.png"
CAMERA_SUFFIX = "_camera.json"
MAX_SEG = 1024                                           # limit of cp_segment_medians
REFUSED = {"kitti_poly": "kittiscripts' instance evaluator has no disparity convention (no medDist / distConf source)",
           "IDD": "IDDscripts' instance evaluator has no disparity convention (no medDist / distConf source)"}
DATASETS = ("cityscapes",)


def pixel_distance(p, baseline, fx):
    """float64 distances of disparity pixels p (p != 0), by the module's formula; p == 1 gives +inf."""
    d = (np.asarray(p, np.float64) - 1.0) / 256.0
    with np.errstate(divide="ignore"):
        return (np.float64(baseline) * np.float64(fx)) / d


def table_from_counts(raw, camera):
    """float64 [G, 2] (medDist, distConf) from cp_segment_medians' int [G, 4] (pixels, valid, v_lo, v_hi) and the
    camera (baseline, fx).  distConf of a segment without pixels is 0."""
    raw = np.asarray(raw, np.int64).reshape(-1, 4)
    baseline, fx = camera
    out = np.zeros((len(raw), 2), np.float64)
    has = raw[:, 1] > 0
    out[:, 0] = np.inf
    out[has, 0] = 0.5 * (pixel_distance(raw[has, 2], baseline, fx) + pixel_distance(raw[has, 3], baseline, fx))
    out[:, 1] = raw[:, 1] / np.maximum(raw[:, 0], 1).astype(np.float64)
    return out


def read_disparity(path):
    """A `*_disparity.png` as uint16 [H, W] (PIL hands it over as uint16 or as 32-bit mode I)."""
    from PIL import Image
    arr = np.array(Image.open(path))
    if arr.ndim != 2 or arr.dtype.kind not in "iu":
        raise ValueError("%s is not a single-channel integer disparity image (shape %s, %s)"
                         % (path, arr.shape, arr.dtype))
    if arr.size and (arr.min() < 0 or arr.max() > 65535):
        raise ValueError("%s holds disparities outside 16 bits (%d .. %d)" % (path, arr.min(), arr.max()))
    return np.ascontiguousarray(arr.astype(np.uint16))


def read_camera(path):
    """(baseline, fx) of a `*_camera.json`: extrinsic.baseline and intrinsic.fx, both finite and positive."""
    with open(path) as f:
        try:
            cam = json.load(f)
        except ValueError as e:
            raise ValueError("%s is not a JSON file: %s" % (path, e))
    out = []
    for group, key in (("extrinsic", "baseline"), ("intrinsic", "fx")):
        try:
            v = cam[group][key]
        except (KeyError, TypeError):
            raise ValueError("%s has no %s.%s" % (path, group, key))
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or v <= 0:
            raise ValueError("%s: %s.%s must be a finite positive number, got %r" % (path, group, key, v))
        out.append(float(v))
    return tuple(out)


def find_files(disparity_dir, camera_dir):
    """{image key: (disparity path, camera path)} of the `*_disparity.png` below disparity_dir and the
    `*_camera.json` below camera_dir, keyed like find_gt_files (the image prefix).  A key with one of the two only
    has None for the other; two files for one key are refused."""
    found = []
    for top, suffix, what in ((disparity_dir, DISPARITY_SUFFIX, "disparity"), (camera_dir, CAMERA_SUFFIX, "camera")):
        if not os.path.isdir(top):
            raise FileNotFoundError("the %s directory %s is not a directory" % (what, top))
        one = {}
        for root, _, files in os.walk(top):
            for f in sorted(files):
                if not f.endswith(suffix):
                    continue
                key = f[:-len(suffix)]
                if key in one:
                    raise ValueError("two %s files for %s: %s and %s" % (what, key, one[key], os.path.join(root, f)))
                one[key] = os.path.join(root, f)
        found.append(one)
    disp, cam = found
    return {key: (disp.get(key), cam.get(key)) for key in sorted(set(disp) | set(cam))}


def frame_files(files, key, image=""):
    """(disparity path, camera path) of one frame out of find_files' dictionary; a frame without either file is a
    FileNotFoundError that names it."""
    disp, cam = files.get(key, (None, None))
    for path, suffix, flag in ((disp, DISPARITY_SUFFIX, "--disparity_dir"), (cam, CAMERA_SUFFIX, "--camera_dir")):
        if path is None:
            raise FileNotFoundError("no %s%s below %s%s" % (key, suffix, flag, image and " for image " + image))
    return disp, cam


def segment_medians(ids_dev, seg_ids, disparity_dev):
    """cp_segment_medians on device ids and disparity [H, W] (16-bit elements): the int32 [G, 4] DEVICE tensor
    (pixels, valid, v_lo, v_hi), G <= 1024.  Nothing is read back."""
    import torch
    G = len(seg_ids)
    dev = ids_dev.device
    seg = torch.as_tensor(np.asarray(seg_ids, np.int64).astype(np.int32)).to(dev)
    out = torch.empty((G, 4), dtype=torch.int32, device=dev)
    enqueue_medians(ids_dev, disparity_dev, seg, G, out)
    return out


def enqueue_medians(ids_dev, disparity_dev, seg_dev, G, out_dev):
    """The call itself: seg_dev int32 [>= G] and out_dev int32 [>= 4 G] (views into larger tensors are fine) on the
    device of ids_dev."""
    from ... import _C
    H, W = ids_dev.shape
    if tuple(disparity_dev.shape) != (H, W):
        raise ValueError("the disparity image is %s, the id image is %s" % (tuple(disparity_dev.shape), (H, W)))
    L = _C.lib()
    nbytes = L.cp_segment_medians_workspace_bytes(G, H, W)
    ws = _C.workspace(nbytes, ids_dev.device)
    _C.check(L.cp_segment_medians(_C.ptr(ids_dev), _C.ptr(disparity_dev), H, W, _C.ptr(seg_dev), G, _C.ptr(out_dev),
                                  _C.ptr(ws), nbytes, _C.stream()), "cp_segment_medians")


def instance_distances(ids_dev, seg_ids, disparity, camera):
    """(float64 [G, 2] table of (medDist, distConf), int64 [G, 4] raw (pixels, valid, v_lo, v_hi)) of the segments
    `seg_ids` of the device id image ids_dev [H, W] (16-bit elements).  disparity: a host uint16 [H, W] array (see
    read_disparity) or a device tensor of 16-bit elements; camera: (baseline, fx).  Any number of segments: the
    kernel is called on slices of 1024."""
    from . import instance_level
    seg_ids = np.asarray(seg_ids, np.int64).reshape(-1)
    disp = instance_level.device_ids(disparity, ids_dev.device, "disparity")
    raw = np.zeros((len(seg_ids), 4), np.int64)
    for g in range(0, len(seg_ids), MAX_SEG):
        raw[g:g + MAX_SEG] = segment_medians(ids_dev, seg_ids[g:g + MAX_SEG], disp).cpu().numpy()
    return table_from_counts(raw, camera), raw

"""GPU probe: the merge of the test scales on the device (cp_merge_detections) against merge_outputs on the host.

A DLA-34 with seeded weights (synth.fill_by_name; K = 128, 8 classes, 16 vertices) on one seeded 512x1024 image, with
two (--test_scales 1,0.5) and three (0.5,1,2) test scales.  The rows of each class are reported with the times: the
classes run in parallel on the device, one after the other on the host.

1. cp_merge_detections alone on the detector's own rows [S, 128, 39]: HIP events around `--iters` calls, median and
   [min, max] of `--rounds` rounds after warm-up.
2. The wall clock per image of what lies between the decoded detections and a table on the device: the `post` and
   `merge` times run() reports plus device_rows() (ended by a synchronise), with PolydetDetector.device_merge on and
   off, alternating per image; median and [min, max] over `--passes` passes of the mean over `--images` images, after
   two warm-up passes.  (With device_merge on, post_process only enqueues its kernel; it runs before merge's copy
   back, so the sum holds it.)  Both settings must give the same results, bit for bit, or the probe stops.

Usage:  python tools/probe_merge.py [--json OUT] [--untrained]
"""
import argparse
import contextlib
import io
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from centerpoly_amd import _C, synth
from centerpoly_amd.detectors.detector_factory import detector_factory
from centerpoly_amd.opts import opts


def spread(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def kernel_alone(det, a):
    rows, C = det.scale_rows, det.num_classes
    S, K, ncols = rows.shape
    L = _C.lib()
    ws = _C.workspace(L.cp_merge_detections_workspace_bytes(S, K, ncols, C), rows.device)
    out = torch.empty((S * K, ncols), dtype=torch.float32, device=rows.device)
    counts = torch.empty((1 + C,), dtype=torch.int32, device=rows.device)

    def call():
        _C.check(L.cp_merge_detections(_C.ptr(rows), S, K, ncols, C, det.max_per_image, 1, 0.5, 0.5, 0.001, 2,
                                       _C.ptr(out), _C.ptr(counts), _C.ptr(ws), ws.numel(), _C.stream()),
                 "cp_merge_detections")
    for _ in range(20):
        call()
    torch.cuda.synchronize()
    us = []
    for _ in range(a.rounds):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(a.iters):
            call()
        e.record()
        torch.cuda.synchronize()
        us.append(s.elapsed_time(e) / a.iters * 1e3)
    per_class = np.bincount(rows[:, :, 5].cpu().numpy().astype(np.int64).ravel(), minlength=C).tolist()
    return dict(spread(us), S=S, K=K, ncols=ncols, classes=C, rows_per_class=per_class, kept=counts.cpu().tolist())


def same(a, b):
    return sorted(a) == sorted(b) and all(a[j].shape == b[j].shape and np.array_equal(a[j].view(np.uint32),
                                                                                      b[j].view(np.uint32)) for j in a)


def wall(det, img, a):
    per_pass = {"on": [], "off": []}
    for rnd in range(a.passes + 2):                                       # two warm-up passes
        acc = {"on": [], "off": []}
        for i in range(a.images):
            res = {}
            for name in (("on", "off") if (rnd + i) % 2 == 0 else ("off", "on")):
                det.device_merge = name == "on"
                with contextlib.redirect_stdout(io.StringIO()):
                    ret = det.run(img)
                t0 = time.perf_counter()
                det.device_rows(ret["results"])
                torch.cuda.synchronize()
                acc[name].append((ret["post"] + ret["merge"] + time.perf_counter() - t0) * 1e3)
                res[name] = ret["results"]
            if not same(res["on"], res["off"]):
                raise SystemExit("device_merge on and off disagree on the results")
        if rnd >= 2:
            for k in per_pass:
                per_pass[k].append(float(np.mean(acc[k])))
    det.device_merge = True
    return {k: spread(v) for k, v in per_pass.items()}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rounds", type=int, default=7)
    p.add_argument("--iters", type=int, default=200)
    p.add_argument("--passes", type=int, default=10)
    p.add_argument("--images", type=int, default=8)
    p.add_argument("--untrained", action="store_true",
                   help="keep the random initialisation: every row falls into class 0, the longest chain for one wave")
    p.add_argument("--json", default="")
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("probe_merge needs a GPU: nothing is measured without one")
    img = (synth.uniform("probe_merge/img", (512, 1024, 3)) * 255).astype(np.uint8)
    result = {"unit_kernel": "us", "unit_wall": "ms per image", "passes": a.passes, "images": a.images}
    # seeded weights by parameter name: a freshly initialised network scores every centre alike, and the 128 best of
    # a tie are all of class 0
    from centerpoly_amd.models.model import create_model, save_model
    model = create_model("dla_34", {"hm": 8, "poly": 32, "pseudo_depth": 1, "reg": 2}, 256)
    w = synth.fill_by_name({k: tuple(v.shape) for k, v in model.state_dict().items()})
    model.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()})
    weights = os.path.join(tempfile.mkdtemp(), "model_seeded.pth")
    save_model(weights, 1, model)
    del model
    for scales in ("1,0.5", "0.5,1,2"):
        opt = opts().init(["polydet", "--arch", "dla_34", "--test_scales", scales, "--K", "128", "--load_model",
                           "" if a.untrained else weights])
        with contextlib.redirect_stdout(io.StringIO()):
            det = detector_factory["polydet"](opt)
        det.device_merge = True
        with contextlib.redirect_stdout(io.StringIO()):
            det.run(img)
        S = len(opt.test_scales)
        k = kernel_alone(det, a)
        w = wall(det, img, a)
        result["S%d" % S] = {"kernel_us": k, "wall_ms": w}
        print("S = %d: cp_merge_detections %.1f us [%.1f, %.1f] (kept %d of %d rows); post + merge + device_rows per "
              "image: device_merge on %.3f ms [%.3f, %.3f], off %.3f ms [%.3f, %.3f]"
              % (S, k["median"], k["min"], k["max"], k["kept"][0], S * k["K"], w["on"]["median"], w["on"]["min"],
                 w["on"]["max"], w["off"]["median"], w["off"]["min"], w["off"]["max"]))
        del det
        torch.cuda.empty_cache()
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()

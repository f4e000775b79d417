"""GPU probe: the merge of --mask_nms (cp_polygon_overlaps, cp_merge_detections_mask) against the literal merge
(cp_merge_detections) and against torch ops that count the same pairs.

A DLA-34 with seeded weights (synth.fill_by_name; K = 128, 8 classes, 16 vertices) on seeded 512x1024 and 1024x2048
images, with two (--test_scales 1,0.5) and three (0.5,1,2) test scales; and, at 512x1024 with two scales, the freshly
initialised network, whose rows all fall into class 0 (the longest chain for the one wave that selects a class, and the
most pairs).

1. The entry points alone on the detector's own rows [S, 128, 39] and the image's canvas: HIP events around `--iters`
   calls, median and [min, max] of `--rounds` rounds after warm-up: cp_polygon_overlaps, cp_merge_detections_mask,
   and cp_merge_detections on the same rows as the baseline.
2. The same pair counts from torch ops: one bool plane per row (its box as a rectangle -- torch has no polygon fill,
   so this is the cheapest raster it could have), float32, and one matrix product [R, H W] x [H W, R].
3. The wall clock per image of what lies between the decoded detections and a table on the device: the `post` and
   `merge` times run() reports plus device_rows() (ended by a synchronise), with --mask_nms and without it (the literal
   device merge), alternating per image; median and [min, max] over `--passes` passes of the mean over `--images`
   images, after two warm-up passes.
4. The seeded network's polygons are small and never overlap, so the entry points are also timed on synthetic rows that
   overlap as a trained detector's do -- 128 objects of radius 20 .. 150 pixels in 8 classes, every object once per
   scale (synthetic_rows) -- and on the pathological case: every row in one class, every polygon over the middle half of
   the canvas, at 256 and at 1024 rows.

Usage:  python tools/probe_mask_nms.py [--json profiles/probe_mask_nms.json]
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


def timed(call, rounds, iters, warm=5):
    for _ in range(warm):
        call()
    torch.cuda.synchronize()
    us = []
    for _ in range(rounds):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(iters):
            call()
        e.record()
        torch.cuda.synchronize()
        us.append(s.elapsed_time(e) / iters * 1e3)
    return spread(us)


class Rows(object):
    """What kernels_alone reads of a detector, for rows that no network made."""

    def __init__(self, rows, num_classes, max_per_image):
        self.scale_rows, self.num_classes, self.max_per_image = rows, num_classes, max_per_image


def synthetic_rows(tag, S, K, C, W, H, cover=False):
    """[S, K, 39] rows of K objects seen at S scales: 16-gons of radius 20 .. 150 pixels scattered over the canvas, every
    scale's copy moved by up to 3 pixels, classes of [0, C).  `cover`: one class and every polygon over the middle
    half of the canvas -- every pair overlaps: what a freshly initialised network can give."""
    u = lambda name, shape, lo=0.0, hi=1.0: synth.uniform("probe_mask_nms/%s/%s" % (tag, name), shape, lo, hi)
    r = u("r", (K, 1), 0.42, 0.5) * min(W, H) if cover else u("r", (K, 1), 20.0, 150.0)
    cx = u("cx", (K, 1), 0.45, 0.55) * W if cover else u("cx", (K, 1), 0.0, 1.0) * W
    cy = u("cy", (K, 1), 0.45, 0.55) * H if cover else u("cy", (K, 1), 0.0, 1.0) * H
    ang = (np.arange(16)[None, :] + u("a", (K, 16), -0.3, 0.3)) * (2 * np.pi / 16)
    rad = r * (1 + u("j", (K, 16), -0.2, 0.2))
    rows = np.zeros((S, K, 39), np.float32)
    for s in range(S):
        dx, dy = u("dx%d" % s, (K, 1), -3.0, 3.0), u("dy%d" % s, (K, 1), -3.0, 3.0)
        x, y = cx + dx + rad * np.cos(ang), cy + dy + rad * np.sin(ang)
        rows[s, :, 0], rows[s, :, 1], rows[s, :, 2], rows[s, :, 3] = x.min(1), y.min(1), x.max(1), y.max(1)
        rows[s, :, 4] = u("score%d" % s, (K,), 0.02, 1.0)
        rows[s, :, 5] = 0 if cover else synth.integers("probe_mask_nms/%s/cls" % tag, (K,), 0, C)
        rows[s, :, 6:38:2], rows[s, :, 7:38:2] = x, y
        rows[s, :, 38] = u("depth%d" % s, (K,))
    return torch.from_numpy(rows).cuda()


def kernels_alone(det, canvas, a, torch_too=True):
    rows, C = det.scale_rows, det.num_classes
    S, K, ncols = rows.shape
    R, (W, H) = S * K, canvas
    L = _C.lib()
    flat = rows.view(R, ncols)
    ws_o = _C.workspace(L.cp_polygon_overlaps_workspace_bytes(R, ncols, H, W), rows.device)
    ws_m = _C.workspace(L.cp_merge_detections_mask_workspace_bytes(S, K, ncols, C, H, W), rows.device)
    ws_l = _C.workspace(L.cp_merge_detections_workspace_bytes(S, K, ncols, C), rows.device)
    area = torch.empty(R, dtype=torch.int32, device=rows.device)
    inter = torch.empty((R, R), dtype=torch.int32, device=rows.device)
    out = torch.empty((R, ncols), dtype=torch.float32, device=rows.device)
    counts = torch.empty((1 + C,), dtype=torch.int32, device=rows.device)

    def overlaps():
        _C.check(L.cp_polygon_overlaps(_C.ptr(flat), R, ncols, C, H, W, _C.ptr(area), _C.ptr(inter), _C.ptr(ws_o),
                                       ws_o.numel(), _C.stream()), "cp_polygon_overlaps")

    def mask():
        _C.check(L.cp_merge_detections_mask(_C.ptr(rows), S, K, ncols, C, det.max_per_image, 1, 0.5, 0.5, 0.001, 2, H, W,
                                            _C.ptr(out), _C.ptr(counts), _C.ptr(ws_m), ws_m.numel(), _C.stream()),
                 "cp_merge_detections_mask")

    def literal():
        _C.check(L.cp_merge_detections(_C.ptr(rows), S, K, ncols, C, det.max_per_image, 1, 0.5, 0.5, 0.001, 2,
                                       _C.ptr(out), _C.ptr(counts), _C.ptr(ws_l), ws_l.numel(), _C.stream()),
                 "cp_merge_detections")

    ys = torch.arange(H, device=rows.device, dtype=torch.float32).view(1, H, 1)
    xs = torch.arange(W, device=rows.device, dtype=torch.float32).view(1, 1, W)

    def torch_pairs():
        b = flat[:, :4].round()
        planes = ((xs >= b[:, 0].view(R, 1, 1)) & (xs <= b[:, 2].view(R, 1, 1))
                  & (ys >= b[:, 1].view(R, 1, 1)) & (ys <= b[:, 3].view(R, 1, 1))).view(R, H * W).float()
        same = flat[:, 5].view(R, 1) == flat[:, 5].view(1, R)
        return (planes @ planes.t()) * same

    r = {"S": S, "K": K, "ncols": ncols, "classes": C, "canvas": [W, H],
         "workspace_bytes": {"overlaps": int(ws_o.numel()), "mask": int(ws_m.numel()), "literal": int(ws_l.numel())},
         "rows_per_class": np.bincount(rows[:, :, 5].cpu().numpy().astype(np.int64).ravel(), minlength=C).tolist()}
    r["cp_polygon_overlaps_us"] = timed(overlaps, a.rounds, a.iters)
    r["pairs_nonzero"] = int(((inter != 0).sum().item() - (area != 0).sum().item()) // 2)
    r["mask_pixels"] = int(area.sum().item())
    r["cp_merge_detections_mask_us"] = timed(mask, a.rounds, a.iters)
    r["kept_mask"] = counts.cpu().tolist()
    r["cp_merge_detections_us"] = timed(literal, a.rounds, a.iters)
    r["kept_literal"] = counts.cpu().tolist()
    if torch_too:
        r["torch_box_planes_matmul_us"] = timed(torch_pairs, a.rounds, max(1, a.iters // 20), warm=2)
    return r


def wall(dets, img, a):
    per_pass = {k: [] for k in dets}
    names = sorted(dets)
    for rnd in range(a.passes + 2):                                       # two warm-up passes
        acc = {k: [] for k in dets}
        for i in range(a.images):
            for name in (names if (rnd + i) % 2 == 0 else names[::-1]):
                det = dets[name]
                with contextlib.redirect_stdout(io.StringIO()):
                    ret = det.run(img)
                t0 = time.perf_counter()
                det.device_rows(ret["results"])
                torch.cuda.synchronize()
                acc[name].append((ret["post"] + ret["merge"] + time.perf_counter() - t0) * 1e3)
        if rnd >= 2:
            for k in per_pass:
                per_pass[k].append(float(np.mean(acc[k])))
    return {k: spread(v) for k, v in per_pass.items()}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rounds", type=int, default=7)
    p.add_argument("--iters", type=int, default=100)
    p.add_argument("--passes", type=int, default=6)
    p.add_argument("--images", type=int, default=6)
    p.add_argument("--json", default="")
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("probe_mask_nms needs a GPU: nothing is measured without one")
    result = {"unit_kernel": "us", "unit_wall": "ms per image", "rounds": a.rounds, "iters": a.iters, "passes": a.passes,
              "images": a.images}
    from centerpoly_amd.models.model import create_model, save_model
    model = create_model("dla_34", {"hm": 8, "poly": 32, "pseudo_depth": 1, "reg": 2}, 256)
    w = synth.fill_by_name({k: tuple(v.shape) for k, v in model.state_dict().items()})
    model.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()})
    weights = os.path.join(tempfile.mkdtemp(), "model_seeded.pth")
    save_model(weights, 1, model)
    del model
    configs = [("seeded", h, wd, sc) for (h, wd) in ((512, 1024), (1024, 2048)) for sc in ("1,0.5", "0.5,1,2")]
    configs.append(("untrained", 512, 1024, "1,0.5"))
    for kind, h, wd, scales in configs:
        img = (synth.uniform("probe_mask_nms/img%d" % h, (h, wd, 3)) * 255).astype(np.uint8)
        dets = {}
        for name, extra in (("mask_nms", ["--mask_nms"]), ("literal", [])):
            opt = opts().init(["polydet", "--arch", "dla_34", "--test_scales", scales, "--K", "128", "--load_model",
                               weights if kind == "seeded" else ""] + extra)
            with contextlib.redirect_stdout(io.StringIO()):
                dets[name] = detector_factory["polydet"](opt)
                dets[name].run(img)
        S = len(scales.split(","))
        k = kernels_alone(dets["mask_nms"], (wd, h), a)
        wl = wall(dets, img, a)
        key = "%s_S%d_%dx%d" % (kind, S, h, wd)
        result[key] = {"kernel_us": k, "wall_ms": wl}
        print("%s: overlaps %.1f us [%.1f, %.1f]; mask merge %.1f us [%.1f, %.1f] (kept %d of %d); literal merge %.1f us "
              "[%.1f, %.1f]; torch box planes + matmul %.1f us; %d pairs overlap, rows per class %s; post + merge + "
              "device_rows per image: --mask_nms %.3f ms [%.3f, %.3f], literal %.3f ms [%.3f, %.3f]"
              % (key, k["cp_polygon_overlaps_us"]["median"], k["cp_polygon_overlaps_us"]["min"],
                 k["cp_polygon_overlaps_us"]["max"], k["cp_merge_detections_mask_us"]["median"],
                 k["cp_merge_detections_mask_us"]["min"], k["cp_merge_detections_mask_us"]["max"], k["kept_mask"][0],
                 S * k["K"], k["cp_merge_detections_us"]["median"], k["cp_merge_detections_us"]["min"],
                 k["cp_merge_detections_us"]["max"], k["torch_box_planes_matmul_us"]["median"], k["pairs_nonzero"],
                 k["rows_per_class"], wl["mask_nms"]["median"], wl["mask_nms"]["min"], wl["mask_nms"]["max"],
                 wl["literal"]["median"], wl["literal"]["min"], wl["literal"]["max"]), flush=True)
        del dets
        torch.cuda.empty_cache()
    # rows that overlap as a trained detector's do: every object once per scale; and the pathological case
    for tag, S, K, cover, iters in (("objects_S2", 2, 128, False, a.iters), ("objects_S3", 3, 128, False, a.iters),
                                    ("cover_S2", 2, 128, True, 5), ("cover_1024rows", 4, 256, True, 2)):
        for h, wd in ((512, 1024), (1024, 2048)):
            rows = synthetic_rows(tag, S, K, 8, wd, h, cover)
            b = argparse.Namespace(rounds=a.rounds if iters > 2 else 3, iters=iters)
            k = kernels_alone(Rows(rows, 8, 128), (wd, h), b, torch_too=not cover)
            key = "%s_%dx%d" % (tag, h, wd)
            result[key] = {"kernel_us": k}
            print("%s: overlaps %.1f us [%.1f, %.1f]; mask merge %.1f us [%.1f, %.1f] (kept %d of %d); literal merge %.1f "
                  "us [%.1f, %.1f]; %d pairs overlap, %d mask pixels, rows per class %s"
                  % (key, k["cp_polygon_overlaps_us"]["median"], k["cp_polygon_overlaps_us"]["min"],
                     k["cp_polygon_overlaps_us"]["max"], k["cp_merge_detections_mask_us"]["median"],
                     k["cp_merge_detections_mask_us"]["min"], k["cp_merge_detections_mask_us"]["max"], k["kept_mask"][0],
                     S * K, k["cp_merge_detections_us"]["median"], k["cp_merge_detections_us"]["min"],
                     k["cp_merge_detections_us"]["max"], k["pairs_nonzero"], k["mask_pixels"], k["rows_per_class"]),
                  flush=True)
            del rows
            torch.cuda.empty_cache()
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()

"""GPU probe: what the panoptic evaluation costs (cp_panoptic_pairs + cp_panoptic_match, the torch composition of the
same pair counts, what --panoptic adds to an image of test.py's loop).

1. The two entry points on 2048 x 1024, HIP events around `--kernel_iters` pairs of calls, median and [min, max] over
   `--rounds`, on four contents:
     scene         the seeded street scene of tools/probe_pixel_level.py (30 instances over sky, buildings and road), the
                   prediction its instances shifted by 7 pixels: tens x tens of cells, the dense (LDS) regime
     one_pair      every pixel in one cell
     checkerboard  two cells, alternating pixel by pixel: no run longer than one
     limit         1024 segments x 255 slots, both random per pixel: 1025 x 256 cells, the sparse (global atomics) regime
   and cp_panoptic_pairs alone on the scene.  The algorithm reads the ids twice and the index once, 5 bytes a pixel.
2. The same pair counts from torch ops: torch.unique with counts on the combined key (segment value, VOID as 0) * 256 +
   column.  The kernel's non-zero cells must equal them in every number or the probe stops.
3. --panoptic per image: a DLA-34 with seeded weights at 1024 x 2048, K = 128, --dataset cityscapes; after run() the two
   calls test.py adds, detector.instances() and PanopticEvaluator.add_maps().  add_maps is timed three ways: with the id
   image as test.py hands it over (a host array: the upload is part of the call) and a synchronise at the end, which is
   what probe_pixel_level.py's add_maps figure holds; with the id image on the device and a synchronise; and the host
   time of the call alone with the id image on the device, nothing waited for.

Usage:  python tools/probe_panoptic.py [--json profiles/probe_panoptic.json]
"""
import argparse
import contextlib
import ctypes
import io
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

from tools.probe_instances import seeded_weights, spread, timed
from tools.probe_pixel_level import H, W, scene

LABELS = (24, 25, 26, 27, 28, 31, 32, 33)


def contents():
    """{name: (ids uint16 [H, W], index uint8 [H, W], n, slot labels)}"""
    ids = scene()[0]
    wide = ids.astype(np.int64)
    index = np.roll(np.where(wide >= 1000, wide % 1000 - 1, 255).astype(np.uint8), 7, axis=1)
    out = {"scene": (ids, index, 30, np.array([LABELS[k % 8] for k in range(30)], np.int32))}
    out["one_pair"] = (np.full((H, W), 26001, np.uint16), np.zeros((H, W), np.uint8), 1, np.array([26], np.int32))
    k = np.add.outer(np.arange(H), np.arange(W)) % 2
    out["checkerboard"] = (np.where(k == 0, 26001, 24002).astype(np.uint16), k.astype(np.uint8), 2,
                           np.array([26, 24], np.int32))
    rng = np.random.RandomState(29)
    out["limit"] = ((24001 + rng.randint(0, 1024, (H, W))).astype(np.uint16), rng.randint(0, 255, (H, W)).astype(np.uint8),
                    255, (24 + np.arange(255) % 2).astype(np.int32))
    return out


def kernels(a):
    import torch
    from centerpoly_amd import _C
    from centerpoly_amd.datasets.evaluation import panoptic as pq
    dev = torch.device("cuda")
    p = pq.CITYSCAPES
    lib = _C.lib()
    flags = np.ascontiguousarray(p.flags)
    fp = flags.ctypes.data_as(ctypes.c_void_p)
    evaluated = torch.from_numpy((flags & 1).astype(np.int64)).to(dev)
    nbytes = lib.cp_panoptic_pairs_workspace_bytes()
    ws = _C.workspace(nbytes, dev)
    seg = torch.zeros((1025, 4), dtype=torch.int32, device=dev)
    stat = torch.zeros((p.L, 3), dtype=torch.int64, device=dev)
    iou = torch.zeros((p.L,), dtype=torch.float64, device=dev)
    bad = torch.zeros((2,), dtype=torch.int32, device=dev)
    out = {}
    for name, (ids, index, n, labels) in contents().items():
        ids_dev = torch.from_numpy(ids.view(np.int16)).to(dev)
        index_dev = torch.from_numpy(index).to(dev)
        pairs = torch.zeros((1025 * (n + 1),), dtype=torch.int32, device=dev)

        def count():
            _C.check(lib.cp_panoptic_pairs(_C.ptr(index_dev), n, _C.ptr(ids_dev), H, W, p.id_divisor, p.id_direct_below,
                                           p.L, fp, _C.ptr(seg), _C.ptr(pairs), _C.ptr(ws), nbytes, _C.stream()),
                     "cp_panoptic_pairs")

        def both():
            count()
            _C.check(lib.cp_panoptic_match(_C.ptr(seg), _C.ptr(pairs), n, labels.ctypes.data_as(ctypes.c_void_p), p.L, fp,
                                           _C.ptr(stat), _C.ptr(iou), _C.ptr(bad), None, _C.stream()), "cp_panoptic_match")

        wide = torch.from_numpy(ids.astype(np.int64)).to(dev)

        def composed():
            v = wide.reshape(-1)
            g = torch.where(v < p.id_direct_below, v, v // p.id_divisor)
            gid = torch.where(evaluated[g.clamp(max=p.L - 1)].bool() & (g < p.L), v, torch.zeros_like(v))
            return torch.unique(gid * 256 + index_dev.reshape(-1).long().clamp(max=n), return_counts=True)

        both()
        keys, counts = composed()
        cells = pairs.reshape(1025, n + 1)
        G = int(seg[0, 0])
        if G > 1024 or not torch.equal(cells[cells > 0].long(), counts) or int(cells.sum()) != H * W:
            raise SystemExit("the torch composition and the kernel disagree on the %s image" % name)
        r = out[name] = {"G": G, "n": n, "cells": int((cells > 0).sum()), "regime": "dense" if (G + 1) * (n + 1) <= 15360
                         else "sparse", "us": timed(both, a.kernel_iters, a.rounds),
                         "pairs_only_us": timed(count, a.kernel_iters, a.rounds),
                         "torch_us": timed(composed, max(1, a.kernel_iters // 10), a.rounds), "bytes_read": 5 * H * W}
        r["GBps"] = r["bytes_read"] / (r["pairs_only_us"]["median"] * 1e-6) / 1e9
    worst = max(out, key=lambda k: out[k]["us"]["median"])
    out["worst"] = worst
    out["worst_over_scene"] = out[worst]["us"]["median"] / out["scene"]["us"]["median"]
    return out


def per_image(a, weights):
    import torch
    from centerpoly_amd import synth
    from centerpoly_amd.datasets.dataset_factory import dataset_factory
    from centerpoly_amd.datasets.evaluation import panoptic as pq
    from centerpoly_amd.detectors.detector_factory import detector_factory
    from centerpoly_amd.opts import opts
    with contextlib.redirect_stdout(io.StringIO()):
        opt = opts().parse(["polydet", "--arch", "dla_34", "--K", "128", "--input_h", str(H), "--input_w", str(W),
                            "--dataset", "cityscapes", "--load_model", weights])
        opt = opts().update_dataset_info_and_set_heads(opt, dataset_factory["cityscapes"])
        det = detector_factory["polydet"](opt)
    ids = scene()[0]
    ids_dev = torch.from_numpy(ids.view(np.int16)).cuda()
    img = (synth.uniform("probe_pixel_level/img", (H, W, 3)) * 255).astype(np.uint8)
    ret = det.run(img)
    ev = pq.PanopticEvaluator(pq.CITYSCAPES)
    ms = {"instances": [], "host_gt_sync": [], "device_gt_sync": [], "device_gt_enqueue": [], "run": []}
    for k in range(3 + a.image_calls):
        t0 = time.perf_counter()
        maps = det.instances(ret["results"])
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        ev.add_maps(maps, ids)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        ev.add_maps(maps, ids_dev)
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        ev.add_maps(maps, ids_dev)
        t4 = time.perf_counter()
        torch.cuda.synchronize()
        if k >= 3:
            for key, v in (("instances", t1 - t0), ("host_gt_sync", t2 - t1), ("device_gt_sync", t3 - t2),
                           ("device_gt_enqueue", t4 - t3)):
                ms[key].append(v * 1e3)
    for _ in range(5):
        t0 = time.perf_counter()
        det.run(img)
        torch.cuda.synchronize()
        ms["run"].append((time.perf_counter() - t0) * 1e3)
    res = ev.results()
    return {"instances_ms": spread(ms["instances"]), "add_maps_ms": spread(ms["host_gt_sync"]),
            "add_maps_device_gt_ms": spread(ms["device_gt_sync"]),
            "add_maps_device_gt_enqueue_ms": spread(ms["device_gt_enqueue"]), "run_ms": spread(ms["run"]),
            "live": int(maps.table["live"].sum()), "n_counted": res["All"]["n"]}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rounds", type=int, default=7)
    p.add_argument("--kernel_iters", type=int, default=100)
    p.add_argument("--image_calls", type=int, default=30)
    p.add_argument("--json", default=os.path.join(ROOT, "profiles", "probe_panoptic.json"))
    a = p.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("probe_panoptic needs a GPU: nothing is measured without one")
    result = {"unit_kernel": "us per call", "unit_per_image": "ms per image", "rounds": a.rounds,
              "kernel_iters": a.kernel_iters, "device": torch.cuda.get_device_name(0), "shape": [H, W]}
    k = result["kernel"] = kernels(a)
    for name in ("scene", "one_pair", "checkerboard", "limit"):
        r = k[name]
        print("cp_panoptic_pairs + cp_panoptic_match %dx%d %s (G = %d, n = %d, %d cells, %s): %.1f us [%.1f, %.1f]; pairs "
              "alone %.1f us, %.0f GB/s; torch.unique %.1f us [%.1f, %.1f]"
              % (W, H, name, r["G"], r["n"], r["cells"], r["regime"], r["us"]["median"], r["us"]["min"], r["us"]["max"],
                 r["pairs_only_us"]["median"], r["GBps"], r["torch_us"]["median"], r["torch_us"]["min"],
                 r["torch_us"]["max"]), flush=True)
    print("worst content: %s, %.2f x the scene" % (k["worst"], k["worst_over_scene"]), flush=True)
    r = result["per_image"] = {"cityscapes": per_image(a, seeded_weights())}["cityscapes"]
    print("--panoptic per image at %dx%d, K = 128: instances() %.3f ms + add_maps() %.3f ms [%.3f, %.3f] with the host id "
          "image, %.3f ms with it on the device, %.3f ms of host time without waiting (%d live); run() itself %.2f ms"
          % (H, W, r["instances_ms"]["median"], r["add_maps_ms"]["median"], r["add_maps_ms"]["min"],
             r["add_maps_ms"]["max"], r["add_maps_device_gt_ms"]["median"], r["add_maps_device_gt_enqueue_ms"]["median"],
             r["live"], r["run_ms"]["median"]), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()

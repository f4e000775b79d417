#!/usr/bin/env python3
"""Times the ground-truth painter on one MI355X against PIL on the same frame.

On a seeded synthetic frame of 2048 x 1024 with about 300 polygons of 4 to 400 vertices (IDD labels):
  * `cp_polygon_paint` alone between HIP events, the vertices already on the device (median [min, max] of --calls
    calls), and `instance_image` from the host object list to the device tensor;
  * the same frame drawn by PIL on the host with the scripts' call, ImageDraw.polygon(pts, fill=v) onto a mode I
    canvas (one thread; the scripts add the JSON parse and the PNG write around it);
  * `make_ground_truth.py` on --images copies of the frame written as files, with --workers workers: frames / s,
    PNG compression included.
The device image must equal PIL's or the probe stops.

Usage:  python tools/probe_ground_truth.py [--json OUT] [--calls 50] [--images 48] [--workers 4]
"""
import argparse
import ctypes
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, W = 1024, 2048
LABELS = ["road", "sidewalk", "building", "vegetation", "sky", "car", "person", "rider", "truck", "bus", "motorcycle",
          "autorickshaw", "pole", "billboard", "vehicle fallback"]


def make_objects(seed, n=300):
    """n polygons, 4 .. 400 vertices each: a few large surfaces first, then objects of a street scene's sizes."""
    rng = np.random.RandomState(seed)
    objects = []
    for k in range(n):
        m = int(rng.randint(4, 401))
        th = np.linspace(0, 2 * np.pi, m, endpoint=False)
        big = k < 12
        cx, cy = rng.uniform(0, W), rng.uniform(0, H) if big else rng.uniform(0.3 * H, 0.95 * H)
        r = (rng.uniform(0.3, 0.6) if big else rng.uniform(0.01, 0.12)) * H * rng.uniform(0.8, 1.2, m)
        pts = np.stack([cx + 1.5 * r * np.cos(th), cy + r * np.sin(th)], 1)
        objects.append({"label": LABELS[k % 5] if big else LABELS[5 + k % 10], "polygon": np.rint(pts).astype(int).tolist()})
    return objects


def stats(ms):
    ms = sorted(ms)
    return {"median_ms": ms[len(ms) // 2], "min_ms": ms[0], "max_ms": ms[-1]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default="")
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--images", type=int, default=48)
    ap.add_argument("--workers", type=int, default=4)
    a = ap.parse_args()
    import torch
    from PIL import Image, ImageDraw

    import make_ground_truth as mg
    from centerpoly_amd import _C
    from centerpoly_amd.datasets import ground_truth as gt
    if not torch.cuda.is_available():
        sys.exit("probe_ground_truth.py measures on a HIP device; none is visible")
    L = _C.lib()
    dev = torch.device("cuda:0")
    objects = make_objects(1)
    polygons, values, background = gt.paint_list(objects, "IDD", "instance", "id")
    res = {"canvas": [W, H], "polygons": len(polygons), "vertices": int(sum(len(p) for p in polygons))}

    # PIL on the host, the scripts' call
    host_ms = []
    for _ in range(3):
        t0 = time.perf_counter()
        img = Image.new("I", (W, H), background)
        drawer = ImageDraw.Draw(img)
        for p, v in zip(polygons, values):
            drawer.polygon([tuple(q) for q in p.tolist()], fill=v)
        host_ms.append((time.perf_counter() - t0) * 1e3)
    want = np.array(img).astype(np.int32)
    res["pil_host"] = stats(host_ms)

    # the kernel alone
    got = gt.paint(polygons, values, background, (W, H), dev)
    if not np.array_equal(got.cpu().numpy(), want):
        sys.exit("cp_polygon_paint differs from PIL on the probe's frame")
    n = len(polygons)
    first = np.concatenate([[0], np.cumsum([len(p) for p in polygons])]).astype(np.int32)
    xy = torch.from_numpy(np.concatenate(polygons)).to(dev)
    val = torch.from_numpy(np.asarray(values, np.int32)).to(dev)
    first_arr = (ctypes.c_int32 * (n + 1))(*first.tolist())
    nbytes = L.cp_polygon_paint_workspace_bytes(n, int(first[-1]))
    ws = _C.workspace(nbytes, dev)
    image = torch.empty((H, W), dtype=torch.int32, device=dev)

    def call():
        _C.check(L.cp_polygon_paint(_C.ptr(xy), first_arr, _C.ptr(val), n, background, H, W, _C.ptr(image), _C.ptr(ws),
                                    nbytes, _C.stream()), "cp_polygon_paint")
    for _ in range(5):
        call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(a.calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    res["cp_polygon_paint"] = stats(ms)
    res["written_GBps_at_median"] = 4.0 * H * W / (res["cp_polygon_paint"]["median_ms"] * 1e-3) / 1e9

    ms = []
    for _ in range(max(3, a.calls // 5)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        gt.instance_image(objects, (W, H), "IDD", "id", device=dev)
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    res["instance_image"] = stats(ms)

    # the driver on files
    tmp = tempfile.mkdtemp(prefix="probe_gt_")
    try:
        os.makedirs(os.path.join(tmp, "val", "7"))
        for i in range(a.images):
            with open(os.path.join(tmp, "val", "7", "%06d_gtFine_polygons.json" % i), "w") as f:
                json.dump({"imgHeight": H, "imgWidth": W, "objects": make_objects(1 + i % 4)}, f)
        opt = mg.parse_args(["--dataset", "IDD", "--gt_dir", os.path.join(tmp, "val"), "--num_workers", str(a.workers)])
        t0 = time.perf_counter()
        written = mg.run(opt)
        dt = time.perf_counter() - t0
        res["driver"] = {"frames": a.images, "images": len(written), "workers": a.workers, "frames_per_s": a.images / dt}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    print(json.dumps(res, indent=1, sort_keys=True))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()

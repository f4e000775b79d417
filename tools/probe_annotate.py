#!/usr/bin/env python3
"""Times the annotation recipe on one MI355X against its host statement on the same inputs.

At 1024 x 2048 and N = 32:
  * the `ids` path on a seeded id image of about 30 instances: `cp_annot_id_instances` and `cp_annot_rays_ids` alone
    between HIP events (median [min, max] of --calls calls), `from_id_image` from device-idle to host arrays;
  * the `polygons` path on a seeded object list of about 30 polygons: `cp_polygon_masks` and `cp_annot_rays_masks`
    alone, `from_polygons` from the host lists to host arrays;
  * the host statement (tests/golden/annotations_host.py, one thread, Python loops like the reference's tools), with
    the masks of the polygon path drawn by PIL as the tools draw them.  The reference's scripts cannot run here (cv2,
    bresenham, hard-coded paths): this is the only baseline.
  * `make_annotations.py` on --images copies of those inputs written as files, with --workers workers: images / s.
The device results must equal the host statement's or the probe stops.

Usage:  python tools/probe_annotate.py [--json OUT] [--calls 50] [--images 48] [--workers 4]
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
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

H, W, N = 1024, 2048, 32
LABELS = [24, 25, 26, 27, 28, 31, 32, 33]
NAMES = ["person", "rider", "car", "truck", "bus", "train", "motorcycle", "bicycle"]


def make_objects(seed, n=30):
    """n polygons of a street scene's sizes, 20 .. 120 vertices each."""
    rng = np.random.RandomState(seed)
    objects = [{"label": "road", "polygon": [[0, 600], [2047, 600], [2047, 1023], [0, 1023]]}]
    for k in range(n):
        m = rng.randint(20, 121)
        th = np.linspace(0, 2 * np.pi, m, endpoint=False)
        cx, cy = rng.uniform(0, W), rng.uniform(0.35 * H, 0.9 * H)
        r = rng.uniform(0.03, 0.2) * H * rng.uniform(0.8, 1.2, m)
        pts = np.stack([cx + 1.5 * r * np.cos(th), cy + r * np.sin(th)], 1)
        objects.append({"label": NAMES[k % 8] if k % 6 else "pole", "polygon": np.rint(pts).astype(int).tolist()})
    return objects


def make_ids(objects):
    """The id image of those objects, drawn back to front (the last one is nearest)."""
    from PIL import Image, ImageDraw
    img = Image.new("I;16", (W, H), 0)
    d = ImageDraw.Draw(img)
    for k, o in enumerate(objects):
        if o["label"] in NAMES:
            d.polygon([tuple(p) for p in o["polygon"]], fill=LABELS[NAMES.index(o["label"])] * 256 + k)
    return np.array(img).astype(np.uint16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default="")
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--images", type=int, default=48)
    ap.add_argument("--workers", type=int, default=4)
    a = ap.parse_args()
    import torch

    import annotations_host as host
    import make_annotations as ma
    from centerpoly_amd import _C
    from centerpoly_amd.datasets import annotate
    from centerpoly_amd.datasets.dataset.polygons import CITYSCAPES
    if not torch.cuda.is_available():
        sys.exit("probe_annotate.py measures on a HIP device; none is visible")
    L = _C.lib()
    dev = torch.device("cuda:0")
    have = list(CITYSCAPES.class_name[1:])
    objects = make_objects(3)
    ids = make_ids(objects)
    out = {"device": torch.cuda.get_device_name(0), "H": H, "W": W, "N": N, "calls": a.calls}

    def timed(fn):
        ms = []
        for _ in range(a.calls):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        ms = sorted(ms[a.calls // 5:])                    # the first fifth warms up
        return [ms[len(ms) // 2], ms[0], ms[-1]]

    def wall(fn, reps):
        ts = []
        for _ in range(reps + 2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        ts = sorted(ts[2:])
        return [ts[len(ts) // 2], ts[0], ts[-1]], res

    # ---- ids
    ids_dev = torch.from_numpy(ids.view(np.int16)).to(dev)
    lab = (ctypes.c_int32 * 8)(*LABELS)
    head = torch.empty((1 + 6 * 1024,), dtype=torch.int32, device=dev)
    ws = _C.workspace(L.cp_annot_id_instances_workspace_bytes(), dev)
    k_inst = timed(lambda: _C.check(L.cp_annot_id_instances(
        _C.ptr(ids_dev), H, W, lab, 8, 256, 1024, _C.ptr(head[:1]), _C.ptr(head[1:1025]), _C.ptr(head[1025:2049]),
        _C.ptr(head[2049:]), _C.ptr(ws), ws.numel(), _C.stream()), "instances"))
    n = int(head[0].item())
    box = head[2049:].view(1024, 4)[:n].to(torch.float64).contiguous()
    poly = torch.empty((n, N, 2), dtype=torch.int32, device=dev)
    k_rays = timed(lambda: _C.check(L.cp_annot_rays_ids(
        _C.ptr(ids_dev), H, W, _C.ptr(head[1:1025]), _C.ptr(box), n, N, _C.ptr(poly), _C.stream()), "rays"))
    lib_ms, res = wall(lambda: annotate.from_id_image(ids_dev, LABELS, 256, N), 10)
    t0 = time.perf_counter()
    ref = host.from_id_image(ids, LABELS, 256, N)
    host_ms = (time.perf_counter() - t0) * 1e3
    if not (np.array_equal(res["poly"], ref["poly"]) and np.array_equal(res["bbox"], ref["bbox"])):
        sys.exit("the ids path differs from the host statement")
    out["ids"] = {"instances": n, "id_instances_ms": k_inst, "rays_ms": k_rays, "from_id_image_ms": lib_ms,
                  "host_statement_ms": host_ms, "id_image_bytes": H * W * 2,
                  "id_instances_GBps": H * W * 2 / (k_inst[0] * 1e-3) / 1e9}
    print(json.dumps(out["ids"]), flush=True)

    # ---- polygons
    kept = annotate.kept_objects(objects, have)
    m = len(kept)
    verts = [np.asarray(p, np.int32) for _, p in kept]
    first = np.cumsum([0] + [len(v) for v in verts])
    xy = torch.from_numpy(np.concatenate(verts)).to(dev)
    masks = torch.empty((m, H, W), dtype=torch.uint8, device=dev)
    cnt = torch.empty((m,), dtype=torch.int32, device=dev)
    nbytes = L.cp_polygon_masks_workspace_bytes(m, int(first[-1]))
    ws2 = _C.workspace(nbytes, dev)
    first_arr = (ctypes.c_int32 * (m + 1))(*first.tolist())
    k_masks = timed(lambda: _C.check(L.cp_polygon_masks(
        _C.ptr(xy), first_arr, m, H, W, _C.ptr(masks), _C.ptr(cnt), _C.ptr(ws2), nbytes, _C.stream()), "masks"))
    pbox = torch.from_numpy(np.array([host.polygon_box(p) for _, p in kept], np.float64)).to(dev)
    ppoly = torch.empty((m, N, 2), dtype=torch.int32, device=dev)
    k_prays = timed(lambda: _C.check(L.cp_annot_rays_masks(
        _C.ptr(masks), H, W, _C.ptr(pbox), m, N, _C.ptr(ppoly), _C.stream()), "rays"))
    plib_ms, pres = wall(lambda: annotate.from_polygons(objects, (W, H), have, N, device=dev), 10)
    from PIL import Image, ImageDraw
    t0 = time.perf_counter()
    pil = []
    for _, p in kept:
        im = Image.new("L", (W, H), 0)
        ImageDraw.Draw(im).polygon([tuple(q) for q in p], outline=0, fill=255)
        pil.append(np.array(im))
    pref = host.from_polygons(objects, (W, H), have, N, pil)
    phost_ms = (time.perf_counter() - t0) * 1e3
    if not (np.array_equal(pres["poly"], pref["poly"]) and np.array_equal(masks.cpu().numpy(), np.stack(pil))):
        sys.exit("the polygons path differs from PIL and the host statement")
    out["polygons"] = {"objects": m, "vertices": int(first[-1]), "polygon_masks_ms": k_masks, "rays_ms": k_prays,
                       "from_polygons_ms": plib_ms, "host_statement_with_pil_masks_ms": phost_ms,
                       "mask_bytes": m * H * W, "polygon_masks_GBps_of_2_passes": 2 * m * H * W / (k_masks[0] * 1e-3) / 1e9}
    print(json.dumps(out["polygons"]), flush=True)

    # ---- the driver: files in, files out
    tmp = tempfile.mkdtemp(prefix="probe_annotate_")
    try:
        img_dir, gt_dir = os.path.join(tmp, "leftImg8bit", "train"), os.path.join(tmp, "gtFine", "train")
        os.makedirs(os.path.join(img_dir, "c"))
        os.makedirs(os.path.join(gt_dir, "c"))
        small = Image.new("RGB", (8, 4))
        for i in range(a.images):
            small.save(os.path.join(img_dir, "c", "c_%06d_000019_leftImg8bit.png" % i))
            with open(os.path.join(gt_dir, "c", "c_%06d_000019_gtFine_polygons.json" % i), "w") as f:
                json.dump({"imgHeight": H, "imgWidth": W, "objects": make_objects(100 + i)}, f)
            Image.fromarray(make_ids(make_objects(100 + i))).save(
                os.path.join(gt_dir, "c", "c_%06d_000019_gtFine_instanceIds.png" % i))
        out["driver"] = {"images": a.images, "workers": a.workers}
        for source, extra in (("polygons", []), ("ids", ["--id_divisor", "256"])):
            opt = ma.parse_args(["--dataset", "cityscapes", "--source", source, "--img_dir", img_dir, "--gt_dir", gt_dir,
                                 "--out_dir", os.path.join(tmp, "out_" + source), "--nbr_points", str(N),
                                 "--num_workers", str(a.workers)] + extra)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ma.run(opt)
            out["driver"][source + "_images_per_s"] = a.images / (time.perf_counter() - t0)
        print(json.dumps(out["driver"]), flush=True)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()

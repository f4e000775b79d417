#!/usr/bin/env python3
"""Times the KITTI / IDD scoring tail on one MI355X against the same work done the reference's way.

Per shape (canvas, live instances; seeded 16-gons of a street scene's sizes in 3 classes, a seeded id image):
  * `cp_class_instance_masks` alone between HIP events (median [min, max] of --calls calls) and the bytes it is
    bound by: n * H * W mask bytes written by the fill kernel, read and written again by the occlusion kernel;
  * `cp_class_writer_instances` alone;
  * the whole tail, wall clock from device-idle to "count tables on the host": `score_instances_device`
    (selection, masks, `cp_instance_overlaps`, one read);
  * the reference's way on this host, one thread as its loop is: the PIL drawing loop of
    format_and_write_to_kitti (no file output) and the evaluator's counting (one np.logical_and + count_nonzero per
    (mask, ground-truth instance) pair and the void overlap, as assignGt2Preds does).
The two ways must give the same masks and the same counts or the probe stops.

Usage:  python tools/probe_class_masks.py [--json OUT] [--calls 50] [--images 5]
"""
import argparse
import ctypes
import json
import os
import sys
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(1242, 375, 32), (1242, 375, 128), (1920, 1080, 32), (1920, 1080, 128)]


def make_rows(W, H, n, seed):
    rng = np.random.RandomState(seed)
    N = 16
    rows = np.zeros((n, 2 * N + 7), np.float32)
    th = np.linspace(0, 2 * np.pi, N, endpoint=False)
    for k in range(n):
        cx, cy = rng.uniform(0, W), rng.uniform(0.3 * H, 0.9 * H)
        r = rng.uniform(0.03, 0.15) * H * rng.uniform(0.7, 1.3, N)
        pts = np.stack([cx + 1.6 * r * np.cos(th), cy + r * np.sin(th)], 1)
        rows[k, 6:6 + 2 * N] = pts.reshape(-1)
        rows[k, 0:2], rows[k, 2:4] = pts.min(0), pts.max(0)
        rows[k, 4] = rng.uniform(0.31, 1.0)
        rows[k, 5] = rng.choice([0, 2, 7])
        rows[k, -1] = rng.uniform(1.0, 60.0)
    return rows


def reference_way(ds, rows, gt, table, void_ids):
    """The PIL loop and the evaluator's counting on the host: (seconds drawing, seconds counting, masks, tables)."""
    from PIL import Image, ImageDraw
    H, W = gt.shape
    per_class = {c + 1: np.delete(rows[rows[:, 5] == c], 5, axis=1) for c in range(8)}
    t0 = time.perf_counter()
    masks, count = {}, 0
    thresh = np.float32(ds.opt.thresh)
    for cls_ind in per_class:
        param_list = []
        to_remove = Image.new("L", (W, H), 1)
        for bbox in per_class[cls_ind]:
            if bbox[4] > thresh:
                polygon = [float("{:.2f}".format(v)) for v in bbox[5:-1]]
                param_list.append((polygon, count, bbox[4], bbox[-1]))
                count += 1
        for polygon, k, score, depth in sorted(param_list, key=lambda x: x[-1]):
            pts = [(int(polygon[i]), int(polygon[i + 1])) for i in range(0, len(polygon), 2)]
            m = Image.new("L", (W, H), 0)
            ImageDraw.Draw(m).polygon(pts, outline=0, fill=255)
            m = Image.fromarray(np.array(m) * np.array(to_remove))
            if float(score) >= 0.5:
                ImageDraw.Draw(to_remove).polygon(pts, outline=0, fill=0)
            masks[k] = np.array(m)
    t1 = time.perf_counter()
    bool_void = np.isin(gt, [v for v in void_ids if v >= 0])
    inter = np.zeros((count, len(table)), np.int64)
    void = np.zeros(count, np.int64)
    for k in range(count):
        pred = masks[k] != 0
        void[k] = np.count_nonzero(np.logical_and(bool_void, pred))
        for j, inst in enumerate(table[:, 0]):
            inter[k, j] = np.count_nonzero(np.logical_and(gt == inst, pred))
    t2 = time.perf_counter()
    return t1 - t0, t2 - t1, masks, inter, void


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default="")
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--images", type=int, default=5)
    a = ap.parse_args()
    import torch

    from centerpoly_amd import _C
    from centerpoly_amd.datasets.dataset.polygons import KITTIPOLY
    from centerpoly_amd.datasets.evaluation import instance_level as il
    ds = KITTIPOLY.__new__(KITTIPOLY)
    ds.opt = types.SimpleNamespace(thresh=0.3)
    L = _C.lib()
    out = {"device": torch.cuda.get_device_name(0), "calls": a.calls, "images": a.images, "shapes": []}

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

    for W, H, n in SHAPES:
        rows = make_rows(W, H, n, 11)
        rng = np.random.RandomState(5)
        gt = np.full((H, W), 7, np.uint16)
        for k in range(24):                                # 24 ground-truth boxes in KITTI's encoding, a void strip
            x, y = rng.randint(0, W - 40), rng.randint(H // 3, H - 30)
            gt[y:y + rng.randint(20, H // 4), x:x + rng.randint(30, W // 6)] = [24, 26, 33][k % 3] * 256 + k
        gt[:, :W // 10] = 3
        table = il.gt_instances(np.bincount(gt.reshape(-1), minlength=65536), il.KITTI)
        rows_dev = torch.from_numpy(rows).cuda()
        gt_dev = torch.from_numpy(gt.view(np.int16)).cuda()
        params = ds.image_instances({c + 1: np.delete(rows[rows[:, 5] == c], 5, axis=1) for c in range(8)})
        N = 16
        poly = torch.tensor([p[0] for p in params], dtype=torch.int32).reshape(n, N, 2).cuda()
        group = torch.tensor([p[2] for p in params], dtype=torch.int32).cuda()
        flags = torch.tensor([1 | (2 if p[1] >= 0.5 else 0) for p in params], dtype=torch.uint8).cuda()
        masks = torch.empty((n, H, W), dtype=torch.uint8, device="cuda")
        counts = torch.empty((n,), dtype=torch.int32, device="cuda")
        k_masks = timed(lambda: _C.check(L.cp_class_instance_masks(
            _C.ptr(poly), _C.ptr(group), _C.ptr(flags), n, N, H, W, _C.ptr(masks), _C.ptr(counts), _C.stream()), "masks"))
        i32 = lambda *s: torch.empty(s, dtype=torch.int32, device="cuda")      # noqa: E731
        bufs = [i32(1), i32(n), i32(n, N, 2), i32(n), torch.empty((n,), dtype=torch.uint8, device="cuda"), i32(n),
                torch.empty((n,), dtype=torch.float32, device="cuda"), i32(n)]
        tab = np.ascontiguousarray(ds.class_label_table())
        k_sel = timed(lambda: _C.check(L.cp_class_writer_instances(
            _C.ptr(rows_dev), n, N, 0.3, 0, tab.ctypes.data_as(ctypes.c_void_p), len(tab),
            *[_C.ptr(b) for b in bufs], _C.stream()), "selection"))
        tail = []
        for _ in range(a.images + 2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = ds.score_instances_device(rows_dev, gt_dev, gt_table=table)
            tail.append((time.perf_counter() - t0) * 1e3)
        tail = sorted(tail[2:])
        draw, count = [], []
        for _ in range(max(1, a.images // 2)):
            d, c, ref_masks, ref_inter, ref_void = reference_way(ds, rows, gt, table, il.KITTI.void_ids)
            draw.append(d * 1e3)
            count.append(c * 1e3)
        dev_masks = masks.cpu().numpy()
        for p, m in zip(params, dev_masks):
            if not np.array_equal(m, ref_masks[p[4]]):
                sys.exit("device mask of text line %d differs from PIL's at %dx%d" % (p[4], W, H))
        if not (np.array_equal(res["inter"], ref_inter) and np.array_equal(res["void"], ref_void)):
            sys.exit("count tables differ at %dx%d n=%d" % (W, H, n))
        nbytes = n * H * W
        rec = {"W": W, "H": H, "n": n, "mask_bytes": nbytes, "masks_ms": k_masks, "selection_ms": k_sel,
               "masks_GBps_of_3_passes": 3 * nbytes / (k_masks[0] * 1e-3) / 1e9,
               "tail_ms": [tail[len(tail) // 2], tail[0], tail[-1]],
               "pil_draw_ms": [float(np.median(draw)), min(draw), max(draw)],
               "numpy_count_ms": [float(np.median(count)), min(count), max(count)], "gt_instances": int(len(table))}
        out["shapes"].append(rec)
        print(json.dumps(rec), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Times the detection overlay on one MI355X against drawing the same instances on the host.

Per shape (canvas, live instances; seeded 16-gons of a street scene's sizes, all above the threshold):
  * `cp_writer_instances` + `cp_render_overlay` between HIP events, in place on a device image: median [min, max] of
    --calls launches after --warmup;
  * the host's way in the same process, wall clock, median of --host-runs: the rows copied back from the device, one
    `ImageDraw` pass over the host image (translucent polygon with outline, box, label background and text per
    instance, farthest first -- PIL's own primitives, the cheapest host drawing of the same content, not the same
    bits) and the finished picture uploaded again;
  * the host statement of the tests (tests/golden/render_host.py: exact, built for clarity, not for speed), once.
The device picture must equal the host statement or the probe stops.

Usage:  python tools/probe_render.py [--json OUT] [--calls 200] [--warmup 20] [--host-runs 5]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

SHAPES = [(2048, 1024, 128), (1242, 375, 32)]
NAMES = ["person", "rider", "car", "truck", "bus", "train", "motorcycle", "bicycle"]
N = 16


def make_rows(W, H, n, seed):
    rng = np.random.RandomState(seed)
    rows = np.zeros((n, 2 * N + 7), np.float32)
    th = np.linspace(0, 2 * np.pi, N, endpoint=False)
    for k in range(n):
        cx, cy = rng.uniform(0, W), rng.uniform(0.3 * H, 0.9 * H)
        r = rng.uniform(0.03, 0.15) * H * rng.uniform(0.7, 1.3, N)
        pts = np.stack([cx + 1.6 * r * np.cos(th), cy + r * np.sin(th)], 1)
        rows[k, 6:6 + 2 * N] = pts.reshape(-1)
        rows[k, 0:2], rows[k, 2:4] = pts.min(0), pts.max(0)
        rows[k, 4] = rng.uniform(0.31, 1.0)
        rows[k, 5] = rng.randint(0, 8)
        rows[k, -1] = rng.uniform(1.0, 60.0)
    return rows


def pil_draw(image, rows, thresh, palette):
    """One ImageDraw pass: the same content with PIL's own primitives."""
    import render_host as rh
    from PIL import Image, ImageDraw, ImageFont
    font = ImageFont.load_default_imagefont()
    im = Image.fromarray(image)
    draw = ImageDraw.Draw(im, "RGBA")
    for _, cls, score, pts, (x1, y1, x2, y2) in reversed(rh.instances(rows, thresh, len(NAMES))):
        col = tuple(int(v) for v in palette[cls])
        draw.polygon(pts, fill=col + (102,), outline=(0, 255, 255, 255), width=3)
        draw.rectangle([x1, y1, x2, y2], outline=col + (255,), width=2)
        text = rh.label(NAMES[cls], score)
        draw.rectangle([x1, y1 - 12, x1 + 6 * len(text) - 1, y1 - 2], fill=col + (255,))
        draw.text((x1, y1 - 12), text, fill=(0, 0, 0, 255), font=font)
    return np.asarray(im)


def main():
    import torch

    import render_host as rh
    from centerpoly_amd import _C
    from centerpoly_amd.utils import debugger as dbg
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default="")
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--host-runs", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda")
    L = _C.lib()
    d = dbg.Debugger(NAMES, theme="black", device=dev)
    palette = d.palette_bgr
    out = {"device": torch.cuda.get_device_name(0), "calls": args.calls, "warmup": args.warmup, "shapes": []}
    for W, H, n in SHAPES:
        rows = make_rows(W, H, n, 100 + n)
        rng = np.random.RandomState(n)
        image = rng.randint(0, 256, (H, W, 3)).astype(np.uint8)
        rows_dev = torch.from_numpy(rows).to(dev)
        # correctness first: the Debugger's picture against the host statement
        d.add_img(image, "p")
        d.add_polydet_detections(rows_dev, rows, 0.3, img_id="p")
        t0 = time.perf_counter()
        want, _ = rh.overlay(image, rows, 0.3, NAMES, palette)
        t_statement = time.perf_counter() - t0
        if d.last_n != n or not np.array_equal(d.imgs["p"].cpu().numpy(), want):
            raise SystemExit("the device picture differs from the host statement at %dx%d, %d" % (W, H, n))
        # device: selection + overlay between events, in place
        R = n
        img_dev = torch.from_numpy(image).to(dev)
        ints = torch.empty((1 + 2 * R + (R + 3) // 4,), dtype=torch.int32, device=dev)
        conf = torch.empty((R,), dtype=torch.float32, device=dev)
        poly = torch.empty((R, N, 2), dtype=torch.int32, device=dev)
        codes = torch.from_numpy(d.row_labels(rows)).to(dev)
        pal_dev, atlas_dev = d._tables()
        table = np.ascontiguousarray(np.stack([np.arange(8), np.ones(8)], 1), np.int32)
        prm = _C.OverlayParams(dbg.FILL_ALPHA, dbg.OUTLINE_RADIUS, dbg.BOX_THICKNESS, 0, 1, 1)
        prm.outline_colour[:] = (0, 255, 255)
        nbytes = L.cp_render_overlay_workspace_bytes(H, W)
        ws = _C.workspace(nbytes, dev)
        at = lambda o: ctypes.c_void_p(ints.data_ptr() + 4 * o)           # noqa: E731
        st = _C.stream()

        def launch():
            _C.check(L.cp_writer_instances(_C.ptr(rows_dev), R, N, 0.3, table.ctypes.data_as(ctypes.c_void_p), 8,
                                           at(0), at(1), _C.ptr(poly), at(1 + 2 * R), at(1 + R), _C.ptr(conf), st),
                     "cp_writer_instances")
            _C.check(L.cp_render_overlay(_C.ptr(img_dev), H, W, _C.ptr(rows_dev), R, N, at(0), at(1), _C.ptr(poly),
                                         _C.ptr(pal_dev), 8, _C.ptr(codes), 16, _C.ptr(atlas_dev), 96,
                                         ctypes.byref(prm), _C.ptr(img_dev), _C.ptr(ws), nbytes, st),
                     "cp_render_overlay")
        for _ in range(args.warmup):
            launch()
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.calls):
            img_dev.copy_(torch.from_numpy(image), non_blocking=False)    # a fresh image, outside the events
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            launch()
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        # host: rows down, one ImageDraw pass, picture up
        host = []
        for _ in range(args.host_runs):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = rows_dev.cpu().numpy()
            pic = pil_draw(image, r, 0.3, palette)
            torch.from_numpy(np.ascontiguousarray(pic)).to(dev)
            torch.cuda.synchronize()
            host.append((time.perf_counter() - t0) * 1e3)
        rec = {"canvas": [W, H], "instances": n,
               "device_ms": {"median": float(np.median(ms)), "min": float(np.min(ms)), "max": float(np.max(ms))},
               "host_pil_ms": {"median": float(np.median(host)), "min": float(np.min(host)), "max": float(np.max(host))},
               "host_statement_ms": t_statement * 1e3}
        out["shapes"].append(rec)
        print("%dx%d, %d instances: device %.3f ms [%.3f, %.3f]; host PIL pass %.1f ms [%.1f, %.1f]; host statement "
              "%.0f ms" % (W, H, n, rec["device_ms"]["median"], rec["device_ms"]["min"], rec["device_ms"]["max"],
                           rec["host_pil_ms"]["median"], rec["host_pil_ms"]["min"], rec["host_pil_ms"]["max"],
                           rec["host_statement_ms"]), flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()

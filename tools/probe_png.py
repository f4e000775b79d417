"""GPU probe: what --device_png costs and saves (cp_png_deflate; utils.png.encode with the read-back; save_masks,
save_ids and make_ground_truth.py with the flag on and off).

All at 2048 x 1024 on the street scene of tools/probe_instances.py (128 seeded 16-gons drawn by the KITTI writer:
`InstanceMaps.masks`, `.ids`, `.labels`), HIP events around `--kernel_iters` calls, median and [min, max] over
`--rounds`; the wall-clock cases are per call over `--image_calls` calls, files written to --tmp.
1. cp_png_deflate alone, nothing read back, at the wrapper's first capacity: the 128 planes without bounds and with the
   polygons' bounds, and the one 16-bit id image.
2. utils.png.encode with the read-back and the framing (wall clock); the host's share alone: CRC-32 and framing of the
   streams, and writing the files.
3. instances.save_masks and instances.save_ids per image with the flag on and off (the flag-off path is PIL's, as
   before), and the bytes of the files either way.
4. make_ground_truth.py on --images copies of tools/probe_ground_truth.py's frame with --workers workers, frames per
   second with the flag on and off.

Usage:  python tools/probe_png.py [--json profiles/probe_png.json]
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.probe_instances import H, W, spread, timed
from tools.probe_rle import scene_maps, wall


def raw_deflate(planes, images, bits, bounds, cap):
    """A closure that issues cp_png_deflate on fixed buffers, and (out, table, head)."""
    import torch
    from centerpoly_amd import _C
    src = planes if planes is not None else images
    L, dev = _C.lib(), src.device
    n = int(src.shape[0])
    out = torch.empty((cap + 16,), dtype=torch.uint8, device=dev)
    table = torch.empty((n, 4), dtype=torch.int32, device=dev)
    head = torch.empty((4,), dtype=torch.int32, device=dev)
    nbytes = L.cp_png_deflate_workspace_bytes(n, H, W, bits)
    ws = _C.workspace(nbytes, dev)

    def call():
        _C.check(L.cp_png_deflate(_C.ptr(planes), _C.ptr(images), n, H, W, bits, _C.ptr(bounds), _C.ptr(out), cap,
                                  _C.ptr(table), _C.ptr(head), _C.ptr(ws), nbytes, _C.stream()), "cp_png_deflate")
    return call, (out, table, head), nbytes


def dir_bytes(path):
    return sum(os.path.getsize(os.path.join(r, f)) for r, _, fs in os.walk(path) for f in fs if f.endswith(".png"))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rounds", type=int, default=7)
    p.add_argument("--kernel_iters", type=int, default=20)
    p.add_argument("--image_calls", type=int, default=7)
    p.add_argument("--images", type=int, default=24)
    p.add_argument("--workers", type=int, default=4)
    p.add_argument("--json", default=os.path.join(ROOT, "profiles", "probe_png.json"))
    p.add_argument("--tmp", default="")
    a = p.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("probe_png needs a GPU: nothing is measured without one")
    from centerpoly_amd.detectors import instances
    from centerpoly_amd.utils import png
    dev = torch.device("cuda")
    maps = scene_maps()
    t = maps.table
    n = int(t["n"])
    masks = maps.masks[:n]
    bounds = instances.vertex_bounds_host(t["poly"], instances.MARGIN[maps.family], maps.canvas)
    b_dev = torch.from_numpy(bounds).to(dev)
    ids = maps.ids.to(torch.int32)[None].contiguous()
    result = {"unit_kernel": "us per call", "unit_wall": "ms per call", "rounds": a.rounds, "kernel_iters": a.kernel_iters,
              "device": torch.cuda.get_device_name(0), "shape": [H, W], "n": n}
    fmt = lambda r, u="us": "%.1f %s [%.1f, %.1f]" % (r["median"], u, r["min"], r["max"])              # noqa: E731

    # 1. the kernels alone
    raw = H * (1 + W)
    cap = n * (raw // png.FIRST_DIVISOR + png.FIRST_FLOOR)
    cap16 = H * (1 + 2 * W) // png.FIRST_DIVISOR + png.FIRST_FLOOR
    k = result["deflate"] = {}
    for name, (pl, im, bits, bd, c) in {"planes": (masks, None, 8, None, cap), "planes_bounds": (masks, None, 8, b_dev, cap),
                                        "ids16": (None, ids, 16, None, cap16)}.items():
        call, (out, table, head), nbytes = raw_deflate(pl, im, bits, bd, c)
        us = timed(call, a.kernel_iters, a.rounds)
        h = head.cpu().numpy()
        k[name] = {"us": us, "total_bytes": int(h[0]), "overflow": int(h[1]), "cap_bytes": c, "workspace_bytes": int(nbytes),
                   "raw_bytes": int((n if pl is not None else 1) * H * W * bits // 8)}
        print("cp_png_deflate %s: %s; %d bytes of streams for %d raw (overflow %d)"
              % (name, fmt(us), h[0], k[name]["raw_bytes"], h[1]), flush=True)

    # 2. with the read-back, and the host's share
    result["encode_ms"] = wall(lambda: png.encode(planes=masks, bounds=bounds), a.image_calls)
    result["encode_no_bounds_ms"] = wall(lambda: png.encode(planes=masks), a.image_calls)
    streams = png.zlib_stream(planes=masks, bounds=bounds)
    tmp = a.tmp or tempfile.mkdtemp(prefix="probe_png_")
    files = [png.frame(s, W, H, 8) for s in streams]

    def frame_all():
        return [png.frame(s, W, H, 8) for s in streams]

    def write_all():
        for i, data in enumerate(files):
            with open(os.path.join(tmp, "w_%d.png" % i), "wb") as f:
                f.write(data)
    result["host_crc_frame_ms"] = wall(frame_all, a.image_calls)
    result["host_write_ms"] = wall(write_all, a.image_calls)
    print("utils.png.encode of the %d planes with the read-back: %s with bounds, %s without; of that the CRC-32 and "
          "framing %s, and writing the files %s" % (n, fmt(result["encode_ms"], "ms"), fmt(result["encode_no_bounds_ms"], "ms"),
                                                    fmt(result["host_crc_frame_ms"], "ms"), fmt(result["host_write_ms"], "ms")),
          flush=True)

    # 3. the writers, the flag on and off
    for name, fn in (("save_masks", instances.save_masks), ("save_ids", instances.save_ids)):
        for flag in (True, False):
            d = os.path.join(tmp, "%s_%d" % (name, flag))
            key = "%s_%s" % (name, "device" if flag else "pil")
            result[key + "_ms"] = wall(lambda: fn(maps, d, "scene", device_png=flag), a.image_calls if flag else 3)
            result[key + "_png_bytes"] = dir_bytes(d)
        print("%s per image: %s with --device_png (%d bytes of PNG), %s without (%d bytes)"
              % (name, fmt(result[name + "_device_ms"], "ms"), result[name + "_device_png_bytes"],
                 fmt(result[name + "_pil_ms"], "ms"), result[name + "_pil_png_bytes"]), flush=True)

    # 4. the ground-truth driver on files
    import make_ground_truth as mg
    from tools.probe_ground_truth import make_objects
    gt = os.path.join(tmp, "val", "7")
    os.makedirs(gt)
    for i in range(a.images):
        with open(os.path.join(gt, "%06d_gtFine_polygons.json" % i), "w") as f:
            json.dump({"imgHeight": H, "imgWidth": W, "objects": make_objects(1 + i % 4)}, f)
    result["make_ground_truth"] = {"frames": a.images, "workers": a.workers}
    for flag in (True, False):
        fps = []
        for _ in range(3):
            out_dir = os.path.join(tmp, "gt_out_%d" % flag)
            opt = mg.parse_args(["--dataset", "IDD", "--gt_dir", os.path.join(tmp, "val"), "--num_workers", str(a.workers),
                                 "--out_dir", out_dir] + (["--device_png"] if flag else []))
            t0 = time.perf_counter()
            mg.run(opt)
            fps.append(a.images / (time.perf_counter() - t0))
        result["make_ground_truth"]["device" if flag else "pil"] = dict(spread(fps), png_bytes=dir_bytes(out_dir))
    g = result["make_ground_truth"]
    print("make_ground_truth.py, %d frames, %d workers: %s with --device_png (%d bytes), %s without (%d bytes)"
          % (a.images, a.workers, fmt(g["device"], "frames/s"), g["device"]["png_bytes"], fmt(g["pil"], "frames/s"),
             g["pil"]["png_bytes"]), flush=True)
    if not a.tmp:
        shutil.rmtree(tmp, ignore_errors=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()

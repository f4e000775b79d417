"""GPU probe: what the run-length masks cost (cp_rle_encode, cp_rle_decode; the torch statement of the same counts; the
host statement on planes read back; --save_rle beside --save_masks per image).

All at 2048 x 1024 on the street scene of tools/probe_instances.py (128 seeded 16-gons of 40 to 120 pixels radius, drawn
by the KITTI writer: `InstanceMaps.masks` and `.index`), HIP events around `--kernel_iters` calls, median and [min, max]
over `--rounds`; the wall-clock cases are per call over `--image_calls` calls.
1. cp_rle_encode alone, nothing read back, the capacities of the wrapper's first call:
     planes          the 128 planes, no bounds        planes_bounds   with the polygons' bounds
     index           the 128 slots of the owner map, with the boxes of the owned pixels (the MOTS case)
     checkerboard    one plane, every pixel a change: m = H * W counts, the capacities sized for them
2. cp_rle_decode of the scene's 128 strings (the counts already on the device).
3. The same counts from torch ops on the device (transpose, diff, nonzero per plane), checked against the kernel's.
4. utils.rle.encode with the read-back (wall clock), beside the host way: the 128 planes copied to the host and numpy's
   vectorised counts (transpose, diff, flatnonzero) there, copy included.  How often the wrapper's second call fired.
5. instances.save_rle beside instances.save_masks per image (wall clock, the files written to --tmp).

Usage:  python tools/probe_rle.py [--json profiles/probe_rle.json]
"""
import argparse
import ctypes
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

from tools.probe_instances import H, W, realistic_rows, spread, timed


def scene_maps():
    import torch
    from centerpoly_amd.datasets.dataset_factory import dataset_factory
    from centerpoly_amd.detectors import instances
    rows = torch.from_numpy(realistic_rows()).cuda()
    return instances.instance_maps(rows, dataset_factory["kitti_poly"], (W, H), thresh=0.05)


def raw_encoder(planes, index, n, bounds, cap_counts, cap_bytes):
    """A closure that issues cp_rle_encode on fixed buffers, and the buffers (counts, chars, table, head)."""
    import torch
    from centerpoly_amd import _C
    L, dev = _C.lib(), (planes if planes is not None else index).device
    counts = torch.empty((max(cap_counts, 1),), dtype=torch.int32, device=dev)
    chars = torch.empty((max(cap_bytes, 1),), dtype=torch.uint8, device=dev)
    table = torch.empty((n, 4), dtype=torch.int32, device=dev)
    head = torch.empty((4,), dtype=torch.int32, device=dev)
    nbytes = L.cp_rle_encode_workspace_bytes(n, H, W, cap_counts)
    ws = _C.workspace(nbytes, dev)

    def call():
        _C.check(L.cp_rle_encode(_C.ptr(planes), _C.ptr(index), n, H, W, _C.ptr(bounds), _C.ptr(counts), cap_counts,
                                 _C.ptr(chars), cap_bytes, _C.ptr(table), _C.ptr(head), _C.ptr(ws), nbytes, _C.stream()),
                 "cp_rle_encode")
    return call, (counts, chars, table, head), nbytes


def torch_counts(plane):
    """The counts of one device plane from torch ops: positions of the changes in column-major order, differences."""
    import torch
    flat = (plane.t() != 0).reshape(-1).to(torch.int8)
    change = torch.nonzero(torch.diff(flat, prepend=flat.new_zeros(1)) != 0).reshape(-1)
    ends = torch.cat([change, change.new_full((1,), flat.numel())])
    return torch.diff(ends, prepend=ends.new_zeros(1))


def numpy_counts(plane):
    flat = (plane.T != 0).reshape(-1).astype(np.int8)
    change = np.flatnonzero(np.diff(flat, prepend=np.int8(0)))
    return np.diff(np.concatenate([[0], change, [flat.size]]))


def wall(call, calls):
    import torch
    ms = []
    for i in range(3 + calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        if i >= 3:
            ms.append((time.perf_counter() - t0) * 1e3)
    return spread(ms)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rounds", type=int, default=7)
    p.add_argument("--kernel_iters", type=int, default=20)
    p.add_argument("--image_calls", type=int, default=10)
    p.add_argument("--json", default=os.path.join(ROOT, "profiles", "probe_rle.json"))
    p.add_argument("--tmp", default="")
    a = p.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("probe_rle needs a GPU: nothing is measured without one")
    from centerpoly_amd import _C
    from centerpoly_amd.detectors import instances
    from centerpoly_amd.utils import rle
    dev = torch.device("cuda")
    maps = scene_maps()
    t = maps.table
    n = int(t["n"])
    masks = maps.masks[:n]
    poly_bounds = instances.vertex_bounds_host(t["poly"], instances.MARGIN[maps.family], maps.canvas)
    own_bounds = np.ascontiguousarray(t["box"], np.int32).reshape(n, 4)
    result = {"unit_kernel": "us per call", "unit_wall": "ms per call", "rounds": a.rounds, "kernel_iters": a.kernel_iters,
              "device": torch.cuda.get_device_name(0), "shape": [H, W], "n": n}
    fmt = lambda r, u="us": "%.1f %s [%.1f, %.1f]" % (r["median"], u, r["min"], r["max"])              # noqa: E731

    # 1. the kernel alone
    enc = result["encode"] = {}
    cases = {"planes": (masks, None, None, rle._first_capacity(n, None)),
             "planes_bounds": (masks, None, poly_bounds, rle._first_capacity(n, poly_bounds)),
             "index": (None, maps.index, own_bounds, rle._first_capacity(n, own_bounds))}
    yy, xx = np.mgrid[0:H, 0:W]
    board = torch.from_numpy(((yy + xx) & 1).astype(np.uint8)[None]).to(dev)
    cases["checkerboard"] = (board, None, None, (H * W + 1, 2 * (H * W + 1)))
    heads = {}
    for name, (planes, index, bounds, (cap_c, cap_b)) in cases.items():
        k = n if name != "checkerboard" else 1
        b_dev = None if bounds is None else torch.from_numpy(bounds).to(dev)
        call, (counts, chars, table, head), nbytes = raw_encoder(planes, index, k, b_dev, cap_c, cap_b)
        us = timed(call, a.kernel_iters, a.rounds)
        h = head.cpu().numpy()
        heads[name] = (counts, table, h)
        enc[name] = {"n": k, "us": us, "total_counts": int(h[0]), "total_bytes": int(h[1]), "overflow": int(h[2]),
                     "cap_counts": cap_c, "cap_bytes": cap_b, "workspace_bytes": int(nbytes)}
        print("cp_rle_encode %s: %s; %d counts, %d bytes of string (overflow %d)" % (name, fmt(us), h[0], h[1], h[2]),
              flush=True)
    same = heads["planes"][1].cpu().numpy()[:, :2].tolist() == heads["planes_bounds"][1].cpu().numpy()[:, :2].tolist()
    if not same:
        raise SystemExit("the counts with bounds and without differ on the scene")
    result["mask_bytes"] = int(n * H * W)

    # 2. decode of the scene
    rles = rle.encode(masks=masks, bounds=poly_bounds, want_counts=True)
    flat = torch.from_numpy(np.concatenate([r["cnts"] for r in rles]).astype(np.int64)).to(torch.int32).to(dev)
    m = np.array([len(r["cnts"]) for r in rles])
    table = np.ascontiguousarray(np.stack([np.cumsum(m) - m, m], 1).astype(np.int32))
    planes = torch.empty((n, H, W), dtype=torch.uint8, device=dev)
    status = torch.empty((n,), dtype=torch.int32, device=dev)
    L = _C.lib()
    nbytes = L.cp_rle_decode_workspace_bytes(n, int(m.sum()))
    ws = _C.workspace(nbytes, dev)

    def decode():
        _C.check(L.cp_rle_decode(_C.ptr(flat), table.ctypes.data_as(ctypes.c_void_p), n, H, W, 255, _C.ptr(planes),
                                 _C.ptr(status), _C.ptr(ws), nbytes, _C.stream()), "cp_rle_decode")
    result["decode_us"] = timed(decode, a.kernel_iters, a.rounds)
    if int(status.any()) or not bool((planes == (masks != 0) * 255).all()):
        raise SystemExit("decode(encode(scene)) is not the scene")
    print("cp_rle_decode of the scene's %d counts into %d planes: %s" % (m.sum(), n, fmt(result["decode_us"])), flush=True)

    # 3. torch ops on the device
    def by_torch():
        return [torch_counts(masks[k]) for k in range(n)]
    got = by_torch()
    if any(got[k].cpu().tolist() != rles[k]["cnts"].tolist() for k in (0, n // 2, n - 1)):
        raise SystemExit("torch ops and cp_rle_encode disagree on the scene")
    result["torch_us"] = timed(by_torch, max(1, a.kernel_iters // 10), a.rounds)
    print("the same counts from torch ops (transpose, diff, nonzero; %d planes): %s" % (n, fmt(result["torch_us"])),
          flush=True)

    # 4. with the read-back, beside the host way
    def wrapped_encode():
        return rle.encode(masks=masks, bounds=poly_bounds)

    def by_host():
        host = masks.cpu().numpy()
        return [numpy_counts(host[k]) for k in range(n)]
    if [c.tolist() for c in by_host()[:2]] != [r["cnts"].tolist() for r in rles[:2]]:
        raise SystemExit("numpy and cp_rle_encode disagree on the scene")
    result["encode_wrapper_ms"] = wall(wrapped_encode, a.image_calls)
    result["encode_wrapper_no_bounds_ms"] = wall(lambda: rle.encode(masks=masks), a.image_calls)
    result["host_numpy_ms"] = wall(by_host, max(1, a.image_calls // 3))
    for name in ("planes", "planes_bounds", "index"):                     # (the wrapper asks for strings only)
        enc[name]["wrapper_retry"] = bool(enc[name]["total_bytes"] > enc[name]["cap_bytes"])
    result["wrapper_retries"] = "%d of 3 cases" % sum(enc[name]["wrapper_retry"] for name in ("planes", "planes_bounds",
                                                                                              "index"))
    print("utils.rle.encode with the read-back: %s with bounds, %s without; planes copied to the host and numpy: %s; "
          "second calls: %s" % (fmt(result["encode_wrapper_ms"], "ms"), fmt(result["encode_wrapper_no_bounds_ms"], "ms"),
                                fmt(result["host_numpy_ms"], "ms"), result["wrapper_retries"]), flush=True)

    # 5. the files
    tmp = a.tmp or tempfile.mkdtemp(prefix="probe_rle_")
    result["save_rle_ms"] = wall(lambda: instances.save_rle(maps, tmp, "scene"), a.image_calls)
    result["save_masks_ms"] = wall(lambda: instances.save_masks(maps, tmp, "scene"), max(1, a.image_calls // 3))
    result["rle_json_bytes"] = os.path.getsize(os.path.join(tmp, "scene_rle.json"))
    result["png_bytes"] = sum(os.path.getsize(os.path.join(tmp, "masks", f)) for f in os.listdir(os.path.join(tmp, "masks")))
    print("save_rle %s (%d bytes of JSON) beside save_masks %s (%d bytes of PNG)"
          % (fmt(result["save_rle_ms"], "ms"), result["rle_json_bytes"], fmt(result["save_masks_ms"], "ms"),
             result["png_bytes"]), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()

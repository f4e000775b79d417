"""GPU probe: what instance tracking costs (cp_map_pairs, cp_track_associate, cp_track_update; the torch statement of the
same counts; cp_panoptic_pairs on the same bytes; InstanceTracker.step per frame).

1. cp_map_pairs alone at 2048 x 1024 on the tracker's own inputs (the memory map after a frame of the seeded street scene
   of tools/probe_pixel_level.py, 30 instances, against the scene shifted by 7 pixels), HIP events around
   `--kernel_iters` calls, median and [min, max] over `--rounds`.  It reads 3 bytes a pixel.  Beside it
     torch       torch.bincount of mem * (n + 1) + index, the counts' statement in torch ops (must give the same table or
                 the probe stops)
     panoptic    cp_panoptic_pairs on the scene's id image and the same index, and cp_map_pairs on those same bytes
                 through a lookup: the plain-pass yardstick (it reads the ids twice, 5 bytes a pixel, in five launches)
2. The full step (the three calls, nothing read back) on
     scene       the street scene, alternating between the scene and its shifted copy
     one_pair    every pixel owned by instance 0: one cell of the table takes every count (the contention case)
     random_128  128 x 128 pixels, every pixel a random one of 128 instances: a full 257 x 129 table, 128 instances to
                 associate, hardly a run longer than one pixel
3. InstanceTracker.step_index per frame on the scene with the read-back, wall clock, beside detector.instances() (0.63 ms)
   and run() (3.2 ms), which profiles/probe_instances.json holds.

Usage:  python tools/probe_track.py [--json profiles/probe_track.json]
"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

from tools.probe_instances import spread, timed
from tools.probe_pixel_level import H, W, scene

LABELS = (24, 25, 26, 27, 28, 31, 32, 33)


def scene_frames():
    """(ids uint16 [H, W], [index, index shifted by 7 pixels], n, labels)"""
    ids = scene()[0]
    wide = ids.astype(np.int64)
    index = np.where(wide >= 1000, wide % 1000 - 1, 255).astype(np.uint8)
    return ids, [index, np.roll(index, 7, axis=1)], 30, np.array([LABELS[k % 8] for k in range(30)], np.int32)


def counting(a):
    import torch
    from centerpoly_amd import _C
    from centerpoly_amd.datasets.evaluation import panoptic as pq
    from centerpoly_amd.detectors import tracking
    dev = torch.device("cuda")
    ids, frames, n, labels = scene_frames()
    live = np.ones((n,), np.uint8)
    tr = tracking.InstanceTracker((W, H), 0.3, 0, multiplier=1000)
    tr.step_index(torch.from_numpy(frames[0]).to(dev), n, labels, live)
    index = torch.from_numpy(frames[1]).to(dev)
    pairs = torch.empty((257 * (n + 1),), dtype=torch.int32, device=dev)
    count = lambda: tracking.map_pairs(tr.mem, index, tracking.SLOTS, n, out=pairs)                    # noqa: E731

    def composed():
        rows = (tr.mem.reshape(-1).to(torch.int64) & 0xffff).clamp(max=tracking.SLOTS)
        return torch.bincount(rows * (n + 1) + index.reshape(-1).to(torch.int64).clamp(max=n), minlength=257 * (n + 1))

    if not torch.equal(count().reshape(-1).long(), composed()):
        raise SystemExit("torch.bincount and cp_map_pairs disagree on the scene")
    out = {"n": n, "cells": 257 * (n + 1), "bytes_read": 3 * H * W,
           "map_pairs_us": timed(count, a.kernel_iters, a.rounds),
           "torch_us": timed(composed, max(1, a.kernel_iters // 10), a.rounds)}
    out["GBps"] = out["bytes_read"] / (out["map_pairs_us"]["median"] * 1e-6) / 1e9
    # the plain-pass yardstick: the same id image and index through cp_panoptic_pairs and through cp_map_pairs
    p, lib = pq.CITYSCAPES, _C.lib()
    flags = np.ascontiguousarray(p.flags)
    nbytes = lib.cp_panoptic_pairs_workspace_bytes()
    ws = _C.workspace(nbytes, dev)
    seg = torch.zeros((1025, 4), dtype=torch.int32, device=dev)
    pan_pairs = torch.zeros((1025 * (n + 1),), dtype=torch.int32, device=dev)
    ids_dev = torch.from_numpy(ids.view(np.int16)).to(dev)

    def panoptic():
        _C.check(lib.cp_panoptic_pairs(_C.ptr(index), n, _C.ptr(ids_dev), H, W, p.id_divisor, p.id_direct_below, p.L,
                                       flags.ctypes.data_as(ctypes.c_void_p), _C.ptr(seg), _C.ptr(pan_pairs), _C.ptr(ws),
                                       nbytes, _C.stream()), "cp_panoptic_pairs")

    values = np.unique(ids[ids >= 1000])
    row_of = np.full((65536,), 0xffff, np.uint16)
    row_of[values] = np.arange(len(values))
    row_dev = torch.from_numpy(row_of.view(np.int16)).to(dev)
    looked = torch.empty(((len(values) + 1) * (n + 1),), dtype=torch.int32, device=dev)
    through_lookup = lambda: tracking.map_pairs(ids_dev, index, len(values), n, row_of=row_dev, out=looked)   # noqa: E731
    panoptic()
    G = int(seg[0, 0])
    things = pan_pairs.reshape(1025, n + 1)[1:G + 1]
    things = things[torch.from_numpy(np.isin(seg[1:G + 1, 0].cpu().numpy(), values)).to(dev)]
    if not torch.equal(through_lookup()[:len(values)], things):
        raise SystemExit("cp_panoptic_pairs and cp_map_pairs disagree on the scene's instances")
    out["same_bytes"] = {"rows": int(len(values)), "panoptic_pairs_us": timed(panoptic, a.kernel_iters, a.rounds),
                         "map_pairs_lookup_us": timed(through_lookup, a.kernel_iters, a.rounds)}
    return out


def steps(a):
    import torch
    from centerpoly_amd.detectors import tracking
    dev = torch.device("cuda")
    _, frames, n, labels = scene_frames()
    rng = np.random.RandomState(31)
    cases = {"scene": ((W, H), [torch.from_numpy(f).to(dev) for f in frames], n, labels),
             "one_pair": ((W, H), [torch.zeros((H, W), dtype=torch.uint8, device=dev)], 1, np.array([26], np.int32)),
             "random_128": ((128, 128), [torch.from_numpy(rng.randint(0, 128, (128, 128)).astype(np.uint8)).to(dev)
                                         for _ in range(2)], 128, np.full((128,), 26, np.int32))}
    out = {}
    for name, (canvas, indexes, k, lab) in cases.items():
        tr = tracking.InstanceTracker(canvas, 0.3, 0, multiplier=1000)
        live = np.ones((k,), np.uint8)
        turn = [0]

        def step():
            tr.enqueue(indexes[turn[0] % len(indexes)], k, lab, live, 1000)
            tr.frame += 1
            turn[0] += 1

        us = timed(step, a.kernel_iters, a.rounds)
        tab = tracking._split_state(tr.state.cpu().numpy(), k)
        if tab["status"]:
            raise SystemExit("the tracker refused the %s frames" % name)
        out[name] = {"canvas": list(canvas), "n": k, "us": us, "alive": int((tab["slots"][:, 0] != 0).sum())}
    tr = tracking.InstanceTracker((W, H), 0.3, 0, multiplier=1000)
    indexes, live, ms = cases["scene"][1], np.ones((n,), np.uint8), []
    for i in range(3 + a.image_calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        tracked = tr.step_index(indexes[i % 2], n, labels, live)
        torch.cuda.synchronize()
        if i >= 3:
            ms.append((time.perf_counter() - t0) * 1e3)
    out["step_index_ms"] = spread(ms)
    out["matched_in_last_frame"] = int((~tracked.table["is_new"]).sum())
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rounds", type=int, default=7)
    p.add_argument("--kernel_iters", type=int, default=100)
    p.add_argument("--image_calls", type=int, default=30)
    p.add_argument("--json", default=os.path.join(ROOT, "profiles", "probe_track.json"))
    a = p.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("probe_track needs a GPU: nothing is measured without one")
    result = {"unit_kernel": "us per call", "unit_step_index": "ms per frame", "rounds": a.rounds,
              "kernel_iters": a.kernel_iters, "device": torch.cuda.get_device_name(0), "shape": [H, W]}
    c = result["counting"] = counting(a)
    fmt = lambda r: "%.1f us [%.1f, %.1f]" % (r["median"], r["min"], r["max"])                         # noqa: E731
    print("cp_map_pairs %dx%d, 257 x %d cells: %s, %.0f GB/s; torch.bincount %s" % (W, H, c["n"] + 1, fmt(c["map_pairs_us"]),
                                                                                   c["GBps"], fmt(c["torch_us"])), flush=True)
    print("the scene's ids against the index: cp_panoptic_pairs %s; cp_map_pairs through a lookup %s"
          % (fmt(c["same_bytes"]["panoptic_pairs_us"]), fmt(c["same_bytes"]["map_pairs_lookup_us"])), flush=True)
    s = result["step"] = steps(a)
    for name in ("scene", "one_pair", "random_128"):
        print("full step %s (%d x %d, n = %d, %d tracks alive): %s" % (name, s[name]["canvas"][0], s[name]["canvas"][1],
                                                                       s[name]["n"], s[name]["alive"], fmt(s[name]["us"])),
              flush=True)
    r = s["step_index_ms"]
    print("InstanceTracker.step_index with the read-back: %.3f ms [%.3f, %.3f] per frame (%d of 30 matched)"
          % (r["median"], r["min"], r["max"], s["matched_in_last_frame"]), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()

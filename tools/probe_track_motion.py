"""GPU probe: what tracking with motion costs (cp_map_pairs_shifted beside cp_map_pairs, cp_track_kinematics, the full
motion step beside the plain step, and the torch statement of the shifted table).

tools/probe_track.py's protocol: 2048 x 1024, HIP events around `--kernel_iters` calls, median and [min, max] over
`--rounds`.  The maps are the tracker's own: the memory map after a frame of the seeded street scene (30 instances)
against the scene shifted by 7 pixels.

1. cp_map_pairs_shifted, each case beside cp_map_pairs on the same maps (that kernel is the baseline):
     zero       all shifts zero (the table must equal cp_map_pairs' or the probe stops)
     per_track  a seeded shift of up to 40 pixels either way per slot (must equal the torch statement)
     one_pair   every pixel of one slot and one instance, shift (13, 5): one cell takes every count
   and the torch statement of the per_track table: index arithmetic, a gather and torch.bincount.
2. cp_track_predict and cp_track_kinematics alone on the scene.
3. The full step (nothing read back) with and without motion on the scene, alternating between the two frames.

Nothing here is a real sequence: whether --track_motion lowers the identity switches on real data is not measured.

Usage:  python tools/probe_track_motion.py [--json profiles/probe_track_motion.json]
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

from tools.probe_instances import timed
from tools.probe_pixel_level import H, W
from tools.probe_track import scene_frames


def torch_statement(mem, shift, index, R, n):
    """The shifted table from torch ops, int64 [R + 1, n + 1]."""
    import torch
    rows = mem.reshape(-1).to(torch.int64) & 0xffff
    p = torch.arange(H * W, device=mem.device)
    x, y = p % W, p // W
    r = rows.clamp(max=R - 1)
    d = shift.to(torch.int64)[r]
    qx, qy = x + d[:, 0], y + d[:, 1]
    on = (rows < R) & (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
    flat = index.reshape(-1).to(torch.int64).clamp(max=n)
    col = flat[(qy * W + qx).clamp(0, H * W - 1)]
    counts = torch.bincount((r * (n + 1) + col)[on], minlength=R * (n + 1)).view(R, n + 1)
    none = torch.bincount(flat, minlength=n + 1) - counts.sum(0)
    return torch.cat([counts, none[None]], 0)


def counting(a):
    import torch
    from centerpoly_amd.detectors import tracking
    dev = torch.device("cuda")
    _, frames, n, labels = scene_frames()
    live = np.ones((n,), np.uint8)
    tr = tracking.InstanceTracker((W, H), 0.3, 0, multiplier=1000)
    tr.step_index(torch.from_numpy(frames[0]).to(dev), n, labels, live)
    index = torch.from_numpy(frames[1]).to(dev)
    R = tracking.SLOTS
    rng = np.random.RandomState(41)
    one_shift = np.zeros((R, 2), np.int32)
    one_shift[0] = [13, 5]
    cases = {"zero": (tr.mem, index, n, np.zeros((R, 2), np.int32)),
             "per_track": (tr.mem, index, n, rng.randint(-40, 41, (R, 2)).astype(np.int32)),
             "one_pair": (torch.zeros((H, W), dtype=torch.int16, device=dev),
                          torch.zeros((H, W), dtype=torch.uint8, device=dev), 1, one_shift)}
    out = {"n": n, "bytes_read": 4 * H * W}
    for name, (mem, idx, k, shift) in cases.items():
        shift_dev = torch.from_numpy(shift).to(dev)
        table = torch.empty((257 * (k + 1),), dtype=torch.int32, device=dev)
        base = torch.empty((257 * (k + 1),), dtype=torch.int32, device=dev)
        shifted = lambda: tracking.map_pairs_shifted(mem, shift_dev, idx, R, k, out=table)                 # noqa: E731
        plain = lambda: tracking.map_pairs(mem, idx, R, k, out=base)                                       # noqa: E731
        if name == "zero" and not torch.equal(shifted(), plain()):
            raise SystemExit("cp_map_pairs_shifted with zero shifts and cp_map_pairs disagree on the scene")
        if not torch.equal(shifted().long(), torch_statement(mem, shift_dev, idx, R, k)):
            raise SystemExit("the torch statement and cp_map_pairs_shifted disagree on %s" % name)
        out[name] = {"shifted_us": timed(shifted, a.kernel_iters, a.rounds),
                     "map_pairs_us": timed(plain, a.kernel_iters, a.rounds)}
        out[name]["ratio"] = out[name]["shifted_us"]["median"] / out[name]["map_pairs_us"]["median"]
        if name == "per_track":
            out[name]["torch_us"] = timed(lambda: torch_statement(mem, shift_dev, idx, R, k),
                                          max(1, a.kernel_iters // 10), a.rounds)
    out["GBps_zero"] = out["bytes_read"] / (out["zero"]["shifted_us"]["median"] * 1e-6) / 1e9
    return out


def steps(a):
    import torch
    from centerpoly_amd import _C
    from centerpoly_amd.detectors import tracking
    dev = torch.device("cuda")
    _, frames, n, labels = scene_frames()
    indexes, live = [torch.from_numpy(f).to(dev) for f in frames], np.ones((n,), np.uint8)
    out = {}
    for name, motion in (("plain", False), ("motion", True)):
        tr = tracking.InstanceTracker((W, H), 0.3, 0, multiplier=1000, motion=motion)
        turn = [0]

        def step():
            tr.enqueue(indexes[turn[0] % 2], n, labels, live, 1000)
            tr.frame += 1
            turn[0] += 1

        us = timed(step, a.kernel_iters, a.rounds)
        host = tr.state.cpu().numpy()
        tab = tracking._split_state(host, n)
        if tab["status"]:
            raise SystemExit("the tracker refused the scene")
        out[name] = {"us": us, "alive": int((tab["slots"][:, 0] != 0).sum()), "matched": int((tab["inst"][:, 4] == 0).sum())}
        if motion:
            shift = host[tracking.O_SHIFT:tracking.MOTION_INTS].reshape(-1, 2)
            out[name]["largest_shift"] = int(np.abs(shift).max())
            at = lambda o: ctypes.c_void_p(tr.state.data_ptr() + 4 * o)                                    # noqa: E731
            lib, t = _C.lib(), int(tr.frame)
            predict = lambda: _C.check(lib.cp_track_predict(at(0), at(tracking.O_KIN), t, H, W, at(tracking.O_SHIFT),  # noqa: E731
                                                            _C.stream()), "cp_track_predict")
            kinematics = lambda: _C.check(lib.cp_track_kinematics(                                         # noqa: E731
                _C.ptr(indexes[0]), n, H, W, at(tracking.O_INST), at(0), at(tracking.O_STATUS), t, at(tracking.O_KIN),
                _C.ptr(tr.moments), tr.moments_bytes, _C.stream()), "cp_track_kinematics")
            out["predict_us"] = timed(predict, a.kernel_iters, a.rounds)
            out["kinematics_us"] = timed(kinematics, a.kernel_iters, a.rounds)
    out["ratio"] = out["motion"]["us"]["median"] / out["plain"]["us"]["median"]
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rounds", type=int, default=7)
    p.add_argument("--kernel_iters", type=int, default=100)
    p.add_argument("--json", default=os.path.join(ROOT, "profiles", "probe_track_motion.json"))
    a = p.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("probe_track_motion needs a GPU: nothing is measured without one")
    result = {"unit": "us per call", "rounds": a.rounds, "kernel_iters": a.kernel_iters,
              "device": torch.cuda.get_device_name(0), "shape": [H, W]}
    fmt = lambda r: "%.1f us [%.1f, %.1f]" % (r["median"], r["min"], r["max"])                             # noqa: E731
    c = result["counting"] = counting(a)
    for name in ("zero", "per_track", "one_pair"):
        print("%-9s cp_map_pairs_shifted %s; cp_map_pairs %s; x%.2f" % (name, fmt(c[name]["shifted_us"]),
                                                                       fmt(c[name]["map_pairs_us"]), c[name]["ratio"]),
              flush=True)
    print("the per_track table from torch ops: %s; zero shifts stream %.0f GB/s" % (fmt(c["per_track"]["torch_us"]),
                                                                                   c["GBps_zero"]), flush=True)
    s = result["step"] = steps(a)
    print("cp_track_predict %s; cp_track_kinematics %s" % (fmt(s["predict_us"]), fmt(s["kinematics_us"])), flush=True)
    print("full step on the scene: plain %s; with motion %s (x%.2f, largest shift %d px, %d of 30 matched)"
          % (fmt(s["plain"]["us"]), fmt(s["motion"]["us"]), s["ratio"], s["motion"]["largest_shift"],
             s["motion"]["matched"]), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()

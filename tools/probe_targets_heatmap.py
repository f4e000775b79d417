"""GPU probe: build_targets with the UMich and the elliptical (--elliptical_gt) centre heat map, each with and without
--dense_poly, on a batch of 4 images of 1024x2048 (8x256x512 maps) with 30 and with 128 objects each.

HIP events around `--iters` calls (memset + kernels + output allocation, as the trainer calls it); the four variants of
one object count are timed in alternation for `--rounds` rounds and the median round is reported.  Also prints the
centre-splat pixels both modes cover (what the splat kernel's work grows with).

Usage:  python tools/probe_targets_heatmap.py [--rounds 7] [--iters 50] [--json OUT]
"""
import argparse
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from centerpoly_amd import synth
from centerpoly_amd.datasets.sample.polydet import build_targets, collate, pack_annotations
from centerpoly_amd.utils.image import get_affine_transform
from oracle.targets import gaussian_radius

IN_H, IN_W, OH, OW, C = 1024, 2048, 256, 512, 8


def batch(n_objs):
    packed = []
    for b in range(4):
        anns = synth.raw_annotations("probe_hm/%d/%d" % (n_objs, b), IN_H, IN_W, n_objs=n_objs)
        t = get_affine_transform(np.array([1000., 500.], np.float32), 2048.0, 0, [OW, OH])
        packed.append(pack_annotations(anns, t, b % 2, IN_W, 128, 16))
    return {k: v.cuda() for k, v in collate(packed).items()}


def splat_pixels(wh):
    """Centre-splat window sizes (unclipped) of the live objects: UMich (2r+1)^2 and ellipse (2rx+1)(2ry+1)."""
    um = el = 0
    for w, h in wh.reshape(-1, 2):
        if not (h > 0 and w > 0):
            continue
        r = max(0, int(gaussian_radius((math.ceil(h), math.ceil(w)))))
        rx = r if h > w else int(np.float32(r) * (w / h))
        ry = r if w >= h else int(np.float32(r) * (h / w))
        um += (2 * r + 1) ** 2
        el += (2 * rx + 1) * (2 * ry + 1)
    return um, el


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rounds", type=int, default=7)
    p.add_argument("--iters", type=int, default=50)
    p.add_argument("--json", default="")
    a = p.parse_args()
    variants = [("umich", False, False), ("ellipse", True, False), ("umich+dense", False, True),
                ("ellipse+dense", True, True)]
    result = {"shape": "B=4, 8x256x512 maps, 16 vertices", "rounds": a.rounds, "iters": a.iters, "us": {}}
    for n_objs in (30, 128):
        raw = batch(n_objs)
        calls = {name: (lambda e=e, d=d: build_targets(raw, OH, OW, C, dense_poly=d, elliptical_gt=e))
                 for name, e, d in variants}
        for fn in calls.values():                      # warm-up: code objects, allocator blocks
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        times = {name: [] for name in calls}
        for _ in range(a.rounds):
            for name, fn in calls.items():
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                for _ in range(a.iters):
                    fn()
                e.record()
                torch.cuda.synchronize()
                times[name].append(s.elapsed_time(e) / a.iters * 1e3)
        um, el = splat_pixels(calls["umich"]()["wh"].cpu().numpy())
        row = {name: float(np.median(v)) for name, v in times.items()}
        row["spread_us"] = {name: [round(min(v), 1), round(max(v), 1)] for name, v in times.items()}
        row["centre_splat_px"] = {"umich": um, "ellipse": el}
        result["us"]["%d_objects" % n_objs] = row
        print("B=4 x %3d objects: " % n_objs + ", ".join("%s %.1f us" % (k, row[k]) for k, _, _ in variants) +
              "; centre-splat pixels umich %d, ellipse %d (x%.2f)" % (um, el, el / max(um, 1)))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()

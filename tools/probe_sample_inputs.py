#!/usr/bin/env python3
"""Times the two image paths of the training sampler on one MI355X, device time per batch.

  * equal sizes: four seeded 1024 x 2048 sources -> 512 x 1024, colour augmentation on, through `build_inputs` (the
    per-image loop: 3 launches and a copy per image) and through `build_inputs_batch` (cp_sample_inputs_batch: two
    launches for the batch), alternating in the same run; the two outputs must agree or the probe stops;
  * mixed sizes: four KITTI-sized sources (375 x 1242, 376 x 1241, 374 x 1238, 370 x 1224) -> 384 x 1280 through the
    batch path, the only one that takes them.
Every figure is the time between two HIP events around --calls consecutive calls, divided by --calls (the host's
marshalling is inside when it is slower than the device), median [min, max] over --windows windows after a warm-up.
The byte figures count the OUTPUT side only (12 B written by the warp, 12 B read and 12 B written by the colour pass:
36 B per output pixel; the loop: 72 B); `source_px_per_output_px` (1 / scale^2 of the drawn maps) says what the
source reads add to both paths: three bytes times that, per output pixel inside the source.

Usage:  python tools/probe_sample_inputs.py [--json OUT] [--calls 20] [--windows 15]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
KITTI_SIZES = ((375, 1242), (376, 1241), (374, 1238), (370, 1224))


def stats(ms):
    ms = sorted(ms)
    return {"median_ms": ms[len(ms) // 2], "min_ms": ms[0], "max_ms": ms[-1]}


def draw(sizes, in_h, in_w, seed):
    """Seeded sources with the sampler's own parameters: a random crop's affine map and a colour row per image."""
    from centerpoly_amd.utils.image import get_affine_transform
    rng = np.random.RandomState(seed)
    images = [rng.randint(0, 256, (h, w, 3), dtype=np.uint8) for h, w in sizes]
    trans, color = [], []
    for h, w in sizes:
        c = np.array([w * rng.uniform(0.4, 0.6), h * rng.uniform(0.4, 0.6)], np.float32)
        trans.append(get_affine_transform(c, max(h, w) * rng.uniform(0.6, 1.3), 0, [in_w, in_h]).reshape(6))
        color.append([1.0, *rng.permutation(3), *rng.uniform(0.6, 1.4, 3), *rng.uniform(-0.05, 0.05, 3)])
    return images, np.stack(trans), np.array(color, np.float64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default="")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--windows", type=int, default=15)
    a = ap.parse_args()
    import torch

    from centerpoly_amd.datasets.sample.polydet import build_inputs, build_inputs_batch, collate_ragged
    if not torch.cuda.is_available():
        sys.exit("probe_sample_inputs.py measures on a HIP device; none is visible")
    dev = torch.device("cuda:0")

    def window(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.calls):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / a.calls

    def ragged(images):
        b = collate_ragged([{"image_u8": im} for im in images])
        return b["image_flat"].to(dev), b["image_hw"].numpy(), b["image_offset"].numpy()

    res = {"calls_per_window": a.calls, "windows": a.windows}

    # equal sizes: both paths, alternating
    images, trans, color = draw(((1024, 2048),) * 4, 512, 1024, 1)
    dense = torch.from_numpy(np.stack(images)).to(dev)
    flat, hw, off = ragged(images)
    old = lambda: build_inputs(dense, trans, color, MEAN, STD, 512, 1024)
    new = lambda: build_inputs_batch(flat, hw, off, trans, color, MEAN, STD, 512, 1024)
    if not torch.allclose(old(), new(), rtol=1e-6, atol=1e-5):
        sys.exit("build_inputs_batch differs from build_inputs on the probe's batch")
    for _ in range(3):
        window(old), window(new)
    t_old, t_new = [], []
    for _ in range(a.windows):
        t_old.append(window(old))
        t_new.append(window(new))
    px = 4 * 512 * 1024
    res["equal_4x1024x2048_to_512x1024"] = {
        "source_px_per_output_px": [float(1.0 / (t[0] * t[4] - t[1] * t[3])) for t in trans],
        "build_inputs": dict(stats(t_old), launches=3 * 4, copies=4, output_side_bytes_per_px=72),
        "build_inputs_batch": dict(stats(t_new), launches=2, copies=0, output_side_bytes_per_px=36)}
    med = res["equal_4x1024x2048_to_512x1024"]["build_inputs_batch"]["median_ms"]
    res["equal_4x1024x2048_to_512x1024"]["build_inputs_batch"]["output_side_GBps_at_median"] = 36.0 * px / (med * 1e-3) / 1e9

    # mixed sizes: the batch path alone
    images, trans, color = draw(KITTI_SIZES, 384, 1280, 2)
    flat, hw, off = ragged(images)
    new = lambda: build_inputs_batch(flat, hw, off, trans, color, MEAN, STD, 384, 1280)
    for _ in range(3):
        window(new)
    res["kitti_4_mixed_to_384x1280"] = {"sizes": [list(s) for s in KITTI_SIZES],
                                        "source_px_per_output_px": [float(1.0 / (t[0] * t[4] - t[1] * t[3])) for t in trans],
                                        "build_inputs_batch": dict(stats([window(new) for _ in range(a.windows)]),
                                                                   launches=2, copies=0)}
    print(json.dumps(res, indent=1, sort_keys=True))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()

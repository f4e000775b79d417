#!/usr/bin/env python3
"""Generate the `--elliptical_gt` fixtures from the REFERENCE's own code (src/lib/datasets/sample/polydet.py:156-159,
223-228 and src/lib/utils/image.py:144-173):

  sampler_ell_*.npz   PolydetDataset.__getitem__ with elliptical_gt=True, through gen_sampler_golden.py (same stubs,
                      same annotations, same schema; the cases below replace its CASES, plus an `elliptical_gt` flag)
  ellipse_prims.npz   draw_ellipse_gaussian on a small map: radii (0, 0), equal, 1:20 and 20:1 and in between, centres
                      on every border and corner, splats one by one and max-composited over each other

Runs only where the reference tree is present (gen_sampler_golden.REF / ANN); the fixtures hold inputs and expected
arrays, no reference source.

Usage:  python tests/golden/gen_elliptical_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import gen_sampler_golden as gsg                       # noqa: E402

ELL = {"elliptical_gt": True}
CASES = [
    # name, rep, split, not_rand_crop, flip probability, no_reorder_flip, image ids, seed, extra opt flags
    ("ell_cart_crop", "cartesian", "train", False, 0.5, False, [0, 1, 2], 41, ELL),
    ("ell_cart_flip", "cartesian", "train", False, 1.0, False, [5, 6], 42, ELL),
    ("ell_polar_flip", "polar", "train", False, 1.0, False, [3, 4], 43, ELL),
    ("ell_cart_dense", "cartesian", "train", False, 0.5, False, [0, 2, 5], 44, dict(ELL, dense_poly=True)),
    ("ell_cart_catspec", "cartesian", "train", False, 0.5, False, [1, 3], 45, dict(ELL, cat_spec_poly=True)),
    ("ell_cart_val", "cartesian", "val", False, 0.0, False, [7, 9], 46, ELL),
]

PRIM_HW = (30, 44)
# (cx, cy, rx, ry), drawn in this order
PRIM_SPLATS = [
    (0, 0, 0, 0), (43, 0, 4, 4), (0, 29, 1, 20), (43, 29, 20, 1),             # corners
    (0, 14, 20, 1), (43, 15, 1, 20), (21, 0, 2, 9), (22, 29, 11, 3),          # borders
    (20, 14, 1, 20), (21, 15, 20, 1), (20, 16, 5, 5), (24, 12, 3, 7),         # overlapping in the middle
    (10, 8, 7, 2), (33, 21, 0, 5), (12, 22, 6, 0), (38, 6, 2, 2),
]


def prims():
    gsg._stubs()
    from utils.image import draw_ellipse_gaussian                 # the reference's own helper
    h, w = PRIM_HW
    singles = np.zeros((len(PRIM_SPLATS), h, w), np.float32)
    stacked = np.zeros((h, w), np.float32)
    for i, (cx, cy, rx, ry) in enumerate(PRIM_SPLATS):
        draw_ellipse_gaussian(singles[i], (cx, cy), rx, ry)
        draw_ellipse_gaussian(stacked, (cx, cy), rx, ry)
    path = os.path.join(HERE, "ellipse_prims.npz")
    np.savez_compressed(path, hw=np.array(PRIM_HW), splats=np.array(PRIM_SPLATS, np.int64), singles=singles,
                        stacked=stacked)
    print("wrote", os.path.basename(path))


def main():
    gsg.CASES = CASES
    gsg.main()
    for case in CASES:                                            # mark the fixtures as elliptical
        path = os.path.join(HERE, "sampler_%s.npz" % case[0])
        if os.path.exists(path):
            with np.load(path) as f:
                d = dict(f)
            d["elliptical_gt"] = np.array(True)
            np.savez_compressed(path, **d)
    prims()


if __name__ == "__main__":
    main()

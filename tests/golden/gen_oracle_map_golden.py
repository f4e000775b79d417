#!/usr/bin/env python3
"""Generate oracle_map.npz from the REFERENCE's own gen_oracle_map (src/lib/utils/oracle_utils.py:8-42), the
breadth-first flood fill behind the `--eval_oracle_*` switches.

numba is not needed: a stub module whose `jit(...)` returns the function unchanged lets the loop run as plain Python
(the other generators stub cv2 the same way).  Inputs come from centerpoly_amd.synth; the feature of (j, c) is
j * D + c plus a fraction below one half, so every value is distinct and an output pixel names its owner.

Cases, the smallest shapes at which the kernel can still go wrong:
  a  1x1, M=1, ind=[0]: all zeros (the `ind > 0` skip)
  b  5x7, M=4, D=1: an ind == 0 row between valid rows, two rows on one centre (the pixel shows the later row, its
     neighbours the earlier one), seeds in two opposite corners
  c  13x37, M=128, D=2: 20 seeds at non-contiguous slots on a lattice with one seed moved, so that pixels are equidistant
     from 2, 3 and 4 seeds along both axes; w is a multiple of no vector width
  d  24x80, B=3, D=32: image 0 without a seed, image 1 with all 128 slots valid, image 2 with one seed at the last pixel
  e  64x96, D=33: odd channel count, several pixel tiles in both axes
  f  9x65, M=8, D=3: the kernel's tile (64 x 8) plus one in both axes
  g  13x21, M=1024, D=9: the largest object list the kernel takes, too large for its staged feature rows (it reads
     them from global memory instead), 200 objects on 272 centres: many share one

Runs only where the reference tree is present; the fixture holds inputs and recorded outputs, no reference source.

Usage:  python tests/golden/gen_oracle_map_golden.py
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference/src/lib"
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

from centerpoly_amd import synth                         # noqa: E402
from oracle_map_host import tie_counts                   # noqa: E402


def _stubs():
    numba = types.ModuleType("numba")
    numba.jit = lambda *a, **kw: (lambda f: f)
    sys.modules["numba"] = numba
    sys.path.insert(0, REF)


def _feat(name, B, M, D):
    base = np.arange(M * D, dtype=np.float64).reshape(1, M, D)
    f = (base + synth.uniform("oracle_map/%s/feat" % name, (B, M, D), 0.0, 0.5, dtype=np.float64)).astype(np.float32)
    for b in range(B):
        assert np.unique(f[b]).size == M * D
    return f


def _perm(stream, n):
    return np.argsort(synth.bits(stream, n), kind="stable")


def cases():
    out = []
    out.append(("a", 1, 1, _feat("a", 1, 1, 1), np.zeros((1, 1), np.int64)))
    # b: top-right corner twice (rows 0 and 3), a zero row, bottom-left corner
    out.append(("b", 5, 7, _feat("b", 1, 4, 1), np.array([[6, 0, 28, 6]], np.int64)))
    # c: lattice x in {2, 10, 18, 26, 34}, y in {0, 4, 8, 12}; the seed at (18, 8) moved to (16, 6)
    h, w = 13, 37
    pts = [(x, y) for y in (0, 4, 8, 12) for x in (2, 10, 18, 26, 34)]
    pts[pts.index((18, 8))] = (16, 6)
    order = _perm("oracle_map/c/order", len(pts))
    ind = np.zeros((1, 128), np.int64)
    for k, p in enumerate(order):
        ind[0, 3 + 6 * k] = pts[p][1] * w + pts[p][0]
    ties = tie_counts(ind, w, h)[0]
    assert min(ties) > 0, ties                           # pixels with 1, 2, 3 and 4 nearest seeds all occur
    out.append(("c", h, w, _feat("c", 1, 128, 2), ind))
    # d
    h, w = 24, 80
    ind = np.zeros((3, 128), np.int64)
    ind[1] = 1 + _perm("oracle_map/d/ctr", h * w - 1)[:128]
    ind[2, 5] = h * w - 1
    out.append(("d", h, w, _feat("d", 3, 128, 32), ind))
    # e: 40 objects in the first slots, 5 more further up, the rest padding
    h, w = 64, 96
    ind = np.zeros((1, 128), np.int64)
    ctr = 1 + _perm("oracle_map/e/ctr", h * w - 1)[:45]
    ind[0, :40] = ctr[:40]
    ind[0, [50, 77, 100, 126, 127]] = ctr[40:]
    out.append(("e", h, w, _feat("e", 1, 128, 33), ind))
    # f
    h, w = 9, 65
    ind = np.zeros((1, 8), np.int64)
    ind[0, :6] = [8 * w + 64, 3 * w + 63, 7 * w + 64, 1, 4 * w + 20, 8 * w + 0]
    out.append(("f", h, w, _feat("f", 1, 8, 3), ind))
    # g: 200 objects scattered over the 1024 slots, drawn with repetition from 272 centres
    h, w = 13, 21
    ind = np.zeros((1, 1024), np.int64)
    ind[0, _perm("oracle_map/g/slot", 1024)[:200]] = synth.integers("oracle_map/g/ctr", (200,), 1, h * w)
    out.append(("g", h, w, _feat("g", 1, 1024, 9), ind))
    return out


def main():
    _stubs()
    from utils.oracle_utils import gen_oracle_map        # the reference's own function
    d = {"names": np.array([c[0] for c in cases()])}
    for name, h, w, feat, ind in cases():
        ref = gen_oracle_map(feat, ind, w, h)
        assert ref.dtype == np.float32 and ref.shape == (feat.shape[0], feat.shape[2], h, w)
        d[name + "_hw"] = np.array([h, w], np.int64)
        d[name + "_feat"] = feat
        d[name + "_ind"] = ind
        d[name + "_out"] = ref
    path = os.path.join(HERE, "oracle_map.npz")
    np.savez_compressed(path, **d)
    print("wrote %s (%d bytes)" % (os.path.basename(path), os.path.getsize(path)))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Fixtures of the decode at 64 vertices (N2 = 128, the widest polygon row), from the REFERENCE's own Python (build
container only): decode_cart64.npz and decode_polar64.npz, the outputs of models/decode.py::_nms, _topk and
polydet_decode (with and without `reg`) as gen_golden.py::gen_decode records them for the narrower cases.  Outputs
only; the inputs regenerate from cases.decode_inputs_np with the tuples of wide_cases.py.

Usage:  python tests/golden/gen_decode_wide_golden.py"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

from cases import decode_inputs_np            # noqa: E402
from wide_cases import WIDE_DECODE_CASES      # noqa: E402

T = torch.from_numpy


def main():
    sys.path.insert(0, "/root/reference/src/lib")
    sys.modules["cv2"] = types.ModuleType("cv2")
    sys.modules["seaborn"] = types.ModuleType("seaborn")
    from models.decode import _nms, _topk, polydet_decode            # the reference's own

    for case in WIDE_DECODE_CASES:
        name, B, C, h, w, N, K, rep = case
        heat, polys, depth, reg = (T(a) for a in decode_inputs_np(*case))
        nm = _nms(heat)
        # tie-free requirement: the top K+1 of the image distinct and positive, and in every class's top K+1 the values
        # that can reach the image's top K (those >= its (K+1)-th value) distinct.  (A 32 x 64 map holds fewer than
        # K + 1 = 129 local maxima per class: a class's list ends in zeros and low scores, ties among which torch.topk
        # may order as it likes -- none of them is among the image's K best.)
        v2 = torch.sort(nm.view(B, -1), -1, descending=True)[0][..., :K + 1]
        assert (v2[..., :-1] > v2[..., 1:]).all() and (v2 > 0).all(), "ties in " + name
        v = torch.sort(nm.view(B, C, -1), -1, descending=True)[0][..., :K + 1]
        assert ((v[..., :-1] > v[..., 1:]) | (v[..., 1:] < v2[..., -1:, None])).all(), "ties in " + name
        scores, inds, clses, ys, xs = _topk(nm, K=K)
        dets = polydet_decode(heat.clone(), polys.clone(), depth.clone(), reg=reg.clone(), K=K, rep=rep)
        dets_noreg = polydet_decode(heat.clone(), polys.clone(), depth.clone(), reg=None, K=K, rep=rep)
        path = os.path.join(HERE, "decode_%s.npz" % name)
        np.savez_compressed(path, nms_sum=nm.double().sum().numpy(), nms_nnz=(nm != 0).sum().numpy(),
                            scores=scores.numpy(), inds=inds.numpy(), clses=clses.numpy(), ys=ys.numpy(), xs=xs.numpy(),
                            dets=dets.numpy(), dets_noreg=dets_noreg.numpy())
        print("wrote %-22s %7.1f KB" % (os.path.basename(path), os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()

"""GPU probe: the two kernels of the instance-level evaluation (cp_id_histogram, cp_instance_overlaps) on a
1024x2048 canvas with n = 16, 64 and 128 masks against about 150 ground-truth ids, and the numpy restatement of the
same counts on the host.  Also the share of the file output in CITYSCAPES.run_eval on the four writer fixtures:
files only (no ground truth), scored in memory (--no_mask_files), scored and written.

HIP events around `--iters` calls (for cp_instance_overlaps: its prepare kernel and the counting kernel, as the
evaluator calls it; for cp_id_histogram: its fill and its kernel), median of `--rounds` rounds after warm-up.  The roofline fraction is algorithmic bytes
(n * H * W mask bytes + 2 * H * W id bytes) / time / 8 TB/s.

Usage:  python tools/probe_instance_eval.py [--rounds 7] [--iters 200] [--json OUT]
"""
import argparse
import contextlib
import io
import json
import os
import sys
import tempfile
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from centerpoly_amd import _C
from centerpoly_amd.datasets.evaluation import instance_level as il

H, W, G = 1024, 2048, 150
HBM_PEAK = 8.0e12


def scene(n, seed=5):
    """A street-like id image (road, void strips, G rectangles of instance / group ids) and n masks: discs and
    rectangles of instance size, about a third of them large."""
    rng = np.random.RandomState(seed)
    gt = np.full((H, W), 7, np.uint16)
    gt[:, :40] = 3
    gt[H - 30:, :] = 1
    inst = []
    for j in range(G):
        lab = int(il.LABEL_IDS[rng.randint(8)])
        v = lab * 1000 + j if j % 9 or lab in inst else lab
        inst.append(v)
        y, x = rng.randint(0, H), rng.randint(0, W)
        gt[y:y + rng.randint(8, 200), x:x + rng.randint(8, 300)] = v
    masks = np.zeros((n, H, W), np.uint8)
    yy, xx = np.mgrid[0:H, 0:W]
    for i in range(n):
        y, x = rng.randint(0, H), rng.randint(0, W)
        big = i % 3 == 0
        if i % 2:
            r = rng.randint(60, 260) if big else rng.randint(6, 60)
            masks[i][(yy - y) ** 2 + (xx - x) ** 2 <= r * r] = 255
        else:
            masks[i, y:y + (rng.randint(100, 400) if big else rng.randint(8, 100)),
                  x:x + (rng.randint(100, 500) if big else rng.randint(8, 100))] = 255
    return gt, masks, inst


def numpy_counts(masks, gt, inst):
    col = np.full(65536, len(inst), np.int64)
    col[np.asarray(inst)] = np.arange(len(inst))
    is_void = np.zeros(65536, bool)
    is_void[[v for v in il.VOID_IDS if v >= 0]] = True
    flat = gt.reshape(-1)
    inter = np.zeros((len(masks), len(inst) + 1), np.int64)
    void = np.zeros(len(masks), np.int64)
    pix = np.zeros(len(masks), np.int64)
    for i in range(len(masks)):
        ids = flat[masks[i].reshape(-1) != 0]
        inter[i] = np.bincount(col[ids], minlength=len(inst) + 1)
        void[i] = is_void[ids].sum()
        pix[i] = len(ids)
    return inter[:, :-1], void, pix


def timed(fn, rounds, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(rounds):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(iters):
            fn()
        e.record()
        torch.cuda.synchronize()
        us.append(s.elapsed_time(e) / iters * 1e3)
    return float(np.median(us)), [round(min(us), 1), round(max(us), 1)]


def kernels(a, result):
    L = _C.lib()
    dev = torch.device("cuda")
    for n in (16, 64, 128):
        gt, masks, inst = scene(n)
        g_dev = torch.from_numpy(gt.view(np.int16)).to(dev)
        m_dev = torch.from_numpy(masks).to(dev)
        i_dev = torch.tensor(inst, dtype=torch.int32, device=dev)
        v_dev = torch.tensor(il.VOID_IDS, dtype=torch.int32, device=dev)
        inter = torch.empty((n, G), dtype=torch.int32, device=dev)
        void = torch.empty((n,), dtype=torch.int32, device=dev)
        pix = torch.empty((n,), dtype=torch.int32, device=dev)
        hist = torch.empty((65536,), dtype=torch.int32, device=dev)
        nbytes = L.cp_instance_overlaps_workspace_bytes(n, G, H, W)
        ws = _C.workspace(nbytes, dev)

        def overlaps():
            _C.check(L.cp_instance_overlaps(_C.ptr(m_dev), n, _C.ptr(g_dev), H, W, _C.ptr(i_dev), G, _C.ptr(v_dev),
                                            len(il.VOID_IDS), _C.ptr(inter), _C.ptr(void), _C.ptr(pix), _C.ptr(ws),
                                            nbytes, _C.stream()), "cp_instance_overlaps")

        def histogram():
            _C.check(L.cp_id_histogram(_C.ptr(g_dev), H, W, _C.ptr(hist), _C.stream()), "cp_id_histogram")

        t_ov, sp_ov = timed(overlaps, a.rounds, a.iters)
        t_hi, sp_hi = timed(histogram, a.rounds, a.iters)
        t0 = time.perf_counter()
        want = numpy_counts(masks, gt, inst)
        t_np = time.perf_counter() - t0
        t0 = time.perf_counter()
        want_hist = np.bincount(gt.reshape(-1), minlength=65536)
        t_np_hist = time.perf_counter() - t0
        ok = (np.array_equal(inter.cpu().numpy(), want[0]) and np.array_equal(void.cpu().numpy(), want[1])
              and np.array_equal(pix.cpu().numpy(), want[2]) and np.array_equal(hist.cpu().numpy(), want_hist))
        alg = n * H * W + 2 * H * W
        row = {"overlaps_us": t_ov, "overlaps_spread_us": sp_ov, "algorithmic_bytes": alg,
               "hbm_frac": alg / (t_ov * 1e-6) / HBM_PEAK, "histogram_us": t_hi, "histogram_spread_us": sp_hi,
               "histogram_hbm_frac": 2 * H * W / (t_hi * 1e-6) / HBM_PEAK, "numpy_overlaps_ms": t_np * 1e3,
               "numpy_histogram_ms": t_np_hist * 1e3, "host_ratio": t_np * 1e6 / t_ov, "equal_to_numpy": bool(ok),
               "mask_coverage": float((masks != 0).mean())}
        result["kernels"]["n=%d" % n] = row
        print("n = %3d: overlaps %.1f us (%.2f of HBM on %.0f MB), histogram %.1f us; numpy %.0f ms + %.1f ms "
              "(x%.0f); equal %s; masks cover %.1f %% of their canvases"
              % (n, t_ov, row["hbm_frac"], alg / 1e6, t_hi, t_np * 1e3, t_np_hist * 1e3, row["host_ratio"], ok,
                 100 * row["mask_coverage"]))


def file_share(result):
    """run_eval's parts on the four writer fixtures (4 images, 8-12 kept masks each), wall clock."""
    from PIL import Image
    from centerpoly_amd.datasets.dataset.polygons import CITYSCAPES
    from centerpoly_amd.opts import opts
    cases = ["star16", "mixed32", "selfcross16", "small16"]
    gold = os.path.join(ROOT, "tests", "golden")
    tmp = tempfile.mkdtemp()
    os.makedirs(os.path.join(tmp, "gt"))
    results = {}
    for k, c in enumerate(cases):
        z = np.load(os.path.join(gold, "writer_%s.npz" % c))
        # (the 8 classes of the data set: the pole / sign / light rows of mixed32 draw nothing)
        results[k] = {int(f[4:]): z[f] for f in z.files if f.startswith("det_") and int(f[4:]) <= 8}
        ids = np.load(os.path.join(gold, "instance_ap_%s.npz" % c))["gt_ids"]
        Image.fromarray(ids).save(os.path.join(tmp, "gt", "frankfurt_%s_gtFine_instanceIds.png" % c))
    ds = CITYSCAPES.__new__(CITYSCAPES)
    ds.coco = types.SimpleNamespace(imgs={k: {"id": k, "file_name": "frankfurt_%s_leftImg8bit.png" % c}
                                          for k, c in enumerate(cases)})
    out = {}
    with contextlib.redirect_stdout(io.StringIO()):
        variants = [("files_only", []), ("score_in_memory", ["--gt_dir", os.path.join(tmp, "gt"), "--no_mask_files"]),
                    ("score_and_files", ["--gt_dir", os.path.join(tmp, "gt")])]
        for name, extra in variants:
            ds.opt = opts().parse(["polydet"] + extra)
            ms = []
            for rep in range(4):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                ap = ds.run_eval(results, os.path.join(tmp, name))
                torch.cuda.synchronize()
                ms.append((time.perf_counter() - t0) * 1e3)
            out[name] = {"ms": float(np.median(ms[1:])), "allAp": ap}
    result["run_eval_4_images_ms"] = out
    print("run_eval on 4 images: " + ", ".join("%s %.0f ms" % (k, v["ms"]) for k, v in out.items()) +
          "; allAp %.4f" % out["score_and_files"]["allAp"])


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rounds", type=int, default=7)
    p.add_argument("--iters", type=int, default=200)
    p.add_argument("--json", default="")
    a = p.parse_args()
    result = {"shape": "%dx%d canvas, G = %d ids" % (H, W, G), "rounds": a.rounds, "iters": a.iters, "kernels": {}}
    kernels(a, result)
    file_share(result)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()

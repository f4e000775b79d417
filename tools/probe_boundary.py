"""GPU probe: what Boundary IoU costs (cp_boundary_overlaps, the torch composition of the same counts,
cp_instance_overlaps on the same inputs, what --boundary adds to an image of test.py's loop).

1. cp_boundary_overlaps at 2048 x 1024 with n = 128 planes, d = 11 (ratio 0.005) and d = 46 (ratio 0.02), HIP events
   around `--kernel_iters` calls, median and [min, max] over `--rounds`, on two contents:
     scene       the seeded street scene of tools/probe_pixel_level.py (30 instances over sky, buildings and road); plane
                 i is instance i % 30 shifted by a few pixels, its bounds the shifted instance's box
     full        128 full planes against the same id image: every word of every plane is read and walked
   each with and without `bounds`.
2. The same three tables from torch ops on the same inputs: the planes (and one plane per id of interest, from a
   comparison) as float16, padded with d zeros, eroded by max_pool2d of the negated planes -- separably, window
   (1, 2d + 1) then (2d + 1, 1), the cheaper form of the (2d + 1)^2 window with the same result -- bands by subtraction,
   counts by sums and one matrix product.  The kernel's tables must equal them in every number or the probe stops.
3. cp_instance_overlaps on the same planes and ids: one pass over the same bytes, the practical floor.
4. --boundary per image: a DLA-34 with seeded weights at 1024 x 2048, K = 128, --dataset cityscapes; after run(),
   score_instances_device on the rows left on the device with boundary=None (the path as it was) and with a
   BoundaryEvaluator, wall clock from device-idle to the tables on the host.

Usage:  python tools/probe_boundary.py [--json profiles/probe_boundary.json]
"""
import argparse
import contextlib
import io
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

from tools.probe_instances import seeded_weights, spread, timed
from tools.probe_pixel_level import H, W, scene

N = 128
WIDTHS = (11, 46)


def contents():
    """{name: (masks uint8 [N, H, W], bounds int32 [N, 4])}, the id image and its ids of interest."""
    ids = scene()[0]
    inst = np.unique(ids[ids >= 1000]).astype(np.int64)
    masks = np.zeros((N, H, W), np.uint8)
    bounds = np.zeros((N, 4), np.int32)
    for i in range(N):
        m = np.roll(ids == inst[i % len(inst)], (i % 5 - 2, 3 + i % 7), axis=(0, 1))
        masks[i] = m.astype(np.uint8) * 255
        ys, xs = np.flatnonzero(m.any(1)), np.flatnonzero(m.any(0))
        bounds[i] = (xs[0], ys[0], xs[-1], ys[-1])
    whole = np.tile(np.array([0, 0, W - 1, H - 1], np.int32), (N, 1))
    return {"scene": (masks, bounds), "full": (np.full((N, H, W), 255, np.uint8), whole)}, ids, inst


def torch_tables(masks, ids_wide, inst, d):
    import torch
    import torch.nn.functional as F

    def bands(planes):                                                    # bool [k, H, W] -> bool
        x = F.pad(planes.to(torch.float16)[:, None], (d, d, d, d), value=0.0)
        x = -F.max_pool2d(-x, (1, 2 * d + 1), stride=1)
        x = -F.max_pool2d(-x, (2 * d + 1, 1), stride=1)
        return planes & ~(x[:, 0] > 0)

    pb = bands(masks != 0)
    gb = bands(ids_wide[None] == inst[:, None, None])
    b_inter = pb.reshape(len(pb), -1).float() @ gb.reshape(len(gb), -1).float().t()       # exact below 2^24
    return b_inter.long(), pb.reshape(len(pb), -1).sum(1), gb.reshape(len(gb), -1).sum(1)


def kernels(a):
    import ctypes

    import torch
    from centerpoly_amd import _C
    from centerpoly_amd.datasets.evaluation import instance_level as il
    dev = torch.device("cuda")
    L = _C.lib()
    sets, ids, inst = contents()
    G = len(inst)
    ids_dev = torch.from_numpy(ids.view(np.int16)).to(dev)
    ids_wide = torch.from_numpy(ids.astype(np.int64)).to(dev)
    inst_dev = torch.from_numpy(inst.astype(np.int32)).to(dev)
    inst_wide = torch.from_numpy(inst).to(dev)
    void = torch.tensor(il.VOID_IDS, dtype=torch.int32, device=dev)
    tables = torch.zeros((N * G + N + G,), dtype=torch.int32, device=dev)
    at = lambda o: ctypes.c_void_p(tables.data_ptr() + 4 * o)             # noqa: E731
    out = {"G": G, "n": N}
    for name, (masks, bounds) in sets.items():
        masks_dev, bounds_dev = torch.from_numpy(masks).to(dev), torch.from_numpy(bounds).to(dev)
        r = out[name] = {"mask_pixels": int((masks != 0).sum()), "box_pixels": int(
            ((bounds[:, 2] - bounds[:, 0] + 1).astype(np.int64) * (bounds[:, 3] - bounds[:, 1] + 1)).sum())}
        nb = L.cp_instance_overlaps_workspace_bytes(N, G, H, W)
        ws0 = _C.workspace(nb, dev)

        def overlaps():
            _C.check(L.cp_instance_overlaps(_C.ptr(masks_dev), N, _C.ptr(ids_dev), H, W, _C.ptr(inst_dev), G, _C.ptr(void),
                                            len(il.VOID_IDS), at(0), at(N * G), at(N * G + N), _C.ptr(ws0), nb,
                                            _C.stream()), "cp_instance_overlaps")
        r["instance_overlaps_us"] = timed(overlaps, a.kernel_iters, a.rounds)
        for d in WIDTHS:
            nbytes = L.cp_boundary_overlaps_workspace_bytes(N, G, H, W, d)
            ws = _C.workspace(nbytes, dev)

            def boundary(b):
                _C.check(L.cp_boundary_overlaps(_C.ptr(masks_dev), N, _C.ptr(b) if b is not None else None,
                                                _C.ptr(ids_dev), H, W, d, _C.ptr(inst_dev), G, at(0), at(N * G),
                                                at(N * G + N), None, None, _C.ptr(ws), nbytes, _C.stream()),
                         "cp_boundary_overlaps")
            want = torch_tables(masks_dev, ids_wide, inst_wide, d)
            for b in (None, bounds_dev):
                boundary(b)
                got = tables.long()
                if not (torch.equal(got[:N * G].reshape(N, G), want[0]) and torch.equal(got[N * G:N * G + N], want[1])
                        and torch.equal(got[N * G + N:], want[2])):
                    raise SystemExit("the torch composition and the kernel disagree on %s, d = %d" % (name, d))
            k = r["d%d" % d] = {
                "workspace_bytes": int(nbytes), "band_pixels": int(want[1].sum()), "pair_pixels": int(want[0].sum()),
                "us": timed(lambda: boundary(None), a.kernel_iters, a.rounds),
                "bounds_us": timed(lambda: boundary(bounds_dev), a.kernel_iters, a.rounds),
                "torch_us": timed(lambda: torch_tables(masks_dev, ids_wide, inst_wide, d), a.torch_iters, a.rounds)}
            k["torch_over_kernel"] = k["torch_us"]["median"] / k["us"]["median"]
            k["kernel_over_instance_overlaps"] = k["us"]["median"] / r["instance_overlaps_us"]["median"]
            k["bounds_over_instance_overlaps"] = k["bounds_us"]["median"] / r["instance_overlaps_us"]["median"]
            del want
        del masks_dev
        torch.cuda.empty_cache()
    return out


def per_image(a, weights):
    import torch
    from centerpoly_amd import synth
    from centerpoly_amd.datasets.dataset_factory import dataset_factory
    from centerpoly_amd.datasets.evaluation import boundary as bd
    from centerpoly_amd.datasets.evaluation import instance_level as il
    from centerpoly_amd.detectors.detector_factory import detector_factory
    from centerpoly_amd.opts import opts
    with contextlib.redirect_stdout(io.StringIO()):
        opt = opts().parse(["polydet", "--arch", "dla_34", "--K", "128", "--input_h", str(H), "--input_w", str(W),
                            "--dataset", "cityscapes", "--load_model", weights])
        opt = opts().update_dataset_info_and_set_heads(opt, dataset_factory["cityscapes"])
        det = detector_factory["polydet"](opt)
    ds = dataset_factory["cityscapes"].__new__(dataset_factory["cityscapes"])
    ds.opt = opt
    ids = scene()[0]
    ids_dev = torch.from_numpy(ids.view(np.int16)).cuda()
    table = il.gt_instances(np.bincount(ids.reshape(-1), minlength=65536))
    img = (synth.uniform("probe_pixel_level/img", (H, W, 3)) * 255).astype(np.uint8)
    ret = det.run(img)
    rows = det.device_rows(ret["results"])
    out = {}
    for ratio in (0.005, 0.02):
        ms = {"plain": [], "boundary": []}
        for k in range(3 + a.image_calls):
            ev, bev = il.InstanceLevelEvaluator(), bd.BoundaryEvaluator(il.CITYSCAPES, ratio)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = ds.score_instances_device(rows, ids_dev, table, ev)
            t1 = time.perf_counter()
            ds.score_instances_device(rows, ids_dev, table, ev, boundary=bev)
            t2 = time.perf_counter()
            if k >= 3:
                ms["plain"].append((t1 - t0) * 1e3)
                ms["boundary"].append((t2 - t1) * 1e3)
        out["ratio_%g" % ratio] = {"d": bev.band_widths[(H, W)], "score_instances_device_ms": spread(ms["plain"]),
                                   "with_boundary_ms": spread(ms["boundary"]), "live": int(res["n"]),
                                   "added_ms": float(np.median(ms["boundary"]) - np.median(ms["plain"]))}
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--kernel_iters", type=int, default=20)
    p.add_argument("--torch_iters", type=int, default=2)
    p.add_argument("--image_calls", type=int, default=20)
    p.add_argument("--json", default=os.path.join(ROOT, "profiles", "probe_boundary.json"))
    a = p.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("probe_boundary needs a GPU: nothing is measured without one")
    result = {"unit_kernel": "us per call", "unit_per_image": "ms per image", "rounds": a.rounds,
              "kernel_iters": a.kernel_iters, "torch_iters": a.torch_iters, "device": torch.cuda.get_device_name(0),
              "shape": [H, W]}
    k = result["kernel"] = kernels(a)
    for name in ("scene", "full"):
        for d in WIDTHS:
            r = k[name]["d%d" % d]
            print("cp_boundary_overlaps %dx%d n = %d G = %d %s d = %d: %.1f us [%.1f, %.1f], with bounds %.1f us [%.1f, %.1f]; "
                  "torch %.0f us [%.0f, %.0f] = %.1f x; cp_instance_overlaps %.1f us, the kernel is %.2f x (%.2f x with "
                  "bounds)" % (W, H, N, k["G"], name, d, r["us"]["median"], r["us"]["min"], r["us"]["max"],
                               r["bounds_us"]["median"], r["bounds_us"]["min"], r["bounds_us"]["max"],
                               r["torch_us"]["median"], r["torch_us"]["min"], r["torch_us"]["max"], r["torch_over_kernel"],
                               k[name]["instance_overlaps_us"]["median"], r["kernel_over_instance_overlaps"],
                               r["bounds_over_instance_overlaps"]), flush=True)
    result["per_image"] = per_image(a, seeded_weights())
    for key, r in result["per_image"].items():
        print("--boundary per image at %dx%d, K = 128, %s (d = %d, %d live): score_instances_device %.3f ms [%.3f, %.3f], "
              "with the band tables %.3f ms [%.3f, %.3f]: + %.3f ms"
              % (H, W, key, r["d"], r["live"], r["score_instances_device_ms"]["median"],
                 r["score_instances_device_ms"]["min"], r["score_instances_device_ms"]["max"],
                 r["with_boundary_ms"]["median"], r["with_boundary_ms"]["min"], r["with_boundary_ms"]["max"],
                 r["added_ms"]), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()

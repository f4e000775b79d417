"""GPU probe: what the pixel-level evaluation costs (cp_pixel_confusion, the torch composition of the same counts, what
--pixel_iou adds to an image of test.py's loop).

1. The kernel alone on 2048 x 1024, HIP events around `--kernel_iters` calls, median and [min, max] over `--rounds`:
   on a seeded street scene (sky, buildings and road in bands, 30 elliptical instances of eight classes, the prediction
   the label image shifted by 7 pixels, so G = 30) and on a constant image, every pixel in one bin and one instance.
   The algorithm reads 3 bytes a pixel (one prediction byte, one 16-bit id): 6.3 MB, over the time over 8.0 TB/s is the
   fraction of the HBM peak.  The ratio constant / scene shows what contention on one bin costs.
2. The same counts composed from torch ops on the same device tensors: torch.bincount of g * L + p and three masked
   counts per instance.  Kernel and composition must agree in every number or the probe stops.
3. --pixel_iou per image: a DLA-34 with seeded weights at 1024 x 2048, K = 128, --dataset cityscapes and kitti_poly;
   after run() the two calls test.py adds, detector.instances() and PixelLevelEvaluator.add_maps() (upload of the id
   image, cp_id_histogram, cp_pixel_confusion, the one copy back), host clock around calls that end in a synchronise.
   With --save_ids / --save_masks the maps are made anyway and only add_maps is added.

Usage:  python tools/probe_pixel_level.py [--json profiles/probe_pixel_level.json]
"""
import argparse
import contextlib
import ctypes
import io
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

from tools.probe_instances import seeded_weights, spread, timed

H, W, N_INST = 1024, 2048, 30
HBM_PEAK = 8.0e12                                                         # bytes per second, the data sheet's


def scene():
    """(ids uint16 [H, W], pred uint8 [H, W]) of the seeded scene."""
    rng = np.random.RandomState(17)
    ids = np.full((H, W), 7, np.uint16)
    ids[:H // 4] = 23
    ids[H // 4:H // 2] = 11
    yy, xx = np.mgrid[0:H, 0:W]
    labels = (24, 25, 26, 27, 28, 31, 32, 33)
    for k in range(N_INST):
        cx, cy = rng.uniform(0, W), rng.uniform(H // 3, H)
        rx, ry = rng.uniform(30, 160), rng.uniform(25, 110)
        ids[((xx - cx) / rx) ** 2 + ((yy - cy) / ry) ** 2 < 1] = labels[k % 8] * 1000 + k + 1
    label = np.where(ids < 1000, ids, ids // 1000).astype(np.uint8)
    return ids, np.roll(label, 7, axis=1)


def torch_counts(pred, ids, table, inst_ids, protocol, group):
    """conf [L * L], inst [G, 3] from torch ops; ids int32 [H, W], pred uint8 [H, W], table the label of a byte."""
    import torch
    L = protocol.L
    v = ids.reshape(-1)
    g = torch.where(v < protocol.id_direct_below, v, v // protocol.id_divisor).long()
    p = table[pred.reshape(-1).long()]
    conf = torch.bincount(g * L + p, minlength=L * L)
    pg = group[p]
    rows = []
    for i in inst_ids:
        gl = i if i < protocol.id_direct_below else i // protocol.id_divisor
        mine = v == i
        rows.append(torch.stack([mine.sum(), (mine & (p == gl)).sum(), (mine & (pg == group[gl])).sum()]))
    return conf, torch.stack(rows)


def kernels(a):
    import torch
    from centerpoly_amd import _C
    from centerpoly_amd.datasets.evaluation import pixel_level as pl
    dev = torch.device("cuda")
    p = pl.CITYSCAPES
    lib = _C.lib()
    identity = np.arange(256, dtype=np.uint8)
    group = np.ascontiguousarray(p.label_group)
    out = {}
    images = {"scene": scene(), "constant": (np.full((H, W), 26001, np.uint16), np.full((H, W), 26, np.uint8))}
    for name, (ids, pred) in images.items():
        inst_ids = p.instances_of_interest(np.bincount(ids.reshape(-1), minlength=65536))
        G = len(inst_ids)
        ids_dev = torch.from_numpy(ids.view(np.int16)).to(dev)
        pred_dev = torch.from_numpy(pred).to(dev)
        cols = torch.tensor(inst_ids.tolist(), dtype=torch.int32).to(dev)
        conf = torch.zeros(p.L * p.L, dtype=torch.int64, device=dev)
        inst = torch.zeros((G, 3), dtype=torch.int32, device=dev)
        bad = torch.zeros(2, dtype=torch.int32, device=dev)
        nbytes = lib.cp_pixel_confusion_workspace_bytes(G)
        ws = _C.workspace(nbytes, dev)

        def call():
            _C.check(lib.cp_pixel_confusion(_C.ptr(pred_dev), identity.ctypes.data_as(ctypes.c_void_p), _C.ptr(ids_dev),
                                            H, W, p.id_divisor, p.id_direct_below, p.L,
                                            group.ctypes.data_as(ctypes.c_void_p), _C.ptr(cols), G, _C.ptr(conf),
                                            _C.ptr(inst), _C.ptr(bad), _C.ptr(ws), nbytes, _C.stream()),
                     "cp_pixel_confusion")

        call()
        wide = torch.from_numpy(ids.astype(np.int32)).to(dev)
        table, grp = torch.arange(256, device=dev), torch.from_numpy(group.astype(np.int64)).to(dev)
        composed = lambda: torch_counts(pred_dev, wide, table, inst_ids.tolist(), p, grp)   # noqa: E731
        t_conf, t_inst = composed()
        if not torch.equal(conf, t_conf) or not torch.equal(inst.long(), t_inst) or int(bad.sum()):
            raise SystemExit("the torch composition and the kernel disagree on the %s image" % name)
        r = out[name] = {"G": G, "us": timed(call, a.kernel_iters, a.rounds),
                         "torch_us": timed(composed, max(1, a.kernel_iters // 10), a.rounds), "bytes_read": 3 * H * W}
        r["GBps"] = r["bytes_read"] / (r["us"]["median"] * 1e-6) / 1e9
        r["fraction_of_hbm_peak"] = r["GBps"] * 1e9 / HBM_PEAK
    out["constant_over_scene"] = out["constant"]["us"]["median"] / out["scene"]["us"]["median"]
    return out


def per_image(a, weights, dataset):
    import torch
    from centerpoly_amd import synth
    from centerpoly_amd.datasets.dataset_factory import dataset_factory
    from centerpoly_amd.datasets.evaluation import pixel_level as pl
    from centerpoly_amd.detectors.detector_factory import detector_factory
    from centerpoly_amd.opts import opts
    with contextlib.redirect_stdout(io.StringIO()):
        opt = opts().parse(["polydet", "--arch", "dla_34", "--K", "128", "--input_h", str(H), "--input_w", str(W),
                            "--dataset", dataset, "--load_model", weights])
        opt = opts().update_dataset_info_and_set_heads(opt, dataset_factory[dataset])
        det = detector_factory["polydet"](opt)
    protocol = pl.PROTOCOLS[pl.DATASET_PROTOCOL[dataset]]
    ids = scene()[0]
    if protocol is pl.KITTI:
        wide = ids.astype(np.int64)
        ids = np.where(wide < 1000, wide * 256, wide // 1000 * 256 + wide % 1000).astype(np.uint16)
    img = (synth.uniform("probe_pixel_level/img", (H, W, 3)) * 255).astype(np.uint8)
    ret = det.run(img)
    ev = pl.PixelLevelEvaluator(protocol)
    ms = {"instances": [], "add_maps": [], "run": []}
    for k in range(3 + a.image_calls):
        t0 = time.perf_counter()
        maps = det.instances(ret["results"])
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        rows = ev.add_maps(maps, ids)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        if k >= 3:
            ms["instances"].append((t1 - t0) * 1e3)
            ms["add_maps"].append((t2 - t1) * 1e3)
    for _ in range(5):
        t0 = time.perf_counter()
        det.run(img)
        torch.cuda.synchronize()
        ms["run"].append((time.perf_counter() - t0) * 1e3)
    ev.summarize()
    return {"instances_ms": spread(ms["instances"]), "add_maps_ms": spread(ms["add_maps"]), "run_ms": spread(ms["run"]),
            "G": int(len(rows)), "live": int(maps.table["live"].sum())}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rounds", type=int, default=7)
    p.add_argument("--kernel_iters", type=int, default=100)
    p.add_argument("--image_calls", type=int, default=30)
    p.add_argument("--json", default=os.path.join(ROOT, "profiles", "probe_pixel_level.json"))
    a = p.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("probe_pixel_level needs a GPU: nothing is measured without one")
    result = {"unit_kernel": "us per call", "unit_per_image": "ms per image", "rounds": a.rounds,
              "kernel_iters": a.kernel_iters, "device": torch.cuda.get_device_name(0), "shape": [H, W]}
    k = result["kernel"] = kernels(a)
    for name in ("scene", "constant"):
        r = k[name]
        print("cp_pixel_confusion %dx%d %s (G = %d): %.1f us [%.1f, %.1f]; reads %.1f MB: %.0f GB/s, %.1f %% of the HBM "
              "peak; torch composition %.1f us [%.1f, %.1f]"
              % (W, H, name, r["G"], r["us"]["median"], r["us"]["min"], r["us"]["max"], r["bytes_read"] / 1e6, r["GBps"],
                 100 * r["fraction_of_hbm_peak"], r["torch_us"]["median"], r["torch_us"]["min"], r["torch_us"]["max"]),
              flush=True)
    print("constant / scene: %.2f" % k["constant_over_scene"], flush=True)
    weights = seeded_weights()
    result["per_image"] = {}
    for dataset in ("cityscapes", "kitti_poly"):
        r = result["per_image"][dataset] = per_image(a, weights, dataset)
        print("--pixel_iou per image, %s at %dx%d, K = 128: instances() %.3f ms + add_maps() %.3f ms [%.3f, %.3f] "
              "(G = %d, %d live); run() itself %.2f ms"
              % (dataset, H, W, r["instances_ms"]["median"], r["add_maps_ms"]["median"], r["add_maps_ms"]["min"],
                 r["add_maps_ms"]["max"], r["G"], r["live"], r["run_ms"]["median"]), flush=True)
        torch.cuda.empty_cache()
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()

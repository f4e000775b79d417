"""GPU probe: what the distance columns (AP 100 m / AP 50 m) cost: cp_segment_medians, the same medians from torch
ops, cp_id_histogram on the same id bytes, what `distances=` adds to an image of score_instances_device, and what
--disparity_dir adds to test.py's loop.  Everything at 2048 x 1024, median and [min, max].

1. cp_segment_medians (all six launches), HIP events around `--kernel_iters` calls over `--rounds`, on three contents:
     scene       the seeded street scene of tools/probe_pixel_level.py (30 instances over sky, buildings and road), its
                 disparity a ground plane with the instances at their own depth, seeded noise and 10 % holes
     one_bucket  ONE instance on every pixel, every value in one high byte: pass 1 touches one counter per lane, pass 2
                 sends every pixel to the 256 low-byte counters of one segment: the contention case
     random1024  G = 1024, every pixel a random one of the ids, random values: both passes on global atomics
   The integers must equal np.sort's or the probe stops.
2. The same [G, 4] from torch ops: per segment a boolean mask, the masked values sorted, the two middles picked.
3. cp_id_histogram on the same id image: the plain pass over the same id bytes.
4. Per image: a DLA-34 with seeded weights at 1024 x 2048, K = 128, --dataset cityscapes; after run(),
   score_instances_device on the rows left on the device without and with `distances=` (the disparity already on the
   device, and as a host array that is uploaded in the call), wall clock from device-idle to the tables on the host.
5. test.py's scored images per second on PNG files with and without --disparity_dir / --camera_dir (prefetching
   loader, --no_mask_files; the workers decode one more 16-bit PNG per image), and the decode of one disparity PNG.

Usage:  python tools/probe_segment_median.py [--json profiles/probe_segment_median.json]
"""
import argparse
import contextlib
import importlib.util
import io
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

from tools.probe_instances import seeded_weights, spread, timed
from tools.probe_pixel_level import H, W, scene

CAMERA = (0.209313, 2262.52)


def scene_disparity(ids):
    """uint16 [H, W]: a ground plane, every instance around its own disparity, seeded noise, 10 % holes."""
    rng = np.random.RandomState(29)
    y, x = np.mgrid[0:H, 0:W]
    p = (300 + 20 * y + (x * 7 + y * 13) % 31).astype(np.int64)
    noise = rng.randint(-40, 41, (H, W))
    for k, inst in enumerate(np.unique(ids[ids >= 1000])):
        m = ids == inst
        p[m] = (int(256 * CAMERA[0] * CAMERA[1] / (8.0 + 6.0 * k)) + 1 + noise)[m]
    p = np.clip(p, 1, 65535)
    p[rng.random_sample((H, W)) < 0.1] = 0
    return p.astype(np.uint16)


def contents():
    """{name: (ids uint16 [H, W], values uint16 [H, W], seg ids int64 [G])}."""
    ids = scene()[0]
    rng = np.random.RandomState(31)
    seg = rng.permutation(65536)[:1024].astype(np.int64)
    return {"scene": (ids, scene_disparity(ids), np.unique(ids[ids >= 1000]).astype(np.int64)),
            "one_bucket": (np.full((H, W), 26001, np.uint16),
                           (0x2a00 + rng.randint(0, 256, (H, W))).astype(np.uint16), np.array([26001], np.int64)),
            "random1024": (seg[rng.randint(0, 1024, (H, W))].astype(np.uint16),
                           rng.randint(0, 65536, (H, W)).astype(np.uint16), seg)}


def host_medians(ids, val, seg):
    out = np.zeros((len(seg), 4), np.int64)
    order = np.argsort(ids.reshape(-1), kind="stable")                    # one sort, then a slice per segment
    sid, sval = ids.reshape(-1)[order], val.reshape(-1)[order]
    for j, s in enumerate(seg):
        v = sval[np.searchsorted(sid, s, "left"):np.searchsorted(sid, s, "right")]
        out[j, 0] = v.size
        v = np.sort(v[v != 0])
        out[j, 1] = v.size
        if v.size:
            out[j, 2], out[j, 3] = v[(v.size - 1) // 2], v[v.size // 2]
    return out


def torch_medians(ids_wide, val_wide, seg):
    """The masked sort per instance: int64 [G, 4] on the device."""
    import torch
    rows = []
    zero = torch.zeros((), dtype=torch.int64, device=ids_wide.device)
    for s in seg.tolist():
        mine = ids_wide == s
        v = val_wide[mine & (val_wide != 0)]
        n = v.numel()
        if n:
            v = torch.sort(v).values
            rows.append(torch.stack([mine.sum(), zero + n, v[(n - 1) // 2], v[n // 2]]))
        else:
            rows.append(torch.stack([mine.sum(), zero, zero, zero]))
    return torch.stack(rows)


def kernels(a):
    import torch
    from centerpoly_amd import _C
    from centerpoly_amd.datasets.evaluation import distances
    dev = torch.device("cuda")
    L = _C.lib()
    out = {}
    for name, (ids, val, seg) in contents().items():
        G = len(seg)
        ids_dev = torch.from_numpy(ids.view(np.int16)).to(dev)
        val_dev = torch.from_numpy(val.view(np.int16)).to(dev)
        seg_dev = torch.from_numpy(seg.astype(np.int32)).to(dev)
        res = torch.zeros((G, 4), dtype=torch.int32, device=dev)
        nbytes = L.cp_segment_medians_workspace_bytes(G, H, W)
        ws = _C.workspace(nbytes, dev)
        hist = torch.empty((65536,), dtype=torch.int32, device=dev)

        def medians():
            _C.check(L.cp_segment_medians(_C.ptr(ids_dev), _C.ptr(val_dev), H, W, _C.ptr(seg_dev), G, _C.ptr(res),
                                          _C.ptr(ws), nbytes, _C.stream()), "cp_segment_medians")

        def histogram():
            _C.check(L.cp_id_histogram(_C.ptr(ids_dev), H, W, _C.ptr(hist), _C.stream()), "cp_id_histogram")
        medians()
        want = host_medians(ids, val, seg)
        if not np.array_equal(res.cpu().numpy().astype(np.int64), want):
            raise SystemExit("cp_segment_medians and np.sort disagree on %s" % name)
        ids_wide, val_wide = torch.from_numpy(ids.astype(np.int64)).to(dev), torch.from_numpy(val.astype(np.int64)).to(dev)
        if not np.array_equal(torch_medians(ids_wide, val_wide, seg).cpu().numpy(), want):
            raise SystemExit("the torch composition and np.sort disagree on %s" % name)
        r = out[name] = {"G": G, "workspace_bytes": int(nbytes), "valid_pixels": int(want[:, 1].sum()),
                         "segment_pixels": int(want[:, 0].sum()),
                         "us": timed(medians, a.kernel_iters, a.rounds),
                         "id_histogram_us": timed(histogram, a.kernel_iters, a.rounds),
                         "torch_us": timed(lambda: torch_medians(ids_wide, val_wide, seg), 1 if G > 100 else a.torch_iters,
                                           a.rounds)}
        r["torch_over_kernel"] = r["torch_us"]["median"] / r["us"]["median"]
        r["kernel_over_id_histogram"] = r["us"]["median"] / r["id_histogram_us"]["median"]
        del ids_wide, val_wide
        torch.cuda.empty_cache()
    out["scene"]["table"] = distances.table_from_counts(host_medians(*contents()["scene"]), CAMERA).tolist()
    return out


def per_image(a, weights):
    import torch
    from centerpoly_amd import synth
    from centerpoly_amd.datasets.dataset_factory import dataset_factory
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
    disp = scene_disparity(ids)
    ids_dev = torch.from_numpy(ids.view(np.int16)).cuda()
    disp_dev = torch.from_numpy(disp.view(np.int16)).cuda()
    table = il.gt_instances(np.bincount(ids.reshape(-1), minlength=65536))
    img = (synth.uniform("probe_pixel_level/img", (H, W, 3)) * 255).astype(np.uint8)
    rows = det.device_rows(det.run(img)["results"])
    ms = {"plain": [], "device_disparity": [], "host_disparity": []}
    for k in range(3 + a.image_calls):
        stamps = []
        for d in (None, (disp_dev, CAMERA), (disp, CAMERA)):              # the three alternate within a repetition
            ev = il.InstanceLevelEvaluator(distances=d is not None)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = ds.score_instances_device(rows, ids_dev, table, ev, **({} if d is None else {"distances": d}))
            stamps.append((time.perf_counter() - t0) * 1e3)
        if k >= 3:
            for key, v in zip(ms, stamps):
                ms[key].append(v)
    out = {k + "_ms": spread(v) for k, v in ms.items()}
    out.update(live=int(res["n"]), G=len(table),
               added_ms=float(np.median(ms["device_disparity"]) - np.median(ms["plain"])),
               added_with_upload_ms=float(np.median(ms["host_disparity"]) - np.median(ms["plain"])))
    return out


def driver_rates(a, tmp):
    """test.py on PNG files: the probe_eval_tail set (four fixture images listed `repeat` times) plus the files of
    tests/distance_ref.py's disparities."""
    from PIL import Image
    from centerpoly_amd.datasets.evaluation import distances
    from centerpoly_amd.opts import opts
    from tools.probe_eval_tail import CASES, make_set
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import distance_ref
    base, gt_dir = make_set(tmp, a.repeat, "")
    disp_dir, cam_dir = os.path.join(tmp, "disparity"), os.path.join(tmp, "camera")
    for d in (disp_dir, cam_dir):
        os.makedirs(os.path.join(d, "val", "frankfurt"))
    for index, c in enumerate(CASES):
        ids = np.load(os.path.join(ROOT, "tests", "golden", "instance_ap_%s.npz" % c))["gt_ids"]
        Image.fromarray(distance_ref.disparity(ids, index)).save(
            os.path.join(disp_dir, "val", "frankfurt", "frankfurt_%s_disparity.png" % c))
        with open(os.path.join(cam_dir, "val", "frankfurt", "frankfurt_%s_camera.json" % c), "w") as f:
            json.dump({"extrinsic": {"baseline": distance_ref.camera(index)[0]},
                       "intrinsic": {"fx": distance_ref.camera(index)[1]}}, f)
    dec = []
    for _ in range(3):
        for c in CASES:
            t0 = time.perf_counter()
            distances.read_disparity(os.path.join(disp_dir, "val", "frankfurt", "frankfurt_%s_disparity.png" % c))
            dec.append((time.perf_counter() - t0) * 1e3)
    spec = importlib.util.spec_from_file_location("centerpoly_test_driver", os.path.join(ROOT, "test.py"))
    drv = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(drv)
    import torch
    scored = ["--gt_dir", gt_dir, "--no_mask_files", "--num_workers", str(a.num_workers)]
    variants = [("scored", scored), ("scored_with_distances", scored + ["--disparity_dir", disp_dir, "--camera_dir",
                                                                        cam_dir])]
    out = {}
    for rep in range(a.driver_reps):                                      # the two alternate within a repetition
        for name, extra in variants:
            opt = opts().parse(base + extra)
            opt.save_dir = os.path.join(tmp, "exp_%s_%d" % (name, rep))
            with contextlib.redirect_stdout(io.StringIO()):
                st = drv.run_test(opt)["stamps"]
            out.setdefault(name, []).append((len(st) - 1 - a.skip) / (st[-1] - st[a.skip]))
            torch.cuda.empty_cache()
    res = {k: dict(spread(v), unit="img/s") for k, v in out.items()}
    res["disparity_png_decode_ms"] = spread(dec)
    res["images"], res["num_workers"] = 4 * a.repeat - a.skip, a.num_workers
    return res


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--kernel_iters", type=int, default=50)
    p.add_argument("--torch_iters", type=int, default=2)
    p.add_argument("--image_calls", type=int, default=20)
    p.add_argument("--repeat", type=int, default=10, help="the four images are listed this many times for test.py")
    p.add_argument("--skip", type=int, default=8)
    p.add_argument("--driver_reps", type=int, default=3)
    p.add_argument("--num_workers", type=int, default=4)
    p.add_argument("--json", default=os.path.join(ROOT, "profiles", "probe_segment_median.json"))
    a = p.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("probe_segment_median needs a GPU: nothing is measured without one")
    result = {"unit_kernel": "us per call (all six launches)", "unit_per_image": "ms per image", "rounds": a.rounds,
              "kernel_iters": a.kernel_iters, "torch_iters": a.torch_iters, "device": torch.cuda.get_device_name(0),
              "shape": [H, W]}
    k = result["kernel"] = kernels(a)
    for name, r in k.items():
        print("cp_segment_medians %dx%d %s G = %d: %.1f us [%.1f, %.1f]; torch %.0f us [%.0f, %.0f] = %.0f x; "
              "cp_id_histogram %.1f us [%.1f, %.1f], the medians are %.2f x"
              % (W, H, name, r["G"], r["us"]["median"], r["us"]["min"], r["us"]["max"], r["torch_us"]["median"],
                 r["torch_us"]["min"], r["torch_us"]["max"], r["torch_over_kernel"], r["id_histogram_us"]["median"],
                 r["id_histogram_us"]["min"], r["id_histogram_us"]["max"], r["kernel_over_id_histogram"]), flush=True)
    r = result["per_image"] = per_image(a, seeded_weights())
    print("distances per image at %dx%d, K = 128 (%d live, G = %d): score_instances_device %.3f ms [%.3f, %.3f], with a "
          "device disparity %.3f ms [%.3f, %.3f]: + %.3f ms; with a host disparity %.3f ms [%.3f, %.3f]: + %.3f ms"
          % (H, W, r["live"], r["G"], r["plain_ms"]["median"], r["plain_ms"]["min"], r["plain_ms"]["max"],
             r["device_disparity_ms"]["median"], r["device_disparity_ms"]["min"], r["device_disparity_ms"]["max"],
             r["added_ms"], r["host_disparity_ms"]["median"], r["host_disparity_ms"]["min"],
             r["host_disparity_ms"]["max"], r["added_with_upload_ms"]), flush=True)
    r = result["driver"] = driver_rates(a, tempfile.mkdtemp())
    print("test.py --gt_dir --no_mask_files, %d images, %d workers: %.2f img/s [%.2f, %.2f]; with --disparity_dir "
          "%.2f img/s [%.2f, %.2f]; one disparity PNG decodes in %.1f ms [%.1f, %.1f]"
          % (r["images"], r["num_workers"], r["scored"]["median"], r["scored"]["min"], r["scored"]["max"],
             r["scored_with_distances"]["median"], r["scored_with_distances"]["min"], r["scored_with_distances"]["max"],
             r["disparity_png_decode_ms"]["median"], r["disparity_png_decode_ms"]["min"],
             r["disparity_png_decode_ms"]["max"]), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()

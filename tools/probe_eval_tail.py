"""GPU probe: what lies between the network and the count tables of a scored image, and test.py's rate on PNG files.

The data set is four seeded 2048x1024 PNG images (listed `--repeat` times) with the id images of
tests/golden/instance_ap_*.npz as ground truth, and a seeded, randomly initialised DLA-34 whose `poly` bias draws a
16-gon around every centre (as tests/test_writer_instances.py builds them; a trained checkpoint: --load_model).

1. cp_writer_instances alone on the detector's own rows (R = K = 128): HIP events around `--iters` calls, median of
   `--rounds` rounds after warm-up, as tools/probe_instance_eval.py measures its kernels.
2. The wall clock per image from the end of process() (device idle) to "count tables on the host":
     common      post_process + merge_outputs (both paths need the host rows for results.json)
     tail_new    score_instances_device on the rows post_process left on the device, ground-truth table from the
                 loader worker (np.bincount)
     tail_parent image_instances -> instance_masks_device -> counts read back -> masks gathered -> add_image
                 (cp_id_histogram read back, cp_instance_overlaps), run from the unchanged host methods
   alternating per image, `--tail-rounds` passes over the four images; median and [min, max] over the passes of the
   per-image mean.  Both paths must give the same tables or the probe stops.
3. test.py's images per second on the PNG files (after `--skip` warm-up images; the final run_eval is outside the
   window): plain and scored with --gt_dir ... --no_mask_files, each with and without prefetching;
   PolydetDetector.run alone on the decoded arrays; and the PNG decode time per image on the host (seeded noise
   compresses worse than a street scene: an upper bound).

Usage:  python tools/probe_eval_tail.py [--json OUT] [--repeat 10] [--num_workers 4]
"""
import argparse
import contextlib
import ctypes
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
import torch

from centerpoly_amd import _C
from centerpoly_amd.datasets.evaluation import instance_level as il
from centerpoly_amd.opts import opts

CASES = ["star16", "mixed32", "selfcross16", "small16"]


def make_set(tmp, repeat, load_model):
    from PIL import Image
    from centerpoly_amd.models.model import create_model, save_model
    rng = np.random.RandomState(11)
    img_dir, annot_dir, gt_dir = os.path.join(tmp, "images"), os.path.join(tmp, "BBoxes"), os.path.join(tmp, "gtFine")
    for d in (img_dir, annot_dir, os.path.join(gt_dir, "val", "frankfurt")):
        os.makedirs(d)
    for c in CASES:
        coarse = rng.randint(0, 256, (32, 64, 3)).astype(np.uint8)
        img = np.kron(coarse, np.ones((32, 32, 1), np.uint8)) // 2 + rng.randint(0, 128, (1024, 2048, 3)).astype(np.uint8)
        Image.fromarray(img.astype(np.uint8)).save(os.path.join(img_dir, "frankfurt_%s_leftImg8bit.png" % c),
                                                   compress_level=1)
        ids = np.load(os.path.join(ROOT, "tests", "golden", "instance_ap_%s.npz" % c))["gt_ids"]
        Image.fromarray(ids).save(os.path.join(gt_dir, "val", "frankfurt", "frankfurt_%s_gtFine_instanceIds.png" % c))
    images = [{"id": 10 + k, "file_name": "frankfurt_%s_leftImg8bit.png" % CASES[k % 4], "height": 1024, "width": 2048}
              for k in range(4 * repeat)]
    with open(os.path.join(annot_dir, "val16_regular_interval.json"), "w") as f:
        json.dump({"images": images, "annotations": [], "categories": []}, f)
    if not load_model:
        torch.manual_seed(23)
        model = create_model("dla_34", {"hm": 8, "poly": 32, "pseudo_depth": 1, "reg": 2}, 256)
        with torch.no_grad():
            ang = np.arange(16) * (2 * np.pi / 16)
            rad = rng.uniform(6, 10, 16)
            bias = np.stack([rad * np.cos(ang), rad * np.sin(ang)], 1).reshape(-1)
            model.state_dict()["poly.2.bias"].copy_(torch.from_numpy(bias.astype(np.float32)))
            model.state_dict()["hm.2.bias"].fill_(-1.0)
        load_model = os.path.join(tmp, "model_seeded.pth")
        save_model(load_model, 1, model)
    return ["polydet", "--dataset", "cityscapes", "--annot_dir", annot_dir, "--img_dir", img_dir,
            "--load_model", load_model], gt_dir


def spread(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def kernel_alone(ds, rows_dev, a):
    R, N = int(rows_dev.shape[0]), (int(rows_dev.shape[1]) - 7) // 2
    dev = rows_dev.device
    table = np.ascontiguousarray(ds.class_table())
    n = torch.empty((1,), dtype=torch.int32, device=dev)
    src, label = (torch.empty((R,), dtype=torch.int32, device=dev) for _ in range(2))
    poly = torch.empty((R, N, 2), dtype=torch.int32, device=dev)
    flags = torch.empty((R,), dtype=torch.uint8, device=dev)
    conf = torch.empty((R,), dtype=torch.float32, device=dev)
    L = _C.lib()

    def call():
        _C.check(L.cp_writer_instances(_C.ptr(rows_dev), R, N, float(ds.opt.thresh),
                                       table.ctypes.data_as(ctypes.c_void_p), len(table), _C.ptr(n), _C.ptr(src),
                                       _C.ptr(poly), _C.ptr(flags), _C.ptr(label), _C.ptr(conf), _C.stream()),
                 "cp_writer_instances")
    for _ in range(10):
        call()
    torch.cuda.synchronize()
    us = []
    for _ in range(a.rounds):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(a.iters):
            call()
        e.record()
        torch.cuda.synchronize()
        us.append(s.elapsed_time(e) / a.iters * 1e3)
    return dict(spread(us), R=R, N=N, live=int(n.cpu()[0]))


def tables_of(ev):
    return [(t.tolist(), [(p[0], p[1], p[2], p[3], p[4].tolist()) for p in preds]) for t, preds in ev.images]


def tails(detector, ds, items, a):
    """Per image: process() -> synchronise -> [common] -> the two tails in alternating order, timed by the host clock
    (each tail ends with its tables on the host)."""
    def parent_tail(results, item, ev):
        params = ds.image_instances(results)
        masks_dev, counts_dev = ds.instance_masks_device(params)
        counts = counts_dev.cpu().numpy()
        kept = [k for k, (p, nz) in enumerate(zip(params, counts)) if p[2] not in ds.no_mask_labels and nz > 100]
        confs = [str(min(1, params[k][1] * 1.2)) for k in kept]
        sel = masks_dev if len(kept) == len(params) else masks_dev[kept]
        ev.add_image(sel, [ds.label_to_id[params[k][2]] for k in kept], [float(c) for c in confs], item["gt_ids"])

    def new_tail(results, item, ev):
        ds.score_instances_device(detector.device_rows(results), item["gt_ids"], item["gt_table"], ev)

    per_pass = {"common": [], "tail_new": [], "tail_parent": []}
    kept = []
    for rnd in range(a.tail_rounds + 2):                                  # two warm-up passes
        acc = {k: [] for k in per_pass}
        evs = {"tail_new": il.InstanceLevelEvaluator(), "tail_parent": il.InstanceLevelEvaluator()}
        for i, item in enumerate(items):
            images, meta = detector.pre_process(item["image"], 1.0)
            _, dets = detector.process(images)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            results = detector.merge_outputs([detector.post_process(dets, meta, 1.0)])
            acc["common"].append((time.perf_counter() - t0) * 1e3)
            order = [("tail_new", new_tail), ("tail_parent", parent_tail)]
            for name, fn in (order if (rnd + i) % 2 == 0 else order[::-1]):
                torch.cuda.synchronize()
                s = time.perf_counter()
                fn(results, item, evs[name])
                acc[name].append((time.perf_counter() - s) * 1e3)
        if tables_of(evs["tail_new"]) != tables_of(evs["tail_parent"]):
            raise SystemExit("the two tails disagree on the count tables")
        kept = [len(p) for _, p in evs["tail_new"].images]
        if rnd >= 2:
            for k in per_pass:
                per_pass[k].append(float(np.mean(acc[k])))
    out = {k: spread(v) for k, v in per_pass.items()}
    out["kept_per_image"] = kept
    out["passes"] = a.tail_rounds
    return out


def driver_rates(base, gt_dir, a, tmp):
    spec = importlib.util.spec_from_file_location("centerpoly_test_driver", os.path.join(ROOT, "test.py"))
    drv = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(drv)
    scored = ["--gt_dir", gt_dir, "--no_mask_files"]
    # (the plain variants would end in run_eval's mask files: the loop alone is run)
    variants = [("plain_prefetch", []), ("plain_loop", ["--not_prefetch_test"]), ("scored_prefetch", scored),
                ("scored_loop", scored + ["--not_prefetch_test"])]
    out = {}
    for rep in range(a.driver_reps):                                      # variants alternate within a repetition
        for name, extra in variants:
            opt = opts().parse(base + extra + ["--num_workers", str(a.num_workers)])
            opt.save_dir = os.path.join(tmp, "exp_%s_%d" % (name, rep))
            with contextlib.redirect_stdout(io.StringIO()):
                st = drv.run_test(opt, evaluate=bool(opt.gt_dir))["stamps"]
            out.setdefault(name, []).append((len(st) - 1 - a.skip) / (st[-1] - st[a.skip]))
            torch.cuda.empty_cache()
    return {k: dict(spread(v), unit="img/s") for k, v in out.items()}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rounds", type=int, default=7)
    p.add_argument("--iters", type=int, default=200)
    p.add_argument("--tail-rounds", type=int, default=10)
    p.add_argument("--repeat", type=int, default=10, help="the four images are listed this many times for test.py")
    p.add_argument("--skip", type=int, default=8)
    p.add_argument("--driver-reps", type=int, default=3)
    p.add_argument("--num_workers", type=int, default=4)
    p.add_argument("--load_model", default="")
    p.add_argument("--json", default="")
    a = p.parse_args()
    tmp = tempfile.mkdtemp()
    base, gt_dir = make_set(tmp, a.repeat, a.load_model)
    from centerpoly_amd.datasets import eval_images
    from centerpoly_amd.datasets.dataset_factory import get_dataset
    from centerpoly_amd.detectors.detector_factory import detector_factory
    opt = opts().parse(base + ["--gt_dir", gt_dir, "--no_mask_files"])
    Dataset = get_dataset(opt.dataset, opt.task)
    opt = opts().update_dataset_info_and_set_heads(opt, Dataset)
    with contextlib.redirect_stdout(io.StringIO()):
        ds = Dataset(opt, "val")
        detector = detector_factory[opt.task](opt)
    images = eval_images.EvalImages(ds, il.find_gt_files(gt_dir))
    t0 = time.perf_counter()
    items = [images[i] for i in range(4)]
    decode_all = (time.perf_counter() - t0) / 4 * 1e3
    dec = []
    for _ in range(3):
        for i in range(4):
            t0 = time.perf_counter()
            ds.read_image(images.info(i)[1])
            dec.append((time.perf_counter() - t0) * 1e3)
    result = {"png_decode_ms_per_image": spread(dec), "image_and_gt_decode_ms_per_image": decode_all}
    print("PNG decode %.1f ms per image (with id image and table %.1f ms)" % (np.median(dec), decode_all))

    ret = detector.run(items[0]["image"])
    result["kernel_us"] = kernel_alone(ds, detector.device_rows(ret["results"]), a)
    print("cp_writer_instances: %.1f us [%.1f, %.1f] at R = %d, N = %d, %d live"
          % tuple(result["kernel_us"][k] for k in ("median", "min", "max", "R", "N", "live")))

    t = result["tail_ms_per_image"] = tails(detector, ds, items, a)
    print("per image after process(): common %.2f ms; tail new %.2f [%.2f, %.2f] ms, parent %.2f [%.2f, %.2f] ms; "
          "kept %s" % (t["common"]["median"], t["tail_new"]["median"], t["tail_new"]["min"], t["tail_new"]["max"],
                       t["tail_parent"]["median"], t["tail_parent"]["min"], t["tail_parent"]["max"],
                       t["kept_per_image"]))

    rates = []
    for rep in range(a.driver_reps + 1):                                  # PolydetDetector.run on host arrays
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for k in range(4 * a.repeat):
            detector.run(items[k % 4]["image"])
        rates.append(4 * a.repeat / (time.perf_counter() - t0))
    result["detector_run_img_per_s"] = spread(rates[1:])
    print("PolydetDetector.run on decoded arrays: %.0f img/s [%.0f, %.0f]"
          % tuple(result["detector_run_img_per_s"][k] for k in ("median", "min", "max")))
    del detector
    torch.cuda.empty_cache()

    result["test_py_img_per_s"] = driver_rates(base, gt_dir, a, tmp)
    for k, v in result["test_py_img_per_s"].items():
        print("test.py %-16s %.1f img/s [%.1f, %.1f]" % (k, v["median"], v["min"], v["max"]))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()

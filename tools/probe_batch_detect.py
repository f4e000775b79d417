"""GPU probe: what a batch of images per launch gains the detector (run_batch against run).

A DLA-34 with seeded weights (synth.fill_by_name; K = 128, 8 classes, 16 vertices) on seeded host uint8 images of the
network's input size, at 512x1024 and 1024x2048, for B in {1, 2, 4, 8}.

1. Whole path: images per second through `run` (one image per call, the unchanged baseline) and through `run_batch`
   (B images per call, B = 1 included), host clock around calls that end in a synchronise.  The two alternate in the
   same process, every shape is warmed up, a window lasts `--window` seconds; median and [min, max] over `--passes`
   passes.  At B = 1 the two must give the same results, bit for bit, or the probe stops.
2. Network alone: HIP events around model(x) at each B, ms per image, so that the network's scaling is separate from
   the host tail.
3. The new kernel alone: cp_preprocess_warp_normalize_batch against B calls of cp_preprocess_warp_normalize (HIP
   events, us per batch), with the bytes each moves per output pixel.

Usage:  python tools/probe_batch_detect.py [--json OUT]
        python tools/probe_batch_detect.py --trace B --shape HxW     (a fixed number of run_batch calls and nothing
            else, for `rocprofv3 --kernel-trace --stats -- python ...` in a run of its own)
        python tools/probe_batch_detect.py --compare STATS_B1.csv STATS_BN.csv --per 1 N
            (host only: the two runs' kernel statistics as time per image side by side with their ratio, the
            most time per image at B = N first; a ratio near 1 is a launch that did not scale)
"""
import argparse
import contextlib
import csv
import io
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

SHAPES = ((512, 1024), (1024, 2048))
BATCHES = (1, 2, 4, 8)
TRACE_CALLS = 24                                                          # images per --trace run: 8 warm-up + 24


def spread(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def same(a, b):
    return sorted(a) == sorted(b) and all(a[j].shape == b[j].shape and np.array_equal(a[j].view(np.uint32),
                                                                                      b[j].view(np.uint32)) for j in a)


def seeded_weights():
    """Seeded weights by parameter name: a freshly initialised network scores every centre alike."""
    import torch
    from centerpoly_amd import synth
    from centerpoly_amd.models.model import create_model, save_model
    model = create_model("dla_34", {"hm": 8, "poly": 32, "pseudo_depth": 1, "reg": 2}, 256)
    w = synth.fill_by_name({k: tuple(v.shape) for k, v in model.state_dict().items()})
    model.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()})
    path = os.path.join(tempfile.mkdtemp(), "model_seeded.pth")
    save_model(path, 1, model)
    return path


def detector(h, w, weights):
    from centerpoly_amd.detectors.detector_factory import detector_factory
    from centerpoly_amd.opts import opts
    with contextlib.redirect_stdout(io.StringIO()):
        opt = opts().init(["polydet", "--arch", "dla_34", "--K", "128", "--input_h", str(h), "--input_w", str(w),
                           "--load_model", weights])
        return detector_factory["polydet"](opt)


def images(h, w, n):
    from centerpoly_amd import synth
    return [(synth.uniform("probe_batch_detect/img%d" % i, (h, w, 3)) * 255).astype(np.uint8) for i in range(n)]


def window(call, per_call, seconds):
    """Images per second of `call` (which ends synchronised) repeated for at least `seconds`."""
    import torch
    torch.cuda.synchronize()
    n, t0 = 0, time.perf_counter()
    while True:
        call()
        n += per_call
        dt = time.perf_counter() - t0
        if dt >= seconds:
            return n / dt


def whole_path(det, imgs, B, a):
    group = imgs[:B]
    state = {"i": 0}

    def single():
        det.run(imgs[state["i"] % len(imgs)])
        state["i"] += 1

    def batch():
        det.run_batch(group)

    for _ in range(2):                                                    # every shape is warmed up
        for im in group:
            det.run(im)
        batch()
    if B == 1 and not same(det.run(group[0])["results"], det.run_batch(group)["results"][0]):
        raise SystemExit("run and run_batch disagree on one image")
    rates = {"run": [], "run_batch": []}
    for p in range(a.passes):
        for name in (("run", "run_batch") if p % 2 == 0 else ("run_batch", "run")):
            rates[name].append(window(single if name == "run" else batch, 1 if name == "run" else B, a.window))
    return {k: spread(v) for k, v in rates.items()}


def network_alone(det, imgs, B, a):
    import torch
    x, _ = det.pre_process_batch(imgs[:B], 1.0)
    with torch.no_grad():
        for _ in range(3):
            det.model(x)
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.rounds):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(a.net_iters):
                det.model(x)
            e.record()
            torch.cuda.synchronize()
            ms.append(s.elapsed_time(e) / a.net_iters / B)
    return spread(ms)


def kernel_alone(det, imgs, B, h, w, a):
    import torch
    from centerpoly_amd.utils.image import get_affine_transform, warp_affine_normalize, warp_affine_normalize_batch
    dev = det.opt.device
    group = imgs[:B]
    c = np.array([w / 2.0, h / 2.0], dtype=np.float32)
    t = get_affine_transform(c, max(h, w) * 1.0, 0, [w, h])
    singles = [torch.from_numpy(im).to(dev) for im in group]
    flat = torch.cat([s.view(-1) for s in singles])
    hw = np.array([[h, w]] * B, np.int32)
    off = np.arange(B, dtype=np.int64) * (h * w * 3)
    trans = np.stack([t.reshape(6)] * B)

    def per_image():
        for s in singles:
            warp_affine_normalize(s, t, det.mean, det.std, h, w)

    def batched():
        warp_affine_normalize_batch(flat, hw, off, trans, det.mean, det.std, h, w)

    out = {}
    for name, call in (("per_image_calls", per_image), ("batch_call", batched)):
        for _ in range(5):
            call()
        torch.cuda.synchronize()
        us = []
        for _ in range(a.rounds):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(a.kernel_iters):
                call()
            e.record()
            torch.cuda.synchronize()
            us.append(s.elapsed_time(e) / a.kernel_iters * 1e3)
        out[name] = spread(us)
    # bytes the algorithm needs: 12 B written per output pixel, 3 B read per source pixel (scale 1 here)
    out["bytes_per_batch"] = B * h * w * (12 + 3)
    out["GBps_batch_call"] = out["bytes_per_batch"] / (out["batch_call"]["median"] * 1e-6) / 1e9
    return out


def trace(a):
    """A fixed amount of run_batch work and nothing else (for rocprofv3 around this process)."""
    import torch
    h, w = (int(v) for v in a.shape.lower().split("x"))
    det = detector(h, w, seeded_weights())
    imgs = images(h, w, a.trace)
    for _ in range(max(1, 8 // a.trace)):
        det.run_batch(imgs)
    for _ in range(max(1, TRACE_CALLS // a.trace)):
        det.run_batch(imgs)
    torch.cuda.synchronize()
    print("traced %d warm-up and %d timed images at B = %d, %dx%d"
          % (max(1, 8 // a.trace) * a.trace, max(1, TRACE_CALLS // a.trace) * a.trace, a.trace, h, w))


def compare(a):
    """Two rocprofv3 kernel_stats CSVs (B = per[0] and B = per[1], the same number of images each) as time per image."""
    tables = []
    for path in a.compare:
        with open(path, newline="") as f:
            tables.append({r["Name"]: (int(r["Calls"]), float(r["TotalDurationNs"])) for r in csv.DictReader(f)})
    images_run = [(max(1, 8 // b) + max(1, TRACE_CALLS // b)) * b for b in a.per]
    rows = []
    for name in sorted(set(tables[0]) | set(tables[1])):
        one, many = tables[0].get(name, (0, 0.0)), tables[1].get(name, (0, 0.0))
        rows.append((many[1] / images_run[1] / 1e3, one[1] / images_run[0] / 1e3, one[0], many[0], name))
    tot = [sum(r[1] for r in rows), sum(r[0] for r in rows)]
    print("kernel time per image: B = %d %.1f us, B = %d %.1f us" % (a.per[0], tot[0], a.per[1], tot[1]))
    print("%10s %10s %7s %7s %7s  kernel" % ("us/img B=%d" % a.per[0], "us/img B=%d" % a.per[1], "ratio", "calls", "calls"))
    for many, one, c1, cn, name in sorted(rows, reverse=True):              # the most time per image at B = per[1] first
        if max(many, one) < 1.0:
            continue
        print("%10.1f %10.1f %7.2f %7d %7d  %s" % (one, many, many / one if one else float("inf"), c1, cn, name[:110]))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--passes", type=int, default=3)
    p.add_argument("--window", type=float, default=2.5, help="seconds per timed window")
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--net_iters", type=int, default=10)
    p.add_argument("--kernel_iters", type=int, default=50)
    p.add_argument("--json", default="")
    p.add_argument("--trace", type=int, default=0, help="B: only run_batch calls at this batch size")
    p.add_argument("--shape", default="512x1024")
    p.add_argument("--compare", nargs=2, default=None)
    p.add_argument("--per", nargs=2, type=int, default=[1, 8])
    a = p.parse_args()
    if a.compare:
        return compare(a)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("probe_batch_detect needs a GPU: nothing is measured without one")
    if a.trace:
        return trace(a)
    weights = seeded_weights()
    result = {"unit_whole_path": "images per second", "unit_network": "ms per image", "unit_kernel": "us per batch",
              "passes": a.passes, "window_s": a.window, "device": torch.cuda.get_device_name(0)}
    for h, w in SHAPES:
        det = detector(h, w, weights)
        imgs = images(h, w, max(BATCHES))
        shape = result["%dx%d" % (h, w)] = {}
        for B in BATCHES:
            r = shape["B%d" % B] = {"whole_path": whole_path(det, imgs, B, a), "network": network_alone(det, imgs, B, a),
                                    "warp_kernel": kernel_alone(det, imgs, B, h, w, a)}
            wp, net, k = r["whole_path"], r["network"], r["warp_kernel"]
            print("%dx%d B = %d: run %.1f img/s [%.1f, %.1f], run_batch %.1f img/s [%.1f, %.1f]; network %.3f ms/img "
                  "[%.3f, %.3f]; warp: %d single calls %.1f us, one batch call %.1f us (%.0f GB/s)"
                  % (h, w, B, wp["run"]["median"], wp["run"]["min"], wp["run"]["max"], wp["run_batch"]["median"],
                     wp["run_batch"]["min"], wp["run_batch"]["max"], net["median"], net["min"], net["max"], B,
                     k["per_image_calls"]["median"], k["batch_call"]["median"], k["GBps_batch_call"]), flush=True)
        del det
        torch.cuda.empty_cache()
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()

"""GPU probe: what the instance maps cost (cp_instance_map, the torch composition of the same maps, instances()).

1. The kernel alone at n = 128 on 2048 x 1024: 128 seeded polygons of about 1 % of the frame each, selected and drawn by
   the KITTI writer's kernels (cp_class_writer_instances -> cp_class_instance_masks), merged by depth.  HIP events
   around `--kernel_iters` calls, median and [min, max] over `--rounds`, with NULL bounds (every plane is a candidate
   everywhere) and with the bounds instance_maps passes (the vertices' boxes).  The bytes the algorithm needs are counted
   from the inputs by `needed_bytes`: a 16-byte piece of a plane is read where the piece meets the clipped bounds and
   still holds an undecided pixel when the instance's turn comes, plus 9 bytes written per pixel (index, ids, labels).
   A lane issues 8 planes of its tile's list at once, so pieces that an earlier plane of those 8 decides are read as
   well; they are not counted.  The fraction of HBM bandwidth is that count over the time over 8.0 TB/s.
2. The same six outputs composed with torch ops on the masks (an [n, H, W] key tensor, amin over n, look-ups, bincount
   and scatter-reduce for the boxes), HIP events likewise.  The two must agree in every bit or the probe stops.
3. instances() after run(): a DLA-34 with seeded weights (polygon bias of 10 to 40 output pixels radius, so the
   instances have masks) at 1024 x 2048 and K = 128, --dataset cityscapes and kitti_poly; host clock around calls that
   end in a synchronise, ms per image.

Usage:  python tools/probe_instances.py [--json OUT]
        python tools/probe_instances.py --trace CALLS     (CALLS calls of cp_instance_map with NULL bounds, then CALLS
            with the vertices' bounds, and nothing else timed: for `rocprofv3 --kernel-trace --stats -- python ...` in a
            run of its own, which gives the two kernels' own times without the launches' gaps)
"""
import argparse
import contextlib
import io
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

H, W, N_INST, N_VERT = 1024, 2048, 128, 16
HBM_PEAK = 8.0e12                                                         # bytes per second, the data sheet's


def spread(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def realistic_rows():
    """128 seeded rows: 16-gons of 40 to 120 pixels radius (about 1 % of the frame on average), 8 classes."""
    rng = np.random.RandomState(3)
    rows = np.zeros((N_INST, 2 * N_VERT + 7), np.float32)
    for r in range(N_INST):
        cx, cy, rad = rng.uniform(0, W), rng.uniform(0, H), rng.uniform(40, 120)
        ang = np.sort(rng.uniform(0, 2 * np.pi, N_VERT))
        rr = rad * rng.uniform(0.7, 1.0, N_VERT)
        pts = np.stack([cx + rr * np.cos(ang), cy + rr * np.sin(ang)], 1)
        rows[r, 6:6 + 2 * N_VERT] = pts.reshape(-1)
        rows[r, 0:4] = [pts[:, 0].min(), pts[:, 1].min(), pts[:, 0].max(), pts[:, 1].max()]
        rows[r, 4], rows[r, 5], rows[r, -1] = rng.uniform(0.3, 0.95), rng.randint(0, 8), rng.uniform(1, 80)
    return rows


def timed(call, iters, rounds):
    """us per call: HIP events around `iters` calls, `rounds` times, after a warm-up."""
    import torch
    for _ in range(3):
        call()
    torch.cuda.synchronize()
    us = []
    for _ in range(rounds):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(iters):
            call()
        e.record()
        torch.cuda.synchronize()
        us.append(s.elapsed_time(e) / iters * 1e3)
    return spread(us)


def needed_bytes(masks, live, order, bounds):
    """Bytes the algorithm needs for these inputs (see the module's text): (read, written)."""
    import torch
    n, h, w = masks.shape
    undecided = torch.ones((h, w), dtype=torch.bool, device=masks.device)
    ys = torch.arange(h, device=masks.device)[:, None]
    xs = torch.arange(w, device=masks.device)[None, :]
    pieces = 0
    for i in order:
        if not live[i]:
            continue
        x0, y0, x1, y1 = (0, 0, w - 1, h - 1) if bounds is None else bounds[i]
        window = (ys >= y0) & (ys <= y1) & (xs >= x0) & (xs <= x1)
        wanted = undecided & window
        pieces += int(wanted.view(h, w // 16, 16).any(-1).sum())
        undecided &= ~(wanted & (masks[i] != 0))
    return pieces * 16, h * w * 9


def torch_maps(masks, live, rank, label, value):
    """The six outputs from torch ops on the masks (no bounds: they change nothing here)."""
    import torch
    n, h, w = masks.shape
    dev = masks.device
    key = torch.where((masks != 0) & live.view(n, 1, 1), rank.view(n, 1, 1), torch.tensor(255, dtype=torch.int16, device=dev))
    first = key.amin(0).long()                                            # the winner's rank, 255 for none
    by_rank = torch.full((256,), 255, dtype=torch.long, device=dev)
    by_rank[rank[live].long()] = torch.nonzero(live).view(-1)
    index = by_rank[first]
    lut_value = torch.zeros((256,), dtype=torch.int32, device=dev)
    lut_label = torch.zeros((256,), dtype=torch.int32, device=dev)
    lut_value[:n], lut_label[:n] = value, label
    ids, labels = lut_value[index], lut_label[index]
    flat = index.view(-1)
    visible = torch.bincount(flat, minlength=256)[:n].to(torch.int32)
    ys = torch.arange(h, device=dev).view(h, 1).expand(h, w).reshape(-1)
    xs = torch.arange(w, device=dev).view(1, w).expand(h, w).reshape(-1)
    box = torch.stack([torch.full((256,), w, device=dev).scatter_reduce(0, flat, xs, "amin"),
                       torch.full((256,), h, device=dev).scatter_reduce(0, flat, ys, "amin"),
                       torch.full((256,), -1, device=dev).scatter_reduce(0, flat, xs, "amax"),
                       torch.full((256,), -1, device=dev).scatter_reduce(0, flat, ys, "amax")], 1)[:n].to(torch.int32)
    return index.to(torch.uint8), ids, labels, visible, box


def kernel_and_composition(a):
    import ctypes

    import torch
    from centerpoly_amd import _C
    from centerpoly_amd.datasets.dataset_factory import dataset_factory
    from centerpoly_amd.detectors import instances
    dev = torch.device("cuda")
    rows = torch.from_numpy(realistic_rows()).to(dev)
    maps = instances.instance_maps(rows, dataset_factory["kitti_poly"], (W, H), thresh=0.05)
    t = maps.table
    n = t["n"]
    assert n == N_INST and t["live"].all()
    masks = maps.masks
    flags = torch.ones((n,), dtype=torch.uint8, device=dev)
    label = torch.from_numpy(t["label"]).to(dev)
    prio = rows[torch.from_numpy(t["src"]).long().to(dev), -1].contiguous()
    bounds = instances.vertex_bounds(torch.from_numpy(t["poly"]).to(dev), instances.MARGIN["class"], (W, H))
    order = np.argsort(prio.cpu().numpy(), kind="stable")
    rank = torch.empty((n,), dtype=torch.int16, device=dev)
    rank[torch.from_numpy(order).to(dev)] = torch.arange(n, dtype=torch.int16, device=dev)
    live = torch.ones((n,), dtype=torch.bool, device=dev)
    out = {"n": n, "H": H, "W": W, "mask_bytes": n * H * W,
           "covered_fraction": float((maps.index != 255).float().mean()),
           "mean_mask_fraction": float((masks != 0).float().mean())}
    results = {}
    # the timed call is the C entry alone on buffers made once (instances.instance_map allocates its outputs on every
    # call, which costs the host more than the kernel takes with bounds)
    L = _C.lib()
    index = torch.empty((H, W), dtype=torch.uint8, device=dev)
    ids, labels = (torch.empty((H, W), dtype=torch.int32, device=dev) for _ in range(2))
    value, visible = (torch.empty((n,), dtype=torch.int32, device=dev) for _ in range(2))
    box = torch.empty((n, 4), dtype=torch.int32, device=dev)
    nbytes = L.cp_instance_map_workspace_bytes(n, H, W)
    ws = _C.workspace(nbytes, dev)

    def entry(b):
        _C.check(L.cp_instance_map(_C.ptr(masks), n, H, W, _C.ptr(flags), 1, None, 0, _C.ptr(label), _C.ptr(prio),
                                   _C.ptr(b), 256, 0, _C.ptr(index), _C.ptr(ids), _C.ptr(labels), _C.ptr(value),
                                   _C.ptr(visible), _C.ptr(box), _C.ptr(ws), nbytes, _C.stream()), "cp_instance_map")

    if a.trace:                                                           # for rocprofv3 around this process
        for b in (None, bounds):
            for _ in range(a.trace):
                entry(b)
        torch.cuda.synchronize()
        print("traced %d calls with NULL bounds, then %d with the vertices' bounds" % (a.trace, a.trace))
        return None
    for name, b in (("null_bounds", None), ("vertex_bounds", bounds)):
        call = lambda b=b: entry(b)                                       # noqa: E731
        call()
        results[name] = [v.clone() for v in (index, ids, labels, value, visible, box)]
        wrapped = instances.instance_map(masks, flags, label, 1, None, 0, prio, b, 256, 0)
        if not all(torch.equal(x, y) for x, y in zip(results[name], wrapped)):
            raise SystemExit("the wrapper and the entry disagree")
        r = out[name] = {"us": timed(call, a.kernel_iters, a.rounds)}
        read, written = needed_bytes(masks, [True] * n, order.tolist(), None if b is None else b.cpu().numpy().tolist())
        r["bytes_read"], r["bytes_written"] = read, written
        r["GBps"] = (read + written) / (r["us"]["median"] * 1e-6) / 1e9
        r["fraction_of_hbm_peak"] = r["GBps"] * 1e9 / HBM_PEAK
        r["read_fraction_of_all_planes"] = read / float(n * H * W)
    for x, y in zip(results["null_bounds"], results["vertex_bounds"]):
        if not torch.equal(x, y):
            raise SystemExit("the bounds changed the maps")
    value = results["null_bounds"][3]
    call = lambda: torch_maps(masks, live, rank, label, value)            # noqa: E731
    index, ids, labels, visible, box = call()
    k = results["null_bounds"]
    for name, x, y in (("index", index, k[0]), ("ids", ids, k[1]), ("labels", labels, k[2]), ("visible", visible, k[4]),
                       ("box", box, k[5])):
        if not torch.equal(x, y):
            raise SystemExit("the torch composition and the kernel disagree on %s" % name)
    out["torch_composition"] = {"us": timed(call, max(1, a.kernel_iters // 10), a.rounds)}
    return out


def seeded_weights():
    import torch
    from centerpoly_amd import synth
    from centerpoly_amd.models.model import create_model, save_model
    model = create_model("dla_34", {"hm": 8, "poly": 32, "pseudo_depth": 1, "reg": 2}, 256)
    w = synth.fill_by_name({k: tuple(v.shape) for k, v in model.state_dict().items()})
    ang = np.arange(16) * (2 * np.pi / 16)
    rad = np.random.RandomState(11).uniform(10, 40, 16)
    w["poly.2.bias"] = np.stack([rad * np.cos(ang), rad * np.sin(ang)], 1).reshape(-1).astype(np.float32)
    w["hm.2.bias"] = np.full_like(w["hm.2.bias"], -1.0)
    model.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in w.items()})
    path = os.path.join(tempfile.mkdtemp(), "model_seeded.pth")
    save_model(path, 1, model)
    return path


def per_image(a, weights, dataset):
    import torch
    from centerpoly_amd import synth
    from centerpoly_amd.datasets.dataset_factory import dataset_factory
    from centerpoly_amd.detectors.detector_factory import detector_factory
    from centerpoly_amd.opts import opts
    with contextlib.redirect_stdout(io.StringIO()):
        opt = opts().parse(["polydet", "--arch", "dla_34", "--K", "128", "--input_h", str(H), "--input_w", str(W),
                            "--dataset", dataset, "--load_model", weights])
        opt = opts().update_dataset_info_and_set_heads(opt, dataset_factory[dataset])
        det = detector_factory["polydet"](opt)
    img = (synth.uniform("probe_instances/img", (H, W, 3)) * 255).astype(np.uint8)
    ret = det.run(img)
    for _ in range(3):
        maps = det.instances(ret["results"])
    torch.cuda.synchronize()
    ms = []
    for _ in range(a.image_calls):
        t0 = time.perf_counter()
        maps = det.instances(ret["results"])
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    run_ms = []
    for _ in range(5):
        t0 = time.perf_counter()
        det.run(img)
        torch.cuda.synchronize()
        run_ms.append((time.perf_counter() - t0) * 1e3)
    return {"instances_ms": spread(ms), "run_ms": spread(run_ms), "selected": int(maps.table["n"]),
            "live": int(maps.table["live"].sum()), "covered_fraction": float((maps.index != 255).float().mean())}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rounds", type=int, default=7)
    p.add_argument("--kernel_iters", type=int, default=50)
    p.add_argument("--image_calls", type=int, default=30)
    p.add_argument("--json", default="")
    p.add_argument("--trace", type=int, default=0, help="only this many cp_instance_map calls per kind of bounds")
    a = p.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("probe_instances needs a GPU: nothing is measured without one")
    if a.trace:
        return kernel_and_composition(a)
    result = {"unit_kernel": "us per call", "unit_per_image": "ms per image", "rounds": a.rounds,
              "kernel_iters": a.kernel_iters, "device": torch.cuda.get_device_name(0)}
    k = result["kernel"] = kernel_and_composition(a)
    for name in ("null_bounds", "vertex_bounds"):
        r = k[name]
        print("cp_instance_map n = %d %dx%d %s: %.1f us [%.1f, %.1f]; needs %.1f MB read (%.1f %% of the planes) + %.1f MB "
              "written: %.0f GB/s, %.1f %% of the HBM peak"
              % (k["n"], W, H, name, r["us"]["median"], r["us"]["min"], r["us"]["max"], r["bytes_read"] / 1e6,
                 100 * r["read_fraction_of_all_planes"], r["bytes_written"] / 1e6, r["GBps"],
                 100 * r["fraction_of_hbm_peak"]), flush=True)
    tc = k["torch_composition"]["us"]
    print("the same maps from torch ops: %.1f us [%.1f, %.1f]" % (tc["median"], tc["min"], tc["max"]), flush=True)
    weights = seeded_weights()
    result["per_image"] = {}
    for dataset in ("cityscapes", "kitti_poly"):
        r = result["per_image"][dataset] = per_image(a, weights, dataset)
        print("instances() after run(), %s at %dx%d, K = 128: %.3f ms per image [%.3f, %.3f] (%d selected, %d live, "
              "%.0f %% of the frame covered); run() itself %.2f ms"
              % (dataset, H, W, r["instances_ms"]["median"], r["instances_ms"]["min"], r["instances_ms"]["max"],
                 r["selected"], r["live"], 100 * r["covered_fraction"], r["run_ms"]["median"]), flush=True)
        torch.cuda.empty_cache()
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()

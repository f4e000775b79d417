"""Ragged training batches: images of different sizes travel back to back (`collate_ragged`) and
cp_sample_inputs_batch forms the dense network input on the device, image for image what `build_inputs` gives.
CPU: the collate's layout, a loader over a mixed-size data set, the entry point's refusals.  GPU: the batch kernel
against the per-image path (bit for bit without colour augmentation) and against oracle/pre.py, chunking, the trainer."""
import ctypes
import functools
import itertools
import json
import os

import numpy as np
import pytest
import torch

from centerpoly_amd import _C

MEAN, STD = (0.284, 0.323, 0.282), (0.0423, 0.0409, 0.0427)
SIZES = ((37, 53), (64, 48), (20, 91))                       # (H, W) of the three sources
DST_H, DST_W = 24, 300                                       # two x-blocks of 256, the second ragged
# forward maps source -> 24 x 300: a ~0.6x downscale (slightly sheared), a 1.7x upscale, and a 3.4x / 1.5x stretch
# whose window leaves the 20 x 91 source on the left and the top (constant border 0)
TRANS = np.array([[0.6, 0.03, 40.25, -0.02, 0.6, 1.5],
                  [1.7, 0.0, 110.0, 0.0, 1.7, -30.5],
                  [3.4, 0.1, 35.5, 0.0, 1.5, 6.25]], np.float64)
ORDERS = list(itertools.permutations((0, 1, 2)))             # all six op orders, two per parametrised case


def _sources(sizes=SIZES, seed=21):
    rng = np.random.RandomState(seed)
    return [rng.randint(0, 256, (h, w, 3), dtype=np.uint8) for h, w in sizes]


def _color_rows(order0, order2):
    return np.array([[1, *order0, 0.7, 1.3, 0.9, 0.01, -0.02, 0.005],
                     [0, 0, 0, 0, 1, 1, 1, 0, 0, 0],
                     [1, *order2, 1.25, 0.8, 1.1, -0.015, 0.004, 0.02]], np.float64)


def _items(images):
    """What PolydetDataset.__getitem__ returns, as far as the collate is concerned."""
    from centerpoly_amd.datasets.sample.polydet import pack_annotations
    items = []
    for i, im in enumerate(images):
        anns = [{"bbox": [1.0 + i, 2.0, 9.0, 11.0], "poly": [float(k + i) for k in range(8)], "cls_id": i % 3,
                 "pseudo_depth": 0.5 * i, "freq": 0.2}]
        it = pack_annotations(anns, np.arange(6.0) + i, bool(i & 1), im.shape[1], 4, 4)
        it["image_u8"] = im
        it["trans_input"] = np.arange(6.0) * (i + 1)
        it["color"] = np.full(10, float(i))
        it["input_hw"] = np.array([64, 128], np.int32)
        items.append(it)
    return items


def _flat(images, dev=None):
    from centerpoly_amd.datasets.sample.polydet import collate_ragged
    b = collate_ragged([{"image_u8": im} for im in images])
    flat = b["image_flat"] if dev is None else b["image_flat"].to(dev)
    return flat, b["image_hw"], b["image_offset"]


@functools.lru_cache(maxsize=None)
def _oracle_warps():
    """x / 255 of oracle.pre.warp_affine_u8 for the three sources, float32 HWC; computed once, never modified."""
    from oracle import pre as opre
    out = []
    for im, t in zip(_sources(), TRANS):
        w = (opre.warp_affine_u8(im, t.reshape(2, 3), (DST_W, DST_H)) / 255.).astype(np.float32)
        w.setflags(write=False)
        out.append(w)
    return tuple(out)


def _write_mixed_dataset(root, nbr_points=16):
    """Four PNGs of two sizes (96x160 and 80x200, alternating) + train/val annotation files with the keys CocoIndex
    reads; returns the argument list of the drivers."""
    from PIL import Image
    rng = np.random.RandomState(4)
    images, anns = [], []
    for i in range(4):
        h, w = ((96, 160), (80, 200))[i % 2]
        name = "%06d_10.png" % i
        Image.fromarray(rng.randint(0, 256, (h, w, 3), dtype=np.uint8)).save(os.path.join(str(root), name))
        images.append({"id": i + 1, "file_name": name, "height": h, "width": w})
        for j in range(2):
            cx, cy, rx, ry = w * (0.3 + 0.4 * j), h * 0.5, w * 0.12, h * 0.2
            th = 2 * np.pi * np.arange(nbr_points) / nbr_points
            poly = np.stack([cx + rx * np.cos(th), cy + ry * np.sin(th)], 1).reshape(-1)
            anns.append({"id": len(anns) + 1, "image_id": i + 1, "category_id": (3, 1)[j], "pseudo_depth": 0.2 + 0.5 * j,
                         "bbox": [cx - rx, cy - ry, 2 * rx, 2 * ry], "poly": [float(v) for v in poly]})
    cats = [{"id": k, "name": n} for k, n in enumerate(("person", "rider", "car", "truck", "bus", "train",
                                                         "motorcycle", "bicycle"), 1)]
    for split in ("train", "val"):
        with open(os.path.join(str(root), "%s%d.json" % (split, nbr_points)), "w") as f:
            json.dump({"images": images, "annotations": anns, "categories": cats}, f)
    return ["polydet", "--dataset", "kitti_poly", "--annot_dir", str(root), "--img_dir", str(root), "--input_h", "64",
            "--input_w", "128", "--nbr_points", str(nbr_points)]


def _train_set(args):
    import contextlib
    import io
    from centerpoly_amd.datasets.dataset_factory import get_dataset
    from centerpoly_amd.opts import opts
    with contextlib.redirect_stdout(io.StringIO()):
        opt = opts().parse(args)
        Dataset = get_dataset(opt.dataset, opt.task)
        opt = opts().update_dataset_info_and_set_heads(opt, Dataset)
        return opt, Dataset(opt, "train")


# ------------------------------------------------------------------------------------------------ CPU

def test_collate_ragged_layout():
    from centerpoly_amd.datasets.sample.polydet import _FIELDS, collate, collate_ragged
    images = _sources()
    items = _items(images)
    batch = collate_ragged([dict(it) for it in items])
    assert "image_u8" not in batch and all("image_u8" in it for it in items)          # the items themselves are kept
    flat, hw, off = batch["image_flat"], batch["image_hw"], batch["image_offset"]
    assert flat.dtype == torch.uint8 and flat.dim() == 1 and hw.dtype == torch.int32 and off.dtype == torch.int64
    assert off.tolist() == [0, 37 * 53 * 3, 37 * 53 * 3 + 64 * 48 * 3]
    assert hw.tolist() == [[37, 53], [64, 48], [20, 91]]
    assert flat.numel() == sum(im.size for im in images)
    for b, im in enumerate(images):
        assert np.array_equal(flat[off[b]: off[b] + im.size].numpy().reshape(im.shape), im)
    ref = collate(items)
    for k in _FIELDS:
        assert batch[k].dtype == ref[k].dtype and torch.equal(batch[k], ref[k]), k
    for k in ("trans_input", "color", "input_hw"):
        assert np.array_equal(batch[k].numpy(), np.stack([it[k] for it in items])), k
    # `meta` (validation items) goes through the default collate as before
    for i, it in enumerate(items):
        it["meta"] = {"c": np.array([1.0, 2.0], np.float32) + i, "img_id": 7 + i}
    meta = collate_ragged(items)["meta"]
    assert meta["img_id"].tolist() == [7, 8, 9] and tuple(meta["c"].shape) == (3, 2)
    with pytest.raises(TypeError):
        collate_ragged([{"image_u8": np.zeros((4, 4), np.uint8)}])


@pytest.mark.parametrize("workers", [0, 2])
def test_loader_yields_mixed_size_batches(tmp_path, workers):
    """KITTI-like frames of two sizes at batch 2: the ragged collate yields every batch, torch's default collate dies
    in its stack (the limit this collate removes)."""
    from centerpoly_amd.datasets.sample.polydet import collate_ragged
    opt, ds = _train_set(_write_mixed_dataset(tmp_path))
    assert len(ds) == 4
    loader = torch.utils.data.DataLoader(ds, batch_size=2, shuffle=False, num_workers=workers, collate_fn=collate_ragged)
    np.random.seed(5)
    batches = list(loader)
    assert len(batches) == 2
    for batch in batches:
        assert sorted(batch["image_hw"].tolist()) == [[80, 200], [96, 160]]
        assert batch["image_offset"].tolist() == [0, 96 * 160 * 3]
        assert batch["image_flat"].numel() == 96 * 160 * 3 + 80 * 200 * 3
        assert batch["input_hw"].tolist() == [[64, 128], [64, 128]]
        assert tuple(batch["poly"].shape) == (2, 128, 32) and batch["num_objs"].tolist() == [2, 2]
        assert tuple(batch["trans_input"].shape) == (2, 6) and tuple(batch["color"].shape) == (2, 10)
    with pytest.raises(RuntimeError):
        next(iter(torch.utils.data.DataLoader(ds, batch_size=2, shuffle=False, num_workers=workers)))


@pytest.mark.parametrize("extra", [[], ["--device_targets"]])
def test_main_train_loader_keeps_the_synthetic_set(extra):
    """main.py's train loader on the offline synthetic set, whose items carry a ready `input` and no `image_u8`, with
    host targets and with --device_targets: the ragged collate hands such items to the default collate unchanged."""
    import contextlib
    import io
    from torch.utils.data import default_collate
    import main as driver
    from centerpoly_amd.datasets.dataset_factory import get_dataset
    from centerpoly_amd.datasets.sample.polydet import collate_ragged
    from centerpoly_amd.opts import opts
    with contextlib.redirect_stdout(io.StringIO()):
        opt = opts().parse(["polydet", "--dataset", "synthetic", "--input_h", "64", "--input_w", "64", "--batch_size", "2",
                            "--num_workers", "0"] + extra)
        Dataset = get_dataset(opt.dataset, opt.task)
        opt = opts().update_dataset_info_and_set_heads(opt, Dataset)
        ds = Dataset(opt, "train")
    loader, sampler = driver.make_train_loader(opt, ds, 2)
    assert sampler is None and loader.collate_fn is collate_ragged
    batch = next(iter(loader))
    assert tuple(batch["input"].shape) == (2, 3, 64, 64) and "image_flat" not in batch
    assert ("trans_output" in batch) == bool(extra) and ("hm" in batch) == (not extra)
    items = [ds[0], ds[1]]
    got, want = collate_ragged(items), default_collate(items)
    assert set(got) == set(want)
    for k in want:
        assert got[k].dtype == want[k].dtype and torch.equal(got[k], want[k]), k


def test_main_train_loader_takes_mixed_sizes(tmp_path):
    import main as driver
    opt, ds = _train_set(_write_mixed_dataset(tmp_path) + ["--batch_size", "2", "--num_workers", "0"])
    loader, _ = driver.make_train_loader(opt, ds, 2)
    np.random.seed(8)
    batches = list(loader)
    assert len(batches) == 2                                 # (shuffled: a batch may hold two frames of one size)
    assert sum(b["image_flat"].numel() for b in batches) == 2 * (96 * 160 * 3 + 80 * 200 * 3)
    for b in batches:
        assert b["image_offset"].tolist() == [0, int(b["image_hw"][0].prod()) * 3]


def test_sample_inputs_refusals_without_gpu():
    """The entry point validates on the host before any device work: callable with null device pointers."""
    L = _C.lib()
    assert L.cp_sample_inputs_workspace_bytes(3, 24, 300) == 3 * 6 * 2 * 8         # 4-row x 256-column workgroups
    assert L.cp_sample_inputs_workspace_bytes(1, 1, 1) == 8
    assert L.cp_sample_inputs_workspace_bytes(0, 24, 300) == 0
    off = np.zeros(2, np.int64)
    hw = np.array([[4, 5], [6, 7]], np.int32)
    trans = np.tile(np.array([1.0, 0, 0, 0, 1.0, 0]), (2, 1))
    color = np.zeros((2, 10), np.float64)
    m, s = np.zeros(3, np.float32), np.ones(3, np.float32)
    P = lambda a: ctypes.c_void_p(a.ctypes.data)

    def call(off=off, hw=hw, color=color, batch=2, dh=8, dw=8, host=True):
        h = (P(off), P(hw), P(trans), P(color), P(m), P(s)) if host else (None,) * 6
        return L.cp_sample_inputs_batch(None, *h, batch, dh, dw, None, None, 0, None)

    assert call(host=False) == -1
    assert call() == -1                                      # sound tables, null device pointers
    assert call(batch=0) == -1 and call(dh=0) == -1 and call(dw=-3) == -1
    assert call(hw=np.array([[4, 5], [0, 7]], np.int32)) == -1
    assert call(off=np.array([0, -1], np.int64)) == -1
    bad = color.copy()
    bad[1, :4] = (1, 0, 3, 1)
    assert call(color=bad) == -1
    # the existing warp's limits: sources up to 32767 a side, up to 65535 output rows
    assert call(hw=np.array([[4, 5], [32768, 7]], np.int32)) == -2
    assert call(hw=np.array([[4, 32768], [6, 7]], np.int32)) == -2
    assert call(dh=65536) == -2
    assert call(hw=np.array([[32767, 32767], [6, 7]], np.int32), dh=65535) == -1


def test_build_inputs_batch_refuses_host_tensors():
    from centerpoly_amd.datasets.sample.polydet import build_inputs_batch
    flat, hw, off = _flat(_sources())
    with pytest.raises(_C.NativeError):
        build_inputs_batch(flat, hw, off, TRANS, _color_rows(ORDERS[0], ORDERS[5]), MEAN, STD, DST_H, DST_W)


# ------------------------------------------------------------------------------------------------ GPU

def _per_image(images, trans, color, h, w, dev, mean=MEAN, std=STD):
    """The path the batch kernel restates: build_inputs on every image alone."""
    from centerpoly_amd.datasets.sample.polydet import build_inputs
    return [build_inputs(torch.from_numpy(im[None]).to(dev), trans[b: b + 1], color[b: b + 1], mean, std, h, w)[0]
            .cpu().numpy() for b, im in enumerate(images)]


@pytest.mark.gpu
@pytest.mark.parametrize("case", [0, 1, 2])
def test_batch_kernel_matches_per_image_path_and_oracle(case):
    from centerpoly_amd.datasets.sample.polydet import build_inputs_batch
    from oracle import pre as opre
    dev = torch.device("cuda")
    images = _sources()
    color = _color_rows(ORDERS[case], ORDERS[5 - case])
    flat, hw, off = _flat(images, dev)
    out = build_inputs_batch(flat, hw, off, TRANS, color, MEAN, STD, DST_H, DST_W)
    assert out.dtype == torch.float32 and tuple(out.shape) == (3, 3, DST_H, DST_W)
    again = build_inputs_batch(flat, hw, off, TRANS, color, MEAN, STD, DST_H, DST_W)
    assert torch.equal(out, again)                           # no atomics: a second call returns the same bits
    out = out.cpu().numpy()
    single = _per_image(images, TRANS, color, DST_H, DST_W, dev)
    assert np.array_equal(out[1], single[1])                 # colour off: operation for operation, bit for bit
    warps = _oracle_warps()
    assert any((w == 0).all(axis=2).any() for w in warps) and all(w.any() for w in warps)    # border and content
    for b in range(3):
        ref = opre.color_aug_normalize(warps[b], color[b, 1:4].astype(int), color[b, 4:7], color[b, 7:10], MEAN, STD,
                                       color_on=bool(color[b, 0]))
        np.testing.assert_allclose(out[b], ref, rtol=1e-6, atol=1e-5)
        np.testing.assert_allclose(out[b], single[b], rtol=1e-6, atol=1e-5)       # (the grey mean's summation order is free)


@pytest.mark.gpu
def test_seventeen_images_cross_the_chunk_boundary():
    """B = 17 (one more than a launch carries): every image equals its own B = 1 result bit for bit, the 1x1 source
    and the lone image of the second chunk included."""
    from centerpoly_amd.datasets.sample.polydet import build_inputs_batch
    dev = torch.device("cuda")
    sizes = [SIZES[i % 3] for i in range(17)]
    sizes[5] = (1, 1)
    images = _sources(tuple(sizes), seed=33)
    rng = np.random.RandomState(34)
    trans = TRANS[np.arange(17) % 3].copy()
    trans[:, 2] += rng.uniform(-8, 8, 17)                    # no two images share a window
    trans[:, 5] += rng.uniform(-3, 3, 17)
    trans[5] = (40.0, 0, 100.0, 0, 9.0, 7.0)                 # the single pixel spread over a patch
    color = np.zeros((17, 10), np.float64)
    for b in range(17):
        if b % 4 != 1:                                       # images 1, 5, 9, 13 only normalise
            color[b] = [1, *ORDERS[b % 6], *rng.uniform(0.6, 1.4, 3), *rng.uniform(-0.03, 0.03, 3)]
    assert color[16, 0] == 1 and color[5, 0] == 0 and color[0, 0] == 1
    flat, hw, off = _flat(images, dev)
    out = build_inputs_batch(flat, hw, off, trans, color, MEAN, STD, DST_H, DST_W).cpu().numpy()
    assert out.shape == (17, 3, DST_H, DST_W) and np.isfinite(out).all()
    for b in range(17):
        f1, hw1, off1 = _flat(images[b: b + 1], dev)
        one = build_inputs_batch(f1, hw1, off1, trans[b: b + 1], color[b: b + 1], MEAN, STD, DST_H, DST_W)
        assert np.array_equal(out[b], one[0].cpu().numpy()), b
    # an image placed away from the start of the buffer, addressed by its offset alone
    pad = torch.cat([torch.zeros(1001, dtype=torch.uint8, device=dev), flat])
    shifted = build_inputs_batch(pad, hw, off + 1001, trans, color, MEAN, STD, DST_H, DST_W).cpu().numpy()
    assert np.array_equal(shifted, out)
    with pytest.raises(ValueError):
        build_inputs_batch(flat, hw, off + 1, trans, color, MEAN, STD, DST_H, DST_W)       # the last image overruns


@pytest.mark.gpu
def test_equal_sizes_match_build_inputs():
    """The [2,96,160,3] case of test_device_color_aug_and_training_input_pipeline through both paths."""
    from centerpoly_amd.datasets.sample.polydet import build_inputs, build_inputs_batch
    from centerpoly_amd.utils.image import get_affine_transform
    rng = np.random.RandomState(9)
    img = rng.randint(0, 255, (2, 96, 160, 3), dtype=np.uint8)
    trans = np.stack([get_affine_transform(np.array([80., 48.], np.float32), 160.0 * s, 0, [128, 64]).reshape(6)
                      for s in (0.8, 1.2)])
    color = np.array([[1, 2, 0, 1, 0.7, 1.3, 0.9, 0.01, -0.02, 0.005], [0, 0, 0, 0, 1, 1, 1, 0, 0, 0]], np.float64)
    dev = torch.device("cuda")
    ref = build_inputs(torch.from_numpy(img).to(dev), trans, color, MEAN, STD, 64, 128).cpu().numpy()
    flat, hw, off = _flat(list(img), dev)
    out = build_inputs_batch(flat, hw, off, trans, color, MEAN, STD, 64, 128).cpu().numpy()
    np.testing.assert_allclose(out, ref, rtol=1e-6, atol=1e-5)
    assert np.array_equal(out[1], ref[1])
    off_color = np.zeros_like(color)
    ref0 = build_inputs(torch.from_numpy(img).to(dev), trans, off_color, MEAN, STD, 64, 128).cpu().numpy()
    out0 = build_inputs_batch(flat, hw, off, trans, off_color, MEAN, STD, 64, 128).cpu().numpy()
    assert np.array_equal(out0, ref0)


@pytest.mark.gpu
def test_trainer_on_a_mixed_size_dataset(tmp_path):
    """The mixed-size data set through collate_ragged -> prepare_batch (inputs and targets against the per-image
    builders) -> one epoch of two steps."""
    import contextlib
    import io
    from centerpoly_amd.datasets.sample.polydet import _FIELDS, build_targets, collate_ragged
    from centerpoly_amd.models.model import create_model
    from centerpoly_amd.trains.train_factory import train_factory
    args = _write_mixed_dataset(tmp_path) + ["--arch", "dla_34", "--batch_size", "2", "--num_iters", "2"]
    opt, ds = _train_set(args)
    dev = opt.device = torch.device("cuda")
    torch.manual_seed(11)
    with contextlib.redirect_stdout(io.StringIO()):
        model = create_model(opt.arch, opt.heads, opt.head_conv)
    trainer = train_factory["polydet"](opt, model, torch.optim.Adam(model.parameters(), opt.lr))
    trainer.set_device(opt.gpus, opt.chunk_sizes, dev)
    loader = torch.utils.data.DataLoader(ds, batch_size=2, shuffle=False, num_workers=0, collate_fn=collate_ragged)
    np.random.seed(6)
    host = next(iter(loader))
    assert sorted(host["image_hw"].tolist()) == [[80, 200], [96, 160]] and host["color"][:, 0].tolist() == [1, 1]
    for colour_on in (True, False):
        raw = {k: v.clone() for k, v in host.items()}
        if not colour_on:
            raw["color"][:, 0] = 0
        batch = trainer.prepare_batch({k: v.to(dev) for k, v in raw.items()})
        assert tuple(batch["input"].shape) == (2, 3, 64, 128)
        off, hw = raw["image_offset"].tolist(), raw["image_hw"].tolist()
        images = [raw["image_flat"][off[b]: off[b] + hw[b][0] * hw[b][1] * 3].numpy().reshape(hw[b][0], hw[b][1], 3)
                  for b in range(2)]
        single = _per_image(images, raw["trans_input"].numpy(), raw["color"].numpy(), 64, 128, dev, opt.mean, opt.std)
        got = batch["input"].cpu().numpy()
        for b in range(2):
            if colour_on:
                np.testing.assert_allclose(got[b], single[b], rtol=1e-6, atol=1e-5)
            else:
                assert np.array_equal(got[b], single[b])
        targets = build_targets({k: raw[k].to(dev) for k in _FIELDS}, 16, 32, opt.num_classes, rep=opt.rep,
                                with_border_hm=False)
        assert set(targets) <= set(batch) and float(targets["hm"].max()) == 1.0
        for k, v in targets.items():
            assert torch.equal(batch[k], v), k
    stats, _ = trainer.train(1, loader)
    assert all(np.isfinite(stats[k]) for k in ("loss", "hm_l", "poly_l", "depth_l", "off_l")) and stats["hm_l"] > 0
    bad = {k: v.to(dev) for k, v in host.items()}
    bad["input_hw"] = torch.tensor([[64, 128], [96, 128]], dtype=torch.int32, device=dev)
    with pytest.raises(ValueError, match=r"--keep_res.*batch"):
        trainer.prepare_batch(bad)

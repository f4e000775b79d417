"""Instance maps through the Python layer (detectors/instances.py), the detector method and the drivers.

Real drawings: synthetic rows on a 160 x 96 canvas through instance_maps once per family (Cityscapes, KITTI, IDD),
against the restatement of cp_instance_map (tests/golden/instance_map_host.py) applied, WITHOUT bounds, to the masks
the host statements of the writers draw (oracle/writer.py; PIL's fill and outline as tests/golden/pil_scanline_host.py
restates them) -- so also the check that the bounds of instance_maps never cut a drawn pixel.  Interface: instances()
after run() and run_batch(); demo.py and test.py with --save_ids / --save_masks write the named files, and what is read
back equals the API's tensors and table."""
import contextlib
import importlib.util
import io
import json
import os
import types

import numpy as np
import pytest

import instance_map_host as host
from oracle import writer as ow
from pil_scanline_host import fill as pil_fill, outline as pil_outline

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, N = 160, 96, 16
THRESH = 0.25                                                # a float32 number: `score == thresh` is exact
f32 = np.float32


# --------------------------------------------------------------------------------------------- real drawings --
def _rows(C):
    """24 seeded rows x1,y1,x2,y2,score,cls,poly,depth: polygons around centres inside and outside the canvas; rows 0
    and 1 confident occluders of one class over the middle, row 2 a large unconfident polygon nearest of all (what it
    covers stays in the farther masks: overlap), every fifth row a polygon of a few pixels (under the Cityscapes
    writer's 100-pixel rule), row 3 a score equal to the threshold, rows 6 and 7 below it, rows 10 and 2 at one depth."""
    rng = np.random.RandomState(5)
    R = 24
    rows = np.zeros((R, 2 * N + 7), f32)
    for r in range(R):
        cx, cy = rng.uniform(-10, W + 10), rng.uniform(-10, H + 10)
        rad = rng.uniform(1.5, 3) if r % 5 == 4 else rng.uniform(12, 45)
        if r < 3:
            cx, cy, rad = W / 2 + 12 * r, H / 2 - 6 * r, 36 - 4 * r
        ang = np.sort(rng.uniform(0, 2 * np.pi, N))
        rr = rad * rng.uniform(0.6, 1.0, N)
        pts = np.stack([cx + rr * np.cos(ang), cy + rr * np.sin(ang)], 1)
        rows[r, 6:6 + 2 * N] = pts.reshape(-1)
        rows[r, 0:4] = [pts[:, 0].min(), pts[:, 1].min(), pts[:, 0].max(), pts[:, 1].max()]
        rows[r, 4] = rng.uniform(0.3, 0.95)
        rows[r, 5] = rng.randint(0, C)
        rows[r, -1] = rng.uniform(1, 50)
    rows[0, 4], rows[1, 4], rows[2, 4] = 0.9, 0.6, 0.3
    rows[0, 5] = rows[1, 5] = 2
    rows[2, 5] = 0
    rows[2, -1] = 0.5
    rows[10, -1] = rows[2, -1]
    rows[3, 4] = THRESH
    rows[6, 4], rows[7, 4] = 0.2, np.nextafter(f32(THRESH), f32(0))
    return rows


def _per_class(rows, C):
    return {c + 1: np.delete(rows[rows[:, 5] == c], 5, axis=1) for c in range(C)}


def _selected(rows, C, at_threshold, by_depth_only):
    """Source rows in slot order: class by class the rows that pass, sorted (stable) by depth over all classes
    (Cityscapes) or within the class (KITTI / IDD)."""
    out = []
    for c in range(C):
        mine = [r for r in range(len(rows)) if rows[r, 5] == c
                and (rows[r, 4] >= f32(THRESH) if at_threshold else rows[r, 4] > f32(THRESH))]
        out += mine if by_depth_only else sorted(mine, key=lambda r: rows[r, -1])
    return sorted(out, key=lambda r: rows[r, -1]) if by_depth_only else out


def _dataset(name):
    from centerpoly_amd.datasets.dataset_factory import dataset_factory
    cls = dataset_factory[name]
    ds = cls.__new__(cls)
    ds.opt = types.SimpleNamespace(thresh=THRESH)
    return ds


def _compare(maps, rows, src, masks, want, labels, counts, live):
    import torch
    torch.cuda.synchronize()
    n, t = len(src), maps.table
    index, ids, lab, value, visible, box = want
    assert n >= 8 and t["n"] == n and t["src"].tolist() == src
    got_masks = maps.masks.cpu().numpy()
    assert got_masks.shape[1:] == (H, W) and np.array_equal(got_masks[:n], masks) and not got_masks[n:].any()
    assert np.array_equal(maps.index.cpu().numpy(), index)
    assert np.array_equal(maps.ids.cpu().numpy(), ids) and np.array_equal(maps.labels.cpu().numpy(), lab)
    assert t["label"].tolist() == labels and t["count"].tolist() == counts and t["live"].tolist() == live
    assert np.array_equal(t["value"], value) and np.array_equal(t["visible"], visible) and np.array_equal(t["box"], box)
    assert t["score"].view(np.uint32).tolist() == rows[src, 4].view(np.uint32).tolist()
    assert t["poly"].reshape(n, -1).tolist() == [[int(float("%.2f" % v)) for v in rows[r, 6:6 + 2 * N]] for r in src]
    # it shows something: two live instances overlap, one is hidden at least in part, vertices leave the canvas
    stack = np.stack([masks[k] != 0 for k in range(n) if live[k]])
    assert stack.sum(0).max() >= 2 and (visible[np.array(live)] < stack.sum((1, 2))).any()
    assert (t["poly"] < 0).any() and (t["poly"][:, :, 0] >= W).any()


@pytest.mark.gpu
def test_cityscapes_family_against_the_host_writer():
    import torch
    from centerpoly_amd.detectors.instances import instance_maps
    ds = _dataset("cityscapes")
    C = len(ds.class_name) - 1                                             # 11: pole, traffic sign and light too
    rows = _rows(C)
    params = ow.image_instances(_per_class(rows, C), ds.class_name, THRESH)
    src = _selected(rows, C, False, True)
    assert [p[1] for p in params] == rows[src, 4].tolist() and 3 not in src and 6 not in src and 7 not in src
    drawn = ow.instance_masks(params, W, H)
    masks = np.stack([m for m, _ in drawn])
    labels = [int(ds.label_to_id[p[2]]) for p in params]
    flags = np.array([0 if p[2] in ow.NO_MASK_LABELS else 1 for p in params], np.uint8)
    counts = [int(np.count_nonzero(m)) for m in masks]
    live = [bool(keep) for _, keep in drawn]
    assert (flags == 0).any() and any(f and 0 < c <= 100 for f, c in zip(flags, counts))   # both ways to be dead
    assert any(p[1] >= 0.5 for p in params)
    want = host.instance_map(masks, flags, 1, np.array(counts), 100, np.array(labels), None, None, 1000, 0)
    maps = instance_maps(torch.from_numpy(rows).cuda(), ds, (W, H))
    assert maps.family == "cityscapes" and maps.multiplier == 1000 and maps.canvas == (W, H)
    _compare(maps, rows, src, masks, want, labels, counts, live)
    assert maps.written() == [k for k in range(len(src)) if live[k]]
    k = maps.written()[0]
    assert maps.conf_text(k) == str(min(1, rows[src[k], 4] * f32(1.2)))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["kitti_poly", "IDD"])
def test_class_family_against_the_host_writer(name):
    import torch
    from centerpoly_amd.detectors.instances import instance_maps
    ds = _dataset(name)
    C = len(ds.class_name) - 1
    rows = _rows(C)
    params = ds.image_instances(_per_class(rows, C))                       # drawing order: class, depth, row
    src = _selected(rows, C, ds.at_threshold, False)
    assert [p[1] for p in params] == rows[src, 4].tolist() and (3 in src) == (name == "IDD") and 7 not in src
    masks, removed = [], {}
    for pts, score, cls, _depth, _count in params:                         # F \ O, less the fills of nearer confident
        F, O = pil_fill(pts, W, H), pil_outline(pts, W, H)                 # instances of the class
        rem = removed.setdefault(cls, np.zeros((H, W), bool))
        masks.append(((F & ~O & ~rem) * 255).astype(np.uint8))
        if score >= f32(0.5):
            rem |= F
    masks = np.stack(masks)
    labels = [int(ds.label_to_id[ds.class_name[p[2] + 1]]) for p in params]
    multiplier = 256 if name == "kitti_poly" else 1000
    want = host.instance_map(masks, np.ones(len(src), np.uint8), 1, None, 0, np.array(labels), rows[src, -1], None,
                             multiplier, 0)
    maps = instance_maps(torch.from_numpy(rows).cuda(), type(ds), (W, H), thresh=THRESH)     # the class alone
    assert maps.family == "class" and maps.multiplier == multiplier
    _compare(maps, rows, src, masks, want, labels, [int(np.count_nonzero(m)) for m in masks], [True] * len(src))
    assert maps.table["text_index"].tolist() == [p[4] for p in params]
    assert [int(maps.table["text_index"][k]) for k in maps.written()] == list(range(len(src)))
    # the nearer instance wins across classes: somewhere a later slot owns a pixel an earlier slot's mask covers
    index = want[0]
    assert any(((masks[i] != 0) & (index > i) & (index != 255)).any() for i in range(len(src)))
    with pytest.raises(ValueError, match="thresh"):
        instance_maps(torch.from_numpy(rows).cuda(), type(ds), (W, H))


@pytest.mark.gpu
def test_more_than_128_live_rows_are_refused_like_the_scoring_path():
    import torch
    from centerpoly_amd.detectors.instances import instance_maps
    rows = np.tile(_rows(8)[:1], (130, 1))
    with pytest.raises(ValueError, match="more than 128 instances in one image"):
        instance_maps(torch.from_numpy(rows).cuda(), _dataset("kitti_poly"), (W, H))
    with pytest.raises(TypeError, match="no result writer"):
        from centerpoly_amd.datasets.dataset_factory import dataset_factory
        instance_maps(torch.from_numpy(rows).cuda(), dataset_factory["synthetic"], (W, H), thresh=0.1)


# ------------------------------------------------------------------------------------------------- interface --
SIZES = ((37, 53), (64, 96))                                 # (height, width) of the two images


def _image(h, w, seed):
    return np.random.RandomState(seed).randint(0, 256, (h, w, 3)).astype(np.uint8)


def _checkpoint(tmp):
    """A seeded, randomly initialised DLA-34 whose `poly` bias is a 16-gon of 6 to 10 output pixels radius and whose
    `hm` bias is -1 (a random `poly` head gives polygons of a pixel or two: empty masks would show nothing)."""
    import torch
    from centerpoly_amd.models.model import create_model, save_model
    rng = np.random.RandomState(11)
    torch.manual_seed(23)
    model = create_model("dla_34", {"hm": 8, "poly": 32, "pseudo_depth": 1, "reg": 2}, 256)
    with torch.no_grad():
        ang = np.arange(16) * (2 * np.pi / 16)
        rad = rng.uniform(6, 10, 16)
        bias = np.stack([rad * np.cos(ang), rad * np.sin(ang)], 1).reshape(-1)
        model.state_dict()["poly.2.bias"].copy_(torch.from_numpy(bias.astype(np.float32)))
        model.state_dict()["hm.2.bias"].fill_(-1.0)
    path = os.path.join(str(tmp), "model_seeded.pth")
    save_model(path, 1, model)
    return path


def _args(tmp, dataset, extra=()):
    return ["polydet", "--arch", "dla_34", "--dataset", dataset, "--load_model", _checkpoint(tmp), "--input_h", "64",
            "--input_w", "96", "--K", "32", "--thresh", "0.05", "--root_dir", os.path.join(str(tmp), "exp_root")] \
        + list(extra)


def _same_maps(a, b):
    assert a.family == b.family and a.canvas == b.canvas and sorted(a.table) == sorted(b.table)
    for name in ("index", "ids", "labels", "masks"):
        x, y = getattr(a, name), getattr(b, name)
        assert x.is_cuda and x.dtype == y.dtype and x.shape == y.shape and bool((x == y).all()), name
    for key in a.table:
        assert np.array_equal(np.asarray(a.table[key]), np.asarray(b.table[key])), key


@pytest.mark.gpu
@pytest.mark.parametrize("extra", [(), ("--test_scales", "1,0.5")], ids=["plain", "scales"])
def test_detector_instances_after_run_and_run_batch(tmp_path, extra):
    import torch
    from centerpoly_amd.datasets.dataset_factory import dataset_factory
    from centerpoly_amd.detectors.detector_factory import detector_factory
    from centerpoly_amd.detectors.instances import instance_maps
    from centerpoly_amd.opts import opts
    with contextlib.redirect_stdout(io.StringIO()):
        opt = opts().parse(_args(tmp_path, "kitti_poly", extra))
        opt = opts().update_dataset_info_and_set_heads(opt, dataset_factory[opt.dataset])
        det = detector_factory["polydet"](opt)
    images = [_image(h, w, 70 + k) for k, (h, w) in enumerate(SIZES)]
    ret = det.run(images[1])
    assert sorted(ret) == ["dec", "load", "merge", "net", "post", "pre", "results", "tot"]     # nothing added
    maps = det.instances(ret["results"])
    assert maps.canvas == (96, 64) and tuple(maps.index.shape) == (64, 96)
    _same_maps(maps, instance_maps(det.device_rows(ret["results"]), dataset_factory["kitti_poly"], (96, 64), 0.05))
    assert maps.table["n"] >= 2 and (maps.table["visible"] > 0).sum() >= 2
    assert int((maps.index != 255).sum()) == int(maps.table["visible"].sum()) > 0
    with pytest.raises(IndexError):
        det.instances(image=1)
    big = det.instances(canvas=(200, 120), thresh=0.2)                    # another canvas, another threshold
    assert tuple(big.ids.shape) == (120, 200) and big.table["n"] <= maps.table["n"]
    ret = det.run_batch(images)
    assert sorted(ret) == ["dec", "load", "merge", "n", "net", "post", "pre", "results", "tot"]
    for b, (h, w) in enumerate(SIZES):
        maps = det.instances(image=b)
        assert maps.canvas == (w, h) and tuple(maps.masks.shape[1:]) == (h, w)
        _same_maps(maps, instance_maps(det.device_rows(image=b), dataset_factory["kitti_poly"], (w, h), 0.05))
        _same_maps(maps, det.instances(ret["results"][b], image=b))
        assert maps.table["n"] >= 2 and int((maps.index != 255).sum()) == int(maps.table["visible"].sum()) > 0
    torch.cuda.synchronize()


def _module(name):
    spec = importlib.util.spec_from_file_location("centerpoly_%s_driver" % name, os.path.join(ROOT, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _record_instances(monkeypatch):
    from centerpoly_amd.detectors.polydet import PolydetDetector
    seen, inner = [], PolydetDetector.instances

    def recording(self, *a, **k):
        seen.append(inner(self, *a, **k))
        return seen[-1]

    monkeypatch.setattr(PolydetDetector, "instances", recording)
    return seen


def _check_files(inst_dir, stem, maps, ids=True, masks=True):
    """The files of one image read back against the API's tensors and table."""
    from PIL import Image
    from centerpoly_amd.datasets.evaluation import instance_level as il
    t = maps.table
    live = [k for k in range(t["n"]) if t["live"][k]]
    if ids:
        assert np.array_equal(il.read_gt_ids(os.path.join(inst_dir, stem + "_instanceIds.png")), maps.ids.cpu().numpy())
        lab = Image.open(os.path.join(inst_dir, stem + "_labelIds.png"))
        assert lab.mode == "L" and np.array_equal(np.array(lab), maps.labels.cpu().numpy())
        js = json.load(open(os.path.join(inst_dir, stem + ".json")))
        assert (js["width"], js["height"]) == maps.canvas and js["multiplier"] == maps.multiplier
        assert [e["value"] for e in js["instances"]] == t["value"][live].tolist()
        assert [e["visible"] for e in js["instances"]] == t["visible"][live].tolist()
        assert [e["box"] for e in js["instances"]] == t["box"][live].tolist()
        assert [e["source_row"] for e in js["instances"]] == t["src"][live].tolist()
        assert [e["label_id"] for e in js["instances"]] == t["label"][live].tolist()
        assert [e["class_name"] for e in js["instances"]] == [maps.names[int(v)] for v in t["label"][live]]
        assert [f32(e["score"]) for e in js["instances"]] == t["score"][live].tolist()
        assert [f32(e["confidence"]) for e in js["instances"]] == t["conf"][live].tolist()
        assert [e["polygon"] for e in js["instances"]] == t["poly"][live].tolist()
    if masks:
        lines = open(os.path.join(inst_dir, stem + ".txt")).read().splitlines()
        slots = maps.written()
        assert sorted(slots) == live and len(lines) == len(live) > 0
        drawn = maps.masks.cpu().numpy()
        for count, (k, line) in enumerate(zip(slots, lines)):
            assert line == "masks/%s_%d.png %d %s" % (stem, count, t["label"][k], maps.conf_text(k))
            assert np.array_equal(np.array(Image.open(os.path.join(inst_dir, line.split(" ")[0]))), drawn[k])
    return live


@pytest.mark.gpu
def test_demo_writes_ids_and_masks(tmp_path, monkeypatch):
    from PIL import Image
    from centerpoly_amd.opts import opts
    os.makedirs(str(tmp_path / "imgs"))
    for k, (stem, (h, w)) in enumerate(zip(["frame_b", "frame_a"], SIZES)):
        Image.fromarray(_image(h, w, 80 + k)[:, :, ::-1]).save(str(tmp_path / "imgs" / (stem + ".png")))
    seen = _record_instances(monkeypatch)
    with contextlib.redirect_stdout(io.StringIO()):
        opt = opts().parse(_args(tmp_path, "kitti_poly", ["--demo", str(tmp_path / "imgs"), "--save_ids", "--save_masks"]))
        out = _module("demo").demo(opt)
    assert [os.path.basename(n) for n, _ in out] == ["frame_a.png", "frame_b.png"] and len(seen) == 2
    inst_dir = os.path.join(opt.save_dir, "instances")
    for stem, maps, (h, w) in zip(["frame_a", "frame_b"], seen, SIZES[::-1]):
        assert maps.canvas == (w, h) and maps.family == "class" and maps.multiplier == 256
        assert len(_check_files(inst_dir, stem, maps)) >= 2
    names = sorted(os.listdir(inst_dir))
    assert [n for n in names if n != "masks"] == sorted(s + e for s in ("frame_a", "frame_b")
                                                        for e in ("_instanceIds.png", "_labelIds.png", ".json", ".txt"))
    assert len(os.listdir(os.path.join(inst_dir, "masks"))) == sum(int(m.table["live"].sum()) for m in seen)


@pytest.mark.gpu
@pytest.mark.parametrize("batch", [1, 2])
def test_driver_writes_ids_of_a_tiny_cityscapes_set(tmp_path, monkeypatch, batch):
    """test.py --save_ids --save_masks on two small images (the new path draws on the image's own canvas, not on the
    writer's 2048 x 1024), per image and with --test_batch_size 2; the mask directory is one evaluate_result_dir reads."""
    import shutil

    from PIL import Image
    from centerpoly_amd.datasets.evaluation import instance_level as il
    from centerpoly_amd.opts import opts
    img_dir, annot_dir = str(tmp_path / "images"), str(tmp_path / "BBoxes")
    os.makedirs(img_dir)
    os.makedirs(annot_dir)
    stems = ["frankfurt_a_leftImg8bit", "frankfurt_b_leftImg8bit"]
    for k, (stem, (h, w)) in enumerate(zip(stems, SIZES)):
        Image.fromarray(_image(h, w, 90 + k)[:, :, ::-1]).save(os.path.join(img_dir, stem + ".png"))
    with open(os.path.join(annot_dir, "val16_regular_interval.json"), "w") as f:
        json.dump({"images": [{"id": 10 + k, "file_name": s + ".png", "height": h, "width": w}
                              for k, (s, (h, w)) in enumerate(zip(stems, SIZES))], "annotations": [], "categories": []}, f)
    seen = _record_instances(monkeypatch)
    with contextlib.redirect_stdout(io.StringIO()):
        opt = opts().parse(_args(tmp_path, "cityscapes", ["--annot_dir", annot_dir, "--img_dir", img_dir, "--save_ids",
                                                          "--save_masks", "--not_prefetch_test", "--test_batch_size",
                                                          str(batch)]))
        out = _module("test").run_test(opt, evaluate=False)
    assert list(out["results"]) == [10, 11] and len(seen) == 2
    inst_dir = os.path.join(opt.save_dir, "instances")
    for stem, maps, (h, w) in zip(stems, seen, SIZES):
        assert maps.canvas == (w, h) and maps.family == "cityscapes"
        assert len(_check_files(inst_dir, stem, maps)) >= 2
    # the written id image as ground truth: the result directory is in the layout the evaluator reads
    gt = str(tmp_path / "frankfurt_b_gtFine_instanceIds.png")
    shutil.copy(os.path.join(inst_dir, stems[1] + "_instanceIds.png"), gt)
    res = il.evaluate_result_dir(inst_dir, [gt])
    assert 0.0 <= res["allAp"] <= 1.0

"""cp_writer_instances (the writer's selection on the device), the device-resident scoring path built on it
(CityscapesWriterMixin.score_instances_device) and test.py on a data set.

References: the recorded writer fixtures (tests/golden/writer_*.npz: order, text lines), oracle.writer.image_instances,
the host method CITYSCAPES.image_instances (unchanged, an independent implementation of the same selection), the
reference evaluator's recorded counts and AP (tests/golden/instance_ap_*.npz) and CITYSCAPES.run_eval on the host
dict.  Selections, orders, vertices, labels, flags and counts are integers and the confidence is one float32
product: every comparison of them is exact.  AP against the recording is compared with atol 1e-12, the tolerance
test_instance_ap.py uses for the same quantity; AP of the driver against run_eval on the same run is compared bit
for bit."""
import ctypes
import importlib.util
import json
import os
import types

import numpy as np
import pytest

from centerpoly_amd import _C
from centerpoly_amd.datasets.evaluation import instance_level as il
from oracle import writer as ow

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CASES = ["star16", "mixed32", "selfcross16", "small16"]
CLASS_NAME = ["__background__", "person", "rider", "car", "truck", "bus", "train", "motorcycle", "bicycle", "pole",
              "traffic sign", "traffic light"]
LABEL_TO_ID = {"person": 24, "rider": 25, "car": 26, "truck": 27, "bus": 28, "train": 31, "motorcycle": 32,
               "bicycle": 33, "pole": -1, "traffic sign": -1, "traffic light": -1}
NO_MASKS = ("pole", "traffic sign", "traffic light")
TABLE = np.array([[LABEL_TO_ID[c], 0 if c in NO_MASKS else 1] for c in CLASS_NAME[1:]], np.int32)
THRESH = 0.05


def _writer(name):
    z = np.load(os.path.join(HERE, "golden", "writer_%s.npz" % name), allow_pickle=False)
    det = {c: z["det_%d" % c] for c in sorted(int(k[4:]) for k in z.files if k.startswith("det_"))}
    return det, [str(v) for v in z["lines"]], z["order_depth"]


def _rec(name):
    return np.load(os.path.join(HERE, "golden", "instance_ap_%s.npz" % name), allow_pickle=False)


def _stack(det):
    """{class index (from 1): rows x1,y1,x2,y2,score,poly,depth} -> float32 [R, 2N + 7] with the class column
    (from 0), classes ascending: the layout cp_polydet_post_process writes."""
    rows = [np.concatenate([r[:, :5], np.full((len(r), 1), c - 1, np.float32), r[:, 5:]], axis=1)
            for c, r in sorted(det.items())]
    return np.ascontiguousarray(np.concatenate(rows, axis=0), np.float32)


def _split(rows, C):
    """The inverse, as polydet_post_process_device splits the rows it copied back."""
    keep = np.concatenate([rows[:, :5], rows[:, 6:]], axis=1)
    return {j + 1: keep[rows[:, 5] == j] for j in range(C)}


def _kernel(rows, thresh=THRESH, table=TABLE):
    """cp_writer_instances on host rows: (n, src, poly, flags, label, conf) as host arrays of all R slots."""
    import torch
    R, N = rows.shape[0], (rows.shape[1] - 7) // 2
    dev = torch.device("cuda")
    d_rows = torch.from_numpy(rows).to(dev)
    n = torch.full((1,), -7, dtype=torch.int32, device=dev)
    src = torch.full((R,), -7, dtype=torch.int32, device=dev)
    poly = torch.full((R, N, 2), -7, dtype=torch.int32, device=dev)
    flags = torch.full((R,), 77, dtype=torch.uint8, device=dev)
    label = torch.full((R,), -7, dtype=torch.int32, device=dev)
    conf = torch.full((R,), -7.0, dtype=torch.float32, device=dev)
    table = np.ascontiguousarray(table, np.int32)
    _C.check(_C.lib().cp_writer_instances(_C.ptr(d_rows), R, N, thresh, table.ctypes.data_as(ctypes.c_void_p),
                                          len(table), _C.ptr(n), _C.ptr(src), _C.ptr(poly), _C.ptr(flags),
                                          _C.ptr(label), _C.ptr(conf), _C.stream()), "cp_writer_instances")
    return (int(n.cpu()[0]), src.cpu().numpy(), poly.cpu().numpy(), flags.cpu().numpy(), label.cpu().numpy(),
            conf.cpu().numpy())


def _dataset(thresh=THRESH):
    from centerpoly_amd.datasets.dataset.polygons import CITYSCAPES
    ds = CITYSCAPES.__new__(CITYSCAPES)
    ds.opt = types.SimpleNamespace(thresh=thresh)
    return ds


def _assert_dead(n, src, poly, flags, label, conf):
    assert (flags[n:] == 0).all() and (src[n:] == -1).all() and (label[n:] == -1).all()
    assert (conf[n:] == 0).all() and (poly[n:] == 0).all()


def _assert_equals_host_list(rows, params, got):
    """The kernel's output against a host instance list [(points, score, class name, depth)] of the same rows."""
    n, src, poly, flags, label, conf = got
    assert n == len(params)
    _assert_dead(*got)
    live = np.flatnonzero(rows[:, 4] > np.float32(THRESH))
    assert sorted(src[:n].tolist()) == live.tolist()                      # every live row once, nothing else
    # ascending depth, then class, then row -- spelled out on the rows themselves
    want = live[np.lexsort((live, rows[live, 5], rows[live, -1]))]
    assert src[:n].tolist() == want.tolist()
    for k, (pts, score, name, depth) in enumerate(params):
        r = rows[src[k]]
        assert np.float32(score).tobytes() == r[4].tobytes() and np.float32(depth).tobytes() == r[-1].tobytes()
        assert name == CLASS_NAME[int(r[5]) + 1] and label[k] == LABEL_TO_ID[name]
        assert poly[k].tolist() == [list(p) for p in pts], "instance %d (row %d)" % (k, src[k])
        assert flags[k] == (0 if name in NO_MASKS else 1) | (2 if score >= 0.5 else 0)
        host_conf = min(1, score * 1.2)                                   # the writer's expression, on np.float32
        assert np.float32(host_conf).tobytes() == conf[k].tobytes() and str(host_conf) == str(min(1, conf[k]))


# ------------------------------------------------------------------------------------------------ refusals --
def _refusals():
    L = _C.lib()
    p = ctypes.c_void_p(256)                                # never dereferenced: every call below returns first
    tab = TABLE.ctypes.data_as(ctypes.c_void_p)
    call = lambda R, N, C, rows=p, t=tab, n=p, src=p, poly=p, fl=p, lab=p, conf=p, th=THRESH: \
        L.cp_writer_instances(rows, R, N, th, t, C, n, src, poly, fl, lab, conf, None)      # noqa: E731
    assert call(1025, 16, 11) == -2 and call(128, 65, 11) == -2 and call(128, 16, 33) == -2
    assert call(0, 16, 11) == -1 and call(-1, 16, 11) == -1
    assert call(128, 2, 11) == -1 and call(128, 0, 11) == -1             # cp_instance_masks needs a triangle
    assert call(128, 16, 0) == -1 and call(128, 16, -3) == -1            # a short class table
    assert call(128, 16, 11, t=None) == -1
    for name in ("rows", "n", "src", "poly", "fl", "lab", "conf"):
        assert call(128, 16, 11, **{name: None}) == -1, name
    assert call(128, 16, 11, th=float("nan")) == -1
    return 18


def test_refusals_come_before_any_device_work():
    assert _refusals() == 18


@pytest.mark.gpu
def test_refusals_on_the_gpu_box():
    assert _refusals() == 18


# ------------------------------------------------------------------- 1. kernel against the recorded writer --
@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_kernel_against_the_recorded_writer(name):
    import torch
    det, lines, order = _writer(name)
    rows = _stack(det)
    got = _kernel(rows)
    n, src = got[0], got[1]
    assert n == len(order)
    assert np.array_equal(rows[src[:n], -1].astype(np.float64), order)
    _assert_equals_host_list(rows, ow.image_instances(det, CLASS_NAME, THRESH), got)
    # through cp_instance_masks and the host's selection on the count rows: the recorded text, line for line
    ds = _dataset()
    res = ds.score_instances_device(torch.from_numpy(rows).cuda(), _rec(name)["gt_ids"])
    assert res["n"] == n and np.array_equal(res["src"], src[:n])
    base = "frankfurt_%s_leftImg8bit.png" % name
    text = ["masks/" + base.replace(".png", "_%d.png" % count) + " " + str(int(res["labels"][k])) + " " + conf + "\n"
            for count, (k, conf) in enumerate(zip(res["kept"], res["conf_text"]))]
    assert text == lines
    assert all(res["counts"][k] > 100 for k in res["kept"])


# ------------------------------------------------------------------ 2. kernel against image_instances --
def _seeded_rows(R, N, kind, seed):
    """float32 [R, 2N + 7].  `mixed`: every special value of the selection; `zero`: nothing above the threshold;
    `live128` / `live129`: exactly that many rows above it."""
    rng = np.random.RandomState(seed)
    f32 = np.float32
    th = f32(THRESH)
    rows = np.zeros((R, 2 * N + 7), f32)
    rows[:, 0:4] = rng.uniform(0, 2048, (R, 4)).astype(f32)
    rows[:, 5] = rng.randint(0, 11, R)
    rows[:, 6:-1] = rng.uniform(-100, 2200, (R, 2 * N)).astype(f32)
    if kind == "zero":
        rows[:, 4] = rng.choice([th, f32(0.0), f32(0.01), np.nextafter(th, f32(0)), f32(-1)], R)
        rows[:, -1] = rng.uniform(0, 50, R).astype(f32)
        return rows
    if kind in ("live128", "live129"):
        want = int(kind[4:])
        rows[:, 4] = th                                                   # at the threshold: not live
        pick = rng.permutation(R)[:want]
        rows[pick, 4] = rng.choice([np.nextafter(th, f32(1)), f32(0.3), f32(0.5), f32(0.97)], want)
        rows[:, -1] = rng.choice(np.arange(0, 40, dtype=f32), R)         # with ties
        return rows
    assert kind == "mixed"
    one = f32(1.0 / 1.2)
    scores = [th, np.nextafter(th, f32(1)), np.nextafter(th, f32(0)), f32(0.5), np.nextafter(f32(0.5), f32(0)),
              np.nextafter(f32(0.5), f32(1)), one, np.nextafter(one, f32(0)), np.nextafter(one, f32(1)),
              np.nextafter(np.nextafter(one, f32(1)), f32(1)), f32(0.9), f32(1.0), f32(0.02), f32(0.2), f32(0.7)]
    rows[:, 4] = rng.choice(scores, R)
    depths = np.array([-0.0, 0.0, 1.5, 1.5000001, 3.25, 7.0, 7.0, 12.75, 30.0, -2.5], f32)
    rows[:, -1] = rng.choice(depths, R)
    # vertices: both float32 neighbours of k + 0.995 (and the value itself), the two-decimal ties, negative values,
    # values past the canvas
    special = []
    for k in (0, 1, 2, 7, 63, 100, 511, 1023, 2047):
        v = f32(k + 0.995)
        special += [v, np.nextafter(v, f32(0)), np.nextafter(v, f32(1e9)), -v, -np.nextafter(v, f32(0)),
                    -np.nextafter(v, f32(1e9))]
        special += [f32(k + q) for q in (0.125, 0.375, 0.625, 0.875, 0.25, 0.75, 0.005, 0.985, 0.99, 0.996, 0.5)]
        special += [-f32(k + q) for q in (0.125, 0.875, 0.996, 0.5, 0.999)]
    special += [f32(v) for v in (-0.0, 0.0, -0.4, -0.996, -0.9999, -3.999, -1e5, 5000.7, 1e5, 2048.0, 2047.996,
                                 1023.9951)]
    special = np.array(special, f32)
    verts = rows[:, 6:-1]
    where = rng.rand(R, 2 * N) < 0.5
    verts[where] = rng.choice(special, int(where.sum()))
    flat = verts.reshape(-1)
    flat[:len(special)] = special                                         # each at least once (rows 0, 1, ...)
    rows[:, 6:-1] = flat.reshape(R, 2 * N)
    rows[:(len(special) + 2 * N - 1) // (2 * N), 4] = f32(0.7)           # ... and those rows are live
    rows[-len(scores):, 4] = scores                                       # every special score at least once
    return rows


SEEDED = [(128, 16, "mixed"), (128, 16, "zero"), (128, 16, "live128"), (1024, 16, "mixed"), (1024, 16, "zero"),
          (1024, 16, "live128"), (1024, 16, "live129"),
          # R = 128 cannot hold 129 live rows: the smallest R that can
          (129, 16, "live129"),
          (1024, 64, "mixed"), (128, 3, "mixed")]


@pytest.mark.gpu
def test_kernel_equals_image_instances_bit_for_bit():
    import torch
    ds = _dataset()
    gt = torch.zeros((1024, 2048), dtype=torch.int16, device="cuda")
    done = 0
    for case, (R, N, kind) in enumerate(SEEDED):
        rows = _seeded_rows(R, N, kind, seed=1000 + case)
        live = rows[:, 4] > np.float32(THRESH)
        if kind == "mixed":                                               # the case holds what it is there for
            lr = rows[live]
            th = np.float32(THRESH)
            assert (rows[:, 4] == th).any() and (rows[:, 4] == np.nextafter(th, np.float32(1))).any()
            assert (lr[:, 4] == np.float32(0.5)).any()
            c12 = lr[:, 4] * np.float32(1.2)
            assert (c12 < 1).any() and (c12 >= 1).any()
            key = {}
            for d, c in zip(lr[:, -1].tolist(), lr[:, 5].tolist()):
                key.setdefault(d, []).append(c)
            assert any(len(v) != len(set(v)) for v in key.values())       # a depth tie within a class
            assert any(len(set(v)) > 1 for v in key.values())             # ... and across classes
            v = lr[:, 6:-1]
            assert (v < 0).any() and (v > 2048).any() and (v == np.float32(7.995)).any()
            assert (v == np.nextafter(np.float32(7.995), np.float32(0))).any()
            assert (v == np.nextafter(np.float32(7.995), np.float32(1e9))).any() and (v == np.float32(7.125)).any()
        elif kind == "zero":
            assert not live.any()
        else:
            assert int(live.sum()) == int(kind[4:])
        params = ds.image_instances(_split(rows, 11))
        got = _kernel(rows)
        _assert_equals_host_list(rows, params, got)
        if kind == "zero":
            assert got[0] == 0
        if kind == "live129":
            assert got[0] == 129
            with pytest.raises(ValueError, match="more than 128 instances"):
                ds.score_instances_device(torch.from_numpy(rows).cuda(), gt, gt_table=np.zeros((0, 3), np.int64))
            with pytest.raises(ValueError, match="more than 128 instances"):   # the message of the host path
                ds.instance_masks_device(params)
        elif kind in ("live128", "zero") or R <= 128:
            # the scoring path takes it, and a dead slot draws nothing: as many counts as live instances
            res = ds.score_instances_device(torch.from_numpy(rows).cuda(), gt, gt_table=np.zeros((0, 3), np.int64))
            assert res["n"] == got[0] and np.array_equal(res["src"], got[1][:got[0]])
            assert res["inter"].shape == (got[0], 0)
        done += 1
    assert done == len(SEEDED) == 10


@pytest.mark.gpu
def test_vertex_rule_equals_the_text_form():
    """int(float("%.2f" % v)) on a dense set of float32 values: the kernel formats no text, the host does."""
    rng = np.random.RandomState(3)
    vals = []
    for k in range(0, 2049, 1):
        v = np.float32(k + 0.995)
        vals += [v, np.nextafter(v, np.float32(0)), np.nextafter(v, np.float32(1e9))]
    vals = np.array(vals, np.float32)
    vals = np.concatenate([vals, -vals, rng.uniform(-3000, 3000, 1024 * 2 * 64 - 2 * len(vals)).astype(np.float32)])
    rows = np.zeros((1024, 2 * 64 + 7), np.float32)
    rows[:, 4] = 0.3
    rows[:, -1] = np.arange(1024)                                         # slot k = row k
    rows[:, 6:-1] = vals.reshape(1024, 128)
    n, src, poly, _, _, _ = _kernel(rows)
    assert n == 1024 and np.array_equal(src, np.arange(1024))
    want = np.array([int(float("%.2f" % v)) for v in vals.tolist()], np.int64)
    assert np.array_equal(poly.reshape(-1).astype(np.int64), want)


# ------------------------------------------------ 3. the scoring path against the reference's recorded AP --
def _recorded_inter(rec):
    table = rec["gt_table"]
    col = {int(i): j for j, i in enumerate(table[:, 0])}
    inter = np.zeros((len(rec["label_id"]), len(table)), np.int64)
    for k, inst, cnt in rec["intersections"]:
        inter[k, col[int(inst)]] = cnt
    return inter


@pytest.mark.gpu
@pytest.mark.parametrize("table_from", ["device_histogram", "worker_bincount"])
def test_scoring_path_reproduces_recorded_counts_and_ap(table_from):
    import torch
    ds = _dataset()
    ev = il.InstanceLevelEvaluator()
    for name in CASES:
        r = _rec(name)
        rows = torch.from_numpy(_stack(_writer(name)[0])).cuda()
        table = None
        if table_from == "worker_bincount":
            table = il.gt_instances(np.bincount(r["gt_ids"].reshape(-1), minlength=65536))
        res = ds.score_instances_device(rows, r["gt_ids"], table, ev)
        kept = res["kept"]
        assert np.array_equal(res["gt_table"], r["gt_table"])
        assert np.array_equal(res["labels"][kept], r["label_id"])
        assert [float(c) for c in res["conf_text"]] == r["conf"].tolist()
        assert np.array_equal(res["counts"][kept], r["pixel_count"])
        assert np.array_equal(res["void"][kept], r["void_intersection"])
        # the recording holds the intersections of a prediction with the ground truth of its own label
        same = r["gt_table"][:, 1][None, :] == r["label_id"][:, None]
        assert same.any() and np.array_equal(res["inter"][kept][same], _recorded_inter(r)[same])
        # what the evaluator was handed: the same rows
        gt_table, preds = ev.images[-1]
        assert len(preds) == len(kept) and [p[2] for p in preds] == r["pixel_count"].tolist()
    got = ev.summarize()
    want = _rec("set")
    assert np.array_equal(np.isnan(got["resultApMatrix"]), np.isnan(want["ap"]))
    np.testing.assert_allclose(got["resultApMatrix"], want["ap"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(got["allAp"], float(want["all_ap"]), rtol=0, atol=1e-12)


# ------------------------------------------------------------------------------------------- 4. the driver --
def _driver():
    spec = importlib.util.spec_from_file_location("centerpoly_test_driver", os.path.join(ROOT, "test.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _cityscapes_set(tmp):
    """Four seeded 2048x1024 images with the fixture id images as ground truth, and a seeded, randomly initialised
    DLA-34 saved as a checkpoint.  A random `poly` head gives polygons of a pixel or two, which the writer's
    100-pixel rule drops: its bias is set to a seeded 16-gon of 6 to 10 output pixels radius and the `hm` bias to
    -1, so every image has live instances with masks that can meet the ground truth."""
    import torch
    from PIL import Image
    from centerpoly_amd.models.model import create_model, save_model
    rng = np.random.RandomState(11)
    img_dir, annot_dir, gt_dir = os.path.join(tmp, "images"), os.path.join(tmp, "BBoxes"), os.path.join(tmp, "gtFine")
    for d in (img_dir, annot_dir, os.path.join(gt_dir, "val", "frankfurt")):
        os.makedirs(d)
    images = []
    for k, c in enumerate(CASES):
        coarse = rng.randint(0, 256, (32, 64, 3)).astype(np.uint8)       # blocks of 32 pixels plus fine noise
        img = np.kron(coarse, np.ones((32, 32, 1), np.uint8)) // 2 + rng.randint(0, 128, (1024, 2048, 3)).astype(np.uint8)
        Image.fromarray(img.astype(np.uint8)).save(os.path.join(img_dir, "frankfurt_%s_leftImg8bit.png" % c),
                                                   compress_level=1)
        Image.fromarray(_rec(c)["gt_ids"]).save(os.path.join(gt_dir, "val", "frankfurt",
                                                             "frankfurt_%s_gtFine_instanceIds.png" % c))
        images.append({"id": 10 + k, "file_name": "frankfurt_%s_leftImg8bit.png" % c, "height": 1024, "width": 2048})
    with open(os.path.join(annot_dir, "val16_regular_interval.json"), "w") as f:
        json.dump({"images": images, "annotations": [], "categories": []}, f)
    torch.manual_seed(23)
    model = create_model("dla_34", {"hm": 8, "poly": 32, "pseudo_depth": 1, "reg": 2}, 256)
    with torch.no_grad():
        ang = np.arange(16) * (2 * np.pi / 16)
        rad = rng.uniform(6, 10, 16)
        bias = np.stack([rad * np.cos(ang), rad * np.sin(ang)], 1).reshape(-1)
        model.state_dict()["poly.2.bias"].copy_(torch.from_numpy(bias.astype(np.float32)))
        model.state_dict()["hm.2.bias"].fill_(-1.0)
    ckpt = os.path.join(tmp, "model_seeded.pth")
    save_model(ckpt, 1, model)
    return ["polydet", "--dataset", "cityscapes", "--annot_dir", annot_dir, "--img_dir", img_dir, "--gt_dir", gt_dir,
            "--load_model", ckpt, "--thresh", "0.05", "--num_workers", "2"]


def _tables(evaluator):
    return [(t.tolist(), [(lab, conf, pix, void, row.tolist()) for lab, conf, pix, void, row in preds])
            for t, preds in evaluator.images]


def _run_and_compare(driver, args, tmp_path, what, capsys):
    """test.py's run against CITYSCAPES.run_eval on the results dict of the same run: (allAp, tables, results.json)."""
    from centerpoly_amd.opts import opts
    opt = opts().parse(args)
    assert opt.K == 128                                                   # no image can exceed the 128-instance limit
    opt.save_dir = str(tmp_path / ("exp_" + what))
    out = driver.run_test(opt)
    ds = out["dataset"]
    tables = _tables(ds.last_evaluator)
    assert list(out["results"]) == [10, 11, 12, 13] and len(tables) == 4
    assert "AP_50%" in capsys.readouterr().out
    # equality of empty tables would prove nothing
    assert all(len(preds) > 0 for _, preds in tables)
    assert any(any(v > 0 for v in p[4]) for _, preds in tables for p in preds), "no mask met the ground truth"
    # the same run through the host path: CITYSCAPES.run_eval on the results dict
    ref_dir = str(tmp_path / ("ref_" + what))
    ref_ap = ds.run_eval(out["results"], ref_dir)
    assert not np.isnan(out["ap"]) and out["ap"] == ref_ap                 # to the last bit
    assert _tables(ds.last_evaluator) == tables
    a = open(os.path.join(opt.save_dir, "results.json"), "rb").read()
    assert a == open(os.path.join(ref_dir, "results.json"), "rb").read() and len(json.loads(a)) > 0
    js = os.path.join("results", "evaluationResults", "resultInstanceLevelSemanticLabeling.json")
    assert open(os.path.join(opt.save_dir, js)).read() == open(os.path.join(ref_dir, js)).read()
    files = sorted(f for _, _, fs in os.walk(os.path.join(opt.save_dir, "results")) for f in fs)
    assert files == sorted(f for _, _, fs in os.walk(os.path.join(ref_dir, "results")) for f in fs)
    if opt.no_mask_files:
        assert files == ["resultInstanceLevelSemanticLabeling.json"]
    else:
        assert sum(f.endswith(".txt") for f in files) == 4
        assert sum(f.endswith(".png") for f in files) == sum(len(preds) for _, preds in tables)
        for c in CASES:
            t = os.path.join("results", "frankfurt_%s_leftImg8bit.txt" % c)
            assert open(os.path.join(opt.save_dir, t)).read() == open(os.path.join(ref_dir, t)).read()
    return out["ap"], tables, a


@pytest.mark.gpu
def test_driver_scores_the_data_set(tmp_path, capsys):
    driver = _driver()
    base = _cityscapes_set(str(tmp_path))
    runs = {}
    for what, extra in (("prefetch", ["--no_mask_files"]), ("loop", ["--not_prefetch_test"])):
        runs[what] = _run_and_compare(driver, base + extra, tmp_path, what, capsys)
        assert len(json.loads(runs[what][2])) == 4 * 128                  # one scale: the K rows of every image
    assert runs["prefetch"] == runs["loop"]


@pytest.mark.gpu
def test_driver_uploads_rows_merged_on_the_host(tmp_path, capsys):
    """--nms (as --test_scales with more than one scale) keeps merge_outputs and its soft-NMS on the host: the merged
    rows are uploaded and scored by the same kernels."""
    driver = _driver()
    base = _cityscapes_set(str(tmp_path))
    nms = _run_and_compare(driver, base + ["--nms", "--no_mask_files"], tmp_path, "nms", capsys)
    plain = _run_and_compare(driver, base + ["--no_mask_files"], tmp_path, "plain", capsys)
    assert nms[2] != plain[2]                                             # soft-NMS moved scores: another input


@pytest.mark.gpu
def test_driver_names_a_missing_image(tmp_path):
    from centerpoly_amd.opts import opts
    driver = _driver()
    base = _cityscapes_set(str(tmp_path))
    os.remove(os.path.join(str(tmp_path), "images", "frankfurt_mixed32_leftImg8bit.png"))
    opt = opts().parse(base + ["--no_mask_files"])
    opt.save_dir = str(tmp_path / "exp")
    with pytest.raises(FileNotFoundError, match="frankfurt_mixed32_leftImg8bit.png"):
        driver.test(opt)

"""Cityscapes instance-level AP (centerpoly_amd/datasets/evaluation/instance_level.py on cp_id_histogram /
cp_instance_overlaps) against the fixtures recorded from the reference's own evaluator
(tests/golden/gen_instance_ap_golden.py).

CPU: the protocol on the recorded counts, the ground-truth table from a numpy histogram, the options, the limits of
the entry points.  GPU: the two kernels count for count against the recording and against a numpy restatement (a
joint np.bincount) at training-set scale and at odd sizes, the evaluator from device masks and from a result
directory, and CITYSCAPES.run_eval end to end.  Counts are integers: every comparison of them is exact.  AP values
are compared with atol 1e-12: their inputs are integer counts and parsed confidences, so the only freedom is the
order of one float64 dot product of at most a few hundred terms in [0, 1]."""
import ctypes
import json
import os
import types

import numpy as np
import pytest

from centerpoly_amd import _C
from centerpoly_amd.datasets.evaluation import instance_level as il

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = ["star16", "mixed32", "selfcross16", "small16"]
ODD = "odd37x53"


def _rec(name):
    return np.load(os.path.join(HERE, "golden", "instance_ap_%s.npz" % name), allow_pickle=False)


def _writer(name):
    z = np.load(os.path.join(HERE, "golden", "writer_%s.npz" % name), allow_pickle=False)
    masks = np.unpackbits(z["packed"], axis=2)[:, :, :2048].astype(np.uint8) * 255
    det = {int(k[4:]): z[k] for k in z.files if k.startswith("det_")}
    return masks[z["keep"]], det


def _masks(name):
    if name == ODD:
        return np.unpackbits(_rec(name)["masks_packed"], axis=2)[:, :, :53].astype(np.uint8) * 255
    return _writer(name)[0]


def _recorded_inter(rec):
    table = rec["gt_table"]
    col = {int(i): j for j, i in enumerate(table[:, 0])}
    inter = np.zeros((len(rec["label_id"]), len(table)), np.int64)
    for k, inst, cnt in rec["intersections"]:
        inter[k, col[int(inst)]] = cnt
    return inter


def _assert_ap(res):
    want = _rec("set")
    ap = res["resultApMatrix"]
    assert ap.shape == (1, 8, 10) and ap.dtype == np.float64
    assert np.array_equal(np.isnan(ap), np.isnan(want["ap"]))
    np.testing.assert_allclose(ap, want["ap"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(res["allAp"], float(want["all_ap"]), rtol=0, atol=1e-12)
    np.testing.assert_allclose(res["allAp50%"], float(want["all_ap50"]), rtol=0, atol=1e-12)
    assert [str(v) for v in want["inst_labels"]] == list(il.INST_LABELS) == list(res["classes"])
    for k, name in enumerate(il.INST_LABELS):
        np.testing.assert_allclose(res["classes"][name]["ap"], want["class_ap"][k], rtol=0, atol=1e-12)
        np.testing.assert_allclose(res["classes"][name]["ap50%"], want["class_ap50"][k], rtol=0, atol=1e-12)


def numpy_counts(masks, gt, inst_ids, void_ids):
    """The restatement: one joint np.bincount of (mask, id column) over the set pixels of every mask."""
    n, G = len(masks), len(inst_ids)
    col = np.full(65536, G, np.int64)                       # column G: an id nobody asked for
    col[np.asarray(inst_ids, np.int64)] = np.arange(G)
    is_void = np.zeros(65536, bool)
    is_void[[v for v in void_ids if 0 <= v < 65536]] = True
    flat = gt.reshape(-1)
    inter = np.zeros((n, G + 1), np.int64)
    void = np.zeros(n, np.int64)
    pix = np.zeros(n, np.int64)
    for i in range(n):
        ids = flat[masks[i].reshape(-1) != 0]
        inter[i] = np.bincount(col[ids], minlength=G + 1)
        void[i] = is_void[ids].sum()
        pix[i] = len(ids)
    return inter[:, :G], void, pix


# ------------------------------------------------------------------------------------------------------- CPU --
def test_fixture_is_worth_having():
    want = _rec("set")
    assert 0.05 < float(want["all_ap"]) < 0.95 and np.isfinite(want["ap"][0]).any(axis=1).sum() >= 6
    recs = [_rec(c) for c in CASES]
    assert any((r["void_intersection"] > 0).any() for r in recs)
    assert any((r["intersections"][:, 1] < 1000).any() for r in recs)
    assert any(((r["gt_table"][:, 0] >= 1000) & (r["gt_table"][:, 2] < 100)).any() for r in recs)
    assert any(np.bincount(r["intersections"][:, 1]).max() >= 2 for r in recs)


def test_summarize_reproduces_the_recorded_ap():
    ev = il.InstanceLevelEvaluator()
    for c in CASES:
        r = _rec(c)
        ev.add_counts(r["gt_table"], r["label_id"], r["conf"], r["pixel_count"], r["void_intersection"],
                      _recorded_inter(r))
    _assert_ap(ev.summarize())


def test_summarize_edge_cases():
    ev = il.InstanceLevelEvaluator()
    # a car with ground truth and no prediction: 0.0; every other class has no ground truth: nan
    ev.add_counts(np.array([[26001, 26, 500]]), [], [], [], [], np.zeros((0, 1)))
    res = ev.summarize()
    assert res["classes"]["car"]["ap"] == 0.0 and np.isnan(res["classes"]["person"]["ap"]) and res["allAp"] == 0.0
    # one perfect prediction -> 1.0; a label outside the eight and an empty mask are skipped
    ev = il.InstanceLevelEvaluator()
    ev.add_counts(np.array([[26001, 26, 500]]), [26, 7, 26], [0.9, 0.9, 0.9], [500, 500, 0], [0, 0, 0],
                  np.array([[500], [0], [0]]))
    assert ev.summarize()["allAp"] == 1.0
    # IoU test is `>`: 300 / (500 + 400 - 300) = 0.5 exactly does not match at 0.50, and the unmatched prediction
    # stays a false positive (its ignore share 0 <= 0.5)
    ev = il.InstanceLevelEvaluator()
    ev.add_counts(np.array([[26001, 26, 500]]), [26], [0.9], [400], [0], np.array([[300]]))
    assert ev.summarize()["classes"]["car"]["ap50%"] == 0.0
    # ignore test is `<=`: a void share of exactly 0.5 keeps the false positive at 0.50 and drops it at 0.45
    ev = il.InstanceLevelEvaluator()
    ev.add_counts(np.array([[26001, 26, 500], [26002, 26, 500]]), [26, 26], [0.9, 0.8], [500, 400], [0, 200],
                  np.array([[500, 0], [0, 0]]))
    res = ev.summarize()
    assert res["resultApMatrix"][0, 2, 0] == 0.5                     # tp at 0.9, fp at 0.8, one hard false negative


@pytest.mark.parametrize("name", CASES + [ODD])
def test_gt_instances_from_a_numpy_histogram(name):
    r = _rec(name)
    assert r["gt_ids"].dtype == np.uint16
    table = il.gt_instances(np.bincount(r["gt_ids"].reshape(-1), minlength=65536))
    assert table.dtype == np.int64 and np.array_equal(table, r["gt_table"])


def test_label_table():
    assert il.LABEL_IDS == (24, 25, 26, 27, 28, 31, 32, 33) and len(il.INST_LABELS) == 8
    assert sorted(il.VOID_IDS) == [-1, 0, 1, 2, 3, 4, 5, 6, 9, 10, 14, 15, 16, 18, 29, 30]
    np.testing.assert_allclose(il.OVERLAPS, np.arange(0.5, 1.0, 0.05), rtol=0, atol=0)
    assert il.MIN_REGION_SIZE == 100


def test_options(tmp_path, capsys):
    from centerpoly_amd.datasets.dataset.polygons import CITYSCAPES
    from centerpoly_amd.opts import opts
    opt = opts().parse(["polydet"])
    assert opt.gt_dir == "" and opt.no_mask_files is False
    opt = opts().parse(["polydet", "--gt_dir", str(tmp_path), "--no_mask_files"])
    assert opt.gt_dir == str(tmp_path) and opt.no_mask_files is True
    with pytest.raises(SystemExit):
        opts().parse(["polydet", "--no_mask_files"])
    assert "--no_mask_files needs --gt_dir" in capsys.readouterr().err
    # the default leaves run_eval as it was: files only, 0.0 (no detections here, so no device either)
    ds = CITYSCAPES.__new__(CITYSCAPES)
    ds.opt = opts().parse(["polydet"])
    ds.coco = types.SimpleNamespace(imgs={})
    assert ds.run_eval({}, str(tmp_path / "out")) == 0.0
    assert os.path.exists(str(tmp_path / "out" / "results.json"))
    assert not os.path.exists(str(tmp_path / "out" / "results" / "evaluationResults"))


def test_id_image_reading(tmp_path):
    from PIL import Image
    ids = np.array([[0, 7, 26001], [65535, 24, 3]], np.uint16)
    Image.fromarray(ids).save(str(tmp_path / "a_gtFine_instanceIds.png"))                  # 16-bit PNG
    Image.fromarray(ids.astype(np.int32)).save(str(tmp_path / "b_gtFine_instanceIds.tif"))   # 32-bit mode I
    for f in ("a_gtFine_instanceIds.png", "b_gtFine_instanceIds.tif"):
        got = il.read_gt_ids(str(tmp_path / f))
        assert got.dtype == np.uint16 and np.array_equal(got, ids)
    Image.fromarray(np.array([[70000, 1]], np.int32)).save(str(tmp_path / "c.tif"))
    with pytest.raises(ValueError, match="c.tif"):
        il.read_gt_ids(str(tmp_path / "c.tif"))
    os.makedirs(str(tmp_path / "x" / "y"))
    os.rename(str(tmp_path / "a_gtFine_instanceIds.png"), str(tmp_path / "x" / "y" / "a_gtFine_instanceIds.png"))
    assert il.find_gt_files(str(tmp_path)) == {"a": str(tmp_path / "x" / "y" / "a_gtFine_instanceIds.png")}


def test_abi_limits_without_gpu():
    """The entry points refuse what they cannot do before any device work: callable with no GPU."""
    L = _C.lib()
    p = ctypes.c_void_p(256)                                # never dereferenced: every call below returns first
    need = L.cp_instance_overlaps_workspace_bytes(128, 1024, 1024, 2048)
    assert need >= 65536 * 2
    ok_args = lambda n, G, V, H, W, ws: (p, n, p, H, W, p, G, p, V, p, p, p, p, ws, None)   # noqa: E731
    assert L.cp_instance_overlaps(*ok_args(129, 8, 15, 1024, 2048, need)) == -2
    assert L.cp_instance_overlaps(*ok_args(4, 1025, 15, 1024, 2048, need)) == -2
    assert L.cp_instance_overlaps(*ok_args(4, 8, 65, 1024, 2048, need)) == -2
    assert L.cp_instance_overlaps(*ok_args(4, 8, 15, 65536, 32768, need)) == -2           # H * W = 2^31
    assert L.cp_instance_overlaps(*ok_args(4, 8, 15, 1024, 2048, need - 1)) == -3         # short workspace
    assert L.cp_instance_overlaps(*ok_args(4, 8, 15, 0, 2048, need)) == -1
    assert L.cp_instance_overlaps(*ok_args(-1, 8, 15, 8, 8, need)) == -1
    assert L.cp_instance_overlaps(None, 4, p, 8, 8, p, 8, p, 15, p, p, p, p, need, None) == -1
    assert L.cp_id_histogram(None, 8, 8, p, None) == -1 and L.cp_id_histogram(p, 8, 0, p, None) == -1
    assert L.cp_id_histogram(p, 65536, 32768, p, None) == -2


# ------------------------------------------------------------------------------------------------------- GPU --
def _dev_ids(gt):
    import torch
    return torch.from_numpy(np.ascontiguousarray(gt).view(np.int16)).cuda()


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES + [ODD])
def test_kernels_reproduce_the_recorded_counts(name):
    import torch
    r = _rec(name)
    gt = _dev_ids(r["gt_ids"])
    hist = il.device_histogram(gt)
    assert np.array_equal(hist, np.bincount(r["gt_ids"].reshape(-1), minlength=65536))
    assert np.array_equal(il.gt_instances(hist), r["gt_table"])
    masks = torch.from_numpy(_masks(name)).cuda()
    inter, void, pix = il.device_counts(masks, gt, r["gt_table"][:, 0])
    assert np.array_equal(pix, r["pixel_count"])
    assert np.array_equal(void, r["void_intersection"])
    # the evaluator only intersects a prediction with the ground truth of its own label; the other pairs the
    # kernel counts as well are held to numpy in the next test
    same = r["gt_table"][:, 1][None, :] == r["label_id"][:, None]
    assert same.any() and np.array_equal(inter[same], _recorded_inter(r)[same])


def _scene(H, W, n, G, seed):
    """Seeded id image with G ids of interest (instances, groups) plus void and road, and n masks: discs,
    rectangles, one all-zero and one all-ones mask."""
    rng = np.random.RandomState(seed)
    gt = np.full((H, W), 7, np.uint16)
    gt[:, :max(W // 50, 1)] = 3
    gt[H - max(H // 40, 1):, :] = 1
    labels = np.array(il.LABEL_IDS)
    inst = []
    for j in range(G):
        lab = int(labels[rng.randint(8)])
        v = lab * 1000 + j if j % 7 else (lab if lab not in inst else lab * 1000 + j)     # some groups
        inst.append(v)
        h, w = rng.randint(1, max(H // 6, 2)), rng.randint(1, max(W // 8, 2))
        y, x = rng.randint(0, H), rng.randint(0, W)
        gt[y:y + h, x:x + w] = v
    gt[H // 3:H // 3 + max(H // 30, 1), W // 2:] = 29004                                  # a caravan: not void
    masks = np.zeros((n, H, W), np.uint8)
    yy, xx = np.mgrid[0:H, 0:W]
    for i in range(n):
        if i == n // 2:
            continue                                                                       # all zero
        if i == n // 3:
            masks[i] = 255                                                                 # all ones
            continue
        y, x = rng.randint(0, H), rng.randint(0, W)
        if i % 2:
            r = rng.randint(1, max(min(H, W) // 5, 2))
            masks[i][(yy - y) ** 2 + (xx - x) ** 2 <= r * r] = rng.choice([1, 128, 255])
        else:
            masks[i, y:y + rng.randint(1, max(H // 4, 2)), x:x + rng.randint(1, max(W // 4, 2))] = 255
    return gt, masks, inst


@pytest.mark.gpu
@pytest.mark.parametrize("H,W,n,G", [(1024, 2048, 128, 150), (1, 1, 3, 2), (37, 53, 9, 12), (1024, 2047, 20, 40),
                                     (256, 512, 17, 1024)])
def test_kernels_equal_numpy_at_scale_and_odd_sizes(H, W, n, G):
    import torch
    gt, masks, inst = _scene(H, W, n, G, seed=H * 7 + W)
    assert len(set(inst)) == G
    g_dev, m_dev = _dev_ids(gt), torch.from_numpy(masks).cuda()
    assert np.array_equal(il.device_histogram(g_dev), np.bincount(gt.reshape(-1), minlength=65536))
    got = il.device_counts(m_dev, g_dev, inst)
    want = numpy_counts(masks, gt, inst, il.VOID_IDS)
    for a, b, what in zip(got, want, ("inter", "void", "pixels")):
        assert np.array_equal(a, b), "%s differs at %s" % (what, np.argwhere(a != b)[:5].tolist())
    assert want[1].sum() > 0 or H == 1                      # the void strips are hit, the caravan is not void
    again = il.device_counts(m_dev, g_dev, inst)            # same call, same output
    assert all(np.array_equal(a, b) for a, b in zip(got, again))
    assert np.array_equal(il.device_histogram(g_dev), il.device_histogram(g_dev))


@pytest.mark.gpu
def test_evaluator_from_device_masks():
    import torch
    ev = il.InstanceLevelEvaluator()
    for c in CASES:
        r = _rec(c)
        ev.add_image(torch.from_numpy(_masks(c)).cuda(), r["label_id"].tolist(), r["conf"].tolist(), r["gt_ids"])
    _assert_ap(ev.summarize())


@pytest.mark.gpu
def test_evaluate_result_dir(tmp_path):
    from PIL import Image
    os.makedirs(str(tmp_path / "res" / "masks"))
    os.makedirs(str(tmp_path / "gt" / "frankfurt"))
    gt_files = []
    for c in CASES:
        r = _rec(c)
        gt_files.append(str(tmp_path / "gt" / "frankfurt" / ("frankfurt_%s_gtFine_instanceIds.png" % c)))
        Image.fromarray(r["gt_ids"]).save(gt_files[-1])
        lines = [str(l) for l in r["lines"]]
        with open(str(tmp_path / "res" / ("frankfurt_%s_leftImg8bit.txt" % c)), "w") as f:
            f.write("".join(lines))
        for line, m in zip(lines, _masks(c)):
            Image.fromarray(m).save(str(tmp_path / "res" / line.split(" ")[0]))
    _assert_ap(il.evaluate_result_dir(str(tmp_path / "res"), gt_files))
    with pytest.raises(FileNotFoundError, match="zurich"):
        il.evaluate_result_dir(str(tmp_path / "res"), [str(tmp_path / "gt" / "zurich_gtFine_instanceIds.png")])


def _dataset(tmp_path, extra):
    from PIL import Image
    from centerpoly_amd.datasets.dataset.polygons import CITYSCAPES
    from centerpoly_amd.opts import opts
    gt_dir = tmp_path / "gtFine" / "val" / "frankfurt"
    os.makedirs(str(gt_dir), exist_ok=True)
    for c in CASES:
        Image.fromarray(_rec(c)["gt_ids"]).save(str(gt_dir / ("frankfurt_%s_gtFine_instanceIds.png" % c)))
    ds = CITYSCAPES.__new__(CITYSCAPES)
    ds.opt = opts().parse(["polydet", "--gt_dir", str(tmp_path / "gtFine")] + extra)
    assert ds.opt.thresh == 0.05
    ds.coco = types.SimpleNamespace(imgs={k: {"id": k, "file_name": "/data/frankfurt_%s_leftImg8bit.png" % c}
                                          for k, c in enumerate(CASES)})
    # CITYSCAPES is an 8-class data set here (as in the reference's mode this project mirrors): run_eval's
    # results.json has no category for the pole / sign / light rows mixed32 carries for the writer's label rule.
    # Those rows draw nothing and hide nothing, so the masks and the recorded lines are the same without them
    # (test_run_eval_end_to_end compares the written lines with the recording).
    return ds, {k: {cls: rows for cls, rows in _writer(c)[1].items() if cls <= ds.num_classes}
                for k, c in enumerate(CASES)}


@pytest.mark.gpu
def test_run_eval_end_to_end(tmp_path, capsys):
    want = _rec("set")
    ds, results = _dataset(tmp_path, [])
    save = str(tmp_path / "exp")
    ap = ds.run_eval(results, save)
    np.testing.assert_allclose(ap, float(want["all_ap"]), rtol=0, atol=1e-12)
    out = capsys.readouterr().out
    assert "AP_50%" in out and "average" in out and "bicycle" in out
    js = json.load(open(os.path.join(save, "results", "evaluationResults", "resultInstanceLevelSemanticLabeling.json")))
    assert set(js) == {"averages", "overlaps", "minRegionSizes", "instLabels", "resultApMatrix"}
    assert js["instLabels"] == list(il.INST_LABELS) and js["minRegionSizes"] == [100, 1000, 1000]
    np.testing.assert_allclose(np.array(js["resultApMatrix"], np.float64), want["ap"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(js["averages"]["allAp"], float(want["all_ap"]), rtol=0, atol=1e-12)
    # the files are still written, with the recorded lines (the confidences the evaluator used)
    for c in CASES:
        txt = open(os.path.join(save, "results", "frankfurt_%s_leftImg8bit.txt" % c)).read()
        assert txt == "".join(str(l) for l in _rec(c)["lines"])
    assert len(os.listdir(os.path.join(save, "results", "masks"))) == sum(len(_rec(c)["lines"]) for c in CASES)


@pytest.mark.gpu
def test_run_eval_in_memory_writes_no_masks(tmp_path):
    ds, results = _dataset(tmp_path, ["--no_mask_files"])
    save = str(tmp_path / "exp")
    ap = ds.run_eval(results, save)
    np.testing.assert_allclose(ap, float(_rec("set")["all_ap"]), rtol=0, atol=1e-12)
    found = [f for _, _, files in os.walk(save) for f in files]
    assert not [f for f in found if f.endswith(".png") or f.endswith(".txt")]
    assert "resultInstanceLevelSemanticLabeling.json" in found and "results.json" in found


@pytest.mark.gpu
def test_run_eval_names_a_missing_ground_truth(tmp_path):
    ds, results = _dataset(tmp_path, [])
    os.remove(str(tmp_path / "gtFine" / "val" / "frankfurt" / "frankfurt_mixed32_gtFine_instanceIds.png"))
    with pytest.raises(FileNotFoundError, match="frankfurt_mixed32_gtFine_instanceIds.png"):
        ds.run_eval(results, str(tmp_path / "exp"))

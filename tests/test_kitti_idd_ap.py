"""Instance-level AP of the KITTI and IDD recipes: the evaluator's protocols against the reference's own kittiscripts
and IDDscripts evaluators (tests/golden/kitti_idd_ap_*.npz, made by tests/golden/gen_kitti_idd_ap_golden.py from the
masks of tests/golden/class_writer_*.npz), run_eval and test.py's per-image path end to end on the device."""
import json
import os
import types

import numpy as np
import pytest

from centerpoly_amd.datasets.evaluation import instance_level as il

HERE = os.path.dirname(os.path.abspath(__file__))
SETS = {"kitti": (il.KITTI, ["kitti_a", "kitti_b"], ["odd"]), "idd": (il.IDD, ["idd_a", "idd_b"], [])}
ALL = [(s, c) for s, (_, scored, extra) in SETS.items() for c in scored + extra]


def _rec(name):
    return np.load(os.path.join(HERE, "golden", "kitti_idd_ap_%s.npz" % name), allow_pickle=False)


def _writer(name):
    return np.load(os.path.join(HERE, "golden", "class_writer_%s.npz" % name), allow_pickle=False)


def _masks(name):
    z = _writer(name)
    return np.unpackbits(z["packed"], axis=2)[:, :, :int(z["width"])].astype(np.uint8) * 255


def _confs(name):
    return [float(str(l).split(" ")[2]) for l in _writer(name)["lines"]]


def _same_label(inter, labels, table):
    """The evaluator looks at a prediction's overlap with ground truth of its own label only: the other columns of
    a count table are counted by the kernel and never read."""
    return inter * (np.asarray(labels)[:, None] == np.asarray(table)[None, :, 1])


def _recorded_inter(rec, n_lines):
    """[text lines, G]: the recorded intersections (a prediction's, with the ground truth of its label); lines the
    evaluator skipped (empty masks) stay zero."""
    table = rec["gt_table"]
    col = {int(i): j for j, i in enumerate(table[:, 0])}
    inter = np.zeros((n_lines, len(table)), np.int64)
    for k, inst, cnt in rec["intersections"]:
        inter[k, col[int(inst)]] = cnt
    return inter


def _recorded_columns(rec, name):
    """label, pixels, void per text line; a line the evaluator skipped has no pixels."""
    z = _writer(name)
    n = len(z["lines"])
    lab = np.array([int(str(l).split(" ")[1]) for l in z["lines"]], np.int64)
    pix, void = np.zeros(n, np.int64), np.zeros(n, np.int64)
    pix[rec["scored_lines"]], void[rec["scored_lines"]] = rec["pixel_count"], rec["void_intersection"]
    assert np.array_equal(lab[rec["scored_lines"]], rec["label_id"])
    assert np.array_equal(pix, z["counts"])
    return lab, pix, void


def _assert_ap(res, which):
    proto = SETS[which][0]
    want = _rec("set_" + which)
    ap = res["resultApMatrix"]
    assert ap.shape == (1, len(proto.label_ids), 10) and ap.dtype == np.float64
    assert np.array_equal(np.isnan(ap), np.isnan(want["ap"]))
    np.testing.assert_allclose(ap, want["ap"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(res["allAp"], float(want["all_ap"]), rtol=0, atol=1e-12)
    np.testing.assert_allclose(res["allAp50%"], float(want["all_ap50"]), rtol=0, atol=1e-12)
    assert [str(v) for v in want["inst_labels"]] == list(proto.inst_labels) == list(res["classes"])
    for k, name in enumerate(proto.inst_labels):
        np.testing.assert_allclose(res["classes"][name]["ap"], want["class_ap"][k], rtol=0, atol=1e-12, equal_nan=True)
        np.testing.assert_allclose(res["classes"][name]["ap50%"], want["class_ap50"][k], rtol=0, atol=1e-12,
                                   equal_nan=True)


# ------------------------------------------------------------------------------------------------------- CPU --
@pytest.mark.parametrize("which", sorted(SETS))
def test_summarize_reproduces_the_reference(which):
    """Fed the recorded counts in text-line order, the protocol reproduces the reference's AP matrix and averages."""
    proto, scored, _ = SETS[which]
    ev = il.InstanceLevelEvaluator(protocol=proto)
    for c in scored:
        r = _rec(c)
        lab, pix, void = _recorded_columns(r, c)
        ev.add_counts(r["gt_table"], lab, _confs(c), pix, void, _recorded_inter(r, len(lab)))
    res = ev.summarize()
    _assert_ap(res, which)
    js = il.results_json(res, proto)
    assert js["instLabels"] == list(proto.inst_labels)
    assert "average" in il.format_results(res, proto) and proto.inst_labels[-1] in il.format_results(res, proto)


@pytest.mark.parametrize("which", sorted(SETS))
def test_protocol_tables(which):
    """Labels, ids and void values are the evaluator's own (read from its label table when the fixtures were made)."""
    proto = SETS[which][0]
    want = _rec("set_" + which)
    assert list(proto.inst_labels) == [str(v) for v in want["inst_labels"]]
    assert list(proto.label_ids) == want["inst_ids"].tolist()
    assert sorted(proto.void_ids) == sorted(want["void_ids"].tolist()) and len(proto.void_ids) <= 64
    assert il.PROTOCOLS[proto.name] is proto


@pytest.mark.parametrize("which,name", ALL)
def test_gt_instances(which, name):
    proto = SETS[which][0]
    r = _rec(name)
    hist = np.bincount(r["gt_ids"].reshape(-1), minlength=65536)
    assert np.array_equal(il.gt_instances(hist, protocol=proto), r["gt_table"])
    assert len(np.unique(r["gt_ids"])) > len(r["gt_table"])            # some ids are kept out


def test_idd_fixtures_hold_what_the_filter_drops():
    ids = np.unique(np.concatenate([_rec(c)["gt_ids"].reshape(-1) for c in SETS["idd"][1]]))
    kept = np.unique(np.concatenate([_rec(c)["gt_table"][:, 0] for c in SETS["idd"][1]]))
    out = np.setdiff1d(ids, kept)
    assert 255 in out and (out // 1000 >= 19).any() and ((out >= 1000) & (out // 1000 <= 5)).any()
    assert ((out >= 6) & (out <= 18)).any()                               # a bare label id: a group elsewhere
    assert (kept // 1000 > 5).all() and (kept // 1000 < 19).all()


def test_default_protocol_is_cityscapes_as_before():
    """No protocol given: the Cityscapes fixtures score bit for bit as with the protocol named."""
    cases = ["star16", "mixed32", "selfcross16", "small16"]
    a, b = il.InstanceLevelEvaluator(), il.InstanceLevelEvaluator(protocol=il.CITYSCAPES)
    for c in cases:
        r = np.load(os.path.join(HERE, "golden", "instance_ap_%s.npz" % c), allow_pickle=False)
        table = r["gt_table"]
        col = {int(i): j for j, i in enumerate(table[:, 0])}
        inter = np.zeros((len(r["label_id"]), len(table)), np.int64)
        for k, inst, cnt in r["intersections"]:
            inter[k, col[int(inst)]] = cnt
        for ev in (a, b):
            ev.add_counts(table, r["label_id"], r["conf"], r["pixel_count"], r["void_intersection"], inter)
        hist = np.bincount(r["gt_ids"].reshape(-1), minlength=65536)
        assert np.array_equal(il.gt_instances(hist), il.gt_instances(hist, il.CITYSCAPES))
        assert np.array_equal(il.gt_instances(hist), table)
    ra, rb = a.summarize(), b.summarize()
    want = np.load(os.path.join(HERE, "golden", "instance_ap_set.npz"), allow_pickle=False)
    assert ra["resultApMatrix"].tobytes() == rb["resultApMatrix"].tobytes() and ra["allAp"] == rb["allAp"]
    np.testing.assert_allclose(ra["resultApMatrix"], want["ap"], rtol=0, atol=1e-12)
    assert il.results_json(ra) == il.results_json(rb, il.CITYSCAPES)
    assert il.format_results(ra) == il.format_results(rb, il.CITYSCAPES)
    assert (il.CITYSCAPES.inst_labels, il.CITYSCAPES.label_ids, il.CITYSCAPES.void_ids) == \
        (il.INST_LABELS, il.LABEL_IDS, il.VOID_IDS)


def test_ground_truth_matchers(tmp_path):
    def touch(*parts):
        os.makedirs(str(tmp_path.joinpath(*parts[:-1])), exist_ok=True)
        tmp_path.joinpath(*parts).write_bytes(b"")
        return str(tmp_path.joinpath(*parts))
    k1 = touch("kitti", "training", "instance", "000012.png")
    touch("kitti", "training", "instance", "notes.txt")
    assert il.find_gt_files(str(tmp_path / "kitti"), protocol=il.KITTI) == {"000012": k1}
    assert il.KITTI.image_key("/data/training/image_2/000012.png") == "000012"
    assert il.KITTI.pred_match("000012.txt", "000012") and not il.KITTI.pred_match("1000012.txt", "000012")
    i1 = touch("idd", "gtFine", "val", "201", "frame0029_gtFine_instanceids.png")
    i2 = touch("idd", "gtFine", "val", "305", "frame0029_gtFine_instanceids.png")      # the same frame, another city
    touch("idd", "gtFine", "val", "305", "frame0029_gtFine_labelids.png")
    touch("idd", "gtFine", "val", "305", "frame0030_gtFine_instanceIds.png")           # Cityscapes' spelling: not IDD's
    assert il.find_gt_files(str(tmp_path / "idd"), protocol=il.IDD) == {"201/frame0029": i1, "305/frame0029": i2}
    assert il.IDD.image_key("/data/leftImg8bit/val/201/frame0029_leftImg8bit.png") == "201/frame0029"
    assert il.IDD.pred_match("201/frame0029_leftImg8bit.txt", "201/frame0029")
    assert not il.IDD.pred_match("305/frame0029_leftImg8bit.txt", "201/frame0029")
    assert il.IDD.gt_name("201/frame0029") == "201/frame0029_gtFine_instanceids.png"
    c1 = touch("cs", "val", "frankfurt", "frankfurt_000000_000294_gtFine_instanceIds.png")
    assert il.find_gt_files(str(tmp_path / "cs")) == {"frankfurt_000000_000294": c1}
    touch("kitti", "other", "000012.png")
    with pytest.raises(ValueError, match="two ground-truth files"):
        il.find_gt_files(str(tmp_path / "kitti"), protocol=il.KITTI)


def test_metric_ap_is_still_refused_and_test_py_has_its_own_switch():
    from centerpoly_amd.datasets.dataset.polygons import CITYSCAPES, IDD, KITTIPOLY
    assert (KITTIPOLY.scores_ap, IDD.scores_ap, CITYSCAPES.scores_ap) == (False, False, True)
    assert (KITTIPOLY.ap_protocol, IDD.ap_protocol) == ("kitti", "IDD") and not hasattr(CITYSCAPES, "ap_protocol")
    assert (KITTIPOLY.at_threshold, IDD.at_threshold, KITTIPOLY.per_city, IDD.per_city) == (False, True, False, True)


# ------------------------------------------------------------------------------------------------------- GPU --
def _dataset(tmp_path, which, extra=(), sizes=True):
    """The data set object run_eval needs, its ground truth written below tmp_path/gt in the data set's layout."""
    from PIL import Image
    from centerpoly_amd.datasets.dataset.polygons import IDD, KITTIPOLY
    from centerpoly_amd.opts import opts
    proto, scored, _ = SETS[which]
    cls = KITTIPOLY if which == "kitti" else IDD
    imgs, results = {}, {}
    for k, c in enumerate(scored):
        z = _writer(c)
        file_name = "/data/" + str(z["file_name"])
        key = proto.image_key(file_name)
        path = tmp_path / "gt" / (proto.gt_name(key) if which == "idd" else os.path.join("training", "instance", proto.gt_name(key)))
        os.makedirs(str(path.parent), exist_ok=True)
        Image.fromarray(_rec(c)["gt_ids"]).save(str(path))
        imgs[k] = {"id": k, "file_name": file_name}
        if sizes:
            imgs[k].update(width=int(z["width"]), height=int(z["height"]))
        rows = z["rows"]
        results[k] = {j + 1: np.delete(rows[rows[:, 5] == j], 5, axis=1) for j in range(len(z["labels"]))}
    ds = cls.__new__(cls)
    ds.opt = opts().parse(["polydet", "--dataset", cls.name, "--gt_dir", str(tmp_path / "gt"), "--thresh", "0.3"]
                          + list(extra))
    ds.coco = types.SimpleNamespace(imgs=imgs)
    ds.img_dir = str(tmp_path / "images")
    return ds, results


def _written(save, which, c):
    z = _writer(c)
    base = os.path.basename(str(z["file_name"]))
    sub = os.path.basename(os.path.dirname(str(z["file_name"]))) if which == "idd" else ""
    return os.path.join(save, "results", sub), base


@pytest.mark.gpu
@pytest.mark.parametrize("which", sorted(SETS))
def test_run_eval_end_to_end(tmp_path, capsys, which):
    from PIL import Image
    proto, scored, _ = SETS[which]
    want = _rec("set_" + which)
    ds, results = _dataset(tmp_path, which)
    save = str(tmp_path / "exp")
    ap = ds.run_eval(results, save)
    np.testing.assert_allclose(ap, float(want["all_ap"]), rtol=0, atol=1e-12)
    _assert_ap(ds.last_evaluator.summarize(), which)
    out = capsys.readouterr().out
    assert "AP_50%" in out and "average" in out and proto.inst_labels[-1] in out
    js = json.load(open(os.path.join(save, "results", "evaluationResults", "resultInstanceLevelSemanticLabeling.json")))
    assert set(js) == {"averages", "overlaps", "minRegionSizes", "instLabels", "resultApMatrix"}
    assert js["instLabels"] == list(proto.inst_labels)
    got = np.array([[np.nan if v is None else v for v in row] for row in js["resultApMatrix"][0]], np.float64)
    np.testing.assert_allclose(got, want["ap"][0], rtol=0, atol=1e-12, equal_nan=True)
    np.testing.assert_allclose(js["averages"]["allAp"], float(want["all_ap"]), rtol=0, atol=1e-12)
    for c in scored:                                        # the files: the recorded bytes, the recorded masks
        d, base = _written(save, which, c)
        z = _writer(c)
        assert open(os.path.join(d, base.replace(".png", ".txt"))).read() == "".join(str(l) for l in z["lines"])
        masks = _masks(c)
        for k in range(len(masks)):
            got = np.array(Image.open(os.path.join(d, base.replace(".png", "_%d.png" % k))))
            assert got.dtype == np.uint8 and np.array_equal(got, masks[k]), "%s mask %d" % (c, k)
        assert len([f for f in os.listdir(d) if f.startswith(base[:-4] + "_") and f.endswith(".png")]) == len(masks)
    # the written directory scores the same through the file reader
    res = il.evaluate_result_dir(os.path.join(save, "results"), sorted(il.find_gt_files(str(tmp_path / "gt"), proto).values()),
                                 protocol=proto)
    _assert_ap(res, which)


@pytest.mark.gpu
@pytest.mark.parametrize("which", sorted(SETS))
def test_per_image_path_gives_run_evals_tables(tmp_path, which):
    """test.py's path: rows on the device -> selection -> masks -> overlaps, one read; the same evaluator tables."""
    import torch
    proto, scored, extra = SETS[which]
    ds, results = _dataset(tmp_path, which, ["--no_mask_files"])
    ds.run_eval(results, str(tmp_path / "exp"))
    by_run_eval = ds.last_evaluator
    ev = il.InstanceLevelEvaluator(proto)
    for c in scored:
        z, r = _writer(c), _rec(c)
        res = ds.score_instances_device(torch.from_numpy(z["rows"]).cuda(), r["gt_ids"], evaluator=ev)
        lab, pix, void = _recorded_columns(r, c)
        assert res["n"] == len(lab) and res["text_index"].tolist() == list(range(len(lab)))
        assert res["labels"].tolist() == lab.tolist() and res["counts"].tolist() == pix.tolist()
        assert res["void"].tolist() == void.tolist()
        assert np.array_equal(res["gt_table"], r["gt_table"])
        assert np.array_equal(_same_label(res["inter"], lab, r["gt_table"]), _recorded_inter(r, len(lab)))
        assert [c2 + "\n" for c2 in res["conf_text"]] == [str(l).split(" ")[2] for l in z["lines"]]
    assert len(ev.images) == len(by_run_eval.images)
    for (ta, pa), (tb, pb) in zip(ev.images, by_run_eval.images):
        assert np.array_equal(ta, tb) and len(pa) == len(pb)
        for x, y in zip(pa, pb):
            assert x[:4] == y[:4] and np.array_equal(x[4], y[4])
    _assert_ap(ev.summarize(), which)
    for c in extra:                                         # the odd canvas: counts only, with the table given
        z, r = _writer(c), _rec(c)
        res = ds.score_instances_device(torch.from_numpy(z["rows"]).cuda(), r["gt_ids"], gt_table=r["gt_table"])
        lab, pix, void = _recorded_columns(r, c)
        assert res["counts"].tolist() == pix.tolist() and res["void"].tolist() == void.tolist()
        assert np.array_equal(_same_label(res["inter"], lab, r["gt_table"]), _recorded_inter(r, len(lab)))


@pytest.mark.gpu
@pytest.mark.parametrize("which", sorted(SETS))
def test_no_mask_files_and_no_gt_dir(tmp_path, which):
    ds, results = _dataset(tmp_path, which, ["--no_mask_files"])
    save = str(tmp_path / "exp")
    ap = ds.run_eval(results, save)
    np.testing.assert_allclose(ap, float(_rec("set_" + which)["all_ap"]), rtol=0, atol=1e-12)
    found = [f for _, _, files in os.walk(save) for f in files]
    assert not [f for f in found if f.endswith(".png") or f.endswith(".txt")]
    assert "resultInstanceLevelSemanticLabeling.json" in found and "results.json" in found
    # without --gt_dir: the files, no score
    ds.opt.gt_dir, ds.opt.no_mask_files = "", False
    assert ds.run_eval(results, str(tmp_path / "plain")) == 0.0
    found = [f for _, _, files in os.walk(str(tmp_path / "plain")) for f in files]
    n_lines = sum(len(_writer(c)["lines"]) for c in SETS[which][1])
    assert len([f for f in found if f.endswith(".png")]) == n_lines and "results.json" in found
    assert "resultInstanceLevelSemanticLabeling.json" not in found


@pytest.mark.gpu
def test_canvas_and_ground_truth_errors(tmp_path):
    from PIL import Image
    ds, results = _dataset(tmp_path, "kitti", sizes=False)
    with pytest.raises(FileNotFoundError, match="000012.png"):          # no width / height and no image file
        ds.run_eval(results, str(tmp_path / "exp"))
    os.makedirs(ds.img_dir)
    for c in SETS["kitti"][1]:                                           # the canvas from the image's header
        z = _writer(c)
        Image.new("RGB", (int(z["width"]), int(z["height"]))).save(os.path.join(ds.img_dir, os.path.basename(str(z["file_name"]))))
    np.testing.assert_allclose(ds.run_eval(results, str(tmp_path / "exp")), float(_rec("set_kitti")["all_ap"]),
                               rtol=0, atol=1e-12)
    Image.new("RGB", (1000, 375)).save(os.path.join(ds.img_dir, "000347.png"))
    with pytest.raises(ValueError, match=r"000347.png is \(375, 1242\), the image .*000347.png is \(375, 1000\)"):
        ds.run_eval(results, str(tmp_path / "exp2"))
    os.remove(str(tmp_path / "gt" / "training" / "instance" / "000012.png"))
    with pytest.raises(FileNotFoundError, match="no ground truth 000012.png"):
        ds.run_eval(results, str(tmp_path / "exp3"))

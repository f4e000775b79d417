"""The Cityscapes instance-level AP with distances (AP 100 m / AP 50 m) without a GPU: the evaluator on the recorded
counts plus the recorded distance tables against the reference evaluator's `distanceAvailable = True` results
(tests/golden/instance_ap_dist_set.npz, made by tests/golden/gen_instance_ap_dist_golden.py), the host mapping from
the median integers to metres, the file readers, the options and the argument checks of cp_segment_medians."""
import ctypes
import json
import os

import numpy as np
import pytest

import distance_ref
from centerpoly_amd import _C
from centerpoly_amd.datasets.evaluation import distances
from centerpoly_amd.datasets.evaluation import instance_level as il

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = ["star16", "mixed32", "selfcross16", "small16"]


def _rec(name):
    return np.load(os.path.join(HERE, "golden", "instance_ap_%s.npz" % name), allow_pickle=False)


def _recorded_inter(rec):
    table = rec["gt_table"]
    col = {int(i): j for j, i in enumerate(table[:, 0])}
    inter = np.zeros((len(rec["label_id"]), len(table)), np.int64)
    for k, inst, cnt in rec["intersections"]:
        inter[k, col[int(inst)]] = cnt
    return inter


def _evaluator(with_distances):
    want = _rec("dist_set")
    ev = il.InstanceLevelEvaluator(il.CITYSCAPES, distances=with_distances)
    for c in CASES:
        r = _rec(c)
        extra = {"gt_dist": want["dist_%s" % c]} if with_distances else {}
        ev.add_counts(r["gt_table"], r["label_id"], r["conf"], r["pixel_count"], r["void_intersection"],
                      _recorded_inter(r), **extra)
    return ev


def assert_golden(res):
    """A summarize() dictionary against the recorded matrix and averages, within 1e-12."""
    want = _rec("dist_set")
    ap = res["resultApMatrix"]
    assert ap.shape == (3, 8, 10) and ap.dtype == np.float64
    assert np.array_equal(np.isnan(ap), np.isnan(want["ap"]))
    np.testing.assert_allclose(ap, want["ap"], rtol=0, atol=1e-12)
    assert [str(v) for v in want["average_names"]] == ["allAp", "allAp50%", "allAp50m", "allAp100m", "allAp50%50m"]
    for k, v in zip(want["average_names"], want["averages"]):
        np.testing.assert_allclose(res[str(k)], v, rtol=0, atol=1e-12)
    assert [str(v) for v in want["inst_labels"]] == list(il.INST_LABELS) == list(res["classes"])
    for li, name in enumerate(il.INST_LABELS):
        assert sorted(res["classes"][name]) == sorted(str(k) for k in want["class_average_names"])
        for k, v in zip(want["class_average_names"], want["class_averages"][li]):
            np.testing.assert_allclose(res["classes"][name][str(k)], v, rtol=0, atol=1e-12, equal_nan=True)


def test_fixture_meets_its_conditions():
    want = _rec("dist_set")
    t = np.concatenate([want["dist_%s" % c] for c in CASES])
    g = np.concatenate([_rec(c)["gt_table"] for c in CASES])
    assert t.shape == (len(g), 2) and t.dtype == np.float64
    real = g[:, 0] >= 1000
    big, dense = real & (g[:, 2] >= 1000), t[:, 1] >= 0.5
    assert (big & dense & (t[:, 0] > 100)).sum() >= 1                      # excluded by the 100 m bound alone
    assert (big & dense & (t[:, 0] > 50) & (t[:, 0] <= 100)).sum() >= 1    # by the 50 m bound alone
    assert (big & ~dense & (t[:, 0] <= 50)).sum() >= 1                     # by the stereo density alone
    assert (real & (g[:, 2] >= 100) & (g[:, 2] < 1000)).sum() >= 1
    ap = want["ap"]
    for a in range(3):
        for b in range(a + 1, 3):
            assert not np.array_equal(ap[a], ap[b], equal_nan=True)
    assert int(np.isfinite(ap).all(axis=(0, 2)).sum()) >= 3
    # the instance at the bound: every pixel 2561 under baseline 0.25, fx 2000 is 50.0 exactly, and `<=` keeps it
    exact = np.flatnonzero(big & dense & (t[:, 0] == 50.0))
    assert len(exact) >= 1
    assert distance_ref.camera(0) == (0.25, 2000.0)
    assert float(distances.pixel_distance(2561, 0.25, 2000.0)) == 50.0
    row = exact[0]
    assert row < len(_rec("star16")["gt_table"]) and t[row, 1] == 1.0
    lab, inst = int(g[row, 1]), int(g[row, 0])
    with_it = _evaluator(True)
    moved = _evaluator(True)
    moved.gt_dists[0] = moved.gt_dists[0].copy()
    moved.gt_dists[0][row, 0] = np.nextafter(50.0, np.inf)
    assert inst >= 1000 and il.LABEL_IDS.index(lab) >= 0
    a, b = with_it.ap_matrix(), moved.ap_matrix()
    assert np.array_equal(a[:2], b[:2], equal_nan=True) and not np.array_equal(a[2], b[2], equal_nan=True)


def test_the_disparity_helper_reproduces_the_recorded_tables():
    """The recorded tables are np.median on the helper's images; the kernel's integers map onto them bit for bit."""
    want = _rec("dist_set")
    for index, c in enumerate(CASES[:2]):
        r = _rec(c)
        disp = distance_ref.disparity(r["gt_ids"], index)
        assert disp.dtype == np.uint16 and disp.shape == (1024, 2048) and (disp == 0).any()
        cam = distance_ref.camera(index)
        assert np.array_equal(distance_ref.host_distances(r["gt_ids"], disp, r["gt_table"][:, 0], cam),
                              want["dist_%s" % c])
        raw = distance_ref.median_counts(r["gt_ids"], disp, r["gt_table"][:, 0])
        assert np.array_equal(raw[:, 0], r["gt_table"][:, 2])
        assert np.array_equal(distances.table_from_counts(raw, cam), want["dist_%s" % c])


def test_summarize_reproduces_the_reference_with_distances():
    assert_golden(_evaluator(True).summarize())


def test_the_table_matches_line_for_line():
    want = _rec("dist_set")
    res = _evaluator(True).summarize()
    text = il.format_results(res)
    assert text.split("\n") == [str(v) for v in want["table_lines"]][:len(text.split("\n"))]
    assert all(v == "" for v in want["table_lines"][len(text.split("\n")):])
    assert len(text.split("\n")[1]) == 90 and "AP_50m" in text and "AP_100m" in text and "AP_50%50m" in text


def test_without_distances_nothing_changes():
    ev = _evaluator(False)
    res = ev.summarize()
    want = _rec("set")
    assert res["resultApMatrix"].shape == (1, 8, 10)
    np.testing.assert_allclose(res["resultApMatrix"], want["ap"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(res["allAp"], float(want["all_ap"]), rtol=0, atol=1e-12)
    assert sorted(res) == ["allAp", "allAp50%", "classes", "resultApMatrix"]
    assert all(sorted(c) == ["ap", "ap50%"] for c in res["classes"].values())
    assert np.array_equal(_evaluator(True).ap_matrix()[0], res["resultApMatrix"][0], equal_nan=True)
    js = il.results_json(res)
    assert sorted(js) == ["averages", "instLabels", "minRegionSizes", "overlaps", "resultApMatrix"]
    assert len(il.format_results(res).split("\n")[1]) == 50


def test_results_json_with_distances_is_finite_json():
    js = il.results_json(_evaluator(True).summarize())
    assert js["distanceThresholds"] == [None, 100.0, 50.0] and js["minStereoDensities"] == [None, 0.5, 0.5]
    assert js["minRegionSizes"] == [100, 1000, 1000] and np.asarray(js["resultApMatrix"], float).shape == (3, 8, 10)
    for k in ("allAp50m", "allAp100m", "allAp50%50m"):
        assert k in js["averages"]
    assert set(js["averages"]["classes"]["car"]) == {"ap", "ap50%", "ap50m", "ap100m", "ap50%50m"}


def test_an_evaluator_refuses_the_wrong_mode():
    r = _rec("star16")
    args = (r["gt_table"], r["label_id"], r["conf"], r["pixel_count"], r["void_intersection"], _recorded_inter(r))
    with pytest.raises(ValueError, match="gt_dist"):
        il.InstanceLevelEvaluator(distances=True).add_counts(*args)
    with pytest.raises(ValueError, match="distances=False"):
        il.InstanceLevelEvaluator().add_counts(*args, gt_dist=np.zeros((len(r["gt_table"]), 2)))
    ev = il.InstanceLevelEvaluator(distances=True)
    with pytest.raises(ValueError, match=r"\[9, 2\]"):
        ev.add_counts(*args, gt_dist=np.zeros((3, 2)))
    assert not ev.images and not ev.gt_dists


def test_group_and_outside_count_twice():
    """The unmatched-prediction rule: a group that is also outside the setting gives its intersection twice."""
    table = np.array([[26, 26, 5000], [26001, 26, 5000]])
    dist = np.array([[120.0, 1.0], [20.0, 1.0]])
    counts = ([26, 26], [0.8, 0.9], [5000, 400], [0, 0], np.array([[0, 5000], [210, 0]]))
    ev = il.InstanceLevelEvaluator(distances=True)
    ev.add_counts(table, *counts, gt_dist=dist)
    ap = ev.ap_matrix()
    # The second prediction has 210 of its 400 pixels on the group and matches nothing.  First setting: the group
    # counts once, share 0.525: dropped at 0.50 (AP 1), a false positive ABOVE the match from 0.55 on: precision
    # [0.5, 0, 1] at recall [1, 0, 0], recall steps [0.5, 0.5, 0], AP 0.25.  100 m setting: the group is also beyond
    # the bound, so it counts twice, share 1.05: dropped at every threshold.
    assert ap[0, 2, 0] == 1.0 and (ap[0, 2, 1:] == 0.25).all() and (ap[1, 2] == 1.0).all() and (ap[2, 2] == 1.0).all()
    # the same group within both bounds counts once in every setting
    ev = il.InstanceLevelEvaluator(distances=True)
    ev.add_counts(table, *counts, gt_dist=np.array([[20.0, 1.0], [20.0, 1.0]]))
    ap = ev.ap_matrix()
    assert np.array_equal(ap[1], ap[0], equal_nan=True) and np.array_equal(ap[2], ap[0], equal_nan=True)
    assert (ap[0, 2, 1:] == 0.25).all()


def test_the_boundary_evaluator_inherits_the_settings():
    """With every band the whole mask, boundary IoU is mask IoU: the Boundary AP matrix under the three settings is the
    reference's AP matrix; the printed table keeps its columns."""
    from centerpoly_amd.datasets.evaluation import boundary as bd
    want = _rec("dist_set")
    ev = bd.BoundaryEvaluator(il.CITYSCAPES, distances=True)
    for c in CASES:
        r = _rec(c)
        inter = _recorded_inter(r)
        ev.add_counts(r["gt_table"], r["label_id"], r["conf"], r["pixel_count"], r["void_intersection"], inter,
                      r["pixel_count"], r["gt_table"][:, 2], inter, gt_dist=want["dist_%s" % c])
    res = ev.summarize()
    for k in ("resultBoundaryApMatrix", "resultApMatrix"):
        assert res[k].shape == (3, 8, 10)
        np.testing.assert_allclose(res[k], want["ap"], rtol=0, atol=1e-12, equal_nan=True)
    np.testing.assert_allclose(res["allBoundaryAp"], want["averages"][0], rtol=0, atol=1e-12)
    assert "bAP_50%" in bd.format_results(res, il.CITYSCAPES) and "50m" not in bd.format_results(res, il.CITYSCAPES)
    r = _rec("star16")
    with pytest.raises(ValueError, match="gt_dist"):
        ev.add_counts(r["gt_table"], [], [], [], [], np.zeros((0, 9)), [], r["gt_table"][:, 2], np.zeros((0, 9)))


# ------------------------------------------------------------------------------------------- host pieces --
def test_distance_formula():
    b, fx = 0.209313, 2262.52
    d = distances.pixel_distance(np.array([1, 2, 65535]), b, fx)
    assert d.dtype == np.float64 and np.isinf(d[0]) and d[0] > 0
    assert d[1] == (b * fx) / (1.0 / 256.0) and d[2] == (b * fx) / (65534.0 / 256.0)
    assert np.array_equal(d, distance_ref.pixel_distance(np.array([1, 2, 65535]), b, fx))
    # p == 0 never reaches the formula: it is "no measurement" (valid == 0 gives +inf, density 0)
    t = distances.table_from_counts(np.array([[10, 0, 0, 0], [10, 4, 300, 400], [8, 3, 1, 1], [0, 0, 0, 0]]), (b, fx))
    assert np.isinf(t[0, 0]) and t[0, 1] == 0.0 and np.isinf(t[2, 0]) and np.isinf(t[3, 0]) and t[3, 1] == 0.0
    lo, hi = (b * fx) / (299.0 / 256.0), (b * fx) / (399.0 / 256.0)
    assert t[1, 0] == 0.5 * (lo + hi) and t[1, 1] == 0.4 and lo != hi         # an even count, two different middles
    ids = np.array([[5, 5, 5, 5, 7]], np.uint16)
    disp = np.array([[300, 0, 400, 500, 0]], np.uint16)
    raw = distance_ref.median_counts(ids, disp, [5, 7, 9])
    assert raw.tolist() == [[4, 3, 400, 400], [1, 0, 0, 0], [0, 0, 0, 0]]
    assert np.array_equal(distances.table_from_counts(raw, (b, fx)),
                          distance_ref.host_distances(ids, disp, [5, 7, 9], (b, fx)))


def test_readers_and_their_refusals(tmp_path):
    from PIL import Image
    disp = np.array([[0, 1, 2561], [65535, 24, 3]], np.uint16)
    Image.fromarray(disp).save(str(tmp_path / "a_disparity.png"))
    Image.fromarray(disp.astype(np.int32)).save(str(tmp_path / "b_disparity.tif"))
    for f in ("a_disparity.png", "b_disparity.tif"):
        got = distances.read_disparity(str(tmp_path / f))
        assert got.dtype == np.uint16 and np.array_equal(got, disp)
    Image.fromarray(np.array([[70000, 1]], np.int32)).save(str(tmp_path / "c.tif"))
    with pytest.raises(ValueError, match="c.tif"):
        distances.read_disparity(str(tmp_path / "c.tif"))
    Image.fromarray(np.zeros((2, 2, 3), np.uint8)).save(str(tmp_path / "rgb.png"))
    with pytest.raises(ValueError, match="rgb.png"):
        distances.read_disparity(str(tmp_path / "rgb.png"))

    def cam(name, obj):
        with open(str(tmp_path / name), "w") as f:
            json.dump(obj, f)
        return str(tmp_path / name)
    assert distances.read_camera(cam("ok_camera.json", {"extrinsic": {"baseline": 0.209313, "pitch": 0.03},
                                                        "intrinsic": {"fx": 2262.52, "fy": 2265.3}})) \
        == (0.209313, 2262.52)
    for name, obj in (("nofx.json", {"extrinsic": {"baseline": 0.2}, "intrinsic": {}}),
                      ("noext.json", {"intrinsic": {"fx": 2000}}),
                      ("zero.json", {"extrinsic": {"baseline": 0.0}, "intrinsic": {"fx": 2000}}),
                      ("neg.json", {"extrinsic": {"baseline": 0.2}, "intrinsic": {"fx": -1}}),
                      ("text.json", {"extrinsic": {"baseline": "0.2"}, "intrinsic": {"fx": 2000}})):
        with pytest.raises(ValueError, match=name):
            distances.read_camera(cam(name, obj))
    with open(str(tmp_path / "inf.json"), "w") as f:
        f.write('{"extrinsic": {"baseline": Infinity}, "intrinsic": {"fx": 2000}}')
    with pytest.raises(ValueError, match="inf.json"):
        distances.read_camera(str(tmp_path / "inf.json"))


def test_find_files(tmp_path):
    d, c = tmp_path / "disparity" / "val" / "frankfurt", tmp_path / "camera" / "val" / "frankfurt"
    os.makedirs(str(d))
    os.makedirs(str(c))
    for key in ("frankfurt_000000_000294", "frankfurt_000000_000576"):
        open(str(d / (key + "_disparity.png")), "w").close()
    open(str(c / "frankfurt_000000_000294_camera.json"), "w").close()
    open(str(c / "notes.txt"), "w").close()
    files = distances.find_files(str(tmp_path / "disparity"), str(tmp_path / "camera"))
    assert files == {"frankfurt_000000_000294": (str(d / "frankfurt_000000_000294_disparity.png"),
                                                 str(c / "frankfurt_000000_000294_camera.json")),
                     "frankfurt_000000_000576": (str(d / "frankfurt_000000_000576_disparity.png"), None)}
    assert distances.frame_files(files, "frankfurt_000000_000294")[1].endswith("_camera.json")
    with pytest.raises(FileNotFoundError, match="frankfurt_000000_000576_camera.json"):
        distances.frame_files(files, "frankfurt_000000_000576")
    with pytest.raises(FileNotFoundError, match="munich_1_disparity.png"):
        distances.frame_files(files, "munich_1")
    os.makedirs(str(tmp_path / "disparity" / "val" / "other"))
    open(str(tmp_path / "disparity" / "val" / "other" / "frankfurt_000000_000294_disparity.png"), "w").close()
    with pytest.raises(ValueError, match="two disparity files for frankfurt_000000_000294"):
        distances.find_files(str(tmp_path / "disparity"), str(tmp_path / "camera"))
    with pytest.raises(FileNotFoundError):
        distances.find_files(str(tmp_path / "nowhere"), str(tmp_path / "camera"))


def test_eval_images_names_a_frame_without_its_files(tmp_path):
    import types

    from centerpoly_amd.datasets import eval_images
    names = {1: "frankfurt_000000_000294_leftImg8bit.png", 2: "frankfurt_000000_000576_leftImg8bit.png"}
    ds = types.SimpleNamespace(images=[1, 2], coco=types.SimpleNamespace(
        loadImgs=lambda ids: [{"file_name": names[ids[0]]}]))
    files = {"frankfurt_000000_000294": ("a_disparity.png", "a_camera.json"),
             "frankfurt_000000_000576": ("b_disparity.png", None)}
    with pytest.raises(FileNotFoundError, match="frankfurt_000000_000576_camera.json below --camera_dir"):
        eval_images.EvalImages(ds, {}, il.CITYSCAPES, files)
    files["frankfurt_000000_000576"] = ("b_disparity.png", "b_camera.json")
    assert len(eval_images.EvalImages(ds, {}, il.CITYSCAPES, files)) == 2


def test_options(tmp_path, capsys):
    from centerpoly_amd.opts import opts
    d = str(tmp_path)
    opt = opts().parse(["polydet"])
    assert opt.disparity_dir == "" and opt.camera_dir == ""
    opt = opts().parse(["polydet", "--dataset", "cityscapes", "--gt_dir", d, "--disparity_dir", d, "--camera_dir", d])
    assert opt.disparity_dir == d and opt.camera_dir == d
    for args, said in ((["--gt_dir", d, "--disparity_dir", d], "--disparity_dir and --camera_dir come together"),
                       (["--gt_dir", d, "--camera_dir", d], "--disparity_dir and --camera_dir come together"),
                       (["--disparity_dir", d, "--camera_dir", d], "--disparity_dir needs --gt_dir"),
                       (["--dataset", "kitti_poly", "--gt_dir", d, "--disparity_dir", d, "--camera_dir", d],
                        "no disparity convention"),
                       (["--dataset", "IDD", "--gt_dir", d, "--disparity_dir", d, "--camera_dir", d],
                        "no disparity convention")):
        with pytest.raises(SystemExit):
            opts().parse(["polydet"] + (args if "--dataset" in args else ["--dataset", "cityscapes"] + args))
        assert said in capsys.readouterr().err


def test_abi_without_gpu():
    """cp_segment_medians refuses what it cannot do before any device work: callable with null device pointers."""
    L = _C.lib()
    assert L.cp_abi_version() == 3 and _C.ABI_VERSION == 3
    assert "cp_segment_medians" in _C.EXPORTS and "cp_segment_medians_workspace_bytes" in _C.EXPORTS
    need = L.cp_segment_medians_workspace_bytes(1024, 1024, 2048)
    assert need >= 65536 * 2 + 1024 * (258 + 512) * 4
    assert L.cp_segment_medians_workspace_bytes(8, 1024, 2048) < need
    call = lambda G, H, W, ws: L.cp_segment_medians(None, None, H, W, None, G, None, None, ws, None)   # noqa: E731
    assert call(-1, 8, 8, need) == -1
    assert call(1025, 8, 8, need) == -2
    assert call(8, 0, 8, need) == -1 and call(8, 8, 0, need) == -1 and call(8, -3, 8, need) == -1
    assert call(8, 65536, 32768, need) == -2                                # H * W = 2^31
    assert call(0, 8, 8, 0) == 0                                            # G == 0: nothing to do
    p = ctypes.c_void_p(256)                                                # never dereferenced
    short = L.cp_segment_medians_workspace_bytes(8, 8, 8) - 1
    assert L.cp_segment_medians(p, p, 8, 8, p, 8, p, p, short, None) == -3
    assert call(8, 8, 8, short) == -3
    assert L.cp_segment_medians(None, p, 8, 8, p, 8, p, p, need, None) == -1    # a null image
    assert L.cp_segment_medians(p, p, 8, 8, p, 8, p, ctypes.c_void_p(260), need, None) == -1   # workspace alignment

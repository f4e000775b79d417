"""cp_segment_medians on the GPU against numpy (np.sort per segment: the four integers are exact), the distances made
of them against the recorded tables, and AP 100 m / AP 50 m end to end: score_instances_device with distances on the
four fixtures against the reference evaluator's matrix, and test.py with --disparity_dir / --camera_dir."""
import json
import os
import types

import numpy as np
import pytest

import distance_ref
from centerpoly_amd import _C
from centerpoly_amd.datasets.evaluation import distances
from centerpoly_amd.datasets.evaluation import instance_level as il
from test_distance_ap_cpu import CASES, _rec, assert_golden

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def _offset_dev(arr):
    """The uint16 image on the device, one element into its buffer: an unaligned base pointer."""
    import torch
    buf = torch.empty((arr.size + 1,), dtype=torch.int16, device="cuda")
    buf[1:] = torch.from_numpy(np.ascontiguousarray(arr).view(np.int16).reshape(-1))
    return buf[1:].view(arr.shape)


def _dev(arr):
    import torch
    return torch.from_numpy(np.ascontiguousarray(arr).view(np.int16)).cuda()


def _medians(ids_dev, disp_dev, seg_ids):
    return distances.segment_medians(ids_dev, seg_ids, disp_dev).cpu().numpy().astype(np.int64)


def _case_37x53():
    """Every path of the selection on an image of unaligned rows with a tail; see the assertions for what is in it."""
    H, W = 37, 53
    ids = np.full((H, W), 9, np.uint16)
    val = np.full((H, W), 777, np.uint16)
    rng = np.random.RandomState(5)
    ids[0:4, 0:10] = 100                     # no valid pixel
    val[0:4, 0:10] = 0
    ids[0:4, 10:20] = 101                    # one valid pixel
    val[0:4, 10:20] = 0
    val[2, 13] = 4242
    ids[4:6, 0:3] = 102                      # an even count, the middles on both sides of a high-byte boundary
    val[4:6, 0:3] = np.array([[0x1200, 0x12fe, 0x12ff], [0x1300, 0x1301, 0x2000]], np.uint16)
    ids[6:9, 0:5] = 103                      # an odd count (15) of distinct values, shuffled
    val[6:9, 0:5] = rng.permutation(np.arange(15) * 1000 + 3).reshape(3, 5).astype(np.uint16)
    ids[10:20, 20:53] = 104                  # all equal, running into the last column
    val[10:20, 20:53] = 2561
    ids[20:30, 0:40] = 105                   # the values 1 and 65535, random ones and holes in between
    v = rng.randint(0, 65536, (10, 40))
    v[rng.random_sample((10, 40)) < 0.2] = 0
    v[0, 0], v[9, 39] = 1, 65535
    val[20:30, 0:40] = v.astype(np.uint16)
    ids[30:37, 45:53] = 106                  # the image's last pixel, only 1 and 65535: an even count of each
    val[30:37, 45:53] = np.where(np.arange(56).reshape(7, 8) % 2 == 0, 1, 65535).astype(np.uint16)
    seg = [100, 101, 102, 555, 103, 70000, 104, 105, 106, 9, -1]
    return ids, val, seg


def test_every_path_on_37x53():
    ids, val, seg = _case_37x53()
    want = distance_ref.median_counts(ids, val, seg)
    got = _medians(_offset_dev(ids), _offset_dev(val), seg)
    assert np.array_equal(got, want), (got.tolist(), want.tolist())
    by = dict(zip(seg, want.tolist()))
    assert by[100] == [40, 0, 0, 0] and by[101] == [40, 1, 4242, 4242]
    assert by[102] == [6, 6, 0x12ff, 0x1300] and by[103][1] == 15 and by[103][2] == by[103][3] == 7003
    assert by[555] == by[70000] == by[-1] == [0, 0, 0, 0]
    assert by[104] == [330, 330, 2561, 2561] and by[106] == [56, 56, 1, 65535]
    assert by[105][0] == 400 and 0 < by[105][1] < 400
    # one segment that covers the whole image
    whole = np.full_like(ids, 26001)
    want = distance_ref.median_counts(whole, val, [26001])
    assert want[0, 0] == 37 * 53
    assert np.array_equal(_medians(_offset_dev(whole), _offset_dev(val), [26001]), want)


def test_1024_segments_of_random_ids():
    """G = 1024, more than either LDS table holds: the global-atomic regime of both passes."""
    rng = np.random.RandomState(8)
    seg = rng.permutation(65536)[:1024]
    ids = seg[rng.randint(0, 1100, (64, 1024)) % 1024].astype(np.uint16)
    ids[rng.random_sample(ids.shape) < 0.1] = 7                               # pixels of no segment
    val = rng.randint(0, 65536, (64, 1024)).astype(np.uint16)
    val[rng.random_sample(val.shape) < 0.3] = 0
    val[:, 512:] = (val[:, 512:] % 300 + 5000)                               # few high bytes: the two ranks share one
    want = distance_ref.median_counts(ids, val, seg)
    assert (want[:, 1] > 0).sum() > 1000 and (want[:, 2] != want[:, 3]).any()
    assert np.array_equal(_medians(_dev(ids), _dev(val), seg), want)
    # between the two LDS bounds (30 < G <= 59): pass 1 in LDS, pass 2 with global atomics
    assert np.array_equal(_medians(_dev(ids), _dev(val), seg[:45]), want[:45])


def test_no_segment_is_a_no_op():
    import torch
    ids, val, _ = _case_37x53()
    out = distances.segment_medians(_dev(ids), [], _dev(val))
    torch.cuda.synchronize()
    assert tuple(out.shape) == (0, 4)
    table, raw = distances.instance_distances(_dev(ids), [], val, (0.25, 2000.0))
    assert table.shape == (0, 2) and raw.shape == (0, 4)


def test_a_scene_gives_the_recorded_distances_bit_for_bit():
    """The first fixture's id image with its helper disparity: integers equal to np.sort's, and after the host mapping
    the [G, 2] table of np.median that the golden records.  The disparity goes in as a host array here."""
    r = _rec("star16")
    disp = distance_ref.disparity(r["gt_ids"], 0)
    seg = r["gt_table"][:, 0]
    table, raw = distances.instance_distances(_dev(r["gt_ids"]), seg, disp, distance_ref.camera(0))
    assert np.array_equal(raw, distance_ref.median_counts(r["gt_ids"], disp, seg))
    assert np.array_equal(raw[:, 0], r["gt_table"][:, 2])
    assert table.dtype == np.float64 and np.array_equal(table, _rec("dist_set")["dist_star16"])
    assert (table[:, 0] == 50.0).any()


def test_one_segment_and_one_bucket_everywhere():
    """The contention shape: one id on every pixel of 1024 x 2048, every value in one high byte."""
    rng = np.random.RandomState(3)
    ids = np.full((1024, 2048), 26001, np.uint16)
    val = (0x2a00 + rng.randint(0, 256, ids.shape)).astype(np.uint16)
    want = distance_ref.median_counts(ids, val, [26001, 26002])
    assert want[0, 0] == want[0, 1] == 1024 * 2048 and want[0, 2] >> 8 == 0x2a
    assert np.array_equal(_medians(_dev(ids), _dev(val), [26001, 26002]), want)


# ------------------------------------------------------------------------------------------- end to end --
def _cityscapes(name):
    """(data set, rows [R, 2N + 7]) of a writer fixture, as test_boundary makes them."""
    from centerpoly_amd.datasets.dataset.polygons import CITYSCAPES
    z = np.load(os.path.join(HERE, "golden", "writer_%s.npz" % name), allow_pickle=False)
    det = {c: z["det_%d" % c] for c in sorted(int(k[4:]) for k in z.files if k.startswith("det_"))}
    rows = [np.concatenate([r[:, :5], np.full((len(r), 1), c - 1, np.float32), r[:, 5:]], axis=1)
            for c, r in sorted(det.items())]
    ds = CITYSCAPES.__new__(CITYSCAPES)
    ds.opt = types.SimpleNamespace(thresh=0.05)
    return ds, np.ascontiguousarray(np.concatenate(rows, axis=0), np.float32)


def test_score_instances_device_gives_the_reference_matrix():
    import torch
    ev, plain = il.InstanceLevelEvaluator(distances=True), il.InstanceLevelEvaluator()
    want = _rec("dist_set")
    for index, c in enumerate(CASES):
        ds, rows = _cityscapes(c)
        r = _rec(c)
        rows_dev = torch.from_numpy(rows).cuda()
        disp = distance_ref.disparity(r["gt_ids"], index)
        res = ds.score_instances_device(rows_dev, r["gt_ids"], evaluator=ev,
                                        distances=(disp, distance_ref.camera(index)))
        res0 = ds.score_instances_device(rows_dev, r["gt_ids"], evaluator=plain)
        assert set(res) - set(res0) == {"gt_dist", "gt_dist_raw"}
        for k, v in res0.items():
            assert np.array_equal(np.asarray(v), np.asarray(res[k])), k
        assert np.array_equal(res["gt_dist"], want["dist_%s" % c])
        assert np.array_equal(res["gt_dist_raw"], distance_ref.median_counts(r["gt_ids"], disp, r["gt_table"][:, 0]))
    assert_golden(ev.summarize())
    # without distances: the tables and the matrix of before
    res0 = plain.summarize()
    assert res0["resultApMatrix"].shape == (1, 8, 10) and sorted(res0) == ["allAp", "allAp50%", "classes",
                                                                            "resultApMatrix"]
    np.testing.assert_allclose(res0["resultApMatrix"], _rec("set")["ap"], rtol=0, atol=1e-12)
    # a distance table for an evaluator that scores none, and the reverse
    ds, rows = _cityscapes("star16")
    r = _rec("star16")
    with pytest.raises(ValueError, match="distances=False"):
        ds.score_instances_device(torch.from_numpy(rows).cuda(), r["gt_ids"], evaluator=il.InstanceLevelEvaluator(),
                                  distances=(distance_ref.disparity(r["gt_ids"], 0), distance_ref.camera(0)))
    with pytest.raises(ValueError, match="gt_dist"):
        ds.score_instances_device(torch.from_numpy(rows).cuda(), r["gt_ids"],
                                  evaluator=il.InstanceLevelEvaluator(distances=True))


def _distance_files(tmp, cases):
    """The helper's disparity images and cameras of `cases` as Cityscapes files: (disparity_dir, camera_dir)."""
    from PIL import Image
    disp_dir, cam_dir = os.path.join(tmp, "disparity"), os.path.join(tmp, "camera")
    for d in (disp_dir, cam_dir):
        os.makedirs(os.path.join(d, "val", "frankfurt"))
    for index, c in enumerate(cases):
        Image.fromarray(distance_ref.disparity(_rec(c)["gt_ids"], index)).save(
            os.path.join(disp_dir, "val", "frankfurt", "frankfurt_%s_disparity.png" % c), compress_level=1)
        baseline, fx = distance_ref.camera(index)
        with open(os.path.join(cam_dir, "val", "frankfurt", "frankfurt_%s_camera.json" % c), "w") as f:
            json.dump({"extrinsic": {"baseline": baseline}, "intrinsic": {"fx": fx}}, f)
    return disp_dir, cam_dir


def test_run_eval_scores_the_reference_matrix_from_files(tmp_path, capsys):
    """CITYSCAPES.run_eval with --disparity_dir / --camera_dir on the four fixtures: add_image reads the files."""
    from test_instance_ap import _dataset
    disp_dir, cam_dir = _distance_files(str(tmp_path), CASES)
    ds, results = _dataset(tmp_path, ["--no_mask_files", "--disparity_dir", disp_dir, "--camera_dir", cam_dir])
    ap = ds.run_eval(results, str(tmp_path / "exp"))
    assert_golden(ds.last_summary)
    assert ap == ds.last_summary["allAp"] and "AP_100m" in capsys.readouterr().out
    os.remove(os.path.join(disp_dir, "val", "frankfurt", "frankfurt_small16_disparity.png"))
    with pytest.raises(FileNotFoundError, match="frankfurt_small16_disparity.png"):
        ds.run_eval(results, str(tmp_path / "exp2"))


def test_driver_scores_the_distance_columns(tmp_path, capsys):
    """test.py --disparity_dir --camera_dir on a two-image Cityscapes tree: the five-column table, the averages in the
    returned dict and the JSON, equal to evaluate_result_dir on the files it wrote.  (That a frame without its files
    stops the run when the image list is made is test_distance_ap_cpu's, on EvalImages.)"""
    import importlib.util

    from centerpoly_amd.opts import opts
    from test_boundary import _cityscapes_set
    root = os.path.dirname(HERE)
    spec = importlib.util.spec_from_file_location("centerpoly_test_driver", os.path.join(root, "test.py"))
    driver = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(driver)
    args = _cityscapes_set(str(tmp_path))
    disp_dir, cam_dir = _distance_files(str(tmp_path), ("star16", "mixed32"))
    opt = opts().parse(args + ["--disparity_dir", disp_dir, "--camera_dir", cam_dir])
    opt.save_dir = str(tmp_path / "exp")
    out = driver.run_test(opt)
    text = capsys.readouterr().out
    assert "AP_100m" in text and "AP_50%50m" in text and "#" * 90 in text
    ev = out["dataset"].last_evaluator
    assert ev.distances and len(ev.gt_dists) == 2
    assert np.array_equal(ev.gt_dists[0], _rec("dist_set")["dist_star16"])
    assert np.array_equal(ev.gt_dists[1], _rec("dist_set")["dist_mixed32"])
    js = json.load(open(os.path.join(opt.save_dir, "results", "evaluationResults",
                                     "resultInstanceLevelSemanticLabeling.json")))
    assert js["distanceThresholds"] == [None, 100.0, 50.0] and np.asarray(js["resultApMatrix"], float).shape == (3, 8, 10)
    files = il.evaluate_result_dir(os.path.join(opt.save_dir, "results"), sorted(il.find_gt_files(opt.gt_dir).values()),
                                   disparity_dir=disp_dir, camera_dir=cam_dir)
    assert out["ap"] == files["allAp"]
    for k in ("allAp100m", "allAp50m", "allAp50%50m"):
        np.testing.assert_allclose(out[k], files[k], rtol=0, atol=0, equal_nan=True)
        np.testing.assert_allclose(js["averages"][k], files[k], rtol=0, atol=0, equal_nan=True)
    np.testing.assert_allclose(files["resultApMatrix"], ev.ap_matrix(), rtol=0, atol=1e-12, equal_nan=True)

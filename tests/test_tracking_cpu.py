"""Instance tracking without a GPU: the host statement (tests/golden/tracking_host.py) against hand-worked numbers, the
scoring rule of evaluation/tracking.py on pair tables against the host statement, the options, and the result files."""
import contextlib
import io
import math
import os

import numpy as np
import pytest

import tracking_host as host

CAR = 26
H, W = 8, 12


def _rect(image, rows, cols, value):
    image[rows[0]:rows[1] + 1, cols[0]:cols[1] + 1] = value
    return image


def swap_sequence():
    """Three frames of 8 x 12, label 26 (car), multiplier 1000: [(gt ids, index, n)], every instance live.
      frame 0  objects A = 26001 at rows 1..4 x cols 0..3 and B = 26002 at rows 1..4 x cols 7..10 (16 px each);
               instance 0 is A's rectangle, instance 1 is B's.
      frame 1  A moves to cols 1..4, B stays; instance 0 = A's rectangle, instance 1 = rows 1..4 x cols 7..9 (12 px).
      frame 2  the ground truth says the two have changed places: A at cols 7..10, B at cols 1..4; a third object
               C = 26003 at rows 6..7 x cols 0..5 (12 px) is not detected; instance 0 = rows 1..4 x cols 1..4, instance
               1 = rows 1..4 x cols 7..9, instance 2 = rows 6..7 x cols 8..11 (8 px) lies on no object."""
    frames = []
    for a_cols, b_cols, extra in (((0, 3), (7, 10), False), ((1, 4), (7, 10), False), ((7, 10), (1, 4), True)):
        gt = np.zeros((H, W), np.uint16)
        _rect(gt, (1, 4), a_cols, 26001)
        _rect(gt, (1, 4), b_cols, 26002)
        frames.append([gt, None, 2])
    frames[2][0] = _rect(frames[2][0], (6, 7), (0, 5), 26003)
    for f, cols0, cols1 in ((0, (0, 3), (7, 10)), (1, (1, 4), (7, 9)), (2, (1, 4), (7, 9))):
        index = np.full((H, W), 255, np.uint8)
        _rect(index, (1, 4), cols0, 0)
        _rect(index, (1, 4), cols1, 1)
        frames[f][1] = index
    _rect(frames[2][1], (6, 7), (8, 11), 2)
    frames[2][2] = 3
    return [tuple(f) for f in frames]


def test_host_statement_on_the_swap_sequence_by_hand():
    """Tracker (iou_thresh 0.3, max_age 0):
      frame 0  nothing remembered: instance 0 -> slot 0, track 1; instance 1 -> slot 1, track 2; next_id 3.
      frame 1  slot 0 remembers cols 0..3: instance 0 (cols 1..4) shares 3 columns x 4 rows = 12 px, union 16 + 16 - 12 =
               20, IoU 0.6; slot 1 remembers cols 7..10: instance 1 (cols 7..9) shares 12 px, union 16, IoU 0.75.  Both
               above 0.3: 0.75 is matched first, then 0.6.  No new track.
      frame 2  slot 0 remembers cols 1..4 = instance 0: 16 / 16; slot 1 remembers cols 7..9 = instance 1: 12 / 12;
               instance 2 overlaps nothing: slot 2, track 3, next_id 4.
    Scoring (IoU > 0.5):
      frame 0  A - instance 0 (track 1) IoU 1, B - instance 1 (track 2) IoU 1:                  TP 2, soft 2
      frame 1  A - instance 0 (track 1) IoU 1, B - instance 1 (track 2) IoU 12 / 16 = 0.75:      TP 2, soft 1.75
      frame 2  B - instance 0 (track 1) IoU 1, but B was track 2: IDS; A - instance 1 (track 2) IoU 0.75, but A was
               track 1: IDS; C unmatched: FN; instance 2 unmatched, none of it ignored: FP.       TP 2, soft 1.75
      TP 6, FP 1, FN 1, IDS 2, soft TP 5.5, |M| = 7:
      MOTSA = (6 - 1 - 2) / 7 = 3 / 7, sMOTSA = (5.5 - 1 - 2) / 7 = 2.5 / 7, MOTSP = 5.5 / 6."""
    tr = host.Tracker(H, W, 0.3, 0, 1000)
    mots = host.Mots(1000, (24, 25, CAR), 10000)
    want_inst = ([[0, 1, 0, 0, 1], [1, 2, 0, 0, 1]],
                 [[0, 1, 12, 20, 0], [1, 2, 12, 16, 0]],
                 [[0, 1, 16, 16, 0], [1, 2, 12, 12, 0], [2, 3, 0, 0, 1]])
    for t, (gt, index, n) in enumerate(swap_sequence()):
        out = tr.step(index, n, [CAR] * n, [1] * n)
        assert out["inst"].tolist() == want_inst[t]
        mots.add_frame("s", gt, index, n, [CAR] * n, [1] * n, out["inst"][:, 1])
    assert tr.next_id == 4 and tr.t == 3
    assert tr.slots[:4].tolist() == [[1, CAR, 0, 2, 3], [2, CAR, 0, 2, 3], [3, CAR, 2, 2, 1], [0, 0, 0, 0, 0]]
    assert out["ids"][1, 1] == 26001 and out["ids"][1, 7] == 26002 and out["ids"][6, 8] == 26003 and out["ids"][0, 0] == 0
    assert tr.mem[1, 1] == 0 and tr.mem[1, 9] == 1 and tr.mem[1, 10] == host.NONE and tr.mem[7, 11] == 2
    res = mots.results()
    car = res["per_class"][CAR]
    assert (car["tp"], car["fp"], car["fn"], car["ids"]) == (6, 1, 1, 2) and car["soft_tp"] == 5.5
    assert car["motsa"] == 3 / 7 and car["smotsa"] == 2.5 / 7 and car["motsp"] == 5.5 / 6
    assert res["all"]["motsa"] == 3 / 7 and res["all"]["smotsa"] == 2.5 / 7
    assert math.isnan(res["per_class"][24]["motsa"]) and math.isnan(res["per_class"][24]["motsp"])


def _one_pair(inter, mem_only, cur_only):
    pairs = np.zeros((host.T + 1, 2), np.int64)
    pairs[0, 0], pairs[0, 1], pairs[host.T, 0] = inter, mem_only, cur_only
    return pairs


def test_host_statement_at_the_threshold_boundary():
    """inter 3, union 3 + 3 + 4 = 10 at iou_thresh 0.3: 3.0 / 10.0 is the float64 0.3, matched.  inter 29, union
    29 + 30 + 41 = 100: 0.29 < 0.3, a new track."""
    slots = np.zeros((host.T, 5), np.int64)
    slots[0] = [7, CAR, 0, 4, 5]
    s, next_id, inst, assigned = host.associate(_one_pair(3, 3, 4), 1, [CAR], [1], slots, 8, 0.3, 0, 5)
    assert inst.tolist() == [[0, 7, 3, 10, 0]] and next_id == 8 and s[0].tolist() == [7, CAR, 0, 5, 6]
    s, next_id, inst, assigned = host.associate(_one_pair(29, 30, 41), 1, [CAR], [1], slots, 8, 0.3, 0, 5)
    assert inst.tolist() == [[1, 8, 0, 0, 1]] and next_id == 9
    assert s[0].tolist() == [0] * 5 and s[1].tolist() == [8, CAR, 5, 5, 1]      # the old track ends at max_age 0
    assert assigned[:2].tolist() == [0, 1]


def tie_tables():
    """Hand-made pair tables [257, n + 1] with equal IoUs as different fractions: (name, slots, pairs, n, thresh, inst).
      column  slots 0 (track 9) and 1 (track 4) both want instance 0: 2 / 6 against 3 / 9 (areas 3 and 7 against 5).
              Equal, so the smaller track id wins: slot 1; slot 0 is left and instance 0 is not new.
      row     slot 0 wants instances 0 and 1: 3 / 9 against 2 / 6 (area 5 against 7 and 3).  Equal, so the smaller k
              wins and instance 1 starts track 10 in slot 1.
      apart   slot 0 - instance 0 at 2 / 4 and slot 1 - instance 1 at 3 / 6, no conflict: both matched."""
    T = host.T
    slots = np.zeros((T, 5), np.int64)
    slots[0], slots[1] = [9, CAR, 0, 0, 1], [4, CAR, 0, 0, 1]
    column = np.zeros((T + 1, 2), np.int64)
    column[0], column[1] = [2, 1], [3, 4]
    one = np.zeros((T, 5), np.int64)
    one[0] = [9, CAR, 0, 0, 1]
    row = np.zeros((T + 1, 3), np.int64)
    row[0], row[T] = [3, 2, 0], [4, 1, 0]
    apart = np.zeros((T + 1, 3), np.int64)
    apart[0], apart[1], apart[T] = [2, 0, 1], [0, 3, 1], [1, 2, 0]
    return [("column", slots, column, 1, 0.3, [[1, 4, 3, 9, 0]]),
            ("row", one, row, 2, 0.3, [[0, 9, 3, 9, 0], [1, 10, 0, 0, 1]]),
            ("apart", slots, apart, 2, 0.5, [[0, 9, 2, 4, 0], [1, 4, 3, 6, 0]])]


def test_host_statement_orders_equal_ious_by_track_id_then_instance():
    for name, slots, pairs, n, thresh, want in tie_tables():
        s, next_id, inst, assigned = host.associate(pairs, n, [CAR] * n, [1] * n, slots, 10, thresh, 0, 1)
        assert inst.tolist() == want, name


def test_scoring_rule_of_the_package_on_host_tables():
    """evaluation/tracking.py's rule on pair tables (no device): the swap sequence, and a frame with an ignore region
    and a crowd id, against the host statement."""
    from centerpoly_amd.datasets.evaluation import instance_level as il
    from centerpoly_amd.datasets.evaluation import tracking as mots
    ev = mots.TrackingEvaluator(il.CITYSCAPES, 10000)
    want = host.Mots(1000, il.LABEL_IDS, 10000)
    tr = host.Tracker(H, W, 0.3, 0, 1000)
    frames = swap_sequence()
    gt3 = frames[2][0].copy()
    _rect(gt3, (6, 7), (8, 10), 10000)                    # instance 2: 6 of 8 px ignored -> no FP
    _rect(gt3, (0, 0), (0, 11), CAR)                      # a crowd row of cars
    frames.append((gt3, frames[2][1], 3))
    for gt, index, n in frames:
        track = tr.step(index, n, [CAR] * n, [1] * n)["inst"][:, 1]
        want.add_frame("s", gt, index, n, [CAR] * n, [1] * n, track)
        objects = sorted(set(int(v) for v in gt.reshape(-1) if v >= 1000 and v != 10000))
        row_of = np.full((65536,), 0xffff, np.int64)
        row_of[10000] = 0
        row_of[list(il.LABEL_IDS)] = 0
        row_of[objects] = 1 + np.arange(len(objects))
        G = len(objects)
        pairs = host.map_pairs(gt, index, G + 1, n, row_of)
        ev.add_table("s", objects, pairs, n, [CAR] * n, [1] * n, track)
    got, ref = ev.results(), want.results()
    assert ref["all"]["fp"] == 1 and ref["all"]["tp"] == 8 and ref["all"]["ids"] == 2 and ref["all"]["fn"] == 2
    for c in il.LABEL_IDS:
        for key in ("tp", "fp", "fn", "ids"):
            assert got["per_class"][c][key] == ref["per_class"][c][key], (c, key)
        for key in ("soft_tp", "motsa", "smotsa", "motsp"):
            a, b = got["per_class"][c][key], ref["per_class"][c][key]
            assert (math.isnan(a) and math.isnan(b)) or abs(a - b) <= 1e-12, (c, key)
    assert abs(got["all"]["smotsa"] - ref["all"]["smotsa"]) <= 1e-12
    text = ev.format_table(got)
    assert "sMOTSA" in text and "car" in text and text.splitlines()[-1].startswith("all")


def _parse(args):
    from centerpoly_amd.opts import opts
    with contextlib.redirect_stdout(io.StringIO()):
        return opts().parse(args)


def test_options_parse():
    opt = _parse(["polydet"])
    assert opt.track is False and opt.track_iou == 0.3 and opt.track_max_age == 0 and opt.track_ignore_id == 10000
    opt = _parse(["polydet", "--track", "--track_iou", "1", "--track_max_age", "3", "--dataset", "kitti_poly"])
    assert opt.track is True and opt.track_iou == 1.0 and opt.track_max_age == 3
    assert _parse(["polydet", "--track", "--debug", "2"]).track is True
    for bad in (["--track_iou", "0"], ["--track_iou", "nan"], ["--track_iou", "inf"], ["--track_iou", "1.5"],
                ["--track_max_age", "-1"], ["--track", "--dataset", "synthetic"], ["--track", "--debug", "3"]):
        with pytest.raises(SystemExit), contextlib.redirect_stderr(io.StringIO()):
            _parse(["polydet"] + bad)


def test_sequence_keys_and_track_png(tmp_path):
    from centerpoly_amd.datasets.evaluation import tracking as mots
    from centerpoly_amd.datasets.ground_truth import write_id_png
    assert mots.sequence_key("a/b/frankfurt_000001_000019_leftImg8bit.png") == "a/b/frankfurt_000001"
    assert mots.sequence_key("a/b/frankfurt_000001_000020_leftImg8bit.png") == "a/b/frankfurt_000001"
    assert mots.sequence_key("a/b/frankfurt_000002_000020_leftImg8bit.png") != mots.sequence_key("a/b/frankfurt_000001_000020.png")
    assert mots.sequence_key("drive7/000031.png") == "drive7/" != mots.sequence_key("drive8/000031.png")
    ids = np.zeros((5, 7), np.int32)
    ids[1:3, 1:4], ids[3:, 4:] = 26 * 1000 + 17, 24 * 1000 + 2
    path = str(tmp_path / "x_trackIds.png")
    write_id_png(path, ids, 16)
    index, labels, tracks = mots.index_of_track_png(path, 1000)
    assert labels.tolist() == [24, 26] and tracks.tolist() == [2, 17]
    assert index[1, 1] == 1 and index[4, 6] == 0 and index[0, 0] == 255 and int((index == 1).sum()) == 6


@pytest.mark.gpu
def test_evaluate_result_dir_on_written_files(tmp_path):
    """*_trackIds.png files written here, scored against ground-truth files: the counts and measures of the host
    statement (the pixel counting runs on the device, so this one needs it)."""
    import torch

    from centerpoly_amd.datasets.evaluation import instance_level as il
    from centerpoly_amd.datasets.evaluation import tracking as mots
    from centerpoly_amd.datasets.ground_truth import write_id_png
    pred_dir, gt_dir = str(tmp_path / "pred"), str(tmp_path / "gt" / "frankfurt")
    os.makedirs(pred_dir)
    os.makedirs(gt_dir)
    want = host.Mots(1000, il.LABEL_IDS, 10000)
    tr = host.Tracker(H, W, 0.3, 0, 1000)
    for f, (gt, index, n) in enumerate(swap_sequence()):
        out = tr.step(index, n, [CAR] * n, [1] * n)
        stem = "frankfurt_000000_%06d" % f
        write_id_png(os.path.join(gt_dir, stem + il.GT_SUFFIX), gt.astype(np.int32), 16)
        write_id_png(os.path.join(pred_dir, stem + "_leftImg8bit_trackIds.png"), out["ids"].astype(np.int32), 16)
        # the files hold the instances in ascending id order, which here is the slot order
        want.add_frame("s", gt, index, n, [CAR] * n, [1] * n, out["inst"][:, 1])
    res = mots.evaluate_result_dir(pred_dir, str(tmp_path / "gt"), torch.device("cuda"))
    ref = want.results()
    for key in ("tp", "fp", "fn", "ids"):
        assert res["all"][key] == ref["all"][key]
    for key in ("motsa", "smotsa", "motsp"):
        assert abs(res["all"][key] - ref["all"][key]) <= 1e-12
    assert (res["all"]["tp"], res["all"]["fp"], res["all"]["fn"], res["all"]["ids"]) == (6, 1, 1, 2)


def test_track_id_that_reaches_the_multiplier_is_refused_after_the_json(tmp_path):
    import json
    import types

    from centerpoly_amd.detectors import tracking
    maps = types.SimpleNamespace(table={"n": 1, "live": np.array([True]), "label": np.array([CAR]),
                                        "score": np.array([0.5], np.float32), "box": np.array([[0, 0, 1, 1]])},
                                 names={CAR: "car"}, canvas=(4, 3))
    ids = np.zeros((3, 4), np.int32)
    ids[:2, :2] = CAR * 256 + 255
    tracked = types.SimpleNamespace(table={"track_id": np.array([256]), "is_new": np.array([True])}, frame=7,
                                    multiplier=256, ids=ids)
    with pytest.raises(ValueError, match="frame 7"):
        tracking.save_tracks(maps, tracked, str(tmp_path), "f")
    assert json.load(open(str(tmp_path / "f_tracks.json")))["instances"][0]["track_id"] == 256
    assert not os.path.exists(str(tmp_path / "f_trackIds.png"))
    tracked.table["track_id"][0] = 255
    paths = tracking.save_tracks(maps, tracked, str(tmp_path), "f")
    from centerpoly_amd.datasets.evaluation import instance_level as il
    assert np.array_equal(il.read_gt_ids(paths[1]), ids)

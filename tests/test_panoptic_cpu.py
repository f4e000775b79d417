"""Panoptic evaluation without a GPU: the host restatement of cp_panoptic_pairs / cp_panoptic_match against the tables
and per-image statistics recorded from the reference's converter and evaluator (tests/golden/panoptic_*.npz,
gen_panoptic_golden.py), the evaluator's scores and table against the recorded set, and the options' refusals."""
import json
import os

import numpy as np
import pytest

import panoptic_host as host
from centerpoly_amd.datasets.evaluation import panoptic as pq

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = ["star16", "mixed32", "selfcross16", "small16", "odd37x53", "missed29x41", "edge31x47"]
P = pq.CITYSCAPES
REL = 1e-12


def rec(name):
    return np.load(os.path.join(HERE, "golden", "panoptic_%s.npz" % name), allow_pickle=False)


def gt_ids(name):
    z = rec(name)
    if "gt_ids" in z.files:
        return z["gt_ids"]
    if name == "missed29x41":
        return np.load(os.path.join(HERE, "golden", "pixel_level_%s.npz" % name), allow_pickle=False)["gt_ids"]
    return np.load(os.path.join(HERE, "golden", "instance_ap_%s.npz" % name), allow_pickle=False)["gt_ids"]


def recorded_set():
    with open(os.path.join(HERE, "golden", "panoptic_set.json")) as f:
        return json.load(f)


def close(a, b):
    return abs(a - b) <= REL * max(abs(a), abs(b))


def assert_results(got, want):
    """`want` may come from JSON (string keys); integers exact, scores within 1e-12 relative."""
    assert set(got) == set(want) == {"All", "Things", "Stuff", "per_class"}
    for group in ("All", "Things", "Stuff"):
        assert got[group]["n"] == want[group]["n"], group
        for k in ("pq", "sq", "rq"):
            assert close(got[group][k], want[group][k]), (group, k, got[group][k], want[group][k])
    assert sorted(int(k) for k in got["per_class"]) == sorted(int(k) for k in want["per_class"])
    mine = {int(k): v for k, v in got["per_class"].items()}
    for label, scores in want["per_class"].items():
        for k in ("pq", "sq", "rq"):
            assert close(mine[int(label)][k], scores[k]), (label, k)


@pytest.fixture(scope="module")
def restated():
    out = {}
    for name in CASES:
        z = rec(name)
        n = len(z["labels"])
        seg, pairs = host.panoptic_pairs(z["index"], n, gt_ids(name), 1000, 1000, P.L, P.flags)
        out[name] = (seg, pairs) + host.panoptic_match(seg, pairs, n, z["labels"], P.L, P.flags)
    return out


def test_host_restatement_reproduces_the_recorded_tables_and_stats(restated):
    for name in CASES:
        z = rec(name)
        seg, pairs, stat, iou, bad, match = restated[name]
        assert np.array_equal(seg, z["seg"]) and np.array_equal(pairs, z["pairs"]), name
        assert np.array_equal(stat, z["stat"]) and bad.tolist() == [0, 0], name
        assert all(close(a, b) for a, b in zip(iou, z["iou"])), name
        assert pairs.sum() == z["index"].size and (match > 0).sum() == stat[:, 0].sum()
    # the edge image: IoU exactly one half is no match, one pixel more is; the crowd saves slot 3; slot 4 (2 x == area)
    # and slot 0 are false positives; slot 7 owns nothing (rows: 7, 23, 26, 24001, 25001, 26001, 26002)
    assert restated["edge31x47"][0][1:, 0].tolist() == [7, 23, 26, 24001, 25001, 26001, 26002]
    assert restated["edge31x47"][5].tolist() == [0, 7, 4, 0, 0, 0, 5, -1]
    z = rec("edge31x47")
    assert z["stat"][26].tolist() == [1, 2, 1] and z["stat"][24].tolist() == [1, 1, 0] and z["stat"][7].tolist() == [0, 0, 1]
    assert 29001 in gt_ids("edge31x47") and 29001 not in z["seg"][:, 0]               # the caravan is VOID


def test_evaluator_reproduces_the_reference_scores(capsys):
    want = recorded_set()
    assert want["images"] == CASES
    ev = pq.PanopticEvaluator(P)
    for name in CASES:
        z = rec(name)
        ev.add_stats(z["stat"], z["iou"])
    got = ev.results()
    assert_results(got, want["result"])
    stat, iou, bad = ev.tables()
    for label, (tp, fp, fn, total) in want["stat"].items():
        assert stat[int(label)].tolist() == [tp, fp, fn] and close(iou[int(label)], total)
    assert got["Stuff"]["n"] == 2 and got["Things"]["n"] == 8 and got["All"]["n"] == 10
    assert got["per_class"][33] == {"pq": 0.0, "sq": 0.0, "rq": 0.0}                 # a zero row: nothing counted
    assert sum(0.02 < got["per_class"][l]["pq"] < 0.98 for l in (24, 25, 26, 27, 28, 31, 32)) >= 3
    ev.print_table()
    lines = capsys.readouterr().out.splitlines()
    assert lines[0] == "Category      |    PQ     SQ     RQ" and lines[1].startswith("road          |   0.0    0.0    0.0")
    assert "person        |  18.8   75.2   25.0" in lines and "car           |  33.9   59.3   57.1" in lines
    assert lines[-5] == "-" * 41 and lines[-4] == "              |    PQ     SQ     RQ     N"
    assert lines[-3:] == ["All           |  25.5   51.9   34.8    10", "Things        |  31.8   64.9   43.5     8",
                          "Stuff         |   0.0    0.0    0.0     2"]
    assert len(lines) == 1 + 19 + 5 and not any("caravan" in l for l in lines)


def test_categories_equal_the_recorded_ones_and_empty_results():
    want = recorded_set()["categories"]
    assert [P.categories[c["id"]] for c in want] == want and len(P.categories) == 19
    assert P.flags[26] == 3 and P.flags[7] == 1 and P.flags[29] == 2 and P.flags[0] == 0
    empty = pq.PanopticEvaluator(P).results()
    assert empty["All"] == {"pq": 0.0, "sq": 0.0, "rq": 0.0, "n": 0} and len(empty["per_class"]) == 19


def test_write_json(tmp_path):
    ev = pq.PanopticEvaluator(P)
    z = rec("edge31x47")
    ev.add_stats(z["stat"], z["iou"])
    path = ev.write_json(str(tmp_path))
    assert os.path.basename(path) == "resultPanopticSemanticLabeling.json"
    with open(path) as f:
        assert_results(ev.results(), json.load(f))


def test_opts_accept_and_refuse_panoptic(capsys):
    from centerpoly_amd.opts import opts
    parse = lambda extra: opts().parse(["polydet"] + extra)                        # noqa: E731
    opt = parse(["--dataset", "cityscapes", "--gt_dir", "g", "--panoptic", "--save_panoptic"])
    assert opt.panoptic is True and opt.save_panoptic is True
    opt = parse(["--dataset", "cityscapes"])
    assert opt.panoptic is False and opt.save_panoptic is False
    assert parse(["--dataset", "cityscapes", "--save_panoptic"]).save_panoptic is True      # needs no ground truth
    for dataset, words in (("kitti_poly", ["Cityscapes label ids"]), ("IDD", ["Cityscapes label ids"]),
                           ("synthetic", ["no result writer"])):
        with pytest.raises(SystemExit):
            parse(["--dataset", dataset, "--save_panoptic"])
        err = capsys.readouterr().err
        assert "--save_panoptic" in err and dataset in err and all(w in err for w in words), err
    for extra, words in ((["--dataset", "cityscapes", "--panoptic"], ["--gt_dir"]),
                         (["--dataset", "kitti_poly", "--gt_dir", "g", "--panoptic"], ["kitti_poly", "no panoptic evaluator for KITTI"]),
                         (["--dataset", "IDD", "--gt_dir", "g", "--panoptic"], ["IDD", "no panoptic evaluator for IDD"]),
                         (["--dataset", "synthetic", "--gt_dir", "g", "--panoptic"], ["synthetic", "no ground truth"])):
        with pytest.raises(SystemExit):
            parse(extra)
        err = capsys.readouterr().err
        assert "--panoptic" in err and all(w in err for w in words), err

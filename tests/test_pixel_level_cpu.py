"""Pixel-level evaluation without a GPU: the host restatement of cp_pixel_confusion against the matrices and instance
rows recorded from the reference's evaluators (tests/golden/pixel_level_*.npz, gen_pixel_level_golden.py), the
evaluator's float64 scores against the recorded result dictionaries, the label table, the option's refusals and the
entry point's argument checks (all of which come before the device is touched)."""
import ctypes
import json
import math
import os

import numpy as np
import pytest

import pixel_level_host as host
from centerpoly_amd import _C
from centerpoly_amd.datasets.evaluation import pixel_level as pl

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = ["star16", "mixed32", "selfcross16", "small16", "odd37x53", "missed29x41"]
PROTOS = {"cityscapes": pl.CITYSCAPES, "kitti": pl.KITTI}
IDENTITY = np.arange(256, dtype=np.uint8)


def rec(name):
    return np.load(os.path.join(HERE, "golden", "pixel_level_%s.npz" % name), allow_pickle=False)


def gt_ids(name, proto):
    z = rec(name)
    if proto == "kitti":
        return z["kitti_ids"]
    if "gt_ids" in z.files:
        return z["gt_ids"]
    return np.load(os.path.join(HERE, "golden", "instance_ap_%s.npz" % name), allow_pickle=False)["gt_ids"]


def recorded_set():
    with open(os.path.join(HERE, "golden", "pixel_level_set.json")) as f:
        return json.load(f)


def restated(name, proto):
    p = PROTOS[proto]
    ids = gt_ids(name, proto)
    inst_ids = p.instances_of_interest(np.bincount(ids.reshape(-1), minlength=65536))
    conf, inst, bad = host.pixel_confusion(rec(name)["pred"], IDENTITY, ids, p.id_divisor, p.id_direct_below, p.L,
                                           p.label_group, inst_ids)
    return conf, np.concatenate([inst_ids[:, None], inst], 1), bad


@pytest.fixture(scope="module")
def tables():
    return {(proto, name): restated(name, proto) for proto in PROTOS for name in CASES}


@pytest.mark.parametrize("proto", sorted(PROTOS))
def test_host_restatement_reproduces_the_recorded_counts(tables, proto):
    groups = tp0 = 0
    for name in CASES:
        conf, rows, bad = tables[proto, name]
        z = rec(name)
        assert np.array_equal(conf, z["conf_" + proto]), name
        assert np.array_equal(rows, z["rows_" + proto]), name
        assert bad.tolist() == [0, 0] and conf.sum() == z["pred"].size
        tp0 += int((rows[:, 2] == 0).sum())
        groups += int((rows[:, 3] > rows[:, 2]).sum())
    assert tp0 >= 1 and groups >= 1            # a missed instance, and one labelled within its category only


def assert_scores(got, want):
    assert set(want) <= set(got) | {"perImageScores"}
    assert got["confMatrix"] == want["confMatrix"] and got["labels"] == want["labels"]
    for key in ("priors", "classScores", "classInstScores", "categoryScores", "categoryInstScores"):
        assert list(got[key]) == list(want[key]), key
        for name, v in want[key].items():
            if math.isnan(v):
                assert math.isnan(got[key][name]), (key, name)
            else:
                assert abs(got[key][name] - v) <= 1e-12, (key, name, got[key][name], v)
    for key in pl.AVERAGES:
        assert abs(got[key] - want[key]) <= 1e-12, key


@pytest.mark.parametrize("proto", sorted(PROTOS))
def test_evaluator_reproduces_the_reference_scores(proto):
    want = recorded_set()["protocols"][proto]["result"]
    ev = pl.PixelLevelEvaluator(PROTOS[proto])
    for name in recorded_set()["images"]:
        z = rec(name)
        ev.add_counts(z["conf_" + proto], z["rows_" + proto])
    got = ev.summarize()
    assert_scores(got, want)
    # the fixture is worth having: finite class scores away from 0 and 1, iIoU apart from IoU, NaN for ignored labels
    assert sum(0.02 < got["classInstScores"][n] < 0.98 for n in ("person", "rider", "car", "truck", "bus")) >= 3
    assert abs(got["classScores"]["person"] - got["classInstScores"]["person"]) > 0.01
    assert math.isnan(got["classScores"]["caravan"]) and math.isnan(got["classInstScores"]["road"])
    assert math.isnan(got["categoryInstScores"]["flat"]) and not math.isnan(got["categoryInstScores"]["human"])
    text = pl.format_results(got, PROTOS[proto])
    assert "classes          IoU      nIoU" in text and "categories       IoU      nIoU" in text
    assert "caravan" not in text and "void" not in text and "%5.3f" % got["averageScoreInstClasses"] in text
    js = json.loads(json.dumps(pl.results_json(got)))
    assert set(js) == {"confMatrix", "priors", "labels", "classScores", "classInstScores", "categoryScores",
                       "categoryInstScores"} | set(pl.AVERAGES)


@pytest.mark.parametrize("proto", sorted(PROTOS))
def test_label_table_and_sizes_equal_the_recorded_ones(proto):
    want = recorded_set()["protocols"][proto]
    p = PROTOS[proto]
    assert [list(r) for r in p.labels] == want["labels"] and p.L == 34
    assert p.avg_class_size == want["avgClassSize"]
    assert p.inst_categories == ["human", "vehicle"]
    assert p.label_group.tolist() == [-1] * 24 + [0, 0] + [1] * 8
    assert pl.CITYSCAPES.avg_class_size != pl.KITTI.avg_class_size


def test_instances_of_interest():
    hist = np.zeros(65536, np.int64)
    for v in (7, 26, 1000, 7001, 24000, 24001, 26005, 29001, 33999, 34001, 65535):
        hist[v] = 3
    assert pl.CITYSCAPES.instances_of_interest(hist).tolist() == [24000, 24001, 26005, 33999]
    hist[:] = 0
    for v in (7 * 256, 24 * 256, 24 * 256 + 1, 26 * 256 + 255, 29 * 256 + 1, 34 * 256 + 1, 65535):
        hist[v] = 3
    assert pl.KITTI.instances_of_interest(hist).tolist() == [24 * 256 + 1, 26 * 256 + 255]


def test_every_pixel_is_counted_once():
    """sum(conf) + bad == H * W with bad labels of both kinds; a pixel bad in both counts in bad[0] only."""
    rng = np.random.RandomState(3)
    H, W = 23, 31
    ids = rng.choice(np.array([7, 26, 26001, 24002, 35000, 40, 999, 1000], np.uint16), (H, W))
    pred = rng.choice(np.array([0, 7, 24, 26, 33, 34, 200], np.uint8), (H, W))
    p = pl.CITYSCAPES
    conf, inst, bad = host.pixel_confusion(pred, IDENTITY, ids, 1000, 1000, p.L, p.label_group, [26001, 24002, 35000, 5])
    bad_g = np.isin(ids, [35000, 40, 999])
    assert bad[0] == bad_g.sum() > 0 and bad[1] == (~bad_g & (pred >= 34)).sum() > 0
    assert (bad_g & (pred >= 34)).any() and conf.sum() + bad.sum() == H * W
    assert inst[:, 0].tolist() == [(ids == v).sum() for v in (26001, 24002, 35000, 5)]
    assert inst[0, 1] == ((ids == 26001) & (pred == 26)).sum() and inst[0, 2] == ((ids == 26001) & np.isin(pred, [26, 33])).sum()
    assert inst[2, 1:].tolist() == [0, 0] and inst[3].tolist() == [0, 0, 0]


def test_empty_evaluator_and_the_pixel_count_check():
    ev = pl.PixelLevelEvaluator()
    ev.add_counts(np.zeros((34, 34), np.int64), np.zeros((0, 4)))
    ev.pixels += 5                                          # as if an image had passed that the matrix does not hold
    with pytest.raises(RuntimeError, match="disagree"):
        ev.summarize()
    empty = pl.PixelLevelEvaluator().summarize()
    assert all(math.isnan(empty[k]) for k in pl.AVERAGES)


def test_opts_accept_and_refuse_pixel_iou(capsys):
    from centerpoly_amd.opts import opts
    parse = lambda extra: opts().parse(["polydet"] + extra)                        # noqa: E731
    assert parse(["--dataset", "cityscapes", "--gt_dir", "g", "--pixel_iou"]).pixel_iou is True
    assert parse(["--dataset", "kitti_poly", "--gt_dir", "g", "--pixel_iou"]).pixel_iou is True
    assert parse(["--dataset", "cityscapes"]).pixel_iou is False
    for extra, words in ((["--dataset", "cityscapes", "--pixel_iou"], ["--gt_dir"]),
                         (["--dataset", "IDD", "--gt_dir", "g", "--pixel_iou"], ["IDD", "level ids"]),
                         (["--dataset", "synthetic", "--gt_dir", "g", "--pixel_iou"], ["synthetic", "no ground truth"])):
        with pytest.raises(SystemExit):
            parse(extra)
        err = capsys.readouterr().err
        assert "--pixel_iou" in err and all(w in err for w in words), err


# ------------------------------------------------------------------------------------------------------ ABI --
def _call(**over):
    """cp_pixel_confusion on HOST buffers (a valid call but for what `over` changes): every refusal comes before
    the device is touched, so nothing reads them."""
    L = _C.lib()
    bufs = {"pred": np.zeros(64, np.uint8), "pred_label": np.zeros(256, np.uint8), "gt_ids": np.zeros(64, np.uint16),
            "label_group": np.full(64, -1, np.int8), "inst_ids": np.zeros(1024, np.int32),
            "conf": np.zeros(64 * 64, np.int64), "inst": np.zeros(3 * 1024, np.int32), "bad": np.zeros(2, np.int32),
            "workspace": np.zeros(L.cp_pixel_confusion_workspace_bytes(4), np.uint8)}
    a = dict(H=8, W=8, id_divisor=1000, id_direct_below=1000, L=34, G=4, workspace_bytes=len(bufs["workspace"]))
    a.update({k: v.ctypes.data_as(ctypes.c_void_p) for k, v in bufs.items()})
    a.update(over)
    a["_keep"] = bufs
    return L.cp_pixel_confusion(a["pred"], a["pred_label"], a["gt_ids"], a["H"], a["W"], a["id_divisor"],
                                a["id_direct_below"], a["L"], a["label_group"], a["inst_ids"], a["G"], a["conf"],
                                a["inst"], a["bad"], a["workspace"], a["workspace_bytes"], None)


def test_abi_exports_and_refusals_before_the_device():
    L = _C.lib()
    assert "cp_pixel_confusion" in _C.EXPORTS and "cp_pixel_confusion_workspace_bytes" in _C.EXPORTS
    need = L.cp_pixel_confusion_workspace_bytes(0)
    assert need == L.cp_pixel_confusion_workspace_bytes(1024) and need >= 65536 * 2
    EINVAL, EUNSUPPORTED, EWORKSPACE = -1, -2, -3
    for name in ("pred", "pred_label", "gt_ids", "label_group", "inst_ids", "conf", "inst", "bad"):
        assert _call(**{name: None}) == EINVAL, name
    for over in ({"H": 0}, {"W": -1}, {"L": 0}, {"G": -1}, {"id_divisor": 0}, {"id_direct_below": -1}):
        assert _call(**over) == EINVAL, over
    for over in ({"L": 65}, {"G": 1025}, {"H": 65536, "W": 32768}):
        assert _call(**over) == EUNSUPPORTED, over
    assert _call(workspace_bytes=need - 1) == EWORKSPACE and _call(workspace=None) == EWORKSPACE

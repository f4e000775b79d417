"""Boundary IoU / Boundary AP without a GPU: the host statement (tests/golden/boundary_host.py) against the set
definition, BoundaryEvaluator's protocol on count tables, the band-width formula, the options, and cp_boundary_overlaps'
refusals (they come before any device work, so they run anywhere)."""
import numpy as np
import pytest

import boundary_cases
import boundary_host as bh
from centerpoly_amd.datasets.evaluation import boundary as bd
from centerpoly_amd.datasets.evaluation import instance_level as il


# ------------------------------------------------------------------------------------------ host statement --
@pytest.mark.parametrize("seed", range(8))
def test_host_statement_is_the_set_definition(seed):
    rng = np.random.RandomState(100 + seed)
    H, W = rng.randint(1, 13, 2)
    for d in (1, 2, 3, 7):
        m = rng.rand(H, W) < (0.55 + 0.05 * seed)
        assert np.array_equal(bh.band(m, d), bh.band_brute(m, d)), (H, W, d)
    full = np.ones((H, W), bool)
    assert np.array_equal(bh.band(full, 2), bh.band_brute(full, 2))
    assert not bh.band(np.zeros((H, W), bool), 3).any()


@pytest.mark.parametrize("seed", range(4))
def test_cropped_host_statement_is_the_host_statement(seed):
    rng = np.random.RandomState(200 + seed)
    H, W = rng.randint(8, 40, 2)
    m = np.zeros((H, W), bool)
    y, x = rng.randint(0, H - 4), rng.randint(0, W - 4)
    m[y:y + rng.randint(2, H), x:x + rng.randint(2, W)] = True
    m &= rng.rand(H, W) < 0.95
    if seed == 0:
        m[0, :] = m[:, -1] = True                                         # touching the image's edges
    for d in (1, 3, 9):
        assert np.array_equal(bh.band_of_crop(m, d), bh.band(m, d))
    c = boundary_cases.all_cases()[3]
    full = bh.boundary_counts(c["masks"], c["ids"], c["inst_ids"], c["d"])
    for a, b in zip(bh.boundary_tables(c["masks"], c["ids"], c["inst_ids"], c["d"]), full[:3]):
        assert np.array_equal(a, b)


def test_host_statement_on_hand_made_shapes():
    d = 3
    full = np.ones((20, 30), bool)
    frame = full.copy()
    frame[d:-d, d:-d] = False
    assert np.array_equal(bh.band(full, d), frame)                        # the full plane: a frame of width d
    wide, wider = np.zeros((20, 30), bool), np.zeros((20, 30), bool)
    wide[:, 5:5 + 2 * d], wider[:, 5:5 + 2 * d + 1] = True, True
    assert np.array_equal(bh.band(wide, d), wide)                         # a strip of width 2d is all band
    inner = wider & ~bh.band(wider, d)
    assert inner[:, 5 + d].sum() == 20 - 2 * d and inner.sum() == 20 - 2 * d   # 2d + 1: one interior line
    ids = np.zeros((8, 8), np.uint16)
    ids[:, 4:] = 5
    g = bh.gt_band(ids, 1)
    assert g[:, 3:5].all() and g[0].all() and not g[2:6, 1:3].any()       # both sides of a shared border are band


def test_random_scenes_of_the_gpu_cases_are_not_vacuous():
    seen = 0
    for c in boundary_cases.all_cases():
        if "x" not in c["name"] or len(c["masks"]) == 0 or not c["inst_ids"] or c["masks"].shape[1] * c["masks"].shape[2] > 20000:
            continue
        b_inter, b_pred, b_gt, _, gband = bh.boundary_counts(c["masks"][:4], c["ids"], c["inst_ids"], c["d"], c["bounds"])
        assert b_pred.any() and gband.any() and b_gt.any() and b_inter.any(), c["name"]
        seen += 1
    assert seen >= 15


# ------------------------------------------------------------------------------------------------ protocol --
def _random_tables(seed, ev_list):
    rng = np.random.RandomState(seed)
    for _ in range(4):
        G, n = rng.randint(0, 7), rng.randint(0, 9)
        labs = rng.choice(il.LABEL_IDS[:3], G)
        gid = np.array([l * 1000 + k if rng.rand() < 0.8 else l for k, l in enumerate(labs)], np.int64).reshape(G)
        order = np.argsort(gid, kind="stable")
        size = rng.randint(50, 3000, G)
        table = np.stack([gid, labs, size], 1).astype(np.int64).reshape(G, 3)[order]
        pix = rng.randint(0, 3000, n)
        inter = np.minimum(rng.randint(0, 3000, (n, G)) * (rng.rand(n, G) < 0.4), np.minimum(pix[:, None], table[None, :, 2]))
        args = (table, rng.choice(il.LABEL_IDS[:4], n).tolist(), np.round(rng.rand(n), 2).tolist(), pix,
                rng.randint(0, 50, n), inter)
        for ev in ev_list:
            if isinstance(ev, bd.BoundaryEvaluator):
                ev.add_counts(*args, b_pred=pix, b_gt=table[:, 2], b_inter=inter)
            else:
                ev.add_counts(*args)


@pytest.mark.parametrize("seed", range(4))
def test_band_tables_equal_to_mask_tables_give_the_plain_ap(seed):
    plain, bnd = il.InstanceLevelEvaluator(), bd.BoundaryEvaluator()
    _random_tables(seed, [plain, bnd])
    want = plain.ap_matrix()
    assert np.array_equal(bnd.ap_matrix(), want, equal_nan=True)
    assert np.array_equal(bnd.plain_ap_matrix(), want, equal_nan=True)
    res, ref = bnd.summarize(), plain.summarize()
    for a, b in (("allBoundaryAp", "allAp"), ("allBoundaryAp50%", "allAp50%"), ("allAp", "allAp"), ("allAp50%", "allAp50%")):
        assert res[a] == ref[b] or (np.isnan(res[a]) and np.isnan(ref[b]))


def test_a_pair_with_a_good_mask_and_a_poor_contour():
    """Mask IoU 800 / (900 + 900 - 800) = 0.8, boundary IoU 90 / (145 + 145 - 90) = 0.45: a match of the plain AP at
    0.5 (AP 1: one true positive, nothing else), no match of the Boundary AP there (the prediction is a false positive,
    the ground truth a false negative: AP 0), and a match again just below 0.45 (the comparison is strict)."""
    ev = bd.BoundaryEvaluator()
    ev.add_counts(np.array([[26001, 26, 900]]), [26], [0.9], [900], [0], [[800]], b_pred=[145], b_gt=[145], b_inter=[[90]])
    car = il.LABEL_IDS.index(26)
    res = ev.summarize()
    assert res["resultApMatrix"][0, car, 0] == 1.0 and res["resultBoundaryApMatrix"][0, car, 0] == 0.0
    assert res["classes"]["car"]["ap50%"] == 1.0 and res["classes"]["car"]["bap50%"] == 0.0
    assert (res["resultApMatrix"][0, car, :6] == 1.0).all() and (res["resultApMatrix"][0, car, 6:] == 0.0).all()   # 0.8 itself: no
    assert (res["resultBoundaryApMatrix"][0, car] == 0.0).all()
    assert ev._class_ap(26, 0.45) == 0.0 and ev._class_ap(26, 0.4499) == 1.0 and ev._class_ap(26, 0.3) == 1.0
    ev._plain = True
    assert ev._class_ap(26, 0.5) == 1.0
    ev._plain = False
    # a pair that shares no mask pixel has overlap 0 whatever its band tables say
    ev2 = bd.BoundaryEvaluator()
    ev2.add_counts(np.array([[26001, 26, 900]]), [26], [0.9], [900], [0], [[0]], b_pred=[145], b_gt=[145], b_inter=[[0]])
    assert ev2._class_ap(26, 0.0) == 0.0
    with pytest.raises(ValueError, match="b_pred"):
        ev2.add_counts(np.array([[26001, 26, 900]]), [26], [0.9], [900], [0], [[0]])


def test_results_text_and_json(tmp_path):
    import json
    ev = bd.BoundaryEvaluator(ratio=0.02)
    assert ev.band_width(1024, 2048) == 46 and ev.band_width(375, 1242) == 26
    ev.add_counts(np.array([[26001, 26, 900]]), [26], [0.9], [900], [0], [[800]], b_pred=[145], b_gt=[145], b_inter=[[90]])
    res = ev.summarize()
    assert res["ratio"] == 0.02 and res["bandWidths"] == {"1024x2048": 46, "375x1242": 26}
    text = bd.format_results(res)
    assert "bAP" in text and "car" in text and "46 px at 1024x2048" in text
    path = bd.write_results(res, str(tmp_path))
    assert path.endswith("resultBoundaryInstanceLevel.json")
    js = json.load(open(path))
    assert set(js) == {"averages", "overlaps", "minRegionSizes", "instLabels", "resultBoundaryApMatrix", "resultApMatrix"}
    assert js["averages"]["allBoundaryAp"] == 0.0 and js["averages"]["ratio"] == 0.02


# ------------------------------------------------------------------------------------- band width, options --
def test_band_width_formula():
    """d = max(1, round(ratio * diagonal)): 0.005 * 2289.73 = 11.45, 0.005 * 1297.38 = 6.49, 0.005 * 2202.91 = 11.01,
    0.005 * 1468.60 = 7.34; with 0.02: 45.79, 25.95, 44.06, 29.37."""
    sizes = ((1024, 2048), (375, 1242), (1080, 1920), (720, 1280))
    assert [bd.band_width(h, w) for h, w in sizes] == [11, 6, 11, 7]
    assert [bd.band_width(h, w, 0.02) for h, w in sizes] == [46, 26, 44, 29]
    assert bd.band_width(3, 4, 0.005) == 1 and bd.DEFAULT_RATIO == 0.005
    with pytest.raises(ValueError, match=r"d = 92 pixels on a 2048 x 1024 image"):
        bd.checked_band_width(1024, 2048, 0.04)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="finite and > 0"):
            bd.BoundaryEvaluator(ratio=bad)


def test_opts_accept_and_refuse_boundary(capsys):
    from centerpoly_amd.opts import opts
    parse = lambda extra: opts().parse(["polydet"] + extra)               # noqa: E731
    for ds in ("cityscapes", "kitti_poly", "IDD"):
        opt = parse(["--dataset", ds, "--gt_dir", "g", "--boundary"])
        assert opt.boundary is True and opt.boundary_ratio == 0.005
    assert parse(["--dataset", "cityscapes"]).boundary is False
    assert parse(["--dataset", "cityscapes", "--gt_dir", "g", "--boundary", "--boundary_ratio", "0.02"]).boundary_ratio == 0.02
    for extra, words in ((["--dataset", "cityscapes", "--boundary"], ["--gt_dir"]),
                         (["--dataset", "synthetic", "--gt_dir", "g", "--boundary"], ["synthetic", "no ground truth"]),
                         (["--dataset", "cityscapes", "--gt_dir", "g", "--boundary", "--boundary_ratio", "0"], ["--boundary_ratio"]),
                         (["--dataset", "cityscapes", "--gt_dir", "g", "--boundary", "--boundary_ratio", "-0.01"], ["--boundary_ratio"]),
                         (["--dataset", "cityscapes", "--gt_dir", "g", "--boundary", "--boundary_ratio", "nan"], ["--boundary_ratio"])):
        with pytest.raises(SystemExit):
            parse(extra)
        err = capsys.readouterr().err
        assert "--boundary" in err and all(w in err for w in words), err


# ---------------------------------------------------------------------------------------------- refusals --
def test_refusals_come_before_any_device_work():
    assert boundary_cases.refusals() == 23

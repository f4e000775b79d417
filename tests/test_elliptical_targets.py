"""`--elliptical_gt`: elliptical centre heat maps (reference src/lib/datasets/sample/polydet.py:156-159,223-228,401-403,
src/lib/utils/image.py:144-173).

CPU: the options accept the published CenterPoly v2 recipe and refuse `--mse_loss` with it, cp_polydet_targets_ex
validates without a device, and a numpy restatement of the elliptical heat map and of the --dense_poly replay (on top
of oracle/targets.py's UMich targets, which stay the same) reproduces the reference's own arrays: sampler_ell_*.npz
(its PolydetDataset.__getitem__ with elliptical_gt=True) and ellipse_prims.npz (its draw_ellipse_gaussian), bit for bit.
GPU: cp_polydet_targets_ex against those fixtures and against the restatement at training size, and two trainer steps.
"""
import math

import numpy as np
import pytest
import torch

from centerpoly_amd import _C, synth
from oracle import post as opost
from oracle import targets as otg
from test_targets import _replay_draws, _sampler_anns

ELL_CASES = ["ell_cart_crop", "ell_cart_flip", "ell_polar_flip", "ell_cart_dense", "ell_cart_catspec", "ell_cart_val"]

# experiments/centerpolyV2_cityscapes_polar.sh of the reference, minus the dataset and checkpoint paths
RECIPE = ["polydet", "--elliptical_gt", "--arch", "smallhourglass", "--poly_loss", "l1+iou", "--rep", "polar",
          "--poly_weight", "1", "--nbr_points", "16", "--batch_size", "4", "--master_batch", "4", "--lr", "2e-4",
          "--val_intervals", "24"]


# ---------------------------------------------------------------------------------------------------------------------
# numpy restatement
def ellipse_radii(radius, h, w):
    """sample/polydet.py:223-225 with h, w the float32 box sides: float32 ratio and product, truncated."""
    h, w = np.float32(h), np.float32(w)
    rx = radius if h > w else int(np.float32(radius) * (w / h))
    ry = radius if w >= h else int(np.float32(radius) * (h / w))
    return rx, ry


def draw_ellipse(hm, cx, cy, rx, ry):
    """draw_ellipse_gaussian (utils/image.py:159-173) on a float32 map: float64 values, no epsilon cut, np.maximum."""
    H, W = hm.shape
    left, right = min(cx, rx), min(W - cx, rx + 1)
    top, bottom = min(cy, ry), min(H - cy, ry + 1)
    m = max(2 * rx + 1, 2 * ry + 1)
    mr, mc = (2 * rx + 1) / m, (2 * ry + 1) / m          # the reference's y_modifier scales the ROW offset
    sigma = (2 * min(rx, ry) + 1) / 6
    dy = np.arange(-top, bottom, dtype=np.float64).reshape(-1, 1)
    dx = np.arange(-left, right, dtype=np.float64).reshape(1, -1)
    g = np.exp(-(((dy * mr) ** 2 + (dx * mc) ** 2) / (2 * sigma ** 2)))
    window = hm[cy - top:cy + bottom, cx - left:cx + right]
    np.maximum(window, g, out=window)
    return hm


def elliptical_targets(anns, t, flipped, width, oh, ow, num_classes, max_objs, N, rep, no_reorder_flip=False,
                       dense_poly=False, cat_spec_poly=False):
    """oracle.targets.build_targets with the centre heat map (and the --dense_poly replay) of --elliptical_gt.  The
    UMich oracle's wh / peak / poly give every live object's sides, centre and polygon row."""
    ret = otg.build_targets(anns, t, flipped, width, oh, ow, num_classes, max_objs, N, rep,
                            no_reorder_flip=no_reorder_flip, dense_poly=dense_poly, cat_spec_poly=cat_spec_poly)
    base = otg.build_targets(anns, t, flipped, width, oh, ow, num_classes, max_objs, N, rep,
                             no_reorder_flip=no_reorder_flip)
    hm = np.zeros((num_classes, oh, ow), np.float32)
    dense = np.zeros((2 * N, oh, ow), np.float32)
    for k in range(min(len(anns), max_objs)):
        w, h = base["wh"][k]
        if not (h > 0 and w > 0):
            continue
        radius = max(0, int(otg.gaussian_radius((math.ceil(h), math.ceil(w)))))
        cx, cy = [int(v) for v in base["peak"][k].astype(np.int32)]
        rx, ry = ellipse_radii(radius, h, w)
        draw_ellipse(hm[int(anns[k]["cls_id"])], cx, cy, rx, ry)
        if dense_poly:                                  # draw_dense_reg keeps the UMich window and Gaussian
            otg.draw_dense_reg(dense, hm.max(axis=0), (cx, cy), base["poly"][k], radius)
    ret["hm"] = hm
    if dense_poly:
        mask = dense.copy()
        mask[mask != 0] = 1
        ret["dense_poly"], ret["dense_poly_mask"] = dense, mask
    return ret


def _sampler_inputs(g):
    oh, ow = [int(v) for v in g["out_hw"]]
    W = int(g["img_hw"][1])
    for j, (c, s, flipped) in enumerate(_replay_draws(g, len(g["img_ids"]))):
        yield j, _sampler_anns(g, j), opost.get_affine_transform(c, s, 0, [ow, oh]), flipped, W, oh, ow


# ---------------------------------------------------------------------------------------------------------------------
# CPU
def test_published_recipe_parses():
    from centerpoly_amd.opts import opts
    opt = opts().parse(RECIPE)
    assert opt.elliptical_gt and opt.rep == "polar" and opt.master_batch_size == 4 and opt.val_intervals == 24
    assert not opts().parse(["polydet"]).elliptical_gt


def test_mse_loss_with_elliptical_gt_is_refused(capsys):
    from centerpoly_amd.opts import opts
    with pytest.raises(SystemExit):
        opts().parse(["polydet", "--mse_loss", "--elliptical_gt"])
    assert "--mse_loss" in capsys.readouterr().err
    assert opts().parse(["polydet", "--mse_loss"]).mse_loss


def test_targets_ex_validates_without_gpu():
    L = _C.lib()
    s = _C.TargetShape(2, 8, 16, 8, 64, 128, 0, 0)
    nil = [None] * 19
    assert L.cp_polydet_targets_ex(s, _C.HEATMAP_ELLIPSE, *nil, None, 0, None) == -1
    # an unknown mode is refused before anything is dereferenced or launched
    junk = [_C.c_void_p(16)] * 19
    nws = L.cp_polydet_targets_workspace_bytes(s)
    for mode in (-1, 2, 7):
        assert L.cp_polydet_targets_ex(s, mode, *junk, _C.c_void_p(16), nws, None) == -1
    # the descriptor rows hold the ellipse radii and the mode as well as radius, class, centre and vertices
    assert nws >= 2 * 8 * (7 + 2 * 16) * 4


def test_synthetic_dataset_needs_device_targets():
    import contextlib
    import io
    from centerpoly_amd.datasets.synthetic import SyntheticPolydet
    from centerpoly_amd.opts import opts
    with contextlib.redirect_stdout(io.StringIO()):
        opt = opts().init(["polydet", "--elliptical_gt", "--input_h", "64", "--input_w", "64"])
        with pytest.raises(ValueError, match="--device_targets"):
            SyntheticPolydet(opt, "train")
        opt = opts().init(["polydet", "--elliptical_gt", "--device_targets", "--input_h", "64", "--input_w", "64"])
        assert "trans_output" in SyntheticPolydet(opt, "train")[0]


def test_restatement_matches_reference_ellipse_prims(golden):
    g = golden("ellipse_prims")
    h, w = [int(v) for v in g["hw"]]
    stacked = np.zeros((h, w), np.float32)
    for i, (cx, cy, rx, ry) in enumerate(g["splats"].tolist()):
        single = draw_ellipse(np.zeros((h, w), np.float32), cx, cy, rx, ry)
        assert np.array_equal(single, g["singles"][i]), (cx, cy, rx, ry)
        draw_ellipse(stacked, cx, cy, rx, ry)
    assert np.array_equal(stacked, g["stacked"])
    assert stacked.max() == 1.0 and (g["singles"] > 0).sum(axis=(1, 2)).min() >= 1


@pytest.mark.parametrize("case", ELL_CASES)
def test_restatement_matches_reference_sampler(case, golden):
    """Every array of the reference's elliptical __getitem__: hm (and dense_poly) from the restatement, the rest from
    the UMich oracle unchanged.  The fixtures do exercise the mode: hm differs from the UMich one in each case."""
    g = golden("sampler_" + case)
    assert bool(g["elliptical_gt"])
    dense, catspec = bool(g["dense_poly"]), bool(g["cat_spec_poly"])
    differs = 0
    for j, anns, t, flipped, W, oh, ow in _sampler_inputs(g):
        r = elliptical_targets(anns, t, flipped, W, oh, ow, 8, 128, 16, str(g["rep"]),
                               no_reorder_flip=bool(g["no_reorder_flip"]), dense_poly=dense, cat_spec_poly=catspec)
        assert sorted(r) == sorted(str(k) for k in g["s%d_keys" % j]), (case, sorted(r))
        for k in r:
            if k == "freq_mask":
                assert float(r[k]) == float(g["s%d_freq_mask" % j])
                continue
            ref = g["s%d_%s" % (j, k)]
            assert r[k].dtype == ref.dtype and np.array_equal(r[k], ref), (case, j, k)
        umich = otg.build_targets(anns, t, flipped, W, oh, ow, 8, 128, 16, str(g["rep"]),
                                  no_reorder_flip=bool(g["no_reorder_flip"]), dense_poly=dense)
        differs += int(not np.array_equal(umich["hm"], r["hm"]))
        if dense:
            assert not np.array_equal(umich["dense_poly"], r["dense_poly"])
    assert differs >= 1


# ---------------------------------------------------------------------------------------------------------------------
# GPU
@pytest.mark.gpu
@pytest.mark.parametrize("case", ELL_CASES)
def test_device_elliptical_targets_match_reference_sampler(case, golden):
    """cp_polydet_targets_ex(CP_HEATMAP_ELLIPSE) against the reference's elliptical __getitem__, with the rules of
    test_targets.py::test_device_targets_match_reference_sampler: masks, indices and heat maps bit-exact, float targets
    to its tolerances, at most 2 pixels of dense ownership difference per image."""
    from centerpoly_amd.datasets.sample.polydet import build_targets, collate, pack_annotations
    g = golden("sampler_" + case)
    packed = [pack_annotations(anns, t, fl, W, 128, 16) for _, anns, t, fl, W, _, _ in _sampler_inputs(g)]
    oh, ow = [int(v) for v in g["out_hw"]]
    raw = {k: v.cuda() for k, v in collate(packed).items()}
    dense, catspec = bool(g["dense_poly"]), bool(g["cat_spec_poly"])
    out = build_targets(raw, oh, ow, 8, rep=str(g["rep"]), no_reorder_flip=bool(g["no_reorder_flip"]),
                        dense_poly=dense, cat_spec_poly=catspec, elliptical_gt=True)
    for j in range(len(packed)):
        assert sorted(out) == sorted(str(k) for k in g["s%d_keys" % j]), (case, sorted(out))
        for k in ("reg_mask", "ind", "hm", "border_hm", "cat_spec_mask"):
            if k in out:
                assert np.array_equal(out[k][j].cpu().numpy(), g["s%d_%s" % (j, k)]), (case, j, k)
        for k in ("poly", "pseudo_depth", "wh", "peak", "reg", "cat_spec_poly"):
            if k in out:
                ref = g["s%d_%s" % (j, k)]
                np.testing.assert_allclose(out[k][j].cpu().numpy(), ref, rtol=2.4e-7,
                                           atol=1e-6 * max(1.0, np.abs(ref).max()), err_msg="%s %d %s" % (case, j, k))
        if "freq_mask" in out:
            np.testing.assert_allclose(float(out["freq_mask"][j]), float(g["s%d_freq_mask" % j]), rtol=1e-6)
        if dense:
            ref_m, got_m = g["s%d_dense_poly_mask" % j], out["dense_poly_mask"][j].cpu().numpy()
            ref_d, got_d = g["s%d_dense_poly" % j], out["dense_poly"][j].cpu().numpy()
            px_diff = (ref_m != got_m).any(axis=0)
            assert px_diff.sum() <= 2, (case, j, int(px_diff.sum()))
            np.testing.assert_allclose(got_d[:, ~px_diff], ref_d[:, ~px_diff], rtol=2.4e-7, atol=1e-5)


def _box_ann(x, y, w, h, cls, N=16):
    """A box [x, y, w, h] in image pixels with an N-gon inscribed in it (vertex 0 near the top-left)."""
    th = -0.75 * np.pi + np.arange(N) * (2 * np.pi / N)
    xs, ys = x + w / 2 + w / 2 * np.cos(th), y + h / 2 + h / 2 * np.sin(th)
    return {"bbox": [float(x), float(y), float(w), float(h)], "poly": [float(v) for v in np.stack([xs, ys], 1).ravel()],
            "cls_id": cls, "pseudo_depth": 0.5, "freq": 0.1}


def _extremes(in_h, in_w):
    """Constructed boxes (output scale 1/4, a power of two): 1:20 and 20:1, exact squares, boxes clipped at each
    border and corner, radius 0, and overlaps of elongated objects of one class."""
    a = [_box_ann(400, 100, 40, 800, 0), _box_ann(300, 500, 800, 40, 0),              # 1:20 / 20:1, crossing
         _box_ann(1000, 200, 40, 40, 1), _box_ann(1100, 600, 256, 256, 2),            # exact squares
         _box_ann(1500, 100, 8, 800, 3), _box_ann(1200, 900, 800, 8, 3),              # radius 1, 1:100
         _box_ann(60, 60, 4, 4, 4), _box_ann(600, 950, 2, 6, 4),                      # radius 0
         _box_ann(-300, 400, 500, 60, 5), _box_ann(in_w - 200, 420, 500, 60, 5),       # clipped left / right
         _box_ann(700, -350, 60, 500, 6), _box_ann(760, in_h - 150, 60, 500, 6),       # clipped top / bottom
         _box_ann(-40, -40, 400, 80, 7), _box_ann(in_w - 60, in_h - 300, 120, 400, 7)]  # corners
    return a + synth.raw_annotations("ell/fill", in_h, in_w, nbr_points=16, n_objs=128 - len(a))


@pytest.mark.gpu
def test_elliptical_targets_training_size():
    """B=4 x 128 objects at 1024x2048 (256x512 maps): hm bit-exact against the restatement, dense ownership within 2
    pixels; every other target and the UMich call with elliptical_gt=False bit-identical to the plain call."""
    from centerpoly_amd.datasets.sample.polydet import build_targets, collate, pack_annotations
    in_h, in_w, N = 1024, 2048, 16
    oh, ow = in_h // 4, in_w // 4
    images = [synth.raw_annotations("ell/img%d" % i, in_h, in_w, nbr_points=N, n_objs=128) for i in range(3)]
    images.append(_extremes(in_h, in_w))
    views = [(np.array([in_w * 0.47, in_h * 0.55], np.float32), in_w * 0.9, True),
             (np.array([in_w * 0.5, in_h * 0.5], np.float32), in_w * 1.2, False),
             (np.array([in_w * 0.6, in_h * 0.4], np.float32), in_w * 0.7, False),
             (np.array([in_w * 0.5, in_h * 0.5], np.float32), float(in_w), False)]     # exactly 1/4, no shift
    trans = [opost.get_affine_transform(c, s, 0, [ow, oh]) for c, s, _ in views]
    packed = [pack_annotations(a, t, v[2], in_w, 128, N) for a, t, v in zip(images, trans, views)]
    raw = {k: v.cuda() for k, v in collate(packed).items()}
    ell = {k: v.cpu().numpy() for k, v in build_targets(raw, oh, ow, 8, dense_poly=True, elliptical_gt=True).items()}
    umich = {k: v.cpu().numpy() for k, v in build_targets(raw, oh, ow, 8, dense_poly=True).items()}
    off = {k: v.cpu().numpy() for k, v in build_targets(raw, oh, ow, 8, dense_poly=True, elliptical_gt=False).items()}
    assert sorted(off) == sorted(umich)
    for k in umich:
        assert np.array_equal(off[k], umich[k]), k
        if k not in ("hm", "dense_poly", "dense_poly_mask"):
            assert np.array_equal(ell[k], umich[k]), k
    assert not np.array_equal(ell["hm"], umich["hm"])
    stretched = 0
    for b, (anns, t, v) in enumerate(zip(images, trans, views)):
        r = elliptical_targets(anns, t, v[2], in_w, oh, ow, 8, 128, N, "cartesian", dense_poly=True)
        assert np.array_equal(ell["hm"][b], r["hm"]), b
        px_diff = (ell["dense_poly_mask"][b] != r["dense_poly_mask"]).any(axis=0)
        assert px_diff.sum() <= 2, (b, int(px_diff.sum()))
        np.testing.assert_allclose(ell["dense_poly"][b][:, ~px_diff], r["dense_poly"][:, ~px_diff], rtol=2.4e-7,
                                   atol=1e-5)
        wh = r["wh"][r["wh"][:, 0] > 0]
        stretched += int((wh[:, 0] != wh[:, 1]).sum())
    assert stretched > 100
    # the constructed extremes took the paths they were built for
    wh = ell["wh"][3][:14]
    assert wh[2, 0] == wh[2, 1] == 10.0 and wh[0, 1] == 20 * wh[0, 0] and wh[1, 0] == 20 * wh[1, 1]
    assert ell["hm"][3].max() == 1.0


@pytest.mark.gpu
def test_trainer_steps_with_elliptical_gt():
    """--elliptical_gt --device_targets on the synthetic set: two optimisation steps with finite losses, and the hm the
    trainer builds differs from the UMich one of the same batch."""
    import contextlib
    import io
    from centerpoly_amd.datasets.dataset_factory import get_dataset
    from centerpoly_amd.models.model import create_model
    from centerpoly_amd.opts import opts
    from centerpoly_amd.trains.train_factory import train_factory
    with contextlib.redirect_stdout(io.StringIO()):
        opt = opts().init(["polydet", "--elliptical_gt", "--device_targets", "--arch", "smallhourglass", "--rep",
                           "polar", "--poly_loss", "l1+iou", "--input_h", "256", "--input_w", "256",
                           "--batch_size", "2", "--num_iters", "2"])
        Dataset = get_dataset("synthetic", opt.task)
        opt = opts().update_dataset_info_and_set_heads(opt, Dataset)
        ds = Dataset(opt, "train")
    opt.device = torch.device("cuda")
    torch.manual_seed(317)
    model = create_model(opt.arch, opt.heads, opt.head_conv)
    trainer = train_factory["polydet"](opt, model, torch.optim.Adam(model.parameters(), opt.lr))
    trainer.set_device(opt.gpus, opt.chunk_sizes, opt.device)
    loader = torch.utils.data.DataLoader(ds, batch_size=2, shuffle=False, num_workers=0)
    stats, _ = trainer.train(1, loader)
    assert np.isfinite(stats["loss"]) and stats["hm_l"] > 0 and stats["poly_l"] > 0
    batch = {k: v.to(opt.device) for k, v in next(iter(loader)).items() if torch.is_tensor(v)}
    hm_ell = trainer.prepare_batch(dict(batch))["hm"]
    opt.elliptical_gt = False
    hm_umich = trainer.prepare_batch(dict(batch))["hm"]
    assert not torch.equal(hm_ell, hm_umich)
    assert torch.equal(hm_ell.amax(dim=(1, 2, 3)), hm_umich.amax(dim=(1, 2, 3)))     # 1 at every centre in both

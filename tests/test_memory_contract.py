"""Every entry point that takes a workspace, run in memory that behaves like production memory at its worst: the caching
allocator's free blocks hold a fill pattern (so the wrappers' `torch.empty` outputs start dirty), every workspace is
exactly as long as its `cp_*_workspace_bytes` says, starts out holding the same pattern, and lies between guard bands that
are checked afterwards (tests/memory_guard.py).  The checks themselves are the families' existing ones -- host statement,
oracle or golden, at their own tolerances -- imported from their test modules, at the shapes that cross each sizing
constant.

Where the existing check is bit-equality with a reference that does not depend on the memory, the three fills agree with
each other bit for bit because each equals that reference; where a family hands its raw outputs back they are compared
across the fills as well (`_agree`)."""
import os
import types

import numpy as np
import pytest

import memory_guard as mg
from centerpoly_amd import _C

HERE = os.path.dirname(os.path.abspath(__file__))
FILL_IDS = ["fill_%02X" % f for f in mg.FILLS]


def _golden(name):
    return np.load(os.path.join(HERE, "golden", name + ".npz"), allow_pickle=False)


def _run(test, *args, **kw):
    """An imported test function: one that skips has checked nothing, which counts as a failure here."""
    try:
        return test(*args, **kw)
    except pytest.skip.Exception as e:                                     # pragma: no cover
        pytest.fail("%s skipped (%s): nothing was checked" % (test.__name__, e))


# ======================================================================================================= CPU ====
# which guarded family exercises each workspace formula: a new `cp_*_workspace_bytes` without a line here fails the suite
COVERED_BY = {
    "cp_bn_workspace_bytes": "batchnorm",
    "cp_sigmoid_focal_workspace_bytes": "losses",
    "cp_mse_workspace_bytes": "losses",
    "cp_dense_l1_workspace_bytes": "losses",
    "cp_poly_iou_order_workspace_bytes": "losses",
    "cp_polydet_targets_workspace_bytes": "targets",
    "cp_sample_inputs_workspace_bytes": "training_inputs",
    "cp_color_aug_workspace_bytes": "training_inputs",
    "cp_polydet_decode_workspace_bytes": "decode",
    "cp_merge_detections_workspace_bytes": "merge_nms",
    "cp_merge_detections_mask_workspace_bytes": "merge_nms",
    "cp_polygon_overlaps_workspace_bytes": "merge_nms",
    "cp_rle_encode_workspace_bytes": "rle_png",
    "cp_rle_decode_workspace_bytes": "rle_png",
    "cp_png_deflate_workspace_bytes": "rle_png",
    "cp_track_kinematics_workspace_bytes": "track",
    "cp_instance_map_workspace_bytes": "pixel_counts",
    "cp_instance_overlaps_workspace_bytes": "pixel_counts",
    "cp_boundary_overlaps_workspace_bytes": "pixel_counts",
    "cp_segment_medians_workspace_bytes": "pixel_counts",
    "cp_pixel_confusion_workspace_bytes": "pixel_counts",
    "cp_panoptic_pairs_workspace_bytes": "pixel_counts",
    "cp_polygon_masks_workspace_bytes": "rasterisers",
    "cp_polygon_paint_workspace_bytes": "rasterisers",
    "cp_annot_id_instances_workspace_bytes": "rasterisers",
    "cp_render_overlay_workspace_bytes": "rasterisers",
    "cp_dcn_v2_forward_workspace_bytes": "dcn",
    "cp_dcn_v2_forward_fused_workspace_bytes": "dcn",
    "cp_dcn_v2_backward_workspace_bytes": "dcn",
    "cp_conv_mfma_input_grad_relu_workspace_bytes": "dcn",
}


def test_every_workspace_formula_has_a_guarded_case():
    exported = {name for name in _C.EXPORTS if name.endswith("_workspace_bytes")}
    assert set(COVERED_BY) == exported, (sorted(exported - set(COVERED_BY)), sorted(set(COVERED_BY) - exported))
    assert set(COVERED_BY.values()) == set(FAMILIES)
    L = _C.lib()
    for name in COVERED_BY:                                                # bound, with a size_t result
        assert getattr(L, name).restype is _C.c_size_t


@pytest.mark.parametrize("nbytes", [-3, 0, 1, 16, 17, 255, 65535, 65536, 65537, 100001, (8 << 20) - 1, 8 << 20,
                                    (8 << 20) + 1, 100 << 20])
def test_arena_layout(nbytes):
    front, n, back = mg.layout(nbytes)
    assert n == max(nbytes, 16)                                            # the payload's length, as _C.workspace has it
    assert front % 256 == 0 and front % 16 == 0
    for band in (front, back):
        assert band >= min(max(64 << 10, n), 8 << 20) and band <= 8 << 20  # an overrun of up to 100 % stays inside
    if n <= 8 << 20:
        assert front >= n and back >= n


def test_fills_and_guard_byte():
    assert mg.FILLS == (0x00, 0xA5, 0xFF) and mg.GUARD not in mg.FILLS
    assert np.array([0xA5] * 4, np.uint8).view(np.float32)[0] < 0 and np.isfinite(np.array([0xA5] * 4, np.uint8).view(np.float32)[0])
    assert np.array([0xA5] * 4, np.uint8).view(np.int32)[0] < -(1 << 30)
    assert np.isnan(np.array([0xFF] * 4, np.uint8).view(np.float32)[0]) and np.array([0xFF] * 4, np.uint8).view(np.int32)[0] == -1
    assert max(mg.SMALL_SIZES) <= 1 << 20 and min(mg.LARGE_SIZES) > 1 << 20


# ==================================================================================================== families ==
# Each takes (fill, tools) and returns None or {name: numpy array} of raw outputs to be compared across the fills.

# ---------------------------------------------------------------------------------------------- BatchNorm ------
BN_SHAPES = [(2, 3, 8192 + 4), (2, 3, 8192 + 3), (1, 1, 1)]     # (B, C, HW): SEG = 8192 floats a workgroup segment; two segments
#                                                                  with a ragged tail on the float4 path (HW % 4 == 0) and on
#                                                                  the scalar path, and the smallest input
BN_VARIANTS = [(True, True), (False, True), (False, False), (True, False)]     # (relu, residual); the last: the RECOMP kernels


def _bn_reference(x, res, gout, w, b, rm, rv, momentum, eps, relu):
    """Training-mode BatchNorm (+ residual) (+ ReLU) and its gradients in float64.  The running variance takes the
    unbiased estimate, which with a single value per channel is the biased one (batchnorm.hip's `N > 1 ? ... : var`)."""
    x, gout, w, b = x.astype(np.float64), gout.astype(np.float64), w.astype(np.float64), b.astype(np.float64)
    N = x.shape[0] * x.shape[2]
    mean = x.mean((0, 2))
    var = x.var((0, 2))
    invstd = 1.0 / np.sqrt(var + eps)
    xhat = (x - mean[None, :, None]) * invstd[None, :, None]
    pre = xhat * w[None, :, None] + b[None, :, None]
    if res is not None:
        pre = pre + res.astype(np.float64)
    y = np.maximum(pre, 0) if relu else pre
    g = gout * (pre > 0) if relu else gout
    gb = g.sum((0, 2))
    gw = (g * xhat).sum((0, 2))
    gx = (w * invstd)[None, :, None] * (g - gb[None, :, None] / N - xhat * gw[None, :, None] / N)
    new_rm = (1 - momentum) * rm.astype(np.float64) + momentum * mean
    new_rv = (1 - momentum) * rv.astype(np.float64) + momentum * (var * N / (N - 1) if N > 1 else var)
    return {"y": y, "pre": pre, "rm": new_rm, "rv": new_rv, "gx": gx, "gw": gw, "gb": gb, "gres": g}


def _bn_inputs(shape, relu, with_res):
    """Seeded inputs whose pre-activations all stay 1e-4 away from the ReLU's threshold, so that the float32 kernel and
    the float64 reference cut the same elements."""
    B, C, HW = shape
    for seed in range(64):
        rng = np.random.RandomState(1000 * HW % 9973 + 10 * seed + 2 * relu + with_res)
        x = (0.3 + 1.7 * rng.standard_normal(shape)).astype(np.float32)
        res = rng.standard_normal(shape).astype(np.float32) if with_res else None
        gout = rng.standard_normal(shape).astype(np.float32)
        w = rng.uniform(0.5, 1.5, C).astype(np.float32)
        b = rng.standard_normal(C).astype(np.float32)
        rm = rng.standard_normal(C).astype(np.float32)
        rv = rng.uniform(0.5, 2.0, C).astype(np.float32)
        ref = _bn_reference(x, res, gout, w, b, rm, rv, 0.1, 1e-5, relu)
        if not relu or np.abs(ref["pre"]).min() > 1e-4:
            return x, res, gout, w, b, rm, rv, ref
    raise AssertionError("no seed keeps the pre-activations away from zero")


def family_batchnorm(fill, tools):
    """cp_bn_act_forward_train / cp_bn_act_backward at the tolerances of test_fused_bn_act_vs_torch."""
    import torch
    from centerpoly_amd.models.networks.pose_dla_dcn import _BnAct
    dev = torch.device("cuda")
    close = np.testing.assert_allclose
    for shape in BN_SHAPES:
        B, C, HW = shape
        for relu, with_res in BN_VARIANTS:
            x, res, gout, w, b, rm, rv, ref = _bn_inputs(shape, relu, with_res)
            t = lambda a, grad=False: torch.from_numpy(a.reshape(a.shape[:2] + (1, -1)) if a.ndim == 3 else a) \
                .to(dev).requires_grad_(grad)                              # noqa: E731
            xd, wd, bd = t(x, True), t(w, True), t(b, True)
            rd = t(res, True) if with_res else None
            rmd, rvd = t(rm), t(rv)
            yd = _BnAct.apply(xd, wd, bd, rd, rmd, rvd, 0.1, 1e-5, relu)
            yd.backward(t(gout))
            what = "%s relu=%s residual=%s" % (shape, relu, with_res)
            flat = lambda v: v.detach().cpu().numpy().reshape(B, C, HW)    # noqa: E731
            close(flat(yd), ref["y"], rtol=1e-4, atol=1e-5, err_msg=what)
            close(rmd.cpu().numpy(), ref["rm"], rtol=1e-5, atol=1e-6, err_msg=what)
            close(rvd.cpu().numpy(), ref["rv"], rtol=1e-5, atol=1e-6, err_msg=what)
            gs = np.abs(ref["gx"]).max()
            close(flat(xd.grad), ref["gx"], rtol=1e-3, atol=1e-5 * max(gs, 1.0), err_msg=what)
            close(wd.grad.cpu().numpy(), ref["gw"], rtol=1e-4, atol=1e-4, err_msg=what)
            close(bd.grad.cpu().numpy(), ref["gb"], rtol=1e-4, atol=1e-4, err_msg=what)
            if with_res:
                close(flat(rd.grad), ref["gres"], rtol=0, atol=0, err_msg=what)


# ------------------------------------------------------------------------------------------------- losses ------
# a 256-thread block spans 1024 elements of the focal kernels (float4 a thread) and 256 of the MSE / dense-L1 ones; one
# element past FOCAL_MAX_BLOCKS (2048) and MSE_BLOCKS (1024) blocks is 8 MiB and 1 MiB of floats: well within a second
FOCAL_COUNTS = [1, 1023, 1025, 2048 * 1024 + 4 + 1]
STREAM_COUNTS = [1, 255, 257, 1024 * 256 + 1]


def _loss_inputs(n, seed):
    rng = np.random.RandomState(seed + n % 1000)
    x = rng.standard_normal(n).astype(np.float32) * 2
    gt = (rng.random_sample(n) ** 4).astype(np.float32) * np.float32(0.999)
    gt[:: max(n // 7, 1)] = 1.0                                             # positives, the first element among them
    mask = (rng.random_sample(n) < 0.3).astype(np.float32)
    return x, gt, mask


def family_losses(fill, tools):
    """Focal, MSE and dense L1 at their block spans, gather L1 and the polygon IoU / order terms, against the oracle at
    the tolerances of test_gpu_parity.py and test_catspec_dense.py."""
    import torch
    import test_gpu_parity as tp
    from centerpoly_amd.models import losses
    from oracle import losses as olos
    close = np.testing.assert_allclose
    for n in FOCAL_COUNTS:
        x, gt, _ = _loss_inputs(n, 1)
        xc = torch.from_numpy(x).requires_grad_(True)
        ref = olos.neg_loss(olos.sigmoid_clamp(xc), torch.from_numpy(gt))
        ref.backward()
        xd = torch.from_numpy(x).cuda().requires_grad_(True)
        loss, act = losses.sigmoid_focal_loss(xd.clone(), torch.from_numpy(gt).cuda())
        loss.backward()
        close(loss.item(), ref.item(), rtol=1e-4, err_msg="focal n=%d" % n)
        gs = xc.grad.abs().max().item()
        close(xd.grad.cpu().numpy(), xc.grad.numpy(), rtol=1e-3, atol=1e-5 * gs, err_msg="focal n=%d" % n)
        close(act.detach().cpu().numpy(), olos.sigmoid_clamp(torch.from_numpy(x)).numpy(), rtol=1e-5, atol=1e-7)
    for n in STREAM_COUNTS:
        x, gt, mask = _loss_inputs(n, 2)
        # the oracle's expressions (F.mse_loss; oracle.losses.dense_poly_l1) with every float32 product as the tensor
        # expression rounds it and the sum carried in float64
        d = x - gt
        xd = torch.from_numpy(x).cuda().requires_grad_(True)
        loss = losses.MSELoss()(xd, torch.from_numpy(gt).cuda())
        loss.backward()
        close(loss.item(), (d * d).astype(np.float64).sum() / n, rtol=1e-5, err_msg="mse n=%d" % n)
        close(xd.grad.cpu().numpy(), 2.0 * d.astype(np.float64) / n, rtol=1e-5, atol=1e-10, err_msg="mse n=%d" % n)
        den = np.float32(mask.astype(np.float64).sum()) + np.float32(1e-4)
        diff = x * mask - gt * mask
        pd = torch.from_numpy(x).cuda().requires_grad_(True)
        loss = losses.dense_poly_l1_loss(pd, torch.from_numpy(gt).cuda(), torch.from_numpy(mask).cuda())
        loss.backward()
        close(loss.item(), np.float32(np.abs(diff).astype(np.float64).sum()) / den, rtol=1e-6, err_msg="dense n=%d" % n)
        want = (np.sign(diff) * mask / den).astype(np.float32)
        got = pd.grad.cpu().numpy()
        assert np.array_equal(got != 0, want != 0), "dense n=%d" % n
        close(got, want, rtol=1e-6, atol=0, err_msg="dense n=%d" % n)
        if n <= 257:                                                        # and the oracle's own float32 sums where they are short
            ref = olos.dense_poly_l1(torch.from_numpy(x), torch.from_numpy(gt), torch.from_numpy(mask))
            close(loss.item(), ref.item(), rtol=1e-5)
    _run(tp.test_gather_l1_duplicate_centres_accumulate)
    for key in ("reg", "pseudo_depth"):
        _run(tp.test_regl1_vs_golden, key, _golden)
        _run(tp.test_regsl1_vs_golden, key, _golden)
    for case in tp.IOU_ORDER:                                               # IoU, order and their sum, every representation
        _run(tp.test_polyloss_iou_and_order_vs_reference_golden, case, _golden)
    _run(tp.test_polyloss_many_random_objects_vs_oracle)


# ------------------------------------------------------------------------------------------------ targets ------
def _zero_height(ann):
    a = dict(ann)
    a["bbox"] = [a["bbox"][0], a["bbox"][1], a["bbox"][2], 0.0]
    return a


def _target_images(N, M):
    """[(annotations, flipped)]: no object, more objects than slots, fewer, and a zero-height object in the first slot."""
    from centerpoly_amd import synth
    few = synth.raw_annotations("mc/few%d" % N, 128, 256, nbr_points=N, n_objs=3)
    flat = [_zero_height(few[0])] + few[1:]
    many = synth.raw_annotations("mc/many%d" % N, 128, 256, nbr_points=N, n_objs=M + 5)
    if M > 1:
        many[M // 2] = _zero_height(many[M // 2])
    return [([], False), (many, N >= 4), (few, False), (flat, False)]   # (the flip re-orders from 4 vertices on)


def _compare_targets(out, b, ref, tt, ell_hm=None):
    """The rules of test_targets._compare (and of the elliptical tests for an elliptical hm), border_hm optional."""
    assert np.array_equal(out["reg_mask"][b], ref["reg_mask"]) and np.array_equal(out["ind"][b], ref["ind"])
    assert np.array_equal(out["pseudo_depth"][b], ref["pseudo_depth"])
    for k in ("peak", "reg", "wh", "poly"):
        if k in out:
            assert tt._ulp_close(out[k][b], ref[k]), k
    for k in ("hm", "border_hm"):
        if k not in out:
            continue
        if k == "hm" and ell_hm is not None:
            assert np.array_equal(out[k][b], ell_hm), "elliptical hm"
            continue
        assert np.array_equal(out[k][b] > 0, ref[k] > 0), k
        assert tt._ulp_close(out[k][b], ref[k]), k
        assert np.array_equal(out[k][b] == 1.0, ref[k] == 1.0), k
    np.testing.assert_allclose(out["freq_mask"][b], ref["freq_mask"], rtol=1e-6)


def family_targets(fill, tools):
    """cp_polydet_targets_ex / cp_polydet_dense_targets against oracle/targets.py: max_objs 1 and 65, no object and more
    than max_objs, a zero-height object, 3 and 16 vertices, with and without border_hm, dense_poly and elliptical_gt."""
    import test_elliptical_targets as te
    import test_targets as tt
    from centerpoly_amd.datasets.sample.polydet import build_targets, collate, pack_annotations
    from oracle import post as opost
    from oracle import targets as otg
    oh, ow, C = 32, 64, 8
    # 128 x 256 -> 32 x 64, axis-aligned with a power-of-two scale: x' = 0.25 x + 1.92 is one correctly rounded sum in
    # whatever order, fused or not, the host's BLAS runs np.dot in affine_transform, so the float32 centre (and reg, its
    # fractional part, held to ONE ulp of itself) is defined to the bit.  get_affine_transform's matrices carry 1e-17
    # off-diagonal terms; the centres of these 16-gons then land on float32 rounding ties often enough (object 25 of
    # the 70) that the order of np.dot's three-term sum, which is the BLAS kernel's business, decides reg.
    t = np.array([[0.25, 0.0, 1.92], [0.0, 0.25, -1.6]], np.float64)
    assert np.allclose(t, opost.get_affine_transform(np.array([256 * 0.47, 128 * 0.55], np.float32), 256.0, 0, [ow, oh]),
                       rtol=0, atol=1e-6)
    kept = {}
    for M, N in ((65, 16), (1, 3), (1, 16), (65, 3)):
        images = _target_images(N, M)
        raw = {k: v.cuda() for k, v in collate([pack_annotations(a, t, fl, 256, M, N) for a, fl in images]).items()}
        for border, dense, ell in ((True, False, False), (False, True, False), (True, True, True), (False, False, True)):
            out = build_targets(raw, oh, ow, C, with_border_hm=border, dense_poly=dense, elliptical_gt=ell)
            assert ("border_hm" in out) == border and ("dense_poly" in out) == dense and ("poly" in out) == (not dense)
            out = {k: v.cpu().numpy() for k, v in out.items()}
            for b, (anns, fl) in enumerate(images):
                ref = otg.build_targets(anns, t, fl, 256, oh, ow, C, M, N, "cartesian", dense_poly=dense)
                r = te.elliptical_targets(anns, t, fl, 256, oh, ow, C, M, N, "cartesian", dense_poly=dense) if ell else ref
                _compare_targets(out, b, ref, tt, r["hm"] if ell else None)
                if not anns:                                                # the rows of empty slots, the whole image here
                    for k, v in out.items():
                        assert not v[b].any() or k == "freq_mask", k
                if dense:
                    px = (out["dense_poly_mask"][b] != r["dense_poly_mask"]).any(axis=0)
                    assert px.sum() <= 2, (M, N, b, int(px.sum()))
                    np.testing.assert_allclose(out["dense_poly"][b][:, ~px], r["dense_poly"][:, ~px], rtol=2.4e-7, atol=1e-5)
            for k in ("reg_mask", "ind", "pseudo_depth"):                   # bit-exact in the existing check
                kept["%d/%d/%d%d%d/%s" % (M, N, border, dense, ell, k)] = out[k]
    for case in ("cart_dense", "cart_catspec", "polar_flip"):              # and the reference sampler's own arrays
        _run(tt.test_device_targets_match_reference_sampler, case, _golden)
    _run(te.test_device_elliptical_targets_match_reference_sampler, "ell_cart_dense", _golden)
    return kept


# ---------------------------------------------------------------------------------------- training inputs ------
def family_training_inputs(fill, tools):
    """cp_sample_inputs_batch at dst 5 x 257 (two x-blocks of 256, the second one column wide) with 17 images (one more
    than a launch carries) of different sizes, 1 x 1 among them, colour augmentation on for some: every image against
    the per-image path (the warp and cp_color_aug_normalize) and oracle/pre.py as in test_ragged_batches.py."""
    import torch
    import test_ragged_batches as tr
    from centerpoly_amd.datasets.sample.polydet import build_inputs_batch
    from oracle import pre as opre
    dev = torch.device("cuda")
    H, W = 5, 257
    sizes = [tr.SIZES[i % 3] for i in range(17)]
    sizes[5] = (1, 1)
    images = tr._sources(tuple(sizes), seed=41)
    rng = np.random.RandomState(42)
    trans = tr.TRANS[np.arange(17) % 3].copy()
    trans[:, 2] += rng.uniform(-8, 8, 17)
    trans[:, 5] += rng.uniform(-3, 3, 17) - 8.0                              # the 5 rows look at the sources' upper part
    trans[5] = (40.0, 0, 100.0, 0, 2.0, 1.0)
    color = np.zeros((17, 10), np.float64)
    for b in range(17):
        if b % 4 != 1:
            color[b] = [1, *tr.ORDERS[b % 6], *rng.uniform(0.6, 1.4, 3), *rng.uniform(-0.03, 0.03, 3)]
    flat, hw, off = tr._flat(images, dev)
    out = build_inputs_batch(flat, hw, off, trans, color, tr.MEAN, tr.STD, H, W)
    assert torch.equal(out, build_inputs_batch(flat, hw, off, trans, color, tr.MEAN, tr.STD, H, W))
    out = out.cpu().numpy()
    assert out.shape == (17, 3, H, W) and np.isfinite(out).all()
    single = tr._per_image(images, trans, color, H, W, dev)
    for b in range(17):
        warp = (opre.warp_affine_u8(images[b], trans[b].reshape(2, 3), (W, H)) / 255.).astype(np.float32)
        ref = opre.color_aug_normalize(warp, color[b, 1:4].astype(int), color[b, 4:7], color[b, 7:10], tr.MEAN, tr.STD,
                                       color_on=bool(color[b, 0]))
        np.testing.assert_allclose(out[b], ref, rtol=1e-6, atol=1e-5, err_msg=str(b))
        np.testing.assert_allclose(out[b], single[b], rtol=1e-6, atol=1e-5, err_msg=str(b))
        if not color[b, 0]:
            assert np.array_equal(out[b], single[b]), b                     # colour off: operation for operation
    _run(tr.test_batch_kernel_matches_per_image_path_and_oracle, 1)
    _run(tr.test_equal_sizes_match_build_inputs)
    return {"batch": out}                                                   # no atomics: the same bits whatever the memory held


# ------------------------------------------------------------------------------------------------- decode ------
# (C, H, W, K, N): K = 1; the most winners a call takes; H * W below K; C * H * W one past the S1_TILE of 4096 keys; the
# widest rows (N2 = 2 N = 128)
DECODE_SHAPES = [(3, 9, 11, 1, 4), (3, 24, 40, 256, 4), (8, 4, 5, 32, 4), (1, 17, 241, 40, 4), (2, 16, 20, 20, 64)]


def _decode(C, H, W, K, N):
    import torch
    import test_gpu_parity as tp
    from centerpoly_amd import synth
    heat = torch.sigmoid(torch.from_numpy(synth.heat_logits("mc/dec%dx%dx%d" % (C, H, W), 2, C, H, W)))
    ref, rinds, rcls, dets, inds, clses = tp._decode_both(heat, N=N, K=K)
    assert torch.equal(inds, rinds) and torch.equal(clses, rcls) and torch.equal(dets, ref), (C, H, W, K, N)
    return dets.numpy()


def family_decode(fill, tools):
    import test_gpu_parity as tp
    kept = {"%dx%dx%d_K%d_N%d" % s: _decode(*s) for s in DECODE_SHAPES}
    for kind in ("constant", "sparse", "ragged"):
        _run(tp.test_decode_ties_and_edge_inputs, kind)
    _run(tp.test_decode_vs_oracle_and_golden, tp.cases.DECODE_CASES[2], _golden)       # polar: the tolerance of that test
    return kept


# ------------------------------------------------------------ merge, soft-NMS, mask NMS, polygon overlaps ------
def _polygon_rows(tag, S, K, C, H, W, N=8):
    """Rows [S, K, 2 N + 7] of star-shaped N-gons on an H x W canvas (some hang over its edge, all overlap their
    neighbours), scores in (0.05, 1), classes 0 .. C - 1, a depth that tells the rows apart."""
    rng = np.random.RandomState(sum(map(ord, tag)) + 1000 * S + K + 7 * C)
    R = S * K
    rows = np.zeros((R, 2 * N + 7), np.float32)
    ang = np.arange(N) * (2 * np.pi / N)
    for r in range(R):
        cx, cy = rng.uniform(-2, W + 2), rng.uniform(-2, H + 2)
        rad = rng.uniform(3, min(H, W) / 2.0, N)
        pts = np.stack([cx + rad * np.cos(ang), cy + rad * np.sin(ang)], 1)
        rows[r, 6:6 + 2 * N] = np.round(pts.reshape(-1), 2)
        rows[r, 0:4] = [pts[:, 0].min(), pts[:, 1].min(), pts[:, 0].max(), pts[:, 1].max()]
    rows[:, 4] = rng.uniform(0.05, 1.0, R)
    rows[:, 5] = rng.randint(0, C, R)
    rows[:, -1] = 1.0 + np.arange(R)
    return rows.reshape(S, K, -1)


def _mask_merge_shapes(tm):
    """cp_merge_detections_mask and cp_polygon_overlaps at S * K of 1 and of 65 (one past a 64-row wave), 1 and 64
    classes, max_per_image above and below the kept count, against the host statement (tests/golden/mask_nms_host.py,
    its masks drawn by the scan-line transcription that the CPU tests hold against PIL) bit for bit; tm._merge_device
    brings the check that nothing is written beyond the kept rows."""
    import pil_scanline_host as scan
    H, W = 48, 64
    fill = lambda pts, h, w: np.asarray(scan.fill(pts, w, h)) != 0          # noqa: E731
    kept = {}
    for S, K, C in ((1, 1, 1), (1, 65, 1), (5, 13, 64), (1, 65, 64), (1, 1, 64)):
        rows = _polygon_rows("mask", S, K, C, H, W)
        area, inter = tm.host.overlaps(rows, C, H, W, fill=fill)
        assert area.max() > 0
        got_area, got_inter = tm._overlaps_device(rows.reshape(S * K, -1), C, H, W)
        assert np.array_equal(got_area, area) and np.array_equal(got_inter, inter), (S, K, C)
        for mpi in (100, 7):
            par = (mpi, 0.5, 0.5, 0.001, 2)
            want, want_counts = tm.host.mask_nms(rows, C, area, inter, mpi, 0.5, 0.5, 0.001, 2)
            got, counts = tm._merge_device(rows, C, H, W, par)
            assert counts.tolist() == want_counts.tolist(), (S, K, C, mpi)
            assert tm._same_bits(got, want), (S, K, C, mpi, tm._report(got, want))
            assert K == 1 or ((counts[0] >= 7 and counts[0] < S * K) if mpi == 7 else counts[0] > 7), (S, K, C, mpi, counts[0])
            kept["mask_%d_%d_%d_%d" % (S, K, C, mpi)] = got
    return kept


def family_merge_nms(fill, tools):
    """test_merge_device.py and test_mask_nms.py with their sentinel checks; S * K of 1 and of 65 (one past a 64-row
    wave), max_per_image below and above the kept count, 1 and 64 classes."""
    import test_mask_nms as tm
    import test_merge_device as td
    kept = {}
    for S, K, C, mpi in ((1, 65, 1, 100), (1, 65, 1, 7), (5, 13, 64, 100), (5, 13, 64, 7), (1, 1, 64, 100)):
        rows = td._merge_rows("mc%d_%d_%d" % (S, K, C), S=S, K=K, C=C)
        want, want_counts = td._merge_reference(rows, C, mpi, 1)
        got, counts = td._merge_device(rows, C, mpi, 1)
        assert counts.tolist() == want_counts.tolist(), (S, K, C, mpi)
        assert td._same_bits(got, want), (S, K, C, mpi)
        assert (mpi <= counts[0] < S * K) if mpi == 7 else (K == 1 or counts[0] > 7)       # cut, and not cut
        kept["%d_%d_%d_%d" % (S, K, C, mpi)] = got
    kept.update(_mask_merge_shapes(tm))
    for case in sorted(td.MERGE_CASES):
        _run(td.test_merge_detections_matches_the_oracle_bitwise, case)
    _run(td.test_soft_nms_device_segments_with_gaps)
    for name in ("m0_s1", "m1_s2", "m2_s3", "ties", "cut_ties", "cut_one", "threshold"):
        _run(tm.test_merge_detections_mask_matches_the_host_statement_bitwise, name)
    _run(tm.test_every_output_row_is_one_input_row)
    for name in ("canvas_1x1", "rows_1", "rows_63", "rows_64", "rows_65", "random_n3_37x53", "triangles_n3", "width_33"):
        _run(tm.test_polygon_overlaps_match_pil, name)
    return kept


# ---------------------------------------------------------------------------------------------- RLE, PNG ------
def family_rle_png(fill, tools):
    """The degenerate canvases, the tile edges and the capacities (exact, short, zero: the head reports, nothing is
    written past the capacity) of test_rle.py and test_png.py."""
    import test_png as tg
    import test_rle as tr
    _run(tr.test_degenerate_canvases)
    for H in (7, 65):
        for W in (63, 64, 65):
            _run(tr.test_tile_edges, H, W)
    _run(tr.test_uniform_planes_and_the_first_pixel)
    _run(tr.test_the_carry_between_columns)
    _run(tr.test_bounds)
    _run(tr.test_index_mode, 1)
    _run(tr.test_capacities, tools.monkeypatch)
    tools.monkeypatch.undo()
    _run(tr.test_decode_zero_length_runs_and_wrong_sums)
    for name in ("one_pixel", "one_pixel_16", "W1", "H1", "zeros", "ids16_odd", "labels8", "noise", "noise16"):
        _run(tg.test_the_cases_of_the_statement, name)
    for W in (15, 16, 17):
        _run(tg.test_piece_tails_and_runs_across_row_ends, W)
    _run(tg.test_planes_of_different_contents, 1)
    _run(tg.test_bounds_given_empty_and_null)
    _run(tg.test_capacities, tools.monkeypatch)
    tools.monkeypatch.undo()


# -------------------------------------------------------------------------------------------------- track ------
def family_track(fill, tools):
    """cp_map_pairs(_shifted), associate, update, predict and kinematics against tracking_host.py and
    tracking_motion_host.py: n of 0, 1 and 128, and 257 tracks alive."""
    import test_tracking as tt
    import test_tracking_motion as tm
    for name in ("unaligned", "one_pair", "lookup", "lds_128", "lds_bound", "past_bound"):
        _run(tt.test_map_pairs, name)
    _run(tt.test_association_ties_and_equal_fractions)
    _run(tt.test_association_threshold_boundary)
    _run(tt.test_association_label_mismatch_and_dead_instance)
    _run(tt.test_association_max_age_with_a_track_hidden_for_two_frames, 3, 1)
    _run(tt.test_association_with_257_tracks_alive_changes_nothing)
    sequence = tt.build_sequence("cityscapes")                             # six whole steps: update included
    _run(tt.test_whole_steps_against_the_host_statement, sequence)
    for shape, table in (("1x1", "lds"), ("37x53_unaligned", "lds"), ("37x53_unaligned", "global"), ("9x21", "no_columns"),
                         ("9x21", "no_rows")):
        _run(tm.test_map_pairs_shifted, shape, table)
    _run(tm.test_a_negative_none_row)
    for offset in (False, True):
        _run(tm.test_kinematics_cases, offset)                              # n = 6 and n = 0
    _run(tm.test_a_freed_slot_is_reused_without_its_kinematics)            # n = 0 and 1 through the tracker: predict, update
    _run(tm.test_more_than_256_tracks_alive_changes_nothing)               # n = 128, and the 257th track
    _run(tm.test_the_tracker_on_the_scenario)


# ------------------------- instance map / overlaps, boundary overlaps, segment medians, confusion, panoptic ------
def _overlap_corners(ta):
    """cp_instance_overlaps with no mask, one mask, no id of interest and one, on the 37 x 53 scene of test_instance_ap
    against its numpy_counts.  With G == 0 the id table holds nothing but `no column` and the void marks, and void_inter
    and pred_pixels are all a call writes; with n == 0 it writes nothing."""
    import torch
    from centerpoly_amd.datasets.evaluation import instance_level as il
    gt, masks, inst = ta._scene(37, 53, 9, 12, seed=37 * 7 + 53)
    full = 9 // 3                                                           # the all-ones mask of the scene
    assert masks[full].all() and masks[1].any() and not masks[1].all()
    g_dev = ta._dev_ids(gt)
    kept = {}
    for name, sel, ids in (("n0", slice(0, 0), inst), ("n1", slice(1, 2), inst), ("n1_full", slice(full, full + 1), inst),
                           ("G0", slice(0, 9), []), ("G0_n1", slice(full, full + 1), []), ("G1", slice(0, 9), inst[5:6]),
                           ("n0_G0", slice(0, 0), [])):
        m = np.ascontiguousarray(masks[sel])
        got = il.device_counts(torch.from_numpy(m).cuda(), g_dev, ids)
        want = ta.numpy_counts(m, gt, ids, il.VOID_IDS)
        for a, b, what in zip(got, want, ("inter", "void", "pixels")):
            assert a.shape == b.shape and np.array_equal(a, b), (name, what)
            kept["overlaps_%s_%s" % (name, what)] = a
        if m.shape[0]:
            assert want[2].sum() > 0 and (name != "n1_full" or want[1][0] > 0)
    return kept


def family_pixel_counts(fill, tools):
    """n and G of 0 and 1 and the 37 x 53 canvas of the existing tests, against their host statements.  conf and bad of
    cp_pixel_confusion ADD: they start from known non-zero values and must end at start + reference."""
    import test_boundary as tb
    import test_instance_ap as ta
    import test_instance_map as ti
    import test_panoptic as tq
    import test_pixel_level as tl
    import test_segment_median as ts
    for shape in ((5, 37, 53), (1, 1, 1)):
        for variant in ("plain", "full"):
            _run(ti.test_kernel_equals_the_restatement, shape, variant)
    _run(ti.test_kernel_with_no_instance_fills_the_maps)
    _run(ti.test_kernel_leaves_null_outputs_alone_and_takes_another_background)
    _run(ta.test_kernels_reproduce_the_recorded_counts, ta.ODD)
    for H, W, n, G in ((1, 1, 3, 2), (37, 53, 9, 12), (37, 53, 2, 1)):
        _run(ta.test_kernels_equal_numpy_at_scale_and_odd_sizes, H, W, n, G)
    kept = _overlap_corners(ta)
    for name in ("1x1", "37x53_d1", "37x53_d2", "37x53_d11", "24x40_n0_d2", "24x40_G0_d2", "20x17_shapes_d2",
                 "45x83_bounds_d2"):
        _run(tb.test_bands_and_tables_against_the_host_statement, name)
    _run(tb.test_two_runs_give_the_same_bits)
    _run(ts.test_every_path_on_37x53)
    _run(ts.test_no_segment_is_a_no_op)
    # pixel confusion: conf and bad add
    ids, pred = tl.gt_ids("odd37x53", "cityscapes"), tl.rec("odd37x53")["pred"]
    label = tl.IDENTITY.copy()
    label[26] = 200                                                         # cars map outside the table: bad[1] counts
    inst_ids = tl.interest(ids)
    conf0 = np.arange(34 * 34, dtype=np.int64).reshape(34, 34) * 3 + 7
    bad0 = np.array([11, 5], np.int64)
    one = tl.want(pred, ids, inst_ids, pred_label=label)
    assert one[2][1] > 0 and one[0].sum() > 0
    got = tl.run_kernel(pred, ids, inst_ids, pred_label=label, conf=conf0, bad=bad0, inst_fill=-7)
    assert np.array_equal(got[0], conf0 + one[0]) and np.array_equal(got[2], bad0 + one[2]) and np.array_equal(got[1], one[1])
    for inst in ([], [int(inst_ids[0])]):                                   # G = 0 (with NULL tables too) and G = 1
        tl.same(tl.run_kernel(pred, ids, inst), tl.want(pred, ids, inst))
    tl.same(tl.run_kernel(pred, ids, [], null_tables=True)[::2], tl.want(pred, ids, [])[::2])
    for shape in ((1, 1), (1, 17), (19, 1)):
        _run(tl.test_tiny_shapes, shape)
    _run(tl.test_accumulation)
    _run(tl.test_bad_labels_of_both_kinds)
    # panoptic pairs and match
    for name in tq.CASES:
        _run(tq.test_fixtures_from_unaligned_buffers, name)
    for shape in ((1, 1), (1, 17), (19, 1)):
        _run(tq.test_tiny_shapes, shape)
    _run(tq.test_no_slots_and_all_void)                                     # n = 0
    _run(tq.test_small_table_regime)
    _run(tq.test_more_than_1024_segments)
    _run(tq.test_accumulation_and_order)
    kept.update({"conf": got[0], "inst": got[1], "bad": got[2]})
    return kept


# -------------------------------------------------------------------------------------------- rasterisers ------
def family_rasterisers(fill, tools):
    """Polygon masks, polygon paint, class masks, result writer, writer instances, render overlay, annotation rays and
    ids: one polygon case each from their tests, no polygon at all, and a polygon wholly outside the canvas."""
    import torch
    import test_annotations as ta
    import test_class_masks as tc
    import test_ground_truth as tg
    import test_render as tr
    import test_result_writer as tw
    import test_writer_instances as ti
    from centerpoly_amd.datasets import annotate, ground_truth
    za, zg = ta.load_fixture(), tg.load_fixture()
    for name in ("one", "shapes", "many129"):
        _run(ta.test_id_instances_kernel, za, name)
        _run(ta.test_rays_ids_kernel, za, name)
    _run(ta.test_id_instances_reports_more_than_max_inst, za)
    for name in ("small", "idd"):
        _run(ta.test_polygon_masks_kernel, za, name)
        _run(ta.test_rays_masks_kernel, za, name)
    for name in ("two_vertex", "floats", "pixel", "none", "one", "column", "row", "overlap"):
        _run(tg.test_gpu_paint_equals_the_fixture, zg, name)
    _run(tg.test_gpu_paint_is_deterministic_and_stays_on_the_canvas, zg)
    # no polygon, and polygons wholly outside the canvas (left, below, and around it without touching: a ring's hole is
    # not modelled, so the last one is a triangle far to the right): nothing but the background
    W, H = 53, 37
    outside = [np.array([[-30, 5], [-2, 9], [-10, 30]], np.int32), np.array([[5, H + 1], [40, H + 9], [20, H + 30]], np.int32),
               np.array([[W + 1, -5], [W + 40, 10], [W + 3, 60]], np.int32)]
    for polygons in ([], outside):
        image = ground_truth.paint(polygons, list(range(1, len(polygons) + 1)), 9, (W, H), "cuda")
        assert tuple(image.shape) == (H, W) and bool((image == 9).all())
    objects = [{"label": "car", "polygon": [[float(x), float(y)] for x, y in p]} for p in outside]
    for objs in ([], objects):
        got = annotate.from_polygons(objs, (W, H), {"car"}, 16, device="cuda")
        assert got["counts"].tolist() == [0] * len(objs) and got["poly"].shape == (len(objs), 16, 2)
    for args in ((97, 61, 16, 0), (2, 3, 3, 3)):
        _run(tc.test_masks_equal_the_transcription_on_random_polygons, *args)
        _run(tc.test_wave_and_workgroup_scan_lines_agree, *args)            # class masks, polygon masks and paint together
    _run(tc.test_masks_equal_the_fixtures, "odd")
    for mode in (0, 1):
        _run(tc.test_selection_kernel, "odd", mode)
    _run(tw.test_device_masks_equal_pil_fixtures, "small16", tools.tmp_path)
    _run(ti.test_kernel_against_the_recorded_writer, "small16")
    _run(ti.test_vertex_rule_equals_the_text_form)
    for name in ("generated_37x53", "class_writer_odd", "generated_375x1242"):
        _run(tr.test_overlay_equals_the_host_statement, name)
    _run(tr.test_overlay_boxes_only_and_other_outline_colour)
    _run(tr.test_overlay_nothing_live_and_too_many)                        # n = 0
    _run(tr.test_debugger_draws_what_the_statement_draws, tools.tmp_path)  # the wrapper's own workspace
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------- DCN ------
def family_dcn(fill, tools):
    """The smallest entries of DCN_SHAPES, BF16X3_SHAPES and REGION_SHAPES and the K-split ones next to them, the fused
    module, the slices form, the backward in every mode, and cp_conv_mfma_input_grad_relu, against the oracle at the
    existing tolerances.  (The `prepared` forms keep their workspace between calls on purpose: it is filled once, when
    it is allocated.)"""
    import test_conv_mfma as tc
    import test_gpu_parity as tp
    import test_up_slices as tu
    from centerpoly_amd.models.networks.DCNv2.dcn_v2 import DCN
    for shape in ((2, 9, 33, 5, 3), (1, 512, 256, 8, 16)):                 # the smallest; small and wide: K is split
        _run(tp.test_dcn_forward_vs_oracle, shape)
    for shape in ((2, 24, 40, 13, 19), (1, 512, 64, 8, 16)):
        _run(tp.test_dcn_forward_split_bf16_contraction, shape)
    for shape in ((1, 16, 20, 9, 7), (1, 256, 128, 16, 32)):
        _run(tp.test_dcn_forward_region_kernel, shape, 2.0)
    _run(tp.test_dcn_module_fused_offset_conv, (1, 16, 64, 128, 256), 0.4)
    _run(tu.test_idaup_fold_slices_is_bit_identical)
    keep = DCN.backward_flags
    try:
        for flags in (0, _C.DCN_BWD_NARROW_TILES, _C.DCN_BWD_EXACT_F32):
            DCN.backward_flags = flags
            _run(tp.test_dcn_backward_vs_oracle_autograd, tp.DCN_BWD_SHAPES[0])
            _run(tp.test_dcn_backward_vs_oracle_autograd, (1, 16, 24, 6, 64))          # a channel-split plan
    finally:
        DCN.backward_flags = keep
    _run(tp.test_dcn_backward_fallback_kernels_vs_oracle_autograd, tp.DCN_BWD_FALLBACK_CASES[0])
    _run(tp.test_dcn_backward_overwrites_grad_x_and_flags, 0.3)
    _run(tc.test_training_head_single_node, (4, 48, 64, 1, 36, 132))
    _run(tc.test_training_head_single_node, (4, 64, 256, 2, 32, 64))


FAMILIES = {"batchnorm": family_batchnorm, "losses": family_losses, "targets": family_targets,
            "training_inputs": family_training_inputs, "decode": family_decode, "merge_nms": family_merge_nms,
            "rle_png": family_rle_png, "track": family_track, "pixel_counts": family_pixel_counts,
            "rasterisers": family_rasterisers, "dcn": family_dcn}

def _agree(family, seen):
    """The raw outputs a family handed back under the fills agree bit for bit."""
    fills = sorted(seen)
    for other in fills[1:]:
        a, b = seen[fills[0]], seen[other]
        assert (a is None) == (b is None)
        if a is None:
            continue
        assert sorted(a) == sorted(b)
        for k in a:
            assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), \
                "%s: %s under fill 0x%02X differs from fill 0x%02X" % (family, k, other, fills[0])


@pytest.mark.gpu
@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_family_in_dirty_guarded_memory(family, monkeypatch, tmp_path):
    """The family under each of the three fills, in one test so that their agreement is always checked.  A failed
    assertion under one fill does not keep the others from running: which fills fail is what tells a missing clear
    (0xA5 or 0xFF only) from a wrong size or a wrong value (all three)."""
    tools = types.SimpleNamespace(monkeypatch=monkeypatch, tmp_path=tmp_path)
    seen, failed = {}, []
    for fill in mg.FILLS:
        try:
            mg.dirty_allocator(fill)
            with mg.guarded_workspaces(fill) as guard:
                seen[fill] = FAMILIES[family](fill, tools)
            assert guard.requests >= 1, "the family asked for no workspace"
        except AssertionError as e:
            failed.append("under fill 0x%02X: %s" % (fill, str(e)[:2000]))
        finally:
            monkeypatch.undo()
            mg.clean_allocator()
    assert not failed, "%s: %d of %d fills failed\n%s" % (family, len(failed), len(mg.FILLS), "\n".join(failed))
    assert sorted(seen) == sorted(mg.FILLS)
    _agree(family, seen)


# ================================================================================================ repeated use ==
def _twice_decode():
    return [lambda: _decode(8, 64, 96, 100, 16), lambda: {"dets": _decode(3, 9, 11, 5, 4)}]


def _twice_panoptic():
    import test_panoptic as tq

    def big():
        ids, index = tq.random_image(1024, 255, 1)                          # the global-table regime: 1025 x 256 cells
        labels = 24 + np.arange(255) % 2
        tq.same(tq.run(index, 255, labels, ids), tq.want(index, 255, labels, ids))

    def small():
        rng = np.random.RandomState(4)
        ids = rng.choice(np.array([7, 26001, 24002, 3], np.uint16), (21, 35))
        index = rng.choice(np.array([0, 1, 255], np.uint8), ids.shape)
        got = tq.run(index, 2, [26, 24], ids)
        tq.same(got, tq.want(index, 2, [26, 24], ids))
        return dict(zip(("seg", "pairs", "stat", "iou", "bad", "match"), got))
    return [big, small]


def _twice_kinematics():
    import test_tracking_motion as tm
    T, CAR = tm.T, tm.CAR

    def case(n, seed):
        rng = np.random.RandomState(seed)
        H, W, t = 12, 21, 7
        index = rng.choice(np.concatenate([np.arange(n), [255]]).astype(np.uint8), (H, W))
        inst = [[k, 10 + k, 1, 2, int(k % 2)] for k in range(n)]
        slots, kin = np.zeros((T, 5), np.int64), np.zeros((T, 6), np.int64)
        for k in range(n):
            slots[k] = [10 + k, CAR, 0, t, 1]
            kin[k] = [16 * k + 3, 16 * 2 + 5, 1, -1, t - 1 - k % 3, 1]
        kin[n + 3] = [1, 2, 3, 4, 5, 1]                                     # a free slot with stale numbers
        want = tm.host.kinematics(index, n, inst, slots, t, kin)
        got = tm._kinematics(tm._dev(index), n, inst, slots, 0, t, kin)
        assert np.array_equal(got, want), n
        return {"kin": got}
    return [lambda: case(128, 1), lambda: case(3, 2)]


REPEATS = {"decode": _twice_decode, "panoptic_pairs": _twice_panoptic, "track_kinematics": _twice_kinematics}


@pytest.mark.gpu
@pytest.mark.parametrize("fill", mg.FILLS, ids=FILL_IDS)
@pytest.mark.parametrize("entry", sorted(REPEATS))
def test_a_workspace_used_twice(entry, fill):
    """Shape A, then a smaller shape B through the same payload as A left it (how the allocator hands a block back): B
    equals B run alone, and both equal their references."""
    first, second = REPEATS[entry]()
    try:
        mg.dirty_allocator(fill)
        with mg.guarded_workspaces(fill) as guard:
            alone = second()
        with mg.guarded_workspaces(fill, reuse=True) as guard:
            first()
            after = second()
            assert len(guard.arenas) == 1 and guard.requests >= 2          # B ran in A's payload
    finally:
        mg.clean_allocator()
    assert sorted(alone) == sorted(after)
    for k in alone:
        assert np.asarray(alone[k]).tobytes() == np.asarray(after[k]).tobytes(), k


# ================================================================================================ the harness ==
@pytest.mark.gpu
def test_the_guard_reports_a_write_outside_the_payload():
    """The harness itself: a byte written just past a payload, and one just before it, are found and located.  (Both
    land in the arena's own bands: nothing outside the test's allocation is touched.)"""
    import torch
    for where, offset, text in ((100, 100, "byte 100 of the payload's range (0 past its end)"), (-1, -1, "byte -1 (before")):
        with pytest.raises(AssertionError, match="request 1 of 100 bytes") as e:
            with mg.guarded_workspaces(0xA5) as guard:
                _C.workspace(40, "cuda")
                ws = _C.workspace(100, torch.device("cuda"))
                assert ws.numel() == 100 and ws.data_ptr() % 256 == 0 and bool((ws == 0xA5).all())
                arena, front, n = guard.arenas[1]
                arena[front + where] = 0
        assert text in str(e.value)
    # a body that fails on a value is still told about the damage
    with pytest.raises(AssertionError, match="(?s)wrong value.*guard bytes damaged: request 0 of 64 bytes: byte 64 "):
        with mg.guarded_workspaces(0x00) as guard:
            ws = _C.workspace(64, "cuda")
            arena, front, n = guard.arenas[0]
            arena[front + 64] = 1
            assert False, "wrong value"
    with pytest.raises(AssertionError, match="^wrong value"):
        with mg.guarded_workspaces(0x00):
            assert False, "wrong value"
    # reuse hands the first payload out again only once the earlier view is gone: two live workspaces never alias
    with mg.guarded_workspaces(0xA5, reuse=True) as guard:
        a = _C.workspace(512, "cuda")
        b = _C.workspace(64, "cuda")
        assert a.data_ptr() != b.data_ptr() and len(guard.arenas) == 2
        a[:64] = 7
        del a, b
        c = _C.workspace(64, "cuda")
        assert len(guard.arenas) == 2 and bool((c == 7).all())              # as the first call left it
    assert _C.workspace.__module__ == _C.__name__                           # restored
    with mg.guarded_workspaces(0xFF) as guard:
        assert _C.workspace(0, "cuda").numel() == 16 and guard.requests == 1

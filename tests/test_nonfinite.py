"""NaN and Inf through the library: every fused ReLU and the focal clamp carry a NaN as torch does, nothing leaks.

Each kernel runs on an input from the usual synth streams with NaN, +Inf and -Inf planted at fixed positions of image 0
(tests/nonfinite_ref.py), next to the same operation in plain CPU torch: float32 on the planted input for WHERE the
output is non-finite, float64 on the unplanted input for the finite values.

    no scrubbing   every element the float32 reference makes non-finite is non-finite on the device -- and of the same
                   class (NaN, +Inf, -Inf) for the exact-float32 kernels; the split-bf16 kernels split an Inf into an
                   Inf and a NaN part, so there "non-finite" is the requirement;
    no leak        every element whose receptive field holds no planted value is finite and within the tolerance the
                   kernel's existing test uses (no new tolerance anywhere in this file).

The CPU-only tests at the top check that the comparison means something: each reference leaves more than half of its
output finite, and the whole-network oracle leaves image 1 wholly finite."""
import ctypes
import types

import numpy as np
import pytest
import torch

import nonfinite_ref as N
import train_grad_ref as R
from centerpoly_amd import _C, synth
from oracle import losses as olos

T = torch.from_numpy
DEV = "cuda"
TOL = 2e-5                                             # test_conv_mfma.TOL: one split-bf16 contraction, of the max-norm
gpu = pytest.mark.gpu


def P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def g(a):
    return None if a is None else (T(a) if isinstance(a, np.ndarray) else a).to(DEV)


def _ids(names):
    return dict(argvalues=names, ids=[n.replace(" ", "_") for n in names])


def _named(prefix):
    return _ids([n for n in N.CASES if n.startswith(prefix)])


# =================================================================================== CPU: the references themselves ==
@pytest.mark.parametrize("name", **_ids(list(N.CASES)))
def test_reference_leaves_more_than_half_finite(name):
    c = N.get(name)
    bad = ~torch.isfinite(c.ref32)
    if name == "focal inf":                            # the one case whose point is a finite result: sigmoid saturates
        assert not bad.any() and torch.isfinite(c.loss32)
        return
    assert bad.any(), "nothing non-finite in the reference: the case checks nothing"
    assert not (bad & ~c.taint).any(), "a non-finite reference element outside the receptive fields of the planted values"
    frac = N.finite_fraction(c.ref32)
    print("%s: %.3f of the reference finite, %d non-finite elements" % (name, frac, int(bad.sum())))
    if name in N.SMALL_RECEPTIVE_EXCEPTIONS:           # see nonfinite_ref.py: geometry leaves one clean column of four
        assert frac >= N.SMALL_RECEPTIVE_EXCEPTIONS[name] and not c.taint[..., 0].any()
        return
    assert frac > 0.5
    assert (~c.taint).float().mean() > 0.5
    if hasattr(c, "reach"):                            # the set the DCN device comparison leaves out
        assert not (c.taint & ~c.reach).any()
        print("%s: %.3f outside `reach`" % (name, float((~c.reach).float().mean())))
        assert (~c.reach).float().mean() > 0.5
    if c.ref64 is not None:                            # outside the receptive fields both references are the same function
        clean = ~c.taint
        np.testing.assert_allclose(c.ref32[clean].numpy(), c.ref64[clean].float().numpy(), rtol=1e-3, atol=1e-4)


def test_relu_and_clamp_references_keep_a_nan():
    """What the kernels are held to: torch.relu and torch.clamp return NaN for NaN; -0 and denormals pass through
    max(v, 0) with their bits (the finite path of cp_relu is that same single maximum)."""
    v = torch.tensor([N.NAN, -N.INF, N.INF, -0.0, 1e-42, -1e-42])
    r = torch.relu(v)
    assert torch.isnan(r[0]) and r[1] == 0 and r[2] == N.INF and r[4] == v[4] and r[5] == 0
    assert torch.isnan(torch.clamp(torch.sigmoid(v[:1]), 1e-4, 1 - 1e-4)).all()


@pytest.mark.parametrize("name", list(N.NET_CASES))
def test_network_oracle_keeps_image_1_finite(name):
    c = N.net_case(name)
    for h in c.eval32:
        assert not torch.isfinite(c.eval32[h][0]).all(), h             # the NaN pixel reaches every head of image 0
        assert torch.isfinite(c.eval32[h][1]).all(), h                 # and eval mode keeps it out of image 1
        assert not torch.isfinite(c.train32[h]).any(), h               # batch statistics: everything, everywhere


# ============================================================================================== device-side checks ==
def _same(a, b):
    """torch.equal that takes a NaN for a NaN."""
    return a.shape == b.shape and bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all())


def _check(out, c, exact, close, allowed=None):
    """`exact`: True -- NaN for NaN and the same infinity for an infinity; "inf or nan" -- an infinity may also have become
    a NaN; False -- non-finite for non-finite (the split-bf16 kernels).
    `close(out_clean, ref64_clean, ref64)`: the existing test's tolerance on the untouched elements.
    `allowed`: where the device may be non-finite (default: the receptive fields, c.taint)."""
    out = out.detach().cpu()
    bad = ~torch.isfinite(c.ref32)
    dev_bad = ~torch.isfinite(out)
    scrubbed = bad & ~dev_bad
    assert not scrubbed.any(), "%d of %d non-finite reference elements are finite on the device, e.g. at %s: %s" % (
        int(scrubbed.sum()), int(bad.sum()), scrubbed.nonzero()[0].tolist(), out[scrubbed][:4].tolist())
    if exact:
        nan, inf = torch.isnan(c.ref32), torch.isinf(c.ref32)
        assert torch.isnan(out[nan]).all(), "%d NaN of the reference are Inf on the device" % int((~torch.isnan(out[nan])).sum())
        same = out[inf] == c.ref32[inf]
        if exact == "inf or nan":                      # (a kernel that multiplies a neighbouring value by a weight of 0)
            same = same | torch.isnan(out[inf])
        assert same.all(), "%d of %d infinities of the reference are %s on the device" % (
            int((~same).sum()), int(inf.sum()), out[inf][~same][:4].tolist())
    allowed = c.taint if allowed is None else allowed
    leaked = dev_bad & ~allowed
    assert not leaked.any(), "%d non-finite device elements outside the receptive fields, e.g. at %s" % (
        int(leaked.sum()), leaked.nonzero()[0].tolist())
    clean = ~allowed
    assert clean.any()
    if c.ref64 is not None:
        close(out[clean], c.ref64[clean], c.ref64)


def _max_norm(tol):
    def close(a, r, full):
        err = (a.double() - r).abs().max().item() / max(full[torch.isfinite(full)].abs().max().item(), 1e-30)
        assert err <= tol, err
    return close


def _allclose(rtol, atol=0.0, atol_of_max=0.0):
    def close(a, r, full):
        np.testing.assert_allclose(a.double().numpy(), r.numpy(), rtol=rtol, atol=atol + atol_of_max * full.abs().max().item())
    return close


# ---- training BatchNorm ----------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name", **_named("bn "))
def test_bn_act_poisons_its_channel_only(name):
    """One bad channel of one image: that channel is NaN in every image, as in torch (the statistics are NaN); its
    running statistics and saved mean / invstd are non-finite; every other channel keeps test_fused_bn_act_vs_torch's
    tolerances."""
    from centerpoly_amd.models.networks.pose_dla_dcn import bn_act, flush_batch_counts
    c = N.get(name)
    C = c.x.shape[1]
    bn = torch.nn.BatchNorm2d(C, momentum=0.1).to(DEV).train()
    with torch.no_grad():
        bn.weight.copy_(g(c.p["w"])), bn.bias.copy_(g(c.p["b"]))
        bn.running_mean.copy_(g(c.p["rm"])), bn.running_var.copy_(g(c.p["rv"]))
    y = bn_act(bn, g(c.x).requires_grad_(True), relu=c.relu, residual=g(c.res))
    flush_batch_counts()
    assert "BnAct" in type(y.grad_fn).__name__                          # the fused kernel ran
    assert torch.isnan(c.ref32[:, N.BN_CHANNEL]).all()
    _check(y, c, True, _allclose(1e-4, 1e-5))
    mean, invstd = y.grad_fn.saved_tensors[4:6]
    other = torch.arange(C) != N.BN_CHANNEL
    for dev, r32, r64 in zip((bn.running_mean, bn.running_var, mean, invstd), c.stats32, c.stats64):
        dev = dev.detach().cpu()
        assert not torch.isfinite(r32[N.BN_CHANNEL]) and not torch.isfinite(dev[N.BN_CHANNEL])
        np.testing.assert_allclose(dev[other].numpy(), r64[other].numpy(), rtol=1e-5, atol=1e-6)


# ---- cp_bias_act_inplace ---------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name", **_named("bias_act "))
def test_bias_act_inplace(name):
    c = N.get(name)
    y, bias, res = g(c.y), g(c.bias), g(c.res)
    B, C, H, W = y.shape
    _C.check(_C.lib().cp_bias_act_inplace(P(y), P(bias), P(res), B, C, H * W, 1 if c.relu else 0, _C.stream()),
             "cp_bias_act_inplace")
    _check(y, c, True, _allclose(1e-4, 1e-5))                          # test_folded_conv_epilogue_matches_bn_relu's


@gpu
def test_relu_keeps_the_bits_of_every_other_value():
    """cp_relu through cp_bias_act_inplace (no bias, no residual: v + 0, then the ReLU) over a sweep of float32 bit
    patterns -- every 4093rd of all 2^32, and the edges: zeros, the smallest and largest denormals and normals, the
    infinities, quiet and signalling NaNs of both signs.  Bit for bit max(v + 0, 0) for everything that is not a NaN
    (-0 and negative denormals give +0, positive denormals themselves); a NaN for a NaN."""
    n = 1 << 20
    edges = [0, 0x80000000, 1, 0x80000001, 0x007fffff, 0x807fffff, 0x00800000, 0x80800000, 0x7f7fffff, 0xff7fffff,
             0x7f800000, 0xff800000, 0x7fc00000, 0xffc00000, 0x7f800001, 0xff800001]
    bits = torch.cat([torch.tensor(edges, dtype=torch.int64), torch.arange(n, dtype=torch.int64) * 4093 % (1 << 32)])[:n]
    x = (bits - ((bits >> 31) << 32)).to(torch.int32).view(torch.float32).reshape(1, 64, n // 64)
    nan = torch.isnan(x)
    den = (x.abs() < torch.finfo(torch.float32).tiny) & (x != 0)
    assert int(nan.sum()) > 1000 and int(den.sum()) > 1000
    y = g(x)
    _C.check(_C.lib().cp_bias_act_inplace(P(y), None, None, 1, 64, n // 64, 1, _C.stream()), "cp_bias_act_inplace")
    y = y.cpu()
    want = torch.where(x > 0, x, torch.zeros(()))                       # +0 for -0, negatives and negative denormals
    assert torch.equal(y.view(torch.int32)[~nan], want.view(torch.int32)[~nan])
    assert torch.isnan(y[nan]).all()


# ---- direct convolution ----------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name", **_named("direct "))
def test_direct_conv(name):
    c = N.get(name)
    cin, cout, k, stride, pad = c.cfg
    x, w, b = g(c.x), g(c.w), g(c.b)
    B, _, H, W = x.shape
    L = _C.lib()
    out = torch.zeros(tuple(c.ref32.shape), device=DEV)
    _C.check(L.cp_conv_direct_forward(P(x), P(w), P(b), P(out), B, cin, H, W, cout, k, stride, pad, 1, _C.stream()), "direct")
    _check(out, c, True, _allclose(1e-4, atol_of_max=1e-5))
    if k == 3:                                                          # the split-bf16 arithmetic of the same call
        o2 = torch.zeros_like(out)
        _C.check(L.cp_conv_direct_forward_ex(P(x), P(w), P(b), P(o2), B, cin, H, W, cout, k, stride, pad, 1, 1, _C.stream()),
                 "direct_ex")
        _check(o2, c, False, _max_norm(TOL))


# ---- the DLA base ----------------------------------------------------------------------------------------------------
def _base_device(kind, c):
    L = _C.lib()
    p = {k: g(v) for k, v in c.p.items()}
    x = g(c.x)
    B, _, H, W = x.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    wp = torch.empty(L.cp_conv7x7_c3_weight_bytes(16), dtype=torch.uint8, device=DEV)
    _C.check(L.cp_conv7x7_c3_prepare(P(p["ws"]), 16, P(wp), _C.stream()), "prepare")
    if kind == "stem":
        out = torch.zeros((B, 16, H, W), device=DEV)
        _C.check(L.cp_conv7x7_c3_forward(P(x), P(wp), P(p["bs"]), P(out), B, H, W, 16, 1, 1, _C.stream()), "stem")
    elif kind == "pair":
        out = torch.zeros((B, 32, Ho, Wo), device=DEV)
        _C.check(L.cp_dla_base_pair_forward(P(x), P(p["w0"]), P(p["b0"]), P(p["w1"]), P(p["b1"]), P(out), B, H, W,
                                            _C.stream()), "pair")
    else:
        assert L.cp_dla_base_trio_supported(H, W)
        out = torch.zeros((B, 32, Ho, Wo), device=DEV)
        _C.check(L.cp_dla_base_trio_forward(P(x), P(wp), P(p["bs"]), P(p["w0"]), P(p["b0"]), P(p["w1"]), P(p["b1"]), P(out),
                                            B, H, W, _C.stream()), "trio")
    return out


@gpu
@pytest.mark.parametrize("name", **_named("base "))
def test_dla_base_kernels_keep_a_nan_through_their_inner_relus(name):
    """The 7x7 stem, the fused level0 + level1 pair and the fused trio: between the fused layers sit ReLUs that no
    tensor in memory ever shows.  One TOL per chained split-bf16 contraction, as test_base_trio.py allows."""
    c = N.get(name)
    kind = name.split()[1]
    out = _base_device(kind, c)
    _check(out, c, False, _max_norm({"stem": 1, "pair": 2, "trio": 3}[kind] * TOL))


@gpu
def test_base_trio_still_has_the_bits_of_stem_then_pair_on_non_finite_input():
    c = N.get("base trio 2x37x100")
    trio = _base_device("trio", c)
    s = _base_device("stem", c)
    pair = _base_device("pair", types.SimpleNamespace(x=s, p=c.p))
    assert _same(trio, pair)


# ---- split-bf16 convolutions -----------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name", **_named("conv_mfma "))
def test_conv_mfma_epilogue(name):
    from test_conv_mfma import _conv
    c = N.get(name)
    out = _conv(g(c.x), g(c.w), bias=g(c.bias), residual=g(c.res), relu=True)
    _check(out, c, False, _max_norm(TOL))


@gpu
def test_stream_1x1_every_form():
    import test_conv_stream as S
    c = N.get("stream1x1 2x32x64x5x37")
    x, w, bias, res = g(c.x), g(c.w), g(c.bias), g(c.res)
    for form in [(0, 0)] + S.FORMS:
        _check(S._stream([x], w, bias, res, True, form), c, False, _max_norm(TOL))


@gpu
def test_stream_3x3():
    """The 3x3 stream kernel applies no ReLU (it refuses one): plain propagation, and the staged kernel's bits."""
    import test_conv3x3_stream as S
    c = N.get("stream3x3 2x32x27x5x37")
    x, w, bias = g(c.x), g(c.w), g(c.bias)
    out = S._stream(x, w, bias)
    _check(out, c, False, _max_norm(TOL))
    assert _same(out, S._staged(x, w, bias))


# ---- heads -----------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name", **_named("head stage "))
def test_head_output_stage_relu_in(name):
    c = N.get(name)
    cin, cout, H, W = c.cfg
    ytot, b3, w1, b1 = g(c.ytot), g(c.b3), g(c.w1), g(c.b1)
    c0 = N.HEAD_C0
    out = torch.zeros(2, cout, H, W, device=DEV)
    _C.check(_C.lib().cp_conv1x1_act_forward(
        _C.c_void_p(ytot.data_ptr() + 4 * c0 * H * W), (cin + 7) * H * W, _C.c_void_p(b3.data_ptr() + 4 * c0), 1,
        _C.ptr(w1.t().contiguous()), _C.ptr(b1), _C.ptr(out), 2, cin, cout, H * W, _C.stream()), "head")
    _check(out, c, True, _allclose(1e-5, 1e-5))


@gpu
@pytest.mark.parametrize("name", **_named("fused heads "))
def test_fused_heads_do_not_turn_a_nan_feature_into_head_maps(name):
    from test_wide_polygons import _fused_heads, _prepare_w2
    c = N.get(name)
    couts, hc, cin, H, W = c.cfg
    L = _C.lib()
    nh = len(couts)
    x, w1, b1 = g(c.x), g(c.w1), g(c.b1)
    w2, b2 = [g(w) for w in c.w2], [g(b) for b in c.b2]
    wp1 = torch.empty(L.cp_conv_mfma_weight_bytes(cin, nh * hc, 9), dtype=torch.uint8, device=DEV)
    _C.check(L.cp_conv_mfma_prepare(P(w1), cin, nh * hc, 9, 0, P(wp1), _C.stream()), "prepare")
    w2p = [_prepare_w2(L, w, co, hc) for w, co in zip(w2, couts)]
    rc, outs = _fused_heads(L, x, wp1, b1, w2p, b2, couts, hc)
    assert rc == 0
    _check(torch.cat(outs, 1), c, False, _max_norm(TOL))


# ---- DCN -------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("contraction", ["f32", "bf16x3", "bf16x3_region"])
@pytest.mark.parametrize("name", **_ids([n for n in N.CASES if n.startswith(("dcn 2x", "dcn origin"))]))
def test_dcn_forward_epilogue(name, contraction):
    """relu(dcn(x) * scale + shift) in the kernel's epilogue, x non-finite.  The device may add the outputs that sample
    a NEIGHBOUR of a planted pixel: the gather kernels load the two columns of a row as one pair and give the column
    that lies outside the sample's cell a weight of 0, and 0 * NaN is NaN.  And a tap outside the image loads pixels
    (0, 0) and (0, 1) of its image with a weight of 0: in the "origin" cases, planted there, every output of image 0 with
    such a tap may be non-finite too.  c.reach is the union (nonfinite_ref._dcn_case); nothing outside it may be.  For the same reason an Inf of the
    exact-float32 kernel may come out as a NaN (0 * Inf beside it), never as a finite value or the other infinity."""
    from centerpoly_amd.models.networks.DCNv2.dcn_v2 import _shape, dcn_v2_forward_raw
    c = N.get(name)
    x, om, w = g(c.x), g(c.om), g(c.w)
    kernel = _C.lib().cp_dcn_v2_forward_kernel(_shape(x, w, 1, 1, 1, 1), _C.DCN_CONTRACTION[contraction])
    if contraction == "bf16x3_region":
        if x.shape[1] % 16:
            assert kernel != 2
            return                                                      # the gather kernel again: covered by "bf16x3"
        assert kernel == 2
    out = dcn_v2_forward_raw(x, om, w, None, ep_scale=g(c.sc), ep_shift=g(c.sh), relu=True, contraction=contraction)
    if contraction == "f32":
        close = _allclose(1e-3, atol_of_max=2e-5)                       # test_dcn_forward_vs_oracle
    else:
        close = _allclose(1e-3, atol_of_max=1e-4)                       # test_dcn_forward_split_bf16_contraction / region
    _check(out, c, "inf or nan" if contraction == "f32" else False, close, allowed=c.reach)


@gpu
def test_dcn_splitk_reduce_relu():
    c = N.get("dcn splitk reduce 13x2x5x3x5")
    n, B, C, H, W = N.REDUCE
    part, sc, sh = g(c.part), g(c.sc), g(c.sh)
    out = torch.zeros((B, C, H, W), device=DEV)
    _C.check(_C.lib().cp_dcn_splitk_reduce(P(part), n, P(sc), P(sh), 1, P(out), B, C, H * W, _C.stream()), "reduce")
    _check(out, c, True, _allclose(1e-5, 1e-6))


# ---- max pooling -----------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name", **_named("maxpool "))
def test_maxpool_a_nan_wins_and_takes_the_gradient(name):
    from centerpoly_amd.models.networks.pose_dla_dcn import downsample2
    c = N.get(name)
    x = g(c.x).requires_grad_(True)
    y = downsample2(torch.nn.MaxPool2d(2, stride=2), x)
    assert "MaxPool2x2Fn" in type(y.grad_fn).__name__
    assert torch.isnan(c.ref32).sum() >= 4
    assert _same(y.detach().cpu(), c.ref32)
    (gx,) = torch.autograd.grad(y, x, g(c.go))
    assert torch.equal(gx.cpu(), c.grad)                               # go, or 0: at the position torch picks


# ---- up-sampling -----------------------------------------------------------------------------------------------------
@gpu
def test_upsample2x_add_propagates():
    from centerpoly_amd.models.networks.large_hourglass import MergeUp
    c = N.get("upsample2x_add 1x3x7x9")
    out = MergeUp().fused(g(c.up1), g(c.low))
    assert out is not None
    assert _same(out.cpu(), c.ref32)                                   # test_upsample2x_add_vs_torch: torch.equal
    _check(out, c, True, None)


@gpu
@pytest.mark.parametrize("name", **_named("depthwise up "))
def test_depthwise_up_add_propagates(name):
    from centerpoly_amd.models.networks.pose_dla_dcn import depthwise_up_add
    c = N.get(name)
    f, C = c.f, c.x.shape[1]
    up = torch.nn.ConvTranspose2d(C, C, f * 2, stride=f, padding=f // 2, groups=C, bias=False).to(DEV)
    with torch.no_grad():
        up.weight.copy_(g(c.w))
        out = depthwise_up_add(g(c.x), up, g(c.skip))
    _check(out, c, True, _allclose(1e-5, 1e-6))


# ---- focal loss ------------------------------------------------------------------------------------------------------
@gpu
def test_focal_nan_logit_gives_nan_loss_and_nan_only_there():
    from centerpoly_amd.models.losses import sigmoid_focal_loss
    c = N.get("focal nan")
    assert torch.isnan(c.loss32) and int(torch.isnan(c.ref32).sum()) == len(N.FOCAL_NAN_AT)
    loss, act = sigmoid_focal_loss(g(c.x), g(c.gt))
    _, today = sigmoid_focal_loss(g(c.clean), g(c.gt))                  # the same kernel on the unplanted logits
    assert torch.isnan(loss), float(loss)
    act, today = act.cpu(), today.cpu()
    assert torch.equal(torch.isnan(act), c.taint)
    assert torch.equal(act[~c.taint], today[~c.taint])                 # bit-equal elsewhere
    np.testing.assert_allclose(today.numpy(), olos.sigmoid_clamp(T(c.clean).double()).numpy(), rtol=1e-5, atol=1e-7)


@gpu
def test_focal_infinite_logits_stay_finite_and_equal_the_oracle():
    from centerpoly_amd.models.losses import sigmoid_focal_loss
    c = N.get("focal inf")
    assert torch.isfinite(c.loss32) and torch.isfinite(c.ref32).all()
    loss, act = sigmoid_focal_loss(g(c.x), g(c.gt))
    assert torch.isfinite(loss) and torch.isfinite(act).all()
    np.testing.assert_allclose(loss.item(), c.loss64.item(), rtol=1e-5)     # test_sigmoid_focal_vs_oracle_and_golden's
    np.testing.assert_allclose(act.cpu().numpy(), c.ref64.numpy(), rtol=1e-5, atol=1e-7)
    lo, hi = float(np.float32(1e-4)), float(np.float32(1 - 1e-4))
    for i, v in N.FOCAL_INF_AT:
        assert act.reshape(-1)[i].item() == (hi if v > 0 else lo)


# =================================================================================================== whole network ==
NET_TOL = {"dla_eighths": (1e-3, 1e-4), "hourglass": (2e-3, 2e-4)}      # test_*_forward_vs_reference_golden: rtol, atol / max
SETTINGS = [("dla_eighths", s) for s in (False, "f32", "bf16x3", "auto", "bf16x3_region")] + \
           [("hourglass", False), ("hourglass", "auto")]
_MODELS = {}


def _model(name, train=False):
    from centerpoly_amd.models.model import create_model
    c = N.net_case(name)
    m = create_model(c.arch, dict(R.HEADS), c.head_conv)
    m.load_state_dict(c.state_dict())
    return m.to(DEV).train(train)


def _eval_heads(name, setting):
    if (name, setting) not in _MODELS:
        c = N.net_case(name)
        m = _model(name)
        if setting:
            m.prepare_inference(**({"dcn_contraction": setting} if c.arch == "dla_34" else {}))
        with torch.no_grad():
            _MODELS[(name, setting)] = {k: v.clone().cpu() for k, v in m(g(c.xp))[-1].items()}
        del m
    return _MODELS[(name, setting)]


@gpu
@pytest.mark.parametrize("name,setting", SETTINGS, ids=["%s-%s" % (n, s or "plain") for n, s in SETTINGS])
def test_network_eval_carries_the_nan_and_keeps_image_1(name, setting):
    c = N.net_case(name)
    out = _eval_heads(name, setting)
    rtol, atol = NET_TOL[name]
    for h, ref in c.eval32.items():
        bad = ~torch.isfinite(ref)
        scrubbed = bad & torch.isfinite(out[h])
        assert not scrubbed.any(), "%s: %d of %d non-finite oracle elements are finite on the device" % (
            h, int(scrubbed.sum()), int(bad.sum()))
        assert torch.isfinite(out[h][1]).all(), h
        r1 = ref[1].numpy()
        np.testing.assert_allclose(out[h][1].numpy(), r1, rtol=rtol, atol=atol * np.abs(r1).max(), err_msg=h)


@gpu
def test_decode_is_not_reached_with_plausible_scores():
    """After the fused heads (prepare_inference, what the detector runs) the heat map of the image with the NaN pixel is
    non-finite: nothing hands decode an ordinary-looking map made from garbage."""
    hm = _eval_heads("dla_eighths", "auto")["hm"]
    assert not torch.isfinite(hm[0]).all()
    assert not torch.isfinite(torch.sigmoid(hm[0])).all()


@gpu
@pytest.mark.parametrize("name", list(N.NET_CASES))
def test_network_train_mode_and_loss_are_nan(name):
    from centerpoly_amd.opts import opts
    from centerpoly_amd.trains.polydet import PolydetLoss
    c = N.net_case(name)
    B, _, H, W = c.x.shape
    m = _model(name, train=True)
    with torch.no_grad():
        out = m(g(c.xp))[-1]
    for h in c.train32:
        assert not torch.isfinite(out[h]).any(), "%s: %d finite elements" % (h, int(torch.isfinite(out[h]).sum()))
    opt = opts().init(["polydet", "--arch", c.arch, "--nbr_points", "16", "--poly_loss", "l1"])
    opt.device = torch.device(DEV)
    nb = synth.train_batch(B, H // 4, W // 4, nbr_points=16, mean_objs=5, with_input=False, stream="nonfinite/" + name)
    assert int(nb["reg_mask"][0].sum()) > 0 and int(nb["reg_mask"][1].sum()) > 0
    loss, stats = PolydetLoss(opt)([{k: v.clone() for k, v in out.items()}], {k: g(v) for k, v in nb.items()})
    assert torch.isnan(loss) and torch.isnan(stats["hm_l"]), (float(loss), float(stats["hm_l"]))

"""GPU parity of the split-bf16 MFMA 3x3 convolution (csrc/conv_mfma.hip) through the C ABI.

float64 torch convolution is the checker (a floating-point kernel: plain torch reference, per the task's rule
for such kernels).  Tolerance: every product is formed from bf16 halves hi*hi + hi*lo + lo*hi, i.e. with a
relative error <= ~2^-16 before the float32 accumulation; measured 4e-6 of the output's max-norm on the layer
shapes of DLA-34, asserted at 2e-5 -- fifty times inside the path's 1e-3 bar."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from centerpoly_amd import _C, synth

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 2e-5


def P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _t(tag, shape, scale=1.0):
    return torch.from_numpy(synth.normal("convmfma/" + tag, shape) * np.float32(scale)).to(DEV)


def _conv(x, w, bias=None, residual=None, relu=False, transposed=False):
    L = _C.lib()
    B, cin, H, W = x.shape
    cout = w.shape[1] if transposed else w.shape[0]
    assert L.cp_conv3x3_mfma_supported(cin, cout, H, W)
    wp = torch.empty(L.cp_conv3x3_mfma_weight_bytes(cin, cout), dtype=torch.uint8, device=DEV)
    _C.check(L.cp_conv3x3_mfma_prepare(P(w), cin, cout, 1 if transposed else 0, P(wp), _C.stream()), "prepare")
    out = torch.full((B, cout, H, W), float("nan"), device=DEV)
    _C.check(L.cp_conv3x3_mfma_forward(P(x), P(wp), P(bias), P(residual), P(out), B, cin, H, W, cout,
                                       1 if relu else 0, _C.stream()), "forward")
    return out


def _rel(a, ref):
    return (a.double() - ref).abs().max().item() / max(ref.abs().max().item(), 1e-30)


# (B, Cin, Cout, H, W): the layer families of DLA-34 / Hourglass plus ragged edges -- map sizes that are not a
# multiple of the 8 x 32 (16 x 32) tile, output channels that do not fill a 16-row fragment (27, 80), input
# channels that do not fill the 32-channel step (27, 48), a single tile, one row, one column
SHAPES = [(2, 64, 64, 32, 64), (1, 64, 256, 40, 72), (2, 64, 27, 24, 80), (1, 128, 128, 17, 33),
          (3, 32, 80, 9, 31), (1, 256, 96, 8, 32), (2, 27, 64, 12, 40), (1, 48, 16, 5, 7), (1, 32, 32, 1, 50),
          (1, 32, 48, 37, 1), (1, 512, 64, 6, 10)]


@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_forward_matches_float64_convolution(shape):
    B, ci, co, H, W = shape
    x, w = _t("x%s" % (shape,), (B, ci, H, W)), _t("w%s" % (shape,), (co, ci, 3, 3), 0.05)
    ref = F.conv2d(x.double(), w.double(), padding=1)
    out = _conv(x, w)
    assert torch.isfinite(out).all()                      # every output element was written
    assert _rel(out, ref) <= TOL


@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[2], SHAPES[4]], ids=["64", "27", "80"])
def test_epilogue_bias_residual_relu(shape):
    B, ci, co, H, W = shape
    x, w = _t("ex", (B, ci, H, W)), _t("ew", (co, ci, 3, 3), 0.05)
    bias, res = _t("eb", (co,)), _t("er", (B, co, H, W))
    lin = F.conv2d(x.double(), w.double(), bias.double(), padding=1)
    assert _rel(_conv(x, w, bias=bias), lin) <= TOL
    assert _rel(_conv(x, w, bias=bias, relu=True), F.relu(lin)) <= TOL
    full = F.relu(lin + res.double())
    out = _conv(x, w, bias=bias, residual=res, relu=True)
    assert _rel(out, full) <= TOL
    assert (out >= 0).all()


@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[1], SHAPES[2], SHAPES[4], SHAPES[6]],
                         ids=["64->64", "64->256", "64->27", "32->80", "27->64"])
def test_input_gradient_through_transposed_weights(shape):
    """grad_in = conv(grad_out, W transposed and flipped): the prologue's `transposed` mode, ragged K = Cout."""
    B, ci, co, H, W = shape
    w, go = _t("gw", (co, ci, 3, 3), 0.05), _t("ggo", (B, co, H, W))
    ref = torch.nn.grad.conv2d_input((B, ci, H, W), w.double(), go.double(), padding=1)
    assert _rel(_conv(go, w, transposed=True), ref) <= TOL


def test_linearity_and_determinism():
    x1, x2, w = _t("l1", (2, 64, 24, 64)), _t("l2", (2, 64, 24, 64)), _t("lw", (64, 64, 3, 3), 0.05)
    a, b, c = _conv(x1, w), _conv(x2, w), _conv(x1 + x2, w)
    assert (a + b - c).abs().max().item() <= TOL * c.abs().max().item()
    assert torch.equal(_conv(x1, w), a)                   # no atomics, fixed order: bit-identical reruns
    assert torch.equal(_conv(2.0 * x1, w), 2.0 * a)       # power-of-two scaling commutes with the bf16 split


def test_zero_padding_and_impulse():
    """An impulse input returns the flipped kernel around it; borders see zeros, not neighbours' rows."""
    w = _t("iw", (32, 32, 3, 3))
    x = torch.zeros((1, 32, 8, 32), device=DEV)
    x[0, 5, 0, 0] = 1.0
    x[0, 7, 7, 31] = 1.0
    out = _conv(x, w)
    ref = F.conv2d(x.double(), w.double(), padding=1)
    assert _rel(out, ref) <= TOL
    assert (out[0, :, 3:5, 8:24] == 0).all()


def test_autograd_wrapper_against_library():
    from centerpoly_amd.models.networks import conv3x3
    conv = torch.nn.Conv2d(64, 96, 3, padding=1, bias=False).to(DEV)
    x = _t("ax", (4, 64, 48, 64)).requires_grad_(True)
    assert conv3x3.usable(conv, x)
    y = conv3x3.conv_raw(conv, x)
    go = _t("ago", tuple(y.shape))
    gx, gw = torch.autograd.grad(y, (x, conv.weight), go)
    xd = x.detach().double().requires_grad_(True)
    wd = conv.weight.detach().double().requires_grad_(True)
    yd = F.conv2d(xd, wd, padding=1)
    gxd, gwd = torch.autograd.grad(yd, (xd, wd), go.double())
    assert _rel(y, yd.detach()) <= TOL and _rel(gx, gxd) <= TOL and _rel(gw, gwd) <= 1e-4


def test_unsupported_and_bad_arguments():
    L = _C.lib()
    assert not L.cp_conv3x3_mfma_supported(64, 64, 40000, 40000)          # beyond 32-bit offsets
    assert L.cp_conv3x3_mfma_forward(None, None, None, None, None, 1, 64, 8, 8, 64, 0, _C.stream()) != 0


def _wgrad(x, go, cout):
    L = _C.lib()
    B, cin, H, W = x.shape
    assert L.cp_conv3x3_mfma_wgrad_supported(cin, cout, H, W)
    gw = torch.zeros((cout, cin, 3, 3), device=DEV)
    _C.check(L.cp_conv3x3_mfma_wgrad(P(x), P(go), P(gw), B, cin, H, W, cout, _C.stream()), "wgrad")
    return gw


# ragged everything: rows not a multiple of 4, widths not a multiple of 32, 27 / 80 / 200 channels, several
# pixel tiles per workgroup and fewer tiles than workgroups
WG_SHAPES = [(2, 64, 64, 32, 64), (1, 64, 256, 40, 72), (2, 64, 27, 24, 80), (1, 128, 128, 17, 36), (3, 32, 80, 9, 28),
             (2, 27, 64, 12, 40), (1, 200, 48, 5, 8), (1, 32, 32, 1, 52), (1, 32, 48, 37, 4), (1, 512, 64, 6, 12),
             (4, 64, 64, 128, 256)]


@pytest.mark.parametrize("shape", WG_SHAPES, ids=["x".join(map(str, s)) for s in WG_SHAPES])
def test_weight_gradient_matches_float64(shape):
    B, ci, co, H, W = shape
    x, go = _t("wx%s" % (shape,), (B, ci, H, W)), _t("wgo%s" % (shape,), (B, co, H, W))
    ref = torch.nn.grad.conv2d_weight(x.double(), (co, ci, 3, 3), go.double(), padding=1)
    gw = _wgrad(x, go, co)
    assert _rel(gw, ref) <= TOL
    # accumulation semantics: a second call adds onto the first
    L = _C.lib()
    _C.check(L.cp_conv3x3_mfma_wgrad(P(x), P(go), P(gw), B, ci, H, W, co, _C.stream()), "wgrad")
    assert _rel(gw, 2.0 * ref) <= TOL


def test_weight_gradient_adjoint_identity():
    """<conv(x, w), go> == <w, wgrad(x, go)> with the forward of the same library: an oracle-free check."""
    x, w, go = _t("jx", (2, 64, 40, 96)), _t("jw", (96, 64, 3, 3), 0.05), _t("jgo", (2, 96, 40, 96))
    lhs = (_conv(x, w).double() * go.double()).sum().item()
    rhs = (w.double() * _wgrad(x, go, 96).double()).sum().item()
    norm = (_conv(x, w).double().abs() * go.double().abs()).sum().item()
    assert abs(lhs - rhs) <= 1e-5 * norm


def test_wgrad_refuses_unaligned_width():
    L = _C.lib()
    assert not L.cp_conv3x3_mfma_wgrad_supported(64, 64, 8, 30)
    x, go, gw = _t("ux", (1, 64, 8, 30)), _t("ugo", (1, 64, 8, 30)), torch.zeros((64, 64, 3, 3), device=DEV)
    assert L.cp_conv3x3_mfma_wgrad(P(x), P(go), P(gw), 1, 64, 8, 30, 64, _C.stream()) == -2


def _conv_multi(xs, w, bias=None, residual=None, relu=False):
    L = _C.lib()
    B, _, H, W = xs[0].shape
    cs = [x.shape[1] for x in xs]
    cin, cout, taps = sum(cs), w.shape[0], w.shape[2] * w.shape[3]
    wp = torch.empty(L.cp_conv_mfma_weight_bytes(cin, cout, taps), dtype=torch.uint8, device=DEV)
    _C.check(L.cp_conv_mfma_prepare(P(w), cin, cout, taps, 0, P(wp), _C.stream()), "prepare")
    out = torch.full((B, cout, H, W), float("nan"), device=DEV)
    ptrs = (ctypes.c_void_p * len(xs))(*[x.data_ptr() for x in xs])
    chans = (ctypes.c_int32 * len(xs))(*cs)
    rc = L.cp_conv_mfma_forward(ptrs, chans, len(xs), P(wp), P(bias), P(residual), P(out), B, H, W, cout, taps,
                                1 if relu else 0, _C.stream())
    return rc, out


# (channels of the sources, Cout, k, H, W): the Root layers of DLA-34 (two to four inputs), a 1x1 projection,
# a 3x3 over two sources, ragged single-source 1x1
MULTI = [((64, 64), 64, 1, 40, 72), ((128, 128, 64), 128, 1, 17, 33), ((256, 256, 128, 64), 256, 1, 8, 32),
         ((64,), 128, 1, 24, 80), ((32, 64), 48, 3, 12, 40), ((200,), 27, 1, 9, 31)]


@pytest.mark.parametrize("case", MULTI, ids=[str(m[0]) + "->%d k%d" % (m[1], m[2]) for m in MULTI])
def test_concatenated_sources_and_1x1(case):
    cs, co, k, H, W = case
    xs = [_t("ms%d_%d" % (i, c), (2, c, H, W)) for i, c in enumerate(cs)]
    w = _t("msw%s" % (case,), (co, sum(cs), k, k), 0.05)
    bias, res = _t("msb", (co,)), _t("msr", (2, co, H, W))
    rc, out = _conv_multi(xs, w, bias, res, True)
    assert rc == 0
    ref = F.relu(F.conv2d(torch.cat(xs, 1).double(), w.double(), bias.double(), padding=k // 2) + res.double())
    assert torch.isfinite(out).all() and _rel(out, ref) <= TOL


def test_multi_source_needs_whole_k_steps():
    xs = [_t("bad0", (1, 48, 8, 32)), _t("bad1", (1, 64, 8, 32))]
    rc, _ = _conv_multi(xs, _t("badw", (32, 112, 1, 1)))
    assert rc == -2                                       # CP_EUNSUPPORTED: 48 is not a multiple of 32


def test_training_trajectory_matches_exact_arithmetic():
    """Eight Adam steps of DLA-34 + DCNv2 on synthetic data, twice in fresh processes: default arithmetic (split-bf16
    convolutions and DCN backward) against library convolutions + exact-f32 DCN backward.  Step 0 (same weights):
    every loss term agrees to 1e-4 relative.  Later steps are compared on the heat-map loss only: steps 1-2 (the
    first updates: a wrong gradient shows here) at 1 % (measured 0.02 % / 0.15 %), steps 3-7 at 8 % -- with
    random-init weights Adam amplifies last-bit differences of tiny gradients, and two runs of the SAME arithmetic
    already differ by 1.5-2.5 % there (float-atomic summation order in the weight gradients; the polygon terms swing
    by far more)."""
    import json, os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    runs = []
    for arithmetic in ("split_bf16", "exact_f32"):
        out = subprocess.run([sys.executable, os.path.join(root, "tools", "train_trajectory.py"), "8", arithmetic],
                             capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stderr[-2000:]
        runs.append(json.loads(out.stdout.strip().splitlines()[-1])["trajectory"])
    assert len(runs[0]) == len(runs[1]) == 8
    for k in runs[0][0]:
        a, b = runs[0][0][k], runs[1][0][k]
        assert abs(a - b) <= 1e-4 * max(abs(b), 1e-3), (k, a, b)
    for i, (a, b) in enumerate(zip(*runs)):
        assert abs(a["hm_l"] - b["hm_l"]) <= (1e-2 if i < 3 else 8e-2) * b["hm_l"], (i, a["hm_l"], b["hm_l"])
    assert runs[0][-1]["hm_l"] < 0.6 * runs[0][0]["hm_l"]    # and it does learn


# (Cin, Cout, k, stride, pad): stem, level0, level1 of the DLA base; map sizes off the 8 x 32 (4 x 32) tile grid
SMALL = [(3, 16, 7, 1, 3), (16, 16, 3, 1, 1), (16, 32, 3, 2, 1)]


@pytest.mark.parametrize("cfg", SMALL, ids=["stem7x7", "level0", "level1s2"])
@pytest.mark.parametrize("hw", [(40, 72), (17, 33), (64, 256)], ids=["40x72", "17x33", "64x256"])
def test_direct_weight_gradient_of_the_base_layers(cfg, hw):
    cin, cout, k, stride, pad = cfg
    H, W = hw
    L = _C.lib()
    assert L.cp_conv_direct_wgrad_supported(cin, cout, k, stride, pad)
    x = _t("dw/x%s%s" % (cfg, hw), (3, cin, H, W))
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    go = _t("dw/go%s%s" % (cfg, hw), (3, cout, Ho, Wo))
    gw = torch.zeros((cout, cin, k, k), device=DEV)
    _C.check(L.cp_conv_direct_wgrad(P(x), P(go), P(gw), 3, cin, H, W, cout, k, stride, pad, _C.stream()), "wgrad")
    ref = torch.nn.grad.conv2d_weight(x.double(), (cout, cin, k, k), go.double(), stride=stride, padding=pad)
    assert _rel(gw, ref) <= 2e-6                       # exact f32 products, f32 accumulation
    _C.check(L.cp_conv_direct_wgrad(P(x), P(go), P(gw), 3, cin, H, W, cout, k, stride, pad, _C.stream()), "wgrad")
    assert _rel(gw, 2.0 * ref) <= 2e-6                 # accumulates
    assert not L.cp_conv_direct_wgrad_supported(16, 16, 3, 2, 1)


@pytest.mark.parametrize("shape", [(2, 128, 64, 40, 72), (1, 256, 27, 17, 36), (3, 64, 256, 9, 28), (2, 96, 8, 24, 64)],
                         ids=["128->64", "256->27", "64->256", "96->8"])
def test_1x1_weight_gradient_and_autograd(shape):
    """The 1x1 form: weight gradient through the C ABI, and forward / both gradients through the autograd wrapper."""
    from centerpoly_amd.models.networks import conv3x3
    B, ci, co, H, W = shape
    L = _C.lib()
    x, go = _t("p1x%s" % (shape,), (B, ci, H, W)), _t("p1go%s" % (shape,), (B, co, H, W))
    gw = torch.zeros((co, ci, 1, 1), device=DEV)
    _C.check(L.cp_conv_mfma_wgrad(P(x), P(go), P(gw), B, ci, H, W, co, 1, _C.stream()), "wgrad")
    ref = torch.nn.grad.conv2d_weight(x.double(), (co, ci, 1, 1), go.double())
    assert _rel(gw, ref) <= TOL
    conv = torch.nn.Conv2d(ci, co, 1, bias=False).to(DEV)
    xr = x.clone().requires_grad_(True)
    if conv3x3.usable(conv, xr):
        y = conv3x3.conv_raw(conv, xr)
        gx, gwa = torch.autograd.grad(y, (xr, conv.weight), go)
        xd, wd = x.double().requires_grad_(True), conv.weight.detach().double().requires_grad_(True)
        yd = F.conv2d(xd, wd)
        gxd, gwd = torch.autograd.grad(yd, (xd, wd), go.double())
        assert _rel(y, yd.detach()) <= TOL and _rel(gx, gxd) <= TOL and _rel(gwa, gwd) <= TOL


@pytest.mark.parametrize("shape", [(2, 32, 64, 40, 72), (1, 64, 128, 17, 33), (1, 128, 256, 64, 128), (2, 256, 48, 9, 31),
                                   (1, 27, 64, 12, 130), (1, 64, 256, 128, 512), (1, 128, 256, 256, 256)],
                         ids=["32->64", "64->128", "128->256", "256->48", "27->64", "64->256 wide tiles", "hourglass pre"])
def test_stride_2_forward(shape):
    """The stride-2 3x3 form (first convolution of DLA levels 2-5): odd and even map sizes, ragged channels."""
    B, ci, co, H, W = shape
    L = _C.lib()
    x, w = _t("s2x%s" % (shape,), (B, ci, H, W)), _t("s2w%s" % (shape,), (co, ci, 3, 3), 0.05)
    bias = _t("s2b", (co,))
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    res = _t("s2r%s" % (shape,), (B, co, Ho, Wo))
    wp = torch.empty(L.cp_conv_mfma_weight_bytes(ci, co, 9), dtype=torch.uint8, device=DEV)
    _C.check(L.cp_conv_mfma_prepare(P(w), ci, co, 9, 0, P(wp), _C.stream()), "prepare")
    out = torch.full((B, co, Ho, Wo), float("nan"), device=DEV)
    ptrs, chans = (ctypes.c_void_p * 1)(x.data_ptr()), (ctypes.c_int32 * 1)(ci)
    _C.check(L.cp_conv_mfma_forward_strided(ptrs, chans, 1, P(wp), P(bias), P(res), P(out), B, H, W, co, 9, 2, 1,
                                            _C.stream()), "forward")
    ref = F.relu(F.conv2d(x.double(), w.double(), bias.double(), stride=2, padding=1) + res.double())
    assert tuple(ref.shape) == tuple(out.shape)
    assert torch.isfinite(out).all() and _rel(out, ref) <= TOL
    out2 = torch.full((B, co, Ho, Wo), float("nan"), device=DEV)
    _C.check(L.cp_conv_mfma_forward_strided(ptrs, chans, 1, P(wp), P(bias), P(res), P(out2), B, H, W, co, 9, 2, 1,
                                            _C.stream()), "forward")
    assert torch.equal(out, out2)                         # fixed order, no atomics: bit-identical reruns
    assert L.cp_conv_mfma_forward_strided(ptrs, chans, 1, P(wp), None, None, P(out), B, H, W, co, 9, 3, 0,
                                          _C.stream()) == -2      # strides 1 and 2 only


@pytest.mark.parametrize("shape", [(2, 32, 64, 40, 72), (1, 64, 128, 17, 33), (1, 128, 256, 256, 512), (1, 256, 384, 64, 128),
                                   (1, 384, 384, 16, 32), (2, 384, 512, 8, 16), (1, 27, 40, 9, 131)],
                         ids=["32->64", "odd map", "hourglass pre skip", "256->384", "384->384 small", "tiny map", "ragged"])
def test_stride_2_pointwise_forward(shape):
    """The stride-2 1x1 form (skip convolutions of the Hourglass' down-sampling residuals, large_hourglass.py:55-81):
    a 1x1 convolution of every second pixel, with bias + residual + ReLU in the epilogue."""
    B, ci, co, H, W = shape
    L = _C.lib()
    x, w = _t("p2x%s" % (shape,), (B, ci, H, W)), _t("p2w%s" % (shape,), (co, ci, 1, 1), 0.05)
    bias = _t("p2b", (co,))
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    res = _t("p2r%s" % (shape,), (B, co, Ho, Wo))
    wp = torch.empty(L.cp_conv_mfma_weight_bytes(ci, co, 1), dtype=torch.uint8, device=DEV)
    _C.check(L.cp_conv_mfma_prepare(P(w), ci, co, 1, 0, P(wp), _C.stream()), "prepare")
    out = torch.full((B, co, Ho, Wo), float("nan"), device=DEV)
    ptrs, chans = (ctypes.c_void_p * 1)(x.data_ptr()), (ctypes.c_int32 * 1)(ci)
    _C.check(L.cp_conv_mfma_forward_strided(ptrs, chans, 1, P(wp), P(bias), P(res), P(out), B, H, W, co, 1, 2, 1,
                                            _C.stream()), "forward")
    ref = F.relu(F.conv2d(x.double(), w.double(), bias.double(), stride=2) + res.double())
    assert tuple(ref.shape) == tuple(out.shape)
    assert torch.isfinite(out).all() and _rel(out, ref) <= TOL


@pytest.mark.parametrize("shape", [(2, 32, 64, 40, 72), (1, 64, 128, 17, 33), (1, 128, 256, 64, 128), (2, 256, 512, 32, 64),
                                   (1, 27, 64, 12, 130), (4, 32, 64, 128, 256), (2, 16, 32, 96, 160)],
                         ids=["32->64", "odd map", "128->256", "256->512", "ragged channels", "level2 size / 4", "level1 (16 <- 32)"])
def test_stride_2_input_gradient(shape):
    """cp_conv3x3_s2_input_grad: the input gradient of a 3x3 / stride 2 / pad 1 convolution against
    torch.nn.grad.conv2d_input in float64; every element of grad_in written (NaN prefill)."""
    B, ci, co, H, W = shape
    L = _C.lib()
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    w, go = _t("s2gw%s" % (shape,), (co, ci, 3, 3), 0.05), _t("s2go%s" % (shape,), (B, co, Ho, Wo))
    ref = torch.nn.grad.conv2d_input((B, ci, H, W), w.double(), go.double(), stride=2, padding=1)
    # one launch (four class accumulators over one staged grad_out tile), alone and onto a residual in place
    wp = torch.empty(L.cp_conv_mfma_weight_bytes(co, ci, 9), dtype=torch.uint8, device=DEV)
    _C.check(L.cp_conv_mfma_prepare(P(w), co, ci, 9, 6, P(wp), _C.stream()), "prepare")
    g1 = torch.full((B, ci, H, W), float("nan"), device=DEV)
    _C.check(L.cp_conv3x3_s2_input_grad(P(go), P(wp), None, P(g1), B, ci, H, W, co, _C.stream()), "igrad one launch")
    assert torch.isfinite(g1).all() and _rel(g1, ref) <= TOL
    res = _t("s2res%s" % (shape,), (B, ci, H, W))
    g2 = res.clone()
    _C.check(L.cp_conv3x3_s2_input_grad(P(go), P(wp), P(g2), P(g2), B, ci, H, W, co, _C.stream()), "igrad + residual")
    assert _rel(g2, ref + res.double()) <= TOL


@pytest.mark.parametrize("cfg", [(2, 64, 256, 8, 64, 136), (2, 64, 128, 32, 64, 136), (4, 48, 64, 1, 36, 132), (4, 64, 256, 2, 32, 64)],
                         ids=["hm (8)", "poly (32)", "pseudo_depth (1), ragged map", "reg (2)"])
def test_training_head_single_node(cfg):
    """conv3x3.head_train: Conv2d(3x3, bias) -> ReLU -> Conv2d(1x1, bias) as one autograd node whose backward masks the
    1x1 input gradient and sums the 3x3 bias gradient in the kernel's epilogue (cp_conv_mfma_input_grad_relu): outputs and
    all five gradients against float64 torch."""
    from centerpoly_amd.models.networks import conv3x3
    B, cin, hc, co, H, W = cfg
    fc = torch.nn.Sequential(torch.nn.Conv2d(cin, hc, 3, padding=1), torch.nn.ReLU(), torch.nn.Conv2d(hc, co, 1)).to(DEV)
    with torch.no_grad():
        fc[0].weight.copy_(_t("hw1%s" % (cfg,), (hc, cin, 3, 3), 0.05)); fc[0].bias.copy_(_t("hb1%s" % (cfg,), (hc,), 0.3))
        fc[2].weight.copy_(_t("hw2%s" % (cfg,), (co, hc, 1, 1), 0.1)); fc[2].bias.copy_(_t("hb2%s" % (cfg,), (co,)))
    x = _t("hx%s" % (cfg,), (B, cin, H, W)).requires_grad_(True)
    out = conv3x3.head_train(fc, x)
    if out is None:
        pytest.skip("shape not taken by the MFMA kernels (grid too small)")
    go = _t("hgo%s" % (cfg,), tuple(out.shape))
    params = [fc[0].weight, fc[0].bias, fc[2].weight, fc[2].bias]
    grads = torch.autograd.grad(out, [x] + params, go)
    xd = x.detach().double().requires_grad_(True)
    pd = [p.detach().double().requires_grad_(True) for p in params]
    # the reference takes the ReLU's mask from the kernel's own hidden map (the same launch head_train makes): a hidden
    # value within rounding of zero may sit on the other side in float64, and one flipped element is 1e-2 of grad_x's norm
    with torch.no_grad():
        keep = (conv3x3.conv_bias_act(fc[0], x.detach(), True) > 0).double()
    yd = F.conv2d(F.conv2d(xd, pd[0], pd[1], padding=1) * keep, pd[2], pd[3])
    gd = torch.autograd.grad(yd, [xd] + pd, go.double())
    assert _rel(out, yd.detach()) <= TOL
    for name, a, b in zip(("x", "w1", "b1", "w2", "b2"), grads, gd):
        assert torch.isfinite(a).all() and _rel(a, b) <= 1e-4, name


def test_training_heads_share_one_node():
    """conv3x3.heads_train: the four polydet heads over one feature map as ONE autograd node -- the shared input's gradient
    is accumulated by the heads' input-gradient launches; all outputs and the input gradient against float64 torch (the
    ReLU masks taken from the kernel's own hidden maps, as above), also with one head's output unused."""
    from centerpoly_amd.models.networks import conv3x3
    B, cin, hc, H, W = 2, 64, 128, 64, 136
    couts = (8, 32, 1, 2)
    fcs = []
    for i, co in enumerate(couts):
        fc = torch.nn.Sequential(torch.nn.Conv2d(cin, hc, 3, padding=1), torch.nn.ReLU(), torch.nn.Conv2d(hc, co, 1)).to(DEV)
        with torch.no_grad():
            fc[0].weight.copy_(_t("mh1%d" % i, (hc, cin, 3, 3), 0.05)); fc[0].bias.copy_(_t("mhb1%d" % i, (hc,), 0.3))
            fc[2].weight.copy_(_t("mh2%d" % i, (co, hc, 1, 1), 0.1)); fc[2].bias.copy_(_t("mhb2%d" % i, (co,)))
        fcs.append(fc)
    x = _t("mhx", (B, cin, H, W)).requires_grad_(True)
    outs = conv3x3.heads_train(fcs, x)
    assert outs is not None and len(outs) == 4
    gos = [_t("mhgo%d" % i, tuple(o.shape)) for i, o in enumerate(outs)]
    xd = x.detach().double().requires_grad_(True)
    refs = []
    for fc in fcs:
        with torch.no_grad():
            keep = (conv3x3.conv_bias_act(fc[0], x.detach(), True) > 0).double()
        refs.append(F.conv2d(F.conv2d(xd, fc[0].weight.detach().double(), fc[0].bias.detach().double(), padding=1) * keep,
                             fc[2].weight.detach().double(), fc[2].bias.detach().double()))
    for used in ((0, 1, 2, 3), (0, 2, 3)):
        (gx,) = torch.autograd.grad([outs[i] for i in used], [x], [gos[i] for i in used], retain_graph=True)
        (gxd,) = torch.autograd.grad([refs[i] for i in used], [xd], [gos[i].double() for i in used], retain_graph=True)
        assert _rel(gx, gxd) <= 1e-4, used
    for o, r in zip(outs, refs):
        assert _rel(o, r.detach()) <= TOL
    gw = torch.autograd.grad(outs, [fc[0].weight for fc in fcs], gos, retain_graph=True)
    gwd = torch.autograd.grad(refs, [xd], [g.double() for g in gos])          # (keeps the float64 graph alive until here)
    assert all(torch.isfinite(g).all() for g in gw) and torch.isfinite(gwd[0]).all()


def test_skip_gradient_joins_in_the_input_gradient_launch():
    """conv3x3.conv_raw_skip: (conv(x), x) as one autograd node whose backward adds the skip's gradient in the
    input-gradient kernel's epilogue; against float64 torch, with and without a gradient on the skip."""
    from centerpoly_amd.models.networks import conv3x3
    conv = torch.nn.Conv2d(64, 64, 3, padding=1, bias=False).to(DEV)
    x = _t("skx", (2, 64, 64, 136)).requires_grad_(True)
    y, skip = conv3x3.conv_raw_skip(conv, x)
    assert skip.data_ptr() == x.data_ptr()
    gy, gs = _t("skgy", tuple(y.shape)), _t("skgs", tuple(x.shape))
    gx, gw = torch.autograd.grad([y, skip], (x, conv.weight), [gy, gs], retain_graph=True)
    xd, wd = x.detach().double().requires_grad_(True), conv.weight.detach().double().requires_grad_(True)
    yd = F.conv2d(xd, wd, padding=1)
    gxd, gwd = torch.autograd.grad([yd, xd * 1.0], (xd, wd), [gy.double(), gs.double()])
    assert _rel(y, yd.detach()) <= TOL and _rel(gx, gxd) <= 1e-4 and _rel(gw, gwd) <= 1e-4
    (gx2,) = torch.autograd.grad(y, x, gy)                     # skip unused: plain input gradient
    (gxd2,) = torch.autograd.grad(F.conv2d(xd, wd, padding=1), xd, gy.double())
    assert _rel(gx2, gxd2) <= 1e-4


@pytest.mark.parametrize("cs", [(64, 64), (128, 128, 64), (256, 256, 128, 64)], ids=["2 sources", "3 sources", "4 sources"])
def test_concatenated_1x1_training_node(cs):
    """conv3x3.concat_conv1x1 (Root in training): conv(cat(xs)) with the sources read in place, per-source input and
    weight gradients; against float64 torch over the concatenation."""
    from centerpoly_amd.models.networks import conv3x3
    co = cs[0]
    conv = torch.nn.Conv2d(sum(cs), co, 1, bias=False).to(DEV)
    xs = [_t("ccx%d%s" % (i, cs), (2, c, 64, 128)).requires_grad_(True) for i, c in enumerate(cs)]
    y = conv3x3.concat_conv1x1(conv, xs)
    assert y is not None
    go = _t("ccgo%s" % (cs,), tuple(y.shape))
    grads = torch.autograd.grad(y, xs + [conv.weight], go)
    xd = [x.detach().double().requires_grad_(True) for x in xs]
    wd = conv.weight.detach().double().requires_grad_(True)
    yd = F.conv2d(torch.cat(xd, 1), wd)
    gd = torch.autograd.grad(yd, xd + [wd], go.double())
    assert _rel(y, yd.detach()) <= TOL
    for a, b in zip(grads, gd):
        assert a.is_contiguous() and _rel(a, b) <= 1e-4


def test_weight_bank_serves_only_current_versions():
    """conv3x3's weight bank (one cp_conv_mfma_prepare_batch launch per optimizer step): a parameter's permuted forms
    are served from the bank only at the version they were permuted at; an in-place change falls back to the per-use
    path until the next refresh; temporaries never enter the bank."""
    from centerpoly_amd.models.networks import conv3x3
    conv = torch.nn.Conv2d(64, 64, 3, padding=1, bias=False).to(DEV)
    conv2 = torch.nn.Conv2d(64, 128, 3, stride=2, padding=1, bias=False).to(DEV)
    x = _t("wbx", (2, 64, 128, 136)).requires_grad_(True)
    ref = lambda c: F.conv2d(x.detach().double(), c.weight.detach().double(), stride=c.stride, padding=1)

    def run():
        y, y2 = conv3x3.conv_raw(conv, x), conv3x3.conv_raw(conv2, x)
        gx, = torch.autograd.grad([y.sum() + y2.sum()], [x])
        return y, y2, gx
    y, y2, gx0 = run()                                           # registers the forms (forward, transposed, stride-2 gradient)
    assert _rel(y, ref(conv)) <= TOL and _rel(y2, ref(conv2)) <= TOL
    assert conv3x3._BANK.get(conv.weight, 64, 64, 0) is None     # registered, not yet permuted
    conv3x3.refresh_weight_bank()
    for code, (ci, co, w) in {0: (64, 64, conv.weight), 1: (64, 64, conv.weight), 6: (128, 64, conv2.weight)}.items():
        assert conv3x3._BANK.get(w, ci, co, code) is not None, code
    y, y2, gx1 = run()                                           # served from the bank
    assert _rel(y, ref(conv)) <= TOL and _rel(y2, ref(conv2)) <= TOL and torch.equal(gx0, gx1)
    with torch.no_grad():
        conv.weight.mul_(-1.5)
        conv2.weight.add_(0.01)
    assert conv3x3._BANK.get(conv.weight, 64, 64, 0) is None     # stale: per-use path
    y, y2, gx2 = run()
    assert _rel(y, ref(conv)) <= TOL and _rel(y2, ref(conv2)) <= TOL and not torch.equal(gx1, gx2)
    conv3x3.refresh_weight_bank()
    y, y2, gx3 = run()
    assert _rel(y, ref(conv)) <= TOL and _rel(y2, ref(conv2)) <= TOL and torch.equal(gx2, gx3)
    n = len(conv3x3._BANK.entries)
    conv3x3._prepare(conv.weight[:, :32].contiguous(), 32, 64, False)      # a temporary: not registered
    assert len(conv3x3._BANK.entries) == n


@pytest.mark.parametrize("cfg", [(2, 128, 64, 96, 2), (1, 128, 37, 70, 2), (1, 96, 130, 258, 2), (3, 64, 9, 33, 2),
                                 (2, 16, 64, 96, 1), (1, 16, 37, 70, 1), (1, 16, 130, 258, 1), (1, 24, 9, 33, 1), (2, 16, 41, 67, 2)],
                         ids=["128 ch", "ragged map", "96 channels, off the tile grid", "tiny", "base layer (16, stride 1)",
                              "base layer, ragged map", "base layer, off the tile grid", "24 channels stride 1", "16 channels stride 2"])
def test_hourglass_stem_kernel(cfg):
    """cp_conv7x7_c3_forward: 7x7 / pad 3 over a 3-channel image (+ bias + ReLU), stride 2 (Hourglass stem) and stride 1
    (DLA base layer), against float64 torch."""
    B, co, H, W, S = cfg
    L = _C.lib()
    x, w, bias = _t("stx%s" % (cfg,), (B, 3, H, W)), _t("stw%s" % (cfg,), (co, 3, 7, 7), 0.1), _t("stb%s" % (cfg,), (co,))
    assert L.cp_conv7x7_c3_supported(co, H, W, S)
    wp = torch.empty(L.cp_conv7x7_c3_weight_bytes(co), dtype=torch.uint8, device=DEV)
    _C.check(L.cp_conv7x7_c3_prepare(P(w), co, P(wp), _C.stream()), "prepare")
    Ho, Wo = (H - 1) // S + 1, (W - 1) // S + 1
    for relu in (1, 0):
        out = torch.full((B, co, Ho, Wo), float("nan"), device=DEV)
        _C.check(L.cp_conv7x7_c3_forward(P(x), P(wp), P(bias), P(out), B, H, W, co, S, relu, _C.stream()), "stem")
        ref = F.conv2d(x.double(), w.double(), bias.double(), stride=S, padding=3)
        ref = F.relu(ref) if relu else ref
        assert tuple(ref.shape) == tuple(out.shape)
        assert torch.isfinite(out).all() and _rel(out, ref) <= TOL


@pytest.mark.parametrize("shape", [(2, 32, 64, 40, 72), (1, 64, 128, 17, 40), (1, 128, 256, 64, 128), (2, 256, 512, 32, 64),
                                   (1, 27, 70, 12, 136), (4, 32, 64, 128, 256)],
                         ids=["32->64", "odd height", "128->256", "256->512", "ragged channels", "level2 size / 4"])
def test_stride_2_weight_gradient(shape):
    """cp_conv3x3_s2_wgrad: the weight gradient of a 3x3 / stride 2 / pad 1 convolution against torch.nn.grad.conv2d_weight
    in float64; accumulates into gw."""
    B, ci, co, H, W = shape
    L = _C.lib()
    assert L.cp_conv3x3_s2_wgrad_supported(ci, co, H, W)
    Ho, Wo = (H - 1) // 2 + 1, W // 2
    x, go = _t("s2wx%s" % (shape,), (B, ci, H, W)), _t("s2wgo%s" % (shape,), (B, co, Ho, Wo))
    gw = torch.zeros((co, ci, 3, 3), device=DEV)
    _C.check(L.cp_conv3x3_s2_wgrad(P(x), P(go), P(gw), B, ci, H, W, co, _C.stream()), "s2 wgrad")
    ref = torch.nn.grad.conv2d_weight(x.double(), (co, ci, 3, 3), go.double(), stride=2, padding=1)
    assert torch.isfinite(gw).all() and _rel(gw, ref) <= 1e-4
    _C.check(L.cp_conv3x3_s2_wgrad(P(x), P(go), P(gw), B, ci, H, W, co, _C.stream()), "s2 wgrad")      # accumulates
    assert _rel(gw, 2 * ref) <= 1e-4


def test_stride_2_autograd_wrapper():
    """conv_raw on a stride-2 3x3 convolution: forward, input gradient and weight gradient from the MFMA kernels."""
    from centerpoly_amd.models.networks import conv3x3
    conv = torch.nn.Conv2d(64, 128, 3, stride=2, padding=1, bias=False).to(DEV)
    x = _t("s2ax", (4, 64, 64, 128)).requires_grad_(True)
    assert conv3x3.usable(conv, x)
    y = conv3x3.conv_raw(conv, x)
    assert tuple(y.shape) == (4, 128, 32, 64)
    go = _t("s2ago", tuple(y.shape))
    gx, gw = torch.autograd.grad(y, (x, conv.weight), go)
    xd, wd = x.detach().double().requires_grad_(True), conv.weight.detach().double().requires_grad_(True)
    yd = F.conv2d(xd, wd, stride=2, padding=1)
    gxd, gwd = torch.autograd.grad(yd, (xd, wd), go.double())
    assert _rel(y, yd.detach()) <= TOL and _rel(gx, gxd) <= 1e-4 and _rel(gw, gwd) <= 1e-4


@pytest.mark.parametrize("cfg", [((8, 32, 1, 2), 256, 64, 40, 72), ((8, 32), 128, 96, 17, 33), ((3,), 64, 32, 8, 32),
                                 ((8, 48, 1, 2), 256, 256, 16, 64), ((64, 2), 64, 32, 9, 31)],
                         ids=["polydet heads", "two heads hc128", "one head hc64", "hourglass polar heads (48)", "64 classes"])
def test_fused_heads_kernel(cfg):
    """cp_heads_fused_forward: conv3x3 + bias + ReLU + conv1x1 + bias of up to four heads in one launch against
    float64 torch (ragged map sizes, 1 .. 32 classes, head_conv 64 / 128 / 256)."""
    couts, hc, cin, H, W = cfg
    L = _C.lib()
    B, nh = 2, len(couts)
    x = _t("hf/x%s" % (cfg,), (B, cin, H, W))
    w1 = _t("hf/w1%s" % (cfg,), (nh * hc, cin, 3, 3), 0.05)
    b1 = _t("hf/b1%s" % (cfg,), (nh * hc,))
    w2 = [_t("hf/w2_%d%s" % (i, cfg), (co, hc), 0.1) for i, co in enumerate(couts)]
    b2 = [_t("hf/b2_%d%s" % (i, cfg), (co,)) for i, co in enumerate(couts)]
    wp1 = torch.empty(L.cp_conv_mfma_weight_bytes(cin, nh * hc, 9), dtype=torch.uint8, device=DEV)
    _C.check(L.cp_conv_mfma_prepare(P(w1), cin, nh * hc, 9, 0, P(wp1), _C.stream()), "prepare")
    w2p = []
    for w, co in zip(w2, couts):
        buf = torch.empty(L.cp_heads_fused_w2_bytes(hc), dtype=torch.uint8, device=DEV)
        _C.check(L.cp_heads_fused_prepare_w2(P(w), co, hc, P(buf), _C.stream()), "prepare_w2")
        w2p.append(buf)
    outs = [torch.full((B, co, H, W), float("nan"), device=DEV) for co in couts]
    vp = ctypes.c_void_p
    rc = L.cp_heads_fused_forward(P(x), P(wp1), P(b1), (vp * nh)(*[t.data_ptr() for t in w2p]),
                                  (vp * nh)(*[t.data_ptr() for t in b2]), (vp * nh)(*[t.data_ptr() for t in outs]),
                                  (ctypes.c_int32 * nh)(*couts), nh, B, cin, H, W, hc, _C.stream())
    assert rc == 0
    hid = F.relu(F.conv2d(x.double(), w1.double(), b1.double(), padding=1))
    for i, co in enumerate(couts):
        ref = F.conv2d(hid[:, i * hc:(i + 1) * hc], w2[i].double().view(co, hc, 1, 1), b2[i].double())
        assert torch.isfinite(outs[i]).all() and _rel(outs[i], ref) <= TOL, i


# ---- split activations (round 4): [hi | lo] bf16 planes between producer and consumer ---------------------------------
def _np_split(x):
    """[B][C][H][W] float32 -> (hi, lo) planes [B][C/8][H][W][8] as uint16 bf16 bit patterns, round-to-nearest-even."""
    def bf16_bits(v):
        u = v.view(np.uint32).astype(np.uint64)
        r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
        return r
    B, C, H, W = x.shape
    hi = bf16_bits(x)
    hif = (hi.astype(np.uint32) << 16).view(np.float32)
    lo = bf16_bits((x - hif).astype(np.float32))
    lay = lambda p: np.ascontiguousarray(p.reshape(B, C // 8, 8, H, W).transpose(0, 1, 3, 4, 2))
    return lay(hi), lay(lo)


def _split_conv(x, x_split, w, bias, residual, out_split, relu, stride=1):
    L = _C.lib()
    B, cin, H, W = x.shape
    cout = w.shape[0]
    wp = torch.empty(L.cp_conv_mfma_weight_bytes(cin, cout, 9), dtype=torch.uint8, device=DEV)
    _C.check(L.cp_conv_mfma_prepare(P(w), cin, cout, 9, 0, P(wp), _C.stream()), "prepare")
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    out = torch.full((B, cout, Ho, Wo), float("nan"), device=DEV)
    rc = L.cp_conv_mfma_forward_split(P(x_split if x_split is not None else x), 1 if x_split is not None else 0, P(wp), P(bias),
                                      P(residual), P(out), 1 if out_split else 0, B, cin, H, W, cout, 9, stride,
                                      1 if relu else 0, _C.stream())
    return rc, out


def _to_split(x):
    B, C, H, W = x.shape
    s = torch.empty_like(x)
    _C.check(_C.lib().cp_activation_split(P(x), P(s), B, C, H, W, _C.stream()), "cp_activation_split")
    return s


def test_activation_split_layout_and_round_trip():
    x = _t("splitx", (2, 24, 5, 19), 3.0)
    x[0, 3, 2, 7] = 0.0
    x[1, 9, 4, 18] = 1e-30
    s = _to_split(x)
    hi, lo = _np_split(x.cpu().numpy())
    got = s.cpu().numpy().view(np.uint16).reshape(2, *hi.shape)          # [plane][B][C/8][H][W][8]
    assert np.array_equal(got[0], hi) and np.array_equal(got[1], lo)
    back = torch.empty_like(x)
    _C.check(_C.lib().cp_activation_unsplit(P(s), P(back), 2, 24, 5, 19, _C.stream()), "cp_activation_unsplit")
    assert (back - x).abs().max().item() <= 2.0 ** -16 * x.abs().max().item()
    assert _C.lib().cp_activation_split(P(x), P(s), 2, 12, 5, 38, _C.stream()) == -2          # C % 8 != 0


# (B, Cin, Cout, H, W): every tile form of the dispatch (64 x 8 rows, 32 x 16, 32 x 8, the in-workgroup K splits, 32 x 4)
# and ragged map edges
SPLIT_SHAPES = [(2, 64, 64, 64, 128), (1, 32, 32, 256, 64), (1, 64, 64, 40, 72), (1, 256, 64, 16, 32), (1, 128, 32, 24, 40),
                (1, 32, 24, 9, 31), (3, 96, 40, 7, 33)]


@pytest.mark.parametrize("shape", SPLIT_SHAPES, ids=["x".join(map(str, s)) for s in SPLIT_SHAPES])
def test_split_forms_equal_the_float32_route_bitwise(shape):
    B, ci, co, H, W = shape
    x, w, bias = _t("sx%s" % (shape,), (B, ci, H, W)), _t("sw%s" % (shape,), (co, ci, 3, 3), 0.05), _t("sb", (co,))
    res = _t("sr%s" % (shape,), (B, co, H, W))
    xs = _to_split(x)
    rc, ref = _split_conv(x, None, w, bias, res, False, True)
    assert rc == 0 and torch.isfinite(ref).all()
    assert _rel(ref, F.relu(F.conv2d(x.double(), w.double(), bias.double(), padding=1) + res.double())) <= TOL
    rc, out = _split_conv(x, xs, w, bias, res, False, True)                    # split in, float32 out (conv2 of a block)
    assert rc == 0 and torch.equal(out, ref)
    rc, ref1 = _split_conv(x, None, w, bias, None, False, True)                # conv1 of a block: bias + ReLU
    want = _to_split(ref1)
    for xin in (None, xs):
        rc, out = _split_conv(x, xin, w, bias, None, True, True)
        assert rc == 0
        assert torch.equal(out.view(torch.int32), want.view(torch.int32))      # every unit of both planes written
    # stride-2 producer (the first convolution of a DLA level) writing split planes
    rc, ref2 = _split_conv(x, None, w, bias, None, False, True, stride=2)
    rc2, out2 = _split_conv(x, None, w, bias, None, True, True, stride=2)
    assert rc == 0 and rc2 == 0
    assert torch.equal(out2.view(torch.int32), _to_split(ref2).view(torch.int32))


def test_split_forms_refuse_what_they_do_not_cover():
    x, w = _t("rx", (1, 48, 8, 32)), _t("rw", (20, 48, 3, 3), 0.05)
    assert _split_conv(x, _to_split(x), w, None, None, False, False)[0] == -2     # Cin % 32 != 0
    assert _split_conv(x, None, w, None, None, True, False)[0] == -2              # Cout % 8 != 0
    w2, r = _t("rw2", (16, 48, 3, 3), 0.05), _t("rr", (1, 16, 8, 32))
    assert _split_conv(x, None, w2, None, r, True, False)[0] == -2                # residual with split output


@pytest.mark.parametrize("case", [("dla", 64, 128, 2, 96, 192), ("dla", 128, 128, 1, 40, 72), ("hourglass", 256, 256, 1, 24, 40),
                                  ("hourglass", 256, 384, 2, 32, 64)], ids=lambda c: "%s-%d-%d-s%d" % c[:4])
def test_residual_blocks_with_split_intermediate_equal_the_float32_route(case):
    """BasicBlock (pose_dla_dcn.py:38-66) / residual (large_hourglass.py:55-81) at inference: conv1 -> split planes ->
    conv2 gives the bits of conv1 -> float32 -> conv2."""
    from centerpoly_amd.models.networks import conv3x3, large_hourglass, pose_dla_dcn
    kind, cin, cout, stride, H, W = case
    torch.manual_seed(3)
    if kind == "dla":
        blk = pose_dla_dcn.BasicBlock(cin, cout, stride).to(DEV).eval()
    else:
        blk = large_hourglass.residual(3, cin, cout, stride=stride).to(DEV).eval()
    for m in blk.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_mean.normal_(0, 0.2)
            m.running_var.uniform_(0.5, 1.5)
            m.weight.data.uniform_(0.5, 1.5)
            m.bias.data.normal_(0, 0.2)
    blk.fold()
    x = _t("blk%s" % (case,), (2, cin, H, W))
    skip = _t("blkskip%s" % (case,), (2, cout, (H - 1) // stride + 1, (W - 1) // stride + 1))
    f1, f2 = blk._folded[0], blk._folded[1]
    with torch.no_grad():
        z = conv3x3.block_infer(x, blk.conv1, f1, blk.conv2, f2, skip)
        assert z is not None                                   # the split route ran
        y = conv3x3.conv_infer([x], blk.conv1, f1[0], f1[1], None, True, conv=blk.conv1)
        ref = conv3x3.conv_infer([y], blk.conv2, f2[0], f2[1], skip, True, conv=blk.conv2)
        assert torch.equal(z, ref)
        lin = F.relu(F.conv2d(x.double(), f1[0].double(), f1[1].double(), stride=stride, padding=1))
        full = F.relu(F.conv2d(lin, f2[0].double(), f2[1].double(), padding=1) + skip.double())
        assert _rel(z, full) <= 2 * TOL                        # two chained contractions
        if kind == "dla":
            assert torch.equal(blk(x, skip), ref)              # the module takes the same route


@pytest.mark.parametrize("k,cin,cout,stride", [(3, 64, 64, 1), (7, 3, 128, 2)], ids=["conv_infer", "stem_infer"])
def test_prepared_weights_follow_a_repointed_parameter(k, cin, cout, stride):
    """Hourglass convolution(with_bn=False) folds to its Parameters themselves: a `.data` swap after fold() points the
    weight at new storage without a version bump, and the next inference call must run with the new weights, not with
    the permuted form prepared from the old ones (3x3: the MFMA convolution; 7x7 / 3 channels: the stem kernel)."""
    from centerpoly_amd.models.networks import large_hourglass
    torch.manual_seed(4)
    m = large_hourglass.convolution(k, cin, cout, stride=stride, with_bn=False).to(DEV).eval()
    m.fold()
    x = _t("repoint/x%d" % k, (1, cin, 64, 128))
    new = _t("repoint/w%d" % k, tuple(m.conv.weight.shape), 0.05)
    keys = set(m.conv.__dict__)
    with torch.no_grad():
        m(x)
        assert set(m.conv.__dict__) != keys                # the kernel route ran: it kept a prepared form on the conv
        m.conv.weight.data = new
        out = m(x)
    ref = F.relu(F.conv2d(x.double(), new.double(), m.conv.bias.double(), stride=stride, padding=k // 2))
    assert _rel(out, ref) <= TOL


# ---- level0 + level1 of the DLA base in one launch (csrc/conv_base_pair.hip) -------------------------------------------
PAIR_SHAPES = [(1, 64, 128), (2, 37, 100), (1, 8, 4), (1, 5, 36), (2, 130, 72), (1, 1, 8)]


@pytest.mark.parametrize("shape", PAIR_SHAPES, ids=["x".join(map(str, s)) for s in PAIR_SHAPES])
def test_base_pair_kernel_matches_float64_and_the_separate_route(shape):
    """cp_dla_base_pair_forward against relu(conv_s2(relu(conv(x)))) in float64 (2 chained split-bf16 contractions: 4e-5
    of the max-norm) and against the two direct kernels it replaces; odd heights, maps smaller than a tile, borders."""
    B, H, W = shape
    L = _C.lib()
    x = _t("pairx%s" % (shape,), (B, 16, H, W))
    w0, b0 = _t("pairw0", (16, 16, 3, 3), 0.1), _t("pairb0", (16,), 0.2)
    w1, b1 = _t("pairw1", (32, 16, 3, 3), 0.1), _t("pairb1", (32,), 0.2)
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    assert L.cp_dla_base_pair_supported(H, W)
    out = torch.full((B, 32, Ho, Wo), float("nan"), device=DEV)
    _C.check(L.cp_dla_base_pair_forward(P(x), P(w0), P(b0), P(w1), P(b1), P(out), B, H, W, _C.stream()), "pair")
    assert torch.isfinite(out).all()
    ref = F.relu(F.conv2d(F.relu(F.conv2d(x.double(), w0.double(), b0.double(), padding=1)), w1.double(), b1.double(),
                          stride=2, padding=1))
    assert _rel(out, ref) <= 2 * TOL
    y0 = torch.empty((B, 16, H, W), device=DEV)
    _C.check(L.cp_conv_direct_forward_ex(P(x), P(w0), P(b0), P(y0), B, 16, H, W, 16, 3, 1, 1, 1, 1, _C.stream()), "level0")
    y1 = torch.empty((B, 32, Ho, Wo), device=DEV)
    _C.check(L.cp_conv_direct_forward_ex(P(y0), P(w1), P(b1), P(y1), B, 16, H, W, 32, 3, 2, 1, 1, 1, _C.stream()), "level1")
    assert _rel(out, y1.double()) <= 2 * TOL
    out2 = torch.empty_like(out)
    _C.check(L.cp_dla_base_pair_forward(P(x), P(w0), P(b0), P(w1), P(b1), P(out2), B, H, W, _C.stream()), "pair")
    assert torch.equal(out, out2)                                   # run-to-run identical
    # without biases
    _C.check(L.cp_dla_base_pair_forward(P(x), P(w0), None, P(w1), None, P(out2), B, H, W, _C.stream()), "pair")
    ref0 = F.relu(F.conv2d(F.relu(F.conv2d(x.double(), w0.double(), padding=1)), w1.double(), stride=2, padding=1))
    assert _rel(out2, ref0) <= 2 * TOL


def test_base_pair_kernel_refuses_widths_it_does_not_cover():
    L = _C.lib()
    assert not L.cp_dla_base_pair_supported(16, 30)
    x = _t("pairrx", (1, 16, 16, 30))
    w0, w1 = _t("pairw0", (16, 16, 3, 3), 0.1), _t("pairw1", (32, 16, 3, 3), 0.1)
    out = torch.empty((1, 32, 8, 15), device=DEV)
    assert L.cp_dla_base_pair_forward(P(x), P(w0), None, P(w1), None, P(out), 1, 16, 30, _C.stream()) == -2

"""GPU parity of the streaming 3x3 convolution to <= 32 channels (csrc/conv3x3_stream.hip, cp_conv3x3_stream_*) through the
C ABI and through conv3x3.conv_infer's dispatch.

Two checkers, as in test_conv_stream.py.  The staged kernel (cp_conv_mfma_forward, taps = 9): the streaming kernel's
default form runs the same sequence of floating-point operations per output element, so the two results must be EQUAL
BIT FOR BIT.  And float64 torch convolution with that file's bar: one split-bf16 contraction (hi*hi + hi*lo + lo*hi, fp32
accumulate) at 2e-5 of the output's max-norm -- for every form.  The shapes are the smallest at which each mechanism of
the kernel can still go wrong."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from centerpoly_amd import _C, synth

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 2e-5
FORMS = [(nt, ks) for ks in (1, 2, 4) for nt in (1, 2, 4)]       # every instantiation of the kernel
CP_EUNSUPPORTED = -2


def P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _t(tag, shape, scale=1.0):
    return torch.from_numpy(synth.normal("conv3stream/" + tag, shape) * np.float32(scale)).to(DEV)


def _rel(a, ref):
    return (a.double() - ref).abs().max().item() / max(ref.abs().max().item(), 1e-30)


def _prepare(w):
    L = _C.lib()
    co, ci = w.shape[:2]
    wp = torch.empty(L.cp_conv_mfma_weight_bytes(ci, co, 9), dtype=torch.uint8, device=DEV)
    _C.check(L.cp_conv_mfma_prepare(P(w), ci, co, 9, 0, P(wp), _C.stream()), "prepare")
    return wp


def _stream(x, w, bias=None, form=(0, 0), wp=None):
    """One launch with the weight w [Cout][Cin][3][3]; `out` starts as NaN."""
    L = _C.lib()
    B, ci, H, W = x.shape
    co = w.shape[0]
    assert L.cp_conv3x3_stream_supported(ci, co, H, W)
    wp = _prepare(w) if wp is None else wp
    out = torch.full((B, co, H, W), float("nan"), device=DEV)
    _C.check(L.cp_conv3x3_stream_forward_form(P(x), P(wp), P(bias), None, P(out), B, ci, H, W, co, 0, form[0], form[1],
                                              _C.stream()), "forward")
    return out


def _staged(x, w, bias=None, wp=None):
    L = _C.lib()
    B, ci, H, W = x.shape
    co = w.shape[0]
    wp = _prepare(w) if wp is None else wp
    out = torch.full((B, co, H, W), float("nan"), device=DEV)
    ptrs, chans = (ctypes.c_void_p * 1)(x.data_ptr()), (ctypes.c_int32 * 1)(ci)
    _C.check(L.cp_conv_mfma_forward(ptrs, chans, 1, P(wp), P(bias), None, P(out), B, H, W, co, 9, 0, _C.stream()),
             "cp_conv_mfma_forward")
    return out


def _staged_ks(ci, co, H, W, B):
    """The K split of conv_mfma.hip's conv_dispatch for a 3x3 / stride 1 float32 launch to <= 32 channels, restated."""
    nchunk, tiles_x = (ci + 31) // 32, (W + 31) // 32
    wgs = lambda mt, th: tiles_x * ((H + th - 1) // th) * B * ((co + 16 * mt - 1) // (16 * mt))
    if wgs(2, 16) >= 448 or wgs(2, 8) >= 320:
        return 1
    if wgs(2, 4) < 384 and nchunk >= 8:
        return 4
    if wgs(2, 4) < 768 and nchunk >= 4:
        return 2
    return 1


# (B, Cin, Cout, H, W) -> the K split the staged kernel picks: 2 chunks / none, 4 / two groups, 8 / four groups, 5 = 3 + 2,
# 9 = 3 + 2 + 2 + 2 (odd counts per wave against the prefetch depth), a half-empty last chunk; then K splits on widths
# that put the row form's halo between wave tiles and a ragged last wave tile under the bitwise comparison
KSPLIT = [((1, 64, 27, 8, 32), 1), ((1, 128, 27, 8, 32), 2), ((1, 256, 27, 8, 32), 4), ((1, 160, 27, 8, 32), 2),
          ((1, 288, 27, 8, 32), 4), ((1, 48, 27, 8, 32), 1),
          ((1, 128, 27, 4, 132), 2), ((1, 256, 27, 3, 68), 4)]     # the row form (nt = 4) over three and two wave tiles of a row


@pytest.mark.parametrize("shape,ks", KSPLIT, ids=["x".join(map(str, s)) for s, _ in KSPLIT])
def test_k_splits_have_the_staged_kernels_bits(shape, ks):
    B, ci, co, H, W = shape
    L = _C.lib()
    assert _staged_ks(ci, co, H, W, B) == ks
    assert L.cp_conv3x3_stream_form(ci, co, H, W, B) & 255 == ks
    x, w, bias = _t("kx%s" % (shape,), (B, ci, H, W)), _t("kw%s" % (shape,), (co, ci, 3, 3), 0.05), _t("kb", (co,))
    wp = _prepare(w)                                          # one prepared buffer serves both kernels
    old = _staged(x, w, bias, wp)
    assert torch.isfinite(old).all()
    new = _stream(x, w, bias, wp=wp)
    assert torch.isfinite(new).all() and torch.equal(new, old)
    assert torch.equal(_stream(x, w, None, wp=wp), _staged(x, w, None, wp))
    ref = F.conv2d(x.double(), w.double(), bias.double(), padding=1)
    for form in FORMS:
        out = _stream(x, w, bias, form, wp)
        assert torch.isfinite(out).all() and _rel(out, ref) <= TOL, form
        if form[1] == ks:                                     # the bits depend on the K split, not on the tile form
            assert torch.equal(out, old), form


# (B, Cin, Cout, H, W): widths off the 16-pixel grid and one pixel into a new tile, heights 1-9, Cout 1, 18, 27, 32, a batch;
# then widths that are multiples of 4 (the row form of nt = 4: wave tiles of 64 pixels) off the 64-pixel grid: one lane
# and nine lanes of a wave tile inside the row, four pixels into a second and a third wave tile
RAGGED = [(2, 32, 27, 5, 37), (1, 32, 27, 1, 1), (1, 64, 18, 3, 33), (1, 32, 32, 9, 70), (1, 32, 1, 4, 16), (1, 32, 27, 2, 15),
          (2, 32, 27, 5, 36), (1, 32, 27, 1, 4), (1, 64, 18, 3, 68), (1, 32, 32, 9, 132)]


@pytest.mark.parametrize("shape", RAGGED, ids=["x".join(map(str, s)) for s in RAGGED])
def test_ragged_maps_and_halo_match_float64(shape):
    B, ci, co, H, W = shape
    x, w, bias = _t("rx%s" % (shape,), (B, ci, H, W)), _t("rw%s" % (shape,), (co, ci, 3, 3), 0.05), _t("rb%s" % (shape,), (co,))
    wp = _prepare(w)
    ref = F.conv2d(x.double(), w.double(), bias.double(), padding=1)
    for form in [(0, 0)] + FORMS:
        out = _stream(x, w, bias, form, wp)
        assert torch.isfinite(out).all(), form              # every output element was written
        assert _rel(out, ref) <= TOL, form
    assert torch.equal(_stream(x, w, bias, wp=wp), _staged(x, w, bias, wp))


@pytest.mark.parametrize("W", [37, 36, 64, 68])
@pytest.mark.parametrize("col", ["last", "first"])
def test_a_row_end_does_not_wrap_into_the_next_row(col, W):
    """In the flat plane the right neighbour of a row's last pixel is the next row's first one (and the other way
    round): with an input that is zero except one edge column and a zero bias, every output column further than one
    pixel from that edge is exactly 0 -- a wrapped tap would put the edge column's values at the opposite edge."""
    B, ci, co, H = 2, 32, 27, 5
    x = torch.zeros(B, ci, H, W, device=DEV)
    edge = _t("wrap%s%d" % (col, W), (B, ci, H))
    w = _t("wrapw", (co, ci, 3, 3), 0.05)
    wp = _prepare(w)
    if col == "last":
        x[..., W - 1] = edge
    else:
        x[..., 0] = edge
    ref = F.conv2d(x.double(), w.double(), None, padding=1)
    for form in [(0, 0)] + FORMS:
        out = _stream(x, w, None, form, wp)
        assert torch.isfinite(out).all() and _rel(out, ref) <= TOL, form
        quiet, loud = (out[..., :W - 2], out[..., W - 2:]) if col == "last" else (out[..., 2:], out[..., :2])
        assert (quiet == 0).all(), form
        assert (loud != 0).any(), form


def test_refusals_launch_nothing():
    L = _C.lib()
    assert L.cp_conv3x3_stream_supported(64, 27, 8, 32) and L.cp_conv3x3_stream_supported(64, 32, 8, 32)
    assert not L.cp_conv3x3_stream_supported(64, 33, 8, 32)                  # three weight tiles
    assert not L.cp_conv3x3_stream_supported(64, 27, 40000, 40000)           # beyond 32-bit offsets
    x, res = _t("ux", (1, 64, 8, 32)), _t("ur", (1, 27, 8, 32))
    w33, w27 = _t("uw33", (33, 64, 3, 3), 0.05), _t("uw27", (27, 64, 3, 3), 0.05)
    out = torch.full((1, 33, 8, 32), float("nan"), device=DEV)
    st = _C.stream()
    assert L.cp_conv3x3_stream_forward(P(x), P(_prepare(w33)), None, None, P(out), 1, 64, 8, 32, 33, 0, st) == CP_EUNSUPPORTED
    wp = _prepare(w27)
    assert L.cp_conv3x3_stream_forward(P(x), P(wp), None, P(res), P(out), 1, 64, 8, 32, 27, 0, st) == CP_EUNSUPPORTED
    assert L.cp_conv3x3_stream_forward(P(x), P(wp), None, None, P(out), 1, 64, 8, 32, 27, 1, st) == CP_EUNSUPPORTED
    assert L.cp_conv3x3_stream_forward(P(x), P(wp), None, None, P(out), 1, 64, 40000, 40000, 27, 0, st) == CP_EUNSUPPORTED
    assert L.cp_conv3x3_stream_forward_form(P(x), P(wp), None, None, P(out), 1, 64, 8, 32, 27, 0, 3, 1, st) == -1
    assert L.cp_conv3x3_stream_forward(None, None, None, None, None, 1, 64, 8, 32, 27, 0, st) == -1
    torch.cuda.synchronize()
    assert torch.isnan(out).all()                             # nothing was launched


def test_an_image_gives_the_same_bits_alone_and_in_a_batch():
    x, w, bias = _t("bx", (3, 64, 7, 45)), _t("bw", (27, 64, 3, 3), 0.05), _t("bb", (27,))
    wp = _prepare(w)
    out = _stream(x, w, bias, wp=wp)
    for i in range(3):
        assert torch.equal(out[i:i + 1], _stream(x[i:i + 1].contiguous(), w, bias, wp=wp)), i
    L = _C.lib()
    assert L.cp_conv3x3_stream_form(64, 27, 7, 45, 1) >> 8 == L.cp_conv3x3_stream_form(64, 27, 7, 45, 3) >> 8


# ---- module level: conv3x3.conv_infer's dispatch -------------------------------------------------------------------------
class _Streamed(object):
    """Counts the launches conv_infer sends through the streaming kernel while it is active."""

    def __enter__(self):
        from centerpoly_amd.models.networks import conv3x3
        self.n, self.inner = 0, conv3x3._stream3_infer

        def counted(*args):
            out = self.inner(*args)
            self.n += out is not None
            return out
        conv3x3._stream3_infer = counted
        return self

    def __exit__(self, *exc):
        from centerpoly_amd.models.networks import conv3x3
        conv3x3._stream3_infer = self.inner


def _deform_conv():
    """DeformConv(256, 64) as prepare_inference leaves it, with live offsets, its DCN on the K-split region kernel."""
    from centerpoly_amd.models.networks.pose_dla_dcn import DeformConv
    torch.manual_seed(11)
    m = DeformConv(256, 64)
    with torch.no_grad():
        bn = m.actf[0]
        bn.running_mean.normal_(0, 0.05)
        bn.running_var.uniform_(0.7, 1.3)
        bn.weight.uniform_(0.8, 1.2)
        bn.bias.normal_(0, 0.1)
        m.conv.conv_offset_mask.weight.normal_(0, 0.02)
        m.conv.conv_offset_mask.bias.normal_(0, 0.2)
        m.conv.bias.normal_(0, 0.1)
    m = m.to(DEV).eval()
    m.fold()
    m.conv.contraction = "bf16x3_region"
    return m


def test_deform_conv_module_forced_against_off():
    """1 x 256 x 16 x 128 is the smallest map at which conv3x3._fills still sends the offset convolution to the MFMA kernel
    (16 workgroups, Cin >= 256): the module's output, and its K-split slices reduced, have the same bits with the offset
    convolution streamed ("force") and staged ("off")."""
    from centerpoly_amd.models.networks import conv3x3
    m = _deform_conv()
    x = _t("dcn", (1, 256, 16, 128))
    L = _C.lib()

    def reduced():
        ws, off, nsl, scale, shift = m.forward_slices(x)
        assert nsl > 1
        out = torch.full((1, 64, 16, 128), float("nan"), device=DEV)
        _C.check(L.cp_dcn_splitk_reduce(ctypes.c_void_p(ws.data_ptr() + off), nsl, P(scale), P(shift), 1, P(out), 1, 64,
                                        16 * 128, _C.stream()), "cp_dcn_splitk_reduce")
        return out

    assert conv3x3.STREAM_3X3 == "auto"
    try:
        with torch.no_grad(), _Streamed() as s:
            conv3x3.STREAM_3X3 = "force"
            a, ra = m(x), reduced()
            assert s.n == 2                                   # both forced calls streamed their offset convolution
            conv3x3.STREAM_3X3 = "off"
            b, rb = m(x), reduced()
            assert s.n == 2                                   # ... and the others did not
    finally:
        conv3x3.STREAM_3X3 = "auto"
    assert torch.isfinite(a).all() and torch.isfinite(ra).all()
    assert torch.equal(a, b) and torch.equal(ra, rb)

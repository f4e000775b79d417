"""GPU parity of the streaming 1x1 convolution (csrc/conv_stream.hip, cp_conv1x1_stream_*) through the C ABI and through
conv3x3.conv_infer's dispatch.

Two checkers.  The staged kernel (cp_conv_mfma_forward, taps = 1): the streaming kernel's default form runs the same
sequence of floating-point operations per output element, so the two results must be EQUAL BIT FOR BIT wherever both take
the shape.  And float64 torch convolution, as in test_conv_mfma.py, with the same bar: one split-bf16 contraction
(hi*hi + hi*lo + lo*hi, fp32 accumulate) at 2e-5 of the output's max-norm -- for every form and the shapes only the
streaming kernel takes.  The shapes are the smallest at which each mechanism of the kernel can still go wrong."""
import ctypes
import itertools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from centerpoly_amd import _C, synth

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 2e-5
FORMS = [(nb, ks) for ks in (1, 2, 4) for nb in (2, 1)]          # every instantiation of the kernel


def P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _t(tag, shape, scale=1.0):
    return torch.from_numpy(synth.normal("convstream/" + tag, shape) * np.float32(scale)).to(DEV)


def _rel(a, ref):
    return (a.double() - ref).abs().max().item() / max(ref.abs().max().item(), 1e-30)


def _stream(xs, w, bias=None, residual=None, relu=False, form=(0, 0)):
    """One launch over the sources `xs` with the weight w [Cout][Cin][1][1]; `out` starts as NaN."""
    L = _C.lib()
    B, _, H, W = xs[0].shape
    cs = [x.shape[1] for x in xs]
    cin, cout, n = sum(cs), w.shape[0], len(xs)
    chans = (ctypes.c_int32 * n)(*cs)
    assert L.cp_conv1x1_stream_supported(chans, n, cout, H, W)
    wp = torch.empty(L.cp_conv1x1_stream_weight_bytes(cin, cout), dtype=torch.uint8, device=DEV)
    _C.check(L.cp_conv1x1_stream_prepare(P(w), cin, cout, P(wp), _C.stream()), "prepare")
    out = torch.full((B, cout, H, W), float("nan"), device=DEV)
    ptrs = (ctypes.c_void_p * n)(*[x.data_ptr() for x in xs])
    _C.check(L.cp_conv1x1_stream_forward_form(ptrs, chans, n, P(wp), P(bias), P(residual), P(out), B, H, W, cout,
                                              1 if relu else 0, form[0], form[1], _C.stream()), "forward")
    return out


# (B, Cin, Cout, H, W): widths off the 32- and 4-pixel grids, heights below any row tiling, Cout off the 32-channel tile,
# a single k-step
RAGGED = [(2, 32, 64, 5, 37), (1, 16, 27, 1, 1), (1, 48, 40, 3, 33), (1, 64, 128, 9, 70)]


@pytest.mark.parametrize("shape", RAGGED, ids=["x".join(map(str, s)) for s in RAGGED])
def test_ragged_maps_match_float64(shape):
    B, ci, co, H, W = shape
    x, w = _t("rx%s" % (shape,), (B, ci, H, W)), _t("rw%s" % (shape,), (co, ci, 1, 1), 0.05)
    ref = F.conv2d(x.double(), w.double())
    for form in [(0, 0)] + FORMS:
        out = _stream([x], w, form=form)
        assert torch.isfinite(out).all(), form              # every output element was written
        assert _rel(out, ref) <= TOL, form


SOURCES = [((64, 64), 64), ((32, 32, 16, 32), 48), ((128, 128, 64, 128), 128)]


@pytest.mark.parametrize("case", SOURCES, ids=[str(c[0]) for c in SOURCES])
def test_several_sources_equal_their_concatenation_bitwise(case):
    cs, co = case
    xs = [_t("sx%d%s" % (i, cs), (2, c, 6, 40)) for i, c in enumerate(cs)]
    w, bias = _t("sw%s" % (cs,), (co, sum(cs), 1, 1), 0.05), _t("sb%s" % (cs,), (co,))
    cat = torch.cat(xs, 1).contiguous()
    ref = F.conv2d(cat.double(), w.double(), bias.double())
    for form in [(0, 0)] + FORMS:
        out = _stream(xs, w, bias, form=form)
        assert torch.equal(out, _stream([cat], w, bias, form=form)), form     # same kernel, same order
        assert torch.isfinite(out).all() and _rel(out, ref) <= TOL, form


@pytest.mark.parametrize("cin", [112, 1280])
@pytest.mark.parametrize("form", FORMS, ids=["nb%d-ks%d" % f for f in FORMS])
def test_every_k_split_with_uneven_steps(cin, form):
    """4 and 40 chunks (the last of 112 channels half empty) over 1, 2 and 4 interleaved wave groups: 4 = 2 + 2 = 1 + 1 + 1 + 1,
    40 = 20 + 20 = 10 each; odd counts per wave against the prefetch depth of 2 at 112 / 2 groups... every form, twice."""
    x, w = _t("kx%d" % cin, (1, cin, 4, 32)), _t("kw%d" % cin, (96, cin, 1, 1), 0.05)
    bias, res = _t("kb", (96,)), _t("kr", (1, 96, 4, 32))
    ref = F.relu(F.conv2d(x.double(), w.double(), bias.double()) + res.double())
    out = _stream([x], w, bias, res, True, form)
    assert torch.isfinite(out).all() and _rel(out, ref) <= TOL
    assert torch.equal(out, _stream([x], w, bias, res, True, form))          # fixed order, no atomics


@pytest.mark.parametrize("use_bias,use_res,relu", list(itertools.product((False, True), repeat=3)))
def test_epilogue_combinations(use_bias, use_res, relu):
    x, w = _t("ex", (1, 64, 4, 36)), _t("ew", (64, 64, 1, 1), 0.05)
    bias = _t("eb", (64,)) if use_bias else None
    res = _t("er", (1, 64, 4, 36)) if use_res else None
    ref = F.conv2d(x.double(), w.double(), bias.double() if use_bias else None)
    if use_res:
        ref = ref + res.double()
    out = _stream([x], w, bias, res, relu)
    assert torch.isfinite(out).all() and _rel(out, F.relu(ref) if relu else ref) <= TOL
    if relu:
        assert (out >= 0).all()


def test_relu_on_exact_negatives_and_zeros():
    x, w = _t("nx", (1, 64, 4, 36)), _t("nw", (64, 64, 1, 1), 0.05)
    neg = -(_t("nb", (64,)).abs() + 1e3)                    # every pre-activation is negative by construction
    assert (_stream([x], w, neg, None, False) < 0).all()
    assert (_stream([x], w, neg, None, True) == 0).all()
    zero = torch.zeros_like(x)                              # every pre-activation is exactly zero
    assert (_stream([zero], w, None, None, True) == 0).all()
    assert (_stream([zero], w, None, None, False) == 0).all()


def test_an_image_gives_the_same_bits_alone_and_in_a_batch():
    xs = [_t("b0", (3, 64, 7, 45)), _t("b1", (3, 32, 7, 45))]
    w, bias, res = _t("bw", (80, 96, 1, 1), 0.05), _t("bb", (80,)), _t("br", (3, 80, 7, 45))
    out = _stream(xs, w, bias, res, True)
    for i in range(3):
        one = _stream([x[i:i + 1].contiguous() for x in xs], w, bias, res[i:i + 1].contiguous(), True)
        assert torch.equal(out[i:i + 1], one), i
    L = _C.lib()
    assert L.cp_conv1x1_stream_form(96, 80, 7, 45, 1) == L.cp_conv1x1_stream_form(96, 80, 7, 45, 3)


def test_scaling_by_a_power_of_two_is_exact():
    x, w = _t("px", (2, 64, 5, 37)), _t("pw", (64, 64, 1, 1), 0.05)
    a = _stream([x], w)
    assert torch.equal(_stream([2.0 * x], w), 2.0 * a)      # a power of two commutes with the bf16 split
    assert torch.equal(_stream([x], w), a)


# the cases both kernels take (sources that are multiples of 32, maps the staged kernel supports), at the batch sizes and
# shapes that make the staged kernel pick each of its K splits: none (large or shallow maps), 2 and 4 wave groups
# (256 + 256 -> 256 @64x128 and 512 + 512 + 256 -> 512 @32x64 at batch 1, the Roots of DLA-34 levels 4 and 5), a ragged
# last chunk (48 and 80 channels), Cout off the 16-channel tile, a plane that is no multiple of 4 (dword epilogue)
BOTH = [(2, (64,), 128, 24, 80), (2, (64, 64), 64, 40, 72), (2, (128, 128, 64), 128, 17, 33), (1, (256, 256), 256, 64, 128),
        (1, (512, 512, 256), 512, 32, 64), (1, (48,), 27, 9, 31), (3, (80,), 40, 16, 32), (1, (256, 256, 128, 256), 256, 64, 128)]


@pytest.mark.parametrize("case", BOTH, ids=["B%d %s->%d" % (c[0], c[1], c[2]) for c in BOTH])
def test_default_form_has_the_staged_kernels_bits(case):
    B, cs, co, H, W = case
    L = _C.lib()
    xs = [_t("ax%d%s" % (i, case), (B, c, H, W)) for i, c in enumerate(cs)]
    w, bias = _t("aw%s" % (case,), (co, sum(cs), 1, 1), 0.05), _t("ab%s" % (case,), (co,))
    res = _t("ar%s" % (case,), (B, co, H, W))
    wp = torch.empty(L.cp_conv_mfma_weight_bytes(sum(cs), co, 1), dtype=torch.uint8, device=DEV)
    _C.check(L.cp_conv_mfma_prepare(P(w), sum(cs), co, 1, 0, P(wp), _C.stream()), "prepare")
    ptrs = (ctypes.c_void_p * len(xs))(*[x.data_ptr() for x in xs])
    chans = (ctypes.c_int32 * len(xs))(*cs)
    for b_, r_, relu in ((bias, res, True), (None, None, False), (bias, None, True)):
        old = torch.full((B, co, H, W), float("nan"), device=DEV)
        _C.check(L.cp_conv_mfma_forward(ptrs, chans, len(xs), P(wp), P(b_), P(r_), P(old), B, H, W, co, 1, 1 if relu else 0,
                                        _C.stream()), "cp_conv_mfma_forward")
        assert torch.equal(_stream(xs, w, b_, r_, relu), old), (b_ is not None, r_ is not None, relu)


def test_unsupported_and_bad_arguments():
    L = _C.lib()
    one = lambda *cs: ((ctypes.c_int32 * len(cs))(*cs), len(cs))
    assert L.cp_conv1x1_stream_supported(*one(64, 48), 32, 8, 32)
    assert not L.cp_conv1x1_stream_supported(*one(40), 32, 8, 32)              # not a multiple of 16
    assert not L.cp_conv1x1_stream_supported(*one(64, 24), 32, 8, 32)
    assert not L.cp_conv1x1_stream_supported(*one(64), 64, 40000, 40000)       # beyond 32-bit offsets
    x, w = _t("ux", (1, 40, 8, 32)), _t("uw", (32, 40, 1, 1))
    wp, out = torch.empty(1 << 16, dtype=torch.uint8, device=DEV), torch.empty((1, 32, 8, 32), device=DEV)
    ptrs, (chans, n) = (ctypes.c_void_p * 1)(x.data_ptr()), one(40)
    assert L.cp_conv1x1_stream_forward(ptrs, chans, n, P(wp), None, None, P(out), 1, 8, 32, 32, 0, _C.stream()) == -2
    assert L.cp_conv1x1_stream_forward(None, None, 1, None, None, None, None, 1, 8, 32, 32, 0, _C.stream()) == -1


# ---- module level: conv3x3.conv_infer's dispatch -------------------------------------------------------------------------
def _randomize_bn(net):
    for m in net.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_mean.normal_(0, 0.2)
            m.running_var.uniform_(0.5, 1.5)
            m.weight.data.uniform_(0.5, 1.5)
            m.bias.data.normal_(0, 0.2)


def _fold_all(net):
    net.eval()
    for m in net.modules():
        if hasattr(m, "fold"):
            m.fold()


def _routes(fn):
    """fn() under STREAM_1X1 = "force" and "off"; the switch is left at "auto"."""
    from centerpoly_amd.models.networks import conv3x3
    try:
        with torch.no_grad():
            conv3x3.STREAM_1X1 = "force"
            a = fn()
            conv3x3.STREAM_1X1 = "off"
            b = fn()
    finally:
        conv3x3.STREAM_1X1 = "auto"
    return a, b


class _Streamed(object):
    """Counts the launches conv_infer sends through the streaming kernel while it is active."""

    def __enter__(self):
        from centerpoly_amd.models.networks import conv3x3
        self.n, self.inner = 0, conv3x3._stream_infer

        def counted(*args):
            out = self.inner(*args)
            self.n += out is not None
            return out
        conv3x3._stream_infer = counted
        return self

    def __exit__(self, *exc):
        from centerpoly_amd.models.networks import conv3x3
        conv3x3._stream_infer = self.inner


def test_root_module_forced_against_off():
    from centerpoly_amd.models.networks import pose_dla_dcn
    torch.manual_seed(5)
    root = pose_dla_dcn.Root(128, 64, 1, True).to(DEV)
    _randomize_bn(root)
    _fold_all(root)
    xs = [_t("root%d" % i, (1, 64, 16, 32)) for i in range(2)]
    with _Streamed() as s:
        a, b = _routes(lambda: root(*xs))
    assert s.n == 1                                           # the forced route ran, the other did not
    assert (a - b).abs().max().item() <= 2 * TOL * b.abs().max().item()
    w, bias = root._folded
    ref = F.relu(F.conv2d(torch.cat(xs, 1).double(), w.double(), bias.double()) + xs[0].double())
    assert _rel(a, ref) <= TOL


@pytest.mark.parametrize("levels,cin,cout,nstream", [(1, 32, 64, 2), (2, 64, 128, 3)], ids=["levels1-project", "levels2-four-sources"])
def test_tree_module_forced_against_off(levels, cin, cout, nstream):
    """levels = 1: `project` (32 -> 64) and a two-source Root; levels = 2: the inner Root and the outer one over four
    sources (128 + 128 + 64 + 128), the live projection of the inner tree."""
    from centerpoly_amd.models.networks import pose_dla_dcn
    torch.manual_seed(6)
    tree = pose_dla_dcn.Tree(levels, pose_dla_dcn.BasicBlock, cin, cout, stride=2, level_root=levels > 1).to(DEV)
    _randomize_bn(tree)
    _fold_all(tree)
    x = _t("tree%d" % levels, (1, cin, 32, 64))
    with _Streamed() as s:
        a, b = _routes(lambda: tree(x))
    assert tuple(a.shape) == (1, cout, 16, 32)
    assert s.n == nstream
    assert (a - b).abs().max().item() <= 2 * TOL * b.abs().max().item()


def test_default_route_streams_a_level_3_root_with_the_staged_kernels_bits():
    """A level-3 Root of DLA-34 at its inference size (128 + 128 -> 128 @128x256): "auto" sends it through the streaming
    kernel, and the module's output has the bits of the staged route ("off")."""
    from centerpoly_amd.models.networks import conv3x3, pose_dla_dcn
    torch.manual_seed(8)
    root = pose_dla_dcn.Root(256, 128, 1, True).to(DEV)
    _randomize_bn(root)
    _fold_all(root)
    xs = [_t("level3root%d" % i, (1, 128, 128, 256)) for i in range(2)]
    try:
        with torch.no_grad(), _Streamed() as s:
            assert conv3x3.STREAM_1X1 == "auto"
            auto = root(*xs)
            assert s.n == 1
            conv3x3.STREAM_1X1 = "off"
            off = root(*xs)
            assert s.n == 1
    finally:
        conv3x3.STREAM_1X1 = "auto"
    assert torch.equal(auto, off)


def test_prepared_stream_weights_follow_a_replaced_folded_weight():
    from centerpoly_amd.models.networks import conv3x3, pose_dla_dcn
    from centerpoly_amd.models.networks.prepared import ATTR
    torch.manual_seed(7)
    root = pose_dla_dcn.Root(128, 64, 1, False).to(DEV)
    _randomize_bn(root)
    _fold_all(root)
    xs = [_t("prep%d" % i, (1, 64, 16, 32)) for i in range(2)]
    form = lambda: root.conv.__dict__[ATTR]["conv"][2]
    try:
        conv3x3.STREAM_1X1 = "force"
        with torch.no_grad():
            root(*xs)
            first = form()
            root(*xs)
            assert form() is first                           # served, not rebuilt
            new = _t("prepw", tuple(root._folded[0].shape), 0.05)
            root._folded = (new, root._folded[1])
            out = root(*xs)
        assert form() is not first
        ref = F.relu(F.conv2d(torch.cat(xs, 1).double(), new.double(), root._folded[1].double()))
        assert _rel(out, ref) <= TOL
    finally:
        conv3x3.STREAM_1X1 = "auto"

"""Helpers of tests/test_nonfinite.py: the cases (inputs from fixed synth streams with NaN, +Inf and -Inf planted at
fixed positions) and their references in plain CPU torch.  TEST INFRASTRUCTURE, CPU only (the device side lives in the
test file).

Every case carries
    ref32   the operation in float32 on the planted input: WHERE the output is non-finite, and of which class;
    ref64   the operation in float64 on the input before planting: the finite values.  An output element whose
            receptive field holds no planted value is the same function of the same numbers in both;
    taint   True where the receptive field holds a planted value (the planted indicator pushed through the
            operation's geometry); a superset of ref32's non-finite set (a ReLU may turn -Inf into 0 inside it).
The planted positions sit in the bottom-right corner of image 0: (H-2, W-2) is interior, (H-1, W-2) is on the last row,
(H-1, W-1) is the last element of the plane -- the tail of every 4-, 16- and 32-pixel tiling of a ragged map."""
import functools
import types

import numpy as np
import torch
import torch.nn.functional as F

from centerpoly_amd import synth
from oracle import dcn as odcn
from oracle import losses as olos

T = torch.from_numpy
NAN, INF = float("nan"), float("inf")
VALUES = (NAN, INF, -INF)
CASES = {}                                             # name -> builder (cached)


def case(name):
    def deco(fn):
        assert name not in CASES
        CASES[name] = functools.lru_cache(maxsize=None)(fn)
        return fn
    return deco


def get(name):
    return CASES[name]()


def positions(H, W):
    return [(max(H - 2, 0), max(W - 2, 0)), (H - 1, max(W - 2, 0)), (H - 1, W - 1)]


def plant(x, chans=None, at=None):
    """-> (planted copy, indicator [B,C,H,W]): NaN, +Inf, -Inf at positions() of image 0 (or at `at`), in the channels
    `chans`."""
    B, C, H, W = x.shape
    chans = chans if chans is not None else (0, C - 1, C // 2)
    xp, ind = x.copy(), np.zeros(x.shape, np.float32)
    for (y, xx), c, v in zip(at or positions(H, W), chans, VALUES):
        xp[0, c, y, xx] = v
        ind[0, c, y, xx] = 1.0
    return xp, ind


def pixels(ind):
    """[B,C,H,W] indicator -> [B,1,H,W]: the pixels that hold a planted value in any channel."""
    return T(ind).amax(1, keepdim=True)


def spread(pix, k, stride=1):
    """The output pixels of a k x k / stride / pad k // 2 convolution whose window holds a marked input pixel."""
    return F.max_pool2d(pix, k, stride, k // 2) if k > 1 else pix


def over(pix, channels):
    return (pix > 0).expand(-1, channels, -1, -1).clone()


def finite_fraction(t):
    return float(torch.isfinite(t).float().mean())


def _n(stream, shape, scale=1.0, mean=0.0):
    return (synth.normal(stream, shape) * np.float32(scale) + np.float32(mean)).astype(np.float32)


def _conv(x, w, b, k, stride=1):
    return F.conv2d(x, w, b, stride=stride, padding=k // 2)


def _d(a):
    return None if a is None else T(a).double()


def _f(a):
    return None if a is None else T(a)


# ------------------------------------------------------------------------------------------- training BatchNorm -----
BN_SHAPES = [(1, 8, 3, 5), (2, 16, 12, 20)]                          # scalar path (H*W % 4 != 0); float4 path
BN_CHANNEL = 1


def _bn_run(x, res, p, relu, dtype):
    """torch.nn.BatchNorm2d (train) + residual + ReLU -> y, running_mean, running_var, batch mean, batch invstd."""
    C = x.shape[1]
    bn = torch.nn.BatchNorm2d(C, momentum=0.1).to(dtype).train()
    with torch.no_grad():
        bn.weight.copy_(T(p["w"])), bn.bias.copy_(T(p["b"]))
        bn.running_mean.copy_(T(p["rm"])), bn.running_var.copy_(T(p["rv"]))
        xt = T(x).to(dtype)
        y = bn(xt)
        if res is not None:
            y = y + T(res).to(dtype)
        if relu:
            y = torch.relu(y)
        mean = xt.mean((0, 2, 3))
        var = ((xt - mean.view(1, -1, 1, 1)) ** 2).mean((0, 2, 3))
    return y, bn.running_mean.clone(), bn.running_var.clone(), mean, torch.rsqrt(var + bn.eps)


def _bn_case(shape, relu, with_res):
    C = shape[1]
    x = synth.normal("bn/x%d" % C, shape, 0.3, 1.7)
    res = synth.normal("bn/r%d" % C, shape) if with_res else None
    p = dict(w=synth.uniform("bn/w%d" % C, (C,), 0.5, 1.5), b=synth.normal("bn/b%d" % C, (C,)),
             rm=synth.normal("bn/rm%d" % C, (C,)), rv=synth.uniform("bn/rv%d" % C, (C,), 0.5, 2.0))
    xp, ind = plant(x, (BN_CHANNEL,) * 3)
    r32, r64 = _bn_run(xp, res, p, relu, torch.float32), _bn_run(x, res, p, relu, torch.float64)
    taint = torch.zeros(shape, dtype=torch.bool)
    taint[:, BN_CHANNEL] = True                        # the statistics are the channel's: every image of it
    return types.SimpleNamespace(x=xp, res=res, p=p, relu=relu, ref32=r32[0], ref64=r64[0], taint=taint,
                                 stats32=r32[1:], stats64=r64[1:])


for _s in BN_SHAPES:
    for _relu in (True, False):
        for _res in (True, False):
            case("bn %s relu=%d res=%d" % ("x".join(map(str, _s)), _relu, _res))(
                functools.partial(_bn_case, _s, _relu, _res))


# ----------------------------------------------------------------------------- cp_bias_act_inplace (folded conv) -----
# the shapes of test_folded_conv_epilogue_matches_bn_relu and test_conv_bias_relu_training_epilogue_vs_torch, and a plane
# of 15 elements: the kernel's scalar tail
BIAS_ACT = [((2, 16, 12, 20), True, False, False), ((2, 16, 12, 20), True, True, True), ((2, 20, 10, 16), True, False, True),
            ((2, 5, 3, 5), True, True, True)]


def _bias_act_case(shape, with_bias, with_res, relu):
    tag = "x".join(map(str, shape))
    y = _n("nonfinite/ba/y" + tag, shape)
    bias = _n("nonfinite/ba/b" + tag, (shape[1],)) if with_bias else None
    res = _n("nonfinite/ba/r" + tag, shape) if with_res else None
    yp, ind = plant(y)

    def run(yy, dt):
        o = T(yy).to(dt)
        if res is not None:
            o = o + T(res).to(dt)
        if bias is not None:
            o = o + T(bias).to(dt).view(1, -1, 1, 1)
        return torch.relu(o) if relu else o
    return types.SimpleNamespace(y=yp, bias=bias, res=res, relu=relu, ref32=run(yp, torch.float32),
                                 ref64=run(y, torch.float64), taint=T(ind) > 0)


for _c in BIAS_ACT:
    case("bias_act %s bias=%d res=%d relu=%d" % (("x".join(map(str, _c[0])),) + tuple(map(int, _c[1:]))))(
        functools.partial(_bias_act_case, *_c))


# ------------------------------------------------------------------------------------------ direct convolution -----
DIRECT = [(3, 16, 7, 1, (2, 9, 70)), (16, 16, 3, 1, (2, 11, 50)), (16, 32, 3, 2, (2, 13, 70))]


def _direct_case(cin, cout, k, stride, shape):
    B, H, W = shape
    x = synth.normal("dconv/x%d%d" % (cin, H), (B, cin, H, W))
    w = synth.normal("dconv/w%d%d%d" % (cin, cout, k), (cout, cin, k, k), 0.0, 1.0 / np.sqrt(cin * k * k))
    b = synth.normal("dconv/b%d" % cout, (cout,), 0.0, 0.3)
    xp, ind = plant(x)
    ref32 = torch.relu(_conv(T(xp), T(w), T(b), k, stride))
    ref64 = torch.relu(_conv(_d(x), _d(w), _d(b), k, stride))
    return types.SimpleNamespace(x=xp, w=w, b=b, cfg=(cin, cout, k, stride, k // 2), ref32=ref32, ref64=ref64,
                                 taint=over(spread(pixels(ind), k, stride), cout))


for _c in DIRECT:
    case("direct %d->%d k%d s%d %s" % (_c[:4] + ("x".join(map(str, _c[4])),)))(functools.partial(_direct_case, *_c))


# -------------------------------------------------------------------------- the DLA base: stem, pair and trio -----
BASE_SHAPES = [(1, 5, 8), (2, 37, 100)]


def base_weights():
    t = lambda tag, shape, scale: _n("convmfma/" + tag, shape, scale)
    return dict(ws=t("triows", (16, 3, 7, 7), 0.1), bs=t("triobs", (16,), 0.2), w0=t("pairw0", (16, 16, 3, 3), 0.1),
                b0=t("pairb0", (16,), 0.2), w1=t("pairw1", (32, 16, 3, 3), 0.1), b1=t("pairb1", (32,), 0.2))


def _base_case(kind, shape):
    B, H, W = shape
    p = base_weights()
    x = _n("nonfinite/base/%s%s" % (kind, shape), (B, 16 if kind == "pair" else 3, H, W))
    # 5 x 8: a 7x7 window around each of three pixels would cover the map; all three values share the corner pixel, in
    # three channels
    xp, ind = plant(x, at=[(H - 1, W - 1)] * 3 if H * W < 64 else None)

    def run(xx, cv):
        s = xx
        if kind != "pair":
            s = torch.relu(_conv(s, cv(p["ws"]), cv(p["bs"]), 7))
        if kind != "stem":
            s = torch.relu(_conv(torch.relu(_conv(s, cv(p["w0"]), cv(p["b0"]), 3)), cv(p["w1"]), cv(p["b1"]), 3, 2))
        return s
    pix = pixels(ind)
    if kind != "pair":
        pix = spread(pix, 7)
    if kind != "stem":
        pix = spread(spread(pix, 3), 3, 2)
    return types.SimpleNamespace(x=xp, p=p, ref32=run(T(xp), _f), ref64=run(_d(x), _d),
                                 taint=over(pix, 16 if kind == "stem" else 32))


for _k in ("stem", "pair", "trio"):
    for _s in BASE_SHAPES:
        case("base %s %s" % (_k, "x".join(map(str, _s))))(functools.partial(_base_case, _k, _s))

# The one case whose reference cannot stay half finite: the trio's 3 x 4 output of the 5 x 8 image.  Through 7x7, 3x3 and
# 3x3 / stride 2 an output column sees image columns 2 ox - 5 .. 2 ox + 5 and every row, so a value planted anywhere
# leaves at most one of the four columns clean.  Its clean quarter (column 0) is still compared.
SMALL_RECEPTIVE_EXCEPTIONS = {"base trio 1x5x8": 0.25}


# ------------------------------------------------------------- split-bf16 convolutions (conv_mfma, the streams) -----
def _conv_case(stream, shape, k, with_bias, with_res, relu, wscale=0.05):
    B, ci, co, H, W = shape
    t = lambda tag, sh, scale=1.0: _n("%s/nf%s%s" % (stream, tag, shape), sh, scale)
    x, w = t("x", (B, ci, H, W)), t("w", (co, ci, k, k), wscale)
    bias = t("b", (co,)) if with_bias else None
    res = t("r", (B, co, H, W)) if with_res else None
    xp, ind = plant(x)

    def run(xx, cv):
        o = _conv(xx, cv(w), cv(bias), k)
        if res is not None:
            o = o + cv(res)
        return torch.relu(o) if relu else o
    return types.SimpleNamespace(x=xp, w=w, bias=bias, res=res, relu=relu, ref32=run(T(xp), _f), ref64=run(_d(x), _d),
                                 taint=over(spread(pixels(ind), k), co))


MFMA_SHAPES = [(3, 32, 80, 9, 31), (1, 48, 16, 5, 7)]
for _s in MFMA_SHAPES:
    case("conv_mfma %s" % "x".join(map(str, _s)))(functools.partial(_conv_case, "convmfma", _s, 3, True, True, True))
STREAM1 = (2, 32, 64, 5, 37)
case("stream1x1 2x32x64x5x37")(functools.partial(_conv_case, "convstream", STREAM1, 1, True, True, True))
STREAM3 = (2, 32, 27, 5, 37)
case("stream3x3 2x32x27x5x37")(functools.partial(_conv_case, "conv3stream", STREAM3, 3, True, False, False))


# ----------------------------------------------------------------------------------- the heads' output stage -----
HEAD_STAGE = [(256, 2, (16, 20)), (5, 3, (2, 2))]
HEAD_C0 = 4                                            # the stage reads a channel slice of a wider tensor


def _head_stage_case(cin, cout, hw):
    H, W = hw
    ytot = synth.normal("head/y%d_%d" % (cin, cout), (2, cin + 7, H, W))
    b3 = synth.normal("head/b3", (cin + 7,))
    w1 = synth.normal("head/w1%d_%d" % (cin, cout), (cout, cin), 0.0, 0.1)
    b1 = synth.normal("head/b1", (cout,))
    c0 = HEAD_C0
    yp, ind = plant(ytot, (c0, c0 + cin - 1, c0 + cin // 2))

    def run(yy, cv):
        x = torch.relu(yy[:, c0:c0 + cin] + cv(b3)[c0:c0 + cin].view(1, -1, 1, 1))
        return F.conv2d(x, cv(w1).view(cout, cin, 1, 1), cv(b1))
    return types.SimpleNamespace(ytot=yp, b3=b3, w1=w1, b1=b1, cfg=(cin, cout, H, W), ref32=run(T(yp), _f),
                                 ref64=run(_d(ytot), _d), taint=over(pixels(ind), cout))


for _c in HEAD_STAGE:
    case("head stage %d->%d %dx%d" % (_c[0], _c[1], _c[2][0], _c[2][1]))(functools.partial(_head_stage_case, *_c))


# ------------------------------------------------------------------------------------------------ fused heads -----
FUSED_HEADS = [((128,), 64, 32, 8, 32), ((8, 66, 1, 2), 64, 32, 9, 31)]      # the two smallest of WIDE_HEADS


def _fused_heads_case(couts, hc, cin, H, W):
    cfg = (couts, hc, cin, H, W)
    t = lambda tag, sh, scale=1.0: _n("widehf/%s%s" % (tag, cfg), sh, scale)
    nh = len(couts)
    x, w1, b1 = t("x", (2, cin, H, W)), t("w1", (nh * hc, cin, 3, 3), 0.05), t("b1", (nh * hc,))
    w2 = [t("w2_%d" % i, (co, hc), 0.1) for i, co in enumerate(couts)]
    b2 = [t("b2_%d" % i, (co,)) for i, co in enumerate(couts)]
    xp, ind = plant(x)

    def run(xx, cv):
        hid = torch.relu(_conv(xx, cv(w1), cv(b1), 3))
        return torch.cat([F.conv2d(hid[:, i * hc:(i + 1) * hc], cv(w2[i]).view(co, hc, 1, 1), cv(b2[i]))
                          for i, co in enumerate(couts)], 1)
    return types.SimpleNamespace(x=xp, w1=w1, b1=b1, w2=w2, b2=b2, cfg=cfg, ref32=run(T(xp), _f), ref64=run(_d(x), _d),
                                 taint=over(spread(pixels(ind), 3), sum(couts)))


for _c in FUSED_HEADS:
    case("fused heads %s hc%d %d %dx%d" % _c)(functools.partial(_fused_heads_case, *_c))


# ---------------------------------------------------------------------------------------------------------- DCN -----
# the gather kernels take any channel count; the region kernel needs Cin % 16 == 0: REGION_SHAPES' (2, 32, 40, 13, 19)
DCN_SHAPES = [(2, 24, 40, 13, 19), (2, 9, 33, 5, 3), (2, 32, 40, 13, 19)]


def _dcn_case(shape, origin=False):
    """relu(dcn(x) * scale + shift) with the non-finite values in x only, in the bottom-right corner or (`origin`) at
    pixels (0, 0), (0, 1) and (1, 1).  `taint`: the outputs that sample a planted pixel with a weight above 0 (the
    oracle on the indicator, |weights|).  `reach`: the most the kernels may add, see DESIGN 'Non-finite values' -- the
    outputs that sample a pixel within one pixel of a planted one, and, where pixel (0, 0) or (0, 1) of the image is
    planted, every output of that image with a tap outside the image (such a tap loads those two with a weight of 0)."""
    B, Cin, Cout, H, W = shape
    tag = "%dx%d" % (Cin, Cout)
    x = synth.normal("dcn/%s/x" % tag, (B, Cin, H, W))
    om = synth.normal("dcn/%s/om" % tag, (B, 27, H, W), 0.0, 2.0)
    w = synth.normal("dcn/%s/w" % tag, (Cout, Cin, 3, 3), 0.0, 1.0 / np.sqrt(Cin * 9))
    sc = synth.uniform("nonfinite/dcn/%s/sc" % tag, (Cout,), 0.5, 1.5)
    sh = synth.normal("nonfinite/dcn/%s/sh" % tag, (Cout,), 0.0, 0.1)
    xp, ind = plant(x, at=[(0, 0), (0, 1), (1, 1)] if origin else None)
    o1, o2, m = torch.chunk(T(om), 3, dim=1)
    off, mask = torch.cat((o1, o2), 1), torch.sigmoid(m)

    def run(xx, cv):
        y = odcn.dcn_v2_forward(xx, off.to(xx.dtype), mask.to(xx.dtype), cv(w), None)
        return torch.relu(y * cv(sc).view(1, -1, 1, 1) + cv(sh).view(1, -1, 1, 1))

    def sampled(pix):
        return over(odcn.dcn_v2_forward(pix, off, mask, torch.ones(1, 1, 3, 3), None), Cout)
    pix = pixels(ind)
    ho = torch.arange(H, dtype=torch.float32).view(1, H, 1) - 1
    wo = torch.arange(W, dtype=torch.float32).view(1, 1, W) - 1
    outside = torch.zeros(B, H, W, dtype=torch.bool)       # an output with a tap that is not inside the image
    for k in range(9):
        py, px = ho + k // 3 + off[:, 2 * k], wo + k % 3 + off[:, 2 * k + 1]
        outside |= ~((py > -1) & (px > -1) & (py < H) & (px < W))
    dummy = outside & (pix[:, 0, 0, :2].amax(1) > 0).view(B, 1, 1)    # ... in an image whose pixel (0,0) or (0,1) is planted
    return types.SimpleNamespace(x=xp, om=om, w=w, sc=sc, sh=sh, ref32=run(T(xp), _f), ref64=run(_d(x), _d),
                                 taint=sampled(pix), reach=sampled(spread(pix, 3)) | over(dummy.unsqueeze(1).float(), Cout))


for _s in DCN_SHAPES:
    case("dcn %s" % "x".join(map(str, _s)))(functools.partial(_dcn_case, _s))
for _s in (DCN_SHAPES[0], DCN_SHAPES[2]):              # (5 x 3: every output of the image has a tap outside)
    case("dcn origin %s" % "x".join(map(str, _s)))(functools.partial(_dcn_case, _s, True))

REDUCE = (13, 2, 5, 3, 5)                              # 13 slices = one block of 8, one of 4, one single; a 15-element plane


@case("dcn splitk reduce 13x2x5x3x5")
def _reduce_case():
    n, B, C, H, W = REDUCE
    part = _n("nonfinite/reduce/p", (n, B, C, H, W))
    sc, sh = synth.uniform("nonfinite/reduce/sc", (C,), 0.5, 1.5), _n("nonfinite/reduce/sh", (C,), 0.1)
    pp = part.copy()
    p1, ind = plant(part[1])                           # slice 1 of 13
    pp[1] = p1

    def run(q, cv):
        s = q[0]
        for i in range(1, n):                          # slices added in order
            s = s + q[i]
        return torch.relu(s * cv(sc).view(1, -1, 1, 1) + cv(sh).view(1, -1, 1, 1))
    return types.SimpleNamespace(part=pp, sc=sc, sh=sh, ref32=run(T(pp), _f), ref64=run(_d(part), _d), taint=T(ind) > 0)


# ---------------------------------------------------------------------------------------- max pooling 2 x 2 -----
POOL_SHAPES = [(1, 3, 9, 7), (3, 5, 16, 30)]


def _pool_case(shape):
    """ReLU-like input (half zeros: ties) with a NaN in each of the four window slots, +Inf beside a NaN, -Inf alone
    in a window of zeros; all inside the pooled area (odd rows / columns are dropped), image 0."""
    B, C, H, W = shape
    x = np.maximum(synth.normal("pool/x%s" % (shape,), shape), 0).astype(np.float32)
    y0, x0 = 2 * (H // 2) - 4, 2 * (W // 2) - 4        # the last two windows of the pooled area, each way
    xp = x.copy()
    for c, (dy, dx) in enumerate([(0, 0), (0, 1), (1, 0)]):
        xp[0, c % C, y0 + dy, x0 + dx] = NAN           # slot (dy, dx) of window (y0 / 2, x0 / 2)
    xp[0, 0, y0 + 3, x0 + 3] = NAN                     # slot (1, 1) of the last window
    xp[0, 1 % C, y0 + 2, x0 + 2] = INF                 # +Inf first, NaN later in the same window
    xp[0, 1 % C, y0 + 3, x0 + 3] = NAN
    xp[0, 2 % C, y0 + 2, x0 + 1] = -INF
    go = synth.normal("pool/go%s" % (shape,), (B, C, H // 2, W // 2))
    xt = T(xp).requires_grad_(True)
    y = F.max_pool2d(xt, 2, 2)
    (gx,) = torch.autograd.grad(y, xt, T(go))
    return types.SimpleNamespace(x=xp, go=go, ref32=y.detach(), grad=gx, ref64=None, taint=~torch.isfinite(y.detach()))


for _s in POOL_SHAPES:
    case("maxpool %s" % "x".join(map(str, _s)))(functools.partial(_pool_case, _s))


# ------------------------------------------------------------------------------------------------ up-sampling -----
@case("upsample2x_add 1x3x7x9")
def _up2_case():
    B, C, H, W = shape = (1, 3, 7, 9)
    up1 = synth.normal("up2/a%s" % (shape,), (B, C, 2 * H, 2 * W))
    low = synth.normal("up2/l%s" % (shape,), (B, C, H, W))
    lp, ind = plant(low)
    up1[0, 0, 0, 0] = INF                              # and one in the skip, away from the others
    ref = lambda a, l: a + F.interpolate(l, scale_factor=2, mode="nearest")
    taint = ref(torch.zeros(B, C, 2 * H, 2 * W), T(ind)) > 0
    taint[0, 0, 0, 0] = True
    # one float32 addition per element: the existing test asks for torch.equal, so ref32 is the whole reference
    return types.SimpleNamespace(up1=up1, low=lp, ref32=ref(T(up1), T(lp)), ref64=None, taint=taint)


UP_SHAPES = [(2, 5, 7, 10), (4, 8, 9, 11)]             # f, C, H, W of test_depthwise_up_add_vs_conv_transpose


def up_weight(f, C):
    """fill_up_weights' bilinear kernel plus the existing test's trainable noise -> [C,1,2f,2f]."""
    k = 2 * f
    c = (2 * f - 1 - f % 2) / (2.0 * f)
    i = np.arange(k, dtype=np.float64)
    g = 1 - np.abs(i / f - c)
    w = np.broadcast_to((g[:, None] * g[None, :]).astype(np.float32), (C, 1, k, k)).copy()
    return w + synth.normal("up/w%d" % f, (C, 1, k, k), 0, 0.05)


def _up_case(f, C, H, W):
    w = up_weight(f, C)
    x = synth.normal("up/x%d" % f, (2, C, H, W))
    skip = synth.normal("up/s%d" % f, (2, C, H * f, W * f))
    xp, ind = plant(x)
    ref = lambda xx, cv: F.conv_transpose2d(xx, cv(w), None, stride=f, padding=f // 2, groups=C) + cv(skip)
    taint = F.conv_transpose2d(T(ind), torch.ones(C, 1, 2 * f, 2 * f), None, stride=f, padding=f // 2, groups=C) > 0
    return types.SimpleNamespace(x=xp, w=w, skip=skip, f=f, ref32=ref(T(xp), _f), ref64=ref(_d(x), _d), taint=taint)


for _c in UP_SHAPES:
    case("depthwise up f%d %dx%dx%d" % _c)(functools.partial(_up_case, *_c))


# ------------------------------------------------------------------------------------------------- focal loss -----
FOCAL_N = 4 * 300 + 3                                  # the float4 body and a tail of 3


def focal_inputs():
    logits = synth.normal("nonfinite/focal/x", (1, 1, 1, FOCAL_N), -2.0, 2.0)
    gt = (synth.uniform("nonfinite/focal/gt", (1, 1, 1, FOCAL_N)) ** 4).astype(np.float32)
    gt.reshape(-1)[::37] = 1.0                         # the positives, one of them in the tail (37 * 32 = 1184 < 1200)
    gt.reshape(-1)[FOCAL_N - 1] = 1.0
    return logits, gt


FOCAL_NAN_AT = (4 * 77 + 2, FOCAL_N - 2)               # one in the float4 body, one in the tail
FOCAL_INF_AT = ((4 * 50 + 1, INF), (4 * 120 + 3, -INF), (37 * 5, INF), (FOCAL_N - 1, -INF), (FOCAL_N - 3, INF))


def _focal_case(kind):
    logits, gt = focal_inputs()
    xp = logits.copy()
    if kind == "nan":
        for i in FOCAL_NAN_AT:
            xp.reshape(-1)[i] = NAN
    else:
        for i, v in FOCAL_INF_AT:                      # on negatives and on positives (index 185, the last element)
            xp.reshape(-1)[i] = v
    act32 = olos.sigmoid_clamp(T(xp))
    loss32 = olos.neg_loss(act32, T(gt))
    act64 = olos.sigmoid_clamp(_d(xp))
    loss64 = olos.neg_loss(act64, _d(gt))
    return types.SimpleNamespace(x=xp, clean=logits, gt=gt, ref32=act32, loss32=loss32, ref64=act64, loss64=loss64,
                                 taint=torch.isnan(T(xp)))


for _k in ("nan", "inf"):
    case("focal %s" % _k)(functools.partial(_focal_case, _k))


# ---------------------------------------------------------------------------------------------- whole network -----
NET_CASES = {"dla_eighths": ("dla_34", (2, 3, 128, 160), "eighths"), "hourglass": ("smallhourglass", (2, 3, 256, 256), None)}
_NETS = {}


def net_case(name):
    """The case of train_grad_ref.py with one NaN in one input pixel of image 0, and the CPU float32 oracle's heads in
    eval and in train mode."""
    if name not in _NETS:
        import train_grad_ref as R
        from oracle import nets as onet
        arch, shape, regime = NET_CASES[name]
        c = R.Case(name, arch, shape, regime, True)
        c.xp = c.x.copy()
        c.xp[0, 1, shape[2] // 2 + 3, shape[3] // 2 + 5] = NAN
        with torch.no_grad():
            c.eval32 = c.forward(c.state_dict(), T(c.xp), onet.Options(bn_train=False))
            c.train32 = c.forward(c.state_dict(), T(c.xp), onet.Options(bn_train=True))
        _NETS[name] = c
    return _NETS[name]

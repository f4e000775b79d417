"""Up-sampling straight from a K-split DCN's slices (cp_depthwise_up_forward_slices), the f = 4 patch kernel and the
pool a two-level Tree hands down to `tree1`.  The slices forms must give the bits of the launches they replace
(cp_dcn_splitk_reduce, then cp_depthwise_up_forward): every comparison between the two routes is torch.equal."""
import contextlib
import ctypes
import itertools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from centerpoly_amd import _C, synth

pytestmark = pytest.mark.gpu
DEV = "cuda"
CP_EUNSUPPORTED = -2


def P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


@contextlib.contextmanager
def _reproducible_library_convs():
    """Maps too small for the MFMA convolution's gate (the offset convolutions of the deepest maps at these sizes) go
    to the vendor library, whose default algorithm there sums in an order that changes from launch to launch
    (BaseDetector.run): two runs of the SAME route then differ in the last bits.  Ask for its reproducible
    algorithms while two routes are compared with torch.equal."""
    keep = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        yield
    finally:
        torch.backends.cudnn.deterministic = keep


def _t(tag, shape, scale=1.0):
    return torch.from_numpy(synth.normal("upslices/" + tag, shape) * np.float32(scale)).to(DEV)


def _up_weight(tag, C, f):
    from centerpoly_amd.models.networks.pose_dla_dcn import fill_up_weights
    up = torch.nn.ConvTranspose2d(C, C, f * 2, stride=f, padding=f // 2, groups=C, bias=False)
    fill_up_weights(up)
    with torch.no_grad():
        w = up.weight.detach().clone() + torch.from_numpy(synth.normal("upslices/w" + tag, tuple(up.weight.shape), 0, 0.05))
    return w.to(DEV).contiguous()


def _two_launches(part, scale, shift, relu, w, skip, f):
    """The route the slices entry replaces: the K-split reduce, then the up-sample + add."""
    L = _C.lib()
    n, B, C, H, W = part.shape
    x = torch.full((B, C, H, W), float("nan"), device=DEV)
    _C.check(L.cp_dcn_splitk_reduce(P(part), n, P(scale), P(shift), relu, P(x), B, C, H * W, _C.stream()), "reduce")
    out = torch.full((B, C, H * f, W * f), float("nan"), device=DEV)
    _C.check(L.cp_depthwise_up_forward(P(x), P(w), P(skip), P(out), B, C, H, W, f, _C.stream()), "up")
    return x, out


def _from_slices(part, scale, shift, relu, w, skip, f):
    n, B, C, H, W = part.shape
    out = torch.full((B, C, H * f, W * f), float("nan"), device=DEV)
    rc = _C.lib().cp_depthwise_up_forward_slices(P(part), n, B * C * H * W, P(scale), P(shift), relu, P(w), P(skip), P(out),
                                                 B, C, H, W, f, _C.stream())
    return rc, out


# every image edge inside one tile, a row of one patch (f = 4, H = 3, W = 5: a ragged last workgroup in the patch kernel
# too), more slices than the unrolled loop's width
SLICE_CASES = [(2, 2, 3, 5, 6, 1), (2, 2, 3, 5, 6, 2), (2, 2, 3, 5, 6, 5), (4, 1, 2, 3, 5, 1), (4, 1, 2, 3, 5, 8)]


@pytest.mark.parametrize("f,B,C,H,W,n", SLICE_CASES, ids=lambda v: str(v))
def test_slices_entry_equals_reduce_then_upsample(f, B, C, H, W, n):
    tag = "%d_%d" % (f, n)
    part = _t("p" + tag, (n, B, C, H, W))                      # (negatives included: the ReLU has something to cut)
    assert (part < 0).any() and (part > 0).any()
    w, skip = _up_weight(tag, C, f), _t("s" + tag, (B, C, H * f, W * f))
    scale, shift = _t("sc" + tag, (C,)) + 1.5, _t("sh" + tag, (C,), 0.3)
    for relu, with_scale in itertools.product((0, 1), (False, True)):
        sc, sh = (scale, shift) if with_scale else (None, None)
        x, want = _two_launches(part, sc, sh, relu, w, skip, f)
        rc, got = _from_slices(part, sc, sh, relu, w, skip, f)
        assert rc == 0
        assert torch.isfinite(want).all() and (not relu or (x == 0).any())
        assert torch.equal(got, want), (relu, with_scale, (got - want).abs().max().item())


@pytest.mark.parametrize("C,H,W", [(2, 1, 1), (3, 3, 5), (64, 8, 16)])
@pytest.mark.parametrize("with_skip", [False, True])
def test_up4_patch_kernel_vs_conv_transpose(C, H, W, with_skip):
    """The f = 4 patch kernel against a float64 conv_transpose2d + add at test_depthwise_up_add_vs_conv_transpose's
    tolerance, and bit-equal to the slices form on one slice with the identity epilogue."""
    B, f = 2, 4
    tag = "u4_%d_%d" % (C, H)
    x, w = _t("x" + tag, (B, C, H, W)), _up_weight(tag, C, f)
    skip = _t("s" + tag, (B, C, H * f, W * f)) if with_skip else None
    ref = F.conv_transpose2d(x.cpu().double(), w.cpu().double(), None, stride=f, padding=f // 2, groups=C)
    if with_skip:
        ref = ref + skip.cpu().double()
    out = torch.full((B, C, H * f, W * f), float("nan"), device=DEV)
    _C.check(_C.lib().cp_depthwise_up_forward(P(x), P(w), P(skip), P(out), B, C, H, W, f, _C.stream()), "up")
    np.testing.assert_allclose(out.cpu().double().numpy(), ref.numpy(), rtol=1e-5, atol=1e-6)
    rc, got = _from_slices(x.reshape(1, B, C, H, W), None, None, 0, w, skip, f)
    assert rc == 0 and torch.equal(got, out)


def test_unsupported_factors_keep_the_two_launches():
    """f = 2 on an odd width and f = 8 have no slices kernel: the entry says so, and IDAUp keeps reduce + up-sample."""
    for f, W in ((2, 5), (8, 4)):
        part, w = _t("un%d" % f, (2, 1, 2, 3, W)), _up_weight("un%d" % f, 2, f)
        rc, _ = _from_slices(part, None, None, 0, w, None, f)
        assert rc == CP_EUNSUPPORTED
    ida = _prepared_ida([64, 128], [1, 8])
    layers = [_t("un/l0", (1, 64, 32, 32)), _t("un/l1", (1, 128, 4, 4))]
    L = _C.lib()
    calls = {"slices": 0, "up": 0}
    orig_s, orig_u = L.cp_dcn_v2_forward_slices, L.cp_depthwise_up_forward

    def count(name, fn):
        def wrapped(*a):
            calls[name] += 1
            return fn(*a)
        return wrapped
    L.cp_dcn_v2_forward_slices, L.cp_depthwise_up_forward = count("slices", orig_s), count("up", orig_u)
    try:
        on = _run_ida(ida, layers, True)
    finally:
        L.cp_dcn_v2_forward_slices, L.cp_depthwise_up_forward = orig_s, orig_u
    assert calls == {"slices": 0, "up": 1}
    assert torch.isfinite(on).all() and torch.equal(on, _run_ida(ida, layers, False))


def _prepared_ida(channels, up_f):
    """An IDAUp as prepare_inference leaves it (folded BatchNorm, region kernel forced), with live offsets."""
    from centerpoly_amd.models.networks.DCNv2.dcn_v2 import DCN
    from centerpoly_amd.models.networks.pose_dla_dcn import IDAUp
    torch.manual_seed(7)
    ida = IDAUp(channels[0], channels, up_f)
    with torch.no_grad():
        for m in ida.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.normal_(0, 0.05)
                m.running_var.uniform_(0.7, 1.3)
                m.weight.uniform_(0.8, 1.2)
                m.bias.normal_(0, 0.1)
            if isinstance(m, DCN):
                m.conv_offset_mask.weight.normal_(0, 0.02)
                m.conv_offset_mask.bias.normal_(0, 0.2)
                m.bias.normal_(0, 0.1)
    ida = ida.to(DEV).eval()
    for m in ida.modules():
        if hasattr(m, "fold"):
            m.fold()
        if isinstance(m, DCN):
            m.contraction = "bf16x3_region"
    return ida


def _run_ida(ida, layers, fold):
    from centerpoly_amd.models.networks.pose_dla_dcn import IDAUp
    keep = IDAUp.fold_slices
    IDAUp.fold_slices = fold
    try:
        with torch.no_grad(), _reproducible_library_convs():
            ls = list(layers)
            ida(ls, 0, len(ls))
            torch.cuda.synchronize()
            return ls[-1]
    finally:
        IDAUp.fold_slices = keep


def test_idaup_fold_slices_is_bit_identical():
    """IDAUp(64, [64, 128], [1, 2]) on maps small enough to force the region kernel's K split: the same bits with the
    slices folded into the up-sample and with the DCN's own reduce; first call (weights permuted by the call) and
    second call (prepared workspace) alike."""
    from centerpoly_amd.models.networks.DCNv2.dcn_v2 import dcn_v2_slices_count
    ida = _prepared_ida([64, 128], [1, 2])
    layers = [_t("ida/l0", (1, 64, 16, 64)), _t("ida/l1", (1, 128, 8, 32))]
    nsl = dcn_v2_slices_count(layers[1], ida.proj_1.conv.weight, contraction="bf16x3_region")
    assert nsl > 1                                            # (else both runs below are the two-launch route)
    L = _C.lib()
    calls = [0]
    orig = L.cp_depthwise_up_forward_slices

    def wrapped(*a):
        calls[0] += 1
        return orig(*a)
    L.cp_depthwise_up_forward_slices = wrapped
    try:
        on1 = _run_ida(ida, layers, True)
        off = _run_ida(ida, layers, False)
        on2 = _run_ida(ida, layers, True)
    finally:
        L.cp_depthwise_up_forward_slices = orig
    assert calls[0] == 2
    assert torch.isfinite(off).all() and off.abs().max().item() > 0
    assert torch.equal(on1, off) and torch.equal(on2, off)


def test_dla34_heads_and_pool_count_with_switches():
    """DLA-34 at the smoke test's 64x96 input, prepared: the four heads are the same bits with IDAUp.fold_slices and
    Tree.share_pool on and off, and the two-level trees (levels 3 and 4) pool once instead of twice: 4 launches, not 6."""
    from centerpoly_amd.models.model import create_model
    from centerpoly_amd.models.networks.pose_dla_dcn import IDAUp, Tree
    heads = {"hm": 8, "poly": 32, "pseudo_depth": 1, "reg": 2}
    model = create_model("dla_34", heads, 256)
    w = synth.fill_by_name({k: tuple(v.shape) for k, v in model.state_dict().items()})
    model.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()})
    model = model.to(DEV).eval()
    model.prepare_inference()
    x = torch.from_numpy(synth.normal("smoke/input", (1, 3, 64, 96))).to(DEV)
    L = _C.lib()
    orig = L.cp_maxpool2x2_forward
    pools = [0]

    def wrapped(*a):
        pools[0] += 1
        return orig(*a)

    def run(on):
        keep = IDAUp.fold_slices, Tree.share_pool
        IDAUp.fold_slices = Tree.share_pool = on
        pools[0] = 0
        L.cp_maxpool2x2_forward = wrapped
        try:
            with torch.no_grad(), _reproducible_library_convs():
                out = {k: v.clone() for k, v in model(x)[-1].items()}
            torch.cuda.synchronize()
        finally:
            L.cp_maxpool2x2_forward = orig
            IDAUp.fold_slices, Tree.share_pool = keep
        return out, pools[0]
    a, na = run(True)
    b, nb = run(False)
    assert (na, nb) == (4, 6)
    for h in heads:
        assert torch.isfinite(a[h]).all() and torch.equal(a[h], b[h]), h

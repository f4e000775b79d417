"""GPU parity: the HIP path (through the C ABI) against the CPU oracle and the
reference-generated golden vectors, on identical seeded inputs.

Tolerances (north_star): top-k / NMS indices bit-exact; fp32 heat maps, vertex
offsets and losses within 1e-3 relative (most checks are far tighter).
"""
import json

import numpy as np
import pytest
import torch

import cases
from centerpoly_amd import _C, synth
from oracle import dcn as odcn
from oracle import decode as odec
from oracle import losses as olos

pytestmark = pytest.mark.gpu
T = torch.from_numpy
DEV = "cuda"


def g(a):
    return (T(a) if isinstance(a, np.ndarray) else a).to(DEV)


# ----------------------------------------------------------------- decode ---

@pytest.mark.parametrize("case", cases.DECODE_CASES, ids=lambda c: c[0])
def test_decode_vs_oracle_and_golden(case, golden):
    from centerpoly_amd.models.decode import polydet_decode
    name, B, C, h, w, N, K, rep = case
    heat, polys, depth, reg = (T(a) for a in cases.decode_inputs_np(*case))
    for use_reg, key in ((True, "dets"), (False, "dets_noreg")):
        ref, rinds, rcls = odec.polydet_decode(heat, polys, depth, reg if use_reg else None, K=K, rep=rep)
        dets, inds, clses = polydet_decode(g(heat), g(polys), g(depth), reg=g(reg) if use_reg else None,
                                           K=K, rep=rep, return_inds=True)
        assert torch.equal(inds.cpu(), rinds), "top-k indices must be bit-exact"
        assert torch.equal(clses.cpu(), rcls)
        d = dets.cpu()
        assert torch.equal(d[..., 4], ref[..., 4])            # scores bit-exact
        if rep == "cartesian":
            assert torch.equal(d, ref)                         # whole record bit-exact
        else:
            np.testing.assert_allclose(d.numpy(), ref.numpy(), rtol=1e-6, atol=1e-5)
        gold = golden("decode_" + name)
        assert np.array_equal(inds.cpu().numpy(), gold["inds"])
        np.testing.assert_allclose(d.numpy(), gold[key], rtol=1e-6, atol=1e-5)


def _decode_both(heat, N=4, K=16, rep="cartesian"):
    from centerpoly_amd.models.decode import polydet_decode
    B, C, h, w = heat.shape
    polys = T(synth.normal("tie/poly", (B, 2 * N, h, w)))
    depth = T(synth.uniform("tie/depth", (B, 1, h, w)))
    reg = T(synth.uniform("tie/reg", (B, 2, h, w)))
    ref, rinds, rcls = odec.polydet_decode(heat, polys, depth, reg, K=K, rep=rep)
    dets, inds, clses = polydet_decode(g(heat), g(polys), g(depth), reg=g(reg), K=K, rep=rep,
                                       return_inds=True)
    return ref, rinds, rcls, dets.cpu(), inds.cpu(), clses.cpu()


@pytest.mark.parametrize("kind", ["constant", "sparse", "plateaus", "zeros", "ragged"])
def test_decode_ties_and_edge_inputs(kind):
    if kind == "constant":            # every pixel is a 3x3 maximum: all tie
        heat = torch.full((2, 3, 40, 52), 0.25)
    elif kind == "zeros":
        heat = torch.zeros((1, 8, 64, 64))
    elif kind == "sparse":            # fewer positives than K -> zeros fill in index order
        heat = torch.zeros((2, 8, 64, 96))
        idx = synth.integers("tie/sparse", (2, 9), 0, 8 * 64 * 96)
        for b in range(2):
            heat[b].view(-1)[T(idx[b])] = T(synth.uniform("tie/v%d" % b, (9,), 0.1, 0.9))
    elif kind == "plateaus":          # quantised field: many equal maxima
        heat = torch.round(T(synth.smooth_field("tie/pl", (1, 4, 48, 80))) * 2) / 8 + 0.5
    else:                             # ragged: C*H*W not a multiple of the 4096 tile, odd W
        heat = torch.sigmoid(T(synth.heat_logits("tie/rag", 3, 5, 37, 53)))
    ref, rinds, rcls, dets, inds, clses = _decode_both(heat, K=100 if kind != "ragged" else 77)
    assert torch.equal(inds, rinds) and torch.equal(clses, rcls)
    assert torch.equal(dets, ref)


def test_decode_full_size_config2():
    """BASELINE config 2 shape: 8 x 256 x 512 heat, K=128, N=16."""
    heat = torch.sigmoid(T(synth.heat_logits("full/hm", 1, 8, 256, 512)))
    ref, rinds, rcls, dets, inds, clses = _decode_both(heat, N=16, K=128)
    assert torch.equal(inds, rinds) and torch.equal(clses, rcls) and torch.equal(dets, ref)
    # size-independent properties: sorted scores, indices in range and unique per (cls, ind)
    s = dets[0, :, 4]
    assert bool((s[:-1] >= s[1:]).all())
    keys = clses[0].long() * 256 * 512 + inds[0]
    assert keys.unique().numel() == 128


@pytest.mark.parametrize("C,H,W,K", [(40, 128, 256, 128), (3, 96, 160, 256), (80, 64, 512, 100)],
                         ids=["40cls-two-merge-levels", "K256", "80cls-K100"])
def test_decode_many_classes_and_merge_levels(C, H, W, K):
    """Round-4 decode: more than 32 tiles x K candidates need the parallel merge stage, more than 32 x 32 tiles need it
    twice (the lists ping-pong between the two workspace halves); K = 256 is the kernel's maximum (one winner per
    thread of the last stage); K = 100 does not divide the 4096-key segments evenly.  Dense white-noise heat: every tile
    holds more than K local maxima, so no zero-valued key survives -- plus a copy with a plateau of equal scores."""
    heat = torch.sigmoid(T(synth.normal("manycls/hm%d" % C, (2, C, H, W))))
    heat[1, C // 2, 10:20, 30:60] = 0.999                     # ties that straddle the cut: the index passes run
    ref, rinds, rcls, dets, inds, clses = _decode_both(heat, N=4, K=K)
    assert torch.equal(inds, rinds) and torch.equal(clses, rcls) and torch.equal(dets, ref)


def test_decode_rejects_bad_arguments():
    from centerpoly_amd.models.decode import polydet_decode
    heat = torch.rand(1, 2, 8, 8, device=DEV)
    with pytest.raises(_C.NativeError):
        polydet_decode(heat, torch.zeros(1, 4, 8, 8, device=DEV), torch.zeros(1, 1, 8, 8, device=DEV),
                       K=300)           # K > 256 unsupported
    with pytest.raises(_C.NativeError):
        polydet_decode(heat, torch.zeros(1, 4, 8, 8, device=DEV), torch.zeros(1, 1, 8, 8, device=DEV),
                       K=129)           # K > C*H*W


# ------------------------------------------------------------------ focal ---

def test_sigmoid_focal_vs_oracle_and_golden(golden):
    from centerpoly_amd.models.losses import sigmoid_focal_loss
    batch, out = cases.loss_batch("base", 2, 32, 48, 16, "cartesian")
    gold = golden("loss_focal")
    x = g(out["hm"]).requires_grad_(True)
    loss, act = sigmoid_focal_loss(x.clone(), g(batch["hm"]))
    loss.backward()
    np.testing.assert_allclose(act.detach().cpu().numpy(), gold["act"], rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(loss.item(), gold["loss"], rtol=1e-5)
    scale = np.abs(gold["grad"]).max()
    np.testing.assert_allclose(x.grad.cpu().numpy(), gold["grad"], rtol=1e-3, atol=1e-6 * scale)
    # num_pos == 0 branch
    g0 = golden("loss_focal_nopos")
    x0 = g(out["hm"]).requires_grad_(True)
    l0, _ = sigmoid_focal_loss(x0.clone(), torch.zeros_like(x0))
    l0.backward()
    np.testing.assert_allclose(l0.item(), g0["loss"], rtol=1e-5)
    np.testing.assert_allclose(x0.grad.cpu().numpy(), g0["grad"], rtol=1e-3,
                               atol=1e-6 * np.abs(g0["grad"]).max())


def test_sigmoid_focal_full_size_and_extremes():
    from centerpoly_amd.models.losses import sigmoid_focal_loss
    B, C, h, w = 2, 8, 256, 512
    logits = synth.heat_logits("focal/full", B, C, h, w)
    logits.reshape(-1)[:64] = np.linspace(-30, 30, 64)          # saturates both clamp ends
    gt = synth.train_batch(B, h, w, with_input=False, stream="focal/gt")["hm"]
    x = T(logits).requires_grad_(True)
    ref = olos.neg_loss(olos.sigmoid_clamp(x), T(gt))
    ref.backward()
    xd = g(logits).requires_grad_(True)
    loss, act = sigmoid_focal_loss(xd.clone(), g(gt))
    loss.backward()
    np.testing.assert_allclose(loss.item(), ref.item(), rtol=1e-4)
    gs = x.grad.abs().max().item()
    np.testing.assert_allclose(xd.grad.cpu().numpy(), x.grad.numpy(), rtol=1e-3, atol=1e-5 * gs)
    a = act.detach()
    assert float(a.min()) >= float(np.float32(1e-4)) and float(a.max()) <= float(np.float32(1 - 1e-4))


# ------------------------------------------------------------ gathered L1 ---

@pytest.mark.parametrize("key", ["reg", "pseudo_depth"])
def test_regl1_vs_golden(key, golden):
    from centerpoly_amd.models.losses import RegL1Loss
    batch, out = cases.loss_batch("base", 2, 32, 48, 16, "cartesian")
    gold = golden("loss_regl1_" + key)
    o = g(out[key]).requires_grad_(True)
    l = RegL1Loss()(o, g(batch["reg_mask"]), g(batch["ind"]), g(batch[key]))
    l.backward()
    np.testing.assert_allclose(l.item(), gold["loss"], rtol=1e-5)
    np.testing.assert_allclose(o.grad.cpu().numpy(), gold["grad"], rtol=1e-5, atol=1e-9)


@pytest.mark.parametrize("key", ["reg", "pseudo_depth"])
def test_regsl1_vs_golden(key, golden):
    """--reg_loss sl1: cp_gather_l1 in smooth-L1 mode against the reference's RegLoss."""
    from centerpoly_amd.models.losses import RegLoss
    batch, out = cases.loss_batch("base", 2, 32, 48, 16, "cartesian")
    gold = golden("loss_regsl1_" + key)
    o = g(out[key] * 3.0).requires_grad_(True)
    l = RegLoss()(o, g(batch["reg_mask"]), g(batch["ind"]), g(batch[key]))
    l.backward()
    np.testing.assert_allclose(l.item(), gold["loss"], rtol=1e-5)
    np.testing.assert_allclose(o.grad.cpu().numpy(), gold["grad"], rtol=1e-5, atol=1e-9)


def test_mse_heat_loss_vs_golden_and_in_polydet_loss(golden):
    """--mse_loss: cp_mse_forward/backward against torch MSELoss recorded from the reference environment, and
    PolydetLoss with --mse_loss --reg_loss sl1 against the oracle."""
    from centerpoly_amd.models.losses import MSELoss
    from centerpoly_amd.trains.polydet import PolydetLoss
    batch, out = cases.loss_batch("base", 2, 32, 48, 16, "cartesian")
    gold = golden("loss_mse")
    x = g(out["hm"]).requires_grad_(True)
    l = MSELoss()(x, g(batch["hm"]))
    l.backward()
    np.testing.assert_allclose(l.item(), gold["loss"], rtol=1e-5)
    np.testing.assert_allclose(x.grad.cpu().numpy(), gold["grad"], rtol=1e-5, atol=1e-10)
    opt = _Opt(num_stacks=1, poly_loss="l1", rep="cartesian", poly_order=False, hm_weight=1.0, off_weight=1.0,
               poly_weight=1.0, depth_weight=0.1, reg_offset=True, reg_loss="sl1", mse_loss=True, task="polydet")
    loss, stats = PolydetLoss(opt)([{k: g(v) for k, v in out.items()}], {k: g(v) for k, v in batch.items()})
    ref, rstats = olos.polydet_loss([{k: T(v) for k, v in out.items()}], {k: T(v) for k, v in batch.items()},
                                    poly_loss_kind="l1", rep="cartesian", reg_loss="sl1", mse_loss=True)
    for k in rstats:
        np.testing.assert_allclose(float(stats[k]), float(rstats[k]), rtol=1e-4, atol=1e-6, err_msg=k)


class _Opt:
    def __init__(self, **kw):
        self.__dict__.update(kw)


L1_ONLY = [c for c in cases.POLY_CASES if c[6] == "l1" and not c[7]]


@pytest.mark.parametrize("case", L1_ONLY, ids=lambda c: c[0])
def test_polyloss_l1_variants_vs_golden(case, golden):
    from centerpoly_amd.models.losses import PolyLoss
    name, B, h, w, N, rep, pl, order = case
    gold = golden("loss_poly_" + name)
    batch, out = cases.loss_batch(name, B, h, w, N, rep)
    o = g(out["poly"]).requires_grad_(True)
    l = PolyLoss(_Opt(poly_loss=pl, rep=rep, poly_order=order))(
        o, g(batch["reg_mask"]), g(batch["ind"]), g(batch["poly"]))
    l.backward()
    np.testing.assert_allclose(l.item(), gold["loss"], rtol=1e-5)
    idx = g(batch["ind"])
    rows = torch.gather(o.grad.view(B, 2 * N, -1), 2, idx.unsqueeze(1).expand(B, 2 * N, idx.shape[1]))
    np.testing.assert_allclose(rows.cpu().numpy(), gold["grad_rows"], rtol=1e-3,
                               atol=1e-6 * np.abs(gold["grad_rows"]).max())
    np.testing.assert_allclose(o.grad.abs().double().sum().item(), gold["grad_abs_sum"], rtol=1e-4)


IOU_ORDER = [c for c in cases.POLY_CASES if c[6] != "l1" or c[7]]


@pytest.mark.parametrize("case", IOU_ORDER, ids=lambda c: c[0])
def test_polyloss_iou_and_order_vs_reference_golden(case, golden):
    """Weiler-Atherton IoU and order terms (HIP) vs values AND gradients recorded from the
    reference's PolyLoss (autograd through its Python clipper)."""
    from centerpoly_amd.models.losses import PolyLoss
    name, B, h, w, N, rep, pl, order = case
    gold = golden("loss_poly_" + name)
    batch, out = cases.loss_batch(name, B, h, w, N, rep)
    o = g(out["poly"]).requires_grad_(True)
    r = PolyLoss(_Opt(poly_loss=pl, rep=rep, poly_order=order))(
        o, g(batch["reg_mask"]), g(batch["ind"]), g(batch["poly"]))
    if order:
        np.testing.assert_allclose(r[1].item(), gold["order"], rtol=1e-4, atol=1e-6)
        total, main = r[0] + r[1], r[0]
    else:
        total = main = r
    np.testing.assert_allclose(main.item(), gold["loss"], rtol=1e-3, atol=1e-5)
    total.backward()
    idx = g(batch["ind"])
    rows = torch.gather(o.grad.view(B, 2 * N, -1), 2, idx.unsqueeze(1).expand(B, 2 * N, idx.shape[1]))
    scale = np.abs(gold["grad_rows"]).max()
    np.testing.assert_allclose(rows.cpu().numpy(), gold["grad_rows"], rtol=2e-3, atol=2e-4 * scale)
    np.testing.assert_allclose(o.grad.abs().double().sum().item(), gold["grad_abs_sum"], rtol=1e-3)


def _single_object_iou(subject, clip):
    """IoU of one (subject, clip) pair through the kernel: B = M = 1, loss = 1 - iou/(1+1e-6)."""
    from centerpoly_amd.models.losses import PolyLoss
    N = subject.shape[0]
    feat = torch.zeros((1, 2 * N, 2, 2))
    feat[0, :, 1, 0] = T(subject.reshape(-1))
    l = PolyLoss(_Opt(poly_loss="iou", rep="polar", poly_order=False))(
        g(feat), torch.ones((1, 1), dtype=torch.uint8, device=DEV),
        torch.full((1, 1), 2, dtype=torch.int64, device=DEV), g(clip.reshape(1, 1, -1)))
    return (1.0 - l.item()) * (1.0 + 1e-6)


def test_weiler_atherton_known_answers_on_gpu(golden):
    gk = golden("wa_kats")
    for n in ("same16", "inside", "rot015", "contains"):
        # the kernel sorts its subject by theta; these subjects are already sorted
        iou = _single_object_iou(gk[n + "_subject"], gk[n + "_clip"])
        np.testing.assert_allclose(iou, gk[n + "_iou"], rtol=1e-4, err_msg=n)


def test_polyloss_many_random_objects_vs_oracle():
    """A larger population of objects (cartesian read as polar = spirals, and genuine polar
    stars) against the oracle's literal Python clipper: values and gradients."""
    from centerpoly_amd.models.losses import PolyLoss
    for rep, tag in (("polar", "rndp"), ("cartesian", "rndc")):
        batch, out = cases.loss_batch(tag, 2, 24, 40, 16, rep, mean_objs=12)
        args = (T(batch["reg_mask"]), T(batch["ind"]), T(batch["poly"]))
        oc = T(out["poly"]).requires_grad_(True)
        ref = olos.poly_loss(oc, *args, "l1+iou", rep, False)
        ref.backward()
        od = g(out["poly"]).requires_grad_(True)
        l = PolyLoss(_Opt(poly_loss="l1+iou", rep=rep, poly_order=False))(od, *(g(a) for a in args))
        l.backward()
        np.testing.assert_allclose(l.item(), ref.item(), rtol=1e-3, atol=1e-5)
        gs = oc.grad.abs().max().item()
        np.testing.assert_allclose(od.grad.cpu().numpy(), oc.grad.numpy(), rtol=2e-3, atol=2e-4 * gs)


def test_polydet_loss_end_to_end_vs_oracle():
    """PolydetLoss (trains/polydet.py) on raw head outputs: total, every stat and the
    gradient w.r.t. every head, config-3 flavour (cartesian, l1+iou)."""
    from centerpoly_amd.trains.polydet import PolydetLoss
    batch, out = cases.loss_batch("e2e", 2, 32, 48, 16, "cartesian", mean_objs=6)
    opt = _Opt(num_stacks=1, poly_loss="l1+iou", rep="cartesian", poly_order=False, hm_weight=1.0,
               off_weight=1.0, poly_weight=1.0, depth_weight=0.1, reg_offset=True, reg_loss="l1",
               task="polydet")
    heads_c = {k: T(v).requires_grad_(True) for k, v in out.items()}
    bt = {k: T(v) for k, v in batch.items()}
    ref, rstats = olos.polydet_loss([heads_c], bt, poly_loss_kind="l1+iou", rep="cartesian")
    ref.backward()
    leaf = {k: g(v).requires_grad_(True) for k, v in out.items()}
    heads_d = {k: v * 1.0 for k, v in leaf.items()}          # non-leaf, like a conv output
    loss, stats = PolydetLoss(opt)([heads_d], {k: g(v) for k, v in batch.items()})
    loss.backward()
    np.testing.assert_allclose(loss.item(), ref.item(), rtol=1e-3)
    for k in rstats:
        np.testing.assert_allclose(float(stats[k]), float(rstats[k]), rtol=1e-3, atol=1e-6, err_msg=k)
    for k in out:
        want = heads_c[k].grad
        np.testing.assert_allclose(leaf[k].grad.cpu().numpy(), want.numpy(), rtol=2e-3,
                                   atol=2e-4 * want.abs().max().item(), err_msg=k)
    # the reference mutates output['hm'] into the activated map
    np.testing.assert_allclose(heads_d["hm"].detach().cpu().numpy(),
                               olos.sigmoid_clamp(T(out["hm"])).numpy(), rtol=1e-5, atol=1e-7)


def test_gather_l1_duplicate_centres_accumulate():
    from centerpoly_amd.models.losses import RegL1Loss
    feat = g(synth.normal("dup/f", (1, 2, 8, 8))).requires_grad_(True)
    ind = torch.tensor([[5, 5, 9]], device=DEV)
    mask = torch.tensor([[1, 1, 1]], dtype=torch.uint8, device=DEV)
    tgt = g(synth.normal("dup/t", (1, 3, 2)))
    l = RegL1Loss()(feat, mask, ind, tgt)
    l.backward()
    fc = feat.detach().cpu().requires_grad_(True)
    lr = olos.reg_l1_loss(fc, mask.cpu(), ind.cpu(), tgt.cpu())
    lr.backward()
    np.testing.assert_allclose(l.item(), lr.item(), rtol=1e-6)
    np.testing.assert_allclose(feat.grad.cpu().numpy(), fc.grad.numpy(), rtol=1e-6, atol=1e-9)


# -------------------------------------------------------------------- DCN ---

DCN_SHAPES = [
    # B, Cin, Cout, H, W
    (1, 64, 64, 32, 64),
    (2, 128, 64, 24, 40),
    (1, 256, 128, 16, 32),
    (1, 512, 256, 8, 16),
    (1, 256, 256, 12, 20),
    (2, 24, 40, 13, 19),        # ragged: channels not multiples of the tile, odd extent
    (1, 8, 300, 9, 7),          # Cout > 256 -> three 128-wide N tiles
    (1, 12, 20, 7, 2),          # narrowest supported width: every x-pair gather starts at column 0
    (2, 9, 33, 5, 3),
    # wide rows, ragged Cin
    (1, 24, 40, 5, 128),
    (2, 130, 200, 4, 64),
    (1, 64, 128, 6, 192),
    (1, 16, 64, 40, 64),
]


def _dcn_inputs(tag, B, Cin, Cout, H, W, offset_scale=2.0):
    x = synth.normal("dcn/%s/x" % tag, (B, Cin, H, W))
    om = synth.normal("dcn/%s/om" % tag, (B, 27, H, W), 0.0, offset_scale)
    w = synth.normal("dcn/%s/w" % tag, (Cout, Cin, 3, 3), 0.0, 1.0 / np.sqrt(Cin * 9))
    b = synth.normal("dcn/%s/b" % tag, (Cout,), 0.0, 0.1)
    return x, om, w, b


def _dcn_ref(x, om, w, b):
    o1, o2, m = torch.chunk(T(om), 3, dim=1)
    return odcn.dcn_v2_forward(T(x), torch.cat((o1, o2), 1), torch.sigmoid(m), T(w), T(b))


@pytest.mark.parametrize("shape", DCN_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_dcn_forward_vs_oracle(shape):
    from centerpoly_amd.models.networks.DCNv2.dcn_v2 import dcn_v2_forward_raw
    B, Cin, Cout, H, W = shape
    x, om, w, b = _dcn_inputs("%dx%d" % (Cin, Cout), *shape)
    ref = _dcn_ref(x, om, w, b)
    out = dcn_v2_forward_raw(g(x), g(om), g(w), g(b)).cpu()
    scale = ref.abs().max().item()
    np.testing.assert_allclose(out.numpy(), ref.numpy(), rtol=1e-3, atol=2e-5 * scale)


BF16X3_SHAPES = [(1, 64, 64, 32, 64), (2, 24, 40, 13, 19), (1, 256, 128, 16, 32), (1, 512, 64, 8, 16)]


@pytest.mark.parametrize("shape", BF16X3_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_dcn_forward_split_bf16_contraction(shape):
    """Inference option: split-bf16 (hi/lo, 3 bf16 MFMAs, fp32 accumulate).  Tolerance is the
    north-star's 1e-3 relative on the layer output; the measured error is ~1e-5."""
    from centerpoly_amd.models.networks.DCNv2.dcn_v2 import dcn_v2_forward_raw
    B, Cin, Cout, H, W = shape
    x, om, w, b = _dcn_inputs("%dx%d" % (Cin, Cout), *shape)
    ref = _dcn_ref(x, om, w, b)
    out = dcn_v2_forward_raw(g(x), g(om), g(w), g(b), contraction="bf16x3").cpu()
    scale = ref.abs().max().item()
    err = (out - ref).abs().max().item() / scale
    assert err < 1e-4, err
    np.testing.assert_allclose(out.numpy(), ref.numpy(), rtol=1e-3, atol=1e-4 * scale)


REGION_SHAPES = [(1, 64, 64, 32, 64), (2, 128, 64, 24, 40), (1, 256, 128, 16, 32), (1, 16, 64, 40, 64), (2, 32, 40, 13, 19),
                 (1, 64, 128, 6, 192), (1, 16, 20, 9, 7), (1, 48, 300, 7, 2), (3, 16, 64, 8, 32), (1, 32, 64, 70, 33)]


@pytest.mark.parametrize("scale", [0.2, 1.0, 2.0, 6.0])
@pytest.mark.parametrize("shape", REGION_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_dcn_forward_region_kernel(shape, scale):
    """The LDS-region kernel (dcn_fwd_region.hip; what "bf16x3" runs on the large maps), forced here on small and
    ragged maps: tiles cut by the image edge, Cout off the 64-channel block, offsets from inside the staged window
    (scale 0.2) to mostly outside it (scale 6: the cold gather path carries most samples)."""
    from centerpoly_amd.models.networks.DCNv2.dcn_v2 import dcn_v2_forward_raw
    B, Cin, Cout, H, W = shape
    x, om, w, b = _dcn_inputs("region%dx%d" % (Cin, Cout), *shape, offset_scale=scale)
    ref = _dcn_ref(x, om, w, b)
    out = dcn_v2_forward_raw(g(x), g(om), g(w), g(b), contraction="bf16x3_region").cpu()
    s_ = ref.abs().max().item()
    err = (out - ref).abs().max().item() / s_
    assert err < 1e-4, err
    np.testing.assert_allclose(out.numpy(), ref.numpy(), rtol=1e-3, atol=1e-4 * s_)


@pytest.mark.parametrize("shape,om_scale", [((1, 64, 64, 64, 512), 0.02), ((2, 32, 40, 70, 250), 0.05), ((1, 48, 64, 128, 256), 0.15),
                                            ((1, 16, 64, 128, 256), 0.4)],
                         ids=["64->64", "ragged", "48->64", "large offsets"])
def test_dcn_module_fused_offset_conv(shape, om_scale):
    """cp_dcn_v2_forward_fused: the DCN module (conv_offset_mask -> chunk / sigmoid -> deformable convolution) in one
    launch, against conv2d in float64 + the oracle's DCN on the same inputs; its copy-out of the 27 offset / mask
    channels against the convolution.  om_scale sets the size of the offsets the convolution produces (0.02: a tenth
    of a pixel; 0.4: several pixels, most samples through the cold gathers, image borders included)."""
    from centerpoly_amd.models.networks.DCNv2.dcn_v2 import dcn_v2_module_forward
    B, Cin, Cout, H, W = shape
    x, _, w, b = _dcn_inputs("fused%dx%d" % (Cin, Cout), *shape)
    wom = synth.normal("dcn/fused/wom%d" % Cin, (27, Cin, 3, 3), 0.0, om_scale)
    bom = synth.normal("dcn/fused/bom", (27,), 0.0, 0.3)
    om_ref = torch.nn.functional.conv2d(T(x).double(), T(wom).double(), T(bom).double(), padding=1).float()
    ref = _dcn_ref(x, om_ref.numpy(), w, b)
    r = dcn_v2_module_forward(g(x), g(wom), g(bom), g(w), g(b), want_om=True)
    assert r is not None
    out, om = r[0].cpu(), r[1].cpu()
    so = om_ref.abs().max().item()
    np.testing.assert_allclose(om.numpy(), om_ref.numpy(), rtol=0, atol=3e-5 * so)
    s_ = ref.abs().max().item()
    err = (out - ref).abs().max().item() / s_
    assert err < 2e-4, err
    # fused BN + ReLU epilogue and no copy-out: the same values through the other code path
    sc, sh = g(synth.uniform("dcn/fused/sc", (Cout,), 0.5, 1.5)), g(synth.normal("dcn/fused/sh", (Cout,)))
    r2 = dcn_v2_module_forward(g(x), g(wom), g(bom), g(w), None, ep_scale=sc, ep_shift=sh, relu=True)
    exp = torch.relu((r[0] - g(b).view(1, -1, 1, 1)) * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1))
    torch.testing.assert_close(r2[0], exp, rtol=1e-5, atol=1e-5 * s_)
    assert r2[1] is None


def test_dcn_large_offsets_and_borders():
    """Offsets that throw samples far outside the image (zero contribution) and exactly
    onto integer / border positions."""
    from centerpoly_amd.models.networks.DCNv2.dcn_v2 import dcn_v2_forward_raw
    B, Cin, Cout, H, W = 1, 16, 32, 10, 12
    x, om, w, b = _dcn_inputs("border", B, Cin, Cout, H, W, offset_scale=9.0)
    om[:, :18, :2] = np.round(om[:, :18, :2])                  # integer offsets
    om[:, :18, 2:4] = -1.0                                       # lands on -1 / H-1 edges
    ref = _dcn_ref(x, om, w, b)
    out = dcn_v2_forward_raw(g(x), g(om), g(w), g(b)).cpu()
    np.testing.assert_allclose(out.numpy(), ref.numpy(), rtol=1e-3, atol=2e-5 * ref.abs().max().item())


def test_dcn_zero_offset_known_answer():
    """Upstream zero-initialises conv_offset_mask => DCN(x) == 0.5*conv2d(x, W, pad=1) + b."""
    from centerpoly_amd.models.networks.DCNv2.dcn_v2 import DCN
    d = DCN(32, 48, kernel_size=(3, 3), stride=1, padding=1, dilation=1, deformable_groups=1).to(DEV)
    with torch.no_grad():
        d.bias.copy_(g(synth.normal("dcn/kat/b", (48,))))
        x = g(synth.normal("dcn/kat/x", (2, 32, 20, 28)))
        out = d(x)
        ref = 0.5 * torch.nn.functional.conv2d(x.cpu(), d.weight.cpu(), None, padding=1) \
            + d.bias.cpu().view(1, -1, 1, 1)
    np.testing.assert_allclose(out.cpu().numpy(), ref.numpy(), rtol=1e-4, atol=1e-5)


def test_dcn_full_size_properties():
    """BASELINE config 2's dominant layer (64->64 @256x512, the launch bench.py reports), too big
    for the oracle in a test: size-independent properties instead -- zero offsets reproduce the
    library convolution, the op is linear in x and in the weight, integer offsets are a shifted
    convolution tap, and an 8-bit-exact split of the batch gives the batched result."""
    from centerpoly_amd.models.networks.DCNv2.dcn_v2 import dcn_v2_forward_raw
    Cin, Cout, H, W = 64, 64, 256, 512
    x = g(synth.normal("dcn/full/x", (2, Cin, H, W)))
    w = g(synth.normal("dcn/full/w", (Cout, Cin, 3, 3), 0.0, 0.05))
    b = g(synth.normal("dcn/full/b", (Cout,)))
    zero = torch.zeros(2, 27, H, W, device=DEV)
    out0 = dcn_v2_forward_raw(x, zero, w, b)
    ref0 = 0.5 * torch.nn.functional.conv2d(x, w, None, padding=1) + b.view(1, -1, 1, 1)
    torch.testing.assert_close(out0, ref0, rtol=1e-4, atol=1e-4)
    om = g(synth.normal("dcn/full/om", (2, 27, H, W), 0.0, 1.5))
    base = dcn_v2_forward_raw(x, om, w, b)
    nb = torch.zeros_like(b)
    lin = dcn_v2_forward_raw(2.0 * x, om, w, nb) - 2.0 * dcn_v2_forward_raw(x, om, w, nb)
    assert float(lin.abs().max()) <= 1e-4 * float(base.abs().max())
    w2 = g(synth.normal("dcn/full/w2", (Cout, Cin, 3, 3), 0.0, 0.05))
    add = dcn_v2_forward_raw(x, om, w + w2, nb) - dcn_v2_forward_raw(x, om, w, nb) - dcn_v2_forward_raw(x, om, w2, nb)
    assert float(add.abs().max()) <= 2e-4 * float(base.abs().max())
    # batch entries are independent
    one = dcn_v2_forward_raw(x[1:2].contiguous(), om[1:2].contiguous(), w, b)
    assert torch.equal(one[0], base[1])
    # integer offset (+1 row, +2 columns on every tap) == the zero-offset result of the shifted image
    sh = torch.zeros(1, 27, H, W, device=DEV)
    sh[:, 0:18:2] = 1.0
    sh[:, 1:18:2] = 2.0
    xs = torch.zeros_like(x[:1])
    xs[:, :, :H - 1, :W - 2] = x[:1, :, 1:, 2:]
    a1 = dcn_v2_forward_raw(x[:1].contiguous(), sh, w, b)
    a2 = dcn_v2_forward_raw(xs, zero[:1].contiguous(), w, b)
    torch.testing.assert_close(a1[:, :, 2:H - 2, 2:W - 4], a2[:, :, 2:H - 2, 2:W - 4], rtol=1e-5, atol=1e-5)


def test_dcn_rejects_unsupported_shapes():
    from centerpoly_amd.models.networks.DCNv2.dcn_v2 import dcn_v2_forward_raw
    x = torch.zeros(1, 4, 8, 1, device=DEV)                 # W = 1: the x-pair gathers need two columns
    with pytest.raises(_C.NativeError):
        dcn_v2_forward_raw(x, torch.zeros(1, 27, 8, 1, device=DEV), torch.zeros(4, 4, 3, 3, device=DEV),
                           torch.zeros(4, device=DEV))


@pytest.mark.parametrize("cin,cout,hw,relu", [(256, 8, (32, 64), True), (256, 32, (32, 64), True), (256, 1, (16, 20), True),
                                              (256, 2, (16, 20), True), (70, 20, (9, 12), False), (5, 3, (2, 2), True)])
def test_head_output_stage_vs_torch(cin, cout, hw, relu):
    """cp_conv1x1_act_forward on a channel slice of a larger tensor == conv1x1(relu(y + b3)) + b1."""
    H, W = hw
    ytot = g(synth.normal("head/y%d_%d" % (cin, cout), (2, cin + 7, H, W)))
    b3 = g(synth.normal("head/b3", (cin + 7,)))
    w1 = g(synth.normal("head/w1%d_%d" % (cin, cout), (cout, cin), 0.0, 0.1))
    b1 = g(synth.normal("head/b1", (cout,)))
    c0 = 4
    out = torch.empty(2, cout, H, W, device=DEV)
    _C.check(_C.lib().cp_conv1x1_act_forward(
        _C.c_void_p(ytot.data_ptr() + 4 * c0 * H * W), (cin + 7) * H * W, _C.c_void_p(b3.data_ptr() + 4 * c0),
        1 if relu else 0, _C.ptr(w1.t().contiguous()), _C.ptr(b1), _C.ptr(out), 2, cin, cout, H * W, _C.stream()), "head")
    x = ytot[:, c0:c0 + cin] + b3[c0:c0 + cin].view(1, -1, 1, 1)
    if relu:
        x = x.relu()
    ref = torch.nn.functional.conv2d(x.double(), w1.double().view(cout, cin, 1, 1), b1.double()).float()
    torch.testing.assert_close(out, ref, rtol=1e-5, atol=1e-5)
    # unsupported shapes are refused, not approximated
    assert _C.lib().cp_conv1x1_act_forward(_C.ptr(ytot), 0, None, 0, _C.ptr(w1), None, _C.ptr(out), 1, cin, 33, 4,
                                           _C.stream()) == -2


def test_conv_bias_training_epilogue_vs_torch():
    """conv_offset_mask in training: in-place bias add + channel-sum bias gradient."""
    from centerpoly_amd.models.networks.DCNv2.dcn_v2 import conv_bias
    torch.manual_seed(6)
    conv = torch.nn.Conv2d(10, 27, 3, padding=1, bias=True).to(DEV)
    x1 = g(synth.normal("cb/x", (3, 10, 12, 20))).requires_grad_()
    x2 = x1.detach().clone().requires_grad_()
    go = g(synth.normal("cb/go", (3, 27, 12, 20)))
    y1 = conv_bias(conv, x1)
    (y1 * 1.0).backward(go)
    grads1 = (x1.grad.clone(), conv.weight.grad.clone(), conv.bias.grad.clone())
    conv.zero_grad()
    y2 = conv(x2)
    y2.backward(go)
    torch.testing.assert_close(y1, y2, rtol=1e-5, atol=1e-6)
    for a, b in zip(grads1, (x2.grad, conv.weight.grad, conv.bias.grad)):
        torch.testing.assert_close(a, b, rtol=1e-4, atol=1e-4)


def test_conv_bias_relu_training_epilogue_vs_torch():
    """Heads' Conv3x3(bias) -> ReLU in training: fused in-place epilogue + one-pass backward."""
    from centerpoly_amd.models.networks.pose_dla_dcn import conv_bias_relu
    torch.manual_seed(5)
    conv = torch.nn.Conv2d(12, 20, 3, padding=1, bias=True).to(DEV)
    x1 = g(synth.normal("cbr/x", (2, 12, 10, 16))).requires_grad_()
    x2 = x1.detach().clone().requires_grad_()
    go = g(synth.normal("cbr/go", (2, 20, 10, 16)))
    y1 = conv_bias_relu(conv, x1)
    y1.backward(go)
    grads1 = (x1.grad.clone(), conv.weight.grad.clone(), conv.bias.grad.clone())
    conv.zero_grad()
    y2 = torch.relu(conv(x2))
    y2.backward(go)
    torch.testing.assert_close(y1, y2, rtol=1e-5, atol=1e-6)
    for a, b in zip(grads1, (x2.grad, conv.weight.grad, conv.bias.grad)):
        torch.testing.assert_close(a, b, rtol=1e-4, atol=1e-5)


def test_dcn_fused_bn_relu_epilogue():
    from centerpoly_amd.models.networks.pose_dla_dcn import DeformConv
    m = DeformConv(32, 64).to(DEV)
    sd = {k: T(v) for k, v in cases.fill_weights({k: tuple(v.shape) for k, v in m.state_dict().items()}).items()}
    m.load_state_dict(sd)
    x = g(synth.normal("dcn/fused/x", (1, 32, 16, 24)))
    m.eval()
    with torch.no_grad():
        fused = m(x)                                  # one kernel
    with torch.enable_grad():
        plain = m.actf(m.conv(x)).detach()            # DCN, then torch BN + ReLU
    np.testing.assert_allclose(fused.cpu().numpy(), plain.cpu().numpy(), rtol=1e-4, atol=1e-5)


DCN_BWD_SHAPES = [(1, 16, 24, 12, 20), (2, 8, 140, 9, 11), (1, 64, 64, 16, 32), (1, 130, 32, 8, 8),
                  # cp_dcn_bwd_data2 on channel-split plans (maps this small split Cin over grid z and reduce the partial
                  # grad_offset / grad_mask sums) at Cout <= 64, <= 128 and <= 256: one, two and four weight fragments
                  (1, 16, 24, 6, 64), (2, 10, 70, 5, 128), (1, 6, 200, 4, 64), (1, 64, 64, 9, 192),
                  # partial tiles: heights that are no multiple of the 8-row tile, KITTI-shaped widths 160 / 80, and a
                  # width of 64 + 1 whose last 16-pixel tile holds one column
                  (1, 16, 16, 6, 160), (2, 8, 24, 5, 80), (1, 12, 8, 3, 65),
                  # Cout 260 > 256: data gradients from the generic dcn_bwd_data_kernel (weight from cp_dcn_bwd_weight2)
                  (1, 8, 260, 4, 16)]


def _check_dcn_backward_vs_oracle(x, om, w, b, gout, stride=1, pad=1, dil=1):
    """All five gradients of `_DCNv2Function` (x, offsets + mask logits `om`, weight, bias) against torch autograd
    through the oracle's DCN at the same stride / pad / dilation."""
    from centerpoly_amd.models.networks.DCNv2.dcn_v2 import _DCNv2Function
    tx, tom, tw, tb = (T(v).requires_grad_(True) for v in (x, om, w, b))
    o1, o2, m = torch.chunk(tom, 3, dim=1)
    ref = odcn.dcn_v2_forward(tx, torch.cat((o1, o2), 1), torch.sigmoid(m), tw, tb, stride, pad, dil)
    assert ref.shape == gout.shape
    ref.backward(T(gout))
    dx, dom, dw, db = (g(v).requires_grad_(True) for v in (x, om, w, b))
    out = _DCNv2Function.apply(dx, dom, dw, db, stride, pad, dil, 1)
    out.backward(g(gout))
    for name, got, want in (("x", dx.grad, tx.grad), ("om", dom.grad, tom.grad),
                            ("w", dw.grad, tw.grad), ("b", db.grad, tb.grad)):
        assert got.shape == want.shape, name
        scale = want.abs().max().item()
        np.testing.assert_allclose(got.cpu().numpy(), want.numpy(), rtol=1e-3, atol=2e-5 * scale,
                                   err_msg="grad_" + name)


@pytest.mark.parametrize("shape", DCN_BWD_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_dcn_backward_vs_oracle_autograd(shape):
    """grad_input, grad_offset, grad_mask(logit), grad_weight, grad_bias vs torch autograd
    through the oracle's DCN (the `DCN` module path: conv_offset_mask output `om` is a leaf)."""
    B, Cin, Cout, H, W = shape
    x, om, w, b = _dcn_inputs("bwd%dx%d" % (Cin, Cout), *shape)
    gout = synth.normal("dcn/bwd/go%dx%d" % (Cin, Cout), (B, Cout, H, W))
    _check_dcn_backward_vs_oracle(x, om, w, b, gout)


# Inputs that only the generic pair (dcn_bwd_data_kernel / dcn_bwd_weight_kernel) serves: (B, Cin, Cout, H, W, stride, pad, dil)
DCN_BWD_FALLBACK_CASES = [(1, 8, 12, 9, 11, 2, 1, 1),      # stride 2, output 5 x 6
                          (2, 6, 140, 7, 10, 1, 0, 1),     # pad != dil, output 5 x 8, a ragged second 128-channel slab
                          (1, 4, 6, 9, 12, 2, 2, 2),       # stride 2 with dilation 2, output 5 x 6
                          (1, 5, 9, 5, 131, 2, 1, 1)]      # output rows of 66 pixels: the 64-pixel tiles straddle rows


@pytest.mark.parametrize("case", DCN_BWD_FALLBACK_CASES, ids=lambda c: "x".join(map(str, c)))
def test_dcn_backward_fallback_kernels_vs_oracle_autograd(case):
    """The same comparison on strided, dilated and pad != dilation inputs (outside every network configuration): both
    generic kernels on their own inputs, `om` and grad_out at the output size [B, 27 | Cout, Ho, Wo]."""
    B, Cin, Cout, H, W, stride, pad, dil = case
    Ho, Wo = (H + 2 * pad - 2 * dil - 1) // stride + 1, (W + 2 * pad - 2 * dil - 1) // stride + 1
    tag = "fb%dx%ds%dp%dd%d" % (Cin, Cout, stride, pad, dil)
    x, _, w, b = _dcn_inputs(tag, B, Cin, Cout, H, W)
    om = synth.normal("dcn/%s/om_out" % tag, (B, 27, Ho, Wo), 0.0, 2.0)
    gout = synth.normal("dcn/%s/go" % tag, (B, Cout, Ho, Wo))
    _check_dcn_backward_vs_oracle(x, om, w, b, gout, stride, pad, dil)


@pytest.mark.parametrize("shape", [(2, 64, 64, 64, 128), (1, 128, 64, 128, 128)], ids=["64->64 fused forward", "128->64 separate conv"])
def test_dcn_module_single_autograd_node(shape):
    """DCN.forward in training on maps the MFMA convolution takes: one autograd node for conv_offset_mask + the deformable
    convolution (forward through cp_dcn_v2_forward_fused where the library fuses them), gradients of x, both weights
    and both biases against torch autograd through conv2d + the oracle's DCN."""
    from centerpoly_amd.models.networks.DCNv2.dcn_v2 import DCN, _DCNModuleFunction
    B, Cin, Cout, H, W = shape
    d = DCN(Cin, Cout, kernel_size=(3, 3), stride=1, padding=1, dilation=1, deformable_groups=1).to(DEV)
    with torch.no_grad():
        d.weight.copy_(g(synth.normal("dcn/node/w%d" % Cin, (Cout, Cin, 3, 3), 0.0, 1.0 / np.sqrt(Cin * 9))))
        d.bias.copy_(g(synth.normal("dcn/node/b", (Cout,), 0.0, 0.1)))
        d.conv_offset_mask.weight.copy_(g(synth.normal("dcn/node/wom%d" % Cin, (27, Cin, 3, 3), 0.0, 0.03)))
        d.conv_offset_mask.bias.copy_(g(synth.normal("dcn/node/bom", (27,), 0.0, 0.3)))
    x = g(synth.normal("dcn/node/x%d" % Cin, (B, Cin, H, W))).requires_grad_(True)
    go = g(synth.normal("dcn/node/go%d" % Cin, (B, Cout, H, W)))
    out = d(x)
    assert type(out.grad_fn).__name__ == "_DCNModuleFunctionBackward"
    params = [d.weight, d.bias, d.conv_offset_mask.weight, d.conv_offset_mask.bias]
    grads = torch.autograd.grad(out, [x] + params, go)
    # Reference: the oracle's DCN differentiated at the offsets / mask logits the KERNEL computed (the same 27 channels the
    # node saved for its backward -- two float convolutions would differ in the last bits, and a sample within ~1e-5 px
    # of an integer position would land on the other side of a bilinear kink, where grad_offset jumps), then the
    # convolution's gradients from that grad_om with torch.
    from centerpoly_amd.models.networks import conv3x3
    from centerpoly_amd.models.networks.DCNv2.dcn_v2 import dcn_v2_module_forward
    with torch.no_grad():
        r = dcn_v2_module_forward(x.detach(), params[2], params[3], params[0], params[1], want_om=True)
        om_k = r[1] if r is not None else conv3x3._launch(x.detach(), conv3x3._prepare(params[2], Cin, 27, False), params[3],
                                                          None, 27, False, 9)
    om_ref = torch.nn.functional.conv2d(x.detach().cpu().double(), params[2].detach().cpu().double(),
                                        params[3].detach().cpu().double(), padding=1)
    assert (om_k.cpu().double() - om_ref).abs().max().item() <= 3e-5 * om_ref.abs().max().item()
    tx = x.detach().cpu().requires_grad_(True)
    tom = om_k.cpu().requires_grad_(True)
    tw, tb = params[0].detach().cpu().requires_grad_(True), params[1].detach().cpu().requires_grad_(True)
    o1, o2, m = torch.chunk(tom, 3, dim=1)
    ref = odcn.dcn_v2_forward(tx, torch.cat((o1, o2), 1), torch.sigmoid(m), tw, tb)
    s_ = ref.abs().max().item()
    assert (out.detach().cpu() - ref.detach()).abs().max().item() <= 1e-4 * s_
    gx_d, gom, gw, gb = torch.autograd.grad(ref, [tx, tom, tw, tb], go.cpu())
    wom = params[2].detach().cpu()
    gx_c = torch.nn.grad.conv2d_input(tuple(tx.shape), wom, gom, padding=1)
    gw_c = torch.nn.grad.conv2d_weight(tx.detach(), tuple(wom.shape), gom, padding=1)
    want = [gx_d + gx_c, gw, gb, gw_c, gom.sum(dim=(0, 2, 3))]
    for name, a, b in zip(("x", "weight", "bias", "conv_offset_mask.weight", "conv_offset_mask.bias"), grads, want):
        scale = b.abs().max().item()
        np.testing.assert_allclose(a.cpu().numpy(), b.numpy(), rtol=2e-3, atol=3e-4 * scale, err_msg="grad_" + name)


@pytest.mark.parametrize("scale", [0.3, 6.0], ids=["window", "cold"])
def test_dcn_backward_overwrites_grad_x_and_flags(scale):
    """cp_dcn_v2_backward's contract: grad_x is OVERWRITTEN whatever it holds -- also when taps leave the staged
    window and the cold path adds into it with float atomics (scale 6) -- and the exact-f32 / narrow-tile flags
    compute the same gradients as the default split-bf16 kernels."""
    L = _C.lib()
    B, Cin, Cout, H, W = 2, 64, 64, 24, 40
    x, om, w, b = _dcn_inputs("ovw", B, Cin, Cout, H, W, offset_scale=scale)
    go = synth.normal("dcn/ovw/go", (B, Cout, H, W))
    s = _C.DcnShape(B, Cin, H, W, Cout, 3, 3, 1, 1, 1, 1)
    xg, omg, wg, gog = g(x), g(om), g(w), g(go)
    bs, off_m = 27 * H * W, 4 * 18 * H * W
    nws = L.cp_dcn_v2_backward_workspace_bytes(s)
    ws = _C.workspace(nws, xg.device)

    def run(flags, fill):
        gx = torch.full_like(xg, fill)
        gom = torch.full_like(omg, float("nan"))
        rc = L.cp_dcn_v2_backward(s, _C.ptr(xg), _C.ptr(omg), bs, _C.c_void_p(omg.data_ptr() + off_m), bs, 1, _C.ptr(wg),
                                  _C.ptr(gog), _C.ptr(gx), _C.ptr(gom), bs, _C.c_void_p(gom.data_ptr() + off_m), bs,
                                  None, None, flags, _C.ptr(ws), nws, _C.stream())
        _C.check(rc, "cp_dcn_v2_backward")
        return gx.cpu(), gom.cpu()

    base_x, base_om = run(0, 0.0)
    assert torch.isfinite(base_x).all() and torch.isfinite(base_om).all()
    sx = base_x.abs().max().item()
    for fill in (float("nan"), 123.0):
        gx, gom = run(0, fill)
        if scale < 1:                                    # inside the window: no float atomics, bit-identical reruns
            assert torch.equal(gx, base_x) and torch.equal(gom, base_om), fill
        else:                                            # cold path: float atomics, summation order varies
            np.testing.assert_allclose(gx.numpy(), base_x.numpy(), rtol=0, atol=1e-5 * sx, err_msg="fill %r" % fill)
            assert torch.equal(gom, base_om), fill
    for flags in (_C.DCN_BWD_EXACT_F32, _C.DCN_BWD_NARROW_TILES):
        gx, gom = run(flags, float("nan"))
        np.testing.assert_allclose(gx.numpy(), base_x.numpy(), rtol=0, atol=2e-4 * sx, err_msg="flags %d" % flags)
    for unknown in (64, 4):                              # no such flag: CP_EINVAL
        assert L.cp_dcn_v2_backward(s, _C.ptr(xg), _C.ptr(omg), bs, _C.c_void_p(omg.data_ptr() + off_m), bs, 1, _C.ptr(wg),
                                    _C.ptr(gog), None, None, bs, None, bs, None, None, unknown, _C.ptr(ws), nws,
                                    _C.stream()) == -1, unknown


def test_dcn_backward_propagates_non_finite_grad_out():
    """A NaN / Inf in grad_out (a loss overflow) must reach grad_x as NaN, not as silent zeros: the fixed-point
    accumulation of the data-gradient kernel has no scale for such a tile and flushes NaN instead."""
    L = _C.lib()
    B, Cin, Cout, H, W = 1, 64, 64, 24, 40
    x, om, w, b = _dcn_inputs("nan", B, Cin, Cout, H, W, offset_scale=0.3)
    go = synth.normal("dcn/nan/go", (B, Cout, H, W))
    go[0, 3, 10, 17] = np.float32("nan")
    go[0, 5, 20, 3] = np.float32("inf")
    s = _C.DcnShape(B, Cin, H, W, Cout, 3, 3, 1, 1, 1, 1)
    xg, omg, wg, gog = g(x), g(om), g(w), g(go)
    bs, off_m = 27 * H * W, 4 * 18 * H * W
    nws = L.cp_dcn_v2_backward_workspace_bytes(s)
    ws = _C.workspace(nws, xg.device)
    gx, gom = torch.empty_like(xg), torch.empty_like(omg)
    rc = L.cp_dcn_v2_backward(s, _C.ptr(xg), _C.ptr(omg), bs, _C.c_void_p(omg.data_ptr() + off_m), bs, 1, _C.ptr(wg),
                              _C.ptr(gog), _C.ptr(gx), _C.ptr(gom), bs, _C.c_void_p(gom.data_ptr() + off_m), bs,
                              None, None, 0, _C.ptr(ws), nws, _C.stream())
    _C.check(rc, "cp_dcn_v2_backward")
    gx = gx.cpu()
    assert not torch.isfinite(gx[0, :, 8:13, 14:21]).all() and not torch.isfinite(gx[0, :, 18:23, 1:6]).all()
    assert not torch.isfinite(gom.cpu()[0, :, 10, 17]).all()
    assert torch.isfinite(gx[0, :, 0:4, 30:40]).all()          # tiles away from the bad pixels are untouched


def test_dcn_backward_finite_difference():
    """Independent of the oracle: central differences on a scalar loss through the HIP forward."""
    from centerpoly_amd.models.networks.DCNv2.dcn_v2 import _DCNv2Function, dcn_v2_forward_raw
    B, Cin, Cout, H, W = 1, 6, 5, 7, 9
    x, om, w, b = _dcn_inputs("fd", B, Cin, Cout, H, W, offset_scale=0.7)
    om[:, :18] += 0.37                       # keep samples away from integer positions (kinks)
    gout = synth.normal("dcn/fd/go", (B, Cout, H, W))
    dx, dom, dw, db = (g(v).double().float().requires_grad_(True) for v in (x, om, w, b))
    _DCNv2Function.apply(dx, dom, dw, db, 1, 1, 1, 1).backward(g(gout))

    def loss(xx, oo):
        return (dcn_v2_forward_raw(xx, oo, g(w), g(b)).double() * g(gout).double()).sum().item()

    eps = 2e-3
    # perturb only offsets whose sample coordinate stays clear of integer positions (kinks of
    # the bilinear interpolant), mask logits anywhere
    ch, hh, ww = np.unravel_index(np.arange(om.size), om.shape[1:])
    tap = np.where(ch < 18, ch // 2, 0)
    base = np.where(ch % 2 == 0, hh - 1 + tap // 3, ww - 1 + tap % 3)
    coord = base + om.reshape(-1)
    frac = coord - np.floor(coord)
    safe = (ch >= 18) | ((frac > 0.05) & (frac < 0.95))
    cand = np.nonzero(safe)[0]
    idxs = cand[synth.integers("dcn/fd/idx", (8,), 0, cand.size)]
    for flat in idxs:
        d = np.zeros(om.size, np.float32)
        d[flat] = eps
        d = d.reshape(om.shape)
        num = (loss(g(x), g(om + d)) - loss(g(x), g(om - d))) / (2 * eps)
        ana = dom.grad.cpu().numpy().reshape(-1)[flat]
        assert abs(num - ana) <= 2e-2 * max(1.0, abs(ana)), (flat, num, ana)


def test_deformconv_training_path_backward():
    """DeformConv (DCN -> BN -> ReLU) in train mode: parameter grads exist and match the oracle."""
    from centerpoly_amd.models.networks.pose_dla_dcn import DeformConv
    m = DeformConv(16, 24).to(DEV).train()
    sd = {k: T(v) for k, v in cases.fill_weights({k: tuple(v.shape) for k, v in m.state_dict().items()}).items()}
    m.load_state_dict(sd)
    x = synth.normal("dcn/train/x", (2, 16, 10, 14))
    y = m(g(x))
    y.square().mean().backward()
    # oracle
    p = {k: v.clone().requires_grad_(True) for k, v in sd.items() if v.is_floating_point()}
    yo = odcn.dcn_module_forward(T(x), p["conv.weight"], p["conv.bias"], p["conv.conv_offset_mask.weight"],
                                 p["conv.conv_offset_mask.bias"])
    yo = torch.relu(torch.nn.functional.batch_norm(yo, None, None, p["actf.0.weight"], p["actf.0.bias"], True))
    yo.square().mean().backward()
    np.testing.assert_allclose(y.detach().cpu().numpy(), yo.detach().numpy(), rtol=1e-3, atol=1e-5)
    gscale = max(p[k].grad.abs().max().item() for k, _ in m.named_parameters())
    for k, v in m.named_parameters():
        want = p[k].grad
        if k == "conv.bias":      # sits before a train-mode BN: its true gradient is exactly 0
            assert v.grad.abs().max().item() <= 1e-3 * gscale
            continue
        np.testing.assert_allclose(v.grad.cpu().numpy(), want.numpy(), rtol=2e-3,
                                   atol=3e-5 * want.abs().max().item(), err_msg=k)


@pytest.mark.parametrize("f,C,H,W", [(2, 64, 16, 24), (4, 8, 9, 11), (8, 5, 6, 7), (2, 3, 5, 6), (2, 5, 7, 10), (2, 4, 1, 2), (2, 3, 6, 130)])
def test_depthwise_up_add_vs_conv_transpose(f, C, H, W):
    from centerpoly_amd.models.networks.pose_dla_dcn import depthwise_up_add, fill_up_weights
    up = torch.nn.ConvTranspose2d(C, C, f * 2, stride=f, padding=f // 2, groups=C, bias=False)
    fill_up_weights(up)
    with torch.no_grad():
        up.weight.add_(T(synth.normal("up/w%d" % f, tuple(up.weight.shape), 0, 0.05)))   # trainable
        x = T(synth.normal("up/x%d" % f, (2, C, H, W)))
        skip = T(synth.normal("up/s%d" % f, (2, C, H * f, W * f)))
        ref = up(x) + skip
        out = depthwise_up_add(g(x), up.to(DEV), g(skip)).cpu()
    np.testing.assert_allclose(out.numpy(), ref.numpy(), rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("f,C,H,W", [(2, 16, 12, 18), (4, 6, 7, 9), (2, 64, 8, 64), (2, 5, 19, 134), (2, 3, 1, 2), (2, 4, 7, 10),
                                     (2, 8, 33, 260)])
def test_depthwise_up_add_backward_vs_autograd(f, C, H, W):
    from centerpoly_amd.models.networks.pose_dla_dcn import _DepthwiseUpAdd, fill_up_weights
    up = torch.nn.ConvTranspose2d(C, C, f * 2, stride=f, padding=f // 2, groups=C, bias=False)
    fill_up_weights(up)
    with torch.no_grad():
        up.weight.add_(T(synth.normal("upb/w%d" % f, tuple(up.weight.shape), 0, 0.05)))
    x = synth.normal("upb/x%d" % f, (2, C, H, W))
    skip = synth.normal("upb/s%d" % f, (2, C, H * f, W * f))
    gout = synth.normal("upb/g%d" % f, (2, C, H * f, W * f))
    xc, sc = T(x).requires_grad_(True), T(skip).requires_grad_(True)
    wc = up.weight.detach().clone().requires_grad_(True)
    ref = torch.nn.functional.conv_transpose2d(xc, wc, None, stride=f, padding=f // 2, groups=C) + sc
    ref.backward(T(gout))
    xd, sd = g(x).requires_grad_(True), g(skip).requires_grad_(True)
    wd = up.weight.detach().to(DEV).requires_grad_(True)
    out = _DepthwiseUpAdd.apply(xd, wd, sd, f)
    out.backward(g(gout))
    np.testing.assert_allclose(out.detach().cpu().numpy(), ref.detach().numpy(), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(xd.grad.cpu().numpy(), xc.grad.numpy(), rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(sd.grad.cpu().numpy(), sc.grad.numpy(), rtol=0, atol=0)
    np.testing.assert_allclose(wd.grad.cpu().numpy(), wc.grad.numpy(), rtol=1e-3,
                               atol=1e-4 * wc.grad.abs().max().item())


@pytest.mark.parametrize("shape,relu,with_res", [((2, 16, 12, 20), True, True), ((3, 5, 7, 9), True, False),
                                                 ((2, 64, 64, 128), False, False), ((1, 8, 3, 5), True, True)])
def test_fused_bn_act_vs_torch(shape, relu, with_res):
    """Fused training BatchNorm (+residual)(+ReLU): outputs, running statistics and all gradients
    against torch.nn.BatchNorm2d + add + relu on the CPU."""
    from centerpoly_amd.models.networks.pose_dla_dcn import bn_act
    C = shape[1]
    x = synth.normal("bn/x%d" % C, shape, 0.3, 1.7)
    res = synth.normal("bn/r%d" % C, shape) if with_res else None
    gout = synth.normal("bn/g%d" % C, shape)

    def make(dev):
        bn = torch.nn.BatchNorm2d(C, momentum=0.1).to(dev).train()
        with torch.no_grad():
            bn.weight.copy_(T(synth.uniform("bn/w%d" % C, (C,), 0.5, 1.5)))
            bn.bias.copy_(T(synth.normal("bn/b%d" % C, (C,))))
            bn.running_mean.copy_(T(synth.normal("bn/rm%d" % C, (C,))))
            bn.running_var.copy_(T(synth.uniform("bn/rv%d" % C, (C,), 0.5, 2.0)))
        return bn

    bc = make("cpu")
    xc = T(x).requires_grad_(True)
    rc = T(res).requires_grad_(True) if with_res else None
    yc = bc(xc)
    if with_res:
        yc = yc + rc
    if relu:
        yc = torch.relu(yc)
    yc.backward(T(gout))
    bd = make(DEV)
    xd = g(x).requires_grad_(True)
    rd = g(res).requires_grad_(True) if with_res else None
    yd = bn_act(bd, xd, relu=relu, residual=rd)
    yd.backward(g(gout))
    np.testing.assert_allclose(yd.detach().cpu().numpy(), yc.detach().numpy(), rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(bd.running_mean.cpu().numpy(), bc.running_mean.numpy(), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(bd.running_var.cpu().numpy(), bc.running_var.numpy(), rtol=1e-5, atol=1e-6)
    from centerpoly_amd.models.networks.pose_dla_dcn import flush_batch_counts
    flush_batch_counts()                      # (the networks' forward does this once for all their BatchNorms)
    assert int(bd.num_batches_tracked) == int(bc.num_batches_tracked) == 1
    gs = xc.grad.abs().max().item()
    np.testing.assert_allclose(xd.grad.cpu().numpy(), xc.grad.numpy(), rtol=1e-3, atol=1e-5 * max(gs, 1.0))
    np.testing.assert_allclose(bd.weight.grad.cpu().numpy(), bc.weight.grad.numpy(), rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(bd.bias.grad.cpu().numpy(), bc.bias.grad.numpy(), rtol=1e-4, atol=1e-4)
    if with_res:
        np.testing.assert_allclose(rd.grad.cpu().numpy(), rc.grad.numpy(), rtol=0, atol=0)


def test_folded_conv_epilogue_matches_bn_relu():
    """BasicBlock in eval mode: folded conv + fused bias/residual/ReLU pass == conv, BN, add, ReLU."""
    from centerpoly_amd.models.networks.pose_dla_dcn import BasicBlock
    blk = BasicBlock(16, 16).to(DEV).eval()
    sd = {k: T(v) for k, v in cases.fill_weights({k: tuple(v.shape) for k, v in blk.state_dict().items()}).items()}
    blk.load_state_dict(sd)
    x = g(synth.normal("fold/x", (2, 16, 12, 20)))
    res = g(synth.normal("fold/r", (2, 16, 12, 20)))
    with torch.no_grad():
        ref = blk(x, res)
        blk.fold()
        out = blk(x, res)
    np.testing.assert_allclose(out.cpu().numpy(), ref.cpu().numpy(), rtol=1e-4, atol=1e-5)


# ------------------------------------------------------------------- nets ---

def _inference_state(model):
    """(module, attribute) pairs through which `model` still holds a tensor outside its parameters and buffers: folded
    weights, concatenated heads, prepared forms."""
    def holds(v):
        if isinstance(v, dict):
            v = list(v.values())
        return isinstance(v, torch.Tensor) or (isinstance(v, (tuple, list)) and any(holds(u) for u in v))
    return [(name, k) for name, q in model.named_modules() for k, v in vars(q).items()
            if k not in ("_parameters", "_buffers") and holds(v)]


def _load_by_name(model, gold):
    shapes = {k: tuple(v) for k, v in json.loads(str(gold["shapes"])).items()}
    model.load_state_dict({k: T(v) for k, v in cases.fill_weights(shapes).items()})
    return model.to(DEV).eval()


@pytest.mark.parametrize("fused", [False, "f32", "bf16x3", "auto", "bf16x3_region"],
                         ids=["plain", "prepare_inference", "bf16x3", "auto", "region"])
def test_dla34_forward_vs_reference_golden(fused, golden):
    """Reference DLASeg wiring (with the oracle's DCN in the plugin slot) vs the HIP path, with and
    without the inference fusions (folded BN, fused epilogues, concatenated heads), for every DCN contraction:
    exact f32, split-bf16, "auto" (what bench.py and BaseDetector run) and the LDS-region kernel forced on every
    DCN layer (what "auto" runs on the bench's large maps)."""
    from centerpoly_amd.models.model import create_model
    gold = golden("net_dla34")
    m = _load_by_name(create_model("dla_34", dict(cases.HEADS), 256), gold)
    if fused:
        m.prepare_inference(dcn_contraction=fused)
    with torch.no_grad():
        out = m(g(cases.net_input("dla")))[0]
    for h in dict(cases.HEADS):
        ref = gold["s0_" + h]
        np.testing.assert_allclose(out[h].cpu().numpy(), ref, rtol=1e-3, atol=1e-4 * np.abs(ref).max())
    if fused:
        m.train()
        assert not _inference_state(m)


@pytest.mark.parametrize("shape", [(2, 5, 6, 8), (1, 3, 7, 9), (1, 256, 16, 32)], ids=["even", "odd", "wide"])
def test_upsample2x_add_vs_torch(shape):
    """cp_upsample2x_add == up1 + nn.Upsample(scale_factor=2)(low) (Hourglass kp_module merge), values and gradients."""
    from centerpoly_amd.models.networks.large_hourglass import MergeUp
    B, C, H, W = shape
    up1 = g(synth.normal("up2/a%s" % (shape,), (B, C, 2 * H, 2 * W))).requires_grad_(True)
    low = g(synth.normal("up2/l%s" % (shape,), (B, C, H, W))).requires_grad_(True)
    out = MergeUp().fused(up1, low)
    assert out is not None
    ref = up1.detach() + torch.nn.functional.interpolate(low.detach(), scale_factor=2, mode="nearest")
    assert torch.equal(out.detach(), ref)
    go = g(synth.normal("up2/g%s" % (shape,), (B, C, 2 * H, 2 * W)))
    ga, gl = torch.autograd.grad(out, (up1, low), go)
    a2, l2 = up1.detach().clone().requires_grad_(True), low.detach().clone().requires_grad_(True)
    r2 = a2 + torch.nn.functional.interpolate(l2, scale_factor=2, mode="nearest")
    ra, rl = torch.autograd.grad(r2, (a2, l2), go)
    assert torch.equal(ga, ra)
    torch.testing.assert_close(gl, rl, rtol=1e-6, atol=1e-6)


@pytest.mark.parametrize("arch,ns", [("smallhourglass", 1), ("hourglass", 2)])
def test_hourglass_forward_vs_reference_golden(arch, ns, golden):
    from centerpoly_amd.models.model import create_model
    gold = golden("net_hourglass%d" % ns)
    m = _load_by_name(create_model(arch, dict(cases.HEADS), 64), gold)
    with torch.no_grad():
        outs = m(g(cases.net_input("hourglass")))
    for s in range(ns):
        for h in dict(cases.HEADS):
            ref = gold["s%d_%s" % (s, h)]
            np.testing.assert_allclose(outs[s][h].cpu().numpy(), ref, rtol=2e-3,
                                       atol=2e-4 * np.abs(ref).max())


def test_detector_run_config1_plumbing():
    """BASELINE config 1 (Hourglass-small, one synthetic 512x512 image, 16-vertex cartesian)
    through PolydetDetector.run, decode checked against the oracle on the same head outputs."""
    from centerpoly_amd.detectors.detector_factory import detector_factory
    from centerpoly_amd.opts import opts
    from oracle import post as opost
    opt = opts().init(["polydet", "--arch", "smallhourglass", "--input_h", "512", "--input_w", "512"])
    torch.manual_seed(317)
    det = detector_factory["polydet"](opt)
    img = (synth.uniform("cfg1/img", (512, 512, 3)) * 255).astype(np.uint8)
    # the head outputs of THIS run (a second forward would not do: on the 4x4 maps of the hourglass the library's
    # convolutions sum in a run-dependent order, and last-bit differences reorder near-tied peaks)
    grabbed = []
    handle = det.model.register_forward_hook(
        lambda m, i, o: grabbed.append({k: v.detach().clone() for k, v in o[-1].items()}))
    ret = det.run(img)
    handle.remove()
    assert set(ret) == {"results", "tot", "load", "pre", "net", "dec", "post", "merge"}
    res = ret["results"]
    assert sorted(res) == list(range(1, 9))
    assert sum(len(v) for v in res.values()) == opt.K
    assert all(v.shape[1] == 2 * 16 + 6 for v in res.values())
    # oracle on the same head outputs
    _, meta = det.pre_process(img, 1.0)
    assert len(grabbed) == 1
    out = grabbed[0]
    hm = out["hm"].sigmoid().cpu()
    dref, _, _ = odec.polydet_decode(hm, out["poly"].cpu(), out["pseudo_depth"].cpu(), out["reg"].cpu(),
                                     K=opt.K, rep="cartesian")
    ref = opost.merge_outputs([opost.detector_post_process(dref.numpy(), meta, 1.0, 8)], 8, opt.K)
    for j in range(1, 9):
        assert res[j].shape == ref[j].shape
        np.testing.assert_allclose(res[j], ref[j], rtol=1e-5, atol=1e-3)


# ---------------------------------------------------------------- trainer ---

def _tiny_train_setup(arch, extra, B, H, W, N, rep):
    from centerpoly_amd.models.model import create_model
    from centerpoly_amd.opts import opts
    from centerpoly_amd.trains.train_factory import train_factory
    opt = opts().init(["polydet", "--arch", arch, "--nbr_points", str(N), "--rep", rep] + extra)
    opt.device = torch.device(DEV)
    torch.manual_seed(317)
    model = create_model(opt.arch, opt.heads, opt.head_conv)
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    model.load_state_dict({k: T(v) for k, v in cases.fill_weights(shapes).items()})
    optim = torch.optim.Adam(model.parameters(), opt.lr)
    trainer = train_factory["polydet"](opt, model, optim)
    nb = synth.train_batch(B, H // 4, W // 4, nbr_points=N, rep=rep, mean_objs=5, in_h=H, in_w=W,
                           stream="trainer/%s" % arch)
    return opt, model, trainer, nb


@pytest.mark.parametrize("arch,extra,N,rep", [
    ("dla_34", ["--poly_loss", "l1+iou"], 16, "cartesian"),                 # config 3 flavour
    ("dla_34", ["--poly_loss", "l1", "--poly_order"], 32, "cartesian"),     # config 5 flavour
], ids=["cfg3_l1iou", "cfg5_order"])
def test_trainer_step_matches_oracle_losses(arch, extra, N, rep):
    """One PolydetTrainer step on a tiny batch: loss stats equal the oracle's on the model's own
    head outputs, every parameter receives a finite gradient and Adam moves the weights."""
    opt, model, trainer, nb = _tiny_train_setup(arch, extra, 2, 64, 128, N, rep)
    trainer.set_device(opt.gpus, opt.chunk_sizes, opt.device)
    batch = {k: g(v) for k, v in nb.items()}
    model.train()
    # head outputs in train mode (BN batch statistics), before the loss mutates 'hm'
    with torch.no_grad():
        heads = {k: v.clone().cpu() for k, v in model(batch["input"])[-1].items()}
    model.zero_grad(set_to_none=True)
    before = {k: v.detach().clone() for k, v in model.named_parameters()}
    # undo the BN running-stat update of the probe forward so the step sees the same state
    out, loss, stats = trainer.step(batch, train=True)
    ref, rstats = olos.polydet_loss([heads], {k: T(v) for k, v in nb.items()},
                                    poly_loss_kind=opt.poly_loss, rep=rep, poly_order=opt.poly_order)
    for k in rstats:
        np.testing.assert_allclose(float(stats[k]), float(rstats[k]), rtol=1e-3, atol=1e-5, err_msg=k)
    moved = 0
    for k, v in model.named_parameters():
        if not v.requires_grad:            # the reference's dead Tree.project branches
            assert ".project." in k and k.startswith(("base.level3.", "base.level4.")), k
            continue
        assert v.grad is not None and torch.isfinite(v.grad).all(), k
        moved += int(not torch.equal(v.detach(), before[k]))
    assert moved > 0.9 * len(before)


def test_trainer_hourglass_polar_two_stacks():
    """Config 4 flavour at toy size: 2-stack Hourglass, polar 24-vertex head, l1 loss averaged over
    both stacks (trains/polydet.py:43,81-125).  BatchNorm runs on its running statistics here: at
    this toy size the deepest level is 1x1, and batch statistics over two values make the forward
    pass chaotic (two identical train-mode forwards differ by O(1)), which is a property of the
    toy shape, not of the code under test."""
    opt, model, trainer, nb = _tiny_train_setup("hourglass", ["--poly_loss", "l1"], 2, 128, 128, 24, "polar")
    trainer.set_device(opt.gpus, opt.chunk_sizes, opt.device)
    batch = {k: g(v) for k, v in nb.items()}
    model.eval()
    with torch.no_grad():
        outs = [{k: v.clone().cpu() for k, v in o.items()} for o in model(batch["input"])]
    with torch.enable_grad():
        out, loss, stats = trainer.model_with_loss(batch)
        loss.backward()
    ref, rstats = olos.polydet_loss(outs, {k: T(v) for k, v in nb.items()}, num_stacks=2,
                                    poly_loss_kind="l1", rep="polar")
    for k in rstats:
        np.testing.assert_allclose(float(stats[k]), float(rstats[k]), rtol=1e-3, atol=1e-5, err_msg=k)
    for k, v in model.named_parameters():          # every Hourglass parameter is live (DDP-safe)
        assert v.grad is not None and torch.isfinite(v.grad).all(), k


def test_losses_with_no_objects_and_full_object_table():
    from centerpoly_amd.trains.polydet import PolydetLoss
    opt = _Opt(num_stacks=1, poly_loss="l1+iou", rep="cartesian", poly_order=True, hm_weight=1.0,
               off_weight=1.0, poly_weight=1.0, depth_weight=0.1, reg_offset=True, reg_loss="l1",
               task="polydet")
    for fill in (0, 1):                     # empty image / all 128 slots used
        batch, out = cases.loss_batch("edge%d" % fill, 1, 24, 40, 16, "cartesian", mean_objs=4)
        batch["reg_mask"][:] = fill
        if fill:
            batch["ind"][0] = np.arange(128) * 7 % (24 * 40)
            batch["poly"][0] = synth.normal("edge/poly", (128, 32), 0, 6.0)
        if not fill:
            batch["hm"][:] = 0
        hc = {k: T(v).requires_grad_(True) for k, v in out.items()}
        ref, rstats = olos.polydet_loss([hc], {k: T(v) for k, v in batch.items()},
                                        poly_loss_kind="l1+iou", rep="cartesian", poly_order=True)
        ref.backward()
        leaf = {k: g(v).requires_grad_(True) for k, v in out.items()}
        loss, stats = PolydetLoss(opt)([{k: v * 1.0 for k, v in leaf.items()}], {k: g(v) for k, v in batch.items()})
        loss.backward()
        for k in rstats:
            np.testing.assert_allclose(float(stats[k]), float(rstats[k]), rtol=1e-3, atol=1e-5, err_msg=k)
        want = hc["poly"].grad
        np.testing.assert_allclose(leaf["poly"].grad.cpu().numpy(), want.numpy(), rtol=3e-3,
                                   atol=3e-4 * max(want.abs().max().item(), 1e-9))


def test_polyiou_max_vertices_64():
    """N = 64 (the kernel's maximum): 105 KB of LDS per object."""
    from centerpoly_amd.models.losses import PolyLoss
    batch, out = cases.loss_batch("n64", 1, 16, 24, 64, "polar", mean_objs=3)
    args = (T(batch["reg_mask"]), T(batch["ind"]), T(batch["poly"]))
    oc = T(out["poly"]).requires_grad_(True)
    ref = olos.poly_loss(oc, *args, "iou", "polar", False)
    ref.backward()
    od = g(out["poly"]).requires_grad_(True)
    l = PolyLoss(_Opt(poly_loss="iou", rep="polar", poly_order=False))(od, *(g(a) for a in args))
    l.backward()
    np.testing.assert_allclose(l.item(), ref.item(), rtol=1e-3, atol=1e-5)
    gs = oc.grad.abs().max().item()
    np.testing.assert_allclose(od.grad.cpu().numpy(), oc.grad.numpy(), rtol=3e-3, atol=3e-4 * gs)


def test_ddp_wrapper_on_gpu_matches_plain_step():
    """The multi-GPU wrapper (DistributedDataParallel over RCCL) around the real trainer, forced at
    world_size 1: same loss as the plain step, gradients flow through every custom autograd op."""
    import os
    import torch.distributed as dist
    losses = []
    for force in ("0", "1"):
        os.environ["CP_FORCE_DDP"] = force
        started = False
        if force == "1" and not dist.is_initialized():
            os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT="29611", RANK="0", WORLD_SIZE="1")
            dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
            started = True
        try:
            opt, model, trainer, nb = _tiny_train_setup("dla_34", ["--poly_loss", "l1+iou"], 2, 64, 128, 16,
                                                        "cartesian")
            trainer.set_device(opt.gpus, opt.chunk_sizes, torch.device("cuda", 0))
            assert (trainer._ddp is not None) == (force == "1")
            batch = {k: g(v) for k, v in nb.items()}
            model.train()
            _, loss, _ = trainer.step(batch, train=True)
            _, loss2, _ = trainer.step(batch, train=True)
            losses.append((loss.item(), loss2.item()))
        finally:
            if started:
                dist.destroy_process_group()
            os.environ["CP_FORCE_DDP"] = "0"
    np.testing.assert_allclose(losses[0], losses[1], rtol=1e-4)


# ------------------------------------------------------- direct convolution (DLA base, full resolution) ---
@pytest.mark.parametrize("cin,cout,k,stride,shape", [
    (3, 16, 7, 1, (1, 40, 136)), (3, 16, 7, 1, (2, 9, 70)), (16, 16, 3, 1, (1, 24, 128)), (16, 16, 3, 1, (2, 11, 50)),
    (16, 32, 3, 2, (1, 32, 256)), (16, 32, 3, 2, (2, 13, 70)), (16, 16, 3, 2, (1, 10, 64)), (16, 32, 3, 1, (1, 8, 64)),
], ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_direct_conv_vs_torch_conv2d(cin, cout, k, stride, shape):
    """cp_conv_direct_forward (+ bias + ReLU epilogue) against F.conv2d fp32, including ragged tiles."""
    B, H, W = shape
    x = g(synth.normal("dconv/x%d%d" % (cin, H), (B, cin, H, W)))
    w = g(synth.normal("dconv/w%d%d%d" % (cin, cout, k), (cout, cin, k, k), 0.0, 1.0 / np.sqrt(cin * k * k)))
    b = g(synth.normal("dconv/b%d" % cout, (cout,), 0.0, 0.3))
    pad = k // 2
    L = _C.lib()
    assert L.cp_conv_direct_supported(cin, cout, k, stride, pad) == 1
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    for relu in (1, 0):
        out = torch.full((B, cout, Ho, Wo), float("nan"), device=DEV)
        _C.check(L.cp_conv_direct_forward(_C.ptr(x), _C.ptr(w), _C.ptr(b), _C.ptr(out), B, cin, H, W, cout, k, stride,
                                          pad, relu, _C.stream()), "cp_conv_direct_forward")
        ref = torch.nn.functional.conv2d(x.cpu(), w.cpu(), b.cpu(), stride=stride, padding=pad)
        if relu:
            ref = torch.relu(ref)
        np.testing.assert_allclose(out.cpu().numpy(), ref.numpy(), rtol=1e-4, atol=1e-5 * ref.abs().max().item())
        if k == 3:
            # round 4: the same call under the split-bf16 arithmetic (cp_conv_direct_forward_ex, bf16 matrix cores) against
            # float64, 2e-5 of the max-norm like every split-bf16 convolution (tests/test_conv_mfma.py); rerun bit-identical
            ref64 = torch.nn.functional.conv2d(x.cpu().double(), w.cpu().double(), b.cpu().double(), stride=stride, padding=pad)
            if relu:
                ref64 = torch.relu(ref64)
            outs = []
            for _ in range(2):
                o2 = torch.full((B, cout, Ho, Wo), float("nan"), device=DEV)
                _C.check(L.cp_conv_direct_forward_ex(_C.ptr(x), _C.ptr(w), _C.ptr(b), _C.ptr(o2), B, cin, H, W, cout, k,
                                                     stride, pad, relu, 1, _C.stream()), "cp_conv_direct_forward_ex")
                outs.append(o2)
            assert torch.equal(outs[0], outs[1]) and torch.isfinite(outs[0]).all()
            err = (outs[0].cpu().double() - ref64).abs().max().item() / ref64.abs().max().item()
            assert err <= 2e-5, err
    assert L.cp_conv_direct_supported(8, 16, 3, 1, 1) == 0


def test_direct_conv_full_resolution_stem():
    """The three layers at the bench shape (1x3x1024x2048) against the library convolution on the device."""
    x = g(synth.normal("dconv/full/x", (1, 3, 1024, 2048)))
    L = _C.lib()
    cin = 3
    for cout, k, stride in ((16, 7, 1), (16, 3, 1), (32, 3, 2)):
        w = g(synth.normal("dconv/full/w%d%d" % (cout, k), (cout, cin, k, k), 0.0, 1.0 / np.sqrt(cin * k * k)))
        b = g(synth.normal("dconv/full/b%d%d" % (cout, k), (cout,), 0.0, 0.1))
        pad = k // 2
        H, W = x.shape[2:]
        Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
        out = torch.empty((1, cout, Ho, Wo), device=DEV)
        _C.check(L.cp_conv_direct_forward(_C.ptr(x), _C.ptr(w), _C.ptr(b), _C.ptr(out), 1, cin, H, W, cout, k, stride,
                                          pad, 1, _C.stream()), "cp_conv_direct_forward")
        ref = torch.relu(torch.nn.functional.conv2d(x, w, b, stride=stride, padding=pad))
        assert (out - ref).abs().max().item() <= 1e-4 * ref.abs().max().item()
        if k == 3:                                   # the split-bf16 form at the bench shape (what inference runs)
            o2 = torch.empty_like(out)
            _C.check(L.cp_conv_direct_forward_ex(_C.ptr(x), _C.ptr(w), _C.ptr(b), _C.ptr(o2), 1, cin, H, W, cout, k, stride,
                                                 pad, 1, 1, _C.stream()), "cp_conv_direct_forward_ex")
            assert (o2 - ref).abs().max().item() <= 2e-5 * ref.abs().max().item()
        x, cin = out, cout


@pytest.mark.parametrize("ns,poly,hw", [(1, 32, (128, 256)), (2, 48, (128, 128))], ids=["1stack-cart16", "2stack-polar24"])
def test_hourglass_prepare_inference_matches_plain_eval(ns, poly, hw):
    """Hourglass inference fusions (folded BatchNorm, fused bias/residual/ReLU epilogues, heads' 3x3
    convolutions as one + streaming 1x1 tails, 48-channel polar head in 32-channel slices) against the
    plain eval-mode modules, every stack's every head."""
    from centerpoly_amd.models.networks.large_hourglass import HourglassNet
    heads = {"hm": 8, "poly": poly, "pseudo_depth": 1, "reg": 2}
    m = HourglassNet(heads, ns)
    sd = {k: T(v) for k, v in cases.fill_weights({k: tuple(v.shape) for k, v in m.state_dict().items()}).items()}
    m.load_state_dict(sd)
    m = m.to(DEV).eval()
    x = g(synth.normal("hg/fused/x", (2, 3) + hw))
    with torch.no_grad():
        plain = m(x)
        m.prepare_inference()
        fused = m(x)
    assert len(plain) == len(fused) == ns
    for a, b in zip(plain, fused):
        for h in heads:
            scale = a[h].abs().max().item()
            assert (a[h] - b[h]).abs().max().item() <= 2e-4 * scale, h
    m.train()
    assert m._heads_cat is None and all(getattr(q, "_folded", None) is None for q in m.modules())
    assert not _inference_state(m)


def test_direct_conv_training_function_gradients():
    """conv_train (direct forward, library gradients) against nn.Conv2d autograd."""
    from centerpoly_amd.models.networks.pose_dla_dcn import conv_train
    for cin, cout, k, stride in ((3, 16, 7, 1), (16, 16, 3, 1), (16, 32, 3, 2)):
        conv = torch.nn.Conv2d(cin, cout, k, stride, k // 2, bias=False).to(DEV)
        x1 = g(synth.normal("dconv/train/x%d" % cin, (2, cin, 24, 64))).requires_grad_(True)
        x2 = x1.detach().clone().requires_grad_(True)
        go = g(synth.normal("dconv/train/go%d%d" % (cout, stride), (2, cout, 24 // stride, 64 // stride)))
        y1 = conv_train(conv, x1)
        y1.backward(go)
        gw1 = conv.weight.grad.clone()
        conv.zero_grad()
        y2 = conv(x2)
        y2.backward(go)
        torch.testing.assert_close(y1, y2, rtol=1e-4, atol=1e-5)
        # (3x3 / stride 1: both gradients come from the split-bf16 kernels -- ~2^-16 per product, max-norm bound)
        mfma = k == 3 and stride == 1
        for got, ref in ((x1.grad, x2.grad), (gw1, conv.weight.grad)):
            if mfma:
                assert (got - ref).abs().max().item() <= 2e-5 * ref.abs().max().item()
            else:
                torch.testing.assert_close(got, ref, rtol=1e-4, atol=1e-4)


def test_hip_graph_replay_of_an_inference_step():
    """utils/hip_graph.GraphedStep: the captured step (library convolutions, the hand-written kernels launched
    through ctypes on torch's current stream, decode) replays to the eager step's result, also after the static
    input has been rewritten in place."""
    from centerpoly_amd.models.decode import polydet_decode
    from centerpoly_amd.models.model import create_model
    from centerpoly_amd.utils.hip_graph import GraphedStep
    heads = {"hm": 8, "poly": 32, "pseudo_depth": 1, "reg": 2}
    torch.manual_seed(5)
    model = create_model("dla_34", heads, 256).to(DEV).eval()
    model.prepare_inference()
    x = g(synth.normal("graph/x0", (1, 3, 256, 512)))

    def step():
        with torch.no_grad():
            out = model(x)[-1]
            return polydet_decode(out["hm"].sigmoid_(), out["poly"], out["pseudo_depth"], reg=out["reg"], K=32)

    ref0 = step().clone()
    gs = GraphedStep(step)
    assert torch.equal(gs(), ref0)
    x.copy_(g(synth.normal("graph/x1", (1, 3, 256, 512))))      # new image into the static input
    ref1 = step().clone()
    assert not torch.equal(ref0, ref1)
    assert torch.equal(gs(), ref1)


@pytest.mark.parametrize("shape", [(2, 16, 64, 128), (1, 3, 9, 7), (3, 5, 16, 30), (1, 2, 2, 2)],
                         ids=["aligned", "odd rows and columns", "W % 4 != 0", "single window"])
def test_maxpool2x2_forward_backward_match_torch(shape):
    """cp_maxpool2x2_*: values and gradient routing equal torch's MaxPool2d(2, 2), ties included (ReLU-like input with
    many equal zeros: the first maximum in row-major order takes the gradient)."""
    import torch.nn.functional as F
    from centerpoly_amd.models.networks.pose_dla_dcn import downsample2
    x = torch.relu(g(synth.normal("pool/x%s" % (shape,), shape))).requires_grad_(True)    # ~half zeros -> ties
    pool = torch.nn.MaxPool2d(2, stride=2)
    y = downsample2(pool, x)
    yr = F.max_pool2d(x.detach().clone().requires_grad_(True), 2, 2)
    assert torch.equal(y, yr)
    go = g(synth.normal("pool/go%s" % (shape,), tuple(y.shape)))
    (gx,) = torch.autograd.grad(y, x, go)
    xr = x.detach().clone().requires_grad_(True)
    (gr,) = torch.autograd.grad(F.max_pool2d(xr, 2, 2), xr, go)
    assert torch.equal(gx, gr)


def test_zero_pool_hands_out_disjoint_zeroed_tensors():
    """_C.zeros (the pooled accumulators the weight-gradient kernels add into): every tensor is zero, 256-byte aligned
    and disjoint from every other live one; a used-up block is replaced, never re-zeroed under live tensors; large
    requests bypass the pool."""
    from centerpoly_amd import _C
    pool = _C._zero_pool
    taken, spans = [], []
    n_blocks = 0
    last_block = None
    for i in range(60):
        shape = (256, 64, 3, 3) if i % 3 == 0 else ((512,) if i % 3 == 1 else (1024, 1024))      # 0.6 MB, 2 KB, 4 MB
        t = _C.zeros(shape, DEV)
        assert t.is_contiguous() and t.dtype == torch.float32 and tuple(t.shape) == shape and t.data_ptr() % 256 == 0
        assert not t.any()
        t.fill_(float(i + 1))                              # what a kernel accumulating into it would do
        taken.append(t)
        spans.append((t.data_ptr(), t.data_ptr() + t.numel() * 4))
        if pool.block is not last_block:
            n_blocks += 1
            last_block = pool.block
    assert n_blocks >= 2                                   # 60 x ~1.5 MB crossed the 64 MB block at least once
    spans.sort()
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))
    for i, t in enumerate(taken):
        assert (t == float(i + 1)).all()                   # nothing was re-zeroed or overwritten behind a live tensor
    big = _C.zeros((4096, 4096), DEV)                      # 64 MB: not carved from a block
    assert not big.any() and big.untyped_storage().nbytes() == 4096 * 4096 * 4

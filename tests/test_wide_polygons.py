"""Detection with polygons of up to 64 vertices: the decode with polygon rows of up to 128 numbers at every K <= 256
(csrc/decode.hip stages the winners' rows [K][N2] in up to 128 KB of LDS), heads of 65 .. 128 output channels inside
the one fused heads launch (csrc/heads_fused.hip: two 64-column segments over the same 3x3 tiles), and the chain
around them -- models, detector, result writer, training -- at N = 64.

Decode: indices bit-exact against the oracle, records bit-exact (cartesian) or within rtol 1e-6 / atol 1e-5 (polar:
double trig on both sides), and against fixtures recorded from the reference's own decode at N = 64
(tests/golden/gen_decode_wide_golden.py).  Fused heads: float64 torch, 2e-5 of the max-norm, the bound of every
split-bf16 contraction (tests/test_conv_mfma.py)."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cases
import wide_cases
from centerpoly_amd import _C, synth
from oracle import decode as odec
from oracle import losses as olos
from oracle import post as opost

T = torch.from_numpy
DEV = "cuda"
TOL = 2e-5


def P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def g(a):
    return (T(a) if isinstance(a, np.ndarray) else a).to(DEV)


# ------------------------------------------------------------------------------------------------------------ decode --
def _decode_both(heat, polys, depth, reg, K, rep="cartesian", cat_spec=False):
    from centerpoly_amd.models.decode import polydet_decode
    ref, rinds, rcls = odec.polydet_decode(heat, polys, depth, reg, K=K, rep=rep, cat_spec_poly=cat_spec)
    dets, inds, clses = polydet_decode(g(heat), g(polys), g(depth), reg=g(reg) if reg is not None else None, K=K,
                                       rep=rep, cat_spec_poly=cat_spec, return_inds=True)
    return ref, rinds, rcls, dets.cpu(), inds.cpu(), clses.cpu()


def _assert_decode(ref, rinds, rcls, dets, inds, clses, rep):
    assert torch.equal(inds, rinds), "top-k indices must be bit-exact"
    assert torch.equal(clses, rcls)
    assert torch.equal(dets[..., 4], ref[..., 4])                 # scores bit-exact
    if rep == "cartesian":
        assert torch.equal(dets, ref)                             # whole record bit-exact
    else:
        np.testing.assert_allclose(dets.numpy(), ref.numpy(), rtol=1e-6, atol=1e-5)


# name, B, C, h, w, N, K, rep -- K * N2 * 4 bytes of polygon rows: 64 KB, 57 KB (the first row width over the old
# 56 KB cap), 128 KB (the largest), and the two polar representations
WIDE = [("w/cart64", 2, 3, 16, 32, 64, 128, "cartesian"), ("w/cart57", 1, 3, 16, 32, 57, 128, "cartesian"),
        ("w/cart64k256", 1, 3, 16, 32, 64, 256, "cartesian"), ("w/polar64", 2, 3, 16, 32, 64, 128, "polar"),
        ("w/polarfixed64", 2, 3, 16, 32, 64, 128, "polar_fixed")]


@pytest.mark.gpu
@pytest.mark.parametrize("case", WIDE, ids=lambda c: c[0][2:])
def test_decode_wide_rows_vs_oracle(case):
    rep, K = case[7], case[6]
    heat, polys, depth, reg = (T(a) for a in cases.decode_inputs_np(*case))
    _assert_decode(*_decode_both(heat, polys, depth, reg, K, rep), rep)


@pytest.mark.gpu
def test_decode_wide_rows_without_reg():
    case = WIDE[0]
    heat, polys, depth, _ = (T(a) for a in cases.decode_inputs_np(*case))
    _assert_decode(*_decode_both(heat, polys, depth, None, case[6]), "cartesian")


@pytest.mark.gpu
def test_decode_wide_rows_plateaus():
    """A quantised field, many equal maxima (the "plateaus" kind of test_decode_ties_and_edge_inputs) at N = 64."""
    heat = torch.round(T(synth.smooth_field("wide/pl", (1, 4, 48, 80))) * 2) / 8 + 0.5
    polys = T(synth.normal("wide/pl/poly", (1, 128, 48, 80)))
    depth = T(synth.uniform("wide/pl/depth", (1, 1, 48, 80)))
    reg = T(synth.uniform("wide/pl/reg", (1, 2, 48, 80)))
    _assert_decode(*_decode_both(heat, polys, depth, reg, 128), "cartesian")


@pytest.mark.gpu
def test_decode_wide_rows_cat_spec_poly():
    """One 64-vertex polygon per class; the reference's view precondition needs w == 2N = 128."""
    case = ("w/catspec64", 1, 2, 4, 128, 64, 128)
    heat, polys, depth, reg = (T(a) for a in cases.catspec_decode_inputs_np(*case))
    _assert_decode(*_decode_both(heat, polys, depth, reg, 128, cat_spec=True), "cartesian")


@pytest.mark.gpu
def test_decode_refuses_rows_wider_than_128():
    L = _C.lib()
    B, C, h, w, K = 1, 2, 8, 16, 16
    heat = torch.rand(B, C, h, w, device=DEV)
    depth = torch.zeros(B, 1, h, w, device=DEV)
    ws = torch.empty(max(L.cp_polydet_decode_workspace_bytes(B, C, h, w, K), 8), dtype=torch.uint8, device=DEV)
    for N2, want in ((128, 0), (130, -2)):                        # -2: CP_EUNSUPPORTED
        polys = torch.zeros(B, N2, h, w, device=DEV)
        dets = torch.empty(B, K, N2 + 7, device=DEV)
        rc = L.cp_polydet_decode_ex(P(heat), P(polys), P(depth), None, B, C, h, w, N2, K, 0, 0, P(dets), None, None,
                                    P(ws), ws.numel(), _C.stream())
        assert rc == want, (N2, rc)
        rc = L.cp_polydet_decode(P(heat), P(polys), P(depth), None, B, C, h, w, N2, K, 0, P(dets), None, None, P(ws),
                                 ws.numel(), _C.stream())
        assert rc == want, (N2, rc)
    torch.cuda.synchronize()


@pytest.mark.parametrize("case", wide_cases.WIDE_DECODE_CASES, ids=lambda c: c[0])
def test_oracle_decode_matches_reference_at_64_vertices(case, golden):
    """The oracle against the reference's own decode at N = 64 (the comparison of tests/test_oracle_golden.py)."""
    name, B, C, h, w, N, K, rep = case
    gold = golden("decode_" + name)
    heat, polys, depth, reg = (T(a) for a in cases.decode_inputs_np(*case))
    nm = odec.nms(heat)
    assert int((nm != 0).sum()) == int(gold["nms_nnz"])
    assert float(nm.double().sum()) == float(gold["nms_sum"])
    scores, inds, clses, ys, xs = odec.topk(nm, K)
    assert np.array_equal(inds.numpy(), gold["inds"])             # bit-exact indices
    assert np.array_equal(clses.numpy(), gold["clses"])
    assert np.array_equal(scores.numpy(), gold["scores"])
    assert np.array_equal(ys.numpy(), gold["ys"]) and np.array_equal(xs.numpy(), gold["xs"])
    dets, inds2, _ = odec.polydet_decode(heat, polys, depth, reg, K=K, rep=rep)
    assert np.array_equal(inds2.numpy(), gold["inds"])
    np.testing.assert_allclose(dets.numpy(), gold["dets"], rtol=1e-6, atol=1e-5)
    dets_nr, _, _ = odec.polydet_decode(heat, polys, depth, None, K=K, rep=rep)
    np.testing.assert_allclose(dets_nr.numpy(), gold["dets_noreg"], rtol=1e-6, atol=1e-5)
    if rep == "cartesian":                                        # no trig: bit-exact
        assert np.array_equal(dets.numpy(), gold["dets"])


@pytest.mark.gpu
@pytest.mark.parametrize("case", wide_cases.WIDE_DECODE_CASES, ids=lambda c: c[0])
def test_decode_kernel_matches_reference_at_64_vertices(case, golden):
    from centerpoly_amd.models.decode import polydet_decode
    name, B, C, h, w, N, K, rep = case
    gold = golden("decode_" + name)
    heat, polys, depth, reg = (g(a) for a in cases.decode_inputs_np(*case))
    for use_reg, key in ((True, "dets"), (False, "dets_noreg")):
        dets, inds, clses = polydet_decode(heat, polys, depth, reg=reg if use_reg else None, K=K, rep=rep,
                                           return_inds=True)
        assert np.array_equal(inds.cpu().numpy(), gold["inds"])
        assert np.array_equal(clses.cpu().numpy(), gold["clses"])
        np.testing.assert_allclose(dets.cpu().numpy(), gold[key], rtol=1e-6, atol=1e-5)
        if rep == "cartesian":
            assert np.array_equal(dets.cpu().numpy(), gold[key])


# ------------------------------------------------------------------------------------------------------- fused heads --
def _t(tag, shape, scale=1.0):
    return torch.from_numpy(synth.normal("widehf/" + tag, shape) * np.float32(scale)).to(DEV)


def _rel(a, ref):
    return (a.double() - ref).abs().max().item() / max(ref.abs().max().item(), 1e-30)


def _prepare_w2(L, w, co, hc):
    """The head's prepared 1x1 weights: one block of cp_heads_fused_w2_bytes per 64-row segment, back to back."""
    seg = L.cp_heads_fused_w2_bytes(hc)
    nseg = (co + 63) // 64
    buf = torch.empty(nseg * seg, dtype=torch.uint8, device=DEV)
    for s in range(nseg):
        _C.check(L.cp_heads_fused_prepare_w2(ctypes.c_void_p(w.data_ptr() + 4 * 64 * s * hc), min(64, co - 64 * s), hc,
                                             ctypes.c_void_p(buf.data_ptr() + s * seg), _C.stream()), "prepare_w2")
    return buf


def _fused_heads(L, x, wp1, b1, w2p, b2, couts, hc):
    B, cin, H, W = x.shape
    nh = len(couts)
    outs = [torch.full((B, co, H, W), float("nan"), device=DEV) for co in couts]
    vp = ctypes.c_void_p
    rc = L.cp_heads_fused_forward(P(x), P(wp1), P(b1), (vp * nh)(*[t.data_ptr() for t in w2p]),
                                  (vp * nh)(*[t.data_ptr() for t in b2]), (vp * nh)(*[t.data_ptr() for t in outs]),
                                  (ctypes.c_int32 * nh)(*couts), nh, B, cin, H, W, hc, _C.stream())
    return rc, outs


# (couts), head_conv, cin, H, W
WIDE_HEADS = [((8, 128, 1, 2), 256, 64, 40, 72), ((8, 96, 1, 2), 256, 64, 17, 33), ((8, 66, 1, 2), 64, 32, 9, 31),
              ((8, 128, 1, 2), 64, 256, 16, 64), ((128,), 64, 32, 8, 32), ((128, 128), 128, 96, 8, 40)]


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", WIDE_HEADS, ids=["dla heads N=64 (resident)", "N=48 unequal segments, ragged map",
                                                 "66: first width over 64", "hourglass heads (plain form)",
                                                 "one wide head alone", "two wide heads"])
def test_fused_heads_kernel_wide_heads(cfg):
    """cp_heads_fused_forward with heads of 65 .. 128 output channels against float64 torch: every output element
    written (NaN prefill), 2e-5 of the max-norm, a second call bit-identical."""
    couts, hc, cin, H, W = cfg
    L = _C.lib()
    B, nh = 2, len(couts)
    x = _t("x%s" % (cfg,), (B, cin, H, W))
    w1 = _t("w1%s" % (cfg,), (nh * hc, cin, 3, 3), 0.05)
    b1 = _t("b1%s" % (cfg,), (nh * hc,))
    w2 = [_t("w2_%d%s" % (i, cfg), (co, hc), 0.1) for i, co in enumerate(couts)]
    b2 = [_t("b2_%d%s" % (i, cfg), (co,)) for i, co in enumerate(couts)]
    wp1 = torch.empty(L.cp_conv_mfma_weight_bytes(cin, nh * hc, 9), dtype=torch.uint8, device=DEV)
    _C.check(L.cp_conv_mfma_prepare(P(w1), cin, nh * hc, 9, 0, P(wp1), _C.stream()), "prepare")
    w2p = [_prepare_w2(L, w, co, hc) for w, co in zip(w2, couts)]
    rc, outs = _fused_heads(L, x, wp1, b1, w2p, b2, couts, hc)
    assert rc == 0
    hid = F.relu(F.conv2d(x.double(), w1.double(), b1.double(), padding=1))
    for i, co in enumerate(couts):
        ref = F.conv2d(hid[:, i * hc:(i + 1) * hc], w2[i].double().view(co, hc, 1, 1), b2[i].double())
        err = _rel(outs[i], ref)
        print("head %d (%d channels): %.3g of the max-norm" % (i, co, err))
        assert torch.isfinite(outs[i]).all() and err <= TOL, i
    rc, again = _fused_heads(L, x, wp1, b1, w2p, b2, couts, hc)
    assert rc == 0 and all(torch.equal(a, b) for a, b in zip(outs, again))


@pytest.mark.gpu
def test_fused_heads_kernel_refuses_129_channels():
    L = _C.lib()
    couts, hc, cin, H, W = (8, 129), 64, 32, 8, 32
    x, b1 = _t("rx", (1, cin, H, W)), _t("rb1", (2 * hc,))
    w1 = _t("rw1", (2 * hc, cin, 3, 3), 0.05)
    wp1 = torch.empty(L.cp_conv_mfma_weight_bytes(cin, 2 * hc, 9), dtype=torch.uint8, device=DEV)
    _C.check(L.cp_conv_mfma_prepare(P(w1), cin, 2 * hc, 9, 0, P(wp1), _C.stream()), "prepare")
    w2p = [torch.zeros(3 * L.cp_heads_fused_w2_bytes(hc), dtype=torch.uint8, device=DEV) for _ in couts]
    b2 = [torch.zeros(co, device=DEV) for co in couts]
    rc, outs = _fused_heads(L, x, wp1, b1, w2p, b2, couts, hc)
    torch.cuda.synchronize()
    assert rc == -2                                               # CP_EUNSUPPORTED, before any device work
    assert all(torch.isnan(o).all() for o in outs)


# ------------------------------------------------------------------------------------------------------------ models --
HEADS64 = {"hm": 8, "poly": 128, "pseudo_depth": 1, "reg": 2}


def _count_fused(monkeypatch):
    from centerpoly_amd.models.networks import pose_dla_dcn
    real, calls = pose_dla_dcn.heads_fused_infer, []

    def counted(*a, **kw):
        out = real(*a, **kw)
        calls.append(out)
        return out
    monkeypatch.setattr(pose_dla_dcn, "heads_fused_infer", counted)
    return calls


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["dla_34", "hourglass1"])
def test_models_run_the_64_vertex_heads_in_the_fused_launch(kind, monkeypatch):
    """prepare_inference() against plain eval at --nbr_points 64 (2e-4 of each head's max-norm, the bound of
    test_hourglass_prepare_inference_matches_plain_eval), and the heads really take the one-launch path:
    heads_fused_infer returns the outputs, not None."""
    if kind == "dla_34":
        from centerpoly_amd.models.model import create_model
        m, shape = create_model("dla_34", HEADS64, 256), (2, 3, 64, 96)
    else:
        from centerpoly_amd.models.networks.large_hourglass import HourglassNet
        m, shape = HourglassNet(HEADS64, 1), (2, 3, 128, 128)
    m.load_state_dict({k: T(v) for k, v in cases.fill_weights({k: tuple(v.shape) for k, v in m.state_dict().items()}).items()})
    m = m.to(DEV).eval()
    x = g(synth.normal("wide/model/x/" + kind, shape))
    with torch.no_grad():
        plain = m(x)
        m.prepare_inference()
        calls = _count_fused(monkeypatch)
        fused = m(x)
    assert len(plain) == len(fused) == 1
    for h in HEADS64:
        a, b = plain[0][h], fused[0][h]
        assert a.shape == b.shape and (a - b).abs().max().item() <= 2e-4 * a.abs().max().item(), h
    assert len(calls) == 1 and isinstance(calls[0], dict) and sorted(calls[0]) == sorted(HEADS64)


# -------------------------------------------------------------------------------------------------------- end to end --
@pytest.mark.gpu
def test_detector_runs_end_to_end_with_64_vertices():
    """PolydetDetector.run at --nbr_points 64 --K 128 on a 128 x 256 image: the result rows against the oracle's decode
    and post-process of the model's own head maps (as tests/test_detector_io.py checks the N = 16 path), then the rows
    through cp_writer_instances and cp_instance_masks on the image's own canvas."""
    from centerpoly_amd.detectors.detector_factory import detector_factory
    from centerpoly_amd.opts import opts
    N, K, C = 64, 128, 8
    opt = opts().init(["polydet", "--arch", "dla_34", "--nbr_points", str(N), "--K", str(K)])
    det = detector_factory["polydet"](opt)
    det.model.train()                                             # drops the prepared forms of the random weights
    sd = det.model.state_dict()
    det.model.load_state_dict({k: g(v) for k, v in cases.fill_weights({k: tuple(v.shape) for k, v in sd.items()}).items()})
    det.model.eval()
    det.model.prepare_inference()
    img = (synth.uniform("wide/e2e/img", (128, 256, 3)) * 255).astype(np.uint8)
    res = det.run(img)["results"]
    assert sorted(res) == list(range(1, C + 1))
    images, meta = det.pre_process(img, 1.0)
    with torch.no_grad():
        out = det.model(images)[-1]
        assert out["poly"].shape[1] == 2 * N
        hm = out["hm"].sigmoid().cpu()
    dref, _, _ = odec.polydet_decode(hm, out["poly"].cpu(), out["pseudo_depth"].cpu(), out["reg"].cpu(), K=K,
                                     rep="cartesian")
    ref = opost.merge_outputs([opost.detector_post_process(dref.numpy(), meta, 1.0, C)], C, K)
    assert sum(len(v) for v in res.values()) == K
    for j in range(1, C + 1):
        assert res[j].shape == ref[j].shape and res[j].shape[1] == 2 * N + 6
        np.testing.assert_allclose(res[j], ref[j], rtol=1e-4, atol=2e-3)

    # the result writer's device path on those rows
    rows = det.device_rows()
    assert tuple(rows.shape) == (K, 2 * N + 7)
    scores = np.sort(det.host_rows()[:, 4])[::-1]
    thresh = float(scores[8])                                     # rows with score > thresh: the (up to) 8 best
    live = int((det.host_rows()[:, 4] > np.float32(thresh)).sum())
    assert 1 <= live <= 8
    L = _C.lib()
    H, W = img.shape[:2]
    table = np.ascontiguousarray(np.array([[24 + c, 1] for c in range(C)], np.int32))      # every class has masks
    n_out = torch.zeros(1, dtype=torch.int32, device=DEV)
    src, label = (torch.empty(K, dtype=torch.int32, device=DEV) for _ in range(2))
    poly = torch.empty((K, N, 2), dtype=torch.int32, device=DEV)
    flags = torch.empty(K, dtype=torch.uint8, device=DEV)
    conf = torch.empty(K, dtype=torch.float32, device=DEV)
    rc = L.cp_writer_instances(P(rows), K, N, thresh, table.ctypes.data_as(ctypes.c_void_p), C, P(n_out), P(src), P(poly),
                               P(flags), P(label), P(conf), _C.stream())
    assert rc == 0
    masks = torch.empty((K, H, W), dtype=torch.uint8, device=DEV)
    counts = torch.empty(K, dtype=torch.int32, device=DEV)
    rc = L.cp_instance_masks(P(poly), P(flags), K, N, H, W, P(masks), P(counts), _C.stream())
    assert rc == 0
    n, cnt = int(n_out.item()), counts.cpu().numpy()
    print("live rows %d, pixel counts %s" % (n, cnt[:n].tolist()))
    assert n == live
    assert np.array_equal(cnt, masks.view(K, -1).ne(0).sum(1).cpu().numpy())
    # a live instance's own drawing is non-empty unless nearer confident instances (drawn before it) hide all of it or it
    # lies off the canvas: the nearest one (slot 0) has nothing in front of it, and dead slots draw nothing
    assert (cnt[n:] == 0).all() and cnt[:n].sum() > 0
    p0 = poly[0].cpu().numpy()
    if ((p0[:, 0] >= 0) & (p0[:, 0] < W) & (p0[:, 1] >= 0) & (p0[:, 1] < H)).any():
        assert cnt[0] > 0


# ---------------------------------------------------------------------------------------------------------- training --
@pytest.mark.gpu
def test_trainer_step_at_64_vertices_matches_oracle_losses():
    """PolydetTrainer's losses at --arch smallhourglass --nbr_points 64 --poly_loss l1+iou on a 2 x 128 x 128 batch
    against oracle.losses at 1e-3 (the bound of test_trainer_step_matches_oracle_losses), finite gradients for every
    parameter.  BatchNorm runs on its running statistics, as in test_trainer_hourglass_polar_two_stacks: at 128 x 128
    the Hourglass's deepest level is 1 x 1 and batch statistics over two values make the forward pass chaotic."""
    from centerpoly_amd.models.model import create_model
    from centerpoly_amd.opts import opts
    from centerpoly_amd.trains.train_factory import train_factory
    N = 64
    opt = opts().init(["polydet", "--arch", "smallhourglass", "--nbr_points", str(N), "--poly_loss", "l1+iou"])
    opt.device = torch.device(DEV)
    model = create_model(opt.arch, opt.heads, opt.head_conv)
    assert opt.heads["poly"] == 2 * N
    model.load_state_dict({k: T(v) for k, v in
                           cases.fill_weights({k: tuple(v.shape) for k, v in model.state_dict().items()}).items()})
    trainer = train_factory["polydet"](opt, model, torch.optim.Adam(model.parameters(), opt.lr))
    trainer.set_device(opt.gpus, opt.chunk_sizes, opt.device)
    nb = synth.train_batch(2, 32, 32, nbr_points=N, rep="cartesian", mean_objs=5, in_h=128, in_w=128,
                           stream="trainer/wide64")
    batch = {k: g(v) for k, v in nb.items()}
    model.eval()
    with torch.no_grad():
        outs = [{k: v.clone().cpu() for k, v in o.items()} for o in model(batch["input"])]
    with torch.enable_grad():
        out, loss, stats = trainer.model_with_loss(batch)
        loss.backward()
    ref, rstats = olos.polydet_loss(outs, {k: T(v) for k, v in nb.items()}, num_stacks=1, poly_loss_kind="l1+iou",
                                    rep="cartesian", poly_order=False)
    for k in rstats:
        print("%s: %.7g (oracle %.7g)" % (k, float(stats[k]), float(rstats[k])))
        np.testing.assert_allclose(float(stats[k]), float(rstats[k]), rtol=1e-3, atol=1e-5, err_msg=k)
    for k, v in model.named_parameters():
        assert v.grad is not None and torch.isfinite(v.grad).all(), k

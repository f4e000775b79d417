"""GPU parity of the fused DLA base (csrc/conv_base_trio.hip): base_layer 7x7 + level0 + level1 in one launch.

The yardstick is the route it replaces, bit for bit: cp_conv7x7_c3_forward (stride 1, ReLU) followed by
cp_dla_base_pair_forward on the same tensors.  A float64 torch chain bounds the arithmetic: three chained split-bf16
contractions, one TOL of test_conv_mfma.py each (the pair test allows 2 * TOL for two)."""
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


def _rel(a, ref):
    return (a.double() - ref).abs().max().item() / max(ref.abs().max().item(), 1e-30)


def _run_rows(B, H, W):
    """The kernel's run-length rule (cp_dla_base_trio_forward): a strip of 32 y1 columns is cut into as many vertical runs
    as give each of 256 workgroups one, but into at most ceil(Ho / 32) runs, each an even number of rows."""
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    columns = ((Wo + 31) // 32) * B
    nruns = min((256 + columns - 1) // columns, (Ho + 31) // 32)
    rows = (Ho + nruns - 1) // nruns
    return rows + (rows & 1)


# (B, H, W).  The last one is the run boundary: by _run_rows a 200-row image (100 y1 rows, 2 strips) is cut into 4 runs of
# 26 y1 rows, so runs start at y1 rows 26, 52 and 78, inside the image, and the last run (22 rows) is shorter.
# (2, 130, 72) has 3 runs of 22 rows; its last step holds the single row 64.
SHAPES = [(1, 1, 4), (1, 5, 8), (1, 8, 36), (2, 37, 100), (1, 7, 132), (2, 130, 72), (1, 200, 72)]


def test_the_run_boundary_shape_spans_several_runs():
    assert _run_rows(1, 200, 72) == 26 and _run_rows(2, 130, 72) == 22
    assert _run_rows(1, 1024, 2048) == 64 and _run_rows(4, 512, 1024) == 64


def _weights():
    ws, bs = _t("triows", (16, 3, 7, 7), 0.1), _t("triobs", (16,), 0.2)
    w0, b0 = _t("pairw0", (16, 16, 3, 3), 0.1), _t("pairb0", (16,), 0.2)
    w1, b1 = _t("pairw1", (32, 16, 3, 3), 0.1), _t("pairb1", (32,), 0.2)
    L = _C.lib()
    wp = torch.empty(L.cp_conv7x7_c3_weight_bytes(16), dtype=torch.uint8, device=DEV)
    _C.check(L.cp_conv7x7_c3_prepare(P(ws), 16, P(wp), _C.stream()), "prepare")
    return ws, bs, w0, b0, w1, b1, wp


def _ref64(x, ws, bs, w0, b0, w1, b1):
    d = lambda t: None if t is None else t.double()
    s = F.relu(F.conv2d(x.double(), ws.double(), d(bs), padding=3))
    return F.relu(F.conv2d(F.relu(F.conv2d(s, w0.double(), d(b0), padding=1)), w1.double(), d(b1), stride=2, padding=1))


@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_base_trio_kernel_has_the_bits_of_stem_then_pair(shape):
    """(a) torch.equal to stem + pair, (b) <= 3 * TOL of the max-norm against float64, (c) a second call repeats the
    first, (d) the same without biases.  Measured against float64 on an MI355X: see DESIGN 4.10c."""
    B, H, W = shape
    L = _C.lib()
    x = _t("triox%s" % (shape,), (B, 3, H, W))
    ws, bs, w0, b0, w1, b1, wp = _weights()
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    assert L.cp_dla_base_trio_supported(H, W)
    out = torch.full((B, 32, Ho, Wo), float("nan"), device=DEV)
    _C.check(L.cp_dla_base_trio_forward(P(x), P(wp), P(bs), P(w0), P(b0), P(w1), P(b1), P(out), B, H, W, _C.stream()), "trio")
    assert torch.isfinite(out).all()                                # every output element was written
    s = torch.full((B, 16, H, W), float("nan"), device=DEV)
    _C.check(L.cp_conv7x7_c3_forward(P(x), P(wp), P(bs), P(s), B, H, W, 16, 1, 1, _C.stream()), "stem")
    y1 = torch.full((B, 32, Ho, Wo), float("nan"), device=DEV)
    _C.check(L.cp_dla_base_pair_forward(P(s), P(w0), P(b0), P(w1), P(b1), P(y1), B, H, W, _C.stream()), "pair")
    assert torch.equal(out, y1)                                     # (a)
    err = _rel(out, _ref64(x, ws, bs, w0, b0, w1, b1))
    print("trio %s: %.3e of the max-norm against float64" % (shape, err))
    assert err <= 3 * TOL                                           # (b)
    out2 = torch.full_like(out, float("nan"))
    _C.check(L.cp_dla_base_trio_forward(P(x), P(wp), P(bs), P(w0), P(b0), P(w1), P(b1), P(out2), B, H, W, _C.stream()), "trio")
    assert torch.equal(out, out2)                                   # (c)
    out2.fill_(float("nan"))
    _C.check(L.cp_dla_base_trio_forward(P(x), P(wp), None, P(w0), None, P(w1), None, P(out2), B, H, W, _C.stream()), "trio")
    assert torch.isfinite(out2).all()
    err0 = _rel(out2, _ref64(x, ws, None, w0, None, w1, None))
    print("trio %s without biases: %.3e" % (shape, err0))
    assert err0 <= 3 * TOL                                          # (d)


def test_base_trio_kernel_refuses_widths_it_does_not_cover():
    L = _C.lib()
    assert L.cp_dla_base_trio_supported(16, 30) == 0
    x = _t("triorx", (1, 3, 16, 30))
    ws, bs, w0, b0, w1, b1, wp = _weights()
    out = torch.full((1, 32, 8, 15), float("nan"), device=DEV)
    assert L.cp_dla_base_trio_forward(P(x), P(wp), None, P(w0), None, P(w1), None, P(out), 1, 16, 30, _C.stream()) == -2
    torch.cuda.synchronize()
    assert torch.isnan(out).all()                                   # nothing written


def test_base_trio_host_argument_checks():
    """Null pointers and a batch of zero return the argument-error code before any launch (no device memory is named)."""
    L = _C.lib()
    one = ctypes.c_void_p(16)
    assert L.cp_dla_base_trio_supported(1024, 2048) == 1 and L.cp_dla_base_trio_supported(37, 100) == 1
    assert L.cp_dla_base_trio_supported(0, 64) == 0 and L.cp_dla_base_trio_supported(16384, 16384) == 0
    assert L.cp_dla_base_trio_forward(None, None, None, None, None, None, None, None, 1, 64, 64, None) == -1
    for hole in (0, 1, 3, 5, 7):                                    # image, stem weights, w0, w1, out
        args = [one] * 8
        args[hole] = None
        assert L.cp_dla_base_trio_forward(*args, 1, 64, 64, None) == -1
    assert L.cp_dla_base_trio_forward(*([one] * 8), 0, 64, 64, None) == -1


HEADS = {"hm": 8, "poly": 32, "pseudo_depth": 1, "reg": 2}
_MODEL = []


def _dla34():
    """One dla_34 DLASeg after prepare_inference, shared by the module-level tests (they only run it forward)."""
    if not _MODEL:
        from centerpoly_amd.models.model import create_model
        model = create_model("dla_34", HEADS, 256)
        shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
        model.load_state_dict({k: torch.from_numpy(v) for k, v in synth.fill_by_name(shapes).items()})
        model = model.to(DEV).eval()
        model.prepare_inference()
        _MODEL.append(model)
    return _MODEL[0]


def test_a_refused_launch_leaves_no_open_kernel_timer_record():
    """cp_dla_base_trio_forward refuses (-2) an image that is not 16-byte aligned, before any launch: _base_trio then
    returns None for the caller's stem + pair route and takes back the event pair it opened, so KernelTimer.summary()
    meets no pair whose end was never recorded."""
    from centerpoly_amd.models.networks import pose_dla_dcn
    dla = _dla34().base
    x = _t("triomis", (1 + 3 * 64 * 96,))[1:].view(1, 3, 64, 96)      # contiguous, 4 bytes off the allocation's alignment
    assert x.is_contiguous() and x.data_ptr() % 16 == 4
    saved, saved_timer = pose_dla_dcn.BASE_TRIO, _C.kernel_timer
    try:
        pose_dla_dcn.BASE_TRIO = "auto"
        _C.kernel_timer = _C.KernelTimer()
        with torch.no_grad():
            assert pose_dla_dcn._base_trio(dla, x) is None
        assert _C.kernel_timer.records == {} and _C.kernel_timer.summary() == {}
    finally:
        pose_dla_dcn.BASE_TRIO, _C.kernel_timer = saved, saved_timer


@pytest.mark.parametrize("size", [(1, 64, 96), (2, 64, 96)], ids=["1x64x96", "2x64x96"])
def test_dla34_heads_are_the_same_bits_with_and_without_the_trio(size):
    """(g) DLASeg dla_34 after prepare_inference: every head map with BASE_TRIO = auto equals the one with BASE_TRIO = off;
    the kernel-timer keys show one trio launch per forward, and the pair launch (fed by the stem launch) when it is off.
    At this input the deepest maps are 2 x 3: their convolutions are below the MFMA kernel's gate and go to the vendor
    library, whose default algorithm choice sums in an order that changes from call to call (two BASE_TRIO = off forwards
    differed by 7e-7 in every head), so the library is asked for its reproducible algorithms for the duration, as
    BaseDetector.run does.  2 x 3 x 64 x 96 stands in for the issue's 2 x 3 x 40 x 72: it is there for batch 2 through
    DLA.forward's routed path, and 40 is not a multiple of the network's stride of 32 -- at level4 the max-pooled skip
    of the 5 x 9 map is 2 x 4 and the stride-2 convolution's output 3 x 5 (the reference raises a size mismatch there),
    and the stem + pair route (BASE_TRIO = off, nothing of the fused launch in it) met a GPU memory fault inside the
    backbone at that input, so no route can run it; the fused kernel's own ragged-edge cases are the kernel tests
    above."""
    from centerpoly_amd.models.networks import pose_dla_dcn
    heads, model = HEADS, _dla34()
    x = _t("trionet%s" % (size,), (size[0], 3, size[1], size[2]))
    outs, keys = {}, {}
    saved, saved_timer, saved_det = pose_dla_dcn.BASE_TRIO, _C.kernel_timer, torch.backends.cudnn.deterministic
    try:
        torch.backends.cudnn.deterministic = True
        for mode in ("auto", "off"):
            pose_dla_dcn.BASE_TRIO = mode
            _C.kernel_timer = _C.KernelTimer()
            with torch.no_grad():
                outs[mode] = {k: v.clone() for k, v in model(x)[-1].items()}
            keys[mode] = {}
            for key, evs in _C.kernel_timer.records.items():
                keys[mode][key[0]] = keys[mode].get(key[0], 0) + len(evs)
    finally:
        pose_dla_dcn.BASE_TRIO, _C.kernel_timer = saved, saved_timer
        torch.backends.cudnn.deterministic = saved_det
    assert keys["auto"].get("conv_base_trio", 0) == 1 and "conv_base_pair" not in keys["auto"]
    assert keys["off"].get("conv_base_pair", 0) == 1 and "conv_base_trio" not in keys["off"]
    for h in heads:
        assert torch.isfinite(outs["auto"][h]).all()
        assert torch.equal(outs["auto"][h], outs["off"][h]), h

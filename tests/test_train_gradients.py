"""Whole-network training gradients on the device against a float64 reference ("Whole-network gradients").

The step is model.train(), one forward, L = sum(head * cotangent) with fixed synth cotangents, backward().  The
reference is the oracle network (oracle/nets.py) in float64 with train-mode BatchNorm, and it REPLAYS THE DEVICE'S OWN
DISCRETE DECISIONS: every ReLU gate and every 2x2 pool winner is taken from the device's forward (recorded here by
wrapping pose_dla_dcn.bn_act / downsample2 / conv_bias_relu and reading the fused heads node's saved activations --
no product code is changed).  Without that a handful of gates fall differently in float32 and float64 and every
parameter tensor differs by ~1.4e-2 relative L2 whatever the implementation; with it the reference is the gradient of
exactly the function the device backward differentiates, and a faithful float32 implementation agrees to ~1e-5.

DCN sampling cells cannot be observed from outside the fused module, so the network cases fix them by construction:
conv_offset_mask.weight = 0 makes offsets and masks constants (exact in float32 and float64), once with bias 0 (the
state every training run starts in) and once with 18 different non-integer multiples of 1/8 in (-2, 2) and masks
spread over sigmoid([-1, 1]).  The gradient of conv_offset_mask.weight is non-zero in both and is checked (grad_offset,
grad_mask, the offset convolution's weight gradient).  Spatially varying offsets stay with the per-kernel test
(test_gpu_parity.py::test_dcn_backward_vs_oracle_autograd).

Bound rule, per parameter tensor k with requires_grad:  e_k = ||g_dev - g_ref||2 / ||g_ref||2  must satisfy
    e_k <= m * max(f_k, median f)   and never more than 1e-3,
where f_k is the same figure for the CPU float32 oracle against the float64 oracle replaying the float32 run's own
decisions (reference only; DLA: max 3.4e-5, median 8.2e-6).  m = 4 for exact_f32: the same arithmetic in another
summation order.  m = 32 for split_bf16, whose products carry ~2^-17 instead of 2^-24: 16 does not hold for the
number format itself -- the same CPU float32 oracle with its convolutions' forward and both gradients contracted as
ah*bh + ah*bl + al*bh against its gate-forced float64 run gives 21 .. 24 x the plain floor at the median of the
three cases -- and 32 is the next power of two above that.  The device measures 12 x at the median and
at most 21 x on single tensors.
A second figure guards what the wider split_bf16 bound would hide: on the tensors of >= 65536 elements the coherent
part beta_k = <g_dev - g_ref, g_ref> / ||g_ref||^2 must stay within (m / 4) * max(4 * the largest |beta| of the floor
run, median f): noise leaves ~e / sqrt(elements) there, a wrong factor on one path stays whole.  (The clamp at median
f, a quarter of the smallest e_k bound, is there because the largest of 40 signed noise figures from one float32 run
is itself uncertain: exact_f32 measures 2.5e-6 .. 2.8e-6 on the offset convolution of the 4x5 map against
4 * 6.4e-7 from the floor run.)
The 16 DCN conv.bias tensors sit in front of a train-mode BatchNorm (gradient analytically zero): ||g_dev|| is
measured against ||g_ref|| of the following actf.0.bias, with the bound from the floor run's own ratio by the same
rule.  The same bounds hold for the accumulated gradient of two backward passes and for the gradient after one SGD
step (prepared weights refreshed, BatchNorm counters at 2, zero-pool buffers reused).  That step updates every
trainable tensor in the k/8 case (offsets then vary by ~1e-5 px, far from any cell border) and leaves conv_offset_mask.*
alone in the zero-offset case, where every sampling position sits ON a cell border: float32 positions (ulp 4e-6 at
row 40) round a tiny negative offset away and land in the neighbouring cell of the float64 ones, in any implementation.  Measured e_k per parameter
family: the table in DESIGN.md, "Whole-network gradients"; on the MI355X, DLA-34 with zero offsets, step 1, max / median:
    family                    exact_f32            split_bf16
    conv weight               2.3e-5 / 7.9e-6      2.8e-4 / 1.0e-4
    bn weight, bias           2.5e-5 / 8.3e-6      3.4e-4 / 1.0e-4
    root conv weight          2.1e-5 / 9.0e-6      2.6e-4 / 1.1e-4
    root bn weight, bias      2.4e-5 / 9.8e-6      2.8e-4 / 1.3e-4
    project conv, bn          1.8e-5 / 8.3e-6      2.3e-4 / 1.0e-4
    dcn weight                2.4e-5 / 1.2e-5      3.0e-4 / 1.5e-4
    dcn offset conv weight    3.3e-5 / 1.7e-5      4.2e-4 / 2.0e-4
    dcn offset conv bias      3.0e-5 / 1.3e-5      4.5e-4 / 1.4e-4
    dcn bn weight             2.2e-5 / 1.2e-5      2.7e-4 / 1.7e-4
    dcn bn bias               3.7e-6 / 1.6e-6      4.9e-5 / 2.3e-5
    dcn bias (zero)           1.4e-6 / 7.2e-7      1.3e-6 / 6.6e-7
    up weight                 2.4e-5 / 1.5e-5      2.9e-4 / 1.9e-4
    head 3x3 weight           1.5e-5 / 1.3e-5      1.8e-4 / 1.6e-4
    head 1x1 weight           1.5e-5 / 1.1e-5      1.8e-4 / 1.4e-4
    head biases               <= 1.4e-7            <= 4.5e-6
    all tensors               3.3e-5 / 8.1e-6      4.5e-4 / 1.0e-4   (offsets k/8: 3.1e-5 / 7.0e-6, 3.6e-4 / 9.9e-5;
                                                                      Hourglass: 5.0e-5 / 2.0e-5, 5.1e-4 / 2.0e-4)

Hourglass-small (one stack) runs in train mode at 2x3x256x256, the smallest input whose reference-only floor stays
<= 1e-4 on every tensor (max 3.3e-5): at 2x3x128x128 the deepest level is 1x1 (two values per BatchNorm channel) and
the floor is O(1), at 2x3x128x256 it is 9e-4.  It has no pooling; its gates are the BatchNorm sites of
large_hourglass.py and the heads' bias+ReLU convolutions (forward hooks).
"""
import collections

import numpy as np
import pytest
import torch

import train_grad_ref as R
from centerpoly_amd import arithmetic

pytestmark = pytest.mark.gpu
T = torch.from_numpy
DEV = "cuda"
MODES = ("exact_f32", "split_bf16")
M = {"exact_f32": 4.0, "split_bf16": 32.0}         # see the bound rule above

CASES = {
    # name: (arch, input shape, DCN regime, train-mode BatchNorm)
    "dla_zero": ("dla_34", (2, 3, 128, 160), "zero", True),
    "dla_eighths": ("dla_34", (2, 3, 128, 160), "eighths", True),
    "hourglass": ("smallhourglass", (2, 3, 256, 256), None, True),
}


class _Recorder(object):
    """The device forward's discrete decisions in the oracle's tape format, and which fused paths ran."""

    def __init__(self, model, mp):
        from centerpoly_amd.models.networks import conv3x3, large_hourglass, pose_dla_dcn
        self.names = {id(m): n for n, m in model.named_modules()}
        self.tape, self.paths, self.hooks = {}, collections.Counter(), []
        bn_act, downsample2, conv_bias_relu = pose_dla_dcn.bn_act, pose_dla_dcn.downsample2, pose_dla_dcn.conv_bias_relu
        heads_train, concat, raw_skip = conv3x3.heads_train, conv3x3.concat_conv1x1, conv3x3.conv_raw_skip

        def rec_bn_act(bn, x, relu=True, residual=None):
            y = bn_act(bn, x, relu=relu, residual=residual)
            if relu:
                self.tape[self.names[id(bn)]] = (y.detach() > 0).cpu()
            if y.grad_fn is None:                       # under no_grad: the dead Tree.project branches (statistics only)
                self.paths["bn_no_grad"] += 1
            else:
                self.paths["bn_act" if "BnAct" in type(y.grad_fn).__name__ else "bn_torch"] += 1
            return y

        def rec_downsample2(pool, x):
            # torch's winners on the device's own input: the tie rule cp_maxpool2x2_backward documents
            k = pool.kernel_size if isinstance(pool.kernel_size, int) else pool.kernel_size[0]
            idx = torch.nn.functional.max_pool2d(x.detach(), k, k, return_indices=True)[1]
            self.tape[self.names[id(pool)]] = idx.cpu()
            y = downsample2(pool, x)
            self.paths["maxpool_fn" if "MaxPool2x2Fn" in type(y.grad_fn).__name__ else "maxpool_torch"] += 1
            return y

        def rec_conv_bias_relu(conv, x):
            y = conv_bias_relu(conv, x)
            self.tape[self.names[id(conv)]] = (y.detach() > 0).cpu()
            return y

        def rec_heads_train(fcs, x):
            outs = heads_train(fcs, x)
            if outs is not None:                        # _HeadsFn saved (x, then w1, w2, y per head)
                saved = outs[0].grad_fn.saved_tensors
                assert len(saved) == 1 + 3 * len(fcs)
                for h, fc in enumerate(fcs):
                    y = saved[3 + 3 * h]
                    assert y.shape[1] == fc[0].out_channels and y.shape[2:] == x.shape[2:]
                    self.tape[self.names[id(fc[0])]] = (y.detach() > 0).cpu()
                self.paths["heads_fn"] += 1
            return outs

        def rec_concat(conv, xs):
            y = concat(conv, xs)
            self.paths["concat_conv1x1" if y is not None else "concat_none"] += 1
            return y

        def rec_raw_skip(conv, x):
            pair = raw_skip(conv, x)
            self.paths["conv_raw_skip" if pair is not None else "raw_skip_none"] += 1
            return pair

        mp.setattr(pose_dla_dcn, "bn_act", rec_bn_act)
        mp.setattr(large_hourglass, "bn_act", rec_bn_act)
        mp.setattr(pose_dla_dcn, "downsample2", rec_downsample2)
        mp.setattr(pose_dla_dcn, "conv_bias_relu", rec_conv_bias_relu)
        mp.setattr(conv3x3, "heads_train", rec_heads_train)
        mp.setattr(conv3x3, "concat_conv1x1", rec_concat)
        mp.setattr(conv3x3, "conv_raw_skip", rec_raw_skip)
        for n, m in model.named_modules():              # Hourglass heads: convolution(with_bn=False) = conv + bias + ReLU
            if isinstance(m, large_hourglass.convolution) and not isinstance(m.bn, torch.nn.BatchNorm2d):
                self.hooks.append(m.register_forward_hook(
                    lambda mod, args, y, key=n + ".conv": self.tape.__setitem__(key, (y.detach() > 0).cpu())))

    def take(self):
        tape, self.tape = self.tape, {}
        return tape

    def close(self):
        for h in self.hooks:
            h.remove()


def _grads(model):
    return {k: v.grad.detach().clone().cpu() for k, v in model.named_parameters() if v.requires_grad}


def _counters(model):
    return {k: int(v) for k, v in model.named_buffers() if k.endswith("num_batches_tracked")}


def _loss(out, cot):
    return sum((out[h] * T(cot[h]).to(out[h].device)).sum() for h in R.HEADS)


def _device_steps(case):
    """Step 1 (forward, backward with cotangent 0, a second backward with cotangent 1 on top), one SGD step of ~1 % of
    the weights' norm with the trainer's weight-bank refresh, step 2 (forward, backward with cotangent 0).
    case.hold_offsets: the step leaves conv_offset_mask.* where they are (zero offsets, see the module docstring)."""
    from centerpoly_amd.models.model import create_model
    from centerpoly_amd.models.networks import conv3x3
    d = {}
    with pytest.MonkeyPatch.context() as mp:
        model = create_model(case.arch, dict(R.HEADS), case.head_conv)
        model.load_state_dict(case.state_dict())
        model = model.to(DEV)
        model.train(case.bn_train)
        d["requires_grad"] = {k: v.requires_grad for k, v in model.named_parameters()}
        rec = _Recorder(model, mp)
        try:
            x = T(case.x).to(DEV)
            out = model(x)[-1]
            d["tape1"] = rec.take()
            d["counters1"] = _counters(model)                       # read directly after the forward ...
            sd = model.state_dict()                                 # ... and through state_dict()
            d["sd1"] = {k: v.detach().clone().cpu() for k, v in sd.items()}
            _loss(out, case.cots[0]).backward(retain_graph=True)
            d["g1"] = _grads(model)
            _loss(out, case.cots[1]).backward()                     # no zero_grad: accumulates
            d["g12"] = _grads(model)
            del out
            params = [v for k, v in model.named_parameters()
                      if v.requires_grad and not (case.hold_offsets and ".conv_offset_mask." in k)]
            wn = torch.sqrt(sum((v.detach().double() ** 2).sum() for v in params))
            gn = torch.sqrt(sum((v.grad.double() ** 2).sum() for v in params))
            optim = torch.optim.SGD(params, lr=float(0.01 * wn / gn))
            optim.step()
            conv3x3.refresh_weight_bank()                           # what the trainer does after optimizer.step()
            model.zero_grad(set_to_none=True)                       # (the held offset convolutions included)
            d["sd_step"] = {k: v.detach().clone().cpu() for k, v in model.state_dict().items()}
            d["moved"] = float(torch.sqrt(sum(((d["sd_step"][k].double() - d["sd1"][k].double()) ** 2).sum()
                                              for k in d["g1"])) / wn.cpu())
            d["held"] = [k for k in d["g1"] if torch.equal(d["sd_step"][k], d["sd1"][k])]
            out = model(x)[-1]
            d["tape2"] = rec.take()
            d["counters2"] = _counters(model)
            d["sd2"] = {k: v.detach().clone().cpu() for k, v in model.state_dict().items()}
            _loss(out, case.cots[0]).backward()
            d["g2"] = _grads(model)
            d["paths"] = dict(rec.paths)
            torch.cuda.synchronize()
        finally:
            rec.close()
    return d


_CASES, _FLOORS = {}, {}


def _case(name):
    if name not in _CASES:
        arch, shape, regime, bn_train = CASES[name]
        _CASES[name] = R.Case(name, arch, shape, regime, bn_train)
    return _CASES[name]


def _floor(name):
    if name not in _FLOORS:
        _FLOORS[name] = R.floor(_case(name))
    return _FLOORS[name]


def _report(tag, e, bound, case):
    worst = max(e, key=lambda k: e[k] / bound[k])
    print("\n[%s] e_k max %.3g median %.3g; worst against its bound: %s %.3g (bound %.3g)"
          % (tag, max(e.values()), float(np.median(list(e.values()))), worst, e[worst], bound[worst]))
    for fam, (mx, md, n) in R.by_family(e, case).items():
        print("    %-26s n=%3d  max %.3g  median %.3g" % (fam, n, mx, md))


def _check(tag, run, grads, ref):
    case, bound = run["case"], run["bound"]
    e = R.errors(grads, ref, case.bn_train)
    _report(tag, e, bound, case)
    sc = R.scale_errors(grads, ref)
    worst = max(sc, key=lambda k: abs(sc[k]))
    print("    coherent scale error on the %d tensors of >= %d elements: max |beta| %.3g (%s), bound %.3g"
          % (len(sc), R.BIG, abs(sc[worst]), worst, run["scale_bound"]))
    assert set(e) == set(bound) and len(sc) >= 20
    assert max(bound.values()) <= 1e-3
    bad = {k: (e[k], bound[k]) for k in e if not e[k] <= bound[k]}
    assert not bad, "%s: %d of %d tensors over their bound: %s" % (
        tag, len(bad), len(e), sorted(bad.items(), key=lambda kv: -kv[1][0] / kv[1][1])[:8])
    bad = {k: v for k, v in sc.items() if not abs(v) <= run["scale_bound"]}
    assert not bad, "%s: coherent scale error over %.3g: %s" % (
        tag, run["scale_bound"], sorted(bad.items(), key=lambda kv: -abs(kv[1]))[:8])


@pytest.fixture(scope="module", params=[(c, m) for c in CASES for m in MODES], ids=lambda p: "%s-%s" % p)
def run(request):
    """Per case and arithmetic: the device's two steps, and the float64 references that replay their decisions
    (computed once; every test below only compares)."""
    name, mode = request.param
    case = _case(name)
    before = arithmetic.current()
    arithmetic.configure(mode)
    try:
        d = _device_steps(case)
    finally:
        arithmetic.configure(before)
    (r1, r2), run1 = R.oracle_gradients(case, case.state_dict(), case.cots, torch.float64, tape=d["tape1"])
    (s1,), run2 = R.oracle_gradients(case, d["sd_step"], case.cots[:1], torch.float64, tape=d["tape2"])
    r12 = {k: (r1[k] + r2[k] if r1[k] is not None else None) for k in r1}
    fl, m = _floor(name), M[mode]
    f = fl["e"]
    med = float(np.median(list(f.values())))
    d.update(name=name, mode=mode, case=case, ref1=r1, ref12=r12, ref_step2=s1, running1=run1, running2=run2,
             floor=f, bound=R.bounds(f, m),
             scale_bound=m / 4 * max(4 * max(abs(v) for v in fl["scale"].values()), med),
             running_bound=max(1e-5, m * max(fl["running"].values())))
    print("\n[%s %s] floor f_k max %.3g median %.3g, coherent part bound %.3g, running statistics bound %.3g; SGD step "
          "moved the weights by %.3g of their norm (%d tensors stood still, besides offset convolutions: %s); paths %s"
          % (name, mode, max(f.values()), med, d["scale_bound"], d["running_bound"], d["moved"], len(d["held"]),
             sorted(k for k in d["held"] if ".conv_offset_mask." not in k), d["paths"]))
    return d


def test_every_trainable_tensor_is_compared(run):
    """The reference reaches exactly the parameters the device trains: dead Tree.project branches stay
    requires_grad=False on the device and get no gradient in the reference."""
    live = {k for k, r in run["ref1"].items() if r is not None}
    assert live == set(run["g1"]) == {k for k, v in run["requires_grad"].items() if v}
    dead = {k for k, v in run["requires_grad"].items() if not v}
    assert all(".project." in k and k.startswith(("base.level3.", "base.level4.")) for k in dead), dead
    assert (len(dead) > 0) == (run["case"].arch == "dla_34")
    assert all(float(r.norm()) > 0 for k, r in run["ref1"].items() if r is not None)
    om = [k for k in live if k.endswith("conv_offset_mask.weight")]
    assert len(om) == (16 if run["case"].arch == "dla_34" else 0)


def test_fused_paths_ran(run):
    """split_bf16 must have gone through the nodes this file is about (a silent detour to the library would make the
    comparison pass without testing them)."""
    p = run["paths"]
    if run["case"].bn_train:
        assert p.get("bn_act", 0) > 0 and p.get("bn_torch", 0) == 0, p
    if run["case"].arch == "dla_34":
        assert p.get("maxpool_fn", 0) == 2 * 6 and p.get("maxpool_torch", 0) == 0, p
        if run["mode"] == "split_bf16":
            assert p.get("heads_fn", 0) == 2 and p.get("concat_conv1x1", 0) > 0 and p.get("conv_raw_skip", 0) > 0, p


def test_gradients_step1(run):
    _check("%s %s step 1" % (run["name"], run["mode"]), run, run["g1"], run["ref1"])


def test_gradients_accumulate(run):
    """Two backward passes with two cotangents and no zero_grad give g1 + g2."""
    _check("%s %s g1+g2" % (run["name"], run["mode"]), run, run["g12"], run["ref12"])


def test_gradients_after_sgd_step(run):
    """After one SGD step (~1 % of the weights' norm) and the trainer's weight-bank refresh, against the reference on
    the device's own state_dict: a stale prepared weight shows here."""
    assert 0.003 < run["moved"] < 0.03, run["moved"]
    held = {k for k in run["held"] if ".conv_offset_mask." in k}
    assert len(held) == (32 if run["case"].hold_offsets else 0), held
    # nothing else stands still, except analytically-zero DCN biases whose update is below their float32 resolution
    assert all(k in R.dcn_bias_keys(run["g1"]) for k in set(run["held"]) - held), run["held"]
    _check("%s %s step 2" % (run["name"], run["mode"]), run, run["g2"], run["ref_step2"])


def test_batchnorm_bookkeeping(run):
    """Running statistics equal the reference update after each forward; num_batches_tracked reads 1 then 2, directly
    after the forward and through state_dict() (the pending counters are flushed by the forward).

    The running statistics are compared in float32 against each tensor's max-norm: within 1e-5, or within m x the
    largest figure of the reference-only float32 floor where that is more (m as for the gradients: split_bf16, whose
    activations carry ~1e-5 themselves, 4.0e-5 for DLA and 1.4e-4 for Hourglass, measured 1.8e-5 and 8.6e-5; Hourglass
    in exact_f32, whose deepest level takes the variance of 8 values, 1.7e-5, measured 9.1e-6 .. 9.8e-6).  Element by
    element (rtol 1e-5, atol 0) is not a property of any float32 BatchNorm: torch's own CPU float32 BatchNorm on the
    Hourglass case differs from the float64 update by up to 3e-2 relative on means that lie near zero."""
    assert run["counters1"] and set(run["counters1"].values()) == {1}
    assert set(run["counters2"].values()) == {2}
    bound = run["running_bound"]
    for step, (sd, ref, n) in enumerate(((run["sd1"], run["running1"], 1), (run["sd2"], run["running2"], 2))):
        assert {k for k in sd if k.endswith(("running_mean", "running_var"))} == set(ref)
        for k, v in sd.items():
            if k.endswith("num_batches_tracked"):
                assert int(v) == n, k
        assert all(sd[k].dtype == torch.float32 for k in ref)
        r = R.running_errors(sd, ref)
        worst = max(r, key=r.get)
        print("\n[%s %s forward %d] running statistics: max %.3g of the tensor's max-norm (%s), bound %.3g"
              % (run["name"], run["mode"], step + 1, r[worst], worst, bound))
        bad = {k: v for k, v in r.items() if not v <= bound}
        assert not bad, sorted(bad.items(), key=lambda kv: -kv[1])[:8]

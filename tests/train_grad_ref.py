"""Helpers of tests/test_train_gradients.py: the cases, the gate-forced float64 reference and the reference-only floor.
TEST INFRASTRUCTURE, CPU only (the device side lives in the test file)."""
import numpy as np
import torch

import cases
from centerpoly_amd import synth
from oracle import nets as onet

HEADS = dict(cases.HEADS)
T = torch.from_numpy


def is_param(key):
    return not key.endswith(("running_mean", "running_var", "num_batches_tracked"))


def dcn_regime(w, regime):
    """Constant DCN offsets and masks: conv_offset_mask.weight = 0, so offset = bias[:18] (dy, dx interleaved) and
    mask = sigmoid(bias[18:]) at every pixel, exactly, in float32 and float64 alike.
      "zero"    bias 0 -- the state every real training run starts in (test_dcn_init_is_zero_offset);
      "eighths" 18 different offsets, non-integer multiples of 1/8 in (-2, 2) (a sampling position is then never
                within 1/8 of a cell border), mask biases spread over [-1, 1]."""
    steps = np.array([k for k in range(-15, 16) if k % 8 != 0], dtype=np.int64)            # 28 candidates
    for k in sorted(w):
        if k.endswith("conv_offset_mask.weight"):
            w[k] = np.zeros_like(w[k])
        elif k.endswith("conv_offset_mask.bias"):
            b = np.zeros_like(w[k])
            if regime == "eighths":
                order = np.argsort(synth.uniform("traingrad/offs/" + k, (len(steps),)), kind="stable")
                b[:18] = steps[order[:18]].astype(np.float32) / 8.0
                morder = np.argsort(synth.uniform("traingrad/mask/" + k, (9,)), kind="stable")
                b[18:] = np.linspace(-1.0, 1.0, 9, dtype=np.float32)[morder]
            else:
                assert regime == "zero"
            w[k] = b
    return w


class Case(object):
    """arch, input shape, weights (name -> float32 numpy), input and two cotangent sets from fixed synth streams."""

    def __init__(self, name, arch, shape, regime=None, bn_train=True):
        from centerpoly_amd.models.model import create_model
        self.name, self.arch, self.bn_train = name, arch, bn_train
        # zero offsets sit exactly on the cell borders: an SGD step must leave the offset convolutions alone there
        self.hold_offsets = regime == "zero"
        self.head_conv = 256 if arch == "dla_34" else 64
        model = create_model(arch, dict(HEADS), self.head_conv)
        shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
        self.requires_grad = {k: v.requires_grad for k, v in model.named_parameters()}
        w = cases.fill_weights(shapes)
        if regime is not None:
            w = dcn_regime(w, regime)
        self.weights = {k: np.ascontiguousarray(v) for k, v in w.items()}
        B, _, H, W = shape
        self.x = synth.normal("traingrad/%s/input" % name, shape)
        self.cots = [{h: synth.normal("traingrad/%s/cot%d/%s" % (name, i, h), (B, c, H // 4, W // 4))
                      for h, c in HEADS.items()} for i in range(2)]

    def state_dict(self):
        return {k: T(v.copy()) for k, v in self.weights.items()}

    def forward(self, sd, x, opt):
        if self.arch == "dla_34":
            return onet.dla_seg_forward(sd, x, HEADS, opt=opt)[0]
        return onet.hourglass_forward(sd, x, HEADS, 1, opt=opt)[0]


def oracle_gradients(case, sd, cots, dtype, tape=None, record=None):
    """One oracle forward in `dtype` (train-mode BatchNorm if the case says so; decisions replayed from `tape`,
    recorded into `record`), then one backward of sum(head * cotangent) per cotangent set.
    -> ([name -> gradient (float64, None where the loss does not depend on the parameter)] per set, running stats)."""
    sd = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}
    names = [k for k in sd if is_param(k)]
    for k in names:
        sd[k] = sd[k].clone().requires_grad_(True)
    opt = onet.Options(bn_train=case.bn_train, tape=tape, record=record)
    out = case.forward(sd, T(case.x).to(dtype), opt)
    grads = []
    for i, cot in enumerate(cots):
        loss = sum((out[h] * T(cot[h]).to(dtype)).sum() for h in HEADS)
        gs = torch.autograd.grad(loss, [sd[k] for k in names], allow_unused=True, retain_graph=i + 1 < len(cots))
        grads.append({k: (g.double() if g is not None else None) for k, g in zip(names, gs)})
    return grads, {k: v.detach() for k, v in opt.running.items()}


def rel_l2(g, ref):
    return float((g.double() - ref).norm() / ref.norm())


def dcn_bias_keys(names):
    """DCN `conv.bias` sits in front of a train-mode BatchNorm: its gradient is analytically zero, so it is measured
    against the gradient norm of the `actf.0.bias` that follows it.  -> {conv.bias key: actf.0.bias key}."""
    return {k: k[:-len("conv.bias")] + "actf.0.bias" for k in names
            if k.endswith(".conv.bias") and (k[:-len("conv.bias")] + "actf.0.bias") in names}


def errors(grads, ref, bn_train):
    """name -> the measured figure: ||g - g_ref|| / ||g_ref||, or for an analytically zero DCN bias ||g|| / ||g_ref of
    the following BatchNorm bias||.  Parameters the loss does not reach (dead Tree.project) are left out."""
    zero = dcn_bias_keys(ref) if bn_train else {}
    e = {}
    for k, r in ref.items():
        if r is None:
            continue
        if k in zero:
            e[k] = float(grads[k].double().norm() / ref[zero[k]].norm())
        else:
            e[k] = rel_l2(grads[k], r)
    return e


BIG = 65536


def scale_errors(grads, ref):
    """name -> <g - g_ref, g_ref> / ||g_ref||^2 for the tensors of at least BIG elements: the part of the error that
    is a coherent scale of the gradient.  Rounding noise of relative size e leaves ~e / sqrt(elements) here, a wrong
    factor on one of the paths into the tensor stays at full size."""
    return {k: float(((grads[k].double() - r) * r).sum() / (r * r).sum()) for k, r in ref.items()
            if r is not None and r.numel() >= BIG}


def running_errors(sd, ref):
    """name -> max |running - reference update| over the tensor's max-norm, in float32."""
    return {k: float((sd[k].float() - r.float()).abs().max() / r.float().abs().max()) for k, r in ref.items()}


def floor(case):
    """The reference-only floor: the CPU float32 oracle against the float64 oracle that replays the float32 run's own
    decisions -- what a faithful float32 implementation differs by.
    -> dict(e = f_k, scale = coherent part on the big tensors, running = running-statistics figures)."""
    rec = {}
    g32, run32 = oracle_gradients(case, case.state_dict(), case.cots[:1], torch.float32, record=rec)
    g64, run64 = oracle_gradients(case, case.state_dict(), case.cots[:1], torch.float64, tape=rec)
    return dict(e=errors(g32[0], g64[0], case.bn_train), scale=scale_errors(g32[0], g64[0]),
                running=running_errors(run32, run64))


def bounds(f, m, cap=1e-3):
    """e_k <= m * max(f_k, median f), never above the project's 1e-3 bar."""
    med = float(np.median(list(f.values())))
    return {k: min(m * max(v, med), cap) for k, v in f.items()}


def family(name, ndim):
    """Parameter family for the tables: the layer kind, not the position."""
    leaf = name.rsplit(".", 1)[1]
    if ".conv_offset_mask." in name:
        return "dcn offset conv " + leaf
    if ".proj_" in name or ".node_" in name:
        if ".actf." in name:
            return "dcn bn " + leaf
        return "dcn weight" if leaf == "weight" else "dcn bias (zero)"
    if ".up_" in name:
        return "up weight"
    if name.split(".")[0] in HEADS:
        return "head %s %s" % ("3x3" if (".conv." in name or name.endswith((".0.weight", ".0.bias"))) else "1x1", leaf)
    where = "root " if ".root." in name else "project/skip " if (".project." in name or ".skip." in name) else ""
    return where + ("conv weight" if ndim == 4 else "bn " + leaf)


def by_family(e, case):
    """family -> (max, median, tensors)."""
    fam = {}
    for k, v in e.items():
        fam.setdefault(family(k, case.weights[k].ndim), []).append(v)
    return {k: (max(v), float(np.median(v)), len(v)) for k, v in sorted(fam.items())}

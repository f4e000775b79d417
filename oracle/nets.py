"""Oracle: functional forward of DLA-34(+DCN up-sampling) and Hourglass from a
state_dict, torch CPU, any float dtype, eval-mode BN by default.  TEST INFRASTRUCTURE.

Independent of the product's nn.Module classes: it walks the reference's
checkpoint key grammar with torch.nn.functional only.

Follows:
  * DLA base      src/lib/models/networks/pose_dla_dcn.py:225-293 (BasicBlock 32-60,
                  Root 148-166, Tree 169-222; dla34 levels/channels :310-313)
  * DLAUp/IDAUp   pose_dla_dcn.py:362-413, DeformConv :347-359
  * DLASeg        pose_dla_dcn.py:427-482
  * Hourglass     src/lib/models/networks/large_hourglass.py:24-81, 283-342, 345-484
"""
import torch
import torch.nn.functional as F

from .dcn import dcn_module_forward


class Options(object):
    """Optional switches of both forwards (`opt=None` is the plain inference oracle, unchanged).

    bn_train  True: train-mode BatchNorm -- batch statistics, the biased variance in the normalisation, the unbiased
              one in the running update; the updated running statistics land in `running` (checkpoint key -> tensor).
    tape      the decision tape, a dict keyed by the checkpoint key prefix of the site: relu(y) at a site it names
              becomes y * tape[site] (a 0/1 gate) and max_pool2d becomes a gather of tape[site] (flat H*W indices
              as max_pool2d(..., return_indices=True) gives them).  Sites: the BatchNorm's prefix for every
              BN(+residual)+ReLU, the convolution's prefix for a bias+ReLU (the heads), `<tree>.downsample` for a pool.
              The forward is then the smooth function that a backward with those decisions differentiates.
    record    a dict that receives this run's own decisions in the tape's format."""

    def __init__(self, bn_train=False, tape=None, record=None, momentum=0.1):
        self.bn_train, self.tape, self.record, self.momentum = bn_train, tape, record, momentum
        self.running = {}


def _bn(sd, p, x, opt=None, eps=1e-5):
    if opt is None or not opt.bn_train:
        return F.batch_norm(x, sd[p + ".running_mean"], sd[p + ".running_var"],
                            sd[p + ".weight"], sd[p + ".bias"], False, 0.0, eps)
    n = x.numel() // x.shape[1]
    mean = x.mean((0, 2, 3))
    var = ((x - mean.view(1, -1, 1, 1)) ** 2).mean((0, 2, 3))              # biased
    m = opt.momentum
    with torch.no_grad():
        opt.running[p + ".running_mean"] = (1 - m) * sd[p + ".running_mean"] + m * mean
        opt.running[p + ".running_var"] = (1 - m) * sd[p + ".running_var"] + m * var * (n / (n - 1.0))
    xhat = (x - mean.view(1, -1, 1, 1)) * torch.rsqrt(var + eps).view(1, -1, 1, 1)
    return xhat * sd[p + ".weight"].view(1, -1, 1, 1) + sd[p + ".bias"].view(1, -1, 1, 1)


def _relu(y, p, opt=None):
    if opt is None or (opt.tape is None and opt.record is None):
        return F.relu(y)
    if opt.record is not None:
        opt.record[p] = (y > 0).detach()
    if opt.tape is not None:
        return y * opt.tape[p].to(y.dtype)
    return F.relu(y)


def _max_pool(x, p, stride, opt=None):
    if opt is None or (opt.tape is None and opt.record is None):
        return F.max_pool2d(x, stride, stride)
    if opt.record is not None:
        opt.record[p] = F.max_pool2d(x.detach(), stride, stride, return_indices=True)[1]
    if opt.tape is not None:
        idx = opt.tape[p]
        return x.flatten(2).gather(2, idx.flatten(2)).view(idx.shape)
    return F.max_pool2d(x, stride, stride)


def _conv(sd, p, x, stride=1, pad=0):
    return F.conv2d(x, sd[p + ".weight"], sd.get(p + ".bias"), stride=stride, padding=pad)


# ------------------------------- DLA-34 --------------------------------------

def _basic_block(sd, p, x, stride, residual=None, opt=None):
    if residual is None:
        residual = x
    out = _relu(_bn(sd, p + ".bn1", _conv(sd, p + ".conv1", x, stride, 1), opt), p + ".bn1", opt)
    out = _bn(sd, p + ".bn2", _conv(sd, p + ".conv2", out, 1, 1), opt)
    return _relu(out + residual, p + ".bn2", opt)


def _root(sd, p, xs, opt=None):
    x = _conv(sd, p + ".conv", torch.cat(xs, 1))
    return _relu(_bn(sd, p + ".bn", x, opt), p + ".bn", opt)          # residual_root=False for dla34


def _tree(sd, p, x, levels, stride, level_root, residual=None, children=None, opt=None):
    children = [] if children is None else children
    bottom = _max_pool(x, p + ".downsample", stride, opt) if stride > 1 else x
    if (p + ".project.0.weight") in sd:
        residual = _bn(sd, p + ".project.1", _conv(sd, p + ".project.0", bottom), opt)
    else:
        residual = bottom
    if level_root:
        children.append(bottom)
    if levels == 1:
        x1 = _basic_block(sd, p + ".tree1", x, stride, residual, opt)
        x2 = _basic_block(sd, p + ".tree2", x1, 1, opt=opt)
        return _root(sd, p + ".root", [x2, x1] + children, opt)
    x1 = _tree(sd, p + ".tree1", x, levels - 1, stride, False, residual, opt=opt)
    children.append(x1)
    return _tree(sd, p + ".tree2", x1, levels - 1, 1, False, children=children, opt=opt)


def dla34_base(sd, x, p="base", opt=None):
    levels = [1, 1, 1, 2, 2, 1]
    x = _relu(_bn(sd, p + ".base_layer.1", _conv(sd, p + ".base_layer.0", x, 1, 3), opt), p + ".base_layer.1", opt)
    ys = []
    x = _relu(_bn(sd, p + ".level0.1", _conv(sd, p + ".level0.0", x, 1, 1), opt), p + ".level0.1", opt)
    ys.append(x)
    x = _relu(_bn(sd, p + ".level1.1", _conv(sd, p + ".level1.0", x, 2, 1), opt), p + ".level1.1", opt)
    ys.append(x)
    for lv in range(2, 6):
        x = _tree(sd, "%s.level%d" % (p, lv), x, levels[lv], 2, lv >= 3, opt=opt)
        ys.append(x)
    return ys


def _deform_conv(sd, p, x, opt=None):
    y = dcn_module_forward(x, sd[p + ".conv.weight"], sd[p + ".conv.bias"],
                           sd[p + ".conv.conv_offset_mask.weight"],
                           sd[p + ".conv.conv_offset_mask.bias"])
    return _relu(_bn(sd, p + ".actf.0", y, opt), p + ".actf.0", opt)


def _ida_up(sd, p, layers, startp, endp, opt=None):
    for i in range(startp + 1, endp):
        k = i - startp
        w = sd["%s.up_%d.weight" % (p, k)]
        f = w.shape[2] // 2
        y = _deform_conv(sd, "%s.proj_%d" % (p, k), layers[i], opt)
        y = F.conv_transpose2d(y, w, None, stride=f, padding=f // 2, groups=w.shape[0])
        layers[i] = _deform_conv(sd, "%s.node_%d" % (p, k), y + layers[i - 1], opt)


def dla_seg_forward(sd, x, heads, down_ratio=4, last_level=5, opt=None):
    """pose_dla_dcn.py:470-482 -> [dict].  opt: see Options (None: the inference oracle)."""
    first = {2: 1, 4: 2, 8: 3, 16: 4}[down_ratio]
    layers = dla34_base(sd, x, opt=opt)
    out = [layers[-1]]
    for i in range(len(layers) - first - 1):
        _ida_up(sd, "dla_up.ida_%d" % i, layers, len(layers) - i - 2, len(layers), opt)
        out.insert(0, layers[-1])
    y = [out[i].clone() for i in range(last_level - first)]
    _ida_up(sd, "ida_up", y, 0, len(y), opt)
    z = {}
    for h in heads:
        t = _relu(_conv(sd, h + ".0", y[-1], 1, 1), h + ".0", opt)
        z[h] = _conv(sd, h + ".2", t)
    return [z]


# ------------------------------ Hourglass ------------------------------------

def _convolution(sd, p, x, k, stride=1, with_bn=True, opt=None):
    y = _conv(sd, p + ".conv", x, stride, (k - 1) // 2)
    if with_bn:
        return _relu(_bn(sd, p + ".bn", y, opt), p + ".bn", opt)
    return _relu(y, p + ".conv", opt)


def _residual(sd, p, x, stride=1, opt=None):
    y = _relu(_bn(sd, p + ".bn1", _conv(sd, p + ".conv1", x, stride, 1), opt), p + ".bn1", opt)
    y = _bn(sd, p + ".bn2", _conv(sd, p + ".conv2", y, 1, 1), opt)
    if (p + ".skip.0.weight") in sd:
        s = _bn(sd, p + ".skip.1", _conv(sd, p + ".skip.0", x, stride), opt)
    else:
        s = x
    return _relu(y + s, p + ".bn2", opt)


def _seq_residual(sd, p, x, count, first_stride=1, opt=None):
    for i in range(count):
        x = _residual(sd, "%s.%d" % (p, i), x, first_stride if i == 0 else 1, opt)
    return x


def _kp_module(sd, p, x, n, modules, opt=None):
    up1 = _seq_residual(sd, p + ".up1", x, modules[0], opt=opt)
    low1 = _seq_residual(sd, p + ".low1", x, modules[0], 2, opt)      # stride-2 conv replaces pooling
    if n > 1:
        low2 = _kp_module(sd, p + ".low2", low1, n - 1, modules[1:], opt)
    else:
        low2 = _seq_residual(sd, p + ".low2", low1, modules[1], opt=opt)
    low3 = _seq_residual(sd, p + ".low3", low2, modules[0], opt=opt)
    up2 = F.interpolate(low3, scale_factor=2)                       # nearest
    return up1 + up2


def hourglass_forward(sd, x, heads, nstack, opt=None):
    """large_hourglass.py:438-462 -> list of dicts, one per stack.  opt: see Options (None: the inference oracle)."""
    modules = [2, 2, 2, 2, 2, 4]
    inter = _convolution(sd, "pre.0", x, 7, 2, opt=opt)
    inter = _residual(sd, "pre.1", inter, 2, opt)
    outs = []
    for s in range(nstack):
        kp = _kp_module(sd, "kps.%d" % s, inter, 5, modules, opt)
        cnv = _convolution(sd, "cnvs.%d" % s, kp, 3, opt=opt)
        out = {}
        for h in heads:
            t = _convolution(sd, "%s.%d.0" % (h, s), cnv, 3, with_bn=False, opt=opt)
            out[h] = _conv(sd, "%s.%d.1" % (h, s), t)
        outs.append(out)
        if s < nstack - 1:
            a = _bn(sd, "inters_.%d.1" % s, _conv(sd, "inters_.%d.0" % s, inter), opt)
            b = _bn(sd, "cnvs_.%d.1" % s, _conv(sd, "cnvs_.%d.0" % s, cnv), opt)
            inter = _residual(sd, "inters.%d" % s, _relu(a + b, "cnvs_.%d.1" % s, opt), opt=opt)
    return outs

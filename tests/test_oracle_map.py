"""The `--eval_oracle_*` switches: cp_oracle_map (the closed form of the reference's breadth-first gen_oracle_map)
against the fixture recorded from the reference, and PolydetLoss / save_result with ground-truth heads."""
import contextlib
import ctypes
import sys

import numpy as np
import pytest
import torch

from centerpoly_amd import _C, synth
from oracle_map_host import gen_oracle_map_host

FLAGS = ("eval_oracle_hm", "eval_oracle_border_hm", "eval_oracle_offset", "eval_oracle_poly",
         "eval_oracle_pseudo_depth")
HEADS = {"hm": 8, "poly": 32, "pseudo_depth": 1, "reg": 2}
CASES = ("a", "b", "c", "d", "e", "f", "g")


def _opt(args):
    from centerpoly_amd.opts import opts
    with contextlib.redirect_stdout(sys.stderr):
        return opts().init(["polydet"] + list(args))


def _case(g, name):
    h, w = (int(v) for v in g[name + "_hw"])
    return g[name + "_feat"], g[name + "_ind"], h, w, g[name + "_out"]


# ---------------------------------------------------------------------------------------------- without a GPU

def test_fixture_holds_the_cases(golden):
    g = golden("oracle_map")
    assert tuple(str(n) for n in g["names"]) == CASES
    assert not g["a_out"].any() and int(g["a_ind"][0, 0]) == 0
    assert not g["d_out"][0].any() and (g["d_ind"][1] > 0).all() and (g["d_ind"][2] > 0).sum() == 1
    b = g["b_ind"][0]
    assert b[1] == 0 and b[0] == b[3] and b[0] > 0 and b[2] > 0
    assert g["g_ind"].shape[1] == 1024 and g["e_feat"].shape[2] == 33


@pytest.mark.parametrize("name", CASES)
def test_closed_form_equals_the_reference_fill(golden, name):
    feat, ind, h, w, ref = _case(golden("oracle_map"), name)
    assert np.array_equal(gen_oracle_map_host(feat, ind, w, h), ref)


def test_argument_validation_without_gpu():
    L = _C.lib()
    buf = (ctypes.c_char * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert L.cp_oracle_map(None, None, 1, 1, 1, 1, 1, None, None) == -1
    assert L.cp_oracle_map(p, p, 1, 1, 1, 1, 1, None, None) == -1
    assert L.cp_oracle_map(p, p, 1, 0, 1, 4, 4, p, None) == -1
    assert L.cp_oracle_map(p, p, 1, 4, 1, 4, -4, p, None) == -1
    assert L.cp_oracle_map(p, p, 1, 1025, 2, 4, 4, p, None) == -2          # beyond the kernel's seed table
    assert L.cp_oracle_map(p, p, 1, 4, 2, 1 << 16, 1 << 15, p, None) == -2  # h * w = 2^31


def test_gen_oracle_map_refuses_host_tensors():
    from centerpoly_amd.utils.oracle_utils import gen_oracle_map
    with pytest.raises(_C.NativeError):
        gen_oracle_map(torch.zeros(1, 4, 2), torch.zeros(1, 4, dtype=torch.int64), 8, 8)


@pytest.mark.parametrize("flag", FLAGS)
def test_switch_parses_and_the_loss_constructs(flag):
    from centerpoly_amd.trains.polydet import PolydetLoss
    opt = _opt(["--" + flag])
    assert getattr(opt, flag) is True
    assert sum(bool(getattr(opt, f)) for f in FLAGS) == 1
    PolydetLoss(opt)


def test_oracle_poly_with_cat_spec_poly_is_refused():
    from centerpoly_amd.trains.polydet import PolydetLoss
    opt = _opt(["--eval_oracle_poly", "--cat_spec_poly"])
    with pytest.raises(ValueError) as e:
        PolydetLoss(opt)
    assert "--eval_oracle_poly" in str(e.value) and "--cat_spec_poly" in str(e.value)


# ---------------------------------------------------------------------------------------------- on the GPU

@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_device_map_equals_the_fixture(golden, name):
    from centerpoly_amd.utils.oracle_utils import gen_oracle_map
    feat, ind, h, w, ref = _case(golden("oracle_map"), name)
    dev = torch.device("cuda:0")
    out = gen_oracle_map(torch.from_numpy(feat).to(dev), torch.from_numpy(ind).to(dev), w, h)
    assert out.shape == ref.shape and out.dtype == torch.float32
    assert np.array_equal(out.cpu().numpy(), ref)


_PROPERTY_IND = {}


def _property_ind(h, w):
    if (h, w) not in _PROPERTY_IND:
        _PROPERTY_IND[(h, w)] = synth.train_batch(2, h, w, stream="oracle_map/prop%dx%d" % (h, w),
                                                  with_input=False)["ind"]
    return _PROPERTY_IND[(h, w)]


@pytest.mark.gpu
@pytest.mark.parametrize("D", [1, 2, 32])
@pytest.mark.parametrize("h,w", [(96, 320), (128, 128)])
def test_device_map_equals_the_closed_form(h, w, D):
    from centerpoly_amd.utils.oracle_utils import gen_oracle_map
    ind = _property_ind(h, w)
    assert ind.shape == (2, 128)
    feat = synth.normal("oracle_map/prop%dx%d/feat%d" % (h, w, D), (2, 128, D))
    dev = torch.device("cuda:0")
    out = gen_oracle_map(torch.from_numpy(feat).to(dev), torch.from_numpy(ind).to(dev), w, h)
    assert np.array_equal(out.cpu().numpy(), gen_oracle_map_host(feat, ind, w, h))


def _smoke_state():
    """The model, weights and training batch of smoke(), in eval mode (one set of head outputs for every switch)."""
    from centerpoly_amd.models.model import create_model
    dev = torch.device("cuda:0")
    model = create_model("dla_34", dict(HEADS), 256)
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    model.load_state_dict({k: torch.from_numpy(v) for k, v in synth.fill_by_name(shapes).items()})
    model = model.to(dev).eval()
    nb = synth.train_batch(2, 16, 32, nbr_points=16, rep="cartesian", stream="smoke/train", in_h=64, in_w=128)
    return model, nb, dev


@pytest.fixture(scope="module")
def smoke_state():
    model, nb, dev = _smoke_state()
    batch = {k: torch.from_numpy(v).to(dev) for k, v in nb.items()}
    with torch.no_grad():
        probe = {k: v.clone().cpu() for k, v in model(batch["input"])[-1].items()}
    return model, nb, dev, probe


def _trainer(model, dev, args):
    from centerpoly_amd.trains.train_factory import train_factory
    opt = _opt(["--arch", "dla_34", "--nbr_points", "16"] + list(args))
    opt.device = dev
    trainer = train_factory["polydet"](opt, model)
    trainer.set_device(opt.gpus, opt.chunk_sizes, dev)
    return opt, trainer


@pytest.mark.gpu
@pytest.mark.parametrize("flag,head", [("eval_oracle_offset", "reg"), ("eval_oracle_poly", "poly"),
                                       ("eval_oracle_pseudo_depth", "pseudo_depth")])
def test_polydet_loss_with_an_oracle_map(smoke_state, flag, head):
    from oracle import losses as olos
    model, nb, dev, probe = smoke_state
    opt, trainer = _trainer(model, dev, ["--batch_size", "2", "--" + flag])
    batch = {k: torch.from_numpy(v).to(dev) for k, v in nb.items()}
    with torch.no_grad():
        output, loss, stats = trainer.step(batch, train=False)
    torch.cuda.synchronize()
    h, w = probe[head].shape[2:]
    want = gen_oracle_map_host(nb[head], nb["ind"], w, h)
    assert np.array_equal(output[head].cpu().numpy(), want)
    replaced = dict(probe)
    replaced[head] = torch.from_numpy(want)
    _, rstats = olos.polydet_loss([replaced], {k: torch.from_numpy(v) for k, v in nb.items()},
                                  poly_loss_kind="l1", rep="cartesian", poly_order=False)
    assert set(stats) == set(rstats)
    for k in rstats:
        a, b = float(stats[k].detach()), float(rstats[k])
        print("%s %s: %.9g vs oracle %.9g" % (flag, k, a, b))
        assert abs(a - b) <= 1e-3 * abs(b) + 1e-5, "loss term %s differs from the oracle: %g vs %g" % (k, a, b)


@pytest.mark.gpu
def test_polydet_loss_with_the_oracle_heat_map(smoke_state):
    from centerpoly_amd.models.losses import FocalLoss
    model, nb, dev, probe = smoke_state
    opt, trainer = _trainer(model, dev, ["--batch_size", "2", "--eval_oracle_hm"])
    batch = {k: torch.from_numpy(v).to(dev) for k, v in nb.items()}
    with torch.no_grad():
        output, loss, stats = trainer.step(batch, train=False)
    assert output["hm"] is batch["hm"]
    assert torch.equal(batch["hm"].cpu(), torch.from_numpy(nb["hm"]))             # and nothing wrote into it
    gt = torch.from_numpy(nb["hm"])
    want = FocalLoss()(gt, gt)                                                   # the same expression on the CPU
    assert nb["reg_mask"].sum() > 0 and torch.isnan(want)
    assert torch.isnan(stats["hm_l"]).item() and torch.isnan(stats["loss"]).item()
    assert torch.allclose(stats["hm_l"].cpu(), want, equal_nan=True)
    for k in ("off_l", "poly_l", "depth_l"):                                     # the other terms are untouched
        assert torch.isfinite(stats[k]).item(), k


@pytest.mark.gpu
def test_oracle_heads_decode_to_the_ground_truth(smoke_state):
    """All four heads replaced: what save_result decodes is the oracle decode of the replaced maps, and every object
    with ind > 0 comes back at its own centre with score 1 and its own polygon."""
    from centerpoly_amd.models.decode import polydet_decode
    from centerpoly_amd.utils.post_process import polydet_post_process
    from oracle import decode as odec
    model, _, dev, _ = smoke_state
    opt, trainer = _trainer(model, dev, ["--batch_size", "1", "--eval_oracle_hm", "--eval_oracle_offset",
                                         "--eval_oracle_poly", "--eval_oracle_pseudo_depth"])
    assert opt.rep == "cartesian" and opt.reg_offset
    h, w, N = 16, 32, 16
    nb = synth.train_batch(1, h, w, nbr_points=N, rep="cartesian", stream="oracle_map/e2e", in_h=64, in_w=128)
    batch = {k: torch.from_numpy(v).to(dev) for k, v in nb.items()}
    meta_c, meta_s = np.array([[64.0, 32.0]], np.float32), np.array([128.0], np.float32)
    batch["meta"] = {"c": torch.from_numpy(meta_c), "s": torch.from_numpy(meta_s), "img_id": torch.tensor([7])}
    with torch.no_grad():
        output, _, _ = trainer.step(batch, train=False)
        results = {}
        trainer.save_result(output, batch, results)
        dets = polydet_decode(output["hm"], output["poly"], output["pseudo_depth"], reg=output["reg"], K=opt.K,
                              rep=opt.rep)
    maps = {"hm": torch.from_numpy(nb["hm"])}
    for head in ("reg", "poly", "pseudo_depth"):
        maps[head] = torch.from_numpy(gen_oracle_map_host(nb[head], nb["ind"], w, h))
        assert torch.equal(output[head].cpu(), maps[head]), head
    dref, iref, cref = odec.polydet_decode(maps["hm"], maps["poly"], maps["pseudo_depth"], maps["reg"], K=opt.K,
                                           rep=opt.rep)
    assert torch.equal(dets.cpu(), dref)                                         # indices and values, bit for bit
    want = polydet_post_process(dref.numpy().reshape(1, -1, dref.shape[2]).copy(), meta_c, meta_s, h, w,
                                HEADS["hm"])[0]
    assert list(results) == [7] and results[7] == want
    # the objects themselves
    rows = dets.cpu().numpy()[0]
    n = int(nb["reg_mask"][0].sum())
    seen = 0
    for j in range(n):
        ind = int(nb["ind"][0, j])
        if ind <= 0:
            continue
        seen += 1
        k = np.nonzero(iref[0].numpy() == ind)[0]
        k = [q for q in k if rows[q, 4] == 1.0]
        assert len(k) == 1, "object %d at %d is not among the detections" % (j, ind)
        row = rows[k[0]]
        cx = np.float32(ind % w) + nb["reg"][0, j, 0]
        cy = np.float32(ind // w) + nb["reg"][0, j, 1]
        assert nb["hm"][0, int(row[5]), ind // w, ind % w] == 1.0
        assert np.array_equal(row[6:6 + 2 * N:2], nb["poly"][0, j, 0::2] + cx)
        assert np.array_equal(row[7:7 + 2 * N:2], nb["poly"][0, j, 1::2] + cy)
        assert row[6 + 2 * N] == nb["pseudo_depth"][0, j, 0]
    assert seen >= n - 1 and seen > 0

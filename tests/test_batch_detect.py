"""Detecting a batch of images per launch: cp_preprocess_warp_normalize_batch, BaseDetector.pre_process_batch /
run_batch, PolydetDetector's batched tail and test.py --test_batch_size.
CPU: the entry point's refusals, the options, the grouping generator.  GPU: the batch warp against the single-image
kernel and oracle/pre.py bit for bit, the network at B = 3 against B = 1, the chain behind the network against the
per-image functions on the batch's own heads bit for bit, B = 1 against run(), --keep_res, run_test."""
import contextlib
import ctypes
import functools
import io

import numpy as np
import pytest
import torch

import cases
from centerpoly_amd import _C, synth

MEAN = np.array([0.284, 0.323, 0.282], dtype=np.float32)
STD = np.array([0.0423, 0.0409, 0.0427], dtype=np.float32)
SIZES = ((37, 53), (64, 96), (90, 41))                       # (H, W): the first is smaller than the 64 x 96 output
DST_H, DST_W = 64, 96


def _img(tag, h, w):
    return (synth.uniform("batchdet/" + tag, (h, w, 3)) * 256).astype(np.uint8)


def _sources(sizes=SIZES):
    return [_img("src%d" % i, h, w) for i, (h, w) in enumerate(sizes)]


def _fix_res_map(h, w, dst_h, dst_w):
    """trans_input as pre_process makes it under --fix_res at scale 1."""
    from centerpoly_amd.utils.image import get_affine_transform
    c = np.array([w / 2.0, h / 2.0], dtype=np.float32)
    return get_affine_transform(c, max(h, w) * 1.0, 0, [dst_w, dst_h])


def _maps():
    """The fix_res maps of the first two sources; for the 90 x 41 one a shifted 1.5x map whose window leaves the image
    on the left and at the top (constant border 0)."""
    t = [_fix_res_map(h, w, DST_H, DST_W) for h, w in SIZES[:2]]
    t.append(np.array([[1.5, 0.04, 20.25], [-0.03, 1.5, 9.5]], np.float64))
    return np.stack([m.reshape(6) for m in t])


def _flat(images, dev):
    sizes = np.array([im.size for im in images], dtype=np.int64)
    flat = torch.from_numpy(np.concatenate([im.reshape(-1) for im in images])).to(dev)
    return flat, np.array([im.shape[:2] for im in images], np.int32), np.cumsum(sizes) - sizes


@functools.lru_cache(maxsize=None)
def _oracle_inputs():
    """oracle/pre.py on the host for the three sources, fp32 CHW; computed once, never modified."""
    from oracle import pre as opre
    out = []
    for im, t in zip(_sources(), _maps()):
        ref = opre.normalize_chw(opre.warp_affine_u8(im, t.reshape(2, 3), (DST_W, DST_H)), MEAN, STD)
        ref.setflags(write=False)
        out.append(ref)
    return tuple(out)


def _parse(args):
    from centerpoly_amd.opts import opts
    with contextlib.redirect_stdout(io.StringIO()):
        return opts().init(args)


# ------------------------------------------------------------------------------------------------ CPU

def test_batch_warp_is_exported_and_refuses_without_gpu():
    """The entry point validates on the host before any device work: callable with null device pointers."""
    assert "cp_preprocess_warp_normalize_batch" in _C.EXPORTS
    L = _C.lib()
    off = np.zeros(2, np.int64)
    hw = np.array([[4, 5], [6, 7]], np.int32)
    trans = np.tile(np.array([1.0, 0, 0, 0, 1.0, 0]), (2, 1))
    m, s = np.zeros(3, np.float32), np.ones(3, np.float32)
    P = lambda a: ctypes.c_void_p(a.ctypes.data)

    def call(off=off, hw=hw, batch=2, dh=8, dw=8, flip=0, host=True):
        h = (P(off), P(hw), P(trans), P(m), P(s)) if host else (None,) * 5
        return L.cp_preprocess_warp_normalize_batch(None, *h, batch, dh, dw, flip, None, None)

    assert call(host=False) == -1
    assert call() == -1 and call(flip=1) == -1               # sound tables, null device pointers
    assert call(batch=0) == -1 and call(batch=-2) == -1
    assert call(dh=0) == -1 and call(dw=0) == -1 and call(dw=-3) == -1
    assert call(hw=np.array([[4, 5], [0, 7]], np.int32)) == -1
    assert call(off=np.array([0, -1], np.int64)) == -1
    # the single-image limits hold per image: sources up to 32767 a side, up to 65535 output rows
    assert call(hw=np.array([[4, 5], [32768, 7]], np.int32)) == -2
    assert call(hw=np.array([[4, 32768], [6, 7]], np.int32)) == -2
    assert call(dh=65536) == -2
    assert call(hw=np.array([[32767, 32767], [6, 7]], np.int32), dh=65535) == -1


def test_batch_warp_wrapper_checks_the_buffer_on_the_host():
    from centerpoly_amd.utils.image import warp_affine_normalize_batch
    with pytest.raises(_C.NativeError):
        warp_affine_normalize_batch(torch.zeros(48, dtype=torch.uint8), [[4, 4]], [0], np.eye(2, 3)[None], MEAN, STD, 8, 8)


def test_test_batch_size_option(capsys):
    assert _parse(["polydet"]).test_batch_size == 1
    assert _parse(["polydet", "--test_batch_size", "4"]).test_batch_size == 4
    assert _parse(["polydet", "--test_batch_size", "1", "--debug", "1"]).debug == 1
    for bad in (["--test_batch_size", "0"], ["--test_batch_size", "-3"]):
        with pytest.raises(SystemExit):
            _parse(["polydet"] + bad)
        assert "--test_batch_size" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        _parse(["polydet", "--test_batch_size", "2", "--debug", "1"])
    err = capsys.readouterr().err
    assert "--test_batch_size" in err and "--debug" in err


def test_group_keeps_order_and_ends_where_the_size_changes():
    from centerpoly_amd.datasets.eval_images import group
    A, B = np.zeros((4, 6, 3), np.uint8), np.zeros((5, 6, 3), np.uint8)
    items = [{"img_id": i, "image": im} for i, im in enumerate([A, A, B, A, A, A])]
    ids = lambda groups: [[it["img_id"] for it in grp] for grp in groups]
    assert ids(group(iter(items), 2, True)) == [[0, 1], [2], [3, 4], [5]]
    assert ids(group(iter(items), 2, False)) == [[0, 1], [2, 3], [4, 5]]
    assert ids(group(iter(items), 4, False)) == [[0, 1, 2, 3], [4, 5]]
    assert ids(group(iter(items), 4, True)) == [[0, 1], [2], [3, 4, 5]]
    assert ids(group(iter(items), 1, True)) == [[i] for i in range(6)]
    assert [len(grp) for grp in group([A, B, B], 2, True)] == [1, 2]            # bare arrays are items too
    assert list(group(iter([]), 3, True)) == []
    with pytest.raises(ValueError):
        list(group(iter(items), 0, False))


# ------------------------------------------------------------------------------------------------ GPU

@pytest.mark.gpu
@pytest.mark.parametrize("flip", [False, True])
def test_batch_warp_matches_single_image_kernel_and_oracle(flip):
    from centerpoly_amd.utils.image import warp_affine_normalize, warp_affine_normalize_batch
    dev = torch.device("cuda")
    images, trans, B = _sources(), _maps(), len(SIZES)
    flat, hw, off = _flat(images, dev)
    out = warp_affine_normalize_batch(flat, hw, off, trans, MEAN, STD, DST_H, DST_W, flip_copy=flip)
    assert tuple(out.shape) == ((2 if flip else 1) * B, 3, DST_H, DST_W) and out.dtype == torch.float32
    zero = ((0.0 / 255. - MEAN.astype(np.float64)) / STD).astype(np.float32)    # what a border pixel becomes
    for b, im in enumerate(images):
        single = warp_affine_normalize(torch.from_numpy(im).to(dev), trans[b].reshape(2, 3), MEAN, STD, DST_H, DST_W,
                                       flip_copy=flip)
        assert torch.equal(out[b], single[0]), b
        ref = _oracle_inputs()[b]
        assert np.array_equal(out[b].cpu().numpy(), ref), b
        if flip:
            assert torch.equal(out[B + b], single[1]), b
            assert np.array_equal(out[B + b].cpu().numpy(), ref[:, :, ::-1]), b
    # the shifted map really shows the border, the fix_res maps of the wide sources pad top and bottom
    last = out[2].cpu().numpy()
    assert all((last[c, 0, :] == zero[c]).all() and (last[c, :, 0] == zero[c]).all() for c in range(3))
    assert not all((last[c] == zero[c]).all() for c in range(3))


@pytest.mark.gpu
def test_batch_warp_crosses_the_16_image_chunk():
    from centerpoly_amd.utils.image import warp_affine_normalize, warp_affine_normalize_batch
    dev = torch.device("cuda")
    B = 17
    images = [_img("chunk%d" % i, 8, 8) for i in range(B)]
    trans = np.stack([np.array([2.0 + 0.05 * i, 0.0, 3.0 + i, 0.0, 2.0, 0.25 * i]) for i in range(B)])
    flat, hw, off = _flat(images, dev)
    out = warp_affine_normalize_batch(flat, hw, off, trans, MEAN, STD, 16, 32, flip_copy=True)
    assert tuple(out.shape) == (2 * B, 3, 16, 32)
    for b, im in enumerate(images):
        single = warp_affine_normalize(torch.from_numpy(im).to(dev), trans[b].reshape(2, 3), MEAN, STD, 16, 32,
                                       flip_copy=True)
        assert torch.equal(out[b], single[0]) and torch.equal(out[B + b], single[1]), b


@pytest.mark.gpu
def test_batch_warp_partial_last_block_in_x():
    from centerpoly_amd.utils.image import warp_affine_normalize, warp_affine_normalize_batch
    from oracle import pre as opre
    dev = torch.device("cuda")
    images = [_img("wide0", 9, 130), _img("wide1", 12, 77)]
    trans = np.array([[2.3, 0.0, 0.5, 0.0, 0.9, 0.0], [3.9, 0.1, -2.0, 0.0, 0.7, 0.25]], np.float64)
    flat, hw, off = _flat(images, dev)
    out = warp_affine_normalize_batch(flat, hw, off, trans, MEAN, STD, 8, 300, flip_copy=True)
    for b, im in enumerate(images):
        single = warp_affine_normalize(torch.from_numpy(im).to(dev), trans[b].reshape(2, 3), MEAN, STD, 8, 300,
                                       flip_copy=True)
        assert torch.equal(out[b], single[0]) and torch.equal(out[2 + b], single[1]), b
        ref = opre.normalize_chw(opre.warp_affine_u8(im, trans[b].reshape(2, 3), (300, 8)), MEAN, STD)
        assert np.array_equal(out[b].cpu().numpy(), ref), b


@pytest.mark.gpu
def test_batch_warp_wrapper_refuses_images_outside_the_buffer():
    from centerpoly_amd.utils.image import warp_affine_normalize_batch
    flat = torch.zeros(4 * 4 * 3 + 10, dtype=torch.uint8, device="cuda")
    t = np.tile(np.array([1.0, 0, 0, 0, 1.0, 0]), (2, 1))
    with pytest.raises(ValueError):
        warp_affine_normalize_batch(flat, [[4, 4], [4, 4]], [0, 48], t, MEAN, STD, 8, 8)
    with pytest.raises(ValueError):
        warp_affine_normalize_batch(flat, [[4, 4], [0, 4]], [0, 48], t, MEAN, STD, 8, 8)
    with pytest.raises(TypeError):
        warp_affine_normalize_batch(flat.float(), [[4, 4]], [0], t[:1], MEAN, STD, 8, 8)


def _seed(model):
    """cases.fill_weights into a detector's or a bare model, then prepare_inference()."""
    dev = next(model.parameters()).device
    model.train()                                                 # drops the prepared forms of the random weights
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    model.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)).to(dev)
                           for k, v in cases.fill_weights(shapes).items()})
    model.eval()
    model.prepare_inference()
    return model


@pytest.mark.gpu
def test_network_at_batch_3_matches_single_images():
    """DLA-34 as the detector prepares it: every head of model(batch)[b] against model(batch[b:b+1]) within 2e-4 of
    the head's max-norm, the bound test_hourglass_prepare_inference_matches_plain_eval and tests/test_wide_polygons.py
    hold between two device paths of the same weights.  Equal bits are not expected: staged_ks and region_ksplit choose
    their K split from the launch's workgroup count, which includes B."""
    from centerpoly_amd.models.model import create_model
    heads = dict(cases.HEADS)
    model = _seed(create_model("dla_34", heads, 256).to("cuda"))
    x = torch.from_numpy(synth.normal("batchdet/net/x", (3, 3, 64, 96)).astype(np.float32)).cuda()
    with torch.no_grad():
        whole = model(x)[-1]
        for b in range(3):
            alone = model(x[b:b + 1].contiguous())[-1]
            for h in heads:
                a, got = alone[h], whole[h][b:b + 1]
                err, bound = (a - got).abs().max().item(), 2e-4 * a.abs().max().item()
                print("image %d head %s: max error %.3e, bound %.3e" % (b, h, err, bound))
                assert a.shape == got.shape and err <= bound, (b, h)


class _Recorder(torch.nn.Module):
    """The detector's model with a copy of every launch's heads kept (process applies the sigmoid in place)."""

    def __init__(self, model):
        super(_Recorder, self).__init__()
        self.model, self.seen = model, []

    def forward(self, x):
        out = self.model(x)
        self.seen.append({k: v.clone() for k, v in out[-1].items()})
        return out


def _detector(extra=()):
    from centerpoly_amd.detectors.detector_factory import detector_factory
    opt = _parse(["polydet", "--arch", "dla_34", "--input_h", "64", "--input_w", "96", "--K", "32"] + list(extra))
    with contextlib.redirect_stdout(io.StringIO()):
        det = detector_factory["polydet"](opt)
    _seed(det.model)
    return det, opt


def _same_results(got, want, C):
    assert sorted(got) == sorted(want) == list(range(1, C + 1))
    for j in range(1, C + 1):
        assert got[j].dtype == want[j].dtype == np.float32 and got[j].shape == want[j].shape, j
        assert np.array_equal(got[j], want[j]), j


SETTINGS = {"plain": [], "flip": ["--flip_test"], "scales": ["--test_scales", "1,0.5"], "nms": ["--nms"],
            "host_merge": ["--test_scales", "1,0.5"]}       # the last with device_merge off: merge_outputs on the host


@pytest.mark.gpu
@pytest.mark.parametrize("setting", sorted(SETTINGS))
def test_run_batch_tail_matches_per_image_functions_on_the_batch_heads(setting):
    """run_batch(imgs)["results"][b] against polydet_decode -> post_process (image b's meta) -> merge on the slices
    [b:b+1] of the batched network's own heads, class by class, bit for bit: three images of different sizes share a
    batch under --fix_res.  The check runs on the batch's own heads so that near-ties in the top-K cannot make it flaky."""
    from centerpoly_amd.models.decode import polydet_decode
    from centerpoly_amd.models.utils import flip_tensor
    det, opt = _detector(SETTINGS[setting])
    det.device_merge = setting != "host_merge"
    imgs = [_img("tail0", 128, 256), _img("tail1", 100, 180), _img("tail2", 64, 96)]
    B, C = len(imgs), opt.num_classes
    rec = det.model = _Recorder(det.model)
    ret = det.run_batch(imgs)
    det.model = rec.model
    assert ret["n"] == B and len(ret["results"]) == B and len(rec.seen) == len(opt.test_scales)
    assert all(ret[t] >= 0 for t in ("tot", "load", "pre", "net", "dec", "post", "merge"))
    kept = [(det.device_rows(image=b).cpu().numpy(), det.host_rows(image=b).copy()) for b in range(B)]
    with pytest.raises(IndexError):
        det.device_rows(image=B)
    for b, img in enumerate(imgs):
        det._slot, det._merged, det._batch = 0, False, None                 # as run() begins
        detections = []
        for scale, heads in zip(opt.test_scales, rec.seen):
            assert heads["hm"].shape[0] == (2 if opt.flip_test else 1) * B
            meta = det.pre_process(img, scale)[1]
            with torch.no_grad():
                hm = heads["hm"][b:b + 1].sigmoid()
                if opt.flip_test:
                    hm = (hm + flip_tensor(heads["hm"][B + b:B + b + 1].sigmoid())) / 2
                dets = polydet_decode(hm, heads["poly"][b:b + 1], heads["pseudo_depth"][b:b + 1],
                                      reg=heads["reg"][b:b + 1], cat_spec_poly=opt.cat_spec_poly, K=opt.K, rep=opt.rep)
            detections.append(det.post_process(dets, meta, scale))
        want = det.merge(detections)
        _same_results(ret["results"][b], want, C)
        assert sum(len(v) for v in want.values()) > 0
        # the rows run_batch kept for image b are the ones run()'s tail keeps
        assert np.array_equal(kept[b][0], det.device_rows(want).cpu().numpy()), b
        assert np.array_equal(kept[b][1], det.host_rows(want)), b
    # the images differ, and so do their detections
    assert not all(np.array_equal(ret["results"][0][j], ret["results"][1][j]) for j in range(1, C + 1))


@pytest.mark.gpu
@pytest.mark.parametrize("setting", ["plain", "scales"])
def test_run_batch_of_one_equals_run(setting):
    det, opt = _detector(SETTINGS[setting])
    img = _img("one", 100, 180)
    single = det.run(img)
    rows, host = det.device_rows().clone(), det.host_rows().copy()
    batch = det.run_batch([img])
    assert batch["n"] == 1 and len(batch["results"]) == 1
    _same_results(batch["results"][0], single["results"], opt.num_classes)
    assert torch.equal(det.device_rows(image=0), rows) and np.array_equal(det.host_rows(image=0), host)
    # run() afterwards holds one image again
    det.run(img)
    assert torch.equal(det.device_rows(), rows)
    with pytest.raises(IndexError):
        det.device_rows(image=1)


@pytest.mark.gpu
def test_keep_res_batches_need_equal_source_sizes():
    det, opt = _detector(["--keep_res"])
    a, b, c = _img("keep0", 64, 96), _img("keep1", 64, 96), _img("keep2", 40, 96)
    with pytest.raises(ValueError) as e:
        det.run_batch([a, c])
    assert "(64, 96)" in str(e.value) and "(40, 96)" in str(e.value)
    ret = det.run_batch([a, b])
    assert ret["n"] == 2 and all(sum(len(v) for v in r.values()) == opt.K for r in ret["results"])
    with pytest.raises(TypeError):
        det.run_batch([a.astype(np.float32)])
    with pytest.raises(ValueError):
        det.run_batch([])
    det.opt.debug = 1
    with pytest.raises(ValueError):
        det.run_batch([a, b])
    det.opt.debug = 0


@pytest.mark.gpu
def test_run_test_groups_the_synthetic_set(tmp_path, monkeypatch):
    """test.py's loop at --synthetic_samples 4 --test_batch_size 3: groups of 3 + 1, four result entries of K rows,
    and host_rows(image=b) split by class reproduces results[b]."""
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("centerpoly_test_driver", os.path.join(root, "test.py"))
    driver = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(driver)
    from centerpoly_amd.detectors.polydet import PolydetDetector
    from centerpoly_amd.opts import opts
    groups = []
    inner = PolydetDetector.run_batch

    def recording(self, images):
        ret = inner(self, images)
        groups.append([self.host_rows(image=b).copy() for b in range(ret["n"])])
        return ret

    monkeypatch.setattr(PolydetDetector, "run_batch", recording)
    with contextlib.redirect_stdout(io.StringIO()):
        opt = opts().parse(["polydet", "--dataset", "synthetic", "--synthetic_samples", "4", "--test_batch_size", "3",
                            "--input_h", "64", "--input_w", "96", "--K", "32"])
        opt.save_dir = str(tmp_path)
        out = driver.run_test(opt)
    assert [len(g) for g in groups] == [3, 1]
    assert sorted(out["results"]) == [0, 1, 2, 3]
    for ind, rows in enumerate(r for g in groups for r in g):
        res = out["results"][ind]
        assert sum(len(v) for v in res.values()) == 32 and tuple(rows.shape) == (32, rows.shape[1])
        for j in sorted(res):
            r = rows[rows[:, 5] == j - 1]
            assert np.array_equal(res[j], np.concatenate([r[:, :5], r[:, 6:]], axis=1)), (ind, j)


@pytest.mark.gpu
def test_driver_scores_the_cityscapes_set_in_batches(tmp_path, capsys):
    """test.py --dataset cityscapes --gt_dir ... --test_batch_size 3 on four 1024 x 2048 images (groups of 3 + 1): every
    image is scored on the device from device_rows(image=b), and the allAp, the count tables and results.json equal
    what CITYSCAPES.run_eval makes on the host of the results of the same run (the check tests/test_writer_instances.py
    holds for the per-image loop)."""
    import json
    import test_writer_instances as twi
    driver = twi._driver()
    base = twi._cityscapes_set(str(tmp_path))
    ap, tables, text = twi._run_and_compare(driver, base + ["--no_mask_files", "--test_batch_size", "3"], tmp_path,
                                            "batched", capsys)
    assert len(json.loads(text)) == 4 * 128 and len(tables) == 4

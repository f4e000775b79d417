"""cp_pixel_confusion on the device against its host restatement (tests/golden/pixel_level_host.py), exact, and the
pixel-level evaluator end to end: instance maps, the files --save_ids writes, test.py --pixel_iou."""
import contextlib
import ctypes
import io
import json
import os

import numpy as np
import pytest

import pixel_level_host as host
from centerpoly_amd import _C
from centerpoly_amd.datasets.evaluation import pixel_level as pl
from test_pixel_level_cpu import CASES, IDENTITY, PROTOS, assert_scores, gt_ids, rec

pytestmark = pytest.mark.gpu
CS = pl.CITYSCAPES


def run_kernel(pred, ids, inst_ids, pred_label=IDENTITY, proto=CS, L=None, group=None, conf=None, inst_fill=0,
               pred_offset=0, ids_offset=0, null_tables=False, bad=None):
    """The kernel on host arrays pred uint8 [H, W] and ids uint16 [H, W], uploaded `pred_offset` bytes / `ids_offset`
    elements into their buffers: (conf int64 [L, L], inst int64 [G, 3], bad int64 [2]) as the device leaves them; conf
    and bad start from the given tables (zeros when None)."""
    import torch
    dev = torch.device("cuda")
    H, W = pred.shape
    L = proto.L if L is None else L
    group = np.ascontiguousarray(proto.label_group[:L] if group is None else group, np.int8)
    G = len(inst_ids)
    pbuf = torch.zeros(H * W + pred_offset + 16, dtype=torch.uint8, device=dev)
    ibuf = torch.zeros(H * W + ids_offset + 16, dtype=torch.int16, device=dev)
    pbuf[pred_offset:pred_offset + H * W] = torch.from_numpy(np.ascontiguousarray(pred).reshape(-1)).to(dev)
    ibuf[ids_offset:ids_offset + H * W] = torch.from_numpy(np.ascontiguousarray(ids).view(np.int16).reshape(-1)).to(dev)
    conf_dev = torch.from_numpy(np.zeros(L * L, np.int64) if conf is None else conf.reshape(-1).copy()).to(dev)
    inst_dev = torch.full((max(3 * G, 1),), inst_fill, dtype=torch.int32, device=dev)
    ids_dev = torch.tensor([int(v) for v in inst_ids] or [0], dtype=torch.int32).to(dev)
    bad_dev = torch.from_numpy(np.zeros(2, np.int32) if bad is None else np.array(bad, np.int32)).to(dev)
    lib = _C.lib()
    nbytes = lib.cp_pixel_confusion_workspace_bytes(G)
    ws = _C.workspace(nbytes, dev)
    label = np.ascontiguousarray(pred_label, np.uint8)
    at = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)                      # noqa: E731
    _C.check(lib.cp_pixel_confusion(at(pbuf, pred_offset), label.ctypes.data_as(ctypes.c_void_p), at(ibuf, 2 * ids_offset),
                                    H, W, proto.id_divisor, proto.id_direct_below, L,
                                    group.ctypes.data_as(ctypes.c_void_p), None if null_tables else at(ids_dev), G,
                                    at(conf_dev), None if null_tables else at(inst_dev), at(bad_dev), at(ws), nbytes,
                                    _C.stream()), "cp_pixel_confusion")
    torch.cuda.synchronize()
    return (conf_dev.cpu().numpy().reshape(L, L), inst_dev.cpu().numpy().astype(np.int64)[:3 * G].reshape(G, 3),
            bad_dev.cpu().numpy().astype(np.int64))


def want(pred, ids, inst_ids, pred_label=IDENTITY, proto=CS, L=None, group=None):
    L = proto.L if L is None else L
    return host.pixel_confusion(pred, pred_label, ids, proto.id_divisor, proto.id_direct_below, L,
                                proto.label_group[:L] if group is None else group, inst_ids)


def same(got, exp):
    for g, e, what in zip(got, exp, ("conf", "inst", "bad")):
        assert np.array_equal(g, e), what


def interest(ids, proto=CS):
    return proto.instances_of_interest(np.bincount(ids.reshape(-1), minlength=65536))


@pytest.mark.parametrize("proto", sorted(PROTOS))
def test_odd_image_from_unaligned_buffers(proto):
    p = PROTOS[proto]
    ids, pred = gt_ids("odd37x53", proto), rec("odd37x53")["pred"]
    inst_ids = interest(ids, p)
    got = run_kernel(pred, ids, inst_ids, proto=p, pred_offset=1, ids_offset=1)
    same(got, want(pred, ids, inst_ids, proto=p))
    z = rec("odd37x53")
    assert np.array_equal(got[0], z["conf_" + proto]) and np.array_equal(got[1], z["rows_" + proto][:, 1:])


@pytest.mark.parametrize("shape", [(1, 1), (1, 17), (19, 1)])
def test_tiny_shapes(shape):
    rng = np.random.RandomState(shape[0] * 100 + shape[1])
    ids = rng.choice(np.array([7, 26001, 24002], np.uint16), shape)
    pred = rng.choice(np.array([0, 24, 26], np.uint8), shape)
    for offsets in ((0, 0), (3, 5)):
        same(run_kernel(pred, ids, [24002, 26001], pred_offset=offsets[0], ids_offset=offsets[1]),
             want(pred, ids, [24002, 26001]))


@pytest.mark.parametrize("proto", sorted(PROTOS))
def test_full_size_fixture_against_its_golden(proto):
    p = PROTOS[proto]
    z = rec("star16")
    ids = gt_ids("star16", proto)
    inst_ids = interest(ids, p)
    assert ids.shape == (1024, 2048) and inst_ids.tolist() == z["rows_" + proto][:, 0].tolist()
    conf, inst, bad = run_kernel(z["pred"], ids, inst_ids, proto=p)
    assert np.array_equal(conf, z["conf_" + proto]) and np.array_equal(inst, z["rows_" + proto][:, 1:])
    assert bad.tolist() == [0, 0]
    again = run_kernel(z["pred"], ids, inst_ids, proto=p)                           # the same bits on every run
    same(again, (conf, inst, bad))


def test_constant_image_fills_one_bin():
    H, W = 512, 2048
    ids = np.full((H, W), 26007, np.uint16)
    pred = np.full((H, W), 27, np.uint8)
    conf, inst, bad = run_kernel(pred, ids, [26007])
    assert conf[26, 27] == H * W == conf.sum() and inst.tolist() == [[H * W, 0, H * W]] and bad.tolist() == [0, 0]


def test_alternating_pixels_leave_no_run_longer_than_one():
    H, W = 67, 131                                           # odd width: the pattern shifts from row to row
    k = np.arange(H * W).reshape(H, W)
    ids = np.where(k % 2 == 0, 26001, 24002).astype(np.uint16)
    pred = np.where(k % 2 == 0, 24, 26).astype(np.uint8)
    pred[k % 3 == 0] = 26
    got = run_kernel(pred, ids, [24002, 26001])
    same(got, want(pred, ids, [24002, 26001]))
    assert (got[0] > 0).sum() >= 3 and got[1][:, 0].min() > 0


def test_1024_instances_absent_ids_and_no_table():
    """A 32 x 32 grid of 2 x 3 cells, one instance each (ids 24001 .. 25024: two labels); half of the columns name ids
    the image does not hold, and ids of the image that are in no column touch no column."""
    cell = np.arange(32 * 32).reshape(32, 32)
    ids = np.kron(cell, np.ones((2, 3), np.int64)) + 24001
    assert ids.shape == (64, 96) and ids.max() == 25024
    ids = ids.astype(np.uint16)
    rng = np.random.RandomState(9)
    pred = rng.choice(np.array([0, 24, 25, 26], np.uint8), ids.shape)
    every = np.unique(ids).astype(np.int64)
    same(run_kernel(pred, ids, every), want(pred, ids, every))
    mixed = np.concatenate([every[::2], every[1::2][:510] + 30000, [-5, 70000]])      # 512 present, 512 absent
    assert len(mixed) == 1024
    got = run_kernel(pred, ids, mixed)
    same(got, want(pred, ids, mixed))
    assert (got[1][:512, 0] == 6).all() and not got[1][512:].any()
    exp = want(pred, ids, [])
    got = run_kernel(pred, ids, [], null_tables=True)                               # G == 0 with NULL tables
    assert np.array_equal(got[0], exp[0]) and got[1].shape == (0, 3) and got[2].tolist() == [0, 0]


def test_accumulation():
    ids, pred = gt_ids("odd37x53", "cityscapes"), rec("odd37x53")["pred"]
    inst_ids = interest(ids)
    one = want(pred, ids, inst_ids)
    first = run_kernel(pred, ids, inst_ids, inst_fill=12345)                        # inst is written, not added to
    same(first, one)
    second = run_kernel(pred[::-1].copy(), ids[::-1].copy(), inst_ids, conf=first[0], inst_fill=-7)
    assert np.array_equal(second[0], 2 * one[0]) and np.array_equal(second[1], one[1])      # two calls add up
    preset = np.full((34, 34), 2 ** 32 - 1, np.int64)                               # carries into the high word
    got = run_kernel(pred, ids, inst_ids, conf=preset)
    assert np.array_equal(got[0], preset + one[0]) and (got[0] >= 2 ** 32).any()


def test_bad_labels_of_both_kinds():
    rng = np.random.RandomState(3)
    H, W = 23, 31
    ids = rng.choice(np.array([7, 26, 26001, 24002, 35000, 40, 999, 1000], np.uint16), (H, W))
    pred = rng.choice(np.arange(7, dtype=np.uint8), (H, W))
    label = np.zeros(256, np.uint8)
    label[:7] = [0, 7, 24, 26, 33, 34, 200]                 # a table that is no identity: two bytes map outside
    cols = [26001, 24002, 35000, 5]
    got = run_kernel(pred, ids, cols, pred_label=label)
    exp = want(pred, ids, cols, pred_label=label)
    same(got, exp)
    both = np.isin(ids, [35000, 40, 999]) & (pred >= 5)
    assert both.any() and got[2][0] == np.isin(ids, [35000, 40, 999]).sum() and got[2][1] > 0
    assert got[0].sum() + got[2].sum() == H * W             # a pixel bad in both counts in bad[0] only
    # a smaller table: L = 27 turns labels 27 .. 33 into bad ones
    got = run_kernel(pred, ids, cols, pred_label=label, L=27)
    same(got, want(pred, ids, cols, pred_label=label, L=27))
    assert got[2][1] > exp[2][1]


def test_evaluator_on_the_fixture_set_and_its_errors():
    import torch
    for proto, p in sorted(PROTOS.items()):
        ev = pl.PixelLevelEvaluator(p)
        for k, name in enumerate(CASES):
            z = rec(name)
            pred = torch.from_numpy(z["pred"]).cuda()
            ids = gt_ids(name, proto)
            rows = ev.add_image(pred, IDENTITY, ids if k % 2 else torch.from_numpy(ids.view(np.int16)).cuda(), name)
            assert np.array_equal(rows, z["rows_" + proto])
        with open(os.path.join(os.path.dirname(__file__), "golden", "pixel_level_set.json")) as f:
            assert_scores(ev.summarize(), json.load(f)["protocols"][proto]["result"])
    ev = pl.PixelLevelEvaluator()
    pred = torch.zeros((8, 8), dtype=torch.uint8, device="cuda")
    ids = np.full((8, 8), 7, np.uint16)
    with pytest.raises(ValueError, match="frame_x.*ground truth is"):
        ev.add_image(pred, IDENTITY, np.full((8, 9), 7, np.uint16), "frame_x")
    bad_gt = ids.copy()
    bad_gt[3, 3] = 35001
    with pytest.raises(ValueError, match="frame_y.*Unknown label"):
        ev.add_image(pred, IDENTITY, bad_gt, "frame_y")
    with pytest.raises(ValueError, match="frame_z.*predicted pixels"):
        ev.add_image(torch.full((8, 8), 34, dtype=torch.uint8, device="cuda"), IDENTITY, ids, "frame_z")
    many = (np.arange(40 * 40).reshape(40, 40) % 1100 + 24001).astype(np.uint16)
    with pytest.raises(ValueError, match="frame_w.*more than 1024"):
        ev.add_image(torch.zeros((40, 40), dtype=torch.uint8, device="cuda"), IDENTITY, many, "frame_w")


def test_add_maps_equals_the_written_files_and_the_host(tmp_path):
    """add_maps on instances() of synthetic detection rows == evaluate_result_dir on what save_ids wrote == the host
    restatement of the same maps, for both writer families."""
    import torch
    from PIL import Image
    import test_instances_api as tia
    from centerpoly_amd.detectors import instances
    for dataset, proto, stem, gt_name in (("cityscapes", "cityscapes", "frankfurt_a_leftImg8bit",
                                           "frankfurt_a_gtFine_instanceIds.png"), ("kitti_poly", "kitti", "000007", "000007.png")):
        p = PROTOS[proto]
        ds = tia._dataset(dataset)
        rows = tia._rows(len(ds.class_name) - 1)
        maps = instances.instance_maps(torch.from_numpy(rows).cuda(), ds, (tia.W, tia.H))
        labels = maps.labels.cpu().numpy()
        assert len(np.unique(labels)) >= 3
        # ground truth: the prediction's own ids shifted by 9 pixels, so every count is between nothing and all
        gt = np.roll(maps.ids.cpu().numpy(), 9, axis=1).astype(np.uint16)
        gt[gt == 0] = 7 if proto == "cityscapes" else 7 * 256
        ev = pl.PixelLevelEvaluator(p)
        got_rows = ev.add_maps(maps, gt, stem)
        got = ev.summarize()
        inst_ids = interest(gt, p)
        conf, inst, bad = host.pixel_confusion(labels.astype(np.uint8), IDENTITY, gt, p.id_divisor, p.id_direct_below, p.L,
                                               p.label_group, inst_ids)
        assert got["confMatrix"] == conf.tolist() and np.array_equal(got_rows[:, 1:], inst) and len(inst) >= 1
        assert 0 < inst[:, 1].sum() < inst[:, 0].sum()
        by_host = pl.PixelLevelEvaluator(p)
        by_host.add_counts(conf, got_rows)
        out = str(tmp_path / dataset)
        instances.save_ids(maps, os.path.join(out, "instances"), stem)
        os.makedirs(os.path.join(out, "gt"))
        Image.fromarray(gt).save(os.path.join(out, "gt", gt_name))
        by_files = pl.evaluate_result_dir(os.path.join(out, "instances"), [os.path.join(out, "gt", gt_name)], protocol=p)
        for other in (by_host.summarize(), by_files):
            assert json.dumps(other, sort_keys=True) == json.dumps(got, sort_keys=True)


def _kitti_set(tmp):
    """Two small KITTI-style images with an annotation file and an instance ground truth of their own size."""
    from PIL import Image
    import test_instances_api as tia
    img_dir, annot_dir, gt_dir = (os.path.join(tmp, d) for d in ("image_2", "BBoxes", "instance"))
    for d in (img_dir, annot_dir, gt_dir):
        os.makedirs(d)
    stems = ["000010", "000011"]
    for k, (stem, (h, w)) in enumerate(zip(stems, tia.SIZES)):
        Image.fromarray(tia._image(h, w, 90 + k)[:, :, ::-1]).save(os.path.join(img_dir, stem + ".png"))
        gt = np.full((h, w), 7 * 256, np.uint16)
        gt[h // 4:h // 2, w // 8:w // 2] = 26 * 256 + 1
        gt[h // 2:, w // 2:] = 24 * 256 + 2
        gt[:h // 5, w // 2:] = 26 * 256
        Image.fromarray(gt).save(os.path.join(gt_dir, stem + ".png"))
    with open(os.path.join(annot_dir, "val16.json"), "w") as f:
        json.dump({"images": [{"id": 10 + k, "file_name": s + ".png", "height": h, "width": w}
                              for k, (s, (h, w)) in enumerate(zip(stems, tia.SIZES))], "annotations": [], "categories": []}, f)
    return tia._args(tmp, "kitti_poly", ["--annot_dir", annot_dir, "--img_dir", img_dir, "--gt_dir", gt_dir,
                                         "--not_prefetch_test", "--no_mask_files"])


def _drive(args, tmp_path, monkeypatch, capsys, proto, n_images, plain=True):
    """test.py --pixel_iou per image and with --test_batch_size 2: the returned scores are the evaluator's on the maps
    the run saw, the tables are printed after the AP table, the JSON file is written; without the flag, no trace."""
    import test_instances_api as tia
    from centerpoly_amd.opts import opts
    seen = tia._record_instances(monkeypatch)
    driver = tia._module("test")
    for batch in (1, 2):
        opt = opts().parse(args + ["--pixel_iou", "--test_batch_size", str(batch)])
        opt.save_dir = str(tmp_path / ("exp_b%d" % batch))
        del seen[:]
        out = driver.run_test(opt)
        text = capsys.readouterr().out
        assert len(seen) == n_images and "pixel" in out
        assert text.index("AP_50%") < text.index("classes          IoU      nIoU") < text.index("categories       IoU")
        ev = pl.PixelLevelEvaluator(PROTOS[proto])
        for maps, item in zip(seen, out["dataset"].images):
            ev.add_maps(maps, _gt_of(out, opt, item))
        want_res = ev.summarize()
        assert json.dumps(out["pixel"], sort_keys=True) == json.dumps(want_res, sort_keys=True)
        with open(os.path.join(opt.save_dir, pl.RESULT_FILE)) as f:
            assert json.dumps(json.load(f), sort_keys=True) == json.dumps(want_res, sort_keys=True)
        assert np.array(out["pixel"]["confMatrix"])[:, 24:].sum() > 0              # something was predicted
    # (a batched launch may round the heads differently from a single one, so the two runs need not agree with each
    # other: each is compared with the evaluator on the maps of its own run)
    if not plain:
        return
    opt = opts().parse(args)
    opt.save_dir = str(tmp_path / "exp_plain")
    del seen[:]
    out = driver.run_test(opt)
    assert "pixel" not in out and not seen and not os.path.exists(os.path.join(opt.save_dir, pl.RESULT_FILE))
    assert "nIoU" not in capsys.readouterr().out


def _gt_of(out, opt, img_id):
    from centerpoly_amd.datasets.evaluation import instance_level as il
    ds = out["dataset"]
    proto = il.PROTOCOLS[getattr(ds, "ap_protocol", None) or "cityscapes"]
    files = il.find_gt_files(opt.gt_dir, proto)
    return il.read_gt_ids(files[proto.image_key(ds.coco.loadImgs(ids=[img_id])[0]["file_name"])])


def test_driver_kitti(tmp_path, monkeypatch, capsys):
    with contextlib.redirect_stderr(io.StringIO()):
        _drive(_kitti_set(str(tmp_path)), tmp_path, monkeypatch, capsys, "kitti", 2)


def test_driver_cityscapes(tmp_path, monkeypatch, capsys):
    import test_writer_instances as twi
    args = twi._cityscapes_set(str(tmp_path)) + ["--no_mask_files", "--not_prefetch_test"]
    _drive(args, tmp_path, monkeypatch, capsys, "cityscapes", 4, plain=False)

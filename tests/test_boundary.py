"""cp_boundary_overlaps on the device against the host statement (tests/golden/boundary_host.py, the literal ring of
zeros and d 3 x 3 minima), and Boundary AP end to end through score_instances_device of both writer mixins.  Everything
is integer: every comparison of bands and tables is exact; the AP numbers are compared within 1e-12 (sums of a few
float64 ratios in another order at most)."""
import ctypes
import os
import types

import numpy as np
import pytest

import boundary_cases
import boundary_host as bh
from centerpoly_amd import _C
from centerpoly_amd.datasets.evaluation import boundary as bd
from centerpoly_amd.datasets.evaluation import instance_level as il

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = {c["name"]: c for c in boundary_cases.all_cases()}
_REFERENCE = {}


def _reference(name):
    """The host statement's result of a case, computed once."""
    if name not in _REFERENCE:
        c = CASES[name]
        _REFERENCE[name] = bh.boundary_counts(c["masks"], c["ids"], c["inst_ids"], c["d"], c["bounds"])
    return _REFERENCE[name]


def _device(c):
    """The case's inputs on the device: (masks, ids, bounds)."""
    import torch
    dev = torch.device("cuda")
    n, H, W = c["masks"].shape
    if c["offset"]:                                                       # planes one byte off a 16-byte boundary
        flat = torch.zeros((n * H * W + 1,), dtype=torch.uint8, device=dev)
        masks = flat[1:].view(n, H, W)
        masks.copy_(torch.from_numpy(c["masks"]))
        assert masks.data_ptr() % 16 == 1 and masks.is_contiguous()
    else:
        masks = torch.from_numpy(c["masks"]).to(dev)
    bounds = None if c["bounds"] is None else torch.from_numpy(c["bounds"]).to(dev)
    return masks, il.device_ids(c["ids"], dev), bounds


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_bands_and_tables_against_the_host_statement(name):
    c = CASES[name]
    masks, ids, bounds = _device(c)
    b_inter, b_pred, b_gt, pbands, gband = bd.device_boundary_counts(masks, ids, c["inst_ids"], c["d"], bounds, True)
    want = _reference(name)
    assert np.array_equal(gband.cpu().numpy(), want[4])
    assert np.array_equal(pbands.cpu().numpy(), want[3])
    assert np.array_equal(b_pred, want[1]) and np.array_equal(b_gt, want[2]) and np.array_equal(b_inter, want[0])
    assert b_inter.shape == (len(c["masks"]), len(c["inst_ids"]))
    # without the band images: the same tables
    again = bd.device_boundary_counts(masks, ids, c["inst_ids"], c["d"], bounds)
    for a, b in zip(again, (b_inter, b_pred, b_gt)):
        assert np.array_equal(a, b)


@pytest.mark.gpu
def test_more_masks_and_ids_than_one_call_takes():
    """130 masks: two slices of the wrapper; every slice counts the ground-truth side again and agrees."""
    c = CASES["24x40_n128_d2"]
    import torch
    masks = np.concatenate([c["masks"], c["masks"][:2]])
    got = bd.device_boundary_counts(torch.from_numpy(masks).cuda(), il.device_ids(c["ids"], torch.device("cuda")),
                                    c["inst_ids"], c["d"])
    want = _reference("24x40_n128_d2")
    assert np.array_equal(got[0][:128], want[0]) and np.array_equal(got[0][128:], want[0][:2])
    assert np.array_equal(got[1][:128], want[1]) and np.array_equal(got[2], want[2])


@pytest.mark.gpu
def test_two_runs_give_the_same_bits():
    c = CASES["70x75_shapes_d11"]
    masks, ids, bounds = _device(c)
    runs = [bd.device_boundary_counts(masks, ids, c["inst_ids"], c["d"], bounds, True) for _ in range(2)]
    for a, b in zip(*runs):
        a, b = (a.cpu().numpy(), b.cpu().numpy()) if hasattr(a, "cpu") else (a, b)
        assert a.tobytes() == b.tobytes()


@pytest.mark.gpu
def test_refusals_write_nothing():
    import torch
    assert boundary_cases.refusals() == 23
    dev = torch.device("cuda")
    L = _C.lib()
    n, G, H, W = 2, 3, 10, 12
    masks = torch.ones((n, H, W), dtype=torch.uint8, device=dev)
    ids = torch.zeros((H, W), dtype=torch.int16, device=dev)
    inst = torch.tensor([0, 1, 2], dtype=torch.int32, device=dev)
    out = torch.full((n * G + n + G,), -7, dtype=torch.int32, device=dev)
    bands = torch.full((n + 1, H, W), 77, dtype=torch.uint8, device=dev)
    need = L.cp_boundary_overlaps_workspace_bytes(n, G, H, W, 2)
    ws = torch.full((need,), 99, dtype=torch.uint8, device=dev)
    at = lambda o: ctypes.c_void_p(out.data_ptr() + 4 * o)                # noqa: E731

    def call(n_=n, G_=G, d=2, ws_bytes=need, ids_=ids):
        return L.cp_boundary_overlaps(_C.ptr(masks), n_, None, _C.ptr(ids_) if ids_ is not None else None, H, W, d,
                                      _C.ptr(inst), G_, at(0), at(n * G), at(n * G + n), _C.ptr(bands[:n]),
                                      _C.ptr(bands[n]), _C.ptr(ws), ws_bytes, _C.stream())
    assert call(n_=129) == -2 and call(G_=1025) == -2 and call(d=65) == -2 and call(d=0) == -1
    assert call(ws_bytes=need - 1) == -3 and call(ids_=None) == -1
    torch.cuda.synchronize()
    assert (out == -7).all() and (bands == 77).all() and (ws == 99).all()
    assert call() == 0                                                    # and the same call, valid, writes all of it
    torch.cuda.synchronize()
    assert not (out == -7).any() and not (bands == 77).any()


# ------------------------------------------------------------------------------------------- end to end --


def _golden(kind, name):
    return np.load(os.path.join(HERE, "golden", "%s_%s.npz" % (kind, name)), allow_pickle=False)


def _cityscapes(name):
    """(data set, rows [R, 2N + 7], gt ids, the masks score_instances_device draws)."""
    from centerpoly_amd.datasets.dataset.polygons import CITYSCAPES
    z = _golden("writer", name)
    det = {c: z["det_%d" % c] for c in sorted(int(k[4:]) for k in z.files if k.startswith("det_"))}
    rows = [np.concatenate([r[:, :5], np.full((len(r), 1), c - 1, np.float32), r[:, 5:]], axis=1)
            for c, r in sorted(det.items())]
    rows = np.ascontiguousarray(np.concatenate(rows, axis=0), np.float32)
    ds = CITYSCAPES.__new__(CITYSCAPES)
    ds.opt = types.SimpleNamespace(thresh=0.05)
    masks, _ = ds.instance_masks_device(ds.image_instances(det))
    return ds, rows, _golden("instance_ap", name)["gt_ids"], masks


def _class_writer(name):
    import torch
    from centerpoly_amd.datasets.dataset.polygons import IDD, KITTIPOLY
    z = _golden("class_writer", name)
    cls = KITTIPOLY if name.startswith("kitti") else IDD
    ds = cls.__new__(cls)
    ds.opt = types.SimpleNamespace(thresh=0.3)
    masks = np.unpackbits(z["packed"], axis=2)[:, :, :int(z["width"])].astype(np.uint8) * 255
    return ds, z["rows"], _golden("kitti_idd_ap", name)["gt_ids"], torch.from_numpy(masks).cuda()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["star16", "mixed32", "kitti_a", "idd_a"])
def test_score_instances_device_with_a_boundary_evaluator(name):
    import torch
    city = name in ("star16", "mixed32")
    ds, rows, gt_ids, masks = _cityscapes(name) if city else _class_writer(name)
    proto = il.CITYSCAPES if city else ds.protocol()
    rows_dev = torch.from_numpy(rows).cuda()
    plain, plain0, ev = il.InstanceLevelEvaluator(proto), il.InstanceLevelEvaluator(proto), bd.BoundaryEvaluator(proto)
    res = ds.score_instances_device(rows_dev, gt_ids, evaluator=plain, boundary=ev)
    # boundary=None: the tables of today, and the same ones beside the band tables
    res0 = ds.score_instances_device(rows_dev, gt_ids, evaluator=plain0)
    assert set(res) - set(res0) == {"b_inter", "b_pred", "b_gt", "band_width"}
    for k, v in res0.items():
        assert np.array_equal(np.asarray(v), np.asarray(res[k])), k
    assert np.array_equal(plain.ap_matrix(), plain0.ap_matrix(), equal_nan=True)
    H, W = gt_ids.shape
    d = bd.band_width(H, W)
    assert res["band_width"] == d == {(1024, 2048): 11, (375, 1242): 6, (720, 1280): 7}[(H, W)]
    n, table = res["n"], res["gt_table"]
    assert n == len(masks) and n > 3 and len(table) > 3
    # the kernel on the same masks without bounds, and the host statement
    gt_dev = il.device_ids(gt_ids, torch.device("cuda"))
    dev_tables = bd.device_boundary_counts(masks, gt_dev, table[:, 0], d)
    host_tables = bh.boundary_tables(masks.cpu().numpy(), gt_ids, table[:, 0], d)
    for k, a, b in zip(("b_inter", "b_pred", "b_gt"), dev_tables, host_tables):
        assert np.array_equal(res[k], a), k
        assert np.array_equal(res[k], b), k
    assert res["b_pred"].any() and res["b_gt"].any() and res["b_inter"].any()
    # the protocol on the host statement's tables
    rows_kept = res["kept"] if city else list(range(n))
    pix = (masks.cpu().numpy() != 0).reshape(n, -1).sum(1)
    host = bd.BoundaryEvaluator(proto)
    host.band_width(H, W)
    host.add_counts(table, res["labels"][rows_kept].tolist(), [float(c) for c in res["conf_text"]], pix[rows_kept],
                    res["void"][rows_kept], res["inter"][rows_kept], host_tables[1][rows_kept], host_tables[2],
                    host_tables[0][rows_kept])
    got, want = ev.summarize(), host.summarize()
    for k in ("resultBoundaryApMatrix", "resultApMatrix"):
        np.testing.assert_allclose(got[k], want[k], rtol=0, atol=1e-12, equal_nan=True)
    for k in ("allBoundaryAp", "allBoundaryAp50%", "allAp", "allAp50%"):
        np.testing.assert_allclose(got[k], want[k], rtol=0, atol=1e-12, equal_nan=True)
    assert got["bandWidths"] == want["bandWidths"] == {"%dx%d" % (H, W): d}
    assert np.array_equal(got["resultApMatrix"], plain.ap_matrix(), equal_nan=True)      # the plain AP beside it
    with np.errstate(invalid="ignore"):
        assert not (got["resultBoundaryApMatrix"] > got["resultApMatrix"] + 1e-12).any()
    # the evaluator's own image path (mask files made anywhere) gives the same tables
    ev2 = bd.BoundaryEvaluator(proto)
    ev2.add_image(masks[rows_kept], res["labels"][rows_kept].tolist(), [float(c) for c in res["conf_text"]], gt_ids)
    np.testing.assert_allclose(ev2.summarize()["resultBoundaryApMatrix"], got["resultBoundaryApMatrix"], rtol=0,
                               atol=1e-12, equal_nan=True)


@pytest.mark.gpu
def test_a_ratio_beyond_the_kernels_band_is_refused_at_the_first_image():
    import torch
    ds, rows, gt_ids, _ = _class_writer("kitti_a")
    ev = bd.BoundaryEvaluator(ds.protocol(), 0.06)
    with pytest.raises(ValueError, match=r"d = 78 pixels on a 1242 x 375 image"):
        ds.score_instances_device(torch.from_numpy(rows).cuda(), gt_ids, boundary=ev)
    assert not ev.images


# ------------------------------------------------------------------------------------------- the driver --
def _cityscapes_set(tmp, cases=("star16", "mixed32")):
    """Two seeded 2048 x 1024 images with fixture id images as ground truth and a seeded DLA-34 whose `poly` bias is a
    16-gon of 6 to 10 output pixels radius (a random head's polygons are a pixel or two, which the writer's 100-pixel
    rule drops), saved as a checkpoint: the arguments of test.py."""
    import json

    import torch
    from PIL import Image
    from centerpoly_amd.models.model import create_model, save_model
    rng = np.random.RandomState(11)
    img_dir, annot_dir, gt_dir = os.path.join(tmp, "images"), os.path.join(tmp, "BBoxes"), os.path.join(tmp, "gtFine")
    for d in (img_dir, annot_dir, os.path.join(gt_dir, "val", "frankfurt")):
        os.makedirs(d)
    images = []
    for k, c in enumerate(cases):
        coarse = rng.randint(0, 256, (32, 64, 3)).astype(np.uint8)
        img = np.kron(coarse, np.ones((32, 32, 1), np.uint8)) // 2 + rng.randint(0, 128, (1024, 2048, 3)).astype(np.uint8)
        Image.fromarray(img.astype(np.uint8)).save(os.path.join(img_dir, "frankfurt_%s_leftImg8bit.png" % c),
                                                   compress_level=1)
        Image.fromarray(_golden("instance_ap", c)["gt_ids"]).save(
            os.path.join(gt_dir, "val", "frankfurt", "frankfurt_%s_gtFine_instanceIds.png" % c))
        images.append({"id": 10 + k, "file_name": "frankfurt_%s_leftImg8bit.png" % c, "height": 1024, "width": 2048})
    with open(os.path.join(annot_dir, "val16_regular_interval.json"), "w") as f:
        json.dump({"images": images, "annotations": [], "categories": []}, f)
    torch.manual_seed(23)
    model = create_model("dla_34", {"hm": 8, "poly": 32, "pseudo_depth": 1, "reg": 2}, 256)
    with torch.no_grad():
        ang = np.arange(16) * (2 * np.pi / 16)
        rad = rng.uniform(6, 10, 16)
        bias = np.stack([rad * np.cos(ang), rad * np.sin(ang)], 1).reshape(-1)
        model.state_dict()["poly.2.bias"].copy_(torch.from_numpy(bias.astype(np.float32)))
        model.state_dict()["hm.2.bias"].fill_(-1.0)
    ckpt = os.path.join(tmp, "model_seeded.pth")
    save_model(ckpt, 1, model)
    return ["polydet", "--dataset", "cityscapes", "--annot_dir", annot_dir, "--img_dir", img_dir, "--gt_dir", gt_dir,
            "--load_model", ckpt, "--thresh", "0.05", "--num_workers", "2"]


@pytest.mark.gpu
def test_driver_prints_and_writes_the_boundary_ap(tmp_path, capsys):
    """test.py --boundary with --test_batch_size 2: both tables, both JSON files, "boundary" in the returned dict; the
    mask files it wrote score the same through evaluate_result_dir (files -> add_image, no bounds)."""
    import importlib.util
    import json

    from centerpoly_amd.opts import opts
    root = os.path.dirname(HERE)
    spec = importlib.util.spec_from_file_location("centerpoly_test_driver", os.path.join(root, "test.py"))
    driver = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(driver)
    opt = opts().parse(_cityscapes_set(str(tmp_path)) + ["--boundary", "--test_batch_size", "2"])
    opt.save_dir = str(tmp_path / "exp")
    out = driver.run_test(opt)
    text = capsys.readouterr().out
    assert "AP_50%" in text and "bAP_50%" in text and "11 px at 1024x2048" in text
    res = out["boundary"]
    assert res["ratio"] == 0.005 and res["bandWidths"] == {"1024x2048": 11}
    assert res["allAp"] == out["ap"] and not np.isnan(res["allBoundaryAp"])
    tables = out["dataset"].last_evaluator.images
    assert any((p[4] > 0).any() for _, preds in tables for p in preds), "no mask met the ground truth"
    js = json.load(open(os.path.join(opt.save_dir, bd.RESULT_FILE)))
    np.testing.assert_allclose(js["averages"]["allBoundaryAp"], res["allBoundaryAp"], rtol=0, atol=0)
    assert os.path.exists(os.path.join(opt.save_dir, "results", "evaluationResults",
                                       "resultInstanceLevelSemanticLabeling.json"))
    files = bd.evaluate_result_dir(os.path.join(opt.save_dir, "results"), sorted(il.find_gt_files(opt.gt_dir).values()))
    for k in ("resultBoundaryApMatrix", "resultApMatrix"):
        np.testing.assert_allclose(files[k], res[k], rtol=0, atol=1e-12, equal_nan=True)

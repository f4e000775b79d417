"""cp_panoptic_pairs / cp_panoptic_match on the device against their host restatement (tests/golden/panoptic_host.py),
exact, and the panoptic evaluator end to end: instance maps, the files --save_panoptic writes, test.py --panoptic."""
import contextlib
import ctypes
import io
import json
import os

import numpy as np
import pytest

import panoptic_host as host
from centerpoly_amd import _C
from centerpoly_amd.datasets.evaluation import panoptic as pq
from test_panoptic_cpu import CASES, P, assert_results, close, gt_ids, rec

pytestmark = pytest.mark.gpu
ROWS = 1025
EINVAL, EUNSUPPORTED, EWORKSPACE = -1, -2, -3


def at(t, off=0):
    return ctypes.c_void_p(t.data_ptr() + off)


def run(index, n, labels, ids, L=None, flags=None, index_offset=0, ids_offset=0, stat=None, iou=None, bad=None,
        fill=-9):
    """Both entry points on host arrays index uint8 [H, W] and ids uint16 [H, W], uploaded `index_offset` bytes /
    `ids_offset` elements into their buffers.  Returns (seg, pairs) cut to the rows the call writes, and (stat, iou, bad,
    match) as the device leaves them; the run-long tables start from the given ones."""
    import torch
    dev = torch.device("cuda")
    H, W = index.shape
    L = P.L if L is None else L
    flags = np.ascontiguousarray(P.flags[:L] if flags is None else flags, np.uint8)
    labels = np.ascontiguousarray(labels, np.int32)
    xbuf = torch.zeros(H * W + index_offset + 16, dtype=torch.uint8, device=dev)
    ibuf = torch.zeros(H * W + ids_offset + 16, dtype=torch.int16, device=dev)
    xbuf[index_offset:index_offset + H * W] = torch.from_numpy(np.ascontiguousarray(index).reshape(-1)).to(dev)
    ibuf[ids_offset:ids_offset + H * W] = torch.from_numpy(np.ascontiguousarray(ids).view(np.int16).reshape(-1)).to(dev)
    seg = torch.full((ROWS, 4), fill, dtype=torch.int32, device=dev)
    pairs = torch.full((ROWS * (n + 1),), fill, dtype=torch.int32, device=dev)
    stat_dev = torch.from_numpy(np.zeros((L, 3), np.int64) if stat is None else np.array(stat, np.int64)).to(dev)
    iou_dev = torch.from_numpy(np.zeros((L,), np.float64) if iou is None else np.array(iou, np.float64)).to(dev)
    bad_dev = torch.from_numpy(np.zeros((2,), np.int32) if bad is None else np.array(bad, np.int32)).to(dev)
    match = torch.full((max(n, 1),), fill, dtype=torch.int32, device=dev)
    lib = _C.lib()
    nbytes = lib.cp_panoptic_pairs_workspace_bytes()
    ws = _C.workspace(nbytes, dev)
    fp = flags.ctypes.data_as(ctypes.c_void_p)
    _C.check(lib.cp_panoptic_pairs(at(xbuf, index_offset), n, at(ibuf, 2 * ids_offset), H, W, P.id_divisor,
                                   P.id_direct_below, L, fp, at(seg), at(pairs), at(ws), nbytes, _C.stream()),
             "cp_panoptic_pairs")
    _C.check(lib.cp_panoptic_match(at(seg), at(pairs), n, labels.ctypes.data_as(ctypes.c_void_p) if n else None, L, fp,
                                   at(stat_dev), at(iou_dev), at(bad_dev), at(match), _C.stream()), "cp_panoptic_match")
    torch.cuda.synchronize()
    seg_h = seg.cpu().numpy().astype(np.int64)
    R = min(int(seg_h[0, 0]), 1024) + 1
    return (seg_h[:R], pairs.cpu().numpy().astype(np.int64).reshape(ROWS, n + 1)[:R], stat_dev.cpu().numpy(),
            iou_dev.cpu().numpy(), bad_dev.cpu().numpy().astype(np.int64), match.cpu().numpy().astype(np.int64)[:n])


def want(index, n, labels, ids, L=None, flags=None, stat=None, iou=None, bad=None):
    L = P.L if L is None else L
    flags = P.flags[:L] if flags is None else flags
    seg, pairs = host.panoptic_pairs(index, n, ids, P.id_divisor, P.id_direct_below, L, flags)
    return (seg, pairs) + host.panoptic_match(seg, pairs, n, labels, L, flags, stat, iou, bad)


def same(got, exp):
    for g, e, what in zip(got, exp, ("seg", "pairs", "stat", "iou", "bad", "match")):
        if what == "iou":
            assert all(close(a, b) for a, b in zip(g, e)), (what, g, e)
        else:
            assert np.array_equal(g, e), (what, g, e)


@pytest.mark.parametrize("name", CASES)
def test_fixtures_from_unaligned_buffers(name):
    z = rec(name)
    index, labels, ids = z["index"], z["labels"], gt_ids(name)
    n = len(labels)
    got = run(index, n, labels, ids, index_offset=1, ids_offset=1)
    same(got, want(index, n, labels, ids))
    assert np.array_equal(got[0], z["seg"]) and np.array_equal(got[1], z["pairs"]) and np.array_equal(got[2], z["stat"])
    assert all(close(a, b) for a, b in zip(got[3], z["iou"]))
    again = run(index, n, labels, ids)                                    # aligned this time: the same bits
    for g, a in zip(got, again):
        assert g.tobytes() == a.tobytes()


@pytest.mark.parametrize("shape", [(1, 1), (1, 17), (19, 1)])
def test_tiny_shapes(shape):
    rng = np.random.RandomState(shape[0] * 100 + shape[1])
    ids = rng.choice(np.array([7, 26001, 24002, 0], np.uint16), shape)
    index = rng.choice(np.array([0, 1, 255], np.uint8), shape)
    for offsets in ((0, 0), (3, 5)):
        same(run(index, 2, [26, 24], ids, index_offset=offsets[0], ids_offset=offsets[1]), want(index, 2, [26, 24], ids))


def test_no_slots_and_all_void():
    rng = np.random.RandomState(4)
    ids = rng.choice(np.array([7, 26001, 24002, 3], np.uint16), (21, 35))
    index = rng.choice(np.array([0, 9, 255], np.uint8), ids.shape)
    got = run(index, 0, [], ids)                                         # n == 0: every pixel in column 0
    same(got, want(index, 0, [], ids))
    assert got[1].shape == (4, 1) and got[2][:, 2].sum() == 3 and got[5].shape == (0,)
    void = rng.choice(np.array([0, 3, 29001, 35000, 65535], np.uint16), ids.shape)       # ignored labels, labels >= L
    got = run(index % 2, 1, [26], void)
    same(got, want(index % 2, 1, [26], void))
    assert got[0].tolist() == [[0, void.size, 0, 0]] and got[2][26].tolist() == [0, 0, 0] and got[5].tolist() == [0]
    # (the slot lies wholly on VOID: neither matched nor a false positive)


def random_image(G, n, seed, first=24001):
    """64 x 512 with every one of G segment values and n slots present, in random runs."""
    rng = np.random.RandomState(seed)
    values = np.concatenate([np.arange(G), rng.randint(0, G, 64 * 512 - G)])
    rng.shuffle(values)
    ids = (first + values).reshape(64, 512).astype(np.uint16)
    index = rng.randint(0, n + 1, ids.shape).astype(np.uint8)
    index[index == n] = 255
    index[0, :n] = np.arange(n)
    return ids, index


def test_large_table_regime():
    ids, index = random_image(1024, 255, 1)                              # 24001 .. 25024: 1025 x 256 cells, global atomics
    labels = 24 + np.arange(255) % 2
    got = run(index, 255, labels, ids)
    same(got, want(index, 255, labels, ids))
    assert got[0][0, 0] == 1024 and (got[1] > 0).sum() > 15360 and got[1].sum() == ids.size


def test_small_table_regime():
    ids, index = random_image(5, 3, 2, first=26001)
    ids[10:40, 100:400] = 26003                                          # something to match
    index[10:40, 100:400] = 1
    got = run(index, 3, [26, 26, 24], ids)
    same(got, want(index, 3, [26, 26, 24], ids))
    assert got[0][0, 0] == 5 and got[2][26, 0] == 1 and got[5][1] == 3


def test_one_pair_and_checkerboard():
    ids = np.full((64, 512), 26007, np.uint16)
    index = np.zeros((64, 512), np.uint8)
    got = run(index, 1, [26], ids)
    same(got, want(index, 1, [26], ids))
    assert got[1].tolist() == [[0, 0], [64 * 512, 0]] and got[2][26].tolist() == [1, 0, 0] and got[3][26] == 1.0
    k = np.add.outer(np.arange(64), np.arange(512))                      # (x + y) % 2: a lane's 16 pixels alternate
    ids = np.where(k % 2 == 0, 26001, 24002).astype(np.uint16)
    index = (k % 2).astype(np.uint8)
    got = run(index, 2, [26, 24], ids)                                   # no run longer than one
    same(got, want(index, 2, [26, 24], ids))
    assert got[2][:, 0].sum() == 2 and (got[1] > 0).sum() == 2


def test_more_than_1024_segments():
    values = (np.arange(40 * 55) % 1100 + 24001).astype(np.uint16).reshape(40, 55)
    index = (np.arange(40 * 55) % 3).astype(np.uint8).reshape(40, 55)
    preset = (np.full((P.L, 3), 5, np.int64), np.full((P.L,), 0.25), np.array([2, 1], np.int32))
    got = run(index, 3, [24, 25, 26], values, stat=preset[0], iou=preset[1], bad=preset[2])
    exp = want(index, 3, [24, 25, 26], values, stat=preset[0], iou=preset[1], bad=preset[2])
    same(got, exp)
    assert got[0][0, 0] == 1100 and got[0].shape == (1025, 4) and got[0][1024, 0] == 24001 + 1023
    assert got[1].sum() == 1024 * 2 and got[4].tolist() == [3, 1] and got[5].tolist() == [-1, -1, -1]
    assert np.array_equal(got[2], preset[0]) and got[3].tobytes() == preset[1].tobytes()      # stat and iou untouched
    import torch
    ev = pq.PanopticEvaluator(P)                                         # the host half: results() names the count
    for _ in range(2):
        ev.add_index(torch.from_numpy(index).cuda(), 3, [24, 25, 26], values, "crowded")
    with pytest.raises(ValueError, match="2 images hold more than 1024 ground-truth segments"):
        ev.results()


def test_more_than_1024_segments_in_the_large_table_regime():
    """G > 1024 with n = 255: 1025 x 256 cells go through the global atomics, and the dropped segments' pixels are
    counted nowhere."""
    ids, index = random_image(1100, 255, 6)
    labels = 24 + np.arange(255) % 2
    got = run(index, 255, labels, ids)
    same(got, want(index, 255, labels, ids))
    kept = (ids <= 24001 + 1023).sum()
    assert got[0][0, 0] == 1100 and got[1].shape == (1025, 256) and got[1].sum() == kept < ids.size
    assert got[4].tolist() == [1, 0] and not got[2].any() and (got[5] == -1).all()


def test_unevaluated_slot_label_and_labels_past_the_table():
    rng = np.random.RandomState(8)
    ids = rng.choice(np.array([7, 26001, 33001, 34001, 40000], np.uint16), (25, 33))
    index = rng.choice(np.array([0, 1, 2, 3, 255], np.uint8), ids.shape)
    labels = [26, 29, 99, -4]                                            # ignored, past the table, negative
    got = run(index, 4, labels, ids)
    same(got, want(index, 4, labels, ids))
    assert got[4].tolist() == [0, 3] and got[5].tolist() == [0, -1, -1, -1]
    assert got[0][1:, 0].tolist() == [7, 26001, 33001] and got[0][0, 1] == np.isin(ids, [34001, 40000]).sum()
    import torch
    ev = pq.PanopticEvaluator(P)                                         # the host half: results() names the count
    ev.add_index(torch.from_numpy(index).cuda(), 4, labels, ids, "odd labels")
    with pytest.raises(ValueError, match="3 predicted segments carry a label that is not evaluated"):
        ev.results()
    with pytest.raises(ValueError, match="odd labels: the ground truth is torch.float16"):
        ev.add_index(torch.from_numpy(index).cuda(), 4, labels, torch.zeros(ids.shape, dtype=torch.float16, device="cuda"),
                     "odd labels")
    got = run(index, 4, labels, ids, L=33)                               # a shorter table: label 33 is VOID too
    same(got, want(index, 4, labels, ids, L=33))
    assert got[0][1:, 0].tolist() == [7, 26001]


def test_accumulation_and_order():
    tables = [None, None, None]
    exp = [None, None, None]
    for name in ("odd37x53", "edge31x47"):
        z = rec(name)
        got = run(z["index"], len(z["labels"]), z["labels"], gt_ids(name), stat=tables[0], iou=tables[1], bad=tables[2])
        tables = list(got[2:5])
        exp = list(host.panoptic_match(z["seg"], z["pairs"], len(z["labels"]), z["labels"], P.L, P.flags, *exp)[:3])
    assert np.array_equal(tables[0], exp[0]) and tables[2].tolist() == [0, 0]
    assert all(close(x, y) for x, y in zip(tables[1], exp[1]))
    assert tables[0][:, 0].sum() == 5
    import torch
    forward, backward = pq.PanopticEvaluator(P), pq.PanopticEvaluator(P)
    for ev, order in ((forward, CASES), (backward, CASES[::-1])):
        for name in order:
            z = rec(name)
            ev.add_index(torch.from_numpy(z["index"]).cuda(), len(z["labels"]), z["labels"], gt_ids(name), name)
    a, b = forward.tables(), backward.tables()
    assert np.array_equal(a[0], b[0]) and all(close(x, y) for x, y in zip(a[1], b[1]))
    with open(os.path.join(os.path.dirname(__file__), "golden", "panoptic_set.json")) as f:
        ref = json.load(f)
    assert_results(forward.results(), ref["result"])
    assert all(close(x, ref["stat"].get(str(l), [0, 0, 0, 0.0])[3]) for l, x in enumerate(forward.tables()[1]))


def test_argument_errors_leave_the_outputs_untouched():
    import torch
    dev = torch.device("cuda")
    lib = _C.lib()
    need = lib.cp_panoptic_pairs_workspace_bytes()
    assert need >= 65536 * 3 and "cp_panoptic_pairs" in _C.EXPORTS and "cp_panoptic_match" in _C.EXPORTS
    index = torch.zeros(64, dtype=torch.uint8, device=dev)
    ids = torch.zeros(64, dtype=torch.int16, device=dev)
    seg = torch.full((ROWS, 4), 77, dtype=torch.int32, device=dev)
    pairs = torch.full((ROWS * 256,), 77, dtype=torch.int32, device=dev)
    stat = torch.full((64, 3), 77, dtype=torch.int64, device=dev)
    iou = torch.full((64,), 77.0, dtype=torch.float64, device=dev)
    bad = torch.full((2,), 77, dtype=torch.int32, device=dev)
    match = torch.full((256,), 77, dtype=torch.int32, device=dev)
    ws = _C.workspace(need, dev)
    flags = np.ones(65, np.uint8)
    labels = np.zeros(256, np.int32)
    hp = lambda a: a.ctypes.data_as(ctypes.c_void_p)                               # noqa: E731

    def pairs_call(**over):
        a = dict(index=at(index), n=2, ids=at(ids), H=8, W=8, div=1000, below=1000, L=34, flags=hp(flags), seg=at(seg),
                 pairs=at(pairs), ws=at(ws), nbytes=need)
        a.update(over)
        return lib.cp_panoptic_pairs(a["index"], a["n"], a["ids"], a["H"], a["W"], a["div"], a["below"], a["L"], a["flags"],
                                     a["seg"], a["pairs"], a["ws"], a["nbytes"], _C.stream())

    def match_call(**over):
        a = dict(seg=at(seg), pairs=at(pairs), n=2, labels=hp(labels), L=34, flags=hp(flags), stat=at(stat), iou=at(iou),
                 bad=at(bad), match=at(match))
        a.update(over)
        return lib.cp_panoptic_match(a["seg"], a["pairs"], a["n"], a["labels"], a["L"], a["flags"], a["stat"], a["iou"],
                                     a["bad"], a["match"], _C.stream())

    for name in ("index", "ids", "flags", "seg", "pairs"):
        assert pairs_call(**{name: None}) == EINVAL, name
    for over in ({"H": 0}, {"W": -1}, {"L": 0}, {"n": -1}, {"div": 0}, {"below": -1}):
        assert pairs_call(**over) == EINVAL, over
    for over in ({"n": 256}, {"L": 65}, {"H": 65536, "W": 32768}):                 # H * W == 2^31, by the sizes alone
        assert pairs_call(**over) == EUNSUPPORTED, over
    assert pairs_call(nbytes=need - 1) == EWORKSPACE and pairs_call(ws=None) == EWORKSPACE
    for name in ("seg", "pairs", "labels", "flags", "stat", "iou", "bad"):
        assert match_call(**{name: None}) == EINVAL, name
    assert match_call(n=-1) == EINVAL and match_call(L=0) == EINVAL
    assert match_call(n=256) == EUNSUPPORTED and match_call(L=65) == EUNSUPPORTED
    torch.cuda.synchronize()
    for t in (seg, pairs, stat, bad, match):
        assert bool((t == 77).all())
    assert bool((iou == 77.0).all())


def _maps_and_gt():
    import torch
    import test_instances_api as tia
    from centerpoly_amd.detectors import instances
    ds = tia._dataset("cityscapes")
    rows = tia._rows(len(ds.class_name) - 1)
    maps = instances.instance_maps(torch.from_numpy(rows).cuda(), ds, (tia.W, tia.H))
    # ground truth: the prediction's own ids shifted by 9 pixels over road, a strip of VOID and a car crowd region
    gt = np.roll(maps.ids.cpu().numpy(), 9, axis=1).astype(np.uint16)
    gt[gt == 0] = 7
    gt[:6, :] = 0
    gt[-8:, :40] = 26
    return maps, gt


def test_add_maps_equals_the_written_files_and_the_host(tmp_path):
    import torch
    from PIL import Image
    maps, gt = _maps_and_gt()
    stem = "frankfurt_a_leftImg8bit"
    ev = pq.PanopticEvaluator(P)
    ev.add_maps(maps, torch.from_numpy(gt.view(np.int16)).cuda(), stem)
    got = ev.results()
    t = maps.table
    seg, pairs = host.panoptic_pairs(maps.index.cpu().numpy(), t["n"], gt, 1000, 1000, P.L, P.flags)
    stat, iou, bad, match = host.panoptic_match(seg, pairs, t["n"], t["label"], P.L, P.flags)
    by_host = pq.PanopticEvaluator(P)
    by_host.add_stats(stat, iou)
    assert np.array_equal(ev.tables()[0], stat) and all(close(x, y) for x, y in zip(ev.tables()[1], iou))
    assert stat[:, 0].sum() >= 1 and stat[7, 2] == 1 and 0 < got["Things"]["pq"] < 1
    out = str(tmp_path / "panoptic")
    entry = pq.save_panoptic(maps, out, stem)
    assert entry["image_id"] == "frankfurt_a" and entry["file_name"] == stem + "_panoptic.png"
    owners = np.unique(maps.ids.cpu().numpy())
    assert sorted(s["id"] for s in entry["segments_info"]) == [int(v) for v in owners if v]
    for s in entry["segments_info"]:
        ys, xs = np.nonzero(maps.ids.cpu().numpy() == s["id"])
        assert s["area"] == len(ys) and s["bbox"] == [xs.min(), ys.min(), xs.max() - xs.min() + 1, ys.max() - ys.min() + 1]
        assert s["category_id"] == s["id"] // 1000 and s["iscrowd"] == 0
    path = pq.write_panoptic_json(out, [entry])
    assert os.path.basename(path) == "cityscapes_panoptic_val.json"
    rgb = np.array(Image.open(os.path.join(out, entry["file_name"]))).astype(np.int64)
    assert np.array_equal(rgb[:, :, 0] + 256 * rgb[:, :, 1] + 65536 * rgb[:, :, 2], maps.ids.cpu().numpy())
    gt_dir = str(tmp_path / "gt")
    os.makedirs(gt_dir)
    Image.fromarray(gt).save(os.path.join(gt_dir, "frankfurt_a_gtFine_instanceIds.png"))
    by_files = pq.evaluate_result_dir(path, out, gt_dir)
    assert_results(by_host.results(), got)
    assert json.dumps(by_files, sort_keys=True) == json.dumps(got, sort_keys=True)
    # the evaluator's complaints about files that disagree
    with open(path) as f:
        doc = json.load(f)
    dropped = doc["annotations"][0]["segments_info"].pop()
    with open(path, "w") as f:
        json.dump(doc, f)
    with pytest.raises(ValueError, match="segment %d is painted in the PNG but the JSON lists no such segment" % dropped["id"]):
        pq.evaluate_result_dir(path, out, gt_dir)
    doc["annotations"][0]["segments_info"] += [dropped, {"id": 33999, "category_id": 33}]
    with open(path, "w") as f:
        json.dump(doc, f)
    with pytest.raises(ValueError, match=r"the JSON lists segments \[33999\], which own no pixel of the PNG"):
        pq.evaluate_result_dir(path, out, gt_dir)
    many = np.arange(8 * 40).reshape(8, 40) + 24001                                  # 320 segments in one image
    Image.fromarray(np.stack([many % 256, many // 256, many * 0], 2).astype(np.uint8)).save(os.path.join(out, "many.png"))
    with pytest.raises(ValueError, match="many.png: 320 segments"):
        pq.index_of_png(os.path.join(out, "many.png"), [{"id": int(v), "category_id": 24} for v in many.reshape(-1)])


def test_add_maps_copies_nothing_to_the_host(monkeypatch):
    """No tensor of the call comes back and nothing waits for the device: every way of torch's to read a tensor or to
    synchronise raises while add_maps runs (the run-long tables are read by results(), afterwards)."""
    import torch
    maps, gt = _maps_and_gt()
    gt_dev = torch.from_numpy(gt.view(np.int16)).cuda()
    ev = pq.PanopticEvaluator(P)
    ev.add_maps(maps, gt_dev)                                            # the tables exist now
    first = ev.tables()

    def refuse(*a, **k):
        raise AssertionError("add_maps reads from the device or waits for it")

    with monkeypatch.context() as m:
        for name in ("cpu", "item", "numpy", "tolist", "__bool__", "__int__", "__float__", "nonzero"):
            m.setattr(torch.Tensor, name, refuse)
        m.setattr(torch.cuda, "synchronize", refuse)
        m.setattr(torch.cuda.Stream, "synchronize", refuse)
        m.setattr(torch.cuda.Event, "synchronize", refuse)
        ev.add_maps(maps, gt_dev)
    second = ev.tables()
    assert np.array_equal(second[0], 2 * first[0]) and second[0].sum() > 0 and ev.images == 2


def test_driver_cityscapes(tmp_path, monkeypatch, capsys):
    """test.py --panoptic --save_panoptic per image and with --test_batch_size 2: the returned scores are the
    evaluator's on the maps the run saw and the ones the written files score to, the table follows the AP table, the
    JSON file is written; without the flags, no trace."""
    import test_instances_api as tia
    import test_writer_instances as twi
    from test_pixel_level import _gt_of
    from centerpoly_amd.opts import opts
    with contextlib.redirect_stderr(io.StringIO()):
        args = twi._cityscapes_set(str(tmp_path)) + ["--no_mask_files", "--not_prefetch_test"]
        seen = tia._record_instances(monkeypatch)
        driver = tia._module("test")
        for batch in (1, 2):
            opt = opts().parse(args + ["--panoptic", "--save_panoptic", "--test_batch_size", str(batch)])
            opt.save_dir = str(tmp_path / ("exp_b%d" % batch))
            del seen[:]
            out = driver.run_test(opt)
            text = capsys.readouterr().out
            assert len(seen) == 4 and "panoptic" in out and "pixel" not in out
            assert text.index("AP_50%") < text.index("Category      |    PQ     SQ     RQ") < text.index("Things        |")
            ev = pq.PanopticEvaluator(P)
            for maps, item in zip(seen, out["dataset"].images):
                ev.add_maps(maps, _gt_of(out, opt, item))
            res = ev.results()
            assert json.dumps(out["panoptic"], sort_keys=True) == json.dumps(res, sort_keys=True)
            with open(os.path.join(opt.save_dir, pq.RESULT_FILE)) as f:
                assert_results(res, json.load(f))
            assert ev.tables()[0][24:, :2].sum() > 0 and res["Stuff"]["n"] >= 1   # something was predicted
            pan_dir = os.path.join(opt.save_dir, "panoptic")
            by_files = pq.evaluate_result_dir(os.path.join(pan_dir, "cityscapes_panoptic_val.json"), pan_dir, opt.gt_dir)
            assert json.dumps(by_files, sort_keys=True) == json.dumps(res, sort_keys=True)
        opt = opts().parse(args)
        opt.save_dir = str(tmp_path / "exp_plain")
        del seen[:]
        out = driver.run_test(opt)
        assert "panoptic" not in out and not seen and not os.path.exists(os.path.join(opt.save_dir, pq.RESULT_FILE))
        assert not os.path.exists(os.path.join(opt.save_dir, "panoptic")) and "RQ" not in capsys.readouterr().out

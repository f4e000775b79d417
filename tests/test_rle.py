"""Run-length masks on the device against the host statement (tests/golden/rle_host.py): every string, count, area and
decoded byte equal.  The references are computed once per mask and shared."""
import contextlib
import ctypes
import io
import json
import os

import numpy as np
import pytest

import rle_host as host
import test_instances_api as tia
from test_rle_cpu import random_mask

pytestmark = pytest.mark.gpu

_REF = {}


def _ref(m):
    """(counts, string) of one mask by the literal statement, once per mask."""
    key = (m.shape, m.tobytes())
    if key not in _REF:
        cnts = host.encode(m.tolist())
        _REF[key] = (cnts, host.to_string(cnts))
    return _REF[key]


def _check(masks, bounds=None, value=200):
    """Planes [n, H, W] through encode (strings, counts, areas against the statement) and back through decode."""
    import torch
    from centerpoly_amd.utils import rle
    masks = np.ascontiguousarray(masks, np.uint8)
    dev = torch.from_numpy(masks).cuda()
    got = rle.encode(masks=dev, bounds=bounds, want_counts=True)
    assert len(got) == len(masks)
    for k, m in enumerate(masks):
        cnts, text = _ref(m)
        assert got[k]["size"] == list(m.shape)
        assert got[k]["cnts"].tolist() == cnts, k
        assert got[k]["counts"] == text, k
        assert got[k]["area"] == int((m != 0).sum())
    plain = rle.encode(masks=dev, bounds=bounds)                          # without the counts: the same strings
    assert [r["counts"] for r in plain] == [r["counts"] for r in got] and "cnts" not in plain[0]
    planes, status = rle.decode([{"size": r["size"], "counts": r["counts"]} for r in got], dev.device, value)
    assert planes.dtype == torch.uint8 and not status.any()
    assert bool((planes == (dev != 0) * value).all())
    return got


def _blobs(rng, H, W):
    m = np.zeros((H, W), np.uint8)
    yy, xx = np.mgrid[0:H, 0:W]
    for _ in range(4):
        cy, cx, r = rng.integers(0, H), rng.integers(0, W), rng.integers(1, max(2, min(H, W) // 2 + 1))
        m[(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = 255
    return m


def test_degenerate_canvases():
    _check(np.array([[[0]], [[1]]]))
    rng = np.random.default_rng(1)
    _check((rng.random((2, 300, 1)) < 0.5).astype(np.uint8))              # W = 1
    _check((rng.random((2, 1, 300)) < 0.5).astype(np.uint8))              # H = 1


def test_every_character_length_and_the_delta_boundaries():
    """H = 1: column-major is row-major, the counts are the runs of the row.  Deltas against cnts[i - 2] of -17, -16, -1,
    0, 15, 16, 511, 512 (the one / two / three character boundaries), then +-20000 (four) and +-600000 (five)."""
    cnts = [40, 40, 40]
    for d in (-17, -16, -1, 0, 15, 16, 511, 512, 20000, 600000, -20000, -600000):
        cnts.append(cnts[-2] + d)
    row = np.repeat(np.arange(len(cnts)) % 2, cnts).astype(np.uint8)[None, None]
    assert _ref(row[0])[0] == cnts
    lengths = [len(host.to_string([0, 0, 0, 0, d])) - 4 for d in (-17, -16, 15, 16, 511, 512, 20000, 600000, -600000)]
    assert lengths == [2, 1, 1, 2, 2, 3, 4, 5, 5]
    got = _check(row)
    assert got[0]["counts"] == host.to_string(cnts)


def test_uniform_planes_and_the_first_pixel():
    m = np.zeros((4, 9, 70), np.uint8)
    m[1] = 3
    m[2, 0, 0] = 1
    m[3, 8, 69] = 1
    got = _check(m)
    assert [r["cnts"].tolist() for r in got] == [[630], [0, 630], [0, 1, 629], [629, 1]]


def test_the_carry_between_columns():
    """M(H - 1, x - 1) and M(0, x) in all four combinations, on both sides of a tile edge (x = 64)."""
    m = np.zeros((1, 5, 130), np.uint8)
    for x, (bottom, top) in ((3, (0, 0)), (10, (0, 1)), (20, (1, 0)), (30, (1, 1)), (63, (1, 1)), (64, (1, 0)), (66, (0, 1))):
        m[0, 4, x - 1], m[0, 0, x] = bottom, top
    m = np.concatenate([m, 1 - m])
    _check(m)
    _check(m[:, :, 1:])


@pytest.mark.parametrize("W", [63, 64, 65, 130])
@pytest.mark.parametrize("H", [7, 64, 65, 257])
def test_tile_edges(H, W):
    rng = np.random.default_rng(H * 1000 + W)
    _check(np.stack([(rng.random((H, W)) < 0.5).astype(np.uint8), _blobs(rng, H, W)]))


def test_checkerboard():
    yy, xx = np.mgrid[0:37, 0:53]
    board = ((yy + xx) & 1).astype(np.uint8)
    got = _check(np.stack([board, 1 - board]))
    assert [len(r["cnts"]) for r in got] == [37 * 53, 37 * 53 + 1]


def test_128_planes():
    rng = np.random.default_rng(3)
    _check(np.stack([random_mask(rng, 40, 30) for _ in range(128)]))


def test_full_size_pair():
    """2048 x 1024: a 3 x 3 blob near the last pixel and a full plane (counts of five characters)."""
    m = np.zeros((2, 1024, 2048), np.uint8)
    m[0, 1020:1023, 2044:2047] = 1
    m[1] = 1
    got = _check(m)
    assert got[1]["counts"] == "0PPPP2" and got[0]["area"] == 9


def _boxed(rng, n, H, W, boxes):
    m = np.zeros((n, H, W), np.uint8)
    for k, (x0, y0, x1, y1) in enumerate(boxes):
        if x1 >= x0 and y1 >= y0:
            m[k, y0:y1 + 1, x0:x1 + 1] = rng.random((y1 - y0 + 1, x1 - x0 + 1)) < 0.6
    return m


def test_bounds():
    import torch
    H, W = 70, 150
    rng = np.random.default_rng(9)
    boxes = [(10, 5, 40, 30),                 # inside
             (100, 40, W - 1, H - 1),         # touches the bottom row and the right edge
             (60, 50, 70, H - 1),             # ends at x1 < W - 1 and touches row H - 1: column x1 + 1 has a change
             (63, 0, 64, H - 1),              # a full-height box across a tile edge
             (0, 0, 0, 0), (W - 1, H - 1, W - 1, H - 1),
             (W, H, -1, -1), (5, 5, 4, 9),    # empty boxes
             (0, 0, W - 1, H - 1)]
    m = _boxed(rng, len(boxes), H, W, boxes)
    m[2, H - 1, 70] = 1                       # the bottom pixel of column x1 is set
    m[3, :, 63:65] = 1
    m[4, 0, 0] = m[5, H - 1, W - 1] = 1
    b = np.array(boxes, np.int32)
    with_bounds = _check(m, bounds=b)
    without = _check(m)
    assert [r["counts"] for r in with_bounds] == [r["counts"] for r in without]
    _check(m, bounds=torch.from_numpy(b).cuda())                           # bounds already on the device
    loose = b.copy()
    loose[:, :2] -= 7                                                      # boxes larger than the masks, beyond the canvas
    loose[:, 2:] += 7
    loose[6:8] = b[6:8]
    _check(m, bounds=loose)


@pytest.mark.parametrize("n", [1, 255])
def test_index_mode(n):
    import torch
    from centerpoly_amd.utils import rle
    H, W = 29, 67
    rng = np.random.default_rng(n)
    index = rng.integers(0, n + 40, (H, W))
    index = np.where(index >= n, 255, index).astype(np.uint8)
    index[10:20, 30:50] = n - 1                                            # one larger region
    dev = torch.from_numpy(index).cuda()
    got = rle.encode(index=dev, n=n, want_counts=True)
    planes = np.stack([(index == k).astype(np.uint8) for k in range(n)])
    want = sum((rle.encode(masks=torch.from_numpy(planes[a:a + 128]).cuda(), want_counts=True)
                for a in range(0, n, 128)), [])
    assert [r["counts"] for r in got] == [r["counts"] for r in want]
    assert [r["cnts"].tolist() for r in got] == [r["cnts"].tolist() for r in want]
    assert [r["area"] for r in got] == planes.sum((1, 2)).tolist()
    for k in (0, n // 2, n - 1):
        assert got[k]["counts"] == _ref(planes[k])[1]
    box = np.array([[W, H, -1, -1] if not p.any() else
                    [np.nonzero(p.any(0))[0][0], np.nonzero(p.any(1))[0][0], np.nonzero(p.any(0))[0][-1],
                     np.nonzero(p.any(1))[0][-1]] for p in planes], np.int32)
    boxed = rle.encode(index=dev, n=n, bounds=box)
    assert [r["counts"] for r in boxed] == [r["counts"] for r in got]


def _raw_encode(dev_masks, cap_counts, cap_bytes, guard=64, fill=0xA5):
    """cp_rle_encode with `guard` bytes behind both buffers: (head, table, counts bytes, chars bytes), guards included."""
    import torch
    from centerpoly_amd import _C
    L = _C.lib()
    n, H, W = (int(v) for v in dev_masks.shape)
    counts = torch.full((4 * cap_counts + guard,), fill, dtype=torch.uint8, device=dev_masks.device)
    chars = torch.full((cap_bytes + guard,), fill, dtype=torch.uint8, device=dev_masks.device)
    table = torch.zeros((n, 4), dtype=torch.int32, device=dev_masks.device)
    head = torch.zeros((4,), dtype=torch.int32, device=dev_masks.device)
    nbytes = L.cp_rle_encode_workspace_bytes(n, H, W, cap_counts)
    ws = _C.workspace(nbytes, dev_masks.device)
    _C.check(L.cp_rle_encode(_C.ptr(dev_masks), None, n, H, W, None, _C.ptr(counts), cap_counts, _C.ptr(chars), cap_bytes,
                             _C.ptr(table), _C.ptr(head), _C.ptr(ws), nbytes, _C.stream()), "cp_rle_encode")
    return head.cpu().numpy(), table.cpu().numpy(), counts.cpu().numpy(), chars.cpu().numpy()


def test_capacities(monkeypatch):
    import torch
    from centerpoly_amd.utils import rle
    rng = np.random.default_rng(21)
    masks = np.stack([random_mask(rng, 33, 70) for _ in range(5)])
    masks[4] = (rng.random((33, 70)) < 0.5)
    dev = torch.from_numpy(masks).cuda()
    refs = [_ref(m) for m in masks]
    total_counts, total_bytes = sum(len(c) for c, _ in refs), sum(len(s) for _, s in refs)
    head, table, counts, chars = _raw_encode(dev, total_counts, total_bytes)
    assert head.tolist() == [total_counts, total_bytes, 0, 0]
    assert table[:, 0].tolist() == [len(c) for c, _ in refs] and table[:, 3].tolist() == [len(s) for _, s in refs]
    assert table[:, 1].tolist() == [int((m != 0).sum()) for m in masks]
    assert table[:, 2].tolist() == np.cumsum([0] + [len(s) for _, s in refs[:-1]]).tolist()
    assert counts[:4 * total_counts].view(np.uint32).tolist() == sum((c for c, _ in refs), [])
    assert chars[:total_bytes].tobytes().decode("ascii") == "".join(s for _, s in refs)
    assert (counts[4 * total_counts:] == 0xA5).all() and (chars[total_bytes:] == 0xA5).all()
    for cap_c, cap_b in ((total_counts - 1, total_bytes), (total_counts, total_bytes - 1), (3, 2), (0, 0)):
        h2, t2, c2, s2 = _raw_encode(dev, cap_c, cap_b)
        assert h2.tolist() == [total_counts, total_bytes, 1, 0] and np.array_equal(t2, table)
        assert np.array_equal(c2[:4 * cap_c], counts[:4 * cap_c]) and (c2[4 * cap_c:] == 0xA5).all()
        assert np.array_equal(s2[:cap_b], chars[:cap_b]) and (s2[cap_b:] == 0xA5).all()
    # the wrapper's first capacities too small: the second call, sized by the head, gives the strings
    monkeypatch.setattr(rle, "FIXED_COUNTS", 8)
    got = rle.encode(masks=dev, want_counts=True)
    assert [r["counts"] for r in got] == [s for _, s in refs] and [r["cnts"].tolist() for r in got] == [c for c, _ in refs]
    monkeypatch.setattr(rle, "RUNS_PER_COLUMN", 0)
    got = rle.encode(masks=dev, bounds=np.array([[0, 0, 69, 32]] * 5, np.int32))
    assert [r["counts"] for r in got] == [s for _, s in refs]


def test_decode_zero_length_runs_and_wrong_sums():
    import torch
    from centerpoly_amd import _C
    from centerpoly_amd.utils import rle
    H, W = 9, 70
    rng = np.random.default_rng(4)
    good = []
    for _ in range(3):
        runs = rng.integers(0, 12, 200).tolist()                           # zeros inside: legal
        cut = int(np.searchsorted(np.cumsum(runs), H * W, side="right"))
        runs = runs[:cut] + [H * W - sum(runs[:cut])]
        good.append(runs)
    short, long_ = good[1][:-1] + [good[1][-1] - 1], good[1][:40] + [H * W]
    sets = [good[0], short, good[1], long_, good[2], [], [0, 0, 0, H * W]]
    want = [host.decode(c, H, W, 9) for c in sets]
    assert [s for _, s in want] == [0, 1, 0, 1, 0, 1, 0]
    planes, status = rle.decode([{"size": [H, W], "counts": c} for c in sets], "cuda", value=9)
    assert status.tolist() == [s for _, s in want]
    assert np.array_equal(planes.cpu().numpy(), np.stack([p for p, _ in want]))
    as_text = [{"size": [H, W], "counts": host.to_string(c)} for c in sets if c]
    planes2, status2 = rle.decode(as_text, "cuda", value=9)
    keep = [i for i, c in enumerate(sets) if c]
    assert np.array_equal(planes2.cpu().numpy(), np.stack([want[i][0] for i in keep]))
    assert status2.tolist() == [want[i][1] for i in keep]
    # planes that held garbage are written in full: the raw call on a filled buffer
    L = _C.lib()
    flat = torch.tensor(sum(sets, []), dtype=torch.int64).to(torch.int32).cuda()
    m = np.array([len(c) for c in sets])
    table = np.ascontiguousarray(np.stack([np.cumsum(m) - m, m], 1).astype(np.int32))
    out = torch.full((len(sets) * H * W + 64,), 0x5A, dtype=torch.uint8, device="cuda")
    st = torch.full((len(sets),), 77, dtype=torch.int32, device="cuda")
    nbytes = L.cp_rle_decode_workspace_bytes(len(sets), int(m.sum()))
    ws = _C.workspace(nbytes, flat.device)
    _C.check(L.cp_rle_decode(_C.ptr(flat), table.ctypes.data_as(ctypes.c_void_p), len(sets), H, W, 9, _C.ptr(out),
                             _C.ptr(st), _C.ptr(ws), nbytes, _C.stream()), "cp_rle_decode")
    got = out.cpu().numpy()
    assert np.array_equal(got[:-64].reshape(len(sets), H, W), np.stack([p for p, _ in want]))
    assert (got[-64:] == 0x5A).all() and st.cpu().tolist() == [s for _, s in want]


# ------------------------------------------------------------------------------------------------------ drivers --
@pytest.fixture(scope="module")
def driver_run(tmp_path_factory):
    """test.py --track --save_ids --save_masks --save_rle once, on the KITTI-style frames of test_tracking's driver
    case: {names, opt, out}."""
    import test_tracking as tt
    from centerpoly_amd.opts import opts
    tmp = tmp_path_factory.mktemp("rle_driver")
    names, args = tt._track_set(str(tmp))
    with contextlib.redirect_stderr(io.StringIO()), contextlib.redirect_stdout(io.StringIO()):
        opt = opts().parse(args + ["--save_masks", "--save_rle", "--mots_class_map", "26:1,24:2"])
        opt.save_dir = str(tmp / "exp")
        out = tia._module("test").run_test(opt)
    return {"names": names, "opt": opt, "out": out, "tmp": str(tmp)}


def test_save_rle_equals_the_png_masks(driver_run):
    from PIL import Image
    from centerpoly_amd.datasets.dataset_factory import dataset_factory
    from centerpoly_amd.utils import rle
    opt, ds = driver_run["opt"], dataset_factory["kitti_poly"]
    inst_dir = os.path.join(opt.save_dir, "instances")
    with open(os.path.join(opt.save_dir, "results_segm.json")) as f:
        segm = json.load(f)
    total, at = 0, 0
    for k, name in enumerate(driver_run["names"]):
        stem = os.path.basename(name)
        with open(os.path.join(inst_dir, stem + "_rle.json")) as f:
            js = json.load(f)
        with open(os.path.join(inst_dir, stem + ".txt")) as f:
            lines = [line.split(" ") for line in f]
        assert (js["width"], js["height"]) == (96, 64) and len(js["instances"]) == len(lines)
        with open(os.path.join(inst_dir, stem + ".json")) as f:
            by_ids = {e["source_row"]: e for e in json.load(f)["instances"]}
        for e, (png, label, _) in zip(js["instances"], lines):
            assert e["label_id"] == int(label)
            plain = dict(e)
            bbox, seg = plain.pop("bbox"), plain.pop("segmentation")
            assert plain == by_ids[e["source_row"]]                        # --save_ids' entry, plus the two
            pixels = np.array(Image.open(os.path.join(inst_dir, png)))
            planes, status = rle.decode([seg], "cuda")
            assert not status.any() and np.array_equal(planes[0].cpu().numpy(), (pixels != 0) * 255)
            assert bbox == host.to_bbox(host.from_string(seg["counts"]), 64, 96)
            r = segm[at]
            at += 1
            assert r["image_id"] == 10 + k and r["segmentation"] == seg and r["bbox"] == bbox
            assert r["category_id"] == ds._valid_ids[ds.class_name.index(e["class_name"]) - 1]
            assert np.float32(r["score"]) == np.float32(e["score"])
        total += len(lines)
    assert total >= 4 and at == len(segm)


def test_mots_files_equal_the_track_ids(driver_run):
    from centerpoly_amd.datasets.evaluation import instance_level as il
    from centerpoly_amd.utils import rle
    opt = driver_run["opt"]
    inst_dir = os.path.join(opt.save_dir, "instances")
    files = sorted(os.listdir(os.path.join(inst_dir, "mots")))
    assert len(files) == 2 and files[0].endswith("image_2_drive_a.txt") and files[1].endswith("image_2_drive_b.txt")
    back = {24: 2, 26: 1}
    lines_seen = 0
    for fname, names in zip(files, (driver_run["names"][:3], driver_run["names"][3:])):
        with open(os.path.join(inst_dir, "mots", fname)) as f:
            rows = [line.split() for line in f]
        for frame, name in enumerate(names):
            ids = il.read_gt_ids(os.path.join(inst_dir, os.path.basename(name) + "_trackIds.png")).astype(np.int64)
            mine = [r for r in rows if int(r[0]) == frame]
            want = {}
            for v in np.unique(ids[ids > 0]):
                if int(v) // 256 in back:
                    want[back[int(v) // 256] * 1000 + int(v) % 256] = ids == v
            assert sorted(int(r[1]) for r in mine) == sorted(want)
            cover = np.zeros((64, 96), np.int64)
            for r in mine:
                assert int(r[2]) == int(r[1]) // 1000 and (int(r[3]), int(r[4])) == (64, 96)
                planes, status = rle.decode([{"size": [64, 96], "counts": r[5]}], "cuda", value=1)
                mask = planes[0].cpu().numpy()
                assert not status.any() and np.array_equal(mask != 0, want[int(r[1])])
                cover += mask
            assert cover.max() <= 1                                        # disjoint
            lines_seen += len(mine)
    assert lines_seen >= 4


def test_evaluate_coco_results_equals_the_mask_files(driver_run):
    from centerpoly_amd.datasets.dataset_factory import dataset_factory
    from centerpoly_amd.datasets.evaluation import instance_level as il
    opt, ds = driver_run["opt"], dataset_factory["kitti_poly"]
    with open(os.path.join(driver_run["tmp"], "BBoxes", "val16.json")) as f:
        annot = json.load(f)
    annot["categories"] = [{"id": int(i), "name": c} for i, c in zip(ds._valid_ids, ds.class_name[1:])]
    annot_json = os.path.join(driver_run["tmp"], "with_categories.json")
    with open(annot_json, "w") as f:
        json.dump(annot, f)
    gt_files = il.find_gt_files(opt.gt_dir, il.KITTI)
    by_rle = il.evaluate_coco_results(os.path.join(opt.save_dir, "results_segm.json"), annot_json, gt_files,
                                      protocol=il.KITTI)
    by_png = il.evaluate_result_dir(os.path.join(opt.save_dir, "instances"), sorted(gt_files.values()), protocol=il.KITTI)
    assert by_rle["allAp"] == by_png["allAp"] or (np.isnan(by_rle["allAp"]) and np.isnan(by_png["allAp"]))
    assert json.dumps(il.results_json(by_rle, il.KITTI), sort_keys=True) == \
        json.dumps(il.results_json(by_png, il.KITTI), sort_keys=True)
    # a segmentation of another canvas names its entry
    with open(os.path.join(opt.save_dir, "results_segm.json")) as f:
        segm = json.load(f)
    segm[0]["segmentation"] = {"size": [32, 96], "counts": host.to_string([32 * 96])}
    bad = os.path.join(driver_run["tmp"], "bad_segm.json")
    with open(bad, "w") as f:
        json.dump(segm, f)
    with pytest.raises(ValueError) as e:
        il.evaluate_coco_results(bad, annot_json, gt_files, protocol=il.KITTI)
    assert "entry 0" in str(e.value)

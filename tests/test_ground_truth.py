"""make_ground_truth.py and its kernel (csrc/paint.hip): id images from polygon files.

The fixture tests/golden/ground_truth.npz holds what the reference's own createInstanceImage / createLabelImage (IDD
and Cityscapes) draw with PIL for the inputs of tests/golden/ground_truth_cases.py: per case the drawn (value, polygon)
sequence and the image, per driver frame the default images, and the two label tables.  The CPU tests hold the label
tables, `paint_list`, a host statement of the painter (the fill of tests/golden/annotations_host.py applied in order)
and the installed PIL against it; the GPU tests hold the kernel, the library and the driver against it.  Everything is
integers: exact equality."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest
import torch

import annotations_host as host
import ground_truth_cases as gc
from centerpoly_amd import _C
from centerpoly_amd.datasets import ground_truth as gt
from centerpoly_amd.datasets.evaluation import instance_level

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

NAMES = sorted(gc.CASES)


def load_fixture():
    return np.load(os.path.join(HERE, "golden", "ground_truth.npz"), allow_pickle=False)


@pytest.fixture(scope="module")
def z():
    return load_fixture()


def sequence_of(z, name):
    """(polygons, values) as the fixture recorded them."""
    counts, xy = z[name + "_counts"], z[name + "_xy"]
    first = np.concatenate([[0], np.cumsum(counts)])
    return [xy[first[i]:first[i + 1]] for i in range(len(counts))], [int(v) for v in z[name + "_values"]]


def background_of(name):
    dataset, kind, encoding = gc.CASES[name][:3]
    return gt.paint_list([], dataset, kind, encoding)[2]


def fill_of(pts, W, H):
    pts = [(int(x), int(y)) for x, y in pts]
    return host.polygon_fill(pts + pts[:1] if len(pts) == 2 else pts, W, H)      # (a, b) is drawn as (a, b, a)


_painted = {}


def host_paint(z, name):
    """The painter on the host (once per case): every polygon's fill, in order, over the background; with it the
    image of "the first polygon that covers the pixel" (-1 where none does)."""
    if name not in _painted:
        W, H = gc.CASES[name][3]
        polygons, values = sequence_of(z, name)
        img = np.full((H, W), background_of(name), np.int32)
        first = np.full((H, W), -1, np.int64)
        for p, v in zip(polygons, values):
            m = fill_of(p, W, H)
            img[m] = v
            first[m & (first < 0)] = v
        _painted[name] = (img, first)
    return _painted[name]


# ------------------------------------------------------------------------------------------------------ CPU ----
@pytest.mark.parametrize("name", NAMES)
def test_fixture_is_worth_having(z, name):
    """Every case has pixels of at least two values and a pixel whose value is not that of the first polygon that
    covers it.  Three cases cannot: no polygon (`none`), a single polygon (`one`: two values, nothing to overwrite) and
    the canvas of one pixel (`pixel`: one value, but drawn over)."""
    img = z[name + "_image"]
    W, H = gc.CASES[name][3]
    assert img.shape == (H, W) and img.dtype == np.int32
    n = len(z[name + "_values"])
    if name == "none":
        assert n == 0 and np.all(img == background_of(name))
        return
    assert len(np.unique(img)) >= 2 or name == "pixel"
    first = host_paint(z, name)[1]
    assert np.any((first >= 0) & (first != img)) or name == "one"


def test_fixture_holds_the_cases_of_the_issue(z):
    counts = {name: z[name + "_counts"] for name in NAMES}
    assert 300 in counts["long"] and 4096 in counts["long"]
    assert len(counts["many"]) == 600 and len(counts["one"]) == 1 and len(counts["none"]) == 0
    assert (counts["two_vertex"] == 2).sum() >= 5 and (counts["many"] == 2).sum() >= 5
    assert sorted(set(gc.CASES[n][3] for n in NAMES)) == [(1, 1), (1, 40), (37, 53), (40, 1), (64, 48), (96, 64), (16384, 3)]
    assert z["floats_xy"].min() < 0 and z["wide_image"].shape == (3, 16384)
    used = set((gc.CASES[n][0], gc.CASES[n][1], gc.CASES[n][2]) for n in NAMES)
    for kind in ("instance", "label"):
        assert all(("IDD", kind, e) in used for e in gt.IDD_ENCODINGS)
        assert all(("cityscapes", kind, e) in used for e in gt.CITYSCAPES_ENCODINGS)
    # the shared counter: a caravan, a train and a vehicle fallback are 15000, 17001 and 18002
    v = z["idd_instance_id_values"].tolist()
    assert [x for x in v if x in (15000, 17001, 18002)] == [15000, 17001, 18002] and 16003 in v
    assert 12 in v and 12000 in v and 12001 in v and 12002 not in v          # the group and the deleted car
    assert 26 in z["cs_instance_ids_values"].tolist() and 255 in z["cs_instance_trainIds_values"].tolist()
    assert os.path.getsize(os.path.join(HERE, "golden", "ground_truth.npz")) < 200 * 1024


@pytest.mark.parametrize("dataset", ["IDD", "cityscapes"])
def test_label_tables(z, dataset):
    rows, encodings = gt.TABLES[dataset]
    assert [r[0] for r in rows] == z["table_%s_names" % dataset].tolist()
    assert np.array_equal(np.array([r[1:1 + len(encodings)] for r in rows], np.int32), z["table_%s_ids" % dataset])
    assert [bool(r[-1]) for r in rows] == z["table_%s_instances" % dataset].tolist()
    assert gt.label_table(dataset)["car"][1] and not gt.label_table(dataset)["road"][1]


@pytest.mark.parametrize("name", NAMES)
def test_paint_list(z, name):
    dataset, kind, encoding, canvas, build = gc.CASES[name]
    unknown = []
    polygons, values, background = gt.paint_list(build(), dataset, kind, encoding, unknown=unknown)
    want_p, want_v = sequence_of(z, name)
    assert values == want_v
    assert len(polygons) == len(want_p)
    for i, (a, b) in enumerate(zip(polygons, want_p)):
        assert a.dtype == np.int32 and np.array_equal(a, b), i
    if build is gc.books_idd:
        assert unknown == ["spaceship", "spaceship"]
    if len(values) == 0:
        assert np.all(z[name + "_image"] == background)


def test_paint_list_rules():
    car = [[0, 0], [4, 0], [0, 4]]
    with pytest.raises(ValueError, match="spaceship"):
        gt.paint_list([{"label": "spaceship", "polygon": car}], "cityscapes", "instance", "ids", what="f.json")
    with pytest.raises(ValueError, match="encoding"):
        gt.paint_list([], "IDD", "instance", "ids")
    with pytest.raises(ValueError, match="kind"):
        gt.paint_list([], "IDD", "colour", "id")
    with pytest.raises(ValueError, match="f.json.*object 0 .car.*4097 vertices"):
        gt.paint_list([{"label": "car", "polygon": car * 1365 + car[:2]}], "IDD", "instance", "id", what="f.json")
    with pytest.raises(ValueError, match="2\\^24"):
        gt.paint_list([{"label": "car", "polygon": [[0, 0], [1 << 25, 0], [0, 4]]}], "IDD", "label", "id")
    with pytest.raises(ValueError, match="1 vertices"):
        gt.paint_list([{"label": "car", "polygon": car[:1]}], "cityscapes", "label", "ids")
    # truncation towards zero, the counter that moves before a negative value is dropped, backgrounds
    p, v, b = gt.paint_list([{"label": "car", "polygon": [[-0.9, 1.9], [2.5, -3.5], [7.99, 8.01]]}], "IDD", "instance")
    assert p[0].tolist() == [[0, 1], [2, -3], [7, 8]] and v == [12000] and b == 35
    assert [gt.paint_list([], "IDD", "label", e)[2] for e in gt.IDD_ENCODINGS] == [35, 0, 255, 255, 255, 255, 255]
    assert [gt.paint_list([], "cityscapes", "instance", e)[2] for e in gt.CITYSCAPES_ENCODINGS] == [0, 255]
    assert gt.paint_list([{"label": "license plate", "polygon": car}], "cityscapes", "instance", "trainIds")[1] == []
    assert gt.paint_list([{"label": "car", "polygon": car[:2]}], "IDD", "label")[1] == []
    assert gt.paint_list([{"label": "car", "polygon": car[:2]}], "IDD", "instance")[1] == [12000]


@pytest.mark.parametrize("name", NAMES)
def test_host_painter_equals_the_fixture_and_the_installed_pil(z, name):
    from PIL import Image, ImageDraw
    dataset, kind, encoding, (W, H), build = gc.CASES[name]
    mine = host_paint(z, name)[0]
    assert np.array_equal(mine, z[name + "_image"])
    polygons, values = sequence_of(z, name)
    img = Image.new("I" if kind == "instance" else "L", (W, H), background_of(name))
    drawer = ImageDraw.Draw(img)
    for p, v in zip(polygons, values):
        drawer.polygon([tuple(int(c) for c in q) for q in p], fill=v)
    assert np.array_equal(mine, np.array(img).astype(np.int32))


def test_argument_validation_without_gpu():
    L = _C.lib()
    one = ctypes.c_void_p(16)                                      # never dereferenced: every check comes first
    first = lambda *v: (ctypes.c_int32 * len(v))(*v)
    need = L.cp_polygon_paint_workspace_bytes(2, 7)
    assert need >= 7 * 32 + 3 * 4 + 2 * 2 * 4
    assert L.cp_polygon_paint_workspace_bytes(-1, 7) == 0 and L.cp_polygon_paint_workspace_bytes(2, -1) == 0
    pp = lambda f, n=2, H=8, W=8, xy=one, value=one, image=one, ws=one, nbytes=need: \
        L.cp_polygon_paint(xy, f, value, n, 0, H, W, image, ws, nbytes, None)
    assert pp(first(0, 3, 7), xy=None) == -1
    assert pp(None) == -1
    assert pp(first(0, 3, 7), value=None) == -1
    assert pp(first(0, 3, 7), image=None) == -1
    assert pp(first(0, 3, 7), ws=None) == -1
    assert pp(first(0, 3, 7), n=-1) == -1
    assert pp(first(0, 3, 7), H=0) == -1
    assert pp(first(0, 3, 7), W=-4) == -1
    assert pp(first(0, 1, 7)) == -1                                # fewer than 2 vertices
    assert pp(first(0, 5, 4)) == -1                                # a length below zero
    assert pp(first(1, 4, 8)) == -1
    assert pp(first(0, 3, 3 + 4097)) == -2
    assert pp(first(*range(0, 2 * 4098, 2)), n=4097) == -2
    assert pp(first(*([4096 * i for i in range(257)] + [(1 << 20) + 2])), n=257) == -2       # T beyond 2^20
    assert pp(first(0, 3, 7), W=16385) == -2
    assert pp(first(0, 3, 7), H=65536 * 4, W=8192) == -2
    assert pp(first(0, 3, 7), nbytes=need - 1) == -3
    assert pp(None, n=0, image=None) == -1


def test_library_refuses_host_tensors_and_bad_input():
    tri = np.array([[0, 0], [4, 0], [0, 4]], np.int32)
    with pytest.raises(_C.NativeError):
        gt.paint([tri], [1], 0, (8, 8), device="cpu")
    with pytest.raises(ValueError, match="canvas"):
        gt.paint([tri], [1], 0, (16385, 8), device="cpu")
    with pytest.raises(ValueError, match="canvas"):
        gt.paint([tri], [1], 0, (0, 8), device="cpu")
    with pytest.raises(ValueError, match="values"):
        gt.paint([tri], [1, 2], 0, (8, 8), device="cpu")
    with pytest.raises(ValueError, match="polygon 0"):
        gt.paint([tri[:1]], [1], 0, (8, 8), device="cpu")
    with pytest.raises(ValueError, match="4097 polygons"):
        gt.paint([tri] * 4097, [1] * 4097, 0, (8, 8), device="cpu")


def test_write_id_png_round_trip_and_refusal(tmp_path):
    from PIL import Image
    ids = np.array([[0, 35, 12000], [18002, 65535, 255]], np.int32)
    path = str(tmp_path / "a_gtFine_instanceids.png")
    gt.write_id_png(path, torch.from_numpy(ids), 16)
    assert Image.open(path).mode == "I;16"
    back = instance_level.read_gt_ids(path)
    assert back.dtype == np.uint16 and np.array_equal(back, ids)
    lab = str(tmp_path / "a_gtFine_labelids.png")
    gt.write_id_png(lab, ids.clip(0, 255), 8)
    assert Image.open(lab).mode == "L" and np.array_equal(np.array(Image.open(lab)), ids.clip(0, 255))
    # IDD csId: vehicle fallback is 355, 355000 as an instance
    bad = str(tmp_path / "bad.png")
    with pytest.raises(ValueError, match="bad.png.*355000"):
        gt.write_id_png(bad, np.array([[355000, 1]], np.int32), 16)
    with pytest.raises(ValueError, match="bad.png.*355"):
        gt.write_id_png(bad, np.array([[355, 1]], np.int32), 8)
    with pytest.raises(ValueError, match="bad.png.*-1"):
        gt.write_id_png(bad, np.array([[-1, 1]], np.int32), 16)
    with pytest.raises(ValueError):
        gt.write_id_png(bad, ids, 32)
    assert not os.path.exists(bad)


def write_frames(root, frames):
    for city, stem, case in frames:
        os.makedirs(os.path.join(root, city), exist_ok=True)
        with open(os.path.join(root, city, stem + "_gtFine_polygons.json"), "w") as f:
            json.dump(gc.frame_json(case), f)


def test_idd_tree_of_the_host_painter_is_found_by_the_scoring_side(z, tmp_path):
    import make_ground_truth as mg
    root = str(tmp_path / "val")
    write_frames(root, gc.IDD_FRAMES)
    for city, stem, case in gc.IDD_FRAMES:
        name = mg.output_names("IDD", "id", stem + "_gtFine")[0]
        assert name == stem + instance_level.IDD_GT_SUFFIX
        gt.write_id_png(os.path.join(root, city, name), z["frame_IDD_%s_instance" % case], 16)
    found = instance_level.find_gt_files(root, instance_level.IDD)
    assert sorted(found) == sorted("%s/%s" % (c, s) for c, s, _ in gc.IDD_FRAMES)
    for city, stem, case in gc.IDD_FRAMES:
        ids = instance_level.read_gt_ids(found["%s/%s" % (city, stem)])
        assert np.array_equal(ids, z["frame_IDD_%s_instance" % case])
    table = instance_level.gt_instances(np.bincount(instance_level.read_gt_ids(found["9/000005"]).reshape(-1),
                                                    minlength=65536), instance_level.IDD)
    assert 12000 in table[:, 0] and 18002 in table[:, 0]


def test_driver_arguments_names_and_refusals(tmp_path):
    import make_ground_truth as mg
    opt = mg.parse_args(["--dataset", "IDD", "--gt_dir", "g"])
    assert (opt.id_type, opt.no_instance, opt.labels, opt.num_workers, opt.gpu, opt.out_dir) == ("id", False, False, 4, 0, "")
    assert mg.parse_args(["--dataset", "cityscapes", "--gt_dir", "g"]).id_type == "ids"
    assert mg.parse_args(["--dataset", "IDD", "--gt_dir", "g", "--id_type", "level3Id", "--labels"]).id_type == "level3Id"
    for bad in (["--dataset", "IDD"], ["--dataset", "kitti_poly", "--gt_dir", "g"],
                ["--dataset", "IDD", "--gt_dir", "g", "--id_type", "trainIds"],
                ["--dataset", "cityscapes", "--gt_dir", "g", "--id_type", "id"],
                ["--dataset", "IDD", "--gt_dir", "g", "--no_instance"]):
        with pytest.raises(SystemExit):
            mg.parse_args(bad)
    assert mg.output_names("IDD", "id", "000010_gtFine") == ("000010_gtFine_instanceids.png", "000010_gtFine_labelids.png")
    assert mg.output_names("IDD", "level3Id", "1_gtFine") == ("1_gtFine_instancelevel3Ids.png", "1_gtFine_labellevel3Ids.png")
    assert mg.output_names("cityscapes", "ids", "a_1_2_gtFine") == ("a_1_2_gtFine_instanceIds.png", "a_1_2_gtFine_labelIds.png")
    assert mg.output_names("cityscapes", "trainIds", "a_1_2_gtFine") == ("a_1_2_gtFine_instanceTrainIds.png",
                                                                         "a_1_2_gtFine_labelTrainIds.png")
    run = lambda d, ds="IDD": mg.run(mg.parse_args(["--dataset", ds, "--gt_dir", str(d), "--num_workers", "0"]))
    # no frames, no directory
    (tmp_path / "empty" / "7").mkdir(parents=True)
    with pytest.raises(FileNotFoundError, match="empty"):
        run(tmp_path / "empty")
    with pytest.raises(FileNotFoundError, match="nowhere"):
        run(tmp_path / "nowhere")
    # two JSON files for one frame
    two = tmp_path / "two" / "7"
    two.mkdir(parents=True)
    for name in ("000010_gtFine_polygons.json", "000010_gtCoarse_polygons.json"):
        (two / name).write_text(json.dumps(gc.frame_json("overlap")))
    with pytest.raises(ValueError, match="7/000010.*000010_gtCoarse_polygons.json.*000010_gtFine_polygons.json"):
        run(tmp_path / "two")
    cs = tmp_path / "twocs" / "aa"
    cs.mkdir(parents=True)
    for name in ("aa_1_2_gtFine_polygons.json", "aa_1_2_gtCoarse_polygons.json", "aa_1_3_gtFine_polygons.json"):
        (cs / name).write_text(json.dumps(gc.frame_json("overlap_cs")))
    with pytest.raises(ValueError, match="aa/aa_1_2"):
        run(tmp_path / "twocs", "cityscapes")
    # a missing size: refused before the device is asked for, the message names the file
    for k, key in enumerate(("imgWidth", "imgHeight")):
        d = tmp_path / ("nosize%d" % k) / "7"
        d.mkdir(parents=True)
        (d / "000010_gtFine_polygons.json").write_text(json.dumps(gc.frame_json("overlap")))
        frame = gc.frame_json("one")
        del frame[key]
        (d / "000020_gtFine_polygons.json").write_text(json.dumps(frame))
        with pytest.raises(ValueError, match="000020_gtFine_polygons.json has no " + key):
            run(d.parent)
    assert not [f for _, _, fs in os.walk(str(tmp_path)) for f in fs if f.endswith(".png")]


# ------------------------------------------------------------------------------------------------------ GPU ----
def device_paint(z, name):
    polygons, values = sequence_of(z, name)
    return gt.paint(polygons, values, background_of(name), gc.CASES[name][3], "cuda")


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_gpu_paint_equals_the_fixture(z, name):
    got = device_paint(z, name)
    assert got.dtype == torch.int32 and got.is_cuda
    assert np.array_equal(got.cpu().numpy(), z[name + "_image"])


@pytest.mark.gpu
def test_gpu_paint_is_deterministic_and_stays_on_the_canvas(z):
    for name in ("many", "long", "wide", "floats"):
        a, b = device_paint(z, name), device_paint(z, name)
        assert torch.equal(a, b), name
    # the rows above and below a canvas cut out of a larger buffer keep their bits
    W, H = gc.CASES["floats"][3]
    polygons, values = sequence_of(z, "floats")
    first = np.concatenate([[0], np.cumsum([len(p) for p in polygons])]).astype(np.int32)
    L = _C.lib()
    buf = torch.full((H + 8, W), -7, dtype=torch.int32, device="cuda")
    xy = torch.from_numpy(np.concatenate(polygons)).cuda()
    val = torch.tensor(values, dtype=torch.int32, device="cuda")
    nbytes = L.cp_polygon_paint_workspace_bytes(len(values), int(first[-1]))
    ws = _C.workspace(nbytes, "cuda")
    first_arr = (ctypes.c_int32 * len(first))(*first.tolist())
    _C.check(L.cp_polygon_paint(_C.ptr(xy), first_arr, _C.ptr(val), len(values), 35, H, W, _C.ptr(buf[4:]), _C.ptr(ws),
                                nbytes, _C.stream()), "cp_polygon_paint")
    out = buf.cpu().numpy()
    assert np.all(out[:4] == -7) and np.all(out[H + 4:] == -7)
    assert np.array_equal(out[4:H + 4], z["floats_image"])


@pytest.mark.gpu
@pytest.mark.parametrize("name", [n for n in NAMES if gc.CASES[n][3] == (37, 53) or n in ("overlap", "overlap_cs")])
def test_gpu_instance_and_label_images(z, name):
    dataset, kind, encoding, canvas, build = gc.CASES[name]
    fn = gt.instance_image if kind == "instance" else gt.label_image
    got = fn(build(), canvas, dataset, encoding, device="cuda")
    assert np.array_equal(got.cpu().numpy(), z[name + "_image"])


@pytest.mark.gpu
@pytest.mark.parametrize("dataset,frames,inst,lab,workers", [
    ("IDD", gc.IDD_FRAMES, "_gtFine_instanceids.png", "_gtFine_labelids.png", "2"),        # DataLoader workers
    ("cityscapes", gc.CITYSCAPES_FRAMES, "_gtFine_instanceIds.png", "_gtFine_labelIds.png", "0")])
def test_gpu_driver_end_to_end(z, tmp_path, dataset, frames, inst, lab, workers):
    import make_ground_truth as mg
    from PIL import Image
    root = str(tmp_path / "val")
    write_frames(root, frames)
    written = mg.run(mg.parse_args(["--dataset", dataset, "--gt_dir", root, "--labels", "--num_workers", workers]))
    assert len(written) == 2 * len(frames)
    assert written == [os.path.join(root, c, s + sfx) for c, s, _ in sorted(frames) for sfx in (inst, lab)]
    for city, stem, case in frames:
        ids = instance_level.read_gt_ids(os.path.join(root, city, stem + inst))
        assert np.array_equal(ids, z["frame_%s_%s_instance" % (dataset, case)]), case
        img = Image.open(os.path.join(root, city, stem + lab))
        assert img.mode == "L" and np.array_equal(np.array(img), z["frame_%s_%s_label" % (dataset, case)]), case
    # what --gt_dir scoring opens
    proto = instance_level.IDD if dataset == "IDD" else instance_level.CITYSCAPES
    found = instance_level.find_gt_files(root, proto)
    assert len(found) == len(frames)
    if dataset == "IDD":
        assert sorted(found) == sorted("%s/%s" % (c, s) for c, s, _ in frames)
        # one prediction, the first car of the last frame as the ground truth has it; the other frames predict nothing
        pred = tmp_path / "pred"
        car = (instance_level.read_gt_ids(found["9/000005"]) == 12000).astype(np.uint8) * 255
        for city, stem, case in frames:
            (pred / city).mkdir(parents=True, exist_ok=True)
            (pred / city / (stem + "_pred.txt")).write_text("car.png 12 0.9\n" if stem == "000005" else "")
        Image.fromarray(car).save(str(pred / "9" / "car.png"))
        res = instance_level.evaluate_result_dir(str(pred), sorted(found.values()), device=torch.device("cuda"), protocol=proto)
        assert 0.0 < res["allAp50%"] <= 1.0
    # --out_dir keeps the city directory; --no_instance writes the label image alone
    out = str(tmp_path / "out")
    written = mg.run(mg.parse_args(["--dataset", dataset, "--gt_dir", root, "--out_dir", out, "--labels", "--no_instance",
                                    "--num_workers", "0"]))
    assert sorted(written) == sorted(os.path.join(out, c, s + lab) for c, s, _ in frames)
    assert all(os.path.isfile(p) for p in written)

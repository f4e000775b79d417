"""make_annotations.py and its kernels (csrc/annotate.hip): training polygons from ground truth.

The fixture tests/golden/annotations.npz holds what the reference's own functions give for the inputs of
tests/golden/annotation_cases.py (gen_annotations_golden.py: the tools' `find_points_from_box`,
`find_first_non_zero_pixel` and `polygon_to_box` compiled from their files, masks drawn by PIL, the converter
transcribed).  The CPU tests hold the host statement (tests/golden/annotations_host.py) and the JSON writer against it;
the GPU tests hold the kernels, the library and the driver against it.  Everything is integers: exact equality."""
import ctypes
import json
import os
import sys
import types

import numpy as np
import pytest
import torch

import annotation_cases as ac
import annotations_host as host
from centerpoly_amd import _C
from centerpoly_amd.datasets import annotate

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
PATH_ROOT = "/ROOT"                                             # what the recorded file names start with


def load_fixture():
    return np.load(os.path.join(HERE, "golden", "annotations.npz"), allow_pickle=False)


@pytest.fixture(scope="module")
def z():
    return load_fixture()


_built = {}


def ids_of(z, name):
    """The id image of a case: from the fixture when it is stored there, rebuilt otherwise (once)."""
    if name not in _built:
        _built[name] = z["ids_" + name] if name in ac.ID_STORED else ac.ID_CASES[name]()
    return _built[name]


def objects_of(z, name):
    return json.loads(str(z["poly_%s_objects" % name]))


def masks_of(z, name):
    W, H = ac.POLY_CASES[name][1]
    return np.unpackbits(z["poly_%s_masks" % name], axis=2)[:, :, :W].astype(np.uint8) * 255


def label_class(labels):
    return np.array([ac.KITTI_LABELS.index({"person": 24, "rider": 25, "car": 26, "truck": 27, "bus": 28, "train": 31,
                                            "motorcycle": 32, "bicycle": 33}[str(s)]) for s in labels], np.int64)


ID_NAMES = sorted(ac.ID_CASES)
POLY_NAMES = [n for n in sorted(ac.POLY_CASES) if n != "small_full"]


# ------------------------------------------------------------------------------------------------ CPU: host ----
def test_fixture_is_worth_having(z):
    assert z["ids_shapes_bbox"].shape[0] == 8 and "train" in z["ids_shapes_label"].tolist()
    assert z["ids_many128_bbox"].shape[0] == 128 and z["ids_many129_bbox"].shape[0] == 129
    assert z["ids_kitti_bbox"].shape[0] >= 25
    # half-to-even matters, and the two line walks of more than 64 and 128 steps are there
    assert z["points_int_16"][2, :4, 0].tolist() == [3, 4, 4, 4]
    wide = ids_of(z, "wide")
    assert wide.shape == (70, 300)
    labels = z["poly_small_label"].tolist()
    assert "pole" in labels and "traffic sign" in labels and "cargroup" not in labels
    m = masks_of(z, "small")
    assert m[labels.index("motorcycle")].sum() == 0 and m[labels.index("car")].sum() > 0
    assert len(objects_of(z, "long")[0]["polygon"]) == 700 and z["poly_none_bbox"].shape[0] == 0


@pytest.mark.parametrize("kind", ["int", "float"])
def test_host_box_points(z, kind):
    boxes = ac.point_boxes()[0 if kind == "int" else 1]
    W, H = ac.POINT_CANVAS
    full = np.ones((H, W), np.uint8)
    for N in ac.BOX_POINT_COUNTS:
        got = [host.object_polygon(tuple(int(c) for c in b) if kind == "int" else tuple(float(c) for c in b), full, N)
               for b in boxes]
        assert np.array_equal(np.array(got, np.int32), z["points_%s_%d" % (kind, N)]), N


@pytest.mark.parametrize("name", ID_NAMES)
def test_host_id_images(z, name):
    ids = ids_of(z, name)
    for N in ac.ID_COUNTS[name]:
        got = host.from_id_image(ids, ac.KITTI_LABELS, 256, N)
        assert np.array_equal(got["bbox"], z["ids_%s_bbox" % name])
        assert np.array_equal(got["cls"], label_class(z["ids_%s_label" % name]))
        assert np.array_equal(got["poly"], z["ids_%s_poly%d" % (name, N)]), N
        assert got["inst_id"].tolist() == sorted(got["inst_id"].tolist())


@pytest.mark.parametrize("name", POLY_NAMES)
def test_host_fill_equals_the_installed_pil(z, name):
    from PIL import Image, ImageDraw
    W, H = ac.POLY_CASES[name][1]
    kept = annotate.kept_objects(objects_of(z, name), ac.POLY_CASES[name][2])
    recorded = masks_of(z, name)
    assert len(kept) == len(recorded)
    for k, (label, polygon) in enumerate(kept):
        img = Image.new("L", (W, H), 0)
        ImageDraw.Draw(img).polygon([tuple(p) for p in polygon], outline=0, fill=255)
        mine = host.polygon_mask(polygon, W, H)
        assert np.array_equal(mine, np.array(img)), (name, k, label)
        assert np.array_equal(mine, recorded[k]), (name, k, label)


@pytest.mark.parametrize("name", sorted(ac.POLY_CASES))
def test_host_polygon_lists(z, name):
    build, canvas, have = ac.POLY_CASES[name]
    masks = masks_of(z, name) if name == "full" else None          # (the large canvas: the fill is held above)
    for N in ac.POLY_COUNTS[name]:
        got = host.from_polygons(objects_of(z, name), canvas, have, N, masks)
        assert got["label"] == z["poly_%s_label" % name].tolist()
        assert np.array_equal(got["bbox"], z["poly_%s_bbox" % name])
        assert np.array_equal(got["poly"], z["poly_%s_poly%d" % (name, N)]), N


# ---------------------------------------------------------------------------------------- CPU: the interface ----
def test_argument_validation_without_gpu():
    L = _C.lib()
    lab = (ctypes.c_int32 * 8)(*ac.KITTI_LABELS)
    one = ctypes.c_void_p(16)                                      # never dereferenced: every check comes first
    ws = L.cp_annot_id_instances_workspace_bytes()
    assert ws == 65536 * 16
    args = lambda **k: [k.get("ids", one), k.get("H", 4), k.get("W", 4), k.get("lab", lab), k.get("C", 8),
                        k.get("div", 256), k.get("max", 1024), one, one, one, one, k.get("ws", one),
                        k.get("bytes", ws), None]
    assert L.cp_annot_id_instances(*args(ids=None)) == -1
    assert L.cp_annot_id_instances(*args(H=0)) == -1
    assert L.cp_annot_id_instances(*args(div=0)) == -1
    assert L.cp_annot_id_instances(*args(C=0)) == -1
    assert L.cp_annot_id_instances(*args(C=33)) == -2
    assert L.cp_annot_id_instances(*args(max=1025)) == -2
    assert L.cp_annot_id_instances(*args(H=65536, W=32768)) == -2
    assert L.cp_annot_id_instances(*args(bytes=ws - 1)) == -3
    assert L.cp_annot_id_instances(*args(ws=None)) == -1

    first = lambda *v: (ctypes.c_int32 * len(v))(*v)
    need = L.cp_polygon_masks_workspace_bytes(2, 7)
    assert need >= 7 * 32 + 16
    pm = lambda f, n=2, H=8, W=8, xy=one, nbytes=need: L.cp_polygon_masks(xy, f, n, H, W, one, one, one, nbytes, None)
    assert pm(first(0, 3, 7), n=0) == 0
    assert pm(first(0, 3, 7), xy=None) == -1
    assert pm(first(0, 3, 7), H=0) == -1
    assert pm(first(0, 2, 7)) == -1                                # fewer than 3 vertices
    assert pm(first(1, 4, 8)) == -1
    assert pm(first(0, 3, 3 + 4097)) == -2
    assert pm(first(*range(0, 3 * 130, 3)), n=129) == -2
    assert pm(first(0, 3, 7), H=65536, W=32768) == -2
    assert pm(first(0, 3, 7), nbytes=need - 1) == -3

    for fn, lead in ((L.cp_annot_rays_ids, lambda src: [src, 8, 8, one, one]),
                     (L.cp_annot_rays_masks, lambda src: [src, 8, 8, one])):
        assert fn(*(lead(one) + [0, 16, one, None])) == 0
        assert fn(*(lead(None) + [1, 16, one, None])) == -1
        assert fn(*(lead(one) + [1, 16, None, None])) == -1
        assert fn(*(lead(one) + [1, 0, one, None])) == -1
        assert fn(*(lead(one) + [1, 18, one, None])) == -1
        assert fn(*(lead(one) + [1, 68, one, None])) == -2
        assert fn(*(lead(one) + [1025, 16, one, None])) == -2
        assert fn(*(lead(one) + [-1, 16, one, None])) == -1
    assert L.cp_annot_rays_ids(one, 8, 8, None, one, 1, 16, one, None) == -1
    assert L.cp_annot_rays_ids(one, 65536, 32768, one, one, 1, 16, one, None) == -2


def test_library_refuses_host_tensors_and_bad_input():
    with pytest.raises(_C.NativeError):
        annotate.from_id_image(torch.zeros((4, 4), dtype=torch.int16), ac.KITTI_LABELS, 256, 16)
    for bad in (6, 0, 68, [16, 18]):
        with pytest.raises(ValueError):
            annotate.check_nbr_points(bad)
    tri = [[0, 0], [4, 0], [0, 4]]
    with pytest.raises(ValueError, match="object 0 .car.*2 vertices"):
        annotate.from_polygons([{"label": "car", "polygon": tri[:2]}], (8, 8), ["car"], 16, what="a.png")
    with pytest.raises(ValueError, match="4097 vertices"):
        annotate.from_polygons([{"label": "car", "polygon": tri * 1365 + tri[:2]}], (8, 8), ["car"], 16)
    with pytest.raises(ValueError, match="2\\^24"):
        annotate.from_polygons([{"label": "car", "polygon": [[0, 0], [1 << 25, 0], [0, 4]]}], (8, 8), ["car"], 16)


def test_driver_arguments_and_file_names(tmp_path):
    import make_annotations as ma
    base = ["--img_dir", "i", "--gt_dir", "g", "--out_dir", "o"]
    opt = ma.parse_args(["--dataset", "cityscapes"] + base + ["--nbr_points", "16", "24", "64"])
    assert (opt.source, opt.id_divisor, opt.nbr_points, opt.split, opt.num_workers) == ("polygons", 1000, [16, 24, 64], "train", 4)
    opt = ma.parse_args(["--dataset", "kitti_poly"] + base)
    assert (opt.source, opt.id_divisor, opt.nbr_points) == ("ids", 256, [16])
    opt = ma.parse_args(["--dataset", "IDD", "--source", "ids", "--id_divisor", "1000", "--split", "val"] + base)
    assert (opt.source, opt.id_divisor, opt.split) == ("ids", 1000, "val")
    for bad in (["--dataset", "kitti_poly", "--source", "polygons"] + base, ["--dataset", "coco"] + base,
                ["--dataset", "IDD", "--nbr_points", "18"] + base[:2] + base[4:],
                ["--dataset", "IDD", "--img_dir", "i", "--out_dir", "o"],
                ["--dataset", "IDD", "--nbr_points", "16", "16"] + base):
        with pytest.raises((SystemExit, ValueError)):
            ma.parse_args(bad)
    ma.parse_args(["--dataset", "IDD", "--img_dir", "i", "--out_dir", "o", "--split", "test"])
    assert ma.output_names("cityscapes", "train", 24) == {"train": "train24_regular_interval.json"}
    assert ma.output_names("cityscapes", "val", 8) == {"val": "val8_regular_interval.json"}
    assert ma.output_names("IDD", "val", 32) == {"val": "val32_regular_interval.json"}
    assert ma.output_names("kitti_poly", "train", 32) == {"train": "train32.json", "val": "val32.json",
                                                          "trainval": "trainval32.json"}
    for d in ma.DATASETS:
        assert ma.output_names(d, "test", 16) == {"test": "test.json"}
    opt = ma.parse_args(["--dataset", "cityscapes", "--img_dir", "/d/leftImg8bit/val", "--gt_dir", "/d/gtFine/val",
                         "--out_dir", "o"])
    assert ma.gt_path(opt, "/d/leftImg8bit/val/aa/aa_1_2_leftImg8bit.png") == "/d/gtFine/val/aa/aa_1_2_gtFine_polygons.json"
    opt.source = "ids"
    assert ma.gt_path(opt, "/d/leftImg8bit/val/aa/aa_1_2_leftImg8bit.png") == "/d/gtFine/val/aa/aa_1_2_gtFine_instanceIds.png"
    opt = ma.parse_args(["--dataset", "kitti_poly", "--img_dir", "/k/image_2", "--gt_dir", "/k/instance", "--out_dir", "o"])
    assert ma.gt_path(opt, "/k/image_2/000003_10.png") == "/k/instance/000003_10.png"
    # the test split needs no device and no ground truth
    (tmp_path / "image_2").mkdir()
    for i in range(3):
        (tmp_path / "image_2" / ("%06d_10.png" % i)).write_bytes(b"")
    opt = ma.parse_args(["--dataset", "kitti_poly", "--split", "test", "--img_dir", str(tmp_path / "image_2"),
                         "--out_dir", str(tmp_path / "out")])
    assert list(ma.run(opt).values()) == [(3, 3)]


def same_json(a, b, where="$"):
    """Key for key and type for type."""
    assert type(a) is type(b), (where, type(a), type(b))
    if isinstance(a, dict):
        assert list(a) == list(b), where
        for k in a:
            same_json(a[k], b[k], where + "." + k)
    elif isinstance(a, list):
        assert len(a) == len(b), where
        for i, (x, y) in enumerate(zip(a, b)):
            same_json(x, y, "%s[%d]" % (where, i))
    else:
        assert a == b, (where, a, b)


def recorded_json(z, key, root):
    return json.loads(str(z[key]).replace(PATH_ROOT, root))


def kitti_images(z, count, N, root):
    """[(path, rows)] of the split-rule directory from the host statement (held against the fixtures above)."""
    names = ["person", "rider", "car", "truck", "bus", "train", "motorcycle", "bicycle"]
    images = []
    for i in range(count):
        r = host.from_id_image(ac.kitti_dir_image(i), ac.KITTI_LABELS, 256, N)
        images.append(("%s/image_2/%06d_10.png" % (root, i),
                       [(r["bbox"][k], names[r["cls"][k]], int(r["pseudo_depth"][k]), r["poly"][k])
                        for k in range(len(r["cls"]))]))
    return images


@pytest.mark.parametrize("count", [19, 20, 21, 40])
def test_json_writer_and_the_kitti_split_rule(z, count):
    images = kitti_images(z, count, 4, PATH_ROOT)
    numbered = [(k + 1, im) for k, im in enumerate(images) if im[1]]
    parts = {"trainval": [im for _, im in numbered],
             "val": [im for k, im in numbered if annotate.kitti_val_image(k)],
             "train": [im for k, im in numbered if not annotate.kitti_val_image(k)]}
    for part, ims in parts.items():
        got = json.loads(json.dumps(annotate.coco_dict(ims, ac.CITYSCAPES_CATS)))
        same_json(got, recorded_json(z, "json_kitti%d_%s" % (count, part), PATH_ROOT))
    assert len(parts["val"]) == (count // 20 if count != 40 else 2)


def test_json_writer_polygon_files(z):
    """IDD (float boxes are truncated, an image without objects stays) and Cityscapes (pole and traffic sign take a
    pseudo-depth and are dropped) from the recorded polygons."""
    def rows(case, N):
        labels = z["poly_%s_label" % case].tolist()
        return [(z["poly_%s_bbox" % case][k], labels[k], k, z["poly_%s_poly%d" % (case, N)][k]) for k in range(len(labels))]
    idd = [("%s/leftImg8bit/train/%s_leftImg8bit.png" % (PATH_ROOT, s), rows(c, 16))
           for s, c in (("7/000010", "idd"), ("7/000020", "none"), ("9/000005", "idd"))]
    got = json.loads(json.dumps(annotate.coco_dict(idd, ac.IDD_HAVE)))
    same_json(got, recorded_json(z, "json_idd_train16", PATH_ROOT))
    assert len(got["images"]) == 3 and {a["image_id"] for a in got["annotations"]} == {0, 2}
    city = [("%s/leftImg8bit/val/%s_leftImg8bit.png" % (PATH_ROOT, s), rows(c, 8))
            for s, c in (("aa/aa_000001_000019", "small_full"), ("aa/aa_000002_000019", "none"), ("bb/bb_000000_000001", "full"))]
    got = json.loads(json.dumps(annotate.coco_dict(city, ac.CITYSCAPES_CATS)))
    same_json(got, recorded_json(z, "json_cityscapes_val8", PATH_ROOT))
    depths = [a["pseudo_depth"] for a in got["annotations"] if a["image_id"] == 0]
    assert depths != list(range(len(depths)))                      # the gaps of the dropped labels are kept
    same_json(json.loads(json.dumps(annotate.coco_dict([("%s/image_2/%06d_10.png" % (PATH_ROOT, i), [annotate.placeholder_row()])
                                                        for i in range(3)], ac.CITYSCAPES_CATS))),
              recorded_json(z, "json_kitti_test", PATH_ROOT))


def test_written_kitti_file_loads_through_the_data_set(z, tmp_path):
    from centerpoly_amd.datasets.dataset.polygons import KITTIPOLY
    images = [im for im in kitti_images(z, 5, 16, str(tmp_path)) if im[1]]
    n_img, n_ann = annotate.write_annotations(str(tmp_path / "annot" / "train16.json"), images, ac.CITYSCAPES_CATS)
    opt = types.SimpleNamespace(annot_dir=str(tmp_path / "annot"), data_dir="", img_dir=str(tmp_path), nbr_points=16)
    ds = KITTIPOLY(opt, "train")
    assert (len(ds.images), n_img, n_ann) == (4, 4, sum(len(r) for _, r in images))
    for img_id, (path, rows) in zip(ds.images, images):
        assert ds.coco.loadImgs([img_id])[0]["file_name"] == path
        anns = ds.coco.loadAnns(ds.coco.getAnnIds([img_id]))
        assert len(anns) == len(rows)
        for a, (box, label, depth, poly) in zip(anns, rows):
            x0, y0, x1, y1 = (float(c) for c in box)
            assert a["bbox"] == [x0, y0, x1 - x0, y1 - y0] and a["pseudo_depth"] == depth
            assert a["poly"] == [float(c) for c in poly.reshape(-1)] and len(a["poly"]) == 32
            assert ds.class_name[a["category_id"]] == label


# ------------------------------------------------------------------------------------------------------ GPU ----
def _dev():
    return torch.device("cuda:0")


def device_id_instances(ids):
    dev = _dev()
    L = _C.lib()
    ids_dev = torch.from_numpy(ids.view(np.int16)).to(dev)
    lab = (ctypes.c_int32 * 8)(*ac.KITTI_LABELS)
    out = torch.full((1 + 6 * 1024,), -7, dtype=torch.int32, device=dev)
    ws = _C.workspace(L.cp_annot_id_instances_workspace_bytes(), dev)
    H, W = ids.shape
    _C.check(L.cp_annot_id_instances(_C.ptr(ids_dev), H, W, lab, 8, 256, 1024, _C.ptr(out[:1]), _C.ptr(out[1:1025]),
                                     _C.ptr(out[1025:2049]), _C.ptr(out[2049:]), _C.ptr(ws), ws.numel(), _C.stream()),
             "cp_annot_id_instances")
    return out.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ID_NAMES)
def test_id_instances_kernel(z, name):
    ids = ids_of(z, name)
    a, b = device_id_instances(ids), device_id_instances(ids)
    assert np.array_equal(a, b)                                    # the same bits on every run
    exp = host.id_objects(ids, ac.KITTI_LABELS, 256)
    n = a[0]
    assert n == len(exp) == len(z["ids_%s_bbox" % name])
    assert a[1:1 + n].tolist() == [v for v, _, _ in exp]
    assert np.array_equal(a[1025:1025 + n], label_class(z["ids_%s_label" % name]))
    assert np.array_equal(a[2049:].reshape(1024, 4)[:n], z["ids_%s_bbox" % name])
    assert not a[1 + n:1025].any() and (a[1025 + n:2049] == -1).all() and not a[2049 + 4 * n:].any()


@pytest.mark.gpu
def test_id_instances_reports_more_than_max_inst(z):
    """129 objects into 128 slots: the count says so, the first 128 are written, nothing past them."""
    ids = ids_of(z, "many129")
    dev = _dev()
    L = _C.lib()
    ids_dev = torch.from_numpy(ids.view(np.int16)).to(dev)
    lab = (ctypes.c_int32 * 8)(*ac.KITTI_LABELS)
    out = torch.full((1 + 6 * 128 + 8,), -7, dtype=torch.int32, device=dev)
    ws = _C.workspace(L.cp_annot_id_instances_workspace_bytes(), dev)
    _C.check(L.cp_annot_id_instances(_C.ptr(ids_dev), 64, 96, lab, 8, 256, 128, _C.ptr(out[:1]), _C.ptr(out[1:129]),
                                     _C.ptr(out[129:257]), _C.ptr(out[257:769]), _C.ptr(ws), ws.numel(), _C.stream()), "")
    a = out.cpu().numpy()
    assert a[0] == 129 and (a[769:] == -7).all()
    assert np.array_equal(a[257:769].reshape(128, 4), z["ids_many129_bbox"][:128])


def device_polygon_masks(objects, canvas, have):
    dev = _dev()
    L = _C.lib()
    W, H = canvas
    kept = annotate.kept_objects(objects, have)
    verts = [np.trunc(np.asarray(p, np.float64)).astype(np.int32) for _, p in kept]
    first = np.cumsum([0] + [len(v) for v in verts])
    n = len(kept)
    xy = torch.from_numpy(np.concatenate(verts)).to(dev)
    masks = torch.full((n, H, W), 7, dtype=torch.uint8, device=dev)
    counts = torch.full((n,), -7, dtype=torch.int32, device=dev)
    nbytes = L.cp_polygon_masks_workspace_bytes(n, int(first[-1]))
    ws = _C.workspace(nbytes, dev)
    _C.check(L.cp_polygon_masks(_C.ptr(xy), (ctypes.c_int32 * (n + 1))(*first.tolist()), n, H, W, _C.ptr(masks),
                                _C.ptr(counts), _C.ptr(ws), nbytes, _C.stream()), "cp_polygon_masks")
    return masks, counts.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("name", [n for n in POLY_NAMES if n != "none"])
def test_polygon_masks_kernel(z, name):
    build, canvas, have = ac.POLY_CASES[name]
    objects = objects_of(z, name)
    m1, c1 = device_polygon_masks(objects, canvas, have)
    m2, c2 = device_polygon_masks(objects, canvas, have)
    assert torch.equal(m1, m2) and np.array_equal(c1, c2)
    exp = masks_of(z, name)
    got = m1.cpu().numpy()
    for k in range(len(exp)):
        assert np.array_equal(got[k], exp[k]), (name, k, int((got[k] != exp[k]).sum()))
    assert np.array_equal(c1, (exp > 0).sum(axis=(1, 2)))


def device_rays(kind, src, H, W, boxes, N, inst_id=None):
    dev = _dev()
    L = _C.lib()
    n = len(boxes)
    box = torch.from_numpy(np.ascontiguousarray(boxes, np.float64)).to(dev)
    poly = torch.full((n, N, 2), -7, dtype=torch.int32, device=dev)
    if kind == "ids":
        iid = torch.from_numpy(np.asarray(inst_id, np.int32)).to(dev)
        rc = L.cp_annot_rays_ids(_C.ptr(src), H, W, _C.ptr(iid), _C.ptr(box), n, N, _C.ptr(poly), _C.stream())
    else:
        rc = L.cp_annot_rays_masks(_C.ptr(src), H, W, _C.ptr(box), n, N, _C.ptr(poly), _C.stream())
    _C.check(rc, "cp_annot_rays_" + kind)
    return poly.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["int", "float"])
def test_rays_box_points(z, kind):
    """An all-set mask returns every ray's start point: the box points themselves, through both entry points."""
    boxes = ac.point_boxes()[0 if kind == "int" else 1]
    W, H = ac.POINT_CANVAS
    dev = _dev()
    ids = torch.full((H, W), 26 * 256 + 3, dtype=torch.int16, device=dev)
    masks = torch.full((len(boxes), H, W), 255, dtype=torch.uint8, device=dev)
    for N in ac.BOX_POINT_COUNTS:
        exp = z["points_%s_%d" % (kind, N)]
        a = device_rays("ids", ids, H, W, boxes, N, [26 * 256 + 3] * len(boxes))
        b = device_rays("masks", masks, H, W, boxes, N)
        assert np.array_equal(a, exp), (N, np.argwhere(a != exp)[:4])
        assert np.array_equal(b, exp), N


@pytest.mark.gpu
@pytest.mark.parametrize("name", ID_NAMES)
def test_rays_ids_kernel(z, name):
    ids = ids_of(z, name)
    H, W = ids.shape
    src = torch.from_numpy(ids.view(np.int16)).to(_dev())
    inst = [v for v, _, _ in host.id_objects(ids, ac.KITTI_LABELS, 256)]
    boxes = z["ids_%s_bbox" % name]
    for N in ac.ID_COUNTS[name]:
        a = device_rays("ids", src, H, W, boxes, N, inst)
        b = device_rays("ids", src, H, W, boxes, N, inst)
        assert np.array_equal(a, b)
        assert np.array_equal(a, z["ids_%s_poly%d" % (name, N)]), (name, N)


@pytest.mark.gpu
@pytest.mark.parametrize("name", [n for n in POLY_NAMES if n != "none"])
def test_rays_masks_kernel(z, name):
    W, H = ac.POLY_CASES[name][1]
    src = torch.from_numpy(masks_of(z, name)).to(_dev())           # PIL's recorded masks
    boxes = z["poly_%s_bbox" % name]
    for N in ac.POLY_COUNTS[name]:
        a = device_rays("masks", src, H, W, boxes, N)
        b = device_rays("masks", src, H, W, boxes, N)
        assert np.array_equal(a, b)
        assert np.array_equal(a, z["poly_%s_poly%d" % (name, N)]), (name, N)


@pytest.mark.gpu
def test_library_on_the_device(z):
    for name in ("shapes", "many129", "one"):
        ids = ids_of(z, name)
        counts = list(ac.ID_COUNTS[name])
        r = annotate.from_id_image(torch.from_numpy(ids.view(np.int16)).to(_dev()), ac.KITTI_LABELS, 256, counts)
        assert np.array_equal(r["bbox"], z["ids_%s_bbox" % name])
        assert np.array_equal(r["cls"], label_class(z["ids_%s_label" % name]))
        assert r["pseudo_depth"].tolist() == list(range(len(r["cls"])))
        for N in counts:
            assert np.array_equal(r["poly"][N], z["ids_%s_poly%d" % (name, N)])
    empty = annotate.from_id_image(torch.zeros((5, 7), dtype=torch.int16, device=_dev()), ac.KITTI_LABELS, 256, 16)
    assert empty["poly"].shape == (0, 16, 2) and empty["bbox"].shape == (0, 4)
    for name in ("small", "idd", "none", "long"):
        build, canvas, have = ac.POLY_CASES[name]
        counts = list(ac.POLY_COUNTS[name])
        r = annotate.from_polygons(objects_of(z, name), canvas, have, counts, device=_dev())
        assert r["label"] == z["poly_%s_label" % name].tolist()
        assert np.array_equal(r["bbox"], z["poly_%s_bbox" % name])
        assert np.array_equal(r["counts"], (masks_of(z, name) > 0).sum(axis=(1, 2)))
        for N in counts:
            assert np.array_equal(r["poly"][N], z["poly_%s_poly%d" % (name, N)]), (name, N)
    # more objects than one kernel call takes: the list is walked in slices
    tri = [{"label": "car", "polygon": [[1 + k % 40, 2], [9 + k % 40, 5 + k % 7], [3 + k % 40, 11]]} for k in range(131)]
    r = annotate.from_polygons(tri, (53, 37), ["car"], 8, device=_dev())
    h = host.from_polygons(tri, (53, 37), ["car"], 8)
    assert np.array_equal(r["poly"], h["poly"]) and np.array_equal(r["counts"], h["counts"])


def _write_ids_png(path, ids):
    from PIL import Image
    os.makedirs(os.path.dirname(path), exist_ok=True)
    Image.fromarray(ids).save(path)


@pytest.mark.gpu
def test_driver_end_to_end(z, tmp_path):
    import make_annotations as ma
    from PIL import Image
    root = str(tmp_path)
    # KITTI: 21 id images, the three files of the split rule
    for i in range(21):
        os.makedirs(os.path.join(root, "image_2"), exist_ok=True)
        Image.new("RGB", (9, 6)).save(os.path.join(root, "image_2", "%06d_10.png" % i))
        _write_ids_png(os.path.join(root, "instance", "%06d_10.png" % i), ac.kitti_dir_image(i))
    ma.run(ma.parse_args(["--dataset", "kitti_poly", "--img_dir", os.path.join(root, "image_2"), "--gt_dir",
                          os.path.join(root, "instance"), "--out_dir", os.path.join(root, "out"), "--nbr_points", "4",
                          "--num_workers", "0"]))
    for part in ("train", "val", "trainval"):
        with open(os.path.join(root, "out", "%s4.json" % part)) as f:
            same_json(json.load(f), recorded_json(z, "json_kitti21_%s" % part, root))
    # IDD: polygon files on the images' own canvas; Cityscapes: the fixed canvas
    for ds, split, N, key, items, size in (
            ("IDD", "train", 16, "json_idd_train16", (("7/000010", "idd"), ("7/000020", "none"), ("9/000005", "idd")), (53, 37)),
            ("cityscapes", "val", 8, "json_cityscapes_val8",
             (("aa/aa_000001_000019", "small"), ("aa/aa_000002_000019", "none"), ("bb/bb_000000_000001", "full")), (8, 4))):
        img_dir, gt_dir = os.path.join(root, "leftImg8bit", split), os.path.join(root, "gtFine", split)
        for stem, case in items:
            os.makedirs(os.path.dirname(os.path.join(img_dir, stem)), exist_ok=True)
            os.makedirs(os.path.dirname(os.path.join(gt_dir, stem)), exist_ok=True)
            Image.new("RGB", size).save(os.path.join(img_dir, stem + "_leftImg8bit.png"))
            with open(os.path.join(gt_dir, stem + "_gtFine_polygons.json"), "w") as f:
                json.dump({"imgHeight": size[1], "imgWidth": size[0], "objects": objects_of(z, case)}, f)
        out = os.path.join(root, "out_" + ds)
        ma.run(ma.parse_args(["--dataset", ds, "--split", split, "--img_dir", img_dir, "--gt_dir", gt_dir, "--out_dir",
                              out, "--nbr_points", str(N), "--num_workers", "0"]))
        with open(os.path.join(out, "%s%d_regular_interval.json" % (split, N))) as f:
            same_json(json.load(f), recorded_json(z, key, root))

"""Generates tests/golden/annotations.npz: what the reference's offline annotation tools and its converter give for
the inputs of annotation_cases.py.  Run from the repository root where the reference lies beside it:
    python tests/golden/gen_annotations_golden.py [REFERENCE_ROOT]

The three tools (KITTIPolyStuff/Tools/create_annotations.py, cityscapesStuff/Tools/create_bouding_box_annotations.py,
IDDStuff/Tools/create_annotations.py) run their loops over hard-coded paths at import and need cv2 and the
`bresenham` package, so they are not imported: each file is parsed, and only its function definitions
`find_points_from_box`, `find_first_non_zero_pixel` and `polygon_to_box` are compiled, into a namespace that holds
numpy and a `bresenham` module made of oracle.writer.bresenham (the package's generator, restated).  The expected
values come from those functions.  The per-image loops and src/tools/convert_csv_to_coco.py are transcribed below with
line citations; masks are drawn by the installed PIL with the tools' own calls.  The fixture holds inputs and recorded
outputs only."""
import ast
import csv
import io
import json
import os
import sys
import types

import numpy as np
from PIL import Image, ImageDraw

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import annotation_cases as ac  # noqa: E402
from oracle.writer import bresenham as _bresenham  # noqa: E402

WANTED = ("find_points_from_box", "find_first_non_zero_pixel", "polygon_to_box")
TOOLS = {"kitti": "KITTIPolyStuff/Tools/create_annotations.py",
         "cityscapes": "cityscapesStuff/Tools/create_bouding_box_annotations.py",
         "IDD": "IDDStuff/Tools/create_annotations.py"}
PATH_ROOT = "/ROOT"                                             # stands for the directory the test makes


def tool_functions(path):
    tree = ast.parse(open(path).read(), path)
    body = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in WANTED]
    assert sorted(n.name for n in body) == sorted(WANTED), path
    mod = types.ModuleType("bresenham")
    mod.bresenham = _bresenham
    ns = {"np": np, "bresenham": mod}
    exec(compile(ast.Module(body=body, type_ignores=[]), path, "exec"), ns)
    return types.SimpleNamespace(**{k: ns[k] for k in WANTED})


def regular_interval(fn, bbox, mask, N):
    """create_bouding_box_annotations.py:185-190 = create_annotations.py (KITTI) :152-157 = (IDD) :139-144."""
    x0, y0, x1, y1 = bbox
    points_on_box = fn.find_points_from_box(box=bbox, n_points=N)
    points_on_border = []
    ct = int(x0 + ((x1 - x0) / 2)), int(y0 + ((y1 - y0) / 2))
    for point_on_box in points_on_box:
        line = fn.bresenham_line(int(point_on_box[0]), int(point_on_box[1]), int(ct[0]), int(ct[1]))
        points_on_border.append(fn.find_first_non_zero_pixel(line, mask))
    return points_on_border


def kitti_rows(fn, path, gt16, N):
    """KITTI create_annotations.py:112-166 for one image: cv2.imread(gt, 0) of a 16-bit PNG is its high byte,
    IMREAD_UNCHANGED the 16-bit values."""
    gt_labels = (gt16 >> 8).astype(np.uint8)                                                  # :114
    id_to_label = {24: "person", 25: "rider", 26: "car", 27: "truck", 28: "bus", 31: "train", 32: "motorcycle",
                   33: "bicycle"}                                                             # :15-16
    instances_mask = np.isin(gt_labels, list(id_to_label)).astype(gt16.dtype)                 # :115-126
    gt_ids = gt16 * instances_mask                                                            # :128
    rows, count = [], 0
    for id in np.unique(gt_ids):                                                              # :129-132
        if id == 0:
            continue
        id_mask = gt_ids.copy()                                                               # :135-138
        id_mask[id_mask == 255] = 0
        id_mask[id_mask == id] = 255
        id_mask[id_mask != 255] = 0
        ys, xs = np.where(gt_ids == id)                                                       # :141
        bbox = x0, y0, x1, y1 = np.min(xs), np.min(ys), np.max(xs), np.max(ys)                # :142
        if gt_labels[ys[0], xs[0]] not in id_to_label:                                        # :146
            continue
        label = id_to_label[gt_labels[ys[0], xs[0]]]
        items = [path, x0, y0, x1, y1, label, count]                                          # :150
        for point in np.array(regular_interval(fn, bbox, id_mask, N)).flatten():              # :152-160
            items.append(point)
        rows.append(tuple(items))
        count += 1                                                                            # :166
    return rows


def polygon_rows(fn, path, objects, canvas, have_instances, N, masks_out=None):
    """create_bouding_box_annotations.py:141-213 (method regular_interval) = IDD create_annotations.py:107-166."""
    objects = [dict(o) for o in objects]
    objects.reverse()                                                                         # :143
    rows, count = [], 0
    for object in objects:
        label = object["label"]
        if label in have_instances:                                                           # :147
            bbox = x0, y0, x1, y1 = fn.polygon_to_box(object["polygon"])                      # :149
            items = [path, x0, y0, x1, y1, label, count]
            poly_img = Image.new("L", canvas, 0)                                              # :182-184
            ImageDraw.Draw(poly_img).polygon([tuple(item) for item in object["polygon"]], outline=0, fill=255)
            poly_img = np.array(poly_img)
            if masks_out is not None:
                masks_out.append(poly_img)
            for point in np.array(regular_interval(fn, bbox, poly_img, N)).flatten():         # :185-207
                items.append(point)
            rows.append(tuple(items))
            count += 1
    if count == 0:
        rows.append((path, -1, -1, -1, -1, "no_object", 0))                                   # :212-213
    return rows


def csv_lines(rows):
    """The tools' csv.writer (delimiter ',', QUOTE_NONE), read back as convert_csv_to_coco.py reads it: readlines()."""
    buf = io.StringIO()
    w = csv.writer(buf, delimiter=",", quotechar="", quoting=csv.QUOTE_NONE)
    for r in rows:
        w.writerow(r)
    return buf.getvalue().splitlines(True)


def convert_csv_to_coco(csv_lines_, cats):
    """src/tools/convert_csv_to_coco.py:110-174."""
    def _bbox_to_coco_bbox(bbox):                                                             # :110-112
        return [(bbox[0]), (bbox[1]), (bbox[2] - bbox[0]), (bbox[3] - bbox[1])]
    cat_ids = {cat: i + 1 for i, cat in enumerate(cats)}                                      # :117-120
    cat_info = [{"name": cat, "id": i + 1} for i, cat in enumerate(cats)]
    image_to_boxes = {}
    for line in csv_lines_:                                                                   # :128-137
        items = line.split(",")
        if items[0] in image_to_boxes:
            image_to_boxes[items[0]].append(items[1:])
        else:
            image_to_boxes[items[0]] = [items[1:]]
    ret = {"images": [], "annotations": [], "categories": cat_info}
    for count, path in enumerate(sorted(image_to_boxes)):                                     # :139
        ret["images"].append({"file_name": path, "id": count, "calib": ""})
        for ann_ind, box in enumerate(image_to_boxes[path]):
            x0, y0, x1, y1, label, pseudo_depth = int(float(box[0])), int(float(box[1])), int(float(box[2])), \
                int(float(box[3])), box[4], int(box[5])                                       # :147
            poly_points = [float(item) for item in box[6:]]
            if label.strip() == "no_object" or label.strip() not in cat_ids:                  # :149
                continue
            bbox = [float(x0), float(y0), float(x1), float(y1)]
            ret["annotations"].append({"image_id": count, "id": int(len(ret["annotations"]) + 1),
                                       "category_id": cat_ids[label.strip()], "bbox": _bbox_to_coco_bbox(bbox),
                                       "truncated": 0, "occluded": 0, "iscrowd": 0,
                                       "area": (bbox[3] - bbox[1]) * (bbox[2] - bbox[0]), "poly": poly_points,
                                       "pseudo_depth": pseudo_depth})
    return ret


def rows_to_arrays(rows, N):
    """(bbox float64 [n, 4], labels, depth, poly int32 [n, N, 2]) of one image's rows (no_object rows left out)."""
    rows = [r for r in rows if r[5] != "no_object"]
    return (np.array([[float(c) for c in r[1:5]] for r in rows], np.float64).reshape(-1, 4), [r[5] for r in rows],
            np.array([r[6] for r in rows], np.int64), np.array([r[7:] for r in rows], np.int32).reshape(len(rows), N, 2))


def main(ref):
    fns = {}
    for k, rel in TOOLS.items():
        fns[k] = tool_functions(os.path.join(ref, rel))
        fns[k].bresenham_line = _bresenham
    out = {}

    # box points: an all-set mask returns the (clipped) start point of every ray
    ints, floats = ac.point_boxes()
    W, H = ac.POINT_CANVAS
    full = np.full((H, W), 255, np.uint8)
    for name, boxes, fn in (("int", ints, fns["kitti"]), ("float", floats, fns["IDD"])):
        for N in ac.BOX_POINT_COUNTS:
            exp = []
            for b in boxes:
                b = tuple(int(c) for c in b) if name == "int" else tuple(float(c) for c in b)
                exp.append(regular_interval(fn, b, full, N))
            out["points_%s_%d" % (name, N)] = np.array(exp, np.int32)

    # id images
    for name, build in ac.ID_CASES.items():
        ids = build()
        if name in ac.ID_STORED:
            out["ids_%s" % name] = ids
        for N in ac.ID_COUNTS[name]:
            rows = kitti_rows(fns["kitti"], "x.png", ids, N)
            bbox, labels, depth, poly = rows_to_arrays(rows, N)
            out["ids_%s_bbox" % name] = bbox.astype(np.int64)
            out["ids_%s_label" % name] = np.array(labels, dtype="U16")
            out["ids_%s_poly%d" % (name, N)] = poly

    # polygon lists
    for name, (build, canvas, have) in ac.POLY_CASES.items():
        objects = build()
        out["poly_%s_objects" % name] = np.array(json.dumps(objects))
        fn = fns["IDD" if have is ac.IDD_HAVE else "cityscapes"]
        for N in ac.POLY_COUNTS[name]:
            masks = []
            rows = polygon_rows(fn, "x.png", objects, canvas, have, N, masks)
            bbox, labels, depth, poly = rows_to_arrays(rows, N)
            out["poly_%s_bbox" % name] = bbox
            out["poly_%s_label" % name] = np.array(labels, dtype="U16")
            out["poly_%s_poly%d" % (name, N)] = poly
        if name != "small_full":
            m = np.stack(masks) if masks else np.zeros((0, canvas[1], canvas[0]), np.uint8)
            assert set(np.unique(m)) <= {0, 255}
            out["poly_%s_masks" % name] = np.packbits(m > 0, axis=2)

    # files: the KITTI split rule
    for count in (19, 20, 21, 40):
        N = 4
        train, val, trainval = [], [], []
        image_count = 0
        for i in range(count):                                                                # KITTI :106-166
            path = "%s/image_2/%06d_10.png" % (PATH_ROOT, i)
            image_count += 1
            rows = kitti_rows(fns["kitti"], path, ac.kitti_dir_image(i), N)
            trainval += rows
            (val if image_count % 20 == 0 else train).extend(rows)
        for key, rows in (("train", train), ("val", val), ("trainval", trainval)):
            out["json_kitti%d_%s" % (count, key)] = np.array(json.dumps(convert_csv_to_coco(csv_lines(rows), ac.CITYSCAPES_CATS)))
    rows = [("%s/image_2/%06d_10.png" % (PATH_ROOT, i), 0, 0, 1, 1, "car", 0) for i in range(3)]   # KITTI :110
    out["json_kitti_test"] = np.array(json.dumps(convert_csv_to_coco(csv_lines(rows), ac.CITYSCAPES_CATS)))

    # files: IDD (the image's own canvas) and Cityscapes (2048 x 1024)
    rows = []
    for stem, case in (("7/000010", "idd"), ("7/000020", "none"), ("9/000005", "idd")):
        path = "%s/leftImg8bit/train/%s_leftImg8bit.png" % (PATH_ROOT, stem)
        rows += polygon_rows(fns["IDD"], path, ac.POLY_CASES[case][0](), (53, 37), ac.IDD_HAVE, 16)
    out["json_idd_train16"] = np.array(json.dumps(convert_csv_to_coco(csv_lines(rows), ac.IDD_HAVE)))
    rows = []
    for stem, case in (("aa/aa_000001_000019", "small"), ("aa/aa_000002_000019", "none"), ("bb/bb_000000_000001", "full")):
        path = "%s/leftImg8bit/val/%s_leftImg8bit.png" % (PATH_ROOT, stem)
        rows += polygon_rows(fns["cityscapes"], path, ac.POLY_CASES[case][0](), (2048, 1024), ac.CITYSCAPES_HAVE, 8)
    out["json_cityscapes_val8"] = np.array(json.dumps(convert_csv_to_coco(csv_lines(rows), ac.CITYSCAPES_CATS)))

    dst = os.path.join(HERE, "annotations.npz")
    np.savez_compressed(dst, **out)
    print("wrote %s: %d arrays, %d bytes" % (dst, len(out), os.path.getsize(dst)))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(ROOT), "reference"))

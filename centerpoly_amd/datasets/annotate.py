"""Training annotations from ground truth: the "regular interval" recipe of the reference's offline tools
(KITTIPolyStuff/Tools/create_annotations.py, cityscapesStuff/Tools/create_bouding_box_annotations.py,
IDDStuff/Tools/create_annotations.py) and the file format of src/tools/convert_csv_to_coco.py.

The pixel work of one image -- the objects and boxes of an id image, the PIL masks of ground-truth polygons, the N
rays of every object -- runs on the device (csrc/annotate.hip; the contracts are in include/centerpoly_hip.h).  This
module holds the bookkeeping around it: which objects are kept and which pseudo-depth they take, the limits, and the
JSON writer.  There is no CPU fallback: a host tensor raises `_C.NativeError`."""
import json
import os

import numpy as np
import torch

from .. import _C

MAX_INSTANCES = 1024              # objects of one id image (cp_annot_id_instances)
MAX_POLYGONS = 128                # polygons of one cp_polygon_masks call; from_polygons walks longer lists in slices
MAX_POLYGON_VERTICES = 4096
VERTEX_BOUND = 1 << 24            # the rasteriser's exactness bound
KITTI_VAL_EVERY = 20              # create_annotations.py:162


def check_nbr_points(nbr_points):
    """The list of vertex counts, each a multiple of four in 4 .. 64."""
    values = [nbr_points] if isinstance(nbr_points, (int, np.integer)) else list(nbr_points)
    for n in values:
        if int(n) != n or n < 4 or n > 64 or n % 4:
            raise ValueError("nbr_points must be a multiple of four in 4 .. 64, got %r" % (n,))
    return [int(n) for n in values]


def _poly_result(polys, nbr_points):
    return polys[0] if isinstance(nbr_points, (int, np.integer)) else dict(zip(check_nbr_points(nbr_points), polys))


def from_id_image(ids_dev, class_label, divisor, nbr_points):
    """The objects of one 16-bit instance image v = label * divisor + k, as the KITTI tool takes them
    (create_annotations.py:107-166): the distinct non-zero values whose label is one of `class_label`, ascending.
    ids_dev: device tensor [H, W] of 16-bit elements holding the uint16 bits.  Returns host arrays
    bbox int64 [n, 4] (x0, y0, x1, y1: min / max of the object's pixels), cls int64 [n] (index into class_label),
    inst_id int64 [n], pseudo_depth int64 [n] (the rank) and poly int32 [n, N, 2] -- a dict {N: array} when
    nbr_points is a list."""
    ids_ptr = _C.ptr(ids_dev)
    counts = check_nbr_points(nbr_points)
    if ids_dev.dim() != 2 or ids_dev.element_size() != 2 or ids_dev.is_floating_point():
        raise ValueError("the id image must be [H, W] of 16-bit integers, got %s %s" % (tuple(ids_dev.shape), ids_dev.dtype))
    labels = [int(v) for v in class_label]
    if not 1 <= len(labels) <= 32 or int(divisor) < 1:
        raise ValueError("1 .. 32 class labels and a divisor >= 1 are needed")
    H, W = (int(v) for v in ids_dev.shape)
    dev = ids_dev.device
    L = _C.lib()
    label_arr = (_C.c_int32 * len(labels))(*labels)
    head = torch.empty((1 + 6 * MAX_INSTANCES,), dtype=torch.int32, device=dev)     # n, ids, classes, boxes: one read
    n_out, inst_id, cls = head[:1], head[1:1 + MAX_INSTANCES], head[1 + MAX_INSTANCES:1 + 2 * MAX_INSTANCES]
    box = head[1 + 2 * MAX_INSTANCES:]
    ws_bytes = L.cp_annot_id_instances_workspace_bytes()
    ws = _C.workspace(ws_bytes, dev)
    _C.check(L.cp_annot_id_instances(ids_ptr, H, W, label_arr, len(labels), int(divisor), MAX_INSTANCES,
                                     _C.ptr(n_out), _C.ptr(inst_id), _C.ptr(cls), _C.ptr(box), _C.ptr(ws), ws_bytes,
                                     _C.stream()), "cp_annot_id_instances")
    n = int(n_out.item())
    if n > MAX_INSTANCES:
        raise ValueError("%d objects in one id image, at most %d are supported" % (n, MAX_INSTANCES))
    box_f64 = box.view(MAX_INSTANCES, 4)[:n].to(torch.float64).contiguous()
    polys = []
    for N in counts:
        poly = torch.zeros((n, N, 2), dtype=torch.int32, device=dev)
        _C.check(L.cp_annot_rays_ids(ids_ptr, H, W, _C.ptr(inst_id), _C.ptr(box_f64) if n else None, n, N,
                                     _C.ptr(poly) if n else None, _C.stream()), "cp_annot_rays_ids")
        polys.append(poly)
    host = head.cpu().numpy().astype(np.int64)
    return {"bbox": host[1 + 2 * MAX_INSTANCES:].reshape(MAX_INSTANCES, 4)[:n].copy(),
            "cls": host[1 + MAX_INSTANCES:1 + MAX_INSTANCES + n].copy(),
            "inst_id": host[1:1 + n].copy(),
            "pseudo_depth": np.arange(n, dtype=np.int64),
            "poly": _poly_result([p.cpu().numpy() for p in polys], nbr_points)}


def kept_objects(objects, have_instances):
    """[(label, polygon)] of a `*_gtFine_polygons.json` object list in the tools' order: the list reversed, the
    objects whose label is in have_instances (create_bouding_box_annotations.py:142-147).  The place in this list is
    the pseudo-depth."""
    return [(o["label"], o["polygon"]) for o in reversed(objects) if o["label"] in have_instances]


def from_polygons(objects, canvas, have_instances, nbr_points, device=None, what="the image"):
    """The kept objects of one `*_gtFine_polygons.json` (`objects`: the file's list, in file order) on a canvas
    (width, height), as the Cityscapes and IDD tools take them.  The mask of an object is PIL's
    polygon(outline=0, fill=255) of its own polygon, vertices truncated towards zero; its box is the min / max of the
    vertices as they are.  Returns label (list of str), bbox float64 [n, 4], pseudo_depth int64 [n], counts int64 [n]
    (the mask's pixels) and poly int32 [n, N, 2] -- a dict {N: array} when nbr_points is a list.  A polygon of fewer
    than 3 or more than MAX_POLYGON_VERTICES vertices, or a vertex beyond +-2^24, is an error that names it."""
    counts = check_nbr_points(nbr_points)
    W, H = int(canvas[0]), int(canvas[1])
    if W < 1 or H < 1 or W * H >= 1 << 31:
        raise ValueError("canvas %s: width and height must be positive and width * height < 2^31" % (canvas,))
    kept = kept_objects(objects, have_instances)
    n = len(kept)
    bbox = np.zeros((n, 4), np.float64)
    verts, first = [], [0]
    for k, (label, polygon) in enumerate(kept):
        pts = np.asarray(polygon, np.float64).reshape(-1, 2) if len(polygon) else np.zeros((0, 2))
        if not 3 <= len(pts) <= MAX_POLYGON_VERTICES:
            raise ValueError("%s: object %d (%s, counted from the end of the file) has %d vertices; 3 .. %d are supported"
                             % (what, k, label, len(pts), MAX_POLYGON_VERTICES))
        if not np.all(np.abs(pts) <= VERTEX_BOUND):
            raise ValueError("%s: object %d (%s) has a vertex beyond +-2^24" % (what, k, label))
        bbox[k] = pts[:, 0].min(), pts[:, 1].min(), pts[:, 0].max(), pts[:, 1].max()
        verts.append(np.trunc(pts).astype(np.int32))
        first.append(first[-1] + len(pts))
    dev = torch.device("cuda") if device is None else torch.device(device)
    L = _C.lib()
    polys = [np.zeros((n, N, 2), np.int32) for N in counts]
    pixels = np.zeros((n,), np.int64)
    for lo in range(0, n, MAX_POLYGONS):
        hi = min(n, lo + MAX_POLYGONS)
        m, T = hi - lo, first[hi] - first[lo]
        xy = torch.from_numpy(np.concatenate(verts[lo:hi])).to(dev)
        box_dev = torch.from_numpy(bbox[lo:hi].copy()).to(dev)
        first_arr = (_C.c_int32 * (m + 1))(*[f - first[lo] for f in first[lo:hi + 1]])
        masks = torch.empty((m, H, W), dtype=torch.uint8, device=dev)
        cnt = torch.empty((m,), dtype=torch.int32, device=dev)
        ws_bytes = L.cp_polygon_masks_workspace_bytes(m, T)
        ws = _C.workspace(ws_bytes, dev)
        _C.check(L.cp_polygon_masks(_C.ptr(xy), first_arr, m, H, W, _C.ptr(masks), _C.ptr(cnt), _C.ptr(ws), ws_bytes,
                                    _C.stream()), "cp_polygon_masks")
        outs = []
        for N in counts:
            poly = torch.empty((m, N, 2), dtype=torch.int32, device=dev)
            _C.check(L.cp_annot_rays_masks(_C.ptr(masks), H, W, _C.ptr(box_dev), m, N, _C.ptr(poly), _C.stream()),
                     "cp_annot_rays_masks")
            outs.append(poly)
        for dst, poly in zip(polys, outs):
            dst[lo:hi] = poly.cpu().numpy()
        pixels[lo:hi] = cnt.cpu().numpy()
    return {"label": [label for label, _ in kept], "bbox": bbox, "pseudo_depth": np.arange(n, dtype=np.int64),
            "counts": pixels, "poly": _poly_result(polys, nbr_points)}


# ------------------------------------------------------------------------------------------- the file format ----
def placeholder_row():
    """The row the tools write for an image of a test split: (0, 0, 1, 1, 'car', 0) and no polygon."""
    return ((0, 0, 1, 1), "car", 0, [])


def coco_dict(images, class_names):
    """convert_csv_to_coco.py:123-174.  images: [(file_name, rows)], rows [(box (x0, y0, x1, y1), label,
    pseudo_depth, poly: flat numbers)] in the tools' order; class_names: the data set's classes, category ids
    count from 1.  Images are numbered in sorted path order; a row whose label is no class (Cityscapes' pole, traffic
    sign and traffic light) is dropped and leaves its gap in the pseudo-depths; the box is int(float(.)) of the
    tool's numbers."""
    cat_ids = {name: i + 1 for i, name in enumerate(class_names)}
    ret = {"images": [], "annotations": [], "categories": [{"name": name, "id": i + 1} for i, name in enumerate(class_names)]}
    by_path = {}
    for file_name, rows in images:
        by_path.setdefault(file_name, []).extend(rows)
    for count, path in enumerate(sorted(by_path)):
        ret["images"].append({"file_name": path, "id": count, "calib": ""})
        for box, label, pseudo_depth, poly in by_path[path]:
            if label not in cat_ids:
                continue
            x0, y0, x1, y1 = (float(int(float(v))) for v in box)
            ret["annotations"].append({"image_id": count, "id": len(ret["annotations"]) + 1,
                                       "category_id": cat_ids[label], "bbox": [x0, y0, x1 - x0, y1 - y0],
                                       "truncated": 0, "occluded": 0, "iscrowd": 0, "area": (y1 - y0) * (x1 - x0),
                                       "poly": [float(v) for v in np.asarray(poly).reshape(-1)],
                                       "pseudo_depth": int(pseudo_depth)})
    return ret


def write_annotations(path, images, class_names):
    """coco_dict as a JSON file; returns (images, annotations) written."""
    ret = coco_dict(images, class_names)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(ret, f)
    return len(ret["images"]), len(ret["annotations"])


def kitti_val_image(image_count):
    """create_annotations.py:162: every 20th image of the sorted list (counted from 1) is a validation image."""
    return image_count % KITTI_VAL_EVERY == 0

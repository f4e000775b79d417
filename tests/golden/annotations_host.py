"""The annotation recipe on the host, stated from its contract (include/centerpoly_hip.h, "training annotations"):
what csrc/annotate.hip computes, in plain Python and numpy.  TEST INFRASTRUCTURE: the CPU tests hold it against the
fixtures that tests/golden/gen_annotations_golden.py recorded from the reference's own functions and the installed
PIL; tools/probe_annotate.py times it as the host baseline.

`polygon_mask` is the long-polygon fill of cp_polygon_masks: the rules of csrc/class_masks_core.h as
tests/golden/pil_scanline_host.py states them, of any length."""
import numpy as np

import pil_scanline_host
from oracle.writer import bresenham


# ------------------------------------------------------------------------------------------------- the rays ----
def box_points(box, N):
    """The N start points: N / 4 on each side, clockwise from the top-left corner, round() = half to even on
    fl(x0 + fl(i * q)) in float64; the other coordinate is the box's own number."""
    x0, y0, x1, y1 = box
    k = N // 4
    qx, qy = (x1 - x0) / k, (y1 - y0) / k
    pts = [(round(x0 + i * qx), y0) for i in range(k)]
    pts += [(x1, round(y0 + i * qy)) for i in range(k)]
    pts += [(round(x1 - i * qx), y1) for i in range(k)]
    pts += [(x0, round(y1 - i * qy)) for i in range(k)]
    return pts


def centre(box):
    x0, y0, x1, y1 = box
    return int(x0 + (x1 - x0) / 2), int(y0 + (y1 - y0) / 2)


def ray_vertex(start, end, mask):
    """The first pixel of the package's line start -> end, clipped to the canvas, whose mask is set; the last
    (clipped) pixel when there is none."""
    H, W = mask.shape
    px = py = 0
    for x, y in bresenham(int(start[0]), int(start[1]), int(end[0]), int(end[1])):
        px, py = min(max(x, 0), W - 1), min(max(y, 0), H - 1)
        if mask[py, px] > 0:
            break
    return px, py


def object_polygon(box, mask, N):
    ct = centre(box)
    return [ray_vertex(p, ct, mask) for p in box_points(box, N)]


# -------------------------------------------------------------------------------------------- the id image ----
def id_objects(ids, class_label, divisor):
    """[(value, class index, (x0, y0, x1, y1))]: the distinct non-zero values whose label v // divisor is one of
    class_label, ascending."""
    out = []
    labels = [int(v) for v in class_label]
    for v in np.unique(ids):
        v = int(v)
        if v == 0 or v // divisor not in labels:
            continue
        ys, xs = np.nonzero(ids == v)
        out.append((v, labels.index(v // divisor), (int(xs.min()), int(ys.min()), int(xs.max()), int(ys.max()))))
    return out


def from_id_image(ids, class_label, divisor, N):
    objs = id_objects(ids, class_label, divisor)
    poly = [object_polygon(box, ids == v, N) for v, _, box in objs]
    return {"bbox": np.array([b for _, _, b in objs], np.int64).reshape(-1, 4),
            "cls": np.array([c for _, c, _ in objs], np.int64),
            "inst_id": np.array([v for v, _, _ in objs], np.int64),
            "pseudo_depth": np.arange(len(objs), dtype=np.int64),
            "poly": np.array(poly, np.int32).reshape(len(objs), N, 2)}


# ------------------------------------------------------------------------------------------ polygon masks ----
polygon_fill = pil_scanline_host.fill                          # F: what ImageDraw.polygon(pts, fill=...) sets
polygon_outline = pil_scanline_host.outline                    # O: what ImageDraw.polygon(pts, outline=...) sets


def polygon_mask(polygon, W, H):
    """polygon(outline=0, fill=255) on a fresh 'L' image: F \\ O of the vertices truncated towards zero."""
    pts = [(int(x), int(y)) for x, y in polygon]
    return ((polygon_fill(pts, W, H) & ~polygon_outline(pts, W, H)) * 255).astype(np.uint8)


# ---------------------------------------------------------------------------------------- the polygon files ----
def polygon_box(polygon):
    xs, ys = [p[0] for p in polygon], [p[1] for p in polygon]
    return min(xs), min(ys), max(xs), max(ys)


def from_polygons(objects, canvas, have_instances, N, masks=None):
    """The kept objects of one polygon file (objects in file order) on canvas (W, H).  `masks`, when given, are
    used in place of polygon_mask (one per kept object)."""
    W, H = canvas
    kept = [(o["label"], o["polygon"]) for o in reversed(objects) if o["label"] in have_instances]
    bbox, poly, counts = [], [], []
    for k, (label, polygon) in enumerate(kept):
        box = polygon_box(polygon)
        mask = polygon_mask(polygon, W, H) if masks is None else masks[k]
        bbox.append(box)
        counts.append(int((mask > 0).sum()))
        poly.append(object_polygon(box, mask, N))
    return {"label": [label for label, _ in kept], "bbox": np.array(bbox, np.float64).reshape(-1, 4),
            "pseudo_depth": np.arange(len(kept), dtype=np.int64), "counts": np.array(counts, np.int64),
            "poly": np.array(poly, np.int32).reshape(len(kept), N, 2)}

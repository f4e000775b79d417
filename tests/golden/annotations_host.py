"""The annotation recipe on the host, stated from its contract (include/centerpoly_hip.h, "training annotations"):
what csrc/annotate.hip computes, in plain Python and numpy.  TEST INFRASTRUCTURE: the CPU tests hold it against the
fixtures that tests/golden/gen_annotations_golden.py recorded from the reference's own functions and the installed
PIL; tools/probe_annotate.py times it as the host baseline.

`polygon_mask` is the long-polygon fill of cp_polygon_masks: the rules of csrc/class_masks_core.h (transcribed in
tests/test_class_masks.py for polygons of up to 64 vertices) with each row's crossing list taken from the edges that
span the row."""
import numpy as np

from oracle.writer import bresenham

f32 = np.float32


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


# ---------------------------------------------------------------------------- class_masks_core.h, any length ----
def _round_up(f):
    f = f32(f)
    return int(np.floor(f + f32(0.5))) if f >= 0 else -int(np.floor(abs(f) + f32(0.5)))


def _round_down(f):
    f = f32(f)
    return int(np.ceil(f - f32(0.5))) if f >= 0 else -int(np.ceil(abs(f) - f32(0.5)))


def _edges(pts):
    """cm_make_edge for every k: (kind, x0, y0, ymin, ymax, xmin, xmax, dx); kind 0 absent, 1 flat, 2 sloped."""
    N, out = len(pts), []
    for k in range(N):
        (x0, y0), (x1, y1) = pts[k], pts[(k + 1) % N]
        kind = 0 if (k + 1 == N and (x0, y0) == (x1, y1)) else 1 if y0 == y1 else 2
        dx = f32(x1 - x0) / f32(y1 - y0) if kind == 2 else f32(0)
        out.append((kind, x0, y0, min(y0, y1), max(y0, y1), min(x0, x1), max(x0, x1), dx))
    return out


def _x_at(e, y):
    return f32(f32(y - e[2]) * e[7]) + f32(e[1])


def _crossings(E, k, y, last_row):
    """cm_crossings: what edge k adds to row y."""
    e = E[k]
    if e[0] != 2 or y < e[3] or y > e[4]:
        return []
    x = _x_at(e, y)
    if y == e[4] and y < last_row:
        return [x, x]
    if (y == e[3] or y == e[4]) and e[7] != 0:
        for j in range(k):
            o = E[j]
            if o[0] != 2 or o[7] == 0:
                continue
            if not ((y == e[3] and y == o[3]) or (y == e[4] and y == o[4])):
                continue
            if np.rint(x) != np.rint(_x_at(o, y)):
                continue
            if (e[7] > 0) == (o[7] > 0):
                adj = y - 1 if y == last_row else y + 1
                a, b = _x_at(e, adj), _x_at(o, adj)
                if (y == e[4]) != (e[7] > 0):
                    x = max(f32(_round_up(min(a, b)) - 1), x)
                else:
                    x = min(f32(_round_up(max(a, b)) + 1), x)
            break
    return [x]


def polygon_fill(pts, W, H):
    """F: what ImageDraw.polygon(pts, fill=...) sets."""
    m = np.zeros((H, W), bool)
    E = _edges(pts)
    ys = [p[1] for p in pts]
    last_row = min(max(0, max(ys)), H)
    by_row = {}
    for k, e in enumerate(E):                                  # the edges that can touch a row, in table order
        if e[0] == 0:
            continue
        for y in range(max(e[3], 0), min(e[4], H - 1) + 1):
            by_row.setdefault(y, []).append(k)
    for y in range(max(0, min(ys)), min(H - 1, last_row) + 1):
        ks = by_row.get(y, [])
        xx = sorted(v for k in ks for v in _crossings(E, k, y, last_row))
        spans = [(_round_up(xx[i - 1]), _round_down(xx[i])) for i in range(1, len(xx), 2)]
        spans += [(E[k][5], E[k][6]) for k in ks if E[k][0] == 1 and E[k][3] == y]
        for lo, hi in spans:
            lo, hi = max(lo, 0), min(hi, W - 1)
            if lo <= hi:
                m[y, lo:hi + 1] = True
    return m


def polygon_outline(pts, W, H):
    """O: what ImageDraw.polygon(pts, outline=...) sets (PIL's integer line of every edge)."""
    m = np.zeros((H, W), bool)
    for k in range(len(pts)):
        (x0, y0), (x1, y1) = pts[k], pts[(k + 1) % len(pts)]
        ax, ay = abs(x1 - x0), abs(y1 - y0)
        if ax == 0 and ay == 0:
            continue
        sx, sy = (1 if x1 >= x0 else -1), (1 if y1 >= y0 else -1)
        t = np.arange(max(ax, ay) + 1, dtype=np.int64)
        if ax > ay:
            px, py = x0 + sx * t, y0 + sy * ((2 * ay * t + ax) // (2 * ax))
        else:
            px, py = x0 + sx * ((2 * ax * t + ay) // (2 * ay)), y0 + sy * t
        ok = (px >= 0) & (px < W) & (py >= 0) & (py < H)
        m[py[ok], px[ok]] = True
    return m


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

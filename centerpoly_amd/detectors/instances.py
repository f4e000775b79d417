"""Instance maps of one image from its detection rows: which instance owns each pixel, the id and label images in the
data set's own `*_instanceIds.png` / `*_labelIds.png` convention, the per-instance masks as the data set's result
writer draws them, and a table of what every instance shows -- for any image and canvas, no annotation file needed.

Everything is done on the device by the kernels the result writers and the scoring path already use, followed by the
depth-resolved merge (cp_instance_map); one copy brings the small tables back.
  Cityscapes family (CityscapesWriterMixin): cp_writer_instances -> cp_instance_masks -> cp_instance_map.  Live: the
      writer's own selection, the label has masks and the mask has more than 100 pixels.  The slots are already in
      ascending depth, so the earlier slot wins; ids are label * 1000 + k.
  KITTI / IDD family (ClassWriterMixin): cp_class_writer_instances -> cp_class_instance_masks -> cp_instance_map.  Live:
      every instance the writer writes a mask file for, that is every selected row.  The slots are in drawing order
      (class, then depth), so the priority is the depth of the instance's source row: the nearer instance wins across
      classes too, ties go to the earlier slot.  Ids are label * 256 + k (KITTI) or label * 1000 + k (IDD), the
      multiplier of the data set's evaluation protocol.
`save_ids`, `save_masks` and `save_rle` write what demo.py and test.py offer as --save_ids, --save_masks and --save_rle
(the masks as COCO run-length strings, encoded on the device by utils/rle.py)."""
import ctypes
import json
import os

import numpy as np
import torch

from .. import _C
from ..datasets.dataset.polygons import CityscapesWriterMixin, ClassWriterMixin
from ..datasets.evaluation import instance_level as il

TILE = (16, 256)                                        # cp_instance_map's tile: rows, columns
MIN_PIXELS = 100                                        # the Cityscapes writer keeps a mask with more pixels than this
CITYSCAPES_MULTIPLIER = 1000
# Vertices beyond this are outside the range in which the mask kernels restate PIL: no statement about where such a
# drawing lies, so its bounds are the whole canvas.
EXACT_VERTEX = 1 << 24
# How far a drawing can reach beyond the box of its integer vertices.
#   KITTI / IDD: the mask is part of PIL's polygon fill.  A scan line y lies between the lowest and the highest vertex;
#   a span runs from round(xa) to round(xb) of two edge crossings, each between the x of its edge's end points, and
#   rounding a number of an interval with integer ends stays inside it; horizontal edges are drawn between their end
#   points.  So the fill stays inside the box: margin 0.
#   Cityscapes: the same fill, PIL's outline (integer lines between consecutive vertices, inside the box of their end
#   points) and a radius-2 ellipse, a subset of the 5 x 5 square, around every pixel of the Bresenham contour, which
#   again stays inside the box of its end points.  So the drawing stays inside the box grown by 2: margin 2.
MARGIN = {"cityscapes": 2, "class": 0}
TOO_MANY = "more than 128 instances in one image (max_per_image = K <= 128)"


def writer_family(dataset):
    """("cityscapes" | "class", the data set's class) of a data-set class or object."""
    cls = dataset if isinstance(dataset, type) else type(dataset)
    if issubclass(cls, CityscapesWriterMixin):
        return "cityscapes", cls
    if issubclass(cls, ClassWriterMixin):
        return "class", cls
    raise TypeError("data set %s has no result writer to draw instance masks with (cityscapes, kitti_poly and IDD "
                    "have)" % getattr(cls, "__name__", cls))


def vertex_bounds(poly, margin, canvas):
    """cp_instance_map's bounds of integer vertices int32 [S, N, 2] (device): the vertices' box grown by `margin` and
    clipped to the canvas, int32 [S, 4] inclusive x0, y0, x1, y1; the whole canvas for vertices beyond EXACT_VERTEX."""
    W, H = canvas
    p = poly.to(torch.int64)
    lo, hi = p.amin(1) - margin, p.amax(1) + margin
    b = torch.stack([lo[:, 0].clamp(0, W), lo[:, 1].clamp(0, H), hi[:, 0].clamp(-1, W - 1), hi[:, 1].clamp(-1, H - 1)], 1)
    far = p.abs().amax((1, 2)) > EXACT_VERTEX
    whole = torch.tensor([0, 0, W - 1, H - 1], dtype=torch.int64, device=poly.device)
    return torch.where(far[:, None], whole[None], b).to(torch.int32).contiguous()


def instance_map(masks, flags, label, flag_mask=1, counts=None, min_count=0, prio=None, bounds=None, multiplier=1000,
                 background=0, want_ids=True, want_labels=True):
    """cp_instance_map on device tensors: masks uint8 [n, H, W], flags uint8 [n], label int32 [n], optional counts
    int32 [n], prio float32 [n], bounds int32 [n, 4].  Returns device tensors (index uint8 [H, W], ids int32 [H, W] or
    None, labels int32 [H, W] or None, value int32 [n], visible int32 [n], box int32 [n, 4])."""
    n, H, W = (int(v) for v in masks.shape)
    dev = masks.device
    index = torch.empty((H, W), dtype=torch.uint8, device=dev)
    ids = torch.empty((H, W), dtype=torch.int32, device=dev) if want_ids else None
    labels = torch.empty((H, W), dtype=torch.int32, device=dev) if want_labels else None
    tables = torch.empty((6 * max(n, 1),), dtype=torch.int32, device=dev)
    value, visible, box = tables[:n], tables[n:2 * n], tables[2 * n:6 * n].view(n, 4)
    L = _C.lib()
    nbytes = L.cp_instance_map_workspace_bytes(n, H, W)
    ws = _C.workspace(nbytes, dev)
    at = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None and t.numel() else None      # noqa: E731
    _C.check(L.cp_instance_map(_C.ptr(masks) if n else None, n, H, W, at(flags), int(flag_mask), at(counts),
                               int(min_count), at(label), at(prio), at(bounds), int(multiplier), int(background),
                               _C.ptr(index), _C.ptr(ids), _C.ptr(labels), at(value), at(visible), at(box),
                               _C.ptr(ws), nbytes, _C.stream()), "cp_instance_map")
    return index, ids, labels, value, visible, box


class InstanceMaps(object):
    """What instance_maps returns.
      index   device uint8 [H, W]: the slot of the instance that owns the pixel, 255 where none does
      ids     device int32 [H, W]: label * multiplier + k of the owner, 0 where none
      labels  device int32 [H, W]: label id of the owner, 0 where none
      masks   device uint8 [S, H, W]: every slot's mask as the data set's writer draws it (hidden parts of a live
              instance included where the writer keeps them; `index` says who shows)
      table   host dict, read back in one copy, arrays over the n selected instances in slot order: n, src (source
              row), label, conf, count (pixels of the mask), live, value (-1 for a dead instance), visible (pixels
              owned), box (inclusive x0, y0, x1, y1 of the owned pixels; W, H, -1, -1 for none), and with them score,
              poly (integer vertices [n, N, 2]) and, in the KITTI / IDD family, text_index (the writer's numbering)
      family  "cityscapes" or "class"; canvas (width, height); names {label id: class name}; multiplier"""

    def __init__(self, family, canvas, index, ids, labels, masks, table, names, multiplier):
        self.family, self.canvas, self.index, self.ids, self.labels, self.masks = family, canvas, index, ids, labels, masks
        self.table, self.names, self.multiplier = table, names, multiplier

    def written(self):
        """The live slots in the order the data set's writer numbers its mask files."""
        live = [k for k in range(self.table["n"]) if self.table["live"][k]]
        if self.family == "class":
            live.sort(key=lambda k: int(self.table["text_index"][k]))
        return live

    def conf_text(self, k):
        """The confidence of slot k as the writer's text line spells it."""
        c = self.table["conf"][k]
        return str(min(1, c)) if self.family == "cityscapes" else str(c)


def instance_maps(rows_dev, dataset, canvas, thresh=None):
    """The instance maps of one image: device rows float32 [R, 2N + 7] in the layout of PolydetDetector.device_rows
    (x1,y1,x2,y2,score,cls,poly,depth; R <= 1024), a data-set class or object of the Cityscapes or the KITTI / IDD
    family (dataset_factory's classes: no annotation file is read), the canvas (width, height).  `thresh` defaults to
    the object's opt.thresh and is compared as the data set's writer compares it (> for Cityscapes and KITTI, >= for
    IDD).  Returns an InstanceMaps."""
    family, cls = writer_family(dataset)
    if thresh is None:
        opt = getattr(dataset, "opt", None)
        if opt is None:
            raise ValueError("instance_maps needs `thresh` when the data set is given as a class")
        thresh = opt.thresh
    W, H = (int(v) for v in canvas)
    if W < 1 or H < 1:
        raise ValueError("the canvas must be at least 1 x 1 (width, height), got %r" % (canvas,))
    if rows_dev.dim() != 2 or rows_dev.dtype != torch.float32 or rows_dev.shape[1] < 13 or rows_dev.shape[1] % 2 == 0:
        raise ValueError("rows must be float32 [R, 2N + 7], got %s %s" % (rows_dev.dtype, tuple(rows_dev.shape)))
    dev = rows_dev.device
    rows_dev = rows_dev.contiguous()
    R, N = int(rows_dev.shape[0]), (int(rows_dev.shape[1]) - 7) // 2
    if R == 0:                                                             # no detection at all: one dead row
        rows_dev = torch.full((1, 2 * N + 7), float("-inf"), dtype=torch.float32, device=dev)
        R = 1
    S = min(R, il.MAX_MASKS)                                              # slots drawn and merged
    # one buffer for everything that comes back: n, per row src / label / conf / text index / group, per slot counts /
    # value / visible / box / score / depth, the flag bytes, the vertices
    o_src, o_lab, o_conf, o_text, o_grp = 4, 4 + R, 4 + 2 * R, 4 + 3 * R, 4 + 4 * R
    o_cnt = 4 + 5 * R
    o_val, o_vis, o_box, o_score, o_depth = o_cnt + S, o_cnt + 2 * S, o_cnt + 3 * S, o_cnt + 7 * S, o_cnt + 8 * S
    o_flag = o_cnt + 9 * S
    o_poly = o_flag + (R + 3) // 4
    out = torch.empty((o_poly + R * N * 2,), dtype=torch.int32, device=dev)
    poly = out[o_poly:].view(R, N, 2)
    masks = torch.empty((S, H, W), dtype=torch.uint8, device=dev)
    index = torch.empty((H, W), dtype=torch.uint8, device=dev)
    ids = torch.empty((H, W), dtype=torch.int32, device=dev)
    labels = torch.empty((H, W), dtype=torch.int32, device=dev)
    at = lambda o: ctypes.c_void_p(out.data_ptr() + 4 * o)                # noqa: E731
    L, st = _C.lib(), _C.stream()
    if family == "cityscapes":
        table = np.ascontiguousarray(cls.writer_class_table())
        _C.check(L.cp_writer_instances(_C.ptr(rows_dev), R, N, float(thresh), table.ctypes.data_as(ctypes.c_void_p),
                                       len(table), at(0), at(o_src), _C.ptr(poly), at(o_flag), at(o_lab), at(o_conf),
                                       st), "cp_writer_instances")
        _C.check(L.cp_instance_masks(_C.ptr(poly), at(o_flag), S, N, H, W, _C.ptr(masks), at(o_cnt), st),
                 "cp_instance_masks")
        multiplier, counts, min_count, prio = CITYSCAPES_MULTIPLIER, at(o_cnt), MIN_PIXELS, None
    else:
        table = np.ascontiguousarray(cls.writer_class_label_table())
        _C.check(L.cp_class_writer_instances(_C.ptr(rows_dev), R, N, float(thresh), int(cls.at_threshold),
                                             table.ctypes.data_as(ctypes.c_void_p), len(table), at(0), at(o_src),
                                             _C.ptr(poly), at(o_grp), at(o_flag), at(o_lab), at(o_conf), at(o_text),
                                             st), "cp_class_writer_instances")
        _C.check(L.cp_class_instance_masks(_C.ptr(poly), at(o_grp), at(o_flag), S, N, H, W, _C.ptr(masks), at(o_cnt),
                                           st), "cp_class_instance_masks")
        multiplier, counts, min_count, prio = il.PROTOCOLS[cls.ap_protocol].id_multiplier, None, 0, at(o_depth)
    # score and depth of every slot's source row (a dead slot has src -1: row 0 stands in, nobody reads it)
    src = out[o_src:o_src + S].clamp(min=0).long()
    out[o_score:o_score + S].view(torch.float32).copy_(rows_dev[src, 4])
    out[o_depth:o_depth + S].view(torch.float32).copy_(rows_dev[src, 2 * N + 6])
    bounds = vertex_bounds(poly[:S], MARGIN[family], (W, H))
    nbytes = L.cp_instance_map_workspace_bytes(S, H, W)
    ws = _C.workspace(nbytes, dev)
    _C.check(L.cp_instance_map(_C.ptr(masks), S, H, W, at(o_flag), 1, counts, min_count, at(o_lab), prio,
                               _C.ptr(bounds), multiplier, 0, _C.ptr(index), _C.ptr(ids), _C.ptr(labels), at(o_val),
                               at(o_vis), at(o_box), _C.ptr(ws), nbytes, st), "cp_instance_map")
    host = out.cpu().numpy()                                              # the one copy
    n = int(host[0])
    if n > il.MAX_MASKS:
        raise ValueError(TOO_MANY)
    value = host[o_val:o_val + n].copy()
    tab = {"n": n, "src": host[o_src:o_src + n].copy(), "label": host[o_lab:o_lab + n].copy(),
           "conf": host[o_conf:o_conf + n].view(np.float32).copy(), "count": host[o_cnt:o_cnt + n].copy(),
           "live": value >= 0, "value": value, "visible": host[o_vis:o_vis + n].copy(),
           "box": host[o_box:o_box + 4 * n].reshape(n, 4).copy(),
           "score": host[o_score:o_score + n].view(np.float32).copy(),
           "poly": host[o_poly:o_poly + n * N * 2].reshape(n, N, 2).copy()}
    if family == "class":
        tab["text_index"] = host[o_text:o_text + n].copy()
    names = {int(cls.label_to_id[c]): c for c in cls.class_name[1:] if int(cls.label_to_id[c]) >= 0}
    return InstanceMaps(family, (W, H), index, ids, labels, masks, tab, names, multiplier)


def image_stem(name):
    """`<stem>` of the files: the image file's base name without its extension."""
    return os.path.splitext(os.path.basename(str(name)))[0]


def instance_entry(maps, k):
    """What <stem>.json says about slot k."""
    t = maps.table
    return {"label_id": int(t["label"][k]), "class_name": maps.names.get(int(t["label"][k]), ""),
            "score": float(t["score"][k]), "confidence": float(t["conf"][k]), "value": int(t["value"][k]),
            "visible": int(t["visible"][k]), "box": [int(v) for v in t["box"][k]], "source_row": int(t["src"][k]),
            "polygon": [[int(x), int(y)] for x, y in t["poly"][k]]}


def save_ids(maps, out_dir, stem, device_png=False):
    """--save_ids: <stem>_instanceIds.png (16 bit), <stem>_labelIds.png (8 bit) and <stem>.json (one entry per live
    instance) in out_dir; device_png: the two images compressed on the device (utils/png.py).  Returns the three
    paths."""
    from ..datasets.ground_truth import write_id_png
    os.makedirs(out_dir, exist_ok=True)
    paths = [os.path.join(out_dir, stem + "_instanceIds.png"), os.path.join(out_dir, stem + "_labelIds.png"),
             os.path.join(out_dir, stem + ".json")]
    write_id_png(paths[0], maps.ids, 16, device_png=device_png)
    write_id_png(paths[1], maps.labels, 8, device_png=device_png)
    t = maps.table
    entries = [instance_entry(maps, k) for k in range(t["n"]) if t["live"][k]]
    with open(paths[2], "w") as f:
        json.dump({"width": maps.canvas[0], "height": maps.canvas[1], "multiplier": int(maps.multiplier),
                   "instances": entries}, f)
    return paths


def save_masks(maps, out_dir, stem, device_png=False):
    """--save_masks: <stem>.txt with one line `masks/<stem>_<k>.png <label id> <confidence>` per live instance and the
    masks as 8-bit PNG files, the Cityscapes result layout (evaluation.instance_level.evaluate_result_dir reads it)
    for every data set.  device_png: the masks are compressed on the device within the polygons' bounds, one call for
    all live slots (utils/png.py), and only the compressed bytes come back.  Returns the text file's path."""
    from PIL import Image
    os.makedirs(os.path.join(out_dir, "masks"), exist_ok=True)
    slots = maps.written()
    masks = maps.masks.cpu().numpy() if slots and not device_png else None
    path = os.path.join(out_dir, stem + ".txt")
    names = []
    with open(path, "w") as f:
        for count, k in enumerate(slots):
            name = "masks/%s_%d.png" % (stem, count)
            f.write("%s %d %s\n" % (name, int(maps.table["label"][k]), maps.conf_text(k)))
            if device_png:
                names.append(os.path.join(out_dir, name))
            else:
                Image.fromarray(masks[k]).save(os.path.join(out_dir, name))
    if names:
        from ..utils import png
        bounds = vertex_bounds_host(maps.table["poly"], MARGIN[maps.family], maps.canvas)
        n = int(maps.table["n"])
        if list(slots) == list(range(n)):
            png.write(names, planes=maps.masks[:n], bounds=bounds)
        else:
            sel = torch.as_tensor(slots, dtype=torch.long, device=maps.masks.device)
            png.write(names, planes=maps.masks.index_select(0, sel), bounds=bounds[slots])
    return path


def vertex_bounds_host(poly, margin, canvas):
    """vertex_bounds on the host: integer vertices numpy [n, N, 2] -> int32 [n, 4]."""
    W, H = canvas
    p = np.asarray(poly, dtype=np.int64).reshape(len(poly), -1, 2)
    if len(p) == 0:
        return np.zeros((0, 4), np.int32)
    lo, hi = p.min(1) - margin, p.max(1) + margin
    b = np.stack([lo[:, 0].clip(0, W), lo[:, 1].clip(0, H), hi[:, 0].clip(-1, W - 1), hi[:, 1].clip(-1, H - 1)], 1)
    far = np.abs(p).max((1, 2)) > EXACT_VERTEX
    b[far] = [0, 0, W - 1, H - 1]
    return np.ascontiguousarray(b, dtype=np.int32)


def rle_instances(maps):
    """The live instances in `maps.written()` order as (slot, entry): the entry of <stem>.json plus "bbox" ([x, y, w,
    h] of the mask) and "segmentation" (the COCO RLE of the writer's mask `maps.masks[k]`), encoded on the device
    within the polygons' bounds (cp_rle_encode) and read back in one copy."""
    from ..utils import rle
    slots, n = maps.written(), int(maps.table["n"])
    if not slots:
        return []
    bounds = vertex_bounds_host(maps.table["poly"], MARGIN[maps.family], maps.canvas)
    rles = rle.encode(masks=maps.masks[:n], bounds=bounds)
    out = []
    for k in slots:
        seg = {"size": rles[k]["size"], "counts": rles[k]["counts"]}
        entry = instance_entry(maps, k)
        entry["bbox"] = rle.to_bbox([seg])[0]
        entry["segmentation"] = seg
        out.append((k, entry))
    return out


def save_rle(maps, out_dir, stem):
    """--save_rle: <stem>_rle.json = {"width", "height", "instances"} in out_dir, the instances of rle_instances.
    Returns (path, [(slot, entry)])."""
    os.makedirs(out_dir, exist_ok=True)
    found = rle_instances(maps)
    path = os.path.join(out_dir, stem + "_rle.json")
    with open(path, "w") as f:
        json.dump({"width": maps.canvas[0], "height": maps.canvas[1], "instances": [e for _, e in found]}, f)
    return path, found

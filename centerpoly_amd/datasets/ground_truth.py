"""Ground-truth id images from polygon files: what the evaluators' preparation scripts make of a
`*_polygons.json` (IDDscripts/preperation/createLabels.py with json2instanceImg.py and json2labelImg.py,
cityscapesscripts/preparation/json2instanceImg.py and json2labelImg.py).

The scripts draw every kept object of a file with PIL, in file order, onto one canvas.  Here the drawing is one call
of cp_polygon_paint (csrc/paint.hip; the contract is in include/centerpoly_hip.h) and this module holds the
bookkeeping around it: the two label tables, which objects are drawn with which value (`paint_list`), and the PNG
writer.  There is no CPU fallback: without a HIP device `instance_image` / `label_image` raise."""
import sys

import numpy as np
import torch

from .. import _C

MAX_POLYGONS = 4096               # of one cp_polygon_paint call
MAX_POLYGON_VERTICES = 4096
MAX_TOTAL_VERTICES = 1 << 20
MAX_WIDTH = 16384
VERTEX_BOUND = 1 << 24            # the rasteriser's exactness bound
INSTANCE_FACTOR = 1000            # an instance is label id * 1000 + its number

# ------------------------------------------------------------------------------------------ the label tables ----
# Cityscapes (cityscapesscripts/helpers/labels.py): name, id, trainId, has instances.  An instance number counts the
# objects of the same NAME.
CITYSCAPES_ENCODINGS = ("ids", "trainIds")
CITYSCAPES_LABELS = (
    ("unlabeled", 0, 255, False), ("ego vehicle", 1, 255, False), ("rectification border", 2, 255, False),
    ("out of roi", 3, 255, False), ("static", 4, 255, False), ("dynamic", 5, 255, False), ("ground", 6, 255, False),
    ("road", 7, 0, False), ("sidewalk", 8, 1, False), ("parking", 9, 255, False), ("rail track", 10, 255, False),
    ("building", 11, 2, False), ("wall", 12, 3, False), ("fence", 13, 4, False), ("guard rail", 14, 255, False),
    ("bridge", 15, 255, False), ("tunnel", 16, 255, False), ("pole", 17, 5, False), ("polegroup", 18, 255, False),
    ("traffic light", 19, 6, False), ("traffic sign", 20, 7, False), ("vegetation", 21, 8, False),
    ("terrain", 22, 9, False), ("sky", 23, 10, False), ("person", 24, 11, True), ("rider", 25, 12, True),
    ("car", 26, 13, True), ("truck", 27, 14, True), ("bus", 28, 15, True), ("caravan", 29, 255, True),
    ("trailer", 30, 255, True), ("train", 31, 16, True), ("motorcycle", 32, 17, True), ("bicycle", 33, 18, True),
    ("license plate", -1, -1, False),
)

# IDD (IDDscripts/helpers/anue_labels.py): name, id, csId, csTrainId, level4Id, level3Id, level2Id, level1Id, has
# instances.  An instance number counts the objects of the same level3Id: caravan, trailer, train and vehicle fallback
# (level3Id 12) share one counter, person and animal (4) another.
IDD_ENCODINGS = ("id", "csId", "csTrainId", "level4Id", "level3Id", "level2Id", "level1Id")
IDD_COUNTER_COLUMN = IDD_ENCODINGS.index("level3Id")
IDD_LABELS = (
    ("road", 0, 7, 0, 0, 0, 0, 0, False), ("parking", 1, 9, 255, 1, 1, 1, 0, False),
    ("drivable fallback", 2, 255, 255, 2, 1, 1, 0, False), ("sidewalk", 3, 8, 1, 3, 2, 2, 1, False),
    ("rail track", 4, 10, 255, 3, 3, 3, 1, False), ("non-drivable fallback", 5, 255, 9, 4, 3, 3, 1, False),
    ("person", 6, 24, 11, 5, 4, 4, 2, True), ("animal", 7, 255, 255, 6, 4, 4, 2, True),
    ("rider", 8, 25, 12, 7, 5, 5, 2, True), ("motorcycle", 9, 32, 17, 8, 6, 6, 3, True),
    ("bicycle", 10, 33, 18, 9, 7, 6, 3, True), ("autorickshaw", 11, 255, 255, 10, 8, 7, 3, True),
    ("car", 12, 26, 13, 11, 9, 7, 3, True), ("truck", 13, 27, 14, 12, 10, 8, 3, True),
    ("bus", 14, 28, 15, 13, 11, 8, 3, True), ("caravan", 15, 29, 255, 14, 12, 8, 3, True),
    ("trailer", 16, 30, 255, 15, 12, 8, 3, True), ("train", 17, 31, 16, 15, 12, 8, 3, True),
    ("vehicle fallback", 18, 355, 255, 15, 12, 8, 3, True), ("curb", 19, 255, 255, 16, 13, 9, 4, False),
    ("wall", 20, 12, 3, 17, 14, 9, 4, False), ("fence", 21, 13, 4, 18, 15, 10, 4, False),
    ("guard rail", 22, 14, 255, 19, 16, 10, 4, False), ("billboard", 23, 255, 255, 20, 17, 11, 4, False),
    ("traffic sign", 24, 20, 7, 21, 18, 11, 4, False), ("traffic light", 25, 19, 6, 22, 19, 11, 4, False),
    ("pole", 26, 17, 5, 23, 20, 12, 4, False), ("polegroup", 27, 18, 255, 23, 20, 12, 4, False),
    ("obs-str-bar-fallback", 28, 255, 255, 24, 21, 12, 4, False), ("building", 29, 11, 2, 25, 22, 13, 5, False),
    ("bridge", 30, 15, 255, 26, 23, 13, 5, False), ("tunnel", 31, 16, 255, 26, 23, 13, 5, False),
    ("vegetation", 32, 21, 8, 27, 24, 14, 5, False), ("sky", 33, 23, 10, 28, 25, 15, 6, False),
    ("fallback background", 34, 255, 255, 29, 25, 15, 6, False), ("unlabeled", 35, 0, 255, 255, 255, 255, 255, False),
    ("ego vehicle", 36, 1, 255, 255, 255, 255, 255, False),
    ("rectification border", 37, 2, 255, 255, 255, 255, 255, False),
    ("out of roi", 38, 3, 255, 255, 255, 255, 255, False), ("license plate", 39, 255, 255, 255, 255, 255, 255, False),
)

TABLES = {"cityscapes": (CITYSCAPES_LABELS, CITYSCAPES_ENCODINGS), "IDD": (IDD_LABELS, IDD_ENCODINGS)}
DEFAULT_ENCODING = {"cityscapes": "ids", "IDD": "id"}
BACKGROUND_LABEL = "unlabeled"


def label_table(dataset):
    """{name: (ids of every encoding in the order of the data set's ENCODINGS, has instances)}."""
    rows, encodings = TABLES[dataset]
    return {r[0]: (tuple(r[1:1 + len(encodings)]), bool(r[-1])) for r in rows}


def _encoding_column(dataset, encoding):
    encodings = TABLES[dataset][1]
    if encoding not in encodings:
        raise ValueError("unknown encoding %r for %s: one of %s" % (encoding, dataset, ", ".join(encodings)))
    return encodings.index(encoding)


def _vertices(polygon, what, k, label):
    pts = np.asarray(polygon, np.float64).reshape(-1, 2) if len(polygon) else np.zeros((0, 2))
    if len(pts) > MAX_POLYGON_VERTICES:
        raise ValueError("%s: object %d (%s) has %d vertices; at most %d are supported"
                         % (what, k, label, len(pts), MAX_POLYGON_VERTICES))
    if not np.all(np.abs(pts) <= VERTEX_BOUND):
        raise ValueError("%s: object %d (%s) has a vertex beyond +-2^24" % (what, k, label))
    return np.trunc(pts).astype(np.int32)                     # PIL takes int() of a float coordinate


def paint_list(objects, dataset, kind, encoding=None, what="the file", unknown=None):
    """What the scripts draw for one polygon file, in their order: (polygons, values, background).
    objects: the file's `objects` list, in file order; kind: "instance" or "label"; encoding: one of the data set's
    ENCODINGS (default: ids / id).  polygons: int32 [m, 2] arrays, the vertices truncated towards zero; values: the
    fill of each.  An unknown IDD label is reported on stderr (and appended to `unknown` when given) and skipped; an
    unknown Cityscapes label is an error."""
    if dataset not in TABLES:
        raise ValueError("unknown data set %r: cityscapes or IDD" % (dataset,))
    if kind not in ("instance", "label"):
        raise ValueError("kind must be instance or label, got %r" % (kind,))
    encoding = DEFAULT_ENCODING[dataset] if encoding is None else encoding
    col = _encoding_column(dataset, encoding)
    table = label_table(dataset)
    idd = dataset == "IDD"
    background = table[BACKGROUND_LABEL][0][col]
    # json2instanceImg.py (IDD) :139-142: one counter per level3Id; (Cityscapes) :118-121: one per name
    counters = {}
    polygons, values = [], []
    for k, o in enumerate(objects):
        label, polygon = str(o["label"]), o["polygon"]
        if o.get("deleted", 0):                               # IDD :152 / :101, Cityscapes :129 / :93
            continue
        if idd and len(polygon) < (2 if kind == "instance" else 3):   # IDD instance :152, label :101
            continue
        is_group = False
        if label not in table and label.endswith("group"):    # IDD :159-161 / :106-107, Cityscapes :136-138 / :98-99
            label, is_group = label[:-len("group")], True
        if label not in table:
            if not idd:                                       # Cityscapes :140-141 / :101-102
                raise ValueError("%s: object %d has the label %r, which Cityscapes does not know" % (what, k, label))
            print("%s: label %r not known, object %d skipped" % (what, label, k), file=sys.stderr)   # IDD :163-166
            if unknown is not None:
                unknown.append(label)
            continue
        ids, has_instances = table[label]
        if kind == "instance":
            value = ids[col]
            # IDD :189-191; Cityscapes :154-156, where a value of 255 stays the class value
            if has_instances and not is_group and (idd or value != 255):
                key = ids[IDD_COUNTER_COLUMN] if idd else label
                value = value * INSTANCE_FACTOR + counters.get(key, 0)
                counters[key] = counters.get(key, 0) + 1
            if value < 0:                                     # IDD :194, Cityscapes :159: after the counter moved
                continue
        else:
            if ids[0] < 0:                                    # the regular id decides, whatever the encoding:
                continue                                      # IDD label :115, Cityscapes label :105
            value = ids[col]
        pts = _vertices(polygon, what, k, label)
        if len(pts) < 2:
            raise ValueError("%s: object %d (%s) has %d vertices; a polygon needs two" % (what, k, label, len(pts)))
        polygons.append(pts)
        values.append(int(value))
    return polygons, values, int(background)


def paint(polygons, values, background, canvas, device=None):
    """cp_polygon_paint: the polygons drawn in order onto a canvas (width, height) of `background`.  Returns the device
    int32 tensor [H, W].  The vertices and the values go up in one copy each."""
    W, H = int(canvas[0]), int(canvas[1])
    if W < 1 or H < 1 or W * H >= 1 << 31 or W > MAX_WIDTH:
        raise ValueError("canvas %s: width 1 .. %d, a positive height and width * height < 2^31 are supported"
                         % (tuple(canvas), MAX_WIDTH))
    n = len(polygons)
    if n != len(values):
        raise ValueError("%d polygons and %d values" % (n, len(values)))
    if n > MAX_POLYGONS:
        raise ValueError("%d polygons in one image, at most %d are supported" % (n, MAX_POLYGONS))
    first = np.zeros((n + 1,), np.int64)
    for i, p in enumerate(polygons):
        p = np.asarray(p)
        if p.ndim != 2 or p.shape[1] != 2 or not 2 <= len(p) <= MAX_POLYGON_VERTICES:
            raise ValueError("polygon %d has the shape %s; [2 .. %d, 2] is supported" % (i, p.shape, MAX_POLYGON_VERTICES))
        first[i + 1] = first[i] + len(p)
    T = int(first[n])
    if T > MAX_TOTAL_VERTICES:
        raise ValueError("%d vertices in one image, at most %d are supported" % (T, MAX_TOTAL_VERTICES))
    dev = torch.device("cuda") if device is None else torch.device(device)
    if dev.type != "cuda":
        raise _C.NativeError("centerpoly_amd ops need a HIP device (got %s); there is no CPU fallback" % dev)
    L = _C.lib()
    image = torch.empty((H, W), dtype=torch.int32, device=dev)
    if n == 0:
        _C.check(L.cp_polygon_paint(None, None, None, 0, int(background), H, W, _C.ptr(image), None, 0, _C.stream()),
                 "cp_polygon_paint")
        return image
    xy = torch.from_numpy(np.concatenate([np.asarray(p, np.int32) for p in polygons])).to(dev)
    val = torch.from_numpy(np.asarray(values, np.int32)).to(dev)
    first_arr = (_C.c_int32 * (n + 1))(*[int(f) for f in first])
    ws_bytes = L.cp_polygon_paint_workspace_bytes(n, T)
    ws = _C.workspace(ws_bytes, dev)
    _C.check(L.cp_polygon_paint(_C.ptr(xy), first_arr, _C.ptr(val), n, int(background), H, W, _C.ptr(image), _C.ptr(ws),
                                ws_bytes, _C.stream()), "cp_polygon_paint")
    return image


def instance_image(objects, canvas, dataset, encoding=None, device=None, what="the file"):
    """The instance image of one polygon file (createInstanceImage) as a device int32 tensor [H, W]."""
    polygons, values, background = paint_list(objects, dataset, "instance", encoding, what)
    return paint(polygons, values, background, canvas, device)


def label_image(objects, canvas, dataset, encoding=None, device=None, what="the file"):
    """The label image of one polygon file (createLabelImage, no colours) as a device int32 tensor [H, W]."""
    polygons, values, background = paint_list(objects, dataset, "label", encoding, what)
    return paint(polygons, values, background, canvas, device)


def id_array(path, image, bits):
    """The uint16 (bits 16) or uint8 (bits 8) host array of an id image; a value that does not fit is a ValueError
    that names the file and the value (the scripts let PIL wrap it around; that is not imitated)."""
    if bits not in (8, 16):
        raise ValueError("an id image has 8 or 16 bits, not %r" % (bits,))
    arr = image.cpu().numpy() if isinstance(image, torch.Tensor) else np.asarray(image)
    if arr.ndim != 2 or arr.dtype.kind not in "iu":
        raise ValueError("%s: an id image is a 2-D integer array, got %s %s" % (path, arr.shape, arr.dtype))
    if arr.size:
        lo, hi = int(arr.min()), int(arr.max())
        bad = lo if lo < 0 else hi if hi >= 1 << bits else None
        if bad is not None:
            raise ValueError("%s: the value %d does not fit a %d-bit image" % (path, bad, bits))
    return np.ascontiguousarray(arr.astype(np.uint16 if bits == 16 else np.uint8))


def write_id_png(path, image, bits=16, device_png=False):
    """A 16-bit (mode I;16) or 8-bit (mode L) PNG of an id image: a device or host tensor or an array.  device_png: a
    device tensor is compressed on the device (utils/png.py) and only the file's bytes come back; the same ValueError
    for a value that does not fit."""
    if device_png and isinstance(image, torch.Tensor) and image.is_cuda:
        from ..utils import png
        if image.dim() != 2 or image.dtype not in (torch.int32, torch.int16, torch.uint8, torch.int64):
            raise ValueError("%s: an id image is a 2-D integer array, got %s %s" % (path, tuple(image.shape), image.dtype))
        if bits not in (8, 16):
            raise ValueError("an id image has 8 or 16 bits, not %r" % (bits,))
        if image.dtype == torch.int64 and image.numel():
            lo, hi = int(image.min()), int(image.max())                   # (int32 below would wrap these around)
            bad = lo if lo < 0 else hi if hi >= 1 << bits else None
            if bad is not None:
                raise ValueError("%s: the value %d does not fit a %d-bit image" % (path, bad, bits))
        png.write([path], images=image.to(torch.int32), bits=bits)
        return
    from PIL import Image
    Image.fromarray(id_array(path, image, bits)).save(path, format="PNG")

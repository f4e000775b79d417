"""The inputs of the annotation tests (tests/test_annotations.py, gen_annotations_golden.py): id images and
ground-truth polygon lists, built from seeds and plain geometry -- the smallest shapes at which the recipe can go
wrong.  Images up to about 100 x 160 are also stored in the fixture; the larger ones are rebuilt from here."""
import math

import numpy as np

from centerpoly_amd import synth

KITTI_LABELS = [24, 25, 26, 27, 28, 31, 32, 33]                # person .. bicycle, the KITTI tool's id_to_label
CITYSCAPES_HAVE = ["person", "rider", "car", "truck", "bus", "train", "motorcycle", "bicycle", "pole", "traffic sign",
                   "traffic light"]
CITYSCAPES_CATS = CITYSCAPES_HAVE[:8]
IDD_HAVE = ["person", "rider", "motorcycle", "bicycle", "autorickshaw", "car", "truck", "bus", "vehicle fallback"]
BOX_POINT_COUNTS = (4, 16, 24, 40, 64)
SIDES = 98                                                      # 0 .. 97


def v(label, k):
    return label * 256 + k


# --------------------------------------------------------------------------------------------------- boxes ----
def point_boxes():
    """Integer boxes with x sides 0 .. 97 (the y side runs through the same values in another order) and their
    float cousins, as an IDD file has them."""
    ints = np.array([[3, 5, 3 + s, 5 + (s * 37) % SIDES] for s in range(SIDES)], np.float64)
    floats = np.array([[1.25 - (s % 3), 2.5 - (s % 2) * 4, 1.25 - (s % 3) + s * 0.75, 2.5 - (s % 2) * 4 + ((s * 37) % SIDES) * 0.625]
                       for s in range(SIDES)], np.float64)
    return ints, floats


POINT_CANVAS = (112, 108)                                       # (W, H): every start point of point_boxes lies inside


# ------------------------------------------------------------------------------------------------ id images ----
def ids_one():
    return np.full((1, 1), v(26, 0), np.uint16)


def ids_shapes():
    """37 x 53: see the issue's list; raster order differs from value order."""
    H, W = 37, 53
    a = np.zeros((H, W), np.uint16)
    yy, xx = np.mgrid[:H, :W]
    a[0, :] = a[H - 1, :] = v(24, 9)                            # touches all four borders (a frame)
    a[:, 0] = a[:, W - 1] = v(24, 9)
    a[((xx - 12) / 9.0) ** 2 + ((yy - 10) / 6.0) ** 2 <= 1.0] = v(33, 1)     # ellipse, the largest value first in raster
    a[np.abs(xx - 40) + np.abs(yy - 9) <= 6] = v(26, 0)        # diamond
    a[20, 3:25] = v(26, 1)                                      # bar one pixel high
    a[24:35, 28:41] = v(28, 2)                                  # C-shape: its centre pixel is empty
    a[26:33, 31:41] = 0
    a[22:25, 44:48] = v(25, 0)                                  # two disconnected parts
    a[31:34, 49:52] = v(25, 0)
    a[24:30, 4:10] = v(29, 1)                                   # caravan: between kept labels, takes no pseudo-depth
    a[24:30, 12:18] = v(31, 0)
    a[31:35, 4:8] = v(7, 3)                                     # road
    a[31:35, 10:14] = 255                                       # the tool's own "255"
    a[31:35, 16:20] = v(255, 255)                               # label 255
    a[28:30, 33:35] = v(27, 5)                                  # inside the C, near its centre but not on it
    return a


def ids_many(n):
    """64 x 96 with n instances of 5 x 5 pixels."""
    a = np.zeros((64, 96), np.uint16)
    for k in range(n):
        r, c = divmod(k, 16)
        a[1 + 6 * r:6 + 6 * r, 6 * c:5 + 6 * c] = v(KITTI_LABELS[k % 8], (k * 5) % 131)
    assert len(np.unique(a)) == n + 1
    return a


def ids_wide():
    """70 x 300: rays of more than 64 and more than 128 steps before they hit, and rays that never hit."""
    a = np.zeros((70, 300), np.uint16)
    a[30:41, 2:9] = a[30:41, 290:298] = v(26, 4)
    a[34:37, 148:152] = v(26, 4)
    a[5:65, 100:102] = v(24, 1)                                 # a thin wall another object's rays pass through
    a[2:4, 20:280] = v(27, 0)                                   # a long bar and a far-away foot: a hollow box
    a[66:68, 150:154] = v(27, 0)
    return a


def ids_kitti():
    """375 x 1242 (odd width), about 30 instances of blobs from seeded ellipses."""
    H, W = 375, 1242
    a = np.zeros((H, W), np.uint16)
    yy, xx = np.mgrid[:H, :W]
    p = synth.integers("annot/kitti", (30, 5), 0, 1 << 16)
    for k in range(30):
        cx, cy = int(p[k, 0]) % W, 120 + int(p[k, 1]) % 230
        rx, ry = 6 + int(p[k, 2]) % 90, 4 + int(p[k, 3]) % 40
        a[((xx - cx) / float(rx)) ** 2 + ((yy - cy) / float(ry)) ** 2 <= 1.0] = v(KITTI_LABELS[int(p[k, 4]) % 8], k)
    return a


ID_CASES = {"one": ids_one, "shapes": ids_shapes, "many128": lambda: ids_many(128), "many129": lambda: ids_many(129),
            "wide": ids_wide, "kitti": ids_kitti}
ID_STORED = ("one", "shapes", "many128", "many129", "wide")     # in the fixture; "kitti" is rebuilt
ID_COUNTS = {"one": (4, 16), "shapes": (4, 16, 24, 64), "many128": (8,), "many129": (8,), "wide": (16, 40),
             "kitti": (32,)}


def kitti_dir_image(i):
    """Image i (from 0) of the split-rule directories: 6 x 9, one or two objects; every seventh has none kept."""
    a = np.zeros((6, 9), np.uint16)
    if i % 7 == 3:
        a[1:3, 1:4] = v(7, 1)
        return a
    a[1:4, 1 + i % 3:5 + i % 3] = v(26, i % 5)
    if i % 2:
        a[4:6, 5:9] = v(24, 1 + i % 4)
    return a


# ------------------------------------------------------------------------------------------------- polygons ----
def star(cx, cy, r_out, r_in, n):
    return [[int(round(cx + (r_out if k % 2 == 0 else r_in) * math.cos(2 * math.pi * k / n))),
             int(round(cy + (r_out if k % 2 == 0 else r_in) * math.sin(2 * math.pi * k / n)))] for k in range(n)]


def noisy_circle(stream, cx, cy, r, n, amp):
    d = synth.uniform(stream, (n,), -amp, amp, dtype=np.float64)
    return [[int(round(cx + (r + d[k]) * math.cos(2 * math.pi * k / n))),
             int(round(cy + (r + d[k]) * math.sin(2 * math.pi * k / n)))] for k in range(n)]


def _obj(label, polygon):
    return {"label": label, "polygon": polygon}


def polys_small():
    """53 x 37, Cityscapes labels."""
    return [
        _obj("road", [[0, 30], [52, 30], [52, 36], [0, 36]]),
        _obj("car", [[4, 3], [16, 9], [7, 15]]),                                             # 3 vertices
        _obj("pole", [[20, 2], [22, 2], [22, 30], [20, 30]]),                                # takes a depth, dropped
        _obj("person", star(34, 12, 11, 5, 64)),                                             # 64
        _obj("cargroup", [[1, 1], [9, 1], [9, 9], [1, 9]]),                                  # skipped, no depth
        _obj("rider", noisy_circle("annot/c65", 14, 25, 8, 65, 2.0)),                        # 65
        _obj("truck", [[26, 20], [40, 34], [40, 20], [26, 34]]),                             # self-touching bow tie
        _obj("bus", [[42, 4], [42, 4], [50, 4], [50, 4], [50, 12], [46, 12], [46, 12], [42, 12]]),   # repeated vertices
        _obj("train", [[30, 30], [30, 30], [30, 30], [30, 30]]),                             # one point
        _obj("motorcycle", [[44, 16], [45, 16], [45, 33], [44, 33]]),                        # 2-pixel sliver: empty
        _obj("traffic sign", [[2, 17], [5, 17], [5, 21], [2, 21]]),
        _obj("bicycle", [[-3, 12], [20, -3], [55, 18], [30, 38]]),                           # beyond every border
        _obj("sky", [[0, 0], [52, 0], [52, 5], [0, 5]]),
    ]


def polys_idd():
    """53 x 37, IDD labels, float vertices with negatives."""
    return [
        _obj("autorickshaw", [[3.7, 2.2], [25.5, 4.9], [30.25, 19.5], [12.5, 27.75], [-2.6, 14.4]]),
        _obj("road", [[0.0, 30.0], [52.0, 30.0], [52.0, 36.0]]),
        _obj("vehicle fallback", [[33.9, -1.5], [51.2, 6.7], [54.8, 30.1], [40.4, 35.99], [35.5, 20.5]]),
        _obj("person", [[20.5, 28.5], [28.5, 28.5], [28.5, 35.5], [20.5, 35.5]]),
        _obj("car", [[-0.9, -0.9], [6.2, -0.4], [5.5, 5.5], [-0.2, 6.9]]),
    ]


def polys_none():
    return [_obj("road", [[0, 20], [52, 20], [52, 36], [0, 36]]), _obj("sky", [[0, 0], [52, 0], [52, 5]])]


def polys_long():
    """160 x 100: a star of 700 vertices and a noisy circle of 701."""
    return [_obj("car", star(55, 50, 46, 30, 700)), _obj("person", noisy_circle("annot/c701", 118, 48, 34, 701, 4.0))]


def polys_full():
    """2048 x 1024 (the Cityscapes canvas): one object."""
    return [_obj("car", [[int(p[0] * 12 + 300), int(p[1] * 9 + 80)] for p in star(60, 50, 50, 28, 40)])]


POLY_CASES = {"small": (polys_small, (53, 37), CITYSCAPES_HAVE), "idd": (polys_idd, (53, 37), IDD_HAVE),
              "none": (polys_none, (53, 37), CITYSCAPES_HAVE), "long": (polys_long, (160, 100), CITYSCAPES_HAVE),
              "full": (polys_full, (2048, 1024), CITYSCAPES_HAVE), "small_full": (polys_small, (2048, 1024), CITYSCAPES_HAVE)}
POLY_COUNTS = {"small": (4, 16, 24), "idd": (16, 40), "none": (16,), "long": (32, 64), "full": (8, 32), "small_full": (8,)}

"""Inputs of the ground-truth image tests (tests/test_ground_truth.py) and of gen_ground_truth_golden.py: polygon
files as the data sets ship them, `{"imgWidth", "imgHeight", "objects": [{"label", "polygon", "deleted"?}]}`, built
from integers only (a fixed linear congruential sequence, no library's random numbers).

CASES: name -> (dataset, kind, encoding, (W, H), builder of the object list).  The geometry cases use the IDD instance
image (it alone draws polygons of two vertices); the bookkeeping cases run every encoding of both data sets once."""

IDD_ENCODINGS = ("id", "csId", "csTrainId", "level4Id", "level3Id", "level2Id", "level1Id")
CITYSCAPES_ENCODINGS = ("ids", "trainIds")


class Lcg(object):
    def __init__(self, seed):
        self.s = seed

    def next(self, n):
        """An integer in 0 .. n-1."""
        self.s = (self.s * 1103515245 + 12345) % (1 << 31)
        return (self.s >> 8) % n


def obj(label, polygon, **extra):
    o = {"label": label, "polygon": [list(p) for p in polygon]}
    o.update(extra)
    return o


def rect(x0, y0, x1, y1):
    return [(x0, y0), (x1, y0), (x1, y1), (x0, y1)]


def star(cx, cy, n, rmin, rmax, seed):
    """n vertices around (cx, cy) on an integer "circle" of 8 directions stretched to n steps, radius from the
    sequence: a ragged outline with many crossings per row."""
    g = Lcg(seed)
    # a coarse integer sine table, quarter wave of 16 steps, scaled by 1024
    quarter = [0, 100, 200, 297, 392, 483, 569, 650, 724, 792, 851, 903, 946, 980, 1004, 1019, 1024]

    def sin64(k):
        k %= 64
        if k < 16:
            return quarter[k]
        if k < 32:
            return quarter[32 - k]
        if k < 48:
            return -quarter[k - 32]
        return -quarter[64 - k]
    pts = []
    for i in range(n):
        a = (i * 64) // n
        r = rmin + g.next(rmax - rmin + 1)
        pts.append((cx + (r * sin64(a + 16)) // 1024, cy + (r * sin64(a)) // 1024))
    return pts


# ------------------------------------------------------------------------------------------------ geometry ----
def overlap():
    """Later over earlier, partly and wholly; nested three deep; equal values overlapping."""
    return [obj("road", rect(2, 2, 60, 44)),
            obj("car", rect(5, 5, 30, 25)),
            obj("car", rect(20, 15, 45, 35)),                      # partly over the first car
            obj("person", [(8, 8), (28, 10), (18, 24)]),
            obj("truck", rect(4, 4, 32, 27)),                      # wholly over the first car and the person
            obj("sidewalk", rect(34, 3, 61, 30)),
            obj("bus", rect(38, 6, 58, 26)),                       # nested three deep: road > sidewalk > bus > rider
            obj("rider", [(42, 10), (54, 10), (54, 22), (48, 16), (42, 22)]),
            obj("sky", rect(0, 36, 30, 47)), obj("sky", [(20, 30), (40, 40), (20, 47), (10, 40)]),   # equal values
            obj("building", [(50, 30), (63, 47), (40, 47)])]


def two_vertex():
    """Polygons of two vertices, flat, upright, sloped both ways and a point, among larger ones."""
    return [obj("road", rect(0, 0, 36, 52)),
            obj("car", [(3, 4), (30, 4)]),                         # horizontal
            obj("car", [(5, 8), (5, 40)]),                         # vertical
            obj("person", [(8, 10), (30, 45)]),                    # sloped, steep
            obj("person", [(10, 48), (34, 40)]),                   # sloped, shallow, going up
            obj("bus", [(20, 20), (20, 20)]),                      # one point twice
            obj("truck", rect(12, 12, 26, 30)),                    # over the steep line
            obj("rider", [(0, 30), (36, 31)]),                     # almost flat, over the truck
            obj("bicycle", [(33, 2), (14, 50)]),
            obj("motorcycle", [(-5, 45), (50, 52)])]               # both ends off the canvas


def floats():
    """Float and negative vertices; polygons partly and wholly off the canvas on every side."""
    return [obj("road", [(-10.5, -3.25), (50.75, -8.5), (45.5, 60.25), (-4.75, 55.5)]),
            obj("car", [(2.9, 3.9), (20.1, 4.5), (18.7, 20.2), (3.3, 18.8)]),
            obj("car", [(-8.9, 10.5), (6.5, 12.5), (4.5, 30.5), (-9.5, 28.5)]),        # over the left edge
            obj("truck", [(30.5, 5.5), (45.5, 8.5), (44.5, 25.5), (28.5, 22.5)]),      # over the right edge
            obj("bus", [(10.5, -7.5), (25.5, -6.5), (22.5, 6.5), (12.5, 5.99)]),       # over the top
            obj("person", [(8.2, 45.7), (20.9, 44.1), (22.4, 60.6), (6.6, 58.3)]),     # over the bottom
            obj("rider", [(-30, 5), (-20, 5), (-20, 25), (-30, 25)]),                  # wholly left
            obj("rider", [(40, 5), (60, 5), (60, 25), (40, 25)]),                      # wholly right
            obj("bicycle", [(5, -20), (25, -20), (15, -2)]),                           # wholly above
            obj("bicycle", [(5, 53), (25, 53), (15, 70)]),                             # wholly below (from the last row + 1)
            obj("motorcycle", [(-0.5, -0.5), (-0.99, 30.5), (12.5, 40.99), (36.99, 52.99), (36.01, -0.99)]),
            obj("autorickshaw", [(15.5, 22.5), (30.5, 26.5), (20.5, 38.5)])]


def long():
    """A polygon of 300 vertices (more than one pass of the workgroup's lanes) and one of 4096."""
    return [obj("road", rect(0, 20, 95, 63)),
            obj("car", star(30, 30, 300, 6, 28, 7)),
            obj("vegetation", star(60, 34, 4096, 4, 33, 11)),
            obj("person", star(48, 32, 70, 3, 12, 5))]


def many():
    """600 small polygons of 3 to 5 vertices and a few of two."""
    g = Lcg(99)
    labels = ("car", "person", "road", "truck", "sky", "rider", "bus", "pole", "bicycle", "wall")
    out = []
    for i in range(600):
        cx, cy = g.next(70) - 3, g.next(54) - 3
        n = 2 if i % 50 == 49 else 3 + g.next(3)
        out.append(obj(labels[g.next(len(labels))], [(cx + g.next(13) - 6, cy + g.next(13) - 6) for _ in range(n)]))
    return out


def none():
    return []


def one():
    return [obj("car", [(0, 5), (0, 30), (0, 12)])]


def pixel():
    return [obj("road", rect(-2, -2, 3, 3)), obj("car", [(0, 0), (0, 0)])]


def column():
    """A canvas one pixel wide."""
    return [obj("road", rect(0, 2, 0, 35)), obj("car", [(0, 10), (0, 20)]), obj("bus", [(-3, 15), (4, 18), (-2, 30)]),
            obj("person", [(0, 38), (0, 39), (0, 38)])]


def row():
    """A canvas one pixel high."""
    return [obj("road", rect(2, 0, 35, 0)), obj("car", [(10, 0), (20, 0)]), obj("bus", [(15, -3), (18, 4), (30, -2)]),
            obj("person", [(38, 0), (39, 0), (38, 0)])]


def wide():
    """Three rows of 16384 pixels: the widest row image."""
    return [obj("road", rect(-5, 0, 16390, 2)),
            obj("car", rect(100, 0, 9000, 1)),
            obj("truck", [(16383, 0), (8000, 2), (12000, 0)]),
            obj("person", [(0, 1), (16383, 1)]),
            obj("bus", [(3, 0), (16000, 2)]),
            obj("sky", rect(16380, 1, 16500, 5)),
            obj("rider", star(5000, 1, 300, 1, 900, 3))]


# --------------------------------------------------------------------------------------------- bookkeeping ----
def books_idd():
    """Deleted, `...group`, unknown, two vertices, shared counter (caravan, train, vehicle fallback: level3Id 12)."""
    return [obj("road", rect(0, 0, 36, 52)),
            obj("car", rect(2, 2, 12, 12)),
            obj("car", rect(8, 8, 18, 18), deleted=1),
            obj("cargroup", rect(14, 2, 24, 12)),
            obj("car", rect(20, 8, 30, 18)),                       # the second counted car
            obj("spaceship", rect(0, 0, 36, 52)),                  # unknown: reported and skipped
            obj("spaceshipgroup", rect(0, 0, 36, 52)),
            obj("caravan", rect(2, 22, 12, 32)),
            obj("train", rect(8, 26, 20, 36)),
            obj("vehicle fallback", rect(16, 30, 28, 40)),
            obj("trailer", rect(24, 34, 35, 44), deleted=0),
            obj("person", [(3, 40), (30, 50)]),                    # two vertices: instance image only
            obj("animal", rect(1, 44, 9, 51)),
            obj("polegroup", rect(30, 20, 34, 50)),                # a known label that ends in group
            obj("license plate", rect(4, 4, 8, 6)),
            obj("ridergroup", [(26, 2), (35, 2), (30, 9)]),
            obj("sky", [(31, 11)]),                                # one vertex: skipped by both
            obj("out of roi", rect(0, 50, 36, 52))]


def books_idd_narrow():
    """books_idd without the label whose csId (355) does not fit the 8-bit label image."""
    return [o for o in books_idd() if o["label"] != "vehicle fallback"]


def books_cityscapes():
    """Deleted, `...group`, the negative id (license plate), trainId 255 with instances (caravan), counters per name."""
    return [obj("road", rect(0, 0, 36, 52)),
            obj("car", rect(2, 2, 12, 12)),
            obj("car", rect(8, 8, 18, 18), deleted=1),
            obj("cargroup", rect(14, 2, 24, 12)),
            obj("car", rect(20, 8, 30, 18)),
            obj("license plate", rect(4, 4, 8, 6)),
            obj("caravan", rect(2, 22, 12, 32)),
            obj("train", rect(8, 26, 20, 36)),
            obj("caravan", rect(16, 30, 28, 40)),
            obj("trailer", rect(24, 34, 35, 44), deleted=0),
            obj("person", [(3.5, 40.5), (30.5, 50.5), (10.2, 51.9)]),
            obj("persongroup", rect(1, 44, 9, 51)),
            obj("polegroup", rect(30, 20, 34, 50)),
            obj("bicyclegroup", [(26, 2), (35, 2), (30, 9)]),
            obj("ego vehicle", rect(0, 50, 36, 52))]


CASES = {
    "overlap": ("IDD", "instance", "id", (64, 48), overlap),
    "two_vertex": ("IDD", "instance", "id", (37, 53), two_vertex),
    "floats": ("IDD", "instance", "id", (37, 53), floats),
    "long": ("IDD", "instance", "id", (96, 64), long),
    "many": ("IDD", "instance", "id", (64, 48), many),
    "none": ("IDD", "instance", "id", (40, 1), none),
    "one": ("IDD", "instance", "id", (1, 40), one),
    "pixel": ("IDD", "instance", "id", (1, 1), pixel),
    "column": ("IDD", "instance", "id", (1, 40), column),
    "row": ("IDD", "instance", "id", (40, 1), row),
    "wide": ("IDD", "instance", "id", (16384, 3), wide),
    "overlap_cs": ("cityscapes", "label", "ids", (64, 48), overlap),
}
for _e in IDD_ENCODINGS:
    CASES["idd_instance_" + _e] = ("IDD", "instance", _e, (37, 53), books_idd)
    CASES["idd_label_" + _e] = ("IDD", "label", _e, (37, 53), books_idd_narrow if _e == "csId" else books_idd)
for _e in CITYSCAPES_ENCODINGS:
    CASES["cs_instance_" + _e] = ("cityscapes", "instance", _e, (37, 53), books_cityscapes)
    CASES["cs_label_" + _e] = ("cityscapes", "label", _e, (37, 53), books_cityscapes)

# the frames of the driver test: (city, frame stem, case whose objects and canvas it holds)
IDD_FRAMES = (("7", "000010", "overlap"), ("7", "000020", "none"), ("9", "000005", "idd_instance_id"))
CITYSCAPES_FRAMES = (("aa", "aa_000001_000019", "overlap_cs"), ("aa", "aa_000002_000019", "cs_instance_ids"),
                     ("bb", "bb_000000_000001", "cs_label_trainIds"))


def frame_json(case):
    """The polygon file of a case as the data sets write it."""
    dataset, kind, encoding, (W, H), build = CASES[case]
    return {"imgHeight": H, "imgWidth": W, "objects": build()}

"""The synthetic disparity images and cameras of the distance-AP fixtures, and the host statement of medDist /
distConf: pure numpy, shared by tests/golden/gen_instance_ap_dist_golden.py and the tests, so that no disparity
file has to be committed.

disparity(gt_ids, index) paints, over a ground plane whose disparity grows towards the bottom row, every id of an
instance class (real instances and groups alike) around the disparity of a target distance.  The targets cycle through
the ids of an image in ascending order: near (about 20 m), between the bounds (about 70 m), beyond both (about
150 m), near with most measurements missing (stereo density about 0.3).  A seeded share of all pixels is 0, "no
measurement".  In image 0 the first instance of at least 1000 pixels has p = 2561 everywhere, which its camera
(baseline 0.25, fx 2000) puts at exactly 50 m."""
import numpy as np

CAMERAS = ((0.25, 2000.0), (0.209313, 2262.52), (0.222384, 2268.36), (0.209313, 2262.52))
KINDS = ("near", "mid", "far", "sparse")
TARGET_M = {"near": 20.0, "mid": 70.0, "far": 150.0, "sparse": 30.0}
EXACT_P = 2561
INST_LABELS = (24, 25, 26, 27, 28, 31, 32, 33)


def camera(index):
    return CAMERAS[index]


def pixel_distance(p, baseline, fx):
    """float64, in this order of operations: d = (p - 1) / 256; distance = (baseline * fx) / d."""
    d = (np.asarray(p, np.float64) - 1.0) / 256.0
    with np.errstate(divide="ignore"):
        return (np.float64(baseline) * np.float64(fx)) / d


def instance_ids(gt_ids):
    ids = np.unique(gt_ids).astype(np.int64)
    return ids[np.isin(np.where(ids < 1000, ids, ids // 1000), INST_LABELS)]


def disparity(gt_ids, index):
    """uint16 [H, W] for fixture image `index` (0 .. 3) with id image gt_ids."""
    H, W = gt_ids.shape
    rng = np.random.RandomState(4200 + index)
    baseline, fx = camera(index)
    y, x = np.mgrid[0:H, 0:W]
    p = (300 + 20 * y + (x * 7 + y * 13) % 31).astype(np.int64)              # the ground plane, nearer further down
    holes = rng.random_sample((H, W))
    noise = rng.randint(-40, 41, (H, W))
    gone = holes < 0.1
    exact_given = index != 0
    for k, inst in enumerate(instance_ids(gt_ids)):
        m = gt_ids == inst
        if not exact_given and inst >= 1000 and int(m.sum()) >= 1000:
            p[m] = EXACT_P
            gone[m] = False
            exact_given = True
            continue
        kind = KINDS[(k + index) % len(KINDS)]
        centre = int(round(256.0 * baseline * fx / TARGET_M[kind])) + 1
        p[m] = (centre + (x * 7 + y * 13) % 31 - 15 + noise)[m]
        if kind == "sparse":
            gone[m] = holes[m] < 0.7
    p = np.clip(p, 1, 65535)
    p[gone] = 0
    return p.astype(np.uint16)


def median_counts(gt_ids, disp, seg_ids):
    """What cp_segment_medians returns, by np.sort per segment: int64 [G, 4] (pixels, valid, v_lo, v_hi)."""
    out = np.zeros((len(seg_ids), 4), np.int64)
    for j, s in enumerate(seg_ids):
        if not 0 <= int(s) < 65536:
            continue
        v = disp[gt_ids == s]
        out[j, 0] = v.size
        v = np.sort(v[v != 0])
        out[j, 1] = v.size
        if v.size:
            out[j, 2], out[j, 3] = v[(v.size - 1) // 2], v[v.size // 2]
    return out


def host_distances(gt_ids, disp, seg_ids, cam):
    """float64 [G, 2] (medDist, distConf) by np.median of the pixel distances, the definition itself."""
    out = np.zeros((len(seg_ids), 2), np.float64)
    for j, s in enumerate(seg_ids):
        v = disp[gt_ids == s]
        valid = v[v != 0]
        out[j, 0] = np.median(pixel_distance(valid, *cam)) if valid.size else np.inf
        out[j, 1] = valid.size / float(max(v.size, 1))
    return out

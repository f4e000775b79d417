"""The literal host statement of --mask_nms (include/centerpoly_hip.h, "mask NMS"): numpy and math.exp, one row at a
time.  cp_polygon_overlaps and cp_merge_detections_mask (csrc/mask_nms.hip) are compared with it bit for bit.

    vertex_int, polygon      the writers' vertex int(float("%.2f" % v)) and a row's vertex list
    pil_fill                 the mask of a polygon: ImageDraw.polygon(pts, fill=1) on an H x W 'L' image (needs PIL)
    masks, overlaps          the masks of rows, their areas and the matrix of common pixels (0 across classes)
    mask_nms                 the class split, the selection with its decay, the cut: (table, counts)

tests/golden/gen_mask_nms_golden.py draws with pil_fill and records the masks' numbers in tests/golden/mask_nms.npz, so a
test on the GPU machine needs no PIL: mask_nms takes `area` and `inter` as arrays."""
import math

import numpy as np


def vertex_int(v):
    return int(float("%.2f" % v))


def polygon(row):
    n = (len(row) - 7) // 2
    return [(vertex_int(row[6 + 2 * k]), vertex_int(row[7 + 2 * k])) for k in range(n)]


def class_of(c, num_classes):
    """The class of a row as `cls == j` sees it: -1 when no j of [0, num_classes) equals it."""
    for j in range(num_classes):
        if c == j:
            return j
    return -1


def pil_fill(pts, H, W):
    from PIL import Image, ImageDraw
    im = Image.new("L", (W, H), 0)
    ImageDraw.Draw(im).polygon(pts, fill=1)
    return np.asarray(im, dtype=np.uint8) != 0


def masks(rows, num_classes, H, W, fill=pil_fill):
    """bool [R, H, W]: the mask of every row; all False for a row without a class."""
    out = np.zeros((len(rows), H, W), bool)
    for i, row in enumerate(rows):
        if class_of(row[5], num_classes) >= 0:
            out[i] = fill(polygon(row), H, W)
    return out


def overlaps_from_masks(m, classes):
    """(area int32 [R], inter int32 [R, R]) of bool masks [R, H, W] and the rows' classes (-1: none)."""
    R = len(m)
    flat = m.reshape(R, -1).astype(np.float32)                # pixel counts < 2^24: the products are exact
    inter = np.rint(flat @ flat.T).astype(np.int32)
    classes = np.asarray(classes)
    same = (classes[:, None] == classes[None, :]) & (classes[:, None] >= 0)
    inter[~same] = 0
    return np.ascontiguousarray(np.diagonal(inter)).astype(np.int32), inter


def overlaps(rows, num_classes, H, W, fill=pil_fill):
    rows = np.asarray(rows, np.float32).reshape(-1, np.shape(rows)[-1])
    classes = [class_of(r[5], num_classes) for r in rows]
    return overlaps_from_masks(masks(rows, num_classes, H, W, fill), classes)


def weight(ov, sigma, Nt, method):
    if method == 1:
        return 1.0 - ov if ov > Nt else 1.0
    if method == 2:
        return math.exp(-(ov * ov) / sigma)
    return 0.0 if ov > Nt else 1.0


def mask_nms(rows, num_classes, area, inter, max_per_image, sigma=0.5, Nt=0.5, threshold=0.001, method=2, trace=None):
    """rows float32 [S, K, ncols] -> (table float32 [n, ncols], counts int32 [1 + num_classes]).  `trace`, a list,
    receives per selection step (class, best score, second-best live score or None, whether either has decayed)."""
    rows = np.asarray(rows, np.float32)
    flat = rows.reshape(-1, rows.shape[-1])
    sigma, Nt, threshold = float(np.float32(sigma)), float(np.float32(Nt)), np.float32(threshold)
    classes = [class_of(r[5], num_classes) for r in flat]
    kept = []                                                 # (class, source row, final score)
    for j in range(num_classes):
        cand = [i for i, c in enumerate(classes) if c == j]   # position p is candidate cand[p]
        score = [np.float32(flat[i, 4]) for i in cand]
        live = [True] * len(cand)
        touched = [False] * len(cand)
        while any(live):
            best = -1
            for p in range(len(cand)):
                if live[p] and (best < 0 or score[p] > score[best]):
                    best = p
            if trace is not None:
                second = -1
                for p in range(len(cand)):
                    if live[p] and p != best and (second < 0 or score[p] > score[second]):
                        second = p
                trace.append((j, score[best], score[second] if second >= 0 else None,
                              touched[best] or (second >= 0 and touched[second])))
            if score[best] < threshold:
                break
            live[best] = False
            kept.append((j, cand[best], score[best]))
            for p in range(len(cand)):
                if not live[p]:
                    continue
                common = int(inter[cand[best], cand[p]])
                if common == 0:
                    continue
                uni = int(area[cand[best]]) + int(area[cand[p]]) - common
                ov = float(common) / float(uni) if uni else 0.0
                score[p] = np.float32(weight(ov, sigma, Nt, method) * float(score[p]))
                touched[p] = True
    scores = np.array([s for _, _, s in kept], np.float32)
    if len(scores) > max_per_image:
        kth = len(scores) - max_per_image
        thresh = np.partition(scores, kth)[kth]
        kept = [k for k in kept if k[2] >= thresh]
    table = np.zeros((len(kept), flat.shape[1]), np.float32)
    counts = np.zeros(1 + num_classes, np.int32)
    for d, (j, i, s) in enumerate(kept):
        table[d] = flat[i]
        table[d, 4] = s
        counts[1 + j] += 1
    counts[0] = len(kept)
    return table, counts

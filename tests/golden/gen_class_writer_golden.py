"""Fixtures of the KITTI / IDD result writers, drawn by PIL itself (development machine only; needs no reference
checkout: the two loops of format_and_write_to_kitti / format_and_write_to_IDD are restated here with the same PIL
calls, `ImageDraw.polygon(points, outline=0, fill=255)` on a canvas of the image's size, one to_remove_mask per
class).

Per case (tests/golden/class_writer_<name>.npz, data only): the detection rows in the layout
cp_polydet_post_process writes ([R, 2N + 7] float32: x1,y1,x2,y2,score,cls,poly,depth), threshold and mode, the
canvas, the text lines, the masks in text-line order (bit-packed), their pixel counts, the drawing order and
PIL.__version__.  The rows hold, by construction: random polygons, stars, self-crossing ones, vertices off the canvas
on every side, horizontal and vertical edges, repeated and collinear vertices, the spikes PIL's vertex rule
stretches, fractions that `%.2f` rounds up, two classes whose instances overlap, a score of exactly 0.5 and a score
exactly at the threshold.

    python tests/golden/gen_class_writer_golden.py
"""
import os

import numpy as np
import PIL
from PIL import Image, ImageDraw

HERE = os.path.dirname(os.path.abspath(__file__))
KITTI_LABELS = [24, 25, 26, 27, 28, 31, 32, 33]
IDD_LABELS = [6, 8, 9, 10, 11, 12, 13, 14, 18]
THRESH = 0.3
# name, file name of the image, labels, keeps score == thresh, width, height, vertices, rows, seed
CASES = [("kitti_a", "training/image_2/000012.png", KITTI_LABELS, False, 1242, 375, 16, 30, 1),
         ("kitti_b", "training/image_2/000347.png", KITTI_LABELS, False, 1242, 375, 16, 26, 2),
         ("idd_a", "leftImg8bit/val/201/frame0029_leftImg8bit.png", IDD_LABELS, True, 1280, 720, 16, 30, 3),
         ("idd_b", "leftImg8bit/val/305/frame1175_leftImg8bit.png", IDD_LABELS, True, 1280, 720, 16, 26, 4),
         ("odd", "training/image_2/000003.png", KITTI_LABELS, False, 37, 53, 5, 14, 5)]
SPIKES = [[(21, 11), (32, 16), (29, 16)], [(47, 8), (34, 4), (47, 7)], [(6, 10), (37, 27), (17, 15)],
          [(28, 4), (11, 14), (9, 7)], [(30, 12), (44, 9), (9, 7)]]


def polygon(rng, kind, N, W, H):
    """N float vertices of one detection."""
    cx, cy = rng.uniform(0.1 * W, 0.9 * W), rng.uniform(0.2 * H, 0.8 * H)
    r = rng.uniform(0.06, 0.3) * min(W, H) * (3 if W > 4 * H else 1.5)
    if kind == "star":
        th = np.sort(rng.uniform(0, 2 * np.pi, N))
        rad = r * np.where(np.arange(N) % 2, 0.45, 1.0) * rng.uniform(0.8, 1.2, N)
        pts = np.stack([cx + rad * np.cos(th), cy + 0.6 * rad * np.sin(th)], 1)
    elif kind == "cross":                                    # vertices in random angular order: self-crossing
        th = rng.uniform(0, 2 * np.pi, N)
        pts = np.stack([cx + r * np.cos(th), cy + 0.6 * r * np.sin(th)], 1)
    elif kind == "random":
        pts = np.stack([cx + rng.uniform(-r, r, N), cy + rng.uniform(-0.6 * r, 0.6 * r, N)], 1)
    elif kind == "off":                                      # leaves the canvas on every side
        th = np.sort(rng.uniform(0, 2 * np.pi, N))
        pts = np.stack([W / 2 + 0.75 * W * np.cos(th), H / 2 + 0.75 * H * np.sin(th)], 1) + rng.uniform(-3, 3, (N, 2))
    elif kind == "grid":                                     # flat and upright edges, repeated and collinear vertices
        th = np.sort(rng.uniform(0, 2 * np.pi, N))
        pts = np.round(np.stack([cx + r * np.cos(th), cy + 0.6 * r * np.sin(th)], 1) / 9.0) * 9.0
        pts[3] = pts[2]
        if N > 8:
            pts[7] = (pts[6] + pts[8]) / 2
    else:                                                    # "spike": a 3-vertex probe, padded with repeats
        base = np.array(SPIKES[kind], np.float64) + rng.randint(0, 3) * np.array([1.0, 0.0])
        pts = np.concatenate([base, np.repeat(base[-1:], N - 3, 0)]) if N > 3 else base
        return pts + 0.25
    pts = pts + rng.choice([0.0, 0.3, 0.994, 0.996, 0.999], (N, 2))   # %.2f rounds the last two up to the next integer
    return pts


def make_rows(labels, W, H, N, R, seed):
    rng = np.random.RandomState(seed)
    C = len(labels)
    kinds = ["star", "cross", "random", "off", "grid"]
    rows = np.zeros((R, 2 * N + 7), np.float32)
    for k in range(R):
        kind = (k - (R - len(SPIKES))) if k >= R - len(SPIKES) else kinds[k % len(kinds)]
        pts = polygon(rng, kind, N, W, H)
        rows[k, 6:6 + 2 * N] = pts.reshape(-1)
        rows[k, 0:2], rows[k, 2:4] = pts.min(0), pts.max(0)
        rows[k, 4] = rng.uniform(0.05, 1.0)
        rows[k, 5] = [2, 0, 2, 5 % C, 0][k % 5]             # two busy classes that overlap each other, one sparse
        rows[k, -1] = rng.uniform(1.0, 60.0)
    rows[1, 4] = 0.5                                          # occludes: score >= 0.5
    rows[2, 4] = np.float32(THRESH)                           # kept by IDD (>=), dropped by KITTI (>)
    rows[3, 4] = np.nextafter(np.float32(0.5), np.float32(0))  # just below 0.5: hides nothing
    rows[4, -1] = rows[9, -1]                                 # equal depths in one class: the sort is stable
    rows[6, -1] = 0.5                                         # the nearest of its class, and confident
    rows[6, 4] = 0.9
    return rows


def per_class_results(rows, C):
    """What test.py hands to run_eval: {class index from 1: rows [k, 2N + 6] without the class column}."""
    out = {}
    for c in range(C):
        out[c + 1] = np.delete(rows[rows[:, 5] == c], 5, axis=1)
    return out


def to_float(x):
    return float("{:.2f}".format(x))


def reference_writer(per_class, labels, base, w, h, at_threshold):
    """The reference's loop: (text lines, {count: mask}, drawing order as counts)."""
    thresh = np.float32(THRESH)                               # the rows are float32: a float32 comparison
    lines, masks, drawn = [], {}, []
    count = 0
    for cls_ind in per_class:
        param_list = []
        to_remove_mask = Image.new("L", (w, h), 1)
        for bbox in per_class[cls_ind]:
            if (bbox[4] >= thresh) if at_threshold else (bbox[4] > thresh):
                score = str(bbox[4])
                polygon_ = list(map(to_float, bbox[5:-1]))
                mask_path = base.replace(".png", "_" + str(count) + ".png")
                lines.append(mask_path + " " + str(labels[cls_ind - 1]) + " " + score + "\n")
                param_list.append((polygon_, count, bbox[4], bbox[-1]))
                count += 1
        for polygon_, k, score, depth in sorted(param_list, key=lambda x: x[-1]):
            poly_points = [(int(polygon_[i]), int(polygon_[i + 1])) for i in range(0, len(polygon_), 2)]
            polygon_mask = Image.new("L", (w, h), 0)
            ImageDraw.Draw(polygon_mask).polygon(poly_points, outline=0, fill=255)
            polygon_mask = Image.fromarray(np.array(polygon_mask) * np.array(to_remove_mask))
            if float(score) >= 0.5:
                ImageDraw.Draw(to_remove_mask).polygon(poly_points, outline=0, fill=0)
            masks[k] = np.array(polygon_mask)
            drawn.append(k)
    return lines, masks, drawn


def main():
    for name, file_name, labels, at_threshold, W, H, N, R, seed in CASES:
        rows = make_rows(labels, W, H, N, R, seed)
        per_class = per_class_results(rows, len(labels))
        lines, masks, drawn = reference_writer(per_class, labels, os.path.basename(file_name), W, H, at_threshold)
        stack = np.stack([masks[k] for k in range(len(lines))])
        assert set(np.unique(stack)) <= {0, 255}
        hidden = sum(1 for k in range(len(lines)) if 0 < (stack[k] > 0).sum())
        print(name, "rows", R, "lines", len(lines), "non-empty", hidden, "pixels", int((stack > 0).sum()))
        np.savez_compressed(os.path.join(HERE, "class_writer_%s.npz" % name), rows=rows, thresh=np.float64(THRESH),
                            at_threshold=np.int32(at_threshold), width=np.int32(W), height=np.int32(H),
                            labels=np.array(labels, np.int32), file_name=np.array(file_name), lines=np.array(lines),
                            packed=np.packbits(stack > 0, axis=2), counts=(stack > 0).sum((1, 2)).astype(np.int64),
                            drawn=np.array(drawn, np.int32), pil_version=np.array(PIL.__version__))


if __name__ == "__main__":
    main()

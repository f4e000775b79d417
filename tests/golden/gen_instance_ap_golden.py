"""Fixtures of the Cityscapes instance-level AP, from the reference's own evaluator (development machine only: it
imports evalInstanceLevelSemanticLabeling from the reference checkout given as argument and copies none of its text).

Predictions: the kept masks and the recorded text lines of the four writer fixtures (tests/golden/writer_*.npz), a
four-image data set on the 2048x1024 canvas.  Ground truth: a seeded 16-bit id image per fixture derived from the
masks -- each shifted by up to 12 px and painted far to near as label * 1000 + k; some cut in half, some shrunk
below 100 pixels, some turned into groups (id = label) or caravans (29000 + k), some left out; a void strip on the
left (3) and at the bottom (1) over road (7).  A fifth 37x53 image of hand-placed rectangles pins row tails and
unaligned rows; it is matched for its counts only and is not part of the scored set.

Recorded per image (tests/golden/instance_ap_<name>.npz, data only): the id image, the reference's ground-truth
table, per prediction labelID / conf / pixelCount / voidIntersection and its intersections as (prediction, instID,
count) triples; once for the set (instance_ap_set.npz) the AP matrix and the averages.

    python tests/golden/gen_instance_ap_golden.py /path/to/reference/src/lib
"""
import os
import sys
import tempfile
from types import SimpleNamespace

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = ["star16", "mixed32", "selfcross16", "small16"]
VOID_IDS = (0, 1, 2, 3, 4, 5, 6, 9, 10, 14, 15, 16, 18, 29, 30)         # raw pixel values that count as void
H, W = 1024, 2048


def writer_predictions(name):
    z = np.load(os.path.join(HERE, "writer_%s.npz" % name), allow_pickle=False)
    masks = np.unpackbits(z["packed"], axis=2)[:, :, :W].astype(np.uint8) * 255
    return masks[z["keep"]], [str(v) for v in z["lines"]]


def shifted(mask, dx, dy):
    out = np.zeros_like(mask)
    ys, xs = np.nonzero(mask)
    ys, xs = ys + dy, xs + dx
    ok = (ys >= 0) & (ys < mask.shape[0]) & (xs >= 0) & (xs < mask.shape[1])
    out[ys[ok], xs[ok]] = 1
    return out


def ground_truth(masks, labels, seed):
    """The id image of one fixture; masks are in depth order, nearest first."""
    rng = np.random.RandomState(seed)
    gt = np.full((H, W), 7, np.uint16)
    for k in reversed(range(len(masks))):
        kind = rng.choice(["plain", "plain", "plain", "half", "tiny", "group", "caravan", "none"])
        m = shifted(masks[k] > 0, int(rng.randint(-12, 13)), int(rng.randint(-12, 13)))
        ys, xs = np.nonzero(m)
        if kind == "none" or len(ys) == 0:
            continue
        if kind == "half":
            m[:, int(xs.mean()):] = 0
        if kind == "tiny":
            keep = np.zeros_like(m)
            cy, cx = int(np.median(ys)), int(np.median(xs))
            keep[max(cy - 4, 0):cy + 4, max(cx - 4, 0):cx + 4] = 1
            m &= keep
        gt[m > 0] = labels[k] if kind == "group" else 29000 + k if kind == "caravan" else labels[k] * 1000 + k
    road = gt == 7
    strip = np.zeros((H, W), bool)
    strip[:, :160] = True
    gt[strip & road] = 3
    strip[:] = False
    strip[H - 120:, :] = True
    gt[strip & (gt == 7)] = 1
    return gt


def small_image():
    """37x53: rectangles by hand -- two cars, a car group, a person of 12 pixels, a caravan, void on the right."""
    gt = np.full((37, 53), 7, np.uint16)
    gt[2:14, 3:20] = 26001
    gt[10:30, 25:44] = 26002
    gt[30:37, 0:17] = 26
    gt[16:20, 5:8] = 24003
    gt[20:28, 8:20] = 29001
    gt[:, 47:53] = 4
    masks = np.zeros((5, 37, 53), np.uint8)
    masks[0, 1:15, 2:22] = 255                 # car 1
    masks[1, 8:37, 23:53] = 1                  # car 2, running into the void and the last column; value 1, not 255
    masks[2, 28:37, 0:16] = 255                # on the group
    masks[3, 15:29, 4:21] = 255                # person: the small instance and the caravan
    masks[4, 36:37, 52:53] = 255               # one pixel, the image's last
    lines = ["masks/tiny_000000_000001_leftImg8bit_%d.png %d %s\n" % (k, lab, conf)
             for k, (lab, conf) in enumerate([(26, "0.9"), (26, "0.54"), (26, "0.24000001"), (24, "0.6"), (26, "1")])]
    return gt, masks, lines


def main(ref_lib):
    import PIL
    from PIL import Image
    PIL.PILLOW_VERSION = PIL.__version__            # the three names the evaluator's imports still expect
    np.float = float
    np.bool = bool
    sys.path.insert(0, ref_lib)
    tmp = tempfile.mkdtemp()
    os.chdir(tmp)                                   # the evaluator writes matches.json into the working directory
    from datasets.evaluation.cityscapesscripts.evaluation import evalInstanceLevelSemanticLabeling as E
    args = E.args
    args.gtInstancesFile = os.path.join(tmp, "gtInstances.json")
    args.predictionPath = os.path.join(tmp, "results")
    args.quiet = True
    os.makedirs(os.path.join(tmp, "results", "masks"))
    os.makedirs(os.path.join(tmp, "gt"))

    images = []
    for seed, name in enumerate(CASES):
        masks, lines = writer_predictions(name)
        labels = [int(l.split(" ")[1]) for l in lines]
        images.append(("frankfurt_%s" % name, name, ground_truth(masks, labels, 100 + seed), masks, lines))
    gt5, masks5, lines5 = small_image()
    images.append(("tiny_000000_000001", "odd37x53", gt5, masks5, lines5))

    pred_list, gt_list = [], []
    for prefix, name, gt, masks, lines in images:
        gt_path = os.path.join(tmp, "gt", prefix + "_gtFine_instanceIds.png")
        Image.fromarray(gt).save(gt_path)
        assert np.array_equal(np.array(Image.open(gt_path)), gt)
        txt = os.path.join(tmp, "results", prefix + "_leftImg8bit.txt")
        with open(txt, "w") as f:
            f.write("".join(lines))
        for line, m in zip(lines, masks):
            Image.fromarray(m).save(os.path.join(tmp, "results", line.split(" ")[0]))
        pred_list.append(txt)
        gt_list.append(gt_path)

    E.setInstanceLabels(args)
    gt_instances = E.getGtInstances(gt_list, args)
    matches = E.matchGtWithPreds(pred_list, gt_list, gt_instances, args)
    scored = {os.path.abspath(p): matches[os.path.abspath(p)] for p in gt_list[:len(CASES)]}
    ap = E.evaluateMatches(scored, args)
    avg = E.computeAverages(ap, args)

    stats = SimpleNamespace(void=0, multi=0, group=0, small=0, caravan=0)
    for (prefix, name, gt, masks, lines), gt_path in zip(images, gt_list):
        m = matches[os.path.abspath(gt_path)]
        table = sorted((g["instID"], g["labelID"], g["pixelCount"]) for lab in args.instLabels
                       for g in gt_instances[os.path.abspath(gt_path)][lab])
        by_file = {}
        for lab in args.instLabels:
            for p in m["prediction"][lab]:
                by_file[os.path.basename(p["imgName"])] = p
            for g in m["groundTruth"][lab]:
                stats.multi += len(g["matchedPred"]) >= 2 and name != "odd37x53"
                stats.small += g["instID"] >= 1000 and g["pixelCount"] < 100 and name != "odd37x53"
        rows, triples = [], []
        for k, line in enumerate(lines):
            p = by_file[os.path.basename(line.split(" ")[0])]          # every prediction here has pixels and a label
            rows.append((p["labelID"], p["pixelCount"], p["voidIntersection"]))
            assert p["confidence"] == float(line.split(" ")[2])
            for g in p["matchedGt"]:
                triples.append((k, g["instID"], g["intersection"]))
                stats.group += g["instID"] < 1000 and name != "odd37x53"
            if name != "odd37x53":
                stats.void += p["voidIntersection"] > 0
                caravan = int(((gt >= 29000) & (gt < 30000) & (masks[k] > 0)).sum())
                raw_void = int((np.isin(gt, VOID_IDS) & (masks[k] > 0)).sum())
                stats.caravan += caravan > 0 and p["voidIntersection"] == raw_void
        rows = np.array(rows, np.int64).reshape(-1, 3)
        extra = {"masks_packed": np.packbits(masks > 0, axis=2)} if name == "odd37x53" else {}
        np.savez_compressed(os.path.join(HERE, "instance_ap_%s.npz" % name), gt_ids=gt,
                            gt_table=np.array(table, np.int64).reshape(-1, 3), label_id=rows[:, 0],
                            conf=np.array([float(l.split(" ")[2]) for l in lines], np.float64),
                            pixel_count=rows[:, 1], void_intersection=rows[:, 2],
                            intersections=np.array(triples, np.int64).reshape(-1, 3), lines=np.array(lines), **extra)
        print(name, "gt", len(table), "preds", len(lines), "pairs", len(triples))

    # what makes the fixture worth having; a regeneration that loses one of these fails here
    finite = int(np.isfinite(ap[0]).any(axis=1).sum())
    print("allAp %.4f allAp50%% %.4f finite classes %d" % (avg["allAp"], avg["allAp50%"], finite), vars(stats))
    assert 0.05 < avg["allAp"] < 0.95 and finite >= 6
    assert stats.void >= 1, "no prediction touches void"
    assert stats.multi >= 1, "no ground truth with two matched predictions"
    assert stats.group >= 1, "no intersected group id below 1000"
    assert stats.small >= 1, "no kept ground-truth instance under 100 pixels"
    assert stats.caravan >= 1, "no caravan overlap that stays out of the void count"
    np.savez_compressed(os.path.join(HERE, "instance_ap_set.npz"), ap=np.asarray(ap, np.float64),
                        all_ap=np.float64(avg["allAp"]), all_ap50=np.float64(avg["allAp50%"]),
                        class_ap=np.array([avg["classes"][l]["ap"] for l in args.instLabels], np.float64),
                        class_ap50=np.array([avg["classes"][l]["ap50%"] for l in args.instLabels], np.float64),
                        inst_labels=np.array(args.instLabels), images=np.array(CASES))


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(os.path.abspath(sys.argv[1]))

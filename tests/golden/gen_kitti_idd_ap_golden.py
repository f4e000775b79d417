"""Fixtures of the KITTI and IDD instance-level AP, from the reference's own evaluators (development machine only:
it imports kittiscripts' evalInstanceLevelSemanticLabeling and IDDscripts' evaluate_instance_segmentation from the
reference checkout given as argument and copies none of their text).

Predictions: the masks and text lines of the class writer fixtures (tests/golden/class_writer_*.npz), written in
each data set's layout (KITTI flat, IDD one directory per city).  Ground truth: a seeded 16-bit id image per fixture
derived from the masks -- each shifted by up to 12 px and painted in turn in the data set's encoding (KITTI
label * 256 + k, IDD label * 1000 + k); some cut in half, some shrunk below 100 pixels, some left out, some given
an id the evaluator does not take (KITTI: a label without instances; IDD: thousands outside 6..18, a bare label id
below 1000, and a region of 255); a strip of a label ignored in evaluation on the left.  The 37x53 image is matched
for its counts only and is not part of a scored set.

Recorded per image (tests/golden/kitti_idd_ap_<name>.npz, data only): the id image, the reference's ground-truth
table, per prediction labelID / conf / pixelCount / voidIntersection and its intersections as (prediction, instID,
count) triples; per data set (kitti_idd_ap_set_<kitti|idd>.npz) the AP matrix, the averages, the label names and
ids and the void values as the evaluator's own label table has them.

    python tests/golden/gen_kitti_idd_ap_golden.py /path/to/reference/src/lib
"""
import importlib
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SETS = {"kitti": (["kitti_a", "kitti_b", "odd"], 2, "datasets.evaluation.kittiscripts.evaluation.evalInstanceLevelSemanticLabeling"),
        "idd": (["idd_a", "idd_b"], 2, "datasets.evaluation.IDDscripts.evaluation.evaluate_instance_segmentation")}


def writer_fixture(name):
    z = np.load(os.path.join(HERE, "class_writer_%s.npz" % name), allow_pickle=False)
    W = int(z["width"])
    masks = np.unpackbits(z["packed"], axis=2)[:, :, :W].astype(np.uint8) * 255
    return masks, [str(v) for v in z["lines"]], str(z["file_name"])


def shifted(mask, dx, dy):
    out = np.zeros_like(mask)
    ys, xs = np.nonzero(mask)
    ys, xs = ys + dy, xs + dx
    ok = (ys >= 0) & (ys < mask.shape[0]) & (xs >= 0) & (xs < mask.shape[1])
    out[ys[ok], xs[ok]] = 1
    return out


def ground_truth(masks, labels, seed, kind_of_set, background, void_value):
    rng = np.random.RandomState(seed)
    H, W = masks.shape[1:]
    gt = np.full((H, W), background, np.uint16)
    step = 256 if kind_of_set == "kitti" else 1000
    refused = 0
    for k in reversed(range(len(masks))):
        kind = rng.choice(["plain", "plain", "plain", "half", "tiny", "refused", "refused", "none"])
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
        value = labels[k] * step + k
        if kind == "refused":
            value = [20 * step + k, 4 * step + k, labels[k], 255][refused % 4] if kind_of_set == "idd" else 21 * step + k
            refused += 1
        gt[m > 0] = value
    strip = np.zeros((H, W), bool)
    strip[:, :max(W // 8, 2)] = True
    gt[strip & (gt == background)] = void_value
    return gt


def main(ref_lib):
    import PIL
    from PIL import Image
    PIL.PILLOW_VERSION = PIL.__version__            # the three names the evaluators' imports still expect
    np.float = float
    np.bool = bool
    sys.path.insert(0, ref_lib)
    for which, (cases, scored, module) in SETS.items():
        tmp = tempfile.mkdtemp()
        os.chdir(tmp)                               # the evaluators write matches.json into the working directory
        argv, sys.argv = sys.argv, sys.argv[:1]
        E = importlib.import_module(module)
        sys.argv = argv
        args = E.config if hasattr(E, "config") else E.args
        args.gtInstancesFile = os.path.join(tmp, "gtInstances.json")
        args.predictionPath = os.path.join(tmp, "results")
        args.predictionWalk = None
        args.quiet = True
        void_ids = [l.id for l in E.labels if l.ignoreInEval]
        # background: road, which neither evaluator ignores (7 in KITTI's table, 0 in IDD's); the strip: a label it does
        background, void_value = (7, 3) if which == "kitti" else (0, 7)
        assert background not in void_ids and void_value in void_ids
        images, pred_list, gt_list = [], [], []
        for seed, name in enumerate(cases):
            masks, lines, file_name = writer_fixture(name)
            labels = [int(l.split(" ")[1]) for l in lines]
            gt = ground_truth(masks, labels, 200 + seed, which, background, void_value)
            base = os.path.basename(file_name)
            if which == "kitti":
                gt_path = os.path.join(tmp, "gt", base)
                res_dir = os.path.join(tmp, "results")
            else:
                city = os.path.basename(os.path.dirname(file_name))
                gt_path = os.path.join(tmp, "gt", city, base.split("_")[0] + "_gtFine_instanceids.png")
                res_dir = os.path.join(tmp, "results", city)
            os.makedirs(os.path.dirname(gt_path), exist_ok=True)
            os.makedirs(res_dir, exist_ok=True)
            Image.fromarray(gt).save(gt_path)
            assert np.array_equal(np.array(Image.open(gt_path)), gt)
            txt = os.path.join(res_dir, base.replace(".png", ".txt"))
            with open(txt, "w") as f:
                f.write("".join(lines))
            for line, m in zip(lines, masks):
                Image.fromarray(m).save(os.path.join(res_dir, line.split(" ")[0]))
            images.append((name, gt, masks, lines))
            pred_list.append(txt)
            gt_list.append(gt_path)

        for gt_path, txt in zip(gt_list, pred_list):         # the evaluator's own file lookup finds each text file
            assert os.path.abspath(E.getPrediction(gt_path, args)) == os.path.abspath(txt)
        E.setInstanceLabels(args)
        gt_instances = E.getGtInstances(gt_list, args)
        matches = E.matchGtWithPreds(pred_list, gt_list, gt_instances, args)
        ap = E.evaluateMatches({os.path.abspath(p): matches[os.path.abspath(p)] for p in gt_list[:scored]}, args)
        avg = E.computeAverages(ap, args)

        refused = 0
        for (name, gt, masks, lines), gt_path in zip(images, gt_list):
            m = matches[os.path.abspath(gt_path)]
            table = sorted((g["instID"], g["labelID"], g["pixelCount"]) for lab in args.instLabels
                           for g in gt_instances[os.path.abspath(gt_path)][lab])
            refused += len(np.unique(gt)) - len(table)
            by_file = {}
            for lab in args.instLabels:
                for p in m["prediction"][lab]:
                    by_file[os.path.basename(p["imgName"])] = p
            rows, triples, scored_lines = [], [], []
            for k, line in enumerate(lines):
                p = by_file.get(os.path.basename(line.split(" ")[0]))
                if p is None:                                         # a mask without pixels: the evaluator skips it
                    assert not (masks[k] > 0).any()
                    continue
                scored_lines.append(k)
                rows.append((p["labelID"], p["pixelCount"], p["voidIntersection"]))
                assert p["confidence"] == float(line.split(" ")[2])
                for g in p["matchedGt"]:
                    triples.append((k, g["instID"], g["intersection"]))
            rows = np.array(rows, np.int64).reshape(-1, 3)
            np.savez_compressed(os.path.join(HERE, "kitti_idd_ap_%s.npz" % name), gt_ids=gt,
                                gt_table=np.array(table, np.int64).reshape(-1, 3),
                                scored_lines=np.array(scored_lines, np.int64), label_id=rows[:, 0],
                                pixel_count=rows[:, 1], void_intersection=rows[:, 2],
                                intersections=np.array(triples, np.int64).reshape(-1, 3))
            print(which, name, "gt", len(table), "preds", len(scored_lines), "pairs", len(triples))
        finite = int(np.isfinite(ap[0]).any(axis=1).sum())
        print(which, "allAp %.4f allAp50%% %.4f finite classes %d, ids kept out %d"
              % (avg["allAp"], avg["allAp50%"], finite, refused))
        assert 0.02 < avg["allAp"] < 0.98 and finite >= 2 and refused >= 3
        np.savez_compressed(os.path.join(HERE, "kitti_idd_ap_set_%s.npz" % which), ap=np.asarray(ap, np.float64),
                            all_ap=np.float64(avg["allAp"]), all_ap50=np.float64(avg["allAp50%"]),
                            class_ap=np.array([avg["classes"][l]["ap"] for l in args.instLabels], np.float64),
                            class_ap50=np.array([avg["classes"][l]["ap50%"] for l in args.instLabels], np.float64),
                            inst_labels=np.array(args.instLabels),
                            inst_ids=np.array(args.instIds if hasattr(args, "instIds") else
                                              [E.name2label[l].id for l in args.instLabels], np.int64),
                            void_ids=np.array(void_ids, np.int64), images=np.array(cases[:scored]),
                            pil_version=np.array(PIL.__version__))


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(os.path.abspath(sys.argv[1]))

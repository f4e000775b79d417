"""Fixtures of the pixel-level evaluation, from the reference's own evaluators (development machine only: it imports
evalPixelLevelSemanticLabeling of the cityscapesscripts and of the kittiscripts from the reference checkout given as
argument, runs their pure-Python paths and copies none of their text).

Ground truth: the id images of tests/golden/instance_ap_{star16,mixed32,selfcross16,small16,odd37x53}.npz and a sixth
29x41 image made here (`missed_image`: instances without a correct pixel, which the five do not have); for KITTI
the same images re-encoded as label * 256 + k (pixel_level_host-independent: `kitti_ids` below).  The label images the
evaluators read are derived from them by each protocol's id rule.  Predictions: the kept masks of the writer fixtures
(tests/golden/writer_*.npz; for the 37x53 image the masks recorded with it) painted far to near with the label of
their text line over label 0.

Recorded (data only):
  pixel_level_<name>.npz   the prediction, the KITTI id image, and per protocol the image's 34x34 matrix and its
                           instance rows (id, size, tp, category tp).  The evaluators keep no per-instance numbers, so
                           the rows are counted here with numpy and must add up to the evaluators' per-image class and
                           category sums (tp, fn, tpWeighted, fnWeighted), which is asserted.
  pixel_level_set.json     per protocol every entry of the result dictionary over the six images, and the label table
                           (id, name, category, hasInstances, ignoreInEval) as the evaluators hold it.

    python tests/golden/gen_pixel_level_golden.py /path/to/reference/src/lib
"""
import importlib.util
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = ["star16", "mixed32", "selfcross16", "small16", "odd37x53", "missed29x41"]
W = 2048


def missed_image():
    """29x41, by hand: what the other fixtures lack -- instances without one correct pixel.  A car predicted as a
    truck (tp 0, category tp > 0), a person nobody predicted (both 0), a rider half found."""
    gt = np.full((29, 41), 7, np.uint16)
    gt[2:12, 3:19] = 26001
    gt[14:27, 5:9] = 24002
    gt[5:25, 24:33] = 25003
    pred = np.zeros((29, 41), np.uint8)
    pred[1:13, 2:17] = 27
    pred[5:16, 22:35] = 25
    pred[20:29, 30:41] = 33
    return gt, pred


def kitti_ids(gt):
    """A Cityscapes id image in the KITTI encoding: label * 256 + k, k = 0 for a region that is no instance."""
    gt = gt.astype(np.int64)
    return np.where(gt < 1000, gt * 256, gt // 1000 * 256 + gt % 1000).astype(np.uint16)


def prediction(name, shape):
    """Label image of the fixture's predicted masks, painted far to near (the masks are in depth order, nearest
    first) over label 0."""
    z = np.load(os.path.join(HERE, "instance_ap_%s.npz" % name), allow_pickle=False)
    if name == "odd37x53":
        masks = np.unpackbits(z["masks_packed"], axis=2)[:, :, :shape[1]]
    else:
        w = np.load(os.path.join(HERE, "writer_%s.npz" % name), allow_pickle=False)
        masks = np.unpackbits(w["packed"], axis=2)[:, :, :W][w["keep"]]
    labels = [int(str(l).split(" ")[1]) for l in z["lines"]]
    assert len(labels) == len(masks)
    pred = np.zeros(shape, np.uint8)
    for k in reversed(range(len(masks))):
        pred[masks[k] > 0] = labels[k]
    return pred


def instance_rows(pred, inst, ids, label_of, group_ids):
    rows = []
    for i in ids:
        mask = inst == i
        lab = int(label_of(i))
        cat = [g for g in group_ids if lab in g]
        rows.append((int(i), int(np.count_nonzero(mask)), int(np.count_nonzero(pred[mask] == lab)),
                     int(np.count_nonzero(mask & np.isin(pred, cat[0]))) if cat else 0))
    return np.array(rows, np.int64).reshape(-1, 4)


def load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def main(ref_lib):
    import PIL
    from PIL import Image
    PIL.PILLOW_VERSION = PIL.__version__            # the three names the evaluators' imports still expect
    np.float = float
    np.bool = bool
    ev_dir = os.path.join(ref_lib, "datasets", "evaluation")
    sys.path[:0] = [ref_lib, ev_dir]
    tmp = tempfile.mkdtemp(prefix="pixlevel")
    assert "semantic" not in tmp and "labelIds" not in tmp
    C = load(os.path.join(ev_dir, "cityscapesscripts", "evaluation", "evalPixelLevelSemanticLabeling.py"), "cs_pixel")
    K = load(os.path.join(ev_dir, "kittiscripts", "evaluation", "evalPixelLevelSemanticLabeling.py"), "kitti_pixel")
    assert not C.CSUPPORT and not K.CSUPPORT
    setups = {"cityscapes": (C, C.args, lambda v: v if v < 1000 else v // 1000, lambda v: v > 1000),
              "kitti": (K, K.config, lambda v: v // 256, lambda v: v % 256 > 0)}
    for mod, cfg, _, _ in setups.values():
        cfg.quiet = True
    images, per_image = {}, {}
    for name in CASES:
        if name == "missed29x41":
            gt, pred = missed_image()
        else:
            gt = np.load(os.path.join(HERE, "instance_ap_%s.npz" % name), allow_pickle=False)["gt_ids"]
            pred = prediction(name, gt.shape)
        images[name] = {"cityscapes": gt, "kitti": kitti_ids(gt), "pred": pred}
        per_image[name] = {"pred": pred, "kitti_ids": images[name]["kitti"]}
        if name == "missed29x41":
            per_image[name]["gt_ids"] = gt
    out = {}
    for proto, (mod, cfg, label_of, interest) in setups.items():
        root = os.path.join(tmp, proto)
        # the label image's path holds what the evaluator replaces to find the instance image
        gt_dir, inst_dir = (("semantic", "instance") if proto == "kitti" else ("labelIds", "instanceIds"))
        for d in (gt_dir, inst_dir, "pred"):
            os.makedirs(os.path.join(root, d))
        cfg.exportFile = os.path.join(root, "export", "result.json")
        table = [(l.id, l.name, l.category, bool(l.hasInstances), bool(l.ignoreInEval)) for l in mod.labels if l.id >= 0]
        group_ids = [[l.id for l in mod.category2labels[c] if l.id >= 0] for c in ("human", "vehicle")]
        ignore = {l.id: l.ignoreInEval for l in mod.labels}
        has = {l.id: l.hasInstances for l in mod.labels}
        preds, gts = [], []
        stats = {"group": 0, "caravan": 0, "tp0": 0}
        for name in CASES:
            inst = images[name][proto]
            wide = inst.astype(np.int64)
            lab = (wide // 256 if proto == "kitti" else np.where(wide < 1000, wide, wide // 1000)).astype(np.uint8)
            paths = [os.path.join(root, d, name + ".png") for d in (gt_dir, inst_dir, "pred")]
            for path, arr in zip(paths, (lab, inst, images[name]["pred"])):
                Image.fromarray(arr).save(path)
                assert np.array_equal(np.array(Image.open(path)), arr)
            gts.append(paths[0])
            preds.append(paths[2])
            conf = mod.generateMatrix(cfg)
            inst_stats = mod.generateInstanceStats(cfg)
            n = mod.evaluatePair(paths[2], paths[0], conf, inst_stats, {}, cfg)
            assert n == inst.size == int(conf.sum())
            ids = [int(i) for i in np.unique(inst) if interest(int(i)) and not ignore[label_of(int(i))]]
            assert all(has[label_of(i)] for i in ids)
            rows = instance_rows(images[name]["pred"], inst, ids, label_of, group_ids)
            # the rows add up to the evaluator's own sums, in its order
            mine = {}
            for i, size, tp, cat_tp in rows:
                l = mod.id2label[label_of(int(i))]
                weight = cfg.avgClassSize[l.name] / float(size)
                for key, t in ((("classes", l.name), tp), (("categories", l.category), cat_tp)):
                    s = mine.setdefault(key, {"tp": 0.0, "tpWeighted": 0.0, "fn": 0.0, "fnWeighted": 0.0})
                    s["tp"] += t
                    s["fn"] += size - t
                    s["tpWeighted"] += float(t) * weight
                    s["fnWeighted"] += float(size - t) * weight
            for kind in ("classes", "categories"):
                for key, s in inst_stats[kind].items():
                    want = mine.get((kind, key), {"tp": 0.0, "tpWeighted": 0.0, "fn": 0.0, "fnWeighted": 0.0})
                    for f in want:
                        assert s[f] == want[f], (proto, name, kind, key, f, s[f], want[f])
            per_image[name]["conf_" + proto] = conf.astype(np.int64)
            per_image[name]["rows_" + proto] = rows
            regions = np.unique(inst)
            stats["group"] += sum(1 for v in regions if not interest(int(v)) and has[label_of(int(v))])
            stats["caravan"] += sum(1 for v in regions if label_of(int(v)) == 29)
            stats["tp0"] += int((rows[:, 2] == 0).sum())
            print(proto, name, "instances", len(rows), "pixels", n)
        res = mod.evaluateImgLists(preds, gts, cfg)
        # what makes the fixture worth having; a regeneration that loses one of these fails here
        inside = lambda v: np.isfinite(v) and 0.02 < v < 0.98                       # noqa: E731
        good = [n for n in res["classScores"] if inside(res["classScores"][n]) and inside(res["classInstScores"][n])]
        print(proto, {n: (round(res["classScores"][n], 3), round(res["classInstScores"][n], 3))
                      for n in res["classInstScores"] if np.isfinite(res["classInstScores"][n])}, stats)
        assert len(good) >= 3, good
        for c in ("human", "vehicle"):
            assert inside(res["categoryScores"][c]) and inside(res["categoryInstScores"][c]), c
        assert stats["group"] >= 1, "no group region"
        assert stats["caravan"] >= 1, "no ignored label with instances (caravan)"
        assert stats["tp0"] >= 1, "no instance with tp == 0"
        assert any(abs(res["classScores"][n] - res["classInstScores"][n]) > 0.01 for n in good)
        out[proto] = {"result": res, "labels": table,
                      "avgClassSize": {k: float(v) for k, v in cfg.avgClassSize.items()}}
    for name in CASES:
        np.savez_compressed(os.path.join(HERE, "pixel_level_%s.npz" % name), **per_image[name])
    with open(os.path.join(HERE, "pixel_level_set.json"), "w") as f:
        json.dump({"images": CASES, "protocols": out}, f, indent=1)


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(os.path.abspath(sys.argv[1]))

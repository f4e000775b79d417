"""Fixtures of the panoptic evaluation, from the reference's own converter and evaluator (development machine only: it
imports createPanopticImgs and evalPanopticSemanticLabeling of the cityscapesscripts from the reference checkout given
as argument, runs them and copies none of their text).

Images: the six of the pixel-level fixtures (gen_pixel_level_golden.CASES) and a seventh made here, `edge31x47`, which
holds the edge cases of the protocol (see edge_image).  Ground truth: the reference's convert2panoptic run on the id
images in a temporary gtFine/{val,train,test}/<city>/ tree.  Predictions: the kept masks of the writer fixtures painted
far to near, segment id = label * 1000 + k for slot k; `edge31x47` carries its own.  Scoring: pq_compute_single_core,
called directly (no process pool) per image and over the set, and average_pq over the set.

Recorded (data only):
  panoptic_<name>.npz   index (uint8: the slot that owns a pixel, 255 none), labels (the slots' labels), gt_ids where
                        the id image is no fixture yet, seg [G + 1, 4] and pairs [G + 1, n + 1] in the layout of
                        cp_panoptic_pairs, counted with np.unique on the converter's PNG and the prediction as the
                        evaluator counts them, and the image's stat [L, 3] = tp, fp, fn and iou [L] from the evaluator
  panoptic_set.json     the set's result dictionary, its tp / fp / fn / iou, the categories and the image list

    python tests/golden/gen_panoptic_golden.py /path/to/reference/src/lib
"""
import copy
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from gen_pixel_level_golden import CASES, W, load  # noqa: E402

EDGE = "edge31x47"
L = 34


def edge_image():
    """31 x 47, by hand.  Ground truth over road (7), with sky (23) below: two stuff segments nobody predicts.
    Returns (gt uint16, index uint8, slot labels)."""
    gt = np.full((31, 47), 7, np.uint16)
    index = np.full((31, 47), 255, np.uint8)
    gt[28:31, :] = 23
    # slot 0: IoU exactly 1/2 (areas 15 and 15, intersection 10): no match, a false positive and a false negative
    gt[1, 0:15] = 26001
    index[1, 5:20] = 0
    # slot 1: just above (intersection 11, union 19): a match
    gt[3, 0:15] = 26002
    index[3, 4:19] = 1
    # slot 2: 7 of its 14 pixels on the person, 7 on VOID: union 10 with the VOID pixels taken out (IoU 0.7), 17 without
    gt[5, 0:10] = 24001
    gt[5, 10:17] = 0
    index[5, 3:17] = 2
    # slot 3: a car inside the car crowd region (value 26): unmatched, saved from fp by the crowd
    gt[8:10, 0:10] = 26
    index[8:10, 2:8] = 3
    # slot 4: a person, 5 of 10 pixels on VOID and no crowd: 2 x == area exactly, not saved
    gt[12, 0:5] = 0
    index[12, 0:10] = 4
    # a caravan (ignored label with instances): VOID; slot 5, a car, lies partly on it
    gt[15:17, 0:6] = 29001
    index[15:17, 3:10] = 5
    # slot 6: a rider found well; slot 7 owns no pixel
    gt[20:26, 20:31] = 25001
    index[20:26, 21:32] = 6
    return gt, index, np.array([26, 26, 24, 26, 24, 26, 25, 33], np.int32)


def fixture_prediction(name, shape):
    """(index, labels) of a fixture's predicted masks (depth order, nearest first): the nearest mask owns a pixel."""
    z = np.load(os.path.join(HERE, "instance_ap_%s.npz" % name), allow_pickle=False)
    if name == "odd37x53":
        masks = np.unpackbits(z["masks_packed"], axis=2)[:, :, :shape[1]]
    else:
        w = np.load(os.path.join(HERE, "writer_%s.npz" % name), allow_pickle=False)
        masks = np.unpackbits(w["packed"], axis=2)[:, :, :W][w["keep"]]
    labels = np.array([int(str(l).split(" ")[1]) for l in z["lines"]], np.int32)
    assert len(labels) == len(masks) <= 255
    index = np.full(shape, 255, np.uint8)
    for k in reversed(range(len(masks))):
        index[masks[k] > 0] = k
    return index, labels


def image(name):
    """(gt ids, index, labels, whether the id image is a fixture already)."""
    if name == EDGE:
        return edge_image() + (False,)
    if name == "missed29x41":
        z = np.load(os.path.join(HERE, "pixel_level_missed29x41.npz"), allow_pickle=False)
        gt = z["gt_ids"]
        index = np.full(gt.shape, 255, np.uint8)                 # its label image: one slot per predicted label
        labels = np.array([v for v in np.unique(z["pred"]) if v], np.int32)
        for k, v in enumerate(labels):
            index[z["pred"] == v] = k
        return gt, index, labels, True
    gt = np.load(os.path.join(HERE, "instance_ap_%s.npz" % name), allow_pickle=False)["gt_ids"]
    return (gt,) + fixture_prediction(name, gt.shape) + (True,)


def tables(pan_gt, gt_ann, index, n):
    """seg and pairs in the device layout from the converter's PNG ids and annotation, counted with np.unique."""
    segs = sorted(gt_ann["segments_info"], key=lambda s: s["id"])
    row = {s["id"]: r for r, s in enumerate(segs, 1)}
    row[0] = 0
    pairs = np.zeros((len(segs) + 1, n + 1), np.int64)
    col = np.minimum(index.astype(np.int64), n)
    keys, counts = np.unique(pan_gt.astype(np.int64) * 256 + col, return_counts=True)
    for key, cnt in zip(keys, counts):
        pairs[row[int(key) // 256], int(key) % 256] = cnt
    seg = np.zeros((len(segs) + 1, 4), np.int64)
    seg[0] = [len(segs), pairs[0].sum(), 0, 0]
    for r, s in enumerate(segs, 1):
        seg[r] = [s["id"], s["category_id"], s["iscrowd"], s["area"]]
        assert pairs[r].sum() == s["area"]
    return seg, pairs


def notable(seg, pairs, labels):
    """Which of the protocol's edge cases an image shows, from its tables (floats as the evaluator compares)."""
    n = len(labels)
    area_p = pairs[:, :n].sum(0)
    found = set()
    matched = set()
    for r in range(1, len(seg)):
        for i in range(n):
            inter = int(pairs[r, i])
            if not inter or seg[r, 2] or seg[r, 1] != labels[i]:
                continue
            with_void = int(seg[r, 3] + area_p[i] - inter)
            union = with_void - int(pairs[0, i])
            if inter / union > 0.5:
                matched.add(i)
                if not inter / with_void > 0.5:
                    found.add("void flips a match")
                if 2 * inter - union <= 3:
                    found.add("just above one half")
            elif 2 * inter == union:
                found.add("exactly one half")
    crowd = {int(seg[r, 1]): r for r in range(1, len(seg)) if seg[r, 2]}
    for i in range(n):
        if area_p[i] == 0 or i in matched:
            continue
        void = int(pairs[0, i])
        x = void + (int(pairs[crowd[labels[i]], i]) if labels[i] in crowd else 0)
        if x / area_p[i] > 0.5 and not void / area_p[i] > 0.5:
            found.add("crowd saves")
        if 2 * x == area_p[i]:
            found.add("not saved at exactly half")
    return found


def main(ref_lib):
    import PIL
    from PIL import Image
    PIL.PILLOW_VERSION = PIL.__version__            # the name the scripts' imports still expect
    ev_dir = os.path.join(ref_lib, "datasets", "evaluation")
    sys.path[:0] = [ref_lib, ev_dir]
    make = load(os.path.join(ev_dir, "cityscapesscripts", "preparation", "createPanopticImgs.py"), "cs_make_panoptic")
    ev = load(os.path.join(ev_dir, "cityscapesscripts", "evaluation", "evalPanopticSemanticLabeling.py"), "cs_panoptic")
    tmp = tempfile.mkdtemp(prefix="panoptic")
    names = CASES + [EDGE]
    data = {name: image(name) for name in names}
    for split, members in (("val", names), ("train", [EDGE]), ("test", [EDGE])):
        os.makedirs(os.path.join(tmp, "gtFine", split, "city"))
        for name in members:
            path = os.path.join(tmp, "gtFine", split, "city", name + "_gtFine_instanceIds.png")
            Image.fromarray(data[name][0]).save(path)
            assert np.array_equal(np.array(Image.open(path)), data[name][0])
    out = os.path.join(tmp, "panoptic")
    pred_dir = os.path.join(tmp, "pred")
    os.makedirs(out)
    os.makedirs(pred_dir)
    make.convert2panoptic(os.path.join(tmp, "gtFine"), out)
    with open(os.path.join(out, "cityscapes_panoptic_val.json")) as f:
        gt_json = json.load(f)
    gt_folder = os.path.join(out, "cityscapes_panoptic_val")
    categories = {c["id"]: c for c in gt_json["categories"]}
    gt_anns = {a["image_id"]: a for a in gt_json["annotations"]}
    pairs_of, found, void_caravan = [], set(), 0
    for name in names:
        gt, index, labels, known = data[name]
        ids = np.zeros(gt.shape, np.int64)
        owned = index < 255
        ids[owned] = labels[index[owned]].astype(np.int64) * 1000 + index[owned]
        Image.fromarray(np.stack([ids % 256, ids // 256 % 256, ids // 65536], 2).astype(np.uint8)).save(
            os.path.join(pred_dir, name + "_panoptic.png"))
        pred_ann = {"image_id": name, "file_name": name + "_panoptic.png",
                    "segments_info": [{"id": int(labels[k]) * 1000 + k, "category_id": int(labels[k])}
                                      for k in range(len(labels)) if (index == k).any()]}
        pairs_of.append((gt_anns[name], pred_ann))
        stat = ev.pq_compute_single_core(0, [copy.deepcopy(pairs_of[-1])], gt_folder, pred_dir, categories)
        pan_gt = ev.rgb2id(np.array(Image.open(os.path.join(gt_folder, gt_anns[name]["file_name"])), dtype=np.uint32))
        seg, pairs = tables(pan_gt, gt_anns[name], index, len(labels))
        rec = {"index": index, "labels": labels, "seg": seg, "pairs": pairs,
               "stat": np.array([[stat[l].tp, stat[l].fp, stat[l].fn] for l in range(L)], np.int64),
               "iou": np.array([stat[l].iou for l in range(L)], np.float64)}
        if not known:
            rec["gt_ids"] = gt
        np.savez_compressed(os.path.join(HERE, "panoptic_%s.npz" % name), **rec)
        mine = notable(seg, pairs, labels)
        found |= mine
        values = np.unique(gt)
        void_caravan += sum(1 for v in values if v >= 1000 and v // 1000 == 29 and v not in seg[1:, 0])
        print(name, "segments", len(seg) - 1, "slots", len(labels), "tp/fp/fn", rec["stat"].sum(0).tolist(), sorted(mine))
        if name == EDGE:
            assert {"exactly one half", "just above one half"} <= mine, mine
    total = ev.pq_compute_single_core(0, copy.deepcopy(pairs_of), gt_folder, pred_dir, categories)
    res = ev.average_pq(total, categories)
    # what makes the fixtures worth having; a regeneration that loses one of these fails here
    things = [l for l, c in categories.items() if c["isthing"] and 0.02 < res["per_class"][l]["pq"] < 0.98]
    assert len(things) >= 3, things
    for what in ("crowd saves", "not saved at exactly half", "void flips a match"):
        assert what in found, what
    assert void_caravan >= 1, "no ignored label with instances (caravan) in VOID"
    assert any(not c["isthing"] and total[l].fn > 0 and total[l].tp == 0 and total[l].fp == 0
               for l, c in categories.items()), "no stuff class that only collects fn"
    ev.print_results(res, categories)
    with open(os.path.join(HERE, "panoptic_set.json"), "w") as f:
        json.dump({"images": names, "result": res,
                   "stat": {str(l): [int(total[l].tp), int(total[l].fp), int(total[l].fn), float(total[l].iou)]
                            for l in sorted(categories)},
                   "categories": [{k: c[k] for k in ("id", "name", "supercategory", "isthing")}
                                  for c in gt_json["categories"]]}, f, indent=1)


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(os.path.abspath(sys.argv[1]))

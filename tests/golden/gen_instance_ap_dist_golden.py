"""Fixture of the Cityscapes instance-level AP WITH distances (AP 100 m / AP 50 m), from the reference's own evaluator
with `distanceAvailable = True` (development machine only: it imports evalInstanceLevelSemanticLabeling from the
reference checkout given as argument and copies none of its text).

The four scored images of instance_ap_*.npz: the same id images, masks (writer_*.npz) and text lines.  Each gets the
seeded synthetic disparity image and the camera of tests/distance_ref.py; medDist / distConf of every ground-truth
instance are np.median of the pixel distances and the stereo density (distance_ref.host_distances), written into the
evaluator's ground-truth instance JSON, which is where the evaluator reads them from.

Recorded (tests/golden/instance_ap_dist_set.npz, data only): per image the [G, 2] table aligned with the image's
gt_table, the [3, 8, 10] AP matrix, all averages, the lines of the printed table.

    python tests/golden/gen_instance_ap_dist_golden.py /path/to/reference/src/lib
"""
import contextlib
import io
import json
import os
import sys
import tempfile

import numpy as np
import numpy.ma  # noqa: F401  (np.median imports it lazily: before np.bool is patched for the evaluator)

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import distance_ref  # noqa: E402
from gen_instance_ap_golden import CASES, writer_predictions  # noqa: E402

AVERAGES = ("allAp", "allAp50%", "allAp50m", "allAp100m", "allAp50%50m")
CLASS_AVERAGES = ("ap", "ap50%", "ap50m", "ap100m", "ap50%50m")


def check_conditions(tables, gt_tables, ap):
    """What makes the fixture worth having; the test asserts the same on the recorded data."""
    t = np.concatenate(tables)
    g = np.concatenate(gt_tables)
    real = g[:, 0] >= 1000
    big, dense = real & (g[:, 2] >= 1000), t[:, 1] >= 0.5
    assert (big & dense & (t[:, 0] > 100)).sum() >= 1, "no instance excluded by the 100 m bound alone"
    assert (big & dense & (t[:, 0] > 50) & (t[:, 0] <= 100)).sum() >= 1, "none excluded by the 50 m bound alone"
    assert (big & ~dense & (t[:, 0] <= 50)).sum() >= 1, "none excluded by distConf < 0.5 alone"
    assert (real & (g[:, 2] >= 100) & (g[:, 2] < 1000)).sum() >= 1, "no instance of 100 .. 999 pixels"
    assert (big & dense & (t[:, 0] == 50.0)).sum() >= 1, "no instance at exactly 50 m"
    for a in range(3):
        for b in range(a + 1, 3):
            assert not np.array_equal(ap[a], ap[b], equal_nan=True), "slices %d and %d are equal" % (a, b)
    assert int(np.isfinite(ap).all(axis=(0, 2)).sum()) >= 3, "fewer than three classes scored in every slice"


def main(ref_lib):
    import PIL
    from PIL import Image
    PIL.PILLOW_VERSION = PIL.__version__            # the three names the evaluator's imports still expect
    np.float = float
    np.bool = bool
    sys.path.insert(0, ref_lib)
    tmp = tempfile.mkdtemp()
    os.chdir(tmp)
    from datasets.evaluation.cityscapesscripts.evaluation import evalInstanceLevelSemanticLabeling as E
    args = E.args
    args.gtInstancesFile = os.path.join(tmp, "gtInstances.json")
    args.predictionPath = os.path.join(tmp, "results")
    args.quiet = True
    args.colorized = False
    os.makedirs(os.path.join(tmp, "results", "masks"))
    os.makedirs(os.path.join(tmp, "gt"))

    pred_list, gt_list, tables, gt_tables = [], [], [], []
    for index, name in enumerate(CASES):
        z = np.load(os.path.join(HERE, "instance_ap_%s.npz" % name), allow_pickle=False)
        masks, lines = writer_predictions(name)
        assert [str(v) for v in z["lines"]] == lines
        gt, prefix = z["gt_ids"], "frankfurt_%s" % name
        gt_path = os.path.join(tmp, "gt", prefix + "_gtFine_instanceIds.png")
        Image.fromarray(gt).save(gt_path)
        txt = os.path.join(tmp, "results", prefix + "_leftImg8bit.txt")
        with open(txt, "w") as f:
            f.write("".join(lines))
        for line, m in zip(lines, masks):
            Image.fromarray(m).save(os.path.join(tmp, "results", line.split(" ")[0]))
        pred_list.append(txt)
        gt_list.append(gt_path)
        disp = distance_ref.disparity(gt, index)
        tables.append(distance_ref.host_distances(gt, disp, z["gt_table"][:, 0], distance_ref.camera(index)))
        gt_tables.append(z["gt_table"])

    E.setInstanceLabels(args)
    E.getGtInstances(gt_list, args)                                       # writes the JSON
    with open(args.gtInstancesFile) as f:
        gt_json = json.load(f)
    for gt_path, table, gt_table in zip(gt_list, tables, gt_tables):
        row = {int(i): k for k, i in enumerate(gt_table[:, 0])}
        for label, insts in gt_json[os.path.abspath(gt_path)].items():
            for inst in insts:
                if inst["instID"] in row:
                    inst["medDist"], inst["distConf"] = (float(v) for v in table[row[inst["instID"]]])
    with open(args.gtInstancesFile, "w") as f:
        json.dump(gt_json, f)
    args.distanceAvailable = True
    gt_instances = E.getGtInstances(gt_list, args)                        # reads it back
    matches = E.matchGtWithPreds(pred_list, gt_list, gt_instances, args)
    ap = np.asarray(E.evaluateMatches(matches, args), np.float64)
    avg = E.computeAverages(ap, args)
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        E.printResults(avg, args)
    text = out.getvalue()
    print(text)
    assert ap.shape == (3, len(args.instLabels), 10)
    check_conditions(tables, gt_tables, ap)
    np.savez_compressed(
        os.path.join(HERE, "instance_ap_dist_set.npz"), ap=ap,
        averages=np.array([avg[k] for k in AVERAGES], np.float64), average_names=np.array(AVERAGES),
        class_averages=np.array([[avg["classes"][l][k] for k in CLASS_AVERAGES] for l in args.instLabels], np.float64),
        class_average_names=np.array(CLASS_AVERAGES), inst_labels=np.array(args.instLabels), images=np.array(CASES),
        table_lines=np.array(text.split("\n")), **{"dist_%s" % n: t for n, t in zip(CASES, tables)})
    for n, t, g in zip(CASES, tables, gt_tables):
        print(n, np.column_stack([g[:, 0], g[:, 2], np.round(t[:, 0], 2), np.round(t[:, 1], 3)]).tolist())


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(os.path.abspath(sys.argv[1]))

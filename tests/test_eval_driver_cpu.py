"""The host side of scoring from the command line, without a GPU: --metric ap at parse time, the rule that picks
model_best.pth, and test.py's image list (centerpoly_amd/datasets/eval_images.py) on a temporary JSON + PNG data set:
ids, path resolution, the decoded arrays, the ground-truth table a loader worker hands over, the prefetching
DataLoader against the plain loop, and the errors that name a missing file."""
import json
import math
import os

import numpy as np
import pytest

from centerpoly_amd.opts import opts
from centerpoly_amd.utils.utils import BestMetric


def _refused(args, capsys):
    with pytest.raises(SystemExit) as e:
        opts().parse(["polydet"] + args)
    assert e.value.code == 2
    return capsys.readouterr().err


def test_metric_option(capsys):
    assert opts().parse(["polydet"]).metric == "loss"
    assert opts().parse(["polydet", "--metric", "hm_l"]).metric == "hm_l"
    assert opts().parse(["polydet", "--metric", "poly_l", "--dataset", "kitti_poly"]).metric == "poly_l"
    opt = opts().parse(["polydet", "--metric", "ap", "--gt_dir", "/data/gtFine"])
    assert opt.metric == "ap" and opt.no_mask_files is False            # defaults do not move with the metric
    assert opts().parse(["polydet", "--metric", "ap", "--gt_dir", "/g", "--no_mask_files"]).no_mask_files is True
    err = _refused(["--metric", "ap"], capsys)
    assert "--metric ap needs --gt_dir" in err
    for name in ("kitti_poly", "IDD", "synthetic"):
        err = _refused(["--metric", "ap", "--gt_dir", "/g", "--dataset", name], capsys)
        assert "scores nothing" in err and name in err


def test_best_checkpoint_rule():
    nan = float("nan")
    ap = BestMetric("ap")
    wins = [ap.update(v) for v in (nan, 0.0, nan, 0.25, 0.25, 0.1, nan, 0.3)]
    assert wins == [False, True, False, True, False, False, False, True] and ap.best == 0.3
    only_nan = BestMetric("ap")
    assert [only_nan.update(nan), only_nan.update(nan)] == [False, False] and math.isinf(only_nan.best)
    # every other metric is a validation loss statistic: lower wins, from the 1e10 main.py always started at
    for name in ("loss", "hm_l"):
        lo = BestMetric(name)
        assert lo.best == 1e10
        assert [lo.update(v) for v in (2.0, nan, 3.0, 2.0, 1.5, 2e10)] == [True, False, False, False, True, False]
        assert lo.best == 1.5


# ------------------------------------------------------------------------------------------- the image list --
NAMES = ["frankfurt_000000_000294", "frankfurt_000001_011835", "munster_000002_000019"]


def _make_set(tmp_path, gt=True):
    from PIL import Image
    rng = np.random.RandomState(5)
    img_dir, annot_dir, gt_dir = tmp_path / "images", tmp_path / "BBoxes", tmp_path / "gtFine" / "val"
    for d in (img_dir, annot_dir, gt_dir / "frankfurt", gt_dir / "munster"):
        os.makedirs(str(d))
    images, rgb, ids = [], {}, {}
    for k, name in enumerate(NAMES):
        # the annotation files carry the absolute paths of the machine they were made on: re-rooted by base name
        images.append({"id": 100 + 7 * k, "file_name": "/somewhere/else/leftImg8bit/val/%s_leftImg8bit.png" % name,
                       "height": 24, "width": 40})
        rgb[name] = rng.randint(0, 256, (24, 40, 3)).astype(np.uint8)
        Image.fromarray(rgb[name]).save(str(img_dir / (name + "_leftImg8bit.png")))
        g = np.full((24, 40), 7, np.uint16)
        g[2:9, 3:20] = 26000 + k
        g[12:20, 10:30] = 24001
        g[0:2, :] = 33                                                  # a group of bicycles
        g[20:, :] = 1
        ids[name] = g
        if gt:
            Image.fromarray(g).save(str(gt_dir / name.split("_")[0] / (name + "_gtFine_instanceIds.png")))
    with open(str(annot_dir / "val16_regular_interval.json"), "w") as f:
        json.dump({"images": images, "annotations": [], "categories": []}, f)
    return img_dir, annot_dir, tmp_path / "gtFine", rgb, ids


def _dataset(annot_dir, img_dir):
    from centerpoly_amd.datasets.dataset.polygons import CITYSCAPES
    opt = opts().parse(["polydet", "--annot_dir", str(annot_dir), "--img_dir", str(img_dir)])
    return CITYSCAPES(opt, "val")


def test_image_list_and_paths(tmp_path):
    from centerpoly_amd.datasets import eval_images
    from centerpoly_amd.datasets.evaluation import instance_level as il
    img_dir, annot_dir, gt_root, rgb, ids = _make_set(tmp_path)
    ds = _dataset(annot_dir, img_dir)
    assert eval_images.image_prefix("/a/b/%s_leftImg8bit.png" % NAMES[0]) == NAMES[0]
    assert eval_images.image_prefix("000017.png") == "000017"
    plain = eval_images.EvalImages(ds)
    assert len(plain) == 3 and [plain.info(i)[0] for i in range(3)] == [100, 107, 114] == ds.images
    for i, name in enumerate(NAMES):
        item = plain[i]
        assert set(item) == {"img_id", "image"} and item["img_id"] == 100 + 7 * i
        assert item["image"].dtype == np.uint8 and np.array_equal(item["image"], rgb[name][:, :, ::-1])   # BGR
    gt_files = il.find_gt_files(str(gt_root))
    scored = eval_images.EvalImages(ds, gt_files)
    loops = {}
    for what, prefetch, workers in (("loop", False, 0), ("loader", True, 2), ("loader0", True, 0)):
        loops[what] = list(eval_images.iterate(scored, prefetch, workers))
        assert [it["img_id"] for it in loops[what]] == [100, 107, 114]               # in order, none twice
    for i, name in enumerate(NAMES):
        for what in loops:
            it = loops[what][i]
            assert isinstance(it["image"], np.ndarray) and np.array_equal(it["image"], rgb[name][:, :, ::-1])
            assert it["gt_ids"].dtype == np.uint16 and np.array_equal(it["gt_ids"], ids[name])
            assert np.array_equal(it["gt_table"], il.gt_instances(np.bincount(ids[name].reshape(-1), minlength=65536)))
        assert loops["loop"][i]["gt_table"].tolist() == [[33, 33, 80], [24001, 24, 160], [26000 + i, 26, 119]]


def test_missing_files_are_named(tmp_path):
    from centerpoly_amd.datasets import eval_images
    from centerpoly_amd.datasets.evaluation import instance_level as il
    img_dir, annot_dir, gt_root, _, _ = _make_set(tmp_path)
    ds = _dataset(annot_dir, img_dir)
    gt_files = il.find_gt_files(str(gt_root))
    os.remove(str(img_dir / (NAMES[1] + "_leftImg8bit.png")))
    images = eval_images.EvalImages(ds, gt_files)
    images[0]
    with pytest.raises(FileNotFoundError, match=NAMES[1] + "_leftImg8bit.png"):
        images[1]
    with pytest.raises(FileNotFoundError, match=NAMES[1] + "_leftImg8bit.png"):       # not swallowed by a worker
        list(eval_images.iterate(images, True, 2))
    gone = gt_files.pop(NAMES[2])
    with pytest.raises(FileNotFoundError, match=NAMES[2] + "_gtFine_instanceIds.png"):
        eval_images.EvalImages(ds, gt_files)[2]
    gt_files[NAMES[2]] = gone
    os.remove(gone)
    with pytest.raises(FileNotFoundError, match=NAMES[2] + "_gtFine_instanceIds.png"):
        eval_images.EvalImages(ds, gt_files)[2]

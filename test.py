#!/usr/bin/env python3
"""Evaluation driver with the reference's CLI and control flow (src/test.py:47-131):
`python test.py polydet --arch dla_34 --load_model model_last.pth`.  `cityscapes`, `kitti_poly` and `IDD` read their
image files (`dataset.images` -> `coco.loadImgs` -> `read_image`), by default through a prefetching DataLoader whose
workers decode ahead of the detector, with --not_prefetch_test in a plain loop.  With --gt_dir every image is scored on
the device as it passes (score_instances_device of the data set's writer: Cityscapes, or KITTI / IDD by their own
evaluators' protocols) and the instance-level allAp is returned.  With --save_ids / --save_masks every image's
instance maps (detector.instances: id and label images, the table, the masks) are written under
`<save_dir>/instances/` as it passes.  With --pixel_iou (and --gt_dir) the same maps are also scored at pixel level on
the device (evaluation/pixel_level.py): the class and category tables follow the AP table,
resultPixelLevelSemanticLabeling.json is written to save_dir and run_test's dict gains "pixel".  With --panoptic (and
--gt_dir, cityscapes) the maps are scored as a panoptic segmentation on the device (evaluation/panoptic.py): the PQ
table follows, resultPanopticSemanticLabeling.json is written and the dict gains "panoptic"; --save_panoptic writes
the maps in COCO panoptic format under `<save_dir>/panoptic/`.  With --boundary (and --gt_dir; cityscapes, kitti_poly,
IDD) the masks drawn for the AP also go through cp_boundary_overlaps (evaluation/boundary.py): the Boundary AP table
follows the AP table, resultBoundaryInstanceLevel.json is written and the dict gains "boundary".  With --disparity_dir
and --camera_dir (and --gt_dir, cityscapes) the loader also reads every frame's 16-bit disparity image and camera file,
the ground-truth instances' median disparities come from cp_segment_medians in the same read
(evaluation/distances.py), the AP table gets the evaluator's AP_50m / AP_100m / AP_50%50m columns and the dict gains
"allAp100m", "allAp50m" and "allAp50%50m".  With --track the instance maps of the images, in the loader's order, go
through an instance tracker (detectors/tracking.py) that starts anew where the sequence changes (the image's directory
plus `<city>_<seq>` of `<city>_<seq>_<frame>` names); --save_ids then also writes `<stem>_trackIds.png` and
`<stem>_tracks.json`, and with --gt_dir -- whose instance ids must then be consistent over a sequence -- the MOTS
measures (evaluation/tracking.py) are printed after the other tables, resultTracking.json is written and the dict gains
"tracking".  With --save_rle every image's live instances also go to
`<save_dir>/instances/<stem>_rle.json` with their masks as COCO run-length strings, encoded on the device
(utils/rle.py), all of them are collected in `<save_dir>/results_segm.json` (COCO segm results: image_id, category_id,
score, bbox, segmentation), and with --track the frames' owned pixels go to `instances/mots/<sequence>.txt` in the MOTS
text format (--mots_class_map picks and renames the classes).  `--dataset synthetic`
feeds hash-generated uint8 arrays (no files)."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import numpy as np

from centerpoly_amd import synth
from centerpoly_amd.datasets.dataset_factory import get_dataset
from centerpoly_amd.detectors.detector_factory import detector_factory
from centerpoly_amd.opts import opts
from centerpoly_amd.utils.utils import AverageMeter


def run_test(opt, evaluate=True):
    """One pass over the validation images: {"ap": run_eval's return value (None for the synthetic set),
    "results": {image id: {class: rows}}, "dataset": the data set object (its last_evaluator holds the count
    tables of a scored run), "stamps": the clock before the first image and after every image, and with --pixel_iou
    "pixel": the pixel-level result dictionary}.  evaluate=False
    stops after the image loop (tools/probe_eval_tail.py times the loop without run_eval's files)."""
    Dataset = get_dataset(opt.dataset, opt.task)
    opt = opts().update_dataset_info_and_set_heads(opt, Dataset)
    dataset = Dataset(opt, "val")
    detector = detector_factory[opt.task](opt)
    results = {}
    time_stats = ["tot", "load", "pre", "net", "dec", "post", "merge"]
    avg = {t: AverageMeter() for t in time_stats}
    from centerpoly_amd.datasets import eval_images
    batch_size = getattr(opt, "test_batch_size", 1)
    same_size = not opt.fix_res                      # --keep_res: the network input follows the source size

    def detect(items, images):
        """One image through run, several through run_batch: the per-image `results` in order; the averages are per
        image (a batch's times / n)."""
        if batch_size == 1:
            ret = detector.run(images[0])
            per_image, n = [ret["results"]], 1
        else:
            ret = detector.run_batch(images)
            per_image, n = ret["results"], ret["n"]
        for t in avg:
            avg[t].update(ret[t] / n, n)
        return per_image

    save_ids, save_masks = getattr(opt, "save_ids", False), getattr(opt, "save_masks", False)
    device_png = getattr(opt, "device_png", False)
    save_rle, segm = getattr(opt, "save_rle", False), []
    inst_dir = os.path.join(opt.save_dir, "instances")

    def instances_stem(file_name):
        from centerpoly_amd.detectors import instances
        return instances.image_stem(file_name)

    def save_instances(file_name, maps):
        """--save_ids / --save_masks: the instance maps of one image, on its own canvas."""
        from centerpoly_amd.detectors import instances
        stem = instances.image_stem(file_name)
        if save_ids:
            instances.save_ids(maps, inst_dir, stem, device_png=device_png)
        if save_masks:
            instances.save_masks(maps, inst_dir, stem, device_png=device_png)

    def save_rle_instances(item, file_name, maps, rows):
        """--save_rle: <stem>_rle.json, and the image's entries of results_segm.json (the class and the score are the
        source row's)."""
        from centerpoly_amd.detectors import instances
        for _, e in instances.save_rle(maps, inst_dir, instances.image_stem(file_name))[1]:
            row = rows[e["source_row"]]
            segm.append({"image_id": int(item["img_id"]), "category_id": int(dataset._valid_ids[int(row[5])]),
                         "score": float(row[4]), "bbox": e["bbox"], "segmentation": e["segmentation"]})

    if opt.dataset == "synthetic":
        if save_ids or save_masks or save_rle:
            raise ValueError("--save_ids / --save_masks / --save_rle draw with a data set's result writer; the synthetic "
                             "set has none (use cityscapes, kitti_poly or IDD)")
        synthetic =((ind, (synth.uniform("test/img%d" % ind, (opt.input_h, opt.input_w, 3)) * 255).astype(np.uint8))
                     for ind in range(len(dataset)))
        for items in eval_images.group(({"img_id": ind, "image": img} for ind, img in synthetic), batch_size, same_size):
            for item, res in zip(items, detect(items, [item["image"] for item in items])):
                results[item["img_id"]] = res
            print("[{}/{}] ".format(items[-1]["img_id"], len(dataset))
                  + " ".join("|{} {:.3f}s".format(t, avg[t].avg) for t in avg))
        dataset.run_eval(results, opt.save_dir)
        return {"ap": None, "results": results, "dataset": dataset, "stamps": []}
    evaluator = gt_files = protocol = dist_files = None
    if getattr(opt, "gt_dir", "") and (getattr(dataset, "scores_ap", False) or getattr(dataset, "ap_protocol", None)):
        from centerpoly_amd.datasets.evaluation import instance_level
        if not os.path.isdir(opt.gt_dir):
            raise FileNotFoundError("--gt_dir %s is not a directory" % opt.gt_dir)
        protocol = instance_level.PROTOCOLS[getattr(dataset, "ap_protocol", None) or "cityscapes"]
        gt_files = instance_level.find_gt_files(opt.gt_dir, protocol)
        if getattr(opt, "disparity_dir", "") or getattr(opt, "camera_dir", ""):
            from centerpoly_amd.datasets.evaluation import distances
            if opt.dataset not in distances.DATASETS or not (opt.disparity_dir and opt.camera_dir):
                raise ValueError("--disparity_dir needs --camera_dir and the cityscapes data set")
            dist_files = distances.find_files(opt.disparity_dir, opt.camera_dir)
        evaluator = instance_level.InstanceLevelEvaluator(protocol, distances=dist_files is not None)
    pixel = None
    save_pan, pan_entries, pan_dir = getattr(opt, "save_panoptic", False), [], os.path.join(opt.save_dir, "panoptic")
    pan = None
    if getattr(opt, "panoptic", False):
        from centerpoly_amd.datasets.evaluation import panoptic
        if evaluator is None or opt.dataset not in panoptic.DATASETS:
            raise ValueError("--panoptic needs --gt_dir and the cityscapes data set")
        pan = panoptic.PanopticEvaluator(panoptic.CITYSCAPES)
    if getattr(opt, "pixel_iou", False):
        from centerpoly_amd.datasets.evaluation import pixel_level
        if evaluator is None:
            raise ValueError("--pixel_iou needs --gt_dir and a data set with a pixel-level protocol (cityscapes, "
                             "kitti_poly)")
        pixel = pixel_level.PixelLevelEvaluator(pixel_level.PROTOCOLS[pixel_level.DATASET_PROTOCOL[opt.dataset]])
    bnd = None
    if getattr(opt, "boundary", False):
        from centerpoly_amd.datasets.evaluation import boundary
        if evaluator is None:
            raise ValueError("--boundary needs --gt_dir and a data set with an AP protocol (cityscapes, kitti_poly, IDD)")
        bnd = boundary.BoundaryEvaluator(protocol, opt.boundary_ratio, distances=dist_files is not None)
    seq = mots = None
    if getattr(opt, "track", False):
        from centerpoly_amd.detectors import tracking
        seq = tracking.SequenceTracker(opt.track_iou, opt.track_max_age, getattr(opt, "track_motion", False))
        mots_files = tracking.MotsWriter(inst_dir, getattr(opt, "mots_classes", None)) if save_rle else None
        if evaluator is not None:
            from centerpoly_amd.datasets.evaluation import tracking as mots_eval
            mots = mots_eval.TrackingEvaluator(protocol, opt.track_ignore_id)
    images = eval_images.EvalImages(dataset, gt_files, protocol, dist_files)
    stamps = [time.time()]
    ind = -1
    for items in eval_images.group(eval_images.iterate(images, not opt.not_prefetch_test, opt.num_workers), batch_size,
                                   same_size):
        for b, (item, res) in enumerate(zip(items, detect(items, [item["image"] for item in items]))):
            ind += 1
            results[item["img_id"]] = res
            if evaluator is not None:
                extra = {}
                if bnd is not None:                                        # the same masks, the band tables in the same read
                    extra["boundary"] = bnd
                if dist_files is not None:                                 # the instances' median disparities, the same read
                    extra["distances"] = (item["disparity"], item["camera"])
                dataset.score_instances_device(detector.device_rows(res, image=b), item["gt_ids"], item["gt_table"],
                                               evaluator, **extra)
            if save_ids or save_masks or save_rle or pixel is not None or pan is not None or save_pan or seq is not None:
                file_name = dataset.coco.loadImgs(ids=[item["img_id"]])[0]["file_name"]
                maps = detector.instances(res, image=b)                    # once for the files and the score
                if save_ids or save_masks:
                    save_instances(file_name, maps)
                if save_rle:
                    save_rle_instances(item, file_name, maps, detector.host_rows(res, image=b))
                if seq is not None:                                        # step per image, in the loader's order
                    key, tracked = seq.step(file_name, maps)
                    if save_ids:
                        tracking.save_tracks(maps, tracked, inst_dir, instances_stem(file_name), device_png=device_png)
                    if mots_files is not None:
                        mots_files.add(key, maps, tracked, instances_stem(file_name))
                    if mots is not None:
                        mots.add_maps(key, maps, tracked, item["gt_ids"], file_name)
                if pixel is not None:
                    pixel.add_maps(maps, item["gt_ids"], file_name)
                if pan is not None:
                    pan.add_maps(maps, item["gt_ids"], file_name)               # two calls, nothing comes back
                if save_pan:
                    from centerpoly_amd.datasets.evaluation import panoptic as pan_files
                    from centerpoly_amd.detectors import instances
                    pan_entries.append(pan_files.save_panoptic(maps, pan_dir, instances.image_stem(file_name)))
            stamps.append(time.time())
        print("[{}/{}] ".format(ind, len(images)) + " ".join("|{} {:.3f}s".format(t, avg[t].avg) for t in avg))
    if save_rle:
        import json
        with open(os.path.join(opt.save_dir, "results_segm.json"), "w") as f:
            json.dump(segm, f)
    if not evaluate:
        ap = None
    elif evaluator is None:
        ap = dataset.run_eval(results, opt.save_dir)
    else:
        ap = dataset.finish_scored_eval(results, opt.save_dir, evaluator)
    out = {"ap": ap, "results": results, "dataset": dataset, "stamps": stamps}
    if dist_files is not None and evaluate:
        out.update({k: dataset.last_summary[k] for k in ("allAp100m", "allAp50m", "allAp50%50m")})
    if bnd is not None and evaluate:
        out["boundary"] = bnd.summarize()
        print(boundary.format_results(out["boundary"], protocol))
        boundary.write_results(out["boundary"], opt.save_dir, protocol)
    if pixel is not None and evaluate:
        out["pixel"] = pixel.summarize()
        print(pixel_level.format_results(out["pixel"], pixel.protocol))
        pixel_level.write_results(out["pixel"], opt.save_dir)
    if save_pan:                                                       # before the score, which may refuse the run
        from centerpoly_amd.datasets.evaluation import panoptic as pan_files
        pan_files.write_panoptic_json(pan_dir, pan_entries)
    if pan is not None and evaluate:
        out["panoptic"] = pan.results()
        pan.print_table(out["panoptic"])
        pan.write_json(opt.save_dir, out["panoptic"])
    if mots is not None and evaluate:
        out["tracking"] = mots.results()
        mots.print_table(out["tracking"])
        mots.write_json(opt.save_dir, out["tracking"])
    return out


def test(opt):
    return run_test(opt)["ap"]


if __name__ == "__main__":
    test(opts().parse())

"""Options for the polydet hot path (reference: src/lib/opts.py).

Same flag names, defaults and derived fields as the reference for everything the
path consumes (SURVEY.md section 5 "Config / flags"); flags of other tasks are
not restated.  Fixed here: the undefined `r_variation` (reference :391-396) is a
real option, `--clip_value` has type float (reference :104), the duplicate
`reg` head update is dropped.
"""
import argparse
import os


def chunk_sizes_for(batch_size, master_batch_size, n):
    """Per-replica share of a global batch (reference: src/lib/opts.py:301-310): replica 0 takes
    `master_batch_size` (default batch_size // n), the rest is spread over the others, the first ones
    taking the remainder."""
    master = batch_size // n if master_batch_size == -1 else master_batch_size
    rest = batch_size - master
    sizes = [master]
    for i in range(n - 1):
        chunk = rest // (n - 1)
        if i < rest % (n - 1):
            chunk += 1
        sizes.append(chunk)
    return sizes


class opts(object):
    def __init__(self):
        p = argparse.ArgumentParser()
        p.add_argument("task", default="polydet", nargs="?", help="polydet")
        p.add_argument("--dataset", default="cityscapes",
                       help="cityscapes | kitti_poly | IDD (annotation JSON + images) | synthetic (offline)")
        p.add_argument("--exp_id", default="default")
        p.add_argument("--test", action="store_true")
        p.add_argument("--debug", type=int, default=0,
                       help="detector pictures, rendered on the GPU and written as PNG files into the experiment's "
                            "debug directory: 1 the detections, 2 also the heat-map view and the centre boxes, 4 the "
                            "same (all files); 3 (matplotlib) is refused")
        p.add_argument("--demo", default="", help="demo.py: an image file or a directory of images")
        p.add_argument("--vis_thresh", type=float, default=0.3, help="detections drawn: score above it")
        p.add_argument("--debugger_theme", default="white", choices=["white", "black"])
        p.add_argument("--center_thresh", type=float, default=0.1,
                       help="--debug 2: centres whose boxes the out_pred view shows")
        p.add_argument("--load_model", default="")
        p.add_argument("--resume", action="store_true")
        p.add_argument("--gpus", default="0", help="-1 is rejected: no CPU path")
        p.add_argument("--num_workers", type=int, default=4)
        p.add_argument("--not_cuda_benchmark", action="store_true")
        p.add_argument("--seed", type=int, default=317)
        p.add_argument("--print_iter", type=int, default=0)
        p.add_argument("--hide_data_time", action="store_true")
        p.add_argument("--save_all", action="store_true")
        p.add_argument("--metric", default="loss",
                       help="what picks model_best.pth: a validation loss statistic (loss, hm_l, poly_l, ...; lower "
                            "is better) or `ap`, run_eval's instance-level AP (higher is better; needs --gt_dir)")
        # model
        p.add_argument("--arch", default="dla_34",
                       help="dla_34 | hourglass | smallhourglass")
        p.add_argument("--head_conv", type=int, default=-1)
        p.add_argument("--down_ratio", type=int, default=4)
        p.add_argument("--nbr_points", type=int, default=16)
        p.add_argument("--rep", default="cartesian", choices=["cartesian", "polar", "polar_fixed"])
        p.add_argument("--r_variation", default="none", choices=["none", "one", "two", "four"])
        # input
        p.add_argument("--input_res", type=int, default=-1)
        p.add_argument("--input_h", type=int, default=-1)
        p.add_argument("--input_w", type=int, default=-1)
        # train
        p.add_argument("--lr", type=float, default=4e-6)
        p.add_argument("--lr_step", type=str, default="90,120")
        p.add_argument("--num_epochs", type=int, default=240)
        p.add_argument("--batch_size", type=int, default=32)
        p.add_argument("--master_batch_size", type=int, default=-1)
        p.add_argument("--num_iters", type=int, default=-1)
        p.add_argument("--val_intervals", type=int, default=5)
        p.add_argument("--trainval", action="store_true")
        p.add_argument("--clip", action="store_true")
        p.add_argument("--clip_value", type=float, default=1.0)
        p.add_argument("--root_dir", default="../",
                       help="where exp/<dataset>/<task>/<exp_id> is created (reference: hard-coded ../)")
        p.add_argument("--synthetic_samples", type=int, default=64,
                       help="items per epoch of the synthetic dataset")
        p.add_argument("--device_targets", action="store_true",
                       help="loader workers only pack the raw annotations; heat maps and regression "
                            "targets are built on the GPU (cp_polydet_targets) after the batch upload")
        p.add_argument("--arithmetic", default="split_bf16", choices=["split_bf16", "exact_f32"],
                       help="contraction arithmetic of the convolutions / heads / DCNv2 (centerpoly_amd/arithmetic.py): "
                            "split-bf16 x3 on the bf16 matrix cores (default, ~2^-16 per product) or exact fp32 chains")
        p.add_argument("--no_reorder_flip", action="store_true")
        # sampler augmentation (reference: opts.py "train" group)
        p.add_argument("--not_rand_crop", action="store_true")
        p.add_argument("--shift", type=float, default=0.1)
        p.add_argument("--scale", type=float, default=0.4)
        p.add_argument("--flip", type=float, default=0.5)
        p.add_argument("--no_color_aug", action="store_true")
        p.add_argument("--annot_dir", default="",
                       help="directory of the annotation JSON files (reference: ../<dataset>Stuff/BBoxes)")
        p.add_argument("--img_dir", default="", help="directory of the image files")
        p.add_argument("--bucket_cap_mb", type=int, default=32,
                       help="gradient all-reduce bucket size (RCCL over xGMI)")
        # test
        p.add_argument("--flip_test", action="store_true")
        p.add_argument("--test_scales", type=str, default="1")
        p.add_argument("--nms", action="store_true")
        p.add_argument("--mask_nms", action="store_true",
                       help="merge the test scales by a whole-row, per-class soft-NMS whose overlap is the IoU of the "
                            "polygons' masks, on the GPU (cp_merge_detections_mask): every output row is one detection "
                            "with its own polygon and depth.  Replaces the reference's literal merge of --nms / "
                            "--test_scales a,b, which moves boxes and scores only; implies the merge at one scale too "
                            "and wins over --nms.  At most 1024 rows (scales x K) and 64 classes")
        p.add_argument("--mask_nms_method", default="gaussian", choices=["gaussian", "linear", "hard"],
                       help="--mask_nms: the decay of a row that overlaps a selected one: exp(-ov^2 / 0.5), 1 - ov above "
                            "0.5, or removal above 0.5")
        p.add_argument("--K", type=int, default=128)
        p.add_argument("--thresh", type=float, default=0.05,
                       help="threshold for the outputs kept for evaluation (result writer)")
        p.add_argument("--gt_dir", default="",
                       help="directory searched recursively for <city>_<seq>_<frame>_gtFine_instanceIds.png: with it "
                            "run_eval scores the masks on the GPU (Cityscapes instance-level AP); empty: files only")
        p.add_argument("--no_mask_files", action="store_true",
                       help="with --gt_dir: score in memory and skip the PNG and text output")
        p.add_argument("--device_png", action="store_true",
                       help="compress every mask and id PNG (run_eval's mask files, --save_masks, --save_ids, "
                            "_trackIds.png) on the GPU and read back only the files' bytes: one fixed-Huffman block of "
                            "run-length matches, larger files than PIL's with the same pixels; off: PIL on the host")
        p.add_argument("--save_ids", action="store_true",
                       help="demo.py / test.py: per image <stem>_instanceIds.png (16 bit), <stem>_labelIds.png (8 bit) "
                            "and <stem>.json (the live instances) under <save_dir>/instances/, from the detections "
                            "above --thresh (detector.instances)")
        p.add_argument("--save_masks", action="store_true",
                       help="demo.py / test.py: per image <stem>.txt and masks/<stem>_<k>.png under "
                            "<save_dir>/instances/, the Cityscapes result layout for every data set")
        p.add_argument("--save_rle", action="store_true",
                       help="demo.py / test.py: per image <stem>_rle.json under <save_dir>/instances/, the live instances "
                            "with their masks as COCO run-length strings, encoded on the GPU; test.py also collects "
                            "<save_dir>/results_segm.json (COCO segm results); with --track also "
                            "instances/mots/<sequence>.txt (MOTS text format); not for the synthetic set")
        p.add_argument("--mots_class_map", default="",
                       help="--track --save_rle: label id : class id pairs of the MOTS file, e.g. 26:1,24:2 (KITTI MOTS "
                            "car and pedestrian); a label the map lacks is left out; empty: the label ids themselves")
        p.add_argument("--pixel_iou", action="store_true",
                       help="test.py: also score every image's label map (detector.instances) at pixel level on the "
                            "GPU: class and category IoU and instance-weighted iIoU, the confusion matrix; needs "
                            "--gt_dir; cityscapes and kitti_poly")
        p.add_argument("--panoptic", action="store_true",
                       help="test.py: also score every image's instance map (detector.instances) as a panoptic "
                            "segmentation on the GPU: PQ / SQ / RQ per class and for All / Things / Stuff; needs "
                            "--gt_dir; cityscapes only")
        p.add_argument("--save_panoptic", action="store_true",
                       help="demo.py / test.py: per image <stem>_panoptic.png and one cityscapes_panoptic_val.json in "
                            "COCO panoptic format under <save_dir>/panoptic/, from the detections above --thresh; "
                            "cityscapes only")
        p.add_argument("--boundary", action="store_true",
                       help="test.py: also score the masks by Boundary IoU on the GPU: Boundary AP per class (the AP "
                            "protocol on min(mask IoU, boundary IoU)) beside the plain AP; needs --gt_dir; cityscapes, "
                            "kitti_poly and IDD")
        p.add_argument("--boundary_ratio", type=float, default=0.005,
                       help="--boundary: the band's width as a share of the image diagonal, d = max(1, round(ratio * "
                            "diagonal)), 11 pixels at 2048 x 1024 (0.02 is usual for COCO-sized images); d <= 64")
        p.add_argument("--disparity_dir", default="",
                       help="directory searched recursively for <city>_<seq>_<frame>_disparity.png (16 bit): with it "
                            "(and --camera_dir, --gt_dir) the instance-level AP is also scored within 100 m and 50 m "
                            "(AP_100m, AP_50m), by the median disparity of every ground-truth instance on the GPU; "
                            "cityscapes only")
        p.add_argument("--camera_dir", default="",
                       help="directory searched recursively for <city>_<seq>_<frame>_camera.json (extrinsic.baseline, "
                            "intrinsic.fx); needed with --disparity_dir")
        p.add_argument("--track", action="store_true",
                       help="demo.py / test.py: link the instances (detector.instances) of consecutive frames by the IoU "
                            "of the pixels they own, on the GPU; the frames run in sorted / loader order and one "
                            "sequence is one directory (plus <city>_<seq> of <city>_<seq>_<frame> names).  With "
                            "--save_ids also <stem>_trackIds.png (16 bit, label * multiplier + track id) and "
                            "<stem>_tracks.json; test.py with --gt_dir scores MOTSA / sMOTSA / MOTSP (the ground-truth "
                            "ids must be consistent over a sequence); not for the synthetic set, not with --debug 3")
        p.add_argument("--track_iou", type=float, default=0.3,
                       help="--track: least mask IoU between a track's remembered pixels and an instance of its label, "
                            "finite and in (0, 1]; 0.3 is this project's untuned choice")
        p.add_argument("--track_max_age", type=int, default=0,
                       help="--track: frames a track may go unseen before it ends, >= 0; 0 (a track not seen in a frame "
                            "ends there) is this project's untuned choice")
        p.add_argument("--track_motion", action="store_true",
                       help="--track: compare a track's remembered pixels where the track should be now, moved at the "
                            "velocity between its last two sightings (constant velocity, no smoothing: untuned), on "
                            "the GPU; needs --track and pays off with --track_max_age > 0, where an object that was "
                            "hidden for some frames returns displaced; with --save_ids <stem>_tracks.json also holds "
                            "every track's centroid and velocity")
        p.add_argument("--track_ignore_id", type=int, default=10000,
                       help="--track with --gt_dir: the ground-truth id of the ignore region (10000 in KITTI MOTS)")
        p.add_argument("--not_prefetch_test", action="store_true")
        p.add_argument("--test_batch_size", type=int, default=1,
                       help="test.py: images per network launch (detector.run_batch); 1 keeps the per-image loop. "
                            "Under --keep_res a batch ends where the image size changes; not with --debug > 0")
        p.add_argument("--fix_res", action="store_true")
        p.add_argument("--keep_res", action="store_true")
        # loss
        p.add_argument("--mse_loss", action="store_true")
        p.add_argument("--reg_loss", default="l1")
        p.add_argument("--poly_loss", default="l1", choices=["l1", "iou", "l1+iou", "relu"])
        p.add_argument("--poly_order", action="store_true")
        p.add_argument("--hm_weight", type=float, default=1)
        p.add_argument("--off_weight", type=float, default=1)
        p.add_argument("--poly_weight", type=float, default=1)
        p.add_argument("--depth_weight", type=float, default=0.1)
        p.add_argument("--wh_weight", type=float, default=0.1)
        # task
        p.add_argument("--not_reg_offset", action="store_true")
        p.add_argument("--cat_spec_poly", action="store_true")
        p.add_argument("--dense_poly", action="store_true")
        p.add_argument("--elliptical_gt", action="store_true",
                       help="elliptical centre heat maps, stretched along the longer box side "
                            "(draw_ellipse_gaussian); needs device-built targets")
        # ground truth in place of a head's output, for --test / validation: the AP a perfect head would give (the
        # replaced head gets no gradient)
        for flag, what in (
                ("eval_oracle_hm", "use the ground-truth centre heat map instead of the hm head (hm_l and loss are "
                                   "then NaN for every image with an object, as in the reference)"),
                ("eval_oracle_border_hm", "put the ground-truth border heat map into the outputs (nothing reads it); "
                                          "device-built targets then carry border_hm"),
                ("eval_oracle_offset", "use the ground-truth centre offsets instead of the reg head"),
                ("eval_oracle_poly", "use the ground-truth polygons instead of the poly head (not with "
                                     "--cat_spec_poly)"),
                ("eval_oracle_pseudo_depth", "use the ground-truth depth order instead of the pseudo_depth head")):
            p.add_argument("--" + flag, action="store_true",
                           help=what + "; for --test / validation, an upper bound of the score, not for training")
        self.parser = p

    def parse(self, args=""):
        opt = self.parser.parse_args() if args == "" else self.parser.parse_args(args)
        if opt.elliptical_gt and opt.mse_loss:
            # reference sample/polydet.py:201 replaces the radius by opt.hm_gauss under --mse_loss, an option its
            # opts.py never defines: the combination has no target semantics to follow
            self.parser.error("--elliptical_gt cannot be combined with --mse_loss: the reference sizes --mse_loss "
                              "targets by --hm_gauss, which it never defines")
        if opt.no_mask_files and not opt.gt_dir:
            self.parser.error("--no_mask_files needs --gt_dir: without a ground truth to score against, the mask files "
                              "are the only result of the evaluation")
        if opt.pixel_iou:
            from .datasets.evaluation import pixel_level
            if opt.dataset not in pixel_level.DATASET_PROTOCOL:
                self.parser.error("--pixel_iou scores %s only; dataset %r is refused: %s"
                                  % (" and ".join(sorted(pixel_level.DATASET_PROTOCOL)), opt.dataset,
                                     pixel_level.REFUSED.get(opt.dataset, "it has no pixel-level protocol here")))
            if not opt.gt_dir:
                self.parser.error("--pixel_iou needs --gt_dir: the label maps are scored against the instance-id "
                                  "ground truth found there")
        if opt.panoptic:
            from .datasets.evaluation import panoptic
            if opt.dataset not in panoptic.DATASETS:
                self.parser.error("--panoptic scores %s only; dataset %r is refused: %s"
                                  % (" and ".join(panoptic.DATASETS), opt.dataset,
                                     panoptic.REFUSED.get(opt.dataset, "it has no panoptic protocol here")))
            if not opt.gt_dir:
                self.parser.error("--panoptic needs --gt_dir: the instance maps are scored against the instance-id "
                                  "ground truth found there")
        if opt.boundary:
            import math

            from .datasets.evaluation import boundary
            if opt.dataset not in boundary.DATASETS:
                self.parser.error("--boundary scores %s only; dataset %r is refused: %s"
                                  % (", ".join(boundary.DATASETS), opt.dataset,
                                     "the synthetic set has no ground truth to score against" if opt.dataset == "synthetic"
                                     else "it has no instance-level AP protocol here"))
            if not opt.gt_dir:
                self.parser.error("--boundary needs --gt_dir: the masks are scored against the instance-id ground "
                                  "truth found there")
            if not (math.isfinite(opt.boundary_ratio) and opt.boundary_ratio > 0):
                self.parser.error("--boundary_ratio must be finite and > 0 (got %r)" % opt.boundary_ratio)
        if opt.disparity_dir or opt.camera_dir:
            from .datasets.evaluation import distances
            if not (opt.disparity_dir and opt.camera_dir):
                self.parser.error("--disparity_dir and --camera_dir come together: a disparity becomes a distance "
                                  "through the frame's baseline and focal length")
            if opt.dataset not in distances.DATASETS:
                self.parser.error("--disparity_dir scores %s only; dataset %r is refused: %s"
                                  % (", ".join(distances.DATASETS), opt.dataset,
                                     distances.REFUSED.get(opt.dataset, "it has no instance-level AP protocol here")))
            if not opt.gt_dir:
                self.parser.error("--disparity_dir needs --gt_dir: the distances are those of the ground-truth "
                                  "instances found there")
        if opt.save_panoptic and opt.dataset != "cityscapes":
            self.parser.error("--save_panoptic writes %s only; dataset %r is refused: %s"
                              % ("cityscapes", opt.dataset,
                                 "the synthetic set has no result writer to draw instance maps with"
                                 if opt.dataset == "synthetic" else
                                 "cityscapes_panoptic_<split>.json is the Cityscapes format and carries Cityscapes label "
                                 "ids, which this data set's instances do not have"))
        if opt.save_rle and opt.dataset == "synthetic":
            self.parser.error("--save_rle draws with a data set's result writer; the synthetic set has none (use "
                              "cityscapes, kitti_poly or IDD)")
        try:
            from .detectors.tracking import parse_class_map
            opt.mots_classes = parse_class_map(opt.mots_class_map)
        except ValueError as e:
            self.parser.error(str(e))
        if not (opt.track_iou == opt.track_iou and 0 < opt.track_iou <= 1):
            self.parser.error("--track_iou must be finite and in (0, 1] (got %r)" % opt.track_iou)
        if opt.track_max_age < 0:
            self.parser.error("--track_max_age must be at least 0 (got %d)" % opt.track_max_age)
        if opt.track_motion and not opt.track:
            self.parser.error("--track_motion predicts the tracks of --track: give --track as well")
        if opt.track:
            if opt.dataset == "synthetic":
                self.parser.error("--track links the instance maps a data set's result writer draws; dataset "
                                  "'synthetic' is refused: the synthetic set has no result writer and no sequences")
            if opt.debug == 3:
                self.parser.error("--track cannot be combined with --debug 3: the matplotlib display is not built, the "
                                  "detector would refuse the first frame of the sequence")
        if opt.test_batch_size < 1:
            self.parser.error("--test_batch_size must be at least 1 (got %d)" % opt.test_batch_size)
        if opt.test_batch_size > 1 and opt.debug > 0:
            self.parser.error("--test_batch_size %d cannot be combined with --debug %d: the debug pictures are drawn "
                              "per image by run(); use --test_batch_size 1" % (opt.test_batch_size, opt.debug))
        if opt.metric == "ap":
            from .datasets.dataset_factory import dataset_factory
            if not getattr(dataset_factory.get(opt.dataset), "scores_ap", False):
                self.parser.error("--metric ap: run_eval of dataset %r writes result files and scores nothing, so "
                                  "there is no AP to pick model_best.pth by (cityscapes scores; the others keep a "
                                  "loss statistic)" % opt.dataset)
            if not opt.gt_dir:
                self.parser.error("--metric ap needs --gt_dir: without the *_gtFine_instanceIds.png ground truth "
                                  "run_eval has nothing to score the validation masks against")
        opt.gpus_str = opt.gpus
        from . import arithmetic
        arithmetic.configure(opt.arithmetic)
        opt.gpus = [int(g) for g in opt.gpus.split(",")]
        opt.gpus = [i for i in range(len(opt.gpus))] if opt.gpus[0] >= 0 else [-1]
        opt.lr_step = [int(i) for i in opt.lr_step.split(",")]
        opt.test_scales = [float(i) for i in opt.test_scales.split(",")]
        opt.fix_res = not opt.keep_res
        opt.reg_offset = not opt.not_reg_offset
        if opt.head_conv == -1:
            opt.head_conv = 256 if "dla" in opt.arch else 64
        opt.pad = 127 if "hourglass" in opt.arch else 31
        opt.num_stacks = 2 if opt.arch == "hourglass" else 1
        if opt.trainval:
            opt.val_intervals = 100000000
        opt.master_batch_size_arg = opt.master_batch_size
        opt.chunk_sizes = chunk_sizes_for(opt.batch_size, opt.master_batch_size, len(opt.gpus))
        opt.master_batch_size = opt.chunk_sizes[0]
        opt.root_dir = os.path.join(opt.root_dir)
        opt.data_dir = opt.root_dir
        opt.exp_dir = os.path.join(opt.root_dir, "exp", opt.dataset, opt.task)
        opt.save_dir = os.path.join(opt.exp_dir, opt.exp_id)
        opt.debug_dir = os.path.join(opt.save_dir, "debug")
        if opt.resume and opt.load_model == "":
            path = opt.save_dir[:-4] if opt.save_dir.endswith("TEST") else opt.save_dir
            opt.load_model = os.path.join(path, "model_last.pth")
        return opt

    def update_dataset_info_and_set_heads(self, opt, dataset):
        input_h, input_w = dataset.default_resolution
        opt.mean, opt.std = dataset.mean, dataset.std
        opt.num_classes = dataset.num_classes
        input_h = opt.input_res if opt.input_res > 0 else input_h
        input_w = opt.input_res if opt.input_res > 0 else input_w
        opt.input_h = opt.input_h if opt.input_h > 0 else input_h
        opt.input_w = opt.input_w if opt.input_w > 0 else input_w
        opt.output_h = opt.input_h            # literal: the reference does not divide
        opt.output_w = opt.input_w
        opt.input_res = max(opt.input_h, opt.input_w)
        opt.output_res = max(opt.output_h, opt.output_w)
        if opt.task != "polydet":
            raise AssertionError("task not defined!")
        n_poly = opt.nbr_points * 2
        opt.heads = {"hm": opt.num_classes,
                     "poly": n_poly if not opt.cat_spec_poly else n_poly * opt.num_classes,
                     "pseudo_depth": 1}
        extra = {"one": 1, "two": 2, "four": 4}.get(opt.r_variation)
        if opt.reg_offset:
            opt.heads.update({"reg": 2})
        if extra:
            opt.heads.update({"radius": extra})
        print("heads", opt.heads)
        return opt

    def init(self, args=""):
        class Struct:
            def __init__(self, entries):
                for k, v in entries.items():
                    self.__setattr__(k, v)

        opt = self.parse(args)
        info = {"default_resolution": [512, 1024], "num_classes": 8,
                "mean": [0.284, 0.323, 0.282], "std": [0.04, 0.04, 0.04],
                "dataset": "cityscapes"}
        dataset = Struct(info)
        opt.dataset = dataset.dataset
        return self.update_dataset_info_and_set_heads(opt, dataset)

#!/usr/bin/env python3
"""Demo driver with the reference's CLI (src/demo.py): `python demo.py polydet --demo <image or directory>
--load_model model_last.pth`.  Every image (jpg, jpeg, png, webp; a directory's in sorted order) goes through the
detector with --debug >= 1: the detections are drawn on the GPU and written as `<stem>_polydet.png` into the
experiment's debug directory (--debug 2 adds the heat-map view and the centre boxes).  One timing line per image, as
the reference prints it, with the time of the pictures appended.  `--load_model ''` runs the random initialisation.
--save_ids / --save_masks also write every image's instance maps (detector.instances, drawn by the writer of --dataset
on the image's own canvas from the detections above --thresh) under `<save_dir>/instances/`: `<stem>_instanceIds.png`,
`<stem>_labelIds.png` and `<stem>.json`; `<stem>.txt` and `masks/<stem>_<k>.png`.
--track takes the sorted frames of the directory as one sequence and links their instances (detectors/tracking.py);
with --save_ids it also writes `<stem>_trackIds.png` and `<stem>_tracks.json` there.
--save_rle writes `<stem>_rle.json` there, the live instances with their masks as COCO run-length strings encoded on the
GPU (utils/rle.py), and with --track the sequence's MOTS text file `mots/<the directory's path, joined by _>.txt`.
There is no video decoder here: `webcam` and video files are refused."""
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

image_ext = ["jpg", "jpeg", "png", "webp"]
video_ext = ["mp4", "mov", "avi", "mkv"]
time_stats = ["tot", "load", "pre", "net", "dec", "post", "merge"]


def _ext(name):
    return name[name.rfind(".") + 1:].lower()


def image_names(demo):
    """The files --demo names: the images of a directory in sorted order, or the one file."""
    if demo == "webcam" or _ext(demo) in video_ext:
        raise ValueError("--demo %s: no video decoder is available (cv2 is absent); pass an image file or a "
                         "directory of images" % demo)
    if not demo:
        raise ValueError("--demo needs an image file or a directory of images")
    if os.path.isdir(demo):
        return [os.path.join(demo, f) for f in sorted(os.listdir(demo)) if _ext(f) in image_ext]
    return [demo]


def demo(opt):
    """Runs the detector over opt.demo; returns [(image name, run()'s dict)]."""
    from centerpoly_amd.datasets.dataset_factory import dataset_factory
    from centerpoly_amd.detectors.detector_factory import detector_factory
    from centerpoly_amd.opts import opts
    names = image_names(opt.demo)                            # refusals come before the model is built
    os.environ["CUDA_VISIBLE_DEVICES"] = opt.gpus_str
    opt.debug = max(opt.debug, 1)
    opt = opts().update_dataset_info_and_set_heads(opt, dataset_factory[opt.dataset])
    detector = detector_factory[opt.task](opt)
    out = []
    pan_entries = []
    seq = None
    if getattr(opt, "track", False):
        from centerpoly_amd.detectors import tracking
        seq = tracking.SequenceTracker(opt.track_iou, opt.track_max_age, getattr(opt, "track_motion", False))
    save_rle, mots_files = getattr(opt, "save_rle", False), None
    device_png = getattr(opt, "device_png", False)
    for name in names:
        ret = detector.run(name)
        print("".join("{} {:.3f}s |".format(stat, ret[stat]) for stat in time_stats)
              + "vis {:.3f}s |".format(ret["vis_time"]))
        if opt.save_ids or opt.save_masks or save_rle or seq is not None:
            from centerpoly_amd.detectors import instances
            maps = detector.instances(ret["results"])
            inst_dir, stem = os.path.join(opt.save_dir, "instances"), instances.image_stem(name)
            if seq is not None:                                  # the directory is one sequence
                key, ret["tracked"] = seq.step(os.path.join(os.path.dirname(name), "frame"), maps)
                if save_rle:
                    if mots_files is None:
                        mots_files = tracking.MotsWriter(inst_dir, getattr(opt, "mots_classes", None))
                    mots_files.add(key, maps, ret["tracked"], stem)
                if opt.save_ids:
                    tracking.save_tracks(maps, ret["tracked"], inst_dir, stem, device_png=device_png)
            if opt.save_ids:
                instances.save_ids(maps, inst_dir, stem, device_png=device_png)
            if opt.save_masks:
                instances.save_masks(maps, inst_dir, stem, device_png=device_png)
            if save_rle:
                instances.save_rle(maps, inst_dir, stem)
        if getattr(opt, "save_panoptic", False):
            from centerpoly_amd.datasets.evaluation import panoptic
            from centerpoly_amd.detectors import instances
            pan_dir = os.path.join(opt.save_dir, "panoptic")
            pan_entries.append(panoptic.save_panoptic(detector.instances(ret["results"]), pan_dir,
                                                      instances.image_stem(name)))
        out.append((name, ret))
    if pan_entries:
        panoptic.write_panoptic_json(pan_dir, pan_entries)
    return out


if __name__ == "__main__":
    from centerpoly_amd.opts import opts
    demo(opts().parse())

#!/usr/bin/env python3
"""Makes the annotation files the data sets open (`train<N>_regular_interval.json`, `train<N>.json`, `val<N>...json`,
`test.json`) from a data set's own ground truth, with the "regular interval" recipe of the reference's offline tools
(KITTIPolyStuff/Tools/create_annotations.py, cityscapesStuff/Tools/create_bouding_box_annotations.py,
IDDStuff/Tools/create_annotations.py followed by src/tools/convert_csv_to_coco.py) run on the GPU:

    python make_annotations.py --dataset cityscapes --split train --nbr_points 16 32 64 \\
        --img_dir cityscapes/leftImg8bit/train --gt_dir cityscapes/gtFine/train --out_dir cityscapesStuff/BBoxes
    python make_annotations.py --dataset kitti_poly --split train --nbr_points 32 \\
        --img_dir KITTIPoly/training/image_2 --gt_dir KITTIPoly/training/instance --out_dir KITTIPolyStuff/BBoxes

--img_dir holds the split's images: `<city>/<frame>_leftImg8bit.png` (Cityscapes, IDD) or `<frame>.png` (KITTI), taken
in sorted order.  --gt_dir holds the ground truth beside them: `<city>/<frame>_gtFine_polygons.json` for --source
polygons (the recipe of Cityscapes and IDD), the 16-bit instance image for --source ids (the recipe of KITTI:
`<frame>.png`; `<city>/<frame>_gtFine_instanceIds.png` for Cityscapes, `..._instanceids.png` for IDD).  A KITTI
`--split train` (or val) run writes train<N>.json, val<N>.json (every 20th image) and trainval<N>.json, as the tool
does.  `--split test` needs no ground truth: one placeholder row per image.  The files are written into --out_dir
under the names `annot_file()` of the data set expects; pass that directory to main.py / test.py as --annot_dir.
Decoding runs in --num_workers DataLoader workers ahead of the device."""
import argparse
import glob
import json
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

DATASETS = ("cityscapes", "kitti_poly", "IDD")
DEFAULT_SOURCE = {"cityscapes": "polygons", "kitti_poly": "ids", "IDD": "polygons"}
DEFAULT_DIVISOR = {"cityscapes": 1000, "kitti_poly": 256, "IDD": 1000}
CITYSCAPES_CANVAS = (2048, 1024)
IMAGE_SUFFIX = "_leftImg8bit.png"


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="training annotations from ground truth, on the GPU")
    p.add_argument("--dataset", required=True, choices=DATASETS)
    p.add_argument("--source", choices=("polygons", "ids"), default=None,
                   help="default: polygons for cityscapes and IDD, ids for kitti_poly")
    p.add_argument("--img_dir", required=True)
    p.add_argument("--gt_dir", default="")
    p.add_argument("--split", choices=("train", "val", "test"), default="train")
    p.add_argument("--nbr_points", type=int, nargs="+", default=[16])
    p.add_argument("--out_dir", required=True)
    p.add_argument("--id_divisor", type=int, default=None,
                   help="an id image holds label * divisor + k; default 256 for kitti_poly, 1000 for cityscapes and IDD")
    p.add_argument("--num_workers", type=int, default=4)
    p.add_argument("--gpu", type=int, default=0)
    opt = p.parse_args(argv)
    from centerpoly_amd.datasets.annotate import check_nbr_points
    try:
        opt.nbr_points = check_nbr_points(opt.nbr_points)
    except ValueError as e:
        p.error(str(e))
    if len(set(opt.nbr_points)) != len(opt.nbr_points):
        p.error("--nbr_points names a value twice")
    opt.source = opt.source or DEFAULT_SOURCE[opt.dataset]
    if opt.dataset == "kitti_poly" and opt.source == "polygons":
        p.error("kitti_poly has no polygon files: use --source ids")
    opt.id_divisor = DEFAULT_DIVISOR[opt.dataset] if opt.id_divisor is None else opt.id_divisor
    if opt.id_divisor < 1:
        p.error("--id_divisor must be positive")
    if opt.split != "test" and not opt.gt_dir:
        p.error("--gt_dir is needed for the %s split" % opt.split)
    return opt


def dataset_class(name):
    from centerpoly_amd.datasets.dataset import polygons
    return {"cityscapes": polygons.CITYSCAPES, "kitti_poly": polygons.KITTIPOLY, "IDD": polygons.IDD}[name]


def output_names(dataset, split, nbr_points):
    """{part: file name} of one run at one N, part in train / val / trainval / test: what annot_file() opens."""
    import types
    cls = dataset_class(dataset)
    ds = cls.__new__(cls)
    ds.opt = types.SimpleNamespace(nbr_points=nbr_points)
    if split == "test":
        return {"test": ds.annot_file("test")}
    if dataset == "kitti_poly":
        return {"train": ds.annot_file("train"), "val": ds.annot_file("val"), "trainval": "trainval%d.json" % nbr_points}
    return {split: ds.annot_file(split)}


def image_list(dataset, img_dir):
    pattern = os.path.join(img_dir, "*.png") if dataset == "kitti_poly" else os.path.join(img_dir, "*", "*.png")
    names = sorted(glob.glob(pattern))
    if not names:
        raise FileNotFoundError("no images match %s" % pattern)
    return names


def gt_path(opt, image_path):
    """The ground-truth file of an image: same place below --gt_dir, the data set's suffix."""
    from centerpoly_amd.datasets.evaluation import instance_level
    rel = os.path.relpath(image_path, opt.img_dir)
    if opt.dataset == "kitti_poly":
        return os.path.join(opt.gt_dir, rel)
    if not rel.endswith(IMAGE_SUFFIX):
        raise ValueError("%s does not end in %s" % (image_path, IMAGE_SUFFIX))
    suffix = "_gtFine_polygons.json" if opt.source == "polygons" else \
        (instance_level.IDD_GT_SUFFIX if opt.dataset == "IDD" else instance_level.GT_SUFFIX)
    return os.path.join(opt.gt_dir, rel[:-len(IMAGE_SUFFIX)] + suffix)


class GroundTruth(object):
    """One item per image, decoded on the host only (DataLoader workers): the polygon file's objects and the
    canvas, or the 16-bit id image."""

    def __init__(self, opt, names):
        self.opt, self.names = opt, names

    def __len__(self):
        return len(self.names)

    def __getitem__(self, ind):
        from centerpoly_amd.datasets.evaluation import instance_level
        opt, path = self.opt, self.names[ind]
        item = {"path": os.path.abspath(path)}
        if opt.split == "test":
            return item
        gt = gt_path(opt, path)
        if not os.path.isfile(gt):
            raise FileNotFoundError("ground truth %s of image %s not found" % (gt, path))
        if opt.source == "ids":
            item["ids"] = instance_level.read_gt_ids(gt)
        else:
            with open(gt) as f:
                item["objects"] = json.load(f)["objects"]
            if opt.dataset == "cityscapes":
                item["canvas"] = CITYSCAPES_CANVAS
            else:
                from PIL import Image
                with Image.open(path) as im:
                    item["canvas"] = im.size
        return item


def run(opt):
    """Writes the files; returns {file name: (images, annotations)}."""
    import numpy as np
    import torch

    from centerpoly_amd.datasets import annotate, eval_images
    cls = dataset_class(opt.dataset)
    class_names = list(cls.class_name[1:1 + cls.num_classes])
    names = image_list(opt.dataset, opt.img_dir)
    counts = opt.nbr_points
    written = {}
    if opt.split == "test":
        images = [(os.path.abspath(p), [annotate.placeholder_row()]) for p in names]
        out = os.path.join(opt.out_dir, output_names(opt.dataset, "test", counts[0])["test"])
        written[out] = annotate.write_annotations(out, images, class_names)
        print("%s: %d images, %d annotations" % ((out,) + written[out]))
        return written
    if not torch.cuda.is_available():
        raise RuntimeError("make_annotations.py needs a HIP device: the recipe runs on the GPU, there is no CPU path")
    dev = torch.device("cuda", opt.gpu)
    if opt.source == "ids":
        labels = [cls.label_to_id[c] for c in class_names if cls.label_to_id[c] >= 0]
        label_names = [c for c in class_names if cls.label_to_id[c] >= 0]
    else:
        have_instances = list(cls.class_name[1:])
    per_image = {N: [] for N in counts}                          # N -> [(path, rows)] in image order
    frequencies, max_objects = {}, 0
    items = eval_images.iterate(GroundTruth(opt, names), opt.num_workers > 0, opt.num_workers)
    for item in items:
        if opt.source == "ids":
            ids_dev = torch.from_numpy(item["ids"].view(np.int16)).to(dev)
            res = annotate.from_id_image(ids_dev, labels, opt.id_divisor, counts)
            obj_labels = [label_names[c] for c in res["cls"]]
        else:
            res = annotate.from_polygons(item["objects"], item["canvas"], have_instances, counts, device=dev,
                                         what=item["path"])
            obj_labels = res["label"]
        for label in obj_labels:
            frequencies[label] = frequencies.get(label, 0) + 1
        max_objects = max(max_objects, len(obj_labels))
        for N in counts:
            rows = [(res["bbox"][k], obj_labels[k], int(res["pseudo_depth"][k]), res["poly"][N][k])
                    for k in range(len(obj_labels))]
            per_image[N].append((item["path"], rows))
    for N in counts:
        files = output_names(opt.dataset, opt.split, N)
        images = per_image[N]
        if opt.source == "ids":
            # the id recipe writes no row for an image without an object: it is not in the file (and still counts
            # for the split)
            numbered = [(k + 1, im) for k, im in enumerate(images)]
            parts = {"trainval": [im for _, im in numbered if im[1]]}
            parts["val"] = [im for k, im in numbered if im[1] and annotate.kitti_val_image(k)]
            parts["train"] = [im for k, im in numbered if im[1] and not annotate.kitti_val_image(k)]
            if opt.dataset != "kitti_poly":
                parts = {opt.split: parts["trainval"]}
        else:
            parts = {opt.split: images}
        for part, file_name in files.items():
            out = os.path.join(opt.out_dir, file_name)
            written[out] = annotate.write_annotations(out, parts[part], class_names)
            print("%s: %d images, %d annotations" % ((out,) + written[out]))
    print("max objects: ", max_objects)
    print(frequencies)
    return written


if __name__ == "__main__":
    run(parse_args())

#!/usr/bin/env python3
"""Makes the ground-truth id images of a data set from its polygon files, as the evaluators' preparation scripts do
(IDDscripts/preperation/createLabels.py with json2instanceImg.py and json2labelImg.py; cityscapesscripts/preparation/
json2instanceImg.py, json2labelImg.py, createTrainIdInstanceImgs.py and createTrainIdLabelImgs.py), drawn on the GPU:

    python make_ground_truth.py --dataset IDD --gt_dir IDD_Segmentation/gtFine/val
    python make_ground_truth.py --dataset cityscapes --gt_dir cityscapes/gtFine/val --labels --out_dir gt/val

--gt_dir is walked recursively for `*_polygons.json`, in sorted order.  Beside each file (or below --out_dir, under
the same city directory) the run writes the 16-bit instance image and, with --labels, the 8-bit label image, under the
scripts' own names: `<stem>_instance<id_type>s.png` / `<stem>_label<id_type>s.png` for IDD (--id_type id, the default,
gives `..._gtFine_instanceids.png`, the file `test.py --gt_dir` scores against), `<stem>_instanceIds.png` /
`<stem>_labelIds.png` for Cityscapes (`...TrainIds.png` with --id_type trainIds).  --no_instance leaves the instance
image out.  The colour images, the panoptic output and the domain-adaptation subsets of createLabels.py are not made.
The JSON is parsed and the list of polygons to draw is made in --num_workers DataLoader workers ahead of the device;
the same number of threads compresses the PNGs behind it.  With --device_png the painted image is compressed on the
GPU before it leaves the device (centerpoly_amd/utils/png.py) and the threads only write the files' bytes."""
import argparse
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

DATASETS = ("IDD", "cityscapes")
JSON_SUFFIX = "_polygons.json"
SIZE_KEYS = ("imgWidth", "imgHeight")


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="ground-truth id images from polygon files, on the GPU")
    p.add_argument("--dataset", required=True, choices=DATASETS)
    p.add_argument("--gt_dir", required=True, help="walked recursively for *_polygons.json")
    p.add_argument("--out_dir", default="", help="default: beside each JSON file")
    p.add_argument("--id_type", default=None,
                   help="IDD: id (default), csId, csTrainId, level4Id .. level1Id; cityscapes: ids (default), trainIds")
    p.add_argument("--no_instance", action="store_true", help="do not write the instance image")
    p.add_argument("--labels", action="store_true", help="also write the label image")
    p.add_argument("--num_workers", type=int, default=4)
    p.add_argument("--device_png", action="store_true",
                   help="compress the PNGs on the GPU (larger files, same pixels); the threads then only write bytes")
    p.add_argument("--gpu", type=int, default=0)
    opt = p.parse_args(argv)
    from centerpoly_amd.datasets import ground_truth
    encodings = ground_truth.TABLES[opt.dataset][1]
    opt.id_type = ground_truth.DEFAULT_ENCODING[opt.dataset] if opt.id_type is None else opt.id_type
    if opt.id_type not in encodings:
        p.error("--id_type %s: %s has %s" % (opt.id_type, opt.dataset, ", ".join(encodings)))
    if opt.no_instance and not opt.labels:
        p.error("--no_instance without --labels leaves nothing to write")
    if opt.num_workers < 0:
        p.error("--num_workers must not be negative")
    return opt


def output_names(dataset, id_type, stem):
    """(instance image, label image) file names of a JSON whose name is stem + `_polygons.json`."""
    if dataset == "IDD":                                       # createLabels.py:32 and :42-43
        return "%s_instance%ss.png" % (stem, id_type), "%s_label%ss.png" % (stem, id_type)
    tag = "Ids" if id_type == "ids" else "TrainIds"            # createTrainIdInstanceImgs.py / createTrainIdLabelImgs.py
    return "%s_instance%s.png" % (stem, tag), "%s_label%s.png" % (stem, tag)


def frame_key(dataset, path):
    """What the scoring side calls the frame of a file: `<city>/<frame>` for IDD (the name up to its first `_`),
    `<city>/<name up to _gt...>` for Cityscapes."""
    city, name = os.path.basename(os.path.dirname(path)), os.path.basename(path)
    if dataset == "IDD":
        return city + "/" + name.split("_")[0]
    stem = name[:-len(JSON_SUFFIX)]
    cut = stem.rfind("_gt")
    return city + "/" + (stem[:cut] if cut > 0 else stem)


def frame_list(dataset, gt_dir):
    """The polygon files below gt_dir, sorted; none at all, or two for one frame, is an error that names them."""
    if not os.path.isdir(gt_dir):
        raise FileNotFoundError("--gt_dir %s is not a directory" % gt_dir)
    names = []
    for root, dirs, files in os.walk(gt_dir):
        dirs.sort()
        names += [os.path.join(root, f) for f in files if f.endswith(JSON_SUFFIX)]
    names.sort()
    if not names:
        raise FileNotFoundError("no *%s below %s" % (JSON_SUFFIX, gt_dir))
    seen = {}
    for path in names:
        key = frame_key(dataset, path)
        if key in seen:
            raise ValueError("two polygon files for the frame %s: %s and %s" % (key, seen[key], path))
        seen[key] = path
    return names


def read_frame(path):
    """(objects, (width, height)) of a polygon file; a missing size is an error that names the file."""
    with open(path) as f:
        d = json.load(f)
    for key in SIZE_KEYS + ("objects",):
        if not isinstance(d, dict) or key not in d:
            raise ValueError("%s has no %s" % (path, key))
    return d["objects"], (int(d["imgWidth"]), int(d["imgHeight"]))


def check_size_fields(path):
    """The first pass, before the device does anything: the file's text must name both size fields.  This is a scan
    of the text, so that no file is parsed twice; a file that names a field only inside a nested object or a string
    passes it and is refused by `read_frame` when its turn comes, after the frames before it were drawn."""
    with open(path) as f:
        text = f.read()
    for key in SIZE_KEYS:
        if not re.search(r'"%s"\s*:' % key, text):
            raise ValueError("%s has no %s" % (path, key))


class Frames(object):
    """One item per polygon file, made on the host only (DataLoader workers): the file parsed and, for every image
    that is asked for, the polygons and values to draw."""

    def __init__(self, names, dataset, id_type, kinds):
        self.names, self.dataset, self.id_type, self.kinds = names, dataset, id_type, kinds

    def __len__(self):
        return len(self.names)

    def __getitem__(self, ind):
        from centerpoly_amd.datasets import ground_truth
        path = self.names[ind]
        objects, canvas = read_frame(path)
        lists = [ground_truth.paint_list(objects, self.dataset, kind, self.id_type, what=path) for kind in self.kinds]
        return {"path": path, "canvas": canvas, "lists": lists}


def output_dir(opt, path):
    if not opt.out_dir:
        return os.path.dirname(path)
    rel = os.path.relpath(os.path.dirname(path), opt.gt_dir)
    return os.path.normpath(os.path.join(opt.out_dir, rel))


def write_bytes(path, data):
    with open(path, "wb") as f:
        f.write(data)


def run(opt):
    """Writes the images; returns the list of files written, in frame order."""
    from concurrent.futures import ThreadPoolExecutor

    import torch

    from centerpoly_amd.datasets import eval_images, ground_truth
    from centerpoly_amd.utils import png
    names = frame_list(opt.dataset, opt.gt_dir)
    for path in names:
        check_size_fields(path)
    if not torch.cuda.is_available():
        raise RuntimeError("make_ground_truth.py needs a HIP device: the images are drawn on the GPU, there is no CPU path")
    dev = torch.device("cuda", opt.gpu)
    kinds = ([] if opt.no_instance else [("instance", 0, 16)]) + ([("label", 1, 8)] if opt.labels else [])
    frames = Frames(names, opt.dataset, opt.id_type, [k for k, _, _ in kinds])
    written, pending = [], []
    with torch.cuda.device(dev):                               # the library launches on the current device's stream
        with ThreadPoolExecutor(max_workers=max(1, opt.num_workers)) as pool:
            for item in eval_images.iterate(frames, opt.num_workers > 0, opt.num_workers):
                path = item["path"]
                stem = os.path.basename(path)[:-len(JSON_SUFFIX)]
                out_dir = output_dir(opt, path)
                os.makedirs(out_dir, exist_ok=True)
                files = output_names(opt.dataset, opt.id_type, stem)
                for (kind, which, bits), (polygons, values, background) in zip(kinds, item["lists"]):
                    image = ground_truth.paint(polygons, values, background, item["canvas"], dev)
                    out = os.path.join(out_dir, files[which])
                    if getattr(opt, "device_png", False):
                        data = png.encode(images=image, bits=bits, names=[out])[0]
                        pending.append(pool.submit(write_bytes, out, data))
                    else:
                        pending.append(pool.submit(ground_truth.write_id_png, out, image.cpu().numpy(), bits))
                    written.append(out)
                while len(pending) > 4 * max(1, opt.num_workers):   # a bounded queue of images that wait for a thread
                    pending.pop(0).result()
            for job in pending:
                job.result()
    print("%d frames, %d images written" % (len(names), len(written)))
    return written


if __name__ == "__main__":
    run(parse_args())

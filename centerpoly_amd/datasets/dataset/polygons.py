"""The reference's polygon datasets (src/lib/datasets/dataset/{cityscapes,kitti_poly,IDD}.py) without
pycocotools / cv2: the annotation files are plain COCO-style JSON (`images`, `annotations` with `bbox`
[x, y, w, h], `poly` [2N numbers], `category_id`, `pseudo_depth`; `categories`), indexed here with the
`json` module; images are read with PIL and handed on as 8-bit BGR arrays (what `cv2.imread` returns).

Constants (class lists, class frequencies, mean / std, default resolution, colour-augmentation PCA)
are the datasets' own.  Paths: the reference hard-codes `../cityscapesStuff/BBoxes` etc. relative to
`src/`; here `--annot_dir` / `--data_dir` say where the JSON files and the images are, and a missing
file is an error that names the path -- no silent substitution by synthetic data."""
import json
import os

import numpy as np
import torch.utils.data as data


class CocoIndex(object):
    """The four pycocotools.coco.COCO calls the sampler uses (sample/polydet.py:69-77)."""

    def __init__(self, annot_path):
        with open(annot_path) as f:
            d = json.load(f)
        self.imgs = {im["id"]: im for im in d["images"]}
        self.anns = {a["id"]: a for a in d["annotations"]}
        self.cats = {c["id"]: c for c in d.get("categories", [])}
        self._by_img = {}
        for a in d["annotations"]:
            self._by_img.setdefault(a["image_id"], []).append(a["id"])

    def getImgIds(self):
        return list(self.imgs.keys())

    def loadImgs(self, ids):
        return [self.imgs[i] for i in ids]

    def getAnnIds(self, imgIds):
        return [a for i in imgIds for a in self._by_img.get(i, [])]

    def loadAnns(self, ids):
        return [self.anns[i] for i in ids]


class PolygonDataset(data.Dataset):
    num_classes = 8
    default_resolution = [512, 1024]
    max_objs = 128
    # PCA of the colour augmentation (identical in the three dataset files)
    _eig_val = np.array([0.2141788, 0.01817699, 0.00341571], dtype=np.float32)
    _eig_vec = np.array([[-0.58752847, -0.69563484, 0.41340352], [-0.5832747, 0.00994535, -0.81221408],
                         [-0.56089297, 0.71832671, 0.41158938]], dtype=np.float32)
    class_name = ["__background__", "person", "rider", "car", "truck", "bus", "train", "motorcycle", "bicycle"]
    _valid_ids = [1, 2, 3, 4, 5, 6, 7, 8]
    annot_subdir = ""
    name = ""
    scores_ap = False                                        # run_eval writes results.json and scores nothing

    def annot_file(self, split):
        raise NotImplementedError

    def __init__(self, opt, split):
        super(PolygonDataset, self).__init__()
        self.opt = opt
        self.split = split
        annot_dir = getattr(opt, "annot_dir", "") or os.path.join(opt.data_dir, self.annot_subdir)
        self.annot_path = os.path.join(annot_dir, self.annot_file(split))
        self.img_dir = getattr(opt, "img_dir", "") or os.path.join(opt.data_dir, self.name, "images")
        if not os.path.isfile(self.annot_path):
            raise FileNotFoundError(
                "dataset %r (%s split): annotation file %s not found -- pass --annot_dir / --data_dir, or use "
                "--dataset synthetic for the offline synthetic set" % (self.name, split, self.annot_path))
        self.cat_ids = {v: i for i, v in enumerate(self._valid_ids)}
        self._data_rng = np.random.RandomState(123)
        print("==> initializing %s %s data." % (self.name, split))
        self.coco = CocoIndex(self.annot_path)
        self.images = self.coco.getImgIds()
        self.num_samples = len(self.images)
        print("Loaded {} {} samples".format(split, self.num_samples))

    def __len__(self):
        return self.num_samples

    def read_image(self, file_name):
        """8-bit BGR [H, W, 3] (cv2.imread's layout).  Absolute paths of the annotation files are
        re-rooted under img_dir by their base name when they do not exist as given."""
        from PIL import Image
        path = file_name if os.path.isabs(file_name) and os.path.exists(file_name) else \
            os.path.join(self.img_dir, os.path.basename(file_name))
        if not os.path.exists(path):
            raise FileNotFoundError("image %s not found (img_dir %s)" % (file_name, self.img_dir))
        return np.ascontiguousarray(np.asarray(Image.open(path).convert("RGB"))[:, :, ::-1])

    def run_eval(self, results, save_dir):
        """The vendored evaluators (cityscapesscripts, pycocotools) are outside the accelerated path: the
        detections are written in the reference's json layout (convert_polygon_eval_format) for them."""
        dets = []
        for image_id, per_cls in results.items():
            for cls_ind, rows in per_cls.items():
                for row in rows:
                    dets.append({"image_id": int(image_id), "category_id": int(self._valid_ids[cls_ind - 1]),
                                 "bbox": [float("%.2f" % v) for v in row[0:4]], "score": float("%.2f" % row[4]),
                                 "polygon": [float("%.2f" % v) for v in row[5:-1]],
                                 "depth": float(row[-1])})
        os.makedirs(save_dir, exist_ok=True)
        with open(os.path.join(save_dir, "results.json"), "w") as f:
            json.dump(dets, f)
        print("%s: wrote %d detections to %s/results.json" % (self.name, len(dets), save_dir))
        return 0.0

    def report_eval(self, evaluator, res_dir):
        """The evaluator's table on the screen, its JSON below res_dir; returns allAp (the whole dictionary stays in
        last_summary: with distances it holds allAp100m, allAp50m and allAp50%50m too)."""
        from ..evaluation import instance_level
        self.last_evaluator = evaluator
        res = self.last_summary = evaluator.summarize()
        print(instance_level.format_results(res, evaluator.protocol))
        out_dir = os.path.join(res_dir, "evaluationResults")
        os.makedirs(out_dir, exist_ok=True)
        with open(os.path.join(out_dir, "resultInstanceLevelSemanticLabeling.json"), "w") as f:
            json.dump(instance_level.results_json(res, evaluator.protocol), f, indent=4)
        return res["allAp"]


def _to_float(x):
    return float("{:.2f}".format(x))


class CityscapesWriterMixin(object):
    """format_and_write_to_cityscapes (src/lib/datasets/dataset/cityscapes.py:196-283): per image a text
    file `<image>.txt` listing `masks/<image>_<k>.png <label id> <confidence>` and the instance masks as
    8-bit PNG files, instances processed in ascending depth, nearer confident ones hiding farther ones.
    The masks are rasterised on the GPU (cp_instance_masks); selection, ordering, naming and the file
    output (PIL, like the reference) stay on the host."""
    canvas = (2048, 1024)                                    # (width, height), hard-coded by the reference
    no_mask_labels = ("pole", "traffic sign", "traffic light")

    def image_instances(self, per_class):
        params = []
        for cls_ind in per_class:
            if cls_ind == "fg":
                continue
            for row in per_class[cls_ind]:
                if row[4] > self.opt.thresh:
                    poly = [_to_float(v) for v in row[5:-1]]
                    pts = [(int(x), int(y)) for x, y in zip(poly[0::2], poly[1::2])]
                    params.append((pts, row[4], self.class_name[cls_ind], row[-1]))
        return sorted(params, key=lambda a: a[-1])

    def instance_masks_device(self, params, device=None):
        """Occlusion-ordered masks of depth-sorted instances, left on the device:
        (uint8 [n, H, W] tensor, int32 [n] tensor of pixel counts)."""
        import torch

        from ... import _C
        W, H = self.canvas
        n = len(params)
        if n == 0:                                           # nothing to draw: no device needed (or touched)
            return torch.zeros((0, H, W), dtype=torch.uint8), torch.zeros((0,), dtype=torch.int32)
        dev = device or torch.device("cuda")
        if n > 128:
            raise ValueError("more than 128 instances in one image (max_per_image = K <= 128)")
        N = len(params[0][0])
        poly = torch.tensor([p[0] for p in params], dtype=torch.int32).reshape(n, N, 2).to(dev)
        flags = torch.tensor([(0 if p[2] in self.no_mask_labels else 1) | (2 if p[1] >= 0.5 else 0) for p in params],
                             dtype=torch.uint8).to(dev)
        masks = torch.empty((n, H, W), dtype=torch.uint8, device=dev)
        counts = torch.empty((n,), dtype=torch.int32, device=dev)
        _C.check(_C.lib().cp_instance_masks(_C.ptr(poly), _C.ptr(flags), n, N, H, W, _C.ptr(masks), _C.ptr(counts),
                                            _C.stream()), "cp_instance_masks")
        return masks, counts

    def instance_masks(self, params, device=None):
        """Occlusion-ordered masks of depth-sorted instances: (uint8 [n, H, W] host array, counts [n])."""
        masks, counts = self.instance_masks_device(params, device)
        return masks.cpu().numpy(), counts.cpu().numpy()

    def class_table(self):
        """cp_writer_instances' table: int32 [C, 2] rows (label id, label has masks) of class 0 .. C-1."""
        return self.writer_class_table()

    @classmethod
    def writer_class_table(cls):
        """class_table without an object: the table comes from the class's names and label ids alone (demo.py has no
        annotation file to construct a data set from)."""
        names = cls.class_name[1:]
        return np.array([[cls.label_to_id[c], 0 if c in cls.no_mask_labels else 1] for c in names], np.int32)

    def score_instances_device(self, rows_dev, gt_ids, gt_table=None, evaluator=None, boundary=None, distances=None):
        """One image scored from its detection rows without a pass through host Python: device float32 rows
        [R, 2N + 7] in the layout cp_polydet_post_process writes (x1,y1,x2,y2,score,cls,poly,depth; R <= 1024)
        -> cp_writer_instances -> cp_instance_masks -> cp_instance_overlaps on all slots, then ONE read of the small
        tables.  gt_ids: host uint16 [H, W] (see read_gt_ids) or a device tensor of 16-bit elements; gt_table: what
        instance_level.gt_instances gives for it (a loader worker can make it from np.bincount), by default taken
        from cp_id_histogram.  The writer's selection (label has masks, more than 100 pixels) is applied to the rows
        of the tables; with an `evaluator` the kept rows are added to it (add_counts).  Returns the tables:
        n, src, labels, conf (float32), conf_text, counts, kept, gt_table, inter, void.
        boundary: an evaluation.boundary.BoundaryEvaluator, or None.  With one, the masks also go through
        cp_boundary_overlaps (bounds: the polygons' boxes grown by the writer's radius-2 dilation); the band tables come
        back in the same read, are returned as b_inter, b_pred, b_gt and band_width, and the kept rows are added to it.
        distances: (disparity, camera) of the image -- a host uint16 [H, W] array or a device tensor of 16-bit elements,
        and (baseline, fx) -- or None.  With it the ground-truth table's ids go through cp_segment_medians on the id
        image (evaluation/distances.py); the integers come back in the same read, the [G, 2] table (medDist, distConf)
        is returned as gt_dist (gt_dist_raw: the integers) and goes to the evaluators as add_counts' gt_dist."""
        import ctypes

        import torch

        from ... import _C
        from ..evaluation import instance_level as il
        W, H = self.canvas
        if rows_dev.dim() != 2 or rows_dev.dtype != torch.float32 or rows_dev.shape[1] < 13 or rows_dev.shape[1] % 2 == 0:
            raise ValueError("rows must be float32 [R, 2N + 7], got %s %s" % (rows_dev.dtype, tuple(rows_dev.shape)))
        dev = rows_dev.device
        R, N = int(rows_dev.shape[0]), (int(rows_dev.shape[1]) - 7) // 2
        if R == 0:                                                         # no detection at all: one dead row
            rows_dev = torch.full((1, 2 * N + 7), float("-inf"), dtype=torch.float32, device=dev)
            R = 1
        S = min(R, il.MAX_MASKS)                                          # slots drawn and counted
        gt_dev = il.device_ids(gt_ids, dev)
        if tuple(gt_dev.shape) != (H, W):
            raise ValueError("the id image is %s, the result canvas is %s" % (tuple(gt_dev.shape), (H, W)))
        if gt_table is None:
            gt_table = il.gt_instances(il.device_histogram(gt_dev))
        gt_table = np.asarray(gt_table, np.int64).reshape(-1, 3)
        G = len(gt_table)
        G0 = min(G, il.MAX_INST)
        L = _C.lib()
        table = np.ascontiguousarray(self.class_table())
        # one upload: the ids of interest and the void ids; one buffer for everything that comes back
        ids = torch.from_numpy(np.concatenate([gt_table[:G0, 0], il.VOID_IDS]).astype(np.int32)).to(dev)
        fw = (R + 3) // 4
        o_band = 4 + 3 * R + 3 * S + fw + S * G0                          # the band tables, after everything else
        if boundary is not None:
            from ...detectors import instances
            from ..evaluation import boundary as bd
            band_d = boundary.band_width(H, W)
        o_med = o_band + (bd.table_words(S, G0) if boundary is not None else 0)   # the median integers, last
        out = torch.empty((o_med + (4 * G0 if distances is not None else 0),), dtype=torch.int32, device=dev)
        o_src, o_lab, o_conf = 4, 4 + R, 4 + 2 * R
        o_cnt = 4 + 3 * R
        o_void, o_pix, o_flag, o_int = o_cnt + S, o_cnt + 2 * S, o_cnt + 3 * S, o_cnt + 3 * S + fw
        poly = torch.empty((R, N, 2), dtype=torch.int32, device=dev)
        masks = torch.empty((S, H, W), dtype=torch.uint8, device=dev)
        at = lambda o: ctypes.c_void_p(out.data_ptr() + 4 * o)            # noqa: E731
        st = _C.stream()
        _C.check(L.cp_writer_instances(_C.ptr(rows_dev), R, N, float(self.opt.thresh),
                                       table.ctypes.data_as(ctypes.c_void_p), len(table), at(0), at(o_src),
                                       _C.ptr(poly), at(o_flag), at(o_lab), at(o_conf), st), "cp_writer_instances")
        _C.check(L.cp_instance_masks(_C.ptr(poly), at(o_flag), S, N, H, W, _C.ptr(masks), at(o_cnt), st),
                 "cp_instance_masks")
        nbytes = L.cp_instance_overlaps_workspace_bytes(S, G0, H, W)
        ws = _C.workspace(nbytes, dev)
        _C.check(L.cp_instance_overlaps(_C.ptr(masks), S, _C.ptr(gt_dev), H, W, _C.ptr(ids), G0,
                                        ctypes.c_void_p(ids.data_ptr() + 4 * G0), len(il.VOID_IDS), at(o_int),
                                        at(o_void), at(o_pix), _C.ptr(ws), nbytes, st), "cp_instance_overlaps")
        if boundary is not None:
            bounds = instances.vertex_bounds(poly[:S], instances.MARGIN["cityscapes"], (W, H))
            bd.enqueue_tables(masks, bounds, gt_dev, band_d, ids, G0, out, o_band)
        if distances is not None:
            from ..evaluation import distances as dist
            disp_dev = il.device_ids(distances[0], dev, "disparity")
            if G0:
                dist.enqueue_medians(gt_dev, disp_dev, ids, G0, out[o_med:])
        host = out.cpu().numpy()
        n = int(host[0])
        if n > il.MAX_MASKS:
            raise ValueError("more than 128 instances in one image (max_per_image = K <= 128)")
        flags = host[o_flag:o_flag + fw].view(np.uint8)[:n]
        counts = host[o_cnt:o_cnt + n].astype(np.int64)
        inter = host[o_int:o_int + S * G0].reshape(S, G0)[:n].astype(np.int64)
        for g in range(il.MAX_INST, G, il.MAX_INST):                      # more ids than one call takes: rare
            more = il.device_counts(masks, gt_dev, gt_table[g:g + il.MAX_INST, 0])[0]
            inter = np.concatenate([inter, more[:n]], axis=1)
        conf = host[o_conf:o_conf + n].view(np.float32)
        res = {"n": n, "src": host[o_src:o_src + n].copy(), "labels": host[o_lab:o_lab + n].astype(np.int64),
               "conf": conf.copy(), "counts": counts, "gt_table": gt_table, "inter": inter,
               "void": host[o_void:o_void + n].astype(np.int64)}
        # the writer's selection and the confidence as the text line spells it (what the evaluator reads back)
        kept = [k for k in range(n) if flags[k] & 1 and counts[k] > 100]
        res["kept"] = kept
        res["conf_text"] = [str(min(1, conf[k])) for k in kept]
        extra = {}
        if distances is not None:
            raw = host[o_med:o_med + 4 * G0].reshape(G0, 4).astype(np.int64)
            if G > G0:                                                    # more ids than one call takes: rare
                raw = np.concatenate([raw, dist.instance_distances(gt_dev, gt_table[G0:, 0], disp_dev, distances[1])[1]])
            res["gt_dist_raw"] = raw
            res["gt_dist"] = dist.table_from_counts(raw, distances[1])
            extra = {"gt_dist": res["gt_dist"]}
        if evaluator is not None:
            pix = host[o_pix:o_pix + n].astype(np.int64)
            evaluator.add_counts(gt_table, res["labels"][kept].tolist(), [float(c) for c in res["conf_text"]],
                                 pix[kept], res["void"][kept], inter[kept], **extra)
        if boundary is not None:
            b_inter, b_pred, b_gt = bd.read_tables(host, o_band, S, G0, n, masks, bounds, gt_dev, band_d, gt_table)
            res.update(b_inter=b_inter, b_pred=b_pred, b_gt=b_gt, band_width=band_d)
            pix = host[o_pix:o_pix + n].astype(np.int64)
            boundary.add_counts(gt_table, res["labels"][kept].tolist(), [float(c) for c in res["conf_text"]],
                                pix[kept], res["void"][kept], inter[kept], b_pred[kept], b_gt, b_inter[kept], **extra)
        return res

    def format_and_write_to_cityscapes(self, all_bboxes, save_dir, evaluator=None, gt_files=None, write_files=True,
                                       dist_files=None):
        """Writes the result files; with an `evaluator` (evaluation.instance_level.InstanceLevelEvaluator) the kept
        masks are also scored against `gt_files` ({image prefix: id image path}) while they are on the device; for an
        evaluator with distances, dist_files is evaluation.distances.find_files' dictionary."""
        from PIL import Image
        id_to_file = {im["id"]: im["file_name"] for im in self.coco.imgs.values()}
        masks_dir = os.path.join(save_dir, "masks")
        if write_files:
            os.makedirs(masks_dir, exist_ok=True)
        for image_id in all_bboxes:
            base = os.path.basename(id_to_file[int(image_id)])
            params = self.image_instances(all_bboxes[image_id])
            masks_dev, counts_dev = self.instance_masks_device(params)
            counts = counts_dev.cpu().numpy()
            # the writer's selection: labels with masks, more than 100 pixels; the confidence is the text line's
            kept = [k for k, (p, nz) in enumerate(zip(params, counts)) if p[2] not in self.no_mask_labels and nz > 100]
            confs = [str(min(1, params[k][1] * 1.2)) for k in kept]
            if evaluator is not None:
                from ..evaluation import instance_level
                prefix = base[:-len("_leftImg8bit.png")] if base.endswith("_leftImg8bit.png") else os.path.splitext(base)[0]
                if prefix not in gt_files:
                    raise FileNotFoundError("no ground truth %s%s below --gt_dir for image %s"
                                            % (prefix, instance_level.GT_SUFFIX, base))
                gt_ids = instance_level.read_gt_ids(gt_files[prefix])
                if gt_ids.shape != tuple(masks_dev.shape[1:]):
                    raise ValueError("%s is %s, the result canvas is %s" % (gt_files[prefix], gt_ids.shape,
                                                                            tuple(masks_dev.shape[1:])))
                sel = masks_dev if len(kept) == len(params) else masks_dev[kept]
                extra = {}
                if dist_files is not None:
                    from ..evaluation import distances
                    disp_path, cam_path = distances.frame_files(dist_files, prefix, base)
                    disp = distances.read_disparity(disp_path)
                    if disp.shape != gt_ids.shape:
                        raise ValueError("%s is %s, the ground truth %s is %s" % (disp_path, disp.shape,
                                                                                  gt_files[prefix], gt_ids.shape))
                    extra = {"disparity": disp, "camera": distances.read_camera(cam_path)}
                evaluator.add_image(sel, [self.label_to_id[params[k][2]] for k in kept], [float(c) for c in confs],
                                    gt_ids, **extra)
            if not write_files:
                continue
            device_png = getattr(self.opt, "device_png", False)
            masks = None if device_png else masks_dev.cpu().numpy()
            names = []
            with open(os.path.join(save_dir, base.replace(".png", ".txt")), "w") as text_file:
                for count, (k, conf) in enumerate(zip(kept, confs)):
                    name = base.replace(".png", "_" + str(count) + ".png")
                    text_file.write("masks/" + name + " " + str(self.label_to_id[params[k][2]]) + " " + conf + "\n")
                    if device_png:
                        names.append(os.path.join(masks_dir, name))
                    else:
                        Image.fromarray(masks[k]).save(os.path.join(masks_dir, name))
            if names:                                                     # --device_png: compressed on the device
                from ...utils import png
                png.write(names, planes=masks_dev if len(kept) == len(params) else masks_dev[kept])


class ClassWriterMixin(object):
    """format_and_write_to_kitti / format_and_write_to_IDD (src/lib/datasets/dataset/kitti_poly.py:95-136,
    IDD.py:123-170): per image a text file listing `<image>_<k>.png <label id> <score>` and the instance masks as
    8-bit PNG files on a canvas of the image's own size.  Class by class: a text line per row above the threshold in
    row order, numbered through the image; the masks drawn in ascending depth within the class as PIL's
    polygon(outline=0, fill=255), a nearer instance with score >= 0.5 hiding farther ones of ITS class with its fill
    (PIL draws no outline in the fill's ink, so polygon(outline=0, fill=0) clears the fill alone).  The masks come
    from cp_class_instance_masks; `ap_protocol` names the evaluator's protocol (evaluation.instance_level.PROTOCOLS),
    `at_threshold` whether a score equal to the threshold is kept, `per_city` whether the files go into one directory
    per city (the image's parent directory)."""
    ap_protocol = None
    at_threshold = False
    per_city = False

    def protocol(self):
        from ..evaluation import instance_level
        return instance_level.PROTOCOLS[self.ap_protocol]

    def canvas_of(self, image_id):
        """(width, height) of an image: the annotation record's if it has them, else the image file's header."""
        im = self.coco.imgs[int(image_id)]
        if "width" in im and "height" in im:
            return int(im["width"]), int(im["height"])
        from PIL import Image
        file_name = im["file_name"]
        path = file_name if os.path.isabs(file_name) and os.path.exists(file_name) else \
            os.path.join(self.img_dir, os.path.basename(file_name))
        if not os.path.exists(path):
            raise FileNotFoundError("image %s not found (img_dir %s): its size is the canvas of its masks"
                                    % (file_name, self.img_dir))
        with Image.open(path) as img:
            return img.size

    def image_instances(self, per_class):
        """The instances of one image in DRAWING order (class, depth, row): (points, score, class index counted
        from 0, depth, index of the text line).  Scores are compared in float32, as the selection kernel does."""
        thresh = np.float32(self.opt.thresh)
        out, count = [], 0
        for cls_ind in per_class:
            if cls_ind == "fg":
                continue
            params = []
            for row in per_class[cls_ind]:
                score = np.float32(row[4])
                if score >= thresh if self.at_threshold else score > thresh:
                    poly = [_to_float(v) for v in row[5:-1]]
                    pts = [(int(x), int(y)) for x, y in zip(poly[0::2], poly[1::2])]
                    params.append((pts, score, cls_ind - 1, row[-1], count))
                    count += 1
            out += sorted(params, key=lambda a: a[3])
        return out

    def class_label_table(self):
        """cp_class_writer_instances' table: int32 [C] label id of class 0 .. C-1."""
        return self.writer_class_label_table()

    @classmethod
    def writer_class_label_table(cls):
        """class_label_table without an object (see CityscapesWriterMixin.writer_class_table)."""
        return np.array([cls.label_to_id[c] for c in cls.class_name[1:]], np.int32)

    def class_masks_device(self, params, canvas, device=None):
        """Masks of instances in drawing order, left on the device: (uint8 [n, H, W], int32 [n] pixel counts)."""
        import torch

        from ... import _C
        W, H = canvas
        n = len(params)
        if n == 0:                                           # nothing to draw: no device needed (or touched)
            return torch.zeros((0, H, W), dtype=torch.uint8), torch.zeros((0,), dtype=torch.int32)
        dev = device or torch.device("cuda")
        if n > 128:
            raise ValueError("more than 128 instances in one image (max_per_image = K <= 128)")
        N = len(params[0][0])
        poly = torch.tensor([p[0] for p in params], dtype=torch.int32).reshape(n, N, 2).to(dev)
        group = torch.tensor([p[2] for p in params], dtype=torch.int32).to(dev)
        flags = torch.tensor([1 | (2 if p[1] >= 0.5 else 0) for p in params], dtype=torch.uint8).to(dev)
        masks = torch.empty((n, H, W), dtype=torch.uint8, device=dev)
        counts = torch.empty((n,), dtype=torch.int32, device=dev)
        _C.check(_C.lib().cp_class_instance_masks(_C.ptr(poly), _C.ptr(group), _C.ptr(flags), n, N, H, W,
                                                  _C.ptr(masks), _C.ptr(counts), _C.stream()),
                 "cp_class_instance_masks")
        return masks, counts

    def score_instances_device(self, rows_dev, gt_ids, gt_table=None, evaluator=None, boundary=None):
        """One image scored from its detection rows without a pass through host Python, the KITTI / IDD way: device
        float32 rows [R, 2N + 7] (x1,y1,x2,y2,score,cls,poly,depth; R <= 1024) -> cp_class_writer_instances ->
        cp_class_instance_masks -> cp_instance_overlaps on all slots, then ONE read of the small tables.  The canvas
        is the id image's (an image of another size is refused where both files are known: eval_images, run_eval).
        gt_ids, gt_table as CityscapesWriterMixin.score_instances_device takes them.  With an `evaluator` the
        instances are added to it in the order of the text lines.  Returns the tables in that order: n, src, labels,
        conf (float32), conf_text, counts, text_index, draw_slot, gt_table, inter, void.
        boundary: an evaluation.boundary.BoundaryEvaluator, or None.  With one, the masks also go through
        cp_boundary_overlaps (bounds: the polygons' boxes, which PIL's fill stays inside); the band tables come back in
        the same read, are returned as b_inter, b_pred, b_gt (text-line order) and band_width, and are added to it."""
        import ctypes

        import torch

        from ... import _C
        from ..evaluation import instance_level as il
        proto = self.protocol()
        if rows_dev.dim() != 2 or rows_dev.dtype != torch.float32 or rows_dev.shape[1] < 13 or rows_dev.shape[1] % 2 == 0:
            raise ValueError("rows must be float32 [R, 2N + 7], got %s %s" % (rows_dev.dtype, tuple(rows_dev.shape)))
        dev = rows_dev.device
        R, N = int(rows_dev.shape[0]), (int(rows_dev.shape[1]) - 7) // 2
        if R == 0:                                                         # no detection at all: one dead row
            rows_dev = torch.full((1, 2 * N + 7), float("-inf"), dtype=torch.float32, device=dev)
            R = 1
        S = min(R, il.MAX_MASKS)                                          # slots drawn and counted
        gt_dev = il.device_ids(gt_ids, dev)
        H, W = (int(v) for v in gt_dev.shape)
        if gt_table is None:
            gt_table = il.gt_instances(il.device_histogram(gt_dev), proto)
        gt_table = np.asarray(gt_table, np.int64).reshape(-1, 3)
        G = len(gt_table)
        G0 = min(G, il.MAX_INST)
        L = _C.lib()
        table = np.ascontiguousarray(self.class_label_table())
        ids = torch.from_numpy(np.concatenate([gt_table[:G0, 0], proto.void_ids]).astype(np.int32)).to(dev)
        fw = (R + 3) // 4
        # one buffer for everything that comes back: n, then per row src / label / conf / text index / group, per
        # slot counts / void / pixels, the flag bytes, the intersections
        o_src, o_lab, o_conf, o_text, o_grp = 4, 4 + R, 4 + 2 * R, 4 + 3 * R, 4 + 4 * R
        o_cnt = 4 + 5 * R
        o_void, o_pix, o_flag, o_int = o_cnt + S, o_cnt + 2 * S, o_cnt + 3 * S, o_cnt + 3 * S + fw
        o_band = o_int + S * G0                                           # the band tables, after everything else
        if boundary is not None:
            from ...detectors import instances
            from ..evaluation import boundary as bd
            band_d = boundary.band_width(H, W)
        out = torch.empty((o_band + (bd.table_words(S, G0) if boundary is not None else 0),), dtype=torch.int32,
                          device=dev)
        poly = torch.empty((R, N, 2), dtype=torch.int32, device=dev)
        masks = torch.empty((S, H, W), dtype=torch.uint8, device=dev)
        at = lambda o: ctypes.c_void_p(out.data_ptr() + 4 * o)            # noqa: E731
        st = _C.stream()
        _C.check(L.cp_class_writer_instances(_C.ptr(rows_dev), R, N, float(self.opt.thresh), int(self.at_threshold),
                                             table.ctypes.data_as(ctypes.c_void_p), len(table), at(0), at(o_src),
                                             _C.ptr(poly), at(o_grp), at(o_flag), at(o_lab), at(o_conf), at(o_text),
                                             st), "cp_class_writer_instances")
        _C.check(L.cp_class_instance_masks(_C.ptr(poly), at(o_grp), at(o_flag), S, N, H, W, _C.ptr(masks), at(o_cnt),
                                           st), "cp_class_instance_masks")
        nbytes = L.cp_instance_overlaps_workspace_bytes(S, G0, H, W)
        ws = _C.workspace(nbytes, dev)
        _C.check(L.cp_instance_overlaps(_C.ptr(masks), S, _C.ptr(gt_dev), H, W, _C.ptr(ids), G0,
                                        ctypes.c_void_p(ids.data_ptr() + 4 * G0), len(proto.void_ids), at(o_int),
                                        at(o_void), at(o_pix), _C.ptr(ws), nbytes, st), "cp_instance_overlaps")
        if boundary is not None:
            bounds = instances.vertex_bounds(poly[:S], instances.MARGIN["class"], (W, H))
            bd.enqueue_tables(masks, bounds, gt_dev, band_d, ids, G0, out, o_band)
        host = out.cpu().numpy()
        n = int(host[0])
        if n > il.MAX_MASKS:
            raise ValueError("more than 128 instances in one image (max_per_image = K <= 128)")
        inter = host[o_int:o_int + S * G0].reshape(S, G0)[:n].astype(np.int64)
        for g in range(il.MAX_INST, G, il.MAX_INST):                      # more ids than one call takes: rare
            more = il.device_counts(masks, gt_dev, gt_table[g:g + il.MAX_INST, 0], proto)[0]
            inter = np.concatenate([inter, more[:n]], axis=1)
        text = host[o_text:o_text + n]
        order = np.argsort(text, kind="stable")                           # slot of text line 0, 1, ...
        conf = host[o_conf:o_conf + n].view(np.float32)[order]
        res = {"n": n, "src": host[o_src:o_src + n][order], "labels": host[o_lab:o_lab + n][order].astype(np.int64),
               "conf": conf.copy(), "conf_text": [str(c) for c in conf],
               "counts": host[o_cnt:o_cnt + n][order].astype(np.int64), "text_index": text[order].copy(),
               "draw_slot": order, "gt_table": gt_table, "inter": inter[order],
               "void": host[o_void:o_void + n][order].astype(np.int64)}
        if evaluator is not None:
            pix = host[o_pix:o_pix + n][order].astype(np.int64)
            evaluator.add_counts(gt_table, res["labels"].tolist(), [float(c) for c in res["conf_text"]], pix,
                                 res["void"], res["inter"])
        if boundary is not None:
            b_inter, b_pred, b_gt = bd.read_tables(host, o_band, S, G0, n, masks, bounds, gt_dev, band_d, gt_table)
            res.update(b_inter=b_inter[order], b_pred=b_pred[order], b_gt=b_gt, band_width=band_d)
            pix = host[o_pix:o_pix + n][order].astype(np.int64)
            boundary.add_counts(gt_table, res["labels"].tolist(), [float(c) for c in res["conf_text"]], pix,
                                res["void"], res["inter"], res["b_pred"], b_gt, res["b_inter"])
        return res

    def format_and_write_class_masks(self, all_bboxes, save_dir, evaluator=None, gt_files=None, write_files=True):
        """Writes the result files; with an `evaluator` the masks are also scored against `gt_files` ({image key:
        id image path}) while they are on the device."""
        from PIL import Image
        proto = self.protocol()
        for image_id in all_bboxes:
            file_name = self.coco.imgs[int(image_id)]["file_name"]
            base = os.path.basename(file_name)
            params = self.image_instances(all_bboxes[image_id])
            canvas = self.canvas_of(image_id)
            masks_dev, _ = self.class_masks_device(params, canvas)
            by_line = sorted(range(len(params)), key=lambda k: params[k][4])
            labels = [int(self.label_to_id[self.class_name[params[k][2] + 1]]) for k in by_line]
            confs = [str(params[k][1]) for k in by_line]
            if evaluator is not None:
                from ..evaluation import instance_level
                key = proto.image_key(file_name)
                if key not in gt_files:
                    raise FileNotFoundError("no ground truth %s below --gt_dir for image %s" % (proto.gt_name(key), base))
                gt_ids = instance_level.read_gt_ids(gt_files[key])
                if gt_ids.shape != (canvas[1], canvas[0]):
                    raise ValueError("%s is %s, the image %s is %s" % (gt_files[key], gt_ids.shape, file_name,
                                                                       (canvas[1], canvas[0])))
                evaluator.add_image(masks_dev[by_line] if len(params) else masks_dev, labels, [float(c) for c in confs],
                                    gt_ids)
            if not write_files:
                continue
            write_dir = os.path.join(save_dir, os.path.basename(os.path.dirname(file_name))) if self.per_city else save_dir
            os.makedirs(write_dir, exist_ok=True)
            device_png = getattr(self.opt, "device_png", False)
            masks = None if device_png else masks_dev.cpu().numpy()
            names = []
            with open(os.path.join(write_dir, base.replace(".png", ".txt")), "w") as text_file:
                for count, (k, lab, conf) in enumerate(zip(by_line, labels, confs)):
                    name = base.replace(".png", "_" + str(count) + ".png")
                    text_file.write(name + " " + str(lab) + " " + conf + "\n")
                    if device_png:
                        names.append(os.path.join(write_dir, name))
                    else:
                        Image.fromarray(masks[k]).save(os.path.join(write_dir, name))
            if names:                                                     # --device_png: compressed on the device
                from ...utils import png
                png.write(names, planes=masks_dev[by_line])

    def run_eval(self, results, save_dir):
        """kitti_poly.py / IDD.py run_eval: results.json + the per-image mask files their instance-level evaluation
        reads.  With --gt_dir the masks are also scored on the device (evaluation/instance_level.py, this data set's
        protocol), the evaluator's table is printed, its JSON written and allAp returned; --no_mask_files then skips
        the mask and text files.  Without --gt_dir nothing is scored and the return value is 0.0."""
        PolygonDataset.run_eval(self, results, save_dir)
        res_dir = os.path.join(save_dir, "results")
        os.makedirs(res_dir, exist_ok=True)
        gt_dir = getattr(self.opt, "gt_dir", "")
        if not gt_dir:
            self.format_and_write_class_masks(results, res_dir)
            return 0.0
        from ..evaluation import instance_level
        if not os.path.isdir(gt_dir):
            raise FileNotFoundError("--gt_dir %s is not a directory" % gt_dir)
        evaluator = instance_level.InstanceLevelEvaluator(self.protocol())
        self.format_and_write_class_masks(results, res_dir, evaluator,
                                          instance_level.find_gt_files(gt_dir, self.protocol()),
                                          write_files=not getattr(self.opt, "no_mask_files", False))
        return self.report_eval(evaluator, res_dir)

    def finish_scored_eval(self, results, save_dir, evaluator):
        """run_eval for a run whose images were already scored as they passed (score_instances_device with
        `evaluator`): results.json, the mask and text files unless --no_mask_files, the report."""
        PolygonDataset.run_eval(self, results, save_dir)
        res_dir = os.path.join(save_dir, "results")
        os.makedirs(res_dir, exist_ok=True)
        if not getattr(self.opt, "no_mask_files", False):
            self.format_and_write_class_masks(results, res_dir)
        return self.report_eval(evaluator, res_dir)


class CITYSCAPES(CityscapesWriterMixin, PolygonDataset):
    """src/lib/datasets/dataset/cityscapes.py:39-110."""
    name = "cityscapes"
    annot_subdir = os.path.join("cityscapesStuff", "BBoxes")
    mean = np.array([0.28404999637454165, 0.32266921542410754, 0.2816898182839038], dtype=np.float32).reshape(1, 1, 3)
    std = np.array([0.04230349568017417, 0.04088212241688149, 0.04269893084955519], dtype=np.float32).reshape(1, 1, 3)
    class_name = PolygonDataset.class_name + ["pole", "traffic sign", "traffic light"]
    class_frequencies = {"person": 0.14062428170827013, "rider": 0.015518384984665498, "car": 0.20898266905714155,
                         "truck": 0.003822132907776267, "bus": 0.0031719762791339126,
                         "train": 0.0012740443025920892, "motorcycle": 0.005831707941761728,
                         "bicycle": 0.0322057384531526, "pole": 0.34640870553158515,
                         "traffic sign": 0.16402335310072175, "traffic light": 0.07813700573319936}

    label_to_id = {"person": 24, "rider": 25, "car": 26, "truck": 27, "bus": 28, "train": 31, "motorcycle": 32,
                   "bicycle": 33, "pole": -1, "traffic sign": -1, "traffic light": -1}
    scores_ap = True                                         # run_eval returns the instance-level AP with --gt_dir

    def annot_file(self, split):
        if split == "test":
            return "test.json"
        return "%s%d_regular_interval.json" % ("val" if split == "val" else "train", self.opt.nbr_points)

    def run_eval(self, results, save_dir):
        """cityscapes.py:400-432: results.json + the per-image mask files the Cityscapes instance-level evaluation
        reads.  With --gt_dir the masks are also scored on the device (evaluation/instance_level.py), the evaluator's
        table is printed, its JSON written and allAp returned; --no_mask_files then skips the mask and text files.
        Without --gt_dir nothing is scored and the return value is 0.0."""
        super(CITYSCAPES, self).run_eval(results, save_dir)
        res_dir = os.path.join(save_dir, "results")
        os.makedirs(res_dir, exist_ok=True)
        gt_dir = getattr(self.opt, "gt_dir", "")
        if not gt_dir:
            self.format_and_write_to_cityscapes(results, res_dir)
            return 0.0
        from ..evaluation import instance_level
        if not os.path.isdir(gt_dir):
            raise FileNotFoundError("--gt_dir %s is not a directory" % gt_dir)
        dist_files = None
        if getattr(self.opt, "disparity_dir", "") and getattr(self.opt, "camera_dir", ""):
            from ..evaluation import distances                             # AP 100 m / AP 50 m beside the AP
            dist_files = distances.find_files(self.opt.disparity_dir, self.opt.camera_dir)
            for im in self.coco.imgs.values():                             # a frame without its files: before any score
                if im["id"] in results or str(im["id"]) in results:
                    distances.frame_files(dist_files, instance_level.CITYSCAPES.image_key(im["file_name"]),
                                          os.path.basename(im["file_name"]))
        evaluator = instance_level.InstanceLevelEvaluator(distances=dist_files is not None)
        self.format_and_write_to_cityscapes(results, res_dir, evaluator, instance_level.find_gt_files(gt_dir),
                                            write_files=not getattr(self.opt, "no_mask_files", False),
                                            dist_files=dist_files)
        return self.report_eval(evaluator, res_dir)

    def finish_scored_eval(self, results, save_dir, evaluator):
        """run_eval for a run whose images were already scored as they passed (score_instances_device with
        `evaluator`): results.json, the mask and text files through the writer unless --no_mask_files, the report."""
        PolygonDataset.run_eval(self, results, save_dir)
        res_dir = os.path.join(save_dir, "results")
        os.makedirs(res_dir, exist_ok=True)
        if not getattr(self.opt, "no_mask_files", False):
            self.format_and_write_to_cityscapes(results, res_dir)
        return self.report_eval(evaluator, res_dir)


class KITTIPOLY(ClassWriterMixin, PolygonDataset):
    """src/lib/datasets/dataset/kitti_poly.py:15-60; its writer keeps a row when score > thresh."""
    name = "kitti_poly"
    label_to_id = {"person": 24, "rider": 25, "car": 26, "truck": 27, "bus": 28, "train": 31, "motorcycle": 32,
                   "bicycle": 33}
    ap_protocol = "kitti"                                    # test.py / run_eval score with --gt_dir (scores_ap stays
    at_threshold = False                                     # False: `main.py --metric ap` is still refused here)
    annot_subdir = os.path.join("KITTIPolyStuff", "BBoxes")
    mean = np.array([0.485, 0.456, 0.406], np.float32).reshape(1, 1, 3)
    std = np.array([0.229, 0.224, 0.225], np.float32).reshape(1, 1, 3)
    class_frequencies = {"person": 0.15, "rider": 0.03, "car": 0.20, "truck": 0.03, "bus": 0.03, "train": 0.03,
                         "motorcycle": 0.03, "bicycle": 0.03}

    def annot_file(self, split):
        if split == "test":
            return "test.json"
        return "%s%d.json" % ("val" if split == "val" else "train", self.opt.nbr_points)


class IDD(ClassWriterMixin, PolygonDataset):
    """src/lib/datasets/dataset/IDD.py:15-60 (9 classes, the Cityscapes statistics); its writer keeps a row when
    score >= thresh and writes one directory per city."""
    name = "IDD"
    label_to_id = {"person": 6, "rider": 8, "motorcycle": 9, "bicycle": 10, "autorickshaw": 11, "car": 12,
                   "truck": 13, "bus": 14, "vehicle fallback": 18}
    ap_protocol = "IDD"
    at_threshold = True
    per_city = True
    num_classes = 9
    annot_subdir = os.path.join("IDDStuff", "BBoxes")
    mean = CITYSCAPES.mean
    std = CITYSCAPES.std
    class_name = ["__background__", "person", "rider", "motorcycle", "bicycle", "autorickshaw", "car", "truck",
                  "bus", "vehicle fallback"]
    _valid_ids = [1, 2, 3, 4, 5, 6, 7, 8, 9]
    class_frequencies = {"person": 0.15, "rider": 0.03, "car": 0.20, "truck": 0.03, "bus": 0.03, "motorcycle": 0.03,
                         "bicycle": 0.03, "autorickshaw": 0.33, "vehicle fallback": 0.18}

    def annot_file(self, split):
        if split == "test":
            return "test.json"
        return "%s%d_regular_interval.json" % ("val" if split == "val" else "train", self.opt.nbr_points)

"""The image list of test.py (reference: src/test.py:23-44 PrefetchDataset and :99-112): `dataset.images` ->
`coco.loadImgs` -> `read_image`, one item per image.  An item is decoded on the host only, so the items can come from
`DataLoader` workers while the detector runs: the 8-bit BGR image and, when ground truth is scored, the 16-bit id
image with its ground-truth table (`gt_instances` on an `np.bincount`, so no histogram has to come back from the
device before the overlap kernel starts).  With --disparity_dir / --camera_dir also the frame's 16-bit disparity image
and its camera's (baseline, fx), for the distance columns of the AP.  A missing image or ground-truth file is an error
that names the path; a frame without its disparity or camera file is one when the list is made."""
import os

import numpy as np
import torch.utils.data as data

from .evaluation import instance_level


def image_prefix(file_name):
    """`frankfurt_000000_000294` of `.../frankfurt_000000_000294_leftImg8bit.png`: the key of the ground truth."""
    return instance_level.CITYSCAPES.image_key(file_name)


class EvalImages(data.Dataset):
    def __init__(self, dataset, gt_files=None, protocol=None, dist_files=None):
        self.dataset = dataset
        self.gt_files = gt_files                               # {image key: id image path} or None
        self.protocol = protocol or instance_level.CITYSCAPES  # whose key, ground-truth table and file names
        self.dist_files = dist_files                           # distances.find_files' dictionary or None
        if dist_files is not None:                             # a frame without its two files: before anything is scored
            for ind in range(len(self)):
                self.distance_paths(self.info(ind)[1])

    def __len__(self):
        return len(self.dataset.images)

    def info(self, ind):
        """(image id, file name as the annotation file gives it)."""
        img_id = self.dataset.images[ind]
        return img_id, self.dataset.coco.loadImgs(ids=[img_id])[0]["file_name"]

    def gt_path(self, file_name):
        key = self.protocol.image_key(file_name)
        if key not in self.gt_files:
            raise FileNotFoundError("no ground truth %s below --gt_dir for image %s"
                                    % (self.protocol.gt_name(key), os.path.basename(file_name)))
        return self.gt_files[key]

    def distance_paths(self, file_name):
        from .evaluation import distances
        return distances.frame_files(self.dist_files, self.protocol.image_key(file_name), os.path.basename(file_name))

    def __getitem__(self, ind):
        img_id, file_name = self.info(ind)
        item = {"img_id": img_id, "image": self.dataset.read_image(file_name)}
        if self.gt_files is not None:
            path = self.gt_path(file_name)
            if not os.path.isfile(path):
                raise FileNotFoundError("ground truth %s not found" % path)
            ids = instance_level.read_gt_ids(path)
            if self.protocol is not instance_level.CITYSCAPES and ids.shape != item["image"].shape[:2]:
                raise ValueError("%s is %s, the image %s is %s: KITTI / IDD masks are drawn on the image's own canvas"
                                 % (path, ids.shape, file_name, item["image"].shape[:2]))
            item["gt_ids"] = ids
            item["gt_table"] = instance_level.gt_instances(np.bincount(ids.reshape(-1), minlength=65536),
                                                           self.protocol)
            if self.dist_files is not None:
                from .evaluation import distances
                disp_path, cam_path = self.distance_paths(file_name)
                disp = distances.read_disparity(disp_path)
                if disp.shape != ids.shape:
                    raise ValueError("%s is %s, the ground truth %s is %s" % (disp_path, disp.shape, path, ids.shape))
                item["disparity"] = disp
                item["camera"] = distances.read_camera(cam_path)
        return item


def _first(batch):
    return batch[0]


def group(items, n, same_size=False):
    """Lists of up to `n` consecutive items, in order, for `detector.run_batch` (test.py --test_batch_size); the last
    may be short.  An item is an image array or a dict with one under "image".  same_size (--keep_res, where the
    network input follows the source): a group also ends where the next image's (h, w) differs from its first's.
    Pure host, nothing is copied: the loader's workers keep decoding ahead, one image each."""
    n = int(n)
    if n < 1:
        raise ValueError("group size must be at least 1 (got %d)" % n)
    size = lambda item: tuple((item["image"] if isinstance(item, dict) else item).shape[:2])
    current = []
    for item in items:
        if current and (len(current) == n or (same_size and size(item) != size(current[0]))):
            yield current
            current = []
        current.append(item)
    if current:
        yield current


def iterate(images, prefetch, num_workers):
    """The items in order: a plain loop, or a DataLoader whose `num_workers` workers decode ahead of the consumer
    (batches of one, handed over as they are: the arrays are not collated into tensors)."""
    if not prefetch:
        return (images[i] for i in range(len(images)))
    return data.DataLoader(images, batch_size=1, shuffle=False, num_workers=max(0, int(num_workers)),
                           collate_fn=_first, pin_memory=False)

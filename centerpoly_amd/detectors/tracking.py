"""Instance tracking: link the instances of consecutive frames by the IoU of the pixels they own ("instance tracking" in
include/centerpoly_hip.h, pinned by tests/golden/tracking_host.py; not in the reference).

A tracker belongs to one canvas and keeps its memory map and slot table on the device.  A step issues three calls on
the current stream -- cp_map_pairs (memory map against the frame's owner map), cp_track_associate (greedy matching, new
tracks, ageing, one workgroup) and cp_track_update (the new memory map and the id image) -- and one copy brings the small
tables back.  The defaults iou_thresh = 0.3 and max_age = 0 are this project's untuned choices.

With motion=True ("instance tracking with motion", pinned by tests/golden/tracking_motion_host.py) a track's remembered
pixels are compared where the track should be now, at the velocity between its last two sightings: the step is
cp_track_predict, cp_map_pairs_shifted, cp_track_associate, cp_track_kinematics, cp_track_update.  The velocity is not
smoothed: that, too, is an untuned choice."""
import ctypes
import math
import os

import numpy as np
import torch

from .. import _C

SLOTS = 256                                             # CP_TRACK_SLOTS
MAX_INSTANCES = 128
MAX_ROWS, MAX_COLS = 1024, 255                          # cp_map_pairs
NONE = 0xffff
TOO_MANY = "more than 256 tracks alive"
# the state buffer, int32: slots [256][5], next_id, status, inst [128][5], assigned (256 bytes)
O_NEXT = SLOTS * 5
O_STATUS = O_NEXT + 1
O_INST = O_STATUS + 1
O_ASSIGNED = O_INST + MAX_INSTANCES * 5
STATE_INTS = O_ASSIGNED + SLOTS // 4
# behind them under motion: kin [256][6] = {cx, cy, vx, vy, seen, valid} (1/16 pixel), shift [256][2] = {dx, dy}
O_KIN = STATE_INTS
O_SHIFT = O_KIN + SLOTS * 6
MOTION_INTS = O_SHIFT + SLOTS * 2
SUBPIXEL = 16.0


def _host_ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def as_bits16(t):
    """A device tensor of 16-bit integers as the kernels take it (int16 holding the bits)."""
    if t.dtype == torch.int16:
        return t
    if t.dtype == getattr(torch, "uint16", None):
        return t.view(torch.int16)
    raise ValueError("a 16-bit map must be int16 or uint16, got %s" % t.dtype)


def map_pairs(a, b, R, n, row_of=None, out=None):
    """cp_map_pairs on device tensors: a 16-bit [H, W], b uint8 [H, W], optional row_of 16-bit [65536].  Returns the
    device table int32 [R + 1, n + 1] (a view of `out` when given), the none row and column last."""
    a = as_bits16(a)
    if a.dim() != 2 or b.dim() != 2 or b.dtype != torch.uint8 or tuple(a.shape) != tuple(b.shape):
        raise ValueError("map_pairs takes a 16-bit map and a uint8 map of one shape [H, W], got %s %s and %s %s"
                         % (a.dtype, tuple(a.shape), b.dtype, tuple(b.shape)))
    R, n = int(R), int(n)
    if not (0 <= R <= MAX_ROWS and 0 <= n <= MAX_COLS):
        raise ValueError("map_pairs: R = %d rows (at most %d), n = %d columns (at most %d)" % (R, MAX_ROWS, n, MAX_COLS))
    if row_of is not None:
        row_of = as_bits16(row_of)
        if row_of.numel() != 65536:
            raise ValueError("row_of must hold 65536 entries, got %d" % row_of.numel())
    H, W = (int(v) for v in a.shape)
    cells = (R + 1) * (n + 1)
    if out is None:
        out = torch.empty((cells,), dtype=torch.int32, device=a.device)
    _C.check(_C.lib().cp_map_pairs(_C.ptr(a), _C.ptr(row_of), R, _C.ptr(b), n, H, W, _C.ptr(out), _C.stream()),
             "cp_map_pairs")
    return out[:cells].view(R + 1, n + 1)


def map_pairs_shifted(a, shift, b, R, n, out=None):
    """cp_map_pairs_shifted on device tensors: a 16-bit [H, W], shift int32 [R, 2] = (dx, dy) per row, b uint8 [H, W].
    Returns the device table int32 [R + 1, n + 1] (a view of `out` when given): row r counts the pixels of r moved by
    its shift and clipped to the canvas, row R is what is left of every column's area (it may be negative)."""
    a = as_bits16(a)
    if a.dim() != 2 or b.dim() != 2 or b.dtype != torch.uint8 or tuple(a.shape) != tuple(b.shape):
        raise ValueError("map_pairs_shifted takes a 16-bit map and a uint8 map of one shape [H, W], got %s %s and %s %s"
                         % (a.dtype, tuple(a.shape), b.dtype, tuple(b.shape)))
    R, n = int(R), int(n)
    if not (0 <= R <= MAX_ROWS and 0 <= n <= MAX_COLS):
        raise ValueError("map_pairs_shifted: R = %d rows (at most %d), n = %d columns (at most %d)"
                         % (R, MAX_ROWS, n, MAX_COLS))
    if shift.dtype != torch.int32 or shift.numel() != 2 * R:
        raise ValueError("shift must be int32 [%d, 2], got %s %s" % (R, shift.dtype, tuple(shift.shape)))
    H, W = (int(v) for v in a.shape)
    cells = (R + 1) * (n + 1)
    if out is None:
        out = torch.empty((cells,), dtype=torch.int32, device=a.device)
    _C.check(_C.lib().cp_map_pairs_shifted(_C.ptr(a), _C.ptr(shift) if R else None, R, _C.ptr(b), n, H, W, _C.ptr(out),
                                           _C.stream()), "cp_map_pairs_shifted")
    return out[:cells].view(R + 1, n + 1)


def _check_params(iou_thresh, max_age):
    if not (math.isfinite(iou_thresh) and 0 < iou_thresh <= 1):
        raise ValueError("iou_thresh must be finite and in (0, 1], got %r" % (iou_thresh,))
    if int(max_age) != max_age or max_age < 0:
        raise ValueError("max_age must be an integer >= 0, got %r" % (max_age,))


def _associate(state, pairs, n, label, live, iou_thresh, max_age, t):
    at = lambda o: ctypes.c_void_p(state.data_ptr() + 4 * o)              # noqa: E731
    _C.check(_C.lib().cp_track_associate(_C.ptr(pairs), n, _host_ptr(label) if n else None,
                                         _host_ptr(live) if n else None, at(0), at(O_NEXT), float(iou_thresh),
                                         int(max_age), int(t), at(O_INST), at(O_ASSIGNED), at(O_STATUS), _C.stream()),
             "cp_track_associate")


def _instances(n, label, live):
    n = int(n)
    if not 0 <= n <= MAX_INSTANCES:
        raise ValueError("%d instances in one frame, more than %d" % (n, MAX_INSTANCES))
    label = np.ascontiguousarray(np.asarray(label).reshape(-1)[:n], np.int32)
    live = np.ascontiguousarray(np.asarray(live).reshape(-1)[:n] != 0, np.uint8)
    if len(label) < n or len(live) < n:
        raise ValueError("%d labels and %d live flags for %d instances" % (len(label), len(live), n))
    return n, label, live


def _split_state(host, n):
    return {"slots": host[:O_NEXT].reshape(SLOTS, 5).copy(), "next_id": int(host[O_NEXT]), "status": int(host[O_STATUS]),
            "inst": host[O_INST:O_INST + 5 * n].reshape(n, 5).copy(),
            "assigned": host[O_ASSIGNED:O_ASSIGNED + SLOTS // 4].view(np.uint8).copy()}


def associate(pairs, n, label, live, slots, next_id, iou_thresh=0.3, max_age=0, t=0):
    """cp_track_associate on a device pair table int32 [257, n + 1] and a host slot table int [256, 5]: the dictionary
    {slots, next_id, inst [n, 5], assigned [256], status} after the step, as host arrays.  With status 1 (more than 256
    tracks alive) slots and next_id are the ones given and inst / assigned are not meaningful."""
    _check_params(iou_thresh, max_age)
    n, label, live = _instances(n, label, live)
    if pairs.dtype != torch.int32 or pairs.numel() != (SLOTS + 1) * (n + 1):
        raise ValueError("the pair table must be int32 [%d, %d], got %s %s" % (SLOTS + 1, n + 1, pairs.dtype,
                                                                             tuple(pairs.shape)))
    host = np.zeros((STATE_INTS,), np.int32)
    host[:O_NEXT] = np.asarray(slots, np.int32).reshape(-1)
    host[O_NEXT] = int(next_id)
    state = torch.from_numpy(host).to(pairs.device)
    _associate(state, pairs.contiguous(), n, label, live, iou_thresh, max_age, t)
    return _split_state(state.cpu().numpy(), n)


class TrackedFrame(object):
    """What InstanceTracker.step returns.
      ids                device int32 [H, W]: label * multiplier + track_id of the pixel's owner, 0 where none
      track_of_instance  device int32 [n]: the track id of every instance, 0 for a dead one
      table              host dict, read back in one copy: n, track_id / slot / is_new / inter / union (arrays over the
                         n instances; slot -1 for a dead instance, inter = union = 0 for a new track), alive (int
                         [A, 6] rows slot, track_id, label, first_frame, last_seen, hits of the occupied slots), slots
                         (the whole table [256, 5]), assigned ([256], slots that took an instance in this frame),
                         next_id, status; under motion also kin ([256, 6], after the step), shift ([256, 2], the
                         shifts used in this frame), centroid and velocity ([n, 2] float pixels and pixels per frame
                         of the instance's track, kin / 16; zeros for a dead instance)
      frame              the frame counter t of this step; multiplier"""

    def __init__(self, ids, track_of_instance, table, frame, multiplier):
        self.ids, self.track_of_instance, self.table, self.frame, self.multiplier = ids, track_of_instance, table, frame, multiplier


class InstanceTracker(object):
    """InstanceTracker(canvas = (width, height)).step(maps) for the InstanceMaps of consecutive frames."""

    def __init__(self, canvas, iou_thresh=0.3, max_age=0, multiplier=None, device=None, motion=False):
        W, H = (int(v) for v in canvas)
        if W < 1 or H < 1:
            raise ValueError("the canvas must be at least 1 x 1 (width, height), got %r" % (canvas,))
        _check_params(iou_thresh, max_age)
        if multiplier is not None and int(multiplier) < 1:
            raise ValueError("multiplier must be >= 1, got %r" % (multiplier,))
        self.canvas, self.iou_thresh, self.max_age = (W, H), float(iou_thresh), int(max_age)
        self.multiplier = None if multiplier is None else int(multiplier)
        self.motion = bool(motion)
        self.device = torch.device(device if device is not None else "cuda")
        if self.device.type != "cuda":
            raise _C.NativeError("InstanceTracker needs a HIP device (got %s); there is no CPU fallback" % self.device)
        _C.lib()
        self.pairs = torch.empty(((SLOTS + 1) * (MAX_INSTANCES + 1),), dtype=torch.int32, device=self.device)
        if self.motion:
            self.moments_bytes = int(_C.lib().cp_track_kinematics_workspace_bytes(MAX_INSTANCES))
            self.moments = _C.workspace(self.moments_bytes, self.device)
        self.reset()

    def reset(self):
        """Forget every track: the state of a new tracker."""
        W, H = self.canvas
        self.mem = torch.full((H, W), -1, dtype=torch.int16, device=self.device)       # 0xffff
        host = np.zeros((MOTION_INTS if self.motion else STATE_INTS,), np.int32)
        host[O_NEXT] = 1
        self.state = torch.from_numpy(host).to(self.device)
        self.frame = 0

    def step(self, maps):
        """One frame from its InstanceMaps (detector.instances / instance_maps)."""
        if tuple(maps.canvas) != self.canvas:
            raise ValueError("the tracker's canvas is %d x %d and the frame's is %d x %d: call reset() on a tracker of "
                             "the new canvas, tracks do not carry over" % (self.canvas + tuple(maps.canvas)))
        t = maps.table
        return self.step_index(maps.index, t["n"], t["label"], t["live"],
                               maps.multiplier if self.multiplier is None else self.multiplier)

    def enqueue(self, index, n, label, live, multiplier):
        """The three calls of a step for frame `self.frame` (five under motion), nothing read back and the frame
        counter left alone: the id image.  Arguments as _instances returns them; step_index is the checked way in."""
        W, H = self.canvas
        at = lambda o: ctypes.c_void_p(self.state.data_ptr() + 4 * o)     # noqa: E731
        if self.motion:
            _C.check(_C.lib().cp_track_predict(at(0), at(O_KIN), int(self.frame), H, W, at(O_SHIFT), _C.stream()),
                     "cp_track_predict")
            pairs = map_pairs_shifted(self.mem, self.state[O_SHIFT:O_SHIFT + 2 * SLOTS], index, SLOTS, n, out=self.pairs)
        else:
            pairs = map_pairs(self.mem, index, SLOTS, n, out=self.pairs)
        _associate(self.state, pairs, n, label, live, self.iou_thresh, self.max_age, self.frame)
        if self.motion:
            _C.check(_C.lib().cp_track_kinematics(_C.ptr(index), n, H, W, at(O_INST), at(0), at(O_STATUS),
                                                  int(self.frame), at(O_KIN), _C.ptr(self.moments), self.moments_bytes,
                                                  _C.stream()), "cp_track_kinematics")
        ids = torch.empty((H, W), dtype=torch.int32, device=self.device)
        _C.check(_C.lib().cp_track_update(_C.ptr(index), n, _host_ptr(label) if n else None, H, W, at(0), at(O_INST),
                                          at(O_ASSIGNED), at(O_STATUS), multiplier, _C.ptr(self.mem), _C.ptr(ids),
                                          _C.stream()), "cp_track_update")
        return ids

    def step_index(self, index, n, label, live, multiplier=None):
        """One frame from its owner map: index device uint8 [H, W] (255 = none), n instances, their labels and live
        flags (host)."""
        W, H = self.canvas
        if multiplier is None:
            multiplier = self.multiplier
        if multiplier is None or int(multiplier) < 1:
            raise ValueError("step_index needs a multiplier >= 1 (the tracker was made without one)")
        if index.dtype != torch.uint8 or tuple(index.shape) != (H, W):
            raise ValueError("the owner map must be uint8 [%d, %d], got %s %s: a canvas change needs a new tracker"
                             % (H, W, index.dtype, tuple(index.shape)))
        if index.device != self.mem.device:
            raise ValueError("the owner map is on %s, the tracker on %s" % (index.device, self.mem.device))
        n, label, live = _instances(n, label, live)
        ids = self.enqueue(index.contiguous(), n, label, live, int(multiplier))
        track_of_instance = self.state[O_INST:O_INST + 5 * n].view(n, 5)[:, 1].clone()
        host = self.state.cpu().numpy()                                   # the one copy
        tab = _split_state(host, n)
        if tab["status"]:
            raise ValueError("%s in frame %d: the step changed nothing; lower --track_max_age or raise --thresh"
                             % (TOO_MANY, self.frame))
        inst, slots = tab.pop("inst"), tab["slots"]
        occupied = np.flatnonzero(slots[:, 0])
        tab.update({"n": n, "slot": inst[:, 0], "track_id": inst[:, 1], "inter": inst[:, 2], "union": inst[:, 3],
                    "is_new": inst[:, 4] != 0, "alive": np.concatenate([occupied[:, None], slots[occupied]], 1)})
        if self.motion:
            kin = host[O_KIN:O_SHIFT].reshape(SLOTS, 6).copy()
            of_inst = np.where(inst[:, :1] >= 0, kin[np.maximum(inst[:, 0], 0)], 0) / SUBPIXEL
            tab.update({"kin": kin, "shift": host[O_SHIFT:MOTION_INTS].reshape(SLOTS, 2).copy(),
                        "centroid": of_inst[:, 0:2], "velocity": of_inst[:, 2:4]})
        frame = self.frame
        self.frame += 1
        return TrackedFrame(ids, track_of_instance, tab, frame, int(multiplier))


def save_tracks(maps, tracked, out_dir, stem, device_png=False):
    """--track --save_ids: `<stem>_tracks.json` (per live instance: track id, label, score, box, is_new; under
    --track_motion also centroid [x, y] in pixels and velocity [vx, vy] in pixels per frame of its track) and
    `<stem>_trackIds.png` (16 bit, label * multiplier + track_id) in out_dir.  The PNG cannot hold a track id that
    reaches the multiplier: a ValueError that names the frame; the JSON has no such limit and is written first.
    device_png: the PNG is compressed on the device (utils/png.py).  Returns the two paths."""
    import json
    import os

    from ..datasets.ground_truth import write_id_png
    os.makedirs(out_dir, exist_ok=True)
    paths = [os.path.join(out_dir, stem + "_tracks.json"), os.path.join(out_dir, stem + "_trackIds.png")]
    t, k_tab = maps.table, tracked.table
    entries = [{"track_id": int(k_tab["track_id"][k]), "label_id": int(t["label"][k]),
                "class_name": maps.names.get(int(t["label"][k]), ""), "score": float(t["score"][k]),
                "box": [int(v) for v in t["box"][k]], "is_new": bool(k_tab["is_new"][k])}
               for k in range(int(t["n"])) if t["live"][k]]
    if "centroid" in k_tab:
        for e, k in zip(entries, [k for k in range(int(t["n"])) if t["live"][k]]):
            e["centroid"] = [float(v) for v in k_tab["centroid"][k]]
            e["velocity"] = [float(v) for v in k_tab["velocity"][k]]
    with open(paths[0], "w") as f:
        json.dump({"frame": int(tracked.frame), "width": maps.canvas[0], "height": maps.canvas[1],
                   "multiplier": int(tracked.multiplier), "instances": entries}, f)
    worst = max([e["track_id"] for e in entries], default=0)
    if worst >= tracked.multiplier or max([e["label_id"] for e in entries], default=0) * tracked.multiplier + worst > 65535:
        raise ValueError("%s (frame %d of its sequence): track id %d does not fit label * %d + track_id in 16 bits; "
                         "%s holds the tracks" % (stem, tracked.frame, worst, tracked.multiplier, paths[0]))
    write_id_png(paths[1], tracked.ids, 16, device_png=device_png)
    return paths


MOTS_ID_BASE = 1000                                     # object_id = class_id * 1000 + track id (KITTI MOTS)


def parse_class_map(text):
    """--mots_class_map: "26:1,24:2" -> {26: 1, 24: 2} (label id : class id of the MOTS file); empty: None.  A
    malformed pair, a negative number or a label named twice is a ValueError."""
    if text is None or not str(text).strip():
        return None
    out = {}
    for pair in str(text).split(","):
        parts = pair.split(":")
        try:
            if len(parts) != 2:
                raise ValueError
            label, cls = int(parts[0]), int(parts[1])
        except ValueError:
            raise ValueError("--mots_class_map takes label:class pairs such as 26:1,24:2; %r is none" % pair)
        if label < 0 or cls < 0 or label in out:
            raise ValueError("--mots_class_map: label %d is negative, maps to a negative class or is named twice" % label)
        out[label] = cls
    return out


def mots_lines(maps, tracked, class_map=None, what=""):
    """The frame's lines of a MOTS text file, `frame object_id class_id H W rle`, one per live tracked instance that
    owns a pixel: the RLE (cp_rle_encode on the owner map, so the masks of a frame are disjoint) of the pixels the
    instance owns, class_id the label id or its image under `class_map` (a label the map lacks is skipped), object_id
    = class_id * 1000 + track id.  A track id >= 1000 is a ValueError naming the frame."""
    from ..utils import rle
    t, k_tab = maps.table, tracked.table
    n = int(t["n"])
    keep = []
    for k in range(n):
        if not t["live"][k] or int(t["visible"][k]) <= 0 or int(k_tab["track_id"][k]) <= 0:
            continue
        label = int(t["label"][k])
        if class_map is not None and label not in class_map:
            continue
        track = int(k_tab["track_id"][k])
        if track >= MOTS_ID_BASE:
            raise ValueError("%s (frame %d of its sequence): track id %d does not fit object_id = class_id * %d + track id"
                             % (what, tracked.frame, track, MOTS_ID_BASE))
        keep.append((k, label if class_map is None else class_map[label], track))
    if not keep:
        return []
    rles = rle.encode(index=maps.index, n=n, bounds=np.ascontiguousarray(t["box"], np.int32).reshape(n, 4))
    W, H = maps.canvas
    return ["%d %d %d %d %d %s" % (tracked.frame, cls * MOTS_ID_BASE + track, cls, H, W, rles[k]["counts"])
            for k, cls, track in keep]


class MotsWriter(object):
    """--track --save_rle: `<out_dir>/mots/<sequence key>.txt`, the lines of mots_lines frame after frame.  A
    sequence's file starts anew the first time this writer sees its key."""

    def __init__(self, out_dir, class_map=None):
        self.dir, self.class_map, self.seen = os.path.join(out_dir, "mots"), class_map, set()

    def path(self, key):
        name = "_".join(p for p in str(key).replace("\\", "/").split("/") if p and p != ".") or "sequence"
        return os.path.join(self.dir, name + ".txt")

    def add(self, key, maps, tracked, what=""):
        lines = mots_lines(maps, tracked, self.class_map, what)
        os.makedirs(self.dir, exist_ok=True)
        path = self.path(key)
        with open(path, "a" if key in self.seen else "w") as f:
            f.write("".join(line + "\n" for line in lines))
        self.seen.add(key)
        return path


class SequenceTracker(object):
    """The drivers' tracker: frames arrive in order with their file names, the tracker starts anew where the sequence
    key (evaluation.tracking.sequence_key) changes, on a tracker of the frame's canvas."""

    def __init__(self, iou_thresh=0.3, max_age=0, motion=False):
        self.iou_thresh, self.max_age, self.motion = iou_thresh, max_age, bool(motion)
        self.tracker, self.key = None, None

    def step(self, file_name, maps):
        """(sequence key, TrackedFrame) of the frame."""
        from ..datasets.evaluation.tracking import sequence_key
        key = sequence_key(file_name)
        if key != self.key:
            if self.tracker is None or self.tracker.canvas != tuple(maps.canvas) or \
                    self.tracker.device != maps.index.device:
                self.tracker = InstanceTracker(maps.canvas, self.iou_thresh, self.max_age, device=maps.index.device,
                                               motion=self.motion)
            else:
                self.tracker.reset()
            self.key = key
        return key, self.tracker.step(maps)

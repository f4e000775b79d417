"""Instance tracking on the device against the host statement (tests/golden/tracking_host.py), exact equality: the
pair counting, the association on hand-made pair tables, whole steps through instance_maps, the MOTS scoring and the
drivers."""
import contextlib
import io
import json
import math
import os

import numpy as np
import pytest

import tracking_host as host
import test_instances_api as tia
from test_tracking_cpu import CAR, _one_pair, tie_tables

pytestmark = pytest.mark.gpu

T = host.T
f32 = np.float32


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _offset_by_one(a):
    """The array as a device tensor that starts one element into its buffer: an unaligned base."""
    import torch
    flat = torch.from_numpy(np.ascontiguousarray(a).reshape(-1))
    buf = torch.empty((flat.numel() + 9,), dtype=flat.dtype, device="cuda")
    buf[1:1 + flat.numel()] = flat.cuda()
    out = buf[1:1 + flat.numel()].view(a.shape)
    assert out.is_contiguous() and out.data_ptr() % 16 == out.element_size()
    return out


# ------------------------------------------------------------------------------------------------ cp_map_pairs --
def _pair_case(name):
    """(a uint16 [H, W], b uint8 [H, W], R, n, row_of or None, offset by one element)"""
    rng = np.random.RandomState(sum(map(ord, name)))
    if name == "unaligned":             # a tail, rows without a pixel (5 .. 8), the none row (9, 0xffff) and column
        a = rng.choice([0, 1, 2, 4, 9, 0xffff], (37, 53)).astype(np.uint16)
        b = rng.choice([0, 1, 2, 3, 7, 255], (37, 53)).astype(np.uint8)
        return a, b, 9, 4, None, True
    if name == "one_pair":              # every pixel in one pair
        return np.full((37, 53), 3, np.uint16), np.full((37, 53), 1, np.uint8), 5, 2, None, False
    if name == "lookup":                # several ids to one row, some to none, runs of equal values
        a = np.ascontiguousarray(np.repeat(rng.choice([26001, 26002, 24001, 10000, 26, 7, 0], (37, 9)), 6, 1)[:, :53],
                                 np.uint16)
        b = np.ascontiguousarray(np.repeat(rng.choice([0, 1, 255], (37, 14)), 4, 1)[:, :53], np.uint8)
        row_of = np.full((65536,), 0xffff, np.uint16)
        row_of[[10000, 26]] = 0
        row_of[[26001, 26002]] = 1
        row_of[24001] = 2
        return a, b, 3, 2, row_of, True
    H, W = 64, 256
    R, n = {"limits": (1024, 255), "lds_128": (128, 128), "lds_bound": (256, 128), "past_bound": (256, 129)}[name]
    a = rng.randint(0, R + R // 8 + 2, (H, W)).astype(np.uint16)      # some values past the last row
    b = rng.randint(0, 256, (H, W)).astype(np.uint8)
    return a, b, R, n, None, False


@pytest.mark.parametrize("name", ["unaligned", "one_pair", "lookup", "limits", "lds_128", "lds_bound", "past_bound"])
def test_map_pairs(name):
    import torch
    from centerpoly_amd.detectors import tracking
    a, b, R, n, row_of, offset = _pair_case(name)
    want = host.map_pairs(a, b, R, n, row_of)
    place = _offset_by_one if offset else _dev
    got = tracking.map_pairs(place(a.view(np.int16)), place(b), R, n, None if row_of is None else _dev(row_of.view(np.int16)))
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    assert got.shape == (R + 1, n + 1) and np.array_equal(got, want)
    # row sums and column sums are the areas
    rows = a.astype(np.int64) if row_of is None else row_of[a].astype(np.int64)
    rows, cols = np.minimum(rows, R), np.minimum(b.astype(np.int64), n)
    assert np.array_equal(got.sum(1), np.bincount(rows.reshape(-1), minlength=R + 1))
    assert np.array_equal(got.sum(0), np.bincount(cols.reshape(-1), minlength=n + 1))
    assert got.sum() == a.size
    if name == "unaligned":
        assert not got[5:9].any() and got[9].sum() > 0 and got[:, 4].sum() > 0
    if name == "one_pair":
        assert got[3, 1] == a.size
    if name in ("lds_bound", "past_bound"):                                 # the two sides of the LDS bound
        assert ((R + 1) * (n + 1) <= 257 * 129) == (name == "lds_bound")


def test_map_pairs_refuses_what_it_cannot_count():
    from centerpoly_amd import _C
    L = _C.lib()
    assert L.cp_map_pairs(None, None, 4, None, 4, 8, 8, None, None) == -1
    assert L.cp_map_pairs(None, None, 1025, None, 4, 8, 8, None, None) == -2
    assert L.cp_map_pairs(None, None, 4, None, 256, 8, 8, None, None) == -2
    assert L.cp_track_associate(None, 129, None, None, None, None, 0.3, 0, 0, None, None, None, None) == -2
    assert L.cp_track_associate(None, 1, None, None, None, None, float("nan"), 0, 0, None, None, None, None) == -1
    assert L.cp_track_update(None, 1, None, 8, 8, None, None, None, None, 0, None, None, None) == -1


# ------------------------------------------------------------------------------------------------- association --
def _assoc_both(pairs, n, label, live, slots, next_id, thresh, max_age, t):
    """The device and the host statement on one hand-made table; returns the device dictionary after comparing."""
    from centerpoly_amd.detectors import tracking
    got = tracking.associate(_dev(np.asarray(pairs, np.int32)), n, label, live, slots, next_id, thresh, max_age, t)
    s, nid, inst, assigned = host.associate(pairs, n, label, live, slots, next_id, thresh, max_age, t)
    assert got["status"] == 0 and got["next_id"] == nid
    assert np.array_equal(got["slots"], s) and np.array_equal(got["inst"], inst) and np.array_equal(got["assigned"], assigned)
    return got


def test_association_ties_and_equal_fractions():
    for name, slots, pairs, n, thresh, want in tie_tables():
        got = _assoc_both(pairs, n, [CAR] * n, [1] * n, slots, 10, thresh, 0, 1)
        assert got["inst"].tolist() == want, name


def test_association_threshold_boundary():
    slots = np.zeros((T, 5), np.int64)
    slots[0] = [7, CAR, 0, 4, 5]
    assert _assoc_both(_one_pair(3, 3, 4), 1, [CAR], [1], slots, 8, 0.3, 0, 5)["inst"].tolist() == [[0, 7, 3, 10, 0]]
    assert _assoc_both(_one_pair(29, 30, 41), 1, [CAR], [1], slots, 8, 0.3, 0, 5)["inst"].tolist() == [[1, 8, 0, 0, 1]]


def test_association_label_mismatch_and_dead_instance():
    """Slot 0 (car) overlaps instance 0 (a person) most and instance 1 (a car) a little; instance 2 (a car) overlaps it
    well but is dead.  The car of instance 1 is matched, the person starts a track, the dead instance gets nothing."""
    slots = np.zeros((T, 5), np.int64)
    slots[0] = [3, CAR, 0, 0, 1]
    pairs = np.zeros((T + 1, 4), np.int64)
    pairs[0] = [40, 12, 30, 5]
    pairs[T] = [2, 8, 1, 100]
    got = _assoc_both(pairs, 3, [24, CAR, CAR], [1, 1, 0], slots, 4, 0.1, 0, 1)
    assert got["inst"].tolist() == [[1, 4, 0, 0, 1], [0, 3, 12, 87 + 20 - 12, 0], [-1, 0, 0, 0, 0]]


@pytest.mark.parametrize("max_age,want_id", [(0, 2), (1, 2), (3, 1)])
def test_association_max_age_with_a_track_hidden_for_two_frames(max_age, want_id):
    """A track seen at t = 0, hidden at t = 1 and 2, back at t = 3 on its remembered pixels: re-identified at max_age 3,
    a new id -- in the reused slot 0, ids keep rising -- at 0 and 1."""
    slots, next_id = np.zeros((T, 5), np.int64), 1
    seen, hidden = _one_pair(0, 0, 20), np.zeros((T + 1, 1), np.int64)
    back = _one_pair(15, 5, 3)
    hidden[0, 0] = 20
    for t, (pairs, n) in enumerate(((seen, 1), (hidden, 0), (hidden, 0), (back, 1))):
        if slots[0, 0] == 0 and t:                                          # the track has ended: nothing is remembered
            pairs = _one_pair(0, 0, int(pairs[:, :n].sum())) if n else np.zeros((T + 1, 1), np.int64)
        got = _assoc_both(pairs, n, [CAR] * n, [1] * n, slots, next_id, 0.3, max_age, t)
        slots, next_id = got["slots"].astype(np.int64), got["next_id"]
    assert got["inst"][0, :2].tolist() == [0, want_id] and got["inst"][0, 4] == (want_id != 1)
    assert slots[0].tolist() == ([1, CAR, 0, 3, 2] if want_id == 1 else [2, CAR, 3, 3, 1]) and next_id == want_id + 1
    assert not slots[1:].any()


def test_association_with_257_tracks_alive_changes_nothing():
    import torch
    from centerpoly_amd.detectors import tracking
    slots = np.zeros((T, 5), np.int64)
    slots[:, 0], slots[:, 1], slots[:, 3], slots[:, 4] = 1 + np.arange(T), CAR, 4, 1
    pairs = _one_pair(0, 0, 9)
    got = tracking.associate(_dev(pairs.astype(np.int32)), 1, [CAR], [1], slots, 300, 0.3, 3, 5)
    assert got["status"] == 1 and got["next_id"] == 300 and np.array_equal(got["slots"], slots)
    with pytest.raises(ValueError, match=host.TOO_MANY):
        host.associate(pairs, 1, [CAR], [1], slots, 300, 0.3, 3, 5)
    # through the tracker: 128 + 127 tracks alive at max_age 3 (instance 0 owns pixels and is matched in the second
    # frame), two more are refused and the step changes nothing
    tr = tracking.InstanceTracker((53, 37), 0.3, 3, multiplier=1000)
    index = torch.full((37, 53), 255, dtype=torch.uint8, device="cuda")
    index[3:9, 4:20] = 0
    for _ in range(2):
        tr.step_index(index, 128, [CAR] * 128, [1] * 128)
    mem, state = tr.mem.clone(), tr.state.clone()
    with pytest.raises(ValueError, match="more than 256 tracks alive"):
        tr.step_index(index, 2, [24, 24], [1, 1])                           # two persons: no car to match, two new tracks
    assert tr.frame == 2 and torch.equal(tr.mem, mem)
    assert torch.equal(tr.state[:tracking.O_STATUS], state[:tracking.O_STATUS])
    after = tr.step_index(index, 1, [CAR], [1])                             # the tracker goes on: the car is matched
    assert after.table["track_id"].tolist() == [1] and not after.table["is_new"][0] and after.frame == 2


# -------------------------------------------------------------------------------------------------- whole steps --
W, H, N = 53, 37, 16


def _polygon_rows(t, C_of):
    """Four 16-gons at frame t: 0 and 1 (cars) cross on their way, 2 (a car) is not detected in frames 2 and 3 (it
    leaves and returns), 3 (a person) walks along the bottom.  Rows x1,y1,x2,y2,score,cls,poly,depth."""
    centres = [(8 + 7 * t, 12), (44 - 7 * t, 15), (26, 29), (8 + t, 29)]
    rows = np.zeros((4, 2 * N + 7), f32)
    ang = np.arange(N) * (2 * np.pi / N)
    for p, (cx, cy) in enumerate(centres):
        pts = np.stack([cx + 7.3 * np.cos(ang), cy + 7.3 * np.sin(ang)], 1)
        rows[p, 6:6 + 2 * N] = pts.reshape(-1)
        rows[p, 0:4] = [pts[:, 0].min(), pts[:, 1].min(), pts[:, 0].max(), pts[:, 1].max()]
        rows[p, 4] = 0.1 if p == 2 and t in (2, 3) else 0.9 - 0.1 * p
        rows[p, 5] = C_of["person" if p == 3 else "car"]
        rows[p, -1] = 5 + 3 * p
    return rows, centres


def _gt_frame(t, centres, labels, multiplier):
    """The objects as discs of radius 8 (between the two writers' drawings of the 7.3-pixel polygons) with ids
    label * multiplier + p + 1, an ignore region (10000) in the lower right corner and a crowd of cars (the bare label)
    along the top.  The walker is no object in frame 3 (a false positive) and an ignore region in frames 4 and 5
    (neither matched nor a false positive)."""
    yy, xx = np.mgrid[0:H, 0:W]
    gt = np.zeros((H, W), np.uint16)
    gt[0:3, :] = labels[0]
    gt[30:, 44:] = 10000
    for p, (cx, cy) in enumerate(centres):
        if p == 3 and t == 3:
            continue
        gt[(xx - cx) ** 2 + (yy - cy) ** 2 <= 64] = 10000 if p == 3 and t > 3 else labels[p] * multiplier + p + 1
    return gt


def build_sequence(name):
    """Six frames through instance_maps and the tracker (max_age 3 for Cityscapes, 0 for KITTI): per frame the maps,
    the TrackedFrame and the tracker's mem / state, all on the host, and the ground truth."""
    import torch
    from centerpoly_amd.detectors import tracking
    from centerpoly_amd.detectors.instances import instance_maps
    ds = tia._dataset(name)
    C_of = {name: ds.class_name.index(name) - 1 for name in ("car", "person")}
    labels = [int(ds.label_to_id[c]) for c in ("car", "car", "car", "person")]
    max_age = 3 if name == "cityscapes" else 0
    tr = tracking.InstanceTracker((W, H), 0.3, max_age)
    frames = []
    for t in range(6):
        rows, centres = _polygon_rows(t, C_of)
        maps = instance_maps(torch.from_numpy(rows).cuda(), ds, (W, H))
        tracked = tr.step(maps)
        frames.append({"maps": maps, "tracked": tracked, "mem": tr.mem.cpu().numpy().view(np.uint16).copy(),
                       "ids": tracked.ids.cpu().numpy(), "index": maps.index.cpu().numpy(),
                       "track_of_instance": tracked.track_of_instance.cpu().numpy(),
                       "gt": _gt_frame(t, centres, labels, maps.multiplier)})
    return {"name": name, "ds": ds, "tracker": tr, "frames": frames, "max_age": max_age,
            "multiplier": frames[0]["maps"].multiplier}


@pytest.fixture(scope="module", params=["cityscapes", "kitti_poly"])
def sequence(request):
    return build_sequence(request.param)


def test_whole_steps_against_the_host_statement(sequence):
    ref = host.Tracker(H, W, 0.3, sequence["max_age"], sequence["multiplier"])
    ids_of_polygon = {}
    for t, f in enumerate(sequence["frames"]):
        tab, k_tab = f["maps"].table, f["tracked"].table
        n = int(tab["n"])
        assert n == (3 if t in (2, 3) else 4) and tab["live"].all()
        want = ref.step(f["index"], n, tab["label"], tab["live"])
        inst = np.stack([k_tab[key] for key in ("slot", "track_id", "inter", "union", "is_new")], 1)
        assert np.array_equal(inst, want["inst"]) and np.array_equal(k_tab["assigned"], want["assigned"])
        assert np.array_equal(k_tab["slots"], ref.slots) and k_tab["next_id"] == ref.next_id and k_tab["status"] == 0
        assert np.array_equal(f["mem"], ref.mem) and np.array_equal(f["ids"], want["ids"])
        assert f["tracked"].frame == t and np.array_equal(f["track_of_instance"], want["inst"][:, 1])
        alive = np.flatnonzero(ref.slots[:, 0])
        assert np.array_equal(k_tab["alive"], np.concatenate([alive[:, None], ref.slots[alive]], 1))
        for k in range(n):
            ids_of_polygon.setdefault(int(tab["src"][k]), []).append(int(k_tab["track_id"][k]))
    assert sequence["tracker"].frame == 6
    # what the sequence shows: the walker keeps one id; the car that leaves returns under its id only with max_age 3
    assert len(set(ids_of_polygon[3])) == 1
    assert (len(set(ids_of_polygon[2])) == 1) == (sequence["max_age"] == 3)
    assert ref.next_id >= 5


def test_reset_restores_the_initial_state(sequence):
    import torch
    from centerpoly_amd.detectors import tracking
    tr = tracking.InstanceTracker((W, H), 0.3, sequence["max_age"])
    first = sequence["frames"][0]
    for f in sequence["frames"][:3]:
        tr.step(f["maps"])
    tr.reset()
    assert tr.frame == 0 and bool((tr.mem == -1).all())
    state = tr.state.cpu().numpy()
    assert state[tracking.O_NEXT] == 1 and not np.delete(state, tracking.O_NEXT).any()
    again = tr.step(first["maps"])
    assert np.array_equal(again.ids.cpu().numpy(), first["ids"]) and again.frame == 0
    assert np.array_equal(again.table["track_id"], first["tracked"].table["track_id"])
    assert np.array_equal(tr.mem.cpu().numpy().view(np.uint16), first["mem"])
    other = type("Maps", (), {"canvas": (W + 1, H), "table": first["maps"].table, "index": first["maps"].index,
                             "multiplier": 1000})()
    with pytest.raises(ValueError, match="canvas"):
        tr.step(other)
    with pytest.raises(ValueError, match="uint8"):
        tr.step_index(torch.zeros((H, W + 1), dtype=torch.uint8, device="cuda"), 0, [], [], 1000)


# ------------------------------------------------------------------------------------------------------ scoring --
def _same_results(got, ref, labels):
    for c in list(labels) + ["all"]:
        a, b = (got["all"], ref["all"]) if c == "all" else (got["per_class"][c], ref["per_class"][c])
        for key in ("tp", "fp", "fn", "ids"):
            assert a[key] == b[key], (c, key, a[key], b[key])
        for key in ("soft_tp", "motsa", "smotsa", "motsp"):
            assert (math.isnan(a[key]) and math.isnan(b[key])) or abs(a[key] - b[key]) <= 1e-12, (c, key, a[key], b[key])


def test_scoring_against_the_host_statement(sequence, tmp_path):
    from centerpoly_amd.datasets.evaluation import instance_level as il
    from centerpoly_amd.datasets.evaluation import tracking as mots
    protocol = il.PROTOCOLS[getattr(sequence["ds"], "ap_protocol", None) or "cityscapes"]
    assert protocol.id_multiplier == sequence["multiplier"]
    ev = mots.TrackingEvaluator(protocol, 10000)
    ref = host.Mots(sequence["multiplier"], protocol.label_ids, 10000)
    for t, f in enumerate(sequence["frames"]):
        tab = f["maps"].table
        seq = "a" if t < 5 else "b"                                         # the last frame starts another sequence
        ev.add_maps(seq, f["maps"], f["tracked"], f["gt"])
        ref.add_frame(seq, f["gt"], f["index"], int(tab["n"]), tab["label"], tab["live"], f["tracked"].table["track_id"])
    got, want = ev.results(), ref.results()
    _same_results(got, want, protocol.label_ids)
    assert want["all"]["tp"] >= 10 and want["all"]["fn"] >= 2 and want["all"]["fp"] >= 1 and got["frames"] == 6
    assert want["all"]["ids"] >= (0 if sequence["max_age"] == 3 else 1)
    with open(ev.write_json(str(tmp_path))) as fh:
        assert json.load(fh)["all"]["tp"] == want["all"]["tp"]


# ------------------------------------------------------------------------------------------------------ drivers --
def _frames(n=3):
    """Frames of 64 x 96: the first two are the same picture (every instance of the second is a track of the first),
    the others are it shifted by two pixels more each."""
    base = tia._image(64, 96, 123)
    return [base if k < 2 else np.roll(base, 2 * (k - 1), 1) for k in range(n)]


def _record_steps(monkeypatch):
    from centerpoly_amd.detectors.tracking import InstanceTracker
    seen, inner = [], InstanceTracker.step

    def recording(self, maps):
        seen.append((maps, inner(self, maps)))
        return seen[-1][1]

    monkeypatch.setattr(InstanceTracker, "step", recording)
    return seen


def _check_track_files(inst_dir, stem, maps, tracked):
    from centerpoly_amd.datasets.evaluation import instance_level as il
    assert np.array_equal(il.read_gt_ids(os.path.join(inst_dir, stem + "_trackIds.png")), tracked.ids.cpu().numpy())
    with open(os.path.join(inst_dir, stem + "_tracks.json")) as f:
        js = json.load(f)
    t = maps.table
    live = [k for k in range(t["n"]) if t["live"][k]]
    assert js["frame"] == tracked.frame and js["multiplier"] == maps.multiplier
    assert [e["track_id"] for e in js["instances"]] == tracked.table["track_id"][live].tolist()
    assert [e["label_id"] for e in js["instances"]] == t["label"][live].tolist()
    assert [e["is_new"] for e in js["instances"]] == tracked.table["is_new"][live].tolist()
    assert [e["box"] for e in js["instances"]] == t["box"][live].tolist()
    assert [f32(e["score"]) for e in js["instances"]] == t["score"][live].tolist()


def _host_replay(seen, multiplier, iou=0.3, max_age=0):
    """The host statement over the recorded maps of ONE sequence: ids and tables equal what the driver's tracker gave."""
    ref = host.Tracker(64, 96, iou, max_age, multiplier)
    for maps, tracked in seen:
        t = maps.table
        want = ref.step(maps.index.cpu().numpy(), int(t["n"]), t["label"], t["live"])
        assert np.array_equal(tracked.ids.cpu().numpy(), want["ids"])
        assert np.array_equal(tracked.table["track_id"], want["inst"][:, 1])


def test_demo_track_writes_track_files(tmp_path, monkeypatch):
    from PIL import Image
    from centerpoly_amd.opts import opts
    os.makedirs(str(tmp_path / "imgs"))
    stems = ["f_000", "f_001", "f_002"]
    for stem, img in zip(stems, _frames()):
        Image.fromarray(img[:, :, ::-1]).save(str(tmp_path / "imgs" / (stem + ".png")))
    seen = _record_steps(monkeypatch)
    with contextlib.redirect_stdout(io.StringIO()):
        opt = opts().parse(tia._args(tmp_path, "kitti_poly", ["--demo", str(tmp_path / "imgs"), "--save_ids", "--track",
                                                              "--track_max_age", "1"]))
        out = tia._module("demo").demo(opt)
    assert len(out) == 3 and len(seen) == 3 and [tr.frame for _, tr in seen] == [0, 1, 2]
    inst_dir = os.path.join(opt.save_dir, "instances")
    for stem, (maps, tracked) in zip(stems, seen):
        _check_track_files(inst_dir, stem, maps, tracked)
        assert os.path.exists(os.path.join(inst_dir, stem + "_instanceIds.png"))
    _host_replay(seen, 256, 0.3, 1)
    first, second = seen[0][1].table, seen[1][1].table
    shown = seen[1][0].table["visible"] > 0
    assert first["is_new"][seen[0][0].table["live"]].all() and shown.sum() >= 2
    assert not second["is_new"][shown].any()                                # the same picture: every shown instance is known
    assert set(second["track_id"][shown]) <= set(first["track_id"])


def _track_set(tmp):
    """Three KITTI-style frames of one drive and one of another (a directory each), with ground-truth id images of the
    frames' size: a car that moves two pixels a frame, a person, an ignore region (10000) and a crowd of cars (26)."""
    from PIL import Image
    img_dir, annot_dir, gt_dir = (os.path.join(tmp, d) for d in ("image_2", "BBoxes", "instance"))
    names = ["drive_a/000000", "drive_a/000001", "drive_a/000002", "drive_b/000003"]
    for d in (img_dir, gt_dir):
        for drive in ("drive_a", "drive_b"):
            os.makedirs(os.path.join(d, drive))
    os.makedirs(annot_dir)
    yy, xx = np.mgrid[0:64, 0:96]
    for k, (name, img) in enumerate(zip(names, _frames(4))):
        Image.fromarray(img[:, :, ::-1]).save(os.path.join(img_dir, name + ".png"))
        gt = np.full((64, 96), 7 * 256, np.uint16)
        gt[(xx - 30 - 2 * k) ** 2 + (yy - 30) ** 2 <= 144] = 26 * 256 + 1
        gt[40:60, 60:90] = 24 * 256 + 2
        gt[0:8, :] = 10000
        gt[56:, 0:30] = 26
        Image.fromarray(gt).save(os.path.join(gt_dir, name + ".png"))
    with open(os.path.join(annot_dir, "val16.json"), "w") as f:
        # absolute names, as annotation files carry them: the loader keeps the directory, which is the sequence
        json.dump({"images": [{"id": 10 + k, "file_name": os.path.join(img_dir, s + ".png"), "height": 64, "width": 96}
                              for k, s in enumerate(names)], "annotations": [], "categories": []}, f)
    return names, tia._args(tmp, "kitti_poly", ["--annot_dir", annot_dir, "--img_dir", img_dir, "--gt_dir", gt_dir,
                                                "--not_prefetch_test", "--no_mask_files", "--track", "--save_ids"])


def test_driver_track_scores_and_batches(tmp_path, monkeypatch, capsys):
    """test.py --track --gt_dir --save_ids per image and with --test_batch_size 2: the tracker starts anew where the
    directory changes, the files hold the tracker's output, the scores are the host statement's on the maps of the run,
    and the two runs give the same tables."""
    from centerpoly_amd.datasets.evaluation import instance_level as il
    from centerpoly_amd.datasets.evaluation import tracking as mots
    from centerpoly_amd.opts import opts
    names, args = _track_set(str(tmp_path))
    seen = _record_steps(monkeypatch)
    driver = tia._module("test")
    tables = []
    with contextlib.redirect_stderr(io.StringIO()):
        for batch in (1, 2):
            opt = opts().parse(args + ["--test_batch_size", str(batch)])
            opt.save_dir = str(tmp_path / ("exp_b%d" % batch))
            del seen[:]
            out = driver.run_test(opt)
            text = capsys.readouterr().out
            assert len(seen) == 4 and [tr.frame for _, tr in seen] == [0, 1, 2, 0]
            assert text.index("AP_50%") < text.index("sMOTSA")
            inst_dir = os.path.join(opt.save_dir, "instances")
            ref = host.Mots(256, il.LABEL_IDS, 10000)
            for name, (maps, tracked) in zip(names, seen):
                _check_track_files(inst_dir, os.path.basename(name), maps, tracked)
                t = maps.table
                gt = il.read_gt_ids(os.path.join(opt.gt_dir, name + ".png"))
                ref.add_frame(os.path.dirname(name), gt, maps.index.cpu().numpy(), int(t["n"]), t["label"], t["live"],
                              tracked.table["track_id"])
            _host_replay(seen[:3], 256)
            _host_replay(seen[3:], 256)
            _same_results(out["tracking"], ref.results(), il.LABEL_IDS)
            with open(os.path.join(opt.save_dir, mots.RESULT_FILE)) as f:
                assert json.load(f)["all"]["tp"] == out["tracking"]["all"]["tp"]
            by_files = mots.evaluate_result_dir(inst_dir, opt.gt_dir, protocol=il.KITTI)
            _same_results(by_files, ref.results(), il.LABEL_IDS)
            tables.append(([tr.table["track_id"].tolist() for _, tr in seen], out["tracking"]))
    assert tables[0][0] == tables[1][0]
    assert json.dumps(tables[0][1], sort_keys=True) == json.dumps(tables[1][1], sort_keys=True)

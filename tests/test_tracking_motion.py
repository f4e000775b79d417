"""Tracking with motion on the device against the host statement (tests/golden/tracking_motion_host.py), exact integer
equality: the shifted pair counting, a table whose none row is negative, the kinematics, the whole tracker on the
scenario of test_tracking_motion_cpu.py, and the drivers."""
import contextlib
import io
import json
import os
import types

import numpy as np
import pytest

import tracking_host as plain
import tracking_motion_host as host
import test_instances_api as tia
import test_tracking_motion_cpu as cpu
from test_tracking import _dev, _offset_by_one, _track_set

pytestmark = pytest.mark.gpu

T = host.T
CAR = cpu.CAR


# ---------------------------------------------------------------------------------------- cp_map_pairs_shifted --
SHAPES = {"1x1": (1, 1), "9x21": (9, 21), "37x53_unaligned": (37, 53), "64x256": (64, 256)}
TABLES = {"lds": (256, 128), "global": (1024, 255), "no_columns": (3, 0), "no_rows": (0, 0)}


def _maps(H, W, R, n, rng):
    """A 16-bit map of blocks of one value 24 wide and 3 high (whole pieces of one row, and mixed ones), with single
    pixels of other values, some values past the last row and 0xffff; a byte map of runs, some bytes past the columns."""
    values = np.concatenate([np.arange(0, R + R // 8 + 2), [0xffff] * 3])
    a = np.repeat(np.repeat(rng.choice(values, (H // 3 + 1, W // 24 + 1)), 3, 0), 24, 1)[:H, :W].copy()
    noise = rng.random_sample((H, W)) < 0.05
    a[noise] = rng.choice(values, int(noise.sum()))
    b = np.repeat(rng.randint(0, 256, (H, W // 5 + 1)), 5, 1)[:, :W].copy()
    low = rng.random_sample((H, W)) < 0.5
    b[low] = b[low] % (n + 2)
    return a.astype(np.uint16), b.astype(np.uint8)


def _shifts(H, W, R, rng):
    return {"zero": np.zeros((R, 2), np.int32),
            "constant": np.tile(np.array([[3, 1]], np.int32), (R, 1)),
            "random": np.stack([rng.randint(-(W + 3), W + 4, R), rng.randint(-(H + 3), H + 4, R)], 1).astype(np.int32),
            "negative": np.stack([-rng.randint(0, W // 2 + 2, R), -rng.randint(0, H // 2 + 2, R)], 1).astype(np.int32)}


@pytest.mark.parametrize("table", sorted(TABLES))
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_map_pairs_shifted(shape, table):
    import torch
    from centerpoly_amd.detectors import tracking
    (H, W), (R, n) = SHAPES[shape], TABLES[table]
    rng = np.random.RandomState(sum(map(ord, shape + table)))
    a, b = _maps(H, W, R, n, rng)
    place = _offset_by_one if "unaligned" in shape else _dev
    a_dev, b_dev = place(a.view(np.int16)), place(b)
    for name, shift in _shifts(H, W, R, rng).items():
        want = host.map_pairs_shifted(a, shift, b, R, n)
        got = tracking.map_pairs_shifted(a_dev, _dev(shift), b_dev, R, n)
        torch.cuda.synchronize()
        got = got.cpu().numpy()
        assert got.shape == (R + 1, n + 1) and np.array_equal(got, want), name
        # every column sum is the column's true area
        assert np.array_equal(got.sum(0), np.bincount(np.minimum(b.reshape(-1), n), minlength=n + 1)), name
        if name == "zero":
            same = tracking.map_pairs(a_dev, b_dev, R, n)
            assert torch.equal(same.cpu(), torch.from_numpy(got)) and np.array_equal(want, plain.map_pairs(a, b, R, n))
        if name == "random" and R >= 256 and H > 1:
            assert (got[:R].sum(1) == 0).sum() > (np.bincount(np.minimum(a.reshape(-1), R), minlength=R + 1)[:R] == 0).sum()


def test_a_negative_none_row():
    """Two slots with disjoint footprints of 16 pixels whose shifts put both exactly onto the one instance, which has no
    other pixel: the none row of its column is 16 - 32, and the association gives the instance to the slot of the
    smaller track id at IoU 16 / 16."""
    from centerpoly_amd.detectors import tracking
    mem = np.full((16, 40), plain.NONE, np.uint16)
    mem[2:6, 2:6], mem[2:6, 20:24] = 0, 1
    index = np.full((16, 40), 255, np.uint8)
    index[6:10, 10:14] = 0
    shift = np.zeros((T, 2), np.int32)
    shift[0], shift[1] = [8, 4], [-10, 4]
    pairs = tracking.map_pairs_shifted(_dev(mem.view(np.int16)), _dev(shift), _dev(index), T, 1)
    got = pairs.cpu().numpy()
    assert np.array_equal(got, host.map_pairs_shifted(mem, shift, index, T, 1))
    assert got[0].tolist() == [16, 0] and got[1].tolist() == [16, 0] and got[T].tolist() == [-16, 16 * 40 - 16]
    slots = np.zeros((T, 5), np.int64)
    slots[0], slots[1] = [5, CAR, 0, 0, 1], [3, CAR, 0, 0, 1]
    dev = tracking.associate(pairs, 1, [CAR], [1], slots, 6, 0.3, 1, 1)
    s, next_id, inst, assigned = plain.associate(got, 1, [CAR], [1], slots, 6, 0.3, 1, 1)
    assert dev["status"] == 0 and dev["next_id"] == next_id == 6 and np.array_equal(dev["slots"], s)
    assert np.array_equal(dev["inst"], inst) and np.array_equal(dev["assigned"], assigned)
    assert dev["inst"].tolist() == [[1, 3, 16, 16, 0]]


# -------------------------------------------------------------------------------------------------- kinematics --
def _kinematics(index_dev, n, inst, slots, status, t, kin):
    """cp_track_kinematics on host tables: the new kin [256, 6]."""
    import torch
    from centerpoly_amd import _C
    H, W = (int(v) for v in index_dev.shape)
    inst_dev = _dev(np.asarray(inst, np.int32).reshape(-1, 5)) if n else None
    slots_dev, kin_dev = _dev(np.asarray(slots, np.int32)), _dev(np.asarray(kin, np.int32))
    status_dev = _dev(np.array([status], np.int32))
    nbytes = _C.lib().cp_track_kinematics_workspace_bytes(n)
    ws = _C.workspace(nbytes, index_dev.device)
    _C.check(_C.lib().cp_track_kinematics(_C.ptr(index_dev), n, H, W, _C.ptr(inst_dev), _C.ptr(slots_dev),
                                          _C.ptr(status_dev), t, _C.ptr(kin_dev), _C.ptr(ws), nbytes, _C.stream()),
             "cp_track_kinematics")
    torch.cuda.synchronize()
    return kin_dev.cpu().numpy()


def test_kinematics_sums_past_32_bits():
    """One instance owns a 1100 x 2048 canvas: Sx = 1100 * 2047 * 2048 / 2 = 2305822720 > 2^31.  The centroid is
    (1023.5, 549.5): 16 * 1023.5 + 0.5 -> 16376 and 8792; from (100, 50) three frames ago the velocity is 16276 / 3 ->
    5425 and 8742 / 3 = 2914."""
    import torch
    Hb, Wb = 1100, 2048
    A, Sx, Sy = Hb * Wb, Hb * (Wb - 1) * Wb // 2, Wb * (Hb - 1) * Hb // 2
    assert Sx > 2 ** 31 and host.centroid16(Sx, A) == 16376 and host.centroid16(Sy, A) == 8792
    slots, kin = np.zeros((T, 5), np.int64), np.zeros((T, 6), np.int64)
    slots[0], kin[0] = [1, CAR, 0, 4, 2], [100, 50, 0, 0, 2, 1]
    index = torch.zeros((Hb, Wb), dtype=torch.uint8, device="cuda")
    got = _kinematics(index, 1, [[0, 1, 9, 9, 0]], slots, 0, 5, kin)
    assert got[0].tolist() == [16376, 8792, 5425, 2914, 5, 1] and not got[1:].any()


@pytest.mark.parametrize("offset", [False, True])
def test_kinematics_cases(offset):
    """On 12 x 21: matched tracks seen one and three frames ago whose centroids moved backwards (the quotient truncates
    toward zero), a matched track without kinematics, a new track in a slot that holds stale numbers, a new track
    without a pixel, a dead instance, a free slot with stale numbers and an occupied slot that took no instance."""
    Hs, Ws, t = 12, 21, 7
    index = np.full((Hs, Ws), 255, np.uint8)
    index[1:4, 2:7], index[5:9, 10:13], index[9:12, 0:20], index[0, 19:21], index[4, 15] = 0, 1, 2, 3, 200
    # instance:  0 -> slot 2 (g = 1)   1 -> slot 5 (g = 3)   2 -> slot 4 (no kinematics yet)   3 -> slot 1 (new)
    #            4 -> slot 7 (new, owns no pixel)   5 dead
    inst = [[2, 11, 5, 9, 0], [5, 12, 4, 8, 0], [4, 13, 3, 90, 0], [1, 20, 0, 0, 1], [7, 21, 0, 0, 1], [-1, 0, 0, 0, 0]]
    slots, kin = np.zeros((T, 5), np.int64), np.zeros((T, 6), np.int64)
    for s, track in ((1, 20), (2, 11), (3, 14), (4, 13), (5, 12), (7, 21)):
        slots[s] = [track, CAR, 0, t, 1]
    kin[1] = [999, 999, 99, 99, 2, 1]
    kin[2] = [16 * 4 + 23, 16 * 2 + 5, 1, 1, t - 1, 1]
    kin[3] = [300, 100, -40, 3, t - 2, 1]
    kin[5] = [16 * 11 + 7, 16 * 6 + 8 - 14, 0, 0, t - 3, 1]
    kin[7] = [5, 5, 5, 5, 5, 1]
    kin[9] = [1, 2, 3, 4, 5, 1]
    want = host.kinematics(index, 6, inst, slots, t, kin)
    assert want[2].tolist() == [64, 32, -23, -5, t, 1]                      # g = 1: the differences themselves
    assert want[5].tolist() == [176, 104, -2, 4, t, 1]                      # -7 / 3 -> -2 (the floor is -3), 14 / 3 -> 4
    assert want[4].tolist() == [16 * 9 + 8, 16 * 10, 0, 0, t, 1]    # x 0 .. 19, y 9 .. 11
    assert want[1].tolist() == [16 * 19 + 8, 0, 0, 0, t, 1]
    assert not want[7].any() and not want[9].any() and want[3].tolist() == kin[3].tolist()
    place = _offset_by_one if offset else _dev
    got = _kinematics(place(index), 6, inst, slots, 0, t, kin)
    assert np.array_equal(got, want)
    # with the status set nothing changes
    assert np.array_equal(_kinematics(place(index), 6, inst, slots, 1, t, kin), kin)
    # no instance at all: only the free slots are cleared
    none = _kinematics(place(index), 0, [], slots, 0, t, kin)
    assert not none[9].any() and np.array_equal(np.delete(none, 9, 0), np.delete(kin, 9, 0))


def _same_frame(tracked, tracker, want, ref, n):
    """The device step against the host statement's, every table."""
    tab = tracked.table
    pairs = tracker.pairs[:(T + 1) * (n + 1)].cpu().numpy().reshape(T + 1, n + 1)
    assert np.array_equal(pairs, want["pairs"]) and np.array_equal(tab["shift"], want["shift"])
    inst = np.stack([tab[key] for key in ("slot", "track_id", "inter", "union", "is_new")], 1)
    assert np.array_equal(inst, want["inst"]) and np.array_equal(tab["assigned"], want["assigned"])
    assert np.array_equal(tab["kin"], ref.kin) and np.array_equal(tab["slots"], ref.slots)
    assert tab["next_id"] == ref.next_id and tab["status"] == 0
    assert np.array_equal(tracker.mem.cpu().numpy().view(np.uint16), ref.mem)
    assert np.array_equal(tracked.ids.cpu().numpy(), want["ids"])


def test_a_freed_slot_is_reused_without_its_kinematics():
    """max_age 0: a track moves for two frames, is not seen in the third (its slot and its kinematics are cleared) and
    another object takes slot 0 in the fourth: no velocity, no shift in the fifth."""
    from centerpoly_amd.detectors import tracking
    Hs, Ws = 20, 40
    tr = tracking.InstanceTracker((Ws, Hs), 0.3, 0, multiplier=1000, motion=True)
    ref = host.Tracker(Hs, Ws, 0.3, 0, 1000)
    boxes = [(2, 3), (5, 4), None, (25, 9), (25, 9)]
    for t, box in enumerate(boxes):
        index = np.full((Hs, Ws), 255, np.uint8)
        n = 0
        if box is not None:
            index[box[1]:box[1] + 8, box[0]:box[0] + 10], n = 0, 1
        want = ref.step(index, n, [CAR] * n, [1] * n)
        tracked = tr.step_index(_dev(index), n, [CAR] * n, [1] * n)
        _same_frame(tracked, tr, want, ref, n)
        if t == 1:
            assert tracked.table["kin"][0].tolist() == [16 * 9 + 8, 16 * 7 + 8, 48, 16, 1, 1]
            assert tracked.table["velocity"].tolist() == [[3.0, 1.0]] and tracked.table["centroid"].tolist() == [[9.5, 7.5]]
        if t == 2:
            assert not tracked.table["kin"].any() and not tracked.table["slots"].any()
        if t >= 3:
            assert tracked.table["slot"].tolist() == [0] and tracked.table["track_id"].tolist() == [2]
            assert tracked.table["kin"][0].tolist() == [16 * 29 + 8, 16 * 12 + 8, 0, 0, t, 1]
            assert not tracked.table["shift"].any()


def test_more_than_256_tracks_alive_changes_nothing():
    """16 x 16, max_age 2: 128 one-pixel cars in each of two frames, then 128 persons: no slot is free, the step is
    refused and kin, slots and mem stay as they were."""
    import torch
    from centerpoly_amd.detectors import tracking
    tr = tracking.InstanceTracker((16, 16), 0.3, 2, multiplier=1000, motion=True)
    ref = host.Tracker(16, 16, 0.3, 2, 1000)
    for t in range(2):
        index = np.full((256,), 255, np.uint8)
        index[128 * t:128 * t + 128] = np.arange(128)
        index = index.reshape(16, 16)
        want = ref.step(index, 128, [CAR] * 128, [1] * 128)
        _same_frame(tr.step_index(_dev(index), 128, [CAR] * 128, [1] * 128), tr, want, ref, 128)
    assert (ref.slots[:, 0] != 0).all() and (ref.kin[:, 5] == 1).all()
    mem, state = tr.mem.clone(), tr.state.clone()
    with pytest.raises(ValueError, match=plain.TOO_MANY):
        ref.step(index, 128, [24] * 128, [1] * 128)
    with pytest.raises(ValueError, match="more than 256 tracks alive"):
        tr.step_index(_dev(index), 128, [24] * 128, [1] * 128)
    assert tr.frame == 2 and torch.equal(tr.mem, mem)
    assert torch.equal(tr.state[:tracking.O_STATUS], state[:tracking.O_STATUS])
    kin = tr.state[tracking.O_KIN:tracking.O_SHIFT].cpu().numpy().reshape(T, 6)
    assert torch.equal(tr.state[tracking.O_KIN:tracking.O_SHIFT], state[tracking.O_KIN:tracking.O_SHIFT])
    assert np.array_equal(kin, ref.kin) and np.array_equal(tr.mem.cpu().numpy().view(np.uint16), ref.mem)


# ----------------------------------------------------------------------------------------------- whole tracker --
def test_the_tracker_on_the_scenario():
    """The eleven frames of test_tracking_motion_cpu.scenario: with motion every table of every frame is the host
    statement's and the mover keeps track 1; without, the tracker is tracking_host.Tracker and the mover returns as
    track 3 at frame 8."""
    from centerpoly_amd.detectors import tracking
    canvas = (cpu.W, cpu.H)
    moving = tracking.InstanceTracker(canvas, cpu.IOU, cpu.MAX_AGE, multiplier=cpu.MULTIPLIER, motion=True)
    still = tracking.InstanceTracker(canvas, cpu.IOU, cpu.MAX_AGE, multiplier=cpu.MULTIPLIER)
    assert moving.motion and not still.motion and still.state.numel() == tracking.STATE_INTS
    ref_moving = host.Tracker(cpu.H, cpu.W, cpu.IOU, cpu.MAX_AGE, cpu.MULTIPLIER)
    ref_still = plain.Tracker(cpu.H, cpu.W, cpu.IOU, cpu.MAX_AGE, cpu.MULTIPLIER)
    ids = {"moving": [], "still": []}
    for t, (_, index, n, k) in enumerate(cpu.scenario()):
        label, live, index_dev = [CAR] * n, [1] * n, _dev(index)
        want = ref_moving.step(index, n, label, live)
        tracked = moving.step_index(index_dev, n, label, live)
        _same_frame(tracked, moving, want, ref_moving, n)
        want = ref_still.step(index, n, label, live)
        other = still.step_index(index_dev, n, label, live)
        tab = other.table
        assert "kin" not in tab and "shift" not in tab and "centroid" not in tab
        inst = np.stack([tab[key] for key in ("slot", "track_id", "inter", "union", "is_new")], 1)
        assert np.array_equal(inst, want["inst"]) and np.array_equal(tab["slots"], ref_still.slots)
        assert np.array_equal(still.pairs[:(T + 1) * (n + 1)].cpu().numpy().reshape(T + 1, n + 1), want["pairs"])
        assert np.array_equal(still.mem.cpu().numpy().view(np.uint16), ref_still.mem)
        assert np.array_equal(other.ids.cpu().numpy(), want["ids"])
        if k is not None:
            ids["moving"].append(int(tracked.table["track_id"][k]))
            ids["still"].append(int(tab["track_id"][k]))
        if t == 8:
            assert tracked.table["shift"][0].tolist() == [30, 5] and tab["track_id"][k] == 3
            assert tracked.table["inter"][k] == tracked.table["union"][k] == 400
    assert ids["moving"] == [1] * 7 and ids["still"] == [1, 1, 1, 1, 3, 3, 3]


# ----------------------------------------------------------------------------------------------------- drivers --
def _fake_maps(index, n):
    return types.SimpleNamespace(canvas=(index.shape[1], index.shape[0]), index=_dev(index), multiplier=1000,
                                 table={"n": n, "label": np.array([CAR] * n), "live": np.array([True] * n),
                                        "score": np.linspace(0.9, 0.5, n).astype(np.float32),
                                        "box": np.array([[0, 0, 1, 1]] * n).reshape(n, 4)},
                                 names={CAR: "car"})


def test_sequence_tracker_resets_the_kinematics_and_the_files_hold_them(tmp_path):
    from centerpoly_amd.detectors import tracking
    seq = tracking.SequenceTracker(cpu.IOU, cpu.MAX_AGE, motion=True)
    frames = cpu.scenario()
    for t in range(3):
        key, tracked = seq.step("drive_a/%06d.png" % t, _fake_maps(frames[t][1], 2))
    assert key == "drive_a/" and tracked.frame == 2 and seq.tracker.motion
    assert tracked.table["kin"][0].tolist() == [16 * 25 + 8, 16 * 15 + 8, 96, 16, 2, 1]
    assert tracked.table["shift"][0].tolist() == [6, 1]
    maps = _fake_maps(frames[2][1], 2)
    with open(tracking.save_tracks(maps, tracked, str(tmp_path), "f")[0]) as fh:
        entries = json.load(fh)["instances"]
    assert [e["centroid"] for e in entries] == [[25.5, 15.5], [109.5, 29.5]]
    assert [e["velocity"] for e in entries] == [[6.0, 1.0], [0.0, 0.0]]
    assert [e["track_id"] for e in entries] == [1, 2] and sorted(entries[0]) == sorted(
        ["track_id", "label_id", "class_name", "score", "box", "is_new", "centroid", "velocity"])
    tracker = seq.tracker
    key, tracked = seq.step("drive_b/%06d.png" % 3, _fake_maps(frames[3][1], 2))
    assert key == "drive_b/" and seq.tracker is tracker and tracked.frame == 0
    assert tracked.table["is_new"].all() and tracked.table["track_id"].tolist() == [1, 2]
    assert tracked.table["kin"][0].tolist() == [16 * 31 + 8, 16 * 16 + 8, 0, 0, 0, 1]
    assert not tracked.table["kin"][2:].any() and not tracked.table["shift"].any()
    plain_seq = tracking.SequenceTracker(cpu.IOU, cpu.MAX_AGE)
    assert "kin" not in plain_seq.step("drive_a/000000.png", _fake_maps(frames[0][1], 2))[1].table


def test_driver_runs_with_track_motion(tmp_path):
    """test.py --track --track_motion --track_max_age 1 on the frames of the --track driver test: it runs through, the
    trackers it makes predict, and it writes resultTracking.json and the tracks with their kinematics.  No score is
    asserted: the detections of a seeded model carry no motion."""
    from centerpoly_amd.datasets.evaluation import tracking as mots
    from centerpoly_amd.opts import opts
    names, args = _track_set(str(tmp_path))
    driver = tia._module("test")
    with contextlib.redirect_stderr(io.StringIO()), contextlib.redirect_stdout(io.StringIO()):
        opt = opts().parse(args + ["--track_motion", "--track_max_age", "1"])
        opt.save_dir = str(tmp_path / "exp_motion")
        out = driver.run_test(opt)
    assert opt.track_motion is True and "tracking" in out
    with open(os.path.join(opt.save_dir, mots.RESULT_FILE)) as f:
        assert json.load(f)["all"]["tp"] == out["tracking"]["all"]["tp"]
    for name in names:
        with open(os.path.join(opt.save_dir, "instances", os.path.basename(name) + "_tracks.json")) as f:
            js = json.load(f)
        assert js["instances"] and all(len(e["centroid"]) == 2 and len(e["velocity"]) == 2 for e in js["instances"])
        assert js["frame"] == (0 if name.startswith("drive_b") else int(os.path.basename(name)))

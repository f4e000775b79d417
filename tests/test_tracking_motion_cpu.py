"""Tracking with motion without a GPU: the options, the host statement (tests/golden/tracking_motion_host.py) on the
scenario that shows what a constant-velocity prediction is for, the entry points' argument checks, and the result file
without motion."""
import contextlib
import ctypes
import io
import json
import types

import numpy as np
import pytest

import tracking_host as plain
import tracking_motion_host as host

CAR = 26
H, W = 48, 128
FRAMES, HIDDEN = 11, (4, 5, 6, 7)
IOU, MAX_AGE, MULTIPLIER = 0.3, 5, 1000


def scenario():
    """Eleven frames of 48 x 128, label 26: [(gt ids, index, n, k of the mover or None)].  A 20 x 20 square starts at
    (4, 4) and moves (6, 1) pixels a frame; it is seen in frames 0 .. 3, hidden in 4 .. 7 and seen again in 8 .. 10.  A
    parked square of the same label at (100, 20) is seen in every frame.  The mover is instance 0 where it is seen; the
    ground truth holds both objects in every frame, ids 26001 (the mover) and 26002.
    Consecutive sightings overlap by 14 x 19 of 2 * 400 - 266 pixels, IoU 0.498; at frame 8 the mover lies 30 pixels to
    the right of where it was last seen, more than its size."""
    frames = []
    for t in range(FRAMES):
        gt, index = np.zeros((H, W), np.uint16), np.full((H, W), 255, np.uint8)
        x, y = 4 + 6 * t, 4 + t
        gt[y:y + 20, x:x + 20] = CAR * MULTIPLIER + 1
        gt[20:40, 100:120] = CAR * MULTIPLIER + 2
        seen = t not in HIDDEN
        if seen:
            index[y:y + 20, x:x + 20] = 0
        index[20:40, 100:120] = 1 if seen else 0
        frames.append((gt, index, 2 if seen else 1, 0 if seen else None))
    return frames


def run_host(tracker):
    """(ids of the mover over its visible frames, MOTS counts) of a host tracker over the scenario."""
    mots = plain.Mots(MULTIPLIER, (CAR,), 10000)
    mover = []
    for gt, index, n, k in scenario():
        out = tracker.step(index, n, [CAR] * n, [1] * n)
        mots.add_frame("s", gt, index, n, [CAR] * n, [1] * n, out["inst"][:, 1])
        if k is not None:
            mover.append(int(out["inst"][k, 1]))
    return mover, mots.results()["all"]


def _parse(args):
    from centerpoly_amd.opts import opts
    with contextlib.redirect_stdout(io.StringIO()):
        return opts().parse(args)


def test_options():
    assert _parse(["polydet"]).track_motion is False
    assert _parse(["polydet", "--track"]).track_motion is False
    opt = _parse(["polydet", "--track", "--track_motion", "--track_max_age", "2"])
    assert opt.track is True and opt.track_motion is True and opt.track_max_age == 2
    err = io.StringIO()
    with pytest.raises(SystemExit), contextlib.redirect_stderr(err):
        _parse(["polydet", "--track_motion"])
    assert "--track" in err.getvalue().replace("--track_motion", "")


def test_host_statement_on_the_scenario():
    """Without motion the mover returns 30 pixels from its remembered pixels and starts track 3 (the parked square is
    track 2): one identity switch.  With motion its velocity is (96, 16) / 16 pixels a frame from frame 1 on, the shift
    at frame 8 is five frames of it, (30, 5), the predicted pixels are the mover's, and it keeps track 1."""
    ids_plain, res_plain = run_host(plain.Tracker(H, W, IOU, MAX_AGE, MULTIPLIER))
    tracker = host.Tracker(H, W, IOU, MAX_AGE, MULTIPLIER)
    ids_motion, res_motion = run_host(tracker)
    assert ids_plain == [1, 1, 1, 1, 3, 3, 3]
    assert ids_motion == [1] * 7
    assert res_plain["ids"] == 1 and res_motion["ids"] == 0
    for key in ("tp", "fp", "fn"):
        assert res_plain[key] == res_motion[key], key
    assert res_plain["tp"] == 7 + 11 and res_plain["fn"] == 4 and res_plain["fp"] == 0
    # the mover's centroid at frame 10 is (64 + 9.5, 14 + 9.5) and its velocity (6, 1), in 1/16 pixel
    assert tracker.kin[0].tolist() == [16 * 73 + 8, 16 * 23 + 8, 96, 16, 10, 1]
    assert tracker.kin[1].tolist() == [16 * 109 + 8, 16 * 29 + 8, 0, 0, 10, 1] and not tracker.kin[2:].any()


def test_host_statement_by_hand():
    """Step 1 rounds half up and clamps; step 2 clips at the canvas and lets row R go negative; step 4 truncates the
    velocity toward zero."""
    slots, kin = np.zeros((host.T, 5), np.int64), np.zeros((host.T, 6), np.int64)
    slots[0], slots[1], slots[2] = [1, CAR, 0, 0, 1], [2, CAR, 0, 0, 1], [3, CAR, 0, 0, 1]
    kin[0], kin[1], kin[2] = [0, 0, 8, -8, 2, 1], [0, 0, -24, 40, 2, 1], [0, 0, 9999, -9999, 2, 0]
    kin[3] = [0, 0, 50, 50, 2, 1]                                           # a free slot does not move
    shift = host.predict(slots, kin, 3, 10, 20)
    # 8 / 16 = 0.5 -> 1, -0.5 -> 0; -1.5 -> -1, 2.5 -> 3; not valid -> 0
    assert shift[:4].tolist() == [[1, 0], [-1, 3], [0, 0], [0, 0]]
    kin[0, 2:4] = [16 * 1000, -16 * 1000]
    assert host.predict(slots, kin, 3, 10, 20)[0].tolist() == [20, -10]
    # two 1 x 2 footprints moved onto one instance of two pixels; a third leaves the canvas
    a = np.full((2, 6), plain.NONE, np.int64)
    a[0, 0:2], a[1, 4:6], a[1, 0] = 0, 1, 2
    b = np.full((2, 6), 255, np.uint8)
    b[0, 2:4] = 0
    pairs = host.map_pairs_shifted(a, [[2, 0], [-2, -1], [-1, 0]], b, 3, 1)
    assert pairs.tolist() == [[2, 0], [2, 0], [0, 0], [-2, 10]]
    assert pairs.sum(0).tolist() == [2, 10] and pairs.sum(1)[:3].tolist() == [2, 2, 0]
    # an instance whose centroid moved by (-7, +7) sixteenths in 3 frames: -2 and +2, not -3
    index = np.full((2, 6), 255, np.uint8)
    index[0, 2:4] = 0                                                       # centroid (2.5, 0) -> (40, 0)
    old = np.zeros((host.T, 6), np.int64)
    old[0] = [47, -7, 5, 5, 1, 1]
    new = host.kinematics(index, 1, [[0, 1, 2, 2, 0]], slots, 4, old)
    assert new[0].tolist() == [40, 0, -2, 2, 4, 1] and not new[1:].any()


FAKE = ctypes.c_void_p(0x10000)                                             # never dereferenced: every call is refused
ODD, OFF2, OFF4 = ctypes.c_void_p(0x10001), ctypes.c_void_p(0x10002), ctypes.c_void_p(0x10004)
EINVAL, EUNSUPPORTED, EWORKSPACE = -1, -2, -3


def test_map_pairs_shifted_refusals():
    from centerpoly_amd import _C
    f = _C.lib().cp_map_pairs_shifted
    good = [FAKE, FAKE, 4, FAKE, 4, 8, 8, FAKE, None]

    def call(**change):
        args = list(good)
        for name, value in change.items():
            args[("a", "shift", "R", "b", "n", "H", "W", "pairs").index(name)] = value
        return f(*args)

    for change in ({"H": 0}, {"W": 0}, {"H": -3}, {"R": -1}, {"n": -1}, {"a": None}, {"b": None}, {"pairs": None},
                   {"shift": None}, {"a": ODD}, {"shift": OFF2}, {"pairs": OFF2}):
        assert call(**change) == EINVAL, change
    for change in ({"R": 1025}, {"n": 256}, {"H": 65536, "W": 32768}):
        assert call(**change) == EUNSUPPORTED, change
        assert call(a=None, b=None, pairs=None, shift=None, **change) == EUNSUPPORTED, change   # as cp_map_pairs orders them


def test_track_predict_refusals():
    from centerpoly_amd import _C
    f = _C.lib().cp_track_predict
    for args in ([None, FAKE, 0, 8, 8, FAKE], [FAKE, None, 0, 8, 8, FAKE], [FAKE, FAKE, 0, 8, 8, None],
                 [OFF2, FAKE, 0, 8, 8, FAKE], [FAKE, OFF2, 0, 8, 8, FAKE], [FAKE, FAKE, 0, 8, 8, OFF2],
                 [FAKE, FAKE, -1, 8, 8, FAKE], [FAKE, FAKE, 0, 0, 8, FAKE], [FAKE, FAKE, 0, 8, 0, FAKE]):
        assert f(*(args + [None])) == EINVAL, args


def test_track_kinematics_refusals():
    from centerpoly_amd import _C
    L = _C.lib()
    assert [L.cp_track_kinematics_workspace_bytes(n) for n in (0, 1, 128)] == [0, 24, 3072]
    names = ("index", "n", "H", "W", "inst", "slots", "status", "t", "kin", "workspace", "bytes")
    good = [FAKE, 2, 8, 8, FAKE, FAKE, FAKE, 0, FAKE, FAKE, 48, None]

    def call(**change):
        args = list(good)
        for name, value in change.items():
            args[names.index(name)] = value
        return L.cp_track_kinematics(*args)

    for change in ({"H": 0}, {"W": 0}, {"n": -1}, {"t": -1}, {"index": None}, {"inst": None}, {"slots": None},
                   {"status": None}, {"kin": None}, {"inst": OFF2}, {"slots": OFF2}, {"status": OFF2}, {"kin": OFF2},
                   {"workspace": OFF4}):
        assert call(**change) == EINVAL, change
    for change in ({"n": 129}, {"H": 65536, "W": 32768}, {"H": 1, "W": (1 << 26) + 1}, {"H": (1 << 26) + 1, "W": 1}):
        assert call(**change) == EUNSUPPORTED, change
    for change in ({"workspace": None}, {"bytes": 47}, {"bytes": 0}, {"n": 128, "bytes": 3071}):
        assert call(**change) == EWORKSPACE, change


def test_save_tracks_without_motion_writes_the_file_as_before(tmp_path):
    from centerpoly_amd.detectors import tracking
    maps = types.SimpleNamespace(table={"n": 2, "live": np.array([True, True]), "label": np.array([CAR, 24]),
                                        "score": np.array([0.5, 0.25], np.float32),
                                        "box": np.array([[0, 0, 1, 1], [2, 1, 3, 2]])},
                                 names={CAR: "car", 24: "person"}, canvas=(4, 3))
    ids = np.zeros((3, 4), np.int32)
    table = {"track_id": np.array([7, 9]), "is_new": np.array([True, False])}
    tracked = types.SimpleNamespace(table=table, frame=3, multiplier=1000, ids=ids)
    path = tracking.save_tracks(maps, tracked, str(tmp_path), "f")[0]
    want = {"frame": 3, "width": 4, "height": 3, "multiplier": 1000, "instances": [
        {"track_id": 7, "label_id": CAR, "class_name": "car", "score": 0.5, "box": [0, 0, 1, 1], "is_new": True},
        {"track_id": 9, "label_id": 24, "class_name": "person", "score": 0.25, "box": [2, 1, 3, 2], "is_new": False}]}
    with open(path) as fh:
        assert fh.read() == json.dumps(want)
    # the tables of a tracker with motion add the two keys and change nothing else
    table.update({"centroid": np.array([[1.5, 0.25], [8.0, 2.0]]), "velocity": np.array([[-0.5, 0.0], [6.0, 1.0]])})
    tracking.save_tracks(maps, tracked, str(tmp_path), "f")
    want["instances"][0].update({"centroid": [1.5, 0.25], "velocity": [-0.5, 0.0]})
    want["instances"][1].update({"centroid": [8.0, 2.0], "velocity": [6.0, 1.0]})
    with open(path) as fh:
        assert fh.read() == json.dumps(want)

"""cp_instance_map: the depth-resolved merge of an image's masks into one map with its per-instance tables.

CPU: the host restatement (tests/golden/instance_map_host.py) pinned by a hand-written case, the entry refusals with no
device, the new options, the id images' PNG round trip.  GPU: the kernel against the restatement, all six outputs
equal, on shapes that take every path (a mask one byte off a 16-byte boundary, one pixel, a canvas narrower than a
piece, several tiles with partial ones, n = 0 and n = 128)."""
import contextlib
import ctypes
import functools
import io
import os

import numpy as np
import pytest

import instance_map_host as host
from centerpoly_amd import _C

TH, TW = 16, 256                                             # the kernel's tile (csrc/instance_map.hip)
NAN = float("nan")


# ------------------------------------------------------------------------------------------------------- CPU --
def _hand_case():
    """6 x 8, three overlapping masks: 0 a 3 x 4 block, 1 a 3 x 4 block one row down and two columns right and NEARER
    (it wins the overlap), 2 the whole column 4, farthest, its bounds cutting row 0 and reaching below the canvas."""
    masks = np.zeros((3, 6, 8), np.uint8)
    masks[0, 1:4, 1:5] = 255
    masks[1, 2:5, 3:7] = 1
    masks[2, :, 4] = 255
    bounds = np.array([[0, 0, 7, 5], [3, 2, 6, 4], [4, 1, 4, 9]], np.int32)
    return masks, np.array([1, 1, 1], np.uint8), np.array([26, 26, 24], np.int32), \
        np.array([2.0, 1.0, 3.0], np.float32), bounds


def test_host_restatement_on_a_hand_written_case():
    masks, flags, label, prio, bounds = _hand_case()
    index, ids, labels, value, visible, box = host.instance_map(masks, flags, 1, None, 0, label, prio, bounds, 1000, 0)
    _ = 255
    assert index.tolist() == [[_, _, _, _, _, _, _, _],
                              [_, 0, 0, 0, 0, _, _, _],
                              [_, 0, 0, 1, 1, 1, 1, _],
                              [_, 0, 0, 1, 1, 1, 1, _],
                              [_, _, _, 1, 1, 1, 1, _],
                              [_, _, _, _, 2, _, _, _]]
    assert value.tolist() == [26000, 26001, 24000]
    assert ids.tolist() == [[0, 0, 0, 0, 0, 0, 0, 0],
                            [0, 26000, 26000, 26000, 26000, 0, 0, 0],
                            [0, 26000, 26000, 26001, 26001, 26001, 26001, 0],
                            [0, 26000, 26000, 26001, 26001, 26001, 26001, 0],
                            [0, 0, 0, 26001, 26001, 26001, 26001, 0],
                            [0, 0, 0, 0, 24000, 0, 0, 0]]
    assert labels.tolist() == [[0, 0, 0, 0, 0, 0, 0, 0],
                               [0, 26, 26, 26, 26, 0, 0, 0],
                               [0, 26, 26, 26, 26, 26, 26, 0],
                               [0, 26, 26, 26, 26, 26, 26, 0],
                               [0, 0, 0, 26, 26, 26, 26, 0],
                               [0, 0, 0, 0, 24, 0, 0, 0]]
    assert visible.tolist() == [8, 12, 1]
    assert box.tolist() == [[1, 1, 4, 3], [3, 2, 6, 4], [4, 5, 4, 5]]
    # without priorities the earlier slot wins the overlap; without bounds column 4 shows in row 0 too
    index = host.instance_map(masks, flags, 1, None, 0, label, None, None, 1000, 0)[0]
    assert index[2].tolist() == [_, 0, 0, 0, 0, 1, 1, _] and index[0].tolist() == [_, _, _, _, 2, _, _, _]
    # a NaN sorts last, a tie goes to the earlier slot, a dead instance neither wins nor counts in the ordinals
    index, _i, _l, value, visible, box = host.instance_map(masks, np.array([0, 1, 1], np.uint8), 1, None, 0,
                                                           np.array([26, 26, 26], np.int32),
                                                           np.array([0.0, NAN, 5.0], np.float32), None, 256, 9)
    assert value.tolist() == [-1, 26 * 256, 26 * 256 + 1] and visible.tolist() == [0, 9, 6]
    assert box[0].tolist() == [8, 6, -1, -1] and index[2].tolist() == [_, _, _, 1, 2, 1, 1, _] and _i[0, 0] == 9


def _call(n=3, H=6, W=8, multiplier=1000, index=True, ws_bytes=None, ws=True):
    """cp_instance_map on HOST buffers: every refusal returns before the device is touched."""
    L = _C.lib()
    buf = (ctypes.c_uint8 * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    need = L.cp_instance_map_workspace_bytes(min(max(n, 0), 128), 6, 8)
    return L.cp_instance_map(p, n, H, W, p, 1, None, 0, p, None, None, multiplier, 0, p if index else None, None, None,
                             p, p, p, p if ws else None, need if ws_bytes is None else ws_bytes, None)


def test_entry_refusals_without_a_device():
    L = _C.lib()
    need = L.cp_instance_map_workspace_bytes(128, 1024, 2048)
    assert 0 < need <= 1 << 16
    assert _call(n=129) == -2                                              # CP_EUNSUPPORTED
    assert _call(H=65536, W=32768) == -2                                   # H * W = 2^31
    assert _call(multiplier=0) == -1                                       # CP_EINVAL
    assert _call(index=False) == -1
    assert _call(n=-1) == -1 and _call(H=0) == -1
    assert _call(ws_bytes=need - 1) == -3 and _call(ws=False) == -3         # CP_EWORKSPACE


def test_save_options_parse_and_default_off():
    from centerpoly_amd.opts import opts
    with contextlib.redirect_stdout(io.StringIO()):
        off = opts().parse(["polydet"])
        on = opts().parse(["polydet", "--save_ids", "--save_masks", "--test_batch_size", "2"])
    assert off.save_ids is False and off.save_masks is False
    assert on.save_ids is True and on.save_masks is True and on.test_batch_size == 2


def test_id_images_round_trip_and_refuse_what_does_not_fit(tmp_path):
    """save_ids on host tensors: the 16-bit and the 8-bit PNG read back equal; 65536 raises and names the file."""
    import json

    import torch
    from PIL import Image
    from centerpoly_amd.datasets.evaluation import instance_level as il
    from centerpoly_amd.detectors import instances
    masks, flags, label, prio, bounds = _hand_case()
    index, ids, labels, value, visible, box = host.instance_map(masks, flags, 1, None, 0, label, prio, bounds, 1000, 0)
    table = {"n": 3, "src": np.array([5, 6, 7]), "label": label, "conf": np.array([0.5, 0.25, 1.0], np.float32),
             "count": np.array([12, 12, 6]), "live": value >= 0, "value": value, "visible": visible, "box": box,
             "score": np.array([0.5, 0.25, 0.875], np.float32), "poly": np.zeros((3, 4, 2), np.int32)}
    maps = instances.InstanceMaps("cityscapes", (8, 6), torch.from_numpy(index), torch.from_numpy(ids),
                                  torch.from_numpy(labels), torch.from_numpy(masks), table, {24: "person", 26: "car"},
                                  1000)
    paths = instances.save_ids(maps, str(tmp_path / "instances"), "frame")
    assert [os.path.basename(p) for p in paths] == ["frame_instanceIds.png", "frame_labelIds.png", "frame.json"]
    assert Image.open(paths[0]).mode in ("I;16", "I") and Image.open(paths[1]).mode == "L"
    assert np.array_equal(il.read_gt_ids(paths[0]), ids) and np.array_equal(np.array(Image.open(paths[1])), labels)
    js = json.load(open(paths[2]))
    assert [e["value"] for e in js["instances"]] == [26000, 26001, 24000]
    assert js["instances"][1] == {"label_id": 26, "class_name": "car", "score": 0.25, "confidence": 0.25,
                                  "value": 26001, "visible": 12, "box": [3, 2, 6, 4], "source_row": 6,
                                  "polygon": [[0, 0]] * 4}
    maps.ids = torch.from_numpy(np.where(ids == 24000, 65536, ids).astype(np.int32))
    with pytest.raises(ValueError, match="other_instanceIds.png.*65536"):
        instances.save_ids(maps, str(tmp_path / "instances"), "other")


# ------------------------------------------------------------------------------------------------------- GPU --
SHAPES = [(5, 37, 53), (128, 64, 96), (1, 1, 1), (3, 200, 3), (17, 3 * TH + 5, 3 * TW + 7)]
MIN_COUNT = 100


@functools.lru_cache(maxsize=None)
def _inputs(n, H, W, variant):
    """Seeded inputs, made once per case and never written to.  Slot 0 is live and nearest, slot 1 (n >= 3) live and
    lies wholly under slot 0, slot 2 is dead, covers the whole canvas and sorts first.  `plain`: no counts, no prio,
    no bounds, the masked bit is bit 1.  `full`: counts at MIN_COUNT and MIN_COUNT + 1, prio with ties and a NaN, bounds
    of every kind (exact, tighter than the mask, empty, reaching outside the canvas, and NULL-like whole canvas)."""
    rng = np.random.RandomState(1000 * n + 10 * H + W + (7 if variant == "full" else 0))
    full = variant == "full"
    bit = 1 if full else 2
    masks = np.zeros((n, H, W), np.uint8)
    for i in range(n):
        h, w = int(rng.randint(1, H + 1)), int(rng.randint(1, W + 1))
        if i % 4 == 3:                                                     # a small one: about 1 % of the canvas
            h, w = max(1, h // 8), max(1, w // 8)
        y, x = int(rng.randint(0, H - h + 1)), int(rng.randint(0, W - w + 1))
        masks[i, y:y + h, x:x + w] = rng.choice(np.array([0, 1, 255], np.uint8), (h, w), p=[0.2, 0.4, 0.4])
    flags = rng.choice(np.array([0, 1, 2, 3], np.uint8), n)
    label = rng.randint(1, 5, n).astype(np.int32)                          # four labels: the ordinals repeat
    counts = (MIN_COUNT + rng.randint(0, 2, n)).astype(np.int32) if full else None
    prio = rng.randint(0, 4, n).astype(np.float32) if full else None       # many ties
    if full and n > 4:
        prio[4] = NAN
    if full and n > 9:
        prio[9] = NAN
    flags[0] = 3
    masks[0, :max(1, H // 2), :max(1, W // 2)] = 255
    if full:
        counts[0] = MIN_COUNT + 1
        prio[0] = -1.0
    if n >= 3:
        flags[1], flags[2] = 3, 3 - bit                                    # 2 lacks the masked bit
        masks[1] = 0
        masks[1, :max(1, H // 4), :max(1, W // 4)] = 1
        masks[2] = 255
        label[1] = label[0]
        if full:
            counts[1] = MIN_COUNT + 1
            prio[1], prio[2] = 0.0, -2.0
    bounds = None
    if full:
        bounds = np.zeros((n, 4), np.int32)
        for i in range(n):
            ys, xs = np.nonzero(masks[i])
            exact = [xs.min(), ys.min(), xs.max(), ys.max()] if len(ys) else [0, 0, -1, -1]
            kind = 0 if i < 3 else i % 5
            bounds[i] = (exact, [exact[0] + 1, exact[1] + 1, exact[2] - 2, exact[3] - 1], [W // 2, 0, W // 2 - 1, H - 1],
                         [-5, -7, W + 5, H + 9], [0, 0, W - 1, H - 1])[kind]
    arrays = dict(masks=masks, flags=flags, label=label, counts=counts, prio=prio, bounds=bounds)
    for a in arrays.values():
        if a is not None:
            a.setflags(write=False)
    want = host.instance_map(masks, flags, bit, counts, MIN_COUNT, label, prio, bounds, 1000, 0)
    for a in want:
        a.setflags(write=False)
    return arrays, bit, want


def _device_map(a, bit, offset=0, background=0, multiplier=1000, want_ids=True, want_labels=True):
    import torch
    from centerpoly_amd.detectors import instances
    n, H, W = a["masks"].shape
    buf = torch.zeros(n * H * W + 32, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    masks = buf[offset:offset + n * H * W].view(n, H, W)
    masks.copy_(torch.from_numpy(np.array(a["masks"])))
    up = lambda v: None if v is None else torch.from_numpy(np.array(v)).cuda()      # noqa: E731
    out = instances.instance_map(masks, up(a["flags"]), up(a["label"]), bit, up(a["counts"]), MIN_COUNT, up(a["prio"]),
                                 up(a["bounds"]), multiplier, background, want_ids, want_labels)
    torch.cuda.synchronize()
    return [None if t is None else t.cpu().numpy() for t in out]


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["plain", "full"])
@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%dx%d" % s for s in SHAPES])
def test_kernel_equals_the_restatement(shape, variant):
    import torch
    n, H, W = shape
    a, bit, want = _inputs(n, H, W, variant)
    offset = 1 if shape == SHAPES[0] else 0                                # one byte off a 16-byte boundary
    got = _device_map(a, bit, offset)
    for name, g, w in zip(("index", "ids", "labels", "value", "visible", "box"), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), name
    again = _device_map(a, bit, offset)
    assert all(np.array_equal(g, h) for g, h in zip(got, again))           # the same bits on every run
    index, ids, labels, value, visible, box = got
    assert int(visible.sum()) == int((index != 255).sum())
    live = value >= 0
    assert live[0] and visible[0] > 0
    if n >= 3:                                                             # hidden completely; dead over live ones
        assert live[1] and visible[1] == 0 and box[1].tolist() == [W, H, -1, -1]
        assert not live[2] and value[2] == -1 and visible[2] == 0 and not (index == 2).any()
        assert value[1] == value[0] + 1
    if n >= 17:
        assert (~live).sum() >= 3 and live.sum() >= 4 and (visible[live] > 0).sum() >= 3
    # cp_id_histogram of the id image counts visible[i] pixels at value[i]
    hist = torch.empty((65536,), dtype=torch.int32, device="cuda")
    ids16 = torch.from_numpy(ids.astype(np.uint16).view(np.int16)).cuda()
    _C.check(_C.lib().cp_id_histogram(_C.ptr(ids16), H, W, _C.ptr(hist), _C.stream()), "cp_id_histogram")
    hist = hist.cpu().numpy()
    assert len(set(value[live].tolist())) == int(live.sum()) and value[live].min() > 0
    assert hist[value[live]].tolist() == visible[live].tolist()
    assert hist.sum() == H * W and hist[0] == int((index == 255).sum())


@pytest.mark.gpu
def test_kernel_with_no_instance_fills_the_maps():
    import torch
    from centerpoly_amd.detectors import instances
    masks = torch.empty((0, 21, 300), dtype=torch.uint8, device="cuda")
    none = torch.empty((0,), dtype=torch.int32, device="cuda")
    index, ids, labels, value, visible, box = instances.instance_map(masks, none.to(torch.uint8), none, background=7)
    assert (index.cpu().numpy() == 255).all() and (ids.cpu().numpy() == 7).all() and (labels.cpu().numpy() == 7).all()
    assert tuple(index.shape) == tuple(ids.shape) == (21, 300) and value.numel() == visible.numel() == box.numel() == 0


@pytest.mark.gpu
def test_kernel_leaves_null_outputs_alone_and_takes_another_background():
    n, H, W = SHAPES[0]
    a, bit, want = _inputs(n, H, W, "full")
    index, ids, labels, value, visible, box = _device_map(a, bit, 3, background=65535, multiplier=256, want_ids=False)
    w = host.instance_map(a["masks"], a["flags"], bit, a["counts"], MIN_COUNT, a["label"], a["prio"], a["bounds"], 256,
                          65535)
    assert ids is None and np.array_equal(index, w[0]) and np.array_equal(labels, w[2]) and np.array_equal(value, w[3])
    assert np.array_equal(visible, w[4]) and np.array_equal(box, w[5]) and (labels == 65535).any()
    index, ids, labels = _device_map(a, bit, 0, background=65535, multiplier=256, want_labels=False)[:3]
    assert labels is None and np.array_equal(ids, w[1]) and np.array_equal(index, w[0])

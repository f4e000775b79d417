"""The piece reader the four pixel-counting kernels share (csrc/pixel_pieces.h), through each of them: cp_id_histogram,
cp_instance_overlaps, cp_pixel_confusion and cp_panoptic_pairs against plain numpy counts, exact, on the shapes where
the reader changes its path -- one partial piece, exactly one piece, a tile plus one pixel, an odd width -- from an
aligned buffer and from one that starts one element in.  And instance_level.device_ids on host input."""
import ctypes
import functools

import numpy as np
import pytest

from centerpoly_amd.datasets.evaluation import instance_level as il

gpu = pytest.mark.gpu
SHAPES = [(1, 5), (1, 16), (17, 241), (37, 53)]
cases = pytest.mark.parametrize("offset", [0, 1])
shapes = pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d" % s for s in SHAPES])

L = 34                                                    # labels: id < 1000 is its own label, else id // 1000
INST_IDS = [24001, 26001, 33005]                          # G = 3; 33005 is the last pixel's and nobody else's
VOID_ID = 3
PALETTE = np.array([VOID_ID, 7, 8, 24001, 26001], np.uint16)
LAST_ID, LAST_BYTE = 33005, 32                            # the last pixel: a leaking pad or an unflushed run miscounts them
SLACK_ID, SLACK_BYTE = 26001, 26                          # around the image, both in the tables: a counted over-read shows
N_MASKS, N_SLOTS = 2, 3
GROUP = (np.arange(L) // 4).astype(np.int8)               # label -> category
FLAGS = (np.arange(L) >= 7).astype(np.uint8)              # panoptic: labels 0 .. 6 are not evaluated (VOID)
ROWS = 1025                                               # rows of cp_panoptic_pairs' tables


def _runs(rng, values, size, stay=0.7):
    """`size` draws from `values` in runs: a pixel repeats the one before it with probability `stay`."""
    fresh = rng.rand(size) >= stay
    fresh[0] = True
    return np.asarray(values)[rng.randint(0, len(values), size)][np.maximum.accumulate(np.where(fresh, np.arange(size), 0))]


@functools.lru_cache(maxsize=None)
def image(shape):
    """(ids uint16 [HW], bytes uint8 [HW] < L, masks uint8 [2, HW]) of a shape, made once.  Pixels 1000 .. 2099 of an
    image that long are one run under a full mask: a whole wave of one id."""
    size = shape[0] * shape[1]
    rng = np.random.RandomState(size)
    ids = _runs(rng, PALETTE, size)
    byte = _runs(rng, [0, 7, 8, 24, 26], size).astype(np.uint8)
    masks = np.stack([_runs(rng, [0, 0, 1, 255], size), _runs(rng, [0, 200, 0, 0], size, 0.9)]).astype(np.uint8)
    if size > 2100:
        ids[1000:2100], byte[1000:2100], masks[0, 1000:2100] = 26001, 24, 1
    ids[-1], byte[-1], masks[:, -1] = LAST_ID, LAST_BYTE, 5
    for a in (ids, byte, masks):
        a.setflags(write=False)
    return ids, byte, masks


def at(t, elements=0):
    return ctypes.c_void_p(t.data_ptr() + elements * t.element_size())


def upload(host, offset, slack):
    """The flat host array `offset` elements into a 16-byte aligned device buffer that holds `slack` everywhere else
    (the elements before it and 16 after it)."""
    import torch
    buf = torch.full((offset + host.size + 16,), slack, dtype=torch.uint8 if host.dtype == np.uint8 else torch.int16,
                     device="cuda")
    assert buf.data_ptr() % 16 == 0
    flat = host.reshape(-1)
    buf[offset:offset + host.size] = torch.tensor(flat if host.dtype == np.uint8 else flat.view(np.int16)).cuda()
    return buf


def upload_ids(ids, offset):
    return upload(ids, offset, int(np.uint16(SLACK_ID).view(np.int16)))


def device(values, dtype):
    import torch
    return torch.from_numpy(np.ascontiguousarray(values, dtype)).cuda()


def host_ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def fetch(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy().astype(np.int64)


def labels_of(ids):
    return np.where(ids < 1000, ids, ids // 1000).astype(np.int64)


@gpu
@shapes
@cases
def test_id_histogram(shape, offset):
    import torch

    from centerpoly_amd import _C
    ids = image(shape)[0]
    buf = upload_ids(ids, offset)
    hist = torch.full((65536,), -9, dtype=torch.int32, device="cuda")
    _C.check(_C.lib().cp_id_histogram(at(buf, offset), shape[0], shape[1], at(hist), _C.stream()), "cp_id_histogram")
    got, exp = fetch(hist), np.bincount(ids, minlength=65536)
    assert got[LAST_ID] == 1 and got[SLACK_ID] == exp[SLACK_ID]
    assert np.array_equal(got, exp)


@gpu
@shapes
@cases
def test_instance_overlaps(shape, offset):
    """In the offset case the ids start one element in and mask 0 is aligned while mask 1, HW bytes on, is not; only
    where HW is a multiple of 16 both masks start one byte in instead."""
    import torch

    from centerpoly_amd import _C
    ids, _, masks = image(shape)
    H, W = shape
    n, G = N_MASKS, len(INST_IDS)
    mask_offset = offset if (H * W) % 16 == 0 else 0
    ibuf, mbuf = upload_ids(ids, offset), upload(masks, mask_offset, 9)
    inst, void = device(INST_IDS, np.int32), device([VOID_ID], np.int32)
    out = torch.full((n * G + 2 * n,), -9, dtype=torch.int32, device="cuda")
    lib = _C.lib()
    nbytes = lib.cp_instance_overlaps_workspace_bytes(n, G, H, W)
    ws = _C.workspace(nbytes, "cuda")
    _C.check(lib.cp_instance_overlaps(at(mbuf, mask_offset), n, at(ibuf, offset), H, W, at(inst), G, at(void), 1, at(out),
                                      at(out, n * G), at(out, n * G + n), at(ws), nbytes, _C.stream()),
             "cp_instance_overlaps")
    got = fetch(out)
    column = np.full((65536,), G + 1, np.int64)                          # id -> column; G: void, G + 1: neither
    column[INST_IDS] = np.arange(G)
    column[VOID_ID] = G
    exp = np.zeros((n, G + 2), np.int64)
    for m in range(n):
        np.add.at(exp[m], column[ids[masks[m] != 0]], 1)
    assert got[:n * G].reshape(n, G)[:, 2].tolist() == [1, 1]            # the last pixel, once per mask
    assert np.array_equal(got[:n * G].reshape(n, G), exp[:, :G])
    assert np.array_equal(got[n * G:n * G + n], exp[:, G])
    assert np.array_equal(got[n * G + n:], (masks != 0).sum(1))


@gpu
@shapes
@cases
def test_pixel_confusion(shape, offset):
    import torch

    from centerpoly_amd import _C
    ids, pred, _ = image(shape)
    H, W = shape
    G = len(INST_IDS)
    ibuf, pbuf = upload_ids(ids, offset), upload(pred, offset, SLACK_BYTE)
    conf = torch.zeros((L * L,), dtype=torch.int64, device="cuda")        # the call adds to it
    inst = torch.full((3 * G,), -9, dtype=torch.int32, device="cuda")
    bad = torch.zeros((2,), dtype=torch.int32, device="cuda")
    inst_ids = device(INST_IDS, np.int32)
    identity = np.arange(256, dtype=np.uint8)
    lib = _C.lib()
    nbytes = lib.cp_pixel_confusion_workspace_bytes(G)
    ws = _C.workspace(nbytes, "cuda")
    _C.check(lib.cp_pixel_confusion(at(pbuf, offset), host_ptr(identity), at(ibuf, offset), H, W, 1000, 1000, L,
                                    host_ptr(GROUP), at(inst_ids), G, at(conf), at(inst), at(bad), at(ws), nbytes,
                                    _C.stream()), "cp_pixel_confusion")
    g, p = labels_of(ids), pred.astype(np.int64)
    exp = np.zeros((L, L), np.int64)
    np.add.at(exp, (g, p), 1)
    rows = np.array([[(ids == v).sum(), ((ids == v) & (p == v // 1000)).sum(),
                      ((ids == v) & (GROUP[p] == GROUP[v // 1000])).sum()] for v in INST_IDS], np.int64)
    got = fetch(conf).reshape(L, L)
    assert got[33, LAST_BYTE] == 1 and got[33].sum() == 1 and got[:, LAST_BYTE].sum() == 1
    assert np.array_equal(got, exp)
    assert np.array_equal(fetch(inst).reshape(G, 3), rows) and fetch(bad).tolist() == [0, 0]


@gpu
@shapes
@cases
def test_panoptic_pairs(shape, offset):
    """At most five segments and three slots: 24 cells, the dense regime."""
    import torch

    from centerpoly_amd import _C
    ids, byte, _ = image(shape)
    H, W = shape
    n = N_SLOTS
    index = np.where(byte == LAST_BYTE, 1, byte % (n + 1)).astype(np.uint8)      # slots 0 .. 2, 3 for none
    index[index == n] = 255
    ibuf, xbuf = upload_ids(ids, offset), upload(index, offset, 2)
    seg = torch.full((ROWS, 4), -9, dtype=torch.int32, device="cuda")
    pairs = torch.full((ROWS * (n + 1),), -9, dtype=torch.int32, device="cuda")
    lib = _C.lib()
    nbytes = lib.cp_panoptic_pairs_workspace_bytes()
    ws = _C.workspace(nbytes, "cuda")
    _C.check(lib.cp_panoptic_pairs(at(xbuf, offset), n, at(ibuf, offset), H, W, 1000, 1000, L, host_ptr(FLAGS), at(seg),
                                   at(pairs), at(ws), nbytes, _C.stream()), "cp_panoptic_pairs")
    values = np.unique(ids[FLAGS[labels_of(ids)] != 0])                  # the segments, ascending: row 1 on
    R = len(values) + 1
    assert R * (n + 1) <= 24
    row = np.where(FLAGS[labels_of(ids)] != 0, np.searchsorted(values, ids) + 1, 0)
    exp = np.zeros((R, n + 1), np.int64)
    np.add.at(exp, (row, np.minimum(index, n).astype(np.int64)), 1)
    got, got_seg = fetch(pairs).reshape(ROWS, n + 1)[:R], fetch(seg)[:R]
    assert got[R - 1].tolist() == [0, 1, 0, 0]                           # the last pixel's segment: one pixel of slot 1
    assert np.array_equal(got, exp)
    assert got_seg[0, 0] == len(values) and got_seg[0, 1] == exp[0].sum()
    assert np.array_equal(got_seg[1:, 0], values) and np.array_equal(got_seg[1:, 3], exp[1:].sum(1))


def test_device_ids_on_host_input():
    import torch
    ids = np.array([[0, 26001, 32767], [32768, 40000, 65535]], np.uint16)
    dev = il.device_ids(ids, torch.device("cpu"))
    assert dev.dtype == torch.int16 and tuple(dev.shape) == (2, 3)
    assert np.array_equal(dev.numpy().view(np.uint16), ids)              # the bits round-trip past 32767
    assert np.array_equal(il.device_ids(ids[:, ::2], "cpu").numpy().view(np.uint16), ids[:, ::2])   # a strided view
    with pytest.raises(ValueError, match=r"^gt_ids must be uint16 \(see read_gt_ids\), got int32"):
        il.device_ids(ids.astype(np.int32), "cpu")
    with pytest.raises(ValueError, match=r"^frame_7: gt_ids must be uint16 \(see read_gt_ids\), got uint8"):
        il.device_ids(ids.astype(np.uint8), "cpu", "frame_7")
    with pytest.raises(ValueError, match=r"^frame_8: the ground truth is torch.float16: gt_ids must be uint16 \(see read_gt_ids\)"):
        il.device_ids(torch.zeros((2, 3), dtype=torch.float16), "cpu", "frame_8")
    kept = torch.zeros((2, 3), dtype=torch.int16)
    assert il.device_ids(kept, "cuda") is kept                           # a tensor stays where it is

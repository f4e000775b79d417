"""The merge of the test scales and soft-NMS on the device: cp_soft_nms_device and cp_merge_detections
(csrc/merge_nms.hip), external.nms.soft_nms_device and PolydetDetector.merge_outputs_device.

Every comparison is of bits (np.array_equal on .view(np.uint32)): the device code restates the reference's merge, stale
slots included, and has no tolerance.  References: tests/golden/softnms_ref.npz (the reference's own Cython build),
the host cp_soft_nms, and oracle.post.merge_outputs."""
import ctypes
import os

import numpy as np
import pytest
import torch

from centerpoly_amd import _C, synth
from oracle import post as opost

HERE = os.path.dirname(os.path.abspath(__file__))
EINVAL, EUNSUPPORTED = -1, -2
SENTINEL = np.uint32(0x7FC0DEAD)                       # a NaN pattern no arithmetic here produces


def _boxes(tag, n, ncols=38, spread=200.0):
    """The rows of tests/test_detector_io.py::_boxes."""
    c = synth.uniform("nms/c" + tag, (n, 2), 0.0, spread)
    wh = synth.uniform("nms/wh" + tag, (n, 2), 5.0, 80.0)
    b = synth.uniform("nms/rest" + tag, (n, ncols), 0.0, 300.0).astype(np.float32)
    b[:, 0:2] = c - wh / 2
    b[:, 2:4] = c + wh / 2
    b[:, 4] = synth.uniform("nms/s" + tag, (n,), 0.0, 1.0)
    return b.astype(np.float32)


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(np.ascontiguousarray(a).view(np.uint32),
                                                                        np.ascontiguousarray(b).view(np.uint32))


# ------------------------------------------------------------------- CPU ---
# The argument checks come before any device work: they run without a GPU, on pointers that are never followed.

P = ctypes.c_void_p(4096)                              # a non-null pointer


def _nms_rc(rows=P, stride=7, start=P, length=P, n_seg=1, method=2, live=P):
    return _C.lib().cp_soft_nms_device(rows, stride, start, length, n_seg, 0.5, 0.5, 0.001, method, live, None)


def _merge_rc(rows=P, S=2, K=32, ncols=15, C=8, max_per_image=100, method=2, out=ctypes.c_void_p(8192), counts=P,
              ws=P, ws_bytes=None):
    lib = _C.lib()
    if ws_bytes is None:
        ws_bytes = max(lib.cp_merge_detections_workspace_bytes(S, K, ncols, C), 16)
    return lib.cp_merge_detections(rows, S, K, ncols, C, max_per_image, 1, 0.5, 0.5, 0.001, method, out, counts, ws,
                                   ws_bytes, None)


def test_entry_points_are_declared_and_bound():
    with open(os.path.join(HERE, "..", "include", "centerpoly_hip.h")) as f:
        header = f.read()
    lib = _C.lib()
    for name in ("cp_soft_nms_device", "cp_merge_detections", "cp_merge_detections_workspace_bytes"):
        assert name in _C._SIGNATURES and name in _C.EXPORTS
        assert name + "(" in header
        assert getattr(lib, name).argtypes == _C._SIGNATURES[name][1]
    assert lib.cp_abi_version() == 3
    assert "stale" in header and "UNDECAYED" in header                    # the stale-slot rule is part of the contract


def test_soft_nms_device_refuses_bad_arguments_without_a_device():
    for kw in ({"rows": None}, {"start": None}, {"length": None}, {"live": None}, {"n_seg": -1}, {"method": 3},
               {"method": -1}):
        assert _nms_rc(**kw) == EINVAL, kw
    assert _nms_rc(stride=4) == EUNSUPPORTED
    assert _nms_rc(n_seg=65) == EUNSUPPORTED


def test_merge_detections_refuses_bad_arguments_without_a_device():
    lib = _C.lib()
    for kw in ({"rows": None}, {"out": None}, {"counts": None}, {"ws": None}, {"S": -1}, {"K": 0}, {"C": -2},
               {"max_per_image": 0}, {"method": 3}):
        assert _merge_rc(**kw) == EINVAL, kw
    assert _merge_rc(S=1, K=4097) == EUNSUPPORTED                         # S * K = 4097
    assert _merge_rc(S=17, K=241) == EUNSUPPORTED                         # 4097 again, as a product
    assert _merge_rc(C=65) == EUNSUPPORTED
    assert _merge_rc(ncols=6) == EUNSUPPORTED
    need = lib.cp_merge_detections_workspace_bytes(2, 32, 15, 8)
    assert need >= 2 * 32 * 15 * 4
    assert _merge_rc(ws_bytes=need - 1) == EINVAL                         # one byte short
    assert lib.cp_merge_detections_workspace_bytes(4, 1024, 15, 64) > 0   # the limits themselves are supported
    assert lib.cp_merge_detections_workspace_bytes(1, 4097, 15, 8) == 0
    assert lib.cp_merge_detections_workspace_bytes(2, 32, 15, 65) == 0


# ------------------------------------------------------------------- GPU ---

def _i32(v):
    return torch.tensor(v, dtype=torch.int32, device="cuda")


def _golden_tables():
    d = np.load(os.path.join(HERE, "golden", "softnms_ref.npz"))
    for i in range(int(d["n_cases"])):
        sigma, Nt, thr, method = d["c%d_par" % i]
        yield i, d["c%d_in" % i], d["c%d_out" % i], len(d["c%d_keep" % i]), float(sigma), float(Nt), float(thr), int(method)


@pytest.mark.gpu
def test_soft_nms_device_matches_the_reference_build_bitwise():
    """Each of the 18 tables of the reference's own Cython build as one segment: table and live count."""
    from centerpoly_amd.external.nms import soft_nms_device
    n = 0
    for i, a, want, live, sigma, Nt, thr, method in _golden_tables():
        rows = torch.from_numpy(np.ascontiguousarray(a)).cuda()
        got = soft_nms_device(rows, _i32([0]), _i32([a.shape[0]]), sigma=sigma, Nt=Nt, threshold=thr, method=method)
        assert got.is_cuda and got.cpu().tolist() == [live], i
        assert _same_bits(rows.cpu().numpy(), want), i
        n += 1
    assert n == 18


@pytest.mark.gpu
def test_soft_nms_device_segments_with_gaps():
    """Lengths around the wave size in one buffer, gaps between them: every segment equals the host cp_soft_nms on a
    copy (method 2, threshold 0.05: rows are discarded and stale slots arise), the gaps keep their bits."""
    from centerpoly_amd.external.nms import soft_nms, soft_nms_device
    lens, gap, stride = [0, 1, 63, 64, 65, 129], 3, 7
    buf = np.full((sum(lens) + gap * (len(lens) + 1), stride), SENTINEL, np.uint32).view(np.float32)
    starts, at = [], gap
    for n in lens:
        starts.append(at)
        buf[at:at + n] = _boxes("seg%d" % n, n, ncols=stride, spread=60.0)
        at += n + gap
    want, live = buf.copy(), []
    for s, n in zip(starts, lens):
        seg = want[s:s + n].copy()
        live.append(len(soft_nms(seg, sigma=0.5, Nt=0.5, threshold=0.05, method=2)))
        want[s:s + n] = seg
    assert any(k < n for k, n in zip(live, lens))                         # rows were discarded
    rows = torch.from_numpy(buf.copy()).cuda()
    got = soft_nms_device(rows, _i32(starts), _i32(lens), sigma=0.5, Nt=0.5, threshold=0.05, method=2)
    assert got.cpu().tolist() == live
    out = rows.cpu().numpy()
    for s, n in zip(starts, lens):
        assert _same_bits(out[s:s + n], want[s:s + n]), n
    assert _same_bits(out, want)                                          # gaps (and columns 5, 6) included


def _merge_device(rows, C, max_per_image, nms, threshold=0.001):
    """cp_merge_detections on host rows [S, K, ncols]: (table out[:counts[0]], counts)."""
    lib = _C.lib()
    S, K, ncols = rows.shape
    dev = torch.from_numpy(np.ascontiguousarray(rows)).cuda()
    out = torch.from_numpy(np.full((S * K, ncols), SENTINEL, np.uint32).view(np.float32)).cuda()
    counts = torch.full((1 + C,), -7, dtype=torch.int32, device="cuda")
    ws = _C.workspace(lib.cp_merge_detections_workspace_bytes(S, K, ncols, C), dev.device)
    _C.check(lib.cp_merge_detections(_C.ptr(dev), S, K, ncols, C, max_per_image, int(nms), 0.5, 0.5, threshold, 2,
                                     _C.ptr(out), _C.ptr(counts), _C.ptr(ws), ws.numel(), _C.stream()),
             "cp_merge_detections")
    assert _same_bits(dev.cpu().numpy(), np.ascontiguousarray(rows))      # the input is not written
    counts = counts.cpu().numpy()
    return out.cpu().numpy()[:counts[0]], counts


def _split(d, C):
    """The class split of polydet_post_process_device: {1..C: rows without the class column}."""
    keep = np.concatenate([d[:, :5], d[:, 6:]], axis=1)
    return {j + 1: keep[d[:, 5] == j] for j in range(C)}


def _merge_reference(rows, C, max_per_image, nms, threshold=0.001, soft_nms=opost.soft_nms):
    """oracle.post.merge_outputs on the split rows, then device_rows' table (the class column put back).  A
    threshold other than merge_outputs' own 0.001 restates its lines around soft_nms."""
    dets = [_split(d, C) for d in rows]
    if threshold == 0.001 and soft_nms is opost.soft_nms:
        res = opost.merge_outputs(dets, C, max_per_image, nms=bool(nms))
    else:
        res = {}
        for j in range(1, C + 1):
            res[j] = np.concatenate([d[j] for d in dets], axis=0).astype(np.float32)
            if nms:
                soft_nms(res[j], sigma=0.5, Nt=0.5, threshold=threshold, method=2)
        scores = np.hstack([res[j][:, 4] for j in range(1, C + 1)])
        if len(scores) > max_per_image:
            kth = len(scores) - max_per_image
            thresh = np.partition(scores, kth)[kth]
            res = {j: r[r[:, 4] >= thresh] for j, r in res.items()}
    table = np.concatenate([np.concatenate([r[:, :5], np.full((len(r), 1), j - 1, np.float32), r[:, 5:]], axis=1)
                            for j, r in sorted(res.items())], axis=0).astype(np.float32)
    return table, np.array([len(table)] + [len(res[j]) for j in range(1, C + 1)], np.int32)


def _merge_rows(tag, S=2, K=32, C=8, spread=60.0):
    rows = _boxes("mg" + tag, S * K, ncols=15, spread=spread)
    rows[:, 5] = synth.integers("nms/cls" + tag, (S * K,), 0, C).astype(np.float32)
    return rows.reshape(S, K, 15)


def _case_rows(case):
    if case == "b":                                   # quantised scores, few overlaps: ties at the threshold survive
        rows = _merge_rows("ties", spread=400.0)
        rows[:, :, 4] = np.round(rows[:, :, 4] * 8) / 8
        return rows
    if case == "e":                                   # classes 6 and 7 empty, 40 rows of class 3, one row -1, one row 8
        rows = _merge_rows("e")
        cls = np.array([3] * 40 + [-1, 8] + [0, 1, 2, 4, 5] * 4 + [0, 1], np.float32)
        rows[:, :, 5] = cls[np.argsort(synth.uniform("nms/perm-e", (64,)), kind="stable")].reshape(2, 32)
        return rows
    if case == "f":
        return _merge_rows("f", S=1, K=1)
    return _merge_rows(case)


MERGE_CASES = {                                       # max_per_image, nms, threshold
    "a": (100, 1, 0.001),                             # no cut: 64 <= 100
    "b": (20, 1, 0.001),                              # ties at the threshold: longer than 20
    "c": (20, 1, 0.2),                                # rows are discarded: stale slots take part in the cut
    "d": (20, 0, 0.001),                              # partition and cut only
    "e": (50, 1, 0.001),                              # out-of-range classes are dropped
    "f": (100, 1, 0.001),                             # the smallest input
}


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(MERGE_CASES))
def test_merge_detections_matches_the_oracle_bitwise(case):
    max_per_image, nms, threshold = MERGE_CASES[case]
    rows = _case_rows(case)
    want, want_counts = _merge_reference(rows, 8, max_per_image, nms, threshold)
    if case == "b":
        assert want_counts[0] > 20
    if case == "c":                                   # soft-nms discarded rows: the blocks hold stale slots
        blocks = [np.concatenate([_split(d, 8)[j] for d in rows], axis=0) for j in range(1, 9)]
        live = sum(len(opost.soft_nms(b.copy(), sigma=0.5, Nt=0.5, threshold=threshold, method=2)) for b in blocks)
        assert live < 64
    if case == "e":
        assert want_counts[7] == 0 and want_counts[8] == 0 and want_counts[0] <= 62
    got, counts = _merge_device(rows, 8, max_per_image, nms, threshold)
    assert counts.tolist() == want_counts.tolist()
    assert _same_bits(got, want)


@pytest.mark.gpu
def test_merge_detections_at_the_limit_size():
    """S * K = 4096 rows of one class: the largest segment.  The reference is the host cp_soft_nms with
    merge_outputs' numpy cut around it -- oracle.post.soft_nms, a Python double loop, takes minutes on 4096 rows;
    cp_soft_nms equals it bit for bit (tests/test_detector_io.py)."""
    from centerpoly_amd.external.nms import soft_nms
    rows = _boxes("limit", 4096, ncols=15, spread=300.0)                 # soft-nms discards almost half of them
    rows[:, 5] = 0
    rows = rows.reshape(4, 1024, 15)
    want, want_counts = _merge_reference(rows, 1, 1000, 1, 0.001, soft_nms=soft_nms)
    got, counts = _merge_device(rows, 1, 1000, 1, 0.001)
    assert counts.tolist() == want_counts.tolist() and counts[0] >= 1000
    assert _same_bits(got, want)


@pytest.mark.gpu
@pytest.mark.parametrize("args", [["--test_scales", "1,0.5", "--flip_test"], ["--nms"]], ids=["two-scales-flip", "nms"])
def test_detector_device_merge_equals_host_merge(args):
    """run() with device_merge on returns the `results` of the same detector with it off, bit for bit, and
    device_rows / host_rows are the table the old path builds from them."""
    from centerpoly_amd.detectors.detector_factory import detector_factory
    from centerpoly_amd.opts import opts
    opt = opts().init(["polydet", "--arch", "smallhourglass", "--K", "32"] + args)
    torch.manual_seed(317)
    det = detector_factory["polydet"](opt)
    img = (synth.uniform("ms/img", (192, 256, 3)) * 255).astype(np.uint8)
    det.device_merge = False
    off = det.run(img)["results"]
    rows_off, host_off = det.device_rows(off), det.host_rows(off)
    det.device_merge = True
    on = det.run(img)["results"]
    rows_on, host_on = det.device_rows(on), det.host_rows(on)
    assert sorted(on) == sorted(off) == list(range(1, 9))
    for j in range(1, 9):
        assert _same_bits(on[j], off[j]), j
    total = sum(len(r) for r in on.values())
    assert total > 0
    assert rows_on.is_cuda and rows_on.dtype == torch.float32 and tuple(rows_on.shape) == (total, rows_off.shape[1])
    assert _same_bits(rows_on.cpu().numpy(), rows_off.cpu().numpy())
    assert _same_bits(host_on, host_off)

"""--mask_nms: the whole-row merge by the polygons' mask IoU (csrc/mask_nms.hip: cp_polygon_overlaps and
cp_merge_detections_mask; external.nms.polygon_overlaps_device / mask_nms_device; PolydetDetector).

Every comparison is of bits.  References: tests/golden/mask_nms.npz -- PIL's own ImageDraw.polygon, drawn by
tests/golden/gen_mask_nms_golden.py -- and the literal host statement tests/golden/mask_nms_host.py.  The fixture's
Gaussian cases keep the best two live scores of every selection step more than 1e-4 apart (relative), so the last bit of
the device's double exp cannot change an order; a score that differs in a bit fails its test."""
import contextlib
import ctypes
import functools
import io
import os
import sys

import numpy as np
import pytest
import torch

from centerpoly_amd import _C

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import mask_nms_host as host  # noqa: E402

EINVAL, EUNSUPPORTED, EWORKSPACE = -1, -2, -3
SENTINEL = np.uint32(0x7FC0DEAD)                       # a NaN pattern no arithmetic here produces

OV_CASES = ["shapes_n8", "shapes_n16", "shapes_n64", "triangles_n3", "random_n64", "random_n3_37x53", "canvas_1x1",
            "width_31", "width_32", "width_33", "width_64", "width_65", "rows_1", "rows_63", "rows_64", "rows_65",
            "rows_129", "canvas_128x256", "canvas_1024x2048", "rows_1024"]
MG_CASES = ["m%d_s%d" % (m, s) for m in (0, 1, 2) for s in (1, 2, 3)] + ["ties", "cut_ties", "cut_one", "threshold",
                                                                         "limit"]


@functools.lru_cache(maxsize=None)
def _fixture():
    d = np.load(os.path.join(HERE, "golden", "mask_nms.npz"))
    return {k: d[k] for k in d.files}


@functools.lru_cache(maxsize=None)
def _case(key):
    """A case of the fixture: rows, canvas (H, W), C, area, inter (from the packed masks where the matrix is not
    recorded), and for a merge case par, table, counts.  Computed once, never modified."""
    f = _fixture()
    c = {k[len(key) + 1:]: v for k, v in f.items() if k.startswith(key + "/")}
    c["H"], c["W"], c["C"] = int(c["canvas"][0]), int(c["canvas"][1]), int(c["C"])
    if "inter" not in c:
        flat = c["rows"].reshape(-1, c["rows"].shape[-1])
        m = np.unpackbits(c["masks"], axis=1)[:, :c["H"] * c["W"]].astype(bool)
        area, c["inter"] = host.overlaps_from_masks(m, [host.class_of(r[5], c["C"]) for r in flat])
        assert np.array_equal(area, c["area"])
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(np.ascontiguousarray(a).view(np.uint32),
                                                                        np.ascontiguousarray(b).view(np.uint32))


def _parse(args):
    from centerpoly_amd.opts import opts
    with contextlib.redirect_stdout(io.StringIO()):
        return opts().init(args)


# ------------------------------------------------------------------- CPU ---

def test_fixture_lists_the_cases():
    f = _fixture()
    assert f["ov/names"].tolist() == OV_CASES and f["mg/names"].tolist() == MG_CASES


def test_options_parse():
    opt = _parse(["polydet"])
    assert opt.mask_nms is False and opt.mask_nms_method == "gaussian"
    opt = _parse(["polydet", "--mask_nms", "--mask_nms_method", "linear", "--nms", "--test_scales", "1,0.5"])
    assert opt.mask_nms is True and opt.mask_nms_method == "linear" and opt.nms is True
    assert _parse(["polydet", "--mask_nms", "--mask_nms_method", "hard"]).mask_nms_method == "hard"
    with pytest.raises(SystemExit), contextlib.redirect_stderr(io.StringIO()):
        _parse(["polydet", "--mask_nms_method", "median"])
    from centerpoly_amd.external import nms
    assert nms.MASK_NMS_METHODS == {"hard": 0, "linear": 1, "gaussian": 2}
    assert callable(nms.polygon_overlaps_device) and callable(nms.mask_nms_device)


def test_entry_points_are_declared_and_bound():
    with open(os.path.join(HERE, "..", "include", "centerpoly_hip.h")) as f:
        header = f.read()
    lib = _C.lib()
    for name in ("cp_polygon_overlaps", "cp_polygon_overlaps_workspace_bytes", "cp_merge_detections_mask",
                 "cp_merge_detections_mask_workspace_bytes"):
        assert name in _C._SIGNATURES and name in _C.EXPORTS
        assert name + "(" in header
        assert getattr(lib, name).argtypes == _C._SIGNATURES[name][1]
    assert lib.cp_abi_version() == 3
    assert "cp_polygon_overlaps(_workspace_bytes)" in header and "cp_merge_detections_mask(_workspace_bytes)" in header
    assert "no stale slots" in header and "ONE source row" in header      # the point of the feature is in the contract


# The argument checks come before any device work: they run without a GPU, on pointers that are never followed.
P = ctypes.c_void_p(4096)                              # a non-null, 16-byte aligned pointer
Q = ctypes.c_void_p(8192)


def _ov_rc(rows=P, R=8, ncols=39, C=3, H=48, W=64, area=P, inter=P, ws=P, ws_bytes=None):
    lib = _C.lib()
    if ws_bytes is None:
        ws_bytes = max(lib.cp_polygon_overlaps_workspace_bytes(R, ncols, H, W), 16)
    return lib.cp_polygon_overlaps(rows, R, ncols, C, H, W, area, inter, ws, ws_bytes, None)


def _mg_rc(rows=P, S=2, K=32, ncols=39, C=8, max_per_image=100, method=2, H=48, W=64, out=Q, counts=P, ws=P,
           ws_bytes=None):
    lib = _C.lib()
    if ws_bytes is None:
        ws_bytes = max(lib.cp_merge_detections_mask_workspace_bytes(S, K, ncols, C, H, W), 16)
    return lib.cp_merge_detections_mask(rows, S, K, ncols, C, max_per_image, 1, 0.5, 0.5, 0.001, method, H, W, out,
                                        counts, ws, ws_bytes, None)


def test_polygon_overlaps_refuses_bad_arguments_without_a_device():
    lib = _C.lib()
    for kw in ({"rows": None}, {"area": None}, {"inter": None}, {"ws": None}, {"R": 0}, {"R": -3}, {"ncols": 0},
               {"C": 0}, {"H": 0}, {"W": -1}, {"ncols": 11}, {"ncols": 38}, {"ws": ctypes.c_void_p(4100)}):
        assert _ov_rc(**kw) == EINVAL, kw
    assert _ov_rc(R=1025) == EUNSUPPORTED
    assert _ov_rc(C=65) == EUNSUPPORTED
    assert _ov_rc(ncols=2 * 65 + 7) == EUNSUPPORTED                       # N = 65
    assert _ov_rc(H=1 << 16, W=1 << 15) == EUNSUPPORTED                   # H * W = 2^31
    need = lib.cp_polygon_overlaps_workspace_bytes(8, 39, 48, 64)
    assert need >= 8 * 48 * 2 * 4                                         # the bit planes: two words a row
    assert _ov_rc(ws_bytes=need - 1) == EWORKSPACE
    assert lib.cp_polygon_overlaps_workspace_bytes(1024, 2 * 64 + 7, 48, 64) > 0      # the limits themselves
    assert lib.cp_polygon_overlaps_workspace_bytes(1, 13, 1, 1) > 0
    assert lib.cp_polygon_overlaps_workspace_bytes(1025, 39, 48, 64) == 0
    assert lib.cp_polygon_overlaps_workspace_bytes(8, 38, 48, 64) == 0


def test_merge_detections_mask_refuses_bad_arguments_without_a_device():
    lib = _C.lib()
    for kw in ({"rows": None}, {"out": None}, {"counts": None}, {"ws": None}, {"S": -1}, {"K": 0}, {"C": -2}, {"C": 0},
               {"max_per_image": 0}, {"method": 3}, {"method": -1}, {"H": 0}, {"W": 0}, {"ncols": 7}, {"ncols": 40},
               {"out": P}, {"ws": ctypes.c_void_p(4104)}):
        assert _mg_rc(**kw) == EINVAL, kw
    assert _mg_rc(S=1, K=1025) == EUNSUPPORTED                            # S * K = 1025
    assert _mg_rc(S=5, K=205) == EUNSUPPORTED                             # 1025 again, as a product
    assert _mg_rc(S=1 << 16, K=1 << 16) == EUNSUPPORTED                   # a product beyond int32
    assert _mg_rc(C=65) == EUNSUPPORTED
    assert _mg_rc(ncols=2 * 65 + 7) == EUNSUPPORTED
    assert _mg_rc(H=1 << 15, W=1 << 16) == EUNSUPPORTED
    need = lib.cp_merge_detections_mask_workspace_bytes(2, 32, 39, 8, 48, 64)
    assert need >= 64 * 48 * 2 * 4 + 64 * 64 * 4                          # the planes and the matrix
    assert _mg_rc(ws_bytes=need - 1) == EWORKSPACE
    assert lib.cp_merge_detections_mask_workspace_bytes(4, 256, 135, 64, 48, 64) > 0  # the limits themselves
    assert lib.cp_merge_detections_mask_workspace_bytes(2, 128, 39, 8, 1024, 2048) <= 65 << 20    # "64 MiB" and tables
    assert lib.cp_merge_detections_mask_workspace_bytes(1, 1025, 39, 8, 48, 64) == 0
    assert lib.cp_merge_detections_mask_workspace_bytes(2, 32, 39, 65, 48, 64) == 0


def test_host_statement_with_pil_reproduces_the_fixture():
    """Every case drawn again with the installed PIL: areas, matrix (or masks), and the merge cases' tables."""
    for name in OV_CASES + ["mg:" + n for n in MG_CASES]:
        key = "mg/" + name[3:] if name.startswith("mg:") else "ov/" + name
        c = _case(key)
        area, inter = host.overlaps(c["rows"], c["C"], c["H"], c["W"])
        assert np.array_equal(area, c["area"]) and np.array_equal(inter, c["inter"]), name
        assert np.array_equal(inter, inter.T) and np.array_equal(np.diagonal(inter), area)
        if key.startswith("mg/"):
            mpi, sigma, Nt, thr, method = c["par"]
            table, counts = host.mask_nms(c["rows"], c["C"], area, inter, int(mpi), sigma, Nt, thr, int(method))
            assert _same_bits(table, c["table"]) and counts.tolist() == c["counts"].tolist(), name


def test_fixture_covers_what_it_names():
    c = _case("ov/shapes_n16")
    cls = c["rows"][:, 5]
    assert 2.5 in cls and -1 in cls and 3 in cls                          # rows without a class
    assert all(c["area"][i] == 0 and not c["inter"][i].any() for i in np.nonzero((cls == 2.5) | (cls == -1) | (cls == 3))[0])
    assert c["inter"][2, 3] == c["area"][2] == c["area"][3] > 0           # identical polygons: ov = 1
    assert c["inter"][4, 5] == c["area"][5] < c["area"][4]                # nested
    assert c["inter"][6, 7] == 1 and c["inter"][6, 8] == 0                # PIL's boxes share the corner pixel only
    assert (c["area"] == 0).sum() >= 7 and c["area"].max() == 48 * 64     # wholly off; covering the canvas
    assert _case("ov/canvas_1x1")["area"].max() == 1
    t = _case("mg/ties")
    assert len(np.unique(t["rows"][:, :, 4])) <= 9                        # equal scores
    assert _case("mg/cut_ties")["counts"][0] > _case("mg/cut_ties")["par"][0]
    assert _case("mg/cut_one")["counts"][0] == 1
    assert _case("mg/m0_s2")["counts"].tolist()[3:] == [1, 0]             # a class of one row, an empty class
    th = _case("mg/threshold")
    assert th["counts"][0] * 3 < th["rows"].shape[0] * th["rows"].shape[1]
    assert _case("mg/limit")["rows"].shape[:2] == (4, 256) and _case("mg/limit")["C"] == 1


def test_the_two_triangles_do_not_overlap_and_survive_undecayed():
    """The pair of the issue: box IoU 0.908, masks of 861 pixels each with none in common."""
    c = _case("ov/shapes_n16")
    rows = c["rows"][:2].copy()
    assert host.polygon(rows[0])[:3] == [(0, 0), (40, 0), (0, 40)] and host.polygon(rows[1])[:3] == [(41, 1), (41, 41), (1, 41)]
    area, inter = host.overlaps(rows, 1, 48, 64)
    assert area.tolist() == [861, 861] and inter[0, 1] == 0
    assert c["area"][:2].tolist() == [861, 861] and c["inter"][0, 1] == 0
    b = rows[:, :4].astype(np.float64)
    iw, ih = min(b[0, 2], b[1, 2]) - max(b[0, 0], b[1, 0]) + 1, min(b[0, 3], b[1, 3]) - max(b[0, 1], b[1, 1]) + 1
    box_iou = iw * ih / (2 * 41 * 41 - iw * ih)
    assert abs(box_iou - 0.908) < 1e-3
    for method in (0, 1, 2):
        table, counts = host.mask_nms(rows[None], 1, area, inter, 100, method=method)
        assert counts.tolist() == [2, 2] and _same_bits(table, rows), method


def test_constructor_refuses_more_rows_than_the_device_merge_holds():
    """5 scales x K = 256 = 1280 rows: a ValueError with the numbers, before anything touches a device."""
    from centerpoly_amd.detectors.detector_factory import detector_factory
    opt = _parse(["polydet", "--arch", "dla_34", "--mask_nms", "--test_scales", "1,0.5,0.75,1.25,1.5", "--K", "256"])
    with pytest.raises(ValueError) as e:
        detector_factory["polydet"](opt)
    assert "1280" in str(e.value) and "256" in str(e.value) and "1024" in str(e.value)


# ------------------------------------------------------------------- GPU ---

def _overlaps_device(rows, C, H, W):
    from centerpoly_amd.external.nms import polygon_overlaps_device
    dev = torch.from_numpy(np.array(rows, np.float32)).cuda()
    area, inter = polygon_overlaps_device(dev, (W, H), num_classes=C)
    assert _same_bits(dev.cpu().numpy(), np.ascontiguousarray(rows))      # the input is not written
    return area.cpu().numpy(), inter.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("name", OV_CASES)
def test_polygon_overlaps_match_pil(name):
    c = _case("ov/" + name)
    area, inter = _overlaps_device(c["rows"], c["C"], c["H"], c["W"])
    assert area.dtype == np.int32 and inter.dtype == np.int32
    bad = np.nonzero(area != c["area"])[0]
    assert bad.size == 0, (name, bad[:8], area[bad[:8]], c["area"][bad[:8]])
    bad = np.argwhere(inter != c["inter"])
    assert bad.size == 0, (name, bad[:8])
    again = _overlaps_device(c["rows"], c["C"], c["H"], c["W"])           # integers: a call repeats its bits
    assert np.array_equal(again[0], area) and np.array_equal(again[1], inter)


def _merge_device(rows, C, H, W, par, nms=1):
    """cp_merge_detections_mask on host rows [S, K, ncols]: (table out[:counts[0]], counts)."""
    lib = _C.lib()
    S, K, ncols = rows.shape
    mpi, sigma, Nt, thr, method = par
    dev = torch.from_numpy(np.array(rows, np.float32)).cuda()
    out = torch.from_numpy(np.full((S * K, ncols), SENTINEL, np.uint32).view(np.float32)).cuda()
    counts = torch.full((1 + C,), -7, dtype=torch.int32, device="cuda")
    ws = _C.workspace(lib.cp_merge_detections_mask_workspace_bytes(S, K, ncols, C, H, W), dev.device)
    _C.check(lib.cp_merge_detections_mask(_C.ptr(dev), S, K, ncols, C, int(mpi), int(nms), float(sigma), float(Nt), float(thr),
                                          int(method), H, W, _C.ptr(out), _C.ptr(counts), _C.ptr(ws), ws.numel(),
                                          _C.stream()), "cp_merge_detections_mask")
    assert _same_bits(dev.cpu().numpy(), np.ascontiguousarray(rows))      # the input is not written
    counts = counts.cpu().numpy()
    out = out.cpu().numpy()
    assert (out[counts[0]:].view(np.uint32) == SENTINEL).all()            # nothing is written beyond the kept rows
    return out[:counts[0]], counts


def _report(got, want):
    """The first rows whose bits differ, for the assertion message."""
    n = min(len(got), len(want))
    bad = [i for i in range(n) if not _same_bits(got[i], want[i])][:4]
    return [(i, got[i, 4], want[i, 4], got[i, 5]) for i in bad]


@pytest.mark.gpu
@pytest.mark.parametrize("name", MG_CASES)
def test_merge_detections_mask_matches_the_host_statement_bitwise(name):
    c = _case("mg/" + name)
    mpi, sigma, Nt, thr, method = c["par"]
    if name == "limit":                               # the host statement's table is the fixture's (the CPU test above)
        want, want_counts = c["table"], c["counts"]
    else:
        want, want_counts = host.mask_nms(c["rows"], c["C"], c["area"], c["inter"], int(mpi), sigma, Nt, thr, int(method))
        assert _same_bits(want, c["table"])
    got, counts = _merge_device(c["rows"], c["C"], c["H"], c["W"], c["par"])
    assert counts.tolist() == want_counts.tolist(), name
    assert _same_bits(got, want), (name, _report(got, want))
    again, counts2 = _merge_device(c["rows"], c["C"], c["H"], c["W"], c["par"])
    assert _same_bits(again, got) and counts2.tolist() == counts.tolist()
    from centerpoly_amd.external.nms import mask_nms_device
    out, n = mask_nms_device(torch.from_numpy(np.array(c["rows"])).cuda(), c["C"], (c["W"], c["H"]), int(mpi),
                             sigma=sigma, Nt=Nt, threshold=thr, method={0: "hard", 1: "linear", 2: "gaussian"}[int(method)])
    assert n.cpu().tolist() == counts.tolist() and _same_bits(out.cpu().numpy()[:counts[0]], got)


def _rows_are_whole(table, rows):
    """Every row of `table` equals one row of `rows` in all columns but 4, and no row of `rows` appears twice."""
    src = np.delete(rows.reshape(-1, rows.shape[-1]), 4, axis=1).view(np.uint32)
    index = {r.tobytes(): i for i, r in enumerate(src)}
    assert len(index) == len(src)                                         # the fixture's rows are distinct (the depth)
    used = [index.get(r.tobytes()) for r in np.delete(table, 4, axis=1).view(np.uint32)]
    return all(u is not None for u in used) and len(set(used)) == len(used)


@pytest.mark.gpu
def test_every_output_row_is_one_input_row():
    """What the feature is for.  The literal merge on the same rows breaks it (asserted as a statement about the
    fixture: its rows overlap enough for soft_nms to swap columns 0-4)."""
    c = _case("mg/m2_s3")
    got, counts = _merge_device(c["rows"], c["C"], c["H"], c["W"], c["par"])
    assert counts[0] > 40 and _rows_are_whole(got, c["rows"])
    lib = _C.lib()
    S, K, ncols = c["rows"].shape
    dev = torch.from_numpy(np.array(c["rows"])).cuda()
    out = torch.zeros((S * K, ncols), dtype=torch.float32, device="cuda")
    n = torch.zeros(1 + c["C"], dtype=torch.int32, device="cuda")
    ws = _C.workspace(lib.cp_merge_detections_workspace_bytes(S, K, ncols, c["C"]), dev.device)
    _C.check(lib.cp_merge_detections(_C.ptr(dev), S, K, ncols, c["C"], 100, 1, 0.5, 0.5, 0.001, 2, _C.ptr(out),
                                     _C.ptr(n), _C.ptr(ws), ws.numel(), _C.stream()), "cp_merge_detections")
    literal = out.cpu().numpy()[:int(n[0])]
    assert len(literal) > 0 and not _rows_are_whole(literal, c["rows"])


def _image(tag, h, w):
    from centerpoly_amd import synth
    return (synth.uniform("masknms/" + tag, (h, w, 3)) * 256).astype(np.uint8)


def _detector(extra):
    """A DLA-34 with seeded weights at a 64 x 96 input, K = 32."""
    import cases
    from centerpoly_amd.detectors.detector_factory import detector_factory
    opt = _parse(["polydet", "--arch", "dla_34", "--dataset", "kitti_poly", "--input_h", "64", "--input_w", "96",
                  "--K", "32", "--mask_nms"] + list(extra))
    with contextlib.redirect_stdout(io.StringIO()):
        det = detector_factory["polydet"](opt)
    model = det.model
    model.train()                                                 # drops the prepared forms of the random weights
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    model.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)).cuda()
                           for k, v in cases.fill_weights(shapes).items()})
    model.eval()
    model.prepare_inference()
    return det, opt


def _check_against_host(det, opt, results, scale_rows, size, image=0):
    """results, device_rows and host_rows of one image against the host statement (PIL's masks) on the detector's own
    scale rows."""
    W, H = size
    C = opt.num_classes
    rows = scale_rows.cpu().numpy()
    area, inter = host.overlaps(rows, C, H, W)
    method = {"hard": 0, "linear": 1, "gaussian": 2}[opt.mask_nms_method]
    want, counts = host.mask_nms(rows, C, area, inter, opt.K, 0.5, 0.5, 0.001, method)
    assert counts[0] > 0 and _rows_are_whole(want, rows)
    dev, hst = det.device_rows(image=image), det.host_rows(image=image)
    assert dev.is_cuda and _same_bits(dev.cpu().numpy(), want), _report(dev.cpu().numpy(), want)
    assert _same_bits(np.ascontiguousarray(hst), want)
    assert sorted(results) == list(range(1, C + 1))
    first = 0
    for j in range(1, C + 1):
        r = want[first:first + counts[j]]
        assert _same_bits(results[j], np.concatenate([r[:, :5], r[:, 6:]], axis=1)), j
        first += counts[j]
    return want


@pytest.mark.gpu
@pytest.mark.parametrize("extra", [["--test_scales", "1,0.5", "--flip_test"], [], ["--mask_nms_method", "hard", "--nms"]],
                         ids=["two-scales-flip", "one-scale", "hard-with-nms"])
def test_detector_mask_nms_equals_the_host_statement(extra):
    det, opt = _detector(extra)
    img = _image("run", 100, 180)
    ret = det.run(img)
    S = len(opt.test_scales)
    assert tuple(det.scale_rows.shape) == (S, 32, 2 * 16 + 7)
    want = _check_against_host(det, opt, ret["results"], det.scale_rows, (180, 100))
    # everything downstream reads device_rows
    maps = det.instances(ret["results"])
    assert maps.canvas == (180, 100) and tuple(maps.index.shape) == (100, 180)
    from centerpoly_amd.detectors.base_detector import class_names
    from centerpoly_amd.utils.debugger import Debugger
    dbg = Debugger(class_names(opt), down_ratio=opt.down_ratio, device=opt.device)
    assert det.show_results(dbg, img, ret["results"]) == "polydet"
    assert tuple(dbg.imgs["polydet"].shape[:2]) == (100, 180)
    torch.cuda.synchronize()
    assert len(want) <= S * 32


class _Recorder(torch.nn.Module):
    """The detector's model with a copy of every launch's heads kept (process applies the sigmoid in place)."""

    def __init__(self, model):
        super(_Recorder, self).__init__()
        self.model, self.seen = model, []

    def forward(self, x):
        out = self.model(x)
        self.seen.append({k: v.clone() for k, v in out[-1].items()})
        return out


@pytest.mark.gpu
def test_run_batch_with_mask_nms_equals_run_image_for_image():
    """Two images of different sizes in one batch.  The network picks some K splits by its launch size, so the heads of
    a batch of two agree with a single-image launch to rounding only (BaseDetector.run_batch; measured here: vertices
    differ in the seventh digit), with or without --mask_nms.  So, as tests/test_batch_detect.py does it: every image
    of the batch against the host statement on the batch's own scale rows, and against run()'s own tail (post_process,
    merge) fed with the batch's own heads, bit for bit; and run_batch of ONE image against run() itself, bit for bit,
    for both sizes."""
    from centerpoly_amd.models.decode import polydet_decode
    det, opt = _detector(["--test_scales", "1,0.5"])
    imgs = [_image("b0", 100, 180), _image("b1", 64, 96)]
    C = opt.num_classes
    rec = det.model = _Recorder(det.model)
    ret = det.run_batch(imgs)
    det.model = rec.model
    assert ret["n"] == 2 and tuple(det.scale_rows.shape) == (2, 2, 32, 39) and len(rec.seen) == 2
    kept = []
    for b, im in enumerate(imgs):
        _check_against_host(det, opt, ret["results"][b], det.scale_rows[b], (im.shape[1], im.shape[0]), image=b)
        assert det.instances(image=b).canvas == (im.shape[1], im.shape[0])
        kept.append((det.device_rows(image=b).cpu().numpy(), det.host_rows(image=b).copy()))
    assert not _same_bits(kept[0][0], kept[1][0])                         # the images differ, and so do their rows
    for b, im in enumerate(imgs):                                         # run()'s tail on the batch's own heads
        det._slot, det._merged, det._batch = 0, False, None               # as run() begins
        det.image_sizes = [(int(im.shape[1]), int(im.shape[0]))]
        detections = []
        for scale, heads in zip(opt.test_scales, rec.seen):
            meta = det.pre_process(im, scale)[1]
            with torch.no_grad():
                dets = polydet_decode(heads["hm"][b:b + 1].sigmoid(), heads["poly"][b:b + 1],
                                      heads["pseudo_depth"][b:b + 1], reg=heads["reg"][b:b + 1],
                                      cat_spec_poly=opt.cat_spec_poly, K=opt.K, rep=opt.rep)
            detections.append(det.post_process(dets, meta, scale))
        want = det.merge(detections)
        for j in range(1, C + 1):
            assert _same_bits(ret["results"][b][j], want[j]), (b, j)
        assert _same_bits(det.device_rows().cpu().numpy(), kept[b][0]), b
        assert _same_bits(np.ascontiguousarray(det.host_rows()), kept[b][1]), b
    for im in imgs:                                                       # a batch of one is run() itself
        single = det.run(im)
        rows, hst = det.device_rows().cpu().numpy(), det.host_rows().copy()
        one = det.run_batch([im])
        for j in range(1, C + 1):
            assert _same_bits(one["results"][0][j], single["results"][j]), j
        assert _same_bits(det.device_rows(image=0).cpu().numpy(), rows) and _same_bits(det.host_rows(image=0), hst)

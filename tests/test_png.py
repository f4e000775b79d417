"""Device PNG streams (cp_png_deflate, utils/png.py) against the host statement (tests/golden/png_host.py): the device's
bytes are the statement's bytes, twice; and the writers behind --device_png leave files with the pixels, text and scores
of the files PIL writes.  The references are computed once per image and shared."""
import contextlib
import io
import os

import numpy as np
import pytest

import png_host as host
import test_instances_api as tia
from test_png_cpu import cases, check_file, id_image, polygon_mask

pytestmark = pytest.mark.gpu

_REF = {}
LOOPS_BELOW = 20000                                      # stream bytes up to which the literal loops make the reference


def _ref(a, bits):
    """The statement's zlib stream of one image, once per image: the literal loops for small images, the numpy run
    search (held against the loops in test_png_cpu.py) for larger ones."""
    key = (a.shape, bits, a.tobytes())
    if key not in _REF:
        small = a.shape[0] * (1 + a.shape[1] * bits // 8) <= LOOPS_BELOW
        _REF[key] = host.zlib_stream(a.tolist(), bits) if small else host.zlib_stream(a, bits, fast=True)
    return _REF[key]


def _check(images, bits, as_planes=False, bounds=None, capacity=None):
    """Images [n, H, W] through zlib_stream (the statement's bytes, and the same bytes again) and encode (files PIL
    opens).  as_planes: as uint8 planes, else as int32 images.  Returns the streams."""
    import torch
    from centerpoly_amd.utils import png
    images = np.ascontiguousarray(images)
    dev = torch.from_numpy(images.astype(np.uint8 if as_planes else np.int32)).cuda()
    kw = {"planes": dev} if as_planes else {"images": dev}
    got = png.zlib_stream(bits=bits, bounds=bounds, capacity=capacity, **kw)
    assert len(got) == len(images)
    for k, a in enumerate(images):
        assert got[k] == _ref(a, bits), "image %d of %s" % (k, images.shape)
    assert png.zlib_stream(bits=bits, bounds=bounds, capacity=capacity, **kw) == got
    files = png.encode(bits=bits, bounds=bounds, **kw)
    for k in sorted({0, len(images) // 2, len(images) - 1}):
        assert files[k] == host.png_file(got[k], images.shape[2], images.shape[1], bits)
        check_file(files[k], images[k], bits)
    return got


@pytest.mark.parametrize("name", sorted(cases()))
def test_the_cases_of_the_statement(name):
    a, bits = cases()[name]
    _check(a[None], bits)
    if a.dtype == np.uint8:
        _check(a[None], bits, as_planes=True)


@pytest.mark.parametrize("W", [15, 16, 17, 33, 257])
def test_piece_tails_and_runs_across_row_ends(W):
    """H = 3: rows of zeros whose run passes the filter byte into the next row, a row that ends in a set pixel, noise."""
    rng = np.random.default_rng(W)
    a = np.zeros((4, 3, W), np.int32)
    a[0, 1, W // 2] = 255                                                  # two long runs of zeros across the row ends
    a[1, 0, W - 1] = a[1, 1, 0] = 255                                      # literals on both sides of a filter byte
    a[2] = (rng.random((3, W)) < 0.2) * 255
    a[3] = rng.integers(0, 256, (3, W))
    _check(a, 8)
    _check(a, 8, as_planes=True)
    _check(a * 257, 16)                                                    # both bytes of a pixel alike: runs at distance 2
    _check(np.where(a > 0, 26000 + a, 0), 16)


@pytest.mark.parametrize("n", [1, 128])
def test_planes_of_different_contents(n):
    """9 x 70 (639 stream bytes, one tile each): densities from empty to noise.  Among 128 streams some end on a byte
    boundary and some do not, and neighbours share words of the output (the lengths are not multiples of 4)."""
    rng = np.random.default_rng(100 + n)
    a = np.stack([(rng.random((9, 70)) < (k % 16) / 30.0).astype(np.uint8) * (255 if k % 3 else 1 + k) for k in range(n)])
    got = _check(a, 8, as_planes=True)
    if n > 1:
        bits = [host.deflate(host.tokens(host.filtered(p.tolist(), 8), 1), 1, want_bits=True) % 8 for p in a]
        assert 0 in bits and any(bits) and len({len(s) % 4 for s in got}) == 4
        _check(a, 8)


def test_bounds_given_empty_and_null():
    import torch
    H, W = 70, 150
    rng = np.random.default_rng(9)
    boxes = [(10, 5, 40, 30), (100, 40, W - 1, H - 1), (60, 50, 70, H - 1), (63, 0, 64, H - 1), (0, 0, 0, 0),
             (W - 1, H - 1, W - 1, H - 1), (W, H, -1, -1), (5, 5, 4, 9), (0, 0, W - 1, H - 1)]
    m = np.zeros((len(boxes), H, W), np.uint8)
    for k, (x0, y0, x1, y1) in enumerate(boxes):
        if x1 >= x0 and y1 >= y0:
            m[k, y0:y1 + 1, x0:x1 + 1] = (rng.random((y1 - y0 + 1, x1 - x0 + 1)) < 0.6) * 255
    b = np.array(boxes, np.int32)
    with_bounds = _check(m, 8, as_planes=True, bounds=b)
    assert _check(m, 8, as_planes=True) == with_bounds
    assert _check(m, 8, as_planes=True, bounds=torch.from_numpy(b).cuda()) == with_bounds
    loose = b.copy()
    loose[:, :2] -= 7                                                      # larger than the masks, beyond the canvas
    loose[:, 2:] += 7
    loose[6:8] = b[6:8]
    assert _check(m, 8, as_planes=True, bounds=loose) == with_bounds
    empty = np.zeros((2, H, W), np.uint8)
    assert _check(empty, 8, as_planes=True, bounds=np.array([[W, H, -1, -1]] * 2, np.int32)) == _check(empty, 8, as_planes=True)
    _check(m.astype(np.int32) * 100, 16, bounds=b)                         # an id image within bounds


def test_sixteen_bit_values():
    a = np.zeros((1, 5, 9), np.int32)
    a[0, 0, :5] = [0, 255, 256, 0xFF00, 65535]
    a[0, 2] = 65535
    a[0, 3, ::2] = 0x0101
    a[0, 4] = [0x1200, 0x0012, 0x1200, 0x0012, 0x1212, 0x1212, 0x12FF, 0xFF12, 0]
    _check(a, 16)


@pytest.mark.parametrize("bits,value", [(8, -3), (8, 256), (16, 65536), (16, -1), (16, 1 << 30)])
def test_a_value_that_does_not_fit_is_named(bits, value, tmp_path):
    import torch
    from centerpoly_amd.datasets import ground_truth
    from centerpoly_amd.utils import png
    a = np.full((2, 6, 7), 5, np.int32)
    a[1, 3, 4] = value
    dev = torch.from_numpy(a).cuda()
    with pytest.raises(ValueError, match="image 1: the value %d does not fit a %d-bit image" % (value, bits)):
        png.encode(images=dev, bits=bits)
    path = str(tmp_path / "ids.png")
    with pytest.raises(ValueError) as by_device:
        ground_truth.write_id_png(path, dev[1], bits, device_png=True)
    with pytest.raises(ValueError) as by_host:
        ground_truth.write_id_png(path, dev[1], bits)
    assert str(by_device.value) == str(by_host.value) and str(value) in str(by_host.value)
    assert not os.path.exists(path)


def _raw(dev, bits, cap, guard=64, fill=0xA5, bounds=None):
    """cp_png_deflate on a filled buffer with `guard` bytes behind the capacity: (head, table, all bytes)."""
    import torch
    from centerpoly_amd import _C
    L = _C.lib()
    n, H, W = (int(v) for v in dev.shape)
    out = torch.full((cap + guard,), fill, dtype=torch.uint8, device=dev.device)
    table = torch.zeros((n, 4), dtype=torch.int32, device=dev.device)
    head = torch.zeros((4,), dtype=torch.int32, device=dev.device)
    nbytes = L.cp_png_deflate_workspace_bytes(n, H, W, bits)
    assert nbytes > 0
    ws = _C.workspace(nbytes, dev.device)
    planes = dev.dtype == torch.uint8
    _C.check(L.cp_png_deflate(_C.ptr(dev) if planes else None, None if planes else _C.ptr(dev), n, H, W, bits,
                              _C.ptr(bounds), _C.ptr(out), cap, _C.ptr(table), _C.ptr(head), _C.ptr(ws), nbytes,
                              _C.stream()), "cp_png_deflate")
    return head.cpu().numpy(), table.cpu().numpy(), out.cpu().numpy()


def test_capacities(monkeypatch):
    import torch
    from centerpoly_amd import _C
    from centerpoly_amd.utils import png
    rng = np.random.default_rng(21)
    a = np.stack([polygon_mask(33, 70, seed=k) for k in range(4)] + [rng.integers(0, 256, (33, 70)).astype(np.uint8)])
    refs = [_ref(p, 8) for p in a]
    total = sum(len(s) for s in refs)
    dev = torch.from_numpy(a).cuda()
    for cap in (total, total + 1, total + 2, total + 3, total + 64):       # every remainder of the capacity mod 4
        head, table, out = _raw(dev, 8, cap)
        assert head.tolist() == [total, 0, 0, 0]
        assert table[:, 1].tolist() == [len(s) for s in refs]
        assert table[:, 0].tolist() == np.cumsum([0] + [len(s) for s in refs[:-1]]).tolist()
        assert table[:, 2].tolist() == [int(p.min()) for p in a] and table[:, 3].tolist() == [int(p.max()) for p in a]
        assert out[:total].tobytes() == b"".join(refs)
        assert not out[total:cap].any() and (out[cap:] == 0xA5).all()
    for cap in (total - 1, total - 2, total - 3, 64, 5, 0):
        head, table2, out = _raw(dev, 8, cap)
        assert head.tolist() == [total, 1, 0, 0] and np.array_equal(table2, table)
        assert not out[:cap].any() and (out[cap:] == 0xA5).all()
    # the wrapper: capacity=64 is too small, and the second call, sized by the head, gives the streams
    calls = []
    inner = _C.check
    monkeypatch.setattr(png._C, "check", lambda rc, what="": (calls.append(what), inner(rc, what))[1])
    assert png.zlib_stream(planes=dev, capacity=64) == refs and calls == ["cp_png_deflate"] * 2
    del calls[:]
    assert png.zlib_stream(planes=dev) == refs and calls == ["cp_png_deflate"]


def test_arguments_are_checked_before_the_device():
    import torch
    from centerpoly_amd import _C
    L = _C.lib()
    dev = torch.zeros((1, 4, 5), dtype=torch.uint8, device="cuda")
    img = torch.zeros((1, 4, 5), dtype=torch.int32, device="cuda")
    out = torch.full((256 + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    table = torch.zeros((4,), dtype=torch.int32, device="cuda")
    head = torch.full((4,), 77, dtype=torch.int32, device="cuda")
    ws = _C.workspace(L.cp_png_deflate_workspace_bytes(1, 4, 5, 8), dev.device)
    p = _C.ptr

    def call(planes=dev, images=None, n=1, H=4, W=5, bits=8, o=out, cap=256, t=table, h=head, w=ws, wb=None):
        return L.cp_png_deflate(p(planes), p(images), n, H, W, bits, None, p(o), cap, p(t), p(h), p(w),
                                int(w.numel()) if w is not None and wb is None else (wb or 0), _C.stream())
    assert call() == 0
    assert call(planes=None) == -1 and call(images=img) == -1              # neither, both
    assert call(t=None) == -1 and call(h=None) == -1 and call(o=None) == -1
    assert call(bits=16) == -1 and call(bits=12) == -1 and call(n=0) == -1 and call(H=0) == -1 and call(cap=-1) == -1
    assert call(planes=None, images=img, bits=16) == 0
    assert call(n=129) == -2 and call(W=16385) == -2 and call(H=16385) == -2          # CP_EUNSUPPORTED
    assert call(n=128, H=16384, W=1024) == -2                                          # 2^31 stream bytes and more
    assert call(w=None) == -3 and call(wb=16) == -3                                    # CP_EWORKSPACE
    assert L.cp_png_deflate_workspace_bytes(129, 4, 5, 8) == 0 and L.cp_png_deflate_workspace_bytes(1, 4, 5, 12) == 0
    torch.cuda.synchronize()
    assert head.cpu().tolist()[1] == 0 and (out.cpu().numpy()[256:] == 0xA5).all()


@pytest.fixture(scope="module")
def street():
    """The seeded street scene at 2048 x 1024 (128 polygons drawn by the KITTI writer): its instance maps."""
    import torch
    from tools.probe_instances import H, W, realistic_rows
    from centerpoly_amd.datasets.dataset_factory import dataset_factory
    from centerpoly_amd.detectors import instances
    rows = torch.from_numpy(realistic_rows()).cuda()
    return instances.instance_maps(rows, dataset_factory["kitti_poly"], (W, H), thresh=0.05)


def test_full_size_planes(street):
    """4 planes of 1024 x 2048 (513 tiles each), with the polygons' bounds and without; and the 16-bit id image."""
    from centerpoly_amd.detectors import instances
    n = int(street.table["n"])
    assert n >= 4 and tuple(street.masks.shape[1:]) == (1024, 2048)
    pick = [0, 1, n // 2, n - 1]
    bounds = instances.vertex_bounds_host(street.table["poly"], instances.MARGIN[street.family], street.canvas)[pick]
    planes = street.masks[pick].cpu().numpy()
    assert all(p.any() for p in planes)
    with_bounds = _check(planes, 8, as_planes=True, bounds=bounds)
    assert _check(planes, 8, as_planes=True) == with_bounds
    ids = street.ids.cpu().numpy()
    assert ids.max() > 255
    _check(ids[None], 16)


# ------------------------------------------------------------------------------------------------------ writers --
def _same_tree(plain, device):
    """Two output directories: the same names; text and JSON byte for byte; every PNG pair the same mode, size, pixels.
    Returns the number of PNG pairs."""
    from PIL import Image
    names = sorted(os.path.relpath(os.path.join(r, f), plain) for r, _, fs in os.walk(plain) for f in fs)
    assert names == sorted(os.path.relpath(os.path.join(r, f), device) for r, _, fs in os.walk(device) for f in fs)
    pairs = 0
    for name in names:
        a, b = open(os.path.join(plain, name), "rb").read(), open(os.path.join(device, name), "rb").read()
        if not name.endswith(".png"):
            assert a == b, name
            continue
        x, y = Image.open(io.BytesIO(a)), Image.open(io.BytesIO(b))
        assert (x.mode, x.size) == (y.mode, y.size) and np.array_equal(np.array(x), np.array(y)), name
        assert a != b and b[37:41] == b"IDAT" and b[41:43] == b"\x78\x01", name        # it is the device's stream
        pairs += 1
    return pairs


@pytest.mark.parametrize("name", ["cityscapes", "kitti_poly"])
def test_save_masks_and_save_ids_with_the_flag_on_and_off(tmp_path, name):
    import shutil

    import torch
    from centerpoly_amd.datasets.evaluation import instance_level as il
    from centerpoly_amd.detectors import instances
    ds = tia._dataset(name)
    rows = tia._rows(len(ds.class_name) - 1)
    maps = instances.instance_maps(torch.from_numpy(rows).cuda(), ds, (tia.W, tia.H))
    stem = "frankfurt_a_leftImg8bit"
    dirs = {}
    for flag in (False, True):
        d = dirs[flag] = str(tmp_path / ("device" if flag else "plain"))
        instances.save_ids(maps, d, stem, device_png=flag)
        instances.save_masks(maps, d, stem, device_png=flag)
        live = tia._check_files(d, stem, maps)
    assert _same_tree(dirs[False], dirs[True]) == len(live) + 2
    if name == "cityscapes":
        assert len(live) < int(maps.table["n"])                            # dead slots: the kept planes are gathered
        gt = str(tmp_path / "frankfurt_a_gtFine_instanceIds.png")
        shutil.copy(os.path.join(dirs[True], stem + "_instanceIds.png"), gt)
        res = [il.evaluate_result_dir(dirs[flag], [gt]) for flag in (False, True)]
        assert res[0]["allAp"] == res[1]["allAp"] and 0.0 <= res[0]["allAp"] <= 1.0


def test_track_ids_with_the_flag(tmp_path):
    """`_trackIds.png` goes through write_id_png: a device id image with the flag on and off."""
    import torch
    from centerpoly_amd.datasets import ground_truth
    a = id_image(37, 53)
    dev = torch.from_numpy(a).cuda()
    for sub, flag in (("plain", False), ("device", True)):
        os.makedirs(str(tmp_path / sub))
        ground_truth.write_id_png(str(tmp_path / sub / "f_trackIds.png"), dev, 16, device_png=flag)
        ground_truth.write_id_png(str(tmp_path / sub / "f_labelIds.png"), torch.from_numpy(a // 1000).cuda(), 8,
                                  device_png=flag)
    assert _same_tree(str(tmp_path / "plain"), str(tmp_path / "device")) == 2
    ground_truth.write_id_png(str(tmp_path / "host.png"), a, 16, device_png=True)     # a host array: PIL, as before
    assert open(str(tmp_path / "host.png"), "rb").read() == open(str(tmp_path / "plain" / "f_trackIds.png"), "rb").read()


def test_cityscapes_run_eval_with_the_flag(tmp_path):
    import test_instance_ap as tap
    from centerpoly_amd.datasets.evaluation import instance_level as il
    aps, saves = [], []
    for sub, extra in (("plain", []), ("device", ["--device_png"])):
        ds, results = tap._dataset(tmp_path / sub, extra)
        saves.append(str(tmp_path / sub / "exp"))
        with contextlib.redirect_stdout(io.StringIO()):
            aps.append(ds.run_eval(results, saves[-1]))
    assert aps[0] == aps[1]
    np.testing.assert_allclose(aps[0], float(tap._rec("set")["all_ap"]), rtol=0, atol=1e-12)
    a, b = (os.path.join(s, "results") for s in saves)
    assert _same_tree(a, b) == sum(len(tap._rec(c)["lines"]) for c in tap.CASES)
    gt = sorted(il.find_gt_files(str(tmp_path / "device" / "gtFine")).values())
    assert il.evaluate_result_dir(b, gt)["allAp"] == il.evaluate_result_dir(a, gt)["allAp"] == aps[0]


def test_kitti_run_eval_with_the_flag(tmp_path):
    import test_kitti_idd_ap as tk
    from centerpoly_amd.datasets.evaluation import instance_level as il
    proto, scored, _ = tk.SETS["kitti"]
    aps, saves = [], []
    for sub, extra in (("plain", []), ("device", ["--device_png"])):
        ds, results = tk._dataset(tmp_path / sub, "kitti", extra)
        saves.append(str(tmp_path / sub / "exp"))
        with contextlib.redirect_stdout(io.StringIO()):
            aps.append(ds.run_eval(results, saves[-1]))
    assert aps[0] == aps[1]
    np.testing.assert_allclose(aps[0], float(tk._rec("set_kitti")["all_ap"]), rtol=0, atol=1e-12)
    a, b = (os.path.join(s, "results") for s in saves)
    assert _same_tree(a, b) == sum(len(tk._writer(c)["lines"]) for c in scored)
    gt = sorted(il.find_gt_files(str(tmp_path / "device" / "gt"), proto).values())
    assert il.evaluate_result_dir(b, gt, protocol=proto)["allAp"] == il.evaluate_result_dir(a, gt, protocol=proto)["allAp"]

"""cp_class_instance_masks / cp_class_writer_instances: the KITTI and IDD writers' masks and selection.

The fixtures (tests/golden/class_writer_*.npz) were drawn by PIL itself through the reference's two loops
(tests/golden/gen_class_writer_golden.py).  `pil_fill` / `pil_outline` are tests/golden/pil_scanline_host.py, a
transcription of centerpoly_amd/csrc/class_masks_core.h, the rules the kernels run: the CPU test holds them against
the installed PIL on seeded random polygons (zero differing pixels), the GPU tests hold the kernels against the
fixtures and against the transcription."""
import ctypes
import functools
import os
import types

import numpy as np
import pytest

from centerpoly_amd import _C
from pil_scanline_host import fill as pil_fill, outline as pil_outline

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = ["kitti_a", "kitti_b", "idd_a", "idd_b", "odd"]
f32 = np.float32


def _fix(name):
    return np.load(os.path.join(HERE, "golden", "class_writer_%s.npz" % name), allow_pickle=False)


def _fixture_masks(z):
    return np.unpackbits(z["packed"], axis=2)[:, :, :int(z["width"])].astype(np.uint8) * 255


def _per_class(rows, C):
    return {c + 1: np.delete(rows[rows[:, 5] == c], 5, axis=1) for c in range(C)}


def _dataset(z, thresh=None):
    from centerpoly_amd.datasets.dataset.polygons import IDD, KITTIPOLY
    cls = IDD if int(z["at_threshold"]) else KITTIPOLY
    ds = cls.__new__(cls)
    ds.opt = types.SimpleNamespace(thresh=float(z["thresh"]) if thresh is None else thresh)
    assert [ds.label_to_id[c] for c in ds.class_name[1:]] == z["labels"].tolist()
    return ds


@functools.lru_cache(maxsize=None)
def _fill_outline(pts, W, H):
    """(F, O) of the polygon `pts`, a tuple of (x, y): computed once, shared by the tests, never written to."""
    return pil_fill(pts, W, H), pil_outline(pts, W, H)


def host_masks(polys, groups, flags, W, H):
    """mask_i = (F_i \\ O_i) \\ union of F_j over earlier occluding instances of the group."""
    out, removed = [], {}
    for pts, g, fl in zip(polys, groups, flags):
        if not fl & 1:
            out.append(np.zeros((H, W), np.uint8))
            continue
        F, O = _fill_outline(tuple(pts), W, H)
        rem = removed.setdefault(g, np.zeros((H, W), bool))
        out.append(((F & ~O & ~rem) * 255).astype(np.uint8))
        if fl & 2:
            rem |= F
    return np.stack(out)


def _random_polygon(rng, t, W, H):
    n = int(rng.randint(3, 17))
    m = int(rng.randint(1, max(W, H)))
    pts = np.stack([rng.randint(-m, W + m, n), rng.randint(-m, H + m, n)], 1)
    kind = t % 5
    if kind == 1:                                            # repeated, collinear, flat and upright
        for _ in range(int(rng.randint(1, 5))):
            i = int(rng.randint(0, n))
            j, c = (i + 1) % n, int(rng.randint(0, 4))
            if c == 0:
                pts[j] = pts[i]
            elif c == 1:
                pts[j, 1] = pts[i, 1]
            elif c == 2:
                pts[j, 0] = pts[i, 0]
            else:
                pts[j] = (pts[i] + pts[(i + 2) % n]) // 2
    elif kind == 2:                                          # star
        th = np.sort(rng.uniform(0, 2 * np.pi, n))
        r = rng.uniform(1, max(W, H) / 2.0, n)
        pts = (np.array([rng.randint(0, W), rng.randint(0, H)]) + np.stack([r * np.cos(th), r * np.sin(th)], 1)).astype(np.int64)
    elif kind == 3:                                          # a few pixels: vertices and edges coincide
        pts = np.stack([rng.randint(0, 8, n), rng.randint(0, 8, n)], 1)
    elif kind == 4:                                          # closed by hand: PIL adds no closing edge
        pts[-1] = pts[0]
    return [tuple(int(v) for v in p) for p in pts]


# ------------------------------------------------------------------------------------------------------- CPU --
def test_restatement_equals_the_installed_pil():
    """5200 seeded polygons, every one compared, zero differing pixels, fill and outline each, and their
    combination against polygon(outline=0, fill=255)."""
    import PIL
    from PIL import Image, ImageDraw
    recorded = str(_fix("kitti_a")["pil_version"])
    if PIL.__version__ != recorded:
        pytest.skip("the fixtures and class_masks_core.h were fitted against PIL %s, installed is %s"
                    % (recorded, PIL.__version__))
    rng = np.random.RandomState(7)
    differing = []
    for t in range(5200):
        W, H = (int(rng.randint(200, 1300)), int(rng.randint(100, 400))) if t % 26 == 25 else \
            (int(rng.randint(5, 70)), int(rng.randint(5, 70)))
        pts = _random_polygon(rng, t, W, H)
        imgs = []
        for kw in ({"fill": 255}, {"outline": 255}, {"outline": 0, "fill": 255}):
            im = Image.new("L", (W, H), 0)
            ImageDraw.Draw(im).polygon(pts, **kw)
            imgs.append(np.array(im) > 0)
        F, O = pil_fill(pts, W, H), pil_outline(pts, W, H)
        bad = int((F != imgs[0]).sum() + (O != imgs[1]).sum() + ((F & ~O) != imgs[2]).sum())
        if bad:
            differing.append((t, W, H, pts, bad))
    assert not differing, "%d polygons differ, first: %r" % (len(differing), differing[0])


def test_issue_examples():
    """The rows the issue quotes from PIL."""
    row = lambda pts, y: np.flatnonzero(pil_fill(pts, 64, 32)[y]).tolist()   # noqa: E731
    assert row([(21, 11), (32, 16), (29, 16)], 11) == [21, 22]
    assert row([(47, 8), (34, 4), (47, 7)], 4) == [34, 35, 36] and row([(47, 8), (34, 4), (47, 7)], 5) == [37, 38]
    assert row([(6, 10), (37, 27), (17, 15)], 10) == [6, 7] and row([(6, 10), (37, 27), (17, 15)], 27) == [36, 37]
    assert row([(28, 4), (11, 14), (9, 7)], 4) == [27, 28]


@pytest.mark.parametrize("name", CASES)
def test_host_selection_reproduces_the_recorded_lines(name):
    """image_instances (the host restatement run_eval uses): text lines, their order and the drawing order."""
    z = _fix(name)
    ds = _dataset(z)
    params = ds.image_instances(_per_class(z["rows"], len(z["labels"])))
    base = os.path.basename(str(z["file_name"]))
    by_line = sorted(range(len(params)), key=lambda k: params[k][4])
    lines = ["%s %d %s\n" % (base.replace(".png", "_%d.png" % params[k][4]), z["labels"][params[k][2]], str(params[k][1]))
             for k in by_line]
    assert lines == [str(l) for l in z["lines"]]
    assert [p[4] for p in params] == z["drawn"].tolist()
    assert [p[4] for p in sorted(params, key=lambda p: p[4])] == list(range(len(params)))


def test_fixtures_are_worth_having():
    for name in CASES:
        z = _fix(name)
        rows, th = z["rows"], f32(float(z["thresh"]))
        assert (rows[:, 4] == f32(0.5)).any() and (rows[:, 4] == th).any()
        kept = int((rows[:, 4] >= th).sum() if int(z["at_threshold"]) else (rows[:, 4] > th).sum())
        assert kept == len(z["lines"]) and (kept == int((rows[:, 4] > th).sum())) != bool(int(z["at_threshold"]))
        assert len(np.unique(rows[rows[:, 4] > th][:, 5])) >= 3
    # occlusion stays inside a class: some pixel belongs to masks of two classes, none to two masks of one class
    z = _fix("kitti_a")
    masks, labels = _fixture_masks(z) > 0, np.array([int(str(l).split(" ")[1]) for l in z["lines"]])
    confident = np.array([float(str(l).split(" ")[2]) >= 0.5 for l in z["lines"]])
    assert (masks.sum(0) >= 2).any()
    for lab in np.unique(labels):
        assert (masks[(labels == lab) & confident].sum(0) <= 1).all()


def test_abi_limits_without_gpu():
    """Both entries refuse what they cannot do before any device work: callable with no GPU."""
    L = _C.lib()
    p = ctypes.c_void_p(256)                                # never dereferenced: every call below returns first
    masks = lambda n, N, H, W: L.cp_class_instance_masks(p, p, p, n, N, H, W, p, p, None)   # noqa: E731
    assert masks(129, 16, 8, 8) == -2 and masks(4, 65, 8, 8) == -2 and masks(4, 16, 65536, 32768) == -2
    assert masks(4, 2, 8, 8) == -1 and masks(4, 16, 0, 8) == -1 and masks(-1, 16, 8, 8) == -1
    assert L.cp_class_instance_masks(p, None, p, 4, 16, 8, 8, p, p, None) == -1
    assert masks(0, 16, 8, 8) == 0                          # nothing to draw: no device touched
    sel = lambda R, N, C, mode, thresh=0.3: L.cp_class_writer_instances(      # noqa: E731
        p, R, N, thresh, mode, p, C, p, p, p, p, p, p, p, p, None)
    assert sel(1025, 16, 8, 0) == -2 and sel(8, 65, 8, 0) == -2 and sel(8, 16, 33, 0) == -2
    assert sel(0, 16, 8, 0) == -1 and sel(8, 2, 8, 0) == -1 and sel(8, 16, 8, 2) == -1
    assert sel(8, 16, 8, 0, float("nan")) == -1
    assert L.cp_class_writer_instances(p, 8, 16, 0.3, 0, None, 8, p, p, p, p, p, p, p, p, None) == -1


# ------------------------------------------------------------------------------------------------------- GPU --
def _device_masks(polys, groups, flags, W, H):
    import torch
    n, N = len(polys), len(polys[0])
    poly = torch.tensor(polys, dtype=torch.int32).reshape(n, N, 2).cuda()
    grp = torch.tensor(groups, dtype=torch.int32).cuda()
    fl = torch.tensor(flags, dtype=torch.uint8).cuda()
    masks = torch.full((n, H, W), 77, dtype=torch.uint8, device="cuda")      # every byte has to be written
    counts = torch.full((n,), -5, dtype=torch.int32, device="cuda")
    _C.check(_C.lib().cp_class_instance_masks(_C.ptr(poly), _C.ptr(grp), _C.ptr(fl), n, N, H, W, _C.ptr(masks),
                                              _C.ptr(counts), _C.stream()), "cp_class_instance_masks")
    return masks.cpu().numpy(), counts.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_masks_equal_the_fixtures(name):
    z = _fix(name)
    W, H = int(z["width"]), int(z["height"])
    ds = _dataset(z)
    params = ds.image_instances(_per_class(z["rows"], len(z["labels"])))
    polys, groups = [p[0] for p in params], [p[2] for p in params]
    flags = [1 | (2 if p[1] >= 0.5 else 0) for p in params]
    masks, counts = _device_masks(polys, groups, flags, W, H)
    want = _fixture_masks(z)
    line = [p[4] for p in params]                           # the fixtures are in text-line order
    for k in range(len(params)):
        assert np.array_equal(masks[k], want[line[k]]), "mask of text line %d" % line[k]
    assert counts.tolist() == z["counts"][line].tolist()
    again = _device_masks(polys, groups, flags, W, H)       # the same bits on a second run
    assert np.array_equal(again[0], masks) and np.array_equal(again[1], counts)
    for g in sorted(set(groups)):                           # a group at a time gives the same masks
        sel = [k for k in range(len(params)) if groups[k] == g]
        part = _device_masks([polys[k] for k in sel], [g] * len(sel), [flags[k] for k in sel], W, H)
        assert np.array_equal(part[0], masks[sel]) and np.array_equal(part[1], counts[sel])
    # through the data set's own call, as run_eval makes it
    m2, c2 = ds.class_masks_device(params, (W, H))
    assert np.array_equal(m2.cpu().numpy(), masks) and np.array_equal(c2.cpu().numpy(), counts)


def _random_instances(rng, W, H, N):
    polys = []
    for t in range(128):
        pts = _random_polygon(rng, t, W, H)
        polys.append((pts * N)[:N] if len(pts) < N else pts[:N])             # N vertices: the polygon walked again
    return polys


@pytest.mark.gpu
@pytest.mark.parametrize("W,H,N,seed", [(97, 61, 16, 0), (64, 48, 7, 1), (33, 130, 64, 2), (2, 3, 3, 3)])
def test_masks_equal_the_transcription_on_random_polygons(W, H, N, seed):
    """Beyond the fixtures, without PIL: 128 random instances a call, groups interleaved, some not drawn."""
    rng = np.random.RandomState(seed)
    polys = _random_instances(rng, W, H, N)
    groups = [int(g) for g in rng.randint(-2, 3, 128) * 1000003]
    flags = [int(f) for f in rng.choice([0, 1, 3, 3], 128)]
    masks, counts = _device_masks(polys, groups, flags, W, H)
    want = host_masks(polys, groups, flags, W, H)
    bad = [k for k in range(128) if not np.array_equal(masks[k], want[k])]
    assert not bad, "instances %r differ" % bad[:8]
    assert counts.tolist() == (want > 0).sum((1, 2)).tolist()


@pytest.mark.gpu
@pytest.mark.parametrize("W,H,N,seed", [(97, 61, 16, 0), (33, 130, 64, 2), (2, 3, 3, 3)])
def test_wave_and_workgroup_scan_lines_agree(W, H, N, seed):
    """The two forms of csrc/scanline.h share neither sort nor compaction: the polygons of the test above, each alone
    in its group and drawn, through cp_class_instance_masks (wave form), cp_polygon_masks (workgroup form, stores to
    memory) and cp_polygon_paint (workgroup form, stores to LDS) against the host F and O, byte for byte.  A width
    that is no multiple of 16, the wave form's 64 vertices, a canvas smaller than one store."""
    import torch
    from centerpoly_amd.datasets import ground_truth
    polys = _random_instances(np.random.RandomState(seed), W, H, N)
    n = len(polys)
    FO = [_fill_outline(tuple(pts), W, H) for pts in polys]
    want = np.stack([((F & ~O) * 255).astype(np.uint8) for F, O in FO])
    wave, wave_counts = _device_masks(polys, list(range(n)), [1] * n, W, H)
    L = _C.lib()
    xy = torch.tensor(polys, dtype=torch.int32).reshape(n * N, 2).cuda()
    first = (ctypes.c_int32 * (n + 1))(*range(0, n * N + 1, N))
    group = torch.full((n, H, W), 77, dtype=torch.uint8, device="cuda")
    counts = torch.full((n,), -5, dtype=torch.int32, device="cuda")
    nbytes = L.cp_polygon_masks_workspace_bytes(n, n * N)
    ws = _C.workspace(nbytes, "cuda")
    _C.check(L.cp_polygon_masks(_C.ptr(xy), first, n, H, W, _C.ptr(group), _C.ptr(counts), _C.ptr(ws), nbytes,
                                _C.stream()), "cp_polygon_masks")
    group = group.cpu().numpy()
    assert np.array_equal(wave, want) and np.array_equal(group, want) and np.array_equal(wave, group)
    assert wave_counts.tolist() == counts.cpu().numpy().tolist() == (want > 0).sum((1, 2)).tolist()
    painted = torch.stack([ground_truth.paint([np.array(pts, np.int32)], [255], 0, (W, H), "cuda") for pts in polys])
    bad = [k for k in range(n) if not np.array_equal(painted[k].cpu().numpy(), FO[k][0] * 255)]
    assert not bad, "painted polygons %r differ from the host fill" % bad[:8]


def _host_selection(z, ds):
    """The reference's loop on the rows: per instance in drawing order (row, text index, class)."""
    rows, th = z["rows"], f32(ds.opt.thresh)
    out, count = [], 0
    for c in range(len(z["labels"])):
        live = [r for r in range(len(rows)) if rows[r, 5] == c and (rows[r, 4] >= th if ds.at_threshold else rows[r, 4] > th)]
        numbered = [(r, count + i) for i, r in enumerate(live)]
        count += len(live)
        out += [(r, t, c) for r, t in sorted(numbered, key=lambda a: rows[a[0], -1])]
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("mode", [0, 1])
def test_selection_kernel(name, mode):
    import torch
    z = _fix(name)
    ds = _dataset(z)
    ds.at_threshold = bool(mode)                            # both rules on every fixture
    rows = z["rows"]
    R, N, C = len(rows), (rows.shape[1] - 7) // 2, len(z["labels"])
    want = _host_selection(z, ds)
    dev = torch.from_numpy(rows).cuda()
    i32 = lambda *s: torch.full(s, -77, dtype=torch.int32, device="cuda")      # noqa: E731
    n_out, src, poly, group, label, text = i32(1), i32(R), i32(R, N, 2), i32(R), i32(R), i32(R)
    flags = torch.full((R,), 9, dtype=torch.uint8, device="cuda")
    conf = torch.full((R,), -1.0, dtype=torch.float32, device="cuda")
    table = np.ascontiguousarray(ds.class_label_table())
    _C.check(_C.lib().cp_class_writer_instances(_C.ptr(dev), R, N, float(z["thresh"]), mode,
                                                table.ctypes.data_as(ctypes.c_void_p), C, _C.ptr(n_out), _C.ptr(src),
                                                _C.ptr(poly), _C.ptr(group), _C.ptr(flags), _C.ptr(label),
                                                _C.ptr(conf), _C.ptr(text), _C.stream()), "cp_class_writer_instances")
    n = int(n_out.cpu()[0])
    assert n == len(want) and (mode == 1) == (n == int((rows[:, 4] >= f32(float(z["thresh"]))).sum()))
    assert src.cpu().numpy()[:n].tolist() == [w[0] for w in want]
    assert text.cpu().numpy()[:n].tolist() == [w[1] for w in want]
    assert group.cpu().numpy()[:n].tolist() == [w[2] for w in want]
    assert label.cpu().numpy()[:n].tolist() == [int(z["labels"][w[2]]) for w in want]
    got_conf = conf.cpu().numpy()
    assert got_conf[:n].view(np.uint32).tolist() == rows[[w[0] for w in want], 4].view(np.uint32).tolist()
    assert flags.cpu().numpy()[:n].tolist() == [1 | (2 if rows[w[0], 4] >= f32(0.5) else 0) for w in want]
    to_int = lambda v: int(float("%.2f" % v))               # noqa: E731
    want_poly = [[to_int(v) for v in rows[w[0], 6:6 + 2 * N]] for w in want]
    assert poly.cpu().numpy()[:n].reshape(n, -1).tolist() == want_poly
    # dead slots draw nothing
    assert (src.cpu().numpy()[n:] == -1).all() and (flags.cpu().numpy()[n:] == 0).all()
    assert (text.cpu().numpy()[n:] == -1).all() and (got_conf[n:] == 0).all() and (poly.cpu().numpy()[n:] == 0).all()
    if mode == int(z["at_threshold"]):                      # the recorded lines, from the kernel's tables alone
        order = np.argsort(text.cpu().numpy()[:n], kind="stable")
        base = os.path.basename(str(z["file_name"]))
        lines = ["%s %d %s\n" % (base.replace(".png", "_%d.png" % t), label.cpu().numpy()[k], str(got_conf[k]))
                 for t, k in enumerate(order)]
        assert lines == [str(l) for l in z["lines"]]

"""Detection overlays rendered on the GPU: cp_render_overlay / cp_render_heatmap, utils/debugger.py, the detectors'
--debug views and demo.py.

The reference for every picture is the host statement tests/golden/render_host.py (the installed PIL's polygon fill,
polygon outline and bitmap font; numpy for everything else; a loop in which a later operation overwrites an earlier
one).  Pictures are 8-bit integers produced by integer arithmetic (the heat-map view by float32 steps that numpy
rounds the same way), so every comparison is exact."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest

import render_host as rh
from centerpoly_amd import _C
from centerpoly_amd.utils import debugger as dbg

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NAMES8 = ["person", "rider", "car", "truck", "bus", "train", "motorcycle", "bicycle"]
NAMES11 = NAMES8 + ["pole", "traffic sign", "traffic light"]


def _demo_module():
    spec = importlib.util.spec_from_file_location("cp_demo", os.path.join(ROOT, "demo.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _palette(C):
    return np.ascontiguousarray(dbg.palette_rgb(C)[:, ::-1])             # BGR, as the drivers hand it


def _image(H, W, seed):
    """A smooth gradient plus noise: no large area equals any palette colour."""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    base = np.stack([(xx * 3 + yy) % 200, (xx + yy * 2) % 180 + 20, (xx * 2 + yy * 3) % 160 + 40], 2)
    return np.ascontiguousarray(np.clip(base + rng.randint(0, 30, (H, W, 3)), 0, 255).astype(np.uint8))


# ------------------------------------------------------------------------------------------------- cases --
def _stack(det):
    rows = [np.concatenate([r[:, :5], np.full((len(r), 1), c - 1, np.float32), r[:, 5:]], axis=1)
            for c, r in sorted(det.items())]
    return np.ascontiguousarray(np.concatenate(rows, axis=0), np.float32)


def _writer_rows(name):
    z = np.load(os.path.join(HERE, "golden", "writer_%s.npz" % name), allow_pickle=False)
    return _stack({int(k[4:]): z[k] for k in z.files if k.startswith("det_")})


def _class_writer(name):
    z = np.load(os.path.join(HERE, "golden", "class_writer_%s.npz" % name), allow_pickle=False)
    return np.ascontiguousarray(z["rows"], np.float32), int(z["height"]), int(z["width"])


def _row(pts, score, cls, depth, box=None):
    pts = np.asarray(pts, np.float32)
    if box is None:
        box = [pts[:, 0].min(), pts[:, 1].min(), pts[:, 0].max(), pts[:, 1].max()]
    return np.concatenate([box, [score, cls], pts.reshape(-1), [depth]]).astype(np.float32)


def _generated_rows(W, H, seed, N=16):
    """Self-crossing, degenerate (repeated vertices, zero area, one point), partly and wholly off-canvas polygons,
    fractions at the writers' two-decimal rule, equal depths within and across classes, one vertex beyond +-2^29."""
    rng = np.random.RandomState(seed)
    m = min(W, H)
    rows = []
    th = np.sort(rng.uniform(0, 2 * np.pi, N))
    star = lambda cx, cy, r: np.stack([cx + r * np.cos(th), cy + r * np.sin(th)], 1)          # noqa: E731
    rows.append(_row(star(W * 0.5, H * 0.55, rng.uniform(0.25, 0.45, N) * m), 0.91, 2, 5.0))  # a large one
    cross = rng.uniform(0, 2 * np.pi, N)                                                      # self-crossing
    rows.append(_row(np.stack([W * 0.3 + 0.3 * m * np.cos(cross), H * 0.4 + 0.3 * m * np.sin(cross)], 1), 0.62, 0, 5.0))
    rep = star(W * 0.7, H * 0.5, 0.2 * m)                                                     # repeated vertices
    rep[3] = rep[2]; rep[4] = rep[2]; rep[-1] = rep[0]
    rows.append(_row(rep, 0.55, 2, 5.0))                                                      # (depth tie, same class)
    line = np.stack([np.linspace(2, W - 3, N), np.linspace(H * 0.2, H * 0.8, N)], 1)          # zero area
    rows.append(_row(line, 0.7, 5, 9.5))
    rows.append(_row(np.full((N, 2), [W * 0.25, H * 0.75]), 0.8, 1, 1.0,                      # one point, a real box
                     box=[W * 0.2, H * 0.7, W * 0.3, H * 0.8]))
    rows.append(_row(star(W * 0.02, H * 0.1, 0.3 * m), 0.45, 7, 2.0))                         # partly off, top left
    rows.append(_row(star(W * 0.99, H * 0.98, 0.35 * m), 0.5, 3, 2.0))                        # partly off, bottom right
    rows.append(_row(star(-3.0 * W, -2.0 * H, 0.4 * m), 0.99, 4, 0.5))                        # wholly off
    rows.append(_row(star(W * 0.5, H * 4.0, 0.4 * m), 0.99, 4, 0.25))
    frac = np.floor(star(W * 0.6, H * 0.3, 0.15 * m)) + np.resize([0.994, 0.996, 0.5, 0.004], (N, 2))
    rows.append(_row(frac, 0.66, 6, 7.25))                                                    # the two-decimal rule
    rows.append(_row(star(W * 0.4, H * 0.6, 0.1 * m), 0.1, 0, 0.1))                           # below the threshold
    wild = star(W * 0.45, H * 0.5, 0.2 * m)                                                   # a vertex beyond 2^29: the
    wild[5] = (3.0e9, -7.0e8)                                                                 # polygon is not drawn, its
    rows.append(_row(wild, 0.77, 3, 3.0, box=[W * 0.35, H * 0.4, W * 0.55, H * 0.6]))         # box and label are
    return np.stack(rows)


def _many_rows(W, H, R, seed, N=16):
    rng = np.random.RandomState(seed)
    rows = []
    for k in range(R):
        th = np.sort(rng.uniform(0, 2 * np.pi, N))
        r = rng.uniform(15, 160, N)
        c = [rng.uniform(0, W), rng.uniform(0, H)]
        rows.append(_row(np.stack([c[0] + r * np.cos(th), c[1] + r * np.sin(th)], 1), rng.uniform(0.3, 1.0),
                         rng.randint(0, 8), rng.uniform(0, 50)))
    return np.stack(rows)


def _case(name):
    """-> (rows, H, W, names, thresh, keyword arguments of the picture)."""
    if name == "writer_star16":
        return _writer_rows("star16"), 1024, 2048, NAMES11, 0.05, {}
    if name == "writer_mixed32":
        return _writer_rows("mixed32"), 1024, 2048, NAMES11, 0.05, {"white": True}
    if name == "writer_selfcross16":
        return _writer_rows("selfcross16"), 1024, 2048, NAMES11, 0.05, {"alpha": 256, "r": 3}
    if name == "writer_small16":
        # (twelve polygons of 2 to 14 pixels radius cannot change 1 % of their own 1024 x 2048 canvas and keep a
        # visible fill; on the KITTI canvas, where the upper left ones fall, a wider outline and frame do)
        return _writer_rows("small16"), 375, 1242, NAMES11, 0.02, {"r": 4, "t": 6, "white": True}
    if name.startswith("class_writer_"):
        rows, H, W = _class_writer(name[len("class_writer_"):])
        kw = {"kitti_a": {}, "kitti_b": {"show_txt": False, "white": True}, "idd_a": {"alpha": 0},
              "idd_b": {"r": 0, "white": True}, "odd": {"alias": True}}[name[len("class_writer_"):]]
        return rows, H, W, NAMES8, 0.0, kw
    if name == "generated_375x1242":
        return _generated_rows(1242, 375, 11), 375, 1242, NAMES8, 0.3, {"alias": True}
    if name == "generated_37x53":
        return _generated_rows(53, 37, 12), 37, 53, NAMES8, 0.3, {"white": True, "r": 0}
    if name == "generated_1024x2048_notxt":
        return _generated_rows(2048, 1024, 13), 1024, 2048, NAMES8, 0.3, {"show_txt": False, "alpha": 256}
    if name == "n128":
        return _many_rows(2048, 1024, 128, 21), 1024, 2048, NAMES8, 0.2, {"alias": True}
    raise KeyError(name)


CASES = ["writer_star16", "writer_mixed32", "writer_selfcross16", "writer_small16", "class_writer_kitti_a",
         "class_writer_kitti_b", "class_writer_idd_a", "class_writer_idd_b", "class_writer_odd",
         "generated_375x1242", "generated_37x53", "generated_1024x2048_notxt", "n128"]


def _host_picture(name):
    rows, H, W, names, thresh, kw = _case(name)
    kw = {k: v for k, v in kw.items() if k != "alias"}
    image = _image(H, W, len(name))
    pic, winner = rh.overlay(image, rows, thresh, names, _palette(len(names)), **kw)
    return image, pic, winner, kw


# --------------------------------------------------------------------------------------------------- CPU --
def test_options_and_defaults():
    from centerpoly_amd.opts import opts
    o = opts().parse(["polydet"])
    assert (o.demo, o.vis_thresh, o.debugger_theme, o.center_thresh, o.debug) == ("", 0.3, "white", 0.1, 0)
    o = opts().parse(["polydet", "--demo", "imgs", "--vis_thresh", "0.5", "--debugger_theme", "black",
                      "--center_thresh", "0.2", "--debug", "2"])
    assert (o.demo, o.vis_thresh, o.debugger_theme, o.center_thresh, o.debug) == ("imgs", 0.5, "black", 0.2, 2)
    with pytest.raises(SystemExit):
        opts().parse(["polydet", "--debugger_theme", "green"])


def test_demo_file_listing_and_refusals(tmp_path):
    demo = _demo_module()
    for f in ["b.png", "a.JPG", "c.jpeg", "d.webp", "notes.txt", "e.npy", "z.PNG", "clip.mp4"]:
        (tmp_path / f).write_bytes(b"")
    got = demo.image_names(str(tmp_path))
    assert [os.path.basename(p) for p in got] == ["a.JPG", "b.png", "c.jpeg", "d.webp", "z.PNG"]
    assert demo.image_names(str(tmp_path / "b.png")) == [str(tmp_path / "b.png")]
    for bad in ("webcam", "film.mp4", "x.MOV", "y.avi", "z.mkv"):
        with pytest.raises(ValueError, match="no video decoder"):
            demo.image_names(bad)
    with pytest.raises(ValueError):
        demo.image_names("")


def test_run_loads_image_files_as_bgr(tmp_path):
    from PIL import Image
    from centerpoly_amd.detectors.base_detector import load_image
    rgb = _image(21, 34, 3)
    Image.fromarray(rgb).save(str(tmp_path / "a.png"))
    Image.fromarray(rgb).save(str(tmp_path / "a.jpg"), quality=90)
    np.save(str(tmp_path / "a.npy"), rgb)
    got = load_image(str(tmp_path / "a.png"))
    assert got.dtype == np.uint8 and got.flags["C_CONTIGUOUS"] and np.array_equal(got, rgb[:, :, ::-1])
    decoded = np.asarray(Image.open(str(tmp_path / "a.jpg")).convert("RGB"))
    assert np.array_equal(load_image(str(tmp_path / "a.jpg")), decoded[:, :, ::-1])
    assert np.array_equal(load_image(str(tmp_path / "a.npy")), rgb)      # an array file is the array, untouched


def test_atlas_palette_and_labels():
    a, b = dbg.glyph_atlas(), dbg.glyph_atlas()
    assert a.shape == (96, 11, 6) and a.dtype == np.uint8 and np.array_equal(a, b) and set(np.unique(a)) == {0, 1}
    assert not a[0].any() and a[ord("A") - 32].any()
    for ch in "g0.5":                                                    # the production atlas against PIL, directly
        assert np.array_equal(a[ord(ch) - 32] != 0, rh.glyph(ch))
    p = dbg.palette_rgb(8)
    assert p.shape == (8, 3) and p.dtype == np.uint8 and np.array_equal(p, dbg.palette_rgb(8))
    assert np.array_equal(dbg.palette_rgb(32)[:8], p)                    # a function of the class index alone
    assert len({tuple(c) for c in p.tolist()}) == 8
    assert dbg.label_text("car", np.float32(0.449)) == "car0.4" == rh.label("car", np.float32(0.449))
    assert dbg.label_text("traffic light", 0.96) == "traffic light1.0"[:16] and len(dbg.label_text("x" * 30, 1)) == 16
    codes = dbg.label_codes("aé~")
    assert codes.tolist() == [ord("a") - 32, 0, ord("~") - 32] + [-1] * 13
    d = dbg.Debugger(NAMES8, device="cpu")
    rows = np.zeros((3, 39), np.float32)
    rows[:, 4], rows[:, 5] = [0.5, 0.26, 0.9], [2, 7, 9]
    got = d.row_labels(rows)
    assert got[0].tolist() == dbg.label_codes("car0.5").tolist() and got[1].tolist() == dbg.label_codes("bicycle0.3").tolist()
    assert (got[2] == -1).all()                                          # no such class: no label


def test_known_answer_one_triangle():
    """One instance on a 28 x 40 canvas, every number below worked out by hand: the right triangle (4,16) (10,16)
    (4,22) (PIL fills rows 16..22 from x = 4 to 10 - (y - 16) and outlines its border), box (3,15,11,23) with
    t = 1, label 'g0.5' (4 cells: x 3..26, y 3..13), r = 0, alpha = 128."""
    H, W = 28, 40
    image = np.empty((H, W, 3), np.uint8)
    image[:] = (50, 100, 150)
    pts = np.zeros((16, 2), np.float32)
    pts[:] = (4, 22)
    pts[0], pts[1] = (4, 16), (10.4, 16.994)                             # 16.994 -> 16.99 -> 16; repeats close it
    row = _row(pts, 0.52, 0, 1.0, box=[3.7, 15.2, 11.9, 23.5])
    pic, winner = rh.overlay(image, row[None], 0.3, ["g"], np.array([[200, 40, 90]], np.uint8), alpha=128, r=0, t=1)
    want = image.copy()
    op = np.zeros((H, W), np.uint8)
    for y in range(16, 23):
        for x in range(4, 10 - (y - 16) + 1):
            edge = y == 16 or x == 4 or x == 10 - (y - 16)
            want[y, x] = (0, 255, 255) if edge else (125, 70, 120)       # (50 * 128 + 200 * 128 + 128) >> 8 = 125, ...
            op[y, x] = 2 if edge else 1
    for y in range(15, 24):
        for x in range(3, 12):
            if y in (15, 23) or x in (3, 11):
                want[y, x], op[y, x] = (200, 40, 90), 3
    want[3:14, 3:27], op[3:14, 3:27] = (200, 40, 90), 4
    glyphs = {"g": ["......", "......", "......", "......", ".##.##", "##.##.", "##.##.", "##.##.", ".####.", "...##.", "####.."],
              "0": ["......", "......", ".###..", "##.##.", "##.##.", "##.##.", "##.##.", "##.##.", ".###..", "......", "......"],
              ".": ["......", "......", "......", "......", "......", "......", "......", "......", ".##...", "......", "......"],
              "5": ["......", "......", "#####.", "##....", "####..", "##.##.", "...##.", "#..##.", "####..", "......", "......"]}
    for j, ch in enumerate("g0.5"):
        for cy, line in enumerate(glyphs[ch]):
            for cx, v in enumerate(line):
                if v == "#":
                    want[3 + cy, 3 + 6 * j + cx], op[3 + cy, 3 + 6 * j + cx] = (0, 0, 0), 5
    assert np.array_equal(winner, op)
    assert np.array_equal(pic, want)
    rh.check_condition(image, pic, winner)
    # the white theme inverts the class colour (fill, box, label background), not the outline or the glyphs
    pic_w, winner_w = rh.overlay(image, row[None], 0.3, ["g"], np.array([[200, 40, 90]], np.uint8), white=True,
                                 alpha=128, r=0, t=1)
    assert np.array_equal(winner_w, op)
    assert pic_w[15, 3].tolist() == [55, 215, 165] and pic_w[18, 5].tolist() == [53, 158, 158]
    assert pic_w[16, 4].tolist() == [0, 255, 255] and np.array_equal(pic_w[op == 5], pic[op == 5])
    # a threshold at the score draws nothing: strict
    pic_0, winner_0 = rh.overlay(image, row[None], float(np.float32(0.52)), ["g"], np.array([[200, 40, 90]], np.uint8))
    assert np.array_equal(pic_0, image) and not winner_0.any()


def test_host_statement_order_and_dilation():
    """Nearest last: of two overlapping squares the nearer one's fill shows; equal depths fall to class, then row;
    r dilates the outline by a square."""
    H, W = 40, 60
    image = np.full((H, W, 3), 10, np.uint8)
    def sq(x0, y0, s):                                                   # 16 points round a square, 4 a side
        f = np.arange(4) * s / 4.0
        return np.concatenate([np.stack([x0 + f, np.full(4, y0)], 1), np.stack([np.full(4, x0 + s), y0 + f], 1),
                               np.stack([x0 + s - f, np.full(4, y0 + s)], 1), np.stack([np.full(4, x0), y0 + s - f], 1)])
    pal = np.array([[250, 0, 0], [0, 250, 0]], np.uint8)
    kw = dict(show_txt=False, alpha=256, r=0, t=0)
    rows = np.stack([_row(sq(10, 10, 20), 0.9, 0, 3.0), _row(sq(20, 15, 20), 0.9, 1, 2.0)])
    pic, _ = rh.overlay(image, rows, 0.3, ["a", "b"], pal, **kw)
    assert pic[20, 25].tolist() == [0, 250, 0] and pic[12, 12].tolist() == [250, 0, 0]
    rows[:, -1] = 2.0                                                    # a tie: class 0 is "nearer", drawn last
    pic, _ = rh.overlay(image, rows, 0.3, ["a", "b"], pal, **kw)
    assert pic[20, 25].tolist() == [250, 0, 0]
    assert [i[0] for i in rh.instances(rows, 0.3, 2)] == [0, 1]
    one = np.zeros((9, 9), bool)
    one[0, 0] = one[4, 4] = True
    d = rh.dilate(one, 2)
    assert d.sum() == 9 + 25 - 1 and d[:3, :3].all() and d[2:7, 2:7].all() and not d[0, 3]


@pytest.mark.parametrize("name", CASES)
def test_cases_draw_something_of_every_kind(name):
    """The condition on the host statement alone: at least 1 % of the pixels change and every operation kind wins
    a pixel, so an empty drawing cannot pass the device comparison."""
    image, pic, winner, kw = _host_picture(name)
    rh.check_condition(image, pic, winner, kw.get("show_txt", True))


def test_render_argument_checks_without_gpu():
    L = _C.lib()
    p = ctypes.c_void_p(256)                                             # never dereferenced: every call returns first
    assert L.cp_render_overlay_workspace_bytes(1024, 2048) == 4 * 1024 * 2048
    assert L.cp_render_overlay_workspace_bytes(37, 53) == 4 * 37 * 53

    def call(H=64, W=64, R=128, N=16, C=8, Lc=16, G=96, ws=1 << 20, alpha=102, r=1, t=2, **ptrs):
        a = dict(image=p, rows=p, n=p, src=p, poly=p, palette=p, codes=p, atlas=p, out=p, work=p)
        a.update(ptrs)
        prm = _C.OverlayParams(alpha, r, t, 0, 1, 1)
        params = None if ptrs.get("params", 1) is None else ctypes.byref(prm)
        return L.cp_render_overlay(a["image"], H, W, a["rows"], R, N, a["n"], a["src"], a["poly"], a["palette"], C,
                                   a["codes"], Lc, a["atlas"], G, params, a["out"], a["work"], ws, None)
    assert call(R=1025) == -2 and call(N=65) == -2 and call(C=33) == -2 and call(Lc=17) == -2 and call(G=129) == -2
    assert call(H=1 << 16, W=1 << 15, ws=1 << 40) == -2 and call(r=17) == -2
    assert call(N=2) == -1 and call(R=0) == -1 and call(C=0) == -1 and call(H=0) == -1 and call(W=-4) == -1
    assert call(alpha=-1) == -1 and call(alpha=257) == -1 and call(r=-1) == -1 and call(t=-1) == -1
    for name in ("image", "rows", "n", "src", "poly", "palette", "codes", "atlas", "out", "work", "params"):
        assert call(**{name: None}) == -1, name
    assert call(ws=64 * 64 * 4 - 1) == -3 and call(ws=0) == -3
    m = (ctypes.c_float * 3)(0, 0, 0)
    heat = lambda hm=p, C=8, h=8, w=8, ratio=4, inp=p, mean=m, std=m, pal=p, P=8, out=p: \
        L.cp_render_heatmap(hm, C, h, w, ratio, inp, mean, std, pal, P, 0, out, None)          # noqa: E731
    assert heat(hm=None) == -1 and heat(inp=None) == -1 and heat(mean=None) == -1 and heat(std=None) == -1
    assert heat(pal=None) == -1 and heat(out=None) == -1
    assert heat(h=0) == -1 and heat(w=0) == -1 and heat(ratio=0) == -1 and heat(P=0) == -1 and heat(C=-1) == -1
    assert heat(P=33) == -2 and heat(h=1 << 20, w=1 << 20) == -2


def test_debug_3_is_refused():
    """Before anything else, so without a device."""
    from centerpoly_amd.detectors.polydet import PolydetDetector
    from centerpoly_amd.opts import opts
    with pytest.raises(ValueError, match="matplotlib"):
        PolydetDetector(opts().init(["polydet", "--debug", "3"]))


# --------------------------------------------------------------------------------------------------- GPU --
def _device_overlay(image, rows, thresh, names, palette, white=False, show_txt=True, alpha=102, r=1, t=2,
                    outline=(0, 255, 255), show_polygons=True, alias=False):
    """cp_writer_instances + cp_render_overlay through the C ABI -> (picture, n)."""
    import torch
    dev = torch.device("cuda")
    L = _C.lib()
    H, W = image.shape[:2]
    C = len(names)
    R, N = rows.shape[0], (rows.shape[1] - 7) // 2
    d_rows = torch.from_numpy(np.ascontiguousarray(rows, np.float32)).to(dev)
    d_img = torch.from_numpy(image).to(dev)
    d_out = d_img if alias else torch.full_like(d_img, 77)
    n = torch.full((1,), -7, dtype=torch.int32, device=dev)
    src = torch.empty((R,), dtype=torch.int32, device=dev)
    label = torch.empty((R,), dtype=torch.int32, device=dev)
    poly = torch.empty((R, N, 2), dtype=torch.int32, device=dev)
    flags = torch.empty((R,), dtype=torch.uint8, device=dev)
    conf = torch.empty((R,), dtype=torch.float32, device=dev)
    table = np.ascontiguousarray(np.stack([np.arange(C), np.ones(C)], 1), np.int32)
    _C.check(L.cp_writer_instances(_C.ptr(d_rows), R, N, float(thresh), table.ctypes.data_as(ctypes.c_void_p), C,
                                   _C.ptr(n), _C.ptr(src), _C.ptr(poly), _C.ptr(flags), _C.ptr(label), _C.ptr(conf),
                                   _C.stream()), "cp_writer_instances")
    codes = np.full((R, 16), -1, np.int32)
    for k in range(R):
        c = int(rows[k, 5])
        if 0 <= c < C:
            text = rh.label(names[c], rows[k, 4])
            codes[k, :len(text)] = [ord(ch) - 32 if 32 <= ord(ch) <= 127 else 0 for ch in text]
    d_codes = torch.from_numpy(codes).to(dev)
    d_pal = torch.from_numpy(np.ascontiguousarray(palette, np.uint8)).to(dev)
    d_atlas = torch.from_numpy(dbg.glyph_atlas()).to(dev)
    prm = _C.OverlayParams(alpha, r, t, int(white), int(show_txt), int(show_polygons))
    prm.outline_colour[:] = outline
    nbytes = L.cp_render_overlay_workspace_bytes(H, W)
    # stale on purpose: the call clears it.  Taken from _C.workspace so that tests/test_memory_contract.py can hand it an
    # exact-size, guard-banded payload; such a payload already holds a uniform non-zero fill, which is kept -- anything
    # else (the allocator's own memory, or the zero fill) is replaced by 0xAB as before
    ws = _C.workspace(nbytes, dev)
    if int(ws[0]) == 0 or not bool((ws == ws[0]).all()):
        ws.fill_(0xAB)
    _C.check(L.cp_render_overlay(_C.ptr(d_img), H, W, _C.ptr(d_rows), R, N, _C.ptr(n), _C.ptr(src), _C.ptr(poly),
                                 _C.ptr(d_pal), C, _C.ptr(d_codes), 16, _C.ptr(d_atlas), 96, ctypes.byref(prm),
                                 _C.ptr(d_out), _C.ptr(ws), nbytes, _C.stream()), "cp_render_overlay")
    return d_out.cpu().numpy(), int(n.cpu()[0])


def _assert_same_picture(got, want, winner):
    bad = (got != want).any(axis=2)
    assert not bad.any(), "%d pixels differ, the first at (y, x) = %s where the statement shows operation %d" % (
        bad.sum(), tuple(np.argwhere(bad)[0]), winner[tuple(np.argwhere(bad)[0])])


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_overlay_equals_the_host_statement(name):
    rows, H, W, names, thresh, kw = _case(name)
    image, want, winner, hkw = _host_picture(name)
    rh.check_condition(image, want, winner, hkw.get("show_txt", True))
    got, n = _device_overlay(image, rows, thresh, names, _palette(len(names)), **kw)
    assert n == len(rh.instances(rows, thresh, len(names))) and n > 0
    if name == "n128":
        assert n == 128
    _assert_same_picture(got, want, winner)


@pytest.mark.gpu
def test_overlay_small_polygons_on_their_own_canvas():
    """The small16 set at 1024 x 2048 with the default parameters (too little of that canvas changes for the 1 %
    condition, which the same set meets in CASES on a smaller canvas): the comparison alone."""
    rows, image = _writer_rows("small16"), _image(1024, 2048, 77)
    want, winner = rh.overlay(image, rows, 0.02, NAMES11, _palette(11))
    assert (winner > 0).any()
    got, n = _device_overlay(image, rows, 0.02, NAMES11, _palette(11))
    assert n == len(rh.instances(rows, 0.02, 11)) > 0
    _assert_same_picture(got, want, winner)


@pytest.mark.gpu
@pytest.mark.parametrize("alpha,r,white,show_txt,alias", [(0, 0, False, True, False), (102, 1, True, False, True),
                                                          (256, 3, False, True, True), (102, 3, True, True, False),
                                                          (0, 1, True, False, False), (256, 0, False, False, True)])
def test_overlay_parameters(alpha, r, white, show_txt, alias):
    """Both themes, text on and off, a in {0, 102, 256}, r in {0, 1, 3}, in place and not, on the generated set."""
    H, W = 375, 1242
    rows = _generated_rows(W, H, 31 + alpha + r)
    image = _image(H, W, 5)
    kw = dict(white=white, show_txt=show_txt, alpha=alpha, r=r)
    want, winner = rh.overlay(image, rows, 0.3, NAMES8, _palette(8), **kw)
    rh.check_condition(image, want, winner, show_txt)
    got, n = _device_overlay(image, rows, 0.3, NAMES8, _palette(8), alias=alias, **kw)
    assert n == 11
    _assert_same_picture(got, want, winner)


@pytest.mark.gpu
def test_overlay_boxes_only_and_other_outline_colour():
    H, W = 37, 53
    rows, image = _generated_rows(W, H, 44), _image(H, W, 6)
    kw = dict(show_polygons=False, outline=(9, 8, 7), t=1)
    want, winner = rh.overlay(image, rows, 0.3, NAMES8, _palette(8), **kw)
    assert (winner == 3).any() and (winner == 5).any() and not (winner == 1).any() and not (winner == 2).any()
    got, _ = _device_overlay(image, rows, 0.3, NAMES8, _palette(8), **kw)
    _assert_same_picture(got, want, winner)
    kw = dict(outline=(9, 8, 7), t=3)
    want, winner = rh.overlay(image, rows, 0.3, NAMES8, _palette(8), **kw)
    got, _ = _device_overlay(image, rows, 0.3, NAMES8, _palette(8), **kw)
    _assert_same_picture(got, want, winner)


@pytest.mark.gpu
def test_overlay_nothing_live_and_too_many():
    import torch
    H, W = 375, 1242
    image = _image(H, W, 7)
    rows = _generated_rows(W, H, 3)
    for alias in (False, True):
        got, n = _device_overlay(image, rows, 2.0, NAMES8, _palette(8), alias=alias)          # n = 0
        assert n == 0 and np.array_equal(got, image)
    many = _many_rows(W, H, 160, 9)
    got, n = _device_overlay(image, many, 0.2, NAMES8, _palette(8))       # the ABI draws nothing and reports n
    assert n == 160 and np.array_equal(got, image)
    d = dbg.Debugger(NAMES8)
    d.add_img(image, "x")
    with pytest.raises(ValueError, match="more than 128 instances in one image"):
        d.add_polydet_detections(torch.from_numpy(many).cuda(), many, 0.2, img_id="x")
    assert rh.instances(many, 0.2, 8).__len__() == 160
    with pytest.raises(ValueError, match="more than 128 instances in one image"):
        rh.overlay(image, many, 0.2, NAMES8, _palette(8))


@pytest.mark.gpu
def test_debugger_draws_what_the_statement_draws(tmp_path):
    import torch
    from PIL import Image
    H, W = 375, 1242
    rows, image = _generated_rows(W, H, 17), _image(H, W, 8)
    for theme in ("white", "black"):
        d = dbg.Debugger(NAMES8, theme=theme)
        d.add_img(image, "polydet")
        d.add_polydet_detections(torch.from_numpy(rows).cuda(), rows, 0.3, img_id="polydet")
        want, winner = rh.overlay(image, rows, 0.3, NAMES8, _palette(8), white=theme == "white")
        assert d.last_n == 11 and d.imgs["polydet"].is_cuda and d.imgs["polydet"].dtype == torch.uint8
        _assert_same_picture(d.imgs["polydet"].cpu().numpy(), want, winner)
        files = d.show_all_imgs(path=str(tmp_path), prefix=theme + "_")
        assert files == [str(tmp_path / (theme + "_polydet.png"))]
        back = np.asarray(Image.open(files[0]).convert("RGB"))[:, :, ::-1]
        assert np.array_equal(back, want)


@pytest.mark.gpu
@pytest.mark.parametrize("C,white", [(8, False), (8, True), (3, False), (3, True), (11, True)])
def test_heatmap_equals_its_statement(C, white):
    import torch
    rng = np.random.RandomState(100 + C)
    h, w, ratio = 24, 40, 4
    hm = rng.uniform(0, 1, (C, h, w)).astype(np.float32)
    hm[:, :2] = 0
    hm[0, 3] = 1
    x = rng.normal(0, 2.5, (3, h * ratio, w * ratio)).astype(np.float32)         # some of it leaves 0 .. 255
    mean, std = np.array([0.284, 0.323, 0.282], np.float32), np.array([0.04, 0.05, 0.06], np.float32)
    d = dbg.Debugger(NAMES8, theme="white" if white else "black", down_ratio=ratio)
    got = d.add_blend_img(torch.from_numpy(x).cuda(), torch.from_numpy(hm).cuda(), mean, std, "hm").cpu().numpy()
    want = rh.heatmap(hm, x, mean, std, _palette(8), ratio, white)
    assert want.std() > 20 and np.array_equal(got, want)
    plain = d.add_blend_img(torch.from_numpy(x).cuda(), None, mean, std, "in").cpu().numpy()
    back = np.clip((x.transpose(1, 2, 0) * std + mean) * np.float32(255), 0, 255).astype(np.uint8)
    assert np.array_equal(plain, back)


def _demo_opt(tmp_path, extra=()):
    from centerpoly_amd.opts import opts
    return opts().parse(["polydet", "--arch", "smallhourglass", "--load_model", "", "--demo", str(tmp_path / "imgs"),
                         "--root_dir", str(tmp_path / "exp_root")] + list(extra))


def _results_rows(results):
    return _stack({j: np.asarray(r, np.float32) for j, r in results.items() if len(r)})


def _write_demo_images(tmp_path):
    from PIL import Image
    os.makedirs(str(tmp_path / "imgs"))
    images = {}
    for k, stem in enumerate(["frame_b", "frame_a"]):
        images[stem] = _image(512, 1024, 40 + k)
        Image.fromarray(images[stem][:, :, ::-1]).save(str(tmp_path / "imgs" / (stem + ".png")))
    return images


def _plain_runs(tmp_path, images):
    """The run without --debug, the images in demo.py's order, and a --vis_thresh just below the 30th score (ten
    of this network's small random polygons change less than 1 % of the picture)."""
    import torch
    from centerpoly_amd.datasets.dataset_factory import dataset_factory
    from centerpoly_amd.detectors.detector_factory import detector_factory
    from centerpoly_amd.opts import opts
    opt0 = opts().update_dataset_info_and_set_heads(_demo_opt(tmp_path), dataset_factory["cityscapes"])
    torch.manual_seed(1234)
    det0 = detector_factory["polydet"](opt0)
    plain = {stem: det0.run(str(tmp_path / "imgs" / (stem + ".png"))) for stem in sorted(images)}
    assert all(sorted(r) == ["dec", "load", "merge", "net", "post", "pre", "results", "tot"] for r in plain.values())
    assert det0.debugger is None
    score = min(np.sort(_results_rows(r["results"])[:, 4])[-30] for r in plain.values())
    return opt0, plain, float(np.nextafter(np.float32(score), np.float32(-1)))


def _run_demo(tmp_path, vis_thresh, level):
    import torch
    torch.manual_seed(1234)
    return _demo_module().demo(_demo_opt(tmp_path, ["--vis_thresh", repr(vis_thresh), "--debug", str(level)]))


def _debug_dir(tmp_path):
    return str(tmp_path / "exp_root" / "exp" / "cityscapes" / "polydet" / "default" / "debug")


@pytest.mark.gpu
def test_demo_end_to_end(tmp_path, capsys):
    """Two synthetic PNG files through demo.py with a random-init smallhourglass: at least 8 instances are drawn in
    each, and the written overlay (and ret['vis']) is the host statement applied to the returned results."""
    from PIL import Image
    from centerpoly_amd.detectors.base_detector import class_names
    images = _write_demo_images(tmp_path)
    opt0, _, vis_thresh = _plain_runs(tmp_path, images)
    capsys.readouterr()
    out = _run_demo(tmp_path, vis_thresh, 0)                             # demo.py forces --debug 1
    printed = capsys.readouterr().out
    assert [os.path.basename(n) for n, _ in out] == ["frame_a.png", "frame_b.png"]
    assert printed.count("tot ") == 2 and printed.count("|vis ") == 2 and "merge " in printed
    names = class_names(opt0)
    for path, ret in out:
        stem = os.path.basename(path)[:-4]
        rows = _results_rows(ret["results"])
        assert 8 <= len(rh.instances(rows, vis_thresh, 8)) <= 128
        want, winner = rh.overlay(images[stem], rows, vis_thresh, names, _palette(8), white=True)
        assert (winner == 3).any() and (winner == 4).any() and (winner == 5).any()   # boxes and labels show (a random
        assert (want != images[stem]).any()                              # network's polygons may hide under their outline)
        assert ret["vis"].is_cuda and np.array_equal(ret["vis"].cpu().numpy(), want)
        name = os.path.join(_debug_dir(tmp_path), stem + "_polydet.png")
        assert ret["vis_files"] == [name]
        _assert_same_picture(np.asarray(Image.open(name).convert("RGB"))[:, :, ::-1], want, winner)


@pytest.mark.gpu
def test_debug_2_views_equal_their_statements(tmp_path):
    """--debug 2: pred_hm_1.0 is the statement on the heat map and the network input of that very run (recorded as
    they are handed to debug()), out_pred_1.0 the centre boxes on the de-normalised input."""
    import torch
    from PIL import Image
    from centerpoly_amd.datasets.dataset_factory import dataset_factory
    from centerpoly_amd.detectors.base_detector import class_names
    from centerpoly_amd.detectors.detector_factory import detector_factory
    from centerpoly_amd.opts import opts
    images = _write_demo_images(tmp_path)
    opt = opts().update_dataset_info_and_set_heads(_demo_opt(tmp_path, ["--debug", "2"]), dataset_factory["cityscapes"])
    torch.manual_seed(1234)
    det = detector_factory["polydet"](opt)
    seen, real_debug = {}, det.debug

    def spy(debugger, net_in, dets, output, scale=1):
        seen["in"], seen["hm"] = net_in[0].cpu().numpy(), output["hm"][0].cpu().numpy()
        seen["dets"] = dets[0].cpu().numpy().copy()
        return real_debug(debugger, net_in, dets, output, scale)
    det.debug = spy
    names = class_names(opt)
    for stem in sorted(images):
        ret = det.run(str(tmp_path / "imgs" / (stem + ".png")))
        assert sorted(os.path.basename(f) for f in ret["vis_files"]) == sorted(
            stem + "_" + v + ".png" for v in ("polydet", "pred_hm_1.0", "out_pred_1.0"))
        read = lambda v: np.asarray(Image.open(os.path.join(_debug_dir(tmp_path), stem + "_" + v + ".png"))  # noqa: E731
                                    .convert("RGB"))[:, :, ::-1]
        want = rh.heatmap(seen["hm"], seen["in"], opt.mean, opt.std, _palette(8), opt.down_ratio, white=True)
        no_heat = rh.heatmap(np.zeros_like(seen["hm"]), seen["in"], opt.mean, opt.std, _palette(8), opt.down_ratio,
                             white=True)
        assert (want != no_heat).any(axis=2).mean() >= 0.01             # the heat map shows
        assert np.array_equal(read("pred_hm_1.0"), want)
        rows = seen["dets"]
        rows[:, :4] *= opt.down_ratio
        plain_in = np.clip((seen["in"].transpose(1, 2, 0) * np.asarray(opt.std, np.float32)
                            + np.asarray(opt.mean, np.float32)) * np.float32(255), 0, 255).astype(np.uint8)
        want_boxes, _ = rh.overlay(plain_in, rows, opt.center_thresh, names, _palette(8), white=True,
                                   show_polygons=False)
        assert np.array_equal(read("out_pred_1.0"), want_boxes)


@pytest.mark.gpu
def test_debug_leaves_results_alone_and_two_runs_write_the_same_files(tmp_path):
    """ret['results'] of the demo run is bit-equal to the same run with --debug 0, and two demo runs write identical
    files.  Both rest on run() giving the same detections for the same image every time, which BaseDetector.run
    secures by asking the vendor library for its reproducible convolution algorithms while it runs (the hourglass
    has convolutions too small for the project's own kernel); the pictures themselves are integer arithmetic."""
    images = _write_demo_images(tmp_path)
    _, plain, vis_thresh = _plain_runs(tmp_path, images)
    first = {}
    for path, ret in _run_demo(tmp_path, vis_thresh, 1):
        stem = os.path.basename(path)[:-4]
        for j in ret["results"]:
            assert np.asarray(ret["results"][j]).tobytes() == np.asarray(plain[stem]["results"][j]).tobytes()
        first[stem] = open(os.path.join(_debug_dir(tmp_path), stem + "_polydet.png"), "rb").read()
    for path, ret in _run_demo(tmp_path, vis_thresh, 1):
        stem = os.path.basename(path)[:-4]
        assert open(os.path.join(_debug_dir(tmp_path), stem + "_polydet.png"), "rb").read() == first[stem]

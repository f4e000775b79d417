"""Generator of tests/golden/mask_nms.npz, the fixture of tests/test_mask_nms.py (run it from the repository root:
`python tests/golden/gen_mask_nms_golden.py`).  It draws every polygon with PIL's own ImageDraw.polygon
(mask_nms_host.pil_fill) and records, per case, the rows (their vertices are columns 6 .. 6 + 2 N), the canvas, the
areas, the matrix of common pixels and -- for the merge cases -- the parameters and the table and counts the host
statement (mask_nms_host.mask_nms) gives.  The cases of 1024 rows record the packed masks instead of the 4 MiB
matrix; the test takes the matrix from them with one product.

Overlap cases `ov/<name>`: rows, canvas (H, W), C, area, inter | masks.  Merge cases `mg/<name>`: rows [S, K, ncols],
canvas, C, par (max_per_image, sigma, Nt, threshold, method), area, inter | masks, table, counts.

For method 2 the device's double exp may differ from math.exp in the last bit; so that this could never change an
order, every Gaussian case is generated (seed by seed until it holds) such that at every selection step of the host
statement the best two live scores differ by more than 1e-4 relative -- or are exactly equal and neither has decayed --
and no kept or stopping score lies within 1e-4 relative of the threshold or, unless equal to it and undecayed, of the
cut."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import mask_nms_host as host  # noqa: E402

REL = 1e-4


def make_rows(polys, classes, scores, N):
    """Rows [R, 2 N + 7]: a polygon of fewer than N vertices repeats its last one."""
    rows = np.zeros((len(polys), 2 * N + 7), np.float32)
    for i, (p, c, s) in enumerate(zip(polys, classes, scores)):
        p = [tuple(v) for v in p]
        assert 1 <= len(p) <= N
        p = p + [p[-1]] * (N - len(p))
        xy = np.array(p, np.float32)
        rows[i, 0:2] = xy.min(axis=0)
        rows[i, 2:4] = xy.max(axis=0)
        rows[i, 4] = s
        rows[i, 5] = c
        rows[i, 6:6 + 2 * N] = xy.reshape(-1)
        rows[i, -1] = 0.25 + i
    return rows


def tri_pair():
    return [[(0, 0), (40, 0), (0, 40)], [(41, 1), (41, 41), (1, 41)]]


def shapes(H, W):
    """The named shapes of the issue on an H x W canvas (at least 48 x 64), each of at most 8 vertices: (polygon, class)."""
    out = [(p, 0) for p in tri_pair()]
    out += [([(5, 5), (30, 8), (25, 30), (4, 22)], 0)] * 2                       # identical: ov = 1
    out += [([(2, 2), (60, 3), (58, 44), (3, 40)], 1), ([(20, 12), (40, 14), (36, 30), (22, 28)], 1)]    # nested
    out += [([(10, 10), (20, 10), (20, 20), (10, 20)], 2), ([(20, 20), (30, 20), (30, 30), (20, 30)], 2),
            ([(21, 10), (30, 10), (30, 19), (21, 19)], 2)]                       # boxes touch, corner and side
    out += [([(8, 8), (40, 36), (40, 8), (8, 36)], 0)]                           # a bow tie
    out += [([(12, 30), (12, 30), (30, 30), (30, 44), (30, 44), (12, 44)], 1)]   # repeated vertices
    out += [([(17, 23)], 1), ([(17, 23)] * 5, 0)]                                # all vertices at one point
    out += [([(10, 5), (50, 5), (40, 25), (20, 25)], 2), ([(22, 6), (38, 6), (50, 26), (10, 26)], 2)]   # flat top, flat bottom
    out += [([(3, 33), (55, 33), (30, 33)], 0), ([(3, 33), (55, 33), (30, 34)], 0),                     # one-pixel slivers
            ([(3, 32), (55, 33), (30, 33)], 0)]
    out += [([(10.994, 12.994), (40.996, 12.996), (40.9951, 30.9949), (10.99, 30.999)], 1),             # around .995
            ([(-0.994, -0.996), (20.5, -3.5), (18.25, 17.75), (-2.996, 15.994)], 1)]                    # negative ones
    out += [([(-10, 10), (12, 4), (9, 30)], 0), ([(W - 8, 20), (W + 15, 12), (W + 3, 40)], 0),           # partly off
            ([(20, -12), (44, -3), (30, 9)], 0), ([(25, H - 6), (50, H + 9), (12, H + 20)], 0),
            ([(-20, -20), (W + 20, -25), (W + 30, H + 20), (-15, H + 30)], 0)]                           # covers the canvas
    out += [([(-30, 5), (-5, 8), (-12, 30)], 0), ([(W, 5), (W + 20, 8), (W + 4, 30)], 0),                # wholly off
            ([(5, -30), (40, -4), (20, -1)], 0), ([(5, H), (40, H + 4), (20, H + 30)], 0)]
    out += [([(5, 5), (30, 8), (25, 30), (4, 22)], 1), ([(5, 5), (30, 8), (25, 30), (4, 22)], 2)]       # other classes
    out += [([(5, 5), (30, 8), (25, 30), (4, 22)], 2.5), ([(5, 5), (30, 8), (25, 30), (4, 22)], -1),
            ([(5, 5), (30, 8), (25, 30), (4, 22)], 3)]                           # no class: 2.5, -1, C itself
    return out


def triangles(H, W):
    out = [(p, 0) for p in tri_pair()]
    out += [([(5, 5), (30, 8), (12, 30)], 0)] * 2
    out += [([(2, 2), (60, 3), (30, 44)], 1), ([(25, 10), (36, 11), (30, 24)], 1)]
    out += [([(3, 33), (55, 33), (30, 33)], 0), ([(3, 33), (55, 33), (30, 34)], 0), ([(17, 23)], 1)]
    out += [([(10, 5), (50, 5), (30, 25)], 2), ([(30, 6), (50, 26), (10, 26)], 2)]
    out += [([(10.994, 12.994), (40.996, 12.996), (20.9951, 30.9949)], 1), ([(-0.994, -0.996), (20.5, -3.5), (-2.996, 15.994)], 1)]
    out += [([(-10, 10), (12, 4), (9, 30)], 0), ([(W - 8, 20), (W + 15, 12), (W + 3, 40)], 0), ([(20, -12), (44, -3), (30, 9)], 0),
            ([(25, H - 6), (50, H + 9), (12, H + 20)], 0), ([(-30, 5), (-5, 8), (-12, 30)], 0), ([(5, H), (40, H + 4), (20, H + 30)], 0)]
    out += [([(5, 5), (30, 8), (12, 30)], 1), ([(5, 5), (30, 8), (12, 30)], 2.5), ([(5, 5), (30, 8), (12, 30)], -1)]
    return out


def blob(rng, cx, cy, r, n, jitter=0.35, star=False):
    """n vertices around (cx, cy): radius r with a random relative jitter (a star alternates r and r / 2)."""
    a = np.sort(rng.uniform(0, 2 * np.pi, n)) if not star else np.arange(n) * 2 * np.pi / n
    rr = r * (1 + rng.uniform(-jitter, jitter, n))
    if star:
        rr = rr * np.where(np.arange(n) % 2 == 0, 1.0, 0.5)
    return [(float(np.float32(cx + q * np.cos(t))), float(np.float32(cy + q * np.sin(t)))) for t, q in zip(a, rr)]


def random_polys(seed, R, N, H, W, C, rmax=None, bad=True, rmin=0.6):
    """R polygons of up to N vertices scattered over and around the canvas, classes of [0, C) (some rows without one)."""
    rng = np.random.RandomState(seed)
    rmax = rmax or max(2.0, min(H, W) / 2.5)
    polys, classes = [], []
    for i in range(R):
        n = N if i % 3 else int(rng.randint(1, N + 1))
        cx, cy = rng.uniform(-0.15 * W, 1.15 * W), rng.uniform(-0.15 * H, 1.15 * H)
        p = blob(rng, cx, cy, rng.uniform(rmin, rmax), n, star=(i % 5 == 4))
        if i % 7 == 3:                                                           # integer vertices: flat edges, repeats
            p = [(float(round(x)), float(round(y))) for x, y in p]
        polys.append(p)
        classes.append(float(rng.randint(0, C)) if not (bad and i % 17 == 11) else (-1.0 if i % 2 else 1.5))
    return polys, classes


def check_inside_box(rows, m, H, W):
    """PIL's fill stays inside the clipped bounding box of the integer vertices (what the raster kernel writes)."""
    for row, mk in zip(rows, m):
        if not mk.any():
            continue
        p = np.array(host.polygon(row))
        ys, xs = np.nonzero(mk)
        assert xs.min() >= max(p[:, 0].min(), 0) and xs.max() <= min(p[:, 0].max(), W - 1), row
        assert ys.min() >= max(p[:, 1].min(), 0) and ys.max() <= min(p[:, 1].max(), H - 1), row


def measure(rows, C, H, W):
    flat = rows.reshape(-1, rows.shape[-1])
    m = host.masks(flat, C, H, W)
    check_inside_box(flat, m, H, W)
    area, inter = host.overlaps_from_masks(m, [host.class_of(r[5], C) for r in flat])
    return m, area, inter


def put(out, key, rows, C, H, W):
    m, area, inter = measure(rows, C, H, W)
    out[key + "/rows"] = rows
    out[key + "/canvas"] = np.array([H, W], np.int32)
    out[key + "/C"] = np.int32(C)
    out[key + "/area"] = area
    if rows.reshape(-1, rows.shape[-1]).shape[0] > 256:
        out[key + "/masks"] = np.packbits(m.reshape(len(m), -1), axis=1)
    else:
        out[key + "/inter"] = inter
    return area, inter


def overlap_cases(out):
    names = []

    def case(name, polys, classes, N, H, W, C=3):
        scores = np.linspace(0.9, 0.1, len(polys))
        put(out, "ov/" + name, make_rows(polys, classes, scores, N), C, H, W)
        names.append(name)

    for N in (8, 16, 64):
        ps, cs = zip(*shapes(48, 64))
        case("shapes_n%d" % N, ps, cs, N, 48, 64)
    ps, cs = zip(*triangles(48, 64))
    case("triangles_n3", ps, cs, 3, 48, 64)
    ps, cs = random_polys(11, 40, 64, 48, 64, 3)
    case("random_n64", ps, cs, 64, 48, 64)
    ps, cs = random_polys(12, 24, 3, 37, 53, 3)
    case("random_n3_37x53", ps, cs, 3, 37, 53)
    case("canvas_1x1", [[(0, 0), (0, 0), (0, 0)], [(-3, -2), (4, -1), (1, 5)], [(1, 0), (3, 0), (2, 2)], [(0, 0)], [(-2, -2), (3, -2), (0, 4)]],
         [0, 0, 0, 1, 1], 16, 1, 1)
    for W in (31, 32, 33, 64, 65):
        ps, cs = random_polys(20 + W, 32, 16, 20, W, 3, rmax=W / 2.0)
        ps = list(ps) + [[(W - 3, 2), (W - 1, 2), (W - 1, 17), (W - 3, 17)], [(0, 1), (W - 1, 1), (W - 1, 18), (0, 18)],
                         [(30, 0), (33, 0), (33, 19), (30, 19)], [(31, 3), (32, 3), (32, 9), (31, 9)], [(32, 4), (W + 5, 6), (32, 12)]]
        cs = list(cs) + [0, 0, 0, 0, 0]
        case("width_%d" % W, ps, cs, 16, 20, W)
    for R in (1, 63, 64, 65, 129):
        ps, cs = random_polys(100 + R, R, 16, 37, 53, 3)
        case("rows_%d" % R, ps, cs, 16, 37, 53)
    ps, cs = random_polys(7, 48, 16, 128, 256, 3, rmax=70.0)
    case("canvas_128x256", ps, cs, 16, 128, 256)
    big = [[(100.5, 80.25), (1900.75, 120.5), (1700.0, 900.996), (300.25, 1000.5)],
           [(1000, 10), (2047, 500), (1500, 1023), (600, 700)],
           [(-50, 500), (700, -40), (2100, 400), (900, 1100)],
           blob(np.random.RandomState(5), 1024, 512, 400, 16, star=True),
           [(2040, 1000), (2047, 1000), (2047, 1023), (2040, 1023)],
           [(100.5, 80.25), (1900.75, 120.5), (1700.0, 900.996), (300.25, 1000.5)]]
    case("canvas_1024x2048", big, [0, 0, 0, 0, 0, 1], 16, 1024, 2048)
    ps, cs = random_polys(1024, 1024, 16, 48, 64, 3, rmax=6.0)
    case("rows_1024", ps, cs, 16, 48, 64)
    out["ov/names"] = np.array(names)


def gaps_hold(trace, threshold):
    """The order of every selection step, and every comparison with the threshold, survives a last-bit difference."""
    for _, best, second, touched in trace:
        if second is not None and not (abs(float(best) - float(second)) > REL * abs(float(best)) or (best == second and not touched)):
            return False
        if not abs(float(best) - float(threshold)) > REL * float(threshold):
            return False
    return True


def cut_gap_holds(rows, C, area, inter, par):
    """No kept score within REL of the cut's threshold unless equal to it."""
    max_per_image, sigma, Nt, threshold, method = par
    table, _ = host.mask_nms(rows, C, area, inter, 1 << 30, sigma, Nt, threshold, int(method))
    s = table[:, 4]
    if len(s) <= max_per_image:
        return True
    kth = len(s) - int(max_per_image)
    t = np.partition(s, kth)[kth]
    return all(v == t or abs(float(v) - float(t)) > REL * abs(float(t)) for v in s)


def merge_rows(seed, S, K, H, W, C, quantise=0, one_class=False, rmax=22.0, rmin=6.0, small_class=True):
    rng = np.random.RandomState(seed)
    ps, cs = random_polys(seed, S * K, 16, H, W, C - 1 if small_class else C, rmax=rmax, bad=not one_class, rmin=rmin)
    cs = list(cs)
    if one_class:
        cs = [0.0] * len(cs)
    elif small_class:
        cs[len(cs) // 2] = float(C - 2)                                          # a class of one row; class C - 1 stays empty
        cs = [c if (c != C - 2 or i == len(cs) // 2) else 0.0 for i, c in enumerate(cs)]
    scores = rng.uniform(0.02, 1.0, S * K)
    if quantise:
        scores = np.round(scores * quantise) / quantise + 1.0 / (2 * quantise)
    rows = make_rows(ps, cs, scores, 16)
    return rows.reshape(S, K, rows.shape[1])


def merge_cases(out):
    names = []

    def case(name, par, **kw):
        par = np.array(par, np.float32)
        seed = kw.pop("seed")
        H, W, C = kw["H"], kw["W"], kw["C"]
        for attempt in range(400):
            rows = merge_rows(seed + 7919 * attempt, **kw)
            _, area, inter = measure(rows, C, H, W)
            trace = []
            table, counts = host.mask_nms(rows, C, area, inter, int(par[0]), par[1], par[2], par[3], int(par[4]), trace=trace)
            if int(par[4]) != 2 or (gaps_hold(trace, np.float32(par[3])) and cut_gap_holds(rows, C, area, inter, par)):
                break
        else:
            raise AssertionError("no seed gives case %s its score gaps" % name)
        put(out, "mg/" + name, rows, C, H, W)
        out["mg/%s/par" % name] = par
        out["mg/%s/table" % name] = table
        out["mg/%s/counts" % name] = counts
        names.append(name)
        print("%-12s seed +%d: %d rows in, %d out, counts %s, %d selection steps" % (
            name, attempt, rows.shape[0] * rows.shape[1], counts[0], counts[1:].tolist(), len(trace)))
        return rows, table, counts

    base = dict(H=48, W=64, C=4, K=24)
    for method in (0, 1, 2):
        for S in (1, 2, 3):
            case("m%d_s%d" % (method, S), (100, 0.5, 0.5, 0.001, method), seed=31 * method + S, S=S, **base)
    # equal scores: eight levels among 48 rows; the lowest position wins, and ties sit at the cut
    _, table, _ = case("ties", (100, 0.5, 0.5, 0.001, 2), seed=77, S=2, quantise=8, **base)
    _, table, counts = case("cut_ties", (12, 0.5, 0.5, 0.001, 0), seed=78, S=2, quantise=8, **base)
    assert counts[0] > 12                                                        # ties at the cut are kept
    _, table, counts = case("cut_one", (1, 0.5, 0.5, 0.001, 2), seed=79, S=2, **base)
    assert counts[0] == 1
    rows, table, counts = case("threshold", (100, 0.5, 0.5, 0.6, 2), seed=80, S=3, **base)
    assert counts[0] < rows.shape[0] * rows.shape[1] // 3                        # most rows are dropped
    # 1024 rows of one class.  Linear decay: its arithmetic is exact IEEE on both sides, while no set of 1024 scores keeps
    # the best two 1e-4 apart over a thousand Gaussian steps
    rows, table, counts = case("limit", (100, 0.5, 0.5, 0.001, 1), seed=81, S=4, K=256, H=48, W=64, C=1, one_class=True,
                               small_class=False, rmax=9.0, rmin=1.0)
    assert counts[0] >= 100
    out["mg/names"] = np.array(names)


def main():
    out = {}
    overlap_cases(out)
    merge_cases(out)
    # the motivating pair
    rows = make_rows(tri_pair(), [0, 0], [0.9, 0.8], 16)
    _, area, inter = measure(rows, 1, 48, 64)
    assert area.tolist() == [861, 861] and inter[0, 1] == 0, (area, inter)
    path = os.path.join(HERE, "mask_nms.npz")
    np.savez_compressed(path, **out)
    print("wrote %s: %d bytes, %d arrays" % (path, os.path.getsize(path), len(out)))


if __name__ == "__main__":
    main()

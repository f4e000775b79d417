"""PIL's two polygon primitives on the host: centerpoly_amd/csrc/class_masks_core.h quoted function by function, in
plain Python and numpy float32.  TEST INFRASTRUCTURE, the one host statement of the rule: tests/test_class_masks.py
holds it against the installed PIL (test_restatement_equals_the_installed_pil) and the kernels against it;
tests/golden/annotations_host.py builds its masks from it."""
import numpy as np

f32 = np.float32


def round_up(f):
    """cm_round_up: PIL's ROUND_UP, round half up."""
    f = f32(f)
    return int(np.floor(f + f32(0.5))) if f >= 0 else -int(np.floor(abs(f) + f32(0.5)))


def round_down(f):
    """cm_round_down: PIL's ROUND_DOWN, round half down."""
    f = f32(f)
    return int(np.ceil(f - f32(0.5))) if f >= 0 else -int(np.ceil(abs(f) - f32(0.5)))


def edges(pts):
    """cm_make_edge for every k: (kind, x0, y0, ymin, ymax, xmin, xmax, dx); kind 0 absent, 1 flat, 2 sloped."""
    N, out = len(pts), []
    for k in range(N):
        (x0, y0), (x1, y1) = pts[k], pts[(k + 1) % N]
        kind = 0 if (k + 1 == N and (x0, y0) == (x1, y1)) else 1 if y0 == y1 else 2
        dx = f32(x1 - x0) / f32(y1 - y0) if kind == 2 else f32(0)
        out.append((kind, x0, y0, min(y0, y1), max(y0, y1), min(x0, x1), max(x0, x1), dx))
    return out


def x_at(e, y):
    """cm_x_at: every step rounded to float32."""
    return f32(f32(y - e[2]) * e[7]) + f32(e[1])


def crossings(E, k, y, last_row):
    """cm_crossings: what edge k adds to row y."""
    e = E[k]
    if e[0] != 2 or y < e[3] or y > e[4]:
        return []
    x = x_at(e, y)
    if y == e[4] and y < last_row:
        return [x, x]
    if (y == e[3] or y == e[4]) and e[7] != 0:
        for j in range(k):
            o = E[j]
            if o[0] != 2 or o[7] == 0:
                continue
            if not ((y == e[3] and y == o[3]) or (y == e[4] and y == o[4])):
                continue
            if np.rint(x) != np.rint(x_at(o, y)):
                continue
            if (e[7] > 0) == (o[7] > 0):
                adj = y - 1 if y == last_row else y + 1
                a, b = x_at(e, adj), x_at(o, adj)
                if (y == e[4]) != (e[7] > 0):
                    x = max(f32(round_up(min(a, b)) - 1), x)
                else:
                    x = min(f32(round_up(max(a, b)) + 1), x)
            break
    return [x]


def fill(pts, W, H):
    """F: what ImageDraw.polygon(pts, fill=...) sets."""
    pts = [tuple(int(v) for v in p) for p in pts]
    m = np.zeros((H, W), bool)
    E = edges(pts)
    ys = [p[1] for p in pts]
    last_row = min(max(0, max(ys)), H)
    by_row = {}
    for k, e in enumerate(E):                                  # the edges that can touch a row, in table order
        if e[0] == 0:
            continue
        for y in range(max(e[3], 0), min(e[4], H - 1) + 1):
            by_row.setdefault(y, []).append(k)
    for y in range(max(0, min(ys)), min(H - 1, last_row) + 1):
        ks = by_row.get(y, [])
        xx = sorted(v for k in ks for v in crossings(E, k, y, last_row))
        spans = [(round_up(xx[i - 1]), round_down(xx[i])) for i in range(1, len(xx), 2)]
        spans += [(E[k][5], E[k][6]) for k in ks if E[k][0] == 1 and E[k][3] == y]
        for lo, hi in spans:
            lo, hi = max(lo, 0), min(hi, W - 1)
            if lo <= hi:
                m[y, lo:hi + 1] = True
    return m


def outline(pts, W, H):
    """O: what ImageDraw.polygon(pts, outline=...) sets (cm_line_steps / cm_line_pixel for every edge)."""
    pts = [tuple(int(v) for v in p) for p in pts]
    m = np.zeros((H, W), bool)
    for k in range(len(pts)):
        (x0, y0), (x1, y1) = pts[k], pts[(k + 1) % len(pts)]
        ax, ay = abs(x1 - x0), abs(y1 - y0)
        if ax == 0 and ay == 0:
            continue
        sx, sy = (1 if x1 >= x0 else -1), (1 if y1 >= y0 else -1)
        t = np.arange(max(ax, ay) + 1, dtype=np.int64)
        if ax > ay:
            px, py = x0 + sx * t, y0 + sy * ((2 * ay * t + ax) // (2 * ax))
        else:
            px, py = x0 + sx * ((2 * ax * t + ay) // (2 * ay)), y0 + sy * t
        ok = (px >= 0) & (px < W) & (py >= 0) & (py < H)
        m[py[ok], px[ok]] = True
    return m

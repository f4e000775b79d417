"""The inputs of tests/test_boundary.py: small images at which cp_boundary_overlaps can go wrong.  A case is a dict
    name, d, masks uint8 [n, H, W], ids uint16 [H, W], inst_ids list, bounds int32 [n, 4] or None, offset (the mask
    planes start one byte off a 16-byte boundary)
The kernel's tiles: a workgroup of the row pass owns 64 words = 2048 pixels of a line, a thread of the column pass a
strip of 32 rows (64 from d = 17 on, 8 for the id image) and 32 columns."""
import ctypes

import numpy as np

RANDOM_SEEDS = (11, 12, 13, 14, 15, 16)                  # test_boundary_cpu.py checks that none of them is vacuous


def _case(name, d, masks, ids, inst_ids, bounds=None, offset=False):
    masks = np.ascontiguousarray(masks, np.uint8).reshape((-1,) + ids.shape)
    return {"name": name, "d": int(d), "masks": masks, "ids": np.ascontiguousarray(ids, np.uint16),
            "inst_ids": [int(v) for v in inst_ids], "offset": offset,
            "bounds": None if bounds is None else np.ascontiguousarray(bounds, np.int32).reshape(len(masks), 4)}


def random_scene(seed, H, W, n, values=6):
    """(masks, ids, inst_ids): rectangles of instance values on a background of stuff, a group region below 1000,
    masks that are those rectangles shifted and resized by a few pixels (so bands and their intersections exist),
    with holes punched into some."""
    rng = np.random.RandomState(seed)
    ids = np.full((H, W), 7, np.uint16)
    ids[:, W // 2:] = 8                                                   # two stuff regions delimit each other
    boxes = []
    for k in range(values):
        h, w = rng.randint(max(2, H // 6), max(3, H // 2 + 1)), rng.randint(max(2, W // 6), max(3, W // 2 + 1))
        y, x = rng.randint(0, max(1, H - h + 1)), rng.randint(0, max(1, W - w + 1))
        v = 26 if k == 0 else 26000 + k                                   # k == 0: a group id below 1000
        ids[y:y + h, x:x + w] = v
        boxes.append((y, x, h, w))
    masks = np.zeros((n, H, W), np.uint8)
    for i in range(n):
        y, x, h, w = boxes[i % len(boxes)]
        dy, dx, gh, gw = rng.randint(-2, 3, 4)
        y0, x0 = max(0, y + dy), max(0, x + dx)
        masks[i, y0:max(y0 + 1, y + h + gh), x0:max(x0 + 1, x + w + gw)] = rng.choice([1, 255, 128])
        if i % 3 == 1 and h > 2 and w > 2:
            masks[i, y0 + h // 2, x0 + w // 2] = 0                        # a hole
    present = [int(v) for v in np.unique(ids) if v >= 26]
    return masks, ids, present[::-1]                                      # (not ascending: columns are by position)


def shaped_scene(H, W, d):
    """Hand-made masks on an H x W image: every edge and corner touched, the full plane, a 1-pixel hole, strips of
    width 2d (all band) and 2d + 1 (an interior line), both ways; ids: two instances sharing a border, a group id,
    values that are not of interest."""
    ids = np.zeros((H, W), np.uint16)
    ids[:, : W // 3] = 26001
    ids[:, W // 3: 2 * W // 3] = 26002                                    # shares a border with 26001
    ids[: H // 2, 2 * W // 3:] = 26                                       # a group
    ids[H // 2:, 2 * W // 3:] = 11                                        # stuff, not of interest
    ids[H // 3: H // 3 + 2, :] = 24005                                    # a thin instance across everything
    m = []
    full = np.full((H, W), 255, np.uint8)
    m.append(full)
    hole = full.copy()
    hole[H // 2, W // 2] = 0
    m.append(hole)
    for rows in (True, False):
        for width in (2 * d, 2 * d + 1):
            s = np.zeros((H, W), np.uint8)
            if rows:
                s[1:1 + width, :] = 1
            else:
                s[:, 1:1 + width] = 1
            m.append(s)
    corners = np.zeros((H, W), np.uint8)
    k = max(1, min(H, W) // 3)
    corners[:k, :k] = corners[:k, -k:] = corners[-k:, :k] = corners[-k:, -k:] = 200
    m.append(corners)
    edges = np.zeros((H, W), np.uint8)
    edges[0, :] = edges[-1, :] = edges[:, 0] = edges[:, -1] = 3
    m.append(edges)
    return np.stack(m), ids, [26002, 26001, 26, 24005, 70000, -1, 999]    # 70000, -1: outside 16 bits; 999: absent


def seam_scene(H, W):
    """One object whose band crosses every tile seam of the image: a frame-shaped mask from border to border with a
    diagonal cut, against an instance of nearly the same shape."""
    ids = np.full((H, W), 7, np.uint16)
    ids[3:H - 3, 4:W - 5] = 26001
    ids[H // 2 - 1:H // 2 + 2, :] = 26002                                 # a horizontal bar through every column tile
    mask = np.zeros((H, W), np.uint8)
    mask[2:H - 4, 3:W - 3] = 255
    yy, xx = np.mgrid[0:H, 0:W]
    mask[(xx * H // W) == yy] = 0                                         # a diagonal 1-pixel cut through every tile
    return mask[None], ids, [26001, 26002, 7]


def bounds_scene(H, W):
    """The same rectangle four times: bounds equal to it, looser, tighter, inverted."""
    ids = np.full((H, W), 26001, np.uint16)
    ids[:, W // 2:] = 26002
    y0, y1, x0, x1 = H // 4, 3 * H // 4, W // 5, 4 * W // 5
    m = np.zeros((4, H, W), np.uint8)
    m[:, y0:y1 + 1, x0:x1 + 1] = 255
    b = [[x0, y0, x1, y1], [x0 - 5, -3, W + 7, y1 + 2], [x0 + 3, y0 + 2, x1 - 4, y1 - 1], [x1, y0, x0, y1]]
    return m, ids, [26001, 26002], b


def checkerboard(H, W, G):
    """Every pixel its own id: everything is band; G of the ids are of interest."""
    ids = (np.arange(H * W, dtype=np.int64).reshape(H, W) * 7 % 60013 + 1000).astype(np.uint16)
    assert len(np.unique(ids)) == H * W
    m = np.zeros((2, H, W), np.uint8)
    m[0, 1:H - 1, 2:W - 3] = 1
    m[1, ::2, ::3] = 9
    return m, ids, ids.reshape(-1)[:G][::-1].tolist()


def all_cases():
    out = []
    out.append(_case("1x1", 1, np.full((1, 1, 1), 255), np.full((1, 1), 26001), [26001]))
    m, ids, inst = random_scene(11, 9, 13, 3)
    out.append(_case("9x13_d16_all_band", 16, m, ids, inst))
    for seed, d in zip((12, 13, 14, 15), (1, 2, 5, 11)):
        m, ids, inst = random_scene(seed, 37, 53, 3)
        out.append(_case("37x53_d%d" % d, d, m, ids, inst, offset=(d == 5)))
    for W in (255, 256, 257):
        m, ids, inst = random_scene(16, 40, W, 3)
        out.append(_case("40x%d_d5" % W, 5, m, ids, inst))
    for W in (15, 16, 17):
        m, ids, inst = shaped_scene(20, W, 2)
        out.append(_case("20x%d_shapes_d2" % W, 2, m, ids, inst))
    m, ids, inst = shaped_scene(70, 75, 11)
    out.append(_case("70x75_shapes_d11", 11, m, ids, inst))
    m, ids, inst = shaped_scene(140, 150, 64)
    out.append(_case("140x150_shapes_d64", 64, m[:5], ids, inst))
    m, ids, inst = seam_scene(129, 4097)                                  # two tiles plus a pixel each way
    out.append(_case("129x4097_seams_d11", 11, m, ids, inst))
    m, ids, inst = seam_scene(200, 70)                                    # four strips, d as large as a strip
    out.append(_case("200x70_seams_d64", 64, m, ids, inst))
    m, ids, inst, b = bounds_scene(45, 83)
    for d in (2, 11):
        out.append(_case("45x83_bounds_d%d" % d, d, m, ids, inst, bounds=b))
    m, ids, inst = random_scene(12, 24, 40, 128)
    out.append(_case("24x40_n128_d2", 2, m, ids, inst))
    out.append(_case("24x40_n0_d2", 2, m[:0], ids, inst))
    out.append(_case("24x40_G0_d2", 2, m[:3], ids, []))
    m, ids, inst = checkerboard(32, 40, 1024)
    out.append(_case("32x40_G1024_d1", 1, m, ids, inst))
    return out


def refusals():
    """Every limit and every null pointer of cp_boundary_overlaps; no pointer is dereferenced: each call returns first."""
    from centerpoly_amd import _C
    L = _C.lib()
    p = ctypes.c_void_p(256)
    big = 1 << 40

    def call(n=3, G=5, H=10, W=12, d=2, masks=p, bounds=None, ids=p, inst=p, bi=p, bp=p, bg=p, ws=p, ws_bytes=big):
        return L.cp_boundary_overlaps(masks, n, bounds, ids, H, W, d, inst, G, bi, bp, bg, None, None, ws, ws_bytes, None)
    count = 0
    for kw in (dict(n=129), dict(G=1025), dict(d=65), dict(H=1 << 16, W=1 << 15), dict(H=46341, W=46341)):
        assert call(**kw) == -2, kw
        count += 1
    for kw in (dict(n=-1), dict(G=-1), dict(H=0), dict(W=0), dict(H=-4), dict(d=0), dict(d=-3), dict(masks=None),
               dict(ids=None), dict(inst=None), dict(bi=None), dict(bp=None), dict(bg=None)):
        assert call(**kw) == -1, kw
        count += 1
    need = L.cp_boundary_overlaps_workspace_bytes(3, 5, 10, 12, 2)
    assert need >= 65536 * 2 + (3 + 2 * 3) * 10 * 1 * 4
    assert call(ws=None) == -3 and call(ws_bytes=need - 1) == -3 and call(ws_bytes=0) == -3
    # what a call does not need may be null: no masks without n, no ids of interest without G (workspace checked last)
    assert call(n=0, masks=None, bp=None, bi=None, ws_bytes=0) == -3
    assert call(G=0, inst=None, bg=None, bi=None, ws_bytes=0) == -3
    return count + 5

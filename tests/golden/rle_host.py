"""The host statement of "run-length masks" (include/centerpoly_hip.h): the literal loops of the definition, one pixel,
one count and one character at a time, and nothing cleverer.  The tests compare the device and the package's
vectorised host code with these."""
import numpy as np


def encode(mask):
    """Counts (list of int) of mask [H][W], a pixel set when non-zero, read in column-major order."""
    H, W = len(mask), len(mask[0])
    cnts, prev, run = [], 0, 0
    for x in range(W):
        for y in range(H):
            v = 1 if mask[y][x] else 0
            if v != prev:
                cnts.append(run)
                run, prev = 0, v
            run += 1
    cnts.append(run)
    return cnts


def to_string(cnts):
    out = []
    for i in range(len(cnts)):
        x = int(cnts[i])
        if i > 2:
            x -= int(cnts[i - 2])
        more = True
        while more:
            c = x & 0x1f
            x >>= 5                                                       # (Python's >> is arithmetic)
            more = (x != -1) if (c & 0x10) else (x != 0)
            if more:
                c |= 0x20
            out.append(chr(c + 48))
    return "".join(out)


def from_string(s):
    cnts, p = [], 0
    while p < len(s):
        x, k, more = 0, 0, True
        while more:
            c = ord(s[p]) - 48
            x |= (c & 0x1f) << (5 * k)
            more = bool(c & 0x20)
            p += 1
            k += 1
            if not more and (c & 0x10):
                x |= -1 << (5 * k)
        if len(cnts) > 2:
            x += cnts[len(cnts) - 2]
        cnts.append(x)
    return cnts


def decode(cnts, H, W, value=255):
    """(mask uint8 [H, W], status): status 1 and a zero mask when the counts do not add up to H * W or pass it."""
    flat, j, v = [0] * (H * W), 0, 0
    for c in cnts:
        if j + c > H * W:
            return np.zeros((H, W), np.uint8), 1
        for _ in range(c):
            flat[j] = value if v else 0
            j += 1
        v = 1 - v
    if j != H * W:
        return np.zeros((H, W), np.uint8), 1
    return np.array(flat, np.uint8).reshape(W, H).T.copy(), 0


def area(cnts):
    return sum(cnts[1::2])


def to_bbox(cnts, H, W):
    """[x, y, w, h] of the set pixels, zeros for an empty mask."""
    m, _ = decode(cnts, H, W, 1)
    ys, xs = np.nonzero(m)
    if len(xs) == 0:
        return [0, 0, 0, 0]
    return [int(xs.min()), int(ys.min()), int(xs.max() - xs.min() + 1), int(ys.max() - ys.min() + 1)]

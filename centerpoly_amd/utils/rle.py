"""COCO run-length masks ("run-length masks" in include/centerpoly_hip.h): `{"size": [H, W], "counts": "<string>"}`.

`encode` turns device masks -- planes, or the slots of an index image -- into strings on the device (cp_rle_encode) and
reads them back in one copy; `decode` parses strings on the host (`parse_counts`, vectorised numpy) and paints the
planes on the device (cp_rle_decode).  `area` and `to_bbox` work on the counts alone.  There is no host fallback for
encode / decode.  The format is restated from the published algorithm (tests/golden/rle_host.py is its literal
statement); it has not been checked against pycocotools itself, which is not part of this project."""
import ctypes

import numpy as np
import torch

from .. import _C

MAX_PLANES, MAX_INDEX, MAX_DECODE = 128, 255, 255
FIXED_COUNTS = 1 << 18                                  # first capacity without host bounds: counts, and bytes below
RUNS_PER_COLUMN = 4                                     # first capacity with host bounds: counts per box column
BYTES_PER_COUNT = 2


def _first_capacity(n, bounds_host):
    if bounds_host is None:
        return FIXED_COUNTS, BYTES_PER_COUNT * FIXED_COUNTS
    b = np.asarray(bounds_host, dtype=np.int64).reshape(-1, 4)
    cols = np.maximum(b[:, 2] - b[:, 0] + 2, 0)
    cap = int(RUNS_PER_COLUMN * cols.sum()) + 2 * n
    return cap, BYTES_PER_COUNT * cap


def encode(masks=None, index=None, n=None, bounds=None, want_counts=False):
    """RLE of device masks.  masks uint8 [n, H, W] (non-zero = set, n <= 128), or index uint8 [H, W] with n (mask k is
    index == k, n <= 255).  bounds int32 [n, 4] inclusive x0, y0, x1, y1 (a host array or a device tensor; W, H, -1,
    -1 = empty): a promise that mask k is zero outside its box.  Returns a list of n dictionaries {"size": [H, W],
    "counts": str, "area": int}, with "cnts" (numpy uint32) on request.  One copy comes back; a second call follows
    when the first capacities were too small."""
    if (masks is None) == (index is None):
        raise ValueError("encode takes exactly one of masks and index")
    src = masks if masks is not None else index
    if src.dtype != torch.uint8 or src.dim() != (3 if masks is not None else 2):
        raise ValueError("masks must be uint8 [n, H, W] and index uint8 [H, W], got %s %s" % (src.dtype, tuple(src.shape)))
    if masks is not None:
        n = int(masks.shape[0])
    elif n is None:
        raise ValueError("encode(index=...) needs n, the number of slots")
    n = int(n)
    if n == 0:
        return []
    limit = MAX_PLANES if masks is not None else MAX_INDEX
    if not 0 < n <= limit:
        raise ValueError("encode takes 1 .. %d masks per call in this mode, got %d" % (limit, n))
    H, W = int(src.shape[-2]), int(src.shape[-1])
    dev = src.device
    src = src.contiguous()
    bounds_host = None
    if bounds is not None and not torch.is_tensor(bounds):
        bounds_host = np.ascontiguousarray(bounds, dtype=np.int32).reshape(n, 4)
        bounds = torch.from_numpy(bounds_host).to(dev)
    if bounds is not None:
        if bounds.dtype != torch.int32 or tuple(bounds.shape) != (n, 4):
            raise ValueError("bounds must be int32 [n, 4], got %s %s" % (bounds.dtype, tuple(bounds.shape)))
        bounds = bounds.contiguous()
    L = _C.lib()
    cap_counts, cap_bytes = _first_capacity(n, bounds_host)
    if not want_counts:
        cap_counts = 0
    nbytes = L.cp_rle_encode_workspace_bytes(n, H, W, cap_counts)
    ws = _C.workspace(nbytes, dev)
    for attempt in range(2):
        o_table, o_counts = 16, 16 + 16 * n
        o_chars = o_counts + 4 * cap_counts
        out = torch.empty((o_chars + cap_bytes + 16,), dtype=torch.uint8, device=dev)
        at = lambda o: ctypes.c_void_p(out.data_ptr() + o)                # noqa: E731
        _C.check(L.cp_rle_encode(_C.ptr(src) if masks is not None else None, _C.ptr(src) if masks is None else None,
                                 n, H, W, _C.ptr(bounds), at(o_counts) if want_counts else None, cap_counts,
                                 at(o_chars), cap_bytes, at(o_table), at(0), _C.ptr(ws), nbytes, _C.stream()),
                 "cp_rle_encode")
        host = out.cpu().numpy()                                          # the one copy
        head = host[:16].view(np.int32)
        if not head[2]:
            break
        if attempt:
            raise _C.NativeError("cp_rle_encode reports an overflow at the capacities its own head asked for")
        cap_counts, cap_bytes = (int(head[0]) if want_counts else 0), int(head[1])
    table = host[o_table:o_counts].view(np.int32).reshape(n, 4)
    cnts = host[o_counts:o_chars].view(np.uint32)
    chars = host[o_chars:o_chars + cap_bytes].tobytes()
    res, first = [], 0
    for k in range(n):
        m, a, off, length = (int(v) for v in table[k])
        r = {"size": [H, W], "counts": chars[off:off + length].decode("ascii"), "area": a}
        if want_counts:
            r["cnts"] = cnts[first:first + m].copy()
        first += m
        res.append(r)
    return res


def parse_counts(counts, hw=None, what="counts"):
    """The counts (numpy int64) of a compressed string (str or bytes).  Raises ValueError naming `what` for a character
    outside 48..111, a number longer than 7 characters, a truncated number and, with hw = H * W, a count below 0 or
    above hw."""
    raw = counts.encode("latin-1", "replace") if isinstance(counts, str) else bytes(counts)
    b = np.frombuffer(raw, dtype=np.uint8).astype(np.int64)
    if b.size == 0:
        return np.zeros((0,), np.int64)
    if b.min() < 48 or b.max() > 111:
        raise ValueError("%s: a character outside the RLE alphabet (codes 48..111)" % what)
    c = b - 48
    last = (c & 0x20) == 0                                                # the number's closing character
    if not last[-1]:
        raise ValueError("%s: the last number is truncated" % what)
    pos = np.arange(b.size)
    starts = np.concatenate([[0], pos[last][:-1] + 1])                    # first character of every number
    number = np.cumsum(last) - last                                       # the number a character belongs to
    k = pos - starts[number]
    if k.max() > 6:
        raise ValueError("%s: a number longer than 7 characters" % what)
    x = np.add.reduceat((c & 0x1f) << (5 * k), starts)
    ends = pos[last]
    neg = (c[ends] & 0x10) != 0
    x = x - np.where(neg, np.int64(1) << (5 * (k[ends] + 1)), 0)
    cnts = x.copy()
    cnts[1::2] = np.cumsum(x[1::2])                                       # cnts[i] = x[i] + cnts[i - 2] for i > 2:
    cnts[2::2] = np.cumsum(x[2::2])                                       # two running sums; cnts[0] stands alone
    if hw is not None and (cnts.min() < 0 or cnts.max() > hw):
        raise ValueError("%s: a count below 0 or above H * W = %d" % (what, hw))
    return cnts


def _counts_of(rle, i, check=True, names=None):
    """(H, W, counts as numpy int64) of entry i of a list of RLE dictionaries; `names` are the entries' names in errors."""
    what = names[i] if names is not None else "rle %d" % i
    try:
        H, W = (int(v) for v in rle["size"])
        counts = rle["counts"]
    except (KeyError, TypeError, ValueError):
        raise ValueError("%s: not an RLE dictionary with size [H, W] and counts" % what)
    if H < 1 or W < 1:
        raise ValueError("%s: size %r" % (what, rle["size"]))
    if isinstance(counts, (str, bytes, bytearray)):
        return H, W, parse_counts(counts, H * W if check else None, what)
    cnts = np.asarray(counts, dtype=np.int64).reshape(-1)
    if check and cnts.size and (cnts.min() < 0 or cnts.max() > H * W):
        raise ValueError("%s: a count below 0 or above H * W = %d" % (what, H * W))
    return H, W, cnts


def decode(rles, device, value=255, names=None):
    """Planes of a list of RLE dictionaries of one size, `counts` a compressed string, bytes or an uncompressed list:
    (device uint8 [n, H, W] with `value` where set, status numpy int32 [n]: 1 and a zero plane where the counts do not
    add up to H * W).  A malformed string raises ValueError naming the entry ("rle <i>", or names[i])."""
    rles = list(rles)
    if not rles:
        raise ValueError("decode needs at least one RLE")
    parsed = [_counts_of(r, i, names=names) for i, r in enumerate(rles)]
    H, W = parsed[0][0], parsed[0][1]
    for i, p in enumerate(parsed):
        if (p[0], p[1]) != (H, W):
            raise ValueError("%s: size [%d, %d] differs from the first entry's [%d, %d]"
                             % (names[i] if names is not None else "rle %d" % i, p[0], p[1], H, W))
    dev = torch.device(device)
    n = len(parsed)
    planes = torch.empty((n, H, W), dtype=torch.uint8, device=dev)
    status = torch.empty((n,), dtype=torch.int32, device=dev)
    L = _C.lib()
    for k0 in range(0, n, MAX_DECODE):
        part = parsed[k0:k0 + MAX_DECODE]
        m = np.array([p[2].size for p in part], dtype=np.int64)
        total = int(m.sum())
        table = np.ascontiguousarray(np.stack([np.cumsum(m) - m, m], 1).astype(np.int32))
        flat = np.concatenate([p[2] for p in part]).astype(np.uint32) if total else np.zeros((1,), np.uint32)
        counts = torch.from_numpy(flat).to(dev)
        nbytes = L.cp_rle_decode_workspace_bytes(len(part), total)
        ws = _C.workspace(nbytes, dev)
        _C.check(L.cp_rle_decode(_C.ptr(counts), table.ctypes.data_as(ctypes.c_void_p), len(part), H, W, int(value),
                                 ctypes.c_void_p(planes[k0].data_ptr()), ctypes.c_void_p(status[k0:].data_ptr()),
                                 _C.ptr(ws), nbytes, _C.stream()), "cp_rle_decode")
    return planes, status.cpu().numpy()


def area(rles):
    """Set pixels of every RLE, from the counts (host)."""
    return [int(_counts_of(r, i)[2][1::2].sum()) for i, r in enumerate(rles)]


def to_bbox(rles):
    """[x, y, w, h] of the set pixels of every RLE, zeros for an empty mask, from the counts (host)."""
    out = []
    for i, r in enumerate(rles):
        H, W, cnts = _counts_of(r, i)
        end = np.cumsum(cnts)
        s, e = (end - cnts)[1::2], end[1::2]                              # the runs of ones, [s, e)
        keep = e > s
        s, e = s[keep], e[keep] - 1
        if s.size == 0:
            out.append([0, 0, 0, 0])
            continue
        xs, xe, ys, ye = s // H, e // H, s % H, e % H
        wraps = xe > xs                                                   # the run holds (H - 1, xs) and (0, xs + 1)
        y0 = 0 if wraps.any() else int(ys.min())
        y1 = H - 1 if wraps.any() else int(ye.max())
        x0, x1 = int(xs.min()), int(xe.max())
        out.append([x0, y0, x1 - x0 + 1, y1 - y0 + 1])
    return out

"""The host statement of "device PNG stream" (include/centerpoly_hip.h): the literal loops of the definition, one byte,
one token and one code at a time, and nothing cleverer.  The tests compare the device with these.  `tokens_fast` is the
same run search with numpy, for images too large for the loops; the tests hold it against `tokens`."""
import struct
import zlib

import numpy as np

SIGNATURE = b"\x89PNG\r\n\x1a\n"
LENGTH_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195,
               227, 258]
LENGTH_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]


def filtered(image, bits):
    """S of an image [H][W] of integers in [0, 2^bits): rows of a filter byte 0 and the pixel bytes, big-endian."""
    out = bytearray()
    for row in image:
        out.append(0)
        for v in row:
            v = int(v)
            if not 0 <= v < 1 << bits:
                raise ValueError("the value %d does not fit a %d-bit image" % (v, bits))
            if bits == 16:
                out.append(v >> 8)
            out.append(v & 0xff)
    return bytes(out)


def tokens(S, D):
    """The greedy tokens of S: ("lit", byte) and ("match", length), distance D."""
    out, i, n = [], 0, len(S)
    while i < n:
        r = 0
        while r < 258 and i + r < n and i + r >= D and S[i + r] == S[i + r - D]:
            r += 1
        if r >= 3:
            out.append(("match", r))
            i += r
        else:
            out.append(("lit", S[i]))
            i += 1
    return out


def tokens_fast(S, D):
    """`tokens` through the intervals of equal bytes (numpy): chunks of 258, a remainder of 3 or more as one match, a
    shorter one as literals."""
    s = np.frombuffer(bytes(S), dtype=np.uint8)
    n = s.size
    eq = np.zeros(n + 1, dtype=bool)                                      # (one beyond the end closes the last interval)
    eq[D:n] = s[D:] == s[:n - D]
    edge = np.flatnonzero(eq[1:] != eq[:-1]) + 1
    if eq[0]:
        edge = np.concatenate([[0], edge])
    starts, ends = edge[0::2], edge[1::2]
    is_lit = ~eq[:n]
    pos, length = [np.flatnonzero(is_lit)], [np.zeros(int(is_lit.sum()), np.int64)]
    for a, b in zip(starts.tolist(), ends.tolist()):
        full, rest = divmod(b - a, 258)
        if full:
            pos.append(a + 258 * np.arange(full)); length.append(np.full(full, 258, np.int64))
        at = a + 258 * full
        if rest >= 3:
            pos.append(np.array([at])); length.append(np.array([rest], np.int64))
        elif rest:
            pos.append(at + np.arange(rest)); length.append(np.zeros(rest, np.int64))
    pos, length = np.concatenate(pos), np.concatenate(length)
    order = np.argsort(pos, kind="stable")
    return [("match", int(m)) if m else ("lit", int(s[p])) for p, m in zip(pos[order].tolist(), length[order].tolist())]


class _Bits(object):
    """Bits packed LSB first."""

    def __init__(self):
        self.out, self.acc, self.n, self.total = bytearray(), 0, 0, 0

    def put(self, value, nbits):                                          # `value` as it is, its bit 0 first
        self.acc |= value << self.n
        self.n += nbits
        self.total += nbits
        while self.n >= 8:
            self.out.append(self.acc & 0xff)
            self.acc >>= 8
            self.n -= 8

    def put_code(self, code, nbits):                                      # a Huffman code, its highest bit first
        for k in range(nbits - 1, -1, -1):
            self.put((code >> k) & 1, 1)

    def put_symbol(self, sym):
        if sym <= 143:
            self.put_code(0x30 + sym, 8)
        elif sym <= 255:
            self.put_code(0x190 + sym - 144, 9)
        elif sym <= 279:
            self.put_code(sym - 256, 7)
        else:
            self.put_code(0xC0 + sym - 280, 8)

    def done(self):
        if self.n:
            self.out.append(self.acc & 0xff)
        return bytes(self.out)


def adler32(S):
    s1, s2 = 1, 0
    for b in S:
        s1 = (s1 + b) % 65521
        s2 = (s2 + s1) % 65521
    return (s2 << 16) | s1


def deflate(toks, D, want_bits=False):
    """One fixed-Huffman block of the tokens, end-of-block and the padding (want_bits: its bits before the padding)."""
    w = _Bits()
    w.put(1, 1)                                                           # BFINAL
    w.put(1, 2)                                                           # BTYPE = 01
    for kind, v in toks:
        if kind == "lit":
            w.put_symbol(v)
            continue
        k = max(j for j in range(29) if LENGTH_BASE[j] <= v)
        if v == 258:
            k = 28
        elif k == 28:
            k = 27
        w.put_symbol(257 + k)
        w.put(v - LENGTH_BASE[k], LENGTH_EXTRA[k])
        w.put_code(D - 1, 5)
    w.put_symbol(256)
    return w.total if want_bits else w.done()


def zlib_stream_of(S, D, fast=False):
    S = bytes(S)
    toks = tokens_fast(S, D) if fast else tokens(S, D)
    check = zlib.adler32(S) if fast else adler32(S)
    return b"\x78\x01" + deflate(toks, D) + struct.pack(">I", check)


def zlib_stream(image, bits, fast=False):
    """The device PNG stream of an image [H][W]."""
    if fast:
        a = np.asarray(image)
        H = a.shape[0]
        px = a.astype(">u2" if bits == 16 else np.uint8).reshape(H, -1).view(np.uint8)
        S = np.concatenate([np.zeros((H, 1), np.uint8), px], 1).tobytes()
    else:
        S = filtered(image, bits)
    return zlib_stream_of(S, bits // 8, fast)


def chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xffffffff)


def png_file(stream, W, H, bits):
    """The PNG file around a zlib stream: signature, IHDR (grey), one IDAT, IEND."""
    return (SIGNATURE + chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, bits, 0, 0, 0, 0)) + chunk(b"IDAT", stream)
            + chunk(b"IEND", b""))

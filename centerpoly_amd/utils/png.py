"""Grey PNG files, 8 or 16 bit, compressed on the device ("device PNG stream" in include/centerpoly_hip.h).

`encode` turns device planes (uint8 masks) or device id images (int32) into complete PNG files: cp_png_deflate builds
every image's zlib stream -- filter "None", run-length matches in one fixed-Huffman block, Adler-32 -- and one copy
brings the compressed bytes back; the host only frames them (signature, IHDR, IDAT, IEND and their CRC-32s).  zlib and
PIL read the files; they are larger than PIL's own (fixed codes, matches of at most 258 bytes).  There is no host
fallback.  tests/golden/png_host.py is the format's literal statement."""
import ctypes
import struct
import zlib

import numpy as np
import torch

from .. import _C

MAX_PLANES, MAX_SIDE = 128, 16384
SIGNATURE = b"\x89PNG\r\n\x1a\n"
FIRST_DIVISOR, FIRST_FLOOR = 32, 1024                    # first capacity per image: stream bytes / 32 + 1 KiB


def _chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(data, zlib.crc32(kind)) & 0xffffffff)


def frame(stream, W, H, bits):
    """The PNG file around one zlib stream."""
    return b"".join([SIGNATURE, _chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, bits, 0, 0, 0, 0)),
                     _chunk(b"IDAT", stream), _chunk(b"IEND", b"")])


def _source(planes, images, bits):
    if (planes is None) == (images is None):
        raise ValueError("encode takes exactly one of planes and images")
    if bits not in (8, 16):
        raise ValueError("an id image has 8 or 16 bits, not %r" % (bits,))
    src = planes if planes is not None else images
    if not torch.is_tensor(src) or not src.is_cuda:
        raise _C.NativeError("png.encode needs HIP device tensors (got %s); there is no CPU fallback"
                             % (src.device if torch.is_tensor(src) else type(src).__name__))
    if src.dim() == 2:
        src = src[None]
    if planes is not None and (src.dtype != torch.uint8 or src.dim() != 3 or bits != 8):
        raise ValueError("planes must be uint8 [n, H, W] with bits 8, got %s %s, bits %d"
                         % (src.dtype, tuple(src.shape), bits))
    if images is not None and (src.dtype != torch.int32 or src.dim() != 3):
        raise ValueError("images must be int32 [n, H, W], got %s %s" % (src.dtype, tuple(src.shape)))
    return src.contiguous()


def zlib_stream(planes=None, images=None, bits=8, bounds=None, capacity=None, names=None):
    """The zlib streams (list of n bytes objects) of device planes uint8 [n, H, W] (bits 8, the bytes as they are) or
    device images int32 [n, H, W] (bits 8 or 16); a single [H, W] counts as n = 1.  bounds int32 [n, 4] inclusive x0,
    y0, x1, y1 (a host array or a device tensor; W, H, -1, -1 = empty): a promise that image k is zero outside its box.
    capacity: the first call's output bytes (default: 1/32 of the raw bytes and 1 KiB per image).  One copy comes
    back; a second call follows when the capacity was too small.  An image value outside [0, 2^bits) is a ValueError
    that names the image (names[k], default "image k") and the value."""
    src = _source(planes, images, bits)
    n, H, W = (int(v) for v in src.shape)
    if n == 0:
        return []
    D = bits // 8
    stream_bytes = H * (1 + W * D)
    if n > MAX_PLANES or H > MAX_SIDE or W > MAX_SIDE or n * stream_bytes >= 1 << 31:
        raise ValueError("encode takes 1 .. %d images of at most %d x %d and less than 2^31 stream bytes per call, got "
                         "%d of %d x %d" % (MAX_PLANES, MAX_SIDE, MAX_SIDE, n, W, H))
    dev = src.device
    if bounds is not None and not torch.is_tensor(bounds):
        bounds = torch.from_numpy(np.ascontiguousarray(bounds, dtype=np.int32).reshape(n, 4)).to(dev)
    if bounds is not None:
        if bounds.dtype != torch.int32 or tuple(bounds.shape) != (n, 4):
            raise ValueError("bounds must be int32 [n, 4], got %s %s" % (bounds.dtype, tuple(bounds.shape)))
        bounds = bounds.contiguous()
    L = _C.lib()
    cap = int(capacity) if capacity is not None else n * (stream_bytes // FIRST_DIVISOR + FIRST_FLOOR)
    nbytes = L.cp_png_deflate_workspace_bytes(n, H, W, bits)
    ws = _C.workspace(nbytes, dev)
    o_table = 16
    o_out = o_table + 16 * n
    for attempt in range(2):
        out = torch.empty((o_out + cap + 16,), dtype=torch.uint8, device=dev)
        at = lambda o: ctypes.c_void_p(out.data_ptr() + o)                # noqa: E731
        _C.check(L.cp_png_deflate(_C.ptr(src) if planes is not None else None, _C.ptr(src) if planes is None else None,
                                  n, H, W, bits, _C.ptr(bounds), at(o_out), cap, at(o_table), at(0), _C.ptr(ws), nbytes,
                                  _C.stream()), "cp_png_deflate")
        host = out.cpu().numpy()                                          # the one copy
        head = host[:16].view(np.int32)
        if not head[1]:
            break
        if attempt:
            raise _C.NativeError("cp_png_deflate reports an overflow at the capacity its own head asked for")
        cap = int(head[0])
    table = host[o_table:o_out].view(np.int32).reshape(n, 4)
    if images is not None:
        for k in range(n):
            lo, hi = int(table[k, 2]), int(table[k, 3])
            bad = lo if lo < 0 else hi if hi >= 1 << bits else None
            if bad is not None:
                raise ValueError("%s: the value %d does not fit a %d-bit image"
                                 % (names[k] if names is not None else "image %d" % k, bad, bits))
    data = host[o_out:o_out + cap].tobytes()
    return [data[int(table[k, 0]):int(table[k, 0]) + int(table[k, 1])] for k in range(n)]


def encode(planes=None, images=None, bits=8, bounds=None, capacity=None, names=None):
    """The complete PNG files (list of n bytes objects, mode L or I;16) of zlib_stream's inputs."""
    src = planes if planes is not None else images
    streams = zlib_stream(planes, images, bits, bounds, capacity, names)
    H, W = (int(src.shape[-2]), int(src.shape[-1])) if streams else (0, 0)
    return [frame(s, W, H, bits) for s in streams]


def write(paths, planes=None, images=None, bits=8, bounds=None):
    """encode, and file k to paths[k] (more than 128 images in batches).  A single [H, W] image takes one path in a
    list.  Returns the bytes written."""
    paths = list(paths)
    src = planes if planes is not None else images
    if src is not None and torch.is_tensor(src) and src.dim() == 2:
        src = src[None]
        planes, images = (src, None) if planes is not None else (None, src)
    if src is None or int(src.shape[0]) != len(paths):
        raise ValueError("write takes one path per image, got %d paths for %s"
                         % (len(paths), None if src is None else tuple(src.shape)))
    total = 0
    for k0 in range(0, len(paths), MAX_PLANES):
        part = slice(k0, k0 + MAX_PLANES)
        files = encode(planes[part] if planes is not None else None, images[part] if images is not None else None,
                       bits, bounds[part] if bounds is not None else None, names=paths[part])
        for path, data in zip(paths[part], files):
            with open(path, "wb") as f:
                f.write(data)
            total += len(data)
    return total

"""The device PNG stream's host statement (tests/golden/png_host.py) against zlib and PIL: every stream inflates to the
filtered bytes, every file opens with the mode, size and pixels of PIL's own.  No device.  test_png.py runs the same
cases on the GPU."""
import contextlib
import io
import zlib

import numpy as np
import pytest

import png_host as host

_CASES = {}


def polygon_mask(H, W, seed=5):
    from PIL import Image, ImageDraw
    rng = np.random.default_rng(seed)
    ang = np.sort(rng.uniform(0, 2 * np.pi, 11))
    rad = rng.uniform(0.2, 0.45, 11) * min(H, W)
    pts = [(float(W / 2 + r * np.cos(a)), float(H / 2 + r * np.sin(a))) for a, r in zip(ang, rad)]
    im = Image.new("L", (W, H), 0)
    ImageDraw.Draw(im).polygon(pts, outline=0, fill=255)
    return np.array(im)


def id_image(H, W, seed=7):
    """A 16-bit id image: boxes of label * 1000 + instance over regions of plain labels, and the format's corner values."""
    rng = np.random.default_rng(seed)
    a = np.zeros((H, W), np.int32)
    a[H // 2:] = 7
    for k in range(12):
        y, x = int(rng.integers(0, H - 3)), int(rng.integers(0, W - 3))
        a[y:y + int(rng.integers(2, H // 2)), x:x + int(rng.integers(2, W // 2))] = int(rng.integers(24, 34)) * 1000 + k
    a[0, :5] = [0, 255, 256, 0xFF00, 65535]
    return a


def every_length():
    """One 8-bit image whose stream holds every match length 3 .. 258 and intervals of 1, 2, 259, 260, 261 and 516 + 2
    equal bytes: row r starts with r + 1 equal pixels (a literal and r bytes equal to their predecessor), then pixels
    that alternate, so nothing else repeats; the values lie on both sides of 144."""
    W = 530
    lengths = list(range(3, 259)) + [1, 2, 259, 260, 261, 518]
    a = np.zeros((len(lengths), W), np.uint8)
    for y, r in enumerate(lengths):
        a[y, :r + 1] = 100 if y % 2 else 200
        rest = W - (r + 1)
        a[y, r + 1:] = np.where(np.arange(rest) % 2 == 0, 9, 150)
    return a


def cases():
    """{name: (image, bits)}, made once."""
    if not _CASES:
        rng = np.random.default_rng(12)
        _CASES.update({
            "one_pixel": (np.array([[200]], np.uint8), 8),
            "one_pixel_16": (np.array([[0x1234]], np.int32), 16),
            "W1": ((rng.random((300, 1)) < 0.5).astype(np.uint8) * 255, 8),
            "H1": ((rng.random((1, 300)) < 0.3).astype(np.uint8) * 255, 8),
            "zeros": (np.zeros((40, 70), np.uint8), 8),
            "polygon": (polygon_mask(64, 96), 8),
            "ids16_odd": (id_image(37, 53), 16),
            "labels8": (np.minimum(id_image(37, 53) // 1000, 255).astype(np.int32), 8),
            "noise": (rng.integers(0, 256, (37, 53)).astype(np.uint8), 8),
            "noise16": (rng.integers(0, 65536, (9, 31)).astype(np.int32), 16),
            "every_length": (every_length(), 8),
        })
    return _CASES


def pil_file_pixels(a, bits):
    """(mode, size, pixels) of the file PIL itself writes for the image."""
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(a.astype(np.uint16 if bits == 16 else np.uint8)).save(buf, "PNG")
    im = Image.open(io.BytesIO(buf.getvalue()))
    return im.mode, im.size, np.array(im)


def check_file(data, a, bits):
    """A PNG file's bytes open with PIL's mode, size and pixels for the image."""
    from PIL import Image
    im = Image.open(io.BytesIO(data))
    mode, size, pixels = pil_file_pixels(a, bits)
    assert (im.mode, im.size) == (mode, size) and mode == ("I;16" if bits == 16 else "L")
    got = np.array(im)
    assert got.dtype == pixels.dtype and np.array_equal(got, pixels)


@pytest.mark.parametrize("name", sorted(cases()))
def test_the_statement_inflates_and_opens(name):
    a, bits = cases()[name]
    S = host.filtered(a.tolist(), bits)
    assert len(S) == a.shape[0] * (1 + a.shape[1] * bits // 8)
    stream = host.zlib_stream(a.tolist(), bits)
    assert stream[:2] == b"\x78\x01" and zlib.decompress(stream) == S
    assert host.adler32(S) == zlib.adler32(S)
    toks = host.tokens(S, bits // 8)
    assert host.tokens_fast(S, bits // 8) == toks
    assert host.zlib_stream(a, bits, fast=True) == stream
    assert sum(v if kind == "match" else 1 for kind, v in toks) == len(S)
    check_file(host.png_file(stream, a.shape[1], a.shape[0], bits), a, bits)


def test_every_match_length_occurs():
    a, bits = cases()["every_length"]
    toks = host.tokens(host.filtered(a.tolist(), bits), 1)
    lengths = [v for kind, v in toks if kind == "match"]
    assert set(lengths) == set(range(3, 259))
    lits = {v for kind, v in toks if kind == "lit"}
    assert min(lits) < 144 <= max(lits)
    # the rows of 1, 2, 259, 260, 261 and 518 equal bytes: literals; 258 + 1; 258 + 2; 258 + 3; 258 + 258 + 2
    rows = {}
    at = 0
    for kind, v in toks:
        rows.setdefault(at // 531, []).append((kind, v))
        at += v if kind == "match" else 1
    head = lambda y, k: [t if t[0] == "match" else "lit" for t in rows[y][1:k + 1]]                   # noqa: E731
    first = 256
    assert head(first, 3) == ["lit"] * 3 and head(first + 1, 4) == ["lit"] * 4
    assert head(first + 2, 3) == ["lit", ("match", 258), "lit"]
    assert head(first + 3, 4) == ["lit", ("match", 258), "lit", "lit"]
    assert head(first + 4, 3) == ["lit", ("match", 258), ("match", 3)]
    assert head(first + 5, 5) == ["lit", ("match", 258), ("match", 258), "lit", "lit"]


def test_sizes_of_the_streams_are_as_expected():
    """Fixed codes: a literal costs 8 or 9 bits, so noise grows by about an eighth; a plane of zeros costs 13 bits per
    258 bytes (symbol 285 in 8 bits, the distance in 5)."""
    a, bits = cases()["zeros"]
    n = a.shape[0] * (1 + a.shape[1])
    stream = host.zlib_stream(a.tolist(), bits)
    full, rest = divmod(n - 1, 258)
    assert rest < 3                                                       # (this shape's remainder is literals)
    want_bits = 3 + 8 + 13 * full + 8 * rest + 7
    assert len(stream) == 2 + (want_bits + 7) // 8 + 4
    a, bits = cases()["noise"]
    assert a.size < len(host.zlib_stream(a.tolist(), bits)) < a.size * 9 // 8 + 64


def test_the_flag_parses_and_is_off_by_default():
    import importlib.util
    import os
    from centerpoly_amd.opts import opts
    with contextlib.redirect_stdout(io.StringIO()):
        assert opts().parse(["polydet"]).device_png is False
        assert opts().parse(["polydet", "--device_png"]).device_png is True
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("centerpoly_make_ground_truth", os.path.join(root, "make_ground_truth.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.parse_args(["--dataset", "IDD", "--gt_dir", "x"]).device_png is False
    assert mod.parse_args(["--dataset", "IDD", "--gt_dir", "x", "--device_png"]).device_png is True


def test_the_module_refuses_host_tensors_and_bad_bits():
    import torch
    from centerpoly_amd import _C
    from centerpoly_amd.utils import png
    plane = torch.zeros((1, 4, 5), dtype=torch.uint8)
    with pytest.raises(_C.NativeError, match="no CPU fallback"):
        png.encode(planes=plane)
    with pytest.raises(_C.NativeError, match="no CPU fallback"):
        png.zlib_stream(images=torch.zeros((4, 5), dtype=torch.int32), bits=16)
    with pytest.raises(ValueError, match="8 or 16 bits"):
        png.encode(images=torch.zeros((4, 5), dtype=torch.int32), bits=12)
    with pytest.raises(ValueError, match="exactly one"):
        png.encode()
    with pytest.raises(ValueError, match="exactly one"):
        png.encode(planes=plane, images=plane)


def test_the_module_frames_as_the_statement_does():
    from centerpoly_amd.utils import png
    a, bits = cases()["ids16_odd"]
    stream = host.zlib_stream(a.tolist(), bits)
    assert png.frame(stream, a.shape[1], a.shape[0], bits) == host.png_file(stream, a.shape[1], a.shape[0], bits)

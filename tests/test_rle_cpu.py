"""Run-length masks without a GPU: the literal host statement (tests/golden/rle_host.py) on the vectors of the
definition, the package's vectorised host code (parse_counts, area, to_bbox) against it, every malformed-input error,
the entry points' argument checks and the options."""
import contextlib
import ctypes
import io

import numpy as np
import pytest

import rle_host as host

NUMBERS = [(0, "0"), (5, "5"), (15, "?"), (16, "`0"), (31, "o0"), (32, "P1"), (-1, "O"), (-16, "@"), (-17, "_O"),
           (511, "o?"), (512, "P`0"), (1024, "PP1"), (2097152, "PPPP2"), (2 ** 31 - 1, "oooooo1"),
           (-2 ** 31, "PPPPPPN")]


def random_mask(rng, H, W):
    """Random density, or a few rectangles (long runs)."""
    if rng.random() < 0.5:
        return (rng.random((H, W)) < rng.random()).astype(np.uint8)
    m = np.zeros((H, W), np.uint8)
    for _ in range(int(rng.integers(0, 4))):
        y0, x0 = int(rng.integers(0, H)), int(rng.integers(0, W))
        m[y0:y0 + int(rng.integers(1, H + 1)), x0:x0 + int(rng.integers(1, W + 1))] = rng.integers(1, 256)
    return m


@pytest.mark.parametrize("number,text", NUMBERS)
def test_single_numbers(number, text):
    # the number stands alone as cnts[0] (no delta applies before i = 3)
    assert host.to_string([number]) == text
    assert host.from_string(text) == [number]


def test_whole_vectors():
    assert host.encode([[0, 1, 1], [1, 1, 0]]) == [1, 4, 1]
    assert host.to_string([1, 4, 1]) == "141"
    cnts = [3, 1, 2, 40, 1, 7, 300, 5]
    assert host.to_string(cnts) == "312W1OoN[9N"
    assert host.from_string("312W1OoN[9N") == cnts
    assert host.encode([[1]]) == [0, 1] and host.encode([[0]]) == [1]


def test_string_round_trip_with_zero_length_runs():
    rng = np.random.default_rng(5)
    for _ in range(200):
        m = int(rng.integers(1, 40))
        cnts = [int(v) for v in rng.choice([0, 0, 1, 2, 15, 16, 17, 31, 32, 500, 1024, 70000], m)]
        assert host.from_string(host.to_string(cnts)) == cnts


def test_package_host_code_against_the_statement():
    from centerpoly_amd.utils import rle
    rng = np.random.default_rng(7)
    for i in range(300):
        H, W = (int(v) for v in rng.integers(1, 41, 2))
        m = random_mask(rng, H, W)
        cnts = host.encode(m.tolist())
        text = host.to_string(cnts)
        assert sum(cnts) == H * W and host.area(cnts) == int((m != 0).sum())
        assert rle.parse_counts(text, H * W).tolist() == cnts
        assert rle.parse_counts(text.encode("ascii")).tolist() == cnts
        forms = [{"size": [H, W], "counts": text}, {"size": [H, W], "counts": text.encode("ascii")},
                 {"size": [H, W], "counts": cnts}]
        assert rle.area(forms) == [host.area(cnts)] * 3
        assert rle.to_bbox(forms) == [host.to_bbox(cnts, H, W)] * 3
        back, status = host.decode(cnts, H, W, 7)
        assert status == 0 and np.array_equal(back, (m != 0) * 7)
    # counts with zero-length runs inside, and the numbers of the table as deltas
    cnts = [0, 3, 0, 0, 2, 1, 0, 4]
    assert rle.parse_counts(host.to_string(cnts)).tolist() == cnts
    for number, _ in NUMBERS[:-2]:
        cnts = [1, 40, 2, 40 + number] if number >= -40 else None
        if cnts:
            assert rle.parse_counts(host.to_string(cnts)).tolist() == cnts
    assert rle.parse_counts("oooooo1").tolist() == [2 ** 31 - 1] and rle.parse_counts("PPPPPPN").tolist() == [-2 ** 31]


def test_host_decode_refuses_wrong_sums():
    assert host.decode([3, 2], 2, 2)[1] == 1 and host.decode([1, 2], 2, 2)[1] == 1
    assert host.decode([2, 0, 2], 2, 2)[1] == 0


@pytest.mark.parametrize("counts,words", [
    ("14/1", "outside the RLE alphabet"), ("14p", "outside the RLE alphabet"), ("14é", "outside the RLE alphabet"),
    ("PPPPPPP1", "longer than 7"), ("14P", "truncated"), ("O", "below 0"), ("27", "above H * W"),
    ("113N", "below 0"),                                                  # 1, 1, 3, then -2 + 1 = -1 after the delta
])
def test_malformed_strings_name_the_entry(counts, words):
    from centerpoly_amd.utils import rle
    rles = [{"size": [2, 3], "counts": "6"}, {"size": [2, 3], "counts": counts}]
    for call in (lambda: rle.decode(rles, "cpu"), lambda: rle.area(rles), lambda: rle.to_bbox(rles)):
        with pytest.raises(ValueError) as e:
            call()
        assert "rle 1" in str(e.value) and words in str(e.value)
    with pytest.raises(ValueError) as e:
        rle.decode(rles, "cpu", names=["first", "second"])
    assert "second" in str(e.value)


def test_decode_refuses_mixed_sizes_and_bad_dictionaries():
    from centerpoly_amd.utils import rle
    with pytest.raises(ValueError) as e:
        rle.decode([{"size": [2, 3], "counts": "6"}, {"size": [3, 2], "counts": "6"}], "cpu")
    assert "rle 1" in str(e.value) and "size" in str(e.value)
    with pytest.raises(ValueError):
        rle.decode([{"counts": "6"}], "cpu")
    with pytest.raises(ValueError):
        rle.decode([{"size": [2, 3], "counts": [7]}], "cpu")
    with pytest.raises(ValueError):
        rle.decode([], "cpu")


def test_encode_and_decode_have_no_host_fallback():
    import torch
    from centerpoly_amd import _C
    from centerpoly_amd.utils import rle
    with pytest.raises(_C.NativeError):
        rle.encode(masks=torch.zeros((1, 4, 4), dtype=torch.uint8))
    with pytest.raises(_C.NativeError):
        rle.decode([{"size": [2, 3], "counts": "6"}], "cpu")
    with pytest.raises(ValueError):
        rle.encode()
    with pytest.raises(ValueError):
        rle.encode(index=torch.zeros((4, 4), dtype=torch.uint8))           # n is missing


def test_argument_validation_without_gpu():
    """The entry points check everything before any device work: callable with no GPU, on made-up addresses."""
    from centerpoly_amd import _C
    L = _C.lib()
    p = ctypes.c_void_p(4096)                                             # never dereferenced: every call is refused
    EINVAL, EUNSUPPORTED, EWORKSPACE = -1, -2, -3
    need = L.cp_rle_encode_workspace_bytes(2, 8, 10, 100)
    assert need >= 2 * 10 * 4 * 24 and need == L.cp_rle_encode_workspace_bytes(2, 8, 10, 0)
    assert L.cp_rle_encode_workspace_bytes(0, 8, 10, 0) == 0

    def enc(planes=p, index=None, n=2, H=8, W=10, bounds=None, counts=p, cap_counts=10, chars=p, cap_bytes=10, table=p,
            head=p, ws=p, ws_bytes=need):
        return L.cp_rle_encode(planes, index, n, H, W, bounds, counts, cap_counts, chars, cap_bytes, table, head, ws,
                               ws_bytes, None)
    assert enc(planes=None) == EINVAL and enc(index=p) == EINVAL          # neither, both
    assert enc(n=0) == EINVAL and enc(H=0) == EINVAL and enc(W=-1) == EINVAL
    assert enc(cap_counts=-1) == EINVAL and enc(cap_bytes=-1) == EINVAL
    assert enc(table=None) == EINVAL and enc(head=None) == EINVAL and enc(chars=None) == EINVAL
    assert enc(bounds=ctypes.c_void_p(4098)) == EINVAL and enc(counts=ctypes.c_void_p(4097)) == EINVAL
    assert enc(n=129, ws_bytes=1 << 30) == EUNSUPPORTED
    assert enc(planes=None, index=p, n=256, ws_bytes=1 << 30) == EUNSUPPORTED
    assert enc(H=1 << 16, W=1 << 15, ws_bytes=1 << 40) == EUNSUPPORTED
    assert enc(ws=None) == EWORKSPACE and enc(ws_bytes=need - 1) == EWORKSPACE
    assert enc(ws=ctypes.c_void_p(4100)) == EINVAL                        # the workspace is 16-byte aligned

    table = (ctypes.c_int32 * 4)(0, 3, 3, 2)
    need = L.cp_rle_decode_workspace_bytes(2, 5)
    assert need >= 20 and L.cp_rle_decode_workspace_bytes(0, 5) == 0

    def dec(counts=p, table=table, n=2, H=8, W=10, value=255, planes=p, status=p, ws=p, ws_bytes=need):
        return L.cp_rle_decode(counts, table, n, H, W, value, planes, status, ws, ws_bytes, None)
    assert dec(counts=None) == EINVAL and dec(table=None) == EINVAL and dec(planes=None) == EINVAL
    assert dec(status=None) == EINVAL and dec(n=0) == EINVAL and dec(H=0) == EINVAL
    assert dec(value=256) == EINVAL and dec(value=-1) == EINVAL
    assert dec(table=(ctypes.c_int32 * 4)(0, 3, -1, 2)) == EINVAL and dec(table=(ctypes.c_int32 * 4)(0, -3, 3, 2)) == EINVAL
    assert dec(n=256, table=(ctypes.c_int32 * 512)()) == EUNSUPPORTED
    assert dec(H=1 << 16, W=1 << 15) == EUNSUPPORTED
    assert dec(ws=None) == EWORKSPACE and dec(ws_bytes=need - 1) == EWORKSPACE


def _parse(args):
    from centerpoly_amd.opts import opts
    with contextlib.redirect_stdout(io.StringIO()):
        return opts().parse(["polydet", "--arch", "dla_34"] + args)


def test_options(capsys):
    opt = _parse(["--dataset", "kitti_poly", "--save_rle", "--mots_class_map", "26:1,24:2"])
    assert opt.save_rle and opt.mots_classes == {26: 1, 24: 2}
    opt = _parse(["--dataset", "kitti_poly"])
    assert not opt.save_rle and opt.mots_classes is None
    with pytest.raises(SystemExit):
        _parse(["--dataset", "synthetic", "--save_rle"])
    err = capsys.readouterr().err
    assert "draws with a data set's result writer; the synthetic set has none" in err
    for bad in ("26", "26:1:2", "a:1", "26:1,,24:2", "26:1,26:2", "-3:1", "26:-1", "26:1,"):
        with pytest.raises(SystemExit):
            _parse(["--dataset", "kitti_poly", "--mots_class_map", bad])
        assert "--mots_class_map" in capsys.readouterr().err


def test_class_map_and_mots_file_names():
    from centerpoly_amd.detectors import tracking
    assert tracking.parse_class_map("") is None and tracking.parse_class_map(" 26:1 , 24:2 ") == {26: 1, 24: 2}
    w = tracking.MotsWriter("/x/instances")
    assert w.path("/data/image_2/drive_a/") == "/x/instances/mots/data_image_2_drive_a.txt"
    assert w.path("/") == "/x/instances/mots/sequence.txt"

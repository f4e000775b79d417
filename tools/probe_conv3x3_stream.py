"""GPU probe: the streaming 3x3 convolution to <= 32 channels (cp_conv3x3_stream_forward, csrc/conv3x3_stream.hip) against
the LDS-staged one (cp_conv_mfma_forward_strided, taps = 9) back to back on the same tensors, at the three
conv_offset_mask shapes that the 1 x 3 x 1024 x 2048 DLA-34 inference step runs as launches of their own.

Per shape: average / minimum launch time of the staged kernel, then of every tile form nt x ks (ks = the staged kernel's K
split, the only one with its bits) of the streaming kernel (HIP events around each launch, 40 launches after 5 of
warm-up), the default form marked with *, and whether the default form's result has the staged result's bits (it must).
A shape enters conv3x3._STREAM3_SHAPES only where the default form's AVERAGE is below the staged kernel's MINIMUM.
Usage: probe_conv3x3_stream.py [out.txt]"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from centerpoly_amd import _C
if os.environ.get("CP_PROBE_LIB"):                # another build of the library
    _C.LIB_PATH = os.path.abspath(os.environ["CP_PROBE_LIB"])
L = _C.lib()
dev = "cuda"
torch.manual_seed(0)

# (Cin, Cout, H, W), launches per step
DLA = [((128, 27, 128, 256), 6), ((256, 27, 64, 128), 4), ((512, 27, 32, 64), 1)]


def timed(call, n=40):
    """(average, minimum) us per launch."""
    for _ in range(5):
        call()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    for e0, e1 in ev:
        e0.record()
        call()
        e1.record()
    torch.cuda.synchronize()
    ts = [e0.elapsed_time(e1) * 1e3 for e0, e1 in ev]
    return sum(ts) / n, min(ts)


def main():
    args = sys.argv[1:]
    lines = ["%-22s %4s %6s | staged avg / min | stream forms nt x ks: avg / min us (* default) | result"
             % ("layer", "/stp", "MB")]
    for (cin, co, H, W), per_step in DLA:
        x = torch.randn(1, cin, H, W, device=dev)
        w = torch.randn(co, cin, 3, 3, device=dev) * (1.0 / (9 * cin) ** 0.5)
        b = torch.randn(co, device=dev) * 0.1
        ptrs, chans = (_C.c_void_p * 1)(x.data_ptr()), (_C.c_int32 * 1)(cin)
        wp = torch.empty(L.cp_conv_mfma_weight_bytes(cin, co, 9), dtype=torch.uint8, device=dev)
        _C.check(L.cp_conv_mfma_prepare(_C.ptr(w), cin, co, 9, 0, _C.ptr(wp), _C.stream()), "prepare")
        old = torch.empty(1, co, H, W, device=dev)             # one prepared form serves both kernels
        new = torch.empty_like(old)

        def staged():
            _C.check(L.cp_conv_mfma_forward_strided(ptrs, chans, 1, _C.ptr(wp), _C.ptr(b), None, _C.ptr(old), 1, H, W, co,
                                                    9, 1, 0, _C.stream()), "staged")
        mb = (cin + co) * H * W * 4 / 1e6
        line = "%-22s %4d %6.1f | %6.1f / %6.1f |" % ("%d->%d @%dx%d" % (cin, co, H, W), per_step, mb, *timed(staged))
        default = L.cp_conv3x3_stream_form(cin, co, H, W, 1)
        ks = default & 255
        for nt in (1, 2, 4):
            def stream():
                _C.check(L.cp_conv3x3_stream_forward_form(_C.ptr(x), _C.ptr(wp), _C.ptr(b), None, _C.ptr(new), 1, cin, H, W,
                                                          co, 0, nt, ks, _C.stream()), "stream")
            new.fill_(float("nan"))
            line += " %dx%d%s %.1f / %.1f" % (nt, ks, "*" if default == (nt << 8 | ks) else "", *timed(stream))
            line += "" if torch.equal(new, old) else " (DIFFERS)"
        new.fill_(float("nan"))
        _C.check(L.cp_conv3x3_stream_forward(_C.ptr(x), _C.ptr(wp), _C.ptr(b), None, _C.ptr(new), 1, cin, H, W, co, 0,
                                             _C.stream()), "stream")
        line += " | %s" % ("same bits" if torch.equal(new, old) else "DIFFERS %.1e" % ((new - old).abs().max().item() / old.abs().max().item()))
        print(line, flush=True)
        lines.append(line)
    if args:
        with open(args[0], "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

"""GPU probe: the streaming 1x1 convolution (cp_conv1x1_stream_forward, csrc/conv_stream.hip) against the LDS-staged one
(cp_conv_mfma_forward_strided, taps = 1) back to back on the same tensors, at the ten Root / project shapes of the
1 x 3 x 1024 x 2048 DLA-34 inference step.

Per shape: average / minimum launch time of the staged kernel, then of every tile form of the streaming kernel (HIP
events around each launch, 40 launches after 5 of warm-up), the default form marked with *, and whether the default
form's result has the staged result's bits (it must).  A shape enters conv3x3._STREAM_SHAPES only where the default
form's AVERAGE is below the staged kernel's MINIMUM.  Usage: probe_conv1x1_stream.py [out.txt]"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from centerpoly_amd import _C
if os.environ.get("CP_PROBE_LIB"):                # another build of the library (e.g. -DCP_STREAM_DEPTH=4)
    _C.LIB_PATH = os.path.abspath(os.environ["CP_PROBE_LIB"])
L = _C.lib()
dev = "cuda"
torch.manual_seed(0)

# (sources, Cout, H, W)
DLA = [((32,), 64, 256, 512), ((64, 64), 64, 256, 512), ((64,), 128, 128, 256), ((128, 128), 128, 128, 256),
       ((128, 128, 64, 128), 128, 128, 256), ((128,), 256, 64, 128), ((256, 256), 256, 64, 128),
       ((256, 256, 128, 256), 256, 64, 128), ((256,), 512, 32, 64), ((512, 512, 256), 512, 32, 64)]
FORMS = [(2, 1), (1, 1), (2, 2), (1, 2), (2, 4), (1, 4)]


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
    lines = ["%-34s %6s | staged avg / min | stream forms nb x ks: avg / min us (* default) | result" % ("layer", "MB")]
    for cs, co, H, W in DLA:
        cin, n = sum(cs), len(cs)
        xs = [torch.randn(1, c, H, W, device=dev) for c in cs]
        w = torch.randn(co, cin, 1, 1, device=dev) * (1.0 / cin ** 0.5)
        b, res = torch.randn(co, device=dev) * 0.1, torch.randn(1, co, H, W, device=dev)
        ptrs, chans = (_C.c_void_p * n)(*[x.data_ptr() for x in xs]), (_C.c_int32 * n)(*cs)
        wp0 = torch.empty(L.cp_conv_mfma_weight_bytes(cin, co, 1), dtype=torch.uint8, device=dev)
        _C.check(L.cp_conv_mfma_prepare(_C.ptr(w), cin, co, 1, 0, _C.ptr(wp0), _C.stream()), "prepare")
        wp1 = wp0                                                 # one prepared form serves both kernels
        old, new = torch.empty_like(res), torch.empty_like(res)
        rp = _C.ptr(res) if n > 1 else None                       # Root adds its first child, project adds nothing

        def staged():
            _C.check(L.cp_conv_mfma_forward_strided(ptrs, chans, n, _C.ptr(wp0), _C.ptr(b), rp, _C.ptr(old), 1, H, W, co,
                                                    1, 1, 1, _C.stream()), "staged")
        mb = (cin + co + (co if n > 1 else 0)) * H * W * 4 / 1e6
        line = "%-34s %6.1f | %6.1f / %6.1f |" % ("%s->%d @%dx%d" % ("+".join(map(str, cs)), co, H, W), mb, *timed(staged))
        default = L.cp_conv1x1_stream_form(cin, co, H, W, 1)
        for nb, ks in FORMS:
            def stream():
                _C.check(L.cp_conv1x1_stream_forward_form(ptrs, chans, n, _C.ptr(wp1), _C.ptr(b), rp, _C.ptr(new), 1, H, W,
                                                          co, 1, nb, ks, _C.stream()), "stream")
            line += " %dx%d%s %.1f / %.1f" % (nb, ks, "*" if default == (nb << 8 | ks) else "", *timed(stream))
        _C.check(L.cp_conv1x1_stream_forward(ptrs, chans, n, _C.ptr(wp1), _C.ptr(b), rp, _C.ptr(new), 1, H, W, co, 1,
                                             _C.stream()), "stream")
        line += " | %s" % ("same bits" if torch.equal(new, old) else "DIFFERS %.1e" % ((new - old).abs().max().item() / old.abs().max().item()))
        print(line, flush=True)
        lines.append(line)
    if args:
        with open(args[0], "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

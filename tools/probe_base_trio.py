"""GPU probe: the three full-resolution layers of the DLA base as the stem launch + the pair launch
(cp_conv7x7_c3_forward, cp_dla_base_pair_forward) against the one-launch form cp_dla_base_trio_forward, at
1 x 3 x 1024 x 2048 and 4 x 3 x 512 x 1024: HIP events around each of 40 launches, back to back on the same tensors;
average and fastest launch in us, and whether the results are the same bits.  Writes profiles/base_trio_probe.txt
(PROBE_OUT names another file; PROBE_LAUNCHES another count, for counter passes)."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from centerpoly_amd import _C
L = _C.lib(); dev = "cuda"
torch.manual_seed(0)
N = int(os.environ.get("PROBE_LAUNCHES", "40"))


def timed(call, n=N):
    for _ in range(3):
        call()
    torch.cuda.synchronize()
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    for e0, e1 in evs:
        e0.record()
        call()
        e1.record()
    torch.cuda.synchronize()
    us = [e0.elapsed_time(e1) * 1e3 for e0, e1 in evs]
    return sum(us) / n, min(us)


lines = []
for B, H, W in ((1, 1024, 2048), (4, 512, 1024)):
    x = torch.randn(B, 3, H, W, device=dev)
    ws = torch.randn(16, 3, 7, 7, device=dev) * 0.08; bs = torch.randn(16, device=dev) * 0.1
    w0 = torch.randn(16, 16, 3, 3, device=dev) * 0.08; b0 = torch.randn(16, device=dev) * 0.1
    w1 = torch.randn(32, 16, 3, 3, device=dev) * 0.08; b1 = torch.randn(32, device=dev) * 0.1
    wp = torch.empty(L.cp_conv7x7_c3_weight_bytes(16), dtype=torch.uint8, device=dev)
    assert L.cp_conv7x7_c3_prepare(_C.ptr(ws), 16, _C.ptr(wp), _C.stream()) == 0
    s = torch.empty(B, 16, H, W, device=dev)
    y1 = torch.full((B, 32, H // 2, W // 2), float("nan"), device=dev); o = torch.full_like(y1, float("nan"))

    def stem():
        rc = L.cp_conv7x7_c3_forward(_C.ptr(x), _C.ptr(wp), _C.ptr(bs), _C.ptr(s), B, H, W, 16, 1, 1, _C.stream())
        assert rc == 0, rc

    def pair():
        rc = L.cp_dla_base_pair_forward(_C.ptr(s), _C.ptr(w0), _C.ptr(b0), _C.ptr(w1), _C.ptr(b1), _C.ptr(y1), B, H, W,
                                        _C.stream())
        assert rc == 0, rc

    def trio():
        rc = L.cp_dla_base_trio_forward(_C.ptr(x), _C.ptr(wp), _C.ptr(bs), _C.ptr(w0), _C.ptr(b0), _C.ptr(w1), _C.ptr(b1),
                                        _C.ptr(o), B, H, W, _C.stream())
        assert rc == 0, rc

    for rep in range(2):
        (sa, sm), (pa, pm), (ta, tm) = timed(stem), timed(pair), timed(trio)
        lines.append("%d x 3 x %d x %d  stem %.1f (min %.1f) + pair %.1f (min %.1f) = %.1f us   trio %.1f (min %.1f) us"
                     % (B, H, W, sa, sm, pa, pm, sa + pa, ta, tm))
        print(lines[-1], flush=True)
    lines.append("%d x 3 x %d x %d  torch.equal(trio, stem + pair): %s" % (B, H, W, torch.equal(o, y1)))
    print(lines[-1], flush=True)
out = os.environ.get("PROBE_OUT", os.path.join(ROOT, "profiles", "base_trio_probe.txt"))
with open(out, "w") as fh:
    fh.write("\n".join(lines) + "\n")

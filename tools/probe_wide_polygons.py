"""GPU probe of the 64-vertex detection path (needs an MI355X; no fall-back):

  heads   the inference heads stage Cin -> 4 x head_conv -> 8 / 128 / 1 / 2 through heads_infer, B = 1, as the one fused
          launch (cp_heads_fused_forward, the 128-channel polygon head as two 64-column segments) and as the path taken
          before it accepted wide heads (one 3x3 convolution writing the 4 x head_conv-channel map, then the streaming
          1x1 kernels; selected here by switching HEADS_FUSED off) -- DLA-34 (64 -> 4 x 256 at 256 x 512) and Hourglass
          (256 -> 4 x 64 at 128 x 256);
  decode  polydet_decode at 8 x 256 x 512, K = 128, N = 64 beside N = 16.

Every figure: warm-up, then ROUNDS samples of CALLS back-to-back calls between device events, the variants alternating
within a round; median, min and max of the per-call time in ms.  Usage: python tools/probe_wide_polygons.py [out.json]
(default profiles/probe_wide_polygons.json)."""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from centerpoly_amd import synth  # noqa: E402
from centerpoly_amd.models.decode import polydet_decode  # noqa: E402
from centerpoly_amd.models.networks import pose_dla_dcn as pdd  # noqa: E402

DEV = "cuda"
ROUNDS, CALLS, WARM = 9, 20, 5


def sample(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(CALLS):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / CALLS


def alternate(variants):
    """{name: fn} -> {name: {median_ms, min_ms, max_ms}}, the variants taking turns within every round."""
    for fn in variants.values():
        for _ in range(WARM):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(ROUNDS):
        for k, fn in variants.items():
            times[k].append(sample(fn))
    return {k: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}
            for k, v in times.items()}


def heads_stage(tag, cin, hc, H, W, couts=(8, 128, 1, 2)):
    torch.manual_seed(5)
    fcs = [torch.nn.Sequential(torch.nn.Conv2d(cin, hc, 3, padding=1), torch.nn.ReLU(), torch.nn.Conv2d(hc, co, 1)).to(DEV)
           for co in couts]
    cat = pdd.cat_heads([(fc[0], fc[2]) for fc in fcs])
    names = ["hm", "poly", "pseudo_depth", "reg"]
    feat = torch.from_numpy(synth.normal("probe_wide/" + tag, (1, cin, H, W))).to(DEV)
    owner = torch.nn.Module()

    def run(fused):
        pdd.HEADS_FUSED = fused
        try:
            with torch.no_grad():
                return pdd.heads_infer(owner, 0, feat, cat, names)
        finally:
            pdd.HEADS_FUSED = True

    a, b = run(True), run(False)
    with torch.no_grad():
        assert pdd.heads_fused_infer(owner, 0, feat, *cat, names) is not None, "the fused launch refused the shape"
    diff = max(((a[h] - b[h]).abs().max() / b[h].abs().max()).item() for h in names)
    res = alternate({"fused": lambda: run(True), "separate": lambda: run(False)})
    res.update(shape="%d -> 4 x %d -> %s at %d x %d, B = 1" % (cin, hc, "/".join(map(str, couts)), H, W),
               fused_vs_separate_max_norm=diff)
    return res


def decode_stage():
    B, C, H, W, K = 1, 8, 256, 512, 128
    heat = torch.sigmoid(torch.from_numpy(synth.heat_logits("probe_wide/hm", B, C, H, W))).to(DEV)
    depth = torch.from_numpy(synth.uniform("probe_wide/depth", (B, 1, H, W))).to(DEV)
    reg = torch.from_numpy(synth.uniform("probe_wide/reg", (B, 2, H, W))).to(DEV)
    polys = {N: torch.from_numpy(synth.normal("probe_wide/poly%d" % N, (B, 2 * N, H, W))).to(DEV) for N in (16, 64)}
    res = alternate({"N%d" % N: (lambda p=p: polydet_decode(heat, p, depth, reg=reg, K=K)) for N, p in polys.items()})
    res["shape"] = "%d x %d x %d heat, K = %d, B = %d" % (C, H, W, K, B)
    return res


def main():
    assert torch.cuda.is_available(), "the probe needs a HIP device"
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "probe_wide_polygons.json")
    res = {"device": torch.cuda.get_device_name(0), "rounds": ROUNDS, "calls_per_sample": CALLS,
           "heads_dla34": heads_stage("dla", 64, 256, 256, 512),
           "heads_hourglass": heads_stage("hg", 256, 64, 128, 256),
           "decode": decode_stage()}
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()

"""bench.py contract checks: argument defaults, the JSON line's shape and the output dump need no GPU; one GPU test
runs the plain path end to end."""
import ast
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_defaults_and_keys():
    src = open(os.path.join(ROOT, "bench.py")).read()
    tree = ast.parse(src)
    # defaults: N=1, steps/warmup present
    assert '"--gpus", type=int, default=1' in src
    assert '"--steps", type=int' in src and '"--warmup", type=int' in src
    for key in ('"metric"', '"value"', '"unit"', '"n_gpus"', '"steps"', '"warmup"', '"ms_per_step"',
                '"higher_is_better"', '"scaling"', '"vs_baseline"', '"dtype"', '"data"', '"config"',
                '"roofline"', '"cpu_baseline"'):
        assert key in src, key
    # exactly one print to stdout (the JSON line); everything else goes to stderr
    prints = [n for n in ast.walk(tree) if isinstance(n, ast.Call) and getattr(n.func, "id", "") == "print"]
    to_stdout = [p for p in prints if not any(k.arg == "file" for k in p.keywords)]
    assert len(to_stdout) == 1
    # only the cpu_baseline leg touches the oracle
    fn = {n.name: n for n in tree.body if isinstance(n, ast.FunctionDef)}
    for name, node in fn.items():
        uses_oracle = "oracle" in ast.get_source_segment(src, node)
        assert uses_oracle == (name == "cpu_baseline"), name


def test_product_never_imports_oracle():
    for base, _, files in os.walk(os.path.join(ROOT, "centerpoly_amd")):
        for f in files:
            if f.endswith(".py"):
                text = open(os.path.join(base, f)).read()
                assert "import oracle" not in text and "from oracle" not in text, f
    for f in ("main.py", "test.py"):
        text = open(os.path.join(ROOT, f)).read()
        assert "oracle" not in text, f


def _bench():
    import importlib
    import sys
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    return importlib.import_module("bench")


def test_launch_plan_spawns_n_ranks_or_refuses():
    """`--gpus N` must never silently become a 1-GPU line (round-1 defect): without WORLD_SIZE it
    plans an N-rank torch.distributed.run child, with a disagreeing WORLD_SIZE it refuses."""
    bench = _bench()
    argv = ["--gpus", "4", "--steps", "3", "--warmup", "1"]
    args = bench.parse(argv)
    plan, cmd = bench.launch_plan(args, {}, argv)
    assert plan == "spawn"
    assert cmd[1:3] == ["-m", "torch.distributed.run"]
    assert cmd[cmd.index("--nproc-per-node") + 1] == "4"
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1"
    assert cmd[-len(argv):] == argv and cmd[-len(argv) - 1].endswith("bench.py")
    assert bench.launch_plan(args, {"WORLD_SIZE": "4"}, argv) == ("run", None)
    assert bench.launch_plan(args, {"WORLD_SIZE": "2"}, argv)[0] == "refuse"
    one = bench.parse([])
    assert bench.launch_plan(one, {}, []) == ("run", None)
    assert bench.launch_plan(one, {"WORLD_SIZE": "8"}, [])[0] == "refuse"


def test_gpus_2_without_enough_devices_exits_nonzero_and_prints_no_line():
    """On a box with fewer than N devices (this container: 0, a gpurun box: 1) `--gpus 2` exits with
    the refusal code and prints no JSON line -- it does not fall into the 1-GPU inference leg."""
    import subprocess
    import sys
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0"],
                       env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    import torch
    if torch.cuda.device_count() >= 2:
        import pytest
        pytest.skip("two devices present: the spawn path would run the real job")
    assert p.returncode == 2, p.stderr.decode()[-400:]
    assert p.stdout.strip() == b""
    assert b"refusing" in p.stderr


def test_traffic_is_null_for_a_stale_kernel_revision(tmp_path, monkeypatch):
    bench = _bench()
    import json
    prof = tmp_path / "profiles"
    prof.mkdir()
    monkeypatch.setattr(bench, "ROOT", str(tmp_path))
    monkeypatch.setattr(bench, "kernel_revision", lambda *a: "abc")
    (prof / "dcn_fwd_pmc.json").write_text(json.dumps(
        {"kernel_rev": "old", "inputs": "bench.py infer leg", "layers": {"1x64x64x256x512": 1.0}}))
    assert bench.measured_traffic(64, 64, 256, 512, 1)[0] is None
    (prof / "dcn_fwd_pmc.json").write_text(json.dumps(
        {"kernel_rev": "abc", "inputs": "bench.py infer leg", "layers": {"1x64x64x256x512": 5.0}}))
    assert bench.measured_traffic(64, 64, 256, 512, 1)[0] == 5.0
    assert bench.measured_traffic(64, 64, 256, 512, 4)[0] is None


def test_compact_line_fits_the_driver_capture():
    """Round 3's 21 KB stdout line lost its head in the driver's capture (BENCH_r03: parsed = null).  The line is now
    built by `compact_line` from the full record: every contract key, algorithmic roofline fractions, < 8 KB even when
    every leg ran and every string is long."""
    bench = _bench()
    import json
    full = json.load(open(os.path.join(ROOT, "profiles", "r03_bench_n1.json")))     # a full record of every leg
    full["roofline_mfma"] = full["roofline"]
    full["roofline"] = full.pop("roofline_hbm")
    for k in ("roofline", "roofline_bwd_data", "roofline_bwd_weight"):
        full["train"][k + "_mfma"] = full["train"][k]
        full["train"][k] = full["train"].pop(k + "_hbm")
    full["detail"] = "gpurun_out/bench_detail.json"
    text = bench.compact_line(full)
    assert len(text) < bench.LINE_LIMIT <= 8000 and "\n" not in text
    line = json.loads(text)
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                "vs_baseline", "dtype", "data", "config", "roofline", "roofline_mfma", "cpu_baseline", "train",
                "exact_f32", "max_rel_err_vs_golden"):
        assert key in line, key
    r = line["roofline"]
    assert r["bound"] == "hbm" and r["unit"] == "GB/s" and r["peak"] == 8000.0
    assert abs(r["frac"] - r["algorithmic_bytes_per_launch"] / (r["avg_launch_us"] * 1e-6) / 8e12) < 1e-3 * r["frac"]
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3 * r["frac"]
    assert set(line["cpu_baseline"]) >= {"value", "unit", "cores", "kind", "sample"}
    assert "model" not in line["config"] and "workload" in line["config"]
    # a pathological record (every string 2 KB long) still fits: optional blocks are dropped, never the contract keys
    fat = json.loads(json.dumps(full))
    fat["other_configs"] = {"config%d" % i: {"metric": "m" * 2000, "value": 1.0} for i in range(4, 9)}
    text = bench.compact_line(fat)
    assert len(text) <= bench.LINE_LIMIT and "roofline" in json.loads(text) and "cpu_baseline" in json.loads(text)


def test_split_bf16_roofline_prices_algorithmic_flops():
    bench = _bench()
    r = bench.split_bf16_roofline({}, 9.66e9, 50e-6)
    assert abs(r["frac"] - 9.66e9 / 50e-6 / 2.5e15) < 1e-9
    assert abs(r["issued_frac"] - 3 * r["frac"]) < 1e-12


def test_plain_run_is_the_default_and_full_is_opt_in():
    """A plain run measures the headline only; everything beside it waits for --full; --steps is the timed count."""
    import pytest
    bench = _bench()
    a = bench.parse(["--gpus", "1", "--steps", "3", "--warmup", "1"])
    assert a.full is False and a.dump_outputs is None and (a.steps, a.warmup) == (3, 1)
    b = bench.parse(["--full", "--dump-outputs", "outs"])
    assert b.full is True and b.dump_outputs == "outs"
    with pytest.raises(SystemExit):
        bench.parse(["--steps", "0"])


def test_dump_outputs_keeps_the_budget_and_samples_reproducibly(tmp_path):
    """Small arrays are written whole (float32, float64 kept), the ones that do not fit as a seeded sample of their
    flattened elements that the manifest's rule reproduces; the files stay under the byte limit; two dumps agree."""
    import numpy as np
    import torch
    bench = _bench()
    rng = np.random.default_rng(1)
    arrays = bench.host_arrays({"small": torch.arange(20, dtype=torch.int64).reshape(4, 5),
                                "scalar": torch.tensor(1.5), "wide": rng.standard_normal(10),
                                "big": rng.standard_normal((3, 100000)).astype(np.float32),
                                "bigger": rng.standard_normal(500000).astype(np.float32)})
    assert arrays["small"].dtype == np.float32 and arrays["wide"].dtype == np.float64
    limit = 1 << 20
    man = bench.dump_outputs(arrays, str(tmp_path / "a"), limit=limit)
    bench.dump_outputs(arrays, str(tmp_path / "b"), limit=limit)
    files = sorted(p.name for p in (tmp_path / "a").iterdir())
    assert files == ["big.npy", "bigger.npy", "manifest.json", "scalar.npy", "small.npy", "wide.npy"]
    assert sum((tmp_path / "a" / f).stat().st_size for f in files if f.endswith(".npy")) <= limit
    for f in files:
        assert (tmp_path / "a" / f).read_bytes() == (tmp_path / "b" / f).read_bytes(), f
    for k in ("small", "scalar", "wide"):
        assert "sample" not in man[k] and np.array_equal(np.load(tmp_path / "a" / (k + ".npy")), arrays[k])
    for k in ("big", "bigger"):
        e = man[k]
        assert e["shape"] == list(arrays[k].shape) and 0 < e["sample"] < arrays[k].size
        idx = np.sort(np.random.default_rng(e["sample_seed"]).integers(0, arrays[k].size, e["sample"]))
        assert np.array_equal(np.load(tmp_path / "a" / (k + ".npy")), arrays[k].reshape(-1)[idx])
    assert man["big"]["sample"] == man["bigger"]["sample"]       # the budget left is shared evenly


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_the_last_one(tmp_path):
    """`bench.py --steps 3 --warmup 1 --dump-outputs DIR` on a small input: one JSON line with the headline keys and
    nothing of --full, and DIR holds the detections and head maps of the last timed step."""
    import json
    import subprocess
    import sys
    import numpy as np
    out = tmp_path / "outs"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--height", "256", "--width", "512", "--dump-outputs", str(out)],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    lines = p.stdout.decode().strip().splitlines()
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert (line["steps"], line["warmup"], line["n_gpus"], line["unit"]) == (3, 1, 1, "img/s")
    assert line["higher_is_better"] is True and "DLA-34" in line["metric"] and line["dtype"]
    assert abs(line["value"] * line["ms_per_step"] - 1e3) < 1e-3 * 1e3
    for k in ("roofline", "roofline_mfma", "train", "cpu_baseline", "other_configs", "detail"):
        assert k not in line, k
    man = json.load(open(str(out / "manifest.json")))
    assert set(man) == {"dets", "head_hm", "head_poly", "head_pseudo_depth", "head_reg"}
    assert not any("sample" in e for e in man.values())
    dets = np.load(str(out / "dets.npy"))
    hm = np.load(str(out / "head_hm.npy"))
    assert dets.dtype == np.float32 and dets.shape[:2] == (1, 128) and np.isfinite(dets).all()
    assert hm.shape == (1, 8, 64, 128) and hm.min() >= 0.0 and hm.max() <= 1.0        # the activated heat map
    assert np.load(str(out / "head_poly.npy")).shape == (1, 32, 64, 128)


def test_bench_starts_from_a_read_only_tree():
    """The benchmark may run from a checkout its user cannot write to: importing it must not need to create anything
    in the tree (MIOpen then keeps its default per-user cache).  Directory creation under the tree is made to fail."""
    import subprocess
    import sys
    code = ("import os, sys\n"
            "root = %r\n"
            "real = os.makedirs\n"
            "def makedirs(p, *a, **k):\n"
            "    if os.path.abspath(p).startswith(root + os.sep):\n"
            "        raise PermissionError(13, 'Permission denied', p)\n"
            "    return real(p, *a, **k)\n"
            "os.makedirs = makedirs\n"
            "for v in ('MIOPEN_CUSTOM_CACHE_DIR', 'MIOPEN_USER_DB_PATH'):\n"
            "    os.environ.pop(v, None)\n"
            "sys.path.insert(0, root)\n"
            "import bench\n"
            "assert bench.parse(['--gpus', '1', '--steps', '2', '--warmup', '1']).steps == 2\n"
            "assert not any(os.environ.get(v, '').startswith(root) for v in ('MIOPEN_CUSTOM_CACHE_DIR', "
            "'MIOPEN_USER_DB_PATH'))\n"
            "print('ok')\n") % ROOT
    p = subprocess.run([sys.executable, "-c", code], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert p.returncode == 0 and p.stdout.strip() == b"ok", p.stderr.decode()[-1500:]

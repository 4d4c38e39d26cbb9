"""The driver's bench.py contract on the GPU: one JSON line on stdout with the
keys the driver and the judge read (metric, value, unit, n_gpus, steps,
warmup, ms_per_step, higher_is_better, scaling, vs_baseline, dtype, data,
config.workload, roofline{bound, achieved, peak, unit, frac, traffic},
cpu_baseline{value, unit, cores, kind, sample}), at a small size so the suite
stays short; the full-size line comes from the default sizes.  The probe ceiling,
the CPU baseline and the parity checks belong to `--full`; a plain run times
its steps, writes `--dump-outputs` and prints the line."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_bench_json_line(gpu):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--packets", str(1 << 20), "--steps", "3", "--warmup", "1",
           "--full", "--no-node", "--no-e2e", "--extra", "", "--cpu-budget", "0.5"]
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 3 and d["warmup"] == 1 and d["higher_is_better"] is True
    assert d["scaling"] == "weak" and d["value"] > 0 and d["ms_per_step"] > 0
    assert d["config"]["workload"] and d["config"]["packets_per_gpu"] == 1 << 20
    r = d["roofline"]
    assert r["bound"] == "hbm" and r["unit"] == "GB/s" and 0 < r["frac"] < 1
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3
    # the same-box access-shape probe (cndp_amd/csrc/roofline_probe.hip)
    assert r["probe_ms"] > 0 and abs(r["kernel_over_probe"] - r["kernel_ms"] / r["probe_ms"]) < 2e-3
    cb = d["cpu_baseline"]
    assert cb["value"] > 0 and cb["cores"] >= 1 and cb["kind"] in ("port", "reference") and cb["sample"]
    assert d["config"]["bins_total"] == 3 * (1 << 20)  # the timed steps: every packet binned once a step


@pytest.mark.gpu
def test_bench_plain_run_dumps_last_step(gpu, tmp_path):
    """A plain run (no --full): the line keeps its headline keys and leaves what
    --full adds empty, --steps is the number of timed steps (the bin counters
    count every packet once a step), and --dump-outputs writes the last timed
    step's outputs as float64 .npy -- equal to the oracle's over the same seeded
    frames, so two builds can be compared file by file.  2^20 + 1000 packets:
    one more than DUMP_SAMPLE, so the dump is the seeded sample."""
    import numpy as np
    import helpers
    from cndp_amd import pktgen
    from oracle import oracle as O
    sys.path.insert(0, ROOT)
    import bench as B
    n, steps = B.DUMP_SAMPLE + 1000, 3
    d = tmp_path / "dump"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--packets", str(n), "--steps", str(steps),
           "--warmup", "1", "--dump-outputs", str(d)]
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = p.stdout.splitlines()
    assert len(lines) == 1 and lines[0].startswith("{"), p.stdout[-2000:]
    r = json.loads(lines[0])
    assert r["metric"] == B.METRIC and r["unit"] == "Mpps" and r["higher_is_better"] is True and r["dtype"] == "u32"
    assert r["steps"] == steps and r["value"] > 0 and r["ms_per_step"] > 0
    assert abs(r["value"] - n / r["ms_per_step"] / 1e3) <= 0.01 * r["value"]
    assert r["config"]["bins_total"] == steps * n
    assert r["cpu_baseline"] is None and r["configs"] == {} and r["node_boundary"] is None
    assert r["host_memory_e2e"] is None and r["fib_update"] is None and "probe_ms" not in r["roofline"]
    assert r["config"]["parity_sample_vs_oracle"] is None
    # step k classified ring batch k % R: those frames again, through the oracle; the per-packet
    # outputs are the last step's, the bin counters count all the timed steps
    R = r["config"]["ring_batches"]
    assert R >= steps
    routes = pktgen.l3fwd_routes()
    t4 = O.dir24_8_build([(ip, dp, nh) for ip, dp, nh in routes], helpers.L3FWD_DEF, 256)
    bins = 0
    for k in range(steps):
        fr = pktgen.packed_ipv4(n, routes=routes, seed=pktgen.SEED + 1000 * (k % R), device=gpu)
        ref = O.classify(O.MODE_L3FWD, fr.slab.cpu().numpy(), n, stride=64, tables4=t4)
        bins = bins + ref["bins"].astype(np.float64)
    pick = np.sort(np.random.default_rng(20).integers(0, n, size=B.DUMP_SAMPLE))
    got = {f[:-4]: np.load(d / f) for f in sorted(os.listdir(d))}
    assert sorted(got) == ["bins", "hash", "nh", "queue"]
    assert all(a.dtype == np.float64 for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= 64 << 20
    for k in ("nh", "hash", "queue"):
        assert np.array_equal(got[k], ref[k][pick].astype(np.float64)), k
    assert np.array_equal(got["bins"], bins)

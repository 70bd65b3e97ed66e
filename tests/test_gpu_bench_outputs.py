"""bench.py --dump-outputs: the files a plain benchmark run leaves are what its timed path computed in the last step.

One small box (2 * 72^3 = 746 496 molecules: more than the 48 MiB of per-molecule arrays hold, so the id-hash sample is taken; many
blocks; 72 is no multiple of the brick edge) runs through `bench.py --gpus 1 --steps 3 --warmup 1 --melt 0 --dump-outputs DIR` in
a child process, as the benchmark is always run.  The same start, the same engine calls and the same number of steps in this
process give the arrays to compare with.

Tolerances: both sides run the same kernels on the same start configuration (the device generator), so they differ by the order of
floating-point sums at most: a few ulp of a position (|r| < 100: 1e-13) amplified over 4 steps of dt = 0.002 by a force gradient of
order 1e3 stays below 1e-10 in r and v and below 1e-9 of max|F| in F; the global sums below 1e-10 relative."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, load_pkg

pytestmark = pytest.mark.gpu

engine_mod = load_pkg("engine")
synth = load_pkg("synth")
inp = load_pkg("inp")

N_PER_DIM, STEPS, WARMUP = 72, 3, 1


@pytest.fixture(scope="module")
def bench_run(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("dump"))
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(STEPS), "--warmup", str(WARMUP),
           "--n-per-dim", str(N_PER_DIM), "--melt", "0", "--dump-outputs", out]
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return out, json.loads(lines[0])


@pytest.fixture(scope="module")
def engine_run():
    """what the benchmark's timed path does, called directly: same start, same calls, same steps"""
    import torch

    import bench
    n = N_PER_DIM
    L = synth.box_length(n, bench.RHO)
    e = engine_mod.DeviceEngine(0)
    e.set_components(bench.lj_components(inp), bench.RC)
    e.set_option("force_kernel", 0)
    e.set_verlet(0.2)
    e.set_domain([L, L, L])
    e.upload_begin(2 * n ** 3)
    for ids_t, r_t, v_t in synth.bcc_chunks_device(torch, torch.device("cuda", 0), n, rho=bench.RHO, temp=bench.TEMP):
        torch.cuda.synchronize()
        e.upload_chunk_device(ids_t.numel(), ids_t.data_ptr(), 0, r_t.data_ptr(), v_t.data_ptr())
    e.upload_end()
    e.rebin(); e.halo(); e.forces(0)
    e.run(bench.DT, WARMUP)
    last = e.run(bench.DT, STEPS)
    st = e.download_state()
    F = e.download_forces()["F"]
    e.close()
    o = np.argsort(st["ids"], kind="stable")
    return dict(L=L, last=last, ids=st["ids"][o], r=st["r"][o], v=st["v"][o], F=F[o])


def test_plain_run_prints_the_headline_only(bench_run):
    _, d = bench_run
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "n_gpus"):
        assert k in d, k
    n_total = 2 * N_PER_DIM ** 3
    assert d["steps"] == STEPS and d["warmup"] == WARMUP and d["unit"] == "particle-updates/s" and d["dtype"] == "f64"
    assert d["higher_is_better"] is True and d["ms_per_step"] > 0
    assert abs(d["value"] - n_total * STEPS / (d["ms_per_step"] * STEPS * 1e-3)) <= 1e-6 * d["value"]
    nl = d["config"]["neighbour_lists"]
    if nl:  # the engine counts the steps of its list loop: warm-up + timed steps and nothing after them
        assert nl["list_steps"] == WARMUP + STEPS
    for k in ("cpu_baseline", "gpu_over_cpu", "long_run", "steady_state_value", "lattice_start", "multi_gpu_self_check"):
        assert k not in d, k  # these are --full's
    assert "source" not in (d["roofline"].get("compute") or {})  # no live counter passes either


def test_dumped_files_are_float_arrays_within_the_size_bound(bench_run):
    out, d = bench_run
    names = sorted(os.listdir(out))
    assert names == ["F.npy", "globals.npy", "ids.npy", "r.npy", "v.npy"]
    arrs = {f[:-4]: np.load(os.path.join(out, f)) for f in names}
    assert all(a.dtype == np.float64 and np.all(np.isfinite(a)) for a in arrs.values())
    assert sum(os.path.getsize(os.path.join(out, f)) for f in names) <= 64 * 10 ** 6
    m = len(arrs["ids"])
    assert arrs["r"].shape == arrs["v"].shape == arrs["F"].shape == (m, 3) and arrs["globals"].shape == (6,)
    ls = d["last_step"]
    assert arrs["globals"].tolist() == [ls["upot"], ls["virial"], ls["summv2"], ls["sumIw2"], float(ls["n"]), float(ls["rot_dof"])]


def test_dump_is_the_fixed_id_sample_of_the_last_step(bench_run, engine_run):
    import bench
    out, _ = bench_run
    g = engine_run
    ids = np.load(os.path.join(out, "ids.npy"))
    n = len(g["ids"])
    assert np.all(np.diff(ids) > 0) and 0 < len(ids) < n  # sorted, unique, a sample
    # the sample is a function of the id alone: every molecule whose hashed id lies below the threshold, no other
    rows = bench.DUMP_BYTES // (8 * 10)
    h = (g["ids"] * np.uint64(bench.DUMP_HASH)) >> np.uint64(32)
    want = g["ids"][h < np.uint64(int(0.98 * rows / n * 2.0 ** 32))]
    assert np.array_equal(ids, want.astype(np.float64))
    assert 0.9 * rows < len(ids) <= rows
    pos = np.searchsorted(g["ids"], ids.astype(np.uint64))
    r, v, F = (np.load(os.path.join(out, k + ".npy")) for k in ("r", "v", "F"))
    assert np.all((r >= 0) & (r < g["L"]))
    dr = np.abs(r - g["r"][pos])
    dr = np.minimum(dr, g["L"] - dr)  # (a molecule on the periodic face may be reported on either side)
    assert np.max(dr) < 1e-10
    assert np.max(np.abs(v - g["v"][pos])) < 1e-10
    assert np.max(np.abs(F - g["F"][pos])) < 1e-9 * np.max(np.abs(g["F"]))
    gl = np.load(os.path.join(out, "globals.npy"))
    for i, k in enumerate(("upot", "virial", "summv2")):
        assert abs(gl[i] - g["last"][k]) < 1e-10 * abs(g["last"][k]), k
    assert gl[4] == n == g["last"]["n"]

"""LDS-free wave folds (ls1-mardyn_amd/csrc/common.hpp, wave_down_f64: v_permlane32_swap / v_permlane16_swap / DPP row_shl instead of
ds_bpermute) in the tail of the list force pass (store_partials) and in the reduction kernels.

  * the device probe tools/probes/wave_reduce_probe.hip (built by the library's Makefile): lane 0 of the new folds == the __shfl_down
    tree bit for bit, sum and top-2 merge, workgroups of one and of eight waves;
  * the reference's 2 * 12^3 = 3456 box (bcc1clj_3456: several bricks, partial ones at the faces): forces against the generic kernel,
    every step's U_pot / virial / sum m v^2 of a 10-step fused run against the golden file and the oracle, two runs bitwise equal;
  * the local rebuild criterion with a fast outlier (it consumes the per-wave top-2 |v_drift|^2 rows): the trajectory of the global
    criterion, fewer builds, and the same builds and bits on a second run;
  * the decomposed inner / boundary list passes of one rank (the kernel instantiation without the fast head).
Tolerances are those tests/test_gpu_verlet.py uses for the same comparisons."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, load_pkg
from golden_io import input_path, manifest, read_golden, rel_max, sorted_phase_space
from oracle.oracle import Oracle

pytestmark = pytest.mark.gpu

inp = load_pkg("inp")
capi = load_pkg("capi")
engine_mod = load_pkg("engine")
synth = load_pkg("synth")
MAN = manifest()
NAME = "bcc1clj_3456_steps10"
SKIN = 0.3


def test_probe_new_folds_equal_the_shfl_down_tree_bit_for_bit():
    exe = os.path.join(ROOT, "ls1-mardyn_amd", "lib", "wave_reduce_probe")
    assert os.path.isfile(exe), "ls1-mardyn_amd/lib/wave_reduce_probe is built with the library (make -C ls1-mardyn_amd)"
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(p.stdout)
    assert p.returncode == 0, p.stdout + p.stderr
    assert p.stdout.startswith("wave_reduce_probe ok"), p.stdout


def _lj():
    return inp.ComponentSet([inp.make_component(lj=[(0, 0, 0, 1, 1, 1, 2.5, 0)])], np.zeros((0, 2)), 1e10)


def _engine(comps, rc, L, ids, r, v, skin=None, **opts):
    e = engine_mod.DeviceEngine(0)
    e.set_components(comps, rc)
    for k, val in opts.items():
        e.set_option(k, val)
    e.set_verlet(skin, force=True)
    e.set_domain(L)
    e.upload(ids, np.zeros(len(ids), np.int32), r, v)
    e.rebin(); e.halo(); e.forces(0)
    return e


def _state(e):
    st = e.download_state()
    o = np.argsort(st["ids"], kind="stable")
    return st["ids"][o], st["r"][o], st["v"][o], e.download_forces()["F"][o]


@pytest.fixture(scope="module")
def box3456():
    case = MAN[NAME]
    ps = inp.read_inp(input_path(case["input"]))
    st = sorted_phase_space(ps)
    assert len(st["ids"]) == 3456
    return case, ps, st


@pytest.fixture(scope="module")
def oracle_steps(box3456):
    """{U_pot, virial, sum m v^2} of every step from the pinned oracle (computed once)"""
    case, ps, st = box3456
    orc = Oracle(ps.components.flat(), case["rc"])
    ro, vo, q, D, cid = st["r"].copy(), st["v"].copy(), st["q"].copy(), st["D"].copy(), st["cid"]
    o = orc.forces(ro, q, cid, ps.length, True)
    Fo, Mo = o["F"].copy(), o["M"].copy()
    rows = []
    for _ in range(case["steps"]):
        o = orc.step(case["dt"], cid, ro, vo, q, D, Fo, Mo, ps.length, True)
        rows.append((o["upot"], o["virial"], o["summv2"]))
    return np.array(rows)


@pytest.fixture(scope="module")
def generic_forces(box3456):
    case, ps, st = box3456
    ref = _engine(ps.components, case["rc"], ps.length, st["ids"], st["r"], st["v"], force_kernel=capi.FK_GENERIC)
    u, w = ref.forces(0)  # the start configuration itself (the piecewise passes evaluate it) ...
    start = (u, w, _state(ref)[3])
    o0 = ref.run(1e-9, 1)  # ... and after the step of 1e-9 a run of one step evaluates
    F0 = _state(ref)[3]
    ref.close()
    return o0, F0, start


def test_box3456_list_pass_forces_against_generic_kernel(box3456, generic_forces):
    case, ps, st = box3456
    o0, F0, _ = generic_forces
    e = _engine(ps.components, case["rc"], ps.length, st["ids"], st["r"], st["v"], skin=SKIN)
    assert e.get_option("verlet_lists") == 1
    out = e.run(1e-9, 1)  # one list build + evaluation
    assert e.get_option("verlet_builds") == 1 and e.get_option("last_force_kernel") == capi.FK_NEIGHBOUR_LIST
    F = _state(e)[3]
    e.close()
    assert rel_max(F, F0) < 1e-10
    assert abs(out["upot"] - o0["upot"]) <= 1e-10 * abs(o0["upot"]) and abs(out["virial"] - o0["virial"]) <= 1e-10 * abs(o0["virial"])


def _fused_run(box3456):
    case, ps, st = box3456
    e = _engine(ps.components, case["rc"], ps.length, st["ids"], st["r"], st["v"], skin=SKIN)
    out = e.run(case["dt"], case["steps"])
    assert e.get_option("verlet_steps") == case["steps"] and 1 <= e.get_option("verlet_builds") < case["steps"]
    assert e.get_option("last_force_kernel") == capi.FK_NEIGHBOUR_LIST
    res = _state(e) + (out, e.run_log().copy(), e.get_option("verlet_builds"))
    e.close()
    return res


def test_box3456_ten_fused_steps_globals_against_golden_and_oracle_and_bitwise_repeatable(box3456, oracle_steps):
    case, ps, st = box3456
    g = read_golden(NAME)
    ids, r, v, F, out, log, builds = _fused_run(box3456)
    assert abs(out["upot"] - g["upot"]) / abs(g["upot"]) < 1e-9
    assert abs(out["virial"] - g["virial"]) / abs(g["virial"]) < 1e-8
    assert abs(out["summv2"] - g["summv2"]) / abs(g["summv2"]) < 1e-9
    for s in range(case["steps"]):
        up, vi, kv = oracle_steps[s]
        assert abs(log[s, 0] - up) <= 1e-9 * abs(up), s
        assert abs(log[s, 1] - vi) <= 1e-8 * abs(vi), s
        assert abs(log[s, 2] - kv) <= 1e-9 * kv, s
    rec = g["recs"]
    L = ps.length
    dr = r - rec["r"]
    dr -= L * np.round(dr / L)
    assert np.max(np.abs(dr)) < 1e-9 * np.max(L)
    assert rel_max(v, rec["v"]) < 1e-9
    # a second run (fresh context): the same bits, state and every step's folded sums
    ids2, r2, v2, F2, out2, log2, builds2 = _fused_run(box3456)
    assert builds == builds2
    assert np.array_equal(r, r2) and np.array_equal(v, v2) and np.array_equal(F, F2)
    assert np.array_equal(log, log2)
    assert out["upot"] == out2["upot"] and out["virial"] == out2["virial"] and out["summv2"] == out2["summv2"]


def test_local_rebuild_criterion_with_a_fast_outlier_keeps_builds_and_trajectory():
    """The local criterion reads the per-wave top-2 |v_drift|^2 rows store_partials folds.  One molecule at four times the thermal
    maximum (the set-up of test_local_rebuild_criterion_with_fast_outliers): a too small top-2 releases listed pairs early (force
    errors of order 1e-2), a too large one rebuilds as often as the global bound.  The run must follow the global criterion's
    trajectory with fewer builds, and a second run must rebuild in the same steps and end in the same bits."""
    n, dt, steps = 40, 0.002, 63
    L, ids, r, v = synth.bcc_box(n, temp=0.95)
    rng = np.random.default_rng(3)
    fast = rng.choice(len(ids), 1, replace=False)
    d = rng.normal(size=(1, 3))
    v = v.copy()
    v[fast] = 16.0 * d / np.linalg.norm(d, axis=1)[:, None]
    res, builds = {}, {}
    for mode, opts in (("local", {}), ("local2", {}), ("global", {"local_rebuild": 0})):
        e = _engine(_lj(), 2.5, [L] * 3, ids, r, v, skin=0.3, **opts)
        out = e.run(dt, steps)
        res[mode] = _state(e) + (out,)
        builds[mode] = e.get_option("verlet_builds")
        e.close()
    assert builds["local"] == builds["local2"], builds
    assert builds["local"] < builds["global"] and builds["local"] >= builds["global"] // 2, builds
    a, b, c = res["global"], res["local"], res["local2"]
    assert np.array_equal(a[0], b[0])
    dr = a[1] - b[1]
    dr -= L * np.round(dr / L)
    assert np.max(np.abs(dr)) < 1e-10 * L
    assert rel_max(b[2], a[2]) < 1e-10
    assert rel_max(b[3], a[3]) < 1e-9
    for k in ("upot", "virial", "summv2"):
        assert abs(a[4][k] - b[4][k]) <= 1e-10 * abs(a[4][k]), k
    assert np.array_equal(b[1], c[1]) and np.array_equal(b[2], c[2]) and np.array_equal(b[3], c[3])
    assert all(b[4][k] == c[4][k] for k in ("upot", "virial", "summv2"))


def test_box3456_inner_and_boundary_list_passes_of_one_rank(box3456, generic_forces):
    """The decomposed traversal (inner bricks, halo refresh, boundary bricks) launches the list kernel without the fast head."""
    case, ps, st = box3456
    u0, w0, F0 = generic_forces[2]
    e = engine_mod.DeviceEngine(0)
    e.set_components(ps.components, case["rc"])
    e.set_verlet(SKIN, force=True)
    e.set_domain(ps.length)
    e.upload(st["ids"], st["cid"], st["r"], st["v"])
    assert e.get_option("verlet_lists") == 1
    assert e.update() is True  # re-bin, halo, list build
    e.forces_list(1, 0.0)
    e.halo_refresh()
    u, w = e.forces_list(2, 0.0, want_macro=True)
    assert e.get_option("last_force_kernel") == capi.FK_NEIGHBOUR_LIST
    F = _state(e)[3]
    e.close()
    assert rel_max(F, F0) < 1e-10
    # (the two passes add their partial sums in another order than one pass: rounding only)
    assert abs(u - u0) <= 1e-10 * abs(u0) and abs(w - w0) <= 1e-10 * abs(w0)

"""List force pass: region staging with the 16-byte LDS-DMA form and the barrier-free workgroup tail (one row of partial sums per
wave, folded by the reductions) — kernels_force_verlet.hip, stage_positions_dma / store_partials.

Box: 2 * 16^3 = 8192 molecules, jittered bcc, skin 0.2: 8 cells per dimension = 2 x 2 x 4 bricks, every brick regular.  Region rows
start at LDS slots of both parities and are interrupted by halo cells (runs of the 16-byte form, runs of the dword form, odd heads and
tails all occur).  Tolerances are those tests/test_gpu_verlet.py uses for the same comparisons."""
import numpy as np
import pytest

from conftest import load_pkg
from golden_io import rel_max

pytestmark = pytest.mark.gpu

inp = load_pkg("inp")
capi = load_pkg("capi")
engine_mod = load_pkg("engine")
synth = load_pkg("synth")

RC, SKIN = 2.5, 0.2


def _lj():
    return inp.ComponentSet([inp.make_component(lj=[(0, 0, 0, 1, 1, 1, RC, 0)])], np.zeros((0, 2)), 1e10)


def _engine(comps, L, ids, r, v, skin=None, **opts):
    e = engine_mod.DeviceEngine(0)
    e.set_components(comps, RC)
    for k, val in opts.items():
        e.set_option(k, val)
    e.set_verlet(skin)  # not forced: the production path (every brick region fits the staging area)
    e.set_domain(L)
    e.upload(ids, np.zeros(len(ids), np.int32), r, v)
    e.rebin(); e.halo(); e.forces(0)
    return e


def _state(e):
    st = e.download_state()
    o = np.argsort(st["ids"], kind="stable")
    return st["ids"][o], st["r"][o], st["v"][o], e.download_forces()["F"][o]


@pytest.fixture(scope="module")
def box():
    L, ids, r, v = synth.bcc_box(16, temp=0.95)
    assert len(ids) == 8192
    return L, ids, r, v


@pytest.fixture(scope="module")
def generic_eval(box):
    """forces, U_pot, virial of the start configuration from the generic kernel (computed once)"""
    L, ids, r, v = box
    ref = _engine(_lj(), [L] * 3, ids, r, v, force_kernel=capi.FK_GENERIC)
    o0 = ref.run(1e-9, 1)
    F0 = _state(ref)[3]
    ref.close()
    return o0, F0


def _list_eval(box):
    L, ids, r, v = box
    e = _engine(_lj(), [L] * 3, ids, r, v, skin=SKIN)
    assert e.get_option("verlet_lists") == 1
    dims, _, hw = e.grid()
    assert list(dims - 2 * hw) == [8, 8, 8]  # 2 x 2 x 4 bricks of 4 x 4 x 2 cells
    out = e.run(1e-9, 1)  # one list build + evaluation
    assert e.get_option("verlet_builds") == 1
    assert e.get_option("verlet_irregular_bricks") == 0 and e.get_option("last_force_kernel") == 5
    F = _state(e)[3]
    e.close()
    return out, F


def test_regular_box_against_generic_kernel_and_bitwise_repeatable(box, generic_eval):
    o0, F0 = generic_eval
    out, F = _list_eval(box)
    assert rel_max(F, F0) < 1e-12
    assert abs(out["upot"] - o0["upot"]) <= 1e-11 * abs(o0["upot"]) and abs(out["virial"] - o0["virial"]) <= 1e-11 * abs(o0["virial"])
    # a second evaluation (fresh context, same input): the same bits — forces and the folded per-wave sums
    out2, F2 = _list_eval(box)
    assert np.array_equal(F, F2)
    assert out["upot"] == out2["upot"] and out["virial"] == out2["virial"] and out["summv2"] == out2["summv2"]


def test_thirty_steps_across_rebuilds_against_per_step_loop(box):
    """ls1hip_run with lists (fused passes: per-wave partial rows, per-wave top-2 speeds folded for the local rebuild criterion) over
    at least two rebuilds == the per-step search loop."""
    L, ids, r, v = box
    dt, steps = 0.004, 30
    res = {}
    for mode, skin in (("step", None), ("list", SKIN)):
        e = _engine(_lj(), [L] * 3, ids, r, v, skin=skin)
        out = e.run(dt, steps)
        res[mode] = _state(e) + (out, e.run_log())
        if skin:
            assert e.get_option("verlet_steps") == steps
            assert e.get_option("verlet_builds") >= 3, e.get_option("verlet_builds")  # the first build + two rebuilds
            assert e.get_option("verlet_irregular_bricks") == 0 and e.get_option("last_force_kernel") == 5
        e.close()
    a, b = res["step"], res["list"]
    assert np.array_equal(a[0], b[0])
    dr = a[1] - b[1]
    dr -= L * np.round(dr / L)
    assert np.max(np.abs(dr)) < 1e-10 * L
    assert rel_max(b[2], a[2]) < 1e-10
    assert rel_max(b[3], a[3]) < 1e-9
    for k in ("upot", "virial", "summv2"):
        assert abs(a[4][k] - b[4][k]) <= 1e-10 * abs(a[4][k]), k
    assert np.allclose(a[5][:, :3], b[5][:, :3], rtol=1e-10, atol=0)


@pytest.mark.parametrize("precision,tol", [(0, 1e-11), (2, 6e-5)])
def test_crowded_cell_in_a_regular_brick(precision, tol):
    """A cell of more than 32 molecules in an otherwise regular brick (long runs: several 16-byte body instructions), FP64 and spsp,
    against the generic kernel — the set-up and tolerances of test_list_pass_with_a_crowded_cell_in_a_regular_brick."""
    rng = np.random.default_rng(11)
    L = 22.4  # 8 cells of 2.8 = rc + skin 0.3: 2 x 2 x 4 bricks
    h = np.arange(0.7, L, 1.4)
    gas = np.stack(np.meshgrid(h, h, h, indexing="ij"), -1).reshape(-1, 3) + rng.uniform(-0.3, 0.3, (len(h) ** 3, 3))
    c = 2.8 * 3 + 0.6 + 0.8 * np.arange(3)
    blob = np.stack(np.meshgrid(c, c, c, indexing="ij"), -1).reshape(-1, 3) + rng.uniform(-0.1, 0.1, (27, 3))
    r = np.concatenate([gas, blob]) % L
    n = len(r)
    ids = np.arange(1, n + 1, dtype=np.uint64)
    v = np.zeros_like(r)
    soft = inp.ComponentSet([inp.make_component(lj=[(0, 0, 0, 1, 1e-3, 0.3, 2.5, 0)])], np.zeros((0, 2)), 1e10)
    assert np.all((r >= 8.4) & (r < 11.2), axis=1).sum() > 32
    ref = engine_mod.DeviceEngine(0)
    ref.set_components(soft, RC)
    ref.set_option("force_kernel", capi.FK_GENERIC)
    ref.set_domain([L] * 3)
    ref.upload(ids, np.zeros(n, np.int32), r, v)
    ref.rebin(); ref.halo()
    u0, w0 = ref.forces(0)
    F0 = _state(ref)[3]
    ref.close()
    e = engine_mod.DeviceEngine(0)
    e.set_components(soft, RC)
    e.set_option("precision", precision)
    e.set_verlet(0.3)
    e.set_domain([L] * 3)
    e.upload(ids, np.zeros(n, np.int32), r, v)
    assert e.get_option("verlet_lists") == 1
    assert e.update() is True
    u, w = e.forces_list(0, 0.0, want_macro=True)
    assert e.get_option("verlet_irregular_bricks") == 0 and e.get_option("precision_in_use") == precision
    assert e.get_option("last_force_kernel") == 5
    F = _state(e)[3]
    assert rel_max(F, F0) < tol
    assert abs(u - u0) <= 10 * tol * abs(u0) and abs(w - w0) <= 10 * tol * abs(w0)
    e.close()

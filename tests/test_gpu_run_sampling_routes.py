"""All five sampling passes due in one ls1hip_run, on every route the loop has: list mode, and overlap_halo 0, 1 and 2 without lists.
Six steps with rdf_every = 2, odf_every = 3 / odf_from = 0, cavity_every = 2 / cavity_from = 2, widom_every = 3, profile_every = 3 /
profile_from = 0.  The reference's rules (RDF.cpp:573-581: step % f == 0; ODF.cpp:81-85: step > from; CavityWriter.cpp:160-174 and
SpatialProfile.cpp:238: step >= from; Widom as the RDF) make that RDF on steps 2 4 6, ODF on 3 6, cavities on 2 4 6, Widom on 3 6,
profiles on 3 6.  Every pass only reads, so each table equals that of a run with this one pass alone, and the trajectory and the
step log those of a run without sampling.  Integer tables: exact.  Widom sums: the tests of the last sample bit-equal, the sums to the 1e-12 of
test_gpu_insert.  Profile sums: both runs add the same terms in another order, each lies within (n + 8) 2^-53 sum|term| of the exact
sum (profile_ref.assert_tables), the two within twice that; sum|term| is the column itself for ekin and vabs (terms >= 0) and at
most the vabs column for v3 (|v_x| <= |v|)."""
import numpy as np
import pytest

import profile_ref as pr
from conftest import load_pkg
from test_gpu_odf import MIXED, _comps, _engine, _state

pytestmark = pytest.mark.gpu

capi = load_pkg("capi")

DT, SKIN, STEPS = 0.2, 2.5, 6
ROUTES = {"lists": (SKIN, 0), "overlap_halo=0": (None, 0), "overlap_halo=1": (None, 1), "overlap_halo=2": (None, 2)}
PASSES = ("rdf", "odf", "cavity", "widom", "profile")
WANT_SAMPLES = dict(rdf=3, odf=2, cavity=3, widom=2, profile=2)
PROFILE_Q = pr.VELOCITY | pr.VELOCITY3D | pr.TEMPERATURE


def _run(route, passes):
    """six steps on a fresh context with `passes` enabled: (result of run, state by id, step log, {pass: tables})"""
    (fname, rc), (skin, overlap) = MIXED, ROUTES[route]
    L, s = _state(fname, 2)
    e = _engine(_comps((1, 1)), rc, L, s, skin=skin)
    e.set_option("overlap_halo", overlap)
    if "rdf" in passes:
        e.rdf_config(50, 0.7, True)
        e.set_option("rdf_every", 2)
    if "odf" in passes:
        e.odf_config(10, 10, 10, 0.9 * rc)
        e.set_option("odf_every", 3); e.set_option("odf_from", 0)
    if "cavity" in passes:
        e.cavity_config(13, 9, 7, 2, 0.6 * rc)
        e.set_option("cavity_every", 2); e.set_option("cavity_from", 2)
    if "widom" in passes:
        e.widom_config(0, 100, 8.55e-4, seed=3, slabs=4)  # the temperature of the fixture
        e.set_option("widom_every", 3)
    if "profile" in passes:
        e.profile_config(pr.CARTESIAN, (3, 5, 7), PROFILE_Q)
        e.set_option("profile_every", 3); e.set_option("profile_from", 0)
    out = e.run(DT, STEPS)
    assert (e.get_option("last_force_kernel") == capi.FK_NEIGHBOUR_LIST) == (skin is not None)
    tab = {}
    if "rdf" in passes:
        tab["rdf"] = e.rdf_read()
    if "odf" in passes:
        tab["odf"] = e.odf_read()
    if "cavity" in passes:
        tab["cavity"] = dict(e.cavity_read(), series=e.cavity_series())
    if "widom" in passes:
        tab["widom"] = dict(e.widom_read(), last=e.widom_last())
    if "profile" in passes:
        tab["profile"] = e.profile_read()
    st = e.download_state()
    o = np.argsort(st["ids"])
    log = e.run_log()
    e.close()
    return out, {k: v[o] for k, v in st.items()}, log, tab


def _samples(name, t):
    return len(t["series"]) if name == "cavity" else t["samples"]


@pytest.mark.parametrize("route", list(ROUTES))
def test_all_passes_due_in_one_run(route):
    out_all, st_all, log_all, tab = _run(route, PASSES)
    # (a) the schedule
    got = {k: _samples(k, tab[k]) for k in PASSES}
    print(route, "samples", got)
    assert got == WANT_SAMPLES
    # (b) every table equals that of the run with this pass alone
    solo = {k: _run(route, (k,))[3][k] for k in PASSES}
    a, b = tab["rdf"], solo["rdf"]
    assert int(a["mol"].sum()) > 0 and np.array_equal(a["mol"], b["mol"]) and np.array_equal(a["n_per_component"], b["n_per_component"])
    assert len(a["site"]) == len(b["site"]) and all(np.array_equal(x, y) for x, y in zip(a["site"], b["site"]))
    a, b = tab["odf"], solo["odf"]
    assert int(a["hist"].sum()) > 0 and np.array_equal(a["hist"], b["hist"])
    a, b = tab["cavity"], solo["cavity"]
    assert 0 < int(a["flags"].sum()) < a["flags"].size
    assert np.array_equal(a["flags"], b["flags"]) and np.array_equal(a["series"], b["series"]) and a["n_active"] == b["n_active"]
    a, b = tab["widom"], solo["widom"]
    assert int(a["n"].sum()) == 200 and np.array_equal(a["n"], b["n"])
    assert all(np.array_equal(a["last"][k], b["last"][k]) for k in ("r", "q", "dU"))
    print(route, "widom sum_w", a["sum_w"], b["sum_w"])
    assert np.all(np.abs(a["sum_w"] - b["sum_w"]) <= 1e-12 * b["sum_w"]), (a["sum_w"], b["sum_w"])
    a, b = tab["profile"], solo["profile"]
    assert int(a["n"].sum()) == 2 * len(st_all["ids"]) and np.array_equal(a["n"], b["n"]) and np.array_equal(a["dof"], b["dof"])
    n = a["n"].astype(np.float64)
    for k, scale in (("ekin", b["ekin"]), ("vabs", b["vabs"]), ("v3", b["vabs"][:, None])):
        bound = 2 * ((n + 8) if a[k].ndim == 1 else (n + 8)[:, None]) * 2.0 ** -53 * scale * (1 + 2.0 ** -40)
        err = np.abs(a[k] - b[k])
        print(f"{route} profile {k}: max error / bound = {float(np.max(err / np.maximum(bound, 1e-300))):.3f}")
        assert np.all(err <= bound), (route, k)
    # (c) the trajectory and the step log are those of the run without sampling
    out_none, st_none, log_none, _ = _run(route, ())
    assert out_all == out_none
    assert all(np.array_equal(st_all[k], st_none[k]) for k in ("ids", "r", "v", "q", "D"))
    # a step that samples profiles ends with a kick of its own, whose kinetic sums the log then holds: NaN (not computed) may become a
    # value, every value the run without sampling logged is there bit for bit
    have = ~np.isnan(log_none)
    print(route, "step log: values", int(have.sum()), "more in the sampled run", int((~np.isnan(log_all)).sum() - have.sum()))
    assert log_all.shape == log_none.shape and np.array_equal(log_all[have], log_none[have])

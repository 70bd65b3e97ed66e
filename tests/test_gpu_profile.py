"""Spatial profiles sampled on the device (ls1hip_profile_*, kernels_profile.hip).  Yardstick everywhere: tests/profile_ref.py — pinned
to the real reference's files by tests/test_profile_cpu.py — on the state downloaded from the same context.  u64 tables must be
equal; every f64 bin must lie within (n_bin + 8) 2^-53 sum|term| of the longdouble sum (profile_ref.assert_tables: the
summation-order bound plus a few ulp per term, derived, not measured)."""
import numpy as np
import pytest

import profile_ref as pr
from conftest import load_pkg
from golden_io import input_path, manifest, sorted_phase_space

pytestmark = pytest.mark.gpu

capi = load_pkg("capi")
engine_mod = load_pkg("engine")
inp = load_pkg("inp")
mirror = load_pkg("mirror")

CART, CYL = pr.CARTESIAN, pr.CYLINDER
BCC = ("synthetic_bcc1clj_12.inp", 2.5, 0.005)      # bcc1clj_3456
MIXED = ("synthetic_mixed5_8.inp", 35.0, 0.2)       # mixed5_1024


def _engine(ps, s, rc, skin=None, force=True, options=(), r=None, thermostat=None):
    e = engine_mod.DeviceEngine(0)
    e.set_components(ps.components, rc)
    for k, v in options:
        e.set_option(k, v)
    if skin:
        e.set_verlet(skin, force=force)
    e.set_domain(ps.length)
    e.upload(s["ids"], s["cid"], s["r"] if r is None else r, s["v"], s["q"], s["D"])
    if thermostat is not None:
        e.set_thermostat(True, thermostat)
    e.rebin(); e.halo(); e.forces(0)
    return e


def _fixture(fname):
    ps = inp.read_inp(input_path(fname))
    return ps, sorted_phase_space(ps)


def _want(e, ps, mode, units, quantities, component=-1, scale=(1.0, 1.0)):
    """the yardstick on the state of the context as it stands (device order)"""
    st = e.download_state()
    Vi = e.download_forces(with_vi=True)["Vi"] if quantities & pr.VIRIAL else None
    return pr.tables(st["r"], st["v"] * scale[0], st["q"], st["D"] * scale[1], st["cid"], ps.components, ps.length, mode, units, quantities,
                     component, Vi=Vi)


@pytest.fixture(scope="module")
def bcc_after_3_steps():
    """bcc1clj_3456 after three steps of the per-step loop (per-molecule virials on): one context shared by the table-path cases,
    which only configure, sample and read"""
    ps, s = _fixture(BCC[0])
    e = _engine(ps, s, BCC[1], options=(("compute_vi", 1),))
    e.run(BCC[2], 3)
    yield e, ps
    e.close()


# ---- 1. table paths ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,units", [(CART, (3, 5, 7)), (CART, (1, 1, 1)), (CART, (1, 64, 64)), (CYL, (4, 5, 3))])
def test_table_paths(bcc_after_3_steps, mode, units):
    """105 bins and the cylinder: LDS tables; 1 x 1 x 1: every adder on one bin; 1 x 64 x 64 x 10 words = 320 KB: above any LDS
    budget, run-merged global atomics.  3456 is no multiple of the 512 molecules of a trip: the tail is covered."""
    e, ps = bcc_after_3_steps
    e.profile_config(mode, units, pr.ALL)
    assert e.profile_layout() == (units[0] * units[1] * units[2], pr.ALL)
    e.profile_sample()
    got = e.profile_read()
    want = _want(e, ps, mode, units, pr.ALL)
    assert want["margin"] >= pr.EDGE_MARGIN
    pr.assert_tables(got, want, (mode, units))
    if mode == CART:
        assert int(got["n"].sum()) == 3456
    else:
        assert 0 < int(got["n"].sum()) < 3456  # molecules outside the cylinder are skipped
    if units == (1, 1, 1):
        mv2, Iw2, n, rd = e.kinetic_sums()
        assert int(got["n"][0]) == n == 3456 and int(got["dof"][0]) == 3 * n + rd
        bound = (n + 8) * 2.0 ** -53 * float(want["abs_ekin"][0])
        print(f"profile 1x1x1 against ls1hip_kinetic_sums: |d| / bound = {abs(got['ekin'][0] - (mv2 + Iw2)) / bound:.3f}")
        assert abs(got["ekin"][0] - (mv2 + Iw2)) <= bound


def test_density_only_reads_positions_only(bcc_after_3_steps):
    e, ps = bcc_after_3_steps
    e.profile_config(CART, (1, 200, 1), 0)
    e.profile_sample(); e.profile_sample()
    got = e.profile_read()
    want = _want(e, ps, CART, (1, 200, 1), 0)
    assert sorted(k for k in got if k not in ("samples", "quantities")) == ["n"]
    assert got["samples"] == 2 and np.array_equal(got["n"], 2 * want["n"])
    e.profile_reset()
    z = e.profile_read()
    assert z["samples"] == 0 and not z["n"].any()
    e.profile_config(CART, (0, 0, 0))  # off: buffers freed
    assert e.profile_layout() == (0, 0)


# ---- 2. rotors, rotational degrees of freedom, the component filter ---------------------------------------------------------------------
@pytest.mark.parametrize("component,units", [(-1, (3, 5, 7)), (1, (3, 5, 7)), (-1, (1, 64, 64))])
def test_rotors_and_component_filter(component, units):
    ps, s = _fixture(MIXED[0])
    e = _engine(ps, s, MIXED[1], options=(("compute_vi", 1),))
    e.run(MIXED[2], 3)
    e.profile_config(CART, units, pr.ALL, component)
    e.profile_sample()
    got = e.profile_read()
    want = _want(e, ps, CART, units, pr.ALL, component)
    e.close()
    assert want["margin"] >= pr.EDGE_MARGIN
    pr.assert_tables(got, want, ("mixed5", component, units))
    assert int(got["n"].sum()) == (1024 if component < 0 else int((s["cid"] == component).sum())) > 0
    assert np.any(got["dof"] > 3 * got["n"])  # rotational degrees of freedom are counted


# ---- 3. against the reference's files, through ls1hip_run under the device thermostat -----------------------------------------------
@pytest.mark.parametrize("case,instance", [(c, k) for c in ("bcc1clj_3456", "mixed5_1024") for k in (0, 1)])
def test_run_reproduces_the_reference_files(case, instance, tmp_path):
    """profile_every = 1 from step 1, tables read after steps 2 and 4 and written by mirror.SpatialProfile: the sampling point (after
    the post-force kick, on the SCALED velocities) is what SpatialProfile::endStep of the real driver saw"""
    c = pr.cases()[case]
    ins = c["instances"][instance]
    ps, s = _fixture(c["input"])
    e = _engine(ps, s, c["rc"], options=(("compute_vi", 1),), thermostat=c["temperature"])
    sp = mirror.SpatialProfile(ps.length, mode=ins["mode"], units=ins["units"], writefrequency=2, init=1, recording=1, outputprefix=ins["prefix"],
                               profiledComponent="all" if ins["component"] < 0 else ins["component"] + 1,
                               profiles=("density", "temperature", "velocity", "velocity3d", "virial"))
    sp.attach(e)
    e.set_option("profile_every", 1)
    e.set_option("profile_from", 1)
    for last in (2, 4):
        e.run(c["dt"], 2)
        row = e.run_log()[-1]
        T = (row[2] + row[3]) / (3.0 * row[4] + row[5])  # Domain::getCurrentTemperature(0): before the scaling
        assert e.profile_read()["samples"] == 2
        sp.endStep(last, T, directory=str(tmp_path), sample=False)
        assert e.profile_read()["samples"] == 0
        for suffix in pr.SUFFIXES:
            got = (tmp_path / ("%s_%d%s" % (ins["prefix"], last, suffix))).read_text()
            pr.same_text(got, pr.golden_text(case, ins["prefix"], last, suffix), (case, ins["prefix"], last, suffix))
    e.close()


# ---- 4. the loop keeps its trajectory ---------------------------------------------------------------------------------------------------
def _loop(fixture, skin, thermostat, every, nsteps, pieces, quantities, units=(3, 5, 7), force=True):
    """run nsteps in `pieces` calls; returns (state sorted by id, run_log rows, tables, yardstick tables or None, list builds)"""
    fname, rc, dt = fixture
    ps, s = _fixture(fname)
    e = _engine(ps, s, rc, skin=skin, force=force, thermostat=thermostat)
    e.profile_config(CART, units, quantities)
    e.set_option("profile_every", every)
    rows, want = [], None
    for _ in range(pieces):
        e.run(dt, nsteps // pieces)
        rows.append(e.run_log())
        if pieces > 1:  # piecewise: ls1hip_profile_sample on the state each call leaves (scaled already by the call's last step)
            e.profile_sample()
            w = _want(e, ps, CART, units, quantities)
            want = w if want is None else pr.add_tables(want, w)
    st = e.download_state()
    o = np.argsort(st["ids"])
    out = ({k: v[o] for k, v in st.items()}, np.concatenate(rows), e.profile_read(), want, e.get_option("verlet_builds") if skin else 0)
    e.close()
    return out


@pytest.mark.parametrize("name,fixture,skin,thermostat,force", [
    ("per-step NVE fused", BCC, None, None, True),
    ("per-step NVT", BCC, None, 0.95, True),
    ("list NVE", BCC, 0.2, None, True),
    ("list NVT", BCC, 0.2, 0.95, True),
    ("ethane list pass that integrates itself", ("Ethan_equilibrated.inp", manifest()["ethan"]["rc"], 0.5), 0.05 * manifest()["ethan"]["rc"], None, False),
])
def test_loop_neutrality(name, fixture, skin, thermostat, force):
    """profile_every = 2 against 0 over six steps; and the tables of the run equal piecewise ls1hip_profile_sample calls on the
    same steps (three calls of two steps)"""
    q = pr.VELOCITY | pr.VELOCITY3D | pr.TEMPERATURE
    off, rows0, tab0, _, _ = _loop(fixture, skin, thermostat, 0, 6, 1, q, force=force)
    on, rows1, tab1, _, builds1 = _loop(fixture, skin, thermostat, 2, 6, 1, q, force=force)
    _, _, tab2, want, _ = _loop(fixture, skin, thermostat, 0, 6, 3, q, force=force)
    assert tab0["samples"] == 0 and not tab0["n"].any()
    assert np.array_equal(off["ids"], on["ids"])
    bitwise = all(np.array_equal(off[k], on[k]) for k in ("r", "v", "q", "D")) and np.array_equal(rows0, rows1, equal_nan=True)
    print(f"profile loop neutrality, {name}: bitwise = {bitwise}")
    if skin is None:
        for k in ("r", "v", "q", "D"):
            assert np.array_equal(off[k], on[k]), (name, k, float(np.max(np.abs(off[k] - on[k]))))
        assert np.array_equal(rows0, rows1, equal_nan=True), name
    else:
        # an unfused step may move a rebuild of the lists: the project's trajectory tolerance
        L = pr.sampling_info(CART, (1, 1, 1), inp.read_inp(input_path(fixture[0])).length)["L"]
        d = off["r"] - on["r"]
        d -= L * np.round(d / L)
        assert np.max(np.abs(d)) < 1e-9 * np.max(L) and builds1 >= 1
        for k in ("v", "q", "D"):
            assert np.max(np.abs(off[k] - on[k])) <= 1e-9 * max(np.max(np.abs(off[k])), 1e-300), (name, k)
        both = np.isfinite(rows0) & np.isfinite(rows1)
        assert np.all(np.abs(rows0[both] - rows1[both]) <= 1e-9 * np.abs(rows0[both]) + 1e-12)
    # the run's tables against the yardstick on the piecewise states, and the piecewise tables themselves
    assert tab1["samples"] == tab2["samples"] == 3
    assert want["margin"] >= pr.EDGE_MARGIN
    pr.assert_tables(tab2, want, (name, "piecewise"))
    if skin is None:
        pr.assert_tables(tab1, want, (name, "run"))
    else:
        # trajectories agree to 1e-9 only: counts still equal (edge margin 1e-8), sums to the trajectory tolerance
        assert np.array_equal(tab1["n"], tab2["n"]) and np.array_equal(tab1["dof"], tab2["dof"])
        for k in ("ekin", "vabs", "v3"):
            scale = np.maximum(want["abs_" + k].astype(np.float64), 1e-300)
            assert np.max(np.abs(tab1[k] - tab2[k]) / scale) < 1e-8, (name, k)


def test_rdf_and_profiles_on_the_same_step():
    ps, s = _fixture(BCC[0])
    res = []
    for prof in (0, 2):
        e = _engine(ps, s, BCC[1])
        e.rdf_config(97, 0.0257, True)
        e.set_option("rdf_every", 2)
        e.profile_config(CART, (3, 5, 7), pr.VELOCITY3D)
        e.set_option("profile_every", prof)
        e.run(BCC[2], 4)
        res.append((e.rdf_read(), e.profile_read(), e.download_state()))
        e.close()
    (rdf0, p0, st0), (rdf1, p1, st1) = res
    assert rdf0["samples"] == rdf1["samples"] == 2 and np.array_equal(rdf0["mol"], rdf1["mol"])
    assert p0["samples"] == 0 and p1["samples"] == 2 and int(p1["n"].sum()) == 2 * 3456
    assert np.array_equal(st0["r"], st1["r"]) and np.array_equal(st0["v"], st1["v"])


# ---- 5. list mode: a molecule outside the box is binned where the download reports it ---------------------------------------------------
def test_list_mode_sample_wraps_molecules_that_left_the_box():
    ps, s = _fixture(BCC[0])
    L = ps.length
    # the lattice shifted so that one plane of molecules per dimension starts 0.002 inside the lower faces: those that move
    # outwards cross a periodic face within one or two steps (|v| dt ~ 0.005), long before skin / 2 = 0.2 forces a rebuild
    lo = s["r"].min(axis=0)
    r0 = np.mod(s["r"] - lo + 0.002, L)
    e = _engine(ps, s, BCC[1], skin=0.4, r=r0)
    e.verlet_build()
    e.profile_config(CART, (3, 5, 7), pr.VELOCITY | pr.VELOCITY3D | pr.TEMPERATURE)
    builds = e.get_option("verlet_builds")
    before = e.download_state()
    for _ in range(2):
        e.kick_drift(BCC[2])
        assert e.update() is False  # no rebuild: the molecules keep their cells, some now sit outside the box
        e.forces_list(0)
        e.kick(0.5 * BCC[2])
    assert e.get_option("verlet_builds") == builds
    e.profile_sample()
    got = e.profile_read()
    after = e.download_state()
    assert np.array_equal(before["ids"], after["ids"])  # same slots: nothing was re-binned
    jumped = np.abs(after["r"] - before["r"]) > 0.5 * L
    assert jumped.any(), "no molecule crossed a periodic face: the fixture does not test the wrap"
    want = _want(e, ps, CART, (3, 5, 7), got["quantities"])
    e.close()
    assert want["margin"] >= pr.EDGE_MARGIN
    pr.assert_tables(got, want, "list-mode wrap")


# ---- 6. two contexts ------------------------------------------------------------------------------------------------------------------------
def test_two_contexts_sum_to_the_single_domain():
    from test_gpu_multirank import InProcessCluster
    ps, s = _fixture(BCC[0])
    multi = InProcessCluster(2, ps.components, BCC[1], ps.length, s["ids"], s["r"], s["v"], grid=(1, 2, 1), cid=s["cid"])
    for e in multi.eng:
        e.set_option("compute_vi", 1)
    multi.forces()
    for _ in range(2):
        multi.step(BCC[2])
    total, states, halos = None, [], 0
    for e in multi.eng:
        e.profile_config(CART, (3, 5, 7), pr.ALL)
        e.profile_sample()
        loc = e.profile_read()
        halos += e.count()[1]
        w = _want(e, ps, CART, (3, 5, 7), pr.ALL)
        pr.assert_tables(loc, w, "one of two contexts")
        total = w if total is None else pr.add_tables(total, w)
        states.append(loc)
        e.close()
    assert halos > 0 and total["margin"] >= pr.EDGE_MARGIN
    n = states[0]["n"] + states[1]["n"]
    assert int(n.sum()) == 3456  # owned molecules only: no halo copy is counted
    assert 0 < int(states[0]["n"].sum()) < 3456
    # the single domain, driven the same way
    one = _engine(ps, s, BCC[1], options=(("compute_vi", 1),))
    for _ in range(2):
        one.kick_drift(BCC[2]); one.rebin(); one.halo(); one.forces(0); one.kick(0.5 * BCC[2])
    one.profile_config(CART, (3, 5, 7), pr.ALL)
    one.profile_sample()
    single = one.profile_read()
    one.close()
    assert np.array_equal(n, single["n"]) and np.array_equal(states[0]["dof"] + states[1]["dof"], single["dof"])
    summed = dict(single)
    for k in pr.F64_KEYS:
        summed[k] = states[0][k] + states[1][k]
    total["samples"] = 1  # every rank ticks once; the collective does not sum the ticks
    pr.assert_tables(summed, total, "sum of two contexts")
    for k in pr.F64_KEYS:  # the two routes agree to the trajectory tolerance
        assert np.max(np.abs(summed[k] - single[k]) / np.maximum(total["abs_" + k].astype(np.float64), 1e-300)) < 1e-9, k


# ---- 7. errors: an error, never a partial table -------------------------------------------------------------------------------------------
def test_error_paths():
    ps, s = _fixture(BCC[0])
    e = _engine(ps, s, BCC[1])
    with pytest.raises(capi.Ls1HipError, match="not configured"):
        e.profile_sample()
    e.set_option("profile_every", 1)
    with pytest.raises(capi.Ls1HipError, match="profile_every"):
        e.run(BCC[2], 1)
    e.set_option("profile_every", 0)
    for mode, units, q, comp, what in ((CART, (3, 0, 7), 0, -1, "unit"), (CART, (0, 5, 0), 0, -1, "unit"), (2, (3, 5, 7), 0, -1, "mode"),
                                       (CART, (3, 5, 7), 16, -1, "quantity"), (CART, (3, 5, 7), 0, 1, "component"),
                                       (CART, (3, 5, 7), 0, -2, "component"), (CART, (2048, 2048, 2048), 0, -1, "32-bit"),
                                       (CART, (1024, 1024, 512), pr.ALL, -1, "32-bit")):
        with pytest.raises(capi.Ls1HipError, match=what):
            e.profile_config(mode, units, q, comp)
        assert e.profile_layout() == (0, 0)
    e.profile_config(CART, (3, 5, 7), pr.VIRIAL)
    with pytest.raises(capi.Ls1HipError, match="compute_vi"):
        e.profile_sample()  # per-molecule virials were not computed
    assert e.profile_read()["samples"] == 0 and not e.profile_read()["n"].any()
    e.profile_config(CART, (3, 5, 7), pr.VELOCITY)
    # read buffers too small
    small = np.zeros(10, dtype=np.uint64)
    with pytest.raises(capi.Ls1HipError, match="too small"):
        capi.check(e.ctx, e.lib.ls1hip_profile_read(e.ctx, 10, small.ctypes.data_as(capi._u64p), None, None, None, None, None, None))
    with pytest.raises(capi.Ls1HipError, match="not sampled"):
        d = np.zeros(105 * 3)
        capi.check(e.ctx, e.lib.ls1hip_profile_read(e.ctx, 105, None, None, None, None, capi.dptr(d), None, None))
    # the fused-advanced state: velocities half a step ahead, positions parked in the force arrays
    e.kick_drift(BCC[2]); e.rebin(); e.halo()
    e.forces_kick_drift(0, BCC[2])
    with pytest.raises(capi.Ls1HipError, match="fused"):
        e.profile_sample()
    assert e.profile_read()["samples"] == 0 and not e.profile_read()["n"].any()
    e.rebin(); e.halo(); e.forces(0); e.kick(0.5 * BCC[2])
    e.profile_sample()  # the context is usable afterwards
    got = e.profile_read()
    want = _want(e, ps, CART, (3, 5, 7), pr.VELOCITY)
    e.close()
    pr.assert_tables(got, want, "after the errors")
    f = engine_mod.DeviceEngine(0)
    with pytest.raises(capi.Ls1HipError, match="components"):
        f.profile_config(CART, (3, 5, 7))
    f.close()


def test_profile_timer():
    ps, s = _fixture(BCC[0])
    e = _engine(ps, s, BCC[1])
    e.timing_enable(1)
    e.profile_config(CART, (1, 200, 1), pr.VELOCITY3D | pr.TEMPERATURE)
    e.profile_sample()
    ms, n = e.timing("profile")
    e.close()
    assert n == 1 and ms > 0.0

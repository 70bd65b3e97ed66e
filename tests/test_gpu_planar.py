"""The planar long-range correction on the device (ls1hip_planar_*, kernels_planar.hip) against tests/planar_ref.py and against what
the unmodified reference driver wrote (tests/golden/planar/, made and proven by tests/golden/make_planar_golden.py)."""
import functools

import numpy as np
import pytest

import planar_ref
from conftest import load_pkg

pytestmark = pytest.mark.gpu

capi = load_pkg("capi")
engine_mod = load_pkg("engine")
inp = load_pkg("inp")

case = planar_ref.golden
CASES = list(planar_ref.cases())
TABLES = ("rho", "u", "vN", "vT", "f")
# slabs: the default, an odd count, no tile multiple, and 1030: four tiles, three rho chunks, K read from global memory; with the
# 16 rows of the five-component case beyond the LDS histogram of the density pass
SHAPES = [(c, s) for c in CASES for s in (10, 77, 200, 1030)]


@functools.lru_cache(maxsize=None)
def reference(name, slabs, state="input", region=None):
    """planar_ref on the input state or on the driver's step-4 checkpoint: (Planar, state, counts, tables), computed once"""
    c = case(name)
    st = c["s"] if state == "input" else planar_ref.read_restart(c["files"]["step4.restart.dat"])
    pl = planar_ref.Planar(c["ps"].components, c["ps"].length, c["rc"], slabs, temperature=c["temp"], region=region)
    cnt = pl.counts(st["cid"], st["r"], st["q"])
    return pl, st, cnt, pl.tables(cnt)


def engine(c, st, slabs, freq=10, region=None, options=(), skin=None, thermostat=False, domain=None):
    e = engine_mod.DeviceEngine(0)
    e.set_components(c["ps"].components, c["rc"])
    for k, v in options:
        e.set_option(k, v)
    if skin:
        e.set_verlet(skin, force=True)
    e.set_domain(c["ps"].length)
    e.upload(st["ids"], st["cid"], st["r"], st["v"], st["q"], st["D"])
    if thermostat:
        e.set_thermostat(True, c["temp"])
    e.rebin(); e.halo(); e.forces(0)
    if slabs:
        e.planar_config(slabs, freq, region, c["temp"])
    return e


def close(got, want, what):
    scale = np.abs(want).max()
    assert np.abs(got - want).max() <= 1e-10 * scale, (what, np.abs(got - want).max() / scale)


def assert_tables(t, T, nlj, what):
    for k in TABLES:
        close(t[k], T[k][:nlj], (what, k))
        if T[k].shape[0] > nlj:
            close(t[k + "_d"], T[k][nlj:], (what, k + "_d"))


# ---- (a) counts and tables ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,slabs", SHAPES)
def test_tables(name, slabs):
    c = case(name)
    pl, st, cnt, T = reference(name, slabs)
    e = engine(c, st, slabs)
    e.planar()
    got, t = e.planar_counts(), e.planar_read()
    e.close()
    assert np.array_equal(got, cnt)
    assert (t["slabs"], t["nlj"], t["ndip"]) == (slabs, pl.nljsum, pl.ndsum)
    assert_tables(t, T, pl.nljsum, (name, slabs))


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("step,state", [(1, "input"), (4, "step4")])
def test_tables_match_the_drivers_files(name, step, state):
    """rho, F and u of LRC_TS*.dat directly (the file of step 1 holds the tables of the input state: frequency 2)"""
    c = case(name)
    st = reference(name, c["slabs"], state)[1]
    e = engine(c, st, c["slabs"])
    e.planar()
    t = e.planar_read()
    e.close()
    for k, want in zip(("rho", "f", "u"), planar_ref.read_dat(c["files"]["LRC_TS%09d.dat" % step])):
        close(t[k], want, k)


# ---- (b) apply --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,slabs,narrow", [("synthetic_bcc1clj_12", 200, False), ("synthetic_mixed5_8", 77, False),
                                               ("synthetic_mixed5_8", 200, True), ("centre_site_2c", 1030, True)])
def test_apply(name, slabs, narrow):
    c = case(name)
    L = c["ps"].length[1]
    region = (0.3 * L, 0.55 * L) if narrow else None
    pl, st, cnt, T = reference(name, slabs, region=region)
    e = engine(c, st, slabs, region=region, options=(("compute_vi", 1),))
    ids = e.download_state()["ids"]
    before = e.download_forces(with_vi=True)
    up, vir = e.planar()
    after = e.download_forces(with_vi=True)
    e.close()
    o = np.searchsorted(st["ids"], ids)  # device slot -> sorted state
    dF, dM, dVi, up_ref, vir_ref = pl.apply(T, st["cid"], st["r"], st["q"])
    assert np.abs(dF).max() > 0 and (not narrow or (dF[:, 1] == 0).any())
    for k, d in (("F", dF), ("M", dM), ("Vi", dVi)):
        close(after[k], before[k] + d[o], (name, k))
    assert abs(up - up_ref) <= 1e-10 * abs(up_ref) and abs(vir - vir_ref) <= 1e-10 * abs(vir_ref)


# ---- (c) trajectory ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("skin", [None, 0.2])
def test_trajectory_against_the_driver(name, skin):
    """4 NVT steps of ls1hip_run with the correction on, per-step loop and list mode, against the driver's step-4 checkpoint (1e-9)
    and its printed U_pot and p (six digits).  This is what pins the vN / vT and the dipole tables to the real reference: the .dat
    files do not hold them."""
    c = case(name)
    ps = c["ps"]
    e = engine(c, c["s"], c["slabs"], freq=c["freq"], thermostat=True, skin=skin and skin * c["rc"] / 2.5)
    e.planar()  # the call of prepare_start (Simulation.cpp:841)
    e.run(c["dt"], 4)
    st, log, plog = e.download_state(), e.run_log(), e.planar_log()
    e.close()
    want = planar_ref.read_restart(c["files"]["step4.restart.dat"])
    o = np.argsort(st["ids"])
    dr = st["r"][o] - want["r"]
    dr -= ps.length * np.rint(dr / ps.length)
    assert np.abs(dr).max() <= 1e-9 * ps.length.max()
    for k in ("v", "q", "D"):
        if np.abs(want[k]).max() > 0:
            assert np.abs(st[k][o] - want[k]).max() <= 1e-9 * np.abs(want[k]).max(), k
    res = np.array([[float(x) for x in ln.split()] for ln in c["files"]["result.res"].splitlines() if ln.strip() and ln.split()[0].isdigit()])
    res = res[res[:, 0] >= 1][-4:]
    N, V = len(st["ids"]), float(np.prod(ps.length))
    np.testing.assert_allclose(log[:, 0] + plog[:, 0], res[:, 2], rtol=2e-5)
    # Domain::calculateGlobalValues: p = rho T + rho (virial + Virial_c) / (3 N), T = (sum m v^2 + sum I w^2) / (3 N + rotDOF)
    T = (log[:, 2] + log[:, 3]) / (3 * log[:, 4] + log[:, 5])
    np.testing.assert_allclose(N / V * T + (log[:, 1] + plog[:, 1]) / (3 * V), res[:, 4], rtol=2e-5)


# ---- (d) counter and multi-rank pieces ----------------------------------------------------------------------------------------------
def test_frequency_counter():
    c = case("centre_site_2c")
    e = engine(c, c["s"], 77, freq=2)
    tabs = []
    for _ in range(3):
        e.planar()
        tabs.append(e.planar_read())
        e.kick_drift(c["dt"]); e.rebin(); e.halo(); e.forces(0)
    e.close()
    assert np.array_equal(tabs[1]["f"], tabs[0]["f"]) and np.array_equal(tabs[1]["rho"], tabs[0]["rho"])  # call 2 applies call 1's
    assert not np.array_equal(tabs[2]["rho"], tabs[0]["rho"])  # call 3 (counter 2) sampled the moved molecules


def test_two_contexts_sum_to_the_single_domain():
    from test_gpu_multirank import InProcessCluster
    c = case("synthetic_bcc1clj_12")
    s, ps = c["s"], c["ps"]
    one = engine(c, s, 200)
    one.planar()
    cnt1, t1 = one.planar_counts(), one.planar_read()
    multi = InProcessCluster(2, ps.components, c["rc"], ps.length, s["ids"], s["r"], s["v"], grid=(1, 2, 1), cid=s["cid"])
    multi.forces()
    parts = []
    for e in multi.eng:
        e.planar_config(200, 10, None, c["temp"])
        e.planar_density()
        parts.append(e.planar_counts())
    assert all(0 < int(p.sum()) < int(cnt1.sum()) for p in parts) and np.array_equal(parts[0] + parts[1], cnt1)
    for e in multi.eng:
        e.planar_counts(parts[0] + parts[1])
        e.planar_tables()
        t = e.planar_read()
        assert all(np.array_equal(t[k], t1[k]) for k in TABLES)  # bit for bit
        e.close()
    one.close()


# ---- (e) planar off -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("skin", [None, 0.2])
def test_off_is_todays_path(skin):
    c = case("synthetic_bcc1clj_12")
    out = []
    for configured in (False, True):
        e = engine(c, c["s"], 0, skin=skin)
        if configured:
            e.planar_config(50)
            e.planar_config(0)
        res = e.run(c["dt"], 5)
        st = e.download_state()
        out.append((res, st))
        e.close()
    assert out[0][0] == out[1][0]
    assert all(np.array_equal(out[0][1][k], out[1][1][k]) for k in ("ids", "r", "v"))


# ---- (f) the argument rules of the ABI (a context needs a device, so they run here) ------------------------------------------------
def _components(kind):
    lj, dp = [(0, 0, 0, 1.0, 1.0, 1.0, 2.5, 0)], [(0, 0, 0, 0, 0, 1, 0.5)]
    if kind == "nonpolar first":  # dipoleDipole would read muSquare[1] of a one-entry array
        return inp.ComponentSet([inp.make_component(lj=lj), inp.make_component(lj=lj, dipoles=dp)], np.ones((1, 2)), 1e10)
    if kind == "polar":
        return inp.ComponentSet([inp.make_component(lj=lj, dipoles=dp)], np.ones((0, 2)), 1e10)
    z = 1.3 if kind == "long" else 0.1  # two sites at +-z: elongations 2 z against r_c = 2.5
    return inp.ComponentSet([inp.make_component(lj=[(0, 0, -z, 1.0, 1.0, 1.0, 2.5, 0), (0, 0, z, 1.0, 1.0, 1.0, 2.5, 0)])], np.ones((0, 2)), 1e10)


@pytest.mark.parametrize("kind,args,what", [
    ("short", (-1, 10, 0.0, 5.0, 1.0), "slabs"), ("short", (1, 10, 0.0, 5.0, 1.0), "2 slabs"), ("short", (50, 0, 0.0, 5.0, 1.0), "frequency"),
    ("short", (50, 10, 3.0, 2.0, 1.0), "empty"), ("polar", (50, 10, 0.0, 5.0, 0.0), "temperature"), ("long", (50, 10, 0.0, 5.0, 1.0), "elongations"),
    ("nonpolar first", (50, 10, 0.0, 5.0, 1.0), "earlier component"), ("no domain", (50, 10, 0.0, 5.0, 1.0), "domain")])
def test_config_rules(kind, args, what):
    e = engine_mod.DeviceEngine(0)
    e.set_components(_components("short" if kind == "no domain" else kind), 2.5)
    if kind != "no domain":
        e.set_domain([10.0, 10.0, 10.0])
    rc = e.lib.ls1hip_planar_config(e.ctx, *args)
    assert rc == -1 and what in e.lib.ls1hip_last_error(e.ctx).decode()  # LS1HIP_EINVAL
    assert e.lib.ls1hip_planar_config(None, *args) == -1
    e.close()


def test_refused_states():
    c = case("synthetic_bcc1clj_12")
    e = engine(c, c["s"], 0)
    with pytest.raises(capi.Ls1HipError, match="not configured"):
        e.planar()
    e.planar_config(50)
    e.kick_drift(c["dt"])  # the forces are stale now
    with pytest.raises(capi.Ls1HipError, match="valid forces"):
        e.planar()
    e.close()

"""The wall + mirror pass on the device (ls1hip_wall_*, ls1hip_mirror_config, kernels_wall.hip) against tests/wall_ref.py and against
what the unmodified reference driver wrote with the plugins WallPotential and Mirror on (tests/golden/wall/, made by
tests/golden/make_wall_golden.py)."""
import functools

import numpy as np
import pytest

import planar_ref
import wall_ref
from conftest import load_pkg
from golden_io import input_path, sorted_phase_space

pytestmark = pytest.mark.gpu

engine_mod = load_pkg("engine")
inp = load_pkg("inp")
mirror = load_pkg("mirror")
RC = 2.5
YOFF, WIDTH = 0.45, 3.0  # wall of the apply tests: yoff in box lengths, width; surfaces at yoff -+ 1.5
WALL = dict(density=1.07, sigma=1.0, epsilon=1.0, delta=0.775)
# reach -> ycut: nobody although centres lie inside the conservative reach (the nearest site is 0.85 away), part of the box, everything;
# "outside": the wall and a mirror beyond the box, no centre inside any reach: every workgroup takes the early exit of k_wall_apply
YCUT = {"outside": 0.5, "none": 0.5, "part": 2.0, "all": 40.0}


@functools.lru_cache(maxsize=None)
def state(kind):
    """The 3456-molecule bcc box (two workgroup chunks of 2048, a ragged last wave) without the molecules within 0.95 of a wall
    surface, so that no site comes closer than 0.8 sig_wi (sig_wi <= 1, offsets 0.1); 'rotors': a one-centre and a two-centre component
    on alternating lattice sites with random orientations (the construction of the centre / site film)."""
    ps = inp.read_inp(input_path("synthetic_bcc1clj_12.inp"))
    y, yoff = ps.r[:, 1], YOFF * ps.length[1]
    keep = (np.abs(y - (yoff - WIDTH / 2)) >= 0.95) & (np.abs(y - (yoff + WIDTH / 2)) >= 0.95)
    for k in ("ids", "cid", "r", "v", "q", "D"):
        setattr(ps, k, getattr(ps, k)[keep])
    n = len(ps.ids)
    assert n > 2048 and n % 256 and ((y[keep] > yoff - 0.5) & (y[keep] < yoff + 0.5)).any()  # ... and molecules INSIDE the wall slab
    if kind == "rotors":
        b = inp.make_component(lj=[(0, 0, -0.1, 0.5, 0.6, 0.9, 2.5, 0), (0, 0, 0.1, 0.5, 0.6, 0.9, 2.5, 0)])
        ps.components = inp.ComponentSet([ps.components.components[0], b], np.ones((1, 2)), ps.components.eps_rf)
        ps.cid = (np.arange(n) % 2).astype(np.int32)
        q = np.random.default_rng(7).normal(size=(n, 4))
        ps.q, ps.D = q / np.linalg.norm(q, axis=1)[:, None], np.zeros((n, 3))
    return ps, sorted_phase_space(ps)


def engine(ps, s, skin=None, thermostat=None):
    e = engine_mod.DeviceEngine(0)
    e.set_components(ps.components, RC)
    if skin:
        e.set_verlet(skin, force=True)
    e.set_domain(ps.length)
    e.upload(s["ids"], s["cid"], s["r"], s["v"], s["q"], s["D"])
    if thermostat:
        e.set_thermostat(True, thermostat)
    e.rebin(); e.halo(); e.forces(0)
    return e


def configure(e, wall, mirrors):
    """through the public classes: mirror.Mirror per slot, mirror.WallPotential with the XML's names"""
    for slot, m in enumerate(mirrors):
        mirror.Mirror(type=m["type"], direction=m["direction"], coord=m["coord"], cid=m.get("cid", 0), forceConstant=m.get("forceConstant", 100.0),
                      slot=slot).init(e)
    if wall:
        mirror.WallPotential(**wall).init(e)


def check_apply(kind, wall, mirrors):
    """forces(0), one pass, and everything it may and may not have changed against wall_ref on the downloaded state"""
    ps, s = state(kind)
    e = engine(ps, s)
    configure(e, wall, mirrors)
    st, before = e.download_state(), e.download_forces()
    up1 = e.wall_apply()
    after, v_after = e.download_forces(), e.download_state()["v"]
    e.close()
    ref = wall_ref.apply(ps.components, ps.length, st["cid"], st["r"], st["v"], st["q"], wall, mirrors)
    for k, d in (("F", ref["dF"]), ("M", ref["dM"])):  # 1e-10 of the largest restated CHANGE (0: nothing may change)
        assert np.abs(after[k] - (before[k] + d)).max() <= 1e-10 * np.abs(d).max(), k
        assert np.array_equal(after[k][~ref["touched"]], before[k][~ref["touched"]]), k  # bit for bit out of reach
    assert np.abs(up1 - ref["upot"]).max() <= 1e-10 * np.abs(ref["upot"]).max()  # (exactly 0 where nothing is in reach)
    assert np.array_equal(v_after[:, 1], ref["vy"]) and np.array_equal(v_after[:, [0, 2]], st["v"][:, [0, 2]])
    return ref, st


@pytest.mark.parametrize("potential", [93, 104])
@pytest.mark.parametrize("kind", ["1clj", "rotors"])
@pytest.mark.parametrize("reach", ["outside", "none", "part", "all"])
def test_apply(potential, kind, reach):
    ps, _ = state(kind)
    # 'part' of the rotors: the one-centre component is not considered; 'all': both are (the centred-site path beside the rotating one)
    comps = {"1": (1.0, 1.0)} if kind == "1clj" else {"2": (0.9, 1.0)} if reach == "part" else {"1": (1.0, 1.0), "2": (0.9, 1.0)}
    L = float(ps.length[1])
    wall = dict(WALL, potential=potential, yoff=L + 10 if reach == "outside" else YOFF * L, ycut=YCUT[reach], width=WIDTH, components=comps)
    ref, st = check_apply(kind, wall, [dict(type=1, direction=1, coord=2 * L)] if reach == "outside" else ())
    t = ref["touched"]
    assert ref["margin"] >= 0.8
    assert {"outside": not t.any(), "none": not t.any(), "part": t.any() and not t.all(), "all": t[np.isin(st["cid"] + 1, [int(k) for k in comps])].all()}[reach]
    if reach in ("part", "all"):
        assert (ref["dF"][:, 1] > 0).any() and (ref["dF"][:, 1] < 0).any() and (kind == "1clj" or np.abs(ref["dM"]).max() > 0)


@pytest.mark.parametrize("kind", ["1clj", "rotors"])
@pytest.mark.parametrize("mirrors", [[(1, 0, 0, 0)], [(1, 1, 0, 0)], [(2, 0, 0, 0)], [(2, 1, 2, 0)], [(1, 1, 1, 0), (2, 0, 0, -3), (1, 0, 2, -3)]])
def test_mirrors(kind, mirrors):
    """(type, direction, cid, offset of coord): both types, both directions, a component filter, several slots; the first coord is the
    y of a molecule: the half-open edge of inBox"""
    ps, s = state(kind)
    edge = len(s["ids"]) // 2
    ms = [dict(type=t, direction=d, coord=float(s["r"][edge, 1]) + dy, cid=c if kind == "rotors" else 0, forceConstant=20.0) for t, d, c, dy in mirrors]
    ref, st = check_apply(kind, None, ms)
    on_edge = st["r"][:, 1] == ms[0]["coord"]
    assert on_edge.any() and 0 < ref["touched"].sum() < len(on_edge)
    if len(ms) == 1 and not ms[0]["cid"]:
        assert ref["touched"][on_edge].all() == (ms[0]["direction"] == 1)  # a right mirror owns r >= coord, a left one r < coord
    if any(m["type"] == 1 for m in ms):
        assert (ref["vy"] != st["v"][:, 1]).any()


def test_energies_are_bit_reproducible():
    ps, s = state("rotors")
    e = engine(ps, s)
    configure(e, dict(WALL, potential=104, yoff=YOFF * ps.length[1], ycut=YCUT["all"], width=WIDTH, components={"1": (1.0, 1.0), "2": (0.9, 1.0)}), ())
    a, b = e.wall_apply().copy(), e.wall_apply().copy()
    e.close()
    assert np.all(a != 0) and np.array_equal(a, b)


@pytest.mark.parametrize("name", list(wall_ref.cases()))
@pytest.mark.parametrize("skin", [None, 0.2])
def test_trajectory_against_the_driver(name, skin):
    """4 NVT steps of ls1hip_run, per-step loop and list mode, against the driver's step-4 checkpoint (1e-9) and its printed U_pot and p
    (six digits): pins the placement in the step, and that the initial forces see the mirrors but not the wall."""
    c = wall_ref.golden(name)
    ps = c["ps"]
    e = engine(ps, c["s"], skin=skin, thermostat=c["temp"])
    configure(e, None, c["mirrors"])
    if c["mirrors"]:
        e.wall_apply()  # Mirror::afterForces in prepare_start (Simulation.cpp:880-886); WallPotential returns at simstep 0
    configure(e, c["wall"], ())
    e.run(c["dt"], c["steps"])
    st, log, wlog = e.download_state(), e.run_log(), e.wall_log()
    lrc = e.long_range_homogeneous(np.bincount(c["s"]["cid"], minlength=len(ps.components.components)), len(c["s"]["ids"]) / float(np.prod(ps.length)))
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
    res = res[res[:, 0] >= 1][-c["steps"]:]
    N, V = len(st["ids"]), float(np.prod(ps.length))
    np.testing.assert_allclose(log[:, 0] + lrc[0], res[:, 2], rtol=2e-5)  # (the wall energy is no part of U_pot)
    T = (log[:, 2] + log[:, 3]) / (3 * log[:, 4] + log[:, 5])
    np.testing.assert_allclose(N / V * T + (log[:, 1] + lrc[1]) / (3 * V), res[:, 4], rtol=2e-5)
    considered = np.isin(np.arange(wlog.shape[1]) + 1, [int(k) for k in c["wall"]["components"]])
    assert wlog.shape[0] == c["steps"] and np.all(wlog[:, considered] != 0) and np.all(wlog[:, ~considered] == 0)


@pytest.mark.parametrize("skin", [None, 0.2])
def test_off_is_todays_path(skin):
    ps, s = state("1clj")
    out = []
    for configured in (False, True):
        e = engine(ps, s, skin=skin)
        if configured:
            e.wall_config(0)
            e.mirror_config(0, 0)
        res = e.run(0.005, 5)
        out.append((res, e.download_state()))
        e.mirror_config(0, 1, 1, 0.0)  # configured AFTER the run: the log has no row of it
        assert len(e.wall_log()) == 0
        e.close()
    assert out[0][0] == out[1][0] and all(np.array_equal(out[0][1][k], out[1][1][k]) for k in ("ids", "r", "v"))

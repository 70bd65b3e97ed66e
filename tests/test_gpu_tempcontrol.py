"""Region-wise temperature control on the device (ls1hip_tempcontrol_*, kernels_tempcontrol.hip) against tests/tempcontrol_ref.py, on the
two film inputs of the planar goldens: slab sums, betas, scaling, the pieces, the folded kick + drift; ls1hip_run (per-step and list
loop) and the beta log writer against what the unmodified driver wrote (tests/golden/tempcontrol/, made by make_tempcontrol_golden.py)."""
import numpy as np
import pytest

import planar_ref
import tempcontrol_ref
from conftest import load_pkg

pytestmark = pytest.mark.gpu

engine_mod = load_pkg("engine")
mirror = load_pkg("mirror")
case = planar_ref.golden
LJ, MIX = "synthetic_bcc1clj_12", "synthetic_mixed5_8"


def regions(c, kind, slabs, directions="xz", component=0):
    """whole: the box; inner: faces inside the film, all three directions; two: an inner region over a whole-box one"""
    L = c["ps"].length
    whole = dict(lc=[0.0, 0.0, 0.0], uc=list(L), temperature=c["temp"], component=0, numslabs=slabs, exponent=0.4, directions=directions)
    inner = dict(whole, lc=[0.13 * L[0], 0.31 * L[1], 0.07 * L[2]], uc=[0.81 * L[0], 0.62 * L[1], 0.93 * L[2]], component=component, exponent=0.7,
                 temperature=1.1 * c["temp"])
    return {"whole": [dict(whole, component=component)], "inner": [inner], "two": [dict(whole, numslabs=7, directions="xyz"), inner]}[kind]


def engine(c, regs, control=(0, 1, 10 ** 6), skin=None, planar=0):
    st = c["s"]
    e = engine_mod.DeviceEngine(0)
    e.set_components(c["ps"].components, c["rc"])
    if skin:
        e.set_verlet(skin, force=True)
    e.set_domain(c["ps"].length)
    e.upload(st["ids"], st["cid"], st["r"], st["v"], st["q"], st["D"])
    e.rebin(); e.halo(); e.forces(0)
    if planar:
        e.planar_config(planar, 1, None, c["temp"])
    e.tempcontrol_config(*control)
    for r in regs:
        e.tempcontrol_region(r["lc"], r["uc"], r["temperature"], r["component"], r["numslabs"], r["exponent"], r["directions"])
    return e


def sorted_state(e):
    st = e.download_state()
    o = np.argsort(st["ids"])
    return {k: st[k][o] for k in ("r", "v", "q", "D")}


def close(got, want, what):
    want = np.asarray(want, float)
    scale = np.abs(want[np.isfinite(want)]).max()
    assert np.array_equal(np.isfinite(got), np.isfinite(want)) and np.abs(got - want)[np.isfinite(want)].max() <= 1e-10 * scale, what


# directions x / xz / xyz; slabs 1, 20, 77 (no tile multiple), 300 (factors read from global memory), 1100 (sums added to global
# memory directly); component filter; faces inside the film; two overlapping regions
CASES = [(LJ, "whole", 20, "xz", 0), (LJ, "whole", 1, "x", 0), (LJ, "inner", 77, "xyz", 0), (LJ, "whole", 300, "xz", 0), (LJ, "whole", 1100, "xyz", 0),
         (MIX, "whole", 20, "xz", 0), (MIX, "inner", 77, "xyz", 2), (MIX, "whole", 1100, "x", 3), (MIX, "two", 20, "xz", 4), (LJ, "two", 300, "x", 0)]


@pytest.mark.parametrize("name,kind,slabs,directions,component", CASES)
def test_sums_betas_and_scaling(name, kind, slabs, directions, component):
    c = case(name)
    st, regs = c["s"], regions(c, kind, slabs, directions, component)
    lay = engine_mod.DeviceEngine.tempcontrol_layout
    ref = tempcontrol_ref.TemperatureControl(c["ps"].components, 0, 1, 10 ** 6, regs)
    v, D = st["v"].copy(), st["D"].copy()
    ref.control(0, st["cid"], st["r"], v, st["q"], D)
    e = engine(c, regs)
    assert lay(e)["lds_slabs"] == 1024 and lay(e)["apply_lds_slabs"] == 256  # the limits the slab counts above straddle
    e.temperature_control(0)
    got, after = [e.tempcontrol_read(k + 1) for k in range(len(regs))], sorted_state(e)
    e.close()
    for g, reg in zip(got, ref.regions):
        assert reg["n"].sum() > 0 and np.array_equal(g["n"], reg["n"]) and np.array_equal(g["rotdof"], reg["rotdof"])
        for k in ("ekin_trans", "ekin_rot", "beta_trans", "beta_rot"):
            close(g[k], reg[k], (name, kind, slabs, k))
        assert g["configs"] == 1 and all(abs(g[k] - reg[k]) <= 1e-10 * reg[k] for k in ("beta_trans_sum", "beta_rot_sum"))
    close(after["v"], v, "v")
    if np.abs(D).max() > 0:
        close(after["D"], D, "D")
    # what the reference does not multiply keeps its bits: unmasked components, molecules outside every region
    assert (v != st["v"]).any()
    assert np.array_equal(after["v"][v == st["v"]], st["v"][v == st["v"]]) and np.array_equal(after["D"][D == st["D"]], st["D"][D == st["D"]])
    assert np.array_equal(after["r"], st["r"]) and np.array_equal(after["q"], st["q"])


@pytest.mark.parametrize("name,kind,slabs", [(LJ, "whole", 20), (MIX, "two", 300)])
def test_pieces_equal_the_one_call_form(name, kind, slabs):
    c = case(name)
    regs = regions(c, kind, slabs, component=2 if name == MIX else 0)
    one, two = engine(c, regs), engine(c, regs)
    one.temperature_control(0)
    two.tempcontrol_measure()
    sums = two.tempcontrol_sums()
    two.tempcontrol_sums(np.zeros_like(sums))
    two.tempcontrol_sums(sums)
    two.tempcontrol_betas()
    two.tempcontrol_apply()
    a, b = sorted_state(one), sorted_state(two)
    ra, rb = one.tempcontrol_read(1), two.tempcontrol_read(1)
    one.close(); two.close()
    assert sums["n"].sum() > 0 and np.array_equal(ra["n"], rb["n"])
    # (the f64 sums of two sweeps may differ in the last bits: the states agree to the parity tolerance, not bit for bit)
    for k in ("v", "D"):
        assert np.abs(a[k] - b[k]).max() <= 1e-10 * max(np.abs(a[k]).max(), 1e-300), k


@pytest.mark.parametrize("name", [LJ, MIX])
@pytest.mark.parametrize("slabs", [20, 300])
@pytest.mark.parametrize("skin", [None, 0.2])
def test_folded_apply_is_apply_then_kick_drift(name, slabs, skin):
    """bit for bit, 1CLJ and rotors, factors staged in LDS and read from global memory, per-step state and list mode"""
    c = case(name)
    regs = regions(c, "two", slabs, component=1)
    out = []
    for folded in (False, True):
        e = engine(c, regs, skin=skin and skin * c["rc"] / 2.5)
        if skin:
            e.update(); e.forces_list(0)
        e.tempcontrol_measure()
        sums = e.tempcontrol_sums() if not out else out[0][1]
        e.tempcontrol_sums(sums)  # the same sums on both engines: everything after them is deterministic
        e.tempcontrol_betas()
        if folded:
            e.tempcontrol_apply_kick_drift(c["dt"])
        else:
            e.tempcontrol_apply()
            e.kick_drift(c["dt"])
        out.append((e.download_state(), sums))
        e.close()
    assert all(np.array_equal(out[0][0][k], out[1][0][k]) for k in ("ids", "r", "v", "q", "D"))
    assert not np.array_equal(out[0][0]["v"], c["s"]["v"][np.searchsorted(c["s"]["ids"], out[0][0]["ids"])])


def run_engine(c, regs, control, steps, skin, planar=0, chunk=None, tc=None, directory=None):
    """ls1hip_run over `steps` steps (in chunks of `chunk` with the beta log written between them) -> state, step log, engine reads"""
    e = engine(c, regs if tc is None else [], control=control, skin=skin and skin * c["rc"] / 2.5, planar=planar)
    if tc is not None:
        tc.init(e, directory)
    for first in range(0, steps, chunk or steps):
        e.run(c["dt"], chunk or steps)
        if tc is not None:
            tc.write(first + (chunk or steps), directory)
    ps = c["ps"]  # the driver's default long-range correction (longRange/Homogeneous): constants of the run, added by the host
    lrc = e.long_range_homogeneous(np.bincount(c["s"]["cid"], minlength=len(ps.components.components)), len(c["s"]["ids"]) / float(np.prod(ps.length)))
    out = dict(lrc=lrc, st=sorted_state(e), log=e.run_log(), read=[e.tempcontrol_read(k + 1) for k in range(len(regs))], builds=e.get_option("verlet_builds") if skin else 0)
    e.close()
    return out


def assert_state(got, want, L):
    dr = got["r"] - want["r"]
    dr -= L * np.rint(dr / L)
    assert np.abs(dr).max() <= 1e-9 * L.max()
    for k in ("v", "q", "D"):
        if np.abs(want[k]).max() > 0:
            assert np.abs(got[k] - want[k]).max() <= 1e-9 * np.abs(want[k]).max(), k


# the driver's cases (tests/golden/tempcontrol): a = frequency 1; b = frequency 2 inside [2, 5): measurements at steps 2 and 4, step 6
# scales with the factors of step 4 (stale) inside the kick + drift of step 7.  skin 0.05: a list rebuild falls into the run, and
# between rebuilds the molecules that crossed a face sit outside the box on control steps
@pytest.mark.parametrize("name", sorted(tempcontrol_ref.cases()))
@pytest.mark.parametrize("skin", [None, 0.05])
def test_run_against_the_driver(name, skin):
    c = tempcontrol_ref.golden(name)
    ps, steps = c["ps"], c["steps"]
    # (skin / 2 of about two steps of the fastest molecule: 0.0135 per step in the LJ film, 0.097 in the slow five-component one)
    got = run_engine(c, c["regions"], c["control"], steps, skin and (skin if name.startswith("bcc") else 0.4 * skin))
    assert_state(got["st"], planar_ref.read_restart(c["files"]["step%d.restart.dat" % steps].decode()), ps.length)
    res, log = tempcontrol_ref.read_result(c["files"]["result.res"].decode())[-steps:], got["log"]
    N, V = len(c["s"]["ids"]), float(np.prod(ps.length))
    # result.res prints six digits: U_pot, p = rho T + rho virial / (3 N), and T through thermostat 0's beta_trans / beta_rot of
    # Domain::calculateGlobalValues (Domain.cpp:225-240), all from the velocities BEFORE the control
    T = (log[:, 2] + log[:, 3]) / (3 * log[:, 4] + log[:, 5])
    np.testing.assert_allclose(log[:, 0] + got["lrc"][0], res[:, 2], rtol=1e-5)
    np.testing.assert_allclose(N / V * T + (log[:, 1] + got["lrc"][1]) / (3 * V), res[:, 4], rtol=1e-5)
    np.testing.assert_allclose((3 * log[:, 4] * c["temp"] / log[:, 2]) ** 0.4, res[:, 6], rtol=1e-5)
    if log[:, 3].max() > 0:
        np.testing.assert_allclose((log[:, 5] * c["temp"] / log[:, 3]) ** 0.4, res[:, 7], rtol=1e-5)
    if skin:
        assert 2 <= got["builds"] <= steps, got["builds"]


@pytest.mark.parametrize("skin", [None, 0.05])
def test_run_with_the_planar_correction(skin):
    """both configured in one run, against tempcontrol_ref + planar_ref stepped on the CPU"""
    c = tempcontrol_ref.golden("bcc1clj_b")
    pl = planar_ref.Planar(c["ps"].components, c["ps"].length, c["rc"], 50, temperature=c["temp"])
    regs = [{k: v for k, v in r.items() if k != "writefreq"} for r in c["regions"]]  # (no beta log writes: the accumulators stay)
    want = tempcontrol_ref.run(c, c["control"], regs, c["steps"], planar=pl)
    got = run_engine(c, c["regions"], c["control"], c["steps"], skin, planar=50)
    assert_state(got["st"], want, c["ps"].length)
    np.testing.assert_allclose(got["log"][:, 2], want["log"][:, 2], rtol=1e-9)  # unscaled sum m v^2 of every step
    for g, reg in zip(got["read"], want["tc"].regions):
        assert g["configs"] == reg["configs"] == 2 and np.array_equal(g["n"], reg["n"])
        assert abs(g["beta_trans_sum"] - reg["beta_trans_sum"]) <= 1e-9 * reg["beta_trans_sum"]


@pytest.mark.parametrize("name", ["bcc1clj_a", "mixed5_b"])
def test_beta_log_writer_reproduces_the_drivers_files(name, tmp_path):
    """mirror.TemperatureControl.write: the header byte for byte, the doubles to 1e-10 (mixed5_b, region 1: one record that is the sum
    over slabs and over TWO configurations divided by 2, the reference's quirk)"""
    c = tempcontrol_ref.golden(name)
    tc = mirror.TemperatureControl(c["ps"].length, *c["control"], c["regions"])
    run_engine(c, c["regions"], c["control"], c["steps"], None, chunk=1, tc=tc, directory=str(tmp_path))
    for k in range(len(c["regions"])):
        want, got = c["files"]["beta_log_reg%d.dat" % (k + 1)], (tmp_path / ("beta_log_reg%d.dat" % (k + 1))).read_bytes()
        assert got[:8] == want[:8] and len(got) == len(want) > 8
        a, b = tempcontrol_ref.read_beta_log(got)[1], tempcontrol_ref.read_beta_log(want)[1]
        assert np.abs(a / b - 1).max() <= 1e-10


def test_refused_states():
    c = case(LJ)
    e = engine(c, [])
    with pytest.raises(load_pkg("capi").Ls1HipError, match="not configured"):
        e.temperature_control(0)
    e.tempcontrol_region([0, 0, 0], list(c["ps"].length), c["temp"], 0, 20, 0.4, "xz")
    with pytest.raises(load_pkg("capi").Ls1HipError, match="exclude each other"):
        e.set_thermostat(True, c["temp"])
    e.tempcontrol_config(0, 0, 0)  # removed: the global thermostat may come back, a run takes today's path
    e.set_thermostat(True, c["temp"])
    e.close()

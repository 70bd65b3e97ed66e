"""Test-particle insertion energies and Widom sampling on the device (ls1hip_insertion_energies, ls1hip_widom_*; kernels_insert.hip).

Reference for dU: the committed oracle, PAIR BY PAIR — for test k and every molecule j whose minimum-image centre distance is below
r_c, Oracle.forces on the two-molecule non-periodic system {test, image of j}; dU_k = math.fsum of those.  Bar: the project's parity
bar |got - want| <= 1e-10 sum_j |u_kj|, and exactly 0.0 where no partner is in range.

The golden cases hold 5-37 (lj_periodic, multi_periodic: 250 molecules, r_c 35 in a box of 134) and 0-14 (ethan) partners per point,
never 65: the mid-scan flush of the hit queue is covered by the two `dense` rows (r_c 60, two cells per cutoff: ~93 partners), which
assert their partner counts.  lj_periodic is a two-centre LJ fluid, so the single-centre kernel gets a case of its own (bcc1clj_3456).
In the boxes of 134 the middle of an emptied half is only 33.6 < r_c from the molecules left on either side (periodic images), so the
void test keeps one quarter of the box and asserts that its probes have no partner."""
import functools
import math

import numpy as np
import pytest

from conftest import load_pkg
from golden_io import input_path, manifest, sorted_phase_space
from oracle.oracle import Oracle

pytestmark = pytest.mark.gpu

capi = load_pkg("capi")
engine_mod = load_pkg("engine")
inp = load_pkg("inp")

CASES = ("lj_periodic", "ethan", "multi_periodic", "bcc1clj_3456")
LIST_RUN = {"lj_periodic": (2.0, 2.0), "ethan": (2.0, 0.5), "bcc1clj_3456": (None, 0.005)}  # skin, dt (the manifest's step cases)


@functools.lru_cache(maxsize=None)
def _case(name):
    c = manifest()[name]
    ps = inp.read_inp(input_path(c["input"]))
    return ps, sorted_phase_space(ps), np.asarray(ps.length, dtype=np.float64), c["rc"]


def _engine(name, rc, s, cic=1, skin=None):
    ps = _case(name)[0]
    e = engine_mod.DeviceEngine(0)
    e.set_components(ps.components, rc)
    e.set_option("cells_in_cutoff", cic)
    if skin:
        e.set_verlet(skin, force=True)
    e.set_domain(ps.length)
    e.upload(s["ids"], s["cid"], s["r"], s["v"], s["q"], s["D"])
    return e


def _min_image(s, L, r):
    d = s["r"] - r
    d -= L * np.round(d / L)
    return d, (d * d).sum(axis=1)


def _tests(s, L, rc, single):
    """about 40 deliberately placed tests (cid, r, q, exclude_id) for the state s"""
    rng = np.random.default_rng(7)
    N, up = len(s["ids"]), np.nextafter(L, 0.0)
    none = np.uint64(int(s["ids"].max()) + 1)
    sr = np.minimum(s["r"] % L, up)  # list mode: a molecule may sit up to skin / 2 outside the box between two builds
    pick = np.arange(0, N, max(1, N // 400))  # the molecules the placed tests choose from
    sr, ids, N = sr[pick], s["ids"][pick], len(pick)
    cnt = np.array([int((_min_image(s, L, p)[1] < rc * rc).sum()) for p in sr])
    r = [rng.uniform(0.2, 0.8, 3) * L for _ in range(8)]  # faces and corners: every partner through halo cells and images
    for d in range(3):
        r[d][d], r[3 + d][d] = 0.0, up[d]
    r[6][:], r[7][:] = 0.0, up
    own = [0, 1, 2, N // 2, N - 1, int(np.argmax(cnt))]  # on an existing molecule, which is not to be seen
    r += [sr[i].copy() for i in own]
    ex = [none] * 8 + [ids[i] for i in own]
    if not single:  # ... and seen: the centres coincide, the sites (another orientation) do not
        r += [sr[i].copy() for i in own[:4]]
    r += [np.minimum((sr[i] + 0.1 * rc) % L, up) for i in (int(np.argmax(cnt)), int(np.argmin(cnt)))]  # densest / sparsest spot
    r += [rng.uniform(0.0, 1.0, 3) * L for _ in range(40 - len(r))]
    ex += [none] * (40 - len(ex))
    q = rng.normal(size=(40, 4))
    return s["cid"][pick[np.arange(40) % N]].astype(np.int32), np.array(r), q / np.linalg.norm(q, axis=1)[:, None], np.array(ex, dtype=np.uint64)


def _reference(name, rc, s, L, cid, r, q, ex):
    """per test: fsum of the oracle's pair energies, sum of their magnitudes, partners in range"""
    orc = Oracle(_case(name)[0].components.flat(), rc)
    box, out = np.full(3, 4.0 * rc), []
    for k in range(len(r)):
        d, dd = _min_image(s, L, r[k])
        assert np.min(np.abs(np.sqrt(dd) - rc)) > 1e-9 * rc, "a partner sits on the cutoff sphere: the in / out decision is a rounding"
        js = np.nonzero((dd < rc * rc) & (s["ids"] != ex[k]))[0]
        u = [orc.forces(np.array([box / 2, box / 2 + d[j]]), np.array([q[k], s["q"][j]]), np.array([cid[k], s["cid"][j]]), box, False)["upot"]
             for j in js]
        out.append((math.fsum(u), math.fsum(np.abs(u)), len(js)))
    return np.array(out)


def _check(got, ref, what):
    err, bar = np.abs(got - ref[:, 0]), 1e-10 * ref[:, 1]
    print(what, "max |got - want| / sum|u| =", float(np.max(err[bar > 0] / ref[bar > 0, 1], initial=0.0)), "partners", ref[:, 2].astype(int).tolist())
    assert np.all(err <= bar), (what, np.nonzero(err > bar)[0].tolist(), got[err > bar], ref[err > bar])


@functools.lru_cache(maxsize=None)
def _static(name, rc):
    ps, s, L, _ = _case(name)
    t = _tests(s, L, rc, single=name == "bcc1clj_3456")
    return t, _reference(name, rc, s, L, *t)


@pytest.mark.parametrize("name,rc,cic,dense", [(n, None, 1, False) for n in CASES] + [("lj_periodic", None, 2, False)] +
                         [("lj_periodic", 60.0, 2, True), ("multi_periodic", 60.0, 2, True)])
def test_insertion_energies_against_the_oracle(name, rc, cic, dense):
    ps, s, L, rc0 = _case(name)
    rc = rc or rc0
    (cid, r, q, ex), ref = _static(name, rc)
    # the queue is flushed inside the scan (dense rows: 65 partners and more) or only at its end (the others: 1 ... 63)
    assert ref[:, 2].min() >= 65 if dense else np.any((ref[:, 2] >= 1) & (ref[:, 2] <= 63)), ref[:, 2]
    e = _engine(name, rc, s, cic)
    e.rebin(); e.halo()
    rotates = name != "bcc1clj_3456"
    for n in (1, 5, 40):  # fewer tests than waves; no multiple of four; the first eight exclude nothing
        got = e.insertion_energies(cid[:n], r[:n], q[:n] if rotates or n == 40 else None, ex[:n] if n == 40 else None)
        _check(got, ref[:n], (name, rc, cic, n))
    e.close()


@pytest.mark.parametrize("name", CASES)
def test_no_partner_gives_exactly_zero(name):
    ps, s, L, rc = _case(name)
    keep = s["r"][:, 0] >= 0.75 * L[0]
    sub = {k: v[keep] for k, v in s.items()}
    r = np.array([[0.375, 0.5, 0.5], [0.375, 0.0, 0.9], [0.30, 0.2, 0.0]]) * L
    assert all(int((_min_image(sub, L, p)[1] < rc * rc).sum()) == 0 for p in r)
    e = _engine(name, rc, sub)
    e.rebin(); e.halo()
    got = e.insertion_energies(np.zeros(3, np.int32), r, np.tile([1.0, 0, 0, 0], (3, 1)))
    e.close()
    assert np.array_equal(got, np.zeros(3)), got


@pytest.mark.parametrize("name", ["lj_periodic", "ethan"])
def test_list_mode_stale_binning(name):
    """a few list steps: the binning is that of the last build, the halo copies carry build-time orientations"""
    ps, s, L, rc = _case(name)
    skin, dt = LIST_RUN[name]
    e = _engine(name, rc, s, skin=skin)
    e.rebin(); e.halo(); e.forces(0)
    e.run(dt, 4)
    assert e.get_option("last_force_kernel") == capi.FK_NEIGHBOUR_LIST
    now = e.download_state()
    cid, r, q, ex = _tests(now, L, rc, single=False)
    got = e.insertion_energies(cid, r, q, ex)
    e.close()
    _check(got, _reference(name, rc, now, L, cid, r, q, ex), (name, "list mode"))


@pytest.mark.parametrize("name,slabs,instances,cv", [("ethan", 1, 3, None), ("ethan", 7, 3, None), ("ethan", 1, 1000, None),
                                                     ("ethan", 7, 1000, (0.25, 0.75)), ("bcc1clj_3456", 7, 1000, None)])
def test_widom_sampling(name, slabs, instances, cv):
    ps, s, L, rc = _case(name)
    T = float(ps.temperature)
    lo, hi = (np.zeros(3), L) if cv is None else (cv[0] * L, cv[1] * L)
    e = _engine(name, rc, s)
    e.rebin(); e.halo()
    e.widom_config(0, instances, T, seed=11, slabs=slabs, cv_min=None if cv is None else lo, cv_max=None if cv is None else hi)
    e.widom_sample()
    a, t = e.widom_last(), e.widom_read()
    assert a["r"].shape == (instances, 3) and np.all(a["r"] >= lo) and np.all(a["r"] < hi)
    assert np.max(np.abs(np.linalg.norm(a["q"], axis=1) - 1.0)) < 1e-14
    if name == "bcc1clj_3456":
        assert np.array_equal(a["q"], np.tile([1.0, 0, 0, 0], (instances, 1)))
    assert np.array_equal(a["dU"], e.insertion_energies(np.zeros(instances, np.int32), a["r"], a["q"]))
    slab = np.floor(a["r"][:, 1] / L[1] * slabs).astype(int)
    with np.errstate(over="ignore"):
        want = np.bincount(slab, np.exp(-a["dU"] / T), minlength=slabs)
    assert np.array_equal(t["n"], np.bincount(slab, minlength=slabs)) and t["samples"] == 1
    assert np.all(np.abs(t["sum_w"] - want) <= 1e-12 * want), (t["sum_w"], want)
    e.widom_reset()  # the same seed, the same sample index, the same state: the same tests
    e.widom_sample()
    b = e.widom_last()
    assert all(np.array_equal(a[k], b[k]) for k in ("r", "q", "dU"))
    e.widom_sample()  # sample index 1: other tests
    c, t2 = e.widom_last(), e.widom_read()
    assert not np.any(np.all(a["r"] == c["r"], axis=1)) and t2["samples"] == 2 and int(t2["n"].sum()) == 2 * instances
    e.close()


@pytest.mark.parametrize("name", ["bcc1clj_3456", "ethan"])
def test_run_with_widom_every_keeps_the_trajectory(name):
    ps, s, L, rc = _case(name)
    skin, dt = LIST_RUN[name]
    final = []
    for every in (0, 2):
        e = _engine(name, rc, s, skin=skin)
        e.rebin(); e.halo(); e.forces(0)
        if every:
            e.widom_config(0, 100, float(ps.temperature), seed=3, slabs=4)
            e.set_option("widom_every", every)
        out = e.run(dt, 6)
        if every:
            t = e.widom_read()
            assert t["samples"] == 3 and int(t["n"].sum()) == 300
        final.append((out, e.download_state()))
        e.close()
    assert final[0][0] == final[1][0]
    assert all(np.array_equal(final[0][1][k], final[1][1][k]) for k in ("ids", "r", "v", "q", "D"))


def test_refused_calls_name_the_cause():
    ps, s, L, rc = _case("ethan")
    e = _engine("ethan", rc, s)
    one, q1 = np.zeros(1, np.int32), np.array([[1.0, 0, 0, 0]])
    with pytest.raises(capi.Ls1HipError, match="not binned"):
        e.insertion_energies(one, [0.5 * L], q1)
    e.rebin(); e.halo(); e.forces(0)
    with pytest.raises(capi.Ls1HipError, match="test 1: position .* outside the box"):
        e.insertion_energies(np.zeros(2, np.int32), [0.5 * L, [L[0], 1.0, 1.0]], np.tile(q1, (2, 1)))
    with pytest.raises(capi.Ls1HipError, match="test 0: component 0 rotates, q is required"):
        e.insertion_energies(one, [0.5 * L])
    with pytest.raises(capi.Ls1HipError, match="component id 1 out of range"):
        e.insertion_energies(one + 1, [0.5 * L], q1)
    assert e.insertion_energies(np.zeros(0, np.int32), np.zeros((0, 3))).shape == (0,)
    e.set_option("widom_every", 2)
    with pytest.raises(capi.Ls1HipError, match="widom_every is set but Widom sampling is not configured"):
        e.run(0.5, 2)
    e.close()

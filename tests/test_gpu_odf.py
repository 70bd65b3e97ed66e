"""ODF sampling on the device (ls1hip_odf_*, kernels_odf.hip) against a brute-force restatement of ODF::calculateOrientation
(io/ODF.cpp:123-331) over the pair set of ODFCellProcessor.  Counts are integers: every comparison is exact equality of ALL words.
Condition instead of a tolerance: every state used keeps every value the restatement decides on at least EDGE_MARGIN away from
its decision edge (device and numpy differ by rounding of order 1e-15 on these O(1) quantities).  A value the rounding rule
replaced is an exact integer (0, +-1; gamma in {0, pi/2, pi}) on both sides and is decided by edge expressions both sides evaluate
identically, so its margin is that of the rounding decision (|c| and ||c| - 1| against 1e-4), not its distance from a bin edge."""
import functools

import numpy as np
import pytest

from conftest import load_pkg
from golden_io import input_path, sorted_phase_space

pytestmark = pytest.mark.gpu

capi = load_pkg("capi")
engine_mod = load_pkg("engine")
inp = load_pkg("inp")
decomp = load_pkg("decomp")

EDGE_MARGIN = 1e-9


def odf_ref(r, q, cid, dipolar, L, rc, P, G, shell, periodic=True):
    """(hist uint64 [2, 2, P P G + 1], margin) of ONE configuration: O(N^2), minimum image, the literal bin search on the edge arrays."""
    r, q, cid = np.asarray(r, np.float64), np.asarray(q, np.float64), np.asarray(cid, np.int64)
    dot = lambda a, b: a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1] + a[:, 2] * b[:, 2]  # noqa: E731
    i, j = np.triu_indices(len(r), 1)  # arrays are ordered by id: i is the molecule with the smaller id
    d = r[j] - r[i]
    if periodic:
        d -= L * np.round(d / L)
    dd = dot(d, d)
    both = np.asarray(dipolar)[cid[i]] & np.asarray(dipolar)[cid[j]]  # exactly one dipole each (ODFCellProcessor.cpp:25,34)
    dist = np.sqrt(dd[both])
    margin = min(np.abs(dist - shell).min(), np.abs(dist - rc).min())
    use = both & (dd < min(rc * rc, shell * shell))
    i, j, d = i[use], j[use], d[use] / np.sqrt(dd[use])[:, None]
    e = np.stack([2 * (q[:, 1] * q[:, 3] + q[:, 0] * q[:, 2]), 2 * (q[:, 2] * q[:, 3] - q[:, 0] * q[:, 1]),
                  1 - 2 * (q[:, 1] * q[:, 1] + q[:, 2] * q[:, 2])], axis=1)  # quaternion as stored
    c1, c2 = dot(d, e[i]), -dot(d, e[j])
    p1, p2 = np.cross(d, np.cross(e[i], d)), np.cross(d, np.cross(e[j], d))
    with np.errstate(invalid="ignore", divide="ignore"):
        cg = dot(p1 / np.sqrt(dot(p1, p1))[:, None], p2 / np.sqrt(dot(p2, p2))[:, None])
    raw = np.concatenate([c1, c2, cg])
    margin = min(margin, np.nanmin(np.abs(np.abs(raw) - 1e-4)), np.nanmin(np.abs(np.abs(np.abs(raw) - 1.) - 1e-4)))
    rule = lambda c: np.where((np.abs(c) < 1e-4) | (np.abs(np.abs(c) - 1.) < 1e-4), np.round(c), c)  # noqa: E731
    c1, c2, cg = rule(c1), rule(c2), rule(cg)
    gam = np.arccos(cg)
    cedges = 1. - np.arange(P + 1) * 2. / P  # 1 ... -1: bin i has cedges[i] >= c > cedges[i + 1]
    gedges = np.arange(G + 1) * np.pi / G    # bin i has gedges[i] <= gamma < gedges[i + 1]

    def cos_bin(c):
        k = P - np.searchsorted(cedges[::-1], c, side="left")
        k = np.where(c == -1., P - 1, k)
        return np.where((k >= 0) & (k < P), k, 0)  # nothing fits (NaN): the index stays 0

    i1, i2 = cos_bin(c1), cos_bin(c2)
    g = np.where(np.isnan(gam), 0, np.minimum(np.searchsorted(gedges, gam, side="right"), G))
    for c in (c1, c2):
        free = c != np.round(c)
        margin = min(margin, np.abs(c[free, None] - cedges[None, :]).min())
    free = ~np.isnan(cg) & (cg != np.round(cg))
    margin = min(margin, np.abs(gam[free, None] - gedges[None, :]).min())
    H = np.zeros((2, 2, P * P * G + 1), dtype=np.uint64)
    a, b = cid[i], cid[j]
    np.add.at(H, (a, b, (i1 * P + i2) * G + g), 1)
    np.add.at(H, (b, a, (i2 * P + i1) * G + g), 1)
    return H, float(margin)


def _stockmayer(ndip=1):
    return inp.make_component(lj=[(0, 0, 0, 0.016, 0.00042, 6.0, 0, 0)], dipoles=[(0, 0, 0, 0, 0, 1, 0.5)] * ndip,
                              I_file=(0.004, 0.004, 0.004))


def _comps(kinds):
    n = len(kinds)
    return inp.ComponentSet([_stockmayer(k) for k in kinds], np.ones((n * (n - 1) // 2, 2)), 1e10)


@functools.lru_cache(maxsize=None)
def _state(fname, mod):
    """positions, quaternions, velocities of a fixture; component = id % mod"""
    ps = inp.read_inp(input_path(fname))
    s = sorted_phase_space(ps)
    s["cid"] = (s["ids"] % np.uint64(mod)).astype(np.int32)
    return ps.length, s


@functools.lru_cache(maxsize=None)
def _want(fname, rc, periodic, P, G, shell, mod, kinds):
    L, s = _state(fname, mod)
    return odf_ref(s["r"], s["q"], s["cid"], [k == 1 for k in kinds], L, rc, P, G, shell, periodic)


def _engine(comps, rc, L, s, periodic=True, skin=None):
    e = engine_mod.DeviceEngine(0)
    e.set_components(comps, rc)
    if skin:
        e.set_verlet(skin)
    e.set_domain(L, periodic=periodic)
    e.upload(s["ids"], s["cid"], s["r"], s["v"], s["q"], s["D"])
    e.rebin(); e.halo(); e.forces(0)
    return e


WATER, MIXED = ("synthetic_water_5.inp", 12.0), ("synthetic_mixed5_8.inp", 35.0)


# water_5: 125 molecules, 3 cells per edge, 4.6 per cell — partial 4 x 4 x 2 bricks, images of the own brick.  mixed5_8: 1024 molecules, 8
# cells per edge — full 4 x 4 x 4 bricks of 128 molecules, eight workgroups flushing; at shell = r_c 7.5 hits per molecule, ~960 per
# brick, against a hit queue of 1536 entries that is drained as soon as it holds more than 512: at least two drains per workgroup.
@pytest.mark.parametrize("fixture,periodic,P,G,frac,mod,kinds", [
    (WATER, True, 9, 7, 1.0, 2, (1, 1)),
    (WATER, False, 9, 7, 1.0, 2, (1, 1)),
    (MIXED, True, 10, 10, 1.0, 2, (1, 1)),      # 4 W = 4004 words: the LDS histogram
    (MIXED, True, 10, 10, 0.6, 2, (1, 1)),
    (MIXED, True, 24, 24, 1.0, 2, (1, 1)),      # 4 W = 55300 words: global atomics
    (MIXED, True, 10, 10, 1.0, 1, (1, 1)),      # one dipolar component only
    (MIXED, True, 9, 7, 1.0, 3, (1, 1, 2)),     # a third of the molecules carries two dipoles: ignored
])
def test_device_histogram_equals_the_restatement(fixture, periodic, P, G, frac, mod, kinds):
    (fname, rc), shell = fixture, frac * fixture[1]
    want, margin = _want(fname, rc, periodic, P, G, shell, mod, kinds)
    print("edge margin", margin)
    assert margin >= EDGE_MARGIN
    L, s = _state(fname, mod)
    e = _engine(_comps(kinds), rc, L, s, periodic)
    e.odf_config(P, P, G, shell)
    assert e.odf_layout() == P * P * G + 1
    assert (4 * e.odf_layout() <= e.get_option("odf_lds_words")) == (P < 24)
    e.odf_sample()
    got = e.odf_read()
    e.odf_sample()
    twice = e.odf_read()
    e.odf_reset()
    zero = e.odf_read()
    e.close()
    assert got["samples"] == 1 and got["hist"].shape == want.shape and int(want.sum()) > 300
    assert np.array_equal(got["hist"], want), int(np.abs(got["hist"].astype(np.int64) - want.astype(np.int64)).sum())
    assert twice["samples"] == 2 and np.array_equal(twice["hist"], 2 * want)
    assert zero["samples"] == 0 and not zero["hist"].any()
    if mod == 1:
        assert want[0, 0].any() and not want[0, 1].any() and not want[1].any()


def test_run_samples_in_list_mode_between_list_builds():
    """odf_every = 2, odf_from = 1 over five steps: steps 2 and 4; the halo copies' quaternions come from their source molecules"""
    (fname, rc), dt, P, G, shell = MIXED, 0.2, 10, 10, 0.9 * 35.0
    L, s = _state(fname, 2)
    a = _engine(_comps((1, 1)), rc, L, s, skin=2.5)
    a.odf_config(P, P, G, shell)
    a.set_option("odf_every", 2)
    a.set_option("odf_from", 1)
    a.run(dt, 5)
    got = a.odf_read()
    assert a.get_option("last_force_kernel") == capi.FK_NEIGHBOUR_LIST and (a.get_option("odf_every"), a.get_option("odf_from")) == (2, 1)
    a.close()
    b = _engine(_comps((1, 1)), rc, L, s, skin=2.5)
    want = 0
    for step in range(1, 6):
        b.run(dt, 1)
        if step in (2, 4):
            st = b.download_state()
            o = np.argsort(st["ids"])
            H, margin = odf_ref(st["r"][o], st["q"][o], st["cid"][o], [True, True], L, rc, P, G, shell)
            print("step", step, "edge margin", margin)
            assert margin >= EDGE_MARGIN
            want = want + H
    b.close()
    assert got["samples"] == 2
    assert np.array_equal(got["hist"], want)


def test_two_sub_domains_sum_to_the_single_domain():
    from test_gpu_multirank import InProcessCluster
    (fname, rc), P, G = MIXED, 10, 10
    want, margin = _want(fname, rc, True, P, G, rc, 2, (1, 1))
    assert margin >= EDGE_MARGIN
    L, s = _state(fname, 2)
    multi = InProcessCluster(2, _comps((1, 1)), rc, L, s["ids"], s["r"], s["v"], cid=s["cid"], q=s["q"], D=s["D"])
    multi.forces()
    total = 0
    for e in multi.eng:
        e.odf_config(P, P, G, rc)
        e.odf_sample()
        loc = decomp.odf_collect(e)  # no process group: the local arrays; across processes the same call all-reduces them
        assert loc["samples"] == 1 and 0 < loc["hist"].sum() < want.sum()
        total = total + loc["hist"]
        e.close()
    assert np.array_equal(total, want)


def test_refusals_leave_the_context_usable():
    (fname, rc), P, G = MIXED, 10, 10
    L, s = _state(fname, 2)
    e = _engine(_comps((1, 1)), rc, L, s)
    with pytest.raises(capi.Ls1HipError, match="phi1_increments != phi2_increments"):
        e.odf_config(10, 9, 10, rc)
    with pytest.raises(capi.Ls1HipError, match="shell_cutoff"):
        e.odf_config(P, P, G, 1.01 * rc)
    e.set_option("odf_every", 1)
    with pytest.raises(capi.Ls1HipError, match="odf_every"):
        e.run(0.2, 1)
    e.set_option("odf_every", 0)
    e.odf_config(P, P, G, rc)
    e.odf_sample()
    got = e.odf_read()
    e.close()
    assert np.array_equal(got["hist"], _want(fname, rc, True, P, G, rc, 2, (1, 1))[0])
    f = _engine(_comps((1, 1, 1)), rc, L, s)  # a single-dipole component with id 2
    with pytest.raises(capi.Ls1HipError, match="id >= 2"):
        f.odf_config(P, P, G, rc)
    f.run(0.2, 1)
    f.close()

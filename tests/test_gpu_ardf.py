"""The angular RDF on the device (ls1hip_rdf_config_angular, kernels_ardf.hip) against the brute-force restatement of tests/ardf_ref.py
that tests/test_ardf_cpu.py pins to the reference's files.  Counts are integers: every comparison is exact equality.  Every state
used satisfies ardf_ref.usable (no distance within 1e-8 of a bin edge, r_c or bins * dr, no cos(phi) within 1e-8 of an angular edge)."""
import numpy as np
import pytest

import ardf_ref
import rdf_ref
from golden_io import sorted_phase_space
from test_gpu_rdf import _assert_equal, _engine, _fixture

pytestmark = pytest.mark.gpu


def _state(name):  # a fixture file as it stands, or step 1 of a golden case of tests/golden/rdf: ps, phase space in id order, r, q
    if name.endswith(".inp"):
        ps, s = _fixture(name)
        return ps, s, s["r"], s["q"]
    cs = rdf_ref.case_states(name)
    return cs["ps"], sorted_phase_space(cs["ps"]), cs["states"][0]["r"], cs["states"][0]["q"]


def _want(ps, r, q, cid, rc, bins, dr, A, **kw):
    want = ardf_ref.brute_force(r, q, cid, len(ps.components.components), ps.length, rc, bins, dr, A, **kw)
    assert ardf_ref.usable(want), (want["margin"], want["cos_margin"])
    return want


def _sample(e, bins, dr, A, site=False):
    e.rebin(); e.halo(); e.forces(0)
    e.rdf_config(bins, dr, site); e.rdf_config_angular(A); e.rdf_sample()
    return e.rdf_read()


@pytest.mark.parametrize("name,rc,bins,dr,A,site,rot", [
    ("synthetic_water_5.inp", 12.0, 100, 0.1213, 6, False, True),  # everything in LDS, molecule histogram from the same walk
    ("mixed5_1024", 35.0, 113, 0.3097, 7, True, True),             # 25 x 791 words: global atomics, second traversal behind k_rdf_brick
    ("bcc1clj_3456", 2.5, 97, 0.0257, 5, False, False),            # no quaternions: orientation (0, 0, 1)
])
def test_brute_force_parity(name, rc, bins, dr, A, site, rot):
    ps, s, r, q = _state(name)
    want = _want(ps, r, q if rot else None, s["cid"], rc, bins, dr, A)
    e = _engine(ps.components, rc, ps.length, s, r=r, q=q)
    got = _sample(e, bins, dr, A, site); e.close()
    assert np.array_equal(got["ardf"], want["ardf"]) and got["ardf"].sum() > 1000
    ref = rdf_ref.brute_force(r, q, s["cid"], ps.components, ps.length, rc, bins, dr, site_rdf=site)
    _assert_equal(got, ref, name)  # mol, site and n_per_component are what the RDF pass alone gives
    assert len(got["ardf"]) == 1 or any(not np.array_equal(got["ardf"][a, b], got["ardf"][b, a]) for a in range(5) for b in range(a))


def test_flat_index_quirk():
    """open box, one LJ component, orientation (0, 0, 1), coordinates on multiples of 0.25: every difference is exact.  bins 4 x 0.5,
    A = 8.  Around C: +z at 0.75 (row 1), -z at 1.75 (last row), in-plane neighbours; no other pair reaches column 0 of rows 1-3."""
    ps, s0 = _fixture("synthetic_bcc1clj_12.inp")
    r = np.array([[3, 3, 3], [3, 3, 3.75], [3, 3, 1.25], [4.25, 3, 3], [3, 1.25, 3], [2, 3, 3]], dtype=np.float64)
    s = {k: v[:6].copy() for k, v in s0.items()}
    s["ids"] = np.arange(1, 7, dtype=s0["ids"].dtype)
    L = np.array([20., 20., 20.])
    e = _engine(ps.components, 2.5, L, s, r=r, periodic=False)
    got = _sample(e, 4, 0.5, 8); e.close()
    h = got["ardf"][0, 0]
    assert h[1, 0] == 1  # C central, cos = +1: column 0 of its own row
    assert h[2, 0] == 1  # the +z neighbour central, cos = -1, a = A: row b + 1, column 0
    assert h[3, 0] == 1  # the -z neighbour central, cos = +1; C central has cos = -1 in the last row: flat = bins A, dropped
    assert h.sum() == 2 * got["mol"].sum() - 1
    assert h[2, 4] == 4 and h[3, 4] == 2  # cos = 0 is the lower edge of column A / 2: C - X and C - D in row 2, C - Y in row 3, both ways
    assert np.array_equal(h, ardf_ref.brute_force(r, None, s["cid"], 1, L, 2.5, 4, 0.5, 8, periodic=False)["ardf"][0, 0])


def test_accumulate_reset_off():
    def again():
        e.rdf_sample()
        return e.rdf_read()
    ps, s, r, q = _state("synthetic_water_5.inp")
    e = _engine(ps.components, 12.0, ps.length, s)
    e.rebin(); e.halo(); e.forces(0)
    e.rdf_config(100, 0.1213, False)
    before = again()
    e.rdf_reset()
    e.rdf_config_angular(6)
    one, two = again(), again()
    assert "ardf" not in before and one["ardf"].any() and two["samples"] == 2
    assert np.array_equal(two["ardf"], 2 * one["ardf"]) and np.array_equal(two["mol"], 2 * before["mol"])
    e.rdf_reset()
    z = e.rdf_read()
    assert z["samples"] == 0 and not z["ardf"].any() and not z["mol"].any()
    e.rdf_config_angular(1)
    off = again()
    e.close()
    assert "ardf" not in off
    _assert_equal(off, before)


def test_run_samples_with_rdf_every():
    ps, s = _fixture("synthetic_mixed5_8.inp")
    a, b = (_engine(ps.components, 35.0, ps.length, s, skin=2.5) for _ in range(2))
    for e in (a, b):
        e.rebin(); e.halo(); e.forces(0)
    a.rdf_config(113, 0.3097, True); a.rdf_config_angular(7); a.set_option("rdf_every", 1)
    a.run(0.2, 2)
    got = a.rdf_read()
    a.close()
    want = 0
    for step in (1, 2):
        b.run(0.2, 1)
        st = b.download_state()
        o = np.argsort(st["ids"])
        want = want + _want(ps, st["r"][o], st["q"][o], st["cid"][o], 35.0, 113, 0.3097, 7)["ardf"]
    b.close()
    assert got["samples"] == 2 and np.array_equal(got["ardf"], want)


def test_two_ranks_sum_to_the_single_domain():
    from test_gpu_multirank import InProcessCluster
    ps, s, r, q = _state("mixed5_1024")
    want = _want(ps, r, q, s["cid"], 35.0, 113, 0.3097, 7)
    multi = InProcessCluster(2, ps.components, 35.0, ps.length, s["ids"], r, s["v"], cid=s["cid"], q=q, D=s["D"])
    multi.forces()
    total = 0
    for e in multi.eng:
        e.rdf_config(113, 0.3097, True); e.rdf_config_angular(7); e.rdf_sample()
        total = total + e.rdf_read()["ardf"]
        e.close()
    assert np.array_equal(total, want["ardf"])


def test_golden_files_of_the_reference():
    g = ardf_ref.golden_manifest()
    ps, s, r, q = _state(g["case"])
    c = rdf_ref.cases()[g["case"]]
    _want(ps, r, q, s["cid"], c["rc"], c["bins"], c["dr"], g["angularbins"])  # the condition on the state
    e = _engine(ps.components, c["rc"], ps.length, s, r=r, q=q)
    got = _sample(e, c["bins"], c["dr"], g["angularbins"]); e.close()
    for i, j in ((0, 0), (0, 1), (1, 0), (1, 1)):
        assert np.array_equal(ardf_ref.golden_counts(i, j), got["ardf"][i, j].reshape(-1)), (i, j)

"""Cavity detection on the device (ls1hip_cavity_*, kernels_cavity.hip) against the brute-force restatement of tests/cavity_ref.py.
Counts and flags are integers: every comparison is exact equality.  Condition instead of a tolerance: in every state used no
node-molecule distance lies within EDGE_MARGIN (relative) of the search radius — asserted, never skipped."""
import functools

import numpy as np
import pytest

from cavity_ref import cavity_ref, flags_of
from conftest import load_pkg
from golden_io import input_path, manifest, sorted_phase_space

pytestmark = pytest.mark.gpu

capi = load_pkg("capi")
engine_mod = load_pkg("engine")
inp = load_pkg("inp")
decomp = load_pkg("decomp")

EDGE_MARGIN = 1e-9
CASES = ("lj_periodic", "multi_periodic", "bcc1clj_3456")
# skin, dt.  multi_periodic has no dynamics here (the manifest lists it with 0 steps; ls1hip_run refuses that state with "molecules
# left the halo region", with lists or without, before any cavity sample is taken): its list mode is sampled on the built lists
LIST_RUN = {"lj_periodic": (2.0, 2.0), "bcc1clj_3456": (0.3, 0.005)}
SKIN = {"lj_periodic": 2.0, "multi_periodic": 2.0, "bcc1clj_3456": 0.3}
FINE, SMALL = (13, 9, 7), (3, 2, 5)  # partial tiles on every face; smaller than one tile


@functools.lru_cache(maxsize=None)
def _case(name):
    c = manifest()[name]
    ps = inp.read_inp(input_path(c["input"]))
    return ps, sorted_phase_space(ps), np.asarray(ps.length, dtype=np.float64), c["rc"]


def _cv(L, restricted):
    """a control volume whose faces fall inside cells"""
    return (np.array([0.13, 0.07, 0.21]) * L, np.array([0.81, 0.93, 0.77]) * L) if restricted else None


@functools.lru_cache(maxsize=None)
def _want(name, N, radius, restricted=False, images=False):
    _, s, L, _ = _case(name)
    counts, hit, margin = cavity_ref(s["r"], s["ids"], L, N, radius, _cv(L, restricted), images)
    assert margin > EDGE_MARGIN, margin
    return counts, hit


def _engine(name, cic=1, skin=None, **options):
    ps, s, _, rc = _case(name)
    e = engine_mod.DeviceEngine(0)
    e.set_components(ps.components, rc)
    e.set_option("cells_in_cutoff", cic)
    if skin:
        e.set_verlet(skin, force=True)
    e.set_domain(ps.length)
    e.upload(s["ids"], s["cid"], s["r"], s["v"], s["q"], s["D"])
    e.rebin(); e.halo(); e.forces(0)
    for k, v in options.items():
        e.set_option(k, v)
    return e


def _sample(e, N, max_nb, radius, cv=None, counts=True):
    e.cavity_config(*N, max_nb, radius, *(cv or (None, None)))
    e.cavity_sample()
    got = e.cavity_read(counts=counts)
    assert got["n_active"] == int(got["flags"].sum()) and tuple(got["n"]) == tuple(N) and not got["lo"].any()
    return got


@pytest.mark.parametrize("lattice", [FINE, SMALL, "coarse"])
@pytest.mark.parametrize("cic", [1, 2])
@pytest.mark.parametrize("name", CASES)
def test_counts_and_flags_equal_the_restatement(name, cic, lattice):
    """R in {0.3 r_c, r_c} x {whole domain, control volume} x maxNeighbours in {1, median}; "coarse": spacing > 2 R"""
    _, _, L, rc = _case(name)
    e = _engine(name, cic, cavity_counts=1)
    for frac in (0.3, 1.0):
        for restricted in (False, True):
            cv, R = _cv(L, restricted), frac * rc
            ext = L if cv is None else cv[1] - cv[0]
            N = lattice if lattice != "coarse" else tuple(int(k) for k in np.maximum(1, np.floor(ext / (2.0001 * R))))
            want, hit = _want(name, N, R, restricted)
            if N == FINE and frac == 1.0 and not restricted:
                # parity below means something: the id clash changes counts here, and so does the absence of periodic images
                assert (hit.sum(axis=1) != want.reshape(-1)).any() and (_want(name, N, R, images=True)[0] != want).any()
            seen = set()
            for max_nb in (1, max(1, int(np.median(want)))):
                got = _sample(e, N, max_nb, R, cv)
                assert np.array_equal(got["counts"], want), (frac, restricted, N, int((got["counts"] != want).sum()))
                assert np.array_equal(got["flags"], flags_of(want, max_nb))
                seen |= set(np.unique(got["flags"]))
            assert seen == {0, 1}  # cavities and filled nodes both occur
    e.close()


@pytest.mark.parametrize("name", CASES)
def test_flag_mode_equals_count_mode_and_small_chunks_change_nothing(name):
    """flag mode (early exit) against count mode; cavity_chunk = 64 on a lattice whose ONE tile has more than 64 candidates"""
    _, _, L, rc = _case(name)
    e = _engine(name)
    for N, max_nb in ((FINE, 1), (FINE, 14), (SMALL, 16)):
        want, hit = _want(name, N, rc)
        for chunk in (0, 64):
            e.set_option("cavity_chunk", chunk)
            for counts in (0, 1):
                e.set_option("cavity_counts", counts)
                got = _sample(e, N, max_nb, rc, counts=bool(counts))
                assert np.array_equal(got["flags"], flags_of(want, max_nb)), (N, max_nb, chunk, counts)
                assert not counts or np.array_equal(got["counts"], want)
        assert N != SMALL or hit.any(axis=0).sum() > 64  # every candidate of the one tile is in one chunk otherwise
    with pytest.raises(capi.Ls1HipError, match="count mode"):
        e.set_option("cavity_counts", 0); e.cavity_sample(); e.cavity_read(counts=True)
    e.close()


def _ref_now(e, L, N, radius):
    st = e.download_state()
    counts, _, margin = cavity_ref(st["r"], st["ids"], L, N, radius)
    assert margin > EDGE_MARGIN, margin
    return counts


@pytest.mark.parametrize("name", CASES)
def test_list_mode_on_the_built_lists(name):
    """the grid of r_c + skin, lists built, halo positions refreshed: the cell walk widened by the skin finds the same neighbours"""
    rc = _case(name)[3]
    e = _engine(name, skin=SKIN[name], cavity_counts=1)
    e.verlet_build()
    e.halo_refresh()
    got = _sample(e, FINE, 14, rc)
    e.close()
    assert np.array_equal(got["counts"], _want(name, FINE, rc)[0])


@pytest.mark.parametrize("name", sorted(LIST_RUN))
def test_list_mode_and_run_series(name):
    """between list builds: the sample equals the restatement on the downloaded positions wrapped into the box; cavity_every = 2,
    cavity_from = 3 over six steps samples steps 4 and 6, equals separate samples, and leaves the trajectory bit-identical"""
    _, _, L, rc = _case(name)
    (skin, dt), N, max_nb = LIST_RUN[name], FINE, 14
    a = _engine(name, skin=skin, cavity_counts=1)
    a.cavity_config(*N, max_nb, rc)
    a.set_option("cavity_every", 2)
    a.set_option("cavity_from", 3)
    a.run(dt, 6)
    series, last, end_a = a.cavity_series(), a.cavity_read(counts=True), a.download_state()
    a.close()
    b = _engine(name, skin=skin, cavity_counts=1)
    b.cavity_config(*N, max_nb, rc)
    want = []
    for step in range(1, 7):
        b.run(dt, 1)
        if step in (4, 6):
            b.cavity_sample()
            ref = _ref_now(b, L, N, rc)
            got = b.cavity_read(counts=True)
            assert np.array_equal(got["counts"], ref), int((got["counts"] != ref).sum())
            want.append(int(flags_of(ref, max_nb).sum()))
    end_b = b.download_state()
    b.close()
    assert [int(k) for k in series] == want
    assert np.array_equal(last["counts"], ref)
    oa, ob = np.argsort(end_a["ids"]), np.argsort(end_b["ids"])
    assert np.array_equal(end_a["r"][oa], end_b["r"][ob]) and np.array_equal(end_a["v"][oa], end_b["v"][ob])


def test_refusals_leave_the_context_usable():
    name = "lj_periodic"
    _, _, L, rc = _case(name)
    e = _engine(name)
    for args, msg in (((4, 4, 4, 3, 1.01 * rc), "exceeds the cutoff"), ((4, 4, 4, 0, rc), "maxNeighbours"), ((4, 0, 4, 3, rc), "Nx, Ny, Nz"),
                      ((4, 4, 4, 3, 0.0), "radius"), ((2048, 2048, 1024, 3, rc), "node ids"),
                      ((4, 4, 4, 3, rc, np.zeros(3), 1.01 * L), "leaves the domain")):
        with pytest.raises(capi.Ls1HipError, match=msg):
            e.cavity_config(*args)
    e.set_option("cavity_every", 1)
    with pytest.raises(capi.Ls1HipError, match="cavity_every"):
        e.run(2.0, 1)
    e.set_option("cavity_every", 0)
    got = _sample(e, SMALL, 16, rc, counts=False)
    e.close()
    assert np.array_equal(got["flags"], flags_of(_want(name, SMALL, rc)[0], 16))


@pytest.mark.parametrize("name", CASES)
def test_two_sub_domains_partition_the_lattice_and_join_to_the_single_domain(name):
    """halo copies from the neighbouring rank lie inside the global box and count; periodic images do not"""
    from test_gpu_multirank import InProcessCluster
    ps, s, L, rc = _case(name)
    N, max_nb = FINE, 14
    want = _want(name, N, rc)[0]
    multi = InProcessCluster(2, ps.components, rc, L, s["ids"], s["r"], s["v"], cid=s["cid"], q=s["q"], D=s["D"])
    multi.forces()
    pieces, total = [], 0
    for e in multi.eng:
        e.cavity_config(*N, max_nb, rc)
        e.cavity_sample()
        loc = decomp.cavity_collect(e, N)  # no process group: the local piece; across processes the same call gathers them
        pieces += loc["pieces"]
        total += loc["n_active"]
        e.close()
    assert all(0 < int(np.prod(n)) < int(np.prod(N)) for _, n, _ in pieces)
    glob = decomp.cavity_assemble(pieces, N, total)  # raises unless the ranges partition the lattice
    assert np.array_equal(glob["flags"], flags_of(want, max_nb)) and glob["n_active"] == int(flags_of(want, max_nb).sum())

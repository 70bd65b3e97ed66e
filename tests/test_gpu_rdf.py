"""RDF sampling on the device (ls1hip_rdf_*, kernels_rdf.hip) against the reference's files (tests/golden/rdf/) and against the
brute-force restatement that tests/test_rdf_cpu.py pins to them (tests/rdf_ref.py).  Counts are integers: every comparison is exact
equality.  Every state used satisfies the edge condition (no distance within 1e-8 of a bin edge, r_c or bins * dr)."""
import os
import socket
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import rdf_ref
from conftest import ROOT, load_pkg
from golden_io import input_path, sorted_phase_space

pytestmark = pytest.mark.gpu

capi = load_pkg("capi")
engine_mod = load_pkg("engine")
inp = load_pkg("inp")
mirror = load_pkg("mirror")


def _engine(comps, rc, L, s, r=None, q=None, kernel=0, skin=None, periodic=True, options=()):
    e = engine_mod.DeviceEngine(0)
    e.set_components(comps, rc)
    e.set_option("force_kernel", kernel)
    for k, v in options:
        e.set_option(k, v)
    if skin:
        e.set_verlet(skin)
    e.set_domain(L, periodic=periodic)
    e.upload(s["ids"], s["cid"], s["r"] if r is None else r, s["v"], s["q"] if q is None else q, s["D"])
    return e


def _fixture(fname):
    ps = inp.read_inp(input_path(fname))
    return ps, sorted_phase_space(ps)


def _case_engine(case, step, **kw):
    cs = rdf_ref.case_states(case)
    ps, st = cs["ps"], cs["states"][step - 1]
    s = sorted_phase_space(ps)
    return _engine(ps.components, cs["case"]["rc"], ps.length, s, r=st["r"], q=st["q"], **kw), cs


def _assert_equal(got, want, what=""):
    assert got["mol"].shape == want["mol"].shape, what
    assert np.array_equal(got["mol"], want["mol"]), (what, int(np.abs(got["mol"].astype(np.int64) - want["mol"].astype(np.int64)).sum()))
    assert len(got["site"]) == len(want["site"]), what
    for k, (a, b) in enumerate(zip(got["site"], want["site"])):
        assert np.array_equal(a, b), (what, "site block", k)
    assert np.array_equal(got["n_per_component"], want["n_per_component"]), what
    assert got["samples"] == want["samples"], what


def _sample_once(e, bins, dr, site=True):
    e.rebin(); e.halo(); e.forces(0)
    e.rdf_config(bins, dr, site)
    e.rdf_sample()
    return e.rdf_read()


# ---- 1. the golden cases of the real reference -------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,step,kernel", [("bcc1clj_3456", 1, k) for k in range(5)] + [("bcc1clj_3456", 2, 0), ("bcc1clj_3456", 3, 0)] +
                         [(c, s, 0) for c in ("twotherm_1024", "mixed5_1024") for s in (1, 2, 3)])
def test_golden_cases_of_the_reference(case, step, kernel):
    e, cs = _case_engine(case, step, kernel=kernel)
    c = cs["case"]
    nC = len(cs["ps"].components.components)
    got = _sample_once(e, c["bins"], c["dr"])
    e.close()
    mol, ctr = rdf_ref.golden_mol_counts(case, nC, c["bins"], step)
    assert np.array_equal(got["mol"], mol)
    assert np.array_equal(got["n_per_component"], ctr) and got["samples"] == 1
    # the site columns of the files are normalised values (pinned by tests/test_rdf_cpu.py through the writer): the raw site counts
    # are compared with the restatement that reproduces the files
    want = rdf_ref.case_counts(case, step)
    assert want["margin"] >= rdf_ref.EDGE_MARGIN
    _assert_equal(got, want, (case, step, kernel))


@pytest.mark.parametrize("case", ["twotherm_1024", "mixed5_1024"])
def test_mirror_rdf_plugin_writes_the_reference_files_from_the_device(case, tmp_path):
    """LinkedCells.traverseCells(RDFCellProcessor) -> RDF.endStep: the files of step 1, fields as the reference printed them"""
    from test_rdf_cpu import _same_number
    cs = rdf_ref.case_states(case)
    ps, c, st = cs["ps"], cs["case"], cs["states"][0]
    s = sorted_phase_space(ps)
    cont = mirror.LinkedCells(np.zeros(3), ps.length, c["rc"], components=ps.components, device=0)
    dom = mirror.Domain(ps.length)
    cont.addParticles(s["ids"], s["cid"], st["r"], s["v"], st["q"], s["D"])
    cont.update(); mirror.DomainDecompBase().balanceAndExchange(0., False, cont, dom)
    cont.traverseCells(mirror.VectorizedCellProcessor(dom, c["rc"], c["rc"]))
    rdf = mirror.RDF(ps.components, c["rc"], writefrequency=1, samplingfrequency=1, outputprefix="rdf", bins=c["bins"], intervallength=c["dr"])
    rdf.afterForces(cont, None, 1)
    rdf.endStep(cont, None, dom, 1, directory=str(tmp_path))
    nC = len(ps.components.components)
    for i in range(nC):
        for j in range(i, nC):
            got = (tmp_path / ("rdf_%d-%d.%09d.rdf" % (i, j, 1))).read_text().split()
            want = rdf_ref.golden_text(case, i, j, 1).split()
            assert len(got) == len(want)
            for a, b in zip(got, want):
                assert (_same_number(a, b) if rdf_ref.is_number(a) and rdf_ref.is_number(b) else a == b), (i, j, a, b)
    assert rdf._engine.rdf_read()["samples"] == 0  # RDF::reset after the write
    cont.engine.close()


# ---- 2. brute-force parity where no golden exists ------------------------------------------------------------------------------------
@pytest.mark.parametrize("fname,rc,bins,dr,periodic", [
    ("VectorizationMultiComponentMultiPotentials.inp", 35.0, 113, 0.3097, False),
    ("VectorizationMultiComponentMultiPotentials.inp", 35.0, 113, 0.3097, True),
    ("synthetic_water_5.inp", 12.0, 100, 0.1213, True),        # one component with several sites: the same-component m != n path
    ("Ethan_equilibrated.inp", 32.1254, 113, 0.2843, True),    # N = 9826
    ("synthetic_bcc1clj_16.inp", 2.5, 97, 0.0257, True),       # 8 cells per edge: full bricks
])
def test_brute_force_parity(fname, rc, bins, dr, periodic):
    ps, s = _fixture(fname)
    want = rdf_ref.brute_force(s["r"], s["q"], s["cid"], ps.components, ps.length, rc, bins, dr, periodic)
    assert want["margin"] >= rdf_ref.EDGE_MARGIN
    e = _engine(ps.components, rc, ps.length, s, periodic=periodic)
    got = _sample_once(e, bins, dr)
    e.close()
    _assert_equal(got, want, fname)
    assert int(got["mol"].sum()) > 1000


# ---- 3. cut rules ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bins,dr", [(76, 0.025), (124, 0.025), (1, 1.3)])
def test_cut_rules(bins, dr):
    """bins * dr = 1.9 < r_c: the distance cap is active; 3.1 > r_c: bins above r_c stay empty; one bin only"""
    e, cs = _case_engine("bcc1clj_3456", 1)
    st = cs["states"][0]
    want = rdf_ref.brute_force(st["r"], st["q"], cs["cid"], cs["ps"].components, cs["ps"].length, 2.5, bins, dr)
    assert want["margin"] >= rdf_ref.EDGE_MARGIN
    got = _sample_once(e, bins, dr)
    e.close()
    _assert_equal(got, want, (bins, dr))
    if bins * dr > 2.5:
        first_above = int(np.floor(2.5 / dr)) + 1
        inside = rdf_ref.brute_force(st["r"], st["q"], cs["cid"], cs["ps"].components, cs["ps"].length, 2.5, 1, 2.5)["mol"].sum()
        assert got["mol"][:, first_above:].sum() == 0 and got["mol"].sum() == inside  # every pair inside r_c, none above
    else:
        assert 0 < got["mol"].sum() < rdf_ref.case_counts("bcc1clj_3456", 1)["mol"].sum()


def test_site_rdf_off_on_a_multi_site_set():
    e, cs = _case_engine("mixed5_1024", 1)
    c = cs["case"]
    got = _sample_once(e, c["bins"], c["dr"], site=False)
    assert e.rdf_layout() == (15 * c["bins"], 0)
    e.close()
    assert got["site"] == [] and np.array_equal(got["mol"], rdf_ref.case_counts("mixed5_1024", 1)["mol"])


def test_molecule_histogram_beyond_the_lds_budget():
    """fifteen component pairs at 226 bins do not fit the workgroup's histogram: every count goes to global atomics, same integers"""
    e, cs = _case_engine("mixed5_1024", 1)
    st = cs["states"][0]
    want = rdf_ref.brute_force(st["r"], st["q"], cs["cid"], cs["ps"].components, cs["ps"].length, 35.0, 226, 0.15485)
    assert want["margin"] >= rdf_ref.EDGE_MARGIN
    got = _sample_once(e, 226, 0.15485)
    e.close()
    _assert_equal(got, want)


# ---- 4. partial bricks and thin domains -------------------------------------------------------------------------------------------------
def test_thin_domain_two_cells_deep():
    """a slab of the bcc box, four lattice planes (two cells) deep and periodic: every brick is partial in z"""
    cs = rdf_ref.case_states("bcc1clj_3456")
    ps, st = cs["ps"], cs["states"][0]
    a = ps.length[0] / 12
    m = st["r"][:, 2] < 4 * a
    L = np.array([ps.length[0], ps.length[1], 4 * a])
    s0 = sorted_phase_space(ps)
    s = {k: v[m] for k, v in s0.items()}
    want = rdf_ref.brute_force(st["r"][m], st["q"][m], s["cid"], ps.components, L, 2.5, 97, 0.0257)
    assert want["margin"] >= rdf_ref.EDGE_MARGIN
    e = _engine(ps.components, 2.5, L, s, r=st["r"][m], q=st["q"][m])
    assert list(e.grid()[0]) == [8, 8, 4]  # 6 x 6 x 2 cells + halo
    got = _sample_once(e, 97, 0.0257)
    e.close()
    _assert_equal(got, want)


# ---- 5. accumulation, reset, counters ---------------------------------------------------------------------------------------------------
def test_accumulation_reset_and_switching_off():
    e, cs = _case_engine("mixed5_1024", 1)
    c = cs["case"]
    one = _sample_once(e, c["bins"], c["dr"])
    e.rdf_sample()
    two = e.rdf_read()
    assert two["samples"] == 2 and np.array_equal(two["n_per_component"], 2 * one["n_per_component"])
    assert np.array_equal(two["mol"], 2 * one["mol"]) and all(np.array_equal(b, 2 * a) for a, b in zip(one["site"], two["site"]))
    e.rdf_reset()
    z = e.rdf_read()
    assert z["samples"] == 0 and not z["mol"].any() and not z["n_per_component"].any() and not any(b.any() for b in z["site"])
    e.rdf_sample()
    _assert_equal(e.rdf_read(), one)
    e.rdf_config(0, 0.0)  # off: buffers freed
    assert e.rdf_layout() == (0, 0)
    e.rebin(); e.halo(); u1 = e.forces(0)
    F1 = e.download_forces()
    e.close()
    f, _ = _case_engine("mixed5_1024", 1)  # a fresh engine that never sampled
    f.rebin(); f.halo(); u0 = f.forces(0)
    F0 = f.download_forces()
    f.close()
    assert u0 == u1 and np.array_equal(F0["F"], F1["F"]) and np.array_equal(F0["M"], F1["M"])


# ---- 6. ls1hip_run with rdf_every ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fname,rc,dt,skin,every,nsteps,bins,dr,options", [
    # the production list configuration of smoke(); 25 bins: at N = 16000 with ~100 bins about every third state has some distance
    # within 1e-8 of an edge — this width keeps steps 3 and 6 (and step 1, below) clear by 4e-8 and more
    ("synthetic_bcc1clj_20.inp", 2.5, 0.005, 0.2, 3, 6, 25, 0.0997, ()),
    ("synthetic_mixed5_8.inp", 35.0, 0.2, 2.5, 1, 3, 113, 0.3097, ()),          # multi-site list mode
    ("synthetic_bcc1clj_12.inp", 2.5, 0.005, None, 1, 3, 97, 0.0257, ()),       # fused per-step loop
    ("synthetic_bcc1clj_12.inp", 2.5, 0.005, None, 2, 4, 97, 0.0257, (("overlap_halo", 1),)),
])
def test_run_samples_every_nth_step(fname, rc, dt, skin, every, nsteps, bins, dr, options):
    ps, s = _fixture(fname)
    a = _engine(ps.components, rc, ps.length, s, skin=skin, options=options)
    a.rebin(); a.halo(); a.forces(0)
    a.rdf_config(bins, dr, True)
    a.set_option("rdf_every", every)
    a.run(dt, nsteps)
    got = a.rdf_read()
    if skin:
        assert a.get_option("last_force_kernel") == capi.FK_NEIGHBOUR_LIST
    a.close()
    b = _engine(ps.components, rc, ps.length, s, skin=skin, options=options)
    b.rebin(); b.halo(); b.forces(0)
    want = None
    for step in range(1, nsteps + 1):
        b.run(dt, 1)
        if step % every:
            continue
        st = b.download_state()
        o = np.argsort(st["ids"])
        cnt = rdf_ref.brute_force(st["r"][o], st["q"][o], st["cid"][o], ps.components, ps.length, rc, bins, dr)
        assert cnt["margin"] >= rdf_ref.EDGE_MARGIN, (step, cnt["margin"])
        want = cnt if want is None else rdf_ref.add_counts(want, cnt)
    b.close()
    assert want["samples"] == nsteps // every
    _assert_equal(got, want, fname)


def test_run_with_rdf_every_but_no_configuration_is_an_error():
    e, _ = _case_engine("bcc1clj_3456", 1)
    e.rebin(); e.halo(); e.forces(0)
    e.set_option("rdf_every", 1)
    with pytest.raises(capi.Ls1HipError, match="rdf_every"):
        e.run(0.005, 1)
    e.set_option("rdf_every", 0)
    e.run(0.005, 1)
    e.close()


def test_sample_between_list_builds():
    """piecewise list loop: ls1hip_update refreshes the halo while the bins are stale; the sample sees the current positions"""
    ps, s = _fixture("synthetic_bcc1clj_20.inp")
    e = _engine(ps.components, 2.5, ps.length, s, skin=0.2)
    e.rebin(); e.halo(); e.forces(0)
    e.verlet_build()
    e.rdf_config(25, 0.0997, True)
    e.kick_drift(0.005)
    with pytest.raises(capi.Ls1HipError, match="halo"):
        e.rdf_sample()  # drifted: the halo copies are not current
    assert e.update() is False  # no rebuild: stale bins, refreshed halo
    e.rdf_sample()
    got = e.rdf_read()
    st = e.download_state()
    e.close()
    o = np.argsort(st["ids"])
    assert np.max(np.abs(st["r"][o] - s["r"])) > 1e-3  # the molecules moved since the bins were made
    want = rdf_ref.brute_force(st["r"][o], st["q"][o], st["cid"][o], ps.components, ps.length, 2.5, 25, 0.0997)
    assert want["margin"] >= rdf_ref.EDGE_MARGIN
    _assert_equal(got, want)


# ---- 7. multi-rank ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,world", [("bcc1clj_3456", 2), ("bcc1clj_3456", 8), ("mixed5_1024", 2), ("mixed5_1024", 8)])
def test_sub_boxes_sum_to_the_single_domain(case, world):
    from test_gpu_multirank import InProcessCluster
    cs = rdf_ref.case_states(case)
    ps, c, st = cs["ps"], cs["case"], cs["states"][0]
    s = sorted_phase_space(ps)
    multi = InProcessCluster(world, ps.components, c["rc"], ps.length, s["ids"], st["r"], s["v"], cid=s["cid"], q=st["q"], D=s["D"])
    multi.forces()
    total = None
    for e in multi.eng:
        e.rdf_config(c["bins"], c["dr"], True)
        e.rdf_sample()
        loc = e.rdf_read()
        loc["margin"] = np.inf
        total = loc if total is None else rdf_ref.add_counts(total, loc)
        e.close()
    total["samples"] = 1  # every rank ticks once; RDF::collectRDF does not sum the ticks
    _assert_equal(total, rdf_ref.case_counts(case, 1), (case, world))


def test_rdf_collect_over_two_processes():
    cs = rdf_ref.case_states("bcc1clj_3456")
    ps, c, st = cs["ps"], cs["case"], cs["states"][0]
    s = sorted_phase_space(ps)
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    with tempfile.TemporaryDirectory() as td:
        inp_path, out_path = os.path.join(td, "in.npz"), os.path.join(td, "out.npz")
        np.savez(inp_path, L=ps.length, r=st["r"], v=s["v"], ids=s["ids"], rc=c["rc"], bins=c["bins"], dr=c["dr"])
        env = dict(os.environ, LS1_TEST_INPUT=inp_path, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="1")
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
               "--master-port", str(port), os.path.join(ROOT, "tests", "rdf_gpu_worker.py"), out_path]
        res = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
        assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
        z = np.load(out_path)
        want = rdf_ref.case_counts("bcc1clj_3456", 1)
        assert np.array_equal(z["mol"], want["mol"]) and np.array_equal(z["n"], want["n_per_component"]) and int(z["samples"]) == 1
        assert 0 < z["local_mol"].sum() < z["mol"].sum() and 0 < z["local_n"].sum() < z["n"].sum()


# ---- 8. errors ------------------------------------------------------------------------------------------------------------------------------
def test_errors_leave_the_context_usable():
    e, cs = _case_engine("bcc1clj_3456", 1)
    c = cs["case"]
    with pytest.raises(capi.Ls1HipError, match="not configured") as ei:
        e.rdf_sample()
    assert ei.value.code != 0
    for bins, dr in ((-3, 0.1), (10, 0.0), (10, -1.0), (10, float("inf"))):
        with pytest.raises(capi.Ls1HipError, match="bins|interval_length|finite"):
            e.rdf_config(bins, dr)
    e.rdf_config(c["bins"], c["dr"])
    e.rebin()
    with pytest.raises(capi.Ls1HipError, match="halo"):
        e.rdf_sample()  # binned, but no halo yet
    e.halo()
    e.rdf_sample()
    got = e.rdf_read()
    e.close()
    _assert_equal(got, rdf_ref.case_counts("bcc1clj_3456", 1))
    f = engine_mod.DeviceEngine(0)
    with pytest.raises(capi.Ls1HipError, match="components"):
        f.rdf_config(10, 0.1)  # neither components nor domain
    f.close()


def test_rdf_timer():
    e, cs = _case_engine("bcc1clj_3456", 1)
    e.timing_enable(1)
    _sample_once(e, 97, 0.0257)
    ms, n = e.timing("rdf")
    e.close()
    assert n == 1 and ms > 0.0

"""RDF without a GPU: (1) the brute-force restatement the GPU tests use as their yardstick (tests/rdf_ref.py) reproduces every
integer the REAL reference wrote (tests/golden/rdf/, made by tests/golden/make_rdf_golden.py from the unmodified driver with
its RDF plugin); (2) mirror.RDF.writeToFile, fed with those counts, reproduces the reference's .rdf files."""
import math

import numpy as np
import pytest

import rdf_ref
from conftest import load_pkg

CASES = sorted(rdf_ref.cases())


def test_golden_cases_are_the_three_of_the_manifest():
    assert CASES == ["bcc1clj_3456", "mixed5_1024", "twotherm_1024"]
    for c in rdf_ref.cases().values():
        assert c["steps"] == 3


@pytest.mark.parametrize("case", CASES)
def test_restatement_reproduces_the_reference_counts(case):
    cs = rdf_ref.case_states(case)
    c = cs["case"]
    nC = len(cs["ps"].components.components)
    for step in range(1, c["steps"] + 1):
        cnt = rdf_ref.case_counts(case, step)
        # the condition under which last-bit differences of dd cannot move a count (molecule AND site distances)
        assert cnt["margin"] >= rdf_ref.EDGE_MARGIN, (case, step, cnt["margin"])
        mol, ctr = rdf_ref.golden_mol_counts(case, nC, c["bins"], step)
        assert np.array_equal(cnt["mol"], mol), (case, step)
        assert np.array_equal(cnt["n_per_component"], ctr), (case, step)
        assert int(mol.max()) < 10 ** 5  # Npair(curr.) is exact at precision(5)


def _same_number(a: str, b: str) -> bool:
    """two printed numbers agree within one unit of the fifth significant digit (what precision(5) prints)"""
    x, y = float(a), float(b)
    if x == y:
        return True
    top = max(abs(x), abs(y))
    unit = 10.0 ** (math.floor(math.log10(top)) - 4)
    return abs(x - y) <= unit * (1 + 1e-9)


@pytest.mark.parametrize("case", CASES)
def test_mirror_rdf_writes_the_reference_files(case, tmp_path):
    mirror = load_pkg("mirror")
    cs = rdf_ref.case_states(case)
    c, comps = cs["case"], cs["ps"].components
    nC = len(comps.components)
    dom = mirror.Domain(cs["ps"].length)
    rdf = mirror.RDF(comps, c["rc"], writefrequency=1, samplingfrequency=1, outputprefix="rdf", bins=c["bins"], intervallength=c["dr"])
    assert rdf.isEnabledSiteRDF() == any(x.n_sites > 1 for x in comps.components)
    for step in range(1, c["steps"] + 1):
        rdf.setGlobal(rdf_ref.case_counts(case, step))  # what RDF::collectRDF leaves
        rdf.accumulateRDF()
        for i in range(nC):
            for j in range(i, nC):
                out = tmp_path / ("rdf_%d-%d.%09d.rdf" % (i, j, step))
                rdf.writeToFile(dom, str(out), i, j)
                got = out.read_text().split("\n")
                want = rdf_ref.read_rdf(rdf_ref.golden_text(case, i, j, step))["lines"]
                assert len(got) == len(want), (case, i, j, step)
                for ln, (g, w) in enumerate(zip(got, want)):
                    # same fields (tabs and blanks are part of the format), non-numeric ones identical
                    gt, wt = g.replace("\t", " \t ").split(" "), w.replace("\t", " \t ").split(" ")
                    assert len(gt) == len(wt), (case, i, j, step, ln, g[:200], w[:200])
                    for a, b in zip(gt, wt):
                        if rdf_ref.is_number(a) and rdf_ref.is_number(b):
                            assert _same_number(a, b), (case, i, j, step, ln, a, b)
                        else:
                            assert a == b, (case, i, j, step, ln, a, b)
        rdf.reset()


def test_angular_rdf_is_refused():
    mirror = load_pkg("mirror")
    comps = rdf_ref.case_states("bcc1clj_3456")["ps"].components
    with pytest.raises(NotImplementedError):
        mirror.RDF(comps, 2.5, bins=10, intervallength=0.1, angularbins=4)

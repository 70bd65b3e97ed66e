"""The angular RDF without a GPU: the restatement the GPU tests use (tests/ardf_ref.py) reproduces every integer of the .ardf files
the REAL reference wrote (tests/golden/ardf/), and mirror.ARDF.writeToFileARDF, fed with those counts, reproduces a file."""
import numpy as np

import ardf_ref
import rdf_ref
from conftest import load_pkg
from test_rdf_cpu import _same_number


def test_restatement_and_writer_reproduce_the_reference_files(tmp_path):
    mirror = load_pkg("mirror")
    g = ardf_ref.golden_manifest()
    cs = rdf_ref.case_states(g["case"])
    c, st, A = cs["case"], cs["states"][g["step"] - 1], g["angularbins"]
    want = ardf_ref.brute_force(st["r"], st["q"], cs["cid"], 2, cs["ps"].length, c["rc"], c["bins"], c["dr"], A)
    assert ardf_ref.usable(want)
    for i, j in ((0, 0), (0, 1), (1, 0), (1, 1)):
        assert np.array_equal(ardf_ref.golden_counts(i, j), want["ardf"][i, j].reshape(-1)), (i, j)
    ardf = mirror.ARDF(cs["ps"].components, c["rc"], bins=c["bins"], intervallength=c["dr"], angularbins=A, outputprefix="rdf")
    ardf.setGlobal(dict(rdf_ref.case_counts(g["case"], g["step"]), ardf=want["ardf"]))
    ardf.accumulateRDF()
    ardf.writeToFileARDF(mirror.Domain(cs["ps"].length), str(tmp_path / "a.ardf"), 0, 1)
    got, ref = (tmp_path / "a.ardf").read_text().split("\n"), ardf_ref.golden_text(0, 1).split("\n")
    assert len(got) == len(ref)
    for a, b in zip(got, ref):
        ta, tb = a.replace("\t", " \t ").split(" "), b.replace("\t", " \t ").split(" ")
        assert len(ta) == len(tb), (a, b)
        for x, y in zip(ta, tb):
            assert (_same_number(x, y) if rdf_ref.is_number(x) and rdf_ref.is_number(y) else x == y), (a, b)

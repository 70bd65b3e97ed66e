"""CPU side of the planar long-range correction: mirror.Planar's writer against the file the reference driver wrote, from
tests/planar_ref.py tables.  (The argument rules of the ABI need a context, i.e. a device: tests/test_gpu_planar.py.)"""
import os

import numpy as np
import pytest

import planar_ref
from conftest import load_pkg

mirror = load_pkg("mirror")


@pytest.mark.parametrize("name", list(planar_ref.cases()))
def test_writer_reproduces_the_reference_file(name, tmp_path):
    c = planar_ref.golden(name)
    ps, want = c["ps"], c["files"]["LRC_TS000000001.dat"]
    pl = planar_ref.Planar(ps.components, ps.length, c["rc"], c["slabs"], temperature=c["temp"])
    T = pl.tables(pl.counts(ps.cid, ps.r, ps.q))
    w = mirror.Planar(ps.length, slabs=c["slabs"], frequency=c["freq"], start=1, writefrequency=1, stop=4)
    path = w.writeProfiles(1, str(tmp_path), {k: T[k][:pl.nljsum] for k in ("rho", "f", "u")})
    assert os.path.basename(path) == "LRC_TS000000001.dat" and w.writeProfiles(5, str(tmp_path), T) is None
    gl, wl = open(path).read().splitlines(), want.splitlines()
    assert gl[0] == wl[0] and len(gl) == len(wl)
    for a, b in zip(gl[1:], wl[1:]):  # same layout; pos and rho to every digit, F and u to the restatement's proven 1e-10
        assert len(a) == len(b) and a[:48] == b[:48]
        np.testing.assert_allclose([float(x) for x in a.split()], [float(x) for x in b.split()], rtol=0, atol=1e-10 * np.abs(T["f"]).max())


def test_write_control_rules():
    with pytest.raises(ValueError):
        mirror.Planar((1, 1, 1), start=5, stop=5)
    with pytest.raises(ValueError):
        mirror.Planar((1, 1, 1), writefrequency=0)
    assert mirror.Planar((1, 7.5, 1), region=(1.0, "box"))._region == (1.0, 7.5)

"""Spatial profiles without a GPU: (1) the restatement the GPU tests use as their yardstick (tests/profile_ref.py) reproduces the
files the REAL reference wrote (tests/golden/profile/, made by tests/golden/make_profile_golden.py from the unmodified driver with
two instances of its SpatialProfile plugin); (2) mirror.SpatialProfile's writers, fed with the restatement's tables, reproduce
those files token by token; (3) header, binding and library agree on the five entry points."""
import os
import re
import subprocess

import numpy as np
import pytest

import profile_ref
from conftest import ROOT, load_pkg

CASES = sorted(profile_ref.cases())
WRITTEN = [(c, k, last) for c in CASES for k in range(2) for last in (2, 4)]
FUNCTIONS = ["ls1hip_profile_config", "ls1hip_profile_layout", "ls1hip_profile_read", "ls1hip_profile_reset", "ls1hip_profile_sample"]


def test_golden_cases_are_the_two_of_the_manifest():
    assert CASES == ["bcc1clj_3456", "mixed5_1024"]
    cs = profile_ref.cases()
    for c in cs.values():
        assert c["steps"] == 4 and [i["prefix"] for i in c["instances"]] == ["cart", "cyl"]
        assert c["instances"][0]["units"] == (3, 5, 7) and c["instances"][1]["units"] == (4, 5, 3)
    assert cs["mixed5_1024"]["instances"][1]["component"] == 1 and cs["bcc1clj_3456"]["instances"][1]["component"] == -1


def _g6(x):
    return "%.6g" % float(x)


@pytest.mark.parametrize("case,instance,last", WRITTEN)
def test_restatement_reproduces_the_reference_files(case, instance, last):
    cs = profile_ref.case_states(case)
    ins = cs["case"]["instances"][instance]
    t = profile_ref.case_tables(case, instance, last - 1, last)
    info, acc = t["info"], t["samples"]
    assert acc == 2
    # the condition under which last-bit differences of a bin coordinate cannot move a molecule
    assert t["margin"] >= profile_ref.EDGE_MARGIN, (case, ins["prefix"], last, t["margin"])
    assert int(t["n"].max()) < 10 ** 5  # six digits carry the count exactly
    text = lambda suffix: profile_ref.golden_text(case, ins["prefix"], last, suffix)  # noqa: E731
    # density: entry * segment volume * data sets is the integer count
    dens = profile_ref.read_matrix(text(".NDpr"), info)
    cnt = dens * info["segment_volume"] * acc
    assert np.all(np.abs(cnt - np.round(cnt)) <= 1e-5 * np.maximum(np.round(cnt), 1.0) + 1e-9)
    assert np.array_equal(np.round(cnt).astype(np.uint64), t["n"])
    n = t["n"].astype(np.float64)
    with np.errstate(all="ignore"):
        want = {
            ".Temppr": (np.where(t["dof"] != 0, t["ekin"] / np.where(t["dof"] != 0, t["dof"], 1).astype(np.float64), 0.0), 1),
            ".VAbspr": (np.where(n != 0, t["vabs"] / np.where(n != 0, n, 1), 0.0), 1),
            ".V3Dpr": (np.where(n[:, None] != 0, t["v3"] / np.where(n != 0, n, 1)[:, None], 0.0), 3),
        }
    for suffix, (val, per) in want.items():
        got = profile_ref.read_matrix(text(suffix), info, per)
        for a, b in zip(np.asarray(got).reshape(-1), np.asarray(val).reshape(-1)):
            assert profile_ref.same_number(_g6(a), _g6(b)), (case, ins["prefix"], last, suffix, a, b)
    # partial pressures: the layer sums of VirialProfile::output
    rows = [ln.split() for ln in text("_1D-Y.Vipr").split("\n") if ln and not ln.startswith(("/", "#", "\t", "0 "))]
    u, L = info["units"], cs["ps"].length
    assert len(rows) == u[1]
    T = np.longdouble(cs["states"][last - 1]["temperature"])
    height = L[1] / u[1]
    vol = height * np.pi * (L[0] / 2) ** 2 if ins["mode"] == profile_ref.CYLINDER else height * L[0] * L[2]
    for y, row in enumerate(rows):
        if ins["mode"] == profile_ref.CYLINDER:
            ids = [y * u[0] * u[2] + a * u[2] + b for a in range(u[0]) for b in range(u[2])]
        else:
            ids = [a * u[1] * u[2] + y * u[2] + b for a in range(u[0]) for b in range(u[2])]
        P = t["ld_vi3"][ids].sum(axis=0)
        Ny = np.longdouble(int(t["n"][ids].sum()))
        den = np.longdouble(vol * acc)
        vals = [(y + 0.5) / info["inv"][1], (P[1] - np.longdouble(.5) * (P[0] + P[2])) / den] + [(T * Ny + P[d]) / den for d in range(3)]
        assert len(row) == 5
        for a, b in zip(row, vals):
            assert profile_ref.same_number(a, _g6(b)), (case, ins["prefix"], last, y, a, float(b))


@pytest.mark.parametrize("case,instance,last", WRITTEN)
def test_mirror_writers_reproduce_the_reference_files(case, instance, last, tmp_path):
    mirror = load_pkg("mirror")
    cs = profile_ref.case_states(case)
    ins = cs["case"]["instances"][instance]
    sp = mirror.SpatialProfile(cs["ps"].length, mode="cylinder" if ins["mode"] == profile_ref.CYLINDER else "cartesian", units=ins["units"],
                               writefrequency=2, init=1, recording=1, outputprefix=ins["prefix"],
                               profiledComponent="all" if ins["component"] < 0 else ins["component"] + 1,
                               profiles=("density", "temperature", "velocity", "velocity3d", "virial"))
    assert sp.quantities() == profile_ref.ALL and sp.component() == ins["component"]
    assert [sp.samplesAt(s) for s in (0, 1, 2)] == [False, True, True] and [sp.writesAt(s) for s in (0, 1, 2, 3, 4)] == [False, False, True, False, True]
    sp.write(profile_ref.case_tables(case, instance, last - 1, last), last, cs["states"][last - 1]["temperature"], directory=str(tmp_path))
    names = sorted(os.listdir(tmp_path))
    assert names == sorted("%s_%d%s" % (ins["prefix"], last, s) for s in profile_ref.SUFFIXES)
    for suffix in profile_ref.SUFFIXES:
        got = (tmp_path / ("%s_%d%s" % (ins["prefix"], last, suffix))).read_text()
        profile_ref.same_text(got, profile_ref.golden_text(case, ins["prefix"], last, suffix), (case, ins["prefix"], last, suffix))


def test_enable_rules_of_the_plugin():
    """SpatialProfile::readXML (SpatialProfile.cpp:55-127): none given -> all; temperature alone carries no density file"""
    mirror = load_pkg("mirror")
    L = np.array([10., 10., 10.])
    assert mirror.SpatialProfile(L, units=(1, 2, 3)).quantities() == profile_ref.ALL
    only_t = mirror.SpatialProfile(L, units=(1, 2, 3), profiles=("temperature",))
    assert only_t.quantities() == profile_ref.TEMPERATURE
    t = dict(samples=1, n=np.ones(6, dtype=np.uint64), dof=3 * np.ones(6, dtype=np.uint64), ekin=np.full(6, 6.0))
    assert sorted(only_t.render(t, 1, 1.0)) == [".Temppr"]
    assert mirror.SpatialProfile(L, units=(1, 2, 3), profiles=("density",)).quantities() == 0
    assert mirror.SpatialProfile(L, units=(1, 2, 3), profiles=("virial2D",)).quantities() == profile_ref.TEMPERATURE
    assert mirror.SpatialProfile(L, units=(1, 2, 3), profiles=("velocity", "virial")).quantities() == profile_ref.VELOCITY | profile_ref.VIRIAL
    with pytest.raises(ValueError):
        mirror.SpatialProfile(L, mode="spherical", units=(1, 2, 3))


def test_header_binding_and_library_declare_the_same_five_functions():
    capi = load_pkg("capi")
    src = open(os.path.join(ROOT, "include", "ls1hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert sorted(set(re.findall(r"\b(ls1hip_profile_[a-z_0-9]+)\s*\(", src))) == FUNCTIONS
    assert sorted(k for k in capi.SYMBOLS if k.startswith("ls1hip_profile_")) == FUNCTIONS
    syms = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = sorted(set(re.findall(r"\b(ls1hip_profile_[a-z_0-9]+)\b", syms)))
    assert exported == FUNCTIONS
    for name, val in (("CARTESIAN", 0), ("CYLINDER", 1), ("VELOCITY", 1), ("VELOCITY3D", 2), ("TEMPERATURE", 4), ("VIRIAL", 8)):
        assert int(re.search(r"#define LS1HIP_PROF_%s\s+(\d+)" % name, src).group(1)) == val == getattr(profile_ref, name)
        assert getattr(load_pkg("engine").DeviceEngine, "PROF_" + name) == val

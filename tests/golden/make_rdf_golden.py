#!/usr/bin/env python3
"""Regenerates tests/golden/rdf/ from the REAL reference: the unmodified driver oracle/_ref/MarDyn (built by
__graft_entry__.build()) runs three steps of every case with its RDF output plugin, writefrequency = samplingfrequency = 1.
With one sample per file the `Npair(curr.)` column of a .rdf file is the raw integer pair count (exact at precision(5) while
it is below 10^5).

Run where the reference binary exists:   python tests/golden/make_rdf_golden.py [case ...]

Per case it writes tests/golden/rdf/<case>.xml (the driver's config: settings only) and tests/golden/rdf/<case>.tar.gz with the files rdf_i-j.<step>.rdf,
and the list of cases MANIFEST_rdf.txt.  The driver runs NVT with its global velocity-scaling thermostat (the legacy thermostat
lines of an .inp header are not read on the XML path).

Condition, not a tolerance: a state is usable only if no molecule or site distance lies within 1e-8 of a bin edge, of r_c or of
bins * dr — last-bit differences of dd between compilers (the reference is built with -mfma) and the 1e-9 agreement of
trajectories matter only there.  The driver does not dump the positions of intermediate steps, so the condition is asserted on
the CPU oracle's trajectory of the same run, and the script then checks that the brute-force restatement (tests/rdf_ref.py) on
those positions reproduces every integer the reference wrote.  If a step violates the condition, change dr by a few percent.
"""
import gzip
import importlib
import os
import shutil
import subprocess
import sys
import tarfile
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
MARDYN = os.path.join(ROOT, "oracle", "_ref", "MarDyn")
OUT = os.path.join(HERE, "rdf")

# name, input, r_c, dt, temperature of the driver's thermostat, bins, interval length, steps
CASES = [
    ("bcc1clj_3456", "synthetic_bcc1clj_12.inp", 2.5, 0.005, 0.95, 97, 0.0257, 3),
    ("twotherm_1024", "synthetic_twotherm_8.inp", 2.5, 0.004, 0.95, 97, 0.0257, 3),
    ("mixed5_1024", "synthetic_mixed5_8.inp", 35.0, 0.2, 0.000855040543, 113, 0.3097, 3),
]

XML = """<?xml version='1.0' encoding='UTF-8'?>
<mardyn version="20100525">
  <refunits type="SI"><length unit="nm">0.1</length><mass unit="u">1</mass><energy unit="K">1</energy></refunits>
  <simulation type="MD">
    <integrator type="Leapfrog"><timestep unit="reduced">{dt}</timestep></integrator>
    <run><currenttime>0</currenttime><equilibration><steps>0</steps></equilibration><production><steps>{steps}</steps></production></run>
    <ensemble type="NVT">
      <temperature unit="reduced">{temp}</temperature>
      <domain type="box"><lx>{L[0]}</lx><ly>{L[1]}</ly><lz>{L[2]}</lz></domain>
      <components>{components}</components>
      <phasespacepoint><file type="ASCII">{inp}</file></phasespacepoint>
    </ensemble>
    <algorithm>
      <parallelisation type="DomainDecomposition"></parallelisation>
      <datastructure type="LinkedCells"><cellsInCutoffRadius>1</cellsInCutoffRadius></datastructure>
      <cutoffs type="CenterOfMass"><radiusLJ unit="reduced">{rc}</radiusLJ></cutoffs>
      <electrostatic type="ReactionField"><epsilon>{eps_rf}</epsilon></electrostatic>
    </algorithm>
    <output>
      <outputplugin name="RDF"><writefrequency>1</writefrequency><samplingfrequency>1</samplingfrequency><outputprefix>rdf</outputprefix>
        <bins>{bins}</bins><intervallength>{dr}</intervallength></outputplugin>
    </output>
  </simulation>
</mardyn>
"""


def main():
    import numpy as np

    import rdf_ref
    from golden_io import input_path

    inp_mod = importlib.import_module("ls1-mardyn_amd.inp")
    if not os.path.exists(MARDYN):
        sys.exit(f"{MARDYN} not found: run __graft_entry__.build() where the reference's sources are")
    os.makedirs(OUT, exist_ok=True)
    only = set(sys.argv[1:])
    with open(os.path.join(OUT, "MANIFEST_rdf.txt"), "w") as fh:
        fh.write("# name input cutoff dt temperature bins intervallength steps\n")
        for c in CASES:
            fh.write(" ".join([c[0], c[1]] + [repr(x) for x in c[2:]]) + "\n")
    for name, inp, rc, dt, temp, bins, dr, steps in CASES:
        if only and name not in only:
            continue
        ps = inp_mod.read_inp(input_path(inp))
        cfg = XML.format(dt=repr(dt), steps=steps, temp=repr(temp), L=[repr(float(x)) for x in ps.length], rc=repr(rc),
                         components=inp_mod.components_xml(ps.components), inp=inp, eps_rf=repr(float(ps.components.eps_rf)),
                         bins=bins, dr=repr(dr))
        with tempfile.TemporaryDirectory() as tmp:
            shutil.copy(input_path(inp), os.path.join(tmp, inp))
            with open(os.path.join(tmp, "config.xml"), "w") as fh:
                fh.write(cfg)
            run = subprocess.run([MARDYN, "config.xml", "--steps", str(steps), "--final-checkpoint=0"], cwd=tmp,
                                 env=dict(os.environ, OMP_NUM_THREADS="4"), capture_output=True, text=True, timeout=1800)
            if run.returncode != 0:
                sys.exit(run.stdout[-3000:] + run.stderr[-2000:])
            got = sorted(f for f in os.listdir(tmp) if f.endswith(".rdf"))
            nC = len(ps.components.components)
            assert len(got) == steps * nC * (nC + 1) // 2, got
            # one archive per case (the five-component files carry 25 site columns each: 2.5 MB of text); fixed order, owner and time
            with open(os.path.join(OUT, name + ".tar.gz"), "wb") as raw, gzip.GzipFile(fileobj=raw, mode="wb", compresslevel=9, mtime=0) as gz, \
                    tarfile.open(fileobj=gz, mode="w") as tf:
                for f in got:
                    ti = tf.gettarinfo(os.path.join(tmp, f), arcname=f)
                    ti.mtime, ti.uid, ti.gid, ti.uname, ti.gname, ti.mode = 0, 0, 0, "", "", 0o644
                    with open(os.path.join(tmp, f), "rb") as fh:
                        tf.addfile(ti, fh)
        with open(os.path.join(OUT, name + ".xml"), "w") as fh:
            fh.write(cfg)
        # the condition on the positions, and the restatement against what the reference wrote
        rdf_ref.case_states.cache_clear()
        rdf_ref.case_counts.cache_clear()
        rdf_ref._golden_archive.cache_clear()
        for k in range(1, steps + 1):
            cnt = rdf_ref.case_counts(name, k)
            assert cnt["margin"] >= rdf_ref.EDGE_MARGIN, f"{name} step {k}: a distance lies {cnt['margin']:.3e} from an edge — change dr"
            mol, ctr = rdf_ref.golden_mol_counts(name, nC, bins, k)
            assert np.array_equal(mol, cnt["mol"]), f"{name} step {k}: the restatement and the reference disagree"
            assert np.array_equal(ctr, cnt["n_per_component"])
            print(f"{name} step {k}: {int(mol.sum())} pairs, largest bin {int(mol.max())}, edge margin {cnt['margin']:.3e}")


if __name__ == "__main__":
    main()

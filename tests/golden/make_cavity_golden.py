#!/usr/bin/env python3
"""Regenerates tests/golden/cavity/ from the REAL reference: the unmodified driver oracle/_ref/MarDyn (built by
__graft_entry__.build()) runs ONE step of a 250-molecule case with its CavityWriter plugin over the whole domain.

Run where the reference binary exists:   python tests/golden/make_cavity_golden.py

The state the output belongs to: before its first step the driver calls every plugin's afterForces and endStep once with simstep 0
(Simulation::prepare_start and the initial pluginEndStepCall), on the positions of the input file as read.  That call writes
<case>-c<cid>-0.cav.xyz, and only these files are kept; the one step the driver then makes (it refuses to run none) writes -1 files
for positions it does not dump.
Per case it writes tests/golden/cavity/<case>.xml (the driver's config: settings only), the driver's <case>-c<cid>-0.cav.xyz files
and MANIFEST_cavity.txt.  It then asserts that the restatement (tests/cavity_ref.py) on the input positions reproduces the count and
every printed line, under the edge-margin condition of the GPU tests.
"""
import importlib
import os
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
MARDYN = os.path.join(ROOT, "oracle", "_ref", "MarDyn")
OUT = os.path.join(HERE, "cavity")

# name, input, r_c, dt, temperature of the driver's thermostat, Nx Ny Nz, radius, maxNeighbours, componentids (they only name files)
CASES = [
    ("multi_250", "VectorizationMultiComponentMultiPotentials.inp", 35.0, 0.002, 0.0003, (12, 10, 11), 35.0, 14, (0, 2)),
]

XML = """<?xml version='1.0' encoding='UTF-8'?>
<mardyn version="20100525">
  <refunits type="SI"><length unit="nm">0.1</length><mass unit="u">1</mass><energy unit="K">1</energy></refunits>
  <simulation type="MD">
    <integrator type="Leapfrog"><timestep unit="reduced">{dt}</timestep></integrator>
    <run><currenttime>0</currenttime><equilibration><steps>0</steps></equilibration><production><steps>1</steps></production></run>
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
      <outputplugin name="CavityWriter"><writefrequency>1</writefrequency><outputprefix>{name}</outputprefix><incremental>1</incremental>
        <maxNeighbours>{max_nb}</maxNeighbours><radius>{radius}</radius><Nx>{N[0]}</Nx><Ny>{N[1]}</Ny><Nz>{N[2]}</Nz>
        {componentids}</outputplugin>
    </output>
  </simulation>
</mardyn>
"""


def main():
    import numpy as np

    import cavity_ref
    from golden_io import input_path

    inp_mod = importlib.import_module("ls1-mardyn_amd.inp")
    if not os.path.exists(MARDYN):
        sys.exit(f"{MARDYN} not found: run __graft_entry__.build() where the reference's sources are")
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, "MANIFEST_cavity.txt"), "w") as fh:
        fh.write("# name input cutoff Nx Ny Nz radius maxNeighbours componentids\n")
        for name, inp, rc, _, _, N, radius, max_nb, cids in CASES:
            fh.write(" ".join([name, inp, repr(rc)] + [str(k) for k in N] + [repr(radius), str(max_nb), ",".join(str(k) for k in cids)]) + "\n")
    for name, inp, rc, dt, temp, N, radius, max_nb, cids in CASES:
        ps = inp_mod.read_inp(input_path(inp))
        cfg = XML.format(dt=repr(dt), temp=repr(temp), L=[repr(float(x)) for x in ps.length], rc=repr(rc), components=inp_mod.components_xml(ps.components),
                         inp=inp, eps_rf=repr(float(ps.components.eps_rf)), name=name, max_nb=max_nb, radius=repr(radius), N=N,
                         componentids="".join("<componentid>%d</componentid>" % k for k in cids))
        with tempfile.TemporaryDirectory() as tmp:
            shutil.copy(input_path(inp), os.path.join(tmp, inp))
            with open(os.path.join(tmp, "config.xml"), "w") as fh:
                fh.write(cfg)
            run = subprocess.run([MARDYN, "config.xml", "--steps", "1", "--final-checkpoint=0"], cwd=tmp,
                                 env=dict(os.environ, OMP_NUM_THREADS="4"), capture_output=True, text=True, timeout=1800)
            if run.returncode != 0:
                sys.exit(run.stdout[-3000:] + run.stderr[-2000:])
            files = ["%s-c%d-0.cav.xyz" % (name, k) for k in cids]
            assert all(os.path.exists(os.path.join(tmp, f)) for f in files), os.listdir(tmp)
            for f in files:
                shutil.copy(os.path.join(tmp, f), os.path.join(OUT, f))
        with open(os.path.join(OUT, name + ".xml"), "w") as fh:
            fh.write(cfg)
        counts, _, margin = cavity_ref.cavity_ref(ps.r, ps.ids, ps.length, N, radius)
        assert margin > 1e-9, margin
        for k in cids:
            want = cavity_ref.cav_xyz_lines(counts, max_nb, ps.length, k)
            got = open(os.path.join(OUT, "%s-c%d-0.cav.xyz" % (name, k))).read().split("\n")
            assert got == want, (k, got[:4], want[:4])
        print(f"{name}: {int((counts <= max_nb).sum())} cavities of {counts.size} nodes, counts {counts.min()}..{counts.max()}, edge margin {margin:.3e}")


if __name__ == "__main__":
    main()

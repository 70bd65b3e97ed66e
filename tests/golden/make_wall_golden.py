#!/usr/bin/env python3
"""Regenerates tests/golden/wall/ from the REAL reference: the unmodified driver oracle/_ref/MarDyn (built by
__graft_entry__.build()) runs 4 NVT steps of two films (the inputs of tests/golden/planar: tests/golden/inputs/film_*.inp.gz) with
the plugins WallPotential and Mirror on.

Run where the reference binary exists:   python tests/golden/make_wall_golden.py [case ...]

  wall93_reflect   the 1CLJ film, a 9-3 wall one sigma below it and an MT_REFLECT mirror o-| one sigma inside its upper face (so the
                   mirror owns molecules from the initial state on: prepare_start calls it, Simulation.cpp:880-886)
  wall104_rotors   the centre / two-site film, a 10-4-3 wall of width 0.6 below it that only the two-site component feels

Per case: tests/golden/wall/<case>.xml (settings only), <case>.tar.gz with step4.restart.dat (the final checkpoint), result.res
(per-step T / U_pot / p lines) and wall.json (the plugins' arguments as tests/wall_ref.py takes them), MANIFEST_wall.txt.
No step may trigger the explosion heuristic of the driver's thermostat (asserted on its log)."""
import gzip
import importlib
import json
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
from make_planar_golden import XML as PLANAR_XML  # noqa: E402  (the same run, without <longrange>, plus the plugins)

MARDYN = os.path.join(ROOT, "oracle", "_ref", "MarDyn")
OUT = os.path.join(HERE, "wall")
STEPS = 4


def plugins(L):
    """name -> (film input, r_c, dt, temperature, wall, mirrors) for a box of length L in y"""
    lo, hi = L / 4, 3 * L / 4  # the film
    return {
        "wall93_reflect": ("film_synthetic_bcc1clj_12.inp", 2.5, 0.005, 0.95,
                           dict(potential=93, density=1.0, sigma=1.0, epsilon=1.0, yoff=lo - 1.0, ycut=2.5, width=0.0, delta=0.0,
                                components={"1": (1.0, 1.0)}),
                           [dict(type=1, direction=1, coord=hi - 1.0, cid=0, forceConstant=0.0)]),
        "wall104_rotors": ("film_centre_site_2c.inp", 2.5, 0.002, 0.95,
                           dict(potential=104, density=1.07, sigma=1.0, epsilon=1.0, yoff=lo - 1.2, ycut=2.5, width=0.6, delta=0.775,
                                components={"2": (1.0, 1.0)}), []),
    }


def plugin_xml(wall, mirrors):
    comps = "".join(f'<component id="{k}"><xi>{xi!r}</xi><eta>{eta!r}</eta></component>' for k, (xi, eta) in wall["components"].items())
    out = ['    <plugin name="WallPotential">' + "".join(f"<{k}>{wall[k]!r}</{k}>" for k in
                                                         ("potential", "density", "sigma", "epsilon", "yoff", "ycut", "width", "delta")) + comps + "</plugin>"]
    for i, m in enumerate(mirrors):
        out.append(f'    <plugin name="Mirror" type="{m["type"]}" dir="{"o-|" if m["direction"] else "|-o"}"><pluginID>{100 + i}</pluginID><cid>{m["cid"]}</cid>'
                   f'<position><refID>0</refID><coord>{m["coord"]!r}</coord></position><forceConstant>{m["forceConstant"]!r}</forceConstant></plugin>')
    return "\n".join(out) + "\n"


def main():
    from golden_io import input_path
    inp_mod = importlib.import_module("ls1-mardyn_amd.inp")
    if not os.path.exists(MARDYN):
        sys.exit(f"{MARDYN} not found: run __graft_entry__.build() where the reference's sources are")
    os.makedirs(OUT, exist_ok=True)
    only = set(sys.argv[1:])
    L = float(inp_mod.read_inp(input_path("film_synthetic_bcc1clj_12.inp")).length[1])
    cases = plugins(L)
    with open(os.path.join(OUT, "MANIFEST_wall.txt"), "w") as fh:
        fh.write("# name input cutoff dt temperature steps\n")
        for name, (src, rc, dt, temp, _, _) in cases.items():
            fh.write(" ".join([name, src, repr(rc), repr(dt), repr(temp), str(STEPS)]) + "\n")
    for name, (src, rc, dt, temp, wall, mirrors) in cases.items():
        if only and name not in only:
            continue
        ps = inp_mod.read_inp(input_path(src))
        assert float(ps.length[1]) == L
        head, tail = PLANAR_XML.split("      <longrange")
        xml = head + tail.split("</longrange>\n", 1)[1]
        xml = xml.replace("  </simulation>", plugin_xml(wall, mirrors) + "  </simulation>")
        cfg = xml.format(dt=repr(dt), steps=STEPS, temp=repr(temp), L=[repr(float(x)) for x in ps.length], rc=repr(rc),
                         components=inp_mod.components_xml(ps.components), inp=src, eps_rf=repr(float(ps.components.eps_rf)))
        with tempfile.TemporaryDirectory() as tmp:
            inp_mod.write_inp(os.path.join(tmp, src), ps)
            with open(os.path.join(tmp, "config.xml"), "w") as fh:
                fh.write(cfg)
            with open(os.path.join(tmp, "wall.json"), "w") as fh:
                json.dump(dict(wall=wall, mirrors=mirrors), fh, indent=1)
            run = subprocess.run([MARDYN, "config.xml", "--steps", str(STEPS), "--final-checkpoint=1"], cwd=tmp,
                                 env=dict(os.environ, OMP_NUM_THREADS="4"), capture_output=True, text=True, timeout=1800)
            if run.returncode != 0:
                sys.exit(run.stdout[-3000:] + run.stderr[-2000:])
            log = run.stdout + run.stderr
            assert "Explosion" not in log, f"{name}: the driver's explosion heuristic fired"
            assert "[WallPotential]" in log and ("[Mirror]" in log or not mirrors), f"{name}: a plugin did not load"
            os.replace(os.path.join(tmp, "config.restart.dat"), os.path.join(tmp, f"step{STEPS}.restart.dat"))
            with open(os.path.join(OUT, name + ".tar.gz"), "wb") as raw, gzip.GzipFile(fileobj=raw, mode="wb", compresslevel=9, mtime=0) as gz, \
                    tarfile.open(fileobj=gz, mode="w") as tf:
                for f in (f"step{STEPS}.restart.dat", "result.res", "wall.json"):
                    ti = tf.gettarinfo(os.path.join(tmp, f), arcname=f)
                    ti.mtime, ti.uid, ti.gid, ti.uname, ti.gname, ti.mode = 0, 0, 0, "", "", 0o644
                    with open(os.path.join(tmp, f), "rb") as fh:
                        tf.addfile(ti, fh)
            print(name, open(os.path.join(tmp, "result.res")).read())
        with open(os.path.join(OUT, name + ".xml"), "w") as fh:
            fh.write(cfg)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Cost of the ODF sampling pass against the RDF molecule-only pass and the per-step brick force pass of the same build, same box.

    python tools/odf_time.py [--reps 10] [--n-per-dim 171] [--out profiles/odf_pass.txt]

Box: synth.thermal_box with a two-component Stockmayer set (one LJ centre + one dipole (0, 0, 1) each), 2 n^3 molecules (171:
N = 10 000 422) at the number density and temperature of the mixed5 fixture, r_c = 35.  The state is binned once and each pass warmed
up; then, for shellcutoff = 0.6 r_c and for r_c (10 x 10 x 10 increments), the three passes ALTERNATE `reps` times, each call timed
by the library's own HIP events (ls1hip_timing "force" / "rdf" / "odf") and read back call by call.  Reported: median, minimum,
maximum per pass, the ratios of the medians, and whether the expectation "ODF at 0.6 r_c <= RDF molecule-only" held.
"""
import argparse
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

RC = 35.0


def one_call(e, name, fn):
    e.timing_reset()
    fn()
    ms, n = e.timing(name)
    assert n == 1, (name, n)
    return ms


def line(tag, a):
    return f"  {tag:<34s} median {np.median(a):9.3f} ms   min {a.min():9.3f}   max {a.max():9.3f}   (n = {len(a)})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--n-per-dim", type=int, default=171)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    inp = importlib.import_module("ls1-mardyn_amd.inp")
    synth = importlib.import_module("ls1-mardyn_amd.synth")
    engine_mod = importlib.import_module("ls1-mardyn_amd.engine")
    stock = inp.make_component(lj=[(0, 0, 0, 0.016, 0.00042, 6.0, 0, 0)], dipoles=[(0, 0, 0, 0, 0, 1, 0.5)], I_file=(0.004, 0.004, 0.004))
    cs = inp.ComponentSet([stock, stock], np.ones((1, 2)), 1e10)
    ps = synth.thermal_box(inp, cs, args.n_per_dim, synth.MIXED5_NUMBER_DENSITY, synth.MIXED5_TEMPERATURE)
    N = len(ps.ids)
    e = engine_mod.DeviceEngine(0)
    e.set_components(cs, RC)
    e.set_domain(ps.length)
    e.upload(ps.ids, ps.cid, ps.r, ps.v, ps.q, ps.D)
    del ps
    e.rebin(); e.halo(); e.forces(0)
    e.rdf_config(100, RC / 100, False)
    e.timing_enable(1)
    out = [f"ODF sampling pass against the RDF molecule-only pass and the per-step brick force pass (tools/odf_time.py --reps {args.reps}), "
           f"{torch.cuda.get_device_name(0)}",
           f"two-component Stockmayer box, N = {N}, r_c {RC}, grid {list(e.grid()[0])}; ODF 10 x 10 x 10 increments; RDF 100 bins, no site histograms; "
           f"kernel family of the force pass: {e.get_option('last_force_kernel')}"]
    for frac in (0.6, 1.0):
        e.odf_config(10, 10, 10, frac * RC)
        e.forces(0, want_macro=False); e.rdf_sample(); e.odf_sample()  # warm-up: code objects, first touch of the histograms
        f, r, o = [], [], []
        for _ in range(args.reps):
            f.append(one_call(e, "force", lambda: e.forces(0, want_macro=False)))
            r.append(one_call(e, "rdf", e.rdf_sample))
            o.append(one_call(e, "odf", e.odf_sample))
        f, r, o = np.array(f), np.array(r), np.array(o)
        got = e.odf_read()
        assert got["samples"] == args.reps + 1
        pairs = int(got["hist"].sum()) // 2 // got["samples"]
        out += [f"shellcutoff = {frac} r_c: {pairs} pairs per sample ({pairs / N:.2f} per molecule)",
                line("force pass (ls1hip_forces)", f), line("RDF pass, molecule-only", r), line("ODF pass (ls1hip_odf_sample)", o),
                f"  ratio ODF / RDF (medians)    {np.median(o) / np.median(r):.3f}",
                f"  ratio ODF / force (medians)  {np.median(o) / np.median(f):.3f}"]
        if frac == 0.6:
            held = np.median(o) <= np.median(r)
            out.append(f"  expectation 'ODF at 0.6 r_c does not exceed the RDF molecule-only pass': {'held' if held else 'did NOT hold'}")
    e.close()
    text = "\n".join(out) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()

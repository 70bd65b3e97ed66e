#!/usr/bin/env python3
"""Cost of the angular-RDF pass (k_ardf_brick with the molecule histogram in the same walk) against the RDF molecule-only pass and
the per-step brick force pass of the same build, same box, same process.

    python tools/ardf_time.py [--workload lj|stock|both] [--reps 10] [--n-per-dim 171] [--out profiles/ardf_pass.txt]

lj:     configs[1] of bench.py, N = 10 000 422 single-centre LJ molecules (r_c 2.5, no rotation), 100 x 10 bins;
stock:  the two-component Stockmayer box of tools/odf_time.py (r_c 35), 100 x 10 bins (4 300 words: in LDS) and 100 x 40 bins
        (16 300 words: beyond the LDS budget, ARDF counts by global atomics).
The state is binned once and each pass warmed up; then the three passes ALTERNATE `reps` times, each call timed by the library's own
HIP events (ls1hip_timing "force" / "rdf"; the angular part is switched off and on between the two RDF calls, outside the timed
region).  Reported: median, minimum, maximum per pass, the ratios of the medians, whether the expectation held, and a check that the
molecule histogram of the angular pass equals the RDF pass's.

Expectation, stated before the numbers: the yardstick is the RDF molecule-only pass of the same run.  The ARDF pass does the same walk
plus, per hit (~27 per molecule at liquid density), the division chain and two more LDS atomics, with every lane of the drain busy
and no workgroup barrier in the walk: it should land between the RDF pass and the force pass, without the ODF pass' barrier penalty.
"""
import argparse
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def one_call(e, name, fn):
    e.timing_reset()
    fn()
    ms, n = e.timing(name)
    assert n == 1, (name, n)
    return ms


def line(tag, a):
    return f"  {tag:<34s} median {np.median(a):9.3f} ms   min {a.min():9.3f}   max {a.max():9.3f}   (n = {len(a)})"


def window(e, reps, bins, dr, A, N):
    e.rdf_config(bins, dr, False)
    e.forces(0, want_macro=False); e.rdf_sample()
    e.rdf_config_angular(A); e.rdf_sample()  # warm-up: code objects, first touch of the histograms
    f, r, a = [], [], []
    for _ in range(reps):
        f.append(one_call(e, "force", lambda: e.forces(0, want_macro=False)))
        e.rdf_config_angular(1)
        r.append(one_call(e, "rdf", e.rdf_sample))
        e.rdf_config_angular(A)
        a.append(one_call(e, "rdf", e.rdf_sample))
    f, r, a = np.array(f), np.array(r), np.array(a)
    e.rdf_reset(); e.rdf_sample()
    got = e.rdf_read()
    e.rdf_config_angular(1); e.rdf_reset(); e.rdf_sample()
    same = np.array_equal(e.rdf_read()["mol"], got["mol"])
    pairs, counts = int(got["mol"].sum()), int(got["ardf"].sum())
    held = np.median(r) <= np.median(a) <= np.median(f)
    return [f"{bins} x {A} bins ({got['ardf'].size + got['mol'].size} words): {pairs} pairs per sample ({pairs / N:.2f} per molecule), "
            f"{counts} ARDF counts ({2 * pairs - counts} dropped by the flat index); molecule histogram equals the RDF pass's: {same}",
            line("force pass (ls1hip_forces)", f), line("RDF pass, molecule-only", r), line("ARDF pass (RDF + angular, one walk)", a),
            f"  ratio ARDF / RDF (medians)    {np.median(a) / np.median(r):.3f}",
            f"  ratio ARDF / force (medians)  {np.median(a) / np.median(f):.3f}",
            f"  expectation 'between the RDF molecule-only pass and the force pass': {'held' if held else 'did NOT hold'}"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", choices=("lj", "stock", "both"), default="both")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--n-per-dim", type=int, default=171)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    import bench
    inp = importlib.import_module("ls1-mardyn_amd.inp")
    synth = importlib.import_module("ls1-mardyn_amd.synth")
    engine_mod = importlib.import_module("ls1-mardyn_amd.engine")
    n = args.n_per_dim
    out = [f"ARDF pass against the RDF molecule-only pass and the per-step brick force pass (tools/ardf_time.py --reps {args.reps}), "
           f"{torch.cuda.get_device_name(0)}"]
    if args.workload in ("lj", "both"):
        L = synth.box_length(n, bench.RHO)
        e = engine_mod.DeviceEngine(0)
        e.set_components(bench.lj_components(inp), bench.RC)
        e.set_domain([L, L, L])
        dev = torch.device("cuda", 0)
        e.upload_begin(2 * n ** 3)
        for ids_t, r_t, v_t in synth.bcc_chunks_device(torch, dev, n, rho=bench.RHO, temp=bench.TEMP):
            torch.cuda.synchronize()
            e.upload_chunk_device(ids_t.numel(), ids_t.data_ptr(), 0, r_t.data_ptr(), v_t.data_ptr())
        del ids_t, r_t, v_t
        e.upload_end()
        e.rebin(); e.halo(); e.forces(0)
        e.run(bench.DT, 100)  # away from the lattice start
        e.rebin(); e.halo()
        e.timing_enable(1)
        out.append(f"lj: N = {2 * n ** 3}, r_c {bench.RC}, no rotation (orientation (0, 0, 1)), after 100 steps, grid {[int(x) for x in e.grid()[0]]}")
        out += window(e, args.reps, 100, 0.025, 10, 2 * n ** 3)
        e.close()
    if args.workload in ("stock", "both"):
        stock = inp.make_component(lj=[(0, 0, 0, 0.016, 0.00042, 6.0, 0, 0)], dipoles=[(0, 0, 0, 0, 0, 1, 0.5)], I_file=(0.004, 0.004, 0.004))
        cs = inp.ComponentSet([stock, stock], np.ones((1, 2)), 1e10)
        ps = synth.thermal_box(inp, cs, n, synth.MIXED5_NUMBER_DENSITY, synth.MIXED5_TEMPERATURE)
        N = len(ps.ids)
        e = engine_mod.DeviceEngine(0)
        e.set_components(cs, 35.0)
        e.set_domain(ps.length)
        e.upload(ps.ids, ps.cid, ps.r, ps.v, ps.q, ps.D)
        del ps
        e.rebin(); e.halo(); e.forces(0)
        e.timing_enable(1)
        out.append(f"stock: two-component Stockmayer box, N = {N}, r_c 35.0, grid {[int(x) for x in e.grid()[0]]}")
        for A in (10, 40):
            out += window(e, args.reps, 100, 0.35, A, N)
        e.close()
    text = "\n".join(out) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Cost of the RDF sampling pass against the per-step brick force pass of the same build, same box, same GPU.

    python tools/rdf_time.py [--workload lj|ethane|both] [--reps 10] [--out profiles/rdf_pass.txt]

lj:      configs[1] of bench.py, N = 10 000 422 single-centre LJ molecules (r_c 2.5), 100 bins of 0.025;
ethane:  bench.py --workload ethane's box (the reference's equilibrated 2CLJ ethane replicated 10 x 10 x 10, r_c 32.1254),
         113 bins of 0.2843, site histograms on.
Both passes walk the same pairs (the force pass does the force arithmetic on top).  The state is re-binned once, warmed up with
one call of each pass, then the two passes ALTERNATE `reps` times; each call is timed by the library's own HIP events
(ls1hip_timing "force" / "rdf"), read back call by call.  Reported: median, minimum, maximum per pass and the ratio of the medians.
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


def measure(e, reps, melt_dt, melt_steps):
    e.rebin(); e.halo(); e.forces(0)
    if melt_steps:
        e.run(melt_dt, melt_steps)  # away from the lattice start
    e.rebin(); e.halo()
    e.timing_enable(1)
    e.forces(0, want_macro=False); e.rdf_sample()  # warm-up: code objects, first touch of the histograms
    f, r = [], []
    for _ in range(reps):
        f.append(one_call(e, "force", lambda: e.forces(0, want_macro=False)))
        r.append(one_call(e, "rdf", e.rdf_sample))
    got = e.rdf_read()
    assert got["samples"] == reps + 1
    return np.array(f), np.array(r), got


def line(tag, a):
    return f"  {tag:<28s} median {np.median(a):9.3f} ms   min {a.min():9.3f}   max {a.max():9.3f}   (n = {len(a)})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", choices=("lj", "ethane", "both"), default="both")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--n-per-dim", type=int, default=171, help="lj: 2 n^3 molecules (171: configs[1])")
    ap.add_argument("--ethane-k", type=int, default=10, help="ethane: replication factor of the fixture per dimension")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    import bench
    inp = importlib.import_module("ls1-mardyn_amd.inp")
    synth = importlib.import_module("ls1-mardyn_amd.synth")
    engine_mod = importlib.import_module("ls1-mardyn_amd.engine")
    out = [f"RDF sampling pass against the per-step brick force pass (tools/rdf_time.py --reps {args.reps}), {torch.cuda.get_device_name(0)}"]
    if args.workload in ("lj", "both"):
        n = args.n_per_dim
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
        e.rdf_config(100, 0.025, True)
        f, r, got = measure(e, args.reps, bench.DT, 100)
        pairs = int(got["mol"].sum()) // got["samples"]
        out += [f"lj: N = {2 * n ** 3}, r_c {bench.RC}, 100 bins of 0.025, after 100 steps; {pairs} pairs per sample "
                f"(kernel family of the force pass: {e.get_option('last_force_kernel')})",
                line("force pass (ls1hip_forces)", f), line("RDF pass (ls1hip_rdf_sample)", r),
                f"  ratio RDF / force (medians)  {np.median(r) / np.median(f):.3f}"]
        e.close()
    if args.workload in ("ethane", "both"):
        ps0, _ = bench.ethane_fixture(inp)
        big = bench.replicate_phase_space(inp, ps0, args.ethane_k)
        e = engine_mod.DeviceEngine(0)
        e.set_components(big.components, bench.ETHANE_RC)
        e.set_domain(big.length)
        e.upload(big.ids, big.cid, big.r, big.v, big.q, big.D)
        N = len(big.ids)
        del big
        e.rdf_config(113, 0.2843, True)
        f, r, got = measure(e, args.reps, bench.ETHANE_DT, 0)
        pairs = int(got["mol"].sum()) // got["samples"]
        sites = int(sum(int(b.sum()) for b in got["site"])) // got["samples"]
        out += [f"ethane: N = {N}, r_c {bench.ETHANE_RC}, 113 bins of 0.2843, site histograms on; {pairs} pairs, {sites} site counts per sample "
                f"(kernel family of the force pass: {e.get_option('last_force_kernel')})",
                line("force pass (ls1hip_forces)", f), line("RDF pass (ls1hip_rdf_sample)", r),
                f"  ratio RDF / force (medians)  {np.median(r) / np.median(f):.3f}"]
        e.close()
    text = "\n".join(out) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()

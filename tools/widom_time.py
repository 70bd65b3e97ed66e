#!/usr/bin/env python3
"""Cost of a Widom sample (test-particle insertion pass) against the per-step force pass of the same build, same box, same GPU.

    python tools/widom_time.py [--workload lj|ethane|both] [--reps 10] [--out profiles/widom_pass.txt]

lj:      configs[1] of bench.py, N = 10 000 422 single-centre LJ molecules (r_c 2.5), after 100 steps;
ethane:  bench.py --workload ethane's box (the reference's equilibrated 2CLJ ethane replicated 10 x 10 x 10, r_c 32.1254).
instances = N / 1000, N / 100, N / 10 tests per sample, uniform in the box.  The expectation on record: a test costs about what one
owned molecule costs the GENERIC per-step kernel (one lane per molecule, the same neighbourhood walk), so a sample should take near
instances / N of that kernel's time.  The state is re-binned once, each pass warmed up once, then the passes ALTERNATE `reps` times;
each call is timed by the library's own HIP events (ls1hip_timing "force" / "insert": the insertion kernel alone, without the
generator and the accumulation).  Reported: median, minimum, maximum per pass, the ratio of the medians and the ratio expected.
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
    return f"  {tag:<44s} median {np.median(a):9.3f} ms   min {a.min():9.3f}   max {a.max():9.3f}   (n = {len(a)})"


def measure(e, capi, N, T, reps, melt_dt, melt_steps):
    e.rebin(); e.halo(); e.forces(0)
    if melt_steps:
        e.run(melt_dt, melt_steps)  # away from the lattice start
    out = []
    e.timing_enable(1)
    force = {}
    for tag, kernel in (("default", capi.FK_AUTO), ("generic", capi.FK_GENERIC)):
        e.set_option("force_kernel", kernel)
        e.rebin(); e.halo()
        e.forces(0, want_macro=False)
        force[tag] = np.array([one_call(e, "force", lambda: e.forces(0, want_macro=False)) for _ in range(reps)])
        out.append(line(f"force pass, {tag} kernel (family {e.get_option('last_force_kernel')})", force[tag]))
    g = np.median(force["generic"])
    for div in (1000, 100, 10):
        inst = N // div
        e.widom_config(0, inst, T, seed=1, slabs=1)
        e.widom_sample()
        w = np.array([one_call(e, "insert", e.widom_sample) for _ in range(reps)])
        t = e.widom_read()
        assert t["samples"] == reps + 1 and int(t["n"][0]) == (reps + 1) * inst
        out.append(line(f"insertion pass, {inst} tests (N / {div})", w))
        out.append(f"    / generic force pass {np.median(w) / g:.5f}   expected instances / N = {inst / N:.5f}   measured / expected "
                   f"{np.median(w) / g / (inst / N):.2f}   <w> = {t['sum_w'][0] / float(t['n'][0]):.4e}")
    e.widom_config(0, 0, T)
    return out


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
    capi = importlib.import_module("ls1-mardyn_amd.capi")
    out = [f"Widom insertion pass against the per-step force pass (tools/widom_time.py --reps {args.reps}), {torch.cuda.get_device_name(0)}, FP64"]
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
        out.append(f"lj: N = {2 * n ** 3}, r_c {bench.RC}, T = {bench.TEMP}, after 100 steps")
        out += measure(e, capi, 2 * n ** 3, bench.TEMP, args.reps, bench.DT, 100)
        e.close()
    if args.workload in ("ethane", "both"):
        ps0, _ = bench.ethane_fixture(inp)
        big = bench.replicate_phase_space(inp, ps0, args.ethane_k)
        e = engine_mod.DeviceEngine(0)
        e.set_components(big.components, bench.ETHANE_RC)
        e.set_domain(big.length)
        e.upload(big.ids, big.cid, big.r, big.v, big.q, big.D)
        N, T = len(big.ids), float(ps0.temperature)
        del big
        out.append(f"ethane: N = {N}, r_c {bench.ETHANE_RC}, T = {T}")
        out += measure(e, capi, N, T, args.reps, bench.ETHANE_DT, 0)
        e.close()
    text = "\n".join(out) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()

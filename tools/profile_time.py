#!/usr/bin/env python3
"""Cost of the profile sampling pass against a kick + drift pass of the same build, same box, same GPU, and the price of the
unfused sampling steps inside ls1hip_run.

    python tools/profile_time.py [--reps 10] [--n-per-dim 171] [--out profiles/profile_pass.txt]

Workload: configs[1] of bench.py, N = 10 000 422 single-centre LJ molecules (r_c 2.5), melted for 100 steps.
Grids 1 x 200 x 1 (the table lives in LDS) and 1 x 256 x 256 (global path), each with density only and with density + velocity3d +
temperature.  The sampling pass reads at most 52 B per molecule and stores nothing per molecule; the kick + drift pass streams
120 B per molecule (it is called with dt = 0: the same loads and stores, the state stays where it is).  The two passes ALTERNATE
`reps` times; each call is timed by the library's own HIP events (ls1hip_timing "profile" / "integrate"), read back call by call.
Then ms / step of ls1hip_run in its production list configuration (skin 0.2) with profile_every = 10 against 0.
"""
import argparse
import importlib
import os
import sys
import time

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
    return f"  {tag:<44s} median {np.median(a):8.3f} ms   min {a.min():8.3f}   max {a.max():8.3f}   (n = {len(a)})"


def lj_engine(torch, bench, inp, synth, engine_mod, n, skin=None):
    L = synth.box_length(n, bench.RHO)
    e = engine_mod.DeviceEngine(0)
    e.set_components(bench.lj_components(inp), bench.RC)
    if skin:
        e.set_verlet(skin)
    e.set_domain([L, L, L])
    dev = torch.device("cuda", 0)
    e.upload_begin(2 * n ** 3)
    for ids_t, r_t, v_t in synth.bcc_chunks_device(torch, dev, n, rho=bench.RHO, temp=bench.TEMP):
        torch.cuda.synchronize()
        e.upload_chunk_device(ids_t.numel(), ids_t.data_ptr(), 0, r_t.data_ptr(), v_t.data_ptr())
    del ids_t, r_t, v_t
    e.upload_end()
    e.rebin(); e.halo(); e.forces(0)
    return e


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--n-per-dim", type=int, default=171, help="2 n^3 molecules (171: configs[1])")
    ap.add_argument("--run-steps", type=int, default=100)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    import bench
    inp = importlib.import_module("ls1-mardyn_amd.inp")
    synth = importlib.import_module("ls1-mardyn_amd.synth")
    engine_mod = importlib.import_module("ls1-mardyn_amd.engine")
    E = engine_mod.DeviceEngine
    n = args.n_per_dim
    N = 2 * n ** 3
    out = [f"profile sampling pass against the kick + drift pass (tools/profile_time.py --reps {args.reps}), {torch.cuda.get_device_name(0)}",
           f"N = {N} single-centre LJ, r_c {bench.RC}, after 100 steps; LDS table budget {6144} words per workgroup"]
    e = lj_engine(torch, bench, inp, synth, engine_mod, n)
    e.run(bench.DT, 100)  # away from the lattice start; leaves full-step velocities and valid forces
    e.timing_enable(1)
    for units in ((1, 200, 1), (1, 256, 256)):
        for tag, q in (("density", 0), ("density + velocity3d + temperature", E.PROF_VELOCITY3D | E.PROF_TEMPERATURE)):
            e.profile_config(E.PROF_CARTESIAN, units, q)
            e.profile_sample(); e.kick_drift(0.0)  # warm-up: code objects, first touch of the table
            p, k = [], []
            for _ in range(args.reps):
                p.append(one_call(e, "profile", e.profile_sample))
                k.append(one_call(e, "integrate", lambda: e.kick_drift(0.0)))
            got = e.profile_read()
            assert got["samples"] == args.reps + 1 and int(got["n"].sum()) == N * (args.reps + 1)
            p, k = np.array(p), np.array(k)
            out += [f"grid {units[0]} x {units[1]} x {units[2]}, {tag}:",
                    line("profile pass (ls1hip_profile_sample)", p), line("kick + drift pass (ls1hip_kick_drift, dt = 0)", k),
                    f"  ratio profile / kick + drift (medians)      {np.median(p) / np.median(k):.3f}"]
    e.close()
    del e
    torch.cuda.empty_cache()
    # the price of the unfused sampling steps in the production loop
    res = {}
    for every in (0, 10):
        e = lj_engine(torch, bench, inp, synth, engine_mod, n, skin=0.2)
        e.profile_config(E.PROF_CARTESIAN, (1, 200, 1), E.PROF_VELOCITY3D | E.PROF_TEMPERATURE)
        e.run(bench.DT, 20)  # warm-up, first list build
        e.set_option("profile_every", every)
        t0 = time.perf_counter()
        e.run(bench.DT, args.run_steps)
        res[every] = (time.perf_counter() - t0) * 1e3 / args.run_steps
        assert e.profile_read()["samples"] == (args.run_steps // every if every else 0)
        e.close()
        del e
        torch.cuda.empty_cache()
    out += [f"ls1hip_run, list loop (skin 0.2), {args.run_steps} steps, grid 1 x 200 x 1 with velocity3d + temperature:",
            f"  profile_every = 0    {res[0]:8.3f} ms / step",
            f"  profile_every = 10   {res[10]:8.3f} ms / step   (+{res[10] - res[0]:.3f} ms / step, {10 * (res[10] - res[0]):.3f} ms per sampling step)"]
    text = "\n".join(out) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()

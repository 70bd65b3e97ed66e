#!/usr/bin/env python3
"""Cost of the wall + mirror pass against a kick + drift pass of the same build, same process, and of the list loop with a wall on.

    python tools/wall_time.py [--reps 10] [--n-per-dim 171] [--out profiles/wall_pass.txt]

Workloads: the FILMS of tools/planar_time.py (L/4 <= y < 3L/4 of configs[1] of bench.py; of its ethane box).  A 10-4-3 wall sits at the
lower face of the film with a ycut that reaches about 5 % and about 50 % of the molecules; the pass (ls1hip_timing "wall") alternates
with ls1hip_kick_drift at dt = 0 ("integrate").  Expectation from byte counts, stated before the first measurement: a molecule out of
reach costs 8 B (y), one in reach adds cid and a 16 B read-modify-write of F_y (a rotor the quaternion and 32 B more), kick + drift
moves about 120 B per molecule — so about 0.1 x kick + drift at 5 % reach.  Then: 100 steps of the list loop (skin 0.2) on the LJ film
with and without the wall (without: the loop of the commit before, bit for bit)."""
import argparse
import importlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)
from planar_time import ethane_engine, film_engine  # noqa: E402
from profile_time import line, one_call  # noqa: E402

WALL = dict(density=1.07, sigma=1.0, epsilon=1.0, width=0.0, delta=0.775)


def wall_on(e, L, fraction, sigma=1.0):
    """a wall one sigma below the film (which fills L/4 .. 3L/4 evenly) whose ycut reaches `fraction` of it"""
    n = len(e.n_sites)
    e.wall_config(104, WALL["density"], sigma, WALL["epsilon"], L / 4 - sigma, sigma + fraction * L / 2, WALL["width"], WALL["delta"] * sigma,
                  np.ones(n, dtype=np.int32), np.ones(n), np.ones(n))


def measure(e, L, reps, sigma, out):
    e.timing_enable(1)
    for fraction in (0.05, 0.5):
        wall_on(e, L, fraction, sigma)
        e.wall_apply(); e.kick_drift(0.0); e.rebin(); e.halo(); e.forces(0)  # warm-up
        t = {"wall": [], "integrate": []}
        for _ in range(reps):
            t["wall"].append(one_call(e, "wall", e.wall_apply))
            t["integrate"].append(one_call(e, "integrate", lambda: e.kick_drift(0.0)))
            e.rebin(); e.halo(); e.forces(0)  # (a drift invalidates the forces the pass adds to)
        t = {k: np.array(v) for k, v in t.items()}
        out += [f"ycut reaches {100 * fraction:.0f} % of the film:", line("wall pass (ls1hip_wall_apply)", t["wall"]),
                line("kick + drift pass (ls1hip_kick_drift, dt = 0)", t["integrate"]),
                f"  wall pass / kick + drift                           {np.median(t['wall']) / np.median(t['integrate']):.3f}"]
    e.close()


def loop(torch, bench, inp, synth, engine_mod, n, steps, out):
    ms = {}
    for wall in (False, True):
        e, N, L = film_engine(torch, bench, inp, synth, engine_mod, n, skin=0.2)
        if wall:
            wall_on(e, L, 0.05)
        e.run(bench.DT, 10)  # warm-up, first list build
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e.run(bench.DT, steps)
        torch.cuda.synchronize()
        ms[wall] = (time.perf_counter() - t0) * 1e3 / steps
        e.close()
        torch.cuda.empty_cache()
    out += [f"list loop (skin 0.2), N = {N}, {steps} steps: {ms[False]:.3f} ms / step without a wall (fused passes), {ms[True]:.3f} ms / step with the",
            f"  wall at 5 % reach (unfused route + the pass): x {ms[True] / ms[False]:.3f}"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--n-per-dim", type=int, default=171, help="2 n^3 molecules before carving (171: configs[1])")
    ap.add_argument("--ethane-k", type=int, default=10, help="replication of the reference's ethane box per dimension (10: bench.py's)")
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    import bench
    inp = importlib.import_module("ls1-mardyn_amd.inp")
    synth = importlib.import_module("ls1-mardyn_amd.synth")
    engine_mod = importlib.import_module("ls1-mardyn_amd.engine")
    e, N, L = film_engine(torch, bench, inp, synth, engine_mod, args.n_per_dim)
    out = [f"wall + mirror pass against the kick + drift pass (tools/wall_time.py --reps {args.reps}), {torch.cuda.get_device_name(0)}",
           f"film of N = {N} single-centre LJ molecules in a box of {L:.3f}^3, 10-4-3 wall one sigma below it"]
    measure(e, L, args.reps, 1.0, out)
    torch.cuda.empty_cache()
    e, N, length, comps = ethane_engine(bench, inp, engine_mod, args.ethane_k)
    sig = float(comps.components[0].lj[0][5])
    out += [f"film of N = {N} 2CLJ ethane molecules (rigid rotors, two LJ sites) in a box of {length[0]:.3f}^3, wall sigma {sig:g}"]
    measure(e, float(length[1]), args.reps, sig, out)
    torch.cuda.empty_cache()
    loop(torch, bench, inp, synth, engine_mod, args.n_per_dim, args.steps, out)
    text = "\n".join(out) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()

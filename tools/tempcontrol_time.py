#!/usr/bin/env python3
"""Cost of the passes of the region-wise temperature control against a kick + drift pass of the same build, same process.

    python tools/tempcontrol_time.py [--reps 10] [--n-per-dim 171] [--out profiles/tempcontrol_pass.txt]

Workloads: the FILMS of tools/planar_time.py (the molecules with L/4 <= y < 3L/4 of configs[1] of bench.py and of its ethane box),
one region over the whole box, directions xz, exponent 0.4, 20 and 2000 slabs.  Measure sweep, beta kernel and standalone apply are
timed call by call by the library's own HIP events (ls1hip_timing "tempcontrol_measure" / "tempcontrol_betas" / "tempcontrol_apply"),
alternating with ls1hip_kick_drift and with the folded apply + kick + drift, both at dt = 0 ("integrate": the same loads and stores,
the positions stay).  Then a list-loop ls1hip_run window over the full configs[1] box with temperature control at frequency 1 against
the same window with the global device thermostat.  Expectation from byte counts: the sweep reads 52 B per single-centre molecule (r, v, cid) against the 120 B of
kick + drift, so about half of it; the folded pass costs what kick + drift costs.
"""
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
from profile_time import line, lj_engine, one_call  # noqa: E402


def measure(e, N, length, temp, reps, out):
    e.timing_enable(1)
    for slabs in (20, 2000):
        e.tempcontrol_config(0, 0, 0)
        e.tempcontrol_config(0, 1, 2 ** 62)
        e.tempcontrol_region([0.0, 0.0, 0.0], list(length), temp, 0, slabs, 0.4, "xz")
        e.tempcontrol_measure(); e.tempcontrol_betas(); e.tempcontrol_apply(); e.kick_drift(0.0); e.tempcontrol_apply_kick_drift(0.0)  # warm-up
        t = {k: [] for k in ("measure", "betas", "apply", "kick_drift", "folded")}
        for _ in range(reps):
            t["measure"].append(one_call(e, "tempcontrol_measure", e.tempcontrol_measure))
            t["betas"].append(one_call(e, "tempcontrol_betas", e.tempcontrol_betas))
            t["apply"].append(one_call(e, "tempcontrol_apply", e.tempcontrol_apply))
            t["kick_drift"].append(one_call(e, "integrate", lambda: e.kick_drift(0.0)))
            t["folded"].append(one_call(e, "integrate", lambda: e.tempcontrol_apply_kick_drift(0.0)))
        assert 0.99 * N <= int(e.tempcontrol_read(1)["n"].sum()) <= N  # (a molecule exactly on a face of the region takes no part)
        t = {k: np.array(v) for k, v in t.items()}
        kd = np.median(t["kick_drift"])
        out += [f"slabs = {slabs}:", line("measure sweep (ls1hip_tempcontrol_measure)", t["measure"]), line("beta kernel (ls1hip_tempcontrol_betas)", t["betas"]),
                line("standalone apply (ls1hip_tempcontrol_apply)", t["apply"]), line("kick + drift pass (ls1hip_kick_drift, dt = 0)", t["kick_drift"]),
                line("folded apply + kick + drift (ls1hip_tempcontrol_apply_kick_drift, dt = 0)", t["folded"]),
                f"  measure sweep / kick + drift                        {np.median(t['measure']) / kd:.3f}   (expected about 0.5 for single-centre molecules)",
                f"  folded pass / kick + drift                          {np.median(t['folded']) / kd:.3f}   (expected 1)",
                f"  per step at frequency 1 (measure + betas + fold - kick + drift)  {np.median(t['measure']) + np.median(t['betas']) + np.median(t['folded']) - kd:.3f} ms"]
    e.close()


def run_window(torch, bench, inp, synth, engine_mod, n, steps, out):
    """the list loop of ls1hip_run over the full configs[1] box: temperature control at frequency 1 (one region, 20 slabs, xz) against
    the global device thermostat, the same window after the same warm-up, one engine each"""
    L = synth.box_length(n, bench.RHO)
    res = {}
    for mode in ("global", "tempcontrol", "global again"):
        e = lj_engine(torch, bench, inp, synth, engine_mod, n, skin=0.2)
        if mode == "tempcontrol":
            e.tempcontrol_config(0, 1, 2 ** 62)
            e.tempcontrol_region([0.0, 0.0, 0.0], [L, L, L], bench.TEMP, 0, 20, 0.4, "xz")
        else:
            e.set_thermostat(True, bench.TEMP)
        e.run(bench.DT, 20)  # warm-up, first list build
        t0 = time.perf_counter()
        e.run(bench.DT, steps)
        res[mode] = (time.perf_counter() - t0) * 1e3 / steps
        e.close()
        del e
        torch.cuda.empty_cache()
    d = res["tempcontrol"] - min(res["global"], res["global again"])
    out += [f"ls1hip_run, list loop (skin 0.2), N = {2 * n ** 3} single-centre LJ, {steps} steps:",
            f"  global device thermostat              {res['global']:8.3f} ms / step   (again: {res['global again']:.3f})",
            f"  temperature control, frequency 1      {res['tempcontrol']:8.3f} ms / step   ({d:+.3f} ms / step, {100 * d / res['global']:+.1f} %)"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--n-per-dim", type=int, default=171, help="2 n^3 molecules before carving (171: configs[1])")
    ap.add_argument("--ethane-k", type=int, default=10, help="replication of the reference's ethane box per dimension (10: bench.py's)")
    ap.add_argument("--run-steps", type=int, default=100)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    import bench
    inp = importlib.import_module("ls1-mardyn_amd.inp")
    synth = importlib.import_module("ls1-mardyn_amd.synth")
    engine_mod = importlib.import_module("ls1-mardyn_amd.engine")
    e, N, L = film_engine(torch, bench, inp, synth, engine_mod, args.n_per_dim)
    out = [f"region-wise temperature control against the kick + drift pass (tools/tempcontrol_time.py --reps {args.reps}), {torch.cuda.get_device_name(0)}",
           f"film of N = {N} single-centre LJ molecules in a box of {L:.3f}^3"]
    measure(e, N, [L, L, L], bench.TEMP, args.reps, out)
    torch.cuda.empty_cache()
    e, N, length, _ = ethane_engine(bench, inp, engine_mod, args.ethane_k)
    out += [f"film of N = {N} 2CLJ ethane molecules (rigid rotors) in a box of {length[0]:.3f}^3"]
    measure(e, N, length, bench.TEMP, args.reps, out)
    torch.cuda.empty_cache()
    run_window(torch, bench, inp, synth, engine_mod, args.n_per_dim, args.run_steps, out)
    text = "\n".join(out) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()

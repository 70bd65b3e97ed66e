#!/usr/bin/env python3
"""Cost of the three passes of the planar long-range correction against a kick + drift pass of the same build, same process.

    python tools/planar_time.py [--reps 10] [--n-per-dim 171] [--out profiles/planar_pass.txt]

Workloads: FILMS (the molecules with L/4 <= y < 3L/4) carved from configs[1] of bench.py (10 000 422 single-centre LJ molecules,
r_c 2.5) and from its ethane box (the reference's equilibrated 2CLJ box replicated 10^3: rotation, two sites, torques), slabs = 200
and 2000.  Density, table build and apply pass are timed call by call by the library's own HIP
events (ls1hip_timing "planar_density" / "planar_tables" / "planar_apply"), alternating with ls1hip_kick_drift at dt = 0
("integrate": the same loads and stores, the state stays).  Context: the host time of tests/planar_ref.py for the same tables.
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
from profile_time import line, one_call  # noqa: E402


def film_engine(torch, bench, inp, synth, engine_mod, n, skin=None):
    L = synth.box_length(n, bench.RHO)
    dev = torch.device("cuda", 0)
    keep = lambda r: (r.view(-1, 3)[:, 1] >= L / 4) & (r.view(-1, 3)[:, 1] < 3 * L / 4)  # noqa: E731
    total = sum(int(keep(r_t).sum()) for _, r_t, _ in synth.bcc_chunks_device(torch, dev, n, rho=bench.RHO, temp=bench.TEMP))
    e = engine_mod.DeviceEngine(0)
    e.set_components(bench.lj_components(inp), bench.RC)
    if skin:
        e.set_verlet(skin)
    e.set_domain([L, L, L])
    e.upload_begin(total)
    for ids_t, r_t, v_t in synth.bcc_chunks_device(torch, dev, n, rho=bench.RHO, temp=bench.TEMP):
        m = keep(r_t)
        ids_c, r_c, v_c = ids_t[m].contiguous(), r_t.view(-1, 3)[m].contiguous(), v_t.view(-1, 3)[m].contiguous()
        torch.cuda.synchronize()
        e.upload_chunk_device(ids_c.numel(), ids_c.data_ptr(), 0, r_c.data_ptr(), v_c.data_ptr())
    e.upload_end()
    e.rebin(); e.halo(); e.forces(0)
    return e, total, L


def ethane_engine(bench, inp, engine_mod, k):
    ps0, _ = bench.ethane_fixture(inp)
    ps = bench.replicate_phase_space(inp, ps0, k)
    L = float(ps.length[1])
    m = (ps.r[:, 1] >= L / 4) & (ps.r[:, 1] < 3 * L / 4)
    e = engine_mod.DeviceEngine(0)
    e.set_components(ps.components, bench.ETHANE_RC)
    e.set_domain(ps.length)
    e.upload(ps.ids[m], ps.cid[m].astype(np.int32), ps.r[m], ps.v[m], ps.q[m], ps.D[m])
    e.rebin(); e.halo(); e.forces(0)
    return e, int(m.sum()), ps.length, ps.components


def measure(e, N, length, comps, rc, reps, planar_ref, out):
    e.timing_enable(1)
    for slabs in (200, 2000):
        e.planar_config(slabs, 1)
        e.planar_density(); e.planar_tables(); e.planar_apply(); e.kick_drift(0.0); e.rebin(); e.halo(); e.forces(0)  # warm-up
        t = {k: [] for k in ("planar_density", "planar_tables", "planar_apply", "integrate")}
        for _ in range(reps):
            t["planar_density"].append(one_call(e, "planar_density", e.planar_density))
            t["planar_tables"].append(one_call(e, "planar_tables", e.planar_tables))
            t["planar_apply"].append(one_call(e, "planar_apply", e.planar_apply))
            t["integrate"].append(one_call(e, "integrate", lambda: e.kick_drift(0.0)))
            e.rebin(); e.halo(); e.forces(0)  # (a drift invalidates the forces the apply pass adds to)
        cnt = e.planar_counts()
        rows = cnt.shape[0]
        assert int(cnt.sum()) == N * rows * (reps + 1)
        t = {k: np.array(v) for k, v in t.items()}
        kd = np.median(t["integrate"])
        per_step = np.median(t["planar_density"]) / 10 + np.median(t["planar_apply"])
        pl = planar_ref.Planar(comps, length, rc, slabs)
        t0 = time.perf_counter()
        pl.tables(cnt // (reps + 1))
        host = (time.perf_counter() - t0) * 1e3
        out += [f"slabs = {slabs} ({rows} rows):", line("density pass (ls1hip_planar_density)", t["planar_density"]),
                line("table build (ls1hip_planar_tables)", t["planar_tables"]), line("apply pass (ls1hip_planar_apply)", t["planar_apply"]),
                line("kick + drift pass (ls1hip_kick_drift, dt = 0)", t["integrate"]),
                f"  density + apply of one step / kick + drift        {(np.median(t['planar_density']) + np.median(t['planar_apply'])) / kd:.3f}",
                f"  per step at frequency 10 (density / 10 + apply)    {per_step:.3f} ms = {per_step / kd:.3f} x kick + drift",
                f"  table build / 10 against kick + drift              {np.median(t['planar_tables']) / 10 / kd:.3f}",
                f"  the same tables by tests/planar_ref.py (numpy, host) {host:.1f} ms"]
    e.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--n-per-dim", type=int, default=171, help="2 n^3 molecules before carving (171: configs[1])")
    ap.add_argument("--ethane-k", type=int, default=10, help="replication of the reference's ethane box per dimension (10: bench.py's)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    import bench
    import planar_ref
    inp = importlib.import_module("ls1-mardyn_amd.inp")
    synth = importlib.import_module("ls1-mardyn_amd.synth")
    engine_mod = importlib.import_module("ls1-mardyn_amd.engine")
    e, N, L = film_engine(torch, bench, inp, synth, engine_mod, args.n_per_dim)
    out = [f"planar long-range correction against the kick + drift pass (tools/planar_time.py --reps {args.reps}), {torch.cuda.get_device_name(0)}",
           f"film of N = {N} single-centre LJ molecules in a box of {L:.3f}^3, r_c {bench.RC}"]
    measure(e, N, [L, L, L], bench.lj_components(inp), bench.RC, args.reps, planar_ref, out)
    torch.cuda.empty_cache()
    e, N, length, comps = ethane_engine(bench, inp, engine_mod, args.ethane_k)
    out += [f"film of N = {N} 2CLJ ethane molecules (rigid rotors, two LJ sites) in a box of {length[0]:.3f}^3, r_c {bench.ETHANE_RC}"]
    measure(e, N, length, comps, bench.ETHANE_RC, args.reps, planar_ref, out)
    text = "\n".join(out) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()

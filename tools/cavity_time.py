#!/usr/bin/env python3
"""Cost of the cavity pass (ls1hip_cavity_sample) against the per-step brick force pass and against the insertion pass fed the same
nodes, same build, same process, same state.

    python tools/cavity_time.py [--reps 10] [--n-per-dim 171] [--probe 200000] [--out profiles/cavity_pass.txt]

Box: configs[1] of bench.py (2 n^3 single-centre LJ molecules, 171: N = 10 000 422, r_c 2.5 sigma) after 100 steps.  Lattices with
spacings of about 0.5 and 1 sigma over the whole domain, R = 1 sigma (maxNeighbours 2) and R = r_c (maxNeighbours 20), flag mode and
count mode.  Per combination the force pass, the cavity pass and ls1hip_insertion_energies on `probe` randomly chosen nodes of the
lattice ALTERNATE `reps` times, each call timed by the library's HIP events (ls1hip_timing "force" / "cavity" / "insert").  The
expectation from counted work is written BEFORE the measurement of each combination."""
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


def tile_shape(n, h, R):
    """cavity_tile_shape of kernels_cavity.hip: fewest staged candidates per node"""
    best = None
    for a in range(1, min(256, n) + 1):
        for b in range(1, min(256 // a, n) + 1):
            c = min(256 // (a * b), n)
            cost = ((a - 1) * h + 2 * R) * ((b - 1) * h + 2 * R) * ((c - 1) * h + 2 * R) / (a * b * c)
            if best is None or cost < best[0]:
                best = (cost, (a, b, c))
    return best


def line(tag, a):
    return f"  {tag:<40s} median {np.median(a):9.3f} ms   min {a.min():9.3f}   max {a.max():9.3f}   (n = {len(a)})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--n-per-dim", type=int, default=171)
    ap.add_argument("--probe", type=int, default=200000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    import bench
    inp = importlib.import_module("ls1-mardyn_amd.inp")
    synth = importlib.import_module("ls1-mardyn_amd.synth")
    engine_mod = importlib.import_module("ls1-mardyn_amd.engine")
    n = args.n_per_dim
    N, L, rc = 2 * n ** 3, synth.box_length(n, bench.RHO), bench.RC
    e = engine_mod.DeviceEngine(0)
    e.set_components(bench.lj_components(inp), rc)
    e.set_domain([L, L, L])
    e.upload_begin(N)
    for ids_t, r_t, v_t in synth.bcc_chunks_device(torch, torch.device("cuda", 0), n, rho=bench.RHO, temp=bench.TEMP):
        torch.cuda.synchronize()
        e.upload_chunk_device(ids_t.numel(), ids_t.data_ptr(), 0, r_t.data_ptr(), v_t.data_ptr())
    del ids_t, r_t, v_t
    e.upload_end()
    e.rebin(); e.halo(); e.forces(0)
    e.run(bench.DT, 100)
    e.rebin(); e.halo(); e.forces(0)
    e.timing_enable(1)
    cells = e.grid()[0] - 2
    per_cell = N / float(np.prod(cells))
    out = [f"Cavity pass against the per-step brick force pass and the insertion pass on the same nodes (tools/cavity_time.py --reps {args.reps}), "
           f"{torch.cuda.get_device_name(0)}, FP64",
           f"configs[1]: N = {N}, L = {L:.3f}, r_c {rc}, {per_cell:.1f} molecules per cell, after 100 steps; kernel family of the force pass: "
           f"{e.get_option('last_force_kernel')}",
           f"counted work of the force pass: 27 cells x {per_cell:.1f} = {27 * per_cell:.0f} candidate tests per molecule, {27 * per_cell * N:.3g} in all; of the "
           f"insertion pass: the same {27 * per_cell:.0f} candidates per NODE, read from global memory by one wave per node ({27 * per_cell * 24 / 1024:.1f} KB)"]
    rng = np.random.default_rng(5)
    for spacing in (0.5, 1.0):
        K = int(round(L / spacing))
        h = L / K
        for R, max_nb in ((1.0, 2), (rc, 20)):
            cost, shape = tile_shape(K, h, R)
            tests = cost * float(np.prod(shape)) * bench.RHO  # every lane tests every candidate of its tile
            out += [f"lattice {K}^3 = {K ** 3} nodes (spacing {h:.4f}), R = {R}, maxNeighbours {max_nb}: tile {shape}",
                    f"  expectation (count mode): {tests:.0f} pair tests and {tests * 28 / np.prod(shape):.1f} staged bytes per node, "
                    f"{tests * K ** 3:.3g} pair tests = {tests * K ** 3 / (27 * per_cell * N):.2f} x the candidate tests of the force pass, each without a force "
                    f"body: about that multiple of the force pass or less; flag mode below count mode (liquid nodes are decided early); per node "
                    f"{27 * per_cell / tests:.1f} x fewer tests than the insertion pass and no global read per test: faster per node by more than that"]
            e.cavity_config(K, K, K, max_nb, R)
            t = rng.integers(0, K, size=(args.probe, 3))
            probe = (0.5009756 + t) * h
            cid = np.zeros(args.probe, dtype=np.int32)
            res = {}
            for mode, tag in ((0, "flag mode"), (1, "count mode")):
                e.set_option("cavity_counts", mode)
                e.forces(0, want_macro=False); e.cavity_sample(); e.insertion_energies(cid, probe)  # warm-up
                f, c, i = [], [], []
                for _ in range(args.reps):
                    f.append(one_call(e, "force", lambda: e.forces(0, want_macro=False)))
                    c.append(one_call(e, "cavity", e.cavity_sample))
                    i.append(one_call(e, "insert", lambda: e.insertion_energies(cid, probe)))
                f, c, i = np.array(f), np.array(c), np.array(i)
                res[mode] = e.cavity_read()["n_active"]
                per_node_c, per_node_i = np.median(c) / K ** 3, np.median(i) / args.probe
                out += [f"  {tag}: {res[mode]} cavities", line("force pass (ls1hip_forces)", f), line("cavity pass (ls1hip_cavity_sample)", c),
                        line(f"insertion pass, {args.probe} of the nodes", i),
                        f"  cavity / force (medians) {np.median(c) / np.median(f):.3f}   per node: cavity {per_node_c * 1e6:.3f} ns, insertion "
                        f"{per_node_i * 1e6:.3f} ns, insertion / cavity {per_node_i / per_node_c:.1f}"
                        + ("" if per_node_c < per_node_i else "   THE TILE PASS DOES NOT BEAT THE INSERTION PATH HERE")]
            assert res[0] == res[1], res
    e.close()
    text = "\n".join(out) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()

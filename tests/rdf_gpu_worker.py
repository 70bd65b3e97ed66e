"""Worker for tests/test_gpu_rdf.py: one rank of a two-PROCESS world (gloo, both ranks on cuda:0, messages staged through the
host as in tests/decomp_gpu_worker.py).  Every rank samples the RDF of its sub-box after the initial force traversal and
decomp.rdf_collect sums the local histograms with one all-reduce; rank 0 writes the global and its local counts to an .npz."""
import importlib
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)


def main():
    out_path = sys.argv[1]
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    torch.cuda.set_device(0)
    decomp = importlib.import_module("ls1-mardyn_amd.decomp")
    engine_mod = importlib.import_module("ls1-mardyn_amd.engine")
    inp = importlib.import_module("ls1-mardyn_amd.inp")
    data = np.load(os.environ["LS1_TEST_INPUT"])
    L, r, v, ids, rc = data["L"], data["r"], data["v"], data["ids"], float(data["rc"])
    comps = inp.ComponentSet([inp.make_component(lj=[(0, 0, 0, 1, 1, 1, rc, 0)])], np.zeros((0, 2)), 1e10)
    dc = decomp.CartesianDecomposition(world, rank, L)
    lo, hi = dc.bounding_box()
    mine = np.all((r >= lo) & (r < hi), axis=1)
    eng = engine_mod.DeviceEngine(0)
    eng.set_components(comps, rc)
    eng.set_domain(L, lo, hi, rank, dc.neighbor_table())
    eng.upload(ids[mine], np.zeros(int(mine.sum()), np.int32), r[mine], v[mine])
    sim = decomp.DistributedSimulation(dc, eng, dist, torch.device("cuda", 0), stage_through_host=True)
    sim.initial_forces()
    eng.rdf_config(int(data["bins"]), float(data["dr"]), True)
    eng.rdf_sample()
    local = eng.rdf_read()
    glob = decomp.rdf_collect(eng, dist)
    if rank == 0:
        np.savez(out_path, mol=glob["mol"], n=glob["n_per_component"], samples=glob["samples"], local_mol=local["mol"],
                 local_n=local["n_per_component"])
    eng.close()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()

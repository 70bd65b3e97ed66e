"""Brute-force restatement of CavityEnsemble::countNeighbours / decideActivity (ensemble/CavityEnsemble.cpp:254-311) on the node
lattice of CavityEnsemble::init (:158-171): all molecules wrapped into the box, NO minimum image, RR formed in float32, the id clash."""
import numpy as np


def lattice(N, L, cv=None):
    """positions [Nx Ny Nz, 3] and ids tid [Nx Ny Nz] of the nodes; cv = (lo[3], hi[3]) or None (the whole domain)"""
    lo, hi = (np.zeros(3), np.asarray(L, float)) if cv is None else (np.asarray(cv[0], float), np.asarray(cv[1], float))
    ax = [lo[d] + (0.5009756 + np.arange(N[d])) * ((hi[d] - lo[d]) / float(N[d])) for d in range(3)]
    pos = np.stack(np.meshgrid(*ax, indexing="ij"), axis=-1).reshape(-1, 3)
    return pos, np.arange(1, len(pos) + 1, dtype=np.uint64)


def cavity_ref(r, ids, L, N, radius, cv=None, images=False):
    """(counts [Nx, Ny, Nz], hit [nodes, molecules] before the id clash, margin = min | |d| / R - 1 |); images=True: the minimum-image
    count the reference does NOT take (to show that a case has nodes where it matters)"""
    L = np.asarray(L, float)
    r = np.asarray(r, float) - L * np.floor(np.asarray(r, float) / L)
    RR = float(np.float32(radius) * np.float32(radius))
    pos, tid = lattice(N, L, cv)
    d = r[None, :, :] - pos[:, None, :]
    if images:
        d -= L * np.round(d / L)
    dd = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]
    hit = dd < RR
    counts = (hit & (np.asarray(ids, np.uint64)[None, :] != tid[:, None])).sum(axis=1).astype(np.uint32)
    return counts.reshape(tuple(N)), hit, float(np.abs(np.sqrt(dd / RR) - 1.).min())


def flags_of(counts, max_neighbours):
    return (counts <= max_neighbours).astype(np.uint8)


def cav_xyz_lines(counts, max_neighbours, L, cid, cv=None):
    """the lines of CavityWriter::endStep's file (io/CavityWriter.cpp:201-235) for one rank: count, "comment line", the active nodes
    in ascending tid with operator<<'s six significant digits, and the empty string behind the last newline"""
    pos, _ = lattice(counts.shape, L, cv)
    el = ("C ", "N ", "O ", "F ")[cid] if cid < 4 else "Ne "
    act = pos[flags_of(counts, max_neighbours).reshape(-1) != 0]
    return ["%d" % len(act), "comment line"] + [el + "\t".join("%.6g" % x for x in p) for p in act] + [""]

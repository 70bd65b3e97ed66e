"""The RDF yardstick of the tests: a brute-force numpy restatement of the reference's RDF sampling rules (io/RDF.h:111-170,
adapter/RDFCellProcessor.cpp:34,63), the reader of the reference's .rdf files, and the golden cases of tests/golden/rdf/.

The restatement is O(N^2), minimum image (boxes are at least two cutoffs long), chunked over i.  It is pinned to the real
reference by tests/test_rdf_cpu.py and then serves the GPU tests where no golden file exists."""
import functools
import os
import re

import numpy as np

from golden_io import GOLDEN, input_path

RDF_GOLDEN = os.path.join(GOLDEN, "rdf")
# a fixture state is usable only if no molecule or site distance lies this close (absolute) to a bin edge, r_c or bins * dr:
# 10 x the 1e-9 to which trajectories here agree with the reference
EDGE_MARGIN = 1e-8


def cases():
    """Golden cases of MANIFEST_rdf.txt: name -> dict(input, rc, dt, temperature, bins, dr, steps)."""
    out = {}
    with open(os.path.join(RDF_GOLDEN, "MANIFEST_rdf.txt")) as fh:
        for ln in fh:
            if ln.startswith("#") or not ln.strip():
                continue
            name, inp, rc, dt, temp, bins, dr, steps = ln.split()
            out[name] = dict(name=name, input=inp, rc=float(rc), dt=float(dt), temperature=float(temp), bins=int(bins), dr=float(dr),
                             steps=int(steps))
    return out


def site_table(comps):
    """Per component the body-frame site positions [n_sites, 3] in the reference's site order: LJ centres, charges, dipoles,
    quadrupoles (FullMolecule.h:171-185)."""
    return [np.concatenate([np.asarray(t, dtype=np.float64)[:, :3] for t in (c.lj, c.charges, c.dipoles, c.quadrupoles)], axis=0)
            for c in comps.components]


def rotmat(q):
    """Rotation matrices [n, 3, 3] of the NORMALISED quaternions (Quaternion::rotate, Quaternion.cpp:45-61)."""
    q = np.asarray(q, dtype=np.float64)
    q = q / np.sqrt((q * q).sum(axis=1))[:, None]
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = np.empty((len(q), 3, 3))
    R[:, 0, 0] = w * w + x * x - y * y - z * z
    R[:, 0, 1] = 2. * (x * y - w * z)
    R[:, 0, 2] = 2. * (w * y + x * z)
    R[:, 1, 0] = 2. * (w * z + x * y)
    R[:, 1, 1] = w * w - x * x + y * y - z * z
    R[:, 1, 2] = 2. * (y * z - w * x)
    R[:, 2, 0] = 2. * (x * z - w * y)
    R[:, 2, 1] = 2. * (w * x + y * z)
    R[:, 2, 2] = w * w - x * x - y * y + z * z
    return R


def pair_index(i, j, nC):
    return i * nC - (i * (i - 1)) // 2 + (j - i)


def _edge_margin(d, rc, bins, dr):
    """smallest absolute distance of the distances d to a bin edge (k * dr, k = 0..bins), to r_c and to bins * dr"""
    d = np.asarray(d, dtype=np.float64).reshape(-1)
    if d.size == 0:
        return np.inf
    m = min(np.min(np.abs(d - rc)), np.min(np.abs(d - bins * dr)))
    inside = d[d < (bins + 0.5) * dr]
    if inside.size:
        x = inside / dr
        m = min(m, float(np.min(np.abs(x - np.round(x))) * dr))
    return float(m)


def brute_force(r, q, cid, comps, L, rc, bins, dr, periodic=True, site_rdf=True, chunk=512):
    """Histograms of ONE configuration by the rules of RDF::observeRDF.  Returns dict(mol uint64 [pairs, bins], site = list of
    uint64 [n_i, n_j, bins] blocks (pairs with n_i + n_j > 2, order of RDF::collectRDF), site_pairs, n_per_component,
    margin = smallest distance of any observed molecule / site distance to a bin edge, r_c or bins * dr)."""
    r = np.asarray(r, dtype=np.float64)
    cid = np.asarray(cid, dtype=np.int64)
    L = np.asarray(L, dtype=np.float64)
    N, nC = len(r), len(comps.components)
    ns = [int(c.n_sites) for c in comps.components]
    rc2 = rc * rc
    maxd2 = dr * dr * float(bins) * float(bins)  # RDF.cpp:47
    mol = np.zeros((nC * (nC + 1) // 2, bins), dtype=np.uint64)
    margin = np.inf
    pi_, pj_, pd_ = [], [], []
    reach = max(rc, bins * dr) + 2 * EDGE_MARGIN
    # all pairs, chunked over i in the order of x; the only pruning is exact: a chunk meets the molecules whose (minimum-image) x
    # distance to the chunk's x range is below the reach
    order = np.argsort(r[:, 0], kind="stable")
    for i0 in range(0, N, chunk):
        isel = order[i0:min(N, i0 + chunk)]
        xlo, xhi = r[isel[0], 0], r[isel[-1], 0]
        dxc = r[:, 0] - 0.5 * (xlo + xhi)
        if periodic:
            dxc -= L[0] * np.round(dxc / L[0])
        jsel = np.nonzero(np.abs(dxc) <= 0.5 * (xhi - xlo) + reach + 1e-6)[0]
        d = r[None, jsel, :] - r[isel, None, :]  # r_j - r_i
        if periodic:
            d -= L * np.round(d / L)
        dd = d[:, :, 0] * d[:, :, 0] + d[:, :, 1] * d[:, :, 1] + d[:, :, 2] * d[:, :, 2]
        upper = jsel[None, :] > isel[:, None]  # every unordered pair once
        near = upper & (dd < reach * reach)
        margin = min(margin, _edge_margin(np.sqrt(dd[near]), rc, bins, dr))
        ii, jj = np.nonzero(upper & (dd < rc2))
        ddp = dd[ii, jj]
        pd_.append(d[ii, jj])
        ii, jj = isel[ii], jsel[jj]
        pi_.append(ii)
        pj_.append(jj)
        keep = ~(ddp > maxd2)
        b = np.floor(np.sqrt(ddp[keep]) / dr)
        ok = b < bins
        ci, cj = cid[ii][keep][ok], cid[jj][keep][ok]
        ca, cb = np.minimum(ci, cj), np.maximum(ci, cj)
        p = ca * nC - (ca * (ca - 1)) // 2 + (cb - ca)
        np.add.at(mol, (p, b[ok].astype(np.int64)), 1)
    ii, jj, dv = np.concatenate(pi_), np.concatenate(pj_), np.concatenate(pd_)
    site_pairs = [(a, b) for a in range(nC) for b in range(a, nC) if ns[a] + ns[b] > 2] if site_rdf else []
    site = {p: np.zeros((ns[p[0]], ns[p[1]], bins), dtype=np.uint64) for p in site_pairs}
    if site_pairs:
        S = site_table(comps)
        R = rotmat(q)
        ci, cj = cid[ii], cid[jj]
        for a in range(nC):
            for b in range(nC):
                key = (min(a, b), max(a, b))
                if key not in site:
                    continue
                sel = np.nonzero((ci == a) & (cj == b))[0]
                if not sel.size:
                    continue
                Si = np.einsum("pkl,ml->pmk", R[ii[sel]], S[a])  # rotated site offsets of i [p, m, 3]
                Sj = np.einsum("pkl,nl->pnk", R[jj[sel]], S[b])
                # absolute site positions: r_i + d_m and r_j + d_n, r_j = r_i + (r_j - r_i)
                D = Si[:, :, None, :] - (dv[sel][:, None, None, :] + Sj[:, None, :, :])
                d2 = D[..., 0] * D[..., 0] + D[..., 1] * D[..., 1] + D[..., 2] * D[..., 2]  # [p, m, n]
                margin = min(margin, _edge_margin(np.sqrt(d2[d2 < (bins * dr + dr) ** 2]), np.inf, bins, dr))
                bn = np.floor(np.sqrt(d2) / dr)
                ok = ~(d2 > maxd2) & (bn < bins)
                pp, mm, nn = np.nonzero(ok)
                bb = bn[pp, mm, nn].astype(np.int64)
                blk = site[key]
                if a > b:  # (i, j) and (m, n) swapped
                    np.add.at(blk, (nn, mm, bb), 1)
                else:
                    np.add.at(blk, (mm, nn, bb), 1)
                    if a == b:  # the reference's double count of m != n
                        off = mm != nn
                        np.add.at(blk, (nn[off], mm[off], bb[off]), 1)
    return dict(mol=mol, site=[site[p] for p in site_pairs], site_pairs=site_pairs,
                n_per_component=np.bincount(cid, minlength=nC).astype(np.uint64), samples=1, margin=float(margin))


def add_counts(a, b):
    """sum of two count dicts (samples add up too)"""
    return dict(mol=a["mol"] + b["mol"], site=[x + y for x, y in zip(a["site"], b["site"])], site_pairs=a["site_pairs"],
                n_per_component=a["n_per_component"] + b["n_per_component"], samples=a["samples"] + b["samples"],
                margin=min(a.get("margin", np.inf), b.get("margin", np.inf)))


_NUM = re.compile(r"^[+-]?(\d+\.?\d*|\.\d+)([eE][+-]?\d+)?$")


def is_number(tok):
    return bool(_NUM.match(tok))


def read_rdf(text):
    """The text of a .rdf file of RDF::writeToFile (RDF.cpp:457-571): dict(lines, ctr_i, ctr_j, rows = token lists of the data lines)."""
    lines = text.split("\n")
    out = dict(lines=lines, rows=[])
    for ln in lines:
        if ln.startswith("# ctr_i:"):
            out["ctr_i"] = int(ln.split(":")[1])
        elif ln.startswith("# ctr_j:"):
            out["ctr_j"] = int(ln.split(":")[1])
        elif ln and not ln.startswith("#"):
            out["rows"].append(ln.split())
    return out


@functools.lru_cache(maxsize=None)
def _golden_archive(case):
    """the reference's .rdf files of a case, kept as one <case>.tar.gz (the five-component files carry 25 site columns: 2.5 MB of text)"""
    import tarfile
    with tarfile.open(os.path.join(RDF_GOLDEN, case + ".tar.gz"), "r:gz") as tf:
        return {m.name: tf.extractfile(m).read().decode() for m in tf.getmembers() if m.isfile()}


def golden_text(case, i, j, step):
    return _golden_archive(case)["rdf_%d-%d.%09d.rdf" % (i, j, step)]


def golden_mol_counts(case, nC, bins, step):
    """Npair(curr.) of every component pair at one step: with one sample per file the raw integer count (exact at precision(5)
    below 10^5) -> uint64 [pairs, bins]; and ctr per component"""
    mol = np.zeros((nC * (nC + 1) // 2, bins), dtype=np.uint64)
    ctr = np.zeros(nC, dtype=np.uint64)
    for i in range(nC):
        for j in range(i, nC):
            g = read_rdf(golden_text(case, i, j, step))
            assert len(g["rows"]) == bins
            col = [float(row[6]) for row in g["rows"]]
            assert all(c == int(c) and c < 1e5 for c in col)
            mol[pair_index(i, j, nC)] = np.array(col).astype(np.uint64)
            ctr[i], ctr[j] = g["ctr_i"], g["ctr_j"]
    return mol, ctr


@functools.lru_cache(maxsize=None)
def case_states(name):
    """The fixture of a golden case advanced with the CPU oracle under the driver's global velocity-scaling thermostat: list over
    steps 1..n of dict(r, q) (id order), plus the static data.  Computed once per process and shared; callers do not modify it."""
    import importlib

    from golden_io import sorted_phase_space
    from oracle.oracle import Oracle

    inp = importlib.import_module("ls1-mardyn_amd.inp")
    c = cases()[name]
    ps = inp.read_inp(input_path(c["input"]))
    s = sorted_phase_space(ps)
    orc = Oracle(ps.components.flat(), c["rc"])
    r, v, q, D = s["r"].copy(), s["v"].copy(), s["q"].copy(), s["D"].copy()
    out = orc.forces(r, q, s["cid"], ps.length, True)
    F, M = out["F"].copy(), out["M"].copy()
    states = []
    for _ in range(c["steps"]):
        orc.step(c["dt"], s["cid"], r, v, q, D, F, M, ps.length, True, target_T=c["temperature"])
        states.append(dict(r=r.copy(), q=q.copy()))
    return dict(case=c, ps=ps, ids=s["ids"], cid=s["cid"], states=states)


@functools.lru_cache(maxsize=None)
def case_counts(name, step):
    """brute_force of a golden case at step 1..n (shared, unchanged by the callers)"""
    cs = case_states(name)
    c, st = cs["case"], cs["states"][step - 1]
    return brute_force(st["r"], st["q"], cs["cid"], cs["ps"].components, cs["ps"].length, c["rc"], c["bins"], c["dr"])

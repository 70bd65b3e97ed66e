"""Cavities without a GPU: (1) the restatement the GPU tests use as their yardstick (tests/cavity_ref.py) reproduces the count and every
printed line the REAL reference wrote (tests/golden/cavity/, made by tests/golden/make_cavity_golden.py from the unmodified driver with
its CavityWriter plugin), and mirror.CavityWriter writes that file; (2) mirror.CavityWriter's file name, format and rank-by-rank order
(io/CavityWriter.cpp:176-237) and decomp.cavity_collect / cavity_assemble on hand-made flags."""
import os

import numpy as np
import pytest

from cavity_ref import cav_xyz_lines, cavity_ref, flags_of, lattice
from conftest import load_pkg
from golden_io import GOLDEN, input_path

inp = load_pkg("inp")

mirror = load_pkg("mirror")
decomp = load_pkg("decomp")

N, L = (2, 3, 2), (10.0, 12.0, 8.0)


def _golden_cases():
    rows = [ln.split() for ln in open(os.path.join(GOLDEN, "cavity", "MANIFEST_cavity.txt")) if ln.strip() and not ln.startswith("#")]
    return [(r[0], r[1], tuple(int(k) for k in r[3:6]), float(r[6]), int(r[7]), [int(k) for k in r[8].split(",")]) for r in rows]


@pytest.mark.parametrize("name,fname,lat,radius,max_nb,cids", _golden_cases())
def test_restatement_and_writer_give_the_reference_files(tmp_path, name, fname, lat, radius, max_nb, cids):
    """five components (all count), ids 58 ... 629 inside the node ids (the clash decides a flag), r_c = 35 in a box of 134 (a third of
    the flags would differ with periodic images)"""
    ps = inp.read_inp(input_path(fname))
    counts, hit, margin = cavity_ref(ps.r, ps.ids, ps.length, lat, radius)
    assert margin > 1e-9
    flags = flags_of(counts, max_nb)
    assert (flags_of(hit.sum(axis=1), max_nb) != flags.reshape(-1)).any()
    assert (flags_of(cavity_ref(ps.r, ps.ids, ps.length, lat, radius, images=True)[0], max_nb) != flags).sum() > flags.size // 4
    w = mirror.CavityWriter(ps.length, outputprefix=name, maxNeighbours=max_nb, radius=radius, Nx=lat[0], Ny=lat[1], Nz=lat[2], componentid=cids)
    w.setGlobal(dict(lo=np.zeros(3, int), n=np.array(lat), flags=flags, n_active=int(flags.sum())))
    names = w.endStep(None, None, None, 0, str(tmp_path))
    assert [os.path.basename(f) for f in names] == ["%s-c%d-0.cav.xyz" % (name, k) for k in cids]
    for k, mine in zip(cids, names):
        want = open(os.path.join(GOLDEN, "cavity", "%s-c%d-0.cav.xyz" % (name, k))).read()
        assert want.split("\n")[0] == str(int(flags.sum())) and want.split("\n") == cav_xyz_lines(counts, max_nb, ps.length, k)
        assert open(mine).read() == want


def _fake_dist(me, sent):
    """two ranks of torch.distributed in one process: rank `me` sees the tensors the others would send (count, meta, padded flags)"""
    from types import SimpleNamespace
    calls = []

    def all_gather(out, t, group=None):
        calls.append(0)
        for k, o in enumerate(out):
            o.copy_(t if k == me else sent[k][len(calls)])

    return SimpleNamespace(is_available=lambda: True, is_initialized=lambda: True, get_world_size=lambda group=None: len(sent),
                           all_reduce=lambda t, group=None: t.copy_(sum(x[0] for x in sent)), all_gather=all_gather)


def test_collect_across_two_ranks_pads_and_orders_the_pieces():
    """rank 0 owns one y-plane (4 nodes), rank 1 two (8 nodes): the shorter flags are zero-padded for the all-gather and cut back"""
    import torch
    f = _flags()
    ranks = [_Rank(f, 0, 1), _Rank(f, 1, 3)]
    sent = []
    for r in ranks:
        fl = np.zeros(8, dtype=np.uint8)
        fl[:r.res["flags"].size] = r.res["flags"].reshape(-1)
        sent.append((torch.tensor([r.res["n_active"]]), torch.from_numpy(np.concatenate([r.res["lo"], r.res["n"]]).astype(np.int64)), torch.from_numpy(fl)))
    for me in (0, 1):
        glob = decomp.cavity_collect(ranks[me], N, dist=_fake_dist(me, sent))
        assert np.array_equal(glob["flags"], f) and glob["n_active"] == 4
        assert [tuple(p[1]) for p in glob["pieces"]] == [(2, 1, 2), (2, 2, 2)]


class _Rank:
    """what DeviceEngine.cavity_read returns for one half of the lattice split along y"""

    def __init__(self, flags, y0, y1):
        self.res = dict(lo=np.array([0, y0, 0]), n=np.array([2, y1 - y0, 2]), flags=flags[:, y0:y1], n_active=int(flags[:, y0:y1].sum()))

    def cavity_read(self):
        return self.res


def _flags():
    f = np.zeros(N, dtype=np.uint8)
    f[0, 0, 1] = f[0, 2, 0] = f[1, 1, 1] = f[1, 2, 1] = 1
    return f


def test_two_half_lattices_join_and_must_partition():
    f = _flags()
    parts = [decomp.cavity_collect(_Rank(f, 0, 1), N), decomp.cavity_collect(_Rank(f, 1, 3), N)]
    glob = decomp.cavity_assemble([p["pieces"][0] for p in parts], N, sum(p["n_active"] for p in parts))
    assert np.array_equal(glob["flags"], f) and glob["n_active"] == 4 and len(glob["pieces"]) == 2
    with pytest.raises(ValueError, match="partition"):
        decomp.cavity_assemble([parts[0]["pieces"][0]] * 2, N, 0)


@pytest.mark.parametrize("cid,element,incremental,name", [(0, "C ", 1, "cav-c0-007.cav.xyz"), (3, "F ", 0, "cav-c3.cav.xyz"),
                                                          (7, "Ne ", 1, "cav-c7-007.cav.xyz")])
def test_writer_name_and_format(tmp_path, cid, element, incremental, name):
    f = _flags()
    w = mirror.CavityWriter(L, writefrequency=5, outputprefix="cav", incremental=incremental, maxNeighbours=3, radius=1.5, Nx=2, Ny=3, Nz=2,
                            componentid=[cid], numTimesteps=1000)  # ceil(log10(1000 / 5)) = 3 digits
    pos = lattice(N, L)[0].reshape(N + (3,))
    line = lambda p: element + "\t".join("%.6g" % x for x in p)  # noqa: E731
    w.setGlobal(_Rank(f, 0, 3).res)
    assert w.endStep(None, None, None, 34, str(tmp_path)) == []  # 34 % 5 != 0
    (path,) = w.endStep(None, None, None, 35, str(tmp_path))
    assert path == str(tmp_path / name)
    assert open(path).read().split("\n") == ["4", "comment line"] + [line(pos[k]) for k in ((0, 0, 1), (0, 2, 0), (1, 1, 1), (1, 2, 1))] + [""]
    # two ranks split along y: rank by rank, ascending tid inside a rank — not the global tid order
    a, b = _Rank(f, 0, 1).res, _Rank(f, 1, 3).res
    w.setGlobal(dict(n_active=4, pieces=[(a["lo"], a["n"], a["flags"]), (b["lo"], b["n"], b["flags"])]))
    assert w.render(cid).split("\n")[2:6] == [line(pos[k]) for k in ((0, 0, 1), (0, 2, 0), (1, 1, 1), (1, 2, 1))]
    w.setGlobal(dict(n_active=4, pieces=[(b["lo"], b["n"], b["flags"]), (a["lo"], a["n"], a["flags"])]))
    assert w.render(cid).split("\n")[2:6] == [line(pos[k]) for k in ((0, 2, 0), (1, 1, 1), (1, 2, 1), (0, 0, 1))]

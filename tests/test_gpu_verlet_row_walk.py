"""GPU tests of the scalar row walk of the list force pass (brick_forces, kernels_force_verlet.hip): a tile's row count, last
row, loop index and row base live in scalar registers, a row is addressed as scalar base + one 32-bit per-lane offset, the
`k + n < nw` tests are scalar branches, the split tiles walk byte offsets.  One constructed box reaches the corners, compared with
the generic kernel (one evaluation) and with the per-step kernels (a few fused steps) at the suite's 1e-10.

The box: the 2 * 16^3 jittered bcc liquid (8 x 8 x 8 cells of 2.73 at skin 0.2 = 2 x 2 x 4 bricks of 4 x 4 x 2 cells, 512 owned
molecules per full-density brick), thinned by cell layer in z — brick layer 0 full, layer 1 a half (a sixth next to layer 2),
layer 2 a twelfth, layer 3 a sixth to a third — and then edited cell by cell (cells as grid_init forms them):
  * layer 2 sees only dilute neighbours: every molecule has at most 14 neighbours within rc + skin (checked here on the host), so
    its tiles have the minimum of 4 word rows, and most of their lanes hold no molecule;
  * layers 1 and 3 and the interfaces give tiles of 5 .. 20 rows — every residue of the row count mod 4: the rows past the end
    are clamped loads that must be skipped, not evaluated;
  * the four bricks of layer 0 own 516 / 524 / 536 / 548 molecules: leftover tiles of 4 / 12 / 24 / 36 molecules = split tiles of
    8 / 4 / 2 / 1 lanes per molecule, with odd and even trip counts;
  * the list build sees rows (three x-neighbour cells) of exactly 32, 33 and 64 candidates, an empty column of three cells next to
    full ones, the dilute layers, and one cell with more than 32 molecules inside a regular brick;
  * skin 0.12 and 0.3 move every list length; at skin 0.3 the box has 7 cells per dimension and its full bricks own more than 640
    molecules: irregular bricks whose second-pass tiles are listed and whose last molecules are evaluated directly;
  * `cluster`: 85 more molecules within a sphere of radius 2 in the half-density layer: more than 96 neighbours — the tile is
    marked as overflowed and evaluated directly (its brick becomes irregular)."""
import numpy as np
import pytest

from conftest import load_pkg
from golden_io import rel_max

pytestmark = pytest.mark.gpu

inp = load_pkg("inp")
capi = load_pkg("capi")
engine_mod = load_pkg("engine")
synth = load_pkg("synth")

RC = 2.5
NC = 8  # cells per dimension at skin 0.2 (floor(21.85 / 2.7))


def _lj():
    return inp.ComponentSet([inp.make_component(lj=[(0, 0, 0, 1, 1, 1, RC, 0)])], np.zeros((0, 2)), 1e10)


def _engine(L, ids, r, v, skin=None, **opts):
    e = engine_mod.DeviceEngine(0)
    e.set_components(_lj(), RC)
    for k, val in opts.items():
        e.set_option(k, val)
    e.set_verlet(skin, force=True)
    e.set_domain([L] * 3)
    e.upload(ids, np.zeros(len(ids), np.int32), r, v)
    e.rebin(); e.halo(); e.forces(0)
    return e


def _state(e):
    st = e.download_state()
    o = np.argsort(st["ids"], kind="stable")
    return st["ids"][o], st["r"][o], st["v"][o], e.download_forces()["F"][o]


class _Box:
    """positions edited by cell ranges of the skin-0.2 grid; new molecules keep a minimum (periodic) distance to all others"""

    def __init__(self, seed):
        self.L, _, r, _ = synth.bcc_box(16)
        self.r = r.copy()
        self.cl = self.L / NC
        self.rng = np.random.default_rng(seed)

    def cells(self, r=None):
        r = self.r if r is None else r
        return np.clip(np.floor(r / self.cl).astype(int), 0, NC - 1)

    def inside(self, lo, hi):
        c = self.cells()
        return np.all((c >= np.asarray(lo)) & (c < np.asarray(hi)), axis=1)

    def thin(self, keep_of_cell):
        c = self.cells()
        self.r = self.r[self.rng.random(len(self.r)) < keep_of_cell(c)]

    def add(self, k, sample, dmin):
        for _ in range(k):
            for _try in range(4000):
                p = sample()
                d = self.r - p
                d -= self.L * np.round(d / self.L)
                if np.min((d * d).sum(1)) >= dmin * dmin:
                    self.r = np.concatenate([self.r, p[None]])
                    break
            else:
                raise AssertionError("no room for another molecule")

    def set_count(self, lo, hi, target, edit_lo=None, edit_hi=None, dmin=0.7):
        """exactly `target` molecules in the cell range [lo, hi): molecules are removed from / added to [edit_lo, edit_hi)"""
        edit_lo, edit_hi = np.asarray(lo if edit_lo is None else edit_lo), np.asarray(hi if edit_hi is None else edit_hi)
        n = int(self.inside(lo, hi).sum())
        if n > target:
            idx = np.flatnonzero(self.inside(edit_lo, edit_hi))
            assert len(idx) >= n - target
            self.r = np.delete(self.r, self.rng.choice(idx, n - target, replace=False), axis=0)
        elif n < target:
            a, b = (edit_lo + 0.02) * self.cl, (edit_hi - 0.02) * self.cl
            self.add(target - n, lambda: a + (b - a) * self.rng.random(3), dmin)
        assert int(self.inside(lo, hi).sum()) == target


def _neighbours(r, L, cut):
    """molecules within `cut` of every molecule (periodic; 4000 molecules: brute force in slabs)"""
    nn = np.zeros(len(r), int)
    for i0 in range(0, len(r), 256):
        d = r[None, :, :] - r[i0:i0 + 256, None, :]
        d -= L * np.round(d / L)
        nn[i0:i0 + 256] = ((d * d).sum(2) < cut * cut).sum(1) - 1
    return nn


_BOXES = {}


def _corner_box(cluster):
    if cluster in _BOXES:
        return _BOXES[cluster]
    b = _Box(11)
    assert abs(b.L / 2.7 - 8.09) < 0.02  # 8 cells per dimension at skin 0.2, 8 at 0.12, 7 at 0.3
    keep = np.array([1.0, 1.0, 0.5, 1 / 6, 1 / 12, 1 / 12, 1 / 6, 1 / 3])  # by cz: brick layers 0 .. 3
    b.thin(lambda c: keep[c[:, 2]])
    # an empty column of three cells in brick (1, 1, 0)
    b.set_count((5, 4, 0), (6, 7, 1), 0)
    # rows of exactly 32, 33 and 64 candidates: cells 1 .. 3 in x
    b.set_count((1, 1, 0), (4, 2, 1), 32)
    b.set_count((1, 2, 0), (4, 3, 1), 33)
    b.set_count((1, 1, 2), (4, 2, 3), 64)  # (in the half-density layer: the lists around it stay below the capacity)
    # a cell with more than 32 molecules in brick (1, 0, 0)
    b.set_count((6, 1, 0), (7, 2, 1), 33, dmin=0.62)
    # owned molecules of the four full-density bricks (edited in cells the rows above do not use): split tiles of 8 / 4 / 2 / 1 lanes
    b.set_count((0, 0, 0), (4, 4, 2), 516, (0, 3, 0), (4, 4, 2))
    b.set_count((4, 0, 0), (8, 4, 2), 524, (4, 3, 0), (8, 4, 2))
    b.set_count((0, 4, 0), (4, 8, 2), 536, (0, 4, 0), (4, 8, 2))
    b.set_count((4, 4, 0), (8, 8, 2), 548, (6, 4, 0), (8, 8, 2))
    if cluster:
        ctr = np.array([2.5, 2.5, 2.5]) * b.cl

        def ball():
            while True:
                p = b.rng.uniform(-2.0, 2.0, 3)
                if p @ p < 2.0 * 2.0:
                    return ctr + p
        b.add(85, ball, 0.62)
    else:
        for lo, hi, n in (((0, 0, 0), (4, 4, 2), 516), ((4, 0, 0), (8, 4, 2), 524), ((0, 4, 0), (4, 8, 2), 536), ((4, 4, 0), (8, 8, 2), 548),
                          ((1, 1, 0), (4, 2, 1), 32), ((1, 2, 0), (4, 3, 1), 33), ((1, 1, 2), (4, 2, 3), 64), ((5, 4, 0), (6, 7, 1), 0),
                          ((6, 1, 0), (7, 2, 1), 33)):
            assert int(b.inside(lo, hi).sum()) == n
        nn = _neighbours(b.r, b.L, 2.7)
        layer = b.cells()[:, 2] // 2
        assert nn[layer == 2].max() <= 14, nn[layer == 2].max()   # tiles of the minimum row count (16 entries = 4 words)
        assert nn[layer == 0].max() <= 90, nn[layer == 0].max()   # no list overflow (96 entries): every brick regular
    n = len(b.r)
    ids = np.arange(1, n + 1, dtype=np.uint64)
    v = np.random.default_rng(3).normal(0, 0.9, (n, 3))
    _BOXES[cluster] = (b.L, ids, b.r.copy(), v)
    return _BOXES[cluster]


_REF = {}


def _generic(cluster):
    """forces, U and virial of the generic kernel on the box: computed once"""
    if cluster not in _REF:
        L, ids, r, v = _corner_box(cluster)
        ref = _engine(L, ids, r, v, force_kernel=capi.FK_GENERIC)
        o0 = ref.run(1e-9, 1)
        _REF[cluster] = (_state(ref)[3].copy(), o0)
        ref.close()
    return _REF[cluster]


@pytest.mark.parametrize("skin,cluster", [(0.2, False), (0.12, False), (0.3, False), (0.2, True)])
def test_list_kernels_on_the_corner_box_one_evaluation(skin, cluster):
    """one list build + one evaluation from the lists against the generic kernel on the same state"""
    L, ids, r, v = _corner_box(cluster)
    F0, o0 = _generic(cluster)
    e = _engine(L, ids, r, v, skin=skin)
    out = e.run(1e-9, 1)
    assert e.get_option("verlet_lists") == 1 and e.get_option("verlet_builds") == 1
    irregular = e.get_option("verlet_irregular_bricks")
    if skin == 0.2:
        assert (irregular >= 1) if cluster else (irregular == 0), irregular  # every brick regular / the cluster's tile overflowed
    if skin == 0.3:
        assert irregular >= 1  # bricks with more than 640 owned molecules
    F = _state(e)[3]
    print("skin", skin, "cluster", cluster, "N", len(ids), "irregular bricks", irregular, "max|dF|/max|F|", rel_max(F, F0),
          "dU/U", abs(out["upot"] - o0["upot"]) / abs(o0["upot"]), "dW/W", abs(out["virial"] - o0["virial"]) / abs(o0["virial"]))
    assert rel_max(F, F0) < 1e-10
    assert abs(out["upot"] - o0["upot"]) <= 1e-10 * abs(o0["upot"]) and abs(out["virial"] - o0["virial"]) <= 1e-10 * abs(o0["virial"])
    e.close()


@pytest.mark.parametrize("skin,cluster", [(0.2, False), (0.3, False), (0.2, True)])
def test_list_kernels_on_the_corner_box_fused_steps(skin, cluster):
    """six steps of the production loop (fused force + integration pass, lists rebuilt by the displacement bound) stay on the
    trajectory of the per-step kernels"""
    L, ids, r, v = _corner_box(cluster)
    dt, steps = 0.0005, 6
    a = _engine(L, ids, r, v)
    oa = a.run(dt, steps)
    sa = _state(a)
    a.close()
    b = _engine(L, ids, r, v, skin=skin)
    ob = b.run(dt, steps)
    sb = _state(b)
    assert b.get_option("verlet_steps") == steps and b.get_option("verlet_builds") >= 1
    b.close()
    assert np.array_equal(sa[0], sb[0])
    dr = sa[1] - sb[1]
    dr -= L * np.round(dr / L)
    print("skin", skin, "cluster", cluster, "max|dr|/L", np.max(np.abs(dr)) / L, "dv", rel_max(sb[2], sa[2]), "dF", rel_max(sb[3], sa[3]))
    assert np.max(np.abs(dr)) < 1e-10 * L
    assert rel_max(sb[2], sa[2]) < 1e-10
    assert rel_max(sb[3], sa[3]) < 1e-10
    for k in ("upot", "virial", "summv2"):
        assert abs(oa[k] - ob[k]) <= 1e-10 * abs(oa[k]), k

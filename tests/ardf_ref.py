"""The angular-RDF yardstick of the tests: a brute-force numpy restatement of RDF::observeARDFMolecule (io/RDF.h:93-109) and
MoleculeInterface::orientationAngle (MoleculeInterface.h:167-190), O(N^2), f64, minimum image, the reference's expression order,
and the reader of tests/golden/ardf/.  Molecules are given in id order, so id_i < id_j is i < j."""
import functools
import os
import tarfile

import numpy as np

import rdf_ref
from golden_io import GOLDEN

COS_MARGIN = 1e-8  # no cos(phi) this close to an angular edge 1 - k * 2 / A
ARDF_GOLDEN = os.path.join(GOLDEN, "ardf")


def brute_force(r, q, cid, nC, L, rc, bins, dr, A, periodic=True, chunk=512):
    """dict(ardf uint64 [nC, nC, bins, A] (first index: component of the central molecule), margin = smallest distance of a pair
    distance to a bin edge, r_c or bins * dr (rdf_ref.EDGE_MARGIN applies), cos_margin = smallest distance of a cos(phi) to an
    angular edge).  q = None: no rotation, every molecule carries (1, 0, 0, 0)."""
    r, cid, L = np.asarray(r, dtype=np.float64), np.asarray(cid, dtype=np.int64), np.asarray(L, dtype=np.float64)
    N = len(r)
    q = np.tile([1., 0., 0., 0.], (N, 1)) if q is None else np.asarray(q, dtype=np.float64)
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    o = np.stack([2. * (x * z + w * y), 2. * (y * z - w * x), 1. - 2. * (x * x + y * y)], axis=1)
    s = np.sqrt(((0. + o[:, 0] * o[:, 0]) + o[:, 1] * o[:, 1]) + o[:, 2] * o[:, 2])
    rc2, maxd2, aw = rc * rc, dr * dr * float(bins) * float(bins), 2. / A
    reach = max(rc, bins * dr) + 2 * rdf_ref.EDGE_MARGIN
    ardf = np.zeros((nC, nC, bins * A), dtype=np.uint64)
    margin = cos_margin = np.inf
    for i0 in range(0, N, chunk):
        isel = np.arange(i0, min(N, i0 + chunk))
        d = r[None, :, :] - r[isel, None, :]  # r_j - r_i
        if periodic:
            d -= L * np.round(d / L)
        dd = d[:, :, 0] * d[:, :, 0] + d[:, :, 1] * d[:, :, 1] + d[:, :, 2] * d[:, :, 2]
        upper = np.arange(N)[None, :] > isel[:, None]
        margin = min(margin, rdf_ref._edge_margin(np.sqrt(dd[upper & (dd < reach * reach)]), rc, bins, dr))
        ii, jj = np.nonzero(upper & (dd < rc2) & ~(dd > maxd2))
        dv, sq = d[ii, jj], np.sqrt(dd[ii, jj])
        ii = isel[ii]
        b = np.floor(sq / dr)
        ok = b < bins
        ii, jj, dv, sq, b = ii[ok], jj[ok], dv[ok], sq[ok], b[ok].astype(np.int64)
        for c, k, e in ((ii, jj, dv), (jj, ii, -dv)):  # central molecule c, the other one k, e = r_k - r_c
            cos = ((0. + o[c, 0] * e[:, 0] / s[c] / sq) + o[c, 1] * e[:, 1] / s[c] / sq) + o[c, 2] * e[:, 2] / s[c] / sq
            t = (-cos + 1.) / aw
            cos_margin = min(cos_margin, float(np.min(np.abs(t - np.round(t)), initial=np.inf) * aw))
            flat = b * A + np.floor(t).astype(np.int64)  # signed: a = -1 and a = A land in the neighbouring distance row
            keep = (flat >= 0) & (flat < bins * A)
            np.add.at(ardf, (cid[c][keep], cid[k][keep], flat[keep]), 1)
    return dict(ardf=ardf.reshape(nC, nC, bins, A), margin=float(margin), cos_margin=float(cos_margin))


def usable(want):  # the condition on a state: device and restatement may differ in the last bit of d across a periodic face
    return want["margin"] >= rdf_ref.EDGE_MARGIN and want["cos_margin"] >= COS_MARGIN


def golden_manifest():  # tests/golden/ardf/MANIFEST_ardf.txt
    with open(os.path.join(ARDF_GOLDEN, "MANIFEST_ardf.txt")) as fh:
        case, A, step = [ln for ln in fh if ln.strip() and not ln.startswith("#")][0].split()
    return dict(case=case, angularbins=int(A), step=int(step))


@functools.lru_cache(maxsize=None)
def golden_text(i, j):  # the reference's .ardf file of the ordered component pair (i, j)
    g = golden_manifest()
    with tarfile.open(os.path.join(ARDF_GOLDEN, g["case"] + ".tar.gz"), "r:gz") as tf:
        return tf.extractfile("rdf_%d-%d.%09d.ardf" % (i, j, g["step"])).read().decode()


def golden_counts(i, j):
    """its integer `counter` column (column 3): uint64 [bins * A]"""
    return np.array([int(ln.split()[2]) for ln in golden_text(i, j).split("\n") if ln and not ln.startswith("#")], dtype=np.uint64)

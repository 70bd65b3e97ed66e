"""The spatial-profile yardstick of the tests: a numpy restatement of the reference's sampling rules
(plugins/SpatialProfile.cpp:146-222, 233-283, 339-410 and the record() bodies of plugins/profiles/*.h), the reader of the
reference's profile files, and the golden cases of tests/golden/profile/.

Per-molecule terms are formed in float64 with the operations and their order as the device forms them (no contraction on either
side); the sums over a bin are taken in np.longdouble.  Next to every f64 table the restatement returns the sum of the absolute
terms (`abs_*`): the scale of the summation-order bound of the GPU tests.  It is pinned to the real reference by
tests/test_profile_cpu.py and then serves the GPU tests on states downloaded from the device."""
import functools
import math
import os
import re

import numpy as np

from golden_io import GOLDEN, input_path

PROFILE_GOLDEN = os.path.join(GOLDEN, "profile")
# a state is usable only if no bin coordinate (x inv, R^2 inv, phi inv: in units of the bin) lies this close to a bin edge
EDGE_MARGIN = 1e-8
CARTESIAN, CYLINDER = 0, 1
VELOCITY, VELOCITY3D, TEMPERATURE, VIRIAL = 1, 2, 4, 8
ALL = VELOCITY | VELOCITY3D | TEMPERATURE | VIRIAL
F64_KEYS = ("ekin", "vabs", "v3", "vi3")


def sampling_info(mode, units, L):
    """SpatialProfile::init (SpatialProfile.cpp:146-212): inverse units, centre, segment volume, number of bins."""
    L = np.asarray(L, dtype=np.float64)
    u = [int(x) for x in units]
    if mode == CYLINDER:
        minXZ = min(L[0], L[2])
        R2max = .24 * minXZ * minXZ
        inv = np.array([u[0] / R2max, u[1] / L[1], u[2] / (2 * math.pi)])
        vol = math.pi / (inv[0] * inv[1] * u[2])
    else:
        inv = np.array([u[d] / L[d] for d in range(3)])
        vol = L[0] * L[1] * L[2] / (u[0] * u[1] * u[2])
    return dict(mode=mode, units=u, inv=inv, centre=np.array([0.5 * L[0], 0.0, 0.5 * L[2]]), segment_volume=float(vol),
                bins=u[0] * u[1] * u[2], L=L)


def wrap(r, L):
    """global coordinates wrapped into [0, L) by the rule of ls1hip_download_state (DomainDecompBase.cpp:206-219)"""
    r = np.array(r, dtype=np.float64)
    L = np.asarray(L, dtype=np.float64)
    for k in range(3):
        x = r[:, k]
        lo, hi = x < 0.0, x >= L[k]
        x[lo] += L[k]
        x[lo & (x >= L[k])] = np.nextafter(L[k], 0.0)
        x[hi] -= L[k]
        x[hi & (x <= 0.0)] = 0.0
    return r


def bin_index(r, info):
    """uID per molecule (-1: outside the cylinder) and the smallest distance of a bin coordinate to a bin edge, in units of the
    bin (SpatialProfile::getCartesianUID / getCylUID)."""
    r = wrap(r, info["L"])
    u, inv = info["units"], info["inv"]
    if info["mode"] == CARTESIAN:
        c = [r[:, d] * inv[d] for d in range(3)]
        idx = [np.minimum(np.floor(c[d]).astype(np.int64), u[d] - 1) for d in range(3)]
        uid = idx[0] * u[1] * u[2] + idx[1] * u[2] + idx[2]
        keep = np.ones(len(r), dtype=bool)
    else:
        xc, yc, zc = r[:, 0] - info["centre"][0], r[:, 1] - info["centre"][1], r[:, 2] - info["centre"][2]
        R2 = xc * xc + zc * zc
        phi = np.arctan2(zc, xc)
        phi = np.where(phi < 0.0, phi + 2.0 * math.pi, phi)
        c = [R2 * inv[0], yc * inv[1], phi * inv[2]]
        rUn = np.floor(c[0]).astype(np.int64)
        keep = rUn < u[0]
        hUn = np.minimum(np.floor(c[1]).astype(np.int64), u[1] - 1)
        pUn = np.minimum(np.floor(c[2]).astype(np.int64), u[2] - 1)
        uid = hUn * u[0] * u[2] + rUn * u[2] + pUn
    margin = np.inf
    for d in range(3):
        x = c[d]
        if info["mode"] == CYLINDER and d == 0:
            x = x[x < u[0] + 0.5]  # beyond the cylinder only the edge at nR matters
        if x.size:
            margin = min(margin, float(np.min(np.abs(x - np.round(x)))))
    return np.where(keep, uid, -1), margin


def rotate_inv(q, D):
    """R(q)^T D with the expressions of pairphys.hpp (rot_of, rotate_inv: Quaternion.cpp:45-81), q as stored"""
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    ww, xx, yy, zz = w * w, x * x, y * y, z * z
    wx, wy, wz, xy, xz, yz = w * x, w * y, w * z, x * y, x * z, y * z
    m = [ww + xx - yy - zz, 2. * (xy - wz), 2. * (wy + xz), 2. * (wz + xy), ww - xx + yy - zz, 2. * (yz - wx), 2. * (xz - wy),
         2. * (wx + yz), ww - xx - yy + zz]
    dx, dy, dz = D[:, 0], D[:, 1], D[:, 2]
    return np.stack([m[0] * dx + m[3] * dy + m[6] * dz, m[1] * dx + m[4] * dy + m[7] * dz, m[2] * dx + m[5] * dy + m[8] * dz], axis=1)


def kinetic_terms(v, q, D, cid, flat):
    """m v^2 and I w^2 per molecule (Molecule::calculate_mv2_Iw2; the device's kinetic_terms, leapfrog_body.hpp)"""
    mass = np.asarray(flat["mass"], dtype=np.float64)[cid]
    I = np.asarray(flat["I"], dtype=np.float64).reshape(-1, 3)
    invI = np.where(I != 0.0, 1.0 / np.where(I != 0.0, I, 1.0), 0.0)
    mv2 = mass * (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2])
    w = rotate_inv(q, D)
    w = w * invI[cid]
    Ic = I[cid]
    Iw2 = Ic[:, 0] * w[:, 0] * w[:, 0] + Ic[:, 1] * w[:, 1] * w[:, 1] + Ic[:, 2] * w[:, 2] * w[:, 2]
    return mv2, Iw2


def _bin_sum(uid, term, bins):
    """longdouble sum of `term` per bin and the sum of |term| per bin"""
    s = np.zeros((bins,) + term.shape[1:], dtype=np.longdouble)
    a = np.zeros_like(s)
    t = term.astype(np.longdouble)
    np.add.at(s, uid, t)
    np.add.at(a, uid, np.abs(t))
    return s, a


def tables(r, v, q, D, cid, comps, L, mode, units, quantities=ALL, component=-1, Vi=None):
    """Tables of ONE configuration: n, dof (uint64), ekin, vabs, v3, vi3 (longdouble sums rounded to float64 in `ekin` ..., kept
    in `ld_*`), abs_* = sum of |term|, margin, samples = 1."""
    info = sampling_info(mode, units, L)
    cid = np.asarray(cid, dtype=np.int64)
    v = np.asarray(v, dtype=np.float64)
    uid, margin = bin_index(r, info)
    sel = uid >= 0
    if component >= 0:
        sel &= cid == component
    bins = info["bins"]
    flat = comps.flat()
    u = uid[sel]
    out = dict(info=info, margin=margin, samples=1, quantities=quantities,
               n=np.bincount(u, minlength=bins).astype(np.uint64))
    if quantities & TEMPERATURE:
        rd = np.asarray(flat["rot_dof"], dtype=np.int64)
        out["dof"] = np.bincount(u, weights=(3 + rd[cid[sel]]).astype(np.float64), minlength=bins).astype(np.uint64)
        mv2, Iw2 = kinetic_terms(v[sel], np.asarray(q, dtype=np.float64)[sel], np.asarray(D, dtype=np.float64)[sel], cid[sel], flat)
        terms = {"ekin": mv2 + Iw2}
    else:
        terms = {}
    if quantities & VELOCITY:
        vs = v[sel]
        a = vs[:, 0] * vs[:, 0]
        a = a + vs[:, 1] * vs[:, 1]
        a = a + vs[:, 2] * vs[:, 2]
        terms["vabs"] = np.sqrt(a)
    if quantities & VELOCITY3D:
        terms["v3"] = v[sel]
    if quantities & VIRIAL:
        terms["vi3"] = np.asarray(Vi, dtype=np.float64)[sel]
    for k, t in terms.items():
        s, a = _bin_sum(u, t, bins)
        out["ld_" + k], out["abs_" + k], out[k] = s, a, s.astype(np.float64)
    return out


def add_tables(a, b):
    out = dict(a)
    out["samples"] = a["samples"] + b["samples"]
    out["margin"] = min(a["margin"], b["margin"])
    for k in ("n", "dof"):
        if k in a:
            out[k] = a[k] + b[k]
    for k in F64_KEYS:
        if k in a:
            out["ld_" + k] = a["ld_" + k] + b["ld_" + k]
            out["abs_" + k] = a["abs_" + k] + b["abs_" + k]
            out[k] = out["ld_" + k].astype(np.float64)
    return out


def assert_tables(got, want, what=""):
    """u64 tables equal; every f64 bin within (n_bin + 8) 2^-53 sum|term| of the longdouble sum (summation order: n_bin - 1
    roundings of at most 2^-53 of the partial sums, each below sum|term|; plus a few ulp per term for contraction and sqrt)."""
    assert np.array_equal(got["n"], want["n"]), (what, "n", int(np.abs(got["n"].astype(np.int64) - want["n"].astype(np.int64)).sum()))
    assert got["samples"] == want["samples"], (what, got["samples"], want["samples"])
    if "dof" in want:
        assert np.array_equal(got["dof"], want["dof"]), (what, "dof")
    worst = {}
    for k in F64_KEYS:
        if k not in want:
            assert k not in got, (what, k)
            continue
        n = want["n"].astype(np.longdouble)
        if want[k].ndim == 2:
            n = n[:, None]
        bound = (n + 8) * np.longdouble(2.0) ** -53 * want["abs_" + k]
        err = np.abs(got[k].astype(np.longdouble) - want["ld_" + k])
        worst[k] = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1), np.where(err > 0, np.inf, 0))))
        print(f"profile {what} {k}: max error / bound = {worst[k]:.3f}")
        assert np.all(err <= bound), (what, k, worst[k])
    return worst


# ---- the reference's files ----------------------------------------------------------------------------------------------------------
_NUM = re.compile(r"^[+-]?(\d+\.?\d*|\.\d+)([eE][+-]?\d+)?$|^-?nan$|^-?inf$")


def is_number(tok):
    return bool(_NUM.match(tok))


def same_number(a: str, b: str) -> bool:
    """two printed numbers agree within one unit of the sixth significant digit (what precision(6) prints)"""
    x, y = float(a), float(b)
    if x == y or (math.isnan(x) and math.isnan(y)):
        return True
    top = max(abs(x), abs(y))
    unit = 10.0 ** (math.floor(math.log10(top)) - 5)
    return abs(x - y) <= unit * (1 + 1e-9)


def same_text(got: str, want: str, what=""):
    """token by token (tabs and blanks are separators; line structure kept): numbers by same_number, everything else identical"""
    gl, wl = got.split("\n"), want.split("\n")
    assert len(gl) == len(wl), (what, len(gl), len(wl))
    for ln, (g, w) in enumerate(zip(gl, wl)):
        gt, wt = g.split(), w.split()
        assert len(gt) == len(wt), (what, ln, g[:160], w[:160])
        for a, b in zip(gt, wt):
            if is_number(a) and is_number(b):
                assert same_number(a, b), (what, ln, a, b)
            else:
                assert a == b, (what, ln, a, b)


def cases():
    """Golden cases of MANIFEST_profile.txt: name -> dict(input, rc, dt, temperature, steps, instances = [dict(prefix, mode, units,
    component (0-based, -1 = all))])."""
    out = {}
    with open(os.path.join(PROFILE_GOLDEN, "MANIFEST_profile.txt")) as fh:
        for ln in fh:
            if ln.startswith("#") or not ln.strip():
                continue
            t = ln.split()
            name, inp, rc, dt, temp, steps = t[0], t[1], float(t[2]), float(t[3]), float(t[4]), int(t[5])
            inst = []
            for spec in t[6:]:
                prefix, mode, ux, uy, uz, comp = spec.split(":")
                inst.append(dict(prefix=prefix, mode=CYLINDER if mode == "cylinder" else CARTESIAN, units=(int(ux), int(uy), int(uz)),
                                 component=-1 if comp == "all" else int(comp) - 1))
            out[name] = dict(name=name, input=inp, rc=rc, dt=dt, temperature=temp, steps=steps, instances=inst)
    return out


@functools.lru_cache(maxsize=None)
def _golden_archive(case):
    import tarfile
    with tarfile.open(os.path.join(PROFILE_GOLDEN, case + ".tar.gz"), "r:gz") as tf:
        return {m.name: tf.extractfile(m).read().decode() for m in tf.getmembers() if m.isfile()}


SUFFIXES = (".NDpr", ".Temppr", ".V3Dpr", ".VAbspr", "_1D-Y.Vipr")


def golden_text(case, prefix, step, suffix):
    return _golden_archive(case)["%s_%d%s" % (prefix, step, suffix)]


def read_matrix(text, info, per_entry=1):
    """The data block of a file of ProfileBase::writeMatrix -> float array [bins(, per_entry)] indexed by uID."""
    lines = [ln for ln in text.split("\n") if ln.strip()]
    k = next(i for i, ln in enumerate(lines) if ln.startswith("0 \t"))
    rows = lines[k + 1:]
    u = info["units"]
    out = np.zeros((info["bins"], per_entry))
    assert len(rows) == u[1]
    for y, ln in enumerate(rows):
        vals = [float(t) for t in ln.split()][1:]
        assert len(vals) == u[0] * u[2] * per_entry, (len(vals), u)
        at = 0
        if info["mode"] == CYLINDER:
            for phi in range(u[2]):
                for rr in range(u[0]):
                    uid = y * u[0] * u[2] + rr * u[2] + phi
                    out[uid] = vals[at:at + per_entry]
                    at += per_entry
        else:
            for z in range(u[2]):
                for x in range(u[0]):
                    uid = x * u[1] * u[2] + y * u[2] + z
                    out[uid] = vals[at:at + per_entry]
                    at += per_entry
    return out[:, 0] if per_entry == 1 else out


@functools.lru_cache(maxsize=None)
def case_states(name):
    """The fixture of a golden case advanced with the CPU oracle under the driver's global velocity-scaling thermostat: per step
    1..n dict(r, v, q, D, Vi, temperature): the state SpatialProfile::endStep sees (full-step velocities AFTER the scaling) and
    Domain::getCurrentTemperature(0) of that step (from the kinetic sums BEFORE the scaling, Domain.cpp:204-240).  Computed once
    per process and shared; callers do not modify it."""
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
    rot_dof = orc.rot_dof(s["cid"])
    for _ in range(c["steps"]):
        out = orc.step(c["dt"], s["cid"], r, v, q, D, F, M, ps.length, True, target_T=c["temperature"])
        T = (out["summv2"] + out["sumIw2"]) / (3.0 * len(r) + rot_dof)
        states.append(dict(r=r.copy(), v=v.copy(), q=q.copy(), D=D.copy(), Vi=out["Vi"].copy(), temperature=float(T)))
    return dict(case=c, ps=ps, ids=s["ids"], cid=s["cid"], states=states)


@functools.lru_cache(maxsize=None)
def case_tables(name, instance, first, last):
    """tables of one plugin instance of a golden case accumulated over steps first..last (shared, unchanged by the callers)"""
    cs = case_states(name)
    ins = cs["case"]["instances"][instance]
    total = None
    for step in range(first, last + 1):
        st = cs["states"][step - 1]
        t = tables(st["r"], st["v"], st["q"], st["D"], cs["cid"], cs["ps"].components, cs["ps"].length, ins["mode"], ins["units"], ALL,
                   ins["component"], Vi=st["Vi"])
        total = t if total is None else add_tables(total, t)
    return total

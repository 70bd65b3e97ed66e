"""Plain numpy FP64 restatement of the reference's WallPotential::calcTSLJ_9_3 / calcTSLJ_10_4 (plugins/WallPotential.cpp:193-341) and
Mirror::VelocityChange (plugins/Mirror.cpp:421-477, MT_REFLECT and MT_FORCE_CONSTANT): per-site loops vectorised over the molecules.  The
checker of tests/test_gpu_wall.py and tests/test_wall_cpu.py.  One deviation, shared with the device: 2./5. in the 10-4-3 energy."""
import functools
import gzip
import importlib
import io
import os
import tarfile

import numpy as np

from golden_io import GOLDEN, input_path, sorted_phase_space
from planar_ref import rotate


def cases():
    """{name: fields} of tests/golden/wall/MANIFEST_wall.txt"""
    return {ln.split()[0]: ln.split() for ln in open(os.path.join(GOLDEN, "wall", "MANIFEST_wall.txt")) if not ln.startswith("#")}


@functools.lru_cache(maxsize=None)
def golden(name):
    """a case of tests/golden/wall: the film input, the run's settings, the plugins' arguments (wall.json) and the driver's files"""
    import json
    _, fname, rc, dt, temp, steps = cases()[name]
    ps = importlib.import_module("ls1-mardyn_amd.inp").read_inp(input_path(fname))
    with tarfile.open(fileobj=io.BytesIO(gzip.open(os.path.join(GOLDEN, "wall", name + ".tar.gz")).read())) as tf:
        files = {m.name: tf.extractfile(m).read().decode() for m in tf.getmembers()}
    plug = json.loads(files["wall.json"])
    return dict(ps=ps, s=sorted_phase_space(ps), rc=float(rc), dt=float(dt), temp=float(temp), steps=int(steps), files=files,
                wall=plug["wall"], mirrors=plug["mirrors"])


def wall_params(w, components):
    """per component: consider, eps_wi, sig_wi, ushift (WallPotential.cpp:105-187) from a dict of the XML's names; components {cid: (xi, eta)}"""
    cs = components.components
    given = {int(k): v for k, v in (w.get("components") or {}).items()}
    out = []
    for i, c in enumerate(cs):
        consider = not given or (i + 1) in given
        xi, eta = given.get(i + 1, (0.0, 0.0))
        if not consider:
            out.append(None)
            continue
        eps, sig = c.lj[0][4], c.lj[0][5]
        e, s, y = xi * np.sqrt(w["epsilon"] * eps), 0.5 * eta * (w["sigma"] + sig), w["ycut"]
        if w["potential"] == 93:
            sh = 4.0 / 3.0 * np.pi * w["density"] * e * s ** 3 * (s ** 9 / 15.0 / y ** 9 - s ** 3 / 2.0 / y ** 3)
        else:
            d = w["delta"]
            sh = 2 * np.pi * e * w["density"] * s * s * d * ((2. / 5.) * s ** 10 / y ** 10 - s ** 4 / y ** 4 - s ** 4 / (3 * d * (y + 0.61 * d) ** 3))
        out.append((e, s, sh))
    return out


def apply(components, length, cid, r, v, q, wall=None, mirrors=()):
    """One siteWiseForces + afterForces on molecules inside the box.  wall: dict of the XML's names or None; mirrors: dicts with type,
    direction, coord, cid, forceConstant.  -> dF, dM [n, 3] (lab frame), vy [n] after the mirrors, upot [ncomp], touched [n] (a site
    inside ycut or the centre inside a mirror's region), margin (smallest |ryRel| / sig_wi over the considered sites)"""
    n, cs = len(cid), components.components
    dF, dM, upot = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros(len(cs))
    touched, margin = np.zeros(n, dtype=bool), np.inf
    y = r[:, 1]
    if wall is not None and (wall["potential"] == 104 or 0.0 < wall["ycut"] + wall["yoff"]):  # (:197: the 9-3 form's outer test)
        par, yoff, wh, yc = wall_params(wall, components), wall["yoff"], 0.5 * wall.get("width", 0.0), wall["ycut"]
        for c, comp in enumerate(cs):
            m = np.flatnonzero(cid == c)
            if par[c] is None or len(m) == 0:
                continue
            e, s, sh = par[c]
            for site in comp.lj:
                d = rotate(q[m], site[:3]) if np.any(site[:3] != 0) else np.zeros((len(m), 3))
                ry = y[m] + d[:, 1]
                rel = np.where(ry > yoff, ry - (yoff + wh), ry - (yoff - wh))
                ya = np.abs(rel)
                margin = min(margin, (ya / s).min()) if s > 0 else margin
                k = ya < yc
                ya, dk, mk = ya[k], d[k], m[k]
                if wall["potential"] == 93:
                    pre = 4.0 * np.pi * wall["density"] * e * s ** 3
                    f = pre * (s ** 9 / 5.0 / ya ** 9 - s ** 3 / 2.0 / ya ** 3) / ya
                    u = pre * (s ** 9 / 45.0 / ya ** 9 - s ** 3 / 6.0 / ya ** 3) - sh
                else:
                    dl = wall["delta"]
                    pre, br = 2 * np.pi * e * wall["density"] * s * s * dl, ya + 0.61 * dl
                    t3 = s ** 4 / (3 * dl * br ** 3)
                    u = pre * ((2. / 5.) * s ** 10 / ya ** 10 - s ** 4 / ya ** 4 - t3) - sh
                    f = pre * (4 * s ** 10 / ya ** 11 - 4 * s ** 4 / ya ** 5 - t3 * 3 / br)
                f = np.where(rel[k] < 0, -f, f)
                np.add.at(dF[:, 1], mk, f)
                np.add.at(dM[:, 0], mk, -dk[:, 2] * f)  # d x (0, f, 0)
                np.add.at(dM[:, 2], mk, dk[:, 0] * f)
                upot[c] += u.sum()
                touched[mk] = True
    vy = v[:, 1].copy()
    for mr in mirrors:
        if not mr.get("type"):
            continue
        k = (y >= mr["coord"]) if mr["direction"] == 1 else (y < mr["coord"])  # inBox: r >= low and r < high
        if mr.get("cid", 0):
            k &= cid + 1 == mr["cid"]
        touched |= k
        if mr["type"] == 1:
            flip = k & ((vy > 0) if mr["direction"] == 1 else (vy < 0))
            vy[flip] = -vy[flip]
        else:
            dF[k, 1] += mr.get("forceConstant", 100.0) * (mr["coord"] - y[k])
    return dict(dF=dF, dM=dM, vy=vy, upot=upot, touched=touched, margin=margin)

"""mirror.WallPotential / mirror.Mirror without a device: what they hand to ls1hip_wall_config from the XML's parameters, against the
per-component parameters tests/wall_ref.py derives from the same XML, and the refused mirror types."""
import numpy as np
import pytest

import wall_ref
from conftest import load_pkg

inp = load_pkg("inp")
mirror = load_pkg("mirror")

COMPS = inp.ComponentSet([inp.make_component(lj=[(0, 0, 0, 1.0, 1.3, 1.1, 2.5, 0)]),
                          inp.make_component(lj=[(0, 0, -0.1, 0.5, 0.6, 0.9, 2.5, 0), (0, 0, 0.1, 0.5, 0.7, 0.8, 2.5, 0)])], np.ones((1, 2)), 1e10)
WALL = dict(potential=104, density=1.07, sigma=1.2, epsilon=0.8, yoff=4.0, ycut=2.5, width=0.6, delta=0.775)


@pytest.mark.parametrize("components", [{}, {2: (0.9, 1.1)}, {"1": (1.0, 1.0), "2": (0.5, 1.2)}])
def test_parameter_derivation(components):
    """consider / xi / eta per component as readXML leaves them (no <component>: every component, with xi = eta = 0), checked through
    eps_wi = xi sqrt(eps_w eps_i) and sig_wi = eta (sig_w + sig_i) / 2 of LJ centre 0 (eps 1.3 / 0.6, sigma 1.1 / 0.9)"""
    consider, xi, eta = mirror.WallPotential(components=components, **WALL).arrays(2)
    want = wall_ref.wall_params(dict(WALL, components=components), COMPS)
    assert list(consider) == [int(p is not None) for p in want]
    for i, (eps_i, sig_i) in enumerate([(1.3, 1.1), (0.6, 0.9)]):
        if want[i] is not None:
            assert (xi[i] * np.sqrt(0.8 * eps_i), 0.5 * eta[i] * (1.2 + sig_i)) == want[i][:2]
    with pytest.raises(ValueError):
        mirror.WallPotential(components={3: (1.0, 1.0)}, **WALL).arrays(2)


@pytest.mark.parametrize("kind", [3, 4, 5, 6, "refID"])
def test_refused_mirrors_raise(kind):
    with pytest.raises(NotImplementedError):
        mirror.Mirror(type=1, refID=2) if kind == "refID" else mirror.Mirror(type=kind)
    assert mirror.Mirror(type=2, dir="o-|", coord=3.0, cid=1).direction == 1 and mirror.Mirror(type=1, direction=1, dir="|-o").direction == 0

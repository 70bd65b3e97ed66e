"""mirror.Widom's arithmetic and writer on plain arrays (no device)."""
import math

import numpy as np

from conftest import load_pkg

mirror = load_pkg("mirror")


def test_mu_res_and_table():
    T, Ly = 0.8, 12.0
    sum_w = np.array([2.0, 0.0, 0.0, 30.0])
    n = np.array([4, 0, 5, 10], dtype=np.uint64)
    tot, per = mirror.Widom.mu_res_of(sum_w, n, T)
    assert per[0] == -T * math.log(0.5) and math.isnan(per[1]) and per[2] == math.inf and per[3] == -T * math.log(3.0)
    assert tot == -T * math.log(32.0 / 19.0)  # sums and counts are additive over slabs (and ranks), the logarithm is not
    rows = mirror.Widom.render(sum_w, n, T, Ly).splitlines()
    assert rows[0].split() == ["#", "slab", "y_mid", "n", "<w>", "mu_res"] and len(rows) == 6
    k, y, cnt, w, mu = rows[4].split()
    assert (int(k), float(y), int(cnt)) == (3, 10.5, 10) and float(w) == 3.0 and abs(float(mu) - per[3]) < 1e-12
    assert rows[2].split()[3:] == ["nan", "nan"] and rows[5].split()[:3] == ["#", "total", "19"]
    assert math.isnan(mirror.Widom.mu_res_of(np.zeros(2), np.zeros(2), T)[0])

"""tests/tempcontrol_ref.py proven against files the unmodified reference driver wrote (tests/golden/tempcontrol/, made by
tests/golden/make_tempcontrol_golden.py): stepped on the CPU by the oracle's pieces it reproduces the final checkpoint to 1e-9 (the
project's trajectory tolerance) and every value of the beta_log files to 1e-10."""
import numpy as np
import pytest

import planar_ref
import tempcontrol_ref


@pytest.mark.parametrize("name", sorted(tempcontrol_ref.cases()))
def test_reference_reproduces_the_driver(name):
    c = tempcontrol_ref.golden(name)
    L = c["ps"].length
    got = tempcontrol_ref.run(c, c["control"], c["regions"], c["steps"])
    want = planar_ref.read_restart(c["files"]["step%d.restart.dat" % c["steps"]].decode())
    dr = got["r"] - want["r"]
    dr -= L * np.rint(dr / L)
    assert np.abs(dr).max() <= 1e-9 * L.max()
    for k in ("v", "q", "D"):
        if np.abs(want[k]).max() > 0:
            assert np.abs(got[k] - want[k]).max() <= 1e-9 * np.abs(want[k]).max(), k
    for k, reg in enumerate(c["regions"]):
        freq, rec = tempcontrol_ref.read_beta_log(c["files"]["beta_log_reg%d.dat" % (k + 1)])
        assert freq == reg["writefreq"] and rec.shape == got["beta_log"][k].shape and len(rec) > 0
        assert np.abs(rec / got["beta_log"][k] - 1).max() <= 1e-10
    if c["control"][1] == 2:
        # case b: region 1 wrote once (step 4: two configurations in one record); control step 6 lies outside [start, stop) and scaled
        # with the factors of step 4 — a run that measured there, or did not scale there, misses the checkpoint above
        assert len(got["beta_log"][0]) == 1 and got["tc"].regions[0]["configs"] == 0 and c["steps"] > 6

"""The whole-wave step body of k_rollout_geometric on the host (the kernels of csrc compiled as host C++ against the SIMT stand-in of
tests/emul/simt, one thread per lane, under AddressSanitizer + UBSan): the lanes past the last drone load drone n - 1's state and
parameters (a clamped index), run the whole step and store nothing.  For ragged shards -- n = 1, 63, 64, 65, 259 and 256 + 64: a
partial last wave, fully invalid waves, exact multiples of the wave and of the workgroup -- the valid drones' rows and state are
bit-equal to the PREDICATED step body's: k_step_geometric, one launch per control step, whose lanes past the last drone do nothing
at all (launch form 1 of the library), and to the same drones flown in a batch that has no invalid lane.  CPU only."""
import numpy as np
import pytest

from tests import helpers as H
from tests.emul.simt import simt

pytestmark = pytest.mark.skipif(not simt.available(), reason="no clang++ for the host emulation")

STEPS = 9                # launches of 7 + 2 steps in the emulation's rollout forms
N_ALL = 512
CASES = [1, 63, 64, 65, 259, 256 + 64]


@pytest.fixture(scope="module")
def flown():
    """512 drones (two full workgroups: no invalid lane) through the predicated per-step kernel (form 0) and the whole-rollout kernel
    (form 4: rows rewritten in place; form 1: the log ring), once."""
    simt.build()
    from oracle import c_oracle as CO
    xyz, rpy, P = H.c2_setup(N_ALL, 1, seed=4, phase="c3", yaw_rate=0.0)
    P[::3, :, 5] = 0.3
    P[..., 6] = 0.37 * np.arange(N_ALL)[:, None]
    rpy = np.random.default_rng(12).uniform(-0.2, 0.2, size=rpy.shape)
    av = CO.AviaryC(xyz, rpy)
    av.step(np.zeros((N_ALL, 4)))
    state13 = av.st.reshape(N_ALL, 1, 20)[..., :13].copy()
    ref = {form: simt.headline("float32", form, 0.0, P, state13, STEPS)[:2] for form in (0, 1, 4)}
    return P, state13, ref


@pytest.mark.parametrize("n", CASES)
def test_clamped_step_body_equals_the_predicated_one(flown, n):
    P, state13, ref = flown
    for form in (4, 1):
        obs, st, _, err = simt.headline("float32", form, 0.0, P[:n], state13[:n], STEPS)
        assert "ERROR" not in err and "runtime error" not in err, err[-3000:]
        assert np.isfinite(obs).all() and (obs[..., 16:] > 0).all()
        # the same drones where no lane is invalid
        assert np.array_equal(obs, ref[form][0][:n]) and np.array_equal(st, ref[form][1][:n]), (n, form)
        # the predicated step body
        assert np.array_equal(obs, ref[0][0][:n]) and np.array_equal(st, ref[0][1][:n]), (n, form)

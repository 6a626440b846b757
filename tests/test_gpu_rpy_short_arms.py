"""The wave-uniform short arms of the Euler-angle block on the device (csrc/mds_math.hpp: rpy_from_rot, m_atan2, m_asin).

A wave takes a short arm only when every one of its lanes passes the arm's test, so the company a drone keeps in its wave decides
which instructions compute its row -- and must not decide a single bit of it.  Two waves of 64 drones fly the same 64 flights, fp32;
in the second wave one lane starts out of the short arms' range (yaw 2.5 rad: the yaw atan2 leaves its octant; roll 1.2 rad: the roll
atan2 does; pitch 0.7 rad: sin pitch > 0.5, the asin's range arm), which sends its whole wave through the general arms.  The other
63 drones' rows at every step and their final state must be bit for bit those of the first wave, through the whole-rollout kernel
(launch form 2: its log form, 20 steps in one launch; and its rows-in-place form, the headline, one step per launch so that every
step's rows can be read back) and through one launch per step (form 1, k_step_geometric).

And the fp32 m_asin, ocml's asinf restated so that its polynomial can be reached without the range arms, against the device
library's asinf itself: every 64th fp32 of [-1, 1], bit for bit, in ascending order (whole waves below 0.5 take the short arm) and
interleaved (every wave holds arguments on both sides of 0.5: the general arm at every argument)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import helpers as H
from tests.test_gpu_parity import make_env, mds  # noqa: F401  (mds: the module's fixture)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E, D, T = 16, 8, 20                  # 128 drones = two waves of 64; envs 8..15 repeat envs 0..7
ODD = 64 + 21                        # the lane of the second wave that starts out of range
CASES = {"yaw": (2, 2.5), "roll": (0, 1.2), "pitch": (1, 0.7)}


def two_waves(axis, angle):
    xyz, rpy, P = H.c2_setup(E, D, phase="c3")
    xyz[E // 2:], P[E // 2:] = xyz[:E // 2], P[:E // 2]
    rpy.reshape(-1, 3)[ODD, axis] = angle
    return xyz, rpy, P


def rows_every_step(mds, form, xyz, rpy, P):
    """[T, 128, 20] rows and the final [128, 13] state; form "log" / "in_place" (both launch form 2) or "per_step" (form 1)"""
    torch = mds.torch
    env = make_env(mds, E, D, xyz, rpy, "float32")
    env.set_trajectories(P)
    env.step(torch.zeros((E, D, 4), dtype=env.dtype, device=env.device))
    dt = env.CTRL_TIMESTEP
    if form == "log":
        env.set_rollout_form(2, T)
        _, log = env.rollout_geometric_fused(0.0, T, log=True)
        rows = log.cpu().numpy()
    elif form == "in_place":
        env.set_rollout_form(2, 1)
        rows = []
        for k in range(T):           # one step per call: each is one launch of the kernel, and every step's rows are read back
            rows.append(env.rollout_geometric(k * dt, 1, obs_every_step=True).cpu().numpy().copy())
            assert env.last_rollout_form() == 2
        rows = np.stack(rows)
    else:
        rows = np.stack([env.step_geometric(k * dt).cpu().numpy().copy() for k in range(T)])
    state = env.get_state().reshape(-1, 13)
    env.close()
    return rows.reshape(T, E * D, 20), state


# every case through both shapes of the whole-rollout kernel; form 1 runs the same functions per call: once
@pytest.mark.parametrize("case,form", [(c, f) for f in ("log", "in_place") for c in sorted(CASES)] + [("yaw", "per_step")])
def test_a_lanes_bits_do_not_depend_on_the_arm_its_wave_takes(mds, case, form):
    axis, angle = CASES[case]
    rows, state = rows_every_step(mds, form, *two_waves(axis, angle))
    assert rows.dtype == np.float32 and np.isfinite(rows).all()
    first, second = rows[:, :64], rows[:, 64:]
    shared = np.arange(64) != ODD - 64
    # the first wave is in the short arms' range at every step (first octants, |sin pitch| < 0.5), the odd lane starts outside it
    assert np.abs(first[:, :, [7, 9]]).max() < 0.78 and np.abs(first[:, :, 8]).max() < 0.52
    assert abs(second[0, ODD - 64, 7 + axis] - angle) < 0.1
    assert (second[:, ODD - 64] != first[:, ODD - 64]).any()
    np.testing.assert_array_equal(second[:, shared].view(np.uint32), first[:, shared].view(np.uint32))
    np.testing.assert_array_equal(state[64:][shared], state[:64][shared])


def test_m_asin_is_the_device_librarys_asinf_bit_for_bit(tmp_path):
    if shutil.which("hipcc") is None:
        pytest.fail("hipcc not available: the probe is built like the product library")
    import sys
    sys.path.insert(0, ROOT)
    from __graft_entry__ import HIPCC_FLAGS
    so = str(tmp_path / "libasin_sweep_probe.so")
    subprocess.check_call(["hipcc", *HIPCC_FLAGS, "-fPIC", "-shared", "-o", so, os.path.join(ROOT, "tests", "emul", "asin_sweep_probe.hip")])
    lib = C.CDLL(so)
    pos = np.arange(0, int(np.float32(1.0).view(np.uint32)) + 1, 64, dtype=np.uint32).view(np.float32)
    edge = np.array([0.5, np.nextafter(np.float32(0.5), np.float32(0)), np.nextafter(np.float32(0.5), np.float32(1)), 1.0], dtype=np.float32)
    x = np.concatenate([-pos[::-1], pos, edge, -edge])
    x = np.concatenate([x, np.zeros(-x.size % 64, dtype=np.float32)])
    assert x.size > 3.3e7 and x.min() == -1 and x.max() == 1
    _PF = C.POINTER(C.c_float)
    for what, arg in (("ascending", x), ("interleaved", np.ascontiguousarray(x.reshape(64, -1).T).ravel())):
        mine, ref = np.zeros_like(arg), np.zeros_like(arg)
        rc = lib.asin_sweep(arg.ctypes.data_as(_PF), mine.ctypes.data_as(_PF), ref.ctypes.data_as(_PF), C.c_int(arg.size))
        assert rc == 0, "HIP error %d" % rc
        differ = mine.view(np.uint32) != ref.view(np.uint32)
        print("%s: %d arguments, %d differ from asinf" % (what, arg.size, differ.sum()))
        assert not differ.any(), (what, arg[differ][:8], mine[differ][:8], ref[differ][:8])
        assert np.abs(ref - np.arcsin(arg.astype(np.float64))).max() < 5e-7        # (and asinf is asin)

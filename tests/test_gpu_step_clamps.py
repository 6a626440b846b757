"""The fp32 device m_clamp (csrc/mds_math.hpp: one v_med3_f32) against the two selects it replaced, and the step that uses it.

1. A probe kernel evaluates m_clamp and m_min(m_max(x, lo), hi) -- the selects, as the host build and double keep them -- on every
   4096th fp32 bit pattern (both signs, the infinities and NaNs of both kinds among them), +-0, +-inf, NaN, and both bounds with their
   neighbours, for the two pairs of bounds the step clamps to: [min_motor_thrust, max_motor_thrust] of the mixer and [0, max_rpm] of
   the RPM clip, each rounded to fp32 as fill_consts rounds it.  0 differing bit patterns are allowed.  (The bare v_med3_f32 failed
   this on the MI355X: each of the 2046 signalling NaNs gave the upper bound, the selects the lower.  m_clamp canonicalises x first;
   the probe reads x from memory, so here that is an instruction.)
2. 20 control steps of 2 envs x 4 drones and of one ragged 1 x 3 shard, CF2P and CF2X handles (each executes its own arm of
   rotor_wrench alone), through mds_rollout_geometric in launch forms 1 and 2: the rows of every step and the final state are finite,
   the RPM columns within [0, max_rpm] -- and, where MDS_PARENT_LIB names a libmds.so built from the parent commit, bit for bit what
   that library computes (a child process loads it through MDS_LIB_PATH).  Without MDS_PARENT_LIB that comparison is skipped."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from oracle import np_oracle as O
from tests import helpers as H
from tests.test_gpu_parity import make_env, mds  # noqa: F401  (mds: the module's fixture)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 20
SHAPES = ((2, 4), (1, 3))


def bounds():
    """(name, lo, hi) in fp32, rounded from double as csrc/mds_consts.hpp does"""
    c = O.CF2P
    max_rpm = np.sqrt(c.THRUST2WEIGHT * c.GRAVITY / (4.0 * c.KF))
    return (("motor thrust", np.float32(9440.3 * 9440.3 * c.KF), np.float32(4.0 * c.KF * max_rpm * max_rpm)),
            ("rpm", np.float32(0.0), np.float32(max_rpm)))


def sweep_arguments(lo, hi):
    every = np.arange(0, 1 << 32, 4096, dtype=np.uint64).astype(np.uint32).view(np.float32)
    edge = [0.0, -0.0, np.inf, -np.inf, np.nan, -np.nan]
    for b in (lo, hi):
        edge += [b, np.nextafter(b, np.float32(-np.inf)), np.nextafter(b, np.float32(np.inf)), -b]
    x = np.concatenate([every, np.array(edge, dtype=np.float32)])
    return np.concatenate([x, np.zeros(-x.size % 64, dtype=np.float32)])


def test_m_clamp_is_the_two_selects_bit_for_bit(tmp_path):
    if shutil.which("hipcc") is None:
        pytest.fail("hipcc not available: the probe is built like the product library")
    sys.path.insert(0, ROOT)
    from __graft_entry__ import HIPCC_FLAGS
    so = str(tmp_path / "libclamp_sweep_probe.so")
    subprocess.check_call(["hipcc", *HIPCC_FLAGS, "-fPIC", "-shared", "-o", so, os.path.join(ROOT, "tests", "emul", "clamp_sweep_probe.hip")])
    lib = C.CDLL(so)
    _PF = C.POINTER(C.c_float)
    for name, lo, hi in bounds():
        assert np.isfinite(lo) and np.isfinite(hi) and lo < hi
        x = sweep_arguments(lo, hi)
        assert x.size > 1.0e6 and np.isnan(x).any() and np.isinf(x).any()
        mine, ref = np.zeros_like(x), np.zeros_like(x)
        rc = lib.clamp_sweep(x.ctypes.data_as(_PF), mine.ctypes.data_as(_PF), ref.ctypes.data_as(_PF), C.c_int(x.size), C.c_float(lo), C.c_float(hi))
        assert rc == 0, "HIP error %d" % rc
        differ = mine.view(np.uint32) != ref.view(np.uint32)
        print("%s [%r, %r]: %d arguments, %d differ from the selects" % (name, lo, hi, x.size, differ.sum()))
        assert not differ.any(), (name, x[differ][:8], mine[differ][:8], ref[differ][:8])
        # (and the selects are the clamp: a NaN gives the lower bound)
        want = np.where(np.isnan(x), lo, np.clip(x, lo, hi))
        np.testing.assert_array_equal(ref, want)


def fly(mds, model, E, D):
    """{name: array}: the rows of every step through forms 1 and 2 (one step per launch, so that every step's rows can be read back),
    the rows after one 20-step launch of form 2, and the final state of each"""
    torch = mds.torch
    xyz, rpy, P = H.c2_setup(E, D, phase="c3")
    out = {}
    for tag, form, per in (("form1", 1, 1), ("form2", 2, 1), ("form2_one_launch", 2, T)):
        env = make_env(mds, E, D, xyz, rpy, "float32", model=getattr(mds.DroneModel, model))
        env.set_trajectories(P)
        env.step(torch.zeros((E, D, 4), dtype=env.dtype, device=env.device))
        env.set_rollout_form(form, per)
        dt = env.CTRL_TIMESTEP
        rows = [env.rollout_geometric(k * dt * per, per, obs_every_step=True).cpu().numpy().copy() for k in range(T // per)]
        assert env.last_rollout_form() == form
        out[tag + "_rows"] = np.stack(rows).reshape(T // per, E * D, 20)
        out[tag + "_state"] = np.asarray(env.get_state()).reshape(-1, 13)
        env.close()
    return out


def fly_all(mds):
    return {"%s_%dx%d_%s" % (model, E, D, k): v for model in ("CF2P", "CF2X") for E, D in SHAPES for k, v in fly(mds, model, E, D).items()}


@pytest.fixture(scope="module")
def flights(mds):
    return fly_all(mds)


def test_twenty_steps_stay_finite_and_within_the_rpm_clip(flights):
    max_rpm = bounds()[1][2]
    assert len(flights) == 2 * len(SHAPES) * 6
    for k, v in flights.items():
        assert np.isfinite(v).all(), k
        if k.endswith("_rows"):
            assert v.dtype == np.float32, k
            assert v[..., 16:].min() >= 0 and v[..., 16:].max() <= max_rpm, k
            assert v[..., 16:].min() > 1000.0, k          # (flying: the wrench is not a row of zeros)


def test_rows_and_state_are_the_parent_librarys_bit_for_bit(flights, tmp_path):
    H.assert_same_bits(H.parent_library_flights("tests.test_gpu_step_clamps", "fly_all", tmp_path), flights)

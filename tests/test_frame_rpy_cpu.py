"""The rotation frame of csrc/mds_math.hpp on the CPU (g++ build of the header, tests/emul/frame_emul.cpp): the Euler angles read off
the frame's matrix (rpy_from_rot) against the attitudes of tests/golden/euler_convention.npz, gimbal arms included, with the tolerances
of the device test of obs[7:10] (test_gpu_parity.py::test_observation_rpy_is_the_reference_trees_convention_incl_gimbal_branches);
and the quaternion-only entry points (euler_from_quat, quat_rotate, thrust_dir(q)) equal to what the frame holds, bit for bit -- the
per-step kernels form per call what the whole-rollout kernel carries across its loop.  CPU only."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
_PD = C.POINTER(C.c_double)


@pytest.fixture(scope="module")
def frame_lib(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    so = str(tmp_path_factory.mktemp("frame_emul") / "libframe_emul.so")
    # the flags of tests/emul/emul.py
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-mfma", "-ffp-contract=fast", "-o", so,
                           os.path.join(ROOT, "tests", "emul", "frame_emul.cpp")])
    return C.CDLL(so)


def frame_all(lib, dtype, q, w):
    q = np.ascontiguousarray(q, dtype=np.float64)
    w = np.ascontiguousarray(w, dtype=np.float64)
    out = np.zeros((len(q), 18))
    getattr(lib, "frame_all_" + dtype)(C.c_int(len(q)), q.ctypes.data_as(_PD), w.ctypes.data_as(_PD), out.ctypes.data_as(_PD))
    return out


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_frame_rpy_is_the_reference_trees_convention_incl_gimbal_branches(frame_lib, dtype):
    from scipy.spatial.transform import Rotation
    d = np.load(os.path.join(G, "euler_convention.npz"))
    q, rpy_ref, g = d["quat"], d["rpy"], d["gimbal"]
    out = frame_all(frame_lib, dtype, q, np.zeros((len(q), 3)))
    rpy = out[:, 0:3]
    if dtype == "f64":
        print("f64 max |rpy - fixture| = %.3e" % np.abs(rpy - rpy_ref).max())
        np.testing.assert_allclose(rpy, rpy_ref, rtol=0, atol=1e-12)
        assert (rpy[g][:, 0] == 0).all() and g.sum() >= 48
    else:
        wrap = lambda a: (a + np.pi) % (2 * np.pi) - np.pi
        far = np.abs(np.abs(d["euler_in"][:, 1]) - np.pi / 2) > 2e-2              # well away from the threshold (4.47e-3)
        assert far.sum() >= 190
        R = Rotation.from_euler("xyz", rpy).as_matrix()
        print("f32 max |rpy - fixture| away from the arms = %.3e, max |R(rpy) - R(q)| = %.3e (away: %.3e)" % (
            np.abs(wrap(rpy[far] - rpy_ref[far])).max(), np.abs(R - d["R_quat"]).max(), np.abs(R[far] - d["R_quat"][far]).max()))
        assert np.abs(wrap(rpy[far] - rpy_ref[far])).max() < 5e-6
        assert np.abs(R - d["R_quat"]).max() < 5e-3
        assert np.abs(R[far] - d["R_quat"][far]).max() < 5e-6


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_quaternion_entry_points_are_the_frame_bit_for_bit(frame_lib, dtype):
    d = np.load(os.path.join(G, "euler_convention.npz"))
    rng = np.random.default_rng(5)
    q = np.concatenate([d["quat"], rng.normal(size=(4096, 4))])                    # (not normalised: R is scale invariant)
    w = rng.uniform(-6, 6, size=(len(q), 3))
    out = frame_all(frame_lib, dtype, q, w)
    assert np.array_equal(out[:, 0:3], out[:, 3:6])          # rpy_from_rot(frame) == euler_from_quat(q)
    assert np.array_equal(out[:, 6:9], out[:, 9:12])         # frame.av == quat_rotate(q, w)
    assert np.array_equal(out[:, 12:15], out[:, 15:18])      # thrust_dir(frame) == thrust_dir(q)
    # the thrust direction is R's third column less e3, in its cancellation-free form
    qn = q / np.linalg.norm(q, axis=1, keepdims=True)
    x, y, z, ww = qn.T
    ref = np.stack([2 * (x * z + ww * y), 2 * (y * z - ww * x), -2 * (x * x + y * y)], axis=1)
    err = np.abs(out[:, 12:15] - ref).max()
    print(dtype, "max |thrust_dir - float64 formula| = %.3e" % err)
    assert err < (1e-14 if dtype == "f64" else 2e-6)      # a dozen roundings of 6e-8 (the cast of q, v_rcp, the products) on entries up to 2

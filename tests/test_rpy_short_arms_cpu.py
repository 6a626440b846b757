"""The short arms of the Euler-angle block on the CPU (g++ build of csrc/mds_math.hpp, tests/emul/rpy_arms_emul.cpp).

On the device m_atan2, m_asin and rpy_from_rot take a short arm when a test holds in EVERY lane of the wave and the general arm
otherwise, so a lane's bits must not depend on which arm its wave took: each short arm has to give the general arm's bits wherever
its test holds.  The host build takes the flag as an argument, so both arms are run on the same inputs here and compared bit for bit.

1. m_atan2_arm: 0 < x < inf and |y| <= x (m_atan2_in_octant).  Every 64th fp32 ratio y / x of [-1, 1] at x = 1, every 512th at a mantissa
   that is no power of two and at magnitudes from 1e-30 to 1e30, the edges |y| = x and y = +-0, denormal x; and the inputs
   that must fail the test and go through the general arm: x <= 0, |y| > x, NaN, infinities.  The general arm itself is held to
   the one-piece m_atan2 it was cut from (restated in the emulation source), bit for bit, on all of these.
2. m_asin_arm: x * x < 0.25, every 64th fp32 of (-0.5, 0.5); at |x| = 0.5 and beyond the test fails.
3. rpy_from_rot_arm: no gimbal arm and both atan2 in their octant (rpy_is_plain).  Random unit quaternions, attitudes of normal flight,
   and attitudes on either side of |R20| = 0.99999.
CPU only."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_PD = C.POINTER(C.c_double)
_PF = C.POINTER(C.c_float)
_PI = C.POINTER(C.c_int)


@pytest.fixture(scope="module")
def arms_lib(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    so = str(tmp_path_factory.mktemp("rpy_arms_emul") / "librpy_arms_emul.so")
    # the flags of tests/emul/emul.py
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-mfma", "-ffp-contract=fast", "-o", so,
                           os.path.join(ROOT, "tests", "emul", "rpy_arms_emul.cpp")])
    return C.CDLL(so)


def atan2_arms(lib, y, x):
    y, x = (np.ascontiguousarray(a, dtype=np.float32) for a in np.broadcast_arrays(y, x))
    out, ok = np.zeros((x.size, 4), dtype=np.float32), np.zeros(x.size, dtype=np.int32)
    lib.atan2_arms_f32(C.c_int(x.size), y.ctypes.data_as(_PF), x.ctypes.data_as(_PF), out.ctypes.data_as(_PF), ok.ctypes.data_as(_PI))
    return out.view(np.uint32), ok.astype(bool)


def same_bits(a, b):
    """equal bit patterns; a NaN equals a NaN"""
    return (a == b) | (np.isnan(a.view(np.float32)) & np.isnan(b.view(np.float32)))


def floats_between(lo, hi, stride=1):
    """every stride-th non-negative fp32 value of [lo, hi], by bit pattern"""
    a, b = (int(np.float32(v).view(np.uint32)) for v in (lo, hi))
    return np.arange(a, b + 1, stride, dtype=np.uint32).view(np.float32)


@pytest.mark.parametrize("x0,stride", [(1.0, 64), (1.2345678, 512), (1e-30, 512), (3e-10, 512), (7e9, 512), (1e30, 512)])
def test_atan2_short_arm_is_the_general_arm_bit_for_bit_in_its_octant(arms_lib, x0, stride):
    ratio = np.concatenate([floats_between(0.0, 1.0, stride), floats_between(np.float32(0.9999), 1.0), floats_between(0.0, 1e-38, 4096)])
    x = np.float32(x0)
    y = ratio * x                                     # |y| <= x: a ratio <= 1 times x rounds to at most x
    y = np.concatenate([y, -y])
    assert np.abs(y).max() == x and (np.abs(y) <= x).all()
    b, ok = atan2_arms(arms_lib, y, x)
    assert ok.all()
    assert (b[:, 1] == b[:, 0]).all() and (b[:, 2] == b[:, 0]).all() and (b[:, 3] == b[:, 0]).all()
    # ... and the value is atan2's (the polynomial's 1e-7 and the 6e-8 of the reciprocal)
    assert np.abs(b[::8, 0].view(np.float32) - np.arctan2(y[::8].astype(np.float64), np.float64(x))).max() < 3e-7


def test_atan2_short_arm_at_the_edges_of_its_octant(arms_lib):
    tiny, den = np.float32(1.1754944e-38), np.float32(1e-45)            # the smallest normal, the smallest denormal
    x = np.array([1.0, 1.0, 1.0, 1.0, 3.5, 3.5, tiny, tiny, 1e-40, 1e-40, 1e-40, den, den, den, 3.4e38, 3.4e38], dtype=np.float32)
    y = np.array([0.0, -0.0, 1.0, -1.0, 3.5, -3.5, tiny, -0.0, 1e-40, -5e-41, 0.0, den, -den, 0.0, 3.4e38, -1.0], dtype=np.float32)
    b, ok = atan2_arms(arms_lib, y, x)
    assert ok.all()
    assert same_bits(b[:, 1], b[:, 0]).all() and same_bits(b[:, 2], b[:, 0]).all() and same_bits(b[:, 3], b[:, 0]).all()
    v = b[:, 0].view(np.float32)
    assert np.signbit(v[1]) and v[1] == 0 and not np.signbit(v[0])      # atan2(-0, 1) = -0
    assert abs(v[2] - np.pi / 4) < 2e-7 and abs(v[3] + np.pi / 4) < 2e-7


def test_atan2_takes_the_general_arm_outside_the_octant(arms_lib):
    rng = np.random.default_rng(11)
    n = 200_000
    th = rng.uniform(-np.pi, np.pi, n)
    mag = 10.0 ** rng.uniform(-20, 20, n)
    y, x = (mag * np.sin(th)).astype(np.float32), (mag * np.cos(th)).astype(np.float32)
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    sy = np.array([0.0, -0.0, 1.0, 1.0, -2.0, 0.5, nan, 1.0, nan, inf, -inf, 1.0, 1.0, inf, -inf, 0.0, 0.0], dtype=np.float32)
    sx = np.array([0.0, 0.0, 0.0, -1.0, 1.0, -0.0, 1.0, nan, nan, 1.0, 1.0, inf, -inf, inf, inf, -1.0, inf], dtype=np.float32)
    b, ok = atan2_arms(arms_lib, np.concatenate([y, sy]), np.concatenate([x, sx]))
    assert not ok[n:].any()                                             # x <= 0, |y| > x, NaN, Inf: none passes the test
    inside = (np.abs(th) <= np.pi / 4 - 1e-6)
    outside = (np.abs(th) >= np.pi / 4 + 1e-6)
    assert ok[:n][inside].all() and not ok[:n][outside].any() and outside.sum() > 100_000
    assert same_bits(b[:, 3], b[:, 0]).all()                            # the general arm is the one-piece atan2 it was cut from,
    assert same_bits(b[:, 2], b[:, 0]).all()                            # m_atan2 is the general arm wherever the test fails ...
    assert (b[ok, 1] == b[ok, 0]).all()                                 # ... and either arm where it holds
    # the short arm alone is NOT atan2 out there: the test is needed
    assert (b[:n][outside, 1] != b[:n][outside, 0]).mean() > 0.99
    err = np.abs(b[:n, 2].view(np.float32) - np.arctan2(y.astype(np.float64), x.astype(np.float64)))
    assert err.max() < 6e-7


def test_asin_short_arm_is_the_general_arm_bit_for_bit_below_one_half(arms_lib):
    pos = np.concatenate([floats_between(0.0, 0.5, 64), floats_between(np.float32(0.4999), 0.5)])
    pos = pos[pos < np.float32(0.5)]
    x = np.concatenate([pos, -pos]).astype(np.float32)
    assert (x * x < np.float32(0.25)).all() and x.size > 3.2e7          # the device's wave test, in fp32 as it forms it
    out = np.zeros((x.size, 2), dtype=np.float32)
    arms_lib.asin_arms_f32(C.c_int(x.size), x.ctypes.data_as(_PF), out.ctypes.data_as(_PF))
    b = out.view(np.uint32)
    assert (b[:, 1] == b[:, 0]).all()
    assert np.abs(out[::8, 0] - np.arcsin(x[::8].astype(np.float64))).max() < 1.2e-7  # 2 ulp of 0.52
    # from 0.5 on the test fails (x * x rounds to 0.25 or above), and it has to: the short arm leaves its range
    up = floats_between(0.5, 1.0, 4096)
    assert not (up * up < np.float32(0.25)).any()
    out = np.zeros((up.size, 2), dtype=np.float32)
    arms_lib.asin_arms_f32(C.c_int(up.size), up.ctypes.data_as(_PF), out.ctypes.data_as(_PF))
    assert np.abs(out[:, 0] - np.arcsin(up.astype(np.float64))).max() < 5e-7         # the general arm is asin up to 1
    assert (out[up > 0.6, 1] != out[up > 0.6, 0]).all()


def quat_from_rpy(r, p, y):
    from scipy.spatial.transform import Rotation
    return Rotation.from_euler("xyz", np.stack([r, p, y], axis=1)).as_quat()


def rpy_arms(lib, q):
    q = np.ascontiguousarray(q, dtype=np.float64)
    out, plain = np.zeros((len(q), 10), dtype=np.float32), np.zeros(len(q), dtype=np.int32)
    lib.rpy_arms_f32(C.c_int(len(q)), q.ctypes.data_as(_PD), out.ctypes.data_as(_PF), plain.ctypes.data_as(_PI))
    return out, plain.astype(bool)


def test_rpy_plain_block_is_the_general_path_bit_for_bit(arms_lib):
    rng = np.random.default_rng(3)
    n = 200_000
    anywhere = rng.normal(size=(n, 4))
    anywhere /= np.linalg.norm(anywhere, axis=1, keepdims=True)
    flight = quat_from_rpy(rng.uniform(-0.75, 0.75, n), rng.uniform(-0.7, 0.7, n), rng.uniform(-0.75, 0.75, n))   # 40 degrees = 0.698 rad
    # both sides of |R20| = 0.99999 (|pitch| = pi/2 - 4.47e-3), roll and yaw small so that nothing else decides
    m = 20_000
    edge = np.arcsin(0.99999)
    pitch = rng.choice([-1.0, 1.0], m) * (edge + rng.uniform(-2e-4, 2e-4, m))
    near = quat_from_rpy(rng.uniform(-0.1, 0.1, m), pitch, rng.uniform(-0.1, 0.1, m))
    out, plain = rpy_arms(arms_lib, np.concatenate([anywhere, flight, near]))
    b = out.view(np.uint32)
    general, short, picked, r20 = b[:, 0:3], b[:, 3:6], b[:, 6:9], out[:, 9]
    assert (picked == general).all()                         # rpy_from_rot is the general path whichever arm it takes
    assert (short[plain] == general[plain]).all()
    # the block is taken in normal flight, and not next to the gimbal arms
    assert plain[n:2 * n].mean() > 0.95 and 0.01 < plain[:n].mean() < 0.2, (plain[n:2 * n].mean(), plain[:n].mean())
    gimbal = np.abs(r20) >= np.float32(0.99999)
    assert not (plain & gimbal).any()
    e = slice(2 * n, None)
    assert gimbal[e].sum() > 5000 and (~gimbal[e]).sum() > 5000 and plain[e][~gimbal[e]].mean() > 0.99
    assert (out[e][gimbal[e], 0] == 0).all() and (np.abs(out[e][gimbal[e], 1]) == np.float32(np.pi / 2)).all()
    # without the test the block is wrong out there: it is the test that makes it safe
    assert (short[:n][~plain[:n]] != general[:n][~plain[:n]]).any(axis=1).mean() > 0.9

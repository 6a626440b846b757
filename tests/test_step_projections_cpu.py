"""The short forms of the fused step on the CPU (g++ build of csrc/mds_math.hpp, tests/emul/step_proj_emul.cpp).

1. integrate_q's sine and cosine.  Its argument is |w| dt / 2 > 0, 0.05 rad at 10 rad/s and 100 Hz.  For |x| <= 0.75 the fp32 m_sincos
   rounds k to 0, its Cody-Waite steps return x and its quadrant selects keep the first arm, so the two polynomials alone
   (m_sincos_reduced) give the same bits; m_sincos_small takes them when the whole wave is below 0.75 and m_sincos otherwise.  Proved
   here over every 64th fp32 value of [-0.75, 0.75] (16.7 million arguments), the 4096 values on either side of the threshold, and
   -- as a guard for the threshold itself -- by showing that the identity does break further out (beyond pi/4).  x = -0 is the one
   argument in the range where the bits differ (m_sincos returns sin = +0, the polynomials -0); it compares equal.

2. The controller's derivative terms.  (a x b) x a = b - (a . b) a for a unit a: reject(b, a) is one dot product and three FMAs where
   the reference (control/geometric.py:97-99) has two cross products, and b1d = b2d x b3d of two orthonormal vectors needs no
   normalisation (:91).  The tolerance is not chosen from the new forms: it is TWICE the largest error of the PARENT's fp32 form
   (the double cross product, the normalised b1d) against the same expression in float64 on the same fp32 unit vectors, which are
   normalised in fp32 the way the controller normalises them.  Errors are relative to |b| (absolute for the unit vector b1d).
   Measured on the 200 000 samples below, max error against float64, parent's fp32 form / new fp32 form (and new against parent):
       b3d_dot   1.79e-07 / 3.19e-07 (3.58e-07)
       b2d_dot   1.78e-07 / 3.16e-07 (3.51e-07)
       b1d       1.43e-07 / 2.63e-07 (2.98e-07)
   The new forms sit at 1.8 times the parent's error by this yardstick, inside the factor 2 and close to it.  The yardstick favours
   the parent: the float64 reference evaluates the parent's expression, (a x b) x a = |a|^2 b - (a . b) a, on unit vectors whose
   fp32 length is off by up to 1.5e-7, so the parent is charged its rounding alone and the projection also the (|a|^2 - 1) b by
   which the two expressions differ for such an a.  For b1d the new form is held to the factor 2 against float64 like the others;
   its distance from the parent's normalised form (2.98e-07, 2.1 times the parent's error: both roundings plus |b2d| |b3d| - 1) is
   printed and not asserted -- two fp32 values within e and 2 e of the same float64 value may be 3 e apart.
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
THRESHOLD = np.float32(0.75)


@pytest.fixture(scope="module")
def proj_lib(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    so = str(tmp_path_factory.mktemp("step_proj_emul") / "libstep_proj_emul.so")
    # the flags of tests/emul/emul.py
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-mfma", "-ffp-contract=fast", "-o", so,
                           os.path.join(ROOT, "tests", "emul", "step_proj_emul.cpp")])
    return C.CDLL(so)


def sincos_three(lib, x):
    x = np.ascontiguousarray(x, dtype=np.float32)
    out = np.zeros((x.size, 6), dtype=np.float32)
    lib.sincos_three_f32(C.c_int(x.size), x.ctypes.data_as(_PF), out.ctypes.data_as(_PF))
    return out.view(np.uint32)


def floats_between(lo, hi, stride=1):
    """every stride-th non-negative fp32 value of [lo, hi], by bit pattern"""
    a, b = (int(np.float32(v).view(np.uint32)) for v in (lo, hi))
    return np.arange(a, b + 1, stride, dtype=np.uint32).view(np.float32)


def test_reduced_sincos_is_the_general_one_bit_for_bit_up_to_the_threshold(proj_lib):
    pos = np.concatenate([floats_between(0.0, THRESHOLD, 64), floats_between(np.float32(0.7499), THRESHOLD),
                          floats_between(1e-12, 1e-6, 4096), [np.float32(0.05), THRESHOLD]]).astype(np.float32)
    x = np.concatenate([pos, -pos[pos > 0]])
    assert x.size > 3.3e7 and np.abs(x).max() == THRESHOLD
    b = sincos_three(proj_lib, x)
    assert (b[:, 2:4] == b[:, 0:2]).all() and (b[:, 4:6] == b[:, 0:2]).all()
    # -0: equal as numbers (the general path's sine is +0)
    z = sincos_three(proj_lib, [-0.0]).view(np.float32)
    assert (z[:, 2:4] == z[:, 0:2]).all() and (z[:, 4:6] == z[:, 0:2]).all()


def test_above_the_threshold_the_small_form_is_the_general_path(proj_lib):
    up = floats_between(np.nextafter(THRESHOLD, np.float32(1)), np.float32(0.7501))
    far = np.linspace(0.7501, np.pi, 200001).astype(np.float32)
    x = np.concatenate([up, -up, far, -far])
    b = sincos_three(proj_lib, x)
    assert (b[:, 4:6] == b[:, 0:2]).all()
    # the identity is one of the small range and not of the test: it holds up to pi/4 (k = 0), and further out the polynomials
    # alone leave their range (at 2 rad the truncation error of the sine is 5e-5)
    wrong = (b[:, 2:4] != b[:, 0:2]).any(axis=1)
    assert wrong[np.abs(x) > 2.0].all() and not wrong[np.abs(x) < 0.78].any()


def frame_derivs(lib, f, yaw, fd, inner):
    arrs = [np.ascontiguousarray(a, dtype=np.float64) for a in (f, yaw, fd, inner)]
    out = np.zeros((len(yaw), 27))
    lib.frame_derivs(C.c_int(len(yaw)), *[a.ctypes.data_as(_PD) for a in arrs], out.ctypes.data_as(_PD))
    return out.reshape(-1, 9, 3)


def test_projections_are_as_close_to_float64_as_the_double_cross_products(proj_lib):
    rng = np.random.default_rng(7)
    n = 200_000
    # thrust directions within the controller's 40 degree tilt cone and, for half the samples, anywhere; any yaw
    tilt = np.where(np.arange(n) % 2 == 0, rng.uniform(0, np.deg2rad(40), n), np.arccos(rng.uniform(-0.95, 1, n)))
    az = rng.uniform(-np.pi, np.pi, n)
    f = rng.uniform(0.05, 0.6, (n, 1)) * np.stack([np.sin(tilt) * np.cos(az), np.sin(tilt) * np.sin(az), np.cos(tilt)], axis=1)
    yaw = rng.uniform(-np.pi, np.pi, n)
    # f_dot = (m / |f|) R (Kp ev) and inner: up to ~10 / s in closed loop, down to nothing at hover; every direction
    mag = lambda: 10.0 ** rng.uniform(-3, 1, (n, 1))
    direc = lambda: (lambda v: v / np.linalg.norm(v, axis=1, keepdims=True))(rng.normal(size=(n, 3)))
    fd, inner = mag() * direc(), mag() * direc()
    o = frame_derivs(proj_lib, f, yaw, fd, inner)
    err = lambda a, b, scale: (np.abs(a - b).max(axis=1) / scale).max()
    for what, k, scale in (("b3d_dot", 0, np.linalg.norm(fd, axis=1)), ("b2d_dot", 3, np.linalg.norm(inner, axis=1)), ("b1d", 6, 1.0)):
        new, parent, ref = o[:, k], o[:, k + 1], o[:, k + 2]
        e_parent, e_new, d = err(parent, ref, scale), err(new, ref, scale), err(new, parent, scale)
        print("%-8s max error against float64: parent's fp32 form %.2e, new fp32 form %.2e; new against parent %.2e" % (what, e_parent, e_new, d))
        assert 2e-8 < e_parent < 1e-6, (what, e_parent)                  # the yardstick is fp32 rounding, neither zero nor broken
        assert e_new <= 2 * e_parent, (what, e_new, e_parent)
        if what != "b1d":                                                # the two projections: also against the parent's form itself
            assert d <= 2 * e_parent, (what, d, e_parent)

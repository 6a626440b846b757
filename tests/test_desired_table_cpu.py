"""The desired-state table of the whole-rollout loop, host side (csrc/mds_math.hpp built with g++; tests/desired_table_main.cpp):

  * the cut: for 10^5 seeded (a, omega, s, c, p) the two halves -- lemniscate_desired8, then desired8_p_rel / desired8_pre -- return
    the bytes of lemniscate_from_sc<float, true> followed by the controller's p_rel and the x, y of its tw, and the controller
    returns the same u from either.  Both sides are built with
    every product rounded on its own (-ffp-contract=off, and m_fma rounding its product: MDS_HOST_UNFUSED_FMA), which makes the
    comparison one of operations, operands and association; which products the device contracts is stated by the halves in m_fma and
    checked on the GPU, rows with the table on against off (tests/test_gpu_desired_table.py).
  * the eight values are finite and are what they are said to be (des.p = inv (mx, my), des.a = inv3 (Xx, Xy), to rounding).
  * the time of row k is t0 after k additions of the control period, as NumPy adds them -- not t0 + k dt.
  * the rule: true for n <= 64; one a changed at a row >= 64 makes it false while the phase rule stays true; a changed omega makes
    both false; n that is no multiple of 64.
  * the same checks as a program of its own, built plain and under -fsanitize=address,undefined.
CPU only."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "desired_table_main.cpp")
FLAGS = ["-std=c++17", "-ffp-contract=off", "-DMDS_HOST_UNFUSED_FMA"]
N_RAND = 100000


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    so = str(tmp_path_factory.mktemp("desired_table") / "libdesired_table.so")
    subprocess.check_call(["g++", "-O2", *FLAGS, "-fPIC", "-shared", "-o", so, SRC])
    so_lib = C.CDLL(so)
    for f in (so_lib.dt_phase_periodic, so_lib.dt_desired_periodic):
        f.restype = C.c_int
        f.argtypes = [C.c_void_p, C.c_long]
    so_lib.dt_times.argtypes = [C.c_double, C.c_double, C.c_int, C.c_void_p]
    return so_lib


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def halves(lib):
    rng = np.random.default_rng(23)
    th = rng.uniform(-np.pi, np.pi, N_RAND)
    x = np.empty((N_RAND, 14), dtype=np.float32)
    x[:, 0] = rng.uniform(0.2, 3.0, N_RAND)
    x[:, 1] = rng.uniform(-3.0, 3.0, N_RAND)
    x[:, 2], x[:, 3] = np.sin(th), np.cos(th)
    x[:, 4:6] = rng.uniform(-3.0, 3.0, (N_RAND, 2))
    x[:, 6] = rng.uniform(0.0, 2.0, N_RAND)
    q = rng.uniform(-1.0, 1.0, (N_RAND, 4)) * np.array([0.5, 0.5, 0.5, 1.0])
    x[:, 7:11] = q / np.linalg.norm(q, axis=1, keepdims=True)
    x[:, 11:14] = rng.uniform(-2.0, 2.0, (N_RAND, 3))
    whole, split = np.full((N_RAND, 10), np.nan, np.float32), np.full((N_RAND, 10), np.nan, np.float32)
    eight = np.full((N_RAND, 8), np.nan, np.float32)
    lib.dt_both(C.c_int(N_RAND), _ptr(x), _ptr(whole), _ptr(split), _ptr(eight))
    return x, whole, split, eight


def test_the_two_halves_are_from_sc_and_the_controllers_terms_to_the_byte(halves):
    _, whole, split, _ = halves
    assert np.isfinite(whole).all()
    assert np.abs(whole[:, 2:4]).max() > 1.0 and np.abs(whole[:, 4:6]).max() > 5.0 and np.abs(whole[:, 7:]).max() > 0          # (not a row of zeros)
    assert whole.tobytes() == split.tobytes(), np.argwhere(whole.view(np.uint32) != split.view(np.uint32))[:5]


def test_the_eight_values_are_the_factors_of_the_desired_state(halves):
    x, _, _, eight = halves
    assert np.isfinite(eight).all()
    a, om, s, c = (x[:, k].astype(np.float64) for k in range(4))
    inv, mx, my, inv3, vx, vy, Xx, Xy = (eight[:, k].astype(np.float64) for k in range(8))
    den = 1.0 + s * s
    th2 = 2.0 * np.arctan2(s, c)
    # float32 results of a handful of operations each: 2^-20 of the value's scale leaves room for some 16 roundings
    tol = 2.0 ** -20

    def close(got, want, scale):
        assert (np.abs(got - want) <= tol * scale).all(), np.abs(got - want).max()

    close(inv, 1.0 / den, 1.0)
    close(inv * mx, a * s * c / den, a)
    close(inv * my, a * c / den, a)
    close(inv3 * Xx, 4 * a * om * om * np.sin(th2) * (3 * np.cos(th2) + 7) / (np.cos(th2) - 3) ** 3, 40 * a * om * om)
    close(inv3 * Xy, a * om * om * c * (44 * np.cos(th2) + np.cos(2 * th2) - 21) / (np.cos(th2) - 3) ** 3, 66 * a * om * om)
    close(vx, -a * om * (s ** 4 + s * s + (s * s - 1) * c * c) / den ** 2, 3 * a * np.abs(om))
    close(vy, -a * om * s * (s * s + 2 * c * c + 1) / den ** 2, 3 * a * np.abs(om))


@pytest.mark.parametrize("t0", [0.0, 0.37, 1234.5])
def test_row_times_are_repeated_additions(lib, t0):
    n, dt = 2100, 1.0 / 48.0 + 1e-3
    got = np.full(n, np.nan)
    lib.dt_times(C.c_double(t0), C.c_double(dt), C.c_int(n), _ptr(got))
    want = np.empty(n)
    t = np.float64(t0)
    for k in range(n):
        want[k] = t
        t = t + np.float64(dt)
    assert got.tobytes() == want.tobytes()
    assert (got != t0 + np.arange(n) * dt).any()                # (the product form is another sequence: the test can tell them apart)


def _params(n, seed=0):
    rng = np.random.default_rng(seed)
    P = rng.uniform(-2.0, 2.0, (n, 7))
    P[:, 0] = 1.0 + 0.01 * (np.arange(n) % 64)
    P[:, 1] = 0.5 + 0.01 * (np.arange(n) % 64)
    P[:, 6] = 0.1 * (np.arange(n) % 64) - 3.0
    return P


def _rules(lib, P):
    P = np.ascontiguousarray(P, dtype=np.float64)
    return bool(lib.dt_phase_periodic(_ptr(P), C.c_long(P.shape[0]))), bool(lib.dt_desired_periodic(_ptr(P), C.c_long(P.shape[0])))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 100, 128, 259])
def test_the_rule(lib, n):
    P = _params(n, n)
    assert _rules(lib, P) == (True, True)
    for row in (64, n - 1):
        if row >= n:
            continue
        Q = P.copy()
        Q[row, 0] = np.nextafter(Q[row, 0], np.inf)              # one a, by one double ulp
        assert _rules(lib, Q) == (True, n <= 64), (n, row)
        Q = P.copy()
        Q[row, 1] = np.nextafter(Q[row, 1], np.inf)              # one omega
        assert _rules(lib, Q) == (n <= 64, n <= 64), (n, row)
        Q = P.copy()
        Q[row, 6] = np.nextafter(Q[row, 6], np.inf)              # one phase_shift
        assert _rules(lib, Q) == (n <= 64, n <= 64), (n, row)
    if n > 64:      # what differs only below float32 still differs as uploaded
        Q = P.copy()
        Q[64, 0] += 1e-12
        assert np.float32(Q[64, 0]) == np.float32(P[64, 0]) and _rules(lib, Q) == (True, False)
    # the centres and the yaw rate do not enter
    Q = P.copy()
    Q[:, 2:6] += 1.0
    assert _rules(lib, Q) == (True, True)


@pytest.mark.parametrize("san", [False, True])
def test_stand_alone_program_plain_and_under_address_and_undefined_sanitizers(tmp_path, san):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "desired_table_main")
    extra = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if san else ["-O2"]
    subprocess.check_call(["g++", *extra, *FLAGS, "-o", exe, SRC])
    env = dict(os.environ, UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1", ASAN_OPTIONS="detect_leaks=0:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert "0 unequal outputs, 0 wrong row times, 0 wrong periodicity decisions" in r.stdout

"""The phase table of the whole-rollout loop, host side (csrc/mds_math.hpp built with g++, float and double; tests/phase_table_main.cpp):

  * lemniscate_local is lemniscate_from_sc behind (s, c) = m_sincos(reduced_phase(t, omega, phase_shift)): for 10^5 random
    (t in [0, 300], omega, phase_shift, a) the two return the same bytes, in the general and in the yaw-free form -- what lets the
    loop take the pair from a table another kernel filled.
  * lemniscate_phase_periodic, the scan mds_set_lemniscate decides the handle's flag with, against a NumPy statement of the rule.
  * the same two checks as a program of its own under -fsanitize=address,undefined.
CPU only."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "phase_table_main.cpp")
N_RAND = 100000


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    so = str(tmp_path_factory.mktemp("phase_table") / "libphase_table.so")
    # the flags of tests/emul/emul.py
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-mfma", "-ffp-contract=fast", "-o", so, SRC])
    so_lib = C.CDLL(so)
    so_lib.pt_phase_periodic.restype = C.c_int
    so_lib.pt_phase_periodic.argtypes = [C.c_void_p, C.c_long]
    return so_lib


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.mark.parametrize("y0", [0, 1])
@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_from_sc_behind_the_phase_is_lemniscate_local_to_the_byte(lib, dt, y0):
    rng = np.random.default_rng(11)
    P = np.zeros((N_RAND, 7))
    P[:, 0] = rng.uniform(0.2, 3.0, N_RAND)
    P[:, 1] = rng.uniform(-3.0, 3.0, N_RAND)
    P[:, 2:5] = rng.uniform(-5.0, 5.0, (N_RAND, 3))
    P[:, 5] = np.where(rng.integers(0, 3, N_RAND) == 0, 0.0, rng.uniform(-1.0, 1.0, N_RAND))      # (the yaw-free form does not read it)
    P[:, 6] = rng.uniform(-7.0, 7.0, N_RAND)
    t = rng.uniform(0.0, 300.0, N_RAND)
    T = np.float32 if dt == "f32" else np.float64
    whole, split = np.full((N_RAND, 11), np.nan, dtype=T), np.full((N_RAND, 11), np.nan, dtype=T)
    getattr(lib, f"pt_lem_{dt}")(C.c_int(N_RAND), _ptr(P), _ptr(t), C.c_int(y0), _ptr(whole), _ptr(split))
    assert np.isfinite(whole).all()
    assert np.abs(whole[:, :2]).max() > 0.5 and np.abs(whole[:, 6:8]).max() > 1.0          # (not a row of zeros)
    assert whole.tobytes() == split.tobytes(), np.argwhere(whole.view(np.uint8) != split.view(np.uint8))[:5]


def periodic_np(P):
    """The rule: rows 64 apart have the same omega and phase_shift, as doubles."""
    return bool(np.array_equal(P[64:, 1], P[:-64, 1]) and np.array_equal(P[64:, 6], P[:-64, 6])) if P.shape[0] > 64 else True


def periodic_lib(lib, P):
    P = np.ascontiguousarray(P, dtype=np.float64)
    return bool(lib.pt_phase_periodic(_ptr(P), C.c_long(P.shape[0])))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 128, 259])
def test_periodicity_scan(lib, n):
    rng = np.random.default_rng(n)
    P = rng.uniform(-2.0, 2.0, (n, 7))
    P[:, 1] = 0.5 + 0.01 * (np.arange(n) % 64)
    P[:, 6] = 0.1 * (np.arange(n) % 64) - 3.0
    assert periodic_np(P) and periodic_lib(lib, P)
    for col in (1, 6):
        for row in (64, n - 1):
            if row >= n:
                continue
            Q = P.copy()
            Q[row, col] = np.nextafter(Q[row, col], np.inf)                # one double ulp
            want = periodic_np(Q)
            assert want == (n <= 64), (n, col, row)                        # (a row without a partner 64 away decides nothing)
            assert periodic_lib(lib, Q) == want, (n, col, row)
    # what differs in fp32 only after rounding still differs as uploaded: the compare is on the doubles
    if n > 64:
        Q = P.copy()
        Q[64, 1] += 1e-12
        assert np.float32(Q[64, 1]) == np.float32(P[64, 1]) and not periodic_lib(lib, Q)


def test_stand_alone_checks_under_address_and_undefined_sanitizers(tmp_path):
    """tests/phase_table_main.cpp as a program: exit status 0 when the split form returns the whole form's bytes on its own 2 x 10^5
    inputs, the scan decides as the rule does on vectors of exactly n rows, and the sanitizers have nothing to report."""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "phase_table_main")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-mfma", "-ffp-contract=fast", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-o", exe, SRC])
    env = dict(os.environ, UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1", ASAN_OPTIONS="detect_leaks=0:halt_on_error=1")   # as tests/emul/simt/simt.py
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert "0 unequal outputs, 0 wrong periodicity decisions" in r.stdout

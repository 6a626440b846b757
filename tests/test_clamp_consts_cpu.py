"""The products of constants that fill_consts (csrc/mds_consts.hpp) hands the kernels -- arm kf, arm sqrt(1/2) kf, the signed halves
of kR -- are, bit for bit, the expressions the device formed from the rounded constants every step before: in fp32 and in fp64, for
CF2X and CF2P, against the same expressions in the host build and against NumPy's arithmetic of the same width.  And the host
m_clamp is still the two selects: max(x, lo) = x > lo ? x : lo, then min(., hi) = . < hi ? . : hi (a NaN gives lo; -0 against a +0
bound gives +0).  CPU only: a g++ build of tests/emul/clamp_consts_probe.cpp."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MDS_CF2X, MDS_CF2P = 0, 1


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    so = str(tmp_path_factory.mktemp("clamp_consts") / "libclamp_consts_probe.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-mfma", "-ffp-contract=fast", "-o", so,
                           os.path.join(ROOT, "tests", "emul", "clamp_consts_probe.cpp")])
    return C.CDLL(so)


def test_the_model_constants_are_the_headers():
    text = open(os.path.join(ROOT, "include", "mds.h")).read()
    import re
    for name, val in (("MDS_CF2X", MDS_CF2X), ("MDS_CF2P", MDS_CF2P)):
        m = re.search(name + r"\s*=\s*(\d+)", text)
        assert m and int(m.group(1)) == val, name


@pytest.mark.parametrize("model", [MDS_CF2X, MDS_CF2P])
@pytest.mark.parametrize("sfx,dt", [("f32", np.float32), ("f64", np.float64)])
def test_host_products_are_the_device_expressions_bit_for_bit(probe, model, sfx, dt):
    base, got, want = np.zeros(6, dt), np.zeros(5, dt), np.zeros(5, dt)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    getattr(probe, "probe_fields_" + sfx)(C.c_int(model), ptr(base), ptr(got), ptr(want))
    arm, kf, k0, k1, k2, cf2x = base
    assert cf2x == (1 if model == MDS_CF2X else 0)
    assert arm == dt(0.0397) and kf == dt(3.16e-10) and k1 == dt(117.3)
    bits = np.uint32 if dt is np.float32 else np.uint64
    print(sfx, model, got, want)
    np.testing.assert_array_equal(got.view(bits), want.view(bits))
    # the same products in NumPy's arithmetic of the same width (one rounding per operation, left to right)
    mine = np.array([arm * kf, arm * dt(0.70710678118654752440) * kf, dt(-0.5) * k0, dt(0.5) * k1, dt(-0.5) * k2], dtype=dt)
    assert mine.dtype == dt
    np.testing.assert_array_equal(got.view(bits), mine.view(bits))
    assert (got[:2] > 0).all() and got[2] < 0 < got[3] and got[4] < 0


@pytest.mark.parametrize("sfx,dt", [("f32", np.float32), ("f64", np.float64)])
def test_host_m_clamp_is_still_the_two_selects(probe, sfx, dt):
    rng = np.random.default_rng(5)
    for lo, hi in ((dt(0.0), dt(21702.64)), (dt(0.02816), dt(0.59535)), (dt(-3200), dt(3200))):
        edge = [0.0, -0.0, np.inf, -np.inf, np.nan, lo, hi, np.nextafter(lo, dt(-np.inf)), np.nextafter(lo, dt(np.inf)),
                np.nextafter(hi, dt(-np.inf)), np.nextafter(hi, dt(np.inf)), -lo, -hi, np.finfo(dt).tiny / 4, -np.finfo(dt).tiny / 4]
        x = np.concatenate([np.array(edge, dtype=dt), (rng.standard_normal(4096) * float(hi) * 2).astype(dt),
                            (rng.standard_normal(4096) * float(hi) * 1e-3).astype(dt)])
        out = np.zeros_like(x)
        ct = C.c_float if dt is np.float32 else C.c_double
        getattr(probe, "probe_clamp_" + sfx)(x.ctypes.data_as(C.c_void_p), C.c_int(x.size), ct(lo), ct(hi), out.ctypes.data_as(C.c_void_p))
        with np.errstate(invalid="ignore"):
            r = np.where(x > lo, x, lo)
            r = np.where(r < hi, r, hi).astype(dt)
        bits = np.uint32 if dt is np.float32 else np.uint64
        np.testing.assert_array_equal(out.view(bits), r.view(bits))
        assert out[4] == lo                                                       # NaN -> lo

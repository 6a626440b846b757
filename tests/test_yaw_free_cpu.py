"""The yaw-free forms of the trajectory and the controller on the CPU (g++ build of csrc/mds_math.hpp, tests/emul/yaw_free_emul.cpp).

lemniscate_local<T, true> and geometric_control<T, true> -- what the kernels of a handle whose Lemniscates were all uploaded with
yaw_rate = +-0 run -- drop the products by the literal zeros and the literal one of such a desired state and nothing else (DESIGN.md
section 4 has the argument term by term).  The contract, checked here in float and in double against the general forms at
yaw_rate = +-0:

  * every output, GeoAux included, is == the general form's;
  * where no output is a zero the outputs are the same bytes (the only possible difference is the sign of an exact zero);
  * the yaw-free controller is as close to oracle/np_oracle.geometric_compute as the general one is asked to be
    (tests/test_emul_device_math.py::test_geometric_golden: 1e-13 / 1e-6 relative RPM on the golden observations).

Inputs: 10^5 random finite states plus the degenerate ones (identity attitude at rest, p_rel = 0, des.v along one axis, the
commanded force through zero, the tilt limit taken).  The same comparison also runs as a stand-alone program built with
-fsanitize=address,undefined.  CPU only."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from oracle import np_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "emul", "yaw_free_emul.cpp")
G = os.path.join(ROOT, "tests", "golden")
N_RAND = 100000
# rpm 4 | u 4 | force | w_des 3 | b1d 3 | b2d 3 | b3d 3
N_OUT = 21
KP, G_CTRL = 2.25, 9.81          # GeometricControl's defaults (the shim's constants)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    so = str(tmp_path_factory.mktemp("yaw_free_emul") / "libyaw_free_emul.so")
    # the flags of tests/emul/emul.py
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-mfma", "-ffp-contract=fast", "-o", so, SRC])
    return C.CDLL(so)


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def geo_both(lib, dt, obs, des):
    obs, des = np.ascontiguousarray(obs, dtype=np.float64), np.ascontiguousarray(des, dtype=np.float64)
    T = np.float32 if dt == "f32" else np.float64
    gen, y0 = np.zeros((obs.shape[0], N_OUT), dtype=T), np.zeros((obs.shape[0], N_OUT), dtype=T)
    getattr(lib, f"yf_geo_{dt}")(C.c_int(obs.shape[0]), _ptr(obs), _ptr(des), _ptr(gen), _ptr(y0))
    return gen, y0


def lem_both(lib, dt, P, t):
    P, t = np.ascontiguousarray(P, dtype=np.float64), np.ascontiguousarray(t, dtype=np.float64)
    T = np.float32 if dt == "f32" else np.float64
    gen, y0 = np.zeros((P.shape[0], 11), dtype=T), np.zeros((P.shape[0], 11), dtype=T)
    getattr(lib, f"yf_lem_{dt}")(C.c_int(P.shape[0]), _ptr(P), _ptr(t), _ptr(gen), _ptr(y0))
    return gen, y0


def _quat(rng, n, spread):
    q = rng.normal(size=(n, 4)) * np.array([spread, spread, spread, 1.0])
    return q / np.linalg.norm(q, axis=1, keepdims=True)


def _random_inputs(n, seed=7):
    rng = np.random.default_rng(seed)
    obs, des = np.zeros((n, 20)), np.zeros((n, 11))
    obs[:, 0:3] = rng.uniform(-2, 2, (n, 3))
    obs[:, 3:7] = _quat(rng, n, 0.5)
    obs[:, 10:13] = rng.uniform(-2, 2, (n, 3))
    obs[:, 13:16] = rng.uniform(-3, 3, (n, 3))
    des[:, 0:2] = rng.uniform(-1, 1, (n, 2))
    des[:, 3:5] = rng.uniform(-1.5, 1.5, (n, 2))
    des[:, 6:8] = rng.uniform(-5, 5, (n, 2))
    des[:, 10] = np.where(rng.integers(0, 2, n) == 1, -0.0, 0.0)          # yaw_rate = +-0, both signs
    return obs, des


def _degenerate_inputs():
    """Named rows; every one keeps the desired frame defined (b3d not along x), so every output is finite."""
    rows = []

    def add(name, obs, des):
        rows.append((name, np.array(obs, dtype=np.float64), np.array(des, dtype=np.float64)))
    rest = np.zeros(20)
    rest[6] = 1.0
    zero = np.zeros(11)
    add("identity attitude at rest", rest, zero)
    o = rest.copy()
    o[0:3] = [0.3, -0.2, 0.0]
    d = zero.copy()
    d[0:2] = [0.3, -0.2]
    add("p_rel = 0", o, d)
    d = d.copy()
    d[10] = -0.0
    add("p_rel = 0, yaw_rate = -0", o, d)
    for ax in (0, 1):
        for sgn in (1.0, -1.0):
            d = zero.copy()
            d[3 + ax] = sgn * 1.2
            add(f"des.v along {'xy'[ax]} ({sgn:+.0f})", rest, d)
            o = rest.copy()
            o[3:7] = [0.0, 0.0, np.sin(0.4), np.cos(0.4)]                  # yawed: R mixes x and y only
            add(f"des.v along {'xy'[ax]} ({sgn:+.0f}), yawed drone", o, d)
    # commanded force through zero: f_w.z = m (g - Kp p_rel.z) changes sign at p_rel.z = g / Kp; a lateral offset keeps |f_w| > 0
    z0 = G_CTRL / KP
    # (at exactly g / Kp the tilt arm scales the lateral part by f_w.z = 0: the force is zero, its direction undefined, and both forms
    # return NaN -- the reference's own singularity, test_both_forms_are_undefined_where_the_commanded_force_is_zero)
    for dz in (-1e-3, -1e-6, 1e-6, 1e-3, 0.5):
        o = rest.copy()
        o[0:3] = [0.0, 0.4, z0 + dz]
        add(f"force through zero (p_rel.z = g/Kp {dz:+g})", o, zero)
    # tilt limit taken: lateral demand well beyond 40 degrees
    for off in ([3.0, 1.0, 0.0], [-2.5, 2.5, 0.2], [0.0, 4.0, -0.1]):
        o = rest.copy()
        o[0:3] = off
        o[3:7] = [0.1, -0.05, 0.2, 0.97]
        o[3:7] /= np.linalg.norm(o[3:7])
        add(f"tilt limit taken (offset {off})", o, zero)
    # a drone that has already tilted and yawed, at its set-point
    o = rest.copy()
    o[3:7] = [0.3, 0.2, -0.5, 0.78]
    o[3:7] /= np.linalg.norm(o[3:7])
    o[13:16] = [0.5, -1.0, 2.0]
    add("tilted drone at its set-point", o, zero)
    return rows


def _assert_contract(gen, y0, names=None):
    """== everywhere; the same bytes on every row without a zero among its outputs.  Returns the share of byte-equal rows."""
    assert np.isfinite(gen).all() and np.isfinite(y0).all()
    ne = gen != y0
    assert not ne.any(), (np.argwhere(ne)[:5], None if names is None else [names[i] for i in np.unique(np.argwhere(ne)[:, 0])[:5]])
    # b2d.x (column 15) is a zero for every input -- b2d = unit(b3d x (1, 0, 0)) -- with the sign of inv_n1 * (b3d.y * 0 - b3d.z * 0) in the
    # general form and + in the yaw-free one: it is compared with == above and left out of the byte comparison, which would otherwise
    # have no row to look at
    keep = np.arange(gen.shape[1]) != 15
    a, b = np.ascontiguousarray(gen[:, keep]), np.ascontiguousarray(y0[:, keep])
    same = (a.view(np.uint8).reshape(a.shape[0], -1) == b.view(np.uint8).reshape(b.shape[0], -1)).all(axis=1)
    no_zero = ~((a == 0).any(axis=1) | (b == 0).any(axis=1))
    assert same[no_zero].all(), np.flatnonzero(no_zero & ~same)[:5]
    return same.mean(), no_zero.mean()


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_controller_equals_the_general_form_on_random_states(lib, dt):
    obs, des = _random_inputs(N_RAND)
    gen, y0 = geo_both(lib, dt, obs, des)
    share, nz = _assert_contract(gen, y0)
    print(f"{dt}: {N_RAND} random states, byte-equal rows {100 * share:.3f} % (rows without a zero output {100 * nz:.3f} %)")
    # the tilt arm is taken by a fair share of these states, and not by all
    b3z = gen[:, 20]
    lim = np.cos(40 * np.pi / 180)
    taken = np.abs(b3z - lim) < 1e-5
    assert 0.02 < taken.mean() < 0.98, taken.mean()


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_controller_equals_the_general_form_on_degenerate_states(lib, dt):
    rows = _degenerate_inputs()
    names = [r[0] for r in rows]
    gen, y0 = geo_both(lib, dt, np.stack([r[1] for r in rows]), np.stack([r[2] for r in rows]))
    share, nz = _assert_contract(gen, y0, names)
    print(f"{dt}: {len(rows)} degenerate states, byte-equal rows {100 * share:.1f} % (rows without a zero output {100 * nz:.1f} %)")
    for name, a, b in zip(names, gen, y0):
        if a.tobytes() != b.tobytes():
            print("   differs in the sign of a zero:", name, np.flatnonzero(np.signbit(a) != np.signbit(b)))


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_both_forms_are_undefined_where_the_commanded_force_is_zero(lib, dt):
    obs, des = np.zeros((1, 20)), np.zeros((1, 11))
    obs[0, 6] = 1.0
    obs[0, 0:3] = [0.0, 0.4, G_CTRL / KP]        # Kp p_rel.z rounds to g in fp32 and in double
    gen, y0 = geo_both(lib, dt, obs, des)
    # the torques and w_des are NaN in both; the general form is NaN wherever the yaw-free one is (b2d.x is NaN * 0 there, a literal 0 here)
    assert np.isnan(gen[0, 5:8]).all() and np.isnan(y0[0, 5:8]).all() and np.isnan(gen[0, 9:12]).all() and np.isnan(y0[0, 9:12]).all()
    assert (np.isnan(gen) | ~np.isnan(y0)).all()
    ok = ~np.isnan(gen)
    assert (gen[ok] == y0[ok]).all()


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_lemniscate_equals_the_general_form(lib, dt):
    rng = np.random.default_rng(11)
    n = N_RAND
    P = np.zeros((n, 7))
    P[:, 0], P[:, 1] = rng.uniform(0.5, 2.0, n), rng.uniform(0.2, 2.0, n)
    P[:, 2:5] = rng.uniform(-5, 5, (n, 3))
    P[:, 5] = np.where(rng.integers(0, 2, n) == 1, -0.0, 0.0)
    P[:, 6] = rng.uniform(-np.pi, np.pi, n)
    t = rng.uniform(0, 60, n)
    t[:8], P[:8, 6] = 0.0, [0.0, np.pi / 2, np.pi, -np.pi / 2, np.pi / 4, -np.pi / 4, 1e-9, -0.0]       # phases at the curve's special points
    gen, y0 = lem_both(lib, dt, P, t)
    assert np.isfinite(gen).all()
    assert (gen == y0).all(), np.argwhere(gen != y0)[:5]
    # p, v, a are not touched at all: the same bytes; yaw is +0 in both; yaw_rate is +-0 in the general form, +0 here
    assert gen[:, :10].tobytes() == y0[:, :10].tobytes()
    assert not y0[:, 9:].any() and not np.signbit(y0[:, 9:]).any()
    share = (gen.view(np.uint8).reshape(n, -1) == y0.view(np.uint8).reshape(n, -1)).all(axis=1).mean()
    print(f"{dt}: byte-equal rows {100 * share:.2f} % (the others: yaw_rate = -0 uploaded)")


@pytest.mark.parametrize("dt,tol_rpm_rel,tol_aux", [("f64", 1e-13, 1e-13), ("f32", 1e-6, 2e-6)])
def test_yaw_free_controller_against_the_numpy_oracle(lib, dt, tol_rpm_rel, tol_aux):
    """The gate of tests/test_emul_device_math.py::test_geometric_golden, on the golden observations with a planar, yaw-free desired state."""
    d = np.load(os.path.join(G, "geometric_compute.npz"))
    obs, des = d["obs"].copy(), d["des"].copy()
    des[:, [2, 5, 8, 9, 10]] = 0.0
    rpm = O.geometric_compute(obs, des[:, 0:3], des[:, 3:6], des[:, 6:9], des[:, 9], des[:, 10])
    force, w_des, R_des = O.geometric_compute(obs, des[:, 0:3], des[:, 3:6], des[:, 6:9], des[:, 9], des[:, 10], return_omegas=True)
    gen, y0 = geo_both(lib, dt, obs, des)
    _assert_contract(gen, y0)
    err = np.abs(y0[:, 0:4].astype(np.float64) / rpm - 1).max()
    print(f"{dt}: max relative RPM error against the oracle {err:.3e}")
    assert err < tol_rpm_rel
    assert np.abs(y0[:, 8] - force).max() < tol_aux
    assert np.abs(y0[:, 9:12] - w_des).max() < tol_aux * 5
    # b1d | b2d | b3d are the columns of R_des
    Rg = np.stack([y0[:, 12:15], y0[:, 15:18], y0[:, 18:21]], axis=-1).astype(np.float64)
    assert np.abs(Rg - R_des).max() < tol_aux


def test_stand_alone_comparison_under_address_and_undefined_sanitizers(tmp_path):
    """The same comparison as a host program with its own main (-DYAW_FREE_MAIN), built with -fsanitize=address,undefined and run
    as a program: it returns 0 when every output of the two forms is == and the sanitizers have nothing to report."""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "yaw_free_main")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-mfma", "-ffp-contract=fast", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-DYAW_FREE_MAIN", "-o", exe, SRC])
    env = dict(os.environ, UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1", ASAN_OPTIONS="detect_leaks=0:halt_on_error=1")   # as tests/emul/simt/simt.py
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert "0 unequal outputs" in r.stdout

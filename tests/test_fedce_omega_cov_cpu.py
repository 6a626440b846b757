"""The covariance form of the 9-state FedCE learner (theta_update, what simulations/CBFTest.py's fedCE_iteration calls) on the CPU: the
NumPy restatement (tests/fedce_omega_cov_oracle.py, real solve_ivp inside) against the reference-minted fixture
tests/golden/fedce_omega_cov_ref_in_loop.npz, and rls_cov_update of csrc/mds_fedce_omega.hpp compiled with g++ into a stand-alone
program (tests/emul/fedce_omega_cov_host.cpp) against the fixture's cov_unit and long blocks.  The program also runs once under
-fsanitize=address,undefined.  (rls_cov_update_row, the 16-lane split of the same arithmetic, is device code: tests/test_gpu_fedce_omega_cov.py.)

The trap: on the long phase phi^T P phi << 1 and theta_update2 gives the same theta to 1.7e-6 relative, so every gate below is
asserted to lie at least 100 x under the distance between the two forms on its block (the fixture's *_info_thetas).

Measured (float64, relative to the block's largest entry): restatement vs fixture theta 7.9e-18, P 5.4e-15, K 5.2e-14, V P - I
3.0e-15; on cov_unit theta 9.0e-19, P 6.7e-16; on the long phase theta 2.0e-19, P 1.2e-15.  Header rls_cov_update vs cov_unit theta
1.2e-18, P 1.1e-15, V W - I 1.1e-15; vs the long phase theta 9.4e-20, P 3.0e-15; rls2_update after rls_cov_update on one (theta, V, W)
vs the restatement theta 9.0e-19.  Distance between the forms: cov_unit 1.2e-3 (0.054 absolute), long 1.7e-6, d2 / d3 6.4e-4.
These are the yardstick for the GPU gates of tests/test_gpu_fedce_omega_cov.py."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import fedce_omega_cov_oracle as FC
from tests import fedce_omega_oracle as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "multidronesim_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "emul", "fedce_omega_cov_host.cpp")
NEW = ["mds_fedce_omega_get_cov"]
GATE = 1e-12                 # float64 chains of at most 99 rank-one updates at cond(P) <= 31: far above rounding, far below the forms' distance


def rel(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


@pytest.fixture(scope="module")
def fixture(golden_dir):
    return np.load(os.path.join(golden_dir, "fedce_omega_cov_ref_in_loop.npz"))


def _build(tmp, sanitize):
    exe = os.path.join(tmp, "fedce_omega_cov_host" + ("_san" if sanitize else ""))
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else ["-O2"]
    subprocess.check_call(["g++", "-std=c++17", *flags, "-ffp-contract=off", "-I", CSRC, "-o", exe, SRC])
    return exe


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to build the host program")
    return _build(str(tmp_path_factory.mktemp("fedce_omega_cov")), False)


def run(exe, form, phis, xtp1):
    """-> theta [n,D,13,9], W [n,D,13,13], V [n,D,13,13], (status, steps, nfev) [n,D,3]"""
    n, D = phis.shape[:2]
    th0 = np.hstack(F.lin_model()).T
    data = np.concatenate([[float(form), float(n), float(D)], th0.ravel(), np.concatenate([phis, xtp1], axis=2).ravel()]).tobytes()
    p = subprocess.run([exe], input=data, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    assert b"runtime error" not in p.stderr and b"ERROR" not in p.stderr, p.stderr.decode()[-2000:]
    out = np.frombuffer(p.stdout, dtype=np.float64).reshape(n, D, 117 + 169 + 169 + 3)
    return (out[..., :117].reshape(n, D, 13, 9), out[..., 117:286].reshape(n, D, 13, 13), out[..., 286:455].reshape(n, D, 13, 13),
            out[..., 455:])


def long_inputs(g):
    """(phi [99,D,13], x_tp1 [99,D,9]) of the long block's updates, from its recorded observations and inputs (update t uses step t + 1)."""
    D = g["u"].shape[1]
    mg = F.O.CF2P.M * F.O.CF2P.G
    x_des = np.hstack([g["rpy"], np.zeros((D, 3)), g["xyz"]])
    e = np.array([[F.error_state(F.lin_x(o[j]), x_des[j]) for j in range(D)] for o in g["obs_log"]])
    u = g["u"].copy()
    u[..., 0] = np.clip(u[..., 0], 0, None) - mg
    phis = np.concatenate([e[:-1], u], axis=2)
    return phis[1:], e[2:]


def block(fixture, name):
    return {k[len(name) + 1:]: fixture[k] for k in fixture.files if k.startswith(name + "_")}


def test_the_two_forms_are_apart_on_every_block_and_the_gate_is_far_below(fixture):
    """cov_unit: more than 1e-3 relative apart.  Every block: GATE at least 100 x below the distance between the forms."""
    d_unit = rel(fixture["cov_unit_info_thetas"], fixture["cov_unit_thetas"])
    d_long = rel(fixture["long_info_thetas"][-1], fixture["long_theta_updates"][-1])
    d_loop = [rel(fixture[f"d{D}_info_thetas"], fixture[f"d{D}_thetas"]) for D in (2, 3)]
    print(f"distance between theta_update and theta_update2: cov_unit {d_unit:.2e}, long (last update) {d_long:.2e}, d2 {d_loop[0]:.2e}, d3 {d_loop[1]:.2e}")
    assert d_unit > 1e-3
    assert abs(fixture["cov_unit_info_thetas"] - fixture["cov_unit_thetas"]).max() > 1e-2          # O(1) entries: absolute as well
    for d in (d_unit, d_long, *d_loop):
        assert GATE * 100 < d


@pytest.mark.parametrize("D", [2, 3])
def test_restatement_reproduces_the_fixture(fixture, D):
    g, noise, num_iter = FC.fixture_case(fixture, D)
    ora = FC.FedCEOmegaCov(g["xyz"], g["rpy"], g["target_pos"], g["target_rpy"]).run(num_iter, noise)
    print(f"D={D}: theta {rel(np.array(ora.thetas), g['thetas']):.2e} P {rel(np.array(ora.Ps), g['Ps']):.2e} "
          f"K {rel(np.array(ora.Ks), g['Ks']):.2e} obs {np.abs(np.array(ora.obs_log) - g['obs_log']).max():.2e} "
          f"V P - I {np.abs(ora.dlqr.V @ ora.dlqr.P - np.eye(13)).max():.2e}")
    assert rel(np.array(ora.updates), g["theta_updates"]) < GATE
    assert rel(np.array(ora.thetas), g["thetas"]) < GATE and rel(np.array(ora.Ps), g["Ps"]) < GATE
    assert rel(np.array(ora.Ks), g["Ks"]) < 1e-9
    np.testing.assert_allclose(np.array(ora.obs_log), g["obs_log"], atol=1e-12, rtol=1e-12)
    ivp = np.array(ora.dlqr.ivp).reshape(-1, D, 3)
    np.testing.assert_array_equal(ivp[..., 0], g["ivp_steps"])
    np.testing.assert_array_equal(ivp[..., 1], g["ivp_nfev"])
    assert np.abs(ora.dlqr.V @ ora.dlqr.P - np.eye(13)).max() < 1e-12        # the carried information matrix stays P's inverse


def test_restatement_reproduces_cov_unit_and_the_long_phase(fixture):
    u = block(fixture, "cov_unit")
    th, P, _ = FC.unit_chain(u["phis"], u["xtp1"])
    print(f"cov_unit: theta {rel(th, u['thetas']):.2e} P {rel(P, u['Ps']):.2e}")
    assert rel(th, u["thetas"]) < GATE and rel(P, u["Ps"]) < GATE
    g = block(fixture, "long")
    ora = FC.FedCEOmegaCov(g["xyz"], g["rpy"], g["xyz"], g["rpy"])
    obs = ora.step(np.zeros((2, 4)))
    ora._phase(obs, g["u"], np.hstack([g["rpy"], np.zeros((2, 3)), g["xyz"]]))
    print(f"long: theta {rel(np.array(ora.updates), g['theta_updates']):.2e} P {rel(ora.dlqr.P, g['P']):.2e}")
    assert rel(np.array(ora.updates), g["theta_updates"]) < GATE and rel(ora.dlqr.P, g["P"]) < GATE
    np.testing.assert_allclose(np.array(ora.obs_log), g["obs_log"], atol=1e-12, rtol=1e-12)


def test_header_rls_cov_update_reproduces_cov_unit(fixture, host):
    """theta and P = W after each of the 64 calls, solve_ivp's step counts, and V W = I for the carried pair."""
    u = block(fixture, "cov_unit")
    th, W, V, st = run(host, 0, u["phis"], u["xtp1"])
    pair = np.abs(V @ W - np.eye(13)).max()
    print(f"cov_unit: theta {rel(th, u['thetas']):.2e} (last {rel(th[-1], u['thetas'][-1]):.2e}) P {rel(W, u['Ps']):.2e} V W - I {pair:.2e}")
    assert (st[..., 0] == 0).all()
    np.testing.assert_array_equal(st[..., 1], u["ivp_steps"])
    np.testing.assert_array_equal(st[..., 2], u["ivp_nfev"])
    assert rel(th, u["thetas"]) < GATE and rel(W, u["Ps"]) < GATE
    assert rel(th, u["info_thetas"]) > 1e-3                  # and it is not the information form
    assert pair < 1e-12


def test_header_rls_cov_update_reproduces_the_long_phase(fixture, host):
    g = block(fixture, "long")
    phis, xtp1 = long_inputs(g)
    th, W, V, st = run(host, 0, phis, xtp1)
    e_th, e_P = rel(th, g["theta_updates"]), rel(W[-1], g["P"])
    apart = rel(g["info_thetas"][-1], g["theta_updates"][-1])
    print(f"long: theta per update {e_th:.2e}, P {e_P:.2e}, V W - I {np.abs(V[-1] @ W[-1] - np.eye(13)).max():.2e}; the forms are {apart:.2e} apart")
    assert (st[..., 0] == 0).all()
    np.testing.assert_array_equal(st[..., 1], g["ivp_steps"])
    assert e_th < GATE and e_P < GATE and GATE * 100 < apart
    assert np.abs(V[-1] @ W[-1] - np.eye(13)).max() < 1e-12


def test_header_information_form_after_a_covariance_phase(fixture, host):
    """32 theta_update calls, then 32 theta_update2 calls on the same (theta, V, W): the restatement inverts V afresh at every
    theta_update2 call, the header carries W through both forms."""
    u = block(fixture, "cov_unit")
    n = len(u["phis"])
    th, W, V, st = run(host, 1, u["phis"], u["xtp1"])
    dl = FC.unit_chain(u["phis"][:n // 2], u["xtp1"][:n // 2])[2]
    ref = []
    for t in range(n // 2, n):
        dl.theta_update_info(list(u["phis"][t]), list(u["xtp1"][t]))
        ref.append(dl.th.copy())
    e = rel(th[n // 2:], np.array(ref))
    print(f"theta_update2 after theta_update: theta {e:.2e}, V {rel(V[-1], dl.V):.2e}, V W - I {np.abs(V[-1] @ W[-1] - np.eye(13)).max():.2e}")
    assert (st[..., 0] == 0).all() and e < 1e-11 and rel(V[-1], dl.V) < 1e-14


def test_host_program_under_asan_ubsan(fixture, tmp_path):
    """The same arithmetic once under AddressSanitizer + UndefinedBehaviorSanitizer (a stand-alone program: nothing loaded into python
    is sanitized): cov_unit in both modes of the program."""
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to build the host program")
    exe = _build(str(tmp_path), True)
    u = block(fixture, "cov_unit")
    th, W, V, st = run(exe, 0, u["phis"], u["xtp1"])
    assert rel(th[-1], u["thetas"][-1]) < GATE and rel(W[-1], u["Ps"][-1]) < GATE
    th, W, V, st = run(exe, 1, u["phis"], u["xtp1"])
    assert (st[..., 0] == 0).all() and np.isfinite(th).all()


def test_capi_table_header_and_python_carry_the_new_names():
    from multidronesim_amd import _capi as capi
    from multidronesim_amd.control.dlqr import decentralized_lqr_omega as dlo
    header = open(os.path.join(ROOT, "include", "mds.h")).read()
    table = next(v for v in vars(capi).values() if isinstance(v, dict) and "mds_fedce_identify" in v)
    for name in NEW:
        assert name in table, name
        assert re.search(r"\bint " + name + r"\(", header), name
    assert (dlo.UPDATE_COV_ALL, dlo.UPDATE_COV_SKIP_FIRST) == (3, 4)
    assert "update 3 / 4" in header and "3 = DecentralizedLQROmega" in header
    with pytest.raises(NotImplementedError, match="identify\\(form="):
        dlo.DecentralizedLQROmega.theta_update(None, None, None)

"""The covariance form of the 9-state FedCE learner on the device (mds_fedce_omega_identify with update 3 / 4, rls_cov_update_row;
DecentralizedLQROmega.identify(form="theta_update"); simulations/CBFTest.py's fedCE) against the reference-minted fixture
tests/golden/fedce_omega_cov_ref_in_loop.npz and the float64 NumPy restatement tests/fedce_omega_cov_oracle.py.  Every comparison
prints its figure before it asserts.

The trap (tests/test_fedce_omega_cov_cpu.py): where phi^T P phi << 1 the information form gives the same theta to 1.7e-6, so every
theta gate here is at least 100 x below the distance between the forms on its block (asserted in `apart`), and test_cov_unit_* runs
regressors of O(0.3), where the forms are O(1) apart: that test fails with the old update.

Measured on the MI355X against the fixture, gated at the next round number above each figure:
                         float64 handle            float32 handle
  theta (relative)       1.0e-17 -> 1e-16          4.6e-10 -> 1e-9
  P = W (relative)       9.4e-15 -> 1e-14          8.3e-7  -> 1e-6
  V W - I                1.6e-15 -> 1e-14          2.0e-15 -> 1e-14      (both float64 on the device in every dtype)
  K (relative)           5.5e-14 -> 1e-13          2.9e-9  -> 1e-8
  observations           4.3e-13 -> 1e-12          1.8e-5  -> 1e-4       (|a - b| / (1 + |b|) over fedCE's 130 steps)
  one phase alone        1.1e-15 -> 1e-14          4.9e-7  -> 1e-6       (the warm-up and the long phase)
  cov_unit regressors (float64, against the restatement): theta 1.3e-18 -> 1e-17, P 1.2e-15 -> 1e-14.
  theta_update2 after theta_update on one handle (float64): theta 9.0e-19, W at the switch 1.7e-15, V 8.0e-16 -- the gates above.
The CPU restatement's own figures against the fixture are theta 7.9e-18, P 5.4e-15, K 5.2e-14: the float64 figures are within two
decades of them (theta and K at them).  float32 handles are limited by the fp32 physics feeding the float64 learner.  The status
plane is zero everywhere."""
import os

import numpy as np
import pytest

from oracle import np_oracle as O
from tests import fedce_omega_cov_oracle as FC
from tests import fedce_omega_oracle as F

pytestmark = pytest.mark.gpu
TOL = {"float64": dict(theta=1e-16, P=1e-14, K=1e-13, obs=1e-12, warm_obs=1e-14, pair=1e-14),
       "float32": dict(theta=1e-9, P=1e-6, K=1e-8, obs=1e-4, warm_obs=1e-6, pair=1e-14)}


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no HIP device")
    return torch


@pytest.fixture(scope="module")
def fixture(golden_dir):
    return np.load(os.path.join(golden_dir, "fedce_omega_cov_ref_in_loop.npz"))


def rel(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def apart(gate, cov, info):
    """the gate separates the forms: at least 100 x below the distance between theta_update's and theta_update2's result"""
    d = rel(info, cov)
    print(f"forms apart by {d:.2e}, gate {gate:.0e}")
    assert gate * 100 < d, (gate, d)


def make_geo(D, dtype="float64", E=1, controller="lqr", duration=1, g=None):
    """the CBFTest mirror with the fixture's poses (CBFTest.py:383-404: cos for x, sin for y)"""
    from multidronesim_amd.simulations import CBFTest as S
    args = S.parse_args(["--num_drones", str(D), "--dtype", dtype, "--num_envs", str(E), "--controller", controller,
                         "--duration_sec", str(duration)])
    geo = S.GeometricEnv(args, circle_init=True)
    if g is not None:
        geo.INIT_XYZS, geo.INIT_RPYS = g["xyz"].copy(), g["rpy"].copy()
        if "target_pos" in g:
            geo.TARGET_POSITIONS, geo.TARGET_RPYS = g["target_pos"].copy(), g["target_rpy"].copy()
    geo.create_env()
    return geo


def obs_close(a, b, tol, what=""):
    a, b = np.asarray(a, float), np.asarray(b, float)
    err = (np.abs(a - b) / (1 + np.abs(b))).max()
    print(f"{what} observation error {err:.2e}")
    assert err < tol, (what, err)


def pair_error(dl):
    """max |V W - I| over the drones: the handle's information matrix and covariance stay an inverse pair"""
    from multidronesim_amd import _capi as capi
    V, W = dl._get()[1], np.zeros((dl.env.n, 13, 13))
    capi.check(dl.env._lib.mds_fedce_omega_get_cov(dl.env._h, capi.as_double_ptr(W)), "mds_fedce_omega_get_cov")
    return np.abs(V @ W.reshape(V.shape) - np.eye(13)).max()


def block(fixture, name):
    return {k[len(name) + 1:]: fixture[k] for k in fixture.files if k.startswith(name + "_")}


@pytest.mark.parametrize("D,E,dtype", [(2, 1, "float64"), (3, 1, "float64"), (2, 9, "float64"), (2, 9, "float32")])
def test_identify_warmup_matches_the_fixture(gpu, fixture, D, E, dtype):
    """The fixture's warm-up phase in covariance form: theta after every update (theta_log_dev), P = W (mds_fedce_omega_get_cov),
    V W - I, the observation log, the status plane.  D = 3: 48 lanes, a partial wave.  E = 9: 18 drones, past the 16 drones of a
    workgroup; every env gets env 0's noise and must equal it bit for bit."""
    from multidronesim_amd.control import DecentralizedLQROmega
    from multidronesim_amd.control.dlqr.decentralized_lqr_omega import UPDATE_SKIP_FIRST
    import torch
    g, noise, _ = FC.fixture_case(fixture, D)
    geo = make_geo(D, dtype, E, g=g)
    env = geo.env
    dl = DecentralizedLQROmega(env, geo.linear_models)
    env.step(torch.zeros((E, D, 4), dtype=env.dtype, device=env.device))
    uw = np.repeat(noise[0][0][:, None], E, axis=1)
    x_des = np.hstack([geo.INIT_RPYS, np.zeros((D, 3)), geo.INIT_XYZS])
    log, obs, thl = dl.identify(uw, x_des, UPDATE_SKIP_FIRST, log_obs=True, log_theta=True, form="theta_update")
    log, thl = log.double().cpu().numpy(), thl.cpu().numpy()
    th = dl._get()[0]
    P = np.asarray(dl.P).reshape(E, D, 13, 13)
    assert (dl.status == 0).all()
    if E > 1:
        assert (thl == thl[:, :1]).all() and (log == log[:, :1]).all() and (P == P[:1]).all()
    tol = TOL[dtype]
    e_th, e_last, e_P, e_pair = rel(thl[1:, 0], g["theta_updates"][:24]), rel(th[0], g["theta_updates"][23]), rel(P[0], g["Ps"][0]), pair_error(dl)
    print(f"D={D} E={E} {dtype}: theta per update {e_th:.2e}, theta last {e_last:.2e}, P {e_P:.2e}, V W - I {e_pair:.2e}")
    obs_close(log[:, 0], g["obs_log"][1:26], tol["warm_obs"], f"D={D} E={E} {dtype}")
    apart(tol["theta"], g["thetas"][0], g["info_thetas"][0])
    assert e_th < tol["theta"] and e_last < tol["theta"]
    assert e_P < tol["P"] and e_pair < tol["pair"]           # the reference's P after iteration 0 has only the warm-up's updates (Texp = 0)


def unit_states(u, k):
    """cov_unit's regressors of call k as a state the kernel can start from: x_t = phi[:9] = [rpy, vel, pos] against x_des = 0, body
    rates 0, raw input phi[9:] + (M G, 0, 0, 0)"""
    phi = u["phis"][k]
    D = phi.shape[0]
    state = np.concatenate([phi[:, 6:9], O.quat_from_euler_bullet(phi[:, 0:3]), phi[:, 3:6], np.zeros((D, 3))], axis=1)
    uin = phi[:, 9:13].copy()
    uin[:, 0] += O.CF2P.M * O.CF2P.G
    return state, uin


def test_cov_unit_regressors_through_set_and_one_step_launches(gpu, fixture):
    """64 one-step launches (update 3: every step, covariance form) from states that realise cov_unit's regressors phi ~ N(0, 0.3):
    phi^T P phi is O(1) there and the two forms are O(1) apart, so this fails with rls2_update_row in the kernel.  x_tp1 is what the
    physics gives (a caller cannot choose it), so the expected values are the restatement's on the same states and inputs -- which
    tests/test_fedce_omega_cov_cpu.py pins to the fixture's cov_unit block.  Half way the learner state goes through
    mds_fedce_omega_set (theta and V = P^-1 of the restatement; the call inverts V on the host) and must continue the same chain."""
    from multidronesim_amd import _capi as capi
    from multidronesim_amd.control import DecentralizedLQROmega
    from multidronesim_amd.control.dlqr.decentralized_lqr_omega import UPDATE_ALL
    u = block(fixture, "cov_unit")
    n, D = u["phis"].shape[:2]
    geo = make_geo(D, "float64")
    env = geo.env
    dl = DecentralizedLQROmega(env, geo.linear_models)
    ora = O.AviaryOracle(np.zeros((D, 3)), np.zeros((D, 3)), O.CF2P, 100, 100)
    ref = FC.DLQROmegaCov(D).set_model(*F.lin_model())
    info = F.DLQROmega(D).set_model(*F.lin_model())
    x_des = np.zeros((D, 9))
    worst_th = worst_P = 0.0
    for k in range(n):
        state, uin = unit_states(u, k)
        env.set_state(state)
        ora.pos, ora.quat, ora.vel = state[:, 0:3].copy(), state[:, 3:7].copy(), state[:, 7:10].copy()
        ora.rates, ora.ang_v = np.zeros((D, 3)), np.zeros((D, 3))
        obs0 = ora.obs()
        e0 = [F.error_state(F.lin_x(obs0[j]), x_des[j]) for j in range(D)]
        uu = uin.copy()
        action = ref.compute_low_level(uu, obs0)
        uu[:, 0] -= O.CF2P.M * O.CF2P.G
        obs1 = ora.step(action)
        phis = [np.hstack([e0[j], uu[j]]) for j in range(D)]
        e1 = [F.error_state(F.lin_x(obs1[j]), x_des[j]) for j in range(D)]
        ref.theta_update(phis, e1)
        info.theta_update2(phis, e1)
        if k == n // 2:
            th_set = np.ascontiguousarray(th_dev)
            V_set = np.ascontiguousarray(np.linalg.inv(P_prev))
            capi.check(env._lib.mds_fedce_omega_set(env._h, capi.as_double_ptr(th_set), capi.as_double_ptr(V_set)), "mds_fedce_omega_set")
        dl.identify(uin[None, None], x_des, UPDATE_ALL, form="theta_update")
        th_dev = dl._get()[0][0]
        worst_th, worst_P = max(worst_th, rel(th_dev, ref.th)), max(worst_P, rel(dl.P, ref.P))
        P_prev = ref.P.copy()
    d = rel(info.th, ref.th)
    print(f"cov_unit regressors: theta {worst_th:.2e}, P {worst_P:.2e}, V W - I {pair_error(dl):.2e}; theta_update2 on the same inputs is {d:.2e} "
          f"(absolute {np.abs(info.th - ref.th).max():.2e}) away")
    assert (dl.status == 0).all()
    assert d > 1e-3 and np.abs(info.th - ref.th).max() > 1e-2
    assert worst_th < 1e-17 and worst_P < 1e-14 and pair_error(dl) < 1e-14


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_identify_long_phase_of_99_updates_matches_the_fixture(gpu, fixture, dtype):
    """The fixture's `long` block: 99 covariance-form updates in one launch against the reference's theta after every update, its P at
    the end and its observations.  Here the forms are only 1.7e-6 apart: the theta gates (1e-16 / 1e-9) are far below that."""
    import torch
    from multidronesim_amd.control import DecentralizedLQROmega
    from multidronesim_amd.control.dlqr.decentralized_lqr_omega import UPDATE_SKIP_FIRST
    g = block(fixture, "long")
    D = 2
    geo = make_geo(D, dtype, g=g)
    env = geo.env
    dl = DecentralizedLQROmega(env, geo.linear_models)
    env.step(torch.zeros((1, D, 4), dtype=env.dtype, device=env.device))
    x_des = np.hstack([g["rpy"], np.zeros((D, 3)), g["xyz"]])
    log, obs, thl = dl.identify(g["u"][:, None], x_des, UPDATE_SKIP_FIRST, log_obs=True, log_theta=True, form="theta_update")
    thl = thl.cpu().numpy()[1:, 0]
    assert thl.shape == g["theta_updates"].shape == (99, D, 13, 9) and (dl.status == 0).all()
    tol = TOL[dtype]
    e_th = max(rel(thl[k], g["theta_updates"][k]) for k in range(99))
    e_P, e_pair = rel(dl.P, g["P"]), pair_error(dl)
    print(f"long phase {dtype}: theta per update max {e_th:.2e} (last {rel(thl[-1], g['theta_updates'][-1]):.2e}), P {e_P:.2e}, V W - I {e_pair:.2e}")
    obs_close(log.double().cpu().numpy()[:, 0], g["obs_log"][1:], tol["warm_obs"], f"long phase {dtype}")
    apart(tol["theta"], g["theta_updates"][-1], g["info_thetas"][-1])
    assert e_th < tol["theta"] and e_P < tol["P"] and e_pair < tol["pair"]


@pytest.mark.parametrize("D,dtype", [(2, "float64"), (3, "float64"), (2, "float32")])
def test_cbftest_fedce_matches_the_reference_in_the_loop(gpu, fixture, D, dtype):
    """CBFTest.GeometricEnv.fedCE with the fixture's noise: theta, P and K after every iteration and every observation."""
    g, noise, num_iter = FC.fixture_case(fixture, D)
    geo = make_geo(D, dtype, g=g)
    K, theta = geo.fedCE(num_iter=num_iter, noise=[(None if uw is None else uw[:, None], ue[:, None]) for uw, ue in noise],
                         log_observations=True, log_iterations=True)
    tol = TOL[dtype]
    assert (geo.dLQR.status == 0).all()
    for n in range(num_iter):
        e = (rel(geo.fedce_thetas[n], g["thetas"][n]), rel(geo.fedce_Ps[n], g["Ps"][n]), rel(geo.fedce_Ks[n], g["Ks"][n]))
        print(f"D={D} {dtype} iteration {n}: theta {e[0]:.2e} P {e[1]:.2e} K {e[2]:.2e}")
        assert e[0] < tol["theta"] and e[1] < tol["P"] and e[2] < tol["K"], (n, e)
    apart(tol["theta"], g["thetas"], g["info_thetas"])
    obs = np.array(geo.fedce_observations)
    assert obs.shape == g["obs_log"].shape
    obs_close(obs, g["obs_log"], tol["obs"], f"D={D} {dtype}")


def test_information_form_phase_after_a_covariance_phase_on_one_handle(gpu, fixture):
    """The long block's inputs as two phases of 50 steps on one handle: theta_update, then theta_update2.  The kernel carries (V, W)
    through both; the restatement inverts V afresh at every theta_update2 call."""
    import torch
    from multidronesim_amd.control import DecentralizedLQROmega
    from multidronesim_amd.control.dlqr.decentralized_lqr_omega import UPDATE_SKIP_FIRST
    g = block(fixture, "long")
    D = 2
    x_des = np.hstack([g["rpy"], np.zeros((D, 3)), g["xyz"]])
    ora = FC.FedCEOmegaCov(g["xyz"], g["rpy"], g["xyz"], g["rpy"])
    obs = ora.step(np.zeros((D, 4)))
    obs = ora._phase(obs, g["u"][:50], x_des)
    ora_P_mid = ora.dlqr.P.copy()
    ora.dlqr.theta_update2 = ora.dlqr.theta_update_info
    ora._phase(obs, g["u"][50:], x_des)
    ref = np.array(ora.updates)
    geo = make_geo(D, "float64", g=g)
    env = geo.env
    dl = DecentralizedLQROmega(env, geo.linear_models)
    env.step(torch.zeros((1, D, 4), dtype=env.dtype, device=env.device))
    _, _, th1 = dl.identify(g["u"][:50, None], x_des, UPDATE_SKIP_FIRST, log_theta=True, form="theta_update")
    e_W = rel(dl.P, ora_P_mid)                              # P returns W after a covariance-form phase ...
    _, _, th2 = dl.identify(g["u"][50:, None], x_des, UPDATE_SKIP_FIRST, log_theta=True, form="theta_update2")
    got = np.concatenate([th1.cpu().numpy()[1:, 0], th2.cpu().numpy()[1:, 0]])
    e_th, e_V, e_pair = rel(got, ref), rel(dl.P, ora.dlqr.V), pair_error(dl)        # ... and V after an information-form phase
    print(f"theta_update2 after theta_update: theta per update {e_th:.2e}, W at the switch {e_W:.2e}, V {e_V:.2e}, V W - I {e_pair:.2e}")
    assert got.shape == ref.shape == (98, D, 13, 9) and (dl.status == 0).all()
    tol = TOL["float64"]
    assert e_th < tol["theta"] and e_W < tol["P"] and e_V < tol["P"] and e_pair < tol["pair"]

"""FedCE (GeometricEnv.fedCE) and the 'dlqr' controller on the device against the float64 NumPy restatement in
tests/fedce_oracle.py, driven with the same noise draws."""

import os

import numpy as np
import pytest

from oracle import np_oracle as O
from tests import fedce_oracle as F

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no HIP device")
    return torch


def rel(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def make_geo(D, dtype="float64", E=1, controller="lqr", duration=3):
    from multidronesim_amd.simulations import EnvGeometric as S
    args = S.parse_args(["--num_drones", str(D), "--dtype", dtype, "--num_envs", str(E), "--controller", controller,
                         "--duration_sec", str(duration)])
    geo = S.GeometricEnv(args, circle_init=True)
    geo.create_env()
    return geo


def oracle_for(geo):
    return F.FedCE(geo.INIT_XYZS, geo.INIT_RPYS, geo.TARGET_POSITIONS, geo.TARGET_RPYS)


def test_one_identification_step_matches_oracle(gpu):
    """Random states, P and theta: one warm-up step (raw u) and one exploration step (round-tripped u) in float64."""
    from multidronesim_amd import _capi as capi
    from multidronesim_amd.control import DecentralizedLQR
    from multidronesim_amd.control.dlqr.decentralized_lqr import U_RAW, U_ROUND_TRIP
    D = 4
    geo = make_geo(D)
    env = geo.env
    rng = np.random.default_rng(7)
    st = env.get_state().reshape(D, 13)
    st[:, 0:3] += rng.normal(0, .3, (D, 3))
    q = rng.normal(0, 1, (D, 4)) * [.1, .1, .5, 1]
    st[:, 3:7] = q / np.linalg.norm(q, axis=1, keepdims=True)
    st[:, 7:13] = rng.normal(0, .5, (D, 6))
    env.set_state(st)
    dl = DecentralizedLQR(env, geo.linear_models)
    M = rng.normal(0, 1, (D, 16, 16))
    P = np.ascontiguousarray(M @ M.transpose(0, 2, 1) + 5 * np.eye(16))
    th = np.ascontiguousarray(np.stack([np.hstack([m.Ahat, m.Bhat]).T for m in geo.linear_models]) * (1 + rng.normal(0, .1, (D, 16, 12))))
    capi.check(env._lib.mds_fedce_set(env._h, capi.as_double_ptr(th), capi.as_double_ptr(P)), "mds_fedce_set")
    x_des = rng.normal(0, .5, (D, 12))
    x_des[:, 3:5] = 0.0               # fedCE's x_des never has roll / pitch rates: the kernel reads the yaw rate x_des[5] only
    for mode in (U_RAW, U_ROUND_TRIP):
        th_proj, P0 = dl.theta.copy(), dl.P.copy()
        st = env.get_state().reshape(D, 13)
        obs0 = env._computeObs().double().cpu().numpy()[0]
        u = np.column_stack([rng.uniform(.8, 1.5, D) * O.CF2P.M * O.CF2P.G, rng.normal(0, 1e-5, (D, 3))])
        dl.pred_errors = [[] for _ in range(2 * D)]
        dl.pred_thetas = [[] for _ in range(D)]
        _, obs1 = dl.identify(u[None], mode, x_des, True)
        ref = F.DLQR(D)
        ref.theta, ref.P = th_proj.copy(), P0.copy()
        ora = O.AviaryOracle(st[:, 0:3], np.zeros((D, 3)), pyb_freq=100, ctrl_freq=100)
        ora.pos, ora.quat, ora.vel, ora.rates, ora.ang_v = st[:, 0:3], st[:, 3:7], st[:, 7:10], st[:, 10:13], obs0[:, 13:16]
        phis, acts = [], []
        for j in range(D):
            act = O.input_to_action(u[j], O.CF2P)
            if mode == U_RAW:
                uu = u[j].copy()
                uu[0] = max(uu[0], 0) - O.CF2P.M * O.CF2P.G
            else:
                uu = O.action_to_input(act, O.CF2P)
                uu[0] -= O.CF2P.M * O.CF2P.G
            phis.append(np.hstack([F.error_state(F.lin_x(obs0[j]), x_des[j]), uu]))
            acts.append(act)
        o1 = ora.step(np.array(acts))
        np.testing.assert_allclose(obs1.double().cpu().numpy()[0], o1, rtol=1e-12, atol=1e-12)
        ref.approx_theta_update(phis, [F.error_state(F.lin_x(o1[j]), x_des[j]) for j in range(D)], env.CTRL_TIMESTEP)
        assert rel(dl.theta, ref.theta) < 1e-12
        assert rel(dl.P, ref.P) < 1e-12
        assert rel(np.array(dl.pred_errors), np.array(ref.pred_errors)) < 1e-12


def run_fedce(D, num_iter, seed=11, **kw):
    geo = make_geo(D)
    np.random.seed(seed)
    noise = F.draw_reference_noise(num_iter, D)
    K, theta = geo.fedCE(num_iter=num_iter, noise=[(None if uw is None else uw[:, None], ue[:, None]) for uw, ue in noise],
                         log_observations=True, **kw)
    ora = oracle_for(geo).run(num_iter, noise)
    return geo, K, theta, ora


@pytest.mark.parametrize("D", [2, 3])
def test_fedce_matches_the_reference_in_the_loop(gpu, golden_dir, D):
    """GeometricEnv.fedCE with the noise of tests/golden/fedce_ref_in_loop.npz (the reference's DecentralizedLQR in the loop):
    theta and K of every iteration and sampled observations within 1e-9; D = 3 couples only drones 0 and 1."""
    d = np.load(os.path.join(golden_dir, "fedce_ref_in_loop.npz"))
    g, noise, num_iter = F.fixture_case(d, D)
    geo = make_geo(D)
    np.testing.assert_array_equal(geo.INIT_XYZS, g["xyz"])
    np.testing.assert_array_equal(geo.TARGET_POSITIONS, g["target_pos"])
    K, theta = geo.fedCE(num_iter=num_iter, noise=[(None if uw is None else uw[:, None], ue[:, None]) for uw, ue in noise],
                         log_observations=True, log_iterations=True)
    assert len(geo.fedce_thetas) == len(geo.fedce_Ks) == num_iter
    for n in range(num_iter):
        assert rel(geo.fedce_thetas[n], g["thetas"][n]) < 1e-9, n
        assert rel(geo.fedce_Ks[n], g["Ks"][n]) < 1e-9, n
    obs = np.array(geo.fedce_observations)
    assert obs.shape == g["obs_log"].shape
    for k in np.linspace(0, len(obs) - 1, 12).astype(int):
        np.testing.assert_allclose(obs[k], g["obs_log"][k], atol=1e-9, rtol=1e-9)
    if D == 3:      # only drones 0 and 1 are coupled by Q's cross terms
        assert max(np.abs(K[0:8, 24:36]).max(), np.abs(K[8:12, 0:24]).max()) < 1e-12 * np.abs(K).max()   # (ARE rounding only)
        assert np.abs(K[0:4, 12:24]).max() > 1e-6 * np.abs(K).max()


def test_fedce_lemniscate_ce_phase(gpu):
    """do_lemniscate=True: the CE phase tracks Lemniscate(center=[0, 0, .5], omega=1, yaw_rate=.1) from t = 0 and last_desired
    stays zero for the exploration phase."""
    D, num_iter = 2, 4
    geo = make_geo(D)
    np.random.seed(4)
    noise = F.draw_reference_noise(num_iter, D)
    geo.fedCE(num_iter=num_iter, noise=[(None if uw is None else uw[:, None], ue[:, None]) for uw, ue in noise], do_lemniscate=True,
              log_observations=True, log_iterations=True)
    ora = oracle_for(geo).run(num_iter, noise, do_lemniscate=True,
                              trajectory=lambda t: O.lemniscate(t, 1.0, 1.0, np.array([0, 0, .5]), .1, 0.0))
    for n in range(num_iter):
        assert rel(geo.fedce_thetas[n], ora.thetas[n]) < 1e-9, n
        assert rel(geo.fedce_Ks[n], ora.Ks[n]) < 1e-9, n
    np.testing.assert_allclose(np.array(geo.fedce_observations), np.array(ora.obs_log), atol=1e-9, rtol=1e-9)


def test_fedce_draws_the_reference_noise(gpu):
    """One env, no noise= argument: fedCE draws sigma1 / sigma_explore from the global np.random in the reference's order."""
    D, num_iter = 2, 3
    geo = make_geo(D)
    np.random.seed(21)
    K, theta = geo.fedCE(num_iter=num_iter, log_observations=True)
    np.random.seed(21)
    ora = oracle_for(geo).run(num_iter, F.draw_reference_noise(num_iter, D))
    assert rel(theta, ora.thetas[-1]) < 1e-9 and rel(K, ora.Ks[-1]) < 1e-9
    np.testing.assert_allclose(np.array(geo.fedce_observations), np.array(ora.obs_log), atol=1e-9, rtol=1e-9)


def test_approx_theta_update_matches_oracle(gpu):
    """DecentralizedLQR.approx_theta_update on caller-supplied phis / e_{t+1}: theta, P, pred_errors, pred_thetas."""
    from multidronesim_amd.control import DecentralizedLQR
    D = 3
    geo = make_geo(D)
    dl = DecentralizedLQR(geo.env, geo.linear_models)
    ref = F.DLQR(D)
    rng = np.random.default_rng(2)
    for _ in range(3):
        phis = rng.normal(0, .3, (D, 16))
        phis[:, 12] = rng.normal(0, .05, D)
        phis[:, 13:] = rng.normal(0, 1e-5, (D, 3))
        xtp1s = rng.normal(0, .3, (D, 12))
        dl.approx_theta_update(phis, xtp1s)
        ref.approx_theta_update(list(phis), list(xtp1s), geo.env.CTRL_TIMESTEP)
    assert rel(dl.theta, ref.theta) < 1e-13
    assert rel(dl.P, ref.P) < 1e-13
    assert rel(np.array(dl.pred_errors), np.array(ref.pred_errors)) < 1e-13
    assert rel(np.array(dl.pred_thetas), np.array(ref.pred_thetas)) < 1e-13


def per_env_noise(num_iter, E, D, device, seed=5):
    import torch
    g = torch.Generator(device=device)
    g.manual_seed(seed)
    mg = O.CF2P.M * O.CF2P.G
    out = []
    for n in range(num_iter):
        tw, _, texp = F.schedule(n)
        uw = ue = None
        if tw:
            r = torch.rand((tw, E, D, 4), dtype=torch.float64, device=device, generator=g)
            lo = torch.tensor([.8 * mg, -1e-5, -1e-5, -1e-5], dtype=torch.float64, device=device)
            uw = lo + (torch.tensor([1.5 * mg, 1e-5, 1e-5, 1e-5], dtype=torch.float64, device=device) - lo) * r
        if texp:                      # (as fedCE_iteration: no draw for an empty phase)
            z = torch.randn((texp, E, D, 4), dtype=torch.float64, device=device, generator=g)
            sd = torch.tensor([.15 * mg, .005 * O.CF2P.MAX_XY_TORQUE, .005 * O.CF2P.MAX_XY_TORQUE, .005 * O.CF2P.MAX_Z_TORQUE],
                              dtype=torch.float64, device=device)
            ue = torch.tensor([mg, 0, 0, 0], dtype=torch.float64, device=device) + sd * z
        else:
            ue = torch.zeros((0, E, D, 4), dtype=torch.float64, device=device)
        out.append((uw, ue))
    return out


def test_fedce_generator_gives_every_env_its_own_noise(gpu):
    """Several envs, generator=: DecentralizedLQR.draw_inputs draws every env's noise from the device generator; an env equals
    the oracle fed that env's slice of the same draws, and envs differ."""
    import torch
    E, D, num_iter = 64, 2, 3
    geo = make_geo(D, E=E)
    g = torch.Generator(device=geo.env.device)
    g.manual_seed(9)
    K, theta = geo.fedCE(num_iter=num_iter, generator=g)
    noise = per_env_noise(num_iter, E, D, geo.env.device, seed=9)
    assert np.abs(theta[1] - theta[0]).max() > 0
    for e in (0, 63):
        nz = [(None if uw is None else uw[:, e].cpu().numpy(), ue[:, e].cpu().numpy()) for uw, ue in noise]
        ora = oracle_for(geo).run(num_iter, nz)
        assert rel(theta[e], ora.thetas[-1]) < 1e-9 and rel(K[e], ora.Ks[-1]) < 1e-9


@pytest.mark.parametrize("dtype,tol", [("float64", 1e-9), ("float32", None)])
def test_fedce_batched_envs_match_oracle_per_env(gpu, dtype, tol):
    E, D, num_iter = 512, 2, 3
    geo = make_geo(D, dtype=dtype, E=E)
    noise = per_env_noise(num_iter, E, D, geo.env.device)
    K, theta = geo.fedCE(num_iter=num_iter, noise=noise, log_observations=True)
    obs = np.array(geo.fedce_observations)                    # [T, E, D, 20]
    assert theta.shape == (E, 32, 24) and K.shape == (E, 8, 24) and geo.dLQR.are_status.all()
    assert np.abs(theta[1] - theta[0]).max() > 0 and np.abs(obs[-1, 1] - obs[-1, 0]).max() > 0     # per-env noise
    errs = []
    for e in (0, 1, 77, 511):
        nz = [(None if uw is None else uw[:, e].cpu().numpy(), ue[:, e].cpu().numpy()) for uw, ue in noise]
        ora = oracle_for(geo).run(num_iter, nz)
        errs.append((rel(theta[e], ora.thetas[-1]), np.abs(obs[-1, e] - ora.obs_log[-1]).max()))
    errs = np.array(errs)
    if tol is not None:
        assert errs.max() < tol
    else:           # measured on MI355X (E = 512, 3 iterations): theta 9.8e-8 relative, final observation 4.7e-4 absolute
        assert errs[:, 0].max() < 1e-6 and errs[:, 1].max() < 2e-3


def lem_trajs(D):
    from multidronesim_amd.simulations import EnvGeometric as S
    return [S.Lemniscate(center=np.array([0, 0, .5]), omega=1.5, yaw_rate=0.0, phase_shift=(-np.pi / 4) * (num - 1)) for num in range(D)]


def ora_trajs(D):
    def mk(num):
        return lambda t: O.lemniscate(t, 1.0, 1.5, np.array([0, 0, .5]), 0.0, (-np.pi / 4) * (num - 1))
    return [mk(num) for num in range(D)]


def test_do_control_dlqr_with_fedce_gain(gpu):
    geo, K, theta, _ = run_fedce(2, 3)
    geo2 = make_geo(2, controller="dlqr", duration=3)
    geo2.do_control(trajs=lem_trajs(2), computed_K=K)
    obs = np.array(geo2.observations)
    ref = oracle_for(geo2).control(K, ora_trajs(2), 300)
    assert obs.shape == ref.shape == (300, 2, 20)
    for k in (0, 99, 299):
        np.testing.assert_allclose(obs[k], ref[k], atol=1e-9, rtol=1e-9)
    geo.create_env()                  # the gain of the last fedCE() on this GeometricEnv
    geo.args.controller = "dlqr"
    geo.do_control(trajs=lem_trajs(2))
    np.testing.assert_allclose(np.array(geo.observations)[-1], ref[-1], atol=1e-9, rtol=1e-9)


def test_do_control_dlqr_sixteen_drones(gpu):
    D = 16
    ref_dl = F.DLQR(D)
    ref_dl.compute_controller()
    K = ref_dl.K
    geo = make_geo(D, controller="dlqr", duration=1)
    geo.do_control(trajs=lem_trajs(D), computed_K=K)
    obs = np.array(geo.observations)
    ref = oracle_for(geo).control(K, ora_trajs(D), 100)
    for k in (0, 49, 99):
        np.testing.assert_allclose(obs[k], ref[k], atol=1e-9, rtol=1e-9)


def test_record_results_files(gpu, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    geo, K, theta, ora = run_fedce(2, 3, record_results=True)
    preds = np.load("predictions.npy")
    pe = np.load("pred_errors.npy")
    pt = np.load("pred_thetas.npy")
    assert preds.shape == (3, 2, 30)
    assert pe.shape == (4, 25 + 2 + 4) and pt.shape == (2, 31, 12, 16)
    np.testing.assert_allclose(preds[-1], F.features(ora.thetas[-1], 2), rtol=1e-9, atol=0)
    assert rel(pe, np.array(ora.dlqr.pred_errors)) < 1e-9
    assert rel(pt, np.array(ora.dlqr.pred_thetas)) < 1e-9

"""The device Riccati solver (mds_dlqr_solve_gain / mds_dlqr_omega_solve_gain, compute_controller(solver="device")) against scipy on
the full system, through the gain buffer the dLQR kernels read, with an unstabilisable env, with an unsupported Q, and inside fedCE.

Shapes: the 12-state model with D = 1 (no pair), 2 (the pair only), 3 (pair + single), the 9-state model with D = 1 and 3; E = 5 (a
partial last workgroup: four single-drone problems or one pair per workgroup) and, for the 9-state D = 3 case, E = 3 (nine problems:
one more than two workgroups).

Gates: K (float64 in every handle dtype) against scipy within the CPU sweep's gate (tests/test_care_cpu.py, 1e-12 relative to
max |K|); compute() after the device solve against compute() after upload_gain(scipy's K) within that gate x max |K| x |e|_1 in
float64 and within one float32 rounding of K (2^-23 max |K| |e|_1) in float32.  fedCE with riccati="device" against riccati="host"
(E = 4, D = 2, 3 iterations, float64), measured on MI355X: 12-state theta 0, K 1.6e-13, last observation 0; 9-state theta 1.4e-17,
K 6.0e-14, last observation 7.3e-12 absolute -> gates 1e-16 / 1e-12 / 1e-11 (the next power of ten over the larger of the two
models' figures).  Parity measured there: K against scipy 2.3e-14 .. 5.4e-14 over the cases below, 8 to 10 iterations; compute() in
float64 within 2.9e-13, in float32 bit for bit."""
import os

import numpy as np
import pytest
import scipy.linalg as la

from tests import fedce_omega_oracle as FO
from tests import fedce_oracle as F

pytestmark = pytest.mark.gpu

GATE = 1e-12                  # tests/test_care_cpu.py GATE_SWEEP
GATE_LOOP_THETA = 1e-16       # fedCE device against host (module docstring)
GATE_LOOP_K = 1e-12
GATE_LOOP_OBS = 1e-11


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no HIP device")
    return torch


def rel(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def make(model, D, E, dtype="float64"):
    """(geo, controller) of the 12- or 9-state model"""
    if model == 12:
        from multidronesim_amd.simulations import EnvGeometric as S
        from multidronesim_amd.control import DecentralizedLQR as Ctl
    else:
        from multidronesim_amd.simulations import EnvGeometricOmega as S
        from multidronesim_amd.control import DecentralizedLQROmega as Ctl
    args = S.parse_args(["--num_drones", str(D), "--dtype", dtype, "--num_envs", str(E), "--controller", "lqr", "--duration_sec", "1"])
    geo = S.GeometricEnv(args, circle_init=True)
    geo.create_env()
    return geo, Ctl(geo.env, geo.linear_models)


def thetas(model, E, D, golden_dir, seed):
    """[E, D, 16, 12] or [E, D, 13, 9]: the hover model with every free entry moved by 20-30 % (the 9-state ones also by a dense 1e-2),
    different for every drone and env; env 0 holds thetas the reference identified (the fixtures' iteration 1)."""
    rng = np.random.default_rng(seed)
    if model == 12:
        hover = np.hstack(F.lin_model()[2:]).T
        fx = np.load(os.path.join(golden_dir, "fedce_ref_in_loop.npz"))["d3_thetas"][1]
        fixture = [np.vstack([fx[12 * i:12 * (i + 1), 12 * i:12 * (i + 1)], fx[36 + 4 * i:36 + 4 * (i + 1), 12 * i:12 * (i + 1)]]) for i in range(3)]
    else:
        hover = np.hstack(FO.lin_model()).T
        fx = np.load(os.path.join(golden_dir, "fedce_omega_ref_in_loop.npz"))["d3_thetas"][1]
        fixture = [np.vstack([fx[9 * i:9 * (i + 1), 9 * i:9 * (i + 1)], fx[27 + 4 * i:27 + 4 * (i + 1), 9 * i:9 * (i + 1)]]) for i in range(3)]
    th = hover * (1 + rng.choice([-1.0, 1.0], (E, D) + hover.shape) * rng.uniform(.2, .3, (E, D) + hover.shape))
    if model == 12:
        th[..., 3:6, 0:3] = np.eye(3)          # the fixed entries of the projected theta
        th[..., 6:9, 9:12] = np.eye(3)
    else:
        th = th + 1e-2 * rng.normal(size=th.shape)
    for i in range(D):
        th[0, i] = fixture[i]
    return th


def set_thetas(ctl, model, th):
    from multidronesim_amd import _capi as capi
    env = ctl.env
    flat = np.ascontiguousarray(th.reshape((-1,) + th.shape[2:]))
    if model == 12:
        capi.check(env._lib.mds_fedce_set(env._h, capi.as_double_ptr(flat), None), "mds_fedce_set")
    else:
        capi.check(env._lib.mds_fedce_omega_set(env._h, capi.as_double_ptr(flat), None), "mds_fedce_omega_set")


def scipy_gains(ctl, model, th):
    E, D = th.shape[:2]
    out = []
    for e in range(E):
        A = la.block_diag(*[th[e, i, :model].T for i in range(D)])
        B = la.block_diag(*[th[e, i, model:].T for i in range(D)])
        P = la.solve_continuous_are(A, B, ctl.Q, ctl.R, e=None, s=None, balanced=True)
        out.append(la.solve(ctl.R, B.T @ P))
    return np.array(out)


def random_obs(E, D, seed):
    """-> (obs [E, D, 20], |e|_1 per env): the desired state is zero, so the error state is (rpy, [angular velocity,] vel, pos) itself"""
    rng = np.random.default_rng(seed)
    obs = np.zeros((E, D, 20))
    obs[..., 0:3] = rng.normal(0, .3, (E, D, 3))
    obs[..., 7:10] = rng.normal(0, .2, (E, D, 3))
    obs[..., 10:16] = rng.normal(0, .3, (E, D, 6))
    for e in range(E):
        for j in range(D):
            obs[e, j, 3:7] = F.Rotation.from_euler("xyz", obs[e, j, 7:10]).as_quat()
    return obs, np.abs(obs).sum(axis=(1, 2))


def compute_u(ctl, model, obs):
    return np.asarray(ctl.compute(obs)[1] if model == 12 else ctl.compute(obs, skip_low_level=True)[1]).reshape(obs.shape[0], -1)


CASES = [(12, 1, 5), (12, 2, 5), (12, 3, 5), (9, 1, 5), (9, 3, 5), (9, 3, 3)]


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("model,D,E", CASES)
def test_device_gain_matches_scipy_and_lands_where_the_kernels_read(gpu, golden_dir, model, D, E, dtype):
    geo, ctl = make(model, D, E, dtype)
    th = thetas(model, E, D, golden_dir, seed=100 * model + 10 * D + E)
    set_thetas(ctl, model, th)
    Kref = scipy_gains(ctl, model, th)
    ctl.compute_controller(solver="device", host_fallback=False)
    K = np.asarray(ctl.K).reshape(Kref.shape)
    err = max(rel(K[e], Kref[e]) for e in range(E))
    print(f"model {model} D {D} E {E} {dtype}: K vs scipy {err:.2e}, iterations {ctl.care_iters.min()}..{ctl.care_iters.max()}")
    assert (ctl.care_status == 0).all() and ctl.are_status.all()
    assert (ctl.care_iters > 0).all() and (ctl.care_iters < 32).all()
    assert err < GATE
    obs, e1 = random_obs(E, D, seed=3)
    u_dev = compute_u(ctl, model, obs)
    ctl.upload_gain(Kref)
    u_ref = compute_u(ctl, model, obs)
    bound = (GATE if dtype == "float64" else 2.0 ** -23) * np.abs(Kref).max(axis=(1, 2)) * e1
    diff = np.abs(u_dev - u_ref).max(axis=1)
    print(f"  compute(): max |du| {diff.max():.2e} (bound {bound.min():.2e}..{bound.max():.2e}), max |u| {np.abs(u_ref).max():.2e}")
    assert np.abs(u_ref).max() > 0 and (diff <= bound).all()
    geo.env.close()


def bad_theta(model, th, e):
    """drone 0 of env e gets the hover model without its thrust input: (A, B) is not stabilisable (scipy raises LinAlgError)"""
    if model == 12:
        th[e, 0] = np.hstack(F.lin_model()[2:]).T
        th[e, 0, 12, 8] = 0.0             # B[8, 0]
    else:
        th[e, 0] = np.hstack(FO.lin_model()).T
        th[e, 0, 9, 5] = 0.0              # B[5, 0]
    return th


@pytest.mark.parametrize("model", [12, 9])
def test_one_unstabilisable_env_out_of_five(gpu, golden_dir, model):
    E, D, bad = 5, 2, 2
    geo, ctl = make(model, D, E)
    obs, _ = random_obs(E, D, seed=4)
    good = thetas(model, E, D, golden_dir, seed=1)
    # a first call on a fresh handle: the flagged env has zeros, the others scipy's gain; the host cannot solve it either
    th = bad_theta(model, good.copy(), bad)
    set_thetas(ctl, model, th)
    with pytest.raises((np.linalg.LinAlgError, ValueError)):
        scipy_gains(ctl, model, th[bad:bad + 1])
    ctl.compute_controller(solver="device", host_fallback=True)
    ok = np.arange(E) != bad
    moved = ok & (np.arange(E) != 0)          # env 0 holds the fixture's thetas whatever the seed
    assert ctl.care_status[bad] != 0 and (ctl.care_status[ok] == 0).all()
    assert not ctl.are_status[bad] and ctl.are_status[ok].all()
    assert (ctl.K[bad] == 0).all()
    assert max(rel(ctl.K[e], k) for e, k in zip(np.flatnonzero(ok), scipy_gains(ctl, model, th[ok]))) < GATE
    zero = np.zeros_like(obs)
    zero[..., 3:7] = obs[..., 3:7]
    u0 = compute_u(ctl, model, obs)
    np.testing.assert_array_equal(u0[bad], compute_u(ctl, model, zero)[bad])      # a zero gain: the input does not see the state
    assert (u0[ok] != compute_u(ctl, model, zero)[ok]).any(axis=1).all()
    # every env solvable, then the same env unstabilisable again: it keeps the gain of the call before
    set_thetas(ctl, model, good)
    ctl.compute_controller(solver="device", host_fallback=False)
    assert ctl.are_status.all()
    K1, u1 = np.array(ctl.K), compute_u(ctl, model, obs)
    th2 = bad_theta(model, thetas(model, E, D, golden_dir, seed=2), bad)
    set_thetas(ctl, model, th2)
    ctl.compute_controller(solver="device", host_fallback=True)
    assert ctl.care_status[bad] != 0 and not ctl.are_status[bad] and ctl.are_status[ok].all()
    np.testing.assert_array_equal(ctl.K[bad], K1[bad])
    u2 = compute_u(ctl, model, obs)
    np.testing.assert_array_equal(u2[bad], u1[bad])
    assert (u2[moved] != u1[moved]).any(axis=1).all()
    assert max(rel(ctl.K[e], k) for e, k in zip(np.flatnonzero(ok), scipy_gains(ctl, model, th2[ok]))) < GATE
    geo.env.close()


@pytest.mark.parametrize("model", [12, 9])
@pytest.mark.parametrize("host_fallback", [True, False])
def test_one_env_failure_raises(gpu, golden_dir, model, host_fallback):
    geo, ctl = make(model, 2, 1)
    set_thetas(ctl, model, bad_theta(model, thetas(model, 1, 2, golden_dir, seed=1), 0))
    with pytest.raises(np.linalg.LinAlgError):
        ctl.compute_controller(solver="device", host_fallback=host_fallback)
    geo.env.close()


def test_q_that_couples_three_drones_is_unsupported(gpu, golden_dir):
    from multidronesim_amd import _capi as capi
    E, D = 2, 3
    geo, ctl = make(12, D, E)
    set_thetas(ctl, 12, thetas(12, E, D, golden_dir, seed=1))
    ctl.compute_controller(solver="device")
    obs, _ = random_obs(E, D, seed=5)
    K0, u0 = np.array(ctl.K), compute_u(ctl, 12, obs)
    ctl.Q[21:23, 33:35] = ctl.Q[33:35, 21:23] = -50.0              # drone 1 with drone 2, on top of 0 with 1
    with pytest.raises(capi.MdsError) as exc:
        ctl.compute_controller(solver="device")
    assert exc.value.status == -6 and "0 1 2" in str(exc.value)
    np.testing.assert_array_equal(ctl.K, K0)
    np.testing.assert_array_equal(compute_u(ctl, 12, obs), u0)
    geo.env.close()


def test_not_initialised_is_estate(gpu):
    import ctypes as C
    from multidronesim_amd import _capi as capi
    from multidronesim_amd.simulations import EnvGeometric as S
    geo = S.GeometricEnv(S.parse_args(["--num_drones", "2", "--dtype", "float64", "--controller", "lqr", "--duration_sec", "1"]), circle_init=True)
    geo.create_env()
    Q, R = np.eye(24), np.eye(8)
    st = gpu.zeros(1, dtype=gpu.int32, device=geo.env.device)
    for fn in (geo.env._lib.mds_dlqr_solve_gain, geo.env._lib.mds_dlqr_omega_solve_gain):
        assert fn(geo.env._h, capi.as_double_ptr(Q), capi.as_double_ptr(R), 0, None, C.c_void_p(st.data_ptr()), None, None) == -5
    geo.env.close()


@pytest.mark.parametrize("model", [12, 9])
def test_fedce_with_the_device_solver_equals_the_host_path(gpu, model):
    """fedCE(num_iter=3) on E = 4, D = 2 in float64 with the same generator seed: theta, K and the last observations."""
    out = {}
    for riccati in ("host", "device"):
        geo, _ = make(model, 2, 4)
        g = gpu.Generator(device=geo.env.device)
        g.manual_seed(17)
        K, theta = geo.fedCE(num_iter=3, generator=g, log_observations=True, riccati=riccati)
        assert geo.dLQR.are_status.all()
        if riccati == "device":
            assert (geo.dLQR.care_status == 0).all()
        last = geo.fedce_observations[-1]
        last = last.double().cpu().numpy() if hasattr(last, "cpu") else np.asarray(last, float)
        out[riccati] = (np.array(theta), np.array(K), last)
    (th_h, K_h, o_h), (th_d, K_d, o_d) = out["host"], out["device"]
    assert K_h.shape == (4, 8, 2 * model) and np.abs(K_h[1] - K_h[0]).max() > 0
    e_th, e_K, e_o = rel(th_d, th_h), rel(K_d, K_h), np.abs(o_d - o_h).max()
    print(f"model {model}: fedCE device vs host: theta {e_th:.2e}, K {e_K:.2e}, last observation {e_o:.2e}")
    assert e_th < GATE_LOOP_THETA and e_K < GATE_LOOP_K and e_o < GATE_LOOP_OBS

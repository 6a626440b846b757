"""The coupled dLQR (DecentralizedLQROmega) as the nominal controller of the CBF-filtered step: mds_cbf_set_nominal(h, 3),
k_cbf_nominal_dlqr_omega, served by mds_step_cbf_geometric / mds_rollout_cbf_geometric in their QP launch + low-level launch form --
simulations/CBFTest.py:303-350 with ``args.controller == 'dlqr'``.  Against the reference-minted fixture
tests/golden/cbf_dlqr_ref_in_loop.npz (reference: DecentralizedLQROmega, Lemniscate, ThrustOmegaController; oracle: ECBF rows, QP, DYN
step) and, beyond its shapes, against a test-side composition of tests/fedce_omega_oracle.py's compute, np_oracle.cbf_filter and
np_oracle.ThrustOmegaOracle.  Every comparison prints its figure before it asserts.

D = 1 is the reference's own semantics.  For D > 1 the reference's :348 indexes its one-element ``ctrl`` list with j and raises;
fixture and device do what ``ctrl[0]`` evidently stands for (modelled).

Measured on the MI355X, gated at the next round number above each figure (|a - b| / (1 + |b|) over the observations, absolute on
u_hat / u_safe, which are O(0.1)):
                                   float64                float32
  fixture, 300 steps: observations 9.0e-15 -> 1e-14       3.1e-6 -> 1e-5
                      u_hat        5.9e-15 -> 1e-14       1.6e-6 -> 1e-5
                      u_safe       4.3e-15 -> 1e-14       1.6e-6 -> 1e-5
  (3, 86) / (16, 2), 20 steps      1.5e-14 -> 1e-13       4.5e-6 -> 1e-5       (observations)
Where cap_u clips, u_hat[0] + M G is the bound to 1.4e-17 (-> 1e-16).  Statuses equal at every step everywhere; the scenes have no
infeasible step."""
import os

import numpy as np
import pytest

from oracle import np_oracle as O
from tests import fedce_omega_oracle as F

pytestmark = pytest.mark.gpu
MG_ = O.CF2P.M * O.CF2P.G
LO, HI = 4 * (9440.3 ** 2 * O.CF2P.KF), O.CF2P.MAX_THRUST
TOL = {"float64": dict(obs=1e-14, u=1e-14, beyond=1e-13), "float32": dict(obs=1e-5, u=1e-5, beyond=1e-5)}
MDS_ESTATE, MDS_EUNSUPPORTED = -5, -6
START_DZ = 0.04


@pytest.fixture(scope="module")
def mds():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no HIP device")
    from multidronesim_amd.envs.CtrlAviary import CtrlAviary, DroneModel, Physics
    from multidronesim_amd.cbf.cbf import DroneCBF
    from multidronesim_amd.cbf.qptracker import DroneQPTracker
    from multidronesim_amd.control import DecentralizedLQROmega
    from multidronesim_amd.model.linear_omega import LinearizedOmegaModel
    from multidronesim_amd.model.linear_yank_omega import LinearizedYankOmegaModel
    from multidronesim_amd._capi import MdsError
    import types
    return types.SimpleNamespace(**locals())


@pytest.fixture(scope="module")
def fixture(golden_dir):
    return np.load(os.path.join(golden_dir, "cbf_dlqr_ref_in_loop.npz"))


def block(fixture, name):
    return {k[len(name) + 1:]: fixture[k] for k in fixture.files if k.startswith(name + "_")}


def obs_err(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return (np.abs(a - b) / (1 + np.abs(b))).max()


def make(mds, xyz, rpy, P, K, dtype, nominal=True, order=2):
    """env + gain + tracker; xyz / rpy / P [E, D, .], K [4D, 9D] or [E, 4D, 9D] or None"""
    E, D = xyz.shape[:2]
    env = mds.CtrlAviary(drone_model=mds.DroneModel.CF2P, num_drones=D, initial_xyzs=xyz, initial_rpys=rpy, physics=mds.Physics.DYN,
                         pyb_freq=100, ctrl_freq=100, num_envs=E, dtype=dtype)
    env.set_trajectories(P)
    if K is not None:
        dl = mds.DecentralizedLQROmega(env, [mds.LinearizedOmegaModel(env) for _ in range(D)])
        dl.upload_gain(K)
    if nominal:
        env.set_cbf_nominal("dlqr_omega")
    if order == 2:
        cbf = mds.DroneCBF(env, [mds.LinearizedOmegaModel(env) for _ in range(D)], safety_radius=0.1, zscale=1.0, order=2)
        trk = mds.DroneQPTracker(cbf, num_robots=D, xdim=9, env=env)
    else:
        cbf = mds.DroneCBF(env, [mds.LinearizedYankOmegaModel(env) for _ in range(D)], safety_radius=0.125, zscale=2, order=3,
                           cbf_poles=np.array([-3.0, -3.6, -5.6]))
        trk = mds.DroneQPTracker(cbf, num_robots=D, xdim=10, env=env, order=3)
    return env, cbf, trk


_RUNS = {}


def fixture_run(mds, fixture, D, dtype):
    """the fixture's 300 steps through mds_step_cbf_geometric, once per (D, dtype): obs, u_hat, u_safe, status per step"""
    if (D, dtype) not in _RUNS:
        g = block(fixture, f"d{D}")
        x_obs, obs_r = [g["x_obs"][0]], list(g["obs_r"])
        env, cbf, trk = make(mds, g["xyz"][None], g["rpy"][None], g["lem"][None], g["K"], dtype)
        o0, *_ = env.step(mds.torch.zeros((1, D, 4), dtype=env.dtype))
        obs, un, us, st = [o0.double().cpu().numpy()[0].copy()], [], [], []
        t = 0.0
        for k in range(len(g["status"])):
            o, s = env.step_cbf_geometric(t, trk, x_obs, obs_r)
            a, b = env.cbf_step_inputs()
            obs.append(o.double().cpu().numpy()[0].copy())
            un.append(a.double().cpu().numpy()[0])
            us.append(b.double().cpu().numpy()[0])
            st.append(int(s.cpu().numpy()[0]))
            t += env.CTRL_TIMESTEP
        assert env.cbf_last_step_kernel() == 0
        env.close()
        _RUNS[(D, dtype)] = (g, np.array(obs), np.array(un), np.array(us), np.array(st))
    return _RUNS[(D, dtype)]


@pytest.mark.parametrize("D,dtype", [(1, "float64"), (3, "float64"), (1, "float32"), (3, "float32")])
def test_step_cbf_with_the_dlqr_nominal_matches_the_fixture(mds, fixture, D, dtype):
    """All 300 steps: statuses equal at every step, observations, the nominal input the filter saw and the filter's output."""
    g, obs, un, us, st = fixture_run(mds, fixture, D, dtype)
    hat = g["u_nom"] - np.array([MG_, 0, 0, 0])
    e_o, e_n, e_s = obs_err(obs, g["obs_log"]), np.abs(un - hat).max(), np.abs(us - g["u_safe"]).max()
    print(f"D={D} {dtype}: observations {e_o:.2e}, u_hat {e_n:.2e}, u_safe {e_s:.2e}; the filter changes u on "
          f"{int((np.abs(us - un).max(axis=(1, 2)) > 1e-6).sum())} steps")
    np.testing.assert_array_equal(st, g["status"])
    tol = TOL[dtype]
    assert e_o < tol["obs"] and e_n < tol["u"] and e_s < tol["u"]
    assert (np.abs(us - un).max(axis=(1, 2)) > 1e-6).sum() >= 50          # the filter is not idle


@pytest.mark.parametrize("D", [1, 3])
def test_the_thrust_entering_the_filter_is_the_capped_one(mds, fixture, D):
    """Where the fixture's cap_u clips, u_hat[0] + M G sits on the bound (4 x 9440.3^2 KF or MAX_THRUST) -- the uncapped thrust, which
    the unfiltered loop hands its low level, lies beyond it (the restatement's uncapped value is printed)."""
    g, obs, un, us, st = fixture_run(mds, fixture, D, "float64")
    clip = g["clipped"]
    assert clip.sum() >= 20
    thrust = un[..., 0] + MG_
    bound = np.where(np.abs(g["u_nom"][..., 0] - LO) < np.abs(g["u_nom"][..., 0] - HI), LO, HI)
    dl = F.DLQROmega(D).set_model(*F.lin_model())
    dl.K = g["K"]
    beyond = []
    for k in np.flatnonzero(clip.any(axis=1))[:10]:
        pos, vel, acc, yaw, yd = O.lemniscate(k * 0.01, g["lem"][:, 0], g["lem"][:, 1], g["lem"][:, 2:5], g["lem"][:, 5], g["lem"][:, 6])
        dl.des = np.hstack([pos, vel, yaw[:, None]])
        cap, dl.cap_u = dl.cap_u, (lambda u: u)
        _, raw = dl.compute(g["obs_log"][k], skip_low_level=True)
        dl.cap_u = cap
        beyond.append(np.abs(raw[clip[k], 0] - bound[k][clip[k]]).min())
    print(f"D={D}: {int(clip.sum())} clipped drone-steps, |thrust - bound| there {np.abs(thrust[clip] - bound[clip]).max():.2e}; "
          f"the uncapped thrust is {min(beyond):.2e} .. {max(beyond):.2e} beyond the bound on the first clipped steps")
    assert np.abs(thrust[clip] - bound[clip]).max() < 1e-16
    assert ((thrust >= LO - 1e-16) & (thrust <= HI + 1e-16)).all()
    assert max(beyond) > 1e-3


def scene(E, D, seed=5):
    """Beyond the fixture: every env its own phase and gain, stacked Lemniscates 0.15 m apart, drones started 0.04 m below / on / above
    their paths (both bounds of cap_u are met), one sphere next to drone 0's path; the gain has non-zero off-diagonal blocks (random, 1 % of
    the diagonal blocks' scale) and differs from env to env."""
    rng = np.random.default_rng(seed)
    P = np.zeros((E, D, 7))
    P[..., 0], P[..., 1] = 1.0, 0.5
    P[..., 4] = 0.5 + 0.15 * np.arange(D)
    P[..., 6] = 0.02 * np.arange(E)[:, None]
    Pf = P.reshape(-1, 7)
    pos, *_ = O.lemniscate(0.0, Pf[:, 0], Pf[:, 1], Pf[:, 2:5], Pf[:, 5], Pf[:, 6])
    xyz = pos.reshape(E, D, 3).copy()
    xyz[..., 2] += START_DZ * np.array([-1.0, 0.0, 1.0, 0.0])[np.arange(D) % 4]       # neighbours stay more than the safety radius apart
    near, *_ = O.lemniscate(0.3, P[0, :1, 0], P[0, :1, 1], P[0, :1, 2:5], P[0, :1, 5], P[0, :1, 6])
    x_obs, obs_r = [np.array([near[0] - [0, 0, .15], [0, 0, 0]])], [0.1]
    dl = F.DLQROmega(D).set_model(*F.lin_model())
    dl.compute_controller()
    K = np.repeat(dl.K[None], E, axis=0)
    diag = np.abs(dl.K[:4, :9])
    for a in range(D):
        for b in range(D):
            if a != b:
                K[:, 4 * a:4 * a + 4, 9 * b:9 * b + 9] = 0.01 * diag * rng.uniform(-1, 1, (E, 4, 9))
    K *= (1 + 0.02 * np.arange(E) / E)[:, None, None]
    return xyz, np.zeros((E, D, 3)), P, K, x_obs, obs_r


def oracle_loop(xyz, rpy, P, K, x_obs, obs_r, steps, Kcbf, umax):
    """CBFTest.py:303-350 with 'dlqr' on the oracle, env by env -> (obs [steps, E, D, 20], status [steps, E], clipped drone-steps)"""
    E, D = xyz.shape[:2]
    obs_out, st_out, clipped = np.zeros((steps, E, D, 20)), np.zeros((steps, E), dtype=int), 0
    for e in range(E):
        ora = O.AviaryOracle(xyz[e], rpy[e], O.CF2P, 100, 100)
        dl = F.DLQROmega(D).set_model(*F.lin_model())
        dl.K = K[e]
        obs = ora.step(np.zeros((D, 4)))
        t = 0.0
        for k in range(steps):
            pos, vel, acc, yaw, yd = O.lemniscate(t, P[e, :, 0], P[e, :, 1], P[e, :, 2:5], P[e, :, 5], P[e, :, 6])
            dl.des = np.hstack([pos, vel, yaw[:, None]])
            _, u = dl.compute(obs, skip_low_level=True)
            clipped += int(((u[:, 0] == LO) | (u[:, 0] == HI)).sum())
            u[:, 0] -= MG_
            xdes = np.concatenate([np.zeros((D, 2)), yaw[:, None], vel, pos], axis=1)
            us, st_out[k, e] = O.cbf_filter(O.obs_to_lin_model(obs, 9), xdes, u, 2, Kcbf, umax, 0.1, 1.0, O.CF2P, np.array(x_obs), obs_r)
            us = us.copy()
            us[:, 0] += MG_
            obs = ora.step(dl.low.compute_low_level(us, obs, ora.CTRL_TIMESTEP))
            obs_out[k, e] = obs
            t += ora.CTRL_TIMESTEP
    return obs_out, st_out, clipped


_ORACLE = {}


def oracle_case(D, E, steps, Kcbf, umax):
    if (D, E) not in _ORACLE:
        sc = scene(E, D)
        _ORACLE[(D, E)] = (sc, oracle_loop(*sc, steps, Kcbf, umax))
    return _ORACLE[(D, E)]


@pytest.mark.parametrize("D,E", [(3, 86), (16, 2)])
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_shapes_beyond_the_fixture_match_the_oracle_composition(mds, D, E, dtype):
    """(3, 86): 258 drones, 85 whole envs per workgroup, a second, partial workgroup; (16, 2): the widest env.  20 steps.  The gain
    couples the drones of an env (off-diagonal blocks at 1 % of the diagonal ones) and differs per env, so a kernel that ignores the
    coupling, sums in the wrong env or reads another env's gain fails: what the coupling does to a velocity within one step is more
    than 100 x the gate (printed)."""
    steps = 20
    xyz, rpy, P, K, x_obs, obs_r = scene(E, D)
    env, cbf, trk = make(mds, xyz, rpy, P, K, dtype)
    (_, (ref_obs, ref_st, clipped)) = oracle_case(D, E, steps, cbf.Kcbf.reshape(-1), cbf.umax)
    env.step(mds.torch.zeros((E, D, 4), dtype=env.dtype))
    t, worst = 0.0, 0.0
    for k in range(steps):
        o, st = env.step_cbf_geometric(t, trk, x_obs, obs_r)
        np.testing.assert_array_equal(st.cpu().numpy(), ref_st[k])
        worst = max(worst, obs_err(o.double().cpu().numpy(), ref_obs[k]))
        t += env.CTRL_TIMESTEP
    assert env.cbf_last_step_kernel() == 0
    env.close()
    Kd = K.copy()
    for a in range(D):
        for b in range(D):
            if a != b:
                Kd[:, 4 * a:4 * a + 4, 9 * b:9 * b + 9] = 0
    # what the off-diagonal position gains do to the thrust at the start offset, as the velocity it adds within one step
    coupling = np.abs(K - Kd)[..., 6:9].max() * START_DZ / O.CF2P.M * 0.01
    print(f"D={D} E={E} {dtype}: observations {worst:.2e} over {steps} steps, statuses equal, {clipped} clipped drone-steps, "
          f"infeasible env-steps {int(ref_st.sum())}, the coupling moves a velocity by up to {coupling:.2e} per step")
    assert clipped > 0 and coupling > 100 * TOL[dtype]["beyond"]
    assert worst < TOL[dtype]["beyond"]


@pytest.mark.parametrize("D,E", [(3, 86), (16, 32)])
def test_rollout_on_two_streams_equals_one_stream_and_the_step_loop(mds, D, E):
    """mds_rollout_cbf_geometric with set_rollout_streams(2) forced, with one stream, and the step loop: bit-equal.  At (3, 86) no env
    boundary falls on a 256-drone batch, so the library keeps one chain (asserted: nothing else is claimed); at (16, 32) the halves
    are envs [0, 16) and [16, 32) and the nominal kernel runs per EnvRange on two streams."""
    steps = 12
    xyz, rpy, P, K, x_obs, obs_r = scene(E, D)
    out = {}
    for mode in ("loop", 1, 2):
        env, cbf, trk = make(mds, xyz, rpy, P, K, "float64")
        env.step(mds.torch.zeros((E, D, 4), dtype=env.dtype))
        if mode == "loop":
            t = 0.0
            for k in range(steps):
                o, st = env.step_cbf_geometric(t, trk, x_obs, obs_r)
                t += env.CTRL_TIMESTEP
        else:
            env.set_rollout_streams(mode)
            o, st = env.rollout_cbf_geometric(0.0, steps, trk, x_obs, obs_r)
            assert env.last_rollout_streams() == (2 if (mode == 2 and (E // 2 * D) % 256 == 0) else 1)
        assert env.cbf_last_step_kernel() == 0
        out[mode] = (o.double().cpu().numpy().copy(), st.cpu().numpy().copy(), env.get_state())
        env.close()
    for mode in (1, 2):
        np.testing.assert_array_equal(out[mode][0], out["loop"][0])
        np.testing.assert_array_equal(out[mode][1], out["loop"][1])
        np.testing.assert_array_equal(out[mode][2], out["loop"][2])


def test_refusals(mds, fixture):
    g = block(fixture, "d3")
    xyz, rpy, P = g["xyz"][None], g["rpy"][None], g["lem"][None]
    x_obs, obs_r = [g["x_obs"][0]], list(g["obs_r"])
    # no gain: MDS_ESTATE
    env, cbf, trk = make(mds, xyz, rpy, P, None, "float64", nominal=False)
    with pytest.raises(mds.MdsError) as exc:
        env.set_cbf_nominal("dlqr_omega")
    assert exc.value.status == MDS_ESTATE
    env.close()
    # the persistent rollout and the unfiltered nominal calls do not serve it
    env, cbf, trk = make(mds, xyz, rpy, P, g["K"], "float64")
    env.step(mds.torch.zeros((1, 3, 4), dtype=env.dtype))
    with pytest.raises(mds.MdsError) as exc:
        env.rollout_cbf_geometric_fused(0.0, 4, trk, x_obs, obs_r)
    assert exc.value.status == MDS_EUNSUPPORTED
    with pytest.raises(mds.MdsError) as exc:
        env.step_nominal(0.0)
    assert exc.value.status == MDS_ESTATE
    env.set_cbf_step_kernel(2)                               # the persistent form asked for: the step loop serves nominal 3 all the same
    o, st = env.step_cbf_geometric(0.0, trk, x_obs, obs_r)
    assert env.cbf_last_step_kernel() == 0 and np.isfinite(o.double().cpu().numpy()).all()
    env.close()
    # an order-3 CBF: MDS_EUNSUPPORTED
    env, cbf, trk = make(mds, xyz, rpy, P, g["K"], "float64", order=3)
    env.step(mds.torch.zeros((1, 3, 4), dtype=env.dtype))
    with pytest.raises(mds.MdsError) as exc:
        env.step_cbf_geometric(0.0, trk, None, None)
    assert exc.value.status == MDS_EUNSUPPORTED
    env.close()


def mirror(D, duration=2):
    from multidronesim_amd.simulations import CBFTest as S
    args = S.parse_args(["--num_drones", str(D), "--dtype", "float64", "--duration_sec", str(duration)])
    return S, S.GeometricEnv(args, circle_init=True)


def test_cbftest_mirror_fedce_then_dlqr_control(mds):
    """simulations/CBFTest.py's tail (:435-449) at D = 2, 2 s: fedCE(num_iter=3), then 'dlqr' do_control -- with a tracker on the
    fixture's kind of scene (statuses logged, the QP launch + low-level launch form), and without one on a CompoundTrajectory (one
    launch, finite [T, D, 20] observations).  'dlqr' without any gain asks for one."""
    np.random.seed(4)
    S, geo = mirror(2)
    geo.create_env()
    geo.args.controller = 'dlqr'
    with pytest.raises(NotImplementedError, match="needs a gain"):
        geo.do_control(trajs=None)
    geo.args.controller = 'lqr'
    K, theta = geo.fedCE(num_iter=3)
    assert K.shape == (8, 18) and theta.shape == (26, 18) and (geo.dLQR.status == 0).all()
    geo.args.controller = 'dlqr'
    trajs = [S.Lemniscate(a=1, omega=.5, center=np.array([0, 0, .5 + .15 * j]), yaw_rate=0, phase_shift=0) for j in range(2)]
    geo.INIT_XYZS = np.array([np.asarray(tr(0.0)[0], dtype=float) for tr in trajs])
    env = geo.create_env()
    cbf = S.DroneCBF(env, geo.linear_models, safety_radius=0.1, zscale=1)
    trk = S.DroneQPTracker(cbf, num_robots=2)
    x_obs = np.array([[np.asarray(trajs[0](1.5)[0], dtype=float) - [0, 0, .15], np.zeros(3)]])
    geo.do_control(trajs=trajs, qpTracker=trk, render=False, computed_K=K, x_obs_list=x_obs, obs_r_list=[.1])
    obs = np.asarray(geo.observations)
    print(f"with a tracker: statuses {np.bincount(geo.statuses.ravel(), minlength=2).tolist()}, kernel form {geo.last_cbf_kernel}, "
          f"final |pos - target| {np.abs(obs[-1, :, :3] - [tr(2.0)[0] for tr in trajs]).max():.3f} m")
    assert obs.shape == (200, 2, 20) and np.isfinite(obs).all()
    assert geo.statuses.shape == (200, 1) and geo.last_cbf_kernel == 0
    # without a tracker: the gain of the last fedCE() on this object, any trajectory type
    geo.observations = []
    geo.circle_initialize()
    geo.create_env()
    delta = np.array([0, 5, 0])
    comp = [S.CompoundTrajectory([S.LineTrajectory(start=geo.INIT_XYZS[i], end=geo.TARGET_POSITIONS[i], speed=.5),
                                  S.WaitTrajectory(duration=1, position=geo.TARGET_POSITIONS[i]),
                                  S.LineTrajectory(start=geo.TARGET_POSITIONS[i], end=geo.TARGET_POSITIONS[i] + delta, speed=1),
                                  S.LineTrajectory(start=geo.TARGET_POSITIONS[i] + delta, end=geo.TARGET_POSITIONS[i], speed=1)])
            for i in range(2)]
    geo.do_control(trajs=comp, render=False, use_noisy_model=False)
    obs = np.asarray(geo.observations)
    assert obs.shape == (200, 2, 20) and np.isfinite(obs).all()

#!/usr/bin/env python3
"""Mint tests/golden/fedce_omega_ref_in_loop.npz: FedCE on the 9-state thrust / body-rate model with the reference's own
DecentralizedLQROmega in the loop.

Run ONLY in the build container, where the reference lives (see mint_golden.py):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/mint_fedce_omega.py

control/dlqr/decentralized_lqr_omega.py, model/linear_omega.py, control/lqr/lqr_omega_controller.py and
control/low_level/thrust_omega_ctrl.py are loaded BY PATH with the stubs of mint_golden.py (ThrustOmegaController's [UPSTREAM]
BaseControl base class is STUBBED, as in thrust_omega.npz), and GeometricEnv.fedCE_iteration's call sequence
(simulations/EnvGeometricOmega.py:127-263, default arguments: random warm-up, set-point CE phase, no wind) is driven with those
objects -- sigma1 / sigma_explore, compute_low_level, error_state, theta_update2 (forward_predict = scipy's solve_ivp),
compute_controller, set_desired_trajectory, compute -- and the oracle's DYN step (np_oracle.AviaryOracle at 100 / 100 Hz) in place
of Bullet.  The noise draws are recorded by wrapping sigma1 / sigma_explore; scipy.integrate.solve_ivp is wrapped to record the
accepted-step count and nfev of every forward_predict call.
Cases: D = 2, five iterations; D = 3, three iterations (circle_initialize poses of EnvGeometricOmega.py, init_rad 0.2).
A second block, rls2_unit: 64 theta_update2 calls on caller-made (phi, x_tp1) for two drones.
A third block, long: ONE identification phase of 100 steps (99 updates) for two drones with caller-made inputs that keep exciting the
model (thrust within 10 % of hover, body rates up to 0.05 rad/s), through the same reference objects: the long chain of information-
matrix updates that the script's default of 20 iterations builds."""
import contextlib
import io
import os
import sys
import tempfile
import types

import numpy as np
import scipy
import scipy.integrate

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import mint_golden as MG  # noqa: E402
import mint_fedce as MF  # noqa: E402
from oracle import np_oracle as O  # noqa: E402

IVP = {"steps": [], "nfev": []}


def circle(D, init_rad=0.2):
    """GeometricEnv.circle_initialize (EnvGeometricOmega.py:358-379)."""
    xyz = np.zeros((D, 3))
    for i in range(1, D):
        xyz[i, 0] = init_rad * np.sin((i / D) * 2 * np.pi)
        xyz[i, 1] = init_rad * np.cos((i / D) * 2 * np.pi)
    tpos = xyz.copy()
    tpos[:, 2] += 1
    trpy = np.zeros((D, 3))
    trpy[:, 2] = np.pi / 2
    return xyz, np.zeros((D, 3)), tpos, trpy


def load_dlqr_omega():
    ref = MG.load_reference()
    keep = MG.OUT
    MG.OUT = tempfile.mkdtemp()                  # the two helpers below also write their own fixtures: not into tests/golden
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            MG.mint_thrust_omega()               # registers the STUBBED [UPSTREAM] BaseControl
            MG.mint_lqr_omega(ref)               # the module wiring of control.lqr / control.low_level / model
    finally:
        MG.OUT = keep
    mc = ref["mc"]
    sys.modules["utils"].obs_to_lin_model = mc.obs_to_lin_model
    lin = MG.load("model.linearized", MG.REF + "/model/linearized.py")
    sys.modules["model"].LinearizedModel = lin.LinearizedModel
    to = sys.modules["control.low_level.thrust_omega_ctrl"]
    sys.modules["control"].ThrustOmegaController = to.ThrustOmegaController
    sys.modules["control.lqr"].lqr_omega_controller = sys.modules["control.lqr.lqr_omega_controller"]
    dl = MG.load("control.dlqr.decentralized_lqr_omega", MG.REF + "/control/dlqr/decentralized_lqr_omega.py")
    real = scipy.integrate.solve_ivp

    def solve_ivp(*a, **k):
        sol = real(*a, **k)
        IVP["steps"].append(len(sol.t) - 1)
        IVP["nfev"].append(sol.nfev)
        return sol
    scipy.integrate.solve_ivp = solve_ivp
    return dl.DecentralizedLQROmega, ref["lin_o"].LinearizedOmegaModel, mc


def make_env():
    env = MF.make_env()
    env.DRONE_MODEL = sys.modules["gym_pybullet_drones.utils.enums"].DroneModel("cf2p")
    return env


def run(D, num_iter, seed, DLQR, Lin, mc, k=2):
    np.random.seed(seed)
    env = make_env()
    xyz, rpy, tpos, trpy = circle(D)
    with contextlib.redirect_stdout(io.StringIO()):
        dl = DLQR(env, [Lin(env) for _ in range(D)])
    draws = {"warm": [], "explore": []}
    s1, se = dl.sigma1, dl.sigma_explore

    def sigma1():
        u = s1()
        draws["warm"].append(u.copy())
        return u

    def sigma_explore():
        u = se()
        draws["explore"].append(u.copy())
        return u
    dl.sigma1, dl.sigma_explore = sigma1, sigma_explore
    ora = O.AviaryOracle(xyz, rpy, O.CF2P, 100, 100)
    obs_log, thetas, Ps, Ks, upd, ce_act, ce_u = [], [], [], [], [], [], []
    i0 = len(IVP["steps"])

    def step(action):
        o = ora.step(action)
        obs_log.append(o.copy())
        return o

    def update(phis, e_tp1s):
        dl.theta_update2(phis, e_tp1s)
        upd.append(np.array([dl.get_thetai(j) for j in range(D)]))

    for n in range(num_iter):                      # fedCE_iteration(..., do_warmup=(n == 0), random_warmup=True)
        Texp = n * k
        Tce = n * (k ** 3)
        Tw = 25 if n == 0 else 0
        obs = step(np.zeros((D, 4)))
        for i in range(Tw):
            phis, e_tp1s, action = [], [], np.zeros((D, 4))
            for j in range(D):
                x = mc.obs_to_lin_model(obs[j], dim=9)
                u = dl.sigma1()
                act = dl.compute_low_level(u, obs[j], j)
                x_des = np.zeros((9,))
                x_des[0:3] = rpy[j]
                x_des[-3:] = xyz[j]
                u[0] = u[0] - env.M * env.G
                e = dl.error_state(x, x_des)
                action[j, :] = act
                phis.append(np.hstack([e, u]))
            obs = step(action)
            for j in range(D):
                x_tp1 = mc.obs_to_lin_model(obs[j], dim=9)
                x_des = np.zeros((9,))
                x_des[0:3] = rpy[j]
                x_des[-3:] = xyz[j]
                e_tp1s.append(dl.error_state(x_tp1, x_des))
            if i != 0:
                update(phis, e_tp1s)
        last_desired = np.zeros((D, 9))
        dl.compute_controller()
        Ks.append(dl.K.copy())
        for i in range(Tce):
            for j in range(D):
                dl.set_desired_trajectory(j, desired_pos=tpos[j], desired_vel=np.zeros((3,)), desired_acc=np.zeros((3,)),
                                          desired_yaw=trpy[j][2], desired_omega=0)
                last_desired[j, :] = np.hstack([trpy[j], np.zeros((3,)), tpos[j]])
            action, u = dl.compute(obs)
            ce_act.append(np.array(action))
            ce_u.append(np.array(u))
            obs = step(action)
        for i in range(Texp):
            phis, e_tp1s, action = [], [], np.zeros((D, 4))
            for j in range(D):
                x = mc.obs_to_lin_model(obs[j], dim=9)
                e = dl.error_state(x, last_desired[j])
                u = dl.sigma_explore()
                act = dl.compute_low_level(u, obs[j], j)
                u[0] = u[0] - env.M * env.G
                action[j, :] = act
                phis.append(np.hstack([e, u]))
            obs = step(action)
            for j in range(D):
                e_tp1s.append(dl.error_state(mc.obs_to_lin_model(obs[j], dim=9), last_desired[j]))
            if i != 0:
                update(phis, e_tp1s)
        thetas.append(dl.theta.copy())
        Ps.append(dl.P.copy())
    warm = np.array(draws["warm"]).reshape(-1, D, 4)
    explore = np.array(draws["explore"]).reshape(-1, D, 4)
    return dict(xyz=xyz, rpy=rpy, target_pos=tpos, target_rpy=trpy, num_iter=num_iter, seed=seed, u_warm=warm, u_explore=explore,
                thetas=np.array(thetas), Ps=np.array(Ps), Ks=np.array(Ks), theta_updates=np.array(upd), obs_log=np.array(obs_log),
                ce_actions=np.array(ce_act), ce_u=np.array(ce_u),
                ivp_steps=np.array(IVP["steps"][i0:]).reshape(-1, D), ivp_nfev=np.array(IVP["nfev"][i0:]).reshape(-1, D))


def rls2_unit(DLQR, Lin, n_calls=64, D=2, seed=31):
    """theta_update2 on caller-made (phi, x_tp1): entries at the scale the loop above produces."""
    rng = np.random.default_rng(seed)
    env = make_env()
    with contextlib.redirect_stdout(io.StringIO()):
        dl = DLQR(env, [Lin(env) for _ in range(D)])
    phis = rng.normal(0, .3, (n_calls, D, 13))
    phis[..., 9] = rng.normal(0, .05, (n_calls, D))
    phis[..., 10:] = rng.normal(0, .1, (n_calls, D, 3))
    xtp1 = rng.normal(0, .3, (n_calls, D, 9))
    i0 = len(IVP["steps"])
    th, P = [], []
    for t in range(n_calls):
        dl.theta_update2(list(phis[t]), list(xtp1[t]))
        th.append(np.array([dl.get_thetai(j) for j in range(D)]))
        P.append(dl.P.copy())
    return dict(phis=phis, xtp1=xtp1, thetas=np.array(th), Ps=np.array(P),
                ivp_steps=np.array(IVP["steps"][i0:]).reshape(-1, D), ivp_nfev=np.array(IVP["nfev"][i0:]).reshape(-1, D))


def long_phase(DLQR, Lin, mc, T=100, D=2, seed=41):
    """the warm-up loop of fedCE_iteration (:143-193) with caller-made u, T steps in one phase"""
    rng = np.random.default_rng(seed)
    env = make_env()
    xyz, rpy, _, _ = circle(D)
    with contextlib.redirect_stdout(io.StringIO()):
        dl = DLQR(env, [Lin(env) for _ in range(D)])
    mg = env.M * env.G
    us = np.concatenate([rng.uniform(.9 * mg, 1.1 * mg, (T, D, 1)), rng.uniform(-.05, .05, (T, D, 3))], axis=2)
    ora = O.AviaryOracle(xyz, rpy, O.CF2P, 100, 100)
    i0 = len(IVP["steps"])
    obs = ora.step(np.zeros((D, 4)))
    obs_log, upd = [obs.copy()], []
    x_des = np.hstack([rpy, np.zeros((D, 3)), xyz])
    for i in range(T):
        phis, e_tp1s, action = [], [], np.zeros((D, 4))
        for j in range(D):
            u = us[i, j].copy()
            act = dl.compute_low_level(u, obs[j], j)
            u[0] = u[0] - mg
            action[j, :] = act
            phis.append(np.hstack([dl.error_state(mc.obs_to_lin_model(obs[j], dim=9), x_des[j]), u]))
        obs = ora.step(action)
        obs_log.append(obs.copy())
        for j in range(D):
            e_tp1s.append(dl.error_state(mc.obs_to_lin_model(obs[j], dim=9), x_des[j]))
        if i != 0:
            dl.theta_update2(phis, e_tp1s)
            upd.append(np.array([dl.get_thetai(j) for j in range(D)]))
    return dict(xyz=xyz, rpy=rpy, u=us, theta_updates=np.array(upd), P=dl.P.copy(), obs_log=np.array(obs_log),
                ivp_steps=np.array(IVP["steps"][i0:]).reshape(-1, D), ivp_nfev=np.array(IVP["nfev"][i0:]).reshape(-1, D))


if __name__ == "__main__":
    DLQR, Lin, mc = load_dlqr_omega()
    out = {}
    for D, num_iter, seed in ((2, 5, 11), (3, 3, 12)):
        r = run(D, num_iter, seed, DLQR, Lin, mc)
        out.update({f"d{D}_{k}": v for k, v in r.items()})
        print(f"D = {D}: {num_iter} iterations, {len(r['obs_log'])} steps, {len(r['theta_updates'])} updates, solve_ivp steps "
              f"{np.unique(r['ivp_steps'])}, nfev {np.unique(r['ivp_nfev'])}, |theta| max {np.abs(r['thetas']).max():.3g}")
    r = rls2_unit(DLQR, Lin)
    out.update({f"rls2_unit_{k}": v for k, v in r.items()})
    print(f"rls2_unit: solve_ivp steps {np.unique(r['ivp_steps'])}, nfev {np.unique(r['ivp_nfev'])}, |theta| max {np.abs(r['thetas']).max():.3g}")
    r = long_phase(DLQR, Lin, mc)
    out.update({f"long_{k}": v for k, v in r.items()})
    print(f"long: {len(r['theta_updates'])} updates, solve_ivp steps {np.unique(r['ivp_steps'])}, |theta| max {np.abs(r['theta_updates']).max():.3g}, "
          f"cond(P) {np.linalg.cond(r['P'][0]):.3g}, final |pos - start| {np.abs(r['obs_log'][-1][:, :3] - r['xyz']).max():.3g}")
    path = os.path.join(HERE, "fedce_omega_ref_in_loop.npz")
    np.savez_compressed(path, ctrl_timestep=0.01, rtol=1e-3, atol=1e-6, base_class="stubbed",
                        physics="oracle DYN step (np_oracle.AviaryOracle, 100 / 100 Hz, no wind); DecentralizedLQROmega, "
                                "LinearizedOmegaModel, ThrustOmegaController and model conversions: reference objects",
                        **out, **MG.META)
    print(os.path.getsize(path), "bytes")

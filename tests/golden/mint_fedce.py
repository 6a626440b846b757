#!/usr/bin/env python3
"""Mint tests/golden/fedce_ref_in_loop.npz: FedCE with the reference's own DecentralizedLQR in the loop.

Run ONLY in the build container, where the reference lives (see mint_golden.py):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/mint_fedce.py

control/dlqr/decentralized_lqr.py is loaded BY PATH with the stubs of mint_golden.py, and GeometricEnv.fedCE_iteration's call
sequence (simulations/EnvGeometric.py:113-325, default arguments: random warm-up, set-point CE phase) is driven with those objects
-- sigma1 / sigma_explore, error_state, approx_theta_update, compute_controller, set_desired_trajectory, compute, the reference's
input_to_action / action_to_input / obs_to_lin_model -- and the oracle's DYN step (np_oracle.AviaryOracle, wind 2.5e-4 N along x
before every step but the zero-action one) in place of Bullet.  The noise draws are recorded by wrapping sigma1 / sigma_explore.
Cases: D = 2, six iterations; D = 3, three iterations (circle_initialize poses, init_rad 1)."""
import contextlib
import io
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import mint_golden as MG  # noqa: E402
from oracle import np_oracle as O  # noqa: E402

WIND = 0.00025


def circle(D, init_rad=1.0):
    """GeometricEnv.circle_initialize (:502-524) -> INIT_XYZS, INIT_RPYS, TARGET_POSITIONS, TARGET_RPYS."""
    xyz = np.zeros((D, 3))
    for i in range(1, D):
        xyz[i, 0] = init_rad * np.sin(((i - 1) / D) * 2 * np.pi)
        xyz[i, 1] = init_rad * np.cos(((i - 1) / D) * 2 * np.pi)
    tpos = xyz.copy()
    tpos[:, 2] += 1
    trpy = np.zeros((D, 3))
    trpy[:, 2] = np.pi / 2
    return xyz, np.zeros((D, 3)), tpos, trpy


def load_dlqr():
    ref = MG.load_reference()
    mc = ref["mc"]
    import types
    sys.modules["utils"].obs_to_lin_model = mc.obs_to_lin_model
    m = types.ModuleType("model")
    m.__path__ = [MG.REF + "/model"]
    sys.modules["model"] = m
    lin = MG.load("model.linearized", MG.REF + "/model/linearized.py")
    m.LinearizedModel = lin.LinearizedModel
    lq = types.ModuleType("control.lqr")
    lq.__path__ = [MG.REF + "/control/lqr"]
    sys.modules["control.lqr"] = lq
    lq.lqr_controller = MG.load("control.lqr.lqr_controller", MG.REF + "/control/lqr/lqr_controller.py")
    dl = MG.load("control.dlqr.decentralized_lqr", MG.REF + "/control/dlqr/decentralized_lqr.py")
    return dl.DecentralizedLQR, lin.LinearizedModel, mc


def make_env():
    env = MG.make_env()
    c = O.CF2P
    env.MAX_XY_TORQUE, env.MAX_Z_TORQUE = c.MAX_XY_TORQUE, c.MAX_Z_TORQUE
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
    obs_log, thetas, Ps, Ks = [], [], [], []

    def step(action, wind=True):
        ora.wind = np.array([WIND, 0.0, 0.0]) if wind else None
        o = ora.step(action)
        obs_log.append(o.copy())
        return o

    for n in range(num_iter):                      # fedCE_iteration(..., do_warmup=(n == 0), random_warmup=True)
        Texp = min(n * k, 20 * k)
        Tce = k * n * 2
        Tw = 25 if n == 0 else 0
        obs = step(np.zeros((D, 4)), wind=False)
        for i in range(Tw):
            phis, e_tp1s, action = [], [], np.zeros((D, 4))
            for j in range(D):
                x = mc.obs_to_lin_model(obs[j])
                u = dl.sigma1()
                act = mc.input_to_action(env, u)
                x_des = np.zeros((12,))
                x_des[0:3] = rpy[j]
                x_des[-3:] = xyz[j]
                u[0] = u[0] - env.M * env.G
                e = dl.error_state(x, x_des)
                action[j] = act
                phis.append(np.hstack([e, u]))
            for i in range(D):                     # the wind loop that shadows the step counter (:206)
                pass
            obs = step(action)
            for j in range(D):
                x_des = np.zeros((12,))
                x_des[0:3] = rpy[j]
                x_des[-3:] = xyz[j]
                e_tp1s.append(dl.error_state(mc.obs_to_lin_model(obs[j]), x_des))
            if i != 0:
                dl.approx_theta_update(phis, e_tp1s)
        last_desired = np.zeros((D, 12))
        dl.compute_controller()
        Ks.append(dl.K.copy())
        for i in range(Tce):
            for j in range(D):
                dl.set_desired_trajectory(j, desired_pos=tpos[j], desired_vel=np.zeros((3,)), desired_acc=np.zeros((3,)),
                                          desired_yaw=trpy[j][2], desired_omega=0)
                last_desired[j, :] = np.hstack([trpy[j], np.zeros((3,)), np.zeros((3,)), tpos[j]])
            action, u = dl.compute(obs)
            for i in range(D):
                pass
            obs = step(action)
        for i in range(Texp):
            phis, e_tp1s, action = [], [], np.zeros((D, 4))
            for j in range(D):
                x = mc.obs_to_lin_model(obs[j])
                e = dl.error_state(x, last_desired[j])
                u = dl.sigma_explore()
                act = mc.input_to_action(env, u)
                u = mc.action_to_input(env, act)
                u[0] = u[0] - env.M * env.G
                action[j] = act
                phis.append(np.hstack([e, u]))
            for i in range(D):
                pass
            obs = step(action)
            for j in range(D):
                e_tp1s.append(dl.error_state(mc.obs_to_lin_model(obs[j]), last_desired[j]))
            if i != 0:
                dl.approx_theta_update(phis, e_tp1s)
        thetas.append(dl.theta.copy())
        Ps.append(dl.P.copy())
    warm = np.array(draws["warm"]).reshape(-1, D, 4)
    explore = np.array(draws["explore"]).reshape(-1, D, 4)
    return dict(xyz=xyz, rpy=rpy, target_pos=tpos, target_rpy=trpy, num_iter=num_iter, seed=seed, u_warm=warm, u_explore=explore,
                thetas=np.array(thetas), Ps=np.array(Ps), Ks=np.array(Ks), pred_errors=np.array(dl.pred_errors),
                pred_thetas=np.array(dl.pred_thetas), obs_log=np.array(obs_log))


if __name__ == "__main__":
    DLQR, Lin, mc = load_dlqr()
    out = {}
    for D, num_iter, seed in ((2, 6, 11), (3, 3, 12)):
        r = run(D, num_iter, seed, DLQR, Lin, mc)
        out.update({f"d{D}_{k}": v for k, v in r.items()})
        print(f"D = {D}: {num_iter} iterations, {len(r['obs_log'])} steps, {r['pred_errors'].shape[1]} updates")
    np.savez_compressed(os.path.join(HERE, "fedce_ref_in_loop.npz"), wind=WIND,
                        physics="oracle DYN step (np_oracle.AviaryOracle); DecentralizedLQR and model conversions: reference objects",
                        **out, **MG.META)

#!/usr/bin/env python3
"""Mint tests/golden/cbf_dlqr_ref_in_loop.npz: the CBF-filtered loop of simulations/CBFTest.py (:295-350) with
``args.controller == 'dlqr'``, i.e. the reference's DecentralizedLQROmega as the nominal controller under the order-2 ECBF filter.

Run ONLY in the build container, where the reference lives (see mint_golden.py):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/mint_cbf_dlqr.py

Reference objects: DecentralizedLQROmega (compute_controller on the initial (Ahat, Bhat), set_desired_trajectory,
compute(obs, skip_low_level=True) -- whose returned u is the CAPPED one, cap_u :233-236 --, compute_low_level), LinearizedOmegaModel,
ThrustOmegaController (its [UPSTREAM] base class stubbed, as in thrust_omega.npz) and trajectories/Lemniscate.py.
The oracle's: the ECBF rows and the QP (np_oracle.cbf_filter; the reference's cvxopt is absent, and an infeasible QP would follow this
project's modelled fallback -- the scene below has none) and the DYN step (np_oracle.AviaryOracle, 100 / 100 Hz).
With D > 1 the reference's :348 calls ``ctrl[j].compute_low_level`` on its one-element ``ctrl`` list and raises IndexError for j >= 1;
the D = 3 block calls ``ctrl[0].compute_low_level(u_safe[j], obs[j], j)``, what ``ctrl[0]`` evidently stands for (:306, :312, :323).

The scene: drone j on Lemniscate(a=1, omega=.5, center=(0, 0, .5 + j dz), yaw_rate=0, phase_shift=0), started on its own t = 0 point
with rpy 0; one sphere of radius 0.1 at drone 0's path point of t = 1.5 s lowered by 0.15 m; DroneCBF(safety_radius=0.1, zscale=1),
default poles.  Blocks: d1_* (300 steps), d3_* (dz = 0.15, 300 steps).  The script refuses to write the file unless every status is 0,
the filter changes u on >= 50 steps and cap_u clips on >= 20 steps."""
import contextlib
import io
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import mint_golden as MG  # noqa: E402
from mint_fedce_omega import load_dlqr_omega, make_env, circle  # noqa: E402,F401
from oracle import np_oracle as O  # noqa: E402

STEPS = 300


def run(D, dz, DLQR, Lin, Lem):
    c = O.CF2P
    env = make_env()
    mg = env.M * env.G
    P = np.array([[1.0, .5, 0.0, 0.0, .5 + j * dz, 0.0, 0.0] for j in range(D)])        # a, omega, centre, yaw_rate, phase_shift
    trajs = [Lem(a=1, omega=.5, center=np.array([0, 0, .5 + j * dz]), yaw_rate=0, phase_shift=0) for j in range(D)]
    xyz = np.array([np.asarray(trajs[j](0.0)[0], dtype=float) for j in range(D)])
    rpy = np.zeros((D, 3))
    centre = np.asarray(trajs[0](1.5)[0], dtype=float) - np.array([0, 0, .15])
    x_obs, obs_r = np.array([[centre, np.zeros(3)]]), [0.1]
    Kcbf = np.poly(np.array([-2.2, -2.4]))[1:][::-1].copy()              # cbf/cbf.py:115-124 on DroneCBF's default poles
    umax = np.array([env.MAX_THRUST, 10.0, 10.0, 10.0])
    with contextlib.redirect_stdout(io.StringIO()):
        dl = DLQR(env, [Lin(env) for _ in range(D)])
    dl.compute_controller()                                                # force_diagonal=False
    K = dl.K.copy()
    lo, hi = 4 * (9440.3 ** 2 * env.KF), env.MAX_THRUST
    ora = O.AviaryOracle(xyz, rpy, c, 100, 100)
    obs = ora.step(np.zeros((D, 4)))                                       # :297-299
    rec = dict(obs=[obs.copy()], u_nom=[], u_safe=[], status=[], action=[], clipped=[])
    t = 0.0
    for i in range(STEPS):
        for j in range(D):
            pos, vel, acc, yaw, omega = trajs[j](t)
            dl.set_desired_trajectory(j, desired_pos=pos, desired_vel=vel, desired_acc=acc, desired_yaw=yaw, desired_omega=omega)
        action, u = dl.compute(obs, skip_low_level=True)                   # :323: (None, cap_u(u))
        assert action is None
        nominal_us = np.array(u, dtype=float)
        rec["u_nom"].append(nominal_us.copy())
        rec["clipped"].append((nominal_us[:, 0] == lo) | (nominal_us[:, 0] == hi))
        nominal_us[:, 0] = nominal_us[:, 0] - mg                           # :339
        xdes = np.zeros((D, 9))
        for j in range(D):
            pos, vel, acc, yaw, omega = trajs[j](t)
            xdes[j] = np.hstack([0, 0, yaw, vel, pos])                     # :343
        x = np.array([O.obs_to_lin_model(obs[j], 9) for j in range(D)])
        u_safe, st = O.cbf_filter(x, xdes, nominal_us, 2, Kcbf, umax, 0.1, 1.0, c, x_obs, obs_r)     # :345 (oracle rows + QP)
        rec["u_safe"].append(u_safe.copy())
        rec["status"].append(st)
        u_safe = u_safe.copy()
        u_safe[:, 0] = u_safe[:, 0] + mg                                   # :346
        action = np.zeros((D, 4))
        for j in range(D):
            action[j, :] = dl.compute_low_level(u_safe[j, :], obs[j], j)   # :348 with ctrl[0] for ctrl[j]
        rec["action"].append(action.copy())
        obs = ora.step(action)                                             # :350
        rec["obs"].append(obs.copy())
        t += env.CTRL_TIMESTEP
    r = {k: np.array(v) for k, v in rec.items()}
    changed = (np.abs(r["u_safe"] - (r["u_nom"] - np.array([mg, 0, 0, 0]))).max(axis=(1, 2)) > 1e-9)
    offdiag = max(np.abs(K[4 * a:4 * a + 4, 9 * b:9 * b + 9]).max() for a in range(D) for b in range(D) if a != b) if D > 1 else 0.0
    print(f"D = {D}: infeasible steps {int(r['status'].sum())}, the filter changes u on {int(changed.sum())} steps (max "
          f"{np.abs(r['u_safe'] - (r['u_nom'] - np.array([mg, 0, 0, 0]))).max():.3g}), cap_u clips on {int(r['clipped'].any(axis=1).sum())} steps "
          f"({int(r['clipped'].sum())} drone-steps), off-diagonal blocks of K up to {offdiag:.1e}")
    assert (r["status"] == 0).all(), "the scene must stay feasible: an infeasible step is this project's modelled fallback, not the reference's"
    assert changed.sum() >= 50 and r["clipped"].any(axis=1).sum() >= 20
    return dict(xyz=xyz, rpy=rpy, lem=P, x_obs=x_obs, obs_r=np.array(obs_r), Kcbf=Kcbf, umax=umax, K=K, obs_log=r["obs"], u_nom=r["u_nom"],
                u_safe=r["u_safe"], status=r["status"], action=r["action"], clipped=r["clipped"], changed=changed)


if __name__ == "__main__":
    DLQR, Lin, mc = load_dlqr_omega()
    Lem = sys.modules["ref_lem"].Lemniscate
    out = {}
    for D, dz in ((1, 0.0), (3, 0.15)):
        out.update({f"d{D}_{k}": v for k, v in run(D, dz, DLQR, Lin, Lem).items()})
    path = os.path.join(HERE, "cbf_dlqr_ref_in_loop.npz")
    np.savez_compressed(path, ctrl_timestep=0.01, safety_radius=0.1, zscale=1.0, steps=STEPS, base_class="stubbed",
                        parts="reference objects: DecentralizedLQROmega (compute_controller, set_desired_trajectory, compute(obs, "
                              "skip_low_level=True) with cap_u, compute_low_level), LinearizedOmegaModel, ThrustOmegaController, Lemniscate; "
                              "oracle: ECBF rows + QP (np_oracle.cbf_filter, cvxopt absent), DYN step (np_oracle.AviaryOracle, 100 / 100 Hz); "
                              "d3: ctrl[0].compute_low_level in the place of the reference's ctrl[j] (IndexError for j >= 1, CBFTest.py:348); "
                              "u_nom: the capped u as compute returns it (M G included), u_safe: the filter's output (M G not yet added back)",
                        **out, **MG.META)
    print(os.path.getsize(path), "bytes")

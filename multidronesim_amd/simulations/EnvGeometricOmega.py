"""simulations/EnvGeometricOmega.py of the reference: trajectory tracking with the thrust / body-rate input model --
``GeometricEnv(args, circle_init)`` with a LinearizedOmegaModel per drone (:99), ``do_control(trajs, render, computed_K,
use_noisy_model)`` (:262-335) whose 'lqr' branch is ``LQROmegaController(env, model, ThrustOmegaController(env)).compute(obs[j])``
(nominal input + PID low level, :286-289, :314) followed by ``env.step(action)`` (:327), no wind, ``--init_rad 0.2`` and 50 s by
default (:28, :57).  The loop runs fused for every drone of every env (``mds_rollout_nominal_fused``: the whole run in one launch,
PID memory in registers; ``render=True``: ``mds_step_nominal`` step by step in real time).  ``fedCE`` / ``fedCE_iteration``
(:109-263) identify the 9-state model with DecentralizedLQROmega, every phase one launch (mds_fedce_omega_identify,
mds_rollout_dlqr_omega_fused), and ``do_control(..., computed_K=K)`` with ``controller == 'dlqr'`` (:277-280, :317-318) runs the
identified gain.  ``warm_up_only`` is not built."""
from __future__ import annotations

import time

import numpy as np
import torch

from ..trajectories import *  # noqa: F401,F403
from . import CBFTest as _cbf
from . import EnvGeometric as _base

DEFAULT_DURATION_SEC = 50                 # :28
controllers = ['lqr', 'geometric', 'dlqr']        # :32, with 'dlqr' (selected by the script itself, :393) appended: the default stays 'lqr'


def parse_args(argv=None):
    args = _cbf.parse_args(argv)          # init_rad 0.2 (:57)
    if argv is None or '--duration_sec' not in argv:
        args.duration_sec = DEFAULT_DURATION_SEC
    return args


class GeometricEnv(_cbf.GeometricEnv):
    def do_control(self, trajs=None, render=False, computed_K=None, use_noisy_model=True):          # the reference's default (:265)
        if self.args.controller == 'dlqr':
            return self._do_control_dlqr(trajs, computed_K, render)
        if computed_K is not None:
            raise NotImplementedError("do_control(computed_K=...) applies to controller 'dlqr' only (set args.controller = 'dlqr', :393)")
        # LQROmegaController(..., use_noisy_model=True) designs its gain on (Ahat, Bhat) (control/lqr/lqr_omega_controller.py:31-36)
        self._noisy = bool(use_noisy_model)
        return super().do_control(trajs=trajs, render=render, qpTracker=None)

    def _do_control_dlqr(self, trajs, computed_K, render=False):
        """:277-280, :297-329: a fresh DecentralizedLQROmega (fresh PID memory) with K = computed_K, one zero-action step, then the
        whole run in one launch (``render=True``: one launch per step, in real time, as the reference with its GUI)."""
        from ..utils.utils import sync
        from ..control import DecentralizedLQROmega
        from ..trajectories import WaitTrajectory
        env, args = self.env, self.args
        K = computed_K
        if K is None:                     # the reference sets dLQR.K = None here and fails at the first compute (:279, :220)
            raise TypeError("controller 'dlqr' needs do_control(computed_K=K), the gain fedCE() returned")
        dlqr = DecentralizedLQROmega(env, self.linear_models)
        dlqr.K = K
        dlqr.upload_gain(K)
        self._dlqr = dlqr
        if trajs is None:
            trajs = [WaitTrajectory(duration=float(args.duration_sec), position=self.TARGET_POSITIONS[j], yaw=self.TARGET_RPYS[j, 2])
                     for j in range(args.num_drones)]
        env.set_trajectories(list(trajs))
        env.set_wind([0.0, 0.0, 0.0])
        env.step(torch.zeros((env.NUM_ENVS, env.NUM_DRONES, 4), dtype=env.dtype, device=env.device))       # :293-294
        steps = int(args.duration_sec * env.CTRL_FREQ)
        t = 0.0
        if render:
            START = time.time()
            log = torch.empty((steps, env.NUM_ENVS, env.NUM_DRONES, 20), dtype=env.dtype, device=env.device)
            for i in range(steps):
                log[i:i + 1].copy_(dlqr.rollout(t, 1, log=True))
                self.obs_ts.append(t)
                t += env.CTRL_TIMESTEP
                env.render()
                sync(i, START, env.CTRL_TIMESTEP)
        else:
            log = dlqr.rollout(0.0, steps, log=True)
            for i in range(steps):
                self.obs_ts.append(t)
                t += env.CTRL_TIMESTEP
        o = log.double().cpu().numpy()
        self.observations.extend(list(o[:, 0] if env.NUM_ENVS == 1 else o))
        self.obs = self.observations[-1]
        env.close()

    # ------------------------------------------------------------------ FedCE (:109-263)
    def fedCE(self, num_iter=15, noise=None, generator=None, log_observations=False, log_iterations=False, log_updates=False, verbose=False,
              riccati="host"):
        """-> (K, theta) of the last iteration, as the reference (:109-125).  ``noise``: per iteration (u_warm [25,(E,)D,4] or None,
        u_explore [Texp,(E,)D,4]) raw draws instead of sigma1 / sigma_explore.  ``log_iterations`` keeps theta, P and K of every
        iteration in fedce_thetas / fedce_Ps / fedce_Ks; ``log_observations`` every observation in fedce_observations; ``log_updates``
        every drone's theta after every theta_update2 in fedce_theta_updates ([D,13,9] each, or [E,D,13,9]).  ``riccati``: "host" (scipy,
        one env after the other) or "device" (every env at once), passed to compute_controller(solver=...)."""
        from ..control import DecentralizedLQROmega
        env, args = self.env, self.args
        steps = 0
        dLQR = DecentralizedLQROmega(env, self.linear_models)
        START = time.time()
        self.fedce_observations, self.fedce_thetas, self.fedce_Ps, self.fedce_Ks, self.fedce_theta_updates = [], [], [], [], []
        for n in range(num_iter):
            steps = self.fedCE_iteration(env, dLQR, START, steps, n, do_warmup=(n == 0), random_warmup=True,
                                         noise=None if noise is None else noise[n], generator=generator, log_observations=log_observations,
                                         log_updates=log_updates, riccati=riccati)
            if log_iterations:
                self.fedce_thetas.append(dLQR.theta)
                self.fedce_Ps.append(dLQR.P)
                self.fedce_Ks.append(np.copy(dLQR.K))
            if verbose:
                theta = dLQR.theta
                with np.printoptions(precision=3, suppress=True, linewidth=100000):
                    print(f"n: {n}, steps: {steps}")
                    print("Theta A:\n ", theta[..., :9 * args.num_drones, :].swapaxes(-1, -2))
                    print("Theta B:\n ", theta[..., 9 * args.num_drones:, :].swapaxes(-1, -2))
        theta = dLQR.theta
        self._fedce_K = dLQR.K
        self.dLQR = dLQR
        env.close()
        return dLQR.K, theta

    def fedCE_iteration(self, env, dLQR, START, steps, n, k=2, do_warmup=True, random_warmup=True, do_lemniscate=False, do_print=False,
                        noise=None, generator=None, log_observations=False, log_updates=False, riccati="host"):
        """One FedCE iteration (:127-263): the zero-action step, [25-step random warm-up], compute_controller, Tce = n k^3 CE steps
        towards the targets, Texp = n k exploration steps around last_desired; each phase one launch, theta_update2 on every step of
        a phase but its first (`if i != 0`)."""
        from ..control.dlqr.decentralized_lqr_omega import UPDATE_SKIP_FIRST
        from ..trajectories import Lemniscate, WaitTrajectory
        if not random_warmup:
            raise NotImplementedError("fedCE_iteration(random_warmup=False): the LQR-driven warm-up is not built")
        D, E = self.args.num_drones, env.NUM_ENVS
        Texp = n * k
        Tce = n * (k ** 3)
        Tw = 25 if do_warmup else 0
        obs, _, _, _, _ = env.step(torch.zeros((E, D, 4), dtype=env.dtype, device=env.device))   # :136-137
        logs = [obs.clone()[None]] if log_observations else None
        if Tw:
            x_des = np.hstack([self.INIT_RPYS, np.zeros((D, 3)), self.INIT_XYZS])               # :156-158
            u = noise[0] if noise is not None else dLQR.draw_inputs("warmup", Tw, generator)
            log, obs, thl = dLQR.identify(u, x_des, UPDATE_SKIP_FIRST, log_obs=log_observations, log_theta=log_updates)
            self._keep_updates(thl)
            if log_observations:
                logs.append(log)
            steps += Tw
        last_desired = np.zeros((D, 9))
        dLQR.compute_controller(solver=riccati)
        if Tce:
            if do_lemniscate:
                env.set_trajectories([Lemniscate(center=np.array([0, 0, .5]), omega=1, yaw_rate=.1)] * D)
            else:
                env.set_trajectories([WaitTrajectory(position=self.TARGET_POSITIONS[j], duration=Tce * env.CTRL_TIMESTEP + 1.0,
                                                     yaw=self.TARGET_RPYS[j, 2]) for j in range(D)])
                last_desired = np.hstack([self.TARGET_RPYS, np.zeros((D, 3)), self.TARGET_POSITIONS])   # :213-214
            log = dLQR.rollout(0.0, Tce, log=log_observations)
            if log_observations:
                logs.append(log)
            steps += Tce
        if Texp:
            u = noise[1] if noise is not None else dLQR.draw_inputs("explore", Texp, generator)
            log, obs, thl = dLQR.identify(u, last_desired, UPDATE_SKIP_FIRST, log_obs=log_observations, log_theta=log_updates)
            self._keep_updates(thl)
            if log_observations:
                logs.append(log)
            steps += Texp
        if log_observations:
            o = torch.cat([l.reshape(-1, E, D, 20) for l in logs]).double().cpu().numpy()
            self.fedce_observations.extend(list(o[:, 0] if E == 1 else o))
        self.obs = env._obs.double().cpu().numpy()
        self.obs = self.obs[0] if E == 1 else self.obs
        return steps

    def _keep_updates(self, thl):
        """theta log of one phase [T,E,D,13,9] -> fedce_theta_updates: the phase's first step does not update"""
        if thl is not None:
            th = thl[1:].cpu().numpy()
            self.fedce_theta_updates.extend(list(th[:, 0] if th.shape[1] == 1 else th))

    def _nominal(self, env):
        if self.args.controller == 'lqr' and getattr(self, "_noisy", False):
            from ..control import LQROmegaController, ThrustOmegaController
            LQROmegaController(env, self.linear_models[0], ThrustOmegaController(env), use_noisy_model=True)
            return 'lqr_omega'
        return super()._nominal(env)

    def circle_initialize(self):
        """:356-381: drone i > 0 at angle 2 pi i / N (EnvGeometric.py uses (i - 1) / N), targets one metre above, target yaw pi / 2."""
        args = self.args
        self.INIT_XYZS = np.zeros((args.num_drones, 3))
        for i in range(1, args.num_drones):
            self.INIT_XYZS[i, 0] = args.init_rad * np.sin((i / args.num_drones) * 2 * np.pi)
            self.INIT_XYZS[i, 1] = args.init_rad * np.cos((i / args.num_drones) * 2 * np.pi)
        for i in range(args.num_drones):
            self.INIT_RPYS[i, 2] = 0
            self.TARGET_POSITIONS[i, 0:2] = self.INIT_XYZS[i, 0:2]
            self.TARGET_POSITIONS[i, 2] = self.INIT_XYZS[i, 2] + self.starting_target_offset
            self.TARGET_RPYS[i] = [0, 0, np.pi / 2]


def main(argv=None, num_iter=20):
    """The reference's __main__ (:382-407): fedCE(num_iter=20), then the identified gain on the compound line / wait trajectories."""
    ARGS = parse_args(argv)
    geo = GeometricEnv(ARGS, circle_init=True)
    geo.create_env()
    computed_K, theta = geo.fedCE(num_iter=num_iter)                            # :392
    geo.args.controller = 'dlqr'                                                # :393
    geo.create_env()
    delta = np.array([0, 5, 0])
    trajs = [CompoundTrajectory([LineTrajectory(start=geo.INIT_XYZS[idx], end=geo.TARGET_POSITIONS[idx], speed=.5),         # noqa: F405  (:398-405)
                                 WaitTrajectory(duration=1, position=geo.TARGET_POSITIONS[idx]),                             # noqa: F405
                                 LineTrajectory(start=geo.TARGET_POSITIONS[idx], end=geo.TARGET_POSITIONS[idx] + delta, speed=1),   # noqa: F405
                                 LineTrajectory(start=geo.TARGET_POSITIONS[idx] + delta, end=geo.TARGET_POSITIONS[idx], speed=1)])   # noqa: F405
             for idx in range(ARGS.num_drones)]
    geo.do_control(trajs=trajs, computed_K=computed_K, render=False, use_noisy_model=False)      # :406
    return geo


if __name__ == "__main__":
    geo = main()
    np.save("observations_lem_bad_mass.npy", geo.observations)                 # :407
    print("Wrote observations to observations_lem_bad_mass.npy", np.asarray(geo.observations).shape)

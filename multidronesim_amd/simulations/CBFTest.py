"""simulations/CBFTest.py of the reference: the order-2 CBF demo.  Same ``GeometricEnv`` as EnvGeometric.py with
LinearizedOmegaModel per drone (:107), ``--init_rad 0.2`` (:61) and a ``do_control`` that runs nominal controller ->
DroneQPTracker -> + M G -> low level -> env.step (:303-350) when a ``qpTracker`` is given.  ``fedCE`` / ``fedCE_iteration``
(:113-267) identify the 9-state model with DecentralizedLQROmega's ``theta_update``, the covariance form of the recursive least
squares, every phase one launch; ``controller == 'dlqr'`` (:281-284, :322-324) then flies that gain (or ``computed_K``): without a
tracker the whole run in one launch (mds_rollout_dlqr_omega_fused, any trajectory type), with one as the coupled nominal of the
filtered step loop (``set_cbf_nominal("dlqr_omega")``; the filter gets the capped u of ``compute(obs, skip_low_level=True)``).
With 'dlqr' and a tracker the reference calls ``ctrl[j].compute_low_level`` on its one-element ``ctrl`` list (:348) and raises
IndexError for j >= 1: for one drone the mirror is the reference, for more it does what ``ctrl[0]`` evidently stands for (modelled,
like the infeasible-QP branch)."""
from __future__ import annotations

import time

import numpy as np
import torch

from ..cbf import DroneCBF, DroneQPTracker
from ..control import LQROmegaController, ThrustOmegaController
from ..model import LinearizedOmegaModel
from ..trajectories import *  # noqa: F401,F403
from ..utils.utils import sync
from . import EnvGeometric as _base

controllers = ['lqr', 'geometric', 'dlqr']        # :32, with 'dlqr' (selected by the script itself, :437) appended: the default stays 'lqr'


def parse_args(argv=None):
    args = _base.parse_args(argv, init_rad=.2)
    if args.controller == _base.controllers[0] and (argv is None or '--controller' not in argv):
        args.controller = controllers[0]
    return args


class GeometricEnv(_base.GeometricEnv):
    ORDER, XDIM = 2, 9
    FEDCE_FORM = "theta_update"           # :192, :260

    def _make_linear_models(self, env):
        return [LinearizedOmegaModel(env) for _ in range(self.args.num_drones)]

    def _nominal(self, env):
        """The nominal controller objects the script builds (:283-293) and the name the fused step knows them by."""
        if self.args.controller == 'geometric':
            return 'geometric'
        if self.args.controller == 'lqr':
            LQROmegaController(env, self.linear_models[0], ThrustOmegaController(env))
            return 'lqr_omega'
        if self.args.controller == 'dlqr':       # :281-284: a fresh DecentralizedLQROmega (fresh PID memory) with the given gain
            from ..control import DecentralizedLQROmega
            K = self._dlqr_gain()
            self._dlqr = DecentralizedLQROmega(env, self.linear_models)
            self._dlqr.K = K
            self._dlqr.upload_gain(K)
            return 'dlqr_omega'
        raise NotImplementedError(f"controller {self.args.controller!r} is not one of {controllers}")

    def _dlqr_gain(self):
        """computed_K of do_control, or the gain of the last fedCE() on this object"""
        K = self._computed_K if self._computed_K is not None else self._fedce_K
        if K is None:
            raise NotImplementedError(f"controller {self.args.controller!r}: 'dlqr' needs a gain -- do_control(computed_K=...) or a fedCE() "
                                      "on this GeometricEnv first")
        return K

    def do_control(self, trajs=None, render=False, qpTracker=None, computed_K=None, use_noisy_model=False, x_obs_list=None,
                   obs_r_list=None):
        env = self.env
        if self.args.controller == 'geometric' and qpTracker is None:        # plain geometric tracking: the EnvGeometric loop, no wind
            return super().do_control(trajs=trajs, render=render, wind=False)
        self._computed_K = computed_K
        if self.args.controller == 'dlqr' and qpTracker is None and self.XDIM == 9:      # :322-324 + :350, any trajectory type
            return self._do_control_dlqr(trajs, self._dlqr_gain(), render)
        nominal = self._nominal(env)
        saved, self.args.controller = self.args.controller, 'geometric'      # _start only needs the trajectories and the first step
        try:
            steps = self._start(trajs)
        finally:
            self.args.controller = saved
        env.set_cbf_nominal(nominal)
        START = time.time()
        t = 0.0
        log = torch.empty((steps, env.NUM_ENVS, env.NUM_DRONES, 20), dtype=env.dtype, device=env.device)
        st_log = torch.zeros((steps, env.NUM_ENVS), dtype=torch.int32, device=env.device)
        if qpTracker is None and not render:   # ctrl[j].compute(obs[j]) = LQR + low level, then step (:296-300, :350): the whole run in one launch
            env.rollout_geometric_fused(0.0, steps, log=True, log_out=log, controller="nominal")
            for i in range(steps):
                self.obs_ts.append(t)
                t += env.CTRL_TIMESTEP
            steps = 0
        elif qpTracker is not None and not render:
            # nominal -> QP -> low level -> step (:303-350), the whole run through the persistent kernel where the library covers the
            # configuration (order 2, up to 16 drones per env, Lemniscates, Euler DYN at pyb == ctrl): 50 control steps per launch,
            # every step's observation into the log, every step's statuses into st_log.  MDS_EUNSUPPORTED: the step loop below.
            from .._capi import MdsError
            try:
                env.rollout_cbf_geometric_fused(0.0, steps, qpTracker, x_obs_list, obs_r_list, steps_per_launch=50, obs_log=log, status_log=st_log)
                for i in range(steps):
                    self.obs_ts.append(t)
                    t += env.CTRL_TIMESTEP
                steps = 0
            except MdsError as exc:
                if exc.status not in (-6, -5):          # unsupported combination / trajectories that are not Lemniscates
                    raise
        for i in range(steps):
            if qpTracker is not None:     # nominal -> QP -> low level -> step (:303-350)
                obs, st = env.step_cbf_geometric(t, qpTracker, x_obs_list, obs_r_list)
                st_log[i].copy_(st)
            else:
                obs = env.step_nominal(t)
            log[i].copy_(obs)
            self.obs_ts.append(t)
            t += env.CTRL_TIMESTEP
            if render:
                env.render()
                sync(i, START, env.CTRL_TIMESTEP)
        o = log.double().cpu().numpy()
        self.observations.extend(list(o[:, 0] if env.NUM_ENVS == 1 else o))
        self.obs = self.observations[-1]
        self.last_cbf_kernel = env.cbf_last_step_kernel()    # 2: the persistent rollout kernel, 1: one launch per step, 0: QP + low-level launches
        self.statuses = st_log.cpu().numpy()          # 1 where the QP was infeasible and the nominal control was kept (modelled fallback: cbf/qptracker.py docstring)
        env.close()

    def _do_control_dlqr(self, trajs, computed_K, render=False):
        """'dlqr' without a tracker (:281-284, :322-324, :350; EnvGeometricOmega.py:277-280, :297-329): a fresh DecentralizedLQROmega
        (fresh PID memory) with K = computed_K, one zero-action step, then the whole run in one launch (``render=True``: one launch
        per step, in real time, as the reference with its GUI)."""
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

    # ------------------------------------------------------------------ FedCE (:113-267; EnvGeometricOmega.py:109-263 is the same code with theta_update2)
    def fedCE(self, num_iter=15, noise=None, generator=None, log_observations=False, log_iterations=False, log_updates=False, verbose=False,
              riccati="host"):
        """-> (K, theta) of the last iteration, as the reference (:109-125).  ``noise``: per iteration (u_warm [25,(E,)D,4] or None,
        u_explore [Texp,(E,)D,4]) raw draws instead of sigma1 / sigma_explore.  ``log_iterations`` keeps theta, P and K of every
        iteration in fedce_thetas / fedce_Ps / fedce_Ks; ``log_observations`` every observation in fedce_observations; ``log_updates``
        every drone's theta after every update in fedce_theta_updates ([D,13,9] each, or [E,D,13,9]).  ``riccati``: "host" (scipy,
        one env after the other) or "device" (every env at once), passed to compute_controller(solver=...)."""
        from ..control import DecentralizedLQROmega
        if self.XDIM != 9:
            raise NotImplementedError("fedCE on the 10-state yank-omega model is not built (the reference's own call raises on its first update)")
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
        towards the targets, Texp = n k exploration steps around last_desired; each phase one launch, FEDCE_FORM (theta_update here, :192, :260;
        theta_update2 in EnvGeometricOmega.py) on every step of a phase but its first (`if i != 0`)."""
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
            log, obs, thl = dLQR.identify(u, x_des, UPDATE_SKIP_FIRST, log_obs=log_observations, log_theta=log_updates, form=self.FEDCE_FORM)
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
            log, obs, thl = dLQR.identify(u, last_desired, UPDATE_SKIP_FIRST, log_obs=log_observations, log_theta=log_updates, form=self.FEDCE_FORM)
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


def add_env_obstacles(env, x_obs_list, obs_r_list):
    """The reference loads a sphere URDF per obstacle into Bullet for display (:407-412); nothing to draw here."""
    return None


if __name__ == "__main__":
    ARGS = parse_args()
    geo = GeometricEnv(ARGS, circle_init=True)
    env = geo.create_env()
    trajs = [Lemniscate(center=np.array([0, 0, 0.5]), omega=0.5, yaw_rate=0) for _ in range(ARGS.num_drones)]      # noqa: F405  (:418)
    droneCBF = DroneCBF(env, geo.linear_models, safety_radius=0.1, zscale=1)
    droneTracker = DroneQPTracker(droneCBF, num_robots=ARGS.num_drones)
    x_obs_list = np.array([np.array([[0, 0, .5], np.zeros(3)])])
    obs_r_list = [.1]
    add_env_obstacles(env, x_obs_list, obs_r_list)
    geo.do_control(trajs=trajs, qpTracker=droneTracker, render=False, x_obs_list=x_obs_list, obs_r_list=obs_r_list)
    print("final positions (env 0):\n", np.asarray(geo.observations[-1]).reshape(-1, ARGS.num_drones, 20)[0, :, :3],
          "\nQP fallbacks:", int(geo.statuses.sum()), "of", geo.statuses.size)

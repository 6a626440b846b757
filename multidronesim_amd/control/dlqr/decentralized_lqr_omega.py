"""control/dlqr/decentralized_lqr_omega.py of the reference: ``DecentralizedLQROmega(env, lin_models, debug=False)`` -- the 9-state
decentralised LQR on the thrust / body-rate model (x = [rpy, vel, pos], u = [thrust, body rates]) whose models FedCE
(simulations/EnvGeometricOmega.py fedCE) identifies on line with ``theta_update2``: an information-matrix recursive least squares
whose innovation is taken against a forward prediction (scipy's solve_ivp in the reference, restated in csrc/mds_fedce_omega.hpp).

The per-drone learner state (theta [13,9], the information matrix the reference calls P [13,13] and its inverse, float64 in every
env dtype) and the ThrustOmega PID memory live on the device: ``identify`` runs a whole warm-up or exploration phase per launch
(mds_fedce_omega_identify) and ``rollout`` the CE phase / do_control loop (mds_rollout_dlqr_omega_fused).  The Riccati solve runs in
float64 on the host by default (scipy; the gain is uploaded per env with mds_set_dlqr_omega_gain) or, with
``compute_controller(solver="device")``, for every env at once on the device (mds_dlqr_omega_solve_gain).

Arrays gain a leading env axis when ``env.NUM_ENVS > 1``: theta [E, 13D, 9D], P [E, D, 13, 13], K [E, 4D, 9D]."""
from __future__ import annotations

import ctypes as C

import numpy as np
import scipy.linalg as la
import torch

from ... import _capi as capi
from ..._device import stream_ptr, to_device
from ..base_controller import BaseController

UPDATE_NONE, UPDATE_ALL, UPDATE_SKIP_FIRST = 0, 1, 2      # mds_fedce_omega_identify's `update`
UPDATE_COV_ALL, UPDATE_COV_SKIP_FIRST = 3, 4              # the same two in the covariance form (theta_update)
FORMS = ("theta_update2", "theta_update")


class DecentralizedLQROmega(BaseController):
    def __init__(self, env, lin_models, debug=False):
        super().__init__(env)
        self.m, self.n = 9, 4
        self.mn = self.m + self.n
        m, n = self.m, self.n
        max_thrust = env.MAX_THRUST
        rflat = [1 / (max_thrust ** 2), 1 / (0.1 ** 2), 1 / (0.1 ** 2), 1 / (0.1 ** 2)]
        max_vel_error, max_pos_error = .15, .05
        max_yaw_error, max_pitch_roll_error = np.pi / 40, np.pi / 20
        qflat = [1 / (max_pitch_roll_error ** 2), 1 / (max_pitch_roll_error ** 2), 1 / (max_yaw_error ** 2),
                 1 / (max_vel_error ** 2), 1 / (max_vel_error ** 2), 1 / (max_vel_error ** 2),
                 1 / (max_pos_error ** 2), 1 / (max_pos_error ** 2), 1 / (max_pos_error ** 2)]
        self.lin_models = lin_models
        self.num_robots = D = len(lin_models)
        if D != env.NUM_DRONES:
            raise ValueError(f"{D} linear models for {env.NUM_DRONES} drones per env")
        self.num_envs = env.NUM_ENVS
        self.ind_Q = np.diag(qflat)
        self.ind_R = np.diag(rflat)
        self.Q = np.kron(np.eye(D), self.ind_Q)
        self.R = np.kron(np.eye(D), self.ind_R)
        if debug:
            with np.printoptions(precision=3, suppress=True, linewidth=100000):
                print(f"Full Q: \n{self.Q}")
                print(f"Full R: \n{self.R}")
        self.Astar = np.zeros((m * D, m * D))
        self.Bstar = np.zeros((m * D, n * D))
        for i, agent in enumerate(lin_models):
            assert agent.Ahat.shape == (m, m)
            assert agent.Bhat.shape == (m, n)
            self.Astar[i * m:(i + 1) * m, i * m:(i + 1) * m] = agent.Ahat
            self.Bstar[i * m:(i + 1) * m, i * n:(i + 1) * n] = agent.Bhat
        if any(not all(np.array_equal(getattr(a, k), getattr(lin_models[0], k)) for k in ("A", "B", "Ahat", "Bhat")) for a in lin_models[1:]):
            raise NotImplementedError("DecentralizedLQROmega: per-drone linear models that differ are not built (one model for every drone)")
        th0 = np.ascontiguousarray(np.hstack([lin_models[0].Ahat, lin_models[0].Bhat]).T)
        capi.check(env._lib.mds_fedce_omega_init(env._h, capi.as_double_ptr(np.ascontiguousarray(np.eye(self.mn))), capi.as_double_ptr(th0)),
                   "mds_fedce_omega_init")
        # a new reference object starts with fresh ThrustOmegaControllers (:70): the PID memory lives as long as this object
        capi.check(env._lib.mds_lowlevel_reset(env._h, C.c_void_p(stream_ptr(env.device))), "mds_lowlevel_reset")
        self._form = FORMS[0]                                     # the update form of the last identify call (what P returns)
        self.K = None
        self.are_status = np.ones(self.num_envs, dtype=bool)     # False: the last compute_controller kept that env's previous K
        self.status = np.zeros((self.num_envs, D), dtype=np.int32)   # or of the identify calls' failure bits per drone (0: none)
        self._status_dev = torch.zeros((self.num_envs, D), dtype=torch.int32, device=env.device)
        self.desired_positions = np.zeros((D, 3))
        self.desired_vels = np.zeros((D, 3))
        self.desired_yaws = np.zeros(D)
        self.desired_omegas = np.zeros(D)

    # ------------------------------------------------------------------ device state <-> the reference's arrays
    def _get(self):
        n = self.env.n
        th = np.zeros((n, self.mn, self.m))
        V = np.zeros((n, self.mn, self.mn))
        capi.check(self.env._lib.mds_fedce_omega_get(self.env._h, capi.as_double_ptr(th), capi.as_double_ptr(V)), "mds_fedce_omega_get")
        return th.reshape(self.num_envs, self.num_robots, self.mn, self.m), V.reshape(self.num_envs, self.num_robots, self.mn, self.mn)

    def _one(self, a):
        return a[0] if self.num_envs == 1 else a

    def _stack(self, th):
        """per-drone theta_i [.., D, 13, 9] -> the reference's block layout [.., 13D, 9D]"""
        D, m, n = th.shape[-3], self.m, self.n
        out = np.zeros(th.shape[:-3] + (self.mn * D, m * D))
        for i in range(D):
            out[..., i * m:(i + 1) * m, m * i:m * (i + 1)] = th[..., i, :m, :]
            out[..., m * D + n * i:m * D + n * (i + 1), m * i:m * (i + 1)] = th[..., i, m:, :]
        return out

    @property
    def theta(self):
        """[13D, 9D] = [Astar^T; Bstar^T] (a copy of the device state: write back with overwrite_theta)."""
        return self._one(self._stack(self._get()[0]))

    @property
    def P(self):
        """[D, 13, 13]: what the reference's ``self.P`` holds for the update form last used by ``identify``: the information matrix V
        after theta_update2 phases (the reference's name for it, :115), its inverse W after theta_update phases (:130, :139).  The
        device carries both as an inverse pair through either form."""
        if self._form == "theta_update":
            n = self.env.n
            W = np.zeros((n, self.mn, self.mn))
            capi.check(self.env._lib.mds_fedce_omega_get_cov(self.env._h, capi.as_double_ptr(W)), "mds_fedce_omega_get_cov")
            return self._one(W.reshape(self.num_envs, self.num_robots, self.mn, self.mn))
        return self._one(self._get()[1])

    def get_thetai(self, i):
        return self._one(self._get()[0][:, i])

    def overwrite_theta(self, theta_new, i):
        """theta_new [13,9] (or [E,13,9]) for drone i."""
        th, _ = self._get()
        th[:, i] = np.broadcast_to(np.asarray(theta_new, dtype=np.float64), th[:, i].shape)
        th = np.ascontiguousarray(th.reshape(-1, self.mn, self.m))
        capi.check(self.env._lib.mds_fedce_omega_set(self.env._h, capi.as_double_ptr(th), None), "mds_fedce_omega_set")

    # ------------------------------------------------------------------ noise (sigma1 / sigma_explore, :140-154)
    def sigma1(self):
        thrust = np.random.uniform(.7 * self.env.M * self.env.G, 1.5 * self.env.M * self.env.G)
        ang_vs = np.random.uniform(-0.00001, 0.00001, 3)
        return np.hstack([thrust, ang_vs])

    def sigma_explore(self):
        thrust_cov = .005 * self.env.M * self.env.G
        thrust = np.random.normal(self.env.M * self.env.G, thrust_cov)
        angv = np.random.normal(0, [0.000000005, 0.000000005, 0.000000005])
        return np.hstack([thrust, angv])

    def draw_inputs(self, kind, T, generator=None):
        """[T, E, D, 4] float64 device tensor of raw inputs, kind 'warmup' (sigma1) or 'explore' (sigma_explore).  One env: the global
        np.random in the reference's order (step, drone; thrust then rates).  Several envs: drawn on the device from ``generator``."""
        env, E, D = self.env, self.num_envs, self.num_robots
        if E == 1:
            f = self.sigma1 if kind == "warmup" else self.sigma_explore
            u = np.array([[f() for _ in range(D)] for _ in range(T)]).reshape(T, 1, D, 4)
            return torch.as_tensor(u, dtype=torch.float64, device=env.device)
        mg = env.M * env.G
        if kind == "warmup":
            r = torch.rand((T, E, D, 4), dtype=torch.float64, device=env.device, generator=generator)
            lo = torch.tensor([.7 * mg, -1e-5, -1e-5, -1e-5], dtype=torch.float64, device=env.device)
            hi = torch.tensor([1.5 * mg, 1e-5, 1e-5, 1e-5], dtype=torch.float64, device=env.device)
            return lo + (hi - lo) * r
        z = torch.randn((T, E, D, 4), dtype=torch.float64, device=env.device, generator=generator)
        mean = torch.tensor([mg, 0.0, 0.0, 0.0], dtype=torch.float64, device=env.device)
        sd = torch.tensor([.005 * mg, 5e-9, 5e-9, 5e-9], dtype=torch.float64, device=env.device)
        return mean + sd * z

    # ------------------------------------------------------------------ the hot paths
    def identify(self, u, x_des, update, log_obs=False, log_theta=False, form="theta_update2"):
        """One warm-up or exploration phase of fedCE_iteration on the device: u [T,E,D,4] (or [T,D,4]) raw inputs, x_des [D,9] or
        [E,D,9] (reference layout [rpy, vel, pos]); ``update``: UPDATE_NONE, UPDATE_ALL or UPDATE_SKIP_FIRST (the reference's
        `if i != 0` for a call that covers a whole phase); ``form``: "theta_update2" (the information form, EnvGeometricOmega.py) or
        "theta_update" (the covariance form, CBFTest.py:192, :260), which maps UPDATE_ALL / UPDATE_SKIP_FIRST to UPDATE_COV_ALL /
        UPDATE_COV_SKIP_FIRST.  Returns (obs log [T,E,D,20] or None, last obs, theta log [T,E,D,13,9] or
        None); the failure bits of the forward prediction accumulate in ``status``."""
        env, E, D = self.env, self.num_envs, self.num_robots
        if form not in FORMS:
            raise ValueError(f"form must be one of {FORMS}, not {form!r}")
        update = int(update)
        if form == "theta_update" and update in (UPDATE_ALL, UPDATE_SKIP_FIRST):
            update += 2
        if update != UPDATE_NONE:
            self._form = FORMS[update > UPDATE_SKIP_FIRST]
        u = to_device(u, env.device, torch.float64).reshape(-1, env.n, 4).contiguous()
        T = u.shape[0]
        xd = to_device(np.broadcast_to(np.asarray(x_des, dtype=np.float64), (E, D, self.m)), env.device, torch.float64)
        obs_log = torch.empty((T, E, D, capi.OBS_DIM), dtype=env.dtype, device=env.device) if (log_obs and T) else None
        thl = torch.empty((T, E, D, self.mn, self.m), dtype=torch.float64, device=env.device) if (log_theta and T) else None

        def p(t):
            return C.c_void_p(t.data_ptr() if t is not None else None)
        capi.check(env._lib.mds_fedce_omega_identify(env._h, C.c_int(T), p(u), p(xd), C.c_int(int(update)), p(obs_log), p(thl),
                                                     p(self._status_dev), C.c_void_p(env._obs.data_ptr()), C.c_void_p(stream_ptr(env.device))),
                   "mds_fedce_omega_identify")
        env.step_counter += T * env.PYB_STEPS_PER_CTRL
        self.status = self._status_dev.cpu().numpy()
        return obs_log, env._obs, thl

    def _are_gain(self, A, B, force_diagonal):
        """K [4D, 9D] of one env's model on the host (scipy); raises what solve_continuous_are raises."""
        D, m, n = self.num_robots, self.m, self.n
        if not force_diagonal:
            P = la.solve_continuous_are(A, B, self.Q, self.R, e=None, s=None, balanced=True)
            return la.solve(self.R, B.T @ P)
        K = np.zeros((n * D, m * D))
        for i in range(D):
            Ai = A[m * i:m * (i + 1), m * i:m * (i + 1)]
            Bi = B[m * i:m * (i + 1), n * i:n * (i + 1)]
            Pi = la.solve_continuous_are(Ai, Bi, self.ind_Q, self.ind_R, e=None, s=None, balanced=True)
            K[n * i:n * (i + 1), m * i:m * (i + 1)] = la.solve(self.ind_R, Bi.T @ Pi)   # (the reference's R is 4D x 4D here)
        return K

    def compute_controller(self, force_diagonal=False, solver="host", host_fallback=True):
        """K from the continuous ARE on the identified model (:185-204) in float64.  ``solver="host"``: every env on the host (scipy),
        then uploaded.  One env: an ARE failure raises as in the reference.  Several: that env keeps its previous K (zeros before the
        first) and are_status[e] is False.  ``solver="device"``: every env at once on the device (mds_dlqr_omega_solve_gain);
        care_status [E] keeps its status bits and care_iters [E] its iteration counts.  An env it flags is solved again on the host when
        ``host_fallback`` is set; one that stays unsolved is treated as above (one env: np.linalg.LinAlgError)."""
        D, E, m, n = self.num_robots, self.num_envs, self.m, self.n
        if solver == "device":
            return self._compute_controller_device(force_diagonal, host_fallback)
        if solver != "host":
            raise ValueError(f"solver must be 'host' or 'device', not {solver!r}")
        th = self._stack(self._get()[0])                            # [E, 13D, 9D]
        Kprev = None if self.K is None else np.broadcast_to(self.K, (E, n * D, m * D))
        K = np.zeros((E, n * D, m * D))
        status = np.ones(E, dtype=bool)
        for e in range(E):
            A = th[e, :m * D, :].T
            B = th[e, m * D:, :].T
            try:
                K[e] = self._are_gain(A, B, force_diagonal)
            except (np.linalg.LinAlgError, ValueError):
                if E == 1:
                    raise
                status[e] = False
                K[e] = Kprev[e] if Kprev is not None else 0.0
        self.are_status = status
        self.K = self._one(K)
        self.upload_gain(K)

    def _compute_controller_device(self, force_diagonal, host_fallback):
        env, D, E, m, n = self.env, self.num_robots, self.num_envs, self.m, self.n
        Q = np.ascontiguousarray(np.kron(np.eye(D), self.ind_Q) if force_diagonal else self.Q, dtype=np.float64)
        R = np.ascontiguousarray(self.R, dtype=np.float64)
        K_dev = torch.empty((E, n * D, m * D), dtype=torch.float64, device=env.device)
        st_dev = torch.empty(E, dtype=torch.int32, device=env.device)
        it_dev = torch.empty(E, dtype=torch.int32, device=env.device)
        capi.check(env._lib.mds_dlqr_omega_solve_gain(env._h, capi.as_double_ptr(Q), capi.as_double_ptr(R), C.c_int(0),
                                                      C.c_void_p(K_dev.data_ptr()), C.c_void_p(st_dev.data_ptr()), C.c_void_p(it_dev.data_ptr()),
                                                      C.c_void_p(stream_ptr(env.device))), "mds_dlqr_omega_solve_gain")
        K = K_dev.cpu().numpy()
        self.care_status, self.care_iters = st_dev.cpu().numpy(), it_dev.cpu().numpy()
        status = self.care_status == 0
        Kprev = None if self.K is None else np.broadcast_to(self.K, (E, n * D, m * D))
        flagged = np.flatnonzero(~status)
        th = self._stack(self._get()[0]) if (host_fallback and len(flagged)) else None
        resolved = False
        for e in flagged:
            try:
                if not host_fallback:
                    raise np.linalg.LinAlgError(f"mds_dlqr_omega_solve_gain: env {e} ended with status {self.care_status[e]}")
                K[e] = self._are_gain(th[e, :m * D, :].T, th[e, m * D:, :].T, force_diagonal)
                status[e] = resolved = True
            except (np.linalg.LinAlgError, ValueError):
                if E == 1:
                    raise
                K[e] = Kprev[e] if Kprev is not None else 0.0
        self.are_status = status
        self.K = self._one(K)
        if resolved:                                                # the device already holds every other env's gain
            self.upload_gain(K)

    def upload_gain(self, K):
        """K [4D,9D] (every env) or [E,4D,9D] -> the device (mds_set_dlqr_omega_gain)."""
        D, E = self.num_robots, self.num_envs
        K = np.ascontiguousarray(np.broadcast_to(np.asarray(K, dtype=np.float64), (E, self.n * D, self.m * D)))
        capi.check(self.env._lib.mds_set_dlqr_omega_gain(self.env._h, capi.as_double_ptr(K)), "mds_set_dlqr_omega_gain")

    def set_desired_trajectory(self, robot_idx, desired_pos, desired_vel, desired_acc, desired_yaw, desired_omega):
        self.desired_positions[robot_idx] = desired_pos
        self.desired_vels[robot_idx] = desired_vel
        self.desired_yaws[robot_idx] = desired_yaw
        self.desired_omegas[robot_idx] = desired_omega

    def _des(self):
        E, D = self.num_envs, self.num_robots
        des = np.zeros((E, D, capi.DES_DIM))
        des[..., 0:3], des[..., 3:6] = self.desired_positions, self.desired_vels
        des[..., 9], des[..., 10] = self.desired_yaws, self.desired_omegas
        return to_device(des, self.env.device, self.env.dtype)

    def compute(self, obs, skip_low_level=False):
        """-> (action [D,4] or None, capped u [D,4]) as the reference (:212-231); with several envs obs [E,D,20] -> ([E,D,4], [E,D,4]).
        One kernel call (mds_dlqr_omega_compute); skip_low_level leaves the PID memory untouched."""
        env, E, D = self.env, self.num_envs, self.num_robots
        if isinstance(obs, torch.Tensor):
            obs = obs.double().cpu().numpy()
        o = to_device(np.broadcast_to(np.asarray(obs, dtype=np.float64), (E, D, capi.OBS_DIM)), env.device, env.dtype)
        d = self._des()
        u = torch.empty((E, D, 4), dtype=env.dtype, device=env.device)
        act = None if skip_low_level else torch.empty_like(u)
        capi.check(env._lib.mds_dlqr_omega_compute(env._h, C.c_void_p(o.data_ptr()), C.c_void_p(d.data_ptr()), C.c_void_p(u.data_ptr()),
                                                   C.c_void_p(act.data_ptr() if act is not None else None), C.c_void_p(stream_ptr(env.device))),
                   "mds_dlqr_omega_compute")
        uu = u.double().cpu().numpy()
        return (None if act is None else self._one(act.double().cpu().numpy())), self._one(uu)

    def cap_u(self, u):
        u[:, 0] = np.clip(u[:, 0], 4 * (9440.3 ** 2 * self.env.KF), self.env.MAX_THRUST)
        return u

    def compute_low_level(self, u, obs, robot_idx):
        """ThrustOmegaController.computeControlFromInput for every drone at once (:238-249): u [(E,)D,4], obs [(E,)D,20] -> RPM, on the
        handle's PID memory (mds_thrust_omega_compute).  ``robot_idx`` must be None: the reference's per-drone call order (drone by drone
        inside one control step) is what one batched call does."""
        if robot_idx is not None:
            raise NotImplementedError("compute_low_level: pass every drone's u and obs with robot_idx=None (one batched call per control step)")
        env, E, D = self.env, self.num_envs, self.num_robots
        uu = to_device(np.broadcast_to(np.asarray(u, dtype=np.float64), (E, D, 4)), env.device, env.dtype)
        o = to_device(np.broadcast_to(np.asarray(obs, dtype=np.float64), (E, D, capi.OBS_DIM)), env.device, env.dtype)
        rpm = torch.empty_like(uu)
        capi.check(env._lib.mds_thrust_omega_compute(env._h, C.c_void_p(uu.data_ptr()), C.c_void_p(o.data_ptr()), C.c_void_p(rpm.data_ptr()),
                                                     C.c_void_p(stream_ptr(env.device))), "mds_thrust_omega_compute")
        return self._one(rpm.double().cpu().numpy())

    def rollout(self, t0, n_steps, log=True):
        """n_steps of the dLQR loop in one launch (trajectories from env.set_trajectories) -> obs log [T,E,D,20] or None."""
        env = self.env
        out = torch.empty((n_steps, env.NUM_ENVS, env.NUM_DRONES, capi.OBS_DIM), dtype=env.dtype, device=env.device) if log else None
        capi.check(env._lib.mds_rollout_dlqr_omega_fused(env._h, C.c_double(t0), C.c_int(n_steps), C.c_void_p(out.data_ptr() if log else None),
                                                         C.c_void_p(env._obs.data_ptr()), C.c_void_p(stream_ptr(env.device))),
                   "mds_rollout_dlqr_omega_fused")
        env.step_counter += n_steps * env.PYB_STEPS_PER_CTRL
        return out

    # ------------------------------------------------------------------ host helpers of the reference's API
    def error_state(self, x, x_des):
        """DecentralizedLQROmega.error_state (:174-183) for one 9-vector pair (host helper; the kernels use error_state9)."""
        from scipy.spatial.transform import Rotation
        e = np.array(x, dtype=np.float64)
        R_eq = Rotation.from_euler('xyz', [0, 0, x_des[2]]).as_matrix()
        R = Rotation.from_euler('xyz', e[:3]).as_matrix()
        e[:3] = Rotation.from_matrix(R_eq.T @ R).as_euler('xyz')
        e[6:] = R_eq.T @ (x[6:] - x_des[6:])
        e[3:6] = R_eq.T @ (x[3:6] - x_des[3:6])
        return e

    def cost(self, x, u):
        return x.T @ self.Q @ x + u.T @ self.R @ u

    def theta_update2(self, phis, xtp1s):
        raise NotImplementedError("theta_update2 per call is not built: identify() runs it inside the identification kernel for whole phases")

    def theta_update(self, phis, xtp1s):
        raise NotImplementedError("theta_update per call is not built: identify(form=\"theta_update\") runs it inside the identification "
                                  "kernel for whole phases")

    def forward_predict(self, *a, **k):
        raise NotImplementedError("forward_predict (solve_ivp) runs inside the identification kernel (rk45_linear) and has no host entry")

    def solve_xtp1(self, *a, **k):
        raise NotImplementedError("solve_xtp1 is not used by fedCE's default loop and is not built")

    def noisy_control(self, *a, **k):
        raise NotImplementedError("noisy_control is not used by fedCE's default loop and is not built")

    def LQR(self, *a, **k):
        raise NotImplementedError("LQR (the per-drone LQROmegaController warm-up, random_warmup=False) is not built")

"""control/dlqr/decentralized_lqr.py of the reference: ``DecentralizedLQR(env, lin_models)`` -- the 12-state decentralised LQR
whose models FedCE (simulations/EnvGeometric.py fedCE) identifies on line by recursive least squares.

The per-drone RLS state (P [16,16] and theta, float64 in every env dtype) lives on the device: ``identify`` runs a whole warm-up or
exploration phase of fedCE_iteration per launch (mds_fedce_identify) and ``rollout`` the CE phase / do_control loop
(mds_rollout_dlqr_fused).  The Riccati solve runs once per FedCE iteration in float64: on the host by default (scipy, one env after
the other, as control/lqr/lqr_controller.py does; the gain is uploaded per env with mds_set_dlqr_gain), or for every env at once on
the device with ``compute_controller(solver="device")`` (mds_dlqr_solve_gain, which writes the gains where the kernels read them).

Arrays gain a leading env axis when ``env.NUM_ENVS > 1``: theta [E, 16D, 12D], P [E, D, 16, 16], K [E, 4D, 12D]."""
from __future__ import annotations

import ctypes as C

import numpy as np
import scipy.linalg as la
import torch

from ... import _capi as capi
from ..._device import stream_ptr, to_device
from ..base_controller import BaseController

# x_des of the error state (reference layout): rpy, ang_v, vel, pos; the kernels read [2], [5], [6:9], [9:12]
U_RAW, U_ROUND_TRIP = 0, 1


class DecentralizedLQR(BaseController):
    def __init__(self, env, lin_models):
        super().__init__(env)
        max_thrust = env.MAX_THRUST
        max_torque_pitch_roll = 0.001
        max_torque_yaw = 0.001
        rflat = [1 / (max_thrust ** 2), 1 / (max_torque_pitch_roll ** 2), 1 / (max_torque_pitch_roll ** 2), 1 / (max_torque_yaw ** 2)]
        max_vel_error, max_pos_error = .15, .05
        max_yaw_error, max_pitch_roll_error = np.pi / 20, np.pi / 10
        max_pitch_yaw_rate_error, max_yaw_rate_error = .5, .5
        qflat = [1 / (max_pitch_roll_error ** 2), 1 / (max_pitch_roll_error ** 2), 1 / (max_yaw_error ** 2),
                 1 / (max_pitch_yaw_rate_error ** 2), 1 / (max_pitch_yaw_rate_error ** 2), 1 / (max_yaw_rate_error ** 2),
                 1 / (max_vel_error ** 2), 1 / (max_vel_error ** 2), 1 / (max_vel_error ** 2),
                 1 / (max_pos_error ** 2), 1 / (max_pos_error ** 2), 1 / (max_pos_error ** 2)]
        self.lin_models = lin_models
        self.num_robots = D = len(lin_models)
        if D != env.NUM_DRONES:
            raise ValueError(f"{D} linear models for {env.NUM_DRONES} drones per env")
        self.num_envs = env.NUM_ENVS
        self.pred_errors = [[] for _ in range(2 * D)]     # per update: a float (one env) or an [E] array
        self.pred_thetas = [[] for _ in range(D)]         # per update: [12,16] (one env) or [E,12,16]
        self.ind_Q = np.diag(qflat)
        self.ind_R = np.diag(rflat)
        self.Q = np.kron(np.eye(D), self.ind_Q)
        self.R = np.kron(np.eye(D), self.ind_R)
        multi_xy_err = .1                                  # couples the xy positions of drones 0 and 1 only (:44-53)
        self.Q[np.index_exp[9:11, 21:23]] = -1 / (multi_xy_err ** 2)
        self.Q[np.index_exp[21:23, 9:11]] = -1 / (multi_xy_err ** 2)
        for m in lin_models:
            assert m.Ahat.shape == (12, 12) and m.Bhat.shape == (12, 4)
        self.Astar = np.zeros((12 * D, 12 * D))
        self.Bstar = np.zeros((12 * D, 4 * D))
        for i, m in enumerate(lin_models):
            self.Astar[i * 12:(i + 1) * 12, i * 12:(i + 1) * 12] = m.Ahat
            self.Bstar[i * 12:(i + 1) * 12, i * 4:(i + 1) * 4] = m.Bhat
        P0 = 20 * np.eye(16)
        P0[-3:, -3:] = 5_000_000 * np.eye(3)
        th0 = np.ascontiguousarray(np.hstack([lin_models[0].Ahat, lin_models[0].Bhat]).T)
        # One model for every drone: the device state starts from it, and the identification kernel's second pred_errors entry uses
        # the true model of the handle's constants (M, G, J) -- what LinearizedModel(env) gives every drone in the reference's scripts.
        if any(not all(np.array_equal(getattr(m, k), getattr(lin_models[0], k)) for k in ("A", "B", "Ahat", "Bhat")) for m in lin_models[1:]):
            raise NotImplementedError("DecentralizedLQR: per-drone linear models that differ are not built (one model for every drone)")
        capi.check(env._lib.mds_fedce_init(env._h, capi.as_double_ptr(np.ascontiguousarray(P0)), capi.as_double_ptr(th0)), "mds_fedce_init")
        self.K = None
        self.are_status = np.ones(self.num_envs, dtype=bool)     # False: the last compute_controller kept that env's previous K
        self.desired_positions = np.zeros((D, 3))
        self.desired_vels = np.zeros((D, 3))
        self.desired_yaws = np.zeros(D)
        self.desired_omegas = np.zeros(D)
        A_keep_1 = np.index_exp[(6, 7), (1, 0)]
        self.A_keep_2 = np.index_exp[(0, 1, 2), (3, 4, 5)]
        self.A_keep_3 = np.index_exp[(9, 10, 11), (6, 7, 8)]
        self.A_mask = np.zeros((12 * D, 12 * D))
        self.B_mask = np.zeros((12 * D, 4 * D))
        for i in range(D):
            a = self.A_mask[12 * i:12 * (i + 1), 12 * i:12 * (i + 1)]
            a[A_keep_1] = a[self.A_keep_2] = a[self.A_keep_3] = 1
            b = self.B_mask[12 * i:12 * (i + 1), 4 * i:4 * (i + 1)]
            b[3:6, 1:] = 1
            b[8, 0] = 1

    # ------------------------------------------------------------------ device state <-> the reference's arrays
    def _get(self):
        n = self.env.n
        th = np.zeros((n, 16, 12))
        P = np.zeros((n, 16, 16))
        capi.check(self.env._lib.mds_fedce_get(self.env._h, capi.as_double_ptr(th), capi.as_double_ptr(P)), "mds_fedce_get")
        return th.reshape(self.num_envs, self.num_robots, 16, 12), P.reshape(self.num_envs, self.num_robots, 16, 16)

    def _one(self, a):
        return a[0] if self.num_envs == 1 else a

    @staticmethod
    def _stack(th):
        """per-drone theta_i [.., D, 16, 12] -> the reference's block layout [.., 16D, 12D]"""
        D = th.shape[-3]
        out = np.zeros(th.shape[:-3] + (16 * D, 12 * D))
        for i in range(D):
            out[..., i * 12:(i + 1) * 12, 12 * i:12 * (i + 1)] = th[..., i, :12, :]
            out[..., 12 * D + 4 * i:12 * D + 4 * (i + 1), 12 * i:12 * (i + 1)] = th[..., i, 12:, :]
        return out

    @property
    def theta(self):
        """[16D, 12D] = [Astar^T; Bstar^T] (a copy of the device state: write back with overwrite_theta)."""
        return self._one(self._stack(self._get()[0]))

    @property
    def P(self):
        return self._one(self._get()[1])

    def get_thetai(self, i):
        return self._one(self._get()[0][:, i])

    def overwrite_theta(self, theta_new, i):
        """theta_new [16,12] (or [E,16,12]) for drone i, projected on the way in (the device keeps the free entries only)."""
        th, _ = self._get()
        th[:, i] = np.broadcast_to(np.asarray(theta_new, dtype=np.float64), th[:, i].shape)
        th = np.ascontiguousarray(th.reshape(-1, 16, 12))
        capi.check(self.env._lib.mds_fedce_set(self.env._h, capi.as_double_ptr(th), None), "mds_fedce_set")

    def project_theta(self):
        """A no-op on the device state: theta is held projected (its 12 free entries per drone)."""
        return None

    # ------------------------------------------------------------------ noise (sigma1 / sigma_explore)
    def sigma1(self):
        thrust = np.random.uniform(.8 * self.env.M * self.env.G, 1.5 * self.env.M * self.env.G)
        torques = np.random.uniform(-0.00001, 0.00001, 3)
        return np.hstack([thrust, torques])

    def sigma_explore(self):
        thrust_cov = .15 * self.env.M * self.env.G
        torque_xy_cov = 0.005 * self.env.MAX_XY_TORQUE
        torque_z_cov = 0.005 * self.env.MAX_Z_TORQUE
        thrust = np.random.normal(self.env.M * self.env.G, thrust_cov)
        torques = np.random.normal(0, [torque_xy_cov, torque_xy_cov, torque_z_cov])
        return np.hstack([thrust, torques])

    def draw_inputs(self, kind, T, generator=None):
        """[T, E, D, 4] float64 device tensor of raw inputs, kind 'warmup' (sigma1) or 'explore' (sigma_explore).  One env: the global
        np.random in the reference's order (step, drone; thrust then torques), so np.random.seed reproduces its draws.  Several envs:
        drawn on the device from ``generator`` (a torch.Generator on the env's device), every env its own stream of draws."""
        env, E, D = self.env, self.num_envs, self.num_robots
        if E == 1:
            f = self.sigma1 if kind == "warmup" else self.sigma_explore
            u = np.array([[f() for _ in range(D)] for _ in range(T)]).reshape(T, 1, D, 4)
            return torch.as_tensor(u, dtype=torch.float64, device=env.device)
        mg = env.M * env.G
        if kind == "warmup":
            r = torch.rand((T, E, D, 4), dtype=torch.float64, device=env.device, generator=generator)
            lo = torch.tensor([.8 * mg, -1e-5, -1e-5, -1e-5], dtype=torch.float64, device=env.device)
            hi = torch.tensor([1.5 * mg, 1e-5, 1e-5, 1e-5], dtype=torch.float64, device=env.device)
            return lo + (hi - lo) * r
        z = torch.randn((T, E, D, 4), dtype=torch.float64, device=env.device, generator=generator)
        mean = torch.tensor([mg, 0.0, 0.0, 0.0], dtype=torch.float64, device=env.device)
        sd = torch.tensor([.15 * mg, 0.005 * env.MAX_XY_TORQUE, 0.005 * env.MAX_XY_TORQUE, 0.005 * env.MAX_Z_TORQUE],
                          dtype=torch.float64, device=env.device)
        return mean + sd * z

    # ------------------------------------------------------------------ the hot paths
    def identify(self, u, u_mode, x_des, update, log_obs=False, record=True):
        """One warm-up (u_mode U_RAW) or exploration phase (U_ROUND_TRIP) of fedCE_iteration on the device: u [T,E,D,4] (or [T,D,4])
        raw inputs, x_des [D,12] or [E,D,12] (reference layout).  With ``update`` every step runs approx_theta_update and, with
        ``record``, appends to pred_errors / pred_thetas.  Returns the observation log [T,E,D,20] (log_obs) and the last obs."""
        env, E, D = self.env, self.num_envs, self.num_robots
        u = to_device(u, env.device, torch.float64).reshape(-1, env.n, 4)
        T = u.shape[0]
        xd = to_device(np.broadcast_to(np.asarray(x_des, dtype=np.float64), (E, D, 12)), env.device, torch.float64)
        obs_log = torch.empty((T, E, D, capi.OBS_DIM), dtype=env.dtype, device=env.device) if (log_obs and T) else None
        want = bool(update and record and T)
        perr = torch.empty((T, E, D, 2), dtype=torch.float64, device=env.device) if want else None
        thl = torch.empty((T, E, D, 12), dtype=torch.float64, device=env.device) if want else None

        def p(t):
            return C.c_void_p(t.data_ptr() if t is not None else None)
        capi.check(env._lib.mds_fedce_identify(env._h, C.c_int(T), p(u), C.c_int(u_mode), p(xd), C.c_int(int(bool(update))), p(obs_log),
                                               p(perr), p(thl), C.c_void_p(env._obs.data_ptr()), C.c_void_p(stream_ptr(env.device))),
                   "mds_fedce_identify")
        env.step_counter += T * env.PYB_STEPS_PER_CTRL
        if want:
            self._record(perr.cpu().numpy(), thl.cpu().numpy())
        return obs_log, env._obs

    def _record(self, perr, free):
        """pred_errors / pred_thetas entries from the kernel's logs: perr [T,E,D,2], free [T,E,D,12]."""
        D = self.num_robots
        th = np.zeros(free.shape[:3] + (12, 16))                   # hstack([Ahat, Bhat]) [12,16]
        th[..., 0:3, 3:6] = np.eye(3)
        th[..., 9:12, 6:9] = np.eye(3)
        th[..., 6, 1] = free[..., 0]
        th[..., 7, 0] = free[..., 1]
        th[..., 3:6, 13:16] = free[..., 2:11].reshape(free.shape[:3] + (3, 3))
        th[..., 8, 12] = free[..., 11]
        for t in range(perr.shape[0]):
            for i in range(D):
                self.pred_errors[i].append(self._one(perr[t, :, i, 0]))
                self.pred_errors[i + D].append(self._one(perr[t, :, i, 1]))
                self.pred_thetas[i].append(self._one(th[t, :, i]))

    def _are_gain(self, A, B, force_diagonal):
        """K [4D, 12D] of one env's model on the host (scipy); raises what solve_continuous_are raises."""
        D = self.num_robots
        if not force_diagonal:
            P = la.solve_continuous_are(A, B, self.Q, self.R, e=None, s=None, balanced=True)
            return la.solve(self.R, B.T @ P)
        K = np.zeros((4 * D, 12 * D))
        for i in range(D):
            Ai = A[12 * i:12 * (i + 1), 12 * i:12 * (i + 1)]
            Bi = B[12 * i:12 * (i + 1), 4 * i:4 * (i + 1)]
            Pi = la.solve_continuous_are(Ai, Bi, self.ind_Q, self.ind_R, e=None, s=None, balanced=True)
            K[4 * i:4 * (i + 1), 12 * i:12 * (i + 1)] = la.solve(self.ind_R, Bi.T @ Pi)   # (the reference's R is 4D x 4D here)
        return K

    def compute_controller(self, force_diagonal=False, solver="host", host_fallback=True):
        """K from the continuous ARE on the identified model (:300-317) in float64.  ``solver="host"``: every env on the host (scipy),
        then uploaded.  One env: an ARE failure raises as in the reference.  Several: that env keeps its previous K (zeros before the
        first) and are_status[e] is False.  ``solver="device"``: every env at once on the device (mds_dlqr_solve_gain); care_status [E]
        keeps its status bits and care_iters [E] its iteration counts.  An env it flags is solved again on the host when
        ``host_fallback`` is set; one that stays unsolved is treated as above (one env: np.linalg.LinAlgError)."""
        D, E = self.num_robots, self.num_envs
        if solver == "device":
            return self._compute_controller_device(force_diagonal, host_fallback)
        if solver != "host":
            raise ValueError(f"solver must be 'host' or 'device', not {solver!r}")
        th = self._stack(self._get()[0])                            # [E, 16D, 12D]
        Kprev = None if self.K is None else np.broadcast_to(self.K, (E, 4 * D, 12 * D))
        K = np.zeros((E, 4 * D, 12 * D))
        status = np.ones(E, dtype=bool)
        for e in range(E):
            A = th[e, :12 * D, :].T
            B = th[e, 12 * D:, :].T
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
        env, D, E = self.env, self.num_robots, self.num_envs
        Q = np.ascontiguousarray(np.kron(np.eye(D), self.ind_Q) if force_diagonal else self.Q, dtype=np.float64)
        R = np.ascontiguousarray(self.R, dtype=np.float64)
        K_dev = torch.empty((E, 4 * D, 12 * D), dtype=torch.float64, device=env.device)
        st_dev = torch.empty(E, dtype=torch.int32, device=env.device)
        it_dev = torch.empty(E, dtype=torch.int32, device=env.device)
        capi.check(env._lib.mds_dlqr_solve_gain(env._h, capi.as_double_ptr(Q), capi.as_double_ptr(R), C.c_int(0), C.c_void_p(K_dev.data_ptr()),
                                                C.c_void_p(st_dev.data_ptr()), C.c_void_p(it_dev.data_ptr()), C.c_void_p(stream_ptr(env.device))),
                   "mds_dlqr_solve_gain")
        K = K_dev.cpu().numpy()
        self.care_status, self.care_iters = st_dev.cpu().numpy(), it_dev.cpu().numpy()
        status = self.care_status == 0
        Kprev = None if self.K is None else np.broadcast_to(self.K, (E, 4 * D, 12 * D))
        flagged = np.flatnonzero(~status)
        th = self._stack(self._get()[0]) if (host_fallback and len(flagged)) else None
        resolved = False
        for e in flagged:
            try:
                if not host_fallback:
                    raise np.linalg.LinAlgError(f"mds_dlqr_solve_gain: env {e} ended with status {self.care_status[e]}")
                K[e] = self._are_gain(th[e, :12 * D, :].T, th[e, 12 * D:, :].T, force_diagonal)
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
        """K [4D,12D] (every env) or [E,4D,12D] -> the device (mds_set_dlqr_gain).  The layout the kernels read is documented in
        include/mds.h, so a device-side Riccati solver can later write it directly."""
        D, E = self.num_robots, self.num_envs
        K = np.ascontiguousarray(np.broadcast_to(np.asarray(K, dtype=np.float64), (E, 4 * D, 12 * D)))
        capi.check(self.env._lib.mds_set_dlqr_gain(self.env._h, capi.as_double_ptr(K)), "mds_set_dlqr_gain")

    def set_desired_trajectory(self, robot_idx, desired_pos, desired_vel, desired_acc, desired_yaw, desired_omega):
        self.desired_positions[robot_idx] = desired_pos
        self.desired_vels[robot_idx] = desired_vel
        self.desired_yaws[robot_idx] = desired_yaw
        self.desired_omegas[robot_idx] = desired_omega

    def compute(self, obs, skip_low_level=False):
        """-> (action [D,4], u [4D]) as the reference (:326-342); with several envs obs [E,D,20] -> ([E,D,4], [E,4D]).  One kernel call
        (mds_dlqr_compute) with the gain of the last compute_controller / upload_gain."""
        env, E, D = self.env, self.num_envs, self.num_robots
        o = to_device(np.broadcast_to(np.asarray(obs, dtype=np.float64), (E, D, capi.OBS_DIM)), env.device, env.dtype)
        des = np.zeros((E, D, capi.DES_DIM))
        des[..., 0:3], des[..., 3:6] = self.desired_positions, self.desired_vels
        des[..., 9], des[..., 10] = self.desired_yaws, self.desired_omegas
        d = to_device(des, env.device, env.dtype)
        u = torch.empty((E, D, 4), dtype=env.dtype, device=env.device)
        act = torch.empty_like(u)
        capi.check(env._lib.mds_dlqr_compute(env._h, C.c_void_p(o.data_ptr()), C.c_void_p(d.data_ptr()), C.c_void_p(u.data_ptr()),
                                             C.c_void_p(act.data_ptr()), C.c_void_p(stream_ptr(env.device))), "mds_dlqr_compute")
        a = act.double().cpu().numpy()
        uu = u.double().cpu().numpy().reshape(E, 4 * D)
        return self._one(a), self._one(uu)

    def rollout(self, t0, n_steps, log=True):
        """n_steps of the dLQR loop in one launch (trajectories from env.set_trajectories) -> obs log [T,E,D,20] or None."""
        env = self.env
        out = torch.empty((n_steps, env.NUM_ENVS, env.NUM_DRONES, capi.OBS_DIM), dtype=env.dtype, device=env.device) if log else None
        capi.check(env._lib.mds_rollout_dlqr_fused(env._h, C.c_double(t0), C.c_int(n_steps), C.c_void_p(out.data_ptr() if log else None),
                                                   C.c_void_p(env._obs.data_ptr()), C.c_void_p(stream_ptr(env.device))), "mds_rollout_dlqr_fused")
        env.step_counter += n_steps * env.PYB_STEPS_PER_CTRL
        return out

    # ------------------------------------------------------------------ host helpers of the reference's API
    def error_state(self, x, x_des):
        """DecentralizedLQR.error_state (:288-298) for one 12-vector pair (host helper; the kernels share lqr12_error)."""
        from scipy.spatial.transform import Rotation
        e = np.array(x, dtype=np.float64)
        R_eq = Rotation.from_euler('xyz', [0, 0, x_des[2]]).as_matrix()
        R = Rotation.from_euler('xyz', e[:3]).as_matrix()
        e[:3] = Rotation.from_matrix(R_eq.T @ R).as_euler('xyz')
        e[9:] = R_eq.T @ (x[9:] - x_des[9:])
        e[6:9] = R_eq.T @ (x[6:9] - x_des[6:9])
        e[3:6] = R_eq.T @ (x[3:6] - x_des[3:6])
        return e

    def cost(self, x, u):
        return x.T @ self.Q @ x + u.T @ self.R @ u

    def approx_theta_update(self, phis, xtp1s):
        """One RLS step (:200-227) on caller-supplied phis [D,16] and e_{t+1} [D,12] (a leading env axis when E > 1), applied to
        the device state in float64 on the host (mds_fedce_get / mds_fedce_set) -- the per-call form of the update that
        ``identify`` runs inside the identification kernel for whole phases.  Appends to pred_errors / pred_thetas."""
        E, D = self.num_envs, self.num_robots
        phis = np.asarray(phis, dtype=np.float64).reshape(E, D, 16)
        xtp1s = np.asarray(xtp1s, dtype=np.float64).reshape(E, D, 12)
        dt = self.env.CTRL_TIMESTEP
        th, P = self._get()
        perr = np.zeros((1, E, D, 2))
        free = np.zeros((1, E, D, 12))
        for e in range(E):
            for i in range(D):
                phi = phis[e, i].reshape((16, 1))
                x_tp1 = xtp1s[e, i]
                x_dot = np.zeros((12,))                                       # est_x_dot (:185-198)
                x_dot[0:3] = x_tp1[3:6]
                x_dot[3:6] = (x_tp1[3:6] - phi[3:6, 0]) / dt
                x_dot[6:9] = (x_tp1[6:9] - phi[6:9, 0]) / dt
                x_dot[9:] = x_tp1[6:9]
                Pi, th_i = P[e, i].copy(), th[e, i].copy()
                L = Pi @ phi @ np.linalg.inv(1 + phi.T @ Pi @ phi)
                th[e, i] = th_i + L @ (x_dot.T - phi.T @ th_i)
                P[e, i] = (np.eye(16) - L @ phi.T) @ Pi
                m = self.lin_models[i]
                perr[0, e, i] = [np.linalg.norm(x_dot.T - phi.T @ th_i), np.linalg.norm(x_dot.T - phi.T @ np.hstack([m.A, m.B]).T)]
                t = th[e, i]                                                  # the free entries after project_theta
                free[0, e, i] = [t[1, 6], t[0, 7], *t[13:16, 3:6].T.reshape(9), t[12, 8]]
        capi.check(self.env._lib.mds_fedce_set(self.env._h, capi.as_double_ptr(np.ascontiguousarray(th.reshape(-1, 16, 12))),
                                               capi.as_double_ptr(np.ascontiguousarray(P.reshape(-1, 16, 16)))), "mds_fedce_set")
        self._record(perr, free)

    def theta_update(self, phis, xtp1s):
        raise NotImplementedError("theta_update (solve_ivp forward prediction) is not used by fedCE and is not built")

    def theta_update2(self, phis, xtp1s):
        raise NotImplementedError("theta_update2 (solve_ivp forward prediction) is not used by fedCE and is not built")

    def forward_predict(self, *a, **k):
        raise NotImplementedError("forward_predict (solve_ivp) is not used by fedCE and is not built")

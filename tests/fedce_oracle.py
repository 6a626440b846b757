"""Float64 NumPy restatement of FedCE (simulations/EnvGeometric.py fedCE / fedCE_iteration, the default loop) and of the 12-state
DecentralizedLQR (control/dlqr/decentralized_lqr.py) it runs, on oracle.np_oracle.AviaryOracle's DYN physics in place of Bullet.

The noise is an input: ``noise[n] = (u_warm [25, D, 4] or None, u_explore [Texp, D, 4])`` per iteration, the raw draws of
``sigma1`` / ``sigma_explore`` in the order the reference makes them (step-major, then drone).  ``draw_reference_noise`` makes them
with the global ``np.random`` exactly as the reference does."""
from __future__ import annotations

import numpy as np
import scipy.linalg as la
from scipy.spatial.transform import Rotation

from oracle import np_oracle as O

WIND = 0.00025                 # EnvGeometric.py:34


def schedule(n, k=2):
    """(Tw, Tce, Texp) of fedCE_iteration n (:157-166)."""
    return (25 if n == 0 else 0), k * n * 2, min(n * k, 20 * k)


def draw_reference_noise(num_iter, D, c=O.CF2P, k=2):
    """sigma1 / sigma_explore (:242-268) with the global np.random, in the reference's order."""
    mg = c.M * c.G
    out = []
    for n in range(num_iter):
        tw, _, texp = schedule(n, k)
        uw = None
        if tw:
            uw = np.zeros((tw, D, 4))
            for t in range(tw):
                for j in range(D):
                    uw[t, j, 0] = np.random.uniform(.8 * mg, 1.5 * mg)
                    uw[t, j, 1:] = np.random.uniform(-0.00001, 0.00001, 3)
        ue = np.zeros((texp, D, 4))
        for t in range(texp):
            for j in range(D):
                ue[t, j, 0] = np.random.normal(mg, .15 * mg)
                ue[t, j, 1:] = np.random.normal(0, [0.005 * c.MAX_XY_TORQUE, 0.005 * c.MAX_XY_TORQUE, 0.005 * c.MAX_Z_TORQUE])
        out.append((uw, ue))
    return out


def fixture_case(d, D):
    """(poses, noise per iteration, num_iter) of case D of tests/golden/fedce_ref_in_loop.npz."""
    g = {k[len(f"d{D}_"):]: d[k] for k in d.files if k.startswith(f"d{D}_")}
    num_iter = int(g["num_iter"])
    noise, e0 = [], 0
    for n in range(num_iter):
        tw, _, texp = schedule(n)
        noise.append((g["u_warm"] if tw else None, g["u_explore"][e0:e0 + texp]))
        e0 += texp
    return g, noise, num_iter


def lin_model(c=O.CF2P):
    """LinearizedModel (A, B, Ahat, Bhat)."""
    A = np.zeros((12, 12))
    B = np.zeros((12, 4))
    A[0:3, 3:6] = np.eye(3)
    A[9:, 6:9] = np.eye(3)
    A[6, 1] = c.G
    A[7, 0] = -c.G
    B[8, 0] = 1.0 / c.M
    J = np.array([c.J[0], c.J[1], c.J[2]]) if np.ndim(c.J) == 1 else np.diag(c.J)
    B[3:6, 1:] = np.diag(1 / J)
    Bhat = B.copy()
    Bhat[3:6, 1:] = np.diag(1 / J) * 0.75
    Bhat[8, 0] = 1.0 / (c.M * .75)
    return A, B, A.copy(), Bhat


def error_state(x, x_des):
    """DecentralizedLQR.error_state (:288-298)."""
    e = np.copy(x)
    R_eq = Rotation.from_euler('xyz', [0, 0, x_des[2]]).as_matrix()
    R = Rotation.from_euler('xyz', x[:3]).as_matrix()
    e[:3] = Rotation.from_matrix(R_eq.T @ R).as_euler('xyz')
    e[9:] = R_eq.T @ (x[9:] - x_des[9:])
    e[6:9] = R_eq.T @ (x[6:9] - x_des[6:9])
    e[3:6] = R_eq.T @ (x[3:6] - x_des[3:6])
    return e


def lin_x(obs):
    return O.obs_to_lin_model(obs, 12)


class DLQR:
    """DecentralizedLQR (:12-345), the parts fedCE uses."""

    def __init__(self, D, c=O.CF2P):
        self.c, self.D = c, D
        A, B, Ahat, Bhat = lin_model(c)
        self.A_true, self.B_true = A, B
        rflat = [1 / (c.MAX_THRUST ** 2), 1 / (0.001 ** 2), 1 / (0.001 ** 2), 1 / (0.001 ** 2)]
        qflat = [1 / ((np.pi / 10) ** 2)] * 2 + [1 / ((np.pi / 20) ** 2)] + [1 / (.5 ** 2)] * 3 + [1 / (.15 ** 2)] * 3 + [1 / (.05 ** 2)] * 3
        self.ind_Q, self.ind_R = np.diag(qflat), np.diag(rflat)
        self.Q = np.kron(np.eye(D), self.ind_Q)
        self.R = np.kron(np.eye(D), self.ind_R)
        self.Q[np.index_exp[9:11, 21:23]] = -1 / (.1 ** 2)
        self.Q[np.index_exp[21:23, 9:11]] = -1 / (.1 ** 2)
        Astar = np.zeros((12 * D, 12 * D))
        Bstar = np.zeros((12 * D, 4 * D))
        for i in range(D):
            Astar[12 * i:12 * i + 12, 12 * i:12 * i + 12] = Ahat
            Bstar[12 * i:12 * i + 12, 4 * i:4 * i + 4] = Bhat
        self.theta = np.hstack([Astar, Bstar]).T
        self.P = np.repeat(20 * np.eye(16)[:, :, None], D, axis=2).transpose(2, 0, 1)
        for i in range(D):
            self.P[i][-3:, -3:] = 5_000_000 * np.eye(3)
        self.K = None
        self.pred_errors = [[] for _ in range(2 * D)]
        self.pred_thetas = [[] for _ in range(D)]
        self.des = np.zeros((D, 8))            # pos3, vel3, yaw, omega
        self.A_mask = np.zeros((12 * D, 12 * D))
        self.B_mask = np.zeros((12 * D, 4 * D))
        for i in range(D):
            a = self.A_mask[12 * i:12 * (i + 1), 12 * i:12 * (i + 1)]
            a[(6, 7), (1, 0)] = 1
            a[(0, 1, 2), (3, 4, 5)] = 1
            a[(9, 10, 11), (6, 7, 8)] = 1
            b = self.B_mask[12 * i:12 * (i + 1), 4 * i:4 * (i + 1)]
            b[3:6, 1:] = 1
            b[8, 0] = 1

    def get_thetai(self, i):
        D = self.D
        Ai = self.theta[i * 12:(i + 1) * 12, 12 * i:(i + 1) * 12].T
        Bi = self.theta[(12 * D + 4 * i):(12 * D + 4 * (i + 1)), 12 * i:(12 * (i + 1))].T
        return np.hstack([Ai, Bi]).T

    def overwrite_theta(self, theta_new, i):
        D = self.D
        self.theta[i * 12:(i + 1) * 12, 12 * i:(i + 1) * 12] = theta_new[:12, :]
        self.theta[(12 * D + 4 * i):(12 * D + 4 * (i + 1)), 12 * i:(12 * (i + 1))] = theta_new[12:, :]

    def project_theta(self):
        D = self.D
        Ahat = self.theta[:-(4 * D), :].T * self.A_mask
        Bhat = self.theta[-(4 * D):, :].T * self.B_mask
        for i in range(D):
            Ahat[12 * i:12 * (i + 1), 12 * i:12 * (i + 1)][(0, 1, 2), (3, 4, 5)] = 1
            Ahat[12 * i:12 * (i + 1), 12 * i:12 * (i + 1)][(9, 10, 11), (6, 7, 8)] = 1
        self.theta = np.hstack([Ahat, Bhat]).T

    def est_x_dot(self, x_tp1, phi, dt):
        x_dot = np.zeros((12,))
        x_dot[0:3] = x_tp1[3:6]
        x_dot[3:6] = (x_tp1[3:6] - phi[3:6]) / dt
        x_dot[6:9] = (x_tp1[6:9] - phi[6:9]) / dt
        x_dot[9:] = x_tp1[6:9]
        return x_dot

    def approx_theta_update(self, phis, xtp1s, dt):
        for i in range(self.D):
            phi = phis[i].reshape((16, 1))
            x_dot = self.est_x_dot(xtp1s[i], phis[i], dt)
            P = self.P[i]
            L = P @ phi @ np.linalg.inv(1 + phi.T @ P @ phi)
            th_i = self.get_thetai(i)
            theta_new = th_i + L @ (x_dot.T - phi.T @ th_i)
            self.overwrite_theta(theta_new, i)
            self.project_theta()
            self.P[i] = (np.eye(16) - L @ phi.T) @ P
            Ahat = self.get_thetai(i)[:12, :].T
            Bhat = self.get_thetai(i)[12:, :].T
            self.pred_thetas[i].append(np.hstack([Ahat, Bhat]))
            self.pred_errors[i].append(np.linalg.norm(x_dot.T - phi.T @ th_i))
            th_gt = np.hstack([self.A_true, self.B_true]).T
            self.pred_errors[i + self.D].append(np.linalg.norm(x_dot.T - phi.T @ th_gt))

    def compute_controller(self, force_diagonal=False):
        D = self.D
        if force_diagonal:
            self.K = np.zeros((4 * D, 12 * D))
            for i in range(D):
                A = self.theta[:12 * D, :].T[12 * i:12 * (i + 1), 12 * i:12 * (i + 1)]
                B = self.theta[12 * D:, :].T[12 * i:12 * (i + 1), 4 * i:4 * (i + 1)]
                P = la.solve_continuous_are(A, B, self.ind_Q, self.ind_R, e=None, s=None, balanced=True)
                self.K[4 * i:4 * (i + 1), 12 * i:12 * (i + 1)] = la.solve(self.ind_R, B.T @ P)
        else:
            A = self.theta[:12 * D, :].T
            B = self.theta[12 * D:, :].T
            P = la.solve_continuous_are(A, B, self.Q, self.R, e=None, s=None, balanced=True)
            self.K = la.solve(self.R, B.T @ P)

    def compute(self, obs):
        """-> (action [D,4], u [4D]) (:326-342)."""
        D, c = self.D, self.c
        es = [error_state(lin_x(obs[i]), np.hstack([[0, 0, self.des[i, 6]], [0, 0, self.des[i, 7]], self.des[i, 3:6], self.des[i, 0:3]]))
              for i in range(D)]
        us = np.array([-self.K[:, 12 * i:12 * (i + 1)] @ es[i] for i in range(D)])
        u = np.sum(us, axis=0)
        u_robot = np.array([u[4 * i:4 * (i + 1)] for i in range(D)])
        u_robot[:, 0] += c.M * c.G
        return np.array([O.input_to_action(ur, c) for ur in u_robot]), u


def features(theta, D):
    """The [D, 30] row of predictions.npy (fedCE :122-137)."""
    thetaA = theta[:12 * D, :].T
    thetaB = theta[12 * D:, :].T
    rows = []
    for i in range(D):
        A = thetaA[i * 12:(i + 1) * 12, i * 12:(i + 1) * 12]
        B = thetaB[i * 12:(i + 1) * 12, i * 4:(i + 1) * 4]
        rows.append(np.hstack([A[6, 1], A[7, 0], A[:3, 3:6].flatten(), A[9:, 6:9].flatten(), B[3:6, 1:].flatten(), B[8, 0]]))
    return np.array(rows)


class FedCE:
    """GeometricEnv.fedCE on the oracle.  ``trajectory(t) -> (pos, vel, acc, yaw, omega)`` replaces the Lemniscate of
    do_lemniscate=True; obs_log holds every observation env.step returned, in order."""

    def __init__(self, init_xyzs, init_rpys, target_pos, target_rpys, c=O.CF2P, freq=100, physics="dyn", wind=WIND):
        self.c = c
        self.D = len(init_xyzs)
        self.init_xyzs, self.init_rpys = np.asarray(init_xyzs, float), np.asarray(init_rpys, float)
        self.target_pos, self.target_rpys = np.asarray(target_pos, float), np.asarray(target_rpys, float)
        self.env = O.AviaryOracle(self.init_xyzs, self.init_rpys, c, pyb_freq=freq, ctrl_freq=freq, physics=physics)
        self.wind = np.array([wind, 0.0, 0.0])
        self.dlqr = DLQR(self.D, c)
        self.obs_log = []
        self.thetas, self.Ps, self.Ks = [], [], []

    def step(self, action, wind=True):
        self.env.wind = self.wind if wind else None
        obs = self.env.step(action)
        self.obs_log.append(obs)
        return obs

    def iteration(self, n, noise, k=2, do_lemniscate=False, trajectory=None):
        c, D, dl = self.c, self.D, self.dlqr
        dt = self.env.CTRL_TIMESTEP
        mg = c.M * c.G
        tw, tce, texp = schedule(n, k)
        uw, ue = noise
        obs = self.step(np.zeros((D, 4)), wind=False)        # :169-170, before any applyExternalForce
        for t in range(tw):
            phis, action = [], np.zeros((D, 4))
            for j in range(D):
                u = np.array(uw[t, j], dtype=float)
                act = O.input_to_action(u, c)
                u[0] = max(u[0], 0.0) - mg                     # input_to_action clips u[0] in place (model_conversions.py:88)
                x_des = np.zeros((12,))
                x_des[0:3] = self.init_rpys[j]
                x_des[-3:] = self.init_xyzs[j]
                action[j] = act
                phis.append(np.hstack([error_state(lin_x(obs[j]), x_des), u]))
            obs = self.step(action)
            e_tp1s = []
            for j in range(D):
                x_des = np.zeros((12,))
                x_des[0:3] = self.init_rpys[j]
                x_des[-3:] = self.init_xyzs[j]
                e_tp1s.append(error_state(lin_x(obs[j]), x_des))
            if D - 1 != 0:                                    # `i` is the wind loop's last drone index (:206, :232)
                dl.approx_theta_update(phis, e_tp1s, dt)
        last_desired = np.zeros((D, 12))
        dl.compute_controller()
        self.Ks.append(dl.K.copy())
        t = 0.0
        for _ in range(tce):
            for j in range(D):
                if do_lemniscate:
                    pos, vel, acc, yaw, omega = trajectory(t)
                    dl.des[j] = np.hstack([pos, vel, yaw, omega])
                else:
                    dl.des[j] = np.hstack([self.target_pos[j], np.zeros(3), self.target_rpys[j, 2], 0.0])
                    last_desired[j] = np.hstack([self.target_rpys[j], np.zeros(3), np.zeros(3), self.target_pos[j]])
            action, _ = dl.compute(obs)
            obs = self.step(action)
            t += dt
        for _ in range(texp):
            phis, action = [], np.zeros((D, 4))
            for j in range(D):
                e = error_state(lin_x(obs[j]), last_desired[j])
                act = O.input_to_action(np.array(ue[_, j], dtype=float), c)
                u = O.action_to_input(act, c)
                u[0] = u[0] - mg
                action[j] = act
                phis.append(np.hstack([e, u]))
            obs = self.step(action)
            e_tp1s = [error_state(lin_x(obs[j]), last_desired[j]) for j in range(D)]
            if D - 1 != 0:
                dl.approx_theta_update(phis, e_tp1s, dt)
        self.thetas.append(dl.theta.copy())
        self.Ps.append(dl.P.copy())
        return obs

    def run(self, num_iter, noise, **kw):
        for n in range(num_iter):
            self.iteration(n, noise[n], **kw)
        return self

    def control(self, K, trajs, steps, wind=True):
        """do_control(trajs, computed_K=K) with 'dlqr' (:404-481): one zero-action step, then steps of compute -> wind -> step."""
        dl = self.dlqr
        dl.K = K
        obs = self.step(np.zeros((self.D, 4)), wind=False)
        out, t = [], 0.0
        for _ in range(steps):
            for j in range(self.D):
                pos, vel, acc, yaw, omega = trajs[j](t)
                dl.des[j] = np.hstack([pos, vel, yaw, omega])
            action, _ = dl.compute(obs)
            obs = self.step(action, wind=wind)
            out.append(obs)
            t += self.env.CTRL_TIMESTEP
        return np.array(out)

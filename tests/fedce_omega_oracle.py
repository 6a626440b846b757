"""Float64 NumPy restatement of FedCE on the 9-state thrust / body-rate model (simulations/EnvGeometricOmega.py fedCE /
fedCE_iteration, the default loop) and of the DecentralizedLQROmega (control/dlqr/decentralized_lqr_omega.py) it runs, on
oracle.np_oracle.AviaryOracle's DYN physics in place of Bullet, with the real ``scipy.integrate.solve_ivp`` inside
forward_predict.

The noise is an input: ``noise[n] = (u_warm [25, D, 4] or None, u_explore [Texp, D, 4])`` per iteration, the raw draws of
``sigma1`` / ``sigma_explore`` in the order the reference makes them (step-major, then drone)."""
from __future__ import annotations

import numpy as np
import scipy.integrate
import scipy.linalg as la

from oracle import np_oracle as O
from tests.fedce_oracle import error_state as _error12

M, N, MN = 9, 4, 13


def schedule(n, k=2):
    """(Tw, Tce, Texp) of fedCE_iteration n (:129-133)."""
    return (25 if n == 0 else 0), n * k ** 3, n * k


def draw_reference_noise(num_iter, D, c=O.CF2P, k=2):
    """sigma1 / sigma_explore (:140-154) with the global np.random, in the reference's order."""
    mg = c.M * c.G
    out = []
    for n in range(num_iter):
        tw, _, texp = schedule(n, k)
        uw = None
        if tw:
            uw = np.zeros((tw, D, 4))
            for t in range(tw):
                for j in range(D):
                    uw[t, j, 0] = np.random.uniform(.7 * mg, 1.5 * mg)
                    uw[t, j, 1:] = np.random.uniform(-0.00001, 0.00001, 3)
        ue = np.zeros((texp, D, 4))
        for t in range(texp):
            for j in range(D):
                ue[t, j, 0] = np.random.normal(mg, .005 * mg)
                ue[t, j, 1:] = np.random.normal(0, [0.000000005, 0.000000005, 0.000000005])
        out.append((uw, ue))
    return out


def fixture_case(d, D):
    """(arrays, noise per iteration, num_iter) of case D of tests/golden/fedce_omega_ref_in_loop.npz."""
    g = {k[len(f"d{D}_"):]: d[k] for k in d.files if k.startswith(f"d{D}_")}
    num_iter = int(g["num_iter"])
    noise, e0 = [], 0
    for n in range(num_iter):
        tw, _, texp = schedule(n)
        noise.append((g["u_warm"] if tw else None, g["u_explore"][e0:e0 + texp]))
        e0 += texp
    return g, noise, num_iter


def error_state(x, x_des):
    """DecentralizedLQROmega.error_state (:174-183): the 12-state one without the rate block."""
    x12 = np.concatenate([x[:3], np.zeros(3), x[3:]])
    d12 = np.concatenate([x_des[:3], np.zeros(3), x_des[3:]])
    e = _error12(x12, d12)
    return np.concatenate([e[:3], e[6:]])


def lin_x(obs):
    return O.obs_to_lin_model(obs, 9)


def forward_predict(theta_i, e, u, dt, record=None):
    """:87-97 -> the end point; ``record`` (a list) receives (accepted steps, nfev, status)."""
    Ahat, Bhat = theta_i[:M].T, theta_i[M:].T
    sol = scipy.integrate.solve_ivp(lambda t, y: Ahat @ y + Bhat @ u, [0, dt], e)
    if record is not None:
        record.append((len(sol.t) - 1, sol.nfev, sol.status))
    return sol.y[:, -1]


def rls2_update(theta_i, V, phi, x_tp1, dt, record=None):
    """theta_update2 (:110-123) for one drone -> (theta_new, V_new)."""
    phi = phi.reshape(MN, 1)
    x1 = x_tp1.reshape(M, 1)
    pred = forward_predict(theta_i, x1.flatten(), phi[-N:].flatten(), dt, record)
    return theta_i + np.linalg.inv(V) @ phi @ (x1.T - pred), V + phi @ phi.T


class DLQROmega:
    """DecentralizedLQROmega (:13-252), the parts fedCE uses; theta per drone [D, 13, 9], P = V [D, 13, 13]."""

    def __init__(self, D, c=O.CF2P, dt=0.01):
        self.c, self.D, self.dt = c, D, dt
        rflat = [1 / (c.MAX_THRUST ** 2), 1 / (0.1 ** 2), 1 / (0.1 ** 2), 1 / (0.1 ** 2)]
        qflat = [1 / ((np.pi / 20) ** 2)] * 2 + [1 / ((np.pi / 40) ** 2)] + [1 / (.15 ** 2)] * 3 + [1 / (.05 ** 2)] * 3
        self.ind_Q, self.ind_R = np.diag(qflat), np.diag(rflat)
        self.Q = np.kron(np.eye(D), self.ind_Q)
        self.R = np.kron(np.eye(D), self.ind_R)
        self.th = None
        self.P = np.repeat(np.eye(MN)[None], D, axis=0)
        self.K = None
        self.des = np.zeros((D, 7))                              # pos3, vel3, yaw
        self.low = O.ThrustOmegaOracle(D, c)
        self.ivp = []

    def set_model(self, Ahat, Bhat):
        self.th = np.repeat(np.hstack([Ahat, Bhat]).T[None], self.D, axis=0).copy()
        return self

    @property
    def theta(self):
        """the reference's block layout [13D, 9D]"""
        D = self.D
        out = np.zeros((MN * D, M * D))
        for i in range(D):
            out[i * M:(i + 1) * M, M * i:M * (i + 1)] = self.th[i, :M]
            out[M * D + N * i:M * D + N * (i + 1), M * i:M * (i + 1)] = self.th[i, M:]
        return out

    def theta_update2(self, phis, xtp1s):
        for i in range(self.D):
            self.th[i], self.P[i] = rls2_update(self.th[i], self.P[i], np.asarray(phis[i]), np.asarray(xtp1s[i]), self.dt, self.ivp)

    def compute_controller(self):
        D = self.D
        th = self.theta
        A, B = th[:M * D].T, th[M * D:].T
        P = la.solve_continuous_are(A, B, self.Q, self.R, e=None, s=None, balanced=True)
        self.K = la.solve(self.R, B.T @ P)

    def compute_low_level(self, u, obs):
        """every drone at once: u [D,4] (clipped at 0 in place like computeControlFromInput :93), obs [D,20]"""
        u[:, 0] = np.clip(u[:, 0], 0, None)
        return self.low.compute_low_level(u, obs, self.dt)

    def cap_u(self, u):
        u[:, 0] = np.clip(u[:, 0], 4 * (9440.3 ** 2 * self.c.KF), self.c.MAX_THRUST)
        return u

    def compute(self, obs, skip_low_level=False):
        """-> (action [D,4] or None, capped u [D,4]) (:212-231)."""
        D, c = self.D, self.c
        es = [error_state(lin_x(obs[i]), np.hstack([[0, 0, self.des[i, 6]], self.des[i, 3:6], self.des[i, 0:3]])) for i in range(D)]
        us = np.array([-self.K[:, M * i:M * (i + 1)] @ es[i] for i in range(D)])
        u = np.sum(us, axis=0)
        u_robot = np.array([u[N * i:N * (i + 1)] for i in range(D)])
        u_robot[:, 0] += c.M * c.G
        if skip_low_level:
            return None, self.cap_u(u_robot)
        action = self.compute_low_level(u_robot, obs)
        return action, self.cap_u(u_robot)


def lin_model(c=O.CF2P):
    """(Ahat, Bhat) of LinearizedOmegaModel (model/linear_omega.py:56-61: gravity coupling * 1.2, mass * 0.8)."""
    A, B = O.linear_omega_AB(c)
    A[3, 1], A[4, 0] = c.G * 1.2, -c.G * 1.2
    B[5, 0] = 1.0 / (c.M * 0.8)
    return A, B


class FedCEOmega:
    """GeometricEnv.fedCE (EnvGeometricOmega.py) on the oracle; obs_log holds every observation env.step returned, in order."""

    def __init__(self, init_xyzs, init_rpys, target_pos, target_rpys, c=O.CF2P, freq=100):
        self.c = c
        self.D = len(init_xyzs)
        self.init_xyzs, self.init_rpys = np.asarray(init_xyzs, float), np.asarray(init_rpys, float)
        self.target_pos, self.target_rpys = np.asarray(target_pos, float), np.asarray(target_rpys, float)
        self.env = O.AviaryOracle(self.init_xyzs, self.init_rpys, c, pyb_freq=freq, ctrl_freq=freq)
        self.dlqr = DLQROmega(self.D, c, self.env.CTRL_TIMESTEP).set_model(*lin_model(c))
        self.obs_log, self.thetas, self.Ps, self.Ks, self.updates = [], [], [], [], []

    def step(self, action):
        obs = self.env.step(action)
        self.obs_log.append(obs)
        return obs

    def _phase(self, obs, u_raw, x_des):
        D, dl, mg = self.D, self.dlqr, self.c.M * self.c.G
        for t in range(len(u_raw)):
            u = np.array(u_raw[t], dtype=float)
            e = [error_state(lin_x(obs[j]), x_des[j]) for j in range(D)]
            action = dl.compute_low_level(u, obs)
            u[:, 0] -= mg
            phis = [np.hstack([e[j], u[j]]) for j in range(D)]
            obs = self.step(action)
            e1 = [error_state(lin_x(obs[j]), x_des[j]) for j in range(D)]
            if t != 0:
                dl.theta_update2(phis, e1)
                self.updates.append(dl.th.copy())
        return obs

    def iteration(self, n, noise, k=2):
        D, dl = self.D, self.dlqr
        tw, tce, texp = schedule(n, k)
        uw, ue = noise
        obs = self.step(np.zeros((D, 4)))
        if tw:
            x_des = np.hstack([self.init_rpys, np.zeros((D, 3)), self.init_xyzs])
            obs = self._phase(obs, uw, x_des)
        last_desired = np.zeros((D, 9))
        dl.compute_controller()
        self.Ks.append(dl.K.copy())
        for _ in range(tce):
            for j in range(D):
                dl.des[j] = np.hstack([self.target_pos[j], np.zeros(3), self.target_rpys[j, 2]])
                last_desired[j] = np.hstack([self.target_rpys[j], np.zeros(3), self.target_pos[j]])
            action, _ = dl.compute(obs)
            obs = self.step(action)
        obs = self._phase(obs, ue, last_desired)
        self.thetas.append(dl.theta.copy())
        self.Ps.append(dl.P.copy())
        return obs

    def run(self, num_iter, noise):
        for n in range(num_iter):
            self.iteration(n, noise[n])
        return self

    def control(self, K, trajs, steps):
        """do_control(trajs, computed_K=K) with 'dlqr' (:265-335) on a fresh DecentralizedLQROmega: one zero-action step, then compute -> step."""
        dl = self.dlqr
        dl.K = K
        obs = self.step(np.zeros((self.D, 4)))
        out, t = [], 0.0
        for _ in range(steps):
            for j in range(self.D):
                pos, vel, acc, yaw, omega = trajs[j](t)
                dl.des[j] = np.hstack([pos, vel, yaw])
            action, _ = dl.compute(obs)
            obs = self.step(action)
            out.append(obs)
            t += self.env.CTRL_TIMESTEP
        return np.array(out)

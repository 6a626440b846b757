"""Float64 NumPy restatement of FedCE as simulations/CBFTest.py runs it (fedCE_iteration :131-267): tests/fedce_omega_oracle.py with
``theta_update`` (control/dlqr/decentralized_lqr_omega.py:125-139), the covariance form of the recursive least squares, where
EnvGeometricOmega.py calls ``theta_update2``.  P is then the covariance: it starts at I like the information matrix does."""
from __future__ import annotations

import numpy as np

from oracle import np_oracle as O
from tests import fedce_omega_oracle as F

M, N, MN = F.M, F.N, F.MN


def rls_cov_update(theta_i, P, phi, x_tp1, dt, record=None):
    """theta_update (:125-139) for one drone -> (theta_new, P_new); P is not symmetrised."""
    phi = phi.reshape(MN, 1)
    x1 = x_tp1.reshape(M, 1)
    L = P @ phi @ np.linalg.inv(1 + phi.T @ P @ phi)
    pred = F.forward_predict(theta_i, x1.flatten(), phi[-N:].flatten(), dt, record)
    return theta_i + L @ (x1.T - pred), (np.eye(MN) - L @ phi.T) @ P


class DLQROmegaCov(F.DLQROmega):
    """DLQROmega whose learner is theta_update; ``V`` follows as the information matrix (V += phi phi^T), the pair the device carries."""

    def __init__(self, D, c=O.CF2P, dt=0.01):
        super().__init__(D, c, dt)
        self.V = self.P.copy()

    def theta_update(self, phis, xtp1s):
        for i in range(self.D):
            phi = np.asarray(phis[i], dtype=float)
            self.th[i], self.P[i] = rls_cov_update(self.th[i], self.P[i], phi, np.asarray(xtp1s[i]), self.dt, self.ivp)
            self.V[i] = self.V[i] + np.outer(phi, phi)

    def theta_update_info(self, phis, xtp1s):
        """a theta_update2 step on the same object: theta from np.linalg.inv(V) as the reference, P kept its inverse"""
        for i in range(self.D):
            self.th[i], self.V[i] = F.rls2_update(self.th[i], self.V[i], np.asarray(phis[i]), np.asarray(xtp1s[i]), self.dt, self.ivp)
            self.P[i] = np.linalg.inv(self.V[i])

    theta_update2 = theta_update          # the name FedCEOmega._phase calls


class FedCEOmegaCov(F.FedCEOmega):
    """GeometricEnv.fedCE of simulations/CBFTest.py on the oracle."""

    def __init__(self, init_xyzs, init_rpys, target_pos, target_rpys, c=O.CF2P, freq=100):
        super().__init__(init_xyzs, init_rpys, target_pos, target_rpys, c, freq)
        self.dlqr = DLQROmegaCov(self.D, c, self.env.CTRL_TIMESTEP).set_model(*F.lin_model(c))


def fixture_case(d, D):
    """fedce_omega_oracle.fixture_case on tests/golden/fedce_omega_cov_ref_in_loop.npz (the same key layout)."""
    return F.fixture_case(d, D)


def unit_chain(phis, xtp1, dt=0.01, c=O.CF2P):
    """the cov_unit block: theta_update on caller-made (phi, x_tp1) [n, D, 13] / [n, D, 9] -> (theta [n,D,13,9], P [n,D,13,13], dl)"""
    n, D = phis.shape[:2]
    dl = DLQROmegaCov(D, c, dt).set_model(*F.lin_model(c))
    th, P = [], []
    for t in range(n):
        dl.theta_update(list(phis[t]), list(xtp1[t]))
        th.append(dl.th.copy())
        P.append(dl.P.copy())
    return np.array(th), np.array(P), dl

#!/usr/bin/env python3
"""Mint tests/golden/fedce_omega_cov_ref_in_loop.npz: FedCE on the 9-state thrust / body-rate model as simulations/CBFTest.py runs it
(fedCE_iteration :131-267), i.e. with ``theta_update`` (control/dlqr/decentralized_lqr_omega.py:125-139), the covariance form of the
recursive least squares, in the place of EnvGeometricOmega.py's ``theta_update2``.

Run ONLY in the build container, where the reference lives (see mint_golden.py):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/mint_fedce_omega_cov.py

Everything is mint_fedce_omega.py's -- its loader, env, drivers (run / rls2_unit / long_phase) and seeds -- handed a subclass of the
reference's DecentralizedLQROmega whose ``theta_update2`` IS the reference's ``theta_update`` (the drivers call the method by that
name), and with CBFTest.circle_initialize's poses (:383-391: cos for x, sin for y).  Blocks: d2_* (five iterations), d3_* (three),
cov_unit_* (64 calls on caller-made phi ~ N(0, 0.3): phi^T P phi is O(1) there, the two forms are O(1) apart), long_* (one phase of
99 updates, where phi^T P phi << 1 and the forms differ by ~1e-6 only).  Next to each block, ``*_info_thetas``: what the unmodified
reference class (theta_update2) gives on the same inputs (d*: theta after every iteration; cov_unit: after every call; long: after
the last update), so that a test can assert that its gate separates the forms."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import mint_golden as MG  # noqa: E402
import mint_fedce_omega as MO  # noqa: E402
from mint_fedce_omega import load_dlqr_omega, make_env, circle  # noqa: E402,F401


def circle_cbftest(D, init_rad=0.2):
    """GeometricEnv.circle_initialize of simulations/CBFTest.py (:383-404)."""
    xyz = np.zeros((D, 3))
    for i in range(1, D):
        xyz[i, 0] = init_rad * np.cos((i / D) * 2 * np.pi)
        xyz[i, 1] = init_rad * np.sin((i / D) * 2 * np.pi)
    tpos = xyz.copy()
    tpos[:, 2] += 1
    trpy = np.zeros((D, 3))
    trpy[:, 2] = np.pi / 2
    return xyz, np.zeros((D, 3)), tpos, trpy


if __name__ == "__main__":
    DLQR, Lin, mc = load_dlqr_omega()

    class Cov(DLQR):
        theta_update2 = DLQR.theta_update

    MO.circle = circle_cbftest
    out = {}
    for D, num_iter, seed in ((2, 5, 11), (3, 3, 12)):
        r = MO.run(D, num_iter, seed, Cov, Lin, mc)
        info = MO.run(D, num_iter, seed, DLQR, Lin, mc)
        np.testing.assert_array_equal(r["u_warm"], info["u_warm"])
        out.update({f"d{D}_{k}": v for k, v in r.items()})
        out[f"d{D}_info_thetas"] = info["thetas"]
        print(f"D = {D}: {num_iter} iterations, {len(r['obs_log'])} steps, {len(r['theta_updates'])} updates, solve_ivp steps "
              f"{np.unique(r['ivp_steps'])}, |theta| max {np.abs(r['thetas']).max():.3g}, cond(P) {np.linalg.cond(r['Ps'][-1][0]):.3g}, "
              f"forms apart by {np.abs(r['theta_updates'] - info['theta_updates']).max() / np.abs(r['theta_updates']).max():.2e}")
    r = MO.rls2_unit(Cov, Lin)
    info = MO.rls2_unit(DLQR, Lin)
    np.testing.assert_array_equal(r["phis"], info["phis"])
    out.update({f"cov_unit_{k}": v for k, v in r.items()})
    out["cov_unit_info_thetas"] = info["thetas"]
    print(f"cov_unit: solve_ivp steps {np.unique(r['ivp_steps'])}, |theta| max {np.abs(r['thetas']).max():.3g}, forms apart by "
          f"{np.abs(r['thetas'] - info['thetas']).max() / np.abs(r['thetas']).max():.2e}")
    r = MO.long_phase(Cov, Lin, mc)
    info = MO.long_phase(DLQR, Lin, mc)
    out.update({f"long_{k}": v for k, v in r.items()})
    out["long_info_thetas"] = info["theta_updates"][-1:]       # after the last update only: the file stays under 1 MiB
    print(f"long: {len(r['theta_updates'])} updates, |theta| max {np.abs(r['theta_updates']).max():.3g}, cond(P) {np.linalg.cond(r['P'][0]):.3g}, "
          f"asymmetry of P {np.abs(r['P'] - r['P'].swapaxes(-1, -2)).max():.1e}, P_cov V_info - I "
          f"{np.abs(r['P'] @ info['P'] - np.eye(13)).max():.1e}, forms apart by "
          f"{np.abs(r['theta_updates'] - info['theta_updates']).max() / np.abs(r['theta_updates']).max():.2e}")
    path = os.path.join(HERE, "fedce_omega_cov_ref_in_loop.npz")
    np.savez_compressed(path, ctrl_timestep=0.01, rtol=1e-3, atol=1e-6, base_class="stubbed", update="theta_update",
                        physics="oracle DYN step (np_oracle.AviaryOracle, 100 / 100 Hz, no wind); DecentralizedLQROmega (theta_update), "
                                "LinearizedOmegaModel, ThrustOmegaController and model conversions: reference objects; *_info_*: the same "
                                "drivers with the reference's theta_update2",
                        **out, **MG.META)
    print(os.path.getsize(path), "bytes")

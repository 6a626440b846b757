#!/usr/bin/env python3
"""HIP-event timing of mds_fedce_omega_identify (T = 50, every step updating) and mds_rollout_dlqr_omega_fused (T = 200) at
E = 4 096, D = 2, beside the wall time of the NumPy restatement (tests/fedce_omega_oracle.py) of the same phase for ONE env on the
same box.  Prints one line per figure; nothing is gated."""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from multidronesim_amd.control import DecentralizedLQROmega  # noqa: E402
from multidronesim_amd.control.dlqr.decentralized_lqr_omega import UPDATE_ALL  # noqa: E402
from multidronesim_amd.simulations import EnvGeometricOmega as S  # noqa: E402
from tests import fedce_omega_oracle as F  # noqa: E402

E, D = 4096, 2


def timed(fn, reps=3):
    best = None
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms = a.elapsed_time(b)
        best = ms if best is None else min(best, ms)
    return best


for dtype in ("float32", "float64"):
    geo = S.GeometricEnv(S.parse_args(["--num_drones", str(D), "--num_envs", str(E), "--dtype", dtype]), circle_init=True)
    env = geo.create_env()
    dl = DecentralizedLQROmega(env, geo.linear_models)
    g = torch.Generator(device=env.device).manual_seed(0)
    u = dl.draw_inputs("warmup", 50, g)
    x_des = np.hstack([geo.INIT_RPYS, np.zeros((D, 3)), geo.INIT_XYZS])
    env.step(torch.zeros((E, D, 4), dtype=env.dtype, device=env.device))
    ms = timed(lambda: dl.identify(u, x_des, UPDATE_ALL))
    print(f"{dtype}: mds_fedce_omega_identify T=50 E={E} D={D}: {ms:.3f} ms ({ms * 1e3 / 50:.1f} us per step), status max {int(dl.status.max())}")
    dl.compute_controller()
    env.set_trajectories([S.WaitTrajectory(position=geo.TARGET_POSITIONS[j], duration=10.0, yaw=geo.TARGET_RPYS[j, 2]) for j in range(D)])
    ms = timed(lambda: dl.rollout(0.0, 200, log=False))
    print(f"{dtype}: mds_rollout_dlqr_omega_fused T=200 E={E} D={D}: {ms:.3f} ms ({ms * 1e3 / 200:.1f} us per step)")

np.random.seed(0)
noise = F.draw_reference_noise(1, D)
ora = F.FedCEOmega(geo.INIT_XYZS, geo.INIT_RPYS, geo.TARGET_POSITIONS, geo.TARGET_RPYS)
obs = ora.step(np.zeros((D, 4)))
t0 = time.perf_counter()
ora._phase(obs, np.concatenate([noise[0][0], noise[0][0]]), np.hstack([geo.INIT_RPYS, np.zeros((D, 3)), geo.INIT_XYZS]))
t1 = time.perf_counter()
print(f"NumPy restatement, ONE env, identify T=50: {(t1 - t0) * 1e3:.1f} ms")
ora.dlqr.compute_controller()
t0 = time.perf_counter()
ora.control(ora.dlqr.K, [lambda t, j=j: (geo.TARGET_POSITIONS[j], np.zeros(3), np.zeros(3), geo.TARGET_RPYS[j, 2], 0.0) for j in range(D)], 200)
t1 = time.perf_counter()
print(f"NumPy restatement, ONE env, dLQR rollout T=200: {(t1 - t0) * 1e3:.1f} ms")

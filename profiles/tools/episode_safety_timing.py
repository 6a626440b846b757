"""mds_rollout_episodes with the collision causes on (mds_set_episode_safety) against the same call with them off, in one process: 262 144
envs x 2 drones and 32 768 x 16, DYN, 240 Hz, an action table of 8 sets around hover, every step's observation, reward and flags into rings
of 16 slots, fp32 and fp16 storage, 8 and 50 control steps per launch.

Both handles run the rule of episodes_timing.py (max_steps = 1000, every termination test on at thresholds an RL rollout would use); the
safety handle adds safety_radius = 0.1, zscale = 2 (drones of an env are 0.3 m apart: the pair tests run and rarely fire) and `--obstacles`
spheres (default 4) away from the drones.  The two are timed alternately, `--reps` times each, with device events around whole calls of
`--steps` control steps; medians and spread go to one JSON line per case (and to --out).

    python profiles/tools/episode_safety_timing.py --out profiles/episode_safety.json
    python profiles/tools/episode_safety_timing.py --asm TREE.s --out profiles/episode_safety.json      # no GPU: adds the kernels' resources

--asm reads `hipcc -S --cuda-device-only` output (profiles/tools/asm_equiv.py's parser) and records VGPRs, LDS bytes, scratch and waves per
SIMD of every k_rollout_episodes / k_rollout_episodes_safe instantiation under "kernels" of the --out file, keeping its timing rows."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

EPISODE = 1000
RULE = dict(max_steps=EPISODE, z_min=0.2, z_max=3.0, max_dist=2.0, max_tilt=1.0, max_speed=5.0, max_rate=20.0, term_penalty=1.0)
SHAPES = ((262144, 2), (32768, 16))


def kernel_resources(asm_path):
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import asm_equiv
    fns = asm_equiv.functions(asm_path)
    names = [n for n in fns if "k_rollout_episodes" in n]
    shown = asm_equiv.demangled(names)
    out = {}
    for n in names:
        key = shown[n].split("(")[0].replace("void mds::", "") if shown[n] != n else n
        out[key] = {"vgpr": fns[n].get("vgpr"), "agpr": fns[n].get("agpr"), "scratch_bytes": fns[n].get("scratch"), "lds_bytes": fns[n].get("lds"),
                    "waves_per_simd": fns[n].get("occupancy")}
    return out


def timed(torch, fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / steps            # us per control step


def measure(args):
    import numpy as np
    import torch
    from multidronesim_amd.envs.CtrlAviary import CtrlAviary, DroneModel, Physics
    rows = []
    for E, D in SHAPES:
        # every env flies the same place (envs never interact): small coordinates keep the fp16-stored positions 0.3 m apart
        xyz = np.zeros((E, D, 3))
        xyz[..., 0] = 0.3 * np.arange(D)[None, :]
        xyz[..., 2] = 1.0
        obstacles = np.array([[1.0 * k, 0.5, 1.0, 0.1] for k in range(args.obstacles)]).reshape(-1, 4)
        for dtype in ("float16", "float32"):
            envs = {}
            for kind in ("off", "on"):
                env = CtrlAviary(drone_model=DroneModel.CF2P, num_drones=D, initial_xyzs=xyz, initial_rpys=np.zeros((E, D, 3)), physics=Physics.DYN,
                                 pyb_freq=240, ctrl_freq=240, num_envs=E, dtype=dtype)
                env.set_episodes(**RULE)
                if kind == "on":
                    env.set_episode_safety(0.1, 2.0, obstacles)
                envs[kind] = env
            g = torch.Generator(device="cuda").manual_seed(1234)
            ref = envs["off"]
            act = torch.stack([(ref.HOVER_RPM * (1 + 0.05 * torch.randn((E, D, 4), device="cuda", generator=g))).clamp(0, ref.MAX_RPM).to(ref.dtype)
                               for _ in range(8)]).contiguous()
            log = torch.empty((args.slots, E, D, 20), dtype=ref.dtype, device="cuda")
            rlog = torch.empty((args.slots, E), dtype=torch.float32, device="cuda")
            flog = torch.empty((args.slots, E), dtype=torch.int32, device="cuda")
            for spl in (8, 50):
                calls = {k: (lambda k=k: envs[k].rollout_episodes(act, 0, args.steps, log, rlog, flog, steps_per_launch=spl)) for k in envs}
                us = {k: [] for k in calls}
                for k in calls:                               # warm-up: code objects, the ring's pages
                    envs[k]._housekeeping()
                    timed(torch, calls[k], args.steps)
                ended = {}
                for _ in range(args.reps):                    # alternating
                    for k in calls:
                        envs[k]._housekeeping()
                        count = envs[k].episode_counters()["count"]
                        before = int(count.sum().item())
                        us[k].append(timed(torch, calls[k], args.steps))
                        ended[k] = int(count.sum().item()) - before
                row = {"dtype": dtype, "envs": E, "drones": D, "steps_per_launch": spl, "steps": args.steps, "reps": args.reps,
                       "obstacles": int(args.obstacles), "episodes_ended_in_last_call": ended}
                for k in calls:
                    row[f"{k}_us_per_step"] = statistics.median(us[k])
                    row[f"{k}_us_min_max"] = [min(us[k]), max(us[k])]
                    row[f"{k}_drone_steps_per_s"] = E * D / (statistics.median(us[k]) * 1e-6)
                row["on_over_off"] = row["on_us_per_step"] / row["off_us_per_step"]
                rows.append(row)
                print(json.dumps(row), flush=True)
            for env in envs.values():
                env.close()
            del envs, act, log, rlog, flog
            torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--slots", type=int, default=16)
    ap.add_argument("--obstacles", type=int, default=4)
    ap.add_argument("--asm", default=None, help="device assembly of csrc/mds_api.hip (part 1): record the kernels' resources instead of timing")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    doc = {}
    if args.out and os.path.exists(args.out):
        with open(args.out) as f:
            doc = json.load(f)
    if args.asm:
        doc["kernels"] = kernel_resources(args.asm)
    else:
        doc["timing"] = measure(args)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()

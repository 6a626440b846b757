"""What drawing the actions in the rollout kernel costs.  E x D drones (default 65 536 x 8 and 37 x 7), float32, DYN_DRAG at 240 Hz, a
12 -> 64 -> 64 -> 4 tanh policy of small random weights, a rule that keeps the episodes running; in one process, by HIP events around
whole calls of `--steps` control steps, best and median of `--reps` after an untimed call of the same length, the kinds alternating:

  policy          rollout_episodes_policy, no ring                           (the deterministic rollout)
  sampled_bare    rollout_episodes_sampled, no ring                          (the draw alone)
  sampled         rollout_episodes_sampled with the sample and logp rings    (what a learner needs beside the rows)
  sampled_acted   ... and the acted_obs ring                                 (the rows the actions were drawn on)

`--root` names the tree whose multidronesim_amd is imported (default: this one); a tree without the sampled entry points measures
`policy` alone, which is how the parent commit's library is timed on the same device.

    python profiles/tools/episode_sample_timing.py --out profiles/out/episode_sample_timing.json
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
RULE = dict(max_steps=200, z_min=0.2, z_max=3.0, max_dist=2.0, max_tilt=1.0, max_speed=5.0, max_rate=20.0, term_penalty=1.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", type=int, nargs="+", default=[65536, 8, 37, 7], help="E D pairs")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--steps-per-launch", type=int, default=50)
    ap.add_argument("--slots", type=int, default=50, help="slots of every ring")
    ap.add_argument("--log-std", type=float, default=-2.0)
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--tag", default="")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    sys.path.insert(0, os.path.abspath(args.root))
    from multidronesim_amd.envs.CtrlAviary import CtrlAviary, DroneModel, Physics
    nn = torch.nn
    sampled = hasattr(CtrlAviary, "rollout_episodes_sampled")
    kinds = ("policy", "sampled_bare", "sampled", "sampled_acted") if sampled else ("policy",)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1e3 / args.steps                # us per control step

    rows = []
    for E, D in zip(args.shapes[0::2], args.shapes[1::2]):
        xyz = np.zeros((E, D, 3))
        xyz[..., 0] = (np.arange(E) % 512)[:, None] + 0.3 * np.arange(D)[None, :]
        xyz[..., 1] = (np.arange(E) // 512)[:, None]
        xyz[..., 2] = 1.0
        torch.manual_seed(0)
        net = nn.Sequential(nn.Linear(12, 64), nn.Tanh(), nn.Linear(64, 64), nn.Tanh(), nn.Linear(64, 4))
        with torch.no_grad():
            net[4].weight.mul_(0.1)                            # small actions: the episodes keep running
        fns = {}
        envs = []
        for kind in kinds:
            env = CtrlAviary(drone_model=DroneModel.CF2P, num_drones=D, initial_xyzs=xyz, initial_rpys=np.zeros((E, D, 3)), physics=Physics.PYB_DRAG,
                             pyb_freq=240, ctrl_freq=240, num_envs=E, dtype="float32")
            env.set_episodes(**RULE)
            env.set_episode_policy_from_torch(net)
            envs.append(env)
            if kind == "policy":
                fns[kind] = lambda env=env: env.rollout_episodes_policy(0, args.steps, steps_per_launch=args.steps_per_launch)
                continue
            env.set_episode_policy_noise(args.log_std, seed=1)
            z = lambda *shape: torch.zeros((args.slots, E, D) + shape, dtype=torch.float32, device="cuda")   # noqa: E731
            logs = {}
            if kind != "sampled_bare":
                logs.update(sample_log=z(4), logp_log=z())
            if kind == "sampled_acted":
                logs.update(acted_obs_log=z(20))
            fns[kind] = lambda env=env, logs=logs: env.rollout_episodes_sampled(0, args.steps, steps_per_launch=args.steps_per_launch, **logs)
        times = {kind: [] for kind in kinds}
        for fn in fns.values():                                    # untimed: code objects, allocator, the first touch of every buffer
            fn()
        torch.cuda.synchronize()
        for _ in range(args.reps):                                 # alternating: a drift of the device hits every kind alike
            for kind, fn in fns.items():
                times[kind].append(timed(fn))
        row = {"tag": args.tag, "envs": E, "drones": D, "dtype": "float32", "steps": args.steps, "reps": args.reps, "slots": args.slots,
               "steps_per_launch": args.steps_per_launch, "device": torch.cuda.get_device_name(0)}
        for kind, t in times.items():
            row[f"{kind}_us_per_step_best"], row[f"{kind}_us_per_step_median"] = min(t), sorted(t)[len(t) // 2]
        for kind in kinds[1:]:
            row[f"{kind}_over_policy"] = row[f"{kind}_us_per_step_best"] / row["policy_us_per_step_best"]
        rows.append(row)
        print(json.dumps(row), flush=True)
        for env in envs:
            env.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()

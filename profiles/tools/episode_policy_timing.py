"""What the in-kernel MLP policy buys over a policy in the loop.  E x 8 drones (default E = 8 192 and 65 536), float32, DYN_DRAG at 240 Hz,
a 12 -> 64 -> 64 -> 4 tanh policy of small random weights, a rule that keeps the episodes running; in one process, by HIP events around
whole calls, best of `--reps` after a warm-up call:

  fused    rollout_episodes_policy, 50 control steps per launch              (the policy inside the rollout kernel)
  loop     per control step: the same nn.Sequential in torch on the device, its output scaled to RPM, then step_episodes
           (what the library offered before: one launch per step plus the framework's launches for the policy)
  table    rollout_episodes with a replayed action table, 50 steps per launch  (for scale: the step without a policy)

    python profiles/tools/episode_policy_timing.py --out profiles/out/episode_policy_timing.json
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
RULE = dict(max_steps=200, z_min=0.2, z_max=3.0, max_dist=2.0, max_tilt=1.0, max_speed=5.0, max_rate=20.0, term_penalty=1.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, nargs="+", default=[8192, 65536])
    ap.add_argument("--drones", type=int, default=8)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--steps-per-launch", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    from multidronesim_amd.envs.CtrlAviary import CtrlAviary, DroneModel, Physics
    nn = torch.nn

    def best(fn):
        fn()                                                   # warm-up: code objects, allocator, the first touch of every buffer
        torch.cuda.synchronize()
        times = []
        for _ in range(args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            times.append(a.elapsed_time(b) * 1e3 / args.steps)            # us per control step
        return min(times), sorted(times)[len(times) // 2]

    rows = []
    D = args.drones
    for E in args.envs:
        xyz = np.zeros((E, D, 3))
        xyz[..., 0] = (np.arange(E) % 512)[:, None] + 0.3 * np.arange(D)[None, :]
        xyz[..., 1] = (np.arange(E) // 512)[:, None]
        xyz[..., 2] = 1.0
        torch.manual_seed(0)
        net = nn.Sequential(nn.Linear(12, 64), nn.Tanh(), nn.Linear(64, 64), nn.Tanh(), nn.Linear(64, 4))
        with torch.no_grad():
            net[4].weight.mul_(0.1)                            # small actions: the episodes keep running
        envs = {}
        for kind in ("fused", "loop", "table"):
            env = CtrlAviary(drone_model=DroneModel.CF2P, num_drones=D, initial_xyzs=xyz, initial_rpys=np.zeros((E, D, 3)), physics=Physics.PYB_DRAG,
                             pyb_freq=240, ctrl_freq=240, num_envs=E, dtype="float32")
            env.set_episodes(**RULE)
            envs[kind] = env
        envs["fused"].set_episode_policy_from_torch(net)
        dev_net = net.to("cuda")
        ref = envs["loop"]
        target = torch.as_tensor(xyz, device="cuda", dtype=torch.float32)
        hover, scale = float(ref.HOVER_RPM), 0.05 * float(ref.HOVER_RPM)
        g = torch.Generator(device="cuda").manual_seed(1234)
        table = torch.stack([(ref.HOVER_RPM * (1 + 0.01 * torch.randn((E, D, 4), device="cuda", generator=g))).to(ref.dtype) for _ in range(8)]).contiguous()

        def fused():
            envs["fused"].rollout_episodes_policy(0, args.steps, steps_per_launch=args.steps_per_launch)

        def loop():
            env = envs["loop"]
            obs = env._obs
            with torch.no_grad():
                for _ in range(args.steps):
                    x = torch.cat([obs[..., 0:3] - target, obs[..., 7:16]], dim=-1)
                    act = hover + scale * dev_net(x).clamp(-1.0, 1.0)
                    obs = env.step_episodes(act.contiguous())[0]

        def replay():
            envs["table"].rollout_episodes(table, 0, args.steps, steps_per_launch=args.steps_per_launch)

        row = {"envs": E, "drones": D, "dtype": "float32", "steps": args.steps, "reps": args.reps, "steps_per_launch": args.steps_per_launch,
               "device": torch.cuda.get_device_name(0)}
        for name, fn in (("fused", fused), ("loop", loop), ("table", replay)):
            envs[name]._computeObs()
            row[f"{name}_us_per_step_best"], row[f"{name}_us_per_step_median"] = best(fn)
        row["loop_over_fused"] = row["loop_us_per_step_best"] / row["fused_us_per_step_best"]
        row["fused_ns_per_drone_step"] = row["fused_us_per_step_best"] * 1e3 / (E * D)
        rows.append(row)
        print(json.dumps(row), flush=True)
        for env in envs.values():
            env.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()

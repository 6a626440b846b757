"""Scenarios of the per-env episode tests, shared by the CPU and GPU tests (tests/test_episode_*.py).

One flight -- 120 Hz control, two physics substeps, DYN_DRAG, a replayed table of 5 action sets HOVER_RPM (1 + 0.06 randn), homes at
z = 1.0 + 0.1 d, initial roll / pitch within +-0.1 rad, 120 steps -- under several rules: one sub-scenario per cause with only that
test enabled (a single all-tests-on rule does not exercise every cause), truncation alone, and the combined rule.  The thresholds were
tuned on the float64 oracle alone (tests/test_episode_cpu.py states what they must achieve)."""
import functools

import numpy as np

from oracle import np_oracle as O
from tests.episode_oracle import EpisodeOracle

CTRL_FREQ, PYB_FREQ, STEPS, N_SETS = 120, 240, 120, 5
SHAPES = [(130, 1), (200, 2), (37, 7), (17, 16)]          # ragged last wave | two blocks | odd D, envs straddle waves | D = 16

COMBINED = dict(max_steps=30, z_min=0.975, max_dist=0.035, max_tilt=0.30, max_speed=0.30, max_rate=3.0, reward_r0=2.0, term_penalty=1.5)
RULES = {
    # bit 0: a quarter of the envs start at x = +inf.  (max_steps: with no other test on, the finite envs would drift for the whole run, past
    # 1 m from their targets, where the reward's d^4 amplifies a position error of 1e-5 beyond the reward's own 1e-5 gate: d < 0.63 m keeps
    # 4 d^3 < 1 and the two float32 gates consistent.  Truncation is no cause bit.)
    "nonfinite": dict(max_steps=40, reward_r0=2.0, term_penalty=0.5),
    "z": dict(z_min=0.85, z_max=1.15, max_steps=40, reward_r0=0.1),                       # bit 1 (z_max: above the highest home, see scenario)
    "dist": dict(max_dist=0.02),                                       # bit 2
    "tilt": dict(max_tilt=0.45, max_steps=50, reward_r0=0.1),            # bit 3 (max_steps: no tumbling for 100 steps, see "z" in scenario)
                               # bit 3
    "speed": dict(max_speed=0.2),                                      # bit 4
    "rate": dict(max_rate=2.5, reward_r0=0.1),                            # bit 5
    "trunc": dict(max_steps=17),
    "combined": COMBINED,
}
# (reward_r0 = 0.1 where drones wander up to 1 m from their targets before the enabled test ends the episode: the reward is then 0 beyond
# d = 0.56 m -- the max(0, .) arm -- and 4 d^3 < 1 wherever it is not, so a position error within the 1e-5 gate keeps the reward within its own)
CAUSE_BIT = {"nonfinite": 0, "z": 1, "dist": 2, "tilt": 3, "speed": 4, "rate": 5}


def scenario(E, D, name, seed=7):
    """(xyz [E,D,3], rpy [E,D,3], actions [N_SETS, E*D, 4] float64, params) of sub-scenario `name`"""
    rng = np.random.default_rng(seed + 1000 * D + E)
    xyz = np.zeros((E, D, 3))
    xyz[..., 0] = 0.25 * (np.arange(E) % 8)[:, None] + 0.05 * np.arange(D)[None, :]
    xyz[..., 1] = 0.25 * (np.arange(E) // 8)[:, None]
    xyz[..., 2] = 1.0 + 0.1 * np.arange(D)[None, :]
    rpy = np.zeros((E, D, 3))
    rpy[..., :2] = rng.uniform(-0.1, 0.1, size=(E, D, 2))
    actions = O.CF2P.HOVER_RPM * (1.0 + 0.06 * rng.standard_normal((N_SETS, E * D, 4)))
    params = dict(RULES[name])
    if name == "z":
        # mostly collective thrust noise: the drones climb and sink through the z bounds quickly (few steps near a bound) while their rates
        # stay of order 1 -- an uncontrolled tumble of 100 steps takes float32 past the 1e-5 absolute gate whatever the episode rule does
        # (which is also why this rule and "tilt" truncate: max_steps bounds the free flight; many of these RPMs clip at 0 or MAX_RPM)
        actions = O.CF2P.HOVER_RPM * (1.0 + 0.4 * rng.standard_normal((N_SETS, E * D, 1)) + 0.01 * rng.standard_normal((N_SETS, E * D, 4)))
    if name == "nonfinite":
        xyz[::4, 0, 0] = np.inf                              # the first drone of every fourth env is lost from the start
    if name == "z":                                          # (the homes are 0.1 apart in z: bounds relative to the lowest and the highest)
        params["z_max"] = 1.0 + 0.1 * (D - 1) + 0.15
    return xyz, rpy, actions, params


def make_oracle(E, D, name, **kw):
    xyz, rpy, actions, params = scenario(E, D, name, **kw)
    return EpisodeOracle(xyz, rpy, D, params, pyb_freq=PYB_FREQ, ctrl_freq=CTRL_FREQ, physics="dyn_drag"), actions


@functools.lru_cache(maxsize=None)
def oracle_run(E, D, name, steps=STEPS):
    """The oracle's whole run, computed once per (shape, scenario) and shared: dict of stacked per-step arrays obs [T,n,20], obs_now,
    reward [T,E], flags, margin, plus the counters after every step (lists of dicts).  Treat as read-only."""
    ora, actions = make_oracle(E, D, name)
    rows, counters = [], []
    for k in range(steps):
        rows.append(ora.step(actions[k % N_SETS]))
        counters.append(ora.counters())
    out = {key: np.stack([r[key] for r in rows]) for key in ("obs", "obs_now", "reward", "flags", "margin", "cause", "state", "length")}
    out["counters"] = counters
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out

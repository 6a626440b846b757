"""Scenarios of the collision-cause tests (tests/test_episode_safety_*.py), shared by the CPU and GPU tests.

The flight is tests/episode_cases.scenario's (homes 0.05 apart in x and 0.1 in z within an env, 0.25 between envs) under max_steps = 40 and
no other test on, zscale = 2.  Two drones at their homes have (s^2 + (ez / 2)^4)^(1/4) = 0.0595, so a pair threshold Ds = 2 x 0.0285 = 0.057
lies just inside it: the drift of the free flight takes neighbours across it within an episode.  The obstacle scene is 12 spheres of radius
0.03 centred 0.062 in +y from the homes of drone 0 of the envs at x in {0, 0.75, 1.5}, y in {0, 1, 2, 3}, at z = 1 (Ds = 0.0585).  The
values were probed on the float64 oracle alone (tests/test_episode_safety_cpu.py states what they must achieve)."""
import functools

import numpy as np

from tests import episode_cases as EC
from tests.episode_safety_oracle import EpisodeSafetyOracle

STEPS = EC.STEPS
SAFETY_RADIUS, ZSCALE = 0.0285, 2.0
PARAMS = dict(max_steps=40)
OBSTACLES = np.array([[x, y + 0.062, 1.0, 0.03] for x in (0.0, 0.75, 1.5) for y in (0.0, 1.0, 2.0, 3.0)])
# shape -> it flies among the obstacles.  130 x 1: obstacles only (no env-mates) | 200 x 2: two blocks, both causes | 37 x 7: odd D, envs
# straddle waves | 17 x 16
SHAPES = {(130, 1): True, (200, 2): True, (37, 7): False, (17, 16): False}
FP16_SHAPE = (38, 7)          # fp16 rows are 40 bytes: a log ring needs an even number of drones


def scenario(E, D):
    """(xyz [E,D,3], rpy [E,D,3], actions [N_SETS, E*D, 4] float64, params, obstacles [n_obs,4] or None)"""
    xyz, rpy, actions, _ = EC.scenario(E, D, "trunc")          # the plain flight: no scenario-specific changes to it
    return xyz, rpy, actions, dict(PARAMS), (OBSTACLES if SHAPES.get((E, D), False) else None)


def make_oracle(E, D):
    xyz, rpy, actions, params, obstacles = scenario(E, D)
    ora = EpisodeSafetyOracle(xyz, rpy, D, params, SAFETY_RADIUS, ZSCALE, obstacles, pyb_freq=EC.PYB_FREQ, ctrl_freq=EC.CTRL_FREQ,
                              physics="dyn_drag")
    return ora, actions


@functools.lru_cache(maxsize=None)
def oracle_run(E, D, steps=STEPS):
    """The oracle's whole run, computed once per shape and shared (read-only): episode_cases.oracle_run's arrays plus h_drone [T,n],
    h_min_step [T,E] and h_min_episode [T,E]."""
    ora, actions = make_oracle(E, D)
    rows, counters = [], []
    for k in range(steps):
        rows.append(ora.step(actions[k % EC.N_SETS]))
        counters.append(ora.counters())
    keys = ("obs", "obs_now", "reward", "flags", "margin", "cause", "state", "length", "h_drone", "h_min_step", "h_min_episode")
    out = {key: np.stack([r[key] for r in rows]) for key in keys}
    out["counters"] = counters
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def compared_part(r, near=1e-4):
    """The first-close-call rule of the float32 tests: an env is compared up to, not including, its first step whose margin is under
    `near`.  -> (first [E], keep [T,E])"""
    T = r["margin"].shape[0]
    close = r["margin"] < near
    first = np.where(close.any(axis=0), close.argmax(axis=0), T)
    return first, np.arange(T)[:, None] < first[None, :]

"""Scenarios of the sampled-action tests (tests/test_episode_sample_*.py), shared by the CPU and GPU tests.

The flight, the rule, the targets, the weights and the SHAPES are those of tests/episode_policy_cases.py; the policy's mean action is
replaced by a sample around it.  LOG_STD has four different entries (a swapped index shows), NOISE_SEED differs from the seed of the
randomised starts, and FIRST_ENV gives the shapes different global offsets, one of them zero.  The values were probed on the float64
oracle alone; tests/test_episode_sample_cpu.py states what they must achieve (a few percent of the sample components beyond the +-1
clamp, enough staggered rule terminations, a closed loop that does not amplify float32 rounding)."""
import functools

import numpy as np

from tests import episode_policy_cases as PC
from tests import episode_random_cases as RC
from tests import episode_safety_cases as SC
from tests import episode_sample_oracle as SO
from tests.episode_oracle import EpisodeOracle
from tests.episode_random_oracle import RandomEpisodeSafetyOracle

CTRL_FREQ, PYB_FREQ, SHAPES, STEPS = PC.CTRL_FREQ, PC.PYB_FREQ, PC.SHAPES, PC.STEPS
NET = PC.ROLLOUT_NET
LOG_STD = (-1.2, -1.5, -1.0, -1.8)
NOISE_SEED = 0x5EED0F0A1B2C3D4E
assert NOISE_SEED != RC.SEED
FIRST_ENV = {(130, 1): 0, (200, 2): 1000, (37, 7): 0, (17, 16): 5}


class RoundingSamplingDriver(SO.SamplingDriver):
    """SamplingDriver with the state the step starts from and the commanded RPM rounded to float32 at every step (as
    tests/episode_policy_cases.RoundingDriver)"""

    def step(self):
        av = self.ora.av
        for k in ("pos", "quat", "vel", "rates", "ang_v"):
            setattr(av, k, PC._f32(getattr(av, k)))
        acted = av.obs().copy()
        d = self.draw(acted)
        d["action"] = PC._f32(d["action"])
        r = self.ora.step(d["action"])
        r.update(d)
        r["acted_obs"] = acted
        return r


def make_driver(E, D, round32=False, log_std=LOG_STD, seed=NOISE_SEED, first_env=None):
    """the sampling oracle of the flight; round32 == "every step": start poses, targets and weights rounded to float32 first, and the
    state and the commanded RPM again at every step"""
    xyz, rpy, params, target = PC.scenario(E, D)
    w = PC.weights(*NET[:2])
    if round32:
        xyz, rpy, w, target = (PC._f32(a) for a in (xyz, rpy, w, target))
    ora = EpisodeOracle(xyz, rpy, D, params, target=target, pyb_freq=PYB_FREQ, ctrl_freq=CTRL_FREQ, physics="dyn_drag", integrator="euler")
    cls = RoundingSamplingDriver if round32 == "every step" else SO.SamplingDriver
    return cls(ora, w, *NET, log_std=log_std, seed=seed, first_env=FIRST_ENV[(E, D)] if first_env is None else first_env)


KEYS = PC.KEYS + ("sample", "logp", "eps", "acted_obs")


@functools.lru_cache(maxsize=None)
def oracle_run(E, D, round32=False, steps=STEPS, log_std=LOG_STD):
    """The oracle's whole run, computed once per shape and shared (read-only): episode_policy_cases.oracle_run's arrays plus sample
    [T,n,4], logp [T,n], eps [T,n,4] and acted_obs [T,n,20]"""
    return PC._run(make_driver(E, D, round32, log_std), steps, KEYS)


def compared_part(r, near=1e-4):
    return PC.compared_part(r, near)


# ---- with the collision causes and randomised starts configured (tests/episode_policy_cases.make_safety_driver, sampled)
SAFETY_SHAPE = PC.SAFETY_SHAPE


def make_safety_driver(E=SAFETY_SHAPE[0], D=SAFETY_SHAPE[1]):
    xyz, rpy, _, params, obstacles = SC.scenario(E, D)
    ora = RandomEpisodeSafetyOracle(xyz, rpy, D, params, SC.SAFETY_RADIUS, SC.ZSCALE, obstacles, pyb_freq=PYB_FREQ, ctrl_freq=CTRL_FREQ,
                                    physics="dyn_drag")
    ora.set_randomisation(RC.SEED, **RC.HALF)
    return SO.SamplingDriver(ora, PC.weights(*NET[:2]), *NET, log_std=LOG_STD, seed=NOISE_SEED)


@functools.lru_cache(maxsize=None)
def safety_oracle_run(steps=STEPS):
    """reset_episodes() (generation 1, epoch 1), then `steps` sampled steps: the arrays of oracle_run plus h_min_step, h_min_episode
    [T,E] and first_rows [n,20]"""
    drv = make_safety_driver()
    first = drv.reset_episodes()
    out = PC._run(drv, steps, KEYS + ("h_min_step", "h_min_episode"))
    out["first_rows"] = first
    return out

"""Scenarios of the episode-policy tests (tests/test_episode_policy_*.py), shared by the CPU and GPU tests.

The flight is tests/episode_cases.py's -- 120 Hz control, two physics substeps, DYN_DRAG, the homes and initial tilts of its scenario(),
its SHAPES, its combined rule -- with the replayed table replaced by an MLP policy of seeded Gaussian weights (two hidden layers of 64,
tanh: the shape the feature exists for).  The weight scales were probed on the float64 oracle alone
(tests/test_episode_policy_cpu.py states what they must achieve): large enough that the drones do not just hover and that some
action components reach the +-1 clamp, small enough that most do not and that the closed loop does not amplify float32 rounding past a
tenth of the float32 gates."""
import functools

import numpy as np

from tests import episode_cases as EC
from tests import episode_policy_oracle as PO
from tests import episode_safety_cases as SC
from tests import episode_random_cases as RC
from tests.episode_oracle import EpisodeOracle
from tests.episode_random_oracle import RandomEpisodeSafetyOracle

CTRL_FREQ, PYB_FREQ, SHAPES = EC.CTRL_FREQ, EC.PYB_FREQ, EC.SHAPES
STEPS = 120
# The combined rule of tests/episode_cases.py with shorter episodes and a rate bound that the flight crosses inside them.  In float32 the
# closed loop turns every step's rounding into a torque error that stays (the policy's output is nearly steady within an episode), so the
# body rates drift linearly with the episode's age, about 4e-7 rad/s per step in this flight: 12 steps keep that under half of the 1e-5
# gate, 30 reach it (probed on the oracle with the state and the commanded RPM rounded to float32 after every step,
# make_driver(round32="every step")).  max_rate = 1.2 rad/s is crossed at an episode age of 8 to 12 steps, at different steps in
# different envs: terminations (cause bit 5, the penalty arm of the reward) staggered within a workgroup, and truncations beside them.
RULE = dict(EC.COMBINED, max_steps=12, max_rate=1.2)
# What makes the envs differ: every drone's target is its home plus a uniform offset of up to TARGET_OFFSET (e % 4 + 1) / 4 per axis, so
# the position feature starts away from zero, by another amount in every env (with the homes as targets every drone sees nearly the same
# features and all envs end their episodes in lockstep).
TARGET_OFFSET = 0.3
# the networks of the policy-alone tests: (n_hidden, width, activation)
NETS = [(nh, w, act) for w in (5, 32, 64) for nh in (1, 2) for act in ("tanh", "relu")]
ROLLOUT_NET = (2, 64, "tanh")
WEIGHT_SEED = 2024
# standard deviations: a hidden layer's weights are GAIN / sqrt(fan_in), the output layer's OUT_GAIN / sqrt(fan_in), biases BIAS.
# The first layer's rows are further scaled per feature group (position error, angles, velocity, angular velocity: m, rad, m/s, rad/s
# of very different sizes in this flight) so that each group moves the pre-activations by a comparable amount.
GAIN, OUT_GAIN, BIAS = 1.0, 1.6, 0.3
FEATURE_GAIN = np.repeat([2.5, 2.0, 2.0, 0.25], 3)


def weights(n_hidden, width, seed=WEIGHT_SEED):
    """the packed float64 weight vector of a seeded random policy"""
    rng = np.random.default_rng([seed, n_hidden, width])
    dims = [PO.N_IN] + [width] * n_hidden + [PO.N_OUT]
    out = []
    for l, (i, o) in enumerate(zip(dims[:-1], dims[1:])):
        last = l == n_hidden
        A = rng.standard_normal((o, i)) * ((OUT_GAIN if last else GAIN) / np.sqrt(i))
        if l == 0:
            A = A * FEATURE_GAIN[None, :]
        out += [A.reshape(-1), rng.standard_normal(o) * (0.0 if last else BIAS)]
    return np.concatenate(out)


def observations(n, seed=5):
    """random observation rows [n, 20] and world-frame targets [n, 3] of the policy-alone tests: positions within 0.1 m of the targets,
    angles within 0.5 rad, speeds within 0.5 m/s, rates within 3 rad/s (the ranges of the flight)"""
    rng = np.random.default_rng([seed, n])
    obs = np.zeros((n, 20))
    target = rng.uniform(-2.0, 2.0, size=(n, 3))
    obs[:, 0:3] = target + rng.uniform(-0.1, 0.1, size=(n, 3))
    obs[:, 3:7] = rng.standard_normal((n, 4))
    obs[:, 3:7] /= np.linalg.norm(obs[:, 3:7], axis=1, keepdims=True)
    obs[:, 7:10] = rng.uniform(-0.5, 0.5, size=(n, 3))
    obs[:, 10:13] = rng.uniform(-0.5, 0.5, size=(n, 3))
    obs[:, 13:16] = rng.uniform(-3.0, 3.0, size=(n, 3))
    obs[:, 16:20] = 14000.0
    return obs, target


def scenario(E, D):
    """(xyz [E,D,3], rpy [E,D,3], params, target [E,D,3] world frame) of the flight"""
    xyz, rpy, _, _ = EC.scenario(E, D, "combined")
    rng = np.random.default_rng([11, E, D])
    target = xyz + rng.uniform(-TARGET_OFFSET, TARGET_OFFSET, size=xyz.shape) * (((np.arange(E) % 4) + 1) / 4.0)[:, None, None]
    return xyz, rpy, dict(RULE), target


def _f32(a):
    return np.asarray(a).astype(np.float32).astype(np.float64)


class RoundingDriver(PO.PolicyDriver):
    """PolicyDriver with the state the step starts from and the commanded RPM rounded to float32 at every step: what any float32
    implementation stores between steps, whatever its arithmetic within one"""

    def step(self):
        av = self.ora.av
        for k in ("pos", "quat", "vel", "rates", "ang_v"):
            setattr(av, k, _f32(getattr(av, k)))
        action, y = self.act(av.obs())
        action = _f32(action)
        r = self.ora.step(action)
        r["action"], r["y"] = action, y
        return r


def make_driver(E, D, round32=False, net=ROLLOUT_NET, physics="dyn_drag", integrator="euler"):
    """the policy-driven oracle of the flight; round32: start poses, targets and weights rounded to float32 first (and stepped in
    float64); round32 == "every step": the state and the commanded RPM are rounded again at every step as well"""
    xyz, rpy, params, target = scenario(E, D)
    w = weights(*net[:2])
    if round32:
        xyz, rpy, w, target = (_f32(a) for a in (xyz, rpy, w, target))
    ora = EpisodeOracle(xyz, rpy, D, params, target=target, pyb_freq=PYB_FREQ, ctrl_freq=CTRL_FREQ, physics=physics, integrator=integrator)
    return (RoundingDriver if round32 == "every step" else PO.PolicyDriver)(ora, w, *net)


KEYS = ("obs", "obs_now", "reward", "flags", "margin", "action", "y")


def _run(drv, steps, keys=KEYS):
    rows, counters = [], []
    for _ in range(steps):
        rows.append(drv.step())
        counters.append(drv.ora.counters())
    out = {key: np.stack([r[key] for r in rows]) for key in keys}
    out["counters"] = counters
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def oracle_run(E, D, round32=False, steps=STEPS):
    """The oracle's whole run, computed once per shape and shared (read-only): episode_cases.oracle_run's arrays plus action [T,n,4] (the
    commanded RPM) and y [T,n,4] (the network's output before the clamp)."""
    return _run(make_driver(E, D, round32), steps)


RK4_NET, RK4_SHAPE, RK4_STEPS = (2, 5, "tanh"), (37, 7), 40


@functools.lru_cache(maxsize=None)
def rk4_oracle_run():
    """the same flight under the RK4 integrator without drag, a 5-wide policy, 40 steps: the float64 + RK4 handle, whose policy the
    library pads to 64 whatever its width"""
    return _run(make_driver(*RK4_SHAPE, net=RK4_NET, physics="dyn", integrator="rk4"), RK4_STEPS)


def compared_part(r, near=1e-4):
    return SC.compared_part(r, near)


# ---- with the collision causes and randomised starts configured: the safety flight of tests/episode_safety_cases.py (its rule, radius and
# zscale) on 37 x 7, the randomisation of tests/episode_random_cases.py (its seed and half-widths: position and attitude non-zero)
SAFETY_SHAPE = RC.SAFETY_SHAPE
SAFETY_PARAMS = dict(SC.PARAMS)


def make_safety_driver(E=SAFETY_SHAPE[0], D=SAFETY_SHAPE[1]):
    xyz, rpy, _, params, obstacles = SC.scenario(E, D)
    ora = RandomEpisodeSafetyOracle(xyz, rpy, D, params, SC.SAFETY_RADIUS, SC.ZSCALE, obstacles, pyb_freq=PYB_FREQ, ctrl_freq=CTRL_FREQ,
                                    physics="dyn_drag")
    ora.set_randomisation(RC.SEED, **RC.HALF)
    return PO.PolicyDriver(ora, weights(*ROLLOUT_NET[:2]), *ROLLOUT_NET)


@functools.lru_cache(maxsize=None)
def safety_oracle_run(steps=STEPS):
    """reset_episodes() (generation 1), then `steps` policy steps: the arrays of oracle_run plus h_min_step and h_min_episode [T,E], and
    first_rows [n,20]"""
    drv = make_safety_driver()
    first = drv.ora.reset_episodes()
    out = _run(drv, steps, KEYS + ("h_min_step", "h_min_episode"))
    out["first_rows"] = first
    return out

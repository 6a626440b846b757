"""float64 oracle of the per-env episodes (mds_set_episodes / mds_rollout_episodes): oracle.np_oracle.AviaryOracle stepped under the
episode rule of multidronesim_amd/csrc/mds_episode.hpp, restated here in NumPy.

Besides flags and reward every env-step reports its MARGIN: the smallest |tested quantity - threshold| / |threshold| over the enabled
tests and the env's drones -- how far the nearest decision of this step was from going the other way.  A lower-precision run may
decide differently only where the margin is small.  (The max_steps count is an integer compare, exact in every dtype: it has no
margin.)"""
import numpy as np

from oracle import np_oracle as O

TERMINATED, TRUNCATED, CAUSE_SHIFT = 1, 2, 8
PARAM_DEFAULTS = dict(max_steps=0, z_min=-np.inf, z_max=np.inf, max_dist=np.inf, max_tilt=np.inf, max_speed=np.inf, max_rate=np.inf,
                      reward_r0=2.0, term_penalty=0.0)


def _on(name, v):
    """the threshold's test is enabled (mds_episode.hpp fill_episode_rule)"""
    if not np.isfinite(v):
        return False
    if name in ("z_min", "z_max"):
        return True
    if name == "max_tilt":
        return 0.0 < v < np.pi
    return v > 0.0


def causes_and_margin(params, pos, quat, vel, rate_norm2, finite, home):
    """Per drone: cause bits (int [n]) and margin (float [n]) from world position [n,3], quaternion xyzw [n,4], velocity [n,3], the squared
    norm of the angular velocity [n], `finite` [n] (every state component is) and the reset position `home` [n,3]."""
    p = {**PARAM_DEFAULTS, **params}
    n = pos.shape[0]
    cause = np.where(finite, 0, 1).astype(np.int64)
    margin = np.full(n, np.inf)

    def test(bit, fired, quantity, thr):
        nonlocal cause, margin
        cause = cause | np.where(fired, bit, 0)
        with np.errstate(invalid="ignore"):
            m = np.abs(quantity - thr) / (abs(thr) if thr != 0 else 1.0)
        margin = np.fmin(margin, m)                # (a NaN quantity has no margin: bit 0 decides such a drone)

    with np.errstate(invalid="ignore", over="ignore"):
        if _on("z_min", p["z_min"]):
            test(2, pos[:, 2] < p["z_min"], pos[:, 2], p["z_min"])
        if _on("z_max", p["z_max"]):
            test(2, pos[:, 2] > p["z_max"], pos[:, 2], p["z_max"])
        if _on("max_dist", p["max_dist"]):
            d2 = ((pos - home) ** 2).sum(-1)
            test(4, d2 > p["max_dist"] ** 2, np.sqrt(d2), p["max_dist"])
        if _on("max_tilt", p["max_tilt"]):
            cz = 1.0 - 2.0 * (quat[:, 0] ** 2 + quat[:, 1] ** 2)
            test(8, cz < np.cos(p["max_tilt"]), cz, np.cos(p["max_tilt"]))
        if _on("max_speed", p["max_speed"]):
            v2 = (vel ** 2).sum(-1)
            test(16, v2 > p["max_speed"] ** 2, np.sqrt(v2), p["max_speed"])
        if _on("max_rate", p["max_rate"]):
            test(32, rate_norm2 > p["max_rate"] ** 2, np.sqrt(rate_norm2), p["max_rate"])
    return cause, margin


def causes_from_obs(params, obs, home):
    """the same from observation rows [n,20] (pos 0:3 | quat 3:7 | vel 10:13 | world ang_vel 13:16, whose norm is the body rates')"""
    cols = np.r_[0:7, 10:16]
    return causes_and_margin(params, obs[:, 0:3], obs[:, 3:7], obs[:, 10:13], (obs[:, 13:16] ** 2).sum(-1), np.isfinite(obs[:, cols]).all(-1), home)


def env_flags(params, cause_env, length):
    """flags word per env from the OR of its drones' cause bits and the length its episode has reached with this step"""
    p = {**PARAM_DEFAULTS, **params}
    term = cause_env != 0
    trunc = ~term & (p["max_steps"] > 0) & (length >= p["max_steps"])
    return term * TERMINATED + trunc * TRUNCATED + (cause_env << CAUSE_SHIFT)


def tally_step(params, t, cause_env, term_sum):
    """One control step of E envs' counters (mds_episode.hpp episode_env_step).  t holds the arrays length, count, sum_length (integer) and
    ret, sum_return (float64 or float32: the step's arithmetic runs in their dtype), each [E], and is updated in place; cause_env [E] is the
    OR of each env's cause bits, term_sum [E] the sum of its reward terms.  -> flags, reward, done, and the length the episode had reached."""
    p = {**PARAM_DEFAULTS, **params}
    ft = t.ret.dtype.type
    t.length += 1
    flags = env_flags(p, cause_env, t.length)
    length = t.length.copy()
    with np.errstate(invalid="ignore", over="ignore"):
        term_sum = np.asarray(term_sum, dtype=ft)
        reward = np.where(flags & TERMINATED, term_sum - ft(p["term_penalty"]), term_sum)
        t.ret += reward
        done = (flags & (TERMINATED | TRUNCATED)) != 0
        t.count += done
        t.sum_return[done] += t.ret[done]
    t.sum_length[done] += t.length[done]
    t.length[done] = 0
    t.ret[done] = 0.0
    return flags, reward, done, length


class EpisodeOracle:
    """AviaryOracle + the episode rule, for E envs of D drones (drone i belongs to env i // D)."""

    def __init__(self, xyz, rpy, D, params, target=None, **aviary_kw):
        self.av = O.AviaryOracle(np.asarray(xyz, dtype=np.float64).reshape(-1, 3), np.asarray(rpy, dtype=np.float64).reshape(-1, 3), **aviary_kw)
        self.n, self.D = self.av.init_xyzs.shape[0], D
        self.E = self.n // D
        self.params = {**PARAM_DEFAULTS, **params}
        self.home = self.av.init_xyzs.copy()
        self.target = self.home.copy() if target is None else np.asarray(target, dtype=np.float64).reshape(-1, 3)
        self.length = np.zeros(self.E, dtype=np.int64)
        self.ret = np.zeros(self.E)
        self.count = np.zeros(self.E, dtype=np.int64)
        self.sum_return = np.zeros(self.E)
        self.sum_length = np.zeros(self.E, dtype=np.int64)

    def _reset_envs(self, done):
        av, m = self.av, np.repeat(done, self.D)
        av.pos[m] = av.init_xyzs[m]
        av.quat[m] = O.quat_from_euler_bullet(av.init_rpys[m])
        av.vel[m] = 0.0
        av.rates[m] = 0.0
        av.ang_v[m] = 0.0
        av.last_clipped_action = np.where(m[:, None], 0.0, av.last_clipped_action)

    def step(self, action):
        """One control step.  Returns a dict: obs [n,20] the transition's rows (before any reset), reward [E], flags [E], margin [E],
        cause [n] per drone, state [n,13] the stepped state the rule saw, length [E] the episode length it saw, obs_now [n,20] the current rows (after the resets)."""
        av, p, E, D = self.av, self.params, self.E, self.D
        obs = av.step(action)
        state = np.concatenate([av.pos, av.quat, av.vel, av.rates], axis=-1)
        cause, margin = causes_and_margin(p, av.pos, av.quat, av.vel, (av.rates ** 2).sum(-1), np.isfinite(state).all(-1), self.home)
        cause_env = np.bitwise_or.reduce(cause.reshape(E, D), axis=1)
        with np.errstate(invalid="ignore", over="ignore"):
            d2 = ((av.pos - self.target) ** 2).sum(-1)
            v = p["reward_r0"] - d2 * d2
        terms = np.where(v > 0, v, 0.0).reshape(E, D)
        term_sum = np.zeros(E)
        for d in range(D):                                   # drone order
            term_sum = term_sum + terms[:, d]
        flags, reward, done, length = tally_step(p, self, cause_env, term_sum)
        if done.any():
            self._reset_envs(done)
        return dict(obs=obs, reward=reward, flags=flags.astype(np.int64), margin=margin.reshape(E, D).min(axis=1), cause=cause,
                    state=state, length=length, obs_now=av.obs() if done.any() else obs)

    def counters(self):
        return dict(length=self.length.copy(), ret=self.ret.copy(), count=self.count.copy(), sum_return=self.sum_return.copy(),
                    sum_length=self.sum_length.copy())

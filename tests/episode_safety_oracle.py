"""float64 oracle of the collision causes of the per-env episodes (mds_set_episode_safety): tests/episode_oracle.py's EpisodeOracle with
the two cause bits of multidronesim_amd/csrc/mds_episode.hpp added before the env's OR, and the env's smallest h.

    h = (ex^2 + ey^2)^2 + (ez / zscale)^4 - Ds^4      Ds = 2 safety_radius (two drones of an env), safety_radius + r (a sphere obstacle)

bit 6: a drone has an env-mate with h < 0; bit 7: a drone has an obstacle with h < 0; a NaN h fires neither.  The margin of a tested
separation is |(s^2 + (ez / zscale)^4)^(1/4) - Ds| / Ds, s = ex^2 + ey^2: the relative distance to the threshold in the length the set is
stated in, the same kind of quantity as the margins of episode_oracle.causes_and_margin."""
import numpy as np

from tests import episode_oracle as EO

PAIR, OBSTACLE = 1 << 6, 1 << 7


def barrier(e, zscale, Ds):
    """h and margin of separations e [..., 3] against Ds (scalar or broadcastable)"""
    with np.errstate(invalid="ignore", over="ignore"):
        s = e[..., 0] ** 2 + e[..., 1] ** 2
        q = s * s + (e[..., 2] / zscale) ** 4
        return q - Ds ** 4, np.abs(q ** 0.25 - Ds) / Ds


def safety_causes(pos, D, safety_radius, zscale, obstacles):
    """Per drone from world positions [n,3]: cause bits (int [n]), smallest h (float [n], +inf with nothing to test) and margin (float [n])."""
    n = pos.shape[0]
    E = n // D
    cause = np.zeros(n, dtype=np.int64)
    h_min, margin = np.full(n, np.inf), np.full(n, np.inf)
    if D > 1:
        p = pos.reshape(E, D, 3)
        with np.errstate(invalid="ignore"):
            h, m = barrier(p[:, :, None, :] - p[:, None, :, :], zscale, 2.0 * safety_radius)            # [E, D, D]
        other = ~np.eye(D, dtype=bool)[None]
        with np.errstate(invalid="ignore"):
            cause |= np.where((other & (h < 0)).any(axis=2).reshape(n), PAIR, 0)
        h_min = np.fmin(h_min, np.fmin.reduce(np.where(other, h, np.inf), axis=2).reshape(n))
        margin = np.fmin(margin, np.fmin.reduce(np.where(other, m, np.inf), axis=2).reshape(n))
    if obstacles is not None and len(obstacles):
        ob = np.asarray(obstacles, dtype=np.float64).reshape(-1, 4)
        with np.errstate(invalid="ignore"):
            h, m = barrier(pos[:, None, :] - ob[None, :, :3], zscale, safety_radius + ob[None, :, 3])   # [n, n_obs]
            cause |= np.where((h < 0).any(axis=1), OBSTACLE, 0)
        h_min = np.fmin(h_min, np.fmin.reduce(h, axis=1))
        margin = np.fmin(margin, np.fmin.reduce(m, axis=1))
    return cause, h_min, margin


class EpisodeSafetyOracle(EO.EpisodeOracle):
    """EpisodeOracle + the safety set.  step() returns EpisodeOracle.step's dict (cause and margin with the new tests in them) plus h_drone [n],
    h_min_step [E] and h_min_episode [E] (after the step: +inf again where the episode restarted)."""

    def __init__(self, xyz, rpy, D, params, safety_radius, zscale=2.0, obstacles=None, **aviary_kw):
        super().__init__(xyz, rpy, D, params, **aviary_kw)
        self.safety_radius, self.zscale = float(safety_radius), float(zscale)
        self.obstacles = None if obstacles is None else np.asarray(obstacles, dtype=np.float64).reshape(-1, 4)
        self.h_min_episode = np.full(self.E, np.inf)

    def step(self, action):
        av, p, E, D = self.av, self.params, self.E, self.D
        obs = av.step(action)
        state = np.concatenate([av.pos, av.quat, av.vel, av.rates], axis=-1)
        cause, margin = EO.causes_and_margin(p, av.pos, av.quat, av.vel, (av.rates ** 2).sum(-1), np.isfinite(state).all(-1), self.home)
        c2, h_drone, m2 = safety_causes(av.pos, D, self.safety_radius, self.zscale, self.obstacles)
        cause, margin = cause | c2, np.fmin(margin, m2)
        cause_env = np.bitwise_or.reduce(cause.reshape(E, D), axis=1)
        h_min_step = h_drone.reshape(E, D).min(axis=1)
        self.h_min_episode = np.minimum(self.h_min_episode, h_min_step)
        with np.errstate(invalid="ignore", over="ignore"):
            d2 = ((av.pos - self.target) ** 2).sum(-1)
            v = p["reward_r0"] - d2 * d2
        terms = np.where(v > 0, v, 0.0).reshape(E, D)
        term_sum = np.zeros(E)
        for d in range(D):                                   # drone order
            term_sum = term_sum + terms[:, d]
        flags, reward, done, length = EO.tally_step(p, self, cause_env, term_sum)
        self.h_min_episode[done] = np.inf
        if done.any():
            self._reset_envs(done)
        return dict(obs=obs, reward=reward, flags=flags.astype(np.int64), margin=margin.reshape(E, D).min(axis=1), cause=cause,
                    state=state, length=length, obs_now=av.obs() if done.any() else obs, h_drone=h_drone, h_min_step=h_min_step,
                    h_min_episode=self.h_min_episode.copy())

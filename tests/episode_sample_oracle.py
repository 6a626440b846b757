"""float64 oracle of the Gaussian actions of the MLP policy (mds_set_episode_policy_noise / mds_rollout_episodes_sampled /
mds_episode_policy_sample): a NumPy restatement of multidronesim_amd/csrc/mds_policy_noise.hpp on the Philox of
tests/episode_random_oracle.py, and a PolicyDriver that samples.

    key = (seed low word, seed high word)      counter = (g, ordinal, 3 + length, epoch)  (mod 2^32)
    (w0, w1) -> eps[0], eps[1];  (w2, w3) -> eps[2], eps[3]:
        u = (2 (w_a >> 9) + 1) 2^-24,  r = sqrt(-2 ln u),  theta = pi * unit(w_b),  eps = r cos(theta), r sin(theta)
    a = y + exp(log_std) eps          rpm = rpm_base + rpm_scale * clip(a, -1, 1)
    logp = -(0.5 sum eps^2) - (sum log_std + 2 ln(2 pi))"""
import numpy as np

from tests import episode_policy_oracle as PO
from tests import episode_random_oracle as RO

BLOCK0 = 3


def words(seed, g, ordinal, length, epoch):
    """the Philox block [n, 4] (uint64 holding 32-bit words) of drones g [n] at ordinal [n], length [n]; epoch a scalar or [n]"""
    g = np.asarray(g, dtype=np.uint64) & RO.MASK
    ordinal = np.broadcast_to(np.asarray(ordinal, dtype=np.uint64) & RO.MASK, g.shape)
    w2 = np.broadcast_to((np.asarray(length, dtype=np.uint64) + np.uint64(BLOCK0)) & RO.MASK, g.shape)
    ep = np.broadcast_to(np.asarray(epoch, dtype=np.uint64) & RO.MASK, g.shape)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    key = np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64)
    return RO.philox4x32_10(np.stack([g, ordinal, w2, ep], axis=-1), key)


def box_muller(w):
    """eps [..., 4] of words [..., 4]"""
    w = np.asarray(w, dtype=np.uint64)

    def pair(wa, wb):
        u = (2 * (wa >> np.uint64(9)).astype(np.int64) + 1).astype(np.float64) * 2.0 ** -24
        r = np.sqrt(-2.0 * np.log(u))
        theta = np.pi * RO.unit(wb)
        return r * np.cos(theta), r * np.sin(theta)

    e0, e1 = pair(w[..., 0], w[..., 1])
    e2, e3 = pair(w[..., 2], w[..., 3])
    return np.stack([e0, e1, e2, e3], axis=-1)


def eps_of(seed, g, ordinal, length, epoch):
    return box_muller(words(seed, g, ordinal, length, epoch))


def sample(y, eps, log_std):
    """(a [n, 4], logp [n]) of the network's output y [n, 4] and the normals eps [n, 4]"""
    log_std = np.asarray(log_std, dtype=np.float64)
    a = y + np.exp(log_std)[None, :] * eps
    ss = np.zeros(eps.shape[0])
    for j in range(4):                                       # j ascending
        ss = ss + eps[:, j] * eps[:, j]
    return a, -(0.5 * ss) - (log_std.sum() + 2.0 * np.log(2.0 * np.pi))


class SamplingDriver(PO.PolicyDriver):
    """PolicyDriver whose step() draws: it reads the wrapped oracle's count and length per env (before the step), draws, and returns
    beside the oracle's dict action [n, 4] (the commanded RPM of the clipped sample), sample [n, 4], logp [n], eps [n, 4], y [n, 4]
    and acted_obs [n, 20] (the rows the action was drawn on).  epoch: 0 at construction, + 1 with reset_episodes()."""

    def __init__(self, ora, weights, n_hidden, width, activation="tanh", log_std=(0.0, 0.0, 0.0, 0.0), seed=0, first_env=0, rpm_base=None,
                 rpm_scale=None):
        super().__init__(ora, weights, n_hidden, width, activation, rpm_base, rpm_scale)
        self.log_std = np.broadcast_to(np.asarray(log_std, dtype=np.float64), (4,)).copy()
        self.seed, self.first, self.epoch = int(seed), int(first_env) * ora.D, 0

    def draw(self, obs):
        """the action the policy takes on the rows obs at the oracle's current counters"""
        ora = self.ora
        _, y = self.act(obs)
        g = self.first + np.arange(ora.n)
        eps = eps_of(self.seed, g, np.repeat(ora.count, ora.D), np.repeat(ora.length, ora.D), self.epoch)
        a, logp = sample(y, eps, self.log_std)
        return dict(action=PO.rpm_of(a, self.rpm_base, self.rpm_scale), sample=a, logp=logp, eps=eps, y=y)

    def reset_episodes(self):
        self.epoch += 1
        return self.ora.reset_episodes()

    def step(self):
        acted = self.ora.av.obs().copy()
        d = self.draw(acted)
        r = self.ora.step(d["action"])
        r.update(d)
        r["acted_obs"] = acted
        return r

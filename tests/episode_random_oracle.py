"""float64 oracle of the randomised episode starts (mds_set_episode_randomisation / mds_reset_episodes): Philox4x32-10 and the draw of
multidronesim_amd/csrc/mds_episode_random.hpp restated in NumPy (uint64 arithmetic, vectorised), and a mixin that puts the drawn start
where tests/episode_oracle.py and tests/episode_safety_oracle.py put the fixed one.

    key = (seed low word, seed high word)      counter = (g, ordinal, b, generation), b = 0, 1, 2
    word x -> k = 2 (x >> 8) + 1 - 2^24 -> s = k 2^-24 -> offset = s * half_width
    the twelve words of blocks 0..2: position xyz | roll pitch yaw | world velocity xyz | body rates xyz

The oracle does not round through a storage type: the float64 device run has none to round through, and the fp16-storage test states its
own tolerance for it."""
import numpy as np

from oracle import np_oracle as O
from tests import episode_oracle as EO
from tests import episode_safety_oracle as SO

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
MASK = np.uint64(0xFFFFFFFF)
SHIFT = np.uint64(32)


def philox4x32_10(counter, key):
    """counter [..., 4], key [..., 2] (integers below 2^32, broadcast against each other) -> uint64 [..., 4] holding the four output words"""
    counter, key = np.asarray(counter, dtype=np.uint64), np.asarray(key, dtype=np.uint64)
    shape = np.broadcast_shapes(counter.shape[:-1], key.shape[:-1])
    c0, c1, c2, c3 = (np.broadcast_to(counter[..., k], shape).copy() for k in range(4))
    k0, k1 = (np.broadcast_to(key[..., k], shape).copy() for k in range(2))
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2                            # 32 x 32 -> 64: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> SHIFT) ^ c1 ^ k0, p1 & MASK, (p0 >> SHIFT) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return np.stack([c0, c1, c2, c3], axis=-1)


def unit(words):
    """s in (-1, 1) of output words (uint64 holding 32-bit values): an odd multiple of 2^-24"""
    k = 2 * (np.asarray(words, dtype=np.uint64) >> np.uint64(8)).astype(np.int64) + 1 - (1 << 24)
    return k.astype(np.float64) * 2.0 ** -24


def units(seed, g, ordinal, generation):
    """the twelve s values [n, 12] of drones g [n] in the episodes ordinal [n]; generation a scalar or [n]"""
    g, ordinal = np.asarray(g, dtype=np.uint64) & MASK, np.asarray(ordinal, dtype=np.uint64) & MASK
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    key = np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64)
    gen = np.broadcast_to(np.asarray(generation, dtype=np.uint64) & MASK, g.shape)
    blocks = [philox4x32_10(np.stack([g, ordinal, np.full_like(g, b), gen], axis=-1), key) for b in range(3)]
    return unit(np.concatenate(blocks, axis=-1))


def half_widths(pos=0.0, rpy=0.0, vel=0.0, rate=0.0):
    return np.concatenate([np.broadcast_to(np.asarray(v, dtype=np.float64), (3,)) for v in (pos, rpy, vel, rate)])


def offsets(seed, g, ordinal, generation, half):
    """[n, 12]: exactly 0 where the half-width is"""
    return units(seed, g, ordinal, generation) * np.asarray(half, dtype=np.float64)[None, :] + 0.0


def start_state(seed, g, ordinal, generation, half, xyz, rpy):
    """drawn start [n, 13] = pos3 | quat4 xyzw | vel3 | body rates3 around the nominal poses xyz, rpy [n, 3]"""
    o = offsets(seed, g, ordinal, generation, half)
    return np.concatenate([xyz + o[:, 0:3], O.quat_from_euler_bullet(rpy + o[:, 3:6]), o[:, 6:9], o[:, 9:12]], axis=-1)


class RandomStartMixin:
    """_reset_envs of EpisodeOracle / EpisodeSafetyOracle with the drawn start (both call it after `count` is incremented), and
    reset_episodes().  Without set_randomisation the base class's fixed reset stays."""
    rand = None

    def set_randomisation(self, seed, pos=0.0, rpy=0.0, vel=0.0, rate=0.0, first_env=0):
        self.rand = dict(seed=int(seed), half=half_widths(pos, rpy, vel, rate), first=int(first_env) * self.D)
        self.generation = 0

    def _reset_envs(self, done):
        if self.rand is None:
            return super()._reset_envs(done)
        av, m = self.av, np.repeat(done, self.D)
        g = self.rand["first"] + np.flatnonzero(m)
        st = start_state(self.rand["seed"], g, np.repeat(self.count, self.D)[m], self.generation, self.rand["half"], av.init_xyzs[m], av.init_rpys[m])
        av.pos[m], av.quat[m], av.vel[m], av.rates[m] = st[:, 0:3], st[:, 3:7], st[:, 7:10], st[:, 10:13]
        av.ang_v[m] = O.matvec(O.quat_to_rotmat_bullet(av.quat[m]), av.rates[m])
        av.last_clipped_action = np.where(m[:, None], 0.0, av.last_clipped_action)

    def reset_episodes(self):
        """mds_reset_episodes: generation + 1, every drone to its drawn start, every running episode restarted.  Returns the rows [n, 20]."""
        self.generation += 1
        self._reset_envs(np.ones(self.E, dtype=bool))
        self.length[:] = 0
        self.ret[:] = 0.0
        if hasattr(self, "h_min_episode"):
            self.h_min_episode[:] = np.inf
        return self.av.obs()


class RandomEpisodeOracle(RandomStartMixin, EO.EpisodeOracle):
    pass


class RandomEpisodeSafetyOracle(RandomStartMixin, SO.EpisodeSafetyOracle):
    pass

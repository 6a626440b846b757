"""float64 oracle of the MLP policy of the per-env episodes (mds_set_episode_policy / mds_rollout_episodes_policy): a NumPy
restatement of multidronesim_amd/csrc/mds_policy.hpp -- current rows -> features -> layers -> clamp -> RPM -- driving any of the
episode oracles (tests/episode_oracle.py, episode_safety_oracle.py, episode_random_oracle.py) through their own step().

    x = obs[0:3] - target | obs[7:10] | obs[10:13] | obs[13:16]
    hidden layer: act(W x + b), act = tanh (t = exp(-2 |x|), (1 - t) / (1 + t) with the sign of x) or relu;  output: W x + b
    rpm = rpm_base + rpm_scale * clip(y, -1, 1)          (a NaN y clips to -1, as m_clamp does)

Sums are NumPy's (not the header's fma chains): in float64 the two differ by rounding only."""
import numpy as np

from oracle import np_oracle as O

N_IN, N_OUT = 12, 4


def n_weights(n_hidden, width):
    return (N_IN + 1) * width + (n_hidden - 1) * (width + 1) * width + (width + 1) * N_OUT


def unpack(weights, n_hidden, width):
    """[(W [out, in], b [out])] of the packed vector (torch's order: weight row-major, then bias, layer after layer)"""
    w = np.asarray(weights, dtype=np.float64).reshape(-1)
    assert w.size == n_weights(n_hidden, width)
    dims = [N_IN] + [width] * n_hidden + [N_OUT]
    layers, at = [], 0
    for i, o in zip(dims[:-1], dims[1:]):
        layers.append((w[at:at + o * i].reshape(o, i), w[at + o * i:at + o * i + o]))
        at += o * i + o
    return layers


def pad(weights, n_hidden, width, W):
    """the same policy at width W >= width: zero rows, columns and biases for the new neurons"""
    dims = [N_IN] + [W] * n_hidden + [N_OUT]
    out = []
    for (A, b), i, o in zip(unpack(weights, n_hidden, width), dims[:-1], dims[1:]):
        A2, b2 = np.zeros((o, i)), np.zeros(o)
        A2[:A.shape[0], :A.shape[1]], b2[:b.size] = A, b
        out += [A2.reshape(-1), b2]
    return np.concatenate(out)


def m_tanh(x):
    with np.errstate(over="ignore", invalid="ignore"):
        t = np.exp(-2.0 * np.abs(x))
        return np.copysign((1.0 - t) / (1.0 + t), x)


def features(obs, target):
    """[n, 12] from observation rows [n, 20] and world-frame targets [n, 3]"""
    return np.concatenate([obs[:, 0:3] - target, obs[:, 7:10], obs[:, 10:13], obs[:, 13:16]], axis=-1)


def network(weights, n_hidden, width, activation, x):
    """y [n, 4] of features x [n, 12]"""
    layers = unpack(weights, n_hidden, width)
    with np.errstate(over="ignore", invalid="ignore"):
        for A, b in layers[:-1]:
            z = x @ A.T + b
            x = m_tanh(z) if activation == "tanh" else np.where(z > 0, z, 0.0)
        A, b = layers[-1]
        return x @ A.T + b


def rpm_of(y, rpm_base=None, rpm_scale=None):
    base = O.CF2P.HOVER_RPM if rpm_base is None else rpm_base
    scale = 0.05 * O.CF2P.HOVER_RPM if rpm_scale is None else rpm_scale
    with np.errstate(invalid="ignore"):
        c = np.where(y > -1.0, np.where(y < 1.0, y, 1.0), -1.0)          # NaN -> -1
    return base + scale * c


def policy_rpm(weights, n_hidden, width, activation, obs, target, rpm_base=None, rpm_scale=None):
    """(rpm [n, 4], y [n, 4]) of observation rows"""
    y = network(weights, n_hidden, width, activation, features(obs, target))
    return rpm_of(y, rpm_base, rpm_scale), y


class PolicyDriver:
    """An episode oracle stepped by the policy: step() acts on the oracle's current rows (post-reset where an env was just done) and
    returns the oracle's dict plus action [n, 4] (the commanded RPM) and y [n, 4] (the network's output before the clamp)."""

    def __init__(self, ora, weights, n_hidden, width, activation="tanh", rpm_base=None, rpm_scale=None):
        self.ora, self.net = ora, (np.asarray(weights, dtype=np.float64), n_hidden, width, activation)
        self.rpm_base, self.rpm_scale = rpm_base, rpm_scale

    def act(self, obs):
        return policy_rpm(*self.net, obs, self.ora.target, self.rpm_base, self.rpm_scale)

    def step(self):
        action, y = self.act(self.ora.av.obs())
        r = self.ora.step(action)
        r["action"], r["y"] = action, y
        return r

"""The open-loop case set of the DSLPID operator tests (tests/test_dslpid_cpu.py, tests/test_gpu_dslpid.py): K controller calls on n
drones whose observations and targets are prescribed, not flown, so that every clamp of ``dslpid_control`` (csrc/mds_math.hpp) is
reached and left again and every call's RPM row can be compared with the float64 oracle (oracle/np_oracle.py, ``DSLPIDOracle``).

Every value is rounded to float32 before anyone uses it: a float32 handle and the oracle see identical inputs.  The observation's
rpy columns are filled (the kernel reads the quaternion only).  Drone i belongs to group i % 8; every drone starts from a benign
base (|pos_e| <= 0.02, roll and pitch within 0.02, yaw within 0.02 of the target yaw, attitude drift <= 0.03 rad/s, |v| <= 0.05)
and each group changes one thing:

  0  nothing: every output strictly inside all clamps (after the first call's rate spike, which upstream has too)
  1  pos_e x = +-2.5 / (10 dt), y = -+ the same, reversed at call K/2: the xy integral reaches +-2 near call 8, stays, leaves
  2  z error +-(0.05..0.15) for 60 % of the group, +-(0.5..2.0) for the rest: z integral +-0.15 with unsaturated PWM; MAX_PWM
  3  z error -(0.3..20): thrust vector points down, scalar < 0, MIN_PWM
  4  roll +-(0.05..1.2), pitch -+(0.05..0.9), no drift: sustained attitude error, torque +-3200, roll/pitch integral +-1
  5  yaw and target yaw start at +-(pi - 0.05), yaw drifts through +-pi near call 6: the rates_e spike of the wrap, yaw torque clamp
  6  target yaw + 2 pi k, |k| in 3..16: reduced_phase of the target yaw
  7  roll +-(2.0..3.0): nearly inverted

Conditioning (no case is left out of any comparison; a draw that breaks one of these is redrawn, at most MAX_REDRAWS times, and
``make_cases`` asserts that none is left): commanded thrust vector >= 0.05 N, |z_ax x x_c| >= 0.1, Euler yaw of every observed
quaternion at least 1e-3 from +-pi, |pitch| <= 1.4.

``ProbeOracle`` is ``DSLPIDOracle`` restated with switches: clamps that can be dropped (the mutation checks), the float32 storage
model behind the float32 gates, and counters of which clamp acted.  With every switch off it returns DSLPIDOracle's bits
(test_probe_oracle_is_the_oracle)."""
import numpy as np

from oracle import np_oracle as O

N_DRONES, N_CALLS, N_GROUPS = 333, 24, 8
RATES = (240, 10)
MAX_REDRAWS = 8
EPS32 = 2.0 ** -24
MIN_THRUST_NORM, MIN_CROSS, MIN_YAW_MARGIN, MAX_PITCH = 0.05, 0.1, 1e-3, 1.4

_HALF = dict(P_FOR=0.5 * np.array([.4, .4, 1.25]), I_FOR=0.5 * np.array([.05, .05, .05]), D_FOR=0.5 * np.array([.2, .2, .5]))
GAINS = {
    # PIDEnv.py:128-133: every default halved
    "halved": dict(_HALF, P_TOR=0.5 * np.array([70000., 70000., 60000.]), I_TOR=0.5 * np.array([.0, .0, 500.]),
                   D_TOR=0.5 * np.array([20000., 20000., 12000.])),
    # keeps the torque inside +-3200 at large attitude errors, so the attitude integral shows in the output
    "probe": dict(_HALF, P_TOR=np.array([300., 300., 300.]), I_TOR=np.array([1500., 1500., 500.]), D_TOR=np.array([50., 50., 50.])),
    # three distinct, non-zero entries in every vector, each within +-40 % of "halved" (its two zero I_TOR entries: around 250): in the other
    # two sets the x entry equals the y entry everywhere, so a kernel that swapped them computes the same numbers
    "skew": dict(P_FOR=np.array([.16, .26, .55]), I_FOR=np.array([.02, .032, .027]), D_FOR=np.array([.08, .13, .22]),
                 P_TOR=np.array([28000., 44000., 34000.]), I_TOR=np.array([250., 325., 190.]), D_TOR=np.array([8000., 13000., 7000.])),
}


def mirrored(gains):
    """A gain set with the x and y entries of all six vectors swapped."""
    return {k: np.array([v[1], v[0], v[2]]) for k, v in gains.items()}


CLAMPS = ("xy2", "z015", "rp1", "tq3200", "min_pwm", "max_pwm")


def f32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def wrap(a):
    return a - 2 * np.pi * np.round(a / (2 * np.pi))


def _draw(i, attempt, K, dt, seed):
    """One drone's K calls -> (pos_e [K,3], rpy [K,3], vel [K,3], target_pos0 [3], target_yaw)."""
    rng = np.random.default_rng([seed, i, attempt])
    g = i % N_GROUPS
    t = np.arange(K) * dt
    k = np.arange(K)
    sgn = lambda: rng.choice([-1.0, 1.0])
    wob = lambda lo, hi, m: rng.uniform(lo, hi, m) * np.sin(rng.uniform(0.5, 1.5, m) * t[:, None] + rng.uniform(0, 2 * np.pi, m))   # [K,m]
    pos_e = wob(0.003, 0.02 / np.sqrt(3), 3)
    vel = wob(0.01, 0.05 / np.sqrt(3), 3)
    rp = wob(0.005, 0.018, 2)                                     # |rate| <= 0.018 * 1.5 = 0.027 rad/s
    tyaw = rng.uniform(-2.5, 2.5)
    dyaw = wob(0.005, 0.018, 1)[:, 0]
    tp0 = np.concatenate([rng.uniform(-1, 1, 2), rng.uniform(0.5, 1.5, 1)])
    if g == 1:
        s = sgn() * np.where(k < K // 2, 1.0, -1.0)
        big = 2.5 / (10 * dt)
        pos_e[:, 0] += s * big
        pos_e[:, 1] -= s * big
    elif g == 2:
        small = (i // N_GROUPS) % 5 < 3                            # 60 % of the group
        pos_e[:, 2] += sgn() * (rng.uniform(0.05, 0.15) if small else rng.uniform(0.5, 2.0))
    elif g == 3:
        pos_e[:, 2] -= np.exp(rng.uniform(np.log(0.3), np.log(20.0)))
    elif g == 4:
        s = sgn()
        rp = np.broadcast_to([s * rng.uniform(0.05, 1.2), -s * rng.uniform(0.05, 0.9)], (K, 2)).copy()
        dyaw = np.zeros(K)
    elif g == 5:
        s = sgn()
        tyaw = s * (np.pi - 0.05)
        dyaw = s * (0.05 / rng.uniform(5.3, 5.7)) * k             # passes +-pi between calls 5 and 6
    elif g == 6:
        tyaw += 2 * np.pi * sgn() * rng.integers(3, 17)
    elif g == 7:
        rp[:, 0] += sgn() * rng.uniform(2.0, 3.0)
    tyaw = float(f32(tyaw))
    yaw = wrap(wrap(tyaw) + dyaw)
    return pos_e, np.concatenate([rp, yaw[:, None]], axis=1), vel, tp0, tyaw


def _assemble(draws):
    pe, rpy, vel, tp0, tyaw = (np.stack(x, axis=-2 if np.ndim(x[0]) == 2 else 0) for x in zip(*draws))   # [K,n,3] x3, [n,3], [n]
    K, n = pe.shape[0], pe.shape[1]
    obs = np.zeros((K, n, 20))
    obs[..., 0:3] = f32(tp0[None] + 0.01 * np.sin(0.7 * np.arange(K))[:, None, None])               # the drone moves a little
    target_pos = f32(obs[..., 0:3] + pe)
    obs[..., 3:7] = O.quat_from_euler_bullet(rpy)
    obs[..., 7:10] = rpy
    obs[..., 10:13] = vel
    obs[..., 16:20] = O.CF2P.HOVER_RPM
    target_rpy = np.zeros((n, 3))
    target_rpy[:, 2] = tyaw
    return f32(obs), target_pos, f32(target_rpy)


class ProbeOracle:
    """DSLPIDOracle.compute_from_state with switches.  drop: names of CLAMPS to leave out, or "scalar0" (max(0, .)).  storage32: the float32 storage model (Euler angles and the three memory arrays
    rounded to float32; the caller passes a float32 dt).  hits: per call, which clamp acted and on which side."""

    def __init__(self, n, consts, gains, drop=(), storage32=False):
        self.c, self.g, self.drop, self.storage32 = consts, gains, frozenset(drop), storage32
        self.last_rpy, self.integral_pos_e, self.integral_rpy_e = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros((n, 3))
        self.hits = []
        self.aux = []

    def _clip(self, name, a, lo, hi):
        return a if name in self.drop else np.clip(a, lo, hi)

    def compute_from_state(self, dt, obs, target_pos, target_rpy):
        from scipy.spatial.transform import Rotation
        g, D = self.g, O.DSLPIDOracle
        if self.storage32:
            self.last_rpy, self.integral_pos_e, self.integral_rpy_e = f32(self.last_rpy), f32(self.integral_pos_e), f32(self.integral_rpy_e)
        obs = np.asarray(obs, dtype=np.float64)
        pos, quat, vel = obs[..., 0:3], obs[..., 3:7], obs[..., 10:13]
        target_pos, target_rpy = np.asarray(target_pos, dtype=np.float64), np.asarray(target_rpy, dtype=np.float64)
        R = O.quat_to_rotmat_bullet(quat)
        pos_e = target_pos - pos
        raw_pos = self.integral_pos_e + pos_e * dt
        ip = raw_pos.copy()
        ip[..., 0:2] = self._clip("xy2", ip[..., 0:2], -2., 2.)
        z2 = np.clip(ip[..., 2], -2., 2.)
        ip[..., 2] = self._clip("z015", z2, -0.15, .15)
        self.integral_pos_e = ip
        tt = g["P_FOR"] * pos_e + g["I_FOR"] * self.integral_pos_e + g["D_FOR"] * (-vel) + np.array([0, 0, self.c.GRAVITY])
        dot = np.sum(tt * R[..., :, 2], axis=-1)
        scalar = dot if "scalar0" in self.drop else np.maximum(0., dot)
        thrust = (np.sqrt(scalar / (4 * self.c.KF)) - D.CONST) / D.SCALE
        z_ax = tt / O.norm(tt)[..., None]
        x_c = np.stack([np.cos(target_rpy[..., 2]), np.sin(target_rpy[..., 2]), np.zeros_like(target_rpy[..., 2])], axis=-1)
        yc = O.cross(z_ax, x_c)
        y_ax = yc / O.norm(yc)[..., None]
        x_ax = O.cross(y_ax, z_ax)
        Rt = np.stack([x_ax, y_ax, z_ax], axis=-1)
        target_euler = Rotation.from_matrix(Rt).as_euler("XYZ")
        cur_rpy = O.euler_from_quat_bullet(quat)
        if self.storage32:
            cur_rpy = f32(cur_rpy)
        Rt2 = Rotation.from_euler("XYZ", target_euler).as_matrix()
        E = np.einsum("...ji,...jk->...ik", Rt2, R) - np.einsum("...ji,...jk->...ik", R, Rt2)
        rot_e = np.stack([E[..., 2, 1], E[..., 0, 2], E[..., 1, 0]], axis=-1)
        rates_e = -(cur_rpy - self.last_rpy) / dt
        self.last_rpy = cur_rpy.copy()
        raw_rpy = np.clip(self.integral_rpy_e - rot_e * dt, -1500., 1500.)
        ir = raw_rpy.copy()
        ir[..., 0:2] = self._clip("rp1", ir[..., 0:2], -1., 1.)
        self.integral_rpy_e = ir
        raw_tq = -g["P_TOR"] * rot_e + g["D_TOR"] * rates_e + g["I_TOR"] * self.integral_rpy_e
        tq = self._clip("tq3200", raw_tq, -3200, 3200)
        raw_pwm = thrust[..., None] + np.einsum("ij,...j->...i", O.ThrustOmegaOracle.MIX[self.c.MODEL], tq)
        pwm = raw_pwm if "min_pwm" in self.drop else np.maximum(raw_pwm, D.MIN_PWM)
        pwm = pwm if "max_pwm" in self.drop else np.minimum(pwm, D.MAX_PWM)
        side = lambda a, b: np.stack([a < -b, a > b])                                  # [2 sides, n, ...]
        self.hits.append({"xy2": side(raw_pos[..., 0:2], 2.).any(axis=-1), "z015": side(z2, 0.15), "rp1": side(raw_rpy[..., 0:2], 1.).any(axis=-1),
                          "tq3200_x": side(raw_tq[..., 0], 3200.), "tq3200_y": side(raw_tq[..., 1], 3200.), "tq3200_z": side(raw_tq[..., 2], 3200.),
                          "min_pwm": (raw_pwm < D.MIN_PWM).any(axis=-1)[None], "max_pwm": (raw_pwm > D.MAX_PWM).any(axis=-1)[None],
                          "scalar0": (dot < 0)[None]})
        self.aux.append({"tt_norm": O.norm(tt), "cross": O.norm(yc), "rpy": cur_rpy,
                         "inside": (raw_pwm > D.MIN_PWM) & (raw_pwm < D.MAX_PWM)})
        return D.SCALE * pwm + D.CONST


def run(oracle, dt, obs, target_pos, target_rpy, calls=None):
    """rpm [K, n, 4] of the calls (all of them by default) on ``oracle`` (anything with compute_from_state)."""
    calls = range(obs.shape[0]) if calls is None else calls
    return np.stack([oracle.compute_from_state(dt, obs[k], target_pos[k], target_rpy) for k in calls])


def hit_counts(probe):
    """name -> drone-calls on which the clamp acted, per side ([lo, hi]; one entry for the one-sided ones)."""
    return {name: np.sum([h[name] for h in probe.hits], axis=(0, 2)) for name in probe.hits[0]}


def _bad_drones(obs, target_pos, target_rpy, dt):
    n = obs.shape[1]
    bad = np.zeros(n, dtype=bool)
    for gains in GAINS.values():
        p = ProbeOracle(n, O.CF2P, gains)
        run(p, dt, obs, target_pos, target_rpy)
        for a in p.aux:
            bad |= (a["tt_norm"] < MIN_THRUST_NORM) | (a["cross"] < MIN_CROSS) | (np.abs(a["rpy"][:, 1]) > MAX_PITCH)
            bad |= np.pi - np.abs(a["rpy"][:, 2]) < MIN_YAW_MARGIN
    return bad


_cache = {}


def make_cases(n=N_DRONES, K=N_CALLS, ctrl_freq=240, seed=0):
    """-> obs [K,n,20], target_pos [K,n,3], target_rpy [n,3], group [n] (all float32-representable float64; do not write to them)."""
    key = (n, K, ctrl_freq, seed)
    if key not in _cache:
        dt = 1.0 / ctrl_freq
        attempt = np.zeros(n, dtype=int)
        draws = [_draw(i, 0, K, dt, seed) for i in range(n)]
        for _ in range(MAX_REDRAWS + 1):
            obs, target_pos, target_rpy = _assemble(draws)
            bad = _bad_drones(obs, target_pos, target_rpy, dt)
            if not bad.any():
                break
            for i in np.flatnonzero(bad):
                attempt[i] += 1
                draws[i] = _draw(i, attempt[i], K, dt, seed)
        assert not bad.any(), f"ill-conditioned draws left after {MAX_REDRAWS} redraws: drones {np.flatnonzero(bad)}"
        for a in (obs, target_pos, target_rpy):
            a.setflags(write=False)
        _cache[key] = (obs, target_pos, target_rpy, np.arange(n) % N_GROUPS)
    return _cache[key]


def oracle_for(n, model, gains):
    """A DSLPIDOracle of the shipped class with the gain set written into it."""
    o = O.DSLPIDOracle(n, O.CF2P if model == "cf2p" else O.CF2X)
    for k, v in gains.items():
        setattr(o, k, np.array(v, dtype=np.float64))
    return o


def handle_dt(ctrl_freq, dtype):
    """The dt the kernel runs with: (T)(1.0 / ctrl_freq)."""
    return float(np.float32(1.0 / ctrl_freq)) if dtype == "float32" else 1.0 / ctrl_freq


_ref = {}


def reference(model, ctrl_freq, gains_name, dtype, n=N_DRONES, K=N_CALLS):
    """The float64 oracle's rpm [K,n,4] on the case set, computed once per configuration and shared (read-only)."""
    key = (model, ctrl_freq, gains_name, dtype, n, K)
    if key not in _ref:
        obs, tp, tr, _ = make_cases(n, K, ctrl_freq)
        r = run(oracle_for(n, model, GAINS[gains_name]), handle_dt(ctrl_freq, dtype), obs, tp, tr)
        r.setflags(write=False)
        _ref[key] = r
    return _ref[key]


_sens = {}


def storage_sensitivity(ctrl_freq, gains_name):
    """Largest relative RPM deviation of the float64 oracle under float32 storage (Euler angles, the three memory arrays, dt rounded to
    float32) from the plain oracle, over both mixers: what a correct float32 controller may differ by before any arithmetic rounding."""
    key = (ctrl_freq, gains_name)
    if key not in _sens:
        obs, tp, tr, _ = make_cases(ctrl_freq=ctrl_freq)
        worst = 0.0
        for consts in (O.CF2P, O.CF2X):
            plain = run(ProbeOracle(obs.shape[1], consts, GAINS[gains_name]), 1.0 / ctrl_freq, obs, tp, tr)
            stored = run(ProbeOracle(obs.shape[1], consts, GAINS[gains_name], storage32=True), float(np.float32(1.0 / ctrl_freq)), obs, tp, tr)
            worst = max(worst, float(np.abs(stored / plain - 1).max()))
        _sens[key] = worst
    return _sens[key]


def gate(ctrl_freq, gains_name, dtype):
    """Relative gate per RPM value: float64 1e-10 (the gate of test_dslpid_class_reference_signature); float32 4 x the measured
    storage sensitivity (the 4 covers the arithmetic roundings the model leaves out) + 8 x 2^-24 (a floor where it is tiny)."""
    return 1e-10 if dtype == "float64" else 4 * storage_sensitivity(ctrl_freq, gains_name) + 8 * EPS32

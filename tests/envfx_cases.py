"""Scenes and oracle runs for the ground-effect / downwash step kernels (k_step_env, k_step_ctrl_env: the only step kernels where a lane reads
another drone's row), defined once for tests/test_envfx_cpu.py and tests/test_gpu_envfx.py.  Everything here runs on the float64 oracle
alone (no GPU, no library).

  * ``stacked(E, D)``: envs of D drones stacked above each other over the floor, every env from its own seed, every centre on a 2^-10 m grid
    and every start position on a 2^-20 m grid (so that moving an env by 512 m or 256 m is exact in fp32 and in float64: ``displaced``).
  * ``step_loop`` / ``geo_loop``: the oracle under env.step (300 Hz physics / 100 Hz control, open-loop RPM) and under the fused geometric
    path (200 / 100 Hz, one Lemniscate per drone), cached by ``loop_run``; ``variant`` swaps the downwash for one a wrong kernel would compute:
    "cut" loses the env-mates that live in another wavefront, "stale" reads the env-mates' positions after the substep instead of before.
  * ``boundary_envs`` / ``sub_envs``: the envs whose drones lie in two wavefronts (or that start a workgroup), and the <= 63 drones flown
    again in a handle where nothing straddles.
  * ``pair_batch`` / ``tower_batch``: one-substep batches that reach every branch of downwash_pair and ground_effect, with the drones of
    each branch tagged; ``accelerations`` is the oracle's (v' - v) / dt and (w' - w) / dt for such a batch.
  * ``WIND`` / ``wind_runs``: a wind with three non-zero components, and the same with y and z swapped.
  * ``entry_run``: the closed loops of the other entry points on the 37 x 7 scene (12-state LQR, LQR-omega / LQR-yank-omega with their low
    levels, DSLPID with two target sets, Circles through the segment tables, CF2X, env.step with an action table and an episode reset)."""
import functools

import numpy as np

from oracle import np_oracle as O
from tests import aniso_cases as AC
from tests import helpers as H

WAVE, BLOCK = 64, 256                          # wavefront size, kBlock of csrc/mds_kernels.hip
MODES = {"PYB_GND": "dyn_gnd", "PYB_DW": "dyn_dw", "PYB_GND_DRAG_DW": "dyn_gnd_drag_dw"}
SHAPES = [(37, 7), (52, 5), (17, 16), (1, 1), (3, 1)]
BIG = SHAPES[:3]
STEPS = 15                                     # control steps of every loop scene
FACTOR = AC.FACTOR                             # a scene must move the oracle by FACTOR x the gate to count as telling two things apart
GATE_STEP = {"float64": 1e-10, "float32": 3e-5}    # x max(1, |x|): test_ground_effect_and_downwash_match_oracle
GATE_CTRL = {"float64": 1e-9, "float32": 3e-5}     # x max(1, |x|): test_ground_effect_and_downwash_in_the_controller_paths
SPACING = 0.5                                  # vertical distance between env-mates [m]
SHIFT = (512.0, 256.0)                         # part 4: every env's centre goes to (+-512, +-256) m
WIND = np.array([2.5e-4, -1.7e-4, 0.9e-4])     # N, world frame
WIND_SWAPPED = WIND[[0, 2, 1]]


def gate(kind, dtype, ref):
    """the sibling tests' gate: tol x max(1, max |state columns of the oracle's observation|)"""
    tol = (GATE_STEP if kind == "step" else GATE_CTRL)[dtype]
    return tol * max(1.0, float(np.abs(np.asarray(ref)[..., :16]).max()))


def state_err(got, ref):
    return AC.state_err(got, ref)


# ---- which envs lie across a boundary --------------------------------------------------------------------------------------------------------
def boundary_envs(E, D):
    """envs with drones in two wavefronts, and envs (other than env 0) whose first drone starts a workgroup"""
    out = []
    for e in range(E):
        lo, hi = e * D, e * D + D - 1
        if lo // WAVE != hi // WAVE or (lo > 0 and lo % BLOCK == 0):
            out.append(e)
    return out


def sub_envs(E, D):
    """the boundary envs plus the lowest-numbered others, as many envs as fit 63 drones (one wavefront, nothing straddles), in order"""
    b = boundary_envs(E, D)
    m = min(E, (WAVE - 1) // D)
    rest = [e for e in range(E) if e not in b]
    return sorted(b + rest[:max(0, m - len(b))])


def drones_of(envs, D):
    return np.concatenate([np.arange(e * D, e * D + D) for e in envs]) if len(envs) else np.zeros(0, dtype=int)


# ---- scenes -----------------------------------------------------------------------------------------------------------------------------------
def _grid(a, bits):
    return np.round(np.asarray(a) * 2.0 ** bits) / 2.0 ** bits


@functools.lru_cache(maxsize=None)
def _stacked(E, D, seed, spacing):
    cen, xyz, rpy = np.zeros((E, D, 3)), np.zeros((E, D, 3)), np.zeros((E, D, 3))
    ph = np.zeros((E, D, 4))
    for e in range(E):
        rng = np.random.default_rng([seed, e])                 # every env its own stream: no two envs alike
        cen[e, :, 0:2] = rng.uniform(-2, 2, size=(1, 2)) + rng.normal(size=(D, 2)) * 0.03
        cen[e, :, 2] = 0.06 + spacing * np.arange(D)
        cen[e] = _grid(cen[e], 10)
        xyz[e] = _grid(cen[e] + np.concatenate([rng.normal(size=(D, 2)) * 0.05, rng.uniform(0, 0.02, size=(D, 1))], axis=-1), 20)
        rpy[e] = rng.uniform(-0.2, 0.2, size=(D, 3))
        ph[e, :, 0] = rng.uniform(0, 2 * np.pi, size=D)
        ph[e, :, 1:] = rng.uniform(-1, 1, size=(D, 3))
    P = np.zeros((E, D, 7))
    P[..., 0], P[..., 1], P[..., 2:5], P[..., 5] = 0.25, 1.2, cen, 0.15
    P[..., 6] = 2 * np.pi * np.arange(D) / (D + 0.25)
    return dict(E=E, D=D, xyz=xyz, rpy=rpy, P=P, ph=ph, cen=cen)


def stacked(E, D, seed=9, spacing=SPACING):
    """dict(E, D, xyz, rpy [E,D,3], P [E,D,7] one small Lemniscate per drone around its column, ph [E,D,4] open-loop RPM phases,
    cen [E,D,3] the Lemniscate centres)"""
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in _stacked(E, D, seed, spacing).items()}


def take(scene, envs):
    """the scene of the listed envs only, in that order"""
    envs = list(envs)
    out = {k: (v[envs].copy() if isinstance(v, np.ndarray) else v) for k, v in scene.items()}
    out["E"] = len(envs)
    return out


def shifts(E):
    """[E, 3]: (+-512, +-256, 0), the four sign pairs in turn"""
    s = np.zeros((E, 3))
    s[:, 0] = SHIFT[0] * np.where(np.arange(E) % 2 == 0, 1.0, -1.0)
    s[:, 1] = SHIFT[1] * np.where((np.arange(E) // 2) % 2 == 0, 1.0, -1.0)
    return s


def displaced(scene):
    """the scene with every env moved by shifts(E) in x and y (exact: see the module docstring); z stays (ground effect needs the true height)"""
    out = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in scene.items()}
    s = shifts(scene["E"])[:, None, :]
    out["xyz"] = scene["xyz"] + s
    out["cen"] = scene["cen"] + s
    out["P"][..., 2:5] = out["cen"]
    assert np.array_equal(out["xyz"] - s, scene["xyz"]) and np.array_equal(out["cen"] - s, scene["cen"])
    return out


def open_loop_action(scene, k, consts=O.CF2P):
    return H.open_loop_rpm(k, 0.01, scene["ph"].reshape(-1, 4), hover=consts.HOVER_RPM)


# ---- downwash as a wrong kernel would compute it ----------------------------------------------------------------------------------------------
def downwash_general(me, other, D, c, mask=None):
    """O.downwash_force with the drone's own position taken from ``me`` [n,3] and its env-mates' from ``other`` [n,3]; ``mask`` [n,n] bool
    (True: drone i sees drone j) removes pairs.  downwash_general(p, p, D, c) == O.downwash_force(p, D, c)."""
    n = me.shape[0]
    a, b = me.reshape(n // D, D, 3), other.reshape(n // D, D, 3)
    dz = b[:, None, :, 2] - a[:, :, None, 2]                           # [E, i, j] = z_j - z_i
    dxy = np.linalg.norm(b[:, None, :, 0:2] - a[:, :, None, 0:2], axis=-1)
    act = (dz > 0) & (dxy < 10) & ~np.eye(D, dtype=bool)[None]
    if mask is not None:
        idx = np.arange(n).reshape(n // D, D)
        act &= mask[idx[:, :, None], idx[:, None, :]]
    dzs = np.where(act, dz, 1.0)
    alpha = c.DW_COEFF_1 * (c.PROP_RADIUS / (4 * dzs)) ** 2
    beta = c.DW_COEFF_2 * dzs + c.DW_COEFF_3
    with np.errstate(divide="ignore"):
        f = np.where(act, -alpha * np.exp(-0.5 * (dxy / beta) ** 2), 0.0)
    return f.sum(axis=2).reshape(n)


class VariantOracle(O.AviaryOracle):
    """AviaryOracle whose downwash is what a wrong kernel would compute.  "cut": a drone sees only the env-mates of its own wavefront
    (a kernel that lost the mates in the next wavefront / workgroup); "stale": the env-mates' positions are those AFTER the substep (a kernel
    that read the output side of the double buffer; the drone's own position is the one before, which it holds in registers)."""

    def __init__(self, *a, variant, **kw):
        self.variant = variant
        super().__init__(*a, **kw)

    def step(self, action):
        assert self.integrator == "euler" and self.physics in ("dyn_dw", "dyn_gnd_drag_dw")
        clipped = np.clip(np.asarray(action, dtype=np.float64).reshape(-1, 4), 0, self.c.MAX_RPM)
        n, D = self.pos.shape[0], self.drones_per_env
        for _ in range(self.PYB_STEPS_PER_CTRL):
            drag_rpm = self.last_clipped_action if self.physics == "dyn_gnd_drag_dw" else None
            kw = {"wind": self.wind} if self.wind is not None else {}
            if self.physics == "dyn_gnd_drag_dw":
                kw["extra_prop_force"] = O.ground_effect_forces(self.pos, self.quat, clipped, self.c)
            args = (self.pos, self.quat, self.vel, self.rates, clipped, self.PYB_TIMESTEP, self.c, drag_rpm)
            if self.variant == "cut":
                w = np.arange(n) // WAVE
                dw = downwash_general(self.pos, self.pos, D, self.c, mask=w[:, None] == w[None, :])
            else:
                after = O.dyn_step_euler(*args, extra_body_z=O.downwash_force(self.pos, D, self.c), **kw)[0]
                dw = downwash_general(self.pos, after, D, self.c)
            self.pos, self.quat, self.vel, self.rates, self.ang_v = O.dyn_step_euler(*args, extra_body_z=dw, **kw)
            self.last_clipped_action = clipped
        return self.obs()


def make_oracle(scene, name, pyb, ctrl, consts=O.CF2P, variant=None, wind=None):
    n = scene["E"] * scene["D"]
    a = (scene["xyz"].reshape(n, 3), scene["rpy"].reshape(n, 3), consts, pyb, ctrl)
    if variant is None:
        ora = O.AviaryOracle(*a, physics=name, drones_per_env=scene["D"])
    else:
        ora = VariantOracle(*a, physics=name, drones_per_env=scene["D"], variant=variant)
    ora.wind = None if wind is None else np.asarray(wind, dtype=np.float64)
    return ora


# ---- the two loops ----------------------------------------------------------------------------------------------------------------------------
def step_loop(scene, name, steps=STEPS, consts=O.CF2P, variant=None, wind=None, pyb=300):
    """env.step with open-loop RPM, pyb / 100 Hz -> dict(obs [steps, n, 20], rpm [steps, n, 4])"""
    ora = make_oracle(scene, name, pyb, 100, consts, variant, wind)
    obs, rpm = [], []
    for k in range(steps):
        a = open_loop_action(scene, k, consts)
        obs.append(ora.step(a))
        rpm.append(a)
    return dict(obs=np.array(obs), rpm=np.array(rpm))


def geo_step(ora, obs, P, t, consts=O.CF2P):
    pos, vel, acc, yaw, yd = O.lemniscate(t, P[:, 0], P[:, 1], P[:, 2:5], P[:, 5], P[:, 6])
    rpm = O.geometric_compute(obs, pos, vel, acc, yaw, yd, consts)
    return ora.step(rpm), rpm


def geo_loop(scene, name, steps=STEPS, consts=O.CF2P, variant=None, wind=None, pyb=200):
    """the fused geometric path: one env.step of zeros, then ``steps`` x (Lemniscate -> GeometricControl -> env.step), pyb / 100 Hz, t
    accumulated as the reference loop does -> dict(obs [steps, n, 20], rpm [steps, n, 4])"""
    n = scene["E"] * scene["D"]
    P = scene["P"].reshape(n, 7)
    ora = make_oracle(scene, name, pyb, 100, consts, variant, wind)
    o = ora.step(np.zeros((n, 4)))
    t, obs, rpm = 0.0, [], []
    for k in range(steps):
        o, a = geo_step(ora, o, P, t, consts)
        obs.append(o)
        rpm.append(a)
        t += 0.01
    return dict(obs=np.array(obs), rpm=np.array(rpm))


@functools.lru_cache(maxsize=None)
def loop_run(E, D, name, path, variant=None, model="cf2p", wind=None, shifted=False):
    """cached oracle run of the stacked (E, D) scene: path "step" | "geo"; wind: None or a 3-tuple; shifted: the displaced scene"""
    scene = stacked(E, D)
    if shifted:
        scene = displaced(scene)
    consts = O.CF2X if model == "cf2x" else O.CF2P
    f = step_loop if path == "step" else geo_loop
    out = f(scene, name, consts=consts, variant=variant, wind=None if wind is None else np.array(wind))
    for v in out.values():
        v.setflags(write=False)
    return out


def limit_fraction(run, consts=O.CF2P):
    """fraction of the (drone, step) pairs with a motor at the thrust floor or at MAX_RPM"""
    return float(AC.at_limit(run["rpm"], consts).mean())


# ---- one-substep batches that reach every branch of the two force laws -------------------------------------------------------------------------
F32 = np.float32
ULP_IN, ULP_OUT = float(np.nextafter(F32(10), F32(0))), float(np.nextafter(F32(10), F32(20)))
FAR_DZ = 40.0         # height difference of the pairs around the 10 m cut-off: at dz = 40 m the force law's width c_2 dz + c_3 is 6.3 m, so the
#                       force at 10 m is 28 % of its peak (at the stacking distances of the loop scenes it is exp(-5e4) = 0 on either side)
BETA_DZ, BETA_DXY = (0.6870, 0.6875, 0.6880), (0.05, 1e-3)
REPL = 4              # drones per branch


def _state(pos, rpy, rng, v=1.0, w=2.0):
    n = pos.shape[0]
    s = np.zeros((n, 13))
    s[:, 0:3] = pos
    s[:, 3:7] = O.quat_from_euler_bullet(rpy)
    s[:, 7:10] = rng.uniform(-v, v, size=(n, 3))
    s[:, 10:13] = rng.uniform(-w, w, size=(n, 3))
    return s


@functools.lru_cache(maxsize=None)
def pair_batch(model="cf2p"):
    """Envs of two drones (A below or beside, B its only env-mate), REPL envs per branch -> dict(D=2, state [n,13], rpm [n,4],
    tags {branch: drone indices}).  Flown under dyn_gnd_drag_dw: both laws act on every drone."""
    c = O.CF2X if model == "cf2x" else O.CF2P
    rng = np.random.default_rng(31)
    posA, posB, rpyA, tags = [], [], [], {}

    def add(tag, a, b, rpy=None, who="A"):
        i = len(posA)
        posA.append(a), posB.append(b), rpyA.append(rng.uniform(-0.3, 0.3, size=3) if rpy is None else np.asarray(rpy, dtype=float))
        tags.setdefault(tag, []).append(2 * i + (0 if who == "A" else 1))

    def beside(a, dxy, dz, az):
        return a + np.array([dxy * np.cos(az), dxy * np.sin(az), dz])

    for r in range(REPL):
        base = lambda: np.array([*rng.uniform(-1, 1, size=2), rng.uniform(0.8, 1.2)])
        az = rng.uniform(0, 2 * np.pi)
        # downwash: the 10 m lateral cut-off by 1 cm and by one fp32 ulp either side (the latter along x from x = 0: exact in fp32)
        a = base(); add("lat_in", a, beside(a, 9.99, FAR_DZ, az))
        a = base(); add("lat_out", a, beside(a, 10.01, FAR_DZ, az))
        a = np.array([0.0, 0.0, base()[2]]); add("ulp_in", a, a + np.array([ULP_IN, 0.0, FAR_DZ]))
        a = np.array([0.0, 0.0, base()[2]]); add("ulp_out", a, a + np.array([ULP_OUT, 0.0, FAR_DZ]))
        a = base(); add("equal_z", a, beside(a, 0.05, 0.0, az))
        a = base(); b = beside(a, 0.05, 0.3, az); add("mate_above", a, b); tags.setdefault("mate_below_only", []).append(tags["mate_above"][-1] + 1)
        for dz in BETA_DZ:                  # c_2 dz + c_3 passes through zero at dz = 0.6875
            for dxy in BETA_DXY:
                a = base(); add(f"beta_{dz}_{dxy}", a, beside(a, dxy, dz, az))
        # ground effect: propeller heights below / at / above GND_EFF_H_CLIP (B far beside and above: no downwash to speak of)
        lvl = lambda z: np.array([*rng.uniform(-1, 1, size=2), z])
        a = lvl(0.02); add("h_below", a, beside(a, 3.0, 0.5, az), rpy=[0.05, -0.04, 0.3])
        a = lvl(c.GND_EFF_H_CLIP); add("h_at", a, beside(a, 3.0, 0.5, az), rpy=[0.0, 0.0, 0.0])
        a = lvl(0.06); add("h_above", a, beside(a, 3.0, 0.5, az), rpy=[0.05, -0.04, 0.3])
        a = lvl(0.3); add("roll_lo", a, beside(a, 3.0, 0.5, az), rpy=[(np.pi / 2 - 1e-3) * (-1) ** r, 0.1, 0.2])
        a = lvl(0.3); add("roll_hi", a, beside(a, 3.0, 0.5, az), rpy=[(np.pi / 2 + 1e-3) * (-1) ** r, 0.1, 0.2])
        a = lvl(0.1); add("pitch_near_p", a, beside(a, 3.0, 0.5, az), rpy=[0.1, np.pi / 2 - 9e-4, 0.2])
        a = lvl(0.1); add("pitch_near_m", a, beside(a, 3.0, 0.5, az), rpy=[0.1, -(np.pi / 2 - 9e-4), 0.2])
        # (within 4.5e-3 of +-pi/2 Bullet's Euler angles take their gimbal arm and report pitch = +-pi/2 exactly: the ground effect is off
        #  there; 5e-3 away, sin(pitch) = 0.9999875 < 0.99999, it is still on)
        a = lvl(0.1); add("pitch_5mrad", a, beside(a, 3.0, 0.5, az), rpy=[0.1, (np.pi / 2 - 5e-3) * (-1) ** r, 0.2])
    m = len(posA)
    pos, rpy = np.zeros((2 * m, 3)), np.zeros((2 * m, 3))
    pos[0::2], pos[1::2], rpy[0::2] = posA, posB, rpyA
    rpy[1::2] = rng.uniform(-0.3, 0.3, size=(m, 3))
    state = _state(pos, rpy, rng)
    rpm = (c.HOVER_RPM * (1 + 0.1 * rng.uniform(-1, 1, size=(2 * m, 4)))).astype(np.float32).astype(np.float64)
    return dict(D=2, model=model, state=state, rpm=rpm, tags={k: np.array(v) for k, v in tags.items()})


@functools.lru_cache(maxsize=None)
def tower_batch(model="cf2p"):
    """REPL envs of sixteen drones stacked 0.3 m apart: the lowest has all fifteen mates above -> as pair_batch, D = 16"""
    c = O.CF2X if model == "cf2x" else O.CF2P
    rng = np.random.default_rng(37)
    D = 16
    pos = np.zeros((REPL, D, 3))
    pos[..., 0:2] = rng.uniform(-1, 1, size=(REPL, 1, 2)) + rng.normal(size=(REPL, D, 2)) * 0.05
    pos[..., 2] = 0.05 + 0.3 * np.arange(D) + rng.uniform(0, 0.02, size=(REPL, D))
    state = _state(pos.reshape(-1, 3), rng.uniform(-0.3, 0.3, size=(REPL * D, 3)), rng)
    rpm = (c.HOVER_RPM * (1 + 0.1 * rng.uniform(-1, 1, size=(REPL * D, 4)))).astype(np.float32).astype(np.float64)
    return dict(D=D, model=model, state=state, rpm=rpm, tags={"fifteen_above": np.arange(REPL) * D})


def accelerations(batch, state=None, name="dyn_gnd_drag_dw", freq=240):
    """the oracle's ((v' - v) / dt, (w' - w) / dt) [n,3] each for ONE physics substep of the batch from ``state`` (default: the batch's own)"""
    c = O.CF2X if batch["model"] == "cf2x" else O.CF2P
    s = np.asarray(batch["state"] if state is None else state, dtype=np.float64).reshape(-1, 13)
    ora = AC.oracle_from_state(s, c, freq, freq, name, drones_per_env=batch["D"])
    ora.step(batch["rpm"])
    return (ora.vel - s[:, 7:10]) * freq, (ora.rates - s[:, 10:13]) * freq


def pair_geometry(batch, state=None):
    """per drone of a batch: (dz, dxy) to its env-mates [n, D-1] each, from the oracle's arithmetic"""
    s = np.asarray(batch["state"] if state is None else state).reshape(-1, 13)
    D = batch["D"]
    p = s[:, 0:3].reshape(-1, D, 3)
    dz = p[:, None, :, 2] - p[:, :, None, 2]
    dxy = np.linalg.norm(p[:, None, :, 0:2] - p[:, :, None, 0:2], axis=-1)
    off = ~np.eye(D, dtype=bool)
    return dz[:, off].reshape(-1, D - 1), dxy[:, off].reshape(-1, D - 1)


def prop_heights(batch, state=None):
    """[n, 4] unclipped propeller heights, and [n, 3] rpy"""
    c = O.CF2X if batch["model"] == "cf2x" else O.CF2P
    s = np.asarray(batch["state"] if state is None else state).reshape(-1, 13)
    R = O.quat_to_rotmat_bullet(s[:, 3:7])
    off = c.prop_offsets()
    return s[:, 2:3] + R[:, 2, 0:1] * off[:, 0] + R[:, 2, 1:2] * off[:, 1], O.euler_from_quat_bullet(s[:, 3:7])


# ---- wind -------------------------------------------------------------------------------------------------------------------------------------
def wind_scene_dyn():
    """test_wind_force_matches_oracle's scene (8 envs x 2 drones on Lemniscates, plain dyn, 100 / 100 Hz)"""
    xyz, rpy, P = H.c2_setup(8, 2, offset=1.0)
    return dict(E=8, D=2, xyz=xyz, rpy=rpy, P=P, cen=P[..., 2:5].copy(), ph=np.zeros((8, 2, 4)))


WIND_STEPS = 20


@functools.lru_cache(maxsize=None)
def wind_runs(which, swapped=False):
    """"dyn": plain dyn through the geometric path, 100 / 100 Hz, 20 steps; "envfx": dyn_gnd_drag_dw through env.step, 300 / 100 Hz, the
    stacked (7, 5) scene -> the oracle's run under WIND (or WIND_SWAPPED)"""
    w = WIND_SWAPPED if swapped else WIND
    if which == "dyn":
        return geo_loop(wind_scene_dyn(), "dyn", steps=WIND_STEPS, wind=w, pyb=100)
    return step_loop(stacked(7, 5), "dyn_gnd_drag_dw", steps=WIND_STEPS, wind=w)


# ---- the other entry points (part 2): closed loops on the 37 x 7 scene, 200 Hz physics / 100 Hz control unless said otherwise ----------------
ENTRY_SHAPE = (37, 7)
ENTRY_STEPS = 12
DSL_TARGETS = 2        # target sets of the DSLPID rollout
ROLL = dict(sets=3, slots=4, first_step=2, n_steps=7, episode_len=5)       # mds_rollout_step: steps j = 2 .. 8, one reset before j = 5


def circle_params(scene):
    """one Circle per drone through its start column: [n, 4] = (r, v, yaw_rate, 0) and centres [n, 3] (the drone starts near t = 0's point)"""
    n = scene["E"] * scene["D"]
    rng = np.random.default_rng(17)
    r = rng.uniform(0.15, 0.25, size=n)
    v = rng.uniform(0.2, 0.3, size=n)
    yr = rng.uniform(-0.2, 0.2, size=n)
    cen = scene["cen"].reshape(n, 3) - np.stack([r, np.zeros(n), np.zeros(n)], axis=1)
    return r, v, yr, cen


def circles(scene, cls):
    """the Circle objects of ``cls`` (oracle.np_trajectories.Circle or the library's CircleTrajectory), one per drone"""
    r, v, yr, cen = circle_params(scene)
    return [cls(r=float(r[i]), v=float(v[i]), center=cen[i].copy(), yaw_rate=float(yr[i])) for i in range(len(r))]


def dsl_targets(scene):
    """[DSL_TARGETS, E, D, 3] positions and [DSL_TARGETS, E, D, 3] rpy targets, fp32-representable"""
    E, D = scene["E"], scene["D"]
    rng = np.random.default_rng(23)
    tp = scene["xyz"][None] + np.array([0.0, 0.0, 0.2]) + rng.uniform(-0.05, 0.05, size=(DSL_TARGETS, E, D, 3))
    tr = np.zeros((DSL_TARGETS, E, D, 3))
    tr[..., 2] = rng.uniform(-0.5, 0.5, size=(DSL_TARGETS, E, D))
    f32 = lambda a: a.astype(np.float32).astype(np.float64)
    return f32(tp), f32(tr)


def ctrl_loop(scene, name, kind, steps=ENTRY_STEPS, consts=O.CF2P, pyb=200, first_step=0):
    """kind "lqr": 12-state LQRController; "omega" / "yank": LQR-omega + ThrustOmega / LQR-yank-omega + YankOmega low level (the RPM echo of
    the observation is the yank loop's input: the first env.step runs at hover RPM); "dslpid": DSLPID towards dsl_targets, set
    (first_step + k) % DSL_TARGETS at step k; "circle": GeometricControl on per-drone Circles -> dict(obs [steps, n, 20], rpm [steps, n, 4])"""
    from oracle import np_trajectories as NT
    n = scene["E"] * scene["D"]
    P = scene["P"].reshape(n, 7)
    ora = make_oracle(scene, name, pyb, 100, consts)
    dt = ora.CTRL_TIMESTEP
    o = ora.step(np.full((n, 4), consts.HOVER_RPM if kind in ("omega", "yank") else 0.0))
    if kind == "lqr":
        K = O.lqr12_gain(consts)
    elif kind == "omega":
        K, ll = O.lqr_omega_gain(consts), O.ThrustOmegaOracle(n, consts)
    elif kind == "yank":
        K, ll = O.lqr_yank_omega_gain(consts, dt), O.YankOmegaOracle(n, consts)
    elif kind == "dslpid":
        pid, (tp, tr) = O.DSLPIDOracle(n, consts, gain_scale=0.5), dsl_targets(scene)
    elif kind == "circle":
        trs = circles(scene, NT.Circle)
    t, obs, rpm = 0.0, [], []
    for k in range(steps):
        pos, vel, acc, yaw, yd = O.lemniscate(t, P[:, 0], P[:, 1], P[:, 2:5], P[:, 5], P[:, 6])
        if kind == "lqr":
            a, _ = O.lqr12_compute(o, pos, vel, yaw, yd, K, consts)
        elif kind == "omega":
            a = ll.compute_low_level(O.lqr_omega_compute(o, pos, vel, yaw, K, consts), o, dt)
        elif kind == "yank":
            a = ll.compute_low_level(O.lqr_yank_omega_compute(o, pos, vel, yaw, K, consts), o, dt)
        elif kind == "dslpid":
            w = (first_step + k) % DSL_TARGETS
            a = pid.compute_from_state(dt, o, tp[w].reshape(n, 3), tr[w].reshape(n, 3))
        else:
            des = np.array([np.hstack([np.asarray(x, dtype=np.float64) * np.ones(np.size(x)) for x in tr_(t)]) for tr_ in trs])
            a = O.geometric_compute(o, des[:, 0:3], des[:, 3:6], des[:, 6:9], des[:, 9], des[:, 10], consts)
        o = ora.step(a)
        obs.append(o)
        rpm.append(np.array(a, dtype=np.float64))
        t += dt
    return dict(obs=np.array(obs), rpm=np.array(rpm))


def circle_scene(scene):
    """the scene with every drone started 2 cm beside the first point of its Circle"""
    out = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in scene.items()}
    r, v, yr, cen = circle_params(scene)
    start = cen + np.stack([r, np.zeros_like(r), np.zeros_like(r)], axis=1)
    out["xyz"] = _grid(start.reshape(scene["xyz"].shape) + np.array([0.02, -0.015, 0.01]), 20)
    return out


@functools.lru_cache(maxsize=None)
def entry_run(kind, name="dyn_gnd_drag_dw"):
    """cached oracle run of an entry point's loop on the ENTRY_SHAPE scene: kind of ctrl_loop, "cf2x" (the geometric loop on the CF2X
    airframe), "rollout_step" (env.step with the action table, ring and reset of ROLL, 300 Hz physics: obs [n_steps, n, 20] in step order)"""
    scene = stacked(*ENTRY_SHAPE)
    if kind == "cf2x":
        return geo_loop(scene, name, steps=ENTRY_STEPS, consts=O.CF2X)
    if kind == "rollout_step":
        ora = make_oracle(scene, name, 300, 100)
        acts = roll_actions(scene)
        obs, rpm = [], []
        for j in range(ROLL["first_step"], ROLL["first_step"] + ROLL["n_steps"]):
            if j > 0 and j % ROLL["episode_len"] == 0:
                ora.reset()
            obs.append(ora.step(acts[j % ROLL["sets"]]))
            rpm.append(acts[j % ROLL["sets"]])
        return dict(obs=np.array(obs), rpm=np.array(rpm))
    if kind == "lqr":
        return ctrl_loop(lqr_scene(scene), name, kind, steps=LQR_STEPS)
    return ctrl_loop(circle_scene(scene) if kind == "circle" else scene, name, kind)


LQR_STEPS = 20


def lqr_scene(scene):
    """the scene with every drone started beside the first point of its Lemniscate, a quarter of the tilt: the 12-state LQR (1000 rad^-2
    attitude weights) saturates the motors for its first two steps whatever the start, and for many more from the columns' own starts"""
    out = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in scene.items()}
    P = scene["P"].reshape(-1, 7)
    pos = O.lemniscate(0.0, P[:, 0], P[:, 1], P[:, 2:5], P[:, 5], P[:, 6])[0].reshape(scene["xyz"].shape)
    out["xyz"] = _grid(pos + 0.2 * (scene["xyz"] - scene["cen"]), 20)
    out["rpy"] = 0.25 * scene["rpy"]
    return out


def roll_actions(scene):
    """[sets, n, 4] the action table of the mds_rollout_step case"""
    return np.array([open_loop_action(scene, 7 * a + 1) for a in range(ROLL["sets"])])


def cbf_scene():
    """the CBF loop's scene: 37 x 7 stacked drones, one sphere beside the columns of env 0"""
    scene = stacked(*ENTRY_SHAPE)
    c0 = scene["cen"][0, 0]
    return scene, [np.array([[c0[0] + 0.4, c0[1], 0.4], [0, 0, 0]])], [0.05]

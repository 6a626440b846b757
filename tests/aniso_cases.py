"""One x/y-asymmetric parameter set for the parity tests (tests/test_aniso_cpu.py, tests/test_gpu_aniso.py), defined once.

The stock constants are x/y symmetric (Jx == Jy, drag_x == drag_y, isotropic geometric gains, x entry == y entry in every DSLPID gain
vector, the hover Riccati gains with their fixed sparsity): the z component of w x Jw, (Jy - Jx) wx wy, is identically zero with them, and a
kernel that swapped index 0 and 1 of a constant, read a vector gain as a scalar or hoisted a gain through a rotation computes the same
numbers.  Set A below has three distinct entries in every 3-vector; every case built here excites the asymmetry, and says by how much:

  * ``mirrored(constants, gains)``: entries 0 and 1 of every 3-vector swapped;  ``isotropised(...)``: both replaced by their mean.
  * each case is a dict with ``run(constants, gains) -> array`` (the float64 oracle on the case's own seeded inputs), ``metric(got, ref)``
    (the comparison the GPU test makes), ``gate`` (dtype -> the gate of the stock sibling test) and ``clipped(ref) -> fraction`` of the
    (row, step) pairs with a motor at the 9440.3 RPM floor or at MAX_RPM.  ``discrimination(case)`` is the distance, in the case's metric,
    between the oracle with A and the oracle with the mirrored / isotropised set: tests require 100 x the largest gate.

Everything here runs on the oracle alone (no GPU, no library)."""
import functools
import os

import numpy as np

from oracle import np_oracle as O
from tests import helpers as H

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")

# ---- set A ---------------------------------------------------------------------------------------------------------------------------------
CONSTANTS = dict(M=0.031, L=0.0432, KF=2.9e-10, KM=8.6e-12, J=(2.1e-5, 2.9e-5, 3.6e-5), drag_coeff=(7.5e-7, 11.5e-7, 9.0e-7))   # CtrlAviary(constants=...)
GAINS = dict(Kp=(2.0, 2.6, 3.1), Kv=(3.1, 3.9, 4.4), KR=(105.0, 140.0, 90.0), Kw=(8.5, 11.5, 13.0))                                # set_geometric_gains(**GAINS)
DYN_J = (0.9, 1.3, 2.05)                       # case i: the Hummingbird inertia of model/dynamics.py with its x and y entries pulled apart
MIN_RPM = 9440.3                               # the mixer's thrust floor (utils/model_conversions.py:97)
FACTOR = 100                                   # the mirrored / isotropised set must move the oracle by FACTOR x the gate


def consts(constants=None, model="cf2p"):
    """The ``constants=`` dict as an oracle DroneConsts (G and thrust2weight stay stock unless the dict names them)."""
    c = dict(CONSTANTS if constants is None else constants)
    kw = dict(M=c["M"], L=c["L"], KF=c["KF"], KM=c["KM"], J=tuple(c["J"]), DRAG=tuple(c["drag_coeff"]), MODEL=model)
    if "G" in c:
        kw["G"] = c["G"]
    if "thrust2weight" in c:
        kw["THRUST2WEIGHT"] = c["thrust2weight"]
    return O.DroneConsts(**kw)


A, A_CF2X = consts(), consts(model="cf2x")


def _map3(d, f):
    return {k: (tuple(f(np.asarray(v, dtype=np.float64))) if np.ndim(v) == 1 and len(v) == 3 else v) for k, v in d.items()}


def mirrored(constants=CONSTANTS, gains=GAINS):
    """(constants, gains) with entries 0 and 1 of every 3-vector swapped."""
    f = lambda v: (float(v[1]), float(v[0]), float(v[2]))
    return _map3(constants, f), _map3(gains, f)


def isotropised(constants=CONSTANTS, gains=GAINS):
    """(constants, gains) with entries 0 and 1 of every 3-vector replaced by their mean."""
    f = lambda v: (float(0.5 * (v[0] + v[1])), float(0.5 * (v[0] + v[1])), float(v[2]))
    return _map3(constants, f), _map3(gains, f)


def at_limit(rpm, c):
    """[..] bool: a motor at the thrust floor or at MAX_RPM."""
    rpm = np.asarray(rpm)
    return (rpm <= MIN_RPM * (1 + 1e-9)).any(axis=-1) | (rpm >= c.MAX_RPM * (1 - 1e-9)).any(axis=-1)


# ---- seeded inputs -------------------------------------------------------------------------------------------------------------------------
def _nonzero(rng, size, lo, hi):
    """uniform in +-[lo, hi]: no component near zero"""
    return rng.choice([-1.0, 1.0], size=size) * rng.uniform(lo, hi, size=size)


def states(n, seed, att=0.4, w_max=3.0, v=1.5, z0=1.5):
    """World-frame 13-states [n, 13]: attitudes within +-att rad, body rates with all three components non-zero and |w| <= w_max, velocities
    non-zero in x, y and z, positions within a metre of (0, 0, z0)."""
    rng = np.random.default_rng(seed)
    s = np.zeros((n, 13))
    s[:, 0:3] = rng.uniform(-1, 1, size=(n, 3)) + np.array([0.0, 0.0, z0])
    s[:, 3:7] = O.quat_from_euler_bullet(rng.uniform(-att, att, size=(n, 3)))
    s[:, 7:10] = _nonzero(rng, (n, 3), 0.4 * v, v)
    s[:, 10:13] = _nonzero(rng, (n, 3), 0.3 * w_max / np.sqrt(3), w_max / np.sqrt(3))
    return s


def observations(n, seed, centre, att=0.4, w_max=3.0, pos_noise=0.15, vel_noise=0.5, hover=None):
    """Observation rows [n, 20] around ``centre`` [.., 3] with the attitudes / rates / velocities of ``states``; the RPM echo near hover."""
    rng = np.random.default_rng(seed)
    s = states(n, seed + 1000, att=att, w_max=w_max, v=vel_noise)
    s[:, 0:3] = np.asarray(centre) + rng.normal(size=(n, 3)) * pos_noise
    obs = exact_obs(s)
    obs[:, 16:20] = (A.HOVER_RPM if hover is None else hover) * (1 + 0.05 * rng.normal(size=(n, 4)))
    return obs


def exact_obs(state):
    """The observation [.., 20] of a state [.., 13] as the kernels pack it (rpy of q, ang_v = R w; no RPM echo)."""
    x = np.asarray(state, dtype=np.float64)
    q = x[..., 3:7]
    R = O.quat_to_rotmat_bullet(q)
    return np.concatenate([x[..., 0:3], q, O.euler_from_quat_bullet(q), x[..., 7:10], O.matvec(R, x[..., 10:13]), np.zeros(x.shape[:-1] + (4,))], axis=-1)


def oracle_from_state(state13, c, pyb, ctrl, physics="dyn", integrator="euler", drones_per_env=None):
    """An AviaryOracle standing at ``state13`` (what env.set_state does to a handle)."""
    s = np.asarray(state13, dtype=np.float64).reshape(-1, 13)
    ora = O.AviaryOracle(s[:, 0:3], np.zeros((s.shape[0], 3)), c, pyb, ctrl, physics, integrator, drones_per_env=drones_per_env)
    ora.pos, ora.quat, ora.vel, ora.rates = s[:, 0:3].copy(), s[:, 3:7].copy(), s[:, 7:10].copy(), s[:, 10:13].copy()
    ora.ang_v = O.matvec(O.quat_to_rotmat_bullet(ora.quat), ora.rates)
    return ora


def state_err(got, ref):
    """max |state part of the observation| (columns 0..15), the metric of test_gpu_parity.py"""
    return float(np.abs(np.asarray(got)[..., :16] - np.asarray(ref)[..., :16]).max())


def thrust_err(got, ref):
    """the project's thrust metric: max |rpm^2 - ref^2| / max ref^2"""
    got, ref = np.asarray(got), np.asarray(ref)
    return float(np.abs(got ** 2 - ref ** 2).max() / (ref ** 2).max())


def rel_err(got, ref):
    return float(np.abs(np.asarray(got) / np.asarray(ref) - 1).max())


def scaled_err(got, ref):
    """test_lqr*_golden's metric for the controller outputs: per column, relative to the column's largest reference value"""
    got, ref = np.asarray(got), np.asarray(ref)
    return float((np.abs(got - ref) / np.abs(ref).reshape(-1, ref.shape[-1]).max(axis=0)).max())


def rel1_err(got, ref):
    """test_gpu_compare_models' metric: |got - ref| / (1 + |ref|)"""
    return float((np.abs(np.asarray(got) - np.asarray(ref)) / (1 + np.abs(np.asarray(ref)))).max())


# ---- a: mds_step, open loop --------------------------------------------------------------------------------------------------------------
STEP_VARIANTS = {
    "dyn_euler": dict(physics="dyn", integrator="euler", pyb=240, ctrl=240, model="cf2p"),
    "dyn_rk4": dict(physics="dyn", integrator="rk4", pyb=240, ctrl=240, model="cf2p"),
    "drag_euler": dict(physics="dyn_drag", integrator="euler", pyb=240, ctrl=240, model="cf2p"),
    "drag_rk4": dict(physics="dyn_drag", integrator="rk4", pyb=240, ctrl=240, model="cf2p"),
    "dyn_240_48": dict(physics="dyn", integrator="euler", pyb=240, ctrl=48, model="cf2p"),
    "cf2x_drag": dict(physics="dyn_drag", integrator="euler", pyb=240, ctrl=240, model="cf2x"),
}
STEP_N, STEP_STEPS = 69, 12
# test_step_f64_matches_oracle_1000_steps (atol 1e-9), test_step_f32_open_loop (north_star's 1e-5 for both fp32 dtypes)
STEP_GATE = {"float64": 1e-9, "float32": 1e-5, "float32c": 1e-5}


def step_actions(variant, k, c):
    kw = STEP_VARIANTS[variant]
    ph = H.open_loop_setup(STEP_N, seed=3)[2]
    return H.open_loop_rpm(k, 1.0 / kw["ctrl"], ph, hover=c.HOVER_RPM)


def step_run(variant, constants=None, state13=None, steps=STEP_STEPS):
    """-> the observation [n, 20] after ``steps`` control steps from ``state13`` (default: states(69, 1))"""
    kw = STEP_VARIANTS[variant]
    c = consts(constants, kw["model"])
    ora = oracle_from_state(states(STEP_N, 1) if state13 is None else state13, c, kw["pyb"], kw["ctrl"], kw["physics"], kw["integrator"])
    for k in range(steps):
        obs = ora.step(step_actions(variant, k, consts(None, kw["model"])))      # the actions are inputs: set A's hover RPM whatever the constants
    return obs


def case_step(variant):
    return dict(name=f"a/step/{variant}", run=lambda cs, gn: step_run(variant, cs), metric=state_err, gate=STEP_GATE,
                clipped=lambda ref: float(np.mean([at_limit(step_actions(variant, k, consts(None, STEP_VARIANTS[variant]["model"])),
                                                             consts(None, STEP_VARIANTS[variant]["model"])).mean() for k in range(STEP_STEPS)])))


# ---- b: mds_rollout_step / mds_rollout_step_fused on an action table ----------------------------------------------------------------------
TABLE_N, TABLE_STEPS, TABLE_SETS, TABLE_SPL = 296, 11, 3, 5
TABLE_GATE = {"float64": 1e-9, "float32": 1e-5}


def table_actions():
    rng = np.random.default_rng(2)
    a = A.HOVER_RPM * (1 + 0.05 * rng.uniform(-1, 1, size=(TABLE_SETS, TABLE_N, 4)))
    return a.astype(np.float32).astype(np.float64)


def table_run(constants=None, state13=None):
    """-> the observations [11, n, 20] of the 11 steps (DYN_DRAG, 240 Hz)"""
    ora = oracle_from_state(states(TABLE_N, 4) if state13 is None else state13, consts(constants), 240, 240, "dyn_drag")
    acts = table_actions()
    return np.stack([ora.step(acts[k % TABLE_SETS]) for k in range(TABLE_STEPS)])


def case_table():
    return dict(name="b/rollout_step", run=lambda cs, gn: table_run(cs), metric=state_err, gate=TABLE_GATE,
                clipped=lambda ref: float(at_limit(table_actions(), A).mean()))


# ---- c: mds_geometric_compute on the rows of geometric_compute_aniso.npz -----------------------------------------------------------------
# test_geometric_compute_golden: relative RPM 1e-12 / 2e-6, aux 1e-12 / 4e-6 (w_des 5 x that)
GEO_GATE = {"float64": 1e-12, "float32": 2e-6}
GEO_AUX_GATE = {"float64": 1e-12, "float32": 4e-6}


@functools.lru_cache(maxsize=None)
def geo_fixture():
    d = np.load(os.path.join(GOLDEN, "geometric_compute_aniso.npz"))
    return {k: d[k] for k in d.files}


def geo_run(constants=None, gains=None, return_omegas=False):
    d = geo_fixture()
    des = d["des"]
    return O.geometric_compute(d["obs"], des[:, 0:3], des[:, 3:6], des[:, 6:9], des[:, 9], des[:, 10], consts(constants),
                               gains=dict(GAINS if gains is None else gains), return_omegas=return_omegas)


def case_geo():
    n_rand = int(geo_fixture()["n_rand"])
    return dict(name="c/geometric_compute", run=lambda cs, gn: geo_run(cs, gn), metric=rel_err, gate=GEO_GATE,
                clipped=lambda ref: float(at_limit(ref[:n_rand], A).mean()))       # family (a); (b) and (c) exist to clip


# ---- d: the fused geometric loop on Lemniscates -------------------------------------------------------------------------------------------
LOOP_E, LOOP_D, LOOP_STEPS = 3, 23, 40
# test_fused_geometric_1000_steps: float64 1e-9, float32 north_star's 1e-5 (and test_compensated_fp32_storage...: float32c 1e-5);
# RPM echo relative max(tol, 2e-6); action_out: test_fused_loop_against_the_reference_objects_in_the_loop's 1e-9 / 5e-6
LOOP_GATE = {"float64": 1e-9, "float32": 1e-5, "float32c": 1e-5}
LOOP_RPM_GATE = {"float64": 1e-9, "float32": 5e-6, "float32c": 5e-6}


def loop_setup(yaw_rate, E=LOOP_E, D=LOOP_D):
    xyz, _, P = H.c2_setup(E, D, seed=5, phase="c3", yaw_rate=yaw_rate)
    rpy = np.random.default_rng(6).uniform(-0.4, 0.4, size=(E, D, 3))
    return xyz, rpy, P


def loop_run(yaw_rate, constants=None, gains=None, steps=LOOP_STEPS, **kw):
    """-> the observations [steps + 1, n, 20]: after env.step(zeros) and after every control step"""
    xyz, rpy, P = loop_setup(yaw_rate)
    _, hist = H.oracle_closed_loop(xyz, rpy, P, steps, consts=consts(constants), gains=dict(GAINS if gains is None else gains), record_every=1, **kw)
    return np.stack(hist)


def case_loop(yaw_rate):
    return dict(name=f"d/step_geometric/yaw_rate_{yaw_rate}", run=lambda cs, gn: loop_run(yaw_rate, cs, gn), metric=state_err, gate=LOOP_GATE,
                clipped=lambda ref: float(at_limit(ref[1:, :, 16:20], A).mean()))


# ---- e: the same loop on segment tables ---------------------------------------------------------------------------------------------------
SEG_E, SEG_D, SEG_STEPS, SEG_T0, SEG_NAME = 2, 5, 30, 0.35, "compound3_mixed"      # t = 0.35 .. 0.65 crosses the Wait -> Lemniscate boundary at 0.5
SEG_GATE = {"float64": 1e-9, "float32": 1e-5}


def seg_setup():
    rng = np.random.default_rng(12)
    n = SEG_E * SEG_D
    s = states(n, 13, att=0.3, w_max=1.5, v=0.4, z0=0.5)
    s[:, 0:3] = np.array([0.0, 0.0, 0.5]) + rng.uniform(-0.15, 0.15, size=(n, 3))
    return s


def seg_run(constants=None, gains=None, state13=None):
    from tests import traj_cases as TC
    tr = TC.table_objects(TC.oracle_classes())[SEG_NAME]
    c = consts(constants)
    ora = oracle_from_state(seg_setup() if state13 is None else state13, c, 100, 100)
    obs = ora.obs()
    n = obs.shape[0]
    out, t = [], SEG_T0
    for _ in range(SEG_STEPS):
        pos, vel, acc, yaw, yd = (np.asarray(x, dtype=np.float64) for x in tr(float(t)))
        one = np.ones((n, 1))
        obs = ora.step(O.geometric_compute(obs, one * pos, one * vel, one * (acc * np.ones(3)), one[:, 0] * yaw, one[:, 0] * yd, c,
                                           gains=dict(GAINS if gains is None else gains)))
        out.append(obs)
        t += 0.01
    return np.stack(out)


def case_seg():
    return dict(name="e/step_geometric/segment_table", run=lambda cs, gn: seg_run(cs, gn), metric=state_err, gate=SEG_GATE,
                clipped=lambda ref: float(at_limit(ref[:, :, 16:20], A).mean()))


# ---- f: ground effect + drag + downwash -----------------------------------------------------------------------------------------------------
GND_E, GND_D, GND_STEPS = 2, 5, 20
# test_ground_effect_and_downwash_match_oracle / ..._in_the_controller_paths: tol x max(1, |state|max) with tol 1e-10 (step) / 1e-9 (controller), 3e-5
GND_GATE = {"float64": 1e-10, "float32": 3e-5}
GND_CTRL_GATE = {"float64": 1e-9, "float32": 3e-5}


def gnd_step_setup():
    """test_ground_effect_and_downwash_match_oracle's stacked scene, with body rates and velocities on top"""
    rng = np.random.default_rng(9)
    E, D = GND_E, GND_D
    xyz = np.zeros((E, D, 3))
    xyz[..., 0:2] = rng.normal(size=(E, D, 2)) * 0.05
    xyz[..., 2] = 0.03 + 0.35 * np.arange(D) + rng.uniform(0, 0.02, size=(E, D))
    rpy = rng.uniform(-0.3, 0.3, size=(E, D, 3))
    rpy[0, 1, 0] = 1.8                                                     # |roll| > pi/2: ground effect off there
    s = states(E * D, 14, w_max=3.0, v=0.3)
    s[:, 0:3] = xyz.reshape(-1, 3)
    s[:, 3:7] = O.quat_from_euler_bullet(rpy.reshape(-1, 3))
    s[:, 9] = np.abs(s[:, 9])                                              # nobody sinks through the floor in 0.2 s
    ph = rng.uniform(0, 2 * np.pi, size=(E * D, 4))
    ph[:, 1:] = rng.uniform(-1, 1, size=(E * D, 3))
    return s, ph


def gnd_step_run(constants=None, state13=None, physics="dyn_gnd_drag_dw"):
    s, ph = gnd_step_setup()
    ora = oracle_from_state(s if state13 is None else state13, consts(constants), 300, 100, physics, drones_per_env=GND_D)
    for k in range(GND_STEPS):
        obs = ora.step(H.open_loop_rpm(k, 0.01, ph, hover=A.HOVER_RPM))
    return obs


def gnd_loop_setup():
    """_stacked_near_ground of test_gpu_parity.py"""
    rng = np.random.default_rng(9)
    E, D = GND_E, GND_D
    cen = np.zeros((E, D, 3))
    cen[..., 0:2] = rng.uniform(-2, 2, size=(E, 1, 2)) + rng.normal(size=(E, D, 2)) * 0.03
    cen[..., 2] = 0.06 + 0.3 * np.arange(D)
    xyz = cen + np.concatenate([rng.normal(size=(E, D, 2)) * 0.05, rng.uniform(0, 0.02, size=(E, D, 1))], axis=-1)
    rpy = rng.uniform(-0.3, 0.3, size=(E, D, 3))
    P = np.zeros((E, D, 7))
    P[..., 0], P[..., 1], P[..., 2:5], P[..., 5] = 0.25, 1.2, cen, 0.15
    P[..., 6] = 2 * np.pi * np.arange(D) / (D + 0.25)
    return xyz, rpy, P


def gnd_loop_run(constants=None, gains=None, physics="dyn_gnd_drag_dw"):
    """-> observations [steps + 1, n, 20] of the geometric loop, 200 Hz physics / 100 Hz control"""
    xyz, rpy, P = gnd_loop_setup()
    c, gn = consts(constants), dict(GAINS if gains is None else gains)
    Pf = P.reshape(-1, 7)
    ora = O.AviaryOracle(xyz.reshape(-1, 3), rpy.reshape(-1, 3), c, 200, 100, physics=physics, drones_per_env=GND_D)
    obs = ora.step(np.zeros((Pf.shape[0], 4)))
    out, t = [obs], 0.0
    for _ in range(GND_STEPS):
        pos, vel, acc, yaw, yd = O.lemniscate(t, Pf[:, 0], Pf[:, 1], Pf[:, 2:5], Pf[:, 5], Pf[:, 6])
        obs = ora.step(O.geometric_compute(obs, pos, vel, acc, yaw, yd, c, gains=gn))
        out.append(obs)
        t += 0.01
    return np.stack(out)


def scaled_state_err(got, ref):
    """the ground-effect tests' metric: state error over max(1, largest state value)"""
    return state_err(got, ref) / max(1.0, float(np.abs(np.asarray(ref)[..., :16]).max()))


def case_gnd_step():
    return dict(name="f/step/gnd_drag_dw", run=lambda cs, gn: gnd_step_run(cs), metric=scaled_state_err, gate=GND_GATE, clipped=lambda ref: 0.0)


def case_gnd_loop():
    return dict(name="f/step_geometric/gnd_drag_dw", run=lambda cs, gn: gnd_loop_run(cs, gn), metric=scaled_state_err, gate=GND_CTRL_GATE,
                clipped=lambda ref: float(at_limit(ref[1:, :, 16:20], A).mean()))


# ---- g: the LQR family with dense gains --------------------------------------------------------------------------------------------------
LQR_N, LQR_STEPS = 69, 20
# test_lqr12_golden (u: 1e-9 / 3e-5 of the column's largest value; actions: 20 x that in the thrust metric), test_lqr_omega_golden (1e-10 / 2e-5),
# test_lqr_yank_omega_golden (1e-10 / 3e-5); closed loop: test_lqr_loop_against_the_reference_objects_in_the_loop's float64 1e-10
LQR_U_GATE = {"lqr12": {"float64": 1e-9, "float32": 3e-5}, "lqr_omega": {"float64": 1e-10, "float32": 2e-5},
              "lqr_yank_omega": {"float64": 1e-10, "float32": 3e-5}}
LQR_ACT_GATE = {"float64": 20 * 1e-9, "float32": 20 * 3e-5}
# float32, measured on an MI355X (max state error over the 20 steps, all of it in the body rates; every other component <= 4e-6): stock constants
# with their Riccati gain 6.8e-6 (inside north_star's 1e-5), constants A with their Riccati gain 1.6e-5, A with the dense gain 2.8e-5; float64
# 3.1e-14 in all three.  The oracle's own sensitivity to float32 storage of the state grows faster than that (7.3e-7 / 2.9e-6 / 6.5e-6): the excess
# over 1e-5 is rounding through the stiffer loop (smaller Jx, the noise on the rate columns), and the gate is 4 x the measured maximum.
LQR_LOOP_GATE = {"float64": 1e-10, "float32": 4 * 2.83e-5}


def riccati_gain(which, c=None):
    c = A if c is None else c
    return {"lqr12": lambda: O.lqr12_gain(c), "lqr_omega": lambda: O.lqr_omega_gain(c), "lqr_yank_omega": lambda: O.lqr_yank_omega_gain(c, 0.01)}[which]()


def dense_gain(which, c=None):
    """The project's Riccati gain for the model (4 x 12, 4 x 9, 4 x 10) plus seeded N(0, (0.05 max|K|)^2) on EVERY entry, the structural zeros
    included; max|K| is taken per row: row 0 is a force (or a yank) per unit error and rows 1..3 torques (or body rates), orders of magnitude
    apart, and noise of the thrust row's size on a torque row pins every motor at a limit (the saturation cap)."""
    K = np.array(riccati_gain(which, c), dtype=np.float64)
    rng = np.random.default_rng({"lqr12": 31, "lqr_omega": 32, "lqr_yank_omega": 33}[which])
    return K + rng.normal(size=K.shape) * 0.05 * np.abs(K).max(axis=1, keepdims=True)


def sparse_again(which, c=None):
    """The mirror of a dense gain: the dense gain with its structural-zero entries zeroed again."""
    K0 = np.array(riccati_gain(which, c), dtype=np.float64)
    return np.where(np.abs(K0) > 1e-9 * np.abs(K0).max(axis=1, keepdims=True), dense_gain(which, c), 0.0)


def lqr_rows(which, seed=41):
    """-> obs [69, 20], des [69, 11] (pos, vel, -, yaw, yaw rate): attitudes within 0.4 rad, body rates up to 3 rad/s, position noise 0.15 m,
    non-zero desired yaw -- all times 0.03 for the 12-state LQR, whose 1000 rad^-2 attitude weights pin a motor at a limit in every row at
    full size (with the Riccati gain too; tests/traj_cases.py LQR_STATES: tilt 0.01)."""
    k = 0.03 if which == "lqr12" else 1.0
    rng = np.random.default_rng(seed)
    cen = np.array([0.3, -0.2, 0.8])
    obs = observations(LQR_N, seed, cen, att=0.4 * k, w_max=3.0 * k, pos_noise=0.15 * k, vel_noise=0.5 * k)
    des = np.zeros((LQR_N, 11))
    des[:, 0:3] = cen + rng.normal(size=(LQR_N, 3)) * 0.1 * k
    des[:, 3:6] = _nonzero(rng, (LQR_N, 3), 0.1, 0.4) * k
    des[:, 9] = obs[:, 9] + _nonzero(rng, LQR_N, 0.05, 0.3) * k
    des[:, 10] = _nonzero(rng, LQR_N, 0.1, 0.5) * k
    return obs, des


def lqr_compute(which, K, c=None):
    """-> (u [69, 4], actions [69, 4] or None)"""
    c = A if c is None else c
    obs, des = lqr_rows(which)
    if which == "lqr12":
        act, u = O.lqr12_compute(obs, des[:, 0:3], des[:, 3:6], des[:, 9], des[:, 10], K, c)
        return u, act
    f = O.lqr_omega_compute if which == "lqr_omega" else O.lqr_yank_omega_compute
    return f(obs, des[:, 0:3], des[:, 3:6], des[:, 9], K, c), None


def case_lqr(which):
    return dict(name=f"g/{which}_compute", run=lambda cs, gn: lqr_compute(which, dense_gain(which))[0], mirror=lambda: lqr_compute(which, sparse_again(which))[0],
                metric=scaled_err, gate=LQR_U_GATE[which],
                clipped=lambda ref: float(at_limit(lqr_compute(which, dense_gain(which))[1], A).mean()) if which == "lqr12" else 0.0)


LQR_T0 = 1.0                                     # yaw = pi sin(0.2 t): 0.62 rad at the start of the loop


def lqr_loop_setup():
    """-> (P [1, 69, 7], state13 [69, 13]): slow Lemniscates (a 0.5 m, 0.4 rad/s, yaw rate 0.2) and drones standing on them at t = LQR_T0 to
    within tests/traj_cases.py's LQR_STATES sizes (2 cm, 3 cm/s, tilt 0.01, yaw 0.03, rates 0.05): from a standing start, or on a fast
    Lemniscate, the 12-state LQR pins the motors at their limits for the whole 0.2 s."""
    _, _, P = H.c2_setup(1, LQR_N, seed=7, offset=2.0, omega=0.4, yaw_rate=0.2)
    P[..., 0] = 0.5
    Pf = P.reshape(-1, 7)
    pos, vel, acc, yaw, yd = O.lemniscate(LQR_T0, Pf[:, 0], Pf[:, 1], Pf[:, 2:5], Pf[:, 5], Pf[:, 6])
    rng = np.random.default_rng(8)
    s = np.zeros((LQR_N, 13))
    s[:, 0:3] = pos + _nonzero(rng, (LQR_N, 3), 0.005, 0.02)
    rpy = np.concatenate([_nonzero(rng, (LQR_N, 2), 0.003, 0.01), (yaw + _nonzero(rng, LQR_N, 0.01, 0.03))[:, None]], axis=1)
    s[:, 3:7] = O.quat_from_euler_bullet(rpy)
    s[:, 7:10] = vel + _nonzero(rng, (LQR_N, 3), 0.01, 0.03)
    s[:, 10:13] = _nonzero(rng, (LQR_N, 3), 0.015, 0.05)
    s[:, 12] += yd
    return P, s


def lqr_loop_run(constants=None, K=None, state13=None, steps=LQR_STEPS):
    """-> observations [steps, n, 20]: trajectory -> 12-state LQR with the dense gain -> mixer -> DYN step (the 'lqr' loop of EnvGeometric.py)"""
    P, s = lqr_loop_setup()
    c = consts(constants)
    K = dense_gain("lqr12") if K is None else K
    Pf = P.reshape(-1, 7)
    ora = oracle_from_state(s if state13 is None else state13, c, 100, 100)
    obs = ora.obs()
    out, t = [], LQR_T0
    for _ in range(steps):
        pos, vel, acc, yaw, yd = O.lemniscate(t, Pf[:, 0], Pf[:, 1], Pf[:, 2:5], Pf[:, 5], Pf[:, 6])
        act, _ = O.lqr12_compute(obs, pos, vel, yaw, yd, K, c)
        obs = ora.step(act)
        out.append(obs)
        t += 0.01
    return np.stack(out)


def case_lqr_loop():
    return dict(name="g/step_lqr", run=lambda cs, gn: lqr_loop_run(cs), mirror=lambda: lqr_loop_run(None, sparse_again("lqr12")),
                metric=state_err, gate=LQR_LOOP_GATE, clipped=lambda ref: float(at_limit(ref[:, :, 16:20], A).mean()))


# ---- h: DSLPID with the "skew" gain set of tests/dslpid_cases.py (stock constants: upstream's DSLPID hard-codes them) ------------------------
PID_E, PID_D, PID_STEPS = 4, 3, 120
PID_GATE = {"float64": 1e-8, "float32": 2e-5}       # test_dslpid_fused_step_matches_oracle


def pid_setup():
    rng = np.random.default_rng(0)
    xyz = rng.uniform(-1, 1, size=(PID_E, PID_D, 3)) * np.array([1, 1, 0]) + np.array([0, 0, 0.3])
    tgt = xyz + np.array([0.4, -0.3, 0.6])            # errors of different size along x and y
    trpy = np.zeros((PID_E, PID_D, 3))
    trpy[..., 2] = _nonzero(rng, (PID_E, PID_D), 0.2, 1.0)
    return xyz, tgt, trpy


def pid_run(gains=None):
    """-> observations [steps, n, 20] of PIDEnv.sim_step's loop at 240 Hz, a target change half way"""
    from tests import dslpid_cases as DC
    xyz, tgt, trpy = pid_setup()
    n = PID_E * PID_D
    ora = O.AviaryOracle(xyz.reshape(-1, 3), np.zeros((n, 3)), O.CF2P, 240, 240)
    pid = DC.oracle_for(n, "cf2p", DC.GAINS["skew"] if gains is None else gains)
    obs = ora.step(np.zeros((n, 4)))
    out = []
    for k in range(PID_STEPS):
        if k == PID_STEPS // 2:
            tgt = tgt + np.array([0.4, -0.3, 0.2])
        obs = ora.step(pid.compute_from_state(ora.CTRL_TIMESTEP, obs, tgt.reshape(-1, 3), trpy.reshape(-1, 3)))
        out.append(obs)
    return np.stack(out)


def case_pid():
    from tests import dslpid_cases as DC
    sk = DC.GAINS["skew"]
    hi = O.DSLPIDOracle.SCALE * O.DSLPIDOracle.MAX_PWM + O.DSLPIDOracle.CONST
    return dict(name="h/step_dslpid", run=lambda cs, gn: pid_run(), mirror=lambda: pid_run(DC.mirrored(sk)),
                iso=lambda: pid_run({k: np.array([0.5 * (v[0] + v[1]), 0.5 * (v[0] + v[1]), v[2]]) for k, v in sk.items()}),
                metric=state_err, gate=PID_GATE,
                clipped=lambda ref: float(((ref[..., 16:20] <= MIN_RPM * (1 + 1e-9)) | (ref[..., 16:20] >= hi * (1 - 1e-9))).any(axis=-1).mean()))


# ---- i: mds_quadrotor_dynamics / mds_compare_models -----------------------------------------------------------------------------------------
DYN_N = 69
# test_quadrotor_dynamics_golden (1e-12, fp32 2e-5 abs + rel), test_compare_models_golden (1e-12 / 3e-5 in |d| / (1 + |ref|))
DYN_GATE = {"float64": 1e-12, "float32": 2e-5}
CMP_GATE = {"float64": 1e-12, "float32": 3e-5}


def dyn_rows():
    from scipy.spatial.transform import Rotation
    rng = np.random.default_rng(51)
    n = DYN_N
    x = np.zeros((n, 18))
    x[:, 0:3] = rng.normal(size=(n, 3))
    x[:, 3:12] = Rotation.from_euler("xyz", rng.uniform(-0.4, 0.4, size=(n, 3))).as_matrix().reshape(n, 9)
    x[:, 12:15] = _nonzero(rng, (n, 3), 0.3, 1.5)
    x[:, 15:18] = _nonzero(rng, (n, 3), 0.5, 1.7)
    u = np.zeros((n, 4))
    u[:, 0] = rng.uniform(20, 100, size=n)
    u[:, 1:] = rng.normal(size=(n, 3)) * 0.5
    return x, u


def dyn_run(J=DYN_J):
    x, u = dyn_rows()
    return O.quadrotor_dynamics(x, u, J=tuple(J))


def cmp_rows():
    obs = observations(DYN_N, 52, np.array([0.5, -0.4, 1.2]), att=0.4, w_max=3.0, pos_noise=0.5, vel_noise=1.0, hover=O.CF2P.HOVER_RPM)
    return obs


def cmp_run(J=DYN_J):
    """-> (xdot_lin, xdot_geo, x_lin) of O.compare_models with the stock CF2P env constants and the geometric model's inertia J"""
    A_, B_ = O.linearized_AB(O.CF2P)
    return O.compare_models(cmp_rows(), A_, B_, O.CF2P, dyn_J=tuple(J))


def _swap(J):
    return (J[1], J[0], J[2])


def _mean(J):
    return (0.5 * (J[0] + J[1]), 0.5 * (J[0] + J[1]), J[2])


def case_dyn():
    return dict(name="i/quadrotor_dynamics", run=lambda cs, gn: dyn_run(), mirror=lambda: dyn_run(_swap(DYN_J)), iso=lambda: dyn_run(_mean(DYN_J)),
                metric=rel1_err, gate=DYN_GATE, clipped=lambda ref: 0.0)


def case_cmp():
    return dict(name="i/compare_models", run=lambda cs, gn: cmp_run()[1], mirror=lambda: cmp_run(_swap(DYN_J))[1], iso=lambda: cmp_run(_mean(DYN_J))[1],
                metric=rel1_err, gate=CMP_GATE, clipped=lambda ref: 0.0)


# ---- j: the CBF loop with the geometric nominal -------------------------------------------------------------------------------------------
CBF_E, CBF_D, CBF_STEPS = 3, 4, 30
# smoke()'s persistent CBF rollout over 30 steps: 1e-5 (north_star); float64: test_c4_closed_loop_matches_oracle's 1e-11
CBF_GATE = {"float64": 1e-11, "float32": 1e-5}
CBF_POLES, CBF_RADIUS, CBF_ZSCALE = (-2.2, -2.4), 0.1, 1.0


def cbf_setup():
    xyz, rpy, P = H.c2_setup(CBF_E, CBF_D, phase="c3", offset=0.1)
    P[..., 4] = 0.5 + 0.15 * np.arange(CBF_D)             # trajectories 15 cm apart vertically: pair rows go active
    xyz[..., 2] = 0.5 + 0.3 * np.arange(CBF_D)
    rpy = np.random.default_rng(15).uniform(-0.2, 0.2, size=(CBF_E, CBF_D, 3))
    x_obs, obs_r = [np.array([[1.0, 0.0, 0.45], [0, 0, 0]])], [0.1]     # under drone 1's descent from 0.8 m to its trajectory at 0.65 m
    return xyz, rpy, P, x_obs, obs_r


def cbf_run(constants=None, gains=None, sphere=True, filter_log=None):
    """-> (obs [E, D, 20] after 30 steps, statuses [30, E])"""
    xyz, rpy, P, x_obs, obs_r = cbf_setup()
    c = consts(constants)
    K = O.place_poles_chain(list(CBF_POLES))
    umax = np.array([c.MAX_THRUST, 10.0, 10.0, 10.0])
    return H.oracle_cbf_closed_loop(xyz, rpy, P, CBF_STEPS, K, umax, CBF_RADIUS, CBF_ZSCALE, x_obs if sphere else None, obs_r if sphere else None,
                                    consts=c, gains=dict(GAINS if gains is None else gains), filter_log=filter_log)


def case_cbf():
    return dict(name="j/cbf_geometric", run=lambda cs, gn: cbf_run(cs, gn)[0], metric=state_err, gate=CBF_GATE,
                clipped=lambda ref: float(at_limit(ref[..., 16:20], A).mean()))


# ---- k: FedCE, 12-state ------------------------------------------------------------------------------------------------------------------------
FEDCE_E, FEDCE_D, FEDCE_STEPS = 2, 2, 20
FEDCE_GATE = {"float64": 1e-12}                    # test_one_identification_step_matches_oracle: theta and P to 1e-12 of their largest entry


def fedce_setup():
    rng = np.random.default_rng(17)
    n = FEDCE_E * FEDCE_D
    s = states(n, 18, att=0.3, w_max=1.5, v=0.5, z0=1.0)
    mg = A.M * A.G
    u = np.zeros((FEDCE_STEPS, n, 4))
    u[..., 0] = rng.normal(mg, 0.15 * mg, size=(FEDCE_STEPS, n))
    u[..., 1:] = rng.normal(size=(FEDCE_STEPS, n, 3)) * np.array([0.005 * A.MAX_XY_TORQUE, 0.005 * A.MAX_XY_TORQUE, 0.005 * A.MAX_Z_TORQUE])
    x_des = np.zeros((n, 12))
    x_des[:, 2] = rng.uniform(-0.3, 0.3, size=n)
    x_des[:, 9:12] = s[:, 0:3] + rng.normal(size=(n, 3)) * 0.1
    return s, u, x_des


def fedce_run(constants=None, state13=None):
    """One exploration phase of 20 steps (round-tripped inputs, an update every step) on tests/fedce_oracle's DLQR, per env
    -> (theta [E, 16 D, 12 D], P [E, D, 16, 16], last obs [n, 20])"""
    from tests import fedce_oracle as F
    c = consts(constants)
    s, u, x_des = fedce_setup()
    s = s if state13 is None else np.asarray(state13).reshape(-1, 13)
    D = FEDCE_D
    thetas, Ps, last = [], [], []
    for e in range(FEDCE_E):
        sl = slice(e * D, (e + 1) * D)
        ora = oracle_from_state(s[sl], c, 100, 100)
        ref = F.DLQR(D, c)
        obs = ora.obs()
        for t in range(FEDCE_STEPS):
            phis, acts = [], []
            for j in range(D):
                act = O.input_to_action(u[t, sl][j], c)
                uu = O.action_to_input(act, c)
                uu[0] -= c.M * c.G
                phis.append(np.hstack([F.error_state(F.lin_x(obs[j]), x_des[sl][j]), uu]))
                acts.append(act)
            obs = ora.step(np.array(acts))
            ref.approx_theta_update(phis, [F.error_state(F.lin_x(obs[j]), x_des[sl][j]) for j in range(D)], 0.01)
        thetas.append(ref.theta.copy())
        Ps.append(ref.P.copy())
        last.append(obs)
    return np.array(thetas), np.array(Ps), np.concatenate(last)


def max_rel(got, ref):
    """test_gpu_fedce.py's metric: largest difference over the largest reference entry"""
    return float(np.abs(np.asarray(got) - np.asarray(ref)).max() / np.abs(np.asarray(ref)).max())


def case_fedce():
    return dict(name="k/fedce_identify", run=lambda cs, gn: fedce_run(cs)[0], metric=max_rel, gate=FEDCE_GATE, clipped=lambda ref: 0.0)


# ---- the conditions of every case ---------------------------------------------------------------------------------------------------------
def all_cases():
    """Every GPU case of tests/test_gpu_aniso.py (case h's operator half, mds_dslpid_compute, runs in tests/test_gpu_dslpid.py on the case set
    of tests/dslpid_cases.py, where the "skew" gain set is defined)."""
    return ([case_step(v) for v in STEP_VARIANTS] + [case_table(), case_geo(), case_loop(0.0), case_loop(0.3), case_seg(), case_gnd_step(),
             case_gnd_loop()] + [case_lqr(w) for w in ("lqr12", "lqr_omega", "lqr_yank_omega")] + [case_lqr_loop(), case_pid(), case_dyn(), case_cmp(),
             case_cbf(), case_fedce()])


_disc = {}


def discrimination(case):
    """-> (reference with A, distance to the oracle with mirrored(A), distance to the oracle with isotropised(A)), computed once per case"""
    if case["name"] not in _disc:
        ref = case["run"](CONSTANTS, GAINS)
        mir = case["mirror"]() if "mirror" in case else case["run"](*mirrored())
        iso = (case["iso"]() if "iso" in case else None) if "mirror" in case else case["run"](*isotropised())
        _disc[case["name"]] = (ref, case["metric"](mir, ref), None if iso is None else case["metric"](iso, ref))
    return _disc[case["name"]]


def check_conditions(case):
    """The two conditions of a case, asserted on the oracle alone -> (mirror distance, isotropised distance or None, clipped fraction)."""
    ref, d_mir, d_iso = discrimination(case)
    need = FACTOR * max(case["gate"].values())
    assert d_mir >= need, f"{case['name']}: the mirrored set moves the oracle by {d_mir:.3e} < {FACTOR} x gate = {need:.3e}: the inputs do not excite the asymmetry"
    assert d_iso is None or d_iso >= need, f"{case['name']}: the isotropised set moves the oracle by {d_iso:.3e} < {need:.3e}"
    frac = case["clipped"](ref)
    assert frac <= 0.10, f"{case['name']}: {frac:.1%} of the (row, step) pairs have a motor at a limit (cap 10 %)"
    return d_mir, d_iso, frac

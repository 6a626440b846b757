"""GPU parity with x/y-ASYMMETRIC parameters: every kernel family against the float64 oracle with set A of tests/aniso_cases.py
(J = (2.1, 2.9, 3.6)e-5, drag (7.5, 11.5, 9.0)e-7, Kp / Kv / KR / Kw with three distinct entries each, dense LQR gains, the "skew" DSLPID
gains), on handles created with ``CtrlAviary(constants=...)``.

Every other GPU test runs with Jx == Jy, drag_x == drag_y, isotropic geometric gains and the sparse hover Riccati gains: the z component of
w x Jw, (Jy - Jx) wx wy, is identically zero there, and a kernel that swapped index 0 and 1 of J, invJ, drag, kp, kv, kR, kw or kR_half, read
a vector gain as a scalar or hoisted a gain through a rotation passes all of them.  Here each case prints three numbers: its error against
the oracle, its gate (the stock sibling test's, see tests/aniso_cases.py), and how far the oracle moves when x and y of the set are swapped
(``mirrored``) -- at least 100 x the gate, asserted again at the top of each test (tests/test_aniso_cpu.py asserts it, the isotropised
set and the 10 % motor-limit cap for every case on the CPU).  Ragged sizes on purpose: 69 drones, 296 = 4 x 64 + 40, 3 x 23.

Out of scope, deliberately: the fp16-storage kernels (the same arithmetic instantiated with T = float, judged through tests/fp16_oracle.py,
whose storage model would need its own parameter plumbing) and the order-3 CBF loop, the 9-state FedCE and its dLQR (their kernels read M and
G only, through the linear models).

Measured on an MI355X (largest error over the variants and launch forms of a case, in the case's metric; gate in brackets):

    case                                               float64             float32             float32c
    a  mds_step, 6 variants, 12 steps                  3.0e-15 (1e-9)      1.1e-6 (1e-5)       5.0e-7 (1e-5)
    b  rollout_step / rollout_step_fused, 11 steps     1.5e-15 (1e-9)      6.1e-7 (1e-5)
    c  geometric_compute, relative RPM                 1.7e-15 (1e-12)     5.7e-7 (2e-6)
       aux: force / w_des / R_des                      1.4e-15 (1e-12)     5.9e-7 (4e-6)
    d  step_geometric + 3 rollout forms, 40 steps      6.9e-15 (1e-9)      2.7e-6 (1e-5)       2.5e-6 (1e-5)
       RPM echo / action_out, relative                 1.0e-15 (1e-9)      3.9e-7 (5e-6)       3.9e-7 (5e-6)
    e  the same on a segment table, 30 steps           2.8e-15 (1e-9)      9.8e-7 (1e-5)
    f  GND_DRAG_DW under step / step_geometric         5.6e-16 (1e-10)     1.1e-6 (3e-5)
                                                       1.2e-14 (1e-9)      4.2e-7 (3e-5)
    g  lqr / lqr_omega / lqr_yank_omega, dense K       3.7e-16 (1e-10)     1.7e-6 (2e-5)
       step_lqr / rollout_lqr_fused, 20 steps          3.1e-14 (1e-10)     2.8e-5 (1.1e-4, see aniso_cases.LQR_LOOP_GATE)
    h  step_dslpid / rollout_dslpid, "skew", 120 steps 1.4e-14 (1e-8)      7.4e-6 (2e-5)
    i  quadrotor_dynamics / compare_models             8.0e-16 / 2.4e-14 (1e-12)   8.7e-7 (2e-5) / 7.5e-6 (3e-5)
    j  CBF loop, 3 forms, 30 steps (statuses equal)    1.5e-15 (1e-11)     1.2e-6 (1e-5)
    k  fedce_identify: theta / P                       7.9e-16 / 2.1e-15 (1e-12)

The mirrored set moves the oracle by 0.086 (case f) to 1.4 (case d) in the same metrics: four to fourteen orders above these errors.  No
kernel disagreed with the oracle.
"""
import numpy as np
import pytest

from oracle import np_oracle as O
from tests import aniso_cases as AC
from tests import dslpid_cases as DC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mds():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no HIP device: -m gpu tests need a real MI355X (there is no CPU fallback)")
    import types
    import multidronesim_amd
    multidronesim_amd.load_library()
    from multidronesim_amd.envs.CtrlAviary import CtrlAviary, DroneModel, Physics
    return types.SimpleNamespace(CtrlAviary=CtrlAviary, DroneModel=DroneModel, Physics=Physics, torch=torch)


PHYSICS = {"dyn": "DYN", "dyn_drag": "PYB_DRAG", "dyn_gnd_drag_dw": "PYB_GND_DRAG_DW"}


def make_env(mds, E, D, xyz, rpy, dtype, pyb=100, ctrl=100, physics="dyn", integrator="euler", model="cf2p", constants=AC.CONSTANTS, gains=AC.GAINS):
    env = mds.CtrlAviary(drone_model=mds.DroneModel(model), num_drones=D, initial_xyzs=xyz, initial_rpys=rpy, physics=getattr(mds.Physics, PHYSICS[physics]),
                         pyb_freq=pyb, ctrl_freq=ctrl, num_envs=E, dtype=dtype, integrator=integrator, constants=constants)
    if gains is not None:
        env.set_geometric_gains(**gains)
    return env


def host(t):
    return t.detach().double().cpu().numpy()


def report(name, dtype, err, gate, mirror):
    print(f"[aniso] {name:<44s} {dtype:<8s} error {err:.3e}   gate {gate:.1e}   mirrored-set distance {mirror:.3e}")


def conditions(case, dtype):
    """The discrimination condition again, cheaply (cached per case): -> (oracle reference with set A, gate, mirrored-set distance)."""
    ref, d_mir, d_iso = AC.discrimination(case)
    gate = case["gate"][dtype]
    assert d_mir >= AC.FACTOR * gate and (d_iso is None or d_iso >= AC.FACTOR * gate), (case["name"], d_mir, d_iso, gate)
    return ref, gate, d_mir


def test_constants_reach_the_handle_and_its_mirrors(mds):
    env = make_env(mds, 1, 2, np.zeros((2, 3)), np.zeros((2, 3)), "float64")
    a = AC.A
    for name in ("M", "L", "KF", "KM", "G", "MAX_RPM", "MAX_THRUST", "HOVER_RPM", "MAX_XY_TORQUE", "MAX_Z_TORQUE", "GRAVITY"):
        np.testing.assert_allclose(getattr(env, name), getattr(a, name), rtol=1e-14, err_msg=name)
    np.testing.assert_array_equal(np.diag(env.J), a.J)
    np.testing.assert_allclose(np.diag(env.J_INV), 1 / np.asarray(a.J), rtol=1e-15)
    np.testing.assert_array_equal(env.DRAG_COEFF, a.DRAG)
    env.close()
    with pytest.raises(ValueError):
        make_env(mds, 1, 1, np.zeros((1, 3)), np.zeros((1, 3)), "float64", constants={"Jx": 1.0})


# ---- a: mds_step, open loop ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float64", "float32", "float32c"])
@pytest.mark.parametrize("variant", list(AC.STEP_VARIANTS))
def test_step_open_loop(mds, variant, dtype):
    """12 control steps of k_step from states with body rates up to 3 rad/s and 1.5 m/s (set through set_state), 1 x 69 drones."""
    case = AC.case_step(variant)
    _, gate, d_mir = conditions(case, dtype)
    kw = AC.STEP_VARIANTS[variant]
    n = AC.STEP_N
    s = AC.states(n, 1)
    env = make_env(mds, 1, n, s[:, 0:3], np.zeros((n, 3)), dtype, kw["pyb"], kw["ctrl"], kw["physics"], kw["integrator"], kw["model"])
    env.set_state(s)
    s0 = env.get_state().reshape(n, 13)                      # as stored (float32 rounding; float32c: value + residual for the rates)
    c = AC.consts(None, kw["model"])
    for k in range(AC.STEP_STEPS):
        a = AC.step_actions(variant, k, c)
        gobs, *_ = env.step(mds.torch.as_tensor(a.reshape(1, n, 4), dtype=env.dtype))
    ref = AC.step_run(variant, state13=s0)
    got = host(gobs).reshape(n, 20)
    err = AC.state_err(got, ref)
    report(case["name"], dtype, err, gate, d_mir)
    assert err < gate
    np.testing.assert_allclose(got[:, 16:], ref[:, 16:], rtol=1e-7 if dtype != "float64" else 1e-14)
    st = env.get_state().reshape(n, 13)
    assert np.abs(st[:, 0:3] - ref[:, 0:3]).max() < gate and np.abs(st[:, 7:10] - ref[:, 10:13]).max() < gate
    env.close()


# ---- b: mds_rollout_step / mds_rollout_step_fused --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("fused", [False, True])
def test_rollout_step_on_an_action_table(mds, fused, dtype):
    """11 steps of a 3-set action table through mds_rollout_step and mds_rollout_step_fused (5 steps per launch: 5 + 5 + 1), DYN_DRAG at
    240 Hz, 1 x 296 drones, every step's observation against the oracle."""
    case = AC.case_table()
    _, gate, d_mir = conditions(case, dtype)
    torch = mds.torch
    n = AC.TABLE_N
    s = AC.states(n, 4)
    env = make_env(mds, 1, n, s[:, 0:3], np.zeros((n, 3)), dtype, 240, 240, "dyn_drag")
    env.set_state(s)
    s0 = env.get_state().reshape(n, 13)
    ref = AC.table_run(state13=s0)
    acts = torch.as_tensor(AC.table_actions().reshape(AC.TABLE_SETS, 1, n, 4), dtype=env.dtype).to(env.device).contiguous()
    log = torch.zeros((AC.TABLE_STEPS, 1, n, 20), dtype=env.dtype, device=env.device)
    env.rollout_step(acts, 0, AC.TABLE_STEPS, log, steps_per_launch=AC.TABLE_SPL if fused else 1)
    got = host(log).reshape(AC.TABLE_STEPS, n, 20)
    err = max(AC.state_err(got[j], ref[j]) for j in range(AC.TABLE_STEPS))
    np.testing.assert_allclose(got[..., 16:], ref[..., 16:], rtol=1e-7 if dtype != "float64" else 1e-14)
    report(case["name"] + ("_fused" if fused else ""), dtype, err, gate, d_mir)
    assert err < gate
    assert np.abs(env.get_state().reshape(n, 13)[:, 0:3] - ref[-1][:, 0:3]).max() < gate
    env.close()


# ---- c: mds_geometric_compute ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_geometric_compute(mds, dtype):
    """mds_geometric_compute incl. aux on the 128 rows of tests/golden/geometric_compute_aniso.npz (minted from the reference with set A)."""
    from multidronesim_amd.control.geometric import GeometricControl
    case = AC.case_geo()
    ref, gate, d_mir = conditions(case, dtype)
    d = AC.geo_fixture()
    n = d["obs"].shape[0]
    env = make_env(mds, n, 1, np.zeros((n, 1, 3)), np.zeros((n, 1, 3)), dtype, gains=None)
    ctrl = GeometricControl(env)
    np.testing.assert_array_equal(np.diag(ctrl.J), AC.A.J)
    ctrl.Kp, ctrl.Kv, ctrl.KR, ctrl.Kw = (np.array(AC.GAINS[k]) for k in ("Kp", "Kv", "KR", "Kw"))
    rpm, force, w_des, R_des = ctrl.compute_batched(d["obs"].reshape(n, 1, 20), d["des"].reshape(n, 1, 11), return_omegas=True)
    rpm = host(rpm).reshape(n, 4)
    f_ref, w_ref, R_ref = AC.geo_run(return_omegas=True)
    err = AC.rel_err(rpm, ref)
    aux = AC.GEO_AUX_GATE[dtype]
    e_f, e_w, e_R = np.abs(host(force).reshape(n) - f_ref).max(), np.abs(host(w_des).reshape(n, 3) - w_ref).max(), np.abs(host(R_des).reshape(n, 3, 3) - R_ref).max()
    report(case["name"], dtype, err, gate, d_mir)
    print(f"[aniso]     aux: force {e_f:.2e}, w_des {e_w:.2e} (gate {5 * aux:.0e}), R_des {e_R:.2e} (gate {aux:.0e}); against the reference-minted RPM {AC.rel_err(rpm, d['rpm']):.2e}")
    assert err < gate and e_f < aux and e_w < 5 * aux and e_R < aux
    rpm_only = host(ctrl.compute_batched(d["obs"].reshape(n, 1, 20), d["des"].reshape(n, 1, 11))).reshape(n, 4)
    np.testing.assert_array_equal(rpm_only, rpm)
    env.close()


# ---- d: the fused geometric loop on Lemniscates ------------------------------------------------------------------------------------------------
def _loop_env(mds, yaw_rate, dtype, specialise=True):
    xyz, rpy, P = AC.loop_setup(yaw_rate)
    env = make_env(mds, AC.LOOP_E, AC.LOOP_D, xyz, rpy, dtype)
    env.set_trajectories(P)
    if not specialise:
        env.set_traj_specialisation(False)
    assert env.traj_yaw_free() == (yaw_rate == 0.0)
    env.step(mds.torch.zeros((AC.LOOP_E, AC.LOOP_D, 4), dtype=env.dtype))       # EnvGeometric.py:431
    return env


@pytest.mark.parametrize("dtype", ["float64", "float32", "float32c"])
@pytest.mark.parametrize("yaw_rate,specialise", [(0.0, True), (0.0, False), (0.3, True)])
def test_fused_geometric_loop(mds, yaw_rate, specialise, dtype):
    """40 control steps on 3 x 23 drones through mds_step_geometric (with action_out), mds_rollout_geometric in both launch forms (one launch
    per step; the whole-rollout kernel, 7 steps per launch) and mds_rollout_geometric_fused with a log.  Yaw rate 0 runs the yaw-free
    kernels (traj_yaw_free() == 1), the same again with the specialisation switched off, yaw rate 0.3 the general ones."""
    case = AC.case_loop(yaw_rate)
    ref, gate, d_mir = conditions(case, dtype)
    E, D, T = AC.LOOP_E, AC.LOOP_D, AC.LOOP_STEPS
    n = E * D
    rgate = AC.LOOP_RPM_GATE[dtype]
    tag = f"{case['name']}{'' if specialise else '/general kernels'}"
    # one launch per step, the action wanted
    env = _loop_env(mds, yaw_rate, dtype, specialise)
    t, errs, e_act = 0.0, [], 0.0
    for k in range(T):
        gobs, act = env.step_geometric(t, return_action=True)
        t += env.CTRL_TIMESTEP
        if k in (0, T // 2, T - 1):
            errs.append(AC.state_err(host(gobs).reshape(n, 20), ref[k + 1]))
            e_act = max(e_act, AC.rel_err(host(act).reshape(n, 4), ref[k + 1][:, 16:]))
    e_rpm = AC.rel_err(host(gobs).reshape(n, 20)[:, 16:], ref[-1][:, 16:])
    report(tag + " step", dtype, max(errs), gate, d_mir)
    print(f"[aniso]     RPM echo {e_rpm:.2e} (gate {max(gate, 2e-6):.0e}), action_out {e_act:.2e} (gate {rgate:.0e})")
    assert max(errs) < gate and e_rpm < max(gate, 2e-6) and e_act < rgate
    env.close()
    # mds_rollout_geometric, both forms
    for form, spl in ((1, 0), (2, 7)):
        env = _loop_env(mds, yaw_rate, dtype, specialise)
        env.set_rollout_form(form, spl)
        o = env.rollout_geometric(0.0, T, obs_every_step=True)
        assert env.last_rollout_form() == form
        err = AC.state_err(host(o).reshape(n, 20), ref[-1])
        report(tag + f" rollout form {form}", dtype, err, gate, d_mir)
        assert err < gate and AC.rel_err(host(o).reshape(n, 20)[:, 16:], ref[-1][:, 16:]) < max(gate, 2e-6)
        st = env.get_state().reshape(n, 13)
        assert np.abs(st[:, 0:3] - ref[-1][:, 0:3]).max() < 10 * gate
        env.close()
    # one launch for the 40 steps, every step logged
    env = _loop_env(mds, yaw_rate, dtype, specialise)
    last, log = env.rollout_geometric_fused(0.0, T, log=True)
    lg = host(log).reshape(T, n, 20)
    err = max(AC.state_err(lg[k], ref[k + 1]) for k in range(T))
    report(tag + " rollout fused, log", dtype, err, gate, d_mir)
    assert err < gate and mds.torch.equal(last, log[-1])
    env.close()


# ---- e: the same loop on segment tables ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_fused_geometric_loop_on_segment_tables(mds, dtype):
    """30 control steps of the general (segment-table) kernels on 2 x 5 drones following tests/traj_cases.py's ``compound3_mixed``
    (Wait -> Lemniscate -> Circle) across its first piece boundary, through mds_step_geometric and mds_rollout_geometric_fused."""
    from tests import traj_cases as TC
    case = AC.case_seg()
    _, gate, d_mir = conditions(case, dtype)
    E, D, T = AC.SEG_E, AC.SEG_D, AC.SEG_STEPS
    n = E * D
    s = AC.seg_setup()
    tr = TC.table_objects(TC.library_classes())[AC.SEG_NAME]
    outs = {}
    for mode in ("step", "fused"):
        env = make_env(mds, E, D, s[:, 0:3].reshape(E, D, 3), np.zeros((E, D, 3)), dtype)
        env.set_trajectories([tr] * D)
        assert not env.traj_yaw_free()
        env.set_state(s)
        s0 = env.get_state().reshape(n, 13)
        if mode == "step":
            t, rows = AC.SEG_T0, []
            for k in range(T):
                rows.append(host(env.step_geometric(t)).reshape(n, 20).copy())
                t += env.CTRL_TIMESTEP
            got = np.stack(rows)
        else:
            _, log = env.rollout_geometric_fused(AC.SEG_T0, T, log=True)
            got = host(log).reshape(T, n, 20)
        ref = AC.seg_run(state13=s0)
        outs[mode] = max(AC.state_err(got[k], ref[k]) for k in range(T))
        report(case["name"] + " " + mode, dtype, outs[mode], gate, d_mir)
        assert AC.rel_err(got[-1][:, 16:], ref[-1][:, 16:]) < max(gate, 2e-6)
        env.close()
    assert max(outs.values()) < gate


# ---- f: ground effect + drag + downwash ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_ground_effect_drag_and_downwash_under_step(mds, dtype):
    """PYB_GND_DRAG_DW under env.step: 2 envs of 5 drones stacked over the floor (test_ground_effect_and_downwash_match_oracle's scene, one
    drone rolled past 90 degrees), three physics substeps per control step, 20 control steps."""
    case = AC.case_gnd_step()
    _, gate, d_mir = conditions(case, dtype)
    E, D = AC.GND_E, AC.GND_D
    s, ph = AC.gnd_step_setup()
    env = make_env(mds, E, D, s[:, 0:3].reshape(E, D, 3), np.zeros((E, D, 3)), dtype, 300, 100, "dyn_gnd_drag_dw")
    env.set_state(s)
    s0 = env.get_state().reshape(-1, 13)
    from tests import helpers as H
    for k in range(AC.GND_STEPS):
        a = H.open_loop_rpm(k, 0.01, ph, hover=AC.A.HOVER_RPM)
        gobs, *_ = env.step(mds.torch.as_tensor(a.reshape(E, D, 4), dtype=env.dtype))
    ref = AC.gnd_step_run(state13=s0)
    err = AC.scaled_state_err(host(gobs).reshape(-1, 20), ref)
    report(case["name"], dtype, err, gate, d_mir)
    assert err < gate
    plain = AC.gnd_step_run(state13=s0, physics="dyn")
    assert np.abs(plain[:, 2] - ref[:, 2]).max() > 1e-3                      # the effects are doing something in this scene
    env.close()


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_ground_effect_drag_and_downwash_under_step_geometric(mds, dtype):
    """PYB_GND_DRAG_DW under the fused controller path (200 Hz physics / 100 Hz control, _stacked_near_ground's scene), 20 control steps."""
    case = AC.case_gnd_loop()
    ref, gate, d_mir = conditions(case, dtype)
    E, D = AC.GND_E, AC.GND_D
    xyz, rpy, P = AC.gnd_loop_setup()
    env = make_env(mds, E, D, xyz, rpy, dtype, 200, 100, "dyn_gnd_drag_dw")
    env.set_trajectories(P)
    env.step(mds.torch.zeros((E, D, 4), dtype=env.dtype))
    t = 0.0
    for k in range(AC.GND_STEPS):
        gobs = env.step_geometric(t)
        t += 0.01
    g = host(gobs).reshape(-1, 20)
    err = AC.scaled_state_err(g, ref[-1])
    report(case["name"], dtype, err, gate, d_mir)
    assert err < gate
    np.testing.assert_allclose(g[:, 16:], ref[-1][:, 16:], rtol=1e-5 if dtype == "float32" else 1e-10)
    assert AC.state_err(AC.gnd_loop_run(physics="dyn")[-1], ref[-1]) > 1e-3
    env.close()


# ---- g: the LQR family with dense gains ----------------------------------------------------------------------------------------------------------
def _set_gain(env, which, K):
    from multidronesim_amd import _capi as capi
    fn = {"lqr12": env._lib.mds_set_lqr_gain, "lqr_omega": env._lib.mds_set_lqr_omega_gain, "lqr_yank_omega": env._lib.mds_set_lqr_yank_omega_gain}[which]
    capi.check(fn(env._h, capi.as_double_ptr(np.ascontiguousarray(K, dtype=np.float64))), "mds_set_*_gain")


def _lqr_controller(env, which):
    from multidronesim_amd.control import LQRController, LQROmegaController, LQRYankOmegaController, YankOmegaController
    from multidronesim_amd.model import LinearizedModel, LinearizedOmegaModel, LinearizedYankOmegaModel
    if which == "lqr12":
        return LQRController(env, LinearizedModel(env))
    if which == "lqr_omega":
        return LQROmegaController(env, LinearizedOmegaModel(env), None)
    return LQRYankOmegaController(env, LinearizedYankOmegaModel(env), YankOmegaController(env))


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("which", ["lqr12", "lqr_omega", "lqr_yank_omega"])
def test_lqr_operators_with_dense_gains(mds, which, dtype):
    """mds_lqr_compute / mds_lqr_omega_compute / mds_lqr_yank_omega_compute on 69 rows with a DENSE gain (the Riccati gain of the handle's
    constants A plus noise on every entry, the structural zeros included): a kernel that skips the zeros of the hover gain's fixed pattern
    is wrong here.  The mirror of this case is the dense gain with those entries zeroed again."""
    case = AC.case_lqr(which)
    ref, gate, d_mir = conditions(case, dtype)
    obs, des = AC.lqr_rows(which)
    n = AC.LQR_N
    env = make_env(mds, n, 1, np.zeros((n, 1, 3)), np.zeros((n, 1, 3)), dtype)
    ctrl = _lqr_controller(env, which)
    np.testing.assert_allclose(ctrl.K, AC.riccati_gain(which), rtol=1e-7, atol=1e-9)          # the host solver saw constants A
    K = AC.dense_gain(which)
    assert (np.abs(K) > 1e-6 * np.abs(K).max(axis=1, keepdims=True)).all()
    _set_gain(env, which, K)
    out = ctrl.compute_batched(obs.reshape(n, 1, 20), des.reshape(n, 1, 11))
    act, u = out if which == "lqr12" else (None, out)
    err = AC.scaled_err(host(u).reshape(n, 4), ref)
    report(case["name"], dtype, err, gate, d_mir)
    assert err < gate
    if which == "lqr12":
        a_ref = AC.lqr_compute(which, K)[1]
        e_act = AC.thrust_err(host(act).reshape(n, 4), a_ref)
        print(f"[aniso]     actions, thrust metric {e_act:.2e} (gate {AC.LQR_ACT_GATE[dtype]:.0e})")
        assert e_act < AC.LQR_ACT_GATE[dtype]
    env.close()


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_lqr_loop_with_a_dense_gain(mds, dtype):
    """mds_step_lqr and mds_rollout_lqr_fused over 20 control steps on 1 x 69 drones with constants A and the dense 4 x 12 gain, from states
    on slow yawing Lemniscates (the 12-state LQR saturates the motors from anything rougher).  Measured: float64 3.1e-14 (gate 1e-10); float32
    2.7e-5 (step) / 2.8e-5 (one launch), all of it in the body rates, against 6.8e-6 with the stock constants and their Riccati gain in the same
    case: rounding through a stiffer loop, gate 4 x the measured value (tests/aniso_cases.py, LQR_LOOP_GATE)."""
    case = AC.case_lqr_loop()
    _, gate, d_mir = conditions(case, dtype)
    n, T = AC.LQR_N, AC.LQR_STEPS
    P, s = AC.lqr_loop_setup()
    outs = {}
    for mode in ("step", "fused"):
        env = make_env(mds, 1, n, s[:, 0:3], np.zeros((n, 3)), dtype)
        env.set_trajectories(P)
        _lqr_controller(env, "lqr12")
        _set_gain(env, "lqr12", AC.dense_gain("lqr12"))
        env.set_state(s)
        s0 = env.get_state().reshape(n, 13)
        if mode == "step":
            t, rows = AC.LQR_T0, []
            for k in range(T):
                rows.append(host(env.step_lqr(t)).reshape(n, 20).copy())
                t += env.CTRL_TIMESTEP
            got = np.stack(rows)
        else:
            _, log = env.rollout_geometric_fused(AC.LQR_T0, T, log=True, controller="lqr")
            got = host(log).reshape(T, n, 20)
        ref = AC.lqr_loop_run(state13=s0)
        outs[mode] = max(AC.state_err(got[k], ref[k]) for k in range(T))
        report(case["name"] + " " + mode, dtype, outs[mode], gate, d_mir)
        env.close()
    assert max(outs.values()) < gate


# ---- h: DSLPID with the "skew" gains ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_dslpid_loop_with_skew_gains(mds, dtype):
    """mds_step_dslpid and mds_rollout_dslpid with the "skew" gain set (three distinct entries in all six vectors; stock constants: upstream's
    DSLPID hard-codes them), 4 x 3 drones at 240 Hz over 120 steps with a target change half way.  The operator alone, mds_dslpid_compute,
    runs with "skew" call by call in tests/test_gpu_dslpid.py."""
    from tests.test_gpu_dslpid import make_env as pid_env
    case = AC.case_pid()
    ref, gate, d_mir = conditions(case, dtype)
    E, D, T = AC.PID_E, AC.PID_D, AC.PID_STEPS
    xyz, tgt, trpy = AC.pid_setup()
    tgt2 = tgt + np.array([0.4, -0.3, 0.2])
    outs = {}
    for mode in ("step", "rollout"):
        from multidronesim_amd.envs.CtrlAviary import CtrlAviary, DroneModel, Physics
        import types
        gains = DC.GAINS["skew"]
        env = CtrlAviary(drone_model=DroneModel.CF2P, num_drones=D, initial_xyzs=xyz, initial_rpys=np.zeros((E, D, 3)), physics=Physics.DYN,
                         pyb_freq=240, ctrl_freq=240, num_envs=E, dtype=dtype)
        env.set_dslpid_gains(types.SimpleNamespace(P_COEFF_FOR=gains["P_FOR"], I_COEFF_FOR=gains["I_FOR"], D_COEFF_FOR=gains["D_FOR"],
                                                   P_COEFF_TOR=gains["P_TOR"], I_COEFF_TOR=gains["I_TOR"], D_COEFF_TOR=gains["D_TOR"]))
        env.step(mds.torch.zeros((E, D, 4), dtype=env.dtype))
        if mode == "step":
            for k in range(T):
                gobs = env.step_dslpid(tgt if k < T // 2 else tgt2, trpy)
        else:
            env.rollout_dslpid(tgt, trpy, T // 2)
            gobs = env.rollout_dslpid(tgt2, trpy, T - T // 2)
        g = host(gobs).reshape(-1, 20)
        outs[mode] = AC.state_err(g, ref[-1])
        report(case["name"] + " " + mode, dtype, outs[mode], gate, d_mir)
        assert AC.rel_err(g[:, 16:], ref[-1][:, 16:]) < max(gate, 2e-6)
        env.close()
    assert pid_env is not None and max(outs.values()) < gate


# ---- i: mds_quadrotor_dynamics / mds_compare_models ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_quadrotor_dynamics_and_compare_models_with_an_asymmetric_inertia(mds, dtype):
    """model/dynamics.py's derivative and the CompareModels row kernel with J = (0.9, 1.3, 2.05) on 69 rows: every golden of these two uses the
    Hummingbird J = (1.05, 1.05, 2.05) or the urdf's, where the z row of w x Jw vanishes."""
    from multidronesim_amd.model import LinearizedModel, QuadrotorDynamics
    from multidronesim_amd.simulations.CompareModels import compare_models
    torch = mds.torch
    tdt = getattr(torch, dtype)
    cd, cc = AC.case_dyn(), AC.case_cmp()
    ref_d, gate_d, mir_d = conditions(cd, dtype)
    ref_c, gate_c, mir_c = conditions(cc, dtype)
    q = QuadrotorDynamics(sim_freq=100)
    q.J = np.diag(AC.DYN_J)
    x, u = AC.dyn_rows()
    got = q.dynamics(0.0, torch.as_tensor(x, dtype=tdt, device="cuda"), torch.as_tensor(u, dtype=tdt, device="cuda"))
    err = AC.rel1_err(host(got), ref_d)
    report(cd["name"], dtype, err, gate_d, mir_d)
    assert err < gate_d
    env = mds.CtrlAviary(drone_model=mds.DroneModel.CF2P, num_drones=2, initial_xyzs=np.zeros((1, 2, 3)), initial_rpys=np.zeros((1, 2, 3)),
                         physics=mds.Physics.DYN, pyb_freq=100, ctrl_freq=100, num_envs=1, dtype=dtype)
    lin = LinearizedModel(env)
    geo = QuadrotorDynamics(env.PYB_FREQ)
    geo.load_env_params(env)
    geo.J = np.diag(AC.DYN_J)
    a, b, c = compare_models(lin, geo, torch.as_tensor(AC.cmp_rows(), dtype=tdt, device=env.device))
    r_lin, r_geo, r_x = AC.cmp_run()
    err = max(AC.rel1_err(host(b), r_geo), AC.rel1_err(host(a), r_lin), AC.rel1_err(host(c), r_x))
    report(cc["name"], dtype, err, gate_c, mir_c)
    assert err < gate_c
    env.close()


# ---- j: the CBF loop with the geometric nominal --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("form", ["three launches", "one launch", "persistent"])
def test_cbf_loop_with_the_geometric_nominal(mds, form, dtype):
    """30 control steps of the CBF-filtered loop (geometric nominal with set A -> ECBF QP -> ThrustOmega -> step) on 3 x 4 drones, stacked
    trajectories 15 cm apart (pair rows act) and a sphere under drone 1's descent, in all three step-kernel forms: statuses at every step
    and the final state against the oracle's loop."""
    from multidronesim_amd.cbf.cbf import DroneCBF
    from multidronesim_amd.cbf.qptracker import DroneQPTracker
    from multidronesim_amd.model.linear_omega import LinearizedOmegaModel
    torch = mds.torch
    case = AC.case_cbf()
    ref, gate, d_mir = conditions(case, dtype)
    _, ohist = AC.cbf_run()
    E, D, T = AC.CBF_E, AC.CBF_D, AC.CBF_STEPS
    xyz, rpy, P, x_obs, obs_r = AC.cbf_setup()
    env = make_env(mds, E, D, xyz, rpy, dtype)
    env.set_trajectories(P)
    cbf = DroneCBF(env, [LinearizedOmegaModel(env) for _ in range(D)], safety_radius=AC.CBF_RADIUS, zscale=AC.CBF_ZSCALE, order=2, cbf_poles=np.array(AC.CBF_POLES))
    trk = DroneQPTracker(cbf, num_robots=D, xdim=9, env=env)
    np.testing.assert_allclose(cbf.Kcbf.reshape(-1), O.place_poles_chain(list(AC.CBF_POLES)), rtol=1e-10)
    np.testing.assert_allclose(cbf.umax, [AC.A.MAX_THRUST, 10.0, 10.0, 10.0], rtol=1e-12)
    env.step(torch.zeros((E, D, 4), dtype=env.dtype))
    if form == "persistent":
        slog = torch.empty((T, E), dtype=torch.int32, device=env.device)
        gobs, _ = env.rollout_cbf_geometric_fused(0.0, T, trk, x_obs, obs_r, steps_per_launch=16, status_log=slog)
        statuses = slog.cpu().numpy()
    else:
        env.set_cbf_step_kernel(0 if form == "three launches" else 1)
        t, rows = 0.0, []
        for k in range(T):
            gobs, st = env.step_cbf_geometric(t, trk, x_obs, obs_r)
            rows.append(st.cpu().numpy().copy())
            t += env.CTRL_TIMESTEP
        statuses = np.array(rows)
    np.testing.assert_array_equal(statuses, ohist)
    err = AC.state_err(host(gobs), ref)
    report(case["name"] + " " + form + f" (kernel form {env.cbf_last_step_kernel()})", dtype, err, gate, d_mir)
    assert err < gate
    assert env.cbf_last_step_kernel() == {"three launches": 0, "one launch": 1, "persistent": 2}[form]
    env.close()


# ---- k: FedCE, 12-state ------------------------------------------------------------------------------------------------------------------------------
def test_fedce_identification_with_constants_a(mds):
    """One mds_fedce_identify call (20 exploration steps, round-tripped inputs, an update every step) on a 2 x 2 float64 handle with constants
    A against tests/fedce_oracle.py's DLQR(c=A): theta and P afterwards.  The regressor divides the torques by J[0], J[1], J[2] and the mixer
    round trip uses L, KF, KM: with the urdf's Jx == Jy two of those could be swapped unseen."""
    from multidronesim_amd.control import DecentralizedLQR
    from multidronesim_amd.control.dlqr.decentralized_lqr import U_ROUND_TRIP
    from multidronesim_amd.model import LinearizedModel
    case = AC.case_fedce()
    _, gate, d_mir = conditions(case, "float64")
    E, D, T = AC.FEDCE_E, AC.FEDCE_D, AC.FEDCE_STEPS
    s, u, x_des = AC.fedce_setup()
    env = make_env(mds, E, D, s[:, 0:3].reshape(E, D, 3), np.zeros((E, D, 3)), "float64")
    env.set_state(s)
    s0 = env.get_state().reshape(-1, 13)
    dl = DecentralizedLQR(env, [LinearizedModel(env) for _ in range(D)])
    _, obs1 = dl.identify(u.reshape(T, E, D, 4), U_ROUND_TRIP, x_des.reshape(E, D, 12), True)
    th_ref, P_ref, o_ref = AC.fedce_run(state13=s0)
    e_th, e_P = AC.max_rel(dl.theta, th_ref), AC.max_rel(dl.P, P_ref)
    report(case["name"] + " theta", "float64", e_th, gate, d_mir)
    report(case["name"] + " P", "float64", e_P, gate, d_mir)
    np.testing.assert_allclose(host(obs1).reshape(-1, 20)[:, :16], o_ref[:, :16], rtol=1e-12, atol=1e-12)
    assert e_th < gate and e_P < gate
    env.close()

"""The x/y-asymmetric parameter set of tests/aniso_cases.py (constants A, gains A) on the CPU, before any GPU time is spent:

  * the NumPy oracle against two fixtures minted from the reference with set A (tests/golden/geometric_compute_aniso.npz,
    dyn_wrench_accel_aniso.npz; mint_geometric_aniso / mint_dyn_wrench_accel_aniso of tests/golden/mint_golden.py), at the tolerances
    tests/test_oracle_golden.py uses for their stock siblings: the oracle was pinned to the reference with Jx == Jy and isotropic gains only;
  * the plain-C oracle against the NumPy oracle on set A where its constant block exposes the operation;
  * the host builds of the device code (tests/emul: csrc/mds_math.hpp under g++; tests/emul/simt: the step and rollout kernels themselves)
    against the oracle with set A;
  * the two conditions every case of tests/test_gpu_aniso.py must meet, on the oracle alone: the mirrored and the isotropised set move the
    oracle by at least 100 x the case's gate in the case's own metric, and at most 10 % of the (row, step) pairs have a motor at a limit.

Measured here (max error against the oracle with set A): emulated geometric_compute, relative RPM, float64 1.3e-15, float32 5.7e-7 (gate
1e-6); 12 emulated physics steps float64 <= 1.1e-15, float32 <= 5.0e-7; k_step_geometric / k_rollout_geometric on 3 x 5 drones over 40 steps
float64 4.9e-15, float32 1.5e-6, k_step / k_rollout_step 8.9e-15 and 2.4e-6.  With Jx and Jy swapped in fill_consts (csrc/mds_consts.hpp) every
emulated case below fails (7.5e-2 on the state) while tests/test_emul_device_math.py, on the stock constants, still passes."""
import ctypes as C
import os

import numpy as np
import pytest

from oracle import np_oracle as O
from tests import aniso_cases as AC
from tests import dslpid_cases as DC
from tests import helpers as H

G = os.path.join(os.path.dirname(__file__), "golden")


# ---- the oracle itself, pinned to the reference with asymmetric parameters ---------------------------------------------------------------
def test_oracle_geometric_compute_matches_the_reference_with_set_a():
    d = AC.geo_fixture()
    assert tuple(d["J"]) == AC.CONSTANTS["J"] and float(d["M"]) == AC.CONSTANTS["M"] and all(tuple(d[k]) == AC.GAINS[k] for k in AC.GAINS)
    assert d["obs"].shape[0] == 128 and (int(d["n_rand"]), int(d["n_tilt"]), int(d["n_clip"])) == (96, 16, 16)
    rpm = AC.geo_run()
    np.testing.assert_allclose(rpm, d["rpm"], rtol=1e-11, atol=1e-7)
    f, w, Rd = AC.geo_run(return_omegas=True)
    np.testing.assert_allclose(f, d["force"], rtol=1e-11, atol=1e-13)
    np.testing.assert_allclose(w, d["w_des"], rtol=1e-9, atol=1e-11)
    np.testing.assert_allclose(Rd, d["R_des"], rtol=0, atol=1e-12)
    # the fixture tells the mirrored and the isotropised set from A, and the stock set from all of them
    for cs, gn in (AC.mirrored(), AC.isotropised()):
        assert AC.rel_err(AC.geo_run(cs, gn), d["rpm"]) > 1e-3
    assert np.abs(d["des"][:96, 9]).min() > 0.2 and np.abs(d["obs"][:, 13:16]).min() > 0          # non-zero desired yaw, no zero body rate
    assert (np.abs(d["rpm"][96:] - AC.MIN_RPM) < 1e-6).any(axis=1).sum() >= 8                     # families (b) and (c) clip, as in the stock fixture


def test_oracle_wrench_and_accelerations_match_the_reference_with_set_a():
    d = np.load(os.path.join(G, "dyn_wrench_accel_aniso.npz"))
    c = AC.A
    assert d["rpm"].shape == (192, 4)
    assert abs(c.MAX_RPM - float(d["max_rpm"])) < 1e-9 and c.M == float(d["m"]) and c.G == float(d["g"])
    np.testing.assert_allclose(np.asarray(c.J), d["J"], rtol=0, atol=0)
    clipped = np.clip(d["rpm"], 0, c.MAX_RPM)
    thrust, tau = O.rotor_wrench(clipped, c)
    np.testing.assert_allclose(thrust, d["u"][:, 0], rtol=1e-13, atol=1e-16)
    np.testing.assert_allclose(tau, d["u"][:, 1:], rtol=1e-12, atol=1e-18)
    _, _, acc, wdot = O.dyn_derivative(d["pos"], d["quat"], d["vel"], d["rates"], clipped, c)
    np.testing.assert_allclose(acc, d["v_dot"], rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(wdot, d["w_dot"], rtol=1e-12, atol=1e-9)
    for dt in (1 / 240, 1 / 100):
        _, _, v1, w1, _ = O.dyn_step_euler(d["pos"], d["quat"], d["vel"], d["rates"], clipped, dt, c)
        np.testing.assert_allclose((v1 - d["vel"]) / dt, d["v_dot"], rtol=0, atol=1e-10)
        np.testing.assert_allclose((w1 - d["rates"]) / dt, d["w_dot"], rtol=1e-10, atol=1e-7)
    # the z row carries (Jx - Jy) wx wy / Jz, zero with the urdf's inertia: with the mirrored J the oracle misses the fixture by its size
    _, _, _, wdot_m = O.dyn_derivative(d["pos"], d["quat"], d["vel"], d["rates"], clipped, AC.consts(AC.mirrored()[0]))
    gyro_z = (c.J[0] - c.J[1]) * d["rates"][:, 0] * d["rates"][:, 1] / c.J[2]
    assert np.abs(gyro_z).max() > 1.0
    np.testing.assert_allclose(wdot_m[:, 2] - d["w_dot"][:, 2], -2 * gyro_z, rtol=1e-9, atol=1e-9)


# ---- the plain-C oracle on set A -----------------------------------------------------------------------------------------------------------
def c_consts(pyb=100, ctrl=100):
    """oracle/c_oracle.py's constant block with set A written over its fields.  It has M, L, KF, KM, J, G, MAX_RPM, MAX_THRUST and the
    geometric gains; it has NO drag coefficients (and no CF2X mixer): the drag and CF2X operations are not compared here."""
    from oracle import c_oracle as CO
    c = CO.consts(pyb, ctrl)
    assert not hasattr(c, "DRAG") and not hasattr(c, "drag_coeff")
    a = AC.A
    c.M, c.L, c.KF, c.KM, c.G, c.MAX_RPM, c.MAX_THRUST = a.M, a.L, a.KF, a.KM, a.G, a.MAX_RPM, a.MAX_THRUST
    c.J = (C.c_double * 3)(*a.J)
    for k in ("Kp", "Kv", "KR", "Kw"):
        setattr(c, k, (C.c_double * 3)(*AC.GAINS[k]))
    return c


def test_c_oracle_agrees_with_the_numpy_oracle_on_set_a():
    from oracle import c_oracle as CO
    d = AC.geo_fixture()
    np.testing.assert_allclose(CO.geometric_compute(d["obs"], d["des"], c_consts()), AC.geo_run(), rtol=1e-11, atol=1e-7)
    # the DYN step and the whole geometric loop (the yaw-free and the yawing Lemniscates of case d) with the constant block swapped in
    for yaw_rate in (0.0, 0.3):
        xyz, rpy, P = AC.loop_setup(yaw_rate)
        av = CO.AviaryC(xyz.reshape(-1, 3), rpy.reshape(-1, 3), 100, 100)
        av.c = c_consts()
        got, _ = av.geometric_loop(P, AC.LOOP_STEPS)
        ref = AC.loop_run(yaw_rate)[-1]
        assert AC.state_err(got, ref) < 1e-11 and AC.rel_err(got[:, 16:], ref[:, 16:]) < 1e-10
    s = AC.states(AC.STEP_N, 1)
    av = CO.AviaryC(s[:, 0:3], np.zeros((AC.STEP_N, 3)), 240, 240)
    av.c = c_consts(240, 240)
    av.st[:, :13] = s
    for k in range(AC.STEP_STEPS):
        got = av.step(AC.step_actions("dyn_euler", k, AC.A))
    assert AC.state_err(got, AC.step_run("dyn_euler")) < 1e-12


# ---- the two conditions of every GPU case ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", AC.all_cases(), ids=lambda c: c["name"])
def test_gpu_case_discriminates_and_stays_off_the_motor_limits(case):
    d_mir, d_iso, frac = AC.check_conditions(case)
    print("%-36s largest gate %.1e: mirrored set %.3e, isotropised set %s, clipped (row, step) pairs %.1f %%" % (
        case["name"], max(case["gate"].values()), d_mir, "-" if d_iso is None else "%.3e" % d_iso, 100 * frac))


def test_cbf_case_has_an_active_pair_row_and_an_active_sphere():
    """Case j's scene: the filter changes the nominal input with the sphere taken away (pair rows act), the sphere changes the outcome, and the
    statuses are not all alike (feasible and infeasible env-steps both occur, or the filter acts in every env)."""
    log, log0 = [], []
    obs, hist = AC.cbf_run(filter_log=log)
    obs0, hist0 = AC.cbf_run(sphere=False, filter_log=log0)
    assert np.array(log0).max() > 1e-3, "no pair row ever acts"
    assert AC.state_err(obs, obs0) > 1e-4, "the sphere changes nothing"
    assert hist.shape == (AC.CBF_STEPS, AC.CBF_E)
    assert (np.array(log).max(axis=0) > 1e-6).any()


def test_dslpid_skew_gain_set_is_what_the_issue_asks_and_discriminates():
    """Case h: every vector of "skew" has three distinct non-zero entries within +-40 % of "halved" (the two zero I_TOR entries: of 250), and
    the x/y mirror of the set moves the oracle's RPM by more than 100 x the float32 gate at both rates."""
    sk, hv = DC.GAINS["skew"], DC.GAINS["halved"]
    for k, v in sk.items():
        assert len(set(v.tolist())) == 3 and (v != 0).all()
        base = np.where(hv[k] == 0, 250.0, hv[k])
        assert (np.abs(v / base - 1) <= 0.4 + 1e-12).all(), k
    for rate in DC.RATES:
        obs, tp, tr, _ = DC.make_cases(ctrl_freq=rate)
        ref = DC.reference("cf2p", rate, "skew", "float64")
        mir = DC.run(DC.oracle_for(obs.shape[1], "cf2p", DC.mirrored(sk)), 1.0 / rate, obs, tp, tr)
        dist = float(np.abs(mir / ref - 1).max())
        print("skew, %d Hz: mirrored gains move the RPM by %.3e (float32 gate %.3e)" % (rate, dist, DC.gate(rate, "skew", "float32")))
        assert dist >= AC.FACTOR * DC.gate(rate, "skew", "float32")


# ---- the host build of the device arithmetic (tests/emul) ----------------------------------------------------------------------------------
@pytest.mark.parametrize("dt,tol_thrust,tol_aux", [("f64", 1e-13, 1e-13), ("f32", 1e-6, 2e-6)])
def test_emulated_geometric_compute_with_set_a(dt, tol_thrust, tol_aux):
    """test_emul_device_math.py's test_geometric_golden (relative RPM 1e-13 / 1e-6, aux 1e-13 / 2e-6) on the set-A fixture."""
    from tests.emul import emul as E
    d = AC.geo_fixture()
    rpm, aux = E.Emul(dt, constants=AC.CONSTANTS, gains=AC.GAINS).geometric_compute(d["obs"], d["des"])
    err = AC.rel_err(rpm, d["rpm"])
    print(f"emulated geometric_compute {dt}, set A: relative RPM error {err:.2e} (gate {tol_thrust:.0e})")
    assert err < tol_thrust
    assert np.abs(aux[:, 0] - d["force"]).max() < tol_aux
    assert np.abs(aux[:, 1:4] - d["w_des"]).max() < tol_aux * 5
    assert np.abs(aux[:, 4:].reshape(-1, 3, 3) - d["R_des"]).max() < tol_aux
    for cs, gn in (AC.mirrored(), AC.isotropised()):                      # a build with x and y swapped, or averaged, would be this far off
        wrong, _ = E.Emul(dt, constants=cs, gains=gn).geometric_compute(d["obs"], d["des"])
        assert AC.rel_err(wrong, d["rpm"]) > AC.FACTOR * tol_thrust


@pytest.mark.parametrize("variant", ["dyn_euler", "drag_euler", "drag_rk4"])
@pytest.mark.parametrize("dt,tol", [("f64", 1e-12), ("f32", 5e-6)])
def test_emulated_physics_steps_with_set_a(variant, dt, tol):
    """12 steps of step_euler / step_rk4 (with and without the drag term) from case a's states: body rates up to 3 rad/s, so (Jy - Jx) wx wy
    is large.  float64 1e-12 (test_open_loop_f64_matches_oracle: 1e-10 over 300 steps); float32 5e-6 (half of north_star's 1e-5; measured <= 9.8e-7)."""
    from tests.emul import emul as E
    kw = AC.STEP_VARIANTS[variant]
    em = E.Emul(dt, num_envs=AC.STEP_N, pyb_freq=kw["pyb"], ctrl_freq=kw["ctrl"], physics=int(kw["physics"] == "dyn_drag"),
                integrator=int(kw["integrator"] == "rk4"), constants=AC.CONSTANTS)
    em.set_state(AC.states(AC.STEP_N, 1))
    s0 = em.get_state()                                        # as stored (float32-rounded)
    for k in range(AC.STEP_STEPS):
        got = em.step(AC.step_actions(variant, k, AC.A))
    ref = AC.step_run(variant, state13=s0)
    err = AC.state_err(got, ref)
    print(f"emulated {variant} {dt}, set A: max state error {err:.2e} (gate {tol:.0e})")
    assert err < tol
    assert AC.state_err(got, AC.step_run(variant, AC.mirrored()[0], state13=s0)) > AC.FACTOR * tol


# ---- the host build of the kernels themselves (tests/emul/simt) ------------------------------------------------------------------------------
def _simt():
    from tests.emul.simt import simt
    if not simt.available():
        pytest.skip("no host clang++ with sanitizer runtimes")
    return simt


@pytest.fixture(scope="module")
def headline_exe():
    simt = _simt()
    return simt.build(only=(simt.EXE[4],))


SIMT_TOL = {"float64": 1e-11, "float32": 2e-5}                  # HEADLINE_TOL of test_simt_sanitizers_cpu.py


@pytest.mark.parametrize("yaw_rate", [0.0, 0.3])
@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("form", [0, 1])
def test_simt_geometric_kernels_with_set_a(headline_exe, dtype, form, yaw_rate):
    """k_step_geometric (form 0) and k_rollout_geometric (form 1) compiled for the host from their own sources, 3 x 5 drones over 40 steps, the
    yaw-free arm (yaw rate 0) and the general one (0.3), against the oracle's loop with set A."""
    simt = _simt()
    E, D, steps = 3, 5, 40
    xyz, _, P = H.c2_setup(E, D, seed=5, phase="c3", yaw_rate=yaw_rate)
    rpy = np.random.default_rng(6).uniform(-0.4, 0.4, size=(E, D, 3))
    hist = {}
    for name, (cs, gn) in (("A", (AC.CONSTANTS, AC.GAINS)), ("mirrored", AC.mirrored())):
        _, h = H.oracle_closed_loop(xyz, rpy, P, steps, consts=AC.consts(cs), gains=gn, record_every=1)
        hist[name] = np.stack(h)
    o0 = hist["A"][0]                                           # after env.step(zeros): free fall from rest, identical for both sets
    assert not o0[:, 13:16].any()
    state13 = np.concatenate([o0[:, 0:7], o0[:, 10:13], np.zeros((E * D, 3))], axis=1).reshape(E, D, 13)
    obs, st, act, err = simt.headline(dtype, form, 0.0, P, np.ascontiguousarray(state13), steps, constants=AC.CONSTANTS, gains=AC.GAINS)
    assert "ERROR" not in err and "runtime error" not in err, err[-3000:]
    ref = hist["A"][-1].reshape(E, D, 20)
    e = AC.state_err(obs, ref)
    clipped = AC.at_limit(hist["A"][1:, :, 16:20], AC.A).mean()
    print(f"simt form {form} {dtype} yaw rate {yaw_rate}, set A: max state error {e:.2e} (gate {SIMT_TOL[dtype]:.0e}); mirrored set {AC.state_err(hist['mirrored'][-1], hist['A'][-1]):.2e}; clipped {clipped:.1%}")
    assert e < SIMT_TOL[dtype]
    assert AC.rel_err(obs[..., 16:], ref[..., 16:]) < 1e-4
    assert AC.state_err(hist["mirrored"][-1], hist["A"][-1]) > AC.FACTOR * SIMT_TOL[dtype] and clipped <= 0.10


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("form", [2, 3])
def test_simt_step_kernels_with_set_a(headline_exe, dtype, form):
    """k_step (form 2) and k_rollout_step (form 3) on a 3-set action table, 3 x 5 drones over 40 steps from states with body rates up to 3 rad/s."""
    simt = _simt()
    E, D, steps = 3, 5, 40
    s = AC.states(E * D, 21)
    rng = np.random.default_rng(2)
    actions = (AC.A.HOVER_RPM * (1 + 0.05 * rng.uniform(-1, 1, size=(3, E, D, 4)))).astype(np.float32).astype(np.float64)
    refs = {}
    for name, cs in (("A", AC.CONSTANTS), ("mirrored", AC.mirrored()[0])):
        ora = AC.oracle_from_state(s, AC.consts(cs), 100, 100)
        for k in range(steps):
            refs[name] = ora.step(actions[k % 3].reshape(-1, 4))
    P = H.c2_setup(E, D)[2]
    obs, st, _, err = simt.headline(dtype, form, 0.0, P, s.reshape(E, D, 13), steps, actions=actions, constants=AC.CONSTANTS, gains=AC.GAINS)
    assert "ERROR" not in err and "runtime error" not in err, err[-3000:]
    e = AC.state_err(obs.reshape(-1, 20), refs["A"])
    print(f"simt form {form} {dtype}, set A: max state error {e:.2e} (gate {5 * SIMT_TOL[dtype]:.0e}); mirrored set {AC.state_err(refs['mirrored'], refs['A']):.2e}")
    assert e < 5 * SIMT_TOL[dtype]
    assert AC.state_err(refs["mirrored"], refs["A"]) > AC.FACTOR * 5 * SIMT_TOL[dtype]

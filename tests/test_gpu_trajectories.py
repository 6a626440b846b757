"""GPU parity of the general trajectory path: the reference's trajectory classes (golden vectors minted
from trajectories/*.py) through mds_traj_eval, and the fused step driven by segment tables against the
oracle loop."""
import os
import types

import numpy as np
import pytest

from oracle import np_oracle as O
from oracle import np_trajectories as NT
from tests.golden.mint_golden import trajectory_cases
from tests import traj_cases as TC

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")


def gpu_classes():
    import multidronesim_amd.trajectories as TR
    return types.SimpleNamespace(Lemniscate=TR.Lemniscate, Circle=TR.CircleTrajectory, Line=TR.LineTrajectory, Wait=TR.WaitTrajectory,
                                 Compound=TR.CompoundTrajectory, Rotate=TR.RotateTrajectory)


def oracle_classes():
    return types.SimpleNamespace(Lemniscate=NT.Lemniscate, Circle=NT.Circle, Line=NT.Line, Wait=NT.Wait, Compound=NT.Compound, Rotate=NT.Rotate)


def test_trajectory_call_matches_reference_golden():
    d = np.load(os.path.join(G, "trajectories.npz"))
    cases = trajectory_cases(gpu_classes())
    assert list(d["names"]) == list(cases)
    for name, tr in cases.items():
        np.testing.assert_allclose(tr.get_total_time(), float(d[name + "_total"]), rtol=1e-14)
        ts, want = d[name + "_t"], d[name + "_out"]
        for k in range(0, len(ts), 3):
            pos, vel, acc, yaw, om = tr(float(ts[k]))
            got = np.hstack([pos, vel, acc, yaw, om])
            np.testing.assert_allclose(got, want[k], rtol=0, atol=1e-11, err_msg=f"{name} t={ts[k]}")


@pytest.mark.parametrize("dtype,tol", [("float64", 1e-9), ("float32", 2e-5)])
def test_fused_step_on_segment_tables_matches_oracle(dtype, tol):
    """EnvGeometric-style loop where every drone follows a different kind of trajectory (the commented-out
    CompoundTrajectory of EnvGeometric.py:543-550 among them)."""
    from multidronesim_amd.envs.CtrlAviary import CtrlAviary, DroneModel, Physics
    gc, oc = trajectory_cases(gpu_classes()), trajectory_cases(oracle_classes())
    names = ["compound", "circle", "rotate", "line_s0", "compound_mixed", "wait"]
    D, E, steps = len(names), 3, 400
    gtr, otr = [gc[n] for n in names], [oc[n] for n in names]
    xyz = np.array([np.asarray(o(0.0)[0], dtype=np.float64) + np.array([0.05, -0.03, 0.02]) for o in otr])
    xyz = np.broadcast_to(xyz, (E, D, 3)).copy()
    env = CtrlAviary(drone_model=DroneModel.CF2P, num_drones=D, initial_xyzs=xyz, initial_rpys=np.zeros((E, D, 3)), physics=Physics.DYN,
                     pyb_freq=100, ctrl_freq=100, num_envs=E, dtype=dtype)
    env.set_trajectories(gtr)
    n = E * D
    ora = O.AviaryOracle(xyz.reshape(-1, 3), np.zeros((n, 3)), pyb_freq=100, ctrl_freq=100)
    obs = ora.step(np.zeros((n, 4)))
    import torch
    env.step(torch.zeros((E, D, 4), dtype=env.dtype))
    t = 0.0
    for k in range(steps):
        des = np.array([np.hstack([np.asarray(x, dtype=np.float64) * np.ones(np.size(x)) for x in otr[i % D](t)]) for i in range(n)])
        obs = ora.step(O.geometric_compute(obs, des[:, 0:3], des[:, 3:6], des[:, 6:9], des[:, 9], des[:, 10]))
        gobs = env.step_geometric(t)
        t += env.CTRL_TIMESTEP
    g = gobs.double().cpu().numpy().reshape(n, 20)
    per_drone = np.abs(g[:, :16] - obs[:, :16]).max(axis=1).reshape(E, D).max(axis=0)
    err = dict(zip(names, per_drone))
    # the tilted (rotated) Lemniscate is the ill-conditioned one: it rides the 40-degree tilt clamp, and already
    # in float64 its error is 1000x the others' (3e-12 vs 1e-15); in fp32 that factor gives ~1e-3.
    assert max(v for k, v in err.items() if k != "rotate") < tol, err
    assert err["rotate"] < tol * 500, err
    o2 = env.rollout_geometric(t, 10)                       # the C loop also runs the general kernel
    assert np.isfinite(o2.double().cpu().numpy()).all()
    o3, _ = env.rollout_geometric_fused(t + 10 * env.CTRL_TIMESTEP, 5)   # and so does the multi-step kernel (k_rollout_traj)
    assert np.isfinite(o3.double().cpu().numpy()).all()
    env.close()


@pytest.mark.parametrize("dtype,tol,T,T2,marks", [("float64", 1e-9, 150, 90, (0, 70, 149)), ("float32", 1e-5, 60, 30, (0, 46, 59))])
def test_whole_rollout_on_segment_tables_equals_stepwise(dtype, tol, T, T2, marks):
    """mds_rollout_geometric_fused on general trajectories (k_rollout_traj): T steps in one launch == T mds_step_geometric calls.
    float32 (gate: the fp32 form-equivalence gate of test_rollout_launch_form_policy_and_equivalence, 1e-5 on the state columns and
    relative on the RPM echo): 60 + 30 steps on a short Compound whose two piece boundaries (0.45 s, 0.55 s) fall inside the first
    launch and whose end (0.75 s) inside the second, so the rollout kernel's fp32 piece scan and its past-the-end arm are compared too."""
    import torch
    from multidronesim_amd.envs.CtrlAviary import CtrlAviary, DroneModel, Physics
    from multidronesim_amd import trajectories as TR
    E, D = 9, 3
    rng = np.random.default_rng(2)
    xyz = rng.uniform(-0.5, 0.5, size=(E, D, 3)) + np.array([0, 0, 1.0])
    def trajs():
        out = []
        for e in range(E):
            for d in range(D):
                a = xyz[e, d]
                if dtype == "float32":
                    b = a + np.array([0.04, -0.02, 0.0224])
                    out.append(TR.CompoundTrajectory([TR.LineTrajectory(start=a, end=b, speed=0.6), TR.WaitTrajectory(duration=0.1, position=b, yaw=0.2),
                                                      TR.CircleTrajectory(r=0.1, v=0.3, center=b - np.array([0.1, 0, 0]), yaw_rate=0.3, duration=0.2)]))
                    continue
                out.append(TR.CompoundTrajectory([TR.LineTrajectory(start=a, end=a + np.array([0.4, -0.2, 0.3]), speed=0.6),
                                                  TR.WaitTrajectory(duration=0.3, position=a + np.array([0.4, -0.2, 0.3]), yaw=0.2),
                                                  TR.CircleTrajectory(r=0.3, v=0.5, center=a + np.array([0.4, -0.5, 0.3]), yaw_rate=0.3)]))
        return out
    if dtype == "float32":
        ends = trajs()[0].times
        assert 0.0 < ends[0] < ends[1] < (T - 1) * 0.01 and T * 0.01 < ends[2] < (T + T2 - 1) * 0.01, ends
    envs = []
    for _ in range(2):
        env = CtrlAviary(drone_model=DroneModel.CF2P, num_drones=D, initial_xyzs=xyz, initial_rpys=np.zeros((E, D, 3)), physics=Physics.DYN,
                         pyb_freq=200, ctrl_freq=100, num_envs=E, dtype=dtype)
        env.set_trajectories(trajs())
        env.step(torch.zeros((E, D, 4), dtype=env.dtype))
        envs.append(env)
    a, b = envs

    def close(x, y):
        x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
        if dtype == "float64":
            np.testing.assert_allclose(x, y, atol=tol)
        else:
            np.testing.assert_allclose(x[..., :16], y[..., :16], atol=tol)
            np.testing.assert_allclose(x[..., 16:], y[..., 16:], rtol=tol)
    last, log = a.rollout_geometric_fused(0.0, T, log=True)
    t = 0.0
    for k in range(T):
        o = b.step_geometric(t)
        t += b.CTRL_TIMESTEP
        if k in marks:
            close(log[k].double().cpu().numpy(), o.double().cpu().numpy())
    np.testing.assert_allclose(a.get_state(), b.get_state(), atol=tol)
    # the same loop through mds_rollout_geometric in launch form 2 (mds_set_rollout_form: the whole-rollout kernel in launches of 40 steps,
    # every step's observation into the one buffer), continuing both envs: == the step-by-step continuation
    a.set_rollout_form(2, 40)
    oa = a.rollout_geometric(T * a.CTRL_TIMESTEP, T2, obs_every_step=True)
    assert a.last_rollout_form() == 2
    t = T * b.CTRL_TIMESTEP
    for k in range(T2):
        ob = b.step_geometric(t)
        t += b.CTRL_TIMESTEP
    close(oa.double().cpu().numpy(), ob.double().cpu().numpy())
    np.testing.assert_allclose(a.get_state(), b.get_state(), atol=tol)
    a.close(); b.close()


def test_two_stream_rollout_on_segment_tables_is_bit_identical():
    """mds_set_rollout_streams(2) on the general kernel: tables of 1 and 3 pieces (two storage blocks), shared and rotated ones,
    1400 drones (5 full batches + 120): same bits as the one-stream loop."""
    import torch
    from multidronesim_amd.envs.CtrlAviary import CtrlAviary, DroneModel, Physics
    gc = trajectory_cases(gpu_classes())
    names = ["compound", "circle", "rotate", "line_s0", "compound_mixed", "wait", "circle"]
    D, E, T = len(names), 200, 45
    oc = trajectory_cases(oracle_classes())
    xyz = np.array([np.asarray(oc[n](0.0)[0], dtype=np.float64) + np.array([0.05, -0.03, 0.02]) for n in names])
    xyz = np.broadcast_to(xyz, (E, D, 3)).copy()
    out = []
    for streams in (1, 2):
        env = CtrlAviary(drone_model=DroneModel.CF2P, num_drones=D, initial_xyzs=xyz, initial_rpys=np.zeros((E, D, 3)), physics=Physics.DYN,
                         pyb_freq=200, ctrl_freq=100, num_envs=E, dtype="float32")
        env.set_trajectories([gc[n] for n in names])
        env.set_rollout_streams(streams)
        env.step(torch.zeros((E, D, 4), dtype=env.dtype))
        o = env.rollout_geometric(0.0, T, obs_every_step=True).clone()
        out.append((o.cpu().numpy(), env.get_state()))
        env.close()
    assert np.isfinite(out[0][0]).all()
    np.testing.assert_array_equal(out[0][0], out[1][0])
    np.testing.assert_array_equal(out[0][1], out[1][1])


# ---- the segment-table path at operator level: 333 drones on 22 tables (tests/traj_cases.py), 39 edge times ----------------------------
E333, D333 = 9, 37


@pytest.fixture(scope="module")
def tables():
    """The drone set once per module: library objects, names, the 39 times and the oracle's desired state [39, 333, 11]."""
    lobjs, names = TC.drones(TC.library_classes())
    oobjs, _ = TC.drones(TC.oracle_classes())
    ts = TC.times_gpu(oobjs)
    return types.SimpleNamespace(lobjs=lobjs, oobjs=oobjs, names=names, ts=ts, want=TC.oracle_desired(oobjs, names, ts),
                                 scale=TC.f64_gate_scale(oobjs, names, ts), anchors=np.array([lobjs[n].anchor() for n in names]))


def make_env(dtype, E, D, xyz=None):
    from multidronesim_amd.envs.CtrlAviary import CtrlAviary, DroneModel, Physics
    xyz = np.zeros((E, D, 3)) if xyz is None else xyz
    return CtrlAviary(drone_model=DroneModel.CF2P, num_drones=D, initial_xyzs=xyz, initial_rpys=np.zeros((E, D, 3)), physics=Physics.DYN,
                      pyb_freq=100, ctrl_freq=100, num_envs=E, dtype=dtype)


def device_desired(env, ts):
    return np.stack([env.traj_eval(float(t)).double().cpu().numpy().reshape(env.n, 11) for t in ts])


def assert_desired(got, want, dtype, scale=1.0, what=""):
    """float64: 1e-11 (the gate of test_trajectory_call_matches_reference_golden) times max(1, |phase| 2^-52 1e3) for the large-t samples
    (|phase| <= the drone's largest omega, v / r or yaw rate, times |t|).  float32: mds_traj_eval is the double evaluation rounded once,
    so 2^-23 relative per component with max(1, |x|) as the scale.  Yaw modulo 2 pi."""
    d = np.abs(got - want)
    d[..., 9] = np.abs(TC.wrap(got[..., 9] - want[..., 9]))
    gate = 1e-11 * np.asarray(scale)[..., None] if dtype == "float64" else 2.0 ** -23 * np.maximum(1.0, np.abs(want))
    worst = (d / gate).max()
    j = np.unravel_index(np.argmax(d / gate), d.shape)
    print(f"{what} {dtype}: max |device - oracle| / gate = {worst:.3e} at (time, drone, component) {j}")
    assert worst < 1.0, (what, j, got[j], want[j])


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_traj_eval_on_333_drones_of_22_tables_matches_each_drones_own_oracle(tables, dtype):
    """The device image of the tables (de-duplication, blocks by piece count, piece-major ids, the packed tinfo, the affine tag) read by
    k_traj_eval: every drone at every edge time against the oracle object of that drone."""
    env = make_env(dtype, E333, D333)
    env.set_trajectories([tables.lobjs[n] for n in tables.names])
    got = device_desired(env, tables.ts)
    env.close()
    assert_desired(got, tables.want, dtype, tables.scale, "333 drones")


def test_traj_eval_on_a_65535_piece_table():
    """The piece-count limit through mds_set_trajectory_segments itself: one Compound drone of 65535 Wait rows (nseg | compound << 16
    fills all 16 bits) among 63 one-piece drones, first piece, last piece and past the end."""
    import ctypes as C
    from multidronesim_amd import _capi as capi
    from multidronesim_amd._device import stream_ptr
    n, big = 64, 65535
    at = 17                                         # the big table sits in the middle of a wave
    counts = np.ones(n, dtype=np.int64)
    counts[at] = big
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    total = int(off[-1])
    segs = np.zeros((total, capi.SEG_DIM))
    segs[:, 0] = 3.0
    segs[:, 27] = segs[:, 31] = segs[:, 35] = 1.0
    k = np.arange(big)
    rows = slice(off[at], off[at + 1])
    segs[rows, 1], segs[rows, 2] = 0.5 * k, 0.5 * (k + 1)
    segs[rows, 3], segs[rows, 4], segs[rows, 5], segs[rows, 6] = 0.001 * k, -1.0 - 1e-5 * k, 2.0, 1e-4 * k
    for i in range(n):
        if i != at:
            segs[off[i], 2] = 1.0
            segs[off[i], 3:7] = [10.0 + (i % 7), float(i % 5), 1.0, 0.1 * (i % 3)]      # 35 distinct one-piece tables, the rest duplicates
    comp = np.zeros(n, dtype=np.int32)
    comp[at] = 1
    anchors = np.ascontiguousarray(segs[off[:-1], 3:6])
    env = make_env("float64", 1, n)
    capi.check(env._lib.mds_set_trajectory_segments(env._h, capi.as_double_ptr(segs), off.ctypes.data_as(C.POINTER(C.c_int32)),
                                                    comp.ctypes.data_as(C.POINTER(C.c_int32)), capi.as_double_ptr(anchors), C.c_int32(total),
                                                    C.c_void_p(stream_ptr(env.device))), "mds_set_trajectory_segments")
    ts = [0.25, 0.5 * (big - 1) + 0.25, 0.5 * big + 100.0]
    got = device_desired(env, ts)
    env.close()
    want = np.zeros((3, n, 11))
    for j, piece in enumerate([0, big - 1, big - 1]):
        for i in range(n):
            r = segs[off[i] + (piece if i == at else 0)]
            want[j, i, 0:3], want[j, i, 9] = r[3:6], r[6]
    np.testing.assert_array_equal(got, want)


def test_second_upload_and_mode_switches_on_one_handle(tables):
    """Tables X, then tables Y (another total, other piece counts, another duplicate pattern: tinfo is reused, segs freed and allocated
    again), then Lemniscate planes (mds_traj_eval answers with the planes), then X again -- each time the handle evaluates what was set last."""
    E, D = 3, 5
    X = ["compound3", "circle1", "zigzag300", "compound3", "rotate_compound2", "circle1_in_compound", "steps17", "wait", "circle1_again",
         "compound4", "zigzag300", "rotate_line", "line_s0", "compound3_mixed", "rotate_lemniscate"]
    Y = ["wait", "wait", "rotate_compound3", "steps17", "compound_past_end", "rotate_compound3", "lemniscate_far", "circle_far", "wait",
         "rotate_wait", "steps17", "line_short", "rotate_circle_far", "compound_past_end", "lemniscate"]
    ts = np.array([0.3, 4.81662479, 9.0, 77.0])
    env = make_env("float64", E, D)
    rng = np.random.default_rng(4)
    P = np.zeros((E, D, 7))
    P[..., 0], P[..., 1] = rng.uniform(0.5, 1.0, size=(E, D)), rng.uniform(0.5, 1.0, size=(E, D))
    P[..., 2:5], P[..., 5], P[..., 6] = rng.uniform(-2, 2, size=(E, D, 3)), 0.2, rng.uniform(-3, 3, size=(E, D))
    Pf = P.reshape(-1, 7)
    lem = np.stack([np.concatenate([np.asarray(x).reshape(E * D, -1) for x in O.lemniscate(float(t), Pf[:, 0], Pf[:, 1], Pf[:, 2:5], Pf[:, 5], Pf[:, 6])],
                                   axis=1) for t in ts])
    for what in ("X", "Y", "planes", "X"):
        if what == "planes":
            env.set_trajectories(P)
            want = lem
        else:
            names = X if what == "X" else Y
            env.set_trajectories([tables.lobjs[n] for n in names])
            want = TC.oracle_desired(tables.oobjs, names, ts)
        assert_desired(device_desired(env, ts), want, "float64", 1.0, what)
    env.close()


def one_step_actions(env, step, states, ts):
    """A fresh set_state per time, one fused step, the unclipped controller RPM it returns -> [nt, n, 4]."""
    out = []
    for st, t in zip(states, ts):
        env.set_state(st)
        _, act = step(float(t), return_action=True)
        out.append(act.double().cpu().numpy().reshape(env.n, 4))
    return np.stack(out)


def test_step_geometric_on_segment_tables_one_step_at_the_desired_state(tables):
    """TrajLocal<float>::eval on the device through k_step_traj: at each of the 39 times every drone is put near its desired state and one
    mds_step_geometric returns the controller's RPM, compared with O.geometric_compute on the same observation and the oracle's float64
    desired state.  No loop, so nothing absorbs a wrong feed-forward term.
    Gate: G_op + 4 P = 2e-6 + 4 x 2.10e-7 = 2.84e-6 relative RPM (TC.GEO_GATE; G_op: the fp32 gate of test_geometric_compute_golden,
    P: what the host build's fp32 desired state moves the oracle's RPM by, tests/test_traj_tables_cpu.py)."""
    env = make_env("float32", E333, D333)
    env.set_trajectories([tables.lobjs[n] for n in tables.names])
    states = TC.near_states(tables.want, tables.anchors, **TC.GEO_STATES)
    obs = TC.exact_obs(states)
    keep = ~TC.geometric_saturates(obs, tables.want)
    assert keep.mean() >= 0.95 and keep.mean(axis=0).min() >= 0.80
    ref = TC.geometric_rpm(obs, tables.want)
    got = one_step_actions(env, env.step_geometric, states, tables.ts)
    env.close()
    rel = np.abs(got / ref - 1).max(axis=-1)
    j = np.unravel_index(np.argmax(np.where(keep, rel, 0)), rel.shape)
    print(f"step_geometric on tables: max relative RPM error {rel[keep].max():.3e} at (time, drone) {j} ({tables.names[j[1]]}), gate {TC.GEO_GATE:.3e}")
    assert rel[keep].max() < TC.GEO_GATE


def test_step_lqr_on_segment_tables_one_step_at_the_desired_state(tables):
    """The same through k_step_lqr (linear in position, velocity, yaw and yaw rate), against O.lqr12_compute with the gain the library's
    LQRController solved.  Metric and G_op are those of test_lqr12_golden's fp32 action check: motor thrusts (rpm^2) relative to the largest
    reference thrust, 20 x 3e-5; gate G_op + 4 P = 6e-4 + 4 x 1.60e-6 (TC.LQR_GATE).  The states sit closer to the desired state than for the
    geometric controller: this controller's gains (12 N / m in z, 0.036 N m / rad) reach a motor limit from 5 cm or 0.08 rad away."""
    from multidronesim_amd.control import LQRController
    from multidronesim_amd.model import LinearizedModel
    env = make_env("float32", E333, D333)
    ctrl = LQRController(env, LinearizedModel(env))
    K = np.asarray(ctrl.K, dtype=np.float64).reshape(4, 12)
    np.testing.assert_allclose(K, O.lqr12_gain(), rtol=1e-7, atol=1e-9)
    env.set_trajectories([tables.lobjs[n] for n in tables.names])
    states = TC.near_states(tables.want, tables.anchors, **TC.LQR_STATES)
    obs = TC.exact_obs(states)
    keep = ~TC.lqr_saturates(obs, tables.want, K)
    assert keep.mean() >= 0.95 and keep.mean(axis=0).min() >= 0.80
    ref = TC.lqr_rpm(obs, tables.want, K)
    got = one_step_actions(env, env.step_lqr, states, tables.ts)
    env.close()
    rel = TC.thrust_error(got, ref, keep)
    j = np.unravel_index(np.argmax(np.where(keep, rel, 0)), rel.shape)
    print(f"step_lqr on tables: max thrust error / max thrust {rel[keep].max():.3e} at (time, drone) {j} ({tables.names[j[1]]}), gate {TC.LQR_GATE:.3e}")
    assert rel[keep].max() < TC.LQR_GATE

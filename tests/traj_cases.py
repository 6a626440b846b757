"""The drone set and the time sets of the segment-table tests (tests/test_traj_tables_cpu.py, tests/test_gpu_trajectories.py):
333 drones on 22 trajectory objects, built from the same constructor arguments for the library classes and for the float64
oracle classes (oracle/np_trajectories.py), like ``trajectory_cases`` of tests/golden/mint_golden.py.

What the set is shaped to reach in the image builder (csrc/mds_traj_image.hpp):
  * piece counts 1, 2, 3, 4, 17 and 300; distinct tables first appear with 3, 1, 3, 4, 1, 2, 3 pieces, so the blocks of 3 and of 1
    open, pause and reopen (rank and stride of a block grow while other blocks are being filled);
  * the same object at drones i and i + 5, equal rows from distinct objects (``circle1`` / ``circle1_again``), and equal rows with
    different compound flags (``circle1`` / ``circle1_in_compound``: same storage, different values past the end);
  * 333 drones: no multiple of a wave (64) or of a block (256)."""
import types

import numpy as np

N_DRONES = 333
FAR = np.array([4000.0, -3000.0, 120.0])
NAMES = ("compound3", "circle1", "compound3_mixed", "compound4", "wait", "rotate_compound2", "rotate_compound3", "circle1_in_compound",
         "steps17", "zigzag300", "lemniscate_far", "circle_far", "rotate_line", "line_s0", "line_short", "rotate_lemniscate",
         "circle1_again", "lemniscate", "rotate_circle_far", "line_long", "compound_past_end", "rotate_wait")


def library_classes():
    import multidronesim_amd.trajectories as TR
    return types.SimpleNamespace(Lemniscate=TR.Lemniscate, Circle=TR.CircleTrajectory, Line=TR.LineTrajectory, Wait=TR.WaitTrajectory,
                                 Compound=TR.CompoundTrajectory, Rotate=TR.RotateTrajectory)


def oracle_classes():
    from oracle import np_trajectories as NT
    return types.SimpleNamespace(Lemniscate=NT.Lemniscate, Circle=NT.Circle, Line=NT.Line, Wait=NT.Wait, Compound=NT.Compound, Rotate=NT.Rotate)


def _rot(rpy):
    from scipy.spatial.transform import Rotation as Rot
    return Rot.from_euler("xyz", rpy).as_matrix()


def table_objects(T):
    """name -> trajectory object, in the order in which the drones first use them."""
    R1, R2 = _rot([0.2, -0.3, 0.9]), _rot([-0.15, 0.25, -2.1])
    a, b, c = np.array([0.0, 0.0, 0.5]), np.array([1.5, -0.5, 1.0]), np.array([1.5, 2.0, 1.0])
    d = np.array([-2.0, 1.0, 0.8])
    zig = []                      # 300 pieces: 150 short Lines (the short-distance branch) with a Wait after each
    p = d.copy()
    for k in range(150):
        q = p + 0.05 * np.array([np.cos(0.7 * k), np.sin(0.7 * k), 0.3 * np.cos(1.3 * k)])
        zig += [T.Line(start=p, end=q, speed=0.4), T.Wait(position=q, duration=0.05 + 0.01 * (k % 3), yaw=0.01 * k)]
        p = q
    steps = []                    # 17 pieces
    p = c.copy()
    for k in range(8):
        q = p + np.array([0.3, -0.2, 0.1]) * (1 if k % 2 == 0 else -1) + np.array([0.0, 0.1, 0.0])
        steps += [T.Line(start=p, end=q, speed=0.5, s0=0.0, sf=0.0), T.Circle(r=0.2, v=0.3, center=q - np.array([0.2, 0, 0]), yaw_rate=0.2, duration=0.6)]
        p = q
    steps.append(T.Wait(position=p, duration=0.4, yaw=-0.3))
    circle1 = T.Circle(r=0.7, v=0.5, center=np.array([0.3, 0.2, 0.9]), yaw_rate=0.35, revolutions=1)
    line_s0 = T.Line(start=b, end=c + np.array([0, 4.0, 0]), speed=1.0, s0=0.3, sf=0.2)
    return {
        "compound3": T.Compound([T.Line(start=a, end=b, speed=.5), T.Wait(duration=1, position=b, yaw=0.2),
                                 T.Circle(r=0.3, v=0.4, center=b - np.array([0.3, 0, 0]), yaw_rate=0.3)]),                      # 3
        "circle1": circle1,                                                                                                 # 1
        "compound3_mixed": T.Compound([T.Wait(position=a, duration=0.5, yaw=0.1), T.Lemniscate(a=0.5, omega=0.8, center=a, yaw_rate=0.2),
                                       T.Circle(r=0.5, v=0.5, center=a)]),                                                   # 3
        "compound4": T.Compound([T.Line(start=a, end=b, speed=.5), T.Wait(duration=1, position=b),
                                 T.Line(start=b, end=c, speed=1), T.Line(start=c, end=b, speed=1)]),                          # 4
        "wait": T.Wait(position=np.array([0.3, 0.4, 0.5]), duration=2.0, yaw=0.6),                                           # 1
        "rotate_compound2": T.Rotate(T.Compound([T.Line(start=a, end=b, speed=.7), T.Circle(r=0.4, v=0.3, center=b)]), R1, b),  # 2
        "rotate_compound3": T.Rotate(T.Compound([T.Wait(position=d, duration=0.7, yaw=-0.4), T.Line(start=d, end=a, speed=0.8, sf=0.3),
                                                 T.Lemniscate(a=0.4, omega=0.7, center=a, yaw_rate=0.1, phase_shift=0.3)]), R2, d),  # 3
        "circle1_in_compound": T.Compound([circle1]),
        "steps17": T.Compound(steps),
        "zigzag300": T.Compound(zig),
        "lemniscate_far": T.Lemniscate(a=0.6, omega=0.8, center=FAR, yaw_rate=0.15, phase_shift=-0.7),
        "circle_far": T.Circle(r=0.9, v=0.6, center=FAR, yaw_rate=-0.25),
        "rotate_line": T.Rotate(T.Line(start=a, end=b + np.array([3.0, 0, 0]), speed=0.5), R2, np.array([0.5, 0.5, 0.5])),
        "line_s0": line_s0,
        "line_short": T.Line(start=a, end=a + np.array([0.1, 0.05, 0.0]), speed=1.0),
        "rotate_lemniscate": T.Rotate(T.Lemniscate(a=0.5, omega=0.8, center=np.array([0, 0, .5]), yaw_rate=0.3, phase_shift=0.4), R1,
                                      np.array([0.1, 0.2, 0.5])),
        "circle1_again": T.Circle(r=0.7, v=0.5, center=np.array([0.3, 0.2, 0.9]), yaw_rate=0.35, revolutions=1),
        "lemniscate": T.Lemniscate(a=0.4, omega=0.6, center=np.array([-1.0, 0.5, 0.7]), yaw_rate=-0.2, phase_shift=1.1),
        "rotate_circle_far": T.Rotate(T.Circle(r=0.5, v=0.4, center=FAR, yaw_rate=0.1), R1, FAR + np.array([1.0, -2.0, 0.5])),
        "line_long": T.Line(start=a, end=b + np.array([3.0, 0, 0]), speed=0.5),
        "compound_past_end": T.Compound([T.Line(start=b, end=a, speed=0.6), T.Circle(r=0.3, v=0.5, center=a, yaw_rate=0.4, duration=1.3)]),
        "rotate_wait": T.Rotate(T.Wait(position=c, duration=1.0, yaw=1.2), R2, a),
    }


def drone_names():
    """Which object each of the 333 drones follows: the 22 in order, then the same object at drones i and i + 5 (22 and 27, 24 and 29),
    then a fixed shuffle (stride 7 is coprime to 22, so duplicates are never neighbours)."""
    names = list(NAMES)
    out = list(names) + ["line_s0", "wait", "zigzag300", "compound3", "steps17", "line_s0", "circle1", "zigzag300"]
    k = 0
    while len(out) < N_DRONES:
        out.append(names[(7 * k + 3) % len(names)])
        k += 1
    return out


def drones(T):
    """-> (objects {name: trajectory}, names [333]); ``[objects[n] for n in names]`` is what set_trajectories takes."""
    objs = table_objects(T)
    assert tuple(objs) == NAMES
    return objs, drone_names()


def flatten(objs, names):
    """The library objects' rows as mds_set_trajectory_segments takes them -> (segs [total, 40], offsets [n + 1], compound [n], anchors [n, 3])."""
    rows, offsets, compound, anchors = [], [0], [], []
    for nm in names:
        r, c = objs[nm]._segments()
        rows.append(r)
        offsets.append(offsets[-1] + r.shape[0])
        compound.append(1 if c else 0)
        anchors.append(objs[nm].anchor())
    return (np.ascontiguousarray(np.concatenate(rows, axis=0), dtype=np.float64), np.ascontiguousarray(offsets, dtype=np.int32),
            np.ascontiguousarray(compound, dtype=np.int32), np.ascontiguousarray(anchors, dtype=np.float64))


def _around(x):
    return [np.nextafter(x, -np.inf), x, np.nextafter(x, np.inf)]


def _oracle_lines(tr, t0=0.0):
    """(start time, Line) of every Line piece under an oracle object."""
    from oracle import np_trajectories as NT
    if isinstance(tr, NT.Line):
        return [(t0, tr)]
    if isinstance(tr, NT.Rotate):
        return _oracle_lines(tr.tr, t0)
    if isinstance(tr, NT.Compound):
        out, starts = [], np.concatenate([[0.0], tr.times[:-1]])
        for s, piece in zip(starts, tr.trajs):
            out += _oracle_lines(piece, t0 + s)
        return out
    return []


def _piece_ends(tr):
    from oracle import np_trajectories as NT
    if isinstance(tr, NT.Rotate):
        return _piece_ends(tr.tr)
    return list(tr.times) if isinstance(tr, NT.Compound) else [tr.get_total_time()]


def times_full(oobjs):
    """Every edge of every object (CPU tests): 0, -0.25, each cumulative piece end and each Line phase switch with the values one ulp
    either side, T, T (1 - 1e-9), 50 T + 0.123 per object, 1e4 + 0.37, and 25 interior times per object."""
    ts = [0.0, -0.25, 1.0e4 + 0.37]
    for tr in oobjs.values():
        T = tr.get_total_time()
        ts += [T, T * (1 - 1e-9), 50 * T + 0.123] + list(np.linspace(0, 1.25 * T, 25))
        for e in _piece_ends(tr):
            ts += _around(e)
        for s, ln in _oracle_lines(tr):
            for x in (ln.ti, ln.ti + ln.tm, ln.total_time):
                ts += _around(s + x)
    return np.unique(np.array(ts, dtype=np.float64))


def times_gpu(oobjs):
    """The 39 of them that the GPU tests launch (one launch per time, every drone at every time): the edges of one object per code path."""
    def ends(name):
        return _piece_ends(oobjs[name])
    ts = [0.0, -0.25, 1.0e4 + 0.37]
    c3 = ends("compound3")
    for e in c3:                                            # both interior boundaries and the end of a 3-piece Compound
        ts += _around(e)
    ts += _around(ends("compound4")[2])
    z = ends("zigzag300")
    ts += [z[0], z[150]] + _around(z[298])                  # the last interior boundary of the 300-piece table
    ts += _around(ends("steps17")[8])
    ln = oobjs["line_s0"]
    for x in (ln.ti, ln.ti + ln.tm, ln.total_time):         # the three phase switches of a bare Line
        ts += _around(x)
    T1 = oobjs["circle1"].get_total_time()                  # bare Circle and Compound([Circle]) part ways here
    ts += _around(T1) + [T1 * (1 - 1e-9), 50 * T1 + 0.123, oobjs["rotate_lemniscate"].get_total_time(), 50 * c3[-1] + 0.123]
    ts = np.array(ts, dtype=np.float64)
    assert len(ts) <= 40 and len(np.unique(ts)) == len(ts), (len(ts), len(np.unique(ts)))
    return ts


def oracle_desired(oobjs, names, ts):
    """-> [nt, n, 11] float64: every drone's own oracle object at every time (pos3 vel3 acc3 yaw yaw_rate)."""
    per = {}
    for nm in set(names):
        tr = oobjs[nm]
        per[nm] = np.array([np.hstack([np.asarray(x, dtype=np.float64) * np.ones(np.size(x)) for x in tr(float(t))]) for t in ts])
    return np.stack([per[nm] for nm in names], axis=1)


def max_phase_rate(tr):
    """Largest |d phase / dt| of an oracle object's periodic pieces (omega, v / r, yaw rates): |phase| <= rate * |t|."""
    from oracle import np_trajectories as NT
    if isinstance(tr, NT.Rotate):
        return max_phase_rate(tr.tr)
    if isinstance(tr, NT.Compound):
        return max(max_phase_rate(p) for p in tr.trajs)
    if isinstance(tr, NT.Lemniscate):
        return max(abs(tr.p[1]), abs(tr.p[3]))
    if isinstance(tr, NT.Circle):
        return max(abs(tr.v / tr.r), abs(tr.yr))
    return 0.0


def f64_gate_scale(oobjs, names, ts):
    """[nt, n] factor on the float64 gate: max(1, |phase| 2^-52 1e3) with |phase| <= max_phase_rate * |t|."""
    rate = np.array([max_phase_rate(oobjs[nm]) for nm in names])
    return np.maximum(1.0, np.abs(np.asarray(ts))[:, None] * rate[None, :] * 2.0 ** -52 * 1e3)


def wrap(a):
    return (np.asarray(a) + np.pi) % (2 * np.pi) - np.pi


# ---- one control step at the desired state (the fp32 evaluator seen through the controllers) ---------------------------------------------
def f32(x):
    return np.asarray(x, dtype=np.float64).astype(np.float32).astype(np.float64)


def near_states(want, origin, seed, dp=0.05, dv=0.3, tilt=0.08, dyaw=0.15, dw=0.3):
    """World-frame states [nt, n, 13] near the desired state want [nt, n, 11], from a fixed seed: position within dp, velocity within dv,
    roll / pitch within tilt, yaw within dyaw of the desired yaw, body rates within dw of (0, 0, desired yaw rate).  Every value is one an fp32 handle stores exactly
    (position: fp32 origin + fp32 offset), so the oracle and the kernel start from the same numbers."""
    from oracle import np_oracle as O
    rng = np.random.default_rng(seed)
    nt, n = want.shape[:2]
    org = f32(origin)[None]
    s = np.zeros((nt, n, 13))
    s[..., 0:3] = org + f32(want[..., 0:3] + rng.uniform(-dp, dp, size=(nt, n, 3)) - org)
    rpy = np.concatenate([rng.uniform(-tilt, tilt, size=(nt, n, 2)), wrap(want[..., 9:10] + rng.uniform(-dyaw, dyaw, size=(nt, n, 1)))], axis=-1)
    s[..., 3:7] = f32(O.quat_from_euler_bullet(rpy.reshape(-1, 3)).reshape(nt, n, 4))
    s[..., 7:10] = f32(want[..., 3:6] + rng.uniform(-dv, dv, size=(nt, n, 3)))
    rates = rng.uniform(-dw, dw, size=(nt, n, 3))
    rates[..., 2] += want[..., 10]
    s[..., 10:13] = f32(rates)
    return s


def exact_obs(state):
    """The observation [.., 20] of a state [.., 13] as the kernels pack it (the rotation of q / |q|; ang_v = R w; no RPM echo yet)."""
    from oracle import np_oracle as O
    x = np.asarray(state, dtype=np.float64)
    q = x[..., 3:7]
    R = O.quat_to_rotmat_bullet(q)
    rpy = O.euler_from_quat_bullet(q / O.norm(q)[..., None])
    return np.concatenate([x[..., 0:3], q, rpy, x[..., 7:10], O.matvec(R, x[..., 10:13]), np.zeros(x.shape[:-1] + (4,))], axis=-1)


def geometric_rpm(obs, des):
    from oracle import np_oracle as O
    return O.geometric_compute(obs, des[..., 0:3], des[..., 3:6], des[..., 6:9], des[..., 9], des[..., 10])


def lqr_rpm(obs, des, K):
    from oracle import np_oracle as O
    return O.lqr12_compute(obs, des[..., 0:3], des[..., 3:6], des[..., 9], des[..., 10], K)[0]


def geometric_saturates(obs, des):
    """[..] bool, from the oracle alone: the tilt clamp is active (the answer changes when the clamp is moved out to 89 degrees), or a
    motor sits at one of the mixer's thrust limits (which is also where a thrust clipped at 0 ends up)."""
    from oracle import np_oracle as O
    rpm = geometric_rpm(obs, des)
    free = O.geometric_compute(obs, des[..., 0:3], des[..., 3:6], des[..., 6:9], des[..., 9], des[..., 10], gains=dict(max_tilt=89 * np.pi / 180))
    return (np.abs(rpm - free).max(axis=-1) > 0) | motor_at_limit(rpm)


def motor_at_limit(rpm):
    from oracle import np_oracle as O
    lo, hi = 9440.3, np.sqrt(O.CF2P.MAX_THRUST / O.CF2P.KF)
    return (rpm <= lo * (1 + 1e-9)).any(axis=-1) | (rpm >= hi * (1 - 1e-9)).any(axis=-1)


def lqr_saturates(obs, des, K):
    """[..] bool: a motor at a limit (incl. the thrust clipped at 0), or the yaw error within 0.1 of +-pi (where its wrap flips sign)."""
    rpm = lqr_rpm(obs, des, K)
    dy = np.abs(wrap(obs[..., 9] - des[..., 9]))
    return motor_at_limit(rpm) | (dy > np.pi - 0.1)


# components a planted error goes into, per controller, with the size the resolving-power condition plants
PLANT = {"p": (slice(0, 3), 1e-3), "v": (slice(3, 6), 1e-3), "a": (slice(6, 9), 1e-2), "yaw": (slice(9, 10), 1e-3), "yaw_rate": (slice(10, 11), 1e-2)}


def produced_components(oobjs, names, want):
    """[nt, n, 11] bool: the components the drone's segment kind actually produces (a component that is zero for a drone at every time
    of the set, such as a Wait's velocity or a Line's yaw, is not one)."""
    return np.broadcast_to((np.abs(want) > 0).any(axis=0, keepdims=True), want.shape)


# The states and gates of the one-step tests (tests/test_gpu_trajectories.py); P is measured on the CPU by tests/test_traj_tables_cpu.py
# (test_one_step_conditions_hold_on_the_oracle_alone), which also holds the recorded values to what it measures.
GEO_STATES = dict(seed=7, dp=0.05, dv=0.3, tilt=0.08, dyaw=0.15, dw=0.3)
LQR_STATES = dict(seed=8, dp=np.array([0.02, 0.02, 0.002]), dv=np.array([0.03, 0.03, 0.008]), tilt=0.01, dyaw=0.03, dw=0.05)
GEO_G_OP, GEO_P = 2e-6, 2.10e-7          # relative RPM: the fp32 gate of test_geometric_compute_golden; measured P
LQR_G_OP, LQR_P = 20 * 3e-5, 1.60e-6     # thrust / largest thrust: the fp32 action gate of test_lqr12_golden; measured P
GEO_GATE, LQR_GATE = GEO_G_OP + 4 * GEO_P, LQR_G_OP + 4 * LQR_P


def thrust_error(rpm, ref, keep):
    """test_lqr12_golden's action metric: |rpm^2 - ref^2| over the largest reference rpm^2 among the compared cases -> [..]"""
    return (np.abs(rpm ** 2 - ref ** 2) / (ref[keep] ** 2).max()).max(axis=-1)

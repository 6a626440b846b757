"""The phase table of the whole-rollout loop on the GPU (k_rollout_geometric_y0p / k_lemniscate_phase_table; include/mds.h "THE PHASE
TABLE"): a yaw-free handle whose (omega, phase_shift) repeat every 64 drones reads sin / cos of the Lemniscate phase from a table of
its own instead of computing them per drone and step.

  * the flag (mds_traj_phase_periodic) follows the upload, and only yaw-free Lemniscate handles launch the table kernel;
  * table on against table off (mds_set_traj_phase_table), byte for byte: every step's rows through the [T, n, 20] log, the rows
    rewritten in place, the last step's only, get_state() and the last-RPM planes -- 120 steps from t0 = 37.31 s (the double reduction
    of the phase is not the identity there) in launches of 50 + 50 + 20, from perturbed states, on 1 drone, 72 (a second wave of 8
    lanes), 264 (a second workgroup, ragged) and 260 drones in envs of 4; one flight across a refill of the table; two calls on one
    handle, the second continuing the first's time; a launch longer than the table; a flight long enough to fill the whole table and
    run off it; a call captured into a hipGraph (it does not read the table) among eager ones;
  * a ragged shard against the same drones inside a wave-aligned batch, sentinel rows untouched;
  * two handles on two streams, each with a table of its own;
  * the oracle, at the gate tests/test_gpu_yaw_free.py holds the same loop to (1e-5 on the 16 state columns in fp32).
All shapes are tiny: each test is milliseconds of device time."""
import numpy as np
import pytest

from tests import helpers as H

pytestmark = pytest.mark.gpu

T0, STEPS, DT = 37.31, 120, 0.01
TAB_ROWS = 2048                           # kPhaseTabRows (csrc/mds_api.hip)
SENTINEL = 12345.0


@pytest.fixture(scope="module")
def mds():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no HIP device: -m gpu tests need a real MI355X (there is no CPU fallback)")
    import multidronesim_amd
    multidronesim_amd.load_library()
    from multidronesim_amd.envs.CtrlAviary import CtrlAviary, DroneModel, Physics
    import types
    return types.SimpleNamespace(CtrlAviary=CtrlAviary, DroneModel=DroneModel, Physics=Physics, torch=torch)


def setup(E, D, omega=1.5):
    """E envs of D drones, per-slot phases 2 pi d / (D + 0.25), the same in every env (the config-3 generator of SURVEY 8d)."""
    return H.c2_setup(E, D, phase="c3", omega=omega)


def perturbed(state, seed=5):
    """A state away from every exact zero (drone i gets the same offsets whatever the size of the batch it flies in)."""
    rng = np.random.default_rng(seed)
    s = np.array(state, dtype=np.float64).reshape(-1, 13)
    d = rng.uniform(-1.0, 1.0, (512, 13))[:s.shape[0]]
    s[:, 0:3] += 0.05 * d[:, 0:3]
    q = s[:, 3:7] + 0.08 * d[:, 3:7]
    s[:, 3:7] = q / np.linalg.norm(q, axis=1, keepdims=True)
    s[:, 7:10] = 0.3 * d[:, 7:10]
    s[:, 10:13] = 0.4 * d[:, 10:13]
    return s


def make(mds, E, D, table=True, P=None, xyz=None, rpy=None, perturb=True, omega=1.5):
    x0, r0, P0 = setup(E, D, omega)
    xyz, rpy = (x0 if xyz is None else xyz), (r0 if rpy is None else rpy)
    env = mds.CtrlAviary(drone_model=mds.DroneModel.CF2P, num_drones=D, initial_xyzs=xyz, initial_rpys=rpy, physics=mds.Physics.DYN,
                         pyb_freq=100, ctrl_freq=100, num_envs=E, dtype="float32", track_last_rpm=True)
    env.set_trajectories(P0 if P is None else P)
    env.set_traj_phase_table(table)
    env.set_rollout_form(2, 50)
    env.step(mds.torch.zeros((E, D, 4), dtype=env.dtype, device=env.device))
    if perturb:
        env.set_state(perturbed(env.get_state()))
    return env


def after(t, k):
    """t after k additions of the control period, as the library's loops advance it."""
    for _ in range(k):
        t += DT
    return t


def raw(t):
    return t.detach().contiguous().cpu().numpy().copy().view(np.uint8)


def fly(mds, E, D, table, dest, steps=STEPS, t0=T0, expect_table=None, **kw):
    """One flight on a fresh handle -> the bytes of (rows, state, rows with the last-RPM planes read back)."""
    env = make(mds, E, D, table, **kw)
    if dest == "log":
        _, rows = env.rollout_geometric_fused(t0, steps, log=True)
    else:
        rows = env.rollout_geometric(t0, steps, obs_every_step=dest == "in_place")
        assert env.last_rollout_form() == 2
    assert env.last_rollout_phase_table() == (table if expect_table is None else expect_table)
    out = [raw(rows), env.get_state().tobytes(), raw(env._computeObs())]
    env.close()
    return out


SHAPES = [(1, 1), (9, 8), (33, 8), (65, 4)]


@pytest.mark.parametrize("dest", ["log", "in_place", "last"])
@pytest.mark.parametrize("shape", SHAPES)
def test_table_on_equals_table_off_to_the_byte(mds, shape, dest):
    E, D = shape
    on, off = fly(mds, E, D, True, dest), fly(mds, E, D, False, dest)
    rows = on[0].view(np.float32).reshape(-1, 20)
    assert rows.shape[0] == (STEPS if dest == "log" else 1) * E * D
    assert np.isfinite(rows).all() and (rows[:, 16:] > 0).all() and np.abs(rows[:, 10:16]).min() > 0      # rows were written, none trivial
    for a, b, what in zip(on, off, ("rows", "state", "last RPM")):
        assert (a == b).all() if isinstance(a, np.ndarray) else a == b, (shape, dest, what)


def test_a_flight_across_a_refill(mds):
    """TAB_ROWS + 70 steps in launches of 50 at n = 72: the launches run off the end of the filled rows and the table is filled anew."""
    for dest in ("in_place", "last"):
        on, off = fly(mds, 9, 8, True, dest, steps=TAB_ROWS + 70), fly(mds, 9, 8, False, dest, steps=TAB_ROWS + 70)
        assert np.isfinite(on[0].view(np.float32)).all()
        assert (on[0] == off[0]).all() and on[1] == off[1] and (on[2] == off[2]).all(), dest


def test_a_long_flight_reaches_the_whole_table_and_refills_it(mds):
    """5200 steps in launches of 50 at n = 72: the fills of a continuing flight double (50, 100, ... 1600 rows: 3150 steps), the next one
    is the whole table (2048 rows, 40 launches), and the flight runs off its end as well."""
    steps = 5200
    assert steps > 50 * (1 + 2 + 4 + 8 + 16 + 32) + (TAB_ROWS // 50) * 50
    on, off = fly(mds, 9, 8, True, "in_place", steps=steps), fly(mds, 9, 8, False, "in_place", steps=steps)
    assert np.isfinite(on[0].view(np.float32)).all()
    assert (on[0] == off[0]).all() and on[1] == off[1] and (on[2] == off[2]).all()


def test_a_captured_launch_does_not_read_the_table(mds):
    """mds_rollout_geometric may be captured into a hipGraph and replayed (include/mds.h, Conventions).  What the table's rows hold is
    host bookkeeping of eager enqueues, so a launch under capture computes the phase in the kernel and leaves the bookkeeping alone:
    an eager flight, a captured call that continues it, an eager call elsewhere in time (it overwrites the rows the flight left), a
    new upload of the same trajectories, then the replay -- against the same four calls flown eagerly with the table off, byte for
    byte; and an eager call that continues where the flight ended before the capture still reads rows that were written."""
    torch = mds.torch
    t1 = after(T0, 70)
    _, _, P = setup(9, 8)
    off = make(mds, 9, 8, False)
    off.rollout_geometric(T0, 70, obs_every_step=True)
    off.rollout_geometric(5.0, 30, obs_every_step=True)
    off.set_trajectories(P)
    want_rows = raw(off.rollout_geometric(t1, 50, obs_every_step=True))
    want_state = off.get_state().tobytes()
    off.close()
    on = make(mds, 9, 8, True)
    on.rollout_geometric(T0, 70, obs_every_step=True)
    assert on.last_rollout_phase_table()
    state_before = on.get_state().tobytes()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            on.rollout_geometric(t1, 50, obs_every_step=True)
    torch.cuda.current_stream().wait_stream(side)
    assert not on.last_rollout_phase_table()
    assert on.get_state().tobytes() == state_before                         # capturing ran nothing
    on.rollout_geometric(5.0, 30, obs_every_step=True)
    assert on.last_rollout_phase_table()
    on.set_trajectories(P)
    g.replay()
    torch.cuda.synchronize()
    assert (raw(on._obs) == want_rows).all() and on.get_state().tobytes() == want_state
    on.close()
    # the other order: a capture first, then the eager call that starts where an eager flight ended
    got = []
    for table in (True, False):
        env = make(mds, 9, 8, table)
        env.rollout_geometric(T0, 70, obs_every_step=True)
        if table:
            g2 = torch.cuda.CUDAGraph()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                with torch.cuda.graph(g2, stream=side):
                    env.rollout_geometric(t1, 100, obs_every_step=True)     # never replayed
            torch.cuda.current_stream().wait_stream(side)
        got.append((raw(env.rollout_geometric(t1, 50, obs_every_step=True)), env.get_state().tobytes()))
        assert env.last_rollout_phase_table() == table
        env.close()
    assert (got[0][0] == got[1][0]).all() and got[0][1] == got[1][1]


def test_a_launch_longer_than_the_table_computes_the_phase(mds):
    on = fly(mds, 9, 8, True, "log", steps=TAB_ROWS + 1, expect_table=False)
    off = fly(mds, 9, 8, False, "log", steps=TAB_ROWS + 1)
    assert (on[0] == off[0]).all() and on[1] == off[1]


@pytest.mark.parametrize("continues", [True, False])
def test_two_consecutive_calls_on_one_handle(mds, continues):
    """The second call starts where the first ended: at that time to the bit (it reads on in the table), or at t0 + 70 dt as a caller
    that multiplies would pass it (another double: its rows are filled anew)."""
    t1 = after(T0, 70) if continues else T0 + 70 * DT
    assert continues or t1 != after(T0, 70)
    got = []
    for table in (True, False):
        env = make(mds, 9, 8, table)
        a = raw(env.rollout_geometric(T0, 70, obs_every_step=True))
        b = raw(env.rollout_geometric(t1, 50, obs_every_step=True))
        assert env.last_rollout_phase_table() == table
        got.append((a, b, env.get_state().tobytes()))
        env.close()
    assert (got[0][0] == got[1][0]).all() and (got[0][1] == got[1][1]).all() and got[0][2] == got[1][2]
    assert not (got[0][0] == got[0][1]).all()


def test_flag_follows_the_upload(mds):
    env = make(mds, 2, 8)
    assert env.traj_phase_periodic() and env.traj_yaw_free()                 # per-slot parameters, n = 16
    env.close()
    # n = 90, three distinct phases per env: drone 64 (slot 1) is not drone 0 (slot 0)
    xyz, rpy, P = setup(30, 3)
    env = make(mds, 30, 3)
    assert not env.traj_phase_periodic()
    env.rollout_geometric(T0, 60, obs_every_step=True)
    assert not env.last_rollout_phase_table()
    Pe = P.copy()
    Pe[..., 1], Pe[..., 6] = 1.25, 0.7                                       # all drones' (omega, phase_shift) equal
    env.set_trajectories(Pe)
    assert env.traj_phase_periodic()
    env.rollout_geometric(T0, 60, obs_every_step=True)
    assert env.last_rollout_phase_table()
    env.set_trajectories(P)                                                  # ... and back
    assert not env.traj_phase_periodic()
    env.rollout_geometric(T0, 60, obs_every_step=True)
    assert not env.last_rollout_phase_table()
    env.close()
    env = make(mds, 1, 3)
    assert env.traj_phase_periodic()
    env.close()
    # a periodic upload (n = 72) with row 64's omega changed by 1e-12: the same fp32 value, another double
    xyz, rpy, P = setup(9, 8)
    env = make(mds, 9, 8)
    assert env.traj_phase_periodic()
    Pq = P.copy()
    Pq[8, 0, 1] += 1e-12
    assert np.float32(Pq[8, 0, 1]) == np.float32(P[8, 0, 1])
    env.set_trajectories(Pq)
    assert not env.traj_phase_periodic()
    # a yaw rate anywhere: periodic, but no table launch
    Py = P.copy()
    Py[3, 5, 5] = 0.1
    env.set_trajectories(Py)
    assert env.traj_phase_periodic() and not env.traj_yaw_free()
    env.rollout_geometric(T0, 60, obs_every_step=True)
    assert not env.last_rollout_phase_table()
    # the specialisation switched off switches the table off as well
    env.set_trajectories(P)
    env.set_traj_specialisation(False)
    env.rollout_geometric(T0, 60, obs_every_step=True)
    assert env.traj_phase_periodic() and not env.last_rollout_phase_table()
    env.set_traj_specialisation(True)
    env.rollout_geometric(T0, 60, obs_every_step=True)
    assert env.last_rollout_phase_table()
    # segment tables clear it
    from multidronesim_amd import trajectories as TR
    env.set_trajectories([TR.CircleTrajectory(r=0.3, v=0.5, center=np.array([0.0, 0.0, 0.5])) for _ in range(72)])
    assert not env.traj_phase_periodic()
    assert np.isfinite(env.rollout_geometric(0.0, 5).double().cpu().numpy()).all()
    assert not env.last_rollout_phase_table()
    env.close()


def _fly_with_sentinels(mds, n, dest):
    """n drones of one env with equal (omega, phase_shift), the table on; two more rows allocated behind the last drone's."""
    torch = mds.torch
    xyz, rpy, P = setup(1, 320)
    P[..., 6] = 0.7
    env = make(mds, 1, n, True, P=P[:, :n].copy(), xyz=xyz[:, :n].copy(), rpy=rpy[:, :n].copy())
    assert env.traj_phase_periodic()
    obs = torch.full((n + 2, 20), SENTINEL, dtype=env.dtype, device=env.device)
    assert env._obs.shape == (1, n, 20) and env._obs.dtype == obs.dtype          # (the buffer the rollouts write through, as tests/test_gpu_whole_wave.py)
    env._obs = obs[:n].view(1, n, 20)
    log = None
    if dest == "log":
        log = torch.full((60 * n + 2, 20), SENTINEL, dtype=env.dtype, device=env.device)
        env.rollout_geometric_fused(T0, 60, log=True, log_out=log[:60 * n].view(60, 1, n, 20))
    else:
        env.rollout_geometric(T0, 60, obs_every_step=dest == "in_place")
    assert env.last_rollout_phase_table()
    torch.cuda.synchronize()
    tail = torch.cat([obs[n:]] + ([log[60 * n:]] if log is not None else [])).cpu().numpy()
    out = raw(obs[:n]).reshape(n, -1), (raw(log[:60 * n]).reshape(60, n, -1) if log is not None else None), env.get_state().reshape(n, 13), tail
    env.close()
    return out


@pytest.mark.parametrize("dest", ["in_place", "log", "last"])
def test_ragged_shard_equals_the_same_drones_inside_a_wave_aligned_batch(mds, dest):
    rows, log, state, tail = _fly_with_sentinels(mds, 259, dest)
    Rows, Log, State, Tail = _fly_with_sentinels(mds, 320, dest)
    assert np.isfinite(rows.view(np.float32)).all()
    assert (rows == Rows[:259]).all() and state.tobytes() == State[:259].tobytes()
    if log is not None:
        assert (log == Log[:, :259]).all() and (log[-1] == rows).all()
    assert (tail == SENTINEL).all() and (Tail == SENTINEL).all()


def test_two_handles_on_two_streams(mds):
    """Each handle has a table of its own (another omega); enqueued alternately on two streams, each equals its own table-off flight."""
    torch = mds.torch
    omegas = (1.5, 0.9)
    want = [fly(mds, 9, 8, False, "in_place", omega=w) for w in omegas]
    envs = [make(mds, 9, 8, True, omega=w) for w in omegas]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    t = T0
    for k0, ks in ((0, 50), (50, 50), (100, 20)):                            # the launches of one 120-step call, issued by hand
        for env, st in zip(envs, streams):
            with torch.cuda.stream(st):
                env.rollout_geometric(t, ks, obs_every_step=True)
                assert env.last_rollout_phase_table()
        t = after(t, ks)
    torch.cuda.synchronize()
    for env, w in zip(envs, want):
        assert (raw(env._obs) == w[0]).all() and env.get_state().tobytes() == w[1]
        env.close()
    assert not (want[0][0] == want[1][0]).all()


def test_table_flight_tracks_the_oracle(mds):
    E, D, steps, tol = 33, 8, 60, 1e-5
    xyz, rpy, P = setup(E, D)
    oobs, _ = H.oracle_closed_loop(xyz, rpy, P, steps)
    env = make(mds, E, D, True, perturb=False)
    v = env.rollout_geometric(0.0, steps, obs_every_step=True).double().cpu().numpy().reshape(-1, 20)
    assert env.last_rollout_phase_table()
    env.close()
    err = np.abs(v[:, :16] - oobs[:, :16]).max()
    print(f"float32, table on, {E} x {D}: max |state - oracle| after {steps} steps = {err:.3e} (gate {tol:g})")
    assert err < tol

"""The desired-state table of the whole-rollout loop on the GPU (k_rollout_geometric_y0d / k_lemniscate_phase_table<T, true>;
include/mds.h "THE DESIRED-STATE TABLE"): a yaw-free handle whose (a, omega, phase_shift) repeat every 64 drones reads what the
controller needs of the desired state from rows of 64 x 8 values instead of forming it per drone and step.

Wide rows on against off (mds_set_traj_desired_table: off is the table of sin / cos pairs), byte for byte in every step's rows, the
final state and the last-RPM planes:
  * 2 envs x 8 (one partial wave) and 65 envs x 2 (lanes wrap at 64, ragged last wave), through the [T, n, 20] log, the rows rewritten
    in place and the last step's only; 130 drones against the same drones inside a wave-aligned batch, sentinel rows untouched;
  * 16 drones over 2100 and 5200 steps in launches of 50: every refill of a continuing flight (50, 100, ... 1600 rows), the whole table
    and past its end;
  * two consecutive calls, the second continuing at the bit-equal time or at a foreign t0;
  * two handles on two streams;
  * the flag through uploads: one drone's a changed at a row >= 64 drops to the pair's table (the getters say 1 and 0), a yaw rate
    drops both -- the bits stay those of a flight without any table;
  * an eager flight, a captured continuing call, an upload and the replay;
  * the oracle over 60 steps, at the gate of tests/test_gpu_phase_table.py (1e-5 on the 16 state columns).
All shapes are tiny: each test is milliseconds of device time."""
import numpy as np
import pytest

from tests import helpers as H
from tests.test_gpu_phase_table import DT, SENTINEL, T0, TAB_ROWS, after, make as make_pt, mds, raw, setup  # noqa: F401  (mds: the fixture)

pytestmark = pytest.mark.gpu

STEPS = 120


def make(mds, E, D, wide=True, table=True, **kw):
    env = make_pt(mds, E, D, table, **kw)
    env.set_traj_desired_table(wide)
    return env


def fly(mds, E, D, wide, dest, steps=STEPS, t0=T0, table=True, **kw):
    """One flight on a fresh handle -> the bytes of (rows, state, rows with the last-RPM planes read back)."""
    env = make(mds, E, D, wide, table, **kw)
    assert env.traj_desired_periodic() and env.traj_phase_periodic()
    if dest == "log":
        _, rows = env.rollout_geometric_fused(t0, steps, log=True)
    else:
        rows = env.rollout_geometric(t0, steps, obs_every_step=dest == "in_place")
        assert env.last_rollout_form() == 2
    assert env.last_rollout_phase_table() == table and env.last_rollout_desired_table() == (wide and table)
    out = [raw(rows), env.get_state().tobytes(), raw(env._computeObs())]
    env.close()
    return out


def same(a, b):
    return all((x == y).all() if isinstance(x, np.ndarray) else x == y for x, y in zip(a, b))


@pytest.mark.parametrize("dest", ["log", "in_place", "last"])
@pytest.mark.parametrize("shape", [(2, 8), (65, 2)])
def test_wide_rows_on_equal_off_to_the_byte(mds, shape, dest):
    E, D = shape
    on, off, none = fly(mds, E, D, True, dest), fly(mds, E, D, False, dest), fly(mds, E, D, False, dest, table=False)
    rows = on[0].view(np.float32).reshape(-1, 20)
    assert rows.shape[0] == (STEPS if dest == "log" else 1) * E * D
    assert np.isfinite(rows).all() and (rows[:, 16:] > 0).all() and np.abs(rows[:, 10:16]).min() > 0      # rows were written, none trivial
    assert same(on, off) and same(on, none), (shape, dest)


def _fly_with_sentinels(mds, E, dest):
    """E envs of 2 drones, the wide rows on; two more rows allocated behind the last drone's."""
    torch = mds.torch
    n = 2 * E
    xyz, rpy, P = setup(160, 2)
    env = make(mds, E, 2, True, P=P[:E].copy(), xyz=xyz[:E].copy(), rpy=rpy[:E].copy())
    assert env.traj_desired_periodic()
    obs = torch.full((n + 2, 20), SENTINEL, dtype=env.dtype, device=env.device)
    assert env._obs.shape == (E, 2, 20) and env._obs.dtype == obs.dtype
    env._obs = obs[:n].view(E, 2, 20)
    log = None
    if dest == "log":
        log = torch.full((60 * n + 2, 20), SENTINEL, dtype=env.dtype, device=env.device)
        env.rollout_geometric_fused(T0, 60, log=True, log_out=log[:60 * n].view(60, E, 2, 20))
    else:
        env.rollout_geometric(T0, 60, obs_every_step=dest == "in_place")
    assert env.last_rollout_desired_table()
    torch.cuda.synchronize()
    tail = torch.cat([obs[n:]] + ([log[60 * n:]] if log is not None else [])).cpu().numpy()
    out = raw(obs[:n]).reshape(n, -1), (raw(log[:60 * n]).reshape(60, n, -1) if log is not None else None), env.get_state().reshape(n, 13), tail
    env.close()
    return out


@pytest.mark.parametrize("dest", ["in_place", "log", "last"])
def test_130_drones_equal_the_same_drones_inside_a_wave_aligned_batch(mds, dest):
    rows, log, state, tail = _fly_with_sentinels(mds, 65, dest)
    Rows, Log, State, Tail = _fly_with_sentinels(mds, 160, dest)
    assert np.isfinite(rows.view(np.float32)).all()
    assert (rows == Rows[:130]).all() and state.tobytes() == State[:130].tobytes()
    if log is not None:
        assert (log == Log[:, :130]).all() and (log[-1] == rows).all()
    assert (tail == SENTINEL).all() and (Tail == SENTINEL).all()


@pytest.mark.parametrize("steps", [2100, 5200])
def test_a_long_flight_across_every_refill(mds, steps):
    """Launches of 50 at n = 16: the fills of a continuing flight double (50, 100, ... 1600 rows: 3150 steps); the next one is the whole
    table (2048 rows), and the 5200-step flight runs off its end as well."""
    assert 5200 > 50 * (1 + 2 + 4 + 8 + 16 + 32) + (TAB_ROWS // 50) * 50
    on, off = fly(mds, 2, 8, True, "in_place", steps=steps), fly(mds, 2, 8, False, "in_place", steps=steps)
    assert np.isfinite(on[0].view(np.float32)).all()
    assert same(on, off)


@pytest.mark.parametrize("continues", [True, False])
def test_two_consecutive_calls_on_one_handle(mds, continues):
    t1 = after(T0, 70) if continues else T0 + 70 * DT
    assert continues or t1 != after(T0, 70)
    got = []
    for wide in (True, False):
        env = make(mds, 2, 8, wide)
        a = raw(env.rollout_geometric(T0, 70, obs_every_step=True))
        b = raw(env.rollout_geometric(t1, 50, obs_every_step=True))
        assert env.last_rollout_phase_table() and env.last_rollout_desired_table() == wide
        got.append((a, b, env.get_state().tobytes()))
        env.close()
    assert same(got[0], got[1])
    assert not (got[0][0] == got[0][1]).all()


def test_two_handles_on_two_streams(mds):
    """Each handle has a table of its own (another omega); enqueued alternately on two streams, each equals its own flight on the pairs."""
    torch = mds.torch
    omegas = (1.5, 0.9)
    want = [fly(mds, 9, 8, False, "in_place", omega=w) for w in omegas]
    envs = [make(mds, 9, 8, True, omega=w) for w in omegas]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    t = T0
    for ks in (50, 50, 20):                                                  # the launches of one 120-step call, issued by hand
        for env, st in zip(envs, streams):
            with torch.cuda.stream(st):
                env.rollout_geometric(t, ks, obs_every_step=True)
                assert env.last_rollout_desired_table()
        t = after(t, ks)
    torch.cuda.synchronize()
    for env, w in zip(envs, want):
        assert (raw(env._obs) == w[0]).all() and env.get_state().tobytes() == w[1]
        env.close()
    assert not (want[0][0] == want[1][0]).all()


def test_the_flag_follows_the_upload(mds):
    """n = 72: drone 64 is slot 0 of env 8.  Its a changed by one double ulp keeps the phases periodic and drops the wide rows; a yaw rate
    drops both tables.  Each flight against the same upload flown without any table."""
    _, _, P = setup(9, 8)
    Pa = P.copy()
    Pa[8, 0, 0] = np.nextafter(Pa[8, 0, 0], np.inf)
    Pb = P.copy()
    Pb[8, 0, 0] = 1.3                                                        # ... and by enough to show in the rows
    Py = P.copy()
    Py[3, 5, 5] = 0.1
    got = {}
    for table in (True, False):
        env = make(mds, 9, 8, True, table)
        assert env.traj_desired_periodic() and env.traj_phase_periodic()
        for name, Q, flags in (("P", P, (1, 1)), ("Pa", Pa, (1, 0)), ("Pb", Pb, (1, 0)), ("Py", Py, (0, 0)), ("P again", P, (1, 1))):
            env.set_trajectories(Q)
            assert env.traj_desired_periodic() == (name not in ("Pa", "Pb")) and env.traj_phase_periodic()      # (the yaw rate is not the rule's)
            rows = raw(env.rollout_geometric(T0, 60, obs_every_step=True))
            if table:
                assert (int(env.last_rollout_phase_table()), int(env.last_rollout_desired_table())) == flags, name
            else:
                assert not env.last_rollout_phase_table() and not env.last_rollout_desired_table()
            got[name, table] = (rows, env.get_state().tobytes())
        env.close()
    for name in ("P", "Pa", "Pb", "Py", "P again"):
        assert same(got[name, True], got[name, False]), name
    # the first upload of a handle may be the one that does not qualify: the block then grows with the one that does
    env = make(mds, 9, 8, True, P=Pb)
    assert not env.traj_desired_periodic()
    env.rollout_geometric(T0, 60, obs_every_step=True)
    assert env.last_rollout_phase_table() and not env.last_rollout_desired_table()
    env.set_trajectories(P)
    env.rollout_geometric(after(T0, 60), 60, obs_every_step=True)
    assert env.last_rollout_desired_table()
    # the switches: the wide rows off falls back to the pairs, the pairs off switches both off
    env.set_traj_desired_table(False)
    env.rollout_geometric(T0, 10, obs_every_step=True)
    assert env.last_rollout_phase_table() and not env.last_rollout_desired_table()
    env.set_traj_desired_table(True)
    env.set_traj_phase_table(False)
    env.rollout_geometric(T0, 10, obs_every_step=True)
    assert not env.last_rollout_phase_table() and not env.last_rollout_desired_table()
    env.set_traj_phase_table(True)
    env.set_traj_specialisation(False)
    env.rollout_geometric(T0, 10, obs_every_step=True)
    assert not env.last_rollout_phase_table() and not env.last_rollout_desired_table()
    env.close()


def test_a_captured_call_among_eager_ones(mds):
    """An eager flight, a captured call that continues it, an eager call elsewhere in time (it overwrites the rows the flight left), a new
    upload of the same trajectories, then the replay -- against the same four calls flown eagerly without any table, byte for byte."""
    torch = mds.torch
    t1 = after(T0, 70)
    _, _, P = setup(2, 8)
    off = make(mds, 2, 8, False, table=False)
    off.rollout_geometric(T0, 70, obs_every_step=True)
    off.rollout_geometric(5.0, 30, obs_every_step=True)
    off.set_trajectories(P)
    want_rows = raw(off.rollout_geometric(t1, 50, obs_every_step=True))
    want_state = off.get_state().tobytes()
    off.close()
    on = make(mds, 2, 8, True)
    on.rollout_geometric(T0, 70, obs_every_step=True)
    assert on.last_rollout_desired_table()
    state_before = on.get_state().tobytes()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            on.rollout_geometric(t1, 50, obs_every_step=True)
    torch.cuda.current_stream().wait_stream(side)
    assert not on.last_rollout_phase_table() and not on.last_rollout_desired_table()
    assert on.get_state().tobytes() == state_before                         # capturing ran nothing
    on.rollout_geometric(5.0, 30, obs_every_step=True)
    assert on.last_rollout_desired_table()
    on.set_trajectories(P)
    g.replay()
    torch.cuda.synchronize()
    assert (raw(on._obs) == want_rows).all() and on.get_state().tobytes() == want_state
    on.close()


def test_wide_row_flight_tracks_the_oracle(mds):
    E, D, steps, tol = 33, 8, 60, 1e-5
    xyz, rpy, P = setup(E, D)
    oobs, _ = H.oracle_closed_loop(xyz, rpy, P, steps)
    env = make(mds, E, D, True, perturb=False)
    v = env.rollout_geometric(0.0, steps, obs_every_step=True).double().cpu().numpy().reshape(-1, 20)
    assert env.last_rollout_desired_table()
    env.close()
    err = np.abs(v[:, :16] - oobs[:, :16]).max()
    print(f"float32, wide rows on, {E} x {D}: max |state - oracle| after {steps} steps = {err:.3e} (gate {tol:g})")
    assert err < tol

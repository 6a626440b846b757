"""The ground-effect / downwash step kernels (k_step_env, k_step_ctrl_env: a lane reads its env-mates' rows from one state buffer and writes
the other) beyond one wavefront, on every entry point that serves these physics modes.  Scenes and oracle runs: tests/envfx_cases.py (what
they can tell apart is shown on the oracle alone in tests/test_envfx_cpu.py).

1. Envs across wavefront and workgroup boundaries: 37 x 7, 52 x 5, 17 x 16 drones (and 1 x 1, 3 x 1: no env-mates), every mode, float64 and
   float32, env.step with 3 substeps and step_geometric with 2.  (a) against the oracle at the sibling tests' gates; (b) the envs that lie
   across a boundary flown again in a handle of <= 63 drones: rows, get_state() and the state planes bit for bit; (c) two sentinel rows behind
   the observation and action buffers; (d) get_state() / state_views() against the observation after odd and even numbers of launches, and
   set_state / mds_set_origin / reset() / set_trajectories while the handle stands in its second buffer.
2. Every entry point: mds_rollout_geometric(_fused), mds_rollout_step(_fused), mds_rollout_lqr_fused, mds_step_nominal / mds_rollout_nominal_fused (both low levels),
   the CBF step and rollout, the DSLPID step and rollout, segment-table trajectories, CF2X; float16 handles are refused.
3. One substep from constructed states: (v' - v) / dt and (w' - w) / dt against the oracle on every branch of downwash_pair and ground_effect.
4. fp32 far from the world origin: the 37 x 7 scene with every env moved to (+-512, +-256) m, origins at the drones, compared in env-local
   coordinates at the gate of the scene at the origin (3e-5, not scaled by |x|).
5. Wind with three non-zero components.

Measured on an MI355X (every test prints its figures: pytest -s).  Part 1, max |error| over the state columns as a fraction of the gate, over
all shapes and modes: float64 < 0.001 on both paths; float32 0.165 under env.step (0.097 over the boundary envs) and 0.019 under step_geometric
(0.013); every bit-equality of (b) holds.  Part 2, float64 step loops against the oracle: 12-state LQR 2.1e-14, LQR-omega 5.0e-14,
LQR-yank-omega 1.3e-14 (gate 1e-7), CBF 1.3e-15 (gate 1e-6), segment tables 1.0e-14 (gate 1e-9); float32 as a fraction of the gate: rollout_step
loop 0.023, DSLPID 0.061, CF2X 0.020, segment tables 1.1e-6 against 2e-5; every rollout equals its step loop bit for bit.  Part 3: float64
3e-14 (dv/dt) and 1e-13 (dw/dt) against gates of 2e-8 .. 9e-8; float32 1.2e-5 against 2e-3 and 2.8e-5 against 8e-3 .. 2e-2.  Part 4, max |local
state error| after 15 control steps against the gate 3e-5: the scene at the origin 4.8e-7 (env.step) and 1.2e-6 (step_geometric), the displaced
scene the same bits; with the separation formed from world coordinates the displaced scene measured 2.6e-4 and 2.1e-4."""
import ctypes as C

import numpy as np
import pytest

from oracle import np_oracle as O
from tests import envfx_cases as X
from tests import helpers as H
from tests.test_gpu_parity import make_env, mds  # noqa: F401  (mds: the module's fixture)

pytestmark = pytest.mark.gpu

SENTINEL = 12345.0
DTYPES = ["float64", "float32"]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64 if a.dtype == np.float64 else np.int32)


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _host(t):
    return t.detach().cpu().numpy().copy()


def _open(mds, scene, mode, dtype, pyb, model=None):
    """-> (env, obs buffer [n + 2, 20], action buffer [n + 2, 4]): the env writes its observations and actions into the first n rows of two
    larger buffers filled with a sentinel (BaseAviary's _obs / _act replaced by views, as tests/test_gpu_whole_wave.py does)"""
    torch = mds.torch
    E, D = scene["E"], scene["D"]
    n = E * D
    env = make_env(mds, E, D, scene["xyz"], scene["rpy"], dtype, pyb, 100, getattr(mds.Physics, mode), model=model)
    obs = torch.full((n + 2, 20), SENTINEL, dtype=env.dtype, device=env.device)
    act = torch.full((n + 2, 4), SENTINEL, dtype=env.dtype, device=env.device)
    assert env._obs.shape == (E, D, 20) and env._act.shape == (E, D, 4) and env._obs.dtype == obs.dtype
    env._obs, env._act = obs[:n].view(E, D, 20), act[:n].view(E, D, 4)
    return env, obs, act


def _action(mds, env, scene, k, consts=O.CF2P):
    return mds.torch.as_tensor(X.open_loop_action(scene, k, consts).reshape(scene["E"], scene["D"], 4), dtype=env.dtype, device=env.device)


def _planes(env):
    """the 13 state planes and 3 origin planes as the handle holds them now [16, n] (asked for after the call: the modes swap buffers)"""
    sv = env.state_views()
    return np.stack([_host(p) for p in sv["comp"] + sv["origin"]])


def _check_bookkeeping(env, row):
    """get_state() agrees with the observation row [n, 20] just written, and state_views() with get_state()"""
    n = row.shape[0]
    st = env.get_state().reshape(n, 13)
    pl = _planes(env).astype(np.float64)                                                    # (exact: widening only)
    assert np.array_equal(pl[0:3] + pl[13:16], st[:, 0:3].T) and np.array_equal(pl[3:13], st[:, 3:13].T)
    r = row.astype(np.float64)
    assert np.array_equal(r[:, 3:7], st[:, 3:7]) and np.array_equal(r[:, 10:13], st[:, 7:10])
    if row.dtype == np.float64:
        assert np.array_equal(r[:, 0:3], st[:, 0:3])
    else:                                                                                   # the row's position is local + origin rounded to fp32
        assert (np.abs(r[:, 0:3] - st[:, 0:3]) <= 0.5 * np.spacing(np.abs(row[:, 0:3])).astype(np.float64)).all()
    return st


def _fly(mds, scene, mode, dtype, path, steps=X.STEPS, model=None, check_at=()):
    """-> dict(rows [steps, n, 20], acts [steps, n, 4] or None, state [n, 13], planes [16, n], tails: the sentinel rows)"""
    E, D = scene["E"], scene["D"]
    n = E * D
    consts = O.CF2X if model is not None and model.name == "CF2X" else O.CF2P
    env, obs, act = _open(mds, scene, mode, dtype, 300 if path == "step" else 200, model)
    rows, acts = [], []
    if path == "geo":
        env.set_trajectories(scene["P"])
        env.step(mds.torch.zeros((E, D, 4), dtype=env.dtype, device=env.device))
    t = 0.0
    for k in range(steps):
        if path == "step":
            o, *_ = env.step(_action(mds, env, scene, k, consts))
        else:
            o, a = env.step_geometric(t, return_action=True)
            acts.append(_host(a).reshape(n, 4))
            t += 0.01
        assert o.data_ptr() == obs.data_ptr()
        rows.append(_host(o).reshape(n, 20))
        if k in check_at:
            _check_bookkeeping(env, rows[-1])
    st = _check_bookkeeping(env, rows[-1])
    out = dict(rows=np.array(rows), acts=np.array(acts) if acts else None, state=st, planes=_planes(env),
               tails=np.concatenate([_host(obs[n:]).ravel(), _host(act[n:]).ravel()]))
    env.close()
    return out


# ----------------------------------------------------------------------------------------------------------------------------------------------
# 1. envs across wavefront and workgroup boundaries
# ----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["step", "geo"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode", list(X.MODES))
@pytest.mark.parametrize("shape", X.SHAPES)
def test_envs_across_wavefront_and_workgroup_boundaries(mds, shape, mode, dtype, path):  # noqa: F811
    E, D = shape
    n = E * D
    scene, ref = X.stacked(E, D), X.loop_run(E, D, X.MODES[mode], path)
    full = _fly(mds, scene, mode, dtype, path, check_at=(0, 1))           # env.step: 3 and 6 launches so far (odd, even), 45 at the end
    # (a) against the oracle, every step at that step's gate; the drones of the boundary envs reported apart
    b = X.drones_of(X.boundary_envs(E, D), D)
    worst = worst_b = 0.0
    for k in range(X.STEPS):
        g = X.gate(path, dtype, ref["obs"][k])
        worst = max(worst, X.state_err(full["rows"][k], ref["obs"][k]) / g)
        if len(b):
            worst_b = max(worst_b, X.state_err(full["rows"][k][b], ref["obs"][k][b]) / g)
    print(f"\n[envfx] {E}x{D} {mode} {dtype} {path}: max err / gate over all drones {worst:.3f}, over the boundary envs {worst_b:.3f}")
    assert worst < 1.0 and worst_b < 1.0
    np.testing.assert_allclose(full["rows"][-1][:, 16:], ref["obs"][-1][:, 16:], rtol=1e-5 if dtype == "float32" else 1e-10)
    # (c) nothing behind the last drone's row, in the observation buffer or in the action buffer
    assert (full["tails"] == SENTINEL).all()
    # (b) the boundary envs in a handle of one wavefront where nothing straddles: the mate loop runs e0 .. e0 + D in the same order on the
    # same values whatever the lane, so every bit is the same
    if shape in X.BIG:
        sub = X.sub_envs(E, D)
        idx = X.drones_of(sub, D)
        small = _fly(mds, X.take(scene, sub), mode, dtype, path)
        assert (small["tails"] == SENTINEL).all()
        assert _same_bits(full["rows"][:, idx], small["rows"])
        assert _same_bits(full["state"][idx], small["state"]) and _same_bits(full["planes"][:, idx], small["planes"])
        if path == "geo":
            assert _same_bits(full["acts"][:, idx], small["acts"])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode", ["PYB_DW", "PYB_GND_DRAG_DW"])
def test_state_calls_while_the_handle_stands_in_its_second_buffer(mds, mode, dtype):  # noqa: F811
    """env.step with 3 substeps leaves the handle in its second buffer after every odd number of calls.  There: set_state, mds_set_origin and
    reset(), each followed by two more steps (the parity stays odd) against the oracle continued from the same state."""
    E, D = 37, 7
    n = E * D
    scene = X.stacked(E, D)
    env, obs, act = _open(mds, scene, mode, dtype, 300)
    ora = X.make_oracle(scene, X.MODES[mode], 300, 100)
    rng = np.random.default_rng(4)
    home = env.state_views()["comp"][0].data_ptr()
    k = 0

    def steps(m):
        nonlocal k
        for _ in range(m):
            o, *_ = env.step(_action(mds, env, scene, k))
            ref = ora.step(X.open_loop_action(scene, k))
            k += 1
        row = _host(o).reshape(n, 20)
        _check_bookkeeping(env, row)
        e = X.state_err(row, ref) / X.gate("step", dtype, ref)
        assert e < 1.0, e
        return e

    errs = [steps(3)]
    assert env.state_views()["comp"][0].data_ptr() != home                       # 9 launches: the second buffer
    s = env.get_state().reshape(n, 13)
    s[:, 0:3] += rng.uniform(-0.01, 0.01, size=(n, 3))
    s[:, 7:13] += rng.uniform(-0.05, 0.05, size=(n, 6))
    env.set_state(s)
    ora.pos, ora.quat, ora.vel, ora.rates = s[:, 0:3].copy(), s[:, 3:7].copy(), s[:, 7:10].copy(), s[:, 10:13].copy()
    np.testing.assert_allclose(env.get_state().reshape(n, 13), s, rtol=0, atol=1e-12 if dtype == "float64" else 1e-6)
    errs.append(steps(2))
    assert env.state_views()["comp"][0].data_ptr() != home
    before = env.get_state().reshape(n, 13)
    org = np.ascontiguousarray(before[:, 0:3] + rng.normal(size=(n, 3)) * 0.1)
    assert env._lib.mds_set_origin(env._h, org.ctypes.data_as(C.POINTER(C.c_double)), env._stream()) == 0
    np.testing.assert_allclose(env.get_state().reshape(n, 13), before, rtol=0, atol=1e-12 if dtype == "float64" else 1e-6)
    errs.append(steps(2))
    assert env.state_views()["comp"][0].data_ptr() != home
    env.reset()
    ora.reset()
    np.testing.assert_allclose(env.get_state().reshape(n, 13)[:, 0:3], scene["xyz"].reshape(n, 3), rtol=0, atol=1e-12 if dtype == "float64" else 1e-6)
    errs.append(steps(2))
    print(f"\n[envfx] second buffer {mode} {dtype}: err / gate after 3 steps {errs[0]:.3f}, set_state {errs[1]:.3f}, set_origin {errs[2]:.3f}, reset {errs[3]:.3f}")
    assert (_host(obs[n:]) == SENTINEL).all()
    env.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_controller_path_from_the_second_buffer(mds, dtype):  # noqa: F811
    """One substep per control step: every step_geometric call starts from the other buffer.  set_trajectories (it re-bases the origin) lands
    after one launch, in the second buffer; then 6 steps against the oracle, get_state() and state_views() after each."""
    E, D = 37, 7
    n = E * D
    scene = X.stacked(E, D)
    ref = X.geo_loop(scene, "dyn_gnd_drag_dw", steps=6, pyb=100)
    env, obs, act = _open(mds, scene, "PYB_GND_DRAG_DW", dtype, 100)
    home = env.state_views()["comp"][0].data_ptr()
    env.step(mds.torch.zeros((E, D, 4), dtype=env.dtype, device=env.device))
    assert env.state_views()["comp"][0].data_ptr() != home
    env.set_trajectories(scene["P"])
    t, worst = 0.0, 0.0
    for k in range(6):
        row = _host(env.step_geometric(t)).reshape(n, 20)
        t += 0.01
        _check_bookkeeping(env, row)
        assert (env.state_views()["comp"][0].data_ptr() == home) == (k % 2 == 0)
        worst = max(worst, X.state_err(row, ref["obs"][k]) / X.gate("geo", dtype, ref["obs"][k]))
    print(f"\n[envfx] controller path, 1 substep, {dtype}: max err / gate {worst:.3f}")
    assert worst < 1.0 and (_host(obs[n:]) == SENTINEL).all()
    env.close()


# ----------------------------------------------------------------------------------------------------------------------------------------------
# 3. the force laws' branches, one substep at a time
# ----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.filterwarnings("ignore:divide by zero")
@pytest.mark.parametrize("dtype,atol_v,rtol_w", [("float64", None, 1e-9), ("float32", 2e-3, 2e-4)])       # fp32: test_step_accelerations_match_the_reference_tree's
@pytest.mark.parametrize("batch", ["pair", "tower"])
@pytest.mark.parametrize("model", ["cf2p", "cf2x"])
def test_one_substep_accelerations_on_every_branch(mds, model, batch, dtype, atol_v, rtol_w):  # noqa: F811
    b = X.pair_batch(model) if batch == "pair" else X.tower_batch(model)
    D, n = b["D"], b["state"].shape[0]
    E = n // D
    env = make_env(mds, E, D, b["state"][:, 0:3].reshape(E, D, 3), np.zeros((E, D, 3)), dtype, 240, 240, mds.Physics.PYB_GND_DRAG_DW,
                   model=mds.DroneModel.CF2X if model == "cf2x" else None)
    env.set_state(b["state"])
    s0 = env.get_state().reshape(n, 13)                  # the state as stored: float32 handles round it, and the oracle starts from that
    if dtype == "float64":
        assert np.array_equal(s0[:, [0, 1, 2, 7, 8, 9, 10, 11, 12]], b["state"][:, [0, 1, 2, 7, 8, 9, 10, 11, 12]])
    if batch == "pair":                                  # the one-ulp pairs survive the storage: their lateral distance is exact in fp32
        _, dxy = X.pair_geometry(b, s0)
        assert (dxy[b["tags"]["ulp_in"], 0] == X.ULP_IN).all() and (dxy[b["tags"]["ulp_out"], 0] == X.ULP_OUT).all()
    env.step(mds.torch.as_tensor(b["rpm"].reshape(E, D, 4), dtype=env.dtype, device=env.device))
    s1 = env.get_state().reshape(n, 13)
    env.close()
    av, aw = X.accelerations(b, s0)
    gv, gw = (s1[:, 7:10] - s0[:, 7:10]) * 240.0, (s1[:, 10:13] - s0[:, 10:13]) * 240.0
    assert np.isfinite(s1).all()                         # no NaN from the pole of u = dxy / (c_2 dz + c_3), no inf from dz = 0
    ev, ew = np.abs(gv - av).max(axis=1), np.abs(gw - aw).max(axis=1)
    gate_v = 1e-9 * np.abs(av).max() if atol_v is None else atol_v
    gate_w = rtol_w * np.abs(aw).max()
    print(f"\n[envfx] one substep {model} {batch} {dtype}: max |dv/dt err| {ev.max():.3e} (gate {gate_v:.3e}), max |dw/dt err| {ew.max():.3e} (gate {gate_w:.3e})")
    for tag, idx in b["tags"].items():
        assert ev[idx].max() <= gate_v and ew[idx].max() <= gate_w, (tag, ev[idx].max(), ew[idx].max())
    assert ev.max() <= gate_v and ew.max() <= gate_w


# ----------------------------------------------------------------------------------------------------------------------------------------------
# 4. fp32 far from the world origin
# ----------------------------------------------------------------------------------------------------------------------------------------------
def _fly_local(mds, scene, path, steps=X.STEPS):
    """the float32 PYB_GND_DRAG_DW flight of ``scene`` with the origins at the Lemniscate centres (path "geo": set_trajectories puts them
    there; path "step": mds_set_origin, then reset() so that the start is stored relative to them) -> (env-local state [n, 13] from
    get_state(), float64: position minus the drone's centre; the 13 local state planes [13, n])"""
    E, D = scene["E"], scene["D"]
    n = E * D
    env, obs, act = _open(mds, scene, "PYB_GND_DRAG_DW", "float32", 300 if path == "step" else 200)
    cen = np.ascontiguousarray(scene["cen"].reshape(n, 3))
    if path == "step":
        assert env._lib.mds_set_origin(env._h, cen.ctypes.data_as(C.POINTER(C.c_double)), env._stream()) == 0
        env.reset()
        for k in range(steps):
            env.step(_action(mds, env, scene, k))
    else:
        env.set_trajectories(scene["P"])
        env.reset()
        env.step(mds.torch.zeros((E, D, 4), dtype=env.dtype, device=env.device))
        t = 0.0
        for k in range(steps):
            env.step_geometric(t)
            t += 0.01
    pl = _planes(env)
    assert np.array_equal(pl[13:16].astype(np.float64), cen.T)                     # the origins are exact in fp32
    st = env.get_state().reshape(n, 13)
    st[:, 0:3] -= cen
    assert (_host(obs[n:]) == SENTINEL).all()
    env.close()
    return st, pl[:13]


def _local_ref(scene, run):
    o = run["obs"][-1]
    n = o.shape[0]
    R = O.quat_to_rotmat_bullet(o[:, 3:7])
    rates = np.einsum("nji,nj->ni", R, o[:, 13:16])                               # body rates from the observation's world-frame ones
    return np.concatenate([o[:, 0:3] - scene["cen"].reshape(n, 3), o[:, 3:7], o[:, 10:13], rates], axis=1)


@pytest.mark.parametrize("path", ["step", "geo"])
def test_fp32_far_from_the_world_origin(mds, path):  # noqa: F811
    """include/mds.h (mds_set_origin): positions are stored relative to a per-drone origin so that fp32 keeps its resolution far from the world
    origin.  The 37 x 7 scene at (+-512, +-256) m against the float64 oracle in env-local coordinates, at the gate the scene holds at the
    origin: 3e-5, not scaled by |x|.  The separation of two env-mates is formed from local positions and origins differenced separately
    (csrc/mds_kernels.hip, env_substep); formed from world coordinates it carried the 3e-5 m ulp of |x| = 512 m into separations of 0.05 m
    and this test measured 2.6e-4 (env.step) and 2.1e-4 (step_geometric) against 3e-5; now 4.8e-7 and 1.2e-6, as at the origin.  Centres on a
    2^-10 m grid and starts on a 2^-20 m grid make the move exact in fp32 and float64: local start, origin differences, Lemniscate in the
    local frame and the true height under the ground effect are then the same numbers in both handles, so the displaced handle holds the
    same local bits as the undisplaced one."""
    E, D = 37, 7
    base = X.stacked(E, D)
    far = X.displaced(base)
    ref0, ref1 = X.loop_run(E, D, "dyn_gnd_drag_dw", path), X.loop_run(E, D, "dyn_gnd_drag_dw", path, shifted=True)
    st0, pl0 = _fly_local(mds, base, path)
    st1, pl1 = _fly_local(mds, far, path)
    e0 = np.abs(st0 - _local_ref(base, ref0)).max()
    e1 = np.abs(st1 - _local_ref(far, ref1)).max()
    print(f"\n[envfx] far from the origin, {path}: max |local state error| at the origin {e0:.3e}, displaced {e1:.3e} (gate 3e-5); "
          f"local planes bit-equal: {_same_bits(pl0, pl1)}")
    assert np.abs(_local_ref(base, ref0) - _local_ref(far, ref1)).max() < 1e-9       # the oracle itself: float64 does not mind the move
    assert e0 < 3e-5
    assert e1 < 3e-5
    assert _same_bits(pl0, pl1)


# ----------------------------------------------------------------------------------------------------------------------------------------------
# 5. wind with three non-zero components
# ----------------------------------------------------------------------------------------------------------------------------------------------
def test_wind_with_three_components_under_plain_dyn(mds):  # noqa: F811
    """test_wind_force_matches_oracle's scene and gate with the wind (2.5e-4, -1.7e-4, 0.9e-4) N; the same run with y and z swapped is
    FACTOR x the gate away (tests/test_envfx_cpu.py), so a kernel that mixed the components up fails here."""
    scene, ref = X.wind_scene_dyn(), X.wind_runs("dyn")
    E, D = scene["E"], scene["D"]
    env = make_env(mds, E, D, scene["xyz"], scene["rpy"], "float64")
    env.set_trajectories(scene["P"])
    env.set_wind(X.WIND)
    env.step(mds.torch.zeros((E, D, 4), dtype=env.dtype))
    t = 0.0
    for k in range(X.WIND_STEPS):
        g = _host(env.step_geometric(t)).reshape(-1, 20)
        t += env.CTRL_TIMESTEP
        np.testing.assert_allclose(g, ref["obs"][k], atol=1e-9, rtol=1e-11)
    assert X.state_err(g, X.wind_runs("dyn", swapped=True)["obs"][-1]) > X.FACTOR * 1e-9
    env.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_wind_with_three_components_under_ground_effect_and_downwash(mds, dtype):  # noqa: F811
    """The same wind through env_substep (PYB_GND_DRAG_DW, env.step, 3 substeps), 7 x 5 drones stacked over the floor.  The swapped wind is
    FACTOR x the float64 gate away; at this wind strength it is within FACTOR x the float32 gate, so the float32 case pins the path against
    the oracle only."""
    scene, ref = X.stacked(7, 5), X.wind_runs("envfx")
    env, obs, act = _open(mds, scene, "PYB_GND_DRAG_DW", dtype, 300)
    env.set_wind(X.WIND)
    worst = 0.0
    for k in range(X.WIND_STEPS):
        o, *_ = env.step(_action(mds, env, scene, k))
        worst = max(worst, X.state_err(_host(o).reshape(-1, 20), ref["obs"][k]) / X.gate("step", dtype, ref["obs"][k]))
    print(f"\n[envfx] wind under PYB_GND_DRAG_DW {dtype}: max err / gate {worst:.3f}")
    assert worst < 1.0
    if dtype == "float64":
        g = _host(o).reshape(-1, 20)
        assert X.state_err(g, X.wind_runs("envfx", swapped=True)["obs"][-1]) > X.FACTOR * X.gate("step", dtype, ref["obs"][-1])
    env.close()


# ----------------------------------------------------------------------------------------------------------------------------------------------
# 2. every entry point that serves these modes (37 x 7 drones, PYB_GND_DRAG_DW, 2 substeps per control step unless said otherwise)
# ----------------------------------------------------------------------------------------------------------------------------------------------
ENTRY_MODE = "PYB_GND_DRAG_DW"


def _zeros(mds, env):
    return mds.torch.zeros((env.NUM_ENVS, env.NUM_DRONES, 4), dtype=env.dtype, device=env.device)


def _log_buffer(mds, env, slots):
    """a log of ``slots`` observations with two sentinel rows behind it -> (the whole buffer, its [slots, E, D, 20] view)"""
    n = env.n
    buf = mds.torch.full((slots * n + 2, 20), SENTINEL, dtype=env.dtype, device=env.device)
    return buf, buf[:slots * n].view(slots, env.NUM_ENVS, env.NUM_DRONES, 20)


@pytest.mark.parametrize("dtype", DTYPES)
def test_rollout_step_with_action_table_log_ring_and_reset(mds, dtype):  # noqa: F811
    """mds_rollout_step and mds_rollout_step_fused (it forwards) with 3 action sets, a 4-slot ring entered at step 2 and one episode reset in
    the middle of the call, 3 substeps per step: bit for bit the loop of env.step calls with an explicit reset, which lands after 9
    launches, in the second buffer; that loop against the oracle's."""
    E, D = X.ENTRY_SHAPE
    n, R = E * D, X.ROLL
    scene, ref = X.stacked(E, D), X.entry_run("rollout_step")
    table = mds.torch.as_tensor(X.roll_actions(scene).reshape(R["sets"], E, D, 4))
    env, obs, act = _open(mds, scene, ENTRY_MODE, dtype, 300)
    table = table.to(dtype=env.dtype, device=env.device).contiguous()
    home = env.state_views()["comp"][0].data_ptr()
    ring, worst, resets = np.full((R["slots"], n, 20), SENTINEL, dtype=_host(obs).dtype), 0.0, 0
    for i, j in enumerate(range(R["first_step"], R["first_step"] + R["n_steps"])):
        if j > 0 and j % R["episode_len"] == 0:
            assert env.state_views()["comp"][0].data_ptr() != home
            env.reset()
            resets += 1
        o, *_ = env.step(table[j % R["sets"]])
        ring[j % R["slots"]] = _host(o).reshape(n, 20)
        worst = max(worst, X.state_err(ring[j % R["slots"]], ref["obs"][i]) / X.gate("step", dtype, ref["obs"][i]))
    print(f"\n[envfx] rollout_step loop {dtype}: max err / gate {worst:.3f}")
    assert resets == 1 and worst < 1.0
    state = env.get_state()
    env.close()
    for spl in (1, 4):
        b, bobs, _ = _open(mds, scene, ENTRY_MODE, dtype, 300)
        buf, log = _log_buffer(mds, b, R["slots"])
        b.rollout_step(table, R["first_step"], R["n_steps"], obs_log=log, episode_len=R["episode_len"], steps_per_launch=spl)
        assert _same_bits(_host(log).reshape(R["slots"], n, 20), ring)
        assert (_host(buf[R["slots"] * n:]) == SENTINEL).all() and (_host(bobs) == SENTINEL).all()
        assert _same_bits(b.get_state(), state)
        b.close()


def _ctrl_env(mds, scene, dtype, kind):
    """an env of the entry-point tests with its controller attached, after the first env.step of the loop"""
    from multidronesim_amd.control import LQRController, LQROmegaController, LQRYankOmegaController, ThrustOmegaController, YankOmegaController
    from multidronesim_amd.model import LinearizedModel, LinearizedOmegaModel, LinearizedYankOmegaModel
    env, obs, act = _open(mds, scene, ENTRY_MODE, dtype, 200)
    env.set_trajectories(scene["P"])
    first = 0.0
    if kind == "lqr":
        LQRController(env, LinearizedModel(env))
    elif kind == "omega":
        LQROmegaController(env, LinearizedOmegaModel(env), ThrustOmegaController(env))
        env.set_cbf_nominal("lqr_omega")
        first = float(env.HOVER_RPM)
    else:
        LQRYankOmegaController(env, LinearizedYankOmegaModel(env), YankOmegaController(env))
        env.set_cbf_nominal("lqr_yank_omega")
        first = float(env.HOVER_RPM)
    env.step(mds.torch.full((env.NUM_ENVS, env.NUM_DRONES, 4), first, dtype=env.dtype, device=env.device))
    return env, obs


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", ["lqr", "omega", "yank"])
def test_lqr_and_nominal_rollouts_are_their_step_loops(mds, kind, dtype):  # noqa: F811
    """mds_rollout_lqr_fused against mds_step_lqr, mds_rollout_nominal_fused against mds_step_nominal (LQR-omega + ThrustOmega; LQR-yank-omega +
    YankOmega, whose kernel reads the previous row's RPM echo from the observation buffer before the same launch rewrites it): with a log
    and without, bit for bit, the log's last slot equal to the last observation; the step loop in float64 against the oracle's loop at
    1e-7 (test_ground_effect_under_the_lqr_and_cbf_paths, test_plain_lqr_lowlevel_loop_matches_oracle)."""
    E, D = X.ENTRY_SHAPE
    n = E * D
    scene = X.stacked(E, D)
    if kind == "lqr":
        scene = X.lqr_scene(scene)
    ref = X.entry_run(kind)
    T = ref["obs"].shape[0]
    a, aobs = _ctrl_env(mds, scene, dtype, kind)
    t, rows = 0.0, []
    for k in range(T):
        rows.append(_host(a.step_lqr(t) if kind == "lqr" else a.step_nominal(t)).reshape(n, 20))
        t += a.CTRL_TIMESTEP
    rows = np.array(rows)
    assert np.isfinite(rows).all() and (_host(aobs[n:]) == SENTINEL).all()
    if dtype == "float64":
        err = max(X.state_err(rows[k], ref["obs"][k]) for k in range(T))
        print(f"\n[envfx] {kind} step loop float64: max |state err| {err:.3e} (gate 1e-7)")
        assert err < 1e-7
        np.testing.assert_allclose(rows[-1][:, 16:], ref["obs"][-1][:, 16:], rtol=1e-9)
    state = a.get_state()
    a.close()
    ctl = "lqr" if kind == "lqr" else "nominal"
    b, bobs = _ctrl_env(mds, scene, dtype, kind)
    buf, log = _log_buffer(mds, b, T)
    last, _ = b.rollout_geometric_fused(0.0, T, log=True, log_out=log, controller=ctl)
    assert _same_bits(_host(log).reshape(T, n, 20), rows) and _same_bits(_host(last).reshape(n, 20), rows[-1])
    assert (_host(buf[T * n:]) == SENTINEL).all() and (_host(bobs[n:]) == SENTINEL).all() and _same_bits(b.get_state(), state)
    b.close()
    c, cobs = _ctrl_env(mds, scene, dtype, kind)
    last, none = c.rollout_geometric_fused(0.0, T, controller=ctl)
    assert none is None and _same_bits(_host(last).reshape(n, 20), rows[-1]) and (_host(cobs[n:]) == SENTINEL).all()
    assert _same_bits(c.get_state(), state)
    c.close()


def test_cbf_step_and_rollout_under_ground_effect_across_boundaries(mds):  # noqa: F811
    """mds_step_cbf_geometric and mds_rollout_cbf_geometric under PYB_GND on 37 x 7 = 259 drones (nominal -> QP -> ThrustOmega low level ->
    first substep + replay), float64: the statuses are the oracle's at every step, the rollout equals the step loop bit for bit."""
    from multidronesim_amd.cbf.cbf import DroneCBF
    from multidronesim_amd.cbf.qptracker import DroneQPTracker
    from multidronesim_amd.model.linear_omega import LinearizedOmegaModel
    scene, x_obs, obs_r = X.cbf_scene()
    E, D, steps = scene["E"], scene["D"], 10
    n = E * D

    def make():
        env, obs, act = _open(mds, scene, "PYB_GND", "float64", 200)
        env.set_trajectories(scene["P"])
        cbf = DroneCBF(env, [LinearizedOmegaModel(env) for _ in range(D)], safety_radius=0.05, zscale=1.0, order=2)
        trk = DroneQPTracker(cbf, num_robots=D, xdim=9, env=env)
        env.step(_zeros(mds, env))
        return env, obs, cbf, trk

    a, aobs, cbf, trk = make()
    moved = []
    oobs, ohist = H.oracle_cbf_closed_loop(scene["xyz"], scene["rpy"], scene["P"], steps, cbf.Kcbf.reshape(-1), cbf.umax, 0.05, 1.0, x_obs, obs_r,
                                           pyb_freq=200, ctrl_freq=100, physics="dyn_gnd", filter_log=moved)
    t = 0.0
    for k in range(steps):
        gobs, st = a.step_cbf_geometric(t, trk, x_obs, obs_r)
        np.testing.assert_array_equal(st.cpu().numpy(), ohist[k])
        t += 0.01
    row = _host(gobs).reshape(n, 20)
    err = X.state_err(row, oobs.reshape(n, 20))
    print(f"\n[envfx] CBF loop under PYB_GND, 259 drones: max |state err| {err:.3e} (gate 1e-6); the filter moved the input by up to {np.max(moved):.3e}")
    assert err < 1e-6 and (_host(aobs[n:]) == SENTINEL).all()
    state, status = a.get_state(), st.cpu().numpy().copy()
    a.close()
    b, bobs, _, trk_b = make()
    robs, rst = b.rollout_cbf_geometric(0.0, steps, trk_b, x_obs, obs_r)
    assert _same_bits(_host(robs).reshape(n, 20), row) and np.array_equal(rst.cpu().numpy(), status) and _same_bits(b.get_state(), state)
    assert (_host(bobs[n:]) == SENTINEL).all()
    b.close()


@pytest.mark.parametrize("dtype,tol", [("float64", 1e-8), ("float32", 3e-5)])        # test_dslpid_under_ground_effect_and_downwash's
def test_dslpid_step_and_rollout_with_two_target_sets(mds, dtype, tol):  # noqa: F811
    from multidronesim_amd.control.DSLPIDControl import DSLPIDControl
    E, D = X.ENTRY_SHAPE
    n = E * D
    scene, ref = X.stacked(E, D), X.entry_run("dslpid")
    tp, tr = X.dsl_targets(scene)
    T = ref["obs"].shape[0]

    def make():
        env, obs, act = _open(mds, scene, ENTRY_MODE, dtype, 200)
        c = DSLPIDControl(drone_model=mds.DroneModel.CF2P)
        for name in ("P_COEFF_FOR", "I_COEFF_FOR", "D_COEFF_FOR", "P_COEFF_TOR", "I_COEFF_TOR", "D_COEFF_TOR"):
            setattr(c, name, 0.5 * getattr(c, name))
        env.set_dslpid_gains(c)
        env.step(_zeros(mds, env))
        return env, obs

    a, aobs = make()
    worst = 0.0
    for k in range(T):
        row = _host(a.step_dslpid(tp[k % X.DSL_TARGETS], tr[k % X.DSL_TARGETS])).reshape(n, 20)
        worst = max(worst, X.state_err(row, ref["obs"][k]) / (tol * max(1.0, np.abs(ref["obs"][k][:, :16]).max())))
    print(f"\n[envfx] DSLPID loop {dtype}: max err / gate {worst:.3f}")
    assert worst < 1.0 and (_host(aobs[n:]) == SENTINEL).all()
    np.testing.assert_allclose(row[:, 16:], ref["obs"][-1][:, 16:], rtol=1e-5 if dtype == "float32" else 1e-9)
    b, bobs = make()
    r = b.rollout_dslpid(tp, tr, T, first_step=0, obs_every_step=True)
    assert _same_bits(_host(r).reshape(n, 20), row) and _same_bits(b.get_state(), a.get_state()) and (_host(bobs[n:]) == SENTINEL).all()
    a.close()
    b.close()


@pytest.mark.parametrize("dtype,tol", [("float64", 1e-9), ("float32", 2e-5)])        # test_fused_step_on_segment_tables_matches_oracle's
def test_step_geometric_on_segment_tables_under_ground_effect_and_downwash(mds, dtype, tol):  # noqa: F811
    """traj_mode != 1: one Circle per drone through the segment tables (the general trajectory evaluator in k_step_ctrl_env); the C rollout
    issues the same steps."""
    import multidronesim_amd.trajectories as TR
    E, D = X.ENTRY_SHAPE
    n = E * D
    base = X.stacked(E, D)
    scene, ref = X.circle_scene(base), X.entry_run("circle")
    T = ref["obs"].shape[0]
    envs = []
    for _ in range(2):
        env, obs, act = _open(mds, scene, ENTRY_MODE, dtype, 200)
        env.set_trajectories(X.circles(base, TR.CircleTrajectory))
        env.step(_zeros(mds, env))
        envs.append((env, obs))
    (a, aobs), (b, bobs) = envs
    t, worst = 0.0, 0.0
    for k in range(T):
        row = _host(a.step_geometric(t)).reshape(n, 20)
        t += a.CTRL_TIMESTEP
        worst = max(worst, X.state_err(row, ref["obs"][k]))
    print(f"\n[envfx] segment-table loop {dtype}: max |state err| {worst:.3e} (gate {tol:.0e})")
    assert worst < tol and (_host(aobs[n:]) == SENTINEL).all()
    r = b.rollout_geometric(0.0, T, obs_every_step=True)
    assert _same_bits(_host(r).reshape(n, 20), row) and _same_bits(b.get_state(), a.get_state()) and (_host(bobs[n:]) == SENTINEL).all()
    a.close()
    b.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_step_geometric_with_cf2x_under_ground_effect_and_downwash(mds, dtype):  # noqa: F811
    """the CF2X airframe (its own propeller positions and torque arms in ground_effect) in a controller path"""
    E, D = X.ENTRY_SHAPE
    scene, ref = X.stacked(E, D), X.entry_run("cf2x")
    T = ref["obs"].shape[0]
    out = _fly(mds, scene, ENTRY_MODE, dtype, "geo", steps=T, model=mds.DroneModel.CF2X)
    worst = max(X.state_err(out["rows"][k], ref["obs"][k]) / X.gate("geo", dtype, ref["obs"][k]) for k in range(T))
    print(f"\n[envfx] CF2X geometric loop {dtype}: max err / gate {worst:.3f}")
    assert worst < 1.0 and (out["tails"] == SENTINEL).all()
    np.testing.assert_allclose(out["rows"][-1][:, 16:], ref["obs"][-1][:, 16:], rtol=1e-5 if dtype == "float32" else 1e-10)


@pytest.mark.parametrize("dtype", DTYPES)
def test_geometric_rollouts_are_the_step_geometric_loop(mds, dtype):  # noqa: F811
    """mds_rollout_geometric and mds_rollout_geometric_fused (they issue the step loop under these modes) on 259 drones, bit for bit, the log
    with two sentinel rows behind it (the 6 x 5 scene of test_ground_effect_and_downwash_in_the_controller_paths fits one wavefront)"""
    E, D = X.ENTRY_SHAPE
    n, T = E * D, X.STEPS
    scene = X.stacked(E, D)
    loop = _fly(mds, scene, ENTRY_MODE, dtype, "geo")
    envs = []
    for _ in range(2):
        env, obs, act = _open(mds, scene, ENTRY_MODE, dtype, 200)
        env.set_trajectories(scene["P"])
        env.step(_zeros(mds, env))
        envs.append((env, obs))
    (a, aobs), (b, bobs) = envs
    r = a.rollout_geometric(0.0, T, obs_every_step=True)
    assert a.last_rollout_streams() == 1
    assert _same_bits(_host(r).reshape(n, 20), loop["rows"][-1]) and _same_bits(a.get_state().reshape(n, 13), loop["state"])
    buf, log = _log_buffer(mds, b, T)
    last, _ = b.rollout_geometric_fused(0.0, T, log=True, log_out=log)
    assert _same_bits(_host(log).reshape(T, n, 20), loop["rows"]) and _same_bits(_host(last).reshape(n, 20), loop["rows"][-1])
    assert _same_bits(b.get_state().reshape(n, 13), loop["state"])
    assert (_host(buf[T * n:]) == SENTINEL).all() and (_host(aobs[n:]) == SENTINEL).all() and (_host(bobs[n:]) == SENTINEL).all()
    a.close()
    b.close()


@pytest.mark.parametrize("mode", list(X.MODES))
def test_half_precision_storage_is_refused_in_these_modes(mds, mode):  # noqa: F811
    """mds_create: ground effect / downwash run on f32 / f64 storage (compensated fp32 and RK4 are refused in tests/test_gpu_parity.py)"""
    s = X.stacked(2, 2)
    with pytest.raises(RuntimeError):
        make_env(mds, 2, 2, s["xyz"], s["rpy"], "float16", 200, 100, getattr(mds.Physics, mode))

"""Randomised episode starts on the device (mds_set_episode_randomisation / mds_reset_episodes) against the float64 oracle of
tests/episode_random_oracle.py, and the invariances the draw was defined to have -- it is a pure function of (seed, global drone index,
the env's episode ordinal, generation) -- as bitwise tests.  Shapes and scenarios: tests/episode_random_cases.py."""
import ctypes as C

import numpy as np
import pytest

from multidronesim_amd import _capi as capi
from tests import episode_cases as EC
from tests import episode_random_cases as RC
from tests import episode_random_oracle as RO
from tests import episode_safety_cases as SC

pytestmark = pytest.mark.gpu
NEAR = 1e-4
FP16_SHAPES = [(130, 1), (200, 2), (38, 7), (17, 16)]           # fp16 rows are 40 bytes: a log ring needs an even number of drones
T = RC.STEPS


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


def build_env(mds, xyz, rpy, actions, params, dtype, rand=True, seed=RC.SEED, half=None, first_env=0):
    """env over the envs of xyz [E,D,3] with the action table actions [A,E,D,4] (NumPy); rand False: randomisation never configured"""
    E, D = xyz.shape[:2]
    env = mds.CtrlAviary(drone_model=mds.DroneModel.CF2P, num_drones=D, initial_xyzs=xyz, initial_rpys=rpy, physics=mds.Physics.PYB_DRAG,
                         pyb_freq=EC.PYB_FREQ, ctrl_freq=EC.CTRL_FREQ, num_envs=E, dtype=dtype)
    env.set_episodes(**params)
    if rand:
        env.set_episode_randomisation(seed, first_env=first_env, **(RC.HALF if half is None else half))
    acts = mds.torch.as_tensor(np.ascontiguousarray(actions), device="cuda").to(env.dtype).contiguous()
    return env, acts


def make_env(mds, E, D, name, dtype, **kw):
    xyz, rpy, actions, params = EC.scenario(E, D, name)
    return build_env(mds, xyz, rpy, actions.reshape(EC.N_SETS, E, D, 4), params, dtype, **kw)


def make_logs(mds, env, steps):
    torch, E, D = mds.torch, env.NUM_ENVS, env.NUM_DRONES
    rdt = torch.float64 if env.dtype == torch.float64 else torch.float32
    return (torch.zeros((steps, E, D, 20), dtype=env.dtype, device="cuda"), torch.zeros((steps, E), dtype=rdt, device="cuda"),
            torch.full((steps, E), -1, dtype=torch.int32, device="cuda"))


def host(t):
    return t.detach().double().cpu().numpy()


def counters(env):
    return {k: v.cpu().numpy().astype(np.float64 if v.is_floating_point() else np.int64) for k, v in env.episode_counters().items()}


def check_counters(got, want, where):
    for key, w in want.items():
        if w.dtype.kind == "i":
            np.testing.assert_array_equal(got[key], w, err_msg=f"{key} {where}")
        else:
            np.testing.assert_allclose(got[key], w, rtol=1e-9, atol=1e-9, err_msg=f"{key} {where}")


def fly(mds, env, acts, steps, spl, reset=True):
    """reset_episodes() (unless reset is False), then `steps` control steps at `spl` per launch: everything the invariants compare, cloned"""
    first = env.reset_episodes().clone() if reset else None
    obs_log, reward_log, flags_log = make_logs(mds, env, steps)
    now = env.rollout_episodes(acts, 0, steps, obs_log, reward_log, flags_log, steps_per_launch=spl).clone()
    return dict(first=first, obs=obs_log, reward=reward_log, flags=flags_log, now=now,
                counters={k: v.clone() for k, v in env.episode_counters().items()}, state=env.get_state())


def assert_same(mds, a, b, sl=slice(None)):
    """bitwise: a's tensors (the envs `sl` of them) == b's"""
    torch = mds.torch
    for key in ("now", "first"):
        if a[key] is not None or b[key] is not None:
            assert torch.equal(a[key][sl], b[key]), key
    for key in ("obs", "reward", "flags"):
        assert torch.equal(a[key][:, sl], b[key]), key
    for key in a["counters"]:
        assert torch.equal(a["counters"][key][sl], b["counters"][key]), key
    np.testing.assert_array_equal(a["state"][sl], b["state"])


# ---------------------------------------------------------------------------------------------------------------- 1. float64
@pytest.mark.parametrize("name", RC.RULES)
@pytest.mark.parametrize("E,D", RC.SHAPES)
def test_f64_matches_oracle(mds, E, D, name):
    """float64: reset_episodes(), 120 steps, reset_episodes() again.  Flags and the integer counters equal the oracle's at every step;
    reward, the logged rows, the current observation and the rows both reset_episodes() calls return (generation 1 and 2) within
    rtol = atol = 1e-9 -- one launch per step, and 8 steps per launch in a call split at step 75."""
    r = RC.oracle_run(E, D, name)
    env, acts = make_env(mds, E, D, name, "float64")
    np.testing.assert_allclose(host(env.reset_episodes()).reshape(-1, 20), r["first_rows"], rtol=1e-9, atol=1e-9)
    obs_log, reward_log, flags_log = make_logs(mds, env, T)
    for k in range(T):
        now = host(env.rollout_episodes(acts, k, 1, obs_log, reward_log, flags_log)).reshape(-1, 20)
        np.testing.assert_allclose(now, r["obs_now"][k], rtol=1e-9, atol=1e-9, err_msg=f"obs_now after step {k}")
        check_counters(counters(env), r["counters"][k], f"after step {k}")
    np.testing.assert_allclose(host(env.reset_episodes()).reshape(-1, 20), r["last_rows"], rtol=1e-9, atol=1e-9)
    after = counters(env)
    assert (after["length"] == 0).all() and (after["ret"] == 0).all()
    np.testing.assert_array_equal(after["count"], r["counters"][T - 1]["count"])
    env.close()
    flags = flags_log.cpu().numpy().astype(np.int64)
    print(f"{E}x{D} {name} float64: done-events {((flags & 3) != 0).sum()}")
    np.testing.assert_array_equal(flags, r["flags"])
    np.testing.assert_allclose(host(reward_log), r["reward"], rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(host(obs_log).reshape(T, -1, 20), r["obs"], rtol=1e-9, atol=1e-9)
    # 8 steps per launch, the call split at a step that is no multiple of 8
    env, acts = make_env(mds, E, D, name, "float64")
    np.testing.assert_allclose(host(env.reset_episodes()).reshape(-1, 20), r["first_rows"], rtol=1e-9, atol=1e-9)
    obs_log, reward_log, flags_log = make_logs(mds, env, T)
    for k0, k1 in ((0, 75), (75, T)):
        now8 = host(env.rollout_episodes(acts, k0, k1 - k0, obs_log, reward_log, flags_log, steps_per_launch=8)).reshape(-1, 20)
        np.testing.assert_allclose(now8, r["obs_now"][k1 - 1], rtol=1e-9, atol=1e-9)
        check_counters(counters(env), r["counters"][k1 - 1], f"after step {k1 - 1}")
    np.testing.assert_allclose(host(env.reset_episodes()).reshape(-1, 20), r["last_rows"], rtol=1e-9, atol=1e-9)
    env.close()
    np.testing.assert_array_equal(flags_log.cpu().numpy(), r["flags"])
    np.testing.assert_allclose(host(reward_log), r["reward"], rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(host(obs_log).reshape(T, -1, 20), r["obs"], rtol=1e-9, atol=1e-9)


# ---------------------------------------------------------------------------------------------------------------- 2. float32
@pytest.mark.parametrize("name", RC.RULES)
@pytest.mark.parametrize("E,D", RC.SHAPES)
def test_f32_matches_oracle_up_to_the_first_close_call(mds, E, D, name):
    """float32 against the oracle under the margin rule of test_episode_gpu: an env is compared up to, not including, its first step whose
    margin is under 1e-4.  At most 10 % of the envs are cut short, at least 20 done-events are compared.  Flags equal; state columns within
    1e-5 absolute, RPM columns within 1e-5 relative (smoke()'s gates); reward within 1e-5 D.  The rows reset_episodes() returns first
    are held to the same gates.  (The half-widths are tests/episode_random_cases.HALF for both rules: "trunc" stayed inside every gate at
    them, so none was shrunk for this test; the rpy half-width is 0.03 rad for the oracle-only cap that file states.)"""
    r = RC.oracle_run(E, D, name)
    close = r["margin"] < NEAR
    first = np.where(close.any(axis=0), close.argmax(axis=0), T)
    assert (first < T).sum() <= 0.10 * E
    keep = np.arange(T)[:, None] < first[None, :]
    assert int(((r["flags"] & 3) != 0)[keep].sum()) >= 20
    env, acts = make_env(mds, E, D, name, "float32")
    rows0 = host(env.reset_episodes()).reshape(-1, 20)
    obs_log, reward_log, flags_log = make_logs(mds, env, T)
    env.rollout_episodes(acts, 0, 50, obs_log, reward_log, flags_log, steps_per_launch=8)
    env.rollout_episodes(acts, 50, T - 50, obs_log, reward_log, flags_log, steps_per_launch=8)
    env.close()
    flags, reward, obs = flags_log.cpu().numpy(), host(reward_log), host(obs_log).reshape(T, E, D, 20)
    want = r["obs"].reshape(T, E, D, 20)
    print(f"{E}x{D} {name}: envs cut short {(first < T).sum()}, flags differing in the compared part {(flags != r['flags'])[keep].sum()}, "
          f"max reward err {np.abs(reward - r['reward'])[keep].max():.2e}, max state err {np.abs(obs - want)[keep][..., :16].max():.2e}, "
          f"max start err {np.abs(rows0 - r['first_rows'])[:, :16].max():.2e}")
    np.testing.assert_allclose(rows0[:, :16], r["first_rows"][:, :16], rtol=0, atol=1e-5)
    assert (rows0[:, 16:] == 0).all()
    np.testing.assert_array_equal(flags[keep], r["flags"][keep])
    np.testing.assert_allclose(reward[keep], r["reward"][keep], rtol=0, atol=1e-5 * D)
    np.testing.assert_allclose(obs[keep][..., :16], want[keep][..., :16], rtol=0, atol=1e-5)
    np.testing.assert_allclose(obs[keep][..., 16:], want[keep][..., 16:], rtol=1e-5, atol=0)


# ---------------------------------------------------------------------------------------------------------------- 3. bitwise invariants
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("E,D", [(37, 7), (200, 2)])
def test_steps_per_launch_changes_no_bit(mds, E, D, dtype):
    """1, 8 and 50 control steps per launch: the same observation, logs, counters and state, bit for bit"""
    runs = []
    for spl in (1, 8, 50):
        env, acts = make_env(mds, E, D, "combined", dtype)
        runs.append(fly(mds, env, acts, T, spl))
        env.close()
    assert int(((runs[0]["flags"] & 3) != 0).sum()) >= 20
    assert_same(mds, runs[0], runs[1])
    assert_same(mds, runs[0], runs[2])


def shards(mds, E, D, cut, dtype, steps, spl=8):
    """the whole set as one handle, and its envs [0, cut) and [cut, E) as two handles with first_env 0 and cut"""
    xyz, rpy, actions, params = EC.scenario(E, D, "combined")
    actions = actions.reshape(EC.N_SETS, E, D, 4)
    env, acts = build_env(mds, xyz, rpy, actions, params, dtype)
    whole = fly(mds, env, acts, steps, spl)
    env.close()
    parts = []
    for a, b in ((0, cut), (cut, E)):
        env, acts = build_env(mds, xyz[a:b], rpy[a:b], actions[:, a:b], params, dtype, first_env=a)
        parts.append((slice(a, b), fly(mds, env, acts, steps, spl)))
        env.close()
    return whole, parts


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_a_sharded_env_set_draws_what_the_whole_set_draws(mds, dtype):
    """40 x 7 as one handle == two handles of 20 envs with first_env 0 and 20, given the matching slices of poses and actions"""
    whole, parts = shards(mds, 40, 7, 20, dtype, T)
    assert int(((whole["flags"] & 3) != 0).sum()) >= 20
    for sl, part in parts:
        assert_same(mds, whole, part, sl)
    assert not mds.torch.equal(parts[0][1]["first"], parts[1][1]["first"])


@pytest.mark.parametrize("dtype", ["float32", "float64", "float16"])
def test_zero_half_widths_are_the_plain_reset(mds, dtype):
    """All half-widths 0 == a handle with randomisation not configured, bit for bit; and reset_episodes() then writes the reset image"""
    E, D = (38, 7) if dtype == "float16" else (37, 7)
    zero = dict(pos=0.0, rpy=0.0, vel=0.0, rate=0.0)
    plain, acts = make_env(mds, E, D, "combined", dtype, rand=False)
    state0, rows0 = plain.get_state(), plain._computeObs().clone()
    a = fly(mds, plain, acts, T, 8, reset=False)
    plain.close()
    env, acts = make_env(mds, E, D, "combined", dtype, half=zero)
    b = fly(mds, env, acts, T, 8, reset=False)
    assert int(((a["flags"] & 3) != 0).sum()) >= 20
    assert_same(mds, a, b)
    assert mds.torch.equal(env.reset_episodes(), rows0)
    np.testing.assert_array_equal(env.get_state(), state0)
    env.close()


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_the_seed_decides_the_draws(mds, dtype):
    """The same seed twice: equal results.  Another seed: another observation."""
    E, D = 37, 7
    runs = []
    for seed in (RC.SEED, RC.SEED, RC.SEED + 1):
        env, acts = make_env(mds, E, D, "combined", dtype, seed=seed)
        runs.append(fly(mds, env, acts, T, 8))
        env.close()
    assert_same(mds, runs[0], runs[1])
    assert not mds.torch.equal(runs[0]["now"], runs[2]["now"]) and not mds.torch.equal(runs[0]["first"], runs[2]["first"])


@pytest.mark.parametrize("E,D,cut", [(130, 1, 64), (200, 2, 100), (38, 7, 20), (17, 16, 8)])
def test_fp16_storage_shards_and_seeds(mds, E, D, cut):
    """fp16 storage, the shapes of test_episode_gpu.FP16_SHAPES: the shard invariant (the cut leaves both shards an even number of drones,
    as 40 x 7 cut at 20 does) and the same-seed invariant.  (Across chunk sizes the fp16 state is rounded at launch ends already without
    randomisation: no chunking invariant is asked for.)"""
    assert (E, D) in FP16_SHAPES and (cut * D) % 2 == 0 and ((E - cut) * D) % 2 == 0
    whole, parts = shards(mds, E, D, cut, "float16", 60)
    assert int(((whole["flags"] & 3) != 0).sum()) >= 20
    for sl, part in parts:
        assert_same(mds, whole, part, sl)
    env, acts = make_env(mds, E, D, "combined", "float16")
    again = fly(mds, env, acts, 60, 8)
    env.close()
    assert_same(mds, whole, again)


@pytest.mark.parametrize("E,D", FP16_SHAPES)
def test_fp16_storage_start_is_the_oracles_start_rounded(mds, E, D):
    """fp16 storage: the freshly reset state within 2^-11 relative -- half an fp16 ulp -- plus 1e-7 absolute of the oracle's start state, for
    generation 1 and 2; the returned rows carry the stored position, quaternion and velocity.  The nominal positions are put on a 2^-6 m
    grid, exact in fp16 up to 32 m: the image's position then carries no rounding of its own and the stored start is rounded once."""
    xyz, rpy, actions, params = EC.scenario(E, D, "combined")
    xyz = np.round(xyz * 64.0) / 64.0
    env, _ = build_env(mds, xyz, rpy, actions.reshape(EC.N_SETS, E, D, 4), params, "float16")
    g = np.arange(E * D)
    for generation in (1, 2):
        rows = host(env.reset_episodes()).reshape(-1, 20)
        got = env.get_state().reshape(-1, 13)
        want = RO.start_state(RC.SEED, g, np.zeros(E * D), generation, RO.half_widths(**RC.HALF), xyz.reshape(-1, 3), rpy.reshape(-1, 3))
        err = np.abs(got - want) - (2.0 ** -11 * np.abs(want) + 1e-7)
        print(f"{E}x{D} float16 generation {generation}: max |err| - bound = {err.max():.3e} (max |err| {np.abs(got - want).max():.3e})")
        assert (err <= 0).all()
        np.testing.assert_array_equal(rows[:, np.r_[0:7, 10:13]], got[:, 0:10])
    env.close()


# ---------------------------------------------------------------------------------------------------------------- 4. with the safety set
def test_f64_with_the_safety_set_matches_oracle(mds):
    """37 x 7, float64, set_episode_safety on: flags (bits 14 and 15 included) equal the oracle's, h_min_episode within 1e-9 and +inf again
    after reset_episodes(); and 1 step per launch == 8 steps per launch, bitwise."""
    torch = mds.torch
    E, D = RC.SAFETY_SHAPE
    r = RC.safety_oracle_run(E, D)
    xyz, rpy, actions, params, obstacles = SC.scenario(E, D)

    def make():
        env, acts = build_env(mds, xyz, rpy, actions.reshape(EC.N_SETS, E, D, 4), params, "float64", rand=False)
        env.set_episode_safety(SC.SAFETY_RADIUS, SC.ZSCALE, obstacles)
        env.set_episode_randomisation(RC.SEED, **RC.HALF)
        return env, acts
    env, acts = make()
    np.testing.assert_allclose(host(env.reset_episodes()).reshape(-1, 20), r["first_rows"], rtol=1e-9, atol=1e-9)
    obs_log, reward_log, flags_log = make_logs(mds, env, T)
    for k in range(T):
        now = host(env.rollout_episodes(acts, k, 1, obs_log, reward_log, flags_log)).reshape(-1, 20)
        np.testing.assert_allclose(now, r["obs_now"][k], rtol=1e-9, atol=1e-9, err_msg=f"obs_now after step {k}")
        hs = {key: host(v) for key, v in env.episode_safety().items()}
        np.testing.assert_allclose(hs["h_min_step"], r["h_min_step"][k], rtol=1e-9, atol=1e-9, err_msg=f"h_min_step after step {k}")
        np.testing.assert_allclose(hs["h_min_episode"], r["h_min_episode"][k], rtol=1e-9, atol=1e-9, err_msg=f"h_min_episode after step {k}")
    one = dict(obs=obs_log, reward=reward_log, flags=flags_log, now=env._obs.clone(), first=None,
               counters={k: v.clone() for k, v in env.episode_counters().items()}, state=env.get_state())
    assert torch.isfinite(env.episode_safety()["h_min_episode"]).any()
    np.testing.assert_allclose(host(env.reset_episodes()).reshape(-1, 20), r["last_rows"], rtol=1e-9, atol=1e-9)
    assert torch.isinf(env.episode_safety()["h_min_episode"]).all() and (env.episode_safety()["h_min_episode"] > 0).all()
    env.close()
    flags = flags_log.cpu().numpy().astype(np.int64)
    print(f"{E}x{D} float64 with safety: pair events {((flags >> 14) & 1).sum()}, done-events {((flags & 3) != 0).sum()}")
    np.testing.assert_array_equal(flags, r["flags"])
    assert int(((flags >> 14) & 1).sum()) >= 1
    np.testing.assert_allclose(host(reward_log), r["reward"], rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(host(obs_log).reshape(T, -1, 20), r["obs"], rtol=1e-9, atol=1e-9)
    env, acts = make()
    env.reset_episodes()
    eight = fly(mds, env, acts, T, 8, reset=False)
    env.close()
    assert_same(mds, one, eight)


# ---------------------------------------------------------------------------------------------------------------- 5. lifecycle
def test_lifecycle_and_error_codes(mds):
    """MDS_ESTATE before set_episodes; every bad argument MDS_EINVAL, the handle keeping the configuration it had (it draws as before);
    set_episodes(enabled=False) switches randomisation off: with episodes configured again the handle resets nominally."""
    lib = capi.load_library()
    E, D = 37, 7
    xyz, rpy, actions, params = EC.scenario(E, D, "combined")
    actions = actions.reshape(EC.N_SETS, E, D, 4)
    good = capi.MdsEpisodeRandomisation()
    good.seed, good.first_env = RC.SEED, 0
    env = mds.CtrlAviary(drone_model=mds.DroneModel.CF2P, num_drones=D, initial_xyzs=xyz, initial_rpys=rpy, physics=mds.Physics.PYB_DRAG,
                         pyb_freq=EC.PYB_FREQ, ctrl_freq=EC.CTRL_FREQ, num_envs=E, dtype="float32")
    assert lib.mds_set_episode_randomisation(env._h, C.byref(good), None) == -5
    assert lib.mds_reset_episodes(env._h, None, None) == -5
    with pytest.raises(capi.MdsError):
        env.set_episode_randomisation(1, pos=0.01)
    env.set_episodes(**params)
    assert lib.mds_reset_episodes(env._h, None, None) == -5                      # episodes, but no randomisation yet
    env.close()
    # a run to compare with; then the same with refused calls in between
    env, acts = build_env(mds, xyz, rpy, actions, params, "float32")
    want = fly(mds, env, acts, 60, 8)
    env.close()
    env, acts = build_env(mds, xyz, rpy, actions, params, "float32")
    for group in ("pos", "rpy", "vel", "rate"):
        for bad in (-0.01, np.nan, np.inf):
            p = capi.MdsEpisodeRandomisation()
            p.seed = 5
            getattr(p, group)[1] = bad
            assert lib.mds_set_episode_randomisation(env._h, C.byref(p), None) == -1, (group, bad)
    for first_env in (-1, 2 ** 32, (2 ** 32 - 1) // D - E + 1):
        p = capi.MdsEpisodeRandomisation()
        p.first_env = first_env
        assert lib.mds_set_episode_randomisation(env._h, C.byref(p), None) == -1, first_env
    with pytest.raises(capi.MdsError):
        env.set_episode_randomisation(5, vel=[0.1, -0.1, 0.1])
    assert_same(mds, want, fly(mds, env, acts, 60, 8))
    p = capi.MdsEpisodeRandomisation()
    p.first_env = (2 ** 32 - 1) // D - E                                        # the largest shard offset that fits
    assert lib.mds_set_episode_randomisation(env._h, C.byref(p), None) == 0
    assert lib.mds_reset_episodes(env._h, C.c_void_p(env._obs.data_ptr() + 4), None) == -4
    # switched off with the episodes; configured again the handle is the one that never had it
    env.set_episodes(enabled=False)
    env.reset()
    env.set_episodes(**params)
    assert lib.mds_reset_episodes(env._h, None, None) == -5
    got = fly(mds, env, acts, 60, 8, reset=False)
    env.close()
    never, acts = build_env(mds, xyz, rpy, actions, params, "float32", rand=False)
    assert_same(mds, fly(mds, never, acts, 60, 8, reset=False), got)
    assert not mds.torch.equal(got["now"], want["now"])
    # mds_reset and mds_reset_async keep it and still write the nominal poses; enabled=False switches it off alone
    never.reset()
    rows0 = never._computeObs().clone()
    never.set_episode_randomisation(RC.SEED, **RC.HALF)
    never.reset()
    assert mds.torch.equal(never._computeObs(), rows0)
    assert lib.mds_reset_async(never._h, never._stream()) == 0
    assert mds.torch.equal(never._computeObs(), rows0)
    assert not mds.torch.equal(never.reset_episodes(), rows0)
    never.set_episode_randomisation(enabled=False)
    assert lib.mds_reset_episodes(never._h, None, None) == -5
    never.close()

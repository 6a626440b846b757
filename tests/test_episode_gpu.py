"""Per-env episodes on the device (mds_set_episodes / mds_rollout_episodes / mds_step_episodes) against the float64 oracle of
tests/episode_oracle.py, on the shapes that cross every boundary of the kernel's thread mapping (tests/episode_cases.py)."""
import ctypes as C

import numpy as np
import pytest

from multidronesim_amd import _capi as capi
from tests import episode_cases as EC
from tests import episode_oracle as EO

pytestmark = pytest.mark.gpu
NEAR = 1e-4
FP16_SHAPES = [(130, 1), (200, 2), (38, 7), (17, 16)]           # fp16 rows are 40 bytes: a log ring needs an even number of drones


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


def make_env(mds, E, D, name, dtype, episodes=True, params=None):
    xyz, rpy, actions, p = EC.scenario(E, D, name)
    p = dict(p if params is None else params)
    env = mds.CtrlAviary(drone_model=mds.DroneModel.CF2P, num_drones=D, initial_xyzs=xyz, initial_rpys=rpy, physics=mds.Physics.PYB_DRAG,
                         pyb_freq=EC.PYB_FREQ, ctrl_freq=EC.CTRL_FREQ, num_envs=E, dtype=dtype)
    if episodes:
        env.set_episodes(**p)
    acts = mds.torch.as_tensor(actions.reshape(EC.N_SETS, E, D, 4), device="cuda").to(env.dtype).contiguous()
    return env, acts, p, xyz


def make_logs(mds, env, T):
    torch, E, D = mds.torch, env.NUM_ENVS, env.NUM_DRONES
    rdt = torch.float64 if env.dtype == torch.float64 else torch.float32
    return (torch.zeros((T, E, D, 20), dtype=env.dtype, device="cuda"), torch.zeros((T, E), dtype=rdt, device="cuda"),
            torch.full((T, E), -1, dtype=torch.int32, device="cuda"))


def host(t):
    return t.detach().double().cpu().numpy()


def counters(env):
    return {k: v.cpu().numpy().astype(np.float64 if v.is_floating_point() else np.int64) for k, v in env.episode_counters().items()}


def stepwise(mds, env, acts, T):
    """T control steps, one call each (first_step continues): logs, and after every step the current observation and the counters"""
    obs_log, reward_log, flags_log = make_logs(mds, env, T)
    now, cnt = [], []
    for k in range(T):
        o = env.rollout_episodes(acts, k, 1, obs_log, reward_log, flags_log)
        now.append(host(o).reshape(-1, 20))
        cnt.append(counters(env))
    return host(obs_log).reshape(T, -1, 20), host(reward_log), flags_log.cpu().numpy().astype(np.int64), np.stack(now), cnt


@pytest.mark.parametrize("name", list(EC.RULES))
@pytest.mark.parametrize("E,D", EC.SHAPES)
def test_f64_matches_oracle(mds, E, D, name):
    """float64, 120 steps: flags (cause bits included) and counters equal the oracle's at every step; reward, the logged (pre-reset) rows
    and the current (post-reset) observation within rtol = atol = 1e-9 -- one launch per step, and 8 steps per launch in a split call."""
    r = EC.oracle_run(E, D, name)
    T = EC.STEPS
    env, acts, _, _ = make_env(mds, E, D, name, "float64")
    obs, reward, flags, now, cnt = stepwise(mds, env, acts, T)
    env.close()
    np.testing.assert_array_equal(flags, r["flags"])
    np.testing.assert_allclose(reward, r["reward"], rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(obs, r["obs"], rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(now, r["obs_now"], rtol=1e-9, atol=1e-9)
    for k in range(T):
        for key, want in r["counters"][k].items():
            if want.dtype.kind == "i":
                np.testing.assert_array_equal(cnt[k][key], want, err_msg=f"{key} after step {k}")
            else:
                np.testing.assert_allclose(cnt[k][key], want, rtol=1e-9, atol=1e-9, err_msg=f"{key} after step {k}")
    # 8 steps per launch, the call split at a step that is no multiple of 8
    env, acts, _, _ = make_env(mds, E, D, name, "float64")
    obs_log, reward_log, flags_log = make_logs(mds, env, T)
    for k0, k1 in ((0, 75), (75, T)):
        now8 = host(env.rollout_episodes(acts, k0, k1 - k0, obs_log, reward_log, flags_log, steps_per_launch=8)).reshape(-1, 20)
        np.testing.assert_allclose(now8, r["obs_now"][k1 - 1], rtol=1e-9, atol=1e-9)
        c8 = counters(env)
        for key, want in r["counters"][k1 - 1].items():
            np.testing.assert_allclose(c8[key], want, rtol=1e-9, atol=1e-9, err_msg=f"{key} after step {k1 - 1}")
    env.close()
    np.testing.assert_array_equal(flags_log.cpu().numpy(), r["flags"])
    np.testing.assert_allclose(host(reward_log), r["reward"], rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(host(obs_log).reshape(T, -1, 20), r["obs"], rtol=1e-9, atol=1e-9)


@pytest.mark.parametrize("name", list(EC.RULES))
@pytest.mark.parametrize("E,D", EC.SHAPES)
def test_f32_matches_oracle_up_to_the_first_close_call(mds, E, D, name):
    """float32 against the oracle under the margin rule: an env is compared up to, not including, its first step whose margin is under 1e-4
    (from there on a decision may legitimately go the other way).  At most 10 % of the envs are cut short, at least 20 done-events are
    compared.  Flags equal; state columns within 1e-5 absolute, RPM columns within 1e-5 relative (smoke()'s gates); reward within 1e-5 D."""
    r = EC.oracle_run(E, D, name)
    T = EC.STEPS
    close = r["margin"] < NEAR
    first = np.where(close.any(axis=0), close.argmax(axis=0), T)               # [E]: steps compared per env
    assert (first < T).sum() <= 0.10 * E
    keep = np.arange(T)[:, None] < first[None, :]                              # [T, E]
    assert int(((r["flags"] & 3) != 0)[keep].sum()) >= 20
    env, acts, _, _ = make_env(mds, E, D, name, "float32")
    obs_log, reward_log, flags_log = make_logs(mds, env, T)
    env.rollout_episodes(acts, 0, 50, obs_log, reward_log, flags_log, steps_per_launch=8)
    env.rollout_episodes(acts, 50, T - 50, obs_log, reward_log, flags_log, steps_per_launch=8)
    env.close()
    flags, reward, obs = flags_log.cpu().numpy(), host(reward_log), host(obs_log).reshape(T, E, D, 20)
    want = r["obs"].reshape(T, E, D, 20)
    print(f"{E}x{D} {name}: envs cut short {(first < T).sum()}, flags differing in the compared part {(flags != r['flags'])[keep].sum()}, "
          f"max reward err {np.abs(reward - r['reward'])[keep].max():.2e}")
    np.testing.assert_array_equal(flags[keep], r["flags"][keep])
    np.testing.assert_allclose(reward[keep], r["reward"][keep], rtol=0, atol=1e-5 * D)
    np.testing.assert_allclose(obs[keep][..., :16], want[keep][..., :16], rtol=0, atol=1e-5)
    np.testing.assert_allclose(obs[keep][..., 16:], want[keep][..., 16:], rtol=1e-5, atol=0)


@pytest.mark.parametrize("dtype", ["float32", "float16", "float64"])
def test_device_reset_is_the_librarys_reset(mds, dtype):
    """After a step in which an env was done, its drones' state (get_state) and its rows of the current observation are bitwise those of a
    fresh handle after mds_reset; the other envs' rows are not touched by it."""
    E, D = (38, 7) if dtype == "float16" else (37, 7)
    fresh, _, _, _ = make_env(mds, E, D, "combined", dtype, episodes=False)
    state0, obs0 = fresh.get_state(), host(fresh._computeObs())
    fresh.close()
    env, acts, _, _ = make_env(mds, E, D, "combined", dtype)
    _, _, flags_log = make_logs(mds, env, 1)
    events = 0
    for k in range(EC.STEPS):
        obs = host(env.rollout_episodes(acts, k, 1, None, None, flags_log))
        done = (flags_log[0].cpu().numpy() & 3) != 0
        if done.any():
            st = env.get_state()
            np.testing.assert_array_equal(st[done], state0[done])
            np.testing.assert_array_equal(obs[done], obs0[done])
            assert not (st[~done][..., 7:] == 0).all()                         # (the others fly on)
            events += int(done.sum())
        if events >= 20 and k >= 40:
            break
    env.close()
    assert events >= 20


def recompute(params, obs, home, E, D, flags_gpu):
    """flags recomputed in float64 from logged rows [T, n, 20], with the episode lengths the GPU's own flags imply; and the margin [T, E]"""
    T = obs.shape[0]
    length = np.zeros(E, dtype=np.int64)
    flags, margin, ended = np.zeros((T, E), dtype=np.int64), np.zeros((T, E)), []
    for k in range(T):
        cause, m = EO.causes_from_obs(params, obs[k], home)
        length += 1
        flags[k] = EO.env_flags(params, np.bitwise_or.reduce(cause.reshape(E, D), axis=1), length)
        margin[k] = m.reshape(E, D).min(axis=1)
        done = (flags_gpu[k] & 3) != 0
        ended.append(np.where(done, length, 0))
        length[done] = 0
    return flags, margin, np.stack(ended), length


@pytest.mark.parametrize("dtype,band", [("float32", 1e-4), ("float64", 1e-4), ("float16", 1e-2)])
@pytest.mark.parametrize("shape", range(4))
def test_self_consistency(mds, shape, dtype, band):
    """Every dtype, fp16 storage included: the flags recomputed in float64 from the GPU's own logged rows match wherever the recomputed margin
    exceeds the band (1e-4; 1e-2 for fp16, whose rows are rounded to 2^-11), at least half of the done-events lying outside it; and the
    invariants of flags and counters.  fp16: max_dist is 0.1 instead of 0.035 -- a world-frame fp16 row near z = 1 is rounded by up to
    2^-11 = 4.9e-4 m, 1.4e-2 of 0.035 and so above the band, 4.9e-3 of 0.1 -- and max_steps 15 instead of 30: the rates grow by ~3 % of
    max_rate per step, so about a third of the rate terminations fall inside a band of +-1 % whatever the seed; the (exact) truncations
    bring the share of done-events outside the band above one half on every shape (probed on the oracle: 82 % at 17 x 16)."""
    E, D = (FP16_SHAPES if dtype == "float16" else EC.SHAPES)[shape]
    T = EC.STEPS
    params = dict(EC.COMBINED, max_dist=0.1, max_steps=15) if dtype == "float16" else None
    env, acts, p, xyz = make_env(mds, E, D, "combined", dtype, params=params)
    obs_log, reward_log, flags_log = make_logs(mds, env, T)
    env.rollout_episodes(acts, 0, 33, obs_log, reward_log, flags_log, steps_per_launch=8)
    env.rollout_episodes(acts, 33, T - 33, obs_log, reward_log, flags_log, steps_per_launch=8)
    cnt = counters(env)
    env.close()
    flags, obs = flags_log.cpu().numpy().astype(np.int64), host(obs_log).reshape(T, E * D, 20)
    home = host(mds.torch.as_tensor(xyz.reshape(-1, 3)).to(env.dtype))                     # the stored, storage-rounded reset position
    want, margin, ended, length = recompute(p, obs, home, E, D, flags)
    clear, done = margin > band, (flags & 3) != 0
    print(f"{E}x{D} {dtype}: done-events {done.sum()}, outside the band {(done & clear).sum()}, flags differing outside it {(flags != want)[clear].sum()}")
    assert (done & clear).sum() >= 0.5 * done.sum() and done.sum() >= 20
    np.testing.assert_array_equal(flags[clear], want[clear])
    term, trunc, causes = (flags & 1) != 0, (flags & 2) != 0, flags >> 8
    assert not (term & trunc).any() and ((causes != 0) == term).all() and (flags & ~(3 | (63 << 8)) == 0).all()
    assert ended.max() <= p["max_steps"] and (ended[trunc] == p["max_steps"]).all()
    np.testing.assert_array_equal(cnt["count"], done.sum(axis=0))
    np.testing.assert_array_equal(cnt["sum_length"], ended.sum(axis=0))
    np.testing.assert_array_equal(cnt["length"], length)
    assert (cnt["length"] < p["max_steps"]).all()
    # the returns: the logged rewards summed per episode (float64 sums of the logged values: equal to rounding of the compute type)
    reward = host(reward_log)
    ret, total = np.zeros(E), np.zeros(E)
    for k in range(T):
        ret += reward[k]
        total += np.where(done[k], ret, 0.0)
        ret[done[k]] = 0.0
    tol = 1e-12 if dtype == "float64" else 1e-5
    np.testing.assert_allclose(cnt["sum_return"], total, rtol=tol, atol=tol)
    np.testing.assert_allclose(cnt["ret"], ret, rtol=tol, atol=tol)


@pytest.mark.parametrize("dtype,tol", [("float32", 0.0), ("float64", 0.0), ("float16", 5e-2)])
def test_env_never_done_steps_like_rollout_step(mds, dtype, tol):
    """An env with no done flag has the state of mds_rollout_step (episode_len 0) on the same table: the kernel's step is built from k_step's
    pieces, so at one step per launch the float32 / float64 states are bitwise equal (fp16: the tolerance of
    test_fused_rollout_step_equals_stepwise)."""
    E, D, T = 38 if dtype == "float16" else 37, 7, 30
    env, acts, _, _ = make_env(mds, E, D, "tilt", dtype)
    _, _, flags_log = make_logs(mds, env, T)
    env.rollout_episodes(acts, 0, T, None, None, flags_log)
    got = env.get_state()
    env.close()
    ref, acts, _, _ = make_env(mds, E, D, "tilt", dtype, episodes=False)
    ref.rollout_step(acts, 0, T)
    want = ref.get_state()
    ref.close()
    never = ((flags_log.cpu().numpy() & 3) == 0).all(axis=0)
    assert 0 < never.sum() < E
    if tol == 0.0:
        np.testing.assert_array_equal(got[never], want[never])
    else:
        assert (np.abs(got[never] - want[never]) / np.maximum(1.0, np.abs(want[never]))).max() < tol
    assert not np.array_equal(got[~never], want[~never])


@pytest.mark.parametrize("dtype", ["float32", "float16", "float64"])
def test_step_episodes_loop_equals_rollout(mds, dtype):
    """mds_step_episodes in a Python loop == mds_rollout_episodes with one step per launch, bitwise: observation, the transition's rows,
    reward, flags, counters, state."""
    torch = mds.torch
    E, D, T = 38, 7, 40
    a, acts, _, _ = make_env(mds, E, D, "combined", dtype)
    b, _, _, _ = make_env(mds, E, D, "combined", dtype)
    obs_log, reward_log, flags_log = make_logs(mds, b, T)
    final = torch.zeros((E, D, 20), dtype=a.dtype, device="cuda")
    seen_done = 0
    for k in range(T):
        obs, reward, terminated, truncated, info = a.step_episodes(acts[k % EC.N_SETS], final_obs=final)
        now = b.rollout_episodes(acts, k, 1, obs_log, reward_log, flags_log)
        assert torch.equal(obs, now) and torch.equal(final, obs_log[k]) and torch.equal(reward, reward_log[k])
        assert torch.equal(info["flags"], flags_log[k])
        assert torch.equal(terminated, (flags_log[k] & 1) != 0) and torch.equal(truncated, (flags_log[k] & 2) != 0)
        seen_done += int((terminated | truncated).sum())
    assert seen_done >= 20
    ca, cb = a.episode_counters(), b.episode_counters()
    assert all(torch.equal(ca[k], cb[k]) for k in ca)
    np.testing.assert_array_equal(a.get_state(), b.get_state())
    a.close()
    b.close()


def test_existing_calls_are_unchanged_by_configured_episodes(mds):
    """step() and rollout_step() on a handle with episodes configured: the same bits as on one without"""
    torch = mds.torch
    E, D = 37, 7
    a, acts, _, _ = make_env(mds, E, D, "combined", "float32")
    b, _, _, _ = make_env(mds, E, D, "combined", "float32", episodes=False)
    for env in (a, b):
        env.step(acts[0])
        env.log = torch.zeros((3, E, D, 20), dtype=env.dtype, device="cuda")
        env.rollout_step(acts, 1, 40, env.log, episode_len=13, steps_per_launch=8)
        env.out = env.step(acts[1])
    assert torch.equal(a.log, b.log) and torch.equal(a.out[0], b.out[0])
    assert a.out[1:4] == b.out[1:4] == (-1, False, False)
    np.testing.assert_array_equal(a.get_state(), b.get_state())
    a.close()
    b.close()


def test_refusals(mds):
    """MDS_F32C and ground-effect handles: MDS_EUNSUPPORTED; no mds_reset yet: MDS_ESTATE; a rollout before mds_set_episodes: MDS_ESTATE; a
    misaligned log: MDS_EALIGN."""
    lib = capi.load_library()
    p = capi.MdsEpisodeParams()
    assert lib.mds_default_episode_params(C.byref(p)) == 0
    xyz, rpy = np.zeros((4, 2, 3)), np.zeros((4, 2, 3))
    xyz[..., 2] = 1.0
    kw = dict(drone_model=mds.DroneModel.CF2P, num_drones=2, initial_xyzs=xyz, initial_rpys=rpy, num_envs=4)
    for env in (mds.CtrlAviary(physics=mds.Physics.DYN, dtype="float32c", **kw), mds.CtrlAviary(physics=mds.Physics.PYB_GND, **kw)):
        assert lib.mds_set_episodes(env._h, C.byref(p), None, None) == -6
        with pytest.raises(capi.MdsError):
            env.set_episodes(max_steps=5)
        env.close()
    cfg = capi.MdsConfig()
    assert lib.mds_default_config(capi.MDS_CF2P, C.byref(cfg)) == 0
    cfg.num_envs, cfg.num_drones, cfg.device = 4, 2, mds.torch.cuda.current_device()
    h = C.c_void_p()
    assert lib.mds_create(C.byref(cfg), C.byref(h)) == 0
    assert lib.mds_set_episodes(h, C.byref(p), None, None) == -5
    assert lib.mds_destroy(h) == 0
    env = mds.CtrlAviary(physics=mds.Physics.DYN, **kw)
    acts = mds.torch.zeros((1, 4, 2, 4), device="cuda")
    log = mds.torch.zeros((2 * 8 * 20 + 4,), device="cuda")
    args = (C.c_void_p(acts.data_ptr()), 1, 0, 1)
    assert lib.mds_rollout_episodes(env._h, *args, None, 0, None, None, 1, None, None) == -5
    env.set_episodes(max_steps=5)
    assert lib.mds_rollout_episodes(env._h, *args, C.c_void_p(log.data_ptr() + 4), 2, None, None, 1, None, None) == -4
    assert lib.mds_rollout_episodes(env._h, *args, C.c_void_p(log.data_ptr()), 2, None, None, 1, C.c_void_p(log.data_ptr() + 8), None) == -4
    assert lib.mds_rollout_episodes(env._h, *args, C.c_void_p(log.data_ptr()), 2, None, None, 0, None, None) == -1
    assert lib.mds_rollout_episodes(env._h, *args, C.c_void_p(log.data_ptr()), 2, None, None, 1, None, None) == 0
    env.set_episodes(enabled=False)
    assert lib.mds_rollout_episodes(env._h, *args, None, 0, None, None, 1, None, None) == -5
    env.close()

"""An MLP policy inside the episode rollout kernel (mds_set_episode_policy / mds_episode_policy_compute / mds_rollout_episodes_policy)
against the float64 oracle of tests/episode_policy_oracle.py, on the shapes that cross every boundary of the kernel's thread mapping
(tests/episode_policy_cases.py)."""
import ctypes as C
import types

import numpy as np
import pytest

from multidronesim_amd import _capi as capi
from tests import episode_cases as EC
from tests import episode_policy_cases as PC
from tests import episode_policy_oracle as PO
from tests import episode_random_cases as RC
from tests import episode_safety_cases as SC

pytestmark = pytest.mark.gpu
NEAR = 1e-4


@pytest.fixture(scope="module")
def mds():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no HIP device: -m gpu tests need a real MI355X (there is no CPU fallback)")
    import multidronesim_amd
    multidronesim_amd.load_library()
    from multidronesim_amd.envs.CtrlAviary import CtrlAviary, DroneModel, Physics
    return types.SimpleNamespace(CtrlAviary=CtrlAviary, DroneModel=DroneModel, Physics=Physics, torch=torch)


def make_env(mds, E, D, dtype, policy=True, net=PC.ROLLOUT_NET, xyz=None, rpy=None, params=None, physics=None, integrator="euler"):
    """the flight of tests/episode_policy_cases.py (its poses, rule and targets) unless poses and a rule are given (then: default targets)"""
    target = None
    if xyz is None:
        xyz, rpy, sp, target = PC.scenario(E, D)
        params = sp if params is None else params
    env = mds.CtrlAviary(drone_model=mds.DroneModel.CF2P, num_drones=D, initial_xyzs=xyz, initial_rpys=rpy,
                         physics=mds.Physics.PYB_DRAG if physics is None else physics, pyb_freq=PC.PYB_FREQ, ctrl_freq=PC.CTRL_FREQ, num_envs=E,
                         dtype=dtype, integrator=integrator)
    env.set_episodes(**params, target=target)
    if policy:
        env.set_episode_policy(PC.weights(*net[:2]), *net)
    return env


def make_logs(mds, env, T):
    torch, E, D = mds.torch, env.NUM_ENVS, env.NUM_DRONES
    rdt = torch.float64 if env.dtype == torch.float64 else torch.float32
    return types.SimpleNamespace(obs=torch.zeros((T, E, D, 20), dtype=env.dtype, device="cuda"), act=torch.zeros((T, E, D, 4), dtype=env.dtype, device="cuda"),
                                 reward=torch.zeros((T, E), dtype=rdt, device="cuda"), flags=torch.full((T, E), -1, dtype=torch.int32, device="cuda"))


def roll(env, L, first, n, spl=1):
    return env.rollout_episodes_policy(first, n, L.obs, L.act, L.reward, L.flags, steps_per_launch=spl)


def host(t):
    return t.detach().double().cpu().numpy()


def counters(env):
    return {k: v.cpu().numpy().astype(np.float64 if v.is_floating_point() else np.int64) for k, v in env.episode_counters().items()}


def assert_counters(got, want, tol, msg=""):
    for key, w in want.items():
        if w.dtype.kind == "i":
            np.testing.assert_array_equal(got[key], w, err_msg=f"{key} {msg}")
        else:
            np.testing.assert_allclose(got[key], w, rtol=tol, atol=tol, err_msg=f"{key} {msg}")


@pytest.mark.parametrize("n", [1, 63, 64, 65, 300])
@pytest.mark.parametrize("dtype,tol", [("float64", 1e-12), ("float32", 1e-5)])
def test_policy_compute_alone(mds, dtype, tol, n):
    """episode_policy_compute on random rows, every width, depth and activation of the CPU test: the commanded RPM against the oracle,
    1e-12 relative on a float64 handle, 1e-5 relative (smoke()'s RPM gate) in float32.  The handle's targets are its initial positions."""
    obs, target = PC.observations(n)
    env = make_env(mds, n, 1, dtype, policy=False, xyz=target.reshape(n, 1, 3), rpy=np.zeros((n, 1, 3)), params=dict(max_steps=5))
    rows = mds.torch.as_tensor(obs.reshape(n, 1, 20), device="cuda").to(env.dtype).contiguous()
    for n_hidden, width, act in PC.NETS:
        w = PC.weights(n_hidden, width)
        env.set_episode_policy(w, n_hidden, width, act)
        got = host(env.episode_policy_compute(rows)).reshape(n, 4)
        want, y = PO.policy_rpm(w, n_hidden, width, act, obs, target)
        np.testing.assert_allclose(got, want, rtol=tol, atol=0, err_msg=f"{n_hidden} x {width} {act}")
    # other base and scale, and through the torch module
    net = PC.ROLLOUT_NET
    w = PC.weights(*net[:2])
    env.set_episode_policy(w, *net, rpm_base=12000.0, rpm_scale=900.0)
    want, _ = PO.policy_rpm(w, *net, obs, target, 12000.0, 900.0)
    np.testing.assert_allclose(host(env.episode_policy_compute(rows)).reshape(n, 4), want, rtol=tol, atol=0)
    env.close()


def test_policy_from_torch_module(mds):
    """set_episode_policy_from_torch(nn.Sequential) == set_episode_policy(the flat parameter vector), bitwise"""
    torch = mds.torch
    nn = torch.nn
    n = 65
    obs, target = PC.observations(n)
    env = make_env(mds, n, 1, "float32", policy=False, xyz=target.reshape(n, 1, 3), rpy=np.zeros((n, 1, 3)), params=dict(max_steps=5))
    rows = torch.as_tensor(obs.reshape(n, 1, 20), device="cuda").to(env.dtype).contiguous()
    torch.manual_seed(3)
    net = nn.Sequential(nn.Linear(12, 64), nn.Tanh(), nn.Linear(64, 64), nn.Tanh(), nn.Linear(64, 4))
    env.set_episode_policy_from_torch(net)
    a = env.episode_policy_compute(rows)
    env.set_episode_policy(torch.cat([p.detach().flatten() for p in net.parameters()]), 2, 64, "tanh")
    b = env.episode_policy_compute(rows)
    assert torch.equal(a, b)
    with torch.no_grad():
        y = net.double()(torch.as_tensor(PO.features(obs, target))).numpy()
    np.testing.assert_allclose(host(a).reshape(n, 4), PO.rpm_of(y), rtol=1e-5, atol=0)
    env.close()


@pytest.mark.parametrize("E,D", PC.SHAPES)
def test_rollout_f64_matches_oracle(mds, E, D):
    """float64, 120 steps: flags (cause bits included) and integer counters equal the oracle's at every step; the observation, action and
    reward rings, the current observation and the float counters within rtol = atol = 1e-9 -- one launch per step, and 8 steps per
    launch in a call split at a step that is no multiple of 8."""
    r = PC.oracle_run(E, D)
    T = PC.STEPS
    env = make_env(mds, E, D, "float64")
    L = make_logs(mds, env, T)
    for k in range(T):
        now = host(roll(env, L, k, 1)).reshape(-1, 20)
        np.testing.assert_allclose(now, r["obs_now"][k], rtol=1e-9, atol=1e-9, err_msg=f"current observation after step {k}")
        assert_counters(counters(env), r["counters"][k], 1e-9, f"after step {k}")
    env.close()

    def check(L):
        np.testing.assert_array_equal(L.flags.cpu().numpy(), r["flags"])
        np.testing.assert_allclose(host(L.reward), r["reward"], rtol=1e-9, atol=1e-9)
        np.testing.assert_allclose(host(L.obs).reshape(T, -1, 20), r["obs"], rtol=1e-9, atol=1e-9)
        np.testing.assert_allclose(host(L.act).reshape(T, -1, 4), r["action"], rtol=1e-9, atol=1e-9)
    check(L)
    env = make_env(mds, E, D, "float64")
    L = make_logs(mds, env, T)
    for k0, k1 in ((0, 75), (75, T)):
        now = host(roll(env, L, k0, k1 - k0, 8)).reshape(-1, 20)
        np.testing.assert_allclose(now, r["obs_now"][k1 - 1], rtol=1e-9, atol=1e-9)
        assert_counters(counters(env), r["counters"][k1 - 1], 1e-9, f"after step {k1 - 1}")
    env.close()
    check(L)


@pytest.mark.parametrize("E,D", PC.SHAPES)
def test_rollout_f32_matches_oracle_up_to_the_first_close_call(mds, E, D):
    """float32 against the oracle under the margin rule: an env is compared up to, not including, its first step whose margin is under 1e-4.
    Flags equal; state columns within 1e-5 absolute, RPM columns and the action ring within 1e-5 relative; reward within 1e-5 D.
    (The episodes are at most 12 steps long, tests/episode_policy_cases.RULE says why: in an earlier form of this flight, with the
    sibling's 30-step episodes, the world-frame rate columns reached 1.01e-5, 1.14e-5, 1.02e-5 and 1.46e-5 on the four shapes, 4 to 72
    elements over the gate, all in the last steps of the oldest episodes, with the action ring within 2.7e-7 relative throughout: the
    drift of a float32 closed loop, not of the policy.)"""
    r = PC.oracle_run(E, D)
    T = PC.STEPS
    first, keep = PC.compared_part(r, NEAR)
    assert (first < T).sum() <= 0.10 * E and int(((r["flags"] & 3) != 0)[keep].sum()) >= 20
    env = make_env(mds, E, D, "float32")
    L = make_logs(mds, env, T)
    roll(env, L, 0, 50, 8)
    roll(env, L, 50, T - 50, 8)
    env.close()
    flags, reward = L.flags.cpu().numpy(), host(L.reward)
    obs, act = host(L.obs).reshape(T, E, D, 20), host(L.act).reshape(T, E, D, 4)
    want, want_act = r["obs"].reshape(T, E, D, 20), r["action"].reshape(T, E, D, 4)
    print(f"{E}x{D}: envs cut short {(first < T).sum()}, flags differing in the compared part {(flags != r['flags'])[keep].sum()}, max state err "
          f"{np.abs(obs - want)[keep][..., :16].max():.2e}, action rel err {np.abs(act / want_act - 1)[keep].max():.2e}, "
          f"reward err {np.abs(reward - r['reward'])[keep].max():.2e}")
    np.testing.assert_array_equal(flags[keep], r["flags"][keep])
    np.testing.assert_allclose(reward[keep], r["reward"][keep], rtol=0, atol=1e-5 * D)
    np.testing.assert_allclose(obs[keep][..., :16], want[keep][..., :16], rtol=0, atol=1e-5)
    np.testing.assert_allclose(obs[keep][..., 16:], want[keep][..., 16:], rtol=1e-5, atol=0)
    np.testing.assert_allclose(act[keep], want_act[keep], rtol=1e-5, atol=0)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_launch_form_independence(mds, dtype):
    """steps_per_launch 1 and 8: bit-identical rings, current observation, state and counters (the same kernel and instruction stream; the
    state round-trips through its own storage type exactly)."""
    torch = mds.torch
    E, D, T = 37, 7, 60
    out = []
    for spl in (1, 8):
        env = make_env(mds, E, D, dtype)
        L = make_logs(mds, env, T)
        now = roll(env, L, 0, 27, spl).clone()
        now2 = roll(env, L, 27, T - 27, spl).clone()
        out.append((L, now, now2, env.get_state(), {k: v.clone() for k, v in env.episode_counters().items()}))
        env.close()
    (La, na, na2, sa, ca), (Lb, nb, nb2, sb, cb) = out
    for key in ("obs", "act", "reward", "flags"):
        assert torch.equal(getattr(La, key), getattr(Lb, key)), key
    assert torch.equal(na, nb) and torch.equal(na2, nb2)
    np.testing.assert_array_equal(sa, sb)
    assert all(torch.equal(ca[k], cb[k]) for k in ca)
    assert int(((La.flags & 3) != 0).sum()) >= 20


def test_fused_equals_policy_in_the_loop(mds):
    """rollout_episodes_policy(T) against T rounds of episode_policy_compute(current observation) + step_episodes, float64: within 1e-11
    (the gate between two launch forms that contract FMAs differently; the loop's position feature also goes through the world frame);
    flags and integer counters equal."""
    torch = mds.torch
    E, D, T = 37, 7, 60
    a = make_env(mds, E, D, "float64")
    L = make_logs(mds, a, T)
    now_a = host(roll(a, L, 0, T, 8))
    b = make_env(mds, E, D, "float64")
    obs = b._computeObs()
    flags, reward, acts, rows = [], [], [], []
    final = torch.zeros((E, D, 20), dtype=b.dtype, device="cuda")
    for k in range(T):
        act = b.episode_policy_compute(obs)
        obs, rew, _, _, info = b.step_episodes(act, final_obs=final)
        flags.append(info["flags"].cpu().numpy().copy())
        reward.append(host(rew))
        acts.append(host(act))
        rows.append(host(final))
    np.testing.assert_array_equal(np.stack(flags), L.flags.cpu().numpy())
    np.testing.assert_allclose(np.stack(reward), host(L.reward), rtol=1e-11, atol=1e-11)
    np.testing.assert_allclose(np.stack(acts), host(L.act), rtol=1e-11, atol=1e-11)
    np.testing.assert_allclose(np.stack(rows), host(L.obs), rtol=1e-11, atol=1e-11)
    np.testing.assert_allclose(host(obs), now_a, rtol=1e-11, atol=1e-11)
    assert_counters(counters(b), counters(a), 1e-11)
    assert int(((L.flags & 3) != 0).sum()) >= 20
    a.close()
    b.close()


def test_float64_rk4_runs_the_wide_kernel(mds):
    """A float64 handle with the RK4 integrator (no drag) and a 5-wide policy: the library pads it to 64, not 32 (that combination has no
    32-wide rollout kernel).  The policy alone within 1e-12 relative, the rollout (8 steps per launch, split call) against the RK4
    oracle: flags and integer counters equal, rings and current observation within 1e-9; and a second handle given the same policy
    already padded to width 64 by the caller produces the same bits."""
    torch = mds.torch
    E, D = PC.RK4_SHAPE
    T, net = PC.RK4_STEPS, PC.RK4_NET
    r = PC.rk4_oracle_run()
    assert int(((r["flags"] & 1) != 0).sum()) >= 5 and int(((r["flags"] & 2) != 0).sum()) >= 5
    _, _, _, target = PC.scenario(E, D)
    out = []
    for padded in (False, True):
        env = make_env(mds, E, D, "float64", policy=False, physics=mds.Physics.DYN, integrator="rk4")
        w = PC.weights(*net[:2])
        if padded:
            env.set_episode_policy(PO.pad(w, net[0], net[1], 64), net[0], 64, net[2])
        else:
            env.set_episode_policy(w, *net)
        rows = env._computeObs().clone()
        rpm = env.episode_policy_compute(rows)
        want, _ = PO.policy_rpm(w, *net, host(rows).reshape(-1, 20), target.reshape(-1, 3))
        np.testing.assert_allclose(host(rpm).reshape(-1, 4), want, rtol=1e-12, atol=0)
        L = make_logs(mds, env, T)
        roll(env, L, 0, 27, 8)
        now = roll(env, L, 27, T - 27, 8).clone()
        out.append((L, now, rpm, env.get_state()))
        if not padded:
            np.testing.assert_array_equal(L.flags.cpu().numpy(), r["flags"])
            np.testing.assert_allclose(host(L.reward), r["reward"], rtol=1e-9, atol=1e-9)
            np.testing.assert_allclose(host(L.obs).reshape(T, -1, 20), r["obs"], rtol=1e-9, atol=1e-9)
            np.testing.assert_allclose(host(L.act).reshape(T, -1, 4), r["action"], rtol=1e-9, atol=1e-9)
            np.testing.assert_allclose(host(now).reshape(-1, 20), r["obs_now"][T - 1], rtol=1e-9, atol=1e-9)
            assert_counters(counters(env), r["counters"][T - 1], 1e-9)
        env.close()
    (La, na, ra, sa), (Lb, nb, rb, sb) = out
    assert torch.equal(ra, rb) and torch.equal(na, nb)
    for key in ("obs", "act", "reward", "flags"):
        assert torch.equal(getattr(La, key), getattr(Lb, key)), key
    np.testing.assert_array_equal(sa, sb)


def make_safety_env(mds, dtype, policy=True, params=None):
    E, D = PC.SAFETY_SHAPE
    xyz, rpy, _, p, obstacles = SC.scenario(E, D)
    env = make_env(mds, E, D, dtype, policy=False, xyz=xyz, rpy=rpy, params=p if params is None else params)
    env.set_episode_safety(SC.SAFETY_RADIUS, SC.ZSCALE, obstacles)
    env.set_episode_randomisation(RC.SEED, **RC.HALF)
    if policy:
        env.set_episode_policy(PC.weights(*PC.ROLLOUT_NET[:2]), *PC.ROLLOUT_NET)
    return env


def test_with_safety_and_randomised_starts(mds):
    """(37, 7), float64, collision causes and randomised starts (position and attitude half-widths non-zero) configured: flags equal the
    composed oracle's at every step, bit 14 fires at least 5 times, h_min_step, h_min_episode, the reward ring and the counters within
    1e-9 (integer counters equal), and every restarted
    drone's state is bitwise what mds_rollout_episodes with a table gives a drone restarted with the same (seed, g, ordinal,
    generation) -- read off a second handle whose episodes all end after one step, so that after step j every env has ordinal j."""
    E, D = PC.SAFETY_SHAPE
    T = PC.STEPS
    r = PC.safety_oracle_run()
    assert RC.HALF["pos"] > 0 and RC.HALF["rpy"] > 0
    env = make_safety_env(mds, "float64")
    first = host(env.reset_episodes()).reshape(-1, 20)
    np.testing.assert_allclose(first, r["first_rows"], rtol=1e-9, atol=1e-9)
    L = make_logs(mds, env, T)
    restarted = []                                                              # (step, env, count) of every restart, and the state after it
    for k in range(T):
        roll(env, L, k, 1)
        assert_counters(counters(env), r["counters"][k], 1e-9, f"after step {k}")
        s = env.episode_safety()
        np.testing.assert_allclose(host(s["h_min_step"]), r["h_min_step"][k], rtol=1e-9, atol=1e-9, err_msg=f"h_min_step after step {k}")
        np.testing.assert_allclose(host(s["h_min_episode"]), r["h_min_episode"][k], rtol=1e-9, atol=1e-9, err_msg=f"h_min_episode after step {k}")
        done = (L.flags[k].cpu().numpy() & 3) != 0
        if done.any():
            st, cnt = env.get_state(), counters(env)["count"]
            restarted += [(e, int(cnt[e]), st[e].copy()) for e in np.flatnonzero(done)]
    env.close()
    flags = L.flags.cpu().numpy()
    np.testing.assert_array_equal(flags, r["flags"])
    assert int(((flags >> 14) & 1).sum()) >= 5
    np.testing.assert_allclose(host(L.act).reshape(T, -1, 4), r["action"], rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(host(L.obs).reshape(T, -1, 20), r["obs"], rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(host(L.reward), r["reward"], rtol=1e-9, atol=1e-9)
    # the table-driven handle: every episode ends after one step
    top = max(c for _, c, _ in restarted)
    ref = make_safety_env(mds, "float64", policy=False, params=dict(max_steps=1))
    ref.reset_episodes()
    acts = mds.torch.full((1, E, D, 4), 14000.0, dtype=ref.dtype, device="cuda")
    starts = {}
    for j in range(1, top + 1):
        ref.rollout_episodes(acts, j - 1, 1)
        starts[j] = ref.get_state().copy()
    assert (counters(ref)["count"] == top).all()
    ref.close()
    assert len(restarted) >= 20
    for e, c, st in restarted:
        np.testing.assert_array_equal(st, starts[c][e], err_msg=f"env {e}, ordinal {c}")


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_table_rollout_is_unchanged_by_a_configured_policy(mds, dtype):
    """rollout_episodes with an action table on a handle with a policy configured: the bits of a handle without one"""
    torch = mds.torch
    E, D, T = 37, 7, 60
    _, _, actions, _ = EC.scenario(E, D, "combined")
    out = []
    for policy in (True, False):
        env = make_env(mds, E, D, dtype, policy=policy)
        acts = torch.as_tensor(actions.reshape(EC.N_SETS, E, D, 4), device="cuda").to(env.dtype).contiguous()
        L = make_logs(mds, env, T)
        now = env.rollout_episodes(acts, 0, T, L.obs, L.reward, L.flags, steps_per_launch=8).clone()
        out.append((L, now, env.get_state(), {k: v.clone() for k, v in env.episode_counters().items()}))
        env.close()
    (La, na, sa, ca), (Lb, nb, sb, cb) = out
    assert torch.equal(La.obs, Lb.obs) and torch.equal(La.reward, Lb.reward) and torch.equal(La.flags, Lb.flags) and torch.equal(na, nb)
    np.testing.assert_array_equal(sa, sb)
    assert all(torch.equal(ca[k], cb[k]) for k in ca)
    assert int(((La.flags & 3) != 0).sum()) >= 20


def test_switching_off_and_refusals(mds):
    """set_episodes(enabled=False) switches the policy off: rollout_episodes_policy then returns MDS_ESTATE, also after the episodes are
    configured again.  A failed call leaves the handle as it was.  Reconfiguring rule, safety or randomisation keeps the policy.
    fp16-storage and MDS_F32C handles get MDS_EUNSUPPORTED from mds_set_episode_policy and stay usable."""
    torch = mds.torch
    lib = capi.load_library()
    E, D = 4, 2
    xyz, rpy = np.zeros((E, D, 3)), np.zeros((E, D, 3))
    xyz[..., 2] = 1.0
    xyz[..., 0] = np.arange(D)[None, :]
    net = PC.ROLLOUT_NET
    w = PC.weights(*net[:2])
    p = capi.MdsEpisodePolicy(net[0], net[1], 0, 0, float("nan"), float("nan"))
    wp = capi.as_double_ptr(w)
    call = lambda env: lib.mds_rollout_episodes_policy(env._h, 0, 1, None, 0, None, None, None, 1, None, None)   # noqa: E731
    env = make_env(mds, E, D, "float32", policy=False, xyz=xyz, rpy=rpy, params=dict(max_steps=5))
    assert call(env) == -5                                                      # no policy yet
    assert lib.mds_episode_policy_compute(env._h, C.c_void_p(env._obs.data_ptr()), C.c_void_p(env._obs.data_ptr()), None) == -5
    env.set_episode_policy(w, *net)
    assert call(env) == 0
    # failed calls: the handle keeps its policy
    bad = w.copy()
    bad[7] = np.inf
    assert lib.mds_set_episode_policy(env._h, C.byref(p), capi.as_double_ptr(bad), None) == -1
    for field, value in (("n_hidden", 3), ("n_hidden", 0), ("width", 65), ("width", 0), ("activation", 2), ("rpm_scale", float("inf"))):
        q = capi.MdsEpisodePolicy(net[0], net[1], 0, 0, float("nan"), float("nan"))
        setattr(q, field, value)
        assert lib.mds_set_episode_policy(env._h, C.byref(q), wp, None) == -1, field
    assert lib.mds_set_episode_policy(env._h, C.byref(p), None, None) == -1
    assert call(env) == 0
    # reconfiguration keeps it
    env.set_episodes(max_steps=7)
    env.set_episode_safety(0.05)
    env.set_episode_randomisation(3, pos=0.01)
    assert call(env) == 0
    log = torch.zeros((2 * E * D * 4 + 4,), device="cuda")
    assert lib.mds_rollout_episodes_policy(env._h, 0, 1, None, 2, C.c_void_p(log.data_ptr() + 4), None, None, 1, None, None) == -4
    assert lib.mds_rollout_episodes_policy(env._h, 0, 1, None, 2, C.c_void_p(log.data_ptr()), None, None, 0, None, None) == -1
    # switching off
    env.set_episodes(enabled=False)
    assert call(env) == -5
    with pytest.raises(capi.MdsError):
        env.rollout_episodes_policy(0, 1)
    assert lib.mds_set_episode_policy(env._h, C.byref(p), wp, None) == -5      # needs episodes
    env.set_episodes(max_steps=5)
    assert call(env) == -5                                                      # ... and stays off until configured again
    env.set_episode_policy(w, *net)
    assert call(env) == 0
    env.set_episode_policy(None, 0, 0, enabled=False)
    assert call(env) == -5
    env.close()
    kw = dict(drone_model=mds.DroneModel.CF2P, num_drones=D, initial_xyzs=xyz, initial_rpys=rpy, num_envs=E, physics=mds.Physics.DYN)
    for dtype in ("float16", "float32c"):
        env = mds.CtrlAviary(dtype=dtype, **kw)
        if dtype == "float16":
            env.set_episodes(max_steps=5)
        assert lib.mds_set_episode_policy(env._h, C.byref(p), wp, None) == -6, dtype
        with pytest.raises(capi.MdsError):
            env.set_episode_policy(w, *net)
        obs, *_ = env.step(torch.full((E, D, 4), 14000.0, dtype=env.dtype, device="cuda"))
        assert torch.isfinite(obs.float()).all()
        if dtype == "float16":
            acts = torch.full((1, E, D, 4), 14000.0, dtype=env.dtype, device="cuda")
            assert torch.isfinite(env.rollout_episodes(acts, 0, 3).float()).all()
        env.close()

"""Gaussian actions drawn inside the episode rollout kernel (mds_set_episode_policy_noise / mds_rollout_episodes_sampled /
mds_episode_policy_sample) against the float64 oracle of tests/episode_sample_oracle.py, on the shapes that cross every boundary of the
kernel's thread mapping (tests/episode_sample_cases.py)."""
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
from tests import episode_sample_cases as XC
from tests import episode_sample_oracle as SO

pytestmark = pytest.mark.gpu
NEAR = 1e-4
RINGS = ("acted", "obs", "act", "sample", "logp", "reward", "flags")
SIGMA = np.exp(np.asarray(XC.LOG_STD))


@pytest.fixture(scope="module")
def mds():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no HIP device: -m gpu tests need a real MI355X (there is no CPU fallback)")
    import multidronesim_amd
    multidronesim_amd.load_library()
    from multidronesim_amd.envs.CtrlAviary import CtrlAviary, DroneModel, Physics
    return types.SimpleNamespace(CtrlAviary=CtrlAviary, DroneModel=DroneModel, Physics=Physics, torch=torch)


def build_env(mds, xyz, rpy, params, target, dtype, policy=True, noise=True, first_env=0, log_std=XC.LOG_STD, net=XC.NET, physics=None):
    E, D = xyz.shape[0], xyz.shape[1]
    env = mds.CtrlAviary(drone_model=mds.DroneModel.CF2P, num_drones=D, initial_xyzs=xyz, initial_rpys=rpy,
                         physics=mds.Physics.PYB_DRAG if physics is None else physics,
                         pyb_freq=XC.PYB_FREQ, ctrl_freq=XC.CTRL_FREQ, num_envs=E, dtype=dtype)
    env.set_episodes(**params, target=target)
    if policy:
        env.set_episode_policy(PC.weights(*net[:2]), *net)
        if noise:
            env.set_episode_policy_noise(log_std, XC.NOISE_SEED, first_env=first_env)
    return env


def make_env(mds, E, D, dtype, **kw):
    """the flight of tests/episode_sample_cases.py: its poses, rule, targets, weights, log_std, seed and the shape's first_env"""
    kw.setdefault("first_env", XC.FIRST_ENV[(E, D)])
    return build_env(mds, *PC.scenario(E, D), dtype, **kw)


def make_logs(mds, env, T):
    torch, E, D = mds.torch, env.NUM_ENVS, env.NUM_DRONES
    rdt = torch.float64 if env.dtype == torch.float64 else torch.float32
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")   # noqa: E731
    return types.SimpleNamespace(acted=z((T, E, D, 20), env.dtype), obs=z((T, E, D, 20), env.dtype), act=z((T, E, D, 4), env.dtype),
                                 sample=z((T, E, D, 4), env.dtype), logp=z((T, E, D), rdt), reward=z((T, E), rdt),
                                 flags=torch.full((T, E), -1, dtype=torch.int32, device="cuda"))


def roll(env, L, first, n, spl=1):
    return env.rollout_episodes_sampled(first, n, L.acted, L.obs, L.act, L.sample, L.logp, L.reward, L.flags, steps_per_launch=spl)


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


def rings_equal(torch, La, Lb):
    for key in RINGS:
        assert torch.equal(getattr(La, key), getattr(Lb, key)), key


def check_rings(L, r, tol):
    """the seven rings against the oracle's run r"""
    T = r["flags"].shape[0]
    np.testing.assert_array_equal(L.flags.cpu().numpy(), r["flags"])
    for key, want, per in (("reward", "reward", None), ("obs", "obs", 20), ("acted", "acted_obs", 20), ("act", "action", 4), ("sample", "sample", 4),
                           ("logp", "logp", 0)):
        got = host(getattr(L, key))
        got = got if per is None else got.reshape(T, -1) if per == 0 else got.reshape(T, -1, per)
        np.testing.assert_allclose(got, r[want], rtol=tol, atol=tol, err_msg=key)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 300])
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_policy_sample_alone(mds, dtype, n):
    """episode_policy_sample on random rows against the oracle, the env's count and length set through the zero-copy pointers to
    non-trivial values.  float64: 1e-12.  float32: RPM within 1e-5 relative, logp within 1e-4, the sample within 2e-4 absolute (the
    project's 1e-5 relative RPM gate expressed before the clamp: 1e-5 x rpm_base / rpm_scale).  Two networks: the second, uploaded
    after the noise was configured, runs the 32-wide kernel -- a policy re-upload keeps the noise."""
    torch = mds.torch
    obs, target = PC.observations(n)
    first_env = 1000
    env = build_env(mds, target.reshape(n, 1, 3), np.zeros((n, 1, 3)), dict(max_steps=5), None, dtype, first_env=first_env)
    rng = np.random.default_rng([21, n])
    count, length = rng.integers(0, 2 ** 31, size=n), rng.integers(0, 5000, size=n)
    c = env.episode_counters()
    c["count"].copy_(torch.as_tensor(count.astype(np.int32), device="cuda"))
    c["length"].copy_(torch.as_tensor(length.astype(np.int32), device="cuda"))
    rows = torch.as_tensor(obs.reshape(n, 1, 20), device="cuda").to(env.dtype).contiguous()
    eps = SO.eps_of(XC.NOISE_SEED, first_env + np.arange(n), count, length, 0)
    for net in (XC.NET, (1, 5, "relu")):
        w = PC.weights(*net[:2])
        env.set_episode_policy(w, *net)
        rpm, sample, logp = (host(t) for t in env.episode_policy_sample(rows))
        _, y = PO.policy_rpm(w, *net, obs, target)
        a, lp = SO.sample(y, eps, XC.LOG_STD)
        want = PO.rpm_of(a)
        if dtype == "float64":
            np.testing.assert_allclose(rpm.reshape(n, 4), want, rtol=1e-12, atol=0)
            np.testing.assert_allclose(sample.reshape(n, 4), a, rtol=1e-12, atol=1e-12)
            np.testing.assert_allclose(logp.reshape(n), lp, rtol=1e-12, atol=1e-12)
        else:
            print(f"n {n} {net}: RPM rel err {np.abs(rpm.reshape(n, 4) / want - 1).max():.2e}, sample err {np.abs(sample.reshape(n, 4) - a).max():.2e}, "
                  f"logp err {np.abs(logp.reshape(n) - lp).max():.2e}")
            np.testing.assert_allclose(rpm.reshape(n, 4), want, rtol=1e-5, atol=0)
            np.testing.assert_allclose(sample.reshape(n, 4), a, rtol=0, atol=2e-4)
            np.testing.assert_allclose(logp.reshape(n), lp, rtol=0, atol=1e-4)
    env.close()


@pytest.mark.parametrize("E,D", XC.SHAPES)
def test_rollout_f64_matches_oracle(mds, E, D):
    """float64, 120 steps: flags and integer counters equal the oracle's at every step; the seven rings, the current observation and the
    float counters within rtol = atol = 1e-9 -- one launch per step, and 8 steps per launch in a call split at step 75."""
    r = XC.oracle_run(E, D)
    T = XC.STEPS
    env = make_env(mds, E, D, "float64")
    L = make_logs(mds, env, T)
    for k in range(T):
        now = host(roll(env, L, k, 1)).reshape(-1, 20)
        np.testing.assert_allclose(now, r["obs_now"][k], rtol=1e-9, atol=1e-9, err_msg=f"current observation after step {k}")
        assert_counters(counters(env), r["counters"][k], 1e-9, f"after step {k}")
    env.close()
    check_rings(L, r, 1e-9)
    env = make_env(mds, E, D, "float64")
    L = make_logs(mds, env, T)
    for k0, k1 in ((0, 75), (75, T)):
        now = host(roll(env, L, k0, k1 - k0, 8)).reshape(-1, 20)
        np.testing.assert_allclose(now, r["obs_now"][k1 - 1], rtol=1e-9, atol=1e-9)
        assert_counters(counters(env), r["counters"][k1 - 1], 1e-9, f"after step {k1 - 1}")
    env.close()
    check_rings(L, r, 1e-9)


@pytest.mark.parametrize("E,D", XC.SHAPES)
def test_rollout_f32_matches_oracle_up_to_the_first_close_call(mds, E, D):
    """float32 against the oracle under the margin rule (an env is compared up to, not including, its first step whose margin is under
    1e-4; the caps of the sibling test first).  Flags equal; state columns within 1e-5 absolute, RPM columns and the action ring
    within 1e-5 relative; reward within 1e-5 D; the sample ring within 2e-4 absolute; the logp ring within 1e-4 absolute."""
    r = XC.oracle_run(E, D)
    T = XC.STEPS
    first, keep = XC.compared_part(r, NEAR)
    assert (first < T).sum() <= 0.10 * E and int(((r["flags"] & 3) != 0)[keep].sum()) >= 20
    env = make_env(mds, E, D, "float32")
    L = make_logs(mds, env, T)
    roll(env, L, 0, 50, 8)
    roll(env, L, 50, T - 50, 8)
    env.close()
    flags, reward = L.flags.cpu().numpy(), host(L.reward)
    obs, acted, act = host(L.obs).reshape(T, E, D, 20), host(L.acted).reshape(T, E, D, 20), host(L.act).reshape(T, E, D, 4)
    sample, logp = host(L.sample).reshape(T, E, D, 4), host(L.logp).reshape(T, E, D)
    want, want_acted, want_act = r["obs"].reshape(T, E, D, 20), r["acted_obs"].reshape(T, E, D, 20), r["action"].reshape(T, E, D, 4)
    want_sample, want_logp = r["sample"].reshape(T, E, D, 4), r["logp"].reshape(T, E, D)
    print(f"{E}x{D}: envs cut short {(first < T).sum()}, flags differing in the compared part {(flags != r['flags'])[keep].sum()}, max state err "
          f"{np.abs(obs - want)[keep][..., :16].max():.2e}, action rel err {np.abs(act / want_act - 1)[keep].max():.2e}, "
          f"reward err {np.abs(reward - r['reward'])[keep].max():.2e}, sample err {np.abs(sample - want_sample)[keep].max():.2e}, "
          f"logp err {np.abs(logp - want_logp)[keep].max():.2e}")
    np.testing.assert_array_equal(flags[keep], r["flags"][keep])
    np.testing.assert_allclose(reward[keep], r["reward"][keep], rtol=0, atol=1e-5 * D)
    np.testing.assert_allclose(obs[keep][..., :16], want[keep][..., :16], rtol=0, atol=1e-5)
    np.testing.assert_allclose(obs[keep][..., 16:], want[keep][..., 16:], rtol=1e-5, atol=0)
    np.testing.assert_allclose(acted[keep][..., :16], want_acted[keep][..., :16], rtol=0, atol=1e-5)
    np.testing.assert_allclose(act[keep], want_act[keep], rtol=1e-5, atol=0)
    np.testing.assert_allclose(sample[keep], want_sample[keep], rtol=0, atol=2e-4)
    np.testing.assert_allclose(logp[keep], want_logp[keep], rtol=0, atol=1e-4)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_acted_ring_is_the_previous_current_observation(mds, dtype):
    """One step per call, randomised starts configured (restarted rows are not the fixed image): acted_obs[j] is bitwise the current
    observation the previous call returned, and for j = 0 bitwise _computeObs().  8 steps per launch write the same bits."""
    torch = mds.torch
    E, D, T = 37, 7, 40
    env = make_env(mds, E, D, dtype)
    env.set_episode_randomisation(RC.SEED, **RC.HALF)
    L = make_logs(mds, env, T)
    prev = env._computeObs().clone()
    image = prev.clone()
    restarted_differ = 0
    for j in range(T):
        now = roll(env, L, j, 1).clone()
        assert torch.equal(L.acted[j], prev), f"step {j}"
        if j:
            done = (L.flags[j - 1] & 3) != 0
            restarted_differ += int((prev[done][..., :3] != image[done][..., :3]).any(dim=-1).sum())
        prev = now
    env.close()
    assert int(((L.flags & 3) != 0).sum()) >= 20 and restarted_differ >= 20 * D
    env = make_env(mds, E, D, dtype)
    env.set_episode_randomisation(RC.SEED, **RC.HALF)
    M = make_logs(mds, env, T)
    roll(env, M, 0, 27, 8)
    roll(env, M, 27, T - 27, 8)
    env.close()
    rings_equal(torch, L, M)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_acted_ring_echo_on_a_handle_that_does_not_track_the_rpm(mds, dtype):
    """Physics.DYN (no drag: nothing but the sampled call keeps the RPM planes, and the no-drag kernels run).  One step per call:
    acted_obs is bitwise the current observation the previous sampled call returned, echo columns included, and for the first call
    bitwise _computeObs().  After rollout_episodes_policy -- which leaves the planes stale: mds_get_obs then reports a NaN echo -- the
    next sampled call's acted rows are bitwise _computeObs() again: the state columns of the observation the policy call returned, a
    NaN echo; and the sampled call after that carries the true echo once more.  8 steps per launch, split, write the same rings."""
    torch = mds.torch
    bits = lambda t: t.contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)   # noqa: E731  (NaN compares by its bits)
    E, D, T = 37, 7, 24
    env = make_env(mds, E, D, dtype, physics=mds.Physics.DYN)
    L = make_logs(mds, env, T)
    prev = env._computeObs().clone()
    assert (prev[..., 16:] == 0).all()
    for j in range(10):
        now = roll(env, L, j, 1).clone()
        assert torch.equal(L.acted[j], prev), f"step {j}"
        assert (now[..., 16:] != 0).any()
        prev = now
    after = env.rollout_episodes_policy(10, 3).clone()
    stale = env._computeObs().clone()
    assert torch.equal(stale[..., :16], after[..., :16]) and torch.isnan(stale[..., 16:]).all() and torch.isfinite(after).all()
    now = roll(env, L, 13, 1).clone()
    assert torch.equal(bits(L.acted[13]), bits(stale))
    assert torch.isfinite(now).all()
    assert torch.equal(env._computeObs(), now)              # the planes are current again
    prev = now
    for j in range(14, T):
        now = roll(env, L, j, 1).clone()
        assert torch.equal(L.acted[j], prev), f"step {j}"
        prev = now
    env.close()
    env = make_env(mds, E, D, dtype, physics=mds.Physics.DYN)
    M = make_logs(mds, env, T)
    roll(env, M, 0, 3, 8)
    roll(env, M, 3, 7, 8)
    env.close()
    for key in RINGS:
        assert torch.equal(getattr(L, key)[:10], getattr(M, key)[:10]), key


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_launch_form_independence(mds, dtype):
    """steps_per_launch 1 and 8, the call split at a step that is no multiple of 8: bit-identical rings, current observation, state and
    counters"""
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
    rings_equal(torch, La, Lb)
    assert torch.equal(na, nb) and torch.equal(na2, nb2)
    np.testing.assert_array_equal(sa, sb)
    assert all(torch.equal(ca[k], cb[k]) for k in ca)
    assert int(((La.flags & 3) != 0).sum()) >= 20


def test_sharding_over_two_handles(mds):
    """(37, 7) split into 20 + 17 envs on two handles with first_env 0 and 20, float64: the concatenated sample, logp and action rings
    are bitwise those of the one handle that holds the whole set"""
    torch = mds.torch
    E, D, T = 37, 7, 60
    xyz, rpy, params, target = PC.scenario(E, D)
    assert XC.FIRST_ENV[(E, D)] == 0
    whole = make_env(mds, E, D, "float64")
    L = make_logs(mds, whole, T)
    roll(whole, L, 0, T, 8)
    whole.close()
    parts = []
    for e0, e1 in ((0, 20), (20, E)):
        env = build_env(mds, xyz[e0:e1], rpy[e0:e1], params, target[e0:e1], "float64", first_env=e0)
        P = make_logs(mds, env, T)
        roll(env, P, 0, T, 8)
        env.close()
        parts.append(P)
    for key in ("sample", "logp", "act", "flags"):
        assert torch.equal(torch.cat([getattr(P, key) for P in parts], dim=1), getattr(L, key)), key
    assert int(((L.flags & 3) != 0).sum()) >= 20


def test_fused_equals_sampling_in_the_loop(mds):
    """rollout_episodes_sampled(T) against T rounds of episode_policy_sample(current observation) + step_episodes, float64, (37, 7),
    60 steps: flags and integer counters equal, rings within 1e-11 (the existing gate between the two launch forms)"""
    torch = mds.torch
    E, D, T = 37, 7, 60
    a = make_env(mds, E, D, "float64")
    L = make_logs(mds, a, T)
    now_a = host(roll(a, L, 0, T, 8))
    b = make_env(mds, E, D, "float64")
    obs = b._computeObs()
    got = {k: [] for k in RINGS}
    final = torch.zeros((E, D, 20), dtype=b.dtype, device="cuda")
    for k in range(T):
        got["acted"].append(host(obs))
        rpm, sample, logp = b.episode_policy_sample(obs)
        obs, rew, _, _, info = b.step_episodes(rpm, final_obs=final)
        for key, v in (("flags", info["flags"].cpu().numpy().copy()), ("reward", host(rew)), ("act", host(rpm)), ("sample", host(sample)),
                       ("logp", host(logp)), ("obs", host(final))):
            got[key].append(v)
    np.testing.assert_array_equal(np.stack(got["flags"]), L.flags.cpu().numpy())
    for key in RINGS[:-1]:
        np.testing.assert_allclose(np.stack(got[key]), host(getattr(L, key)), rtol=1e-11, atol=1e-11, err_msg=key)
    np.testing.assert_allclose(host(obs), now_a, rtol=1e-11, atol=1e-11)
    assert_counters(counters(b), counters(a), 1e-11)
    assert int(((L.flags & 3) != 0).sum()) >= 20
    a.close()
    b.close()


def test_what_a_learner_recomputes(mds):
    """float64: a torch float64 nn.Sequential of the same weights applied to the features of the acted_obs ring gives the mean;
    Normal(mean, sigma).log_prob(sample ring).sum(-1) equals the logp ring within 1e-9, and the RPM of clip(sample) equals the action
    ring within 1e-9"""
    torch = mds.torch
    from tests.test_episode_policy_cpu import torch_net
    E, D, T = 37, 7, 60
    _, _, _, target = PC.scenario(E, D)
    env = make_env(mds, E, D, "float64")
    L = make_logs(mds, env, T)
    roll(env, L, 0, T, 8)
    env.close()
    net = torch_net(PC.weights(*XC.NET[:2]), *XC.NET)
    acted = L.acted.cpu().reshape(T, E * D, 20)
    tgt = torch.as_tensor(target.reshape(1, E * D, 3))
    x = torch.cat([acted[..., 0:3] - tgt, acted[..., 7:10], acted[..., 10:13], acted[..., 13:16]], dim=-1)
    with torch.no_grad():
        mean = net(x)
    sample = L.sample.cpu().reshape(T, E * D, 4)
    logp = torch.distributions.Normal(mean, torch.as_tensor(SIGMA)).log_prob(sample).sum(-1)
    np.testing.assert_allclose(host(L.logp).reshape(T, -1), logp.numpy(), rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(host(L.act).reshape(T, -1, 4), PO.rpm_of(sample.clamp(-1.0, 1.0).numpy()), rtol=1e-9, atol=1e-9)
    assert 0.01 < float((sample.abs() > 1).double().mean()) < 0.25


def test_small_sigma_is_the_deterministic_rollout(mds):
    """log_std = -40 on all four, float64: the action, obs, reward and flags rings agree with rollout_episodes_policy's on a twin handle
    within 1e-9 (flags equal), and logp equals -0.5 sum(eps^2) + 160 - 2 ln(2 pi) from the oracle's eps"""
    E, D, T = 37, 7, 60
    log_std = (-40.0,) * 4
    r = XC.oracle_run(E, D, False, T, log_std)
    env = make_env(mds, E, D, "float64", log_std=log_std)
    L = make_logs(mds, env, T)
    roll(env, L, 0, T, 8)
    env.close()
    twin = make_env(mds, E, D, "float64", noise=False)
    M = make_logs(mds, twin, T)
    twin.rollout_episodes_policy(0, T, M.obs, M.act, M.reward, M.flags, steps_per_launch=8)
    twin.close()
    assert (L.flags == M.flags).all() and int(((L.flags & 3) != 0).sum()) >= 20
    for key in ("act", "obs", "reward"):
        np.testing.assert_allclose(host(getattr(L, key)), host(getattr(M, key)), rtol=1e-9, atol=1e-9, err_msg=key)
    want = -0.5 * (r["eps"] ** 2).sum(-1) + 160.0 - 2.0 * np.log(2.0 * np.pi)
    np.testing.assert_allclose(host(L.logp).reshape(T, -1), want, rtol=1e-9, atol=1e-9)


def test_epoch_moves_with_a_reset_of_all_envs(mds):
    """Two identical calls separated by mds_reset_async (the counters put back to zero as well, so that count and length repeat) give
    different sample rings: epoch moved, and the first step's difference is sigma (eps(epoch 1) - eps(epoch 0)).  Two fresh handles with
    the same configuration give identical rings."""
    torch = mds.torch
    lib = capi.load_library()
    E, D, T = 37, 7, 20
    env = make_env(mds, E, D, "float64")
    A, B = make_logs(mds, env, T), make_logs(mds, env, T)
    roll(env, A, 0, T, 8)
    capi.check(lib.mds_reset_async(env._h, env._stream()), "mds_reset_async")
    for v in env.episode_counters().values():
        v.zero_()
    roll(env, B, 0, T, 8)
    env.close()
    assert torch.equal(A.acted[0], B.acted[0])
    assert (A.sample[0] != B.sample[0]).all()
    g, zero = XC.FIRST_ENV[(E, D)] * D + np.arange(E * D), np.zeros(E * D, dtype=np.int64)
    d_eps = SO.eps_of(XC.NOISE_SEED, g, zero, zero, 1) - SO.eps_of(XC.NOISE_SEED, g, zero, zero, 0)
    np.testing.assert_allclose(host(B.sample[0] - A.sample[0]).reshape(-1, 4), SIGMA[None, :] * d_eps, rtol=1e-9, atol=1e-9)
    fresh = make_env(mds, E, D, "float64")
    F = make_logs(mds, fresh, T)
    roll(fresh, F, 0, T, 8)
    fresh.close()
    rings_equal(torch, A, F)


def make_safety_env(mds, dtype, policy=True, params=None):
    E, D = XC.SAFETY_SHAPE
    xyz, rpy, _, p, obstacles = SC.scenario(E, D)
    env = build_env(mds, xyz, rpy, p if params is None else params, None, dtype, policy=policy)
    env.set_episode_safety(SC.SAFETY_RADIUS, SC.ZSCALE, obstacles)
    env.set_episode_randomisation(RC.SEED, **RC.HALF)
    return env


def test_with_safety_and_randomised_starts(mds):
    """(37, 7), float64, collision causes and randomised starts configured, against the composed oracle: flags equal with bit 14 firing
    at least 5 times, rings within 1e-9, and the start states of restarted drones are bitwise those of a table-driven handle with the
    same (seed, g, ordinal, generation): the noise does not disturb the start draws."""
    E, D = XC.SAFETY_SHAPE
    T = XC.STEPS
    r = XC.safety_oracle_run()
    env = make_safety_env(mds, "float64")
    first = host(env.reset_episodes()).reshape(-1, 20)
    np.testing.assert_allclose(first, r["first_rows"], rtol=1e-9, atol=1e-9)
    L = make_logs(mds, env, T)
    restarted = []
    for k in range(T):
        roll(env, L, k, 1)
        assert_counters(counters(env), r["counters"][k], 1e-9, f"after step {k}")
        done = (L.flags[k].cpu().numpy() & 3) != 0
        if done.any():
            st, cnt = env.get_state(), counters(env)["count"]
            restarted += [(e, int(cnt[e]), st[e].copy()) for e in np.flatnonzero(done)]
    s = env.episode_safety()
    np.testing.assert_allclose(host(s["h_min_episode"]), r["h_min_episode"][T - 1], rtol=1e-9, atol=1e-9)
    env.close()
    check_rings(L, r, 1e-9)
    assert int(((L.flags.cpu().numpy() >> 14) & 1).sum()) >= 5
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
def test_other_rollouts_are_unchanged_by_configured_noise(mds, dtype):
    """on a handle with noise configured, rollout_episodes_policy and rollout_episodes (table) give the bits of a handle without it"""
    torch = mds.torch
    E, D, T = 37, 7, 60
    _, _, actions, _ = EC.scenario(E, D, "combined")
    out = []
    for noise in (True, False):
        res = []
        for table in (False, True):
            env = make_env(mds, E, D, dtype, noise=noise)
            L = make_logs(mds, env, T)
            if table:
                acts = torch.as_tensor(actions.reshape(EC.N_SETS, E, D, 4), device="cuda").to(env.dtype).contiguous()
                now = env.rollout_episodes(acts, 0, T, L.obs, L.reward, L.flags, steps_per_launch=8).clone()
            else:
                now = env.rollout_episodes_policy(0, T, L.obs, L.act, L.reward, L.flags, steps_per_launch=8).clone()
            res.append((L, now, env.get_state(), {k: v.clone() for k, v in env.episode_counters().items()}))
            env.close()
        out.append(res)
    for (La, na, sa, ca), (Lb, nb, sb, cb) in zip(*out):
        rings_equal(torch, La, Lb)
        assert torch.equal(na, nb)
        np.testing.assert_array_equal(sa, sb)
        assert all(torch.equal(ca[k], cb[k]) for k in ca)
        assert int(((La.flags & 3) != 0).sum()) >= 20


def test_switching_off_and_refusals(mds):
    """MDS_ESTATE before a policy or noise is set and after set_episodes(enabled=False) or switching the policy off; MDS_EINVAL for each
    bad field with the handle keeping its noise; MDS_EALIGN for a misaligned ring; a policy re-upload and a re-configuration of rule,
    safety or randomisation keep the noise; fp16-storage and MDS_F32C handles stay usable after the refusal."""
    torch = mds.torch
    lib = capi.load_library()
    E, D = 4, 2
    xyz, rpy = np.zeros((E, D, 3)), np.zeros((E, D, 3))
    xyz[..., 2] = 1.0
    xyz[..., 0] = np.arange(D)[None, :]
    net = XC.NET
    w = PC.weights(*net[:2])

    def noise(log_std=XC.LOG_STD, first_env=0):
        return capi.MdsEpisodePolicyNoise(7, first_env, (C.c_double * 4)(*log_std))

    def call(env, rings=None):
        return lib.mds_rollout_episodes_sampled(env._h, 0, 1, rings, 2 if rings is not None else 0, 1, None, None)

    def sample(env):
        p = C.c_void_p(env._obs.data_ptr())
        return lib.mds_episode_policy_sample(env._h, p, p, None, None, None)

    env = build_env(mds, xyz, rpy, dict(max_steps=5), None, "float32", policy=False)
    p = noise()
    assert lib.mds_set_episode_policy_noise(env._h, C.byref(p), None) == -5     # no policy yet
    assert call(env) == -5 and sample(env) == -5
    env.set_episode_policy(w, *net)
    assert call(env) == -5 and sample(env) == -5                                # a policy, no noise
    assert lib.mds_rollout_episodes_policy(env._h, 0, 1, None, 0, None, None, None, 1, None, None) == 0
    env.set_episode_policy_noise(XC.LOG_STD, 7)
    assert call(env) == 0 and sample(env) == 0
    # failed calls: the handle keeps its noise
    for bad in (noise((np.nan, 0, 0, 0)), noise((0, np.inf, 0, 0)), noise((0, 0, -np.inf, 0)), noise((0, 0, 0, 200.0)), noise((-200.0, 0, 0, 0)),
                noise(first_env=-1), noise(first_env=2 ** 32 // D)):
        assert lib.mds_set_episode_policy_noise(env._h, C.byref(bad), None) == -1
        assert b"mds_set_episode_policy_noise" in lib.mds_last_error()
    assert call(env) == 0
    # a misaligned ring, and bad arguments
    log = torch.zeros((2 * E * D * 4 + 4,), device="cuda")
    for field in ("sample", "logp", "acted_obs"):
        rings = capi.MdsEpisodeSampleRings()
        setattr(rings, field, log.data_ptr() + 4)
        assert call(env, C.byref(rings)) == -4, field
    rings = capi.MdsEpisodeSampleRings()
    rings.sample = log.data_ptr()
    assert call(env, C.byref(rings)) == 0
    assert lib.mds_rollout_episodes_sampled(env._h, 0, 1, C.byref(rings), 0, 1, None, None) == -1
    assert lib.mds_rollout_episodes_sampled(env._h, 0, 1, C.byref(rings), 2, 0, None, None) == -1
    # a policy re-upload and reconfigurations keep it
    env.set_episode_policy(w * 0.5, *net)
    env.set_episodes(max_steps=7)
    env.set_episode_safety(0.05)
    env.set_episode_randomisation(3, pos=0.01)
    assert call(env) == 0 and sample(env) == 0
    # switching off
    env.set_episode_policy_noise(None, enabled=False)
    assert call(env) == -5 and sample(env) == -5
    env.set_episode_policy_noise(XC.LOG_STD, 7)
    env.set_episode_policy(None, 0, 0, enabled=False)
    assert call(env) == -5
    env.set_episode_policy(w, *net)
    assert call(env) == -5                                                      # ... and stays off until configured again
    env.set_episode_policy_noise(XC.LOG_STD, 7)
    assert call(env) == 0
    env.set_episodes(enabled=False)
    assert call(env) == -5 and sample(env) == -5
    with pytest.raises(capi.MdsError):
        env.rollout_episodes_sampled(0, 1)
    env.set_episodes(max_steps=5)
    assert call(env) == -5
    env.close()
    kw = dict(drone_model=mds.DroneModel.CF2P, num_drones=D, initial_xyzs=xyz, initial_rpys=rpy, num_envs=E, physics=mds.Physics.DYN)
    for dtype in ("float16", "float32c"):
        env = mds.CtrlAviary(dtype=dtype, **kw)
        if dtype == "float16":
            env.set_episodes(max_steps=5)
        assert lib.mds_set_episode_policy_noise(env._h, C.byref(p), None) == -5, dtype      # they have no policy: it was refused
        assert call(env) == -5
        with pytest.raises(capi.MdsError):
            env.set_episode_policy_noise(XC.LOG_STD)
        obs, *_ = env.step(torch.full((E, D, 4), 14000.0, dtype=env.dtype, device="cuda"))
        assert torch.isfinite(obs.float()).all()
        env.close()

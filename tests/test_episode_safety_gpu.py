"""Collision causes of the per-env episodes on the device (mds_set_episode_safety / mds_episode_safety_ptrs) against the float64 oracle of
tests/episode_safety_oracle.py, on the shapes that cross every boundary of the kernel's thread mapping (tests/episode_safety_cases.py)."""
import ctypes as C

import numpy as np
import pytest

from multidronesim_amd import _capi as capi
from tests import episode_cases as EC
from tests import episode_oracle as EO
from tests import episode_safety_cases as SC
from tests import episode_safety_oracle as SO

pytestmark = pytest.mark.gpu
NEAR = 1e-4
SHAPES = list(SC.SHAPES)
UNSET = object()


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


def make_env(mds, E, D, dtype, safety=True, params=None, safety_radius=SC.SAFETY_RADIUS, obstacles=UNSET, xyz=None):
    xyz0, rpy, actions, p, ob = SC.scenario(E, D)
    xyz = xyz0 if xyz is None else xyz
    p = dict(p if params is None else params)
    ob = ob if obstacles is UNSET else obstacles
    env = mds.CtrlAviary(drone_model=mds.DroneModel.CF2P, num_drones=D, initial_xyzs=xyz, initial_rpys=rpy, physics=mds.Physics.PYB_DRAG,
                         pyb_freq=EC.PYB_FREQ, ctrl_freq=EC.CTRL_FREQ, num_envs=E, dtype=dtype)
    env.set_episodes(**p)
    if safety:
        env.set_episode_safety(safety_radius, SC.ZSCALE, ob)
    acts = mds.torch.as_tensor(actions.reshape(EC.N_SETS, E, D, 4), device="cuda").to(env.dtype).contiguous()
    return env, acts


def make_logs(mds, env, T):
    torch, E, D = mds.torch, env.NUM_ENVS, env.NUM_DRONES
    rdt = torch.float64 if env.dtype == torch.float64 else torch.float32
    return (torch.zeros((T, E, D, 20), dtype=env.dtype, device="cuda"), torch.zeros((T, E), dtype=rdt, device="cuda"),
            torch.full((T, E), -1, dtype=torch.int32, device="cuda"))


def host(t):
    return t.detach().double().cpu().numpy()


def counters(env):
    return {k: v.cpu().numpy().astype(np.float64 if v.is_floating_point() else np.int64) for k, v in env.episode_counters().items()}


def safety(env):
    return {k: host(v) for k, v in env.episode_safety().items()}


@pytest.mark.parametrize("E,D", SHAPES)
def test_f64_matches_oracle(mds, E, D):
    """float64, 120 steps: flags (bits 14 and 15 included) and counters equal the oracle's at every step; reward, the logged rows, the current
    observation, h_min_step and h_min_episode within rtol = atol = 1e-9 -- one launch per step, and 8 steps per launch in a call split at
    step 75."""
    r = SC.oracle_run(E, D)
    T = SC.STEPS
    env, acts = make_env(mds, E, D, "float64")
    obs_log, reward_log, flags_log = make_logs(mds, env, T)
    for k in range(T):
        now = host(env.rollout_episodes(acts, k, 1, obs_log, reward_log, flags_log)).reshape(-1, 20)
        np.testing.assert_allclose(now, r["obs_now"][k], rtol=1e-9, atol=1e-9, err_msg=f"obs_now after step {k}")
        hs = safety(env)
        np.testing.assert_allclose(hs["h_min_step"], r["h_min_step"][k], rtol=1e-9, atol=1e-9, err_msg=f"h_min_step after step {k}")
        np.testing.assert_allclose(hs["h_min_episode"], r["h_min_episode"][k], rtol=1e-9, atol=1e-9, err_msg=f"h_min_episode after step {k}")
        cnt = counters(env)
        for key, want in r["counters"][k].items():
            if want.dtype.kind == "i":
                np.testing.assert_array_equal(cnt[key], want, err_msg=f"{key} after step {k}")
            else:
                np.testing.assert_allclose(cnt[key], want, rtol=1e-9, atol=1e-9, err_msg=f"{key} after step {k}")
    env.close()
    flags = flags_log.cpu().numpy().astype(np.int64)
    print(f"{E}x{D} float64: pair events {((flags >> 14) & 1).sum()}, obstacle events {((flags >> 15) & 1).sum()}")
    np.testing.assert_array_equal(flags, r["flags"])
    np.testing.assert_allclose(host(reward_log), r["reward"], rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(host(obs_log).reshape(T, -1, 20), r["obs"], rtol=1e-9, atol=1e-9)
    # 8 steps per launch, the call split at a step that is no multiple of 8
    env, acts = make_env(mds, E, D, "float64")
    obs_log, reward_log, flags_log = make_logs(mds, env, T)
    for k0, k1 in ((0, 75), (75, T)):
        now8 = host(env.rollout_episodes(acts, k0, k1 - k0, obs_log, reward_log, flags_log, steps_per_launch=8)).reshape(-1, 20)
        np.testing.assert_allclose(now8, r["obs_now"][k1 - 1], rtol=1e-9, atol=1e-9)
        hs = safety(env)
        np.testing.assert_allclose(hs["h_min_step"], r["h_min_step"][k1 - 1], rtol=1e-9, atol=1e-9)
        np.testing.assert_allclose(hs["h_min_episode"], r["h_min_episode"][k1 - 1], rtol=1e-9, atol=1e-9)
        c8 = counters(env)
        for key, want in r["counters"][k1 - 1].items():
            np.testing.assert_allclose(c8[key], want, rtol=1e-9, atol=1e-9, err_msg=f"{key} after step {k1 - 1}")
    env.close()
    np.testing.assert_array_equal(flags_log.cpu().numpy(), r["flags"])
    np.testing.assert_allclose(host(reward_log), r["reward"], rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(host(obs_log).reshape(T, -1, 20), r["obs"], rtol=1e-9, atol=1e-9)


def h_min_bounds(pos, D, obstacles, delta):
    """[lo, hi] per env for the smallest h of positions within `delta` (per coordinate) of `pos` [n,3], evaluated in float32.

    A separation component then errs by at most a = 2 delta (two drones) or delta + 2^-24 |c| (a drone and a centre rounded to float32).
    h's partial derivatives are 4 s ex, 4 s ey and 4 ez^3 / zscale^4, each growing with the components' sizes, so over the box
    |dh| <= a (4 s+ (|ex|+ + |ey|+) + 4 |ez|+^3 / zscale^4) =: tol, with x+ = |x| + a and s+ = ex+^2 + ey+^2 (mean value theorem), plus the
    float32 evaluation: 4 ulp of the largest term.  With i* the oracle's minimiser: min_i (h_i - tol_i) <= the device's minimum <= h_i* + tol_i*."""
    n = pos.shape[0]
    E = n // D
    zs4, eps = SC.ZSCALE ** 4, 2.0 ** -23

    def box(e, a, Ds):
        h, _ = SO.barrier(e, SC.ZSCALE, Ds)
        ap = np.abs(e) + a
        sp = ap[..., 0] ** 2 + ap[..., 1] ** 2
        tol = a * (4 * sp * (ap[..., 0] + ap[..., 1]) + 4 * ap[..., 2] ** 3 / zs4) + 4 * eps * np.maximum(sp * sp + ap[..., 2] ** 4 / zs4, Ds ** 4)
        return h, tol
    hs, tols = [], []
    if D > 1:
        p = pos.reshape(E, D, 3)
        h, tol = box(p[:, :, None, :] - p[:, None, :, :], 2 * delta, 2.0 * SC.SAFETY_RADIUS)
        other = ~np.eye(D, dtype=bool)[None]
        hs.append(np.where(other, h, np.inf).reshape(E, D * D))
        tols.append(np.where(other, tol, 0.0).reshape(E, D * D))
    if obstacles is not None:
        a = delta + 2.0 ** -24 * np.abs(obstacles[:, :3]).max()
        h, tol = box(pos[:, None, :] - obstacles[None, :, :3], a, SC.SAFETY_RADIUS + obstacles[None, :, 3])
        hs.append(h.reshape(E, -1))
        tols.append(tol.reshape(E, -1))
    h, tol = np.concatenate(hs, axis=1), np.concatenate(tols, axis=1)
    star = h.argmin(axis=1)
    rows = np.arange(E)
    return (h - tol).min(axis=1), h[rows, star] + tol[rows, star]


@pytest.mark.parametrize("E,D", SHAPES)
def test_f32_matches_oracle_up_to_the_first_close_call(mds, E, D):
    """float32 against the oracle under the first-close-call rule (margin 1e-4, at most 10 % of the envs cut short, at least 20 done-events
    compared): flags equal and rows within smoke()'s gates in the compared part, 8 steps per launch; then one step per launch, h_min_step
    of every compared env-step inside the interval h_min_bounds derives from the 1e-5 position gate."""
    r = SC.oracle_run(E, D)
    T = SC.STEPS
    first, keep = SC.compared_part(r, NEAR)
    assert (first < T).sum() <= 0.10 * E
    assert int(((r["flags"] & 3) != 0)[keep].sum()) >= 20
    env, acts = make_env(mds, E, D, "float32")
    obs_log, reward_log, flags_log = make_logs(mds, env, T)
    env.rollout_episodes(acts, 0, 50, obs_log, reward_log, flags_log, steps_per_launch=8)
    env.rollout_episodes(acts, 50, T - 50, obs_log, reward_log, flags_log, steps_per_launch=8)
    env.close()
    flags, reward, obs = flags_log.cpu().numpy(), host(reward_log), host(obs_log).reshape(T, E, D, 20)
    want = r["obs"].reshape(T, E, D, 20)
    print(f"{E}x{D}: envs cut short {(first < T).sum()}, flags differing in the compared part {(flags != r['flags'])[keep].sum()}, "
          f"max reward err {np.abs(reward - r['reward'])[keep].max():.2e}, max position err {np.abs(obs - want)[keep][..., :3].max():.2e}")
    np.testing.assert_array_equal(flags[keep], r["flags"][keep])
    np.testing.assert_allclose(reward[keep], r["reward"][keep], rtol=0, atol=1e-5 * D)
    np.testing.assert_allclose(obs[keep][..., :16], want[keep][..., :16], rtol=0, atol=1e-5)
    np.testing.assert_allclose(obs[keep][..., 16:], want[keep][..., 16:], rtol=1e-5, atol=0)
    # one step per launch: h_min_step of every step
    _, _, _, _, obstacles = SC.scenario(E, D)
    env, acts = make_env(mds, E, D, "float32")
    _, _, flags_log = make_logs(mds, env, T)
    got = []
    for k in range(T):
        env.rollout_episodes(acts, k, 1, None, None, flags_log)
        got.append(safety(env)["h_min_step"])
    got = np.stack(got)
    env.close()
    np.testing.assert_array_equal(flags_log.cpu().numpy()[keep], r["flags"][keep])
    lo, hi = zip(*(h_min_bounds(r["state"][k][:, :3], D, obstacles, 1e-5) for k in range(T)))
    lo, hi = np.stack(lo), np.stack(hi)
    width = (hi - lo)[keep]
    print(f"{E}x{D}: h_min_step intervals in the compared part: median width {np.median(width):.2e}, max {width.max():.2e}; "
          f"worst position in its interval {np.max(np.abs(got - 0.5 * (lo + hi))[keep] / (0.5 * (hi - lo))[keep]):.3f} of the half width")
    assert (got[keep] >= lo[keep]).all() and (got[keep] <= hi[keep]).all()


def recompute(params, obs, E, D, flags_gpu, safety_radius, obstacles):
    """flags recomputed in float64 from logged rows [T, n, 20], with the episode lengths the GPU's own flags imply; and the margin [T, E]"""
    T = obs.shape[0]
    length = np.zeros(E, dtype=np.int64)
    flags, margin = np.zeros((T, E), dtype=np.int64), np.zeros((T, E))
    for k in range(T):
        cause, m = EO.causes_from_obs(params, obs[k], obs[k][:, 0:3])
        c2, _, m2 = SO.safety_causes(obs[k][:, 0:3], D, safety_radius, SC.ZSCALE, obstacles)
        length += 1
        flags[k] = EO.env_flags(params, np.bitwise_or.reduce((cause | c2).reshape(E, D), axis=1), length)
        margin[k] = np.fmin(m, m2).reshape(E, D).min(axis=1)
        length[(flags_gpu[k] & 3) != 0] = 0
    return flags, margin


def test_fp16_storage_self_consistency(mds):
    """fp16 storage, 38 x 7, the form of test_episode_gpu.test_self_consistency with the safety set on: the flags recomputed in float64 from
    the GPU's own logged rows match wherever the recomputed margin exceeds the band, at least half of the done-events lying outside it.
    The band is 2e-2: a logged fp16 coordinate in [1, 2) is rounded by up to 2^-11 = 4.9e-4, a separation component by twice that, and with
    L = (s^2 + (ez / 2)^4)^(1/4), dL/dex = 0.60 and dL/dez = 0.30 at the homes' separation (0.05, 0, 0.1), so L moves by up to 8.7e-4 =
    1.6e-2 of Ds.  A drone crosses the threshold by drifting, so a pair event itself lies inside any band wider than one step's drift;
    safety_radius 0.0275 and max_steps 12 (probed on the float64 oracle: 380 done-events, 12 of them pair events, 74 % outside the band)
    leave the exact truncations to carry the share outside it, as the existing test's max_steps = 15 does."""
    E, D = SC.FP16_SHAPE
    T, band, radius = SC.STEPS, 2e-2, 0.0275
    params = dict(max_steps=12)
    env, acts = make_env(mds, E, D, "float16", params=params, safety_radius=radius, obstacles=None)
    obs_log, reward_log, flags_log = make_logs(mds, env, T)
    env.rollout_episodes(acts, 0, 33, obs_log, reward_log, flags_log, steps_per_launch=8)
    env.rollout_episodes(acts, 33, T - 33, obs_log, reward_log, flags_log, steps_per_launch=8)
    cnt, hs = counters(env), safety(env)
    env.close()
    flags, obs = flags_log.cpu().numpy().astype(np.int64), host(obs_log).reshape(T, E * D, 20)
    want, margin = recompute(params, obs, E, D, flags, radius, None)
    clear, done, pair = margin > band, (flags & 3) != 0, ((flags >> 14) & 1) != 0
    print(f"{E}x{D} float16: done-events {done.sum()}, pair events {pair.sum()}, outside the band {(done & clear).sum()}, "
          f"flags differing outside it {(flags != want)[clear].sum()}")
    assert (done & clear).sum() >= 0.5 * done.sum() and done.sum() >= 20 and pair.sum() >= 1
    np.testing.assert_array_equal(flags[clear], want[clear])
    assert (flags & ~(3 | (1 << 14))).max() == 0 and (pair == ((flags & 1) != 0)).all()
    np.testing.assert_array_equal(cnt["count"], done.sum(axis=0))
    assert np.isinf(hs["h_min_episode"][done[-1]]).all() and (hs["h_min_step"][pair[-1]] < 0).all() and (hs["h_min_step"][~pair[-1]] >= 0).all()


def run_logs(mds, env, acts, T):
    obs_log, reward_log, flags_log = make_logs(mds, env, T)
    env.rollout_episodes(acts, 0, T, obs_log, reward_log, flags_log, steps_per_launch=8)
    return obs_log, reward_log, flags_log


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_switched_off_is_the_handle_that_never_had_it(mds, dtype):
    """Safety configured and then switched off: logs, counters and state bit-identical to a handle that never had it.  A handle with it on
    differs (its envs end on the pair bit)."""
    torch = mds.torch
    E, D, T = 37, 7, 60
    never, acts = make_env(mds, E, D, dtype, safety=False)
    off, _ = make_env(mds, E, D, dtype)
    off.set_episode_safety(enabled=False)
    on, _ = make_env(mds, E, D, dtype)
    logs = {name: run_logs(mds, env, acts, T) for name, env in (("never", never), ("off", off), ("on", on))}
    assert all(torch.equal(a, b) for a, b in zip(logs["never"], logs["off"]))
    ca, cb = never.episode_counters(), off.episode_counters()
    assert all(torch.equal(ca[k], cb[k]) for k in ca)
    np.testing.assert_array_equal(never.get_state(), off.get_state())
    assert ((logs["never"][2] >> 14) == 0).all()
    assert not torch.equal(logs["never"][2], logs["on"][2]) and int(((logs["on"][2] >> 14) & 1).sum()) >= 20
    # set_episodes(enabled=False) switches safety off with the episodes: configured again, the handle runs without it
    on.set_episodes(enabled=False)
    on.reset()
    on.set_episodes(**SC.PARAMS)
    again = run_logs(mds, on, acts, T)
    assert all(torch.equal(a, b) for a, b in zip(logs["never"], again))
    for env in (never, off, on):
        env.close()


@pytest.mark.parametrize("dtype", ["float32", "float16", "float64"])
def test_a_set_nobody_enters_changes_no_bit(mds, dtype):
    """The safety kernel is a sibling of the plain episode kernel with the same loop.  With a safety radius of 1 mm (nobody gets that close)
    and the combined rule of tests/episode_cases.py ending episodes on every other cause, its logs, counters and state are the plain
    kernel's bit for bit: the two loops have not drifted apart."""
    torch = mds.torch
    E, D, T = (38 if dtype == "float16" else 37), 7, 60
    plain, acts = make_env(mds, E, D, dtype, safety=False, params=EC.COMBINED)
    safe, _ = make_env(mds, E, D, dtype, params=EC.COMBINED, safety_radius=1e-3, obstacles=None)
    a, b = run_logs(mds, plain, acts, T), run_logs(mds, safe, acts, T)
    assert int(((a[2] & 3) != 0).sum()) >= 20 and int((a[2] >> 8 != 0).sum()) >= 20
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    ca, cb = plain.episode_counters(), safe.episode_counters()
    assert all(torch.equal(ca[k], cb[k]) for k in ca)
    np.testing.assert_array_equal(plain.get_state(), safe.get_state())
    assert torch.isfinite(safe.episode_safety()["h_min_step"]).all() and (safe.episode_safety()["h_min_step"] > 0).all()
    plain.close()
    safe.close()


def test_a_reconfigured_rule_keeps_the_safety_settings_and_resets_restart_the_minimum(mds):
    """mds_set_episodes again on a configured handle keeps the safety set; h_min_episode is +inf straight after mds_reset_async, after
    mds_reset and after the re-configuration, and finite again after the next step."""
    torch = mds.torch
    E, D = 37, 7
    env, acts = make_env(mds, E, D, "float32")
    lib = capi.load_library()

    def fly(k0, n):
        _, _, flags_log = make_logs(mds, env, n)
        env.rollout_episodes(acts, k0, n, None, None, flags_log, steps_per_launch=8)
        return flags_log
    fly(0, 5)
    assert torch.isfinite(env.episode_safety()["h_min_episode"]).all() and torch.isfinite(env.episode_safety()["h_min_step"]).all()
    assert lib.mds_reset_async(env._h, env._stream()) == 0
    assert torch.isinf(env.episode_safety()["h_min_episode"]).all()
    fly(0, 5)
    assert torch.isfinite(env.episode_safety()["h_min_episode"]).all()
    env.reset()
    assert torch.isinf(env.episode_safety()["h_min_episode"]).all()
    fly(0, 5)
    env.set_episodes(max_steps=25)
    assert torch.isinf(env.episode_safety()["h_min_episode"]).all()
    env.reset()
    flags = fly(0, 60).cpu().numpy()
    assert int(((flags >> 14) & 1).sum()) >= 20                      # the pair test still runs under the new rule
    env.close()


def test_drones_of_different_envs_never_meet(mds):
    """Two envs of two drones flown on top of each other -- every drone of env 1 starts 1 cm from its counterpart of env 0, far inside Ds --
    while the drones within an env are 0.5 m apart: no bit fires and h_min_step is the env-mates' h."""
    E, D = 2, 2
    xyz = np.zeros((E, D, 3))
    xyz[:, 1, 0] = 0.5
    xyz[1, :, 1] = 0.01
    xyz[..., 2] = 1.0
    for dtype in ("float32", "float64"):
        env = mds.CtrlAviary(drone_model=mds.DroneModel.CF2P, num_drones=D, initial_xyzs=xyz, initial_rpys=np.zeros((E, D, 3)),
                             physics=mds.Physics.PYB_DRAG, pyb_freq=EC.PYB_FREQ, ctrl_freq=EC.CTRL_FREQ, num_envs=E, dtype=dtype)
        env.set_episodes(max_steps=40)
        env.set_episode_safety(SC.SAFETY_RADIUS, SC.ZSCALE)
        acts = mds.torch.full((1, E, D, 4), float(env.HOVER_RPM), dtype=env.dtype, device="cuda")
        flags_log = mds.torch.full((10, E), -1, dtype=mds.torch.int32, device="cuda")
        env.rollout_episodes(acts, 0, 10, None, None, flags_log, steps_per_launch=4)
        hs = safety(env)
        env.close()
        assert (flags_log.cpu().numpy() == 0).all()
        np.testing.assert_allclose(hs["h_min_step"], 0.5 ** 4 - (2 * SC.SAFETY_RADIUS) ** 4, rtol=1e-4)
        np.testing.assert_allclose(hs["h_min_episode"], hs["h_min_step"], rtol=1e-4)


def test_fp32_pair_decisions_do_not_depend_on_a_common_origin_offset(mds):
    """Every origin moved by (512, -256, 64) m (mds_set_origin through ctypes, then reset() so that the start is stored relative to it), the
    starts on a 2^-20 m grid so that the move is exact in float32 and float64: flags, h_min_step and the local state are the bits of the
    flight at the world origin.  Formed from world coordinates the separations of 0.05 m would carry the 3e-5 m ulp of |x| = 512 m."""
    torch = mds.torch
    E, D, T = 37, 7, 60
    xyz0, _, _, _, _ = SC.scenario(E, D)
    xyz0 = np.round(xyz0 * 2.0 ** 20) / 2.0 ** 20
    shift = np.array([512.0, -256.0, 64.0])
    out = {}
    for name, off in (("near", np.zeros(3)), ("far", shift)):
        env, acts = make_env(mds, E, D, "float32", xyz=xyz0 + off, params=dict(max_steps=40))
        org = np.ascontiguousarray(np.broadcast_to(off, (E * D, 3)))
        assert env._lib.mds_set_origin(env._h, org.ctypes.data_as(C.POINTER(C.c_double)), env._stream()) == 0
        env.reset()
        _, _, flags_log = make_logs(mds, env, T)
        env.rollout_episodes(acts, 0, T, None, None, flags_log, steps_per_launch=8)
        local = [host(p) for p in env.state_views()["comp"]]
        out[name] = (flags_log.cpu().numpy(), {k: v.clone() for k, v in env.episode_safety().items()}, np.stack(local))
        env.close()
    assert int(((out["near"][0] >> 14) & 1).sum()) >= 20
    np.testing.assert_array_equal(out["near"][0], out["far"][0])
    assert all(torch.equal(out["near"][1][k], out["far"][1][k]) for k in out["near"][1])
    np.testing.assert_array_equal(out["near"][2], out["far"][2])


def test_error_codes(mds):
    """MDS_ESTATE without mds_set_episodes and for the pointers before the first configuration; MDS_EINVAL for every bad argument, the
    handle keeping the set it had; NULL switches off without an error."""
    lib = capi.load_library()
    xyz, rpy = np.zeros((4, 2, 3)), np.zeros((4, 2, 3))
    xyz[..., 2] = 1.0
    xyz[:, 1, 0] = 1.0                                   # drone 0 of every env at (0, 0, 1), drone 1 a metre away
    env = mds.CtrlAviary(drone_model=mds.DroneModel.CF2P, num_drones=2, initial_xyzs=xyz, initial_rpys=rpy, num_envs=4,
                         physics=mds.Physics.DYN)
    ptrs = (C.c_void_p * 2)()
    good = capi.MdsEpisodeSafety(0.03, 2.0, 0, 0)
    assert lib.mds_set_episode_safety(env._h, C.byref(good), None, None) == -5
    assert lib.mds_episode_safety_ptrs(env._h, ptrs) == -5
    with pytest.raises(capi.MdsError):
        env.set_episode_safety(0.03)
    env.set_episodes(max_steps=5)
    assert lib.mds_episode_safety_ptrs(env._h, ptrs) == -5
    ob = np.array([[0.0, 0.0, 1.0, 0.1]] * 17)
    obp = ob.ctypes.data_as(C.POINTER(C.c_double))
    for bad in (dict(safety_radius=0.0), dict(safety_radius=-0.1), dict(safety_radius=np.inf), dict(safety_radius=np.nan), dict(zscale=0.0),
                dict(zscale=-2.0), dict(zscale=np.inf), dict(zscale=np.nan), dict(n_obs=-1), dict(n_obs=17)):
        p = capi.MdsEpisodeSafety(0.03, 2.0, 0, 0)
        for k, v in bad.items():
            setattr(p, k, v)
        assert lib.mds_set_episode_safety(env._h, C.byref(p), obp, None) == -1, bad
    one = capi.MdsEpisodeSafety(0.03, 2.0, 1, 0)
    assert lib.mds_set_episode_safety(env._h, C.byref(one), None, None) == -1                   # n_obs > 0 without a list
    for bad_ob in ([0.0, 0.0, 1.0, -0.1], [np.nan, 0.0, 1.0, 0.1], [0.0, np.inf, 1.0, 0.1]):
        b = np.array([bad_ob])
        assert lib.mds_set_episode_safety(env._h, C.byref(one), b.ctypes.data_as(C.POINTER(C.c_double)), None) == -1, bad_ob
    assert lib.mds_episode_safety_ptrs(env._h, ptrs) == -5                                     # every refusal left the handle as it was
    assert lib.mds_set_episode_safety(env._h, None, None, None) == 0
    assert lib.mds_set_episode_safety(env._h, C.byref(one), obp, None) == 0
    assert lib.mds_episode_safety_ptrs(env._h, ptrs) == 0 and ptrs[0] and ptrs[1]
    # a refused re-configuration keeps the set: the sphere around drone 0 of every env still ends the envs at the first step, on bit 15 alone
    assert lib.mds_set_episode_safety(env._h, C.byref(capi.MdsEpisodeSafety(-1.0, 2.0, 0, 0)), None, None) == -1
    acts = mds.torch.full((1, 4, 2, 4), float(env.HOVER_RPM), dtype=env.dtype, device="cuda")
    flags_log = mds.torch.zeros((1, 4), dtype=mds.torch.int32, device="cuda")
    env.rollout_episodes(acts, 0, 1, None, None, flags_log)
    assert (flags_log.cpu().numpy() == (1 | (1 << 15))).all()
    env.set_episodes(enabled=False)
    assert lib.mds_set_episode_safety(env._h, C.byref(good), None, None) == -5
    env.close()

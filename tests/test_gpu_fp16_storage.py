"""The fp16-storage instantiations of the step and rollout kernels (dtype="float16": BASELINE config 5) against the storage-faithful
float64 model of tests/fp16_oracle.py, under its one acceptance rule
    |h - u| <= ulp16(u) / 2 + 2^-17 max(|u|, m)
-- a stored component one unit off, a double rounding, a row packed from the rounded state, a substep that re-rounds or a wrong column of
the 40-byte row writer all fail it.  37 x 7 = 259 drones (one full workgroup, then a wave of 3 rows: an odd row count, the 8-byte tail of
write_obs_rows), 1 x 1, and 37 x 8 = 296 (a partial wave of 40 rows, every slot 16-byte aligned) for everything that writes a multi-slot
log or ring.  fp16-exact local states on fp32-exact centres (multiples of 2^-6); env 0's centres are not fp32-exact.  After every launch
the model takes the kernel's stored planes (sync), so each launch is judged on its own inputs; a call that launches several kernels is
followed through its hidden roundings by the model's fork.  Every observation, log and ring buffer has two sentinel rows behind the last
drone's.  The inputs are chosen from the model alone so that the rule is sharp (fp16_oracle.sharp_inputs); each test asserts that 95 %
of every column group is.  (a)-(i) below mark the groups of cases."""
import numpy as np
import pytest

from oracle import np_oracle as O
from tests import fp16_oracle as F
from tests.test_gpu_parity import make_env, mds  # noqa: F401  (mds: the module's fixture)

pytestmark = pytest.mark.gpu

SENTINEL = 12344.0            # (fp16-exact)
SHAPES = [(37, 7), (1, 1)]
_CASES = {}


class Case:
    pass


def case(key, E, D, seed, plan_fn, pyb=100, ctrl=100, integrator="euler", drag=False, K=None, sharp=8, still=False):
    """Inputs of one flight, from the model alone, shared by the tests that fly it: centres, Lemniscates, action table, the launches
    (plan) and local states that keep the rule sharp and the flight well conditioned along them, for every drone.  still: drone n - 2
    (c.still) is at rest with four equal RPM in every action set -- no torque, w stays 0: integrate_q's identity arm."""
    if key in _CASES:
        return _CASES[key]
    c = Case()
    rng = np.random.default_rng(seed)
    c.E, c.D, c.n = E, D, E * D
    c.pyb, c.ctrl, c.integrator, c.drag, c.K = pyb, ctrl, integrator, drag, K
    c.cen = F.draw_centres(rng, E, D)
    c.P = F.draw_lemniscates(rng, c.cen)
    c.acts = F.draw_actions(rng, 3, c.n)
    c.still = c.n - 2 if still and c.n >= 3 else None
    pin = None
    if c.still is not None:
        c.acts[:, c.still, :] = c.acts[:, c.still, 0:1]

        def pin(x):
            x[c.still, 10:13] = 0.0
    c.plan = plan_fn(c)
    c.x, left = F.sharp_inputs(rng, c.n, lambda x, idx: new_model(c, x, idx), c.plan, sharp=sharp, pin=pin)
    assert left == 0                                              # (no drone left that is not sharp and well conditioned)
    _CASES[key] = c
    return c


def new_model(c, x=None, idx=None):
    """the model after reset at the centres, set_trajectories and set_state (idx: the drones of a tiled batch)"""
    idx = np.arange(c.n) if idx is None else idx
    m = F.Fp16Aviary(len(idx), c.pyb, c.ctrl, c.integrator, c.drag)
    m.K = c.K
    m.reset(c.cen.reshape(-1, 3)[idx], np.zeros((len(idx), 3)))
    m.set_trajectories(c.P.reshape(-1, 7)[idx])
    m.sync(c.x[idx] if x is None else x)                          # (x: the states of the drones idx)
    return m


def new_env(mds, c, idx=None, lqr=False):
    """-> (env, its observation buffer [n + 2, 20] with two sentinel rows, the LQRController or None)"""
    torch = mds.torch
    idx = np.arange(c.n) if idx is None else idx
    E, D = (c.E, c.D) if len(idx) == c.n else (len(idx), 1)
    cen, P, x = c.cen.reshape(-1, 3)[idx], c.P.reshape(-1, 7)[idx], c.x[idx]
    env = make_env(mds, E, D, cen.reshape(E, D, 3), np.zeros((E, D, 3)), "float16", c.pyb, c.ctrl,
                   mds.Physics.PYB_DRAG if c.drag else None, c.integrator)
    env.set_trajectories(P.reshape(E, D, 7))
    ctrl = None
    if lqr:
        from multidronesim_amd.control import LQRController
        from multidronesim_amd.model import LinearizedModel
        ctrl = LQRController(env, LinearizedModel(env))
    world = x.copy()
    world[:, 0:3] += F.f32(cen)                                   # exact: the stored position is x again
    env.set_state(world)
    obs = torch.full((E * D + 2, 20), SENTINEL, dtype=env.dtype, device=env.device)
    # (the step and rollout calls write through env._obs.data_ptr(): BaseAviary's observation buffer, replaced by a view of the larger one)
    assert env._obs.shape == (E, D, 20) and env._obs.dtype == obs.dtype
    env._obs = obs[:E * D].view(E, D, 20)
    return env, obs, ctrl


def planes_of(env):
    """the 13 stored planes [n, 13] and the origin planes [n, 3], widened exactly"""
    import torch
    sv = env.state_views()
    return (torch.stack([p.double() for p in sv["comp"]], dim=1).cpu().numpy(), torch.stack([p.double() for p in sv["origin"]], dim=1).cpu().numpy())


def host(t):
    return t.detach().double().cpu().numpy().reshape(-1, t.shape[-1])


def judge_end(env, model, res, what, stats):
    """the stored planes against the end of the launch; then the model takes them"""
    planes, _ = planes_of(env)
    F.check_state(planes, res[-1], what, stats)
    model.commit()
    model.sync(planes)
    return planes


def report(what, stats):
    print(f"[fp16 storage] {what}: bit-equal share >= {100 * min(s[0] for s in stats):.3f} %, largest |h - u| - ulp/2 = {max(s[1] for s in stats):+.2e} fp16 units")


def advance(t, dt, k):
    for _ in range(k):
        t += dt
    return t


# --------------------------------------------------------------------------------------------- (a) state I/O
def _static_m(x, org):
    """the rule's scales for the observation of a state at rest in time (k_get_obs): no step, so no dt terms"""
    om = np.zeros((x.shape[0], 20))
    om[:, 0:3] = np.abs(x[:, 0:3]).max(axis=1, keepdims=True) + np.abs(org).max(axis=1, keepdims=True)
    om[:, 3:7], om[:, 7:10] = 1.0, np.pi
    om[:, 10:13], om[:, 13:16] = np.abs(x[:, 7:10]).max(axis=1, keepdims=True), np.abs(x[:, 10:13]).max(axis=1, keepdims=True)
    return om


def _static_inputs(E, D):
    """centres, Lemniscates, fp16-exact local states, initial positions (fp16-exact) and angles, redrawn from the model alone until the
    rule is sharp for every value the test compares: the observation of the state (R w included), the quaternion of the initial angles
    and the initial position re-based onto the centres"""
    rng = np.random.default_rng(3)
    n = E * D
    cen = F.draw_centres(rng, E, D).reshape(n, 3)
    P = F.draw_lemniscates(rng, cen.reshape(E, D, 3))
    org = F.f32(cen)

    def redraw(draw, sharp_rows):
        a = draw(n)
        for _ in range(200):
            bad = np.nonzero(~sharp_rows(a, np.arange(n)))[0]
            if bad.size == 0:
                return a
            a[bad] = draw(bad.size)
        raise AssertionError("no sharp inputs found")

    def obs_sharp(x, idx):
        m = F.Fp16Aviary(len(idx))
        m.origin = org[idx]
        return F.sharp_share(m.exact_obs(x, np.zeros((len(idx), 4))), _static_m(x, org[idx]))
    x = redraw(lambda k: F.draw_local_states(rng, k), obs_sharp)
    xyz0 = redraw(lambda k: np.round(rng.uniform(-5, 5, size=(k, 3)) * 64) / 64,
                  lambda a, idx: F.sharp_share(a - org[idx], np.abs(a).max(axis=1, keepdims=True) + np.abs(cen[idx]).max(axis=1, keepdims=True)))
    rpy0 = redraw(lambda k: rng.uniform(0.12, 0.4, size=(k, 3)) * rng.choice([-1.0, 1.0], size=(k, 3)),
                  lambda a, idx: F.sharp_share(O.quat_from_euler_bullet(a), 1.0))
    return x, cen, P, xyz0, rpy0


@pytest.mark.parametrize("shape", SHAPES)
def test_state_io_rounds_once_and_rebases_in_double(mds, shape):  # noqa: F811
    torch = mds.torch
    E, D = shape
    n = E * D
    x, cen, P, xyz0, rpy0 = _static_inputs(E, D)
    env = make_env(mds, E, D, xyz0.reshape(E, D, 3), rpy0.reshape(E, D, 3), "float16")
    model = F.Fp16Aviary(n)
    # reset: zero origin, the poses rounded once, the rest zero
    model.reset(xyz0, rpy0)
    planes, org = planes_of(env)
    assert (org == 0).all() and np.array_equal(planes[:, 0:3], xyz0) and (planes[:, 7:13] == 0).all()
    F.assert_sharp(O.quat_from_euler_bullet(rpy0), 1.0, "reset q")
    F.assert_fp16(planes[:, 3:7], O.quat_from_euler_bullet(rpy0), 1.0, "reset q")
    # set_state on the zero origin: fp16-exact values arrive bit for bit
    w0 = x.copy()
    w0[:, 0:3] = xyz0
    env.set_state(w0)
    model.set_state(w0)
    planes, _ = planes_of(env)
    assert np.array_equal(planes, w0) and np.array_equal(planes, model.x)
    # set_trajectories: the origin planes are the fp32-rounded centres, the stored position is re-based in double and rounded once
    env.set_trajectories(P)
    model.set_trajectories(P)
    planes, org = planes_of(env)
    assert np.array_equal(org, F.f32(cen)) and (org[:D] != cen[:D]).all()                 # env 0: centres that fp32 does not hold
    m = np.abs(xyz0).max(axis=1, keepdims=True) + np.abs(cen).max(axis=1, keepdims=True)
    F.assert_sharp(model.rebased, m, "re-based p")
    F.assert_fp16(planes[:, 0:3], model.rebased, m, "re-based p")
    assert np.array_equal(planes[:, 0:3], F.f16(xyz0 - F.f32(cen))) and np.array_equal(planes[:, 3:], w0[:, 3:])
    # set_state on the new origin: world = local + origin gives the local values back bit for bit; get_state returns stored + origin
    world = x.copy()
    world[:, 0:3] += org
    env.set_state(world)
    model.set_state(world)
    planes, _ = planes_of(env)
    assert np.array_equal(planes, x) and np.array_equal(model.x, x)
    got = env.get_state().reshape(n, 13)
    exp = planes.copy()
    exp[:, 0:3] += org
    assert np.array_equal(got, exp)
    # _computeObs (k_get_obs): the rule, with the stored, unnormalised quaternion passed through
    obs = torch.full((n + 2, 20), SENTINEL, dtype=env.dtype, device=env.device)
    env._obs = obs[:n].view(E, D, 20)
    env._computeObs()
    rows = host(obs)
    u = model.exact_obs(model.x, np.zeros((n, 4)))
    rec = dict(obs=u, obs_m=_static_m(x, org), owner=np.arange(n), n=n, determined=np.ones(n, dtype=bool))
    stats = []
    F.check_obs(rows[:n], rec, "get_obs", stats=stats)                    # all six column groups, each asserted sharp
    assert np.array_equal(rows[:n, 3:7], x[:, 3:7]) and np.abs(np.linalg.norm(x[:, 3:7], axis=1) - 1).max() > 1e-5
    assert (rows[n:] == SENTINEL).all()
    report(f"(a) state I/O {shape}", stats)
    env.close()


# --------------------------------------------------------------------------------------------- (b) step
STEP_VARIANTS = {"euler240": dict(pyb=240, ctrl=240), "euler200_100": dict(pyb=200, ctrl=100), "rk4": dict(pyb=240, ctrl=240, integrator="rk4"),
                 "drag": dict(pyb=240, ctrl=240, drag=True)}


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("variant", sorted(STEP_VARIANTS))
def test_step(mds, variant, shape):  # noqa: F811
    """k_step: three successive steps of an action table with a row clipped at both ends and an all-zero row, re-synchronised; one
    drone at rest under equal RPM stays in integrate_q's identity arm (Euler: its stored quaternion, off unit norm, comes back as loaded)"""
    torch = mds.torch
    E, D = shape
    c = case(("step", variant, shape), E, D, 11, lambda c: [dict(kind="step", n_steps=1, actions=c.acts, a0=k) for k in range(3)], still=True, **STEP_VARIANTS[variant])
    env, obs, _ = new_env(mds, c)
    model = new_model(c)
    stats = []
    for k, kw in enumerate(c.plan):
        env.step(torch.as_tensor(c.acts[k].reshape(E, D, 4), dtype=env.dtype, device=env.device))
        res = model.launch(**kw)
        F.check_obs(host(obs)[:c.n], res[0], f"step {variant} {k}", stats=stats)
        planes = judge_end(env, model, res, f"step {variant} {k}", stats)
        if c.still is not None and c.integrator == "euler":       # the identity arm: q as loaded, not renormalised, in the model and in the kernel
            q0 = c.x[c.still, 3:7]
            assert abs(np.linalg.norm(q0) - 1) > 1e-5 and np.array_equal(res[0]["x"][c.still, 3:7], q0) and (res[0]["x"][c.still, 10:13] == 0).all()
            assert np.array_equal(planes[c.still, 3:7], q0) and np.array_equal(host(obs)[c.still, 3:7], q0) and (planes[c.still, 10:13] == 0).all()
    assert (host(obs)[c.n:] == SENTINEL).all()
    report(f"(b) step {variant} {shape}", stats)
    env.close()


# --------------------------------------------------------------------------------------------- (c) rollout_step
def _ring_launches(spl, steps=11):
    return [(j, min(spl, steps - j)) for j in range(0, steps, spl)]


@pytest.mark.parametrize("spl", [1, 5])
def test_rollout_step_ring(mds, spl):  # noqa: F811
    """mds_rollout_step / mds_rollout_step_fused (k_step per step / k_rollout_step): 3 action sets, a 4-slot ring, 11 steps at 296 drones;
    every slot a launch writes is judged, the slots it does not write keep their rows, and the planes are judged after every launch"""
    torch = mds.torch
    E, D, A, T = 37, 8, 3, 4
    c = case(("ring", spl), E, D, 12, lambda c: [dict(kind="step", n_steps=ks, actions=c.acts, a0=j % 3) for j, ks in _ring_launches(spl)])
    n = c.n
    env, obs, _ = new_env(mds, c)
    model = new_model(c)
    acts = torch.as_tensor(c.acts.reshape(A, E, D, 4), dtype=env.dtype, device=env.device)
    log = torch.full((T * n + 2, 20), SENTINEL, dtype=env.dtype, device=env.device)
    ring = log[:T * n].view(T, E, D, 20)
    held = np.full((T, n, 20), SENTINEL)
    stats = []
    for (j, ks), kw in zip(_ring_launches(spl), c.plan):
        env.rollout_step(acts, j, ks, ring, steps_per_launch=spl)
        res = model.launch(**kw)
        got = host(log)[:T * n].reshape(T, n, 20)
        for k in range(max(0, ks - T), ks):                          # (a launch of 5 steps overwrites its own first slot)
            slot = (j + k) % T
            F.check_obs(got[slot], res[k], f"ring spl {spl} step {j + k}", stats=stats)
            held[slot] = got[slot]
        assert np.array_equal(got, held)                              # the other slots: untouched
        judge_end(env, model, res, f"ring spl {spl} steps {j}..{j + ks - 1}", stats)
    assert (host(log)[T * n:] == SENTINEL).all()
    report(f"(c) rollout_step, {spl} step(s) per launch", stats)
    env.close()


# --------------------------------------------------------------------------------------------- (d) step_geometric
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("t", [0.0, 1000.0])
def test_step_geometric_with_action(mds, t, shape):  # noqa: F811
    """k_step_geometric with action_out: rows, the unclipped action and the planes; yaw rate 0.3 on every other env"""
    E, D = shape
    c = case(("geo", t, shape), E, D, 13, lambda c: [dict(kind="geometric", n_steps=1, t=t)])
    env, obs, _ = new_env(mds, c)
    model = new_model(c)
    o, act = env.step_geometric(t, return_action=True)
    res = model.launch(**c.plan[0])
    stats = []
    F.check_obs(host(obs)[:c.n], res[0], f"step_geometric t {t}", stats=stats)
    F.assert_sharp(res[0]["act"], 0.0, "action_out")
    stats.append(F.assert_fp16(host(act), res[0]["act"], 0.0, f"step_geometric t {t} action_out"))
    judge_end(env, model, res, f"step_geometric t {t}", stats)
    assert (host(obs)[c.n:] == SENTINEL).all()
    report(f"(d) step_geometric t {t} {shape}", stats)
    env.close()


# --------------------------------------------------------------------------------------------- (e) rollout_geometric, (h) ragged against aligned
def _rollout_launches(form, steps=9):
    return [1] * steps if form == 1 else [7, steps - 7]


def _rollout_plan(form, steps=9, t=0.0, dt=0.01):
    plan = []
    for ks in _rollout_launches(form, steps):
        plan.append(dict(kind="geometric", n_steps=ks, t=t))
        t = advance(t, dt, ks)
    return plan


_FLOWN = {}


def _fly_rollout(mds, c, form, every, idx=None):
    """one mds_rollout_geometric call of 9 steps -> (rows [n, 20], planes [n, 13], the sentinel rows); flown once per argument set"""
    key = (id(c), form, every, None if idx is None else len(idx))
    if key not in _FLOWN:
        env, obs, _ = new_env(mds, c, idx)
        env.set_rollout_form(form, 7)
        env.rollout_geometric(0.0, 9, obs_every_step=every)
        assert env.last_rollout_form() == form
        n = c.n if idx is None else len(idx)
        _FLOWN[key] = (host(obs)[:n], planes_of(env)[0], host(obs)[n:])
        env.close()
    return _FLOWN[key]


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("every", [True, False])
@pytest.mark.parametrize("form", [1, 2])
def test_rollout_geometric(mds, form, every, shape):  # noqa: F811
    """mds_rollout_geometric, 9 steps in one call: form 1 = nine k_step_geometric launches (the state rounded after each), form 2 forced =
    k_rollout_geometric in launches of 7 + 2, rewriting the rows in place or writing the last step's only.  The roundings between the
    launches are out of sight: the model forks at them."""
    E, D = shape
    c = case(("rollout", form, shape), E, D, 14, lambda c: _rollout_plan(form))
    rows, planes, tail = _fly_rollout(mds, c, form, every)
    model = new_model(c)
    for j, kw in enumerate(c.plan):
        res = model.launch(**kw)
        if j + 1 < len(c.plan):
            model.commit(fork=True)
    assert model.determined.all()                                 # no cap on the candidates: every drone is judged
    stats = []
    F.check_end(rows, planes, res[-1], f"rollout_geometric form {form}", stats)
    assert (tail == SENTINEL).all()
    report(f"(e) rollout_geometric form {form}, obs_every_step {every}, {shape} ({model.x.shape[0]} candidates of {c.n} drones)", stats)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("every", [True, False])
def test_ragged_shard_equals_wave_aligned_batch_fp16(mds, every, shape):  # noqa: F811
    """(h) the fp16 twin of test_gpu_whole_wave's test: the 259- and 1-drone results of the whole-rollout kernel (rows in place / the last
    step's only) are bit-equal to the same drones flown inside a wave-aligned batch of 512"""
    E, D = shape
    c = case(("rollout", 2, shape), E, D, 14, lambda c: _rollout_plan(2))
    rows, planes, _ = _fly_rollout(mds, c, 2, every)
    idx = np.arange(512) % c.n
    rrows, rplanes, _ = _fly_rollout(mds, c, 2, every, idx)
    assert np.array_equal(rows.view(np.int64), rrows[:c.n].view(np.int64)) and np.array_equal(planes.view(np.int64), rplanes[:c.n].view(np.int64))


@pytest.mark.parametrize("dest", ["log", "last"])
def test_fused_rollout_equals_wave_aligned_batch_fp16(mds, dest):  # noqa: F811
    """(h) the same for mds_rollout_geometric_fused's results: the last step's rows only at 259 drones, the [7, n, 20] log at 296, against
    the same drones inside a batch of 512"""
    torch = mds.torch
    E, D, steps = (37, 8, 7) if dest == "log" else (37, 7, 7)
    c = case(("fused", dest, "geometric"), E, D, 15, lambda c: [dict(kind="geometric", n_steps=steps, t=0.0)])
    out = []
    for idx in (None, np.arange(512) % c.n):
        env, obs, _ = new_env(mds, c, idx)
        n = env.n
        log = torch.full((steps * n + 2, 20), SENTINEL, dtype=env.dtype, device=env.device) if dest == "log" else None
        env.rollout_geometric_fused(0.0, steps, log=dest == "log", log_out=None if log is None else log[:steps * n].view(steps, env.NUM_ENVS, env.NUM_DRONES, 20))
        out.append((host(obs)[:n], planes_of(env)[0], None if log is None else host(log)[:steps * n].reshape(steps, n, 20)))
        assert (host(obs)[n:] == SENTINEL).all() and (log is None or (host(log)[steps * n:] == SENTINEL).all())
        env.close()
    (rows, planes, log), (rrows, rplanes, rlog) = out
    assert np.array_equal(rows.view(np.int64), rrows[:c.n].view(np.int64)) and np.array_equal(planes.view(np.int64), rplanes[:c.n].view(np.int64))
    assert log is None or np.array_equal(log.view(np.int64), np.ascontiguousarray(rlog[:, :c.n]).view(np.int64))


# --------------------------------------------------------------------------------------------- (f) rollout_geometric_fused, (g) LQR
@pytest.mark.parametrize("controller", ["geometric", "lqr"])
@pytest.mark.parametrize("dest", ["log", "last"])
def test_rollout_fused(mds, dest, controller):  # noqa: F811
    """k_rollout_geometric in one launch of 7 steps: every row of every step of the [7, n, 20] log at 296 drones, the last step's rows only at
    259 (with (e)'s in-place rows: the three row destinations of the kernel); with the geometric controller and the 12-state LQR"""
    torch = mds.torch
    E, D, steps = (37, 8, 7) if dest == "log" else (37, 7, 7)
    K = O.lqr12_gain(O.CF2P) if controller == "lqr" else None
    c = case(("fused", dest, controller), E, D, 15, lambda c: [dict(kind=controller, n_steps=steps, t=0.0)], K=K)
    n = c.n
    env, obs, ctrl = new_env(mds, c, lqr=controller == "lqr")
    model = new_model(c)
    if ctrl is not None:
        np.testing.assert_allclose(ctrl.K, K, rtol=1e-9, atol=1e-12)       # the gain the inputs were chosen with is the handle's
        model.K = np.asarray(ctrl.K, dtype=np.float64)
    log = torch.full((steps * n + 2, 20), SENTINEL, dtype=env.dtype, device=env.device) if dest == "log" else None
    env.rollout_geometric_fused(0.0, steps, log=dest == "log", log_out=None if log is None else log[:steps * n].view(steps, E, D, 20), controller=controller)
    res = model.launch(**c.plan[0])
    stats = []
    last = host(obs)
    if log is not None:
        got = host(log)
        for k in range(steps):
            F.check_obs(got[k * n:(k + 1) * n], res[k], f"fused {controller} log step {k}", stats=stats)
        assert np.array_equal(got[(steps - 1) * n:steps * n], last[:n]) and (got[steps * n:] == SENTINEL).all()
    F.check_obs(last[:n], res[-1], f"fused {controller} last", stats=stats)
    judge_end(env, model, res, f"fused {controller} {dest}", stats)
    assert (last[n:] == SENTINEL).all()
    report(f"(f/g) rollout_geometric_fused {controller} {dest}", stats)
    env.close()


@pytest.mark.parametrize("shape", SHAPES)
def test_step_lqr(mds, shape):  # noqa: F811
    """(g) k_step_lqr with action_out, the gain set as test_fp16_storage_instantiations_of_the_lqr_paths sets it"""
    E, D = shape
    c = case(("lqr", shape), E, D, 16, lambda c: [dict(kind="lqr", n_steps=1, t=0.0)], K=O.lqr12_gain(O.CF2P))
    env, obs, ctrl = new_env(mds, c, lqr=True)
    model = new_model(c)
    np.testing.assert_allclose(ctrl.K, c.K, rtol=1e-9, atol=1e-12)
    model.K = np.asarray(ctrl.K, dtype=np.float64)
    o, act = env.step_lqr(0.0, return_action=True)
    res = model.launch(**c.plan[0])
    stats = []
    F.check_obs(host(obs)[:c.n], res[0], "step_lqr", stats=stats)
    F.assert_sharp(res[0]["act"], 0.0, "action_out")
    stats.append(F.assert_fp16(host(act), res[0]["act"], 0.0, "step_lqr action_out"))
    judge_end(env, model, res, "step_lqr", stats)
    assert (host(obs)[c.n:] == SENTINEL).all()
    report(f"(g) step_lqr {shape}", stats)
    env.close()


# --------------------------------------------------------------------------------------------- (i) refusals
def test_misaligned_fp16_logs_are_refused(mds):  # noqa: F811
    """(i) fp16 rows are 40 bytes: with an odd n, slot k of a log or ring starts at 40 n k bytes, 8 mod 16 for odd k, and the row writer
    stores 16-byte chunks.  Every entry point refuses that shape with MDS_EALIGN (-4, include/mds.h) before any launch; one-step logs and even n are served."""
    torch = mds.torch
    from multidronesim_amd import _capi as capi
    from multidronesim_amd.control import LQRController
    from multidronesim_amd.model import LinearizedModel
    E, D = 37, 7
    c = case(("refuse",), E, D, 17, lambda c: [dict(kind="geometric", n_steps=1, t=0.0)])
    env, obs, _ = new_env(mds, c)
    LQRController(env, LinearizedModel(env))
    n = c.n
    # (one action set: with an odd n a table of several sets is misaligned too, and refused for that; here the log is the reason)
    acts = torch.as_tensor(c.acts[:1].reshape(1, E, D, 4), dtype=env.dtype, device=env.device)
    ring = torch.full((4, E, D, 20), SENTINEL, dtype=env.dtype, device=env.device)
    assert (n * 20 * ring.element_size()) % 16 == 8
    before, _ = planes_of(env)
    refused = [lambda: env.rollout_step(acts, 0, 4, ring), lambda: env.rollout_step(acts, 0, 4, ring, steps_per_launch=5),
               lambda: env.rollout_geometric_fused(0.0, 2, log=True, log_out=ring[:2]),
               lambda: env.rollout_geometric_fused(0.0, 2, log=True, log_out=ring[:2], controller="lqr")]
    for call in refused:
        with pytest.raises(capi.MdsError) as ei:
            call()
        assert ei.value.status == -4 and "16-byte aligned" in str(ei.value)
    torch.cuda.synchronize()
    assert (ring == SENTINEL).all() and np.array_equal(planes_of(env)[0], before)         # nothing ran
    # accepted: a one-slot ring, a one-step log (both controllers), each in a buffer of its own (16-byte aligned); even n with a
    # multi-step log is test_rollout_fused's case
    one = [torch.full((1, E, D, 20), SENTINEL, dtype=env.dtype, device=env.device) for _ in range(4)]
    env.rollout_step(acts, 0, 1, one[0])
    env.rollout_step(acts, 1, 1, one[1], steps_per_launch=5)
    env.rollout_geometric_fused(0.0, 1, log=True, log_out=one[2])
    env.rollout_geometric_fused(0.0, 1, log=True, log_out=one[3], controller="lqr")
    torch.cuda.synchronize()
    for o in one:
        assert torch.isfinite(o).all() and (o != SENTINEL).any(dim=-1).all()
    env.close()

"""TEST TOOLING ONLY -- the storage-faithful float64 model of a ``dtype="float16"`` handle (fp16 storage of the state, the actions and the
observations, fp32 arithmetic), and the one acceptance rule its tests use.  Built on oracle/np_oracle.py, which stays as it is (its
``integrate_q`` does not renormalise: the reference's behaviour, pinned by other fixtures).

What the kernels do (csrc/mds_kernels.hip, csrc/mds_math.hpp), restated here:
  * the state is 13 fp16 values per drone, widened exactly (load_state); positions are relative to the per-drone origin, an fp32 plane:
    zero on a fresh handle, the fp32-rounded Lemniscate centre after set_trajectories, which re-bases the stored position in double
    (k_set_origin: stored + old origin - new origin, rounded once);
  * the stored quaternion stands for the rotation q / |q|: the thrust direction, the controller's R, the Euler angles and ang_v = R w all
    come from quat_to_rot_m1, which divides by |q|^2.  integrate_q is linear in q and renormalises after every substep, except in its
    |w|^2 <= 1e-16 arm, which returns q as loaded.  step_rk4 runs its stages on unnormalised quaternions (thrust_dir scale invariant, qdot
    linear) and renormalises once at the end of the substep;
  * a control step widens the action, clips it to [0, MAX_RPM] and runs every substep in registers: nothing is rounded between substeps;
  * the observation is packed from the registers after the step (pack_obs): p_local + origin, q, rpy, v, R w, the clipped RPM; each of the
    20 values is rounded once (write_obs_rows).  action_out is the unclipped action, rounded once (it may be inf);
  * the state is rounded once per LAUNCH (store_state at the kernel's end): after every control step for k_step / k_step_geometric /
    k_step_lqr, after the launch's steps for k_rollout_step / k_rollout_geometric, whose per-step rows still come from the registers;
  * the drag term reads the previous clipped RPM from an fp32 plane (never through fp16);
  * the controllers read the state as loaded: np_oracle's geometric_compute / lqr12_compute on the exact world-frame observation of the
    loaded state (not rounded), with the trajectory time a double and the Lemniscate parameters as their fp32 planes hold them.

Acceptance rule (assert_fp16), with u the exact float64 result and h the kernel's fp16 value:
    |h - u| <= ulp16(u) / 2 + 2^-17 max(|u|, m)
2^-17 = 128 fp32 units for the fp32 arithmetic (2^-6 .. 2^-7 of an fp16 unit); m is the scale of the terms summed into the value:
p: max|p| + dt max|v|; v: max|v| + dt g; w: max|w| + dt max|w'|; ang_v: max|w|; q: 1; rpy: pi; RPM: |u|  (maxima over the drone's three
components; an observation's world position adds max|origin|).  The rule is sharp where 2^-17 max(|u|, m) <= ulp16(u) / 8:
assert_sharp asks that of 95 % of every column group, from the reference alone.

Launches that cannot be re-synchronised (a call that launches several kernels) round the state between launches where the caller cannot
see it.  A value whose exact result lies within the rule's allowance of an fp16 rounding boundary may legitimately be stored either way,
and the next launch starts from whichever it was: commit(fork=True) carries both candidates (rows of the model, `owner` = the drone), and
a drone passes when one candidate explains every one of its values -- the observation row and the stored planes together (check_end).
The tests set no cap on the candidates, so every drone is judged (commit's `cap` would keep a drone's first candidate only and mark it
undetermined; the tests assert that none is)."""
import numpy as np

from oracle import np_oracle as O

ALLOW = 2.0 ** -17
OBS_GROUPS = {"p": slice(0, 3), "q": slice(3, 7), "rpy": slice(7, 10), "v": slice(10, 13), "ang_v": slice(13, 16), "rpm": slice(16, 20)}
STATE_GROUPS = {"p": slice(0, 3), "q": slice(3, 7), "v": slice(7, 10), "w": slice(10, 13)}


def f16(x):
    """round to nearest even through np.float16 (one rounding from float64)"""
    with np.errstate(over="ignore"):
        return np.asarray(x, dtype=np.float64).astype(np.float16).astype(np.float64)


def f32(x):
    return np.asarray(x, dtype=np.float64).astype(np.float32).astype(np.float64)


def ulp16(u):
    """spacing of the fp16 binade that holds |u|; 2^-24 below 2^-14"""
    a = np.abs(np.asarray(u, dtype=np.float64))
    _, ex = np.frexp(a)                                                # |u| = f 2^ex, f in [0.5, 1)  (frexp(0) = (0, 0))
    return np.ldexp(1.0, np.maximum(np.where(a == 0, -14, ex - 1), -14) - 10)


def _allowance(u, m):
    return ALLOW * np.maximum(np.abs(u), m)


def excess16(h, u, m):
    """(|h - u| - ulp16(u)/2 - allowance) and (|h - u| - ulp16(u)/2), both in fp16 units of u; an inf is right only where f16(u) is inf"""
    h, u = np.asarray(h, dtype=np.float64), np.asarray(u, dtype=np.float64)
    m = np.broadcast_to(np.asarray(m, dtype=np.float64), u.shape)
    ul = ulp16(u)
    with np.errstate(invalid="ignore"):
        d = np.abs(h - u)
    big = np.isinf(f16(u))
    d = np.where(big, np.where(h == f16(u), 0.0, np.inf), d)
    d = np.where(np.isnan(d), np.inf, d)
    raw = (d - 0.5 * ul) / ul
    return raw - _allowance(u, m) / ul, raw


def assert_sharp(u, m, what, share=0.95):
    """the rule's allowance is at most an eighth of an fp16 unit for `share` of the values: from the reference alone"""
    u = np.asarray(u, dtype=np.float64)
    m = np.broadcast_to(np.asarray(m, dtype=np.float64), u.shape)
    s = float(np.mean(_allowance(u, m) <= ulp16(u) / 8))
    assert s >= share, f"{what}: the rule is sharp for {100 * s:.1f} % of the values only: choose other inputs"
    return s


def assert_fp16(h, u, m, what, owner=None, n=None, judge=None):
    """The acceptance rule on arrays [rows, k] (h: [n, k]).  owner (rows -> drone, from a forked model): a drone passes when one of its
    candidate rows passes in every value.  -> (bit-equal share, largest |h - u| - ulp/2 in fp16 units among the values for which the rule is
    sharp) of the rows that explain the drones."""
    u = np.asarray(u, dtype=np.float64)
    h = np.asarray(h, dtype=np.float64)
    if owner is None:
        owner, n = np.arange(u.shape[0]), u.shape[0]
    ex, raw = excess16(h[owner], u, m)
    worst = ex.reshape(len(owner), -1).max(axis=1)                  # per candidate row
    best = np.full(n, np.inf)
    np.minimum.at(best, owner, worst)
    pick = np.full(n, -1)
    rows = np.nonzero(worst == best[owner])[0]
    pick[owner[rows][::-1]] = rows[::-1]                            # the first best row of each drone
    pick = pick[pick >= 0]
    eq = float(np.mean(h[owner[pick]] == f16(u[pick])))
    mm = np.broadcast_to(np.asarray(m, dtype=np.float64), u.shape)
    sharp = _allowance(u[pick], mm[pick]) <= ulp16(u[pick]) / 8
    top = float(np.where(sharp, raw[pick], -0.5).max())
    print(f"[fp16 rule] {what}: {100 * eq:.3f} % bit-equal, largest |h - u| - ulp/2 = {top:+.2e} fp16 units among the "
          f"{100 * sharp.mean():.1f} % sharp values, {float(raw[pick].max()):+.2e} among all {u[pick].size}")
    bad = np.nonzero((best > 0) & (True if judge is None else judge))[0]
    assert bad.size == 0, (f"{what}: {bad.size} of {n} drones outside |h - u| <= ulp16/2 + 2^-17 max(|u|, m); first drone {bad[0]}, "
                           f"excess {best[bad].max():.3e} fp16 units over the allowance")
    return eq, top


def check_obs(h, res, what, groups=OBS_GROUPS, stats=None):
    """every column group of observation rows h [n, 20] against one step's exact rows of a launch (res: Fp16Aviary.launch's step record)"""
    n = res["n"]                       # (the drones' first candidates: a fork does not weigh a drone by the number of its candidates)
    for name, sl in groups.items():
        assert_sharp(res["obs"][:n, sl], res["obs_m"][:n, sl], f"{what} {name}")
    # a candidate must explain the whole row: the groups are judged together, reported apart
    assert_fp16(h, res["obs"], res["obs_m"], f"{what} row", res["owner"], res["n"], res["determined"])
    for name, sl in groups.items():
        r = assert_fp16(h[:, sl], res["obs"][:, sl], res["obs_m"][:, sl], f"{what} {name}", res["owner"], res["n"], res["determined"])
        if stats is not None:
            stats.append(r)


def check_state(h, res, what, stats=None):
    """the 13 stored planes h [n, 13] against the end of a launch"""
    n = res["n"]
    for name, sl in STATE_GROUPS.items():
        assert_sharp(res["x"][:n, sl], res["x_m"][:n, sl], f"{what} state {name}")
    assert_fp16(h, res["x"], res["x_m"], f"{what} state", res["owner"], res["n"], res["determined"])
    for name, sl in STATE_GROUPS.items():
        r = assert_fp16(h[:, sl], res["x"][:, sl], res["x_m"][:, sl], f"{what} state {name}", res["owner"], res["n"], res["determined"])
        if stats is not None:
            stats.append(r)


def check_end(h_obs, h_planes, res, what, stats=None):
    """the last step's rows and the stored planes of a launch: every group of each, and ONE candidate of a forked model must explain a
    drone's row and planes together"""
    check_obs(h_obs, res, what, stats=stats)
    check_state(h_planes, res, what, stats)
    assert_fp16(np.concatenate([h_obs, h_planes], axis=1), np.concatenate([res["obs"], res["x"]], axis=1),
                np.concatenate([res["obs_m"], res["x_m"]], axis=1), f"{what} row and state", res["owner"], res["n"], res["determined"])


def sharp_share(u, m, sharp=8):
    """per row: is every value's allowance at most ulp16 / sharp"""
    u = np.asarray(u, dtype=np.float64)
    return (_allowance(u, np.broadcast_to(np.asarray(m, dtype=np.float64), u.shape)) <= ulp16(u) / sharp).all(axis=-1)


def _amax(a):
    return np.abs(a).max(axis=-1, keepdims=True)


class Fp16Aviary:
    """n drones of a float16 handle.  x [rows, 13]: p (local), q, v, w as stored (fp16 values in float64); rows = n until a fork."""

    def __init__(self, n, pyb_freq=100, ctrl_freq=100, integrator="euler", drag=False, consts=O.CF2P):
        self.n, self.c = n, consts
        self.substeps, self.dt, self.ctrl_dt = pyb_freq // ctrl_freq, 1.0 / pyb_freq, 1.0 / ctrl_freq
        self.rk4, self.drag = integrator == "rk4", drag
        self.owner = np.arange(n)
        self.determined = np.ones(n, dtype=bool)
        self.x = np.zeros((n, 13))
        self.x[:, 6] = 1.0
        self.origin = np.zeros((n, 3))          # fp32 planes
        self.rpm_prev = np.zeros((n, 4))        # fp32 planes
        self.lem = None                          # [rows, 7] as the fp32 planes hold them (a, omega, centre3, yaw_rate, phase_shift)
        self.K = None                            # LQRController's [4, 12]
        self._end = None

    # ------------------------------------------------------------------ state I/O (k_reset, k_set_state, k_set_origin, k_get_state)
    def reset(self, xyz, rpy):
        """k_reset: the poses relative to the origin planes AS THEY ARE (mds_reset does not touch them: zero on a fresh handle, the
        centres after a set_trajectories), rounded once; zero velocities, rates and RPM echo"""
        self._unfork()
        self.x[:] = 0.0
        self.x[:, 0:3] = f16(np.asarray(xyz, dtype=np.float64).reshape(-1, 3) - self.origin)
        self.x[:, 3:7] = f16(O.quat_from_euler_bullet(np.asarray(rpy, dtype=np.float64).reshape(-1, 3)))
        self.rpm_prev[:] = 0.0

    def set_state(self, world13):
        self._unfork()
        s = np.array(world13, dtype=np.float64).reshape(-1, 13)
        s[:, 0:3] -= self.origin
        self.x = f16(s)

    def get_state(self):
        s = self.x[:self.n].copy()
        s[:, 0:3] += self.origin[:self.n]
        return s

    def set_trajectories(self, P):
        self._unfork()
        P = np.asarray(P, dtype=np.float64).reshape(-1, 7)
        new = f32(P[:, 2:5])
        self.rebased = self.x[:, 0:3] + self.origin - new                 # exact in double: what k_set_origin rounds
        self.x[:, 0:3] = f16(self.rebased)
        self.origin = new
        self.lem = f32(P)

    def sync(self, planes):
        """the kernel's stored planes [n, 13] (local) become the model's state: each launch is judged on its own inputs"""
        self._unfork()
        self.x = np.array(planes, dtype=np.float64).reshape(self.n, 13)

    def _unfork(self):
        n = self.n
        self.owner, self.determined = np.arange(n), np.ones(n, dtype=bool)
        self.x, self.origin, self.rpm_prev = self.x[:n], self.origin[:n], self.rpm_prev[:n]
        if self.lem is not None:
            self.lem = self.lem[:n]

    # ------------------------------------------------------------------ the exact observation of a register state (pack_obs)
    def exact_obs(self, x, rpm):
        q = x[:, 3:7]
        R = O.quat_to_rotmat_bullet(q)                                    # s = 2 / |q|^2: the rotation of q / |q|
        rpy = O.euler_from_quat_bullet(q / O.norm(q)[:, None])
        return np.concatenate([x[:, 0:3] + self.origin, q, rpy, x[:, 7:10], O.matvec(R, x[:, 10:13]), rpm], axis=1)

    # ------------------------------------------------------------------ one control step on registers (aviary_step)
    def _rk4(self, p, q, v, w, rpm, prev):
        """step_rk4: the stages' quaternions are not normalised (thrust_dir is scale invariant, qdot is linear in q); one rsqrt at the end"""
        c, dt = self.c, self.dt

        def f(s):
            return O.dyn_derivative(s[0], s[1], s[2], s[3], rpm, c, prev if self.drag else None)
        s0 = (p, q, v, w)
        k1 = f(s0)
        k2 = f(tuple(a + 0.5 * dt * k for a, k in zip(s0, k1)))
        k3 = f(tuple(a + 0.5 * dt * k for a, k in zip(s0, k2)))
        k4 = f(tuple(a + dt * k for a, k in zip(s0, k3)))
        p, q, v, w = (a + (dt / 6.0) * ((b1 + b4) + 2.0 * (b2 + b3)) for a, b1, b2, b3, b4 in zip(s0, k1, k2, k3, k4))
        return p, q / O.norm(q)[:, None], v, w

    def _step(self, x, action, prev):
        c = self.c
        clipped = np.clip(action, 0.0, c.MAX_RPM)
        p, q, v, w = x[:, 0:3], x[:, 3:7], x[:, 7:10], x[:, 10:13]
        for _ in range(self.substeps):
            if self.rk4:
                p, q, v, w = self._rk4(p, q, v, w, clipped, prev)
            else:
                p, q, v, w, _ = O.dyn_step_euler(p, q, v, w, clipped, self.dt, c, prev if self.drag else None)
                still = np.isclose(O.norm(w), 0.0)                        # integrate_q's identity arm: q stays as it was, unnormalised
                q = np.where(still[:, None], q, q / O.norm(q)[:, None])
            prev = clipped
        return np.concatenate([p, q, v, w], axis=1), clipped, prev

    def _control(self, kind, x, t, jitter=None):
        L = self.lem
        pos, vel, acc, yaw, yd = O.lemniscate(t, L[:, 0], L[:, 1], L[:, 2:5], L[:, 5], L[:, 6])
        if jitter is not None:      # one fp32 unit on what the controller reads (local frame, as the kernels hold it): its sums' terms
            def eps(a):
                return 1.0 + 2.0 ** -24 * jitter.standard_normal(np.shape(a))
            x, vel, acc = x * eps(x), vel * eps(vel), acc * eps(acc)
            pos = L[:, 2:5] + (pos - L[:, 2:5]) * eps(pos)
        obs = self.exact_obs(x, np.zeros((x.shape[0], 4)))
        if kind == "geometric":
            return O.geometric_compute(obs, pos, vel, acc, yaw, yd, self.c)
        return O.lqr12_compute(obs, pos, vel, yaw, yd, self.K, self.c)[0]

    # ------------------------------------------------------------------ one kernel launch
    def launch(self, kind, n_steps=1, t=0.0, actions=None, a0=0, jitter=None):
        """n_steps control steps with the state in registers.  kind "step": step k applies actions[(a0 + k) % A] ([A, n, 4], fp16 values);
        "geometric" / "lqr": the fused controllers at t, t + ctrl_dt, ... (t accumulates as the kernels' does).
        -> one record per step {obs, obs_m [rows, 20], act [rows, 4] (the unclipped action), owner, n}; the last one also holds the end of
        the launch {x, x_m [rows, 13]}.  commit() then rounds the state.  jitter (a Generator; sharp_inputs' use): what the controller reads,
        every computed action and every step's registers are disturbed by one fp32 unit (relative 2^-24, normal), to see how far a flight
        carries such errors."""
        x, prev, rows, g = self.x.copy(), self.rpm_prev.copy(), self.x.shape[0], self.c.G
        xm = np.zeros((rows, 13))
        xm[:, 3:7] = 1.0
        out = []
        for k in range(n_steps):
            if kind == "step":
                A = np.asarray(actions, dtype=np.float64)
                act = A[(a0 + k) % A.shape[0]].reshape(self.n, 4)[self.owner]
            else:
                act = self._control(kind, x, t, jitter)
                t += self.ctrl_dt
            if jitter is not None and kind != "step":
                act = act * (1.0 + 2.0 ** -24 * jitter.standard_normal(act.shape))
            x1, clipped, prev = self._step(x, act, prev)
            if jitter is not None:
                x1 = x1 * (1.0 + 2.0 ** -24 * jitter.standard_normal(x1.shape))
            vmax = np.maximum(_amax(x[:, 7:10]), _amax(x1[:, 7:10]))
            mp = np.maximum(_amax(x[:, 0:3]), _amax(x1[:, 0:3])) + self.ctrl_dt * vmax
            mv = vmax + self.ctrl_dt * g
            mw = _amax(x[:, 10:13]) + _amax(x1[:, 10:13] - x[:, 10:13])
            om = np.zeros((rows, 20))
            om[:, 0:3] = mp + _amax(self.origin)
            om[:, 3:7], om[:, 7:10] = 1.0, np.pi
            om[:, 10:13], om[:, 13:16] = mv, _amax(x1[:, 10:13])
            xm[:, 0:3], xm[:, 7:10], xm[:, 10:13] = np.maximum(xm[:, 0:3], mp), np.maximum(xm[:, 7:10], mv), np.maximum(xm[:, 10:13], mw)
            out.append(dict(obs=self.exact_obs(x1, clipped), obs_m=om, act=act, owner=self.owner, n=self.n, determined=self.determined))
            x = x1
        if n_steps > 0:
            out[-1].update(x=x, x_m=xm.copy())
            self._end = (x, xm, f32(prev))
        return out

    def commit(self, fork=False, cap=None):
        """store_state at the end of the launch: one rounding of the registers.  fork: a value within the rule's allowance of a rounding
        boundary is carried both ways (see the module's docstring)."""
        x, xm, prev = self._end
        h = f16(x)
        self.rpm_prev = prev
        if not fork:
            self.x = h
            return
        h16 = h.astype(np.float16)
        other = np.nextafter(h16, np.where(x > h, np.float16(np.inf), np.float16(-np.inf)).astype(np.float16)).astype(np.float64)
        amb = np.abs(x - 0.5 * (h + other)) <= _allowance(x, xm)
        idx, X = np.arange(x.shape[0]), h.copy()
        for j in range(13):
            sel = np.nonzero(amb[idx, j])[0]
            if sel.size:
                dup = X[sel].copy()
                dup[:, j] = other[idx[sel], j]
                X, idx = np.concatenate([X, dup]), np.concatenate([idx, idx[sel]])
        own = self.owner[idx]
        over = np.bincount(own, minlength=self.n) > (np.inf if cap is None else cap)
        self.determined &= ~over
        keep = ~over[own] | (np.arange(len(idx)) < self.n)            # (the first n rows are the drones' first candidates, in order)
        idx, X = idx[keep], X[keep]
        self.x, self.owner = X, self.owner[idx]
        self.origin, self.rpm_prev = self.origin[idx], self.rpm_prev[idx]
        if self.lem is not None:
            self.lem = self.lem[idx]


# ---------------------------------------------------------------------------------------------- inputs
def draw_local_states(rng, n, tilt=(0.30, 0.40), p=(0.32, 1.5), v=(0.45, 2.0), w=(0.45, 2.0)):
    """fp16-exact local states [n, 13] whose values keep the rule sharp: magnitudes away from zero (p, v, w, roll and pitch in the given
    ranges, random signs; |yaw| in [0.3, 2.8]) and no quaternion component below 0.08."""
    def mag(lo_hi, shape):
        return rng.uniform(*lo_hi, size=shape) * rng.choice([-1.0, 1.0], size=shape)
    x = np.zeros((n, 13))
    x[:, 0:3], x[:, 7:10], x[:, 10:13] = mag(p, (n, 3)), mag(v, (n, 3)), mag(w, (n, 3))
    todo = np.arange(n)
    while todo.size:
        rpy = np.concatenate([mag(tilt, (todo.size, 2)), mag((0.3, 2.8), (todo.size, 1))], axis=1)
        q = O.quat_from_euler_bullet(rpy)
        ok = np.abs(q).min(axis=1) >= 0.08
        x[todo[ok], 3:7] = q[ok]
        todo = todo[~ok]
    return f16(x)


def sharp_inputs(rng, n, make_model, plan, tries=400, sharp=8, pin=None, **draw_kw):
    """Local states [n, 13] for which the rule is sharp along the whole flight `plan` (a list of Fp16Aviary.launch keyword sets): flown on
    the model alone (make_model(x, idx) -> a model of the drones idx holding x), a drone with an unsharp value anywhere (allowance above ulp16 / sharp) gets a
    new state, until none is left or `tries` run out.
    The same for conditioning.  The rule's 128 fp32 units allow for the arithmetic of a flight that carries rounding errors forward about
    as they are; near a singular point of the controller -- a commanded force through zero: m g less the feedback terms, with the tilt
    clamp scaling the rest by what is left -- a flight multiplies them by hundreds, in any precision.  So every candidate is flown a
    second time with one fp32 unit of noise on the controller's inputs, every action and every step's registers, and a drone whose exact
    results move by more than an eighth of the allowance gets a new state too.
    The reference alone decides; what the kernels give plays no part.  The tests still assert the 95 % themselves.
    pin(x): the caller's fixed entries, written into every draw (a drone at rest for integrate_q's identity arm).
    -> (x, the number of drones that were still not sharp and well conditioned when the tries ran out)"""
    pin = pin or (lambda x: None)
    x = draw_local_states(rng, n, **draw_kw)
    pin(x)
    todo = np.arange(n)                          # the drones still to be flown: make_model(x[todo], todo) -> a model of those drones
    for k in range(tries):
        model, noisy, ok = make_model(x[todo], todo), make_model(x[todo], todo), np.ones(todo.size, dtype=bool)
        for kw in plan:
            if kw.get("actions") is not None:
                A = np.asarray(kw["actions"], dtype=np.float64)
                kw = dict(kw, actions=A.reshape(A.shape[0], n, 4)[:, todo])
            res, res2 = model.launch(**kw), noisy.launch(jitter=rng, **kw)
            model.commit()
            noisy.commit()
            noisy.x = model.x.copy()                     # (both continue from the same stored state: one launch's conditioning at a time)
            for r, r2 in zip(res, res2):
                ok &= sharp_share(r["obs"], r["obs_m"], sharp)
                ok &= (np.abs(r2["obs"] - r["obs"]) <= _allowance(r["obs"], r["obs_m"]) / 8).all(axis=1)
            ok &= sharp_share(res[-1]["x"], res[-1]["x_m"], sharp)
            ok &= (np.abs(res2[-1]["x"] - res[-1]["x"]) <= _allowance(res[-1]["x"], res[-1]["x_m"]) / 8).all(axis=1)
        todo = todo[~ok]
        if todo.size == 0 or k + 1 == tries:     # (what is returned has been flown: the count is of these very states)
            break
        x[todo] = draw_local_states(rng, todo.size, **draw_kw)
        pin(x)
    return x, int(todo.size)


def draw_centres(rng, E, D, lo=1.0, hi=5.0, inexact_env=0):
    """[E, D, 3] fp32-exact centres, multiples of 2^-6 with lo <= |c| <= hi; env `inexact_env` gets centres that fp32 does not hold"""
    c = np.round(rng.uniform(lo, hi, size=(E, D, 3)) * 64) / 64 * rng.choice([-1.0, 1.0], size=(E, D, 3))
    if inexact_env is not None:
        c[inexact_env] += 0.001 * np.pi
        assert (f32(c[inexact_env]) != c[inexact_env]).all()
    return c


def draw_lemniscates(rng, centres, yaw_rate_every_other=0.3):
    E, D = centres.shape[:2]
    P = np.zeros((E, D, 7))
    P[..., 0], P[..., 1] = rng.uniform(0.5, 1.5, size=(E, D)), rng.uniform(0.8, 1.6, size=(E, D))
    P[..., 2:5] = centres
    P[::2, :, 5] = yaw_rate_every_other
    P[..., 6] = rng.uniform(-np.pi, np.pi, size=(E, D))
    return P


def draw_actions(rng, A, n, c=O.CF2P, spread=0.03):
    """[A, n, 4] fp16-exact RPM around hover, with one row clipped at both ends and one all-zero row"""
    a = c.HOVER_RPM * (1 + spread * rng.uniform(-1, 1, size=(A, n, 4)))
    a[min(1, A - 1), 0] = [0.0, 5e4, -3.0, 1e4]
    a[0, n - 1] = 0.0
    return f16(a)

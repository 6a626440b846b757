"""The whole-rollout kernel's whole-wave step body on ragged shards (k_rollout_geometric, launch form 2): the lanes past the last drone
fly a copy of drone n - 1 and store nothing.  37 x 7 = 259 drones (one full workgroup, then a wave of 3 drones and three empty waves)
and 1 x 1, 20 control steps from t0 = 0 and t0 = 1000, through the three destinations of the rows (rewritten in place every step, the
[T, n, 20] log, the last step's only):
  (a) rows and final state are bit-equal to the same drones flown inside a wave-aligned batch of 512 (no invalid lane anywhere);
  (b) the two rows allocated behind the last drone's, in the observation array and in the log, come back untouched;
  (c) launches of 7 steps and of 20 steps give the same bits.
One float64 and one compensated-fp32 case at n = 259 cover the other instantiations of the shared source.  The compensated dtype
carries all thirteen residuals in registers for the length of a launch and stores the three rate residuals at its end (csrc/mds_kernels.hip,
"Residual storage"), so there the length of a launch is part of the result by design: its 7-step flight is compared with the aligned batch
flown in 7-step launches, not with the 20-step launch."""
import numpy as np
import pytest

from tests import helpers as H
from tests.test_gpu_parity import make_env, mds  # noqa: F401  (mds: the module's fixture)

pytestmark = pytest.mark.gpu

N_BIG, STEPS, SENTINEL = 512, 20, 12345.0
SHAPES = {(37, 7): 259, (1, 1): 1}


def _drones():
    """259 drones of the config-3 generator with a yawing reference on every other env, flat; the batch of 512 repeats them."""
    xyz, rpy, P = H.c2_setup(37, 7, seed=5, phase="c3", yaw_rate=0.0)
    P[::2, :, 5] = 0.3
    rng = np.random.default_rng(9)
    rpy = rng.uniform(-0.2, 0.2, size=rpy.shape)
    return xyz.reshape(-1, 3), rpy.reshape(-1, 3), P.reshape(-1, 7)


def _bits(t):
    import torch
    t = t.contiguous()
    return t.view(torch.int64 if t.element_size() == 8 else torch.int32)


def _fly(mds, E, D, dtype, dest, t0, chunk):
    """-> (rows of the last step [n, 20], the log [STEPS, n, 20] or None, the 13 state planes + 3 origin planes [16, n], the sentinel rows)"""
    torch = mds.torch
    n = E * D
    xyz, rpy, P = _drones()
    idx = np.arange(n) % len(xyz)
    env = make_env(mds, E, D, xyz[idx].reshape(E, D, 3), rpy[idx].reshape(E, D, 3), dtype)
    env.set_trajectories(P[idx].reshape(E, D, 7))
    env.step(torch.zeros((E, D, 4), dtype=env.dtype))
    # the observation array and the log with two more rows behind the last drone's
    obs = torch.full((n + 2, 20), SENTINEL, dtype=env.dtype, device=env.device)
    # (rollout_geometric / rollout_geometric_fused write through env._obs.data_ptr(): BaseAviary's observation buffer, replaced here by a
    #  view of the larger one -- the one private attribute this test depends on)
    assert env._obs.shape == (E, D, 20) and env._obs.dtype == obs.dtype
    env._obs = obs[:n].view(E, D, 20)
    log = None
    if dest == "log":
        log = torch.full((STEPS * n + 2, 20), SENTINEL, dtype=env.dtype, device=env.device)
        t, dt = t0, env.CTRL_TIMESTEP
        for k in range(0, STEPS, chunk):
            ks = min(chunk, STEPS - k)
            env.rollout_geometric_fused(t, ks, log=True, log_out=log[k * n:(k + ks) * n].view(ks, E, D, 20))
            for _ in range(ks):
                t += dt
    else:
        env.set_rollout_form(2, chunk)
        env.rollout_geometric(t0, STEPS, obs_every_step=dest == "in_place")
        assert env.last_rollout_form() == 2
    torch.cuda.synchronize()
    sv = env.state_views()
    planes = torch.stack([p.clone().to(torch.float64) for p in sv["comp"] + sv["origin"]])      # (exact: widening only)
    tail = torch.cat([obs[n:], log[STEPS * n:]] if log is not None else [obs[n:]]).clone()
    out = obs[:n].clone(), (log[:STEPS * n].view(STEPS, n, 20).clone() if log is not None else None), planes, tail
    env.close()
    return out


_REF = {}


def _reference(mds, dtype, dest, t0, chunk=STEPS):
    """The wave-aligned batch of 512, flown once per (dtype, destination, t0, steps per launch) and shared."""
    key = (dtype, dest, t0, chunk)
    if key not in _REF:
        _REF[key] = _fly(mds, N_BIG, 1, dtype, dest, t0, chunk)
    return _REF[key]


def _check(mds, E, D, dtype, dest, t0, launch_invariant=True):
    torch = mds.torch
    n = E * D
    rows, log, planes, tail = _fly(mds, E, D, dtype, dest, t0, STEPS)
    rows7, log7, planes7, tail7 = _fly(mds, E, D, dtype, dest, t0, 7)
    rrows, rlog, rplanes, _ = _reference(mds, dtype, dest, t0)
    assert torch.isfinite(rows).all() and (rows[:, 16:] > 0).all()                          # rows were written
    # (a) the ragged shard against the same drones in the wave-aligned batch
    assert torch.equal(_bits(rows), _bits(rrows[:n]))
    assert torch.equal(_bits(planes), _bits(rplanes[:, :n]))
    if log is not None:
        assert torch.equal(_bits(log), _bits(rlog[:, :n]))
        assert torch.equal(_bits(log[-1]), _bits(rows))
    # (b) nothing behind the last drone's row
    assert (tail == SENTINEL).all() and (tail7 == SENTINEL).all()
    # (c) launches of 7 steps against one of 20 (the compensated dtype: against the aligned batch in launches of 7)
    if not launch_invariant:
        r7rows, r7log, r7planes, _ = _reference(mds, dtype, dest, t0, 7)
        rows, planes, log = r7rows[:n], r7planes[:, :n], (r7log[:, :n] if r7log is not None else None)
    assert torch.equal(_bits(rows7), _bits(rows)) and torch.equal(_bits(planes7), _bits(planes))
    if log is not None:
        assert torch.equal(_bits(log7), _bits(log))


@pytest.mark.parametrize("t0", [0.0, 1000.0])
@pytest.mark.parametrize("dest", ["in_place", "log", "last"])
@pytest.mark.parametrize("shape", sorted(SHAPES, reverse=True))
def test_ragged_shard_equals_wave_aligned_batch(mds, shape, dest, t0):  # noqa: F811
    _check(mds, *shape, "float32", dest, t0)


@pytest.mark.parametrize("dtype", ["float64", "float32c"])
def test_ragged_shard_other_instantiations(mds, dtype):  # noqa: F811
    _check(mds, 37, 7, dtype, "in_place", 0.0, launch_invariant=dtype != "float32c")

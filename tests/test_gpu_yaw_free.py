"""Yaw-free handles on the GPU: a handle whose Lemniscates were all uploaded with yaw_rate = 0 (mds_traj_yaw_free) steps through
k_step_geometric_y0 / k_rollout_geometric_y0, which do not form the controller's products with the desired yaw, the zero yaw rate
and the zero z components of the planar trajectory (csrc/mds_math.hpp).

Handle A runs as uploaded (flag 1); handle B flies the same drones on the general kernels (mds_set_traj_specialisation(h, 0)).

  * A == B: the state and every step's rows, for fp32, float64, compensated fp32, RK4 and fp16 storage, 259 drones (four waves and
    three lanes) and 1 drone, 60 steps (form 2: a 50-step and a 10-step launch).  From a perturbed, non-degenerate state the fp32
    results are the same bytes; from rest (identity attitude, the drone on its trajectory's height: exact zeros everywhere) they
    are == and may differ in the sign of a zero.
  * within A the launch forms agree as they do on B (fp32: to the byte), and a ragged shard equals the same drones inside a
    larger batch to the byte.
  * one drone with a yaw rate clears the flag and the handle then equals one with the specialisation off, byte for byte;
    uploading zeros again sets it again; segment tables clear it.
  * A tracks the NumPy oracle over the 60 steps within the gates the existing loops are held to against the same oracle
    (tests/test_gpu_trajectories.py / test_gpu_parity.py: 1e-9 in float64, 1e-5 in fp32 arithmetic, on the 16 state columns)."""
import numpy as np
import pytest

from tests import helpers as H

pytestmark = pytest.mark.gpu

STEPS = 60
N = 259                                   # four waves and three lanes


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


def setup(n):
    """One env of n drones (the generator of SURVEY 8d); the first drones of a larger n are the drones of a smaller one."""
    xyz, rpy, P = H.c2_setup(1, 320, phase="c3")
    return xyz[:, :n].copy(), rpy[:, :n].copy(), P[:, :n].copy()


def perturbed(state, seed=5):
    """A state away from every exact zero: offsets in position, attitude, velocity and body rate (drone i gets the same offsets whatever
    the size of the batch it flies in)."""
    rng = np.random.default_rng(seed)
    d = rng.uniform(-1.0, 1.0, (320, 13))
    s = np.array(state, dtype=np.float64).reshape(-1, 13)
    d = d[:s.shape[0]]
    s[:, 0:3] += 0.05 * d[:, 0:3]
    q = s[:, 3:7] + 0.08 * d[:, 3:7]
    s[:, 3:7] = q / np.linalg.norm(q, axis=1, keepdims=True)
    s[:, 7:10] = 0.3 * d[:, 7:10]
    s[:, 10:13] = 0.4 * d[:, 10:13]
    return s


def make(mds, n, dtype, integrator="euler", spec=True, P=None, perturb=True):
    xyz, rpy, P0 = setup(n)
    env = mds.CtrlAviary(drone_model=mds.DroneModel.CF2P, num_drones=n, initial_xyzs=xyz, initial_rpys=rpy, physics=mds.Physics.DYN,
                         pyb_freq=100, ctrl_freq=100, num_envs=1, dtype=dtype, integrator=integrator)
    env.set_trajectories(P0 if P is None else P)
    env.set_traj_specialisation(spec)
    env.step(mds.torch.zeros((1, n, 4), dtype=env.dtype, device=env.device))
    if perturb:
        env.set_state(perturbed(env.get_state()))
    return env


def raw(t):
    """The tensor's bytes (fp16 rows included) as a uint8 array, and its values in float64."""
    c = t.detach().contiguous().cpu()
    return c.view(c.shape[0], -1).numpy().view(np.uint8).copy(), c.double().numpy().copy()


def fly(mds, n, dtype, integrator="euler", spec=True, form=2, P=None, perturb=True, log=False):
    """STEPS steps on a fresh handle: (bytes, values) of the rows -- every step's with log=True (the whole-rollout kernel's log form, one
    launch), else the last step's through mds_rollout_geometric in the given launch form (form 2: 50 + 10 steps, rows rewritten in place
    every step) -- and the state."""
    env = make(mds, n, dtype, integrator, spec, P, perturb)
    assert env.traj_yaw_free() == (P is None or not np.any(P[..., 5]))
    if log:
        _, rows = env.rollout_geometric_fused(0.0, STEPS, log=True)
        rows = rows.reshape(STEPS, -1)
    else:
        env.set_rollout_form(form, 50)
        rows = env.rollout_geometric(0.0, STEPS, obs_every_step=True).reshape(1, -1)
        assert env.last_rollout_form() == form
    out = raw(rows) + (env.get_state(),)
    env.close()
    return out


CASES = [("float32", "euler"), ("float64", "euler"), ("float32c", "euler"), ("float32", "rk4"), ("float16", "euler")]


@pytest.mark.parametrize("n", [N, 1])
@pytest.mark.parametrize("dtype,integrator", CASES)
def test_yaw_free_handle_equals_the_general_kernels(mds, dtype, integrator, n):
    for perturb in (True, False):
        for kw in (dict(log=True), dict(form=2), dict(form=1)):
            if dtype == "float16" and kw.get("log"):
                continue                          # (an odd number of fp16 rows: the log's slots would not be 16-byte aligned, MDS_EALIGN;
                                                  # test_fp16_storage_every_steps_rows_at_an_aligned_drone_count has the log form)
            ba, va, sa = fly(mds, n, dtype, integrator, True, perturb=perturb, **kw)
            bb, vb, sb = fly(mds, n, dtype, integrator, False, perturb=perturb, **kw)
            assert np.isfinite(va).all()
            assert (va == vb).all(), (dtype, integrator, n, perturb, kw, np.argwhere(va != vb)[:5])
            assert (sa == sb).all(), (dtype, integrator, n, perturb, kw)
            same = np.array_equal(ba, bb)
            print(f"{dtype} {integrator} n={n} perturbed={perturb} {kw}: rows byte-equal = {same}")
            if dtype == "float32" and integrator == "euler" and perturb:
                assert same, (n, kw)
                assert sa.tobytes() == sb.tobytes()


def test_fp16_storage_every_steps_rows_at_an_aligned_drone_count(mds):
    """The log form for fp16 storage: 264 drones (four waves and eight lanes; 264 x 20 fp16 rows are a multiple of 16 bytes, which 259 and
    1 are not), every step's rows and the state of handle A == handle B's."""
    for perturb in (True, False):
        ba, va, sa = fly(mds, 264, "float16", "euler", True, perturb=perturb, log=True)
        bb, vb, sb = fly(mds, 264, "float16", "euler", False, perturb=perturb, log=True)
        assert va.shape[0] == STEPS and np.isfinite(va).all()
        assert (va == vb).all(), (perturb, np.argwhere(va != vb)[:5])
        assert (sa == sb).all(), perturb
        print(f"float16 n=264 perturbed={perturb} log: rows byte-equal = {np.array_equal(ba, bb)}")


@pytest.mark.parametrize("dtype,integrator,tol", [("float32", "euler", 1e-5), ("float64", "euler", 1e-9), ("float32c", "euler", 1e-5),
                                                  ("float32", "rk4", 1e-5)])
def test_yaw_free_launch_forms_agree(mds, dtype, integrator, tol):
    """Form 1 against form 2 on handle A: fp32 to the byte (what test_c3_full_size_properties sees between a form-1 and a form-2 shard
    of the general kernels); the other arithmetic within the gate test_rollout_launch_form_policy_and_equivalence holds the general
    kernels' two forms to."""
    b2, v2, s2 = fly(mds, N, dtype, integrator, True, form=2)
    b1, v1, s1 = fly(mds, N, dtype, integrator, True, form=1)
    print(f"{dtype} {integrator}: forms byte-equal = {np.array_equal(b1, b2)}, max |difference| = {np.abs(v1 - v2).max():.3e}")
    if dtype == "float32" and integrator == "euler":
        assert np.array_equal(b1, b2) and s1.tobytes() == s2.tobytes()
    r1, r2 = v1.reshape(-1, 20), v2.reshape(-1, 20)
    np.testing.assert_allclose(r1[:, :16], r2[:, :16], atol=tol)
    np.testing.assert_allclose(r1[:, 16:], r2[:, 16:], rtol=max(tol, 1e-9))
    # the log form (one launch of 60 steps, non-temporal stores) leaves the rows of the in-place form (50 + 10 steps): bit for bit, but
    # for compensated storage, whose rate residuals are rounded to storage between the launches of the in-place form
    bl, vl, sl = fly(mds, N, dtype, integrator, True, log=True)
    if dtype != "float32c":
        assert np.array_equal(bl[-1], b2[0]) and sl.tobytes() == s2.tobytes()
    np.testing.assert_allclose(vl[-1].reshape(-1, 20)[:, :16], r2[:, :16], atol=tol)


@pytest.mark.parametrize("form", [1, 2])
def test_ragged_shard_equals_the_same_drones_inside_a_larger_batch(mds, form):
    b, v, s = fly(mds, N, "float32", form=form)
    B, V, S = fly(mds, 320, "float32", form=form)
    assert np.array_equal(b.reshape(N, -1), B.reshape(320, -1)[:N])
    assert s.reshape(N, 13).tobytes() == S.reshape(320, 13)[:N].tobytes()


def test_flag_follows_the_upload(mds):
    xyz, rpy, P = setup(N)
    Py = P.copy()
    Py[0, 17, 5] = 0.1                                  # ONE drone with a yaw rate
    env = make(mds, N, "float32", P=Py)
    assert not env.traj_yaw_free()
    env.set_rollout_form(2, 50)
    a = raw(env.rollout_geometric(0.0, STEPS, obs_every_step=True).reshape(1, -1))[0]
    bb, vb, _ = fly(mds, N, "float32", spec=False, form=2, P=Py)
    assert np.array_equal(a, bb)                        # the general kernels, specialisation on or off
    assert np.abs(vb.reshape(N, 20)[17, 7:10]).max() > 1e-3          # (the drone does yaw)
    # zeros again (minus zero is a zero): the flag is set again and the handle flies as a fresh yaw-free one does
    P0 = P.copy()
    P0[0, ::2, 5] = -0.0
    env.set_trajectories(P0)
    assert env.traj_yaw_free()
    env.set_state(perturbed(make_state0(mds)))
    c = raw(env.rollout_geometric(0.0, STEPS, obs_every_step=True).reshape(1, -1))[0]
    ba, _, _ = fly(mds, N, "float32", form=2)
    assert np.array_equal(c, ba)
    # segment tables clear it
    from multidronesim_amd import trajectories as TR
    env.set_trajectories([TR.CircleTrajectory(r=0.3, v=0.5, center=np.array([0.0, 0.0, 0.5])) for _ in range(N)])
    assert not env.traj_yaw_free()
    assert np.isfinite(env.rollout_geometric(0.0, 5).double().cpu().numpy()).all()
    env.close()


def make_state0(mds):
    """The state every handle of `make` has after its first (zero-action) step, before the perturbation."""
    env = make(mds, N, "float32", perturb=False)
    s = env.get_state()
    env.close()
    return s


@pytest.mark.parametrize("dtype,integrator,tol", [("float32", "euler", 1e-5), ("float64", "euler", 1e-9), ("float32c", "euler", 1e-5),
                                                  ("float32", "rk4", 1e-5)])
def test_yaw_free_handle_tracks_the_oracle(mds, dtype, integrator, tol):
    xyz, rpy, P = setup(N)
    oobs, _ = H.oracle_closed_loop(xyz, rpy, P, STEPS, integrator=integrator)
    for form in (1, 2):
        _, v, _ = fly(mds, N, dtype, integrator, True, form=form, perturb=False)
        err = np.abs(v.reshape(N, 20)[:, :16] - oobs[:, :16]).max()
        print(f"{dtype} {integrator} form {form}: max |state - oracle| after {STEPS} steps = {err:.3e} (gate {tol:g})")
        assert err < tol

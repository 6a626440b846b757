"""The DSLPID operator on the GPU (k_dslpid through mds_dslpid_compute / BaseAviary.dslpid_compute), open loop, every call's RPM row
against the float64 oracle on the case set of tests/dslpid_cases.py (333 drones = one full 256-batch and a ragged 77, 24 calls; the
groups, the clamps they reach and the conditioning are asserted on the oracle alone in tests/test_dslpid_cpu.py), then the properties
that tie the operator to the rest: it is the fused step's controller bit for bit, its memory is real and is reset by both resets,
and a ragged shard computes what an aligned one does.

Gates (tests/dslpid_cases.py ``gate``; derivation and the host build's errors in tests/test_dslpid_cpu.py): float64 1e-10 relative per
RPM value; float32 4 x S + 8 x 2^-24 with S the float64 oracle's own sensitivity to float32 storage of the Euler angles, the memory
and dt.  Measured on an MI355X (largest relative RPM error over both mixers):

    configuration           S          float32 gate   float32 device error   float64 device error
    240 Hz, halved gains    7.07e-06   2.88e-05       1.18e-05              2.5e-14
    10 Hz,  halved gains    2.97e-07   1.66e-06       7.57e-07              2.4e-15
    240 Hz, probe gains     6.03e-08   7.18e-07       2.85e-07              6.7e-16
    10 Hz,  probe gains     5.50e-09   4.99e-07       2.61e-07              6.7e-16
    240 Hz, skew gains      7.47e-06   3.04e-05       1.33e-05              2.9e-14
    10 Hz,  skew gains      3.21e-07   1.76e-06       7.13e-07              2.4e-15
"""
import types

import numpy as np
import pytest

from tests import dslpid_cases as DC

pytestmark = pytest.mark.gpu

E, D = 37, 9            # 333 drones


def make_env(model, ctrl_freq, gains, dtype, envs=E, drones=D):
    from multidronesim_amd.envs.CtrlAviary import CtrlAviary, DroneModel, Physics
    env = CtrlAviary(drone_model=DroneModel(model), num_drones=drones, physics=Physics.DYN, pyb_freq=ctrl_freq, ctrl_freq=ctrl_freq,
                     num_envs=envs, dtype=dtype)
    env.set_dslpid_gains(types.SimpleNamespace(P_COEFF_FOR=gains["P_FOR"], I_COEFF_FOR=gains["I_FOR"], D_COEFF_FOR=gains["D_FOR"],
                                               P_COEFF_TOR=gains["P_TOR"], I_COEFF_TOR=gains["I_TOR"], D_COEFF_TOR=gains["D_TOR"]))
    return env


def on_device(env, ctrl_freq, drones=slice(None)):
    """The case set as tensors of the env's dtype: obs [K,E,D,20], target_pos [K,E,D,3], target_rpy [E,D,3]."""
    import torch
    obs, tp, tr, _ = DC.make_cases(ctrl_freq=ctrl_freq)
    put = lambda a, lead: torch.as_tensor(np.array(a), dtype=env.dtype).to(env.device).reshape(*lead, env.NUM_ENVS, env.NUM_DRONES, a.shape[-1])
    return put(obs[:, drones], (obs.shape[0],)), put(tp[:, drones], (tp.shape[0],)), put(tr[drones], ())


def run_calls(env, dev, calls=range(DC.N_CALLS)):
    """rpm [len(calls), n, 4] (float64 on the host) of the calls given, in order, on the env's memory as it stands."""
    import torch
    obs, tp, tr = dev
    out = torch.stack([env.dslpid_compute(obs[k], tp[k], tr) for k in calls])
    return out.double().cpu().numpy().reshape(len(calls), env.n, 4)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("gains_name", list(DC.GAINS))
@pytest.mark.parametrize("ctrl_freq", DC.RATES)
@pytest.mark.parametrize("model", ["cf2p", "cf2x"])
def test_operator_matches_the_oracle_call_by_call(model, ctrl_freq, gains_name, dtype):
    env = make_env(model, ctrl_freq, DC.GAINS[gains_name], dtype)
    got = run_calls(env, on_device(env, ctrl_freq))
    env.close()
    ref, gate = DC.reference(model, ctrl_freq, gains_name, dtype), DC.gate(ctrl_freq, gains_name, dtype)
    assert got.shape == ref.shape == (24, 333, 4) and np.isfinite(got).all()
    err = np.abs(got / ref - 1)
    grp = np.arange(333) % DC.N_GROUPS
    print("%s %3d Hz %-6s %s: largest relative RPM error on the device %.3e (gate %.3e; float32 storage sensitivity %.3e), per group %s" % (
        model, ctrl_freq, gains_name, dtype, err.max(), gate, DC.storage_sensitivity(ctrl_freq, gains_name),
        ["%.1e" % err[:, grp == k].max() for k in range(8)]))
    assert err.max() <= gate


def test_operator_on_a_single_drone_float64():
    """1 x 1: drone 12 of the set (group 4, the sustained attitude error) alone on a handle, CF2X, 10 Hz, probe gains."""
    env = make_env("cf2x", 10, DC.GAINS["probe"], "float64", 1, 1)
    got = run_calls(env, on_device(env, 10, slice(12, 13)))
    env.close()
    err = np.abs(got / DC.reference("cf2x", 10, "probe", "float64")[:, 12:13] - 1)
    print("1 x 1 float64: largest relative RPM error %.3e" % err.max())
    assert err.max() <= DC.gate(10, "probe", "float64")


def _twin_flight(a, b, xyz, c=None, c_shift=None, steps=30, after=10):
    """a flies ``steps`` + ``after`` fused steps (a target jump between them); b gets each observation a's controller saw and the same
    targets through dslpid_compute.  -> actions of a, of b (and of c, fed the observations shifted by -c_shift), [steps+after, n, 4]."""
    import torch
    tgt = xyz + np.array([0, 0, 1.0])
    trpy = np.zeros_like(xyz)
    trpy[..., 2] = np.random.default_rng(3).uniform(-1, 1, size=xyz.shape[:2])
    acts = [[], [], []]
    for k in range(steps + after):
        if k == steps:
            tgt = tgt + np.array([0.4, -0.3, 0.2])
        prev = a._computeObs().clone()
        acts[0].append(a.step_dslpid(tgt, trpy, return_action=True)[1].clone())
        acts[1].append(b.dslpid_compute(prev, tgt, trpy))
        if c is not None:
            prev[..., 0:3] -= c_shift
            acts[2].append(c.dslpid_compute(prev, tgt, trpy))
    torch.cuda.synchronize()
    return [torch.stack(x).double().cpu().numpy().reshape(len(x), -1, 4) for x in acts if x]


@pytest.mark.parametrize("dtype_a,dtype_b", [("float64", "float64"), ("float32", "float32"), ("float32c", "float32")])
def test_operator_is_the_fused_steps_controller_bit_for_bit(dtype_a, dtype_b):
    """240 Hz, halved gains, the hover scene of test_gpu_pidenv._pid_env, zero origin.  float32c carries residuals in the step alone:
    its controller is the float32 one."""
    from tests.test_gpu_pidenv import _pid_env
    a, xyz = _pid_env(E, D, dtype_a)
    b, _ = _pid_env(E, D, dtype_b)
    act_a, act_b = _twin_flight(a, b, xyz)
    a.close()
    b.close()
    assert np.isfinite(act_a).all() and np.ptp(act_a, axis=0).max() > 100          # a flight, not a constant
    np.testing.assert_array_equal(act_a, act_b)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_fused_step_forms_the_error_about_its_origin(dtype):
    """After mds_set_origin the state path forms (target - origin) - p_local; the operator sees world positions.  The two agree within
    the operator's gate, and would not if the state path left the origin out (c: the same observations less the origin)."""
    import torch
    from multidronesim_amd import _capi as capi
    from tests.test_gpu_pidenv import _pid_env
    a, xyz = _pid_env(E, D, dtype)
    b, _ = _pid_env(E, D, dtype)
    c, _ = _pid_env(E, D, dtype)
    org = np.ascontiguousarray(np.random.default_rng(5).uniform(0.1, 0.4, size=(a.n, 3)) * np.array([1.0, -1.0, 1.0]))
    capi.check(a._lib.mds_set_origin(a._h, capi.as_double_ptr(org), a._stream()), "mds_set_origin")
    held = torch.stack(a.state_views()["origin"]).double().cpu().numpy().T
    np.testing.assert_allclose(held, org, rtol=1e-7)
    assert np.abs(held).min() >= 0.1                                              # the origin really differs from b's and c's zero
    shift = torch.as_tensor(org.reshape(E, D, 3), dtype=a.dtype).to(a.device)
    act_a, act_b, act_c = _twin_flight(a, b, xyz, c, shift)
    for e in (a, b, c):
        e.close()
    gate = DC.gate(240, "halved", dtype)
    err, err_ignored = np.abs(act_b / act_a - 1).max(), np.abs(act_c / act_a - 1).max()
    print("%s: state path against operator %.3e (gate %.3e); with the origin left out %.3e" % (dtype, err, gate, err_ignored))
    assert err <= gate
    assert err_ignored > 100 * gate


def _reset_pid(env):
    from multidronesim_amd import _capi as capi
    capi.check(env._lib.mds_dslpid_reset(env._h, env._stream()), "mds_dslpid_reset")


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_memory_is_real_and_both_resets_clear_it(dtype):
    env = make_env("cf2p", 10, DC.GAINS["probe"], dtype)
    dev = on_device(env, 10)
    first = run_calls(env, dev)
    again = run_calls(env, dev)                       # no reset: the integrals and last_rpy of call 23 are carried into call 0
    assert (again != first).any(axis=-1).mean() > 0.5
    _reset_pid(env)
    np.testing.assert_array_equal(run_calls(env, dev), first)
    env.reset()
    np.testing.assert_array_equal(run_calls(env, dev), first)
    # calls 12..23 on a handle that ran calls 0..11
    other = make_env("cf2p", 10, DC.GAINS["probe"], dtype)
    head = run_calls(other, dev, range(12))
    tail = run_calls(other, dev, range(12, 24))
    np.testing.assert_array_equal(np.concatenate([head, tail]), first)
    _reset_pid(other)
    assert (run_calls(other, dev, range(12, 24)) != first[12:]).any(axis=-1).mean() > 0.5   # the tail depends on the head
    env.close()
    other.close()


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_ragged_shard_equals_aligned_shard(dtype):
    """The first 256 drones of the 333-drone run against a 256-drone handle (one full batch, no tail)."""
    ragged = make_env("cf2x", 240, DC.GAINS["halved"], dtype)
    aligned = make_env("cf2x", 240, DC.GAINS["halved"], dtype, 32, 8)
    r = run_calls(ragged, on_device(ragged, 240))
    a = run_calls(aligned, on_device(aligned, 240, slice(0, 256)))
    ragged.close()
    aligned.close()
    np.testing.assert_array_equal(r[:, :256], a)

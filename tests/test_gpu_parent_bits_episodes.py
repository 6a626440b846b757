"""The three rollout-episode kernels (k_rollout_episodes, k_rollout_episodes_safe, k_rollout_episodes_policy) against a libmds.so built
from the parent commit: bit for bit.  Their source shares the lane map and the counters' type (csrc/mds_episode_kernels.hip EpisodeLane,
csrc/mds_episode.hpp EpisodeTally) and their entry points share one host helper; any further piece moved into a shared function reorders
their assembly, and this is the test such a change has to pass.  tests/test_gpu_parent_bits.py says how the parent's library is named
(MDS_PARENT_LIB) and flown.

Shapes (E, D) = (90, 3): a workgroup owns 84 envs, so two workgroups, a ragged second one, idle tail lanes and three envs per wave boundary;
and (17, 16): 16 envs per workgroup, two workgroups, no idle lane in the first.  Both have an even drone count, as the fp16 rows need.
Every flight is two calls of 6 control steps at 4 steps per launch (launches of 4, 2, 4, 2 steps: launch boundaries inside a call), with
max_steps = 4 and one height bound, z_max: every drone climbs under about 1.25 times the hover RPM, and the homes of the envs lie 0.8 mm,
2.2 mm and (two envs of every four) 1 m below the bound, so the first two kinds terminate, at differing steps, and the others run into the
truncation -- on step 4, the last of the first launch.  check_scenario asserts that on the flags of every flight.
Flights: the action table plain, with the collision causes (one sphere above a drone of env 2, which ends that env's episodes by bit 7),
with randomised starts, with both; the policy with both run-time flags off and both on, 32 and 64 wide; each under DYN and PYB_DRAG,
with Euler in float32 and float64 and with RK4 in float64, the table flights also with fp16 storage.
Compared: every log ring (observation, action, reward, flags) and the rows each call returns, the final state and the last-RPM planes,
the five counters and, where the collision causes are on, the two h_min arrays."""
import numpy as np
import pytest

from oracle import np_oracle as O
from tests import episode_policy_cases as PC
from tests import helpers as H
from tests.test_gpu_parity import mds  # noqa: F401  (mds: the module's fixture)

pytestmark = pytest.mark.gpu

SHAPES = ((90, 3), (17, 16))
CALLS, STEPS, SPL, MAX_STEPS, N_SETS = 2, 6, 4, 4, 5
LAUNCHES = ((0, 4), (4, 6), (6, 10), (10, 12))          # the steps of each launch
Z_MAX, GAPS = 2.0, (0.0008, 0.0022, 1.0, 1.0)           # env e starts GAPS[e % 4] below the bound
RPM_FACTOR = 1.25
SAFETY_RADIUS, OBSTACLE_RADIUS = 0.05, 0.05
TABLE = {"plain": (False, False), "safe": (True, False), "random": (False, True), "safe_random": (True, True)}
POLICY = {"policy_off": (False, False), "policy_on": (True, True)}
# (dtype, integrator)
PRECISIONS = (("float32", "euler"), ("float64", "euler"), ("float64", "rk4"), ("float16", "euler"))


def scene(E, D):
    rng = np.random.default_rng([3, E, D])
    xyz = np.zeros((E, D, 3))
    xyz[..., 0] = 0.3 * np.arange(D)[None, :]
    xyz[..., 1] = 0.5 * np.arange(E)[:, None]
    xyz[..., 2] = Z_MAX - np.array(GAPS)[np.arange(E) % 4][:, None]
    rpy = rng.uniform(-0.05, 0.05, size=(E, D, 3))
    actions = O.CF2P.HOVER_RPM * RPM_FACTOR * (1.0 + 0.02 * rng.standard_normal((N_SETS, E, D, 4)))
    target = xyz + rng.uniform(-0.3, 0.3, size=xyz.shape)
    # a sphere whose safety set begins 2.5 mm above drone 0 of env 2 (zscale 1: the set is |ez| < safety_radius + radius on the axis)
    obstacle = np.array([[xyz[2, 0, 0], xyz[2, 0, 1], xyz[2, 0, 2] + SAFETY_RADIUS + OBSTACLE_RADIUS + 0.0025, OBSTACLE_RADIUS]])
    return xyz, rpy, actions, target, obstacle


def _host(t):
    return t.detach().cpu().numpy().copy()


def fly_one(mds, E, D, dtype, integrator, physics, kind, width=None):  # noqa: F811
    """{name: array} of one flight"""
    torch = mds.torch
    xyz, rpy, actions, target, obstacle = scene(E, D)
    env = mds.CtrlAviary(drone_model=mds.DroneModel.CF2P, num_drones=D, initial_xyzs=xyz, initial_rpys=rpy, physics=getattr(mds.Physics, physics),
                         pyb_freq=200, ctrl_freq=100, num_envs=E, dtype=dtype, integrator=integrator, track_last_rpm=True)
    env.set_episodes(max_steps=MAX_STEPS, z_max=Z_MAX, term_penalty=1.5, target=target)
    safe, rand = {**TABLE, **POLICY}[kind]
    if safe:
        env.set_episode_safety(SAFETY_RADIUS, 1.0, obstacle)
    if rand:
        env.set_episode_randomisation(21, pos=0.0002, rpy=0.05, vel=0.01, rate=0.2)
    if width is not None:
        env.set_episode_policy(PC.weights(2, width), 2, width, "tanh", rpm_base=RPM_FACTOR * env.HOVER_RPM, rpm_scale=0.05 * env.HOVER_RPM)
    acts = torch.as_tensor(actions, device=env.device).to(env.dtype).contiguous()
    T = CALLS * STEPS
    rdt = torch.float64 if env.dtype == torch.float64 else torch.float32
    obs_log = torch.zeros((T, E, D, 20), dtype=env.dtype, device=env.device)
    act_log = torch.zeros((T, E, D, 4), dtype=env.dtype, device=env.device)
    reward_log = torch.zeros((T, E), dtype=rdt, device=env.device)
    flags_log = torch.full((T, E), -1, dtype=torch.int32, device=env.device)
    out = {}
    for call in range(CALLS):
        if width is None:
            now = env.rollout_episodes(acts, call * STEPS, STEPS, obs_log, reward_log, flags_log, steps_per_launch=SPL)
        else:
            now = env.rollout_episodes_policy(call * STEPS, STEPS, obs_log, act_log, reward_log, flags_log, steps_per_launch=SPL)
        out["now%d" % call] = _host(now)
    out.update(obs=_host(obs_log), reward=_host(reward_log), flags=_host(flags_log))
    if width is not None:
        out["action"] = _host(act_log)
    out.update({"counter_" + k: _host(v) for k, v in env.episode_counters().items()})
    if safe:
        out.update({k: _host(v) for k, v in env.episode_safety().items()})
    out["state"] = np.asarray(env.get_state()).reshape(-1, 13)
    out["last_rpm"] = _host(env._computeObs()).reshape(-1, 20)[:, 16:]
    env.close()
    return out


def fly_all(mds):  # noqa: F811
    out = {}
    for E, D in SHAPES:
        for physics in ("DYN", "PYB_DRAG"):
            for dtype, integrator in PRECISIONS:
                cases = [(kind, None) for kind in TABLE]
                if dtype != "float16":
                    cases += [(kind, width) for kind in POLICY for width in (32, 64)]
                for kind, width in cases:
                    tag = "%dx%d_%s_%s_%s_%s%s" % (E, D, physics, dtype, integrator, kind, "" if width is None else "_w%d" % width)
                    out.update({tag + "." + k: v for k, v in fly_one(mds, E, D, dtype, integrator, physics, kind, width).items()})
    return out


def check_scenario(flights):
    """on every flight's flags: an env terminates, one truncates, one is not done within some launch, a done falls on the last step of a launch,
    the terminating envs do not all terminate first on the same step, and some env never terminates"""
    names = [k for k in flights if k.endswith(".flags")]
    assert len(names) == len(SHAPES) * 2 * (len(PRECISIONS) * len(TABLE) + (len(PRECISIONS) - 1) * len(POLICY) * 2)
    for k in names:
        flags = np.asarray(flights[k])
        term, trunc = (flags & 1) != 0, (flags & 2) != 0
        done = term | trunc
        assert term.any() and trunc.any(), k
        assert any((~done[a:b].any(axis=0)).any() for a, b in LAUNCHES), k
        assert done[[b - 1 for _, b in LAUNCHES]].any(), k
        first = np.where(term.any(axis=0), term.argmax(axis=0), -1)
        assert (first == -1).any() and len(set(first[first >= 0])) >= 2, (k, sorted(set(first)))
        if "_safe" in k or "policy_on" in k:
            assert ((flags >> 15) & 1).any(), k                  # (the sphere's bit)


@pytest.fixture(scope="module")
def flights(mds):  # noqa: F811
    return fly_all(mds)


def test_every_episode_flight_flew_and_meets_the_scenario(flights):
    for k, v in flights.items():
        assert v.size > 0, k
        if not k.endswith(("h_min_step", "h_min_episode")):       # (+inf there: an env with nothing tested, or just restarted)
            assert np.isfinite(v.astype(np.float64)).all(), k
    check_scenario(flights)


def test_logs_rows_state_counters_and_h_min_are_the_parent_librarys_bit_for_bit(flights, tmp_path):
    ref = H.parent_library_flights("tests.test_gpu_parent_bits_episodes", "fly_all", tmp_path)
    check_scenario(ref)
    H.assert_same_bits(ref, flights)

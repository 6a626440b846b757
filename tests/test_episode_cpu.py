"""Per-env episodes without a GPU: the scenarios' own conditions on the float64 oracle, the rule header (csrc/mds_episode.hpp) compiled
with g++ under AddressSanitizer + UBSan and run over the oracle's rows, and the argument checks of the new entry points."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from multidronesim_amd import _capi as capi
from tests import episode_cases as EC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEAR = 1e-4            # a decision with a smaller margin may go the other way in a lower precision


@pytest.mark.parametrize("E,D", EC.SHAPES)
def test_scenarios_exercise_every_cause_and_stay_clear_of_the_thresholds(E, D):
    """Conditions on the test inputs, on the oracle alone: every cause bit and truncation ends at least 20 episodes in its own sub-scenario,
    and in no scenario do more than 10 % of the envs ever come within 1e-4 (relative) of a threshold.  A seed or threshold that fails this
    is changed in tests/episode_cases.py; the caps stay."""
    for name in EC.RULES:
        r = EC.oracle_run(E, D, name)
        flags = r["flags"]
        if name in EC.CAUSE_BIT:
            ended = int(((flags >> (8 + EC.CAUSE_BIT[name])) & 1).sum())
            assert ended >= 20, (name, ended)
            assert ((flags >> 8) & ~(1 << EC.CAUSE_BIT[name]) == 0).all(), name                                       # that cause alone
        if name == "trunc":
            assert int(((flags & 2) != 0).sum()) >= 20 and ((flags & ~2) == 0).all()
        near = int((r["margin"] < NEAR).any(axis=0).sum())
        assert near <= 0.10 * E, (name, near, E)
    comb = EC.oracle_run(E, D, "combined")["flags"]
    assert int(((comb & 3) != 0).sum()) >= 20


@pytest.fixture(scope="module")
def rule_program(tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build the rule header's stand-alone program"
    exe = str(tmp_path_factory.mktemp("episode_rule") / "episode_rule_main")
    # the sanitizer runtimes linked statically: the program needs nothing preloaded and is indifferent to what the environment preloads
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan",
                           "-static-libubsan", "-o", exe, os.path.join(ROOT, "tests", "episode_rule_main.cpp")])
    return exe


def run_rule(exe, tmp_path, E, D, name, prec):
    xyz, rpy, actions, params = EC.scenario(E, D, name)
    r = EC.oracle_run(E, D, name)
    T = r["flags"].shape[0]
    p = {**EC.EpisodeOracle(xyz, rpy, D, params).params}
    home = np.broadcast_to(xyz.reshape(1, -1, 3), (T, E * D, 3))
    rows = np.concatenate([r["state"], home, home], axis=-1)                     # (the default target is the reset position)
    head = [T * E, D] + [p[k] for k in ("max_steps", "z_min", "z_max", "max_dist", "max_tilt", "max_speed", "max_rate", "reward_r0", "term_penalty")]
    fin, fout = str(tmp_path / f"{name}.in"), str(tmp_path / f"{name}_{prec}.out")
    np.concatenate([np.array(head, dtype=np.float64), rows.reshape(-1), r["length"].astype(np.float64).reshape(-1)]).tofile(fin)
    done = subprocess.run([exe, fin, fout, prec], capture_output=True, text=True)
    assert done.returncode == 0, (done.returncode, done.stderr[-2000:])
    out = np.fromfile(fout, dtype=np.float64)
    M = T * E
    return r, out[:M].astype(np.int64).reshape(T, E), out[M:2 * M].reshape(T, E), out[2 * M:].astype(np.int64).reshape(T, E * D)


@pytest.mark.parametrize("E,D", [(130, 1), (37, 7)])
def test_rule_header_matches_the_oracle(rule_program, tmp_path, E, D):
    """mds_episode.hpp on the host (g++, ASan + UBSan, a program of its own) over the states the oracle stepped through: in float64 flags,
    cause bits and reward equal the oracle's on every row; in float32 (state, home and thresholds rounded) the flags equal wherever the
    oracle's margin is at least 1e-4."""
    compared = 0
    for name in EC.RULES:
        r, flags, reward, cause = run_rule(rule_program, tmp_path, E, D, name, "f64")
        np.testing.assert_array_equal(flags, r["flags"], err_msg=name)
        np.testing.assert_array_equal(cause, r["cause"], err_msg=name)
        np.testing.assert_allclose(reward, r["reward"], rtol=1e-12, atol=1e-12, err_msg=name)
        r, flags32, reward32, _ = run_rule(rule_program, tmp_path, E, D, name, "f32")
        clear = r["margin"] >= NEAR
        np.testing.assert_array_equal(flags32[clear], r["flags"][clear], err_msg=name)
        np.testing.assert_allclose(reward32[clear], r["reward"][clear], rtol=1e-5, atol=1e-5 * D, err_msg=name)
        compared += int((r["flags"][clear] & 3 != 0).sum())
    assert compared >= 20 * len(EC.RULES)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return capi.load_library()


def test_default_episode_params_and_struct_layout(lib):
    assert C.sizeof(capi.MdsEpisodeParams) == 2 * 4 + 8 * 8
    assert lib.mds_default_episode_params(None) == -1
    p = capi.MdsEpisodeParams()
    assert lib.mds_default_episode_params(C.byref(p)) == 0
    assert p.max_steps == 0 and p.reward_r0 == 2.0 and p.term_penalty == 0.0
    assert p.z_min == -np.inf and all(getattr(p, k) == np.inf for k in ("z_max", "max_dist", "max_tilt", "max_speed", "max_rate"))


def test_episode_entry_points_validate_before_touching_the_device(lib):
    """null handle -> MDS_EINVAL from every new entry point, with no device present"""
    p = capi.MdsEpisodeParams()
    lib.mds_default_episode_params(C.byref(p))
    buf = C.create_string_buffer(64)
    ptrs = (C.c_void_p * 5)()
    assert lib.mds_set_episodes(None, C.byref(p), None, None) == -1
    assert lib.mds_set_episodes(None, None, None, None) == -1
    assert lib.mds_episode_ptrs(None, ptrs) == -1
    assert lib.mds_step_episodes(None, buf, buf, None, buf, buf, None) == -1
    assert lib.mds_rollout_episodes(None, buf, 1, 0, 1, None, 0, None, None, 1, None, None) == -1
    assert b"mds_rollout_episodes" in lib.mds_last_error()

"""Per-env episodes without a GPU: the scenarios' own conditions on the float64 oracle, the rule header (csrc/mds_episode.hpp) compiled
with g++ under AddressSanitizer + UBSan and run over the oracle's rows, and the argument checks of the new entry points."""
import ctypes as C
import os
import shutil
import subprocess
import types

import numpy as np
import pytest

from multidronesim_amd import _capi as capi
from tests import episode_cases as EC
from tests import episode_oracle as EO

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


TALLY_K, TALLY_E, TALLY_PENALTY = 12, 8, 0.3          # (0.3: not a float32 number, so the f32 replay has a rounded penalty to match)


def tally_inputs():
    """cause words and term sums [K, E] of the counter test, one column per situation (steps counted from 0):
       0  never a cause: length runs on, or truncates every max_steps steps
       1  a cause on step 2 and again on step 5: with max_steps 3 each falls on the step that would also truncate
       2  causes on steps 4 and 5: two terminations in a row
       3  a cause on step 3: with max_steps 3 a truncation and a termination in a row
       4  a NaN term sum on step 1, a cause on step 7: the NaN reaches ret, then sum_return
       5  a NaN term sum on the terminating step 6: NaN less the penalty
       6  several cause bits at once on steps 0 and 9 (bits 0 and 5, bits 6 and 7)
       7  never a cause, other sums"""
    K, E = TALLY_K, TALLY_E
    cause = np.zeros((K, E), dtype=np.int64)
    cause[[2, 5], 1] = 4
    cause[[4, 5], 2] = 2
    cause[3, 3] = 16
    cause[7, 4] = 8
    cause[6, 5] = 2
    cause[0, 6], cause[9, 6] = 0x21, 0xC0
    sums = np.random.default_rng(11).uniform(0.0, 6.0, size=(K, E))
    sums[1, 4] = sums[6, 5] = np.nan
    return cause, sums


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("max_steps", [0, 1, 3])
def test_env_step_carries_the_counters_like_the_oracle(rule_program, tmp_path, max_steps, prec):
    """mds_episode.hpp episode_env_step on the host (g++, ASan + UBSan, a program of its own) carrying an EpisodeTally over 12 steps of 8
    envs from zeroed counters, against tests/episode_oracle.py tally_step -- the EpisodeOracle's own counter lines -- replayed in the same
    precision (np.float64 / np.float32): every step's flags and reward and the five final counters are equal exactly (a NaN equal to a NaN)."""
    K, E = TALLY_K, TALLY_E
    cause, sums = tally_inputs()
    ft = {"f64": np.float64, "f32": np.float32}[prec]
    t = types.SimpleNamespace(length=np.zeros(E, dtype=np.int64), count=np.zeros(E, dtype=np.int64), sum_length=np.zeros(E, dtype=np.int64),
                              ret=np.zeros(E, dtype=ft), sum_return=np.zeros(E, dtype=ft))
    params = dict(max_steps=max_steps, term_penalty=TALLY_PENALTY)
    steps = [EO.tally_step(params, t, cause[k], sums[k].astype(ft)) for k in range(K)]
    flags, reward, done, length = (np.stack([s[j] for s in steps]) for j in range(4))
    assert reward.dtype == ft
    # the situations the inputs are there for
    term, trunc = (flags & 1) != 0, (flags & 2) != 0
    assert not (term & trunc).any() and (done == (term | trunc)).all() and (flags >> 8 == cause).all()
    assert (trunc[:, 0] == ((np.arange(K) + 1) % max_steps == 0 if max_steps else np.zeros(K, dtype=bool))).all()
    assert term[2, 1] and term[5, 1] and (length[[2, 5], 1] == max_steps).all() if max_steps == 3 else term[2, 1]
    assert done[4, 2] and done[5, 2] and length[5, 2] == 1
    assert (trunc[2, 3] and term[3, 3]) if max_steps == 3 else term[3, 3]
    assert np.isnan(reward[1, 4]) and not np.isnan(reward[2, 4]) and np.isnan(t.sum_return[4]) and np.isnan(reward[6, 5]) and np.isnan(t.sum_return[5])
    assert not np.isnan(t.sum_return[[0, 1, 2, 3, 6, 7]]).any()
    fin, fout = str(tmp_path / "tally.in"), str(tmp_path / "tally.out")
    np.concatenate([np.array([K, E, max_steps, TALLY_PENALTY]), cause.astype(np.float64).reshape(-1), sums.reshape(-1)]).tofile(fin)
    ran = subprocess.run([rule_program, fin, fout, prec, "tally"], capture_output=True, text=True)
    assert ran.returncode == 0, (ran.returncode, ran.stderr[-2000:])
    out = np.fromfile(fout, dtype=np.float64)
    assert out.size == 2 * K * E + 5 * E
    np.testing.assert_array_equal(out[:K * E].astype(np.int64).reshape(K, E), flags)
    np.testing.assert_array_equal(out[K * E:2 * K * E].reshape(K, E), reward.astype(np.float64))
    got = out[2 * K * E:].reshape(5, E)
    for row, name in enumerate(("length", "count", "sum_length", "ret", "sum_return")):
        np.testing.assert_array_equal(got[row], getattr(t, name).astype(np.float64), err_msg=name)
    assert t.count.sum() > 0 and (t.sum_length + t.length == K).all()


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

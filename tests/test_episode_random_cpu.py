"""Randomised episode starts without a GPU: the generator's known answers, the header (csrc/mds_episode_random.hpp) compiled with g++
under AddressSanitizer + UBSan against the NumPy restatement of tests/episode_random_oracle.py, the draw's own sanity, the scenarios'
conditions on the float64 oracle, and the argument checks of the new entry points."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from multidronesim_amd import _capi as capi
from tests import episode_random_cases as RC
from tests import episode_random_oracle as RO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEAR = 1e-4
# Random123's known answers of Philox4x32-10: counter[4], key[2] -> out[4]
KNOWN = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
         ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
         ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1")]


def test_numpy_philox_gives_the_known_answers():
    for counter, key, want in KNOWN:
        assert " ".join("%08x" % int(w) for w in RO.philox4x32_10(counter, key)) == want
    # vectorised over a leading axis, the key broadcast: row by row the same
    got = RO.philox4x32_10([k[0] for k in KNOWN], [k[1] for k in KNOWN])
    assert [" ".join("%08x" % int(w) for w in row) for row in got] == [k[2] for k in KNOWN]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build the header's stand-alone program"
    exe = str(tmp_path_factory.mktemp("episode_random") / "episode_random_main")
    # the sanitizer runtimes linked statically: the program needs nothing preloaded and is indifferent to what the environment preloads
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan",
                           "-static-libubsan", "-o", exe, os.path.join(ROOT, "tests", "episode_random_main.cpp")])
    return exe


def test_header_philox_gives_the_known_answers(program):
    done = subprocess.run([program, "kat"], capture_output=True, text=True)
    assert done.returncode == 0, (done.returncode, done.stderr[-2000:])
    assert done.stdout.split("\n")[:3] == [k[2] for k in KNOWN]


def tuples(n=4096):
    """(seed, rows [n, 9] = g, ordinal, generation, xyz, rpy): random 32-bit words, with the corners of g and ordinal (0, 1, 2^31, 2^32 - 2,
    2^32 - 1) among them.  xyz on a 2^-10 m grid: exact in float32, so the image's position is the nominal one in both compute types."""
    rng = np.random.default_rng(11)
    corners = np.array([0, 1, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 2, 2 ** 32 - 1], dtype=np.float64)
    g = rng.integers(0, 2 ** 32, size=n).astype(np.float64)
    ordinal = rng.integers(0, 2 ** 32, size=n).astype(np.float64)
    ordinal[n // 2:] = rng.integers(0, 50, size=n - n // 2)                  # (what a run sees)
    generation = rng.integers(0, 4, size=n).astype(np.float64)
    cg, co = np.meshgrid(corners, corners, indexing="ij")
    g[:36], ordinal[:36], generation[:36] = cg.ravel(), co.ravel(), 2.0 ** 32 - 1
    xyz = np.round(rng.uniform(-4.0, 4.0, size=(n, 3)) * 1024) / 1024
    xyz[36:72] = 0.0
    rpy = rng.uniform(-0.5, 0.5, size=(n, 3))
    return np.concatenate([g[:, None], ordinal[:, None], generation[:, None], xyz, rpy], axis=1)


def run_draw(program, tmp_path, seed, half, rows, prec):
    fin, fout = str(tmp_path / "draw.in"), str(tmp_path / f"draw_{prec}.out")
    head = [rows.shape[0], seed & 0xFFFFFFFF, seed >> 32] + list(half)
    np.concatenate([np.array(head, dtype=np.float64), rows.reshape(-1)]).tofile(fin)
    done = subprocess.run([program, "draw", fin, fout, prec], capture_output=True, text=True)
    assert done.returncode == 0, (done.returncode, done.stderr[-2000:])
    out = np.fromfile(fout, dtype=np.float64).reshape(rows.shape[0], 25)
    return out[:, :12], out[:, 12:]


@pytest.mark.parametrize("half", [RO.half_widths(**RC.HALF), RO.half_widths(pos=[0.3, 0.0, 0.02], rpy=0.0, vel=[0.0, 1.5, 0.0], rate=[2.0, 0.0, 0.0])])
def test_header_draw_matches_the_oracle(program, tmp_path, half):
    """mds_episode_random.hpp on the host (g++, ASan + UBSan, a program of its own) over a few thousand (seed, g, ordinal, generation) tuples:
    the s values bitwise the oracle's in both compute types.  float64: the drawn state within 1e-12.  float32: velocity and rates -- the
    offsets themselves -- within 1 ulp of (float32) of the oracle's (the half-width's rounding and the product's, 2^-24 relative each); a
    position within 1 ulp of its offset + half an ulp of itself (the sum's rounding; the nominal position is exact in float32 here); the
    quaternion within 1e-6.  A zero half-width gives exactly 0, and with the three attitude half-widths 0 the quaternion is the image's."""
    seed, rows = RC.SEED, tuples()
    want_s = RO.units(seed, rows[:, 0], rows[:, 1], rows[:, 2])
    assert (np.abs(want_s) < 1.0).all() and (want_s != 0.0).all()
    want = RO.start_state(seed, rows[:, 0], rows[:, 1], rows[:, 2], half, rows[:, 3:6], rows[:, 6:9])
    off = RO.offsets(seed, rows[:, 0], rows[:, 1], rows[:, 2], half)
    s64, st64 = run_draw(program, tmp_path, seed, half, rows, "f64")
    np.testing.assert_array_equal(s64, want_s)
    np.testing.assert_allclose(st64, want, rtol=0, atol=1e-12)
    s32, st32 = run_draw(program, tmp_path, seed, half, rows, "f32")
    np.testing.assert_array_equal(s32, want_s)
    ulp = lambda x: np.spacing(np.abs(x).astype(np.float32)).astype(np.float64)          # noqa: E731
    assert (np.abs(st32[:, 7:13] - want[:, 7:13]) <= ulp(want[:, 7:13])).all()
    assert (np.abs(st32[:, 0:3] - want[:, 0:3]) <= ulp(off[:, 0:3]) + 0.5 * ulp(want[:, 0:3])).all()
    np.testing.assert_allclose(st32[:, 3:7], want[:, 3:7], rtol=0, atol=1e-6)
    for st, dt in ((st64, np.float64), (st32, np.float32)):
        zero = np.flatnonzero(half == 0.0)
        for k in zero[zero >= 6]:
            assert (st[:, 1 + k] == 0.0).all() and not np.signbit(st[:, 1 + k]).any()
        for k in zero[zero < 3]:
            np.testing.assert_array_equal(st[:, k], rows[:, 3 + k])
        if (half[3:6] == 0.0).all():                 # the image's quaternion: the program's own float64 one, rounded to the compute type
            np.testing.assert_array_equal(st[:, 3:7], st64[:, 3:7].astype(dt).astype(np.float64))
            np.testing.assert_allclose(st64[:, 3:7], want[:, 3:7], rtol=0, atol=1e-15)


def test_draws_are_centred_and_strictly_inside_the_half_width():
    """On the oracle alone, 2^16 draws per component: the mean within 4 standard errors of 0 (a uniform on (-w, w) has the standard
    deviation w / sqrt 3), every value strictly inside +-w."""
    n = 1 << 16
    half = RO.half_widths(**RC.HALF)
    g = np.arange(n) % 257 + 2 ** 32 - 300
    o = RO.offsets(RC.SEED, g, np.arange(n) // 257, 1, half)
    assert (np.abs(o) < half[None, :]).all()
    se = half / np.sqrt(3.0) / np.sqrt(n)
    assert (np.abs(o.mean(axis=0)) <= 4.0 * se).all(), o.mean(axis=0) / se
    assert len(np.unique(o[:, 0])) > 0.99 * n                                         # (no two drones share a stream)


@pytest.mark.parametrize("E,D", RC.SHAPES)
def test_scenarios_end_enough_episodes_and_stay_clear_of_the_thresholds(E, D):
    """Conditions on the test inputs, on the oracle alone: with the half-widths of tests/episode_random_cases.py each rule ends at least 20
    episodes per shape, and at most 10 % of the envs ever come within 1e-4 (relative) of a threshold.  Half-widths that fail this are changed
    in tests/episode_random_cases.py; the caps stay."""
    for name in RC.RULES:
        r = RC.oracle_run(E, D, name)
        ended = int(((r["flags"] & 3) != 0).sum())
        near = int((r["margin"] < NEAR).any(axis=0).sum())
        print(f"{E}x{D} {name}: episodes ended {ended}, envs near a threshold {near}")
        assert ended >= 20, (name, ended)
        assert near <= 0.10 * E, (name, near, E)
        # the starts differ from episode to episode and from the nominal pose
        nominal = RC.EC.oracle_run(E, D, name)
        assert not np.array_equal(r["obs_now"], nominal["obs_now"])
    assert not np.array_equal(RC.oracle_run(E, D, "trunc")["first_rows"], RC.oracle_run(E, D, "trunc")["last_rows"])


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return capi.load_library()


def test_entry_points_validate_before_touching_the_device(lib):
    """null handle -> MDS_EINVAL from both new entry points, with no device present; the struct is 8 + 8 + 12 x 8 bytes"""
    assert C.sizeof(capi.MdsEpisodeRandomisation) == 8 + 8 + 12 * 8
    p = capi.MdsEpisodeRandomisation()
    assert lib.mds_set_episode_randomisation(None, C.byref(p), None) == -1
    assert lib.mds_set_episode_randomisation(None, None, None) == -1
    assert b"mds_set_episode_randomisation" in lib.mds_last_error()
    assert lib.mds_reset_episodes(None, None, None) == -1
    assert b"mds_reset_episodes" in lib.mds_last_error()
    assert lib.mds_version() == 202

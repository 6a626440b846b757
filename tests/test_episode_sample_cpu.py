"""Gaussian actions of the MLP policy without a GPU: the scenarios' own conditions on the float64 oracle, the noise header
(csrc/mds_policy_noise.hpp) compiled with g++ under AddressSanitizer + UBSan against the oracle and torch, the distribution of 2^20
draws, the argument checks of the new entry points, and the compiler's resource figures of the new kernels."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from multidronesim_amd import _capi as capi
from tests import episode_random_oracle as RO
from tests import episode_sample_cases as XC
from tests import episode_sample_oracle as SO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "multidronesim_amd", "csrc")
NEAR = 1e-4
HOVER = SO.PO.O.CF2P.HOVER_RPM
R_MAX = float(np.sqrt(48.0 * np.log(2.0)))          # sqrt(-2 ln 2^-24) = 5.77


@pytest.mark.parametrize("E,D", XC.SHAPES)
def test_scenarios_exercise_the_clamp_and_do_not_amplify_rounding(E, D):
    """Conditions on the test inputs, on the oracle alone.  Between 1 % and 25 % of the sample components lie outside +-1 (the clamp is
    exercised by the noise); at least 20 compared done-events, at least 20 of them rule terminations; in at least 10 steps some envs are
    done while others are not; at most 10 % of the envs ever come within 1e-4 of a threshold; and the oracle re-run with the state and
    the commanded RPM rounded to float32 at every step stays within a third of the float32 gates of the GPU test on the compared part
    (state 1e-5 absolute, RPM and action 1e-5 relative, reward 1e-5 D, sample 2e-4, flags equal).  A log_std or seed that fails this is
    changed in tests/episode_sample_cases.py; the caps stay."""
    r, s = XC.oracle_run(E, D), XC.oracle_run(E, D, "every step")
    T = XC.STEPS
    outside = float((np.abs(r["sample"]) > 1.0).mean())
    assert 0.01 <= outside <= 0.25, outside
    first, keep = XC.compared_part(r, NEAR)
    flags = r["flags"]
    done = (flags & 3) != 0
    assert int(done[keep].sum()) >= 20
    term = ((flags & 1) != 0) & (((flags >> 8) & 0x3F) != 0)
    assert int((term & keep).sum()) >= 20
    assert int(((done.sum(axis=1) > 0) & (done.sum(axis=1) < E)).sum()) >= 10
    assert (first < T).sum() <= 0.10 * E
    np.testing.assert_array_equal(s["flags"][keep], r["flags"][keep])
    obs, obr = (a["obs"].reshape(T, E, D, 20)[keep] for a in (r, s))
    act, acr = (a["action"].reshape(T, E, D, 4)[keep] for a in (r, s))
    smp, smr = (a["sample"].reshape(T, E, D, 4)[keep] for a in (r, s))
    print(f"{E}x{D}: outside the clamp {outside:.3f}; rounded every step: state {np.abs(obr - obs)[..., :16].max():.2e}, RPM "
          f"{np.abs(obr[..., 16:] / obs[..., 16:] - 1).max():.2e}, sample {np.abs(smr - smp).max():.2e}")
    np.testing.assert_allclose(obr[..., :16], obs[..., :16], rtol=0, atol=1e-5 / 3)
    np.testing.assert_allclose(obr[..., 16:], obs[..., 16:], rtol=1e-5 / 3, atol=0)
    np.testing.assert_allclose(acr, act, rtol=1e-5 / 3, atol=0)
    np.testing.assert_allclose(smr, smp, rtol=0, atol=2e-4 / 3)
    np.testing.assert_allclose(s["reward"][keep], r["reward"][keep], rtol=0, atol=1e-5 * D / 3)
    # the noise of the rounded run is the same noise: the draw does not see the state
    np.testing.assert_array_equal(s["eps"].reshape(T, E, D, 4)[keep], r["eps"].reshape(T, E, D, 4)[keep])


def test_cases_are_what_the_tests_assume():
    assert len(set(XC.LOG_STD)) == 4 and XC.NOISE_SEED != XC.RC.SEED
    assert any(v != 0 for v in XC.FIRST_ENV.values()) and set(XC.FIRST_ENV) == set(XC.SHAPES)


def test_safety_scenario_fires_the_pair_cause():
    """the composed scenario of the GPU test (collision causes + randomised starts + sampled actions): bit 14 ends at least 5 episodes"""
    r = XC.safety_oracle_run()
    assert int(((r["flags"] >> 14) & 1).sum()) >= 5


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build the noise header's stand-alone program"
    exe = str(tmp_path_factory.mktemp("episode_sample") / "episode_sample_main")
    # the sanitizer runtimes linked statically: the program needs nothing preloaded and is indifferent to what the environment preloads
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan",
                           "-static-libubsan", "-o", exe, os.path.join(ROOT, "tests", "episode_sample_main.cpp")])
    return exe


def run_program(exe, tmp_path, tag, prec, form, head, *arrays):
    fin, fout = str(tmp_path / f"{tag}.in"), str(tmp_path / f"{tag}_{prec}_{form}.out")
    np.concatenate([np.asarray(head, dtype=np.float64)] + [np.asarray(a, dtype=np.float64).reshape(-1) for a in arrays]).tofile(fin)
    done = subprocess.run([exe, fin, fout, prec, form], capture_output=True, text=True)
    assert done.returncode == 0, (done.returncode, done.stderr[-2000:])
    return np.fromfile(fout, dtype=np.float64)


def seed_words(seed):
    return [seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF]


# the words of the extreme draws: u = 2^-24 (w_a >> 9 == 0) and 1 - 2^-24 (all ones), theta next to -pi (w_b >> 8 == 0) and +pi
EXTREME = np.array([[a, b, b2, a2] for a in (0, 0x1FF, 0xFFFFFFFF, 0xFFFFFE00) for b in (0, 0xFF, 0xFFFFFFFF, 0xFFFFFF00, 0x80000000, 0x7FFFFFFF)
                    for a2, b2 in ((a ^ 0xFFFFFFFF, b ^ 0xFFFFFFFF),)], dtype=np.uint64)


def draw_inputs(n=4096, seed=3):
    rng = np.random.default_rng(seed)
    i = rng.integers(0, 2 ** 20, size=n)
    ordinal = rng.integers(0, 2 ** 32, size=n)
    length = rng.integers(0, 2 ** 32, size=n)                # (the sum 3 + length wraps for the largest)
    length[:3] = [2 ** 32 - 1, 2 ** 32 - 3, 0]
    y = rng.standard_normal((n, 4))
    return i, ordinal, length, y


def run_draw(program, tmp_path, prec, first, epoch, rows, tag="draw", seed=XC.NOISE_SEED, log_std=XC.LOG_STD):
    i, ordinal, length, y = rows
    head = [i.size, *seed_words(seed), first, epoch, HOVER, 0.05 * HOVER, *log_std]
    out = run_program(program, tmp_path, tag, prec, "draw", head, np.column_stack([i, ordinal, length, y])).reshape(i.size, 17)
    return dict(words=out[:, 0:4].astype(np.uint64), eps=out[:, 4:8], a=out[:, 8:12], logp=out[:, 12], rpm=out[:, 13:17])


def test_header_float64_against_the_oracle_and_torch(program, tmp_path):
    """mds_policy_noise.hpp on the host (g++, ASan + UBSan, a program of its own), float64: the words equal the oracle's Philox block;
    eps, a, logp and the RPM against the oracle at rtol 1e-12 (atol 1e-12 where a value crosses zero); logp also against
    torch.distributions.Normal(y, sigma).log_prob(a).sum(-1) in float64 at 1e-12; the extreme words (u = 2^-24 and 1 - 2^-24, theta
    next to +-pi) included."""
    import torch
    rows = draw_inputs()
    i, ordinal, length, y = rows
    first, epoch = 1000 * 7, 5
    got = run_draw(program, tmp_path, "f64", first, epoch, rows)
    w = SO.words(XC.NOISE_SEED, first + i, ordinal, length, epoch)
    np.testing.assert_array_equal(got["words"], w)
    eps = SO.box_muller(w)
    a, logp = SO.sample(y, eps, XC.LOG_STD)
    np.testing.assert_allclose(got["eps"], eps, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(got["a"], a, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(got["logp"], logp, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(got["rpm"], SO.PO.rpm_of(a), rtol=1e-12, atol=0)
    assert 0.01 < (np.abs(a) > 1).mean() < 0.9                                   # both arms of the clamp
    sigma = torch.as_tensor(np.exp(np.asarray(XC.LOG_STD)))
    lt = torch.distributions.Normal(torch.as_tensor(y), sigma).log_prob(torch.as_tensor(got["a"])).sum(-1).numpy()
    np.testing.assert_allclose(got["logp"], lt, rtol=1e-12, atol=1e-12)
    # the extreme words
    e64 = run_program(program, tmp_path, "extreme", "f64", "words", [EXTREME.shape[0]], EXTREME).reshape(-1, 4)
    want = SO.box_muller(EXTREME)
    np.testing.assert_allclose(e64, want, rtol=1e-12, atol=1e-12)
    assert np.isfinite(e64).all() and np.abs(e64).max() <= R_MAX
    assert np.isclose(np.hypot(want[:, 0], want[:, 1]).max(), R_MAX, rtol=1e-12)   # u = 2^-24 is among them
    e32 = run_program(program, tmp_path, "extreme", "f32", "words", [EXTREME.shape[0]], EXTREME).reshape(-1, 4)
    assert np.isfinite(e32).all()
    np.testing.assert_allclose(e32, want, rtol=0, atol=4e-6)


def test_header_float32_against_the_float64_oracle(program, tmp_path):
    """float32 against the float64 oracle.  eps within 4e-6 absolute: r <= 5.77, times the rounding of pi * s (1.2e-7) plus a few ulp
    each from log, sqrt and sincos.  logp within 1e-4 absolute: at most sum |eps_j| * 4e-6 with four terms of at most 5.77.  Over 2^16
    draws plus the inputs of the float64 test.  (If the host build exceeded either bound the arithmetic would be wrong, not the bound.)"""
    rows = draw_inputs(2 ** 16, seed=4)
    i, ordinal, length, y = rows
    got = run_draw(program, tmp_path, "f32", 0, 2, rows, tag="draw32")
    w = SO.words(XC.NOISE_SEED, i, ordinal, length, 2)
    np.testing.assert_array_equal(got["words"], w)
    eps = SO.box_muller(w)
    y32 = y.astype(np.float32).astype(np.float64)
    a, logp = SO.sample(y32, eps, XC.LOG_STD)
    err_eps, err_logp, err_a = np.abs(got["eps"] - eps).max(), np.abs(got["logp"] - logp).max(), np.abs(got["a"] - a).max()
    print(f"float32 host build: max |eps err| {err_eps:.3e}, max |logp err| {err_logp:.3e}, max |a err| {err_a:.3e}, max |eps| {np.abs(eps).max():.3f}")
    assert err_eps <= 4e-6 and err_logp <= 1e-4
    np.testing.assert_allclose(got["a"], a, rtol=0, atol=2e-6 + 4e-6 * np.exp(max(XC.LOG_STD)))
    np.testing.assert_allclose(got["rpm"], SO.PO.rpm_of(a), rtol=1e-5, atol=0)


def test_the_draw_is_a_pure_function_of_its_five_arguments(program, tmp_path):
    """the same (seed, g, ordinal, length, epoch) gives the same words whatever else differs (y, log_std, how g splits into first + i,
    the precision); changing any one of the five changes all four values"""
    rows = draw_inputs(512, seed=9)
    i, ordinal, length, y = rows
    base = run_draw(program, tmp_path, "f64", 700, 3, rows, tag="pure0")
    other = run_draw(program, tmp_path, "f64", 0, 3, (i + 700, ordinal, length, y[::-1] * 3.0), tag="pure1", log_std=(0.1, 0.2, 0.3, 0.4))
    np.testing.assert_array_equal(other["words"], base["words"])
    np.testing.assert_array_equal(other["eps"], base["eps"])
    np.testing.assert_array_equal(run_draw(program, tmp_path, "f32", 700, 3, rows, tag="pure2")["words"], base["words"])
    changed = {"seed": run_draw(program, tmp_path, "f64", 700, 3, rows, tag="pure3", seed=XC.NOISE_SEED ^ (1 << 40)),
               "g": run_draw(program, tmp_path, "f64", 701, 3, rows, tag="pure4"),
               "ordinal": run_draw(program, tmp_path, "f64", 700, 3, (i, (ordinal + 1) % 2 ** 32, length, y), tag="pure5"),
               "length": run_draw(program, tmp_path, "f64", 700, 3, (i, ordinal, (length + 1) % 2 ** 32, y), tag="pure6"),
               "epoch": run_draw(program, tmp_path, "f64", 700, 4, rows, tag="pure7")}
    for name, c in changed.items():
        assert (c["words"] != base["words"]).all(), name
        assert (c["eps"] != base["eps"]).all(), name


def test_no_block_coincides_with_a_start_draw(program, tmp_path):
    """with the seed of the randomised starts and epoch == generation, the noise block of length 0, 1, 2 differs from the start draw's
    blocks b = 0, 1, 2 of the same (g, ordinal): word 2 of the counter starts at 3"""
    n = 200
    rng = np.random.default_rng(12)
    g, ordinal = rng.integers(0, 2 ** 20, size=n), rng.integers(0, 50, size=n)
    seed, gen = XC.RC.SEED, 4
    counters = np.stack([np.stack([g, ordinal, np.full(n, b), np.full(n, gen)], axis=-1) for b in range(3)])          # [3, n, 4]
    start = run_program(program, tmp_path, "start", "f64", "philox", [3 * n, *seed_words(seed)], counters).reshape(3, n, 4).astype(np.uint64)
    np.testing.assert_array_equal(start, np.stack([RO.philox4x32_10(c, np.array(seed_words(seed), dtype=np.uint64)) for c in counters]))
    zeros = np.zeros((n, 4))
    for length in range(3):
        noise = run_draw(program, tmp_path, "f64", 0, gen, (g, ordinal, np.full(n, length), zeros), tag=f"coll{length}", seed=seed)["words"]
        for b in range(3):
            assert (noise != start[b]).any(axis=-1).all(), (length, b)
    # ... and the counter word is what makes them differ: length = b - 3 (mod 2^32) is the start block itself
    same = run_draw(program, tmp_path, "f64", 0, gen, (g, ordinal, np.full(n, 2 ** 32 - 3), zeros), tag="coll_same", seed=seed)["words"]
    np.testing.assert_array_equal(same, start[0])


def test_distribution_of_a_million_draws(program, tmp_path):
    """2^20 draws (g ascending, the rest fixed) from the host program, float32: per-component mean within 5 / sqrt(N), variance within
    1 +- 0.01, excess kurtosis within +-0.05, pairwise correlation of the four components and of consecutive `length` within
    5 / sqrt(N), max |eps| <= 5.77"""
    N = 2 ** 20
    head = [N, *seed_words(XC.NOISE_SEED), 7, 11, 2]
    e = run_program(program, tmp_path, "stream", "f32", "stream", head).reshape(N, 4)
    nxt = run_program(program, tmp_path, "stream_next", "f32", "stream", head[:4] + [12, 2]).reshape(N, 4)
    lim = 5.0 / np.sqrt(N)
    mean, var = e.mean(axis=0), e.var(axis=0)
    kurt = ((e - mean) ** 4).mean(axis=0) / var ** 2 - 3.0
    corr = np.corrcoef(np.concatenate([e, nxt], axis=1), rowvar=False)
    off = corr[~np.eye(8, dtype=bool)]
    print(f"mean {mean}, var {var}, excess kurtosis {kurt}, max |corr| {np.abs(off).max():.2e} (bound {lim:.2e}), max |eps| {np.abs(e).max():.3f}")
    assert (np.abs(mean) <= lim).all()
    assert (np.abs(var - 1.0) <= 0.01).all()
    assert (np.abs(kurt) <= 0.05).all()
    assert (np.abs(off) <= lim).all()
    assert np.abs(e).max() <= 5.77 and np.abs(nxt).max() <= 5.77


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return capi.load_library()


def test_struct_layout_and_null_handles(lib):
    """struct sizes; null handle -> MDS_EINVAL from the three entry points, with no device present; mds_last_error names the call"""
    assert C.sizeof(capi.MdsEpisodePolicyNoise) == 8 + 8 + 4 * 8
    assert C.sizeof(capi.MdsEpisodeSampleRings) == 7 * C.sizeof(C.c_void_p)
    p = capi.MdsEpisodePolicyNoise(1, 0, (C.c_double * 4)(*XC.LOG_STD))
    rings = capi.MdsEpisodeSampleRings()
    buf = C.create_string_buffer(64)
    assert lib.mds_set_episode_policy_noise(None, C.byref(p), None) == -1
    assert b"mds_set_episode_policy_noise" in lib.mds_last_error()
    assert lib.mds_set_episode_policy_noise(None, None, None) == -1
    assert lib.mds_episode_policy_sample(None, buf, buf, None, None, None) == -1
    assert b"mds_episode_policy_sample" in lib.mds_last_error()
    assert lib.mds_rollout_episodes_sampled(None, 0, 1, C.byref(rings), 0, 1, None, None) == -1
    assert b"mds_rollout_episodes_sampled" in lib.mds_last_error()
    assert lib.mds_rollout_episodes_sampled(None, 0, 1, None, 0, 1, None, None) == -1


def test_capi_table_and_header_carry_the_new_names():
    header = open(os.path.join(ROOT, "include", "mds.h")).read()
    for name in ("mds_set_episode_policy_noise", "mds_rollout_episodes_sampled", "mds_episode_policy_sample"):
        assert name in capi.PROTOTYPES, name
        assert re.search(r"\bint " + name + r"\(", header), name
    assert "typedef struct mds_episode_policy_noise" in header and "typedef struct mds_episode_sample_rings" in header
    assert "#define MDS_VERSION 202" in header


ROLL_ARGS = ("const Consts<T>, const EpisodeRule<T>, const int, const size_t, const int, const int, T*, const T*, const T*, const T*, T*, "
             "const EpisodePolicy<T>, T*, T*, T*, int*, int, const int, const int, T*, const EpisodeCounters<T>, const int, "
             "const EpisodeSafetyArgs<T>, const int, const EpisodeRandomArgs<T>")
SAMPLED_ARGS = ("const Consts<T>, const EpisodeRule<T>, const int, const size_t, const int, const int, T*, const T*, const T*, const T*, T*, "
                "const EpisodePolicy<T>, const PolicyNoise<T>, const EpisodeSampleRings<T, T>, int, const int, const int, T*, "
                "const EpisodeCounters<T>, const int, const EpisodeSafetyArgs<T>, const int, const EpisodeRandomArgs<T>")
INCLUDES = ['#include <hip/hip_runtime.h>', '#include "mds_kernels.hip"', '#include "mds_episode_kernels.hip"',
            '#include "mds_episode_policy_kernels.hip"', '#include "mds_episode_sample_kernels.hip"', "namespace mds {"]
# (T, RK4, DRAG, W) of the rollout kernels and (T, W) of the flat ones: the siblings' set (float64 + RK4 is built 64 wide only)
ROLL_SET = [(T, rk4, drag, W) for T in ("float", "double") for W in (32, 64) for rk4 in ("false", "true") for drag in ("false", "true")
            if not (T == "double" and rk4 == "true" and W == 32)]
FLAT_SET = [(T, W) for T in ("float", "double") for W in (32, 64)]


def kernel_figures(text):
    meta = text[text.index("amdhsa.kernels:"):]
    seen = {}
    for blk in meta.split("\n  - "):
        m = re.search(r"\.name:\s+(\S+)\n", blk)
        if m:
            seen[m.group(1)] = {k: int(re.search(r"\." + k + r":\s+(\d+)", blk).group(1)) for k in
                                ("private_segment_fixed_size", "group_segment_fixed_size", "vgpr_count", "agpr_count", "sgpr_count")}
    return seen


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    """the sampled kernels and their deterministic siblings, every instantiation the library holds, cross-compiled to assembly with the
    library's flags (two compilations side by side)"""
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not available")
    import sys
    sys.path.insert(0, ROOT)
    from __graft_entry__ import HIPCC_FLAGS
    d = tmp_path_factory.mktemp("sample_isa")
    files = {}
    for tag, roll, roll_args, flat, flat_args in (
            ("sampled", "k_rollout_episodes_sampled", SAMPLED_ARGS, "k_episode_policy_sample",
             "const int, const size_t, const int, const T*, const T*, const EpisodePolicy<T>, const PolicyNoise<T>, const int*, const int*, "
             "const T*, T*, T*, T*"),
            ("sibling", "k_rollout_episodes_policy", ROLL_ARGS, "k_episode_policy_compute",
             "const int, const size_t, const T*, const T*, const EpisodePolicy<T>, const T*, T*")):
        lines = list(INCLUDES)
        lines.append(f"#define ROLL(T, RK4, DRAG, W) template __global__ void {roll}<T, T, RK4, DRAG, W>({roll_args});")
        lines.append(f"#define FLAT(T, W) template __global__ void {flat}<T, T, W>({flat_args});")
        lines += [f"FLAT({T}, {W})" for T, W in FLAT_SET]
        lines += [f"ROLL({T}, {rk4}, {drag}, {W})" for T, rk4, drag, W in ROLL_SET]
        lines.append("}")
        src = d / f"{tag}_kernels.hip"
        src.write_text("\n".join(lines) + "\n")
        files[tag] = (src, d / f"{tag}_kernels.s")
    procs = {tag: subprocess.Popen(["hipcc", *HIPCC_FLAGS, "-I", CSRC, "-S", "--cuda-device-only", "-o", str(out), str(src)], stderr=subprocess.DEVNULL)
             for tag, (src, out) in files.items()}
    for tag, p in procs.items():
        assert p.wait() == 0, tag
    return {tag: open(out).read() for tag, (src, out) in files.items()}


def waves_per_simd(fig, wave_slots=8, vgpr_file=512):
    """waves per SIMD that the unified VGPR file allows (gfx950: 512 registers per lane, allocated in blocks of 8, at most 8 waves)"""
    v = -(-max(fig["vgpr_count"], 1) // 8) * 8                 # (vgpr_count is the unified total: the AGPRs are part of it)
    return min(wave_slots, vgpr_file // v)


def test_sampled_kernels_resources(isa, lib):
    """0 bytes of scratch in every instantiation, LDS within a workgroup's 64 KiB and not above the sibling's, at most 512 VGPRs, and no
    rollout instantiation in a lower occupancy tier (waves per SIMD) than its sibling.  The
    instantiations compiled here are the (T, RK4, DRAG, W) set of the siblings and the ones the library holds: the kernel names in
    libmds.so's code object are the same set.  The figures are printed beside the siblings' (DESIGN.md has them)."""
    new, old = kernel_figures(isa["sampled"]), kernel_figures(isa["sibling"])
    assert len(new) == len(FLAT_SET) + len(ROLL_SET) == len(old) == 4 + 14, (list(new), list(old))
    blob = open(capi.LIB_PATH, "rb").read()
    in_lib = {m.decode() for m in re.findall(rb"_ZN3mds2[0-9]k_(?:rollout_episodes_sampled|episode_policy_sample)I\w+", blob)}
    assert in_lib == set(new), (sorted(in_lib - set(new)), sorted(set(new) - in_lib))
    # a sampled kernel and its sibling differ in the name only: the template arguments' mangling is the same
    def key(name):
        for mine, theirs in (("26k_rollout_episodes_sampled", "25k_rollout_episodes_policy"), ("23k_episode_policy_sample", "24k_episode_policy_compute")):
            name = name.replace(mine, theirs)
        return name.split("EEv")[0]
    by_key = {key(o): o for o in old}
    pairs = {name: by_key[key(name)] for name in new}
    assert len(set(pairs.values())) == len(old)
    print()
    for name, sib in pairs.items():
        a, b = new[name], old[sib]
        print(f"{name[:60]}: VGPR {a['vgpr_count']} ({b['vgpr_count']}) AGPR {a['agpr_count']} ({b['agpr_count']}) SGPR {a['sgpr_count']} "
              f"({b['sgpr_count']}) LDS {a['group_segment_fixed_size']} ({b['group_segment_fixed_size']}) scratch "
              f"{a['private_segment_fixed_size']} ({b['private_segment_fixed_size']}) waves/SIMD {waves_per_simd(a)} ({waves_per_simd(b)})")
        assert a["group_segment_fixed_size"] <= b["group_segment_fixed_size"], name
        if "rollout" in name:                                # the draw must not cost a rollout kernel its occupancy tier
            assert waves_per_simd(a) >= waves_per_simd(b), name
    assert all(v["group_segment_fixed_size"] <= 65536 for v in new.values())
    assert all(v["vgpr_count"] <= 512 for v in new.values())
    assert not re.search(r"\tscratch_(load|store)", isa["sampled"])
    with_scratch = {k: v["private_segment_fixed_size"] for k, v in new.items() if v["private_segment_fixed_size"]}
    assert not with_scratch, with_scratch

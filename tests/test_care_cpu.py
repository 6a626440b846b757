"""The Riccati solver of the dLQR gains on the CPU: csrc/mds_care.hpp (Gauss-Jordan inverse, scaled Newton sign iteration, P, K and the
residual) compiled with g++ into a stand-alone program (tests/emul/care_host.cpp) against the reference-minted gains of
tests/golden/fedce_ref_in_loop.npz / fedce_omega_ref_in_loop.npz and against scipy.linalg.solve_continuous_are.  The program also runs
once under -fsanitize=address,undefined, and the cross-compiled library's mds_care kernels must carry no scratch.

Measured (float64, relative to max |K|): fixture pairs 12-state 8.4e-14, 9-state 4.5e-14 (gate 1e-13); 200 perturbed hover models per
size against scipy 9-state 1.2e-13, 12-state 1.6e-13, coupled pair 4.6e-13 (gate 1e-12, scipy solves all 600); D = 3 assembled from
the groups {0,1} + {2} against scipy on the 36 x 36 system 3.5e-14.  Iterations: 8 (12-state, pair), 10 (9-state) on the fixture
models, 8..10 over the sweep.  Worst relative residual 7.9e-13 (9-state sweep) -> kCareResidualTol = 1e-11."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import scipy.linalg as la

from tests import fedce_omega_oracle as FO
from tests import fedce_oracle as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "multidronesim_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "emul", "care_host.cpp")
NEW = ["mds_dlqr_solve_gain", "mds_dlqr_omega_solve_gain"]
MODE = {(9, 4): 0, (12, 4): 1, (24, 8): 2}
GATE_FIXTURE = 1e-13          # the measured maximum rounded up to the next power of ten (module docstring)
GATE_SWEEP = 1e-12
RES_TOL = 1e-11               # kCareResidualTol of the header


def rel(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def _build(tmp, sanitize):
    exe = os.path.join(tmp, "care_host" + ("_san" if sanitize else ""))
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else ["-O2"]
    subprocess.check_call(["g++", "-std=c++17", *flags, "-ffp-contract=off", "-I", CSRC, "-o", exe, SRC])
    return exe


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to build the host program")
    return _build(str(tmp_path_factory.mktemp("care")), False)


def run(exe, mode, count, payload, max_iter=32):
    data = np.concatenate([[float(mode), float(count), float(max_iter)], np.asarray(payload, dtype=np.float64).ravel()]).tobytes()
    p = subprocess.run([exe], input=data, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    assert b"runtime error" not in p.stderr and b"ERROR" not in p.stderr, p.stderr.decode()[-2000:]
    return np.frombuffer(p.stdout, dtype=np.float64)


def solve(exe, cases, max_iter=32):
    """cases: list of (A, B, Q, R) of one size -> status [n], iters [n], residual [n], K [n, NU, NS], P [n, NS, NS]"""
    ns, nu = cases[0][1].shape
    payload = np.concatenate([np.concatenate([A.ravel(), B.ravel(), np.linalg.inv(R).ravel(), Q.ravel()]) for A, B, Q, R in cases])
    out = run(exe, MODE[(ns, nu)], len(cases), payload, max_iter).reshape(len(cases), 3 + nu * ns + ns * ns)
    return (out[:, 0].astype(int), out[:, 1].astype(int), out[:, 2], out[:, 3:3 + nu * ns].reshape(-1, nu, ns),
            out[:, 3 + nu * ns:].reshape(-1, ns, ns))


def scipy_gain(A, B, Q, R):
    P = la.solve_continuous_are(A, B, Q, R, e=None, s=None, balanced=True)
    return la.solve(R, B.T @ P)


def blocks(A, B, Q, R, m, drones):
    """the sub-problem of the listed drones of the block system (m states, 4 inputs per drone)"""
    si = np.concatenate([np.arange(m * d, m * (d + 1)) for d in drones])
    ui = np.concatenate([np.arange(4 * d, 4 * (d + 1)) for d in drones])
    return A[np.ix_(si, si)], B[np.ix_(si, ui)], Q[np.ix_(si, si)], R[np.ix_(ui, ui)]


def grouped_gain(exe, A, B, Q, R, m, groups):
    """K [4D, mD] assembled from the header's solutions of the groups -> (K, statuses, iterations, residuals)"""
    K = np.zeros((B.shape[1], A.shape[0]))
    sts, its, ress = [], [], []
    for g in groups:
        st, it, res, Kg, _ = solve(exe, [blocks(A, B, Q, R, m, g)])
        si = np.concatenate([np.arange(m * d, m * (d + 1)) for d in g])
        ui = np.concatenate([np.arange(4 * d, 4 * (d + 1)) for d in g])
        K[np.ix_(ui, si)] = Kg[0]
        sts.append(st[0]); its.append(it[0]); ress.append(res[0])
    return K, sts, its, ress


def groups_of(m, D):
    return ([(0, 1)] if (m == 12 and D >= 2) else [(d,) for d in range(min(D, 2))]) + [(d,) for d in range(2, D)]


def fixture_pairs(golden_dir):
    """(m, D, A, B, Q, R, K of the fixture) for K[i + 1] from theta[i] and K[0] from theta[0]; the last theta has no K"""
    out = []
    for name, m, make in (("fedce_ref_in_loop.npz", 12, F.DLQR), ("fedce_omega_ref_in_loop.npz", 9, FO.DLQROmega)):
        d = np.load(os.path.join(golden_dir, name))
        for D in (2, 3):
            th, Ks = d[f"d{D}_thetas"], d[f"d{D}_Ks"]
            ctl = make(D)
            for dst in range(len(Ks)):
                src = max(dst - 1, 0)
                out.append((m, D, th[src][:m * D].T.copy(), th[src][m * D:].T.copy(), ctl.Q, ctl.R, Ks[dst]))
    return out


def test_fixture_pairs(golden_dir, host):
    worst = {9: 0.0, 12: 0.0}
    res_worst, iters = 0.0, {9: set(), 12: set()}
    for m, D, A, B, Q, R, Kfix in fixture_pairs(golden_dir):
        assert rel(scipy_gain(A, B, Q, R), Kfix) < 1e-11          # the precondition: this theta is the one the fixture's K came from
        K, sts, its, ress = grouped_gain(host, A, B, Q, R, m, groups_of(m, D))
        assert not any(sts), sts
        worst[m] = max(worst[m], rel(K, Kfix))
        res_worst = max(res_worst, max(ress))
        iters[m] |= set(its)
    print(f"fixture pairs: K vs fixture 12-state {worst[12]:.2e}, 9-state {worst[9]:.2e}; iterations 12-state {sorted(iters[12])}, "
          f"9-state {sorted(iters[9])}; worst residual {res_worst:.2e}")
    assert max(its for v in iters.values() for its in v) < 32
    assert res_worst < RES_TOL / 10
    assert max(worst.values()) < GATE_FIXTURE


def perturbed(rng, M, dense):
    A, B = M
    s = lambda X: X * (1 + rng.choice([-1.0, 1.0], X.shape) * rng.uniform(.2, .3, X.shape))      # noqa: E731
    A, B = s(A), s(B)
    if dense:
        A = A + 1e-2 * rng.normal(size=A.shape)
        B = B + 1e-2 * rng.normal(size=B.shape)
    return A, B


def sweep_cases(size, n=200, seed=11):
    rng = np.random.default_rng(seed + size)
    if size == 9:
        c = FO.DLQROmega(1)
        return [(*perturbed(rng, FO.lin_model(), True), c.ind_Q, c.ind_R) for _ in range(n)]
    hover = F.lin_model()[2:]
    if size == 12:
        c = F.DLQR(1)
        return [(*perturbed(rng, hover, False), c.ind_Q, c.ind_R) for _ in range(n)]
    c = F.DLQR(2)
    out = []
    for _ in range(n):
        (A0, B0), (A1, B1) = perturbed(rng, hover, False), perturbed(rng, hover, False)
        out.append((la.block_diag(A0, A1), la.block_diag(B0, B1), c.Q, c.R))
    return out


@pytest.mark.parametrize("size", [9, 12, 24])
def test_perturbed_models_against_scipy(host, size):
    cases = sweep_cases(size)
    ref = []
    for A, B, Q, R in cases:
        try:
            ref.append(scipy_gain(A, B, Q, R))
        except (np.linalg.LinAlgError, ValueError):
            ref.append(None)
    ok = np.array([r is not None for r in ref])
    assert ok.mean() >= 0.95
    st, it, res, K, _ = solve(host, cases)
    err = max(rel(K[k], ref[k]) for k in np.flatnonzero(ok))
    print(f"size {size}: scipy solved {int(ok.sum())}/{len(cases)}; K vs scipy {err:.2e}; iterations {it[ok].min()}..{it[ok].max()}; "
          f"worst residual {res[ok].max():.2e}")
    assert (st[ok] == 0).all(), st[ok]
    assert it.max() < 32
    assert res[ok].max() < RES_TOL / 10          # the threshold sits one order of magnitude over the worst residual seen
    assert err < GATE_SWEEP


def test_group_assembly_matches_the_full_system(golden_dir, host):
    """D = 3, 12-state: K from the groups {0,1} + {2} against scipy on the full 36 x 36 system (every block outside the groups is 0)."""
    d = np.load(os.path.join(golden_dir, "fedce_ref_in_loop.npz"))
    th = d["d3_thetas"][1]
    ctl = F.DLQR(3)
    A, B = th[:36].T, th[36:].T
    K, sts, _, _ = grouped_gain(host, A, B, ctl.Q, ctl.R, 12, [(0, 1), (2,)])
    Kref = scipy_gain(A, B, ctl.Q, ctl.R)
    print(f"group assembly: {rel(K, Kref):.2e}")
    assert not any(sts)
    assert rel(K, Kref) < GATE_FIXTURE * 10


def unstabilisable():
    A12, B12 = (x.copy() for x in F.lin_model()[2:])
    B12[8, 0] = 0.0
    A9, B9 = (x.copy() for x in FO.lin_model())
    B9[5, 0] = 0.0
    c12, c9 = F.DLQR(1), FO.DLQROmega(1)
    return [(A12, B12, c12.ind_Q, c12.ind_R), (A9, B9, c9.ind_Q, c9.ind_R)]


def test_unstabilisable_models_end_with_a_status_and_no_gain(host):
    for case in unstabilisable():
        with pytest.raises(np.linalg.LinAlgError):
            scipy_gain(*case)
        st, it, res, K, P = solve(host, [case])
        print(f"n = {case[0].shape[0]}: status {st[0]} after {it[0]} iterations")
        assert st[0] != 0 and np.isnan(K).all() and np.isnan(P).all()


def test_iteration_cap_sets_bit_0(host):
    c = F.DLQR(1)
    A, B = F.lin_model()[2:]
    st, it, _, K, _ = solve(host, [(A, B, c.ind_Q, c.ind_R)], max_iter=3)
    assert st[0] == 1 and it[0] == 3 and np.isnan(K).all()


def test_model_accessors(host):
    rng = np.random.default_rng(2)
    f = rng.normal(size=12)
    out = run(host, 3, 1, f)
    A, B = out[:144].reshape(12, 12), out[144:].reshape(12, 4)
    Ar, Br = np.zeros((12, 12)), np.zeros((12, 4))
    Ar[0:3, 3:6] = Ar[9:12, 6:9] = np.eye(3)
    Ar[6, 1], Ar[7, 0], Br[3:6, 1:4], Br[8, 0] = f[0], f[1], f[2:11].reshape(3, 3), f[11]
    np.testing.assert_array_equal(A, Ar)
    np.testing.assert_array_equal(B, Br)
    th = rng.normal(size=(13, 9))
    out = run(host, 4, 1, th)
    np.testing.assert_array_equal(out[:81].reshape(9, 9), th[:9].T)
    np.testing.assert_array_equal(out[81:].reshape(9, 4), th[9:].T)


def test_host_program_under_asan_ubsan(golden_dir, tmp_path):
    """The same arithmetic once under AddressSanitizer + UndefinedBehaviorSanitizer (a stand-alone program: nothing loaded into python
    is sanitized): the fixture pairs and the failure cases."""
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to build the host program")
    exe = _build(str(tmp_path), True)
    for m, D, A, B, Q, R, Kfix in fixture_pairs(golden_dir):
        K, sts, _, _ = grouped_gain(exe, A, B, Q, R, m, groups_of(m, D))
        assert not any(sts) and rel(K, Kfix) < GATE_FIXTURE
    for case in unstabilisable():
        st, _, _, K, _ = solve(exe, [case])
        assert st[0] != 0 and np.isnan(K).all()


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not available")
    import sys
    sys.path.insert(0, ROOT)
    from __graft_entry__ import HIPCC_FLAGS
    out = tmp_path_factory.mktemp("isa") / "mds2.s"
    subprocess.check_call(["hipcc", *HIPCC_FLAGS, "-DMDS_PART=2", "-S", "--cuda-device-only", "-o", str(out),
                           os.path.join(CSRC, "mds_api.hip")], stderr=subprocess.DEVNULL)
    return open(out).read()


def test_care_kernels_have_no_scratch(isa):
    meta = isa[isa.index("amdhsa.kernels:"):]
    seen = {}
    for blk in meta.split("\n  - "):
        m = re.search(r"\.name:\s+(\S+)\n", blk)
        if not m or "k_care_" not in m.group(1):
            continue
        seen[m.group(1)] = int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", blk).group(1))
        assert int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1)) == 0, m.group(1)
    solve_k = [k for k in seen if "k_care_solve" in k]
    print({k: v for k, v in seen.items()})
    assert len(solve_k) == 3, seen                        # Hamiltonian widths 18, 24, 48
    assert len(seen) == 3 + 4, seen                       # + the commit kernel: (float | double) x (12 | 9 states)
    assert all(seen[k] <= 65536 for k in solve_k)


def test_capi_table_and_header_carry_the_new_names():
    from multidronesim_amd import _capi as capi
    header = open(os.path.join(ROOT, "include", "mds.h")).read()
    for name in NEW:
        assert name in capi.PROTOTYPES, name
        assert re.search(r"\bint " + name + r"\(", header), name


def test_null_handle_returns_einval():
    from multidronesim_amd import _capi as capi
    if not os.path.exists(capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = capi.load_library()
    assert lib.mds_dlqr_solve_gain(None, None, None, 32, None, None, None, None) == -1
    assert lib.mds_dlqr_omega_solve_gain(None, None, None, 32, None, None, None, None) == -1

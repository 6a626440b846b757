"""The segment-table trajectory path on the CPU: the image builder of csrc/mds_traj_image.hpp (what mds_set_trajectory_segments
uploads) and the evaluators of csrc/mds_traj.hpp (traj_eval, TrajLocal<float>, TrajLocal<double>) reading that image, built with g++
(tests/emul/traj_emul.cpp) and compared with the float64 oracle classes of oracle/np_trajectories.py on the 333 drones and the edge
times of tests/traj_cases.py.  CPU only.

Measured on this case set (host build, g++ -O2 -mfma -ffp-contract=fast), max over 333 drones x 1984 times, and the gates:

    group                               measured    gate (fp32: 4 x measured, see FP32_GATE)
    float64  all 11 components          1.4e-12     1e-11 (the golden gate; 9.1e-13 at t = 1e4 + 0.37)
    fp32  p / max(1 m, |p - origin|)    1.52e-7     6.08e-7
    fp32  v                             1.72e-7     6.88e-7
    fp32  a                             7.02e-7     2.81e-6
    fp32  yaw (mod 2 pi)                5.45e-7     2.18e-6
    fp32  yaw rate                      1.80e-7     7.20e-7

The factor 4 covers what the device build does differently from this one: v_rcp_f32 (1 ulp) for 1/x, and other contraction choices."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import traj_cases as TC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMUL = os.path.join(ROOT, "tests", "emul")
_PD, _PI = C.POINTER(C.c_double), C.POINTER(C.c_int32)
MDS_OK, MDS_EINVAL = 0, -1
SEG_DIM = 40

# measured maxima of the host fp32 evaluator against the oracle on this case set, per component group; the gate is 4 x each
FP32_MEASURED = {"p": 1.52e-7, "v": 1.72e-7, "a": 7.02e-7, "yaw": 5.45e-7, "yaw_rate": 1.80e-7}
FP32_GATE = {k: 4 * v for k, v in FP32_MEASURED.items()}
GROUPS = {"p": slice(0, 3), "v": slice(3, 6), "a": slice(6, 9), "yaw": slice(9, 10), "yaw_rate": slice(10, 11)}


def ip(a):
    return a.ctypes.data_as(_PI)


def dp(a):
    return a.ctypes.data_as(_PD)


class Image:
    """build_traj_image through the shim: .status, and when accepted .nu, .fm [40, nu], .tinfo [n, 3], .info(i), .eval(mode, ts, origin)."""

    def __init__(self, lib, segs, offsets, compound, total=None):
        self.lib = lib
        segs = np.ascontiguousarray(segs, dtype=np.float64)
        offsets, compound = np.ascontiguousarray(offsets, dtype=np.int32), np.ascontiguousarray(compound, dtype=np.int32)
        self.n = len(compound)
        st = C.c_int(0)
        self.h = lib.traj_image_create(dp(segs), ip(offsets), ip(compound), C.c_int(self.n), C.c_int32(segs.shape[0] if total is None else total),
                                       C.byref(st))
        self.status = st.value
        if self.h:
            self.nu = lib.traj_image_nu(C.c_void_p(self.h))
            self.fm, self.tinfo = np.zeros((SEG_DIM, self.nu)), np.zeros((self.n, 3), dtype=np.int32)
            lib.traj_image_copy(C.c_void_p(self.h), dp(self.fm), ip(self.tinfo))

    def info(self, i):
        out = np.zeros(4, dtype=np.int32)
        self.lib.traj_image_info(C.c_void_p(self.h), C.c_int(i), ip(out))
        return tuple(int(x) for x in out)        # first, nseg, compound, stride

    def eval(self, mode, ts, origin):
        ts = np.ascontiguousarray(ts, dtype=np.float64)
        origin = np.ascontiguousarray(origin, dtype=np.float64).reshape(self.n, 3)
        out = np.zeros((len(ts), self.n, 11))
        self.lib.traj_image_eval(C.c_void_p(self.h), C.c_int(mode), C.c_int(len(ts)), dp(ts), dp(origin), dp(out))
        return out

    def __del__(self):
        if getattr(self, "h", None):
            self.lib.traj_image_free(C.c_void_p(self.h))


@pytest.fixture(scope="module")
def traj_lib(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    so = str(tmp_path_factory.mktemp("traj_emul") / "libtraj_emul.so")
    # the flags of tests/emul/emul.py
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-mfma", "-ffp-contract=fast", "-o", so, os.path.join(EMUL, "traj_emul.cpp")])
    lib = C.CDLL(so)
    lib.traj_image_create.restype = C.c_void_p
    lib.traj_image_nu.restype = C.c_int
    return lib


@pytest.fixture(scope="module")
def case(traj_lib):
    """The 333 drones once: rows, image, the full time set, the oracle's desired state and the three evaluators' answers."""
    lobjs, names = TC.drones(TC.library_classes())
    oobjs, _ = TC.drones(TC.oracle_classes())
    segs, off, comp, anchors = TC.flatten(lobjs, names)
    ts = TC.times_full(oobjs)
    im = Image(traj_lib, segs, off, comp)
    assert im.status == MDS_OK
    c = dict(names=names, oobjs=oobjs, segs=segs, off=off, comp=comp, anchors=anchors, ts=ts, im=im, want=TC.oracle_desired(oobjs, names, ts),
             scale=TC.f64_gate_scale(oobjs, names, ts))
    c["f64"], c["f32"], c["local64"] = (im.eval(m, ts, anchors) for m in (0, 1, 2))
    return c


def group_errors(got, want, origin):
    """max |got - want| per component group over [nt, n]: p relative to max(1 m, |p - origin|), yaw modulo 2 pi."""
    d = np.abs(got - want)
    d[..., 9] = np.abs(TC.wrap(got[..., 9] - want[..., 9]))
    d[..., 0:3] /= np.maximum(1.0, np.abs(want[..., 0:3] - origin[None]))
    return {g: d[..., sl].max(axis=-1) for g, sl in GROUPS.items()}


# ---- B1: layout ---------------------------------------------------------------------------------------------------------------------

def test_every_drone_reads_its_own_table_from_the_shared_image(traj_lib, case):
    """traj_eval on the 333-drone image == the oracle for that drone's own object (1e-11), and == the same drone evaluated from a
    one-table image of its own rows to the bit, in all three evaluators: the layout property itself (first + k * stride, blocks, ranks,
    the compound bit, the affine tag)."""
    err = np.abs(case["f64"] - case["want"])
    err[..., 9] = np.abs(TC.wrap(case["f64"][..., 9] - case["want"][..., 9]))
    worst = (err.max(axis=-1) / case["scale"]).max(axis=0)
    print("max |traj_eval(image) - oracle| per drone: %.3e" % worst.max())
    assert worst.max() < 1e-11, {i: (case["names"][i], worst[i]) for i in np.argsort(worst)[-5:]}
    off, comp = case["off"], case["comp"]
    for i in range(len(comp)):
        own = Image(traj_lib, case["segs"][off[i]:off[i + 1]], [0, off[i + 1] - off[i]], comp[i:i + 1])
        assert own.status == MDS_OK and own.info(0)[0] == 0 and own.info(0)[3] == 1
        for mode, key in ((0, "f64"), (1, "f32"), (2, "local64")):
            np.testing.assert_array_equal(own.eval(mode, case["ts"], case["anchors"][i])[:, 0], case[key][:, i], err_msg=f"drone {i} {case['names'][i]} mode {mode}")


def test_image_structure(case):
    """nu = pieces of the distinct tables; drones share `first` exactly when their rows are bytewise equal; stride = distinct tables of
    that piece count; equal rows under different compound flags share storage and differ in tinfo[1] only."""
    im, off, comp, segs, names = case["im"], case["off"], case["comp"], case["segs"], case["names"]
    n = len(comp)
    key = [segs[off[i]:off[i + 1]].tobytes() for i in range(n)]
    distinct = {}
    for k in key:
        distinct.setdefault(k, len(k) // (8 * SEG_DIM))
    assert im.nu == sum(distinct.values())
    assert sorted(set(distinct.values())) == [1, 2, 3, 4, 17, 300]
    # order of first appearance of the distinct tables' piece counts: blocks open, pause and reopen
    assert list(distinct.values())[:7] == [3, 1, 3, 4, 1, 2, 3]
    info = [im.info(i) for i in range(n)]
    for i in range(n):
        first, nseg, cflag, stride = info[i]
        assert nseg == off[i + 1] - off[i] and cflag == comp[i]
        assert stride == sum(1 for v in distinct.values() if v == nseg)
        assert 0 <= first and first + (nseg - 1) * stride < im.nu
    first = np.array([f[0] for f in info])
    same_first = first[:, None] == first[None, :]
    same_rows = np.array([[key[i] == key[j] for j in range(n)] for i in range(n)])
    assert (same_first == same_rows).all()
    # the pieces of every drone, read back from the field-major image, are its rows (field 0 carries the affine tag)
    for i in range(n):
        f0, nseg, _, stride = info[i]
        back = im.fm[:, f0 + stride * np.arange(nseg)].T
        rows = segs[off[i]:off[i + 1]]
        np.testing.assert_array_equal(back[:, 1:], rows[:, 1:])
        ident = (rows[:, 27:36] == np.eye(3).reshape(-1)).all(axis=1) & (rows[:, 36:39] == 0).all(axis=1)
        np.testing.assert_array_equal(back[:, 0], rows[:, 0] + np.where(ident, 0.0, 8.0))
    assert any(n.startswith("rotate") for n in names) and (im.fm[0] >= 8).any() and (im.fm[0] < 8).any()
    # bare Circle / Compound([that Circle]) / an equal Circle from another object: one copy, the flag in tinfo[1] only
    a, b, c = names.index("circle1"), names.index("circle1_in_compound"), names.index("circle1_again")
    assert im.tinfo[a, 0] == im.tinfo[b, 0] == im.tinfo[c, 0] and im.tinfo[a, 2] == im.tinfo[b, 2]
    assert im.tinfo[a, 1] == 1 and im.tinfo[b, 1] == (1 | 1 << 16) and im.tinfo[c, 1] == 1
    # ... and they part ways past the end: the Compound holds the end pose, the bare Circle goes on
    T1 = case["oobjs"]["circle1"].get_total_time()
    late = case["ts"] > T1 * 1.01
    assert np.abs(case["f64"][late][:, a, 0:2] - case["f64"][late][:, b, 0:2]).max() > 0.1
    np.testing.assert_array_equal(case["f64"][:, a], case["f64"][:, c])


def wait_rows(k):
    s = np.zeros((k, SEG_DIM))
    s[:, 0], s[:, 1], s[:, 2] = 3.0, 0.5 * np.arange(k), 0.5 * (np.arange(k) + 1)
    s[:, 3], s[:, 4], s[:, 5], s[:, 6] = 0.001 * np.arange(k), -1.0, 2.0, 0.25
    s[:, 27] = s[:, 31] = s[:, 35] = 1.0
    return s


def test_image_refusals_and_the_piece_count_limit(traj_lib):
    s = wait_rows(4)
    assert Image(traj_lib, s, [0, 1, 4], [0, 1]).status == MDS_OK
    assert Image(traj_lib, s, [1, 2, 4], [0, 1]).status == MDS_EINVAL                 # offsets[0] != 0
    assert Image(traj_lib, s, [0, 1, 3], [0, 1]).status == MDS_EINVAL                 # offsets[n] != total
    assert Image(traj_lib, s, [0, 0, 4], [0, 1]).status == MDS_EINVAL                 # a drone with 0 pieces
    for bad in (-1.0, 4.0):
        for row in (0, 3):
            m = s.copy()
            m[row, 0] = bad
            assert Image(traj_lib, m, [0, 1, 4], [0, 1]).status == MDS_EINVAL         # kind -1, kind 4
    big = wait_rows(65537)
    assert Image(traj_lib, big, [0, 65536, 65537], [1, 0]).status == MDS_EINVAL       # 65536 pieces
    for cflag in (1, 0):
        im = Image(traj_lib, big[:65536], [0, 65535, 65536], [cflag, 1 - cflag])
        assert im.status == MDS_OK
        assert im.info(0) == (0, 65535, cflag, 1) and im.info(1) == (65535, 1, 1 - cflag, 1)    # blocks in order of first appearance
        assert im.tinfo[0, 1] == (65535 | cflag << 16)
        out = im.eval(0, [0.25, 0.5 * 65534 + 0.25, 1e6], np.zeros((2, 3)))
        # drone 0: first piece, last piece; past the end a Compound holds the last piece, a bare table reads piece 0
        np.testing.assert_array_equal(out[:, 0, 0], [0.0, 0.001 * 65534 if cflag else 0.0, 0.001 * 65534 if cflag else 0.0])
        np.testing.assert_array_equal(out[:, 1, 0], [0.001 * 65535] * 3)


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_layout_cases_as_a_host_program_under_asan_and_ubsan(tmp_path):
    """The layout, refusal and 65535-piece cases from tests/emul/traj_image_main.cpp, a plain executable built with
    -fsanitize=address,undefined: an index of the builder or of an evaluator outside the image ends it.  Exit status 0 required."""
    lobjs, names = TC.drones(TC.library_classes())
    oobjs, _ = TC.drones(TC.oracle_classes())
    segs, off, comp, anchors = TC.flatten(lobjs, names)
    ts = TC.times_gpu(oobjs)
    data = tmp_path / "tables.bin"
    with open(data, "wb") as f:
        f.write(np.array([len(comp), segs.shape[0], len(ts)], dtype=np.int32).tobytes())
        for a in (off, comp, segs, ts, anchors):
            f.write(a.tobytes())
    exe = str(tmp_path / "traj_image_main")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-mfma", "-ffp-contract=fast", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", exe, os.path.join(EMUL, "traj_image_main.cpp"), os.path.join(EMUL, "traj_emul.cpp")])
    env = dict(os.environ, UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1", ASAN_OPTIONS="detect_leaks=0:halt_on_error=1")   # as tests/emul/simt/simt.py
    out = subprocess.run([exe, str(data)], capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]


# ---- B2: evaluator arithmetic, host build -----------------------------------------------------------------------------------------------

def test_double_evaluators_match_the_oracle(case):
    """traj_eval against the oracle per component group at 1e-11 (the gate of test_trajectory_call_matches_reference_golden), yaw
    modulo 2 pi.  For the large-t samples the gate is scaled by max(1, |phase| 2^-52 1e3), |phase| <= (largest of omega, v / r and the
    yaw rates of the drone's pieces) |t|.  TrajLocal<double> is traj_eval minus the origin, exactly."""
    got, want = case["f64"], case["want"]
    d = np.abs(got - want)
    d[..., 9] = np.abs(TC.wrap(got[..., 9] - want[..., 9]))
    for g, sl in GROUPS.items():
        e = d[..., sl].max(axis=-1)
        big = case["ts"] > 500
        print("float64 %-8s max err %.3e (t > 500: %.3e)" % (g, e[~big].max(), e[big].max()))
        assert (e / case["scale"]).max() < 1e-11, g
    loc = got.copy()
    loc[..., 0:3] -= case["anchors"][None]
    np.testing.assert_array_equal(case["local64"], loc)


def test_fp32_evaluator_matches_the_oracle(case):
    """TrajLocal<float> (world frame: (double) des.p + (double)(float) origin) against the oracle per component group, each gated at
    4 x the maximum measured on this case set with the host build (FP32_MEASURED, the table in the module docstring)."""
    org = case["anchors"].astype(np.float32).astype(np.float64)
    errs = group_errors(case["f32"], case["want"], org)
    for g, e in errs.items():
        j, i = np.unravel_index(np.argmax(e), e.shape)
        print("fp32 %-8s max err %.3e at drone %d (%s) t = %.17g   [measured %.1e, gate %.1e]" % (g, e.max(), i, case["names"][i], case["ts"][j],
                                                                                                   FP32_MEASURED[g], FP32_GATE[g]))
    for g, e in errs.items():
        assert e.max() < FP32_GATE[g], g


# ---- the conditions of the one-step GPU tests, on the oracle alone ------------------------------------------------------------------------

def test_one_step_conditions_hold_on_the_oracle_alone(traj_lib, case):
    """test_step_geometric_on_segment_tables_one_step_at_the_desired_state and its LQR twin (tests/test_gpu_trajectories.py) compare one
    fused step's RPM with the oracle at G_op + 4 P.  Here, without a GPU and without the kernels:
      * P, the largest change of the oracle's answer when it is fed the host build's fp32 desired state instead of the float64 one, is
        what tests/traj_cases.py records (GEO_P, LQR_P: recorded >= measured, and no more than 1.25 x measured);
      * exclusions (the oracle's controller saturates, or the LQR yaw error lies within 0.1 of +-pi): at most 5 % of the (drone, time)
        cases and at most 20 % of any drone's;
      * resolving power: an error planted in one component of the oracle's desired state moves the answer by more than 3 x the gate in
        at least 95 % of the cases whose segment kind produces that component.  Geometric: 1e-3 in p, v and yaw, 1e-2 in a and yaw rate.
        LQR: ten times those sizes.  Its existing operator gate (test_lqr12_golden: 6e-4 of the largest thrust) is two orders above the
        geometric one, and at 1e-3 only p, v_z and the yaw rate clear 3 x gate = 1.8e-3 (p_xy 1.9e-3; v_xy 1.3e-3 and yaw 1.3e-3 do not);
        what is finer than that is pinned by test_fp32_evaluator_matches_the_oracle and by the geometric step."""
    from oracle import np_oracle as O
    names, oobjs = case["names"], case["oobjs"]
    ts = TC.times_gpu(oobjs)
    want = TC.oracle_desired(oobjs, names, ts)
    d32 = case["im"].eval(1, ts, case["anchors"])
    produced = TC.produced_components(oobjs, names, want)
    K = O.lqr12_gain()
    setups = {
        "geometric": (TC.GEO_STATES, TC.GEO_P, TC.GEO_GATE, 1.0, lambda obs, des: TC.geometric_rpm(obs, des),
                      lambda obs, des: TC.geometric_saturates(obs, des), lambda a, b, keep: np.abs(a / b - 1).max(axis=-1)),
        "lqr": (TC.LQR_STATES, TC.LQR_P, TC.LQR_GATE, 10.0, lambda obs, des: TC.lqr_rpm(obs, des, K),
                lambda obs, des: TC.lqr_saturates(obs, des, K), TC.thrust_error),
    }
    for ctrl, (kw, p_rec, gate, plant_scale, rpm, saturates, metric) in setups.items():
        obs = TC.exact_obs(TC.near_states(want, case["anchors"], **kw))
        keep = ~saturates(obs, want)
        print(f"{ctrl}: excluded {100 * (1 - keep.mean()):.2f} % of the cases, at most {100 * (1 - keep.mean(axis=0).min()):.1f} % of one drone's")
        assert keep.mean() >= 0.95 and keep.mean(axis=0).min() >= 0.80, ctrl
        ref = rpm(obs, want)
        P = metric(rpm(obs, d32), ref, keep)[keep].max()
        print(f"{ctrl}: P = {P:.3e} (recorded {p_rec:.3e}), gate {gate:.3e}")
        assert P <= p_rec <= 1.25 * P, (ctrl, P, p_rec)
        for comp, (sl, size) in TC.PLANT.items():
            if ctrl == "lqr" and comp == "a":
                continue                                         # the LQR law does not read the acceleration
            for k in range(sl.start, sl.stop):
                m = produced[..., k] & keep
                des = want.copy()
                des[..., k] += size * plant_scale
                moved = metric(rpm(obs, des), ref, keep)[m]
                share = (moved > 3 * gate).mean()
                print(f"{ctrl}: {size * plant_scale:g} in component {k} ({comp}) moves {100 * share:.1f} % of {m.sum()} cases by more than 3 x gate "
                      f"(min {moved.min():.2e}, median {np.median(moved):.2e})")
                assert m.sum() > 1000 and share >= 0.95, (ctrl, comp, k)

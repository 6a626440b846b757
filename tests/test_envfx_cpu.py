"""tests/envfx_cases.py on the oracle alone: every scene of tests/test_gpu_envfx.py does what its GPU test claims.

  * every loop scene stays finite, has at most 10 % of its (drone, step) pairs with a motor at a limit, and differs from the same run under
    plain dyn by FACTOR x the largest gate its GPU test uses (one-drone envs under dyn_dw: no env-mate, so the run IS the plain one);
  * a kernel that lost the env-mates across a wavefront boundary, or read them from the output side of the double buffer, moves the oracle's
    result for the boundary envs by FACTOR x that gate;
  * the one-substep batches reach every branch of the two force laws with at least four drones each;
  * the wind with y and z swapped moves the oracle by FACTOR x the gate."""
import numpy as np
import pytest

from oracle import np_oracle as O
from tests import envfx_cases as X

NAMES = list(X.MODES.values())
PATHS = ["step", "geo"]


def _largest_gate(path, ref):
    return X.gate(path, "float32", ref)           # float32's is the larger of the two dtypes' gates


def test_boundary_envs_are_the_ones_the_shapes_were_chosen_for():
    assert X.boundary_envs(37, 7) == [9, 18, 27, 36] and list(X.drones_of([9], 7)) == list(range(63, 70))
    assert list(X.drones_of([36], 7)) == list(range(252, 259))
    assert X.boundary_envs(52, 5) == [12, 25, 38, 51] and list(X.drones_of([12], 5)) == list(range(60, 65))
    assert list(X.drones_of([51], 5)) == list(range(255, 260))
    assert X.boundary_envs(17, 16) == [16] and X.drones_of([16], 16)[0] == X.BLOCK
    assert X.boundary_envs(1, 1) == [] and X.boundary_envs(3, 1) == []
    for E, D in X.BIG:
        sub = X.sub_envs(E, D)
        assert set(X.boundary_envs(E, D)) <= set(sub) and len(sub) * D <= X.WAVE - 1 and (len(sub) + 1) * D > X.WAVE - 1
        assert X.boundary_envs(len(sub), D) == []                      # nothing straddles in the second handle


def test_no_two_envs_of_a_scene_are_alike_and_displacing_is_exact():
    for E, D in X.BIG:
        s = X.stacked(E, D)
        rel = (s["xyz"] - s["cen"][:, :1]).reshape(E, -1)
        assert len(np.unique(np.round(rel, 9), axis=0)) == E and len(np.unique(np.round(s["ph"].reshape(E, -1), 9), axis=0)) == E
        d = X.displaced(s)
        f32 = lambda a: np.asarray(a, dtype=np.float32).astype(np.float64)
        assert np.array_equal(f32(d["cen"]), d["cen"]) and np.array_equal(f32(s["cen"]), s["cen"])      # origins are exact in fp32
        assert np.array_equal(d["xyz"] - d["cen"], s["xyz"] - s["cen"])                                  # local coordinates: the same bits
        assert np.abs(d["xyz"][..., 0]).min() > 500 and np.abs(d["xyz"][..., 1]).min() > 250 and np.array_equal(d["xyz"][..., 2], s["xyz"][..., 2])
        assert len(np.unique(np.sign(d["cen"][:, 0, :2]), axis=0)) == 4                                   # all four sign pairs occur


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("shape", X.SHAPES)
def test_loop_scene_is_finite_unsaturated_and_feels_the_effect(shape, name, path):
    E, D = shape
    run, plain = X.loop_run(E, D, name, path), X.loop_run(E, D, "dyn", path)
    assert np.isfinite(run["obs"]).all()
    assert X.limit_fraction(run) <= 0.10
    eff = X.state_err(run["obs"][-1], plain["obs"][-1])
    if D == 1 and name == "dyn_dw":
        assert eff == 0.0                          # a one-drone env has no env-mate: the downwash mode is plain dyn there, exactly
    else:
        assert eff >= X.FACTOR * _largest_gate(path, run["obs"][-1]), eff


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", ["dyn_dw", "dyn_gnd_drag_dw"])
@pytest.mark.parametrize("shape", X.BIG)
def test_a_wrong_kernel_would_show_on_the_boundary_envs(shape, name, path):
    E, D = shape
    run = X.loop_run(E, D, name, path)
    b = X.drones_of(X.boundary_envs(E, D), D)
    need = X.FACTOR * _largest_gate(path, run["obs"][-1])
    stale = X.loop_run(E, D, name, path, variant="stale")
    assert X.state_err(stale["obs"][-1][b], run["obs"][-1][b]) >= need
    cut = X.loop_run(E, D, name, path, variant="cut")
    straddles = [e for e in X.boundary_envs(E, D) if (e * D) // X.WAVE != (e * D + D - 1) // X.WAVE]
    if straddles:
        for e in straddles:                        # every straddling env on its own
            d = X.drones_of([e], D)
            assert X.state_err(cut["obs"][-1][d], run["obs"][-1][d]) >= need, e
        inner = np.setdiff1d(np.arange(E * D), b)
        assert X.state_err(cut["obs"][-1][inner], run["obs"][-1][inner]) == 0.0
    else:                                          # (17, 16): envs start on wavefront boundaries, none lies across one
        assert X.state_err(cut["obs"][-1], run["obs"][-1]) == 0.0


def test_variant_downwash_reduces_to_the_oracles():
    s = X.stacked(5, 7)
    p = s["xyz"].reshape(-1, 3)
    np.testing.assert_array_equal(X.downwash_general(p, p, 7, O.CF2P), O.downwash_force(p, 7, O.CF2P))
    np.testing.assert_array_equal(X.downwash_general(p, p, 7, O.CF2P, mask=np.ones((35, 35), dtype=bool)), O.downwash_force(p, 7, O.CF2P))


@pytest.mark.filterwarnings("ignore:divide by zero")          # the oracle's u = dxy / (c_2 dz + c_3) at dz = 0.6875 exactly: inf, exp(-inf) = 0
@pytest.mark.parametrize("model", ["cf2p", "cf2x"])
def test_one_substep_batches_reach_every_branch(model):
    c = O.CF2X if model == "cf2x" else O.CF2P
    b = X.pair_batch(model)
    tags, s = b["tags"], b["state"]
    assert all(len(v) >= 4 for v in tags.values()) and len(s) % 2 == 0
    dz, dxy = (a[:, 0] for a in X.pair_geometry(b))
    dw = O.downwash_force(s[:, 0:3], 2, c)
    # the lateral cut-off, either side, by 1 cm and by one fp32 ulp: on or off, and on means a force the float64 gate sees
    av, _ = X.accelerations(b)
    gate64 = 1e-9 * np.abs(av).max()
    for tin, tout in (("lat_in", "lat_out"), ("ulp_in", "ulp_out")):
        i, o = tags[tin], tags[tout]
        assert (dxy[i] < 10).all() and (dxy[o] > 10).all() and (dz[i] > 0).all() and (dz[o] > 0).all()
        assert (dw[o] == 0).all() and (np.abs(dw[i]) / c.M > X.FACTOR * gate64).all()
    assert (dxy[tags["ulp_in"]] == X.ULP_IN).all() and (dxy[tags["ulp_out"]] == X.ULP_OUT).all()
    assert np.float32(X.ULP_IN) < np.float32(10) < np.float32(X.ULP_OUT) and np.float32(X.ULP_IN) == X.ULP_IN
    assert (dz[tags["equal_z"]] == 0).all() and (dw[tags["equal_z"]] == 0).all() and (dw[tags["equal_z"] + 1] == 0).all()   # neither is pushed
    assert (dz[tags["mate_below_only"]] < 0).all() and (dw[tags["mate_below_only"]] == 0).all()
    assert (dw[tags["mate_above"]] < -0.1).all()
    for z in X.BETA_DZ:
        for r in X.BETA_DXY:
            i = tags[f"beta_{z}_{r}"]
            np.testing.assert_allclose(dz[i], z, rtol=0, atol=1e-12)
            np.testing.assert_allclose(dxy[i], r, rtol=0, atol=1e-12)
            assert np.isfinite(dw[i]).all() and (np.abs(dw[i]) < 1e-30).all() and (dxy[i] > 0).all()
    # ground effect
    h, rpy = X.prop_heights(b)
    g = O.ground_effect_forces(s[:, 0:3], s[:, 3:7], b["rpm"], c).sum(axis=1)
    assert (h[tags["h_below"]] < c.GND_EFF_H_CLIP).all() and (h[tags["h_at"]] == c.GND_EFF_H_CLIP).all() and (h[tags["h_above"]] > c.GND_EFF_H_CLIP).all()
    assert 0.03 < c.GND_EFF_H_CLIP < 0.05
    lo, hi = rpy[tags["roll_lo"], 0], rpy[tags["roll_hi"], 0]
    assert (np.abs(lo) < np.pi / 2).all() and (np.abs(lo) > np.pi / 2 - 2e-3).all() and (g[tags["roll_lo"]] > 0).all()
    assert (np.abs(hi) > np.pi / 2).all() and (np.abs(hi) < np.pi / 2 + 2e-3).all() and (g[tags["roll_hi"]] == 0).all()
    assert {-1.0, 1.0} == set(np.sign(lo)) == set(np.sign(hi))
    for t, sign in (("pitch_near_p", 1.0), ("pitch_near_m", -1.0)):
        i = tags[t]
        sarg = -O.quat_to_rotmat_bullet(s[i, 3:7])[:, 2, 0]
        assert (np.abs(np.arcsin(np.clip(sarg, -1, 1)) - sign * np.pi / 2) < 1e-3).all()
        assert (rpy[i, 1] == sign * np.pi / 2).all() and (g[i] == 0).all()          # Bullet's gimbal arm: pitch is +-pi/2 exactly, effect off
    i = tags["pitch_5mrad"]
    assert (np.abs(rpy[i, 1]) < np.pi / 2).all() and (np.abs(rpy[i, 1]) > np.pi / 2 - 6e-3).all() and (g[i] > 0).all()
    assert np.isfinite(np.concatenate(X.accelerations(b))).all()
    t = X.tower_batch(model)
    tz, txy = X.pair_geometry(t)
    i = t["tags"]["fifteen_above"]
    assert len(i) >= 4 and ((tz[i] > 0) & (txy[i] < 10)).sum(axis=1).tolist() == [15] * len(i)


@pytest.mark.parametrize("kind", ["rollout_step", "lqr", "omega", "yank", "dslpid", "circle", "cf2x"])
def test_entry_point_loops_are_finite_unsaturated_and_feel_the_effect(kind):
    """the closed loops of the entry-point tests (the CBF loop needs the library's own pole placement and is checked on the GPU alone)"""
    run, plain = X.entry_run(kind), X.entry_run(kind, "dyn")
    assert np.isfinite(run["obs"]).all()
    assert X.limit_fraction(run, O.CF2X if kind == "cf2x" else O.CF2P) <= 0.10
    # 3e-5 x max(1, |x|) is the largest gate any of these loops is held to
    assert X.state_err(run["obs"][-1], plain["obs"][-1]) >= X.FACTOR * X.gate("geo", "float32", run["obs"][-1])
    if kind == "rollout_step":
        R = X.ROLL
        js = list(range(R["first_step"], R["first_step"] + R["n_steps"]))
        assert [j for j in js if j > 0 and j % R["episode_len"] == 0] == [5] and (5 - R["first_step"]) * 3 % 2 == 1     # one reset, after 9 launches
        assert len({j % R["sets"] for j in js}) == R["sets"] and R["n_steps"] > R["slots"]                              # the ring wraps
    if kind == "dslpid":
        tp, tr = X.dsl_targets(X.stacked(*X.ENTRY_SHAPE))
        assert np.abs(tp[0] - tp[1]).min() > 0 and np.array_equal(tp.astype(np.float32).astype(np.float64), tp)


def test_wind_components_are_told_apart():
    assert np.count_nonzero(X.WIND) == 3 and len(set(np.abs(X.WIND))) == 3
    for which, g in (("dyn", 1e-9), ("envfx", None)):
        a, b = X.wind_runs(which), X.wind_runs(which, swapped=True)
        assert np.isfinite(a["obs"]).all() and X.limit_fraction(a) <= 0.10
        if g is None:
            g = X.gate("step", "float64", a["obs"][-1])
        assert X.state_err(a["obs"][-1], b["obs"][-1]) >= X.FACTOR * g
    calm = X.step_loop(X.stacked(7, 5), "dyn_gnd_drag_dw", steps=X.WIND_STEPS)
    plain = X.step_loop(X.stacked(7, 5), "dyn", steps=X.WIND_STEPS, wind=X.WIND)
    a = X.wind_runs("envfx")
    assert X.state_err(a["obs"][-1], calm["obs"][-1]) >= X.FACTOR * X.gate("step", "float64", a["obs"][-1])      # the wind does something there
    assert X.state_err(a["obs"][-1], plain["obs"][-1]) >= X.FACTOR * X.gate("step", "float32", a["obs"][-1])     # and so do the env effects

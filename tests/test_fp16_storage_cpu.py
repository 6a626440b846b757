"""The fp16-storage instantiations of the headline kernels (S = half_t: k_step_geometric, k_rollout_geometric with a log ring and rewriting
one array, k_step, k_rollout_step), run on the host through tests/emul/simt's `simt_headline` executable, against the storage-faithful
float64 model of tests/fp16_oracle.py under its one acceptance rule: |h - u| <= ulp16(u)/2 + 2^-17 max(|u|, m).  No GPU: this pins the
model itself -- renormalised quaternion, one rounding of the state per launch, rows packed from the unrounded registers -- before the GPU
file (tests/test_gpu_fp16_storage.py) judges the device kernels by it.  100 Hz, CF2P, 37 x 7 = 259 drones (a full workgroup, then a wave
of 3 rows: the 8-byte tail of the 40-byte row writer); the forms with a multi-slot ring run 37 x 8 = 296 (every slot 16-byte aligned).

The executable returns the last observation and the final world state (stored + centre): the planes are that minus the centres.  A run of
9 steps is two launches (7 + 2) with the state rounded in between, out of sight: there the model forks (fp16_oracle's docstring).
Needs the built library besides clang++: the executable's input holds the library's default configuration structs (simt._structs), so
run the repository's build first, as for the other tests on the SIMT stand-in."""
import numpy as np
import pytest

from tests import fp16_oracle as F
from tests.emul.simt import simt

pytestmark = pytest.mark.skipif(not simt.available(), reason="no clang++ for the SIMT stand-in")

# form -> (E, D, the launches of the run)
FORMS = {0: (37, 7, [(1,)]), 2: (37, 7, [(1,)]), 3: (37, 8, [(5,)]), 1: (37, 8, [(7,), (7, 2)]), 4: (37, 7, [(7,), (7, 2)])}
CASES = [(form, launches) for form, (_, _, runs) in sorted(FORMS.items()) for launches in runs]


def _plan(form, launches, acts):
    plan, t, a0 = [], 0.0, 0
    for ks in launches:
        plan.append(dict(kind="step" if form in (2, 3) else "geometric", n_steps=ks, t=t, actions=acts, a0=a0))
        for _ in range(ks):
            t += 0.01
        a0 = (a0 + ks) % 3
    return plan


def _model(P, x):
    model = F.Fp16Aviary(x.shape[0], 100, 100)
    model.set_trajectories(P)                              # origin = lem centre = (float)centre, for every form
    model.sync(x)
    return model


def _inputs(E, D, form, launches):
    rng = np.random.default_rng(40 + form)
    n = E * D
    cen = F.draw_centres(rng, E, D)
    P = F.draw_lemniscates(rng, cen)
    acts = F.draw_actions(rng, 3, n)
    x, left = F.sharp_inputs(rng, n, lambda x, idx: _model(P.reshape(-1, 7)[idx], x), _plan(form, launches, acts))
    assert left == 0                                       # (every drone sharp and well conditioned along the whole flight)
    return x, cen.reshape(n, 3), P, acts


@pytest.fixture(scope="module")
def built():
    return simt.build(only=(simt.EXE[4],))


@pytest.mark.parametrize("form,launches", CASES)
def test_emulated_fp16_kernels_obey_the_storage_model(built, form, launches):
    E, D, _ = FORMS[form]
    n, steps = E * D, sum(launches)
    x, cen, P, acts = _inputs(E, D, form, launches)
    world = x.copy()
    world[:, 0:3] += cen                                   # the executable stores (half)(float)(world - centre) and keeps (float)centre
    obs, st, act, err = simt.headline("float16", form, 0.0, P, world.reshape(E, D, 13), steps, actions=acts.reshape(3, E, D, 4))
    assert "ERROR" not in err and "runtime error" not in err, err[-3000:]
    obs, act = obs.reshape(n, 20), act.reshape(n, 4)
    planes = st.reshape(n, 13).copy()
    planes[:, 0:3] -= cen
    planes = F.f16(planes)                                 # (exact: the planes hold fp16 values; this drops the 1e-16 of the round trip)

    model = _model(P, x)
    for j, kw in enumerate(_plan(form, launches, acts)):
        res = model.launch(**kw)
        if j + 1 < len(launches):
            model.commit(fork=True)
    assert model.determined.all()                          # no cap on the candidates: every drone is judged
    print(f"[fp16 storage, host emulation] form {form}, launches {launches}: {model.x.shape[0] if len(launches) > 1 else n} candidate rows for {n} drones")
    F.check_end(obs, planes, res[-1], f"form {form} {launches}")
    if form == 0:                                          # action_out: the unclipped action, rounded once
        F.assert_sharp(res[-1]["act"], 0.0, "action_out")
        F.assert_fp16(act, res[-1]["act"], 0.0, "form 0 action_out")


def test_rule_helpers():
    """ulp16 at the binade edges and below the normal range; the rule's two sides; a fork carries both roundings of a value at a tie"""
    assert F.ulp16(1.0) == 2.0 ** -10 and F.ulp16(0.999) == 2.0 ** -11 and F.ulp16(2.0 ** -14) == 2.0 ** -24 and F.ulp16(0.0) == 2.0 ** -24
    assert F.ulp16(-3.0) == 2.0 ** -9 and F.f16(1.0 + 2.0 ** -11) == 1.0 and F.f16(1.0 + 3 * 2.0 ** -11) == 1.0 + 2.0 ** -9
    u = np.array([[1.0 + 2.0 ** -11 + 2.0 ** -20]])                                      # just past the tie: rounds up
    assert F.excess16(F.f16(u), u, 1.0)[0].max() < 0
    assert F.excess16(np.array([[1.0]]), u, 1.0)[0].max() < 0                            # the other side: within 2^-17
    assert F.excess16(np.array([[1.0 - 2.0 ** -11]]), u, 1.0)[0].max() > 0               # one more unit off: outside
    with pytest.raises(AssertionError):
        F.assert_fp16(np.array([[1.0 + 2.0 ** -9]]), np.array([[1.0 + 2.0 ** -12]]), 1.0, "one unit off")
    with pytest.raises(AssertionError):                                                  # truncation instead of rounding to nearest
        F.assert_fp16(np.array([[1.0]]), np.array([[1.0 + 0.9 * 2.0 ** -10]]), 1.0, "truncated")
    m = F.Fp16Aviary(2)
    m.sync(F.draw_local_states(np.random.default_rng(0), 2))
    m.launch("step", 1, actions=np.zeros((1, 2, 4)))
    x, xm, prev = m._end
    x = F.f16(x)                                                                          # every value on the fp16 grid: no other candidate
    x[1, 0] = 0.5 + 2.0 ** -12 + 2.0 ** -30                                               # but drone 1's p.x, at a rounding boundary
    m._end = (x, xm, prev)
    m.commit(fork=True)
    assert m.x.shape[0] == 3 and list(m.owner) == [0, 1, 1] and sorted(m.x[1:, 0]) == [0.5, 0.5 + 2.0 ** -11]
    assert np.array_equal(m.x[0], x[0]) and np.array_equal(m.x[1, 1:], x[1, 1:]) and np.array_equal(m.x[2, 1:], x[1, 1:])

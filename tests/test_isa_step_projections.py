"""Instruction count of the whole-rollout kernel's step loop (k_rollout_geometric, fp32 / Euler / GeometricControl, rows written every
step) after the controller's triple products became projections and integrate_q took the reduced sine / cosine, counted from a
cross-compile as test_isa_rollout_contract.py extracts the loop.  Static counts of the step loop:

    instantiation      VALU          transcendental (v_rcp / v_rsq / v_sqrt)
    rows in place      779 -> 773    17 (5 / 7 / 5) -> 16 (5 / 6 / 5)
    [T, n, 20] log     803 -> 797    17 (5 / 7 / 5) -> 16 (5 / 6 / 5)

(parent -> this tree).  The projections and the un-normalised b1d take 19 instructions and one v_rsq out of the straight-line code
(760 / 784 by themselves); integrate_q's short path adds 13 static instructions -- the two polynomials a second time, behind a scalar
branch, and the compare that feeds it -- and executes 14 fewer per drone-step (12 in place of the general arm's 27, plus the compare),
so the static figure understates what the change saves: 33 executed instructions per drone-step.  The bounds are the achieved counts
with 2 % slack for compiler noise, and strictly below the parent's.  CPU only."""
import pytest

from tests.test_isa_rollout_contract import OBS_IN_PLACE, OBS_LOG, ROLL, body, isa, meta, step_loop  # noqa: F401  (isa: the module's fixture)
from tests.test_isa_rollout_diet import loop_counts

#             obs: (parent VALU, parent transcendental), (achieved VALU, transcendental)
COUNTS = {OBS_IN_PLACE: ((779, 17), (773, 16)),
          OBS_LOG: ((803, 17), (797, 16))}


@pytest.mark.parametrize("obs", [OBS_IN_PLACE, OBS_LOG])
def test_step_loop_is_below_the_parents_count(isa, obs):
    (p_valu, p_trans), (valu, trans) = COUNTS[obs]
    c = loop_counts(isa, obs)
    print("obs form %d: step loop now %s; parent VALU %d, transcendental %d" % (obs, c, p_valu, p_trans))
    assert c["valu"] <= int(valu * 1.02), c
    assert c["valu"] < p_valu, c
    assert c["trans"] <= 16 < p_trans, c
    assert c["rsq"] <= 6, c                      # b1d's normalisation is gone


@pytest.mark.parametrize("obs", [OBS_IN_PLACE, OBS_LOG])
def test_integrate_q_reaches_its_short_sincos_by_a_scalar_branch(isa, obs):
    """The wave-uniform test of |x| <= 0.75 is one v_cmp into vcc and an s_cbranch_vcc* on it: no exec-mask arm, so a wave whose lanes
    are all small does not execute the general arm's range reduction (one v_rndne_f32 there, and one in the Lemniscate phase and each
    of the two yaw sines that integrate_q has nothing to do with)."""
    name, _ = meta(isa, ROLL % obs)
    loop = step_loop(body(isa, name))
    cmp_ = [k for k, o in enumerate(loop) if o.startswith("v_cmp_nle_f32") and "|" in o]
    assert len(cmp_) == 1, [loop[k] for k in cmp_]
    nxt = [o for o in loop[cmp_[0] + 1:cmp_[0] + 5] if not o.startswith("s_nop")]
    assert any(o.startswith(("s_cbranch_vcc", "s_cbranch_scc")) for o in nxt) and not any("saveexec" in o for o in nxt), nxt
    assert len([o for o in loop if o.startswith("v_rndne_f32")]) == 4

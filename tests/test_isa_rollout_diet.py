"""Instruction diet of the whole-rollout kernel's step loop (k_rollout_geometric, fp32 / Euler / GeometricControl, rows written every
step), counted from a cross-compile as test_isa_rollout_contract.py extracts the loop.  The loop carries one rotation frame per state
(make_frame in csrc/mds_math.hpp): the frame formed for step k's observation row serves step k + 1's controller and rigid-body step,
and the Lemniscate's second reciprocal is an identity of its first.  Static counts of the step loop:

    instantiation      VALU   transcendental (v_rcp / v_rsq / v_sqrt)   f64
    rows in place      864 -> 779      21 (9 / 7 / 5) -> 17 (5 / 7 / 5)      14 -> 14
    [T, n, 20] log     888 -> 803      21 (9 / 7 / 5) -> 17 (5 / 7 / 5)      14 -> 14

(parent -> this tree).  The bounds below are the achieved counts with 2 % slack for compiler noise; the parent's figures stand beside
them as the reference they must stay below.  CPU only."""
import re

import pytest

from tests.test_isa_rollout_contract import OBS_IN_PLACE, OBS_LOG, ROLL, body, isa, meta, step_loop  # noqa: F401  (isa: the module's fixture)

#             obs: (parent VALU, parent transcendental, parent f64), (achieved VALU, transcendental, f64)
COUNTS = {OBS_IN_PLACE: ((864, 21, 14), (779, 17, 14)),
          OBS_LOG: ((888, 21, 14), (803, 17, 14))}
PARENT_RCP = 9


def loop_counts(isa_text, obs):
    name, _ = meta(isa_text, ROLL % obs)
    ops = [o.split()[0] for o in step_loop(body(isa_text, name)) if not o.endswith(":")]
    valu = [o for o in ops if o.startswith("v_")]
    trans = [o for o in valu if re.match(r"v_(rcp|rsq|sqrt|sin|cos|exp|log)_", o)]
    f64 = [o for o in valu if o.endswith("_f64") or "_f64_" in o]
    return dict(valu=len(valu), trans=len(trans), f64=len(f64), rcp=len([o for o in trans if o.startswith("v_rcp")]),
                rsq=len([o for o in trans if o.startswith("v_rsq")]), sqrt=len([o for o in trans if o.startswith("v_sqrt")]))


@pytest.mark.parametrize("obs", [OBS_IN_PLACE, OBS_LOG])
def test_step_loop_is_below_the_parents_instruction_counts(isa, obs):
    (p_valu, p_trans, p_f64), (valu, trans, f64) = COUNTS[obs]
    c = loop_counts(isa, obs)
    print("obs form %d: step loop now %s; parent VALU %d, transcendental %d, f64 %d" % (obs, c, p_valu, p_trans, p_f64))
    assert c["valu"] <= int(valu * 1.02) < p_valu, c
    assert c["trans"] <= trans < p_trans, c
    assert c["f64"] <= f64 <= p_f64, c
    # 2 / |q|^2 once per step (the parent: controller, rigid-body step and observation each formed it), the Lemniscate's 1 / (1 + sin^2),
    # and what the atan2 bodies need
    assert c["rcp"] <= PARENT_RCP - 3, c

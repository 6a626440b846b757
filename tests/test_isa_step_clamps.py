"""Instruction count of the whole-rollout kernel's step loop (k_rollout_geometric, fp32 / Euler / GeometricControl, rows written every
step) after the clamps became medians, rotor_wrench's airframe test a scalar branch ahead of the substeps, and the products of
constants moved to the host, counted from a cross-compile as test_isa_rollout_contract.py extracts the loop.  Static counts of the
step loop:

    instantiation      VALU          v_cndmask    s_nop    v_med3_f32
    rows in place      777 -> 746    45 -> 31     27 -> 20      0 -> 8
    [T, n, 20] log     801 -> 770    45 -> 31     28 -> 21      0 -> 8

(parent -> this tree).  The eight clamps of a step -- four motor thrusts in input_to_action, four RPM in aviary_step -- were two
compares and two selects each, with three copies of the bounds into VGPRs for the selects to read; each is one v_med3_f32 now (the
thrust clamp's upper bound is copied once for the four: a VOP3 instruction reads one SGPR).  The static figure counts both arms of
rotor_wrench (7 instructions for the X frame, 5 for the + frame); a handle executes one of them, where the parent executed both and
two selects.  The bounds are the achieved counts with 2 % slack for compiler noise, and strictly below the parent's.  CPU only."""
import re

import pytest

from tests.test_isa_rollout_contract import OBS_IN_PLACE, OBS_LOG, ROLL, body, isa, meta, step_loop  # noqa: F401  (isa: the module's fixture)
from tests.test_isa_rollout_diet import loop_counts

#             obs: (parent VALU, parent v_cndmask), (achieved VALU, v_cndmask)
COUNTS = {OBS_IN_PLACE: ((777, 45), (746, 31)),
          OBS_LOG: ((801, 45), (770, 31))}


def loop_of(isa_text, obs):
    name, _ = meta(isa_text, ROLL % obs)
    return [o for o in step_loop(body(isa_text, name)) if not o.endswith(":")]


def operands(op):
    return [a.strip() for a in op.split(None, 1)[1].split(",")] if " " in op else []


def reads(op, reg):
    """op reads the VGPR reg (as a whole operand, with or without a sign or an absolute value)"""
    return any(re.fullmatch(r"-?\|?" + reg + r"\|?", a) for a in operands(op)[1:])


@pytest.mark.parametrize("obs", [OBS_IN_PLACE, OBS_LOG])
def test_step_loop_is_below_the_parents_count(isa, obs):
    (p_valu, p_cnd), (valu, cnd) = COUNTS[obs]
    c = loop_counts(isa, obs)
    n_cnd = len([o for o in loop_of(isa, obs) if o.startswith("v_cndmask")])
    print("obs form %d: step loop now %s, v_cndmask %d; parent VALU %d, v_cndmask %d" % (obs, c, n_cnd, p_valu, p_cnd))
    assert c["valu"] <= int(valu * 1.02), c
    assert c["valu"] < p_valu, c                 # (777 rows in place)
    assert n_cnd <= cnd < 45, n_cnd


@pytest.mark.parametrize("obs", [OBS_IN_PLACE, OBS_LOG])
def test_the_clamps_are_medians_and_no_bound_is_copied_for_a_select(isa, obs):
    loop = loop_of(isa, obs)
    med = [o for o in loop if o.startswith(("v_med3_f32", "v_min_f32"))]
    assert len(med) >= 8, med
    # a copy of an SGPR into a VGPR whose readers, up to the register's next definition, are all v_cndmask: the bound of a select
    for k, o in enumerate(loop):
        m = re.fullmatch(r"v_mov_b32(?:_e32)? (v\d+), s\d+", o)
        if not m:
            continue
        users = []
        for later in loop[k + 1:]:
            if reads(later, m.group(1)):
                users.append(later)
            if later.startswith("v_") and operands(later)[0] == m.group(1):
                break
        assert not users or not all(u.startswith("v_cndmask") for u in users), (o, users)


@pytest.mark.parametrize("obs", [OBS_IN_PLACE, OBS_LOG])
def test_the_airframe_is_a_scalar_branch(isa, obs):
    """c.cf2x is the one flag the loop compares with 0: the compare feeds an s_cbranch_scc*, not an s_cselect of a mask for v_cndmask."""
    loop = loop_of(isa, obs)
    flag = [k for k, o in enumerate(loop) if re.fullmatch(r"s_cmp_(eq|lg)_u32 s\d+, 0", o)]
    assert len(flag) == 1, [loop[k] for k in flag]
    after = loop[flag[0] + 1:flag[0] + 6]
    br = [k for k, o in enumerate(after) if o.startswith("s_cbranch_scc")]
    assert br, after
    assert not [o for o in after[:br[0]] if o.startswith(("s_cselect", "v_cndmask"))], after

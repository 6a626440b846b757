"""Bookkeeping of the whole-rollout kernel's step loop (k_rollout_geometric, fp32 / Euler / GeometricControl, rows written every step),
counted from the cross-compile of test_isa_rollout_contract.py.  The step body runs on whole waves (the lanes past the last drone fly
a copy of drone n - 1 and store nothing), so there is no exec-mask region around it and no copies of q and v into the row at its
join; the row writer's two per-lane offsets are formed once before the loop and its wave index on the scalar side; the double copies
of omega and phase_shift are held.  Static counts of the step loop, parent -> this tree:

    instantiation      VALU          VGPRs      v_mov_b32    v_mul_lo_u32
    rows in place      746 -> 725    79 -> 76   31 -> 21     1 -> 0
    [T, n, 20] log     770 -> 739    79 -> 80   32 -> 21     2 -> 0

The bounds are the achieved counts (VALU with 2 % slack for compiler noise); the parent's VALU counts stand beside them as what they
must stay strictly below.  CPU only."""
import collections

import pytest

from tests.test_isa_rollout_contract import OBS_IN_PLACE, OBS_LOG, ROLL, body, isa, meta, step_loop  # noqa: F401  (isa: the module's fixture)

#             obs: parent VALU, (achieved VALU, VGPRs, v_mov_b32)
COUNTS = {OBS_IN_PLACE: (746, (725, 76, 21)),
          OBS_LOG: (770, (739, 80, 21))}


def loop_ops(isa_text, obs):
    name, m = meta(isa_text, ROLL % obs)
    ops = collections.Counter(o.split()[0] for o in step_loop(body(isa_text, name)) if not o.endswith(":"))
    return m, ops


@pytest.mark.parametrize("obs", [OBS_IN_PLACE, OBS_LOG])
def test_step_loop_bookkeeping_is_off_the_valu(isa, obs):
    p_valu, (valu, vgprs, movs) = COUNTS[obs]
    m, ops = loop_ops(isa, obs)
    n_valu = sum(v for k, v in ops.items() if k.startswith("v_"))
    n_mov = sum(v for k, v in ops.items() if k.startswith("v_mov_b32"))
    print("obs form %d: step loop VALU %d (parent %d), VGPRs %d, v_mov_b32 %d, v_mul_lo_u32 %d, v_add_f64 %d"
          % (obs, n_valu, p_valu, m["vgpr_count"], n_mov, ops["v_mul_lo_u32"], ops["v_add_f64"]))
    assert n_valu <= int(valu * 1.02) < p_valu, n_valu
    assert m["vgpr_count"] <= vgprs, m
    assert n_mov <= movs, n_mov
    assert ops["v_mul_lo_u32"] == 0                                  # the wave's LDS slice: a scalar multiply, once
    # the row writer's hot arm forms no address on the vector side: the five 16-byte stores of a full wave take a scalar base and the
    # carried 32-bit lane offset, and nothing in the loop divides the thread index
    assert ops["v_mad_u32_u24"] == 0 and ops["v_ashrrev_i32_e32"] == 0, ops

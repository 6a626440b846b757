"""The yaw-free whole-rollout kernels (k_rollout_geometric_y0: what a handle whose Lemniscates all have yaw_rate = 0 launches), checked
from the same cross-compile as the general ones (helpers of tests/test_isa_rollout_contract.py).

For the fp32 / Euler / no-drag instantiations that write rows every step (in place: the bench's headline; log: one slot per step):
  * the budget of the general kernel holds: at most 80 VGPRs (6 waves per SIMD), no scratch, no spilled SGPRs;
  * the step loop has strictly fewer VALU instructions than the general kernel's from the same compile;
  * no v_mul_f32 by an inline 0 is left in it (the general loop multiplies by the literal zeros des.v.z, b1c.z, ... : x * 0 may
    not be folded by the compiler, the yaw-free form does not write it).

Counts at the time of writing (VGPRs / instructions of the step loop / VALU instructions of the step loop):
  in place   general 76 / 927 / 725     yaw-free 70 / 805 / 614
  log        general 80 / 1047 / 739    yaw-free 78 / 920 / 626
The static difference (111 VALU) includes the two sincos expansions of the yaw that the general loop carries and skips at run time
(lemniscate_local's and the controller's); executed, the loop goes from 533.5 to 484.5 wave-instructions per drone-step
(profiles/r09_yaw_free_pmc.json).  CPU only."""
import re

import pytest

from tests.test_isa_rollout_contract import OBS_IN_PLACE, OBS_LOG, ROLL, body, isa, meta, step_loop  # noqa: F401  (isa: the fixture)

# <float, float, RK4 = false, DRAG = false, COMP = 0, OBS>
ROLL_Y0 = r"_ZN3mds22k_rollout_geometric_y0IffLb0ELb0ELi0ELi%dEEEv\S+"


def valu(ops):
    return [o for o in ops if o.startswith("v_") and not o.startswith(("v_readlane", "v_writelane"))]


@pytest.mark.parametrize("obs", [OBS_IN_PLACE, OBS_LOG])
def test_yaw_free_rollout_kernel_keeps_the_budget_and_drops_the_zero_products(isa, obs):
    name, m = meta(isa, ROLL_Y0 % obs)
    gname, gm = meta(isa, ROLL % obs)
    loop, gloop = step_loop(body(isa, name)), step_loop(body(isa, gname))
    print(f"obs {obs}: general {gm['vgpr_count']} VGPRs / {len(gloop)} / {len(valu(gloop))} VALU, "
          f"yaw-free {m['vgpr_count']} VGPRs / {len(loop)} / {len(valu(loop))} VALU")
    assert m["vgpr_count"] <= 80, m                  # 6 waves per SIMD
    assert m["private_segment_fixed_size"] == 0 and m["sgpr_spill_count"] == 0 and m["vgpr_spill_count"] == 0, m
    ops = body(isa, name)
    assert not [o for o in ops if o.startswith("scratch_") or "v_accvgpr" in o]
    assert not [o for o in ops if "v_writelane" in o or "v_readlane" in o]
    assert len(valu(loop)) < len(valu(gloop)), (len(valu(loop)), len(valu(gloop)))
    zero_mul = [o for o in loop if re.match(r"v_mul_f32\S*\s+v\d+, (0|0x80000000), ", o) or re.match(r"v_mul_f32\S*\s+v\d+, \S+, (0|0x80000000)$", o)]
    assert not zero_mul, zero_mul
    # (the general loop does have them: the check above looks at the right thing)
    assert [o for o in gloop if re.match(r"v_mul_f32\S*\s+v\d+, 0, ", o)]


def test_the_other_yaw_free_instantiations_do_not_spill(isa):
    """The handle flag is followed by every dtype / integrator / drag instantiation of GeometricControl's loop and of the fused step:
    each has its yaw-free entry point, and those with fp32 arithmetic (the ones tests/test_isa_rollout_contract.py holds the general
    kernels to) none with scratch.  (The float64 RK4 loop, at 308 VGPRs, is left to the allocator as the general one is.)"""
    kern = isa[isa.index("amdhsa.kernels:"):]
    assert len(re.findall(r"\.name:\s+_ZN3mds22k_rollout_geometric_y0Id", kern)) >= 4
    for pat, least in ((r"_ZN3mds22k_rollout_geometric_y0If", 8), (r"_ZN3mds19k_step_geometric_y0If", 32)):
        blocks = [b for b in kern.split("\n  - ") if re.search(r"\.name:\s+" + pat, b)]
        print(pat, len(blocks))
        assert len(blocks) >= least, (pat, len(blocks))
        for b in blocks:
            assert int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", b).group(1)) == 0, re.search(r"\.name:\s+(\S+)", b).group(1)

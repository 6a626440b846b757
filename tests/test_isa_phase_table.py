"""The whole-rollout kernel that reads sin / cos of the Lemniscate phase from the handle's table (k_rollout_geometric_y0p: what a yaw-free
handle whose phases repeat from wave to wave launches, csrc/mds_kernels.hip TAB), checked from a cross-compile beside the yaw-free
kernel it stands in for (k_rollout_geometric_y0) from the same compile.  For the fp32 / Euler / no-drag instantiations that write rows
every step:

  * 6 waves per SIMD (<= 80 VGPRs), no scratch, no spills;
  * the step loop forms no time and no phase: no float64 VALU instruction and no v_readfirstlane_b32;
  * the pair of a step is ONE 8-byte load, and the loop loads nothing else from global memory;
  * at least 30 VALU instructions fewer in the loop than the yaw-free kernel's (its phase block is 38: the round trip of t through
    SGPRs, the double reduction, the Cody-Waite step, two polynomials and the quadrant selects).
CPU only."""
import re

import pytest

from tests.test_isa_rollout_contract import OBS_IN_PLACE, OBS_LOG, body, isa, meta, step_loop  # noqa: F401  (isa: the cross-compile fixture)

# <float, float, RK4 = false, DRAG = false, COMP = 0, OBS>
ROLL_Y0 = r"_ZN3mds22k_rollout_geometric_y0IffLb0ELb0ELi0ELi%dEEEv\S+"
ROLL_Y0P = r"_ZN3mds23k_rollout_geometric_y0pIffLb0ELb0ELi0ELi%dEEEv\S+"


def valu(ops):
    return [o for o in ops if o.startswith("v_")]


@pytest.mark.parametrize("obs", [OBS_IN_PLACE, OBS_LOG])
def test_table_kernel_fits_six_waves_without_spills(isa, obs):
    name, m = meta(isa, ROLL_Y0P % obs)
    print(name, m)
    assert m["vgpr_count"] <= 80, m
    assert m["private_segment_fixed_size"] == 0 and m["sgpr_spill_count"] == 0 and m["vgpr_spill_count"] == 0, m
    assert not [o for o in body(isa, name) if o.startswith("scratch_") or "v_accvgpr" in o]


@pytest.mark.parametrize("obs", [OBS_IN_PLACE, OBS_LOG])
def test_step_loop_reads_the_pair_and_forms_no_phase(isa, obs):
    name, _ = meta(isa, ROLL_Y0P % obs)
    loop = step_loop(body(isa, name))
    f64 = [o for o in valu(loop) if re.match(r"v_\w+_f64\b", o.split()[0])]
    assert not f64, f64
    assert not [o for o in loop if o.startswith("v_readfirstlane_b32")]
    loads = [o for o in loop if o.startswith(("global_load", "flat_load", "buffer_load"))]
    print(obs, loads)
    assert len(loads) == 1 and loads[0].startswith("global_load_dwordx2"), loads
    # scalar base (an SGPR pair) + the lane's 32-bit offset, default cache policy: every wave reads the same row
    assert re.match(r"global_load_dwordx2 v\[\d+:\d+\], v\d+, s\[\d+:\d+\]$", loads[0]), loads[0]


@pytest.mark.parametrize("obs", [OBS_IN_PLACE, OBS_LOG])
def test_the_pair_is_waited_for_ahead_of_the_row_stores(isa, obs):
    """Loads and stores share vmcnt, and the compiler can only wait for the pair with vmcnt(0).  The one such wait of the loop stands
    behind the load and ahead of the step's first store: there it finds the load, a step's arithmetic old, and the stores of the step
    before.  Anywhere from the stores to the pair's first use at the top of the next step it would sit out the stores just issued
    (measured: the default line -0.9 % instead of -4.5 %, and +7 % where a SIMD holds one wave).  No value loaded ahead of the loop may
    bring a wait of its own into it either."""
    name, _ = meta(isa, ROLL_Y0P % obs)
    loop = step_loop(body(isa, name))
    load = [k for k, o in enumerate(loop) if o.startswith("global_load")]
    stores = [k for k, o in enumerate(loop) if o.startswith("global_store")]
    waits = [k for k, o in enumerate(loop) if o.startswith("s_waitcnt") and "vmcnt" in o]
    print(obs, load, waits, stores[:1], [loop[k] for k in waits])
    assert len(load) == 1 and stores
    assert len(waits) == 1 and load[0] < waits[0] < stores[0], (load, waits, stores[0])
    # ... and the registers the load writes are not read between the load and that wait (the pair's uses are all ahead of the load)
    dst = re.match(r"global_load_dwordx2 v\[(\d+):(\d+)\]", loop[load[0]])
    regs = {f"v{dst.group(1)}", f"v{dst.group(2)}"}
    early = [o for o in loop[load[0] + 1:waits[0]] if regs & set(re.findall(r"v\d+", o))]
    assert not early, early


@pytest.mark.parametrize("obs", [OBS_IN_PLACE, OBS_LOG])
def test_step_loop_is_at_least_thirty_valu_instructions_shorter(isa, obs):
    y0, _ = meta(isa, ROLL_Y0 % obs)
    y0p, _ = meta(isa, ROLL_Y0P % obs)
    a, b = len(valu(step_loop(body(isa, y0)))), len(valu(step_loop(body(isa, y0p))))
    print(f"OBS {obs}: VALU in the step loop, yaw-free {a}, with the table {b} ({b - a:+d})")
    assert b <= a - 30, (a, b)

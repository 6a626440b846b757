"""The whole-rollout kernel that reads what the controller needs of the desired state from the handle's table (k_rollout_geometric_y0d:
what a yaw-free handle whose a, omega and phase_shift repeat from wave to wave launches, csrc/mds_kernels.hip TAB 2), checked from a
cross-compile beside the kernel it stands in for (k_rollout_geometric_y0p) from the same compile.  For the fp32 / Euler / no-drag
instantiations that write rows every step:

  * 6 waves per SIMD (<= 80 VGPRs), no scratch, no spills;
  * no float64 VALU instruction and no v_readfirstlane_b32 in the step loop;
  * the loop's only global loads are the row's two 16-byte loads, scalar base + the lane's 32-bit offset, default cache policy;
  * exactly one vmcnt wait, behind those loads and ahead of the step's first row store, and the loaded registers are not read in between;
  * at least 30 VALU instructions fewer in the loop than the pair-table kernel's, one of them a v_rcp_f32.
CPU only."""
import re

import pytest

from tests.test_isa_rollout_contract import OBS_IN_PLACE, OBS_LOG, body, isa, meta, step_loop  # noqa: F401  (isa: the cross-compile fixture)

# <float, float, RK4 = false, DRAG = false, COMP = 0, OBS>
ROLL_Y0P = r"_ZN3mds23k_rollout_geometric_y0pIffLb0ELb0ELi0ELi%dEEEv\S+"
ROLL_Y0D = r"_ZN3mds23k_rollout_geometric_y0dIffLb0ELb0ELi0ELi%dEEEv\S+"


def valu(ops):
    return [o for o in ops if o.startswith("v_")]


def loop_of(isa, pattern, obs):
    name, _ = meta(isa, pattern % obs)
    return step_loop(body(isa, name))


@pytest.mark.parametrize("obs", [OBS_IN_PLACE, OBS_LOG])
def test_desired_table_kernel_fits_six_waves_without_spills(isa, obs):
    name, m = meta(isa, ROLL_Y0D % obs)
    print(name, m)
    assert m["vgpr_count"] <= 80, m
    assert m["private_segment_fixed_size"] == 0 and m["sgpr_spill_count"] == 0 and m["vgpr_spill_count"] == 0, m
    assert not [o for o in body(isa, name) if o.startswith("scratch_") or "v_accvgpr" in o]


@pytest.mark.parametrize("obs", [OBS_IN_PLACE, OBS_LOG])
def test_step_loop_reads_the_row_and_forms_no_time(isa, obs):
    loop = loop_of(isa, ROLL_Y0D, obs)
    f64 = [o for o in valu(loop) if re.match(r"v_\w+_f64\b", o.split()[0])]
    assert not f64, f64
    assert not [o for o in loop if o.startswith("v_readfirstlane_b32")]
    loads = [o for o in loop if o.startswith(("global_load", "flat_load", "buffer_load"))]
    print(obs, loads)
    assert len(loads) == 2, loads
    # scalar base (an SGPR pair) + the lane's 32-bit offset, the second group 64 x 16 bytes behind the first, default cache policy
    m = [re.match(r"global_load_dwordx4 v\[\d+:\d+\], (v\d+), (s\[\d+:\d+\])( offset:1024)?$", o) for o in loads]
    assert all(m), loads
    assert m[0].group(1) == m[1].group(1) and m[0].group(2) == m[1].group(2), loads
    assert sorted(bool(x.group(3)) for x in m) == [False, True], loads


@pytest.mark.parametrize("obs", [OBS_IN_PLACE, OBS_LOG])
def test_the_row_is_waited_for_once_ahead_of_the_row_stores(isa, obs):
    """Loads and stores share vmcnt: the one wait of the loop stands behind the two loads and ahead of the step's first store, where it
    finds the loads a step's arithmetic old and the stores of the step before (tests/test_isa_phase_table.py has the measurement)."""
    loop = loop_of(isa, ROLL_Y0D, obs)
    load = [k for k, o in enumerate(loop) if o.startswith("global_load")]
    stores = [k for k, o in enumerate(loop) if o.startswith("global_store")]
    waits = [k for k, o in enumerate(loop) if o.startswith("s_waitcnt") and "vmcnt" in o]
    print(obs, load, waits, stores[:1], [loop[k] for k in waits])
    assert len(load) == 2 and stores
    assert len(waits) == 1 and max(load) < waits[0] < stores[0], (load, waits, stores[0])
    # ... and the registers the loads write are not read between the loads and that wait
    regs = set()
    for k in load:
        lo, hi = map(int, re.match(r"global_load_dwordx4 v\[(\d+):(\d+)\]", loop[k]).groups())
        regs |= {f"v{r}" for r in range(lo, hi + 1)}
    assert len(regs) == 8

    def names(op):
        out = set(re.findall(r"\bv(\d+)\b", op))
        for lo, hi in re.findall(r"v\[(\d+):(\d+)\]", op):
            out |= {str(r) for r in range(int(lo), int(hi) + 1)}
        return {"v" + r for r in out}

    early = [o for k, o in enumerate(loop[min(load) + 1:waits[0]], min(load) + 1) if k not in load and regs & names(o)]
    assert not early, early


@pytest.mark.parametrize("obs", [OBS_IN_PLACE, OBS_LOG])
def test_step_loop_is_thirty_valu_instructions_and_one_reciprocal_shorter(isa, obs):
    y0p, y0d = loop_of(isa, ROLL_Y0P, obs), loop_of(isa, ROLL_Y0D, obs)
    a, b = len(valu(y0p)), len(valu(y0d))
    ra, rb = (len([o for o in l if o.startswith("v_rcp_f32")]) for l in (y0p, y0d))
    print(f"OBS {obs}: VALU in the step loop, pair table {a}, desired-state table {b} ({b - a:+d}); v_rcp_f32 {ra} -> {rb}")
    assert b <= a - 30, (a, b)
    assert rb == ra - 1, (ra, rb)

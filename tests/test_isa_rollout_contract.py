"""Register budget of the whole-rollout kernel (k_rollout_geometric, the bench's headline in launch form 2), checked from a cross-compile.
The fp32 / Euler / no-drag / GeometricControl instantiations that write rows every step must stay within 80 VGPRs (6 waves per SIMD on
gfx950: 512 registers per lane and SIMD, granule 8) without scratch or spilled SGPRs, and store the rows with the policy of their
destination.  Before the kernel took the compensated storage and the rows' destination as template arguments and stopped carrying its
loop invariants it stood at 125 VGPRs / 106 SGPRs with 4 SGPR spills (4 waves); it is at 71 / 87 / 0 ("The register diet").
CPU only."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# <float, float, RK4 = false, DRAG = false, CTRL = 0, COMP = 0, OBS>
ROLL = r"_ZN3mds19k_rollout_geometricIffLb0ELb0ELi0ELi0ELi%dEEEv\S+"
OBS_LAST, OBS_IN_PLACE, OBS_LOG = 0, 1, 2


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not available")
    d = tmp_path_factory.mktemp("isa_rollout")
    import sys
    sys.path.insert(0, ROOT)
    from __graft_entry__ import HIPCC_FLAGS
    # the rollout entry points live in translation unit 1 (MDS_PART in csrc/mds_api.hip)
    subprocess.check_call(["hipcc", *HIPCC_FLAGS, "-DMDS_PART=1", "-S", "--cuda-device-only", "-o", str(d / "mds1.s"),
                           os.path.join(ROOT, "multidronesim_amd", "csrc", "mds_api.hip")], stderr=subprocess.DEVNULL)
    return open(d / "mds1.s").read()


def meta(isa, pattern):
    names = sorted({m.group(1) for m in re.finditer(r"\.name:\s+(" + pattern + r")\n", isa)})
    assert len(names) == 1, names
    blk = next(b for b in isa[isa.index("amdhsa.kernels:"):].split("\n  - ") if re.search(r"\.name:\s+" + re.escape(names[0]) + r"\n", b))
    return names[0], {k: int(re.search(r"\." + k + r":\s+(\d+)", blk).group(1))
                      for k in ("vgpr_count", "sgpr_count", "sgpr_spill_count", "vgpr_spill_count", "private_segment_fixed_size")}


def body(isa, mangled):
    i = isa.index("\n" + mangled + ":")
    j = isa.index("s_endpgm", i)
    lines = [l.strip() for l in isa[i:j].split("\n")]
    return [l.split(";")[0].strip() for l in lines if l and (re.match(r"\.LBB\w+:", l) or not l.startswith((";", "//", ".")))]      # (block labels kept)


def step_loop(ops):
    """The instructions of the outermost loop: from its header label to its last backward branch."""
    labels = {o[:-1]: k for k, o in enumerate(ops) if o.endswith(":")}
    back = [(labels[o.split()[-1]], k) for k, o in enumerate(ops)
            if o.startswith(("s_cbranch", "s_branch")) and o.split()[-1] in labels and labels[o.split()[-1]] < k]
    assert back
    head = min(h for h, _ in back)
    return ops[head:max(k for h, k in back if h >= head) + 1]


@pytest.mark.parametrize("obs", [OBS_IN_PLACE, OBS_LOG])
def test_rollout_kernel_fits_six_waves_without_spills(isa, obs):
    name, m = meta(isa, ROLL % obs)
    print(name, m)
    assert m["vgpr_count"] <= 80, m                  # 6 waves per SIMD (the required minimum, 96 = 5 waves, is implied)
    assert m["private_segment_fixed_size"] == 0 and m["sgpr_spill_count"] == 0 and m["vgpr_spill_count"] == 0, m
    ops = body(isa, name)
    assert not [o for o in ops if o.startswith("scratch_") or "v_accvgpr" in o]
    assert not [o for o in ops if "v_writelane" in o or "v_readlane" in o]          # no SGPR parked in a VGPR lane


def test_rollout_kernel_writes_each_steps_rows_once_with_the_policy_of_its_destination(isa):
    """Each expansion of write_obs_rows is five 16-byte LDS writes per lane, five 16-byte stores for a full wave and five more, always
    non-temporal, in the chunk-by-chunk drain of the shard's last, partial wave.  In place (the rows rewritten every step) there is ONE
    expansion and its full-wave stores carry the default policy; the log form has two -- step k's slot, and the copy of the last
    step's rows to obs_last -- and every store of both is non-temporal."""
    for obs, writes, plain, nt in ((OBS_IN_PLACE, 5, 5, 5), (OBS_LOG, 10, 0, 20)):
        name, _ = meta(isa, ROLL % obs)
        loop = step_loop(body(isa, name))
        st = [o for o in loop if o.startswith("global_store_dwordx4")]
        print(obs, len(loop), len(st))
        assert len([o for o in loop if o.startswith("ds_write_b128")]) == writes, (obs, name)
        assert len([o for o in st if not o.endswith(" nt")]) == plain, (obs, st)
        assert len([o for o in st if o.endswith(" nt")]) == nt, (obs, st)
        # the state stays in registers: nothing else is stored 16 bytes wide inside the loop, and no state group is loaded there
        assert not [o for o in loop if o.startswith("global_load_dwordx4")], obs


def test_the_other_rollout_instantiations_do_not_spill(isa):
    """The last-step-only form and the run-time-dispatched fp32 forms (RK4, drag, compensated storage, the LQR family) are left to the
    allocator: they must not pay for the headline's budget with scratch."""
    _, m = meta(isa, ROLL % OBS_LAST)
    assert m["vgpr_count"] <= 96 and m["private_segment_fixed_size"] == 0 and m["sgpr_spill_count"] == 0, m
    blocks = [b for b in isa[isa.index("amdhsa.kernels:"):].split("\n  - ") if re.search(r"\.name:\s+_ZN3mds(19k_rollout_geometric|14k_rollout_traj)If", b)]
    assert len(blocks) >= 20
    for b in blocks:
        name = re.search(r"\.name:\s+(\S+)", b).group(1)
        assert int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", b).group(1)) == 0, name

"""FedCE / dLQR without a device: the C-ABI entry points validate before touching the device, the two new kernels carry no
scratch in their f32 / f64 Euler instantiations, and the NumPy oracle (tests/fedce_oracle.py) keeps the reference's quirks."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from multidronesim_amd import _capi as capi
from oracle import np_oracle as O
from tests import fedce_oracle as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return capi.load_library()


def test_null_handle_returns_einval(lib):
    assert lib.mds_fedce_supported(None) == capi.MDS_OK - 1
    assert lib.mds_fedce_init(None, None, None) == -1
    assert lib.mds_fedce_get(None, None, None) == -1
    assert lib.mds_fedce_set(None, None, None) == -1
    assert lib.mds_fedce_identify(None, 5, None, 0, None, 1, None, None, None, None, None) == -1
    assert lib.mds_set_dlqr_gain(None, None) == -1
    assert lib.mds_dlqr_compute(None, None, None, None, None, None) == -1
    assert lib.mds_rollout_dlqr_fused(None, 0.0, 5, None, None, None) == -1


@pytest.mark.parametrize("mut,ok", [(dict(), True), (dict(dtype=capi.MDS_F64), True), (dict(physics=capi.MDS_PHYSICS_DYN_DRAG), True),
                                    (dict(num_drones=1), True), (dict(num_drones=16), True),
                                    (dict(num_drones=17), False), (dict(dtype=capi.MDS_F16), False), (dict(dtype=capi.MDS_F32C), False),
                                    (dict(integrator=capi.MDS_INTEGRATOR_RK4), False), (dict(physics=capi.MDS_PHYSICS_DYN_DW), False)])
def test_supported_configurations(lib, mut, ok):
    cfg = capi.MdsConfig()
    lib.mds_default_config(capi.MDS_CF2P, C.byref(cfg))
    for k, v in mut.items():
        setattr(cfg, k, v)
    rc = lib.mds_fedce_supported(C.byref(cfg))
    assert rc == (capi.MDS_OK if ok else -6)
    if not ok:
        assert lib.mds_last_error() != b""


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not available")
    import sys
    sys.path.insert(0, ROOT)
    from __graft_entry__ import HIPCC_FLAGS
    out = tmp_path_factory.mktemp("isa") / "mds2.s"
    subprocess.check_call(["hipcc", *HIPCC_FLAGS, "-DMDS_PART=2", "-S", "--cuda-device-only", "-o", str(out),
                           os.path.join(ROOT, "multidronesim_amd", "csrc", "mds_api.hip")], stderr=subprocess.DEVNULL)
    return open(out).read()


def test_fedce_kernels_have_no_scratch(isa):
    meta = isa[isa.index("amdhsa.kernels:"):]
    seen = set()
    for blk in meta.split("\n  - "):
        m = re.search(r"\.name:\s+(\S+)\n", blk)
        if not m or not re.match(r"_ZN3mds(16k_fedce_identify|14k_dlqr_rollout)I(ff|dd)", m.group(1)):
            continue
        seen.add(m.group(1))
        assert int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1)) == 0, m.group(1)
        assert int(re.search(r"\.vgpr_count:\s+(\d+)", blk).group(1)) <= 512, m.group(1)
    assert len(seen) == 8, seen          # (identify | rollout) x (float | double) x (DYN | DYN_DRAG), Euler


@pytest.mark.parametrize("D", [2, 3])
def test_oracle_reproduces_the_reference_in_the_loop(golden_dir, D):
    """tests/fedce_oracle.py against the reference's own DecentralizedLQR driven through fedCE_iteration's call sequence
    (tests/golden/mint_fedce.py), given the same noise draws: theta, P, K of every iteration, pred_errors, pred_thetas and every
    observation to 1e-10 relative."""
    d = np.load(os.path.join(golden_dir, "fedce_ref_in_loop.npz"))
    g, noise, num_iter = F.fixture_case(d, D)
    ora = F.FedCE(g["xyz"], g["rpy"], g["target_pos"], g["target_rpy"], wind=float(d["wind"])).run(num_iter, noise)

    def rel(a, b):
        return np.abs(np.asarray(a) - b).max() / np.abs(b).max()
    for n in range(num_iter):
        assert rel(ora.thetas[n], g["thetas"][n]) < 1e-10, n
        assert rel(ora.Ps[n], g["Ps"][n]) < 1e-10, n
        assert rel(ora.Ks[n], g["Ks"][n]) < 1e-10, n
    assert rel(ora.dlqr.pred_errors, g["pred_errors"]) < 1e-10
    assert rel(ora.dlqr.pred_thetas, g["pred_thetas"]) < 1e-10
    np.testing.assert_allclose(np.array(ora.obs_log), g["obs_log"], rtol=1e-10, atol=1e-12)


def test_oracle_loop_quirks():
    """D = 1: no step ever updates (the wind loop's `i` is 0)."""
    np.random.seed(3)
    noise = F.draw_reference_noise(3, 1)
    f1 = F.FedCE(np.zeros((1, 3)), np.zeros((1, 3)), [[0, 0, 1]], [[0, 0, np.pi / 2]]).run(3, noise)
    assert all(np.array_equal(th, f1.thetas[0]) for th in f1.thetas) and f1.dlqr.pred_errors == [[], []]

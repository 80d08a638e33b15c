"""The dynamics-output entry points exist with the documented signatures, sim.py's constants match the
header, and a NULL batch is rejected (CPU: no device is touched)."""
import ctypes as C
import re

from conftest import ROOT
from mujoco_ros2_simulation_amd import sim

MRS_ERR_INVALID = -1
HEADER = (ROOT / "include" / "mrs.h").read_text()


def test_header_declarations():
    for decl in ("int mrs_batch_set_jac_sites(mrs_batch* b, const int* site_ids, int n);",
                 "int mrs_batch_dyn_dim(const mrs_batch* b, int which);",
                 "float* mrs_batch_dyn_device_ptr(mrs_batch* b, int which);",
                 "int mrs_batch_get_dyn(mrs_batch* b, int which, double* host, int env0, int n);"):
        assert decl in HEADER, decl


def test_constants_match_header():
    enum = dict(re.findall(r"MRS_DYNOUT_(\w+) = (\d+)", HEADER))
    assert {k: int(v) for k, v in enum.items()} == {"QFRC_BIAS": sim.DYNOUT_QFRC_BIAS, "MASS_MATRIX": sim.DYNOUT_MASS_MATRIX,
                                                    "SITE_JAC": sim.DYNOUT_SITE_JAC, "SITE_POSE": sim.DYNOUT_SITE_POSE,
                                                    "COUNT": sim.DYNOUT_COUNT}
    assert [sim.DYNOUT_QFRC_BIAS, sim.DYNOUT_MASS_MATRIX, sim.DYNOUT_SITE_JAC, sim.DYNOUT_SITE_POSE, sim.DYNOUT_COUNT] == [0, 1, 2, 3, 4]
    assert int(re.search(r"#define MRS_MAX_JAC_SITES (\d+)", HEADER).group(1)) == sim.MAX_JAC_SITES == 16
    assert sim.LAYOUT_DYN_KEYS == ["dyn_outputs"]


def test_entry_points_and_null_batch():
    L = sim.lib()
    for name in ("mrs_batch_set_jac_sites", "mrs_batch_dyn_dim", "mrs_batch_dyn_device_ptr", "mrs_batch_get_dyn"):
        assert hasattr(L, name), name
    assert L.mrs_batch_dyn_device_ptr.restype is C.c_void_p
    buf = (C.c_double * 12)()
    ids = (C.c_int * 2)(0, 1)
    assert L.mrs_batch_set_jac_sites(None, ids, 2) == MRS_ERR_INVALID
    for which in range(sim.DYNOUT_COUNT):
        assert L.mrs_batch_dyn_dim(None, which) == MRS_ERR_INVALID
        assert L.mrs_batch_dyn_device_ptr(None, which) is None
        assert L.mrs_last_status() == MRS_ERR_INVALID
        assert L.mrs_batch_get_dyn(None, which, buf, 0, 1) == MRS_ERR_INVALID
    out = (C.c_int * 18)()
    assert L.mrs_debug_batch_layout(None, out, 18) == MRS_ERR_INVALID


def test_batch_methods():
    for name in ("set_jac_sites", "dyn", "dyn_dim", "dyn_device_ptr"):
        assert callable(getattr(sim.Batch, name)), name

"""C ABI of the per-env mass / inertia / armature family (MRS_INERTIAL_*): the header's declarations, the
library's exports, the Python wrappers and the null-handle errors.  No GPU."""
import ctypes as C
import re
from pathlib import Path

import numpy as np

from mujoco_ros2_simulation_amd import sim

HEADER = (Path(__file__).resolve().parents[1] / "include" / "mrs.h").read_text()
FLAT = re.sub(r"\s+", " ", HEADER)

DECLS = [
    "int mrs_model_derive_inertial(const mrs_model* m, const double* body_mass, const double* body_inertia, "
    "const double* dof_armature, double* body_subtreemass, double* dof_M0, double* dof_invweight0, "
    "double* body_invweight0, double* meaninertia);",
    "int mrs_batch_inertial_dim(const mrs_batch* b, int which);",
    "int mrs_batch_set_inertial(mrs_batch* b, const double* mass, const double* inertia, const double* armature, "
    "int env0, int n);",
    "int mrs_batch_get_inertial(mrs_batch* b, double* mass, double* inertia, double* armature, int env0, int n);",
    "int mrs_batch_get_inertial_derived(mrs_batch* b, int env, double* body_subtreemass, double* dof_invweight0, "
    "double* body_invweight0, double* meaninertia);",
]


def test_header_declares_the_family():
    for d in DECLS:
        assert d in FLAT, d
    for name, val in (("MRS_INERTIAL_BODY_MASS", 0), ("MRS_INERTIAL_BODY_INERTIA", 1), ("MRS_INERTIAL_DOF_ARMATURE", 2),
                      ("MRS_INERTIAL_COUNT", 3)):
        assert re.search(rf"\b{name} = {val}\b", FLAT), name
    # the other families are as they were
    assert re.search(r"\bMRS_FIELD_COUNT = 13\b", FLAT) and re.search(r"\bMRS_PARAM_COUNT = 4\b", FLAT)
    assert not re.search(r"mrs_batch_inertial\w*device_ptr", FLAT)  # deliberately no raw device access
    assert (sim.INERTIAL_BODY_MASS, sim.INERTIAL_BODY_INERTIA, sim.INERTIAL_DOF_ARMATURE, sim.INERTIAL_COUNT) == (0, 1, 2, 3)


def test_exports_and_wrappers():
    lib = sim.lib()
    for name in ("mrs_model_derive_inertial", "mrs_batch_inertial_dim", "mrs_batch_set_inertial",
                 "mrs_batch_get_inertial", "mrs_batch_get_inertial_derived"):
        assert hasattr(lib, name), name
    for name in ("set_inertial", "get_inertial", "inertial_derived"):
        assert callable(getattr(sim.Batch, name)), name
    assert callable(sim.Model.derive_inertial)


def test_null_handles():
    lib = sim.lib()
    buf = np.zeros(64)
    p = buf.ctypes.data
    calls = [lambda: lib.mrs_model_derive_inertial(None, None, None, None, p, None, None, None, None),
             lambda: lib.mrs_batch_inertial_dim(None, 0),
             lambda: lib.mrs_batch_set_inertial(None, p, None, None, 0, 1),
             lambda: lib.mrs_batch_get_inertial(None, p, None, None, 0, 1),
             lambda: lib.mrs_batch_get_inertial_derived(None, 0, p, None, None, None)]
    for call in calls:
        assert call() == -1
        assert "null" in lib.mrs_last_error().decode()
        assert lib.mrs_last_status() == -1

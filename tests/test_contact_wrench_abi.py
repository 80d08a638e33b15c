"""The contact-force entry points exist and reject a NULL batch (CPU: no device is touched)."""
import ctypes as C

from mujoco_ros2_simulation_amd import sim

MRS_ERR_INVALID = -1


def test_entry_points_and_null_batch():
    L = sim.lib()
    for name in ("mrs_batch_contact_wrench_device_ptr", "mrs_batch_get_contact_wrench", "mrs_batch_get_contact_forces"):
        assert hasattr(L, name), name
    buf = (C.c_double * 12)()
    assert L.mrs_batch_contact_wrench_device_ptr(None) is None
    assert L.mrs_last_status() == MRS_ERR_INVALID
    assert L.mrs_batch_get_contact_wrench(None, buf, 0, 1) == MRS_ERR_INVALID
    assert L.mrs_batch_get_contact_forces(None, 0, 2, buf) == MRS_ERR_INVALID
    out = (C.c_int * 17)()
    assert L.mrs_debug_batch_layout(None, out, 17) == MRS_ERR_INVALID


def test_batch_methods():
    for name in ("contact_wrench", "contact_wrench_device_ptr", "contact_forces"):
        assert callable(getattr(sim.Batch, name)), name
    assert sim.LAYOUT_OUTPUT_KEYS == ["contact_wrench"]

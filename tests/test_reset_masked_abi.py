"""The masked reset and the start-state pool in the C ABI and the Python binding (no GPU needed):
include/mrs.h declares the five entry points, libmrs.so exports them, sim.Batch wraps them, and the
state keeps its 13 fields (the feature adds entry points, no field)."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

from mujoco_ros2_simulation_amd import sim

HEADER = Path(__file__).resolve().parents[1] / "include" / "mrs.h"
NEW = ["mrs_batch_set_start_states", "mrs_batch_set_start_states_device", "mrs_batch_num_start_states",
       "mrs_batch_reset_masked_device", "mrs_batch_reset_masked"]


def test_header_declares_and_library_exports(built):
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    lib = ctypes.CDLL(str(sim.LIB_PATH))
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
        assert hasattr(lib, name), name
    # argument lists as the issue states them
    flat = " ".join(text.split())
    assert "int mrs_batch_set_start_states(mrs_batch* b, const double* qpos, const double* qvel, int count);" in flat
    assert ("int mrs_batch_set_start_states_device(mrs_batch* b, const float* d_qpos, const float* d_qvel, int count);"
            in flat)
    assert "int mrs_batch_num_start_states(const mrs_batch* b);" in flat
    assert ("int mrs_batch_reset_masked_device(mrs_batch* b, const unsigned char* d_mask, const int* d_key, int key);"
            in flat)
    assert "int mrs_batch_reset_masked(mrs_batch* b, const unsigned char* mask, const int* keys, int key);" in flat


def test_field_count_unchanged():
    assert "MRS_FIELD_COUNT = 13" in HEADER.read_text()


def test_binding_has_the_methods(built):
    for name in ("set_start_states", "set_start_states_device", "reset_where", "reset_where_device"):
        assert callable(getattr(sim.Batch, name)), name
    assert isinstance(sim.Batch.num_start_states, property)
    lib = sim.lib()
    for name in NEW:
        assert getattr(lib, name).argtypes is not None, name


def test_null_handles_are_refused(built):
    """the exception firewall: a null batch is MRS_ERR_INVALID (0 rows for the count), not a crash"""
    lib = sim.lib()
    mask = np.ones(4, dtype=np.uint8)
    assert lib.mrs_batch_reset_masked(None, mask.ctypes.data, None, -1) == -1
    assert lib.mrs_batch_reset_masked_device(None, None, None, -1) == -1
    assert lib.mrs_batch_set_start_states(None, None, None, 0) == -1
    assert lib.mrs_batch_set_start_states_device(None, None, None, 0) == -1
    assert lib.mrs_batch_num_start_states(None) == 0


def test_mask_shape_is_checked_before_the_library():
    """reset_where checks the mask's shape and dtype itself (a ValueError, no handle needed)"""
    b = sim.Batch.__new__(sim.Batch)
    b.n, b._h = 8, None
    with pytest.raises(ValueError):
        b.reset_where(np.ones(7, dtype=bool))
    with pytest.raises(ValueError):
        b.reset_where(np.ones(8, dtype=np.float32))
    with pytest.raises(ValueError):
        b.reset_where(np.ones(8, dtype=bool), keys=np.zeros(8, dtype=np.int64))

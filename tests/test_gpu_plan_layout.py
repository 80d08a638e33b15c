"""A batch runs the plan that the host-only planner reports: Batch.layout()'s first 16 values equal
sim.plan_layout for the same model, batch size and the device's compute-unit count."""
from pathlib import Path

import pytest

from mujoco_ros2_simulation_amd import sim

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
SCENES = [ROOT / "tests" / "golden" / "ref_scenes" / "scene.xml", ROOT / "scenes" / "arm7_lidar.xml",
          ROOT / "scenes" / "mobile_base.xml", ROOT / "scenes" / "arm_boxes.xml"]


@pytest.mark.parametrize("scene", SCENES, ids=lambda p: p.stem)
def test_batch_layout_is_the_planned_layout(scene):
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    model = sim.Model.load(scene)
    b = sim.Batch(model, 64)
    lay = b.layout()
    b.close()
    assert {k: lay[k] for k in sim.LAYOUT_KEYS} == sim.plan_layout(model, 64, cus)

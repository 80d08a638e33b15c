"""Stateful actuators on the host: the fields the compiler derives for dyntype integrator / filter /
filterexact, <intvelocity> and <position timeconst>, the constructs it rejects, the closed forms that pin
the fp64 reference of tests/act_ref.py, and the C ABI's activation entry points (no GPU needed)."""
import re
from pathlib import Path

import numpy as np
import pytest

import act_ref
from mujoco_ros2_simulation_amd import sim

HEADER = Path(__file__).resolve().parents[1] / "include" / "mrs.h"


def _load(xml):
    return sim.Model.from_string(xml)


def test_compiled_fields(built):
    m = _load(act_ref.arm_xml("Euler", act_ref.FIVE, key_act="0.3 0.1 -0.2 0.4"))
    assert m.nu == 5 and m.na == 4
    assert m.actuator_actadr.tolist() == [-1, 0, 1, 2, 3]
    assert m.actuator_actnum.tolist() == [0, 1, 1, 1, 1]
    assert m.actuator_dyntype.tolist() == [sim.DYN_NONE, sim.DYN_INTEGRATOR, sim.DYN_FILTER, sim.DYN_FILTEREXACT,
                                           sim.DYN_FILTEREXACT]
    # dynprm: the default 1, the <default class="lag"> value, the element's own, <position timeconst>
    assert m.actuator_dynprm[:, 0].tolist() == [1, 1, 0.05, 0.02, 0.03]
    assert np.all(m.actuator_dynprm[:, 1:] == 0)
    # <intvelocity kp kv>: fixed gain kp, affine bias (0, -kp, -kv); <position> keeps its own
    assert m.actuator_gaintype[1] == 0 and m.actuator_biastype[1] == sim.BIAS_AFFINE
    assert m.actuator_gainprm[1, :3].tolist() == [20, 0, 0] and m.actuator_biasprm[1, :3].tolist() == [0, -20, -1]
    assert m.actuator_gainprm[4, :3].tolist() == [10, 0, 0] and m.actuator_biasprm[4, :3].tolist() == [0, -10, -0.5]
    # actlimited: intvelocity always, a general with actrange under autolimits, none otherwise
    assert m.actuator_actlimited.tolist() == [0, 1, 0, 1, 0]
    assert m.actuator_actrange[1].tolist() == [-1.5, 1.5] and m.actuator_actrange[3].tolist() == [-0.8, 0.8]
    assert m.actuator_actearly.tolist() == [0, 0, 0, 1, 0]
    assert m.actuator_ctrllimited.tolist() == [1, 1, 0, 0, 1]
    assert m.nkey == 1 and m.key_act.shape == (1, 4) and m.key_act[0].tolist() == [0.3, 0.1, -0.2, 0.4]
    # a keyframe without act: zeros
    k = _load(act_ref.arm_xml("Euler", act_ref.FIVE).replace(
        "</mujoco>", '<keyframe><key qpos="0 0"/></keyframe></mujoco>'))
    assert k.key_act.shape == (1, 4) and not k.key_act.any()
    # a model without stateful actuators: na 0, every address -1
    s = _load(act_ref.twin_xml(act_ref.arm_xml("Euler", act_ref.FIVE)))
    assert s.na == 0 and s.actuator_actadr.tolist() == [-1] * 5 and s.actuator_dyntype.tolist() == [0] * 5


def test_autolimits_off_and_dampratio(built):
    xml = act_ref.arm_xml("Euler", act_ref.FIVE).replace('autolimits="true"', 'autolimits="false"')
    xml = xml.replace('ctrlrange="-1 1"', 'ctrllimited="true" ctrlrange="-1 1"').replace(
        'ctrlrange="-2 2"', 'ctrllimited="true" ctrlrange="-2 2"')
    m = _load(xml)
    # without autolimits a range alone limits nothing; intvelocity's activation stays limited
    assert m.actuator_actlimited.tolist() == [0, 1, 0, 0, 0]
    # dampratio on <intvelocity> becomes kv as on <position>
    a = _load(act_ref.arm_xml("Euler", '<intvelocity name="iv" joint="j2" kp="20" dampratio="1" actrange="-1 1"/>\n'))
    p = _load(act_ref.arm_xml("Euler", '<position name="iv" joint="j2" kp="20" dampratio="1"/>\n'))
    assert a.actuator_biasprm[0, 2] < 0 and a.actuator_biasprm[0, 2] == p.actuator_biasprm[0, 2]
    # timeconst 0 on <position> is a stateless actuator
    z = _load(act_ref.arm_xml("Euler", '<position name="p" joint="j1" kp="3" timeconst="0"/>\n'))
    assert z.na == 0 and z.actuator_dyntype.tolist() == [0]


@pytest.mark.parametrize("act,msg", [
    ('<general name="a" joint="j1" dyntype="muscle"/>', "not supported"),
    ('<general name="a" joint="j1" dyntype="user"/>', "not supported"),
    ('<general name="a" joint="j1" dyntype="filter" actdim="2"/>', "not supported"),
    ('<intvelocity name="a" joint="j1" kp="5"/>', "actrange"),
    ('<general name="a" joint="j1" dyntype="integrator" actlimited="true"/>', "invalid range"),
    ('<general name="a" joint="j1" dyntype="integrator" actrange="1 -1"/>', "invalid range"),
    ('<general name="a" joint="j1" dyntype="filter" actdim="0"/>', "actdim"),
    ('<muscle name="a" joint="j1"/>', "unsupported actuator type"),
    ('<damper name="a" joint="j1"/>', "unsupported actuator type"),
])
def test_rejections(built, act, msg):
    with pytest.raises(sim.MrsError) as e:
        _load(act_ref.arm_xml("Euler", "    " + act + "\n"))
    assert msg in str(e.value), str(e.value)


CLOSED = """    <general name="fe" joint="j1" dyntype="filterexact" dynprm="0.04" ctrlrange="-1 1"/>
    <general name="fl" joint="j1" dyntype="filter" dynprm="0.03"/>
    <general name="in" joint="j2" dyntype="integrator" actrange="-0.5 0.25"/>
    <general name="iu" joint="j2" dyntype="integrator"/>
"""


@pytest.mark.parametrize("k", [1, 7, 200])
def test_reference_closed_forms(built, k):
    """constant ctrl c from act0, k steps: filterexact c + (act0 - c) exp(-k h / tau), filter
    c + (act0 - c) (1 - h / tau)^k, integrator act0 + k h c saturating at actrange"""
    r = act_ref.ActRef(act_ref.arm_xml("Euler", CLOSED))
    h = r.h
    act0 = np.array([0.3, -0.7, 0.1, -0.2])
    ctrl = np.array([2.5, 0.6, 1.5, -0.9])  # (the first is clamped to ctrlrange: c = 1)
    c = np.array([1.0, 0.6, 1.5, -0.9])
    want = np.array([c[0] + (act0[0] - c[0]) * np.exp(-k * h / 0.04),
                     c[1] + (act0[1] - c[1]) * (1 - h / 0.03) ** k,
                     min(act0[2] + k * h * c[2], 0.25),
                     act0[3] + k * h * c[3]])
    got = r.rollout_act(act0, ctrl, k)
    assert np.all(np.abs(got - want) <= 1e-12 * np.maximum(1, np.abs(want))), (got, want)
    # clampctrl disabled: the raw ctrl drives the filter
    r2 = act_ref.ActRef(act_ref.arm_xml("Euler", CLOSED, flags='<flag clampctrl="disable"/>'))
    got2 = r2.rollout_act(act0, ctrl, k)[0]
    want2 = 2.5 + (act0[0] - 2.5) * np.exp(-k * h / 0.04)
    assert abs(got2 - want2) <= 1e-12 * max(1, abs(want2))


def test_reference_force_input(built):
    """the twin's ctrl: the clamped ctrl of a stateless actuator, the activation of a stateful one, the
    next activation under actearly"""
    r = act_ref.ActRef(act_ref.arm_xml("Euler", act_ref.FIVE))
    act = np.array([0.2, -0.3, 0.5, 0.1])
    ctrl = np.array([1.7, 0.4, 0.9, -3.0, 0.6])
    x = r.force_input(act, ctrl)
    nxt = 0.5 + (-3.0 - 0.5) * (1 - np.exp(-0.002 / 0.02))
    assert x[0] == 1.0 and x[1] == 0.2 and x[2] == -0.3 and x[4] == 0.1
    assert abs(x[3] - max(nxt, -0.8)) < 1e-15


def test_header_declares_act_entry_points():
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    for name in ("mrs_batch_set_act", "mrs_batch_get_act", "mrs_batch_act_device_ptr"):
        assert re.search(rf"\b{name}\s*\(", text), name
    assert "MRS_FIELD_COUNT = 13" in HEADER.read_text()

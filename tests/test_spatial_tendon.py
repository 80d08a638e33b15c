"""Spatial tendons through sites and pulleys (MJCF <tendon><spatial>; mj_tendon's mjWRAP_SITE /
mjWRAP_PULLEY part): the compiler's constants from closed forms, every construct it rejects by its
message, and the fp64 reference of the GPU tests (tests/tendon_ref.py) against central differences of its
own length.  No GPU."""
import numpy as np
import pytest

import binding
import tendon_ref
from mujoco_ros2_simulation_amd import sim

SLIDER = """<mujoco><option gravity="0 0 0" {option}/>{default}
<worldbody><site name="w"/><site name="w2" pos="0 1 0"/>
<body name="a" pos="{d} 0 0"><joint name="s" type="slide" axis="1 0 0"/>
  <geom type="box" size="0.05 0.05 0.05" mass="{m}" contype="0" conaffinity="0"/><site name="sa"/><site name="sb" pos="0 0.1 0"/></body>
</worldbody><tendon>{tendon}</tendon>{extra}</mujoco>"""


def slider(tendon, d=0.7, m=2.5, extra="", option="", default=""):
    return sim.Model.from_string(SLIDER.format(tendon=tendon, d=d, m=m, extra=extra, option=option, default=default))


def test_slider_constants():
    """a world site at the origin, a site on a slider of mass m at distance d along the axis: length0 = d,
    invweight0 = 1 / m; behind <pulley divisor="2"> the segment counts half: d / 2 and 1 / (4 m)"""
    d, m = 0.7, 2.5
    mod = slider('<spatial name="t"><site site="w"/><site site="sa"/></spatial>', d, m)
    assert mod.ntendon == 1 and mod.nwrap == 2
    np.testing.assert_array_equal(mod.tendon_kind, [sim.TENDON_SPATIAL])
    np.testing.assert_array_equal(mod.wrap_type, [sim.WRAP_SITE, sim.WRAP_SITE])
    np.testing.assert_array_equal(mod.wrap_objid, [mod.name2id(sim.OBJ_SITE, "w"), mod.name2id(sim.OBJ_SITE, "sa")])
    np.testing.assert_allclose(mod.tendon_length0, [d], rtol=1e-14)
    np.testing.assert_allclose(mod.tendon_invweight0, [1 / m], rtol=1e-12)
    # a first branch inside the slider body adds its constant length and no Jacobian
    mod = slider('<spatial><site site="sa"/><site site="sb"/><pulley divisor="2"/><site site="w"/><site site="sa"/></spatial>', d, m)
    np.testing.assert_array_equal(mod.wrap_type, [sim.WRAP_SITE, sim.WRAP_SITE, sim.WRAP_PULLEY, sim.WRAP_SITE, sim.WRAP_SITE])
    np.testing.assert_allclose(mod.wrap_prm[2], 2.0)
    assert mod.wrap_objid[2] == -1
    np.testing.assert_allclose(mod.tendon_length0, [0.1 + d / 2], rtol=1e-14)
    np.testing.assert_allclose(mod.tendon_invweight0, [1 / (4 * m)], rtol=1e-12)


def test_pendulum_length0():
    """a site at radius r on a pendulum, a world site at distance a from the hinge at the polar angle th0:
    length0 = sqrt(a^2 + r^2 - 2 a r cos th0)"""
    a, r = 0.5, 0.3
    for th0 in (0.4, 1.3, 2.9):
        m = tendon_ref.pendulum(a, r, th0)
        np.testing.assert_allclose(m.tendon_length0, [np.sqrt(a * a + r * r - 2 * a * r * np.cos(th0))], rtol=1e-13)
        assert m.sensor_type.tolist() == [sim.SENS_TENDONPOS, sim.SENS_TENDONVEL]
        assert m.sensor_dim.tolist() == [1, 1] and m.sensor_adr.tolist() == [0, 1] and m.nsensordata == 2
        assert m.sensor_objtype.tolist() == [sim.OBJ_TENDON] * 2 and m.sensor_objid.tolist() == [0, 0]


def test_attributes_defaults_and_limits():
    """springlength -1 is the length at qpos0, one value a zero dead band; autolimits set limited from a
    range; the attributes come through a defaults class; width / rgba / material are accepted"""
    d = 0.7
    path = '<site site="w"/><site site="sa"/>'
    m = slider(f'<spatial name="t0" springlength="-1" stiffness="3" width="0.01" rgba="1 0 0 1">{path}</spatial>'
               f'<spatial name="t1" range="0.2 0.9" margin="0.01" springlength="0.3 0.5">{path}</spatial>'
               f'<spatial name="t2" class="c" limited="false">{path}</spatial>'
               f'<spatial name="t3" springlength="0.25">{path}</spatial>',
               d, default='<default><default class="c"><tendon range="0.1 0.2" frictionloss="0.4" damping="0.3" '
                          'solreflimit="0.03 0.9" solimpfriction="0.8 0.9 0.002 0.5 2"/></default></default>')
    np.testing.assert_allclose(m.tendon_lengthspring, [[d, d], [0.3, 0.5], [d, d], [0.25, 0.25]], rtol=1e-14)
    assert m.tendon_limited.tolist() == [0, 1, 0, 0]
    np.testing.assert_allclose(m.tendon_range[1], [0.2, 0.9])
    np.testing.assert_allclose(m.tendon_margin, [0, 0.01, 0, 0])
    np.testing.assert_allclose(m.tendon_stiffness, [3, 0, 0, 0])
    np.testing.assert_allclose(m.tendon_range[2], [0.1, 0.2])
    np.testing.assert_allclose([m.tendon_frictionloss[2], m.tendon_damping[2]], [0.4, 0.3])
    np.testing.assert_allclose(m.tendon_solref_lim[2], [0.03, 0.9])
    np.testing.assert_allclose(m.tendon_solimp_fri[2], [0.8, 0.9, 0.002, 0.5, 2])
    assert slider(f'<spatial limited="true" range="0 1">{path}</spatial>').tendon_limited.tolist() == [1]


def test_mixed_order_and_actuator():
    """fixed and spatial tendons keep document order in tendon_adr / tendon_num / wrap_type; a tendon=
    actuator resolves to the spatial tendon's id; dampratio takes the moment at qpos0"""
    m = slider('<fixed name="f0"><joint joint="s" coef="2"/></fixed>'
               '<spatial name="sp"><site site="w"/><site site="sa"/><pulley divisor="4"/><site site="w2"/><site site="sb"/></spatial>'
               '<fixed name="f1"><joint joint="s" coef="-1"/></fixed>',
               extra='<actuator><motor tendon="f1"/><position tendon="sp" kp="50" gear="2" dampratio="1"/></actuator>')
    assert m.ntendon == 3 and m.nwrap == 7
    assert m.tendon_adr.tolist() == [0, 1, 6] and m.tendon_num.tolist() == [1, 5, 1]
    assert m.tendon_kind.tolist() == [sim.TENDON_FIXED, sim.TENDON_SPATIAL, sim.TENDON_FIXED]
    J, S, P = sim.WRAP_JOINT, sim.WRAP_SITE, sim.WRAP_PULLEY
    assert m.wrap_type.tolist() == [J, S, S, P, S, S, J]
    assert (J, P, S) == (1, 2, 3)  # mjtWrap
    assert m.name2id(sim.OBJ_TENDON, "sp") == 1
    assert m.actuator_trntype.tolist() == [sim.TRN_TENDON] * 2 and m.actuator_trnid[:, 0].tolist() == [2, 1]
    # J(qpos0) of sp on the slider: 1 from the first branch, and the second's direction (0.7, -0.9) / |.|
    # along x over 4
    j0 = 1 + 0.7 / np.hypot(0.7, 0.9) / 4
    np.testing.assert_allclose(m.tendon_invweight0[1], j0 * j0 / 2.5, rtol=1e-12)
    np.testing.assert_allclose(m.actuator_biasprm[1, 2], -2 * np.sqrt(50 * 2.5 / (2 * j0) ** 2), rtol=1e-12)


PATH = '<site site="w"/><site site="sa"/>'


@pytest.mark.parametrize("tendon, msg, kw", [
    ('<spatial><site site="w"/><geom geom="g"/><site site="sa"/></spatial>', "wrapping geoms", {}),
    ('<spatial><site site="w"/><geom geom="g" sidesite="sb"/><site site="sa"/></spatial>', "wrapping geoms", {}),
    ('<spatial><site site="w" sidesite="sb"/><site site="sa"/></spatial>', "sidesite", {}),
    ('<spatial><site site="w"/></spatial>', "spatial tendons need at least two sites", {}),
    ('<spatial><site site="nope"/></spatial>', "spatial tendons need at least two sites", {}),
    ('<spatial></spatial>', "spatial tendons need at least two sites", {}),
    ('<spatial><pulley divisor="2"/><site site="w"/><site site="sa"/></spatial>', "cannot start with a pulley", {}),
    (f'<spatial>{PATH}<pulley divisor="2"/></spatial>', "cannot end with a pulley", {}),
    (f'<spatial>{PATH}<pulley divisor="2"/><pulley divisor="2"/>{PATH}</spatial>', "two pulleys in a row", {}),
    (f'<spatial>{PATH}<pulley divisor="2"/><site site="w"/></spatial>', "branch of a spatial tendon needs at least two sites", {}),
    (f'<spatial><site site="w"/><pulley divisor="2"/>{PATH}</spatial>', "branch of a spatial tendon needs at least two sites", {}),
    (f'<spatial>{PATH}<pulley divisor="0"/>{PATH}</spatial>', "divisor must be positive", {}),
    (f'<spatial>{PATH}<pulley divisor="-2"/>{PATH}</spatial>', "divisor must be positive", {}),
    (f'<spatial>{PATH}<pulley/>{PATH}</spatial>', "requires 'divisor'", {}),
    ('<spatial><site site="w"/><site site="nope"/></spatial>', "unknown site 'nope'", {}),
    (f'<spatial>{PATH}<joint joint="s" coef="1"/></spatial>', "site and pulley elements only", {}),
    (f'<spatial armature="0.1">{PATH}</spatial>', "tendon armature", {}),
    (f'<spatial damping="1">{PATH}</spatial>', "tendon damping", {"option": 'integrator="implicitfast"'}),
    (f'<spatial damping="1">{PATH}</spatial>', "tendon damping", {"option": 'integrator="implicit"'}),
    (f'<spatial name="t">{PATH}</spatial>', "velocity-dependent actuators on tendons",
     {"option": 'integrator="implicitfast"', "extra": '<actuator><velocity tendon="t" kv="2"/></actuator>'}),
    (f'<spatial name="t">{PATH}</spatial>', "unknown object 'u'",
     {"extra": '<sensor><tendonpos tendon="u"/></sensor>'}),
    (f'<spatial name="t">{PATH}</spatial>', "unknown tendon 'u'",
     {"extra": '<actuator><motor tendon="u"/></actuator>'}),
])
def test_rejections(tendon, msg, kw):
    with pytest.raises(sim.MrsError, match=msg):
        slider(tendon, **kw)


def test_tendon_equality_stays_rejected():
    with pytest.raises(sim.MrsError):
        slider(f'<spatial name="t">{PATH}</spatial>', extra='<equality><tendon tendon1="t"/></equality>')


def _chain(tendon, extra="", option=""):
    return tendon_ref.CHAIN.format(tendon=tendon, extra=extra, option=option)


def test_reference_jacobian_is_the_gradient_of_its_length():
    """tendon_ref's J against central differences of its own L on the 4-dof chain with the two-branch
    pulley path (and the plain path), at random poses; its velocity is J qvel"""
    xml = _chain(f'<spatial name="A">{tendon_ref.PATH_A}</spatial><spatial name="B">{tendon_ref.PATH_B}</spatial>'
                 + tendon_ref.FIXED_C)
    ft = tendon_ref.ForceTwin(xml)
    m = ft.model
    assert m.nv == 4 and m.nq == 4 and ft.sp == [0, 1]
    assert [(w) for _, _, w in tendon_ref.segments(m, 1)] == [1.0, 1.0, 0.5]
    rng = np.random.default_rng(5)
    h = 1e-6
    for _ in range(5):
        q = rng.uniform(-1, 1, 4) * [1, 1, 1, 0.2]
        v = rng.uniform(-2, 2, 4)
        L, Ld, J, shortest = ft.kin(q, v)
        assert shortest > 0.05
        num = np.zeros_like(J)
        for j in range(4):
            e = np.zeros(4)
            e[j] = h
            num[:, j] = (ft.kin(q + e, v)[0] - ft.kin(q - e, v)[0]) / (2 * h)
        np.testing.assert_allclose(J, num, rtol=1e-6, atol=1e-9)
        np.testing.assert_allclose(Ld, J @ v, rtol=1e-14)
        np.testing.assert_allclose(J[2], [0.5, 0, 0, 1])  # (the fixed tendon's row)
    # at qpos0 the reference agrees with the compiler's constants
    L, _, J, _ = ft.kin(m.qpos0, np.zeros(4))
    np.testing.assert_allclose(L, m.tendon_length0, rtol=1e-13)
    Minv = np.linalg.inv(binding.OracleData(ft.twin).mass_matrix())
    np.testing.assert_allclose(np.einsum("ti,ij,tj->t", J, Minv, J), m.tendon_invweight0, rtol=1e-10)


def test_force_twin_has_no_spatial_tendon_and_row_twin_is_fixed():
    xml = _chain(f'<spatial name="A" stiffness="2">{tendon_ref.PATH_A}</spatial>' + tendon_ref.FIXED_C,
                 extra='<actuator><motor tendon="A"/><motor joint="sl"/><motor tendon="C"/></actuator>'
                       '<sensor><tendonpos tendon="A"/><jointpos joint="sl"/></sensor>')
    ft = tendon_ref.ForceTwin(xml)
    assert ft.twin.ntendon == 1 and ft.twin.tendon_kind.tolist() == [sim.TENDON_FIXED]
    assert ft.on_sp == [0] and ft.keep == [1, 2] and ft.twin.nu == 2
    assert ft.twin.sensor_type.tolist() == [sim.SENS_JOINTPOS]
    # a straight tendon along a slide axis becomes the fixed tendon with shifted range / springlength
    d = 0.7
    row = tendon_ref.row_twin_xml(SLIDER.format(
        tendon=f'<spatial name="t" range="0.5 0.9" springlength="0.6 0.8" stiffness="3">{PATH}<pulley divisor="2"/>{PATH}</spatial>',
        d=d, m=1, option="", default="", extra='<actuator><position tendon="t" kp="7" gear="2"/></actuator>'))
    t = sim.Model.from_string(row)
    assert t.tendon_kind.tolist() == [sim.TENDON_FIXED] and t.wrap_type.tolist() == [sim.WRAP_JOINT]
    c = 1.5 * d
    np.testing.assert_allclose(t.wrap_prm, [1.5])
    np.testing.assert_allclose(t.tendon_range[0], [0.5 - c, 0.9 - c], rtol=1e-13)
    np.testing.assert_allclose(t.tendon_lengthspring[0], [0.6 - c, 0.8 - c], rtol=1e-13)
    np.testing.assert_allclose(t.actuator_biasprm[0, :3], [-7 * 2 * c, -7, 0], rtol=1e-13)


def test_view_arrays_are_copies_and_reload_equal():
    """the model's arrays are copies of the view (they outlive a second load and do not alias it), and a
    second load of the same scene gives the same path arrays"""
    xml = _chain(f'<spatial name="B">{tendon_ref.PATH_B}</spatial>' + tendon_ref.FIXED_C)
    a = sim.Model.from_string(xml)
    keep = {k: getattr(a, k).copy() for k in ("wrap_type", "tendon_kind", "wrap_objid", "wrap_prm", "tendon_adr", "tendon_num")}
    a.wrap_type[:] = 0  # (writes the copy, not the compiled model)
    b = sim.Model.from_string(xml)
    for k, v in keep.items():
        np.testing.assert_array_equal(getattr(b, k), v)
        assert getattr(b, k).dtype == v.dtype
    assert keep["wrap_type"].shape == (b.nwrap,) and keep["tendon_kind"].shape == (b.ntendon,)
    # a model without tendons has empty arrays of the right type
    e = sim.Model.from_string("<mujoco><worldbody/></mujoco>")
    assert e.wrap_type.shape == (0,) and e.tendon_kind.shape == (0,) and e.wrap_type.dtype == np.int32


def test_plan_counts_the_jacobian_slot(monkeypatch):
    """the per-env LDS slot [nten_spatial][nv] is taken only by a model with a spatial tendon, and is part
    of the planned LDS size; the same scene with the tendon fixed plans what it planned before"""
    path = f'<spatial name="A">{tendon_ref.PATH_A}</spatial><spatial name="B">{tendon_ref.PATH_B}</spatial>'
    sp = sim.Model.from_string(_chain(path + tendon_ref.FIXED_C))
    fx = sim.Model.from_string(_chain('<fixed name="A"><joint joint="h1" coef="1"/></fixed>'
                                      '<fixed name="B"><joint joint="h2" coef="1"/></fixed>' + tendon_ref.FIXED_C))
    for g in (16, 64):
        monkeypatch.setenv("MRS_GROUP", str(g))
        a, b = sim.plan_layout(sp, 6, 256), sim.plan_layout(fx, 6, 256)
        assert a["group"] == b["group"] == g
        assert a["lds_floats"] == b["lds_floats"] + 2 * 4  # two rows of nv = 4 (already a multiple of 4)

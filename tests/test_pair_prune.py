"""Pair pruning on the host (devtables.h prune_pairs; sim.walked_pairs / mrs_debug_pairs, no device): the
list a batch walks is the static filter's list without the automatic pairs whose geoms can never touch.
The expected set comes from the bound restated in pair_prune_scenes.py; soundness is checked against the
fp64 oracle's poses at random joint angles."""
import numpy as np
import pytest

import binding
from mujoco_ros2_simulation_amd import sim
from pair_prune_scenes import (C3, GEOM_PLANE, JNT_BALL, JNT_FREE, ROOT, TREE, c3_box_n_at, c3_explicit, c3_free_body,
                               c3_mocap, c3_slide_root, expected_pruned)

SCENES = str(ROOT / "scenes")


def _lists(model, monkeypatch):
    """(full [k, 2], walked [k', 2], pruned count, indices of the full list that were pruned)"""
    monkeypatch.setenv("MRS_NO_PAIR_PRUNE", "1")
    full, none = sim.walked_pairs(model)
    monkeypatch.delenv("MRS_NO_PAIR_PRUNE")
    walked, pruned = sim.walked_pairs(model)
    assert none == 0 and pruned == len(full) - len(walked)
    # the walked list is the full one with pairs taken out, order kept
    gone, k = [], 0
    for q, pr in enumerate(full.tolist()):
        if k < len(walked) and walked[k].tolist() == pr:
            k += 1
        else:
            gone.append(q)
    assert k == len(walked), "the walked pairs are not a subsequence of the full list"
    return full, walked, pruned, gone


def _names(model, pairs):
    return {(model.id2name(sim.OBJ_GEOM, int(a)), model.id2name(sim.OBJ_GEOM, int(b))) for a, b in pairs}


def test_full_list_is_the_compilers(arm7_model, monkeypatch):
    full, _, _, _ = _lists(arm7_model, monkeypatch)
    m = arm7_model
    assert full.tolist() == [[int(a), int(b)] for a, b in zip(m.pair_geom1, m.pair_geom2)]
    assert len(full) == 35


def test_c3_walks_7_pairs_and_prunes_28(arm7_model, monkeypatch):
    full, walked, pruned, gone = _lists(arm7_model, monkeypatch)
    assert (len(walked), pruned) == (7, 28)
    assert _names(arm7_model, walked) == {("floor", f"g{k}") for k in range(1, 8)}
    assert gone == expected_pruned(arm7_model, full, 0)
    # the compiler's list is untouched
    assert len(arm7_model.pair_geom1) == 35


def test_moved_box_keeps_the_links_that_reach_it(monkeypatch):
    model = sim.Model.from_string(c3_box_n_at(2.3), SCENES)
    full, walked, pruned, gone = _lists(model, monkeypatch)
    assert gone == expected_pruned(model, full, 0)
    kept_box = {p for p in _names(model, walked) if "box_n" in p}
    # by hand: |c| = |(0.2, 2.3, 0.2)| = 2.317, the box's sphere 0.768; g7 reaches 1.5 + 0.08, g6 1.375 + 0.11
    assert kept_box == {("box_n", "g7")} or kept_box == {("g7", "box_n")}, kept_box
    assert pruned == 27 and len(walked) == 8
    nearer = sim.Model.from_string(c3_box_n_at(1.5), SCENES)
    full, walked, pruned, gone = _lists(nearer, monkeypatch)
    assert gone == expected_pruned(nearer, full, 0)
    assert {a if a != "box_n" else b for a, b in _names(nearer, walked) if "box_n" in (a, b)} == {"g3", "g4", "g5", "g6", "g7"}


@pytest.mark.parametrize("xml, loose", [(c3_slide_root, [f"g{k}" for k in range(1, 8)]), (c3_free_body, ["stray"]),
                                        (c3_mocap, ["hand", "finger"])], ids=["slide", "free", "mocap"])
def test_unbounded_geoms_keep_every_pair(xml, loose, monkeypatch):
    model = sim.Model.from_string(xml(), SCENES)
    full, walked, pruned, gone = _lists(model, monkeypatch)
    assert gone == expected_pruned(model, full, 0)
    involved = [q for q, pr in enumerate(_pairs_named(model, full)) if set(pr) & set(loose)]
    assert involved, "the scene has no pair with the unbounded geoms"
    assert not set(involved) & set(gone)
    if xml is not c3_slide_root:  # (the arm is still bounded: its box pairs go as in C3)
        assert pruned >= 28


def _pairs_named(model, pairs):
    return [(model.id2name(sim.OBJ_GEOM, int(a)), model.id2name(sim.OBJ_GEOM, int(b))) for a, b in pairs]


def test_explicit_pairs_survive(monkeypatch):
    model = sim.Model.from_string(c3_explicit(), SCENES)
    full, walked, pruned, gone = _lists(model, monkeypatch)
    nex = len(model.expair_geom1)
    assert nex == 2
    assert walked[:nex].tolist() == full[:nex].tolist() == [[int(a), int(b)] for a, b in zip(model.expair_geom1, model.expair_geom2)]
    assert [set(p) for p in _pairs_named(model, walked[:nex])] == [{"g7", "box_e"}, {"box_s", "g6"}]
    assert gone == expected_pruned(model, full, nex) and all(q >= nex for q in gone) and pruned >= 26


def _random_qpos(model, rng):
    q = np.array(model.qpos0, dtype=np.float64)
    for j in range(model.njnt):
        a = model.jnt_qposadr[j]
        assert model.jnt_type[j] != JNT_FREE
        if model.jnt_type[j] == JNT_BALL:
            v = rng.normal(size=4)
            q[a:a + 4] = v / np.linalg.norm(v)
        else:
            q[a] = rng.uniform(-np.pi, np.pi)
    return q


@pytest.mark.parametrize("scene", ["c3", "tree"])
def test_soundness_against_oracle_poses(scene, monkeypatch):
    """2000 random poses (angles in +-pi, limits ignored): every pruned pair's centres are further apart
    than the bounding spheres plus margin; a pruned plane pair's geom centre is further in front of the
    plane than its bounding sphere plus margin"""
    model = sim.Model.from_string(C3, SCENES) if scene == "c3" else sim.Model.from_string(TREE, SCENES)
    full, walked, pruned, gone = _lists(model, monkeypatch)
    assert gone == expected_pruned(model, full, 0)
    if scene == "c3":
        assert pruned == 28
    else:
        types = [(model.geom_type[a], model.geom_type[b]) for a, b in full[gone]]
        assert any(GEOM_PLANE in t for t in types) and any(GEOM_PLANE not in t for t in types), _pairs_named(model, full[gone])
        assert 0 < len(walked) and any(GEOM_PLANE not in (model.geom_type[a], model.geom_type[b]) for a, b in walked)
    g1, g2 = full[gone, 0], full[gone, 1]
    margin = np.maximum(model.geom_margin[g1], model.geom_margin[g2])
    need = model.geom_rbound[g1] + model.geom_rbound[g2] + margin
    plane = model.geom_type[g1] == GEOM_PLANE
    assert not np.any(model.geom_type[g2] == GEOM_PLANE)  # (the lower geom type comes first)
    d = binding.OracleData(model)
    rng = np.random.default_rng(5)
    worst = np.inf
    for _ in range(2000):
        d.qpos[:] = _random_qpos(model, rng)
        _, _, gpos, gmat = d.kinematics()
        sep = np.linalg.norm(gpos[g1] - gpos[g2], axis=1)
        normal = gmat[g1][:, [2, 5, 8]]
        sep = np.where(plane, np.einsum("ij,ij->i", normal, gpos[g2] - gpos[g1]), sep)
        assert np.all(sep > need), [(_pairs_named(model, full[gone])[i], sep[i], need[i]) for i in np.nonzero(sep <= need)[0]]
        worst = min(worst, float(np.min(sep - need)))
    print(f"{scene}: smallest gap of a pruned pair over 2000 poses {worst:.4f} m")

"""Host tests of the mesh-topology feature: the numpy reference (tests/topology_ref.py) on hand-made meshes and on the
fixtures of tests/golden/mesh_eval_reference.npz, the rules of slice3d_amd.mesh_topology.select_components (pure host
code), and the new flags' defaults.  The device code is tested in tests/test_gpu_mesh_topology.py."""
import os
import sys

import numpy as np
import pytest

import simplify_cases as sc
import simplify_ref as sr
import topology_ref as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _row(t, k):
    return {n: t["table"][n][k] for n in tr.COUNT_COLUMNS}


# ------------------------------------------------------------------------------------------------ hand-made meshes
def test_tetrahedron():
    t = tr.topology(*tr.hand_made("tetrahedron"))
    assert t["n_components"] == 1 and np.array_equal(t["face_component"], [0, 0, 0, 0])
    r = _row(t, 0)
    assert (r["faces"], r["vertices"], r["edges"], r["edges_1"], r["edges_2"], r["edges_3plus"]) == (4, 4, 6, 0, 6, 0)
    assert r["conflicts"] == 0 and r["degenerate"] == 0 and r["euler"] == 2
    assert r["closed_oriented"] and r["oriented_with_border"]
    v, f = tr.hand_made("tetrahedron")
    assert t["table"]["volume"][0] == pytest.approx(sr.signed_volume(v, f)) and t["table"]["volume"][0] > 0
    assert np.array_equal(t["table"]["bbox"][0], [-1, -1, -1, 1, 1, 1])


def test_two_tetrahedra_sharing_one_vertex_are_one_component():
    t = tr.topology(*tr.hand_made("two_tetrahedra_one_vertex"))
    assert t["n_components"] == 1
    r = _row(t, 0)
    assert (r["faces"], r["vertices"], r["edges"], r["edges_2"]) == (8, 7, 12, 12)
    assert r["euler"] == 3 and r["closed_oriented"]          # edge-manifold; the pinched vertex is out of scope


def test_three_faces_on_one_edge():
    t = tr.topology(*tr.hand_made("three_faces_one_edge"))
    r = _row(t, 0)
    assert t["n_components"] == 1 and (r["edges"], r["edges_1"], r["edges_2"], r["edges_3plus"]) == (7, 6, 0, 1)
    assert r["conflicts"] == 1                               # the directed edge 0 -> 1 three times
    assert not r["closed_oriented"] and not r["oriented_with_border"]


def test_flipped_face():
    t = tr.topology(*tr.hand_made("flipped_face"))
    r = _row(t, 0)
    assert (r["edges"], r["edges_2"], r["conflicts"], r["euler"]) == (6, 6, 3, 2)
    assert not r["closed_oriented"] and not r["oriented_with_border"]


def test_face_with_a_repeated_index_connects_and_counts():
    t = tr.topology(*tr.hand_made("repeated_index"))
    r = _row(t, 0)
    assert t["n_components"] == 1 and t["vertex_component"][4] == 0
    assert r["faces"] == 5 and r["degenerate"] == 1 and r["vertices"] == 5
    assert (r["edges"], r["edges_1"], r["edges_2"]) == (8, 1, 7)          # 0-4 twice, 4-4 once
    assert not r["closed_oriented"] and r["oriented_with_border"]


def test_unreferenced_vertices_get_no_component():
    v, f = tr.hand_made("unreferenced_vertex")
    t = tr.topology(v, f)
    assert t["n_components"] == 1 and np.array_equal(t["vertex_component"], [-1, 0, 0, 0, 0, -1])
    vo, fo = tr.keep(v, f, t["face_component"], [True])
    assert np.array_equal(vo, v[1:5]) and np.array_equal(fo, f - 1)


def test_weld_reference_rules():
    v = np.array([[0.0, 0, 0], [1, 0, 0], [0, 1, 0], [-0.0, 0, -0.0], [1, 0, 0], [np.nextafter(1.0, 2.0), 0, 0],
                  [np.nan, 0, 0], [0, 1, 0]])
    f = np.array([[0, 1, 2], [3, 4, 5], [3, 5, 7]], dtype=np.int64)
    assert np.array_equal(tr.weld(v, f), [0, 1, 2, 0, 1, 5, 6, 2])        # both zeros; 1 ulp stays; the NaN is unreferenced
    with pytest.raises(ValueError):
        tr.weld(v, np.array([[0, 1, 6]]))
    vs, fs = tr.soup(*tr.hand_made("tetrahedron"), seed=3)
    t = tr.topology(vs, fs, weld_first=True)
    assert t["n_components"] == 1 and t["table"]["closed_oriented"][0] and t["table"]["vertices"][0] == 4
    assert tr.topology(vs, fs)["n_components"] == 4


def test_component_ids_ascend_with_the_smallest_vertex():
    f = np.array([[7, 8, 6], [0, 4, 5], [3, 1, 2]], dtype=np.int64)
    k, fc, vc = tr.components(f, 10)
    assert k == 3 and np.array_equal(fc, [2, 0, 1]) and np.array_equal(vc, [0, 1, 1, 1, 0, 0, 2, 2, 2, -1])


# ------------------------------------------------------------------------------------------------ fixtures
@pytest.mark.parametrize("name,k,chi,closed", [("sphere", 1, 2, True), ("torus", 1, 0, True), ("boxes", 3, 6, True),
                                               ("zero_area", 2, None, False), ("flat", 1, 1, False)])
def test_fixtures(name, k, chi, closed):
    t = tr.topology(*sc.mesh(name))
    assert t["n_components"] == k
    assert bool(t["summary"]["closed_oriented"]) == closed
    if chi is not None:
        assert t["summary"]["euler"] == chi and t["table"]["euler"].sum() == chi
    if closed:
        assert t["table"]["closed_oriented"].all() and not t["table"]["degenerate"].any()
    if name == "flat":
        assert t["summary"]["oriented_with_border"] and t["summary"]["edges_1"] > 0
    assert t["table"]["faces"].sum() == len(sc.mesh(name)[1]) == t["summary"]["faces"]


# ------------------------------------------------------------------------------------------------ select_components
def _table(faces, area=None, volume=None, closed=None):
    from slice3d_amd.mesh_topology import COUNT_COLUMNS, table_from_arrays
    k = len(faces)
    counts = np.zeros((k, len(COUNT_COLUMNS)), dtype=np.int64)
    counts[:, 0] = faces
    counts[:, COUNT_COLUMNS.index("closed_oriented")] = np.ones(k) if closed is None else closed
    m = np.zeros((k, 8))
    m[:, 0] = faces if area is None else area
    m[:, 1] = faces if volume is None else volume
    return table_from_arrays(counts, m)


def test_select_components_rules_and_ties():
    from slice3d_amd.mesh_topology import select_components
    t = _table([10, 40, 40, 5], area=[9.0, 1.0, 2.0, 3.0], volume=[-8.0, 1.0, 50.0, 2.0], closed=[1, 1, 0, 1])
    assert select_components(t).tolist() == [True] * 4
    assert select_components(t, largest=1).tolist() == [False, True, False, False]            # the tie goes to id 1
    assert select_components(t, largest=2).tolist() == [False, True, True, False]
    assert select_components(t, largest=3).tolist() == [True, True, True, False]
    assert select_components(t, largest=0).tolist() == [False] * 4
    assert select_components(t, largest=9).tolist() == [True] * 4
    assert select_components(t, largest=1, by="area").tolist() == [True, False, False, False]
    # volume: |signed volume|, closed components only; component 2 (the largest number, not closed) ranks last
    assert select_components(t, largest=1, by="volume").tolist() == [True, False, False, False]
    assert select_components(t, largest=3, by="volume").tolist() == [True, True, False, True]
    assert select_components(t, largest=4, by="volume").tolist() == [True] * 4
    assert select_components(t, min_faces=10).tolist() == [True, True, True, False]
    assert select_components(t, min_frac=0.25).tolist() == [True, True, True, False]          # 10 >= 0.25 * 40
    assert select_components(t, min_frac=0.26).tolist() == [False, True, True, False]
    assert select_components(t, min_frac=0.2, by="volume").tolist() == [True, False, False, True]   # of 8: 1 fails, 2 is open
    assert select_components(t, largest=1, min_frac=0.5, by="area").tolist() == [True, False, False, False]
    assert select_components(_table([])).tolist() == []
    with pytest.raises(ValueError):
        select_components(t, by="edges")


# ------------------------------------------------------------------------------------------------ flags
def test_new_flags_default_to_today():
    sys.path.insert(0, os.path.join(ROOT, "reg_slices"))
    from options import get_parser
    import make_sdfs
    import clean_meshes
    a = get_parser().parse_args([])
    assert a.keep_largest is None and a.min_component_frac == 0.0 and a.component_measure == "faces"
    assert a.simplify_nfaces is None
    p = make_sdfs.build_parser()
    base = ["--dir_meshes", "m", "--name_dataset", "d"]
    assert p.parse_args(base).sign == "parity" and p.parse_args(base + ["--sign", "auto"]).sign == "auto"
    c = clean_meshes.build_parser().parse_args(["--dir_meshes", "m", "--dir_out", "o"])
    assert (c.weld, c.keep_largest, c.min_component_frac, c.component_measure, c.drop_degenerate, c.report_only) == \
        (False, None, 0.0, "faces", False, False)


def test_abi_is_declared():
    from slice3d_amd import _lib
    header = open(os.path.join(ROOT, "include", "slice3d_hip.h")).read()
    for name in ("s3d_mesh_topology_workspace_bytes", "s3d_mesh_topology_run", "s3d_mesh_topology_emit_labels",
                 "s3d_mesh_topology_emit_table", "s3d_mesh_topology_keep_run", "s3d_mesh_topology_keep_emit"):
        assert name in _lib.SYMBOLS and name + "(" in header

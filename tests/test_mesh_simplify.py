"""Host tests of the simplification suite: the numpy checkers (tests/simplify_ref.py) on hand-made meshes, the reference's
recorded outputs (tests/golden/mesh_simplify_reference.npz) against the very conditions the device code is held to in
tests/test_gpu_mesh_simplify.py, and the C ABI's declaration and registration."""
import os
import re

import numpy as np
import pytest

import sdf_ref
import simplify_cases as sc
import simplify_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TETRA = np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]])
SQUARE = np.array([[0, 1, 2], [0, 2, 3]])


def test_edge_counts_and_manifold_checks_on_hand_made_meshes():
    e, c = sr.edge_face_counts(TETRA)
    assert len(e) == 6 and np.all(c == 2) and np.all(e[:, 0] < e[:, 1])
    assert sr.is_oriented_manifold(TETRA) and sr.euler_characteristic(TETRA) == 2 and sr.boundary_loops(TETRA) == 0
    flipped = TETRA.copy()
    flipped[1] = flipped[1][::-1]                       # one face turned over: an edge is traversed twice the same way
    assert not sr.is_oriented_manifold(flipped) and np.all(sr.edge_face_counts(flipped)[1] == 2)
    assert not sr.is_oriented_manifold(TETRA[:3])       # open
    assert sr.is_oriented_manifold(TETRA[:3], closed=False) and sr.boundary_loops(TETRA[:3]) == 1
    e, c = sr.edge_face_counts(SQUARE)
    assert len(e) == 5 and sorted(c) == [1, 1, 1, 1, 2]
    assert sr.euler_characteristic(SQUARE) == 1 and sr.boundary_loops(SQUARE) == 1
    assert sorted(sr.border_vertices(SQUARE)) == [0, 1, 2, 3]
    fan3 = np.concatenate([SQUARE, [[0, 2, 4]]])        # three faces on the edge (0, 2)
    assert not sr.is_oriented_manifold(fan3, closed=False)
    two = np.concatenate([SQUARE, SQUARE + 4])          # two squares: two loops
    assert sr.boundary_loops(two) == 2 and sr.euler_characteristic(two) == 2
    bowtie = np.array([[0, 1, 2], [0, 3, 4]])           # two triangles meeting in a vertex: the border pinches
    with pytest.raises(ValueError):
        sr.boundary_loops(bowtie)


def test_volume_and_index_checks_on_hand_made_meshes():
    v, f = sc.mesh("tetrahedron")
    assert sr.signed_volume(v, f) == pytest.approx(8.0 / 3.0)
    assert sr.signed_volume(v, f[:, ::-1]) == pytest.approx(-8.0 / 3.0)
    v, f = sc.mesh("octahedron")
    assert sr.signed_volume(v, f) == pytest.approx(4.0 / 3.0) and sr.is_oriented_manifold(f)
    assert sr.euler_characteristic(f) == 2
    assert sr.no_repeated_index(f) and not sr.no_repeated_index(np.array([[0, 0, 1]]))
    assert sr.indices_valid(v, f) and not sr.indices_valid(v[:5], f) and not sr.indices_valid(np.zeros((7, 3)), f)
    assert sr.indices_valid(np.zeros((7, 3)), f, all_referenced=False)
    assert sr.bbox_diagonal(v, f) == pytest.approx(np.sqrt(12.0))
    assert len(sr.probe_points(v, f)) == 6 + 8
    # E of a mesh against itself is 0; against a copy moved by d along x it is d / diagonal
    d = lambda vv, ff, p: sdf_ref.dist_a(vv, ff, p)[0]   # noqa: E731
    assert sr.mesh_error((v, f), (v, f), 1.0, d) < 1e-15
    assert sr.mesh_error((v, f), (v + [10.0, 0, 0], f), 2.0, d) == pytest.approx(5.0, rel=1e-12)   # apex to apex: 10


def test_case_meshes_are_what_the_tests_assume():
    for name, chi in (("sphere", 2), ("torus", 0), ("boxes", 6), ("genus1", 0)):
        v, f = sc.mesh(name)
        assert sr.is_oriented_manifold(f) and sr.euler_characteristic(f) == chi and sr.signed_volume(v, f) != 0
        assert sr.indices_valid(v, f)
    v, f = sc.mesh("genus1")
    assert 20000 <= len(f) and 3 * len(f) > 4096 * 16       # tens of thousands of faces, many scan tiles
    v, f = sc.mesh("open_sphere")
    assert sr.is_oriented_manifold(f, closed=False) and sr.boundary_loops(f) == 1 and sr.indices_valid(v, f)


@pytest.mark.parametrize("name,t", sc.golden_cases())
def test_reference_outputs_meet_the_conditions(name, t):
    """The conditions of the GPU tests are ones the reference meets on every recorded case."""
    v, f = sc.mesh(name)
    vo, fo = sc.reference(name, t)
    assert np.isfinite(vo).all()
    if name == "open_sphere":
        assert sr.indices_valid(vo, fo) and sr.no_repeated_index(fo) and t - 2 <= len(fo) <= t
        assert sr.is_oriented_manifold(fo, closed=False) and sr.boundary_loops(fo) == 1
    else:
        assert sr.check_closed_result(v, f, vo, fo, t) == []


def test_reference_error_grows_as_the_budget_halves():
    """The right side of the error test, E(input, reference at T / 2), is above E(input, reference at T) on the fixtures."""
    dist = lambda vv, ff, p: sdf_ref.dist_a(vv, ff, p)[0]   # noqa: E731
    for name, r in (("sphere", 10), ("torus", 10), ("boxes", 10)):
        v, f = sc.mesh(name)
        t = sc.target(name, r)
        diag = sr.bbox_diagonal(v, f)
        e_t = sr.mesh_error((v, f), sc.reference(name, t), diag, dist)
        e_h = sr.mesh_error((v, f), sc.reference(name, t // 2), diag, dist)
        print("%s %d%%: E(T) = %.3e, E(T/2) = %.3e" % (name, r, e_t, e_h))
        assert 0 < e_t < e_h


def test_abi_declares_and_registers_the_simplifier():
    from slice3d_amd import _lib
    with open(os.path.join(ROOT, "include", "slice3d_hip.h")) as fh:
        header = fh.read()
    for name in ("s3d_mesh_simplify_workspace_bytes", "s3d_mesh_simplify_run", "s3d_mesh_simplify_emit"):
        assert re.search(r"\b(size_t|int)\s+%s\(" % name, header), name
        assert name in _lib.SYMBOLS
    assert int(re.search(r"#define S3D_VERSION (\d+)", header).group(1)) >= 122
    from slice3d_amd import mesh_simplify as ms
    assert ms.mesh_simplify.__defaults__ == (7.,) and ms.simplify_mesh.__defaults__ == (10000, 7.)

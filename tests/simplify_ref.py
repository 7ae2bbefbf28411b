"""numpy checkers for simplified meshes (tests/test_mesh_simplify.py, tests/test_gpu_mesh_simplify.py): what a mesh must
still be after edge collapses.  Vertices (V, 3) float64, faces (F, 3) integer."""
import numpy as np


def _directed(faces):
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    return np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])


def edge_face_counts(faces):
    """-> (edges (E, 2) with edges[:, 0] < edges[:, 1], sorted; counts (E,)): faces on every undirected edge (an edge
    between a vertex and itself, from a face with a repeated index, is listed too)."""
    d = np.sort(_directed(faces), axis=1)
    if len(d) == 0:
        return np.zeros((0, 2), np.int64), np.zeros(0, np.int64)
    return np.unique(d, axis=0, return_counts=True)


def is_oriented_manifold(faces, closed=True):
    """Every undirected edge has two faces (closed) or one or two, and every directed edge appears at most once: an
    interior edge is traversed once in each direction."""
    d = _directed(faces)
    if len(d) == 0:
        return False
    if len(np.unique(d, axis=0)) != len(d):
        return False
    _, c = edge_face_counts(faces)
    return bool(np.all(c == 2)) if closed else bool(np.all((c == 1) | (c == 2)))


def euler_characteristic(faces):
    """V - E + F over the vertices the faces reference."""
    f = np.asarray(faces).reshape(-1, 3)
    e, _ = edge_face_counts(f)
    return int(len(np.unique(f)) - len(e) + len(f))


def boundary_loops(faces):
    """Number of closed loops that the edges with exactly one face form (0 for a closed mesh).  Every border vertex must
    have one incoming and one outgoing border edge, else ValueError."""
    d = _directed(faces)
    key = np.sort(d, axis=1)
    e, inv, c = np.unique(key, axis=0, return_inverse=True, return_counts=True)
    b = d[c[inv.reshape(-1)] == 1]
    if len(b) == 0:
        return 0
    nxt = {}
    for a0, a1 in b:
        if int(a0) in nxt:
            raise ValueError("border vertex %d has two outgoing border edges" % a0)
        nxt[int(a0)] = int(a1)
    seen, loops = set(), 0
    for s in nxt:
        if s in seen:
            continue
        loops += 1
        x = s
        while x not in seen:
            seen.add(x)
            if x not in nxt:
                raise ValueError("border path ends at vertex %d" % x)
            x = nxt[x]
        if x != s:
            raise ValueError("border path from %d runs into another loop" % s)
    return loops


def border_vertices(faces):
    d = _directed(faces)
    key = np.sort(d, axis=1)
    _, inv, c = np.unique(key, axis=0, return_inverse=True, return_counts=True)
    return np.unique(d[c[inv.reshape(-1)] == 1])


def signed_volume(vertices, faces):
    v = np.asarray(vertices, dtype=np.float64)
    t = v[np.asarray(faces).reshape(-1, 3)]
    return float(np.einsum("ij,ij->i", t[:, 0], np.cross(t[:, 1], t[:, 2])).sum() / 6.0)


def no_repeated_index(faces):
    f = np.asarray(faces).reshape(-1, 3)
    return bool(np.all((f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])))


def indices_valid(vertices, faces, all_referenced=True):
    """Every index inside [0, V), and (all_referenced) every vertex named by a face."""
    f = np.asarray(faces).reshape(-1, 3)
    n = len(np.asarray(vertices))
    if len(f) and (f.min() < 0 or f.max() >= n):
        return False
    return (not all_referenced) or len(np.unique(f)) == n


def bbox_diagonal(vertices, faces):
    p = np.asarray(vertices, dtype=np.float64)[np.unique(np.asarray(faces))]
    return float(np.linalg.norm(p.max(0) - p.min(0)))


def probe_points(vertices, faces):
    """The points E() measures from: the referenced vertices, then the face centroids."""
    v = np.asarray(vertices, dtype=np.float64)
    f = np.asarray(faces).reshape(-1, 3)
    return np.concatenate([v[np.unique(f)], v[f].mean(axis=1)])


def mesh_error(a, b, diag, dist):
    """E(A, B): the larger of the two one-sided maxima over probe_points of the exact distance to the other mesh, over
    `diag`.  dist(vertices, faces, points) -> distances."""
    ab = np.asarray(dist(b[0], b[1], probe_points(*a))).max()
    ba = np.asarray(dist(a[0], a[1], probe_points(*b))).max()
    return float(max(ab, ba) / diag)


def check_closed_result(v_in, f_in, v_out, f_out, target):
    """The conditions of a simplified closed fixture; returns a list of the ones that fail."""
    bad = []
    if not indices_valid(v_out, f_out):
        bad.append("indices")
    if not no_repeated_index(f_out):
        bad.append("repeated index")
    if not is_oriented_manifold(f_out, closed=True):
        bad.append("not a closed oriented manifold")
    if euler_characteristic(f_out) != euler_characteristic(f_in):
        bad.append("Euler characteristic %d != %d" % (euler_characteristic(f_out), euler_characteristic(f_in)))
    if not signed_volume(v_out, f_out) * signed_volume(v_in, f_in) > 0:
        bad.append("signed volume changed sign")
    if not target - 2 <= len(f_out) <= target:
        bad.append("%d faces outside [%d, %d]" % (len(f_out), target - 2, target))
    return bad

"""numpy references of slice3d_amd/mesh_topology.py (tests/test_mesh_topology.py, tests/test_gpu_mesh_topology.py): weld,
union-find components, the per-component table built from tests/simplify_ref.py, keep; and the hand-made meshes both test
files use.  Vertices (V, 3) float64, faces (F, 3) integer."""
import numpy as np

import simplify_ref as sr

COUNT_COLUMNS = ("faces", "vertices", "edges", "edges_1", "edges_2", "edges_3plus", "conflicts", "degenerate", "euler",
                 "closed_oriented", "oriented_with_border")


def weld(vertices, faces):
    """-> vmap (V,) int64: the smallest index among the referenced vertices at the same position (-0.0 equals +0.0); a
    vertex that no face references maps to itself.  ValueError for a referenced vertex that is not finite."""
    v = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    vmap = np.arange(len(v), dtype=np.int64)
    used = np.unique(f)
    if len(used) == 0:
        return vmap
    p = v[used] + 0.0                                  # -0.0 + 0.0 = +0.0
    if not np.isfinite(p).all():
        raise ValueError("a referenced vertex is not finite")
    _, inv = np.unique(p.view(np.int64), axis=0, return_inverse=True)   # equal bits after the zeros are folded
    inv = inv.reshape(-1)
    first = np.full(inv.max() + 1, len(v), dtype=np.int64)
    np.minimum.at(first, inv, used)
    vmap[used] = first[inv]
    return vmap


def components(faces, n_vertices):
    """Union-find over the faces' vertices -> (K, face_component (F,), vertex_component (V,), -1 for an unreferenced
    vertex); ids ascend with the component's smallest vertex index."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    parent = np.arange(n_vertices, dtype=np.int64)

    def find(x):
        r = x
        while parent[r] != r:
            r = parent[r]
        while parent[x] != r:
            parent[x], x = r, parent[x]
        return r

    for a, b, c in f.tolist():
        ra, rb, rc = find(a), find(b), find(c)
        m = min(ra, rb, rc)
        parent[ra] = parent[rb] = parent[rc] = m
    vcomp = np.full(n_vertices, -1, dtype=np.int64)
    used = np.unique(f)
    roots = np.array([find(int(x)) for x in used], dtype=np.int64)
    ids = {int(r): i for i, r in enumerate(np.unique(roots))}          # the root is the smallest vertex of its component
    if len(used):
        vcomp[used] = [ids[int(r)] for r in roots]
    fcomp = vcomp[f[:, 0]] if len(f) else np.zeros(0, dtype=np.int64)
    return len(ids), fcomp, vcomp


def conflicts(faces):
    """Directed edges that occur more than once."""
    d = sr._directed(faces)
    if len(d) == 0:
        return 0
    _, c = np.unique(d, axis=0, return_counts=True)
    return int((c > 1).sum())


def _cross(a, b):
    """(x, y, z) of a x b for (n, 3) arrays"""
    return (a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0])


def row(vertices, faces):
    """(counts dict, area, volume, area terms' absolute sum, volume terms' absolute sum, bbox (6,)) of one face list."""
    v = np.asarray(vertices, dtype=np.float64)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    _, c = sr.edge_face_counts(f)
    counts = dict(faces=len(f), vertices=len(np.unique(f)), edges=len(c), edges_1=int((c == 1).sum()),
                  edges_2=int((c == 2).sum()), edges_3plus=int((c >= 3).sum()), conflicts=conflicts(f),
                  degenerate=int(len(f) - np.count_nonzero((f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2]))),
                  euler=sr.euler_characteristic(f) if len(f) else 0,
                  closed_oriented=sr.is_oriented_manifold(f, closed=True),
                  oriented_with_border=sr.is_oriented_manifold(f, closed=False))
    t = v[f]
    # the terms, every product and sum rounded on its own in this order (what the device code computes per face, too)
    n = _cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    a = 0.5 * np.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2])
    m = _cross(t[:, 1], t[:, 2])
    d = ((t[:, 0, 0] * m[0] + t[:, 0, 1] * m[1]) + t[:, 0, 2] * m[2]) / 6.0
    p = t.reshape(-1, 3)
    bbox = np.concatenate([p.min(0), p.max(0)]) if len(p) else np.zeros(6)
    return counts, float(a.sum()), float(d.sum()), float(np.abs(a).sum()), float(np.abs(d).sum()), bbox


def topology(vertices, faces, weld_first=False):
    """-> dict(n_components, vmap, face_component, vertex_component, table, summary, tol): table and summary as
    slice3d_amd.mesh_topology's, tol = per row (area bound, volume bound) of the GPU tests' float64 tolerance
    (n + 16) 2^-52 sum|term|, the summary's last."""
    v = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    vmap = weld(v, f) if weld_first else np.arange(len(v), dtype=np.int64)
    w = vmap[f]
    k, fcomp, vc = components(w, len(v))
    vcomp = np.where(np.isin(np.arange(len(v)), np.unique(f)), vc[vmap], -1)
    rows = [row(v, w[fcomp == i]) for i in range(k)] + [row(v, w)]
    cols = {name: np.array([r[0][name] for r in rows]) for name in COUNT_COLUMNS}
    cols["area"], cols["volume"] = np.array([r[1] for r in rows]), np.array([r[2] for r in rows])
    cols["bbox"] = np.array([r[5] for r in rows]).reshape(-1, 6)
    eps = 2.0 ** -52
    tol = np.array([[(r[0]["faces"] + 16) * eps * r[3], (r[0]["faces"] + 16) * eps * r[4]] for r in rows])
    return dict(n_components=k, vmap=vmap, face_component=fcomp, vertex_component=vcomp,
                table={n: c[:-1] for n, c in cols.items()}, summary={n: c[-1] for n, c in cols.items()}, tol=tol)


def keep(vertices, faces, face_component, mask, vmap=None, drop_degenerate=False):
    """The faces of the components `mask` selects in their order, the vertices they reference in ascending index, remapped."""
    v = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    w = f if vmap is None else np.asarray(vmap)[f]
    sel = np.asarray(mask, dtype=bool)[face_component] if len(f) else np.zeros(0, dtype=bool)
    if drop_degenerate:
        sel = sel & (w[:, 0] != w[:, 1]) & (w[:, 1] != w[:, 2]) & (w[:, 0] != w[:, 2])
    kept = w[sel]
    used = np.unique(kept)
    remap = np.full(len(v), -1, dtype=np.int64)
    remap[used] = np.arange(len(used))
    return v[used], remap[kept].reshape(-1, 3)


def soup(vertices, faces, seed=0):
    """Every face gets its own three vertices, shuffled: (3 F, 3) vertices, (F, 3) faces."""
    v = np.asarray(vertices, dtype=np.float64)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    perm = np.random.default_rng(seed).permutation(3 * len(f))          # new index of corner i
    vs = np.empty((3 * len(f), 3))
    vs[perm] = v[f.reshape(-1)]
    return vs, perm.reshape(-1, 3).astype(np.int64)


def strip(n, seed, cuts=0):
    """n triangles (i, i + 1, i + 2) on two rows of vertices; `cuts` times two neighbouring triangles are left out, which
    parts the strip; vertex numbering and face order are seeded permutations."""
    rng = np.random.default_rng(seed)
    f = np.stack([np.arange(n), np.arange(n) + 1, np.arange(n) + 2], 1)
    f[1::2] = f[1::2, ::-1]
    keep = np.ones(n, dtype=bool)
    for c in range(1, cuts + 1):
        at = c * n // (cuts + 1)
        keep[at:at + 2] = False
    v = np.stack([np.arange(n + 2) // 2, np.arange(n + 2) % 2, np.zeros(n + 2)], 1).astype(np.float64)
    pv = rng.permutation(n + 2)
    vs = np.empty_like(v)
    vs[pv] = v
    return vs, pv[f[keep]][rng.permutation(int(keep.sum()))].astype(np.int64)


# ------------------------------------------------------------------------------------------------ hand-made meshes
_TET_V = np.array([[1.0, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]])
_TET_F = np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]], dtype=np.int64)

HAND_MADE = ["tetrahedron", "two_tetrahedra_one_vertex", "three_faces_one_edge", "flipped_face", "repeated_index",
             "unreferenced_vertex"]


def hand_made(name):
    if name == "tetrahedron":
        return _TET_V.copy(), _TET_F.copy()
    if name == "two_tetrahedra_one_vertex":          # the tetrahedron and its mirror image through its vertex 3
        v = np.concatenate([_TET_V, 2.0 * _TET_V[3] - _TET_V[:3]])
        g = np.array([4, 5, 6, 3], dtype=np.int64)[_TET_F][:, ::-1]      # the point reflection turns the faces over
        return v, np.concatenate([_TET_F, g])
    if name == "three_faces_one_edge":               # a book of three pages on the edge 0-1
        v = np.array([[0.0, 0, 0], [0, 0, 1], [1, 0, 0], [-1, 1, 0], [-1, -1, 0]])
        return v, np.array([[0, 1, 2], [0, 1, 3], [0, 1, 4]], dtype=np.int64)
    if name == "flipped_face":
        f = _TET_F.copy()
        f[2] = f[2, ::-1]
        return _TET_V.copy(), f
    if name == "repeated_index":                     # a tetrahedron and a face that names vertex 4 twice, hung on vertex 0
        v = np.concatenate([_TET_V, [[3.0, 3, 3]]])
        return v, np.concatenate([_TET_F, [[0, 4, 4]]]).astype(np.int64)
    if name == "unreferenced_vertex":                # vertices 0 and 5 are named by no face
        v = np.concatenate([[[9.0, 9, 9]], _TET_V, [[-9.0, 0, 0]]])
        return v, _TET_F + 1
    raise KeyError(name)

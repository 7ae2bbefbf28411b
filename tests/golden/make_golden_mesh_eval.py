"""Runs the REFERENCE's mesh scoring (reg_slices/src/utils_eval.py: compute_iou, eval_chamfer, eval_hausdoff, and
check_mesh_contains of src_convonet/utils/libmesh/inside_mesh.py) on meshes from this package's host marching cubes and
stores inputs and results in tests/golden/mesh_eval_reference.npz (authoring container only).

The reference's one compiled module on this path, libmesh/triangle_hash.pyx, is replaced by a pure-Python cell list
(_TriangleHash below, checked here against a brute-force listing) injected into sys.modules; nothing of the reference is
compiled or copied.

    python tests/golden/make_golden_mesh_eval.py
"""
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle.ref_import import REG_SLICES  # noqa: E402
from slice3d_amd.mesh import marching_cubes  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
RES = 512


def _c_int(x):
    """C's (int) of a double on x86 (cvttsd2si): truncation, INT_MIN for NaN and out-of-range values."""
    if not np.isfinite(x) or not (-2147483649.0 < x < 2147483648.0):
        return -2147483648
    return int(x)


class _TriangleHash:
    """triangle_hash.pyx:10-88 in Python: cell res*x + y lists the triangles whose (int)-truncated, clamped xy box covers
    it, in triangle order; query returns (point, triangle) pairs of each point's cell as int32 arrays."""

    def __init__(self, triangles, resolution):
        self.resolution = resolution
        self.spatial_hash = [[] for _ in range(resolution * resolution)]
        for i_tri in range(triangles.shape[0]):
            t = triangles[i_tri]
            lo = [min(max(_c_int(min(t[0, j], t[1, j], t[2, j])), 0), resolution - 1) for j in range(2)]
            hi = [min(max(_c_int(max(t[0, j], t[1, j], t[2, j])), 0), resolution - 1) for j in range(2)]
            for x in range(lo[0], hi[0] + 1):
                for y in range(lo[1], hi[1] + 1):
                    self.spatial_hash[resolution * x + y].append(i_tri)

    def query(self, points):
        pi, ti = [], []
        for i in range(points.shape[0]):
            x, y = _c_int(points[i, 0]), _c_int(points[i, 1])
            if not (0 <= x < self.resolution and 0 <= y < self.resolution):
                continue
            for t in self.spatial_hash[self.resolution * x + y]:
                pi.append(i)
                ti.append(t)
        return np.array(pi, dtype=np.int32), np.array(ti, dtype=np.int32)


def check_hash_brute(triangles, points, res):
    """The stand-in against a brute-force listing: every triangle whose box holds the point's cell, in triangle order."""
    h = _TriangleHash(triangles, res)
    pi, ti = h.query(points)
    bp, bt = [], []
    for i in range(points.shape[0]):
        x, y = _c_int(points[i, 0]), _c_int(points[i, 1])
        if not (0 <= x < res and 0 <= y < res):
            continue
        for k in range(triangles.shape[0]):
            t = triangles[k]
            lo = [min(max(_c_int(t[:, j].min()), 0), res - 1) for j in range(2)]
            hi = [min(max(_c_int(t[:, j].max()), 0), res - 1) for j in range(2)]
            if lo[0] <= x <= hi[0] and lo[1] <= y <= hi[1]:
                bp.append(i)
                bt.append(k)
    assert np.array_equal(pi, np.array(bp, dtype=np.int32)) and np.array_equal(ti, np.array(bt, dtype=np.int32))
    return len(pi)


def import_reference():
    mod = types.ModuleType("src_convonet.utils.libmesh.triangle_hash")
    mod.TriangleHash = _TriangleHash
    sys.modules["src_convonet.utils.libmesh.triangle_hash"] = mod
    if REG_SLICES not in sys.path:
        sys.path.insert(0, REG_SLICES)
    from src_convonet.utils.libmesh import inside_mesh
    sys.path.insert(0, os.path.join(REG_SLICES, "src"))
    import utils_eval
    return inside_mesh, utils_eval


def grid(n):
    return np.stack(np.meshgrid(*[np.linspace(-1, 1, n)] * 3, indexing="ij"), -1)


def mc(field, n):
    v, f = marching_cubes(field, 0.0)
    return v * (2.0 / (n - 1)) - 1.0, f          # index units -> [-1, 1]


def meshes():
    out = {}
    g = grid(22)
    out["sphere"] = mc(0.7 - np.linalg.norm(g - 0.03, axis=-1), 22)
    g = grid(26)
    q = np.sqrt(g[..., 0] ** 2 + g[..., 1] ** 2) - 0.55          # torus around the z axis: z rays cross the hole
    out["torus"] = mc(0.25 - np.sqrt(q ** 2 + g[..., 2] ** 2), 26)
    g = grid(25)                                                    # spacing 1/12: box faces on grid-cell midplanes

    def box(c, h):
        return np.min(h - np.abs(g - np.asarray(c)), axis=-1)
    f = np.maximum(box([-0.5, -0.5, 0.0], [0.29, 0.29, 0.54]), box([0.45, 0.45, 0.1], [0.21, 0.375, 0.29]))
    f = np.maximum(f, box([0.0, 0.0, -0.7], [0.79, 0.79, 0.04]))   # thin plate
    out["boxes"] = mc(f, 25)
    v, fc = out["sphere"]
    fc = np.concatenate([fc, [[0, 0, 1], [2, 3, 3]]])               # zero-area triangles (repeated vertices)
    v2 = np.concatenate([v, [[0.1, 0.2, 0.3], [0.2, 0.3, 0.4], [0.3, 0.4, 0.5]]])
    fc = np.concatenate([fc, [[len(v), len(v) + 1, len(v) + 2]]])   # collinear vertices: zero area
    out["zero_area"] = (v2, fc)
    out["flat"] = (np.array([[-0.5, -0.5, 0.2], [0.5, -0.5, 0.2], [0.5, 0.5, 0.2], [-0.5, 0.5, 0.2]]),
                   np.array([[0, 1, 2], [0, 2, 3]]))
    return out


def exact_rescaled(val, scale, translate, rng):
    """A float64 coordinate x with scale*x + translate == val exactly (searched around the algebraic inverse)."""
    x = (val - translate) / scale
    for _ in range(64):
        r = scale * x + translate
        if r == val:
            return x
        x = np.nextafter(x, np.inf if r < val else -np.inf)
    return None


def points_for(v, f, rng, n_uniform=3000):
    tri = v[f]
    lo, hi = tri.reshape(-1, 3).min(0), tri.reshape(-1, 3).max(0)
    ext = np.maximum(hi - lo, 1e-3)
    pts = [rng.uniform(lo - 0.2 * ext, hi + 0.2 * ext, (n_uniform, 3))]
    with np.errstate(all="ignore"):
        scale = (RES - 1) / (hi - lo)
        translate = 0.5 - scale * lo
    crafted = []
    if np.all(np.isfinite(scale)):
        inner = rng.uniform(lo + 0.1 * ext, hi - 0.1 * ext, (60, 3))
        for k, p in enumerate(inner):
            q = p.copy()
            axis = k % 2
            if k % 3 == 2:
                val = float(RES)                                    # == res: outside (x or y == res)
            else:
                val = float(np.floor(scale[axis] * q[axis] + translate[axis]))   # an integer: a cell boundary
            x = exact_rescaled(val, scale[axis], translate[axis], rng)
            if x is not None:
                q[axis] = x
                crafted.append(q)
        for corner in (lo, hi):                                     # bbox corners: rescaled 0.5 / res - 0.5
            crafted.append(corner.copy())
    # on vertices and edge midpoints in xy, at depths inside the box
    sel = rng.choice(len(f), size=min(len(f), 150), replace=False)
    for t in tri[sel]:
        z = rng.uniform(lo[2], hi[2])
        crafted.append([t[0, 0], t[0, 1], z])
        m = 0.5 * (t[0] + t[1])
        crafted.append([m[0], m[1], z])
    pts.append(np.asarray(crafted, dtype=np.float64).reshape(-1, 3))
    return np.concatenate(pts)


def main():
    inside_mesh, utils_eval = import_reference()
    rng = np.random.default_rng(20261016)
    rec = {}
    for name, (v, f) in meshes().items():
        pts = points_for(v, f, rng)
        m = types.SimpleNamespace(vertices=v, faces=f)
        # the stand-in against brute force on a slice of the points (brute force is O(points x faces))
        inter = inside_mesh.MeshIntersector(m, RES)
        tr = inter._triangles[:, :, :2]
        p2 = inter.rescale(pts[:300])[:, :2]
        npairs = check_hash_brute(tr, p2, RES)
        occ = inside_mesh.check_mesh_contains(m, pts)
        rec["%s_v" % name], rec["%s_f" % name], rec["%s_pts" % name], rec["%s_contains" % name] = v, f, pts, occ
        print("%-9s V=%5d F=%5d points=%5d inside=%5d (hash pairs checked: %d)" % (name, len(v), len(f), len(pts),
                                                                                  occ.sum(), npairs))
    # float32 query points (widened to float64 by the rescale) on the sphere
    p32 = rng.uniform(-0.8, 0.8, (2000, 3)).astype(np.float32)
    m = types.SimpleNamespace(vertices=rec["sphere_v"], faces=rec["sphere_f"])
    rec["sphere_pts32"], rec["sphere_contains32"] = p32, inside_mesh.check_mesh_contains(m, p32)
    # compute_iou, incl. an empty union (NaN)
    o1 = rng.uniform(0, 1, (3, 500)).astype(np.float32)
    o2 = rng.uniform(0, 1, (3, 500)).astype(np.float32)
    o1[2], o2[2] = 0.0, 0.0
    rec["iou_occ1"], rec["iou_occ2"] = o1, o2
    with np.errstate(invalid="ignore"):
        rec["iou"] = utils_eval.compute_iou(o1, o2)
    # Chamfer / F-score / Hausdorff on seeded clouds near a unit sphere
    for k, (n1, n2, noise) in enumerate(((3000, 2500, 0.01), (1200, 4000, 0.004))):
        a = rng.standard_normal((n1, 3))
        b = rng.standard_normal((n2, 3))
        a = (a / np.linalg.norm(a, axis=1, keepdims=True) + noise * rng.standard_normal((n1, 3))).astype(np.float32)
        b = (b / np.linalg.norm(b, axis=1, keepdims=True)).astype(np.float32)
        rec["cd%d_p1" % k], rec["cd%d_p2" % k] = a, b
        rec["cd%d_chamfer" % k] = np.array([float(x) for x in utils_eval.eval_chamfer(a, b, f_thresh=0.05)])
        rec["cd%d_hausdorff" % k] = np.array(utils_eval.eval_hausdoff(a, b))
    path = os.path.join(OUT, "mesh_eval_reference.npz")
    np.savez_compressed(path, **rec)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

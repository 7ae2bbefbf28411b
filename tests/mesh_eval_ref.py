"""Host restatement of the reference's point-in-mesh test and a float64 brute-force nearest neighbour — the yardsticks
of slice3d_amd/mesh_eval.py (tests/test_mesh_eval.py pins the restatement to the reference's own output).

contains(): reg_slices/src_convonet/utils/libmesh/inside_mesh.py (MeshIntersector, TriangleIntersector2d) with its
compiled cell hash triangle_hash.pyx (TriangleHash) vectorised in numpy, the float64 expressions in the reference's
order.  Returns (inside, n_disagree): n_disagree counts the points inside the bbox whose two parities differ (the
reference prints a warning for them, inside_mesh.py:66-67)."""
import numpy as np


def _c_int(x):
    """C's (int) of a double as x86 computes it (triangle_hash.pyx:36-39): truncation; NaN and out-of-range -> INT_MIN."""
    x = np.asarray(x, dtype=np.float64)
    ok = np.isfinite(x) & (x > -2147483649.0) & (x < 2147483648.0)
    out = np.full(x.shape, -2147483648, dtype=np.int64)
    out[ok] = np.trunc(x[ok]).astype(np.int64)
    return out


def cell_lists(tri2d, res):
    """triangle_hash.pyx:26-47: (cell, triangle) pairs of every cell res*x + y in each triangle's clamped box, as CSR
    (offsets over res*res cells, triangle ids); order within a cell is the triangle order, as push_back leaves it."""
    lo = np.clip(_c_int(tri2d.min(axis=1)), 0, res - 1)           # (n_tri, 2): pyx:36-41
    hi = np.clip(_c_int(tri2d.max(axis=1)), 0, res - 1)
    nx, ny = hi[:, 0] - lo[:, 0] + 1, hi[:, 1] - lo[:, 1] + 1
    per = nx * ny
    tri = np.repeat(np.arange(len(tri2d)), per)
    k = np.arange(per.sum()) - np.repeat(np.cumsum(per) - per, per)
    x = lo[tri, 0] + k // ny[tri]
    y = lo[tri, 1] + k % ny[tri]
    cell = res * x + y                                             # pyx:45
    order = np.argsort(cell, kind="stable")
    off = np.zeros(res * res + 1, dtype=np.int64)
    np.add.at(off, cell + 1, 1)
    return np.cumsum(off), tri[order]


def contains(vertices, faces, points, res=512):
    triangles = np.asarray(vertices, dtype=np.float64)[np.asarray(faces, dtype=np.int64)]    # inside_mesh.py:13
    n_tri = triangles.shape[0]
    with np.errstate(all="ignore"):
        bbox_min = triangles.reshape(3 * n_tri, 3).min(axis=0)                                 # :17-18
        bbox_max = triangles.reshape(3 * n_tri, 3).max(axis=0)
        scale = (res - 1) / (bbox_max - bbox_min)                                              # :20
        translate = 0.5 - scale * bbox_min                                                     # :21
        triangles = scale * triangles + translate                                              # :23, 135-137
        points = scale * np.asarray(points) + translate                                        # :33
    n = len(points)
    inside = np.zeros(n, dtype=bool)
    inside_aabb = np.all((0 <= points) & (points <= res), axis=1)                              # :40-41
    if not inside_aabb.any():
        return inside, 0
    pts = points[inside_aabb]
    # TriangleHash.query (pyx:60-71): the triangles of each point's cell
    off, cell_tri = cell_lists(triangles[:, :, :2], res)
    x, y = _c_int(pts[:, 0]), _c_int(pts[:, 1])
    ok = (0 <= x) & (x < res) & (0 <= y) & (y < res)
    cell = np.where(ok, res * x + y, 0)
    cnt = np.where(ok, off[cell + 1] - off[cell], 0)
    pidx = np.repeat(np.arange(len(pts)), cnt)
    k = np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    tidx = cell_tri[off[cell][pidx] + k]
    # TriangleIntersector2d.check_triangles (inside_mesh.py:120-139)
    tri2 = triangles[tidx][:, :, :2]
    p2 = pts[pidx][:, :2]
    A = tri2[:, :2] - tri2[:, 2:]
    A = A.transpose([0, 2, 1])
    yv = p2 - tri2[:, 2]
    detA = A[:, 0, 0] * A[:, 1, 1] - A[:, 0, 1] * A[:, 1, 0]
    mask = np.abs(detA) != 0.
    with np.errstate(all="ignore"):
        s_detA = np.sign(detA)
        abs_detA = np.abs(detA)
        u = (A[:, 1, 1] * yv[:, 0] - A[:, 0, 1] * yv[:, 1]) * s_detA
        v = (-A[:, 1, 0] * yv[:, 0] + A[:, 0, 0] * yv[:, 1]) * s_detA
        sum_uv = u + v
        hit = mask & (0 < u) & (u < abs_detA) & (0 < v) & (v < abs_detA) & (0 < sum_uv) & (sum_uv < abs_detA)
    pidx, tidx = pidx[hit], tidx[hit]
    # compute_intersection_depth (inside_mesh.py:74-104)
    t = triangles[tidx]
    p = pts[pidx]
    t1, t2, t3 = t[:, 0, :], t[:, 1, :], t[:, 2, :]
    normals = np.cross(t3 - t1, t2 - t1)
    alpha = np.sum(normals[:, :2] * (t1[:, :2] - p[:, :2]), axis=1)
    n_2 = normals[:, 2]
    abs_n_2 = np.abs(n_2)
    m = abs_n_2 != 0
    depth = np.full(len(p), np.nan)
    depth[m] = t1[m, 2] * abs_n_2[m] + alpha[m] * np.sign(n_2[m])
    with np.errstate(invalid="ignore"):
        smaller = depth >= p[:, 2] * abs_n_2                                                   # :56-57
        bigger = depth < p[:, 2] * abs_n_2
    n0 = np.bincount(pidx[smaller], minlength=len(pts))
    n1 = np.bincount(pidx[bigger], minlength=len(pts))
    c1, c2 = np.mod(n0, 2) == 1, np.mod(n1, 2) == 1                                            # :64-65
    inside[inside_aabb] = c1 & c2
    return inside, int((c1 != c2).sum())


def nn_brute(a, b, chunk=1024, k=4):
    """float64 brute force -> (d2, idx, d2_second): the squared distance of every point of a to its nearest point of b,
    its index (the lowest on ties) and the second-nearest squared distance (for index checks).  The k nearest
    candidates come from the |a|^2 - 2a.b + |b|^2 expansion in float64 (error ~1e-15, far below the spacing of the
    test clouds); their distances are then recomputed from coordinate differences."""
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    k = min(k, len(b))
    bb = (b * b).sum(1)
    d1 = np.empty(len(a))
    d2nd = np.full(len(a), np.inf)
    idx = np.empty(len(a), dtype=np.int64)
    for s in range(0, len(a), chunk):
        aa = a[s:s + chunk]
        approx = (aa * aa).sum(1)[:, None] - 2.0 * aa @ b.T + bb[None, :]
        cand = np.argpartition(approx, k - 1, axis=1)[:, :k] if k < len(b) else np.tile(np.arange(len(b)), (len(aa), 1))
        diff = aa[:, None, :] - b[cand]
        d = (diff * diff).sum(-1)
        order = np.lexsort((cand, d), axis=-1)             # by distance, then by index
        d = np.take_along_axis(d, order, 1)
        cand = np.take_along_axis(cand, order, 1)
        d1[s:s + chunk], idx[s:s + chunk] = d[:, 0], cand[:, 0]
        if k > 1:
            d2nd[s:s + chunk] = d[:, 1]
    return d1, idx, d2nd

"""Host yardsticks of slice3d_amd/mesh_sdf.py: numpy float64, brute force over all faces.

  dist_a   closest point by Voronoi-region classification (Ericson, Real-Time Collision Detection 5.1.5)
  dist_b   independently: the foot of the perpendicular where it falls inside the face, else the minimum over the three
           clamped edge segments
  winding  the generalised winding number by the Van Oosterom-Strackee atan2 form, summed with math.fsum (exactly
           rounded sum)

A and B are two formulations of one quantity; their disagreement is the yardstick's own error.  The code under test is
never the yardstick."""
import math

import numpy as np


def _dot(a, b):
    return (a * b).sum(-1)


def point_tri_a(p, a, b, c):
    """Distance from points p (..., 3) to triangles (a, b, c) (..., 3), broadcast; Ericson's region classification."""
    p, a, b, c = np.broadcast_arrays(p, a, b, c)
    ab, ac, ap = b - a, c - a, p - a
    d1, d2 = _dot(ab, ap), _dot(ac, ap)
    bp = p - b
    d3, d4 = _dot(ab, bp), _dot(ac, bp)
    cp = p - c
    d5, d6 = _dot(ab, cp), _dot(ac, cp)
    vc = d1 * d4 - d3 * d2
    vb = d5 * d2 - d1 * d6
    va = d3 * d6 - d5 * d4
    with np.errstate(all="ignore"):
        t_ab = d1 / (d1 - d3)
        t_ac = d2 / (d2 - d6)
        t_bc = (d4 - d3) / ((d4 - d3) + (d5 - d6))
        den = 1.0 / (va + vb + vc)
        v, w = vb * den, vc * den
        q = a + ab * v[..., None] + ac * w[..., None]                               # interior
    done = np.zeros(p.shape[:-1], dtype=bool)

    def put(mask, val):
        nonlocal q, done
        m = mask & ~done
        q = np.where(m[..., None], val, q)
        done |= m

    put((d1 <= 0) & (d2 <= 0), a)
    put((d3 >= 0) & (d4 <= d3), b)
    put((vc <= 0) & (d1 >= 0) & (d3 <= 0), a + ab * t_ab[..., None])
    put((d6 >= 0) & (d5 <= d6), c)
    put((vb <= 0) & (d2 >= 0) & (d6 <= 0), a + ac * t_ac[..., None])
    put((va <= 0) & ((d4 - d3) >= 0) & ((d5 - d6) >= 0), b + (c - b) * t_bc[..., None])
    d = np.sqrt(_dot(p - q, p - q))
    # va + vb + vc is |ab x ac|^2 whatever the point: a face without area has neither an interior for the classification to
    # end in nor, with a repeated vertex, an edge parameter (both divide 0 by 0).  It is the union of its three edges, each
    # a clamped segment (the book's ClosestPtPointSegment, 5.1.2)
    flat = ~(va + vb + vc > 0)
    if flat.any():
        d = np.where(flat, np.minimum(np.minimum(_seg(p, a, b), _seg(p, b, c)), _seg(p, c, a)), d)
    return d


def _seg(p, a, b):
    e = b - a
    den = _dot(e, e)
    with np.errstate(all="ignore"):
        t = np.where(den > 0, _dot(p - a, e) / np.where(den > 0, den, 1.0), 0.0)
    t = np.clip(t, 0.0, 1.0)
    d = p - (a + e * t[..., None])
    return np.sqrt(_dot(d, d))


def point_tri_b(p, a, b, c):
    """The same distance from the plane: |n.(p - a)| / |n| where the foot of the perpendicular is inside all three edge
    half-planes (and the face has a normal), else the nearest of the three edge segments."""
    p, a, b, c = np.broadcast_arrays(p, a, b, c)
    n = np.cross(b - a, c - a)
    nn = _dot(n, n)
    edges = np.minimum(np.minimum(_seg(p, a, b), _seg(p, b, c)), _seg(p, c, a))
    s0 = _dot(np.cross(b - a, p - a), n)
    s1 = _dot(np.cross(c - b, p - b), n)
    s2 = _dot(np.cross(a - c, p - c), n)
    inside = (nn > 0) & (s0 >= 0) & (s1 >= 0) & (s2 >= 0)
    with np.errstate(all="ignore"):
        plane = np.abs(_dot(n, p - a)) / np.sqrt(np.where(nn > 0, nn, 1.0))
    return np.where(inside, np.minimum(plane, edges), edges)


def _brute(fn, vertices, faces, points, chunk):
    tri = np.asarray(vertices, dtype=np.float64)[np.asarray(faces, dtype=np.int64)]
    pts = np.asarray(points, dtype=np.float64)
    a, b, c = tri[None, :, 0], tri[None, :, 1], tri[None, :, 2]
    out = np.empty(len(pts))
    idx = np.empty(len(pts), dtype=np.int64)
    step = max(1, chunk // max(1, len(tri)))
    for s in range(0, len(pts), step):
        d = fn(pts[s:s + step, None, :], a, b, c)
        idx[s:s + step] = d.argmin(axis=1)
        out[s:s + step] = d.min(axis=1)
    return out, idx


def dist_a(vertices, faces, points, chunk=1 << 20):
    """(distance, face index) of every point, formulation A over all faces."""
    return _brute(point_tri_a, vertices, faces, points, chunk)


def dist_b(vertices, faces, points, chunk=1 << 20):
    return _brute(point_tri_b, vertices, faces, points, chunk)


def dist_a_face(vertices, faces, points, face_idx):
    """Formulation A for one given face per point."""
    tri = np.asarray(vertices, dtype=np.float64)[np.asarray(faces, dtype=np.int64)[np.asarray(face_idx)]]
    return point_tri_a(np.asarray(points, dtype=np.float64), tri[:, 0], tri[:, 1], tri[:, 2])


def winding(vertices, faces, points, chunk=1 << 20):
    """w = sum_f Omega_f / 4 pi, Omega_f = 2 atan2(det[a b c], |a||b||c| + (a.b)|c| + (b.c)|a| + (c.a)|b|); the terms of a
    point are summed exactly (math.fsum) and rounded once."""
    tri = np.asarray(vertices, dtype=np.float64)[np.asarray(faces, dtype=np.int64)]
    pts = np.asarray(points, dtype=np.float64)
    out = np.empty(len(pts))
    step = max(1, chunk // max(1, len(tri)))
    for s in range(0, len(pts), step):
        p = pts[s:s + step, None, :]
        a, b, c = tri[None, :, 0] - p, tri[None, :, 1] - p, tri[None, :, 2] - p
        la, lb, lc = np.sqrt(_dot(a, a)), np.sqrt(_dot(b, b)), np.sqrt(_dot(c, c))
        det = _dot(a, np.cross(b, c))
        den = la * lb * lc + _dot(a, b) * lc + _dot(b, c) * la + _dot(c, a) * lb
        omega = 2.0 * np.arctan2(det, den) / (4.0 * math.pi)
        out[s:s + step] = [math.fsum(row) for row in omega]
    return out


def box_distance(lo, hi, points):
    """Closed form: distance from points outside (or on) the axis-aligned box [lo, hi] to it."""
    p = np.asarray(points, dtype=np.float64)
    d = np.maximum(np.maximum(np.asarray(lo) - p, p - np.asarray(hi)), 0.0)
    return np.sqrt((d * d).sum(-1))

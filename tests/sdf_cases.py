"""Point sets of the signed-distance tests (tests/test_mesh_sdf.py checks their preconditions with the host references
alone, tests/test_gpu_mesh_sdf.py runs the device code on them).  The meshes are the fixtures of
tests/golden/mesh_eval_reference.npz, read and not changed."""
import functools
import os

import numpy as np

from helpers import GOLDEN
import mesh_eval_ref
import sdf_ref

CASES = ["sphere", "torus", "boxes", "zero_area", "flat"]
WATERTIGHT = ["sphere", "torus", "boxes"]
SURFACE_TOL = 1e-9           # in bounding-box diagonals: nearer than this, a point counts as "on the surface"
LEFT_OUT_CAP = 0.005
# seeds of the 5 000 uniform points of the sign comparison, picked so that the ray-parity reference reports no point whose
# two parities differ (tests/test_mesh_sdf.py re-checks it)
SIGN_SEEDS = {"sphere": 0, "torus": 0, "boxes": 0}


@functools.lru_cache(maxsize=None)
def gold():
    z = np.load(os.path.join(GOLDEN, "mesh_eval_reference.npz"))
    return {k: z[k] for k in z.files}


def mesh(name):
    """(vertices, faces) of a fixture, or of "open_sphere": the sphere without the faces whose centroid has z > 0.5."""
    g = gold()
    if name == "open_sphere":
        v, f = g["sphere_v"], g["sphere_f"]
        return v, f[v[f].mean(axis=1)[:, 2] <= 0.5]
    return g[name + "_v"], g[name + "_f"]


def bbox(name):
    v, f = mesh(name)
    used = v[f.reshape(-1)]
    lo, hi = used.min(axis=0), used.max(axis=0)
    return lo, hi, float(np.linalg.norm(hi - lo))


def _uniform(rng, lo, hi, factor, n):
    # an axis on which the bounding box is flat takes the diagonal as its extent: `factor` times nothing would put every
    # point into the mesh's own plane
    c, half = 0.5 * (lo + hi), 0.5 * factor * np.where(hi - lo > 0, hi - lo, np.linalg.norm(hi - lo))
    return rng.uniform(c - half, c + half, (n, 3))


def crafted(name):
    return gold()[("sphere" if name == "open_sphere" else name) + "_pts"]


@functools.lru_cache(maxsize=None)
def distance_points(name):
    """GPU item 1: the fixture's crafted points, 2 000 uniform in a box 3x the bounding box, 200 at 10 - 100 diagonals,
    every 7th vertex, 300 edge midpoints and 300 face centroids (the last three at distance 0 up to rounding).
    -> (points, index of the first on-surface point)."""
    v, f = mesh(name)
    lo, hi, diag = bbox(name)
    rng = np.random.default_rng(100 + CASES.index(name))
    d = rng.standard_normal((200, 3))
    far = 0.5 * (lo + hi) + d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(10, 100, (200, 1)) * diag
    fe = f[rng.integers(0, len(f), 300)]
    k = rng.integers(0, 3, 300)
    mid = 0.5 * (v[fe[np.arange(300), k]] + v[fe[np.arange(300), (k + 1) % 3]])
    cen = v[f[rng.integers(0, len(f), 300)]].mean(axis=1)
    off = [crafted(name), _uniform(rng, lo, hi, 3.0, 2000), far]
    on = [v[np.unique(f)][::7], mid, cen]
    return np.concatenate(off + on), sum(len(x) for x in off)


@functools.lru_cache(maxsize=None)
def reference_distances(name):
    """(d_A, d_B) on distance_points(name): computed once per process."""
    v, f = mesh(name)
    pts = distance_points(name)[0]
    return sdf_ref.dist_a(v, f, pts)[0], sdf_ref.dist_b(v, f, pts)[0]


def tolerance(name):
    """T = max(16 max|d_A - d_B|, 64 * 2^-52 * (diag + max|p|)) on distance_points(name) -> (T, first term, second term)."""
    da, db = reference_distances(name)
    pts = distance_points(name)[0]
    t1 = 16.0 * float(np.abs(da - db).max())
    t2 = 64.0 * 2.0 ** -52 * (bbox(name)[2] + float(np.abs(pts).max()))
    return max(t1, t2), t1, t2


@functools.lru_cache(maxsize=None)
def winding_points(name):
    """GPU item 5: crafted points + 2 000 uniform in a box 1.5x the bounding box, minus the points nearer to the surface
    than SURFACE_TOL diagonals (there w jumps, and two correct evaluations may land on either side).  Where more than
    LEFT_OUT_CAP of that set would be left out, the crafted points are not part of the set at all.
    -> (points, share left out, whether the crafted points are in)."""
    v, f = mesh(name)
    lo, hi, diag = bbox(name)
    uni = _uniform(np.random.default_rng(200 + (CASES + ["open_sphere"]).index(name)), lo, hi, 1.5, 2000)
    pts = np.concatenate([crafted(name), uni])
    near = sdf_ref.dist_a(v, f, pts)[0] < SURFACE_TOL * diag
    with_crafted = near.mean() <= LEFT_OUT_CAP
    if not with_crafted:
        pts, near = uni, near[len(crafted(name)):]
    return pts[~near], float(near.mean()), with_crafted


@functools.lru_cache(maxsize=None)
def sign_points(name):
    """GPU item 6: 5 000 seeded uniform points in a box 1.2x the bounding box -> (points, d_A, parity disagreements)."""
    v, f = mesh(name)
    lo, hi, _ = bbox(name)
    pts = _uniform(np.random.default_rng(SIGN_SEEDS[name]), lo, hi, 1.2, 5000)
    return pts, sdf_ref.dist_a(v, f, pts)[0], mesh_eval_ref.contains(v, f, pts)[1]

"""Cases of the mesh-render tests: the fixtures of tests/golden/mesh_eval_reference.npz (read, not changed), each
normalised with mesh_sdf.normalize_mesh, and the cameras they are rendered with.  tests/test_mesh_render.py checks the
preconditions with the float64 reference alone; tests/test_gpu_mesh_render.py runs the device code on the same cases.
References are computed once per process and shared."""
import functools

import numpy as np

import render_ref
import sdf_cases
from slice3d_amd.mesh_sdf import normalize_mesh

CASES = ["sphere", "torus", "boxes", "zero_area", "flat"]
BASE = dict(az=0.7, el=0.3, distance=1.2, scale=0.9, offset=(0.03, -0.02, 0.04), size=32, S=2, slice_direction="camera")
FLAG_CAP = 0.001

# Shapes that break binning (name -> (fixture, camera overrides)).  Tile edges default to 16 / S pixels.
#   size 36 / 5: no multiple of a tile; S 1 / 4: the other sample counts; scale 3.0 on the sphere: the object fills the
#   image and every tile holds several LDS chunks of 128 faces; scale 5.0: the camera is inside the sphere (radius 1.44 >
#   distance 1.2), with faces behind it and across p_z = 0, which go to every tile; flat: 2 faces, most tiles empty.
VARIANTS = {
    "size36": ("torus", dict(size=36)),
    "size5_s4": ("sphere", dict(size=5, S=4)),
    "s1": ("zero_area", dict(S=1)),
    "s4": ("torus", dict(size=12, S=4)),
    "scale3": ("sphere", dict(scale=3.0, size=16)),
    "scale5_inside": ("sphere", dict(scale=5.0, size=16)),
    "boxes36": ("boxes", dict(size=36, S=1)),
    "flat5": ("flat", dict(size=5, S=4)),
    "axis": ("torus", dict(slice_direction="axis")),
    "axis_boxes": ("boxes", dict(slice_direction="axis", size=16)),
}


@functools.lru_cache(maxsize=None)
def mesh(name):
    v, f = sdf_cases.mesh(name)
    return normalize_mesh(v), np.ascontiguousarray(f, dtype=np.int64)


def camera(key):
    """(fixture name, camera dict) of a case name (the base camera) or a VARIANTS key."""
    if key in VARIANTS:
        name, over = VARIANTS[key]
        cam = dict(BASE)
        cam.update(over)
        return name, cam
    return key, dict(BASE)


@functools.lru_cache(maxsize=None)
def reference(key):
    name, cam = camera(key)
    v, f = mesh(name)
    out = render_ref.render(v, f, **cam)
    for x in out.values():
        if isinstance(x, np.ndarray):
            x.setflags(write=False)
    return out


def flagged(ref):
    """(13, W, W) bool: samples on which two correct evaluations may differ (an edge, a slab boundary or a depth tie)."""
    return ref["tie"] | ref["edge"][None] | ref["slab"][None]


def tolerance(ref, distance):
    """T = max(16 max|s_A - s_B|, 64 * 2^-52 * (distance + 1)) -> (T, first term, second term)"""
    got = np.isfinite(ref["depth"])
    t1 = 16.0 * float(np.abs(ref["depth"][got] - ref["depth_b"][got]).max()) if got.any() else 0.0
    t2 = 64.0 * 2.0 ** -52 * (distance + 1.0)
    return max(t1, t2), t1, t2

"""The meshes and targets of the simplification tests (tests/test_mesh_simplify.py checks the reference's recorded outputs
on the host, tests/test_gpu_mesh_simplify.py runs the device code).  The fixtures are those of
tests/golden/mesh_eval_reference.npz, read and not changed; the reference's outputs (libsimplify's mesh_simplify at
aggressiveness 5, recorded by tests/golden/make_golden_simplify.py) are in tests/golden/mesh_simplify_reference.npz."""
import functools
import os

import numpy as np

from helpers import GOLDEN

CLOSED = ["sphere", "torus", "boxes"]
RATIOS = [50, 25, 10]                       # per cent of the input's faces
AGGRESSIVENESS = 5.0                        # what reconstruct.py passes
# item 2: the cases whose error is held against the reference's at half the face budget (boxes at 50 and 25 % are left
# out: there the reference's error is the fixture's own facet noise)
ERROR_CASES = [(n, r) for n in ("sphere", "torus") for r in RATIOS] + [("boxes", 10)]
GENUS1_RES = 64                             # item 3: marching cubes of an analytic torus field on a 64^3 grid
GENUS1_RATIO = 10
OPEN_RATIO = 25


@functools.lru_cache(maxsize=None)
def _fixtures():
    z = np.load(os.path.join(GOLDEN, "mesh_eval_reference.npz"))
    return {k: z[k] for k in z.files if k.endswith(("_v", "_f"))}


@functools.lru_cache(maxsize=None)
def gold():
    z = np.load(os.path.join(GOLDEN, "mesh_simplify_reference.npz"))
    return {k: z[k] for k in z.files}


def genus1_field(n=GENUS1_RES):
    """Positive inside a torus around the z axis (radii 0.62, 0.33) in [-1, 1]^3, float64 (n, n, n)."""
    a = np.linspace(-1.0, 1.0, n)
    x, y, z = np.meshgrid(a, a, a, indexing="ij")
    q = np.sqrt(x * x + y * y) - 0.62
    return 0.33 - np.sqrt(q * q + z * z)


def genus1_transform(vertices, n=GENUS1_RES):
    """Marching-cubes vertices of the padded grid (index units) -> [-1, 1]^3."""
    return (np.asarray(vertices) - 1.0) * (2.0 / (n - 1)) - 1.0


@functools.lru_cache(maxsize=None)
def genus1_host():
    """The mesh of item 3 from the host marching cubes (bit-identical to the device's), on the grid padded with -1e6 as
    Generator3D.extract_mesh pads it."""
    from slice3d_amd.mesh import marching_cubes
    v, f = marching_cubes(np.pad(genus1_field(), 1, "constant", constant_values=-1e6), 0.0)
    return genus1_transform(v), f


def mesh(name):
    """(vertices (V, 3) float64, faces (F, 3) int64)."""
    if name == "open_sphere":     # the sphere without the faces whose centroid has z > 0.5: one boundary loop
        v, f = mesh("sphere")
        keep = f[v[f].mean(axis=1)[:, 2] <= 0.5]
        used = np.unique(keep)
        remap = np.full(len(v), -1, np.int64)
        remap[used] = np.arange(len(used))
        return v[used], remap[keep]
    if name == "genus1":
        return genus1_host()
    if name == "tetrahedron":
        return (np.array([[1.0, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]]),
                np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]], dtype=np.int64))
    if name == "octahedron":
        return (np.array([[1.0, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]]),
                np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]],
                         dtype=np.int64))
    fx = _fixtures()
    return fx[name + "_v"], fx[name + "_f"]


def target(name, ratio):
    return len(mesh(name)[1]) * ratio // 100


def golden_cases():
    """(name, target) of every reference output the golden file holds: each test target T and floor(T / 2)."""
    out = []
    for name in CLOSED:
        for r in RATIOS:
            out += [(name, target(name, r)), (name, target(name, r) // 2)]
    out += [("genus1", target("genus1", GENUS1_RATIO)), ("genus1", target("genus1", GENUS1_RATIO) // 2)]
    out += [("open_sphere", target("open_sphere", OPEN_RATIO)), ("open_sphere", target("open_sphere", OPEN_RATIO) // 2)]
    return sorted(set(out))


def reference(name, t):
    """The reference's (vertices, faces) for `name` at target `t`."""
    g = gold()
    return g["%s_%d_v" % (name, t)], g["%s_%d_f" % (name, t)]

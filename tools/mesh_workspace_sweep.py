"""Records what the mesh units' *_workspace_bytes functions return over a sweep of sizes, as
tests/golden/mesh_workspace_bytes.json (tests/test_mesh_workspace_bytes.py compares the library against it).

The functions are host arithmetic, so no GPU is needed.  The golden is recorded from the library of the commit BEFORE a
change to the workspace layouts, then compared with the library after it:

    python tools/mesh_workspace_sweep.py tests/golden/mesh_workspace_bytes.json     (S3D_HIP_LIB selects the library)
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# (vertices, faces): empty, tiny, one block, a tile boundary (4096 items per scan tile), more than one tile, large, and
# the largest sizes the simplifier and the topology serve
SIZES = [(0, 0), (1, 1), (3, 1), (8, 12), (1000, 2000), (4097, 4096), (65537, 131070), (2**20, 2**21),
         (2**30 - 1, 2**29 - 1)]
CONTAINS_RES = [1, 2, 64, 512, 8192, 8193]          # 1 and 8193 are outside [2, 8192]: 0
DIST_RES = [1, 2, 64, 256, 257]                     # 257 is outside [1, 256]: 0
WINDING_POINTS = [0, 1, 1000, 2**17, 2**17 + 1, 10**6]


def cases():
    """[(function name, argument tuple)]; the entries past a unit's limit must give 0."""
    out = []
    for nv, nf in SIZES:
        out += [("s3d_mesh_contains_workspace_bytes", (nf, r)) for r in CONTAINS_RES]
        out += [("s3d_mesh_dist_workspace_bytes", (nf, r)) for r in DIST_RES]
        out += [("s3d_mesh_winding_workspace_bytes", (nf, n)) for n in WINDING_POINTS]
        out += [("s3d_mesh_render_workspace_bytes", (nv, nf, 256, 4, 8)),
                ("s3d_mesh_render_workspace_bytes", (nv, nf, 256, 4, 9)),       # 9 * 4 samples > 32: a bad tile
                ("s3d_mesh_simplify_workspace_bytes", (nv, nf)),
                ("s3d_mesh_topology_workspace_bytes", (nv, nf, 0)),
                ("s3d_mesh_topology_workspace_bytes", (nv, nf, 1)),
                ("s3d_nn_workspace_bytes", (nv,)),
                ("s3d_surface_sample_workspace_bytes", (nf,))]
    # one past each unit's limit
    out += [("s3d_mesh_contains_workspace_bytes", (-1, 512)),
            ("s3d_mesh_dist_workspace_bytes", (2**31, 64)),
            ("s3d_mesh_winding_workspace_bytes", (0, 1000)),
            ("s3d_mesh_winding_workspace_bytes", (2000, -1)),
            ("s3d_mesh_render_workspace_bytes", (1000, 2**31, 256, 4, 8)),
            ("s3d_mesh_render_workspace_bytes", (1000, 2000, 1025, 4, 8)),
            ("s3d_mesh_simplify_workspace_bytes", (2**31, 1)),
            ("s3d_mesh_simplify_workspace_bytes", (1, 2**29)),
            ("s3d_mesh_topology_workspace_bytes", (2**30, 1, 0)),
            ("s3d_mesh_topology_workspace_bytes", (1, 2**29, 1)),
            ("s3d_nn_workspace_bytes", (-1,)),
            ("s3d_surface_sample_workspace_bytes", (-1,))]
    return out


def sweep(lib):
    """[[function name, [arguments], bytes]] from a loaded library (slice3d_amd._lib.load())."""
    return [[name, list(args), int(getattr(lib, name)(*args))] for name, args in cases()]


if __name__ == "__main__":
    from slice3d_amd import _lib
    rows = sweep(_lib.load())
    with open(sys.argv[1], "w") as fh:
        fh.write("[\n" + ",\n".join(json.dumps(r) for r in rows) + "\n]\n")
    print("%d values from %s" % (len(rows), _lib.LIB_PATH))

"""Times the mesh-evaluation kernels (slice3d_amd/mesh_eval.py, csrc/mesh_eval.hip) with device events, beside the host
yardsticks: the numpy restatement of the reference's point-in-mesh test (tests/mesh_eval_ref.py) and scipy's cKDTree
(what reg_slices/src/utils_eval.py uses) when scipy is installed.

Workload: the mesh marching_cubes_device extracts from an analytic field (torus + sphere) at 257^3 and 100 k points.

    python tools/time_mesh_eval.py [--n 257] [--points 100000] [--reps 10]

Prints one JSON line (milliseconds).
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def device_ms(fn, reps):
    fn()                                     # warm-up: code objects, allocator
    torch.cuda.synchronize()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for _ in range(reps):
        start.record()
        fn()
        end.record()
        end.synchronize()
        times.append(start.elapsed_time(end))
    return float(np.median(times))


def host_ms(fn, reps=1):
    times = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t) * 1e3)
    return float(np.median(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=257)
    ap.add_argument("--points", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    import mesh_eval_ref
    from slice3d_amd.mesh import marching_cubes_device
    from slice3d_amd.mesh_eval import MeshIntersector, nn_sqdist, sample_surface

    n = args.n
    g = torch.linspace(-1, 1, n, dtype=torch.float64, device="cuda")
    x, y, z = torch.meshgrid(g, g, g, indexing="ij")
    q = torch.sqrt(x ** 2 + y ** 2) - 0.5
    field = torch.maximum(0.22 - torch.sqrt(q ** 2 + z ** 2), 0.35 - torch.sqrt((x - 0.3) ** 2 + y ** 2 + (z - 0.35) ** 2))
    v, f = marching_cubes_device(field, 0.0)
    del x, y, z, q, field
    rng = np.random.default_rng(0)
    pts = torch.from_numpy(rng.uniform(0, n - 1, (args.points, 3)).astype(np.float32)).cuda()
    out = {"mesh": {"grid": n, "vertices": int(v.shape[0]), "faces": int(f.shape[0])}, "points": args.points}

    # point-in-mesh: hash build (one synchronisation inside) + query, and the query alone on a built hash
    out["contains_build_query_ms"] = device_ms(lambda: MeshIntersector((v, f)).query(pts), args.reps)
    inter = MeshIntersector((v, f))
    out["contains_query_ms"] = device_ms(lambda: inter.query(pts), args.reps)
    # surface sampling of the points the Chamfer terms use
    out["sample_surface_ms"] = device_ms(lambda: sample_surface((v, f), args.points, seed=0), args.reps)
    a, _ = sample_surface((v, f), args.points, seed=0)
    b, _ = sample_surface((v, f), args.points, seed=1)
    # one direction of the exact nearest neighbour, na = nb = points
    out["nn_one_direction_ms"] = device_ms(lambda: nn_sqdist(a, b), args.reps)
    pairs = float(args.points) ** 2
    out["nn_pairs_per_s"] = pairs / (out["nn_one_direction_ms"] * 1e-3)

    # host yardsticks
    vh, fh, ph = v.cpu().numpy(), f.cpu().numpy(), pts.cpu().numpy()
    out["host_contains_numpy_ms"] = host_ms(lambda: mesh_eval_ref.contains(vh, fh, ph))
    ah, bh = a.cpu().numpy(), b.cpu().numpy()
    try:
        from scipy.spatial import cKDTree
        out["host_ckdtree_build_query_ms"] = host_ms(lambda: cKDTree(bh).query(ah, k=1), 3)
    except ImportError:
        out["host_ckdtree_build_query_ms"] = None
    # agreement at the timed sizes
    ref, _ = mesh_eval_ref.contains(vh, fh, ph)
    out["contains_equal_to_restatement"] = bool(np.array_equal(inter.query(pts).cpu().numpy(), ref))
    print(json.dumps(out))


if __name__ == "__main__":
    main()

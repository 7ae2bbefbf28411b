"""Times the signed-distance kernels (slice3d_amd/mesh_sdf.py, csrc/mesh_sdf.hip) with device events on the stream, beside
the float64 brute force of tests/sdf_ref.py (formulation A) on the host.

Workload: the marching-cubes mesh of an analytic field (torus + sphere) at 129^3 and 257^3, one million uniform points in
its bounding box.  Per mesh: grid build + fill, the distance query, the winding-number pass (3 warm-ups, median of 10),
the point-triangle tests per point (the query's counter), and the cost of one test measured by a resolution-1 query —
every face against every point, no search — which splits the query time into arithmetic and search.

    python tools/time_mesh_sdf.py [--sizes 129 257] [--points 1000000] [--reps 10] [--out profiles/mesh_sdf_timing.md]

Prints a markdown report (and writes it to --out).
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def device_ms(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
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


def mc_mesh(n):
    from slice3d_amd.mesh import marching_cubes_device
    g = torch.linspace(-1, 1, n, dtype=torch.float64, device="cuda")
    x, y, z = torch.meshgrid(g, g, g, indexing="ij")
    q = torch.sqrt(x ** 2 + y ** 2) - 0.5
    field = torch.maximum(0.22 - torch.sqrt(q ** 2 + z ** 2), 0.35 - torch.sqrt((x - 0.3) ** 2 + y ** 2 + (z - 0.35) ** 2))
    return marching_cubes_device(field, 0.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[129, 257])
    ap.add_argument("--points", type=int, default=1000000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--host_points", type=int, default=2000)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    import sdf_ref
    from slice3d_amd.mesh_sdf import MeshDistance, winding_number

    lines = ["# Signed-distance kernels: timing (`python tools/time_mesh_sdf.py`)", "",
             "%s, %d uniform points in the mesh's bounding box (float64), device events on the stream, 3 warm-ups, median of %d."
             % (torch.cuda.get_device_name(0), args.points, args.reps),
             "Host column: float64 numpy brute force over all faces (`tests/sdf_ref.py`, formulation A) on %d of the points, "
             "one process on a host that shows %d cores (numpy's element-wise loops use one)." % (args.host_points, os.cpu_count()),
             "", "| grid | faces | resolution | build + fill | distance query | tests / point | arithmetic share | winding pass | "
             "host brute force (%d points) |" % args.host_points, "|---|---|---|---|---|---|---|---|---|"]

    def emit():
        text = "\n".join(lines) + "\n"
        if args.out:
            with open(args.out, "w") as fh:
                fh.write(text)
        return text

    for n in args.sizes:
        v, f = mc_mesh(n)
        nf = f.shape[0]
        vn, fn = v.cpu().numpy(), f.cpu().numpy()
        lo, hi = vn[fn.reshape(-1)].min(0), vn[fn.reshape(-1)].max(0)
        pts = torch.from_numpy(np.random.default_rng(n).uniform(lo, hi, (args.points, 3))).cuda()
        t_build = device_ms(lambda: MeshDistance((v, f)), args.reps)
        md = MeshDistance((v, f))
        t_query = device_ms(lambda: md.query(pts), args.reps)
        tests = int(md.n_tests)
        # one test's cost: every face against every point of a subset, no search
        sub = pts[: max(256, min(args.points, int(2e9 // nf)))]
        brute = MeshDistance((v, f), resolution=1)
        t_brute = device_ms(lambda: brute.query(sub), max(3, args.reps // 3), warmup=1)
        assert int(brute.n_tests) == sub.shape[0] * nf
        ns_per_test = t_brute * 1e6 / (sub.shape[0] * nf)
        share = tests * ns_per_test * 1e-6 / t_query
        t_wind = device_ms(lambda: winding_number((v, f), pts), args.reps)
        hp = pts[: args.host_points].cpu().numpy()
        t0 = time.perf_counter()
        da = sdf_ref.dist_a(vn, fn, hp)[0]
        t_host = (time.perf_counter() - t0) * 1e3
        err = float(np.abs(md.query(hp) - da).max())
        lines.append("| %d^3 | %d | %d | %.2f ms | %.2f ms | %.1f | %.0f %% (%.3f ns / test) | %.1f ms (%.2e pairs/s) | %.0f ms "
                     "(max abs difference %.1e) |" % (n, nf, md.resolution, t_build, t_query, tests / args.points, 100 * share,
                                                     ns_per_test, t_wind, args.points * nf / (t_wind * 1e-3), t_host, err))
        print(lines[-1], flush=True)
        emit()
    lines += ["", "Arithmetic share = tests x (time of one point-triangle test, from a resolution-1 query that tests every face "
              "against every point) / query time; the rest is the search: skip-table and offset reads, cell bounds, and the "
              "lanes of a wave that wait for its slowest point."]
    print(emit())


if __name__ == "__main__":
    main()

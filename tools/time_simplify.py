"""Times the device mesh simplifier (slice3d_amd/mesh_simplify.py) on the test fixtures and on marching-cubes meshes of
an analytic genus-1 field at 128^3 and 256^3, and measures its error against the input where the mesh is small enough for
MeshDistance to take a few seconds.  One JSON line per case; profiles/mesh_simplify_timing.md is the record.

    python tools/time_simplify.py [--repeats 5] [--big 128,256]

The time of a case is the median of `repeats` runs after one warm-up, each between two device synchronisations, host
call included (workspace allocation, the rounds with their read-backs, emit).  The input is on the device already.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import simplify_cases as sc  # noqa: E402
import simplify_ref as sr  # noqa: E402
from slice3d_amd.mesh import marching_cubes_device  # noqa: E402
from slice3d_amd.mesh_sdf import MeshDistance  # noqa: E402
from slice3d_amd.mesh_simplify import simplify_stats  # noqa: E402


def timed(v, f, t, agg, repeats):
    out = simplify_stats(v, f, t, agg)
    ms = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = simplify_stats(v, f, t, agg)
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return out, statistics.median(ms)


def error(v, f, vo, fo):
    dist = lambda a, b, p: MeshDistance((a, b)).query(p)   # noqa: E731
    return sr.mesh_error((v, f), (vo, fo), sr.bbox_diagonal(v, f), dist)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--big", type=str, default="128,256", help="grid sizes of the analytic genus-1 field")
    args = ap.parse_args()
    print(json.dumps({"device": torch.cuda.get_device_name(0)}), flush=True)
    for name in sc.CLOSED + ["genus1"]:
        v, f = sc.mesh(name)
        vd, fd = torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda()
        for r in sc.RATIOS:
            t = len(f) * r // 100
            (vo, fo, rounds), ms = timed(vd, fd, t, sc.AGGRESSIVENESS, args.repeats)
            print(json.dumps({"mesh": name, "faces_in": len(f), "target": t, "faces_out": len(fo), "rounds": rounds,
                              "ms": round(ms, 3), "E": error(v, f, vo.cpu().numpy(), fo.cpu().numpy())}), flush=True)
    for n in [int(x) for x in args.big.split(",") if x]:
        vol = torch.from_numpy(sc.genus1_field(n)).cuda()
        v, f = marching_cubes_device(vol, 0.0, pad_value=-1e6)
        v = (v - 1.0) * (2.0 / (n - 1)) - 1.0
        for t in (len(f) // 10, 10000):
            (vo, fo, rounds), ms = timed(v, f, t, sc.AGGRESSIVENESS, args.repeats)
            fo_h = fo.cpu().numpy()
            rec = {"mesh": "genus1_%d" % n, "faces_in": len(f), "target": t, "faces_out": len(fo), "rounds": rounds,
                   "ms": round(ms, 3), "closed_oriented_manifold": sr.is_oriented_manifold(fo_h),
                   "euler": sr.euler_characteristic(fo_h)}
            if len(f) <= 400000:
                rec["E"] = error(v.cpu().numpy(), f.cpu().numpy(), vo.cpu().numpy(), fo_h)
            print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()

"""Times the device mesh-topology unit (slice3d_amd/mesh_topology.py) on marching-cubes meshes of the analytic genus-1 field
at 64^3, 128^3 and 256^3 and writes profiles/mesh_topology_timing.md.

    python tools/time_topology.py [--repeats 5] [--grids 64,128,256] [--out profiles/mesh_topology_timing.md]

A time is the median of `repeats` runs after one warm-up, each between two device synchronisations, host call included
(workspace allocation, the rounds with their read-backs, emit).  The input is on the device already.  Reported apart:
topology of the mesh as it is (labels and table); keep of the largest component; and the weld, as the difference of two
runs on the mesh's triangle soup (every face its own three vertices): with weld=True, and with weld=False on the same 3 F
vertices and the faces already mapped to their representatives (vmap[faces]).  The two runs see the same welded faces, so
they differ by the weld stage alone: the finiteness check, the hash table's fill, insert and read.  The rounds of the tests'
20 000-triangle strips are recorded too.  For information the numpy reference (tests/topology_ref.py) is timed once on the host of the same machine.
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
import topology_ref as tr  # noqa: E402
from slice3d_amd.mesh import marching_cubes_device  # noqa: E402
from slice3d_amd.mesh_topology import mesh_topology  # noqa: E402


def timed(fn, repeats):
    out = fn()
    ms = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return out, statistics.median(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--grids", type=str, default="64,128,256", help="grid sizes of the analytic genus-1 field")
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "mesh_topology_timing.md"))
    args = ap.parse_args()
    device = torch.cuda.get_device_name(0)
    print(json.dumps({"device": device}), flush=True)
    rows = []
    for n in [int(x) for x in args.grids.split(",") if x]:
        v, f = marching_cubes_device(torch.from_numpy(sc.genus1_field(n)).cuda(), 0.0, pad_value=-1e6)
        v = (v - 1.0) * (2.0 / (n - 1)) - 1.0
        topo, ms_topo = timed(lambda: mesh_topology((v, f)), args.repeats)
        mask = np.arange(topo.n_components) == int(np.argmax(topo.table["faces"]))
        _, ms_keep = timed(lambda: topo._run.keep(mask), args.repeats)
        vs, fs = tr.soup(v.cpu().numpy(), f.cpu().numpy(), seed=n)
        vs, fs = torch.from_numpy(vs).cuda(), torch.from_numpy(fs).cuda()
        welded, ms_weld = timed(lambda: mesh_topology((vs, fs), weld=True), args.repeats)
        fw = welded.vmap[fs]                               # the same welded faces, no weld to do
        mapped, ms_soup = timed(lambda: mesh_topology((vs, fw)), args.repeats)
        t0 = time.perf_counter()
        ref = tr.topology(v.cpu().numpy(), f.cpu().numpy())
        ms_ref = (time.perf_counter() - t0) * 1e3
        rec = {"grid": n, "faces": int(f.shape[0]), "vertices": int(v.shape[0]), "components": topo.n_components,
               "rounds": topo.rounds, "topology_ms": round(ms_topo, 3), "keep_ms": round(ms_keep, 3),
               "soup_vertices": int(vs.shape[0]), "weld_topology_ms": round(ms_weld, 3), "weld_rounds": welded.rounds,
               "mapped_topology_ms": round(ms_soup, 3), "mapped_rounds": mapped.rounds, "weld_ms": round(ms_weld - ms_soup, 3),
               "mapped_equals_welded": bool(torch.equal(mapped.face_component, welded.face_component)),
               "welded_vertices": int(welded.summary["vertices"]), "watertight": topo.is_watertight,
               "euler": int(topo.summary["euler"]), "numpy_reference_ms": round(ms_ref, 1),
               "labels_equal_reference": bool(np.array_equal(topo.face_component.cpu().numpy(), ref["face_component"]))}
        print(json.dumps(rec), flush=True)
        rows.append(rec)
    strips = []
    for cuts in (0, 7):
        sv, sf = tr.strip(20000, 11, cuts)
        t = mesh_topology((torch.from_numpy(sv).cuda(), torch.from_numpy(sf).cuda()))
        strips.append({"strip_faces": len(sf), "cuts": cuts, "components": t.n_components, "rounds": t.rounds})
        print(json.dumps(strips[-1]), flush=True)
    with open(args.out, "w") as fh:
        fh.write("# Mesh topology: timing (`python tools/time_topology.py`)\n\n")
        fh.write("One MI355X (the runtime's device name: \"%s\"), marching-cubes meshes of the analytic genus-1 field, input on the "
                 "device, median of %d after one warm-up, host call included (workspace allocation, one read-back per round, "
                 "emit of labels and table).\n" % (device, args.repeats))
        fh.write("The soup columns run on the mesh's triangle soup (3 F vertices): once with weld, once without weld on the faces "
                 "already mapped to their representatives, which is the same work but for the weld stage (finiteness check, hash "
                 "table fill, insert, read); weld = their difference.  The numpy reference (`tests/topology_ref.py`: "
                 "union-find in Python, `np.unique` edge counts) is timed once on the same machine's host, for information.\n\n")
        fh.write("| grid | faces | vertices | components | rounds | topology | keep (largest) | soup: weld + topology (rounds) | "
                 "soup: topology of the mapped faces (rounds) | weld = difference | numpy reference |\n|---|---|---|---|---|---|---|---|---|---|---|\n")
        for r in rows:
            fh.write("| %d^3 | %d | %d | %d | %d | %.2f ms | %.2f ms | %.2f ms (%d) | %.2f ms (%d) | %.2f ms | %.0f ms |\n"
                     % (r["grid"], r["faces"], r["vertices"], r["components"], r["rounds"], r["topology_ms"], r["keep_ms"],
                        r["weld_topology_ms"], r["weld_rounds"], r["mapped_topology_ms"], r["mapped_rounds"], r["weld_ms"],
                        r["numpy_reference_ms"]))
        fh.write("\nRounds of the tests' strips (20 000 triangles, vertex numbering and face order permuted at random; the count may "
                 "differ by a round or two between runs, the labels cannot): %s.\n"
                 % "; ".join("%d faces cut %d times, %d components: %d rounds" % (t["strip_faces"], t["cuts"], t["components"], t["rounds"])
                             for t in strips))
        ok = all(r["components"] == 1 and r["watertight"] and r["euler"] == 0 and r["labels_equal_reference"]
                 and r["welded_vertices"] == r["vertices"] for r in rows)
        fh.write("\n%s  Nothing was profiled: no kernel-level breakdown is claimed.\n"
                 % ("Every mesh came out as one closed oriented component of Euler characteristic 0 with the reference's labels, "
                    "and the welded soup has the mesh's vertex count." if ok else
                    "NOT every mesh came out as one watertight genus-1 component with the reference's labels: see the JSON lines."))


if __name__ == "__main__":
    main()

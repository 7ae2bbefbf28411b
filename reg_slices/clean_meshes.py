"""clean_meshes.py — reports what every `.obj` of a directory is made of and removes small components, on the GPU
(slice3d_amd/mesh_topology.py: weld of equal positions, connected components, per-component topology and measures).

    python reg_slices/clean_meshes.py --dir_meshes <dir of *.obj> --dir_out <dir> [--weld] [--keep_largest K] \
        [--min_component_frac f] [--component_measure faces|area|volume] [--drop_degenerate] [--report_only]

Per mesh `<dir_out>/<shape>.obj` is written (not with --report_only): the kept components' faces and vertices in their
original order, with --weld over the welded vertices.  `<dir_out>/topology.csv` gets one row per component of every mesh.
One line per mesh is printed, and at the end one JSON line: the meshes with components in / kept, faces in / out, watertight
and seconds each.  Exit status 1 when the directory holds no mesh.
"""
import argparse
import glob
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CSV_COLUMNS = ["mesh", "component", "kept", "faces", "vertices", "edges", "edges_1", "edges_2", "edges_3plus", "conflicts",
               "degenerate", "euler", "closed_oriented", "oriented_with_border", "area", "volume", "bbox_lo_x", "bbox_lo_y",
               "bbox_lo_z", "bbox_hi_x", "bbox_hi_y", "bbox_hi_z"]


def build_parser():
    parser = argparse.ArgumentParser()
    parser.add_argument("--dir_meshes", type=str, required=True, help="directory of <shape>.obj")
    parser.add_argument("--dir_out", type=str, required=True, help="directory topology.csv and the cleaned <shape>.obj go to")
    parser.add_argument("--weld", action="store_true", help="weld vertices at equal positions first (triangle soups)")
    parser.add_argument("--keep_largest", type=int, default=None, help="keep this many of the largest components")
    parser.add_argument("--min_component_frac", type=float, default=0.0,
                        help="drop the components below this share of the largest one in --component_measure")
    parser.add_argument("--component_measure", type=str, default="faces", choices=["faces", "area", "volume"])
    parser.add_argument("--drop_degenerate", action="store_true", help="drop the faces that name a (welded) vertex twice")
    parser.add_argument("--report_only", action="store_true", help="write topology.csv, no mesh")
    return parser


def main(argv=None):
    args = build_parser().parse_args(argv)
    if args.keep_largest is not None and args.keep_largest < 0:
        raise SystemExit("--keep_largest %d < 0" % args.keep_largest)
    import torch
    from slice3d_amd.mesh_eval import load_obj
    from slice3d_amd.mesh_topology import COUNT_COLUMNS, keep_components, mesh_topology, select_components

    paths = sorted(glob.glob(os.path.join(args.dir_meshes, "*.obj")))
    os.makedirs(args.dir_out, exist_ok=True)
    rows = []
    with open(os.path.join(args.dir_out, "topology.csv"), "w") as csv:
        csv.write(",".join(CSV_COLUMNS) + "\n")
        for path in paths:
            name = os.path.basename(path)
            mesh = load_obj(path)
            torch.cuda.synchronize()
            t0 = time.time()
            topo = mesh_topology(mesh, weld=args.weld)
            mask = select_components(topo.table, largest=args.keep_largest, by=args.component_measure,
                                     min_frac=args.min_component_frac)
            out = mesh
            if not args.report_only:
                out = keep_components(mesh, mask, drop_degenerate=args.drop_degenerate, weld=args.weld, topology=topo)
            seconds = time.time() - t0
            t = topo.table
            for k in range(topo.n_components):
                cells = [name, str(k), str(int(mask[k]))] + [str(int(t[c][k])) for c in COUNT_COLUMNS]
                cells += [repr(float(t["area"][k])), repr(float(t["volume"][k]))] + [repr(float(x)) for x in t["bbox"][k]]
                csv.write(",".join(cells) + "\n")
            if not args.report_only:
                out.export(os.path.join(args.dir_out, name))
            rows.append({"mesh": name, "components_in": topo.n_components, "components_kept": int(mask.sum()),
                         "faces_in": len(mesh.faces), "faces_out": len(out.faces), "vertices_out": len(out.vertices),
                         "watertight": topo.is_watertight, "rounds": topo.rounds, "seconds": seconds})
            print("%s: %d components, %d kept, %d -> %d faces, watertight %s, %.4f s"
                  % (name, topo.n_components, int(mask.sum()), len(mesh.faces), len(out.faces), topo.is_watertight, seconds))
    print(json.dumps({"n_meshes": len(rows), "weld": bool(args.weld), "report_only": bool(args.report_only), "meshes": rows}))
    return 0 if rows else 1


if __name__ == "__main__":
    sys.exit(main())

"""simplify_meshes.py — simplifies every `.obj` of a directory on the GPU (slice3d_amd/mesh_simplify.py: quadric edge
collapse with the reference's libsimplify parameters) and writes the results under the same names.

    python reg_slices/simplify_meshes.py --dir_meshes <dir of *.obj> --dir_out <dir> (--n_faces 10000 | --ratio 0.1) \
        [--agressiveness 5]

One line per mesh is printed, and at the end one JSON line: the meshes with faces in / out, rounds and seconds each.
Exit status 1 when the directory holds no mesh.
"""
import argparse
import glob
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def build_parser():
    parser = argparse.ArgumentParser()
    parser.add_argument("--dir_meshes", type=str, required=True, help="directory of <shape>.obj")
    parser.add_argument("--dir_out", type=str, required=True, help="directory the simplified <shape>.obj go to")
    target = parser.add_mutually_exclusive_group(required=True)
    target.add_argument("--n_faces", type=int, help="target number of faces")
    target.add_argument("--ratio", type=float, help="target as a share of each mesh's faces, in (0, 1]")
    parser.add_argument("--agressiveness", type=float, default=5.0,
                        help="exponent of the threshold schedule (the reference's spelling; reconstruct.py passes 5)")
    return parser


def main(argv=None):
    args = build_parser().parse_args(argv)
    if args.ratio is not None and not 0.0 < args.ratio <= 1.0:
        raise SystemExit("--ratio %g outside (0, 1]" % args.ratio)
    if args.n_faces is not None and args.n_faces < 0:
        raise SystemExit("--n_faces %d < 0" % args.n_faces)
    import torch
    from slice3d_amd.mesh import Mesh
    from slice3d_amd.mesh_eval import load_obj
    from slice3d_amd.mesh_simplify import simplify_stats

    paths = sorted(glob.glob(os.path.join(args.dir_meshes, "*.obj")))
    os.makedirs(args.dir_out, exist_ok=True)
    rows = []
    for path in paths:
        mesh = load_obj(path)
        n_in = len(mesh.faces)
        target = args.n_faces if args.n_faces is not None else int(n_in * args.ratio)
        rounds, seconds = 0, 0.0
        if n_in:
            torch.cuda.synchronize()
            t0 = time.time()
            v, f, rounds = simplify_stats(mesh.vertices, mesh.faces, target, args.agressiveness)
            seconds = time.time() - t0
            mesh = Mesh(v, f)
        mesh.export(os.path.join(args.dir_out, os.path.basename(path)))
        rows.append({"mesh": os.path.basename(path), "faces_in": n_in, "faces_out": len(mesh.faces), "rounds": rounds,
                     "seconds": seconds})
        print("%s: %d -> %d faces, %d rounds, %.4f s" % (rows[-1]["mesh"], n_in, len(mesh.faces), rounds, seconds))
    print(json.dumps({"n_meshes": len(rows), "meshes": rows}))
    return 0 if rows else 1


if __name__ == "__main__":
    sys.exit(main())

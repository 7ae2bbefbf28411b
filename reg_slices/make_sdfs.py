"""make_sdfs.py — writes the signed-distance training targets `<dir_data>/<name_dataset>/02_sdfs/<shape>.npy` from a
directory of triangle meshes, on the GPU (slice3d_amd/mesh_sdf.py: exact point-to-mesh distance, sign by ray parity or
by generalised winding number).  The reference ships no program for these files; their format is the one its dataset
class reads (reg_slices/src/datasets.py:142-148): float32 (N, 4) rows (x, y, z, signed distance + 0.003).

    python reg_slices/make_sdfs.py --dir_meshes <dir of <shape>.obj> --name_dataset custom --dir_data ../data \
        [--n_points 500000] [--sign parity|winding|auto] [--normalize] [--seed 0] [--dir_out_meshes DIR] [--overwrite]

--normalize centres each mesh's bounding box on 0 and scales its body diagonal to 1 first.  With --dir_out_meshes the
mesh is written as <shape>.obj in the frame of the samples — what eval_meshes.py --dir_gt_meshes expects — and the
samples are computed from that file as a reader sees it, so file and mesh agree to the last digit.  Existing .npy files
are skipped unless --overwrite.  --sign auto chooses per shape: parity when the mesh, after welding equal positions, is
watertight (slice3d_amd/mesh_topology.py: every component closed and oriented), else winding; the distance and sign code
still gets the mesh as loaded, and the summary's `signs` records the choice of each shape written in this run (a shape
skipped because its .npy exists, or one without faces, gets no entry).  One line per shape (shape, points, share of points
inside, seconds) and one JSON summary line are printed.  Exit status 1 when no mesh is found.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def build_parser():
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    p.add_argument("--dir_meshes", type=str, required=True, help="directory of <shape>.obj")
    p.add_argument("--name_dataset", type=str, required=True)
    p.add_argument("--dir_data", type=str, default="../data")
    p.add_argument("--n_points", type=int, default=500000, help="samples per shape")
    p.add_argument("--sign", type=str, default="parity", choices=["parity", "winding", "auto"],
                   help="what 'inside' means: the ray parity eval_meshes.py scores with (watertight meshes), generalised "
                        "winding number > 0.5 (open meshes), or auto: parity for the shapes that are watertight after "
                        "welding, winding for the others")
    p.add_argument("--normalize", action="store_true", help="bounding box centred on 0, body diagonal 1")
    p.add_argument("--seed", type=int, default=0, help="shape i is sampled with seed + i")
    p.add_argument("--dir_out_meshes", type=str, default=None, help="write the meshes in the frame of the samples here")
    p.add_argument("--overwrite", action="store_true")
    return p


def main(argv=None):
    args = build_parser().parse_args(argv)
    names = sorted(f[:-4] for f in os.listdir(args.dir_meshes) if f.endswith(".obj")) if os.path.isdir(args.dir_meshes) else []
    if not names:
        print(json.dumps({"n_shapes": 0, "dir_meshes": args.dir_meshes}))
        return 1
    import torch
    from slice3d_amd.mesh import Mesh
    from slice3d_amd.mesh_eval import load_obj
    from slice3d_amd.mesh_sdf import make_sdf_file, normalize_mesh

    dir_sdf = os.path.join(args.dir_data, args.name_dataset, "02_sdfs")
    os.makedirs(dir_sdf, exist_ok=True)
    if args.dir_out_meshes:
        os.makedirs(args.dir_out_meshes, exist_ok=True)
    written, skipped, empty, shares, signs = 0, 0, [], [], {}
    for i, shape in enumerate(names):
        path = os.path.join(dir_sdf, shape + ".npy")
        if os.path.isfile(path) and not args.overwrite:
            skipped += 1
            continue
        t0 = time.time()
        mesh = load_obj(os.path.join(args.dir_meshes, shape + ".obj"))
        if len(mesh.faces) == 0:
            empty.append(shape)
            continue
        if args.normalize:
            mesh = Mesh(normalize_mesh(mesh.vertices), mesh.faces)
        if args.dir_out_meshes:
            mesh = load_obj(mesh.export(os.path.join(args.dir_out_meshes, shape + ".obj")))
        dev = (torch.from_numpy(mesh.vertices).cuda(), torch.from_numpy(mesh.faces).cuda())    # on the device once
        sign = args.sign
        if sign == "auto":
            from slice3d_amd.mesh_topology import mesh_topology
            sign = "parity" if mesh_topology(dev, weld=True).is_watertight else "winding"
        signs[shape] = sign
        out = make_sdf_file(dev, path, args.n_points, args.seed + i, sign=sign)
        share = float((out[:, 3] - np.float32(0.003) <= 0).mean())
        shares.append(share)
        written += 1
        print("%s %d %.4f %.2f" % (shape, len(out), share, time.time() - t0) + (" " + sign if args.sign == "auto" else ""))
    summary = {"signs": signs} if args.sign == "auto" else {}
    print(json.dumps({"n_shapes": len(names), "written": written, "skipped": skipped, "no_faces": len(empty),
                      "sign": args.sign, "n_points": args.n_points, **summary,
                      "inside_share": float(np.mean(shares)) if shares else None, "dir_sdf": dir_sdf}))
    return 0


if __name__ == "__main__":
    sys.exit(main())

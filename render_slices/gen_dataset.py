"""gen_dataset.py — renders the image half of a dataset from a directory of triangle meshes, on the GPU
(slice3d_amd/mesh_render.py): `<dir_data>/<name_dataset>/00_img_input/<shape>/<view:03d>.png` + `meta.pkl` and
`01_img_slices/<shape>/<view:03d>/{X,Y,Z}_{1..4}.png`, the files the reference makes with Blender
(render_slices/blender_script_input.py, blender_script_slices.py).  With reg_slices/make_sdfs.py, which writes
`02_sdfs/<shape>.npy`, a directory of .obj files becomes a complete training set without an external tool.

    python render_slices/gen_dataset.py --dir_meshes <dir of <shape>.obj> --name_dataset custom --dir_data ../data \
        [--n_views 16] [--img_size 256] [--samples 4] [--slice_direction camera|axis] [--seed 0] [--normalize]
        [--write_splits] [--overwrite]

The conventions are make_sdfs.py's: --normalize centres each mesh's bounding box on 0 and scales its body diagonal to 1
(run both programs with it, or neither, so that images and samples share a frame); shape i draws its cameras with
seed + i; one line per shape (shape, views, mean alpha of the views, seconds) and one JSON summary line are printed;
exit status 1 when no mesh is found.  A shape whose last view and last slice exist is skipped unless --overwrite.  An
existing meta.pkl is reused and never overwritten, so slices can be re-rendered for cameras that already exist.
--write_splits writes 03_splits/{train,val,test}.lst with every shape.

The images are not Blender's: the shading is a two-sided Lambert term on 0.8 grey (see slice3d_amd/mesh_render.py), and
how checkpoints trained on the reference's renders respond to them has not been measured.
"""
import argparse
import json
import os
import pickle
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def build_parser():
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    p.add_argument("--dir_meshes", type=str, required=True, help="directory of <shape>.obj")
    p.add_argument("--name_dataset", type=str, required=True)
    p.add_argument("--dir_data", type=str, default="../data")
    p.add_argument("--n_views", type=int, default=16)
    p.add_argument("--img_size", type=int, default=256)
    p.add_argument("--samples", type=int, default=4, choices=[1, 2, 4], help="samples per pixel edge")
    p.add_argument("--slice_direction", type=str, default="camera", choices=["camera", "axis"])
    p.add_argument("--seed", type=int, default=0, help="shape i draws its cameras with seed + i")
    p.add_argument("--normalize", action="store_true", help="bounding box centred on 0, body diagonal 1")
    p.add_argument("--write_splits", action="store_true", help="03_splits/{train,val,test}.lst with every shape")
    p.add_argument("--overwrite", action="store_true")
    return p


def main(argv=None):
    args = build_parser().parse_args(argv)
    names = sorted(f[:-4] for f in os.listdir(args.dir_meshes) if f.endswith(".obj")) if os.path.isdir(args.dir_meshes) else []
    if not names:
        print(json.dumps({"n_shapes": 0, "dir_meshes": args.dir_meshes}))
        return 1
    import torch
    from slice3d_amd.mesh_eval import load_obj
    from slice3d_amd.mesh_render import SliceRenderer, make_meta, write_shape
    from slice3d_amd.mesh_sdf import normalize_mesh

    base = os.path.join(args.dir_data, args.name_dataset)
    written, skipped, reused, empty = 0, 0, 0, []
    for i, shape in enumerate(names):
        dir_ipt = os.path.join(base, "00_img_input", shape)
        path_meta = os.path.join(dir_ipt, "meta.pkl")
        if os.path.isfile(path_meta):
            with open(path_meta, "rb") as fh:
                meta = pickle.load(fh)
            have_meta = True
        else:
            meta = make_meta(args.n_views, args.seed + i, size=args.img_size)
            have_meta = False
        n = len(meta[1])
        last = (os.path.join(dir_ipt, "%03d.png" % (n - 1)), os.path.join(base, "01_img_slices", shape, "%03d" % (n - 1), "Z_4.png"))
        if n and all(os.path.isfile(x) for x in last) and not args.overwrite:
            skipped += 1
            continue
        t0 = time.time()
        mesh = load_obj(os.path.join(args.dir_meshes, shape + ".obj"))
        if len(mesh.faces) == 0:
            empty.append(shape)
            continue
        v = normalize_mesh(mesh.vertices) if args.normalize else np.asarray(mesh.vertices, dtype=np.float64)
        renderer = SliceRenderer((torch.from_numpy(v).cuda(), torch.from_numpy(np.asarray(mesh.faces)).cuda()))   # on the device once
        write_shape(renderer, base, shape, meta, size=args.img_size, samples=args.samples, slice_direction=args.slice_direction)
        reused += int(have_meta)
        written += 1
        from PIL import Image
        alpha = np.mean([np.asarray(Image.open(os.path.join(dir_ipt, "%03d.png" % k)))[:, :, 3].mean() for k in range(n)]) / 255.0
        print("%s %d %.4f %.2f" % (shape, n, alpha, time.time() - t0))
    if args.write_splits:
        os.makedirs(os.path.join(base, "03_splits"), exist_ok=True)
        for split in ("train", "val", "test"):
            with open(os.path.join(base, "03_splits", split + ".lst"), "w") as fh:
                fh.write("\n".join(n for n in names if n not in empty) + "\n")
    print(json.dumps({"n_shapes": len(names), "written": written, "skipped": skipped, "no_faces": len(empty),
                      "meta_reused": reused, "n_views": args.n_views, "img_size": args.img_size, "samples": args.samples,
                      "slice_direction": args.slice_direction, "dir_dataset": base}))
    return 0


if __name__ == "__main__":
    sys.exit(main())

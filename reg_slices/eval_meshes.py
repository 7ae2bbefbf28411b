"""eval_meshes.py — scores the meshes reconstruct.py wrote (either route) against the test split, on the GPU:
IoU on the dataset's query points, and, where a ground-truth mesh is given, Chamfer-L1 / L2, F-score, precision,
recall and Hausdorff distance on area-weighted surface samples (slice3d_amd/mesh_eval.py, the reference's
reg_slices/src/utils_eval.py scores; F-score as the harmonic mean, see eval_chamfer).

    python reg_slices/eval_meshes.py --name_exp demo --name_dataset custom --dir_data ../data --n_qry 100000 \
        [--dir_gt_meshes <dir of <shape>.obj in the frame of the 02_sdfs samples>]

One row per shape goes to <dir_results>/eval.csv; one JSON line of means is printed.  Exit status 1 when no mesh is
found.
"""
import csv
import json
import os
import pickle
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from options import get_parser  # noqa: E402

COLUMNS = ["shape", "iou", "chamfer_L1", "chamfer_L2", "fscore", "precision", "recall", "hausdorff"]


def build_parser():
    parser = get_parser()
    parser.add_argument("--dir_results", type=str, default=None,
                        help="[build] directory of <shape>.obj (default experiments/<name_exp>/results/<name_dataset>)")
    parser.add_argument("--dir_gt_meshes", type=str, default=None,
                        help="[build] directory of ground-truth <shape>.obj in the frame of the 02_sdfs samples")
    parser.add_argument("--n_surface_points", type=int, default=100000, help="[build] surface samples per mesh")
    parser.add_argument("--f_thresh", type=float, default=0.01, help="[build] F-score distance threshold")
    parser.add_argument("--eval_seed", type=int, default=0, help="[build] seed of the surface sampling")
    return parser


def sdf_frame_to_query_frame(vertices, dir_img_ipt, shape):
    """The map slice3d_amd/datasets.py:141-143 applies to the 02_sdfs samples: p * scale + (ox, oz, -oy)."""
    with open(os.path.join(dir_img_ipt, shape, "meta.pkl"), "rb") as f:
        meta = pickle.load(f)
    scale, offset = meta[5], meta[6]
    return np.asarray(vertices, dtype=np.float64) * scale + np.array([offset[0], offset[2], -offset[1]])


def main(argv=None):
    args = build_parser().parse_args(argv)
    import torch
    from slice3d_amd.datasets import Slice3DDataset
    from slice3d_amd.mesh_eval import eval_chamfer, eval_hausdoff, eval_iou, load_obj, sample_surface

    dir_results = args.dir_results or os.path.join("experiments", args.name_exp, "results", args.name_dataset)
    dataset = Slice3DDataset(split="test", args=args, with_slices=False)
    rows, missing, undefined = [], [], []
    for idx in range(len(dataset)):
        shape = dataset.files[idx][1]
        path = os.path.join(dir_results, shape + ".obj")
        if not os.path.isfile(path):
            missing.append(shape)
            continue
        mesh = load_obj(path)
        item = dataset[idx]
        dev = (torch.from_numpy(mesh.vertices).cuda(), torch.from_numpy(mesh.faces).cuda())   # on the device once
        iou = float(np.asarray(eval_iou(dev, item["qry_norot"].cuda(), item["occ"].numpy())).reshape(()))
        if np.isnan(iou):
            undefined.append(shape)
        row = {"shape": shape, "iou": iou}
        gt_path = os.path.join(args.dir_gt_meshes, shape + ".obj") if args.dir_gt_meshes else None
        if gt_path and os.path.isfile(gt_path) and len(mesh.faces):
            gt = load_obj(gt_path)
            gt_v = torch.from_numpy(sdf_frame_to_query_frame(gt.vertices, dataset.dir_img_ipt, shape)).cuda()
            p_rec, _ = sample_surface(dev, args.n_surface_points, seed=args.eval_seed)
            p_gt, _ = sample_surface((gt_v, torch.from_numpy(gt.faces).cuda()), args.n_surface_points,
                                     seed=args.eval_seed + 1)
            cl1, cl2, fs, pr, rc = eval_chamfer(p_rec, p_gt, f_thresh=args.f_thresh)
            row.update(chamfer_L1=cl1, chamfer_L2=cl2, fscore=fs, precision=pr, recall=rc,
                       hausdorff=eval_hausdoff(p_rec, p_gt)[2])
        rows.append(row)
        print(shape, " ".join("%s=%.6g" % (k, row[k]) for k in COLUMNS[1:] if k in row))
    if not rows:
        print(json.dumps({"n_shapes": 0, "missing": len(missing), "dir_results": dir_results}))
        return 1
    os.makedirs(dir_results, exist_ok=True)
    with open(os.path.join(dir_results, "eval.csv"), "w", newline="") as f:
        w = csv.DictWriter(f, fieldnames=COLUMNS)
        w.writeheader()
        for r in rows:
            w.writerow({k: r.get(k, "") for k in COLUMNS})
    summary = {"n_shapes": len(rows), "missing": len(missing), "undefined_iou": len(undefined)}
    for k in COLUMNS[1:]:
        vals = [r[k] for r in rows if k in r and not np.isnan(r[k])]
        summary[k] = float(np.mean(vals)) if vals else None
    print(json.dumps(summary))
    return 0


if __name__ == "__main__":
    sys.exit(main())

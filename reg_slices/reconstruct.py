"""reconstruct.py — host entry point kept from the reference (reg_slices/reconstruct.py:334-416):
load a checkpoint into Slices3DRegModel(mode='test'), run Generator3D (MISE or dense grid -> eval_points
-> marching cubes) per test object and export `<shape>.obj`, with the reference's flags.

    python reg_slices/reconstruct.py --name_exp demo --name_ckpt x.ckpt --name_dataset synthetic \
        --mode test --img_size 128 --mc_res0 64 --mc_up_steps 2 [--keep_largest 1] [--min_component_frac 0.01] \
        [--component_measure faces|area|volume] [--simplify_nfaces 10000]

With --name_model gtslice --from_which_slices gen --gen_ckpt <LatentDiffusion .ckpt> the slices are generated in memory
(slice3d_amd/gen_route.py): per batch of --n_bs test objects, input view 004 -> SliceDiffusion.generate -> the 8-bit mosaic
quantisation of test_step -> the GT model, the same bits the file route (gen_slices/sample_slices.py + re_org_slices.py)
gives it, without writing or reading slice images.
"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from options import get_parser  # noqa: E402
from slice3d_amd.generator import Generator3D  # noqa: E402
from slice3d_amd.models import Slices3DRegModel  # noqa: E402
from slice3d_amd.synth import SyntheticSlice3DDataset  # noqa: E402


def export_mesh(args, mesh, stats, path_mesh):
    """--simplify_nfaces N: simplify_mesh(mesh, N, 5.) as the reference's Generator3D.extract_mesh does (reconstruct.py:231-235
    there), on the GPU; then `<shape>.obj`.  --keep_largest K / --min_component_frac f (ranked by --component_measure) first
    drop the small detached components marching cubes emits (slice3d_amd/mesh_topology.py), so that they neither reach the
    file nor eat the simplifier's face budget."""
    if (args.keep_largest is not None or args.min_component_frac > 0.0) and len(mesh.faces):
        from slice3d_amd.mesh_topology import keep_components, mesh_topology, select_components
        torch.cuda.synchronize()
        t0 = time.time()
        topo = mesh_topology(mesh)
        mask = select_components(topo.table, largest=args.keep_largest, by=args.component_measure,
                                 min_frac=args.min_component_frac)
        mesh = keep_components(mesh, mask, topology=topo)
        stats["components (in / kept)"] = "%d / %d" % (topo.n_components, int(mask.sum()))
        stats["time (clean)"] = time.time() - t0
    if args.simplify_nfaces is not None and len(mesh.faces):
        from slice3d_amd.mesh_simplify import simplify_mesh
        torch.cuda.synchronize()
        t0 = time.time()
        mesh = simplify_mesh(mesh, args.simplify_nfaces, 5.)
        stats["time (simplify)"] = time.time() - t0
    mesh.export(path_mesh)
    print(path_mesh, "%d verts %d faces" % (len(mesh.vertices), len(mesh.faces)), stats)


def main():
    args = get_parser().parse_args()
    if args.name_model == "slicenet":
        model = Slices3DRegModel(img_size=args.img_size, n_slices=args.n_slices, mode=args.mode)
    elif args.name_model == "gtslice":   # regression from given slices (model_gt.py; --from_which_slices gt|gen|gt_rec)
        from slice3d_amd.models_gt import Slices3DGTModel
        model = Slices3DGTModel(img_size=args.img_size, n_slices=args.n_slices, mode=args.mode)
    else:
        raise SystemExit("--name_model %s is not built (DISN: SURVEY.md section 2, out of scope)" % args.name_model)
    path_ckpt = os.path.join("experiments", args.name_exp, "ckpt", args.name_ckpt)
    if os.path.isfile(path_ckpt):
        model.load_state_dict(torch.load(path_ckpt, map_location="cpu")["model"])     # strict, as the reference
    elif args.synthetic_weights:   # smoke tests without a trained checkpoint; never silently
        print("checkpoint %s not found: --synthetic_weights -> name-seeded random weights" % path_ckpt)
        from slice3d_amd.weights import load_seeded
        load_seeded(model, 0)
    else:   # the reference fails here too (reconstruct.py:343 torch.load)
        raise FileNotFoundError("checkpoint %s not found (check --name_exp / --name_ckpt; --synthetic_weights runs on "
                                "random weights for smoke tests)" % path_ckpt)
    model = model.cuda().eval()
    path_res = os.path.join("experiments", args.name_exp, "results", args.name_dataset)
    os.makedirs(path_res, exist_ok=True)
    generator = Generator3D(model, threshold=args.mc_threshold, resolution0=args.mc_res0,
                            upsampling_steps=args.mc_up_steps, chunk_size=args.mc_chunk_size,
                            pred_type=args.pred_type)
    if args.name_dataset != "synthetic":
        from slice3d_amd.datasets import Slice3DDataset
        dataset = Slice3DDataset(split="test", args=args)
    else:
        dataset = SyntheticSlice3DDataset(args.synthetic_len, args.img_size, 16, args.n_slices, split="test")
    if args.gen_ckpt:
        if args.name_model != "gtslice" or args.from_which_slices != "gen" or args.name_dataset == "synthetic":
            raise SystemExit("--gen_ckpt needs --name_model gtslice --from_which_slices gen and an on-disk dataset")
        return reconstruct_generated(args, generator, path_res)
    with torch.no_grad():
        for idx in range(len(dataset)):
            shape = dataset.files[idx][1] if hasattr(dataset, "files") else "synthetic_%04d" % idx
            path_mesh = os.path.join(path_res, shape + ".obj")
            if not args.overwrite_res and os.path.exists(path_mesh):
                continue
            data = {k: v.unsqueeze(0).cuda() for k, v in dataset[idx].items()}
            mesh, stats = generator.generate_mesh(data)
            export_mesh(args, mesh, stats, path_mesh)


def reconstruct_generated(args, generator, path_res):
    """The in-memory gen route: one generate() per batch of test objects, then a mesh per object."""
    from slice3d_amd import gen_route
    from slice3d_amd.datasets import Slice3DDataset
    if os.path.isfile(args.gen_ckpt):
        diffusion = gen_route.load_ldm_checkpoint(args.gen_ckpt)
    elif args.synthetic_weights:
        print("LDM checkpoint %s not found: --synthetic_weights -> name-seeded random weights" % args.gen_ckpt)
        diffusion = gen_route.synthetic_slice_diffusion(0)
    else:
        raise FileNotFoundError("LDM checkpoint %s not found" % args.gen_ckpt)
    diffusion = diffusion.cuda().eval()
    dataset = Slice3DDataset(split="test", args=args, with_slices=False)
    views = gen_route.ObjaverseLdmDataset(dataset.dir_dataset, "test", size=args.img_size, with_slices=False)
    todo = [idx for idx in range(len(dataset)) if args.overwrite_res or
            not os.path.exists(os.path.join(path_res, dataset.files[idx][1] + ".obj"))]
    rng = torch.Generator(device="cuda").manual_seed(args.gen_seed)
    with torch.no_grad():
        for lo in range(0, len(todo), args.n_bs):
            chunk = todo[lo:lo + args.n_bs]
            ipt = np.stack([views.input_view(dataset.files[idx][1]) for idx in chunk])
            img = torch.from_numpy((ipt / 127.5 - 1.0).astype(np.float32)).permute(0, 3, 1, 2).contiguous()
            slices = diffusion.generate(img, ddim_steps=args.ddim_steps, eta=1.0, generator=rng)
            img_slices = gen_route.gen_slices_to_model_input(gen_route.slices_to_mosaic_u8(slices))
            for j, idx in enumerate(chunk):
                path_mesh = os.path.join(path_res, dataset.files[idx][1] + ".obj")
                data = {k: v.unsqueeze(0).cuda() for k, v in dataset[idx].items()}
                data["img_slices"] = img_slices[j:j + 1]
                mesh, stats = generator.generate_mesh(data)
                export_mesh(args, mesh, stats, path_mesh)


if __name__ == "__main__":
    main()

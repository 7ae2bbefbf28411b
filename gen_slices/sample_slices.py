"""sample_slices.py — slice mosaics of the test split from a LatentDiffusion checkpoint (the reference's
`main.py --base configs/latent-diffusion/objaverse-ldm-kl-8-infer.yaml`, LatentDiffusion.test_step, ddpm.py:368-397):

    python gen_slices/sample_slices.py --ckpt logs/<run>/checkpoints/last.ckpt --name_dataset objaverse --dir_data ../data

For each batch of --n_bs objects of 03_splits/test.lst (view 004) it writes {batch}_{case}.png (the 512 x 512 mosaic of the
12 generated slices) and {batch}_{case}_ipt.png (the input view) under --out_dir, by default <ckpt dir>/../images_testing_sampled.
gen_slices/re_org_slices.py --type_slices gen then cuts the mosaics into 04_img_slices_gen/.
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from slice3d_amd import gen_route  # noqa: E402


def get_parser():
    p = argparse.ArgumentParser()
    p.add_argument("--ckpt", type=str, required=True, help="LatentDiffusion checkpoint ({'state_dict': ...})")
    p.add_argument("--name_dataset", type=str, default="objaverse")
    p.add_argument("--dir_data", type=str, default="../data")
    p.add_argument("--n_bs", type=int, default=8)
    p.add_argument("--ddim_steps", type=int, default=200)
    p.add_argument("--eta", type=float, default=1.0)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--out_dir", type=str, default="", help="default: <ckpt dir>/../images_testing_sampled")
    p.add_argument("--no_ema", action="store_true", help="sample with the trained weights instead of their EMA")
    p.add_argument("--synthetic_weights", action=argparse.BooleanOptionalAction,
                   help="run on name-seeded random weights when --ckpt does not exist (smoke tests only)")
    return p


def main(argv=None):
    args = get_parser().parse_args(argv)
    if os.path.isfile(args.ckpt):
        model = gen_route.load_ldm_checkpoint(args.ckpt, use_ema=not args.no_ema)
    elif args.synthetic_weights:
        print("checkpoint %s not found: --synthetic_weights -> name-seeded random weights" % args.ckpt)
        model = gen_route.synthetic_slice_diffusion(0)
    else:
        raise FileNotFoundError("checkpoint %s not found" % args.ckpt)
    model = model.cuda().eval()
    dataset = gen_route.ObjaverseLdmDataset(os.path.join(args.dir_data, args.name_dataset), "test")
    out_dir = args.out_dir or gen_route.default_out_dir(args.ckpt, "images_testing_sampled")
    rng = torch.Generator(device="cuda").manual_seed(args.seed)
    n = gen_route.sample_slices(model, dataset, out_dir, n_bs=args.n_bs, ddim_steps=args.ddim_steps, eta=args.eta, generator=rng)
    print("%d objects sampled -> %s" % (n, out_dir))


if __name__ == "__main__":
    main()

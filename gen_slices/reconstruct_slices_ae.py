"""reconstruct_slices_ae.py — the ground-truth slices of train + val passed through the kl-f8 autoencoder, the gt_rec
training data of the GT model (the reference's `main.py --base configs/autoencoder/autoencoder_kl_f8_infer.yaml`,
AutoencoderKL.test_step on ObjaverseTrainValRec, autoencoder.py:404-440):

    python gen_slices/reconstruct_slices_ae.py --ckpt logs/autoencoder_kl_f8/checkpoints/model.ckpt --name_dataset objaverse

Item i is object i % n of 03_splits/trainval.lst in view i // n (n objects, 12 views); each batch of --n_bs 13-tile stacks
(12 slices + the input view) is encoded, its posterior sampled and decoded, and {batch}_{case}.png (the 12 reconstructed
slices as a 512 x 512 mosaic) is written under --out_dir, by default <ckpt dir>/../images_reconstructed.
gen_slices/re_org_slices.py --type_slices rec then cuts the mosaics into 05_img_slices_rec/.
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from slice3d_amd import gen_route  # noqa: E402


def get_parser():
    p = argparse.ArgumentParser()
    p.add_argument("--ckpt", type=str, required=True, help="kl-f8 AutoencoderKL checkpoint ({'state_dict': ...})")
    p.add_argument("--name_dataset", type=str, default="objaverse")
    p.add_argument("--dir_data", type=str, default="../data")
    p.add_argument("--n_bs", type=int, default=8)
    p.add_argument("--n_views", type=int, default=12)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--out_dir", type=str, default="", help="default: <ckpt dir>/../images_reconstructed")
    p.add_argument("--synthetic_weights", action=argparse.BooleanOptionalAction,
                   help="run on name-seeded random weights when --ckpt does not exist (smoke tests only)")
    return p


def main(argv=None):
    args = get_parser().parse_args(argv)
    if os.path.isfile(args.ckpt):
        ae = gen_route.load_autoencoder_checkpoint(args.ckpt)
    elif args.synthetic_weights:
        print("checkpoint %s not found: --synthetic_weights -> name-seeded random weights" % args.ckpt)
        ae = gen_route.synthetic_autoencoder(0)
    else:
        raise FileNotFoundError("checkpoint %s not found" % args.ckpt)
    ae = ae.cuda().eval()
    dataset = gen_route.ObjaverseLdmDataset(os.path.join(args.dir_data, args.name_dataset), "trainval_rec", n_views=args.n_views)
    out_dir = args.out_dir or gen_route.default_out_dir(args.ckpt, "images_reconstructed")
    rng = torch.Generator(device="cuda").manual_seed(args.seed)
    n = gen_route.reconstruct_slices(ae, dataset, out_dir, n_bs=args.n_bs, generator=rng)
    print("%d slice stacks reconstructed -> %s" % (n, out_dir))


if __name__ == "__main__":
    main()

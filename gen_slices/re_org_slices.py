"""re_org_slices.py — cut the mosaics of sample_slices.py / reconstruct_slices_ae.py into the per-slice images
Slice3DDataset reads (the reference's gen_slices/re_org_slices.py, with its flags and an added --dir_data):

    python gen_slices/re_org_slices.py --dir_slices logs/<run>/images_testing_sampled --type_slices gen --name_dataset objaverse
    python gen_slices/re_org_slices.py --dir_slices logs/autoencoder_kl_f8/images_reconstructed --type_slices rec ...

Mosaic rows X | Z | Y become X_1..X_4, Z_4..Z_1, Y_1..Y_4 under <dir_data>/<name_dataset>/04_img_slices_gen/<uid>/004/
(gen) or 05_img_slices_rec/<uid>/<view>/ (rec; slice files that already exist are kept, as in the reference).

Known divergence: the reference pairs mosaic {batch}_{case} (item batch * n_bs + case) with an object and a view through
open(trainval.lst).read().split('\\n'), while the dataset that produced the mosaics read the file with splitlines().  When
trainval.lst ends with a newline, read().split('\\n') holds one extra, empty id, and every view after the first is paired
with the wrong object.  Here mosaics are paired by the dataset's own indexing (object i % n, view i // n), which is the
reference's result for a file without the trailing newline.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from slice3d_amd.gen_route import mosaic_to_slice_files  # noqa: E402


def get_parser():
    p = argparse.ArgumentParser()
    p.add_argument("--dir_slices", type=str, default="logs/2024-04-23T02-11-33_objaverse-ldm-kl-8/images_testing_sampled")
    p.add_argument("--type_slices", type=str, default="gen", choices=["gen", "rec"])
    p.add_argument("--name_dataset", type=str, default="objaverse")
    p.add_argument("--img_size", type=int, default=128)
    p.add_argument("--n_bs", type=int, default=8)
    p.add_argument("--n_views", type=int, default=12)
    p.add_argument("--dir_data", type=str, default="../data")
    return p


def main(argv=None):
    args = get_parser().parse_args(argv)
    n = mosaic_to_slice_files(args.dir_slices, os.path.join(args.dir_data, args.name_dataset), args.type_slices,
                              n_bs=args.n_bs, img_size=args.img_size, n_views=args.n_views)
    print("%d mosaics cut" % n)


if __name__ == "__main__":
    main()

"""create_dataset_sin_img.py — a one-object dataset from one RGBA image, for the image -> slices -> mesh demo (the
reference's create_dataset_sin_img.py; same tree, same meta.pkl, same centring):

    python create_dataset_sin_img.py --img_path input.png --name_dataset custom_sin_img

<dir_data>/<name_dataset>/
    00_img_input/00000/004.png     the image, its alpha bounding box moved to the centre (--center_obj, default on)
    00_img_input/00000/meta.pkl    [K 0, azimuths 0, elevations 0, distances 1.2, cam_poses 0, scale 1.0, offset 0]
    01_img_slices/00000/004/{X,Y,Z}_{1..4}.png   transparent placeholders of --img_size
    02_sdfs/00000.npy              (16384, 4) zeros
    03_splits/{train,val,test}.lst "00000" (no trailing newline)

Then, for example: python reg_slices/reconstruct.py --name_model gtslice --from_which_slices gen --gen_ckpt <ldm.ckpt>
--name_dataset custom_sin_img --dir_data ./data --img_size 128 --n_bs 1 --name_exp <exp> --name_ckpt <gt.ckpt> --mode test
"""
import argparse
import os
import pickle

import numpy as np
from PIL import Image

OBJECT_UID = "00000"


def get_parser():
    p = argparse.ArgumentParser()
    p.add_argument("--img_path", type=str, default="./imgs/demo/input.png")
    p.add_argument("--name_dataset", type=str, default="custom_sin_img")
    p.add_argument("--img_size", type=int, default=256)
    p.add_argument("--resize_img", action=argparse.BooleanOptionalAction, default=False)
    p.add_argument("--center_obj", action=argparse.BooleanOptionalAction, default=True)
    p.add_argument("--dir_data", type=str, default="./data")
    return p


def center_by_alpha(img):
    """Move the alpha bounding box to the centre of the canvas (integer offsets, as the reference computes them)."""
    alpha = img.split()[3]
    bbox = alpha.getbbox()
    width, height = img.size
    offset_x = (width - (bbox[2] - bbox[0])) // 2 - bbox[0]
    offset_y = (height - (bbox[3] - bbox[1])) // 2 - bbox[1]
    out = Image.new("RGBA", (width, height), (0, 0, 0, 0))
    out.paste(img, (offset_x, offset_y), mask=alpha)
    return out


def create_dataset(args):
    dir_tgt = os.path.join(args.dir_data, args.name_dataset)
    for sub in ("00_img_input", "01_img_slices", "02_sdfs", "03_splits"):
        os.makedirs(os.path.join(dir_tgt, sub), exist_ok=True)
    img = Image.open(args.img_path)
    if img.mode != "RGBA":
        raise ValueError("%s: an RGBA image is needed (the alpha channel marks the object), got mode %s" % (args.img_path, img.mode))
    dir_ipt = os.path.join(dir_tgt, "00_img_input", OBJECT_UID)
    os.makedirs(dir_ipt, exist_ok=True)
    if args.center_obj:
        img = center_by_alpha(img)
    if args.resize_img:
        img = img.resize((args.img_size, args.img_size), Image.LANCZOS)
    img.save(os.path.join(dir_ipt, "004.png"), "PNG")
    meta = [np.zeros((3, 3)), np.zeros(12), np.zeros(12), np.ones(12) * 1.2, np.zeros((12, 3, 4)), 1.0, np.zeros(3)]
    with open(os.path.join(dir_ipt, "meta.pkl"), "wb") as f:
        pickle.dump(meta, f)
    dir_sl = os.path.join(dir_tgt, "01_img_slices", OBJECT_UID, "004")
    os.makedirs(dir_sl, exist_ok=True)
    for axis in "XYZ":
        for part in "1234":
            Image.new("RGBA", (args.img_size, args.img_size)).save(os.path.join(dir_sl, "%s_%s.png" % (axis, part)))
    np.save(os.path.join(dir_tgt, "02_sdfs", OBJECT_UID + ".npy"), np.zeros((16384, 4)))
    for split in ("train", "val", "test"):
        with open(os.path.join(dir_tgt, "03_splits", split + ".lst"), "w") as f:
            f.write(OBJECT_UID)
    return dir_tgt


if __name__ == "__main__":
    create_dataset(get_parser().parse_args())

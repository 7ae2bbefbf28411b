"""The generation-based slicing route around SliceDiffusion and AutoencoderKL, from data on disk to slice images and back
(reference gen_slices/: ldm/data/objaverse.py ObjaverseBase, LatentDiffusion.test_step ddpm.py:368-397,
AutoencoderKL.test_step autoencoder.py:404-440, re_org_slices.py).

    ObjaverseLdmDataset        the LDM's input data: white-background tiles X1-4 | Z4-1 | Y1-4 | input view in [-1, 1]
    load_ldm_checkpoint        LatentDiffusion .ckpt -> SliceDiffusion (EMA weights by default)
    load_autoencoder_checkpoint  kl-f8 .ckpt -> AutoencoderKL (the loss.* keys of its training losses are dropped)
    slices_to_mosaic_u8        test_step's 512 x 512 mosaic: rows X | Z | Y | zero pad, clamp, (x + 1) / 2, * 255, truncate
    sample_slices              test_step of the LDM: {batch}_{case}.png + {batch}_{case}_ipt.png
    reconstruct_slices         test_step of the autoencoder on the 13-tile stacks: {batch}_{case}.png
    mosaic_to_slice_files      re_org_slices.py: mosaics -> 04_img_slices_gen/<uid>/004/ or 05_img_slices_rec/<uid>/<view>/
    gen_slices_to_model_input  what Slice3DDataset makes of a `gen` slice PNG, from the mosaic in memory

Every device step (condition encoder, DDIM U-Net, autoencoder) runs on libslice3d_hip.so; the functions here only move,
quantise and write images.
"""
import os

import numpy as np
import torch
from PIL import Image

N_VIEWS = 12
GEN_VIEW = 4
SLICE_ORDER = (("X", "1234"), ("Z", "4321"), ("Y", "1234"))     # mosaic rows 0, 1, 2 / tiles 0-3, 4-7, 8-11
SUBDIR = {"gen": "04_img_slices_gen", "rec": "05_img_slices_rec"}


def read_split(root, split):
    """Object ids of 03_splits/<split>.lst as ObjaverseBase reads them (splitlines: a trailing newline adds no id)."""
    with open(os.path.join(root, "03_splits", split + ".lst")) as f:
        return f.read().splitlines()


def png_2_whitebg(img):
    """ObjaverseBase.png_2_whitebg: RGB where alpha > 0, white where alpha == 0 (a hard replacement, not a blend)."""
    a = np.array(img)
    rgb, alpha0 = a[:, :, 0:3], (a[:, :, 3:4] == 0).astype(np.float32)
    return Image.fromarray((np.ones(rgb.shape) * 255 * alpha0 + rgb * (1 - alpha0)).astype(np.uint8))


class ObjaverseLdmDataset(torch.utils.data.Dataset):
    """ObjaverseBase (objaverse.py:9-99) for split 'test' (03_splits/test.lst, view 004) or 'trainval_rec'
    (03_splits/trainval.lst repeated n_views times, view i // n_ids).  Item: {'file_path_': uid, 'view': int,
    'img_ipt_view': (S, S, 3) float32, 'image': (S, S, 39) float32 (with_slices only)}, values u8 / 127.5 - 1.
    with_slices defaults to True for 'trainval_rec' (the autoencoder's input) and False for 'test' (the LDM reads only the
    input view, so the ground-truth slices need not exist)."""

    def __init__(self, root, split, size=128, n_views=N_VIEWS, with_slices=None):
        if split not in ("test", "trainval_rec"):
            raise ValueError("split must be 'test' or 'trainval_rec', got %r" % (split,))
        self.root, self.split, self.size, self.n_views = root, split, size, n_views
        self.ids = read_split(root, "test" if split == "test" else "trainval")
        self.n_ids = len(self.ids)
        self.uids = self.ids * n_views if split == "trainval_rec" else list(self.ids)
        self.with_slices = split == "trainval_rec" if with_slices is None else with_slices

    def __len__(self):
        return len(self.uids)

    def view(self, i):
        return GEN_VIEW if self.split == "test" else i // self.n_ids

    def _tile(self, path):
        img = png_2_whitebg(Image.open(path)).resize((self.size, self.size), resample=Image.BILINEAR)
        return np.array(img)

    def input_view(self, uid, view=GEN_VIEW):
        """(S, S, 3) uint8 of 00_img_input/<uid>/<view>.png."""
        return self._tile(os.path.join(self.root, "00_img_input", uid, "%03d.png" % view))

    def __getitem__(self, i):
        uid, view = self.uids[i], self.view(i)
        ipt = self.input_view(uid, view)
        item = {"file_path_": uid, "view": view, "img_ipt_view": (ipt / 127.5 - 1.0).astype(np.float32)}
        if self.with_slices:
            tiles = [self._tile(os.path.join(self.root, "01_img_slices", uid, "%03d" % view, "%s_%s.png" % (axis, part)))
                     for axis, parts in SLICE_ORDER for part in parts]
            item["image"] = (np.concatenate(tiles + [ipt], -1) / 127.5 - 1.0).astype(np.float32)
        return item


def batches(dataset, n_bs):
    """In-order batches of the dataset (the last may be short), as a non-shuffling DataLoader gives them to test_step."""
    for b, lo in enumerate(range(0, len(dataset), n_bs)):
        items = [dataset[i] for i in range(lo, min(lo + n_bs, len(dataset)))]
        out = {k: [it[k] for it in items] for k in items[0]}
        for k in ("img_ipt_view", "image"):
            if k in out:
                out[k] = torch.from_numpy(np.stack(out[k]))
        yield b, out


# ---------------------------------------------------------------------------------------------------------- checkpoints
def _load_state_dict(path):
    # a Lightning checkpoint pickles its hyper-parameters and loop state next to the weights; as with the reference's
    # torch.load, only load files you trust
    ckpt = torch.load(path, map_location="cpu", weights_only=False)
    return ckpt["state_dict"] if "state_dict" in ckpt else ckpt


def load_ldm_checkpoint(path, use_ema=True, **kw):
    """LatentDiffusion checkpoint ({'state_dict': ...}) -> SliceDiffusion (ldm_pipeline.SliceDiffusion.from_state_dict)."""
    from .ldm_pipeline import SliceDiffusion
    return SliceDiffusion.from_state_dict(_load_state_dict(path), use_ema=use_ema, **kw)


def autoencoder_state_dict(sd):
    """The kl-f8 checkpoint without the loss.* entries (LPIPSWithDiscriminator: perceptual net, discriminator, logvar), which
    the reference skips through strict=False; every other key must match AutoencoderKL exactly."""
    return {k: v for k, v in sd.items() if not k.startswith("loss.")}


def load_autoencoder_checkpoint(path, backend="hip", prec="f16x3", ddconfig=None, embed_dim=4):
    from .ldm_autoencoder import KL_F8, AutoencoderKL
    ae = AutoencoderKL(ddconfig or KL_F8, embed_dim, backend=backend, prec=prec)
    ae.load_state_dict(autoencoder_state_dict(_load_state_dict(path)), strict=True)
    return ae


def synthetic_slice_diffusion(seed=0, scale_factor=0.18215, prec="f16x3"):
    """SliceDiffusion with name-seeded weights (smoke runs and tests without a trained checkpoint)."""
    from .ldm_autoencoder import KL_F8, AutoencoderKL, ImageEncoderVGG16BN
    from .ldm_pipeline import UNET_CFG, SliceDiffusion
    from .ldm_unet import UNetModel
    from .weights import load_seeded
    return SliceDiffusion(load_seeded(UNetModel(prec=prec, **UNET_CFG), seed), load_seeded(AutoencoderKL(KL_F8, 4, prec=prec), seed),
                          load_seeded(ImageEncoderVGG16BN(prec=prec), seed), scale_factor)


def synthetic_autoencoder(seed=0, prec="f16x3"):
    from .ldm_autoencoder import KL_F8, AutoencoderKL
    from .weights import load_seeded
    return load_seeded(AutoencoderKL(KL_F8, 4, prec=prec), seed)


# --------------------------------------------------------------------------------------------------------------- images
def slices_to_mosaic_u8(slices):
    """(B, 3 n, S, S) tiles in [-1, 1] (n >= 12; tiles past the 12th are not shown) -> (B, 4S, 4S, 3) uint8 on the same
    device: tiles 0-3 | 4-7 | 8-11 as rows, a zero row, then clamp(-1, 1), (x + 1) / 2, * 255 and a truncating cast, one
    fp32 operation at a time as test_step does them (ddpm.py:379-396, autoencoder.py:411-431)."""
    x = slices.float()
    b, c, h, w = x.shape
    t = x.view(b, c // 3, 3, h, w)
    rows = [t[:, 4 * r:4 * r + 4].permute(0, 2, 3, 1, 4).reshape(b, 3, h, 4 * w) for r in range(3)]
    grid = torch.cat(rows + [torch.zeros_like(rows[0])], 2)
    grid = torch.clamp(grid, -1.0, 1.0)
    grid = (grid + 1.0) / 2.0
    grid = grid.permute(0, 2, 3, 1) * 255
    return grid.to(torch.uint8)


def input_view_u8(img_ipt_view):
    """test_step's {batch}_{case}_ipt.png: (x + 1) * 127.5 in fp32, truncated."""
    return ((np.asarray(img_ipt_view, dtype=np.float32) + 1) * 127.5).astype(np.uint8)


_U8_TO_MODEL = ((torch.arange(256, dtype=torch.float32).div(255.0)) - 0.5) / 0.5     # Slice3DDataset's ToTensor + Normalize


def gen_slices_to_model_input(mosaic_u8):
    """(B, 4S, 4S, 3) uint8 mosaics -> (B, 36, S, S) float32 img_slices, bit for bit what Slice3DDataset(from_which_slices=
    'gen') reads from the 12 PNGs mosaic_to_slice_files cuts (u8 / 255, then (v - 0.5) / 0.5, as a 256-entry table computed
    by the same operations on the CPU)."""
    b, h4, w4, _ = mosaic_u8.shape
    s = h4 // 4
    tiles = mosaic_u8[:, :3 * s].reshape(b, 3, s, 4, s, 3).permute(0, 1, 3, 5, 2, 4).reshape(b, 36, s, s)
    return _U8_TO_MODEL.to(mosaic_u8.device)[tiles.long()]


def _save_png(arr, path):
    Image.fromarray(np.ascontiguousarray(arr)).save(path)


# --------------------------------------------------------------------------------------------------------------- stages
def default_out_dir(ckpt, name):
    """test_step's '/'.join(ckpt_path.split('/')[:-2]) + '/' + name: beside the checkpoint's directory."""
    return os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(ckpt))), name)


@torch.no_grad()
def sample_slices(model, dataset, out_dir, n_bs=8, ddim_steps=200, eta=1.0, generator=None, noises=None, log=print):
    """LatentDiffusion.test_step over `dataset` (an ObjaverseLdmDataset 'test'): generate() per batch of n_bs input views,
    write {batch}_{case}.png (the slice mosaic) and {batch}_{case}_ipt.png.  noises: optional callable (batch index, batch
    size) -> the noises dict of SliceDiffusion.generate.  Returns the number of objects written."""
    os.makedirs(out_dir, exist_ok=True)
    n = 0
    for b, batch in batches(dataset, n_bs):
        views = batch["img_ipt_view"].permute(0, 3, 1, 2).contiguous()
        slices = model.generate(views, ddim_steps=ddim_steps, eta=eta, generator=generator,
                                noises=noises(b, views.shape[0]) if noises is not None else None)
        mosaic = slices_to_mosaic_u8(slices).cpu().numpy()
        ipt = input_view_u8(batch["img_ipt_view"].numpy())
        for c in range(views.shape[0]):
            _save_png(ipt[c], os.path.join(out_dir, "%d_%d_ipt.png" % (b, c)))
            _save_png(mosaic[c], os.path.join(out_dir, "%d_%d.png" % (b, c)))
        n += views.shape[0]
        if log:
            log("batch %d: %d objects -> %s" % (b, views.shape[0], out_dir))
    return n


@torch.no_grad()
def autoencode_stacks(ae, image, generator=None, noise=None):
    """AutoencoderKL.forward (autoencoder.py:347-355) on (B, S, S, 39) 13-tile stacks: encode every tile, sample the
    posterior (noise: (13 B, 4, S/8, S/8) draws, else the generator's), decode(after_diffusion=False) -> (B, 39, S, S)."""
    dev = ae._device()
    b, s, _, c = image.shape
    x = image.to(dev, torch.float32).permute(0, 3, 1, 2).reshape(b * c // 3, 3, s, s).contiguous()
    z = ae.encode(x).sample(noise, generator)
    return ae.decode(z, after_diffusion=False).reshape(b, c, s, s)


@torch.no_grad()
def reconstruct_slices(ae, dataset, out_dir, n_bs=8, generator=None, noises=None, log=print):
    """AutoencoderKL.test_step over `dataset` (an ObjaverseLdmDataset 'trainval_rec'): {batch}_{case}.png mosaics of the
    reconstructed tiles.  noises: optional callable (batch index, batch size) -> posterior draws (13 B, 4, S/8, S/8)."""
    os.makedirs(out_dir, exist_ok=True)
    n = 0
    for b, batch in batches(dataset, n_bs):
        nb = batch["image"].shape[0]
        rec = autoencode_stacks(ae, batch["image"], generator, noises(b, nb) if noises is not None else None)
        mosaic = slices_to_mosaic_u8(rec).cpu().numpy()
        for c in range(nb):
            _save_png(mosaic[c], os.path.join(out_dir, "%d_%d.png" % (b, c)))
        n += nb
        if log:
            log("batch %d: %d stacks -> %s" % (b, nb, out_dir))
    return n


def mosaic_to_slice_files(dir_slices, data_root, type_slices, n_bs=8, img_size=128, n_views=N_VIEWS):
    """re_org_slices.py crop_slices: cut each {batch}_{case}.png into X_1..4, Z_4..1, Y_1..4 (rows 0, 1, 2) under
    04_img_slices_gen/<uid>/004/ ('gen') or 05_img_slices_rec/<uid>/<view>/ ('rec', existing files are kept).  Mosaic i
    is dataset item i of ObjaverseLdmDataset ('test' / 'trainval_rec'): the pairing follows the dataset's own splitlines
    indexing (the reference's read().split('\\n') shifts the views when trainval.lst ends with a newline).
    Returns the number of mosaics cut."""
    ds = ObjaverseLdmDataset(data_root, "test" if type_slices == "gen" else "trainval_rec", size=img_size, n_views=n_views,
                             with_slices=False)
    dir_tgt = os.path.join(data_root, SUBDIR[type_slices])
    done = 0
    for idx, uid in enumerate(ds.uids):
        src = os.path.join(dir_slices, "%d_%d.png" % (idx // n_bs, idx % n_bs))
        if not os.path.exists(src):
            continue
        img = Image.open(src)
        d = os.path.join(dir_tgt, uid, "%03d" % ds.view(idx))
        os.makedirs(d, exist_ok=True)
        for i, (axis, parts) in enumerate(SLICE_ORDER):
            for j, part in enumerate(parts):
                path = os.path.join(d, "%s_%s.png" % (axis, part))
                if type_slices == "rec" and os.path.exists(path):
                    continue
                img.crop((j * img_size, i * img_size, (j + 1) * img_size, (i + 1) * img_size)).save(path)
        done += 1
    return done

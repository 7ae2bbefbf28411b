"""Goldens of the REAL reference gen_slices first stage and condition encoder (ldm/models/autoencoder.py AutoencoderKL,
ldm/modules/diffusionmodules/model.py, ldm/modules/encoders/modules.py ImageEncoderVGG16BN) with name-seeded weights, and of
the generative route composed from the reference's pieces as LatentDiffusion runs it (get_input -> DDIMSampler ->
decode_first_stage, ddpm.py:478-520, :749-830).  Every noise the reference draws is recorded.  Authoring container only:

    python tests/golden/make_golden_ldm_ae.py
"""
import json
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle.ref_import import LDM_FULL, LDM_ROOT, _install_torchvision_stub, build_reference_ldm_unet  # noqa: E402
from slice3d_amd.weights import load_seeded  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
AE_SMALL = dict(double_z=True, z_channels=4, resolution=32, in_channels=3, out_ch=3, ch=32, ch_mult=[1, 2], num_res_blocks=1,
                attn_resolutions=[], dropout=0.0)
KL_F8 = dict(double_z=True, z_channels=4, resolution=512, in_channels=3, out_ch=3, ch=128, ch_mult=[1, 2, 4, 4],
             num_res_blocks=2, attn_resolutions=[], dropout=0.0)
SCALE_FACTOR = 0.18215
DDIM_STEPS = 2


def _stub(name, **attrs):
    m = types.ModuleType(name)
    for k, v in attrs.items():
        setattr(m, k, v)
    sys.modules[name] = m
    return m


def import_reference():
    """The reference's AutoencoderKL / ImageEncoderVGG16BN modules with their unused training-time imports stubbed."""
    _install_torchvision_stub()
    pl = _stub("pytorch_lightning", LightningModule=nn.Module)
    pl.utilities = _stub("pytorch_lightning.utilities")
    _stub("taming")
    _stub("taming.modules")
    _stub("taming.modules.vqvae")
    _stub("taming.modules.vqvae.quantize", VectorQuantizer2=nn.Module)
    _stub("clip")
    _stub("kornia")
    if LDM_ROOT not in sys.path:
        sys.path.insert(0, LDM_ROOT)
    from ldm.models.autoencoder import AutoencoderKL
    from ldm.modules.encoders.modules import ImageEncoderVGG16BN
    import ldm.modules.diffusionmodules.model  # noqa: F401
    return AutoencoderKL, ImageEncoderVGG16BN


def reference_ae(ddconfig):
    AutoencoderKL, _ = import_reference()
    m = AutoencoderKL(ddconfig, {"target": "torch.nn.Identity"}, embed_dim=4)
    return load_seeded(m, 0).eval()


def reference_cond():
    _, ImageEncoderVGG16BN = import_reference()
    return load_seeded(ImageEncoderVGG16BN(), 0).eval()


def _images(n, size, seed):     # tests/test_ldm_ae.py draws the same images
    g = torch.Generator().manual_seed(seed)
    return torch.rand((n, 3, size, size), generator=g) * 2 - 1


def _mosaic(seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn((1, 4, 64, 64), generator=g)


def ae_golden(name, ddconfig, size, mosaic=True):
    """Encoder moments of one image, and the decode of a latent: the whole 4 x 4 mosaic (reshape_z -> post_quant_conv ->
    decoder -> (1, 39, S, S)) or, to keep the kl-f8 file small, one 16 x 16 tile (post_quant_conv -> decoder -> (1, 3, S, S))."""
    ae = reference_ae(ddconfig)
    x = _images(1, size, 21)
    z = _mosaic(22)
    if not mosaic:
        z = z[:, :, :16, :16].contiguous()
    with torch.no_grad():
        moments = ae.quant_conv(ae.encoder(x))     # AutoencoderKL.encode without its 13-image view (one image)
        # (the reference's decode() always views its output as 13-image stacks: one tile goes through its two stages)
        dec = ae.decode(z, after_diffusion=True) if mosaic else ae.decoder(ae.post_quant_conv(z))
    np.savez_compressed(os.path.join(OUT, name + ".npz"), x=x.numpy(), moments=moments.numpy(), z=z.numpy(), dec=dec.numpy())
    print(name, "moments", tuple(moments.shape), "dec", tuple(dec.shape), "max|dec| %.3f" % float(dec.abs().max()))
    return ae


def cond_golden():
    cond = reference_cond()
    img = _images(1, 128, 31)
    with torch.no_grad():
        f = cond(img)
    np.savez_compressed(os.path.join(OUT, "ldm_cond_b1.npz"), img=img.numpy(), **{k: v.numpy() for k, v in f.items()})
    print("cond", {k: tuple(v.shape) for k, v in f.items()})
    with open(os.path.join(OUT, "state_dict_keys_ldm_cond.json"), "w") as fh:
        json.dump({k: list(v.shape) for k, v in cond.state_dict().items()}, fh, indent=0)
    return cond


def e2e_golden(ae, cond):
    """img_ipt_view = image 12 of the 13-image stack (objaverse.py:80-90) -> get_input's c_concat / c_fmaps -> 2 DDIM steps of
    the full U-Net (EMA weights = the seeded weights here) -> decode_first_stage -> samples[:, :36].  Stored: the drawn noises,
    c_concat, the sampled latent mosaic in full and, of the decoded slices, tile Z4 (channels 33:36, mosaic row 2, column 3);
    the input view is redrawn from its seed."""
    import ldm.models.diffusion.ddim as ddim_mod
    from ldm.modules.diffusionmodules.util import make_beta_schedule
    unet = build_reference_ldm_unet(LDM_FULL)
    stack = _images(13, 128, 41)                       # (13, 3, 128, 128): the `image` entry of one object
    img_ipt_view = stack[12:13].clone()
    x = stack.reshape(1, 39, 128, 128)
    drawn = []
    real_randn = torch.randn

    def recording_randn(*a, **k):
        t = real_randn(*a, **k)
        drawn.append(t.clone())
        return t
    torch.manual_seed(4321)
    with torch.no_grad():
        posterior = ae.encode(x)                       # encode_first_stage
        torch.randn = recording_randn
        try:
            z = SCALE_FACTOR * posterior.sample()      # get_first_stage_encoding
        finally:
            torch.randn = real_randn
        post_noise = drawn[0].reshape(1, 13, 4, 16, 16)[:, 12]
        c_concat = z.view(1, 13, 4, 16, 16)[:, 12].repeat(1, 1, 4, 4)   # ddpm.py:800
        c_fmaps = cond(img_ipt_view)                   # get_learned_conditioning
    x_T = torch.randn((1, 4, 64, 64))

    class Model:      # what DDIMSampler needs of LatentDiffusion (ddpm.py:118-160, 1461-1466)
        num_timesteps = 1000
        device = torch.device("cpu")
        _b = np.asarray(make_beta_schedule("linear", 1000, linear_start=0.0015, linear_end=0.0155))
        betas = torch.tensor(_b, dtype=torch.float32)
        alphas_cumprod = torch.tensor(np.cumprod(1.0 - _b, axis=0), dtype=torch.float32)
        alphas_cumprod_prev = torch.tensor(np.append(1.0, np.cumprod(1.0 - _b, axis=0)[:-1]), dtype=torch.float32)

        def apply_model(self, xt, t, c):
            return unet(torch.cat([xt] + c["c_concat"], dim=1), t, c_fmaps=c["c_fmaps"])

    class CpuSampler(ddim_mod.DDIMSampler):
        def register_buffer(self, name, attr):
            setattr(self, name, attr)

    steps = []
    real_noise_like = ddim_mod.noise_like

    def recording_noise_like(shape, device, repeat=False):
        n = real_noise_like(shape, device, repeat)
        steps.append(n.clone())
        return n
    ddim_mod.noise_like = recording_noise_like
    with torch.no_grad():
        samples, _ = CpuSampler(Model()).sample(DDIM_STEPS, 1, (4, 64, 64), conditioning={"c_concat": [c_concat], "c_fmaps": c_fmaps},
                                                eta=1.0, x_T=x_T, verbose=False)
        dec = ae.decode(samples / SCALE_FACTOR)        # decode_first_stage
    ddim_mod.noise_like = real_noise_like
    out = dec[:, :36]
    np.savez_compressed(os.path.join(OUT, "ldm_ae_e2e_b1.npz"), post_noise=post_noise.numpy(), x_T=x_T.numpy(),
                        steps=np.stack([t.numpy() for t in steps]), samples=samples.numpy(), out_z4=out[:, 33:36].numpy(),
                        c_concat=c_concat.numpy(), meta=np.array([DDIM_STEPS, 41]), scale_factor=np.float32(SCALE_FACTOR))
    print("e2e", tuple(out.shape), "noises", len(steps), "max|out| %.3f" % float(out.abs().max()))


if __name__ == "__main__":
    torch.set_num_threads(os.cpu_count())
    ae_golden("ldm_ae_small", AE_SMALL, 32)
    ae = ae_golden("ldm_ae_kl8", KL_F8, 128, mosaic=False)
    with open(os.path.join(OUT, "state_dict_keys_ldm_ae_kl8.json"), "w") as fh:
        json.dump({k: list(v.shape) for k, v in ae.state_dict().items()}, fh, indent=0)
    cond = cond_golden()
    e2e_golden(ae, cond)

"""SliceDiffusion — the gen_slices generative route from one input view to the 12 slice images
(LatentDiffusion.log_images_when_testing, reference ldm/models/diffusion/ddpm.py:478-520 with get_input :749-810 and
decode_first_stage :812-830; configs/latent-diffusion/objaverse-ldm-kl-8-infer.yaml):

    c_fmaps  = ImageEncoderVGG16BN(img)                               (cond_stage_model)
    c_concat = (AutoencoderKL.encode(img).sample() * scale_factor), repeated 4 x 4
    z_0      = DDIMSampler(UNetModel) from x_T ~ N(0, 1), 200 steps, eta = 1, EMA weights
    slices   = AutoencoderKL.decode(z_0 / scale_factor)[:, :36]      (tiles X1..X4, Y1..Y4, Z1..Z4; the pad tile is skipped)

The result is the `img_slices` tensor Slices3DGTModel.encode reads.
"""
import torch

from .ldm_autoencoder import KL_F8, AutoencoderKL, ImageEncoderVGG16BN, tile_condition
from .ldm_sampler import DDIMSampler
from .ldm_unet import UNetModel

# objaverse-ldm-kl-8-infer.yaml unet_config
UNET_CFG = dict(image_size=64, in_channels=8, out_channels=4, model_channels=192, attention_resolutions=[1, 2, 4, 8],
                num_res_blocks=2, channel_mult=[1, 2, 2, 4, 4], num_heads=8, use_scale_shift_norm=True, resblock_updown=True)


def ema_key(key):
    """LitEma's buffer name of the denoiser parameter `key` (ldm/modules/ema.py: 'diffusion_model.' + key, dots removed)."""
    return "model_ema." + ("diffusion_model." + key).replace(".", "")


class SliceDiffusion(torch.nn.Module):
    N_SLICES = 12

    def __init__(self, unet, first_stage, cond_stage, scale_factor, timesteps=1000, linear_start=0.0015, linear_end=0.0155):
        super().__init__()
        self.unet, self.first_stage, self.cond_stage = unet, first_stage, cond_stage
        self.scale_factor = float(scale_factor)
        self.sampler = DDIMSampler(unet, timesteps, linear_start, linear_end)

    @classmethod
    def from_state_dict(cls, sd, use_ema=True, prec="f16x3", unet_cfg=UNET_CFG, ddconfig=KL_F8, embed_dim=4, backend="hip"):
        """A LatentDiffusion state_dict: model.diffusion_model.* (or, with use_ema, its LitEma copy model_ema.*, which
        log_images_when_testing samples with), first_stage_model.*, cond_stage_model.*, scale_factor.  The schedule buffers
        are recomputed from the configuration, not read."""
        unet = UNetModel(backend=backend, prec=prec, **unet_cfg)
        ae = AutoencoderKL(ddconfig, embed_dim, backend=backend, prec=prec)
        cond = ImageEncoderVGG16BN(backend=backend, prec=prec)

        def sub(prefix):
            return {k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}
        if use_ema:
            usd = {k: sd[ema_key(k)] for k in unet.state_dict()}
        else:
            usd = sub("model.diffusion_model.")
        unet.load_state_dict(usd, strict=True)
        ae.load_state_dict(sub("first_stage_model."), strict=True)
        cond.load_state_dict(sub("cond_stage_model."), strict=True)
        return cls(unet, ae, cond, float(sd["scale_factor"]))

    @torch.no_grad()
    def condition(self, img_ipt_view, posterior_noise=None, generator=None):
        """(c_concat, c_fmaps) of get_input (ddpm.py:753-800) for the (B, 3, S, S) input view in [-1, 1]."""
        c_fmaps = self.cond_stage(img_ipt_view)
        z = self.first_stage.encode(img_ipt_view).sample(posterior_noise, generator) * self.scale_factor
        return tile_condition(z), c_fmaps

    @torch.no_grad()
    def generate(self, img_ipt_view, ddim_steps=200, eta=1.0, generator=None, noises=None, return_latent=False):
        """(B, 3, 128, 128) input views in [-1, 1] -> img_slices (B, 36, 128, 128).  noises: {'posterior': (B, 4, 16, 16),
        'x_T': (B, 4, 64, 64), 'steps': ddim_steps tensors (B, 4, 64, 64)} — the draws to use instead of the generator's.
        return_latent: also return the sampled latent mosaic (B, 4, 64, 64), the reference's `samples` before decoding."""
        noises = noises or {}
        dev = self.unet._device()
        img = img_ipt_view.to(dev, torch.float32).contiguous()
        c_concat, c_fmaps = self.condition(img, noises.get("posterior"), generator)
        x_t = noises.get("x_T")
        if x_t is None:
            x_t = torch.randn(c_concat.shape, device=dev, generator=generator)
        z0, _ = self.sampler.sample(ddim_steps, x_t.to(dev, torch.float32), c_concat, c_fmaps, eta=eta,
                                    noises=noises.get("steps"), generator=generator)
        slices = self.first_stage.decode(z0 / self.scale_factor, after_diffusion=True, n_tiles=self.N_SLICES)
        return (slices, z0) if return_latent else slices

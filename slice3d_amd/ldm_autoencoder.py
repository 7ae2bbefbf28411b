"""AutoencoderKL and ImageEncoderVGG16BN — MI355X-native counterparts of the gen_slices first stage
(ldm/models/autoencoder.py:285-360, blocks in ldm/modules/diffusionmodules/model.py:33-570; configured by
configs/latent-diffusion/objaverse-ldm-kl-8-infer.yaml) and of its condition encoder (ldm/modules/encoders/modules.py:204-267).

Inference only.  The module trees give the reference's state_dict keys (encoder.down.N.block.M.norm1.weight,
decoder.up.N.upsample.conv.weight, decoder.mid.attn_1.q.weight, quant_conv.*, post_quant_conv.*; conv1_2.* ... conv_last.*,
classifier.*, trans1_2.* ... trans5_3.*, mean, std).  Every convolution, GroupNorm, attention and resampling step is an entry
point of libslice3d_hip.so, on channels-last activations, through the operator layer shared with the U-Net (ldm_ops.LdmOps);
there is no CPU fallback.  Host code only moves tensors between layouts (the 4 x 4 latent mosaic, the 4 x 4 repeat of the
condition maps) and draws the posterior sample of a 16 x 16 x 4 latent.
"""
import ctypes as C
import types

import torch
import torch.nn as nn

from . import _lib
from .ldm_ops import LdmOps
from .models import data_ptr
from .models_gt import VGG16BNFeats, gt_encoder_params

KL_F8 = dict(double_z=True, z_channels=4, resolution=512, in_channels=3, out_ch=3, ch=128, ch_mult=[1, 2, 4, 4],
             num_res_blocks=2, attn_resolutions=[], dropout=0.0)   # objaverse-ldm-kl-8-infer.yaml first_stage_config


def _norm(ch):
    return nn.GroupNorm(32, ch, eps=1e-6)


class ResnetBlock(nn.Module):
    """model.py:82-141 without the timestep projection (temb_channels = 0 in the autoencoder)."""

    def __init__(self, in_channels, out_channels):
        super().__init__()
        self.in_channels, self.out_channels = in_channels, out_channels
        self.norm1 = _norm(in_channels)
        self.conv1 = nn.Conv2d(in_channels, out_channels, 3, padding=1)
        self.norm2 = _norm(out_channels)
        self.conv2 = nn.Conv2d(out_channels, out_channels, 3, padding=1)
        if in_channels != out_channels:
            self.nin_shortcut = nn.Conv2d(in_channels, out_channels, 1)


class AttnBlock(nn.Module):
    """model.py:150-202: one attention head as wide as the block."""

    def __init__(self, channels):
        super().__init__()
        self.norm = _norm(channels)
        self.q, self.k, self.v, self.proj_out = (nn.Conv2d(channels, channels, 1) for _ in range(4))


class _Resample(nn.Module):
    def __init__(self, channels):
        super().__init__()
        self.conv = nn.Conv2d(channels, channels, 3, stride=1, padding=1)


class Downsample(_Resample):
    """model.py:60-79 (with_conv): F.pad (0,1,0,1) + Conv2d(3, stride 2)."""


class Upsample(_Resample):
    """model.py:43-57 (with_conv): nearest 2x + Conv2d(3)."""


def _level(blocks, attn):
    m = nn.Module()
    m.block, m.attn = nn.ModuleList(blocks), nn.ModuleList(attn)
    return m


def _mid(ch):
    m = nn.Module()
    m.block_1, m.attn_1, m.block_2 = ResnetBlock(ch, ch), AttnBlock(ch), ResnetBlock(ch, ch)
    return m


class Encoder(nn.Module):
    """model.py:368-465."""

    def __init__(self, *, ch, out_ch, ch_mult, num_res_blocks, attn_resolutions, in_channels, resolution, z_channels,
                 double_z=True, dropout=0.0, **ignore):
        super().__init__()
        self.num_res_blocks = num_res_blocks
        self.conv_in = nn.Conv2d(in_channels, ch, 3, padding=1)
        in_mult, res = (1,) + tuple(ch_mult), resolution
        self.down = nn.ModuleList()
        for i, mult in enumerate(ch_mult):
            blocks, attn, bin_ = [], [], ch * in_mult[i]
            for _ in range(num_res_blocks):
                blocks.append(ResnetBlock(bin_, ch * mult))
                bin_ = ch * mult
                if res in attn_resolutions:
                    attn.append(AttnBlock(bin_))
            lvl = _level(blocks, attn)
            if i != len(ch_mult) - 1:
                lvl.downsample = Downsample(bin_)
                res //= 2
            self.down.append(lvl)
        self.mid = _mid(bin_)
        self.norm_out = _norm(bin_)
        self.conv_out = nn.Conv2d(bin_, 2 * z_channels if double_z else z_channels, 3, padding=1)


class Decoder(nn.Module):
    """model.py:468-570."""

    def __init__(self, *, ch, out_ch, ch_mult, num_res_blocks, attn_resolutions, in_channels, resolution, z_channels,
                 dropout=0.0, **ignore):
        super().__init__()
        self.num_res_blocks = num_res_blocks
        bin_ = ch * ch_mult[-1]
        res = resolution // 2 ** (len(ch_mult) - 1)
        self.conv_in = nn.Conv2d(z_channels, bin_, 3, padding=1)
        self.mid = _mid(bin_)
        up = []
        for i in reversed(range(len(ch_mult))):
            blocks, attn = [], []
            for _ in range(num_res_blocks + 1):
                blocks.append(ResnetBlock(bin_, ch * ch_mult[i]))
                bin_ = ch * ch_mult[i]
                if res in attn_resolutions:
                    attn.append(AttnBlock(bin_))
            lvl = _level(blocks, attn)
            if i != 0:
                lvl.upsample = Upsample(bin_)
                res *= 2
            up.insert(0, lvl)
        self.up = nn.ModuleList(up)
        self.norm_out = _norm(bin_)
        self.conv_out = nn.Conv2d(bin_, out_ch, 3, padding=1)


class DiagonalGaussian:
    """ldm/modules/distributions/distributions.py:24-62 (mean / logvar / mode / sample)."""

    def __init__(self, moments):
        self.mean, logvar = torch.chunk(moments, 2, dim=1)
        self.logvar = torch.clamp(logvar, -30.0, 20.0)
        self.std = torch.exp(0.5 * self.logvar)

    def mode(self):
        return self.mean

    def sample(self, noise=None, generator=None):
        if noise is None:
            noise = torch.randn(self.mean.shape, device=self.mean.device, generator=generator)
        return self.mean + self.std * noise.to(self.mean.device)


def mosaic_to_tiles(z, n_tiles=13):
    """AutoencoderKL.reshape_z (autoencoder.py:327-336): (B, C, 4h, 4w) -> (B * n_tiles, C, h, w), tiles row-major."""
    b, c, h4, w4 = z.shape
    t = z.reshape(b, c, 4, h4 // 4, 4, w4 // 4).permute(0, 2, 4, 1, 3, 5).reshape(b, 16, c, h4 // 4, w4 // 4)
    return t[:, :n_tiles].reshape(b * n_tiles, c, h4 // 4, w4 // 4)


def tile_condition(z):
    """c_concat of LatentDiffusion.get_input (ddpm.py:800): the input view's latent repeated 4 x 4."""
    return z.repeat(1, 1, 4, 4)


class _FirstStageOps(LdmOps):
    """What the first stage and the condition encoder add to the operator layer: their blocks' packing and forwards."""
    _NOT_EVAL = "call model.eval(): inference only"
    _BAD_PREC = "prec must be 'f32' or 'f16x3'"
    _PRECS = ("f16x3", "f32")

    def _pack_module(self, conv):
        self._pack_conv(conv, conv.weight, conv.bias)

    def _pack_padded(self, conv, cout_pad):
        """conv with its output channels padded with zero rows to cout_pad (so the next layer reads a 16-channel pitch)."""
        w, b = conv.weight, conv.bias
        wp = torch.zeros((cout_pad,) + tuple(w.shape[1:]), dtype=w.dtype, device=w.device)
        bp = torch.zeros((cout_pad,), dtype=w.dtype, device=w.device)
        wp[:w.shape[0]], bp[:w.shape[0]] = w, b
        self._pack_conv((conv, "padded"), wp, bp)

    def _pack_tree(self, root):
        for mod in root.modules():
            if isinstance(mod, ResnetBlock):
                for conv in (mod.conv1, mod.conv2) + ((mod.nin_shortcut,) if hasattr(mod, "nin_shortcut") else ()):
                    self._pack_module(conv)
            elif isinstance(mod, AttnBlock):
                self._pack_conv((mod, "qkv"), torch.cat([mod.q.weight, mod.k.weight, mod.v.weight], 0).contiguous(),
                                torch.cat([mod.q.bias, mod.k.bias, mod.v.bias], 0).contiguous())
                self._pack_module(mod.proj_out)
            elif isinstance(mod, _Resample):
                self._pack_module(mod.conv)

    # -- blocks ----------------------------------------------------------------------------------
    def _resnet(self, blk, x):
        """ResnetBlock.forward (model.py:117-141) with temb None; the shortcut is conv2's residual epilogue."""
        h = self._gn_conv(blk.norm1, blk.conv1, x)
        res = self._conv(blk.nin_shortcut, x) if hasattr(blk, "nin_shortcut") else x
        return self._gn_conv(blk.norm2, blk.conv2, h, residual=res)

    def _attn(self, blk, x):
        """AttnBlock.forward (model.py:181-202): q | k | v as one 1x1 convolution, one wide head, proj_out + residual."""
        n, h, w, c = x.shape
        qkv = self._conv((blk, "qkv"), self._group_norm(blk.norm, x, silu=False))
        att = torch.empty((n, h, w, c), dtype=torch.float32, device=x.device)
        _lib.check(self._lib.s3d_wide_attention_fwd(qkv.data_ptr(), att.data_ptr(), n, h * w, c, self._precv(), self._stream()),
                   "s3d_wide_attention_fwd")
        return self._conv(blk.proj_out, att, residual=x)

    def _downsample(self, ds, x):
        return self._conv_strided(ds.conv, x, (x.shape[1] - 2) // 2 + 1, (x.shape[2] - 2) // 2 + 1, 2, 1)

    def _mid_fwd(self, mid, h):
        return self._resnet(mid.block_2, self._attn(mid.attn_1, self._resnet(mid.block_1, h)))


class AutoencoderKL(_FirstStageOps, nn.Module):
    _NO_LIB = "AutoencoderKL(backend=%r) cannot compute: the HIP library is required; there is no CPU fallback"

    def __init__(self, ddconfig=KL_F8, embed_dim=4, backend="hip", prec="f16x3", fuse_gn=True):
        super().__init__()
        if not ddconfig.get("double_z", True):
            raise ValueError("AutoencoderKL needs double_z (autoencoder.py:301)")
        self.ddconfig, self.embed_dim = dict(ddconfig), embed_dim
        self.encoder = Encoder(**ddconfig)
        self.decoder = Decoder(**ddconfig)
        self.quant_conv = nn.Conv2d(2 * ddconfig["z_channels"], 2 * embed_dim, 1)
        self.post_quant_conv = nn.Conv2d(embed_dim, ddconfig["z_channels"], 1)
        self._init_ops(backend, prec, self._PRECS, fuse_gn)

    def _device(self):
        return self.quant_conv.weight.device

    def repack(self):
        self._require_lib()
        self._check_packable()
        self._packed = {}
        for tree in (self.encoder, self.decoder):
            self._pack_tree(tree)
            self._pack_module(tree.conv_in)
        # layers whose output feeds a convolution with fewer than 16 channels, or the 3-channel image: padded output rows
        self._pack_padded(self.encoder.conv_out, self._pad16(self.encoder.conv_out.weight.shape[0]))
        self._pack_padded(self.quant_conv, self._pad16(self.quant_conv.weight.shape[0]))
        self._pack_padded(self.post_quant_conv, self._pad16(self.post_quant_conv.weight.shape[0]))
        self._pack_padded(self.decoder.conv_out, (self.decoder.conv_out.weight.shape[0] + 3) // 4 * 4)
        self._packed_key = self._params_key()

    def _padded_conv(self, conv, x):
        return self._conv((conv, "padded"), x)

    def _begin(self):
        self._require_lib()
        self._require_eval()
        self._ensure_packed()
        self._pending = None

    @torch.no_grad()
    def encode(self, x):
        """Encoder -> quant_conv -> DiagonalGaussianDistribution of the (N, 3, H, W) images in [-1, 1] (autoencoder.py:319-325,
        one image per batch entry; the reference's 13-image view is the caller's reshape)."""
        self._begin()
        enc = self.encoder
        h = self._conv(enc.conv_in, self._to_nhwc(x, self._pad16(x.shape[1])))
        for lvl in enc.down:
            for i, blk in enumerate(lvl.block):
                h = self._resnet(blk, h)
                if len(lvl.attn):
                    h = self._attn(lvl.attn[i], h)
            if hasattr(lvl, "downsample"):
                h = self._downsample(lvl.downsample, h)
        h = self._mid_fwd(enc.mid, h)
        h = self._padded_conv(enc.conv_out, self._group_norm(enc.norm_out, h, silu=True))
        m = self._padded_conv(self.quant_conv, h)
        return DiagonalGaussian(self._to_nchw(m, 2 * self.embed_dim).contiguous())

    @torch.no_grad()
    def decode(self, z, after_diffusion=True, n_tiles=13):
        """post_quant_conv -> Decoder (autoencoder.py:338-345).  after_diffusion: z is the (B, C, 4h, 4w) mosaic, decoded as
        its first n_tiles tiles (13 in the reference, 12 skip the pad tile) -> (B, 3 n_tiles, 8h, 8w); else z is (N, C, h, w)
        -> (N, 3, 8h, 8w)."""
        self._begin()
        if after_diffusion:
            b = z.shape[0]
            z = mosaic_to_tiles(z.to(self._device(), torch.float32), n_tiles)
        dec = self.decoder
        h = self._padded_conv(self.post_quant_conv, self._to_nhwc(z, self._pad16(z.shape[1])))
        h = self._conv(dec.conv_in, h)
        h = self._mid_fwd(dec.mid, h)
        for lvl in reversed(dec.up):
            for i, blk in enumerate(lvl.block):
                h = self._resnet(blk, h)
                if len(lvl.attn):
                    h = self._attn(lvl.attn[i], h)
            if hasattr(lvl, "upsample"):
                h = self._conv(lvl.upsample.conv, self._resample(h, True))
        h = self._padded_conv(dec.conv_out, self._group_norm(dec.norm_out, h, silu=True))
        out_ch = dec.conv_out.weight.shape[0]
        img = self._to_nchw(h, out_ch)
        if after_diffusion:
            return img.reshape(b, n_tiles * out_ch, img.shape[2], img.shape[3])
        return img.contiguous()


# vgg16bn.features slices of modules.py:231-236 and the trans* projections of :239-243 with their resize targets
_TRANS = (("trans1_2", 64, 192), ("trans2_2", 128, 384), ("trans3_3", 256, 384), ("trans4_3", 512, 768), ("trans5_3", 512, 768))


class ImageEncoderVGG16BN(_FirstStageOps, VGG16BNFeats):
    """modules.py:204-267: VGG16-BN pre-BatchNorm taps conv1_2 ... conv5_3, 1x1 trans* projections, nearest resize to
    16 / 8 / 4 / 2 / 1 and a 4 x 4 repeat -> the U-Net's c_fmaps f1 ... f5."""
    _NO_LIB = "ImageEncoderVGG16BN(backend=%r) cannot compute: the HIP library is required; there is no CPU fallback"

    def __init__(self, backend="hip", prec="f16x3"):
        super().__init__()
        for name, cin, cout in _TRANS:
            setattr(self, name, nn.Conv2d(cin, cout, 1))
        self.register_buffer("mean", torch.tensor([0.485, 0.456, 0.406]).view(1, 3, 1, 1))
        self.register_buffer("std", torch.tensor([0.229, 0.224, 0.225]).view(1, 3, 1, 1))
        self._init_ops(backend, prec, self._PRECS)

    def _device(self):
        return self.trans1_2.weight.device

    def repack(self):
        lib = self._require_lib()
        self._check_packable()
        self._enc_packed = self._pack("s3d_gt_encoder_pack", gt_encoder_params(types.SimpleNamespace(img_encoder=self), data_ptr),
                                      lib.s3d_gt_encoder_packed_bytes())
        self._packed = {}
        for name, _, _ in _TRANS:
            self._pack_module(getattr(self, name))
        self._packed_key = self._params_key()

    @torch.no_grad()
    def forward(self, img):
        lib = self._require_lib()
        self._require_eval()
        self._ensure_packed()
        x = self._f32(img)
        n, ch, s, s2 = x.shape
        if ch != 3 or s != s2 or s % 16:
            raise ValueError("img must be (B, 3, S, S) with S a multiple of 16, got %s" % (tuple(x.shape),))
        xn = torch.empty_like(x)
        _lib.check(lib.s3d_image_normalize_fwd(x.data_ptr(), self.mean.data_ptr(), self.std.data_ptr(), xn.data_ptr(), n, 3, s, s,
                                               self._stream()), "s3d_image_normalize_fwd")
        levels = [torch.empty((n, s >> l, s >> l, c), dtype=torch.float32, device=x.device)
                  for l, c in enumerate((64, 128, 256, 512, 512))]
        pyr = _lib.S3dGtPyramid()
        for l in range(5):
            pyr.level[l] = levels[l].data_ptr()
        pyr.n_img, pyr.size = n, s
        nb = lib.s3d_gt_encoder_workspace_bytes(n, s)
        ws = self._workspace("enc", nb)
        _lib.check(lib.s3d_gt_encode_fwd(self._enc_packed.data_ptr(), xn.data_ptr(), C.byref(pyr), n, s, self._precv(),
                                         ws.data_ptr(), nb, self._stream()), "s3d_gt_encode_fwd")
        out, stride = {}, s // 16     # F.interpolate(size=16 >> l) of an (s >> l)-wide map: every stride-th pixel from 0
        for l, (name, _, _) in enumerate(_TRANS):
            t = self._conv_strided(getattr(self, name), levels[l], 16 >> l, 16 >> l, stride, 0)
            out["f%d" % (l + 1)] = self._to_nchw(t).repeat(1, 1, 4, 4)
        return out

"""gen_slices first stage (AutoencoderKL), condition encoder (ImageEncoderVGG16BN) and the image -> slices pipeline
(SliceDiffusion): host contracts (CPU) and parity of the HIP path against goldens of the REAL reference
(tests/golden/make_golden_ldm_ae.py)."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import GOLDEN

AE_SMALL = dict(double_z=True, z_channels=4, resolution=32, in_channels=3, out_ch=3, ch=32, ch_mult=[1, 2], num_res_blocks=1,
                attn_resolutions=[], dropout=0.0)
PRECS = ["f32", "f16x3"]


def _keys(name):
    return {k: tuple(v) for k, v in json.load(open(os.path.join(GOLDEN, name))).items()}


def _close(out, ref, tol=2e-4):
    out = out.detach().cpu().numpy() if torch.is_tensor(out) else out
    assert out.shape == ref.shape, (out.shape, ref.shape)
    err = float(np.abs(out - ref).max())
    assert err < tol * max(1.0, float(np.abs(ref).max())), err
    return err


# ------------------------------------------------------------------------------------------------------------------ CPU
def test_autoencoder_kl_f8_state_dict_contract():
    from slice3d_amd.ldm_autoencoder import KL_F8, AutoencoderKL
    with torch.device("meta"):
        m = AutoencoderKL(KL_F8, 4, backend="none")
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == _keys("state_dict_keys_ldm_ae_kl8.json")


def test_condition_encoder_state_dict_contract():
    from slice3d_amd.ldm_autoencoder import ImageEncoderVGG16BN
    with torch.device("meta"):
        m = ImageEncoderVGG16BN(backend="none")
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == _keys("state_dict_keys_ldm_cond.json")


def _reference_reshape_z(z):
    """autoencoder.py:327-336, restated."""
    n_bs, n_c, n_h, n_w = z.shape
    z_ = z.view(n_bs, n_c, 4, n_h // 4, 4, n_w // 4).permute(0, 2, 4, 1, 3, 5).reshape(n_bs, 16, n_c, n_h // 4, n_w // 4)
    return z_[:, 0:13].reshape(n_bs * 13, n_c, n_h // 4, n_w // 4)


def test_mosaic_packing_matches_reference():
    from slice3d_amd.ldm_autoencoder import mosaic_to_tiles, tile_condition
    z = torch.randn(2, 4, 12, 20)
    assert torch.equal(mosaic_to_tiles(z), _reference_reshape_z(z))
    assert torch.equal(mosaic_to_tiles(z, 12).view(2, 12, 4, 3, 5), _reference_reshape_z(z).view(2, 13, 4, 3, 5)[:, :12])
    # get_input's mosaic (ddpm.py:761-768): slice tiles X1..X4 | Y1..Y4 | Z1..Z4 | pad, row-major -> tile index i = slice i
    tiles = torch.randn(2, 13, 4, 3, 5)
    rows = [torch.cat([tiles[:, 4 * r + c] for c in range(4)], 3) for r in range(3)]
    mosaic = torch.cat(rows + [torch.zeros_like(rows[0])], 2)
    assert torch.equal(mosaic_to_tiles(mosaic, 12).view(2, 12, 4, 3, 5), tiles[:, :12])
    lat = torch.randn(2, 4, 3, 5)     # c_concat (ddpm.py:800)
    assert torch.equal(tile_condition(lat), lat.repeat(1, 1, 4, 4))


def _synthetic_ldm_state_dict(unet, ae, cond):
    from slice3d_amd.ldm_pipeline import ema_key
    sd = {"scale_factor": torch.tensor(0.5), "betas": torch.zeros(1000), "model_ema.decay": torch.tensor(0.9999)}
    for k, v in unet.state_dict().items():
        sd["model.diffusion_model." + k] = torch.full_like(v, 1.0)
        sd[ema_key(k)] = torch.full_like(v, 2.0)
    sd.update({"first_stage_model." + k: v for k, v in ae.state_dict().items()})
    sd.update({"cond_stage_model." + k: v for k, v in cond.state_dict().items()})
    return sd


@pytest.mark.parametrize("use_ema", [True, False])
def test_from_state_dict_picks_ema_weights(use_ema):
    from slice3d_amd.ldm_autoencoder import AutoencoderKL, ImageEncoderVGG16BN
    from slice3d_amd.ldm_pipeline import SliceDiffusion, ema_key
    from slice3d_amd.ldm_unet import UNetModel
    cfg = dict(image_size=16, in_channels=8, out_channels=4, model_channels=32, attention_resolutions=[2], num_res_blocks=1,
               channel_mult=[1, 2], num_heads=2, use_scale_shift_norm=True, resblock_updown=True)
    unet = UNetModel(backend="none", **cfg)
    ae = AutoencoderKL(AE_SMALL, 4, backend="none")
    cond = ImageEncoderVGG16BN(backend="none")
    ae.encoder.conv_in.weight.data.fill_(3.0)
    cond.trans5_3.bias.data.fill_(4.0)
    sd = _synthetic_ldm_state_dict(unet, ae, cond)
    assert ema_key("input_blocks.0.0.weight") == "model_ema.diffusion_modelinput_blocks00weight"
    m = SliceDiffusion.from_state_dict(sd, use_ema=use_ema, unet_cfg=cfg, ddconfig=AE_SMALL, backend="none")
    want = 2.0 if use_ema else 1.0
    assert all(bool((p == want).all()) for p in m.unet.parameters())
    assert bool((m.first_stage.encoder.conv_in.weight == 3.0).all())
    assert bool((m.cond_stage.trans5_3.bias == 4.0).all())
    assert m.scale_factor == 0.5


# ------------------------------------------------------------------------------------------------------------------ GPU
def _lib_stream():
    from slice3d_amd import _lib
    return _lib, _lib.load(), _lib.stream_ptr(torch.device("cuda"))


@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("n,t", [(1, 256), (3, 144), (2, 1000), (1, 4096)])
def test_wide_attention_matches_fp64(prec, n, t):
    _lib, lib, st = _lib_stream()
    c = 512
    g = torch.Generator().manual_seed(t + n)
    qkv = torch.randn((n, t, 3 * c), generator=g, dtype=torch.float64) * 0.5
    q, k, v = qkv[..., :c], qkv[..., c:2 * c], qkv[..., 2 * c:]
    ref = torch.softmax(q @ k.transpose(1, 2) * c ** -0.5, dim=2) @ v
    x = qkv.float().cuda()
    out = torch.empty((n, t, c), device="cuda")
    _lib.check(lib.s3d_wide_attention_fwd(x.data_ptr(), out.data_ptr(), n, t, c, _lib.PREC[prec], st), "s3d_wide_attention_fwd")
    _close(out, ref.numpy())


@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("hw,cin,cout", [((16, 16), 64, 64), ((15, 9), 32, 48), ((33, 32), 128, 128)])
def test_downsample_conv_matches_torch(prec, hw, cin, cout):
    _lib, lib, st = _lib_stream()
    h, w = hw
    g = torch.Generator().manual_seed(h * w)
    x = torch.randn((2, cin, h, w), generator=g)
    wt = torch.randn((cout, cin, 3, 3), generator=g) * (2.0 / (9 * cin)) ** 0.5
    b = torch.randn((cout,), generator=g) * 0.1
    ref = F.conv2d(F.pad(x.double(), (0, 1, 0, 1)), wt.double(), b.double(), stride=2)
    ho, wo = ref.shape[2], ref.shape[3]
    nb = lib.s3d_conv_packed_bytes(cout, cin, 0, 3)
    packed = torch.empty(nb, dtype=torch.uint8, device="cuda")
    wd, bd = wt.cuda(), b.cuda()
    _lib.check(lib.s3d_conv_pack(wd.data_ptr(), bd.data_ptr(), cout, cin, 0, 3, packed.data_ptr(), nb, st), "s3d_conv_pack")
    xn = x.permute(0, 2, 3, 1).contiguous().cuda()
    out = torch.empty((2, ho, wo, cout), device="cuda")
    _lib.check(lib.s3d_conv_strided_fwd(packed.data_ptr(), xn.data_ptr(), out.data_ptr(), 2, h, w, ho, wo, cout, cin, 3, 2, 1,
                                        _lib.PREC[prec], st), "s3d_conv_strided_fwd")
    _close(out.permute(0, 3, 1, 2), ref.numpy())


def _moments(z):
    m = z["moments"]
    return np.concatenate([m[:, :4], np.clip(m[:, 4:], -30, 20)], 1)


def _ae(ddconfig, prec):
    from slice3d_amd.ldm_autoencoder import AutoencoderKL
    from slice3d_amd.weights import load_seeded
    return load_seeded(AutoencoderKL(ddconfig, 4, prec=prec), 0).cuda().eval()


@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECS)
def test_small_autoencoder_matches_reference(prec):
    """ch 32, ch_mult [1, 2]: encoder moments of one image, decode of a whole 4 x 4 mosaic into its 13 tiles."""
    z = np.load(os.path.join(GOLDEN, "ldm_ae_small.npz"))
    m = _ae(AE_SMALL, prec)
    post = m.encode(torch.from_numpy(z["x"]).cuda())
    _close(torch.cat([post.mean, post.logvar], 1), _moments(z))
    _close(m.decode(torch.from_numpy(z["z"]).cuda()), z["dec"])
    twelve = m.decode(torch.from_numpy(z["z"]).cuda(), n_tiles=12)     # per-image GroupNorm: the pad tile changes nothing
    _close(twelve, z["dec"][:, :36])


@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECS)
def test_kl_f8_autoencoder_matches_reference(prec):
    """kl-f8 at 128^2: encoder moments of one image; decode of one 16 x 16 latent tile, on its own and placed as tile 6
    (mosaic row 1, column 2) of a 4 x 4 mosaic whose other tiles are noise."""
    from slice3d_amd.ldm_autoencoder import KL_F8
    z = np.load(os.path.join(GOLDEN, "ldm_ae_kl8.npz"))
    m = _ae(KL_F8, prec)
    post = m.encode(torch.from_numpy(z["x"]).cuda())
    _close(torch.cat([post.mean, post.logvar], 1), _moments(z))
    tile = torch.from_numpy(z["z"]).cuda()
    _close(m.decode(tile, after_diffusion=False), z["dec"])
    mosaic = torch.randn((1, 4, 64, 64), generator=torch.Generator().manual_seed(5)).cuda()
    mosaic[:, :, 16:32, 32:48] = tile
    _close(m.decode(mosaic, n_tiles=12)[:, 18:21], z["dec"])


@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECS)
def test_condition_encoder_matches_reference(prec):
    from slice3d_amd.ldm_autoencoder import ImageEncoderVGG16BN
    from slice3d_amd.weights import load_seeded
    z = np.load(os.path.join(GOLDEN, "ldm_cond_b1.npz"))
    m = load_seeded(ImageEncoderVGG16BN(prec=prec), 0).cuda().eval()
    f = m(torch.from_numpy(z["img"]).cuda())
    for k in ("f1", "f2", "f3", "f4", "f5"):
        _close(f[k], z[k])


def _input_view(seed):
    """Image 12 of the 13-image stack make_golden_ldm_ae.py drew with this seed."""
    g = torch.Generator().manual_seed(seed)
    return (torch.rand((13, 3, 128, 128), generator=g) * 2 - 1)[12:13].clone()


@pytest.mark.gpu
def test_generate_matches_reference_and_feeds_gt_model():
    """img_ipt_view -> condition -> 2 DDIM steps of the full U-Net -> decode, fed the reference's draws: c_concat and the
    sampled latent mosaic against the reference in full, the decoded slices against the reference's tile Z4 and, in full,
    against the decode of the reference's latent (the decoder itself is pinned by the kl-f8 golden); the result is the
    img_slices input of Slices3DGTModel.encode."""
    from slice3d_amd.ldm_autoencoder import KL_F8, AutoencoderKL, ImageEncoderVGG16BN
    from slice3d_amd.ldm_pipeline import UNET_CFG, SliceDiffusion
    from slice3d_amd.ldm_unet import UNetModel
    from slice3d_amd.models_gt import Slices3DGTModel
    from slice3d_amd.weights import load_seeded
    z = np.load(os.path.join(GOLDEN, "ldm_ae_e2e_b1.npz"))
    unet, ae, cond = (load_seeded(m, 0) for m in (UNetModel(backend="none", **UNET_CFG), AutoencoderKL(KL_F8, 4, backend="none"),
                                                   ImageEncoderVGG16BN(backend="none")))
    sd = {"model.diffusion_model." + k: v for k, v in unet.state_dict().items()}
    sd.update({"first_stage_model." + k: v for k, v in ae.state_dict().items()})
    sd.update({"cond_stage_model." + k: v for k, v in cond.state_dict().items()})
    sd["scale_factor"] = torch.tensor(float(z["scale_factor"]))
    m = SliceDiffusion.from_state_dict(sd, use_ema=False).cuda().eval()
    noises = {"posterior": torch.from_numpy(z["post_noise"]), "x_T": torch.from_numpy(z["x_T"]),
              "steps": [torch.from_numpy(s) for s in z["steps"]]}
    img = _input_view(int(z["meta"][1]))
    c_concat, _ = m.condition(img.cuda(), noises["posterior"])
    _close(c_concat, z["c_concat"])
    out, latent = m.generate(img, ddim_steps=int(z["meta"][0]), noises=noises, return_latent=True)
    assert tuple(out.shape) == (1, 36, 128, 128)
    _close(latent, z["samples"], tol=5e-4)
    err = _close(out[:, 33:36], z["out_z4"], tol=5e-4)
    print("generate(): max |tile Z4 - reference| = %.3e (max |ref| %.2f)" % (err, float(np.abs(z["out_z4"]).max())))
    ref_decode = m.first_stage.decode(torch.from_numpy(z["samples"]).cuda() / m.scale_factor, n_tiles=12)
    _close(out, ref_decode.cpu().numpy(), tol=5e-4)
    gt = load_seeded(Slices3DGTModel(img_size=128, n_slices=12, mode="test"), 0).cuda().eval()
    code = gt.encode({"img_slices": out})
    assert code.batch == 1 and all(bool(torch.isfinite(p).all()) for p in code.pyramid)

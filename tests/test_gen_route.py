"""The generation-based slicing route around the models (slice3d_amd/gen_route.py, gen_slices/*.py,
create_dataset_sin_img.py) against goldens of the REAL reference (tests/golden/make_golden_gen_route.py): test_step mosaics,
the re_org_slices file tree, ObjaverseBase items, the single-image dataset, checkpoint loading.  CPU only."""
import json
import os
import pickle
import sys
import types

import numpy as np
import pytest
import torch
from PIL import Image

import gen_route_cases as cases
from helpers import GOLDEN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AE_SMALL = dict(double_z=True, z_channels=4, resolution=32, in_channels=3, out_ch=3, ch=32, ch_mult=[1, 2], num_res_blocks=1,
                attn_resolutions=[], dropout=0.0)


@pytest.fixture(scope="module")
def golden():
    return json.load(open(os.path.join(GOLDEN, "gen_route.json")))


def _script(rel):
    """Import a repository script as a module (gen_slices/re_org_slices.py, create_dataset_sin_img.py)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location(os.path.basename(rel)[:-3] + "_under_test", os.path.join(ROOT, rel))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _toy_tree(tmp, trailing_newline):
    from slice3d_amd.datasets import write_toy_dataset
    base = write_toy_dataset(os.path.join(tmp, "data"), "objaverse", shapes=cases.TOY_SHAPES, n_views=12, size=40, n_pts=16, seed=7)
    cases.write_trainval(base, cases.TOY_SHAPES, trailing_newline)
    return base


# ------------------------------------------------------------------------------------------------------------ mosaics
def test_sample_slices_pngs_match_reference_test_step(tmp_path, golden):
    """LatentDiffusion.test_step's files: {batch}_{case}.png mosaics (values at exactly +-1, beyond, and on and around every
    truncation boundary) and {batch}_{case}_ipt.png, with a short last batch."""
    from slice3d_amd import gen_route
    nbs = golden["meta"]["ldm_batches"]
    samples = [cases.sample_tensor(nb, 39, seed=b) for b, nb in enumerate(nbs)]
    items = [{"img_ipt_view": v.numpy()} for b, nb in enumerate(nbs) for v in cases.input_views(nb, seed=b)]
    calls = []

    def generate(views, **kw):       # a stand-in model: generate() returns the 12 slice tiles (the pad tile is not shown)
        calls.append(tuple(views.shape))
        return samples[len(calls) - 1][:, :36]
    n = gen_route.sample_slices(types.SimpleNamespace(generate=generate), items, str(tmp_path), n_bs=nbs[0], log=None)
    assert n == sum(nbs) and calls == [(nb, 3, cases.SIZE, cases.SIZE) for nb in nbs]
    assert cases.tree_digest(str(tmp_path)) == golden["ldm_test_step"]


def test_reconstruct_slices_pngs_match_reference_test_step(tmp_path, golden, monkeypatch):
    from slice3d_amd import gen_route
    nbs = golden["meta"]["ae_batches"]
    recs = [cases.sample_tensor(nb, 39, seed=10 + b) for b, nb in enumerate(nbs)]
    items = [{"image": np.zeros((cases.SIZE, cases.SIZE, 39), np.float32)} for _ in range(sum(nbs))]
    seen = []

    def autoencode(ae, image, generator=None, noise=None):
        seen.append(tuple(image.shape))
        return recs[len(seen) - 1]
    monkeypatch.setattr(gen_route, "autoencode_stacks", autoencode)
    assert gen_route.reconstruct_slices(None, items, str(tmp_path), n_bs=nbs[0], log=None) == sum(nbs)
    assert seen == [(nb, cases.SIZE, cases.SIZE, 39) for nb in nbs]
    assert cases.tree_digest(str(tmp_path)) == golden["ae_test_step"]


def test_mosaic_quantisation_is_fp32_truncation():
    from slice3d_amd.gen_route import slices_to_mosaic_u8
    x = cases.sample_tensor(1, 36, 16, seed=3)
    m = slices_to_mosaic_u8(x).numpy()
    assert m.shape == (1, 64, 64, 3) and m.dtype == np.uint8
    t = x.numpy()[0].reshape(12, 3, 16, 16)
    want = ((np.clip(t, -1, 1) + np.float32(1)) / np.float32(2) * np.float32(255)).astype(np.uint8)
    assert np.array_equal(m[0, 16:32, 48:64], want[7].transpose(1, 2, 0))      # tile 7: row 1, column 3
    assert (m[0, 48:] == 127).all()                                            # the zero pad row
    edge = torch.tensor([-2.0, -1.0, 1.0, 3.0, float(np.nextafter(np.float32(-1 + 2 / 255), np.float32(-2)))])
    q = slices_to_mosaic_u8(edge.view(5, 1, 1, 1).repeat(1, 36, 1, 1)).numpy()[:, 0, 0, 0]
    assert q.tolist() == [0, 0, 255, 255, 0]


# ------------------------------------------------------------------------------------------------------------ re_org
@pytest.mark.parametrize("type_slices,n_bs", [("gen", 2), ("rec", 8)])
def test_re_org_tree_matches_reference(tmp_path, golden, type_slices, n_bs):
    base = _toy_tree(str(tmp_path), trailing_newline=False)
    n = len(cases.TOY_SHAPES) * (12 if type_slices == "rec" else 1)
    mos = tmp_path / "mosaics"
    mos.mkdir()
    for i in range(n):
        Image.fromarray(cases.mosaic_u8(i)).save(str(mos / ("%d_%d.png" % (i // n_bs, i % n_bs))))
    _script("gen_slices/re_org_slices.py").main(["--dir_slices", str(mos), "--type_slices", type_slices, "--name_dataset",
                                                 "objaverse", "--n_bs", str(n_bs), "--dir_data", os.path.dirname(base)])
    sub = "04_img_slices_gen" if type_slices == "gen" else "05_img_slices_rec"
    want = golden["re_org_gen_nl" if type_slices == "gen" else "re_org_rec_nonl"]
    assert cases.tree_digest(os.path.join(base, sub)) == want


def test_re_org_pairs_by_dataset_indexing_when_trainval_ends_with_newline(tmp_path, golden):
    """The documented divergence (gen_slices/re_org_slices.py): with a trailing newline the reference's split('\\n') pairs
    every view after the first with the wrong object; here the tree is the one the file without the newline gives."""
    from slice3d_amd.gen_route import mosaic_to_slice_files
    base = _toy_tree(str(tmp_path), trailing_newline=True)
    mos = tmp_path / "mosaics"
    mos.mkdir()
    for i in range(36):
        Image.fromarray(cases.mosaic_u8(i)).save(str(mos / ("%d_%d.png" % (i // 8, i % 8))))
    assert mosaic_to_slice_files(str(mos), base, "rec", n_bs=8) == 36
    got = cases.tree_digest(os.path.join(base, "05_img_slices_rec"))
    assert got == golden["re_org_rec_nonl"]
    assert got != golden["re_org_rec_nl"] and "000/X_1.png" in golden["re_org_rec_nl"]   # the reference's shifted tree


def test_re_org_rec_keeps_existing_files(tmp_path):
    from slice3d_amd.gen_route import mosaic_to_slice_files
    base = _toy_tree(str(tmp_path), trailing_newline=False)
    mos = tmp_path / "m"
    mos.mkdir()
    Image.fromarray(cases.mosaic_u8(0)).save(str(mos / "0_0.png"))
    d = os.path.join(base, "05_img_slices_rec", cases.TOY_SHAPES[0], "000")
    os.makedirs(d)
    Image.new("RGB", (4, 4)).save(os.path.join(d, "Z_4.png"))
    assert mosaic_to_slice_files(str(mos), base, "rec") == 1
    assert Image.open(os.path.join(d, "Z_4.png")).size == (4, 4) and len(os.listdir(d)) == 12


def test_gen_slices_to_model_input_equals_the_file_route(tmp_path):
    """mosaic -> re_org -> Slice3DDataset(from_which_slices='gen') gives the same img_slices bits as the in-memory route;
    with_slices=False gives every other entry unchanged."""
    from slice3d_amd.datasets import Slice3DDataset
    from slice3d_amd.gen_route import gen_slices_to_model_input, mosaic_to_slice_files, slices_to_mosaic_u8
    base = _toy_tree(str(tmp_path), trailing_newline=False)
    mosaic = slices_to_mosaic_u8(cases.sample_tensor(len(cases.TOY_SHAPES), 36, seed=5))
    mos = tmp_path / "m"
    mos.mkdir()
    for i, m in enumerate(mosaic.numpy()):
        Image.fromarray(m).save(str(mos / ("%d_%d.png" % (i // 8, i % 8))))
    mosaic_to_slice_files(str(mos), base, "gen")
    args = types.SimpleNamespace(n_qry=8, dir_data=os.path.dirname(base), name_dataset="objaverse", img_size=cases.SIZE,
                                 from_which_slices="gen", use_white_bg=False, n_views=12)
    ds, lean = Slice3DDataset("test", args), Slice3DDataset("test", args, with_slices=False)
    mem = gen_slices_to_model_input(mosaic)
    assert mem.dtype == torch.float32 and tuple(mem.shape) == (3, 36, cases.SIZE, cases.SIZE)
    for i in range(len(ds)):
        full, part = ds[i], lean[i]
        assert torch.equal(full["img_slices"], mem[i])
        assert set(full) - set(part) == {"img_slices"} and all(torch.equal(full[k], part[k]) for k in part)


# ------------------------------------------------------------------------------------------------------------ dataset
@pytest.mark.parametrize("split", ["test", "trainval_rec"])
def test_objaverse_dataset_matches_reference(tmp_path, golden, split):
    from slice3d_amd.gen_route import ObjaverseLdmDataset
    base = _toy_tree(str(tmp_path), trailing_newline=True)
    ds = ObjaverseLdmDataset(base, split, size=cases.SIZE, with_slices=True)
    want = golden["objaverse_base"][split]
    assert len(ds) == len(want) == len(cases.TOY_SHAPES) * (12 if split == "trainval_rec" else 1)
    for i, w in enumerate(want):
        it = ds[i]
        assert it["file_path_"] == w["file_path_"]
        assert cases.array_sha(it["image"]) == w["image"] and cases.array_sha(it["img_ipt_view"]) == w["img_ipt_view"]
    lean = ObjaverseLdmDataset(base, split, size=cases.SIZE)      # 'test' reads only the input view by default
    assert ("image" in lean[0]) == (split == "trainval_rec")


def test_objaverse_test_split_needs_only_the_input_view(tmp_path):
    import shutil
    from slice3d_amd.gen_route import ObjaverseLdmDataset
    base = _toy_tree(str(tmp_path), trailing_newline=False)
    shutil.rmtree(os.path.join(base, "01_img_slices"))
    it = ObjaverseLdmDataset(base, "test")[0]
    assert it["view"] == 4 and it["img_ipt_view"].shape == (128, 128, 3)


def test_png_2_whitebg_replaces_only_zero_alpha():
    from slice3d_amd.gen_route import png_2_whitebg
    a = np.array([[[10, 20, 30, 0], [10, 20, 30, 1], [10, 20, 30, 255]]], np.uint8)
    assert np.asarray(png_2_whitebg(Image.fromarray(a, "RGBA"))).tolist() == [[[255, 255, 255], [10, 20, 30], [10, 20, 30]]]


# ------------------------------------------------------------------------------------------------------------ single image
def test_create_dataset_sin_img_matches_reference(tmp_path, golden):
    img_path = str(tmp_path / "input.png")
    cases.rgba_object().save(img_path)
    mod = _script("create_dataset_sin_img.py")
    base = mod.create_dataset(mod.get_parser().parse_args(["--img_path", img_path, "--img_size", "64", "--dir_data",
                                                           str(tmp_path / "data")]))
    want = golden["create_dataset_sin_img"]
    assert cases.tree_digest(base) == want["tree"]
    meta = pickle.load(open(os.path.join(base, "00_img_input", "00000", "meta.pkl"), "rb"))
    assert [type(m).__name__ for m in meta] == want["meta_types"]
    assert [cases.array_sha(np.asarray(m)) if not isinstance(m, float) else m for m in meta] == want["meta"]
    for split in ("train", "val", "test"):
        assert open(os.path.join(base, "03_splits", split + ".lst")).read() == "00000"


# ------------------------------------------------------------------------------------------------------------ checkpoints
def _ae_sd():
    from slice3d_amd.ldm_autoencoder import AutoencoderKL
    from slice3d_amd.weights import load_seeded
    return load_seeded(AutoencoderKL(AE_SMALL, 4, backend="none"), 1).state_dict()


def test_autoencoder_checkpoint_drops_only_loss_keys(tmp_path):
    from slice3d_amd.gen_route import load_autoencoder_checkpoint
    sd = dict(_ae_sd())
    sd.update({"loss.logvar": torch.zeros(()), "loss.discriminator.main.0.weight": torch.ones(4, 3, 4, 4),
               "loss.perceptual_loss.net.slice1.0.weight": torch.ones(2)})
    path = str(tmp_path / "ae.ckpt")
    torch.save({"state_dict": sd, "epoch": 3}, path)
    ae = load_autoencoder_checkpoint(path, backend="none", ddconfig=AE_SMALL)
    assert torch.equal(ae.encoder.conv_in.weight, sd["encoder.conv_in.weight"])
    for extra in ({"lossy.x": torch.zeros(1)}, {"encoder.extra": torch.zeros(1)}):
        torch.save({"state_dict": dict(sd, **extra)}, path)
        with pytest.raises(RuntimeError, match="Unexpected key"):
            load_autoencoder_checkpoint(path, backend="none", ddconfig=AE_SMALL)
    missing = dict(sd)
    del missing["decoder.conv_out.bias"]
    torch.save({"state_dict": missing}, path)
    with pytest.raises(RuntimeError, match="Missing key"):
        load_autoencoder_checkpoint(path, backend="none", ddconfig=AE_SMALL)


@pytest.mark.parametrize("use_ema", [True, False])
def test_ldm_checkpoint_loads_ema_weights_by_default(tmp_path, use_ema):
    from slice3d_amd.gen_route import load_ldm_checkpoint
    from slice3d_amd.ldm_autoencoder import AutoencoderKL, ImageEncoderVGG16BN
    from slice3d_amd.ldm_pipeline import ema_key
    from slice3d_amd.ldm_unet import UNetModel
    cfg = dict(image_size=16, in_channels=8, out_channels=4, model_channels=32, attention_resolutions=[2], num_res_blocks=1,
               channel_mult=[1, 2], num_heads=2, use_scale_shift_norm=True, resblock_updown=True)
    unet = UNetModel(backend="none", **cfg)
    sd = {"scale_factor": torch.tensor(0.25)}
    for k, v in unet.state_dict().items():
        sd["model.diffusion_model." + k] = torch.full_like(v, 1.0)
        sd[ema_key(k)] = torch.full_like(v, 2.0)
    sd.update({"first_stage_model." + k: v for k, v in AutoencoderKL(AE_SMALL, 4, backend="none").state_dict().items()})
    sd.update({"cond_stage_model." + k: v for k, v in ImageEncoderVGG16BN(backend="none").state_dict().items()})
    path = str(tmp_path / "ldm.ckpt")
    torch.save({"state_dict": sd, "global_step": 7}, path)
    kw = dict(unet_cfg=cfg, ddconfig=AE_SMALL, backend="none")
    m = load_ldm_checkpoint(path, **kw) if use_ema else load_ldm_checkpoint(path, use_ema=False, **kw)
    assert all(bool((p == (2.0 if use_ema else 1.0)).all()) for p in m.unet.parameters()) and m.scale_factor == 0.25


def test_reconstruct_flags_default_to_the_file_route():
    sys.path.insert(0, os.path.join(ROOT, "reg_slices"))
    from options import get_parser
    a = get_parser().parse_args([])
    assert a.gen_ckpt == "" and a.ddim_steps == 200 and a.gen_seed == 0

"""The generation-based slicing route on the GPU (slice3d_amd/gen_route.py): the file route (sample_slices -> re_org ->
Slice3DDataset) against the in-memory route into the GT model, the reference's batch of 8 through generate() and through
the autoencoder's 13-tile pass, and the entry scripts as fresh processes.  Full U-Net, kl-f8 and condition encoder with
name-seeded weights, 2 DDIM steps, caller-supplied noise."""
import glob
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch
from PIL import Image

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = 2


@pytest.fixture(scope="module")
def diffusion():
    from slice3d_amd.gen_route import synthetic_slice_diffusion
    return synthetic_slice_diffusion(0).cuda().eval()


def _noises(seed, n):
    g = torch.Generator().manual_seed(1000 + seed)
    return {"posterior": torch.randn((n, 4, 16, 16), generator=g), "x_T": torch.randn((n, 4, 64, 64), generator=g),
            "steps": [torch.randn((n, 4, 64, 64), generator=g) for _ in range(STEPS)]}


def _pick(noises, j):
    return {"posterior": noises["posterior"][j:j + 1], "x_T": noises["x_T"][j:j + 1], "steps": [s[j:j + 1] for s in noises["steps"]]}


def _toy(tmp, shapes=("obj_a", "obj_b")):
    from slice3d_amd.datasets import write_toy_dataset
    return write_toy_dataset(os.path.join(tmp, "data"), "objaverse", shapes=shapes, n_views=12, size=40, n_pts=400, seed=11)


def test_file_route_and_in_memory_route_give_the_gt_model_the_same_bits(tmp_path, diffusion):
    from slice3d_amd import gen_route
    from slice3d_amd.datasets import Slice3DDataset
    from slice3d_amd.models_gt import Slices3DGTModel
    from slice3d_amd.weights import load_seeded
    base = _toy(str(tmp_path))
    ds = gen_route.ObjaverseLdmDataset(base, "test")
    out = str(tmp_path / "images_testing_sampled")
    assert gen_route.sample_slices(diffusion, ds, out, n_bs=2, ddim_steps=STEPS, noises=_noises, log=None) == 2
    # in memory: the same views and draws
    views = torch.from_numpy(np.stack([ds[i]["img_ipt_view"] for i in range(2)])).permute(0, 3, 1, 2).contiguous()
    slices = diffusion.generate(views, ddim_steps=STEPS, noises=_noises(0, 2))
    assert bool(torch.isfinite(slices).all())
    mosaic = gen_route.slices_to_mosaic_u8(slices)
    assert mosaic.is_cuda
    for c in range(2):
        assert np.array_equal(np.asarray(Image.open(os.path.join(out, "0_%d.png" % c))), mosaic[c].cpu().numpy())
        assert np.array_equal(np.asarray(Image.open(os.path.join(out, "0_%d_ipt.png" % c))),
                              gen_route.input_view_u8(ds[c]["img_ipt_view"]))
    mem = gen_route.gen_slices_to_model_input(mosaic)
    # file route: re_org -> Slice3DDataset(from_which_slices='gen')
    assert gen_route.mosaic_to_slice_files(out, base, "gen", n_bs=2) == 2
    args = types.SimpleNamespace(n_qry=300, dir_data=os.path.dirname(base), name_dataset="objaverse", img_size=128,
                                 from_which_slices="gen", use_white_bg=False, n_views=12)
    fds = Slice3DDataset("test", args)
    files = torch.stack([fds[i]["img_slices"] for i in range(2)]).cuda()
    assert torch.equal(files, mem)
    gt = load_seeded(Slices3DGTModel(img_size=128, n_slices=12, mode="test"), 0).cuda().eval()
    items = [fds[i] for i in range(2)]
    feed = {k: torch.stack([it[k] for it in items]).cuda() for k in items[0] if k != "img_slices"}
    with torch.no_grad():
        sdf_file = gt(dict(feed, img_slices=files))["sdf_pred"]
        sdf_mem = gt(dict(feed, img_slices=mem))["sdf_pred"]
    assert bool(torch.isfinite(sdf_mem).all()) and torch.equal(sdf_file, sdf_mem)


def test_generate_batch_of_8_matches_per_object_runs(diffusion):
    g = torch.Generator().manual_seed(8)
    views = torch.rand((8, 3, 128, 128), generator=g) * 2 - 1
    noises = _noises(8, 8)
    out8 = diffusion.generate(views, ddim_steps=STEPS, noises=noises)
    assert tuple(out8.shape) == (8, 36, 128, 128) and bool(torch.isfinite(out8).all())
    for j in range(8):
        one = diffusion.generate(views[j:j + 1], ddim_steps=STEPS, noises=_pick(noises, j))
        err = float((out8[j:j + 1] - one).abs().max())
        assert err < 1e-4 * max(1.0, float(one.abs().max())), (j, err)


def test_autoencoder_pass_over_8_x_13_tiles_matches_per_object(diffusion):
    from slice3d_amd.gen_route import autoencode_stacks
    ae = diffusion.first_stage
    g = torch.Generator().manual_seed(13)
    image = torch.rand((8, 128, 128, 39), generator=g) * 2 - 1
    noise = torch.randn((8 * 13, 4, 16, 16), generator=g)
    rec = autoencode_stacks(ae, image, noise=noise)
    assert tuple(rec.shape) == (8, 39, 128, 128) and bool(torch.isfinite(rec).all())
    for j in range(8):
        x = image[j].permute(2, 0, 1).reshape(13, 3, 128, 128).cuda()
        one = ae.decode(ae.encode(x).sample(noise[13 * j:13 * (j + 1)]), after_diffusion=False).reshape(1, 39, 128, 128)
        err = float((rec[j:j + 1] - one).abs().max())
        assert err < 1e-4 * max(1.0, float(one.abs().max())), (j, err)


def _run(cmd, cwd, timeout=900):
    r = subprocess.run([sys.executable] + cmd, cwd=cwd, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout


COMMON = ["--name_dataset", "objaverse", "--name_model", "gtslice", "--from_which_slices", "gen", "--img_size", "128",
          "--n_qry", "256", "--mode", "test", "--mc_res0", "8", "--mc_up_steps", "0", "--name_ckpt", "none.ckpt",
          "--synthetic_weights", "--n_bs", "2"]


def test_reconstruct_in_memory_gen_route_writes_one_mesh_per_object(tmp_path):
    base = _toy(str(tmp_path))
    work = tmp_path / "work"
    work.mkdir()
    out = _run([os.path.join(ROOT, "reg_slices", "reconstruct.py"), "--dir_data", os.path.dirname(base), "--name_exp", "mem",
                "--gen_ckpt", "missing_ldm.ckpt", "--ddim_steps", str(STEPS)] + COMMON, str(work))
    meshes = sorted(os.path.basename(p) for p in glob.glob(str(work / "experiments" / "mem" / "results" / "objaverse" / "*.obj")))
    assert meshes == ["obj_a.obj", "obj_b.obj"], out
    assert not os.path.exists(os.path.join(base, "04_img_slices_gen"))      # nothing went through files


def test_sample_then_re_org_then_reconstruct_file_route(tmp_path):
    base = _toy(str(tmp_path))
    work = tmp_path / "work"
    work.mkdir()
    ckpt = str(tmp_path / "ldm" / "checkpoints" / "missing.ckpt")
    _run([os.path.join(ROOT, "gen_slices", "sample_slices.py"), "--ckpt", ckpt, "--name_dataset", "objaverse", "--dir_data",
          os.path.dirname(base), "--n_bs", "2", "--ddim_steps", str(STEPS), "--synthetic_weights"], str(work))
    sampled = tmp_path / "ldm" / "images_testing_sampled"
    assert sorted(os.listdir(str(sampled))) == ["0_0.png", "0_0_ipt.png", "0_1.png", "0_1_ipt.png"]
    _run([os.path.join(ROOT, "gen_slices", "re_org_slices.py"), "--dir_slices", str(sampled), "--type_slices", "gen",
          "--name_dataset", "objaverse", "--n_bs", "2", "--dir_data", os.path.dirname(base)], str(work))
    assert len(glob.glob(os.path.join(base, "04_img_slices_gen", "*", "004", "*.png"))) == 24
    out = _run([os.path.join(ROOT, "reg_slices", "reconstruct.py"), "--dir_data", os.path.dirname(base), "--name_exp", "files"]
               + COMMON, str(work))
    assert len(glob.glob(str(work / "experiments" / "files" / "results" / "objaverse" / "*.obj"))) == 2, out

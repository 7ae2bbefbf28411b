"""Goldens of the REAL reference gen_slices route around the models (LatentDiffusion.test_step, AutoencoderKL.test_step,
re_org_slices.crop_slices, ldm/data/objaverse.py ObjaverseBase, create_dataset_sin_img.create_dataset) on formula-generated
inputs (tests/gen_route_cases.py) and toy trees (slice3d_amd.datasets.write_toy_dataset).  The test_step methods run
unbound on a stand-in `self` that supplies the decoded tiles.  Stored: file lists, pixel SHA-256s, array digests.
Authoring container only (the reference is imported with the stubs of make_golden_ldm_ae.py):

    python tests/golden/make_golden_gen_route.py
"""
import contextlib
import json
import os
import pickle
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, HERE, os.path.join(ROOT, "tests")]
import gen_route_cases as cases  # noqa: E402
from make_golden_ldm_ae import _stub, import_reference  # noqa: E402
from oracle.ref_import import REFERENCE_ROOT  # noqa: E402
from slice3d_amd.datasets import write_toy_dataset  # noqa: E402

OUT = os.path.join(HERE, "gen_route.json")
GEN_SLICES = os.path.join(REFERENCE_ROOT, "gen_slices")
LDM_BATCHES = (2, 1)          # batch sizes of the LDM test_step calls (the last batch short)
AE_BATCHES = (2, 1)


@contextlib.contextmanager
def cwd(path):
    old = os.getcwd()
    os.chdir(path)
    try:
        yield
    finally:
        os.chdir(old)


def import_more():
    import_reference()
    tv = sys.modules["torchvision"]
    tv.utils = _stub("torchvision.utils", make_grid=lambda *a, **k: None)
    tv.transforms = _stub("torchvision.transforms", RandomHorizontalFlip=lambda p=0.5: None)
    pl = sys.modules["pytorch_lightning"]
    pl.utilities.distributed = _stub("pytorch_lightning.utilities.distributed", rank_zero_only=lambda f: f)
    from ldm.models.autoencoder import AutoencoderKL
    from ldm.models.diffusion.ddpm import LatentDiffusion
    import PIL.Image
    if not hasattr(PIL.Image, "LINEAR"):     # (an alias of BILINEAR that Pillow 10 removed; objaverse.py's table names it)
        PIL.Image.LINEAR = PIL.Image.BILINEAR
    from ldm.data.objaverse import ObjaverseBase
    sys.path.insert(0, GEN_SLICES)
    import re_org_slices
    sys.path.insert(0, REFERENCE_ROOT)
    import create_dataset_sin_img
    return LatentDiffusion, AutoencoderKL, ObjaverseBase, re_org_slices, create_dataset_sin_img


def ldm_test_step(LatentDiffusion, tmp):
    out = {}
    for b, nb in enumerate(LDM_BATCHES):
        samples = cases.sample_tensor(nb, 39, seed=b)
        me = types.SimpleNamespace(ckpt_path=os.path.join(tmp, "ldm", "checkpoints", "last.ckpt"),
                                   log_images_when_testing=lambda batch, s=samples: {"samples": s})
        LatentDiffusion.test_step(me, {"img_ipt_view": cases.input_views(nb, seed=b)}, b)
    return cases.tree_digest(os.path.join(tmp, "ldm", "images_testing_sampled"))


def ae_test_step(AutoencoderKL, tmp):
    class Me:
        image_key = "image"
        ckpt_path = os.path.join(tmp, "ae", "checkpoints", "model.ckpt")
        get_input = AutoencoderKL.get_input
        log_dict = None

        def __call__(self, inputs):
            return self.rec, None
    me = Me()
    for b, nb in enumerate(AE_BATCHES):
        me.rec = cases.sample_tensor(nb, 39, seed=10 + b)
        AutoencoderKL.test_step(me, {"image": torch.zeros((nb, cases.SIZE, cases.SIZE, 39))}, b)
    return cases.tree_digest(os.path.join(tmp, "ae", "images_reconstructed"))


def toy_tree(tmp, trailing_newline=False):
    base = write_toy_dataset(os.path.join(tmp, "data"), "objaverse", shapes=cases.TOY_SHAPES, n_views=12, size=40, n_pts=16, seed=7)
    cases.write_trainval(base, cases.TOY_SHAPES, trailing_newline)
    os.makedirs(os.path.join(tmp, "work"), exist_ok=True)
    return base


def re_org(re_org_slices, tmp, type_slices, trailing_newline, n_bs):
    base = toy_tree(tmp, trailing_newline)
    n = len(cases.TOY_SHAPES) * (12 if type_slices == "rec" else 1)
    mos = os.path.join(tmp, "mosaics")
    os.makedirs(mos, exist_ok=True)
    from PIL import Image
    for i in range(n):
        Image.fromarray(cases.mosaic_u8(i)).save(os.path.join(mos, "%d_%d.png" % (i // n_bs, i % n_bs)))
    args = types.SimpleNamespace(dir_slices=mos, type_slices=type_slices, name_dataset="objaverse", img_size=cases.SIZE,
                                 n_bs=n_bs, n_views=12)
    with cwd(os.path.join(tmp, "work")):
        re_org_slices.crop_slices(args)
    sub = "04_img_slices_gen" if type_slices == "gen" else "05_img_slices_rec"
    return cases.tree_digest(os.path.join(base, sub))


def objaverse_items(ObjaverseBase, tmp):
    base = toy_tree(tmp, trailing_newline=True)
    out = {}
    for split, lst in (("test", "test"), ("trainval_rec", "trainval")):
        ds = ObjaverseBase(os.path.join(base, "03_splits", lst + ".lst"), base, split, size=cases.SIZE)
        out[split] = [{"file_path_": it["file_path_"], "image": cases.array_sha(it["image"]),
                       "img_ipt_view": cases.array_sha(it["img_ipt_view"])} for it in (ds[i] for i in range(len(ds)))]
    return out


def sin_img(create_dataset_sin_img, tmp):
    img_path = os.path.join(tmp, "input.png")
    cases.rgba_object().save(img_path)
    args = types.SimpleNamespace(img_path=img_path, name_dataset="custom_sin_img", img_size=64, resize_img=False, center_obj=True)
    with cwd(tmp):
        create_dataset_sin_img.create_dataset(args)
    base = os.path.join(tmp, "data", "custom_sin_img")
    meta = pickle.load(open(os.path.join(base, "00_img_input", "00000", "meta.pkl"), "rb"))
    return {"tree": cases.tree_digest(base),
            "meta": [cases.array_sha(np.asarray(m)) if not isinstance(m, float) else m for m in meta],
            "meta_types": [type(m).__name__ for m in meta]}


def main():
    LatentDiffusion, AutoencoderKL, ObjaverseBase, re_org_slices, sin = import_more()
    g = {}
    with tempfile.TemporaryDirectory() as t:
        g["ldm_test_step"] = ldm_test_step(LatentDiffusion, t)
    with tempfile.TemporaryDirectory() as t:
        g["ae_test_step"] = ae_test_step(AutoencoderKL, t)
    for type_slices, nl, n_bs in (("gen", True, 2), ("rec", False, 8), ("rec", True, 8)):
        with tempfile.TemporaryDirectory() as t:
            g["re_org_%s_%s" % (type_slices, "nl" if nl else "nonl")] = re_org(re_org_slices, t, type_slices, nl, n_bs)
    with tempfile.TemporaryDirectory() as t:
        g["objaverse_base"] = objaverse_items(ObjaverseBase, t)
    with tempfile.TemporaryDirectory() as t:
        g["create_dataset_sin_img"] = sin_img(sin, t)
    g["meta"] = {"ldm_batches": LDM_BATCHES, "ae_batches": AE_BATCHES}
    with open(OUT, "w") as f:
        json.dump(g, f, indent=0, sort_keys=True)
    print(OUT, os.path.getsize(OUT), "bytes;", {k: len(v) for k, v in g.items()})


if __name__ == "__main__":
    main()

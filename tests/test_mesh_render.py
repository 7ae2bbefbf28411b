"""Preconditions of the mesh-render tests, checked without a GPU and with the float64 reference alone
(tests/render_ref.py on the cases of tests/render_cases.py): few samples sit where two correct evaluations may differ,
every slab shows something, the slabs partition the view exactly, the images agree with the projection of the
vertices; and the host-side pieces of slice3d_amd/mesh_render.py: make_meta's format, write_shape's tree as
Slice3DDataset reads it, the header and the binding."""
import os
import pickle
import subprocess
import sys
import types

import numpy as np
import pytest

import render_cases
import render_ref
from render_cases import BASE, CASES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", CASES)
def test_few_samples_are_flagged_and_every_slab_shows_something(name):
    ref = render_cases.reference(name)
    share = render_cases.flagged(ref).mean()
    print("%s: edge %d, slab %d, tie %d samples; flagged share %.5f" % (name, ref["edge"].sum(), ref["slab"].sum(),
                                                                       ref["tie"].sum(), share))
    assert share <= render_cases.FLAG_CAP
    cov = ref["face"] >= 0
    assert cov.reshape(13, -1).any(axis=1).all()
    assert np.array_equal(cov, np.isfinite(ref["depth"]))


@pytest.mark.parametrize("name", CASES + ["axis", "scale5_inside"])
def test_slabs_partition_the_view_exactly(name):
    ref = render_cases.reference(name)
    cov, depth = ref["face"] >= 0, ref["depth"]
    for ax in range(3):
        sl = slice(1 + 4 * ax, 5 + 4 * ax)
        assert np.array_equal(cov[sl].any(axis=0), cov[0])
        assert np.array_equal(depth[sl].min(axis=0), depth[0])
        # the image that attains the view's depth shows the view's face
        k = depth[sl].argmin(axis=0)
        assert np.array_equal(np.take_along_axis(ref["face"][sl], k[None], 0)[0], ref["face"][0])


@pytest.mark.parametrize("name", CASES)
def test_projected_vertices_lie_inside_the_covered_pixel_range(name):
    """The pinhole of the images is the projection the models sample with: [c, 1] @ T of datasets.camera_matrices after
    the divide equals (f p_x / p_z + 0.5, f p_y / p_z + 0.5) to float32 accuracy, and the referenced vertices project into the bounding box
    of the covered pixels (a vertex is a point of the surface: the pixels around it see the object, up to one pixel)."""
    from slice3d_amd.datasets import camera_matrices
    ref = render_cases.reference(name)
    v, f = render_cases.mesh(name)
    c = ref["c"][np.unique(f)]
    uv = render_ref.project(c, BASE["distance"])
    _, T = camera_matrices(-BASE["az"], BASE["el"], BASE["distance"])
    h = np.concatenate([c, np.ones((len(c), 1))], axis=1) @ T
    # the chain's camera rotation carries a float32 pi (entries of 4.37e-8 in datasets._CAM_ROT), which leaves up to
    # 4.37e-8 * distance in T's translation: f / p_z times that on the image, and twice the bound is asked here
    gate = 2 * 4.371138828673793e-08 * BASE["distance"] * render_ref.FOCAL / (c[:, 2] + BASE["distance"]).min()
    assert np.abs(h[:, :2] / h[:, 2:3] - uv).max() <= gate
    ys, xs = np.nonzero(ref["rgba"][0, :, :, 3] > 0)                    # covered pixels
    px = uv * BASE["size"]
    assert px[:, 0].min() >= xs.min() - 1 and px[:, 0].max() <= xs.max() + 2
    assert px[:, 1].min() >= ys.min() - 1 and px[:, 1].max() <= ys.max() + 2


def test_slab_names_follow_image_directions():
    """Camera-aligned: X_k left to right, Y_k top to bottom, Z_k near to far."""
    ref = render_cases.reference("sphere")
    cov = ref["face"] >= 0
    cx = [np.nonzero(cov[1 + k])[1].mean() for k in range(4)]
    cy = [np.nonzero(cov[5 + k])[0].mean() for k in range(4)]
    dz = [ref["depth"][9 + k][cov[9 + k]].mean() for k in range(4)]
    assert cx == sorted(cx) and cy == sorted(cy) and dz == sorted(dz)


def test_reference_image_values():
    ref = render_cases.reference("flat")
    rgba, cov = ref["rgba"], ref["face"] >= 0
    S, size = BASE["S"], BASE["size"]
    cnt = cov.reshape(13, size, S, size, S).sum(axis=(2, 4))
    assert np.array_equal(rgba[..., 3], np.rint(255.0 * cnt / (S * S)).astype(np.uint8))
    assert (rgba[cnt == 0] == 0).all()
    # 0.8 grey times a shade in [0.5, 1]
    lit = rgba[cnt > 0][:, :3]
    assert lit.min() >= 102 and lit.max() <= 204 and (lit[:, 0] == lit[:, 1]).all() and (lit[:, 1] == lit[:, 2]).all()


def test_make_meta_format():
    from slice3d_amd.datasets import blender_proj
    from slice3d_amd.mesh_render import IMAGE_NAMES, make_meta
    assert IMAGE_NAMES == render_ref.NAMES and len(IMAGE_NAMES) == 13
    m = make_meta(6, 3, size=64)
    assert isinstance(m, list) and len(m) == 7
    K, az, el, dist, poses, scale, offset = m
    assert K.dtype == np.float32 and np.array_equal(K, np.array([[70, 0, 32], [0, 70, 32], [0, 0, 1]], np.float32))
    assert az.dtype == np.float32 and np.array_equal(az, (np.arange(6) / 6 * np.pi * 2).astype(np.float32))
    assert el.shape == (6,) and (el >= np.deg2rad(-10)).all() and (el <= np.deg2rad(40)).all()
    assert np.array_equal(dist, np.full(6, 1.2)) and poses.shape == (6, 3, 4)
    assert np.array_equal(poses[2], blender_proj(-float(az[2]), float(el[2]), 1.2)[1])
    assert isinstance(scale, float) and 0.75 <= scale < 1.1 and np.array_equal(offset, np.zeros(3))
    m2, m3 = make_meta(6, 3, size=64), make_meta(6, 4, size=64)
    assert np.array_equal(m2[2], el) and m2[5] == scale and not np.array_equal(m3[2], el)
    assert "never reads" in make_meta.__doc__
    pickle.loads(pickle.dumps(m))


def test_dataset_reads_a_tree_written_from_reference_images(tmp_path):
    from PIL import Image
    from slice3d_amd.datasets import Slice3DDataset
    from slice3d_amd.mesh_render import IMAGE_NAMES, make_meta, write_shape
    v, f = render_cases.mesh("flat")
    size, S, n_views = 8, 1, 5

    class HostRenderer:                                                # the float64 reference in the renderer's place
        def render(self, az, el, distance, scale=1.0, offset=(0, 0, 0), size=256, samples=4, slice_direction="camera",
                   vertex_colors=None, tile=None):
            return render_ref.render(v, f, float(az), float(el), float(distance), scale, offset, size, samples,
                                     slice_direction)["rgba"]

    base = tmp_path / "custom"
    meta = make_meta(n_views, 1, size=size)
    assert write_shape(HostRenderer(), str(base), "shape_a", meta, size=size, samples=S) == n_views
    kept = dict(meta=pickle.load(open(base / "00_img_input" / "shape_a" / "meta.pkl", "rb")))
    write_shape(HostRenderer(), str(base), "shape_a", make_meta(n_views, 2, size=size), size=size, samples=S)
    again = pickle.load(open(base / "00_img_input" / "shape_a" / "meta.pkl", "rb"))
    assert np.array_equal(again[2], kept["meta"][2]) and again[5] == kept["meta"][5]      # never overwritten
    for view in range(n_views):
        assert np.asarray(Image.open(base / "00_img_input" / "shape_a" / ("%03d.png" % view))).shape == (size, size, 4)
        for name in IMAGE_NAMES[1:]:
            assert (base / "01_img_slices" / "shape_a" / ("%03d" % view) / (name + ".png")).is_file()
    os.makedirs(base / "02_sdfs")
    os.makedirs(base / "03_splits")
    np.save(base / "02_sdfs" / "shape_a.npy", np.zeros((20, 4), dtype=np.float32))
    for split in ("train", "val", "test"):
        (base / "03_splits" / (split + ".lst")).write_text("shape_a\n")
    args = types.SimpleNamespace(n_qry=10, dir_data=str(tmp_path), name_dataset="custom", img_size=16, from_which_slices="gt",
                                 use_white_bg=False, n_views=n_views, categories_train="", categories_test="")
    item = Slice3DDataset("test", args)[0]
    assert tuple(item["img_input"].shape) == (3, 16, 16) and tuple(item["img_slices"].shape) == (36, 16, 16)
    assert tuple(item["qry_norot"].shape) == (10, 3) and tuple(item["obj_rot_mat"].shape) == (3, 3)


def test_gen_dataset_help_parses_and_needs_meshes(tmp_path):
    script = os.path.join(ROOT, "render_slices", "gen_dataset.py")
    r = subprocess.run([sys.executable, script, "--help"], capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert r.returncode == 0, r.stderr
    for flag in ("--dir_meshes", "--name_dataset", "--dir_data", "--n_views", "--img_size", "--samples", "--slice_direction",
                 "--seed", "--normalize", "--write_splits", "--overwrite"):
        assert flag in r.stdout
    r = subprocess.run([sys.executable, script, "--dir_meshes", str(tmp_path), "--name_dataset", "x", "--dir_data",
                        str(tmp_path)], capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert r.returncode == 1 and '"n_shapes": 0' in r.stdout


def test_header_and_binding_declare_the_render_entry_points():
    from slice3d_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "slice3d_hip.h")).read()
    for name in ("s3d_mesh_render_workspace_bytes", "s3d_mesh_render_build", "s3d_mesh_render_fill",
                 "s3d_mesh_render_render"):
        assert name in _lib.SYMBOLS and (name + "(") in hdr
    mk = open(os.path.join(ROOT, "slice3d_amd", "csrc", "Makefile")).read()
    assert "mesh_render.o" in mk and "mesh_render.o: EXTRA += -ffp-contract=off" in mk

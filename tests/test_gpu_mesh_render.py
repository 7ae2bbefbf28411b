"""GPU tests of the mesh renderer (csrc/mesh_render.hip) through slice3d_amd/mesh_render.py and
render_slices/gen_dataset.py: coverage, depth, face and colour against the float64 restatement of tests/render_ref.py on
the cases of tests/render_cases.py, the shapes that break binning, bit-level determinism over runs, tile edges and
mesh homes, the exact slab identities, agreement with the dataset's own projection and signed distances, the
program's behaviour, and the argument checks."""
import ctypes as C
import importlib.util
import json
import os
import pickle
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import render_cases
import render_ref
from render_cases import CASES, VARIANTS

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _render(key, **kw):
    from slice3d_amd.mesh_render import SliceRenderer
    name, cam = render_cases.camera(key)
    v, f = render_cases.mesh(name)
    cam = dict(cam)
    cam["samples"] = cam.pop("S")
    cam.update(kw)
    az, el, distance = cam.pop("az"), cam.pop("el"), cam.pop("distance")
    return SliceRenderer((v, f)).render(az, el, distance, return_samples=True, **cam)


def _compare(key, tile=None):
    """Items 1 and 2: coverage equal on every unflagged sample; |depth - s_A| <= T; the returned face's own reference
    depth within T of the returned depth; alpha equal and rgb within one level on pixels without a flagged sample."""
    name, cam = render_cases.camera(key)
    v, f = render_cases.mesh(name)
    ref = render_cases.reference(key)
    rgba, depth, face = _render(key) if tile is None else _render(key, tile=tile)
    size, S = cam["size"], cam["S"]
    W = size * S
    assert rgba.shape == (13, size, size, 4) and rgba.dtype == np.uint8
    assert depth.shape == (13, W, W) and depth.dtype == np.float64 and face.shape == (13, W, W) and face.dtype == np.int32
    flagged = render_cases.flagged(ref)
    T, t1, t2 = render_cases.tolerance(ref, cam["distance"])
    cov, cov_ref = face >= 0, ref["face"] >= 0
    assert np.array_equal(cov, np.isfinite(depth)) and (face < len(f)).all()
    ok = ~flagged
    n_diff = int((cov != cov_ref)[ok].sum())
    both = cov & cov_ref & ok
    own = render_ref.face_depth(ref["p"], f, face, size, S)
    with np.errstate(invalid="ignore"):                                 # inf - inf on the samples both sides miss
        err = float(np.abs(depth - ref["depth"])[both].max()) if both.any() else 0.0
        err_face = float(np.abs(own - depth)[cov].max()) if cov.any() else 0.0
    px_ok = ~flagged.reshape(13, size, S, size, S).any(axis=(2, 4))
    d_alpha = int((rgba[..., 3] != ref["rgba"][..., 3])[px_ok].sum())
    d_rgb = int(np.abs(rgba[..., :3].astype(int) - ref["rgba"][..., :3].astype(int))[px_ok].max()) if px_ok.any() else 0
    print("%s: %d faces, %d samples, flagged %.5f, coverage differences %d, 16 max|s_A - s_B| = %.3e, floor = %.3e, "
          "T = %.3e, max|depth - s_A| = %.3e, max|s_A(face) - depth| = %.3e, faces that differ %d, alpha differences %d, "
          "max rgb difference %d" % (key, len(f), W * W, flagged.mean(), n_diff, t1, t2, T, err, err_face,
                                     int((face != ref["face"])[ok].sum()), d_alpha, d_rgb))
    assert n_diff == 0
    assert err <= T
    assert err_face <= T
    assert d_alpha == 0 and d_rgb <= 1
    return rgba, depth, face


# ---------------------------------------------------------------------------------------------- 1: reference comparison
@pytest.mark.parametrize("name", CASES)
def test_images_match_the_float64_reference(name):
    _compare(name)


# ---------------------------------------------------------------------------------------------- 2: shapes that break binning
@pytest.mark.parametrize("key", sorted(VARIANTS))
def test_shapes_that_break_binning(key):
    _compare(key)


def test_camera_inside_sends_faces_to_every_tile_and_fills_several_chunks():
    """The conditions the scale cases are there for, read from the renderer's own counters."""
    from slice3d_amd.mesh_render import SliceRenderer
    v, f = render_cases.mesh("sphere")
    for key, behind_expected in (("scale3", False), ("scale5_inside", True)):
        _, cam = render_cases.camera(key)
        ref = render_cases.reference(key)
        behind = int((ref["p"][f][:, :, 2] <= 0).any(axis=1).sum())
        r = SliceRenderer((v, f))
        r.render(cam["az"], cam["el"], cam["distance"], scale=cam["scale"], offset=cam["offset"], size=cam["size"],
                 samples=cam["S"])
        tiles = ((cam["size"] + 8 - 1) // 8) ** 2                     # the default tile edge at S = 2
        print("%s: %d faces with a vertex at p_z <= 0, %d entries in %d tiles" % (key, behind, r.n_entries, tiles))
        assert (behind > 0) == behind_expected
        assert r.n_entries >= tiles * behind and r.n_entries > 128 * tiles   # on average more than one LDS chunk per tile
        W = cam["size"] * cam["S"]
        assert int(r.n_tests) == r.n_entries * (W * W // tiles)


def test_vertex_colors_colour_the_view_only():
    from slice3d_amd.mesh_render import SliceRenderer
    name, cam = render_cases.camera("torus")
    v, f = render_cases.mesh(name)
    col = np.random.default_rng(5).uniform(0, 1, (len(v), 3))
    ref = render_ref.resolve(render_cases.reference("torus")["p"], f, render_cases.reference("torus")["face"], cam["size"],
                             cam["S"], vertex_colors=col)
    got = SliceRenderer((v, f)).render(cam["az"], cam["el"], cam["distance"], scale=cam["scale"], offset=cam["offset"],
                                       size=cam["size"], samples=cam["S"], vertex_colors=col)
    assert np.array_equal(got[..., 3], ref[..., 3])
    assert np.abs(got.astype(int) - ref.astype(int)).max() <= 1
    assert np.array_equal(got[1:], _render("torus")[0][1:])
    assert (got[0, ..., 0] != got[0, ..., 1]).any()


# ---------------------------------------------------------------------------------------------- 3: determinism
def _same(a, b):
    return all(torch.equal(torch.as_tensor(x).cpu().view(torch.uint8), torch.as_tensor(y).cpu().view(torch.uint8))
               for x, y in zip(a, b))


@pytest.mark.parametrize("key", ["boxes", "scale5_inside", "s4", "s1"])
def test_bytes_are_equal_over_runs_tiles_and_mesh_homes(key):
    from slice3d_amd.mesh_render import SliceRenderer
    name, cam = render_cases.camera(key)
    v, f = render_cases.mesh(name)
    first = _render(key)
    assert _same(first, _render(key))
    for tile in range(1, 32 // cam["S"] + 1):                          # every tile edge the library accepts
        assert _same(first, _render(key, tile=tile)), tile
    dev = SliceRenderer((torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda()))
    out = dev.render(cam["az"], cam["el"], cam["distance"], scale=cam["scale"], offset=cam["offset"], size=cam["size"],
                     samples=cam["S"], slice_direction=cam["slice_direction"], return_samples=True)
    assert all(x.is_cuda for x in out) and out[0].dtype == torch.uint8 and out[1].dtype == torch.float64
    assert out[2].dtype == torch.int32 and _same(first, out)
    # workspace memory handed back by the caching allocator holds old bytes; the result must not depend on them
    junk = torch.full((64 << 20,), 0x7f, dtype=torch.uint8, device="cuda")
    del junk
    assert _same(first, _render(key))


def test_lowest_face_index_wins_ties():
    from slice3d_amd.mesh_render import SliceRenderer
    v = np.array([[-1, -1, 0], [1, -1, 0], [-1, 1, 0], [1, 1, 0]], dtype=np.float64) * 0.3
    f = np.array([[1, 2, 3], [0, 1, 2], [1, 2, 3], [0, 1, 2]])         # each face twice
    for tile in (1, 4, 8):
        rgba, depth, face = SliceRenderer((v, f)).render(0.7, 0.3, 1.2, size=16, samples=2, return_samples=True, tile=tile)
        assert set(np.unique(face[0])) == {-1, 0, 1}


# ---------------------------------------------------------------------------------------------- 4: exact invariants
@pytest.mark.parametrize("name", ["torus", "boxes"])
def test_slabs_partition_the_view_exactly_on_the_device(name):
    rgba, depth, face = _render(name, size=64, samples=4)
    cov = face >= 0
    assert cov[0].any()
    for direction in ("camera", "axis"):
        if direction == "axis":
            rgba, depth, face = _render(name, size=64, samples=4, slice_direction="axis")
            cov = face >= 0
        for ax in range(3):
            sl = slice(1 + 4 * ax, 5 + 4 * ax)
            assert np.array_equal(cov[sl].any(axis=0), cov[0])
            assert np.array_equal(depth[sl].min(axis=0), depth[0])
            k = depth[sl].argmin(axis=0)
            assert np.array_equal(np.take_along_axis(face[sl], k[None], 0)[0], face[0])
        alpha = rgba[..., 3].astype(int)
        assert np.array_equal(alpha > 0, cov.reshape(13, 64, 4, 64, 4).any(axis=(2, 4)))


# ---------------------------------------------------------------------------------------------- 5: the dataset
def test_images_agree_with_the_dataset_projection_and_signed_distances(tmp_path):
    """gen_dataset.py + make_sdfs.py on two meshes, read back by Slice3DDataset.  With r = sqrt(2) / size * (distance +
    0.6) / f / scale (a pixel's diagonal at the far end of the object, in the mesh's units): a stored point at signed
    distance <= -r is the centre of a ball inside the object that covers its whole pixel, so the pixel has alpha 255; and
    a stored point whose line of sight passes the bounding sphere of the mesh at more than r cannot see the object: its
    pixel has alpha 0 or lies off the image.  (A point outside the bounding sphere but in front of the object does see it,
    so the condition is on the line of sight, not on the point.)"""
    from PIL import Image
    from slice3d_amd.datasets import Slice3DDataset, camera_matrices
    from slice3d_amd.mesh import Mesh
    from slice3d_amd.mesh_sdf import normalize_mesh
    src = tmp_path / "meshes"
    src.mkdir()
    shapes = {"shape_a": "sphere", "shape_b": "torus"}
    for sh, name in shapes.items():
        v, f = render_cases.mesh(name)
        Mesh(v * 1.7 + 0.2, f).export(str(src / (sh + ".obj")))        # --normalize brings it back
    size, n_views, n_pts = 64, 6, 20000
    common = ["--dir_meshes", str(src), "--name_dataset", "custom", "--dir_data", str(tmp_path), "--normalize"]
    for cmd in ([os.path.join(ROOT, "render_slices", "gen_dataset.py")] + common +
                ["--img_size", str(size), "--samples", "2", "--n_views", str(n_views), "--write_splits"],
                [os.path.join(ROOT, "reg_slices", "make_sdfs.py")] + common + ["--n_points", str(n_pts)]):
        r = subprocess.run([sys.executable] + cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert r.returncode == 0, r.stdout + r.stderr
        assert json.loads(r.stdout.strip().splitlines()[-1])["written"] == 2
    args = types.SimpleNamespace(n_qry=512, dir_data=str(tmp_path), name_dataset="custom", img_size=size,
                                 from_which_slices="gt", use_white_bg=False, n_views=n_views, categories_train="",
                                 categories_test="")
    ds = Slice3DDataset("test", args)
    assert len(ds) == 2
    item = ds[0]
    assert tuple(item["img_input"].shape) == (3, size, size) and tuple(item["img_slices"].shape) == (36, size, size)
    assert tuple(item["qry_norot"].shape) == (512, 3) and tuple(item["sdf"].shape) == (512,)
    assert float(item["img_input"].max()) > -1.0 and float(item["img_slices"].max()) > -1.0
    base = tmp_path / "custom"
    for sh in shapes:
        with open(base / "00_img_input" / sh / "meta.pkl", "rb") as fh:
            meta = pickle.load(fh)
        stored = np.load(base / "02_sdfs" / (sh + ".npy")).astype(np.float64)
        sd = stored[:, 3] - float(np.float32(0.003))
        scale, off = meta[5], meta[6]
        mv = normalize_mesh(render_cases.mesh(shapes[sh])[0] * 1.7 + 0.2)
        centre, radius = np.zeros(3), float(np.linalg.norm(mv, axis=1).max())
        n_in = n_out = 0
        for view in range(n_views):
            d = float(meta[3][view])
            R, T = camera_matrices(-meta[1][view], meta[2][view], d)
            alpha = np.asarray(Image.open(base / "00_img_input" / sh / ("%03d.png" % view)))[:, :, 3]
            r = np.sqrt(2.0) / size * (d + 0.6) / render_ref.FOCAL / scale
            t = np.array([off[0], off[2], -off[1]])
            c = (stored[:, :3] * scale + t) @ R
            h = np.concatenate([c, np.ones((len(c), 1))], axis=1) @ T
            px = np.floor(h[:, :2] / h[:, 2:3] * size).astype(int)
            on = (px >= 0).all(axis=1) & (px < size).all(axis=1)
            inside = sd <= -r
            assert on[inside].all()
            assert (alpha[px[inside, 1], px[inside, 0]] == 255).all()
            # line of sight: from the camera at (0, 0, -d) of the c frame through the point
            cc = (centre * scale + t) @ R + np.array([0, 0, d])
            p = c + np.array([0, 0, d])
            miss = np.linalg.norm(np.cross(p, cc[None]), axis=1) / np.linalg.norm(p, axis=1) > (radius + r) * scale
            seen = miss & on
            assert (alpha[px[seen, 1], px[seen, 0]] == 0).all()
            n_in += int(inside.sum())
            n_out += int(seen.sum())
        print("%s: %d inside points on alpha-255 pixels, %d points past the bounding sphere on alpha-0 pixels" % (sh, n_in, n_out))
        assert n_in > 100 and n_out > 100


# ---------------------------------------------------------------------------------------------- 6: the program
def _gen_dataset():
    spec = importlib.util.spec_from_file_location("gen_dataset", os.path.join(ROOT, "render_slices", "gen_dataset.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _tree_bytes(base):
    out = {}
    for sub in ("00_img_input", "01_img_slices"):
        for d, _, files in os.walk(os.path.join(base, sub)):
            for name in files:
                if name.endswith(".png"):
                    with open(os.path.join(d, name), "rb") as fh:
                        out[os.path.relpath(os.path.join(d, name), base)] = fh.read()
    return out


def test_gen_dataset_skips_overwrites_and_reuses_cameras(tmp_path, capsys):
    from PIL import Image
    from slice3d_amd.mesh import Mesh
    from slice3d_amd.mesh_eval import load_obj
    from slice3d_amd.mesh_render import SliceRenderer, make_meta
    gd = _gen_dataset()
    src = tmp_path / "meshes"
    src.mkdir()
    for sh, name in (("a", "flat"), ("b", "sphere")):
        v, f = render_cases.mesh(name)
        Mesh(v, f).export(str(src / (sh + ".obj")))
    common = ["--dir_meshes", str(src), "--dir_data", str(tmp_path), "--img_size", "16", "--samples", "2", "--n_views", "3"]

    def run(extra):
        capsys.readouterr()
        assert gd.main(common + extra) == 0
        lines = capsys.readouterr().out.strip().splitlines()
        return lines[:-1], json.loads(lines[-1])

    rows, summary = run(["--name_dataset", "one", "--write_splits"])
    assert summary["written"] == 2 and summary["skipped"] == 0 and summary["meta_reused"] == 0 and len(rows) == 2
    assert rows[0].split()[0] == "a" and int(rows[0].split()[1]) == 3 and 0.0 < float(rows[1].split()[2]) < 1.0
    base = str(tmp_path / "one")
    first = _tree_bytes(base)
    assert len(first) == 2 * 3 * 13
    for split in ("train", "val", "test"):
        assert open(os.path.join(base, "03_splits", split + ".lst")).read().split() == ["a", "b"]
    meta_bytes = open(os.path.join(base, "00_img_input", "a", "meta.pkl"), "rb").read()
    rows, summary = run(["--name_dataset", "one"])
    assert summary["written"] == 0 and summary["skipped"] == 2 and rows == []
    rows, summary = run(["--name_dataset", "one", "--overwrite", "--seed", "5"])   # cameras exist: the seed is not consulted
    assert summary["written"] == 2 and summary["meta_reused"] == 2
    assert _tree_bytes(base) == first
    assert open(os.path.join(base, "00_img_input", "a", "meta.pkl"), "rb").read() == meta_bytes
    run(["--name_dataset", "two", "--seed", "5"])
    second = _tree_bytes(str(tmp_path / "two"))
    assert second.keys() == first.keys() and any(second[k] != first[k] for k in first)
    # shape i draws its cameras with seed + i
    with open(tmp_path / "two" / "00_img_input" / "b" / "meta.pkl", "rb") as fh:
        meta = pickle.load(fh)
    want = make_meta(3, 6, size=16)
    assert np.array_equal(meta[2], want[2]) and meta[5] == want[5]
    # an existing meta.pkl fixes the cameras of a fresh tree, and the file on disk is the renderer's image
    third = tmp_path / "three" / "00_img_input" / "b"
    os.makedirs(third)
    mine = make_meta(2, 99, size=16)
    with open(third / "meta.pkl", "wb") as fh:
        pickle.dump(mine, fh)
    rows, summary = run(["--name_dataset", "three", "--slice_direction", "axis"])
    assert summary["meta_reused"] == 1 and int(rows[1].split()[1]) == 2
    mesh_b = load_obj(str(src / "b.obj"))
    img = SliceRenderer((mesh_b.vertices, mesh_b.faces)).render(mine[1][1], mine[2][1], mine[3][1], scale=mine[5], offset=mine[6],
                                                               size=16, samples=2, slice_direction="axis")
    assert np.array_equal(np.asarray(Image.open(third / "001.png")), img[0])
    assert np.array_equal(np.asarray(Image.open(tmp_path / "three" / "01_img_slices" / "b" / "001" / "Y_3.png")), img[7])
    empty = tmp_path / "none"
    empty.mkdir()
    assert gd.main(["--dir_meshes", str(empty), "--name_dataset", "x", "--dir_data", str(tmp_path)]) == 1


# ---------------------------------------------------------------------------------------------- 7: arguments
def test_argument_checks_return_codes_and_messages():
    from slice3d_amd import _lib as L
    from slice3d_amd._lib import S3dError
    from slice3d_amd.mesh_render import SliceRenderer
    lib = L.load()
    assert lib.s3d_version() >= 119
    dev = torch.device("cuda")
    st = L.stream_ptr(dev)
    v = torch.eye(3, dtype=torch.float64, device=dev) * 0.2
    f = torch.tensor([[0, 1, 2]], dtype=torch.int64, device=dev)
    cam = (C.c_double * 26)(*([1, 0, 0, 0, 1, 0, 0, 0, 1, 1.2, 1.0, 0, 0, 0] + [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]))
    size, S, tile = 8, 2, 4
    wsb = lib.s3d_mesh_render_workspace_bytes
    nws = wsb(3, 1, size, S, tile)
    assert nws > 0
    for bad in ((0, 1, size, S, tile), (3, 0, size, S, tile), (3, 1, 0, S, tile), (3, 1, 1025, S, tile), (3, 1, size, 3, tile),
                (3, 1, size, S, 0), (3, 1, size, S, 17), (3, 1, size, 4, 9)):
        assert wsb(*bad) == 0, bad
    assert wsb(3, 1, 1024, 4, 8) > 0 and wsb(3, 1, 1, 1, 32) > 0
    ws = torch.empty(nws, dtype=torch.uint8, device=dev)
    ent = torch.empty(64, dtype=torch.int32, device=dev)
    face = torch.empty((13, size * S, size * S), dtype=torch.int32, device=dev)
    rgba = torch.empty((13, size, size, 4), dtype=torch.uint8, device=dev)
    n = C.c_long(0)

    def failed(rc, code):
        return rc == code and len(lib.s3d_last_error() or b"") > 0

    E_ARG, E_WS = -1, -2
    build, fill, render = lib.s3d_mesh_render_build, lib.s3d_mesh_render_fill, lib.s3d_mesh_render_render
    vp, fp, wp = v.data_ptr(), f.data_ptr(), ws.data_ptr()
    assert failed(build(vp, 3, fp, 0, cam, size, S, tile, wp, nws, C.byref(n), st), E_ARG)                   # F == 0
    assert failed(build(vp, 3, fp, 1, cam, 0, S, tile, wp, nws, C.byref(n), st), E_ARG)                      # size
    assert failed(build(vp, 3, fp, 1, cam, 1025, S, tile, wp, nws, C.byref(n), st), E_ARG)
    assert failed(build(vp, 3, fp, 1, cam, size, 3, tile, wp, nws, C.byref(n), st), E_ARG) and b"samples" in lib.s3d_last_error()
    assert failed(build(vp, 3, fp, 1, cam, size, S, 17, wp, nws, C.byref(n), st), E_ARG) and b"tile" in lib.s3d_last_error()
    assert failed(build(vp, 3, fp, 1, None, size, S, tile, wp, nws, C.byref(n), st), E_ARG)
    assert failed(build(vp, 3, fp, 1, cam, size, S, tile, wp, nws, None, st), E_ARG)
    assert failed(build(vp, 3, fp, 1, cam, size, S, tile, wp, nws - 1, C.byref(n), st), E_WS)                # workspace
    nan_cam = (C.c_double * 26)(*([float("nan")] + list(cam)[1:]))
    assert failed(build(vp, 3, fp, 1, nan_cam, size, S, tile, wp, nws, C.byref(n), st), E_ARG)
    bad = torch.tensor([[0, 1, 3]], dtype=torch.int64, device=dev)
    assert failed(build(vp, 3, bad.data_ptr(), 1, cam, size, S, tile, wp, nws, C.byref(n), st), E_ARG)       # face index
    assert b"outside" in lib.s3d_last_error()
    assert build(vp, 3, fp, 1, cam, size, S, tile, wp, nws, C.byref(n), st) == 0 and 1 <= n.value <= 4
    assert failed(fill(3, 1, size, S, tile, wp, 16, ent.data_ptr(), n.value, st), E_WS)
    assert failed(fill(3, 1, size, S, tile, wp, nws, None, n.value, st), E_ARG)
    assert fill(3, 1, size, S, tile, wp, nws, ent.data_ptr(), n.value, st) == 0
    args = (3, fp, 1, size, S, tile, wp, nws, ent.data_ptr(), n.value, None, None)
    assert failed(render(*args, None, rgba.data_ptr(), None, st), E_ARG)                                     # no face buffer
    assert failed(render(3, fp, 1, size, S, tile, wp, 16, ent.data_ptr(), n.value, None, None, face.data_ptr(),
                         rgba.data_ptr(), None, st), E_WS)
    assert failed(render(3, fp, 1, size, 3, tile, wp, nws, ent.data_ptr(), n.value, None, None, face.data_ptr(),
                         rgba.data_ptr(), None, st), E_ARG)
    assert failed(render(3, None, 1, size, S, tile, wp, nws, ent.data_ptr(), n.value, v.data_ptr(), None, face.data_ptr(),
                         rgba.data_ptr(), None, st), E_ARG)                                                  # colours need faces
    assert render(*args, face.data_ptr(), rgba.data_ptr(), None, st) == 0
    torch.cuda.synchronize()
    assert int((face[0] >= 0).sum()) > 0 and int(rgba[0, ..., 3].max()) > 0
    # the Python layer raises what the library reports
    tri = (np.eye(3) * 0.2, np.array([[0, 1, 2]]))
    with pytest.raises(S3dError):
        SliceRenderer((np.eye(3), np.array([[0, 1, 3]]))).render(0.0, 0.0, 1.2, size=8)
    with pytest.raises(ValueError):
        SliceRenderer((np.eye(3), np.zeros((0, 3), dtype=np.int64)))
    for kw in (dict(size=0), dict(size=1025), dict(samples=3), dict(tile=0), dict(tile=9, samples=4),
               dict(slice_direction="world"), dict(vertex_colors=np.zeros((2, 3))), dict(distance=float("inf"))):
        with pytest.raises(ValueError):
            SliceRenderer(tri).render(0.0, 0.0, **dict(dict(distance=1.2, size=8), **kw))
    out = SliceRenderer(tri).render(0.0, 0.0, 1.2, size=1, samples=1)
    assert out.shape == (13, 1, 1, 4)

"""Host tests of the signed-distance targets (slice3d_amd/mesh_sdf.py): the two reference formulations of the
point-triangle distance agree with each other and with closed forms, the sampling recipe and the file format round-trip
through the real dataset class, and the point sets of tests/test_gpu_mesh_sdf.py meet their preconditions — all with
the host references of tests/sdf_ref.py alone."""
import os
import subprocess
import sys
import types

import numpy as np
import pytest

import mesh_eval_ref
import sdf_cases
import sdf_ref
from sdf_cases import CASES, WATERTIGHT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _box_mesh(lo, hi):
    """An axis-aligned box built by hand: 8 corners, 12 outward-facing triangles."""
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    v = np.array([[x, y, z] for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])])
    f = np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6],
                  [0, 2, 6], [0, 6, 4], [1, 5, 7], [1, 7, 3]], dtype=np.int64)
    return v, f


# ---------------------------------------------------------------------------------------------- the yardsticks
@pytest.mark.parametrize("name", CASES)
def test_formulations_agree_on_fixture(name):
    """A and B on the whole point set of the GPU distance test; their disagreement (times 16) is the first term of the
    gate there, and must stay a rounding error: a larger one is a defect of a formulation, not a reason for a wider gate."""
    da, db = sdf_cases.reference_distances(name)
    diag = sdf_cases.bbox(name)[2]
    pts, first_on = sdf_cases.distance_points(name)
    assert np.isfinite(da).all() and np.isfinite(db).all()
    worst = float(np.abs(da - db).max())
    T, t1, t2 = sdf_cases.tolerance(name)
    print("%s: max|d_A - d_B| = %.3e, 16x = %.3e, floor = %.3e, T = %.3e" % (name, worst, t1, t2, T))
    assert worst <= 1e-9 * diag
    # vertices, edge midpoints and face centroids are on the surface up to the rounding of their own construction: B, which
    # measures along the normal, sees that; A rebuilds the closest point from barycentric coordinates and on the fixtures'
    # sliver faces (aspect ratio ~350 on the torus) is off by the cancellation in them, inside T all the same
    assert db[first_on:].max() <= 8 * 2.0 ** -52 * diag
    assert da[first_on:].max() <= T


def test_formulations_match_closed_form_box():
    lo, hi = np.array([-0.3, -0.5, 0.1]), np.array([0.7, 0.2, 0.9])
    v, f = _box_mesh(lo, hi)
    rng = np.random.default_rng(1)
    p = rng.uniform(-2, 2, (4000, 3))
    p = p[np.any((p < lo) | (p > hi), axis=1)]                       # outside: the distance to a box is known exactly
    exact = sdf_ref.box_distance(lo, hi, p)
    for fn in (sdf_ref.dist_a, sdf_ref.dist_b):
        assert np.abs(fn(v, f, p)[0] - exact).max() <= 8 * 2.0 ** -52 * 4
    # winding number of the hand-built box: 1 inside, 0 outside (faces counter-clockwise seen from outside)
    q = np.concatenate([rng.uniform(lo + 0.05, hi - 0.05, (50, 3)), p[:50]])
    w = sdf_ref.winding(v, f, q)
    assert np.abs(w[:50] - 1).max() < 1e-14 and np.abs(w[50:]).max() < 1e-14


def test_formulations_match_closed_form_flat_square():
    v, f = sdf_cases.mesh("flat")
    lo, hi, _ = sdf_cases.bbox("flat")
    assert (hi - lo == 0).sum() == 1                                 # a square in an axis plane
    p = sdf_cases.crafted("flat")
    exact = sdf_ref.box_distance(lo, hi, p)
    for fn in (sdf_ref.dist_a, sdf_ref.dist_b):
        assert np.abs(fn(v, f, p)[0] - exact).max() <= 8 * 2.0 ** -52 * (1 + np.abs(p).max())


def test_zero_area_faces_are_segments_and_points():
    v = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0], [0, 0, 0], [5, 5, 5]], dtype=np.float64)
    f = np.array([[0, 1, 2], [0, 0, 1], [4, 4, 4], [0, 2, 1]])     # collinear, repeated vertex, a point, collinear
    p = np.array([[1.5, 1.0, 0.0], [-1.0, 0.0, 0.0], [5.0, 5.0, 6.0], [3.0, 0.0, 4.0]])
    tri = v[f]
    for fn in (sdf_ref.point_tri_a, sdf_ref.point_tri_b):
        d = fn(p[:, None, :], tri[None, :, 0], tri[None, :, 1], tri[None, :, 2])
        assert np.isfinite(d).all()
        assert np.allclose(d[0], [1.0, np.hypot(0.5, 1.0), np.linalg.norm(p[0] - 5), 1.0], rtol=0, atol=1e-15)
        assert np.allclose(d[3, [0, 1]], [np.hypot(1, 4), np.hypot(2, 4)], rtol=0, atol=1e-15)
        assert d[2, 2] == 1.0 and d[1, 0] == 1.0


# ---------------------------------------------------------------------------------------------- preconditions of the GPU items
@pytest.mark.parametrize("name", CASES + ["open_sphere"])
def test_winding_points_leave_out_few(name):
    """Item 5: at most 0.5 % of the points are nearer to the surface than 1e-9 diagonals.  The crafted points of a
    fixture that would break the cap are not in its set at all (the cap is not raised): that is the case for `boxes`,
    whose crafted points include points on its faces."""
    pts, left_out, with_crafted = sdf_cases.winding_points(name)
    print("%s: %d points, %.3f %% left out, crafted points %s" % (name, len(pts), 100 * left_out,
                                                                   "in" if with_crafted else "dropped"))
    assert left_out <= sdf_cases.LEFT_OUT_CAP
    assert len(pts) >= 1900
    assert with_crafted == (name != "boxes")
    v, f = sdf_cases.mesh(name)
    w = sdf_ref.winding(v, f, pts[:400])
    assert np.isfinite(w).all()
    if name in WATERTIGHT or name == "zero_area":
        assert np.abs(w - np.round(w)).max() < 1e-12                # a closed surface: an integer everywhere off it


@pytest.mark.parametrize("name", WATERTIGHT)
def test_sign_points_have_no_parity_disagreement(name):
    """Item 6: on the seeded uniform points the ray-parity reference reports no point whose two parities differ, at most
    0.5 % of them are within 1e-6 diagonals of the surface, and away from it the winding number of the reference and the
    parity of the reference already give the same sign."""
    pts, da, n_dis = sdf_cases.sign_points(name)
    assert n_dis == 0
    diag = sdf_cases.bbox(name)[2]
    clear = da > 1e-6 * diag
    assert (~clear).mean() <= 0.005
    v, f = sdf_cases.mesh(name)
    sub = np.flatnonzero(clear)[:600]
    inside = mesh_eval_ref.contains(v, f, pts)[0]
    assert np.array_equal(sdf_ref.winding(v, f, pts[sub]) > 0.5, inside[sub])
    assert 0 < inside.sum() < len(pts)


def test_open_sphere_winding_is_fractional_under_the_hole():
    v, f = sdf_cases.mesh("open_sphere")
    assert 0 < len(f) < len(sdf_cases.mesh("sphere")[1])
    p = _cone_points()
    w = sdf_ref.winding(v, f, p)
    assert (w > 0).all() and (w < 1).all()


def _cone_points():
    """Points on the axis of the missing cap and a little off it, inside the sphere and above it."""
    lo, hi, _ = sdf_cases.bbox("sphere")
    c, r = 0.5 * (lo + hi), 0.5 * (hi - lo)[2]
    t = np.linspace(-0.5, 0.9, 15)
    axis = c + np.stack([0 * t, 0 * t, t * r], 1)
    return np.concatenate([axis, axis + [0.05 * r, -0.03 * r, 0.0]])


# ---------------------------------------------------------------------------------------------- python layer
def test_normalize_mesh():
    from slice3d_amd.mesh_sdf import normalize_mesh
    v = np.random.default_rng(0).uniform(-3, 7, (100, 3)) * [1, 2, 0.5]
    n = normalize_mesh(v)
    lo, hi = n.min(0), n.max(0)
    assert np.linalg.norm(hi - lo) == pytest.approx(1.0, abs=1e-15)
    assert np.abs(lo + hi).max() < 1e-15
    assert np.array_equal(normalize_mesh(np.ones((1, 3))), np.zeros((1, 3)))


def test_default_resolution_grows_with_faces():
    from slice3d_amd.mesh_sdf import default_resolution
    assert default_resolution(2) == 4 and default_resolution(10 ** 7) == 128
    assert default_resolution(2000) < default_resolution(100000) <= 128


def test_sample_sdf_points_is_a_pure_function_of_its_inputs():
    from slice3d_amd.mesh_sdf import sample_sdf_points
    v, f = sdf_cases.mesh("torus")
    lo, hi, diag = sdf_cases.bbox("torus")
    tri = v[f]
    n = 4000
    surf = tri[np.arange(3000) % len(f)].mean(axis=1).astype(np.float32)        # stands in for sample_surface
    a = sample_sdf_points((v, f), n, 5, surface_samples=surf)
    b = sample_sdf_points((v, f), n, 5, surface_samples=surf)
    c = sample_sdf_points((v, f), n, 6, surface_samples=surf)
    assert a.shape == (n, 3) and a.dtype == np.float64
    assert np.array_equal(a, b) and not np.array_equal(a, c)
    # regenerated on the host from the documented recipe
    rng = np.random.default_rng(5)
    sigma = np.full((3000, 1), 0.01 * diag)
    sigma[:1500] = 0.0025 * diag
    near = surf.astype(np.float64) + rng.standard_normal((3000, 3)) * sigma
    uni = 0.5 * (lo + hi) + rng.uniform(-0.5, 0.5, (1000, 3))
    assert np.array_equal(a, np.concatenate([near, uni]))
    # shares and box
    off = np.linalg.norm(a[:3000] - surf, axis=1) / diag
    mean_norm = 2 * np.sqrt(2 / np.pi)                               # E|x| of an isotropic unit normal in 3-D
    assert off[:1500].mean() == pytest.approx(0.0025 * mean_norm, rel=0.05)
    assert off[1500:].mean() == pytest.approx(0.01 * mean_norm, rel=0.05)
    assert np.all(np.abs(a[3000:] - 0.5 * (lo + hi)) <= 0.5)
    d = sample_sdf_points((v, f), 10, 0, surface_share=0.0, box=2.0)
    assert d.shape == (10, 3) and np.abs(d - 0.5 * (lo + hi)).max() > 0.5
    with pytest.raises(ValueError):
        sample_sdf_points((v, f), n, 5, surface_samples=surf[:10])
    assert "not been tuned" in sample_sdf_points.__doc__


def test_make_sdf_file_round_trips_through_the_dataset(tmp_path):
    """The file written with a host distance function, read back by the real Slice3DDataset on a toy tree: the dataset's
    sdf is the true signed distance times its scale (to float32 rounding) and its occupancy is the inside mask."""
    import pickle
    from slice3d_amd.datasets import Slice3DDataset, write_toy_dataset
    from slice3d_amd.mesh_sdf import SDF_LEVEL, make_sdf_file, sample_sdf_points
    write_toy_dataset(str(tmp_path), "toy", seed=2)
    v, f = _box_mesh([-0.2, -0.25, -0.3], [0.2, 0.25, 0.3])
    n = 500
    truth = {}

    def host_sdf(mesh, p32):
        assert p32.dtype == np.float32                              # computed from the points that are written
        d = sdf_ref.dist_a(mesh[0], mesh[1], p32)[0]
        inside = sdf_ref.winding(mesh[0], mesh[1], p32) > 0.5
        truth["d"], truth["inside"] = d, inside
        return np.where(inside, -d, d)

    for i, sh in enumerate(("shape_a", "shape_b")):
        surf = v[f][np.arange(n) % len(f)].mean(axis=1)
        pts = sample_sdf_points((v, f), n, 10 + i, surface_samples=surf)
        path = str(tmp_path / "toy" / "02_sdfs" / (sh + ".npy"))
        out = make_sdf_file((v, f), path, n, 10 + i, sdf_fn=host_sdf, points=pts)
        on_disk = np.load(path)
        assert on_disk.dtype == np.float32 and on_disk.shape == (n, 4) and np.array_equal(on_disk, out)
        assert np.array_equal(on_disk[:, :3], pts.astype(np.float32))
        sd = np.where(truth["inside"], -truth["d"], truth["d"])
        assert np.abs(on_disk[:, 3].astype(np.float64) - (sd + SDF_LEVEL)).max() <= 2.0 ** -24 * 1.0
        args = types.SimpleNamespace(n_qry=n, dir_data=str(tmp_path), name_dataset="toy", img_size=16,
                                     from_which_slices="gt", use_white_bg=False, n_views=6, categories_train="",
                                     categories_test="")
        ds = Slice3DDataset("test", args, with_slices=False)
        idx = [k for k in range(len(ds)) if ds.files[k][1] == sh][0]
        item = ds[idx]
        with open(tmp_path / "toy" / "00_img_input" / sh / "meta.pkl", "rb") as fh:
            scale = pickle.load(fh)[5]
        np.random.seed(1234)
        perm = np.random.permutation(n)[:n]                         # the dataset's own query order (datasets.py:149-150)
        got_sdf, got_occ = item["sdf"].numpy().astype(np.float64), item["occ"].numpy()
        # |sd| < 1: the stored value carries half a float32 ulp of (sd + level), the dataset's subtraction and scaling two more
        assert np.abs(got_sdf - sd[perm] * scale).max() <= 4 * 2.0 ** -24 * scale
        clear = np.abs(sd[perm]) > 4 * 2.0 ** -24
        assert clear.mean() > 0.99
        assert np.array_equal(got_occ[clear] > 0.5, truth["inside"][perm][clear])
        assert 0 < truth["inside"].sum() < n


def test_make_sdfs_help_parses_and_needs_meshes(tmp_path):
    script = os.path.join(ROOT, "reg_slices", "make_sdfs.py")
    r = subprocess.run([sys.executable, script, "--help"], capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert r.returncode == 0, r.stderr
    for flag in ("--dir_meshes", "--name_dataset", "--dir_data", "--n_points", "--sign", "--normalize", "--seed",
                 "--dir_out_meshes", "--overwrite"):
        assert flag in r.stdout
    r = subprocess.run([sys.executable, script, "--dir_meshes", str(tmp_path), "--name_dataset", "x", "--dir_data",
                        str(tmp_path)], capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert r.returncode == 1 and '"n_shapes": 0' in r.stdout


def test_header_and_binding_declare_the_same_entry_points():
    from slice3d_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "slice3d_hip.h")).read()
    for name in ("s3d_mesh_dist_workspace_bytes", "s3d_mesh_dist_build", "s3d_mesh_dist_fill", "s3d_mesh_dist_query",
                 "s3d_mesh_winding_workspace_bytes", "s3d_mesh_winding"):
        assert name in _lib.SYMBOLS and (name + "(") in hdr

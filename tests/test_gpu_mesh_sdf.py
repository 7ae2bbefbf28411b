"""GPU tests of the signed-distance kernels (csrc/mesh_sdf.hip) through slice3d_amd/mesh_sdf.py: the exact distance and
the face that attains it against two float64 brute-force formulations (tests/sdf_ref.py), bit-level determinism over
runs, grid resolutions and point widths, the culling counter, the generalised winding number against an exactly rounded
sum, the two sign definitions, the argument checks, and reg_slices/make_sdfs.py end to end into eval_meshes.py."""
import ctypes as C
import csv
import json
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch

import mesh_eval_ref
import sdf_cases
import sdf_ref
from sdf_cases import CASES, WATERTIGHT

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(t):
    t = t if isinstance(t, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(t))
    return t.contiguous().view(torch.int64) if t.dtype == torch.float64 else t


def _same(a, b):
    return torch.equal(_bits(a).cpu(), _bits(b).cpu())


# ---------------------------------------------------------------------------------------------- 1, 2: distance and face
@pytest.mark.parametrize("name", CASES)
def test_distance_and_face_match_both_formulations(name):
    """|dist - d_A| <= T = max(16 max|d_A - d_B|, 64 * 2^-52 * (diag + max|p|)), T computed here from A and B on the same
    points; the face is checked through its own distance: d_A(p, face[p]) within T of dist."""
    from slice3d_amd.mesh_sdf import MeshDistance
    v, f = sdf_cases.mesh(name)
    pts, first_on = sdf_cases.distance_points(name)
    da, _ = sdf_cases.reference_distances(name)
    T, t1, t2 = sdf_cases.tolerance(name)
    dist, face = MeshDistance((v, f)).query(pts, return_face=True)
    assert dist.dtype == np.float64 and face.dtype == np.int64 and np.isfinite(dist).all()
    err = np.abs(dist - da)
    err_face = np.abs(sdf_ref.dist_a_face(v, f, pts, face) - dist)
    print("%s: n = %d, 16 max|d_A - d_B| = %.3e, floor = %.3e, T = %.3e, max|dist - d_A| = %.3e, "
          "max|d_A(face) - dist| = %.3e, max on-surface dist = %.3e"
          % (name, len(pts), t1, t2, T, err.max(), err_face.max(), dist[first_on:].max()))
    assert (face >= 0).all() and (face < len(f)).all()
    assert err.max() <= T
    assert err_face.max() <= T


def test_distance_device_tensors_in_and_out():
    from slice3d_amd.mesh_sdf import MeshDistance
    v, f = sdf_cases.mesh("torus")
    pts = sdf_cases.distance_points("torus")[0][:500]
    md = MeshDistance((torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda()))
    d, fa = md.query(torch.from_numpy(pts).cuda(), return_face=True)
    assert d.is_cuda and d.dtype == torch.float64 and fa.is_cuda and fa.dtype == torch.int64
    assert _same(d, MeshDistance((v, f)).query(pts))
    assert int(md.n_tests) > 0


# ---------------------------------------------------------------------------------------------- 3: determinism
@pytest.mark.parametrize("name", CASES)
def test_distance_is_bit_identical_over_runs_resolutions_and_widths(name):
    from slice3d_amd.mesh_sdf import MeshDistance
    v, f = sdf_cases.mesh(name)
    pts = sdf_cases.distance_points(name)[0]
    d0, f0 = MeshDistance((v, f)).query(pts, return_face=True)
    d1, f1 = MeshDistance((v, f)).query(pts, return_face=True)
    assert _same(d0, d1) and _same(f0, f1)
    for res in (8, 32, 1):
        dr, fr = MeshDistance((v, f), resolution=res).query(pts, return_face=True)
        assert _same(d0, dr) and _same(f0, fr), res
    p32 = pts.astype(np.float32)
    md = MeshDistance((v, f))
    a = md.query(p32, return_face=True)
    b = md.query(p32.astype(np.float64), return_face=True)
    assert _same(a[0], b[0]) and _same(a[1], b[1])
    # workspace memory handed back by the caching allocator holds old bytes; the result must not depend on them
    junk = torch.full((64 << 20,), 0x7f, dtype=torch.uint8, device="cuda")
    del junk
    d2, f2 = MeshDistance((v, f)).query(pts, return_face=True)
    assert _same(d0, d2) and _same(f0, f2)


def test_lowest_face_index_wins_ties():
    from slice3d_amd.mesh_sdf import MeshDistance
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0]], dtype=np.float64)
    f = np.array([[1, 2, 3], [0, 1, 2], [1, 2, 3], [0, 1, 2]])     # each face twice; the shared edge belongs to all four
    p = np.array([[0.5, 0.5, 1.0], [0.9, 0.9, 2.0], [0.1, 0.1, -1.0], [0.25, 0.75, 0.5]])
    for res in (1, 4, 16):
        d, fa = MeshDistance((v, f), resolution=res).query(p, return_face=True)
        assert fa.tolist() == [0, 0, 1, 0] and d.tolist() == [1.0, 2.0, 1.0, 0.5]


# ---------------------------------------------------------------------------------------------- 4: culling
def _mc_torus(n):
    from slice3d_amd.mesh import marching_cubes_device
    g = torch.linspace(-1, 1, n, dtype=torch.float64, device="cuda")
    x, y, z = torch.meshgrid(g, g, g, indexing="ij")
    q = torch.sqrt(x ** 2 + y ** 2) - 0.5
    field = torch.maximum(0.22 - torch.sqrt(q ** 2 + z ** 2), 0.35 - torch.sqrt((x - 0.3) ** 2 + y ** 2 + (z - 0.35) ** 2))
    return marching_cubes_device(field, 0.0)


def test_culling_on_marching_cubes_mesh():
    """A 129^3 marching-cubes mesh straight from the device and 200 k uniform points in its bounding box: the query
    performs at most a quarter of the n * F tests of a brute force (a condition that separates "culls" from "does not",
    not a measurement), and 2 000 of the points equal formulation A."""
    from slice3d_amd.mesh_sdf import MeshDistance
    v, f = _mc_torus(129)
    vn, fn = v.cpu().numpy(), f.cpu().numpy()
    lo, hi = vn[fn.reshape(-1)].min(0), vn[fn.reshape(-1)].max(0)
    n = 200000
    pts = np.random.default_rng(9).uniform(lo, hi, (n, 3))
    md = MeshDistance((v, f))
    dist = md.query(torch.from_numpy(pts).cuda()).cpu().numpy()
    tests = int(md.n_tests)
    print("faces = %d, resolution = %d, tests per point = %.1f (brute force: %d)" % (len(fn), md.resolution, tests / n, len(fn)))
    assert 0 < tests <= n * len(fn) // 4
    sub = np.arange(0, n, n // 2000)[:2000]
    da = sdf_ref.dist_a(vn, fn, pts[sub])[0]
    diag = float(np.linalg.norm(hi - lo))
    T = 64 * 2.0 ** -52 * (diag + np.abs(pts).max())
    print("max|dist - d_A| on %d points = %.3e (floor term of the gate: %.3e)" % (len(sub), np.abs(dist[sub] - da).max(), T))
    assert np.abs(dist[sub] - da).max() <= T


# ---------------------------------------------------------------------------------------------- 5: winding number
@pytest.mark.parametrize("name", CASES + ["open_sphere"])
def test_winding_number_matches_exact_sum(name):
    """|w - w_C| <= 16 * 2^-52 * F: F float64 terms of magnitude <= 1/2 summed in some order against an exactly rounded
    sum, 16x for the device library's atan2.  The bound does not cover the conditioning of the formula itself: within
    ~1e-3 edge lengths of an edge the atan2's two arguments vanish together, and on `flat` (F = 2, crafted points over the
    square's edges) the reference is 4.1e-14 from an 80-bit evaluation.  The gate holds there because the kernel forms
    the arguments with the same unfused IEEE operations in the same order as the reference; with fused dot products it
    measured 1.6e-14 against the gate's 7.1e-15."""
    from slice3d_amd.mesh_sdf import winding_number
    v, f = sdf_cases.mesh(name)
    pts, left_out, _ = sdf_cases.winding_points(name)
    assert left_out <= sdf_cases.LEFT_OUT_CAP
    w = winding_number((v, f), pts)
    ref = sdf_ref.winding(v, f, pts)
    gate = 16 * 2.0 ** -52 * len(f)
    assert w.dtype == np.float64 and np.isfinite(w).all()
    print("%s: n = %d, F = %d, max|w - w_C| = %.3e, gate = %.3e" % (name, len(pts), len(f), np.abs(w - ref).max(), gate))
    assert np.abs(w - ref).max() <= gate
    # bit-equal over two runs, over split counts, and for a few points (which forces the split over faces) against the
    # same points inside a large batch
    assert _same(w, winding_number((v, f), pts))
    for splits in (1, 3, 32):
        assert _same(w, winding_number((v, f), pts, n_splits=splits)), splits
    assert _same(w[:7], winding_number((v, f), pts[:7]))
    big = np.concatenate([pts] * 70)[:300000]
    wb = winding_number((torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda()), torch.from_numpy(big).cuda())
    assert wb.is_cuda and _same(wb[: len(pts)], w) and _same(wb[-len(pts):], wb[len(big) - len(pts):])
    k = len(big) - len(big) % len(pts) - len(pts)                   # the last whole copy: another batch, the same bits
    assert _same(wb[k:k + len(pts)], w)


def test_winding_number_on_surface_points_is_finite():
    from slice3d_amd.mesh_sdf import winding_number
    v, f = sdf_cases.mesh("zero_area")
    pts, first_on = sdf_cases.distance_points("zero_area")
    w = winding_number((v, f), pts[first_on:])                      # vertices, edge midpoints, face centroids
    # on the surface a face holding the point contributes its limit value from either side (+-1/2) or nothing
    assert np.isfinite(w).all() and w.min() > -1.01 and w.max() < 2.01


# ---------------------------------------------------------------------------------------------- 6: sign
@pytest.mark.parametrize("name", CASES)
def test_parity_sign_equals_check_mesh_contains(name):
    from slice3d_amd.mesh_eval import check_mesh_contains
    from slice3d_amd.mesh_sdf import MeshDistance, signed_distance
    v, f = sdf_cases.mesh(name)
    pts = sdf_cases.crafted(name)
    sd = signed_distance((v, f), pts, sign="parity")
    inside = check_mesh_contains((v, f), pts)
    assert np.array_equal(inside, sdf_cases.gold()[name + "_contains"])
    assert np.array_equal(np.signbit(sd), inside)
    assert _same(np.abs(sd), MeshDistance((v, f)).query(pts))
    with pytest.raises(ValueError):
        signed_distance((v, f), pts[:3], sign="normal")


@pytest.mark.parametrize("name", WATERTIGHT)
def test_winding_and_parity_signs_agree_on_fresh_points(name):
    from slice3d_amd.mesh_sdf import signed_distance
    v, f = sdf_cases.mesh(name)
    pts, da, n_dis = sdf_cases.sign_points(name)
    assert n_dis == 0                                               # precondition, references only
    diag = sdf_cases.bbox(name)[2]
    clear = da > 1e-6 * diag
    assert (~clear).mean() <= 0.005
    sp = signed_distance((v, f), pts, sign="parity")
    sw = signed_distance((v, f), pts, sign="winding")
    assert np.array_equal(np.signbit(sp)[clear], np.signbit(sw)[clear])
    assert np.array_equal(np.signbit(sp), mesh_eval_ref.contains(v, f, pts)[0])
    assert _same(np.abs(sp), np.abs(sw))
    assert 0 < np.signbit(sp).sum() < len(pts)


def test_open_sphere_winding_is_fractional_under_the_hole():
    from slice3d_amd.mesh_sdf import winding_number
    from test_mesh_sdf import _cone_points
    w = winding_number(sdf_cases.mesh("open_sphere"), _cone_points())
    assert (w > 0).all() and (w < 1).all()


# ---------------------------------------------------------------------------------------------- 7: arguments
def test_argument_checks_return_codes_and_messages():
    from slice3d_amd import _lib as L
    from slice3d_amd._lib import S3dError
    from slice3d_amd.mesh_sdf import MeshDistance, winding_number
    lib = L.load()
    dev = torch.device("cuda")
    st = L.stream_ptr(dev)
    v = torch.eye(3, dtype=torch.float64, device=dev)
    f = torch.tensor([[0, 1, 2]], dtype=torch.int64, device=dev)
    p = torch.zeros((4, 3), dtype=torch.float64, device=dev)
    out = torch.empty(4, dtype=torch.float64, device=dev)
    nws = lib.s3d_mesh_dist_workspace_bytes(1, 8)
    assert nws > 0 and lib.s3d_mesh_dist_workspace_bytes(1, 0) == 0 and lib.s3d_mesh_dist_workspace_bytes(1, 257) == 0
    assert lib.s3d_mesh_dist_workspace_bytes(0, 8) == 0
    ws = torch.empty(nws, dtype=torch.uint8, device=dev)
    ent = torch.empty(4096, dtype=torch.int32, device=dev)
    n = C.c_long(0)

    def failed(rc, code):
        return rc == code and len(lib.s3d_last_error() or b"") > 0

    E_ARG, E_WS = -1, -2
    build = lib.s3d_mesh_dist_build
    assert failed(build(v.data_ptr(), 3, f.data_ptr(), 0, 8, ws.data_ptr(), nws, C.byref(n), st), E_ARG)      # F == 0
    assert failed(build(v.data_ptr(), 3, f.data_ptr(), 1, 0, ws.data_ptr(), nws, C.byref(n), st), E_ARG)      # resolution
    assert failed(build(v.data_ptr(), 3, f.data_ptr(), 1, 257, ws.data_ptr(), nws, C.byref(n), st), E_ARG)
    assert failed(build(v.data_ptr(), 3, f.data_ptr(), 1, 8, ws.data_ptr(), nws - 1, C.byref(n), st), E_WS)   # workspace
    assert failed(lib.s3d_mesh_dist_query(1, 8, ws.data_ptr(), 16, ent.data_ptr(), 1, p.data_ptr(), 1, 4, out.data_ptr(),
                                          None, None, st), E_WS)
    bad = torch.tensor([[0, 1, 3]], dtype=torch.int64, device=dev)
    assert failed(build(v.data_ptr(), 3, bad.data_ptr(), 1, 8, ws.data_ptr(), nws, C.byref(n), st), E_ARG)    # face index
    assert b"outside" in lib.s3d_last_error()
    assert build(v.data_ptr(), 3, f.data_ptr(), 1, 8, ws.data_ptr(), nws, C.byref(n), st) == 0 and 1 <= n.value <= 4096
    assert lib.s3d_mesh_dist_fill(1, 8, ws.data_ptr(), nws, ent.data_ptr(), n.value, st) == 0
    assert lib.s3d_mesh_dist_query(1, 8, ws.data_ptr(), nws, ent.data_ptr(), n.value, None, 1, 0, None, None, None, st) == 0
    # winding number
    wws = lib.s3d_mesh_winding_workspace_bytes(1, 4)
    w2 = torch.empty(max(wws, 1), dtype=torch.uint8, device=dev)
    wind = lib.s3d_mesh_winding
    assert lib.s3d_mesh_winding_workspace_bytes(0, 4) == 0
    assert failed(wind(v.data_ptr(), 3, f.data_ptr(), 0, p.data_ptr(), 1, 4, 0, w2.data_ptr(), wws, out.data_ptr(), st), E_ARG)
    assert failed(wind(v.data_ptr(), 3, f.data_ptr(), 1, p.data_ptr(), 1, 4, 0, w2.data_ptr(), wws - 1, out.data_ptr(), st), E_WS)
    assert failed(wind(v.data_ptr(), 3, bad.data_ptr(), 1, p.data_ptr(), 1, 4, 0, w2.data_ptr(), wws, out.data_ptr(), st), E_ARG)
    assert wind(v.data_ptr(), 3, f.data_ptr(), 1, None, 1, 0, 0, w2.data_ptr(), wws, None, st) == 0
    assert wind(v.data_ptr(), 3, f.data_ptr(), 1, p.data_ptr(), 1, 4, 0, w2.data_ptr(), wws, out.data_ptr(), st) == 0
    # the Python layer raises what the library reports
    with pytest.raises(S3dError):
        MeshDistance((np.eye(3), np.array([[0, 1, 3]])))
    with pytest.raises(S3dError):
        winding_number((np.eye(3), np.array([[0, 1, 3]])), np.zeros((2, 3)))
    with pytest.raises(ValueError):
        MeshDistance((np.eye(3), np.array([[0, 1, 2]])), resolution=300)
    with pytest.raises(ValueError):
        MeshDistance((np.eye(3), np.zeros((0, 3), dtype=np.int64)))
    assert MeshDistance((np.eye(3), np.array([[0, 1, 2]]))).query(np.zeros((0, 3))).shape == (0,)
    assert winding_number((np.eye(3), np.array([[0, 1, 2]])), np.zeros((0, 3))).shape == (0,)


# ---------------------------------------------------------------------------------------------- 8: end to end
def test_make_sdfs_end_to_end(tmp_path):
    from slice3d_amd.datasets import write_toy_dataset
    from slice3d_amd.mesh import Mesh
    shapes = ("shape_a", "shape_b")
    write_toy_dataset(str(tmp_path), "custom", shapes=shapes, n_pts=500, seed=4)
    base = tmp_path / "custom"
    for sh in shapes:                                               # the dataset's map becomes the identity
        path = base / "00_img_input" / sh / "meta.pkl"
        with open(path, "rb") as fh:
            meta = pickle.load(fh)
        meta[5], meta[6] = 1.0, [0.0, 0.0, 0.0]
        with open(path, "wb") as fh:
            pickle.dump(meta, fh)
    src, out = tmp_path / "meshes", tmp_path / "gt"
    src.mkdir()
    for sh, name in zip(shapes, ("sphere", "torus")):
        v, f = sdf_cases.mesh(name)
        Mesh(v * 0.35, f).export(str(src / (sh + ".obj")))           # inside the dataset's unit cube
    n = 20000
    cmd = [sys.executable, os.path.join(ROOT, "reg_slices", "make_sdfs.py"), "--dir_meshes", str(src), "--name_dataset",
           "custom", "--dir_data", str(tmp_path), "--n_points", str(n), "--sign", "parity", "--dir_out_meshes", str(out)]

    def run(extra):
        r = subprocess.run(cmd + extra, capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert r.returncode == 0, r.stdout + r.stderr
        lines = r.stdout.strip().splitlines()
        return lines[:-1], json.loads(lines[-1])

    # the toy tree already holds 02_sdfs files: they are skipped unless --overwrite
    rows, summary = run([])
    assert summary["written"] == 0 and summary["skipped"] == 2 and rows == []
    rows, summary = run(["--overwrite"])
    assert summary["written"] == 2 and summary["n_shapes"] == 2 and len(rows) == 2
    first = {}
    for sh, row in zip(shapes, rows):
        tok = row.split()
        assert tok[0] == sh and int(tok[1]) == n and 0.0 < float(tok[2]) < 1.0
        a = np.load(base / "02_sdfs" / (sh + ".npy"))
        assert a.dtype == np.float32 and a.shape == (n, 4) and np.isfinite(a).all()
        first[sh] = a
    run(["--overwrite"])
    for sh in shapes:
        assert np.array_equal(np.load(base / "02_sdfs" / (sh + ".npy")), first[sh])
    run(["--overwrite", "--seed", "7"])
    for sh in shapes:
        assert not np.array_equal(np.load(base / "02_sdfs" / (sh + ".npy")), first[sh])
    run(["--overwrite"])
    # scored against the meshes they were made from: both sides read the same .obj, and the occupancy written and the
    # occupancy scored come from the same float32 points through the same point-in-mesh test
    ev = [sys.executable, os.path.join(ROOT, "reg_slices", "eval_meshes.py"), "--dir_data", str(tmp_path), "--name_dataset",
          "custom", "--n_views", "6", "--n_qry", str(n), "--dir_results", str(out)]
    r = subprocess.run(ev, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout + r.stderr
    with open(out / "eval.csv") as fh:
        rows = {row["shape"]: row for row in csv.DictReader(fh)}
    for sh in shapes:
        assert float(rows[sh]["iou"]) == 1.0
    # no mesh at all: exit status 1
    empty = tmp_path / "none"
    empty.mkdir()
    r = subprocess.run(cmd[:3] + [str(empty)] + cmd[4:], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 1

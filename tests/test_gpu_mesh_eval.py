"""GPU tests of the mesh scoring kernels (csrc/mesh_eval.hip) through slice3d_amd/mesh_eval.py: point-in-mesh bit for bit
against the reference's own output (tests/golden/mesh_eval_reference.npz) and the host restatement
(tests/mesh_eval_ref.py), exact nearest neighbours against float64 brute force, Chamfer / Hausdorff against the
reference's numbers, surface sampling, and reg_slices/eval_meshes.py end to end."""
import csv
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from helpers import GOLDEN
import mesh_eval_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["sphere", "torus", "boxes", "zero_area", "flat"]


@pytest.fixture(scope="module")
def gold():
    z = np.load(os.path.join(GOLDEN, "mesh_eval_reference.npz"))
    return {k: z[k] for k in z.files}


# ---------------------------------------------------------------------------------------------- point-in-mesh
@pytest.mark.parametrize("name", CASES)
def test_contains_equals_reference(gold, name):
    from slice3d_amd.mesh_eval import MeshIntersector, check_mesh_contains
    v, f, pts = gold[name + "_v"], gold[name + "_f"], gold[name + "_pts"]
    assert np.array_equal(check_mesh_contains((v, f), pts), gold[name + "_contains"])
    # device tensors in, device tensor out; the disagreement count equals the restatement's
    inter = MeshIntersector((torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda()))
    out = inter.query(torch.from_numpy(pts).cuda())
    assert out.is_cuda and out.dtype == torch.bool
    assert np.array_equal(out.cpu().numpy(), gold[name + "_contains"])
    assert int(inter.n_disagree) == mesh_eval_ref.contains(v, f, pts)[1]


def test_contains_float32_points(gold):
    from slice3d_amd.mesh_eval import check_mesh_contains
    got = check_mesh_contains((gold["sphere_v"], gold["sphere_f"]), gold["sphere_pts32"])
    assert np.array_equal(got, gold["sphere_contains32"])


def test_contains_marching_cubes_mesh_matches_restatement():
    """A 129^3 marching-cubes mesh straight from the device (float64 vertices, int64 faces) and 200 k points."""
    from slice3d_amd.mesh import marching_cubes_device
    from slice3d_amd.mesh_eval import MeshIntersector
    n = 129
    g = torch.linspace(-1, 1, n, dtype=torch.float64, device="cuda")
    x, y, z = torch.meshgrid(g, g, g, indexing="ij")
    q = torch.sqrt(x ** 2 + y ** 2) - 0.5
    field = torch.maximum(0.22 - torch.sqrt(q ** 2 + z ** 2), 0.35 - torch.sqrt((x - 0.3) ** 2 + y ** 2 + (z - 0.35) ** 2))
    v, f = marching_cubes_device(field, 0.0)
    rng = np.random.default_rng(5)
    pts = rng.uniform(-2, n + 1, (200000, 3))
    pts[:20000] = np.round(pts[:20000] * 4) / 4          # many points on vertex / edge planes of the grid
    inter = MeshIntersector((v, f))
    got = inter.query(torch.from_numpy(pts).cuda()).cpu().numpy()
    ref, n_dis = mesh_eval_ref.contains(v.cpu().numpy(), f.cpu().numpy(), pts)
    assert np.array_equal(got, ref)
    assert int(inter.n_disagree) == n_dis
    assert 1000 < ref.sum() < len(pts) - 1000


def test_contains_last_cell_on_dirty_workspace(gold):
    """The bbox max corner rescales to (res - 0.5, res - 0.5): the last cell, whose list ends at the offsets' final
    entry.  Workspace memory handed back by the caching allocator holds old bytes; the result must not depend on them."""
    from slice3d_amd.mesh_eval import MeshIntersector
    v, f = gold["torus_v"], gold["torus_f"]
    junk = torch.full((64 << 20,), 0x7f, dtype=torch.uint8, device="cuda")
    del junk
    inter = MeshIntersector((v, f))
    tri = v[f].reshape(-1, 3)
    pts = np.stack([tri.max(0), tri.min(0), 0.5 * (tri.max(0) + tri.min(0))])
    assert np.array_equal(inter.query(pts), mesh_eval_ref.contains(v, f, pts)[0])


def test_eval_iou_empty_mesh():
    from slice3d_amd.mesh_eval import eval_iou
    empty = (torch.zeros((0, 3), dtype=torch.float64, device="cuda"), torch.zeros((0, 3), dtype=torch.int64, device="cuda"))
    assert eval_iou(empty, torch.zeros((4, 3), device="cuda"), np.ones(4)) == 0.0


def test_contains_rejects_bad_face_index():
    from slice3d_amd._lib import S3dError
    from slice3d_amd.mesh_eval import check_mesh_contains
    with pytest.raises(S3dError):
        check_mesh_contains((np.eye(3), np.array([[0, 1, 3]])), np.zeros((2, 3)))


# ---------------------------------------------------------------------------------------------- nearest neighbour
@pytest.mark.parametrize("na,nb", [(1, 1), (7, 300), (1000, 1), (33333, 20000)])
def test_nn_matches_brute_force(na, nb):
    from slice3d_amd.mesh_eval import nn_sqdist
    rng = np.random.default_rng(na * 7 + nb)
    a = rng.uniform(-1, 1, (na, 3)).astype(np.float32)
    b = rng.uniform(-1, 1, (nb, 3)).astype(np.float32)
    a[: na // 10] = b[rng.integers(0, nb, na // 10)]                  # duplicates: distance exactly 0
    d2, idx = nn_sqdist(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(), return_ind=True)
    d2, idx = d2.cpu().numpy().astype(np.float64), idx.cpu().numpy()
    ref, ref_idx, second = mesh_eval_ref.nn_brute(a, b)
    assert np.all(np.abs(d2 - ref) <= 1e-6 * ref)
    assert np.all(d2[: na // 10] == 0.0)
    clear = second > ref * (1 + 2e-6) + 1e-30
    assert np.array_equal(idx[clear], ref_idx[clear])


def test_nn_lowest_index_wins_ties():
    from slice3d_amd.mesh_eval import nn_sqdist
    b = np.zeros((5000, 3), dtype=np.float32)
    b[:, 0] = 1.0 + np.arange(5000)
    b[[17, 1234, 4321]] = [0.5, 0.0, 0.0]                          # three equal nearest points, far apart in index
    a = np.zeros((3000, 3), dtype=np.float32)
    d2, idx = nn_sqdist(a, b, return_ind=True)
    assert np.all(idx.cpu().numpy() == 17) and np.all(d2.cpu().numpy() == 0.25)


def test_nn_rejects_empty_target():
    from slice3d_amd._lib import S3dError
    from slice3d_amd.mesh_eval import nn_sqdist, points_dist
    with pytest.raises(S3dError):
        nn_sqdist(np.zeros((3, 3), np.float32), np.zeros((0, 3), np.float32))
    assert points_dist(np.zeros((0, 3)), np.ones((2, 3))).shape == (0,)


@pytest.mark.parametrize("k", [0, 1])
def test_chamfer_and_hausdorff_match_reference(gold, k):
    from slice3d_amd.mesh_eval import eval_chamfer, eval_hausdoff
    p1, p2 = gold["cd%d_p1" % k], gold["cd%d_p2" % k]
    ours = eval_chamfer(torch.from_numpy(p1).cuda(), torch.from_numpy(p2).cuda(), f_thresh=0.05)
    ref = gold["cd%d_chamfer" % k]
    for i in (0, 1, 3, 4):
        assert ours[i] == pytest.approx(ref[i], rel=1e-5)
    p, r = ours[3], ours[4]
    assert ours[2] == pytest.approx(2 * p * r / (p + r), rel=1e-12)
    assert np.allclose(eval_hausdoff(p1, p2), gold["cd%d_hausdorff" % k], rtol=1e-5, atol=0)


# ---------------------------------------------------------------------------------------------- surface sampling
def _mc_sphere():
    from slice3d_amd.mesh import marching_cubes_device
    g = torch.linspace(-1, 1, 65, dtype=torch.float64, device="cuda")
    x, y, z = torch.meshgrid(g, g, g, indexing="ij")
    v, f = marching_cubes_device(0.6 - torch.sqrt(x ** 2 + y ** 2 + z ** 2), 0.0)
    return v * (2.0 / 64) - 1.0, f


def _height_field_mesh(n=8):
    """n x n unit squares over [-n/2, n/2]^2, two triangles each, z = 0.3 sin(x) cos(y): well-shaped faces of unit size,
    so float32 rounding of a sample moves its barycentric coordinates by ~1e-7 at most."""
    g = np.arange(n + 1, dtype=np.float64) - n / 2
    x, y = np.meshgrid(g, g, indexing="ij")
    V = np.stack([x, y, 0.3 * np.sin(x) * np.cos(y)], -1).reshape(-1, 3)
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    a = (i * (n + 1) + j).ravel()
    F = np.concatenate([np.stack([a, a + n + 1, a + 1], 1), np.stack([a + 1, a + n + 1, a + n + 2], 1)])
    return V, F


def test_samples_lie_on_their_faces():
    from slice3d_amd.mesh_eval import sample_surface
    V, F = _height_field_mesh()
    pts, fi = sample_surface((torch.from_numpy(V).cuda(), torch.from_numpy(F).cuda()), 200000, seed=3)
    assert pts.is_cuda and pts.dtype == torch.float32 and fi.dtype == torch.int64
    pts, fi = pts.cpu().numpy().astype(np.float64), fi.cpu().numpy()
    tri = V[F[fi]]
    a, b, c = tri[:, 0], tri[:, 1], tri[:, 2]
    e0, e1, e2 = b - a, c - a, pts - a
    d00, d01, d11 = (e0 * e0).sum(1), (e0 * e1).sum(1), (e1 * e1).sum(1)
    d20, d21 = (e2 * e0).sum(1), (e2 * e1).sum(1)
    den = d00 * d11 - d01 * d01
    wb = (d11 * d20 - d01 * d21) / den
    wc = (d00 * d21 - d01 * d20) / den
    wa = 1 - wb - wc
    assert min(wa.min(), wb.min(), wc.min()) >= -1e-6
    assert np.allclose(wa + wb + wc, 1.0, rtol=0, atol=1e-12)
    n = np.cross(e0, e1)
    assert (np.abs((e2 * n).sum(1)) / np.linalg.norm(n, axis=1)).max() < 1e-6      # on the face's plane
    assert len(np.unique(fi)) == len(F)


def test_sampling_is_seeded():
    from slice3d_amd.mesh_eval import sample_surface
    v, f = _mc_sphere()
    p1, f1 = sample_surface((v, f), 50000, seed=7)
    p2, f2 = sample_surface((v, f), 50000, seed=7)
    p3, _ = sample_surface((v, f), 50000, seed=8)
    assert torch.equal(p1.view(torch.int32), p2.view(torch.int32)) and torch.equal(f1, f2)
    assert (p1 != p3).any(dim=1).float().mean() > 0.99
    # the first n samples do not depend on how many are drawn
    p4, _ = sample_surface((v, f), 1000, seed=7)
    assert torch.equal(p4, p1[:1000])


def test_sampling_follows_area_and_skips_zero_area():
    from slice3d_amd.mesh_eval import sample_surface
    # faces: area 0, area 1, area 0 (collinear), area 3, area 0 (repeated vertex)
    V = np.array([[0, 0, 0], [1, 0, 0], [0, 2, 0], [0, 0, 1], [3, 0, 1], [0, 2, 1], [2, 0, 0], [5, 5, 5]], np.float64)
    F = np.array([[0, 1, 6], [0, 1, 2], [0, 1, 6], [3, 4, 5], [7, 7, 3]], np.int64)
    pts, fi = sample_surface((V, F), 10 ** 6, seed=1)
    counts = np.bincount(fi, minlength=5)
    assert counts[0] == counts[2] == counts[4] == 0
    assert abs(counts[1] / 1e6 - 0.25) < 0.002
    # a zero-area face on every tile and thread boundary of the device scan
    nf = 3 * 4096 + 5
    F2 = np.tile(np.array([[0, 1, 2]], np.int64), (nf, 1))
    F2[::16] = [0, 1, 6]
    _, fi2 = sample_surface((V, F2), 200000, seed=2)
    assert not np.any(fi2 % 16 == 0)


# ---------------------------------------------------------------------------------------------- end to end
def _sphere_mesh(radius, n=97):
    from slice3d_amd.mesh import marching_cubes
    g = np.stack(np.meshgrid(*[np.linspace(-0.5, 0.5, n)] * 3, indexing="ij"), -1)
    v, f = marching_cubes(radius - np.linalg.norm(g, axis=-1), 0.0)
    return v * (1.0 / (n - 1)) - 0.5, f


def test_eval_meshes_end_to_end(tmp_path):
    import pickle
    from slice3d_amd.datasets import write_toy_dataset
    from slice3d_amd.mesh import Mesh
    from slice3d_amd.mesh_eval import compute_iou, load_obj
    shapes = ("shape_a", "shape_b")
    write_toy_dataset(str(tmp_path), "custom", shapes=shapes, n_pts=500, seed=4)
    base = tmp_path / "custom"
    res, gt = tmp_path / "results", tmp_path / "gt"
    res.mkdir()
    gt.mkdir()
    v0, f0 = _sphere_mesh(0.3)
    expected, areas = {}, {}
    for sh in shapes:
        with open(base / "00_img_input" / sh / "meta.pkl", "rb") as fh:
            meta = pickle.load(fh)
        scale, off = meta[5], meta[6]
        shift = np.array([off[0], off[2], -off[1]])
        vq = v0 * scale + shift                                    # the dataset's map (datasets.py:143)
        Mesh(vq, f0).export(str(res / (sh + ".obj")))
        Mesh((vq - shift) / scale, f0).export(str(gt / (sh + ".obj")))   # its inverse: the SDF frame
        sdf = np.load(base / "02_sdfs" / (sh + ".npy"))
        qry = (sdf[:, :3] * scale + shift).astype(np.float32)     # n_qry = all 500 points, order irrelevant to IoU
        occ = ((sdf[:, 3] - 0.003) * scale <= 0).astype(np.float32)
        m = load_obj(str(res / (sh + ".obj")))
        expected[sh] = float(compute_iou(mesh_eval_ref.contains(m.vertices, m.faces, qry)[0], occ))
        t = vq[f0]
        areas[sh] = 0.5 * np.linalg.norm(np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]), axis=1).sum()
    cmd = [sys.executable, os.path.join(ROOT, "reg_slices", "eval_meshes.py"), "--dir_data", str(tmp_path),
           "--name_dataset", "custom", "--n_views", "6", "--n_qry", "500", "--dir_results", str(res),
           "--dir_gt_meshes", str(gt)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout + r.stderr
    summary = json.loads(r.stdout.strip().splitlines()[-1])
    assert summary["n_shapes"] == 2 and summary["missing"] == 0 and summary["undefined_iou"] == 0
    with open(res / "eval.csv") as fh:
        rows = {row["shape"]: row for row in csv.DictReader(fh)}
    n = 100000
    for sh in shapes:
        row = rows[sh]
        assert float(row["iou"]) == pytest.approx(expected[sh], rel=0, abs=1e-7)
        assert float(row["fscore"]) > 0.99
        # two independent samplings of one surface: the mean nearest-neighbour distance stays below the spacing
        # sqrt(area / n) of n samples (for uniform points it is about half of it)
        assert float(row["chamfer_L1"]) < np.sqrt(areas[sh] / n)
    # no mesh at all: exit status 1
    r = subprocess.run(cmd[:-4] + ["--dir_results", str(tmp_path / "none")], capture_output=True, text=True, timeout=300,
                       cwd=ROOT)
    assert r.returncode == 1

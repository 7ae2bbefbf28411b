"""GPU tests of the mesh simplifier (csrc/mesh_simplify.hip) through slice3d_amd/mesh_simplify.py: topology, face-count
window and orientation on the fixtures, the error against the reference's recorded outputs (measured on both sides by
slice3d_amd.mesh_sdf.MeshDistance), a mesh that crosses scan tiles, determinism, borders, degenerate input, the argument
checks, and reconstruct.py --simplify_nfaces / simplify_meshes.py end to end.

E(A, B) = max over A's referenced vertices and face centroids of the distance to B, and the same from B to A, the larger
of the two over the bounding-box diagonal of the input (tests/simplify_ref.py).  The bound of the error tests is
E(input, ours at T) <= E(input, reference at floor(T / 2)): independent sets are not the reference's collapse order, and
half its face budget is the most that may cost.  Measured on the MI355X (ours / bound): sphere 0.50, 0.46, 0.54 at 50,
25, 10 %; torus 0.37, 0.61, 0.47; boxes at 10 % 0.17; the 64^3 genus-1 mesh at 10 % 0.63."""
import ctypes as C
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import simplify_cases as sc
import simplify_ref as sr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dist(v, f, p):
    from slice3d_amd.mesh_sdf import MeshDistance
    return MeshDistance((v, f)).query(p)


@functools.lru_cache(maxsize=None)
def _ours(name, t):
    """(vertices, faces, rounds) of `name` simplified to `t` at the reference's aggressiveness, computed once."""
    from slice3d_amd.mesh_simplify import simplify_stats
    v, f = sc.mesh(name)
    return simplify_stats(v, f, t, sc.AGGRESSIVENESS)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _check_error(name, t):
    v, f = sc.mesh(name)
    vo, fo, rounds = _ours(name, t)
    diag = sr.bbox_diagonal(v, f)
    e = sr.mesh_error((v, f), (vo, fo), diag, _dist)
    bound = sr.mesh_error((v, f), sc.reference(name, t // 2), diag, _dist)
    print("%s T = %d: %d faces after %d rounds, E(input, ours) = %.3e, E(input, reference at T / 2) = %.3e, ratio %.2f"
          % (name, t, len(fo), rounds, e, bound, e / bound))
    assert e <= bound


# ---------------------------------------------------------------------------------------------- 1: topology and count
@pytest.mark.parametrize("ratio", sc.RATIOS)
@pytest.mark.parametrize("name", sc.CLOSED)
def test_closed_fixtures_stay_closed_oriented_manifolds(name, ratio):
    v, f = sc.mesh(name)
    t = sc.target(name, ratio)
    vo, fo, rounds = _ours(name, t)
    assert vo.dtype == np.float64 and fo.dtype == np.int64 and np.isfinite(vo).all()
    print("%s %d %%: T = %d -> %d faces, %d vertices, %d rounds" % (name, ratio, t, len(fo), len(vo), rounds))
    assert sr.check_closed_result(v, f, vo, fo, t) == []


# ---------------------------------------------------------------------------------------------- 2: error
@pytest.mark.parametrize("name,ratio", sc.ERROR_CASES)
def test_error_within_the_reference_at_half_the_budget(name, ratio):
    _check_error(name, sc.target(name, ratio))


# ---------------------------------------------------------------------------------------------- 3: across scan tiles
@functools.lru_cache(maxsize=None)
def _genus1_device():
    from slice3d_amd.mesh import marching_cubes_device
    vol = torch.from_numpy(sc.genus1_field()).cuda()
    v, f = marching_cubes_device(vol, 0.0, pad_value=-1e6)
    return (v - 1.0) * (2.0 / (sc.GENUS1_RES - 1)) - 1.0, f


def test_marching_cubes_mesh_across_scan_tiles():
    """Device marching cubes of the 64^3 genus-1 field (the mesh as s3d_mc_dev_emit leaves it, tens of thousands of faces
    against a scan tile of 4 096) simplified to 10 %: the conditions of items 1 and 2 against the golden made from the
    bit-identical host mesh."""
    from slice3d_amd.mesh_simplify import mesh_simplify
    vd, fd = _genus1_device()
    v, f = sc.mesh("genus1")
    assert np.array_equal(fd.cpu().numpy(), f) and np.array_equal(_bits(vd.cpu().numpy()), _bits(v))
    assert len(f) >= 20000
    t = sc.target("genus1", sc.GENUS1_RATIO)
    vo, fo = mesh_simplify(vd, fd, t, sc.AGGRESSIVENESS)
    assert vo.is_cuda and fo.is_cuda and vo.dtype == torch.float64 and fo.dtype == torch.int64
    hv, hf, _ = _ours("genus1", t)                       # numpy in
    assert np.array_equal(fo.cpu().numpy(), hf) and np.array_equal(_bits(vo.cpu().numpy()), _bits(hv))
    assert sr.check_closed_result(v, f, hv, hf, t) == []
    _check_error("genus1", t)


# ---------------------------------------------------------------------------------------------- 4: determinism
def test_two_runs_give_the_same_bits():
    from slice3d_amd.mesh_simplify import simplify_stats
    v, f = sc.mesh("genus1")
    t = sc.target("genus1", sc.GENUS1_RATIO)
    a = _ours("genus1", t)
    b = simplify_stats(v, f, t, sc.AGGRESSIVENESS)
    assert a[2] == b[2] and np.array_equal(a[1], b[1]) and np.array_equal(_bits(a[0]), _bits(b[0]))


# ---------------------------------------------------------------------------------------------- 5: borders
def test_open_mesh_keeps_its_border():
    v, f = sc.mesh("open_sphere")
    t = sc.target("open_sphere", sc.OPEN_RATIO)
    vo, fo, rounds = _ours("open_sphere", t)
    print("open_sphere: T = %d -> %d faces, %d rounds" % (t, len(fo), rounds))
    assert sr.indices_valid(vo, fo) and sr.no_repeated_index(fo) and t - 2 <= len(fo) <= t
    _, c = sr.edge_face_counts(fo)
    assert np.all((c == 1) | (c == 2)) and sr.is_oriented_manifold(fo, closed=False)
    assert sr.boundary_loops(f) == 1 and sr.boundary_loops(fo) == 1
    assert sr.euler_characteristic(fo) == sr.euler_characteristic(f)
    # every output border vertex within the bound of item 2 of the input's border polyline
    diag = sr.bbox_diagonal(v, f)
    bound = sr.mesh_error((v, f), sc.reference("open_sphere", t // 2), diag, _dist)
    d = sr._directed(f)
    _, inv, cnt = np.unique(np.sort(d, axis=1), axis=0, return_inverse=True, return_counts=True)
    seg = d[cnt[inv.reshape(-1)] == 1]
    a, b, p = v[seg[:, 0]][None], v[seg[:, 1]][None], vo[sr.border_vertices(fo)][:, None]
    u = np.clip(((p - a) * (b - a)).sum(-1) / ((b - a) ** 2).sum(-1), 0.0, 1.0)
    dist = np.linalg.norm(p - (a + u[..., None] * (b - a)), axis=-1).min(axis=1)     # point to nearest border segment
    print("open_sphere: max border distance / diagonal = %.3e, bound %.3e" % (dist.max() / diag, bound))
    assert dist.max() / diag <= bound


# ---------------------------------------------------------------------------------------------- 6: degenerate input
@pytest.mark.parametrize("name", ["zero_area", "flat"])
def test_degenerate_fixtures_terminate_with_valid_meshes(name):
    from slice3d_amd.mesh_simplify import simplify_stats
    v, f = sc.mesh(name)
    vo, fo, rounds = simplify_stats(v, f, len(f) // 2, sc.AGGRESSIVENESS)
    print("%s: %d -> %d faces, %d rounds" % (name, len(f), len(fo), rounds))
    assert rounds <= 100 and np.isfinite(vo).all() and len(fo) <= len(f)
    assert sr.indices_valid(vo, fo) and sr.no_repeated_index(fo)


def test_tetrahedron_and_octahedron():
    from slice3d_amd.mesh_simplify import mesh_simplify
    v, f = sc.mesh("tetrahedron")
    vo, fo = mesh_simplify(v, f, 2, sc.AGGRESSIVENESS)      # no legal collapse exists
    assert len(fo) == 4 and np.array_equal(fo, f) and np.array_equal(_bits(vo), _bits(v))
    v, f = sc.mesh("octahedron")
    vo, fo = mesh_simplify(v, f, 4, sc.AGGRESSIVENESS)
    assert len(fo) <= 8 and sr.is_oriented_manifold(fo) and sr.indices_valid(vo, fo) and sr.no_repeated_index(fo)
    assert sr.signed_volume(vo, fo) > 0


# ---------------------------------------------------------------------------------------------- 7: arguments
def test_argument_checks():
    from slice3d_amd import _lib as L
    from slice3d_amd.mesh import Mesh
    from slice3d_amd.mesh_simplify import mesh_simplify, simplify_mesh
    lib = L.load()
    v, f = sc.mesh("octahedron")
    vd, fd = torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda()
    nb = lib.s3d_mesh_simplify_workspace_bytes(len(v), len(f))
    assert nb > 0 and lib.s3d_mesh_simplify_workspace_bytes(len(v), 0) == 0
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    nvo, nfo, nr = C.c_long(0), C.c_long(0), C.c_int(0)
    st = L.stream_ptr(vd.device)

    def run(faces, n_faces, target, n_bytes):
        return lib.s3d_mesh_simplify_run(vd.data_ptr(), len(v), faces.data_ptr(), n_faces, target, 5.0, ws.data_ptr(),
                                         n_bytes, C.byref(nvo), C.byref(nfo), C.byref(nr), st)

    for bad_index in (6, -1):
        fb = fd.clone()
        fb[3, 1] = bad_index
        assert run(fb, len(f), 4, nb) == -1 and b"outside" in lib.s3d_last_error()
    assert run(fd, 0, 4, nb) == -1 and b"no face" in lib.s3d_last_error()
    assert run(fd, len(f), -1, nb) == -1 and b"target_faces" in lib.s3d_last_error()
    assert run(fd, len(f), 4, nb - 1) == -1 and b"workspace" in lib.s3d_last_error()
    out = torch.empty((8, 3), dtype=torch.int64, device="cuda")
    assert lib.s3d_mesh_simplify_emit(ws.data_ptr(), nb - 1, len(v), len(f), vd.data_ptr(), out.data_ptr(), st) == -1
    torch.cuda.synchronize()
    # T >= n_faces: the input, bit for bit
    for name in ("octahedron", "sphere"):
        v, f = sc.mesh(name)
        for t in (len(f), len(f) + 5):
            vo, fo = mesh_simplify(v, f, t)
            assert np.array_equal(fo, f) and np.array_equal(_bits(vo), _bits(v))
    empty = Mesh(np.zeros((0, 3)), np.zeros((0, 3), dtype=np.int64))
    assert simplify_mesh(empty, 10) is empty
    m = simplify_mesh(Mesh(*sc.mesh("sphere")), sc.target("sphere", 50), sc.AGGRESSIVENESS)
    hv, hf, _ = _ours("sphere", sc.target("sphere", 50))
    assert isinstance(m, Mesh) and np.array_equal(m.faces, hf) and np.array_equal(_bits(m.vertices), _bits(hv))


# ---------------------------------------------------------------------------------------------- 8: end to end
def _run(cmd, cwd):
    r = subprocess.run([sys.executable] + cmd, cwd=cwd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout


RECON = ["--name_dataset", "synthetic", "--synthetic_len", "1", "--img_size", "64", "--mode", "test", "--mc_res0", "16",
         "--mc_up_steps", "2", "--name_ckpt", "none.ckpt", "--synthetic_weights", "--overwrite_res"]
N_FACES = 10000      # libsimplify's default f_target; the extracted mesh has about 50 000 faces


def test_reconstruct_with_and_without_simplify_nfaces(tmp_path):
    """reconstruct.py at test_gpu_mesh.py's scaled-down options (MISE 16 -> 64): without the flag the file is what
    Generator3D.generate_mesh exports, twice; with it the file has <= N faces and eval_meshes.py reads it."""
    sys.path.insert(0, os.path.join(ROOT, "reg_slices"))
    from options import get_parser
    from slice3d_amd.datasets import write_toy_dataset
    from slice3d_amd.generator import Generator3D
    from slice3d_amd.mesh_eval import load_obj
    from slice3d_amd.models import Slices3DRegModel
    from slice3d_amd.synth import SyntheticSlice3DDataset
    from slice3d_amd.weights import load_seeded
    script = os.path.join(ROOT, "reg_slices", "reconstruct.py")
    plain = []
    for exp in ("plain_a", "plain_b"):
        _run([script, "--name_exp", exp] + RECON, str(tmp_path))
        with open(tmp_path / "experiments" / exp / "results" / "synthetic" / "synthetic_0000.obj", "rb") as fh:
            plain.append(fh.read())
    args = get_parser().parse_args(RECON)
    assert args.simplify_nfaces is None
    model = load_seeded(Slices3DRegModel(img_size=args.img_size, n_slices=args.n_slices, mode="test"), 0).cuda().eval()
    gen = Generator3D(model, threshold=args.mc_threshold, resolution0=args.mc_res0, upsampling_steps=args.mc_up_steps,
                      chunk_size=args.mc_chunk_size, pred_type=args.pred_type)
    item = SyntheticSlice3DDataset(1, args.img_size, 16, args.n_slices, split="test")[0]
    with torch.no_grad():
        mesh, _ = gen.generate_mesh({k: x.unsqueeze(0).cuda() for k, x in item.items()})
    mesh.export(str(tmp_path / "direct.obj"))
    with open(tmp_path / "direct.obj", "rb") as fh:
        direct = fh.read()
    assert len(mesh.faces) > N_FACES, "the unsimplified mesh must be larger than the target for this test to mean anything"
    assert plain[0] == direct and plain[1] == direct
    out = _run([script, "--name_exp", "simp", "--simplify_nfaces", str(N_FACES)] + RECON, str(tmp_path))
    assert "time (simplify)" in out
    res = tmp_path / "experiments" / "simp" / "results" / "synthetic"
    small = load_obj(str(res / "synthetic_0000.obj"))
    print("reconstruct.py: %d faces -> %d" % (len(mesh.faces), len(small.faces)))
    assert 0 < len(small.faces) <= N_FACES and sr.indices_valid(small.vertices, small.faces)
    # eval_meshes.py scores that file (against a toy dataset that has a shape of its name)
    write_toy_dataset(str(tmp_path / "data"), "custom", shapes=("synthetic_0000",), n_pts=500, seed=4)
    out = _run([os.path.join(ROOT, "reg_slices", "eval_meshes.py"), "--dir_data", str(tmp_path / "data"), "--name_dataset",
                "custom", "--n_views", "6", "--n_qry", "500", "--dir_results", str(res)], str(tmp_path))
    summary = json.loads(out.strip().splitlines()[-1])
    assert summary["n_shapes"] == 1 and summary["missing"] == 0


def test_simplify_meshes_processes_a_directory(tmp_path):
    from slice3d_amd.mesh import Mesh
    from slice3d_amd.mesh_eval import load_obj
    src, dst = tmp_path / "in", tmp_path / "out"
    src.mkdir()
    for name in ("sphere", "torus"):
        Mesh(*sc.mesh(name)).export(str(src / (name + ".obj")))
    script = os.path.join(ROOT, "reg_slices", "simplify_meshes.py")
    out = _run([script, "--dir_meshes", str(src), "--dir_out", str(dst), "--ratio", "0.25"], str(tmp_path))
    summary = json.loads(out.strip().splitlines()[-1])
    assert summary["n_meshes"] == 2
    for row in summary["meshes"]:
        name = row["mesh"][:-4]
        t = int(len(sc.mesh(name)[1]) * 0.25)
        m = load_obj(str(dst / row["mesh"]))
        assert row["faces_in"] == len(sc.mesh(name)[1]) and row["faces_out"] == len(m.faces)
        assert t - 2 <= len(m.faces) <= t and row["rounds"] >= 1 and row["seconds"] > 0
        assert sr.is_oriented_manifold(m.faces) and sr.indices_valid(m.vertices, m.faces)
    r = subprocess.run([sys.executable, script, "--dir_meshes", str(src), "--dir_out", str(dst)], capture_output=True, text=True)
    assert r.returncode != 0                                # one of --n_faces / --ratio is required

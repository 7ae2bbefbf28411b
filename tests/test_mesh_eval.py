"""CPU tests of the mesh scoring (slice3d_amd/mesh_eval.py): the host restatement (tests/mesh_eval_ref.py) against the
reference's own point-in-mesh output, .obj round trip, the F-score formula, and the evaluation script's flags.
Goldens: tests/golden/mesh_eval_reference.npz (tests/golden/make_golden_mesh_eval.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import GOLDEN
import mesh_eval_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["sphere", "torus", "boxes", "zero_area", "flat"]


@pytest.fixture(scope="module")
def gold():
    z = np.load(os.path.join(GOLDEN, "mesh_eval_reference.npz"))
    return {k: z[k] for k in z.files}


@pytest.mark.parametrize("name", CASES)
def test_restatement_equals_reference_contains(gold, name):
    inside, _ = mesh_eval_ref.contains(gold[name + "_v"], gold[name + "_f"], gold[name + "_pts"])
    assert np.array_equal(inside, gold[name + "_contains"])


def test_restatement_float32_points(gold):
    inside, _ = mesh_eval_ref.contains(gold["sphere_v"], gold["sphere_f"], gold["sphere_pts32"])
    assert np.array_equal(inside, gold["sphere_contains32"])


def test_golden_cases_cover_the_edges(gold):
    """The crafted points reach the branches the bit-exactness is about: parity disagreements, points on cell
    boundaries and at res, and nothing inside a flat mesh."""
    n_dis = sum(mesh_eval_ref.contains(gold[c + "_v"], gold[c + "_f"], gold[c + "_pts"])[1] for c in CASES)
    assert n_dis > 0
    assert not gold["flat_contains"].any()
    for c in CASES[:4]:
        assert 0 < gold[c + "_contains"].sum() < len(gold[c + "_pts"])


def test_compute_iou_matches_reference(gold):
    from slice3d_amd.mesh_eval import compute_iou
    iou = compute_iou(gold["iou_occ1"], gold["iou_occ2"])
    assert np.array_equal(np.isnan(iou), np.isnan(gold["iou"])) and np.isnan(iou[2])
    assert np.array_equal(iou[:2], gold["iou"][:2])


def test_eval_iou_empty_mesh_is_zero():
    from slice3d_amd.mesh import Mesh
    from slice3d_amd.mesh_eval import eval_iou
    assert eval_iou(Mesh(np.zeros((0, 3)), np.zeros((0, 3))), np.zeros((5, 3)), np.ones(5)) == 0.0


def test_reference_fscore_is_four_precision(gold):
    """utils_eval.py:85 computes 2 * (recall * precision / recall + precision) = 4 * precision; ours is 2PR/(P+R)."""
    from slice3d_amd import mesh_eval
    for k in (0, 1):
        cl1, cl2, f, p, r = gold["cd%d_chamfer" % k]
        assert 0 < p < 1 and 0 < r < 1
        assert np.isclose(f, 4 * p, rtol=1e-12)
        assert not np.isclose(f, 2 * p * r / (p + r))
    assert "2PR/(P+R)" in mesh_eval.eval_chamfer.__doc__ and "utils_eval.py:85" in mesh_eval.eval_chamfer.__doc__


def test_fscore_is_harmonic_mean(monkeypatch):
    """eval_chamfer's F-score from given precision / recall (the distances come from the device; stubbed here)."""
    import torch
    from slice3d_amd import mesh_eval

    def fake(p1, p2, return_ind=False):
        return torch.as_tensor(np.asarray(p1)[:, 0] ** 2, dtype=torch.float32)
    monkeypatch.setattr(mesh_eval, "nn_sqdist", fake)
    a = np.array([[0.0, 0, 0], [0.0, 0, 0], [0.0, 0, 0], [1.0, 0, 0]])   # precision 3/4
    b = np.array([[0.0, 0, 0], [1.0, 0, 0]])                             # recall 1/2
    cl1, cl2, f, p, r = mesh_eval.eval_chamfer(a, b, f_thresh=0.5)
    assert (p, r) == (0.75, 0.5) and f == pytest.approx(2 * 0.75 * 0.5 / 1.25, rel=1e-15)
    far = np.ones((3, 3))
    assert mesh_eval.eval_chamfer(far, far, f_thresh=0.5)[2] == 0.0


def test_points_dist_rejects_k():
    from slice3d_amd.mesh_eval import points_dist
    with pytest.raises(ValueError):
        points_dist(np.zeros((2, 3)), np.zeros((2, 3)), k=2)


def test_load_obj_round_trips_export(tmp_path, gold):
    from slice3d_amd.mesh import Mesh
    from slice3d_amd.mesh_eval import load_obj
    m = Mesh(gold["torus_v"], gold["torus_f"])
    back = load_obj(m.export(str(tmp_path / "t.obj")))
    assert np.array_equal(back.faces, m.faces)
    assert np.allclose(back.vertices, m.vertices, rtol=0, atol=1e-8)


def test_load_obj_fan_triangulates(tmp_path):
    from slice3d_amd.mesh_eval import load_obj
    p = tmp_path / "q.obj"
    p.write_text("# quad and pentagon\nv 0 0 0\nv 1 0 0\nv 1 1 0\nv 0 1 0\nv 0.5 1.5 0\nvn 0 0 1\n"
                 "f 1/1/1 2/2/1 3/3/1 4/4/1\nf 1 2 3 5 4\nf -3 -2 -1\n")
    m = load_obj(str(p))
    assert m.vertices.shape == (5, 3)
    assert m.faces.tolist() == [[0, 1, 2], [0, 2, 3], [0, 1, 2], [0, 2, 4], [0, 4, 3], [2, 3, 4]]


def test_nn_brute_lowest_index_on_ties():
    d, idx, d2nd = mesh_eval_ref.nn_brute(np.zeros((1, 3)), np.array([[1.0, 0, 0], [0, 1.0, 0], [2.0, 0, 0]]))
    assert d[0] == 1.0 and idx[0] == 0 and d2nd[0] == 1.0


def test_eval_meshes_help_parses():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "reg_slices", "eval_meshes.py"), "--help"],
                       capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert r.returncode == 0, r.stderr
    for flag in ("--dir_results", "--dir_gt_meshes", "--n_surface_points", "--f_thresh", "--eval_seed"):
        assert flag in r.stdout


def test_contains_kernels_hold_no_fused_f64(tmp_path):
    """mesh_eval.hip as the Makefile compiles it: the rescale, cell-list and contains kernels hold no v_fma_f64 (a fused
    multiply-add would move points across cell and triangle edges) and use no scratch."""
    import re
    src = os.path.join(ROOT, "slice3d_amd", "csrc", "mesh_eval.hip")
    out = str(tmp_path / "me.s")
    r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "--cuda-device-only",
                        "-S", src, "-o", out, "-Rpass-analysis=kernel-resource-usage"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert "-ffp-contract=off" in open(os.path.join(ROOT, "slice3d_amd", "csrc", "Makefile")).read()
    scratch = re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)
    assert scratch and all(x == "0" for x in scratch)
    asm = open(out).read()
    bodies = re.findall(r"^(_Z\w+):(.*?)\.Lfunc_end", asm, re.S | re.M)
    names = [n for n, _ in bodies if re.search("me_(rescale_count|fill|contains)_kernel", n)]
    assert len(names) == 4, names
    for name, body in bodies:
        if name in names:
            assert "v_fma_f64" not in body and "v_fmac_f64" not in body, name

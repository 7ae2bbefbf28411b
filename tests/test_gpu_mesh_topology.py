"""GPU tests of the mesh-topology unit (csrc/mesh_topology.hip) through slice3d_amd/mesh_topology.py against the numpy
references of tests/topology_ref.py: labels, the per-component table and the summary on the fixtures, a long strip (the
round bound), a high-valence fan and sizes around a block and a scan tile, weld, the argument checks, non-manifold
meshes, keep, a marching-cubes mesh, and the three scripts end to end.

Integer outputs are compared with array_equal.  Area and volume are held to (n + 16) 2^-52 sum|term| for a row of n faces,
a term being a face's area and its det(v0, v1, v2) / 6: n roundings of the running sum in either summation order plus a few
ulps of each term.  The bound is derived, not measured; the assert messages print the observed maximum over the bound."""
import ctypes as C
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import sdf_cases
import simplify_cases as sc
import simplify_ref as sr
import topology_ref as tr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = ["sphere", "torus", "boxes", "zero_area", "flat"]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


@functools.lru_cache(maxsize=None)
def _fixture_ref(name):
    return tr.topology(*sc.mesh(name))


def _compare(topo, ref, what):
    """labels, table and summary of a MeshTopology against tr.topology's dict"""
    assert topo.n_components == ref["n_components"], what
    assert np.array_equal(topo.vmap, ref["vmap"]), what
    assert np.array_equal(topo.face_component, ref["face_component"]), what
    assert np.array_equal(topo.vertex_component, ref["vertex_component"]), what
    for name in tr.COUNT_COLUMNS:
        assert np.array_equal(topo.table[name], ref["table"][name]), (what, name, topo.table[name], ref["table"][name])
        assert topo.summary[name] == ref["summary"][name], (what, name, topo.summary[name], ref["summary"][name])
    k = topo.n_components
    got = np.stack([np.append(topo.table["area"], topo.summary["area"]), np.append(topo.table["volume"], topo.summary["volume"])], 1)
    want = np.stack([np.append(ref["table"]["area"], ref["summary"]["area"]),
                     np.append(ref["table"]["volume"], ref["summary"]["volume"])], 1)
    err = np.abs(got - want)
    ratio = float((err / np.where(ref["tol"] > 0, ref["tol"], 1.0)).max()) if err.size else 0.0
    print("%s: %d components, max |area, volume error| / bound = %.3f" % (what, k, ratio))
    assert np.all(err <= ref["tol"]), "%s: area / volume error over its bound by a factor of up to %.3f" % (what, ratio)
    if len(ref["face_component"]):
        assert np.array_equal(topo.table["bbox"], ref["table"]["bbox"]) and np.array_equal(topo.summary["bbox"], ref["summary"]["bbox"])


def _same_bits(a, b):
    """everything but the round count, which may depend on how far a hook launch saw the others' labels"""
    assert a.n_components == b.n_components
    for x, y in ((a.vmap, b.vmap), (a.face_component, b.face_component), (a.vertex_component, b.vertex_component)):
        x, y = (t.cpu().numpy() if isinstance(t, torch.Tensor) else t for t in (x, y))
        assert np.array_equal(x, y)
    for name in list(tr.COUNT_COLUMNS):
        assert np.array_equal(a.table[name], b.table[name]) and a.summary[name] == b.summary[name]
    for name in ("area", "volume", "bbox"):
        assert np.array_equal(_bits(a.table[name]), _bits(b.table[name]))
        assert np.array_equal(_bits(a.summary[name]), _bits(b.summary[name]))


# ---------------------------------------------------------------------------------------------- 1: fixtures
@pytest.mark.parametrize("name", FIXTURES)
def test_fixtures_labels_table_summary_and_bits(name):
    from slice3d_amd.mesh_topology import mesh_topology
    v, f = sc.mesh(name)
    a = mesh_topology((v, f))
    _compare(a, _fixture_ref(name), name)
    _same_bits(a, mesh_topology((v, f)))                                       # two runs
    d = mesh_topology((torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda()))     # device input
    assert d.face_component.is_cuda and d.vertex_component.is_cuda and d.face_component.dtype == torch.int64
    _same_bits(a, d)
    closed = name in sc.CLOSED
    assert a.is_watertight == closed


# ---------------------------------------------------------------------------------------------- 2: diameter
@pytest.mark.parametrize("cuts", [0, 7])
def test_long_strip_within_the_round_bound(cuts):
    """A plain min-label propagation needs a round per unit of diameter (thousands here); hooking and pointer jumping a
    few.  The bound of 64 rounds is the library's: exceeding it is an error code."""
    from slice3d_amd.mesh_topology import mesh_topology
    v, f = tr.strip(20000, 11, cuts)
    topo = mesh_topology((v, f))
    print("strip of %d faces, %d cuts: %d components in %d rounds" % (len(f), cuts, topo.n_components, topo.rounds))
    assert topo.n_components == cuts + 1 and 1 <= topo.rounds <= 64
    _compare(topo, tr.topology(v, f), "strip")


# ---------------------------------------------------------------------------------------------- 3: valence, tile edges
def test_fan_of_4096_faces():
    from slice3d_amd.mesh_topology import mesh_topology
    n = 4096
    a = 2 * np.pi * np.arange(n) / n
    v = np.concatenate([[[0.0, 0, 0.5]], np.stack([np.cos(a), np.sin(a), np.zeros(n)], 1)])
    f = np.stack([np.zeros(n, dtype=np.int64), 1 + np.arange(n), 1 + (np.arange(n) + 1) % n], 1)
    topo = mesh_topology((v, f))
    _compare(topo, tr.topology(v, f), "fan")
    assert topo.summary["edges_1"] == n and topo.summary["edges_2"] == n and topo.summary["oriented_with_border"]


def _mix(n_faces, seed):
    """disjoint single triangles and pairs of triangles on a shared edge, vertices renumbered at random"""
    rng = np.random.default_rng(seed)
    faces, nv = [], 0
    while len(faces) < n_faces:
        if n_faces - len(faces) >= 2 and rng.random() < 0.5:
            faces += [[nv, nv + 1, nv + 2], [nv + 2, nv + 1, nv + 3]]
            nv += 4
        else:
            faces.append([nv, nv + 1, nv + 2])
            nv += 3
    pv = rng.permutation(nv)
    return rng.normal(size=(nv, 3)), pv[np.array(faces, dtype=np.int64)]


@pytest.mark.parametrize("n_faces", [1, 255, 256, 257, 4095, 4096, 4097])
def test_sizes_around_a_block_and_a_scan_tile(n_faces):
    from slice3d_amd.mesh_topology import mesh_topology
    v, f = _mix(n_faces, n_faces)
    topo = mesh_topology((v, f))
    ref = tr.topology(v, f)
    _compare(topo, ref, "mix of %d faces" % n_faces)
    mask = np.arange(topo.n_components) % 3 != 1
    vo, fo = topo._run.keep(mask)
    rv, rf = tr.keep(v, f, ref["face_component"], mask)
    assert np.array_equal(fo.cpu().numpy(), rf) and np.array_equal(_bits(vo.cpu().numpy()), _bits(rv))


# ---------------------------------------------------------------------------------------------- 4: weld
@pytest.mark.parametrize("name", sc.CLOSED)
def test_weld_of_a_soup_restores_the_fixture(name):
    from slice3d_amd.mesh_topology import mesh_topology, weld
    v, f = sc.mesh(name)
    vs, fs = tr.soup(v, f, seed=5)
    assert mesh_topology((vs, fs)).n_components == len(f)
    topo = mesh_topology((vs, fs), weld=True)
    ref = tr.topology(vs, fs, weld_first=True)
    _compare(topo, ref, name + " soup, welded")
    fix = _fixture_ref(name)
    assert topo.n_components == fix["n_components"] and topo.is_watertight
    for col in ("faces", "vertices", "edges", "edges_2", "euler"):
        assert sorted(topo.table[col]) == sorted(fix["table"][col]) and topo.summary[col] == fix["summary"][col]
    wv, wf, vmap = weld(vs, fs)
    rv, rf = tr.keep(vs, fs, ref["face_component"], np.ones(ref["n_components"], dtype=bool), vmap=ref["vmap"])
    assert np.array_equal(vmap, ref["vmap"]) and np.array_equal(wf, rf) and np.array_equal(_bits(wv), _bits(rv))
    assert len(wv) == len(np.unique(f))


def test_weld_zeros_ulps_and_nans():
    from slice3d_amd._lib import S3dError
    from slice3d_amd.mesh_topology import mesh_topology, weld
    corners = np.array([[x, y, z] for x in (0.0, 1.0) for y in (0.0, 1.0) for z in (0.0, 1.0)])
    quads = [[0, 1, 3, 2], [4, 6, 7, 5], [0, 4, 5, 1], [2, 3, 7, 6], [0, 2, 6, 4], [1, 5, 7, 3]]
    f = np.array([t for q in quads for t in ([q[0], q[1], q[2]], [q[0], q[2], q[3]])], dtype=np.int64)
    vs, fs = tr.soup(corners, f, seed=2)
    rng = np.random.default_rng(3)
    vs = np.where((vs == 0.0) & (rng.random(vs.shape) < 0.5), -0.0, vs)          # both zeros, at random
    assert np.signbit(vs).any() and (~np.signbit(vs[vs == 0.0])).any()
    wv, wf, vmap = weld(vs, fs)
    assert len(wv) == 8 and np.array_equal(vmap, tr.weld(vs, fs))
    topo = mesh_topology((vs, fs), weld=True)
    assert topo.is_watertight and topo.summary["euler"] == 2 and topo.summary["vertices"] == 8
    # 1 ulp apart: not the same vertex
    v = np.array([[0.0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 0], [np.nextafter(1.0, 2.0), 0, 0], [0, -1, 0]])
    f = np.array([[0, 1, 2], [3, 5, 4]], dtype=np.int64)
    topo = mesh_topology((v, f), weld=True)
    assert np.array_equal(topo.vmap, [0, 1, 2, 0, 4, 5]) and topo.summary["vertices"] == 5 and topo.n_components == 1
    _compare(topo, tr.topology(v, f, weld_first=True), "1 ulp")
    # NaN: an error in a vertex a face names, ignored in one that none names
    v = np.concatenate([v, [[np.nan, 0, 0]]])
    _compare(mesh_topology((v, f), weld=True), tr.topology(v, f, weld_first=True), "unreferenced NaN")
    with pytest.raises(S3dError, match="not finite"):
        mesh_topology((v, np.array([[0, 1, 6]], dtype=np.int64)), weld=True)
    v[6] = [np.inf, 0, 0]
    with pytest.raises(S3dError, match="not finite"):
        mesh_topology((v, np.array([[0, 1, 6]], dtype=np.int64)), weld=True)


# ---------------------------------------------------------------------------------------------- 5: errors
def test_argument_checks():
    from slice3d_amd import _lib as L
    from slice3d_amd.mesh_topology import mesh_topology
    lib = L.load()
    v, f = sc.mesh("octahedron")
    vd, fd = torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda()
    nb = lib.s3d_mesh_topology_workspace_bytes(len(v), len(f), 1)
    assert nb > 0 and lib.s3d_mesh_topology_workspace_bytes(len(v), -1, 0) == 0
    assert lib.s3d_mesh_topology_workspace_bytes(len(v), 1 << 29, 0) == 0 and lib.s3d_mesh_topology_workspace_bytes(1 << 30, 4, 0) == 0
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    k, nr = C.c_long(0), C.c_int(0)
    summary = (C.c_longlong * 11)()
    st = L.stream_ptr(vd.device)

    def run(faces, n_faces, n_bytes, weld=1):
        return lib.s3d_mesh_topology_run(vd.data_ptr(), len(v), faces.data_ptr(), n_faces, weld, ws.data_ptr(), n_bytes,
                                         C.byref(k), C.byref(nr), summary, st)

    for bad_index in (6, -1):
        fb = fd.clone()
        fb[3, 1] = bad_index
        assert run(fb, len(f), nb) == -1 and b"outside" in lib.s3d_last_error()
    assert run(fd, len(f), nb - 1) == -1 and b"workspace" in lib.s3d_last_error()
    out = torch.empty(len(f), dtype=torch.int64, device="cuda")
    assert lib.s3d_mesh_topology_emit_labels(ws.data_ptr(), nb - 1, len(v), len(f), 1, None, out.data_ptr(), None, st) == -1
    assert run(fd, len(f), nb) == 0 and k.value == 1 and 1 <= nr.value <= 64
    assert list(summary)[:3] == [8, 6, 12] and summary[8] == 2 and summary[9] == 1
    # the emit and keep calls hold their arguments against what the run left in the workspace
    big = torch.empty(4 * 11, dtype=torch.int64, device="cuda")
    for wrong_k in (9, 2, 0):
        assert lib.s3d_mesh_topology_emit_table(ws.data_ptr(), nb, len(v), len(f), 1, wrong_k, big.data_ptr(), big.data_ptr(), st) == -1
        assert b"components" in lib.s3d_last_error()
    nvo, nfo = C.c_long(0), C.c_long(0)
    flags = torch.ones(4, dtype=torch.uint8, device="cuda")
    assert lib.s3d_mesh_topology_keep_run(ws.data_ptr(), nb, len(v), len(f), 1, 2, flags.data_ptr(), 0, C.byref(nvo), C.byref(nfo), st) == -1
    assert lib.s3d_mesh_topology_emit_labels(ws.data_ptr(), nb, len(v), len(f) - 1, 1, None, out.data_ptr(), None, st) == -1
    assert b"the run on this workspace had" in lib.s3d_last_error()
    vo, fo = torch.empty((6, 3), dtype=torch.float64, device="cuda"), torch.empty((8, 3), dtype=torch.int64, device="cuda")
    assert lib.s3d_mesh_topology_keep_emit(ws.data_ptr(), nb, vd.data_ptr(), len(v), len(f), 1, vo.data_ptr(), fo.data_ptr(), st) == -1
    assert b"keep_run" in lib.s3d_last_error()
    assert lib.s3d_mesh_topology_keep_run(ws.data_ptr(), nb, len(v), len(f), 1, 1, flags.data_ptr(), 0, C.byref(nvo), C.byref(nfo), st) == 0
    assert (nvo.value, nfo.value) == (6, 8)
    assert lib.s3d_mesh_topology_keep_emit(ws.data_ptr(), nb, vd.data_ptr(), len(v), len(f), 1, vo.data_ptr(), fo.data_ptr(), st) == 0
    assert torch.equal(fo, fd) and torch.equal(vo, vd)
    fresh = torch.zeros(nb, dtype=torch.uint8, device="cuda")
    assert lib.s3d_mesh_topology_emit_labels(fresh.data_ptr(), nb, len(v), len(f), 1, None, out.data_ptr(), None, st) == -1
    assert b"no completed" in lib.s3d_last_error()
    torch.cuda.synchronize()
    # no face: no component
    assert run(fd, 0, nb) == 0 and k.value == 0
    empty = mesh_topology((v, np.zeros((0, 3), dtype=np.int64)))
    assert empty.n_components == 0 and len(empty.face_component) == 0 and np.array_equal(empty.vertex_component, [-1] * 6)
    assert empty.summary["faces"] == 0 and not empty.is_watertight
    assert mesh_topology((np.zeros((0, 3)), np.zeros((0, 3), dtype=np.int64))).n_components == 0


# ---------------------------------------------------------------------------------------------- 6: non-manifold meshes
@pytest.mark.parametrize("name", tr.HAND_MADE)
def test_hand_made_meshes(name):
    from slice3d_amd.mesh_topology import mesh_topology
    v, f = tr.hand_made(name)
    _compare(mesh_topology((v, f)), tr.topology(v, f), name)


# ---------------------------------------------------------------------------------------------- 7: keep
@functools.lru_cache(maxsize=None)
def _boxes_and_tetrahedra():
    """boxes, then three small tetrahedra: two the same (coordinates in eighths: every product exact) and one half their
    size with a face that repeats an index hung on it"""
    v, f = sc.mesh("boxes")
    tv, tf = tr.hand_made("tetrahedron")
    parts_v, parts_f, n = [v], [f], len(v)
    for scale, shift in ((0.125, [4.0, 0, 0]), (0.125, [0, 4.0, 0]), (0.0625, [0, 0, 4.0])):
        parts_v.append(tv * scale + np.array(shift))
        parts_f.append(tf + n)
        n += 4
    parts_f.append(np.array([[n - 1, n - 2, n - 2]], dtype=np.int64))
    return np.concatenate(parts_v), np.concatenate(parts_f)


@functools.lru_cache(maxsize=None)
def _keep_case():
    from slice3d_amd.mesh_topology import mesh_topology
    v, f = _boxes_and_tetrahedra()
    return mesh_topology((v, f)), tr.topology(v, f)


KEEP_RULES = [dict(largest=n, by=by) for by in ("faces", "area", "volume") for n in (1, 2)] + \
             [dict(min_frac=0.02, by="area"), dict(largest=5, by="faces"), dict(largest=4, by="area")]
TIES = [dict(largest=5, by="faces"), dict(largest=4, by="area")]     # the last place is between the two equal tetrahedra


@pytest.mark.parametrize("rules", KEEP_RULES, ids=lambda r: "-".join("%s=%s" % kv for kv in sorted(r.items())))
@pytest.mark.parametrize("drop", [False, True])
def test_keep(rules, drop):
    from slice3d_amd.mesh_topology import keep_components, select_components
    v, f = _boxes_and_tetrahedra()
    topo, ref = _keep_case()
    assert topo.n_components == 6
    mask = select_components(ref["table"], **rules)
    assert np.array_equal(select_components(topo.table, **rules), mask)
    if rules in TIES:                      # components 3 and 4 measure the same: the lower id has the place
        assert ref["table"][rules["by"]][3] == ref["table"][rules["by"]][4] and topo.table[rules["by"]][3] == topo.table[rules["by"]][4]
        assert mask[:3].all() and mask[3] and not mask[4] and mask.sum() == rules["largest"]
    m = keep_components((v, f), rules, drop_degenerate=drop, topology=topo)
    rv, rf = tr.keep(v, f, ref["face_component"], mask, drop_degenerate=drop)
    assert np.array_equal(m.faces, rf) and np.array_equal(_bits(m.vertices), _bits(rv))
    if rules.get("largest") == 1:
        assert sr.is_oriented_manifold(m.faces, closed=True) and sr.euler_characteristic(m.faces) == 2


def test_keep_drop_degenerate_and_split():
    from slice3d_amd.mesh_topology import keep_components, largest_component, split
    v, f = _boxes_and_tetrahedra()
    topo, ref = _keep_case()
    assert ref["table"]["degenerate"].tolist() == [0, 0, 0, 0, 0, 1] and not topo.is_watertight
    everything = np.ones(6, dtype=bool)
    m = keep_components((v, f), everything, drop_degenerate=True, topology=topo)
    rv, rf = tr.keep(v, f, ref["face_component"], everything, drop_degenerate=True)
    assert len(m.faces) == len(f) - 1 and np.array_equal(m.faces, rf) and np.array_equal(_bits(m.vertices), _bits(rv))
    m = keep_components((v, f), everything, topology=topo)
    assert np.array_equal(m.faces, f) and np.array_equal(_bits(m.vertices), _bits(v))
    for other, kw in (((v, f[:-1]), {}), ((v[:-1], f), {}), ((v, f), dict(weld=True))):     # not this topology's mesh
        with pytest.raises(ValueError, match="not of this one"):
            keep_components(other, everything, topology=topo, **kw)
    parts = split((v, f))
    assert [len(p.faces) for p in parts] == ref["table"]["faces"].tolist()
    big = largest_component((v, f), by="volume")
    assert len(big.faces) == ref["table"]["faces"][np.argmax(np.abs(ref["table"]["volume"]))]


# ---------------------------------------------------------------------------------------------- 8: marching cubes
def test_marching_cubes_floaters():
    from slice3d_amd.mesh import marching_cubes_device
    from slice3d_amd.mesh_simplify import simplify_mesh
    from slice3d_amd.mesh_topology import largest_component, mesh_topology
    n = 48
    a = np.linspace(-1.0, 1.0, n)
    x, y, z = np.meshgrid(a, a, a, indexing="ij")
    balls = [((0.0, 0.0, 0.0), 0.5)] + [((sx * 0.75, sy * 0.75, sz * 0.75), 0.12)
                                        for sx, sy, sz in ((1, 1, 1), (-1, 1, 1), (1, -1, 1), (1, 1, -1), (-1, -1, -1))]
    field = np.max([r - np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2) for c, r in balls], axis=0)
    vd, fd = marching_cubes_device(torch.from_numpy(field).cuda(), 0.0, pad_value=-1e6)
    topo = mesh_topology((vd, fd))
    print("marching cubes 48^3: %d faces, %d components in %d rounds" % (fd.shape[0], topo.n_components, topo.rounds))
    assert topo.n_components == 6 and topo.is_watertight
    _compare_host = tr.topology(vd.cpu().numpy(), fd.cpu().numpy())
    assert np.array_equal(topo.face_component.cpu().numpy(), _compare_host["face_component"])
    big = largest_component((vd, fd))
    assert len(big.faces) == topo.table["faces"].max()
    assert sr.is_oriented_manifold(big.faces, closed=True) and sr.euler_characteristic(big.faces) == 2
    assert tr.components(big.faces, len(big.vertices))[0] == 1 and sr.indices_valid(big.vertices, big.faces)
    small = simplify_mesh(big, len(big.faces) // 4, 5.0)
    assert 0 < len(small.faces) <= len(big.faces) // 4 and sr.is_oriented_manifold(small.faces, closed=True)


# ---------------------------------------------------------------------------------------------- 9: scripts
def _run(cmd, cwd):
    r = subprocess.run([sys.executable] + cmd, cwd=cwd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout


RECON = ["--name_dataset", "synthetic", "--synthetic_len", "1", "--img_size", "64", "--mode", "test", "--mc_res0", "16",
         "--mc_up_steps", "2", "--name_ckpt", "none.ckpt", "--synthetic_weights", "--overwrite_res"]


def test_reconstruct_keep_largest(tmp_path):
    """Without the flags the file is what Generator3D.generate_mesh exports; with --keep_largest 1 it has one component, the
    largest of that mesh."""
    sys.path.insert(0, os.path.join(ROOT, "reg_slices"))
    from options import get_parser
    from slice3d_amd.generator import Generator3D
    from slice3d_amd.mesh_eval import load_obj
    from slice3d_amd.models import Slices3DRegModel
    from slice3d_amd.synth import SyntheticSlice3DDataset
    from slice3d_amd.weights import load_seeded
    script = os.path.join(ROOT, "reg_slices", "reconstruct.py")
    out = _run([script, "--name_exp", "plain"] + RECON, str(tmp_path))
    assert "components (in / kept)" not in out and "time (clean)" not in out
    with open(tmp_path / "experiments" / "plain" / "results" / "synthetic" / "synthetic_0000.obj", "rb") as fh:
        plain = fh.read()
    args = get_parser().parse_args(RECON)
    model = load_seeded(Slices3DRegModel(img_size=args.img_size, n_slices=args.n_slices, mode="test"), 0).cuda().eval()
    gen = Generator3D(model, threshold=args.mc_threshold, resolution0=args.mc_res0, upsampling_steps=args.mc_up_steps,
                      chunk_size=args.mc_chunk_size, pred_type=args.pred_type)
    item = SyntheticSlice3DDataset(1, args.img_size, 16, args.n_slices, split="test")[0]
    with torch.no_grad():
        mesh, _ = gen.generate_mesh({k: x.unsqueeze(0).cuda() for k, x in item.items()})
    mesh.export(str(tmp_path / "direct.obj"))
    with open(tmp_path / "direct.obj", "rb") as fh:
        assert plain == fh.read()
    out = _run([script, "--name_exp", "clean", "--keep_largest", "1"] + RECON, str(tmp_path))
    assert "components (in / kept)" in out and "time (clean)" in out
    kept = load_obj(str(tmp_path / "experiments" / "clean" / "results" / "synthetic" / "synthetic_0000.obj"))
    ref = tr.topology(mesh.vertices, mesh.faces)
    print("reconstruct.py: %d components, %d faces -> %d" % (ref["n_components"], len(mesh.faces), len(kept.faces)))
    assert tr.components(kept.faces, len(kept.vertices))[0] == 1 and sr.indices_valid(kept.vertices, kept.faces)
    assert len(kept.faces) == ref["table"]["faces"].max()


def test_clean_meshes_processes_a_directory(tmp_path):
    from slice3d_amd.mesh import Mesh
    from slice3d_amd.mesh_eval import load_obj
    src, src_soup, dst = tmp_path / "in", tmp_path / "in_soup", tmp_path / "out"
    src.mkdir()
    src_soup.mkdir()
    Mesh(*sc.mesh("sphere")).export(str(src / "sphere.obj"))
    Mesh(*_boxes_and_tetrahedra()).export(str(src / "mixed.obj"))
    Mesh(*tr.soup(*sc.mesh("torus"), seed=1)).export(str(src_soup / "soup.obj"))
    script = os.path.join(ROOT, "reg_slices", "clean_meshes.py")
    out = _run([script, "--dir_meshes", str(src), "--dir_out", str(dst), "--keep_largest", "3",
                "--min_component_frac", "0.5", "--component_measure", "faces", "--drop_degenerate"], str(tmp_path))
    summary = json.loads(out.strip().splitlines()[-1])
    rows = {r["mesh"]: r for r in summary["meshes"]}
    assert summary["n_meshes"] == 2 and not summary["weld"] and sorted(rows) == ["mixed.obj", "sphere.obj"]
    assert (rows["mixed.obj"]["components_in"], rows["sphere.obj"]["components_in"]) == (6, 1)
    assert rows["sphere.obj"]["watertight"] and not rows["mixed.obj"]["watertight"]
    boxes_ref = _fixture_ref("boxes")
    expect = int((boxes_ref["table"]["faces"] >= 0.5 * boxes_ref["table"]["faces"].max()).sum())
    assert rows["mixed.obj"]["components_kept"] == expect
    for name, row in rows.items():
        m = load_obj(str(dst / name))
        assert len(m.faces) == row["faces_out"] and len(m.vertices) == row["vertices_out"] and row["seconds"] > 0
        assert tr.components(m.faces, len(m.vertices))[0] == row["components_kept"]
    lines = open(dst / "topology.csv").read().strip().splitlines()
    assert lines[0].split(",")[:4] == ["mesh", "component", "kept", "faces"] and len(lines) == 1 + 6 + 1
    cells = dict(zip(lines[0].split(","), [ln for ln in lines if ln.startswith("sphere.obj")][0].split(",")))
    assert (cells["faces"], cells["euler"], cells["closed_oriented"], cells["kept"]) == (str(len(sc.mesh("sphere")[1])), "2", "1", "1")
    # --weld: the soup is the torus again
    welded = tmp_path / "welded"
    out = _run([script, "--dir_meshes", str(src_soup), "--dir_out", str(welded), "--weld"], str(tmp_path))
    row = json.loads(out.strip().splitlines()[-1])["meshes"][0]
    assert row["components_in"] == 1 and row["watertight"] and row["vertices_out"] == len(np.unique(sc.mesh("torus")[1]))
    m = load_obj(str(welded / "soup.obj"))
    assert sr.is_oriented_manifold(m.faces, closed=True) and sr.euler_characteristic(m.faces) == 0
    # --report_only: the table, no mesh
    rep = tmp_path / "report"
    out = _run([script, "--dir_meshes", str(src_soup), "--dir_out", str(rep), "--report_only"], str(tmp_path))
    assert sorted(os.listdir(rep)) == ["topology.csv"]
    assert json.loads(out.strip().splitlines()[-1])["meshes"][0]["components_in"] == len(sc.mesh("torus")[1])


def test_make_sdfs_sign_auto(tmp_path):
    from slice3d_amd.mesh import Mesh
    src = tmp_path / "meshes"
    src.mkdir()
    Mesh(*sc.mesh("sphere")).export(str(src / "closed.obj"))
    Mesh(*sdf_cases.mesh("open_sphere")).export(str(src / "open.obj"))
    Mesh(*tr.soup(*sc.mesh("sphere"), seed=4)).export(str(src / "soup.obj"))
    script = os.path.join(ROOT, "reg_slices", "make_sdfs.py")
    out = _run([script, "--dir_meshes", str(src), "--name_dataset", "custom", "--dir_data", str(tmp_path / "data"),
                "--n_points", "1000", "--sign", "auto"], str(tmp_path))
    summary = json.loads(out.strip().splitlines()[-1])
    assert summary["sign"] == "auto" and summary["written"] == 3
    assert summary["signs"] == {"closed": "parity", "open": "winding", "soup": "parity"}
    for shape in ("closed", "open", "soup"):
        assert np.load(tmp_path / "data" / "custom" / "02_sdfs" / (shape + ".npy")).shape == (1000, 4)

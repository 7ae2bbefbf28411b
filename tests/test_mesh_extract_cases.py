"""CPU side of the mesh-extraction conformance tests (tests/mesh_extract_cases.py): the case tables do what their ids claim,
the host library (slice3d_amd/csrc_mesh) reproduces the reference goldens of every case bit for bit
(tests/golden/mesh_extract_reference.npz, made by tests/golden/make_golden_mesh_extract.py from the reference's compiled
libmcubes / libmise alone), the committed goldens equal the live reference when oracle/_ref is built, and the device
library's size functions refuse what its int indices cannot address.  The device itself: tests/test_gpu_mesh_extract.py."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import mesh_extract_cases as K
from helpers import GOLDEN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.path.join(ROOT, "oracle", "_ref")
MC_IDS = [c.id for c in K.MC_CASES]
MISE_IDS = [c.id for c in K.MISE_CASES]


@pytest.fixture(scope="module")
def mesh():
    from slice3d_amd import mesh as m
    if not os.path.isfile(m.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(ROOT, "slice3d_amd", "csrc_mesh")], check=True)
    return m


@pytest.fixture(scope="module")
def gold():
    z = np.load(os.path.join(GOLDEN, "mesh_extract_reference.npz"))
    return {k: z[k] for k in z.files}


# ------------------------------------------------------------------------------------------------------------------
# the tables do what their ids claim (reference outputs and regenerated inputs only)
# ------------------------------------------------------------------------------------------------------------------
def test_case_ids_are_unique_and_the_golden_holds_exactly_the_tables(gold):
    assert len(set(MC_IDS)) == len(MC_IDS) and len(set(MISE_IDS)) == len(MISE_IDS)
    want = set()
    for c in K.MC_CASES:
        assert K.MC_BY_ID[c.golden].golden == c.golden
        if c.golden == c.id:
            want |= {"mc/%s/%s" % (c.id, k) for k in (("counts", "sha256") if c.digest_only else ("v", "t"))}
    for c in K.MISE_CASES:
        want |= {"mise/%s/%s" % (c.id, k) for k in (("qn", "qsha", "dsha") if c.digest_only else ("qn", "q", "dense"))}
    assert set(gold) == want
    assert all(a.dtype.kind in "fiu" for a in gold.values())          # numeric arrays and nothing else
    assert os.path.getsize(os.path.join(GOLDEN, "mesh_extract_reference.npz")) <= 512 * 1024


def test_marching_cubes_table_covers_what_the_issue_lists():
    by = lambda **kw: [c for c in K.MC_CASES if all(getattr(c, k) == v for k, v in kw.items())]
    for shape in ((6, 6, 6), (7, 4, 9), (3, 11, 6), (2, 3, 5), (9, 2, 2)):
        assert by(shape=shape, pad=None, six_faces=True) and by(shape=shape, pad=-1e6)
    assert any(c.pad is not None and c.pad > c.iso for c in K.MC_CASES)
    assert by(shape=(1, 4, 4), pad=None, empty=True) and by(shape=(1, 4, 4), pad=-1e6, empty=False)
    assert {0.0, 0.25, -0.3, K.LOGIT_02} <= {c.iso for c in K.MC_CASES}
    assert by(dtype="f32", iso=0.1) and by(dtype="f16")
    assert all(K.MC_BY_ID[c.golden].dtype == "f32" for c in by(dtype="f16"))
    big = by(digest_only=True)
    assert len(big) == 1 and big[0].shape == (66, 65, 67)
    cells = 65 * 64 * 66
    assert cells > 1024 * 256 and cells % 256 != 0


@pytest.mark.parametrize("cid", MC_IDS)
def test_marching_cubes_case_is_what_its_id_says(gold, cid):
    case = K.MC_BY_ID[cid]
    vol = K.mc_volume(case)
    assert vol.shape == case.shape and vol.dtype == K.NP_DTYPE[case.dtype]
    wide = vol.astype(np.float64)
    if case.dtype == "f16":
        assert np.array_equal(wide, K.mc_volume(K.MC_BY_ID[case.golden]).astype(np.float64))
    if case.digest_only:
        nv, nt = gold["mc/%s/counts" % case.golden]
    else:
        v, t = gold["mc/%s/v" % case.golden], gold["mc/%s/t" % case.golden]
        nv, nt = len(v), len(t)
        assert v.dtype == np.float64 and t.dtype == np.int64
    if case.empty:
        assert (nv, nt) == (0, 0)
    else:
        assert nt >= 1 and nv >= 3
    if case.six_faces and not case.digest_only:
        assert case.pad is None
        for axis, n in enumerate(case.shape):      # libmcubes' coordinates are index + 0.5
            assert (v[:, axis] == 0.5).any() and (v[:, axis] == n - 0.5).any(), (cid, axis)
    if "ties" in cid:
        assert int((wide == case.iso).sum()) >= 8
        assert (wide[0] == case.iso).any()          # a plateau on the boundary
    if "naninf" in cid:
        inner = wide[1:-1, 1:-1, 1:-1]
        for pred in (np.isnan, np.isposinf, np.isneginf):
            assert pred(inner).any() and pred(wide).sum() > pred(inner).sum(), cid
        nan = np.isnan(wide)
        assert (nan & np.signbit(wide)).any() and (nan & ~np.signbit(wide)).any()      # NaNs of both signs go in ...
        vn = np.isnan(v)
        assert (vn & np.signbit(v)).any() and (vn & ~np.signbit(v)).any()             # ... and come out of the reference
    if "allbelow" in cid:
        assert (wide <= case.iso).all()
    if "allabove" in cid:
        assert (wide > case.iso).all()
    if case.dtype == "f32" and case.iso == 0.1:
        assert float(np.float32(0.1)) > 0.1 and (vol == np.float32(0.1)).sum() >= 8
        assert not (wide <= case.iso)[vol == np.float32(0.1)].any()
    if case.pad is not None and case.pad > case.iso:
        assert nt >= 1


def test_mise_table_covers_what_the_issue_lists():
    assert {(c.r0, c.depth, c.thr) for c in K.MISE_CASES} == {(3, 2, 0.0), (5, 2, 0.25), (2, 3, -0.25), (6, 1, 0.0),
                                                              (1, 4, 0.0), (7, 2, 0.0), (8, 3, 0.0)}
    for field in ("kind", "policy", "dtype"):
        assert {getattr(c, field) for c in K.MISE_CASES} == {"kind": {"noise", "sparse", "ties"},
                                                             "policy": {"full", "partial", "partial+revalue"},
                                                             "dtype": {"f64", "f32", "f16"}}[field]
    for policy in ("full", "partial", "partial+revalue"):       # every policy through every update entry point
        assert {c.dtype for c in K.MISE_CASES if c.policy == policy} == {"f64", "f32", "f16"}
    assert any(c.kind == "ties" and c.thr != 0.0 for c in K.MISE_CASES)
    g = K.MISE_BY_ID[K.GROWTH_CASE]
    assert (g.r0, g.depth, g.kind) == (8, 3, "noise") and K.mise_r1(g) == 65


@pytest.mark.parametrize("cid", MISE_IDS)
def test_mise_case_is_what_its_id_says(gold, cid):
    case = K.MISE_BY_ID[cid]
    qn = gold["mise/%s/qn" % cid]
    assert case.depth < len(qn) <= K.MAX_ROUNDS
    n = K.mise_r1(case) ** 3
    vals = K.mise_values(case, np.arange(n))
    assert vals.dtype == K.NP_DTYPE[case.dtype]
    if case.kind == "ties":
        assert int((vals.astype(np.float64) == case.thr).sum()) >= 8
    if cid == K.GROWTH_CASE:
        assert qn.max() > 65536
    if case.digest_only:
        return
    sets = K.mise_sets(gold, case)
    assert all((np.diff(s) > 0).all() and s[0] >= 0 and s[-1] < n for s in sets)
    if case.policy != "full":        # a point asked for again in the next round was left unanswered
        assert any(len(np.intersect1d(a, b)) for a, b in zip(sets, sets[1:]))
    else:
        assert not any(len(np.intersect1d(a, b)) for a, b in zip(sets, sets[1:]))


# ------------------------------------------------------------------------------------------------------------------
# the host library against the goldens, bit for bit
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", MC_IDS)
def test_host_marching_cubes_equals_the_reference(mesh, gold, cid):
    case = K.MC_BY_ID[cid]
    v, t = mesh.marching_cubes(K.mc_reference_input(case), case.iso)
    if case.digest_only:
        assert [len(v), len(t)] == list(gold["mc/%s/counts" % case.golden])
        assert np.array_equal(K.sha256_u8(v, t), gold["mc/%s/sha256" % case.golden])
    else:
        assert K.bits_equal(t, gold["mc/%s/t" % case.golden])      # same faces, same vertex numbering
        assert K.bits_equal(v, gold["mc/%s/v" % case.golden])      # bit-exact coordinates


@pytest.mark.parametrize("cid", MISE_IDS)
def test_host_mise_equals_the_reference(mesh, gold, cid):
    case = K.MISE_BY_ID[cid]
    rounds, dense = K.drive_host_style(case, mesh.MISE(case.r0, case.depth, case.thr))
    K.check_mise_against_golden(gold, case, rounds, dense)


# ------------------------------------------------------------------------------------------------------------------
# against the live reference
# ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def live():
    if not (os.path.isfile(os.path.join(REF, "libmcref.so")) and any(f.startswith("mise.") and f.endswith(".so")
                                                                     for f in os.listdir(REF))):
        pytest.skip("oracle/_ref not built here (make -C oracle)")
    sys.path.insert(0, os.path.join(GOLDEN))
    sys.path.insert(0, REF)
    try:
        import make_golden_mesh_extract as G
        from mise import MISE
    finally:
        sys.path.remove(REF)
        sys.path.remove(GOLDEN)
    return G, MISE


def test_committed_goldens_equal_a_fresh_run_of_the_reference(live, gold):
    from helpers import golden_digest
    fresh = live[0].records()
    assert sorted(fresh) == sorted(gold)
    assert [k for k in sorted(gold) if not K.bits_equal(fresh[k], gold[k])] == []
    assert golden_digest(fresh) == golden_digest(gold)


@pytest.mark.parametrize("cid", [c.id for c in K.MISE_CASES if not c.digest_only])
def test_host_mise_queries_in_the_live_references_order(mesh, live, cid):
    """The goldens hold each round's SET; the host port also promises the reference's insertion order."""
    case = K.MISE_BY_ID[cid]
    ref_rounds, ref_dense = K.drive_host_style(case, live[1](case.r0, case.depth, case.thr))
    rounds, dense = K.drive_host_style(case, mesh.MISE(case.r0, case.depth, case.thr))
    assert len(rounds) == len(ref_rounds)
    assert all(np.array_equal(a, b) for a, b in zip(rounds, ref_rounds))
    assert K.bits_equal(dense, ref_dense)


# ------------------------------------------------------------------------------------------------------------------
# host arithmetic of the device library's size functions
# ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hiplib():
    from slice3d_amd import _lib
    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    try:
        ctypes.CDLL(_lib.LIB_PATH)
    except OSError as e:
        pytest.skip("HIP runtime not loadable here: %s" % e)
    return _lib.load()


def test_mise_workspace_bytes_refuses_point_counts_beyond_int(hiplib):
    """Point indices are int throughout (the idx arrays, mise_emit_kernel, mise_points_kernel, the wrapper's int32 buffer):
    (res + 1)^3 must fit, i.e. res <= 1289.  1290^3 = 2 146 689 000 fits, 1291^3 does not."""
    fn = hiplib.s3d_mise_dev_workspace_bytes
    assert 1290 ** 3 <= 2 ** 31 - 1 < 1291 ** 3
    for r0, depth in ((645, 1), (1290, 0), (323, 2), (81, 4), (1291, 0), (2047, 0), (1023, 1), (3, 9), (1, 11)):
        assert ((r0 << depth) + 1) ** 3 > 2 ** 31 - 1
        assert fn(r0, depth) == 0, (r0, depth)
    for r0, depth in ((0, 0), (-1, 2), (4, -1), (4, 13), (2048, 0), (1, 12)):
        assert fn(r0, depth) == 0, (r0, depth)
    # depth 0: non-zero and increasing in the resolution; strictly from res = 3 on, where one more point per axis adds
    # 8 * 3 * (res + 1)^2 >= 256 bytes of values (the sections are aligned to 256 bytes: res 1 and 2 both take 1280)
    prev = 0
    for res in list(range(1, 66)) + [255, 256, 257, 1023, 1024, 1288, 1289]:
        nb = fn(res, 0)
        assert nb > prev or (res < 3 and nb == prev), res
        assert nb >= (res + 1) ** 3 * 9 + res ** 3       # values, point states, one voxel level
        prev = nb
    for r0, depth in ((1, 10), (161, 3), (644, 1), (322, 2), (5, 8)):   # large accepted resolutions at depth > 0
        assert ((r0 << depth) + 1) ** 3 <= 2 ** 31 - 1
        assert fn(r0, depth) > fn(r0 << depth, 0) > 0, (r0, depth)      # the same points, more voxel levels
    sizes = [fn(5, depth) for depth in range(0, 9)]                      # 5 << 8 = 1280 still fits
    assert sizes[0] > 0 and all(b > a for a, b in zip(sizes, sizes[1:]))


def test_mc_workspace_bytes_of_cell_less_and_padded_grids(hiplib):
    fn = hiplib.s3d_mc_dev_workspace_bytes
    for shape in ((1, 4, 4), (4, 1, 4), (4, 4, 1), (1, 1, 1), (1, 1, 9), (0, 4, 4)):
        assert fn(*shape, 0) == 256, shape
    for shape in ((1, 4, 4), (1, 1, 1), (2, 3, 5), (7, 4, 9), (66, 65, 67), (9, 2, 2)):
        padded = tuple(s + 2 for s in shape)
        assert fn(*shape, 1) == fn(*padded, 0) > 256, shape
    for shape in ((2, 2, 2), (7, 4, 9), (66, 65, 67)):
        cells = (shape[0] - 1) * (shape[1] - 1) * (shape[2] - 1)
        assert fn(*shape, 0) >= cells * 9 + 8 * ((cells + 255) // 256 + 1)   # case byte + two offsets per cell, block sums

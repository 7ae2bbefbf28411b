"""Device MISE / marching cubes (csrc/mesh.hip) on the case tables of tests/mesh_extract_cases.py against the goldens the
REFERENCE's compiled libmcubes / libmise produced for them (tests/golden/mesh_extract_reference.npz): unpadded and
non-cubic volumes, iso != 0, float32 / float16 storage, NaN / inf values, cell-less grids, partial answers, re-valued
points, every update entry point — plus the raw C ABI between guarded buffers and the refusals.  Everything is bit-exact:
there is no tolerance in this file.  The CPU side (the tables' own claims, the host library) is
tests/test_mesh_extract_cases.py."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import mesh_extract_cases as K
from helpers import GOLDEN

pytestmark = pytest.mark.gpu

S3D_E_WORKSPACE = -2
GUARD = 128                               # 64-bit words of guard on each side of a buffer (1 KiB)
GUARD_BITS = 0x7FF5A5A5A5A5A5A5           # as float64: a NaN with a payload no kernel computes; as int64: no vertex id
TORCH_DTYPE = {"f64": torch.float64, "f32": torch.float32, "f16": torch.float16}


@pytest.fixture(scope="module")
def gold():
    z = np.load(os.path.join(GOLDEN, "mesh_extract_reference.npz"))
    return {k: z[k] for k in z.files}


def _lib():
    from slice3d_amd import _lib as L
    return L, L.load()


def _guarded(n, dtype):
    """(buffer, out, pointer): `n` elements of a 64- or 32-bit `dtype` with GUARD 64-bit words before and after, all
    GUARD_BITS.  The pointer is given apart because an empty tensor's data_ptr() is null, and a 0 / 0 emit still gets one."""
    size = torch.empty((), dtype=dtype).element_size()
    words = (n * size + 7) // 8
    buf = torch.full((GUARD + words + GUARD,), GUARD_BITS, dtype=torch.int64, device="cuda")
    return buf, buf[GUARD:GUARD + words].view(dtype)[:n], buf.data_ptr() + 8 * GUARD


def _guarded_bytes(nb, fill=None):
    """(buffer, ws): `nb` bytes between 8 * GUARD guard bytes on each side; the inside is GUARD_BITS too, or the byte `fill`."""
    buf = torch.full((2 * GUARD + (nb + 7) // 8,), GUARD_BITS, dtype=torch.int64, device="cuda").view(torch.uint8)
    ws = buf[8 * GUARD:8 * GUARD + nb]
    if fill is not None:
        ws.fill_(fill)
    return buf, ws


def _guards_intact(buf, n_bytes):
    """Everything of `buf` outside the n_bytes after the leading guard still holds the guard pattern."""
    b = buf.view(torch.uint8)
    pristine = torch.full((b.numel() // 8,), GUARD_BITS, dtype=torch.int64, device="cuda").view(torch.uint8)
    lo, hi = 8 * GUARD, 8 * GUARD + n_bytes
    return bool(torch.equal(b[:lo], pristine[:lo])) and bool(torch.equal(b[hi:], pristine[hi:]))


def _untouched(buf):
    return bool((buf.view(torch.int64) == GUARD_BITS).all())


def _bits(t):
    return t.contiguous().view(torch.int64).cpu().numpy()


def _device_volume(case):
    return torch.from_numpy(K.mc_volume(case)).cuda()


# ------------------------------------------------------------------------------------------------------------------
# marching cubes
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", [c.id for c in K.MC_CASES])
def test_device_marching_cubes_equals_the_reference(gold, cid):
    from slice3d_amd.mesh import marching_cubes_device
    case = K.MC_BY_ID[cid]
    vol = _device_volume(case)
    assert vol.dtype == TORCH_DTYPE[case.dtype] and tuple(vol.shape) == case.shape
    v, t = marching_cubes_device(vol, case.iso, pad_value=case.pad)
    assert v.dtype == torch.float64 and t.dtype == torch.int64 and v.shape[1:] == (3,) and t.shape[1:] == (3,)
    v, t = v.cpu().numpy(), t.cpu().numpy()
    print("mc %-42s %7d vertices %7d faces" % (cid, len(v), len(t)))
    if case.digest_only:
        assert [len(v), len(t)] == list(gold["mc/%s/counts" % case.golden])
        assert np.array_equal(K.sha256_u8(v, t), gold["mc/%s/sha256" % case.golden])
        return
    want_v, want_t = gold["mc/%s/v" % case.golden], gold["mc/%s/t" % case.golden]
    assert np.array_equal(t, want_t)                                          # same faces, same vertex numbering
    assert v.shape == want_v.shape
    assert np.array_equal(v.view(np.int64), want_v.view(np.int64))            # same coordinates as bits, NaN included


RAW_CASES = ["pad-1e6_7x4x9_isologit0.2", "open_7x4x9_iso0.25", "f32_iso0.1_pad-1e6_3x11x6", "naninf_f32_open_3x11x6_iso-0.3",
             "open_9x2x2_one_cell_thick_iso0", "allbelow_open_7x4x9", "allbelow_pad-1e6_3x11x6_f32", "axis1_1x4x4_open_no_cells",
             "axis1_1x4x4_pad-1e6", "big_66x65x67_f32_open_isologit0.2"]


def _mc_args(case, vol, ws, nb):
    pad = 0 if case.pad is None else 1
    return (vol.data_ptr(), 1 if vol.dtype == torch.float64 else 0, *case.shape, pad, 0.0 if case.pad is None else case.pad,
            case.iso, ws.data_ptr(), nb)


@pytest.mark.parametrize("cid", RAW_CASES)
def test_mc_raw_abi_stays_inside_its_workspace_and_outputs(gold, cid):
    """s3d_mc_dev_count / s3d_mc_dev_emit with a workspace of exactly s3d_mc_dev_workspace_bytes bytes and outputs of exactly
    the counted sizes, each between guards: nothing outside is written, every output element is, the result does not
    depend on what the workspace held, and a workspace one byte short is refused before anything is written."""
    L, lib = _lib()
    case = K.MC_BY_ID[cid]
    vol = _device_volume(case)
    pad = 0 if case.pad is None else 1
    nb = lib.s3d_mc_dev_workspace_bytes(*case.shape, pad)
    assert nb >= 256
    runs = []
    for fill in (None, 0x7F):
        wbuf, ws = _guarded_bytes(nb, fill)
        assert ws.data_ptr() % 256 == 0
        nv, nt = C.c_long(-1), C.c_long(-1)
        args = _mc_args(case, vol, ws, nb)
        L.check(lib.s3d_mc_dev_count(*args, C.byref(nv), C.byref(nt), None), cid)
        vbuf, verts, vptr = _guarded(3 * nv.value, torch.float64)
        tbuf, tris, tptr = _guarded(3 * nt.value, torch.int64)
        L.check(lib.s3d_mc_dev_emit(*args, vptr, tptr, None), cid)      # 0 / 0 volumes included
        torch.cuda.synchronize()
        assert _guards_intact(wbuf, nb), (cid, "a write outside the workspace")
        assert _guards_intact(vbuf, 24 * nv.value) and _guards_intact(tbuf, 24 * nt.value), (cid, "a write outside an output")
        assert not bool((verts.view(torch.int64) == GUARD_BITS).any()), (cid, "a vertex coordinate left unwritten")
        assert not bool((tris == GUARD_BITS).any()), (cid, "a face index left unwritten")
        runs.append((verts, tris))
    (v0, t0), (v1, t1) = runs
    assert np.array_equal(_bits(v0), _bits(v1)) and np.array_equal(_bits(t0), _bits(t1)), (cid, "workspace contents matter")
    v, t = v0.cpu().numpy().reshape(-1, 3), t0.cpu().numpy().reshape(-1, 3)
    if case.empty:
        assert (len(v), len(t)) == (0, 0)
    if case.digest_only:
        assert np.array_equal(K.sha256_u8(v, t), gold["mc/%s/sha256" % case.golden])
    else:
        assert np.array_equal(t, gold["mc/%s/t" % case.golden])
        assert np.array_equal(v.view(np.int64), gold["mc/%s/v" % case.golden].view(np.int64))
    # one byte short: refused, nothing written anywhere
    wbuf, ws = _guarded_bytes(nb)
    vbuf, _, vptr = _guarded(max(v.size, 3), torch.float64)
    tbuf, _, tptr = _guarded(max(t.size, 3), torch.int64)
    nv, nt = C.c_long(-1), C.c_long(-1)
    args = _mc_args(case, vol, ws, nb - 1)
    assert lib.s3d_mc_dev_count(*args, C.byref(nv), C.byref(nt), None) == S3D_E_WORKSPACE
    assert lib.s3d_mc_dev_emit(*args, vptr, tptr, None) == S3D_E_WORKSPACE
    torch.cuda.synchronize()
    assert _untouched(wbuf) and _untouched(vbuf) and _untouched(tbuf), (cid, "a refused call wrote something")


def test_device_marching_cubes_on_the_float32_product_path_equals_the_host_library():
    """Generator3D.extract_mesh's call shape — a float32 dense grid, pad_value=-1e6, iso = logit(threshold) — on a
    non-cubic grid at threshold 0.2, against the host library on the padded float64 copy."""
    from slice3d_amd import mesh
    shape = (21, 13, 17)
    li = np.arange(shape[0] * shape[1] * shape[2])
    x, y, z = K._coords(li, shape)
    blob = 4.0 - 0.05 * ((x - 10) ** 2 + 2 * (y - 6) ** 2 + (z - 8) ** 2)        # logits: a blob that leaves the grid on y
    vol = (K.LOGIT_02 + blob + 2.0 * (K.hash01(li, 20) - 0.5)).astype(np.float32).reshape(shape)
    v, t = mesh.marching_cubes_device(torch.from_numpy(vol).cuda(), K.LOGIT_02, pad_value=-1e6)
    hv, ht = mesh.marching_cubes(np.pad(vol.astype(np.float64), 1, "constant", constant_values=-1e6), K.LOGIT_02)
    assert len(ht) > 500
    assert np.array_equal(t.cpu().numpy(), ht)
    assert np.array_equal(v.cpu().numpy().view(np.int64), hv.view(np.int64))


# ------------------------------------------------------------------------------------------------------------------
# MISE
# ------------------------------------------------------------------------------------------------------------------
def _drive_device(case, widen=False):
    """run_mise on a DeviceMISE; widen=True sends the case's values as float64 (s3d_mise_dev_update_f64) instead of in the
    case's dtype (float32: s3d_mise_dev_update; float16: the wrapper's .float() in front of it)."""
    from slice3d_amd.mesh import DeviceMISE
    m = DeviceMISE(case.r0, case.depth, case.thr)
    assert m.resolution + 1 == K.mise_r1(case)

    def query():
        idx = m.query()
        assert idx.dtype == torch.int32
        q = idx.cpu().numpy().astype(np.int64)
        assert (np.diff(q) > 0).all()               # ascending, no duplicates
        return q

    def update(li, vals):
        vals = torch.from_numpy(vals.astype(np.float64) if widen else vals).cuda()
        assert vals.dtype == (torch.float64 if widen else TORCH_DTYPE[case.dtype])
        m.update(torch.from_numpy(li.astype(np.int32)).cuda(), vals)

    rounds = K.run_mise(case, query, update)
    return rounds, m.to_dense().cpu().numpy()


@pytest.mark.parametrize("cid", [c.id for c in K.MISE_CASES])
def test_device_mise_equals_the_reference(gold, cid):
    case = K.MISE_BY_ID[cid]
    rounds, dense = _drive_device(case)
    print("mise %-40s %3d rounds %7d queries" % (cid, len(rounds), sum(len(q) for q in rounds)))
    K.check_mise_against_golden(gold, case, rounds, dense)
    if cid == K.GROWTH_CASE:
        assert max(len(q) for q in rounds) > 65536          # DeviceMISE.query() grew its index buffer
    if case.dtype != "f64":                                  # the same numbers through s3d_mise_dev_update_f64
        rounds64, dense64 = _drive_device(case, widen=True)
        assert len(rounds64) == len(rounds) and all(np.array_equal(a, b) for a, b in zip(rounds64, rounds))
        assert K.bits_equal(dense64, dense)


def _advance(case, m, n_rounds):
    """Answers n_rounds rounds of `m` in full with the case's values; -> the union of everything queried so far."""
    seen = []
    for _ in range(n_rounds):
        idx = m.query().clone()
        assert idx.numel()
        seen.append(idx.cpu().numpy().astype(np.int64))
        m.update(idx, torch.from_numpy(K.mise_values(case, seen[-1])).cuda())
    return np.unique(np.concatenate(seen))


def test_mise_query_capacity_contract_raw_abi():
    """s3d_mise_dev_query with a buffer smaller than the round: *n_out is the full count, exactly `capacity` leading indices
    are written, nothing behind them; the retry with room returns the whole set and starts with what the short call wrote."""
    from slice3d_amd.mesh import DeviceMISE
    L, lib = _lib()
    case = K.MISE_BY_ID["r5_d2_thr0.25_ties_full_f64"]
    m = DeviceMISE(case.r0, case.depth, case.thr)
    _advance(case, m, 2)
    want = m.query().cpu().numpy()
    n = len(want)
    assert n > 600                                  # more than one block's worth of points, from several tiles
    for capacity in (n - 1, n // 2 + 1, 257, 1, 0):
        buf, out, ptr = _guarded(capacity, torch.int32)
        got = C.c_long(-1)
        L.check(lib.s3d_mise_dev_query(m._h, ptr, capacity, C.byref(got), None), "s3d_mise_dev_query")
        torch.cuda.synchronize()
        assert got.value == n
        assert _guards_intact(buf, 4 * capacity), (capacity, "an index written past the capacity")
        assert np.array_equal(out.cpu().numpy(), want[:capacity]), capacity
    buf, out, ptr = _guarded(n, torch.int32)
    got = C.c_long(-1)
    L.check(lib.s3d_mise_dev_query(m._h, ptr, n, C.byref(got), None), "s3d_mise_dev_query")
    torch.cuda.synchronize()
    assert got.value == n and _guards_intact(buf, 4 * n) and np.array_equal(out.cpu().numpy(), want)
    got = C.c_long(-1)                              # counting alone: no buffer at all
    L.check(lib.s3d_mise_dev_query(m._h, None, 0, C.byref(got), None), "s3d_mise_dev_query")
    assert got.value == n


def test_mise_update_refusals_leave_the_octree_unchanged():
    """An index >= r1^3, a negative index, and a lattice point the octree has not created yet: update() raises, alone or
    at the end of a round's valid answers, and the instance then behaves like a twin that never saw the call — the same
    next query, the same dense grid, and after the round's real update the same refinement."""
    from slice3d_amd.mesh import DeviceMISE
    case = K.MISE_BY_ID["r2_d3_thr-0.25_noise_full_f16"]     # depth 3: after two rounds the leaves of level 2 wait for a step
    r1 = K.mise_r1(case)
    m, twin = (DeviceMISE(case.r0, case.depth, case.thr) for _ in range(2))
    seen = _advance(case, m, 2)
    assert np.array_equal(_advance(case, twin, 2), seen)
    idx = m.query().clone()
    q = idx.cpu().numpy().astype(np.int64)
    vals = torch.from_numpy(K.mise_values(case, q).astype(np.float64)).cuda()
    exists = np.union1d(seen, q)                    # every point the octree has created was queried at some time
    missing = int(np.setdiff1d(np.arange(r1 ** 3), exists)[0])
    assert 0 < missing < r1 ** 3 and len(q) > 100

    def same_as_twin():
        assert torch.equal(m.query(), twin.query())
        assert np.array_equal(_bits(m.to_dense()), _bits(twin.to_dense()))

    bad_indices = [(r1 ** 3, torch.int32), (2 ** 31 - 1, torch.int32), (-1, torch.int32), (-2 ** 31, torch.int32),
                   (missing, torch.int32), (2 ** 32 + int(q[0]), torch.int64), (r1 ** 3, torch.int64), (-1, torch.int64)]
    for bad, dtype in bad_indices:
        one = torch.tensor([bad], dtype=dtype, device="cuda")
        with pytest.raises(ValueError):
            m.update(one, vals[:1])
        same_as_twin()
        with pytest.raises(ValueError):             # behind the round's valid answers
            m.update(torch.cat([idx.to(dtype), one]), torch.cat([vals, vals[:1]]))
        same_as_twin()
    m.update(idx, vals)
    twin.update(idx, vals)
    assert m.query().numel() > 0
    same_as_twin()


def test_device_mise_refuses_grids_beyond_int_indices():
    """(res + 1)^3 points must fit the int indices: DeviceMISE raises before it allocates anything."""
    from slice3d_amd.mesh import DeviceMISE
    for r0, depth in ((645, 1), (1290, 0), (2047, 0)):
        before = torch.cuda.memory_allocated()
        with pytest.raises(ValueError, match="bad MISE parameters"):
            DeviceMISE(r0, depth, 0.0)
        assert torch.cuda.memory_allocated() == before

"""Case tables of the mesh-extraction conformance tests (device MISE / marching cubes, csrc/mesh.hip, and their host twin
in csrc_mesh/): pure numpy, deterministic, imported by tests/golden/make_golden_mesh_extract.py (which runs the tables
through the reference's compiled libmcubes / libmise), tests/test_mesh_extract_cases.py and tests/test_gpu_mesh_extract.py.

Every value is a function of the grid's LINEAR index (and the case), through an integer hash: the reference visits points
in insertion order, the device in ascending order, the host port in the reference's order, and all three must see the
same numbers.  No libm function takes part, so the inputs are the same bits on every machine; they are not stored."""
import collections
import math
import zlib

import numpy as np

LOGIT_02 = math.log(0.2 / 0.8)          # Generator3D's iso level for threshold 0.2
_MASK = (1 << 64) - 1


def hash01(li, salt):
    """splitmix64 of (linear index, salt) -> float64 in [0, 1), elementwise."""
    x = np.asarray(li).astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15)
    x = x + np.uint64((int(salt) * 0xD1B54A32D192ED03 + 0x8CB92BA72F3D8DD7) & _MASK)
    x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    x = x ^ (x >> np.uint64(31))
    return (x >> np.uint64(11)).astype(np.float64) / float(1 << 53)


def _salt(case_id):
    return zlib.crc32(case_id.encode())


NP_DTYPE = {"f64": np.float64, "f32": np.float32, "f16": np.float16}

# ------------------------------------------------------------------------------------------------------------------
# marching cubes
# ------------------------------------------------------------------------------------------------------------------
McCase = collections.namedtuple("McCase", "id shape dtype iso pad kind six_faces empty digest_only golden")


def _mc(id, shape, dtype, iso, pad, kind, six_faces=False, empty=False, digest_only=False, golden=None):
    return McCase(id, shape, dtype, iso, pad, kind, six_faces, empty, digest_only, golden or id)


MC_CASES = [
    # unpadded: the surface crosses all six faces of the grid, so cells create the vertices of edges whose owner lies outside
    _mc("open_cube_6x6x6_iso0", (6, 6, 6), "f64", 0.0, None, "noise", six_faces=True),
    _mc("open_7x4x9_iso0.25", (7, 4, 9), "f64", 0.25, None, "noise", six_faces=True),
    _mc("open_3x11x6_iso-0.3", (3, 11, 6), "f64", -0.3, None, "noise", six_faces=True),
    _mc("open_2x3x5_isologit0.2", (2, 3, 5), "f64", LOGIT_02, None, "noise", six_faces=True),
    _mc("open_9x2x2_one_cell_thick_iso0", (9, 2, 2), "f64", 0.0, None, "noise", six_faces=True),
    # the same shapes inside a pad layer far below iso (the product's call), and pad layers ABOVE iso that make surface
    _mc("pad-1e6_cube_6x6x6_iso0.25", (6, 6, 6), "f64", 0.25, -1e6, "noise"),
    _mc("pad-1e6_7x4x9_isologit0.2", (7, 4, 9), "f64", LOGIT_02, -1e6, "noise"),
    _mc("pad-1e6_3x11x6_iso0", (3, 11, 6), "f64", 0.0, -1e6, "noise"),
    _mc("pad-1e6_2x3x5_iso-0.3", (2, 3, 5), "f64", -0.3, -1e6, "noise"),
    _mc("pad-1e6_9x2x2_iso0", (9, 2, 2), "f64", 0.0, -1e6, "noise"),
    _mc("pad+1_above_iso_7x4x9_iso0.25", (7, 4, 9), "f64", 0.25, 1.0, "noise"),
    _mc("pad+1_above_iso_allbelow_3x11x6_iso0", (3, 11, 6), "f64", 0.0, 1.0, "allbelow"),
    # one axis of length 1: no cells unpadded, two cells across when padded
    _mc("axis1_1x4x4_open_no_cells", (1, 4, 4), "f64", 0.0, None, "noise", empty=True),
    _mc("axis1_1x4x4_pad-1e6", (1, 4, 4), "f64", 0.0, -1e6, "noise"),
    _mc("axis1_4x1x4_pad-1e6_f32", (4, 1, 4), "f32", 0.25, -1e6, "noise"),
    # float32 storage: iso 0.1 is no float32; np.float32(0.1) widened is > 0.1, so a cell classified after narrowing iso differs
    _mc("f32_iso0.1_open_7x4x9", (7, 4, 9), "f32", 0.1, None, "near_iso_f32", six_faces=True),
    _mc("f32_iso0.1_pad-1e6_3x11x6", (3, 11, 6), "f32", 0.1, -1e6, "near_iso_f32"),
    _mc("f32_noise_pad-1e6_2x3x5_isologit0.2", (2, 3, 5), "f32", LOGIT_02, -1e6, "noise"),
    # float16 input goes through the wrapper's .float(): the expected mesh is the float32 case's
    _mc("f32_eighths_pad-1e6_7x4x9_iso0.25", (7, 4, 9), "f32", 0.25, -1e6, "eighths"),
    _mc("f16_eighths_pad-1e6_7x4x9_iso0.25", (7, 4, 9), "f16", 0.25, -1e6, "eighths", golden="f32_eighths_pad-1e6_7x4x9_iso0.25"),
    _mc("f32_eighths_open_3x11x6_iso0", (3, 11, 6), "f32", 0.0, None, "eighths"),
    _mc("f16_eighths_open_3x11x6_iso0", (3, 11, 6), "f16", 0.0, None, "eighths", golden="f32_eighths_open_3x11x6_iso0"),
    # exact ties with iso on plateaus, also on the boundary
    _mc("ties_open_cube_6x6x6_iso0", (6, 6, 6), "f64", 0.0, None, "ties"),
    _mc("ties_pad-1e6_7x4x9_iso0.25", (7, 4, 9), "f64", 0.25, -1e6, "ties"),
    _mc("ties_open_3x11x6_iso-0.3", (3, 11, 6), "f64", -0.3, None, "ties"),
    _mc("ties_f32_open_7x4x9_iso0.25", (7, 4, 9), "f32", 0.25, None, "ties"),
    # NaN, +inf, -inf at interior and boundary points
    _mc("naninf_open_7x4x9_iso0", (7, 4, 9), "f64", 0.0, None, "naninf"),
    _mc("naninf_pad-1e6_cube_6x6x6_iso0.25", (6, 6, 6), "f64", 0.25, -1e6, "naninf"),
    _mc("naninf_f32_open_3x11x6_iso-0.3", (3, 11, 6), "f32", -0.3, None, "naninf"),
    # nothing to emit
    _mc("allbelow_open_7x4x9", (7, 4, 9), "f64", 0.25, None, "allbelow", empty=True),
    _mc("allabove_open_7x4x9", (7, 4, 9), "f64", 0.25, None, "allabove", empty=True),
    _mc("allbelow_pad-1e6_3x11x6_f32", (3, 11, 6), "f32", LOGIT_02, -1e6, "allbelow", empty=True),
    # 65*64*66 = 274 560 cells = 1072.5 blocks of 256: the block-sum scan takes its carry loop, the last block is partial
    _mc("big_66x65x67_f32_open_isologit0.2", (66, 65, 67), "f32", LOGIT_02, None, "noise", six_faces=True, digest_only=True),
]
MC_BY_ID = {c.id: c for c in MC_CASES}


def _coords(li, shape):
    ny, nz = shape[1], shape[2]
    return li // (ny * nz), (li // nz) % ny, li % nz


def mc_volume(case):
    """The stored volume of a marching-cubes case, in its storage dtype."""
    shape, iso = case.shape, case.iso
    n = shape[0] * shape[1] * shape[2]
    li = np.arange(n, dtype=np.int64)
    salt = _salt("mc/" + case.kind + "/%dx%dx%d" % shape)       # cases of one kind and shape share their hash stream
    u = hash01(li, salt)
    x, y, z = _coords(li, shape)
    cx, cy, cz = shape[0] // 2, shape[1] // 2, shape[2] // 2
    if case.kind in ("noise", "naninf"):
        f = iso + (u - 0.5)
    elif case.kind == "allbelow":
        f = iso - 1.0 - u
    elif case.kind == "allabove":
        f = iso + 1.0 + u
    elif case.kind == "eighths":                                # exact in float16, ties with iso = 0 / 0.25 included
        f = np.floor(u * 17.0) / 8.0 - 1.0
    elif case.kind == "ties":
        f = iso + 0.25 * (np.floor(u * 5.0) - 2.0)
        plateau = ((x <= 1) & (y <= 1)) | ((abs(x - cx) <= 1) & (abs(y - cy) <= 1) & (abs(z - cz) <= 1) & (x >= cx) & (y >= cy))
        f = np.where(plateau, iso, f)
    elif case.kind == "near_iso_f32":
        a = np.float32(iso)                                     # 0.1 -> 0.100000001490116..., above the float64 iso
        below = np.nextafter(a, np.float32(-1.0))
        table = np.array([a, a, below, a + np.float32(0.5), a - np.float32(0.5), a + np.float32(0.25),
                          a - np.float32(0.125), below], dtype=np.float32)
        f = table[np.floor(u * 8.0).astype(np.int64)].astype(np.float64)
    else:
        raise ValueError(case.kind)
    if case.kind == "naninf":
        def at(i, j, k):
            return (i * shape[1] + j) * shape[2] + k
        f[at(0, 0, 0)] = np.nan
        f[at(cx, cy, cz)] = np.nan
        f[at(shape[0] - 1, shape[1] - 1, shape[2] - 1)] = np.inf
        f[at(cx, cy, cz + 1)] = np.inf
        f[at(0, shape[1] - 1, cz)] = -np.inf
        f[at(cx, cy - 1, cz)] = -np.inf
        f[at(cx, cy, cz - 2)] = -np.nan                         # sign bit set: the reference hands a NaN's sign on
        f[at(shape[0] - 1, 0, 0)] = -np.nan
    return f.reshape(shape).astype(NP_DTYPE[case.dtype])


def mc_reference_input(case):
    """What the reference (and the host library) run on: the stored values widened to float64, padded where the case pads."""
    vol = mc_volume(case).astype(np.float64)
    return vol if case.pad is None else np.pad(vol, 1, "constant", constant_values=case.pad)


# ------------------------------------------------------------------------------------------------------------------
# MISE
# ------------------------------------------------------------------------------------------------------------------
MiseCase = collections.namedtuple("MiseCase", "id r0 depth thr kind policy dtype digest_only")


def _mise(r0, depth, thr, kind, policy, dtype, digest_only=False):
    return MiseCase("r%d_d%d_thr%g_%s_%s_%s" % (r0, depth, thr, kind, policy, dtype), r0, depth, thr, kind, policy, dtype,
                    digest_only)


MISE_CASES = [
    _mise(3, 2, 0.0, "noise", "full", "f64"),
    _mise(3, 2, 0.0, "noise", "partial", "f32"),
    _mise(3, 2, 0.0, "ties", "partial+revalue", "f16"),
    _mise(5, 2, 0.25, "noise", "partial", "f16"),
    _mise(5, 2, 0.25, "ties", "full", "f64"),
    _mise(5, 2, 0.25, "sparse", "partial+revalue", "f32"),
    _mise(2, 3, -0.25, "noise", "partial+revalue", "f64"),
    _mise(2, 3, -0.25, "ties", "partial", "f32"),
    _mise(2, 3, -0.25, "noise", "full", "f16"),
    _mise(6, 1, 0.0, "noise", "full", "f32"),
    _mise(6, 1, 0.0, "ties", "partial+revalue", "f64"),
    _mise(6, 1, 0.0, "sparse", "full", "f16"),
    _mise(1, 4, 0.0, "noise", "partial", "f16"),
    _mise(1, 4, 0.0, "ties", "full", "f64"),
    _mise(7, 2, 0.0, "sparse", "partial", "f64"),
    _mise(7, 2, 0.0, "noise", "partial+revalue", "f16"),
    _mise(7, 2, 0.0, "ties", "full", "f32"),
    # r1 = 65: the last rounds return more than 65 536 points, DeviceMISE.query() has to grow its index buffer
    _mise(8, 3, 0.0, "noise", "full", "f32", digest_only=True),
]
MISE_BY_ID = {c.id: c for c in MISE_CASES}
GROWTH_CASE = MISE_CASES[-1].id
MAX_ROUNDS = 500


def mise_r1(case):
    return (case.r0 << case.depth) + 1


def mise_values(case, li):
    """Values of a MISE case at linear indices `li` of its finest (r1, r1, r1) grid, in the case's value dtype.  Every value
    is exactly representable in that dtype, so the reference and the host port, which take float64, get the same numbers."""
    li = np.asarray(li, dtype=np.int64)
    r1, res = mise_r1(case), case.r0 << case.depth
    u = hash01(li, _salt("mise/" + case.id))
    if case.kind == "noise":
        if case.dtype == "f64":
            f = u - 0.5
        elif case.dtype == "f32":
            f = (u - 0.5).astype(np.float32).astype(np.float64)
        else:
            f = (np.floor(u * 64.0) + 0.5) / 64.0 - 0.5          # odd multiples of 1/128: exact in float16, never a tie
    elif case.kind == "sparse":      # isolated positives: hanging points keep flagging coarse neighbours, many rounds
        mag = 0.125 + np.floor(hash01(li, _salt("mise/mag/" + case.id)) * 32.0) / 64.0
        f = np.where(u < 0.02, 1.0, -1.0) * mag
    elif case.kind == "ties":        # a smooth field in steps of 1/4: many values exactly at the threshold
        x, y, z = _coords(li, (r1, r1, r1))
        px, py, pz = x / float(res), y / float(res), z / float(res)
        f = np.round(((2.0 * px - 1.0) * (2.0 * py - 1.0) * 1.5 + (pz - 0.5)) * 4.0) / 4.0
    else:
        raise ValueError(case.kind)
    out = (case.thr + f).astype(NP_DTYPE[case.dtype])
    return out


def run_mise(case, query, update):
    """Drives one MISE instance through the case's answer policy.  `query()` -> the round's points as linear indices (any
    order), `update(li, values)` takes int64 indices and values in the case's dtype.  Returns the list of per-round index
    arrays as query() returned them.  Which points are answered, re-valued and with what depends only on (linear index,
    round), never on the order of the points.
      full             every point is answered
      partial          a point is answered in round k iff hash(li, k) < 0.7; every third round answers everything
      partial+revalue  as partial; odd rounds also re-send a hash-chosen handful of known points with the negated value"""
    n = mise_r1(case) ** 3
    known = np.zeros(n, dtype=bool)
    cur = np.zeros(n, dtype=NP_DTYPE[case.dtype])
    salt = _salt("policy/" + case.id)
    rounds = []
    while True:
        q = np.asarray(query(), dtype=np.int64)
        if not len(q):
            return rounds
        k = len(rounds)
        rounds.append(q)
        assert k < MAX_ROUNDS, case.id
        a = q
        if case.policy != "full" and k % 3 != 2:
            a = q[hash01(q, salt + 2 * k) < 0.7]
        vals = mise_values(case, a)
        if case.policy == "partial+revalue" and k % 2 == 1:
            kn = np.flatnonzero(known)
            pick = kn[hash01(kn, salt + 2 * k + 1) * len(kn) < 4.0]
            a, vals = np.concatenate([a, pick]), np.concatenate([vals, -cur[pick]])
        update(a, vals)
        known[a] = True
        cur[a] = vals


def lin(points, r1):
    p = np.asarray(points, dtype=np.int64).reshape(-1, 3)
    return (p[:, 0] * r1 + p[:, 1]) * r1 + p[:, 2]


def unlin(li, r1):
    li = np.asarray(li, dtype=np.int64)
    return np.stack([li // (r1 * r1), (li // r1) % r1, li % r1], 1)


def drive_host_style(case, m):
    """run_mise on an object with the reference's interface (query() -> (n,3) int64 points, update(points, float64 values)):
    the reference's compiled MISE and slice3d_amd.mesh.MISE.  -> (per-round linear indices in the object's order, dense)."""
    r1 = mise_r1(case)
    rounds = run_mise(case, lambda: lin(m.query(), r1),
                      lambda li, v: m.update(unlin(li, r1), np.asarray(v, dtype=np.float64)))
    return rounds, m.to_dense()


def sha256_u8(*arrays):
    """sha256 over the bytes of the arrays (C order), as 32 uint8: the digest form of the large cases."""
    import hashlib
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return np.frombuffer(h.digest(), dtype=np.uint8).copy()


# ------------------------------------------------------------------------------------------------------------------
# comparing with tests/golden/mesh_extract_reference.npz (gold: its arrays by name)
# ------------------------------------------------------------------------------------------------------------------
def bits_equal(a, b):
    """Same shape, same dtype, same bytes: NaN coordinates and signed zeros compare by their bits."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def mise_sets(gold, case):
    """The reference's per-round sorted index sets of a case with stored indices."""
    ends = np.cumsum(gold["mise/%s/qn" % case.id])
    return np.split(gold["mise/%s/q" % case.id].astype(np.int64), ends[:-1])


def check_mise_against_golden(gold, case, rounds, dense):
    """rounds: per-round int64 linear indices in any order; dense: the final float64 grid."""
    qn = gold["mise/%s/qn" % case.id]
    assert [len(q) for q in rounds] == list(qn)
    if case.digest_only:
        for q, want in zip(rounds, gold["mise/%s/qsha" % case.id]):
            assert np.array_equal(sha256_u8(np.sort(q).astype(np.int32)), want)
        assert np.array_equal(sha256_u8(dense), gold["mise/%s/dsha" % case.id])
    else:
        for k, (q, want) in enumerate(zip(rounds, mise_sets(gold, case))):
            assert np.array_equal(np.sort(q), want), (case.id, k)
        assert bits_equal(dense, gold["mise/%s/dense" % case.id])

"""Inputs, float64 references and gates for the conformance of the query front end: rotation / flip, project_coord, the image-
space locality sort, the bilinear samplers and the token builder (query_geom.h: query_xyz, rotate_query, project, level_cell,
make_taps, make_foot, sort_bin, morton8, tile_origin, tile_footprint; decode.hip: qsort_*, project_coord_kernel,
sample_planes_kernel, sample_pyramid_kernel, sample_tokens_kernel, sample_tokens_gt_kernel, gt_point_tokens_kernel; the
backward kernels of train2.hip / train_sbd.hip, which call the same header).  Nothing here touches a GPU:
tests/test_query_cases.py checks this file on the CPU and tests/test_gpu_query_front_end.py runs it through the entry points.

What slice3d_amd/synth.make_feed_dict cannot give: every object of a batch has its OWN rotation and camera matrix (CAMERAS,
with_cameras), query sets are built from where they must land in the image (on the border, on a pixel centre, all sixteen of
a group inside one pixel cell or far apart), grids leave [-1, 1], and the sort gets inputs whose keys are exact in fp32.

Gate (`gate`): per row  max|out - f64| <= 4 * max|oracle32 - f64| + 2^-22 * max|f64|, never above the project's absolute
bound for the quantity (CAP).  The factor 4 allows another, equally valid operation order; the floor is a quarter ulp of the
largest output.  The right-hand side is formed from the fp32 oracle (oracle/ref_cpu.py) alone, never from the kernels.
"""
import numpy as np
import torch

from oracle import ref_cpu
from slice3d_amd.synth import rotation_az_el

REF_FACTOR = 4.0
FLOOR_REL = 2.0 ** -22
CAP = {"proj": 1e-6, "fc_p": 1e-5, "fc_s": 5e-5, "sdf": 1e-4}     # the project's existing absolute bounds
GRAD_REL_L2 = 2e-2
LOSS_REL = 2e-5
LEVEL_CHANNELS = ref_cpu.LEVEL_CHANNELS


def gate(ref64, ref32, cap=None):
    """-> (bound on max|out - ref64|, e_ref = max|ref32 - ref64|)."""
    e_ref = float((ref32.double() - ref64).abs().max())
    bound = REF_FACTOR * e_ref + FLOOR_REL * float(ref64.abs().max())
    return (bound if cap is None else min(bound, cap)), e_ref


def err(out, ref64):
    d = (out.double() - ref64).abs()
    return float("nan") if bool(torch.isnan(d).any()) else float(d.max())


def _f32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))


# ------------------------------------------------------------------------------------------------------------------ cameras
# (az deg, el deg, focal, distance, centre x, centre y); the first is synth's own
CAMERA_PARAMS = ((-30.0, 20.0, 1.09375, 1.2, 0.5, 0.5), (75.0, -10.0, 0.8, 1.0, 0.45, 0.55), (160.0, 35.0, 1.6, 1.5, 0.5, 0.4))


def make_camera(az, el, f, d, cx, cy):
    trans = np.array([[f, 0, 0], [0, f, 0], [cx, cy, 1], [cx * d, cy * d, d]], dtype=np.float64)
    return _f32(rotation_az_el(az, el)), _f32(trans)


CAMERAS = tuple(make_camera(*p) for p in CAMERA_PARAMS)


def cams_of(batch, first=0):
    return [CAMERAS[(first + b) % len(CAMERAS)] for b in range(batch)]


def with_cameras(fd, cams):
    """A feed dict like `fd` whose obj_rot_mat[b], trans_mat_wo_rot_tp[b] are cams[b]."""
    assert len(cams) == fd["qry_norot"].shape[0]
    out = dict(fd)
    dev = fd["qry_norot"].device
    out["obj_rot_mat"] = torch.stack([c[0] for c in cams]).to(dev).contiguous()
    out["trans_mat_wo_rot_tp"] = torch.stack([c[1] for c in cams]).to(dev).contiguous()
    return out


def rot_trans(cams):
    return torch.stack([c[0] for c in cams]).contiguous(), torch.stack([c[1] for c in cams]).contiguous()


# ------------------------------------------------------------------------------------------------------------------ projection
def rotate(qry, rot, mode, dtype):
    """ref_cpu.rotate_queries in `dtype` (mode 'none': the coordinates are used as they are)."""
    if mode == "none":
        return qry.to(dtype)
    return ref_cpu.rotate_queries({"qry_norot": qry.to(dtype), "obj_rot_mat": rot.to(dtype)}, mode)


def project(qry_rot, trans, dtype):
    return ref_cpu.project_coord(qry_rot.to(dtype), trans.to(dtype))


def project_unclamped64(qry_rot, trans):
    """Float64 image coordinates BEFORE the clamp (numpy): where a query would land were the image unbounded."""
    p = qry_rot.double().numpy()
    t = trans.double().numpy()
    pc = np.einsum("bqk,bkj->bqj", np.concatenate([p, np.ones(p.shape[:2] + (1,))], -1), t)
    return 2.0 * (pc[..., :2] / pc[..., 2:] - 0.5)


def must_be_exact(un64):
    """Where the clamped result must be +-1 to the bit: the unclamped float64 coordinate is +-1 itself or at least the
    project's projection bound (1e-6) outside the image.  (Closer to the border than that, two fp32 evaluations legitimately
    fall on different sides of it: the fp32 oracle itself returns 1 - 2^-24 for float64 values that clamp to 1.)"""
    return (np.abs(un64) == 1.0) | (np.abs(un64) >= 1.0 + CAP["proj"])


def unproject(g, z_rot, cams, mode):
    """Queries (B,Q,3) float32 whose float64 projection through cams[b] is g[b] (up to the rounding of the float32 cast) at
    rotated depth z_rot: x = (u - cx) (z + d) / f with u = g/2 + 1/2, then the inverse of the rotation / flip of `mode`."""
    out = np.empty(g.shape[:2] + (3,), dtype=np.float64)
    for b, (rot, trans) in enumerate(cams):
        t = trans.double().numpy()
        f, cx, cy, d = t[0, 0], t[2, 0], t[2, 1], t[3, 2]
        u = g[b] / 2.0 + 0.5
        zz = z_rot[b] + d
        p = np.stack([(u[:, 0] - cx) * zz / f, (u[:, 1] - cy) * zz / t[1, 1], z_rot[b]], -1)
        if mode == "train":
            p = p @ np.linalg.inv(rot.double().numpy())
        elif mode == "test":
            p = p * np.array([1.0, -1.0, -1.0])
        out[b] = p
    return _f32(out)


# ------------------------------------------------------------------------------------------------------------------ query sets
def uniform(batch, q, seed):
    return _f32(np.random.default_rng(seed).uniform(-0.5, 0.5, (batch, q, 3)))


def pile(batch, q, seed):
    return uniform(batch, 1, seed).expand(batch, q, 3).contiguous()


def _depth(rng, batch, q):
    return rng.uniform(-0.3, 0.3, (batch, q))


def exact_border_points(n):
    """Rotated-space points whose projection through CAMERAS[0] is exactly +1 or -1 in float64 AND in every fp32 evaluation:
    with f = 35/32, c = 1/2 and d = fl32(1.2), z = 35 j / 2^23 - d (j a multiple of 64) makes z + d = 35 j / 2^23 and
    x = +-(z + d) / (2 f) = +-16 j / 2^23 exact, every product and partial sum of X = f x + z / 2 + d / 2 representable, and
    X / Z = 1 or 0.  Rows cycle through (+1, .), (-1, .), (., +1), (., -1), (+1, -1), (-1, +1)."""
    d = float(CAMERAS[0][1][3, 2])
    assert CAMERA_PARAMS[0][2] == 35.0 / 32.0 and CAMERA_PARAMS[0][4:] == (0.5, 0.5)
    j0 = int(np.ceil((d - 0.3) * 2 ** 23 / 35 / 64))
    p = np.empty((n, 3))
    for i in range(n):
        j = 64 * (j0 + 37 * (i % 64))
        zz = 35.0 * j / 2 ** 23
        e = 16.0 * j / 2 ** 23
        other = (i % 7 - 3) / 16.0
        sx, sy = ((1, None), (-1, None), (None, 1), (None, -1), (1, -1), (-1, 1))[i % 6]
        p[i] = (other if sx is None else sx * e, other if sy is None else sy * e, zz - d)
    assert np.abs(p[:, 2]).max() < 0.5
    return p


def border(batch, q, seed, cams=CAMERAS, mode="none"):
    """Rows cycle through eight kinds of image target: both coordinates on +-1 (exact, see exact_border_points, where the
    object's camera is CAMERAS[0] and the mode keeps exactness; else on the border up to rounding), one coordinate 1e-6
    inside / 1e-6 outside / 5e-7 around +-1, far outside (clamped, up to +-4), and interior."""
    rng = np.random.default_rng(seed)
    g = rng.uniform(-0.95, 0.95, (batch, q, 2))
    i = np.arange(q)
    sgn = rng.choice([-1.0, 1.0], (batch, q))
    col = rng.integers(0, 2, (batch, q))
    kind = i % 8
    off = np.select([kind == 0, kind == 1, kind == 2, kind == 3, kind == 4, kind == 5],
                    [0.0, -1e-6, 1e-6, 5e-7, -5e-7, 0.5], 0.0)
    far = rng.uniform(1.0, 3.0, (batch, q))
    val = sgn * (1.0 + np.where(kind == 5, far, off))
    on = kind <= 5
    for c in (0, 1):
        g[..., c] = np.where(on & (col == c), val, g[..., c])
    both = kind == 6                     # a corner, far outside in both coordinates
    g[:, both] = (sgn[:, both] * (1.0 + far[:, both]))[..., None] * np.array([1.0, -1.0])
    out = unproject(g, _depth(rng, batch, q), cams, mode)
    for b, cam in enumerate(cams):
        if cam is CAMERAS[0] and mode in ("none", "test"):
            rows = np.nonzero(kind == 0)[0]
            p = exact_border_points(len(rows))
            if mode == "test":
                p = p * np.array([1.0, -1.0, -1.0])
            out[b, rows] = _f32(p)
    return out


def level_widths(size):
    return [(size // 16) << l for l in range(5)]


def centres(batch, q, seed, cams=CAMERAS, mode="none", size=32):
    """Row i projects onto a pixel centre gx = 2 k / (W - 1) - 1 of pyramid level i % 5 (level 0 first)."""
    rng = np.random.default_rng(seed)
    g = np.zeros((batch, q, 2))
    ws = level_widths(size)
    for i in range(q):
        w = ws[i % 5]
        k = rng.integers(0, w, (batch, 2))
        g[:, i] = 2.0 * k / (w - 1) - 1.0 if w > 1 else 0.0
    return unproject(g, _depth(rng, batch, q), cams, mode)


def neighbours(batch, q, seed, cams=CAMERAS, mode="none", size=32):
    """Every group of 16 consecutive queries projects into ONE level-2 pixel cell (5 % margin from its edges)."""
    rng = np.random.default_rng(seed)
    w2 = level_widths(size)[2]
    ng = (q + 15) // 16
    cell = rng.integers(0, w2 - 1, (batch, ng, 1, 2)).astype(np.float64)
    t = rng.uniform(0.05, 0.95, (batch, ng, 16, 2))
    g = (2.0 * (cell + t) / (w2 - 1) - 1.0).reshape(batch, ng * 16, 2)[:, :q]
    return unproject(g, _depth(rng, batch, q), cams, mode)


def scattered(batch, q, seed, cams=CAMERAS, mode="none", size=32):
    """Consecutive queries alternate between opposite corners of the image: a group of two or more spans the whole level 2."""
    rng = np.random.default_rng(seed)
    s = np.where(np.arange(q) % 2 == 0, -1.0, 1.0)[None, :, None]
    g = s * rng.uniform(0.8, 0.95, (batch, q, 2))
    return unproject(g, _depth(rng, batch, q), cams, mode)


QUERY_SETS = {"uniform": uniform, "border": border, "centres": centres, "pile": pile, "neighbours": neighbours,
              "scattered": scattered}


def query_set(name, batch, q, seed, cams=CAMERAS, mode="none", size=32):
    if name in ("uniform", "pile"):
        return QUERY_SETS[name](batch, q, seed)
    if name == "border":
        return border(batch, q, seed, cams, mode)
    return QUERY_SETS[name](batch, q, seed, cams, mode, size)


def footprint_extents(g32, size):
    """make_foot's floor cells restated in numpy float32: per group of 16 consecutive queries (the last one ragged) and level
    0..2 the extent max - min of x0 and of y0 -> (B, groups, 3, 2) ints, and whether any floor cell is negative."""
    g = g32.numpy().astype(np.float32)
    b, q, _ = g.shape
    ng = (q + 15) // 16
    ext = np.zeros((b, ng, 3, 2), dtype=np.int64)
    neg = False
    for l in range(3):
        w = np.float32(level_widths(size)[l] - 1)
        cell = np.floor(((g + np.float32(1)) / np.float32(2)) * w).astype(np.int64)
        neg = neg or bool((cell < 0).any())
        for k in range(ng):
            c = cell[:, 16 * k:16 * k + 16]
            ext[:, k, l] = c.max(1) - c.min(1)
    return ext, neg


def window_eligible(g32, size):
    """(B, groups) bool: the group takes the shared-window form of sample_tokens_kernel (extent <= 2 in x and y, levels 0-2)."""
    ext, neg = footprint_extents(g32, size)
    assert not neg
    return (ext <= 2).all(axis=(2, 3))


# ------------------------------------------------------------------------------------------------------------------ grid sets
def grid_uniform(n, m, seed):
    return _f32(np.random.default_rng(seed).uniform(-1.3, 1.3, (n, m, 2)))


def grid_pm1(n, m, seed):
    """x or y or both exactly +-1; the other coordinate uniform in [-1.3, 1.3]."""
    rng = np.random.default_rng(seed)
    g = rng.uniform(-1.3, 1.3, (n, m, 2))
    s = rng.choice([-1.0, 1.0], (n, m, 2))
    kind = np.arange(m) % 3
    g[:, kind == 0, 0] = s[:, kind == 0, 0]
    g[:, kind == 1, 1] = s[:, kind == 1, 1]
    g[:, kind == 2] = s[:, kind == 2]
    return _f32(g)


def grid_centres(n, m, seed, w, h):
    rng = np.random.default_rng(seed)
    kx, ky = rng.integers(0, w, (n, m)), rng.integers(0, h, (n, m))
    gx = 2.0 * kx / (w - 1) - 1.0 if w > 1 else np.zeros((n, m))
    gy = 2.0 * ky / (h - 1) - 1.0 if h > 1 else np.zeros((n, m))
    return _f32(np.stack([gx, gy], -1))


def grid_pile(n, m, seed):
    return grid_uniform(n, 1, seed).expand(n, m, 2).contiguous()


WALK_CELLS = lambda w: (-1, 0, 0, -1, w - 2, w - 1, w - 1)
WALK_FRACS = (0.25, 0.5, 0.75, 0.125)


def _walk_axis(w, rep):
    """Coordinates whose floor cells are WALK_CELLS(w), fraction WALK_FRACS[rep + step]; W = 1 has no cells: -1.2 ... 1.2."""
    if w == 1:
        return [-1.2, -1.0, 0.0, 0.5, 1.0, 1.2, -0.3]
    return [2.0 * (c + WALK_FRACS[(rep + i) % 4]) / (w - 1) - 1.0 for i, c in enumerate(WALK_CELLS(w))]


def grid_walk(n, m, sizes, seed=0):
    """Consecutive rows whose floor cells visit x0 = -1, 0, 0, -1, W-2, W-1, W-1 at a fixed y, then the same in y at a fixed
    x, for every (W, H) of `sizes` in turn, repeated with other fractions (and, per image, another fixed coordinate) until M
    rows: rows with equal and with unequal clamped first-tap offsets follow each other, in and out of range."""
    rng = np.random.default_rng(seed)
    g = np.empty((n, m, 2))
    for ni in range(n):
        rows, rep = [], 0
        while len(rows) < m:
            for (w, h) in sizes:
                fixed = rng.choice([-1.1, -1.0, -0.4, 0.3, 1.0, 1.1], 2)
                rows += [(x, fixed[1]) for x in _walk_axis(w, rep)]
                rows += [(fixed[0], y) for y in _walk_axis(h, rep)]
            rep += 1
        g[ni] = np.array(rows[:m])
    return _f32(g)


def plane_grid_sets(n, m, w, h, seed):
    return {"uniform": grid_uniform(n, m, seed), "pm1": grid_pm1(n, m, seed + 1), "centres": grid_centres(n, m, seed + 2, w, h),
            "walk": grid_walk(n, m, [(w, h)], seed + 3)}


def pyramid_grid(name, batch, q, size, seed):
    if name == "uniform":
        return grid_uniform(batch, q, seed)
    if name == "pile":
        return grid_pile(batch, q, seed)
    assert name == "walk"
    return grid_walk(batch, q, [(w, w) for w in level_widths(size)], seed)


def floor_cells32(g32, w):
    """floor of make_taps' ix in numpy float32."""
    g = g32.numpy().astype(np.float32)
    return np.floor(((g + np.float32(1)) / np.float32(2)) * np.float32(w - 1)).astype(np.int64)


# ------------------------------------------------------------------------------------------------------------------ sampling
PLANE_SHAPES = ((1, 1, 4), (1, 9, 8), (5, 7, 36), (16, 16, 128), (64, 64, 32))      # (H, W, C), N = 3
PLANE_M = (1, 63, 1000)


def planes(n, h, w, c, seed):
    """(N, H, W, C) channels-last random normal planes."""
    return torch.randn(n, h, w, c, generator=torch.Generator().manual_seed(seed))


def sample_planes_ref(plane_nhwc, grid, dtype):
    """(N, M, C) in `dtype` through ref_cpu.sample_from_planes (torch grid_sample)."""
    return ref_cpu.sample_from_planes(plane_nhwc.permute(0, 3, 1, 2).to(dtype), grid.to(dtype)).squeeze(1)


def pyramid(n_img, size, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(n_img, w, w, c, generator=g) for w, c in zip(level_widths(size), LEVEL_CHANNELS)]


def sample_pyramid_ref(pyr_nhwc, grid, n_slices, dtype):
    """(B*n_slices, Q, 992): the layout of s3d_sample_pyramid_fwd's result."""
    pts = grid.to(dtype)
    b, q, _ = pts.shape
    pts = pts.view(b, 1, q, 2).expand(-1, n_slices, -1, -1).reshape(b * n_slices, q, 2)
    return torch.cat([ref_cpu.sample_from_planes(p.permute(0, 3, 1, 2).to(dtype), pts).squeeze(1) for p in pyr_nhwc], 2)


PYR_Q = (1, 127, 128, 129, 4095, 4096, 4097)


def token_rows_ref(sd, pyr_nhwc, qry, cams, mode, n_slices, dtype):
    """fc_p (B,Q,128) and fc_s (B,Q,n_slices,128) in `dtype`: ref_cpu.rotate_queries, project_coord, sample_pyramid and the
    token layer of decode_tokens(..., return_layers=True) on the given (channels-last) pyramid."""
    rot, trans = rot_trans(cams)
    sdd = {k: v.to(dtype) for k, v in sd.items() if k.startswith(("fc_p.", "fc_s.", "att_decoder.", "fc_out."))}
    qr = rotate(qry, rot, mode, dtype)
    pts = project(qr, trans, dtype)
    b, q, _ = qr.shape
    with torch.no_grad():
        tok = ref_cpu.sample_pyramid([p.permute(0, 3, 1, 2).to(dtype) for p in pyr_nhwc], pts, n_slices)
        _, layers = ref_cpu.decode_tokens(sdd, tok, qr, return_layers=True)
    x = layers[0].view(b, q, n_slices + 1, 128)
    return x[:, :, 0], x[:, :, 1:]


# ------------------------------------------------------------------------------------------------------------------ sort keys
def morton_key(g):
    """Key of s3d_query_sort for projected coordinates g (..., 2) (numpy float64 or float32), written from the header's
    contract: bin = floor(clamp((g + 1) * 127.5, 0, 255)) per axis, bits interleaved with x in the even positions."""
    t = np.clip((g + 1.0) * 127.5, 0.0, 255.0)
    bx, by = np.floor(t[..., 0]).astype(np.int64), np.floor(t[..., 1]).astype(np.int64)
    key = np.zeros_like(bx)
    for i in range(8):
        key |= ((bx >> i) & 1) << (2 * i)
        key |= ((by >> i) & 1) << (2 * i + 1)
    return key


def edge_distance(g_unclamped):
    """Distance (in bin widths) of the unclamped float64 bin coordinate to the nearest bin edge 1 ... 255, the smaller of x
    and y.  Coordinates below 0 or above 255 sit in bin 0 / 255 whatever their rounding: only edges 1 and 255 count there."""
    t = (g_unclamped + 1.0) * 127.5
    e = np.clip(np.round(t), 1.0, 255.0)
    return np.abs(t - e).min(-1)


SORT_EDGE_EXCLUSION = 1e-3      # bin widths
SORT_EXCLUSION_CAP = 0.01       # of all queries


def expected_perm(keys):
    """Ascending key, ascending query index inside a key: a stable argsort per object."""
    return np.stack([np.argsort(k, kind="stable") for k in keys])


def sort_camera_inputs(seed=31, batch=3, q=30000):
    """uniform + pile + clamped queries for the CAMERAS sort row: object 0 repeats one point 5000 times (one bin of
    thousands: the rank sort), object 1 has 2900 queries thrown far outside the image (x, y times 40)."""
    qry = uniform(batch, q, seed).clone()
    qry[0, :5000] = qry[0, 0]
    qry[1, 100:3000, :2] *= 40.0
    return qry


def sort_camera_keys(qry, cams, mode):
    """-> (float64 keys (B,Q), keep mask (B,Q): farther than SORT_EDGE_EXCLUSION from every bin edge, fp32-oracle keys)."""
    rot, trans = rot_trans(cams)
    qr64 = rotate(qry, rot, mode, torch.float64)
    k64 = morton_key(project(qr64, trans, torch.float64).numpy())
    keep = edge_distance(project_unclamped64(qr64, trans)) >= SORT_EDGE_EXCLUSION
    k32 = morton_key(project(rotate(qry, rot, mode, torch.float32), trans, torch.float32).numpy().astype(np.float32))
    return k64, keep, k32


def strictly_increasing_kept(perm, keys, keep):
    """The kept queries of one object appear in strictly increasing (key, index) order in `perm` (numpy int64 (Q,))."""
    p = perm[keep[perm]]
    comp = keys[p] * len(perm) + p
    return bool((comp[1:] > comp[:-1]).all())


# exact-key sort inputs: X = x, Y = y, Z = 1
SORT_TRANS = ((1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 0.0), (0.0, 0.0, 1.0))
SORT_ROTS = (((0, 1, 0), (0, 0, -1), (-1, 0, 0)), ((0, 0, 1), (-1, 0, 0), (0, -1, 0)), ((-1, 0, 0), (0, 0, 1), (0, 1, 0)))
SORT_Q = (1, 31, 4096, 30000)
SORT_BIN_SIZES = (1, 2, 32, 33, 400, 700)     # 32 | 33: the insertion-sort / rank-sort boundary of qsort_fix_kernel
SORT_SPECIAL_KX = (3, 10, 50, 100, 200, 250)


def bin_of(k):
    """Bin of the coordinate (2k+1)/512 in integers: (g + 1) * 127.5 = (2k+1) * 255 / 512."""
    return ((2 * k + 1) * 255) // 512


def sort_exact_inputs(q, variant, seed=0, batch=3):
    """-> qry (B,Q,3) float32, rot (B,3,3), trans (B,4,3), keys (B,Q) int64 (integer arithmetic), bin sizes (list per object).
    variant 'rot': per-object signed permutation matrices; 'flip': the mode='test' prologue (rot is still returned: the
    kernel must ignore it).  Bins of exactly SORT_BIN_SIZES members as far as Q allows, the rest spread at random over
    bins of other columns; query order shuffled."""
    rng = np.random.default_rng(seed + q)
    ks = np.empty((batch, q, 2), dtype=np.int64)
    free = np.array([k for k in range(256) if k not in SORT_SPECIAL_KX and k != 128])    # k = 127 and 128 share a bin
    for b in range(batch):
        rows = []
        for i, n in enumerate(SORT_BIN_SIZES):
            if len(rows) + n > q:
                break
            rows += [(SORT_SPECIAL_KX[i], (17 * b + 40 * i + 5) % 256)] * n
        rest = q - len(rows)
        rows += list(zip(rng.choice(free, rest), rng.integers(0, 256, rest)))
        ks[b] = np.array(rows, dtype=np.int64).reshape(q, 2)[rng.permutation(q)]
    xy = (2 * ks + 1) / 512.0
    p = np.concatenate([xy, rng.integers(-64, 64, (batch, q, 1)) / 128.0], -1)      # rotated space
    rot = np.array(SORT_ROTS, dtype=np.float64)[:batch]
    if variant == "rot":
        qry = np.einsum("bqk,bjk->bqj", p, rot)         # p @ rot^T: exact for signed permutations
    else:
        assert variant == "flip"
        qry = p * np.array([1.0, -1.0, -1.0])
    bx, by = bin_of(ks[..., 0]), bin_of(ks[..., 1])
    keys = np.zeros_like(bx)
    for i in range(8):
        keys |= ((bx >> i) & 1) << (2 * i)
        keys |= ((by >> i) & 1) << (2 * i + 1)
    sizes = [np.bincount(keys[b]) for b in range(batch)]
    return _f32(qry), _f32(rot), _f32(np.array(SORT_TRANS))[None].repeat(batch, 1, 1).contiguous(), keys, sizes


# ------------------------------------------------------------------------------------------------------------------ layout / MISE
NCHW_SHAPES = ((1, 3, 5, 7), (2, 36, 1, 9), (3, 128, 16, 16))
MISE_CASES = ((5, 4), (16, 2), (3, 0))      # (resolution0, depth)
MISE_BOXES = (1.0, 1.1)


def mise_points_ref(coords, resolution, box):
    """reconstruct.py:160-161 in numpy float32: box * (p / resolution - 0.5)."""
    return np.float32(box) * (coords.astype(np.float32) / np.float32(resolution) - np.float32(0.5))

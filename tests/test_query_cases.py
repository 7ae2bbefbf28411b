"""CPU checks of tests/query_cases.py, the inputs / references / gates of tests/test_gpu_query_front_end.py: the two bilinear
restatements of the oracle agree in float64 on every grid set (out of range included), every query set has the property its
name promises (footprint arithmetic restated in numpy float32), the exact-key sort inputs are exact, the exclusion cap of the
camera sort row holds, every gate of the GPU file is met by the fp32 oracle alone, and the float64 references are quick."""
import time

import numpy as np
import pytest
import torch

import query_cases as K
from helpers import GOLDEN, seeded_sd_from_shapes
from oracle import ref_cpu

F64, F32 = torch.float64, torch.float32
MODES = ("none", "train", "test")


def test_cameras_differ_in_every_entry_and_the_first_is_synths():
    from slice3d_amd import synth
    fd = synth.make_feed_dict(3, 16, 4, 1, seed=0, with_slices=False)
    assert torch.equal(K.CAMERAS[0][0], fd["obj_rot_mat"][0]) and torch.equal(K.CAMERAS[0][1], fd["trans_mat_wo_rot_tp"][0])
    fd2 = K.with_cameras(fd, K.CAMERAS)
    assert fd2["qry_norot"] is fd["qry_norot"] and torch.equal(fd["obj_rot_mat"][1], fd["obj_rot_mat"][0])   # synth untouched
    for b in range(3):
        assert torch.equal(fd2["obj_rot_mat"][b], K.CAMERAS[b][0]) and torch.equal(fd2["trans_mat_wo_rot_tp"][b], K.CAMERAS[b][1])
    for a in range(3):
        for b in range(a + 1, 3):
            assert bool((K.CAMERAS[a][0] != K.CAMERAS[b][0])[:2].all()) and bool((K.CAMERAS[a][0] - K.CAMERAS[b][0]).abs().max() > 0.3)
            ta, tb = K.CAMERAS[a][1], K.CAMERAS[b][1]
            assert ta[0, 0] != tb[0, 0] and ta[1, 1] != tb[1, 1] and ta[3, 2] != tb[3, 2]      # focal length, distance
            assert not torch.equal(ta[2, :2], tb[2, :2]) and not torch.equal(ta[3, :2], tb[3, :2])   # centre, centre * distance
            assert K.CAMERA_PARAMS[a][4:] != K.CAMERA_PARAMS[b][4:]


# ------------------------------------------------------------------------------------------------------------------ bilinear
@pytest.mark.parametrize("h,w", [(1, 1), (1, 9), (5, 7), (16, 16)])
def test_the_two_bilinear_restatements_agree_in_float64(h, w):
    pl = K.planes(3, h, w, 8, seed=h * 100 + w)
    worst = 0.0
    for name, grid in K.plane_grid_sets(3, 257, w, h, seed=7).items():
        a = K.sample_planes_ref(pl, grid, F64)
        b = ref_cpu.bilinear_sample_manual(pl.permute(0, 3, 1, 2).double(), grid.double())
        worst = max(worst, float((a - b).abs().max()))
        assert float((a - b).abs().max()) <= 1e-12, (name, h, w)
    print("bilinear restatements %dx%d: %.1e" % (h, w, worst))


@pytest.mark.parametrize("w", [2, 3, 7, 16, 64])
def test_walk_visits_the_border_cells_in_fp32(w):
    """Rows 0-6 walk x at a fixed y, rows 7-13 walk y at a fixed x; in numpy float32 (make_taps' arithmetic) the floor cells are
    -1, 0, 0, -1, W-2, W-1, W-1: equal and unequal clamped first-tap offsets follow each other on both sides of both borders."""
    g = K.grid_walk(2, 56, [(w, w)], seed=3)
    cells = K.floor_cells32(g, w)
    want = np.array(K.WALK_CELLS(w))
    for n in range(2):
        for rep in range(4):
            r = 14 * rep
            assert np.array_equal(cells[n, r:r + 7, 0], want) and np.array_equal(cells[n, r + 7:r + 14, 1], want)
            assert len(set(g[n, r:r + 7, 1].tolist())) == 1 and len(set(g[n, r + 7:r + 14, 0].tolist())) == 1
    clamped = np.clip(cells[0, :7, 0], 0, w - 1)
    assert (clamped[1:] == clamped[:-1]).any() and (clamped[1:] != clamped[:-1]).any()


def test_grid_sets_leave_the_image():
    for name, g in K.plane_grid_sets(3, 1000, 7, 5, seed=1).items():
        if name != "centres":
            assert float(g.max()) > 1.0 and float(g.min()) < -1.0 or name == "pm1" and bool((g.abs() == 1).any()), name
    assert bool((K.grid_pm1(3, 99, 0).abs() == 1).any(-1).all())
    assert float(K.grid_uniform(2, 4096, 0).abs().max()) > 1.25
    p = K.grid_pile(2, 50, 4)
    assert bool((p == p[:, :1]).all()) and not torch.equal(p[0], p[1])
    w = K.pyramid_grid("walk", 2, 200, 32, 0)
    for wl in K.level_widths(32):
        assert -1 in K.floor_cells32(w, wl) and (wl - 1) in K.floor_cells32(w, wl)


# ------------------------------------------------------------------------------------------------------------------ query sets
def _g32(name, q, mode, seed=11, batch=3, size=32):
    cams = K.cams_of(batch)
    qry = K.query_set(name, batch, q, seed, cams, mode, size)
    rot, trans = K.rot_trans(cams)
    return qry, K.project(K.rotate(qry, rot, mode, F32), trans, F32), K.project(K.rotate(qry, rot, mode, F64), trans, F64)


@pytest.mark.parametrize("mode", MODES)
def test_query_sets_have_the_properties_their_names_promise(mode):
    for q in (17, 250):
        _, g32, _ = _g32("neighbours", q, mode)
        ext, neg = K.footprint_extents(g32, 32)
        assert not neg and int(ext.max()) <= 2 and bool(K.window_eligible(g32, 32).all())
        assert int(ext[:, :, 2].max()) == 0                          # one level-2 cell per group
        _, g32, _ = _g32("scattered", q, mode)
        el = K.window_eligible(g32, 32)
        assert not el[:, :q // 16].any()                             # every full group takes the per-lane form
        assert el[:, q // 16:].all() == (q % 16 == 1)                # (a last group of ONE query always fits)
        _, g32, _ = _g32("uniform", q, mode)
        assert not K.window_eligible(g32, 32)[:, :q // 16].all()
    qry, g32, g64 = _g32("pile", 250, mode)
    assert bool((qry == qry[:, :1]).all()) and bool(K.window_eligible(g32, 32).all())
    _, g32, g64 = _g32("centres", 250, mode)
    for i in range(250):
        w = K.level_widths(32)[i % 5]
        ix = (g64[:, i].numpy() + 1) / 2 * (w - 1)
        assert np.abs(ix - np.round(ix)).max() < 1e-5, (i, ix)
    _, g32, g64 = _g32("border", 250, mode)
    g = g64.numpy()
    assert (np.abs(g) == 1).sum() > 250                              # clamped and exact rows
    near = (np.abs(np.abs(g) - 1) < 2e-6) & (np.abs(g) != 1)
    assert near.sum() >= 30                                          # just inside
    assert (np.abs(g).max(-1) < 0.96).sum() >= 60                    # interior rows


@pytest.mark.parametrize("mode", ["none", "test"])
def test_border_contains_exact_plus_and_minus_one(mode):
    """The kind-0 rows of the CAMERAS[0] object project to exactly +-1 WITHOUT the clamp, in float64 and in the fp32 oracle."""
    cams = K.cams_of(3)
    qry = K.border(3, 250, 11, cams, mode)
    rot, trans = K.rot_trans(cams)
    un = K.project_unclamped64(K.rotate(qry, rot, mode, F64), trans)[0, 0::8]
    g32 = K.project(K.rotate(qry, rot, mode, F32), trans, F32)[0, 0::8].numpy()
    on = np.abs(un) == 1.0
    assert on.any(-1).all() and (un[on] == 1).any() and (un[on] == -1).any()
    assert np.array_equal(g32[on].astype(np.float64), un[on])


# ------------------------------------------------------------------------------------------------------------------ gates, oracle alone
@pytest.mark.parametrize("name", ["uniform", "border"])
@pytest.mark.parametrize("q", [1, 255, 257, 350000])
def test_fp32_oracle_meets_the_projection_gate(q, name):
    cams = K.cams_of(3)
    coords = K.query_set(name, 3, q, 100 + q, cams, "none")
    _, trans = K.rot_trans(cams)
    t0 = time.perf_counter()
    r64 = K.project(coords, trans, F64)
    dt = time.perf_counter() - t0
    r32 = K.project(coords, trans, F32)
    bound, e_ref = K.gate(r64, r32, K.CAP["proj"])
    assert e_ref <= bound and e_ref <= 3.5e-7, (e_ref, bound)
    ex = K.must_be_exact(K.project_unclamped64(coords, trans))
    assert np.array_equal(r32.numpy()[ex].astype(np.float64), r64.numpy()[ex])
    if name == "border":
        assert ex.sum() >= q // 4
    assert dt < 1.0, dt


_pyr_cache = {}


def oracle_pyramid(ns, size=32):
    """(state dict, channels-last fp32 pyramid of the oracle's U-Net on three smooth images): what the token rows are sampled from."""
    import json
    import os
    from slice3d_amd import synth
    if ns not in _pyr_cache:
        shapes = {k: tuple(v) for k, v in json.load(open(os.path.join(GOLDEN, "state_dict_keys.json"))).items()}
        shapes["slices_generator.emds.weight"] = (ns, 128)
        sd = seeded_sd_from_shapes(shapes)
        fd = synth.make_feed_dict(3, size, 1, ns, seed=77, with_slices=False)
        with torch.no_grad():
            feats, _ = ref_cpu.unet_forward(sd, fd["img_input"], ns)
        _pyr_cache[ns] = sd, [f.permute(0, 2, 3, 1).contiguous() for f in feats]
    return _pyr_cache[ns]


@pytest.mark.parametrize("mode", ["train", "test"])
@pytest.mark.parametrize("ns", [12, 3])
def test_fp32_oracle_meets_the_token_gates(ns, mode):
    sd, pyr = oracle_pyramid(ns)
    cams = K.cams_of(3)
    worst = {"fc_p": 0.0, "fc_s": 0.0}
    for q in (1, 17, 250):
        for name in ("uniform", "border", "centres", "neighbours", "scattered"):
            qry = K.query_set(name, 3, q, 500 + q, cams, mode)
            t0 = time.perf_counter()
            p64, s64 = K.token_rows_ref(sd, pyr, qry, cams, mode, ns, F64)
            dt = time.perf_counter() - t0
            p32, s32 = K.token_rows_ref(sd, pyr, qry, cams, mode, ns, F32)
            for key, r64, r32 in (("fc_p", p64, p32), ("fc_s", s64, s32)):
                bound, e_ref = K.gate(r64, r32, K.CAP[key])
                worst[key] = max(worst[key], e_ref)
                assert e_ref <= bound, (key, name, q, e_ref, bound)
            assert dt < 1.0, (name, q, dt)
    print("fp32 oracle token rows ns=%d %s: fc_p %.2e fc_s %.2e" % (ns, mode, worst["fc_p"], worst["fc_s"]))


def test_sampling_references_are_quick():
    pl = K.planes(3, 64, 64, 32, seed=1)
    grid = K.grid_uniform(3, 1000, 2)
    t0 = time.perf_counter()
    K.sample_planes_ref(pl, grid, F64)
    assert time.perf_counter() - t0 < 1.0
    pyr = K.pyramid(2 * 3, 32, seed=3)
    grid = K.pyramid_grid("uniform", 2, 4097, 32, 4)
    t0 = time.perf_counter()
    r64 = K.sample_pyramid_ref(pyr, grid, 3, F64)
    assert time.perf_counter() - t0 < 1.0
    r32 = K.sample_pyramid_ref(pyr, grid, 3, F32)
    bound, e_ref = K.gate(r64, r32)
    assert r64.shape == (6, 4097, 992) and 0 < e_ref <= bound


# ------------------------------------------------------------------------------------------------------------------ sort
@pytest.mark.parametrize("variant", ["rot", "flip"])
@pytest.mark.parametrize("q", K.SORT_Q)
def test_exact_key_sort_inputs_are_exact(q, variant):
    qry, rot, trans, keys, sizes = K.sort_exact_inputs(q, variant)
    mode = "train" if variant == "rot" else "test"
    assert len({tuple(r.reshape(-1).tolist()) for r in rot}) == 3
    for r in rot:                                                     # signed permutation matrices
        assert torch.equal(r.abs().sum(0), torch.ones(3)) and torch.equal(r.abs().sum(1), torch.ones(3)) and set(r.reshape(-1).tolist()) <= {0.0, 1.0, -1.0}
    g64 = K.project(K.rotate(qry, rot, mode, F64), trans, F64).numpy()
    g32 = K.project(K.rotate(qry, rot, mode, F32), trans, F32).numpy()
    assert np.array_equal(g32.astype(np.float64), g64)                # every fp32 operation is exact
    t = (g64 + 1.0) * 127.5
    assert np.array_equal(((g32 + np.float32(1)) * np.float32(127.5)).astype(np.float64), t)
    assert np.abs(t - np.round(t)).min() >= 1.0 / 512 - 1e-12         # no query closer than 1/512 to a bin edge
    assert np.array_equal(K.morton_key(g64), keys) and np.array_equal(K.morton_key(g32), keys)
    perm = K.expected_perm(keys)
    for b in range(3):
        assert np.array_equal(np.sort(perm[b]), np.arange(q))
        comp = keys[b][perm[b]] * q + perm[b]
        assert (comp[1:] > comp[:-1]).all()
        have = set(sizes[b].tolist())
        want = {1} if q == 1 else {1, 2} if q == 31 else {1, 2, 32, 33, 400, 700}
        assert want <= have, (q, b)
        if q >= 4096:                                                  # several hundred members: the rank sort in more than one pass
            assert max(have) == 700
    if q > 1:
        assert not np.array_equal(perm[0], perm[1]) and not np.array_equal(perm[1], perm[2])


@pytest.mark.parametrize("mode", ["train", "test"])
def test_camera_sort_row_exclusion_cap_and_fp32_oracle(mode):
    qry = K.sort_camera_inputs()
    k64, keep, k32 = K.sort_camera_keys(qry, K.cams_of(3), mode)
    excluded = 1.0 - keep.mean()
    print("camera sort row (%s): %.2f %% of the queries within %g bin widths of an edge" % (mode, 100 * excluded, K.SORT_EDGE_EXCLUSION))
    assert excluded <= K.SORT_EXCLUSION_CAP
    perm32 = K.expected_perm(k32)                                      # what a correct fp32 implementation returns
    for b in range(3):
        assert K.strictly_increasing_kept(perm32[b], k64[b], keep[b])
        assert np.bincount(k64[b]).max() >= (5000 if b == 0 else 300 if b == 1 else 1)
    assert not K.strictly_increasing_kept(perm32[0], k64[1], keep[1])  # the keys of another object's camera do not pass
    rot, trans = K.rot_trans(K.cams_of(3))
    clamped = (np.abs(K.project(K.rotate(qry, rot, mode, F64), trans, F64).numpy()) == 1).any(-1)
    assert (clamped.mean(1) > 0.05).all()


def test_uniform_queries_clamp_for_every_camera():
    """10 - 24 % of uniform queries of each object leave the image (the figures the case table was chosen by)."""
    cams = K.cams_of(3)
    rot, trans = K.rot_trans(cams)
    for mode in ("train", "test"):
        g = K.project(K.rotate(K.uniform(3, 20000, 1), rot, mode, F64), trans, F64).numpy()
        frac = (np.abs(g) == 1).any(-1).mean(1)
        assert (frac > 0.05).all() and (frac < 0.35).all(), frac


def test_mise_reference_is_float32():
    c = np.arange(30).reshape(10, 3)
    for box in K.MISE_BOXES:
        r = K.mise_points_ref(c, 80, box)
        assert r.dtype == np.float32

"""Conformance of the query front end against float64, with a different rotation and camera matrix for every object of the batch:
s3d_project_coord_fwd, s3d_sample_planes_fwd, s3d_sample_pyramid_fwd, s3d_query_sort, the token builder (sample_tokens_kernel,
through Slices3DRegModel.decode_stages), the Reg / GT forward and one training step of each trainer end to end, DeviceMISE.points
and the two layout helpers.  Inputs, references and gates are in tests/query_cases.py (checked on the CPU by
tests/test_query_cases.py); nothing here reads a file outside the repository.

Gate of every row stated against float64: max|hip - f64| <= 4 * max|oracle32 - f64| + 2^-22 * max|f64|, capped by the project's
absolute bound for the quantity (query_cases.gate).  Each row prints `ROW id e_kernel e_ref bound` before it asserts
(profiles/query_front_end_conformance.md).  Stand-alone ops write into NaN-prefilled buffers between guards."""

import numpy as np
import pytest
import torch

import query_cases as K
from helpers import GOLDEN, seeded_sd_from_shapes

pytestmark = pytest.mark.gpu

F64, F32 = torch.float64, torch.float32
GUARD = 256
NAN_BITS = 0x7FC5A5A5
PRECS = ("f32", "f16x3")


def _lib():
    from slice3d_amd import _lib as L
    return L, L.load()


def _guarded(shape, dtype=torch.float32):
    n = int(np.prod(shape))
    buf = torch.full((GUARD + n + GUARD,), NAN_BITS, dtype=torch.int32, device="cuda")
    return buf, buf[GUARD:GUARD + n].view(dtype).view(shape)


def _guards_intact(buf):
    return bool((buf[:GUARD] == NAN_BITS).all()) and bool((buf[-GUARD:] == NAN_BITS).all())


def _bits_equal(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _row(name, out, r64, r32, cap=None):
    bound, e_ref = K.gate(r64, r32, cap)
    e = K.err(out.cpu(), r64)
    print("ROW %s e_kernel %.3e e_ref %.3e bound %.3e" % (name, e, e_ref, bound))
    return e, bound


# ------------------------------------------------------------------------------------------------------------------ project_coord
@pytest.mark.parametrize("name", ["uniform", "border"])
@pytest.mark.parametrize("q", [1, 255, 257, 350000])
def test_project_coord_matches_fp64_per_camera(q, name):
    """B = 3, every object its own camera; 350 000 queries per object make the grid-stride loop run twice.  Where the float64
    coordinate is +-1 before the clamp or at least 1e-6 outside the image the result is +-1 to the bit (query_cases.must_be_exact)."""
    L, lib = _lib()
    cams = K.cams_of(3)
    coords = K.query_set(name, 3, q, 100 + q, cams, "none")
    _, trans = K.rot_trans(cams)
    r64, r32 = K.project(coords, trans, F64), K.project(coords, trans, F32)
    cg, tg = coords.cuda(), trans.cuda()
    buf, out = _guarded((3, q, 2))
    L.check(lib.s3d_project_coord_fwd(cg.data_ptr(), tg.data_ptr(), out.data_ptr(), 3, q, None), "s3d_project_coord_fwd")
    torch.cuda.synchronize()
    assert _guards_intact(buf)
    e, bound = _row("project-%s-q%d" % (name, q), out, r64, r32, K.CAP["proj"])
    assert e <= bound
    ex = K.must_be_exact(K.project_unclamped64(coords, trans))
    assert np.array_equal(out.cpu().numpy()[ex].astype(np.float64), r64.numpy()[ex])


# ------------------------------------------------------------------------------------------------------------------ sample_planes
@pytest.mark.parametrize("m", K.PLANE_M)
@pytest.mark.parametrize("h,w,c", K.PLANE_SHAPES)
def test_sample_planes_matches_fp64_in_and_out_of_range(h, w, c, m):
    """Every grid set (unclamped uniform, exact +-1, pixel centres, the border walk) on random normal planes; the same points in
    reversed order give the reversed rows bit for bit (a row does not depend on its neighbours)."""
    L, lib = _lib()
    n = 3
    pl = K.planes(n, h, w, c, seed=1000 * h + 10 * w + c)
    pg = pl.cuda()
    for gname, grid in K.plane_grid_sets(n, m, w, h, seed=m + h).items():
        r64, r32 = K.sample_planes_ref(pl, grid, F64), K.sample_planes_ref(pl, grid, F32)
        outs = []
        for g in (grid, grid.flip(1).contiguous()):
            gg = g.cuda()
            buf, out = _guarded((n, m, c))
            L.check(lib.s3d_sample_planes_fwd(pg.data_ptr(), gg.data_ptr(), out.data_ptr(), n, h, w, c, m, None), "s3d_sample_planes_fwd")
            torch.cuda.synchronize()
            assert _guards_intact(buf)
            outs.append(out)
        e, bound = _row("planes-%dx%dx%d-m%d-%s" % (h, w, c, m, gname), outs[0], r64, r32)
        assert e <= bound, (gname, e, bound)
        assert _bits_equal(outs[1].flip(1), outs[0]), gname


# ------------------------------------------------------------------------------------------------------------------ sample_pyramid
_pyr_models = {}


def _pyr_model(size, ns):
    from slice3d_amd.models import Slices3DRegModel
    if (size, ns) not in _pyr_models:
        _pyr_models[(size, ns)] = Slices3DRegModel(img_size=size, n_slices=ns, mode="test").cuda().eval()
    return _pyr_models[(size, ns)]


@pytest.mark.parametrize("q", K.PYR_Q)
@pytest.mark.parametrize("size", [16, 32])
@pytest.mark.parametrize("ns", [1, 3])
def test_sample_pyramid_matches_fp64_across_chunk_edges_and_borders(ns, size, q):
    """B = 2 with different grids per object; Q on both sides of the 128-row chunk edge and of the 4096-query sort threshold; at
    S = 16 level 0 is a single pixel.  Unclamped uniform grids, one point repeated (the tap cache never reloads) and the border
    walk (rows with equal and unequal first-tap offsets follow each other).  Two calls give the same bits."""
    b = 2
    m = _pyr_model(size, ns)
    pyr = K.pyramid(b * ns, size, seed=size + ns)
    pg = [p.cuda() for p in pyr]
    for gname in ("uniform", "pile", "walk"):
        grid = K.pyramid_grid(gname, b, q, size, seed=q + ns)
        r64, r32 = K.sample_pyramid_ref(pyr, grid, ns, F64), K.sample_pyramid_ref(pyr, grid, ns, F32)
        gg = grid.cuda()
        outs = []
        for _ in range(2):
            buf, out = _guarded((b * ns, q, 992))
            m.sample_pyramid(pg, gg, out=out)
            torch.cuda.synchronize()
            assert _guards_intact(buf)
            outs.append(out)
        e, bound = _row("pyramid-ns%d-s%d-q%d-%s" % (ns, size, q, gname), outs[0], r64, r32)
        assert e <= bound, (gname, e, bound)
        assert _bits_equal(outs[0], outs[1]), gname


# ------------------------------------------------------------------------------------------------------------------ query sort
def _query_sort(qry, rot, trans, flip, times=3):
    L, lib = _lib()
    b, q, _ = qry.shape
    qg, rg, tg = qry.cuda(), rot.cuda(), trans.cuda()
    nbytes = lib.s3d_query_sort_workspace_bytes(b, q)
    ws = torch.empty(nbytes // 4 + 1, dtype=torch.int32, device="cuda")
    perms = []
    for _ in range(times):
        buf, perm = _guarded((b, q), torch.int32)
        L.check(lib.s3d_query_sort(qg.data_ptr(), rg.data_ptr(), tg.data_ptr(), flip, b, q, perm.data_ptr(), ws.data_ptr(), nbytes, None),
                "s3d_query_sort")
        torch.cuda.synchronize()
        assert _guards_intact(buf)
        perms.append(perm.cpu().numpy().astype(np.int64))
    for p in perms[1:]:
        assert np.array_equal(p, perms[0])
    return perms[0]


@pytest.mark.parametrize("variant", ["rot", "flip"])
@pytest.mark.parametrize("q", K.SORT_Q)
def test_query_sort_gives_the_exact_permutation_on_exact_keys(q, variant):
    """Inputs whose key is exact in every fp32 evaluation (query_cases.sort_exact_inputs): the permutation is the stable argsort
    of the key, for every object — each with its own signed permutation matrix, or through the flip — with bins of exactly 1,
    2, 32, 33 (the insertion-sort / rank-sort boundary) and several hundred members.  Three calls, identical."""
    qry, rot, trans, keys, _ = K.sort_exact_inputs(q, variant)
    perm = _query_sort(qry, rot, trans, 1 if variant == "flip" else 0)
    want = K.expected_perm(keys)
    for b in range(3):
        assert np.array_equal(perm[b], want[b]), (b, int((perm[b] != want[b]).sum()))


@pytest.mark.parametrize("mode", ["train", "test"])
def test_query_sort_orders_by_fp64_keys_per_camera(mode):
    """CAMERAS, uniform + piled + clamped queries, Q = 30000: a permutation per object, and the queries farther than 1e-3 bin
    widths from a bin edge (all but <= 1 %, asserted on the CPU) are in strictly increasing (float64 key, index) order."""
    cams = K.cams_of(3)
    qry = K.sort_camera_inputs()
    k64, keep, _ = K.sort_camera_keys(qry, cams, mode)
    rot, trans = K.rot_trans(cams)
    perm = _query_sort(qry, rot, trans, 1 if mode == "test" else 0)
    for b in range(3):
        assert np.array_equal(np.sort(perm[b]), np.arange(qry.shape[1])), b
        assert K.strictly_increasing_kept(perm[b], k64[b], keep[b]), b


# ------------------------------------------------------------------------------------------------------------------ token builder
_models = {}


def _shapes(ns):
    import json
    import os
    shapes = {k: tuple(v) for k, v in json.load(open(os.path.join(GOLDEN, "state_dict_keys.json"))).items()}
    shapes["slices_generator.emds.weight"] = (ns, 128)
    return shapes


def _reg_model(ns, mode, prec):
    from slice3d_amd.models import Slices3DRegModel
    from slice3d_amd.weights import load_seeded
    key = (ns, mode, prec)
    if key not in _models:
        m = Slices3DRegModel(n_slices=ns, mode=mode, prec=prec)
        load_seeded(m, 0)
        _models[key] = m.cuda().eval()
    return _models[key]


def _feed(b, s, q, ns, seed, first_cam=0, with_slices=False):
    from slice3d_amd.synth import make_feed_dict
    return K.with_cameras(make_feed_dict(b, s, q, ns, seed=seed, with_slices=with_slices), K.cams_of(b, first_cam))


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("q", [1, 17, 250])
@pytest.mark.parametrize("mode", ["train", "test"])
@pytest.mark.parametrize("ns", [12, 3])
def test_token_builder_matches_fp64_on_its_own_pyramid(ns, mode, q, prec):
    """Sampler + projection + fc_s only: the float64 reference samples the model's OWN encoded pyramid (code.pyramid) and
    applies fc_p / fc_s.  B = 3 with CAMERAS, rotation (train) and flip (test), ragged last groups, query sets on the border,
    on pixel centres, sixteen to a pixel cell (window form) and far apart (per-lane form).  The shared-window and the per-lane
    form both meet the gate and give the same bits."""
    L, lib = _lib()
    b, s = 3, 32
    cams = K.cams_of(b)
    model = _reg_model(ns, mode, prec)
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items() if k.startswith(("fc_p.", "fc_s.", "att_decoder.", "fc_out."))}
    fd = _feed(b, s, 1, ns, seed=77)
    code = model.encode({k: v.cuda() for k, v in fd.items()})
    pyr = [p.cpu() for p in code.pyramid]
    try:
        for name in ("uniform", "border", "centres", "neighbours", "scattered"):
            qry = K.query_set(name, b, q, 500 + q, cams, mode, s)
            p64, s64 = K.token_rows_ref(sd, pyr, qry, cams, mode, ns, F64)
            p32, s32 = K.token_rows_ref(sd, pyr, qry, cams, mode, ns, F32)
            got = []
            for shared in (0, 1):
                assert lib.s3d_decode_set_shared_footprint(shared) == 0
                st = model.decode_stages(qry.cuda(), code)
                torch.cuda.synchronize()
                got.append((st["fc_p"].clone(), st["fc_s"].clone()))
                tag = "tokens-ns%d-%s-q%d-%s-%s-%s" % (ns, mode, q, prec, name, "window" if shared else "lanes")
                ep, bp = _row(tag + "-fc_p", got[-1][0], p64, p32, K.CAP["fc_p"])
                es, bs = _row(tag + "-fc_s", got[-1][1], s64, s32, K.CAP["fc_s"])
                assert ep <= bp and es <= bs, (name, shared, ep, bp, es, bs)
            assert _bits_equal(got[0][0], got[1][0]) and _bits_equal(got[0][1], got[1][1]), name
    finally:
        lib.s3d_decode_set_shared_footprint(1)


# ------------------------------------------------------------------------------------------------------------------ end to end
@pytest.mark.parametrize("b,s,q,ns,mode", [(3, 32, 257, 4, "train"), (3, 32, 4200, 3, "test")])
def test_reg_forward_matches_oracle_with_per_object_cameras(b, s, q, ns, mode):
    """Slices3DRegModel.forward against the live CPU oracle; and the output of object b changes when only its camera is
    swapped for another one, while the other objects keep their bits."""
    from oracle import ref_cpu
    fd = _feed(b, s, q, ns, seed=600 + q)
    sd = seeded_sd_from_shapes(_shapes(ns))
    want = ref_cpu.forward(sd, fd, mode=mode, n_slices=ns, with_vgg=False)["sdf_pred"]
    model = _reg_model(ns, mode, "f16x3")
    got = model({k: v.cuda() for k, v in fd.items()})["sdf_pred"].clone()
    e = float((got.cpu() - want).abs().max())
    print("ROW reg-forward-b%d-s%d-q%d-ns%d-%s e_kernel %.3e bound %.1e" % (b, s, q, ns, mode, e, K.CAP["sdf"]))
    assert e < K.CAP["sdf"]
    for ob in range(b):
        cams = K.cams_of(b)
        cams[ob] = K.CAMERAS[(ob + 1) % 3]
        other = model({k: v.cuda() for k, v in K.with_cameras(fd, cams).items()})["sdf_pred"]
        for o2 in range(b):
            if o2 == ob:
                assert float((other[o2] - got[o2]).abs().max()) > 1e-3, ob
            else:
                assert torch.equal(other[o2], got[o2]), (ob, o2)


@pytest.mark.parametrize("b,s,q,ns,mode", [(3, 32, 70, 12, "train"), (2, 48, 4500, 5, "test")])
def test_gt_forward_matches_oracle_with_per_object_cameras(b, s, q, ns, mode):
    """Slices3DGTModel.forward (sample_tokens_gt_kernel, gt_point_tokens_kernel) against the live CPU oracle."""
    from oracle import ref_cpu
    from slice3d_amd.models_gt import Slices3DGTModel
    from slice3d_amd.weights import load_seeded
    from test_gt_oracle import gt_shapes
    fd = _feed(b, s, q, ns, seed=900 + q, first_cam=1, with_slices=True)
    sd = seeded_sd_from_shapes(gt_shapes())
    with torch.no_grad():
        want, _ = ref_cpu.gt_forward(sd, fd, mode, ns)
    m = load_seeded(Slices3DGTModel(n_slices=ns, mode=mode, prec="f16x3"), 0).cuda().eval()
    got = m({k: v.cuda() for k, v in fd.items()})["sdf_pred"].cpu()
    e = float((got - want).abs().max())
    print("ROW gt-forward-b%d-s%d-q%d-ns%d-%s e_kernel %.3e bound %.1e" % (b, s, q, ns, mode, e, K.CAP["sdf"]))
    assert e < K.CAP["sdf"]
    if b == 3:       # the same batch through the batch's FIRST camera only is something else
        same = m({k: v.cuda() for k, v in K.with_cameras(fd, [K.CAMERAS[1]] * b).items()})["sdf_pred"].cpu()
        assert torch.equal(same[0], got[0]) and float((same[1:] - got[1:]).abs().max()) > 1e-3


TRAIN_SHAPES = [(3, 32, 50, 12), (2, 32, 4200, 3)]       # the second: sorted order and the tiled / dense sampling backward
_train_oracle = {}


def _reg_train_oracle(b, s, q, ns):
    from oracle import ref_cpu
    from test_gpu_train import PRE_BN_BIASES
    key = ("reg", b, s, q, ns)
    if key not in _train_oracle:
        fd = _feed(b, s, q, ns, seed=200 + q, with_slices=True)
        sd = seeded_sd_from_shapes(_shapes(ns))
        for k, v in sd.items():
            if v.is_floating_point() and "running" not in k and not k.startswith("vggptlossfunc"):
                v.requires_grad_(True)
        loss, parts, out, _ = ref_cpu.forward_train(sd, fd, ns, 0.0)
        loss.backward()
        _train_oracle[key] = (fd, [float(p) for p in parts], {k: v.grad for k, v in sd.items() if v.grad is not None}, PRE_BN_BIASES,
                              out["sdf_pred"].detach())
    return _train_oracle[key]


def _gt_train_oracle(b, s, q, ns):
    from oracle import ref_cpu
    from test_gt_oracle import GT_PRE_BN_BIASES, gt_train_sd
    key = ("gt", b, s, q, ns)
    if key not in _train_oracle:
        fd = _feed(b, s, q, ns, seed=400 + q, first_cam=2, with_slices=True)
        sd = gt_train_sd()
        loss, acc, sdf, _ = ref_cpu.gt_forward_train(sd, fd, ns, 0.0)
        loss.backward()
        _train_oracle[key] = (fd, [float(loss.detach())], {k: v.grad for k, v in sd.items() if v.grad is not None}, GT_PRE_BN_BIASES,
                              sdf.detach())
    return _train_oracle[key]


def _check_grads(tag, m, tr, grads, skip):
    worst, worst_k, n = 0.0, None, 0
    for k, p in m.named_parameters():
        if k not in tr.offsets:
            continue
        if k in skip:
            assert float(p.grad.abs().max()) < 1e-4, k
            continue
        ref = grads.get(k)
        if ref is None:
            continue
        rel = float((p.grad.cpu() - ref).norm() / ref.norm())
        n += 1
        if rel > worst:
            worst, worst_k = rel, k
    print("ROW %s worst rel L2 gradient error %.3e (%s) over %d tensors bound %.1e" % (tag, worst, worst_k, n, K.GRAD_REL_L2))
    assert n > 20 and worst < K.GRAD_REL_L2, (worst_k, worst)


@pytest.mark.parametrize("sbd_off", [0, 1])
@pytest.mark.parametrize("b,s,q,ns", TRAIN_SHAPES)
def test_reg_train_step_matches_oracle_autograd_with_per_object_cameras(b, s, q, ns, sbd_off, monkeypatch):
    """HipTrainer.forward_backward, dropout 0, with the default sampling backward and with S3D_SBD_OFF=1 (the atomic kernels;
    test_atomic_free_sampling_backward_matches_the_atomic_kernels' switch): losses 2e-5 relative, every gradient tensor 2e-2
    relative L2 against autograd through ref_cpu.forward_train."""
    from slice3d_amd.models import Slices3DRegModel
    from slice3d_amd.trainer import HipTrainer
    from slice3d_amd.weights import load_seeded
    fd, parts, grads, skip, _ = _reg_train_oracle(b, s, q, ns)
    monkeypatch.delenv("S3D_SBD_SLOW_MOD", raising=False)
    if sbd_off:
        monkeypatch.setenv("S3D_SBD_OFF", "1")
    else:
        monkeypatch.delenv("S3D_SBD_OFF", raising=False)
    m = load_seeded(Slices3DRegModel(n_slices=ns, mode="train"), 0).cuda()
    tr = HipTrainer(m, dropout=0.0)
    got = tr.forward_backward({k: v.cuda() for k, v in fd.items()}).cpu().numpy()
    tag = "reg-train-b%d-q%d-ns%d-%s" % (b, q, ns, "atomic" if sbd_off else "default")
    for i in range(3):
        print("ROW %s loss%d rel %.3e bound %.1e" % (tag, i, abs(got[i] - parts[i]) / abs(parts[i]), K.LOSS_REL))
        assert abs(got[i] - parts[i]) < K.LOSS_REL * abs(parts[i]) + 1e-7
    _check_grads(tag, m, tr, grads, skip)


@pytest.mark.parametrize("sbd_off", [0, 1])
@pytest.mark.parametrize("b,s,q,ns", TRAIN_SHAPES)
def test_gt_train_step_matches_oracle_autograd_with_per_object_cameras(b, s, q, ns, sbd_off, monkeypatch):
    """HipGtTrainer.forward_backward under the same two settings against autograd through ref_cpu.gt_forward_train."""
    from slice3d_amd.models_gt import Slices3DGTModel
    from slice3d_amd.trainer import HipGtTrainer
    from slice3d_amd.weights import load_seeded
    fd, parts, grads, skip, sdf = _gt_train_oracle(b, s, q, ns)
    monkeypatch.delenv("S3D_SBD_SLOW_MOD", raising=False)
    if sbd_off:
        monkeypatch.setenv("S3D_SBD_OFF", "1")
    else:
        monkeypatch.delenv("S3D_SBD_OFF", raising=False)
    m = load_seeded(Slices3DGTModel(n_slices=ns, mode="train"), 0).cuda()
    tr = HipGtTrainer(m, dropout=0.0)
    losses, sdf_pred = tr.forward_backward({k: v.cuda() for k, v in fd.items()}, want_outputs=True)
    got = losses.cpu().numpy()
    tag = "gt-train-b%d-q%d-ns%d-%s" % (b, q, ns, "atomic" if sbd_off else "default")
    e = float((sdf_pred.cpu() - sdf).abs().max())
    print("ROW %s sdf %.3e bound %.1e loss rel %.3e bound %.1e" % (tag, e, K.CAP["sdf"], abs(got[0] - parts[0]) / abs(parts[0]), K.LOSS_REL))
    assert e < K.CAP["sdf"]
    assert abs(got[0] - parts[0]) < K.LOSS_REL * abs(parts[0]) + 1e-7
    _check_grads(tag, m, tr, grads, skip)


# ------------------------------------------------------------------------------------------------------------------ MISE points, layout
@pytest.mark.parametrize("box", K.MISE_BOXES)
@pytest.mark.parametrize("r0,depth", K.MISE_CASES)
def test_device_mise_points_equal_numpy_float32(r0, depth, box):
    """DeviceMISE.points == box * (p / resolution - 0.5) in numpy float32, bit for bit, for all points of the first round and of
    the round after an update (a sphere, so that cells are refined); resolutions that are no power of two included."""
    from slice3d_amd.mesh import DeviceMISE
    m = DeviceMISE(r0, depth, 0.0)
    res = m.resolution
    assert res == r0 << depth
    idx = m.query()
    assert idx.numel() == (r0 + 1) ** 3
    for rnd in range(2):
        coords = m.coords(idx).cpu().numpy()
        got = m.points(idx, box).cpu().numpy()
        want = K.mise_points_ref(coords, res, box)
        assert got.dtype == want.dtype == np.float32 and got.shape == want.shape
        assert np.array_equal(got.view(np.int32), want.view(np.int32)), (rnd, int((got != want).sum()))
        if rnd == 0:
            val = 0.3 - np.linalg.norm(coords / res - 0.5, axis=-1)
            m.update(idx, torch.from_numpy(val).cuda())
            idx = m.query()
            assert (idx.numel() > 0) == (depth > 0)
            if idx.numel() == 0:
                break


@pytest.mark.parametrize("n,c,h,w", K.NCHW_SHAPES)
def test_layout_helpers_equal_permute(n, c, h, w):
    L, lib = _lib()
    x = torch.randn(n, c, h, w, generator=torch.Generator().manual_seed(n * c + h * w))
    xg = x.cuda()
    buf, nhwc = _guarded((n, h, w, c))
    L.check(lib.s3d_nchw_to_nhwc(xg.data_ptr(), nhwc.data_ptr(), n, c, h, w, None), "s3d_nchw_to_nhwc")
    torch.cuda.synchronize()
    assert _guards_intact(buf) and _bits_equal(nhwc.cpu(), x.permute(0, 2, 3, 1).contiguous())
    buf2, back = _guarded((n, c, h, w))
    L.check(lib.s3d_nhwc_to_nchw(nhwc.data_ptr(), back.data_ptr(), n, c, h, w, None), "s3d_nhwc_to_nchw")
    torch.cuda.synchronize()
    assert _guards_intact(buf2) and _bits_equal(back.cpu(), x)
    y = torch.randn(n, h, w, c, generator=torch.Generator().manual_seed(7)).cuda()      # nhwc -> nchw from independent data
    buf3, o3 = _guarded((n, c, h, w))
    L.check(lib.s3d_nhwc_to_nchw(y.data_ptr(), o3.data_ptr(), n, c, h, w, None), "s3d_nhwc_to_nchw")
    torch.cuda.synchronize()
    assert _guards_intact(buf3) and _bits_equal(o3, y.permute(0, 3, 1, 2).contiguous())

"""Kernel-by-kernel conformance of the convolution engine (launch_conv, conv.hip) through its public entry points:
s3d_conv_pack, s3d_conv_fwd, s3d_conv_gn_fwd (with s3d_group_norm_table_fwd), s3d_conv_finish_fwd and s3d_conv_strided_fwd.

Every row of the case tables is shaped to land on one kernel instantiation (named in its id) and to hit at least one edge:
maps that are no multiple of the 8 x 16 tile, several images with their own content, cout < CoutPad, input channel counts
that force the fp32 kernel, two sources of unequal width, with / without residual and bias, pixel-tile counts that are no
multiple of 8 next to several cout tiles (the XCD-remap tail of conv_block_tile).  The whole output is compared with a
float64 CPU reference (F.conv2d / matmul; F.group_norm -> FiLM -> SiLU for the fused rows):
  * PREC_F32 and PREC_F16X3 within 2e-5 * max(1, max|ref|);
  * PREC_F16 within 5e-3 of the same scale and measurably worse than f16x3 (the single-pass kernel really ran); without an
    f16 weight image (channel counts that are no multiple of 32) all three modes give the same bits;
  * split-K rows: no workspace, a workspace for two splits and a large one all meet the gate and agree to rounding; a
    deferred finish (nsplit_out + s3d_conv_finish_fwd) gives the bits of the direct call;
  * `out` sits inside a NaN-guarded buffer and is NaN-prefilled: both guards intact, every output written; a second call
    gives the same bits; finite garbage in the caller's pad channels (cin .. pad16(cin)) changes no bit.
"""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

GUARD = 256                 # floats of guard on each side of `out` (keeps its 16-byte alignment)
NAN_BITS = 0x7FC5A5A5       # a quiet NaN with a payload no kernel computes
TOL32, TOL16 = 2e-5, 5e-3


def _pad16(c):
    return (c + 15) // 16 * 16


def _lib():
    from slice3d_amd import _lib as L
    return L, L.load()


def _guarded(shape):
    """(buffer, out): `out` of `shape` inside a buffer with GUARD floats before and after it, all of it NAN_BITS."""
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((GUARD + n + GUARD,), NAN_BITS, dtype=torch.int32, device="cuda").view(torch.float32)
    return buf, buf[GUARD:GUARD + n].view(shape)


def _guards_intact(buf):
    b = buf.view(torch.int32)
    return bool((b[:GUARD] == NAN_BITS).all()) and bool((b[-GUARD:] == NAN_BITS).all())


def _nhwc_padded(x, fill=0.0):
    """(N, C, H, W) -> (N, H, W, pad16(C)) on the GPU, the pad channels set to `fill`."""
    n, c, h, w = x.shape
    y = torch.full((n, h, w, _pad16(c)), fill, dtype=torch.float32)
    y[..., :c] = x.permute(0, 2, 3, 1)
    return y.cuda()


def _pack(lib, L, wt, b, cout, cin0, cin1, ks):
    nb = lib.s3d_conv_packed_bytes(cout, cin0, cin1, ks)
    buf = torch.empty(nb, dtype=torch.uint8, device="cuda")
    wg = wt.float().contiguous().cuda()
    bg = b.float().cuda() if b is not None else None
    L.check(lib.s3d_conv_pack(wg.data_ptr(), bg.data_ptr() if bg is not None else None, cout, cin0, cin1, ks, buf.data_ptr(), nb,
                              None), "s3d_conv_pack")
    torch.cuda.synchronize()
    return buf


def _err(out, ref):
    """max |out - ref| over the whole output (NaN if any output is NaN) and the gate's scale max(1, max|ref|)."""
    d = (out.cpu().double() - ref).abs()
    e = float("nan") if torch.isnan(d).any() else float(d.max())
    return e, max(1.0, float(ref.abs().max()))


def _ref_conv(x, wt, b, ks, stride=1, pad=None):
    """float64 convolution of (N, C, H, W); 1x1 stride-1 convolutions as a matmul."""
    xd, wd = x.double(), wt.double()
    if ks == 1 and stride == 1:
        n, c, h, w = x.shape
        y = (xd.permute(0, 2, 3, 1).reshape(-1, c) @ wd[:, :, 0, 0].t()).reshape(n, h, w, -1).permute(0, 3, 1, 2)
    else:
        y = F.conv2d(xd, wd, None, stride=stride, padding=ks // 2 if pad is None else pad)
    if b is not None:
        y = y + b.double().view(1, -1, 1, 1)
    return y


def _inputs(seed, n, cin, cout, h, w, ks, bias, residual):
    g = torch.Generator().manual_seed(seed)
    wt = torch.randn(cout, cin, ks, ks, generator=g) * (1.0 / (cin * ks * ks)) ** 0.5
    b = torch.randn(cout, generator=g) * 0.5 if bias else None
    x = torch.randn(n, cin, h, w, generator=g)
    res = torch.randn(n, cout, h, w, generator=g) if residual else None
    return g, wt, b, x, res


def _check_precisions(outs, ref, has_f16, what):
    """outs: {prec: output (N, H, W, cout) on the GPU}; ref (N, cout, H, W) float64."""
    from slice3d_amd import _lib as L
    refh = ref.permute(0, 2, 3, 1)
    errs = {}
    for prec, out in outs.items():
        e, scale = _err(out, refh)
        errs[prec] = e
        tol = TOL16 if prec == L.PREC_F16 and has_f16 else TOL32
        assert e < tol * scale, (what, prec, e, scale)
    if L.PREC_F16 in outs:
        if has_f16:   # one f16 MFMA per product: visibly coarser than the split-precision products
            assert errs[L.PREC_F16] > 10 * errs[L.PREC_F16X3] and errs[L.PREC_F16] > 1e-4, (what, errs)
        else:         # no f16 weight image: the exact fp32 kernel in every mode
            for prec in (L.PREC_F16X3, L.PREC_F16):
                assert torch.equal(outs[prec].view(torch.int32), outs[L.PREC_F32].view(torch.int32)), (what, prec)
    return errs


# ---------------------------------------------------------------------------------------------------------------- s3d_conv_fwd
# (id, N, H, W, cin0, cin1, cout, ks, residual, bias, split): split = the row takes split-K with a workspace (run three ways)
FWD_CASES = [
    # LDS-staged 3x3 kernel (f16x3 / f16); its F32 run is the fp32 tile menu of the same shape
    ("lds_4_2_2_2-co64-xcdtail", 3, 13, 17, 64, 32, 124, 3, True, True, False),
    ("lds_2_4_1_1-co32-onebuf", 3, 9, 40, 64, 0, 84, 3, False, False, False),
    ("lds_2_4_1_2-co32-twobuf", 2, 17, 33, 96, 32, 32, 3, True, False, False),
    ("lds_4_2_2_2-splitk", 1, 9, 20, 256, 0, 64, 3, True, True, True),
    ("lds_2_4_1_x-splitk", 2, 8, 16, 128, 64, 96, 3, False, True, True),
    # small-map 3x3 kernel (split-K only; without a workspace: the f16x3 tile menu)
    ("small3x3_pt1", 1, 3, 5, 64, 32, 124, 3, True, True, True),
    ("small3x3_pt2", 2, 4, 4, 128, 0, 64, 3, False, False, True),
    ("small3x3_pt4", 4, 3, 5, 64, 0, 188, 3, True, True, True),
    # small-map 1x1 kernel
    ("small1x1_pt1", 1, 3, 5, 96, 0, 64, 1, False, True, True),
    ("small1x1_pt2", 2, 3, 4, 64, 64, 124, 1, True, True, True),
    ("small1x1_pt4", 3, 5, 4, 128, 0, 192, 1, True, False, True),
    # row-linear kernels
    ("lin_stream_1-ragged", 3, 7, 6667, 128, 0, 96, 1, True, True, False),
    ("lin_rows-ragged", 2, 5, 6601, 96, 0, 84, 1, False, True, False),
    # tile menu, 1x1 (two sources keep it off the row-linear kernels)
    ("menu_4_4_2_2-ks1", 2, 33, 1000, 64, 32, 128, 1, True, True, False),
    ("menu_2_4_2_2-ks1", 3, 25, 500, 64, 32, 128, 1, False, True, False),
    ("menu_1_4_2_2-ks1", 3, 20, 150, 64, 32, 128, 1, True, False, False),
    ("menu_1_1_2_2-ks1", 3, 9, 50, 32, 64, 124, 1, True, True, False),
    ("menu_4_4_4_1-ks1", 1, 170, 257, 32, 32, 188, 1, True, True, False),
    ("menu_2_2_2_2-ks1", 3, 45, 130, 32, 32, 64, 1, False, True, False),
    ("menu_4_2_4_1-ks1", 1, 171, 256, 32, 64, 84, 1, True, True, False),
    ("menu_4_1_4_1-ks1", 1, 171, 257, 32, 32, 36, 1, True, True, False),
    ("menu_1_1_4_1-ks1", 3, 9, 50, 32, 32, 4, 1, True, True, False),
    # tile menu, 3x3 (maps below 8 rows without a workspace, or CoutPad % 32 != 0, keep it off the LDS kernel)
    ("menu_4_4_2_2-ks3", 4, 7, 2400, 32, 0, 128, 3, True, True, False),
    ("menu_2_4_2_2-ks3", 3, 5, 2500, 32, 0, 128, 3, False, True, False),
    ("menu_1_4_2_2-ks3", 2, 6, 750, 32, 0, 124, 3, True, False, False),
    ("menu_1_1_2_2-ks3", 3, 7, 13, 32, 32, 128, 3, True, True, False),
    ("menu_4_4_4_1-ks3", 1, 6, 7300, 32, 0, 188, 3, True, True, False),
    ("menu_2_2_2_2-ks3", 2, 7, 1200, 32, 32, 64, 3, False, True, False),
    ("menu_4_2_4_1-ks3", 1, 7, 6300, 32, 0, 84, 3, True, True, False),
    ("menu_4_1_4_1-ks3", 1, 171, 256, 32, 0, 48, 3, True, True, False),
    ("menu_1_1_4_1-ks3", 3, 13, 17, 32, 32, 4, 3, True, True, False),
    # no f16 image (cin % 32 != 0): the fp32 kernel in every mode; pad channels
    ("fp32-cin3-ks3", 3, 13, 17, 3, 0, 36, 3, True, True, False),
    ("fp32-cin8-ks1", 2, 9, 50, 8, 0, 100, 1, False, True, False),
    ("fp32-cin48_16-ks3", 3, 9, 50, 48, 16, 128, 3, True, False, False),
    ("fp32-cin40_24-ks3-ws", 1, 8, 16, 40, 24, 64, 3, True, True, True),
]


def _run_fwd(lib, L, buf, x0, x1, res, shape, cout, cin0, cin1, ks, prec, ws):
    """One s3d_conv_fwd into a guarded, NaN-prefilled output; -> out (guards checked)."""
    n, h, w = shape
    gbuf, out = _guarded((n, h, w, cout))
    wsp, wsb = (ws.data_ptr(), ws.numel() * 4) if ws is not None else (None, 0)
    L.check(lib.s3d_conv_fwd(buf.data_ptr(), x0.data_ptr(), x1.data_ptr() if x1 is not None else None,
                             res.data_ptr() if res is not None else None, out.data_ptr(), n, h, w, cout, cin0, cin1, ks, prec,
                             wsp, wsb, None), "s3d_conv_fwd")
    torch.cuda.synchronize()
    assert _guards_intact(gbuf), "a write outside `out`"
    assert bool(torch.isfinite(out).all()), "an output left unwritten (NaN prefill) or not finite"
    return out


@pytest.mark.parametrize("case", FWD_CASES, ids=[c[0] for c in FWD_CASES])
def test_conv_fwd_matches_fp64(case):
    L, lib = _lib()
    name, n, h, w, cin0, cin1, cout, ks, residual, bias, split = case
    cin = cin0 + cin1
    _, wt, b, x, res = _inputs(sum(map(ord, name)), n, cin, cout, h, w, ks, bias, residual)
    ref = _ref_conv(x, wt, b, ks)
    if res is not None:
        ref = ref + res.double()
    buf = _pack(lib, L, wt, b, cout, cin0, cin1, ks)
    x0, x1 = _nhwc_padded(x[:, :cin0]), (_nhwc_padded(x[:, cin0:]) if cin1 else None)
    rc = res.permute(0, 2, 3, 1).contiguous().cuda() if res is not None else None
    has_f16 = cin0 % 32 == 0 and cin1 % 32 == 0
    out_floats = n * h * w * _pad16(cout)
    ws_runs = {"none": None}
    if split:   # a workspace for exactly two splits, and one for many
        ws_runs["two"] = torch.empty(2 * out_floats, dtype=torch.float32, device="cuda")
        ws_runs["big"] = torch.empty(64 * out_floats, dtype=torch.float32, device="cuda")
    pad_cases = cin0 % 16 or cin1 % 16
    for wsname, ws in ws_runs.items():
        outs = {}
        for prec in (L.PREC_F32, L.PREC_F16X3, L.PREC_F16):
            out = _run_fwd(lib, L, buf, x0, x1, rc, (n, h, w), cout, cin0, cin1, ks, prec, ws)
            again = _run_fwd(lib, L, buf, x0, x1, rc, (n, h, w), cout, cin0, cin1, ks, prec, ws)
            assert torch.equal(out.view(torch.int32), again.view(torch.int32)), (name, wsname, prec, "second call")
            if pad_cases:   # finite garbage in the pad channels meets zero weights: no bit changes
                g0 = _nhwc_padded(x[:, :cin0], 1e3)
                g1 = _nhwc_padded(x[:, cin0:], -1e3) if cin1 else None
                garbage = _run_fwd(lib, L, buf, g0, g1, rc, (n, h, w), cout, cin0, cin1, ks, prec, ws)
                assert torch.equal(out.view(torch.int32), garbage.view(torch.int32)), (name, wsname, prec, "pad channels")
            outs[prec] = out
        errs = _check_precisions(outs, ref, has_f16, (name, wsname))
        if wsname == "none":
            base = outs
        else:       # split-K: the same sums in another grouping
            for prec, out in outs.items():
                tol = TOL16 if prec == L.PREC_F16 and has_f16 else TOL32
                assert float((out - base[prec]).abs().max()) < tol * max(1.0, float(ref.abs().max())), (name, wsname, prec, errs)


# -------------------------------------------------------------------------------------------------------------- s3d_conv_gn_fwd
# (id, N, H, W, cin0, cin1, cout, film, silu, residual, bias)
GN_CASES = [
    ("lds_4_2_2_2_gn-co64", 3, 11, 19, 64, 32, 64, True, 1, True, True),
    ("lds_2_4_1_2_gn-co96", 2, 16, 40, 128, 0, 96, False, 0, False, True),
    ("small3x3_pt1_gn", 1, 4, 4, 64, 0, 64, True, 1, False, True),
    ("small3x3_pt2_gn", 2, 3, 5, 96, 32, 128, False, 1, True, False),
    ("small3x3_pt4_gn", 3, 4, 4, 64, 0, 64, True, 1, True, True),
]
GN_GROUPS, GN_EPS = 32, 1e-5


@pytest.mark.parametrize("case", GN_CASES, ids=[c[0] for c in GN_CASES])
def test_conv_gn_fwd_matches_fp64(case):
    """GroupNorm32 -> [FiLM] -> [SiLU] -> conv3x3 as one operator against the same chain in float64; split-K three ways;
    the deferred finish (nsplit_out + s3d_conv_finish_fwd) against the direct call, bit for bit."""
    L, lib = _lib()
    name, n, h, w, cin0, cin1, cout, film, silu, residual, bias = case
    cin = cin0 + cin1
    g, wt, b, x, res = _inputs(sum(map(ord, name)), n, cin, cout, h, w, 3, bias, residual)
    x = x * 1.5 + 0.3   # statistics away from (0, 1)
    gamma = 1.0 + 0.2 * torch.randn(cin, generator=g)
    beta = 0.2 * torch.randn(cin, generator=g)
    fstride = 2 * cin + 8
    fl = 0.3 * torch.randn(n, fstride, generator=g) if film else None
    y = F.group_norm(x.double(), GN_GROUPS, gamma.double(), beta.double(), GN_EPS)
    if film:
        y = y * (1 + fl[:, :cin].double().view(n, cin, 1, 1)) + fl[:, cin:2 * cin].double().view(n, cin, 1, 1)
    if silu:
        y = F.silu(y)
    ref = _ref_conv(y, wt, b, 3)
    if res is not None:
        ref = ref + res.double()
    buf = _pack(lib, L, wt, b, cout, cin0, cin1, 3)
    x0, x1 = _nhwc_padded(x[:, :cin0]), (_nhwc_padded(x[:, cin0:]) if cin1 else None)
    rc = res.permute(0, 2, 3, 1).contiguous().cuda() if res is not None else None
    gg, bg = gamma.cuda(), beta.cuda()
    fg = fl.cuda() if film else None
    table = torch.empty((n, 2, cin), device="cuda")
    stats = torch.empty(lib.s3d_group_norm_stats_floats(n, GN_GROUPS), device="cuda")
    L.check(lib.s3d_group_norm_table_fwd(x0.data_ptr(), cin0, x1.data_ptr() if x1 is not None else None, cin1, gg.data_ptr(),
                                         bg.data_ptr(), fg.data_ptr() if film else None, fstride if film else 0, table.data_ptr(),
                                         stats.data_ptr(), n, h * w, GN_GROUPS, C.c_float(GN_EPS), None, None),
            "s3d_group_norm_table_fwd")
    out_floats = n * h * w * cout
    ws_runs = {"none": None, "two": torch.empty(2 * out_floats, device="cuda"), "big": torch.empty(64 * out_floats, device="cuda")}
    small = w < 16 or h < 8

    def call(prec, ws, out, nsplit=None):
        wsp, wsb = (ws.data_ptr(), ws.numel() * 4) if ws is not None else (None, 0)
        return lib.s3d_conv_gn_fwd(buf.data_ptr(), x0.data_ptr(), x1.data_ptr() if x1 is not None else None,
                                   rc.data_ptr() if rc is not None else None, out.data_ptr(), n, h, w, cout, cin0, cin1, 3, prec,
                                   table.data_ptr(), silu, wsp, wsb, C.byref(nsplit) if nsplit is not None else None, None)

    outs_by_ws = {}
    for wsname, ws in ws_runs.items():
        if ws is None and small:   # maps below the 8 x 16 tile are served with a split-K workspace only
            _, out = _guarded((n, h, w, cout))
            assert call(L.PREC_F16X3, None, out) != 0
            continue
        outs = {}
        for prec in (L.PREC_F16X3, L.PREC_F16):
            gbuf, out = _guarded((n, h, w, cout))
            L.check(call(prec, ws, out), "s3d_conv_gn_fwd")
            torch.cuda.synchronize()
            assert _guards_intact(gbuf) and bool(torch.isfinite(out).all()), (name, wsname, prec)
            _, again = _guarded((n, h, w, cout))
            L.check(call(prec, ws, again), "s3d_conv_gn_fwd")
            torch.cuda.synchronize()
            assert torch.equal(out.view(torch.int32), again.view(torch.int32)), (name, wsname, prec, "second call")
            if ws is not None:   # deferred finish: the partials stay in the workspace until s3d_conv_finish_fwd
                ns = C.c_int(0)
                dbuf, dout = _guarded((n, h, w, cout))
                L.check(call(prec, ws, dout, ns), "s3d_conv_gn_fwd (deferred)")
                if wsname == "two":
                    assert ns.value == 2, (name, ns.value)
                if ns.value > 1:
                    torch.cuda.synchronize()
                    assert bool(torch.isnan(dout).all()), "a deferred call wrote `out`"
                    desc = L.S3dConvPartial(ws.data_ptr(), ns.value, buf.data_ptr(), cout, cin0, cin1, 3,
                                            rc.data_ptr() if rc is not None else None, dout.data_ptr())
                    L.check(lib.s3d_conv_finish_fwd(C.byref(desc), n, h, w, None), "s3d_conv_finish_fwd")
                torch.cuda.synchronize()
                assert _guards_intact(dbuf), (name, wsname, prec, "deferred")
                assert torch.equal(dout.view(torch.int32), out.view(torch.int32)), (name, wsname, prec, "deferred finish")
            outs[prec] = out
        _check_precisions(outs, ref, True, (name, wsname))
        outs_by_ws[wsname] = outs
    names = list(outs_by_ws)
    for wsname in names[1:]:
        for prec, out in outs_by_ws[wsname].items():
            tol = TOL16 if prec == L.PREC_F16 else TOL32
            d = float((out - outs_by_ws[names[0]][prec]).abs().max())
            assert d < tol * max(1.0, float(ref.abs().max())), (name, wsname, prec, d)


# -------------------------------------------------------------------------------------------------------- s3d_conv_strided_fwd
# (id, N, Hin, Win, cin, cout, ks, stride, pad_origin)
STRIDED_CASES = [
    ("strided_f16x3_1_1_4_1-ks3-s2-origin", 2, 15, 9, 64, 48, 3, 2, 1),
    ("strided_fp32-cin3-ks3-s2", 3, 17, 13, 3, 36, 3, 2, 0),
    ("strided_f16x3_1_1_2_2-ks3-s2", 2, 33, 21, 32, 124, 3, 2, 0),
    ("strided_f16x3-ks1-s2", 2, 19, 23, 128, 100, 1, 2, 0),
    ("strided_fp32-cin24-ks1-s4", 3, 21, 18, 24, 64, 1, 4, 0),
]


@pytest.mark.parametrize("case", STRIDED_CASES, ids=[c[0] for c in STRIDED_CASES])
def test_conv_strided_fwd_matches_fp64(case):
    L, lib = _lib()
    name, n, hin, win, cin, cout, ks, stride, origin = case
    _, wt, b, x, _ = _inputs(sum(map(ord, name)), n, cin, cout, hin, win, ks, True, False)
    if origin:   # Downsample: F.pad(x, (0, 1, 0, 1)) + Conv2d(3, stride 2)
        ref = _ref_conv(F.pad(x.double(), (0, 1, 0, 1)), wt, b, ks, stride, 0)
    else:
        ref = _ref_conv(x, wt, b, ks, stride)
    ho, wo = ref.shape[2], ref.shape[3]
    buf = _pack(lib, L, wt, b, cout, cin, 0, ks)
    outs = {}
    for prec in (L.PREC_F32, L.PREC_F16X3):
        got = []
        for fill in (0.0, 1e3):
            xg = _nhwc_padded(x, fill)
            gbuf, out = _guarded((n, ho, wo, cout))
            L.check(lib.s3d_conv_strided_fwd(buf.data_ptr(), xg.data_ptr(), out.data_ptr(), n, hin, win, ho, wo, cout, cin, ks,
                                             stride, origin, prec, None), "s3d_conv_strided_fwd")
            torch.cuda.synchronize()
            assert _guards_intact(gbuf) and bool(torch.isfinite(out).all()), (name, prec, fill)
            got.append(out)
        assert torch.equal(got[0].view(torch.int32), got[1].view(torch.int32)), (name, prec, "pad channels / second call")
        outs[prec] = got[0]
    _check_precisions(outs, ref, cin % 32 == 0, name)
    if cin % 32:
        assert torch.equal(outs[L.PREC_F32].view(torch.int32), outs[L.PREC_F16X3].view(torch.int32)), name

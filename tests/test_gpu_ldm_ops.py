"""Kernel-by-kernel conformance of the latent-diffusion U-Net's device code outside the convolution engine, through the C
ABI only: GroupNorm (s3d_group_norm_fwd / _film_fwd / group_norm2_fwd / _table_fwd / _partial_fwd), attention
(s3d_qkv_attention_fwd, s3d_qkv_attention_ws_fwd), s3d_small_linear_fwd, s3d_timestep_embedding_fwd, s3d_resample2x_fwd,
s3d_add_fwd, s3d_add_nchw_fwd and s3d_nchw_to_nhwc_pad.

The rows, their generators, the float64 references and the gates are in tests/ldm_ops_cases.py (checked on the CPU by
tests/test_ldm_ops_cases.py): every row is shaped to land on the kernel instantiation named in its id.  Here every output
sits inside a NaN-prefilled buffer between guards (every element written, both guards intact), a second call gives the same
bits, the GroupNorm statistics scratch has exactly s3d_group_norm_stats_floats floats and the attention workspace exactly
s3d_qkv_attention_ws_bytes bytes, both between guards and NaN-prefilled; the second attention call finds other bytes in
the workspace.  Each row prints `ROW id e_kernel e_ref ratio bound` before it asserts (profiles/ldm_ops_conformance_kernels.md).
"""
import ctypes as C

import pytest
import torch

import ldm_ops_cases as K

pytestmark = pytest.mark.gpu

GUARD = 256                 # floats of guard on each side of a buffer (keeps 16-byte alignment; 1024 bytes for the workspace)
NAN_BITS = 0x7FC5A5A5       # a quiet NaN with a payload no kernel computes


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


def _guarded_bytes(nb, fill=None):
    """(buffer, ws): `nb` bytes inside a byte buffer with 4 * GUARD bytes of NAN_BITS on each side; the inside is NAN_BITS too,
    or the byte `fill`."""
    words = 2 * GUARD + (nb + 3) // 4
    buf = torch.full((words,), NAN_BITS, dtype=torch.int32, device="cuda").view(torch.uint8)
    ws = buf[4 * GUARD:4 * GUARD + nb]
    if fill is not None:
        ws.fill_(fill)
    return buf, ws


def _byte_guards_intact(buf, nb):
    pristine = torch.full((buf.numel() // 4,), NAN_BITS, dtype=torch.int32, device="cuda").view(torch.uint8)
    lo, hi = 4 * GUARD, 4 * GUARD + nb
    return bool(torch.equal(buf[:lo], pristine[:lo])) and bool(torch.equal(buf[hi:], pristine[hi:]))


def _bits_equal(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _report_and_assert(name, out, d, ill, tol=K.TOL32):
    bound, e_ref, scale = K.gate(d["ref64"], d["ref32"], ill, tol)
    e, _ = K.err_and_scale(out.cpu(), d["ref64"])
    print("ROW %s e_kernel %.3e e_ref %.3e ratio %.2f bound %.3e scale %.3g" % (name, e, e_ref, e / e_ref if e_ref > 0 else
                                                                             float("inf") if e > 0 else 0.0, bound, scale))
    assert e <= bound, (name, e, bound, e_ref)
    return e


# ------------------------------------------------------------------------------------------------------------------ GroupNorm
def _film_args(d):
    """device film tensor (kept alive by the caller), pointer to this layer's columns, stride"""
    if d["film"] is None:
        return None, None, 0
    fg = d["film"].cuda()
    return fg, fg.data_ptr() + 4 * d["film_off"], d["film_stride"]


def _table_applied(x64, table):
    """y = x * A + B in float64 from the fp32 table (N, 2, C)."""
    t = table.cpu().double()
    return x64 * t[:, 0:1, :] + t[:, 1:2, :]


@pytest.mark.parametrize("case", K.GN_CASES, ids=[c.id for c in K.GN_CASES])
def test_group_norm_matches_fp64(case):
    L, lib = _lib()
    d = K.gn_build(case)
    n, hw, c, groups = case.n, case.hw, case.c, case.groups
    c0 = case.c0 if case.c0 else c
    x = d["x"]
    x0 = x[..., :c0].contiguous().cuda()
    x1 = x[..., c0:].contiguous().cuda() if case.c0 else None
    gg, bg = d["gamma"].cuda(), d["beta"].cuda()
    fg, fptr, fstride = _film_args(d)
    nstats = lib.s3d_group_norm_stats_floats(n, groups)
    assert nstats == K.gn_stats_floats(n, groups)
    eps = C.c_float(K.GN_EPS)
    outs = []
    for _ in range(2):
        sbuf, stats = _guarded((nstats,))
        obuf, out = _guarded((n, 2, c) if case.out == "table" else (n, hw, c))
        if case.out == "table":
            rc = lib.s3d_group_norm_table_fwd(x0.data_ptr(), c0, _ptr(x1), c - c0, gg.data_ptr(), bg.data_ptr(), fptr, fstride,
                                              out.data_ptr(), stats.data_ptr(), n, hw, groups, eps, None, None)
        elif x1 is not None:
            assert fstride in (0, 2 * c)
            rc = lib.s3d_group_norm2_fwd(x0.data_ptr(), c0, x1.data_ptr(), c - c0, gg.data_ptr(), bg.data_ptr(), fptr,
                                         out.data_ptr(), stats.data_ptr(), n, hw, groups, eps, case.silu, None)
        elif case.film == "wide":
            rc = lib.s3d_group_norm_film_fwd(x0.data_ptr(), gg.data_ptr(), bg.data_ptr(), fptr, fstride, out.data_ptr(),
                                             stats.data_ptr(), n, hw, c, groups, eps, case.silu, None)
        else:
            rc = lib.s3d_group_norm_fwd(x0.data_ptr(), gg.data_ptr(), bg.data_ptr(), fptr, out.data_ptr(), stats.data_ptr(), n,
                                        hw, c, groups, eps, case.silu, None)
        L.check(rc, case.id)
        torch.cuda.synchronize()
        assert _guards_intact(obuf), "a write outside the output"
        assert _guards_intact(sbuf), "a write outside the statistics scratch"
        assert bool(torch.isfinite(out).all()), "an output element left unwritten (NaN prefill) or not finite"
        outs.append(out)
    assert _bits_equal(outs[0], outs[1]), (case.id, "second call")
    got = _table_applied(x.double(), outs[0]) if case.out == "table" else outs[0]
    _report_and_assert(case.id, got, d, case.ill)
    if case.inp == "const" and case.out == "y":   # variance 0: exactly beta through FiLM and SiLU, whatever the pixel
        cpg = c // groups
        assert _bits_equal(outs[0][0, :, :cpg], outs[0][0, :1, :cpg].expand(hw, cpg)), case.id


def _pack_bias_only(lib, L, cout, bias):
    """A packed 1x1 convolution whose only use is to carry `bias` (zeros without one) as a deferred output's shift."""
    wt = torch.zeros(cout, 32, 1, 1, device="cuda")
    nb = lib.s3d_conv_packed_bytes(cout, 32, 0, 1)
    buf = torch.empty(nb, dtype=torch.uint8, device="cuda")
    bgpu = bias.cuda() if bias is not None else None
    L.check(lib.s3d_conv_pack(wt.data_ptr(), _ptr(bgpu), cout, 32, 0, 1, buf.data_ptr(), nb, None), "s3d_conv_pack")
    torch.cuda.synchronize()
    return buf


def _partial_call(lib, L, case, d, dev, fin, out, stats):
    desc = L.S3dConvPartial(dev["parts"].data_ptr(), case.nsplit, dev["packed"].data_ptr(), case.c0, 32, 0, 1, _ptr(dev["res"]),
                            fin.data_ptr())
    eps = C.c_float(K.GN_EPS)
    if case.out == "table":
        return lib.s3d_group_norm_table_fwd(None, case.c0, _ptr(dev["x1"]), case.c1, dev["gamma"].data_ptr(),
                                            dev["beta"].data_ptr(), dev["fptr"], dev["fstride"], out.data_ptr(), stats.data_ptr(),
                                            case.n, case.hw, case.groups, eps, C.byref(desc), None)
    return lib.s3d_group_norm_partial_fwd(C.byref(desc), dev["gamma"].data_ptr(), dev["beta"].data_ptr(), dev["fptr"],
                                          dev["fstride"], out.data_ptr(), stats.data_ptr(), case.n, case.hw, case.groups, eps,
                                          case.silu, None)


def _partial_device(lib, L, case, d):
    fg, fptr, fstride = _film_args(d)
    return dict(parts=d["parts"].cuda(), packed=_pack_bias_only(lib, L, case.c0, d["bias"]),
                res=d["res"].cuda() if d["res"] is not None else None, x1=d["x1"].cuda() if d["x1"] is not None else None,
                gamma=d["gamma"].cuda(), beta=d["beta"].cuda(), film=fg, fptr=fptr, fstride=fstride)


@pytest.mark.parametrize("case", K.GN_PARTIAL_CASES, ids=[c.id for c in K.GN_PARTIAL_CASES])
def test_group_norm_of_a_deferred_split_k_output_matches_fp64(case):
    """Source 0 as raw split-K partial sums: the GroupNorm against float64 and the finished tensor it writes on the way
    against s3d_conv_finish_fwd on the same partials, bit for bit."""
    L, lib = _lib()
    d = K.gn_partial_build(case)
    dev = _partial_device(lib, L, case, d)
    n, hw, c = case.n, case.hw, case.c0 + case.c1
    nstats = lib.s3d_group_norm_stats_floats(n, case.groups)
    outs, fins = [], []
    for _ in range(2):
        sbuf, stats = _guarded((nstats,))
        fbuf, fin = _guarded((n, hw, case.c0))
        obuf, out = _guarded((n, 2, c) if case.out == "table" else (n, hw, c))
        L.check(_partial_call(lib, L, case, d, dev, fin, out, stats), case.id)
        torch.cuda.synchronize()
        assert _guards_intact(obuf) and _guards_intact(sbuf) and _guards_intact(fbuf), (case.id, "a write outside a buffer")
        assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(fin).all()), (case.id, "an element left unwritten")
        outs.append(out)
        fins.append(fin)
    assert _bits_equal(outs[0], outs[1]) and _bits_equal(fins[0], fins[1]), (case.id, "second call")
    rbuf, fin_ref = _guarded((n, hw, case.c0))
    desc = L.S3dConvPartial(dev["parts"].data_ptr(), case.nsplit, dev["packed"].data_ptr(), case.c0, 32, 0, 1, _ptr(dev["res"]),
                            fin_ref.data_ptr())
    L.check(lib.s3d_conv_finish_fwd(C.byref(desc), n, hw, 1, None), "s3d_conv_finish_fwd")
    torch.cuda.synchronize()
    assert _guards_intact(rbuf)
    assert _bits_equal(fins[0], fin_ref), (case.id, "finished tensor differs from s3d_conv_finish_fwd")
    e_fin, s_fin = K.err_and_scale(fins[0].cpu(), d["fin64"])
    assert e_fin <= K.TOL32 * s_fin, (case.id, e_fin)
    got = _table_applied(d["x"], outs[0]) if case.out == "table" else outs[0]
    _report_and_assert(case.id, got, d, False)


def test_group_norm_refuses_a_one_split_descriptor():
    """A deferred output has at least two splits (a one-split convolution writes its output itself): nsplit 1 is refused by
    both entry points and by s3d_conv_finish_fwd, and nothing is written."""
    L, lib = _lib()
    case = K.GN_PARTIAL_REFUSED
    d = K.gn_partial_build(case)
    dev = _partial_device(lib, L, case, d)
    nstats = lib.s3d_group_norm_stats_floats(case.n, case.groups)
    def untouched(*bufs):
        torch.cuda.synchronize()
        return all(bool((b.view(torch.int32) == NAN_BITS).all()) for b in bufs)

    for out_kind in ("y", "table"):
        cs = case._replace(out=out_kind)
        sbuf, stats = _guarded((nstats,))
        fbuf, fin = _guarded((cs.n, cs.hw, cs.c0))
        obuf, out = _guarded((cs.n, 2, cs.c0) if out_kind == "table" else (cs.n, cs.hw, cs.c0))
        assert _partial_call(lib, L, cs, d, dev, fin, out, stats) != 0
        assert untouched(sbuf, fbuf, obuf), (out_kind, "a refused call wrote output, finished tensor, scratch or a guard")
    fbuf, fin = _guarded((case.n, case.hw, case.c0))
    desc = L.S3dConvPartial(dev["parts"].data_ptr(), 1, dev["packed"].data_ptr(), case.c0, 32, 0, 1, None, fin.data_ptr())
    assert lib.s3d_conv_finish_fwd(C.byref(desc), case.n, case.hw, 1, None) != 0
    assert untouched(fbuf), "a refused s3d_conv_finish_fwd wrote the finished tensor or a guard"


# ------------------------------------------------------------------------------------------------------------------ attention
@pytest.mark.parametrize("case", K.ATTN_CASES, ids=[c.id for c in K.ATTN_CASES])
def test_attention_matches_fp64(case):
    L, lib = _lib()
    d = K.attn_build(case)
    n, t, heads, ch = case.n, case.t, case.heads, case.ch
    qkv = d["qkv"].reshape(n, t, heads * 3 * ch).cuda()
    outs = []
    if case.entry == "fwd":
        for prec in (L.PREC_F32, L.PREC_F16X3, L.PREC_F32):   # (one kernel serves both modes)
            obuf, out = _guarded((n, t, heads * ch))
            L.check(lib.s3d_qkv_attention_fwd(qkv.data_ptr(), out.data_ptr(), n, t, heads, ch, prec, None), case.id)
            torch.cuda.synchronize()
            assert _guards_intact(obuf) and bool(torch.isfinite(out).all()), (case.id, prec)
            outs.append(out)
    else:
        nb = lib.s3d_qkv_attention_ws_bytes(n, t, heads, ch)
        assert nb > 0
        for fill in (None, 0x3C, None):   # workspace prefill: the NaN pattern, finite garbage, the NaN pattern again
            obuf, out = _guarded((n, t, heads * ch))
            wbuf, ws = _guarded_bytes(nb, fill)
            assert ws.data_ptr() % 256 == 0
            L.check(lib.s3d_qkv_attention_ws_fwd(qkv.data_ptr(), out.data_ptr(), n, t, heads, ch, ws.data_ptr(), nb, None), case.id)
            torch.cuda.synchronize()
            assert _guards_intact(obuf) and bool(torch.isfinite(out).all()), (case.id, fill)
            assert _byte_guards_intact(wbuf, nb), (case.id, "a write outside the workspace")
            outs.append(out)
        if nb > 4:   # one byte less than s3d_qkv_attention_ws_bytes is refused
            assert lib.s3d_qkv_attention_ws_fwd(qkv.data_ptr(), out.data_ptr(), n, t, heads, ch, ws.data_ptr(), nb - 1, None) != 0
    for o in outs[1:]:
        assert _bits_equal(outs[0], o), (case.id, "second call / workspace contents / precision mode")
    _report_and_assert(case.id, outs[0], d, case.ill)
    if case.inp == "allequal":    # the mean of V
        v = d["qkv"][:, :, :, 2].double().mean(1, keepdim=True).expand(n, t, heads, ch).reshape(n, t, heads * ch)
        assert float((outs[0].cpu().double() - v).abs().max()) <= K.TOL32 * max(1.0, float(v.abs().max())), case.id


def test_attention_workspace_entry_point_leaves_other_widths_to_the_fp32_kernel():
    L, lib = _lib()
    for ch in K.WS_UNSERVED_WIDTHS:
        for n, t, heads in ((1, 64, 8), (2, 1025, 3)):
            assert lib.s3d_qkv_attention_ws_bytes(n, t, heads, ch) == 0, ch
    qkv = torch.zeros(1, 64, 8 * 3 * 64, device="cuda")
    out = torch.zeros(1, 64, 8 * 64, device="cuda")
    ws = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda")
    assert lib.s3d_qkv_attention_ws_fwd(qkv.data_ptr(), out.data_ptr(), 1, 64, 8, 64, ws.data_ptr(), ws.numel(), None) != 0
    assert lib.s3d_qkv_attention_fwd(qkv.data_ptr(), out.data_ptr(), 1, 64, 8, 40, L.PREC_F32, None) != 0   # width not built


# --------------------------------------------------------------------------------------------------------------- small layers
@pytest.mark.parametrize("case", K.LIN_CASES, ids=[c.id for c in K.LIN_CASES])
def test_small_linear_matches_fp64(case):
    L, lib = _lib()
    d = K.lin_build(case)
    xg = d["x"].cuda()
    wbuf = torch.zeros(case.m * case.k + 4, device="cuda")
    wg = wbuf[case.woff:case.woff + case.m * case.k].view(case.m, case.k)
    wg.copy_(d["w"])
    assert (wg.data_ptr() % 16 == 0) == (case.woff % 4 == 0)
    bgpu = d["b"].cuda() if d["b"] is not None else None
    outs = []
    for _ in range(2):
        obuf, out = _guarded((case.n, case.m))
        L.check(lib.s3d_small_linear_fwd(xg.data_ptr(), wg.data_ptr(), _ptr(bgpu), out.data_ptr(), case.n, case.k, case.m,
                                         case.silu, None), case.id)
        torch.cuda.synchronize()
        assert _guards_intact(obuf) and bool(torch.isfinite(out).all()), case.id
        outs.append(out)
    assert _bits_equal(outs[0], outs[1]), (case.id, "second call")
    _report_and_assert(case.id, outs[0], d, False)


@pytest.mark.parametrize("case", K.TS_CASES, ids=[c[0] for c in K.TS_CASES])
def test_timestep_embedding_matches_fp64(case):
    """Gate: max(project bound, 4 x the error of the reference formula evaluated in fp32 on the CPU) (t = 999 puts the
    argument's own rounding, 999 * 2^-24, into every fp32 evaluation)."""
    L, lib = _lib()
    name, n, dim = case
    t = K.ts_input(n)
    d = dict(ref64=K.ts_ref(t, dim, torch.float64), ref32=K.ts_ref(t, dim, torch.float32))
    tg = t.cuda()
    outs = []
    for _ in range(2):
        obuf, out = _guarded((n, dim))
        L.check(lib.s3d_timestep_embedding_fwd(tg.data_ptr(), out.data_ptr(), n, dim, C.c_float(K.TS_MAX_PERIOD), None), name)
        torch.cuda.synchronize()
        assert _guards_intact(obuf) and bool(torch.isfinite(out).all()), name
        outs.append(out)
    assert _bits_equal(outs[0], outs[1])
    if dim % 2:
        assert bool((outs[0][:, -1] == 0).all())
    _report_and_assert("timestep_embedding-" + name, outs[0], d, True)


@pytest.mark.parametrize("case", K.RESAMPLE_CASES, ids=[c[0] for c in K.RESAMPLE_CASES])
def test_resample2x_matches_fp64(case):
    L, lib = _lib()
    name, up, n, h, w, c = case
    x = torch.randn(n, h, w, c, generator=torch.Generator().manual_seed(K.seed_of(name))) * 3.0 + 1.0
    xg = x.cuda()
    shape = (n, 2 * h, 2 * w, c) if up else (n, h // 2, w // 2, c)
    outs = []
    for _ in range(2):
        obuf, out = _guarded(shape)
        L.check(lib.s3d_resample2x_fwd(xg.data_ptr(), out.data_ptr(), n, h, w, c, up, None), name)
        torch.cuda.synchronize()
        assert _guards_intact(obuf) and bool(torch.isfinite(out).all()), name
        outs.append(out)
    assert _bits_equal(outs[0], outs[1])
    if up:
        assert torch.equal(outs[0].cpu(), K.resample_ref(x, 1, torch.float32)), name        # a copy: exact
    else:
        d = dict(ref64=K.resample_ref(x, 0, torch.float64), ref32=K.resample_ref(x, 0, torch.float32))
        _report_and_assert("avgpool2x-" + name, outs[0], d, False, K.TOL_POOL)


def test_add_kernels_and_layout_copy_are_exact():
    L, lib = _lib()
    g = torch.Generator().manual_seed(11)
    for nfl in K.ADD_CASES:
        a, b = torch.randn(nfl, generator=g), torch.randn(nfl, generator=g)
        ag, bgpu = a.cuda(), b.cuda()
        obuf, out = _guarded((nfl,))
        L.check(lib.s3d_add_fwd(ag.data_ptr(), bgpu.data_ptr(), out.data_ptr(), nfl, None), "s3d_add_fwd")
        torch.cuda.synchronize()
        assert _guards_intact(obuf) and torch.equal(out.cpu(), a + b), nfl
    for n, c, h, w in K.ADD_NCHW_CASES:
        a, b = torch.randn(n, h, w, c, generator=g), torch.randn(n, c, h, w, generator=g)
        ag, bgpu = a.cuda(), b.cuda()
        obuf, out = _guarded((n, h, w, c))
        L.check(lib.s3d_add_nchw_fwd(ag.data_ptr(), bgpu.data_ptr(), out.data_ptr(), n, c, h, w, None), "s3d_add_nchw_fwd")
        torch.cuda.synchronize()
        assert _guards_intact(obuf) and torch.equal(out.cpu(), a + b.permute(0, 2, 3, 1)), (n, c, h, w)
    for n, c, h, w, cpad in K.NCHW_PAD_CASES:
        x = torch.randn(n, c, h, w, generator=g)
        xg = x.cuda()
        obuf, out = _guarded((n, h, w, cpad))
        L.check(lib.s3d_nchw_to_nhwc_pad(xg.data_ptr(), out.data_ptr(), n, c, h, w, cpad, None), "s3d_nchw_to_nhwc_pad")
        torch.cuda.synchronize()
        assert _guards_intact(obuf), (n, c, h, w, cpad)
        assert torch.equal(out[..., :c].cpu(), x.permute(0, 2, 3, 1)), (n, c, h, w, cpad)
        assert bool((out[..., c:].view(torch.int32) == 0).all()), "pad channels c .. cpad hold +0.0"

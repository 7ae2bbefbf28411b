// api_ldm.inc — C ABI of the latent-diffusion U-Net primitives (SURVEY.md 8(f-4); reference
// gen_slices/ldm/modules/diffusionmodules/openaimodel.py).  The block structure (ResBlock / AttentionBlock /
// UNetModel.forward) is host logic and lives in slice3d_amd/ldm_unet.py, mirroring the reference's modules;
// every tensor op it performs is one of these entry points.  Tensors are channels-last fp32.

struct GenConvLayout {
    int cout_pad, KU;
    size_t w, w16, scale, shift, total;
};
static GenConvLayout gen_conv_layout(int cout, int cin0, int cin1, int ks) {
    GenConvLayout L;
    L.cout_pad = pad16(cout);
    const int taps = ks * ks;
    L.KU = taps * (pad16(cin0) + pad16(cin1)) / 16;
    size_t off = 0;
    auto take = [&](size_t n) {
        size_t o = off;
        off += (n + 3) / 4 * 4;
        return o;
    };
    L.w = take((size_t)L.cout_pad * L.KU * 16);
    L.w16 = take((size_t)L.cout_pad * L.KU * 16);
    L.scale = take(L.cout_pad);
    L.shift = take(L.cout_pad);
    L.total = off;
    return L;
}

extern "C" size_t s3d_conv_packed_bytes(int cout, int cin0, int cin1, int ks) {
    return gen_conv_layout(cout, cin0, cin1, ks).total * sizeof(float);
}

// w: (cout, cin0 + cin1, ks, ks) torch layout (a Conv1d(k=1) weight (cout, cin, 1) is the ks = 1 case); bias or NULL
extern "C" int s3d_conv_pack(const float* w, const float* bias, int cout, int cin0, int cin1, int ks, void* packed,
                             size_t packed_bytes, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    S3D_CHECK_ARG(w && packed && cout >= 1 && cin0 >= 1 && cin1 >= 0 && (ks == 1 || ks == 3), "conv_pack: bad arguments");
    const GenConvLayout L = gen_conv_layout(cout, cin0, cin1, ks);
    if (packed_bytes < L.total * sizeof(float)) {
        s3d_set_error("conv_pack: packed buffer %zu < %zu bytes", packed_bytes, L.total * sizeof(float));
        return S3D_E_WORKSPACE;
    }
    float* b = (float*)packed;
    const int taps = ks * ks, ct = cin0 + cin1;
    const bool f16 = L.KU % 2 == 0 && cin0 % 32 == 0 && cin1 % 32 == 0;
    TRY(pack_conv3(w, b + L.w, cout, L.cout_pad, ct, 0, cin0, L.KU, 0, taps, st));
    if (f16) TRY(pack_conv3(w, b + L.w16, cout, L.cout_pad, ct, 0, cin0, L.KU, 0, taps, st, 1));
    if (cin1 > 0) {
        TRY(pack_conv3(w, b + L.w, cout, L.cout_pad, ct, cin0, cin1, L.KU, taps * pad16(cin0) / 16, taps, st));
        if (f16) TRY(pack_conv3(w, b + L.w16, cout, L.cout_pad, ct, cin0, cin1, L.KU, taps * pad16(cin0) / 16, taps, st, 1));
    }
    TRY(launch_fold_bn(bias, nullptr, b + L.scale, b + L.shift, cout, L.cout_pad, 1, 0, st));
    return 0;
}

// out[n,y,x,:cout] = conv(cat(x0, x1)) + bias (+ residual); x0 (N,H,W,pad16(cin0)), x1 (N,H,W,pad16(cin1)) or NULL;
// out / residual have cout channels (channel stride cout, cout % 4 == 0).  "same" padding, stride 1.
static int conv_fwd_desc(ConvLaunch& c, const void* packed, const float* x0, const float* x1, const float* residual, float* out,
                         int N, int H, int W, int cout, int cin0, int cin1, int ks, int prec, void* workspace,
                         size_t workspace_bytes, const ConvGn* gn, int* splits_out) {
    if (gn)
        S3D_CHECK_ARG(s3d_conv_gn_supported(cout, cin0, cin1, ks, prec, H, W, workspace && workspace_bytes >= sizeof(float)),
                      "conv_gn_fwd: needs ks 3, split precision, channel counts that are multiples of 32 (at most %d inputs) and, below "
                      "an 8 x 16 map, a split-K workspace (s3d_conv_gn_supported)", S3D_GN_CMAX);
    S3D_CHECK_ARG(packed && x0 && out && N >= 1 && H >= 1 && W >= 1 && (ks == 1 || ks == 3) && cout % 4 == 0,
                  "conv_fwd: bad arguments");
    S3D_CHECK_ARG((cin1 > 0) == (x1 != nullptr), "conv_fwd: x1 / cin1 mismatch");
    const GenConvLayout L = gen_conv_layout(cout, cin0, cin1, ks);
    const float* b = (const float*)packed;
    c = {};
    c.N = N; c.H = H; c.W = W; c.ks = ks;
    c.CoutPad = L.cout_pad; c.wpk = b + L.w; c.KU = L.KU;
    const bool f16 = L.KU % 2 == 0 && cin0 % 32 == 0 && cin1 % 32 == 0;
    // S3D_PREC_F16: the single-pass throughput mode (one f16 MFMA per product, what BASELINE configs[4]'s "bf16" names) —
    // layers without an f16 image (channel counts that are not multiples of 32: the stem) stay on the exact fp32 MFMA
    S3D_CHECK_ARG(prec == S3D_PREC_F32 || prec == S3D_PREC_F16X3 || prec == S3D_PREC_F16, "conv_fwd: precision mode %d", prec);
    c.wpk16 = (prec != S3D_PREC_F32 && f16) ? (const void*)(b + L.w16) : nullptr;
    c.single_pass = prec == S3D_PREC_F16 && f16;
    c.scale = nullptr;   // s3d_conv_pack folds no BatchNorm: the packed scale is all ones
    c.shift = b + L.shift; c.act = S3D_ACT_NONE;
    c.out_mode = S3D_OUT_NHWC; c.cout_store = cout; c.out_cstride = cout;
    c.nsrc = cin1 > 0 ? 2 : 1;
    c.src[0] = plain_src(x0, pad16(cin0));
    if (cin1 > 0) c.src[1] = plain_src(x1, pad16(cin1));
    c.out = out; c.residual = residual;
    if (gn) c.gn = *gn;
    c.splits_out = splits_out;
    if (splits_out) *splits_out = 1;
    if (workspace && workspace_bytes >= sizeof(float)) {
        c.splitk_ws = (float*)workspace;
        c.splitk_floats = workspace_bytes / sizeof(float);
    }
    return 0;
}
static int conv_fwd_impl(const void* packed, const float* x0, const float* x1, const float* residual, float* out,
                         int N, int H, int W, int cout, int cin0, int cin1, int ks, int prec, void* workspace,
                         size_t workspace_bytes, void* stream, const ConvGn* gn, int* splits_out = nullptr) {
    ConvLaunch c;
    TRY(conv_fwd_desc(c, packed, x0, x1, residual, out, N, H, W, cout, cin0, cin1, ks, prec, workspace, workspace_bytes, gn, splits_out));
    return launch_conv(c, (hipStream_t)stream);
}

extern "C" int s3d_conv_fwd(const void* packed, const float* x0, const float* x1, const float* residual, float* out,
                            int N, int H, int W, int cout, int cin0, int cin1, int ks, int prec, void* workspace,
                            size_t workspace_bytes, void* stream) {
    return conv_fwd_impl(packed, x0, x1, residual, out, N, H, W, cout, cin0, cin1, ks, prec, workspace, workspace_bytes, stream,
                         nullptr);
}
// GroupNorm32 (+ FiLM) (+ SiLU) of the input fused into the 3x3 convolution that consumes it (openaimodel.py:188-194 in_layers,
// :229-236 out_layers): `table` = what s3d_group_norm_table_fwd wrote for cat([x0, x1]); the normalised tensor is never
// written.  Served by the LDS-staged split-precision 3x3 kernel only: ks == 3, cin0 / cin1 / cout multiples of 32, prec f16x3
// or f16, cin0 + cin1 <= 1536 — anything else is refused (S3D_E_ARG), the caller then runs s3d_group_norm_fwd + s3d_conv_fwd.
// 1 if s3d_conv_gn_fwd serves this shape (the one statement of its eligibility: callers decide the two-source packing of a
// cat([h, skip]) convolution and the fused / unfused path from it instead of restating the conditions; ADVICE r5).  H, W <= 0:
// map size not known yet (pack time) — maps below the kernel's 8 x 16 tile then count as served only with a split-K workspace.
extern "C" int s3d_conv_gn_supported(int cout, int cin0, int cin1, int ks, int prec, int H, int W, int has_workspace) {
    if (ks != 3 || (prec != S3D_PREC_F16X3 && prec != S3D_PREC_F16)) return 0;
    if (cout <= 0 || cin0 <= 0 || cin1 < 0 || cout % 32 || cin0 % 32 || cin1 % 32) return 0;
    if (cin0 + cin1 > S3D_GN_CMAX) return 0;
    if (H > 0 && W > 0 && conv_below_lds_tile(H, W) && !has_workspace) return 0;
    return 1;
}
extern "C" int s3d_conv_gn_fwd(const void* packed, const float* x0, const float* x1, const float* residual, float* out,
                               int N, int H, int W, int cout, int cin0, int cin1, int ks, int prec, const float* table,
                               int silu, void* workspace, size_t workspace_bytes, int* nsplit_out, void* stream) {
    S3D_CHECK_ARG(table, "conv_gn_fwd: null table");
    const ConvGn gn = {table, silu};
    // nsplit_out != NULL: a split-K launch skips its finish pass — *nsplit_out > 1 then means `out` is NOT written, the raw
    // partial sums sit in `workspace` and the caller hands them to the next GroupNorm (S3dConvPartial) or to s3d_conv_finish_fwd
    return conv_fwd_impl(packed, x0, x1, residual, out, N, H, W, cout, cin0, cin1, ks, prec, workspace, workspace_bytes, stream,
                         &gn, nsplit_out);
}
// the finish pass of a deferred split-K convolution on its own (for consumers that are not a GroupNorm)
static int partial_to_gn(const S3dConvPartial* p, int N, int HW, GnPartial& g) {
    S3D_CHECK_ARG(p->part && p->out && p->conv_packed && p->nsplit >= 2, "conv partial: bad descriptor");
    const GenConvLayout L = gen_conv_layout(p->cout, p->cin0, p->cin1, p->ks);
    S3D_CHECK_ARG(L.cout_pad == p->cout, "conv partial: cout %d is padded to %d", p->cout, L.cout_pad);
    g.part = p->part; g.nsplit = p->nsplit; g.shift = (const float*)p->conv_packed + L.shift; g.res = p->residual; g.fin = p->out;
    (void)N; (void)HW;
    return 0;
}
extern "C" int s3d_conv_finish_fwd(const S3dConvPartial* p, int N, int H, int W, void* stream) {
    S3D_CHECK_ARG(p, "conv_finish: null descriptor");
    GnPartial g;
    TRY(partial_to_gn(p, N, H * W, g));
    ConvLaunch c = {};
    c.N = N; c.H = H; c.W = W; c.ks = p->ks; c.CoutPad = p->cout;
    c.scale = nullptr; c.shift = g.shift; c.act = S3D_ACT_NONE;
    c.out_mode = S3D_OUT_NHWC; c.cout_store = p->cout; c.out_cstride = p->cout;
    c.out = p->out; c.residual = p->residual;
    c.splitk_ws = const_cast<float*>(p->part);
    return launch_conv_splitk_finish(c, p->nsplit, (hipStream_t)stream);
}
// scratch of every GroupNorm entry point below: s3d_group_norm_stats_floats(N, groups) floats
extern "C" size_t s3d_group_norm_stats_floats(int N, int groups) {
    return (size_t)N * groups * S3D_GN_SLICES * 3;
}
// GroupNorm statistics of cat([x0, x1]) folded with gamma / beta (and FiLM: film = (N, film_stride) rows of scale | shift, or
// NULL) into the table s3d_conv_gn_fwd consumes: table[n][0][c] = A, table[n][1][c] = B of  y = x * A + B  (N * 2 * (c0 + c1) floats)
// x0_partial != NULL: source 0 is a deferred split-K convolution output (s3d_conv_gn_fwd with nsplit_out): the statistics
// kernel sums its partials, adds bias and residual, writes the finished tensor to x0_partial->out — x0 is ignored
extern "C" int s3d_group_norm_table_fwd(const float* x0, int c0, const float* x1, int c1, const float* gamma,
                                        const float* beta, const float* film, long film_stride, float* table, float* stats,
                                        int N, int HW, int groups, float eps, const S3dConvPartial* x0_partial, void* stream) {
    S3D_CHECK_ARG((x0 || x0_partial) && gamma && beta && table && stats && c0 > 0 && c1 >= 0 && (c1 > 0) == (x1 != nullptr),
                  "group_norm_table: bad argument");
    S3D_CHECK_ARG(!film || film_stride >= 2L * (c0 + c1), "group_norm_table: film stride %ld", film_stride);
    GnPartial g;
    if (x0_partial) {
        TRY(partial_to_gn(x0_partial, N, HW, g));
        S3D_CHECK_ARG(x0_partial->cout == c0, "group_norm_table: partial source has %d channels, c0 = %d", x0_partial->cout, c0);
    }
    return launch_group_norm(x0, gamma, beta, film, nullptr, stats, N, HW, c0 + c1, groups, eps, 0, (hipStream_t)stream, x1, c0,
                             film_stride, table, x0_partial ? &g : nullptr);
}
// GroupNorm (+ FiLM) (+ SiLU) with the normalised output y, source 0 from a deferred split-K convolution (see above)
extern "C" int s3d_group_norm_partial_fwd(const S3dConvPartial* x0_partial, const float* gamma, const float* beta,
                                          const float* film, long film_stride, float* y, float* stats, int N, int HW, int groups,
                                          float eps, int silu, void* stream) {
    S3D_CHECK_ARG(x0_partial && gamma && beta && y && stats, "group_norm_partial: null argument");
    GnPartial g;
    TRY(partial_to_gn(x0_partial, N, HW, g));
    return launch_group_norm(nullptr, gamma, beta, film, y, stats, N, HW, x0_partial->cout, groups, eps, silu, (hipStream_t)stream,
                             nullptr, 0, film_stride, nullptr, &g);
}
extern "C" int s3d_group_norm_fwd(const float* x, const float* gamma, const float* beta, const float* film, float* y,
                                  float* stats, int N, int HW, int C, int groups, float eps, int silu, void* stream) {
    S3D_CHECK_ARG(x && gamma && beta && y && stats, "group_norm: null argument");
    return launch_group_norm(x, gamma, beta, film, y, stats, N, HW, C, groups, eps, silu, (hipStream_t)stream);
}
// the same with the FiLM rows read in place from a wider (N, film_stride) tensor: the emb_layers of all ResBlocks are one
// stacked GEMV (openaimodel.py:222-228,262 per block), a block's (scale | shift) is a column range of its output
extern "C" int s3d_group_norm_film_fwd(const float* x, const float* gamma, const float* beta, const float* film,
                                       long film_stride, float* y, float* stats, int N, int HW, int C, int groups, float eps,
                                       int silu, void* stream) {
    S3D_CHECK_ARG(x && gamma && beta && film && y && stats && film_stride >= 2L * C, "group_norm_film: bad argument");
    return launch_group_norm(x, gamma, beta, film, y, stats, N, HW, C, groups, eps, silu, (hipStream_t)stream, nullptr, 0,
                             film_stride);
}
// GroupNorm of the channel concatenation cat([x0 (c0 channels), x1 (c1 channels)], dim=C) without materialising it
extern "C" int s3d_group_norm2_fwd(const float* x0, int c0, const float* x1, int c1, const float* gamma,
                                   const float* beta, const float* film, float* y, float* stats, int N, int HW,
                                   int groups, float eps, int silu, void* stream) {
    S3D_CHECK_ARG(x0 && x1 && gamma && beta && y && stats && c0 > 0 && c1 > 0, "group_norm2: bad argument");
    return launch_group_norm(x0, gamma, beta, film, y, stats, N, HW, c0 + c1, groups, eps, silu, (hipStream_t)stream, x1,
                             c0);
}
extern "C" int s3d_qkv_attention_fwd(const float* qkv, float* out, int N, int T, int heads, int ch, int prec,
                                     void* stream) {
    S3D_CHECK_ARG(qkv && out, "qkv_attention: null argument");
    S3D_CHECK_ARG(prec == S3D_PREC_F32 || prec == S3D_PREC_F16X3, "qkv_attention: precision mode %d", prec);
    return launch_qkv_attention(qkv, out, N, T, heads, ch, prec, (hipStream_t)stream);
}
// The same attention with fp32-class logits on the f16 MFMA for head widths 8 / 16 / 24 / 32 (ldm_attn.hip); `ws` holds
// the pre-split K / V block images (s3d_qkv_attention_ws_bytes; 0 = width not served, call s3d_qkv_attention_fwd)
extern "C" size_t s3d_qkv_attention_ws_bytes(int N, int T, int heads, int ch) {
    return qkv_attention_ws_bytes(N, T, heads, ch);
}
extern "C" int s3d_qkv_attention_ws_fwd(const float* qkv, float* out, int N, int T, int heads, int ch, void* ws,
                                        size_t ws_bytes, void* stream) {
    S3D_CHECK_ARG(qkv && out, "qkv_attention_ws: null argument");
    return launch_qkv_attention_ws(qkv, out, N, T, heads, ch, ws, ws_bytes, (hipStream_t)stream);
}
extern "C" int s3d_resample2x_fwd(const float* x, float* y, int N, int H, int W, int C, int up, void* stream) {
    S3D_CHECK_ARG(x && y, "resample2x: null argument");
    return launch_resample2x(x, y, N, H, W, C, up, (hipStream_t)stream);
}
extern "C" int s3d_small_linear_fwd(const float* x, const float* w, const float* b, float* out, int N, int K, int M,
                                    int silu_in, void* stream) {
    S3D_CHECK_ARG(x && w && out, "small_linear: null argument");
    return launch_small_linear(x, w, b, out, N, K, M, silu_in, (hipStream_t)stream);
}
extern "C" int s3d_timestep_embedding_fwd(const float* t, float* out, int N, int dim, float max_period, void* stream) {
    S3D_CHECK_ARG(t && out, "timestep_embedding: null argument");
    return launch_timestep_embedding(t, out, N, dim, max_period, (hipStream_t)stream);
}
extern "C" int s3d_add_fwd(const float* a, const float* b, float* out, long n, void* stream) {
    S3D_CHECK_ARG(a && b && out, "add: null argument");
    return launch_add(a, b, out, n, (hipStream_t)stream);
}
extern "C" int s3d_add_nchw_fwd(const float* a, const float* b, float* out, int n, int c, int h, int w, void* stream) {
    S3D_CHECK_ARG(a && b && out && n >= 1 && c >= 1 && h >= 1 && w >= 1, "add_nchw: bad arguments");
    return launch_add_nchw(a, b, out, n, c, h, w, (hipStream_t)stream);
}
extern "C" int s3d_nchw_to_nhwc_pad(const float* in, float* out, int n, int c, int h, int w, int cpad, void* stream) {
    S3D_CHECK_ARG(in && out && cpad >= c && cpad % 4 == 0, "nchw_to_nhwc_pad: bad arguments");
    return launch_nchw_to_nhwc(in, out, n, c, h, w, cpad, (hipStream_t)stream);
}

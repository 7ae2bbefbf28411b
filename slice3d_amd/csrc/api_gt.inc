// api_gt.inc — Slices3DGTModel (reg_slices/src/model_gt.py:12-111), the regression model that reads the GIVEN
// slice images instead of generating them: VGG16-BN feature pyramid of the 12 slice images
// (vgg16bn_feats.py:26-57: raw conv1_2 / conv2_2 / conv3_3 / conv4_3 / conv5_3 outputs), bilinear samples of the
// five levels (1472 channels), fc_local (1472->128->128, ReLU), pts_feat_extractor (3->32->64->128), then the
// same 3-layer transformer + fc_out as Slices3DRegModel.  Included by api.hip; reuses the conv engine, the
// decoder kernels and the packed-head machinery.
//
// fc_local[0] is folded into the four coarse levels (sampling and a linear map commute): conv2_2..conv5_3 are
// projected to 128-channel maps once per object; the 64-channel conv1_2 level (the largest map) stays raw and
// meets its 128x64 weight slice on the MFMA inside the sampler.

static const int kGtC[5] = {64, 128, 256, 512, 512};            // conv1_2 ... conv5_3
static const int kGtCol[5] = {0, 64, 192, 448, 960};            // column offsets inside fc_local[0].weight (128,1472)

struct GtEncLayout {
    EncLayout E;
    size_t total;
};
static GtEncLayout gt_enc_layout() {
    ImageAlloc a;
    const EncLayout E = enc_layout(a);
    return GtEncLayout{E, a.off};
}
extern "C" size_t s3d_gt_encoder_packed_bytes(void) { return gt_enc_layout().total * sizeof(float); }

extern "C" int s3d_gt_encoder_pack(const S3dVgg16BnParams* P, void* packed, size_t packed_bytes, void* stream) {
    S3D_CHECK_ARG(P && packed, "gt_encoder_pack: null argument");
    const GtEncLayout L = gt_enc_layout();
    if (packed_bytes < L.total * sizeof(float)) {
        s3d_set_error("gt_encoder_pack: packed buffer %zu < %zu bytes", packed_bytes, L.total * sizeof(float));
        return S3D_E_WORKSPACE;
    }
    return pack_encoder(P->conv, (float*)packed, L.E, (hipStream_t)stream);
}

struct GtEncWs {
    size_t in16, a, b, p[4], splitk, total;
};
static GtEncWs gt_enc_ws(int n_img, int S) {
    GtEncWs W;
    size_t off = 0;
    auto take = [&](size_t n) {
        size_t o = off;
        off += (n + 63) / 64 * 64;
        return o;
    };
    const size_t px = (size_t)n_img * S * S;
    W.in16 = take(px * 16);
    W.a = take(px * 64);
    W.b = take(px * 64 / 2);
    for (int i = 0; i < 4; ++i) W.p[i] = take((px >> (2 * (i + 1))) * kGtC[i]);
    W.splitk = take(S3D_SPLITK_FLOATS);
    W.total = off;
    return W;
}
extern "C" size_t s3d_gt_encoder_workspace_bytes(int n_img, int size) {
    return gt_enc_ws(n_img, size).total * sizeof(float);
}

extern "C" int s3d_gt_encode_fwd(const void* packed, const float* img_slices, const S3dGtPyramid* out, int n_img,
                                 int S, int prec, void* workspace, size_t workspace_bytes, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    S3D_CHECK_ARG(prec == S3D_PREC_F32 || prec == S3D_PREC_F16X3 || prec == S3D_PREC_F16, "gt_encode: precision mode %d", prec);
    S3D_CHECK_ARG(packed && img_slices && out && workspace, "gt_encode: null argument");
    S3D_CHECK_ARG(n_img >= 1 && S >= 16 && S % 16 == 0, "gt_encode: n_img=%d S=%d (S must be a multiple of 16)", n_img, S);
    S3D_CHECK_ARG(out->n_img == n_img && out->size == S, "gt_encode: pyramid handle mismatch");
    const GtEncLayout L = gt_enc_layout();
    const GtEncWs W = gt_enc_ws(n_img, S);
    if (workspace_bytes < W.total * sizeof(float)) {
        s3d_set_error("gt_encode: workspace %zu < %zu bytes", workspace_bytes, W.total * sizeof(float));
        return S3D_E_WORKSPACE;
    }
    float* ws = (float*)workspace;
    ProfScope prof_(S3D_PROF_UNET, st);
    TRY(launch_nchw_to_nhwc(img_slices, ws + W.in16, n_img, 3, S, S, 16, st));
    float* const pp[2] = {ws + W.a, ws + W.b};
    float* const pool[4] = {ws + W.p[0], ws + W.p[1], ws + W.p[2], ws + W.p[3]};
    return encoder_fwd((const float*)packed, L.E, prec, n_img, S, 0, ws + W.in16, out->level, pp, pool, ws + W.splitk, st);
}

// ------------------------------------------------------------------------------------------------
// head
// ------------------------------------------------------------------------------------------------
struct GtHeadLayout {
    HeadLayout H;            // transformer layers + fc_out live in the standard head image (offset 0)
    size_t wproj[4], wproj16[4];   // fc_local[0] slices for conv5_3, conv4_3, conv3_3, conv2_2 (coarse -> fine)
    size_t wraw, bl0;        // fc_local[0][:, 0:64] fragments, fc_local[0].bias
    size_t wraw16;           // the raw block as f16 hi/lo fragment pairs
    size_t wl1, wl1_16, bl1; // fc_local[2]
    size_t pw0, pb0, pw1, pb1, pw2, pb2;
    size_t total;
};
static GtHeadLayout gt_head_layout() {
    GtHeadLayout G;
    G.H = head_layout();
    size_t off = G.H.total;
    auto take = [&](size_t n) {
        size_t o = off;
        off += (n + 3) / 4 * 4;
        return o;
    };
    for (int l = 0; l < 4; ++l) {
        G.wproj[l] = take((size_t)128 * kGtC[4 - l]);
        G.wproj16[l] = take((size_t)128 * kGtC[4 - l]);
    }
    G.wraw = take(128 * 64);
    G.wraw16 = take(128 * 64);
    G.bl0 = take(128);
    G.wl1 = take(128 * 128);
    G.wl1_16 = take(128 * 128);
    G.bl1 = take(128);
    G.pw0 = take(96); G.pb0 = take(32); G.pw1 = take(2048); G.pb1 = take(64); G.pw2 = take(8192); G.pb2 = take(128);
    G.total = off;
    return G;
}
extern "C" size_t s3d_gt_head_packed_bytes(void) { return gt_head_layout().total * sizeof(float); }

extern "C" int s3d_gt_head_pack(const S3dGtHeadParams* P, void* packed, size_t packed_bytes, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    S3D_CHECK_ARG(P && packed, "gt_head_pack: null argument");
    const GtHeadLayout G = gt_head_layout();
    if (packed_bytes < G.total * sizeof(float)) {
        s3d_set_error("gt_head_pack: packed buffer %zu < %zu bytes", packed_bytes, G.total * sizeof(float));
        return S3D_E_WORKSPACE;
    }
    float* b = (float*)packed;
    TRY(pack_head_layers(P->layer, b, G.H, st, false));
    TRY(copy_vec(b + G.H.fco_w, P->fc_out_w, 128, st));
    TRY(copy_vec(b + G.H.fco_b, P->fc_out_b, 1, st));
    for (int l = 0; l < 4; ++l) {   // proj[l] <- pyramid level 4 - l
        const int C = kGtC[4 - l], col = kGtCol[4 - l];
        TRY(pack_linear(P->local_w[0] + col, b + G.wproj[l], 128, 128, C, 1472, 0, st));
        TRY(pack_linear(P->local_w[0] + col, b + G.wproj16[l], 128, 128, C, 1472, 0, st, 1));
    }
    TRY(pack_linear(P->local_w[0], b + G.wraw, 128, 128, 64, 1472, 0, st));
    TRY(pack_linear(P->local_w[0], b + G.wraw16, 128, 128, 64, 1472, 0, st, 1));
    TRY(copy_vec(b + G.bl0, P->local_b[0], 128, st));
    TRY(pack_linear(P->local_w[1], b + G.wl1, 128, 128, 128, 128, 0, st));
    TRY(pack_linear(P->local_w[1], b + G.wl1_16, 128, 128, 128, 128, 0, st, 1));
    TRY(copy_vec(b + G.bl1, P->local_b[1], 128, st));
    TRY(copy_vec(b + G.pw0, P->pts_w[0], 96, st));
    TRY(copy_vec(b + G.pb0, P->pts_b[0], 32, st));
    TRY(copy_vec(b + G.pw1, P->pts_w[1], 2048, st));
    TRY(copy_vec(b + G.pb1, P->pts_b[1], 64, st));
    TRY(copy_vec(b + G.pw2, P->pts_w[2], 8192, st));
    TRY(copy_vec(b + G.pb2, P->pts_b[2], 128, st));
    return 0;
}

extern "C" int s3d_gt_latent_build(const void* head_packed, const S3dGtPyramid* pyr, const S3dGtLatent* out, int prec,
                                   void* stream) {
    hipStream_t st = (hipStream_t)stream;
    S3D_CHECK_ARG(head_packed && pyr && out, "gt_latent_build: null argument");
    S3D_CHECK_ARG(out->n_img == pyr->n_img && out->size == pyr->size, "gt_latent_build: handle mismatch");
    S3D_CHECK_ARG(out->fine == pyr->level[0], "gt_latent_build: latent.fine must alias pyramid level 0 (conv1_2)");
    const GtHeadLayout G = gt_head_layout();
    const float* b = (const float*)head_packed;
    ProfScope prof_(S3D_PROF_LATENT, st);
    for (int l = 0; l < 4; ++l) {
        const int lev = 4 - l, r = pyr->size >> lev, C = kGtC[lev];
        TRY(launch_conv(proj_desc(b + G.wproj[l], prec != S3D_PREC_F32 ? b + G.wproj16[l] : nullptr, prec == S3D_PREC_F16,
                                  128, C, pyr->level[lev], pyr->n_img, r, r, out->proj[l]),
                        st));
    }
    return 0;
}

// the Reg decoder's workspace (decode_ws) at the fixed pass size, plus the token tensor X1 in front
extern "C" size_t s3d_gt_decode_workspace_bytes(int batch, long n_qry, int n_slices) {
    return decode_ws(batch, n_qry, n_slices, S3D_CHUNK_GROUPS, true).total * sizeof(float);
}

static int gt_decode_impl(const void* head_packed, const S3dGtLatent* lat, const float* qry, const float* rot,
                          const float* trans, int flip_yz, int nx, float box, float sign, float* out, int batch,
                          long n_qry, int ns, int prec, void* workspace, size_t workspace_bytes, hipStream_t st) {
    S3D_CHECK_ARG(head_packed && lat && trans && out && workspace, "gt_decode: null argument");
    S3D_CHECK_ARG(batch >= 1 && n_qry >= 1, "gt_decode: batch=%d n_qry=%ld", batch, n_qry);
    S3D_CHECK_ARG(ns >= 1 && ns <= 12, "gt_decode: n_slices %d", ns);
    S3D_CHECK_ARG(lat->n_img == batch * ns, "gt_decode: latent has %d images, expected %d", lat->n_img, batch * ns);
    S3D_CHECK_ARG(prec == S3D_PREC_F32 || prec == S3D_PREC_F16X3 || prec == S3D_PREC_F16, "gt_decode: precision mode %d not built", prec);
    const DecodeWs W = decode_ws(batch, n_qry, ns, S3D_CHUNK_GROUPS, true);   // fixed pass size: no smaller-pass fallback
    if (workspace_bytes < W.total * sizeof(float)) {
        s3d_set_error("gt_decode: workspace %zu < %zu bytes", workspace_bytes, W.total * sizeof(float));
        return S3D_E_WORKSPACE;
    }
    const GtHeadLayout G = gt_head_layout();
    const float* b = (const float*)head_packed;
    float* X1 = (float*)workspace + W.X1;
    float* X = (float*)workspace + W.X;
    const int T = ns + 1;
    const long gpb = (n_qry + S3D_GROUP - 1) / S3D_GROUP;
    const long Gn = gpb * batch;
    const int* perm = nullptr;
    if (qry && n_qry >= S3D_SORT_MIN_QUERIES) {
        int* pm = (int*)((float*)workspace + W.perm);
        TRY(launch_query_sort(qry, flip_yz ? nullptr : rot, trans, flip_yz, batch, n_qry, pm,
                              (int*)((float*)workspace + W.sortws), st));
        perm = pm;
    }
    DecodeStack D{b, G.H, X, (float*)workspace + W.X0, (float*)workspace + W.last, T, prec, false, false, gpb, n_qry, 0,
                  out, sign, perm, nullptr};
    for (long g0 = 0; g0 < Gn; g0 += S3D_CHUNK_GROUPS) {
        const long gc = Gn - g0 < S3D_CHUNK_GROUPS ? Gn - g0 : S3D_CHUNK_GROUPS;
        {
            ProfScope prof_(S3D_PROF_SAMPLE, st);
            SampleGtArgs sa = {};
            for (int l = 0; l < 4; ++l) sa.proj[l] = lat->proj[l];
            sa.fine = lat->fine;
            sa.wraw = b + G.wraw; sa.bias = b + G.bl0;
            sa.wraw16 = prec != S3D_PREC_F32 ? b + G.wraw16 : nullptr;
            sa.size = lat->size; sa.n_slices = ns;
            sa.qry = qry; sa.rot = rot; sa.trans = trans; sa.flip_yz = flip_yz;
            sa.n_qry = n_qry; sa.groups_per_batch = gpb; sa.g_begin = g0; sa.g_count = gc;
            sa.nx = nx; sa.box = box; sa.X = X1; sa.perm = perm;
            TRY(launch_sample_tokens_gt(sa, st));
            // fc_local[2] + ReLU on every row (token-0 rows are overwritten right after)
            TRY(rows_linear(b, G.wl1, G.wl1_16, 128, 128, b + G.bl1, X1, gc * T * S3D_GROUP, X, nullptr, prec, st,
                            S3D_ACT_RELU));
            GtPointArgs pa = {};
            pa.w0 = b + G.pw0; pa.b0 = b + G.pb0; pa.w1 = b + G.pw1; pa.b1 = b + G.pb1; pa.w2 = b + G.pw2; pa.b2 = b + G.pb2;
            pa.qry = qry; pa.rot = rot; pa.flip_yz = flip_yz; pa.n_slices = ns;
            pa.n_qry = n_qry; pa.groups_per_batch = gpb; pa.g_begin = g0; pa.g_count = gc;
            pa.nx = nx; pa.box = box; pa.X = X; pa.perm = perm;
            TRY(launch_gt_point_tokens(pa, st));
        }
        D.g0 = g0;
        TRY(decode_layers(D, st, 0, gc));
    }
    return 0;
}

extern "C" int s3d_gt_decode_points_fwd(const void* head_packed, const S3dGtLatent* latent, const float* qry,
                                        const float* rot, const float* trans, int flip_yz, float* sdf_out, int batch,
                                        long n_qry, int n_slices, int prec, void* workspace, size_t workspace_bytes,
                                        void* stream) {
    S3D_CHECK_ARG(qry, "gt_decode_points: qry is NULL");
    return gt_decode_impl(head_packed, latent, qry, rot, trans, flip_yz, 0, 1.f, 1.f, sdf_out, batch, n_qry, n_slices,
                          prec, workspace, workspace_bytes, (hipStream_t)stream);
}

extern "C" int s3d_gt_decode_grid_fwd(const void* head_packed, const S3dGtLatent* latent, const float* trans, int nx,
                                      float box, float* logits_out, int n_slices, int prec, void* workspace,
                                      size_t workspace_bytes, void* stream) {
    S3D_CHECK_ARG(nx >= 2 && nx <= 1024, "gt_decode_grid: nx %d", nx);
    const long n = (long)nx * nx * nx;
    return gt_decode_impl(head_packed, latent, nullptr, nullptr, trans, 1, nx, box, -1.f, logits_out, 1, n, n_slices,
                          prec, workspace, workspace_bytes, (hipStream_t)stream);
}

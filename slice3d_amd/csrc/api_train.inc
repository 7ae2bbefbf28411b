// api_train.inc — included at the end of api.hip: train-mode forward + loss + backward orchestration
// (train_step of the reference, reg_slices/train.py:41-53, minus opt.step which is s3d_adam_step).
//
// Everything is fp32.  Weights are re-packed every call (they change every step); activations needed by
// the backward are kept in the caller's workspace (sized by s3d_train_workspace_bytes).

struct Arena {
    float* base;
    size_t off;
    float* take(size_t n) {
        float* p = base ? base + off : nullptr;
        off += (n + 63) / 64 * 64;
        return p;
    }
};

static const int kEncRes[13] = {0, 0, 1, 1, 2, 2, 2, 3, 3, 3, 4, 4, 4};  // log2 downscale of conv i
static const int kTapConv[5] = {1, 3, 6, 9, 12};
static const int kVggRes[14] = {0, 0, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4};

struct FragW {
    float* p;
    float* p16;    // f16 hi/lo fragment-pair image (valid when KU is even and every K segment is a multiple of 32)
    int n_pad, KU;
};

struct TrainBufs {
    // ---- U-Net forward ----
    float* in16;
    float* z[13];
    float* ein[13];          // ein[0] = in16
    float* mean[13];
    float* rstd[13];
    float* F[5];
    float *proj[4], *up[4], *z1[4], *mid[4], *z2[4], *m1[4], *r1[4], *m2[4], *r2[4];
    float* rec;              // (Nd,3,S,S) NCHW
    FragW w_enc[13], w_enc_d[13];
    FragW w_transc, w_transc_d;      // dgrad only w.r.t. the x5 segment
    FragW w_tup[4], w_tup_d[4], w_upt[4], w_upt_d[4], w_c1[4], w_c1_dp[4], w_c1_du[4], w_c2[4], w_c2_d[4];
    FragW w_outc, w_outc_d;
    float* outc_shift;       // padded bias (16)
    float* upt_shift[4];     // ConvT bias tiled over the 4 quadrants
    // ---- U-Net backward ----
    float* drec;
    float* dF[5];
    float* dskip[5];
    float *scrA, *scrB, *scrC, *scrD;   // (Nd,S,S,32)-sized scratch
    float *encA, *encB;                  // (B,S,S,64)-sized scratch
    // ---- VGG ----
    float* vin16;
    float* va[14];
    float* vp[4];
    FragW w_vgg[14], w_vgg_d[14];
    FragW w_vggZ;                         // conv1_1's data gradient as a 1x1 product: rows ci*9 + tap (27), K = 64 output channels
    float *vgA, *vgB;
    // ---- decoder ----
    float* head_packed;
    float* lat_proj[3];
    float* dlat_proj[3];
    FragW w_projT[3];
    float* ws34_t;
    float* ws34_t16;
    float *X0, *raw34, *qrot4;
    int *perm, *sortws;                 // locality order of the queries (Q >= S3D_SORT_MIN_QUERIES)
    float* sb_partial;                  // per-tile footprint slots of the atomic-free sampling backward (train_sbd.hip), or NULL
    float* gxy;                         // projected coordinates of the sorted slots (the tiled sampling backward's pre-pass)
    float *QKV[3], *O[3], *u1[3], *x1[3], *u2[3], *x2[3];
    float *x1c, *u2c, *x2c;             // compact token-0 rows of the last layer
    FragW w_inT[3], w_outT[3], w_1T[3], w_2T[3];
    FragW w_inN[3], w_outN[3], w_1N[3];   // natural-layout images (fp32 + f16) of in_proj / out_proj / linear1
    // last layer, token 0 only, absorbed form (train2.hip): M (512,128) / Naug (128,S3D_ABS_NA) in both operand orders, the matrices
    // themselves, the per-query intermediates (qt, xbar and their gradients) and the gradients of M | m and Naug
    FragW w_absM, w_absMT, w_absN, w_absNT;
    float *absM, *absm, *absN, *qt, *xbar, *dxbar, *dqt, *dMb, *dmb, *dNb;
    float* wT16[3];                       // f16x3 chunk image of (lin2^T, lin1^T) for the fused FFN backward
    float *wrec1[3], *wrec2t[3];          // f16x3 fragment images of lin1 / lin2^T for the recompute weight gradients
    unsigned* fmask[3];                   // activity bits of the FFN hidden units (forward -> backward)
    float* recimg[2];                     // f16 hi/lo operand images of the FFN weight gradients: D^T / R form of dY ...
    float* ximg[3][2];                    // ... and of each layer's FFN input x (written by the forward)
    float *dA, *dB, *dO, *dQKV, *dc1, *dc2, *tmp128, *dmask;
    float *ffA, *ffD;
    long ff_rb;
    float *dsdf, *sdf;
    // ---- shared ----
    float* partial;          // wgrad partial sums
    size_t partial_floats;
    float* cpartial;         // column / scalar reduction partials
    float* vec;              // small vectors (colsum outputs etc.)
    float* fwd_losses;       // [loss_pred, loss_img, loss_vgg, acc] of a forward-only step: the end of vec, beyond its small-vector uses
};

// every size a training step derives from (B, S, Q, ns), computed once: the plans and the run read it from here
struct StepDims {
    int B, S, ns;
    long Q;
    int Nd, Tn, r5;          // slice images B * ns, tokens per query ns + 1, side of the coarsest feature map S / 16
    long gpb, G;             // query groups (of S3D_GROUP) per object / in all
    long rows, rows0;        // token rows G * Tn * S3D_GROUP, token-0 rows G * S3D_GROUP
    long nsdf, nimg;         // elements of sdf_pred (B,Q) and of slices_rec (Nd,3,S,S)
};
static StepDims step_dims(int B, int S, long Q, int ns) {
    StepDims d;
    d.B = B; d.S = S; d.ns = ns; d.Q = Q;
    d.Nd = B * ns; d.Tn = ns + 1; d.r5 = S / 16;
    d.gpb = (Q + S3D_GROUP - 1) / S3D_GROUP; d.G = d.gpb * B;
    d.rows = d.G * d.Tn * S3D_GROUP; d.rows0 = d.G * S3D_GROUP;
    d.nsdf = (long)B * Q; d.nimg = (long)d.Nd * 3 * S * S;
    return d;
}
static const int kLatC[5] = {512, 256, 128, 64, 32};   // channels of the U-Net's feature levels F[0..4]
static const int kFcsCol[3] = {0, 512, 768};            // first column of fc_s.weight that the folded projection of level l uses

static FragW frag_alloc(Arena& A, int n, int k) {
    FragW f;
    f.n_pad = pad16(n);
    f.KU = pad16(k) / 16;
    f.p = A.take((size_t)f.n_pad * f.KU * 16);
    f.p16 = A.take((size_t)f.n_pad * f.KU * 16);
    return f;
}

// VGG16-BN encoder buffers for n_img input images (shared by the two regression models)
static void plan_enc(Arena& A, const StepDims& d, int n_img, TrainBufs& T) {
    const size_t px = (size_t)n_img * d.S * d.S;
    T.in16 = A.take(px * 16);
    T.ein[0] = T.in16;
    for (int i = 0; i < 13; ++i) {
        const size_t pr = px >> (2 * kEncRes[i]);
        T.z[i] = A.take(pr * kEncCout[i]);
        T.mean[i] = A.take(kEncCout[i]);
        T.rstd[i] = A.take(kEncCout[i]);
        if (i < 12) T.ein[i + 1] = A.take((kEncTap[i] ? pr / 4 : pr) * kEncCout[i]);
        T.w_enc[i] = frag_alloc(A, kEncCout[i], 9 * pad16(kEncCin[i]));
        T.w_enc_d[i] = frag_alloc(A, pad16(kEncCin[i]), 9 * kEncCout[i]);
    }
    const int sc[5] = {64, 128, 256, 512, 512};
    for (int k = 0; k < 5; ++k) T.dskip[k] = A.take((px >> (2 * k)) * sc[k]);
    T.encA = A.take(px * 64); T.encB = A.take(px * 64);
}

// transformer decoder buffers (DecoderTrain) for B objects x Q queries x (ns + 1) tokens
static void plan_dec(Arena& A, const StepDims& d, TrainBufs& T) {
    const int B = d.B;
    const long Q = d.Q;
    const size_t rows = (size_t)d.rows, rows0 = (size_t)d.rows0;
    T.X0 = A.take(rows * 128);
    T.perm = (int*)A.take((size_t)B * Q + 4);
    T.sortws = (int*)A.take(query_sort_ws_ints(B, Q) + 4);
    T.gxy = A.take((size_t)B * Q * 2 + 4);
    for (int l = 0; l < 3; ++l) {
        T.QKV[l] = l < 2 ? A.take(rows * 384) : nullptr;   // (the last layer runs in the absorbed token-0 form: no Q | K | V tensor)
        T.O[l] = A.take(rows * 128);
        T.u1[l] = A.take(rows * 128);
        T.x1[l] = A.take(rows * 128);
        if (l < 2) {
            T.u2[l] = A.take(rows * 128);
            T.x2[l] = A.take(rows * 128);
        } else {
            T.u2[l] = T.x2[l] = nullptr;
        }
        T.w_inT[l] = frag_alloc(A, 128, 384);
        T.w_outT[l] = frag_alloc(A, 128, 128);
        T.w_1T[l] = frag_alloc(A, 128, 2048);
        T.w_2T[l] = frag_alloc(A, 2048, 128);
        T.w_inN[l] = frag_alloc(A, 384, 128);
        T.w_outN[l] = frag_alloc(A, 128, 128);
        T.w_1N[l] = frag_alloc(A, 2048, 128);
        T.wT16[l] = A.take((size_t)S3D_FFN_NCHUNK * 8192);
        T.wrec1[l] = A.take(S3D_FFN_REC_IMG_FLOATS);
        T.wrec2t[l] = A.take(S3D_FFN_REC_IMG_FLOATS);
        T.fmask[l] = (unsigned*)A.take(ffn_mask_dwords(l < 2 ? rows : rows0));
    }
    T.w_absM = frag_alloc(A, 512, 128); T.w_absMT = frag_alloc(A, 128, 512);
    T.w_absN = frag_alloc(A, 128, S3D_ABS_NA); T.w_absNT = frag_alloc(A, S3D_ABS_NA, 128);
    T.absM = A.take(512 * 128); T.absm = A.take(512); T.absN = A.take(128 * S3D_ABS_NA);
    T.qt = A.take(rows0 * 512); T.dqt = A.take(rows0 * 512);
    T.xbar = A.take(rows0 * S3D_ABS_NA); T.dxbar = A.take(rows0 * S3D_ABS_NA);
    T.dMb = A.take(512 * 128); T.dmb = A.take(512); T.dNb = A.take(128 * S3D_ABS_NA);
    T.x1c = A.take(rows0 * 128); T.u2c = A.take(rows0 * 128); T.x2c = A.take(rows0 * 128);
    T.dA = A.take(rows * 128); T.dB = A.take(rows * 128); T.dO = A.take(rows * 128);
    T.dQKV = A.take(rows * 384);
    T.dmask = A.take(rows * 128);
    // operand images of the FFN weight gradients (decode.h): of dY (written by the backward data pass, shared by the
    // layers) and of every layer's input x (written by its forward, kept until its backward)
    for (int k = 0; k < 2; ++k) T.recimg[k] = A.take(ffn_rec_image_floats((long)rows));
    for (int l = 0; l < 3; ++l)
        for (int k = 0; k < 2; ++k) T.ximg[l][k] = A.take(ffn_rec_image_floats((long)(l < 2 ? rows : rows0)));
    T.dc1 = A.take(rows0 * 128); T.dc2 = A.take(rows0 * 128);
    T.tmp128 = A.take(rows0 * 128);
    T.ff_rb = rows < 65536 ? (long)rows : 65536;
    T.ffA = A.take((size_t)T.ff_rb * 2048); T.ffD = A.take((size_t)T.ff_rb * 2048);
    T.dsdf = A.take((size_t)B * Q + 64); T.sdf = A.take((size_t)B * Q + 64);
}

static void plan_shared(Arena& A, TrainBufs& T) {
    T.partial_floats = (size_t)64 << 20;
    T.partial = A.take(T.partial_floats);
    T.cpartial = A.take((size_t)2 * CS_CHUNKS_MAX * 2048 + 4096);
    T.vec = A.take(8192);
    T.fwd_losses = T.vec ? T.vec + 8000 : nullptr;
}

static void plan_train(Arena& A, const StepDims& d, TrainBufs& T) {
    const int B = d.B, S = d.S, ns = d.ns, Nd = d.Nd;
    plan_enc(A, d, B, T);
    for (int l = 0; l < 5; ++l) {
        const size_t r = (size_t)d.r5 << l;
        T.F[l] = A.take((size_t)Nd * r * r * kLatC[l]);
        T.dF[l] = A.take((size_t)Nd * r * r * kLatC[l]);
    }
    T.w_transc = frag_alloc(A, 512, 640);
    T.w_transc_d = frag_alloc(A, 512, 512);
    for (int i = 0; i < 4; ++i) {
        const int C = kUpC[i], Ct = C / 2;
        const size_t ro = (size_t)d.r5 << (i + 1);
        T.proj[i] = A.take((size_t)B * ro * ro * Ct);
        T.up[i] = A.take((size_t)Nd * ro * ro * Ct);
        T.z1[i] = A.take((size_t)Nd * ro * ro * Ct);
        T.mid[i] = A.take((size_t)Nd * ro * ro * Ct);
        T.z2[i] = A.take((size_t)Nd * ro * ro * Ct);
        T.m1[i] = A.take(Ct); T.r1[i] = A.take(Ct); T.m2[i] = A.take(Ct); T.r2[i] = A.take(Ct);
        T.w_tup[i] = frag_alloc(A, Ct, C);
        T.w_tup_d[i] = frag_alloc(A, C, Ct);
        T.w_upt[i] = frag_alloc(A, 4 * Ct, C);
        T.w_upt_d[i] = frag_alloc(A, C, 4 * Ct);
        T.w_c1[i] = frag_alloc(A, Ct, 2 * 9 * Ct);
        T.w_c1_dp[i] = frag_alloc(A, Ct, 9 * Ct);
        T.w_c1_du[i] = frag_alloc(A, Ct, 9 * Ct);
        T.w_c2[i] = frag_alloc(A, Ct, 9 * Ct);
        T.w_c2_d[i] = frag_alloc(A, Ct, 9 * Ct);
        T.upt_shift[i] = A.take(4 * Ct);
    }
    T.w_outc = frag_alloc(A, 3, 32);
    T.w_outc_d = frag_alloc(A, 32, 16);
    T.outc_shift = A.take(16);
    T.rec = A.take((size_t)Nd * 3 * S * S);
    T.drec = A.take((size_t)Nd * 3 * S * S);
    const size_t big = (size_t)Nd * S * S * 32;
    T.scrA = A.take(big); T.scrB = A.take(big); T.scrC = A.take(big); T.scrD = A.take(big);
    // VGG
    const size_t vpx = (size_t)2 * Nd * S * S;
    T.vin16 = A.take(vpx * 16);
    int pi = 0;
    for (int i = 0; i < 14; ++i) {
        const size_t pr = vpx >> (2 * kVggRes[i]);
        T.va[i] = A.take(pr * kVggCout[i]);
        if (kVggPoolAfter[i]) T.vp[pi++] = A.take(pr / 4 * kVggCout[i]);
        T.w_vgg[i] = frag_alloc(A, kVggCout[i], 9 * pad16(kVggCin[i]));
        T.w_vgg_d[i] = frag_alloc(A, pad16(kVggCin[i]), 9 * kVggCout[i]);
    }
    T.w_vggZ = frag_alloc(A, 27, 64);
    T.vgA = A.take(vpx / 2 * 64); T.vgB = A.take(vpx / 2 * 64);
    // decoder
    const size_t rows = (size_t)d.rows, rows0 = (size_t)d.rows0;
    T.head_packed = A.take(head_layout().total);
    for (int l = 0; l < 3; ++l) {
        const size_t r = (size_t)d.r5 << l;
        T.lat_proj[l] = A.take((size_t)Nd * r * r * 128);
        T.dlat_proj[l] = A.take((size_t)Nd * r * r * 128);
        T.w_projT[l] = frag_alloc(A, kLatC[l], 128);
    }
    T.ws34_t = A.take(96 * 128);
    T.ws34_t16 = A.take(96 * 128);
    T.raw34 = A.take(rows * 96);
    T.qrot4 = A.take(rows0 * 4);
    plan_dec(A, d, T);
    {
        const size_t n = sample_bwd_partial_floats(S, B, ns);
        T.sb_partial = n ? A.take(n) : nullptr;
    }
    plan_shared(A, T);
}

extern "C" size_t s3d_train_workspace_bytes(int batch, int size, long n_qry, int n_slices) {
    Arena A{nullptr, 0};
    TrainBufs T;
    plan_train(A, step_dims(batch, size, n_qry, n_slices), T);
    return A.off * sizeof(float);
}

// ------------------------------------------------------------------------------------------------
struct TrainRun {
    hipStream_t st;
    TrainBufs& T;
    int prec;
    const BnSync* sync = nullptr;   // cross-rank BatchNorm statistics (S3dTrainBatch.sync_bn)
    bool conv_single = false;       // S3D_PREC_F16 step: the conv engine's forward / data-gradient passes run one f16 MFMA per product

    ConvLaunch mk(const FragW& w, int N, int H, int W, int ks, const float* shift, int act) const {
        ConvLaunch c = {};
        c.N = N; c.H = H; c.W = W; c.ks = ks;
        c.CoutPad = w.n_pad; c.wpk = w.p; c.KU = w.KU;
        c.wpk16 = prec == S3D_PREC_F16X3 ? (const void*)w.p16 : nullptr;   // launch_conv falls back per layer
        c.single_pass = conv_single && c.wpk16;
        c.scale = nullptr; c.shift = shift; c.act = act;
        c.out_mode = S3D_OUT_NHWC; c.cout_store = w.n_pad; c.out_cstride = w.n_pad;
        return c;
    }
    int pack_conv(const FragW& f, const float* w, int cout, int cin_tot, int cin_begin, int cseg, int u_off,
                  int taps) const {
        TRY_RET(pack_conv3(w, f.p, cout, f.n_pad, cin_tot, cin_begin, cseg, f.KU, u_off, taps, st));
        if (prec == S3D_PREC_F16X3 && pad16(cseg) % 32 == 0 && f.KU % 2 == 0 && u_off % 2 == 0)
            TRY_RET(pack_conv3(w, f.p16, cout, f.n_pad, cin_tot, cin_begin, cseg, f.KU, u_off, taps, st, 1));
        return 0;
    }
    // data-gradient pack: rows = input channels [cin_begin, cin_begin + cseg), K = taps * cout
    int pack_dgrad(const FragW& f, const float* w, int cout, int cin_tot, int cin_begin, int cseg, int taps) const {
        PackArgs a = {};
        a.src = w; a.dst = f.p; a.kind = S3D_PACK_CONV_DGRAD;
        a.n_valid = cseg; a.n_pad = f.n_pad;
        a.KU_total = f.KU; a.u_off = 0; a.ku_seg = f.KU;
        a.cseg = pad16(cout); a.cseg_valid = cout; a.cin_tot = cin_tot; a.cin_begin = cin_begin; a.taps = taps;
        TRY_RET(launch_pack(a, st));
        if (prec == S3D_PREC_F16X3 && a.cseg % 32 == 0 && f.KU % 2 == 0) {
            a.f16 = 1; a.dst = f.p16;
            TRY_RET(launch_pack(a, st));
        }
        return 0;
    }
    int pack_lin_t(const FragW& f, const float* w, int n, int k, int ld) const {
        PackArgs a = {};
        a.src = w; a.dst = f.p; a.kind = S3D_PACK_LINEAR_T;
        a.n_valid = n; a.n_pad = f.n_pad; a.KU_total = f.KU; a.u_off = 0; a.ku_seg = f.KU;
        a.ld = ld; a.k_valid = k;
        TRY_RET(launch_pack(a, st));
        if (prec == S3D_PREC_F16X3 && f.KU % 2 == 0 && f.p16) {
            a.f16 = 1; a.dst = f.p16;
            TRY_RET(launch_pack(a, st));
        }
        return 0;
    }
    int pack_lin(const FragW& f, const float* w, int n, int k, int ld) const {
        TRY_RET(pack_linear(w, f.p, n, f.n_pad, k, ld, 0, st));
        if (prec == S3D_PREC_F16X3 && f.KU % 2 == 0) TRY_RET(pack_linear(w, f.p16, n, f.n_pad, k, ld, 0, st, 1));
        return 0;
    }
    WgradArgs wg(const float* dy, int dy_cstride, int N, ConvSrc x, int Cx, int Nimg, int H, int W, int ks) const {
        WgradArgs a = {};
        a.dy = dy; a.dy_cstride = dy_cstride; a.dy_coff = 0; a.N = N;
        a.x = x; a.x_coff = 0; a.Cx = Cx;
        a.Nimg = Nimg; a.H = H; a.W = W; a.ks = ks;
        a.partial = T.partial; a.partial_floats = T.partial_floats;
        a.bias_partial = T.cpartial;
        a.prec = prec;
        return a;
    }
    // the same for row matrices: dy (rows, n), x (rows, k)
    WgradArgs wg_rows(const float* dy, int n, const float* x, int k, long rows) const {
        return wg(dy, n, n, plain_src(x, k), k, 1, 1, (int)rows, 1);
    }
    // out (N,H,W, w's padded channels) = act(conv_ks(x (N,H,W,cx)) + shift), one plain NHWC source; accumulate: out +=
    int conv(const FragW& w, int N, int H, int W, int ks, const float* x, int cx, float* out, const float* shift = nullptr,
             int act = S3D_ACT_NONE, int accumulate = 0) const {
        ConvLaunch c = mk(w, N, H, W, ks, shift, act);
        c.nsrc = 1;
        c.src[0] = plain_src(x, cx);
        c.out = out;
        c.out_accumulate = accumulate;
        return launch_conv(c, st);
    }
    // weight gradient into a linear layer's [n][ld] layout (bias_out: its bias gradient, the column sums of dy) ...
    int wgrad_lin(WgradArgs w, const void* out, int ld, const void* bias_out = nullptr, int single = 0) const {
        w.out = (float*)out; w.out_kind = S3D_PACK_LINEAR; w.ld = ld;
        w.bias_out = (float*)bias_out;
        w.single = single;
        return launch_wgrad(w, st);
    }
    // ... and into input channels [cin_begin, cin_begin + w.Cx) of a convolution's [n][cin_tot][taps] layout
    int wgrad_conv(WgradArgs w, const void* out, int cin_tot, int cin_begin) const {
        w.out = (float*)out; w.out_kind = S3D_PACK_CONV; w.cin_tot = cin_tot; w.cin_begin = cin_begin;
        return launch_wgrad(w, st);
    }
    // weight gradient of a layer with 3 inputs (fc_p, pts_feat_extractor.0): x4 holds its input rows padded to 4, the [n][4]
    // result goes through T.vec to the [n][3] parameter layout
    int wgrad_xyz(const float* dy, int n, const float* x4, long rows, const void* out) const {
        TRY_RET(wgrad_lin(wg_rows(dy, n, x4, 4, rows), T.vec, 4));
        return launch_copy_cols(T.vec, (float*)out, n, 4, 3, st);
    }
    int zero(float* p, size_t n) const {
        if (hipMemsetAsync(p, 0, n * sizeof(float), st) != hipSuccess) {
            s3d_set_error("train: memset failed");
            return (int)hipErrorUnknown;
        }
        return 0;
    }
    int copy(float* d, const float* s, size_t n) const {
        if (hipMemcpyAsync(d, s, n * sizeof(float), hipMemcpyDeviceToDevice, st) != hipSuccess) {
            s3d_set_error("train: memcpy failed");
            return (int)hipErrorUnknown;
        }
        return 0;
    }
};

// ------------------------------------------------------------------------------------------------
// VGG16-BN encoder (vgg16bn_feats.py:26-57) in training mode on n_img images: batch-statistics BatchNorm with
// running-stat updates, every conv output kept.  The five taps are the RAW conv outputs z[1], z[3], z[6], z[9],
// z[12]; the backward expects their incoming gradients in T.dskip[0..4].
// ------------------------------------------------------------------------------------------------
static int enc_pack(const TrainRun& R, const S3dConvParams* enc) {
    TrainBufs& T = R.T;
    for (int i = 0; i < 13; ++i) {
        TRY_RET(R.pack_conv(T.w_enc[i], enc[i].w, kEncCout[i], kEncCin[i], 0, kEncCin[i], 0, 9));
        TRY_RET(R.pack_dgrad(T.w_enc_d[i], enc[i].w, kEncCout[i], kEncCin[i], 0, kEncCin[i], 9));
    }
    return 0;
}

// bn_last: also run the BatchNorm that follows conv5_3 (its output is unused, but model_gt.py's encoder
// evaluates it, so its running statistics move)
static int enc_forward(const TrainRun& R, const S3dConvParams* enc, const float* img_nchw, int n_img, int S,
                       int bn_last) {
    TrainBufs& T = R.T;
    hipStream_t st = R.st;
    TRY_RET(launch_nchw_to_nhwc(img_nchw, T.in16, n_img, 3, S, S, 16, st));
    for (int i = 0; i < 13; ++i) {
        const int r = S >> kEncRes[i];
        if (i == 0 && S % 4 == 0) {   // 3 -> 64 straight from the image (T.in16 is still the wgrad's operand)
            TRY_RET(launch_conv3x3_first(img_nchw, 3, enc[0].w, enc[0].b, T.z[0], n_img, S, S, st));
        } else {
            TRY_RET(R.conv(T.w_enc[i], n_img, r, r, 3, T.ein[i], pad16(kEncCin[i]), T.z[i], enc[i].b));
        }
        if (i < 12 || (bn_last && enc[i].bn[2]))
            TRY_RET(launch_bn_stats(T.z[i], (long)n_img * r * r, kEncCout[i], T.mean[i], T.rstd[i],
                                    (float*)enc[i].bn[2], (float*)enc[i].bn[3], T.cpartial, st, R.sync));
        if (i < 12)
            TRY_RET(launch_bn_apply(T.z[i], T.mean[i], T.rstd[i], enc[i].bn[0], enc[i].bn[1], T.ein[i + 1], n_img, r,
                                    r, kEncCout[i], kEncTap[i] ? 1 : 0, st));
    }
    return 0;
}

// hook (data-parallel training): once the gradients of convs 7..12 and BatchNorms 7..11 are final — 13 M of the
// encoder's 14.7 M parameters, produced before the expensive shallow layers — they are multiplied by inv_gs (the
// inverse backward scale) and ev_deep is recorded, so their all-reduce can run under the rest of the backward
static void add_enc_grads_range(ScaleTable& t, const S3dConvParams* enc, int lo, int hi);
static int enc_backward(const TrainRun& R, const S3dConvParams* enc, const S3dConvParams* denc, int n_img, int S,
                        hipEvent_t ev_deep = nullptr, float inv_gs = 1.f) {
    TrainBufs& T = R.T;
    hipStream_t st = R.st;
    float* dcur = T.encA;   // gradient w.r.t. z[i] is built in place here
    float* dnext = T.encB;
    TRY_RET(R.copy(dcur, T.dskip[4], ((size_t)n_img * S * S >> 8) * 512));      // d z[12] = d conv5_3
    for (int i = 12; i >= 0; --i) {   // walk convs 12 -> 0
        const int r = S >> kEncRes[i];
        const long P = (long)n_img * r * r;
        // dcur = d z[i]
        TRY_RET(launch_colsum(dcur, P, kEncCout[i], 0, kEncCout[i], (float*)denc[i].b, 0, T.cpartial, st));
        TRY_RET(R.wgrad_conv(R.wg(dcur, kEncCout[i], kEncCout[i], plain_src(T.ein[i], pad16(kEncCin[i])), pad16(kEncCin[i]),
                                  n_img, r, r, 3),
                             denc[i].w, kEncCin[i], 0));
        if (i == 7 && (ev_deep || inv_gs != 1.f)) {
            if (inv_gs != 1.f) {
                ScaleTable tb;
                tb.count = 0;
                add_enc_grads_range(tb, denc, 7, 13);
                TRY_RET(launch_scale_table(tb, inv_gs, st));
            }
            if (ev_deep) (void)hipEventRecord(ev_deep, st);
        }
        if (i == 0) break;
        TRY_RET(R.conv(T.w_enc_d[i], n_img, r, r, 3, dcur, kEncCout[i], dnext));   // d ein[i]  (grid of ein[i])
        // ein[i] = [pool](relu(bn(z[i-1])))  ->  d z[i-1]
        const int j = i - 1, rj = S >> kEncRes[j];
        const float* skip = nullptr;
        if (kEncTap[j]) {   // the raw tap output is also a feature level / skip input: its gradient joins here
            int k = 0;
            while (kTapConv[k] != j) ++k;
            skip = T.dskip[k];
        }
        TRY_RET(launch_bn_bwd(T.z[j], T.mean[j], T.rstd[j], enc[j].bn[0], enc[j].bn[1], dnext, dcur,
                              (float*)denc[j].bn[0], (float*)denc[j].bn[1], n_img, rj, rj, kEncCout[j],
                              kEncTap[j] ? 1 : 0, T.cpartial, st, skip, R.sync));
    }
    return 0;
}

// Adam on many tensors at once (the training step has 98 - 137 parameter tensors: one launch per 128 instead of one
// per tensor).  params / offsets / sizes are HOST arrays of n_tensors entries; tensor i reads its gradient and keeps
// its moments at [offsets[i], offsets[i] + sizes[i]) of the three flat device arrays.
extern "C" int s3d_adam_step_multi(float* const* params, const long* offsets, const long* sizes, int n_tensors,
                                   const float* grad_flat, float* exp_avg_flat, float* exp_avg_sq_flat, float lr,
                                   float beta1, float beta2, float eps, int step, void* stream) {
    S3D_CHECK_ARG(params && offsets && sizes && grad_flat && exp_avg_flat && exp_avg_sq_flat && step >= 1 && n_tensors >= 0,
                  "adam_step_multi: bad argument");
    const float bc1 = 1.f - powf(beta1, (float)step), bc2 = 1.f - powf(beta2, (float)step);
    for (int i0 = 0; i0 < n_tensors; i0 += S3D_ADAM_TABLE_MAX) {
        AdamTable t;
        t.count = n_tensors - i0 < S3D_ADAM_TABLE_MAX ? n_tensors - i0 : S3D_ADAM_TABLE_MAX;
        for (int i = 0; i < t.count; ++i) {
            S3D_CHECK_ARG(params[i0 + i] && sizes[i0 + i] >= 0, "adam_step_multi: tensor %d is null", i0 + i);
            t.p[i] = params[i0 + i];
            t.off[i] = offsets[i0 + i];
            t.n[i] = sizes[i0 + i];
        }
        TRY(launch_adam_table(t, grad_flat, exp_avg_flat, exp_avg_sq_flat, lr, beta1, beta2, eps, bc1, bc2,
                              (hipStream_t)stream));
    }
    return 0;
}

// ------------------------------------------------------------------------------------------------
// Backward scale of the split-precision path.  The f16 hi/lo split carries ~22 bits only while the value's low
// half stays a normal f16 (|v| >~ 0.1); the L1 losses hand out gradients of 1/n per element (2.5e-6 at 100k
// queries, 4e-7 on the slice images), which sit in f16's subnormal range and lose most of their bits.  Every
// loss gradient is therefore created multiplied by a power of two that puts d sdf in [8, 16); the whole backward
// is linear in it, and the parameter gradients are multiplied by the inverse at the end — both exact in fp32.
// ------------------------------------------------------------------------------------------------
static float backward_scale(int prec, long nsdf) {
    if (prec != S3D_PREC_F16X3) return 1.f;
    int k = 0;
    while ((1L << k) < nsdf && k < 40) ++k;
    return ldexpf(1.f, k + 3);
}
static void add_layer_grads(ScaleTable& t, const S3dLayerParams* L) {
    for (int l = 0; l < S3D_N_LAYERS; ++l) {
        t.add(L[l].in_proj_w, 384 * 128); t.add(L[l].in_proj_b, 384);
        t.add(L[l].out_proj_w, 128 * 128); t.add(L[l].out_proj_b, 128);
        t.add(L[l].lin1_w, (long)S3D_FFN * 128); t.add(L[l].lin1_b, S3D_FFN);
        t.add(L[l].lin2_w, (long)S3D_FFN * 128); t.add(L[l].lin2_b, 128);
        t.add(L[l].norm1_w, 128); t.add(L[l].norm1_b, 128);
        t.add(L[l].norm2_w, 128); t.add(L[l].norm2_b, 128);
    }
}
static void add_enc_grads_range(ScaleTable& t, const S3dConvParams* enc, int lo, int hi) {
    for (int i = lo; i < hi; ++i) {
        t.add(enc[i].w, (long)kEncCout[i] * kEncCin[i] * 9);
        t.add(enc[i].b, kEncCout[i]);
        if (i < 12) {
            t.add(enc[i].bn[0], kEncCout[i]);
            t.add(enc[i].bn[1], kEncCout[i]);
        }
    }
}
static void add_enc_grads(ScaleTable& t, const S3dConvParams* enc) { add_enc_grads_range(t, enc, 0, 13); }

extern "C" int s3d_adam_step(float* p, const float* g, float* m, float* v, long n, float lr, float beta1,
                             float beta2, float eps, int step, void* stream) {
    S3D_CHECK_ARG(p && g && m && v && step >= 1, "adam_step: bad argument");
    const float bc1 = 1.f - powf(beta1, (float)step), bc2 = 1.f - powf(beta2, (float)step);
    return launch_adam(p, g, m, v, n, lr, beta1, beta2, eps, bc1, bc2, (hipStream_t)stream);
}

// ------------------------------------------------------------------------------------------------
// Transformer decoder of the regression models (models.py:82-84 / model_gt.py:101-106), training mode:
// forward on a token tensor X0 [G][T][16][128] with activations kept, backward from d sdf to d X0.
// Shared by s3d_train_fwd_bwd and s3d_gt_train_fwd_bwd (different token builders, same decoder).
// ------------------------------------------------------------------------------------------------
struct DecoderTrain {
    TrainRun& R;
    TrainBufs& T;
    hipStream_t st;
    const S3dLayerParams* P;      // att_decoder.layers.{0,1,2}
    const S3dLayerParams* dP;     // their gradients
    const float* fc_out_w;        // fc_out.0.weight (1,128)
    float* d_fc_out_w;
    float* d_fc_out_b;
    const float* packed;          // packed head image holding the layer fragments + fc_out (HeadLayout HL)
    HeadLayout HL;
    int prec;
    float dropout_p;
    unsigned long long seed;
    long G, gpb, Q, rows, rows0;
    int Tn;
    const int* perm;
    bool single = false;          // S3D_PREC_F16 throughput mode: one f16 MFMA per product in the decoder's GEMM kernels

    DropCfg drop(int l, int site) const { return make_drop(seed, dropout_p, 4 * l + site); }

    int pack_layers() const {
        for (int l = 0; l < 3; ++l) {
            TRY_RET(R.pack_lin_t(T.w_inT[l], P[l].in_proj_w, 128, 384, 128));
            TRY_RET(R.pack_lin_t(T.w_outT[l], P[l].out_proj_w, 128, 128, 128));
            TRY_RET(R.pack_lin_t(T.w_1T[l], P[l].lin1_w, 128, 2048, 128));
            TRY_RET(R.pack_lin_t(T.w_2T[l], P[l].lin2_w, 2048, 128, 2048));
            TRY_RET(R.pack_lin(T.w_inN[l], P[l].in_proj_w, 384, 128, 128));
            TRY_RET(R.pack_lin(T.w_outN[l], P[l].out_proj_w, 128, 128, 128));
            TRY_RET(R.pack_lin(T.w_1N[l], P[l].lin1_w, 2048, 128, 128));
            TRY_RET(launch_pack_ffn_f16x3_bwd(P[l].lin1_w, P[l].lin2_w, T.wT16[l], st));
            TRY_RET(launch_pack_ffn_rec_f16x3(P[l].lin1_w, 128, 1, T.wrec1[l], st));
            TRY_RET(launch_pack_ffn_rec_f16x3(P[l].lin2_w, 1, S3D_FFN, T.wrec2t[l], st));
        }
        // last layer: the absorbed matrices of this step's weights (double accumulation) and their fragment images
        TRY_RET(launch_absorb_train(P[2].in_proj_w, P[2].in_proj_b, P[2].out_proj_w, T.absM, T.absm, T.absN, st));
        TRY_RET(R.pack_lin(T.w_absM, T.absM, 512, 128, 128));
        TRY_RET(R.pack_lin_t(T.w_absMT, T.absM, 128, 512, 128));
        TRY_RET(R.pack_lin(T.w_absN, T.absN, 128, S3D_ABS_NA, S3D_ABS_NA));
        TRY_RET(R.pack_lin_t(T.w_absNT, T.absN, S3D_ABS_NA, 128, S3D_ABS_NA));
        return 0;
    }

    // ---- last layer: only its token 0 is consumed (models.py:83).  Absorbed form (train2.hip, attn_mix0_kernel): the token-0
    // rows get qt = M x0 + m, the mixing kernel reads every token once, out = Naug [xbar | sigma] + b_o; no K | V tensor.
    // Buffers of layer 2 are reused compactly: x0c = x1[2] (rows0 x 128, layer input of token 0), u1c = u1[2] ----
    float* l2_x0c() const { return T.x1[2]; }
    float* l2_u1c() const { return T.u1[2]; }
    int last_attn_fwd(const float* xin, const LayerPtrs& lp) const {
        TRY_RET(launch_tok0_copy(const_cast<float*>(xin), l2_x0c(), G, Tn, 0, 128, st));
        TRY_RET(lin(T.w_absM, 512, 128, T.absm, l2_x0c(), rows0, T.qt, nullptr, 0));
        TRY_RET(launch_attn_mix0_fwd(xin, T.qt, T.xbar, G, Tn, drop(2, 0), st));
        const DropCfg d1 = drop(2, 1);
        TRY_RET(lin(T.w_absN, 128, S3D_ABS_NA, lp.outb, T.xbar, rows0, l2_u1c(), l2_x0c(), 0, &d1));
        return launch_ln_fwd(l2_u1c(), lp.ln1g, lp.ln1b, T.x1c, rows0, st);
    }
    // dy = d x1c (rows0 x 128)  ->  parameter gradients of the layer's attention block, d xin (rows x 128) in dx_out
    int last_attn_bwd(const float* xin, const float* dy, float* du, float* dx_out) const {
        const S3dLayerParams& g = dP[2];
        // LayerNorm backward, the output dropout's mask and the bias gradient (column sums of dum) in one pass
        const DropCfg d1b = drop(2, 1);
        const float* dum = dropout_p > 0.f ? T.dmask : du;
        TRY_RET(launch_ln_bwd(l2_u1c(), P[2].norm1_w, dy, du, rows0, (float*)g.norm1_w, (float*)g.norm1_b, 0, T.cpartial,
                              st, &d1b, const_cast<float*>(dum), (float*)g.out_proj_b));
        // d Naug = dum^T [xbar | sigma],  d [xbar | sigma] = dum Naug
        TRY_RET(R.wgrad_lin(R.wg_rows(dum, 128, T.xbar, S3D_ABS_NA, rows0), T.dNb, S3D_ABS_NA, nullptr, single));
        TRY_RET(lin(T.w_absNT, S3D_ABS_NA, 128, nullptr, dum, rows0, T.dxbar, nullptr, 0));
        // the mix backward writes d xin of every token (value path + score path) and d qt
        TRY_RET(launch_attn_mix0_bwd(xin, T.qt, T.dxbar, dx_out, T.dqt, G, Tn, drop(2, 0), st));
        TRY_RET(R.wgrad_lin(R.wg_rows(T.dqt, 512, l2_x0c(), 128, rows0), T.dMb, 128, T.dmb, single));
        // chain rule through the absorbed products: in_proj weight / bias and out_proj weight (every element written)
        TRY_RET(launch_absorb_grad(P[2].in_proj_w, P[2].in_proj_b, P[2].out_proj_w, T.dMb, T.dmb, T.dNb, (float*)g.in_proj_w,
                                   (float*)g.in_proj_b, (float*)g.out_proj_w, st));
        // token-0 rows additionally receive dqt M and the residual
        TRY_RET(lin(T.w_absMT, 128, 512, nullptr, T.dqt, rows0, T.tmp128, du, 0));
        TRY_RET(launch_tok0_copy(dx_out, T.dc2, G, Tn, 0, 128, st));
        TRY_RET(launch_axpy(T.dc2, T.tmp128, 1.f, rows0 * 128, st));
        return launch_tok0_copy(dx_out, T.dc2, G, Tn, 1, 128, st);
    }

    int lin(const FragW& wf, int n, int k, const float* bias, const float* x, long nrows, float* out,
            const float* residual, int accumulate, const DropCfg* dc = nullptr, int act = S3D_ACT_NONE,
            unsigned long long drop_base = 0, const float* gate = nullptr, float gate_scale = 1.f) const {
        const float* p16 = prec == S3D_PREC_F16X3 ? wf.p16 : nullptr;
        ConvLaunch c = proj_desc(wf.p, p16, single && p16, n, k, x, 1, 1, (int)nrows, out, bias, act);
        if (dc) c.drop = *dc;
        c.drop_base = drop_base; c.gate = gate; c.gate_scale = gate_scale;
        c.residual = residual; c.out_accumulate = accumulate;
        return launch_conv(c, st);
    }
    // split-precision training runs the attention block of the full layers as fused query-major kernels
    bool fused_attn(const LayerPtrs& lp) const { return prec == S3D_PREC_F16X3 && lp.aq16 != nullptr && Tn >= 2; }
    int ffn_fwd(int l, const float* x, float* y, float* u, unsigned* mk, long n, const LayerPtrs& lp, const DropCfg& dh,
                const DropCfg& dq) const {
        return prec == S3D_PREC_F16X3 && lp.wf16
                   ? launch_ffn_layer_train_f16x3(x, y, u, mk, n, lp, dh, dq, st, T.ximg[l][0], T.ximg[l][1], single)
                   : launch_ffn_layer_train(x, y, u, n, lp, dh, dq, st);
    }

    // X0 -> sdf (B,Q); activations kept in T
    int forward(const float* X0, float* sdf) const {
        const float* xin = X0;
        for (int l = 0; l < 3; ++l) {
            const LayerPtrs lp = layer_ptrs(packed, HL, l);
            if (l == 2) {   // only token 0 of the last layer is consumed (models.py:83): absorbed attention, FFN on those rows only
                TRY_RET(last_attn_fwd(xin, lp));
                TRY_RET(ffn_fwd(l, T.x1c, T.x2c, T.u2c, T.fmask[l], rows0, lp, drop(l, 2), drop(l, 3)));
                break;
            }
            if (fused_attn(lp)) {
                // the whole block in one kernel, query-major (decode_attnq.hip, TRAIN): Q / K / V and the probabilities stay on
                // chip; kept for the backward: O (out_proj's weight gradient), u1 (LayerNorm backward), x1 (the FFN's input)
                TRY_RET(launch_attn_layer_q_train(xin, T.x1[l], T.u1[l], T.O[l], G, Tn, lp, drop(l, 0), drop(l, 1), st, single));
            } else {
                TRY_RET(lin(T.w_inN[l], 384, 128, lp.inb, xin, rows, T.QKV[l], nullptr, 0));
                TRY_RET(launch_attn_core_fwd(T.QKV[l], T.O[l], G, Tn, drop(l, 0), st));
                const DropCfg d1 = drop(l, 1);
                TRY_RET(lin(T.w_outN[l], 128, 128, lp.outb, T.O[l], rows, T.u1[l], xin, 0, &d1));
                TRY_RET(launch_ln_fwd(T.u1[l], lp.ln1g, lp.ln1b, T.x1[l], rows, st));
            }
            TRY_RET(ffn_fwd(l, T.x1[l], T.x2[l], T.u2[l], T.fmask[l], rows, lp, drop(l, 2), drop(l, 3)));
            xin = T.x2[l];
        }
        return launch_fc_out_fwd(T.x2c, packed + HL.fco_w, packed + HL.fco_b, sdf, rows0, gpb, Q, perm, st);
    }

    // FFN backward on a set of rows:  x (input), u (pre-LN), dy -> dx (written to dx_out)
    int ffn_bwd(int l, const float* x, const float* u, const float* dy, float* du, float* dx_out, long nrows) const {
        const S3dLayerParams& g = dP[l];
        const LayerPtrs lp = layer_ptrs(packed, HL, l);
        // LayerNorm backward + the FFN output dropout's mask + lin2's bias gradient (column sums of dum) in one pass;
        // dum = gradient w.r.t. the (pre-dropout) FFN output
        const DropCfg d3 = drop(l, 3);
        // split-precision path: dum is never stored — the LayerNorm backward forms only its column sums and the FFN data
        // pass rebuilds dum = du * mask from the counter-based masks while it loads du (one store and one load of the
        // 2.66 GB row tensor less per full layer)
        const bool regen = prec == S3D_PREC_F16X3 && dropout_p > 0.f;
        const float* dum = regen ? nullptr : dropout_p > 0.f ? T.dmask : du;
        TRY_RET(launch_ln_bwd(u, P[l].norm2_w, dy, du, nrows, (float*)g.norm2_w, (float*)g.norm2_b, 0, T.cpartial, st, &d3,
                              const_cast<float*>(dum), (float*)g.lin2_b));
        if (prec == S3D_PREC_F16X3) {
            // split-precision path: nothing 2048 wide touches memory.  dx from the activity bits of the forward
            // pass; both weight gradients recompute their wide operand tile by tile inside the contraction.
            const DropCfg d2 = drop(l, 2);
            // (the data pass also writes the D^T / R operand images of dY; those of x were written by the layer's forward)
            TRY_RET(launch_ffn_bwd_dx_f16x3(regen ? du : dum, du, T.fmask[l], dx_out, nrows, T.wT16[l], d2.scale, st, T.recimg[0],
                                            T.recimg[1], regen ? &d3 : nullptr, single));
            FfnWgradArgs w2 = {};
            w2.single = single;
            w2.Dimg = T.recimg[0]; w2.Rimg = T.ximg[l][1]; w2.wimg = T.wrec1[l]; w2.bias = lp.b1; w2.mask = T.fmask[l]; w2.scale = d2.scale;
            w2.P = nrows; w2.out = (float*)g.lin2_w; w2.transpose_out = 0; w2.bias_out = nullptr;
            w2.partial = T.partial; w2.partial_floats = T.partial_floats;
            TRY_RET(launch_ffn_wgrad_rec(w2, st));
            FfnWgradArgs w1 = w2;
            w1.Dimg = T.ximg[l][0]; w1.Rimg = T.recimg[1]; w1.wimg = T.wrec2t[l]; w1.bias = nullptr;
            w1.out = (float*)g.lin1_w; w1.transpose_out = 1; w1.bias_out = (float*)g.lin1_b;
            TRY_RET(launch_ffn_wgrad_rec(w1, st));
            return 0;
        }
        for (long r0 = 0; r0 < nrows; r0 += T.ff_rb) {
            const long nb = nrows - r0 < T.ff_rb ? nrows - r0 : T.ff_rb;
            const float* xb = x + r0 * 128;
            const float* dub = dum + r0 * 128;
            // h = dropout(relu(x W1^T + b1));  da = (du W2) * mask * (a > 0)  [h > 0  <=>  a > 0 and kept]
            const DropCfg d2 = drop(l, 2);
            TRY_RET(lin(T.w_1N[l], 2048, 128, lp.b1, xb, nb, T.ffA, nullptr, 0, &d2, S3D_ACT_RELU,
                    (unsigned long long)r0 * 2048));
            TRY_RET(lin(T.w_2T[l], 2048, 128, nullptr, dub, nb, T.ffD, nullptr, 0, nullptr, S3D_ACT_NONE, 0, T.ffA,
                    d2.scale));
            const int acc = r0 > 0;
            WgradArgs w2 = R.wg_rows(dub, 128, T.ffA, 2048, nb);
            w2.accumulate = acc;
            TRY_RET(R.wgrad_lin(w2, g.lin2_w, 2048));
            WgradArgs w1 = R.wg_rows(T.ffD, 2048, xb, 128, nb);
            w1.accumulate = acc;
            TRY_RET(R.wgrad_lin(w1, g.lin1_w, 128));
            TRY_RET(launch_colsum(T.ffD, nb, 2048, 0, 2048, (float*)g.lin1_b, acc, T.cpartial, st));
            TRY_RET(lin(T.w_1T[l], 128, 2048, nullptr, T.ffD, nb, dx_out + r0 * 128, du + r0 * 128, 0));  // dx = da W1 + du
        }
        return 0;
    }
    // attention backward:  xin, QKV, O, u1, dy(d x1) -> d xin (written to dx_out)
    int attn_bwd(int l, const float* xi, const float* dy, float* du, float* dx_out) const {
        const S3dLayerParams& g = dP[l];
        // dum = gradient w.r.t. the (pre-dropout) out_proj output; its column sums = out_proj's bias gradient
        const DropCfg d1b = drop(l, 1);
        const float* dum = dropout_p > 0.f ? T.dmask : du;
        TRY_RET(launch_ln_bwd(T.u1[l], P[l].norm1_w, dy, du, rows, (float*)g.norm1_w, (float*)g.norm1_b, 0, T.cpartial, st,
                              &d1b, const_cast<float*>(dum), (float*)g.out_proj_b));
        TRY_RET(R.wgrad_lin(R.wg_rows(dum, 128, T.O[l], 128, rows), g.out_proj_w, 128, nullptr, single));
        TRY_RET(lin(T.w_outT[l], 128, 128, nullptr, dum, rows, T.dO, nullptr, 0));             // dO = du Wo
        const LayerPtrs lpl = layer_ptrs(packed, HL, l);
        if (fused_attn(lpl))   // the forward kept no Q / K / V: the core backward recomputes them on chip (train_attnq.hip)
            TRY_RET(launch_attn_bwd_q(xi, T.dO, T.dQKV, G, Tn, lpl, drop(l, 0), st, single));
        else
            TRY_RET(launch_attn_core_bwd(T.QKV[l], T.dO, T.dQKV, G, Tn, drop(l, 0), st));
        // (in_proj's bias gradient = the column sums of dQKV, added up while the kernel converts its rows)
        TRY_RET(R.wgrad_lin(R.wg_rows(T.dQKV, 384, xi, 128, rows), g.in_proj_w, 128, g.in_proj_b, single));
        TRY_RET(lin(T.w_inT[l], 128, 384, nullptr, T.dQKV, rows, dx_out, du, 0));              // dx = dQKV Win + du
        return 0;
    }

    // d sdf (B,Q) -> gradients of the layer / fc_out parameters, d X0 left in T.dA
    int backward(const float* X0, const float* dsdf, long nsdf) const {
        TRY_RET(launch_fc_out_bwd(T.x2c, fc_out_w, dsdf, T.dc1, T.tmp128, rows0, gpb, Q, perm, st));
        TRY_RET(launch_colsum(T.tmp128, rows0, 128, 0, 128, d_fc_out_w, 0, T.cpartial, st));
        TRY_RET(launch_scalar_reduce(dsdf, nullptr, nsdf, 0, 1.f, d_fc_out_b, 0, T.cpartial, st));
        // layer 2: FFN on the compact token-0 rows, then scatter its input gradient into a zeroed full tensor
        TRY_RET(ffn_bwd(2, T.x1c, T.u2c, T.dc1, T.dc2, T.dB, rows0));            // dB[0 .. rows0) <- d x1c
        TRY_RET(last_attn_bwd(T.x2[1], T.dB, T.dB + rows0 * 128, T.dA));         // dA <- d x2[1]
        for (int l = 1; l >= 0; --l) {
            // d x1[l] goes straight back into dA: the layer's dy is dead once its LayerNorm backward has produced du
            TRY_RET(ffn_bwd(l, T.x1[l], T.u2[l], T.dA, T.dB, T.dA, rows));       // dA <- d x1[l]
            TRY_RET(attn_bwd(l, l == 0 ? X0 : T.x2[l - 1], T.dA, T.dB, T.dA)); // dA <- d xin
        }
        return 0;
    }
};

// ------------------------------------------------------------------------------------------------
// What every training entry point does before its first launch: argument checks, the derived sizes, the workspace plan
// (X: the GT model's extra buffers, NULL for the Reg model) and the workspace-size check.  `who` prefixes the message.
// ------------------------------------------------------------------------------------------------
struct GtTrainBufs;
static void plan_train_gt(Arena& A, const StepDims& d, TrainBufs& T, GtTrainBufs& X);   // api_train_gt.inc
static int open_step(const char* who, bool pointers_ok, int B, int S, long Q, int ns, float dropout_p, int prec,
                     bool prec_ok, void* workspace, size_t workspace_bytes, StepDims& d, TrainBufs& T, GtTrainBufs* X) {
    S3D_CHECK_ARG(pointers_ok && workspace, "%s: null argument", who);
    S3D_CHECK_ARG(B >= 1 && S >= 16 && S % 16 == 0 && Q >= 1 && ns >= 1 && ns <= 12, "%s: bad dims", who);
    S3D_CHECK_ARG(dropout_p >= 0.f && dropout_p < 1.f, "%s: dropout %g out of range", who, (double)dropout_p);
    S3D_CHECK_ARG(prec_ok, "%s: precision mode %d", who, prec);
    d = step_dims(B, S, Q, ns);
    Arena A{(float*)workspace, 0};
    if (X) plan_train_gt(A, d, T, *X);
    else plan_train(A, d, T);
    if (workspace_bytes < A.off * sizeof(float)) {
        s3d_set_error("%s: workspace %zu < %zu bytes", who, workspace_bytes, A.off * sizeof(float));
        return S3D_E_WORKSPACE;
    }
    return 0;
}

// What the two training steps share once they are open: sizes and workspace, the conv / GEMM launcher, the locality order of
// the queries, the transformer decoder, and the backward scale with its removal from the finished gradients.
struct TrainStep {
    const S3dTrainBatch* batch;
    const StepDims d;
    TrainBufs& T;
    hipStream_t st;
    // S3D_PREC_F16 (round 6): a THROUGHPUT mode of the step — the decoder's GEMMs (the four FFN kernels, the fused attention
    // forward / backward, the row-linear layers and their weight gradients: ~75 % of the step's time) run ONE f16 MFMA per
    // product instead of three; everything else (U-Net, VGG, sampling, all reductions, fp32 master weights, fp32 accumulation,
    // the power-of-two backward scale) is the S3D_PREC_F16X3 path.  Not fp32-class: reported beside the headline, never instead.
    const bool dec_single;
    TrainRun R;
    const int* perm;   // token rows follow the image-space locality order of the queries (sampler gathers / scatter-adds stay local)
    DecoderTrain D;
    float gs;          // every loss gradient carries gs (backward_scale); rescale() removes it from the parameter gradients

    TrainStep(const S3dTrainBatch* batch_, const StepDims& d_, TrainBufs& T_, void* stream, int prec, float dropout_p,
              unsigned long long seed, const S3dLayerParams* P, const S3dLayerParams* dP, const float* fc_out_w,
              const float* d_fc_out_w, const float* d_fc_out_b, const HeadLayout& HL)
        : batch(batch_), d(d_), T(T_), st((hipStream_t)stream), dec_single(prec == S3D_PREC_F16),
          R{st, T, dec_single ? S3D_PREC_F16X3 : prec, batch_->sync_bn},
          perm(d.Q >= S3D_SORT_MIN_QUERIES ? T.perm : nullptr),
          D{R, T, st, P, dP, fc_out_w, (float*)d_fc_out_w, (float*)d_fc_out_b, T.head_packed, HL, R.prec, dropout_p, seed,
            d.G, d.gpb, d.Q, d.rows, d.rows0, d.Tn, perm, dec_single},
          gs(backward_scale(R.prec, d.nsdf)) {
        if (dec_single) if (const char* e = getenv("S3D_TRAIN_F16_CONV")) R.conv_single = atoi(e) != 0;
    }
    int sort_queries() const {
        return perm ? launch_query_sort(batch->qry, batch->rot, batch->trans, 0, d.B, d.Q, T.perm, T.sortws, st) : 0;
    }
    // the sampler backward's arguments that do not depend on the model
    SampleBwdArgs sample_bwd_args(const float* dX) const {
        SampleBwdArgs sb = {};
        sb.dX = dX;
        sb.qry = batch->qry; sb.rot = batch->rot; sb.trans = batch->trans;
        sb.flip_yz = 0; sb.size = d.S; sb.n_slices = d.ns;
        sb.n_qry = d.Q; sb.groups_per_batch = d.gpb; sb.groups = d.G;
        sb.perm = perm; sb.bin_ends = perm ? T.sortws : nullptr;
        sb.gxy = perm ? T.gxy : nullptr;
        return sb;
    }
    int rescale(const ScaleTable& tb) const { return launch_scale_table(tb, 1.f / gs, st); }
};

// caller-supplied output gradients of s3d_train_bwd
struct TrainExt {
    const float* d_sdf;   // d loss / d sdf_pred (B,Q), or NULL (zero)
    const float* d_rec;   // d loss / d slices_rec (B*ns,3,S,S), or NULL
    float d_vgg;          // d loss / d vgg_loss
    float grad_scale;     // power-of-two backward scale of the split-precision path; 0 = automatic (2^k ~ 8 * B*Q)
};

// The Reg model's step, one method per phase (the roctx ranges carry the same names), so that a host can also drive it the way
// autograd does: s3d_train_fwd_bwd = weight packs, the forwards, the reference's losses, the backwards; s3d_train_fwd = packs,
// forwards and the value of vgg_loss, every activation kept in the workspace; s3d_train_bwd = the backwards from caller-supplied
// output gradients (TrainExt) on the workspace the forward left behind.
struct RegStep : TrainStep {
    const S3dUNetParams *U, *dU;   // dU, dH: NULL in a forward-only step
    const S3dHeadParams *Hd, *dH;
    const S3dVggParams* V;
    float *sdf, *rec;              // the step's outputs: the caller's buffers, or the workspace's
    RangeSeq range;                // roctx: one range per phase of the step

    RegStep(const S3dUNetParams* U_, const S3dHeadParams* Hd_, const S3dVggParams* V_, const S3dUNetParams* dU_,
            const S3dHeadParams* dH_, const S3dTrainBatch* batch_, const StepDims& d_, TrainBufs& T_, float dropout_p,
            unsigned long long seed, int prec, float* sdf_pred_out, float* slices_rec_out, void* stream)
        : TrainStep(batch_, d_, T_, stream, prec, dropout_p, seed, Hd_->layer, dH_ ? dH_->layer : nullptr, Hd_->fc_out_w,
                    dH_ ? dH_->fc_out_w : nullptr, dH_ ? dH_->fc_out_b : nullptr, head_layout()),
          U(U_), dU(dU_), Hd(Hd_), dH(dH_), V(V_), sdf(sdf_pred_out ? sdf_pred_out : T_.sdf),
          rec(slices_rec_out ? slices_rec_out : T_.rec) {}

    // ---- 1. weight packs (forward + data-gradient forms) ----
    int pack_weights() {
        range.next("s3d:train:weight_packs");
        const int prec = R.prec;
        PackBatchScope packs;   // the ~270 weight repacks of a step go out as table launches at packs.flush()
        TRY_RET(enc_pack(R, U->enc));
        TRY_RET(R.pack_lin(T.w_transc, U->trans_c.w, 512, 640, 640));
        TRY_RET(R.pack_dgrad(T.w_transc_d, U->trans_c.w, 512, 640, 0, 512, 1));
        for (int i = 0; i < 4; ++i) {
            const int C = kUpC[i], Ct = C / 2;
            TRY_RET(R.pack_lin(T.w_tup[i], U->trans_up[i].w, Ct, C, C));
            TRY_RET(R.pack_dgrad(T.w_tup_d[i], U->trans_up[i].w, Ct, C, 0, C, 1));
            PackArgs a = {};
            a.src = U->up_t[i].w; a.dst = T.w_upt[i].p; a.kind = S3D_PACK_CONVT;
            a.n_valid = 4 * Ct; a.n_pad = 4 * Ct; a.KU_total = C / 16; a.ku_seg = C / 16; a.k_valid = C; a.ct = Ct;
            TRY_RET(launch_pack(a, st));
            if (prec == S3D_PREC_F16X3) {
                a.f16 = 1; a.dst = T.w_upt[i].p16;
                TRY_RET(launch_pack(a, st));
            }
            PackArgs g = {};
            g.src = U->up_t[i].w; g.dst = T.w_upt_d[i].p; g.kind = S3D_PACK_CONVT_DGRAD;
            g.n_valid = C; g.n_pad = C; g.KU_total = 4 * Ct / 16; g.ku_seg = 4 * Ct / 16; g.ct = Ct;
            TRY_RET(launch_pack(g, st));
            if (prec == S3D_PREC_F16X3) {
                g.f16 = 1; g.dst = T.w_upt_d[i].p16;
                TRY_RET(launch_pack(g, st));
            }
            TRY_RET(launch_fold_bn(U->up_t[i].b, nullptr, T.vec, T.upt_shift[i], Ct, 4 * Ct, 4, 0, st));
            TRY_RET(R.pack_conv(T.w_c1[i], U->up_c1[i].w, Ct, C, 0, Ct, 0, 9));
            TRY_RET(R.pack_conv(T.w_c1[i], U->up_c1[i].w, Ct, C, Ct, Ct, 9 * Ct / 16, 9));
            TRY_RET(R.pack_dgrad(T.w_c1_dp[i], U->up_c1[i].w, Ct, C, 0, Ct, 9));
            TRY_RET(R.pack_dgrad(T.w_c1_du[i], U->up_c1[i].w, Ct, C, Ct, Ct, 9));
            TRY_RET(R.pack_conv(T.w_c2[i], U->up_c2[i].w, Ct, Ct, 0, Ct, 0, 9));
            TRY_RET(R.pack_dgrad(T.w_c2_d[i], U->up_c2[i].w, Ct, Ct, 0, Ct, 9));
        }
        TRY_RET(R.pack_lin(T.w_outc, U->outc.w, 3, 32, 32));
        TRY_RET(R.pack_dgrad(T.w_outc_d, U->outc.w, 3, 32, 0, 32, 1));
        TRY_RET(launch_fold_bn(U->outc.b, nullptr, T.vec, T.outc_shift, 3, 16, 1, 0, st));
        for (int i = 0; i < 14; ++i) {
            TRY_RET(R.pack_conv(T.w_vgg[i], V->conv[i].w, kVggCout[i], kVggCin[i], 0, kVggCin[i], 0, 9));
            TRY_RET(R.pack_dgrad(T.w_vgg_d[i], V->conv[i].w, kVggCout[i], kVggCin[i], 0, kVggCin[i], 9));
        }
        TRY_RET(R.pack_lin_t(T.w_vggZ, V->conv[0].w, 27, 64, 27));   // elem(n = ci*9 + tap, k = co) = w[co*27 + n]
        // (no bf16 twins: the trainer never decodes in bf16)
        TRY_RET(head_pack_impl(Hd, T.head_packed, D.HL.total * sizeof(float), st, false));
        for (int l = 0; l < 3; ++l) TRY_RET(R.pack_lin_t(T.w_projT[l], Hd->fc_s_w + kFcsCol[l], kLatC[l], 128, 992));
        {
            FragW f{T.ws34_t, T.ws34_t16, 96, 8};
            TRY_RET(R.pack_lin_t(f, Hd->fc_s_w + 896, 96, 128, 992));
        }
        TRY_RET(D.pack_layers());
        return packs.flush(st);
    }

    // ---- 2. U-Net forward, train-mode BatchNorm (unet_custom.py:40-69) ----
    int unet_forward() {
        range.next("s3d:train:unet_fwd");
        const int B = d.B, S = d.S, ns = d.ns, Nd = d.Nd, r5 = d.r5;
        TRY_RET(enc_forward(R, U->enc, batch->img, B, S, 0));
        {
            ConvLaunch c = R.mk(T.w_transc, Nd, r5, r5, 1, U->trans_c.b, S3D_ACT_NONE);
            c.nsrc = 2;
            c.src[0] = ConvSrc{T.z[12], 512, ns, 0, 0};
            c.src[1] = ConvSrc{U->emds, 128, 1, ns, 1};
            c.out = T.F[0];
            TRY_RET(launch_conv(c, st));
        }
        for (int i = 0; i < 4; ++i) {
            const int C = kUpC[i], Ct = C / 2, rp = r5 << i, ro = rp * 2;
            const long Pd = (long)Nd * ro * ro;
            TRY_RET(R.conv(T.w_tup[i], B, ro, ro, 1, T.z[kTapConv[3 - i]], C, T.proj[i], U->trans_up[i].b));
            {
                ConvLaunch c = R.mk(T.w_upt[i], Nd, rp, rp, 1, T.upt_shift[i], S3D_ACT_NONE);
                c.nsrc = 1;
                c.src[0] = plain_src(T.F[i], C);
                c.out = T.up[i];
                c.out_mode = S3D_OUT_CONVT;
                c.cout_store = Ct;
                TRY_RET(launch_conv(c, st));
            }
            {
                ConvLaunch c = R.mk(T.w_c1[i], Nd, ro, ro, 3, nullptr, S3D_ACT_NONE);
                c.nsrc = 2;
                c.src[0] = ConvSrc{T.proj[i], Ct, ns, 0, 0};
                c.src[1] = plain_src(T.up[i], Ct);
                c.out = T.z1[i];
                TRY_RET(launch_conv(c, st));
            }
            TRY_RET(launch_bn_stats(T.z1[i], Pd, Ct, T.m1[i], T.r1[i], (float*)U->up_c1[i].bn[2], (float*)U->up_c1[i].bn[3],
                                    T.cpartial, st, R.sync));
            TRY_RET(launch_bn_apply(T.z1[i], T.m1[i], T.r1[i], U->up_c1[i].bn[0], U->up_c1[i].bn[1], T.mid[i], Nd, ro, ro, Ct,
                                    0, st));
            TRY_RET(R.conv(T.w_c2[i], Nd, ro, ro, 3, T.mid[i], Ct, T.z2[i]));
            TRY_RET(launch_bn_stats(T.z2[i], Pd, Ct, T.m2[i], T.r2[i], (float*)U->up_c2[i].bn[2], (float*)U->up_c2[i].bn[3],
                                    T.cpartial, st, R.sync));
            TRY_RET(launch_bn_apply(T.z2[i], T.m2[i], T.r2[i], U->up_c2[i].bn[0], U->up_c2[i].bn[1], T.F[i + 1], Nd, ro, ro,
                                    Ct, 0, st));
        }
        ConvLaunch c = R.mk(T.w_outc, Nd, S, S, 1, T.outc_shift, S3D_ACT_TANH);
        c.nsrc = 1;
        c.src[0] = plain_src(T.F[4], 32);
        c.out = rec;
        c.out_mode = S3D_OUT_NCHW;
        c.cout_store = 3;
        return launch_conv(c, st);
    }

    // ---- 3. decoder forward (models.py:53-84), activations kept ----
    int tokens_and_decoder_forward() {
        range.next("s3d:train:sample_and_decoder_fwd");
        const HeadLayout& HL = D.HL;
        for (int l = 0; l < 3; ++l) {   // fp32 in every mode
            const int r = d.r5 << l;
            TRY_RET(launch_conv(proj_desc(T.head_packed + HL.wproj[l], nullptr, false, 128, kLatC[l], T.F[l], d.Nd, r, r,
                                          T.lat_proj[l]),
                                st));
        }
        SampleArgs sa = {};
        for (int l = 0; l < 3; ++l) sa.proj[l] = T.lat_proj[l];
        sa.fine[0] = T.F[3]; sa.fine[1] = T.F[4];
        sa.size = d.S; sa.n_slices = d.ns;
        sa.fcp_w = T.head_packed + HL.fcp_w; sa.fcp_b = T.head_packed + HL.fcp_b;
        sa.fcs_b = T.head_packed + HL.fcs_b; sa.ws34 = T.head_packed + HL.ws34;
        sa.ws34_16 = R.prec == S3D_PREC_F16X3 ? T.head_packed + HL.ws34_16 : nullptr;
        sa.qry = batch->qry; sa.rot = batch->rot; sa.trans = batch->trans; sa.flip_yz = 0;
        sa.n_qry = d.Q; sa.groups_per_batch = d.gpb; sa.g_begin = 0; sa.g_count = d.G;
        sa.nx = 0; sa.box = 1.f; sa.X = T.X0; sa.raw_out = T.raw34;
        TRY_RET(sort_queries());
        sa.perm = perm;
        sa.lane_footprints = !s3d_shared_footprint();
        TRY_RET(launch_sample_tokens(sa, st));
        TRY_RET(launch_qry_rot_rows(batch->qry, batch->rot, 0, d.Q, d.gpb, d.G, perm, T.qrot4, st));
        return D.forward(T.X0, sdf);
    }

    // ---- VGG19 forward on [pred ; target] (vgg_perceptual_loss.py:42-70), activations kept ----
    int vgg_forward() {
        range.next("s3d:train:vgg_fwd");
        const int S = d.S, Nd = d.Nd, N2 = 2 * Nd;
        // conv1_1: in split precision its own kernel straight from the image pairs (K = 27 is one MFMA k-step; conv.hip); the
        // fp32 mode normalises into a 16-channel NHWC image for the generic tile
        const bool vgg_first_fused = R.prec == S3D_PREC_F16X3;
        if (vgg_first_fused)
            TRY_RET(launch_vgg_first_f16x3(rec, batch->img_slices, V->mean, V->std, (const float*)V->conv[0].w,
                                           (const float*)V->conv[0].b, T.va[0], Nd, S, st));
        else
            TRY_RET(launch_vgg_prep(rec, batch->img_slices, V->mean, V->std, T.vin16, Nd, S, st));
        const float* cur = vgg_first_fused ? T.va[0] : T.vin16;
        int curC = vgg_first_fused ? kVggCout[0] : 16, pi = 0;
        for (int i = vgg_first_fused ? 1 : 0; i < 14; ++i) {
            const int r = S >> kVggRes[i];
            TRY_RET(R.conv(T.w_vgg[i], N2, r, r, 3, cur, curC, T.va[i], V->conv[i].b, i == 13 ? S3D_ACT_NONE : S3D_ACT_RELU));
            cur = T.va[i];
            curC = kVggCout[i];
            if (kVggPoolAfter[i]) {
                TRY_RET(launch_bn_relu_pool(cur, nullptr, nullptr, T.vp[pi], N2, r, r, curC, st));
                cur = T.vp[pi++];
            }
        }
        return 0;
    }
    // forward-only step: the value of vgg_loss (models.py:92) added to *acc, no gradients
    int vgg_loss_value(float* acc) {
        for (int i = 13; i >= 0; --i)
            if (kVggTap[i]) {
                const long half = (long)d.Nd * (d.S >> kVggRes[i]) * (d.S >> kVggRes[i]) * kVggCout[i];
                TRY_RET(launch_l1_fwd_bwd(T.va[i], T.va[i] + half, half, 0.001f * kVggW[kVggTap[i] - 1] / (float)half, nullptr,
                                          0, T.cpartial, acc, st));
            }
        return 0;
    }

    // ---- 4. loss gradients: the reference's losses (train.py:29-39,46-47: L1(sdf) + L1(images) + 0.001 * VGG19 perceptual,
    //      the last inside vgg_backward) into losses_out[0..3] with their gradients, or the caller's output gradients ----
    int reference_loss_grads(float* losses_out) {
        range.next("s3d:train:losses_and_vgg_bwd");
        const long nsdf = d.nsdf, nimg = d.nimg;
        TRY_RET(launch_l1_fwd_bwd(sdf, batch->sdf, nsdf, 1.f / (float)nsdf, T.dsdf, 0, T.cpartial, losses_out + 0, st, gs));
        TRY_RET(launch_l1_fwd_bwd(rec, batch->img_slices, nimg, 1.f / (float)nimg, T.drec, 0, T.cpartial, losses_out + 1, st,
                                  gs));
        return launch_scalar_reduce(sdf, batch->sdf, nsdf, 1, 1.f / (float)nsdf, losses_out + 3, 0, T.cpartial, st);
    }
    int external_loss_grads(const TrainExt& ext) {
        range.next("s3d:train:losses_and_vgg_bwd");
        if (ext.grad_scale > 0.f && R.prec == S3D_PREC_F16X3) gs = ext.grad_scale;
        TRY_RET(R.zero(T.dsdf, (size_t)d.nsdf));
        if (ext.d_sdf) TRY_RET(launch_axpy(T.dsdf, ext.d_sdf, gs, d.nsdf, st));
        TRY_RET(R.zero(T.drec, (size_t)d.nimg));
        if (ext.d_rec) TRY_RET(launch_axpy(T.drec, ext.d_rec, gs, d.nimg, st));
        return 0;
    }

    // ---- VGG backward (predicted branch = first Nd images): the taps add vgg_mul times their L1 gradients, and their loss
    //      terms to *loss_acc ----
    int vgg_backward(float* loss_acc, float vgg_mul) {
        const int S = d.S, Nd = d.Nd;
        float* dcur = T.vgA;
        float* dnext = T.vgB;
        for (int i = 13; i >= 0; --i) {
            const int r = S >> kVggRes[i];
            const long half = (long)Nd * r * r * kVggCout[i];
            // The ReLU of layer i (dcur arrives as the gradient w.r.t. its output va[i], leaves as the gradient w.r.t. the conv
            // output) costs no pass of its own: at a loss tap the L1 kernel masks the element it has just completed; elsewhere
            // the producer of dcur did it one iteration ago — the arg-max routing of a pooled layer, or the gate of the data
            // gradient's epilogue (the last layer has no ReLU behind its tap)
            if (kVggTap[i]) {
                const float sc = 0.001f * kVggW[kVggTap[i] - 1] / (float)half;
                TRY_RET(launch_l1_fwd_bwd(T.va[i], T.va[i] + half, half, sc, dcur, i == 13 ? 0 : 1, T.cpartial, loss_acc, st,
                                          gs * vgg_mul, i != 13));
            }
            if (i == 0 && R.prec == S3D_PREC_F16X3) {   // 64 -> 3 channels: a 1x1 product into 27 (channel, tap) planes + a nine-neighbour gather
                TRY_RET(R.conv(T.w_vggZ, Nd, r, r, 1, dcur, kVggCout[0], dnext));
                TRY_RET(launch_vgg_first_bwd(dnext, V->std, T.drec, Nd, S, st));
                break;
            }
            // data gradient of conv i
            ConvLaunch c = R.mk(T.w_vgg_d[i], Nd, r, r, 3, nullptr, S3D_ACT_NONE);
            c.nsrc = 1;
            c.src[0] = plain_src(dcur, kVggCout[i]);
            c.out = dnext;
            const bool mask_below = i > 0 && !kVggTap[i - 1];   // layer i - 1's ReLU is not covered by a tap's L1 kernel
            if (mask_below && !kVggPoolAfter[i - 1]) {
                c.gate = T.va[i - 1];
                c.gate_scale = 1.f;
            }
            TRY_RET(launch_conv(c, st));
            if (i == 0) {
                TRY_RET(launch_vgg_prep_bwd(dnext, V->std, T.drec, Nd, S, st));
            } else if (kVggPoolAfter[i - 1]) {
                // input of conv i was pool(va[i-1]): route to the arg-max positions
                TRY_RET(launch_pool_bwd(T.va[i - 1], dnext, dcur, Nd, 2 * r, 2 * r, kVggCout[i - 1], st, mask_below));
            } else {
                float* t = dcur; dcur = dnext; dnext = t;
            }
        }
        return 0;
    }

    // ---- 5. decoder backward ----
    int decoder_backward() {
        range.next("s3d:train:decoder_bwd");
        return D.backward(T.X0, T.dsdf, d.nsdf);   // d X0 in T.dA
    }

    // ---- sampling backward (dA = d X0), the fc_p / fc_s gradients, and gradient bucket 0 ----
    int sampler_backward_and_head_grads() {
        range.next("s3d:train:sample_bwd_and_head_grads");
        const int Nd = d.Nd, r5 = d.r5;
        for (int l = 0; l < 3; ++l) {
            const size_t r = (size_t)r5 << l;
            TRY_RET(R.zero(T.dlat_proj[l], (size_t)Nd * r * r * 128));
        }
        for (int l = 0; l < 5; ++l) {
            const size_t r = (size_t)r5 << l;
            TRY_RET(R.zero(T.dF[l], (size_t)Nd * r * r * kLatC[l]));
        }
        {
            SampleBwdArgs sb = sample_bwd_args(T.dA);
            for (int l = 0; l < 3; ++l) sb.dproj[l] = T.dlat_proj[l];
            sb.dfine[0] = T.dF[3]; sb.dfine[1] = T.dF[4];
            sb.ws34_t = T.ws34_t;
            sb.ws34_t16 = R.prec == S3D_PREC_F16X3 ? T.ws34_t16 : nullptr;
            sb.partial = perm ? T.sb_partial : nullptr;
            TRY_RET(launch_sample_bwd(sb, st));
        }
        // fc_s / fc_p parameter gradients
        TRY_RET(launch_tok0_copy(T.dA, T.dc1, d.G, d.Tn, 0, 128, st));                          // d token-0 rows
        TRY_RET(launch_colsum(T.dc1, d.rows0, 128, 0, 128, (float*)dH->fc_p_b, 0, T.cpartial, st));
        TRY_RET(R.wgrad_xyz(T.dc1, 128, T.qrot4, d.rows0, dH->fc_p_w));
        // (fc_s's bias gradient: the column sums of all token rows ...
        TRY_RET(R.wgrad_lin(R.wg_rows(T.dA, 128, T.raw34, 96, d.rows), dH->fc_s_w + 896, 992, dH->fc_s_b));
        TRY_RET(launch_axpy((float*)dH->fc_s_b, dH->fc_p_b, -1.f, 128, st));                   // ... slice tokens only)
        // fc_s fold backward: dW_l = dG_l^T f_l ;  dF[l] += dG_l W_l
        for (int l = 0; l < 3; ++l) {
            const int r = r5 << l;
            TRY_RET(R.wgrad_lin(R.wg(T.dlat_proj[l], 128, 128, plain_src(T.F[l], kLatC[l]), kLatC[l], Nd, r, r, 1),
                                dH->fc_s_w + kFcsCol[l], 992));
            TRY_RET(R.conv(T.w_projT[l], Nd, r, r, 1, T.dlat_proj[l], 128, T.dF[l], nullptr, S3D_ACT_NONE, 1));
        }
        // Gradient buckets in the order the backward finishes them (data-parallel training all-reduces a bucket while the
        // rest of the backward runs): each is rescaled by 1/gs as soon as it is final, then its event is recorded.
        // bucket 0: transformer decoder + fc_p / fc_s / fc_out
        ScaleTable tb;
        tb.count = 0;
        tb.add(dH->fc_p_w, 128 * 3); tb.add(dH->fc_p_b, 128);
        tb.add(dH->fc_s_w, 128 * 992); tb.add(dH->fc_s_b, 128);
        add_layer_grads(tb, dH->layer);
        tb.add(dH->fc_out_w, 128); tb.add(dH->fc_out_b, 1);
        TRY_RET(rescale(tb));
        record(0);
        return 0;
    }
    void record(int bucket) const {
        if (batch->ev_grad_ready[bucket]) (void)hipEventRecord((hipEvent_t)batch->ev_grad_ready[bucket], st);
    }

    // ---- 6. U-Net backward ----
    // one up block, F[i+1] -> F[i]: conv c2, conv c1 on cat([proj tiled, up]), trans_up, the transposed conv
    int up_block_backward(int i) {
        const int B = d.B, ns = d.ns, Nd = d.Nd;
        const int C = kUpC[i], Ct = C / 2, rp = d.r5 << i, ro = rp * 2;
        float* g2 = T.scrA;     // dz2
        float* dmid = T.scrB;
        float* g1 = T.scrC;     // dz1
        float* dpt = T.scrD;    // d proj (tiled) / d up
        // F[i+1] = relu(bn2(z2))
        TRY_RET(launch_bn_bwd(T.z2[i], T.m2[i], T.r2[i], U->up_c2[i].bn[0], U->up_c2[i].bn[1], T.dF[i + 1], g2,
                              (float*)dU->up_c2[i].bn[0], (float*)dU->up_c2[i].bn[1], Nd, ro, ro, Ct, 0, T.cpartial, st, nullptr,
                              R.sync));
        TRY_RET(R.wgrad_conv(R.wg(g2, Ct, Ct, plain_src(T.mid[i], Ct), Ct, Nd, ro, ro, 3), dU->up_c2[i].w, Ct, 0));
        TRY_RET(R.conv(T.w_c2_d[i], Nd, ro, ro, 3, g2, Ct, dmid));
        // mid = relu(bn1(z1))
        TRY_RET(launch_bn_bwd(T.z1[i], T.m1[i], T.r1[i], U->up_c1[i].bn[0], U->up_c1[i].bn[1], dmid, g1,
                              (float*)dU->up_c1[i].bn[0], (float*)dU->up_c1[i].bn[1], Nd, ro, ro, Ct, 0, T.cpartial, st, nullptr,
                              R.sync));
        // conv c1 on cat([proj tiled, up])
        TRY_RET(R.wgrad_conv(R.wg(g1, Ct, Ct, ConvSrc{T.proj[i], Ct, ns, 0, 0}, Ct, Nd, ro, ro, 3), dU->up_c1[i].w, C, 0));
        TRY_RET(R.wgrad_conv(R.wg(g1, Ct, Ct, plain_src(T.up[i], Ct), Ct, Nd, ro, ro, 3), dU->up_c1[i].w, C, Ct));
        // d proj (per slice image) -> sum over slices -> trans_up backward
        TRY_RET(R.conv(T.w_c1_dp[i], Nd, ro, ro, 3, g1, Ct, dpt));
        float* dproj = T.encA;   // (B,ro,ro,Ct)
        TRY_RET(launch_slice_sum(dpt, dproj, B, ns, (long)ro * ro * Ct, 0, st));
        TRY_RET(launch_colsum(dproj, (long)B * ro * ro, Ct, 0, Ct, (float*)dU->trans_up[i].b, 0, T.cpartial, st));
        TRY_RET(R.wgrad_lin(R.wg(dproj, Ct, Ct, plain_src(T.z[kTapConv[3 - i]], C), C, B, ro, ro, 1), dU->trans_up[i].w, C));
        TRY_RET(R.conv(T.w_tup_d[i], B, ro, ro, 1, dproj, Ct, T.dskip[3 - i], nullptr, S3D_ACT_NONE, 1));
        // d up
        TRY_RET(R.conv(T.w_c1_du[i], Nd, ro, ro, 3, g1, Ct, dpt));
        // ConvTranspose2d backward: d up (Nd,ro,ro,Ct) -> dF[i] (Nd,rp,rp,C) (+=), dW [C][Ct][2][2], db
        TRY_RET(launch_colsum(dpt, (long)Nd * ro * ro, Ct, 0, Ct, (float*)dU->up_t[i].b, 0, T.cpartial, st));
        ConvSrc dsrc = plain_src(dpt, Ct);
        WgradArgs w = R.wg(T.F[i], C, C, dsrc, Ct, Nd, rp, rp, 2);
        w.stride = 2; w.Hin = ro; w.Win = ro;
        w.out = (float*)dU->up_t[i].w; w.out_kind = S3D_PACK_CONVT; w.ct = Ct;
        TRY_RET(launch_wgrad(w, st));
        ConvLaunch c = R.mk(T.w_upt_d[i], Nd, rp, rp, 2, nullptr, S3D_ACT_NONE);
        c.stride = 2; c.Hin = ro; c.Win = ro;
        c.nsrc = 1;
        c.src[0] = dsrc;
        c.out = T.dF[i];
        c.out_accumulate = 1;
        return launch_conv(c, st);
    }
    // bucket 1: the U-Net's decoder half (trans_c, up1..4, trans_up1..4, outc, slice embeddings)
    int close_unet_decoder_bucket() {
        ScaleTable tb;
        tb.count = 0;
        tb.add(dU->trans_c.w, 512 * 640); tb.add(dU->trans_c.b, 512);
        for (int i = 0; i < 4; ++i) {
            const long C = kUpC[i], Ct = C / 2;
            tb.add(dU->trans_up[i].w, Ct * C); tb.add(dU->trans_up[i].b, Ct);
            tb.add(dU->up_t[i].w, C * Ct * 4); tb.add(dU->up_t[i].b, Ct);
            tb.add(dU->up_c1[i].w, Ct * C * 9); tb.add(dU->up_c1[i].bn[0], Ct); tb.add(dU->up_c1[i].bn[1], Ct);
            tb.add(dU->up_c2[i].w, Ct * Ct * 9); tb.add(dU->up_c2[i].bn[0], Ct); tb.add(dU->up_c2[i].bn[1], Ct);
        }
        tb.add(dU->outc.w, 3 * 32); tb.add(dU->outc.b, 3);
        tb.add(dU->emds, (long)d.ns * 128);
        TRY_RET(rescale(tb));
        record(1);
        return 0;
    }
    int unet_backward() {
        range.next("s3d:train:unet_bwd");
        const int B = d.B, S = d.S, ns = d.ns, Nd = d.Nd, r5 = d.r5;
        {   // OutConv: rec = tanh(W f4 + b)
            float* dz16 = T.scrA;  // (Nd,S,S,16)
            TRY_RET(launch_tanh_bwd(rec, T.drec, dz16, Nd, 3, S, S, 16, st));
            TRY_RET(launch_colsum(dz16, (long)Nd * S * S, 16, 0, 16, T.vec, 0, T.cpartial, st));
            TRY_RET(R.copy((float*)dU->outc.b, T.vec, 3));
            TRY_RET(R.wgrad_lin(R.wg(dz16, 16, 3, plain_src(T.F[4], 32), 32, Nd, S, S, 1), dU->outc.w, 32));
            TRY_RET(R.conv(T.w_outc_d, Nd, S, S, 1, dz16, 16, T.dF[4], nullptr, S3D_ACT_NONE, 1));
        }
        {
            const int skc[5] = {64, 128, 256, 512, 512};
            for (int k = 0; k < 5; ++k) TRY_RET(R.zero(T.dskip[k], ((size_t)B * S * S >> (2 * k)) * skc[k]));
        }
        for (int i = 3; i >= 0; --i) TRY_RET(up_block_backward(i));
        {   // trans_c backward: F[0] = W_a x5(tiled) + W_b emb + b
            const long P0 = (long)Nd * r5 * r5;
            TRY_RET(launch_colsum(T.dF[0], P0, 512, 0, 512, (float*)dU->trans_c.b, 0, T.cpartial, st));
            TRY_RET(R.wgrad_lin(R.wg(T.dF[0], 512, 512, ConvSrc{T.z[12], 512, ns, 0, 0}, 512, Nd, r5, r5, 1), dU->trans_c.w, 640));
            TRY_RET(R.wgrad_lin(R.wg(T.dF[0], 512, 512, ConvSrc{U->emds, 128, 1, ns, 1}, 128, Nd, r5, r5, 1),
                                dU->trans_c.w + 512, 640));
            // d x5 = sum over slices of W_a^T dF0
            TRY_RET(R.conv(T.w_transc_d, Nd, r5, r5, 1, T.dF[0], 512, T.scrA));
            TRY_RET(launch_slice_sum(T.scrA, T.dskip[4], B, ns, (long)r5 * r5 * 512, 1, st));
            // d emds[s][e] = sum over batch and pixels of (W_b^T dF0)[b*ns+s]: column sums of dF0 per slice, times W_b
            TRY_RET(launch_emb_grad(T.dF[0], U->trans_c.w, (float*)dU->emds, B, ns, r5 * r5, st));
        }
        TRY_RET(close_unet_decoder_bucket());
        // bucket 2 (encoder convs 7..12 + their BatchNorms) is closed inside enc_backward; bucket 3 = the shallow rest
        TRY_RET(enc_backward(R, U->enc, dU->enc, B, S, (hipEvent_t)batch->ev_grad_ready[2], 1.f / gs));
        ScaleTable tb;
        tb.count = 0;
        add_enc_grads_range(tb, dU->enc, 0, 7);
        return rescale(tb);
    }

    int forward() {
        TRY_RET(unet_forward());
        TRY_RET(tokens_and_decoder_forward());
        return vgg_forward();
    }
    int backward() {
        TRY_RET(decoder_backward());
        TRY_RET(sampler_backward_and_head_grads());
        return unet_backward();
    }
};

static int open_reg_step(const char* who, bool pointers_ok, int B, int S, long Q, int ns, float dropout_p, int prec,
                         void* workspace, size_t workspace_bytes, StepDims& d, TrainBufs& T) {
    return open_step(who, pointers_ok, B, S, Q, ns, dropout_p, prec,
                     prec == S3D_PREC_F32 || prec == S3D_PREC_F16X3 || prec == S3D_PREC_F16, workspace, workspace_bytes, d, T,
                     nullptr);
}

extern "C" int s3d_train_fwd_bwd(const S3dUNetParams* U, const S3dHeadParams* Hd, const S3dVggParams* V,
                                 const S3dUNetParams* dU, const S3dHeadParams* dH, const S3dTrainBatch* batch,
                                 int B, int S, long Q, int ns, float dropout_p, unsigned long long seed, int prec,
                                 float* losses_out, float* sdf_pred_out, float* slices_rec_out, void* workspace,
                                 size_t workspace_bytes, void* stream) {
    StepDims d;
    TrainBufs T = {};
    TRY(open_reg_step("train", U && Hd && V && dU && dH && batch && losses_out, B, S, Q, ns, dropout_p, prec, workspace,
                      workspace_bytes, d, T));
    RegStep s(U, Hd, V, dU, dH, batch, d, T, dropout_p, seed, prec, sdf_pred_out, slices_rec_out, stream);
    TRY(s.R.zero(losses_out, 4));
    TRY(s.pack_weights());
    TRY(s.forward());
    TRY(s.reference_loss_grads(losses_out));
    TRY(s.vgg_backward(losses_out + 2, 1.f));
    return s.backward();
}

extern "C" int s3d_train_fwd(const S3dUNetParams* U, const S3dHeadParams* Hd, const S3dVggParams* V,
                             const S3dTrainBatch* batch, int B, int S, long Q, int ns, float dropout_p,
                             unsigned long long seed, int prec, float* vgg_loss_out, float* sdf_pred_out,
                             float* slices_rec_out, void* workspace, size_t workspace_bytes, void* stream) {
    S3D_CHECK_ARG(vgg_loss_out && sdf_pred_out && slices_rec_out, "train_fwd: null output");
    StepDims d;
    TrainBufs T = {};
    TRY(open_reg_step("train_fwd", U && Hd && V && batch, B, S, Q, ns, dropout_p, prec, workspace, workspace_bytes, d, T));
    RegStep s(U, Hd, V, nullptr, nullptr, batch, d, T, dropout_p, seed, prec, sdf_pred_out, slices_rec_out, stream);
    TRY(s.R.zero(T.fwd_losses, 4));
    TRY(s.pack_weights());
    TRY(s.forward());
    TRY(s.vgg_loss_value(T.fwd_losses + 2));
    if (hipMemcpyAsync(vgg_loss_out, T.fwd_losses + 2, sizeof(float), hipMemcpyDeviceToDevice, s.st) != hipSuccess) {
        s3d_set_error("train_fwd: copy of vgg_loss failed");
        return S3D_E_ARG;
    }
    return 0;
}

extern "C" int s3d_train_bwd(const S3dUNetParams* U, const S3dHeadParams* Hd, const S3dVggParams* V,
                             const S3dUNetParams* dU, const S3dHeadParams* dH, const S3dTrainBatch* batch,
                             int B, int S, long Q, int ns, float dropout_p, unsigned long long seed, int prec,
                             const float* d_sdf_pred, const float* d_slices_rec, float d_vgg_loss, float grad_scale,
                             float* slices_rec, void* workspace, size_t workspace_bytes, void* stream) {
    S3D_CHECK_ARG(slices_rec, "train_bwd: slices_rec (the forward's output) is NULL");
    StepDims d;
    TrainBufs T = {};
    TRY(open_reg_step("train_bwd", U && Hd && V && dU && dH && batch, B, S, Q, ns, dropout_p, prec, workspace,
                      workspace_bytes, d, T));
    RegStep s(U, Hd, V, dU, dH, batch, d, T, dropout_p, seed, prec, nullptr, slices_rec, stream);
    TRY(s.external_loss_grads(TrainExt{d_sdf_pred, d_slices_rec, d_vgg_loss, grad_scale}));
    // (the tap kernels also sum the loss: into scratch here)
    if (d_vgg_loss != 0.f) TRY(s.vgg_backward(T.vec, d_vgg_loss));
    return s.backward();
}

// dropout mask as the kernels generate it: out[i] = keep(seed, site, idx0 + i) ? 1/(1-p) : 0   (testing hook)
extern "C" int s3d_dropout_mask(unsigned long long seed, int site, unsigned long long idx0, long n, float p,
                                float* out, void* stream) {
    S3D_CHECK_ARG(out && n >= 0 && p >= 0.f && p < 1.f, "dropout_mask: bad argument");
    return launch_dropout_apply(nullptr, out, n, idx0, make_drop(seed, p, site), (hipStream_t)stream);
}

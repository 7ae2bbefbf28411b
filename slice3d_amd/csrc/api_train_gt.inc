// api_train_gt.inc — included by api.hip after api_train.inc: train-mode forward + L1 loss + backward of
// Slices3DGTModel (train_step of reg_slices/train_gt.py:38-52 minus opt.step, model_gt.py:59-111).
//
//   img_slices (B,3*ns,S,S) -> VGG16-BN encoder on B*ns images (batch-stat BatchNorm) -> five raw taps
//   -> fc_local[0] folded into the four coarse levels (1x1 projections), conv1_2 sampled raw
//   -> sampler (+ReLU) -> fc_local[2] (+ReLU) | pts_feat_extractor on token 0 -> transformer -> fc_out -> L1
// and the reverse walk.  The encoder, the decoder (DecoderTrain) and every GEMM / reduction kernel are the ones
// s3d_train_fwd_bwd uses; only the token builder and its backward are specific to this model.

struct GtTrainBufs {
    float* gproj[4];      // folded latent maps, coarse -> fine (n_img, W, W, 128)
    float* dgproj[4];
    FragW w_projT[4];     // fc_local[0] slices, transposed use (d level = d proj W)
    float* wrawT16;       // the same as f16 hi|lo fragment pairs
    float* wrawT;         // LINEAR_T fragment image of fc_local[0][:, 0:64] ([4][8] tiles) for the sampler backward
    float* X1;            // relu(fc_local[0](sampled features)) per token row; token-0 rows zero
    float* raw64;         // sampled conv1_2 features per token row
    FragW w_l1N, w_l1T;   // fc_local[2]
    FragW w_p2T, w_p1T;   // pts_feat_extractor.4 / .2, transposed use
    float *h1, *h2;       // pts_feat_extractor hidden activations per query row
    float *dh1, *dh2;
    float* qrot4;
};

static void plan_train_gt(Arena& A, int B, int S, long Q, int ns, TrainBufs& T, GtTrainBufs& X) {
    const int Nd = B * ns;
    plan_enc(A, Nd, S, T);
    const long gpb = (Q + S3D_GROUP - 1) / S3D_GROUP, G = gpb * B;
    const size_t rows = (size_t)G * (ns + 1) * S3D_GROUP, rows0 = (size_t)G * S3D_GROUP;
    T.head_packed = A.take(gt_head_layout().total);
    for (int l = 0; l < 4; ++l) {
        const size_t r = (size_t)(S / 16) << l;
        X.gproj[l] = A.take((size_t)Nd * r * r * 128);
        X.dgproj[l] = A.take((size_t)Nd * r * r * 128);
        X.w_projT[l] = frag_alloc(A, kGtC[4 - l], 128);
    }
    X.wrawT = A.take(64 * 128);
    X.wrawT16 = A.take(64 * 128);
    X.X1 = A.take(rows * 128);
    X.raw64 = A.take(rows * 64);
    X.w_l1N = frag_alloc(A, 128, 128);
    X.w_l1T = frag_alloc(A, 128, 128);
    X.w_p2T = frag_alloc(A, 64, 128);
    X.w_p1T = frag_alloc(A, 32, 64);
    X.h1 = A.take(rows0 * 32); X.h2 = A.take(rows0 * 64);
    X.dh1 = A.take(rows0 * 32); X.dh2 = A.take(rows0 * 64);
    X.qrot4 = A.take(rows0 * 4);
    plan_dec(A, B, Q, ns, T);
    plan_shared(A, T);
}

extern "C" size_t s3d_gt_train_workspace_bytes(int batch, int size, long n_qry, int n_slices) {
    Arena A{nullptr, 0};
    TrainBufs T;
    GtTrainBufs X;
    plan_train_gt(A, batch, size, n_qry, n_slices, T, X);
    return A.off * sizeof(float);
}

extern "C" int s3d_gt_train_fwd_bwd(const S3dVgg16BnParams* E, const S3dGtHeadParams* Hd, const S3dVgg16BnParams* dE,
                                    const S3dGtHeadParams* dH, const S3dTrainBatch* batch, int B, int S, long Q,
                                    int ns, float dropout_p, unsigned long long seed, int prec, float* losses_out,
                                    float* sdf_pred_out, void* workspace, size_t workspace_bytes, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    S3D_CHECK_ARG(E && Hd && dE && dH && batch && losses_out && workspace, "gt_train: null argument");
    S3D_CHECK_ARG(batch->img_slices && batch->qry && batch->rot && batch->trans && batch->sdf,
                  "gt_train: batch needs img_slices, qry, rot, trans and sdf");
    S3D_CHECK_ARG(B >= 1 && S >= 16 && S % 16 == 0 && Q >= 1 && ns >= 1 && ns <= 12, "gt_train: bad dims");
    S3D_CHECK_ARG(dropout_p >= 0.f && dropout_p < 1.f, "gt_train: dropout %g out of range", (double)dropout_p);
    S3D_CHECK_ARG(prec == S3D_PREC_F32 || prec == S3D_PREC_F16X3, "gt_train: precision mode %d", prec);
    Arena A{(float*)workspace, 0};
    TrainBufs T = {};
    GtTrainBufs X;
    plan_train_gt(A, B, S, Q, ns, T, X);
    if (workspace_bytes < A.off * sizeof(float)) {
        s3d_set_error("gt_train: workspace %zu < %zu bytes", workspace_bytes, A.off * sizeof(float));
        return S3D_E_WORKSPACE;
    }
    const int Nd = B * ns, r5 = S / 16, Tn = ns + 1;
    TrainRun R{st, T, B, S, ns, Nd, prec, batch->sync_bn};
    const GtHeadLayout GL = gt_head_layout();
    const float* hb = T.head_packed;
    const long gpb = (Q + S3D_GROUP - 1) / S3D_GROUP, G = gpb * B;
    const long rows = G * Tn * S3D_GROUP, rows0 = G * S3D_GROUP;
    const long nsdf = (long)B * Q;
    TRY(R.zero(losses_out, 2));

    // ---- 1. weight packs ----
    PackBatchScope packs;
    TRY(enc_pack(R, E->conv));
    TRY(s3d_gt_head_pack(Hd, T.head_packed, GL.total * sizeof(float), stream));
    for (int l = 0; l < 4; ++l)
        TRY(R.pack_lin_t(X.w_projT[l], Hd->local_w[0] + kGtCol[4 - l], kGtC[4 - l], 128, 1472));
    {
        FragW f{X.wrawT, X.wrawT16, 64, 8};
        TRY(R.pack_lin_t(f, Hd->local_w[0], 64, 128, 1472));
    }
    TRY(R.pack_lin(X.w_l1N, Hd->local_w[1], 128, 128, 128));
    TRY(R.pack_lin_t(X.w_l1T, Hd->local_w[1], 128, 128, 128));
    TRY(R.pack_lin_t(X.w_p2T, Hd->pts_w[2], 64, 128, 64));
    TRY(R.pack_lin_t(X.w_p1T, Hd->pts_w[1], 32, 64, 32));
    DecoderTrain D{R, T, st, Hd->layer, dH->layer, Hd->fc_out_w, (float*)dH->fc_out_w, (float*)dH->fc_out_b,
                   T.head_packed, GL.H, prec, dropout_p, seed, G, gpb, Q, rows, rows0, Tn, nullptr};
    TRY(D.pack_layers());
    TRY(packs.flush(st));

    // ---- 2. encoder forward (vgg16bn_feats.py:42-57; conv_last's BatchNorm only moves its running stats) ----
    TRY(enc_forward(R, E->conv, batch->img_slices, Nd, S, 1));
    for (int l = 0; l < 4; ++l) {   // fc_local[0] folded into conv5_3 ... conv2_2
        const int lev = 4 - l, r = r5 << l, C = kGtC[lev];
        TRY(launch_conv(proj_desc(hb + GL.wproj[l], prec == S3D_PREC_F16X3 ? hb + GL.wproj16[l] : nullptr, false, 128, C,
                                  T.z[kTapConv[lev]], Nd, r, r, X.gproj[l]),
                        st));
    }

    // ---- 3. tokens (model_gt.py:78-99) ----
    const int* perm = Q >= S3D_SORT_MIN_QUERIES ? T.perm : nullptr;
    if (perm) TRY(launch_query_sort(batch->qry, batch->rot, batch->trans, 0, B, Q, T.perm, T.sortws, st));
    D.perm = perm;
    {
        SampleGtArgs sa = {};
        for (int l = 0; l < 4; ++l) sa.proj[l] = X.gproj[l];
        sa.fine = T.z[1];
        sa.wraw = hb + GL.wraw; sa.bias = hb + GL.bl0;
        sa.wraw16 = prec == S3D_PREC_F16X3 ? hb + GL.wraw16 : nullptr;
        sa.size = S; sa.n_slices = ns;
        sa.qry = batch->qry; sa.rot = batch->rot; sa.trans = batch->trans; sa.flip_yz = 0;
        sa.n_qry = Q; sa.groups_per_batch = gpb; sa.g_begin = 0; sa.g_count = G;
        sa.nx = 0; sa.box = 1.f; sa.X = X.X1; sa.perm = perm; sa.raw_out = X.raw64;
        TRY(launch_sample_tokens_gt(sa, st));
        TRY(D.lin(X.w_l1N, 128, 128, hb + GL.bl1, X.X1, rows, T.X0, nullptr, 0, nullptr, S3D_ACT_RELU));
        GtPointArgs pa = {};
        pa.w0 = hb + GL.pw0; pa.b0 = hb + GL.pb0; pa.w1 = hb + GL.pw1; pa.b1 = hb + GL.pb1;
        pa.w2 = hb + GL.pw2; pa.b2 = hb + GL.pb2;
        pa.qry = batch->qry; pa.rot = batch->rot; pa.flip_yz = 0; pa.n_slices = ns;
        pa.n_qry = Q; pa.groups_per_batch = gpb; pa.g_begin = 0; pa.g_count = G;
        pa.nx = 0; pa.box = 1.f; pa.X = T.X0; pa.perm = perm; pa.h1_out = X.h1; pa.h2_out = X.h2;
        TRY(launch_gt_point_tokens(pa, st));
        TRY(launch_qry_rot_rows(batch->qry, batch->rot, 0, Q, gpb, G, perm, X.qrot4, st));
    }

    // ---- 4. decoder + loss (train_gt.py:28-36: L1 on the sdf; accuracy = sign agreement) ----
    float* sdf = sdf_pred_out ? sdf_pred_out : T.sdf;
    TRY(D.forward(T.X0, sdf));
    const float gs = backward_scale(prec, nsdf);   // see api_train.inc: removed from the parameter gradients at the end
    TRY(launch_l1_fwd_bwd(sdf, batch->sdf, nsdf, 1.f / (float)nsdf, T.dsdf, 0, T.cpartial, losses_out + 0, st, gs));
    TRY(launch_scalar_reduce(sdf, batch->sdf, nsdf, 1, 1.f / (float)nsdf, losses_out + 1, 0, T.cpartial, st));
    TRY(D.backward(T.X0, T.dsdf, nsdf));   // d X0 in T.dA; T.dB / T.dO / T.dc1 / T.dc2 are free again

    // ---- 5. token builder backward ----
    float* dP2 = T.dB;   // d (pre-ReLU fc_local[2] output); its token-0 rows carry d (pre-ReLU point feature)
    float* dP1 = T.dO;   // d (pre-ReLU fc_local[0] output)
    TRY(R.copy(dP2, T.dA, (size_t)rows * 128));
    TRY(launch_relu_mask_bwd(T.X0, dP2, rows * 128, st));
    TRY(launch_tok0_copy(dP2, T.dc1, G, Tn, 0, 128, st));
    TRY(R.zero(T.dc2, (size_t)rows0 * 128));
    TRY(launch_tok0_copy(dP2, T.dc2, G, Tn, 1, 128, st));          // slice rows only from here on
    {   // fc_local[2]
        WgradArgs w = R.wg(dP2, 128, 128, plain_src(X.X1, 128), 128, 1, 1, (int)rows, 1);
        w.out = (float*)dH->local_w[1]; w.out_kind = S3D_PACK_LINEAR; w.ld = 128;
        w.bias_out = (float*)dH->local_b[1];
        TRY(launch_wgrad(w, st));
        TRY(D.lin(X.w_l1T, 128, 128, nullptr, dP2, rows, dP1, nullptr, 0));
        TRY(launch_relu_mask_bwd(X.X1, dP1, rows * 128, st));       // X1 is zero on token-0 rows
    }
    {   // fc_local[0]: bias, the raw conv1_2 slice, then the sampler backward
        WgradArgs w = R.wg(dP1, 128, 128, plain_src(X.raw64, 64), 64, 1, 1, (int)rows, 1);
        w.out = (float*)dH->local_w[0]; w.out_kind = S3D_PACK_LINEAR; w.ld = 1472;
        w.bias_out = (float*)dH->local_b[0];
        TRY(launch_wgrad(w, st));
        for (int l = 0; l < 4; ++l) {
            const size_t r = (size_t)r5 << l;
            TRY(R.zero(X.dgproj[l], (size_t)Nd * r * r * 128));
        }
        TRY(R.zero(T.dskip[0], (size_t)Nd * S * S * 64));
        SampleBwdArgs sb = {};
        sb.dX = dP1;
        for (int l = 0; l < 3; ++l) sb.dproj[l] = X.dgproj[l];
        sb.dfine[0] = X.dgproj[3]; sb.dfine[1] = T.dskip[0];
        sb.ws34_t = X.wrawT; sb.gt = 1;
        sb.ws34_t16 = prec == S3D_PREC_F16X3 ? X.wrawT16 : nullptr;
        sb.qry = batch->qry; sb.rot = batch->rot; sb.trans = batch->trans;
        sb.flip_yz = 0; sb.size = S; sb.n_slices = ns;
        sb.n_qry = Q; sb.groups_per_batch = gpb; sb.groups = G;
        sb.perm = perm; sb.bin_ends = perm ? T.sortws : nullptr;
        sb.gxy = perm ? T.gxy : nullptr;
        TRY(launch_sample_bwd(sb, st));
    }
    for (int l = 0; l < 4; ++l) {   // folded fc_local[0] slices: dW_l = dG_l^T f_l ;  d f_l = dG_l W_l
        const int lev = 4 - l, r = r5 << l, C = kGtC[lev];
        WgradArgs wf = R.wg(X.dgproj[l], 128, 128, plain_src(T.z[kTapConv[lev]], C), C, Nd, r, r, 1);
        wf.out = (float*)dH->local_w[0] + kGtCol[lev]; wf.out_kind = S3D_PACK_LINEAR; wf.ld = 1472;
        TRY(launch_wgrad(wf, st));
        ConvLaunch c = R.mk(X.w_projT[l], Nd, r, r, 1, nullptr, S3D_ACT_NONE);
        c.nsrc = 1;
        c.src[0] = plain_src(X.dgproj[l], 128);
        c.out = T.dskip[lev];
        TRY(launch_conv(c, st));
    }
    {   // pts_feat_extractor (model_gt.py:24-31) on the token-0 rows; T.dc1 = d (pre-ReLU output)
        float* vec = T.vec;
        TRY(launch_colsum(T.dc1, rows0, 128, 0, 128, (float*)dH->pts_b[2], 0, T.cpartial, st));
        WgradArgs w2 = R.wg(T.dc1, 128, 128, plain_src(X.h2, 64), 64, 1, 1, (int)rows0, 1);
        w2.out = (float*)dH->pts_w[2]; w2.out_kind = S3D_PACK_LINEAR; w2.ld = 64;
        TRY(launch_wgrad(w2, st));
        TRY(D.lin(X.w_p2T, 64, 128, nullptr, T.dc1, rows0, X.dh2, nullptr, 0));
        TRY(launch_relu_mask_bwd(X.h2, X.dh2, rows0 * 64, st));
        TRY(launch_colsum(X.dh2, rows0, 64, 0, 64, (float*)dH->pts_b[1], 0, T.cpartial, st));
        WgradArgs w1 = R.wg(X.dh2, 64, 64, plain_src(X.h1, 32), 32, 1, 1, (int)rows0, 1);
        w1.out = (float*)dH->pts_w[1]; w1.out_kind = S3D_PACK_LINEAR; w1.ld = 32;
        TRY(launch_wgrad(w1, st));
        TRY(D.lin(X.w_p1T, 32, 64, nullptr, X.dh2, rows0, X.dh1, nullptr, 0));
        TRY(launch_relu_mask_bwd(X.h1, X.dh1, rows0 * 32, st));
        TRY(launch_colsum(X.dh1, rows0, 32, 0, 32, (float*)dH->pts_b[0], 0, T.cpartial, st));
        WgradArgs w0 = R.wg(X.dh1, 32, 32, plain_src(X.qrot4, 4), 4, 1, 1, (int)rows0, 1);
        w0.out = vec; w0.out_kind = S3D_PACK_LINEAR; w0.ld = 4;                       // [32][4] -> [32][3]
        TRY(launch_wgrad(w0, st));
        TRY(launch_copy_cols(vec, (float*)dH->pts_w[0], 32, 4, 3, st));
    }

    // ---- 6. encoder backward ----
    TRY(enc_backward(R, E->conv, dE->conv, Nd, S));
    if (gs != 1.f) {
        ScaleTable tb;
        tb.count = 0;
        add_enc_grads(tb, dE->conv);
        tb.add(dH->pts_w[0], 32 * 3); tb.add(dH->pts_w[1], 64 * 32); tb.add(dH->pts_w[2], 128 * 64);
        tb.add(dH->pts_b[0], 32); tb.add(dH->pts_b[1], 64); tb.add(dH->pts_b[2], 128);
        tb.add(dH->local_w[0], 128 * 1472); tb.add(dH->local_w[1], 128 * 128);
        tb.add(dH->local_b[0], 128); tb.add(dH->local_b[1], 128);
        add_layer_grads(tb, dH->layer);
        tb.add(dH->fc_out_w, 128); tb.add(dH->fc_out_b, 1);
        TRY(launch_scale_table(tb, 1.f / gs, st));
    }
    return 0;
}

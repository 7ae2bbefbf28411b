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

static void plan_train_gt(Arena& A, const StepDims& d, TrainBufs& T, GtTrainBufs& X) {
    const int Nd = d.Nd;
    const size_t rows = (size_t)d.rows, rows0 = (size_t)d.rows0;
    plan_enc(A, d, Nd, T);
    T.head_packed = A.take(gt_head_layout().total);
    for (int l = 0; l < 4; ++l) {
        const size_t r = (size_t)d.r5 << l;
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
    plan_dec(A, d, T);
    plan_shared(A, T);
}

extern "C" size_t s3d_gt_train_workspace_bytes(int batch, int size, long n_qry, int n_slices) {
    Arena A{nullptr, 0};
    TrainBufs T;
    GtTrainBufs X;
    plan_train_gt(A, step_dims(batch, size, n_qry, n_slices), T, X);
    return A.off * sizeof(float);
}

// The GT model's step on the skeleton of the Reg model's (TrainStep); its own: the weight packs, the encoder's folded
// projections, the token builder and that builder's backward.
struct GtStep : TrainStep {
    const S3dVgg16BnParams *E, *dE;
    const S3dGtHeadParams *Hd, *dH;
    GtTrainBufs& X;
    const GtHeadLayout GL;
    const float* hb;   // the packed head image

    GtStep(const S3dVgg16BnParams* E_, const S3dGtHeadParams* Hd_, const S3dVgg16BnParams* dE_, const S3dGtHeadParams* dH_,
           const S3dTrainBatch* batch_, const StepDims& d_, TrainBufs& T_, GtTrainBufs& X_, float dropout_p,
           unsigned long long seed, int prec, void* stream)
        : TrainStep(batch_, d_, T_, stream, prec, dropout_p, seed, Hd_->layer, dH_->layer, Hd_->fc_out_w, dH_->fc_out_w,
                    dH_->fc_out_b, gt_head_layout().H),
          E(E_), dE(dE_), Hd(Hd_), dH(dH_), X(X_), GL(gt_head_layout()), hb(T_.head_packed) {}

    // ---- 1. weight packs ----
    int pack_weights() {
        PackBatchScope packs;
        TRY_RET(enc_pack(R, E->conv));
        TRY_RET(s3d_gt_head_pack(Hd, T.head_packed, GL.total * sizeof(float), st));
        for (int l = 0; l < 4; ++l)
            TRY_RET(R.pack_lin_t(X.w_projT[l], Hd->local_w[0] + kGtCol[4 - l], kGtC[4 - l], 128, 1472));
        {
            FragW f{X.wrawT, X.wrawT16, 64, 8};
            TRY_RET(R.pack_lin_t(f, Hd->local_w[0], 64, 128, 1472));
        }
        TRY_RET(R.pack_lin(X.w_l1N, Hd->local_w[1], 128, 128, 128));
        TRY_RET(R.pack_lin_t(X.w_l1T, Hd->local_w[1], 128, 128, 128));
        TRY_RET(R.pack_lin_t(X.w_p2T, Hd->pts_w[2], 64, 128, 64));
        TRY_RET(R.pack_lin_t(X.w_p1T, Hd->pts_w[1], 32, 64, 32));
        TRY_RET(D.pack_layers());
        return packs.flush(st);
    }

    // ---- 2. encoder forward (vgg16bn_feats.py:42-57; conv_last's BatchNorm only moves its running stats) ----
    int encoder_forward() {
        TRY_RET(enc_forward(R, E->conv, batch->img_slices, d.Nd, d.S, 1));
        for (int l = 0; l < 4; ++l) {   // fc_local[0] folded into conv5_3 ... conv2_2
            const int lev = 4 - l, r = d.r5 << l, C = kGtC[lev];
            TRY_RET(launch_conv(proj_desc(hb + GL.wproj[l], R.prec == S3D_PREC_F16X3 ? hb + GL.wproj16[l] : nullptr, false, 128,
                                          C, T.z[kTapConv[lev]], d.Nd, r, r, X.gproj[l]),
                                st));
        }
        return 0;
    }

    // ---- 3. tokens (model_gt.py:78-99) ----
    int tokens_forward() {
        TRY_RET(sort_queries());
        SampleGtArgs sa = {};
        for (int l = 0; l < 4; ++l) sa.proj[l] = X.gproj[l];
        sa.fine = T.z[1];
        sa.wraw = hb + GL.wraw; sa.bias = hb + GL.bl0;
        sa.wraw16 = R.prec == S3D_PREC_F16X3 ? hb + GL.wraw16 : nullptr;
        sa.size = d.S; sa.n_slices = d.ns;
        sa.qry = batch->qry; sa.rot = batch->rot; sa.trans = batch->trans; sa.flip_yz = 0;
        sa.n_qry = d.Q; sa.groups_per_batch = d.gpb; sa.g_begin = 0; sa.g_count = d.G;
        sa.nx = 0; sa.box = 1.f; sa.X = X.X1; sa.perm = perm; sa.raw_out = X.raw64;
        TRY_RET(launch_sample_tokens_gt(sa, st));
        TRY_RET(D.lin(X.w_l1N, 128, 128, hb + GL.bl1, X.X1, d.rows, T.X0, nullptr, 0, nullptr, S3D_ACT_RELU));
        GtPointArgs pa = {};
        pa.w0 = hb + GL.pw0; pa.b0 = hb + GL.pb0; pa.w1 = hb + GL.pw1; pa.b1 = hb + GL.pb1;
        pa.w2 = hb + GL.pw2; pa.b2 = hb + GL.pb2;
        pa.qry = batch->qry; pa.rot = batch->rot; pa.flip_yz = 0; pa.n_slices = d.ns;
        pa.n_qry = d.Q; pa.groups_per_batch = d.gpb; pa.g_begin = 0; pa.g_count = d.G;
        pa.nx = 0; pa.box = 1.f; pa.X = T.X0; pa.perm = perm; pa.h1_out = X.h1; pa.h2_out = X.h2;
        TRY_RET(launch_gt_point_tokens(pa, st));
        return launch_qry_rot_rows(batch->qry, batch->rot, 0, d.Q, d.gpb, d.G, perm, X.qrot4, st);
    }

    // ---- 4. decoder + loss (train_gt.py:28-36: L1 on the sdf; accuracy = sign agreement) + decoder backward ----
    int decoder_loss_and_backward(float* sdf, float* losses_out) {
        const long nsdf = d.nsdf;
        TRY_RET(D.forward(T.X0, sdf));
        TRY_RET(launch_l1_fwd_bwd(sdf, batch->sdf, nsdf, 1.f / (float)nsdf, T.dsdf, 0, T.cpartial, losses_out + 0, st, gs));
        TRY_RET(launch_scalar_reduce(sdf, batch->sdf, nsdf, 1, 1.f / (float)nsdf, losses_out + 1, 0, T.cpartial, st));
        return D.backward(T.X0, T.dsdf, nsdf);   // d X0 in T.dA; T.dB / T.dO / T.dc1 / T.dc2 are free again
    }

    // ---- 5. token builder backward: d X0 (T.dA) -> fc_local gradients, d of the five encoder taps (T.dskip); leaves
    //      d (pre-ReLU point feature) of the token-0 rows in T.dc1 ----
    int tokens_backward() {
        const int S = d.S, Nd = d.Nd, r5 = d.r5;
        const long rows = d.rows, rows0 = d.rows0;
        float* dP2 = T.dB;   // d (pre-ReLU fc_local[2] output); its token-0 rows carry d (pre-ReLU point feature)
        float* dP1 = T.dO;   // d (pre-ReLU fc_local[0] output)
        TRY_RET(R.copy(dP2, T.dA, (size_t)rows * 128));
        TRY_RET(launch_relu_mask_bwd(T.X0, dP2, rows * 128, st));
        TRY_RET(launch_tok0_copy(dP2, T.dc1, d.G, d.Tn, 0, 128, st));
        TRY_RET(R.zero(T.dc2, (size_t)rows0 * 128));
        TRY_RET(launch_tok0_copy(dP2, T.dc2, d.G, d.Tn, 1, 128, st));          // slice rows only from here on
        // fc_local[2]
        TRY_RET(R.wgrad_lin(R.wg_rows(dP2, 128, X.X1, 128, rows), dH->local_w[1], 128, dH->local_b[1]));
        TRY_RET(D.lin(X.w_l1T, 128, 128, nullptr, dP2, rows, dP1, nullptr, 0));
        TRY_RET(launch_relu_mask_bwd(X.X1, dP1, rows * 128, st));       // X1 is zero on token-0 rows
        // fc_local[0]: bias, the raw conv1_2 slice, then the sampler backward
        TRY_RET(R.wgrad_lin(R.wg_rows(dP1, 128, X.raw64, 64, rows), dH->local_w[0], 1472, dH->local_b[0]));
        for (int l = 0; l < 4; ++l) {
            const size_t r = (size_t)r5 << l;
            TRY_RET(R.zero(X.dgproj[l], (size_t)Nd * r * r * 128));
        }
        TRY_RET(R.zero(T.dskip[0], (size_t)Nd * S * S * 64));
        SampleBwdArgs sb = sample_bwd_args(dP1);
        for (int l = 0; l < 3; ++l) sb.dproj[l] = X.dgproj[l];
        sb.dfine[0] = X.dgproj[3]; sb.dfine[1] = T.dskip[0];
        sb.ws34_t = X.wrawT; sb.gt = 1;
        sb.ws34_t16 = R.prec == S3D_PREC_F16X3 ? X.wrawT16 : nullptr;
        TRY_RET(launch_sample_bwd(sb, st));
        for (int l = 0; l < 4; ++l) {   // folded fc_local[0] slices: dW_l = dG_l^T f_l ;  d f_l = dG_l W_l
            const int lev = 4 - l, r = r5 << l, C = kGtC[lev];
            TRY_RET(R.wgrad_lin(R.wg(X.dgproj[l], 128, 128, plain_src(T.z[kTapConv[lev]], C), C, Nd, r, r, 1),
                                dH->local_w[0] + kGtCol[lev], 1472));
            TRY_RET(R.conv(X.w_projT[l], Nd, r, r, 1, X.dgproj[l], 128, T.dskip[lev]));
        }
        return 0;
    }

    // pts_feat_extractor (model_gt.py:24-31) on the token-0 rows; T.dc1 = d (pre-ReLU output)
    int point_features_backward() {
        const long rows0 = d.rows0;
        TRY_RET(launch_colsum(T.dc1, rows0, 128, 0, 128, (float*)dH->pts_b[2], 0, T.cpartial, st));
        TRY_RET(R.wgrad_lin(R.wg_rows(T.dc1, 128, X.h2, 64, rows0), dH->pts_w[2], 64));
        TRY_RET(D.lin(X.w_p2T, 64, 128, nullptr, T.dc1, rows0, X.dh2, nullptr, 0));
        TRY_RET(launch_relu_mask_bwd(X.h2, X.dh2, rows0 * 64, st));
        TRY_RET(launch_colsum(X.dh2, rows0, 64, 0, 64, (float*)dH->pts_b[1], 0, T.cpartial, st));
        TRY_RET(R.wgrad_lin(R.wg_rows(X.dh2, 64, X.h1, 32, rows0), dH->pts_w[1], 32));
        TRY_RET(D.lin(X.w_p1T, 32, 64, nullptr, X.dh2, rows0, X.dh1, nullptr, 0));
        TRY_RET(launch_relu_mask_bwd(X.h1, X.dh1, rows0 * 32, st));
        TRY_RET(launch_colsum(X.dh1, rows0, 32, 0, 32, (float*)dH->pts_b[0], 0, T.cpartial, st));
        return R.wgrad_xyz(X.dh1, 32, X.qrot4, rows0, dH->pts_w[0]);
    }

    // ---- 6. encoder backward, then the backward scale leaves every gradient ----
    int encoder_backward() {
        TRY_RET(enc_backward(R, E->conv, dE->conv, d.Nd, d.S));
        ScaleTable tb;
        tb.count = 0;
        add_enc_grads(tb, dE->conv);
        tb.add(dH->pts_w[0], 32 * 3); tb.add(dH->pts_w[1], 64 * 32); tb.add(dH->pts_w[2], 128 * 64);
        tb.add(dH->pts_b[0], 32); tb.add(dH->pts_b[1], 64); tb.add(dH->pts_b[2], 128);
        tb.add(dH->local_w[0], 128 * 1472); tb.add(dH->local_w[1], 128 * 128);
        tb.add(dH->local_b[0], 128); tb.add(dH->local_b[1], 128);
        add_layer_grads(tb, dH->layer);
        tb.add(dH->fc_out_w, 128); tb.add(dH->fc_out_b, 1);
        return rescale(tb);
    }
};

extern "C" int s3d_gt_train_fwd_bwd(const S3dVgg16BnParams* E, const S3dGtHeadParams* Hd, const S3dVgg16BnParams* dE,
                                    const S3dGtHeadParams* dH, const S3dTrainBatch* batch, int B, int S, long Q,
                                    int ns, float dropout_p, unsigned long long seed, int prec, float* losses_out,
                                    float* sdf_pred_out, void* workspace, size_t workspace_bytes, void* stream) {
    S3D_CHECK_ARG(!batch || (batch->img_slices && batch->qry && batch->rot && batch->trans && batch->sdf),
                  "gt_train: batch needs img_slices, qry, rot, trans and sdf");
    StepDims d;
    TrainBufs T = {};
    GtTrainBufs X;
    TRY(open_step("gt_train", E && Hd && dE && dH && batch && losses_out, B, S, Q, ns, dropout_p, prec,
                  prec == S3D_PREC_F32 || prec == S3D_PREC_F16X3, workspace, workspace_bytes, d, T, &X));
    GtStep s(E, Hd, dE, dH, batch, d, T, X, dropout_p, seed, prec, stream);
    TRY(s.R.zero(losses_out, 2));
    TRY(s.pack_weights());
    TRY(s.encoder_forward());
    TRY(s.tokens_forward());
    TRY(s.decoder_loss_and_backward(sdf_pred_out ? sdf_pred_out : T.sdf, losses_out));
    TRY(s.tokens_backward());
    TRY(s.point_features_backward());
    return s.encoder_backward();
}

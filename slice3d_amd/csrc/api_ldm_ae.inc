// api_ldm_ae.inc — C ABI of the gen_slices first-stage autoencoder (AutoencoderKL, reference
// ldm/modules/diffusionmodules/model.py) and condition encoder (ImageEncoderVGG16BN, ldm/modules/encoders/modules.py) primitives
// that the U-Net's entry points (api_ldm.inc) do not cover.  The module structure is host logic in
// slice3d_amd/ldm_autoencoder.py; tensors are channels-last fp32 unless stated.

// A strided convolution on the generic MFMA kernel: out[n, y, x, :cout] = sum_tap w[tap] . in[n, stride*y + tap_y - pad,
// stride*x + tap_x - pad, :] + bias, with zeros outside the (Hin, Win) input.  pad = ks / 2, or 0 with pad_origin = 1 (ks 3:
// Downsample's F.pad (0,1,0,1) + Conv2d(stride 2), model.py:60-79).  ks 1 with stride s: the nearest s-fold resize of a
// 1x1 convolution's output computed on the picked pixels only (the condition encoder's trans* projections).
static int conv_strided_desc(ConvLaunch& c, const void* packed, const float* x, float* out, int N, int Hin, int Win, int Hout, int Wout,
                             int cout, int cin, int ks, int stride, int pad_origin, int prec) {
    S3D_CHECK_ARG(packed && x && out && N >= 1 && Hin >= 1 && Win >= 1 && Hout >= 1 && Wout >= 1 && cin >= 1 && cout % 4 == 0,
                  "conv_strided: bad arguments");
    S3D_CHECK_ARG((ks == 1 || ks == 3) && stride >= 1 && (pad_origin == 0 || (pad_origin == 1 && ks == 3 && stride > 1)),
                  "conv_strided: ks=%d stride=%d pad_origin=%d", ks, stride, pad_origin);
    S3D_CHECK_ARG(prec == S3D_PREC_F32 || prec == S3D_PREC_F16X3, "conv_strided: precision mode %d", prec);
    const GenConvLayout L = gen_conv_layout(cout, cin, 0, ks);
    const float* b = (const float*)packed;
    c = {};
    c.N = N; c.H = Hout; c.W = Wout; c.ks = ks;
    c.stride = stride; c.Hin = Hin; c.Win = Win; c.pad_origin = pad_origin;
    c.CoutPad = L.cout_pad; c.wpk = b + L.w; c.KU = L.KU;
    const bool f16 = L.KU % 2 == 0 && cin % 32 == 0;
    c.wpk16 = (prec == S3D_PREC_F16X3 && f16) ? (const void*)(b + L.w16) : nullptr;
    c.scale = nullptr;
    c.shift = b + L.shift; c.act = S3D_ACT_NONE;
    c.out_mode = S3D_OUT_NHWC; c.cout_store = cout; c.out_cstride = cout;
    c.nsrc = 1;
    c.src[0] = plain_src(x, pad16(cin));
    c.out = out;
    return 0;
}
extern "C" int s3d_conv_strided_fwd(const void* packed, const float* x, float* out, int N, int Hin, int Win, int Hout, int Wout,
                                    int cout, int cin, int ks, int stride, int pad_origin, int prec, void* stream) {
    ConvLaunch c;
    TRY(conv_strided_desc(c, packed, x, out, N, Hin, Win, Hout, Wout, cout, cin, ks, stride, pad_origin, prec));
    return launch_conv(c, (hipStream_t)stream);
}

// What s3d_conv_fwd / s3d_conv_gn_fwd (fused_gn; nsplit_out_requested) / s3d_conv_strided_fwd (Hin, Win, stride > 0; H, W = the output
// map) would launch for these arguments, without launching it: the ConvLaunch comes from the code those entry points use, the
// plan from the planner launch_conv uses.  No HIP call.  The descriptor's pointers are tested for NULL only (conv_plan.h), so
// one address stands in for every buffer the call would pass.
extern "C" int s3d_conv_plan_describe(int N, int H, int W, int cout, int cin0, int cin1, int ks, int prec, int fused_gn,
                                      size_t workspace_bytes, int nsplit_out_requested, int Hin, int Win, int stride, int pad_origin,
                                      char* buf, size_t buf_len) {
    S3D_CHECK_ARG(buf && buf_len > 0, "conv_plan_describe: no buffer");
    static float some[4];
    const ConvGn gn = {some, 1};
    int nsplit = 0;
    ConvLaunch c;
    if (Hin > 0 || Win > 0 || stride > 0) {
        S3D_CHECK_ARG(!fused_gn && !nsplit_out_requested && !workspace_bytes && !cin1, "conv_plan_describe: the strided entry point takes one source, no GroupNorm, no workspace");
        TRY(conv_strided_desc(c, some, some, some, N, Hin, Win, H, W, cout, cin0, ks, stride, pad_origin, prec));
    } else {
        S3D_CHECK_ARG(fused_gn || !nsplit_out_requested, "conv_plan_describe: nsplit_out is an argument of s3d_conv_gn_fwd");
        TRY(conv_fwd_desc(c, some, some, cin1 > 0 ? some : nullptr, nullptr, some, N, H, W, cout, cin0, cin1, ks, prec, some, workspace_bytes,
                          fused_gn ? &gn : nullptr, nsplit_out_requested ? &nsplit : nullptr));
    }
    const ConvPlan p = conv_plan(c, conv_tuning());
    if (p.err) return p.err;
    conv_plan_describe(c, p, buf, buf_len);
    return 0;
}

extern "C" int s3d_wide_attention_fwd(const float* qkv, float* out, int N, int T, int C, int prec, void* stream) {
    S3D_CHECK_ARG(qkv && out, "wide_attention: null argument");
    S3D_CHECK_ARG(prec == S3D_PREC_F32 || prec == S3D_PREC_F16X3, "wide_attention: precision mode %d", prec);
    return launch_wide_attention(qkv, out, N, T, C, (hipStream_t)stream);
}

extern "C" int s3d_image_normalize_fwd(const float* x, const float* mean, const float* stdv, float* y, int n, int c, int h, int w,
                                       void* stream) {
    S3D_CHECK_ARG(x && mean && stdv && y, "image_normalize: null argument");
    return launch_image_normalize(x, mean, stdv, y, n, c, (long)h * w, (hipStream_t)stream);
}

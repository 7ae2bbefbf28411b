/*
 * slice3d_hip.h — C ABI of libslice3d_hip.so (gfx950 / MI355X).
 *
 * Drop-in boundary for the Slice3D regression hot path.  The reference has NO plugin / FFI layer for
 * this path (it is nn.Module code over ATen ops); the boundary a maintainer binds is
 * therefore "one C entry point per reference function", each citing the reference code it replaces.
 * The Python mirror of the reference's module API (slice3d_amd/models.py, generator.py) calls these
 * through ctypes; INTEGRATION.md shows the stub a reference maintainer would add.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless the name ends in _host; the caller owns all memory
 *     (outputs, packed weights, workspace).  The library never allocates or frees device memory and
 *     keeps no global device state.
 *   - every call enqueues work on `stream` (a hipStream_t passed as void*) and returns immediately.
 *   - return value: 0 = ok, <0 = S3D_E_* argument/size error (message via s3d_last_error()),
 *     >0 = a hipError_t raised by a launch.
 *   - all tensors are fp32.  Activations the library produces are channels-last (NHWC); the image
 *     input and the reconstructed slice images cross the boundary in the reference's NCHW layout.
 *   - batch x slice flattening is batch-major (row b*n_slices+s), as in the reference
 *     (unet_custom.py:35-38, models.py:66,70,78).
 */
#ifndef SLICE3D_HIP_H
#define SLICE3D_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define S3D_VERSION 125         /* 0.1.1: s3d_conv_fwd prec semantics, s3d_conv_gn_supported; 111: s3d_decode_set_last_fused, s3d_decode_set_shared_footprint; 112: S3D_PREC_F16 accepted by s3d_train_*; 113: atomic-free sampling backward (bit-reproducible s3d_train_* gradients, larger workspace); 114: s3d_qkv_attention_ws_* serve head width 48; 115: s3d_add_nchw_fwd; 116: s3d_conv_strided_fwd, s3d_wide_attention_fwd, s3d_image_normalize_fwd; 117: mesh evaluation (s3d_mesh_contains_*, s3d_nn_sqdist, s3d_surface_sample); 118: s3d_mesh_dist_*, s3d_mesh_winding; 119: s3d_mesh_render_*; 120: s3d_unet_encode_fwd computes the decoder's slice-invariant terms once per image, the weights-only ones in s3d_unet_pack (other packed-image and workspace sizes: query them); 121: up2-up4 run ConvTranspose and the first 3x3's up half as one convolution of the low-resolution map with weights composed in s3d_unet_pack (packed-image and workspace sizes change again); 122: s3d_mesh_simplify_*; 123: s3d_conv_plan_describe; 124: s3d_mesh_topology_*; 125: s3d_decode_points_stages_fwd also captures the token tensor after layers 0 and 1 (s3d_decode_stages_floats grows) */
#define S3D_E_ARG (-1)           /* bad argument / unsupported shape */
#define S3D_E_WORKSPACE (-2)     /* workspace or packed-weight buffer too small */
#define S3D_E_ROUNDS (-3)        /* s3d_mesh_topology_run: the component labels did not converge within its round bound */

#define S3D_N_LEVELS 5           /* feature pyramid levels, coarse -> fine (unet_custom.py:58-67) */
#define S3D_D_MODEL 128
#define S3D_N_LAYERS 3
#define S3D_FFN 2048
#define S3D_N_TOKENS_MAX 13      /* 1 point token + up to 12 slice tokens (models.py:82) */

/* arithmetic mode of the MFMA contractions (argument `prec`) */
#define S3D_PREC_F32 0           /* v_mfma_f32_16x16x4_f32: exact fp32, the parity mode */
#define S3D_PREC_F16X3 1         /* fp32 operands split into f16 hi+lo, 3 f16 MFMAs per product (22-bit
                                    significands, fp32 accumulate): fp32-class results; conv / attention / FFN */
#define S3D_PREC_F16 2           /* THROUGHPUT MODE, not fp32-class: operands rounded to f16, ONE f16 MFMA per product,
                                  * fp32 accumulation and fp32 everywhere else (LayerNorm, softmax, sampling).  What
                                  * BASELINE configs[1]'s "bf16" names; fails the 1e-4 parity gate by construction and is
                                  * reported separately with its measured error (bench.py `throughput_mode_f16`).
                                  * Inference entry points of Slices3DRegModel / Slices3DGTModel only. */
#define S3D_PREC_BF16 3          /* THROUGHPUT MODE on the bf16 MFMA (round 5), Slices3DRegModel inference only: the decoder's
                                  * attention and FFN GEMMs (94 % of the decoder's FLOPs; layers 0-1 and the final FFN) run
                                  * v_mfma_f32_16x16x32_bf16 on bf16-rounded operands (weights from a bf16 image, activations
                                  * through v_cvt_pk_bf16_f32), one MFMA per product, fp32 accumulation; every other
                                  * contraction of the path (U-Net, latent projections, token builder, absorbed last-layer
                                  * GEMMs) runs as in S3D_PREC_F16.  Same MFMA rate as S3D_PREC_F16, 8 significand bits
                                  * instead of 11: reported with its measured error (bench.py `throughput_mode_bf16`). */

int s3d_version(void);
const char* s3d_last_error(void);           /* thread-local, valid until the next failing call */

/* ---------------------------------------------------------------------------------------------
 * U-Net slice generator  — replaces UNet.forward (reg_slices/src/unet_custom.py:40-69) and the
 * DoubleConv/Up/OutConv blocks it calls (reg_slices/src/unet_parts.py:8-84), eval-mode BatchNorm.
 * ------------------------------------------------------------------------------------------- */

/* Raw parameters in the reference's own state_dict layout (PyTorch conv weight [Cout][Cin][kh][kw],
 * ConvTranspose2d weight [Cin][Cout][2][2]).  bn_* entries are {weight,bias,running_mean,running_var}. */
typedef struct {
    const float* w;      /* conv weight */
    const float* b;      /* conv bias or NULL */
    const float* bn[4];  /* BN following this conv (gamma, beta, mean, var) or all NULL */
} S3dConvParams;

typedef struct {
    S3dConvParams enc[13];        /* VGG16-BN convs down1.0 ... down5.40 with the BN that follows each
                                     (enc[12].bn = down5_.41 is unused by the forward and may be NULL) */
    S3dConvParams trans_c;        /* 1x1 (512+128)->512, bias            unet_custom.py:22 */
    S3dConvParams trans_up[4];    /* 1x1 skip projections trans_up1..4   unet_custom.py:24-30 */
    S3dConvParams up_t[4];        /* ConvTranspose2d 2x2 s2 of up1..4    unet_parts.py:53 */
    S3dConvParams up_c1[4];       /* DoubleConv conv0 + BN1 (no bias)    unet_parts.py:16-17 */
    S3dConvParams up_c2[4];       /* DoubleConv conv3 + BN4 (no bias)    unet_parts.py:19-20 */
    S3dConvParams outc;           /* 1x1 32->3 + tanh                    unet_parts.py:78-84 */
    const float* emds;            /* (n_slices,128) slice embeddings     unet_custom.py:32 */
    int n_slices;
} S3dUNetParams;

/* Bytes of the packed (MFMA-fragment-ordered, BN-folded) weight image for n_slices.  The image also keeps the pack's
 * own intermediates (the ConvT output behind up1's slice table, the fp32 composed ConvT -> 3x3 operators of up2 .. up4, about
 * 2.6 MB): a queued pack may read them after s3d_unet_pack returns, so they are not shared between stages. */
size_t s3d_unet_packed_bytes(int n_slices);
/* Repack raw parameters into `packed` (device, >= s3d_unet_packed_bytes).  Re-run after every
 * parameter update.  `params_host` is a HOST struct of DEVICE pointers. */
int s3d_unet_pack(const S3dUNetParams* params_host, void* packed, size_t packed_bytes, void* stream);

/* Feature pyramid handle: level l is (B*n_slices, H_l, W_l, C_l) NHWC fp32 with
 * C = {512,256,128,64,32}, H_l = S/16 * 2^l  (coarse -> fine).  Caller allocates. */
typedef struct {
    float* level[S3D_N_LEVELS];
    int n_img;                    /* B*n_slices */
    int size;                     /* S (input image side; levels are S/16 ... S) */
} S3dPyramid;

size_t s3d_unet_workspace_bytes(int batch, int size, int n_slices);
/* img (B,3,S,S) NCHW in [-1,1]  ->  pyramid (5 NHWC levels) and, if slices_rec != NULL, the
 * reconstructed slice images (B*n_slices,3,S,S) NCHW (tanh output, models.py:65-66).
 * S must be a multiple of 16. */
int s3d_unet_encode_fwd(const void* packed, const float* img, const S3dPyramid* out,
                        float* slices_rec, int batch, int size, int n_slices, int prec,
                        void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Per-query decoder — replaces Slices3DRegModel.forward lines models.py:53-84:
 * query rotation / flip, project_coord (models.py:28-36), 5x sample_from_planes (models.py:38-46,
 * 69-78), fc_p / fc_s (models.py:79-80), the 3-layer post-LN TransformerEncoder (models.py:18-19,83)
 * and fc_out (models.py:22-24,84).
 * ------------------------------------------------------------------------------------------- */
typedef struct {
    const float* in_proj_w;  const float* in_proj_b;    /* (384,128), (384) */
    const float* out_proj_w; const float* out_proj_b;   /* (128,128), (128) */
    const float* lin1_w;     const float* lin1_b;       /* (2048,128), (2048) */
    const float* lin2_w;     const float* lin2_b;       /* (128,2048), (128) */
    const float* norm1_w;    const float* norm1_b;      /* (128) */
    const float* norm2_w;    const float* norm2_b;      /* (128) */
} S3dLayerParams;

typedef struct {
    const float* fc_p_w;  const float* fc_p_b;          /* (128,3), (128)   models.py:20 */
    const float* fc_s_w;  const float* fc_s_b;          /* (128,992), (128) models.py:21 */
    S3dLayerParams layer[S3D_N_LAYERS];                 /* att_decoder.layers.{0,1,2} */
    const float* fc_out_w; const float* fc_out_b;       /* (1,128), (1)     models.py:22-24 */
} S3dHeadParams;

size_t s3d_head_packed_bytes(void);
int s3d_head_pack(const S3dHeadParams* params_host, void* packed, size_t packed_bytes, void* stream);

/* "Latent code" c of the ConvONet-style encode()/decode() split: the three coarse pyramid levels with
 * fc_s folded in (bilinear sampling and fc_s are both linear, so sampling the projected maps equals
 * projecting the sampled features; SURVEY.md section 7 "Sampler layout"), plus the two fine levels raw.
 * proj[l] is (n_img, H_l, W_l, 128) NHWC for l = 0,1,2. */
typedef struct {
    float* proj[3];
    const float* fine[2];         /* pyramid levels 3 and 4, (n_img,S/2,S/2,64), (n_img,S,S,32) */
    int n_img;
    int size;
} S3dLatent;

int s3d_latent_build(const void* head_packed, const S3dPyramid* pyr, const S3dLatent* out, int prec, void* stream);

/* Decode workspace.  The decoder walks the queries in passes; `s3d_decode_workspace_bytes` sizes the preferred pass
 * (<= 524 288 queries: 6.4 GB for any larger job — X 3.5 GB, the absorbed last layer's scratch 2.7 GB), and
 * `s3d_decode_workspace_bytes_min` the smallest one the library accepts (65 536 queries per pass: 0.8 GB).  A workspace between
 * the two makes the decode calls halve the pass until it fits (more launch tails, same results); below the minimum they
 * return S3D_E_WORKSPACE. */
size_t s3d_decode_workspace_bytes(int batch, long n_qry, int n_slices);
size_t s3d_decode_workspace_bytes_min(int batch, long n_qry, int n_slices);
/* 1 (default): everything on the caller's stream.  2 (or env S3D_DECODE_LANES=2): passes of >= 131 072 queries run their two
 * halves' layer chains on the caller's stream and on a library-owned side stream (created once per device, ordered behind
 * the caller's stream by events on both ends of every call), so one half's attention kernels share the CUs with the other
 * half's FFN kernels.  Same results bit for bit; measured time-neutral on MI355X (profiles/r05_lanes_ab.md), kept opt-in.
 * Thread safety: the setting is process-wide (an atomic).  The side stream and its two events are shared by every caller of a
 * device; a call holds that device's mutex from its fork to its join (host-side enqueue time only), so host threads may
 * decode concurrently on one device with different caller streams — their side-stream work is serialised, never interleaved.
 * The objects are created under the same mutex, all or nothing; when they cannot be created the call runs in its one-stream
 * form. */
int s3d_decode_set_lanes(int n);
/* 1 (default; env S3D_LAST_FUSED=0 turns it off): the token-0 attention block of the last encoder layer (models.py:83 consumes
 * nothing else) runs as ONE kernel in the split-precision modes (csrc/decode_last.hip: absorbed q GEMM, 13-row mixing step,
 * absorbed output GEMM + residual; only the token rows are read and the 512-byte u rows written).  0: the four-launch form of
 * rounds 2-5 (row copy, row GEMM, mixing kernel, row GEMM).  Same results bit for bit (every accumulator adds the same
 * products in the same order); the switch exists for the test that says so and for A/B timing.  S3D_PREC_F32 always runs the
 * four-launch form.  Process-wide (an atomic). */
int s3d_decode_set_last_fused(int on);
/* 1 (default; env S3D_SHARED_FOOTPRINT=0 turns it off): the token builder evaluates the three folded pyramid levels of a group of
 * 16 queries through the group's shared 4 x 4 pixel window on the fp32 MFMA whenever the group's bilinear footprints fit one
 * (csrc/decode.hip, sample_tokens_kernel) and per lane otherwise.  0: always per lane.  Same results bit for bit (the MFMA is a
 * k-ordered fmaf chain and the window visits a query's taps in the per-lane order); the switch exists for the test that says so
 * and for A/B timing.  Applies to the inference decode calls and to s3d_train_step.  Process-wide (an atomic). */
int s3d_decode_set_shared_footprint(int on);
/* qry (B,Q,3); rot (B,3,3) or NULL; trans (B,4,3) = trans_mat_wo_rot_tp; flip_yz != 0 selects the
 * mode='test' prologue (y,z negated, no rotation; models.py:53-56).  sdf_out (B,Q). */
int s3d_decode_points_fwd(const void* head_packed, const S3dLatent* latent, const float* qry,
                          const float* rot, const float* trans, int flip_yz, float* sdf_out,
                          int batch, long n_qry, int n_slices, int prec,
                          void* workspace, size_t workspace_bytes, void* stream);
/* Debug / test form of s3d_decode_points_fwd that also returns the intermediate rows the reference's stage probes look at
 * (fc_p / fc_s output models.py:79-82, token 0 after each layer of att_decoder models.py:83): stages holds
 * s3d_decode_stages_floats() floats = the token tensor [G][n_slices+1][16][128] (G = B*ceil(Q/16); row of query q of
 * object b: group b*ceil(Q/16) + q/16, lane q%16; token 0 = fc_p, token 1+s = fc_s of slice s), then [3][G*16][128] token-0
 * rows after layers 0, 1, 2, then [2][G][n_slices+1][16][128]: the whole token tensor after layer 0 and after layer 1 (every
 * token row the two full layers write, in the layout of the first block).  One pass in caller order: Q < 4096 per object. */
size_t s3d_decode_stages_floats(int batch, long n_qry, int n_slices);
int s3d_decode_points_stages_fwd(const void* head_packed, const S3dLatent* latent, const float* qry, const float* rot,
                                 const float* trans, int flip_yz, float* sdf_out, float* stages, int batch, long n_qry,
                                 int n_slices, int prec, void* workspace, size_t workspace_bytes, void* stream);

/* Dense-grid evaluation for Generator3D with upsampling_steps == 0 (reconstruct.py:135-146):
 * query coordinates box*linspace(-.5,.5,nx)^3 (x slowest, z fastest; common.py:145-164) are generated
 * in-kernel; logits_out[nx^3] = -sdf (reconstruct.py:97).  batch is 1. */
int s3d_decode_grid_fwd(const void* head_packed, const S3dLatent* latent, const float* trans,
                        int nx, float box, float* logits_out, int n_slices, int prec,
                        void* workspace, size_t workspace_bytes, void* stream);
/* A contiguous slab [q_begin, q_begin + q_count) of the same grid's linear index (x slowest, z fastest):
 * logits_out[q_count].  This is the query-parallel split of reconstruct.py:135-146 over N processes
 * (SURVEY.md 8(e)): every rank encodes the object itself and decodes 1/N of the grid; the host gathers.
 * Workspace: s3d_decode_workspace_bytes(1, q_count, n_slices). */
int s3d_decode_grid_slab_fwd(const void* head_packed, const S3dLatent* latent, const float* trans,
                             int nx, float box, long q_begin, long q_count, float* logits_out,
                             int n_slices, int prec, void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * VGG19 perceptual loss — replaces VGGPerceptualLoss.forward / VGG19Feats.forward
 * (reg_slices/src/vgg_perceptual_loss.py:29-70) as called at models.py:90-92.
 * Taps are what the reference actually compares: torchvision's in-place ReLU makes taps 1-4 post-ReLU,
 * tap 5 (conv5_2) pre-ReLU.  loss_out[0] = 0.001 * sum_i w_i * mean|x_i - y_i|.
 * ------------------------------------------------------------------------------------------- */
typedef struct {
    S3dConvParams conv[14];       /* vgg19.features convs 0,2,5,7,10,12,14,16,19,21,23,25,28,30 (bn NULL) */
    const float* mean;            /* (3) ImageNet mean buffer  vgg_perceptual_loss.py:47 */
    const float* std;             /* (3) */
} S3dVggParams;
size_t s3d_vgg_packed_bytes(void);
int s3d_vgg_pack(const S3dVggParams* params_host, void* packed, size_t packed_bytes, void* stream);
size_t s3d_vgg_workspace_bytes(int n_img, int size);
/* pred, target: (n_img,3,S,S) NCHW in [-1,1]; S multiple of 16. */
int s3d_vgg_loss_fwd(const void* packed, const float* pred, const float* target, int n_img, int size,
                     float* loss_out, void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Slices3DGTModel — reg_slices/src/model_gt.py:12-111 (regression from GIVEN slice images).
 * Same split as above: encoder once per object, folded latent maps, per-query decode.
 * ------------------------------------------------------------------------------------------- */
typedef struct {
    S3dConvParams conv[13];       /* img_encoder (vgg16bn_feats.py:26-40): VGG16-BN convs 0,3,7,10,14,17,20,24,27,30,
                                     34,37,40 each with the BatchNorm that follows it (conv[12].bn unused) */
} S3dVgg16BnParams;
typedef struct {
    float* level[5];              /* raw conv1_2, conv2_2, conv3_3, conv4_3, conv5_3 outputs, channels-last:
                                     (n_img, S>>l, S>>l, {64,128,256,512,512}[l]) */
    int n_img;                    /* B*n_slices */
    int size;
} S3dGtPyramid;
size_t s3d_gt_encoder_packed_bytes(void);
int s3d_gt_encoder_pack(const S3dVgg16BnParams* params_host, void* packed, size_t packed_bytes, void* stream);
size_t s3d_gt_encoder_workspace_bytes(int n_img, int size);
/* img_slices (n_img,3,S,S) NCHW = feed_dict['img_slices'].view(B*n_slices,3,S,S) (model_gt.py:73-76) */
int s3d_gt_encode_fwd(const void* packed, const float* img_slices, const S3dGtPyramid* out, int n_img, int size,
                      int prec, void* workspace, size_t workspace_bytes, void* stream);

typedef struct {
    const float* pts_w[3];  const float* pts_b[3];      /* pts_feat_extractor.{0,2,4}: (32,3) (64,32) (128,64) */
    const float* local_w[2]; const float* local_b[2];   /* fc_local.{0,2}: (128,1472) (128,128) */
    S3dLayerParams layer[S3D_N_LAYERS];                 /* att_decoder.layers.{0,1,2} */
    const float* fc_out_w; const float* fc_out_b;       /* fc_out.0 */
} S3dGtHeadParams;
size_t s3d_gt_head_packed_bytes(void);
int s3d_gt_head_pack(const S3dGtHeadParams* params_host, void* packed, size_t packed_bytes, void* stream);
/* proj[0..3]: conv5_3, conv4_3, conv3_3, conv2_2 levels with fc_local.0 folded in (n_img, W, W, 128);
 * fine: the raw conv1_2 level (must alias pyramid level 0). */
typedef struct {
    float* proj[4];
    const float* fine;
    int n_img;
    int size;
} S3dGtLatent;
int s3d_gt_latent_build(const void* head_packed, const S3dGtPyramid* pyr, const S3dGtLatent* out, int prec,
                        void* stream);
size_t s3d_gt_decode_workspace_bytes(int batch, long n_qry, int n_slices);
int s3d_gt_decode_points_fwd(const void* head_packed, const S3dGtLatent* latent, const float* qry,
                             const float* rot, const float* trans, int flip_yz, float* sdf_out, int batch,
                             long n_qry, int n_slices, int prec, void* workspace, size_t workspace_bytes,
                             void* stream);
int s3d_gt_decode_grid_fwd(const void* head_packed, const S3dGtLatent* latent, const float* trans, int nx,
                           float box, float* logits_out, int n_slices, int prec, void* workspace,
                           size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Latent-diffusion denoising U-Net primitives — gen_slices/ldm/modules/diffusionmodules/openaimodel.py
 * (BASELINE configs[4]).  The reference builds UNetModel from nn.Conv2d / GroupNorm32 / SiLU /
 * QKVAttentionLegacy / F.interpolate / avg_pool2d; the host mirror (slice3d_amd/ldm_unet.py) builds the same
 * module tree over these entry points.  All tensors channels-last fp32; C padded to a multiple of 16 where a
 * convolution reads it.
 * ------------------------------------------------------------------------------------------- */
/* nn.Conv2d(cin0+cin1, cout, ks, padding=ks/2) on cat([x0, x1], channel) (openaimodel.py:772 th.cat + conv), also
 * nn.Conv1d(k=1) over tokens (qkv / proj_out, :291,:299) and the ResBlock skip 1x1 (:240). */
size_t s3d_conv_packed_bytes(int cout, int cin0, int cin1, int ks);
int s3d_conv_pack(const float* w, const float* bias, int cout, int cin0, int cin1, int ks, void* packed,
                  size_t packed_bytes, void* stream);
/* prec (since version 110): S3D_PREC_F32 = exact fp32 MFMA; S3D_PREC_F16X3 = three f16 MFMAs per product (fp32-class);
 * S3D_PREC_F16 = the single-pass throughput mode (ONE f16 MFMA per product, operands rounded to f16 — not fp32-class; before
 * version 110 this value selected the exact fp32 path here).  Layers without an f16 weight image (channel counts that are not
 * multiples of 32: the stem) run the exact fp32 MFMA in every mode.  Any other value (S3D_PREC_BF16 included): S3D_E_ARG.
 * The pad channels of x0 / x1 (cin .. pad16(cin) - 1, here and in s3d_conv_strided_fwd) may hold any FINITE values: they meet
 * zero weights and leave every output bit unchanged (a NaN or Inf there poisons the output). */
int s3d_conv_fwd(const void* packed, const float* x0, const float* x1, const float* residual, float* out, int N,
                 int H, int W, int cout, int cin0, int cin1, int ks, int prec, void* workspace,
                 size_t workspace_bytes, void* stream);
/* GroupNorm32 -> [FiLM] -> [SiLU] -> Conv2d(3x3) as ONE operator (openaimodel.py:188-194 ResBlock.in_layers, :229-236
 * out_layers with use_scale_shift_norm): s3d_group_norm_table_fwd folds the statistics of cat([x0, x1]), gamma / beta and the
 * FiLM rows (film: (N, film_stride >= 2 (c0 + c1)) rows of scale | shift, or NULL) into a per-(image, channel) affine table
 * (N * 2 * (c0 + c1) floats: A | B of y = x * A + B; stats = s3d_group_norm_stats_floats(N, groups) floats of scratch);
 * s3d_conv_gn_fwd applies it (+ SiLU) while it stages its input tile — the normalised tensor is never written.  Served for
 * ks == 3, split precision (f16x3 / f16), cin0, cin1, cout multiples of 32, cin0 + cin1 <= 1536; other shapes are refused
 * with S3D_E_ARG (use s3d_group_norm_fwd + s3d_conv_fwd). */
size_t s3d_group_norm_stats_floats(int N, int groups);
/* 1 if s3d_conv_gn_fwd serves the shape (H, W <= 0: map size not known yet), else 0 — the single statement of the fused
 * operator's eligibility; on 0 run s3d_group_norm_fwd + s3d_conv_fwd. */
int s3d_conv_gn_supported(int cout, int cin0, int cin1, int ks, int prec, int H, int W, int has_workspace);
/* A convolution output whose split-K finish pass is deferred to its consumer (s3d_conv_gn_fwd with nsplit_out != NULL reported
 * nsplit > 1): the raw partial sums [nsplit][N*H*W][cout] sit in the convolution's workspace; `out` (N,H,W,cout) is written by
 * whoever consumes the descriptor — the next GroupNorm's statistics kernel (s3d_group_norm_table_fwd / s3d_group_norm_partial_fwd:
 * it sums the splits, adds the bias of `conv_packed` and `residual`, stores `out` and goes on with the values) or
 * s3d_conv_finish_fwd.  The descriptor is dead once the workspace is reused (the next split-K convolution). */
typedef struct {
    const float* part;
    int nsplit;
    const void* conv_packed;   /* the producing convolution's packed weights (holds its bias) */
    int cout, cin0, cin1, ks;
    const float* residual;     /* or NULL */
    float* out;
} S3dConvPartial;
int s3d_group_norm_table_fwd(const float* x0, int c0, const float* x1, int c1, const float* gamma, const float* beta,
                             const float* film, long film_stride, float* table, float* stats, int N, int HW, int groups,
                             float eps, const S3dConvPartial* x0_partial, void* stream);
int s3d_group_norm_partial_fwd(const S3dConvPartial* x0_partial, const float* gamma, const float* beta, const float* film,
                               long film_stride, float* y, float* stats, int N, int HW, int groups, float eps, int silu,
                               void* stream);
int s3d_conv_gn_fwd(const void* packed, const float* x0, const float* x1, const float* residual, float* out, int N, int H,
                    int W, int cout, int cin0, int cin1, int ks, int prec, const float* table, int silu, void* workspace,
                    size_t workspace_bytes, int* nsplit_out, void* stream);
int s3d_conv_finish_fwd(const S3dConvPartial* partial, int N, int H, int W, void* stream);
/* GroupNorm32 (util.py normalization) [+ FiLM: y*(1+scale)+shift, film = (N, 2C), openaimodel.py:268-270] [+ SiLU].
 * stats: s3d_group_norm_stats_floats(N, groups) floats of scratch (N*groups*192 since round 4; a smaller buffer is
 * overrun silently — size it with the function). */
int s3d_group_norm_fwd(const float* x, const float* gamma, const float* beta, const float* film, float* y,
                       float* stats, int N, int HW, int C, int groups, float eps, int silu, void* stream);
/* the same with film rows read in place from a wider tensor: image n's (scale | shift) at film + n * film_stride floats
 * (replaces ResBlock.emb_layers + the chunk of openaimodel.py:262-270 for a block whose emb_layers output is a column
 * range of one stacked GEMV over all blocks) */
int s3d_group_norm_film_fwd(const float* x, const float* gamma, const float* beta, const float* film, long film_stride,
                            float* y, float* stats, int N, int HW, int C, int groups, float eps, int silu, void* stream);
/* the same on th.cat([x0, x1], dim=1) (openaimodel.py:750, the skip connections of the output blocks) without
 * materialising the concatenation: x0 (N,HW,c0), x1 (N,HW,c1) -> y (N,HW,c0+c1); c0, c1 multiples of 4 */
int s3d_group_norm2_fwd(const float* x0, int c0, const float* x1, int c1, const float* gamma, const float* beta,
                        const float* film, float* y, float* stats, int N, int HW, int groups, float eps, int silu,
                        void* stream);
/* QKVAttentionLegacy.forward (openaimodel.py:362-377): qkv (N, T, heads*3*ch) -> out (N, T, heads*ch);
 * prec: S3D_PREC_F32 = fp32 MFMA, S3D_PREC_F16X3 = split-precision f16 MFMA (fp32-class accuracy) */
int s3d_qkv_attention_fwd(const float* qkv, float* out, int N, int T, int heads, int ch, int prec, void* stream);
/* The same operator for head widths 8 / 16 / 24 / 32 / 48 on the f16 MFMA with fp32-class logits (q, k split three ways,
 * p, v two ways; replaces the same reference lines, openaimodel.py:353-381).  ws: s3d_qkv_attention_ws_bytes() bytes of
 * scratch for the pre-split K / V block images (0 = width not served).  Width 48 (version 114): two 32-channel k-steps;
 * where N * heads * ceil(T / 64) workgroups would not fill the chip (1 024 tokens at batch 1) the keys are split over
 * 2 - 8 workgroups per query block and a merge launch adds their partial results (the scratch holds those as well). */
size_t s3d_qkv_attention_ws_bytes(int N, int T, int heads, int ch);
int s3d_qkv_attention_ws_fwd(const float* qkv, float* out, int N, int T, int heads, int ch, void* ws, size_t ws_bytes,
                             void* stream);
/* Upsample / Downsample with use_conv=False (openaimodel.py:108-158): up != 0: nearest 2x; else 2x2 average pool */
int s3d_resample2x_fwd(const float* x, float* y, int N, int H, int W, int C, int up, void* stream);
/* linear(SiLU?(x)): time_embed (:506-510) and ResBlock.emb_layers (:222-228); x (N,K), w (M,K) */
int s3d_small_linear_fwd(const float* x, const float* w, const float* b, float* out, int N, int K, int M,
                         int silu_in, void* stream);
/* timestep_embedding (util.py:151-170) */
int s3d_timestep_embedding_fwd(const float* t, float* out, int N, int dim, float max_period, void* stream);
/* out = a + b (c_fmaps injection, openaimodel.py:735-746) */
int s3d_add_fwd(const float* a, const float* b, float* out, long n, void* stream);
/* in (n,c,h,w) -> out (n,h,w,cpad), cpad >= c a multiple of 4; the pad channels c .. cpad are written as +0.0 */
int s3d_nchw_to_nhwc_pad(const float* in, float* out, int n, int c, int h, int w, int cpad, void* stream);
/* out (N,H,W,C) = a (N,H,W,C) + b (N,C,H,W): the same injection with the feature map taken as the reference hands it over (version 115) */
int s3d_add_nchw_fwd(const float* a, const float* b, float* out, int n, int c, int h, int w, void* stream);

/* ---------------------------------------------------------------------------------------------
 * First-stage AutoencoderKL (gen_slices/ldm/modules/diffusionmodules/model.py) and condition encoder ImageEncoderVGG16BN
 * (ldm/modules/encoders/modules.py:204-267) — version 116.  The other layers run on the U-Net primitives above.
 * ------------------------------------------------------------------------------------------- */
/* Strided Conv2d on the packed image of s3d_conv_pack (cin1 = 0): x (N,Hin,Win,pad16(cin)) -> out (N,Hout,Wout,cout);
 * input pixel = stride * out + tap - pad, zeros outside the input.  pad = ks / 2; pad_origin = 1 (ks 3, stride > 1):
 * pad 0 at the top / left — Downsample's F.pad(x, (0,1,0,1)) + Conv2d(3, stride 2) (model.py:60-79).  ks 1 with stride s:
 * a 1x1 convolution followed by a nearest s-fold downsize, computed on the picked pixels only (modules.py:262-266).
 * prec: S3D_PREC_F32 or S3D_PREC_F16X3. */
int s3d_conv_strided_fwd(const void* packed, const float* x, float* out, int N, int Hin, int Win, int Hout, int Wout, int cout,
                         int cin, int ks, int stride, int pad_origin, int prec, void* stream);
/* Which kernels a convolution call would launch, without launching them (version 123; no GPU needed): `buf` receives e.g.
 * "conv3x3_small_f16x3_kernel<2,true,9> grid=2x5 block=256 splits=5 finish=1; conv_splitk_finish_kernel grid=2x1 block=256" — the
 * kernel's name as a kernel trace prints it, its grid in workgroups, the split-K count and whether the finish pass follows.
 * Hin = Win = stride = 0: s3d_conv_fwd, or with fused_gn s3d_conv_gn_fwd (nsplit_out_requested: called with nsplit_out).
 * Otherwise s3d_conv_strided_fwd with (H, W) = (Hout, Wout) and cin0 = cin.  Returns 0, or the code the call would return
 * for these arguments (s3d_last_error says why).  The description follows S3D_CONV_SMALL / S3D_CONV_SMALL_1X1 as the calls do. */
int s3d_conv_plan_describe(int N, int H, int W, int cout, int cin0, int cin1, int ks, int prec, int fused_gn, size_t workspace_bytes,
                           int nsplit_out_requested, int Hin, int Win, int stride, int pad_origin, char* buf, size_t buf_len);
/* AttnBlock (model.py:150-202): one head of width C (64, 128, 256 or 512) over T >= 1 tokens, softmax(q k^T C^-0.5) v;
 * qkv (N, T, 3C) rows q | k | v -> out (N, T, C).  prec: S3D_PREC_F32 or S3D_PREC_F16X3 (both exact fp32 arithmetic). */
int s3d_wide_attention_fwd(const float* qkv, float* out, int N, int T, int C, int prec, void* stream);
/* ImageEncoderVGG16BN's input normalisation (modules.py:251-253): y = ((x + 1) / 2 - mean[c]) / std[c], x and y (n,c,h,w) */
int s3d_image_normalize_fwd(const float* x, const float* mean, const float* std, float* y, int n, int c, int h, int w,
                            void* stream);

/* ---------------------------------------------------------------------------------------------
 * Training step — replaces train_step (reg_slices/train.py:41-53): train-mode forward (batch-statistic
 * BatchNorm with the running-stat update, unet_parts.py:17,20), the three losses of cal_loss_pred
 * (train.py:29-39) + cal_acc (train.py:21-27), backward of everything, and Adam (train.py:136).
 * Gradients are written into caller-owned buffers laid out like the parameters: `unet_grad` / `head_grad`
 * are the same structs with every pointer replaced by the gradient buffer of that tensor (bn[0], bn[1] =
 * d gamma, d beta; bn[2], bn[3] ignored).  BatchNorm running_mean / running_var are updated IN PLACE
 * through unet->...bn[2], bn[3].  losses_out[4] = {L1(sdf), L1(slices), vgg_loss (x0.001), sign accuracy}.
 * The caller all-reduces the gradient buffers across ranks (data parallel) between this call and
 * s3d_adam_step.  dropout_p is nn.TransformerEncoderLayer's dropout (reference default 0.1); masks are
 * counter-based functions of (seed, site, element index), regenerated in the backward pass.
 * ------------------------------------------------------------------------------------------- */
/* Cross-rank BatchNorm statistics (train.py has no counterpart: the reference's nn.DataParallel replicas use
 * per-replica statistics, like torch DDP by default; `--sync_bn` is SURVEY.md 8(e)'s option).  The library computes
 * the per-rank partial statistics, calls all_reduce_sum on `n_floats` floats of `scratch` (device memory, >= 2048
 * floats, owned by the caller) on the call's stream, and continues with the reduced values: per BatchNorm layer two
 * small all-reduces in the forward (the means, then var_r + (mu_r - mu)^2: the count-weighted merge of
 * torch.nn.SyncBatchNorm, free of E[x^2] - mu^2 cancellation) and one in the backward: 42 + 21 per train step.  The callback must enqueue the collective so that later work
 * on `stream` sees its result (torch.distributed.all_reduce on the current stream does) and return 0. */
typedef int (*s3d_all_reduce_sum_fn)(void* user, float* device_buf, long n_floats, void* stream);
typedef struct {
    s3d_all_reduce_sum_fn all_reduce_sum;
    void* user;
    int world_size;
    float* scratch;
} S3dSyncBn;
typedef struct {
    const float* img;          /* (B,3,S,S)            img_input            */
    const float* img_slices;   /* (B,3*n_slices,S,S)   img_slices           */
    const float* qry;          /* (B,Q,3)              qry_norot            */
    const float* rot;          /* (B,3,3)              obj_rot_mat          */
    const float* trans;        /* (B,4,3)              trans_mat_wo_rot_tp  */
    const float* sdf;          /* (B,Q)                sdf                  */
    /* Optional hipEvent_t handles (NULL = none), recorded on the call's stream the moment a BUCKET of parameter
     * gradients is final, in the order the backward finishes them, so a data-parallel host can all-reduce bucket k on
     * another stream while the rest of the backward runs (replaces the backward-hook bucketing of
     * torch DDP for train.py:131-132).  [0] transformer decoder + fc_p / fc_s / fc_out; [1] the U-Net's decoder
     * half (trans_c, up*, trans_up*, outc, emds); [2] encoder convs 7..12 + their BatchNorms (13 of the encoder's
     * 14.7 M parameters); the rest (encoder convs 0..6) is final when the call's work is. */
    void* ev_grad_ready[3];
    const S3dSyncBn* sync_bn;  /* NULL: per-rank BatchNorm statistics */
} S3dTrainBatch;
size_t s3d_train_workspace_bytes(int batch, int size, long n_qry, int n_slices);
/* Reproducibility (version 113): with n_qry >= 4096 (the locality-sorted token order) and size <= 256 the step contains no float
 * atomics — the pyramid-sampling backward writes per-tile partial sums into the workspace and adds them in a fixed order
 * (train_sbd.hip) — so the same inputs, seed and weights give bit-identical losses and gradients, call after call.  Smaller query
 * counts / larger images keep the atomic scatter kernels (gradients equal to fp32 summation-order noise).  The workspace holds
 * 29 824 floats (119 KB) of partial sums per (object, slice, 16 x 16-bin image tile) at size 256: 1.47 GB at 4 objects x 12 slices.
 * prec: S3D_PREC_F32 (exact fp32 MFMAs), S3D_PREC_F16X3 (split precision, fp32-class: the mode every parity test and the
 * reported train_samples_per_s use) or — since version 112 — S3D_PREC_F16: a THROUGHPUT mode in which the decoder's GEMM kernels
 * (FFN forward / data pass / both weight-gradient contractions, the fused attention forward and backward, the row-linear layers and
 * their weight gradients) run ONE f16 MFMA per product; the U-Net, VGG, the samplers, every reduction, the fp32 master weights,
 * fp32 accumulation and the power-of-two backward scale are those of S3D_PREC_F16X3.  Not fp32-class (gradients deviate by ~1e-2
 * relative from the split-precision step): bench.py reports it beside the headline as train_throughput_mode_f16. */
int s3d_train_fwd_bwd(const S3dUNetParams* unet, const S3dHeadParams* head, const S3dVggParams* vgg,
                      const S3dUNetParams* unet_grad, const S3dHeadParams* head_grad,
                      const S3dTrainBatch* batch, int batch_size, int size, long n_qry, int n_slices,
                      float dropout_p, unsigned long long seed, int prec, float* losses_out, float* sdf_pred_out,
                      float* slices_rec_out, void* workspace, size_t workspace_bytes, void* stream);
/* The same step as two calls, for a host that owns the loss — the reference's contract `x = model(batch);
 * loss(x).backward(); opt.step()` (train.py:41-53) behind a torch.autograd.Function:
 *   s3d_train_fwd : train-mode forward (batch-statistics BatchNorm with running-stat updates, dropout from `seed`);
 *                   outputs sdf_pred (B,Q), slices_rec (B*n_slices,3,S,S), vgg_loss (device scalar, already x0.001 as
 *                   models.py:92); every activation the backward needs stays in `workspace`.
 *   s3d_train_bwd : from d loss/d sdf_pred, d loss/d slices_rec (device, either may be NULL = zero) and
 *                   d loss/d vgg_loss (host scalar) to the parameter gradients (written, not accumulated).  Same
 *                   dims / dropout_p / seed / prec / workspace as the forward; slices_rec = the forward's output.
 *                   grad_scale: power of two applied to the incoming gradients inside the split-precision (f16x3)
 *                   backward and removed from the results; 0 selects 2^k ~ 8*B*Q, right for mean-reduced losses. */
int s3d_train_fwd(const S3dUNetParams* unet, const S3dHeadParams* head, const S3dVggParams* vgg,
                  const S3dTrainBatch* batch, int batch_size, int size, long n_qry, int n_slices, float dropout_p,
                  unsigned long long seed, int prec, float* vgg_loss_out, float* sdf_pred_out, float* slices_rec_out,
                  void* workspace, size_t workspace_bytes, void* stream);
int s3d_train_bwd(const S3dUNetParams* unet, const S3dHeadParams* head, const S3dVggParams* vgg,
                  const S3dUNetParams* unet_grad, const S3dHeadParams* head_grad, const S3dTrainBatch* batch,
                  int batch_size, int size, long n_qry, int n_slices, float dropout_p, unsigned long long seed,
                  int prec, const float* d_sdf_pred, const float* d_slices_rec, float d_vgg_loss, float grad_scale,
                  float* slices_rec, void* workspace, size_t workspace_bytes, void* stream);
/* Slices3DGTModel training step — reg_slices/train_gt.py:38-52 (train_step: zero_grad, model(batch), L1 on the
 * sdf, backward) without opt.step (s3d_adam_step).  Train-mode forward of model_gt.py:59-111: batch-statistics
 * BatchNorm in the VGG16-BN encoder over the B*n_slices slice images (running statistics updated in place through
 * enc->conv[i].bn[2..3], including conv[12]'s, whose output the model never uses), dropout p in the transformer.
 * batch->img is ignored (model_gt.py:75-76 concatenates it and drops the result).  Gradients are written to the
 * tensors of enc_grad / head_grad (same shapes as the parameters; conv[12].bn, the classifier and the unused
 * att_layer / fc_global never receive one, as in the reference).  losses_out[0] = L1(sdf_pred, sdf),
 * losses_out[1] = sign accuracy (train_gt.py:21-26).  sdf_pred_out (B,Q) optional. */
size_t s3d_gt_train_workspace_bytes(int batch, int size, long n_qry, int n_slices);
int s3d_gt_train_fwd_bwd(const S3dVgg16BnParams* enc, const S3dGtHeadParams* head,
                         const S3dVgg16BnParams* enc_grad, const S3dGtHeadParams* head_grad,
                         const S3dTrainBatch* batch, int batch_size, int size, long n_qry, int n_slices,
                         float dropout_p, unsigned long long seed, int prec, float* losses_out, float* sdf_pred_out,
                         void* workspace, size_t workspace_bytes, void* stream);
/* The same Adam update for n_tensors parameters in one call (one kernel launch per 128 tensors).  params, offsets,
 * sizes: HOST arrays; tensor i takes its gradient from grad_flat[offsets[i] .. + sizes[i]) and keeps its moments at the
 * same range of exp_avg_flat / exp_avg_sq_flat (all three flat arrays on the device). */
int s3d_adam_step_multi(float* const* params, const long* offsets, const long* sizes, int n_tensors,
                        const float* grad_flat, float* exp_avg_flat, float* exp_avg_sq_flat, float lr, float beta1,
                        float beta2, float eps, int step, void* stream);
/* The dropout mask the kernels use: out[i] = keep(seed, site, idx0+i) ? 1/(1-p) : 0.  site = 4*layer +
 * {0 attention probabilities [(row*4 + head)*16 + key], 1 attention-block output [row*128 + c],
 *  2 FFN hidden [row*2048 + unit], 3 FFN output [row*128 + c]}; rows index the token tensor
 * [group][token][16 queries]; all four sites of the LAST layer index its compact token-0 rows [group][16 queries]
 * (only token 0 of that layer is computed). */
int s3d_dropout_mask(unsigned long long seed, int site, unsigned long long idx0, long n, float p, float* out,
                     void* stream);
/* torch.optim.Adam defaults semantics (no weight decay, no amsgrad); step counts from 1. */
int s3d_adam_step(float* p, const float* g, float* m, float* v, long n, float lr, float beta1, float beta2,
                  float eps, int step, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Measurement hook (no reference counterpart): when enabled, the launches of each kernel family are
 * bracketed with hipEvents on the caller's stream; s3d_prof_read waits for them and returns the summed
 * duration and the number of launches since s3d_prof_enable(1).  bench.py uses it to time the
 * dominant kernel inside its timed region.
 * ------------------------------------------------------------------------------------------- */
#define S3D_PROF_UNET 0          /* whole s3d_unet_encode_fwd */
#define S3D_PROF_LATENT 1        /* s3d_latent_build */
#define S3D_PROF_SAMPLE 2        /* sample_tokens_kernel */
#define S3D_PROF_ATTN 3          /* attn_layer_kernel (all layers) */
#define S3D_PROF_FFN 4           /* ffn_layer_kernel, full-row layers */
#define S3D_PROF_FFN_FINAL 5     /* ffn_layer_kernel, token-0 rows of the last layer (+fc_out) */
#define S3D_PROF_VGG 6           /* whole s3d_vgg_loss_fwd */
#define S3D_PROF_SAMPLE_PYR 7    /* sample_pyramid_kernel of s3d_sample_pyramid_fwd (without the locality sort) */
#define S3D_PROF_N 8
int s3d_prof_enable(int on);
int s3d_prof_read(int id, double* total_ms, long* count);
/* Trace ranges (tracing; no reference counterpart): the library brackets its stages and the phases of
 * the train step with roctx ranges ("s3d:...") that `rocprofv3 --marker-trace` records; the host side opens its own ranges
 * (the gradient exchange of trainer.py) through the same roctx library with these two calls.  No-ops (return 0) when no
 * roctx library can be loaded. */
int s3d_range_push(const char* name);
int s3d_range_pop(void);

/* ---------------------------------------------------------------------------------------------
 * Stand-alone ops of the module's helper API
 * ------------------------------------------------------------------------------------------- */
/* project_coord (models.py:28-36): coords (B,Q,3), trans (B,4,3) -> out (B,Q,2) */
int s3d_project_coord_fwd(const float* coords, const float* trans, float* out, int batch, long n_qry,
                          void* stream);
/* Image-space locality order of the queries (no reference counterpart: an execution-order choice of this
 * library, exposed so hosts / tests can map token-tensor rows back to queries).  Queries of each batch item are
 * projected exactly like models.py:28-36 (after models.py:53-60's flip / rotation), binned at 256^2 and ordered by
 * the Morton code of the bin, ascending query index inside a bin: perm_out[b*Q + slot] = query index.
 * Deterministic.  The decoder and the train step use this order internally for Q >= 4096. */
size_t s3d_query_sort_workspace_bytes(int batch, long n_qry);
int s3d_query_sort(const float* qry, const float* rot, const float* trans, int flip_yz, int batch, long n_qry,
                   int* perm_out, void* workspace, size_t workspace_bytes, void* stream);
/* sample_from_planes (models.py:38-46) on a channels-last plane: plane (N,H,W,C), grid (N,M,2)
 * -> out (N,M,C); bilinear, zeros padding, align_corners=True.  C % 4 == 0. */
int s3d_sample_planes_fwd(const float* plane, const float* grid, float* out, int n, int h, int w,
                          int c, long m, void* stream);
/* The reference's feature-sampling block as ONE op (models.py:63-73: five sample_from_planes calls over
 * feat_list + torch.cat(dim=2)): pyr = channels-last pyramid of B*n_slices images, grid (B,Q,2) projected
 * coordinates shared by the n_slices images of a batch item -> out (B*n_slices, Q, 992) fp32, channel order
 * [512 | 256 | 128 | 64 | 32].  HBM-bound on the 3 968-byte row writes (SURVEY.md 8(d) "stand-alone
 * feature-sample kernel").  workspace: s3d_sample_pyramid_workspace_bytes (point records + the locality order
 * the points are visited in for Q >= 4096; results do not depend on the order). */
size_t s3d_sample_pyramid_workspace_bytes(int batch, long n_qry);
int s3d_sample_pyramid_fwd(const S3dPyramid* pyr, const float* grid, float* out, int batch, int n_slices,
                           long n_qry, void* workspace, size_t workspace_bytes, void* stream);
/* layout helpers: (N,C,H,W) <-> (N,H,W,C) */
int s3d_nchw_to_nhwc(const float* in, float* out, int n, int c, int h, int w, void* stream);
int s3d_nhwc_to_nchw(const float* in, float* out, int n, int c, int h, int w, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Mesh extraction on the device — the step right after the hot path in
 * Generator3D.generate_from_latent / extract_mesh (reg_slices/reconstruct.py:148-243).
 *
 * MISE: replaces reg_slices/src_convonet/utils/libmise/mise.pyx:33-368 (MISE.query / update / to_dense).
 * The octree lives in a caller-owned device workspace; a round's points are returned as ascending linear
 * grid indices ((r*x + y)*r + z, r = resolution + 1) in a device buffer and never visit the host.  Same
 * point SET per round and same dense grid as the reference (its order within a round is insertion order).
 * The handle is a small host descriptor; s3d_mise_dev_query / _update synchronise the stream once each
 * (round count / error flag).  Host-side twin (bit-exact order): include/slice3d_mesh.h.
 * ------------------------------------------------------------------------------------------- */
/* 0 for parameters the unit does not serve: resolution0 < 1, depth outside 0..12, or a grid whose (resolution + 1)^3
 * points do not fit the int indices used throughout (resolution = resolution0 << depth <= 1289; 1290^3 is the largest
 * cube below 2^31).  s3d_mise_dev_create refuses the same parameters. */
size_t s3d_mise_dev_workspace_bytes(int resolution0, int depth);
void* s3d_mise_dev_create(void* workspace, size_t workspace_bytes, int resolution0, int depth,
                          double threshold, void* stream);            /* NULL on error (s3d_last_error) */
void s3d_mise_dev_destroy(void* handle);
int s3d_mise_dev_resolution(void* handle);                            /* resolution0 << depth */
/* unknown points of the next round -> idx_out[min(*n_out, capacity)] (device), *n_out (host) */
int s3d_mise_dev_query(void* handle, int* idx_out, long capacity, long* n_out, void* stream);
/* their coordinates as reconstruct.py:160-161 forms them in float32: box*(p/resolution - 0.5) -> qry_out (n,3) */
int s3d_mise_dev_points(void* handle, const int* idx, long n, float box, float* qry_out, void* stream);
/* mise.update(points, values) + one refinement step; values = the logits of the points (device).  Every index is checked
 * first: one that is negative, >= (resolution + 1)^3 or names a lattice point the octree has not created yet makes the
 * call return S3D_E_ARG with the octree unchanged (no value stored, no refinement step). */
int s3d_mise_dev_update(void* handle, const int* idx, const float* values, long n, void* stream);
int s3d_mise_dev_update_f64(void* handle, const int* idx, const double* values, long n, void* stream);
/* mise.to_dense(): (r,r,r) float64, unknown entries forward-filled along x, then y, then z */
int s3d_mise_dev_to_dense(void* handle, double* out, void* stream);

/* Marching cubes: replaces libmcubes.marching_cubes (libmcubes/pywrapper.cpp:90-127 driving
 * marchingcubes.h:23-193) as classify -> scan -> emit.  Vertices and faces are bit-identical to the
 * reference's and in its order.  grid: device (nx,ny,nz) float32 (is_f64 = 0) or float64, C order; pad != 0
 * evaluates the grid as if np.pad(grid, 1, constant_values=pad_value) had been applied (reconstruct.py:189)
 * without materialising it.  Pass 1 returns the counts (one stream synchronisation), pass 2 — same arguments —
 * fills vertices (V,3) float64 in index units + 0.5 of the padded grid (libmcubes' convention, undone by the
 * caller: reconstruct.py:199-201) and triangles (F,3) int64, both device buffers. */
size_t s3d_mc_dev_workspace_bytes(int nx, int ny, int nz, int pad);
int s3d_mc_dev_count(const void* grid, int is_f64, int nx, int ny, int nz, int pad, double pad_value, double iso,
                     void* workspace, size_t workspace_bytes, long* n_vertices, long* n_triangles, void* stream);
int s3d_mc_dev_emit(const void* grid, int is_f64, int nx, int ny, int nz, int pad, double pad_value, double iso,
                    void* workspace, size_t workspace_bytes, double* vertices, long long* triangles, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Mesh evaluation — the scores of reg_slices/src/utils_eval.py:1-109 on the device.
 * Meshes enter as s3d_mc_dev_emit leaves them: vertices (V,3) float64, faces (F,3) int64, device buffers.
 * ------------------------------------------------------------------------------------------- */
/* Point-in-mesh: replaces check_mesh_contains (src_convonet/utils/libmesh/inside_mesh.py:5-139) and its compiled cell
 * hash (libmesh/triangle_hash.pyx:10-88), bit for bit.  float64 throughout: the bbox of the vertices the faces
 * reference, scale = (res-1)/(bmax-bmin), translate = 0.5 - scale*bmin, every coordinate scale*x + translate (float32
 * points widened first); each triangle is listed in every cell res*x + y of its (int)-truncated xy box clamped to
 * [0, res-1]; a point outside [0, res]^3, or whose (int) x or y is res, is outside; otherwise it counts the triangles of
 * its cell that pass the strict 2-D test (det == 0 skipped) at depth >= pz*|n_z| and at depth < pz*|n_z| (|n_z| == 0:
 * neither) and is inside when both counts are odd.  A mesh whose bbox is flat on an axis (or that has no face) contains
 * no point, as the reference's inf / NaN rescale amounts to.
 * Three calls on one workspace (res = hash_resolution, 2..8192):
 *   build: bbox, rescale, cell counts and offsets; returns the entry count (64-bit) through one stream synchronisation.
 *          S3D_E_ARG when a face indexes a vertex outside [0, n_vertices).
 *   fill:  the cell lists into entries[n_entries] (int32 face indices, caller-owned).
 *   query: inside[n_points] (uint8 0/1) for points (n,3) float32 (is_f64 = 0) or float64; n_disagree (optional, one
 *          uint64) = the points inside the bbox whose two parities differ (the reference prints a warning for them).
 *          Any number of queries may follow one build + fill. */
size_t s3d_mesh_contains_workspace_bytes(long n_faces, int hash_resolution);
int s3d_mesh_contains_build(const double* vertices, long n_vertices, const long long* faces, long n_faces,
                            int hash_resolution, void* workspace, size_t workspace_bytes, long* n_entries, void* stream);
int s3d_mesh_contains_fill(long n_faces, int hash_resolution, void* workspace, size_t workspace_bytes, int* entries,
                           long n_entries, void* stream);
int s3d_mesh_contains_query(long n_faces, int hash_resolution, const void* workspace, size_t workspace_bytes,
                            const int* entries, long n_entries, const void* points, int is_f64, long n_points,
                            unsigned char* inside, unsigned long long* n_disagree, void* stream);
/* Exact nearest neighbour (what utils_eval.points_dist gets from cKDTree.query, k = 1): d2[i] = min_j |a_i - b_j|^2 in
 * fp32 from coordinate differences (dx*dx + dy*dy + dz*dz, no MFMA, no |a|^2 - 2a.b + |b|^2 expansion), idx[i] = its j
 * (optional, NULL to skip), the lowest j on ties.  a (na,3), b (nb,3) float32.  nb == 0: S3D_E_ARG; na == 0 launches
 * nothing.  workspace: s3d_nn_workspace_bytes(na). */
size_t s3d_nn_workspace_bytes(long na);
int s3d_nn_sqdist(const float* a, long na, const float* b, long nb, void* workspace, size_t workspace_bytes, float* d2,
                  long long* idx, void* stream);
/* Area-weighted surface sampling: float64 face areas, their inclusive prefix sum, sample i takes the first face whose
 * cdf > u*total and the point (1-sqrt(r1))*A + sqrt(r1)*(1-r2)*B + sqrt(r1)*r2*C, with u, r1, r2 hashed from (seed, i)
 * (independent of the launch geometry).  Zero-area faces are never chosen.  -> points (n,3) float32, face_idx (n)
 * int64; a mesh of zero total area gives NaN points and face -1.  workspace: s3d_surface_sample_workspace_bytes. */
size_t s3d_surface_sample_workspace_bytes(long n_faces);
int s3d_surface_sample(const double* vertices, long n_vertices, const long long* faces, long n_faces, long n_samples,
                       unsigned long long seed, void* workspace, size_t workspace_bytes, float* points,
                       long long* face_idx, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Signed-distance targets from a mesh (csrc/mesh_sdf.hip) — what 02_sdfs/<shape>.npy is made from.  No counterpart in the
 * reference's tree (its README:49 names an external script; reg_slices/src/datasets.py:142-148 is the consumer that fixes
 * the file format).  Same conventions as the mesh evaluation above: vertices (V,3) float64 and faces (F,3) int64 device
 * buffers, points (n,3) float32 (is_f64 = 0) or float64, caller-owned workspace, nothing allocated or kept by the library;
 * S3D_E_ARG with a message when a face indexes a vertex outside [0, n_vertices).
 * ------------------------------------------------------------------------------------------- */
/* Exact unsigned distance: dist[i] = min over ALL faces of the distance from point i to the triangle, float64 (float32
 * points widened first).  A zero-area face is the segment or point it degenerates to: never NaN, never skipped.
 *   build: a grid of resolution^3 cells (1..256 per axis; one cell on an axis where the box is flat) over the bounding box
 *          of the vertices the faces reference; every triangle is counted in every cell its box overlaps; offsets by a
 *          scan; per cell the Chebyshev distance to the nearest occupied cell.  Returns the entry count (64-bit) through
 *          one stream synchronisation.  n_faces == 0: S3D_E_ARG.
 *   fill:  the cell lists into entries[n_entries] (int32 face indices, caller-owned).
 *   query: cells are visited in shells of growing Chebyshev radius around the point's clamped cell, from the first shell
 *          that holds an occupied cell, until the lower bound of everything beyond the last shell exceeds the best
 *          distance; points outside the grid, however far, are legal and exact.  Every loop is bounded by the grid size.
 *          dist (n) float64; face (n) int64 (optional, NULL to skip): the face that attains it; n_tests (optional, one
 *          uint64): the point-triangle tests performed.  n_points == 0 launches nothing.  Any number of queries may
 *          follow one build + fill.
 * Determinism: a face's squared distance to a point is one fixed operation sequence; dist is the square root of the
 * minimum of those values and face the lowest index among the faces that attain it bit for bit — the same bits from run to
 * run, for every resolution, and for float32 points and their widened copies.  No atomics touch the result. */
size_t s3d_mesh_dist_workspace_bytes(long n_faces, int resolution);
int s3d_mesh_dist_build(const double* vertices, long n_vertices, const long long* faces, long n_faces, int resolution,
                        void* workspace, size_t workspace_bytes, long* n_entries, void* stream);
int s3d_mesh_dist_fill(long n_faces, int resolution, void* workspace, size_t workspace_bytes, int* entries,
                       long n_entries, void* stream);
int s3d_mesh_dist_query(long n_faces, int resolution, const void* workspace, size_t workspace_bytes, const int* entries,
                        long n_entries, const void* points, int is_f64, long n_points, double* dist, long long* face,
                        unsigned long long* n_tests, void* stream);
/* Generalised winding number: w[i] = sum over faces of Omega_f(p_i) / 4 pi, Omega_f = 2 atan2(det[a b c], |a||b||c| +
 * (a.b)|c| + (b.c)|a| + (c.a)|b|) with a, b, c the face's vertices relative to the point (Van Oosterom & Strackee),
 * float64.  +1 inside a closed mesh whose faces are counter-clockwise seen from outside, 0 outside, in between near a
 * hole.  A point on a face's plane inside the face gets that face's limit value as the formula gives it (+-2 pi or 0), a
 * point on a vertex 0 from the faces around it; no NaN.  Faces are summed in fixed chunks (a function of n_faces alone) in
 * face order and the chunk sums in chunk order, so w is bit-reproducible whatever n_splits — the number of blocks the
 * chunks are dealt to (0: chosen from n_points so that few points still fill the chip).  The faces are validated by a
 * kernel of their own (one stream synchronisation) before anything dereferences them.  n_faces == 0: S3D_E_ARG;
 * n_points == 0 launches nothing.  workspace: s3d_mesh_winding_workspace_bytes(n_faces, n_points). */
size_t s3d_mesh_winding_workspace_bytes(long n_faces, long n_points);
int s3d_mesh_winding(const double* vertices, long n_vertices, const long long* faces, long n_faces, const void* points,
                     int is_f64, long n_points, int n_splits, void* workspace, size_t workspace_bytes, double* w,
                     void* stream);

/* ---------------------------------------------------------------------------------------------
 * Rendering a mesh into the dataset's images (mesh_render.hip; slice3d_amd/mesh_render.py, render_slices/gen_dataset.py):
 * the RGBA input view and the RGBA images of the 12 slabs (four per axis) that the reference renders with Blender
 * (render_slices/blender_script_input.py, blender_script_slices.py).  One camera per call.  Mesh conventions as above.
 *
 * camera: 26 float64 on the HOST: R (3x3, row-major), distance, scale, t[3], M (3x4, row-major).  A vertex v becomes
 * c = (v * scale + t) R (x right, y down, z away from the camera) and p = c + (0, 0, distance); the pinhole has focal
 * length 35/32 image widths, pixel row 0 at the top.  Each pixel holds samples x samples rays (samples = 1, 2 or 4)
 * d = ((u - 0.5) / f, (v - 0.5) / f, 1), u = (i + (a + 0.5) / samples) / size.  A ray hits the face (a, b, c) iff its normal
 * n = (b - a) x (c - a) is not zero, d.(b x c), d.(c x a), d.(a x b) are all >= 0 or all <= 0 and not all zero, and
 * s = (a.n) / (d.n) > 0; the nearest hit has the smallest s, the lowest face index on equal s.  The hit point
 * P = s d - (0, 0, distance) has slab coordinates M [P, 1]; per axis the slab index is the count of i in {1, 2, 3} with
 * coordinate >= lo + (hi - lo) / 4 * i, lo / hi over the vertices the faces reference (0 where hi == lo).  Image 0 is the
 * nearest hit, images 1 + 4 axis + k the nearest hit among the hits of slab k of the axis: the hollow surface inside it.
 *   build:  transforms, slab bounds, the conservative range of pixel tiles of every face (a face with a vertex at
 *           p_z <= 0 goes to every tile), entries per tile and their scan.  Returns the entry count through one stream
 *           synchronisation.  S3D_E_ARG for size outside 1..1024, samples not in {1, 2, 4}, tile < 1 or tile * samples > 32.
 *   fill:   the tile lists into entries[n_entries] (int32 face indices, caller-owned).
 *   render: one workgroup per tile, one thread per sample; face (13, size * samples, size * samples) int32, -1 = miss;
 *           depth (same shape, float64 s, +inf = miss; optional); rgba (13, size, size, 4) uint8 (optional): alpha =
 *           round(255 * covered / samples^2), straight; rgb = round(255 * mean over the covered samples of albedo *
 *           (0.5 + 0.5 |n.d| / (|n| |d|))), albedo 0.8 or, on image 0 with vertex_colors (V, 3) float64, the mean of the
 *           face's three vertex colours; (0, 0, 0, 0) where nothing is covered.  n_tests (optional, one uint64): ray-face
 *           tests performed.
 * `tile` (pixels per tile edge) changes the speed only: every output is the same bits for every value, and from run to run.
 * ------------------------------------------------------------------------------------------- */
size_t s3d_mesh_render_workspace_bytes(long n_vertices, long n_faces, int size, int samples, int tile);
int s3d_mesh_render_build(const double* vertices, long n_vertices, const long long* faces, long n_faces,
                          const double* camera, int size, int samples, int tile, void* workspace, size_t workspace_bytes,
                          long* n_entries, void* stream);
int s3d_mesh_render_fill(long n_vertices, long n_faces, int size, int samples, int tile, void* workspace,
                         size_t workspace_bytes, int* entries, long n_entries, void* stream);
int s3d_mesh_render_render(long n_vertices, const long long* faces, long n_faces, int size, int samples, int tile,
                           const void* workspace, size_t workspace_bytes, const int* entries, long n_entries,
                           const double* vertex_colors, double* depth, int* face, unsigned char* rgba,
                           unsigned long long* n_tests, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Mesh simplification (mesh_simplify.hip; slice3d_amd/mesh_simplify.py, reg_slices/simplify_meshes.py): quadric
 * edge collapse with the parameters of the reference's libsimplify (src_convonet/utils/libsimplify/Simplify.h), in
 * rounds of independent collapses.  Mesh conventions as above; quadrics, costs and positions are float64.
 *
 * A pass: vertex -> face lists ordered by face index; face normals; in the first pass the vertex quadrics (afterwards a
 * collapse adds the removed vertex's quadric to the kept one); border flags (a vertex with an edge that has exactly one
 * face); per undirected edge the reference's cost and target (the quadric minimiser when the 3x3 system is regular and
 * the endpoints are no border vertices, else the best of the endpoints and the midpoint).  An edge is a candidate when
 * its cost <= 1e-9 (k + 3)^aggressiveness, both endpoints carry the same border flag, no face around either endpoint
 * would flip or degenerate (the reference's `flipped`, against the faces' current normals) and the link condition holds
 * (a vertex next to both endpoints is an apex of a face on the edge: two apexes for an interior edge, one for a border
 * edge; no two surviving faces would coincide; no interior edge between two border vertices).  Every candidate writes a
 * 64-bit key (the cost's sign, exponent and two mantissa bits | a bijective mix of the edge id) by integer atomicMin into
 * all vertices of the faces around its endpoints and wins if it still holds the minimum at both endpoints; winners touch
 * disjoint faces.  All winners are applied, or, when they would pass the target, the cheapest ones that reach it, so
 * n_faces_out is target_faces or one below it (an interior collapse removes two faces) unless the rounds run out first.
 * A round is four passes at one k, then the compaction of the face list and the read-back of the live count; k starts
 * at 0 and advances after a round that removed under 1/8 of the faces; at most 100 rounds, the reference's bound.
 * Closed oriented manifold in -> closed oriented manifold of the same genus out.  The output is the same bits from run
 * to run: no float atomics, every float64 sum in one fixed order.
 *   run:  validates the indices with a kernel of its own before anything dereferences them (S3D_E_ARG with a message
 *         for an index outside [0, n_vertices)), simplifies inside the workspace and returns the counts.  One stream
 *         synchronisation per round.  S3D_E_ARG with a message for n_faces == 0, target_faces < 0 or a workspace below
 *         s3d_mesh_simplify_workspace_bytes(n_vertices, n_faces).  target_faces >= n_faces runs no round: the faces
 *         come back as they are.  Faces that name a vertex twice are dropped before the first round.
 *   emit: vertices_out (n_vertices_out, 3): the vertices still referenced, in ascending original index; faces_out
 *         (n_faces_out, 3) in ascending original face index.  n_vertices / n_faces are the INPUT sizes, as in run.
 * workspace_bytes returns 0 for sizes it cannot serve (n_faces < 1 or >= 2^29, n_vertices < 1 or >= 2^31).
 * ------------------------------------------------------------------------------------------- */
size_t s3d_mesh_simplify_workspace_bytes(long n_vertices, long n_faces);
int s3d_mesh_simplify_run(const double* vertices, long n_vertices, const long long* faces, long n_faces,
                          long target_faces, double aggressiveness, void* workspace, size_t workspace_bytes,
                          long* n_vertices_out, long* n_faces_out, int* n_rounds, void* stream);
int s3d_mesh_simplify_emit(const void* workspace, size_t workspace_bytes, long n_vertices, long n_faces,
                           double* vertices_out, long long* faces_out, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Mesh topology (mesh_topology.hip; slice3d_amd/mesh_topology.py, reg_slices/clean_meshes.py): weld of equal positions,
 * connected components, per-component counts and measures, order-preserving removal of components.  Mesh conventions
 * as above.  `weld` (0 / 1) is part of the workspace's layout: pass the same value to every call on one workspace.
 *
 * Weld: two vertices that faces reference are one when their three coordinates compare equal as doubles (-0.0 equals
 * +0.0, 1 ulp apart does not); the class's representative is its smallest index; vmap[v] = the representative, v itself
 * for a vertex no face references.  Everything below works on vmap[faces].  Without weld vmap is the identity.
 * Components: two faces are connected when they share a welded vertex (a face that repeats an index still connects its
 * vertices); ids 0..K-1 in ascending order of the component's smallest welded vertex index.  Labels only decrease
 * (integer atomicMin); a round is hook, pointer jumping and a re-check of every face in three launches and one stream
 * synchronisation; at most 64 rounds, else S3D_E_ROUNDS.  A stale read of a label may cost a round (n_rounds is the one
 * output that may differ between two runs), never a label.
 * Table: K rows and a summary row over all faces.  counts (K + 1, 11) int64: faces, referenced welded vertices,
 * undirected edges, edges with one / two / three or more half-edges, directed edges that occur more than once,
 * faces that repeat an index, V - E + F, closed_oriented (every edge twice, every directed edge once), oriented_with_border
 * (every edge once or twice, every directed edge once).  measures (K + 1, 8) float64: area, signed volume (sum of
 * det(v0, v1, v2) / 6), bounding box lo xyz, hi xyz.  A float64 sum runs over the row's faces in ascending face index, in
 * blocks of 256 whose sums are added in ascending order: the same bits from run to run.
 *   run:         validates the indices with a kernel of its own before anything dereferences them.  S3D_E_ARG with a
 *                message for an index outside [0, n_vertices), with weld for a referenced vertex with a coordinate that is
 *                not finite (an unreferenced one is ignored), for a workspace below s3d_mesh_topology_workspace_bytes.
 *                n_faces == 0 gives 0 components.  summary_host (optional, HOST, 11 int64): the summary row's counts.
 *   emit_labels: vmap[V], face_component[F], vertex_component[V] (-1 for a vertex no face references); int64, each optional.
 *   emit_table:  counts and measures as above, n_components as run returned it.
 *   keep_run:    keep[K] (uint8, device) selects components; drop_degenerate also drops the faces that repeat a welded index.
 *                Returns the sizes of the kept mesh through one stream synchronisation.
 *   keep_emit:   the kept faces in ascending original face index, the vertices they reference in ascending original index
 *                (with weld, the representative's), indices remapped: the convention of s3d_mesh_simplify_emit.
 *                `vertices` is the input array of run.
 * The last launch of run writes K, the sizes and weld into the workspace's header.  Every emit and keep call reads it back
 * (one stream synchronisation) before anything else and returns S3D_E_ARG when no run has completed on the workspace, when
 * n_vertices, n_faces or weld are not that run's, when n_components is not the K it found, or (keep_emit) when no keep_run
 * has completed since.  keep must hold n_components flags.
 * workspace_bytes returns 0 for sizes it cannot serve (n_faces < 0 or >= 2^29, n_vertices < 0 or >= 2^30).
 * ------------------------------------------------------------------------------------------- */
size_t s3d_mesh_topology_workspace_bytes(long n_vertices, long n_faces, int weld);
int s3d_mesh_topology_run(const double* vertices, long n_vertices, const long long* faces, long n_faces, int weld,
                          void* workspace, size_t workspace_bytes, long* n_components, int* n_rounds,
                          long long* summary_host, void* stream);
int s3d_mesh_topology_emit_labels(const void* workspace, size_t workspace_bytes, long n_vertices, long n_faces, int weld,
                                  long long* vmap, long long* face_component, long long* vertex_component, void* stream);
int s3d_mesh_topology_emit_table(const void* workspace, size_t workspace_bytes, long n_vertices, long n_faces, int weld,
                                 long n_components, long long* counts, double* measures, void* stream);
int s3d_mesh_topology_keep_run(void* workspace, size_t workspace_bytes, long n_vertices, long n_faces, int weld,
                               long n_components, const unsigned char* keep, int drop_degenerate, long* n_vertices_out,
                               long* n_faces_out, void* stream);
int s3d_mesh_topology_keep_emit(const void* workspace, size_t workspace_bytes, const double* vertices, long n_vertices,
                                long n_faces, int weld, double* vertices_out, long long* faces_out, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Dataset staging on the device — the per-sample tensor work of Slice3DDataset.__getitem__
 * (reg_slices/src/datasets.py:89-179) from pre-packed uint8 shards (slice3d_amd/shards.py: PNG decode, alpha
 * compositing datasets.py:73-88 and the PIL bilinear resize are done ONCE at pack time with the reference's own
 * operations, so the 13 PNG decodes per sample leave the loader's critical path).
 * ------------------------------------------------------------------------------------------- */
/* T.ToTensor() + T.Normalize(.5,.5) (datasets.py:31-34): imgs (B, 1+n_slices, S, S, 3) uint8 HWC (image 0 = input
 * view, then the slices in the order X1..X4, Z4..Z1, Y1..Y4, datasets.py:106-120) -> img_input (B,3,S,S) and
 * img_slices (B,3*n_slices,S,S) float32, bit-identical to the reference's tensors. */
int s3d_dataset_images_fwd(const unsigned char* imgs, float* img_input, float* img_slices, int batch,
                           int n_slices, int size, void* stream);
/* the query subset (datasets.py:153-165): pts (N,4) = (qry xyz, sdf) float32 as packed, idx (n) ->
 * qry (n,3), sdf (n), occ (n) = (sdf <= 0) (optional) */
int s3d_dataset_points_fwd(const float* pts, const int* idx, long n, float* qry, float* sdf, float* occ,
                           void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SLICE3D_HIP_H */

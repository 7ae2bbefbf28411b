// ldm_ae.hip — device code of the gen_slices first-stage autoencoder and condition encoder that the LDM U-Net's kernels do not
// cover (reference ldm/modules/diffusionmodules/model.py AttnBlock :150-202, ldm/modules/encoders/modules.py
// ImageEncoderVGG16BN.forward :251-253).
#include "ldm_ops.h"

// ---------------------------------------------------------------------------------------------
// Wide single-head attention (AttnBlock): q, k, v of C = 64 * NQ channels, NQ in {1, 2, 4, 8} (512 in the kl-f8 autoencoder's mid blocks) over
// T tokens of one image, softmax(q k^T * C^-0.5) v.  The per-query accumulator is C floats wide, too wide for one wave, so:
//  - a workgroup (4 waves) owns WA_QB queries of one image; their q rows sit in LDS, pre-scaled by C^-0.5;
//  - per block of WA_KB keys the K rows are staged in LDS and the WA_QB x WA_KB logits are formed once (one fp32 FMA chain
//    per logit) into LDS, where an online softmax (running max / sum per query) turns them into weights;
//  - the V rows then replace K in the same LDS buffer and every thread accumulates P V for NQ queries x 4 channels: the
//    256 threads together hold the 16 x C output tile.
// Keys past T (a ragged last block) get weight exp(-inf) = 0.  Exact fp32 arithmetic: it serves S3D_PREC_F32 and, being at
// least as accurate as the three-product split, S3D_PREC_F16X3.
// ---------------------------------------------------------------------------------------------
#define WA_QB 16
#define WA_KB 32
#define WA_THREADS 256

template <int NQ>
__global__ __launch_bounds__(WA_THREADS) void wide_attention_kernel(const float* __restrict__ qkv, float* __restrict__ out,
                                                                    int T, float scale) {
    constexpr int C = 64 * NQ;
    constexpr int C4 = C / 4;
    constexpr int LD = C + 4;            // row pitch: consecutive rows start 4 banks apart
    constexpr int SLD = WA_KB + 1;
    __shared__ __attribute__((aligned(16))) float s_q[WA_QB * LD];
    __shared__ __attribute__((aligned(16))) float s_kv[WA_KB * LD];
    __shared__ float s_p[WA_QB * SLD];
    __shared__ float s_m[WA_QB], s_l[WA_QB], s_a[WA_QB];

    const int tid = threadIdx.x;
    const int n = blockIdx.y;
    const int q0 = blockIdx.x * WA_QB;
    const float* base = qkv + (size_t)n * T * 3 * C;

    for (int i = tid; i < WA_QB * C4; i += WA_THREADS) {
        const int r = i / C4, c4 = i - r * C4;
        const int q = q0 + r;
        f32x4 v = q < T ? ld4(base + (size_t)q * 3 * C + 4 * c4) : zero4();
        st4(s_q + r * LD + 4 * c4, v * scale);
    }
    if (tid < WA_QB) {
        s_m[tid] = -INFINITY;
        s_l[tid] = 0.f;
    }

    const int cg = tid % C4, qg = tid / C4;   // P V: channels 4cg..4cg+3 of queries qg*NQ .. qg*NQ+NQ-1
    f32x4 acc[NQ];
#pragma unroll
    for (int i = 0; i < NQ; ++i) acc[i] = zero4();

    const int lq = tid >> 4, lj = tid & 15;   // logits: query lq, keys lj and lj + 16 of the block
#pragma unroll 1
    for (int k0 = 0; k0 < T; k0 += WA_KB) {
        __syncthreads();   // the previous block's P V reads of s_kv / s_p are done
        for (int i = tid; i < WA_KB * C4; i += WA_THREADS) {
            const int r = i / C4, c4 = i - r * C4;
            const int key = k0 + r;
            st4(s_kv + r * LD + 4 * c4, key < T ? ld4(base + (size_t)key * 3 * C + C + 4 * c4) : zero4());
        }
        __syncthreads();
        {
            const float* qp = s_q + lq * LD;
            const float* k0p = s_kv + lj * LD;
            const float* k1p = s_kv + (lj + 16) * LD;
            float s0 = 0.f, s1 = 0.f;
#pragma unroll 8
            for (int c = 0; c < C; c += 4) {
                const f32x4 a = ld4(qp + c), b0 = ld4(k0p + c), b1 = ld4(k1p + c);
                s0 = fmaf(a[0], b0[0], s0); s0 = fmaf(a[1], b0[1], s0); s0 = fmaf(a[2], b0[2], s0); s0 = fmaf(a[3], b0[3], s0);
                s1 = fmaf(a[0], b1[0], s1); s1 = fmaf(a[1], b1[1], s1); s1 = fmaf(a[2], b1[2], s1); s1 = fmaf(a[3], b1[3], s1);
            }
            s_p[lq * SLD + lj] = k0 + lj < T ? s0 : -INFINITY;
            s_p[lq * SLD + lj + 16] = k0 + lj + 16 < T ? s1 : -INFINITY;
        }
        __syncthreads();   // logits written, K no longer read
        if (tid < WA_QB) {   // online softmax of query tid's row
            float* row = s_p + tid * SLD;
            const float m_old = s_m[tid];
            float mx = m_old;
            for (int j = 0; j < WA_KB; ++j) mx = fmaxf(mx, row[j]);
            float sum = 0.f;
            for (int j = 0; j < WA_KB; ++j) {
                const float p = expf(row[j] - mx);
                row[j] = p;
                sum += p;
            }
            const float alpha = expf(m_old - mx);   // 0 on the first block (m_old = -inf, mx finite: key k0 < T exists)
            s_a[tid] = alpha;
            s_l[tid] = s_l[tid] * alpha + sum;
            s_m[tid] = mx;
        }
        for (int i = tid; i < WA_KB * C4; i += WA_THREADS) {
            const int r = i / C4, c4 = i - r * C4;
            const int key = k0 + r;
            st4(s_kv + r * LD + 4 * c4, key < T ? ld4(base + (size_t)key * 3 * C + 2 * C + 4 * c4) : zero4());
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < NQ; ++i) acc[i] *= s_a[qg * NQ + i];
        const int jn = T - k0 < WA_KB ? T - k0 : WA_KB;
#pragma unroll 4
        for (int j = 0; j < jn; ++j) {
            const f32x4 v = ld4(s_kv + j * LD + 4 * cg);
#pragma unroll
            for (int i = 0; i < NQ; ++i) acc[i] += s_p[(qg * NQ + i) * SLD + j] * v;
        }
    }
#pragma unroll
    for (int i = 0; i < NQ; ++i) {
        const int r = qg * NQ + i, q = q0 + r;
        if (q < T) st4(out + ((size_t)n * T + q) * C + 4 * cg, acc[i] * (1.f / s_l[r]));
    }
}

template <int NQ>
static int launch_wide_attention_nq(const float* qkv, float* out, int N, int T, hipStream_t stream) {
    const float scale = 1.f / sqrtf((float)(64 * NQ));
    hipLaunchKernelGGL(wide_attention_kernel<NQ>, dim3((T + WA_QB - 1) / WA_QB, N), dim3(WA_THREADS), 0, stream, qkv, out, T,
                       scale);
    S3D_LAUNCH_CHECK();
    return 0;
}

int launch_wide_attention(const float* qkv, float* out, int N, int T, int C, hipStream_t stream) {
    S3D_CHECK_ARG(N >= 1 && N <= 65535 && T >= 1 && (C == 64 || C == 128 || C == 256 || C == 512),
                  "wide_attention: N=%d T=%d C=%d (C must be 64, 128, 256 or 512)", N, T, C);
    switch (C) {
        case 64: return launch_wide_attention_nq<1>(qkv, out, N, T, stream);
        case 128: return launch_wide_attention_nq<2>(qkv, out, N, T, stream);
        case 256: return launch_wide_attention_nq<4>(qkv, out, N, T, stream);
        default: return launch_wide_attention_nq<8>(qkv, out, N, T, stream);
    }
}

// ---------------------------------------------------------------------------------------------
// ImageEncoderVGG16BN's input normalisation (modules.py:251-253): ((x + 1) / 2 - mean[c]) / std[c], NCHW in and out.  A
// separate pass and not folded into conv1_1: the convolution's zero padding is applied to the NORMALISED image.
// ---------------------------------------------------------------------------------------------
__global__ void image_normalize_kernel(const float* __restrict__ x, const float* __restrict__ mean,
                                       const float* __restrict__ stdv, float* __restrict__ y, int c, long hw, long total) {
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const int cc = (int)((idx / hw) % c);
        y[idx] = ((x[idx] + 1.f) / 2.f - mean[cc]) / stdv[cc];
    }
}

int launch_image_normalize(const float* x, const float* mean, const float* stdv, float* y, int n, int c, long hw,
                           hipStream_t stream) {
    S3D_CHECK_ARG(n >= 1 && c >= 1 && hw >= 1, "image_normalize: n=%d c=%d hw=%ld", n, c, hw);
    const long total = (long)n * c * hw;
    const int blocks = (int)((total + 255) / 256 < 8192 ? (total + 255) / 256 : 8192);
    hipLaunchKernelGGL(image_normalize_kernel, dim3(blocks), dim3(256), 0, stream, x, mean, stdv, y, c, hw, total);
    S3D_LAUNCH_CHECK();
    return 0;
}

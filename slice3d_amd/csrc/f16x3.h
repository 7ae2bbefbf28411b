// f16x3.h — device building blocks of the split-precision ("f16x3") MFMA kernels, included by common.h.
//
// Every fp32 operand x is split as x = hi + lo with hi = f16(x), lo = f16(x - hi), and each product is evaluated as three
// f16 MFMAs with fp32 accumulation in the order that s3d_mfma3 defines.
// BF (S3D_PREC_BF16): single pass on the bf16 MFMA; the 16-bit lanes of the "hi" operands then hold bf16 bit patterns.
#pragma once

typedef _Float16 s3d_half2 __attribute__((ext_vector_type(2)));
typedef _Float16 s3d_half4 __attribute__((ext_vector_type(4)));
typedef _Float16 s3d_half8 __attribute__((ext_vector_type(8)));
typedef __bf16 s3d_bf2 __attribute__((ext_vector_type(2)));
typedef __bf16 s3d_bf8 __attribute__((ext_vector_type(8)));
typedef short s3d_short4 __attribute__((ext_vector_type(4)));
typedef float s3d_float2 __attribute__((ext_vector_type(2)));
typedef unsigned s3d_uint2 __attribute__((ext_vector_type(2)));
typedef unsigned s3d_uint4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ s3d_half8 s3d_ldh8(const _Float16* p) { return *reinterpret_cast<const s3d_half8*>(p); }

// hi/lo split of a pair: one v_cvt_pk_f16_f32 + two v_fma_mix{lo,hi}_f16 (lo = f16(x - f32(hi)): the subtraction is exact,
// one rounding — the same value a scalar convert - subtract - convert produces), 1.5 VALU per value.  The halves are
// written by 16-bit partial-register asm ops whose write -> MFMA-read spacing the compiler does not pad: put
// S3D_SPLIT_SETTLE() between a group of splits and MFMAs that read them straight from registers (values that go through
// LDS, or feed MFMAs a whole phase later, need nothing).  One wait state was measured as too few on gfx950: wrong P·V
// products in some schedules of the attention core, fixed by the padding alone (decode_attnq.hip).
__device__ __forceinline__ void s3d_split2(float a, float b, unsigned& hi, unsigned& lo) {
    hi = __builtin_bit_cast(unsigned, __builtin_convertvector(s3d_float2{a, b}, s3d_half2));
    asm("v_fma_mixlo_f16 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]" : "=v"(lo) : "v"(hi), "v"(a));
    asm("v_fma_mixhi_f16 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "+v"(lo) : "v"(hi), "v"(b));
}
__device__ __forceinline__ void s3d_split8(const float (&x)[8], s3d_half8& hi, s3d_half8& lo) {
    unsigned h0, h1, h2, h3, l0, l1, l2, l3;
    s3d_split2(x[0], x[1], h0, l0);
    s3d_split2(x[2], x[3], h1, l1);
    s3d_split2(x[4], x[5], h2, l2);
    s3d_split2(x[6], x[7], h3, l3);
    hi = __builtin_bit_cast(s3d_half8, s3d_uint4{h0, h1, h2, h3});
    lo = __builtin_bit_cast(s3d_half8, s3d_uint4{l0, l1, l2, l3});
}
__device__ __forceinline__ void s3d_split8(const f32x4 a, const f32x4 b, s3d_half8& hi, s3d_half8& lo) {
    unsigned h0, h1, h2, h3, l0, l1, l2, l3;
    s3d_split2(a[0], a[1], h0, l0);
    s3d_split2(a[2], a[3], h1, l1);
    s3d_split2(b[0], b[1], h2, l2);
    s3d_split2(b[2], b[3], h3, l3);
    hi = __builtin_bit_cast(s3d_half8, s3d_uint4{h0, h1, h2, h3});
    lo = __builtin_bit_cast(s3d_half8, s3d_uint4{l0, l1, l2, l3});
}
// four values -> the A / B operand of the 16-deep MFMA (v_mfma_f32_16x16x16_f16: lane group g carries k = 4g..4g+3)
__device__ __forceinline__ void s3d_split4(const f32x4 a, s3d_half4& hi, s3d_half4& lo) {
    unsigned h0, h1, l0, l1;
    s3d_split2(a[0], a[1], h0, l0);
    s3d_split2(a[2], a[3], h1, l1);
    hi = __builtin_bit_cast(s3d_half4, s3d_uint2{h0, h1});
    lo = __builtin_bit_cast(s3d_half4, s3d_uint2{l0, l1});
}
#define S3D_SPLIT_SETTLE()                          \
    __builtin_amdgcn_sched_barrier(0);              \
    asm volatile("s_nop 15" ::: "memory");          \
    __builtin_amdgcn_sched_barrier(0);

// bf16(a) | bf16(b) << 16, round to nearest even
__device__ __forceinline__ unsigned s3d_bf16_pair(float a, float b) {
    return __builtin_bit_cast(unsigned, __builtin_convertvector(s3d_float2{a, b}, s3d_bf2));
}
// the splits with a BF form (only the high halves are operands; the low halves mirror them and are never read)
template <bool BF>
__device__ __forceinline__ void s3d_split8x(const f32x4 a, const f32x4 b, s3d_half8& hi, s3d_half8& lo) {
    if (BF) {
        hi = __builtin_bit_cast(s3d_half8, s3d_uint4{s3d_bf16_pair(a[0], a[1]), s3d_bf16_pair(a[2], a[3]), s3d_bf16_pair(b[0], b[1]), s3d_bf16_pair(b[2], b[3])});
        lo = hi;
    } else {
        s3d_split8(a, b, hi, lo);
    }
}
template <bool BF>
__device__ __forceinline__ void s3d_split4x(const f32x4 a, s3d_half4& hi, s3d_half4& lo) {
    if (BF) {
        hi = __builtin_bit_cast(s3d_half4, s3d_uint2{s3d_bf16_pair(a[0], a[1]), s3d_bf16_pair(a[2], a[3])});
        lo = hi;
    } else {
        s3d_split4(a, hi, lo);
    }
}

// the hi·hi product alone (the single-pass modes), on the f16 or the bf16 MFMA 16x16x32
template <bool BF = false>
__device__ __forceinline__ f32x4 s3d_mfma_hh(const s3d_half8 a, const s3d_half8 b, const f32x4 c) {
    if (BF) return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(s3d_bf8, a), __builtin_bit_cast(s3d_bf8, b), c, 0, 0, 0);
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
}
// c += a·b on one 16x16x32 tile.  The product order is the split-precision rounding contract every kernel shares:
// a_hi·b_lo, then a_lo·b_hi, then a_hi·b_hi, accumulating into one register (SINGLE / BF: a_hi·b_hi only).  Kernels that
// issue the three products as separate loops over tiles (their schedule) keep this order loop by loop.
template <bool SINGLE = false, bool BF = false>
__device__ __forceinline__ f32x4 s3d_mfma3(const s3d_half8 ah, const s3d_half8 al, const s3d_half8 bh, const s3d_half8 bl, f32x4 c) {
    if (!SINGLE && !BF) {
        c = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bl, c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_16x16x32_f16(al, bh, c, 0, 0, 0);
    }
    return s3d_mfma_hh<BF>(ah, bh, c);
}
// the same on one 16x16x16 tile (v_mfma_f32_16x16x16_f16: a different instruction, the same order)
template <bool SINGLE = false, bool BF = false>
__device__ __forceinline__ f32x4 s3d_mfma3_k16(const s3d_half4 ah, const s3d_half4 al, const s3d_half4 bh, const s3d_half4 bl, f32x4 c) {
    if (BF) return __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(__builtin_bit_cast(s3d_short4, ah), __builtin_bit_cast(s3d_short4, bh), c, 0, 0, 0);
    if (!SINGLE) {
        c = __builtin_amdgcn_mfma_f32_16x16x16f16(ah, bl, c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_16x16x16f16(al, bh, c, 0, 0, 0);
    }
    c = __builtin_amdgcn_mfma_f32_16x16x16f16(ah, bh, c, 0, 0, 0);
    return c;
}

// reductions over the 4 lane groups g of one column (l & 15) with the gfx950 lane-swap instructions (no LDS crossbar):
// v_permlane32_swap exchanges the upper half of its first operand with the lower half of its second, so two copies
// of v become {lo, lo} and {hi, hi}; v_permlane16_swap does the same with odd / even rows of 16.  Issued as asm: the
// __builtin_amdgcn_permlane*_swap builtins of this hipcc return the FIRST result for both elements (checked on the
// GPU with unit kernels); s_nop 1 = the VALU-write -> permlane hazard the compiler would have padded.
__device__ __forceinline__ void s3d_lane_swap32(float& x, float& y) { asm("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(x), "+v"(y)); }
__device__ __forceinline__ void s3d_lane_swap16(float& x, float& y) { asm("s_nop 1\n\tv_permlane16_swap_b32 %0, %1" : "+v"(x), "+v"(y)); }
__device__ __forceinline__ float s3d_colsum16(float v) {
    float x = v, y = v;
    s3d_lane_swap32(x, y);
    x += y;
    y = x;
    s3d_lane_swap16(x, y);
    return x + y;
}
__device__ __forceinline__ float s3d_colmax16(float v) {
    float x = v, y = v;
    s3d_lane_swap32(x, y);
    x = fmaxf(x, y);
    y = x;
    s3d_lane_swap16(x, y);
    return fmaxf(x, y);
}

// Hand-issued LDS fragment reads and their counted waits.  With an LDS-DMA refill in flight hipcc models the DMA as an LDS
// access of unknown order: it either degrades every LDS wait to lgkmcnt(0) (waiting for the reads just issued for the NEXT
// step) or guards each read with vmcnt(0) (waiting for the refill).  An asm read is invisible to that bookkeeping; a wait
// names the registers it releases, so their consumers cannot be scheduled above it.  LDS returns in order: lgkmcnt(n)
// leaves exactly the n youngest reads outstanding.
#define S3D_DS_READ(dst, addr, off) asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "n"(off) : "memory")
#define S3D_LGKM_WAIT1(n, r0) asm volatile("s_waitcnt lgkmcnt(%1)" : "+v"(r0) : "n"(n))
#define S3D_LGKM_WAIT2(n, r0, r1) asm volatile("s_waitcnt lgkmcnt(%2)" : "+v"(r0), "+v"(r1) : "n"(n))
#define S3D_LGKM_WAIT3(n, r0, r1, r2) asm volatile("s_waitcnt lgkmcnt(%3)" : "+v"(r0), "+v"(r1), "+v"(r2) : "n"(n))
#define S3D_LGKM_WAIT4(n, r0, r1, r2, r3) asm volatile("s_waitcnt lgkmcnt(%4)" : "+v"(r0), "+v"(r1), "+v"(r2), "+v"(r3) : "n"(n))
#define S3D_LGKM_WAIT5(n, r0, r1, r2, r3, r4) \
    asm volatile("s_waitcnt lgkmcnt(%5)" : "+v"(r0), "+v"(r1), "+v"(r2), "+v"(r3), "+v"(r4) : "n"(n))
#define S3D_LGKM_WAIT6(n, r0, r1, r2, r3, r4, r5) \
    asm volatile("s_waitcnt lgkmcnt(%6)" : "+v"(r0), "+v"(r1), "+v"(r2), "+v"(r3), "+v"(r4), "+v"(r5) : "n"(n))

// global -> LDS copy of one 1 KiB piece by LDS-DMA (16 bytes per lane, no VGPR staging): glane = this lane's 16 bytes of the
// source piece (piece start + 8 lane), lpiece = the destination piece, off = an immediate byte offset added to both (up to
// 3 KiB: the pieces after a first one by immediate offset share its lane address and M0 value).  A macro, not a function:
// the casts stay interleaved with the address arithmetic as written, which the scheduler's tie-breaks depend on.
#define S3D_DMA_PIECE(glane, lpiece, off)                                                                                \
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(glane),                              \
                                     (__attribute__((address_space(3))) void*)(lpiece), 16, off, 0)
template <int PIECES>   // PIECES consecutive pieces from (glane, lpiece) on
__device__ __forceinline__ void s3d_dma_pieces(const _Float16* glane, _Float16* lpiece) {
    static_assert(PIECES >= 1 && PIECES <= 4, "immediate offsets up to 3 KiB");
    S3D_DMA_PIECE(glane, lpiece, 0);
    if (PIECES > 1) S3D_DMA_PIECE(glane, lpiece, 1024);
    if (PIECES > 2) S3D_DMA_PIECE(glane, lpiece, 2048);
    if (PIECES > 3) S3D_DMA_PIECE(glane, lpiece, 3072);
}

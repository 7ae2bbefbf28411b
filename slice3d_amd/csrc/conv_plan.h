// conv_plan.h — which kernel serves a ConvLaunch.  conv_plan() is the one statement of the convolution engine's dispatch: pure
// host integer arithmetic on the launch descriptor and the process's tuning, no HIP call, no pointer dereferenced (pointers
// are tested for NULL only).  launch_conv (conv.hip) launches what the plan says; s3d_conv_plan_describe (api_ldm.inc) prints it.
#pragma once
#include <stdlib.h>
#include <algorithm>
#include "conv.h"

// The small-map switches ("Environment"), read once when the library is loaded: 0 turns the route off, a
// value above 1 is its cap on the pixels of all images together (at most 64: four pixel tiles).
struct ConvTuning {
    bool small3_on, small1_on;
    long small3_pmax, small1_pmax;
};
inline ConvTuning conv_tuning_from_env() {   // S3D_CONV_SMALL: conv3x3_small_f16x3_kernel<PT, GN, 9>; S3D_CONV_SMALL_1X1: <PT, false, 1>
    const char *e3 = getenv("S3D_CONV_SMALL"), *e1 = getenv("S3D_CONV_SMALL_1X1");
    const int v3 = e3 ? atoi(e3) : 1, v1 = e1 ? atoi(e1) : 1;
    return {v3 != 0, v1 != 0, v3 > 1 ? v3 : 32, v1 > 1 ? v1 : 64};
}
const ConvTuning& conv_tuning();   // this process's (conv.hip)

enum ConvFamily { CONV_IGEMM, CONV_IGEMM_F16X3, CONV_LIN_ROWS, CONV_LIN_STREAM, CONV_LDS, CONV_SMALL, CONV_UP2X_LDS, CONV_N_FAMILIES };
// name as a kernel trace prints it, and the number of template arguments
static const struct { const char* name; int nargs; const char* bools; } kConvFamily[CONV_N_FAMILIES] = {
    {"conv_igemm_kernel", 7, "0000011"},       {"conv_igemm_f16x3_kernel", 6, "000001"}, {"lin_rows_f16x3_kernel", 0, ""},
    {"lin_stream_f16x3_kernel", 1, "0"},       {"conv3x3_lds_f16x3_kernel", 6, "000011"}, {"conv3x3_small_f16x3_kernel", 3, "010"},
    {"conv_up2x_lds_f16x3_kernel", 7, "0000000"}};

struct ConvPlan {
    int err;                  // 0, or the refusal's code (its message is in s3d_last_error)
    ConvFamily family;
    int targ[7];              // the kernel's template arguments (bools as 0 / 1)
    unsigned grid_x, grid_y, block;
    int splits, chunks_per_split;   // split-K (1: none)
    int tiles_x, tiles_y;     // 8 x 16 pixel tiles of a map (the LDS-staged kernels)
    long n_tasks;             // lin_stream: row blocks the persistent workgroups share
    bool finish;              // conv_splitk_finish_kernel follows (false with splits > 1: the partials stay for splits_out)
    bool per_parity;          // fp32 up2x: the generic kernel is launched once per output parity (4 launches)
};

constexpr long kSmallHalo = 160, kSmallHalo1 = 64;   // zero-bordered pixels conv3x3_small parks: all forms | the one-pixel-tile form
constexpr int kLinRowsTile = 192;                    // rows of a lin_rows workgroup

inline bool conv_same_grid(const ConvLaunch& a) { return !((a.Hin && a.Hin != a.H) || (a.Win && a.Win != a.W)); }
// every source a whole number of 32-channel chunks (what the LDS-staged and small-map kernels park)
inline bool conv_chunked_sources(const ConvLaunch& a) {
    for (int s = 0; s < a.nsrc; ++s)
        if (a.src[s].C % 32 || a.src[s].sbcast) return false;
    return true;
}
inline bool conv_splittable(const ConvLaunch& a) { return a.splitk_ws && a.out_mode == S3D_OUT_NHWC; }
// A 3x3 map smaller than the LDS-staged kernel's 8 x 16 tile wastes lanes: worth it only when split-K supplies the parallelism
inline bool conv_below_lds_tile(int H, int W) { return W < 16 || H < 8; }
inline int conv_splitk_finish_blocks(const ConvLaunch& a) {
    const long total = (long)(((size_t)a.N * a.H * a.W * a.CoutPad) >> 2);
    return (int)((total + 255) / 256 < 2048 ? (total + 255) / 256 : 2048);
}

// Split count of a split-K launch of `nblk_k` workgroups per split over `nchunk` 32-channel chunks: the chip holds 512 of these
// workgroups at a time (two per CU); a launch runs in ceil(workgroups / 512) rounds of (chunks per split + a fixed fetch /
// epilogue share) each; the finish pass reads `se` partials.  Pick the count with the least rounds x length.
// (doubling until 512 workgroups was the rule before round 4: it landed on 640 — two rounds, the second a quarter full — for
//  every 64 x 64 x 320 layer of the LDM U-Net)
inline void conv_plan_splits(ConvPlan& p, const ConvLaunch& a, long nblk_k, bool may_split) {
    int nchunk = 0;
    for (int s = 0; s < a.nsrc; ++s) nchunk += a.src[s].C >> 5;
    const size_t out_floats = (size_t)a.N * a.H * a.W * a.CoutPad;
    int splits = 1;
    long best = -1;
    for (int sp = 1; may_split && sp <= nchunk && (size_t)sp * out_floats <= a.splitk_floats; ++sp) {
        const int c = (nchunk + sp - 1) / sp, se = (nchunk + c - 1) / c;
        if (se != sp) continue;   // (the same chunking as a smaller count)
        const long rounds = (nblk_k * se + 511) / 512;
        const long cost = rounds * (2 * c + 3) + (se > 1 ? 1 + se / 8 : 0);   // half-chunk units
        if (best < 0 || cost < best) {
            best = cost;
            splits = se;
        }
    }
    p.chunks_per_split = (nchunk + splits - 1) / splits;
    p.splits = (nchunk + p.chunks_per_split - 1) / p.chunks_per_split;
}
inline void conv_plan_kernel(ConvPlan& p, ConvFamily f, std::initializer_list<int> targ, long gx, unsigned gy = 1, unsigned block = 256) {
    p.family = f;
    std::copy(targ.begin(), targ.end(), p.targ);
    p.grid_x = (unsigned)gx; p.grid_y = gy; p.block = block;
}
// conv3x3_small_f16x3_kernel on a split-K plan: PT = 1, 2 or 4 tiles of 16 pixels, one 64-channel output tile per workgroup
inline void conv_plan_small(ConvPlan& p, const ConvLaunch& a, long P, long halo, int taps) {
    const int pt = (int)((P + 15) / 16);
    conv_plan_kernel(p, CONV_SMALL, {pt == 1 && halo <= kSmallHalo1 ? 1 : pt <= 2 ? 2 : 4, a.gn.table != nullptr, taps}, a.CoutPad / 64, (unsigned)p.splits);
}
#define CONV_GRID_CHECK(nblk, lo) S3D_CHECK_ARG((nblk) >= (lo) && (nblk) < (1L << 31), "conv grid out of range (%ld)", (long)(nblk))

inline int conv_plan_route(const ConvLaunch& a, const ConvTuning& t, ConvPlan& p) {
    // ---- what the engine does not serve
    S3D_CHECK_ARG(a.ks >= 1 && a.ks <= 3, "conv: ks must be 1, 2 or 3");
    S3D_CHECK_ARG(!a.pad_origin || (a.ks == 3 && a.stride > 1 && a.out_mode == S3D_OUT_NHWC),
                  "conv: pad_origin is served for strided 3x3 convolutions only");
    S3D_CHECK_ARG(a.CoutPad % 16 == 0 && a.CoutPad > 0, "conv: CoutPad %d", a.CoutPad);
    for (int s = 0; s < a.nsrc; ++s)
        S3D_CHECK_ARG(a.src[s].C % 16 == 0 && a.src[s].bdiv >= 1, "conv: bad source %d", s);
    // ConvTranspose output: the quadrant-scatter store carries affine + activation only.  Its full-line form (32-channel
    // pairs, conv_epilogue) pairs accumulator tiles (jt0 + 2 np, jt0 + 2 np + 1) with jt0 = a multiple of NT — even for
    // every tile shape of the menu below — and would index dropout / gate / residual by the SCATTERED offset.
    S3D_CHECK_ARG(a.out_mode != S3D_OUT_CONVT || (a.drop.p <= 0.f && !a.gate && !a.residual && !a.out_accumulate),
                  "conv: ConvTranspose output takes no dropout / gate / residual / accumulate");
    // A pre-activation addend is the accumulators' starting value in the 3x3 kernels.  Not served: the ConvTranspose scatter,
    // split-K (every split would start at it; the small-map kernels run on split-K only), the 1x1 row-linear kernels, a fused
    // GroupNorm instantiation
    S3D_CHECK_ARG(!a.pre || a.up2x || (a.ks == 3 && a.stride <= 1 && !a.Hin && !a.Win), "conv: a pre-activation addend is served for 3x3 stride-1 convolutions only");
    S3D_CHECK_ARG(!a.pre || a.out_mode != S3D_OUT_CONVT, "conv: a pre-activation addend with a ConvTranspose output");
    S3D_CHECK_ARG(!a.pre || !a.splitk_ws, "conv: a pre-activation addend with a split-K workspace");
    S3D_CHECK_ARG(!a.pre || !a.gn.table, "conv: a pre-activation addend with a fused GroupNorm");
    S3D_CHECK_ARG(!a.pre || (a.pre_bdiv >= 1 && a.pre_bmod >= 0), "conv: addend image rule bdiv %d bmod %d", a.pre_bdiv, a.pre_bmod);
    const long P = (long)a.N * a.H * a.W;
    p.tiles_x = (a.W + 15) / 16; p.tiles_y = (a.H + 7) / 8;
    const long tiles = (long)p.tiles_x * p.tiles_y * a.N;
    const int co_wg = a.CoutPad % 64 == 0 ? 64 : 32;   // output channels of a workgroup of the LDS-staged kernels

    // ---- 1. The composed ConvTranspose -> 3x3: its own 2x2 form on the low-resolution grid with its own kernels.  Not served with
    // it: split-K, a fused GroupNorm, the ConvTranspose scatter or NCHW, a second or broadcast source, any epilogue beyond scale / shift / ReLU
    if (a.up2x) {
        S3D_CHECK_ARG(a.ks == 2 && a.stride <= 1 && !a.Hin && !a.Win, "conv: the composed ConvTranspose -> 3x3 is a 2x2 stride-1 form (ks %d)", a.ks);
        S3D_CHECK_ARG(!a.splitk_ws && !a.splits_out, "conv: the composed ConvTranspose -> 3x3 with a split-K workspace");
        S3D_CHECK_ARG(!a.gn.table, "conv: the composed ConvTranspose -> 3x3 with a fused GroupNorm");
        S3D_CHECK_ARG(a.out_mode == S3D_OUT_NHWC && a.cout_store == a.CoutPad, "conv: the composed ConvTranspose -> 3x3 stores NHWC, all channels");
        S3D_CHECK_ARG(a.pre && a.pre_tab, "conv: the composed ConvTranspose -> 3x3 needs its addend and its border-class table");
        S3D_CHECK_ARG(a.nsrc == 1 && !a.src[0].sbcast && a.src[0].C % 32 == 0 && a.CoutPad % 32 == 0 && a.KU == a.src[0].C / 4,
                      "conv: the composed ConvTranspose -> 3x3 takes one plain source (C %d, Cout %d, KU %d)", a.src[0].C, a.CoutPad, a.KU);
        S3D_CHECK_ARG(!a.pad_origin && a.out_cstride >= a.CoutPad && a.src[0].bdiv >= 1 && a.src[0].bmod >= 0 && a.pre_bdiv >= 1 && a.pre_bmod >= 0,
                      "conv: the composed ConvTranspose -> 3x3: pad_origin %d, channel stride %d < %d, or a bad image rule", a.pad_origin, a.out_cstride, a.CoutPad);
        S3D_CHECK_ARG(a.drop.p <= 0.f && !a.gate && !a.residual && !a.out_accumulate && (a.act == S3D_ACT_NONE || a.act == S3D_ACT_RELU),
                      "conv: the composed ConvTranspose -> 3x3 takes scale / shift / ReLU only");
        if (!a.wpk16) {   // fp32: the generic kernel on each parity's rows of the weight image (correct, not tuned: no caller times it)
            const long nblk = ((P + 31) / 32) * (a.CoutPad / 32);
            CONV_GRID_CHECK(nblk, 1);
            p.per_parity = true;
            conv_plan_kernel(p, CONV_IGEMM, {1, 1, 2, 2, 2, 1, 1}, nblk);
            return 0;
        }
        // Split precision (and single pass): one staged tile serves several parities (profiles/unet_upconv_composite.md): all four on
        // the 32-channel tile (up4: 128 virtual output channels per workgroup; one LDS buffer, K is two chunks), the two of an output
        // row on the 64-channel tile (up3: all of its 64 channels; up2: measured 152 us against 190 us with one parity per
        // workgroup).  Both run two waves per SIMD without scratch.  The 32-channel tile fits the three waves of the plain 3x3 with
        // ONE parity per workgroup only; that form measured 339-340 us at up4 against 275 us for this one (the two parities of a row: 318 us).
        const long nblk = tiles * (a.CoutPad / co_wg) * (co_wg == 64 ? 2 : 1);
        CONV_GRID_CHECK(nblk, 0);
        if (co_wg == 64) conv_plan_kernel(p, CONV_UP2X_LDS, {4, 2, 2, 1, 2, 2, 2}, nblk);
        else conv_plan_kernel(p, CONV_UP2X_LDS, {2, 4, 1, 2, 2, 1, 2}, nblk);
        return 0;
    }
    S3D_CHECK_ARG(!a.pre_tab, "conv: a border-class table without the composed ConvTranspose -> 3x3");
    const bool f16_chunks = a.wpk16 && a.KU % 2 == 0 && conv_chunked_sources(a);
    const bool plain = a.stride <= 1 && conv_same_grid(a);

    // ---- 2. LDS-staged 3x3 (stride 1, "same"), split precision
    if (a.ks == 3 && plain && f16_chunks && a.CoutPad % 32 == 0 && (!conv_below_lds_tile(a.H, a.W) || conv_splittable(a))) {
        const long nblk = tiles * (a.CoutPad / co_wg);
        CONV_GRID_CHECK(nblk, 0);
        // Maps of a few pixels (all images together at most 64 pixels, 160 with their zero borders): conv3x3_small_f16x3_kernel.
        // (P <= 32: at the 8 x 8 maps — four pixel tiles — this kernel measured 16.7-17.5 us per call against the tiled kernel's
        //  16.1, in the compact form, in a conflict-free form over the zero-bordered index space and with the table loads ahead of
        //  the weights; at the 4 x 4 maps 11.2 against 16.0: profiles/r06_ldm_small_maps.md.  S3D_CONV_SMALL=64 forces it there.
        //  Four 4 x 4 images: 7.08 -> 7.01 ms per batch-4 step.)
        const long halo = (long)a.N * (a.H + 2) * (a.W + 2);
        const bool small = t.small3_on && conv_splittable(a) && co_wg == 64 && halo <= kSmallHalo &&
                           (P <= std::min(t.small3_pmax, 64L) || ((long)a.H * a.W <= 16 && P <= 64));
        // split-K when the pixel x channel tiling cannot fill the chip (deep encoder layers at batch 1)
        const long nblk_k = small ? a.CoutPad / 64 : nblk;   // workgroups per split
        conv_plan_splits(p, a, nblk_k, conv_splittable(a) && nblk_k < 512);
        if (small && p.splits > 1) {   // split-K only: same chunk ranges and product order as the tiled kernel, the same bits
            conv_plan_small(p, a, P, halo, 9);
            return 0;
        }
        int ct = 0;   // GroupNorm of the input in the staging path (LDM U-Net): its own instantiations (12 KiB of table)
        for (int s = 0; s < a.nsrc; ++s) ct += a.src[s].C;
        S3D_CHECK_ARG(!a.gn.table || ct <= S3D_GN_CMAX, "conv: fused GroupNorm over %d channels", ct);
        // the single-buffer variant: plain 32-channel-output layers of up to 2 chunks per workgroup (measured -13 % there, +5 % on
        // the 64-wide tile).  An addend comes without a split-K workspace, so splits == 1 with it
        const int nbuf = co_wg == 32 && !a.gn.table && !a.pre && p.chunks_per_split <= 2 ? 1 : 2;
        if (co_wg == 64) conv_plan_kernel(p, CONV_LDS, {4, 2, 2, 2, a.gn.table != nullptr, a.pre != nullptr}, nblk, (unsigned)p.splits);
        else conv_plan_kernel(p, CONV_LDS, {2, 4, 1, nbuf, a.gn.table != nullptr, a.pre != nullptr}, nblk, (unsigned)p.splits);
        return 0;
    }
    // ---- 3. no other kernel applies a GroupNorm to its input
    S3D_CHECK_ARG(!a.gn.table, "conv: a fused GroupNorm needs the LDS-staged 3x3 kernel (ks 3, stride 1, channel counts multiples of 32)");

    // ---- 4. 1x1 convolutions of maps of a few pixels on the small-map kernel (TAPS = 1); what it buys them is the split-K, so a
    // plan that would not split falls through.  (Up to 64 pixels — four pixel tiles: step 4.00-4.08 -> 3.96 ms with 32, 3.88 with 64)
    if (t.small1_on && a.ks == 1 && a.stride <= 1 && !a.Hin && !a.Win && f16_chunks && a.CoutPad % 64 == 0 && conv_splittable(a) &&
        P <= std::min(t.small1_pmax, 64L) && P <= kSmallHalo) {
        conv_plan_splits(p, a, a.CoutPad / 64, true);
        if (p.splits > 1) {
            conv_plan_small(p, a, P, P, 1);
            return 0;
        }
    }
    // ---- 5. / 6. row-linear layers on long row sets: one plain source of whole 32-channel chunks
    const ConvSrc& S = a.src[0];
    if (a.ks == 1 && a.nsrc == 1 && plain && a.wpk16 && a.CoutPad % 32 == 0 && !S.sbcast && !S.bmod && S.bdiv == 1 && a.KU == S.C / 16) {
        // lin_stream's eligibility (K a multiple of 128, P >= 2^17: the decoder token rows).  K > 128: all 128 outputs live; plain products only
        // (no scale / bias / output dropout).  cout_store == CoutPad: the residual rows of a 32-channel output slot are requested
        // without a per-channel guard (hand-issued loads), so every slot must lie inside the output / residual row
        if (S.C % 128 == 0 && S.C <= 384 && !(S.C > 128 && (a.CoutPad != 128 || a.drop.p > 0.f || a.scale || a.shift)) &&
            a.out_mode == S3D_OUT_NHWC && !a.gate && !a.out_accumulate && a.cout_store == a.CoutPad && !a.scale &&
            (a.act == S3D_ACT_NONE || a.act == S3D_ACT_RELU) && P >= (1L << 17)) {
            const int kc = S.C / 128, rows_wg = kc > 1 ? 128 : 192;   // 4 waves x 2 or 3 row tiles
            p.n_tasks = (P + rows_wg - 1) / rows_wg;
            conv_plan_kernel(p, CONV_LIN_STREAM, {kc}, std::min(p.n_tasks, 512L));   // persistent: two workgroups per CU
            return 0;
        }
        // lin_rows (K <= 128); shorter row sets stay on the tile menu (more, smaller workgroups)
        if (a.KU % 2 == 0 && S.C % 32 == 0 && S.C <= 128 && P >= 65536) {
            const long nblk = (P + kLinRowsTile - 1) / kLinRowsTile;
            CONV_GRID_CHECK(nblk, 0);
            conv_plan_kernel(p, CONV_LIN_ROWS, {}, nblk);
            return 0;
        }
    }
    // ---- 7. Tile menu of the implicit-GEMM kernels: (pixels x couts) per workgroup of 4 waves.  Per CoutPad class, the largest
    // tile that still yields `want` workgroups (about 2 per CU); small late-encoder maps fall through to the small tiles.
    static const struct { int mod; long want; int MT, NT, WM, WN; } menu[] = {
        {128, 512, 4, 4, 2, 2}, {128, 512, 2, 4, 2, 2}, {128, 256, 1, 4, 2, 2}, {128, 0, 1, 1, 2, 2},
        {64, 512, 4, 4, 4, 1},  {64, 256, 2, 2, 2, 2},  {64, 0, 1, 1, 2, 2},
        {32, 512, 4, 2, 4, 1},  {32, 0, 1, 1, 2, 2},
        {16, 512, 4, 1, 4, 1},  {16, 0, 1, 1, 4, 1}};
    bool f16 = a.wpk16 != nullptr && (a.KU % 2 == 0);
    for (int s = 0; s < a.nsrc; ++s) f16 = f16 && (a.src[s].C % 32 == 0);
    for (const auto& m : menu) {
        const int pix = m.WM * m.MT * 16, co = m.WN * m.NT * 16;
        const long nblk = ((P + pix - 1) / pix) * (a.CoutPad / co);
        if (a.CoutPad % m.mod || nblk < m.want) continue;
        CONV_GRID_CHECK(nblk, 1);
        conv_plan_kernel(p, f16 ? CONV_IGEMM_F16X3 : CONV_IGEMM, {m.MT, m.NT, m.WM, m.WN, a.ks, a.pre != nullptr, 0}, nblk, 1, m.WM * m.WN * 64);
        return 0;
    }
    return 0;   // (not reached: CoutPad % 16 == 0 was checked and the last row of a class takes every count)
}
#undef CONV_GRID_CHECK

inline ConvPlan conv_plan(const ConvLaunch& a, const ConvTuning& t) {
    ConvPlan p = {};
    p.splits = 1;
    p.err = conv_plan_route(a, t, p);
    p.finish = p.splits > 1 && !a.splits_out;
    return p;
}

// `conv3x3_small_f16x3_kernel<2,true,9> grid=2x5 block=256 splits=5 finish=1`, one launch per `;`-separated part
inline void conv_plan_describe(const ConvLaunch& a, const ConvPlan& p, char* buf, size_t len) {
    const auto& f = kConvFamily[p.family];
    size_t n = (size_t)snprintf(buf, len, "%s%s", f.name, f.nargs ? "<" : "");
    for (int i = 0; i < f.nargs && n < len; ++i) {
        const char* sep = i + 1 < f.nargs ? "," : ">";
        if (f.bools[i] == '1') n += (size_t)snprintf(buf + n, len - n, "%s%s", p.targ[i] ? "true" : "false", sep);
        else n += (size_t)snprintf(buf + n, len - n, "%d%s", p.targ[i], sep);
    }
    if (n < len) n += (size_t)snprintf(buf + n, len - n, " grid=%ux%u block=%u splits=%d finish=%d%s", p.grid_x, p.grid_y, p.block, p.splits, (int)p.finish, p.per_parity ? " launches=4" : "");
    if (p.finish && n < len) snprintf(buf + n, len - n, "; conv_splitk_finish_kernel grid=%dx1 block=256", conv_splitk_finish_blocks(a));
}

// mesh_common.h — what the mesh translation units (mesh_eval.hip, mesh_sdf.hip, mesh_render.hip, mesh_simplify.hip,
// mesh_topology.hip) share, and what a new one starts from.  Host scaffolding: the workspace arena (MeArena), the 1-D
// launch (me_blocks, ME_LAUNCH; S3D_HIP_TRY is common.h's) and the tail of a cell-list build (me_lists_finish).  Device
// code: the deterministic tiled scan (me_scan, me_scan_total), the partial bounding boxes over the vertices that the
// faces reference and their fold (me_bbox_partial_kernel, me_bbox_fold), the float64 3-vectors (me_v3) and the emit of
// the vertices a compaction keeps (me_emit_vertices_kernel).  The algorithms (which cells a face goes to, which lists a
// vertex has) stay with their units.
#pragma once
#include <math.h>

#include <algorithm>

#include "common.h"

#define ME_BLOCK 256
#define ME_ITEMS 16                         // consecutive items per thread of a scan tile
#define ME_TILE (ME_BLOCK * ME_ITEMS)
#define ME_BBOX_BLOCKS 512                  // partial bounding boxes
#define ME_RES_MAX 8192                     // hash_resolution bound: res^2 cells in 32-bit indexing

static inline size_t me_align(size_t x) { return (x + 255) & ~(size_t)255; }

// carves a caller's workspace into 256-byte aligned arrays, in the order of the take calls; with base == nullptr it only
// adds up the bytes.  A unit's layout function is one pass of takes into its struct and returns `off`, so an array's
// size is written once.
struct MeArena {
    char* base;
    size_t off = 0;
    template <typename T>
    T* take(size_t n) {
        const size_t at = off;
        off += me_align(n * sizeof(T));
        return base ? (T*)(base + at) : nullptr;
    }
};

// 1-D launch of ME_BLOCK threads over n items.  The grid is at least one block; for n >= 1 that is ceil(n / ME_BLOCK).
static inline unsigned me_blocks(long n) { return (unsigned)std::max<long>(1, (n + ME_BLOCK - 1) / ME_BLOCK); }
#define ME_LAUNCH(kernel, n, st, ...) hipLaunchKernelGGL(kernel, dim3(me_blocks(n)), dim3(ME_BLOCK), 0, st, __VA_ARGS__)

// =============================================================================================
// tiled scan of n items (exclusive for counts -> offsets, inclusive for areas -> cdf); deterministic order
// =============================================================================================
template <typename T>
__device__ __forceinline__ T me_block_exclusive_scan(T v, T* s_wave, T& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    T x = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const T y = __shfl_up(x, d, 64);
        if (lane >= d) x += y;
    }
    T ex = __shfl_up(x, 1, 64);
    if (lane == 0) ex = 0;
    if (lane == 63) s_wave[wave] = x;
    __syncthreads();
    T base = 0, tot = 0;
    for (int w = 0; w < ME_BLOCK / 64; ++w) {
        const T t = s_wave[w];
        if (w < wave) base += t;
        tot += t;
    }
    __syncthreads();
    total = tot;
    return base + ex;
}

// out[i] = sum of in[0 .. i) (INCL = false) or in[0 .. i] (INCL = true) within the tile; tile total -> tsum[tile].
// out may alias in.
template <typename Tin, typename T, bool INCL>
__global__ __launch_bounds__(ME_BLOCK) void me_scan_tiles_kernel(const Tin* in, T* out, long n, T* tsum) {
    __shared__ T s_wave[ME_BLOCK / 64];
    const long base = (long)blockIdx.x * ME_TILE + (long)threadIdx.x * ME_ITEMS;
    T v[ME_ITEMS];
    T s = 0;
#pragma unroll
    for (int k = 0; k < ME_ITEMS; ++k) {
        v[k] = base + k < n ? (T)in[base + k] : (T)0;
        s += v[k];
    }
    T tot;
    T run = me_block_exclusive_scan<T>(s, s_wave, tot);
#pragma unroll
    for (int k = 0; k < ME_ITEMS; ++k) {
        if (base + k < n) {
            if (INCL) {
                run += v[k];
                out[base + k] = run;
            } else {
                out[base + k] = run;
                run += v[k];
            }
        }
    }
    if (threadIdx.x == 0) tsum[blockIdx.x] = tot;
}
// one block: exclusive scan of the n tile totals in place, grand total -> p[n]
template <typename T>
__global__ __launch_bounds__(ME_BLOCK) void me_scan_totals_kernel(T* p, long n) {
    __shared__ T s_wave[ME_BLOCK / 64];
    T carry = 0;
    for (long b = 0; b < n; b += ME_BLOCK) {
        const long i = b + threadIdx.x;
        const T v = i < n ? p[i] : (T)0;
        T tot;
        const T ex = me_block_exclusive_scan<T>(v, s_wave, tot);
        if (i < n) p[i] = carry + ex;
        carry += tot;
    }
    if (threadIdx.x == 0) p[n] = carry;
}
template <typename T>
__global__ void me_add_tile_offsets_kernel(T* out, long n, const T* tsum) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] += tsum[i / ME_TILE];
}
template <typename Tin, typename T, bool INCL>
static void me_scan(const Tin* in, T* out, long n, T* tsum, hipStream_t st) {
    const long tiles = (n + ME_TILE - 1) / ME_TILE;
    hipLaunchKernelGGL((me_scan_tiles_kernel<Tin, T, INCL>), dim3((unsigned)tiles), dim3(ME_BLOCK), 0, st, in, out, n, tsum);
    hipLaunchKernelGGL((me_scan_totals_kernel<T>), dim3(1), dim3(ME_BLOCK), 0, st, tsum, tiles);
    hipLaunchKernelGGL((me_add_tile_offsets_kernel<T>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, out, n, tsum);
}
// where me_scan leaves the grand total of its n items: behind the tile totals, at tsum[tiles] (tsum holds tiles + 1).
// An exclusive scan over n + 1 items also leaves the total of the first n in out[n]: the simplifier's vertex count and
// the topology's K are read there.
template <typename T>
static inline T* me_scan_total(T* tsum, long n) {
    return tsum + (n + ME_TILE - 1) / ME_TILE;
}

// The tail of a cell-list build (the cells of a hash or grid, the tiles of an image): cnt[0 .. n) -> off[0 .. n], the
// exclusive scan with the grand total behind the last offset; the total and flags[0] come back to the host with the
// build's one stream synchronisation.  flags[0] is what me_bbox_partial_kernel raises.
static int me_lists_finish(const char* what, const unsigned* cnt, long long* off, long n, long long* tsum, const int* flags,
                           long n_vertices, long* n_entries, hipStream_t st) {
    me_scan<unsigned, long long, false>(cnt, off, n, tsum, st);
    S3D_LAUNCH_CHECK();
    long long total = 0;
    int bad = 0;
    // the scan writes off[0 .. n); the end of the last list is the grand total
    S3D_HIP_TRY(what, hipMemcpyAsync(off + n, me_scan_total(tsum, n), 8, hipMemcpyDeviceToDevice, st));
    S3D_HIP_TRY(what, hipMemcpyAsync(&total, me_scan_total(tsum, n), 8, hipMemcpyDeviceToHost, st));
    S3D_HIP_TRY(what, hipMemcpyAsync(&bad, flags, 4, hipMemcpyDeviceToHost, st));
    S3D_HIP_TRY(what, hipStreamSynchronize(st));
    S3D_CHECK_ARG(!bad, "%s: a face indexes a vertex outside [0, %ld)", what, n_vertices);
    *n_entries = (long)total;
    return 0;
}

// bbox over the vertices the faces reference (inside_mesh.py:12-15 takes it over mesh.vertices[mesh.faces])
static __global__ __launch_bounds__(ME_BLOCK) void me_bbox_partial_kernel(const double* __restrict__ verts, long nv,
                                                                  const long long* __restrict__ faces, long nf,
                                                                  double* __restrict__ part, int* __restrict__ flags) {
    __shared__ double s[6][ME_BLOCK];
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (long i = (long)blockIdx.x * ME_BLOCK + threadIdx.x; i < 3 * nf; i += (long)gridDim.x * ME_BLOCK) {
        const long long vi = faces[i];
        if (vi < 0 || vi >= nv) {
            flags[0] = 1;
            continue;
        }
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double x = verts[3 * vi + a];
            lo[a] = fmin(lo[a], x);
            hi[a] = fmax(hi[a], x);
        }
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        s[a][threadIdx.x] = lo[a];
        s[3 + a][threadIdx.x] = hi[a];
    }
    __syncthreads();
    for (int h = ME_BLOCK / 2; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) {
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                s[a][threadIdx.x] = fmin(s[a][threadIdx.x], s[a][threadIdx.x + h]);
                s[3 + a][threadIdx.x] = fmax(s[3 + a][threadIdx.x], s[3 + a][threadIdx.x + h]);
            }
        }
        __syncthreads();
    }
    if (threadIdx.x < 6) part[blockIdx.x * 6 + threadIdx.x] = s[threadIdx.x][0];
}
// the fold of the nb partial boxes in block order (one thread's work): lo / hi stay +inf / -inf without a valid face
__device__ __forceinline__ void me_bbox_fold(const double* __restrict__ part, int nb, double* lo, double* hi) {
    for (int a = 0; a < 3; ++a) lo[a] = INFINITY, hi[a] = -INFINITY;
    for (int b = 0; b < nb; ++b)
        for (int a = 0; a < 3; ++a) {
            lo[a] = fmin(lo[a], part[6 * b + a]);
            hi[a] = fmax(hi[a], part[6 * b + 3 + a]);
        }
}

// =============================================================================================
// float64 3-vectors; every product and sum is rounded on its own (the mesh units are compiled with -ffp-contract=off)
// =============================================================================================
struct me_v3 {
    double x, y, z;
};
static __device__ __forceinline__ me_v3 me_ld(const double* __restrict__ P, int v) {
    return me_v3{P[3 * (long)v], P[3 * (long)v + 1], P[3 * (long)v + 2]};
}
static __device__ __forceinline__ me_v3 me_sub(me_v3 a, me_v3 b) { return me_v3{a.x - b.x, a.y - b.y, a.z - b.z}; }
static __device__ __forceinline__ double me_dot(me_v3 a, me_v3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
static __device__ __forceinline__ me_v3 me_cross(me_v3 a, me_v3 b) {
    return me_v3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}

// out[vmap[v]] = P[v] for the vertices a compaction keeps (used[v]); vmap is the exclusive scan of used
static __global__ void me_emit_vertices_kernel(const double* __restrict__ P, const int* __restrict__ used,
                                               const int* __restrict__ vmap, long nv, double* __restrict__ out) {
    const long v = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= nv || !used[v]) return;
    const long d = vmap[v];
    out[3 * d] = P[3 * v], out[3 * d + 1] = P[3 * v + 1], out[3 * d + 2] = P[3 * v + 2];
}

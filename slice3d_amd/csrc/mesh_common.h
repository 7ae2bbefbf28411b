// mesh_common.h — what the mesh translation units (mesh_eval.hip, mesh_sdf.hip) share: the workspace alignment, the
// deterministic tiled scan and the partial bounding boxes over the vertices that the faces reference.
#pragma once
#include <math.h>

#include "common.h"

#define ME_BLOCK 256
#define ME_ITEMS 16                         // consecutive items per thread of a scan tile
#define ME_TILE (ME_BLOCK * ME_ITEMS)
#define ME_BBOX_BLOCKS 512                  // partial bounding boxes
#define ME_RES_MAX 8192                     // hash_resolution bound: res^2 cells in 32-bit indexing

static inline size_t me_align(size_t x) { return (x + 255) & ~(size_t)255; }

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

// mesh_eval.hip — scoring of reconstructed meshes on the device.
//
//   point-in-mesh:   replaces check_mesh_contains of reg_slices/src_convonet/utils/libmesh/inside_mesh.py:5-139 together
//                    with its compiled cell hash (libmesh/triangle_hash.pyx:10-88), bit for bit: the same float64
//                    rescale, the same cell lists, the same strict 2-D test and depth comparison, the same parity rule.
//   nearest neighbour: the exact squared distance (and index) of each point of A to the nearest point of B — what
//                    utils_eval.points_dist / chamfer_dist / eval_hausdoff (reg_slices/src/utils_eval.py:48-109) get from
//                    scipy's cKDTree and directed_hausdorff.
//   surface sampling: area-weighted points on a triangle mesh, counter-based random numbers (seed, sample index).
//
// This file is compiled with -ffp-contract=off (Makefile): every float64 product and sum of the point-in-mesh path is
// rounded on its own as numpy rounds it, so no fused multiply-add moves a point across a cell or triangle edge.
#include <math.h>
#include <string.h>

#include <algorithm>

#include "mesh_common.h"

// =============================================================================================
// point-in-mesh (inside_mesh.py + triangle_hash.pyx)
// =============================================================================================
struct ContainsWs {
    double* part;          // [ME_BBOX_BLOCKS][6] partial (min xyz, max xyz)
    double* prm;           // scale[3], translate[3], degenerate flag
    int* flags;            // [0]: a face index outside [0, n_vertices)
    double* tri;           // [n_faces][9] rescaled triangles
    unsigned* cnt;         // [res*res] triangles per cell, then the fill cursors
    long long* off;        // [res*res + 1] first entry of each cell
    long long* tsum;       // [tiles + 1]
    long cells;
};
// the arrays in the workspace's order; base == nullptr: only the size
static size_t contains_layout(long nf, int res, ContainsWs& w, char* base) {
    MeArena a{base};
    w.cells = (long)res * res;
    const long tiles = (w.cells + ME_TILE - 1) / ME_TILE;
    w.part = a.take<double>(ME_BBOX_BLOCKS * 6), w.prm = a.take<double>(8), w.flags = a.take<int>(4);
    w.tri = a.take<double>(9 * (size_t)nf), w.cnt = a.take<unsigned>(w.cells), w.off = a.take<long long>(w.cells + 1);
    w.tsum = a.take<long long>(tiles + 1);
    return a.off;
}

// scale = (res-1)/(bmax-bmin), translate = 0.5 - scale*bmin (inside_mesh.py:17-18); a flat (or empty) box marks the mesh
// degenerate: the reference's inf / NaN rescale then fails every point's bbox test (inside_mesh.py:40-41)
__global__ void me_bbox_final_kernel(const double* __restrict__ part, int nb, double* __restrict__ prm, int res) {
    if (threadIdx.x != 0) return;
    double lo[3], hi[3];
    me_bbox_fold(part, nb, lo, hi);
    double flat = 0.0;
    for (int a = 0; a < 3; ++a) {
        const double ext = hi[a] - lo[a];
        if (!(ext > 0.0)) flat = 1.0;
        const double scale = (double)(res - 1) / ext;
        prm[a] = scale;
        prm[3 + a] = 0.5 - scale * lo[a];
    }
    prm[6] = flat;
}

// (int) truncation of a rescaled coordinate clamped to [0, res-1] (triangle_hash.pyx:36-41); the pre-clamp of the double
// keeps the conversion defined and does not change the clamped result
__device__ __forceinline__ int me_cell_coord(double v, int res) {
    const int c = (int)fmin(fmax(v, -1.0), (double)res);
    return min(max(c, 0), res - 1);
}
__device__ __forceinline__ void me_tri_box(const double* t, int res, int& x0, int& x1, int& y0, int& y1) {
    x0 = me_cell_coord(fmin(fmin(t[0], t[3]), t[6]), res);
    x1 = me_cell_coord(fmax(fmax(t[0], t[3]), t[6]), res);
    y0 = me_cell_coord(fmin(fmin(t[1], t[4]), t[7]), res);
    y1 = me_cell_coord(fmax(fmax(t[1], t[4]), t[7]), res);
}

// rescale (inside_mesh.py:20, 135-137: scale * x + translate, two roundings) + count the cells of each triangle's box
__global__ __launch_bounds__(ME_BLOCK) void me_rescale_count_kernel(const double* __restrict__ verts, long nv,
                                                                   const long long* __restrict__ faces, long nf,
                                                                   const double* __restrict__ prm, double* __restrict__ tri,
                                                                   unsigned* __restrict__ cnt, int res) {
    const long f = (long)blockIdx.x * ME_BLOCK + threadIdx.x;
    if (f >= nf || prm[6] != 0.0) return;
    double t[9];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const long long vi = faces[3 * f + k];
        if (vi < 0 || vi >= nv) return;                 // reported by the bbox pass
#pragma unroll
        for (int a = 0; a < 3; ++a) t[3 * k + a] = prm[a] * verts[3 * vi + a] + prm[3 + a];
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) tri[9 * f + k] = t[k];
    int x0, x1, y0, y1;
    me_tri_box(t, res, x0, x1, y0, y1);
    for (int x = x0; x <= x1; ++x)
        for (int y = y0; y <= y1; ++y) atomicAdd(&cnt[(long)res * x + y], 1u);
}
// cell lists: entries[off[c] ..) = the triangles whose box covers cell c, in arrival order (only parities are counted)
__global__ __launch_bounds__(ME_BLOCK) void me_fill_kernel(const double* __restrict__ tri, long nf,
                                                          const double* __restrict__ prm, const long long* __restrict__ off,
                                                          unsigned* __restrict__ cur, int* __restrict__ entries,
                                                          long long n_entries, int res) {
    const long f = (long)blockIdx.x * ME_BLOCK + threadIdx.x;
    if (f >= nf || prm[6] != 0.0) return;
    double t[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) t[k] = tri[9 * f + k];
    int x0, x1, y0, y1;
    me_tri_box(t, res, x0, x1, y0, y1);
    for (int x = x0; x <= x1; ++x)
        for (int y = y0; y <= y1; ++y) {
            const long c = (long)res * x + y;
            const long long slot = off[c] + atomicAdd(&cur[c], 1u);
            if (slot < off[c + 1] && slot < n_entries) entries[slot] = (int)f;
        }
}

// one thread per point: inside_mesh.py:30-71 (bbox cull, depth parities), :74-104 (depth), :120-139 (2-D test),
// triangle_hash.pyx:60-71 (cell lookup)
template <typename P>
__global__ __launch_bounds__(ME_BLOCK) void me_contains_kernel(const P* __restrict__ pts, long n,
                                                              const double* __restrict__ prm,
                                                              const double* __restrict__ tri,
                                                              const long long* __restrict__ off,
                                                              const int* __restrict__ entries, long long n_entries,
                                                              long nf, int res, unsigned char* __restrict__ inside,
                                                              unsigned long long* __restrict__ n_disagree) {
    const long i = (long)blockIdx.x * ME_BLOCK + threadIdx.x;
    if (i >= n) return;
    bool in = false, odd_mismatch = false;
    if (prm[6] == 0.0) {
        const double px = prm[0] * (double)pts[3 * i + 0] + prm[3];
        const double py = prm[1] * (double)pts[3 * i + 1] + prm[4];
        const double pz = prm[2] * (double)pts[3 * i + 2] + prm[5];
        const double r = (double)res;
        if (px >= 0.0 && px <= r && py >= 0.0 && py <= r && pz >= 0.0 && pz <= r) {
            const int x = (int)px, y = (int)py;
            unsigned n0 = 0, n1 = 0;
            if (x < res && y < res) {
                const long c = (long)res * x + y;
                const long long e1 = min(off[c + 1], n_entries);
                for (long long e = max(off[c], 0ll); e < e1; ++e) {
                    const int tf = entries[e];
                    if (tf < 0 || tf >= nf) continue;       // not reachable from a build + fill; never read past tri
                    const double* t = tri + 9L * tf;
                    const double t1x = t[0], t1y = t[1], t1z = t[2], t2x = t[3], t2y = t[4], t2z = t[5];
                    const double t3x = t[6], t3y = t[7], t3z = t[8];
                    // TriangleIntersector2d.check_triangles: A = [[t1-t3, t2-t3]] per axis, y = p - t3
                    const double a00 = t1x - t3x, a01 = t2x - t3x, a10 = t1y - t3y, a11 = t2y - t3y;
                    const double y0 = px - t3x, y1 = py - t3y;
                    const double det = a00 * a11 - a01 * a10;
                    if (det == 0.0) continue;
                    const double sd = det > 0.0 ? 1.0 : (det < 0.0 ? -1.0 : det);   // np.sign (NaN stays NaN)
                    const double ad = fabs(det);
                    const double u = (a11 * y0 - a01 * y1) * sd;
                    const double v = (-a10 * y0 + a00 * y1) * sd;
                    const double suv = u + v;
                    if (!(0.0 < u && u < ad && 0.0 < v && v < ad && 0.0 < suv && suv < ad)) continue;
                    // compute_intersection_depth: n = cross(t3 - t1, t2 - t1)
                    const double v1x = t3x - t1x, v1y = t3y - t1y, v1z = t3z - t1z;
                    const double v2x = t2x - t1x, v2y = t2y - t1y, v2z = t2z - t1z;
                    const double nx = v1y * v2z - v1z * v2y, ny = v1z * v2x - v1x * v2z, nz = v1x * v2y - v1y * v2x;
                    const double alpha = nx * (t1x - px) + ny * (t1y - py);
                    const double an = fabs(nz);
                    if (!(an != 0.0)) continue;                 // depth NaN: counts in neither direction
                    const double sn = nz > 0.0 ? 1.0 : -1.0;
                    const double depth = t1z * an + alpha * sn;
                    const double lim = pz * an;
                    n0 += depth >= lim;
                    n1 += depth < lim;
                }
            }
            const bool c0 = n0 & 1u, c1 = n1 & 1u;
            in = c0 && c1;
            odd_mismatch = c0 != c1;
        }
    }
    inside[i] = in ? 1 : 0;
    if (n_disagree && odd_mismatch) atomicAdd(n_disagree, 1ull);
}

static int contains_check(long nf, int res, const void* ws, size_t ws_bytes, ContainsWs& w, const char* what) {
    S3D_CHECK_ARG(nf >= 0 && nf < (1L << 31), "%s: %ld faces (at most 2^31 - 1)", what, nf);
    S3D_CHECK_ARG(res >= 2 && res <= ME_RES_MAX, "%s: hash_resolution %d outside [2, %d]", what, res, ME_RES_MAX);
    S3D_CHECK_ARG(ws != nullptr, "%s: null workspace", what);
    const size_t need = contains_layout(nf, res, w, nullptr);
    if (ws_bytes < need) {
        s3d_set_error("%s: workspace %zu < %zu bytes", what, ws_bytes, need);
        return S3D_E_WORKSPACE;
    }
    contains_layout(nf, res, w, (char*)ws);
    return 0;
}

extern "C" size_t s3d_mesh_contains_workspace_bytes(long n_faces, int hash_resolution) {
    if (n_faces < 0 || hash_resolution < 2 || hash_resolution > ME_RES_MAX) return 0;
    ContainsWs w;
    return contains_layout(n_faces, hash_resolution, w, nullptr);
}

extern "C" int s3d_mesh_contains_build(const double* vertices, long n_vertices, const long long* faces, long n_faces,
                                       int hash_resolution, void* workspace, size_t workspace_bytes, long* n_entries,
                                       void* stream) {
    hipStream_t st = (hipStream_t)stream;
    ContainsWs w;
    S3D_CHECK_ARG(n_entries != nullptr, "mesh_contains_build: null n_entries");
    S3D_CHECK_ARG(n_vertices >= 0 && (n_faces == 0 || (vertices && faces)), "mesh_contains_build: bad mesh");
    TRY_RET(contains_check(n_faces, hash_resolution, workspace, workspace_bytes, w, "mesh_contains_build"));
    const int res = hash_resolution;
    *n_entries = 0;
    S3D_HIP_TRY("mesh_contains_build", hipMemsetAsync(w.flags, 0, 16, st));
    S3D_HIP_TRY("mesh_contains_build", hipMemsetAsync(w.cnt, 0, (size_t)w.cells * 4, st));
    const int nb = (int)std::min<long>(ME_BBOX_BLOCKS, me_blocks(3 * n_faces));
    hipLaunchKernelGGL(me_bbox_partial_kernel, dim3(nb), dim3(ME_BLOCK), 0, st, vertices, n_vertices, faces, n_faces,
                       w.part, w.flags);
    hipLaunchKernelGGL(me_bbox_final_kernel, dim3(1), dim3(64), 0, st, w.part, nb, w.prm, res);
    if (n_faces > 0)
        ME_LAUNCH(me_rescale_count_kernel, n_faces, st, vertices, n_vertices, faces, n_faces, w.prm, w.tri, w.cnt, res);
    return me_lists_finish("mesh_contains_build", w.cnt, w.off, w.cells, w.tsum, w.flags, n_vertices, n_entries, st);
}

extern "C" int s3d_mesh_contains_fill(long n_faces, int hash_resolution, void* workspace, size_t workspace_bytes,
                                      int* entries, long n_entries, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    ContainsWs w;
    S3D_CHECK_ARG(n_entries >= 0 && (n_entries == 0 || entries), "mesh_contains_fill: bad argument");
    TRY_RET(contains_check(n_faces, hash_resolution, workspace, workspace_bytes, w, "mesh_contains_fill"));
    if (n_faces == 0 || n_entries == 0) return 0;
    S3D_HIP_TRY("mesh_contains_fill", hipMemsetAsync(w.cnt, 0, (size_t)w.cells * 4, st));
    ME_LAUNCH(me_fill_kernel, n_faces, st, w.tri, n_faces, w.prm, w.off, w.cnt, entries, (long long)n_entries, hash_resolution);
    S3D_LAUNCH_CHECK();
    return 0;
}

extern "C" int s3d_mesh_contains_query(long n_faces, int hash_resolution, const void* workspace, size_t workspace_bytes,
                                       const int* entries, long n_entries, const void* points, int is_f64,
                                       long n_points, unsigned char* inside, unsigned long long* n_disagree,
                                       void* stream) {
    hipStream_t st = (hipStream_t)stream;
    ContainsWs w;
    S3D_CHECK_ARG(n_points >= 0 && (n_points == 0 || (points && inside)), "mesh_contains_query: bad argument");
    S3D_CHECK_ARG(n_entries >= 0 && (n_entries == 0 || entries), "mesh_contains_query: bad entries");
    TRY_RET(contains_check(n_faces, hash_resolution, workspace, workspace_bytes, w, "mesh_contains_query"));
    if (n_disagree) S3D_HIP_TRY("mesh_contains_query", hipMemsetAsync(n_disagree, 0, 8, st));
    if (n_points == 0) return 0;
    if (is_f64)
        ME_LAUNCH(me_contains_kernel<double>, n_points, st, (const double*)points, n_points, w.prm, w.tri, w.off, entries,
                  (long long)n_entries, n_faces, hash_resolution, inside, n_disagree);
    else
        ME_LAUNCH(me_contains_kernel<float>, n_points, st, (const float*)points, n_points, w.prm, w.tri, w.off, entries,
                  (long long)n_entries, n_faces, hash_resolution, inside, n_disagree);
    S3D_LAUNCH_CHECK();
    return 0;
}

// =============================================================================================
// exact nearest neighbour (brute force over LDS tiles of B; split over B, merged by one 64-bit atomicMin per split)
// =============================================================================================
#define NN_PPT 4                           // points of A per thread
#define NN_TILE ME_BLOCK                   // points of B per LDS tile
#define NN_A_PER_BLOCK (ME_BLOCK * NN_PPT)

__global__ void nn_init_kernel(unsigned long long* best, long n) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) best[i] = ~0ull;
}
// best[i] = min over this split's j of (bits(d2) << 32 | j): d2 >= 0, so the float's bit pattern orders like its value and
// the packed minimum is the smallest distance, then the lowest index — the same for every split count and arrival order
__global__ __launch_bounds__(ME_BLOCK) void nn_kernel(const float* __restrict__ a, long na, const float* __restrict__ b,
                                                     long nb, long per_split, unsigned long long* __restrict__ best) {
    __shared__ f32x4 sb[NN_TILE];
    float ax[NN_PPT], ay[NN_PPT], az[NN_PPT], bd[NN_PPT];
    int bj[NN_PPT];
    const long j0 = (long)blockIdx.y * per_split, j1 = min(nb, j0 + per_split);
#pragma unroll
    for (int k = 0; k < NN_PPT; ++k) {
        const long i = (long)blockIdx.x * NN_A_PER_BLOCK + k * ME_BLOCK + threadIdx.x;
        const long ic = i < na ? i : na - 1;
        ax[k] = a[3 * ic];
        ay[k] = a[3 * ic + 1];
        az[k] = a[3 * ic + 2];
        bd[k] = INFINITY;
        bj[k] = (int)j0;
    }
    for (long t0 = j0; t0 < j1; t0 += NN_TILE) {
        __syncthreads();
        const long j = t0 + threadIdx.x;
        if (j < j1) sb[threadIdx.x] = f32x4{b[3 * j], b[3 * j + 1], b[3 * j + 2], 0.f};
        __syncthreads();
        const int m = (int)min((long)NN_TILE, j1 - t0);
#pragma unroll 4
        for (int jj = 0; jj < m; ++jj) {
            const f32x4 q = sb[jj];
#pragma unroll
            for (int k = 0; k < NN_PPT; ++k) {
                const float dx = ax[k] - q[0], dy = ay[k] - q[1], dz = az[k] - q[2];
                const float d = __fmaf_rn(dz, dz, __fmaf_rn(dy, dy, dx * dx));
                if (d < bd[k]) {
                    bd[k] = d;
                    bj[k] = (int)t0 + jj;
                }
            }
        }
    }
#pragma unroll
    for (int k = 0; k < NN_PPT; ++k) {
        const long i = (long)blockIdx.x * NN_A_PER_BLOCK + k * ME_BLOCK + threadIdx.x;
        if (i < na)
            atomicMin(&best[i], ((unsigned long long)__float_as_uint(bd[k]) << 32) | (unsigned)bj[k]);
    }
}
__global__ void nn_unpack_kernel(const unsigned long long* __restrict__ best, long n, float* __restrict__ d2,
                                 long long* __restrict__ idx) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const unsigned long long v = best[i];
    d2[i] = __uint_as_float((unsigned)(v >> 32));
    if (idx) idx[i] = (long long)(v & 0xffffffffull);
}

extern "C" size_t s3d_nn_workspace_bytes(long na) { return na < 0 ? 0 : me_align((size_t)std::max(na, 1L) * 8); }

extern "C" int s3d_nn_sqdist(const float* a, long na, const float* b, long nb, void* workspace, size_t workspace_bytes,
                             float* d2, long long* idx, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    S3D_CHECK_ARG(na >= 0 && nb >= 1, "nn_sqdist: na = %ld, nb = %ld (nb must be >= 1)", na, nb);
    S3D_CHECK_ARG(nb < (1L << 31) && na < (1L << 40), "nn_sqdist: nb = %ld (at most 2^31 - 1)", nb);
    if (na == 0) return 0;
    S3D_CHECK_ARG(a && b && d2 && workspace, "nn_sqdist: null pointer");
    if (workspace_bytes < s3d_nn_workspace_bytes(na)) {
        s3d_set_error("nn_sqdist: workspace %zu < %zu bytes", workspace_bytes, s3d_nn_workspace_bytes(na));
        return S3D_E_WORKSPACE;
    }
    unsigned long long* best = (unsigned long long*)workspace;
    const long blocks_a = (na + NN_A_PER_BLOCK - 1) / NN_A_PER_BLOCK;
    // enough blocks to fill 256 CUs x 8 waves per SIMD, each split at least one tile of B
    long splits = std::min<long>((2048 + blocks_a - 1) / blocks_a, (nb + NN_TILE - 1) / NN_TILE);
    splits = std::max<long>(1, std::min<long>(splits, 65535));
    const long per_split = ((nb + splits - 1) / splits + NN_TILE - 1) / NN_TILE * NN_TILE;
    splits = (nb + per_split - 1) / per_split;
    ME_LAUNCH(nn_init_kernel, na, st, best, na);
    hipLaunchKernelGGL(nn_kernel, dim3((unsigned)blocks_a, (unsigned)splits), dim3(ME_BLOCK), 0, st, a, na, b, nb, per_split,
                       best);
    ME_LAUNCH(nn_unpack_kernel, na, st, best, na, d2, idx);
    S3D_LAUNCH_CHECK();
    return 0;
}

// =============================================================================================
// area-weighted surface sampling
// =============================================================================================
__device__ __forceinline__ unsigned long long me_mix64(unsigned long long z) {   // splitmix64's finaliser
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
// uniform in [0, 1) from 53 bits of the hash of (seed, sample, stream c)
__device__ __forceinline__ double me_uniform(unsigned long long key, long i, int c) {
    return (double)(me_mix64(key + 3ull * (unsigned long long)i + (unsigned long long)c) >> 11) * 0x1.0p-53;
}
__global__ void me_area_kernel(const double* __restrict__ verts, long nv, const long long* __restrict__ faces, long nf,
                               double* __restrict__ area) {
    const long f = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= nf) return;
    const long long i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
    double ar = 0.0;
    if (i0 >= 0 && i0 < nv && i1 >= 0 && i1 < nv && i2 >= 0 && i2 < nv) {
        const double* A = verts + 3 * i0;
        const double* B = verts + 3 * i1;
        const double* C = verts + 3 * i2;
        const double ux = B[0] - A[0], uy = B[1] - A[1], uz = B[2] - A[2];
        const double vx = C[0] - A[0], vy = C[1] - A[1], vz = C[2] - A[2];
        const double cx = uy * vz - uz * vy, cy = uz * vx - ux * vz, cz = ux * vy - uy * vx;
        ar = 0.5 * sqrt(cx * cx + cy * cy + cz * cz);
        if (!(ar > 0.0)) ar = 0.0;                      // NaN coordinates: never chosen
    }
    area[f] = ar;
}
__global__ void me_sample_kernel(const double* __restrict__ verts, const long long* __restrict__ faces, long nf,
                                 const double* __restrict__ area, const double* __restrict__ cdf, long n,
                                 unsigned long long key, float* __restrict__ out, long long* __restrict__ face_idx) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double total = cdf[nf - 1];
    const double x = me_uniform(key, i, 0) * total;
    // first face with cdf > x (zero-area faces repeat the cdf of the face before and are never first)
    long lo = 0, hi = nf;
    while (lo < hi) {
        const long mid = (lo + hi) >> 1;
        if (cdf[mid] > x) hi = mid;
        else lo = mid + 1;
    }
    long f = lo < nf ? lo : nf - 1;
    // the tiled scan rounds tile and thread boundaries on their own, so a zero-area face there can sit one ulp above its
    // predecessor: step to the nearest face with area
    while (f < nf - 1 && !(area[f] > 0.0)) ++f;
    while (f > 0 && !(area[f] > 0.0)) --f;
    if (!(total > 0.0) || !(area[f] > 0.0)) {
        out[3 * i] = out[3 * i + 1] = out[3 * i + 2] = NAN;
        face_idx[i] = -1;
        return;
    }
    const double s = sqrt(me_uniform(key, i, 1)), r2 = me_uniform(key, i, 2);
    const double wa = 1.0 - s, wb = s * (1.0 - r2), wc = s * r2;
    const double* A = verts + 3 * faces[3 * f];
    const double* B = verts + 3 * faces[3 * f + 1];
    const double* C = verts + 3 * faces[3 * f + 2];
#pragma unroll
    for (int c = 0; c < 3; ++c) out[3 * i + c] = (float)(wa * A[c] + wb * B[c] + wc * C[c]);
    face_idx[i] = f;
}

extern "C" size_t s3d_surface_sample_workspace_bytes(long n_faces) {
    if (n_faces < 0) return 0;
    const long tiles = (n_faces + ME_TILE - 1) / ME_TILE;
    return 2 * me_align((size_t)std::max(n_faces, 1L) * 8) + me_align((size_t)(tiles + 1) * 8);
}

extern "C" int s3d_surface_sample(const double* vertices, long n_vertices, const long long* faces, long n_faces,
                                  long n_samples, unsigned long long seed, void* workspace, size_t workspace_bytes,
                                  float* points, long long* face_idx, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    S3D_CHECK_ARG(n_faces >= 1 && n_vertices >= 1 && n_samples >= 0, "surface_sample: %ld faces, %ld vertices, %ld samples",
                  n_faces, n_vertices, n_samples);
    S3D_CHECK_ARG(vertices && faces && workspace, "surface_sample: null pointer");
    S3D_CHECK_ARG(n_samples == 0 || (points && face_idx), "surface_sample: null output");
    if (workspace_bytes < s3d_surface_sample_workspace_bytes(n_faces)) {
        s3d_set_error("surface_sample: workspace %zu < %zu bytes", workspace_bytes, s3d_surface_sample_workspace_bytes(n_faces));
        return S3D_E_WORKSPACE;
    }
    if (n_samples == 0) return 0;
    double* area = (double*)workspace;
    double* cdf = (double*)((char*)workspace + me_align((size_t)n_faces * 8));
    double* tsum = (double*)((char*)workspace + 2 * me_align((size_t)n_faces * 8));
    ME_LAUNCH(me_area_kernel, n_faces, st, vertices, n_vertices, faces, n_faces, area);
    me_scan<double, double, true>(area, cdf, n_faces, tsum, st);
    // the key mixes the seed once, so seeds s and s + 1 do not give streams shifted by one sample
    const unsigned long long key = (seed ^ 0x5851F42D4C957F2Dull) * 0xD1342543DE82EF95ull;
    ME_LAUNCH(me_sample_kernel, n_samples, st, vertices, faces, n_faces, area, cdf, n_samples, key, points, face_idx);
    S3D_LAUNCH_CHECK();
    return 0;
}

// mesh_sdf.hip — signed-distance training targets from a triangle mesh on the device: the two halves of a signed distance
// that the point-in-mesh test of mesh_eval.hip does not give.
//
//   exact distance:   for every point the minimum over ALL faces of the point-triangle distance (float64), found through a
//                     uniform 3-D cell grid: cells are visited in shells of growing Chebyshev radius around the point's
//                     (clamped) cell until the lower bound of everything not yet visited exceeds the best distance.
//   winding number:   w(p) = sum over faces of the solid angle / 4 pi (Van Oosterom & Strackee's atan2 form), the notion of
//                     "inside" that still means something on a mesh that is not watertight.
//
// There is no counterpart in the reference's tree: its README points to an external CPU script for 02_sdfs/<shape>.npy;
// reg_slices/src/datasets.py:142-148 is the consumer that fixes the file format.
//
// Determinism.  A face's squared distance to a point is one fixed operation sequence (sd_point_tri2: explicit fma in the dot
// products, everything else rounded on its own: the file is compiled with -ffp-contract=off), the result is the
// lexicographic minimum of (squared distance, face index) over the faces visited, and the search provably visits every
// face that can attain the minimum — so dist and face are the same bits for every grid resolution, float32 points equal
// their widened float64 copies, and the order of the cell lists (atomics) does not matter.  The winding number sums fixed
// chunks of faces (a function of n_faces alone) in face order and the chunk sums in chunk order, whatever the launch
// geometry.
#include <math.h>
#include <string.h>

#include <algorithm>

#include "mesh_common.h"

#define SD_RES_MAX 256                      // res^3 cells: 16.7 M at most
#define SD_SKIP_NONE 65535u                 // "no occupied cell on this line / plane / grid"

// =============================================================================================
// exact point-to-mesh distance
// =============================================================================================
// prm: lo[3], hi[3], h[3] (cell size), inv_h[3], ra[3] (cells in use on the axis: res, or 1 where the box is flat)
#define SD_LO 0
#define SD_HI 3
#define SD_H 6
#define SD_IH 9
#define SD_RA 12
#define SD_PRM 16

struct DistWs {
    double* part;          // [ME_BBOX_BLOCKS][6] partial (min xyz, max xyz)
    double* prm;           // [SD_PRM]
    int* flags;            // [0]: a face index outside [0, n_vertices)
    double* tri;           // [n_faces][9] gathered triangles
    unsigned* cnt;         // [cells] triangles per cell, then the fill cursors
    long long* off;        // [cells + 1] first entry of each cell
    long long* tsum;       // [tiles + 1]
    unsigned short* skip;  // [cells] Chebyshev distance (in cells) to the nearest occupied cell
    unsigned short* tmp;   // [cells] the transform's second buffer
    long cells;
};
// the arrays in the workspace's order; base == nullptr: only the size
static size_t dist_layout(long nf, int res, DistWs& w, char* base) {
    MeArena a{base};
    w.cells = (long)res * res * res;
    const long tiles = (w.cells + ME_TILE - 1) / ME_TILE;
    w.part = a.take<double>(ME_BBOX_BLOCKS * 6), w.prm = a.take<double>(SD_PRM), w.flags = a.take<int>(4);
    w.tri = a.take<double>(9 * (size_t)nf), w.cnt = a.take<unsigned>(w.cells), w.off = a.take<long long>(w.cells + 1);
    w.tsum = a.take<long long>(tiles + 1), w.skip = a.take<unsigned short>(w.cells), w.tmp = a.take<unsigned short>(w.cells);
    return a.off;
}

// the grid: res cells per axis over the bounding box; an axis on which the box is flat (or so thin that res / extent
// overflows) has one cell
__global__ void sd_grid_kernel(const double* __restrict__ part, int nb, double* __restrict__ prm, int res) {
    if (threadIdx.x != 0) return;
    double lo[3], hi[3];
    me_bbox_fold(part, nb, lo, hi);
    for (int a = 0; a < 3; ++a) {
        const double ext = hi[a] - lo[a];
        const double ih = (double)res / ext, h = ext / (double)res;
        const bool ok = ext > 0.0 && ih < INFINITY && h > 0.0;     // false for NaN, too
        prm[SD_LO + a] = lo[a];
        prm[SD_HI + a] = hi[a];
        prm[SD_H + a] = ok ? h : 0.0;
        prm[SD_IH + a] = ok ? ih : 0.0;
        prm[SD_RA + a] = ok ? (double)res : 1.0;
    }
}

// cell of a coordinate, clamped to [0, ra - 1]; monotone in x (NaN -> 0)
__device__ __forceinline__ int sd_cell(double x, double lo, double ih, int ra) {
    return (int)fmin(fmax((x - lo) * ih, 0.0), (double)(ra - 1));
}
struct SdGrid {
    double lo[3], hi[3], h[3], ih[3];
    int ra[3];
};
__device__ __forceinline__ void sd_load_grid(const double* __restrict__ prm, SdGrid& g) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        g.lo[a] = prm[SD_LO + a];
        g.hi[a] = prm[SD_HI + a];
        g.h[a] = prm[SD_H + a];
        g.ih[a] = prm[SD_IH + a];
        g.ra[a] = (int)prm[SD_RA + a];
    }
}
__device__ __forceinline__ void sd_tri_cells(const double* t, const SdGrid& g, int* c0, int* c1) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        c0[a] = sd_cell(fmin(fmin(t[a], t[3 + a]), t[6 + a]), g.lo[a], g.ih[a], g.ra[a]);
        c1[a] = sd_cell(fmax(fmax(t[a], t[3 + a]), t[6 + a]), g.lo[a], g.ih[a], g.ra[a]);
    }
}

// gather the triangles + count the cells of each triangle's box
__global__ __launch_bounds__(ME_BLOCK) void sd_gather_count_kernel(const double* __restrict__ verts, long nv,
                                                                  const long long* __restrict__ faces, long nf,
                                                                  const double* __restrict__ prm, double* __restrict__ tri,
                                                                  unsigned* __restrict__ cnt, int res) {
    const long f = (long)blockIdx.x * ME_BLOCK + threadIdx.x;
    if (f >= nf) return;
    double t[9];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const long long vi = faces[3 * f + k];
        if (vi < 0 || vi >= nv) return;                 // reported by the bbox pass
#pragma unroll
        for (int a = 0; a < 3; ++a) t[3 * k + a] = verts[3 * vi + a];
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) tri[9 * f + k] = t[k];
    SdGrid g;
    sd_load_grid(prm, g);
    int c0[3], c1[3];
    sd_tri_cells(t, g, c0, c1);
    for (int x = c0[0]; x <= c1[0]; ++x)
        for (int y = c0[1]; y <= c1[1]; ++y)
            for (int z = c0[2]; z <= c1[2]; ++z) atomicAdd(&cnt[((long)x * res + y) * res + z], 1u);
}
// cell lists: entries[off[c] ..) = the triangles whose box overlaps cell c, in arrival order (the query takes a
// lexicographic minimum, so the order does not reach its result)
__global__ __launch_bounds__(ME_BLOCK) void sd_fill_kernel(const double* __restrict__ tri, long nf,
                                                          const double* __restrict__ prm, const long long* __restrict__ off,
                                                          unsigned* __restrict__ cur, int* __restrict__ entries,
                                                          long long n_entries, int res) {
    const long f = (long)blockIdx.x * ME_BLOCK + threadIdx.x;
    if (f >= nf) return;
    double t[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) t[k] = tri[9 * f + k];
    SdGrid g;
    sd_load_grid(prm, g);
    int c0[3], c1[3];
    sd_tri_cells(t, g, c0, c1);
    for (int x = c0[0]; x <= c1[0]; ++x)
        for (int y = c0[1]; y <= c1[1]; ++y)
            for (int z = c0[2]; z <= c1[2]; ++z) {
                const long c = ((long)x * res + y) * res + z;
                const long long slot = off[c] + atomicAdd(&cur[c], 1u);
                if (slot < off[c + 1] && slot < n_entries) entries[slot] = (int)f;
            }
}

// One axis of the Chebyshev distance transform: out(c) = min over the cells q of c's line along `axis` of
// max(|q - pos|, in(q)), where in = 0 / SD_SKIP_NONE from the cell counts on the first pass.  min-max separates, so three
// passes (x, y, z) leave min over occupied cells o of max_a |c_a - o_a|.
__global__ __launch_bounds__(ME_BLOCK) void sd_skip_pass_kernel(const unsigned* __restrict__ cnt,
                                                               const unsigned short* __restrict__ in,
                                                               unsigned short* __restrict__ out,
                                                               const double* __restrict__ prm, int res, int axis) {
    const long c = (long)blockIdx.x * ME_BLOCK + threadIdx.x;
    if (c >= (long)res * res * res) return;
    const int z = (int)(c % res), y = (int)((c / res) % res), x = (int)(c / ((long)res * res));
    const int rx = (int)prm[SD_RA], ry = (int)prm[SD_RA + 1], rz = (int)prm[SD_RA + 2];
    if (x >= rx || y >= ry || z >= rz) {                // outside the cells in use: never read
        out[c] = (unsigned short)SD_SKIP_NONE;
        return;
    }
    const int n = axis == 0 ? rx : (axis == 1 ? ry : rz), pos = axis == 0 ? x : (axis == 1 ? y : z);
    const long stride = axis == 0 ? (long)res * res : (axis == 1 ? res : 1);
    const long base = c - pos * stride;
    unsigned best = SD_SKIP_NONE;
    for (int q = 0; q < n; ++q) {
        const unsigned v = cnt ? (cnt[base + q * stride] ? 0u : SD_SKIP_NONE) : (unsigned)in[base + q * stride];
        const unsigned d = (unsigned)abs(q - pos);
        best = min(best, max(d, v));
    }
    out[c] = (unsigned short)best;
}

__device__ __forceinline__ double sd_dot(double ax, double ay, double az, double bx, double by, double bz) {
    return fma(az, bz, fma(ay, by, ax * bx));
}
// squared distance from p to the segment a + s * e, s in [0, 1], given ap = p - a; e = 0 is the point a
__device__ __forceinline__ double sd_point_seg2(double apx, double apy, double apz, double ex, double ey, double ez) {
    const double t = sd_dot(apx, apy, apz, ex, ey, ez), den = sd_dot(ex, ey, ez, ex, ey, ez);
    if (t <= 0.0) return sd_dot(apx, apy, apz, apx, apy, apz);
    if (t >= den) {
        const double bx = apx - ex, by = apy - ey, bz = apz - ez;
        return sd_dot(bx, by, bz, bx, by, bz);
    }
    const double s = t / den;
    const double dx = apx - s * ex, dy = apy - s * ey, dz = apz - s * ez;
    return sd_dot(dx, dy, dz, dx, dy, dz);
}
// Squared distance from p to the triangle (a, b, c): the minimum over its three edge segments and, where p projects
// strictly inside (the three barycentric numerators of Ericson's classification all positive), the foot of the
// perpendicular, taken as a convex combination of the vertices.  Every candidate is a point of the triangle, so a
// degenerate face is the segment or point it collapses to: its edges are still there, and the interior candidate is
// either absent or one more point of the same segment.  A NaN candidate never wins a comparison.
__device__ __forceinline__ double sd_point_tri2(double px, double py, double pz, const double* __restrict__ t) {
    const double ax = t[0], ay = t[1], az = t[2];
    const double abx = t[3] - ax, aby = t[4] - ay, abz = t[5] - az;
    const double acx = t[6] - ax, acy = t[7] - ay, acz = t[8] - az;
    const double bcx = t[6] - t[3], bcy = t[7] - t[4], bcz = t[8] - t[5];
    const double apx = px - ax, apy = py - ay, apz = pz - az;
    const double bpx = px - t[3], bpy = py - t[4], bpz = pz - t[5];
    const double cpx = px - t[6], cpy = py - t[7], cpz = pz - t[8];
    double m = sd_point_seg2(apx, apy, apz, abx, aby, abz);
    const double e1 = sd_point_seg2(bpx, bpy, bpz, bcx, bcy, bcz);
    if (e1 < m) m = e1;
    const double e2 = sd_point_seg2(apx, apy, apz, acx, acy, acz);
    if (e2 < m) m = e2;
    const double d1 = sd_dot(abx, aby, abz, apx, apy, apz), d2 = sd_dot(acx, acy, acz, apx, apy, apz);
    const double d3 = sd_dot(abx, aby, abz, bpx, bpy, bpz), d4 = sd_dot(acx, acy, acz, bpx, bpy, bpz);
    const double d5 = sd_dot(abx, aby, abz, cpx, cpy, cpz), d6 = sd_dot(acx, acy, acz, cpx, cpy, cpz);
    const double vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
    if (va > 0.0 && vb > 0.0 && vc > 0.0) {
        const double sum = va + vb + vc;
        const double v = vb / sum, w = vc / sum;
        const double dx = apx - v * abx - w * acx, dy = apy - v * aby - w * acy, dz = apz - v * abz - w * acz;
        const double e3 = sd_dot(dx, dy, dz, dx, dy, dz);
        if (e3 < m) m = e3;
    }
    return m;
}

// Lower bound, per axis, on |p_a - q_a| for any point q of the mesh whose cell on the axis is >= j (side = +1) or < j
// (side = -1): the cell function is monotone and its j-th boundary is lo + j*h up to a few roundings of magnitudes
// |lo|, |hi|, so the bound is cut by `slack` = 2^-40 (|lo| + |hi| + |p|), a thousand times those roundings and the
// rounding of a face's own computed distance.  Never negative; NaN -> 0 (no pruning).
__device__ __forceinline__ double sd_gap_hi(double p, double lo, double h, int j, double slack) {
    return fmax((lo + (double)j * h) - p - slack, 0.0);
}
__device__ __forceinline__ double sd_gap_lo(double p, double lo, double h, int j, double slack) {
    return fmax(p - (lo + (double)j * h) - slack, 0.0);
}

// lower bound on |p_a - q_a| for a point q of the mesh in cell j of an axis with ra cells (the last cell has no far side)
__device__ __forceinline__ double sd_cell_gap(double p, double lo, double h, int ra, int j, double slack) {
    return fmax(sd_gap_hi(p, lo, h, j, slack), j + 1 < ra ? sd_gap_lo(p, lo, h, j + 1, slack) : 0.0);
}

// One thread per point.  Shell k = the cells at Chebyshev distance k from the point's clamped cell; the search starts at
// the first shell that holds an occupied cell (skip table), walks each shell as runs along z or y and jumps over their
// empty stretches with the same table, drops
// a cell whose box is farther than the best distance (a face is listed in the cell of its own closest point, so the face
// that attains the minimum is never dropped), and stops after shell k once everything listed only in shells > k is
// farther than the best distance.  k never exceeds the grid size.
template <typename P>
__global__ __launch_bounds__(ME_BLOCK) void sd_query_kernel(const P* __restrict__ pts, long n, const double* __restrict__ prm,
                                                           const double* __restrict__ tri,
                                                           const long long* __restrict__ off,
                                                           const unsigned short* __restrict__ skip,
                                                           const int* __restrict__ entries, long long n_entries, long nf,
                                                           int res, double* __restrict__ dist, long long* __restrict__ face,
                                                           unsigned long long* __restrict__ n_tests) {
    const long i = (long)blockIdx.x * ME_BLOCK + threadIdx.x;
    unsigned long long tests = 0;
    if (i < n) {
        SdGrid g;
        sd_load_grid(prm, g);
        const double p[3] = {(double)pts[3 * i], (double)pts[3 * i + 1], (double)pts[3 * i + 2]};
        int c[3];
        double slack[3];
        int kmax = 0;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            c[a] = sd_cell(p[a], g.lo[a], g.ih[a], g.ra[a]);
            slack[a] = 0x1p-40 * (fabs(g.lo[a]) + fabs(g.hi[a]) + fabs(p[a]));
            kmax = max(kmax, max(c[a], g.ra[a] - 1 - c[a]));
        }
        double best = INFINITY;
        long long bf = -1;
        const int k0 = min((int)skip[((long)c[0] * res + c[1]) * res + c[2]], kmax);
        for (int k = k0; k <= kmax; ++k) {
            const int x0 = max(c[0] - k, 0), x1 = min(c[0] + k, g.ra[0] - 1);
            const int y0 = max(c[1] - k, 0), y1 = min(c[1] + k, g.ra[1] - 1);
            const int z0 = max(c[2] - k, 0), z1 = min(c[2] + k, g.ra[2] - 1);
            for (int x = x0; x <= x1; ++x) {
                const double gx = sd_cell_gap(p[0], g.lo[0], g.h[0], g.ra[0], x, slack[0]);
                if (gx * gx > best) continue;
                // The slab's cells of shell k as runs along one axis, so that the skip table can jump along every one of
                // them: on the shell's x sides a z-run for each y; otherwise the z-runs of the two y sides (lines 0, 1)
                // and, between them, a y-run on each of the two z caps (lines 2, 3).
                const bool xs = x == c[0] - k || x == c[0] + k;
                const int n_lines = xs ? y1 - y0 + 1 : 4;
                for (int li = 0; li < n_lines; ++li) {
                    const bool along_z = xs || li < 2;
                    int u, t0 = z0, t1 = z1;                    // the fixed coordinate, the run's range
                    if (xs) {
                        u = y0 + li;
                    } else {
                        u = (along_z ? c[1] : c[2]) + ((li & 1) ? k : -k);
                        if (u < 0 || u > (along_z ? g.ra[1] : g.ra[2]) - 1) continue;
                        if (!along_z) {
                            t0 = max(y0, c[1] - k + 1);
                            t1 = min(y1, c[1] + k - 1);
                        }
                    }
                    const double gu = along_z ? sd_cell_gap(p[1], g.lo[1], g.h[1], g.ra[1], u, slack[1])
                                              : sd_cell_gap(p[2], g.lo[2], g.h[2], g.ra[2], u, slack[2]);
                    const double gfix = gx * gx + gu * gu;
                    if (gfix > best) continue;
                    const double pt = along_z ? p[2] : p[1], lot = along_z ? g.lo[2] : g.lo[1];
                    const double ht = along_z ? g.h[2] : g.h[1], slt = along_z ? slack[2] : slack[1];
                    const int rat = along_z ? g.ra[2] : g.ra[1];
                    const long stride = along_z ? 1 : res;
                    const long base = (long)x * res * res + (along_z ? (long)u * res : (long)u);
                    for (int t = t0; t <= t1;) {
                        const long cell = base + t * stride;
                        const unsigned s = skip[cell];
                        if (s != 0) {                             // no occupied cell within Chebyshev distance s - 1
                            t += (int)s;
                            continue;
                        }
                        const double gt = sd_cell_gap(pt, lot, ht, rat, t, slt);
                        if (!(gfix + gt * gt > best)) {
                            const long long e1 = min(off[cell + 1], n_entries);
                            for (long long e = max(off[cell], 0ll); e < e1; ++e) {
                                const int tf = entries[e];
                                if (tf < 0 || tf >= nf) continue;   // not reachable from a build + fill; never read past tri
                                const double d2 = sd_point_tri2(p[0], p[1], p[2], tri + 9L * tf);
                                ++tests;
                                if (d2 < best || (d2 == best && tf < bf)) {
                                    best = d2;
                                    bf = tf;
                                }
                            }
                        }
                        ++t;
                    }
                }
            }
            if (k == kmax) break;
            double lb = INFINITY;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                if (c[a] + k + 1 <= g.ra[a] - 1) lb = fmin(lb, sd_gap_hi(p[a], g.lo[a], g.h[a], c[a] + k + 1, slack[a]));
                if (c[a] - k >= 1) lb = fmin(lb, sd_gap_lo(p[a], g.lo[a], g.h[a], c[a] - k, slack[a]));
            }
            if (lb * lb > best) break;
        }
        dist[i] = sqrt(best);
        if (face) face[i] = bf;
    }
    if (n_tests) {
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) tests += __shfl_down(tests, d, 64);
        if ((threadIdx.x & 63) == 0 && tests) atomicAdd(n_tests, tests);
    }
}

static int dist_check(long nf, int res, const void* ws, size_t ws_bytes, DistWs& w, const char* what) {
    S3D_CHECK_ARG(nf >= 1 && nf < (1L << 31), "%s: %ld faces (1 .. 2^31 - 1)", what, nf);
    S3D_CHECK_ARG(res >= 1 && res <= SD_RES_MAX, "%s: resolution %d outside [1, %d]", what, res, SD_RES_MAX);
    S3D_CHECK_ARG(ws != nullptr, "%s: null workspace", what);
    const size_t need = dist_layout(nf, res, w, nullptr);
    if (ws_bytes < need) {
        s3d_set_error("%s: workspace %zu < %zu bytes", what, ws_bytes, need);
        return S3D_E_WORKSPACE;
    }
    dist_layout(nf, res, w, (char*)ws);
    return 0;
}

extern "C" size_t s3d_mesh_dist_workspace_bytes(long n_faces, int resolution) {
    if (n_faces < 1 || n_faces >= (1L << 31) || resolution < 1 || resolution > SD_RES_MAX) return 0;
    DistWs w;
    return dist_layout(n_faces, resolution, w, nullptr);
}

extern "C" int s3d_mesh_dist_build(const double* vertices, long n_vertices, const long long* faces, long n_faces,
                                   int resolution, void* workspace, size_t workspace_bytes, long* n_entries, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    DistWs w;
    S3D_CHECK_ARG(n_entries != nullptr, "mesh_dist_build: null n_entries");
    S3D_CHECK_ARG(n_vertices >= 1 && vertices && faces, "mesh_dist_build: bad mesh");
    TRY_RET(dist_check(n_faces, resolution, workspace, workspace_bytes, w, "mesh_dist_build"));
    const int res = resolution;
    *n_entries = 0;
    S3D_HIP_TRY("mesh_dist_build", hipMemsetAsync(w.flags, 0, 16, st));
    S3D_HIP_TRY("mesh_dist_build", hipMemsetAsync(w.cnt, 0, (size_t)w.cells * 4, st));
    const int nb = (int)std::min<long>(ME_BBOX_BLOCKS, me_blocks(3 * n_faces));
    hipLaunchKernelGGL(me_bbox_partial_kernel, dim3(nb), dim3(ME_BLOCK), 0, st, vertices, n_vertices, faces, n_faces,
                       w.part, w.flags);
    hipLaunchKernelGGL(sd_grid_kernel, dim3(1), dim3(64), 0, st, w.part, nb, w.prm, res);
    ME_LAUNCH(sd_gather_count_kernel, n_faces, st, vertices, n_vertices, faces, n_faces, w.prm, w.tri, w.cnt, res);
    // x: counts -> skip, y: skip -> tmp, z: tmp -> skip (the passes read the counts, which the scan after them leaves alone)
    ME_LAUNCH(sd_skip_pass_kernel, w.cells, st, w.cnt, nullptr, w.skip, w.prm, res, 0);
    ME_LAUNCH(sd_skip_pass_kernel, w.cells, st, nullptr, w.skip, w.tmp, w.prm, res, 1);
    ME_LAUNCH(sd_skip_pass_kernel, w.cells, st, nullptr, w.tmp, w.skip, w.prm, res, 2);
    return me_lists_finish("mesh_dist_build", w.cnt, w.off, w.cells, w.tsum, w.flags, n_vertices, n_entries, st);
}

extern "C" int s3d_mesh_dist_fill(long n_faces, int resolution, void* workspace, size_t workspace_bytes, int* entries,
                                  long n_entries, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    DistWs w;
    S3D_CHECK_ARG(n_entries >= 0 && (n_entries == 0 || entries), "mesh_dist_fill: bad argument");
    TRY_RET(dist_check(n_faces, resolution, workspace, workspace_bytes, w, "mesh_dist_fill"));
    if (n_entries == 0) return 0;
    S3D_HIP_TRY("mesh_dist_fill", hipMemsetAsync(w.cnt, 0, (size_t)w.cells * 4, st));
    ME_LAUNCH(sd_fill_kernel, n_faces, st, w.tri, n_faces, w.prm, w.off, w.cnt, entries, (long long)n_entries, resolution);
    S3D_LAUNCH_CHECK();
    return 0;
}

extern "C" int s3d_mesh_dist_query(long n_faces, int resolution, const void* workspace, size_t workspace_bytes,
                                   const int* entries, long n_entries, const void* points, int is_f64, long n_points,
                                   double* dist, long long* face, unsigned long long* n_tests, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    DistWs w;
    S3D_CHECK_ARG(n_points >= 0 && (n_points == 0 || (points && dist)), "mesh_dist_query: bad argument");
    S3D_CHECK_ARG(n_entries >= 0 && (n_entries == 0 || entries), "mesh_dist_query: bad entries");
    TRY_RET(dist_check(n_faces, resolution, workspace, workspace_bytes, w, "mesh_dist_query"));
    if (n_tests) S3D_HIP_TRY("mesh_dist_query", hipMemsetAsync(n_tests, 0, 8, st));
    if (n_points == 0) return 0;
    if (is_f64)
        ME_LAUNCH(sd_query_kernel<double>, n_points, st, (const double*)points, n_points, w.prm, w.tri, w.off, w.skip, entries,
                  (long long)n_entries, n_faces, resolution, dist, face, n_tests);
    else
        ME_LAUNCH(sd_query_kernel<float>, n_points, st, (const float*)points, n_points, w.prm, w.tri, w.off, w.skip, entries,
                  (long long)n_entries, n_faces, resolution, dist, face, n_tests);
    S3D_LAUNCH_CHECK();
    return 0;
}

// =============================================================================================
// generalised winding number (brute force over LDS tiles of faces against a register block of points)
// =============================================================================================
#define WN_PPT 2                           // points per thread
#define WN_TILE 128                        // faces per LDS tile (9 float64 each)
#define WN_P_PER_BLOCK (ME_BLOCK * WN_PPT)
#define WN_CHUNKS_MAX 32                   // fixed chunks of faces: a function of n_faces alone
#define WN_BATCH (1L << 17)                // points per pass: bounds the partial sums kept in the workspace

static long wn_chunk_faces(long nf) {
    const long per = (nf + WN_CHUNKS_MAX - 1) / WN_CHUNKS_MAX;
    return std::max<long>(1, (per + WN_TILE - 1) / WN_TILE) * WN_TILE;
}

// Within ~1e-3 edge lengths of an edge both arguments of the atan2 go to zero together and the angle inherits their
// rounding amplified (measured on a unit square: 4e-14 against an 80-bit evaluation, for this kernel and for a numpy
// float64 evaluation alike).  The products and sums are therefore left unfused and in the textbook order, so that the
// arguments are the very numbers any plain IEEE float64 evaluation of the formula gets, and what remains between two
// such evaluations is their atan2 and the order of the sum.
__device__ __forceinline__ double wn_dot(double ax, double ay, double az, double bx, double by, double bz) {
    return ax * bx + ay * by + az * bz;
}
__global__ __launch_bounds__(ME_BLOCK) void wn_check_faces_kernel(const long long* __restrict__ faces, long nf, long nv,
                                                                 int* __restrict__ flags) {
    for (long i = (long)blockIdx.x * ME_BLOCK + threadIdx.x; i < 3 * nf; i += (long)gridDim.x * ME_BLOCK) {
        const long long vi = faces[i];
        if (vi < 0 || vi >= nv) flags[0] = 1;
    }
}
// part[chunk][i] = sum over the chunk's faces, in face order, of atan2(det[a b c], |a||b||c| + (a.b)|c| + (b.c)|a| +
// (c.a)|b|) with a, b, c the face's vertices relative to the point: half the face's signed solid angle.  blockIdx.y takes
// `cpb` consecutive chunks; each chunk's sum starts from zero, so the launch geometry does not reach the result.
template <typename P>
__global__ __launch_bounds__(ME_BLOCK) void wn_kernel(const P* __restrict__ pts, long n, const double* __restrict__ verts,
                                                     const long long* __restrict__ faces, long nf, long chunk, int n_chunks,
                                                     int cpb, double* __restrict__ part) {
    __shared__ double st[WN_TILE * 9];
    double px[WN_PPT], py[WN_PPT], pz[WN_PPT], acc[WN_PPT];
#pragma unroll
    for (int k = 0; k < WN_PPT; ++k) {
        const long i = (long)blockIdx.x * WN_P_PER_BLOCK + k * ME_BLOCK + threadIdx.x;
        const long ic = i < n ? i : n - 1;
        px[k] = (double)pts[3 * ic];
        py[k] = (double)pts[3 * ic + 1];
        pz[k] = (double)pts[3 * ic + 2];
    }
    const int ch1 = min(n_chunks, ((int)blockIdx.y + 1) * cpb);
    for (int ch = (int)blockIdx.y * cpb; ch < ch1; ++ch) {
        const long f0 = (long)ch * chunk, f1 = min(nf, f0 + chunk);
#pragma unroll
        for (int k = 0; k < WN_PPT; ++k) acc[k] = 0.0;
        for (long t0 = f0; t0 < f1; t0 += WN_TILE) {
            __syncthreads();
            const int m = (int)min((long)WN_TILE, f1 - t0);
            if ((int)threadIdx.x < m) {
                const long f = t0 + threadIdx.x;
#pragma unroll
                for (int v = 0; v < 3; ++v) {
                    const long long vi = faces[3 * f + v];       // checked by wn_check_faces_kernel before this launch
#pragma unroll
                    for (int a = 0; a < 3; ++a) st[threadIdx.x * 9 + 3 * v + a] = verts[3 * vi + a];
                }
            }
            __syncthreads();
            for (int jj = 0; jj < m; ++jj) {
                const double* q = st + 9 * jj;
#pragma unroll
                for (int k = 0; k < WN_PPT; ++k) {
                    const double ax = q[0] - px[k], ay = q[1] - py[k], az = q[2] - pz[k];
                    const double bx = q[3] - px[k], by = q[4] - py[k], bz = q[5] - pz[k];
                    const double cx = q[6] - px[k], cy = q[7] - py[k], cz = q[8] - pz[k];
                    const double la = sqrt(wn_dot(ax, ay, az, ax, ay, az)), lb = sqrt(wn_dot(bx, by, bz, bx, by, bz));
                    const double lc = sqrt(wn_dot(cx, cy, cz, cx, cy, cz));
                    const double det = ax * (by * cz - bz * cy) + ay * (bz * cx - bx * cz) + az * (bx * cy - by * cx);
                    const double den = la * lb * lc + wn_dot(ax, ay, az, bx, by, bz) * lc +
                                       wn_dot(bx, by, bz, cx, cy, cz) * la + wn_dot(cx, cy, cz, ax, ay, az) * lb;
                    acc[k] += atan2(det, den);
                }
            }
        }
#pragma unroll
        for (int k = 0; k < WN_PPT; ++k) {
            const long i = (long)blockIdx.x * WN_P_PER_BLOCK + k * ME_BLOCK + threadIdx.x;
            if (i < n) part[(long)ch * n + i] = acc[k];
        }
    }
}
// w = (sum of the chunk sums in chunk order) / 2 pi
__global__ void wn_sum_kernel(const double* __restrict__ part, long n, int n_chunks, double* __restrict__ w) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double s = 0.0;
    for (int ch = 0; ch < n_chunks; ++ch) s += part[(long)ch * n + i];
    w[i] = s / 6.283185307179586;
}

struct WindingWs {
    int* flags;            // [0]: a face index outside [0, n_vertices)
    double* part;          // [n_chunks][points of a pass] chunk sums
};
static size_t winding_layout(long nf, long n_points, WindingWs& w, char* base) {
    MeArena a{base};
    const long chunk = wn_chunk_faces(nf), n_chunks = (nf + chunk - 1) / chunk;
    w.flags = a.take<int>(4);
    w.part = a.take<double>((size_t)n_chunks * (size_t)std::max<long>(1, std::min(n_points, WN_BATCH)));
    return a.off;
}

extern "C" size_t s3d_mesh_winding_workspace_bytes(long n_faces, long n_points) {
    if (n_faces < 1 || n_points < 0) return 0;
    WindingWs w;
    return winding_layout(n_faces, n_points, w, nullptr);
}

extern "C" int s3d_mesh_winding(const double* vertices, long n_vertices, const long long* faces, long n_faces,
                                const void* points, int is_f64, long n_points, int n_splits, void* workspace,
                                size_t workspace_bytes, double* w, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    S3D_CHECK_ARG(n_faces >= 1 && n_faces < (1L << 31) && n_vertices >= 1, "mesh_winding: %ld faces, %ld vertices", n_faces,
                  n_vertices);
    S3D_CHECK_ARG(n_points >= 0 && n_splits >= 0, "mesh_winding: n_points = %ld, n_splits = %d", n_points, n_splits);
    S3D_CHECK_ARG(vertices && faces && workspace, "mesh_winding: null pointer");
    S3D_CHECK_ARG(n_points == 0 || (points && w), "mesh_winding: null points or output");
    WindingWs ws;
    const size_t need = winding_layout(n_faces, n_points, ws, (char*)workspace);
    if (workspace_bytes < need) {
        s3d_set_error("mesh_winding: workspace %zu < %zu bytes", workspace_bytes, need);
        return S3D_E_WORKSPACE;
    }
    if (n_points == 0) return 0;
    int* const flags = ws.flags;
    double* const part = ws.part;
    // the faces are validated before any kernel dereferences them (one stream synchronisation)
    S3D_HIP_TRY("mesh_winding", hipMemsetAsync(flags, 0, 16, st));
    const int cb = (int)std::min<long>(ME_BBOX_BLOCKS, me_blocks(3 * n_faces));
    hipLaunchKernelGGL(wn_check_faces_kernel, dim3(cb), dim3(ME_BLOCK), 0, st, faces, n_faces, n_vertices, flags);
    S3D_LAUNCH_CHECK();
    int bad = 0;
    S3D_HIP_TRY("mesh_winding", hipMemcpyAsync(&bad, flags, 4, hipMemcpyDeviceToHost, st));
    S3D_HIP_TRY("mesh_winding", hipStreamSynchronize(st));
    S3D_CHECK_ARG(!bad, "mesh_winding: a face indexes a vertex outside [0, %ld)", n_vertices);

    const long chunk = wn_chunk_faces(n_faces);
    const int n_chunks = (int)((n_faces + chunk - 1) / chunk);
    for (long i0 = 0; i0 < n_points; i0 += WN_BATCH) {
        const long nb = std::min(WN_BATCH, n_points - i0);
        const long blocks_p = (nb + WN_P_PER_BLOCK - 1) / WN_P_PER_BLOCK;
        // split over the faces when the points alone leave most of 256 CUs x 8 blocks idle
        int splits = n_splits ? n_splits : (int)std::min<long>(n_chunks, (2048 + blocks_p - 1) / blocks_p);
        splits = std::max(1, std::min(splits, n_chunks));
        const int cpb = (n_chunks + splits - 1) / splits;
        const dim3 grid((unsigned)blocks_p, (unsigned)((n_chunks + cpb - 1) / cpb));
        if (is_f64)
            hipLaunchKernelGGL(wn_kernel<double>, grid, dim3(ME_BLOCK), 0, st, (const double*)points + 3 * i0, nb, vertices,
                               faces, n_faces, chunk, n_chunks, cpb, part);
        else
            hipLaunchKernelGGL(wn_kernel<float>, grid, dim3(ME_BLOCK), 0, st, (const float*)points + 3 * i0, nb, vertices,
                               faces, n_faces, chunk, n_chunks, cpb, part);
        ME_LAUNCH(wn_sum_kernel, nb, st, part, nb, n_chunks, w + i0);
    }
    S3D_LAUNCH_CHECK();
    return 0;
}

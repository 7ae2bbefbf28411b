// mesh_render.hip — the input view and the 12 slab images of a triangle mesh for one camera: what the reference's Blender
// scripts (render_slices/blender_script_input.py, blender_script_slices.py) put into 00_img_input and 01_img_slices.
//
//   build:   vertices -> camera space p = c + (0, 0, distance), c = (v * scale + t) R, and slab coordinates M [c, 1];
//            slab bounds over the vertices the faces reference; per face the gathered triangle and a conservative range
//            of pixel tiles; entries per tile by integer atomics, offsets by the shared scan
//   fill:    the tile lists (integer cursors; the order inside a tile does not reach the result)
//   render:  one workgroup per tile, one thread per sample.  The tile's faces pass through LDS in chunks: each thread
//            prepares one face (b x c, c x a, a x b, n, a.n), then every lane reads the same LDS address.  A thread keeps
//            13 (depth, face) pairs in registers: the view and, per axis, the four slabs.  A hit updates four of them.
//            No atomics and no reductions across threads touch the result.
//   resolve: one thread per pixel and image: coverage -> alpha, Lambert shade of the covered samples -> rgb.
//
// Determinism.  The file is compiled with -ffp-contract=off: every product and sum is rounded on its own, so the three edge
// functions of a face are the exact negatives of its neighbour's across the shared edge (d.(b x a) = -d.(a x b)) and a
// sample on the edge hits one of the two.  A sample's result is the lexicographic minimum of (depth, face index) over the
// faces that hit it, and the tile ranges are supersets of the faces that can hit, so the tile edge and the order of the
// lists do not reach a bit of the output.
#include <math.h>
#include <string.h>

#include <algorithm>

#include "mesh_common.h"

#define MR_SIZE_MAX 1024
#define MR_CHUNK 128                        // faces per LDS chunk (13 float64 + index each: 13.8 KB)
#define MR_FACE_DOUBLES 13
#define MR_THREADS_MAX 1024                 // (tile * samples)^2
#define MR_IMAGES 13
#define MR_FOCAL 1.09375                    // 35 / 32

// prm (float64): R[9] | distance | scale | t[3] | M[12] | slab bounds lo + step * i, i = 1..3, per axis [9]
#define MR_R 0
#define MR_DIST 9
#define MR_SCALE 10
#define MR_T 11
#define MR_M 14
#define MR_BND 26
#define MR_PRM 36
#define MR_CAM 26                           // doubles the caller passes: R .. M

struct RenderCam {
    double v[MR_CAM];
};

struct RenderWs {
    double* part;          // [ME_BBOX_BLOCKS][6] partial bounds of the slab coordinates
    double* prm;           // [MR_PRM]
    int* flags;            // [0]: a face index outside [0, n_vertices)
    double* pv;            // [n_vertices][3] camera space
    double* sv;            // [n_vertices][3] slab coordinates
    double* tri;           // [n_faces][9] gathered camera-space triangles
    int* rng;              // [n_faces][4] tile range x0, x1, y0, y1 (x0 > x1: no tile)
    unsigned* cnt;         // [tiles] entries per tile, then the fill cursors
    long long* off;        // [tiles + 1]
    long long* tsum;       // [scan tiles + 1]
    long tiles;
    int tn;                // tiles per image side
};
// the arrays in the workspace's order; base == nullptr: only the size
static size_t render_layout(long nv, long nf, int size, int tile, RenderWs& w, char* base) {
    MeArena a{base};
    w.tn = (size + tile - 1) / tile;
    w.tiles = (long)w.tn * w.tn;
    const long scan_tiles = (w.tiles + ME_TILE - 1) / ME_TILE;
    w.part = a.take<double>(ME_BBOX_BLOCKS * 6), w.prm = a.take<double>(MR_PRM), w.flags = a.take<int>(4);
    w.pv = a.take<double>(3 * (size_t)nv), w.sv = a.take<double>(3 * (size_t)nv), w.tri = a.take<double>(9 * (size_t)nf);
    w.rng = a.take<int>(4 * (size_t)nf), w.cnt = a.take<unsigned>(w.tiles), w.off = a.take<long long>(w.tiles + 1);
    w.tsum = a.take<long long>(scan_tiles + 1);
    return a.off;
}

// p = (v * scale + t) R + (0, 0, distance); slab coordinates M [c, 1].  Products and sums in index order.
__global__ __launch_bounds__(ME_BLOCK) void mr_vertex_kernel(const double* __restrict__ verts, long nv, RenderCam cam,
                                                            double* __restrict__ prm, double* __restrict__ pv,
                                                            double* __restrict__ sv) {
    const long i = (long)blockIdx.x * ME_BLOCK + threadIdx.x;
    if (i < MR_CAM) prm[i] = cam.v[i];
    if (i >= nv) return;
    const double* R = cam.v + MR_R;
    const double* M = cam.v + MR_M;
    double w[3], c[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) w[a] = verts[3 * i + a] * cam.v[MR_SCALE] + cam.v[MR_T + a];
#pragma unroll
    for (int j = 0; j < 3; ++j) c[j] = w[0] * R[j] + w[1] * R[3 + j] + w[2] * R[6 + j];
    pv[3 * i] = c[0];
    pv[3 * i + 1] = c[1];
    pv[3 * i + 2] = c[2] + cam.v[MR_DIST];
#pragma unroll
    for (int a = 0; a < 3; ++a) sv[3 * i + a] = M[4 * a] * c[0] + M[4 * a + 1] * c[1] + M[4 * a + 2] * c[2] + M[4 * a + 3];
}

// slab bounds: lo + step * i, step = (hi - lo) / 4; an axis without extent has one slab (bounds +inf)
__global__ void mr_bounds_kernel(const double* __restrict__ part, int nb, double* __restrict__ prm) {
    if (threadIdx.x != 0) return;
    double lo[3], hi[3];
    me_bbox_fold(part, nb, lo, hi);
    for (int a = 0; a < 3; ++a) {
        const double step = (hi[a] - lo[a]) / 4.0;
        for (int i = 1; i <= 3; ++i) prm[MR_BND + 3 * a + i - 1] = step == 0.0 ? INFINITY : lo[a] + step * (double)i;
    }
}

// Tile range of a face.  A face in front of the camera (every p_z > 0) projects into the convex hull of its projected
// vertices, and a sample can hit it only there: the range is the vertices' pixel box widened by 2^-20 pixel + 2^-30 of
// its own magnitude (the projection's rounding is 2^-52 relative).  A face with a vertex at p_z <= 0 goes to every tile.
__device__ __forceinline__ void mr_tile_range(const double* t, int size, int tile, int tn, int* r) {
    if (!(t[2] > 0.0 && t[5] > 0.0 && t[8] > 0.0)) {                 // behind or across the camera plane, or NaN
        r[0] = 0, r[1] = tn - 1, r[2] = 0, r[3] = tn - 1;
        return;
    }
    double lo[2], hi[2];
#pragma unroll
    for (int a = 0; a < 2; ++a) {
        const double u0 = (MR_FOCAL * t[a] / t[2] + 0.5) * size, u1 = (MR_FOCAL * t[3 + a] / t[5] + 0.5) * size;
        const double u2 = (MR_FOCAL * t[6 + a] / t[8] + 0.5) * size;
        lo[a] = fmin(fmin(u0, u1), u2);
        hi[a] = fmax(fmax(u0, u1), u2);
        const double m = 0x1p-20 + 0x1p-30 * fmax(fabs(lo[a]), fabs(hi[a]));
        lo[a] -= m;
        hi[a] += m;
    }
    if (!(lo[0] < (double)size && hi[0] >= 0.0 && lo[1] < (double)size && hi[1] >= 0.0)) {
        const bool nan = lo[0] != lo[0] || hi[0] != hi[0] || lo[1] != lo[1] || hi[1] != hi[1];
        r[0] = 0, r[1] = nan ? tn - 1 : -1, r[2] = 0, r[3] = nan ? tn - 1 : -1;
        return;
    }
#pragma unroll
    for (int a = 0; a < 2; ++a) {
        const double l = fmin(fmax(lo[a], 0.0), (double)(size - 1)), h = fmin(fmax(hi[a], 0.0), (double)(size - 1));
        r[2 * a] = min(max((int)l / tile, 0), tn - 1);
        r[2 * a + 1] = min(max((int)h / tile, 0), tn - 1);
    }
}

__global__ __launch_bounds__(ME_BLOCK) void mr_face_kernel(const double* __restrict__ pv, long nv,
                                                          const long long* __restrict__ faces, long nf,
                                                          double* __restrict__ tri, int* __restrict__ rng,
                                                          unsigned* __restrict__ cnt, int size, int tile, int tn) {
    const long f = (long)blockIdx.x * ME_BLOCK + threadIdx.x;
    if (f >= nf) return;
    double t[9];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const long long vi = faces[3 * f + k];
        if (vi < 0 || vi >= nv) {                       // reported by the bounds pass; the face reaches no tile
            rng[4 * f] = 0, rng[4 * f + 1] = -1, rng[4 * f + 2] = 0, rng[4 * f + 3] = -1;
            return;
        }
#pragma unroll
        for (int a = 0; a < 3; ++a) t[3 * k + a] = pv[3 * vi + a];
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) tri[9 * f + k] = t[k];
    int r[4];
    mr_tile_range(t, size, tile, tn, r);
#pragma unroll
    for (int k = 0; k < 4; ++k) rng[4 * f + k] = r[k];
    for (int y = r[2]; y <= r[3]; ++y)
        for (int x = r[0]; x <= r[1]; ++x) atomicAdd(&cnt[(long)y * tn + x], 1u);
}

__global__ __launch_bounds__(ME_BLOCK) void mr_fill_kernel(const int* __restrict__ rng, long nf,
                                                          const long long* __restrict__ off, unsigned* __restrict__ cur,
                                                          int* __restrict__ entries, long long n_entries, int tn) {
    const long f = (long)blockIdx.x * ME_BLOCK + threadIdx.x;
    if (f >= nf) return;
    const int x0 = max(rng[4 * f], 0), x1 = min(rng[4 * f + 1], tn - 1);
    const int y0 = max(rng[4 * f + 2], 0), y1 = min(rng[4 * f + 3], tn - 1);
    for (int y = y0; y <= y1; ++y)
        for (int x = x0; x <= x1; ++x) {
            const long c = (long)y * tn + x;
            const long long slot = off[c] + atomicAdd(&cur[c], 1u);
            if (slot < off[c + 1] && slot < n_entries) entries[slot] = (int)f;
        }
}

// the ray of global sample g (0 .. size * S - 1) on one image axis: ((u - 0.5) / f), u = (i + (a + 0.5) / S) / size
__device__ __forceinline__ double mr_ray(int g, int S, int size) {
    const int i = g / S, a = g - i * S;
    const double u = ((double)i + ((double)a + 0.5) / (double)S) / (double)size;
    return (u - 0.5) / MR_FOCAL;
}

__device__ __forceinline__ void mr_take(double s, int f, double& bd, int& bf) {
    if (s < bd || (s == bd && f < bf)) {
        bd = s;
        bf = f;
    }
}

__global__ __launch_bounds__(MR_THREADS_MAX) void mr_render_kernel(
    const double* __restrict__ tri, long nf, const double* __restrict__ prm, const long long* __restrict__ off,
    const int* __restrict__ entries, long long n_entries, int size, int S, int tile, int tn, double* __restrict__ depth,
    int* __restrict__ face, unsigned long long* __restrict__ n_tests) {
    __shared__ double sh[MR_CHUNK * MR_FACE_DOUBLES];
    __shared__ int sh_f[MR_CHUNK];
    const int edge = tile * S, nthreads = edge * edge, tid = (int)threadIdx.x;
    const int ty = (int)blockIdx.x / tn, tx = (int)blockIdx.x - ty * tn;
    const int ly = tid / edge, lx = tid - ly * edge;
    const int W = size * S;
    const int gx = tx * edge + lx, gy = ty * edge + ly;
    const bool live = gx < W && gy < W;
    const double dx = mr_ray(live ? gx : 0, S, size), dy = mr_ray(live ? gy : 0, S, size);
    const double dist = prm[MR_DIST];
    double M[12], bnd[9];
#pragma unroll
    for (int k = 0; k < 12; ++k) M[k] = prm[MR_M + k];
#pragma unroll
    for (int k = 0; k < 9; ++k) bnd[k] = prm[MR_BND + k];
    double bd[MR_IMAGES];
    int bf[MR_IMAGES];
#pragma unroll
    for (int k = 0; k < MR_IMAGES; ++k) {
        bd[k] = INFINITY;
        bf[k] = -1;
    }
    const long long e0 = max(off[blockIdx.x], 0ll), e1 = min(off[blockIdx.x + 1], n_entries);
    for (long long c0 = e0; c0 < e1; c0 += MR_CHUNK) {
        const int m = (int)min((long long)MR_CHUNK, e1 - c0);
        __syncthreads();
        for (int j = tid; j < m; j += nthreads) {
            int f = entries[c0 + j];
            double* q = sh + j * MR_FACE_DOUBLES;
            if (f < 0 || f >= nf) {                       // not reachable from a build + fill; never read past tri
                f = -1;
#pragma unroll
                for (int k = 0; k < MR_FACE_DOUBLES; ++k) q[k] = 0.0;
            } else {
                const double* t = tri + 9L * f;
                const double ax = t[0], ay = t[1], az = t[2], bx = t[3], by = t[4], bz = t[5], cx = t[6], cy = t[7], cz = t[8];
                q[0] = by * cz - bz * cy, q[1] = bz * cx - bx * cz, q[2] = bx * cy - by * cx;       // b x c
                q[3] = cy * az - cz * ay, q[4] = cz * ax - cx * az, q[5] = cx * ay - cy * ax;       // c x a
                q[6] = ay * bz - az * by, q[7] = az * bx - ax * bz, q[8] = ax * by - ay * bx;       // a x b
                const double ux = bx - ax, uy = by - ay, uz = bz - az, vx = cx - ax, vy = cy - ay, vz = cz - az;
                const double nx = uy * vz - uz * vy, ny = uz * vx - ux * vz, nz = ux * vy - uy * vx;
                q[9] = nx, q[10] = ny, q[11] = nz;
                q[12] = ax * nx + ay * ny + az * nz;
            }
            sh_f[j] = f;
        }
        __syncthreads();
        if (live) {
            for (int j = 0; j < m; ++j) {
                const double* q = sh + j * MR_FACE_DOUBLES;
                const double f0 = dx * q[0] + dy * q[1] + q[2];
                const double f1 = dx * q[3] + dy * q[4] + q[5];
                const double f2 = dx * q[6] + dy * q[7] + q[8];
                const bool pos = f0 >= 0.0 && f1 >= 0.0 && f2 >= 0.0, neg = f0 <= 0.0 && f1 <= 0.0 && f2 <= 0.0;
                if (!(pos || neg) || (pos && neg)) continue;          // mixed signs, NaN, or all three zero
                const double nx = q[9], ny = q[10], nz = q[11];
                const int f = sh_f[j];
                if ((nx == 0.0 && ny == 0.0 && nz == 0.0) || f < 0) continue;
                const double s = q[12] / (dx * nx + dy * ny + nz);
                if (!(s > 0.0)) continue;
                mr_take(s, f, bd[0], bf[0]);
                const double px = s * dx, py = s * dy, pz = s - dist;
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    const double co = M[4 * a] * px + M[4 * a + 1] * py + M[4 * a + 2] * pz + M[4 * a + 3];
                    const int k = (co >= bnd[3 * a] ? 1 : 0) + (co >= bnd[3 * a + 1] ? 1 : 0) + (co >= bnd[3 * a + 2] ? 1 : 0);
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        if (k == i) mr_take(s, f, bd[1 + 4 * a + i], bf[1 + 4 * a + i]);
                }
            }
        }
    }
    if (live) {
        const long plane = (long)W * W, at = (long)gy * W + gx;
#pragma unroll
        for (int k = 0; k < MR_IMAGES; ++k) {
            face[k * plane + at] = bf[k];
            if (depth) depth[k * plane + at] = bd[k];
        }
    }
    if (n_tests && tid == 0 && e1 > e0) {                // face tests of this tile: its live samples x its entries
        const long long lw = min(edge, W - tx * edge), lh = min(edge, W - ty * edge);
        atomicAdd(n_tests, (unsigned long long)(lw * lh * (e1 - e0)));
    }
}

// One thread per pixel and image: alpha = round(255 count / S^2); rgb = round(255 mean over the covered samples of
// albedo * (0.5 + 0.5 |n.d| / (|n| |d|))), the samples summed row by row.  The albedo is 0.8, or on image 0 the mean of the
// face's three vertex colours.  rint rounds halves to even, as numpy does.
__global__ __launch_bounds__(ME_BLOCK) void mr_resolve_kernel(const double* __restrict__ tri, long nf,
                                                             const int* __restrict__ face, const long long* __restrict__ faces,
                                                             const double* __restrict__ colors, int size, int S,
                                                             unsigned char* __restrict__ rgba) {
    const long i = (long)blockIdx.x * ME_BLOCK + threadIdx.x, px_n = (long)size * size;
    if (i >= MR_IMAGES * px_n) return;
    const int img = (int)(i / px_n), y = (int)((i % px_n) / size), x = (int)(i % size);
    const int W = size * S;
    const int* fp = face + (long)img * W * W;
    double sum[3] = {0.0, 0.0, 0.0};
    int count = 0;
    for (int b = 0; b < S; ++b)
        for (int a = 0; a < S; ++a) {
            const int gx = x * S + a, gy = y * S + b;
            const int f = fp[(long)gy * W + gx];
            if (f < 0 || f >= nf) continue;
            const double dx = mr_ray(gx, S, size), dy = mr_ray(gy, S, size);
            const double* t = tri + 9L * f;
            const double ux = t[3] - t[0], uy = t[4] - t[1], uz = t[5] - t[2];
            const double vx = t[6] - t[0], vy = t[7] - t[1], vz = t[8] - t[2];
            const double nx = uy * vz - uz * vy, ny = uz * vx - ux * vz, nz = ux * vy - uy * vx;
            const double nd = fabs(dx * nx + dy * ny + nz);
            const double shade = 0.5 + 0.5 * (nd / (sqrt(nx * nx + ny * ny + nz * nz) * sqrt(dx * dx + dy * dy + 1.0)));
            ++count;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                double alb = 0.8;
                if (img == 0 && colors)
                    alb = (colors[3 * faces[3L * f] + c] + colors[3 * faces[3L * f + 1] + c] + colors[3 * faces[3L * f + 2] + c]) / 3.0;
                sum[c] += alb * shade;
            }
        }
    unsigned char* o = rgba + 4 * i;
    if (count == 0) {
        o[0] = o[1] = o[2] = o[3] = 0;
        return;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c] = (unsigned char)fmin(fmax(rint(255.0 * (sum[c] / (double)count)), 0.0), 255.0);
    o[3] = (unsigned char)rint(255.0 * (double)count / (double)(S * S));
}

static bool render_shape_ok(long nv, long nf, int size, int S, int tile) {
    return nv >= 1 && nf >= 1 && nf < (1L << 31) && size >= 1 && size <= MR_SIZE_MAX && (S == 1 || S == 2 || S == 4) &&
           tile >= 1 && (long)tile * S <= 32;
}
static int render_check(long nv, long nf, int size, int S, int tile, const void* ws, size_t ws_bytes, RenderWs& w,
                        const char* what) {
    S3D_CHECK_ARG(nv >= 1 && nf >= 1 && nf < (1L << 31), "%s: %ld vertices, %ld faces (1 .. 2^31 - 1 faces)", what, nv, nf);
    S3D_CHECK_ARG(size >= 1 && size <= MR_SIZE_MAX, "%s: image size %d outside [1, %d]", what, size, MR_SIZE_MAX);
    S3D_CHECK_ARG(S == 1 || S == 2 || S == 4, "%s: %d samples per pixel edge (1, 2 or 4)", what, S);
    S3D_CHECK_ARG(tile >= 1 && (long)tile * S <= 32, "%s: tile edge %d (1 .. %d pixels at %d samples per pixel edge)", what,
                  tile, 32 / S, S);
    S3D_CHECK_ARG(ws != nullptr, "%s: null workspace", what);
    const size_t need = render_layout(nv, nf, size, tile, w, nullptr);
    if (ws_bytes < need) {
        s3d_set_error("%s: workspace %zu < %zu bytes", what, ws_bytes, need);
        return S3D_E_WORKSPACE;
    }
    render_layout(nv, nf, size, tile, w, (char*)ws);
    return 0;
}

extern "C" size_t s3d_mesh_render_workspace_bytes(long n_vertices, long n_faces, int size, int samples, int tile) {
    if (!render_shape_ok(n_vertices, n_faces, size, samples, tile)) return 0;
    RenderWs w;
    return render_layout(n_vertices, n_faces, size, tile, w, nullptr);
}

extern "C" int s3d_mesh_render_build(const double* vertices, long n_vertices, const long long* faces, long n_faces,
                                     const double* camera, int size, int samples, int tile, void* workspace,
                                     size_t workspace_bytes, long* n_entries, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    RenderWs w;
    S3D_CHECK_ARG(n_entries != nullptr, "mesh_render_build: null n_entries");
    S3D_CHECK_ARG(vertices && faces && camera, "mesh_render_build: null mesh or camera");
    TRY_RET(render_check(n_vertices, n_faces, size, samples, tile, workspace, workspace_bytes, w, "mesh_render_build"));
    *n_entries = 0;
    RenderCam cam;
    memcpy(cam.v, camera, sizeof(cam.v));
    for (int k = 0; k < MR_CAM; ++k) S3D_CHECK_ARG(std::isfinite(cam.v[k]), "mesh_render_build: camera value %d is not finite", k);
    S3D_HIP_TRY("mesh_render_build", hipMemsetAsync(w.flags, 0, 16, st));
    S3D_HIP_TRY("mesh_render_build", hipMemsetAsync(w.cnt, 0, (size_t)w.tiles * 4, st));
    // the first MR_CAM threads also copy the camera into prm
    ME_LAUNCH(mr_vertex_kernel, std::max<long>(n_vertices, MR_CAM), st, vertices, n_vertices, cam, w.prm, w.pv, w.sv);
    const int nb = (int)std::min<long>(ME_BBOX_BLOCKS, me_blocks(3 * n_faces));
    hipLaunchKernelGGL(me_bbox_partial_kernel, dim3(nb), dim3(ME_BLOCK), 0, st, w.sv, n_vertices, faces, n_faces, w.part,
                       w.flags);
    hipLaunchKernelGGL(mr_bounds_kernel, dim3(1), dim3(64), 0, st, w.part, nb, w.prm);
    ME_LAUNCH(mr_face_kernel, n_faces, st, w.pv, n_vertices, faces, n_faces, w.tri, w.rng, w.cnt, size, tile, w.tn);
    return me_lists_finish("mesh_render_build", w.cnt, w.off, w.tiles, w.tsum, w.flags, n_vertices, n_entries, st);
}

extern "C" int s3d_mesh_render_fill(long n_vertices, long n_faces, int size, int samples, int tile, void* workspace,
                                    size_t workspace_bytes, int* entries, long n_entries, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    RenderWs w;
    S3D_CHECK_ARG(n_entries >= 0 && (n_entries == 0 || entries), "mesh_render_fill: bad argument");
    TRY_RET(render_check(n_vertices, n_faces, size, samples, tile, workspace, workspace_bytes, w, "mesh_render_fill"));
    if (n_entries == 0) return 0;
    S3D_HIP_TRY("mesh_render_fill", hipMemsetAsync(w.cnt, 0, (size_t)w.tiles * 4, st));
    ME_LAUNCH(mr_fill_kernel, n_faces, st, w.rng, n_faces, w.off, w.cnt, entries, (long long)n_entries, w.tn);
    S3D_LAUNCH_CHECK();
    return 0;
}

extern "C" int s3d_mesh_render_render(long n_vertices, const long long* faces, long n_faces, int size, int samples, int tile,
                                      const void* workspace, size_t workspace_bytes, const int* entries, long n_entries,
                                      const double* vertex_colors, double* depth, int* face, unsigned char* rgba,
                                      unsigned long long* n_tests, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    RenderWs w;
    S3D_CHECK_ARG(face != nullptr, "mesh_render_render: null face output");
    S3D_CHECK_ARG(n_entries >= 0 && (n_entries == 0 || entries), "mesh_render_render: bad entries");
    S3D_CHECK_ARG(!vertex_colors || faces, "mesh_render_render: vertex colours need the faces");
    TRY_RET(render_check(n_vertices, n_faces, size, samples, tile, workspace, workspace_bytes, w, "mesh_render_render"));
    if (n_tests) S3D_HIP_TRY("mesh_render_render", hipMemsetAsync(n_tests, 0, 8, st));
    const int edge = tile * samples;
    hipLaunchKernelGGL(mr_render_kernel, dim3((unsigned)w.tiles), dim3(edge * edge), 0, st, w.tri, n_faces, w.prm, w.off,
                       entries, (long long)n_entries, size, samples, tile, w.tn, depth, face, n_tests);
    const long px = (long)MR_IMAGES * size * size;
    if (rgba) ME_LAUNCH(mr_resolve_kernel, px, st, w.tri, n_faces, face, faces, vertex_colors, size, samples, rgba);
    S3D_LAUNCH_CHECK();
    return 0;
}

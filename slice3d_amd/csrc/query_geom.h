// query_geom.h — a query's image geometry, defined once: from (x, y, z) to the four bilinear taps of a pyramid level, and the
// locality sort's bins and tiles.  The token builders, the sort, the stand-alone samplers and the three sampling-backward
// kernels all go through these functions: the backward scatters with the weights the forward gathered with, and a sorted
// slot's taps lie in the footprint of the tile its bin belongs to, because both sides evaluate the same expressions.
//
// Floating-point contraction: the rotation and project() keep their translation unit's default; the cell is contract(off).
#pragma once
#include <hip/hip_runtime.h>

// ---------------------------------------------------------------------------------------------
// query coordinates
// ---------------------------------------------------------------------------------------------
// torch.linspace(start,end,steps)[i] as ATen computes it (symmetric halves)
__device__ __forceinline__ float linspace_at(float start, float end, int steps, int i) {
    const float step = (end - start) / (float)(steps - 1);
    return i < steps / 2 ? start + step * (float)i : end - step * (float)(steps - i - 1);
}

// flip (mode='test', models.py:53-56) or rotate (qry @ obj_rot_mat, models.py:58-60) a query of batch item b
__device__ __forceinline__ void rotate_query(const float* rot, int flip_yz, int b, float& x, float& y, float& z) {
    if (flip_yz) {
        y = -y; z = -z;
    } else if (rot) {
        const float* R = rot + b * 9;
        const float rx = x * R[0] + y * R[3] + z * R[6];
        const float ry = x * R[1] + y * R[4] + z * R[7];
        const float rz = x * R[2] + y * R[5] + z * R[8];
        x = rx; y = ry; z = rz;
    }
}
// Query q of batch item b, as the decoder sees it: read through perm (optional) from qry (B, Q, 3) or, with qry == NULL, from
// the dense grid of nx^3 points in a box (x slowest, z fastest, common.py:145-164; q_offset = first point of the slab), then
// flipped or rotated.
__device__ __forceinline__ void query_xyz(const float* qry, const float* rot, int flip_yz, const int* perm, int nx, float box,
                                          long q_offset, int b, long q, long n_qry, float& x, float& y, float& z) {
    if (perm) q = perm[(long)b * n_qry + q];
    if (qry) {
        const float* p = qry + ((long)b * n_qry + q) * 3;
        x = p[0]; y = p[1]; z = p[2];
    } else {
        const long nn = (long)nx * nx, ql = q + q_offset;
        const int ixg = (int)(ql / nn), iyg = (int)((ql / nx) % nx), izg = (int)(ql % nx);
        x = box * linspace_at(-0.5f, 0.5f, nx, ixg);
        y = box * linspace_at(-0.5f, 0.5f, nx, iyg);
        z = box * linspace_at(-0.5f, 0.5f, nx, izg);
    }
    rotate_query(rot, flip_yz, b, x, y, z);
}
// the same for callers whose queries are always explicit points
__device__ __forceinline__ void query_xyz(const float* qry, const float* rot, int flip_yz, const int* perm, int b, long q,
                                          long n_qry, float& x, float& y, float& z) {
    __builtin_assume(qry != nullptr);
    query_xyz(qry, rot, flip_yz, perm, 0, 0.f, 0, b, q, n_qry, x, y, z);
}

// project_coord (models.py:28-36): [x y z 1] @ T(4x3); uv = XY / Z; 2(uv - .5); clamp [-1,1]
__device__ __forceinline__ void project(const float* T, float x, float y, float z, float& gx, float& gy) {
    const float X = x * T[0] + y * T[3] + z * T[6] + T[9];
    const float Y = x * T[1] + y * T[4] + z * T[7] + T[10];
    const float Z = x * T[2] + y * T[5] + z * T[8] + T[11];
    gx = fminf(fmaxf(2.f * (X / Z - 0.5f), -1.f), 1.f);
    gy = fminf(fmaxf(2.f * (Y / Z - 0.5f), -1.f), 1.f);
}

// ---------------------------------------------------------------------------------------------
// the cell of a point in a level (grid_sample, bilinear, align_corners=True) and its adaptors
// ---------------------------------------------------------------------------------------------
// level_cell() is the one place that un-normalises and floors; the four factor differences are Cell's members.  All of it is
// contract(off): the factors must not depend on which products hipcc decides to fuse in a given caller (round 6: two
// instantiations of the token builder — and now the backward — must produce the same bits).
struct Cell {
    int x0, y0;                        // floor cell
    float ix, iy, x0f, y0f, xe, ye;    // pixel coordinates, their floors, floors + 1
    // UNMASKED column / row factors of the tap weights.  Off [-1, 1] they can be negative, huge or non-finite: every adaptor
    // masks, either the factors (make_foot) or their product (make_taps), and must keep doing it where it does
    __device__ __forceinline__ float wx0() const {
#pragma clang fp contract(off)
        return xe - ix;
    }
    __device__ __forceinline__ float wx1() const {
#pragma clang fp contract(off)
        return ix - x0f;
    }
    __device__ __forceinline__ float wy0() const {
#pragma clang fp contract(off)
        return ye - iy;
    }
    __device__ __forceinline__ float wy1() const {
#pragma clang fp contract(off)
        return iy - y0f;
    }
};
__device__ __forceinline__ Cell level_cell(float gx, float gy, int W, int H) {
#pragma clang fp contract(off)
    // ATen grid_sampler_unnormalize (align_corners): ((coord + 1) / 2) * (size - 1)
    const float ix = ((gx + 1.f) / 2.f) * (float)(W - 1);
    const float iy = ((gy + 1.f) / 2.f) * (float)(H - 1);
    const float x0f = floorf(ix), y0f = floorf(iy);
    const int x0 = (int)x0f, y0 = (int)y0f;
    const float xe = x0f + 1.f, ye = y0f + 1.f;
    return Cell{x0, y0, ix, iy, x0f, y0f, xe, ye};
}

struct Tap4 {          // bilinear footprint of one query in one level
    int off[4];        // element offset of the tap pixel (before * C), clamped in-bounds
    float w[4];        // tap weight, 0 for out-of-bounds taps (padding_mode='zeros'): the PRODUCT is masked
};
__device__ __forceinline__ Tap4 make_taps(float gx, float gy, int W, int H) {
#pragma clang fp contract(off)   // (see Cell)
    const Cell c = level_cell(gx, gy, W, H);
    const int x0 = c.x0, y0 = c.y0, x1 = x0 + 1, y1 = y0 + 1;
    Tap4 t;
    const float wnw = c.wx0() * c.wy0(), wne = c.wx1() * c.wy0();
    const float wsw = c.wx0() * c.wy1(), wse = c.wx1() * c.wy1();
    const bool vx0 = x0 >= 0 && x0 < W, vx1 = x1 >= 0 && x1 < W;
    const bool vy0 = y0 >= 0 && y0 < H, vy1 = y1 >= 0 && y1 < H;
    const int cx0 = min(max(x0, 0), W - 1), cx1 = min(max(x1, 0), W - 1);
    const int cy0 = min(max(y0, 0), H - 1), cy1 = min(max(y1, 0), H - 1);
    t.off[0] = cy0 * W + cx0; t.w[0] = (vx0 && vy0) ? wnw : 0.f;
    t.off[1] = cy0 * W + cx1; t.w[1] = (vx1 && vy0) ? wne : 0.f;
    t.off[2] = cy1 * W + cx0; t.w[2] = (vx0 && vy1) ? wsw : 0.f;
    t.off[3] = cy1 * W + cx1; t.w[3] = (vx1 && vy1) ? wse : 0.f;
    return t;
}

struct Foot {            // the same footprint, factorised
    int x0, y0;          // floor cell; >= 0 when the grid is clamped to [-1, 1]
    float wx0, wx1, wy0, wy1;  // column / row factors of the tap weights (make_taps: w = wx * wy), 0 for out-of-bounds columns / rows: the
                               // FACTORS are masked (scalars, not arrays: hipcc turns `g == dx ? wx[0] : g == dx + 1 ? wx[1] : 0` into an
                               // indexed scratch read)
};
__device__ __forceinline__ Foot make_foot(float gx, float gy, int W, int H) {
    const Cell c = level_cell(gx, gy, W, H);
    Foot f;
    f.x0 = c.x0; f.y0 = c.y0;
    const int x1 = f.x0 + 1, y1 = f.y0 + 1;
    f.wx0 = (f.x0 >= 0 && f.x0 < W) ? c.wx0() : 0.f;
    f.wx1 = (x1 >= 0 && x1 < W) ? c.wx1() : 0.f;
    f.wy0 = (f.y0 >= 0 && f.y0 < H) ? c.wy0() : 0.f;
    f.wy1 = (y1 >= 0 && y1 < H) ? c.wy1() : 0.f;
    return f;
}

// ---------------------------------------------------------------------------------------------
// bins and tiles of the locality sort: 256 x 256 bins of the projected coordinate in Morton order, 16 x 16 tiles of 16 x 16 bins
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned sort_bin(float g) {   // g in [-1, 1] -> 0 .. 255
    return (unsigned)fminf(fmaxf((g + 1.f) * 127.5f, 0.f), 255.f);
}
__host__ __device__ __forceinline__ unsigned spread8(unsigned v) {    // 8 bits -> the even bits of a 16-bit Morton code
    v = (v | (v << 4)) & 0x0F0Fu;
    v = (v | (v << 2)) & 0x3333u;
    v = (v | (v << 1)) & 0x5555u;
    return v;
}
__host__ __device__ __forceinline__ unsigned compact8(unsigned v) {   // and back
    v &= 0x5555u;
    v = (v | (v >> 1)) & 0x3333u;
    v = (v | (v >> 2)) & 0x0F0Fu;
    v = (v | (v >> 4)) & 0x00FFu;
    return v;
}
__host__ __device__ __forceinline__ unsigned morton8(unsigned x, unsigned y) { return spread8(x) | (spread8(y) << 1); }
// Tile t (0 .. 15 along one axis) holds the bins 16 t .. 16 t + 15, i.e. the coordinates from pixel 16 t (W - 1) / 255 of a level
// of width W on: its taps start at tile_origin and span at most tile_footprint pixels (the + 2: the floor and the second tap).
__host__ __device__ __forceinline__ int tile_origin(int t, int W) { return 16 * t * (W - 1) / 255; }
__host__ __device__ __forceinline__ int tile_footprint(int W) { return (16 * (W - 1) + 254) / 255 + 2; }

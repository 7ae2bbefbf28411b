// mesh_simplify.hip — quadric edge-collapse simplification of a triangle mesh on the device.
//
// The reference's simplifier (src_convonet/utils/libsimplify/Simplify.h, Fast-Quadric-Mesh-Simplification) walks the
// triangles in order and collapses every edge below the round's threshold as it meets it.  Here a round collapses an
// independent set of edges at once: every legal candidate edge writes a 64-bit key (cost bits | edge id) by integer
// atomicMin into each vertex of the closed neighbourhood of its two endpoints and wins if it still holds the minimum
// at both endpoints, so the winners touch disjoint faces and vertices and the result is independent of scheduling.  Quadrics,
// costs and positions are float64 as in the reference; no float atomic is used anywhere and every float64 sum runs
// over a list in one fixed order, so the output is the same bits from run to run.
//
// Per pass (ms_pass): vertex -> face adjacency (count, me_scan, fill, per-vertex sort by face index), face normals,
// (first pass: vertex quadrics), border flags, per-edge cost / target / legality / key, winners, the cheapest winners
// that still fit the target, apply.  Per round (ms_round): a few passes at the round's threshold, then the compaction of
// the face list and the live count read back (the round's one synchronisation).
#include <algorithm>

#include "mesh_common.h"

#define MS_NOKEY 0xFFFFFFFFFFFFFFFFull
#define MS_MAX_ROUNDS 100            // Simplify.h:359
#define MS_FACES_MAX (1L << 29)      // 3 * n_faces (edge ids, adjacency entries) stays inside 31 bits

typedef unsigned long long ms_u64;

// flags: [0] bad face index, [1] winners in the list, [2] faces the winners would remove
struct SimpWs {
    int* flags;
    long long* hdr;      // [0] faces out, [1] vertices out
    ms_u64* ksel;        // the round's largest applied key
    double *P, *Q, *fn, *etgt;
    int *border, *vcnt, *voff, *vmap;
    ms_u64 *vkey, *ekey, *wkey;
    int *FA, *FB, *alive, *foff, *adj, *erem, *wrem, *tsum;
    long nv, nf;
};

// the arrays in the workspace's order; base == nullptr: only the size
static size_t simp_layout(long nv, long nf, SimpWs& w, char* base) {
    MeArena a{base};
    const size_t V = (size_t)nv, F = (size_t)nf;
    const long tiles = (std::max(nv + 1, nf) + ME_TILE - 1) / ME_TILE;
    w.flags = a.take<int>(16), w.hdr = a.take<long long>(2), w.ksel = a.take<ms_u64>(1);
    w.P = a.take<double>(3 * V), w.Q = a.take<double>(10 * V), w.fn = a.take<double>(3 * F), w.etgt = a.take<double>(9 * F);
    w.border = a.take<int>(V), w.vcnt = a.take<int>(V + 1), w.voff = a.take<int>(V + 1), w.vmap = a.take<int>(V + 1);
    w.vkey = a.take<ms_u64>(V), w.ekey = a.take<ms_u64>(3 * F), w.wkey = a.take<ms_u64>(F);
    w.FA = a.take<int>(3 * F), w.FB = a.take<int>(3 * F), w.alive = a.take<int>(F), w.foff = a.take<int>(F);
    w.adj = a.take<int>(3 * F), w.erem = a.take<int>(3 * F), w.wrem = a.take<int>(F), w.tsum = a.take<int>(tiles + 1);
    w.nv = nv, w.nf = nf;
    return a.off;
}

// =============================================================================================
// input
// =============================================================================================
static __global__ void ms_validate_kernel(const long long* __restrict__ faces, long n3, long nv, int* __restrict__ flags) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n3 && (faces[i] < 0 || faces[i] >= nv)) flags[0] = 1;
}
// int64 faces -> int32; with `drop` a face that names a vertex twice is dead from the start (it spans no area and no
// collapse could ever remove it)
static __global__ void ms_import_kernel(const long long* __restrict__ faces, long nf, int* __restrict__ F,
                                        int* __restrict__ alive, int drop) {
    const long f = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= nf) return;
    const int a = (int)faces[3 * f], b = (int)faces[3 * f + 1], c = (int)faces[3 * f + 2];
    F[3 * f] = a, F[3 * f + 1] = b, F[3 * f + 2] = c;
    alive[f] = !(drop && (a == b || b == c || a == c));
}

// =============================================================================================
// adjacency: vertex -> (face * 4 + corner), ascending
// =============================================================================================
static __global__ void ms_vcount_kernel(const int* __restrict__ F, long n3, const int* __restrict__ alive,
                                        int* __restrict__ vcnt) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n3 && alive[i / 3]) atomicAdd(&vcnt[F[i]], 1);
}
static __global__ void ms_vfill_kernel(const int* __restrict__ F, long n3, const int* __restrict__ alive,
                                       const int* __restrict__ voff, int* __restrict__ vcnt, int* __restrict__ adj) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n3 || !alive[i / 3]) return;
    const int v = F[i];
    const int slot = atomicAdd(&vcnt[v], 1);
    adj[voff[v] + slot] = (int)(i / 3) * 4 + (int)(i % 3);
}
// the fill's order depends on scheduling; the sorted list does not.  Valences are small (about 6), insertion sort.
static __global__ void ms_vsort_kernel(const int* __restrict__ voff, long nv, int* __restrict__ adj) {
    const long v = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= nv) return;
    const int lo = voff[v], hi = voff[v + 1];
    for (int i = lo + 1; i < hi; ++i) {
        const int x = adj[i];
        int j = i - 1;
        while (j >= lo && adj[j] > x) {
            adj[j + 1] = adj[j];
            --j;
        }
        adj[j + 1] = x;
    }
}

// =============================================================================================
// face normals, vertex quadrics, border flags
// =============================================================================================
// unit vector, or 0 with ok = false for a vector without a direction
static __device__ __forceinline__ me_v3 ms_unit(me_v3 a, bool& ok) {
    const double l = sqrt(me_dot(a, a));
    ok = l > 0.0 && isfinite(l);
    return ok ? me_v3{a.x / l, a.y / l, a.z / l} : me_v3{0.0, 0.0, 0.0};
}

// unit normal of every live face (0 for a face without area)
static __global__ void ms_normals_kernel(const int* __restrict__ F, long nf, const double* __restrict__ P,
                                         const int* __restrict__ alive, double* __restrict__ fn) {
    const long f = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= nf || !alive[f]) return;
    const me_v3 p0 = me_ld(P, F[3 * f]), p1 = me_ld(P, F[3 * f + 1]), p2 = me_ld(P, F[3 * f + 2]);
    bool ok;
    const me_v3 n = ms_unit(me_cross(me_sub(p1, p0), me_sub(p2, p0)), ok);
    fn[3 * f] = n.x, fn[3 * f + 1] = n.y, fn[3 * f + 2] = n.z;
}
// Simplify.h:637-650: the sum of the plane quadrics of a vertex's faces, in ascending face order
static __global__ void ms_quadrics_kernel(const int* __restrict__ F, const double* __restrict__ P, const double* __restrict__ fn,
                                          const int* __restrict__ voff, const int* __restrict__ adj, long nv,
                                          double* __restrict__ Q) {
    const long v = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= nv) return;
    double q[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int k = voff[v]; k < voff[v + 1]; ++k) {
        const long f = adj[k] >> 2;
        const double a = fn[3 * f], b = fn[3 * f + 1], c = fn[3 * f + 2];
        const double d = -me_dot(me_v3{a, b, c}, me_ld(P, F[3 * f]));
        q[0] += a * a, q[1] += a * b, q[2] += a * c, q[3] += a * d;
        q[4] += b * b, q[5] += b * c, q[6] += b * d;
        q[7] += c * c, q[8] += c * d;
        q[9] += d * d;
    }
    for (int i = 0; i < 10; ++i) Q[10 * v + i] = q[i];
}

static __device__ __forceinline__ bool ms_face_has(const int* __restrict__ F, long f, int v) {
    return F[3 * f] == v || F[3 * f + 1] == v || F[3 * f + 2] == v;
}
// Simplify.h:694-729: a vertex is a border vertex if one of its edges has exactly one face
static __global__ void ms_border_kernel(const int* __restrict__ F, long n3, const int* __restrict__ alive,
                                        const int* __restrict__ voff, const int* __restrict__ adj, int* __restrict__ border) {
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n3 || !alive[e / 3]) return;
    const long f = e / 3;
    const int j = (int)(e % 3);
    const int a = F[3 * f + j], b = F[3 * f + (j + 1) % 3];
    int c = 0;
    for (int k = voff[a]; k < voff[a + 1]; ++k) c += ms_face_has(F, adj[k] >> 2, b);
    if (c == 1) border[a] = 1, border[b] = 1;
}

// =============================================================================================
// edges: cost, target, legality, key
// =============================================================================================
static __device__ __forceinline__ double ms_det3(const double* q, int a11, int a12, int a13, int a21, int a22, int a23, int a31,
                                                 int a32, int a33) {
    return q[a11] * q[a22] * q[a33] + q[a13] * q[a21] * q[a32] + q[a12] * q[a23] * q[a31] - q[a13] * q[a22] * q[a31] -
           q[a11] * q[a23] * q[a32] - q[a12] * q[a21] * q[a33];
}
static __device__ __forceinline__ double ms_vertex_error(const double* q, me_v3 p) {
    return q[0] * p.x * p.x + 2 * q[1] * p.x * p.y + 2 * q[2] * p.x * p.z + 2 * q[3] * p.x + q[4] * p.y * p.y +
           2 * q[5] * p.y * p.z + 2 * q[6] * p.y + q[7] * p.z * p.z + 2 * q[8] * p.z + q[9];
}
// calculate_error (Simplify.h:777-810); a minimiser that is not finite falls through to the three-point choice
static __device__ double ms_edge_error(const double* __restrict__ Q, const double* __restrict__ P, int a, int b, bool border,
                                       me_v3& p) {
    double q[10];
    for (int i = 0; i < 10; ++i) q[i] = Q[10 * (long)a + i] + Q[10 * (long)b + i];
    const double det = ms_det3(q, 0, 1, 2, 1, 4, 5, 2, 5, 7);
    if (det != 0 && !border) {
        p.x = -1 / det * ms_det3(q, 1, 2, 3, 4, 5, 6, 5, 7, 8);
        p.y = 1 / det * ms_det3(q, 0, 2, 3, 1, 5, 6, 2, 7, 8);
        p.z = -1 / det * ms_det3(q, 0, 1, 3, 1, 4, 6, 2, 5, 8);
        const double err = ms_vertex_error(q, p);
        if (isfinite(p.x) && isfinite(p.y) && isfinite(p.z) && isfinite(err)) return err;
    }
    const me_v3 p1 = me_ld(P, a), p2 = me_ld(P, b);
    const me_v3 p3 = me_v3{(p1.x + p2.x) / 2, (p1.y + p2.y) / 2, (p1.z + p2.z) / 2};
    const double e1 = ms_vertex_error(q, p1), e2 = ms_vertex_error(q, p2), e3 = ms_vertex_error(q, p3);
    const double err = fmin(e1, fmin(e2, e3));
    p = p1;
    if (e2 == err) p = p2;
    if (e3 == err) p = p3;
    return err;
}

// One side of the legality test of collapsing (x, other) to p, over the faces around x that survive:
//   - `flipped` (Simplify.h:541-569) against the face's current normal; a face that has no normal now cannot flip, and
//     a face whose corner would coincide with p degenerates;
//   - the link condition: a vertex next to both endpoints must be the apex of a face on the edge, and no surviving face
//     around `other` may span the same opposite edge (the collapse would lay two faces on each other).
static __device__ bool ms_side_legal(const int* __restrict__ F, const double* __restrict__ P, const double* __restrict__ fn,
                                     const int* __restrict__ voff, const int* __restrict__ adj, int x, int other, me_v3 p,
                                     int apex0, int apex1, bool link) {
    for (int k = voff[x]; k < voff[x + 1]; ++k) {
        const long g = adj[k] >> 2;
        const int s = adj[k] & 3;
        const int id1 = F[3 * g + (s + 1) % 3], id2 = F[3 * g + (s + 2) % 3];
        if (id1 == other || id2 == other) continue;
        if (id1 == x || id2 == x) return false;
        bool ok1, ok2, okn;
        const me_v3 d1 = ms_unit(me_sub(me_ld(P, id1), p), ok1), d2 = ms_unit(me_sub(me_ld(P, id2), p), ok2);
        if (!ok1 || !ok2) return false;
        if (fabs(me_dot(d1, d2)) > 0.999) return false;
        const me_v3 n = ms_unit(me_cross(d1, d2), okn);
        if (!okn) return false;
        const me_v3 old = me_v3{fn[3 * g], fn[3 * g + 1], fn[3 * g + 2]};
        if ((old.x != 0 || old.y != 0 || old.z != 0) && !(me_dot(n, old) >= 0.2)) return false;
        if (!link) continue;
        bool n1 = false, n2 = false;
        for (int m = voff[other]; m < voff[other + 1]; ++m) {
            const long h = adj[m] >> 2;
            const bool h1 = ms_face_has(F, h, id1), h2 = ms_face_has(F, h, id2);
            if (h1 && h2) return false;
            n1 |= h1, n2 |= h2;
        }
        if (n1 && id1 != apex0 && id1 != apex1) return false;
        if (n2 && id2 != apex0 && id2 != apex1) return false;
    }
    return true;
}

// A bijection of the 32-bit edge ids (the finaliser of MurmurHash3): neighbouring edges get unrelated ranks.
static __device__ __forceinline__ unsigned ms_mix(unsigned h) {
    h ^= h >> 16, h *= 0x85ebca6bu, h ^= h >> 13, h *= 0xc2b2ae35u, h ^= h >> 16;
    return h;
}
// The key orders edges by cost class, then by the mixed edge id.  A class is the cost's sign, exponent and upper
// MS_COST_BITS - 12 mantissa bits: costs vary smoothly over a surface and edge ids follow the face order, so a key of the
// full cost, or of the plain id among equal costs (every edge of a flat region costs 0), has one local minimum per
// smooth patch and a round would collapse a handful of edges.  Within a class the mixed id gives a winner every few
// edges.  The keys are distinct because the mix is a bijection.
#define MS_COST_BITS 14
static __device__ __forceinline__ ms_u64 ms_key(double cost, long e) {
    const long long b = __double_as_longlong(cost);
    const ms_u64 u = b < 0 ? ~(ms_u64)b : ((ms_u64)b | 0x8000000000000000ull);   // order-preserving
    return ((u >> (64 - MS_COST_BITS)) << 32) | (ms_u64)ms_mix((unsigned)e);
}
template <typename Fn>
static __device__ __forceinline__ void ms_for_neighbourhood(const int* __restrict__ F, const int* __restrict__ voff,
                                                            const int* __restrict__ adj, int a, int b, Fn fn) {
    for (int side = 0; side < 2; ++side) {
        const int x = side ? b : a;
        for (int k = voff[x]; k < voff[x + 1]; ++k) {
            const long g = adj[k] >> 2;
            fn(F[3 * g]), fn(F[3 * g + 1]), fn(F[3 * g + 2]);
        }
    }
}

// one thread per half-edge; the half-edge on the lowest face of its undirected edge owns the edge (edge id = 3 f + j)
static __global__ __launch_bounds__(ME_BLOCK) void ms_edges_kernel(
    const int* __restrict__ F, long n3, const double* __restrict__ P, const double* __restrict__ Q, const double* __restrict__ fn,
    const int* __restrict__ voff, const int* __restrict__ adj, const int* __restrict__ border, const int* __restrict__ alive,
    double threshold, ms_u64* __restrict__ ekey, double* __restrict__ etgt, int* __restrict__ erem, ms_u64* __restrict__ vkey) {
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n3) return;
    ekey[e] = MS_NOKEY;
    erem[e] = 0;
    const long f = e / 3;
    if (!alive[f]) return;
    const int j = (int)(e % 3);
    const int a = F[3 * f + j], b = F[3 * f + (j + 1) % 3];
    if (a == b || border[a] != border[b]) return;   // Simplify.h:399
    int c = 0, apex[2] = {-1, -1};
    for (int k = voff[a]; k < voff[a + 1]; ++k) {
        const long g = adj[k] >> 2;
        if (!ms_face_has(F, g, b)) continue;
        if (c == 0 && g != f) return;               // a lower face owns this edge
        if (c < 2) apex[c] = (int)((long long)F[3 * g] + F[3 * g + 1] + F[3 * g + 2] - a - b);
        ++c;
    }
    // interior edges have two faces with two apexes; an edge with one face is a border edge; a chord between two border
    // vertices would pinch the surface
    if (c > 2 || (c == 2 && (apex[0] == apex[1] || border[a]))) return;
    me_v3 p;
    const double cost = ms_edge_error(Q, P, a, b, border[a] != 0, p);
    if (!(cost <= threshold)) return;
    if (!ms_side_legal(F, P, fn, voff, adj, a, b, p, apex[0], apex[1], true)) return;
    if (!ms_side_legal(F, P, fn, voff, adj, b, a, p, apex[0], apex[1], false)) return;
    const ms_u64 key = ms_key(cost, e);
    ekey[e] = key;
    erem[e] = c;
    etgt[3 * e] = p.x, etgt[3 * e + 1] = p.y, etgt[3 * e + 2] = p.z;
    ms_for_neighbourhood(F, voff, adj, a, b, [&](int v) { atomicMin(&vkey[v], key); });
}

// A candidate wins if it holds the minimum at its own two endpoints.  Two candidates disturb each other exactly when an
// endpoint of one lies in the closed neighbourhood of the other's endpoints (only then does one read a position or a
// face that the other changes), and that relation is symmetric: each has then written its key to an endpoint of the
// other, so at most the smaller key wins.  Winners therefore own disjoint faces and read nothing a winner writes.
// Their keys and face counts are listed (in any order: only integer sums and comparisons read the list).
static __global__ __launch_bounds__(ME_BLOCK) void ms_winners_kernel(const int* __restrict__ F, long n3, const int* __restrict__ voff,
                                                                     const int* __restrict__ adj, const ms_u64* __restrict__ ekey,
                                                                     const ms_u64* __restrict__ vkey, int* __restrict__ erem,
                                                                     ms_u64* __restrict__ wkey, int* __restrict__ wrem,
                                                                     int* __restrict__ flags) {
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n3) return;
    const ms_u64 key = ekey[e];
    if (key == MS_NOKEY) return;
    const long f = e / 3;
    const int j = (int)(e % 3);
    const int a = F[3 * f + j], b = F[3 * f + (j + 1) % 3];
    if (vkey[a] != key || vkey[b] != key) {
        erem[e] = 0;
        return;
    }
    const int slot = atomicAdd(&flags[1], 1);
    wkey[slot] = key;
    wrem[slot] = erem[e];
    atomicAdd(&flags[2], erem[e]);
}

// flags[3] holds the live face count.  With need = live - target: K = the smallest key such that the winners with key <= K
// remove at least `need` faces; every winner when all of them together remove no more than that (otherwise a bitwise
// search over the list), none when the target is reached already.  The count is brought up to date.  One block.
static __global__ __launch_bounds__(ME_BLOCK) void ms_select_kernel(const ms_u64* __restrict__ wkey, const int* __restrict__ wrem,
                                                                    int* __restrict__ flags, long target, ms_u64* __restrict__ ksel) {
    __shared__ long s_sum[ME_BLOCK];
    const int n = flags[1];
    const long total = flags[2], need = (long)flags[3] - target;
    __syncthreads();   // every thread has read the count before thread 0 updates it
    if (need <= 0 || total <= need) {
        if (threadIdx.x == 0) {
            *ksel = need <= 0 ? 0 : MS_NOKEY;
            if (need > 0) flags[3] -= (int)total;
        }
        return;
    }
    ms_u64 prefix = 0;
    for (int bit = 63; bit >= -1; --bit) {   // the pass at bit = -1 only sums what the chosen key removes
        const ms_u64 k = bit >= 0 ? prefix | ((1ull << bit) - 1) : prefix;   // this bit 0, every lower bit 1
        long s = 0;
        for (int i = threadIdx.x; i < n; i += ME_BLOCK) s += wkey[i] <= k ? wrem[i] : 0;
        s_sum[threadIdx.x] = s;
        __syncthreads();
        for (int h = ME_BLOCK / 2; h > 0; h >>= 1) {
            if ((int)threadIdx.x < h) s_sum[threadIdx.x] += s_sum[threadIdx.x + h];
            __syncthreads();
        }
        const long sum = s_sum[0];
        __syncthreads();
        if (bit < 0) {
            if (threadIdx.x == 0) *ksel = prefix, flags[3] -= (int)sum;
        } else if (sum < need) {
            prefix |= 1ull << bit;
        }
    }
}

// v0 moves to the target and takes v1's quadric (Simplify.h:418-419), the faces around v1 name v0 instead, the faces
// on the edge die.  Winners own disjoint faces and vertices.
static __global__ __launch_bounds__(ME_BLOCK) void ms_apply_kernel(int* __restrict__ F, long n3, const int* __restrict__ voff,
                                                                   const int* __restrict__ adj, const ms_u64* __restrict__ ekey,
                                                                   const int* __restrict__ erem, const double* __restrict__ etgt,
                                                                   const ms_u64* __restrict__ ksel, double* __restrict__ P,
                                                                   double* __restrict__ Q, int* __restrict__ alive) {
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n3 || erem[e] == 0 || ekey[e] > *ksel) return;
    const long f = e / 3;
    const int j = (int)(e % 3);
    const int a = F[3 * f + j], b = F[3 * f + (j + 1) % 3];
    for (int i = 0; i < 3; ++i) P[3 * (long)a + i] = etgt[3 * e + i];
    for (int i = 0; i < 10; ++i) Q[10 * (long)a + i] += Q[10 * (long)b + i];
    for (int k = voff[b]; k < voff[b + 1]; ++k) {
        const long g = adj[k] >> 2;
        if (ms_face_has(F, g, a))
            alive[g] = 0;
        else
            F[3 * g + (adj[k] & 3)] = a;
    }
}

static __global__ void ms_fill_kernel(int* __restrict__ p, long n, int value) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = value;
}
static __global__ void ms_compact_kernel(const int* __restrict__ F, long nf, const int* __restrict__ alive,
                                         const int* __restrict__ foff, int* __restrict__ G) {
    const long f = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= nf || !alive[f]) return;
    const long d = foff[f];
    G[3 * d] = F[3 * f], G[3 * d + 1] = F[3 * f + 1], G[3 * d + 2] = F[3 * f + 2];
}

// =============================================================================================
// output
// =============================================================================================
static __global__ void ms_mark_kernel(const int* __restrict__ F, long n3, int* __restrict__ used) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n3) used[F[i]] = 1;
}
static __global__ void ms_header_kernel(long long* __restrict__ hdr, long long nf_out, const int* __restrict__ vmap, long nv) {
    hdr[0] = nf_out;
    hdr[1] = vmap[nv];
}
static __global__ void ms_emit_faces_kernel(const int* __restrict__ F, const long long* __restrict__ hdr,
                                            const int* __restrict__ vmap, long long* __restrict__ out) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < 3 * hdr[0]) out[i] = vmap[F[i]];
}

// =============================================================================================
// host
// =============================================================================================
static int simp_check(long nv, long nf, const void* ws, size_t ws_bytes, SimpWs& w, const char* what) {
    S3D_CHECK_ARG(nf >= 1, "%s: the mesh has no face", what);
    S3D_CHECK_ARG(nf < MS_FACES_MAX && nv >= 1 && nv < (1L << 31), "%s: %ld faces, %ld vertices (faces < 2^29, vertices < 2^31)",
                  what, nf, nv);
    S3D_CHECK_ARG(ws != nullptr, "%s: null workspace", what);
    const size_t need = simp_layout(nv, nf, w, nullptr);
    S3D_CHECK_ARG(ws_bytes >= need, "%s: workspace %zu < %zu bytes", what, ws_bytes, need);
    simp_layout(nv, nf, w, (char*)ws);
    return 0;
}

// alive -> the other face buffer, in order; the live count comes back to the host
static int ms_compact(SimpWs& w, int*& cur, int*& other, long& live, hipStream_t st) {
    me_scan<int, int, false>(w.alive, w.foff, live, w.tsum, st);
    ME_LAUNCH(ms_compact_kernel, live, st, cur, live, w.alive, w.foff, other);
    S3D_LAUNCH_CHECK();
    int total = 0;
    S3D_HIP_TRY("mesh_simplify_run", hipMemcpyAsync(&total, me_scan_total(w.tsum, live), 4, hipMemcpyDeviceToHost, st));
    S3D_HIP_TRY("mesh_simplify_run", hipStreamSynchronize(st));
    std::swap(cur, other);
    live = total;
    // every listed face is alive again; flags[3] is the count the passes of the next round keep up to date
    ME_LAUNCH(ms_fill_kernel, live, st, w.alive, live, 1);
    ME_LAUNCH(ms_fill_kernel, 1L, st, w.flags + 3, 1L, total);
    S3D_LAUNCH_CHECK();
    return 0;
}

// One pass over the `listed` faces (the live ones and those that died since the last compaction) at the round's threshold.
static int ms_pass(SimpWs& w, int* cur, long listed, bool quadrics, long target, double threshold, hipStream_t st) {
    const long nv = w.nv, n3 = 3 * listed;
    S3D_HIP_TRY("mesh_simplify_run", hipMemsetAsync(w.vcnt, 0, (size_t)(nv + 1) * 4, st));
    ME_LAUNCH(ms_vcount_kernel, n3, st, cur, n3, w.alive, w.vcnt);
    me_scan<int, int, false>(w.vcnt, w.voff, nv + 1, w.tsum, st);
    S3D_HIP_TRY("mesh_simplify_run", hipMemsetAsync(w.vcnt, 0, (size_t)(nv + 1) * 4, st));
    ME_LAUNCH(ms_vfill_kernel, n3, st, cur, n3, w.alive, w.voff, w.vcnt, w.adj);
    ME_LAUNCH(ms_vsort_kernel, nv, st, w.voff, nv, w.adj);
    ME_LAUNCH(ms_normals_kernel, listed, st, cur, listed, w.P, w.alive, w.fn);
    if (quadrics)
        ME_LAUNCH(ms_quadrics_kernel, nv, st, cur, w.P, w.fn, w.voff, w.adj, nv, w.Q);
    S3D_HIP_TRY("mesh_simplify_run", hipMemsetAsync(w.border, 0, (size_t)nv * 4, st));
    S3D_HIP_TRY("mesh_simplify_run", hipMemsetAsync(w.vkey, 0xFF, (size_t)nv * 8, st));
    S3D_HIP_TRY("mesh_simplify_run", hipMemsetAsync(w.flags + 1, 0, 8, st));
    ME_LAUNCH(ms_border_kernel, n3, st, cur, n3, w.alive, w.voff, w.adj, w.border);
    ME_LAUNCH(ms_edges_kernel, n3, st, cur, n3, w.P, w.Q, w.fn, w.voff, w.adj, w.border, w.alive, threshold, w.ekey, w.etgt,
              w.erem, w.vkey);
    ME_LAUNCH(ms_winners_kernel, n3, st, cur, n3, w.voff, w.adj, w.ekey, w.vkey, w.erem, w.wkey, w.wrem, w.flags);
    hipLaunchKernelGGL(ms_select_kernel, dim3(1), dim3(ME_BLOCK), 0, st, w.wkey, w.wrem, w.flags, target, w.ksel);
    ME_LAUNCH(ms_apply_kernel, n3, st, cur, n3, w.voff, w.adj, w.ekey, w.erem, w.etgt, w.ksel, w.P, w.Q, w.alive);
    S3D_LAUNCH_CHECK();
    return 0;
}

// A round at step k of the schedule: MS_PASSES passes at the threshold 1e-9 (k + 3)^aggressiveness (Simplify.h:378).  The reference's iteration
// sweeps every triangle and collapses whatever is below the threshold and not next to a collapse of the same sweep; one
// independent set takes a few per cent of the faces, so a round makes several before the threshold moves on.  The passes
// need no host decision (the kernels skip dead faces and keep the live count in flags[3]); the compaction after them
// brings the round's one synchronisation.
#define MS_PASSES 4
#define MS_STALL 8
static int ms_round(SimpWs& w, int* cur, long listed, int k, bool first, long target, double aggressiveness, hipStream_t st) {
    const double threshold = 0.000000001 * pow((double)(k + 3), aggressiveness);
    for (int pass = 0; pass < MS_PASSES; ++pass)
        TRY_RET(ms_pass(w, cur, listed, first && pass == 0, target, threshold, st));
    return 0;
}

extern "C" size_t s3d_mesh_simplify_workspace_bytes(long n_vertices, long n_faces) {
    if (n_faces < 1 || n_faces >= MS_FACES_MAX || n_vertices < 1 || n_vertices >= (1L << 31)) return 0;
    SimpWs w;
    return simp_layout(n_vertices, n_faces, w, nullptr);
}

extern "C" int s3d_mesh_simplify_run(const double* vertices, long n_vertices, const long long* faces, long n_faces,
                                     long target_faces, double aggressiveness, void* workspace, size_t workspace_bytes,
                                     long* n_vertices_out, long* n_faces_out, int* n_rounds, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    SimpWs w;
    S3D_CHECK_ARG(n_vertices_out && n_faces_out && n_rounds, "mesh_simplify_run: null output count");
    S3D_CHECK_ARG(target_faces >= 0, "mesh_simplify_run: target_faces = %ld < 0", target_faces);
    S3D_CHECK_ARG(n_faces == 0 || (vertices && faces), "mesh_simplify_run: null mesh");
    TRY_RET(simp_check(n_vertices, n_faces, workspace, workspace_bytes, w, "mesh_simplify_run"));
    *n_vertices_out = *n_faces_out = 0;
    *n_rounds = 0;
    const long nv = n_vertices;
    // the indices are checked before anything dereferences them
    S3D_HIP_TRY("mesh_simplify_run", hipMemsetAsync(w.flags, 0, 16 * 4, st));
    ME_LAUNCH(ms_validate_kernel, 3 * n_faces, st, faces, 3 * n_faces, nv, w.flags);
    S3D_LAUNCH_CHECK();
    int bad = 0;
    S3D_HIP_TRY("mesh_simplify_run", hipMemcpyAsync(&bad, w.flags, 4, hipMemcpyDeviceToHost, st));
    S3D_HIP_TRY("mesh_simplify_run", hipStreamSynchronize(st));
    S3D_CHECK_ARG(!bad, "mesh_simplify_run: a face indexes a vertex outside [0, %ld)", n_vertices);

    S3D_HIP_TRY("mesh_simplify_run", hipMemcpyAsync(w.P, vertices, (size_t)nv * 24, hipMemcpyDeviceToDevice, st));
    int *cur = w.FA, *other = w.FB;
    long live = n_faces;
    const bool work = target_faces < n_faces;
    ME_LAUNCH(ms_import_kernel, live, st, faces, live, cur, w.alive, work ? 1 : 0);
    S3D_LAUNCH_CHECK();
    int rounds = 0;
    if (work) {
        TRY_RET(ms_compact(w, cur, other, live, st));
        // The reference's sweep leaves little below its threshold before the next iteration raises it.  A round here
        // takes less, so the schedule moves on (k) only after a round that removed under 1 / MS_STALL of the faces:
        // cheap collapses are used up before dearer ones are admitted.
        for (int k = 0; rounds < MS_MAX_ROUNDS && live > target_faces && live > 0; ++rounds) {
            const long before = live;
            TRY_RET(ms_round(w, cur, live, k, rounds == 0, target_faces, aggressiveness, st));
            TRY_RET(ms_compact(w, cur, other, live, st));
            if ((before - live) * MS_STALL < before) ++k;
        }
    }
    // s3d_mesh_simplify_emit reads FA
    if (cur != w.FA && live > 0)
        S3D_HIP_TRY("mesh_simplify_run", hipMemcpyAsync(w.FA, cur, (size_t)live * 12, hipMemcpyDeviceToDevice, st));
    // referenced vertices keep their order: used -> vcnt, new index -> vmap
    S3D_HIP_TRY("mesh_simplify_run", hipMemsetAsync(w.vcnt, 0, (size_t)(nv + 1) * 4, st));
    ME_LAUNCH(ms_mark_kernel, 3 * live, st, w.FA, 3 * live, w.vcnt);
    me_scan<int, int, false>(w.vcnt, w.vmap, nv + 1, w.tsum, st);
    hipLaunchKernelGGL(ms_header_kernel, dim3(1), dim3(1), 0, st, w.hdr, (long long)live, w.vmap, nv);
    S3D_LAUNCH_CHECK();
    int nv_out = 0;
    S3D_HIP_TRY("mesh_simplify_run", hipMemcpyAsync(&nv_out, w.vmap + nv, 4, hipMemcpyDeviceToHost, st));
    S3D_HIP_TRY("mesh_simplify_run", hipStreamSynchronize(st));
    *n_vertices_out = nv_out;
    *n_faces_out = live;
    *n_rounds = rounds;
    return 0;
}

extern "C" int s3d_mesh_simplify_emit(const void* workspace, size_t workspace_bytes, long n_vertices, long n_faces,
                                      double* vertices_out, long long* faces_out, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    SimpWs w;
    TRY_RET(simp_check(n_vertices, n_faces, workspace, workspace_bytes, w, "mesh_simplify_emit"));
    S3D_CHECK_ARG(vertices_out && faces_out, "mesh_simplify_emit: null output");
    ME_LAUNCH(me_emit_vertices_kernel, n_vertices, st, w.P, w.vcnt, w.vmap, n_vertices, vertices_out);
    ME_LAUNCH(ms_emit_faces_kernel, 3 * n_faces, st, w.FA, w.hdr, w.vmap, faces_out);
    S3D_LAUNCH_CHECK();
    return 0;
}

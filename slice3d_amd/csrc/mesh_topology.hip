// mesh_topology.hip — what a triangle mesh is made of: weld of equal positions, connected
// components, per-component topology counts and measures, and the order-preserving removal of components.
//
// Weld: the referenced vertices go into an open-addressing hash table of vertex indices (linear probing, integer
// atomicCAS to claim a slot, integer atomicMin to leave the smallest index of the class in it); a second launch reads the
// representatives back.  Components: every vertex carries a label, a vertex of its own component with an index no larger
// than its own.  A round is three launches: hook (a face lowers the labels of its vertices and of their labels to the
// smallest of them by integer atomicMin), compress (pointer jumping to the root) and check (every face re-read).  Labels
// only ever decrease and every value a label ever held stays a valid one, so a stale read costs work and never the
// result; at convergence a component's label is its smallest vertex index.  The counts come from vertex -> half-edge
// lists (only counts and minima are taken over a list, so its order does not matter); the float64 sums run over a
// component's faces in ascending face index, in blocks of TP_CHUNK faces whose sums are added in ascending order, so the
// bits are the same from run to run.  No float atomic, no wait on another workgroup anywhere.
#include <algorithm>

#include "mesh_common.h"

#define TP_MAX_ROUNDS 64             // hook / compress / check rounds; more is S3D_E_ROUNDS
#define TP_FACES_MAX (1L << 29)      // 3 * n_faces (half-edge ids) stays inside 31 bits
#define TP_CHUNK 256                 // faces per block of a component's ordered sums
#define TP_NI 11                     // integer columns of a table row
#define TP_ND 8                      // float64 columns of a table row
#define TP_PI 8                      // integer partials per run of faces
#define TP_HDR 8                     // 64-bit words of the workspace header
#define TP_MAGIC 0x746f706f6c6f6779ll

// half-edge status bits
#define TP_S_EDGE 1                  // the lowest half-edge of its undirected edge
#define TP_S_CLASS_SHIFT 1           // 2 bits: 1, 2 or 3 (= three or more) half-edges on the undirected edge
#define TP_S_CONFLICT 8              // the lowest half-edge of a directed edge that occurs more than once
#define TP_S_VERTEX 16               // the lowest half-edge that starts at its vertex

// flags: [0] bad face index, [1] non-finite referenced vertex, [2] a face whose labels still differ
struct TopoWs {
    int* flags;
    long long* hdr;      // [0] faces out, [1] vertices out of the last keep; [2] TP_MAGIC once run has completed, [3] K,
                         // [4] vertices, [5] faces, [6] weld of that run; [7] TP_MAGIC once a keep_run has completed
    long long* sumI;     // the summary row
    double* sumD;
    int *tsum, *vmap, *W, *L, *ref, *refw, *cid, *vcnt, *voff, *vown, *adj, *fcomp, *ordA, *ordB, *z, *zoff, *seg;
    unsigned char* stat;
    int *partI, *spartI, *table;
    double *partD, *spartD;
    long nv, nf, hsize;
};

static long tp_hash_size(long nv) {
    long h = 64;
    while (h < 2 * nv) h <<= 1;
    return h;
}

// the arrays in the workspace's order; base == nullptr: only the size
static size_t topo_layout(long nv, long nf, int weld, TopoWs& w, char* base) {
    MeArena a{base};
    const size_t V = (size_t)nv, F = (size_t)nf;
    const long tiles = (std::max(nv + 1, nf) + ME_TILE - 1) / ME_TILE;
    const size_t chunks = (size_t)((nf + TP_CHUNK - 1) / TP_CHUNK + 1);
    w.nv = nv, w.nf = nf, w.hsize = weld ? tp_hash_size(nv) : 0;
    w.flags = a.take<int>(16), w.hdr = a.take<long long>(TP_HDR), w.sumI = a.take<long long>(TP_NI);
    w.sumD = a.take<double>(TP_ND), w.tsum = a.take<int>(tiles + 2);
    w.vmap = a.take<int>(V), w.W = a.take<int>(3 * F), w.L = a.take<int>(V), w.ref = a.take<int>(V);
    w.refw = a.take<int>(V + 1), w.cid = a.take<int>(V + 1), w.vcnt = a.take<int>(V + 1), w.voff = a.take<int>(V + 1);
    w.vown = a.take<int>(V), w.adj = a.take<int>(3 * F), w.fcomp = a.take<int>(F), w.ordA = a.take<int>(F);
    w.ordB = a.take<int>(F), w.z = a.take<int>(F), w.zoff = a.take<int>(F), w.seg = a.take<int>(F + 1);
    w.stat = a.take<unsigned char>(3 * F);
    w.partI = a.take<int>(F * TP_PI), w.partD = a.take<double>(F * TP_ND);
    w.spartI = a.take<int>(chunks * TP_PI), w.spartD = a.take<double>(chunks * TP_ND);
    w.table = a.take<int>(w.hsize);
    return a.off;
}

// =============================================================================================
// input
// =============================================================================================
// every index is checked here, before anything dereferences it; the valid ones mark their vertex as referenced
static __global__ void tp_validate_kernel(const long long* __restrict__ faces, long n3, long nv, int* __restrict__ ref,
                                          int* __restrict__ flags) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n3) return;
    const long long v = faces[i];
    if (v < 0 || v >= nv)
        flags[0] = 1;
    else
        ref[v] = 1;
}
static __global__ void tp_iota_kernel(int* __restrict__ p, long n) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = (int)i;
}
static __global__ void tp_finite_kernel(const double* __restrict__ P, const int* __restrict__ ref, long nv, int* __restrict__ flags) {
    const long v = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= nv || !ref[v]) return;
    if (!(isfinite(P[3 * v]) && isfinite(P[3 * v + 1]) && isfinite(P[3 * v + 2]))) flags[1] = 1;
}

// =============================================================================================
// weld
// =============================================================================================
static __device__ __forceinline__ bool tp_same_position(const double* __restrict__ P, long a, long b) {
    return P[3 * a] == P[3 * b] && P[3 * a + 1] == P[3 * b + 1] && P[3 * a + 2] == P[3 * b + 2];   // -0.0 == +0.0
}
static __device__ __forceinline__ unsigned long long tp_mix64(unsigned long long h) {   // the finaliser of MurmurHash3
    h ^= h >> 33, h *= 0xff51afd7ed558ccdull, h ^= h >> 33, h *= 0xc4ceb9fe1a85ec53ull, h ^= h >> 33;
    return h;
}
static __device__ __forceinline__ unsigned long long tp_coord_bits(double x) {
    return (unsigned long long)__double_as_longlong(x == 0.0 ? 0.0 : x);   // both zeros hash alike
}
// A referenced vertex walks from its hash to the slot of its class: an empty slot is claimed by atomicCAS, a slot held
// by a vertex at the same position is its class's.  Slots never empty again, so every member of a class ends at the
// same slot; atomicMin leaves the class's smallest index there.  The slot's value is read through the atomic itself.
// Any member serves for the comparison (all have equal coordinates).  At most `hsize` probes; the table has at least
// twice as many slots as vertices, so a free slot exists.
static __global__ void tp_weld_insert_kernel(const double* __restrict__ P, const int* __restrict__ ref, long nv,
                                             int* __restrict__ table, long hsize, int* __restrict__ slot_of) {
    const long v = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= nv || !ref[v]) return;
    unsigned long long h = tp_mix64(tp_coord_bits(P[3 * v]));
    h = tp_mix64(h ^ tp_coord_bits(P[3 * v + 1]));
    h = tp_mix64(h ^ tp_coord_bits(P[3 * v + 2]));
    const unsigned long long mask = (unsigned long long)hsize - 1;
    long at = -1;
    for (long probe = 0; probe < hsize; ++probe) {
        const long s = (long)((h + (unsigned long long)probe) & mask);
        const int old = atomicCAS(&table[s], -1, (int)v);
        if (old == -1 || tp_same_position(P, old, v)) {
            at = s;
            break;
        }
    }
    slot_of[v] = (int)at;
    if (at >= 0) atomicMin(&table[at], (int)v);
}
static __global__ void tp_weld_read_kernel(const int* __restrict__ ref, long nv, const int* __restrict__ table,
                                           int* __restrict__ vmap) {
    const long v = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= nv || !ref[v]) return;     // a vertex no face references stays its own
    const int s = vmap[v];              // its slot, left by the insert
    vmap[v] = s >= 0 ? table[s] : (int)v;
}
// int64 faces -> welded int32 faces; the welded vertices they name are marked
static __global__ void tp_import_kernel(const long long* __restrict__ faces, long n3, const int* __restrict__ vmap,
                                        int* __restrict__ W, int* __restrict__ refw) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n3) return;
    const int v = vmap[faces[i]];
    W[i] = v;
    refw[v] = 1;
}

// =============================================================================================
// components
// =============================================================================================
static __global__ void tp_hook_kernel(const int* __restrict__ W, long nf, int* __restrict__ L) {
    const long f = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= nf) return;
    const int a = W[3 * f], b = W[3 * f + 1], c = W[3 * f + 2];
    const int la = L[a], lb = L[b], lc = L[c];
    if (la == lb && lb == lc) return;
    const int m = min(la, min(lb, lc));
    // the vertices and their labels: all of one component, none below its smallest index
    if (la > m) atomicMin(&L[la], m), atomicMin(&L[a], m);
    if (lb > m) atomicMin(&L[lb], m), atomicMin(&L[b], m);
    if (lc > m) atomicMin(&L[lc], m), atomicMin(&L[c], m);
}
// labels strictly decrease along a chain, so it ends at a root after fewer than nv steps
static __global__ void tp_compress_kernel(int* __restrict__ L, const int* __restrict__ refw, long nv) {
    const long v = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= nv || !refw[v]) return;
    int r = L[v];
    for (long step = 0; step < nv; ++step) {
        const int p = L[r];
        if (p >= r) break;
        r = p;
    }
    if (r < L[v]) atomicMin(&L[v], r);
}
static __global__ void tp_check_kernel(const int* __restrict__ W, long nf, const int* __restrict__ L, int* __restrict__ flags) {
    const long f = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= nf) return;
    const int la = L[W[3 * f]], lb = L[W[3 * f + 1]], lc = L[W[3 * f + 2]];
    if (la != lb || lb != lc || L[la] != la) flags[2] = 1;
}
static __global__ void tp_roots_kernel(const int* __restrict__ L, const int* __restrict__ refw, long nv, int* __restrict__ root) {
    const long v = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (v <= nv) root[v] = v < nv && refw[v] && L[v] == (int)v;
}
static __global__ void tp_face_component_kernel(const int* __restrict__ W, long nf, const int* __restrict__ L,
                                                const int* __restrict__ cid, int* __restrict__ fcomp) {
    const long f = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (f < nf) fcomp[f] = cid[L[W[3 * f]]];
}

// =============================================================================================
// vertex -> half-edge lists (half-edge 3 f + j runs from corner j of face f to corner j + 1) and the half-edge status
// =============================================================================================
static __global__ void tp_vcount_kernel(const int* __restrict__ W, long n3, int* __restrict__ vcnt) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n3) atomicAdd(&vcnt[W[i]], 1);
}
// the list's order depends on scheduling; only counts and minima are ever taken over it
static __global__ void tp_vfill_kernel(const int* __restrict__ W, long n3, const int* __restrict__ voff, int* __restrict__ vcnt,
                                       int* __restrict__ adj, int* __restrict__ vown) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n3) return;
    const int v = W[i];
    adj[voff[v] + atomicAdd(&vcnt[v], 1)] = (int)i;
    atomicMin(&vown[v], (int)i);
}
static __device__ __forceinline__ long tp_next(long t) { return t - t % 3 + (t + 1) % 3; }
static __device__ __forceinline__ long tp_prev(long t) { return t - t % 3 + (t + 2) % 3; }

// One thread per half-edge (a, b).  The half-edges between the same two vertices are found around the endpoint with
// the shorter list: a list entry t (W[t] == x) stands for the outgoing half-edge t and the incoming tp_prev(t).  For
// a == b (a face that repeats an index) every such half-edge is outgoing and incoming at once and is counted once.
static __global__ __launch_bounds__(ME_BLOCK) void tp_edges_kernel(const int* __restrict__ W, long n3, const int* __restrict__ voff,
                                                                   const int* __restrict__ adj, const int* __restrict__ vown,
                                                                   unsigned char* __restrict__ stat) {
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n3) return;
    const int a = W[e], b = W[tp_next(e)];
    const int na = voff[a + 1] - voff[a], nb = voff[b + 1] - voff[b];
    const int x = (nb < na) ? b : a, y = (nb < na) ? a : b;
    const bool x_is_a = x == a;
    int n_und = 0, n_same = 0;
    long min_und = n3, min_same = n3;
    for (int k = voff[x]; k < voff[x + 1]; ++k) {
        const long t = adj[k];
        if (W[tp_next(t)] == y) {   // t runs x -> y
            ++n_und, min_und = min(min_und, t);
            if (x_is_a) ++n_same, min_same = min(min_same, t);
        }
        if (a != b && W[tp_prev(t)] == y) {   // tp_prev(t) runs y -> x
            const long u = tp_prev(t);
            ++n_und, min_und = min(min_und, u);
            if (!x_is_a) ++n_same, min_same = min(min_same, u);
        }
    }
    int s = 0;
    if (min_und == e) s |= TP_S_EDGE | (min(n_und, 3) << TP_S_CLASS_SHIFT);
    if (min_same == e && n_same > 1) s |= TP_S_CONFLICT;
    if (vown[a] == (int)e) s |= TP_S_VERTEX;
    stat[e] = (unsigned char)s;
}

// =============================================================================================
// faces in component order: a stable binary radix sort of the face indices by component id, lowest bit first
// =============================================================================================
static __global__ void tp_bit_kernel(const int* __restrict__ order, const int* __restrict__ fcomp, long nf, int bit, int* __restrict__ z) {
    const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p < nf) z[p] = !((fcomp[order[p]] >> bit) & 1);
}
// zoff = exclusive scan of z, *n_zero its total
static __global__ void tp_split_kernel(const int* __restrict__ order, const int* __restrict__ z, const int* __restrict__ zoff,
                                       const int* __restrict__ n_zero, long nf, int* __restrict__ out) {
    const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= nf) return;
    const long d = z[p] ? zoff[p] : (long)*n_zero + (p - zoff[p]);
    out[d] = order[p];
}

// =============================================================================================
// table: partial rows over runs of faces, then one row per component
// =============================================================================================
// Position p of the ordered face list (order == NULL: the face list itself) heads a run when it starts a chunk of
// TP_CHUNK positions or a component (fcomp == NULL: one component).  The head's thread walks its run, at most to the
// chunk's end, and writes the run's sums to row p (by_chunk: row p / TP_CHUNK): integers [vertices, edges, edges with 1,
// 2, 3+ half-edges, conflicts, degenerate faces, faces], float64 [area, sum of det / 6, bbox lo, bbox hi].
static __global__ __launch_bounds__(ME_BLOCK) void tp_partial_kernel(const int* __restrict__ order, const int* __restrict__ fcomp,
                                                                     long nf, const int* __restrict__ W,
                                                                     const unsigned char* __restrict__ stat,
                                                                     const double* __restrict__ P, int by_chunk,
                                                                     int* __restrict__ partI, double* __restrict__ partD,
                                                                     int* __restrict__ seg) {
    const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= nf) return;
    const int c = fcomp ? fcomp[order ? order[p] : p] : 0;
    const bool first = p == 0 || (fcomp && fcomp[order ? order[p - 1] : p - 1] != c);
    if (first && seg) seg[c] = (int)p;
    if (!first && p % TP_CHUNK != 0) return;
    const long end = min(nf, (p / TP_CHUNK + 1) * TP_CHUNK);
    int cnt[TP_PI] = {0, 0, 0, 0, 0, 0, 0, 0};
    double area = 0.0, det = 0.0;
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (long q = p; q < end; ++q) {
        const long f = order ? order[q] : q;
        if (fcomp && fcomp[f] != c) break;
        const int i0 = W[3 * f], i1 = W[3 * f + 1], i2 = W[3 * f + 2];
        for (int j = 0; j < 3; ++j) {
            const int s = stat[3 * f + j];
            cnt[0] += (s & TP_S_VERTEX) != 0;
            cnt[1] += s & TP_S_EDGE;
            const int cls = (s >> TP_S_CLASS_SHIFT) & 3;
            cnt[2] += cls == 1, cnt[3] += cls == 2, cnt[4] += cls == 3;
            cnt[5] += (s & TP_S_CONFLICT) != 0;
        }
        cnt[6] += i0 == i1 || i1 == i2 || i0 == i2;
        cnt[7] += 1;
        const me_v3 v0 = me_ld(P, i0), v1 = me_ld(P, i1), v2 = me_ld(P, i2);
        const me_v3 n = me_cross(me_v3{v1.x - v0.x, v1.y - v0.y, v1.z - v0.z}, me_v3{v2.x - v0.x, v2.y - v0.y, v2.z - v0.z});
        area += 0.5 * sqrt(n.x * n.x + n.y * n.y + n.z * n.z);
        const me_v3 m = me_cross(v1, v2);
        det += (v0.x * m.x + v0.y * m.y + v0.z * m.z) / 6.0;   // the volume term det(v0, v1, v2) / 6, then the sum
        lo[0] = fmin(lo[0], fmin(v0.x, fmin(v1.x, v2.x))), hi[0] = fmax(hi[0], fmax(v0.x, fmax(v1.x, v2.x)));
        lo[1] = fmin(lo[1], fmin(v0.y, fmin(v1.y, v2.y))), hi[1] = fmax(hi[1], fmax(v0.y, fmax(v1.y, v2.y)));
        lo[2] = fmin(lo[2], fmin(v0.z, fmin(v1.z, v2.z))), hi[2] = fmax(hi[2], fmax(v0.z, fmax(v1.z, v2.z)));
    }
    const long row = by_chunk ? p / TP_CHUNK : p;
    for (int i = 0; i < TP_PI; ++i) partI[TP_PI * row + i] = cnt[i];
    partD[TP_ND * row] = area, partD[TP_ND * row + 1] = det;
    for (int i = 0; i < 3; ++i) partD[TP_ND * row + 2 + i] = lo[i], partD[TP_ND * row + 5 + i] = hi[i];
}
// Row k of the table from the runs of component k, in ascending position: the run at the component's first position,
// then the runs at the chunk starts inside it.  seg == NULL: one component over [0, nf), rows by chunk.
static __global__ void tp_rows_kernel(const int* __restrict__ seg, long K, long nf, int by_chunk, const int* __restrict__ partI,
                                      const double* __restrict__ partD, long long* __restrict__ outI, double* __restrict__ outD) {
    const long k = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= K) return;
    const long s = seg ? seg[k] : 0, e = seg ? (k + 1 < K ? seg[k + 1] : nf) : nf;
    long long cnt[TP_PI] = {0, 0, 0, 0, 0, 0, 0, 0};
    double area = 0.0, det = 0.0;
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (long p = s; p < e; p = (p / TP_CHUNK + 1) * TP_CHUNK) {
        const long row = by_chunk ? p / TP_CHUNK : p;
        for (int i = 0; i < TP_PI; ++i) cnt[i] += partI[TP_PI * row + i];
        area += partD[TP_ND * row], det += partD[TP_ND * row + 1];
        for (int i = 0; i < 3; ++i) {
            lo[i] = fmin(lo[i], partD[TP_ND * row + 2 + i]);
            hi[i] = fmax(hi[i], partD[TP_ND * row + 5 + i]);
        }
    }
    long long* r = outI + TP_NI * k;
    r[0] = cnt[7], r[1] = cnt[0], r[2] = cnt[1], r[3] = cnt[2], r[4] = cnt[3], r[5] = cnt[4], r[6] = cnt[5], r[7] = cnt[6];
    r[8] = cnt[0] - cnt[1] + cnt[7];
    const bool oriented = cnt[7] > 0 && cnt[5] == 0 && cnt[4] == 0;   // no conflict, no edge with three or more
    r[9] = oriented && cnt[2] == 0;
    r[10] = oriented;
    double* d = outD + TP_ND * k;
    d[0] = area, d[1] = det;
    for (int i = 0; i < 3; ++i) d[2 + i] = e > s ? lo[i] : 0.0, d[5 + i] = e > s ? hi[i] : 0.0;
}

// =============================================================================================
// labels out, keep
// =============================================================================================
static __global__ void tp_emit_face_labels_kernel(const int* __restrict__ fcomp, long nf, long long* __restrict__ out) {
    const long f = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (f < nf) out[f] = fcomp[f];
}
static __global__ void tp_emit_vertex_labels_kernel(const int* __restrict__ ref, const int* __restrict__ vmap, const int* __restrict__ L,
                                                    const int* __restrict__ cid, long nv, long long* __restrict__ vmap_out,
                                                    long long* __restrict__ vcomp_out) {
    const long v = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= nv) return;
    if (vmap_out) vmap_out[v] = vmap[v];
    if (vcomp_out) vcomp_out[v] = ref[v] ? cid[L[vmap[v]]] : -1;
}
static __global__ void tp_keep_faces_kernel(const int* __restrict__ W, const int* __restrict__ fcomp, long nf,
                                            const unsigned char* __restrict__ keep, int drop, int* __restrict__ kept,
                                            int* __restrict__ used) {
    const long f = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= nf) return;
    const int a = W[3 * f], b = W[3 * f + 1], c = W[3 * f + 2];
    const int k = keep[fcomp[f]] && !(drop && (a == b || b == c || a == c));
    kept[f] = k;
    if (k) used[a] = 1, used[b] = 1, used[c] = 1;
}
static __global__ void tp_keep_header_kernel(long long* __restrict__ hdr, const int* __restrict__ n_faces, const int* __restrict__ vnew,
                                             long nv) {
    hdr[0] = *n_faces;
    hdr[1] = vnew[nv];
    hdr[7] = TP_MAGIC;
}
// the last launch of a run: what the emit and keep calls check their arguments against
static __global__ void tp_run_header_kernel(long long* __restrict__ hdr, long long K, long long nv, long long nf, long long weld) {
    hdr[0] = hdr[1] = hdr[7] = 0;
    hdr[3] = K, hdr[4] = nv, hdr[5] = nf, hdr[6] = weld;
    hdr[2] = TP_MAGIC;
}
static __global__ void tp_keep_emit_faces_kernel(const int* __restrict__ W, const int* __restrict__ kept, const int* __restrict__ foff,
                                                 const int* __restrict__ vnew, long nf, long long* __restrict__ out) {
    const long f = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= nf || !kept[f]) return;
    const long d = foff[f];
    out[3 * d] = vnew[W[3 * f]], out[3 * d + 1] = vnew[W[3 * f + 1]], out[3 * d + 2] = vnew[W[3 * f + 2]];
}

// =============================================================================================
// host
// =============================================================================================
static bool tp_sizes_ok(long nv, long nf) { return nf >= 0 && nf < TP_FACES_MAX && nv >= 0 && nv < (1L << 30); }

static int topo_check(long nv, long nf, int weld, const void* ws, size_t ws_bytes, TopoWs& w, const char* what) {
    S3D_CHECK_ARG(tp_sizes_ok(nv, nf), "%s: %ld faces, %ld vertices (faces < 2^29, vertices < 2^30)", what, nf, nv);
    S3D_CHECK_ARG(ws != nullptr, "%s: null workspace", what);
    const size_t need = topo_layout(nv, nf, weld, w, nullptr);
    S3D_CHECK_ARG(ws_bytes >= need, "%s: workspace %zu < %zu bytes", what, ws_bytes, need);
    topo_layout(nv, nf, weld, w, (char*)ws);
    return 0;
}

// The header a completed run left (one small read-back): the sizes and weld must be that run's, n_components (unless < 0)
// the K it found, and with `kept` a keep_run must have completed since.  Nothing reads seg, fcomp or the partial rows
// before this has passed.
static int topo_state(const TopoWs& w, int weld, long n_components, bool kept, const char* what, hipStream_t st) {
    long long h[TP_HDR];
    S3D_HIP_TRY(what, hipMemcpyAsync(h, w.hdr, sizeof h, hipMemcpyDeviceToHost, st));
    S3D_HIP_TRY(what, hipStreamSynchronize(st));
    S3D_CHECK_ARG(h[2] == TP_MAGIC, "%s: no completed s3d_mesh_topology_run on this workspace", what);
    S3D_CHECK_ARG(h[4] == w.nv && h[5] == w.nf && h[6] == weld,
                  "%s: %ld vertices, %ld faces, weld %d, but the run on this workspace had %lld, %lld, %lld", what, w.nv, w.nf,
                  weld, h[4], h[5], h[6]);
    S3D_CHECK_ARG(n_components < 0 || h[3] == n_components, "%s: %ld components, but the run found %lld", what, n_components, h[3]);
    S3D_CHECK_ARG(!kept || h[7] == TP_MAGIC, "%s: no completed s3d_mesh_topology_keep_run on this workspace", what);
    return 0;
}

extern "C" size_t s3d_mesh_topology_workspace_bytes(long n_vertices, long n_faces, int weld) {
    if (!tp_sizes_ok(n_vertices, n_faces)) return 0;
    TopoWs w;
    return topo_layout(n_vertices, n_faces, weld ? 1 : 0, w, nullptr);
}

extern "C" int s3d_mesh_topology_run(const double* vertices, long n_vertices, const long long* faces, long n_faces, int weld,
                                     void* workspace, size_t workspace_bytes, long* n_components, int* n_rounds,
                                     long long* summary_host, void* stream) {
    const char* what = "mesh_topology_run";
    hipStream_t st = (hipStream_t)stream;
    TopoWs w;
    weld = weld ? 1 : 0;
    S3D_CHECK_ARG(n_components && n_rounds, "%s: null output count", what);
    TRY_RET(topo_check(n_vertices, n_faces, weld, workspace, workspace_bytes, w, what));
    S3D_CHECK_ARG(n_faces == 0 || (vertices && faces), "%s: null mesh", what);
    *n_components = 0;
    *n_rounds = 0;
    if (summary_host)
        for (int i = 0; i < TP_NI; ++i) summary_host[i] = 0;
    const long nv = n_vertices, nf = n_faces, n3 = 3 * n_faces;
    S3D_HIP_TRY(what, hipMemsetAsync(w.hdr, 0, TP_HDR * 8, st));   // no completed run until the last launch says so
    S3D_HIP_TRY(what, hipMemsetAsync(w.flags, 0, 16 * 4, st));
    S3D_HIP_TRY(what, hipMemsetAsync(w.sumI, 0, TP_NI * 8, st));
    S3D_HIP_TRY(what, hipMemsetAsync(w.sumD, 0, TP_ND * 8, st));
    if (nv > 0) {
        S3D_HIP_TRY(what, hipMemsetAsync(w.ref, 0, (size_t)nv * 4, st));
        ME_LAUNCH(tp_iota_kernel, nv, st, w.vmap, nv);
        ME_LAUNCH(tp_iota_kernel, nv, st, w.L, nv);
        S3D_LAUNCH_CHECK();
    }
    if (nf == 0) {
        hipLaunchKernelGGL(tp_run_header_kernel, dim3(1), dim3(1), 0, st, w.hdr, 0LL, (long long)nv, 0LL, (long long)weld);
        S3D_LAUNCH_CHECK();
        return 0;
    }
    S3D_CHECK_ARG(nv >= 1, "%s: faces without vertices", what);

    // the indices are checked before anything dereferences them
    ME_LAUNCH(tp_validate_kernel, n3, st, faces, n3, nv, w.ref, w.flags);
    if (weld) ME_LAUNCH(tp_finite_kernel, nv, st, vertices, w.ref, nv, w.flags);
    S3D_LAUNCH_CHECK();
    int flags[2] = {0, 0};
    S3D_HIP_TRY(what, hipMemcpyAsync(flags, w.flags, 8, hipMemcpyDeviceToHost, st));
    S3D_HIP_TRY(what, hipStreamSynchronize(st));
    S3D_CHECK_ARG(!flags[0], "%s: a face indexes a vertex outside [0, %ld)", what, n_vertices);
    S3D_CHECK_ARG(!flags[1], "%s: a vertex that a face references has a coordinate that is not finite (weld)", what);

    if (weld) {
        S3D_HIP_TRY(what, hipMemsetAsync(w.table, 0xFF, (size_t)w.hsize * 4, st));
        ME_LAUNCH(tp_weld_insert_kernel, nv, st, vertices, w.ref, nv, w.table, w.hsize, w.vmap);
        ME_LAUNCH(tp_weld_read_kernel, nv, st, w.ref, nv, w.table, w.vmap);
    }
    S3D_HIP_TRY(what, hipMemsetAsync(w.refw, 0, (size_t)(nv + 1) * 4, st));
    ME_LAUNCH(tp_import_kernel, n3, st, faces, n3, w.vmap, w.W, w.refw);
    S3D_LAUNCH_CHECK();

    // components: hook, compress, check in launches of their own; the host reads the verdict once per round
    int rounds = 0;
    for (bool done = false; !done;) {
        if (rounds == TP_MAX_ROUNDS) {
            s3d_set_error("%s: the component labels have not converged after %d rounds", what, TP_MAX_ROUNDS);
            return S3D_E_ROUNDS;
        }
        ++rounds;
        S3D_HIP_TRY(what, hipMemsetAsync(w.flags + 2, 0, 4, st));
        ME_LAUNCH(tp_hook_kernel, nf, st, w.W, nf, w.L);
        ME_LAUNCH(tp_compress_kernel, nv, st, w.L, w.refw, nv);
        ME_LAUNCH(tp_check_kernel, nf, st, w.W, nf, w.L, w.flags);
        S3D_LAUNCH_CHECK();
        int open = 0;
        S3D_HIP_TRY(what, hipMemcpyAsync(&open, w.flags + 2, 4, hipMemcpyDeviceToHost, st));
        S3D_HIP_TRY(what, hipStreamSynchronize(st));
        done = !open;
    }
    // ids in ascending order of the roots, which are the components' smallest welded vertices
    ME_LAUNCH(tp_roots_kernel, nv + 1, st, w.L, w.refw, nv, w.vcnt);
    me_scan<int, int, false>(w.vcnt, w.cid, nv + 1, w.tsum, st);
    ME_LAUNCH(tp_face_component_kernel, nf, st, w.W, nf, w.L, w.cid, w.fcomp);
    S3D_LAUNCH_CHECK();
    int K = 0;
    S3D_HIP_TRY(what, hipMemcpyAsync(&K, w.cid + nv, 4, hipMemcpyDeviceToHost, st));
    S3D_HIP_TRY(what, hipStreamSynchronize(st));

    // vertex -> half-edge lists, half-edge status
    S3D_HIP_TRY(what, hipMemsetAsync(w.vcnt, 0, (size_t)(nv + 1) * 4, st));
    ME_LAUNCH(tp_vcount_kernel, n3, st, w.W, n3, w.vcnt);
    me_scan<int, int, false>(w.vcnt, w.voff, nv + 1, w.tsum, st);
    S3D_HIP_TRY(what, hipMemsetAsync(w.vcnt, 0, (size_t)(nv + 1) * 4, st));
    S3D_HIP_TRY(what, hipMemsetAsync(w.vown, 0x7F, (size_t)nv * 4, st));
    ME_LAUNCH(tp_vfill_kernel, n3, st, w.W, n3, w.voff, w.vcnt, w.adj, w.vown);
    ME_LAUNCH(tp_edges_kernel, n3, st, w.W, n3, w.voff, w.adj, w.vown, w.stat);
    S3D_LAUNCH_CHECK();

    // faces in component order (stable), then the runs' partial rows; the summary's runs are the chunks of the face list
    int *cur = w.ordA, *other = w.ordB;
    ME_LAUNCH(tp_iota_kernel, nf, st, cur, nf);
    for (int bit = 0; bit < 31 && ((long)K - 1) >> bit; ++bit) {
        ME_LAUNCH(tp_bit_kernel, nf, st, cur, w.fcomp, nf, bit, w.z);
        me_scan<int, int, false>(w.z, w.zoff, nf, w.tsum, st);
        ME_LAUNCH(tp_split_kernel, nf, st, cur, w.z, w.zoff, me_scan_total(w.tsum, nf), nf, other);
        std::swap(cur, other);
    }
    if (cur != w.ordA) S3D_HIP_TRY(what, hipMemcpyAsync(w.ordA, cur, (size_t)nf * 4, hipMemcpyDeviceToDevice, st));
    ME_LAUNCH(tp_partial_kernel, nf, st, w.ordA, w.fcomp, nf, w.W, w.stat, vertices, 0, w.partI, w.partD, w.seg);
    ME_LAUNCH(tp_partial_kernel, nf, st, (const int*)nullptr, (const int*)nullptr, nf, w.W, w.stat, vertices, 1, w.spartI,
              w.spartD, (int*)nullptr);
    ME_LAUNCH(tp_rows_kernel, 1, st, (const int*)nullptr, 1L, nf, 1, w.spartI, w.spartD, w.sumI, w.sumD);
    hipLaunchKernelGGL(tp_run_header_kernel, dim3(1), dim3(1), 0, st, w.hdr, (long long)K, (long long)nv, (long long)nf,
                       (long long)weld);
    S3D_LAUNCH_CHECK();
    if (summary_host) S3D_HIP_TRY(what, hipMemcpyAsync(summary_host, w.sumI, TP_NI * 8, hipMemcpyDeviceToHost, st));
    S3D_HIP_TRY(what, hipStreamSynchronize(st));
    *n_components = K;
    *n_rounds = rounds;
    return 0;
}

extern "C" int s3d_mesh_topology_emit_labels(const void* workspace, size_t workspace_bytes, long n_vertices, long n_faces,
                                             int weld, long long* vmap, long long* face_component,
                                             long long* vertex_component, void* stream) {
    const char* what = "mesh_topology_emit_labels";
    hipStream_t st = (hipStream_t)stream;
    TopoWs w;
    TRY_RET(topo_check(n_vertices, n_faces, weld ? 1 : 0, workspace, workspace_bytes, w, what));
    TRY_RET(topo_state(w, weld ? 1 : 0, -1, false, what, st));
    if (n_faces > 0 && face_component) ME_LAUNCH(tp_emit_face_labels_kernel, n_faces, st, w.fcomp, n_faces, face_component);
    if (n_vertices > 0 && (vmap || vertex_component))
        ME_LAUNCH(tp_emit_vertex_labels_kernel, n_vertices, st, w.ref, w.vmap, w.L, w.cid, n_vertices, vmap, vertex_component);
    S3D_LAUNCH_CHECK();
    return 0;
}

extern "C" int s3d_mesh_topology_emit_table(const void* workspace, size_t workspace_bytes, long n_vertices, long n_faces,
                                            int weld, long n_components, long long* counts, double* measures, void* stream) {
    const char* what = "mesh_topology_emit_table";
    hipStream_t st = (hipStream_t)stream;
    TopoWs w;
    TRY_RET(topo_check(n_vertices, n_faces, weld ? 1 : 0, workspace, workspace_bytes, w, what));
    S3D_CHECK_ARG(counts && measures, "%s: null output", what);
    S3D_CHECK_ARG(n_components >= 0, "%s: %ld components", what, n_components);
    TRY_RET(topo_state(w, weld ? 1 : 0, n_components, false, what, st));
    if (n_components > 0)
        ME_LAUNCH(tp_rows_kernel, n_components, st, w.seg, n_components, n_faces, 0, w.partI, w.partD, counts, measures);
    S3D_LAUNCH_CHECK();
    S3D_HIP_TRY(what, hipMemcpyAsync(counts + TP_NI * n_components, w.sumI, TP_NI * 8, hipMemcpyDeviceToDevice, st));
    S3D_HIP_TRY(what, hipMemcpyAsync(measures + TP_ND * n_components, w.sumD, TP_ND * 8, hipMemcpyDeviceToDevice, st));
    return 0;
}

extern "C" int s3d_mesh_topology_keep_run(void* workspace, size_t workspace_bytes, long n_vertices, long n_faces, int weld,
                                          long n_components, const unsigned char* keep, int drop_degenerate,
                                          long* n_vertices_out, long* n_faces_out, void* stream) {
    const char* what = "mesh_topology_keep_run";
    hipStream_t st = (hipStream_t)stream;
    TopoWs w;
    TRY_RET(topo_check(n_vertices, n_faces, weld ? 1 : 0, workspace, workspace_bytes, w, what));
    S3D_CHECK_ARG(n_vertices_out && n_faces_out, "%s: null output count", what);
    S3D_CHECK_ARG(n_components >= 0, "%s: %ld components", what, n_components);
    *n_vertices_out = *n_faces_out = 0;
    TRY_RET(topo_state(w, weld ? 1 : 0, n_components, false, what, st));
    S3D_HIP_TRY(what, hipMemsetAsync(w.hdr, 0, 16, st));
    S3D_HIP_TRY(what, hipMemsetAsync(w.hdr + 7, 0, 8, st));
    if (n_faces == 0 || n_components == 0) return 0;
    S3D_CHECK_ARG(keep != nullptr, "%s: null keep flags", what);
    const long nv = n_vertices, nf = n_faces;
    // kept -> z, its scan -> zoff; used -> vcnt, the new indices -> voff
    S3D_HIP_TRY(what, hipMemsetAsync(w.vcnt, 0, (size_t)(nv + 1) * 4, st));
    ME_LAUNCH(tp_keep_faces_kernel, nf, st, w.W, w.fcomp, nf, keep, drop_degenerate ? 1 : 0, w.z, w.vcnt);
    me_scan<int, int, false>(w.z, w.zoff, nf, w.tsum, st);
    // the face total leaves tsum before the vertex scan reuses it
    S3D_HIP_TRY(what, hipMemcpyAsync(w.flags + 4, me_scan_total(w.tsum, nf), 4, hipMemcpyDeviceToDevice, st));
    me_scan<int, int, false>(w.vcnt, w.voff, nv + 1, w.tsum, st);
    hipLaunchKernelGGL(tp_keep_header_kernel, dim3(1), dim3(1), 0, st, w.hdr, w.flags + 4, w.voff, nv);
    S3D_LAUNCH_CHECK();
    long long hdr[2] = {0, 0};
    S3D_HIP_TRY(what, hipMemcpyAsync(hdr, w.hdr, 16, hipMemcpyDeviceToHost, st));
    S3D_HIP_TRY(what, hipStreamSynchronize(st));
    *n_faces_out = (long)hdr[0];
    *n_vertices_out = (long)hdr[1];
    return 0;
}

extern "C" int s3d_mesh_topology_keep_emit(const void* workspace, size_t workspace_bytes, const double* vertices,
                                           long n_vertices, long n_faces, int weld, double* vertices_out,
                                           long long* faces_out, void* stream) {
    const char* what = "mesh_topology_keep_emit";
    hipStream_t st = (hipStream_t)stream;
    TopoWs w;
    TRY_RET(topo_check(n_vertices, n_faces, weld ? 1 : 0, workspace, workspace_bytes, w, what));
    S3D_CHECK_ARG(vertices && vertices_out && faces_out, "%s: null mesh or output", what);
    if (n_faces == 0 || n_vertices == 0) return 0;
    TRY_RET(topo_state(w, weld ? 1 : 0, -1, true, what, st));
    ME_LAUNCH(me_emit_vertices_kernel, n_vertices, st, vertices, w.vcnt, w.voff, n_vertices, vertices_out);
    ME_LAUNCH(tp_keep_emit_faces_kernel, n_faces, st, w.W, w.z, w.zoff, w.voff, n_faces, faces_out);
    S3D_LAUNCH_CHECK();
    return 0;
}

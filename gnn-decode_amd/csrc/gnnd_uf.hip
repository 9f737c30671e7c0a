// gnnd_uf.hip — the union-find decoder of a matchable Tanner graph (gnnd_uf, include/gnnd.h): grow
// clusters around the defects by half-edges, merge them, peel a spanning forest.  Integers only;
// every output is bit-reproducible and equal to the host mirror's (gnnd_uf_host.h).
#include "gnnd_common.h"
#include "gnnd_wave_tile.h"
#include "gnnd_uf_host.h"

// this translation unit's debug word: gnnd_debug_take_uf() (tests/uf_debug_worker.py reads it next
// to gnnd_debug_flags)
GNND_DEBUG_TU(uf)

// ---------------------------------------------------------------------------------------
// The wave-private-tile plan of gnnd_wave_tile.h.  A wave's tile, all int32:
//   grow[V]     half-edges grown on edge v: 0, 1, 2 (full)
//   label[N]    the cluster of vertex u = the highest vertex index in it
//   par[N]      defect[u]; during the peel the XOR of the defects over u's subtree
//   aux[N]      odd[l] while the clusters grow, then depth[u]
//   parent[N]   the parent edge of u; V = none (a root)
// Lanes stride over edges (the growth step, the sweeps, the outputs) and over vertices (the set-up,
// the cluster parities, the peel's levels).  Every write that another lane may also make is an LDS
// atomic whose result does not depend on the order: xor for the parities, max for the labels, min
// for the depths and the parent edges.  The sweeps repeat until a wave-wide vote finds no lane that
// saw an edge out of its fixed point.  All loop exits are wave-uniform.
// Why no index leaves its array: label[u] starts as u and is only ever replaced by another
// vertex's label, so it is a vertex index; aux as depth is 0 at a root and otherwise one more than
// a neighbour's, below N, or kGnndUfInf, and is only compared, never used as an index; parent[u]
// is V or the index of an edge the parent pass itself visited, and is dereferenced only where
// depth[u] >= 1, which the pass that set the depth guarantees a full edge for (the release build
// clamps nothing; the debug build checks every one of these).  The endpoint and virtual-vertex
// tables come from the host builder, which the CPU tests check.
// ---------------------------------------------------------------------------------------
struct UfPlan {
    int off_label, off_par, off_aux, off_parent;    // byte offsets inside one wave's tile (grow at 0)
    int wave_bytes;                                 // one wave's tile (16-byte multiple)
    int waves;                                      // waves per workgroup (0: the tile does not fit)
};

static UfPlan uf_plan(int V, int N) {
    UfPlan p;
    const size_t edge = wave_tile_align16((size_t)V * sizeof(int32_t));
    const size_t node = wave_tile_align16((size_t)N * sizeof(int32_t));
    const size_t bytes = edge + 4 * node;           // V <= 65535, N <= 131070: far below overflow
    p.off_label = (int)edge;
    p.off_par = (int)(edge + node);
    p.off_aux = (int)(edge + 2 * node);
    p.off_parent = (int)(edge + 3 * node);
    p.wave_bytes = (int)bytes;
    p.waves = wave_tile_waves(bytes);
    return p;
}

struct UfArgs {
    int V, C, N;
    const int* ends;            // [2 V] a_v < b_v
    const int* cvirt;           // [C] the virtual vertex of check c's component, -1: none
    const int32_t* gate;
    int32_t* rounds;
    int32_t* status;
    int32_t* nfull;
};

template <typename T>
__global__ void __launch_bounds__(256)
uf_kernel(UfPlan pl, UfArgs ua, const T* __restrict__ x, T* __restrict__ ehat, int64_t B) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int V = ua.V, C = ua.C, N = ua.N;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    char* tile = smem + (size_t)wave * pl.wave_bytes;
    int* s_grow = (int*)tile;
    int* s_label = (int*)(tile + pl.off_label);
    int* s_par = (int*)(tile + pl.off_par);
    int* s_aux = (int*)(tile + pl.off_aux);
    int* s_parent = (int*)(tile + pl.off_parent);
    const int* __restrict__ ends = ua.ends;

    for (int64_t b = (int64_t)blockIdx.x * pl.waves + wave; b < B;
         b += (int64_t)gridDim.x * pl.waves) {
        if (ua.gate && ua.gate[b] == 0) continue;           // wave-uniform: nothing of b is written
        const T* xc = x + b * (int64_t)(V + C) + V;
        // ---- label[u] = u, defect[u] = t_u, grow = 0 ----
        for (int u = lane; u < N; u += 64) {
            s_label[u] = u;
            s_par[u] = u < C ? (int)(xc[u] < T(0)) : 0;
        }
        for (int v = lane; v < V; v += 64) s_grow[v] = 0;
        wave_tile_sync();
        // ---- a virtual vertex's defect: the XOR of t over its component's checks ----
        for (int c = lane; c < C; c += 64) {
            const int vv = ua.cvirt[c];
            if (vv >= 0 && s_par[c]) atomicXor(&s_par[GNND_DIDX(vv, N, GNND_DBG_NODE)], 1);
        }
        wave_tile_sync();
        int rounds = 0, status = 0;
        for (;;) {
            // ---- odd[l] = XOR of defect[u] over label[u] == l ----
            for (int u = lane; u < N; u += 64) s_aux[u] = 0;
            wave_tile_sync();
            for (int u = lane; u < N; u += 64)
                if (s_par[u]) atomicXor(&s_aux[GNND_DIDX(s_label[u], N, GNND_DBG_NODE)], 1);
            wave_tile_sync();
            int any = 0;
            for (int u = lane; u < N; u += 64) any |= s_aux[u];
            if (__ballot(any) == 0) break;
            // ---- one half-edge from each end that lies in an odd cluster ----
            int grew = 0;
            for (int v = lane; v < V; v += 64) {
                const int a = GNND_DIDX(ends[2 * v], N, GNND_DBG_NODE);
                const int bb = GNND_DIDX(ends[2 * v + 1], N, GNND_DBG_NODE);
                const int g0 = s_grow[v];
                const int g = g0 + s_aux[GNND_DIDX(s_label[a], N, GNND_DBG_NODE)] +
                              s_aux[GNND_DIDX(s_label[bb], N, GNND_DBG_NODE)];
                const int ng = g < 2 ? g : 2;
                grew |= ng != g0;
                s_grow[v] = ng;
            }
            // an odd cluster with no edge left to grow is a whole component: no e satisfies t
            if (__ballot(grew) == 0) { status = 1; break; }
            ++rounds;
            wave_tile_sync();
            // ---- labels: the fixed point of label <- max over the full edges ----
            for (;;) {
                int changed = 0;
                for (int v = lane; v < V; v += 64) {
                    if (s_grow[v] != 2) continue;
                    const int a = GNND_DIDX(ends[2 * v], N, GNND_DBG_NODE);
                    const int bb = GNND_DIDX(ends[2 * v + 1], N, GNND_DBG_NODE);
                    const int la = s_label[a], lb = s_label[bb];
                    if (la == lb) continue;
                    atomicMax(la < lb ? &s_label[a] : &s_label[bb], la < lb ? lb : la);
                    changed = 1;
                }
                wave_tile_sync();
                if (__ballot(changed) == 0) break;
            }
        }
        // ---- forest: depth[u] = BFS distance from the label vertex over the full edges ----
        wave_tile_sync();                                     // the odd[] reads are done
        for (int u = lane; u < N; u += 64) {
            s_aux[u] = s_label[u] == u ? 0 : kGnndUfInf;
            s_parent[u] = V;
        }
        wave_tile_sync();
        for (;;) {
            int changed = 0;
            for (int v = lane; v < V; v += 64) {
                if (s_grow[v] != 2) continue;
                const int a = GNND_DIDX(ends[2 * v], N, GNND_DBG_NODE);
                const int bb = GNND_DIDX(ends[2 * v + 1], N, GNND_DBG_NODE);
                const int da = s_aux[a], db = s_aux[bb];
                if (da + 1 < db) { atomicMin(&s_aux[bb], da + 1); changed = 1; }
                if (db + 1 < da) { atomicMin(&s_aux[a], db + 1); changed = 1; }
            }
            wave_tile_sync();
            if (__ballot(changed) == 0) break;
        }
        // ---- parent edge: the lowest full edge to a vertex one level up; nfull; the deepest level ----
        int nfull = 0, maxd = 0;
        for (int v = lane; v < V; v += 64) {
            if (s_grow[v] != 2) continue;
            ++nfull;
            const int a = GNND_DIDX(ends[2 * v], N, GNND_DBG_NODE);
            const int bb = GNND_DIDX(ends[2 * v + 1], N, GNND_DBG_NODE);
            const int da = s_aux[a], db = s_aux[bb];
            if (da + 1 == db) atomicMin(&s_parent[bb], v);
            if (db + 1 == da) atomicMin(&s_parent[a], v);
        }
        for (int u = lane; u < N; u += 64) {
            const int d = s_aux[u];
            GNND_DCHECK(d < N, GNND_DBG_GRID);              // every vertex was reached from its root
            maxd = d > maxd ? d : maxd;
        }
        for (int s = 32; s >= 1; s >>= 1) {
            nfull += __shfl_xor(nfull, s);
            const int o = __shfl_xor(maxd, s);
            maxd = o > maxd ? o : maxd;
        }
        maxd = maxd < N ? maxd : N - 1;                     // a depth is below N: bounds the loop
        wave_tile_sync();
        // ---- peel: subtree parities, the deepest level first ----
        for (int d = maxd; d >= 1; --d) {
            for (int u = lane; u < N; u += 64) {
                if (s_aux[u] != d || !s_par[u]) continue;
                const int e = GNND_DIDX(s_parent[u], V, GNND_DBG_SLOT);
                const int a = ends[2 * e], bb = ends[2 * e + 1];
                atomicXor(&s_par[GNND_DIDX(a == u ? bb : a, N, GNND_DBG_NODE)], 1);
            }
            wave_tile_sync();
        }
        // ---- outputs: edge v is set where it is the parent edge of an end with an odd subtree ----
        for (int v = lane; v < V; v += 64) {
            int h = 0;
            if (s_grow[v] == 2) {
                const int a = GNND_DIDX(ends[2 * v], N, GNND_DBG_NODE);
                const int bb = GNND_DIDX(ends[2 * v + 1], N, GNND_DBG_NODE);
                h = s_parent[a] == v ? s_par[a] : s_parent[bb] == v ? s_par[bb] : 0;
            }
            ehat[b * V + v] = h ? T(1) : T(0);
        }
        if (lane == 0) {
            if (ua.rounds) ua.rounds[b] = rounds;
            if (ua.status) ua.status[b] = status;
            if (ua.nfull) ua.nfull[b] = nfull;
        }
        wave_tile_sync();                     // tile reads done before the next codeword's writes
    }
}

template <typename T>
static int launch_uf(const UfPlan& pl, const UfArgs& ua, const void* x, void* ehat, int64_t B,
                     hipStream_t st) {
    uf_kernel<T><<<wave_tile_blocks(B, pl.waves, pl.waves), 64 * pl.waves, (size_t)pl.waves * pl.wave_bytes, st>>>(
        pl, ua, (const T*)x, (T*)ehat, B);
    GNND_LAUNCH_CHECK();
    return GNND_OK;
}

extern "C" int gnnd_uf(const gnnd_graph* g, int dtype, const void* d_x, const int32_t* d_gate,
                       void* d_ehat, int32_t* d_rounds, int32_t* d_status, int32_t* d_nfull,
                       int64_t batch, void* stream) {
    const int rc = gnnd_args_rc(g && batch >= 0, dtype);
    if (rc != GNND_OK) return rc;
    if (batch == 0) return GNND_OK;
    if (!d_x || !d_ehat) return GNND_ERR_INVALID_ARG;
    if (g->uf_nvert == 0) return GNND_ERR_UNSUPPORTED;      // not matchable
    const int V = g->view.V, C = g->view.C;
    const UfPlan pl = uf_plan(V, g->uf_nvert);
    if (pl.waves == 0) return GNND_ERR_UNSUPPORTED;
    const UfArgs ua = {V, C, g->uf_nvert, g->uf_dev, g->uf_dev + 2 * V, d_gate,
                       d_rounds, d_status, d_nfull};
    return gnnd_by_dtype(dtype, [&](auto z) {
        return launch_uf<decltype(z)>(pl, ua, d_x, d_ehat, batch, (hipStream_t)stream);
    });
}

extern "C" int gnnd_uf_host(const int64_t* h_var, const int64_t* h_chk, int64_t num_edges,
                            int32_t num_var, int32_t num_chk, int dtype, const void* h_x,
                            const int32_t* h_gate, void* h_ehat, int32_t* h_rounds,
                            int32_t* h_status, int32_t* h_nfull, int64_t batch) {
    return gnnd_uf_host_checked(h_var, h_chk, num_edges, num_var, num_chk, dtype, h_x, h_gate,
                                h_ehat, h_rounds, h_status, h_nfull, batch);
}

// gnnd_uf.hip — the union-find decoder of a matchable Tanner graph (gnnd_uf, include/gnnd.h): grow
// clusters around the defects by half-edges, merge them, peel a spanning forest.  Integers only;
// every output is bit-reproducible and equal to the host mirror's (gnnd_uf_host.h).
#include "gnnd_common.h"
#include "gnnd_wave_tile.h"
#include "gnnd_uf_host.h"
#include "gnnd_uf_tile.h"

GNND_DEBUG_TU(uf)

// ---------------------------------------------------------------------------------------
// The wave-private-tile plan of gnnd_wave_tile.h; the tile, the steps this kernel shares with
// gnnd_ufw.hip and the reasons no index leaves its array are in gnnd_uf_tile.h.  The edge array
// holds grow[V], the half-edges grown on edge v: 0, 1, 2 (full).
// ---------------------------------------------------------------------------------------

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
    const UfTile t = uf_tile(smem, pl, wave);
    int* s_grow = t.edge;
    const int* __restrict__ ends = ua.ends;
    const auto full = [](int g) { return g == 2; };

    for (int64_t b = (int64_t)blockIdx.x * pl.waves + wave; b < B;
         b += (int64_t)gridDim.x * pl.waves) {
        if (ua.gate && ua.gate[b] == 0) continue;           // wave-uniform: nothing of b is written
        // ---- grow = 0, label[u] = u, defect[u] = t_u ----
        for (int v = lane; v < V; v += 64) s_grow[v] = 0;
        uf_defects(t, ua.cvirt, x + b * (int64_t)(V + C) + V, C, N, lane);
        int rounds = 0, status = 0;
        while (uf_cluster_parities(t, N, lane)) {
            // ---- one half-edge from each end that lies in an odd cluster ----
            int grew = 0;
            for (int v = lane; v < V; v += 64) {
                const int a = GNND_DIDX(ends[2 * v], N, GNND_DBG_NODE);
                const int bb = GNND_DIDX(ends[2 * v + 1], N, GNND_DBG_NODE);
                const int g0 = s_grow[v];
                const int g = g0 + t.aux[GNND_DIDX(t.label[a], N, GNND_DBG_NODE)] +
                              t.aux[GNND_DIDX(t.label[bb], N, GNND_DBG_NODE)];
                const int ng = g < 2 ? g : 2;
                grew |= ng != g0;
                s_grow[v] = ng;
            }
            // an odd cluster with no edge left to grow is a whole component: no e satisfies t
            if (__ballot(grew) == 0) { status = 1; break; }
            ++rounds;
            wave_tile_sync();
            uf_merge_labels(t, ends, V, N, lane, full);
        }
        const int nfull = uf_forest_peel(t, ends, V, N, lane, full, ehat + b * V);
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

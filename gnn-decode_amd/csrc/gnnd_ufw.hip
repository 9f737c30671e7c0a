// gnnd_ufw.hip — weighted union-find (gnnd_ufw, include/gnnd.h): gnnd_uf with an edge's length its
// quantised reliability, so clusters grow fast through bits believed flipped and slowly through
// reliable ones.  One multiply and two compares in T per edge; everything after them is integers,
// and every output is bit-reproducible and equal to the host mirror's (gnnd_ufw_host.h).
#include "gnnd_common.h"
#include "gnnd_wave_tile.h"
#include "gnnd_ufw_host.h"
#include "gnnd_uf_tile.h"

GNND_DEBUG_TU(ufw)

// ---------------------------------------------------------------------------------------
// The wave-private-tile plan of gnnd_wave_tile.h with the tile and the shared steps of
// gnnd_uf_tile.h: the same (V + 4 N) int32, the same limits as gnnd_uf.  The edge array holds
// rem[V], the half-units of edge v still to grow: 2 w_v at the start, 0 when full.  A growth event
// is two walks over the edges: the lanes' min of ceil(rem / rate) over their active edges, reduced
// over the wave (so the jump d is wave-uniform), then rem <- max(0, rem - rate d).  Between two
// events no edge fills, so the labels and the parities a walk reads are the ones the event began
// with.  Every event fills at least one edge: at most V events.
// ---------------------------------------------------------------------------------------
constexpr int kUfwNoEdge = 0x7fffffff;      // the min over no active edge

// the device statement of gnnd_ufw_weight (gnnd_ufw_host.h): one multiply in T, a NaN compares false
template <typename T>
__device__ __forceinline__ int ufw_weight(T r, T s, int wmax) {
    const T m = r * s;
    if (m >= (T)(wmax - 1)) return wmax;
    return m > T(0) ? 1 + (int)m : 1;
}

struct UfwArgs {
    int V, C, N;
    const int* ends;            // [2 V] a_v < b_v
    const int* cvirt;           // [C] the virtual vertex of check c's component, -1: none
    const int32_t* gate;
    int passthrough;
    int wmax;
    int32_t* rounds;
    int32_t* status;
    int32_t* nfull;
    int32_t* events;
};

template <typename T>
__global__ void __launch_bounds__(256)
ufw_kernel(UfPlan pl, UfwArgs ua, T scale, const T* __restrict__ x, const T* __restrict__ llr,
           T* __restrict__ ehat, int64_t B) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int V = ua.V, C = ua.C, N = ua.N;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const UfTile t = uf_tile(smem, pl, wave);
    int* s_rem = t.edge;
    const int* __restrict__ ends = ua.ends;
    const auto full = [](int rem) { return rem == 0; };

    for (int64_t b = (int64_t)blockIdx.x * pl.waves + wave; b < B;
         b += (int64_t)gridDim.x * pl.waves) {
        int rounds = 0, status = 0, events = 0, nfull = 0;
        if (ua.gate && ua.gate[b] == 0) {                   // wave-uniform
            if (!ua.passthrough) continue;                  // nothing of b is written
            // pass-through: the hard decision of llr (false for -0.0 and a NaN), zero counters
            for (int v = lane; v < V; v += 64)
                ehat[b * V + v] = llr[b * V + v] < T(0) ? T(1) : T(0);
        } else {
            // ---- rem = 2 w_v, label[u] = u, defect[u] = t_u ----
            const T* xv = x + b * (int64_t)(V + C);
            const T* r = llr ? llr + b * (int64_t)V : xv;
            for (int v = lane; v < V; v += 64) s_rem[v] = 2 * ufw_weight(r[v], scale, ua.wmax);
            uf_defects(t, ua.cvirt, xv + V, C, N, lane);
            while (uf_cluster_parities(t, N, lane)) {
                // ---- d = the steps until the first active edge fills ----
                int d = kUfwNoEdge;
                for (int v = lane; v < V; v += 64) {
                    const int rem = s_rem[v];
                    if (rem == 0) continue;
                    const int a = GNND_DIDX(ends[2 * v], N, GNND_DBG_NODE);
                    const int bb = GNND_DIDX(ends[2 * v + 1], N, GNND_DBG_NODE);
                    const int rate = t.aux[GNND_DIDX(t.label[a], N, GNND_DBG_NODE)] +
                                     t.aux[GNND_DIDX(t.label[bb], N, GNND_DBG_NODE)];
                    if (rate == 0) continue;
                    const int need = rate == 2 ? (rem + 1) >> 1 : rem;
                    d = need < d ? need : d;
                }
                for (int s = 32; s >= 1; s >>= 1) {
                    const int o = __shfl_xor(d, s);
                    d = o < d ? o : d;
                }
                // an odd cluster with no edge left to grow is a whole component: no e satisfies t
                if (d == kUfwNoEdge) { status = 1; break; }
                // ---- every edge grows rate d half-units, all from the same labels ----
                for (int v = lane; v < V; v += 64) {
                    const int rem = s_rem[v];
                    if (rem == 0) continue;
                    const int a = GNND_DIDX(ends[2 * v], N, GNND_DBG_NODE);
                    const int bb = GNND_DIDX(ends[2 * v + 1], N, GNND_DBG_NODE);
                    const int rate = t.aux[GNND_DIDX(t.label[a], N, GNND_DBG_NODE)] +
                                     t.aux[GNND_DIDX(t.label[bb], N, GNND_DBG_NODE)];
                    const int left = rem - rate * d;        // d <= 2 wmax, rate <= 2: no overflow
                    s_rem[v] = left > 0 ? left : 0;
                }
                rounds += d;
                ++events;
                wave_tile_sync();
                uf_merge_labels(t, ends, V, N, lane, full);
            }
            nfull = uf_forest_peel(t, ends, V, N, lane, full, ehat + b * V);
            wave_tile_sync();                 // tile reads done before the next codeword's writes
        }
        if (lane == 0) {
            if (ua.rounds) ua.rounds[b] = rounds;
            if (ua.status) ua.status[b] = status;
            if (ua.nfull) ua.nfull[b] = nfull;
            if (ua.events) ua.events[b] = events;
        }
    }
}

template <typename T>
static int launch_ufw(const UfPlan& pl, const UfwArgs& ua, double scale, const void* x,
                      const void* llr, void* ehat, int64_t B, hipStream_t st) {
    ufw_kernel<T><<<wave_tile_blocks(B, pl.waves, pl.waves), 64 * pl.waves, (size_t)pl.waves * pl.wave_bytes, st>>>(
        pl, ua, (T)scale, (const T*)x, (const T*)llr, (T*)ehat, B);
    GNND_LAUNCH_CHECK();
    return GNND_OK;
}

// the graph-side refusals of gnnd_uf and gnnd_ufw (gnnd_belief_find decides them before its first
// launch): matchable, and the tile fits
bool gnnd_uf_fits(const gnnd_graph* g) {
    return g->uf_nvert != 0 && uf_plan(g->view.V, g->uf_nvert).waves != 0;
}

extern "C" int gnnd_ufw(const gnnd_graph* g, int dtype, const void* d_x, const void* d_llr,
                        double scale, int32_t wmax, const int32_t* d_gate, int32_t passthrough,
                        void* d_ehat, int32_t* d_rounds, int32_t* d_status, int32_t* d_nfull,
                        int32_t* d_events, int64_t batch, void* stream) {
    const int rc = gnnd_args_rc(g && batch >= 0 && gnnd_ufw_params_ok(scale, wmax, passthrough) &&
                                    (passthrough == 0 || (d_gate && d_llr)),
                                dtype);
    if (rc != GNND_OK) return rc;
    if (batch == 0) return GNND_OK;
    if (!d_x || !d_ehat) return GNND_ERR_INVALID_ARG;
    if (!gnnd_uf_fits(g)) return GNND_ERR_UNSUPPORTED;      // not matchable, or the tile over 64 KiB
    const int V = g->view.V, C = g->view.C;
    const UfPlan pl = uf_plan(V, g->uf_nvert);
    const UfwArgs ua = {V, C, g->uf_nvert, g->uf_dev, g->uf_dev + 2 * V, d_gate, passthrough, wmax,
                        d_rounds, d_status, d_nfull, d_events};
    return gnnd_by_dtype(dtype, [&](auto z) {
        return launch_ufw<decltype(z)>(pl, ua, scale, d_x, d_llr, d_ehat, batch,
                                       (hipStream_t)stream);
    });
}

extern "C" int gnnd_ufw_host(const int64_t* h_var, const int64_t* h_chk, int64_t num_edges,
                             int32_t num_var, int32_t num_chk, int dtype, const void* h_x,
                             const void* h_llr, double scale, int32_t wmax, const int32_t* h_gate,
                             int32_t passthrough, void* h_ehat, int32_t* h_rounds,
                             int32_t* h_status, int32_t* h_nfull, int32_t* h_events,
                             int64_t batch) {
    return gnnd_ufw_host_checked(h_var, h_chk, num_edges, num_var, num_chk, dtype, h_x, h_llr,
                                 scale, wmax, h_gate, passthrough, h_ehat, h_rounds, h_status,
                                 h_nfull, h_events, batch);
}

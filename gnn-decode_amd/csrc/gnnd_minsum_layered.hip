// gnnd_minsum_layered.hip — min-sum BP on the layered (check-sequential) schedule
// (gnnd_minsum_layered, include/gnnd.h) and the one-call BP+OSD decoder on top of it
// (gnnd_bposd_layered): the checks are visited layer by layer, every check seeing the posteriors
// the layers before it just updated; bit-reproducible in fp32 and fp64.  Built with
// -ffp-contract=off (Makefile XFLAGS_gnnd_minsum_layered): a * m - b is two roundings, on the
// device and in the host mirror alike.
#include "gnnd_common.h"
#include "gnnd_wave_tile.h"
#include "gnnd_minsum_layered_host.h"

GNND_DEBUG_TU(minsum_layered)

// ---------------------------------------------------------------------------------------
// The sweep is serial over layers and parallel only inside one, so a codeword gets a sub-wave
// group of G lanes (a power of two covering the largest layer, 8 <= G <= 64) and a wave holds
// 64 / G codewords.  Wave-private LDS, no workgroup barrier, no atomics (the fence, the grid rule,
// the syndrome partial and the magnitude are gnnd_wave_tile.h's; the check walk is this unit's own,
// for its q = L_v - r_e).  A codeword's tile:
// r[E] (the check messages), L[V] (the posteriors), all T.  Per iteration, per layer:
//   each lane owns one check of the layer (slots lane, lane + G, ... where a layer is larger than
//   G): one walk over its edges gathers q = L_v - r_e and keeps min1, min2, arg-min and the sign
//   parity, a second walk repeats the subtraction (the variables of one check are distinct, so
//   L_v is still what the first walk read), and writes r' and L_v = q + r'.  The checks of a layer
//   share no variable and every edge belongs to one check: the lanes of a layer touch disjoint
//   tile elements, and any order among them gives the bits of the serial statement.
//   One wave-level fence separates the layers.
// Convergence: each lane XORs (L_v < 0) over the variables of checks lane, lane + G, ... against
// t_c; one __ballot, masked to the group's lanes.
// The groups of a wave finish at different iterations.  The wave's loop stays uniform: it runs
// until every group is done or `iters` is reached, finished groups (and the idle groups of the
// last wave, which neither read nor write) are predicated off with their L, it and ok frozen, and
// every fence and ballot sits outside the predicated regions.  No index depends on the data, so
// a NaN or an infinity in x stays inside its codeword even though its neighbours share the wave.
// ---------------------------------------------------------------------------------------
constexpr size_t kLayeredLdsPerCu = 160 * 1024;

struct LayeredPlan {
    int G, logG;              // lanes per codeword
    int off_L;                // byte offset of L[V] inside a codeword's tile (r at 0)
    int cw_bytes;             // one codeword's tile: an odd number of 16-byte units, so that the
                              // codewords of a wave start on different banks
    int waves;                // waves per workgroup (0: the tiles of one wave do not fit)
    int nlayers, max_layer;
};

static LayeredPlan layered_plan(const gnnd_graph* g, size_t elem) {
    LayeredPlan p;
    const size_t E = (size_t)g->view.E, V = (size_t)g->view.V;
    const size_t r_bytes = wave_tile_align16(E * elem);
    size_t bytes = r_bytes + wave_tile_align16(V * elem);       // E, V <= 65535: no overflow
    if (!((bytes >> 4) & 1)) bytes += 16;
    p.off_L = (int)r_bytes;
    p.cw_bytes = (int)bytes;
    p.nlayers = g->nlayers;
    p.max_layer = g->max_layer;
    int G = 8;
    while (G < 64 && G < g->max_layer) G *= 2;
    while (G < 64 && (size_t)(64 / G) * bytes > kWaveTileLdsLimit) G *= 2;   // fewer codewords per wave
    p.G = G;
    p.logG = 0;
    while ((1 << p.logG) < G) ++p.logG;
    p.waves = 0;
    const size_t wave_bytes = (size_t)(64 / G) * bytes;
    // the workgroup size that keeps most codewords resident on a CU (larger on ties)
    size_t best = 0;
    for (int w = 1; w <= 4; ++w) {
        if (w * wave_bytes > kWaveTileLdsLimit) break;
        const size_t resident = (kLayeredLdsPerCu / (w * wave_bytes)) * w;
        if (resident >= best) { best = resident; p.waves = w; }
    }
    return p;
}

template <typename T>
__global__ void __launch_bounds__(256)
minsum_layered_kernel(GraphView g, LayeredPlan pl, const int* __restrict__ layer_ptr,
                      const int* __restrict__ layer_chk, T a, T bt, int iters, int early_stop,
                      const T* __restrict__ x, T* __restrict__ out, T* __restrict__ llr,
                      int32_t* __restrict__ iters_out, int32_t* __restrict__ status, int64_t B) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int V = g.V, C = g.C, E = g.E, N = g.N;
    (void)C;                                        // read by the debug build's index checks only
    const int G = pl.G, K = 64 >> pl.logG;          // K codewords per wave
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int grp = lane >> pl.logG, gl = lane & (G - 1);
    const uint64_t gmask = (G == 64 ? ~0ull : ((1ull << G) - 1)) << (grp * G);
    char* tile = smem + (size_t)(wave * K + grp) * pl.cw_bytes;
    T* s_r = (T*)tile;
    T* s_L = (T*)(tile + pl.off_L);
    const int64_t per_wg = (int64_t)pl.waves * K;

    for (int64_t b0 = ((int64_t)blockIdx.x * pl.waves + wave) * K; b0 < B;
         b0 += (int64_t)gridDim.x * per_wg) {
        const int64_t b = b0 + grp;
        const bool active = b < B;                  // idle groups of the last wave: no access at all
        const T* xv = x + (active ? b : 0) * N;
        const T* xc = xv + V;
        // ---- L_v = l_v, r_e = +0 ----
        if (active) {
            for (int v = gl; v < V; v += G) s_L[v] = xv[v];
            for (int e = gl; e < E; e += G) s_r[e] = T(0);
        }
        wave_tile_sync();
        int it = 0;
        bool ok = false, done = !active;
        for (int step = 0; step < iters; ++step) {  // wave-uniform trip count
            if (!done) ++it;
            for (int k = 0; k < pl.nlayers; ++k) {
                const int l0 = layer_ptr[k], l1 = layer_ptr[k + 1];
                if (!done) {
                    for (int s = l0 + gl; s < l1; s += G) {
                        const int c = GNND_DIDX(layer_chk[GNND_DIDX(s, C, GNND_DBG_SLOT)], C,
                                                GNND_DBG_NODE);
                        const int i0 = g.chk_ptr[c], i1 = g.chk_ptr[c + 1];
                        T min1 = (T)INFINITY, min2 = (T)INFINITY;
                        int arg = -1;
                        int par = xc[c] < T(0);
                        for (int i = i0; i < i1; ++i) {
                            const int e = GNND_DIDX(g.chk_edge[GNND_DIDX(i, E, GNND_DBG_SLOT)], E, GNND_DBG_SLOT);
                            const int v = GNND_DIDX((int)(g.edge_vc[e] & 0xffffu), V, GNND_DBG_VAR);
                            const T q = s_L[v] - s_r[e];
                            const T aq = g_abs(q);
                            par ^= (int)(q < T(0));
                            if (aq < min1) { min2 = min1; min1 = aq; arg = e; }
                            else if (aq < min2) min2 = aq;
                        }
                        for (int i = i0; i < i1; ++i) {
                            const int e = GNND_DIDX(g.chk_edge[GNND_DIDX(i, E, GNND_DBG_SLOT)], E, GNND_DBG_SLOT);
                            const int v = GNND_DIDX((int)(g.edge_vc[e] & 0xffffu), V, GNND_DBG_VAR);
                            const T q = s_L[v] - s_r[e];
                            const T rn = bp_signed_mag(a, bt, e == arg ? min2 : min1,
                                                       par ^ (int)(q < T(0)));
                            s_L[v] = q + rn;
                            s_r[e] = rn;
                        }
                    }
                }
                wave_tile_sync();                // between layers, outside the predicate
            }
            // ---- H^T h == t ? (wanted where it can stop the loop, and after the last iteration) ----
            if (early_stop || step == iters - 1) {
                int bad = 0;
                if (!done) bad = bp_syndrome_bad(g, s_L, xc, gl, G);
                const uint64_t fails = __ballot(bad);       // every lane of the wave takes part
                if (!done) {
                    ok = (fails & gmask) == 0;
                    if (early_stop && ok) done = true;
                }
                wave_tile_sync();                // the L reads above before the next layer's writes
                if (__ballot(!done) == 0) break;    // wave-uniform: every group has stopped
            }
        }
        // ---- outputs (L of the group's last executed iteration) ----
        if (active) {
            for (int v = gl; v < V; v += G) {
                const T L = s_L[v];
                out[b * V + v] = T(1) / (T(1) + g_exp(L));
                if (llr) llr[b * V + v] = L;
            }
            if (gl == 0) {
                if (iters_out) iters_out[b] = it;
                if (status) status[b] = ok ? 0 : 1;
            }
        }
        wave_tile_sync();                        // tile reads done before the next codewords' writes
    }
}

template <typename T>
static int launch_minsum_layered(const gnnd_graph* g, const void* x, double alpha, double beta,
                                 int iters, int early_stop, void* out, void* llr,
                                 int32_t* iters_out, int32_t* status, int64_t B, hipStream_t st) {
    const LayeredPlan pl = layered_plan(g, sizeof(T));
    if (pl.waves == 0) return GNND_ERR_UNSUPPORTED;
    const size_t lds = (size_t)pl.waves * (64 / pl.G) * pl.cw_bytes;
    minsum_layered_kernel<T><<<wave_tile_blocks(B, (int64_t)pl.waves * (64 / pl.G), pl.waves), 64 * pl.waves, lds, st>>>(
        g->view, pl, g->layer_dev, g->layer_dev + pl.nlayers + 1, (T)alpha, (T)beta, iters,
        early_stop, (const T*)x, (T*)out, (T*)llr, iters_out, status, B);
    GNND_LAUNCH_CHECK();
    return GNND_OK;
}

extern "C" int gnnd_minsum_layered(const gnnd_graph* g, int dtype, const void* d_x, double alpha,
                                   double beta, int32_t iters, int32_t early_stop, void* d_out,
                                   void* d_llr, int32_t* d_iters, int32_t* d_status,
                                   int64_t batch, void* stream) {
    const int rc = gnnd_args_rc(
        g && batch >= 0 && gnnd_minsum_params_ok(alpha, beta, iters, early_stop), dtype);
    if (rc != GNND_OK) return rc;
    if (batch == 0) return GNND_OK;
    if (!d_x || !d_out) return GNND_ERR_INVALID_ARG;
    if (g->min_dc < 2) return GNND_ERR_UNSUPPORTED;
    return gnnd_by_dtype(dtype, [&](auto z) {
        return launch_minsum_layered<decltype(z)>(g, d_x, alpha, beta, iters, early_stop, d_out,
                                                  d_llr, d_iters, d_status, batch,
                                                  (hipStream_t)stream);
    });
}

extern "C" int gnnd_minsum_layered_host(const int64_t* h_var, const int64_t* h_chk,
                                        int64_t num_edges, int32_t num_var, int32_t num_chk,
                                        int dtype, const void* h_x, double alpha, double beta,
                                        int32_t iters, int32_t early_stop, void* h_out,
                                        void* h_llr, int32_t* h_iters, int32_t* h_status,
                                        int64_t batch) {
    return gnnd_minsum_layered_host_checked(h_var, h_chk, num_edges, num_var, num_chk, dtype, h_x,
                                            alpha, beta, iters, early_stop, h_out, h_llr, h_iters,
                                            h_status, batch);
}

extern "C" int gnnd_minsum_layered_plan(const gnnd_graph* g, int dtype, int32_t* h_plan4) {
    const int rc = gnnd_args_rc(g && h_plan4, dtype);
    if (rc != GNND_OK) return rc;
    const LayeredPlan pl = layered_plan(g, dtype == GNND_F32 ? sizeof(float) : sizeof(double));
    if (g->min_dc < 2 || pl.waves == 0) return GNND_ERR_UNSUPPORTED;
    h_plan4[0] = pl.nlayers;
    h_plan4[1] = pl.max_layer;
    h_plan4[2] = pl.G;
    h_plan4[3] = pl.waves * (64 / pl.G);
    return GNND_OK;
}

// ---------------------------------------------------------------------------------------
// gnnd_bposd_layered: gnnd_minsum_layered, then the unchanged gnnd_osd_gated with the min-sum
// status as the gate.  Every refusal of either stage is decided here, before the first launch.
// ---------------------------------------------------------------------------------------
bool gnnd_osd_fits(const gnnd_graph* g, size_t elem);      // gnnd_osd.hip: the LDS limits of gnnd_osd

extern "C" int gnnd_bposd_layered(const gnnd_graph* g, int dtype, const void* d_x, double alpha,
                                  double beta, int32_t iters, int32_t early_stop, int base,
                                  int method, int32_t order, void* d_pred, void* d_llr,
                                  int32_t* d_iters, int32_t* d_bp_status, void* d_ehat,
                                  int32_t* d_status, int32_t* d_choice, void* d_work,
                                  int64_t work_bytes, int64_t batch, void* stream) {
    const int rc = gnnd_args_rc(
        g && batch >= 0 && gnnd_bposd_params_ok(alpha, beta, iters, early_stop, base, method, order),
        dtype);
    if (rc != GNND_OK) return rc;
    if (batch == 0) return GNND_OK;
    if (!d_x || !d_pred || !d_llr || !d_bp_status || !d_ehat || !d_status || !d_work)
        return GNND_ERR_INVALID_ARG;
    if (batch > kOsdGatedMaxBatch) return GNND_ERR_UNSUPPORTED;
    if (work_bytes < gnnd_osd_gated_bytes(batch)) return GNND_ERR_INVALID_ARG;
    const size_t elem = dtype == GNND_F32 ? sizeof(float) : sizeof(double);
    if (g->min_dc < 2 || layered_plan(g, elem).waves == 0 || !gnnd_osd_fits(g, elem))
        return GNND_ERR_UNSUPPORTED;
    const int st = gnnd_minsum_layered(g, dtype, d_x, alpha, beta, iters, early_stop, d_pred, d_llr,
                                       d_iters, d_bp_status, batch, stream);
    if (st != GNND_OK) return st;
    return gnnd_osd_gated(g, dtype, d_x, d_pred, d_llr, d_bp_status, base, method, order, d_ehat,
                          d_status, d_choice, d_work, work_bytes, batch, stream);
}

extern "C" int gnnd_bposd_layered_host(const int64_t* h_var, const int64_t* h_chk,
                                       int64_t num_edges, int32_t num_var, int32_t num_chk,
                                       int dtype, const void* h_x, double alpha, double beta,
                                       int32_t iters, int32_t early_stop, int base, int method,
                                       int32_t order, void* h_pred, void* h_llr, int32_t* h_iters,
                                       int32_t* h_bp_status, void* h_ehat, int32_t* h_status,
                                       int32_t* h_choice, int64_t batch) {
    return gnnd_bposd_layered_host_checked(h_var, h_chk, num_edges, num_var, num_chk, dtype, h_x,
                                           alpha, beta, iters, early_stop, base, method, order,
                                           h_pred, h_llr, h_iters, h_bp_status, h_ehat, h_status,
                                           h_choice, batch);
}

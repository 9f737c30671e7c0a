// gnnd_minsum.hip — min-sum BP with the syndrome-converged early stop (gnnd_minsum,
// include/gnnd.h): normalized / offset min-sum on the flooding schedule, bit-reproducible in
// fp32 and fp64, each codeword stopping once its hard decision satisfies the measured syndrome.
// Built with -ffp-contract=off (Makefile XFLAGS_gnnd_minsum): a * m - b is two roundings, on the
// device and in the host mirror alike.
#include "gnnd_common.h"
#include "gnnd_wave_tile.h"
#include "gnnd_minsum_host.h"
#include "gnnd_bposd_host.h"
#include "gnnd_ufw_host.h"
#include "gnnd_lsd_host.h"

GNND_DEBUG_TU(minsum)

// ---------------------------------------------------------------------------------------
// The wave-private-tile plan and the min-sum steps of gnnd_wave_tile.h.
// A wave's tile: msg[E] (q_e and r_e in place), prior[V] (l_v), llr[V] (L_v), all T.  Per
// iteration:
//   check step     bp_check_step: lanes own checks lane, lane + 64, ...;
//   variable step  lanes own variables: bp_var_sum from l_v (degrees are <= 12 on the shipped
//                  codes), L_v into the tile, bp_var_extrinsic;
//   convergence    bp_syndrome_bad over a lane's checks, one __ballot.
// The early stop is a wave-uniform branch: a finished codeword costs nothing more and the wave
// takes its next codeword.  No index depends on the data, so a NaN or an infinity in x stays
// inside its codeword.
// ---------------------------------------------------------------------------------------
struct MinsumPlan {
    int off_prior, off_llr;   // byte offsets inside one wave's tile (msg at 0)
    int wave_bytes;           // one wave's tile (16-byte multiple)
    int waves;                // waves per workgroup (0: the tile does not fit)
};

static MinsumPlan minsum_plan(int V, int E, size_t elem) {
    MinsumPlan p;
    const size_t msg = wave_tile_align16((size_t)E * elem);
    const size_t node = wave_tile_align16((size_t)V * elem);
    const size_t bytes = msg + 2 * node;          // E, V <= 65535: far below overflow
    p.off_prior = (int)msg;
    p.off_llr = (int)(msg + node);
    p.wave_bytes = (int)bytes;
    p.waves = wave_tile_waves(bytes);
    return p;
}

template <typename T>
__global__ void __launch_bounds__(256)
minsum_kernel(GraphView g, MinsumPlan pl, T a, T bt, int iters, int early_stop,
              const T* __restrict__ x, T* __restrict__ out, T* __restrict__ llr,
              int32_t* __restrict__ iters_out, int32_t* __restrict__ status, int64_t B) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int V = g.V, N = g.N;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    char* tile = smem + (size_t)wave * pl.wave_bytes;
    T* s_msg = (T*)tile;
    T* s_prior = (T*)(tile + pl.off_prior);
    T* s_llr = (T*)(tile + pl.off_llr);

    for (int64_t b = (int64_t)blockIdx.x * pl.waves + wave; b < B;
         b += (int64_t)gridDim.x * pl.waves) {
        const T* xv = x + b * N;
        const T* xc = xv + V;
        // ---- q_e = l_v ----
        for (int v = lane; v < V; v += 64) {
            const T l = xv[v];
            s_prior[v] = l;
            bp_msg_fill(g, s_msg, v, l);
        }
        wave_tile_sync();
        int it = 0;
        bool ok = false;
        while (it < iters) {
            ++it;
            bp_check_step(g, s_msg, xc, a, bt, lane);
            wave_tile_sync();
            for (int v = lane; v < V; v += 64) {
                const int e0 = g.var_ptr[v], e1 = g.var_ptr[v + 1];
                const T s = bp_var_sum(g, s_msg, e0, e1, s_prior[v]);
                s_llr[v] = s;
                bp_var_extrinsic(g, s_msg, e0, e1, s);
            }
            wave_tile_sync();
            // ---- H^T h == t ? (wanted where it can stop the loop, and after the last iteration) ----
            if (early_stop || it == iters) {
                const int bad = bp_syndrome_bad(g, s_llr, xc, lane, 64);
                ok = __ballot(bad) == 0;
                if (early_stop && ok) break;
            }
        }
        // ---- outputs (each lane reads back the L_v it wrote) ----
        for (int v = lane; v < V; v += 64) {
            const T L = s_llr[v];
            out[b * V + v] = T(1) / (T(1) + g_exp(L));
            if (llr) llr[b * V + v] = L;
        }
        if (lane == 0) {
            if (iters_out) iters_out[b] = it;
            if (status) status[b] = ok ? 0 : 1;
        }
        wave_tile_sync();                 // tile reads done before the next codeword's writes
    }
}

template <typename T>
static int launch_minsum(const gnnd_graph* g, const void* x, double alpha, double beta, int iters,
                         int early_stop, void* out, void* llr, int32_t* iters_out,
                         int32_t* status, int64_t B, hipStream_t st) {
    const GraphView& v = g->view;
    const MinsumPlan pl = minsum_plan(v.V, v.E, sizeof(T));
    if (pl.waves == 0) return GNND_ERR_UNSUPPORTED;
    minsum_kernel<T><<<wave_tile_blocks(B, pl.waves, pl.waves), 64 * pl.waves, (size_t)pl.waves * pl.wave_bytes, st>>>(
        v, pl, (T)alpha, (T)beta, iters, early_stop, (const T*)x, (T*)out, (T*)llr, iters_out,
        status, B);
    GNND_LAUNCH_CHECK();
    return GNND_OK;
}

extern "C" int gnnd_minsum(const gnnd_graph* g, int dtype, const void* d_x, double alpha,
                           double beta, int32_t iters, int32_t early_stop, void* d_out,
                           void* d_llr, int32_t* d_iters, int32_t* d_status, int64_t batch,
                           void* stream) {
    const int rc = gnnd_args_rc(
        g && batch >= 0 && gnnd_minsum_params_ok(alpha, beta, iters, early_stop), dtype);
    if (rc != GNND_OK) return rc;
    if (batch == 0) return GNND_OK;
    if (!d_x || !d_out) return GNND_ERR_INVALID_ARG;
    if (g->min_dc < 2) return GNND_ERR_UNSUPPORTED;
    return gnnd_by_dtype(dtype, [&](auto z) {
        return launch_minsum<decltype(z)>(g, d_x, alpha, beta, iters, early_stop, d_out, d_llr,
                                          d_iters, d_status, batch, (hipStream_t)stream);
    });
}

extern "C" int gnnd_minsum_host(const int64_t* h_var, const int64_t* h_chk, int64_t num_edges,
                                int32_t num_var, int32_t num_chk, int dtype, const void* h_x,
                                double alpha, double beta, int32_t iters, int32_t early_stop,
                                void* h_out, void* h_llr, int32_t* h_iters, int32_t* h_status,
                                int64_t batch) {
    return gnnd_minsum_host_checked(h_var, h_chk, num_edges, num_var, num_chk, dtype, h_x, alpha,
                                    beta, iters, early_stop, h_out, h_llr, h_iters, h_status, batch);
}

// ---------------------------------------------------------------------------------------
// gnnd_bposd: gnnd_minsum, then gnnd_osd_gated with the min-sum status as the gate.  Every refusal
// of either stage is decided here, before the first launch.
// ---------------------------------------------------------------------------------------
bool gnnd_osd_fits(const gnnd_graph* g, size_t elem);      // gnnd_osd.hip: the LDS limits of gnnd_osd

extern "C" int gnnd_bposd(const gnnd_graph* g, int dtype, const void* d_x, double alpha,
                          double beta, int32_t iters, int32_t early_stop, int base, int method,
                          int32_t order, void* d_pred, void* d_llr, int32_t* d_iters,
                          int32_t* d_bp_status, void* d_ehat, int32_t* d_status,
                          int32_t* d_choice, void* d_work, int64_t work_bytes, int64_t batch,
                          void* stream) {
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
    if (g->min_dc < 2 || minsum_plan(g->view.V, g->view.E, elem).waves == 0 ||
        !gnnd_osd_fits(g, elem))
        return GNND_ERR_UNSUPPORTED;
    const int st = gnnd_minsum(g, dtype, d_x, alpha, beta, iters, early_stop, d_pred, d_llr,
                               d_iters, d_bp_status, batch, stream);
    if (st != GNND_OK) return st;
    return gnnd_osd_gated(g, dtype, d_x, d_pred, d_llr, d_bp_status, base, method, order, d_ehat,
                          d_status, d_choice, d_work, work_bytes, batch, stream);
}

extern "C" int gnnd_bposd_host(const int64_t* h_var, const int64_t* h_chk, int64_t num_edges,
                               int32_t num_var, int32_t num_chk, int dtype, const void* h_x,
                               double alpha, double beta, int32_t iters, int32_t early_stop,
                               int base, int method, int32_t order, void* h_pred, void* h_llr,
                               int32_t* h_iters, int32_t* h_bp_status, void* h_ehat,
                               int32_t* h_status, int32_t* h_choice, int64_t batch) {
    return gnnd_bposd_host_checked(h_var, h_chk, num_edges, num_var, num_chk, dtype, h_x, alpha,
                                   beta, iters, early_stop, base, method, order, h_pred, h_llr,
                                   h_iters, h_bp_status, h_ehat, h_status, h_choice, batch);
}

// ---------------------------------------------------------------------------------------
// gnnd_bplsd: gnnd_bposd with gnnd_lsd_gated as its second stage.  Every refusal of either stage is
// decided here, before the first launch.
// ---------------------------------------------------------------------------------------
bool gnnd_lsd_fits(const gnnd_graph* g, size_t elem);      // gnnd_lsd.hip: the LDS limits of gnnd_lsd

extern "C" int gnnd_bplsd(const gnnd_graph* g, int dtype, const void* d_x, double alpha,
                          double beta, int32_t iters, int32_t early_stop, int base,
                          int32_t bits_per_step, void* d_pred, void* d_llr, int32_t* d_iters,
                          int32_t* d_bp_status, void* d_ehat, int32_t* d_status,
                          int32_t* d_rounds, int32_t* d_nclus, int32_t* d_ncols, void* d_work,
                          int64_t work_bytes, int64_t batch, void* stream) {
    const int rc = gnnd_args_rc(
        g && batch >= 0 && gnnd_bplsd_params_ok(alpha, beta, iters, early_stop, base, bits_per_step),
        dtype);
    if (rc != GNND_OK) return rc;
    if (batch == 0) return GNND_OK;
    if (!d_x || !d_pred || !d_llr || !d_bp_status || !d_ehat || !d_work)
        return GNND_ERR_INVALID_ARG;
    if (batch > kOsdGatedMaxBatch) return GNND_ERR_UNSUPPORTED;
    if (work_bytes < gnnd_osd_gated_bytes(batch)) return GNND_ERR_INVALID_ARG;
    const size_t elem = dtype == GNND_F32 ? sizeof(float) : sizeof(double);
    if (g->min_dc < 2 || minsum_plan(g->view.V, g->view.E, elem).waves == 0 ||
        !gnnd_lsd_fits(g, elem))
        return GNND_ERR_UNSUPPORTED;
    const int st = gnnd_minsum(g, dtype, d_x, alpha, beta, iters, early_stop, d_pred, d_llr,
                               d_iters, d_bp_status, batch, stream);
    if (st != GNND_OK) return st;
    return gnnd_lsd_gated(g, dtype, d_x, d_pred, d_llr, d_bp_status, base, bits_per_step, d_ehat,
                          d_status, d_rounds, d_nclus, d_ncols, d_work, work_bytes, batch, stream);
}

extern "C" int gnnd_bplsd_host(const int64_t* h_var, const int64_t* h_chk, int64_t num_edges,
                               int32_t num_var, int32_t num_chk, int dtype, const void* h_x,
                               double alpha, double beta, int32_t iters, int32_t early_stop,
                               int base, int32_t bits_per_step, void* h_pred, void* h_llr,
                               int32_t* h_iters, int32_t* h_bp_status, void* h_ehat,
                               int32_t* h_status, int32_t* h_rounds, int32_t* h_nclus,
                               int32_t* h_ncols, int64_t batch) {
    return gnnd_bplsd_host_checked(h_var, h_chk, num_edges, num_var, num_chk, dtype, h_x, alpha,
                                   beta, iters, early_stop, base, bits_per_step, h_pred, h_llr,
                                   h_iters, h_bp_status, h_ehat, h_status, h_rounds, h_nclus,
                                   h_ncols, batch);
}

// ---------------------------------------------------------------------------------------
// gnnd_belief_find: gnnd_minsum, then gnnd_ufw on the min-sum posteriors with the min-sum status as
// the gate, passing the converged codewords through.  Every refusal of either stage is decided
// here, before the first launch.
// ---------------------------------------------------------------------------------------
bool gnnd_uf_fits(const gnnd_graph* g);     // gnnd_ufw.hip: matchable, and the tile of gnnd_uf fits

extern "C" int gnnd_belief_find(const gnnd_graph* g, int dtype, const void* d_x, double alpha,
                                double beta, int32_t iters, int32_t early_stop, double scale,
                                int32_t wmax, void* d_pred, void* d_llr, int32_t* d_iters,
                                int32_t* d_bp_status, void* d_ehat, int32_t* d_status,
                                int32_t* d_rounds, int32_t* d_nfull, int32_t* d_events,
                                int64_t batch, void* stream) {
    const int rc = gnnd_args_rc(g && batch >= 0 &&
                                    gnnd_minsum_params_ok(alpha, beta, iters, early_stop) &&
                                    gnnd_ufw_params_ok(scale, wmax, 1),
                                dtype);
    if (rc != GNND_OK) return rc;
    if (batch == 0) return GNND_OK;
    if (!d_x || !d_pred || !d_llr || !d_bp_status || !d_ehat) return GNND_ERR_INVALID_ARG;
    const size_t elem = dtype == GNND_F32 ? sizeof(float) : sizeof(double);
    if (g->min_dc < 2 || minsum_plan(g->view.V, g->view.E, elem).waves == 0 || !gnnd_uf_fits(g))
        return GNND_ERR_UNSUPPORTED;
    const int st = gnnd_minsum(g, dtype, d_x, alpha, beta, iters, early_stop, d_pred, d_llr,
                               d_iters, d_bp_status, batch, stream);
    if (st != GNND_OK) return st;
    return gnnd_ufw(g, dtype, d_x, d_llr, scale, wmax, d_bp_status, 1, d_ehat, d_rounds, d_status,
                    d_nfull, d_events, batch, stream);
}

extern "C" int gnnd_belief_find_host(const int64_t* h_var, const int64_t* h_chk, int64_t num_edges,
                                     int32_t num_var, int32_t num_chk, int dtype, const void* h_x,
                                     double alpha, double beta, int32_t iters, int32_t early_stop,
                                     double scale, int32_t wmax, void* h_pred, void* h_llr,
                                     int32_t* h_iters, int32_t* h_bp_status, void* h_ehat,
                                     int32_t* h_status, int32_t* h_rounds, int32_t* h_nfull,
                                     int32_t* h_events, int64_t batch) {
    return gnnd_belief_find_host_checked(h_var, h_chk, num_edges, num_var, num_chk, dtype, h_x,
                                         alpha, beta, iters, early_stop, scale, wmax, h_pred, h_llr,
                                         h_iters, h_bp_status, h_ehat, h_status, h_rounds, h_nfull,
                                         h_events, batch);
}

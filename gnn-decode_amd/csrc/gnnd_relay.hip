// gnnd_relay.hip — relay min-sum BP (gnnd_relay, include/gnnd.h): min-sum with a per-variable
// memory term, run as a chain of legs with their own memory strengths; every hard decision that
// satisfies the syndrome is collected and the lightest is kept.  Bit-reproducible in fp32 and fp64.
// gnnd_relay_soft is the same kernel with a soft output (the kept solution's LLRs, or for an
// unsolved codeword the last or the run-averaged posteriors), and gnnd_relay_osd hands that output
// and the relay status to gnnd_osd_gated.
// Built with -ffp-contract=off (Makefile XFLAGS_gnnd_relay): a * m - b is two roundings and
// c * l + g * M three, on the device and in the host mirror alike.
#include "gnnd_common.h"
#include "gnnd_wave_tile.h"
#include "gnnd_relay_host.h"

GNND_DEBUG_TU(relay)

// ---------------------------------------------------------------------------------------
// The wave-private-tile plan and the min-sum steps of gnnd_wave_tile.h.  A wave's tile, all T:
//   msg[E]   q_e and r_e in place
//   pri[V]   the leg's prior term A_v = round(c_v * l_v) (l_v itself where g_v == 0), written
//            once per leg
//   gam[V]   the leg's g_v, read from global memory once per leg (the row is the same for every
//            codeword and stays in L2)
//   llr[V]   L_v, which is also the memory M_v of the next iteration and of the next leg
//   best[V]  L of the lightest solution so far, rewritten only when a solution wins
//   acc[V]   (soft mode MEAN only) the sum of L_v over every executed iteration, from +0
// Lanes own variables lane, lane + 64, ...: the leg set-up, the variable step, the weight partials
// (exactly the contract's p_j, j = lane) and the copy into best touch only a lane's own
// variables, and so do the MEAN accumulation and the soft epilogue, so none of them needs a fence
// of its own.  The six-step xor butterfly leaves the
// same w in every lane.  The prior l_v is re-read from global memory at each leg start and for a
// weight (once per solution), not kept in the tile.
// Leaving a leg, and stopping after S solutions, are wave-uniform branches.  No index depends on
// the data, so a NaN or an infinity in x or gammas stays inside its codeword.
// ---------------------------------------------------------------------------------------
// the kernel's compile-time soft mode: none (gnnd_relay), or gnnd_relay_soft_mode + 1
enum { kRelaySoftNone = 0, kRelaySoftLast = 1, kRelaySoftMean = 2 };

struct RelayPlan {
    int off_pri, off_gam, off_llr, off_best;   // byte offsets inside one wave's tile (msg at 0)
    int off_acc;                               // MEAN only: the accumulator, after best
    int wave_bytes;                            // one wave's tile (16-byte multiple)
    int waves;                                 // waves per workgroup (0: the tile does not fit)
};

static RelayPlan relay_plan(int V, int E, size_t elem, int soft = kRelaySoftNone) {
    RelayPlan p;
    const size_t msg = wave_tile_align16((size_t)E * elem);
    const size_t node = wave_tile_align16((size_t)V * elem);
    // E, V <= 65535: far below overflow
    const size_t bytes = msg + (soft == kRelaySoftMean ? 5 : 4) * node;
    p.off_pri = (int)msg;
    p.off_gam = (int)(msg + node);
    p.off_llr = (int)(msg + 2 * node);
    p.off_best = (int)(msg + 3 * node);
    p.off_acc = (int)(msg + 4 * node);
    p.wave_bytes = (int)bytes;
    p.waves = wave_tile_waves(bytes);
    return p;
}

struct RelayArgs {
    int legs, iters0, iters_leg, stop_after;
    int32_t* iters_out;
    int32_t* status;
    int32_t* leg;
    int32_t* nsol;
};

// the soft outputs of gnnd_relay_soft (unused by the SOFT == kRelaySoftNone instantiation)
template <typename T>
struct RelaySoftOut {
    T* pred;        // [B*V] 1 / (1 + exp(Z_v))
    T* soft;        // [B*V] Z_v, or null
    T inv;          // (T)(1 / (iters0 + (legs - 1) * iters_leg)), computed on the host
};

template <typename T, int SOFT>
__global__ void __launch_bounds__(256)
relay_kernel(GraphView g, RelayPlan pl, RelayArgs ra, T a, T bt, const T* __restrict__ x,
             const T* __restrict__ gammas, T* __restrict__ ehat, T* __restrict__ llr,
             RelaySoftOut<T> so, int64_t B) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int V = g.V, N = g.N;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    char* tile = smem + (size_t)wave * pl.wave_bytes;
    T* s_msg = (T*)tile;
    T* s_pri = (T*)(tile + pl.off_pri);
    T* s_gam = (T*)(tile + pl.off_gam);
    T* s_llr = (T*)(tile + pl.off_llr);
    T* s_best = (T*)(tile + pl.off_best);
    T* s_acc = (T*)(tile + pl.off_acc);     // inside the tile for SOFT == kRelaySoftMean only
    (void)s_acc;

    for (int64_t b = (int64_t)blockIdx.x * pl.waves + wave; b < B;
         b += (int64_t)gridDim.x * pl.waves) {
        const T* xv = x + b * N;
        const T* xc = xv + V;
        for (int v = lane; v < V; v += 64) {
            s_llr[v] = xv[v];                                        // M_v = l_v
            if (SOFT == kRelaySoftMean) s_acc[GNND_DIDX(v, V, GNND_DBG_VAR)] = T(0);
        }
        int total = 0, nsol = 0, bestk = -1;
        T bestw = T(0);
        for (int k = 0; k < ra.legs; ++k) {
            // ---- leg set-up: g_v, A_v, q_e = Lam_v(M) (own variables only) ----
            const T* gk = gammas + (size_t)k * V;
            for (int v = lane; v < V; v += 64) {
                const T l = xv[v];
                const T gm = gk[v];
                const T c = T(1) - gm;
                const T cl = c * l;
                const T A = gm == T(0) ? l : cl;
                s_pri[v] = A;
                s_gam[v] = gm;
                const T gM = gm * s_llr[v];
                const T sum = A + gM;                       // -ffp-contract=off: no fma
                bp_msg_fill(g, s_msg, v, gm == T(0) ? A : sum);
            }
            wave_tile_sync();
            const int Tk = k == 0 ? ra.iters0 : ra.iters_leg;
            for (int it = 0; it < Tk; ++it) {
                ++total;
                bp_check_step(g, s_msg, xc, a, bt, lane);
                wave_tile_sync();
                // ---- variable step: L_v = Lam_v(M) + r_e1 + ..., q_e = L_v - r_e, M_v = L_v ----
                for (int v = lane; v < V; v += 64) {
                    const int e0 = g.var_ptr[v], e1 = g.var_ptr[v + 1];
                    const T A = s_pri[v], gm = s_gam[v];
                    const T gM = gm * s_llr[v];
                    const T sum = A + gM;
                    const T s = bp_var_sum(g, s_msg, e0, e1, gm == T(0) ? A : sum);
                    s_llr[v] = s;
                    if (SOFT == kRelaySoftMean) {
                        const int vi = GNND_DIDX(v, V, GNND_DBG_VAR);
                        s_acc[vi] = s_acc[vi] + s;
                    }
                    bp_var_extrinsic(g, s_msg, e0, e1, s);
                }
                wave_tile_sync();
                const int bad = bp_syndrome_bad(g, s_llr, xc, lane, 64);
                if (__ballot(bad) != 0) continue;
                // ---- a solution: its weight through the contract's tree; keep it if lighter ----
                T p = T(0);
                for (int v = lane; v < V; v += 64) p = p + (s_llr[v] < T(0) ? xv[v] : T(0));
                for (int s = 32; s >= 1; s >>= 1) p = p + __shfl_xor(p, s);
                const int win = __builtin_amdgcn_readfirstlane((int)(nsol == 0 || p < bestw));
                if (win) {
                    bestw = p;
                    bestk = k;
                    for (int v = lane; v < V; v += 64) s_best[v] = s_llr[v];
                }
                ++nsol;
                break;                                          // leave leg k
            }
            if (nsol >= ra.stop_after) break;
        }
        // ---- outputs (each lane reads back the values it wrote) ----
        const T* src = nsol ? s_best : s_llr;
        for (int v = lane; v < V; v += 64) {
            const T L = src[v];
            ehat[b * V + v] = L < T(0) ? T(1) : T(0);
            if (llr) llr[b * V + v] = L;
            if (SOFT != kRelaySoftNone) {
                // Z_v: the kept solution's L; with none, the last L (LAST) or the run's mean
                T Z = L;
                if (SOFT == kRelaySoftMean && !nsol) {
                    const T A = s_acc[GNND_DIDX(v, V, GNND_DBG_VAR)];
                    Z = A * so.inv;                         // -ffp-contract=off: one multiply
                }
                if (so.soft) so.soft[b * V + v] = Z;
                so.pred[b * V + v] = T(1) / (T(1) + g_exp(Z));
            }
        }
        if (lane == 0) {
            if (ra.iters_out) ra.iters_out[b] = total;
            if (ra.status) ra.status[b] = nsol ? 0 : 1;
            if (ra.leg) ra.leg[b] = bestk;
            if (ra.nsol) ra.nsol[b] = nsol;
        }
        wave_tile_sync();                  // tile reads done before the next codeword's writes
    }
}

template <typename T, int SOFT>
static int launch_relay(const gnnd_graph* g, const RelayPlan& pl, const RelayArgs& ra, const void* x,
                        const void* gammas, double alpha, double beta, void* ehat, void* llr,
                        void* pred, void* soft, int64_t B, hipStream_t st) {
    // the MEAN scale: one host division, so the device multiplies
    const double total = (double)ra.iters0 + (double)(ra.legs - 1) * (double)ra.iters_leg;
    const RelaySoftOut<T> so = {(T*)pred, (T*)soft, (T)(1.0 / total)};
    relay_kernel<T, SOFT>
        <<<wave_tile_blocks(B, pl.waves, pl.waves), 64 * pl.waves, (size_t)pl.waves * pl.wave_bytes, st>>>(
            g->view, pl, ra, (T)alpha, (T)beta, (const T*)x, (const T*)gammas, (T*)ehat, (T*)llr, so,
            B);
    GNND_LAUNCH_CHECK();
    return GNND_OK;
}

// the checks of gnnd_relay and gnnd_relay_soft; soft_mode kRelaySoftNone is gnnd_relay
static int relay_run(const gnnd_graph* g, int dtype, const void* d_x, const void* d_gammas,
                     int32_t legs, int32_t iters0, int32_t iters_leg, int32_t stop_after,
                     double alpha, double beta, int soft_mode, void* d_pred, void* d_soft,
                     void* d_ehat, void* d_llr, int32_t* d_iters, int32_t* d_status, int32_t* d_leg,
                     int32_t* d_nsol, int64_t batch, void* stream) {
    const int rc = gnnd_args_rc(
        g && batch >= 0 && gnnd_relay_params_ok(alpha, beta, legs, iters0, iters_leg, stop_after),
        dtype);
    if (rc != GNND_OK) return rc;
    if (batch == 0) return GNND_OK;
    if (!d_x || !d_gammas || !d_ehat || (soft_mode != kRelaySoftNone && !d_pred))
        return GNND_ERR_INVALID_ARG;
    if (g->min_dc < 2) return GNND_ERR_UNSUPPORTED;
    const RelayPlan pl = relay_plan(g->view.V, g->view.E,
                                    dtype == GNND_F32 ? sizeof(float) : sizeof(double), soft_mode);
    if (pl.waves == 0) return GNND_ERR_UNSUPPORTED;
    const RelayArgs ra = {legs, iters0, iters_leg, stop_after, d_iters, d_status, d_leg, d_nsol};
    return gnnd_by_dtype(dtype, [&](auto z) {
        using T = decltype(z);
        hipStream_t st = (hipStream_t)stream;
#define RELAY_LAUNCH(SOFT)                                                                        \
    launch_relay<T, SOFT>(g, pl, ra, d_x, d_gammas, alpha, beta, d_ehat, d_llr, d_pred, d_soft,   \
                          batch, st)
        if (soft_mode == kRelaySoftNone) return RELAY_LAUNCH(kRelaySoftNone);
        if (soft_mode == kRelaySoftLast) return RELAY_LAUNCH(kRelaySoftLast);
        return RELAY_LAUNCH(kRelaySoftMean);
#undef RELAY_LAUNCH
    });
}

extern "C" int gnnd_relay(const gnnd_graph* g, int dtype, const void* d_x, const void* d_gammas,
                          int32_t legs, int32_t iters0, int32_t iters_leg, int32_t stop_after,
                          double alpha, double beta, void* d_ehat, void* d_llr, int32_t* d_iters,
                          int32_t* d_status, int32_t* d_leg, int32_t* d_nsol, int64_t batch,
                          void* stream) {
    return relay_run(g, dtype, d_x, d_gammas, legs, iters0, iters_leg, stop_after, alpha, beta,
                     kRelaySoftNone, nullptr, nullptr, d_ehat, d_llr, d_iters, d_status, d_leg,
                     d_nsol, batch, stream);
}

extern "C" int gnnd_relay_host(const int64_t* h_var, const int64_t* h_chk, int64_t num_edges,
                               int32_t num_var, int32_t num_chk, int dtype, const void* h_x,
                               const void* h_gammas, int32_t legs, int32_t iters0,
                               int32_t iters_leg, int32_t stop_after, double alpha, double beta,
                               void* h_ehat, void* h_llr, int32_t* h_iters, int32_t* h_status,
                               int32_t* h_leg, int32_t* h_nsol, int64_t batch) {
    return gnnd_relay_host_checked(h_var, h_chk, num_edges, num_var, num_chk, dtype, h_x, h_gammas,
                                   legs, iters0, iters_leg, stop_after, alpha, beta, h_ehat, h_llr,
                                   h_iters, h_status, h_leg, h_nsol, batch);
}

// ---------------------------------------------------------------------------------------
// gnnd_relay_soft: the relay kernel's LAST / MEAN instantiations.  A soft mode outside the enum is
// refused with the relay parameters, a null d_pred with the other required pointers.
// ---------------------------------------------------------------------------------------
extern "C" int gnnd_relay_soft(const gnnd_graph* g, int dtype, const void* d_x,
                               const void* d_gammas, int32_t legs, int32_t iters0,
                               int32_t iters_leg, int32_t stop_after, double alpha, double beta,
                               int soft, void* d_pred, void* d_soft, void* d_ehat, void* d_llr,
                               int32_t* d_iters, int32_t* d_status, int32_t* d_leg,
                               int32_t* d_nsol, int64_t batch, void* stream) {
    if (!gnnd_relay_soft_ok(soft)) return GNND_ERR_INVALID_ARG;
    return relay_run(g, dtype, d_x, d_gammas, legs, iters0, iters_leg, stop_after, alpha, beta,
                     soft == GNND_RELAY_SOFT_MEAN ? kRelaySoftMean : kRelaySoftLast, d_pred, d_soft,
                     d_ehat, d_llr, d_iters, d_status, d_leg, d_nsol, batch, stream);
}

extern "C" int gnnd_relay_soft_host(const int64_t* h_var, const int64_t* h_chk, int64_t num_edges,
                                    int32_t num_var, int32_t num_chk, int dtype, const void* h_x,
                                    const void* h_gammas, int32_t legs, int32_t iters0,
                                    int32_t iters_leg, int32_t stop_after, double alpha,
                                    double beta, int soft, void* h_pred, void* h_soft, void* h_ehat,
                                    void* h_llr, int32_t* h_iters, int32_t* h_status,
                                    int32_t* h_leg, int32_t* h_nsol, int64_t batch) {
    return gnnd_relay_soft_host_checked(h_var, h_chk, num_edges, num_var, num_chk, dtype, h_x,
                                        h_gammas, legs, iters0, iters_leg, stop_after, alpha, beta,
                                        soft, h_pred, h_soft, h_ehat, h_llr, h_iters, h_status,
                                        h_leg, h_nsol, batch);
}

// ---------------------------------------------------------------------------------------
// gnnd_relay_osd: gnnd_relay_soft, then gnnd_osd_gated with the relay status as the gate.  Every
// refusal of either stage is decided here, before the first launch.
// ---------------------------------------------------------------------------------------
bool gnnd_osd_fits(const gnnd_graph* g, size_t elem);      // gnnd_osd.hip: the LDS limits of gnnd_osd

extern "C" int gnnd_relay_osd(const gnnd_graph* g, int dtype, const void* d_x, const void* d_gammas,
                              int32_t legs, int32_t iters0, int32_t iters_leg, int32_t stop_after,
                              double alpha, double beta, int soft, int base, int method,
                              int32_t order, void* d_pred, void* d_llr, int32_t* d_iters,
                              int32_t* d_relay_status, int32_t* d_leg, int32_t* d_nsol,
                              void* d_ehat, int32_t* d_status, int32_t* d_choice, void* d_work,
                              int64_t work_bytes, int64_t batch, void* stream) {
    const int rc = gnnd_args_rc(
        g && batch >= 0 &&
            gnnd_relay_osd_params_ok(alpha, beta, legs, iters0, iters_leg, stop_after, soft, base,
                                     method, order),
        dtype);
    if (rc != GNND_OK) return rc;
    if (batch == 0) return GNND_OK;
    if (!d_x || !d_gammas || !d_pred || !d_llr || !d_relay_status || !d_ehat || !d_status ||
        !d_work)
        return GNND_ERR_INVALID_ARG;
    if (batch > kOsdGatedMaxBatch) return GNND_ERR_UNSUPPORTED;
    if (work_bytes < gnnd_osd_gated_bytes(batch)) return GNND_ERR_INVALID_ARG;
    const size_t elem = dtype == GNND_F32 ? sizeof(float) : sizeof(double);
    const int mode = soft == GNND_RELAY_SOFT_MEAN ? kRelaySoftMean : kRelaySoftLast;
    if (g->min_dc < 2 || relay_plan(g->view.V, g->view.E, elem, mode).waves == 0 ||
        !gnnd_osd_fits(g, elem))
        return GNND_ERR_UNSUPPORTED;
    const int st = gnnd_relay_soft(g, dtype, d_x, d_gammas, legs, iters0, iters_leg, stop_after,
                                   alpha, beta, soft, d_pred, nullptr, d_ehat, d_llr, d_iters,
                                   d_relay_status, d_leg, d_nsol, batch, stream);
    if (st != GNND_OK) return st;
    return gnnd_osd_gated(g, dtype, d_x, d_pred, d_llr, d_relay_status, base, method, order, d_ehat,
                          d_status, d_choice, d_work, work_bytes, batch, stream);
}

extern "C" int gnnd_relay_osd_host(const int64_t* h_var, const int64_t* h_chk, int64_t num_edges,
                                   int32_t num_var, int32_t num_chk, int dtype, const void* h_x,
                                   const void* h_gammas, int32_t legs, int32_t iters0,
                                   int32_t iters_leg, int32_t stop_after, double alpha, double beta,
                                   int soft, int base, int method, int32_t order, void* h_pred,
                                   void* h_llr, int32_t* h_iters, int32_t* h_relay_status,
                                   int32_t* h_leg, int32_t* h_nsol, void* h_ehat, int32_t* h_status,
                                   int32_t* h_choice, int64_t batch) {
    return gnnd_relay_osd_host_checked(h_var, h_chk, num_edges, num_var, num_chk, dtype, h_x,
                                       h_gammas, legs, iters0, iters_leg, stop_after, alpha, beta,
                                       soft, base, method, order, h_pred, h_llr, h_iters,
                                       h_relay_status, h_leg, h_nsol, h_ehat, h_status, h_choice,
                                       batch);
}

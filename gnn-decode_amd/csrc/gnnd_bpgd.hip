// gnnd_bpgd.hip — min-sum BP with guided decimation (gnnd_bpgd, include/gnnd.h): rounds of min-sum
// between which the least (or most) reliable undecimated variables get their prior frozen at
// +-clamp, the messages carrying on; a codeword stops at its first hard decision that satisfies the
// syndrome.  Bit-reproducible in fp32 and fp64.
// Built with -ffp-contract=off (Makefile XFLAGS_gnnd_bpgd): a * m - b is two roundings, on the
// device and in the host mirror alike.
#include "gnnd_common.h"
#include "gnnd_wave_tile.h"
#include "gnnd_bpgd_host.h"

GNND_DEBUG_TU(bpgd)

// ---------------------------------------------------------------------------------------
// The wave-private-tile plan and the min-sum steps of gnnd_wave_tile.h.  A wave's tile:
//   msg[E]   T      q_e and r_e in place
//   pri[V]   T      the mutable prior p_v: l_v, or +-c once v is decimated
//   llr[V]   T      L_v of the last variable step, which every pick of a round reads
//   dec[V]   int32  1 once v is decimated
// Lanes own variables lane, lane + 64, ...: the set-up, the variable step, a pick's scan and the
// outputs touch only a lane's own variables.  A pick: each lane scans its own undecimated variables
// in ascending v with a strict compare, starting from the first of them (no sentinel index), then a
// six-step xor butterfly over (|L|, v) pairs, ordered by key and then by lower v, a lane with no
// candidate carrying v = -1 and losing to any lane that has one.  For finite data the order is
// total and every lane ends with the host scan's v*; the value used is lane 0's, broadcast, which
// is some lane's own candidate whatever the data holds (a NaN only fails compares), hence in range
// and undecimated.  Lane 0 writes p_v* and dec_v*, and a wave fence follows before the next pick or
// the next variable step.  That write is the call's one data-dependent index.
// Leaving on ok, and the stop rules, are wave-uniform branches.
// ---------------------------------------------------------------------------------------
struct BpgdPlan {
    int off_pri, off_llr, off_dec;      // byte offsets inside one wave's tile (msg at 0)
    int wave_bytes;                     // one wave's tile (16-byte multiple)
    int waves;                          // waves per workgroup (0: the tile does not fit)
};

static BpgdPlan bpgd_plan(int V, int E, size_t elem) {
    BpgdPlan p;
    const size_t msg = wave_tile_align16((size_t)E * elem);
    const size_t node = wave_tile_align16((size_t)V * elem);
    const size_t dec = wave_tile_align16((size_t)V * sizeof(int32_t));
    const size_t bytes = msg + 2 * node + dec;      // E, V <= 65535: far below overflow
    p.off_pri = (int)msg;
    p.off_llr = (int)(msg + node);
    p.off_dec = (int)(msg + 2 * node);
    p.wave_bytes = (int)bytes;
    p.waves = wave_tile_waves(bytes);
    return p;
}

struct BpgdArgs {
    int iters0, iters_round, rounds, per_round;
    int32_t* iters_out;
    int32_t* status;
    int32_t* ndec;
};

// the pick's strict order on keys: a smaller |L| wins under LEAST, a larger one under MOST
template <typename T, bool MOST>
__device__ __forceinline__ bool bpgd_better(T key, T than) {
    return MOST ? key > than : key < than;
}

// Rule: the pick keeps its running best (bv, bk) with selects, `take ? new : old` on both, never
// with a branch around the two assignments; tests/test_gpu_bpgd.py's toric cases (two to four
// variables per lane) fail if index and key ever get out of step.
template <typename T, bool MOST>
__global__ void __launch_bounds__(256)
bpgd_kernel(GraphView g, BpgdPlan pl, BpgdArgs ba, T a, T bt, T cl, const T* __restrict__ x,
            T* __restrict__ ehat, T* __restrict__ llr, T* __restrict__ pred, int64_t B) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int V = g.V, N = g.N;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    char* tile = smem + (size_t)wave * pl.wave_bytes;
    T* s_msg = (T*)tile;
    T* s_pri = (T*)(tile + pl.off_pri);
    T* s_llr = (T*)(tile + pl.off_llr);
    int32_t* s_dec = (int32_t*)(tile + pl.off_dec);

    for (int64_t b = (int64_t)blockIdx.x * pl.waves + wave; b < B;
         b += (int64_t)gridDim.x * pl.waves) {
        const T* xv = x + b * N;
        const T* xc = xv + V;
        // ---- p_v = l_v, dec_v = 0, q_e = p_v (own variables only) ----
        for (int v = lane; v < V; v += 64) {
            const T l = xv[v];
            s_pri[v] = l;
            s_dec[v] = 0;
            bp_msg_fill(g, s_msg, v, l);
        }
        wave_tile_sync();
        int total = 0, ndec = 0;
        bool ok = false;
        for (int r = 0;; ++r) {
            const int Tr = r == 0 ? ba.iters0 : ba.iters_round;
            for (int it = 0; it < Tr; ++it) {
                ++total;
                bp_check_step(g, s_msg, xc, a, bt, lane);
                wave_tile_sync();
                // ---- L_v = p_v + r_e1 + ..., q_e = L_v - r_e ----
                for (int v = lane; v < V; v += 64) {
                    const int e0 = g.var_ptr[v], e1 = g.var_ptr[v + 1];
                    const T s = bp_var_sum(g, s_msg, e0, e1, s_pri[v]);
                    s_llr[v] = s;
                    bp_var_extrinsic(g, s_msg, e0, e1, s);
                }
                wave_tile_sync();
                const int bad = bp_syndrome_bad(g, s_llr, xc, lane, 64);
                ok = __ballot(bad) == 0;
                if (ok) break;
            }
            if (ok || r == ba.rounds || ndec == V) break;
            // ---- decimation: min(per_round, V - ndec) picks, all reading this round's last L ----
            const int picks = ba.per_round < V - ndec ? ba.per_round : V - ndec;
            for (int k = 0; k < picks; ++k) {
                int bv = -1;                                    // no candidate yet
                T bk = T(0);
                for (int v = lane; v < V; v += 64) {
                    if (s_dec[v]) continue;
                    const T key = g_abs(s_llr[v]);
                    const bool take = bv < 0 || bpgd_better<T, MOST>(key, bk);
                    bv = take ? v : bv;
                    bk = take ? key : bk;
                }
                for (int s = 32; s >= 1; s >>= 1) {
                    const int ov = __shfl_xor(bv, s);
                    const T okey = __shfl_xor(bk, s);
                    const bool take = ov >= 0 && (bv < 0 || bpgd_better<T, MOST>(okey, bk) ||
                                                  (okey == bk && ov < bv));
                    bv = take ? ov : bv;
                    bk = take ? okey : bk;
                }
                // V - ndec >= 1 undecimated variables exist, so lane 0 holds some lane's candidate
                // (the debug build checks that; the vs >= 0 test costs one scalar compare)
                const int vs = GNND_DIDX(__builtin_amdgcn_readfirstlane(bv), V, GNND_DBG_VAR);
                if (lane == 0 && vs >= 0) {
                    s_pri[vs] = s_llr[vs] < T(0) ? -cl : cl;
                    s_dec[vs] = 1;
                }
                ++ndec;
                wave_tile_sync();           // p and dec visible to the next pick / variable step
            }
        }
        // ---- outputs (each lane reads back the L_v it wrote) ----
        for (int v = lane; v < V; v += 64) {
            const T L = s_llr[v];
            ehat[b * V + v] = L < T(0) ? T(1) : T(0);
            if (llr) llr[b * V + v] = L;
            if (pred) pred[b * V + v] = T(1) / (T(1) + g_exp(L));
        }
        if (lane == 0) {
            if (ba.iters_out) ba.iters_out[b] = total;
            if (ba.status) ba.status[b] = ok ? 0 : 1;
            if (ba.ndec) ba.ndec[b] = ndec;
        }
        wave_tile_sync();                   // tile reads done before the next codeword's writes
    }
}

template <typename T, bool MOST>
static int launch_bpgd(const gnnd_graph* g, const BpgdPlan& pl, const BpgdArgs& ba, const void* x,
                       double alpha, double beta, double clamp, void* ehat, void* llr, void* pred,
                       int64_t B, hipStream_t st) {
    bpgd_kernel<T, MOST><<<wave_tile_blocks(B, pl.waves, pl.waves), 64 * pl.waves, (size_t)pl.waves * pl.wave_bytes, st>>>(
        g->view, pl, ba, (T)alpha, (T)beta, (T)clamp, (const T*)x, (T*)ehat, (T*)llr, (T*)pred, B);
    GNND_LAUNCH_CHECK();
    return GNND_OK;
}

extern "C" int gnnd_bpgd(const gnnd_graph* g, int dtype, const void* d_x, double alpha, double beta,
                         int32_t iters0, int32_t iters_round, int32_t rounds, int32_t per_round,
                         int pick, double clamp, void* d_ehat, void* d_llr, void* d_pred,
                         int32_t* d_iters, int32_t* d_status, int32_t* d_ndec, int64_t batch,
                         void* stream) {
    const int rc = gnnd_args_rc(
        g && batch >= 0 &&
            gnnd_bpgd_params_ok(alpha, beta, iters0, iters_round, rounds, per_round, pick, clamp),
        dtype);
    if (rc != GNND_OK) return rc;
    if (!gnnd_bpgd_clamp_fits(dtype, clamp)) return GNND_ERR_INVALID_ARG;
    if (batch == 0) return GNND_OK;
    if (!d_x || !d_ehat) return GNND_ERR_INVALID_ARG;
    if (g->min_dc < 2) return GNND_ERR_UNSUPPORTED;
    const BpgdPlan pl = bpgd_plan(g->view.V, g->view.E,
                                  dtype == GNND_F32 ? sizeof(float) : sizeof(double));
    if (pl.waves == 0) return GNND_ERR_UNSUPPORTED;
    const BpgdArgs ba = {iters0, iters_round, rounds, per_round, d_iters, d_status, d_ndec};
    return gnnd_by_dtype(dtype, [&](auto z) {
        using T = decltype(z);
        hipStream_t st = (hipStream_t)stream;
        if (pick == GNND_BPGD_MOST)
            return launch_bpgd<T, true>(g, pl, ba, d_x, alpha, beta, clamp, d_ehat, d_llr, d_pred,
                                        batch, st);
        return launch_bpgd<T, false>(g, pl, ba, d_x, alpha, beta, clamp, d_ehat, d_llr, d_pred,
                                     batch, st);
    });
}

extern "C" int gnnd_bpgd_host(const int64_t* h_var, const int64_t* h_chk, int64_t num_edges,
                              int32_t num_var, int32_t num_chk, int dtype, const void* h_x,
                              double alpha, double beta, int32_t iters0, int32_t iters_round,
                              int32_t rounds, int32_t per_round, int pick, double clamp,
                              void* h_ehat, void* h_llr, void* h_pred, int32_t* h_iters,
                              int32_t* h_status, int32_t* h_ndec, int64_t batch) {
    return gnnd_bpgd_host_checked(h_var, h_chk, num_edges, num_var, num_chk, dtype, h_x, alpha,
                                  beta, iters0, iters_round, rounds, per_round, pick, clamp, h_ehat,
                                  h_llr, h_pred, h_iters, h_status, h_ndec, batch);
}

// gnnd_minsum.hip — min-sum BP with the syndrome-converged early stop (gnnd_minsum,
// include/gnnd.h): normalized / offset min-sum on the flooding schedule, bit-reproducible in
// fp32 and fp64, each codeword stopping once its hard decision satisfies the measured syndrome.
// Built with -ffp-contract=off (Makefile XFLAGS_gnnd_minsum): a * m - b is two roundings, on the
// device and in the host mirror alike.
#include "gnnd_common.h"
#include "gnnd_minsum_host.h"
#include "gnnd_bposd_host.h"

// this translation unit's debug word: gnnd_debug_take_minsum() (the collector list of
// gnnd_debug_flags lives in the decoder's translation unit, which this feature leaves alone;
// tests/minsum_debug_worker.py reads both)
GNND_DEBUG_TU(minsum)

// ---------------------------------------------------------------------------------------
// One wave per codeword, wave-private LDS, no workgroup barrier (the plan of gnnd_osd.hip).
// A wave's tile: msg[E] (q_e and r_e in place), prior[V] (l_v), llr[V] (L_v), all T.  Per
// iteration:
//   check step     lanes own checks lane, lane + 64, ...: one walk over chk_edge keeps min1,
//                  min2, arg-min and the sign parity, a second walk writes r_e over q_e.  Every
//                  edge belongs to one check, so the two walks of a lane touch only its own
//                  edges: no fence between them;
//   variable step  lanes own variables: l_v + r_e over the var_ptr range in edge order (the
//                  contract's order; degrees are <= 12 on the shipped codes), then q_e = L_v - r_e
//                  and L_v into the tile;
//   convergence    each lane XORs (L_v < 0) over its checks' variables against t_c, one __ballot.
// The early stop is a wave-uniform branch: a finished codeword costs nothing more and the wave
// takes its next codeword.  No index depends on the data, so a NaN or an infinity in x stays
// inside its codeword.
// ---------------------------------------------------------------------------------------
constexpr size_t kMinsumLdsLimit = 64 * 1024;   // dynamic LDS of one workgroup without an opt-in

struct MinsumPlan {
    int off_prior, off_llr;   // byte offsets inside one wave's tile (msg at 0)
    int wave_bytes;           // one wave's tile (16-byte multiple)
    int waves;                // waves per workgroup (0: the tile does not fit)
};

static inline size_t minsum_align16(size_t n) { return (n + 15) & ~(size_t)15; }

static MinsumPlan minsum_plan(int V, int E, size_t elem) {
    MinsumPlan p;
    const size_t msg = minsum_align16((size_t)E * elem), node = minsum_align16((size_t)V * elem);
    const size_t bytes = msg + 2 * node;          // E, V <= 65535: far below overflow
    p.off_prior = (int)msg;
    p.off_llr = (int)(msg + node);
    p.wave_bytes = (int)bytes;
    p.waves = 0;
    if (bytes <= kMinsumLdsLimit) {
        const int fit = (int)(kMinsumLdsLimit / bytes);
        p.waves = fit < 4 ? fit : 4;
    }
    return p;
}

__device__ __forceinline__ void minsum_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <typename T>
__global__ void __launch_bounds__(256)
minsum_kernel(GraphView g, MinsumPlan pl, T a, T bt, int iters, int early_stop,
              const T* __restrict__ x, T* __restrict__ out, T* __restrict__ llr,
              int32_t* __restrict__ iters_out, int32_t* __restrict__ status, int64_t B) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int V = g.V, C = g.C, E = g.E, N = g.N;
    (void)E;                                // read by the debug build's index checks only
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
            for (int e = g.var_ptr[v]; e < g.var_ptr[v + 1]; ++e)
                s_msg[GNND_DIDX(e, E, GNND_DBG_SLOT)] = l;
        }
        minsum_wave_sync();
        int it = 0;
        bool ok = false;
        while (it < iters) {
            ++it;
            // ---- check step ----
            for (int c = lane; c < C; c += 64) {
                const int i0 = g.chk_ptr[c], i1 = g.chk_ptr[c + 1];
                T min1 = (T)INFINITY, min2 = (T)INFINITY;
                int arg = -1;
                int par = xc[c] < T(0);
                for (int i = i0; i < i1; ++i) {
                    const int e = GNND_DIDX(g.chk_edge[GNND_DIDX(i, E, GNND_DBG_SLOT)], E, GNND_DBG_SLOT);
                    const T q = s_msg[e];
                    const T aq = g_abs(q);
                    par ^= (int)(q < T(0));
                    if (aq < min1) { min2 = min1; min1 = aq; arg = e; }
                    else if (aq < min2) min2 = aq;
                }
                for (int i = i0; i < i1; ++i) {
                    const int e = GNND_DIDX(g.chk_edge[GNND_DIDX(i, E, GNND_DBG_SLOT)], E, GNND_DBG_SLOT);
                    const T q = s_msg[e];
                    const T m = e == arg ? min2 : min1;
                    const T am = a * m;
                    const T d = am - bt;                    // -ffp-contract=off: two roundings
                    const T mag = d > T(0) ? d : T(0);
                    s_msg[e] = (par ^ (int)(q < T(0))) ? -mag : mag;
                }
            }
            minsum_wave_sync();
            // ---- variable step ----
            for (int v = lane; v < V; v += 64) {
                const int e0 = g.var_ptr[v], e1 = g.var_ptr[v + 1];
                T s = s_prior[v];
                for (int e = e0; e < e1; ++e) s = s + s_msg[GNND_DIDX(e, E, GNND_DBG_SLOT)];
                s_llr[v] = s;
                for (int e = e0; e < e1; ++e) {
                    const int ei = GNND_DIDX(e, E, GNND_DBG_SLOT);
                    s_msg[ei] = s - s_msg[ei];
                }
            }
            minsum_wave_sync();
            // ---- H^T h == t ? (wanted where it can stop the loop, and after the last iteration) ----
            if (early_stop || it == iters) {
                int bad = 0;
                for (int c = lane; c < C; c += 64) {
                    int par = xc[c] < T(0);
                    for (int i = g.chk_ptr[c]; i < g.chk_ptr[c + 1]; ++i) {
                        const int e = GNND_DIDX(g.chk_edge[GNND_DIDX(i, E, GNND_DBG_SLOT)], E, GNND_DBG_SLOT);
                        const int v = GNND_DIDX((int)(g.edge_vc[e] & 0xffffu), V, GNND_DBG_VAR);
                        par ^= (int)(s_llr[v] < T(0));
                    }
                    bad |= par;
                }
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
        minsum_wave_sync();                 // tile reads done before the next codeword's writes
    }
}

static unsigned minsum_blocks(const MinsumPlan& pl, int64_t B) {
    const int64_t want = (B + pl.waves - 1) / pl.waves;
    const int64_t cap = 8192 / pl.waves;                  // 32 waves per CU, grid-stride
    return (unsigned)(want < cap ? want : cap);
}

template <typename T>
static int launch_minsum(const gnnd_graph* g, const void* x, double alpha, double beta, int iters,
                         int early_stop, void* out, void* llr, int32_t* iters_out,
                         int32_t* status, int64_t B, hipStream_t st) {
    const GraphView& v = g->view;
    const MinsumPlan pl = minsum_plan(v.V, v.E, sizeof(T));
    if (pl.waves == 0) return GNND_ERR_UNSUPPORTED;
    minsum_kernel<T><<<minsum_blocks(pl, B), 64 * pl.waves, (size_t)pl.waves * pl.wave_bytes, st>>>(
        v, pl, (T)alpha, (T)beta, iters, early_stop, (const T*)x, (T*)out, (T*)llr, iters_out,
        status, B);
    GNND_LAUNCH_CHECK();
    return GNND_OK;
}

extern "C" int gnnd_minsum(const gnnd_graph* g, int dtype, const void* d_x, double alpha,
                           double beta, int32_t iters, int32_t early_stop, void* d_out,
                           void* d_llr, int32_t* d_iters, int32_t* d_status, int64_t batch,
                           void* stream) {
    if (!g || batch < 0) return GNND_ERR_INVALID_ARG;
    if (!gnnd_minsum_params_ok(alpha, beta, iters, early_stop)) return GNND_ERR_INVALID_ARG;
    if (dtype == GNND_BF16) return GNND_ERR_UNSUPPORTED;
    if (dtype != GNND_F32 && dtype != GNND_F64) return GNND_ERR_INVALID_ARG;
    if (batch == 0) return GNND_OK;
    if (!d_x || !d_out) return GNND_ERR_INVALID_ARG;
    if (g->min_dc < 2) return GNND_ERR_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    if (dtype == GNND_F32)
        return launch_minsum<float>(g, d_x, alpha, beta, iters, early_stop, d_out, d_llr, d_iters,
                                    d_status, batch, st);
    return launch_minsum<double>(g, d_x, alpha, beta, iters, early_stop, d_out, d_llr, d_iters,
                                 d_status, batch, st);
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
    if (!g || batch < 0) return GNND_ERR_INVALID_ARG;
    if (!gnnd_bposd_params_ok(alpha, beta, iters, early_stop, base, method, order))
        return GNND_ERR_INVALID_ARG;
    if (dtype == GNND_BF16) return GNND_ERR_UNSUPPORTED;
    if (dtype != GNND_F32 && dtype != GNND_F64) return GNND_ERR_INVALID_ARG;
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

// gnnd_relay.hip — relay min-sum BP (gnnd_relay, include/gnnd.h): min-sum with a per-variable
// memory term, run as a chain of legs with their own memory strengths; every hard decision that
// satisfies the syndrome is collected and the lightest is kept.  Bit-reproducible in fp32 and fp64.
// Built with -ffp-contract=off (Makefile XFLAGS_gnnd_relay): a * m - b is two roundings and
// c * l + g * M three, on the device and in the host mirror alike.
#include "gnnd_common.h"
#include "gnnd_relay_host.h"

// this translation unit's debug word: gnnd_debug_take_relay() (tests/relay_debug_worker.py reads it
// next to gnnd_debug_flags)
GNND_DEBUG_TU(relay)

// ---------------------------------------------------------------------------------------
// The plan of gnnd_minsum.hip: one wave per codeword, a wave-private LDS tile, wave fences only, a
// grid-stride loop over codewords.  A wave's tile, all T:
//   msg[E]   q_e and r_e in place
//   pri[V]   the leg's prior term A_v = round(c_v * l_v) (l_v itself where g_v == 0), written
//            once per leg
//   gam[V]   the leg's g_v, read from global memory once per leg (the row is the same for every
//            codeword and stays in L2)
//   llr[V]   L_v, which is also the memory M_v of the next iteration and of the next leg
//   best[V]  L of the lightest solution so far, rewritten only when a solution wins
// Lanes own variables lane, lane + 64, ...: the leg set-up, the variable step, the weight partials
// (exactly the contract's p_j, j = lane) and the copy into best touch only a lane's own
// variables, so none of them needs a fence of its own.  The six-step xor butterfly leaves the
// same w in every lane.  The prior l_v is re-read from global memory at each leg start and for a
// weight (once per solution), not kept in the tile.
// Leaving a leg, and stopping after S solutions, are wave-uniform branches.  No index depends on
// the data, so a NaN or an infinity in x or gammas stays inside its codeword.
// ---------------------------------------------------------------------------------------
constexpr size_t kRelayLdsLimit = 64 * 1024;    // dynamic LDS of one workgroup without an opt-in

struct RelayPlan {
    int off_pri, off_gam, off_llr, off_best;   // byte offsets inside one wave's tile (msg at 0)
    int wave_bytes;                            // one wave's tile (16-byte multiple)
    int waves;                                 // waves per workgroup (0: the tile does not fit)
};

static inline size_t relay_align16(size_t n) { return (n + 15) & ~(size_t)15; }

static RelayPlan relay_plan(int V, int E, size_t elem) {
    RelayPlan p;
    const size_t msg = relay_align16((size_t)E * elem), node = relay_align16((size_t)V * elem);
    const size_t bytes = msg + 4 * node;           // E, V <= 65535: far below overflow
    p.off_pri = (int)msg;
    p.off_gam = (int)(msg + node);
    p.off_llr = (int)(msg + 2 * node);
    p.off_best = (int)(msg + 3 * node);
    p.wave_bytes = (int)bytes;
    p.waves = 0;
    if (bytes <= kRelayLdsLimit) {
        const int fit = (int)(kRelayLdsLimit / bytes);
        p.waves = fit < 4 ? fit : 4;
    }
    return p;
}

__device__ __forceinline__ void relay_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

struct RelayArgs {
    int legs, iters0, iters_leg, stop_after;
    int32_t* iters_out;
    int32_t* status;
    int32_t* leg;
    int32_t* nsol;
};

template <typename T>
__global__ void __launch_bounds__(256)
relay_kernel(GraphView g, RelayPlan pl, RelayArgs ra, T a, T bt, const T* __restrict__ x,
             const T* __restrict__ gammas, T* __restrict__ ehat, T* __restrict__ llr, int64_t B) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int V = g.V, C = g.C, E = g.E, N = g.N;
    (void)E;                                // read by the debug build's index checks only
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    char* tile = smem + (size_t)wave * pl.wave_bytes;
    T* s_msg = (T*)tile;
    T* s_pri = (T*)(tile + pl.off_pri);
    T* s_gam = (T*)(tile + pl.off_gam);
    T* s_llr = (T*)(tile + pl.off_llr);
    T* s_best = (T*)(tile + pl.off_best);

    for (int64_t b = (int64_t)blockIdx.x * pl.waves + wave; b < B;
         b += (int64_t)gridDim.x * pl.waves) {
        const T* xv = x + b * N;
        const T* xc = xv + V;
        for (int v = lane; v < V; v += 64) s_llr[v] = xv[v];         // M_v = l_v
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
                const T lam = gm == T(0) ? A : sum;
                for (int e = g.var_ptr[v]; e < g.var_ptr[v + 1]; ++e)
                    s_msg[GNND_DIDX(e, E, GNND_DBG_SLOT)] = lam;
            }
            relay_wave_sync();
            const int Tk = k == 0 ? ra.iters0 : ra.iters_leg;
            for (int it = 0; it < Tk; ++it) {
                ++total;
                // ---- check step (gnnd_minsum's) ----
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
                        const T d = am - bt;                    // two roundings
                        const T mag = d > T(0) ? d : T(0);
                        s_msg[e] = (par ^ (int)(q < T(0))) ? -mag : mag;
                    }
                }
                relay_wave_sync();
                // ---- variable step: L_v = Lam_v(M) + r_e1 + ..., q_e = L_v - r_e, M_v = L_v ----
                for (int v = lane; v < V; v += 64) {
                    const int e0 = g.var_ptr[v], e1 = g.var_ptr[v + 1];
                    const T A = s_pri[v], gm = s_gam[v];
                    const T gM = gm * s_llr[v];
                    const T sum = A + gM;
                    T s = gm == T(0) ? A : sum;
                    for (int e = e0; e < e1; ++e) s = s + s_msg[GNND_DIDX(e, E, GNND_DBG_SLOT)];
                    s_llr[v] = s;
                    for (int e = e0; e < e1; ++e) {
                        const int ei = GNND_DIDX(e, E, GNND_DBG_SLOT);
                        s_msg[ei] = s - s_msg[ei];
                    }
                }
                relay_wave_sync();
                // ---- H^T h == t ? ----
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
        }
        if (lane == 0) {
            if (ra.iters_out) ra.iters_out[b] = total;
            if (ra.status) ra.status[b] = nsol ? 0 : 1;
            if (ra.leg) ra.leg[b] = bestk;
            if (ra.nsol) ra.nsol[b] = nsol;
        }
        relay_wave_sync();                  // tile reads done before the next codeword's writes
    }
}

static unsigned relay_blocks(const RelayPlan& pl, int64_t B) {
    const int64_t want = (B + pl.waves - 1) / pl.waves;
    const int64_t cap = 8192 / pl.waves;                  // 32 waves per CU, grid-stride
    return (unsigned)(want < cap ? want : cap);
}

template <typename T>
static int launch_relay(const gnnd_graph* g, const RelayPlan& pl, const RelayArgs& ra, const void* x,
                        const void* gammas, double alpha, double beta, void* ehat, void* llr,
                        int64_t B, hipStream_t st) {
    relay_kernel<T><<<relay_blocks(pl, B), 64 * pl.waves, (size_t)pl.waves * pl.wave_bytes, st>>>(
        g->view, pl, ra, (T)alpha, (T)beta, (const T*)x, (const T*)gammas, (T*)ehat, (T*)llr, B);
    GNND_LAUNCH_CHECK();
    return GNND_OK;
}

extern "C" int gnnd_relay(const gnnd_graph* g, int dtype, const void* d_x, const void* d_gammas,
                          int32_t legs, int32_t iters0, int32_t iters_leg, int32_t stop_after,
                          double alpha, double beta, void* d_ehat, void* d_llr, int32_t* d_iters,
                          int32_t* d_status, int32_t* d_leg, int32_t* d_nsol, int64_t batch,
                          void* stream) {
    if (!g || batch < 0) return GNND_ERR_INVALID_ARG;
    if (!gnnd_relay_params_ok(alpha, beta, legs, iters0, iters_leg, stop_after))
        return GNND_ERR_INVALID_ARG;
    if (dtype == GNND_BF16) return GNND_ERR_UNSUPPORTED;
    if (dtype != GNND_F32 && dtype != GNND_F64) return GNND_ERR_INVALID_ARG;
    if (batch == 0) return GNND_OK;
    if (!d_x || !d_gammas || !d_ehat) return GNND_ERR_INVALID_ARG;
    if (g->min_dc < 2) return GNND_ERR_UNSUPPORTED;
    const RelayPlan pl =
        relay_plan(g->view.V, g->view.E, dtype == GNND_F32 ? sizeof(float) : sizeof(double));
    if (pl.waves == 0) return GNND_ERR_UNSUPPORTED;
    const RelayArgs ra = {legs, iters0, iters_leg, stop_after, d_iters, d_status, d_leg, d_nsol};
    hipStream_t st = (hipStream_t)stream;
    if (dtype == GNND_F32)
        return launch_relay<float>(g, pl, ra, d_x, d_gammas, alpha, beta, d_ehat, d_llr, batch, st);
    return launch_relay<double>(g, pl, ra, d_x, d_gammas, alpha, beta, d_ehat, d_llr, batch, st);
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

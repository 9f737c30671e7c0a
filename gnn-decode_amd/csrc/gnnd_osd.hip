// gnnd_osd.hip — OSD post-processing (gnnd_osd0 / gnnd_osd / gnnd_osd_gated, include/gnnd.h): turns
// the decoders' soft outputs into an estimate that satisfies the measured syndrome whenever one exists (order
// 0), and among the higher-order candidates (combination sweep, exhaustive) the lightest one.
#include "gnnd_common.h"
#include "gnnd_wave_tile.h"
#include "gnnd_osd_host.h"
#include "gnnd_osd_tile.h"

GNND_DEBUG_TU(osd)

// ---------------------------------------------------------------------------------------
// The wave-private-tile plan of gnnd_wave_tile.h with the tile and the shared steps of
// gnnd_osd_tile.h (phases 1-3, which gnnd_lsd.hip runs too).  Per codeword:
//   1. keys into LDS; every lane ranks its variables by counting (rank(v) = #{u : key_u > key_v
//      or (key_u == key_v and u < v)}: a permutation, O(V^2 / 64) compares per lane) and scatters
//      v to order[rank];
//   2. A = H^T, bit-packed rows of `stride` words (ceil(V/32) column words, one syndrome word,
//      padded to an odd count: lanes own rows lane, lane + 64, ..., so a wave's accesses to one
//      word of 64 consecutive rows fall on distinct banks), built from the graph's check CSR;
//      the syndrome word holds s = t xor H^T z;
//   3. Gauss-Jordan over the columns in order: __ballot of the unused rows holding the column's
//      bit, the first one is the pivot, its words are broadcast (one LDS address for the wave;
//      all-zero words skipped) and XORed into every other row holding the bit;
//   4. status = some unused row is left with s = 1; else e[pivot column of row r] = s[r].
// gnnd_osd (osd_kernel) runs phases 1-3 through the same functions and, where 4 finds a
// solution, a candidate phase on the reduced tile [I | T] before it writes e:
//   5. the pivot columns are marked (bit 1 of their e byte) and the column order is compacted in
//      place to the free list f_0 .. f_{F-1} (ballot prefix counts; a free column's slot is
//      never after its walk position, so no second array);
//   6. per lane three 32-bit masks over its rows (bit k = row lane + 64 k): used, s, and for a
//      free column f its bits col_f (rpl reads of word f / 32, the same conflict-free access as
//      phase 3).  A candidate S costs |S| + sum over the wave of popc((s ^ XOR_{f in S} col_f)
//      & used): one __ballot + popcount when C <= 64, else a DPP / shuffle add.  Combination
//      sweep: all singles, then the pairs of the first lambda free columns; exhaustive: the
//      2^lambda subsets in Gray-code order, one column XORed into a running mask per step.  The
//      best (cost, index) stays wave-uniform in scalars, ties to the lowest index;
//   7. e is written once, for the chosen candidate: its free columns and the pivots of the rows
//      its mask leaves set.
// ---------------------------------------------------------------------------------------

template <typename T>
__global__ void __launch_bounds__(256)
osd0_kernel(GraphView g, OsdPlan pl, int hard, const T* __restrict__ x,
            const T* __restrict__ pred, T* __restrict__ ehat, int32_t* __restrict__ status,
            int64_t B) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int V = g.V, C = g.C, N = g.N;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int S = pl.stride, syn = pl.words;
    const OsdTile<T> t(smem + (size_t)wave * pl.wave_bytes, pl);
    uint32_t* A = t.A;
    uint16_t* s_piv = t.piv;
    uint8_t* s_e = t.e;

    for (int64_t b = (int64_t)blockIdx.x * pl.waves + wave; b < B;
         b += (int64_t)gridDim.x * pl.waves) {
        osd_keys_and_order(t, V, hard, pred + b * V, lane);
        osd_build_rows(t, g, pl, x + b * N + V, lane);
        const uint32_t used = osd_eliminate(t, pl, V, C, lane);
        // ---- solution ----
        int bad = 0;
        for (int k = 0; k < pl.rpl; ++k) {
            const int r = lane + 64 * k;
            if (r < C && !((used >> k) & 1u)) bad |= (int)(A[(size_t)r * S + syn] & 1u);
        }
        const bool fail = __ballot(bad) != 0;
        if (!fail)
            for (int k = 0; k < pl.rpl; ++k) {
                const int r = lane + 64 * k;
                if (r < C && ((used >> k) & 1u) && (A[(size_t)r * S + syn] & 1u))
                    s_e[GNND_DIDX((int)s_piv[r], V, GNND_DBG_VAR)] ^= 1;    // one pivot per column
            }
        wave_tile_sync();
        T* eb = ehat + b * V;
        for (int v = lane; v < V; v += 64) eb[v] = s_e[v] ? T(1) : T(0);
        if (lane == 0) status[b] = fail ? 1 : 0;
        wave_tile_sync();                    // tile reads done before the next codeword's writes
    }
}

// ---------------------------------------------------------------------------------------
// higher-order candidates (phases 5-7)
// ---------------------------------------------------------------------------------------
template <int CTRL> __device__ __forceinline__ int osd_dpp(int v) {
    return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xf, 0xf, false);
}
// sum over the 64 lanes (all active), the same value in every lane
__device__ __forceinline__ int osd_wave_sum(int v) {
    v += osd_dpp<0xB1>(v);     // quad_perm [1,0,3,2]
    v += osd_dpp<0x4E>(v);     // quad_perm [2,3,0,1]
    v += osd_dpp<0x141>(v);    // row_half_mirror
    v += osd_dpp<0x140>(v);    // row_mirror
    v += __shfl_xor(v, 16);
    v += __shfl_xor(v, 32);
    return v;
}
// number of set bits of a per-lane row mask over the wave, wave-uniform; `one`: one row per lane
__device__ __forceinline__ int osd_weight(uint32_t m, bool one) {
    if (one) return __popcll(__ballot(m & 1u));
    return __builtin_amdgcn_readfirstlane(osd_wave_sum(__popc(m)));
}
// bits of column f over the lane's rows (bit k: row lane + 64 k)
__device__ __forceinline__ uint32_t osd_col_mask(const uint32_t* A, int S, int C, int rpl,
                                                 int lane, int f) {
    const int wf = f >> 5, sh = f & 31;
    uint32_t m = 0;
    for (int k = 0; k < rpl; ++k) {
        const int r = lane + 64 * k;
        if (r < C) m |= ((A[(size_t)r * S + wf] >> sh) & 1u) << k;
    }
    return m;
}

// ---- one codeword of gnnd_osd on the wave's tile: phases 1-7, then e, status and choice ----
template <typename T>
__device__ __forceinline__ void osd_codeword(const OsdTile<T>& t, const GraphView& g,
                                             const OsdPlan& pl, int hard, int method, int order,
                                             const T* __restrict__ x, const T* __restrict__ pred,
                                             T* __restrict__ ehat, int32_t* __restrict__ status,
                                             int32_t* __restrict__ choice, int64_t b, int lane) {
    const int V = g.V, C = g.C, N = g.N;
    const int S = pl.stride, syn = pl.words, rpl = pl.rpl;
    const bool one = rpl == 1;
    const uint32_t* A = t.A;
    uint16_t* s_order = t.order;
    uint8_t* s_e = t.e;
    osd_keys_and_order(t, V, hard, pred + b * V, lane);
    osd_build_rows(t, g, pl, x + b * N + V, lane);
    const uint32_t used = osd_eliminate(t, pl, V, C, lane);
    uint32_t smask = 0;                 // bit k: reduced s of row lane + 64 k
    for (int k = 0; k < rpl; ++k) {
        const int r = lane + 64 * k;
        if (r < C) smask |= (A[(size_t)r * S + syn] & 1u) << k;
    }
    const bool fail = __ballot((smask & ~used) != 0) != 0;
    int best_idx = 0;
    if (!fail) {
        uint32_t fm = smask;            // the chosen candidate's s xor its columns
        if (method != GNND_OSD_0) {
            // ---- free list: mark the pivot columns, compact the order in place ----
            for (int k = 0; k < rpl; ++k)
                if ((used >> k) & 1u)
                    s_e[GNND_DIDX((int)t.piv[lane + 64 * k], V, GNND_DBG_VAR)] |= 2;
            wave_tile_sync();
            int F = 0;
            for (int base = 0; base < V; base += 64) {
                const int pos = base + lane;
                int v = 0;
                bool fr = false;
                if (pos < V) {
                    v = GNND_DIDX((int)s_order[pos], V, GNND_DBG_VAR);
                    fr = !(s_e[v] & 2);
                }
                const unsigned long long m = __ballot(fr);
                wave_tile_sync();        // every slot of the chunk read before one is rewritten
                if (fr)
                    s_order[GNND_DIDX(F + __popcll(m & ((1ull << lane) - 1)), pos + 1,
                                      GNND_DBG_LDS_POS)] = (uint16_t)v;
                F += __popcll(m);
            }
            wave_tile_sync();
            GNND_DCHECK(F <= V, GNND_DBG_LDS_POS);
            // ---- candidates ----
            int best = osd_weight(smask & used, one);
            const int lam = order < F ? order : F;
            if (method == GNND_OSD_CS) {
                int ba = -1, bb = -1;
                for (int i = 0; i < F; ++i) {
                    const int f = GNND_DIDX((int)s_order[i], V, GNND_DBG_VAR);
                    const uint32_t m = smask ^ osd_col_mask(A, S, C, rpl, lane, f);
                    const int c = 1 + osd_weight(m & used, one);
                    if (c < best) { best = c; best_idx = 1 + i; ba = i; }
                }
                int idx = 1 + F;
                for (int a = 0; a + 1 < lam; ++a) {
                    const int fa = GNND_DIDX((int)s_order[a], V, GNND_DBG_VAR);
                    const uint32_t ma = smask ^ osd_col_mask(A, S, C, rpl, lane, fa);
                    for (int q = a + 1; q < lam; ++q, ++idx) {
                        const int fq = GNND_DIDX((int)s_order[q], V, GNND_DBG_VAR);
                        const uint32_t m = ma ^ osd_col_mask(A, S, C, rpl, lane, fq);
                        const int c = 2 + osd_weight(m & used, one);
                        if (c < best) { best = c; best_idx = idx; ba = a; bb = q; }
                    }
                }
                if (ba >= 0) {
                    const int fa = GNND_DIDX((int)s_order[ba], V, GNND_DBG_VAR);
                    fm ^= osd_col_mask(A, S, C, rpl, lane, fa);
                    if (lane == 0) s_e[fa] ^= 1;
                }
                if (bb >= 0) {
                    const int fq = GNND_DIDX((int)s_order[bb], V, GNND_DBG_VAR);
                    fm ^= osd_col_mask(A, S, C, rpl, lane, fq);
                    if (lane == 0) s_e[fq] ^= 1;
                }
            } else {
                uint32_t run = smask;
                int gray = 0;           // the subset visited: Gray code of the step
                for (int i = 1; i < (1 << lam); ++i) {
                    const int bit = __builtin_ctz(i);
                    gray ^= 1 << bit;
                    const int f = GNND_DIDX((int)s_order[bit], V, GNND_DBG_VAR);
                    run ^= osd_col_mask(A, S, C, rpl, lane, f);
                    const int c = __popc(gray) + osd_weight(run & used, one);
                    if (c < best || (c == best && gray < best_idx)) { best = c; best_idx = gray; }
                }
                for (int i = 0; i < lam; ++i)
                    if ((best_idx >> i) & 1) {
                        const int f = GNND_DIDX((int)s_order[i], V, GNND_DBG_VAR);
                        fm ^= osd_col_mask(A, S, C, rpl, lane, f);
                        if (lane == 0) s_e[f] ^= 1;
                    }
            }
        }
        // ---- solution: the pivots of the rows the chosen mask leaves set ----
        for (int k = 0; k < rpl; ++k)
            if ((used >> k) & (fm >> k) & 1u)
                s_e[GNND_DIDX((int)t.piv[lane + 64 * k], V, GNND_DBG_VAR)] ^= 1;
    }
    wave_tile_sync();
    T* eb = ehat + b * V;
    for (int v = lane; v < V; v += 64) eb[v] = (s_e[v] & 1) ? T(1) : T(0);
    if (lane == 0) {
        status[b] = fail ? 1 : 0;
        if (choice) choice[b] = best_idx;
    }
    wave_tile_sync();                    // tile reads done before the next codeword's writes
}

template <typename T>
__global__ void __launch_bounds__(256)
osd_kernel(GraphView g, OsdPlan pl, int hard, int method, int order, const T* __restrict__ x,
           const T* __restrict__ pred, T* __restrict__ ehat, int32_t* __restrict__ status,
           int32_t* __restrict__ choice, int64_t B) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const OsdTile<T> t(smem + (size_t)wave * pl.wave_bytes, pl);
    for (int64_t b = (int64_t)blockIdx.x * pl.waves + wave; b < B;
         b += (int64_t)gridDim.x * pl.waves)
        osd_codeword(t, g, pl, hard, method, order, x, pred, ehat, status, choice, b, lane);
}

// ---------------------------------------------------------------------------------------
// gated OSD (gnnd_osd_gated): only the codewords with gate != 0 are eliminated.  The host does not
// know how many there are, so two launches share the caller's scratch, int32 count then int32
// list[B]:
//   osd_gate_kernel   (gnnd_osd_tile.h) the ascending list of gated codewords and their count, and
//                     the pass-through outputs of the ungated ones: status 0, choice -1;
//   osd_gated_kernel  osd_kernel's plan and grid (the worst case); wave w takes list entries
//                     w, w + (waves in flight), ... below the count it reads from the scratch and
//                     runs osd_codeword on list[i].  With count 0 every wave leaves at once.
// ---------------------------------------------------------------------------------------

template <typename T>
__global__ void __launch_bounds__(256)
osd_gated_kernel(GraphView g, OsdPlan pl, int hard, int method, int order,
                 const T* __restrict__ x, const T* __restrict__ pred, T* __restrict__ ehat,
                 int32_t* __restrict__ status, int32_t* __restrict__ choice,
                 const int32_t* __restrict__ work, int64_t B) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const OsdTile<T> t(smem + (size_t)wave * pl.wave_bytes, pl);
    const int count = GNND_DIDX(work[0], (int)B + 1, GNND_DBG_GRID);    // <= B; the list follows
    // count < 2^31 and at most 8192 waves in flight: the unsigned index cannot wrap; the list
    // entry is the same for the whole wave and stays in scalar registers
    for (unsigned i = blockIdx.x * pl.waves + wave; i < (unsigned)count; i += gridDim.x * pl.waves) {
        const int64_t b = (unsigned)GNND_DIDX(__builtin_amdgcn_readfirstlane(work[1 + (size_t)i]),
                                              (int)B, GNND_DBG_GRID);
        osd_codeword(t, g, pl, hard, method, order, x, pred, ehat, status, choice, b, lane);
    }
}

template <typename T>
static int launch_osd0(const gnnd_graph* g, const void* x, const void* pred, int base, void* ehat,
                       int32_t* status, int64_t B, hipStream_t st) {
    const GraphView& v = g->view;
    const OsdPlan pl = osd_plan(v.V, v.C, sizeof(T));
    if (pl.waves == 0) return GNND_ERR_UNSUPPORTED;
    osd0_kernel<T><<<wave_tile_blocks(B, pl.waves, pl.waves), 64 * pl.waves, (size_t)pl.waves * pl.wave_bytes, st>>>(
        v, pl, base == GNND_OSD_BASE_HARD, (const T*)x, (const T*)pred, (T*)ehat, status, B);
    GNND_LAUNCH_CHECK();
    return GNND_OK;
}

template <typename T>
static int launch_osd(const gnnd_graph* g, const void* x, const void* pred, int base, int method,
                      int order, void* ehat, int32_t* status, int32_t* choice, int64_t B,
                      hipStream_t st) {
    const GraphView& v = g->view;
    const OsdPlan pl = osd_plan(v.V, v.C, sizeof(T));
    if (pl.waves == 0) return GNND_ERR_UNSUPPORTED;
    osd_kernel<T><<<wave_tile_blocks(B, pl.waves, pl.waves), 64 * pl.waves, (size_t)pl.waves * pl.wave_bytes, st>>>(
        v, pl, base == GNND_OSD_BASE_HARD, method, order, (const T*)x, (const T*)pred, (T*)ehat,
        status, choice, B);
    GNND_LAUNCH_CHECK();
    return GNND_OK;
}

extern "C" int gnnd_osd0(const gnnd_graph* g, int dtype, const void* d_x, const void* d_pred,
                         int base, void* d_ehat, int32_t* d_status, int64_t batch, void* stream) {
    const int rc = gnnd_args_rc(g && batch >= 0 && gnnd_osd_base_ok(base), dtype);
    if (rc != GNND_OK) return rc;
    if (batch == 0) return GNND_OK;
    if (!d_x || !d_pred || !d_ehat || !d_status) return GNND_ERR_INVALID_ARG;
    return gnnd_by_dtype(dtype, [&](auto z) {
        return launch_osd0<decltype(z)>(g, d_x, d_pred, base, d_ehat, d_status, batch,
                                        (hipStream_t)stream);
    });
}

extern "C" int gnnd_osd0_host(const int64_t* h_var, const int64_t* h_chk, int64_t num_edges,
                              int32_t num_var, int32_t num_chk, int dtype, const void* h_x,
                              const void* h_pred, int base, void* h_ehat, int32_t* h_status,
                              int64_t batch) {
    return gnnd_osd0_host_checked(h_var, h_chk, num_edges, num_var, num_chk, dtype, h_x, h_pred,
                                  base, h_ehat, h_status, batch);
}

extern "C" int gnnd_osd(const gnnd_graph* g, int dtype, const void* d_x, const void* d_pred,
                        int base, int method, int32_t order, void* d_ehat, int32_t* d_status,
                        int32_t* d_choice, int64_t batch, void* stream) {
    const int rc = gnnd_args_rc(
        g && batch >= 0 && gnnd_osd_base_ok(base) && gnnd_osd_order_ok(method, order), dtype);
    if (rc != GNND_OK) return rc;
    if (batch == 0) return GNND_OK;
    if (!d_x || !d_pred || !d_ehat || !d_status) return GNND_ERR_INVALID_ARG;
    return gnnd_by_dtype(dtype, [&](auto z) {
        return launch_osd<decltype(z)>(g, d_x, d_pred, base, method, order, d_ehat, d_status,
                                       d_choice, batch, (hipStream_t)stream);
    });
}

extern "C" int gnnd_osd_host(const int64_t* h_var, const int64_t* h_chk, int64_t num_edges,
                             int32_t num_var, int32_t num_chk, int dtype, const void* h_x,
                             const void* h_pred, int base, int method, int32_t order,
                             void* h_ehat, int32_t* h_status, int32_t* h_choice, int64_t batch) {
    return gnnd_osd_host_checked(h_var, h_chk, num_edges, num_var, num_chk, dtype, h_x, h_pred,
                                 base, method, order, h_ehat, h_status, h_choice, batch);
}

// ---- gated OSD ----
// the LDS limits of gnnd_osd for this graph and element size (gnnd_bposd, gnnd_minsum.hip, asks
// before its first launch)
bool gnnd_osd_fits(const gnnd_graph* g, size_t elem) {
    return osd_plan(g->view.V, g->view.C, elem).waves != 0;
}

template <typename T>
static int launch_osd_gated(const gnnd_graph* g, const void* x, const void* pred, const void* llr,
                            const int32_t* gate, int base, int method, int order, void* ehat,
                            int32_t* status, int32_t* choice, int32_t* work, int64_t B,
                            hipStream_t st) {
    const GraphView& v = g->view;
    const OsdPlan pl = osd_plan(v.V, v.C, sizeof(T));
    if (pl.waves == 0) return GNND_ERR_UNSUPPORTED;
    const GateInts ints = {{status, choice, nullptr, nullptr}, {0, -1, 0, 0}};
    osd_gate_kernel<T><<<osd_gate_blocks(B), kGateThreads, 0, st>>>(
        v.V, gate, (const T*)pred, (const T*)llr, (T*)ehat, ints, work, B);
    GNND_LAUNCH_CHECK();
    osd_gated_kernel<T><<<wave_tile_blocks(B, pl.waves, pl.waves), 64 * pl.waves, (size_t)pl.waves * pl.wave_bytes, st>>>(
        v, pl, base == GNND_OSD_BASE_HARD, method, order, (const T*)x, (const T*)pred, (T*)ehat,
        status, choice, work, B);
    GNND_LAUNCH_CHECK();
    return GNND_OK;
}

extern "C" int gnnd_osd_gated_workspace(int64_t batch, int64_t* h_bytes) {
    if (batch < 0 || !h_bytes) return GNND_ERR_INVALID_ARG;
    if (batch > kOsdGatedMaxBatch) return GNND_ERR_UNSUPPORTED;
    *h_bytes = gnnd_osd_gated_bytes(batch);
    return GNND_OK;
}

extern "C" int gnnd_osd_gated(const gnnd_graph* g, int dtype, const void* d_x, const void* d_pred,
                              const void* d_llr, const int32_t* d_gate, int base, int method,
                              int32_t order, void* d_ehat, int32_t* d_status, int32_t* d_choice,
                              void* d_work, int64_t work_bytes, int64_t batch, void* stream) {
    const int rc = gnnd_args_rc(
        g && batch >= 0 && gnnd_osd_base_ok(base) && gnnd_osd_order_ok(method, order), dtype);
    if (rc != GNND_OK) return rc;
    if (batch == 0) return GNND_OK;
    if (!d_x || !d_pred || !d_gate || !d_ehat || !d_status || !d_work) return GNND_ERR_INVALID_ARG;
    if (batch > kOsdGatedMaxBatch) return GNND_ERR_UNSUPPORTED;
    if (work_bytes < gnnd_osd_gated_bytes(batch)) return GNND_ERR_INVALID_ARG;
    return gnnd_by_dtype(dtype, [&](auto z) {
        return launch_osd_gated<decltype(z)>(g, d_x, d_pred, d_llr, d_gate, base, method, order,
                                             d_ehat, d_status, d_choice, (int32_t*)d_work, batch,
                                             (hipStream_t)stream);
    });
}

extern "C" int gnnd_osd_gated_host(const int64_t* h_var, const int64_t* h_chk, int64_t num_edges,
                                   int32_t num_var, int32_t num_chk, int dtype, const void* h_x,
                                   const void* h_pred, const void* h_llr, const int32_t* h_gate,
                                   int base, int method, int32_t order, void* h_ehat,
                                   int32_t* h_status, int32_t* h_choice, int64_t batch) {
    return gnnd_osd_gated_host_checked(h_var, h_chk, num_edges, num_var, num_chk, dtype, h_x,
                                       h_pred, h_llr, h_gate, base, method, order, h_ehat,
                                       h_status, h_choice, batch);
}

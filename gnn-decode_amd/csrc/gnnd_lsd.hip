// gnnd_lsd.hip — localized-statistics decoding (gnnd_lsd / gnnd_lsd_gated, include/gnnd.h): clusters
// grow around the unsatisfied checks of any Tanner graph and every round solves them by gnnd_osd0's
// Gauss-Jordan restricted to the cluster columns, so the elimination is as large as the error and
// not as the code.  Everything after the column order is integers: every output is bit-reproducible
// and equal to the host mirror's (gnnd_lsd_host.h).
#include "gnnd_common.h"
#include "gnnd_wave_tile.h"
#include "gnnd_lsd_host.h"
#include "gnnd_osd_tile.h"

GNND_DEBUG_TU(lsd)

// ---------------------------------------------------------------------------------------
// The wave-private-tile plan of gnnd_wave_tile.h with the tile and the shared steps of
// gnnd_osd_tile.h.  A wave's tile is the OSD tile and, behind it, all int32:
//   lab[C]      the label of check c: the smallest check index of its cluster; kLsdNone outside inC
//   sel[2][C]   per cluster root: the position in the order of the candidate the cluster picked in
//               this step and in the step before (bits_per_step > 0); sel[0] also holds the
//               invalid-cluster marks after an elimination
// The keys are dead once the order exists: their bytes then hold pos[V] (uint16, the inverse of
// the order) and flag[V] (uint8: bit 0 inV, bit 1 joined in this round), 3 V <= V sizeof(T) bytes.
// A lane keeps its active checks as a 32-bit mask over its rows (bit k: check lane + 64 k).
// Per round:
//   join       bits_per_step == 0: the lanes mark every variable outside inV at their active
//              checks.  k > 0: k steps; in each the lanes fold, by an LDS atomic min per cluster
//              root, the smallest position above the cluster's previous pick over the candidates at
//              their active checks; the root's lane marks order[that position].  A step in which no
//              cluster picks ends the loop.  All stores that two lanes may make to one byte store
//              the same value.
//   closure    lanes stride over the variables: a marked one enters inV and gives every check at
//              it that has none the label of itself.  No variable marked: status 1.
//   labels     the fixed point of label <- min over the checks at a variable of inV (atomic min,
//              order free), repeated until a wave-wide vote finds no lane that lowered one.
//              Clusters only merge, so the labels of the round before are a valid start.
//   eliminate  osd_build_rows, then osd_eliminate_in_play over flag: the pivots of gnnd_osd0
//              with the columns outside inV skipped.
//   validity   an unused row left with s = 1 marks its label invalid; the checks of the invalid
//              clusters are the next round's active checks.  None: e on the pivots, status 0.
// Every loop exit and every branch around a __ballot, a readlane or a wave_tile_sync depends only
// on ballots, on kernel arguments or on values read at one LDS address by the whole wave.
// Why no index leaves its array: a label is kLsdNone or a check index (it starts as the check's own
// and is only replaced by another check's label), and is used as an index only for checks of inC,
// whose label is not kLsdNone; a pick is kLsdNone or the pos of a variable, below V, and is used as
// an index only where it is not kLsdNone.  The debug build checks each of them.
// ---------------------------------------------------------------------------------------
constexpr int kLsdNone = 0x7fffffff;

struct LsdPlan {
    OsdPlan o;                  // the OSD part, at the start of the wave's tile
    int off_lab, off_sel;       // byte offsets inside one wave's tile
    int wave_bytes;             // one wave's tile (16-byte multiple)
    int waves;                  // waves per workgroup (0: the tile does not fit)
};

static LsdPlan lsd_plan(int V, int C, size_t elem) {
    LsdPlan p;
    p.o = osd_plan(V, C, elem);
    const size_t chk = wave_tile_align16((size_t)C * sizeof(int32_t));
    p.off_lab = p.o.wave_bytes;
    p.off_sel = p.off_lab + (int)chk;
    p.wave_bytes = p.off_sel + 2 * (int)chk;      // C <= 2048 where o.waves != 0
    p.waves = p.o.waves != 0 ? wave_tile_waves((size_t)p.wave_bytes) : 0;
    return p;
}

template <typename T>
struct LsdTile {
    OsdTile<T> o;
    uint16_t* pos;
    uint8_t* flag;
    int* lab;
    int* sel;
    __device__ __forceinline__ LsdTile(char* tile, const LsdPlan& pl, int V)
        : o(tile, pl.o), pos((uint16_t*)(tile + pl.o.off_key)),
          flag((uint8_t*)(tile + pl.o.off_key) + 2 * (size_t)V), lab((int*)(tile + pl.off_lab)),
          sel((int*)(tile + pl.off_sel)) {}
};

struct LsdOuts {
    int32_t* status;
    int32_t* rounds;
    int32_t* nclus;
    int32_t* ncols;
};

// sum over the 64 lanes, the same value in every lane
__device__ __forceinline__ int lsd_wave_sum(int v) {
    for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor(v, s);
    return v;
}

// ---- one codeword of gnnd_lsd on the wave's tile ----
template <typename T>
__device__ __forceinline__ void lsd_codeword(const LsdTile<T>& t, const GraphView& g,
                                             const LsdPlan& pl, int hard, int bits,
                                             const T* __restrict__ x, const T* __restrict__ pred,
                                             T* __restrict__ ehat, const LsdOuts& out, int64_t b,
                                             int lane) {
    const int V = g.V, C = g.C, N = g.N, E = g.E;
    (void)E;                                // read by the debug build's index checks only
    const int S = pl.o.stride, syn = pl.o.words, rpl = pl.o.rpl;
    const uint32_t* A = t.o.A;
    const uint16_t* s_order = t.o.order;
    uint8_t* s_e = t.o.e;
    const T* xc = x + b * N + V;
    osd_keys_and_order(t.o, V, hard, pred + b * V, lane);
    wave_tile_sync();                       // every key is read: its bytes are free
    for (int p = lane; p < V; p += 64) {
        const int v = GNND_DIDX((int)s_order[p], V, GNND_DBG_VAR);
        t.pos[v] = (uint16_t)p;
        t.flag[v] = 0;
    }
    // ---- s = t xor H z; inC = s, every unsatisfied check a cluster of its own ----
    uint32_t act = 0;                       // bit k: check lane + 64 k is active
    for (int k = 0; k < rpl; ++k) {
        const int c = lane + 64 * k;
        if (c >= C) break;
        int par = xc[c] < T(0);
        for (int i = g.chk_ptr[c]; i < g.chk_ptr[c + 1]; ++i) {
            const int e = GNND_DIDX(g.chk_edge[GNND_DIDX(i, E, GNND_DBG_SLOT)], E, GNND_DBG_SLOT);
            par ^= s_e[GNND_DIDX((int)(g.edge_vc[e] & 0xffffu), V, GNND_DBG_VAR)];
        }
        t.lab[c] = par ? c : kLsdNone;
        act |= (uint32_t)par << k;
    }
    wave_tile_sync();
    int rounds = 0, status = 0;
    if (__ballot(act != 0) != 0) {
        status = 1;
        while (rounds <= V) {               // every round adds a variable or stops
            ++rounds;
            // ---- join ----
            if (bits == 0) {
                for (int k = 0; k < rpl; ++k) {
                    if (!((act >> k) & 1u)) continue;
                    const int c = lane + 64 * k;
                    for (int i = g.chk_ptr[c]; i < g.chk_ptr[c + 1]; ++i) {
                        const int e = GNND_DIDX(g.chk_edge[GNND_DIDX(i, E, GNND_DBG_SLOT)], E, GNND_DBG_SLOT);
                        const int v = GNND_DIDX((int)(g.edge_vc[e] & 0xffffu), V, GNND_DBG_VAR);
                        if (!(t.flag[v] & 1)) t.flag[v] = 2;
                    }
                }
            } else {
                int* prev = t.sel;
                int* cur = t.sel + C;
                for (int step = 0; step < bits; ++step) {
                    for (int c = lane; c < C; c += 64) cur[c] = kLsdNone;
                    wave_tile_sync();
                    for (int k = 0; k < rpl; ++k) {
                        if (!((act >> k) & 1u)) continue;
                        const int c = lane + 64 * k;
                        const int root = GNND_DIDX(t.lab[c], C, GNND_DBG_NODE);
                        const int above = step ? prev[root] : -1;
                        if (above == kLsdNone) continue;        // the cluster has run out
                        for (int i = g.chk_ptr[c]; i < g.chk_ptr[c + 1]; ++i) {
                            const int e = GNND_DIDX(g.chk_edge[GNND_DIDX(i, E, GNND_DBG_SLOT)], E, GNND_DBG_SLOT);
                            const int v = GNND_DIDX((int)(g.edge_vc[e] & 0xffffu), V, GNND_DBG_VAR);
                            const int p = t.pos[v];
                            if (!(t.flag[v] & 1) && p > above) atomicMin(&cur[root], p);
                        }
                    }
                    wave_tile_sync();
                    int picked = 0;
                    for (int k = 0; k < rpl; ++k) {
                        if (!((act >> k) & 1u)) continue;
                        const int c = lane + 64 * k;
                        const int p = cur[c];
                        if (t.lab[c] != c || p == kLsdNone) continue;
                        t.flag[GNND_DIDX((int)s_order[GNND_DIDX(p, V, GNND_DBG_LDS_POS)], V, GNND_DBG_VAR)] = 2;
                        picked = 1;
                    }
                    int* const sw = prev;
                    prev = cur;
                    cur = sw;
                    if (__ballot(picked) == 0) break;
                }
            }
            wave_tile_sync();
            // ---- closure ----
            int grew = 0;
            for (int v = lane; v < V; v += 64) {
                if (!(t.flag[v] & 2)) continue;
                t.flag[v] = 1;
                grew = 1;
                for (int e = g.var_ptr[v]; e < g.var_ptr[v + 1]; ++e) {
                    const int c = GNND_DIDX((int)(g.edge_vc[GNND_DIDX(e, E, GNND_DBG_SLOT)] >> 16), C, GNND_DBG_NODE);
                    if (t.lab[c] == kLsdNone) t.lab[c] = c;
                }
            }
            if (__ballot(grew) == 0) break;         // a whole component with no solution
            wave_tile_sync();
            // ---- labels ----
            for (;;) {
                int changed = 0;
                for (int v = lane; v < V; v += 64) {
                    if (!(t.flag[v] & 1)) continue;
                    const int e0 = g.var_ptr[v], e1 = g.var_ptr[v + 1];
                    int m = kLsdNone;
                    for (int e = e0; e < e1; ++e) {
                        const int l = t.lab[GNND_DIDX((int)(g.edge_vc[GNND_DIDX(e, E, GNND_DBG_SLOT)] >> 16), C, GNND_DBG_NODE)];
                        m = l < m ? l : m;
                    }
                    for (int e = e0; e < e1; ++e) {
                        int* l = &t.lab[(int)(g.edge_vc[e] >> 16)];
                        if (*l > m) { atomicMin(l, m); changed = 1; }
                    }
                }
                wave_tile_sync();
                if (__ballot(changed) == 0) break;
            }
            // ---- eliminate over the cluster columns ----
            osd_build_rows(t.o, g, pl.o, xc, lane);
            const uint32_t used = osd_eliminate_in_play(t.o, pl.o, t.flag, V, C, lane);
            uint32_t bad = 0;               // bit k: row lane + 64 k is unused and keeps s = 1
            for (int k = 0; k < rpl; ++k) {
                const int r = lane + 64 * k;
                if (r < C && !((used >> k) & 1u)) bad |= (A[(size_t)r * S + syn] & 1u) << k;
            }
            if (__ballot(bad != 0) == 0) {
                for (int k = 0; k < rpl; ++k) {
                    const int r = lane + 64 * k;
                    if (r < C && ((used >> k) & 1u) && (A[(size_t)r * S + syn] & 1u))
                        s_e[GNND_DIDX((int)t.o.piv[r], V, GNND_DBG_VAR)] ^= 1;   // one pivot per column
                }
                status = 0;
                break;
            }
            // ---- the invalid clusters' checks are the next round's active checks ----
            for (int c = lane; c < C; c += 64) t.sel[c] = 0;
            wave_tile_sync();
            for (int k = 0; k < rpl; ++k) {
                if (!((bad >> k) & 1u)) continue;
                const int l = t.lab[lane + 64 * k];      // such a row is a check of inC
                GNND_DCHECK(l != kLsdNone, GNND_DBG_NODE);
                if (l != kLsdNone) t.sel[GNND_DIDX(l, C, GNND_DBG_NODE)] = 1;
            }
            wave_tile_sync();
            act = 0;
            for (int k = 0; k < rpl; ++k) {
                const int c = lane + 64 * k;
                if (c >= C) break;
                const int l = t.lab[c];
                if (l != kLsdNone && t.sel[GNND_DIDX(l, C, GNND_DBG_NODE)]) act |= 1u << k;
            }
            wave_tile_sync();               // the marks are read before the next round's picks
        }
    }
    wave_tile_sync();
    // ---- outputs ----
    T* eb = ehat + b * V;
    int ncols = 0, nclus = 0;
    for (int v = lane; v < V; v += 64) {
        eb[v] = (s_e[v] & 1) ? T(1) : T(0);
        ncols += t.flag[v] & 1;
    }
    for (int c = lane; c < C; c += 64) nclus += t.lab[c] == c;
    ncols = lsd_wave_sum(ncols);
    nclus = lsd_wave_sum(nclus);
    if (lane == 0) {
        if (out.status) out.status[b] = status;
        if (out.rounds) out.rounds[b] = rounds;
        if (out.nclus) out.nclus[b] = nclus;
        if (out.ncols) out.ncols[b] = ncols;
    }
    wave_tile_sync();                        // tile reads done before the next codeword's writes
}

template <typename T>
__global__ void __launch_bounds__(256, 7)
lsd_kernel(GraphView g, LsdPlan pl, int hard, int bits, const T* __restrict__ x,
           const T* __restrict__ pred, T* __restrict__ ehat, LsdOuts out, int64_t B) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const LsdTile<T> t(smem + (size_t)wave * pl.wave_bytes, pl, g.V);
    for (int64_t b = (int64_t)blockIdx.x * pl.waves + wave; b < B;
         b += (int64_t)gridDim.x * pl.waves)
        lsd_codeword(t, g, pl, hard, bits, x, pred, ehat, out, b, lane);
}

// gnnd_lsd_gated's second launch: lsd_kernel's plan and grid (the worst case); wave w takes list
// entries w, w + (waves in flight), ... below the count it reads from the scratch of
// osd_gate_kernel (gnnd_osd_tile.h).  With count 0 every wave leaves at once.
template <typename T>
__global__ void __launch_bounds__(256, 7)
lsd_gated_kernel(GraphView g, LsdPlan pl, int hard, int bits, const T* __restrict__ x,
                 const T* __restrict__ pred, T* __restrict__ ehat, LsdOuts out,
                 const int32_t* __restrict__ work, int64_t B) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const LsdTile<T> t(smem + (size_t)wave * pl.wave_bytes, pl, g.V);
    const int count = GNND_DIDX(work[0], (int)B + 1, GNND_DBG_GRID);    // <= B; the list follows
    // count < 2^31 and at most 8192 waves in flight: the unsigned index cannot wrap; the list
    // entry is the same for the whole wave and stays in scalar registers
    for (unsigned i = blockIdx.x * pl.waves + wave; i < (unsigned)count; i += gridDim.x * pl.waves) {
        const int64_t b = (unsigned)GNND_DIDX(__builtin_amdgcn_readfirstlane(work[1 + (size_t)i]),
                                              (int)B, GNND_DBG_GRID);
        lsd_codeword(t, g, pl, hard, bits, x, pred, ehat, out, b, lane);
    }
}

// the LDS limits of gnnd_lsd for this graph and element size (gnnd_bplsd, gnnd_minsum.hip, asks
// before its first launch)
bool gnnd_lsd_fits(const gnnd_graph* g, size_t elem) {
    return lsd_plan(g->view.V, g->view.C, elem).waves != 0;
}

template <typename T>
static int launch_lsd(const gnnd_graph* g, const void* x, const void* pred, const void* llr,
                      const int32_t* gate, int base, int bits, void* ehat, const LsdOuts& out,
                      int32_t* work, int64_t B, hipStream_t st) {
    const GraphView& v = g->view;
    const LsdPlan pl = lsd_plan(v.V, v.C, sizeof(T));
    if (pl.waves == 0) return GNND_ERR_UNSUPPORTED;
    const unsigned blocks = wave_tile_blocks(B, pl.waves, pl.waves);
    const size_t lds = (size_t)pl.waves * pl.wave_bytes;
    const int hard = base == GNND_OSD_BASE_HARD;
    if (!gate) {
        lsd_kernel<T><<<blocks, 64 * pl.waves, lds, st>>>(v, pl, hard, bits, (const T*)x,
                                                          (const T*)pred, (T*)ehat, out, B);
        GNND_LAUNCH_CHECK();
        return GNND_OK;
    }
    const GateInts ints = {{out.status, out.rounds, out.nclus, out.ncols}, {0, 0, 0, 0}};
    osd_gate_kernel<T><<<osd_gate_blocks(B), kGateThreads, 0, st>>>(
        v.V, gate, (const T*)pred, (const T*)llr, (T*)ehat, ints, work, B);
    GNND_LAUNCH_CHECK();
    lsd_gated_kernel<T><<<blocks, 64 * pl.waves, lds, st>>>(v, pl, hard, bits, (const T*)x,
                                                            (const T*)pred, (T*)ehat, out, work, B);
    GNND_LAUNCH_CHECK();
    return GNND_OK;
}

extern "C" int gnnd_lsd(const gnnd_graph* g, int dtype, const void* d_x, const void* d_pred,
                        int base, int32_t bits_per_step, void* d_ehat, int32_t* d_status,
                        int32_t* d_rounds, int32_t* d_nclus, int32_t* d_ncols, int64_t batch,
                        void* stream) {
    const int rc = gnnd_args_rc(g && batch >= 0 && gnnd_lsd_params_ok(base, bits_per_step), dtype);
    if (rc != GNND_OK) return rc;
    if (batch == 0) return GNND_OK;
    if (!d_x || !d_pred || !d_ehat) return GNND_ERR_INVALID_ARG;
    const LsdOuts out = {d_status, d_rounds, d_nclus, d_ncols};
    return gnnd_by_dtype(dtype, [&](auto z) {
        return launch_lsd<decltype(z)>(g, d_x, d_pred, nullptr, nullptr, base, bits_per_step,
                                       d_ehat, out, nullptr, batch, (hipStream_t)stream);
    });
}

extern "C" int gnnd_lsd_host(const int64_t* h_var, const int64_t* h_chk, int64_t num_edges,
                             int32_t num_var, int32_t num_chk, int dtype, const void* h_x,
                             const void* h_pred, int base, int32_t bits_per_step, void* h_ehat,
                             int32_t* h_status, int32_t* h_rounds, int32_t* h_nclus,
                             int32_t* h_ncols, int64_t batch) {
    return gnnd_lsd_host_checked(h_var, h_chk, num_edges, num_var, num_chk, dtype, h_x, h_pred,
                                 base, bits_per_step, h_ehat, h_status, h_rounds, h_nclus, h_ncols,
                                 batch);
}

extern "C" int gnnd_lsd_gated(const gnnd_graph* g, int dtype, const void* d_x, const void* d_pred,
                              const void* d_llr, const int32_t* d_gate, int base,
                              int32_t bits_per_step, void* d_ehat, int32_t* d_status,
                              int32_t* d_rounds, int32_t* d_nclus, int32_t* d_ncols, void* d_work,
                              int64_t work_bytes, int64_t batch, void* stream) {
    const int rc = gnnd_args_rc(g && batch >= 0 && gnnd_lsd_params_ok(base, bits_per_step), dtype);
    if (rc != GNND_OK) return rc;
    if (batch == 0) return GNND_OK;
    if (!d_x || !d_pred || !d_gate || !d_ehat || !d_work) return GNND_ERR_INVALID_ARG;
    if (batch > kOsdGatedMaxBatch) return GNND_ERR_UNSUPPORTED;
    if (work_bytes < gnnd_osd_gated_bytes(batch)) return GNND_ERR_INVALID_ARG;
    const LsdOuts out = {d_status, d_rounds, d_nclus, d_ncols};
    return gnnd_by_dtype(dtype, [&](auto z) {
        return launch_lsd<decltype(z)>(g, d_x, d_pred, d_llr, d_gate, base, bits_per_step, d_ehat,
                                       out, (int32_t*)d_work, batch, (hipStream_t)stream);
    });
}

extern "C" int gnnd_lsd_gated_host(const int64_t* h_var, const int64_t* h_chk, int64_t num_edges,
                                   int32_t num_var, int32_t num_chk, int dtype, const void* h_x,
                                   const void* h_pred, const void* h_llr, const int32_t* h_gate,
                                   int base, int32_t bits_per_step, void* h_ehat,
                                   int32_t* h_status, int32_t* h_rounds, int32_t* h_nclus,
                                   int32_t* h_ncols, int64_t batch) {
    return gnnd_lsd_gated_host_checked(h_var, h_chk, num_edges, num_var, num_chk, dtype, h_x,
                                       h_pred, h_llr, h_gate, base, bits_per_step, h_ehat, h_status,
                                       h_rounds, h_nclus, h_ncols, batch);
}

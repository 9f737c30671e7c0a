// gnnd_osd.hip — OSD-0 post-processing (gnnd_osd0, include/gnnd.h): turns the decoders' soft
// outputs into an estimate that satisfies the measured syndrome whenever one exists.
#include "gnnd_common.h"
#include "gnnd_osd_host.h"

GNND_DEBUG_TU(osd)

// ---------------------------------------------------------------------------------------
// One wave per codeword, wave-private LDS, no workgroup barrier.  Per codeword:
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
// ---------------------------------------------------------------------------------------
constexpr int kOsdMaxRowsPerLane = 32;      // `used` is one 32-bit mask per lane: C <= 2048
constexpr size_t kOsdLdsLimit = 64 * 1024;  // dynamic LDS of one workgroup without an opt-in

struct OsdPlan {
    int words;        // column words per row, ceil(V / 32)
    int stride;       // words per row in LDS (columns + syndrome word, odd)
    int rpl;          // rows per lane, ceil(C / 64)
    int off_key, off_order, off_piv, off_e;   // byte offsets inside one wave's tile
    int wave_bytes;   // one wave's tile (16-byte multiple)
    int waves;        // waves per workgroup (0: the matrix does not fit)
};

static inline int osd_align16(int n) { return (n + 15) & ~15; }

static OsdPlan osd_plan(int V, int C, size_t elem) {
    OsdPlan p;
    p.words = (V + 31) / 32;
    p.stride = (p.words + 1) | 1;
    p.rpl = (C + 63) / 64;
    const size_t a = (size_t)C * p.stride * 4;
    p.off_key = osd_align16((int)(a > kOsdLdsLimit ? kOsdLdsLimit : a));
    p.off_order = p.off_key + osd_align16(V * (int)elem);
    p.off_piv = p.off_order + osd_align16(V * 2);
    p.off_e = p.off_piv + osd_align16(C * 2);
    p.wave_bytes = p.off_e + osd_align16(V);
    p.waves = 0;
    if (a <= kOsdLdsLimit && (size_t)p.wave_bytes <= kOsdLdsLimit && p.rpl <= kOsdMaxRowsPerLane) {
        const int fit = (int)(kOsdLdsLimit / (size_t)p.wave_bytes);
        p.waves = fit < 4 ? fit : 4;
    }
    return p;
}

__device__ __forceinline__ void osd_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <typename T>
__global__ void __launch_bounds__(256)
osd0_kernel(GraphView g, OsdPlan pl, int hard, const T* __restrict__ x,
            const T* __restrict__ pred, T* __restrict__ ehat, int32_t* __restrict__ status,
            int64_t B) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int V = g.V, C = g.C, N = g.N;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int S = pl.stride, syn = pl.words;
    char* tile = smem + (size_t)wave * pl.wave_bytes;
    uint32_t* A = (uint32_t*)tile;
    T* s_key = (T*)(tile + pl.off_key);
    uint16_t* s_order = (uint16_t*)(tile + pl.off_order);
    uint16_t* s_piv = (uint16_t*)(tile + pl.off_piv);
    uint8_t* s_e = (uint8_t*)(tile + pl.off_e);

    for (int64_t b = (int64_t)blockIdx.x * pl.waves + wave; b < B;
         b += (int64_t)gridDim.x * pl.waves) {
        const T* pb = pred + b * V;
        // ---- base vector and ordering key ----
        for (int v = lane; v < V; v += 64) {
            const T p = pb[v];
            const T d = p - T(0.5);
            const T k = hard ? -g_abs(d) : p;
            s_key[v] = p != p ? -(T)INFINITY : k;
            s_e[v] = (uint8_t)(hard && p > T(0.5));
        }
        osd_wave_sync();
        // ---- column order by counting ----
        for (int v = lane; v < V; v += 64) {
            const T kv = s_key[v];
            int rank = 0;
            for (int u = 0; u < V; ++u) {
                const T ku = s_key[u];
                rank += (ku > kv) | ((ku == kv) & (u < v));
            }
            s_order[GNND_DIDX(rank, V, GNND_DBG_LDS_POS)] = (uint16_t)v;
        }
        // ---- A = H^T rows with the residual syndrome ----
        for (int k = 0; k < pl.rpl; ++k) {
            const int r = lane + 64 * k;
            if (r >= C) break;
            uint32_t* row = A + (size_t)r * S;
            for (int w = 0; w < S; ++w) row[w] = 0;
            int par = x[b * N + V + r] < T(0);
            for (int i = g.chk_ptr[r]; i < g.chk_ptr[r + 1]; ++i) {
                const int e = GNND_DIDX(g.chk_edge[GNND_DIDX(i, g.E, GNND_DBG_SLOT)], g.E, GNND_DBG_SLOT);
                const int v = GNND_DIDX((int)(g.edge_vc[e] & 0xffffu), V, GNND_DBG_VAR);
                row[v >> 5] |= 1u << (v & 31);
                par ^= s_e[v];
            }
            row[syn] = (uint32_t)par;
        }
        osd_wave_sync();
        // ---- Gauss-Jordan over the ordered columns ----
        uint32_t used = 0;                  // bit k: row lane + 64 k is a pivot row
        int rank = 0;
        for (int pos = 0; pos < V && rank < C; ++pos) {
            const int j = GNND_DIDX((int)s_order[pos], V, GNND_DBG_VAR);
            const int wj = j >> 5;
            const uint32_t bj = 1u << (j & 31);
            uint32_t hit = 0;               // bit k: row lane + 64 k holds column j
            int prow = -1;
            for (int k = 0; k < pl.rpl; ++k) {
                const int r = lane + 64 * k;
                const bool has = r < C && (A[(size_t)r * S + wj] & bj);
                hit |= (uint32_t)has << k;
                if (prow < 0) {
                    const unsigned long long m = __ballot(has && !((used >> k) & 1u));
                    if (m) prow = 64 * k + __builtin_ctzll(m);
                }
            }
            if (prow < 0) continue;
            GNND_DCHECK(prow < C, GNND_DBG_NODE);
            if (lane == (prow & 63)) {
                used |= 1u << (prow >> 6);
                hit &= ~(1u << (prow >> 6));
                s_piv[prow] = (uint16_t)j;
            }
            ++rank;
            const uint32_t* prw = A + (size_t)prow * S;
            for (int w = 0; w < S; ++w) {
                const uint32_t pw = __builtin_amdgcn_readfirstlane(prw[w]);
                if (pw == 0) continue;
                for (int k = 0; k < pl.rpl; ++k)
                    if ((hit >> k) & 1u) A[(size_t)(lane + 64 * k) * S + w] ^= pw;
            }
            osd_wave_sync();
        }
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
        osd_wave_sync();
        T* eb = ehat + b * V;
        for (int v = lane; v < V; v += 64) eb[v] = s_e[v] ? T(1) : T(0);
        if (lane == 0) status[b] = fail ? 1 : 0;
        osd_wave_sync();                    // tile reads done before the next codeword's writes
    }
}

template <typename T>
static int launch_osd0(const gnnd_graph* g, const void* x, const void* pred, int base, void* ehat,
                       int32_t* status, int64_t B, hipStream_t st) {
    const GraphView& v = g->view;
    const OsdPlan pl = osd_plan(v.V, v.C, sizeof(T));
    if (pl.waves == 0) return GNND_ERR_UNSUPPORTED;
    const int64_t want = (B + pl.waves - 1) / pl.waves;
    const int64_t cap = 8192 / pl.waves;                  // 32 waves per CU, grid-stride
    const int64_t blocks = want < cap ? want : cap;
    osd0_kernel<T><<<(unsigned)blocks, 64 * pl.waves, (size_t)pl.waves * pl.wave_bytes, st>>>(
        v, pl, base == GNND_OSD_BASE_HARD, (const T*)x, (const T*)pred, (T*)ehat, status, B);
    GNND_LAUNCH_CHECK();
    return GNND_OK;
}

extern "C" int gnnd_osd0(const gnnd_graph* g, int dtype, const void* d_x, const void* d_pred,
                         int base, void* d_ehat, int32_t* d_status, int64_t batch, void* stream) {
    if (!g || batch < 0) return GNND_ERR_INVALID_ARG;
    if (base != GNND_OSD_BASE_ZERO && base != GNND_OSD_BASE_HARD) return GNND_ERR_INVALID_ARG;
    if (dtype == GNND_BF16) return GNND_ERR_UNSUPPORTED;
    if (dtype != GNND_F32 && dtype != GNND_F64) return GNND_ERR_INVALID_ARG;
    if (batch == 0) return GNND_OK;
    if (!d_x || !d_pred || !d_ehat || !d_status) return GNND_ERR_INVALID_ARG;
    hipStream_t st = (hipStream_t)stream;
    if (dtype == GNND_F32)
        return launch_osd0<float>(g, d_x, d_pred, base, d_ehat, d_status, batch, st);
    return launch_osd0<double>(g, d_x, d_pred, base, d_ehat, d_status, batch, st);
}

extern "C" int gnnd_osd0_host(const int64_t* h_var, const int64_t* h_chk, int64_t num_edges,
                              int32_t num_var, int32_t num_chk, int dtype, const void* h_x,
                              const void* h_pred, int base, void* h_ehat, int32_t* h_status,
                              int64_t batch) {
    return gnnd_osd0_host_checked(h_var, h_chk, num_edges, num_var, num_chk, dtype, h_x, h_pred,
                                  base, h_ehat, h_status, batch);
}

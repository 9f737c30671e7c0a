// gnnd_osd_tile.h — the wave tile and the device steps the elimination kernels share (gnnd_osd.hip,
// gnnd_lsd.hip), each written once: the tile plan, the keys and the column order, the rows of H^T
// with the residual syndrome, one column of the Gauss-Jordan, and the gate kernel of the gated
// entries (compaction of the gate into a list, pass-through of the ungated codewords).
// Include it after gnnd_common.h (GNND_DIDX records into the including unit's own debug word) and
// gnnd_wave_tile.h.
//
// A wave's tile:
//   A[C][stride]  bit-packed rows of H^T: ceil(V/32) column words, one syndrome word, padded to an
//                 odd count (lanes own rows lane, lane + 64, ...: a wave's accesses to one word of
//                 64 consecutive rows fall on distinct banks)
//   key[V]        the ordering keys, T
//   order[V]      the columns by descending key, ties by ascending v, uint16
//   piv[C]        the pivot column of a used row, uint16
//   e[V]          bit 0: the base vector z, then the estimate; bit 1: gnnd_osd's pivot-column mark
#pragma once

constexpr int kOsdMaxRowsPerLane = 32;      // `used` is one 32-bit mask per lane: C <= 2048

struct OsdPlan {
    int words;        // column words per row, ceil(V / 32)
    int stride;       // words per row in LDS (columns + syndrome word, odd)
    int rpl;          // rows per lane, ceil(C / 64)
    int off_key, off_order, off_piv, off_e;   // byte offsets inside one wave's tile
    int wave_bytes;   // one wave's tile (16-byte multiple)
    int waves;        // waves per workgroup (0: the matrix does not fit)
};

static OsdPlan osd_plan(int V, int C, size_t elem) {
    OsdPlan p;
    p.words = (V + 31) / 32;
    p.stride = (p.words + 1) | 1;
    p.rpl = (C + 63) / 64;
    const size_t a = (size_t)C * p.stride * 4;
    // V, C <= 65535 and a is clamped to the limit: every offset fits an int
    p.off_key = (int)wave_tile_align16(a > kWaveTileLdsLimit ? kWaveTileLdsLimit : a);
    p.off_order = p.off_key + (int)wave_tile_align16((size_t)V * elem);
    p.off_piv = p.off_order + (int)wave_tile_align16((size_t)V * 2);
    p.off_e = p.off_piv + (int)wave_tile_align16((size_t)C * 2);
    p.wave_bytes = p.off_e + (int)wave_tile_align16((size_t)V);
    p.waves = a <= kWaveTileLdsLimit && p.rpl <= kOsdMaxRowsPerLane
                  ? wave_tile_waves((size_t)p.wave_bytes) : 0;
    return p;
}

// one wave's tile
template <typename T>
struct OsdTile {
    uint32_t* A;
    T* key;
    uint16_t* order;
    uint16_t* piv;
    uint8_t* e;
    __device__ __forceinline__ OsdTile(char* tile, const OsdPlan& pl)
        : A((uint32_t*)tile), key((T*)(tile + pl.off_key)),
          order((uint16_t*)(tile + pl.off_order)), piv((uint16_t*)(tile + pl.off_piv)),
          e((uint8_t*)(tile + pl.off_e)) {}
};

// ---- phase 1: base vector, ordering key, column order by counting ----
template <typename T>
__device__ __forceinline__ void osd_keys_and_order(const OsdTile<T>& t, int V, int hard,
                                                   const T* __restrict__ pb, int lane) {
    for (int v = lane; v < V; v += 64) {
        const T p = pb[v];
        const T d = p - T(0.5);
        const T k = hard ? -g_abs(d) : p;
        t.key[v] = p != p ? -(T)INFINITY : k;
        t.e[v] = (uint8_t)(hard && p > T(0.5));
    }
    wave_tile_sync();
    for (int v = lane; v < V; v += 64) {
        const T kv = t.key[v];
        int rank = 0;
        for (int u = 0; u < V; ++u) {
            const T ku = t.key[u];
            rank += (ku > kv) | ((ku == kv) & (u < v));
        }
        t.order[GNND_DIDX(rank, V, GNND_DBG_LDS_POS)] = (uint16_t)v;
    }
}

// ---- phase 2: A = H^T rows with the residual syndrome ----
template <typename T>
__device__ __forceinline__ void osd_build_rows(const OsdTile<T>& t, const GraphView& g,
                                               const OsdPlan& pl, const T* __restrict__ xchk,
                                               int lane) {
    const int C = g.C, S = pl.stride, syn = pl.words;
    for (int k = 0; k < pl.rpl; ++k) {
        const int r = lane + 64 * k;
        if (r >= C) break;
        uint32_t* row = t.A + (size_t)r * S;
        for (int w = 0; w < S; ++w) row[w] = 0;
        int par = xchk[r] < T(0);
        for (int i = g.chk_ptr[r]; i < g.chk_ptr[r + 1]; ++i) {
            const int e = GNND_DIDX(g.chk_edge[GNND_DIDX(i, g.E, GNND_DBG_SLOT)], g.E, GNND_DBG_SLOT);
            const int v = GNND_DIDX((int)(g.edge_vc[e] & 0xffffu), g.V, GNND_DBG_VAR);
            row[v >> 5] |= 1u << (v & 31);
            par ^= t.e[v];
        }
        row[syn] = (uint32_t)par;
    }
    wave_tile_sync();
}

// ---- phase 3: Gauss-Jordan over the columns in play ----
// One column j: the first unused row holding it is the pivot (one __ballot per row slot), its
// words are broadcast (one LDS address for the wave; all-zero words skipped) and XORed into every
// other row holding the bit.  `used` is the lane's pivot-row mask (bit k: row lane + 64 k).
// Returns whether the column gave a pivot, the same in every lane.
template <typename T>
__device__ __forceinline__ bool osd_pivot_column(const OsdTile<T>& t, const OsdPlan& pl, int C,
                                                 int lane, int j, uint32_t& used) {
    const int S = pl.stride;
    uint32_t* A = t.A;
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
    if (prow < 0) return false;
    GNND_DCHECK(prow < C, GNND_DBG_NODE);
    if (lane == (prow & 63)) {
        used |= 1u << (prow >> 6);
        hit &= ~(1u << (prow >> 6));
        t.piv[prow] = (uint16_t)j;
    }
    const uint32_t* prw = A + (size_t)prow * S;
    for (int w = 0; w < S; ++w) {
        const uint32_t pw = __builtin_amdgcn_readfirstlane(prw[w]);
        if (pw == 0) continue;
        for (int k = 0; k < pl.rpl; ++k)
            if ((hit >> k) & 1u) A[(size_t)(lane + 64 * k) * S + w] ^= pw;
    }
    wave_tile_sync();
    return true;
}

// every column in play, in the column order, until rank C; returns the lane's pivot-row mask
template <typename T>
__device__ __forceinline__ uint32_t osd_eliminate(const OsdTile<T>& t, const OsdPlan& pl, int V,
                                                  int C, int lane) {
    uint32_t used = 0;
    int rank = 0;
    for (int pos = 0; pos < V && rank < C; ++pos) {
        const int j = GNND_DIDX((int)t.order[pos], V, GNND_DBG_VAR);
        if (osd_pivot_column(t, pl, C, lane, j, used)) ++rank;
    }
    return used;
}

// The same walk over the columns v with in_play[v] & 1 only.  Sixty-four positions of the order are
// tested at a time, one per lane; the set bits of the __ballot are visited in ascending position.
template <typename T>
__device__ __forceinline__ uint32_t osd_eliminate_in_play(const OsdTile<T>& t, const OsdPlan& pl,
                                                          const uint8_t* in_play, int V, int C,
                                                          int lane) {
    uint32_t used = 0;
    int rank = 0;
    for (int base = 0; base < V && rank < C; base += 64) {
        const int pos = base + lane;
        int v = 0;
        bool in = false;
        if (pos < V) {
            v = GNND_DIDX((int)t.order[pos], V, GNND_DBG_VAR);
            in = in_play[v] & 1;
        }
        unsigned long long m = __ballot(in);            // wave-uniform: so is the loop below
        while (m != 0 && rank < C) {
            const int l = __builtin_ctzll(m);
            m &= m - 1;
            const int j = __builtin_amdgcn_readlane(v, l);
            if (osd_pivot_column(t, pl, C, lane, j, used)) ++rank;
        }
    }
    return used;
}

// ---------------------------------------------------------------------------------------
// The gate kernel of the gated entries (gnnd_osd_gated, gnnd_lsd_gated).  The host does not know
// how many codewords are gated, so it shares the caller's scratch, int32 count then int32 list[B],
// with the kernel that follows it:
//   workgroup 0 strides over the gate and writes the ascending list of gated codewords and their
//   count: per chunk of 4096 every lane owns four consecutive codewords, one __ballot per item gives
//   the prefix inside the wave, the 16 wave totals cross the workgroup through LDS (two buffers: one
//   barrier per chunk), the running base stays in a register.  No atomics, so no counter to clear.
//   The other workgroups write the pass-through outputs of the ungated codewords, 64 codewords per
//   workgroup step, consecutive lanes on consecutive elements: the hard decision into ehat, and
//   into each per-codeword int32 output of `ints` that is not NULL its pass-through value.
// ---------------------------------------------------------------------------------------
constexpr int kGateThreads = 1024;          // 16 waves
constexpr int kGatePerLane = 4;
constexpr int kGateChunk = kGateThreads * kGatePerLane;
constexpr int kGateRows = 64;               // codewords per pass-through step of a workgroup
constexpr int64_t kGateMaxBlocks = 2048;
constexpr int kGateInts = 4;

struct GateInts {
    int32_t* out[kGateInts];                // [B] each, or NULL
    int32_t value[kGateInts];               // what a pass-through codeword gets
};

template <typename T>
__global__ void __launch_bounds__(kGateThreads)
osd_gate_kernel(int V, const int32_t* __restrict__ gate, const T* __restrict__ pred,
                const T* __restrict__ llr, T* __restrict__ ehat, GateInts ints,
                int32_t* __restrict__ work, int64_t B) {
    if (blockIdx.x == 0) {
        // ---- compaction ----
        __shared__ int s_tot[2][kGateThreads / 64];
        int32_t* list = work + 1;
        const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
        const unsigned long long below = (1ull << lane) - 1;
        int base = 0;                       // gated codewords before the chunk, workgroup-uniform
        int gv[kGatePerLane];               // the chunk's gates, loaded one chunk ahead
#pragma unroll
        for (int j = 0; j < kGatePerLane; ++j) {
            const int64_t b = (int64_t)threadIdx.x * kGatePerLane + j;
            gv[j] = b < B ? gate[b] : 0;
        }
        int buf = 0;
        for (int64_t c0 = 0; c0 < B; c0 += kGateChunk, buf ^= 1) {
            const int64_t b0 = c0 + (int64_t)threadIdx.x * kGatePerLane;
            bool f[kGatePerLane];
#pragma unroll
            for (int j = 0; j < kGatePerLane; ++j) f[j] = gv[j] != 0;
#pragma unroll
            for (int j = 0; j < kGatePerLane; ++j) {
                const int64_t b = b0 + kGateChunk + j;
                gv[j] = b < B ? gate[b] : 0;
            }
            int before = 0, wtot = 0;       // set items of the lower lanes / of the wave
#pragma unroll
            for (int j = 0; j < kGatePerLane; ++j) {
                const unsigned long long m = __ballot(f[j]);
                before += __popcll(m & below);
                wtot += __popcll(m);
            }
            if (lane == 0) s_tot[buf][wave] = wtot;
            __syncthreads();
            int wbase = 0, tot = 0;
            for (int w = 0; w < kGateThreads / 64; ++w) {
                const int n = s_tot[buf][w];
                wbase += w < wave ? n : 0;
                tot += n;
            }
            int pos = base + wbase + before;
#pragma unroll
            for (int j = 0; j < kGatePerLane; ++j)
                if (f[j]) list[GNND_DIDX(pos++, (int)B, GNND_DBG_GRID)] = (int32_t)(b0 + j);
            base += tot;
        }
        if (threadIdx.x == 0) work[0] = base;
        return;
    }
    // ---- pass-through: the hard decision of the ungated codewords ----
    for (int64_t g0 = (int64_t)(blockIdx.x - 1) * kGateRows; g0 < B;
         g0 += (int64_t)(gridDim.x - 1) * kGateRows) {
        const int rows = B - g0 < kGateRows ? (int)(B - g0) : kGateRows;
        const unsigned n = (unsigned)rows * (unsigned)V;
        for (unsigned i = threadIdx.x; i < n; i += kGateThreads) {
            const unsigned r = i / (unsigned)V;
            const int64_t b = g0 + r;
            if (gate[b] != 0) continue;
            const int64_t at = g0 * V + i;
            const bool h = llr ? llr[at] < T(0) : pred[at] > T(0.5);
            ehat[at] = h ? T(1) : T(0);
            if (i == r * (unsigned)V) {
#pragma unroll
                for (int j = 0; j < kGateInts; ++j)
                    if (ints.out[j]) ints.out[j][b] = ints.value[j];
            }
        }
    }
}

// the gate kernel's grid for B codewords
static inline unsigned osd_gate_blocks(int64_t B) {
    const int64_t groups = (B + kGateRows - 1) / kGateRows;
    return 1 + (unsigned)(groups < kGateMaxBlocks ? groups : kGateMaxBlocks);
}

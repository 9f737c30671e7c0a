// gnnd_wave_tile.h — the wave-private-tile plan the BP, OSD and union-find decoders share, and the
// device statement of the min-sum contract's steps (include/gnnd.h), each written once.
// Include it after gnnd_common.h: GNND_DIDX records into the including unit's own debug word.
//
// The plan: one wave per codeword, the codeword's state in a wave-private tile of dynamic LDS, wave
// fences only (no workgroup barrier), a grid-stride loop over codewords.  Every unit keeps its own
// *Plan struct with the byte offsets of its tile; the limit, the alignment, the fence, the
// waves-per-workgroup rule and the grid size are here.
//
// The min-sum steps work on a T* msg tile that holds q_e and r_e in place.  Units that call them
// are built with -ffp-contract=off (a * m - b is two roundings).  The host mirrors state the same
// steps separately (gnnd_minsum_host.h); the GPU tests compare the two.
#pragma once

constexpr size_t kWaveTileLdsLimit = 64 * 1024;   // dynamic LDS of one workgroup without an opt-in

static inline size_t wave_tile_align16(size_t n) { return (n + 15) & ~(size_t)15; }

// waves per workgroup for a wave tile of `bytes`: as many as fit, at most 4; 0: it does not fit
static inline int wave_tile_waves(size_t bytes) {
    if (bytes > kWaveTileLdsLimit) return 0;
    const int fit = (int)(kWaveTileLdsLimit / bytes);
    return fit < 4 ? fit : 4;
}

// grid size for B codewords, per_wg of them per workgroup of `waves` waves
static inline unsigned wave_tile_blocks(int64_t B, int64_t per_wg, int waves) {
    const int64_t want = (B + per_wg - 1) / per_wg;
    const int64_t cap = 8192 / waves;                     // 32 waves per CU, grid-stride
    return (unsigned)(want < cap ? want : cap);
}

// orders a wave's tile writes before its other lanes' reads
__device__ __forceinline__ void wave_tile_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// r = sign * max(a * m - b, 0), negative where neg != 0
template <typename T>
__device__ __forceinline__ T bp_signed_mag(T a, T bt, T m, int neg) {
    const T am = a * m;
    const T d = am - bt;                        // -ffp-contract=off: two roundings
    const T mag = d > T(0) ? d : T(0);
    return neg ? -mag : mag;
}

// Flooding check step of one wave: lanes own checks lane, lane + 64, ...  One walk over chk_edge
// keeps min1, min2, arg-min and the sign parity, a second walk writes r_e over q_e.  Every edge
// belongs to one check, so the two walks of a lane touch only its own edges: no fence between them.
template <typename T>
__device__ __forceinline__ void bp_check_step(const GraphView& g, T* msg, const T* xc, T a, T bt,
                                              int lane) {
    const int C = g.C, E = g.E;
    (void)E;                                // read by the debug build's index checks only
    for (int c = lane; c < C; c += 64) {
        const int i0 = g.chk_ptr[c], i1 = g.chk_ptr[c + 1];
        T min1 = (T)INFINITY, min2 = (T)INFINITY;
        int arg = -1;
        int par = xc[c] < T(0);
        for (int i = i0; i < i1; ++i) {
            const int e = GNND_DIDX(g.chk_edge[GNND_DIDX(i, E, GNND_DBG_SLOT)], E, GNND_DBG_SLOT);
            const T q = msg[e];
            const T aq = g_abs(q);
            par ^= (int)(q < T(0));
            if (aq < min1) { min2 = min1; min1 = aq; arg = e; }
            else if (aq < min2) min2 = aq;
        }
        for (int i = i0; i < i1; ++i) {
            const int e = GNND_DIDX(g.chk_edge[GNND_DIDX(i, E, GNND_DBG_SLOT)], E, GNND_DBG_SLOT);
            const T q = msg[e];
            msg[e] = bp_signed_mag(a, bt, e == arg ? min2 : min1, par ^ (int)(q < T(0)));
        }
    }
}

// msg[e] = value over the edges of variable v
template <typename T>
__device__ __forceinline__ void bp_msg_fill(const GraphView& g, T* msg, int v, T value) {
    const int E = g.E;
    (void)E;
    for (int e = g.var_ptr[v]; e < g.var_ptr[v + 1]; ++e) msg[GNND_DIDX(e, E, GNND_DBG_SLOT)] = value;
}

// Variable update of a variable whose edges are e0 .. e1 - 1 (var_ptr[v], var_ptr[v + 1], read once
// by the caller), in two halves so that the caller stores L_v (and whatever else it keeps per
// variable) between them, where the kernels have always stored it: a store after the second walk
// would let the compiler keep the first walk's loads, which is other device code.
// bp_var_sum returns s = s0 + r_e0 + r_e0+1 + ... in ascending edge order (the contract's order);
// bp_var_extrinsic rewrites msg[e] = s - msg[e].
template <typename T>
__device__ __forceinline__ T bp_var_sum(const GraphView& g, const T* msg, int e0, int e1, T s0) {
    const int E = g.E;
    (void)E;
    T s = s0;
    for (int e = e0; e < e1; ++e) s = s + msg[GNND_DIDX(e, E, GNND_DBG_SLOT)];
    return s;
}

template <typename T>
__device__ __forceinline__ void bp_var_extrinsic(const GraphView& g, T* msg, int e0, int e1, T s) {
    const int E = g.E;
    (void)E;
    for (int e = e0; e < e1; ++e) {
        const int ei = GNND_DIDX(e, E, GNND_DBG_SLOT);
        msg[ei] = s - msg[ei];
    }
}

// Syndrome partial of one lane over checks first, first + stride, ...: 1 where one of them has
// t_c != XOR of (L_v < 0) over its variables.  The caller ballots.
template <typename T>
__device__ __forceinline__ int bp_syndrome_bad(const GraphView& g, const T* L, const T* xc,
                                               int first, int stride) {
    const int V = g.V, C = g.C, E = g.E;
    (void)V;
    (void)E;
    int bad = 0;
    for (int c = first; c < C; c += stride) {
        int par = xc[c] < T(0);
        for (int i = g.chk_ptr[c]; i < g.chk_ptr[c + 1]; ++i) {
            const int e = GNND_DIDX(g.chk_edge[GNND_DIDX(i, E, GNND_DBG_SLOT)], E, GNND_DBG_SLOT);
            const int v = GNND_DIDX((int)(g.edge_vc[e] & 0xffffu), V, GNND_DBG_VAR);
            par ^= (int)(L[v] < T(0));
        }
        bad |= par;
    }
    return bad;
}

// gnnd_uf_tile.h — the wave tile and the device steps the union-find kernels share (gnnd_uf.hip,
// gnnd_ufw.hip), each written once: the tile plan, the set-up of the labels and defects, the cluster
// parities, the label sweep, and the forest / parent-edge / peel / output phases.  The kernels differ
// only in what they keep in the edge array and how it grows, so the steps that read it take the
// "edge is full" predicate: gnnd_uf keeps the half-edges grown (full is 2), gnnd_ufw the length
// that remains (full is 0).
// Include it after gnnd_common.h (GNND_DIDX records into the including unit's own debug word),
// gnnd_wave_tile.h and gnnd_uf_host.h (kGnndUfInf).
//
// A wave's tile, all int32:
//   edge[V]     the kernel's growth state of edge v
//   label[N]    the cluster of vertex u = the highest vertex index in it
//   par[N]      defect[u]; during the peel the XOR of the defects over u's subtree
//   aux[N]      odd[l] while the clusters grow, then depth[u]
//   parent[N]   the parent edge of u; V = none (a root)
// Lanes stride over edges (the growth step, the sweeps, the outputs) and over vertices (the set-up,
// the cluster parities, the peel's levels).  Every write that another lane may also make is an LDS
// atomic whose result does not depend on the order: xor for the parities, max for the labels, min
// for the depths and the parent edges.  The sweeps repeat until a wave-wide vote finds no lane that
// saw an edge out of its fixed point.  All loop exits are wave-uniform.
// Why no index leaves its array: label[u] starts as u and is only ever replaced by another
// vertex's label, so it is a vertex index; aux as depth is 0 at a root and otherwise one more than
// a neighbour's, below N, or kGnndUfInf, and is only compared, never used as an index; parent[u]
// is V or the index of an edge the parent pass itself visited, and is dereferenced only where
// depth[u] >= 1, which the pass that set the depth guarantees a full edge for (the release build
// clamps nothing; the debug build checks every one of these).  The endpoint and virtual-vertex
// tables come from the host builder, which the CPU tests check.
#pragma once

struct UfPlan {
    int off_label, off_par, off_aux, off_parent;    // byte offsets inside one wave's tile (edge at 0)
    int wave_bytes;                                 // one wave's tile (16-byte multiple)
    int waves;                                      // waves per workgroup (0: the tile does not fit)
};

static UfPlan uf_plan(int V, int N) {
    UfPlan p;
    const size_t edge = wave_tile_align16((size_t)V * sizeof(int32_t));
    const size_t node = wave_tile_align16((size_t)N * sizeof(int32_t));
    const size_t bytes = edge + 4 * node;           // V <= 65535, N <= 131070: far below overflow
    p.off_label = (int)edge;
    p.off_par = (int)(edge + node);
    p.off_aux = (int)(edge + 2 * node);
    p.off_parent = (int)(edge + 3 * node);
    p.wave_bytes = (int)bytes;
    p.waves = wave_tile_waves(bytes);
    return p;
}

struct UfTile {
    int *edge, *label, *par, *aux, *parent;
};

__device__ __forceinline__ UfTile uf_tile(char* smem, const UfPlan& pl, int wave) {
    char* tile = smem + (size_t)wave * pl.wave_bytes;
    return {(int*)tile, (int*)(tile + pl.off_label), (int*)(tile + pl.off_par),
            (int*)(tile + pl.off_aux), (int*)(tile + pl.off_parent)};
}

// label[u] = u, defect[u] = t_u; a virtual vertex's defect: the XOR of t over its component's
// checks.  The caller fills the edge array before it calls (the first fence orders both).
template <typename T>
__device__ __forceinline__ void uf_defects(const UfTile& t, const int* __restrict__ cvirt,
                                           const T* __restrict__ xc, int C, int N, int lane) {
    for (int u = lane; u < N; u += 64) {
        t.label[u] = u;
        t.par[u] = u < C ? (int)(xc[u] < T(0)) : 0;
    }
    wave_tile_sync();
    for (int c = lane; c < C; c += 64) {
        const int vv = cvirt[c];
        if (vv >= 0 && t.par[c]) atomicXor(&t.par[GNND_DIDX(vv, N, GNND_DBG_NODE)], 1);
    }
    wave_tile_sync();
}

// odd[l] = XOR of defect[u] over label[u] == l, into aux; wave-uniform: is any cluster odd
__device__ __forceinline__ bool uf_cluster_parities(const UfTile& t, int N, int lane) {
    for (int u = lane; u < N; u += 64) t.aux[u] = 0;
    wave_tile_sync();
    for (int u = lane; u < N; u += 64)
        if (t.par[u]) atomicXor(&t.aux[GNND_DIDX(t.label[u], N, GNND_DBG_NODE)], 1);
    wave_tile_sync();
    int any = 0;
    for (int u = lane; u < N; u += 64) any |= t.aux[u];
    return __ballot(any) != 0;
}

// labels: the fixed point of label <- max over the full edges
template <typename Full>
__device__ __forceinline__ void uf_merge_labels(const UfTile& t, const int* __restrict__ ends,
                                                int V, int N, int lane, Full full) {
    (void)N;                                // read by the debug build's index checks only
    for (;;) {
        int changed = 0;
        for (int v = lane; v < V; v += 64) {
            if (!full(t.edge[v])) continue;
            const int a = GNND_DIDX(ends[2 * v], N, GNND_DBG_NODE);
            const int bb = GNND_DIDX(ends[2 * v + 1], N, GNND_DBG_NODE);
            const int la = t.label[a], lb = t.label[bb];
            if (la == lb) continue;
            atomicMax(la < lb ? &t.label[a] : &t.label[bb], la < lb ? lb : la);
            changed = 1;
        }
        wave_tile_sync();
        if (__ballot(changed) == 0) break;
    }
}

// Forest, parent edges, peel and ehat of one codeword, once growth has ended; returns the number
// of full edges (wave-uniform).  ehat is the codeword's row.  The caller fences before it writes
// the tile again.
template <typename T, typename Full>
__device__ __forceinline__ int uf_forest_peel(const UfTile& t, const int* __restrict__ ends, int V,
                                              int N, int lane, Full full, T* __restrict__ ehat) {
    // ---- forest: depth[u] = BFS distance from the label vertex over the full edges ----
    wave_tile_sync();                                     // the odd[] reads are done
    for (int u = lane; u < N; u += 64) {
        t.aux[u] = t.label[u] == u ? 0 : kGnndUfInf;
        t.parent[u] = V;
    }
    wave_tile_sync();
    for (;;) {
        int changed = 0;
        for (int v = lane; v < V; v += 64) {
            if (!full(t.edge[v])) continue;
            const int a = GNND_DIDX(ends[2 * v], N, GNND_DBG_NODE);
            const int bb = GNND_DIDX(ends[2 * v + 1], N, GNND_DBG_NODE);
            const int da = t.aux[a], db = t.aux[bb];
            if (da + 1 < db) { atomicMin(&t.aux[bb], da + 1); changed = 1; }
            if (db + 1 < da) { atomicMin(&t.aux[a], db + 1); changed = 1; }
        }
        wave_tile_sync();
        if (__ballot(changed) == 0) break;
    }
    // ---- parent edge: the lowest full edge to a vertex one level up; nfull; the deepest level ----
    int nfull = 0, maxd = 0;
    for (int v = lane; v < V; v += 64) {
        if (!full(t.edge[v])) continue;
        ++nfull;
        const int a = GNND_DIDX(ends[2 * v], N, GNND_DBG_NODE);
        const int bb = GNND_DIDX(ends[2 * v + 1], N, GNND_DBG_NODE);
        const int da = t.aux[a], db = t.aux[bb];
        if (da + 1 == db) atomicMin(&t.parent[bb], v);
        if (db + 1 == da) atomicMin(&t.parent[a], v);
    }
    for (int u = lane; u < N; u += 64) {
        const int d = t.aux[u];
        GNND_DCHECK(d < N, GNND_DBG_GRID);              // every vertex was reached from its root
        maxd = d > maxd ? d : maxd;
    }
    for (int s = 32; s >= 1; s >>= 1) {
        nfull += __shfl_xor(nfull, s);
        const int o = __shfl_xor(maxd, s);
        maxd = o > maxd ? o : maxd;
    }
    maxd = maxd < N ? maxd : N - 1;                     // a depth is below N: bounds the loop
    wave_tile_sync();
    // ---- peel: subtree parities, the deepest level first ----
    for (int d = maxd; d >= 1; --d) {
        for (int u = lane; u < N; u += 64) {
            if (t.aux[u] != d || !t.par[u]) continue;
            const int e = GNND_DIDX(t.parent[u], V, GNND_DBG_SLOT);
            const int a = ends[2 * e], bb = ends[2 * e + 1];
            atomicXor(&t.par[GNND_DIDX(a == u ? bb : a, N, GNND_DBG_NODE)], 1);
        }
        wave_tile_sync();
    }
    // ---- outputs: edge v is set where it is the parent edge of an end with an odd subtree ----
    for (int v = lane; v < V; v += 64) {
        int h = 0;
        if (full(t.edge[v])) {
            const int a = GNND_DIDX(ends[2 * v], N, GNND_DBG_NODE);
            const int bb = GNND_DIDX(ends[2 * v + 1], N, GNND_DBG_NODE);
            h = t.parent[a] == v ? t.par[a] : t.parent[bb] == v ? t.par[bb] : 0;
        }
        ehat[v] = h ? T(1) : T(0);
    }
    return nfull;
}

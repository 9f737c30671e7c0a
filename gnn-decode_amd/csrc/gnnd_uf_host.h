// gnnd_uf_host.h — host mirror of gnnd_uf (include/gnnd.h): the union-find decoder of a matchable
// Tanner graph (grow clusters around the defects, merge them, peel a spanning forest), and the rule
// that turns the Tanner graph into its decoding graph (gnnd_graph_matching), in plain C++.  No HIP
// types: a plain host compiler builds it, so a stand-alone program can run it under host sanitizers
// (tools/uf_host_check.cpp).  Same definition as the kernel in gnnd_uf.hip, bit for bit in every
// output: integers only, each step either an XOR (order free) or the unique fixed point of a
// monotone sweep (label <- max, depth <- min, parent <- min), so the sweep order cannot show.
#pragma once
#include <stdint.h>
#include <vector>
#include "gnnd_host_args.h"

constexpr int kGnndUfInf = 0x3fffffff;      // depth of a vertex no sweep has reached yet

// The decoding graph: vertices 0 .. C-1 the checks, C .. N-1 the virtual vertices; edge v joins
// ends[2 v] < ends[2 v + 1]; cvirt[c] the virtual vertex of check c's component, -1 where it has none.
struct GnndUfGraph {
    int V = 0, C = 0, N = 0;
    std::vector<int> ends, cvirt;
};

// From the edge list gnnd_graph_create takes, with its checks (more than 65535 edges / variables /
// checks GNND_ERR_UNSUPPORTED, an id out of range or a list not sorted by (v, c) GNND_ERR_GRAPH);
// a variable of degree 0 or above 2 is GNND_ERR_UNSUPPORTED: the graph is not matchable.
inline int gnnd_uf_graph_build(const int64_t* h_var, const int64_t* h_chk, int64_t num_edges,
                               int V, int C, GnndUfGraph& ug) {
    if (num_edges > 65535 || V > 65535 || C > 65535) return GNND_ERR_UNSUPPORTED;
    const int E = (int)num_edges;
    std::vector<int> c0(V, -1), c1(V, -1);
    bool matchable = true;
    for (int e = 0; e < E; ++e) {
        const int64_t v = h_var[e], c = h_chk[e];
        if (v < 0 || v >= V || c < 0 || c >= C) return GNND_ERR_GRAPH;
        if (e > 0 && (v < h_var[e - 1] || (v == h_var[e - 1] && c <= h_chk[e - 1])))
            return GNND_ERR_GRAPH;                                   // sorted by (v, c), no duplicate
        if (c0[v] < 0) c0[v] = (int)c;
        else if (c1[v] < 0) c1[v] = (int)c;                          // c0 < c1 by the sort
        else matchable = false;
    }
    for (int v = 0; v < V; ++v) matchable = matchable && c0[v] >= 0;
    if (!matchable) return GNND_ERR_UNSUPPORTED;
    // components of the checks; a component's root is its lowest check
    std::vector<int> root(C);
    for (int c = 0; c < C; ++c) root[c] = c;
    auto find = [&](int c) {
        while (root[c] != c) c = root[c] = root[root[c]];
        return c;
    };
    for (int v = 0; v < V; ++v) {
        if (c1[v] < 0) continue;
        const int a = find(c0[v]), b = find(c1[v]);
        if (a != b) root[a < b ? b : a] = a < b ? a : b;
    }
    std::vector<int> virt(C, -1);                // by root: -2 = wants a virtual vertex
    for (int v = 0; v < V; ++v)
        if (c1[v] < 0) virt[find(c0[v])] = -2;
    int N = C;
    for (int c = 0; c < C; ++c)                  // ascending roots = ascending lowest check
        if (virt[c] == -2) virt[c] = N++;
    ug.V = V; ug.C = C; ug.N = N;
    ug.cvirt.assign(C, -1);
    for (int c = 0; c < C; ++c) ug.cvirt[c] = virt[find(c)];
    ug.ends.assign(2 * (size_t)V, 0);
    for (int v = 0; v < V; ++v) {
        ug.ends[2 * v] = c0[v];
        ug.ends[2 * v + 1] = c1[v] >= 0 ? c1[v] : ug.cvirt[c0[v]];
    }
    return GNND_OK;
}

inline int gnnd_graph_matching_host_checked(const int64_t* h_var, const int64_t* h_chk,
                                            int64_t num_edges, int32_t V, int32_t C,
                                            int32_t* h_nvert, int32_t* h_endpoints) {
    if (!h_var || !h_chk || num_edges <= 0 || V <= 0 || C <= 0 || !h_nvert)
        return GNND_ERR_INVALID_ARG;
    GnndUfGraph ug;
    const int rc = gnnd_uf_graph_build(h_var, h_chk, num_edges, V, C, ug);
    if (rc != GNND_OK) return rc;
    *h_nvert = ug.N;
    if (h_endpoints)
        for (int i = 0; i < 2 * V; ++i) h_endpoints[i] = ug.ends[i];
    return GNND_OK;
}

// grow [V] is the decoder's own growth state of an edge (gnnd_uf: the half-edges grown, full is 2;
// gnnd_ufw: the length that remains, full is 0): the shared steps read it through a predicate
struct GnndUfState {
    std::vector<int> grow, label, par, odd, depth, parent;
};

// label[u] = u, defect[u] = t_u, a virtual vertex's defect the XOR of t over its component's
// checks; sizes the state.  The caller fills s.grow.
inline void gnnd_uf_setup(const GnndUfGraph& ug, const unsigned char* t, GnndUfState& s) {
    const int C = ug.C, N = ug.N;
    s.label.resize(N);
    s.par.assign(N, 0);
    s.odd.resize(N);
    s.depth.resize(N);
    s.parent.resize(N);
    for (int u = 0; u < N; ++u) s.label[u] = u;
    for (int c = 0; c < C; ++c) {
        s.par[c] = t[c];
        if (t[c] && ug.cvirt[c] >= 0) s.par[ug.cvirt[c]] ^= 1;
    }
}

// odd[l] = XOR of defect[u] over label[u] == l; is any cluster odd
inline bool gnnd_uf_cluster_parities(const GnndUfGraph& ug, GnndUfState& s) {
    const int N = ug.N;
    for (int u = 0; u < N; ++u) s.odd[u] = 0;
    for (int u = 0; u < N; ++u) s.odd[s.label[u]] ^= s.par[u];
    bool any = false;
    for (int u = 0; u < N; ++u) any = any || s.odd[u];
    return any;
}

// labels: the fixed point of label <- max over the full edges; full(s.grow[v]) says which they are
template <typename Full>
void gnnd_uf_merge_labels(const GnndUfGraph& ug, GnndUfState& s, Full full) {
    const int* ends = ug.ends.data();
    for (bool changed = true; changed;) {
        changed = false;
        for (int v = 0; v < ug.V; ++v) {
            if (!full(s.grow[v])) continue;
            const int a = ends[2 * v], b = ends[2 * v + 1];
            if (s.label[a] == s.label[b]) continue;
            s.label[a] = s.label[b] = s.label[a] > s.label[b] ? s.label[a] : s.label[b];
            changed = true;
        }
    }
}

// Once growth has ended: the forest (BFS depth from the label vertex, the lowest full edge one
// level up as the parent), the peel and ehat01 [V]; returns the number of full edges.
template <typename Full>
int gnnd_uf_forest_peel(const GnndUfGraph& ug, GnndUfState& s, Full full, unsigned char* ehat01) {
    const int V = ug.V, N = ug.N;
    const int* ends = ug.ends.data();
    std::vector<int>&grow = s.grow, &label = s.label, &par = s.par;
    std::vector<int>&depth = s.depth, &parent = s.parent;
    for (int u = 0; u < N; ++u) {
        depth[u] = label[u] == u ? 0 : kGnndUfInf;
        parent[u] = V;
    }
    for (bool changed = true; changed;) {
        changed = false;
        for (int v = 0; v < V; ++v) {
            if (!full(grow[v])) continue;
            const int a = ends[2 * v], b = ends[2 * v + 1];
            if (depth[a] + 1 < depth[b]) { depth[b] = depth[a] + 1; changed = true; }
            if (depth[b] + 1 < depth[a]) { depth[a] = depth[b] + 1; changed = true; }
        }
    }
    int nfull = 0, maxd = 0;
    for (int v = 0; v < V; ++v) {
        if (!full(grow[v])) continue;
        ++nfull;
        const int a = ends[2 * v], b = ends[2 * v + 1];
        if (depth[a] + 1 == depth[b] && v < parent[b]) parent[b] = v;
        if (depth[b] + 1 == depth[a] && v < parent[a]) parent[a] = v;
    }
    for (int u = 0; u < N; ++u) maxd = depth[u] > maxd ? depth[u] : maxd;
    // peel: the subtree parities, deepest level first
    for (int d = maxd; d >= 1; --d)
        for (int u = 0; u < N; ++u) {
            if (depth[u] != d) continue;
            const int e = parent[u];
            const int w = ends[2 * e] == u ? ends[2 * e + 1] : ends[2 * e];
            par[w] ^= par[u];
        }
    for (int v = 0; v < V; ++v) {
        const int a = ends[2 * v], b = ends[2 * v + 1];
        int h = 0;
        if (full(grow[v])) h = parent[a] == v ? par[a] : parent[b] == v ? par[b] : 0;
        ehat01[v] = (unsigned char)h;
    }
    return nfull;
}

// One codeword: t [C] the syndrome bits -> ehat01 [V], and rounds / status / nfull.
inline void gnnd_uf_decode_one(const GnndUfGraph& ug, const unsigned char* t, GnndUfState& s,
                               unsigned char* ehat01, int32_t* rounds_out, int32_t* status_out,
                               int32_t* nfull_out) {
    const int V = ug.V;
    const int* ends = ug.ends.data();
    const auto full = [](int g) { return g == 2; };
    s.grow.assign(V, 0);
    gnnd_uf_setup(ug, t, s);
    std::vector<int>&grow = s.grow, &label = s.label, &odd = s.odd;
    int rounds = 0, status = 0;
    while (gnnd_uf_cluster_parities(ug, s)) {
        bool grew = false;
        for (int v = 0; v < V; ++v) {
            const int g = grow[v] + odd[label[ends[2 * v]]] + odd[label[ends[2 * v + 1]]];
            const int ng = g < 2 ? g : 2;
            grew = grew || ng != grow[v];
            grow[v] = ng;
        }
        if (!grew) { status = 1; break; }        // an odd cluster that is a whole component
        ++rounds;
        gnnd_uf_merge_labels(ug, s, full);
    }
    *nfull_out = gnnd_uf_forest_peel(ug, s, full, ehat01);
    *rounds_out = rounds;
    *status_out = status;
}

// every output but ehat may be null; gate may be null
template <typename T>
int gnnd_uf_host_impl(const GnndUfGraph& ug, const T* x, const int32_t* gate, T* ehat,
                      int32_t* rounds_out, int32_t* status_out, int32_t* nfull_out, int64_t batch) {
    const int V = ug.V, C = ug.C;
    GnndUfState s;
    std::vector<unsigned char> t(C), h(V);
    for (int64_t b = 0; b < batch; ++b) {
        if (gate && gate[b] == 0) continue;
        const T* xc = x + b * (int64_t)(V + C) + V;
        for (int c = 0; c < C; ++c) t[c] = xc[c] < T(0);
        int32_t rounds, status, nfull;
        gnnd_uf_decode_one(ug, t.data(), s, h.data(), &rounds, &status, &nfull);
        for (int v = 0; v < V; ++v) ehat[b * V + v] = h[v] ? T(1) : T(0);
        if (rounds_out) rounds_out[b] = rounds;
        if (status_out) status_out[b] = status;
        if (nfull_out) nfull_out[b] = nfull;
    }
    return GNND_OK;
}

inline int gnnd_uf_host_checked(const int64_t* h_var, const int64_t* h_chk, int64_t num_edges,
                                int32_t num_var, int32_t num_chk, int dtype, const void* h_x,
                                const int32_t* h_gate, void* h_ehat, int32_t* h_rounds,
                                int32_t* h_status, int32_t* h_nfull, int64_t batch) {
    const int arc = gnnd_args_rc(
        gnnd_host_list_ok(h_var, h_chk, num_edges, num_var, num_chk, batch), dtype);
    if (arc != GNND_OK) return arc;
    if (batch == 0) return GNND_OK;
    if (!h_x || !h_ehat) return GNND_ERR_INVALID_ARG;
    GnndUfGraph ug;
    const int rc = gnnd_uf_graph_build(h_var, h_chk, num_edges, num_var, num_chk, ug);
    if (rc != GNND_OK) return rc;
    return gnnd_by_dtype(dtype, [&](auto z) {
        using T = decltype(z);
        return gnnd_uf_host_impl<T>(ug, (const T*)h_x, h_gate, (T*)h_ehat, h_rounds, h_status,
                                    h_nfull, batch);
    });
}

// gnnd_ufw_host.h — host mirrors of gnnd_ufw and gnnd_belief_find (include/gnnd.h): the union-find
// decoder of gnnd_uf_host.h with weighted growth (an edge's length is its quantised reliability, and
// growth jumps from one filled edge to the next), and min-sum followed by it on the codewords
// min-sum left unsolved.  Plain C++, no HIP types (tools/ufw_host_check.cpp builds it with a host
// compiler).  The set-up, cluster parities, label sweep, forest and peel are gnnd_uf_host.h's; the
// edge state they read is the length that remains, full is 0.  The weight is one multiply and two
// compares in T; everything after it is integers, so every output is the kernel's bits
// (gnnd_ufw.hip).  Build the unit that uses gnnd_belief_find_host_checked with -ffp-contract=off
// (the min-sum contract).
#pragma once
#include <cmath>
#include "gnnd_uf_host.h"
#include "gnnd_minsum_host.h"

constexpr int32_t kGnndUfwMaxWeight = 1024;     // rounds <= 2 wmax V stays inside int32

inline bool gnnd_ufw_params_ok(double scale, int32_t wmax, int32_t passthrough) {
    return std::isfinite(scale) && scale >= 0 && wmax >= 1 && wmax <= kGnndUfwMaxWeight &&
           (passthrough == 0 || passthrough == 1);
}

// w = wmax where r s >= wmax - 1, 1 + (int)(r s) where r s > 0, else 1 (a NaN compares false)
template <typename T>
inline int gnnd_ufw_weight(T r, T s, int wmax) {
    const T m = r * s;
    if (m >= (T)(wmax - 1)) return wmax;
    return m > T(0) ? 1 + (int)m : 1;
}

// One codeword: t [C] the syndrome bits, rem [V] = 2 w_v in s.grow -> ehat01 [V] and the counters.
inline void gnnd_ufw_decode_one(const GnndUfGraph& ug, const unsigned char* t, GnndUfState& s,
                                unsigned char* ehat01, int32_t* rounds_out, int32_t* status_out,
                                int32_t* nfull_out, int32_t* events_out) {
    const int V = ug.V;
    const int* ends = ug.ends.data();
    const auto full = [](int rem) { return rem == 0; };
    gnnd_uf_setup(ug, t, s);
    std::vector<int>&rem = s.grow, &label = s.label, &odd = s.odd;
    int rounds = 0, status = 0, events = 0;
    while (gnnd_uf_cluster_parities(ug, s)) {
        int d = 0x7fffffff;                      // the steps until the first active edge fills
        for (int v = 0; v < V; ++v) {
            const int rate = odd[label[ends[2 * v]]] + odd[label[ends[2 * v + 1]]];
            if (rate == 0 || rem[v] == 0) continue;
            const int need = (rem[v] + rate - 1) / rate;
            d = need < d ? need : d;
        }
        if (d == 0x7fffffff) { status = 1; break; }     // an odd cluster that is a whole component
        for (int v = 0; v < V; ++v) {
            const int rate = odd[label[ends[2 * v]]] + odd[label[ends[2 * v + 1]]];
            const int left = rem[v] - rate * d;
            rem[v] = left > 0 ? left : 0;
        }
        rounds += d;
        ++events;
        gnnd_uf_merge_labels(ug, s, full);
    }
    *nfull_out = gnnd_uf_forest_peel(ug, s, full, ehat01);
    *rounds_out = rounds;
    *status_out = status;
    *events_out = events;
}

// every output but ehat may be null; gate and llr may be null (passthrough needs both)
template <typename T>
int gnnd_ufw_host_impl(const GnndUfGraph& ug, const T* x, const T* llr, double scale, int wmax,
                       const int32_t* gate, int passthrough, T* ehat, int32_t* rounds_out,
                       int32_t* status_out, int32_t* nfull_out, int32_t* events_out,
                       int64_t batch) {
    const int V = ug.V, C = ug.C;
    const T sc = (T)scale;
    GnndUfState s;
    std::vector<unsigned char> t(C), h(V);
    for (int64_t b = 0; b < batch; ++b) {
        int32_t rounds = 0, status = 0, nfull = 0, events = 0;
        if (gate && gate[b] == 0) {
            if (!passthrough) continue;
            for (int v = 0; v < V; ++v) ehat[b * V + v] = llr[b * V + v] < T(0) ? T(1) : T(0);
        } else {
            const T* xv = x + b * (int64_t)(V + C);
            const T* r = llr ? llr + b * (int64_t)V : xv;
            for (int c = 0; c < C; ++c) t[c] = xv[V + c] < T(0);
            s.grow.resize(V);
            for (int v = 0; v < V; ++v) s.grow[v] = 2 * gnnd_ufw_weight(r[v], sc, wmax);
            gnnd_ufw_decode_one(ug, t.data(), s, h.data(), &rounds, &status, &nfull, &events);
            for (int v = 0; v < V; ++v) ehat[b * V + v] = h[v] ? T(1) : T(0);
        }
        if (rounds_out) rounds_out[b] = rounds;
        if (status_out) status_out[b] = status;
        if (nfull_out) nfull_out[b] = nfull;
        if (events_out) events_out[b] = events;
    }
    return GNND_OK;
}

inline int gnnd_ufw_host_checked(const int64_t* h_var, const int64_t* h_chk, int64_t num_edges,
                                 int32_t num_var, int32_t num_chk, int dtype, const void* h_x,
                                 const void* h_llr, double scale, int32_t wmax,
                                 const int32_t* h_gate, int32_t passthrough, void* h_ehat,
                                 int32_t* h_rounds, int32_t* h_status, int32_t* h_nfull,
                                 int32_t* h_events, int64_t batch) {
    const int arc = gnnd_args_rc(
        gnnd_host_list_ok(h_var, h_chk, num_edges, num_var, num_chk, batch) &&
            gnnd_ufw_params_ok(scale, wmax, passthrough) &&
            (passthrough == 0 || (h_gate && h_llr)),
        dtype);
    if (arc != GNND_OK) return arc;
    if (batch == 0) return GNND_OK;
    if (!h_x || !h_ehat) return GNND_ERR_INVALID_ARG;
    GnndUfGraph ug;
    const int rc = gnnd_uf_graph_build(h_var, h_chk, num_edges, num_var, num_chk, ug);
    if (rc != GNND_OK) return rc;
    return gnnd_by_dtype(dtype, [&](auto z) {
        using T = decltype(z);
        return gnnd_ufw_host_impl<T>(ug, (const T*)h_x, (const T*)h_llr, scale, wmax, h_gate,
                                     passthrough, (T*)h_ehat, h_rounds, h_status, h_nfull,
                                     h_events, batch);
    });
}

// gnnd_minsum_host (with the kernel's fp64 exponential for the soft output, as gnnd_bposd_host),
// then gnnd_ufw_host on the min-sum posteriors, gated by the min-sum status, passing through
inline int gnnd_belief_find_host_checked(const int64_t* h_var, const int64_t* h_chk,
                                         int64_t num_edges, int32_t num_var, int32_t num_chk,
                                         int dtype, const void* h_x, double alpha, double beta,
                                         int32_t iters, int32_t early_stop, double scale,
                                         int32_t wmax, void* h_pred, void* h_llr, int32_t* h_iters,
                                         int32_t* h_bp_status, void* h_ehat, int32_t* h_status,
                                         int32_t* h_rounds, int32_t* h_nfull, int32_t* h_events,
                                         int64_t batch) {
    const int rc = gnnd_args_rc(
        gnnd_host_list_ok(h_var, h_chk, num_edges, num_var, num_chk, batch) &&
            gnnd_minsum_params_ok(alpha, beta, iters, early_stop) &&
            gnnd_ufw_params_ok(scale, wmax, 1),
        dtype);
    if (rc != GNND_OK) return rc;
    if (batch == 0) return GNND_OK;
    if (!h_x || !h_pred || !h_llr || !h_bp_status || !h_ehat) return GNND_ERR_INVALID_ARG;
    GnndUfGraph ug;                              // the second stage's refusals, before the first runs
    const int urc = gnnd_uf_graph_build(h_var, h_chk, num_edges, num_var, num_chk, ug);
    if (urc != GNND_OK) return urc;
    const int st = gnnd_minsum_host_checked(h_var, h_chk, num_edges, num_var, num_chk, dtype, h_x,
                                            alpha, beta, iters, early_stop, h_pred, h_llr, h_iters,
                                            h_bp_status, batch, /*device_exp=*/true);
    if (st != GNND_OK) return st;
    return gnnd_ufw_host_checked(h_var, h_chk, num_edges, num_var, num_chk, dtype, h_x, h_llr,
                                 scale, wmax, h_bp_status, 1, h_ehat, h_rounds, h_status, h_nfull,
                                 h_events, batch);
}

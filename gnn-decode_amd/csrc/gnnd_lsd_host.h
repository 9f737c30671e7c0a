// gnnd_lsd_host.h — host mirrors of gnnd_lsd, gnnd_lsd_gated and gnnd_bplsd (include/gnnd.h):
// localized-statistics decoding in plain C++.  Clusters grow around the unsatisfied checks and each
// round solves them by gnnd_osd0's Gauss-Jordan restricted to the cluster columns.  No HIP types: a
// plain host compiler builds it, so a stand-alone program can run it under host sanitizers
// (tools/lsd_host_check.cpp).  Same definition as the kernel in gnnd_lsd.hip, bit for bit; the
// mirror rebuilds and eliminates the whole matrix every round, as the definition is written.
// Build a translation unit that calls gnnd_bplsd_host_checked with -ffp-contract=off (the min-sum
// contract).
#pragma once
#include "gnnd_minsum_host.h"
#include "gnnd_osd_host.h"

inline bool gnnd_lsd_params_ok(int base, int32_t bits_per_step) {
    return gnnd_osd_base_ok(base) && bits_per_step >= 0;
}

// status, rounds, nclus and ncols may each be null
template <typename T>
int gnnd_lsd_host_impl(const int64_t* h_var, const int64_t* h_chk, int64_t num_edges, int V, int C,
                       const T* x, const T* pred, int base, int bits, T* ehat, int32_t* status,
                       int32_t* rounds_out, int32_t* nclus, int32_t* ncols, int64_t batch) {
    for (int64_t e = 0; e < num_edges; ++e)
        if (h_var[e] < 0 || h_var[e] >= V || h_chk[e] < 0 || h_chk[e] >= C) return GNND_ERR_GRAPH;
    // both adjacencies; rows of H^T, bit-packed: words [0, W) hold the V columns, bit V the syndrome
    std::vector<std::vector<int>> vars_of(C), chks_of(V);
    const int W = V / 64 + 1;
    std::vector<uint64_t> A0((size_t)C * W, 0), A;
    for (int64_t e = 0; e < num_edges; ++e) {
        vars_of[h_chk[e]].push_back((int)h_var[e]);
        chks_of[h_var[e]].push_back((int)h_chk[e]);
        A0[(size_t)h_chk[e] * W + (h_var[e] >> 6)] |= (uint64_t)1 << (h_var[e] & 63);
    }
    const int N = V + C;
    const int none = C;                       // the label of a check outside every cluster
    std::vector<T> key(V);
    std::vector<int> order(V), pos(V), piv_col(C), label(C), cand;
    std::vector<uint8_t> z(V), s0(C), inV(V), joined(V), active(C), used(C), invalid(C), seen(V);
    for (int64_t b = 0; b < batch; ++b) {
        const T* p = pred + b * V;
        const T* xc = x + b * N + V;
        T* eb = ehat + b * V;
        for (int v = 0; v < V; ++v) {
            const T pv = p[v];
            const bool nan = pv != pv;
            z[v] = base == GNND_OSD_BASE_HARD && pv > T(0.5);
            const T d = pv - T(0.5);
            const T k = base == GNND_OSD_BASE_HARD ? -(d < T(0) ? -d : d) : pv;
            key[v] = nan ? -std::numeric_limits<T>::infinity() : k;
            order[v] = v;
            inV[v] = 0;
        }
        std::stable_sort(order.begin(), order.end(),
                         [&](int a, int c) { return key[a] > key[c]; });
        for (int i = 0; i < V; ++i) pos[order[i]] = i;
        int any = 0;
        for (int c = 0; c < C; ++c) {            // residual s = t xor H^T z; inC = s
            int par = xc[c] < T(0);
            for (int v : vars_of[c]) par ^= z[v];
            s0[c] = (uint8_t)par;
            label[c] = par ? c : none;
            active[c] = (uint8_t)par;
            any |= par;
        }
        int st = 0, rounds = 0;
        if (any) {
            st = 1;
            while (rounds <= V) {                // every round adds a variable or stops
                ++rounds;
                // ---- join ----
                std::fill(joined.begin(), joined.end(), 0);
                int grew = 0;
                if (bits == 0) {
                    for (int c = 0; c < C; ++c)
                        if (active[c])
                            for (int v : vars_of[c])
                                if (!inV[v]) joined[v] = 1, grew = 1;
                } else {
                    for (int root = 0; root < C; ++root) {
                        if (!active[root] || label[root] != root) continue;
                        cand.clear();
                        for (int c = root; c < C; ++c)
                            if (label[c] == root)
                                for (int v : vars_of[c])
                                    if (!inV[v] && !seen[v]) seen[v] = 1, cand.push_back(v);
                        for (int v : cand) seen[v] = 0;
                        std::sort(cand.begin(), cand.end(),
                                  [&](int a, int c) { return pos[a] < pos[c]; });
                        for (size_t i = 0; i < cand.size() && (int64_t)i < bits; ++i)
                            joined[cand[i]] = 1, grew = 1;
                    }
                }
                if (!grew) break;                // a whole component with no solution
                // ---- closure, labels ----
                for (int v = 0; v < V; ++v)
                    if (joined[v]) {
                        inV[v] = 1;
                        for (int c : chks_of[v])
                            if (label[c] == none) label[c] = c;
                    }
                for (bool changed = true; changed;) {
                    changed = false;
                    for (int v = 0; v < V; ++v) {
                        if (!inV[v]) continue;
                        int m = none;
                        for (int c : chks_of[v]) m = label[c] < m ? label[c] : m;
                        for (int c : chks_of[v])
                            if (label[c] != m) label[c] = m, changed = true;
                    }
                }
                // ---- eliminate over the cluster columns ----
                A = A0;
                for (int c = 0; c < C; ++c) {
                    A[(size_t)c * W + (V >> 6)] |= (uint64_t)s0[c] << (V & 63);
                    used[c] = 0;
                }
                int rank = 0;
                for (int i = 0; i < V && rank < C; ++i) {
                    const int j = order[i];
                    if (!inV[j]) continue;
                    const int wj = j >> 6;
                    const uint64_t bj = (uint64_t)1 << (j & 63);
                    int r = -1;
                    for (int c = 0; c < C; ++c)
                        if (!used[c] && (A[(size_t)c * W + wj] & bj)) { r = c; break; }
                    if (r < 0) continue;
                    used[r] = 1;
                    piv_col[r] = j;
                    ++rank;
                    const uint64_t* pr = &A[(size_t)r * W];
                    for (int c = 0; c < C; ++c) {
                        uint64_t* row = &A[(size_t)c * W];
                        if (c == r || !(row[wj] & bj)) continue;
                        for (int w = 0; w < W; ++w) row[w] ^= pr[w];
                    }
                }
                // ---- invalid labels ----
                std::fill(invalid.begin(), invalid.end(), 0);
                int bad = 0;
                for (int c = 0; c < C; ++c)
                    if (!used[c] && ((A[(size_t)c * W + (V >> 6)] >> (V & 63)) & 1))
                        invalid[label[c]] = 1, bad = 1;      // such a row is in a cluster
                if (!bad) {
                    for (int c = 0; c < C; ++c)
                        if (used[c])
                            z[piv_col[c]] ^= (uint8_t)((A[(size_t)c * W + (V >> 6)] >> (V & 63)) & 1);
                    st = 0;
                    break;
                }
                for (int c = 0; c < C; ++c) active[c] = label[c] != none && invalid[label[c]];
            }
        }
        int nc = 0, nv = 0;
        for (int c = 0; c < C; ++c) nc += label[c] == c;
        for (int v = 0; v < V; ++v) nv += inV[v];
        for (int v = 0; v < V; ++v) eb[v] = z[v] ? T(1) : T(0);
        if (status) status[b] = st;
        if (rounds_out) rounds_out[b] = rounds;
        if (nclus) nclus[b] = nc;
        if (ncols) ncols[b] = nv;
    }
    return GNND_OK;
}

inline int gnnd_lsd_host_checked(const int64_t* h_var, const int64_t* h_chk, int64_t num_edges,
                                 int32_t num_var, int32_t num_chk, int dtype, const void* h_x,
                                 const void* h_pred, int base, int32_t bits_per_step, void* h_ehat,
                                 int32_t* h_status, int32_t* h_rounds, int32_t* h_nclus,
                                 int32_t* h_ncols, int64_t batch) {
    const int rc = gnnd_args_rc(
        gnnd_host_list_ok(h_var, h_chk, num_edges, num_var, num_chk, batch) &&
            gnnd_lsd_params_ok(base, bits_per_step),
        dtype);
    if (rc != GNND_OK) return rc;
    if (batch == 0) return GNND_OK;
    if (!h_x || !h_pred || !h_ehat) return GNND_ERR_INVALID_ARG;
    return gnnd_by_dtype(dtype, [&](auto z) {
        using T = decltype(z);
        return gnnd_lsd_host_impl<T>(h_var, h_chk, num_edges, num_var, num_chk, (const T*)h_x,
                                     (const T*)h_pred, base, bits_per_step, (T*)h_ehat, h_status,
                                     h_rounds, h_nclus, h_ncols, batch);
    });
}

// ---- gated LSD (gnnd_lsd_gated) ----
// The gated codewords are gathered, run through gnnd_lsd_host_impl as one batch and scattered back:
// codewords are independent, so these are the bits of the ungated call.  llr and the int outputs
// may be null.
template <typename T>
int gnnd_lsd_gated_host_impl(const int64_t* h_var, const int64_t* h_chk, int64_t num_edges, int V,
                             int C, const T* x, const T* pred, const T* llr, const int32_t* gate,
                             int base, int bits, T* ehat, int32_t* status, int32_t* rounds,
                             int32_t* nclus, int32_t* ncols, int64_t batch) {
    const int N = V + C;
    std::vector<int64_t> list;
    for (int64_t b = 0; b < batch; ++b)
        if (gate[b] != 0) list.push_back(b);
    const int64_t n = (int64_t)list.size();
    std::vector<T> gx((size_t)n * N), gp((size_t)n * V), ge((size_t)n * V);
    std::vector<int32_t> gi[4];
    for (auto& a : gi) a.resize(n);
    for (int64_t i = 0; i < n; ++i) {
        std::copy(x + list[i] * N, x + (list[i] + 1) * N, gx.begin() + i * N);
        std::copy(pred + list[i] * V, pred + (list[i] + 1) * V, gp.begin() + i * V);
    }
    const int st = gnnd_lsd_host_impl<T>(h_var, h_chk, num_edges, V, C, gx.data(), gp.data(), base,
                                         bits, ge.data(), gi[0].data(), gi[1].data(), gi[2].data(),
                                         gi[3].data(), n);
    if (st != GNND_OK) return st;
    int32_t* outs[4] = {status, rounds, nclus, ncols};
    for (int64_t i = 0; i < n; ++i) {
        std::copy(ge.begin() + i * V, ge.begin() + (i + 1) * V, ehat + list[i] * V);
        for (int j = 0; j < 4; ++j)
            if (outs[j]) outs[j][list[i]] = gi[j][i];
    }
    for (int64_t b = 0; b < batch; ++b) {
        if (gate[b] != 0) continue;
        for (int v = 0; v < V; ++v) {
            const bool h = llr ? llr[b * V + v] < T(0) : pred[b * V + v] > T(0.5);
            ehat[b * V + v] = h ? T(1) : T(0);
        }
        for (int j = 0; j < 4; ++j)
            if (outs[j]) outs[j][b] = 0;
    }
    return GNND_OK;
}

inline int gnnd_lsd_gated_host_checked(const int64_t* h_var, const int64_t* h_chk,
                                       int64_t num_edges, int32_t num_var, int32_t num_chk,
                                       int dtype, const void* h_x, const void* h_pred,
                                       const void* h_llr, const int32_t* h_gate, int base,
                                       int32_t bits_per_step, void* h_ehat, int32_t* h_status,
                                       int32_t* h_rounds, int32_t* h_nclus, int32_t* h_ncols,
                                       int64_t batch) {
    const int rc = gnnd_args_rc(
        gnnd_host_list_ok(h_var, h_chk, num_edges, num_var, num_chk, batch) &&
            gnnd_lsd_params_ok(base, bits_per_step),
        dtype);
    if (rc != GNND_OK) return rc;
    if (batch == 0) return GNND_OK;
    if (!h_x || !h_pred || !h_gate || !h_ehat) return GNND_ERR_INVALID_ARG;
    return gnnd_by_dtype(dtype, [&](auto z) {
        using T = decltype(z);
        return gnnd_lsd_gated_host_impl<T>(h_var, h_chk, num_edges, num_var, num_chk,
                                           (const T*)h_x, (const T*)h_pred, (const T*)h_llr, h_gate,
                                           base, bits_per_step, (T*)h_ehat, h_status, h_rounds,
                                           h_nclus, h_ncols, batch);
    });
}

// ---- gnnd_bplsd: gnnd_minsum_host (the device's fp64 exponential), then the gated mirror ----
inline bool gnnd_bplsd_params_ok(double alpha, double beta, int32_t iters, int32_t early_stop,
                                 int base, int32_t bits_per_step) {
    return gnnd_minsum_params_ok(alpha, beta, iters, early_stop) &&
           gnnd_lsd_params_ok(base, bits_per_step);
}

inline int gnnd_bplsd_host_checked(const int64_t* h_var, const int64_t* h_chk, int64_t num_edges,
                                   int32_t num_var, int32_t num_chk, int dtype, const void* h_x,
                                   double alpha, double beta, int32_t iters, int32_t early_stop,
                                   int base, int32_t bits_per_step, void* h_pred, void* h_llr,
                                   int32_t* h_iters, int32_t* h_bp_status, void* h_ehat,
                                   int32_t* h_status, int32_t* h_rounds, int32_t* h_nclus,
                                   int32_t* h_ncols, int64_t batch) {
    const int rc = gnnd_args_rc(
        gnnd_host_list_ok(h_var, h_chk, num_edges, num_var, num_chk, batch) &&
            gnnd_bplsd_params_ok(alpha, beta, iters, early_stop, base, bits_per_step),
        dtype);
    if (rc != GNND_OK) return rc;
    if (batch == 0) return GNND_OK;
    if (!h_x || !h_pred || !h_llr || !h_bp_status || !h_ehat) return GNND_ERR_INVALID_ARG;
    const int st = gnnd_minsum_host_checked(h_var, h_chk, num_edges, num_var, num_chk, dtype, h_x,
                                            alpha, beta, iters, early_stop, h_pred, h_llr, h_iters,
                                            h_bp_status, batch, /*device_exp=*/true);
    if (st != GNND_OK) return st;
    return gnnd_lsd_gated_host_checked(h_var, h_chk, num_edges, num_var, num_chk, dtype, h_x,
                                       h_pred, h_llr, h_bp_status, base, bits_per_step, h_ehat,
                                       h_status, h_rounds, h_nclus, h_ncols, batch);
}

// gnnd_osd_host.h — host mirror of gnnd_osd0 and gnnd_osd (include/gnnd.h): ordered-statistics
// post-processing (order 0, combination sweep, exhaustive) in plain C++.  No HIP types: a plain
// host compiler builds it, so a stand-alone program can run it under host sanitizers
// (tools/osd_host_check.cpp).  Same definition as the
// kernel in gnnd_osd.hip, bit for bit: columns by descending key (ties: ascending v), Gauss-Jordan
// over the C rows of H^T with the residual syndrome as one more column, solution on the pivots;
// for gnnd_osd the candidates over the free columns follow, lightest first, ties to the lowest
// candidate index.
#pragma once
#include <stdint.h>
#include <math.h>
#include <algorithm>
#include <limits>
#include <vector>
#include "gnnd_host_args.h"

inline bool gnnd_osd_base_ok(int base) {
    return base == GNND_OSD_BASE_ZERO || base == GNND_OSD_BASE_HARD;
}

// method and order of gnnd_osd within the contract's limits
inline bool gnnd_osd_order_ok(int method, int32_t order) {
    if (order < 0) return false;
    if (method == GNND_OSD_0) return true;
    if (method == GNND_OSD_CS) return order <= 64;
    return method == GNND_OSD_E && order <= 12;
}

// weight of (s xor c) over the pivot rows; c may be null
inline int gnnd_osd_host_weight(const uint64_t* s, const uint64_t* c, const uint64_t* c2,
                                const uint64_t* used, int RW) {
    int n = 0;
    for (int w = 0; w < RW; ++w)
        n += __builtin_popcountll((s[w] ^ (c ? c[w] : 0) ^ (c2 ? c2[w] : 0)) & used[w]);
    return n;
}

// choice may be null; method GNND_OSD_0 is gnnd_osd0_host
template <typename T>
int gnnd_osd_host_impl(const int64_t* h_var, const int64_t* h_chk, int64_t num_edges, int V,
                       int C, const T* x, const T* pred, int base, int method, int order_arg,
                       T* ehat, int32_t* status, int32_t* choice, int64_t batch) {
    for (int64_t e = 0; e < num_edges; ++e)
        if (h_var[e] < 0 || h_var[e] >= V || h_chk[e] < 0 || h_chk[e] >= C) return GNND_ERR_GRAPH;
    // rows of H^T, bit-packed: words [0, W) hold the V columns, bit V the syndrome
    const int W = V / 64 + 1;
    std::vector<uint64_t> A0((size_t)C * W, 0), A;
    for (int64_t e = 0; e < num_edges; ++e)
        A0[(size_t)h_chk[e] * W + (h_var[e] >> 6)] |= (uint64_t)1 << (h_var[e] & 63);
    const int N = V + C;
    std::vector<T> key(V);
    std::vector<int> order(V), piv_col(C);
    std::vector<uint8_t> z(V), used(C), is_piv(V);
    // candidates: bits over the C rows, 64 per word: the pivot rows, s, the free columns
    const int RW = (C + 63) / 64;
    std::vector<int> free_col;
    std::vector<uint64_t> usedw(RW), sw(RW), colw, sub;
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
        }
        std::stable_sort(order.begin(), order.end(),
                         [&](int a, int c) { return key[a] > key[c]; });
        A = A0;
        for (int c = 0; c < C; ++c) {            // residual s = t xor H^T z
            uint64_t* row = &A[(size_t)c * W];
            int par = xc[c] < T(0);
            for (int v = 0; v < V; ++v) par ^= (int)((row[v >> 6] >> (v & 63)) & 1) & z[v];
            row[V >> 6] |= (uint64_t)par << (V & 63);
            used[c] = 0;
        }
        int rank = 0;
        for (int pos = 0; pos < V && rank < C; ++pos) {
            const int j = order[pos];
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
        int bad = 0;
        for (int c = 0; c < C; ++c)
            bad |= !used[c] && ((A[(size_t)c * W + (V >> 6)] >> (V & 63)) & 1);
        int best_idx = 0;
        if (!bad && method != GNND_OSD_0) {
            std::fill(is_piv.begin(), is_piv.end(), 0);
            std::fill(usedw.begin(), usedw.end(), 0);
            std::fill(sw.begin(), sw.end(), 0);
            for (int c = 0; c < C; ++c) {
                if (used[c]) {
                    is_piv[piv_col[c]] = 1;
                    usedw[c >> 6] |= (uint64_t)1 << (c & 63);
                }
                sw[c >> 6] |= ((A[(size_t)c * W + (V >> 6)] >> (V & 63)) & 1) << (c & 63);
            }
            free_col.clear();
            for (int pos = 0; pos < V; ++pos)
                if (!is_piv[order[pos]]) free_col.push_back(order[pos]);
            const int F = (int)free_col.size();
            const int lam = order_arg < F ? order_arg : F;
            colw.assign((size_t)F * RW, 0);
            for (int i = 0; i < F; ++i) {
                const int f = free_col[i];
                for (int c = 0; c < C; ++c)
                    colw[(size_t)i * RW + (c >> 6)] |=
                        ((A[(size_t)c * W + (f >> 6)] >> (f & 63)) & 1) << (c & 63);
            }
            int best = gnnd_osd_host_weight(sw.data(), nullptr, nullptr, usedw.data(), RW);
            if (method == GNND_OSD_CS) {
                int ba = -1, bb = -1;
                for (int i = 0; i < F; ++i) {
                    const int c = 1 + gnnd_osd_host_weight(sw.data(), &colw[(size_t)i * RW], nullptr,
                                                           usedw.data(), RW);
                    if (c < best) { best = c; best_idx = 1 + i; ba = i; }
                }
                int idx = 1 + F;
                for (int a = 0; a < lam; ++a)
                    for (int q = a + 1; q < lam; ++q, ++idx) {
                        const int c = 2 + gnnd_osd_host_weight(sw.data(), &colw[(size_t)a * RW],
                                                               &colw[(size_t)q * RW], usedw.data(), RW);
                        if (c < best) { best = c; best_idx = idx; ba = a; bb = q; }
                    }
                for (int i : {ba, bb})
                    if (i >= 0) {
                        z[free_col[i]] ^= 1;
                        for (int w = 0; w < RW; ++w) sw[w] ^= colw[(size_t)i * RW + w];
                    }
            } else {
                // sub[m] = XOR of the columns in subset m, from the subset without m's lowest bit
                sub.assign(((size_t)1 << lam) * RW, 0);
                for (int m = 1; m < (1 << lam); ++m) {
                    const int low = __builtin_ctz(m);
                    for (int w = 0; w < RW; ++w)
                        sub[(size_t)m * RW + w] =
                            sub[(size_t)(m & (m - 1)) * RW + w] ^ colw[(size_t)low * RW + w];
                    const int c = __builtin_popcount(m) +
                                  gnnd_osd_host_weight(sw.data(), &sub[(size_t)m * RW], nullptr,
                                                       usedw.data(), RW);
                    if (c < best) { best = c; best_idx = m; }
                }
                for (int i = 0; i < lam; ++i)
                    if ((best_idx >> i) & 1) z[free_col[i]] ^= 1;
                for (int w = 0; w < RW; ++w) sw[w] ^= sub[(size_t)best_idx * RW + w];
            }
            for (int c = 0; c < C; ++c)
                if (used[c]) z[piv_col[c]] ^= (uint8_t)((sw[c >> 6] >> (c & 63)) & 1);
        } else if (!bad) {
            for (int c = 0; c < C; ++c)
                if (used[c]) z[piv_col[c]] ^= (uint8_t)((A[(size_t)c * W + (V >> 6)] >> (V & 63)) & 1);
        }
        for (int v = 0; v < V; ++v) eb[v] = z[v] ? T(1) : T(0);
        status[b] = bad;
        if (choice) choice[b] = best_idx;
    }
    return GNND_OK;
}

template <typename T>
int gnnd_osd0_host_impl(const int64_t* h_var, const int64_t* h_chk, int64_t num_edges, int V,
                        int C, const T* x, const T* pred, int base, T* ehat, int32_t* status,
                        int64_t batch) {
    return gnnd_osd_host_impl<T>(h_var, h_chk, num_edges, V, C, x, pred, base, GNND_OSD_0, 0, ehat,
                                 status, nullptr, batch);
}

inline int gnnd_osd0_host_checked(const int64_t* h_var, const int64_t* h_chk, int64_t num_edges,
                                  int32_t num_var, int32_t num_chk, int dtype, const void* h_x,
                                  const void* h_pred, int base, void* h_ehat, int32_t* h_status,
                                  int64_t batch) {
    const int rc = gnnd_args_rc(
        gnnd_host_list_ok(h_var, h_chk, num_edges, num_var, num_chk, batch) &&
            gnnd_osd_base_ok(base),
        dtype);
    if (rc != GNND_OK) return rc;
    if (batch == 0) return GNND_OK;
    if (!h_x || !h_pred || !h_ehat || !h_status) return GNND_ERR_INVALID_ARG;
    return gnnd_by_dtype(dtype, [&](auto z) {
        using T = decltype(z);
        return gnnd_osd0_host_impl<T>(h_var, h_chk, num_edges, num_var, num_chk, (const T*)h_x,
                                      (const T*)h_pred, base, (T*)h_ehat, h_status, batch);
    });
}

inline int gnnd_osd_host_checked(const int64_t* h_var, const int64_t* h_chk, int64_t num_edges,
                                 int32_t num_var, int32_t num_chk, int dtype, const void* h_x,
                                 const void* h_pred, int base, int method, int32_t order,
                                 void* h_ehat, int32_t* h_status, int32_t* h_choice,
                                 int64_t batch) {
    const int rc = gnnd_args_rc(
        gnnd_host_list_ok(h_var, h_chk, num_edges, num_var, num_chk, batch) &&
            gnnd_osd_base_ok(base) && gnnd_osd_order_ok(method, order),
        dtype);
    if (rc != GNND_OK) return rc;
    if (batch == 0) return GNND_OK;
    if (!h_x || !h_pred || !h_ehat || !h_status) return GNND_ERR_INVALID_ARG;
    return gnnd_by_dtype(dtype, [&](auto z) {
        using T = decltype(z);
        return gnnd_osd_host_impl<T>(h_var, h_chk, num_edges, num_var, num_chk, (const T*)h_x,
                                     (const T*)h_pred, base, method, order, (T*)h_ehat, h_status,
                                     h_choice, batch);
    });
}

// ---- gated OSD (gnnd_osd_gated): scratch size and host mirror ----
// the device list of gated codewords holds int32 indices and the count check wants batch + 1
constexpr int64_t kOsdGatedMaxBatch = 2147483646;
// int32 count, then int32 list[batch]
inline int64_t gnnd_osd_gated_bytes(int64_t batch) { return 4 * (batch + 1); }

// The gated codewords are gathered, run through gnnd_osd_host_impl as one batch and scattered
// back: codewords are independent, so these are the bits of the ungated call.  llr and choice may
// be null.
template <typename T>
int gnnd_osd_gated_host_impl(const int64_t* h_var, const int64_t* h_chk, int64_t num_edges, int V,
                             int C, const T* x, const T* pred, const T* llr, const int32_t* gate,
                             int base, int method, int order, T* ehat, int32_t* status,
                             int32_t* choice, int64_t batch) {
    const int N = V + C;
    std::vector<int64_t> list;
    for (int64_t b = 0; b < batch; ++b)
        if (gate[b] != 0) list.push_back(b);
    const int64_t n = (int64_t)list.size();
    std::vector<T> gx((size_t)n * N), gp((size_t)n * V), ge((size_t)n * V);
    std::vector<int32_t> gs(n), gc(n);
    for (int64_t i = 0; i < n; ++i) {
        std::copy(x + list[i] * N, x + (list[i] + 1) * N, gx.begin() + i * N);
        std::copy(pred + list[i] * V, pred + (list[i] + 1) * V, gp.begin() + i * V);
    }
    const int st = gnnd_osd_host_impl<T>(h_var, h_chk, num_edges, V, C, gx.data(), gp.data(), base,
                                         method, order, ge.data(), gs.data(), gc.data(), n);
    if (st != GNND_OK) return st;
    for (int64_t i = 0; i < n; ++i) {
        std::copy(ge.begin() + i * V, ge.begin() + (i + 1) * V, ehat + list[i] * V);
        status[list[i]] = gs[i];
        if (choice) choice[list[i]] = gc[i];
    }
    for (int64_t b = 0; b < batch; ++b) {
        if (gate[b] != 0) continue;
        for (int v = 0; v < V; ++v) {
            const bool h = llr ? llr[b * V + v] < T(0) : pred[b * V + v] > T(0.5);
            ehat[b * V + v] = h ? T(1) : T(0);
        }
        status[b] = 0;
        if (choice) choice[b] = -1;
    }
    return GNND_OK;
}

inline int gnnd_osd_gated_host_checked(const int64_t* h_var, const int64_t* h_chk,
                                       int64_t num_edges, int32_t num_var, int32_t num_chk,
                                       int dtype, const void* h_x, const void* h_pred,
                                       const void* h_llr, const int32_t* h_gate, int base,
                                       int method, int32_t order, void* h_ehat, int32_t* h_status,
                                       int32_t* h_choice, int64_t batch) {
    const int rc = gnnd_args_rc(
        gnnd_host_list_ok(h_var, h_chk, num_edges, num_var, num_chk, batch) &&
            gnnd_osd_base_ok(base) && gnnd_osd_order_ok(method, order),
        dtype);
    if (rc != GNND_OK) return rc;
    if (batch == 0) return GNND_OK;
    if (!h_x || !h_pred || !h_gate || !h_ehat || !h_status) return GNND_ERR_INVALID_ARG;
    return gnnd_by_dtype(dtype, [&](auto z) {
        using T = decltype(z);
        return gnnd_osd_gated_host_impl<T>(h_var, h_chk, num_edges, num_var, num_chk,
                                           (const T*)h_x, (const T*)h_pred, (const T*)h_llr, h_gate,
                                           base, method, order, (T*)h_ehat, h_status, h_choice,
                                           batch);
    });
}

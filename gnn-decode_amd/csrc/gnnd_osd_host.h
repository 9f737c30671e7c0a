// gnnd_osd_host.h — host mirror of gnnd_osd0 (include/gnnd.h): order-0 ordered-statistics
// post-processing in plain C++.  No HIP types: a plain host compiler builds it, so a stand-alone
// program can run it under host sanitizers (tools/osd_host_check.cpp).  Same definition as the
// kernel in gnnd_osd.hip, bit for bit: columns by descending key (ties: ascending v), Gauss-Jordan
// over the C rows of H^T with the residual syndrome as one more column, solution on the pivots.
#pragma once
#include <stdint.h>
#include <math.h>
#include <algorithm>
#include <limits>
#include <vector>
#include "../../include/gnnd.h"

template <typename T>
int gnnd_osd0_host_impl(const int64_t* h_var, const int64_t* h_chk, int64_t num_edges, int V,
                        int C, const T* x, const T* pred, int base, T* ehat, int32_t* status,
                        int64_t batch) {
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
    std::vector<uint8_t> z(V), used(C);
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
        if (!bad)
            for (int c = 0; c < C; ++c)
                if (used[c]) z[piv_col[c]] ^= (uint8_t)((A[(size_t)c * W + (V >> 6)] >> (V & 63)) & 1);
        for (int v = 0; v < V; ++v) eb[v] = z[v] ? T(1) : T(0);
        status[b] = bad;
    }
    return GNND_OK;
}

inline int gnnd_osd0_host_checked(const int64_t* h_var, const int64_t* h_chk, int64_t num_edges,
                                  int32_t num_var, int32_t num_chk, int dtype, const void* h_x,
                                  const void* h_pred, int base, void* h_ehat, int32_t* h_status,
                                  int64_t batch) {
    if (!h_var || !h_chk || num_edges <= 0 || num_var <= 0 || num_chk <= 0 || batch < 0)
        return GNND_ERR_INVALID_ARG;
    if (base != GNND_OSD_BASE_ZERO && base != GNND_OSD_BASE_HARD) return GNND_ERR_INVALID_ARG;
    if (dtype == GNND_BF16) return GNND_ERR_UNSUPPORTED;
    if (dtype != GNND_F32 && dtype != GNND_F64) return GNND_ERR_INVALID_ARG;
    if (batch == 0) return GNND_OK;
    if (!h_x || !h_pred || !h_ehat || !h_status) return GNND_ERR_INVALID_ARG;
    if (dtype == GNND_F32)
        return gnnd_osd0_host_impl<float>(h_var, h_chk, num_edges, num_var, num_chk,
                                          (const float*)h_x, (const float*)h_pred, base,
                                          (float*)h_ehat, h_status, batch);
    return gnnd_osd0_host_impl<double>(h_var, h_chk, num_edges, num_var, num_chk,
                                       (const double*)h_x, (const double*)h_pred, base,
                                       (double*)h_ehat, h_status, batch);
}

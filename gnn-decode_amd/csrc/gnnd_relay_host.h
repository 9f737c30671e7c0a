// gnnd_relay_host.h — host mirror of gnnd_relay (include/gnnd.h): relay min-sum BP, a chain of
// memory-strength legs that keeps the lightest solution, in plain C++.  No HIP types: a plain host
// compiler builds it, so a stand-alone program can run it under host sanitizers
// (tools/relay_host_check.cpp).  Same definition as the kernel in gnnd_relay.hip, bit for bit in
// every output: gnnd_minsum_host's check step, c * l + g * M as three roundings (build this header's
// translation unit with -ffp-contract=off), the variable sum over E(v) in ascending edge order, the
// weight through the fixed 64-partial tree.
// Also the mirrors of gnnd_relay_soft (the same loop with the soft output: the MEAN accumulator
// summed in the variable step in the kernel's order, one multiply by the same host-computed inv,
// and in fp64 the kernel's exponential, gnnd_exp_f64_device) and of gnnd_relay_osd (that mirror,
// then gnnd_osd_gated_host).
#pragma once
#include "gnnd_minsum_host.h"
#include "gnnd_osd_host.h"

// legs / iters0 / iters_leg / stop_after / alpha / beta within the contract's limits; the
// iteration total must fit the int32 d_iters reports
inline bool gnnd_relay_params_ok(double alpha, double beta, int32_t legs, int32_t iters0,
                                 int32_t iters_leg, int32_t stop_after) {
    if (legs < 1 || iters0 < 1 || iters_leg < 1 || stop_after < 1) return false;
    if ((int64_t)iters0 + (int64_t)(legs - 1) * iters_leg > 2147483647LL) return false;
    return gnnd_minsum_params_ok(alpha, beta, 1, 1);
}

inline bool gnnd_relay_soft_ok(int soft) {
    return soft == GNND_RELAY_SOFT_LAST || soft == GNND_RELAY_SOFT_MEAN;
}

// the arguments gnnd_relay_osd's two stages refuse with GNND_ERR_INVALID_ARG whatever the graph
// and the pointers
inline bool gnnd_relay_osd_params_ok(double alpha, double beta, int32_t legs, int32_t iters0,
                                     int32_t iters_leg, int32_t stop_after, int soft, int base,
                                     int method, int32_t order) {
    if (!gnnd_relay_params_ok(alpha, beta, legs, iters0, iters_leg, stop_after)) return false;
    if (!gnnd_relay_soft_ok(soft)) return false;
    return gnnd_osd_base_ok(base) && gnnd_osd_order_ok(method, order);
}

// weight(h) of the contract: 64 partials over v = j (mod 64) in ascending v, then the six-step
// butterfly p_j = p_j + p_{j xor s}, s = 32 .. 1; every p_j ends as the same value, w = p_0
template <typename T>
T gnnd_relay_weight(const T* L, const T* l, int V) {
    T p[64], n[64];
    for (int j = 0; j < 64; ++j) {
        T s = T(0);
        for (int v = j; v < V; v += 64) s = s + (L[v] < T(0) ? l[v] : T(0));
        p[j] = s;
    }
    for (int s = 32; s >= 1; s >>= 1) {
        for (int j = 0; j < 64; ++j) n[j] = p[j] + p[j ^ s];
        for (int j = 0; j < 64; ++j) p[j] = n[j];
    }
    return p[0];
}

// every output but ehat may be null.  soft_mode: -1 for gnnd_relay (pred and soft_out unused), else
// a gnnd_relay_soft_mode: pred is then required and soft_out may be null.  device_exp: the fp64
// soft output through gnnd_exp_f64_device instead of the host library's exp, as in
// gnnd_minsum_host_impl
template <typename T>
int gnnd_relay_host_impl(const int64_t* h_var, const int64_t* h_chk, int64_t num_edges, int V,
                         int C, const T* x, const T* gammas, int legs, int iters0, int iters_leg,
                         int stop_after, double alpha, double beta, T* ehat, T* llr,
                         int32_t* iters_out, int32_t* status, int32_t* leg_out, int32_t* nsol_out,
                         int64_t batch, int soft_mode = -1, T* pred = nullptr,
                         T* soft_out = nullptr, bool device_exp = false) {
    GnndHostGraph hg;
    const int rc = gnnd_host_bp_graph_build(h_var, h_chk, num_edges, V, C, hg);
    if (rc != GNND_OK) return rc;
    const T a = (T)alpha, bt = (T)beta;
    const int N = V + C;
    std::vector<T> msg(hg.E), L(V), A(V), best(V);
    const bool mean = soft_mode == GNND_RELAY_SOFT_MEAN;
    std::vector<T> acc(mean ? V : 0);
    const T inv = (T)(1.0 / ((double)iters0 + (double)(legs - 1) * (double)iters_leg));
    for (int64_t b = 0; b < batch; ++b) {
        const T* xv = x + b * N;
        const T* xc = xv + V;
        for (int v = 0; v < V; ++v) L[v] = xv[v];                    // M_v = l_v
        if (mean) std::fill(acc.begin(), acc.end(), T(0));
        int total = 0, nsol = 0, bestk = -1;
        T bestw = T(0);
        for (int k = 0; k < legs; ++k) {
            const T* g = gammas + (size_t)k * V;
            // A_v: the prior term of the leg (l_v itself where g_v == 0: selected, not computed)
            for (int v = 0; v < V; ++v) {
                const T c = T(1) - g[v];
                const T cl = c * xv[v];
                A[v] = g[v] == T(0) ? xv[v] : cl;
            }
            for (int e = 0; e < hg.E; ++e) {
                const int v = hg.evar[e];
                const T gm = g[v] * L[v];
                const T lam = A[v] + gm;
                msg[e] = g[v] == T(0) ? A[v] : lam;
            }
            const int Tk = k == 0 ? iters0 : iters_leg;
            for (int it = 0; it < Tk; ++it) {
                ++total;
                gnnd_minsum_check_step(hg, xc, a, bt, msg.data());
                for (int v = 0; v < V; ++v) {
                    const T gm = g[v] * L[v];
                    const T lam = A[v] + gm;
                    L[v] = gnnd_minsum_var_update(hg, v, g[v] == T(0) ? A[v] : lam, msg.data());
                    if (mean) acc[v] = acc[v] + L[v];
                }
                if (gnnd_syndrome_ok(hg, xc, L.data())) {
                    const T w = gnnd_relay_weight(L.data(), xv, V);
                    if (nsol == 0 || w < bestw) {                    // strict: a tie keeps the earlier
                        bestw = w;
                        bestk = k;
                        best = L;
                    }
                    ++nsol;
                    break;
                }
            }
            if (nsol >= stop_after) break;
        }
        const T* src = nsol ? best.data() : L.data();
        for (int v = 0; v < V; ++v) {
            ehat[b * V + v] = src[v] < T(0) ? T(1) : T(0);
            if (llr) llr[b * V + v] = src[v];
            if (soft_mode < 0) continue;
            T Z = src[v];
            if (mean && !nsol) {
                const T Av = acc[v];
                Z = Av * inv;                                        // one multiply
            }
            if (soft_out) soft_out[b * V + v] = Z;
            pred[b * V + v] = gnnd_soft_output(Z, device_exp);
        }
        if (iters_out) iters_out[b] = total;
        if (status) status[b] = nsol ? 0 : 1;
        if (leg_out) leg_out[b] = bestk;
        if (nsol_out) nsol_out[b] = nsol;
    }
    return GNND_OK;
}

inline int gnnd_relay_host_checked(const int64_t* h_var, const int64_t* h_chk, int64_t num_edges,
                                   int32_t num_var, int32_t num_chk, int dtype, const void* h_x,
                                   const void* h_gammas, int32_t legs, int32_t iters0,
                                   int32_t iters_leg, int32_t stop_after, double alpha, double beta,
                                   void* h_ehat, void* h_llr, int32_t* h_iters, int32_t* h_status,
                                   int32_t* h_leg, int32_t* h_nsol, int64_t batch) {
    const int rc = gnnd_args_rc(
        gnnd_host_list_ok(h_var, h_chk, num_edges, num_var, num_chk, batch) &&
            gnnd_relay_params_ok(alpha, beta, legs, iters0, iters_leg, stop_after),
        dtype);
    if (rc != GNND_OK) return rc;
    if (batch == 0) return GNND_OK;
    if (!h_x || !h_gammas || !h_ehat) return GNND_ERR_INVALID_ARG;
    return gnnd_by_dtype(dtype, [&](auto z) {
        using T = decltype(z);
        return gnnd_relay_host_impl<T>(h_var, h_chk, num_edges, num_var, num_chk, (const T*)h_x,
                                       (const T*)h_gammas, legs, iters0, iters_leg, stop_after,
                                       alpha, beta, (T*)h_ehat, (T*)h_llr, h_iters, h_status, h_leg,
                                       h_nsol, batch);
    });
}

// gnnd_relay_soft_host: gnnd_relay_host's checks, then soft and h_pred.  The fp64 exponential is
// always the device's sequence (device_exp), so h_pred is the device's bits.
inline int gnnd_relay_soft_host_checked(const int64_t* h_var, const int64_t* h_chk,
                                        int64_t num_edges, int32_t num_var, int32_t num_chk,
                                        int dtype, const void* h_x, const void* h_gammas,
                                        int32_t legs, int32_t iters0, int32_t iters_leg,
                                        int32_t stop_after, double alpha, double beta, int soft,
                                        void* h_pred, void* h_soft, void* h_ehat, void* h_llr,
                                        int32_t* h_iters, int32_t* h_status, int32_t* h_leg,
                                        int32_t* h_nsol, int64_t batch) {
    const int rc = gnnd_args_rc(
        gnnd_host_list_ok(h_var, h_chk, num_edges, num_var, num_chk, batch) &&
            gnnd_relay_params_ok(alpha, beta, legs, iters0, iters_leg, stop_after) &&
            gnnd_relay_soft_ok(soft),
        dtype);
    if (rc != GNND_OK) return rc;
    if (batch == 0) return GNND_OK;
    if (!h_x || !h_gammas || !h_ehat || !h_pred) return GNND_ERR_INVALID_ARG;
    return gnnd_by_dtype(dtype, [&](auto z) {
        using T = decltype(z);
        return gnnd_relay_host_impl<T>(h_var, h_chk, num_edges, num_var, num_chk, (const T*)h_x,
                                       (const T*)h_gammas, legs, iters0, iters_leg, stop_after,
                                       alpha, beta, (T*)h_ehat, (T*)h_llr, h_iters, h_status, h_leg,
                                       h_nsol, batch, soft, (T*)h_pred, (T*)h_soft, true);
    });
}

// gnnd_relay_osd_host: the soft mirror, then gnnd_osd_gated_host with the relay status as the gate
inline int gnnd_relay_osd_host_checked(const int64_t* h_var, const int64_t* h_chk,
                                       int64_t num_edges, int32_t num_var, int32_t num_chk,
                                       int dtype, const void* h_x, const void* h_gammas,
                                       int32_t legs, int32_t iters0, int32_t iters_leg,
                                       int32_t stop_after, double alpha, double beta, int soft,
                                       int base, int method, int32_t order, void* h_pred,
                                       void* h_llr, int32_t* h_iters, int32_t* h_relay_status,
                                       int32_t* h_leg, int32_t* h_nsol, void* h_ehat,
                                       int32_t* h_status, int32_t* h_choice, int64_t batch) {
    const int rc = gnnd_args_rc(
        gnnd_host_list_ok(h_var, h_chk, num_edges, num_var, num_chk, batch) &&
            gnnd_relay_osd_params_ok(alpha, beta, legs, iters0, iters_leg, stop_after, soft, base,
                                     method, order),
        dtype);
    if (rc != GNND_OK) return rc;
    if (batch == 0) return GNND_OK;
    if (!h_x || !h_gammas || !h_pred || !h_llr || !h_relay_status || !h_ehat || !h_status)
        return GNND_ERR_INVALID_ARG;
    const int st = gnnd_relay_soft_host_checked(h_var, h_chk, num_edges, num_var, num_chk, dtype,
                                                h_x, h_gammas, legs, iters0, iters_leg, stop_after,
                                                alpha, beta, soft, h_pred, nullptr, h_ehat, h_llr,
                                                h_iters, h_relay_status, h_leg, h_nsol, batch);
    if (st != GNND_OK) return st;
    return gnnd_osd_gated_host_checked(h_var, h_chk, num_edges, num_var, num_chk, dtype, h_x,
                                       h_pred, h_llr, h_relay_status, base, method, order, h_ehat,
                                       h_status, h_choice, batch);
}

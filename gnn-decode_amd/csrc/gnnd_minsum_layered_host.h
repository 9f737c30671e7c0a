// gnnd_minsum_layered_host.h — host mirror of gnnd_minsum_layered and gnnd_bposd_layered
// (include/gnnd.h): min-sum BP on the layered (check-sequential) schedule, in plain C++.  No HIP
// types: a plain host compiler builds it, so a stand-alone program can run it under host
// sanitizers (tools/minsum_layered_host_check.cpp).  Same definition as the kernel in
// gnnd_minsum_layered.hip, bit for bit in llr / iters / status: the greedy layer rule, the checks
// in (layer, c) order, q = L - r as one subtraction, gnnd_minsum's check step in the first-min /
// second-min / arg-min form with a * m - b as two roundings (build this header's translation unit
// with -ffp-contract=off), L = q + r' as one addition.
#pragma once
#include "gnnd_bposd_host.h"

// The layer rule: checks in ascending c, layer(c) = the smallest k >= 0 such that no check
// c' < c of layer k shares a variable with c.  cptr [C+1] / cvar [E]: the variables of check c are
// cvar[cptr[c] .. cptr[c+1]).  -> layer_of [C]; returns the number of layers.
inline int gnnd_layers_build(int V, int C, const int* cptr, const int* cvar,
                             std::vector<int>& layer_of) {
    layer_of.assign(C, 0);
    std::vector<std::vector<int>> seen(V);        // layers of the earlier checks at each variable
    std::vector<char> used;
    int nl = 0;
    for (int c = 0; c < C; ++c) {
        used.assign(nl + 1, 0);
        for (int i = cptr[c]; i < cptr[c + 1]; ++i)
            for (int k : seen[cvar[i]]) used[k] = 1;
        int k = 0;
        while (used[k]) ++k;                       // used[nl] == 0: a new layer at the latest
        layer_of[c] = k;
        if (k == nl) ++nl;
        for (int i = cptr[c]; i < cptr[c + 1]; ++i) seen[cvar[i]].push_back(k);
    }
    return nl;
}

// layer_of [C] -> layer_ptr [nl+1], layer_chk [C]: the checks sorted by (layer, c)
inline void gnnd_layers_order(int C, int nl, const std::vector<int>& layer_of,
                              std::vector<int>& layer_ptr, std::vector<int>& layer_chk) {
    layer_ptr.assign(nl + 1, 0);
    layer_chk.assign(C, 0);
    for (int c = 0; c < C; ++c) layer_ptr[layer_of[c] + 1]++;
    for (int k = 0; k < nl; ++k) layer_ptr[k + 1] += layer_ptr[k];
    std::vector<int> fill(layer_ptr.begin(), layer_ptr.end() - 1);
    for (int c = 0; c < C; ++c) layer_chk[fill[layer_of[c]]++] = c;
}

// cvar[i] = evar[cedge[i]]: the variables check by check, in the order of cedge
inline std::vector<int> gnnd_host_graph_cvar(const GnndHostGraph& hg) {
    std::vector<int> cvar(hg.E);
    for (int i = 0; i < hg.E; ++i) cvar[i] = hg.evar[hg.cedge[i]];
    return cvar;
}

// h_layer_of_check [C] may be null
inline int gnnd_graph_layers_host_checked(const int64_t* h_var, const int64_t* h_chk,
                                          int64_t num_edges, int32_t V, int32_t C,
                                          int32_t* h_nlayers, int32_t* h_layer_of_check) {
    if (!h_var || !h_chk || !h_nlayers || num_edges <= 0 || V <= 0 || C <= 0)
        return GNND_ERR_INVALID_ARG;
    GnndHostGraph hg;                              // a check of degree 1 has its layer too
    const int rc = gnnd_host_graph_build(h_var, h_chk, num_edges, V, C, hg);
    if (rc != GNND_OK) return rc;
    std::vector<int> layer_of;
    *h_nlayers = gnnd_layers_build(V, C, hg.cptr.data(), gnnd_host_graph_cvar(hg).data(), layer_of);
    if (h_layer_of_check)
        for (int c = 0; c < C; ++c) h_layer_of_check[c] = layer_of[c];
    return GNND_OK;
}

// out, llr, iters_out and status may each be null here (the checked entry requires out).
// device_exp as in gnnd_minsum_host_impl.
template <typename T>
int gnnd_minsum_layered_host_impl(const int64_t* h_var, const int64_t* h_chk, int64_t num_edges,
                                  int V, int C, const T* x, double alpha, double beta, int iters,
                                  int early_stop, T* out, T* llr, int32_t* iters_out,
                                  int32_t* status, int64_t batch, bool device_exp = false) {
    GnndHostGraph hg;
    const int rc = gnnd_host_bp_graph_build(h_var, h_chk, num_edges, V, C, hg);
    if (rc != GNND_OK) return rc;
    const int E = hg.E;
    const std::vector<int>&cptr = hg.cptr, &cedge = hg.cedge;
    const std::vector<int> cvar = gnnd_host_graph_cvar(hg);
    std::vector<int> layer_of, layer_ptr, order;
    const int nl = gnnd_layers_build(V, C, cptr.data(), cvar.data(), layer_of);
    gnnd_layers_order(C, nl, layer_of, layer_ptr, order);
    const T a = (T)alpha, bt = (T)beta;
    const int N = V + C;
    std::vector<T> r(E), L(V);
    for (int64_t b = 0; b < batch; ++b) {
        const T* xv = x + b * N;
        const T* xc = xv + V;
        for (int v = 0; v < V; ++v) L[v] = xv[v];
        for (int e = 0; e < E; ++e) r[e] = T(0);
        int it = 0, ok = 0;
        while (it < iters) {
            ++it;
            for (int s = 0; s < C; ++s) {
                const int c = order[s];
                T min1 = std::numeric_limits<T>::infinity(), min2 = min1;
                int arg = -1, par = xc[c] < T(0);
                for (int i = cptr[c]; i < cptr[c + 1]; ++i) {
                    const T q = L[cvar[i]] - r[cedge[i]];
                    const T aq = std::fabs(q);
                    par ^= (int)(q < T(0));
                    if (aq < min1) { min2 = min1; min1 = aq; arg = cedge[i]; }
                    else if (aq < min2) min2 = aq;
                }
                // the variables of one check are distinct: L[v] of a later edge is still the
                // value the first walk read, so q is the same subtraction
                for (int i = cptr[c]; i < cptr[c + 1]; ++i) {
                    const int e = cedge[i], v = cvar[i];
                    const T q = L[v] - r[e];
                    const T rn = gnnd_minsum_signed_mag(a, bt, e == arg ? min2 : min1,
                                                        par ^ (int)(q < T(0)));
                    L[v] = q + rn;
                    r[e] = rn;
                }
            }
            ok = gnnd_syndrome_ok(hg, xc, L.data());
            if (early_stop && ok) break;
        }
        for (int v = 0; v < V; ++v) {
            if (llr) llr[b * V + v] = L[v];
            if (out) out[b * V + v] = gnnd_soft_output(L[v], device_exp);
        }
        if (iters_out) iters_out[b] = it;
        if (status) status[b] = ok ? 0 : 1;
    }
    return GNND_OK;
}

inline int gnnd_minsum_layered_host_checked(const int64_t* h_var, const int64_t* h_chk,
                                            int64_t num_edges, int32_t num_var, int32_t num_chk,
                                            int dtype, const void* h_x, double alpha, double beta,
                                            int32_t iters, int32_t early_stop, void* h_out,
                                            void* h_llr, int32_t* h_iters, int32_t* h_status,
                                            int64_t batch, bool device_exp = false) {
    const int rc = gnnd_args_rc(gnnd_host_list_ok(h_var, h_chk, num_edges, num_var, num_chk, batch) &&
                                    gnnd_minsum_params_ok(alpha, beta, iters, early_stop),
                                dtype);
    if (rc != GNND_OK) return rc;
    if (batch == 0) return GNND_OK;
    if (!h_x || !h_out) return GNND_ERR_INVALID_ARG;
    return gnnd_by_dtype(dtype, [&](auto z) {
        using T = decltype(z);
        return gnnd_minsum_layered_host_impl<T>(h_var, h_chk, num_edges, num_var, num_chk,
                                                (const T*)h_x, alpha, beta, iters, early_stop,
                                                (T*)h_out, (T*)h_llr, h_iters, h_status, batch,
                                                device_exp);
    });
}

// gnnd_bposd_host_checked with the layered loop as its first stage
inline int gnnd_bposd_layered_host_checked(const int64_t* h_var, const int64_t* h_chk,
                                           int64_t num_edges, int32_t num_var, int32_t num_chk,
                                           int dtype, const void* h_x, double alpha, double beta,
                                           int32_t iters, int32_t early_stop, int base, int method,
                                           int32_t order, void* h_pred, void* h_llr,
                                           int32_t* h_iters, int32_t* h_bp_status, void* h_ehat,
                                           int32_t* h_status, int32_t* h_choice, int64_t batch) {
    const int rc = gnnd_args_rc(
        gnnd_host_list_ok(h_var, h_chk, num_edges, num_var, num_chk, batch) &&
            gnnd_bposd_params_ok(alpha, beta, iters, early_stop, base, method, order),
        dtype);
    if (rc != GNND_OK) return rc;
    if (batch == 0) return GNND_OK;
    if (!h_x || !h_pred || !h_llr || !h_bp_status || !h_ehat || !h_status)
        return GNND_ERR_INVALID_ARG;
    const int st = gnnd_minsum_layered_host_checked(h_var, h_chk, num_edges, num_var, num_chk,
                                                    dtype, h_x, alpha, beta, iters, early_stop,
                                                    h_pred, h_llr, h_iters, h_bp_status, batch,
                                                    /*device_exp=*/true);
    if (st != GNND_OK) return st;
    return gnnd_osd_gated_host_checked(h_var, h_chk, num_edges, num_var, num_chk, dtype, h_x,
                                       h_pred, h_llr, h_bp_status, base, method, order, h_ehat,
                                       h_status, h_choice, batch);
}

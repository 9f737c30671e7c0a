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

// the edge list of gnnd_graph_create -> per-check edge lists; the graph checks of gnnd_minsum_host
struct GnndLayeredTables {
    int E = 0;
    std::vector<int> cptr, cedge, evar, cvar;     // cvar[i] = evar[cedge[i]]
};

inline int gnnd_layered_tables(const int64_t* h_var, const int64_t* h_chk, int64_t num_edges,
                               int V, int C, GnndLayeredTables& t) {
    if (num_edges > 65535 || V > 65535 || C > 65535) return GNND_ERR_UNSUPPORTED;
    const int E = (int)num_edges;
    t.E = E;
    t.cptr.assign(C + 1, 0);
    t.cedge.assign(E, 0);
    t.evar.assign(E, 0);
    t.cvar.assign(E, 0);
    for (int e = 0; e < E; ++e) {
        const int64_t v = h_var[e], c = h_chk[e];
        if (v < 0 || v >= V || c < 0 || c >= C) return GNND_ERR_GRAPH;
        if (e > 0 && (v < h_var[e - 1] || (v == h_var[e - 1] && c <= h_chk[e - 1])))
            return GNND_ERR_GRAPH;                                   // sorted by (v, c), no duplicate
        t.evar[e] = (int)v;
        t.cptr[c + 1]++;
    }
    for (int c = 0; c < C; ++c) t.cptr[c + 1] += t.cptr[c];
    std::vector<int> fill(t.cptr.begin(), t.cptr.end() - 1);
    for (int e = 0; e < E; ++e) t.cedge[fill[h_chk[e]]++] = e;
    for (int i = 0; i < E; ++i) t.cvar[i] = t.evar[t.cedge[i]];
    return GNND_OK;
}

// h_layer_of_check [C] may be null
inline int gnnd_graph_layers_host_checked(const int64_t* h_var, const int64_t* h_chk,
                                          int64_t num_edges, int32_t V, int32_t C,
                                          int32_t* h_nlayers, int32_t* h_layer_of_check) {
    if (!h_var || !h_chk || !h_nlayers || num_edges <= 0 || V <= 0 || C <= 0)
        return GNND_ERR_INVALID_ARG;
    GnndLayeredTables t;
    const int rc = gnnd_layered_tables(h_var, h_chk, num_edges, V, C, t);
    if (rc != GNND_OK) return rc;
    std::vector<int> layer_of;
    *h_nlayers = gnnd_layers_build(V, C, t.cptr.data(), t.cvar.data(), layer_of);
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
    GnndLayeredTables t;
    const int rc = gnnd_layered_tables(h_var, h_chk, num_edges, V, C, t);
    if (rc != GNND_OK) return rc;
    const int E = t.E;
    const std::vector<int>&cptr = t.cptr, &cedge = t.cedge, &cvar = t.cvar;
    for (int c = 0; c < C; ++c)
        if (cptr[c + 1] - cptr[c] < 2) return GNND_ERR_UNSUPPORTED;
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
                    const T m = e == arg ? min2 : min1;
                    const T am = a * m;
                    const T d = am - bt;
                    const T mag = d > T(0) ? d : T(0);
                    const T rn = (par ^ (int)(q < T(0))) ? -mag : mag;
                    L[v] = q + rn;
                    r[e] = rn;
                }
            }
            ok = 1;
            for (int c = 0; c < C; ++c) {
                int par = xc[c] < T(0);
                for (int i = cptr[c]; i < cptr[c + 1]; ++i) par ^= (int)(L[cvar[i]] < T(0));
                if (par) { ok = 0; break; }
            }
            if (early_stop && ok) break;
        }
        for (int v = 0; v < V; ++v) {
            if (llr) llr[b * V + v] = L[v];
            if (!out) continue;
            if (device_exp && sizeof(T) == sizeof(double))
                out[b * V + v] = T(1) / (T(1) + (T)gnnd_exp_f64_device((double)L[v]));
            else
                out[b * V + v] = T(1) / (T(1) + (T)exp((double)L[v]));
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
    if (!h_var || !h_chk || num_edges <= 0 || num_var <= 0 || num_chk <= 0 || batch < 0)
        return GNND_ERR_INVALID_ARG;
    if (!gnnd_minsum_params_ok(alpha, beta, iters, early_stop)) return GNND_ERR_INVALID_ARG;
    if (dtype == GNND_BF16) return GNND_ERR_UNSUPPORTED;
    if (dtype != GNND_F32 && dtype != GNND_F64) return GNND_ERR_INVALID_ARG;
    if (batch == 0) return GNND_OK;
    if (!h_x || !h_out) return GNND_ERR_INVALID_ARG;
    if (dtype == GNND_F32)
        return gnnd_minsum_layered_host_impl<float>(h_var, h_chk, num_edges, num_var, num_chk,
                                                    (const float*)h_x, alpha, beta, iters,
                                                    early_stop, (float*)h_out, (float*)h_llr,
                                                    h_iters, h_status, batch, device_exp);
    return gnnd_minsum_layered_host_impl<double>(h_var, h_chk, num_edges, num_var, num_chk,
                                                 (const double*)h_x, alpha, beta, iters, early_stop,
                                                 (double*)h_out, (double*)h_llr, h_iters, h_status,
                                                 batch, device_exp);
}

// gnnd_bposd_host_checked with the layered loop as its first stage
inline int gnnd_bposd_layered_host_checked(const int64_t* h_var, const int64_t* h_chk,
                                           int64_t num_edges, int32_t num_var, int32_t num_chk,
                                           int dtype, const void* h_x, double alpha, double beta,
                                           int32_t iters, int32_t early_stop, int base, int method,
                                           int32_t order, void* h_pred, void* h_llr,
                                           int32_t* h_iters, int32_t* h_bp_status, void* h_ehat,
                                           int32_t* h_status, int32_t* h_choice, int64_t batch) {
    if (!h_var || !h_chk || num_edges <= 0 || num_var <= 0 || num_chk <= 0 || batch < 0)
        return GNND_ERR_INVALID_ARG;
    if (!gnnd_bposd_params_ok(alpha, beta, iters, early_stop, base, method, order))
        return GNND_ERR_INVALID_ARG;
    if (dtype == GNND_BF16) return GNND_ERR_UNSUPPORTED;
    if (dtype != GNND_F32 && dtype != GNND_F64) return GNND_ERR_INVALID_ARG;
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

// gnnd_minsum_host.h — host mirror of gnnd_minsum (include/gnnd.h): normalized / offset min-sum
// BP on the flooding schedule with the syndrome-converged early stop, in plain C++.  No HIP types:
// a plain host compiler builds it, so a stand-alone program can run it under host sanitizers
// (tools/minsum_host_check.cpp).  Same definition as the kernel in gnnd_minsum.hip, bit for bit in
// llr / iters / status: the check step in the first-min / second-min / arg-min form, a * m - b as
// two roundings (build this header's translation unit with -ffp-contract=off), the variable sum
// over E(v) in ascending edge order.
// The steps of that definition (check step, variable update, syndrome test, soft output) are stated
// here once, for this mirror and for those of gnnd_relay, gnnd_bpgd and gnnd_minsum_layered; the
// device states them separately in gnnd_wave_tile.h, and the GPU tests compare the two.
#pragma once
#include <stdint.h>
#include <math.h>
#include <cmath>
#include <limits>
#include <vector>
#include "gnnd_host_args.h"

// iters / alpha / beta / early_stop within the contract's limits
inline bool gnnd_minsum_params_ok(double alpha, double beta, int32_t iters, int32_t early_stop) {
    if (iters < 1 || (early_stop != 0 && early_stop != 1)) return false;
    if (!(alpha > 0.0 && alpha <= 1.0)) return false;               // false for a NaN too
    return beta >= 0.0 && beta <= std::numeric_limits<double>::max();
}

// The kernel's fp64 exponential (g_exp(double), gnnd_common.h), operation for operation: k =
// rint(x log2 e), r = x - k ln2 with a two-part ln2, the degree-13 Taylor polynomial by Horner in
// fused multiply-adds, ldexp.  Every step is one correctly rounded IEEE operation, so a host
// compiler gives the device's bits.  gnnd_bposd_host computes its fp64 soft output with it: its
// OSD stage orders the columns by that output, and the order must be the device's.
inline double gnnd_exp_f64_device(double x) {
    static const double coef[13] = {
        1.0 / 6227020800.0, 1.0 / 479001600.0, 1.0 / 39916800.0, 1.0 / 3628800.0,
        1.0 / 362880.0, 1.0 / 40320.0, 1.0 / 5040.0, 1.0 / 720.0, 1.0 / 120.0, 1.0 / 24.0,
        1.0 / 6.0, 0.5, 1.0};
    x = std::fmin(std::fmax(x, -750.0), 710.0);
    const double k = std::rint(x * 1.4426950408889634);
    double r = std::fma(-k, 6.93147180369123816490e-01, x);
    r = std::fma(-k, 1.90821492927058770002e-10, r);
    double p = coef[0];
    for (int i = 1; i < 13; ++i) p = std::fma(p, r, coef[i]);
    p = std::fma(p, r, 1.0);
    return std::ldexp(p, (int)k);
}

// The graph tables of the host mirrors, built from the edge list gnnd_graph_create takes, with its
// checks: more than 65535 edges / variables / checks is GNND_ERR_UNSUPPORTED, an id out of range or
// an edge list not sorted by (v, c) (or with a duplicate) GNND_ERR_GRAPH.
struct GnndHostGraph {
    int E = 0;
    std::vector<int> vptr, cptr;    // [V + 1], [C + 1]: edge ranges of the variables / checks
    std::vector<int> cedge;         // [E] edge ids check by check, ascending inside a check
    std::vector<int> evar;          // [E] the variable of every edge
};

inline int gnnd_host_graph_build(const int64_t* h_var, const int64_t* h_chk, int64_t num_edges,
                                 int V, int C, GnndHostGraph& hg) {
    if (num_edges > 65535 || V > 65535 || C > 65535) return GNND_ERR_UNSUPPORTED;
    const int E = (int)num_edges;
    hg.E = E;
    hg.vptr.assign(V + 1, 0);
    hg.cptr.assign(C + 1, 0);
    hg.cedge.assign(E, 0);
    hg.evar.assign(E, 0);
    std::vector<int>&vptr = hg.vptr, &cptr = hg.cptr, &cedge = hg.cedge, &evar = hg.evar;
    for (int e = 0; e < E; ++e) {
        const int64_t v = h_var[e], c = h_chk[e];
        if (v < 0 || v >= V || c < 0 || c >= C) return GNND_ERR_GRAPH;
        if (e > 0 && (v < h_var[e - 1] || (v == h_var[e - 1] && c <= h_chk[e - 1])))
            return GNND_ERR_GRAPH;                                   // sorted by (v, c), no duplicate
        evar[e] = (int)v;
        vptr[v + 1]++;
        cptr[c + 1]++;
    }
    for (int v = 0; v < V; ++v) vptr[v + 1] += vptr[v];
    for (int c = 0; c < C; ++c) cptr[c + 1] += cptr[c];
    std::vector<int> fill(cptr.begin(), cptr.end() - 1);
    for (int e = 0; e < E; ++e) cedge[fill[h_chk[e]]++] = e;
    return GNND_OK;
}

// The tables of a BP mirror: gnnd_host_graph_build, then a check of degree < 2 is
// GNND_ERR_UNSUPPORTED (the check step wants a second minimum).
inline int gnnd_host_bp_graph_build(const int64_t* h_var, const int64_t* h_chk, int64_t num_edges,
                                    int V, int C, GnndHostGraph& hg) {
    const int rc = gnnd_host_graph_build(h_var, h_chk, num_edges, V, C, hg);
    if (rc != GNND_OK) return rc;
    for (int c = 0; c < C; ++c)
        if (hg.cptr[c + 1] - hg.cptr[c] < 2) return GNND_ERR_UNSUPPORTED;
    return GNND_OK;
}

// r = sign * max(a * m - b, 0), negative where neg != 0; a * m - b is two roundings
template <typename T>
T gnnd_minsum_signed_mag(T a, T bt, T m, int neg) {
    const T am = a * m;
    const T d = am - bt;
    const T mag = d > T(0) ? d : T(0);
    return neg ? -mag : mag;
}

// flooding check step over msg [E] (q_e in, r_e out), xc [C] the syndrome part of the input
template <typename T>
void gnnd_minsum_check_step(const GnndHostGraph& hg, const T* xc, T a, T bt, T* msg) {
    const std::vector<int>&cptr = hg.cptr, &cedge = hg.cedge;
    const int C = (int)cptr.size() - 1;
    for (int c = 0; c < C; ++c) {
        T min1 = std::numeric_limits<T>::infinity(), min2 = min1;
        int arg = -1, par = xc[c] < T(0);
        for (int i = cptr[c]; i < cptr[c + 1]; ++i) {
            const T q = msg[cedge[i]];
            const T aq = std::fabs(q);
            par ^= (int)(q < T(0));
            if (aq < min1) { min2 = min1; min1 = aq; arg = cedge[i]; }
            else if (aq < min2) min2 = aq;
        }
        for (int i = cptr[c]; i < cptr[c + 1]; ++i) {
            const int e = cedge[i];
            const T q = msg[e];
            msg[e] = gnnd_minsum_signed_mag(a, bt, e == arg ? min2 : min1, par ^ (int)(q < T(0)));
        }
    }
}

// variable update of v: returns s = s0 + r_e1 + ... over E(v) in ascending edge order, and
// q_e = s - r_e into msg
template <typename T>
T gnnd_minsum_var_update(const GnndHostGraph& hg, int v, T s0, T* msg) {
    T s = s0;
    for (int e = hg.vptr[v]; e < hg.vptr[v + 1]; ++e) s = s + msg[e];
    for (int e = hg.vptr[v]; e < hg.vptr[v + 1]; ++e) msg[e] = s - msg[e];
    return s;
}

// H^T h == t for h_v = (L_v < 0), t_c = (xc_c < 0)
template <typename T>
int gnnd_syndrome_ok(const GnndHostGraph& hg, const T* xc, const T* L) {
    const int C = (int)hg.cptr.size() - 1;
    for (int c = 0; c < C; ++c) {
        int par = xc[c] < T(0);
        for (int i = hg.cptr[c]; i < hg.cptr[c + 1]; ++i) par ^= (int)(L[hg.evar[hg.cedge[i]]] < T(0));
        if (par) return 0;
    }
    return 1;
}

// soft output 1 / (1 + exp(L)).  device_exp: in fp64 through gnnd_exp_f64_device instead of the
// host library's exp (fp32 is the host library's either way)
template <typename T>
T gnnd_soft_output(T L, bool device_exp) {
    if (device_exp && sizeof(T) == sizeof(double))
        return T(1) / (T(1) + (T)gnnd_exp_f64_device((double)L));
    return T(1) / (T(1) + (T)exp((double)L));
}

// out, llr, iters_out and status may each be null here (the checked entry requires out).
// device_exp: the fp64 soft output through gnnd_exp_f64_device instead of the host library's exp
// (gnnd_bposd_host; gnnd_minsum_host keeps the library's)
template <typename T>
int gnnd_minsum_host_impl(const int64_t* h_var, const int64_t* h_chk, int64_t num_edges, int V,
                          int C, const T* x, double alpha, double beta, int iters, int early_stop,
                          T* out, T* llr, int32_t* iters_out, int32_t* status, int64_t batch,
                          bool device_exp = false) {
    GnndHostGraph hg;
    const int rc = gnnd_host_bp_graph_build(h_var, h_chk, num_edges, V, C, hg);
    if (rc != GNND_OK) return rc;
    const T a = (T)alpha, bt = (T)beta;
    const int N = V + C;
    std::vector<T> msg(hg.E), L(V);
    for (int64_t b = 0; b < batch; ++b) {
        const T* xv = x + b * N;
        const T* xc = xv + V;
        for (int e = 0; e < hg.E; ++e) msg[e] = xv[hg.evar[e]];
        int it = 0, ok = 0;
        while (it < iters) {
            ++it;
            gnnd_minsum_check_step(hg, xc, a, bt, msg.data());
            for (int v = 0; v < V; ++v) L[v] = gnnd_minsum_var_update(hg, v, xv[v], msg.data());
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

inline int gnnd_minsum_host_checked(const int64_t* h_var, const int64_t* h_chk, int64_t num_edges,
                                    int32_t num_var, int32_t num_chk, int dtype, const void* h_x,
                                    double alpha, double beta, int32_t iters, int32_t early_stop,
                                    void* h_out, void* h_llr, int32_t* h_iters, int32_t* h_status,
                                    int64_t batch, bool device_exp = false) {
    const int rc = gnnd_args_rc(gnnd_host_list_ok(h_var, h_chk, num_edges, num_var, num_chk, batch) &&
                                    gnnd_minsum_params_ok(alpha, beta, iters, early_stop),
                                dtype);
    if (rc != GNND_OK) return rc;
    if (batch == 0) return GNND_OK;
    if (!h_x || !h_out) return GNND_ERR_INVALID_ARG;
    return gnnd_by_dtype(dtype, [&](auto z) {
        using T = decltype(z);
        return gnnd_minsum_host_impl<T>(h_var, h_chk, num_edges, num_var, num_chk, (const T*)h_x,
                                        alpha, beta, iters, early_stop, (T*)h_out, (T*)h_llr,
                                        h_iters, h_status, batch, device_exp);
    });
}

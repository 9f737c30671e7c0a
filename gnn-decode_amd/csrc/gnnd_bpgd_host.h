// gnnd_bpgd_host.h — host mirror of gnnd_bpgd (include/gnnd.h): min-sum BP with guided decimation,
// rounds of BP between which the least (or most) reliable undecimated variables get their prior
// frozen at +-clamp while the messages carry on, in plain C++.  No HIP types: a plain host compiler
// builds it, so a stand-alone program can run it under host sanitizers (tools/bpgd_host_check.cpp).
// Same definition as the kernel in gnnd_bpgd.hip, bit for bit in ehat / llr / iters / status / ndec
// and, in fp64, in pred (gnnd_exp_f64_device): gnnd_minsum_host's check step, a * m - b as two
// roundings (build this header's translation unit with -ffp-contract=off), the variable sum over
// E(v) in ascending edge order, the pick as a plain ascending scan with a strict compare.
#pragma once
#include "gnnd_minsum_host.h"

// iters0 / iters_round / rounds / per_round / pick / clamp / alpha / beta within the contract's
// limits; the iteration total must fit the int32 d_iters reports
inline bool gnnd_bpgd_params_ok(double alpha, double beta, int32_t iters0, int32_t iters_round,
                                int32_t rounds, int32_t per_round, int pick, double clamp) {
    if (iters0 < 1 || iters_round < 1 || rounds < 0 || per_round < 1) return false;
    if ((int64_t)iters0 + (int64_t)rounds * iters_round > 2147483647LL) return false;
    if (pick != GNND_BPGD_LEAST && pick != GNND_BPGD_MOST) return false;
    if (!(clamp > 0.0 && clamp <= std::numeric_limits<double>::max())) return false;   // NaN too
    return gnnd_minsum_params_ok(alpha, beta, 1, 1);
}

// c = (T)clamp must itself be finite: a finite double above FLT_MAX rounds to infinity in float
inline bool gnnd_bpgd_clamp_fits(int dtype, double clamp) {
    return dtype != GNND_F32 || clamp <= (double)std::numeric_limits<float>::max();
}

// v* of the contract: among dec_v == 0 the variable of minimum (LEAST) / maximum (MOST) |L_v|, ties
// to the lowest v.  The running best starts at the first undecimated variable, so the result is an
// in-range undecimated variable whatever L holds (a NaN never wins a strict compare); -1 only
// where every variable is decimated, which the caller excludes.
template <typename T>
int gnnd_bpgd_pick_var(const T* L, const unsigned char* dec, int V, int pick) {
    int best = -1;
    T bk = T(0);
    for (int v = 0; v < V; ++v) {
        if (dec[v]) continue;
        const T k = std::fabs(L[v]);
        if (best < 0 || (pick == GNND_BPGD_MOST ? k > bk : k < bk)) {
            best = v;
            bk = k;
        }
    }
    return best;
}

// every output but ehat may be null
template <typename T>
int gnnd_bpgd_host_impl(const int64_t* h_var, const int64_t* h_chk, int64_t num_edges, int V, int C,
                        const T* x, double alpha, double beta, int iters0, int iters_round,
                        int rounds, int per_round, int pick, double clamp, T* ehat, T* llr, T* pred,
                        int32_t* iters_out, int32_t* status, int32_t* ndec_out, int64_t batch) {
    GnndHostGraph hg;
    const int rc = gnnd_host_bp_graph_build(h_var, h_chk, num_edges, V, C, hg);
    if (rc != GNND_OK) return rc;
    const T a = (T)alpha, bt = (T)beta, cl = (T)clamp;
    const int N = V + C;
    std::vector<T> msg(hg.E), L(V), p(V);
    std::vector<unsigned char> dec(V);
    for (int64_t b = 0; b < batch; ++b) {
        const T* xv = x + b * N;
        const T* xc = xv + V;
        for (int v = 0; v < V; ++v) { p[v] = xv[v]; dec[v] = 0; }
        for (int e = 0; e < hg.E; ++e) msg[e] = p[hg.evar[e]];
        int total = 0, ndec = 0, ok = 0;
        for (int r = 0; ; ++r) {
            const int Tr = r == 0 ? iters0 : iters_round;
            for (int it = 0; it < Tr && !ok; ++it) {
                ++total;
                gnnd_minsum_check_step(hg, xc, a, bt, msg.data());
                for (int v = 0; v < V; ++v) L[v] = gnnd_minsum_var_update(hg, v, p[v], msg.data());
                ok = gnnd_syndrome_ok(hg, xc, L.data());
            }
            if (ok || r == rounds || ndec == V) break;
            const int picks = per_round < V - ndec ? per_round : V - ndec;
            for (int k = 0; k < picks; ++k) {
                const int vs = gnnd_bpgd_pick_var(L.data(), dec.data(), V, pick);
                p[vs] = L[vs] < T(0) ? -cl : cl;
                dec[vs] = 1;
                ++ndec;
            }
        }
        for (int v = 0; v < V; ++v) {
            ehat[b * V + v] = L[v] < T(0) ? T(1) : T(0);
            if (llr) llr[b * V + v] = L[v];
            if (pred) pred[b * V + v] = gnnd_soft_output(L[v], /*device_exp=*/true);
        }
        if (iters_out) iters_out[b] = total;
        if (status) status[b] = ok ? 0 : 1;
        if (ndec_out) ndec_out[b] = ndec;
    }
    return GNND_OK;
}

inline int gnnd_bpgd_host_checked(const int64_t* h_var, const int64_t* h_chk, int64_t num_edges,
                                  int32_t num_var, int32_t num_chk, int dtype, const void* h_x,
                                  double alpha, double beta, int32_t iters0, int32_t iters_round,
                                  int32_t rounds, int32_t per_round, int pick, double clamp,
                                  void* h_ehat, void* h_llr, void* h_pred, int32_t* h_iters,
                                  int32_t* h_status, int32_t* h_ndec, int64_t batch) {
    const int rc = gnnd_args_rc(
        gnnd_host_list_ok(h_var, h_chk, num_edges, num_var, num_chk, batch) &&
            gnnd_bpgd_params_ok(alpha, beta, iters0, iters_round, rounds, per_round, pick, clamp),
        dtype);
    if (rc != GNND_OK) return rc;
    if (!gnnd_bpgd_clamp_fits(dtype, clamp)) return GNND_ERR_INVALID_ARG;
    if (batch == 0) return GNND_OK;
    if (!h_x || !h_ehat) return GNND_ERR_INVALID_ARG;
    return gnnd_by_dtype(dtype, [&](auto z) {
        using T = decltype(z);
        return gnnd_bpgd_host_impl<T>(h_var, h_chk, num_edges, num_var, num_chk, (const T*)h_x,
                                      alpha, beta, iters0, iters_round, rounds, per_round, pick,
                                      clamp, (T*)h_ehat, (T*)h_llr, (T*)h_pred, h_iters, h_status,
                                      h_ndec, batch);
    });
}

// gnnd_bposd_host.h — host mirror of gnnd_bposd (include/gnnd.h): gnnd_minsum_host followed by
// gnnd_osd_gated_host with the min-sum status as the gate and the min-sum LLRs as the source of
// the pass-through hard decision.  Its fp64 soft output uses the kernel's exponential scheme
// (gnnd_exp_f64_device), so the OSD stage sees the device's bits and orders the columns as the
// device does; in fp32 the device calls its math library's expf, which no host code reproduces,
// and the soft output is the host library's as in gnnd_minsum_host.  Plain C++, no HIP types;
// build its translation unit with -ffp-contract=off (the min-sum contract).
#pragma once
#include "gnnd_minsum_host.h"
#include "gnnd_osd_host.h"

// the arguments both stages refuse with GNND_ERR_INVALID_ARG whatever the graph and the pointers
inline bool gnnd_bposd_params_ok(double alpha, double beta, int32_t iters, int32_t early_stop,
                                 int base, int method, int32_t order) {
    if (!gnnd_minsum_params_ok(alpha, beta, iters, early_stop)) return false;
    return gnnd_osd_base_ok(base) && gnnd_osd_order_ok(method, order);
}

inline int gnnd_bposd_host_checked(const int64_t* h_var, const int64_t* h_chk, int64_t num_edges,
                                   int32_t num_var, int32_t num_chk, int dtype, const void* h_x,
                                   double alpha, double beta, int32_t iters, int32_t early_stop,
                                   int base, int method, int32_t order, void* h_pred, void* h_llr,
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
    const int st = gnnd_minsum_host_checked(h_var, h_chk, num_edges, num_var, num_chk, dtype, h_x,
                                            alpha, beta, iters, early_stop, h_pred, h_llr, h_iters,
                                            h_bp_status, batch, /*device_exp=*/true);
    if (st != GNND_OK) return st;
    return gnnd_osd_gated_host_checked(h_var, h_chk, num_edges, num_var, num_chk, dtype, h_x,
                                       h_pred, h_llr, h_bp_status, base, method, order, h_ehat,
                                       h_status, h_choice, batch);
}

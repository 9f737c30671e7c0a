// gnnd_host_args.h — the argument checks and the float / double dispatch every decoder entry of
// include/gnnd.h starts with, host mirrors and device entries alike.  Plain C++, no HIP types.
#pragma once
#include <stdint.h>
#include "../../include/gnnd.h"

// the edge list and the sizes every host mirror takes
inline bool gnnd_host_list_ok(const int64_t* h_var, const int64_t* h_chk, int64_t num_edges,
                              int32_t num_var, int32_t num_chk, int64_t batch) {
    return h_var && h_chk && num_edges > 0 && num_var > 0 && num_chk > 0 && batch >= 0;
}

// The refusals decided before anything else, in the contract's order: args_ok (the handles, the
// sizes and the entry's own parameters: all GNND_ERR_INVALID_ARG), then bf16
// (GNND_ERR_UNSUPPORTED), then a dtype outside the enum.
inline int gnnd_args_rc(bool args_ok, int dtype) {
    if (!args_ok) return GNND_ERR_INVALID_ARG;
    if (dtype == GNND_BF16) return GNND_ERR_UNSUPPORTED;
    if (dtype != GNND_F32 && dtype != GNND_F64) return GNND_ERR_INVALID_ARG;
    return GNND_OK;
}

// f(T()) with T = float or double: `[&](auto z) { using T = decltype(z); return impl<T>(...); }`
template <typename F>
inline int gnnd_by_dtype(int dtype, F&& f) {
    return dtype == GNND_F32 ? f(float()) : f(double());
}

// gnnd_decode_v24.hip — kernel instantiations for model GNND_V24 (see gnnd_decode_impl.h).
#include "gnnd_decode_impl.h"

GNND_DEBUG_TU(decode_v24)

int gnnd_launch_v24(const gnnd_graph* g, int dtype, const void* w, const void* x, void* out,
                       int64_t B, int iters, hipStream_t st) {
    return launch_model<GNND_V24>(g, dtype, w, x, out, B, iters, st);
}

int gnnd_launch_v24_tape(const gnnd_graph* g, int dtype, const void* w, const void* x, void* out,
                         int64_t B, int iters, void* tape, hipStream_t st) {
    if (dtype == GNND_F32) return launch_decode_r<GNND_V24, float>(g, w, x, out, B, iters, st, tape);
    return launch_decode_r<GNND_V24, double>(g, w, x, out, B, iters, st, tape);
}

int gnnd_launch_v24_tape_loss(const gnnd_graph* g, int dtype, const void* w, const void* x, void* out,
                              int64_t B, int iters, void* tape, const void* y, const uint32_t* lmask,
                              int nl, int logical_only, int need_ncomp, void* gp, void* loss_b,
                              hipStream_t st) {
    if (dtype != GNND_F32) return GNND_ERR_UNSUPPORTED;
    const FwdLoss fl{y, lmask, nl, logical_only, need_ncomp, gp, loss_b};
    return launch_decode_r<GNND_V24, float>(g, w, x, out, B, iters, st, tape, &fl);
}

// ---------------------------------------------------------------------------------------
// decoder_v2_4's check-side MLP through the table the fp64 decoder reads (ctab_build_kernel /
// ctab_valid / ctab_eval, gnnd_decode_impl.h): the same staged entries and evaluation, exposed
// so tests can hold it against the reference MLP (quantum/decoder_v2_4.py:241-243, :253-257)
// ---------------------------------------------------------------------------------------
namespace {
__global__ void __launch_bounds__(256)
ctab_eval_kernel(const double* __restrict__ w, int max_dc, const double* __restrict__ u,
                 double* __restrict__ y, int64_t n, int32_t* __restrict__ ok) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double* tab = (double*)smem;
    const int R = max_dc > 1 ? max_dc - 1 : 0, R8 = kCtabInv * R;
    const bool valid = ctab_valid(w, R);
    if (blockIdx.x == 0 && threadIdx.x == 0) *ok = valid ? 1 : 0;
    if (!valid) return;                                       // (uniform)
    const double2* src = (const double2*)(w + kV24CtabOff + (size_t)(kCtabInv * kCtabRcap - R8) * kCtabNC);
    for (int i = threadIdx.x; i < ctab_entries(max_dc) * kCtabNC / 2; i += blockDim.x) ((double2*)tab)[i] = src[i];
    __syncthreads();
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        y[i] = ctab_eval(tab, u[i], R8);
}
}  // namespace

extern "C" int gnnd_v24_check_mlp_table(const gnnd_graph* g, const void* d_w, const void* d_u,
                                        void* d_y, int64_t n, int32_t* d_ok, void* stream) {
    if (!g || !d_w || !d_ok || n < 0 || (n > 0 && (!d_u || !d_y))) return GNND_ERR_INVALID_ARG;
    const int max_dc = g->view.max_dc;
    const size_t lds = (size_t)ctab_entries(max_dc < kCtabRcap + 1 ? max_dc : kCtabRcap + 1) * kCtabNC * 8;
    auto kern = ctab_eval_kernel;
    if (lds > 64 * 1024)
        GNND_HIP_CHECK(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const int64_t blocks = n > 0 ? std::min<int64_t>((n + 255) / 256, 64) : 1;
    kern<<<(unsigned)blocks, 256, lds, (hipStream_t)stream>>>((const double*)d_w, max_dc, (const double*)d_u,
                                                               (double*)d_y, n, d_ok);
    GNND_LAUNCH_CHECK();
    return GNND_OK;
}

// the variable-side MLP through the channel-prior tables (vtab_eval, gnnd_decode_impl.h), for
// tests: y[i] = tanh(ggc1.mlp(u[i], x[i]) / 2) (the check step's pre-op, what the tables hold)
// and hit[i] = 1 where a table covers (u[i], x[i]), else hit[i] = 0 and y[i] untouched (the
// decoder evaluates the 128 units there); x = NULL: the readout MLP's table, y[i] = mlp(u[i])
namespace {
__global__ void __launch_bounds__(256)
vtab_eval_kernel(const double* __restrict__ w, const double* __restrict__ u, const double* __restrict__ xv,
                 double* __restrict__ y, int32_t* __restrict__ hit, int64_t n) {
    const int n_pt = (int)w[kV24PriorHdr];
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        int h = 0;
        if (!xv) {                                        // the readout MLP's table
            double v;
            if (n_pt > 0 && w[kV24PriorHdr + 1] != 0.0 &&
                vtab_eval<kVtInvR, false>(w + kV24PriorOff + (size_t)n_pt * kVtStride, u[i], 0.0, v)) {
                y[i] = v;
                h = 1;
            }
            hit[i] = h;
            continue;
        }
        const long long xb = __double_as_longlong(xv[i]);
        for (int t = 0; t < n_pt; ++t) {
            const double* tb = w + kV24PriorOff + (size_t)t * kVtStride;
            if (__double_as_longlong(tb[0]) != xb) continue;
            double v;
            if (vtab_eval<kVtInvG, true>(tb, u[i], xv[i], v)) {
                y[i] = v;
                h = 1;
            }
            break;
        }
        hit[i] = h;
    }
}
}  // namespace

extern "C" int gnnd_v24_var_mlp_table(const void* d_w, const void* d_u, const void* d_x, void* d_y,
                                      int32_t* d_hit, int64_t n, void* stream) {
    if (!d_w || n < 0 || (n > 0 && (!d_u || !d_y || !d_hit))) return GNND_ERR_INVALID_ARG;
    if (n == 0) return GNND_OK;
    const int64_t blocks = std::min<int64_t>((n + 255) / 256, 1024);
    vtab_eval_kernel<<<(unsigned)blocks, 256, 0, (hipStream_t)stream>>>(
        (const double*)d_w, (const double*)d_u, (const double*)d_x, (double*)d_y, d_hit, n);
    GNND_LAUNCH_CHECK();
    return GNND_OK;
}

// ---------------------------------------------------------------------------------------
// Channel-prior discovery on the device (gnnd_v24_scan_priors): the distinct first variable
// inputs x[b * xs + xv0] of a batch -- the element the decoder keys a codeword's prior table on
// (decode_kernel's staging loop, gnnd_decode_impl.h) -- ascending, into d_priors, with no host
// round trip.  The ABI carries no scratch buffer, so the set under construction lives in
// d_priors itself: 64 slots of an open-addressed set of the values' bit patterns, cleared to
// all ones (a NaN no input can insert: NaN inputs are skipped), exactly as many as tables can be
// built -- the 65th distinct value finds no free slot and raises d_status[1].
//   scan_priors_insert_kernel: one codeword per lane; a wave peels its distinct values off by
//     ballot (first pending lane's value, every lane holding the same bits retires) and lane 0
//     inserts each one with a 64-bit compare-and-swap after a plain read of the slot (a value
//     already present costs no atomic), skipping the value it inserted last.
//   scan_priors_rank_kernel: one wave ranks the occupied slots by value (ties of +-0 by bits)
//     and rewrites d_priors in that order, zeros after them, and d_status = {count, 0} or, on
//     overflow, zeros and {0, 1}.
// Which slot a value lands in depends on the scheduling; the set of occupied values and whether
// an insertion failed (more than 64 distinct values) do not, so the result is a pure function
// of x.
// ---------------------------------------------------------------------------------------
namespace {
constexpr unsigned long long kScanEmpty = ~0ull;

__device__ __forceinline__ void scan_insert(unsigned long long* set, int32_t* status, unsigned long long key) {
    unsigned h = (unsigned)(((key ^ (key >> 29)) * 0x9E3779B97F4A7C15ull) >> 58);   // top 6 bits
    for (int i = 0; i < kVtMaxPriors; ++i, h = (h + 1) & (kVtMaxPriors - 1)) {
        unsigned long long cur = __hip_atomic_load(&set[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == kScanEmpty) cur = atomicCAS(&set[h], kScanEmpty, key);
        if (cur == kScanEmpty || cur == key) return;      // inserted, or already there
    }
    atomicExch(&status[1], 1);                            // 64 other values hold every slot
}

__global__ void __launch_bounds__(256)
scan_priors_insert_kernel(const double* __restrict__ x, int xs, int xv0, int64_t B,
                          unsigned long long* set, int32_t* status) {
    const int lane = threadIdx.x & 63;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    unsigned long long last = kScanEmpty;                 // (wave-uniform) the value inserted last
    for (int64_t b0 = (int64_t)blockIdx.x * blockDim.x + (threadIdx.x - lane); b0 < B; b0 += stride) {
        const int64_t b = b0 + lane;
        const double v = b < B ? x[b * xs + xv0] : __longlong_as_double((long long)kScanEmpty);
        const unsigned long long key = (unsigned long long)__double_as_longlong(v);
        bool todo = v == v;                               // NaN: skipped
        uint64_t pending = __builtin_amdgcn_ballot_w64(todo);
        while (pending) {                                 // (uniform) at most 64 distinct values
            const unsigned long long k = __shfl(key, __ffsll((long long)pending) - 1);
            const bool same = todo && key == k;
            pending &= ~__builtin_amdgcn_ballot_w64(same);
            todo = todo && !same;
            if (k != last) {
                if (lane == 0) scan_insert(set, status, k);
                last = k;
            }
        }
    }
}

__global__ void __launch_bounds__(64) scan_priors_rank_kernel(double* priors, int32_t* status) {
    __shared__ double sorted[kVtMaxPriors];
    const int lane = threadIdx.x;
    const unsigned long long k = ((const unsigned long long*)priors)[lane];
    const double v = __longlong_as_double((long long)k);
    const bool occ = k != kScanEmpty;
    const bool over = status[1] != 0;
    int rank = 0;
    for (int s = 0; s < kVtMaxPriors; ++s) {
        const unsigned long long ks = __shfl(k, s);
        const double vs = __longlong_as_double((long long)ks);
        rank += ks != kScanEmpty && (vs < v || (vs == v && ks < k)) ? 1 : 0;
    }
    const int count = __builtin_popcountll(__builtin_amdgcn_ballot_w64(occ));
    sorted[lane] = 0.0;
    __syncthreads();
    if (occ && !over) sorted[rank] = v;                   // (distinct bits: distinct ranks < count)
    __syncthreads();
    priors[lane] = sorted[lane];
    if (lane == 0) {
        status[0] = over ? 0 : count;
        status[1] = over ? 1 : 0;
    }
}
}  // namespace

extern "C" int gnnd_v24_scan_priors(const gnnd_graph* g, int dtype, const void* d_x, int64_t batch,
                                    double* d_priors, int32_t* d_status, void* stream) {
    if (dtype != GNND_F32 && dtype != GNND_F64 && dtype != GNND_BF16) return GNND_ERR_INVALID_ARG;
    if (dtype != GNND_F64) return GNND_ERR_UNSUPPORTED;
    if (!g || !d_priors || !d_status || batch < 0 || (batch > 0 && !d_x)) return GNND_ERR_INVALID_ARG;
    static_assert(kVtMaxPriors == 64, "one wave ranks the set; the hash keeps 6 bits");
    hipStream_t st = (hipStream_t)stream;
    GNND_HIP_CHECK(hipMemsetAsync(d_priors, 0xFF, kVtMaxPriors * sizeof(double), st));
    GNND_HIP_CHECK(hipMemsetAsync(d_status, 0, 2 * sizeof(int32_t), st));
    if (batch > 0) {
        const int64_t blocks = std::min<int64_t>((batch + 255) / 256, 2048);
        scan_priors_insert_kernel<<<(unsigned)blocks, 256, 0, st>>>(
            (const double*)d_x, g->view.xs, g->view.xv0, batch, (unsigned long long*)d_priors, d_status);
        GNND_LAUNCH_CHECK();
    }
    scan_priors_rank_kernel<<<1, 64, 0, st>>>(d_priors, d_status);
    GNND_LAUNCH_CHECK();
    return GNND_OK;
}

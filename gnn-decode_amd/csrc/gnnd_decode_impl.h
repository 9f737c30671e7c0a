// gnnd_decode_impl.h — fused T-iteration GNN / BP decoder kernels (included by the
// per-model translation units gnnd_decode_<model>.hip; C ABI in gnnd_decode.hip).
//
// Restates GNNI.forward of the five reference decoders (paths relative to
// /root/reference/GNN-decode/):
//   CGNNI  classical/CGNNI.py:259-284   (fp32; c->v MLP 1->10->1 ReLU; residual; node MLP)
//   CBP    classical/BP.py:239-259      (fp32; log-domain sum-product, no weights)
//   QBP    quantum/BP.py:199-219        (fp64; syndrome-aware log-domain BP)
//   QGNNI  quantum/QGNNI.py:228-252     (fp64; c->v MLP 1->10->1 ReLU x syndrome; residual)
//   V24    quantum/decoder_v2_4.py:272-294 (fp64 reference; v->c MLP 2->128->1 Softplus,
//          c->v MLP 1->128->1 Softplus x syndrome, residual, per-edge readout MLP)
//   NBP    quantum/neural_BP.py:263-314  (fp64; weighted BP: per-layer per-edge W on the
//          v->c messages and W_p on the prior, residual alpha, weighted readout)
//   V10    quantum/decoder_v1_0.py:282-313 (fp64; per-layer per-edge W on the c->v input,
//          residual alpha)
//
// MI355X mapping.  Every codeword has the same Tanner graph, so the graph tables and the
// weights are staged once per workgroup into LDS and each workgroup decodes a tile of CW
// codewords whose per-edge messages live in LDS for all T iterations: HBM is touched only
// to read x (N values per codeword) and write the V outputs.  An iteration is two phases
// separated by workgroup barriers (see decode_kernel): a check-group phase where G
// consecutive lanes own one check's edges (R per lane), sum the check with a DPP butterfly
// and run both message updates in registers, and a variable-sum phase in the reference's
// index_add order.  The work is VALU/transcendental-bound, so the
// fp32 MLPs run on packed FMAs (v_pk_fma_f32, two hidden units per instruction) with
// weights in VGPRs (10-hidden) or SGPRs (128-hidden, scalar loads), and the fp32 Softplus
// and tanh use the native base-2 v_exp_f32 / v_log_f32 / v_rcp_f32.
#pragma once
#include "gnnd_common.h"
#include <stdlib.h>
#include <type_traits>

namespace {

constexpr float kLog2e = 1.4426950408889634f;
constexpr float kLn2 = 0.6931471805599453f;

// weight offsets in the packed layout (gnnd.h)
constexpr int kV24Ggc1 = 0, kV24Ggc2 = 513, kV24Mlp = 898;
constexpr int kMlp10Msg = 0, kMlp10Out = 31;
constexpr int kV30Count = 137;       // decoder_v3_0 packed weights (gnnd.h)

template <int MODEL> struct ModelTraits {
    static constexpr bool wbp = (MODEL == GNND_NBP || MODEL == GNND_V10 || MODEL == GNND_V22);   // weighted BP
    static constexpr bool bp = (MODEL == GNND_QBP || MODEL == GNND_CBP || wbp);
};

// ---------------------------------------------------------------------------------------
// weighted quantum BP check step (quantum/neural_BP.py:109-122 = decoder_v1_0.py:109-122):
//   t = tanh(a/2) (no pre-clamp), c = [t < 0], L = log(clamp(|t|, 1e-20, 1e10));
//   Lambda = S_c(L) - L, n = S_c(c) - c + (1 - s)/2,
//   p = clamp(exp(Lambda) cos(pi n), +-(1 - 1e-15)), out = log(1 + p) - log(1 - p).
// fp64: literally.  fp32 cannot represent the clamp (1 - 1e-15 rounds to 1, and tanh
// saturates at |a| ~ 17 where fp64 keeps resolving 1 - t down to 1e-16): the fp32 form
// evaluates the same function through the small quantities instead (base-2 log domain,
// native transcendentals):  log2 tanh(|a|/2) via -2 atanh(e)/ln2, e = exp(-|a|), for
// small e;  1 - |p| = -expm1(Lambda) clamped at 1 - fl64(1 - 1e-15);  so messages track
// the fp64 reference instead of saturating at log(2^25).
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ double wbp_L(double a, double& c) {
    const double t = g_tanh(a / 2.0);
    c = t < 0.0 ? 1.0 : 0.0;
    return g_log(g_clamp(fabs(t), 1e-20, 1e10));
}
// fp32: BASE-2 log magnitude log2|tanh(a/2)| on the native v_exp/v_log/v_rcp, resolving
// 1 - |t| down to fp32's range (fp64 resolves it down to 1e-16; fp32 tanh itself would
// round to 1 from |a| ~ 17):  z = |a|/2 < 0.3: odd Taylor polynomial of tanh (5e-8 rel);
// e = exp(-|a|) >= 1/16: log2((1 - e) / (1 + e)) (1 - e >= 0.45: ~2 ulp);
// e < 1/16: -2 atanh(e) / ln2 by its series to e^7 (~1e-9 relative to the result).
__device__ __forceinline__ float wbp_L(float a, float& c) {
    c = a < 0.f ? 1.f : 0.f;                  // tanh(a/2) < 0 exactly when a < 0
    const float y = fabsf(a), z = 0.5f * y, z2 = z * z;
    float tp = __builtin_fmaf(z2, 62.f / 2835.f, -17.f / 315.f);
    tp = __builtin_fmaf(z2, tp, 2.f / 15.f);
    tp = __builtin_fmaf(z2, tp, -1.f / 3.f);
    tp = __builtin_fmaf(z2 * z, tp, z);
    const float e = __builtin_amdgcn_exp2f(-y * kLog2e);
    const float te = (1.f - e) * __builtin_amdgcn_rcpf(1.f + e);
    const float e2 = e * e;
    float at = __builtin_fmaf(e2, 1.f / 7.f, 1.f / 5.f);
    at = __builtin_fmaf(e2, at, 1.f / 3.f);
    at = __builtin_fmaf(e2 * e, at, e);                       // atanh(e)
    const float lsmall = at * (-2.f * kLog2e);
    // one log: of the polynomial (z < 0.3) or of (1 - e)/(1 + e); e < 1/16 implies z > 1.38
    const float l = __builtin_amdgcn_logf(z < 0.3f ? fmaxf(tp, 1e-20f) : te);
    return e >= 0.0625f ? l : lsmall;
}
// the same on two edges, non-transcendental ops packed (paired check step)
__device__ __forceinline__ f32x2 wbp_L2(f32x2 a, f32x2& c) {
    c = f32x2{a.x < 0.f ? 1.f : 0.f, a.y < 0.f ? 1.f : 0.f};
    const f32x2 y = {fabsf(a.x), fabsf(a.y)};
    const f32x2 z = y * 0.5f, z2 = z * z;
    f32x2 tp = __builtin_elementwise_fma(z2, f32x2{62.f / 2835.f, 62.f / 2835.f},
                                         f32x2{-17.f / 315.f, -17.f / 315.f});
    tp = __builtin_elementwise_fma(z2, tp, f32x2{2.f / 15.f, 2.f / 15.f});
    tp = __builtin_elementwise_fma(z2, tp, f32x2{-1.f / 3.f, -1.f / 3.f});
    tp = __builtin_elementwise_fma(z2 * z, tp, z);
    const f32x2 ya = y * (-kLog2e);
    const f32x2 e = {__builtin_amdgcn_exp2f(ya.x), __builtin_amdgcn_exp2f(ya.y)};
    const f32x2 d = f32x2{1.f, 1.f} + e;
    const f32x2 te = (f32x2{1.f, 1.f} - e) * f32x2{__builtin_amdgcn_rcpf(d.x), __builtin_amdgcn_rcpf(d.y)};
    const f32x2 e2 = e * e;
    f32x2 at = __builtin_elementwise_fma(e2, f32x2{1.f / 7.f, 1.f / 7.f}, f32x2{1.f / 5.f, 1.f / 5.f});
    at = __builtin_elementwise_fma(e2, at, f32x2{1.f / 3.f, 1.f / 3.f});
    at = __builtin_elementwise_fma(e2 * e, at, e);
    const f32x2 lsmall = at * (-2.f * kLog2e);
    const f32x2 l = {__builtin_amdgcn_logf(z.x < 0.3f ? fmaxf(tp.x, 1e-20f) : te.x),
                     __builtin_amdgcn_logf(z.y < 0.3f ? fmaxf(tp.y, 1e-20f) : te.y)};
    return f32x2{e.x >= 0.0625f ? l.x : lsmall.x, e.y >= 0.0625f ? l.y : lsmall.y};
}
__device__ __forceinline__ double wbp_out(double lam, double n, double s) {
    n = n + (1.0 - s) / 2.0;
    const double hi = 1 - 1e-15;
    const double p = g_clamp(g_exp(lam) * cos_pi(n), -hi, hi);
    return g_log(1.0 + p) - g_log(1.0 - p);
}
// fp32: lam2 = base-2 leave-one-out log magnitude (<= 0), |p| = 2^lam2.  1 - |p| through
// expm1 (degree-8 Taylor for |lam| < 0.35) so it stays accurate as |p| -> 1, clamped at
// 1 - fl64(1 - 1e-15) like the fp64 reference's p clamp.
__device__ __forceinline__ float wbp_out(float lam2, float n, float s) {
    n = n + (1.f - s) / 2.f;
    const float sgn = cos_pi(n);
    const float q = __builtin_amdgcn_exp2f(lam2);
    const float x = lam2 * kLn2;                              // natural log of |p|, <= 0
    float em = __builtin_fmaf(x, 1.f / 40320.f, 1.f / 5040.f);
    em = __builtin_fmaf(x, em, 1.f / 720.f);
    em = __builtin_fmaf(x, em, 1.f / 120.f);
    em = __builtin_fmaf(x, em, 1.f / 24.f);
    em = __builtin_fmaf(x, em, 1.f / 6.f);
    em = __builtin_fmaf(x, em, 0.5f);
    em = __builtin_fmaf(x * x, em, x);                        // expm1(x)
    float one_m = x > -0.35f ? -em : 1.f - q;
    one_m = fmaxf(one_m, 9.992007221626409e-16f);
    const float one_p = fminf(1.f + q, 2.f - 9.992007221626409e-16f);
    return sgn * (kLn2 * (__builtin_amdgcn_logf(one_p) - __builtin_amdgcn_logf(one_m)));
}
__device__ __forceinline__ f32x2 wbp_out2(f32x2 lam2, f32x2 n, f32x2 s) {
    n = __builtin_elementwise_fma(f32x2{1.f, 1.f} - s, f32x2{0.5f, 0.5f}, n);
    const f32x2 h = n * 0.5f;                                 // (-1)^n, n integer-valued
    const f32x2 par = __builtin_elementwise_fma(f32x2{__builtin_floorf(h.x), __builtin_floorf(h.y)},
                                                f32x2{-2.f, -2.f}, n);
    const f32x2 sgn = __builtin_elementwise_fma(par, f32x2{-2.f, -2.f}, f32x2{1.f, 1.f});
    const f32x2 q = {__builtin_amdgcn_exp2f(lam2.x), __builtin_amdgcn_exp2f(lam2.y)};
    const f32x2 x = lam2 * kLn2;
    f32x2 em = __builtin_elementwise_fma(x, f32x2{1.f / 40320.f, 1.f / 40320.f}, f32x2{1.f / 5040.f, 1.f / 5040.f});
    em = __builtin_elementwise_fma(x, em, f32x2{1.f / 720.f, 1.f / 720.f});
    em = __builtin_elementwise_fma(x, em, f32x2{1.f / 120.f, 1.f / 120.f});
    em = __builtin_elementwise_fma(x, em, f32x2{1.f / 24.f, 1.f / 24.f});
    em = __builtin_elementwise_fma(x, em, f32x2{1.f / 6.f, 1.f / 6.f});
    em = __builtin_elementwise_fma(x, em, f32x2{0.5f, 0.5f});
    em = __builtin_elementwise_fma(x * x, em, x);
    const f32x2 qm = f32x2{1.f, 1.f} - q, qp = f32x2{1.f, 1.f} + q;
    const float lo = 9.992007221626409e-16f, hi = 2.f - 9.992007221626409e-16f;
    const f32x2 one_m = {fmaxf(x.x > -0.35f ? -em.x : qm.x, lo), fmaxf(x.y > -0.35f ? -em.y : qm.y, lo)};
    const f32x2 one_p = {fminf(qp.x, hi), fminf(qp.y, hi)};
    const f32x2 l = f32x2{__builtin_amdgcn_logf(one_p.x), __builtin_amdgcn_logf(one_p.y)} -
                    f32x2{__builtin_amdgcn_logf(one_m.x), __builtin_amdgcn_logf(one_m.y)};
    return sgn * (l * kLn2);
}
// per-edge weights of iteration t (reference edge order; NBP [T][2][E] + readout, V10 [T][E])
template <int MODEL, typename T> struct WbpW {
    const T* __restrict__ w;
    int E, T_;
    __device__ __forceinline__ T msg(int t, int e) const { return w[(size_t)2 * t * E + e]; }      // NBP W
    __device__ __forceinline__ T prior(int t, int e) const { return w[(size_t)(2 * t + 1) * E + e]; }  // NBP W_p
    __device__ __forceinline__ T chk(int t, int e) const { return w[(size_t)t * E + e]; }          // V10 W
    __device__ __forceinline__ T out_w(int e) const { return w[(size_t)2 * T_ * E + e]; }          // NBP W
    __device__ __forceinline__ T out_p(int e) const { return w[(size_t)(2 * T_ + 1) * E + e]; }    // NBP W_p
    __device__ __forceinline__ T alpha() const {
        return MODEL == GNND_V10 ? w[(size_t)T_ * E] : w[(size_t)2 * T_ * E + 2 * E];
    }
};

// torch constants are Python doubles converted to the tensor dtype
template <typename T> __device__ __forceinline__ T cst(double v) { return (T)v; }

// ---------------------------------------------------------------------------------------
// per-edge MLPs (torch.nn.Linear y = x W^T + b)
// ---------------------------------------------------------------------------------------
// Linear(1,10) -> ReLU -> Linear(10,1); w = {W1[10], b1[10], W2[10], b2}   (scalar form)
template <typename T>
__device__ __forceinline__ T mlp10_relu(const T* w, T u) {
    T acc = T(0);
#pragma unroll
    for (int k = 0; k < 10; ++k) {
        T h = g_fma(u, w[k], w[10 + k]);
        acc = g_fma(fmax(h, T(0)), w[20 + k], acc);
    }
    return acc + w[30];
}

// fp32 form with the 31 weights held in VGPRs.  ReLU is folded into the first FMA as the
// hardware [0, 1] output clamp: unit k is evaluated as clamp(fma(u, W1_k 2^-s_k, b1_k 2^-s_k))
// and weighted by W2_k 2^s_k, where 2^s_k > |W1_k| umax + |b1_k| bounds the pre-activation
// over the input range |u| <= umax.  Scaling by a power of two commutes with the rounding
// of the FMA and of the product, so every unit's contribution is bit-identical to
// W2_k relu(fma(u, W1_k, b1_k)); the clamp saves the separate max.  The second layer
// accumulates two units per v_pk_fma_f32.
__device__ __forceinline__ float uniform(float x) {
    return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(x)));
}
struct Mlp10F32 {
    f32x2 w1[5], b1[5], w2[5];
    float b2;
    __device__ __forceinline__ void load(const float* w, float umax) {
#pragma unroll
        for (int k = 0; k < 10; ++k) {
            int e;
            frexpf(fabsf(w[k]) * umax + fabsf(w[10 + k]), &e);    // 2^e > bound
            // wave-uniform: readfirstlane puts the weights in SGPRs (one scalar operand per
            // packed op), leaving the VGPRs to the resident messages
            const float a = uniform(ldexpf(w[k], -e)), b = uniform(ldexpf(w[10 + k], -e)),
                        v = uniform(ldexpf(w[20 + k], e));
            if (k & 1) { w1[k >> 1].y = a; b1[k >> 1].y = b; w2[k >> 1].y = v; }
            else       { w1[k >> 1].x = a; b1[k >> 1].x = b; w2[k >> 1].x = v; }
        }
        b2 = uniform(w[30]);
    }
    // The two accumulator halves are combined by one scalar add in asm: hipcc otherwise
    // SLP-packs the combines of neighbouring edges into v_mov shuffles + v_pk_add (2 ops per
    // edge instead of 1).  (Folding CGNNI's residual into the accumulator as well saves one
    // more op but spills VGPRs in the 128-register resident kernel: measured slower.)
    __device__ __forceinline__ float operator()(float u) const {
        f32x2 acc = {b2, 0.f};                 // bias rides in the even-unit accumulator
        f32x2 uu;                              // only the lo half is read (op_sel_hi 0)
        uu.x = u;
#pragma unroll
        for (int k = 0; k < 5; ++k) {
#ifdef GNND_SCALAR_CLAMP
            const f32x2 h = {__builtin_amdgcn_fmed3f(__builtin_fmaf(u, w1[k].x, b1[k].x), 0.f, 1.f),
                             __builtin_amdgcn_fmed3f(__builtin_fmaf(u, w1[k].y, b1[k].y), 0.f, 1.f)};
#else
            // hipcc does not fold a clamp into v_pk_fma_f32: one packed FMA + clamp in asm
            f32x2 h;
            asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel_hi:[0,1,1] clamp"
                : "=v"(h) : "v"(uu), "s"(w1[k]), "v"(b1[k]));
#endif
            acc = __builtin_elementwise_fma(h, w2[k], acc);
        }
        float r;
        asm("v_add_f32 %0, %1, %2" : "=v"(r) : "v"(acc.x), "v"(acc.y));
        return r;
    }
};

// fp64 reference forms: Linear(1,128)/Linear(2,128) -> Softplus -> Linear(128,1); the
// Softplus is the table-driven form at the parity contract's accuracy (softplus_v24: the one-read
// kSpTab polynomial; tab = the kernel's LDS copy of its table)
// the unit's bias into a VGPR pair with ONE v_mov_b64 (its weight stays an SGPR operand of the
// layer-1 FMA: VOP3 takes one scalar operand)
__device__ __forceinline__ double vgpr_of(double s) {
    double d;
    asm("v_mov_b64 %0, %1" : "=v"(d) : "s"(s));
    return d;
}
// compile-time loop: f(std::integral_constant<int, i>) for i = 0 .. N-1
template <int N, typename F, int I = 0> __device__ __forceinline__ void static_for(F&& f) {
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        static_for<N, F, I + 1>(static_cast<F&&>(f));
    }
}
// The 128 units are summed in a FIXED order independent of how they are spread over waves:
// chain j (0..3) accumulates units k = 4i + j (i ascending) from 0, and the MLP value is
// ((c0 + c1) + (c2 + c3)) + b2.  A call evaluates NC consecutive chains from J0 (NC = 4: the
// whole MLP; 2 / 1: the half / quarter a unit-split wave owns, mlp128d_split), so every split
// gives the same bits.  Layouts (plain packed weights): 1-input {W1[128], b1[128], W2[128], b2},
// 2-input (TWO: u0 -> W1[:, 0], u1 -> W1[:, 1]) {W1a[128], W1b[128], b1[128], W2[128], b2}.
// bl: the MLP's 128 layer-1 biases staged in LDS (a broadcast ds_read_b64 per unit: VOP3 takes
// one scalar operand, so a bias from SGPRs costs a v_mov_b64 per unit); tab: the Softplus
// table in LDS (softplus_v24).
template <int NC, int J0, bool TWO, bool SAFE = false>
__device__ __forceinline__ double mlp128d_chains(const double* __restrict__ w, const double* bl,
                                                 double u0, double u1, const double* tab) {
    constexpr int kW2 = TWO ? 384 : 256;
    double c[NC];
#pragma unroll
    for (int jj = 0; jj < NC; ++jj) c[jj] = 0.0;
    constexpr int kUnroll = 4 / NC;                          // 4 units per loop trip
#pragma unroll kUnroll
    for (int i = 0; i < 32; ++i) {
        static_for<NC>([&](auto jc) {
            constexpr int jj = decltype(jc)::value;
            const int k = 4 * i + J0 + jj;
            double h;
            if constexpr (TWO) h = fma_vsv(u0, w[k], fma_vsv(u1, w[128 + k], bl[k]));
            else h = fma_vsv(u0, w[k], bl[k]);
            c[jj] = fma(softplus_v24_half<SAFE>(h, tab), w[kW2 + k], c[jj]);
        });
    }
    if constexpr (NC == 4) return (c[0] + c[1]) + (c[2] + c[3]);
    else if constexpr (NC == 2) return c[0] + c[1];
    else return c[0];
}
// the unit-split form's weights (US > 1): each MLP's units staged in LDS CHAIN-major (unit
// k = 4 i + j at entry 32 j + i, {W1a, W1b, b1, W2} per entry), so a wave's chain reads
// consecutive entries as broadcast ds_read_b128s — from global memory a chain's units are
// 4 apart, one scalar load and one wait per weight (measured: 11 lgkmcnt(0) waits per 4 units)
struct WcmEntry {
    double w1a, w1b, b1, w2;
};
// FAIR (the unit split, GNND_FWD_FAIR, default 1): the wave lowers its issue priority as it walks
// its units (3 -> 1, then 0 before the partials meet), so the SIMD's younger waves are not left
// to finish their units alone (the arbiter issues oldest-first; v24_bwd_kernel's GNND_BWD_FAIR).
// Same-box A/B (r05k, config-5 step at B = 128): fp32 0.1766 -> 0.1743 ms, fp64 0.3908 -> 0.3845
#ifndef GNND_FWD_FAIR
#define GNND_FWD_FAIR 1
#endif
template <int NC, int J0, bool TWO, bool FAIR = false, bool SAFE = false>
__device__ __forceinline__ double mlp128d_chains_cm(const WcmEntry* wl, double u0, double u1,
                                                    const double* tab) {
    constexpr int UT = 4, NU = 32 * NC;       // units per stage (NC divides UT), per call
    static_assert(UT % NC == 0, "stage holds whole chain groups");
    double c[NC];
#pragma unroll
    for (int jj = 0; jj < NC; ++jj) c[jj] = 0.0;
#pragma unroll 2
    for (int t0 = 0; t0 < NU; t0 += UT) {
        if constexpr (FAIR) {            // (mlp128_upair's FAIR, in thirds of the units)
            if (t0 == 0) __builtin_amdgcn_s_setprio(3);
            if (t0 == (NU / UT / 3) * UT) __builtin_amdgcn_s_setprio(2);
            if (t0 == (2 * NU / UT / 3) * UT) __builtin_amdgcn_s_setprio(1);
        }
        WcmEntry e[UT];
        double h[UT];
        SpIdx q[UT];
        SpEntry t[UT];
#pragma unroll
        for (int s = 0; s < UT; ++s) e[s] = wl[(J0 + s % NC) * 32 + t0 / NC + s / NC];
#pragma unroll
        for (int s = 0; s < UT; ++s) {
            h[s] = TWO ? fma(u0, e[s].w1a, fma(u1, e[s].w1b, e[s].b1)) : fma(u0, e[s].w1a, e[s].b1);
            q[s] = v24_sp_index<SAFE>(h[s]);
        }
#pragma unroll
        for (int s = 0; s < UT; ++s) t[s] = sp_entry(tab, q[s].j);
#pragma unroll
        for (int s = 0; s < UT; ++s) {
            const double g = GNND_F64_LINFOLD ? v24_sp_half(q[s], t[s], h[s])
                                              : relu_f64(h[s]) + sp_poly(q[s].r, t[s].f0, t[s].s);
            c[s % NC] = fma(g, e[s].w2, c[s % NC]);
        }
    }
    if constexpr (FAIR) __builtin_amdgcn_s_setprio(0);
    if constexpr (NC == 2) return c[0] + c[1];
    else return c[0];
}
// the linear half of the MLP's relu terms (softplus_v24_half leaves out h/2):
// sum_k W2_k h_k / 2 = u0 A + u1 B + C, ln = {A, B, C} staged per MLP (decode_kernel prologue);
// added after the fixed chain tree, before b2, in every split (the same bits)
template <bool TWO>
__device__ __forceinline__ double mlp_lin(const double* ln, double u0, double u1) {
    if (!GNND_F64_LINFOLD) return 0.0;
    return TWO ? fma(u0, ln[0], fma(u1, ln[1], ln[2])) : fma(u0, ln[0], ln[2]);
}
// The MLP's pre-activation bound |h_k| <= max(|u0|, |u1|, 1) ln[3], ln[3] = max_k (|W1a_k| +
// |W1b_k| + |b1_k|) (decode_kernel prologue): a wave with a lane at 2^25 or above takes the
// sg_index_safe units (the same bits wherever sg_index is valid)
__device__ __forceinline__ bool mlp_wave_big(const double* ln, double u0, double u1) {
    const bool big = fmax(fmax(fabs(u0), fabs(u1)), 1.0) * ln[3] >= 0x1p25;
    return __builtin_amdgcn_ballot_w64(big) != 0;
}
__device__ __forceinline__ double mlp128_sp(const double* w, const double* bl, double u,
                                            const double* tab, const double* ln) {
    const double c = mlp_wave_big(ln, u, u) ? mlp128d_chains<4, 0, false, true>(w, bl, u, u, tab)
                                            : mlp128d_chains<4, 0, false>(w, bl, u, u, tab);
    return (c + mlp_lin<false>(ln, u, u)) + w[384];
}
// unit-split evaluation of the fp64 MLPs (decode_kernel US > 1, fp64 decoder_v2_4 small
// batches): wave `sub` evaluates chain group sub, the US partial sums meet in LDS (buf = [US][256]
// doubles, one of two buffers used alternately) and combine in the chain tree above.  Every
// thread of the workgroup must call it (barrier); idle (wave-uniform): no live work item in this
// wave, the units are skipped.
template <int US, bool TWO>
__device__ __forceinline__ double mlp128d_split(const double* __restrict__ w, const double* bl,
                                                double u0, double u1, int sub, double* buf,
                                                int itid, bool idle, const double* tab,
                                                const double* ln, const WcmEntry* wl = nullptr) {
    constexpr int kB2 = TWO ? 512 : 384;
    if constexpr (US == 1) {
        if (idle) return 0.0;
        const double c = mlp_wave_big(ln, u0, u1) ? mlp128d_chains<4, 0, TWO, true>(w, bl, u0, u1, tab)
                                                  : mlp128d_chains<4, 0, TWO>(w, bl, u0, u1, tab);
        return (c + mlp_lin<TWO>(ln, u0, u1)) + w[kB2];
    } else {
        static_assert(US == 2 || US == 4, "fp64 unit split 1, 2 or 4");
        constexpr int NC = 4 / US, IL = GNND_BLOCK;
        double p = 0.0;
        if (!idle) {
#if GNND_F64_SPTAB
            constexpr bool F = GNND_FWD_FAIR;
            if (mlp_wave_big(ln, u0, u1)) {
                switch (sub) {
                    case 0: p = mlp128d_chains_cm<NC, 0, TWO, F, true>(wl, u0, u1, tab); break;
                    case 1: p = mlp128d_chains_cm<NC, NC, TWO, F, true>(wl, u0, u1, tab); break;
                    case 2: if constexpr (US == 4) p = mlp128d_chains_cm<1, 2, TWO, F, true>(wl, u0, u1, tab); break;
                    default: if constexpr (US == 4) p = mlp128d_chains_cm<1, 3, TWO, F, true>(wl, u0, u1, tab); break;
                }
            } else {
                switch (sub) {
                    case 0: p = mlp128d_chains_cm<NC, 0, TWO, F>(wl, u0, u1, tab); break;
                    case 1: p = mlp128d_chains_cm<NC, NC, TWO, F>(wl, u0, u1, tab); break;
                    case 2: if constexpr (US == 4) p = mlp128d_chains_cm<1, 2, TWO, F>(wl, u0, u1, tab); break;
                    default: if constexpr (US == 4) p = mlp128d_chains_cm<1, 3, TWO, F>(wl, u0, u1, tab); break;
                }
            }
#else
            switch (sub) {
                case 0: p = mlp128d_chains<NC, 0, TWO>(w, bl, u0, u1, tab); break;
                case 1: p = mlp128d_chains<NC, NC, TWO>(w, bl, u0, u1, tab); break;
                case 2: if constexpr (US == 4) p = mlp128d_chains<1, 2, TWO>(w, bl, u0, u1, tab); break;
                default: if constexpr (US == 4) p = mlp128d_chains<1, 3, TWO>(w, bl, u0, u1, tab); break;
            }
#endif
        }
        buf[sub * IL + itid] = p;
        __syncthreads();
        double r;
        if constexpr (US == 2) r = buf[itid] + buf[IL + itid];
        else r = (buf[itid] + buf[IL + itid]) + (buf[2 * IL + itid] + buf[3 * IL + itid]);
        return (r + mlp_lin<TWO>(ln, u0, u1)) + w[kB2];
    }
}

// ---------------------------------------------------------------------------------------
// decoder_v2_4's check-side MLP as a table (fp64).  ggc2.mlp (Linear(1, 128)
// -> Softplus -> Linear(128, 1), quantum/decoder_v2_4.py:241-243, :253-257) is applied to ONE
// scalar u = S_c(tanh(m/2)) - tanh(m_e/2) (:135-136), a sum of at most dc - 1 values in
// [-1, 1]: |u| <= R = max_dc - 1.  f(u) = W2 . softplus(W1 u + b1) + b2 is analytic there, so
// gnnd_prepare_weights (and gnnd_train_update after every optimizer step) tabulates it once per
// weight set in the prepared layout, as degree-11 Taylor polynomials about c_j = j / 8 for
// |c_j| <= kCtabRcap (ctab_build_kernel), and the decoder stages the entries its graph needs
// (|c_j| <= R) in LDS and evaluates f as one index (4 VALU), one 96-byte entry (6
// ds_read_b128) and 11 FMAs instead of 128 hidden units (~16 VALU each).
// Coefficients a_n = sum_k W2_k W1_k^n softplus^(n)(h_k) / n!, h_k = W1_k c_j + b1_k, from the
// exact derivatives: softplus' = sigma, sigma^(n) = tau U_n(q), tau = sigma (1 - sigma) =
// e / (1 + e)^2 with e = exp(-|h|) (no cancellation at large |h|), q = 1 - 2 sigma, U_1 = 1,
// U_{n+1} = q U_n - (1 - q^2) U_n' / 2.  Remainder <= (1/16)^12 / 12! * max|sigma^(11)| (= 86.375)
// * sum_k |W2_k| |W1_k|^12: 7.4e-16 for the reference's epoch-67 weights.  The decoder uses the
// table only when that bound is <= 1e-13 and no unit's pre-activation crosses torch's Softplus
// threshold 20 for some u in [-R, R] (the jump there is not polynomial); otherwise it evaluates
// the 128 units (ctab_valid).
// ---------------------------------------------------------------------------------------
#ifndef GNND_V24_CTAB
#define GNND_V24_CTAB 1          // 0: the per-unit check MLP everywhere (A/B builds)
#endif
constexpr int kCtabInv = 8;                  // centres c_j = j / kCtabInv
constexpr int kCtabNC = 12;                  // Taylor coefficients a_0 .. a_11 per entry
constexpr int kCtabRcap = 31;                // prepared table: |c_j| <= 31 (max_dc <= 32)
constexpr int kCtabCap = 2 * kCtabInv * kCtabRcap + 1;               // 497 entries
constexpr int kV24CtabOff = 1288;            // doubles: prepared fp64 V24 = [1283 plain | pad | table]
constexpr int kV24PreparedF64 = kV24CtabOff + kCtabCap * kCtabNC;    // 7 252
// then the channel-prior section (vtab_*, below): [kV24PriorHdr] = number of prior tables (0
// unless gnnd_prepare_weights_priors built them), pad to kV24PriorOff, the tables
constexpr int kV24PriorHdr = kV24PreparedF64;
constexpr int kV24PriorOff = kV24PriorHdr + 12;                      // 7 264 (128-B aligned): the V24 prepared count
// (1/16)^12 / 12! * max|sigma^(11)|: the remainder bound per unit of sum |W2| |W1|^12
constexpr double kCtabBoundCoef = 86.375 / 479001600.0 / 281474976710656.0;
__host__ __device__ constexpr int ctab_entries(int max_dc) {
    return 2 * kCtabInv * (max_dc > 1 ? max_dc - 1 : 0) + 1;
}
// U_n(q) / (n + 1)!  for n = 1..10 (softplus^(n+1) / (n+1)! = tau U_n(q) / (n+1)!); U_n has the
// parity of n - 1, so each is a polynomial in q^2 (times q for even n)
__device__ __forceinline__ double ctab_un(int n, double q, double q2) {
    switch (n) {
        case 1: return 1.0 / 2;
        case 2: return q * (1.0 / 6);
        case 3: return fma(q2, 1.5, -0.5) * (1.0 / 24);
        case 4: return q * fma(q2, 3.0, -2.0) * (1.0 / 120);
        case 5: return fma(q2, fma(q2, 7.5, -7.5), 1.0) * (1.0 / 720);
        case 6: return q * fma(q2, fma(q2, 22.5, -30.0), 8.5) * (1.0 / 5040);
        case 7: return fma(q2, fma(q2, fma(q2, 78.75, -131.25), 57.75), -4.25) * (1.0 / 40320);
        case 8: return q * fma(q2, fma(q2, fma(q2, 315.0, -630.0), 378.0), -62.0) * (1.0 / 362880);
        case 9: return fma(q2, fma(q2, fma(q2, fma(q2, 1417.5, -3307.5), 2520.0), -660.0), 31.0) *
                       (1.0 / 3628800);
        default: return q * fma(q2, fma(q2, fma(q2, fma(q2, 7087.5, -18900.0), 17482.5), -6360.0), 691.0) *
                        (1.0 / 39916800);
    }
}
// softplus^(n)(h) / n!, n = 0 .. kCtabNC - 1, of the smooth function (no threshold)
__device__ __forceinline__ void softplus_taylor(double h, double (&d)[kCtabNC]) {
    const double e = exp(-fabs(h));
    const double sv = 1.0 / (1.0 + e);
    const double tau = e * sv * sv;
    const double q = h >= 0.0 ? (e - 1.0) * sv : (1.0 - e) * sv;
    const double q2 = q * q;
    d[0] = fmax(h, 0.0) + log1p(e);
    d[1] = h >= 0.0 ? sv : e * sv;
#pragma unroll
    for (int n = 2; n < kCtabNC; ++n) d[n] = tau * ctab_un(n - 1, q, q2);
}
// One entry per block (blockIdx.x = j + kCtabInv kCtabRcap), one hidden unit per thread (128):
// w = plain packed V24 weights (ggc2.mlp at kV24Ggc2; may alias prep), prep = the prepared
// buffer: table [kCtabCap][kCtabNC] at kV24CtabOff, and block 0 also writes prep[1283] = the
// remainder bound (kCtabBoundCoef sum |W2| |W1|^12) and prep[1284] = the smallest distance, over
// the units, of their pre-activation's crossing of torch's threshold 20 from u = 0 ((20 - b1) /
// |W1|): the table holds for R below it.  The 128-unit sums run as two fixed 64-lane
// butterflies and one fixed add: the same bits on every launch.
__device__ __forceinline__ double group_min64(double v) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) v = fmin(v, __shfl_xor(v, o));
    return v;
}
// TP = float (the fp32 decoder's table, fp32 coefficients from the same fp64 sums): the fp32
// kernels evaluate Softplus without torch's threshold (its jump, 2e-9, is below fp32's
// resolution at 20), so the table is the smooth function everywhere and prep[1284] = 1e30
template <typename TW, typename TP>
__global__ void __launch_bounds__(128) ctab_build_kernel(const TW* w, TP* prep) {
    constexpr bool kThr = sizeof(TP) == 8;     // torch's threshold (fp64 decoder)
    const TW* wm = w + kV24Ggc2;
    const int k = threadIdx.x, j = blockIdx.x;
    const double c = (double)(j - kCtabInv * kCtabRcap) * (1.0 / kCtabInv);
    const double W1 = wm[k], b1 = wm[128 + k], W2 = wm[256 + k], b2 = wm[384];
    const double h = fma(W1, c, b1);
    double d[kCtabNC];
    if (kThr && h > 20.0) {                    // torch's threshold: softplus(h) = h
        d[0] = h;
        d[1] = 1.0;
#pragma unroll
        for (int n = 2; n < kCtabNC; ++n) d[n] = 0.0;
    } else {
        softplus_taylor(h, d);
    }
    __shared__ double part[kCtabNC + 2];
    double t[kCtabNC];
    double p = W2;
#pragma unroll
    for (int n = 0; n < kCtabNC; ++n) {
        t[n] = group_sum_c<64>(p * d[n]);
        p *= W1;
    }
    double s12 = 0.0, rk = 0.0;
    if (j == 0) {                              // (uniform)
        const double w2 = W1 * W1, w4 = w2 * w2;
        s12 = group_sum_c<64>(fabs(W2) * (w4 * w4 * w4));
        const double a = fabs(W1);
        rk = group_min64(a > 0.0 ? fabs(20.0 - b1) / a : (b1 == 20.0 ? 0.0 : 1e300));
    }
    if (k == 64) {
#pragma unroll
        for (int n = 0; n < kCtabNC; ++n) part[n] = t[n];
        part[kCtabNC] = s12;
        part[kCtabNC + 1] = rk;
    }
    __syncthreads();
    if (k == 0) {
        TP* en = prep + kV24CtabOff + (size_t)j * kCtabNC;
#pragma unroll
        for (int n = 0; n < kCtabNC; ++n) en[n] = (TP)((t[n] + part[n]) + (n == 0 ? b2 : 0.0));
        if (j == 0) {
            prep[1283] = (TP)((s12 + part[kCtabNC]) * kCtabBoundCoef);
            prep[1284] = (TP)(kThr ? fmin(rk, part[kCtabNC + 1]) : 1e30);
            for (int i = 1285; i < kV24CtabOff; ++i) prep[i] = TP(0);   // (defined padding)
            // no channel-prior tables (a weight update leaves any earlier ones stale)
            for (int i = kV24PriorHdr; i < kV24PriorOff; ++i) prep[i] = TP(0);
        }
    }
}
// the table of the plain weights w into the prepared buffer prep (w may alias prep for fp64;
// fp32: w = the plain weights, prep's head holds the base-2 rescaled ones)
template <typename TW, typename TP>
int launch_ctab_build(const TW* w, TP* prep, hipStream_t st) {
    ctab_build_kernel<TW, TP><<<kCtabCap, 128, 0, st>>>(w, prep);
    GNND_LAUNCH_CHECK();
    return GNND_OK;
}
// Whether the prepared table holds for a graph with |u| <= R (w = the prepared weights): no
// unit's pre-activation reaches 20 for |u| <= R unless it stays above 20 there (a crossing at
// distance rk from u = 0 lies outside [-R, R] iff R < rk), and the remainder bound <= 1e-13
template <typename T>
__device__ __forceinline__ bool ctab_valid(const T* __restrict__ w, int R) {
    return GNND_V24_CTAB && R <= kCtabRcap && w[1283] <= T(1e-13) && (T)R < w[1284];
}
// MLP_c(u) from the staged entries (tab[0] at c = -R, R8 = kCtabInv R): the nearest centre,
// then Horner in r = u - c_j
__device__ __forceinline__ double ctab_eval(const double* tab, double u, int R8) {
    int k = round_magic_lo(__builtin_fma(u, (double)kCtabInv, kRoundMagic));
    k = k < -R8 ? -R8 : (k > R8 ? R8 : k);                    // (u is within [-R, R] + rounding)
    const double r = __builtin_fma((double)k, -1.0 / kCtabInv, u);
    const double2* e = (const double2*)(tab + (size_t)(k + R8) * kCtabNC);
    double a[kCtabNC];
#pragma unroll
    for (int i = 0; i < kCtabNC / 2; ++i) {
        const double2 v = e[i];
        a[2 * i] = v.x;
        a[2 * i + 1] = v.y;
    }
    double p = a[kCtabNC - 1];
#pragma unroll
    for (int n = kCtabNC - 2; n >= 0; --n) p = fma(p, r, a[n]);
    return p;
}
// the fp32 form (fp32 V24 decoder): the same nearest centre (round to nearest by the 1.5 2^23
// magic), three ds_read_b128 of fp32 coefficients, Horner in fp32
__device__ __forceinline__ float ctab_eval(const float* tab, float u, int R8) {
    const float tk = __builtin_fmaf(u, (float)kCtabInv, 12582912.f);   // 1.5 2^23
    int k = (int)(__float_as_uint(tk) & 0x7fffffu) - 0x400000;
    k = k < -R8 ? -R8 : (k > R8 ? R8 : k);
    const float r = __builtin_fmaf((float)k, -1.f / kCtabInv, u);
    const float4* e = (const float4*)(tab + (size_t)(k + R8) * kCtabNC);
    float a[kCtabNC];
#pragma unroll
    for (int i = 0; i < kCtabNC / 4; ++i) {
        const float4 v = e[i];
        a[4 * i] = v.x; a[4 * i + 1] = v.y; a[4 * i + 2] = v.z; a[4 * i + 3] = v.w;
    }
    float p = a[kCtabNC - 1];
#pragma unroll
    for (int n = kCtabNC - 2; n >= 0; --n) p = __builtin_fmaf(p, r, a[n]);
    return p;
}

// ---------------------------------------------------------------------------------------
// decoder_v2_4's variable-side MLP per channel prior (fp64).  ggc1.mlp (Linear(2, 128) ->
// Softplus -> Linear(128, 1), quantum/decoder_v2_4.py:237-239, :253-255) takes (u, x_v), u =
// S_v - m_e; the reference's inputs carry ONE prior per codeword, x_v = log((1 - p) / p) with p
// from a short list (quantum/error_generate.py:252-260 gen_syn), so for a fixed x it is a
// one-input MLP with biases b1' = W1b x + b1.  gnnd_prepare_weights_priors tabulates it per
// prior value over |u| <= kVtR as degree-7 Taylor polynomials about c_j = j / INV (INV = 16),
// one cell per centre -- like the check-side table, except that u is not bounded by the graph,
// so units DO cross torch's Softplus threshold 20 inside the range.  Each cell classifies the
// units over its interval |u - c_j| <= 1/(2 INV): h > 20 throughout -> the unit is exactly
// linear (torch's softplus(h) = h); h <= 20 throughout -> smooth; otherwise it crosses inside
// the cell: the polynomial takes its smooth softplus and the cell lists the unit ({W1a, b1',
// -W2 e^-20}, at most kVtNX), the evaluation adding torch's jump -W2 log1p(e^-h) = -W2 e^-20
// e^-(h - 20) (1 + O(2e-9)) on the lanes whose h = fma(u, W1a, b1') -- the decoder's own
// pre-activation -- exceeds 20.  Remainder <= (1/(2 INV))^8 / 8! * max|sigma^(7)| (= 17/16) *
// sum_k |W2_k| |W1a_k|^8: 5.6e-15 for the epoch-67 weights.  A cell with more crossings, a
// crossing unit with |W1a| > 4 INV (h - 20 beyond [0, 1]) or a bound above 1e-13 is invalid;
// its lanes, |u| > kVtR + 1/(2 INV), and inputs whose x_v is not the table's prior (bit-exact
// key) evaluate the 128 units.  The readout MLP (mlp, :291, on every message m_e; SEL = 1) gets
// one such table too, with INV = 32 (its |W1| reaches 4.2: bound 5.3e-15), no prior.
// A table: [0] = the prior x (key), pad to kVtHdr; cells [kVtCells(INV)][8] = a_0 .. a_7, the three
// lowest mantissa bits of a_7 holding the cell's code (0-3 crossing units, 7 invalid: a_7 r^7 <=
// a_7 / 2^35 changes by < 1e-25); then [kVtCells(INV)][kVtNX][3] the crossing units.  A lookup
// reads one 64-byte cell (4 dwordx4), a crossing cell one more line.
// ---------------------------------------------------------------------------------------
constexpr int kVtR = 32;                                  // centres |c_j| <= 32
constexpr int kVtNC = 8;                                  // coefficients a_0 .. a_7 per cell
constexpr int kVtNX = 3;                                  // crossing units per cell
constexpr int kVtHdr = 16;
constexpr int kVtInvG = 16, kVtInvR = 32;                 // cells per unit of u: ggc1, readout
__host__ __device__ constexpr int vt_cells(int inv) { return 2 * inv * kVtR + 1; }
__host__ __device__ constexpr int vt_xoff(int inv) { return kVtHdr + vt_cells(inv) * kVtNC; }
__host__ __device__ constexpr int vt_stride(int inv) { return (vt_xoff(inv) + vt_cells(inv) * kVtNX * 3 + 15) & ~15; }
constexpr int kVtStride = vt_stride(kVtInvG);             // 17 456 doubles per prior table
constexpr int kVtStrideR = vt_stride(kVtInvR);            // 34 864: the readout table
constexpr int kVtMaxPriors = 64;
struct VtPriors {
    double x[kVtMaxPriors];
};
// Where a table build takes its priors and their count from.  VtHostList: the caller's host
// list, passed by value with the launch (gnnd_prepare_weights_priors).  VtDevList: a device-
// resident list and count (gnnd_v24_scan_priors' d_priors / d_status), read by the kernel -- the
// launch then covers kVtMaxPriors block rows and the rows at and past the count exit.
struct VtHostList {
    VtPriors pr;
    int n;
    __device__ __forceinline__ int count() const { return n; }
    __device__ __forceinline__ double prior(int t) const { return pr.x[t]; }
};
struct VtDevList {
    const double* x;          // [kVtMaxPriors]
    const int32_t* status;    // [0] = count (0: build nothing)
    __device__ __forceinline__ int count() const {
        const int n = status[0];
        return n < 0 ? 0 : (n > kVtMaxPriors ? kVtMaxPriors : n);
    }
    __device__ __forceinline__ double prior(int t) const { return x[t]; }
};
// block (j, t): cell j of table t, one unit per thread; w = the plain packed fp64 weights
// (may alias prep).  SEL 0: ggc1 with prior src.prior(t), t < src.count(); SEL 1: the readout
// MLP's table in slot src.count() (prep[kV24PriorHdr + 1] = 1 marks it)
template <int SEL, typename SRC>
__global__ void __launch_bounds__(128) vtab_build_kernel(const double* w, double* prep, SRC src) {
    constexpr int INV = SEL == 0 ? kVtInvG : kVtInvR;
    const int n = src.count();
    // (uniform; a host list launches exactly n rows, n > 0)
    if (n == 0 || (SEL == 0 && (int)blockIdx.y >= n)) return;
    const int t0 = SEL == 0 ? 0 : n;
    const double* wm = w + (SEL == 0 ? kV24Ggc1 : kV24Mlp);
    const int k = threadIdx.x, j = blockIdx.x;
    const double x = SEL == 0 ? src.prior(blockIdx.y) : 0.0;
    const double W1a = wm[k], W1b = SEL == 0 ? wm[128 + k] : 0.0, b1 = wm[(SEL == 0 ? 256 : 128) + k];
    const double W2 = wm[(SEL == 0 ? 384 : 256) + k], b2 = wm[SEL == 0 ? 512 : 384];
    // the decoder's pre-activation: ggc1 fma(u, W1a, fma(x, W1b, b1)), readout fma(m, W1, b1)
    const double bp = SEL == 0 ? fma(x, W1b, b1) : b1;
    const double c = (double)(j - INV * kVtR) * (1.0 / INV);
    const double h = fma(W1a, c, bp);
    const double half = fabs(W1a) * (0.5 / INV) + 1e-9 * (1.0 + fabs(h));
    const bool lin = h - half > 20.0, cross = !lin && h + half > 20.0;
    double d[kCtabNC];
    if (lin) {
        d[0] = h;
        d[1] = 1.0;
#pragma unroll
        for (int i = 2; i < kCtabNC; ++i) d[i] = 0.0;
    } else {
        softplus_taylor(h, d);
    }
    __shared__ double part[kVtNC + 1];
    __shared__ int ncross0, ncross1, bad;
    double a[kVtNC];
    double p = W2;
#pragma unroll
    for (int i = 0; i < kVtNC; ++i) {
        a[i] = group_sum_c<64>(p * d[i]);
        p *= W1a;
    }
    const double w2 = W1a * W1a, w4 = w2 * w2;
    const double s8 = group_sum_c<64>(fabs(W2) * (w4 * w4));
    const uint64_t cm = __builtin_amdgcn_ballot_w64(cross);
    const bool wide_cross = __builtin_amdgcn_ballot_w64(cross && fabs(W1a) > 4.0 * INV) != 0;
    if (k == 0) bad = 0;
    __syncthreads();
    if (k == 64) {                                        // wave 1's sums and crossing count
#pragma unroll
        for (int i = 0; i < kVtNC; ++i) part[i] = a[i];
        part[kVtNC] = s8;
        ncross1 = __builtin_popcountll(cm);
    }
    if (k == 0) ncross0 = __builtin_popcountll(cm);
    if ((k & 63) == 0 && wide_cross) bad = 1;
    __syncthreads();

    double* tbl = prep + kV24PriorOff + (size_t)(t0 + blockIdx.y) * kVtStride;
    double* cell = tbl + kVtHdr + (size_t)j * kVtNC;
    double* xu = tbl + vt_xoff(INV) + (size_t)j * kVtNX * 3;    // the cell's crossing units
    // the crossing units in unit order: rank = crossings below k
    const int below = __builtin_popcountll(cm & ((1ull << (k & 63)) - 1ull)) + (k >= 64 ? ncross0 : 0);
    if (cross && below < kVtNX) {
        xu[3 * below] = W1a;
        xu[3 * below + 1] = bp;
        xu[3 * below + 2] = -W2 * exp(-20.0);
    }
    // (1/(2 INV))^8 / 8! * 17/16
    constexpr double kBound = 1.0625 / 40320.0 / ((2.0 * INV) * (2.0 * INV) * (2.0 * INV) * (2.0 * INV) *
                                                  (2.0 * INV) * (2.0 * INV) * (2.0 * INV) * (2.0 * INV));
    if (k == 0) {                                         // wave 0 + wave 1 (fixed order)
        const int ntot = ncross0 + ncross1;
        bool ok = !bad && ntot <= kVtNX && (s8 + part[kVtNC]) * kBound <= 1e-13;
        for (int i = ntot < kVtNX ? ntot : kVtNX; i < kVtNX; ++i) {
            xu[3 * i] = 0.0;
            xu[3 * i + 1] = 0.0;
            xu[3 * i + 2] = 0.0;
        }
        double v[kVtNC];
#pragma unroll
        for (int i = 0; i < kVtNC; ++i) v[i] = (a[i] + part[i]) + (i == 0 ? b2 : 0.0);
        if constexpr (SEL == 0) {
            // the decoder needs t = tanh(f/2) of ggc1's output (the check step's pre-op,
            // quantum/decoder_v2_4.py:135-136): the cell holds t's own degree-7 Taylor series,
            // composed here -- w = (f - f(c))/2 has no constant term, so tanh(w) = w - w^3/3 +
            // 2w^5/15 - 17w^7/315 is exact to r^8, and T = (t0 + tanh w)/(1 + t0 tanh w) by series
            // division (constant term 1).  No composed remainder bound is derived: the cell is
            // valid only if T's polynomial meets tanh(P_f/2) of f's own polynomial P_f at both
            // cell edges (where the r^8 terms peak) within 2e-14; P_f is within f's bound above
            // (<= 1e-13) of f, and tanh halves that, so T stays within 7e-14 of tanh(f/2).
            double wv[kVtNC], w2v[kVtNC], w3v[kVtNC], w5v[kVtNC], w7v[kVtNC], tb[kVtNC], q[kVtNC];
            auto smul = [](const double* A, const double* B, double* C) {
                for (int n2 = 0; n2 < kVtNC; ++n2) {
                    double acc = 0.0;
                    for (int i = 0; i <= n2; ++i) acc = fma(A[i], B[n2 - i], acc);
                    C[n2] = acc;
                }
            };
            wv[0] = 0.0;
            for (int i = 1; i < kVtNC; ++i) wv[i] = 0.5 * v[i];
            smul(wv, wv, w2v);
            smul(w2v, wv, w3v);
            smul(w3v, w2v, w5v);
            smul(w5v, w2v, w7v);
            for (int i = 0; i < kVtNC; ++i)
                tb[i] = ((wv[i] - w3v[i] * (1.0 / 3.0)) + w5v[i] * (2.0 / 15.0)) - w7v[i] * (17.0 / 315.0);
            const double t0 = tanh(0.5 * v[0]);
            for (int n2 = 0; n2 < kVtNC; ++n2) {          // q = (t0 + tb) / (1 + t0 tb)
                double acc = (n2 == 0 ? t0 : 0.0) + tb[n2];
                for (int i = 1; i <= n2; ++i) acc = fma(-t0 * tb[i], q[n2 - i], acc);
                q[n2] = acc;
            }
#pragma unroll
            for (int e2 = 0; e2 < 2; ++e2) {
                const double r = (e2 ? 0.5 : -0.5) / INV;
                double pv = q[kVtNC - 1], pf = v[kVtNC - 1];
                for (int n2 = kVtNC - 2; n2 >= 0; --n2) {
                    pv = fma(pv, r, q[n2]);
                    pf = fma(pf, r, v[n2]);
                }
                ok = ok && fabs(pv - tanh(0.5 * pf)) <= 2e-14;
            }
            for (int i = 0; i < kVtNC; ++i) v[i] = q[i];
        }
        const long long code = ok ? ntot : 7;
        v[kVtNC - 1] = __longlong_as_double((__double_as_longlong(v[kVtNC - 1]) & ~7ll) | code);
#pragma unroll
        for (int i = 0; i < kVtNC; ++i) cell[i] = v[i];
        if (j == 0) {
            tbl[0] = x;
            for (int i = 1; i < kVtHdr; ++i) tbl[i] = 0.0;
            for (int i = vt_xoff(INV) + vt_cells(INV) * kVtNX * 3; i < vt_stride(INV); ++i) tbl[i] = 0.0;
            if (blockIdx.y == 0) prep[kV24PriorHdr + SEL] = SEL == 0 ? (double)n : 1.0;
        }
    }
}
// e^-t, 0 <= t <= 1 (degree 10: relative error < 3e-8, on a term below 2.1e-9 |W2|)
__device__ __forceinline__ double vtab_expm(double t) {
    double p = 1.0 / 3628800;
    p = fma(p, -t, 1.0 / 362880);
    p = fma(p, -t, 1.0 / 40320);
    p = fma(p, -t, 1.0 / 5040);
    p = fma(p, -t, 1.0 / 720);
    p = fma(p, -t, 1.0 / 120);
    p = fma(p, -t, 1.0 / 24);
    p = fma(p, -t, 1.0 / 6);
    p = fma(p, -t, 0.5);
    p = fma(p, -t, 1.0);
    return fma(p, -t, 1.0);
}
struct VtCell {
    double a[kVtNC];
    double key;
    int k;
};
// phase 1: the cell's loads (and the key's) from the clamped index -- straight-line, so the
// fetches of several evaluations issue back to back
template <int INV, bool KEY>
__device__ __forceinline__ VtCell vtab_fetch(const double* __restrict__ tb, double u) {
    VtCell c;
    int k = round_magic_lo(__builtin_fma(u, (double)INV, kRoundMagic));
    c.k = k < -INV * kVtR ? -INV * kVtR : (k > INV * kVtR ? INV * kVtR : k);
    const double2* e = (const double2*)(tb + kVtHdr + (size_t)(c.k + INV * kVtR) * kVtNC);
#pragma unroll
    for (int i = 0; i < kVtNC / 2; ++i) {
        const double2 v = e[i];
        c.a[2 * i] = v.x;
        c.a[2 * i + 1] = v.y;
    }
    c.key = KEY ? tb[0] : 0.0;
    return c;
}
// phase 2: the tests and the polynomial (the rare threshold-crossing units of the cell last)
template <int INV, bool KEY>
__device__ __forceinline__ bool vtab_finish(const double* __restrict__ tb, const VtCell& c, double u, double x,
                                            double& y) {
    const bool key_ok = !KEY || __double_as_longlong(x) == __double_as_longlong(c.key);
    const int code = (int)(__double_as_longlong(c.a[kVtNC - 1]) & 7);
    const bool hit = key_ok && fabs(u) <= kVtR + 0.5 / INV && code <= kVtNX;
    const double r = __builtin_fma((double)c.k, -1.0 / INV, u);
    double p = c.a[kVtNC - 1];
#pragma unroll
    for (int n = kVtNC - 2; n >= 0; --n) p = fma(p, r, c.a[n]);
    if (hit && code > 0) {                                // (a few % of the cells)
        const double* xu = tb + vt_xoff(INV) + (size_t)(c.k + INV * kVtR) * kVtNX * 3;
        double dj = 0.0;
        for (int i = 0; i < code; ++i) {
            const double h = fma(u, xu[3 * i], xu[3 * i + 1]);
            if (h > 20.0) dj = fma(xu[3 * i + 2], vtab_expm(h - 20.0), dj);
        }
        // the jumps dj (|dj| <= 2.1e-9 |W2| per unit) on f, or on t = tanh(f/2) to first order:
        // t + dj (1 - t^2)/2, the next term below dj^2 / 10 ~ 1e-18
        p = KEY ? fma(0.5 * dj, fma(-p, p, 1.0), p) : p + dj;
    }
    if (hit) y = p;
    return hit;
}
// tanh(ggc1.mlp(u, x)/2) (INV = kVtInvG, KEY: the prior tables hold the check step's pre-op
// directly) or mlp(u) (kVtInvR, no key) from table tb (global memory, L2-resident): false (y untouched) when x is not the table's prior, |u| is outside the table or
// the cell is invalid.  The cell index is clamped into the table before any test (NaN and huge
// |u| included), so the key, the cell's four 16-byte loads and the range test issue together --
// one L2 round trip per evaluation, not the key's and then the cell's -- and the tests select
// the result instead of branching around the loads.
template <int INV, bool KEY>
__device__ __forceinline__ bool vtab_eval(const double* __restrict__ tb, double u, double x, double& y) {
    const VtCell c = vtab_fetch<INV, KEY>(tb, u);
    return vtab_finish<INV, KEY>(tb, c, u, x, y);
}

// fp32 forms: TWO EDGES per call, riding the two halves of packed FMAs (the lane's
// slots are processed in pairs).  Prepared layout (gnnd_prepare_weights; base-2 rescaled:
// W1', b1' = W1, b1 x log2(e); w2' = W2 x ln(2)):
//   1-input (ggc2.mlp, mlp): [0,256) {W1'_k, b1'_k} per unit k | [256,384) w2' | [384] b2
//   2-input (ggc1.mlp):      [0,256) {W1b'_k, b1'_k}           | [256,384) W1a' |
//                            [384,512) w2' | [512] b2
// A unit's {W1'_k, b1'_k} is ONE scalar register pair feeding both the multiplier and the
// addend of one v_pk_fma_f32 through op_sel (the constant bus allows one SGPR pair per
// instruction), so layer 1 is one packed FMA per unit for two edges, with no bias moves.
// Softplus is split as  sp(h) = h/2 + |h|/2 + ln(1 + e^-|h|)  (exact identity; for h > 20
// it equals h to within 2e-9 relative, the reference's threshold branch).  The h/2 terms
// are linear in the inputs: sum_k W2_k h_k / 2 collapses to one FMA per edge (V24Lin,
// computed once per workgroup).  Per unit and edge pair:
//   v_pk_fma (layer 1) | 2 v_exp_f32(-|hs|) | v_pk_add 1 | 2 v_log_f32 |
//   2 v_fma_f32(|hs|, 0.5, l) | v_pk_fma (layer 2)
// The exp argument is <= 0 (no overflow, no clamp) and -|.| / |.| are free source
// modifiers.  tools/micro: v_exp/v_log issue at ~2x a plain VALU op; this form has 5
// plain ops per 4 transcendentals (the max(hs, log2(1 + 2^min(hs, 28))) form had 9).
struct V24Lin {
    float a0, a1, b;     // lin(u0, u1) = a0 u0 + a1 u1 + b  (a1 = 0 for 1-input MLPs)
};
__device__ __forceinline__ f32x2 softplus_tail2(f32x2 hs) {   // |hs|/2 + log2(1 + 2^-|hs|)
    f32x2 e;
    e.x = __builtin_amdgcn_exp2f(-fabsf(hs.x));
    e.y = __builtin_amdgcn_exp2f(-fabsf(hs.y));
    e = e + f32x2{1.0f, 1.0f};
    // |hs| as a source modifier of one v_fma_f32 per value (hipcc otherwise materialises
    // |hs| with v_and and packs the FMA: one extra VALU op per pair).  The two v_log_f32 and the
    // two FMAs in ONE asm block, interleaved, so each FMA reads its log result with one
    // instruction in between: the compiler's TRANS -> VALU-use wait state does not cover an
    // inline-asm consumer, and an FMA placed right after its v_log reads a stale value
    // (tools/trans_hazard_check.py)
    float tx, ty;
    asm("v_log_f32 %0, %2\n\t"
        "v_log_f32 %1, %3\n\t"
        "v_fma_f32 %0, |%4|, 0.5, %0\n\t"
        "v_fma_f32 %1, |%5|, 0.5, %1"
        : "=&v"(tx), "=&v"(ty) : "v"(e.x), "v"(e.y), "v"(hs.x), "v"(hs.y));
    return f32x2{tx, ty};
}
// {u0 wb.x + wb.y, u1 wb.x + wb.y}: one SGPR pair as multiplier (lo) and addend (hi)
__device__ __forceinline__ f32x2 pk_fma_sb(f32x2 u, f32x2 wb) {
    f32x2 h;
    asm("v_pk_fma_f32 %0, %1, %2, %2 op_sel:[0,0,1] op_sel_hi:[1,0,1]" : "=v"(h) : "v"(u), "s"(wb));
    return h;
}
// {u0 w.x + c0, u1 w.x + c1} and {u0 w.y + c0, u1 w.y + c1}: scalar weight broadcast
__device__ __forceinline__ f32x2 pk_fma_lo(f32x2 u, f32x2 w, f32x2 c) {
    f32x2 h;
    asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel_hi:[1,0,1]" : "=v"(h) : "v"(u), "s"(w), "v"(c));
    return h;
}
__device__ __forceinline__ f32x2 pk_fma_hi(f32x2 u, f32x2 w, f32x2 c) {
    f32x2 h;
    asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[0,1,0] op_sel_hi:[1,1,1]" : "=v"(h) : "v"(u), "s"(w), "v"(c));
    return h;
}
// TWO EDGES per call (the paired check step of the resident kernel): the edges ride the
// two halves of every packed FMA, one hidden unit per instruction.  Layer 1 + ReLU is one
// clamped v_pk_fma_f32 per unit whose multiplier and addend are the two halves of ONE
// SGPR pair {W1'_k, b1'_k} (op_sel; the constant bus takes one SGPR pair per instruction),
// layer 2 one v_pk_fma_f32 per unit with the weight broadcast from an SGPR pair half; the
// first unit's pair is {w2'_0, b2} (bias as its addend).  Units accumulate in order
// 0..9 from b2 (no accumulator halves to combine): 20 packed ops per edge PAIR.  Same
// power-of-two scaling as Mlp10F32 (bit-identical unit contributions).
// GNND_MLP_ONEASM 1 (default): Mlp10Pair as one asm block per call (same-box A/B r05b: 0.4718 ->
// 0.4640 ms, profiles/r05/experiments/ab_r05b.txt); 0: one asm statement per packed FMA
#ifndef GNND_MLP_ONEASM
#define GNND_MLP_ONEASM 1
#endif
// GNND_MLP_SPECIALIZE 1 (default): the resident kernel's iteration loop is instantiated per
// live-unit count (10, 9, 8) of the message MLP and selected once per kernel; 0 (compile time
// only: same-box A/B, bisecting): only the 10-unit loop is built
#ifndef GNND_MLP_SPECIALIZE
#define GNND_MLP_SPECIALIZE 1
#endif
struct Mlp10Pair {
    f32x2 w1b[10];     // {W1_k 2^-s_k, b1_k 2^-s_k}
    f32x2 w20b;        // {W2_0 2^s_0, b2}
    f32x2 w2[5];       // {W2_{2i} 2^s, W2_{2i+1} 2^s}  (w2[0].x unused)
    // MLP of the affine input u = in_scale v + in_bias with the output scaled by out_scale,
    // folded into the weights:  W1' = W1 in_scale, b1' = W1 in_bias + b1 (one fp32 fma),
    // W2' = W2 out_scale, b2' = b2 out_scale; vmax bounds |v| for the clamp scaling.
    // Live units: a unit whose pre-activation is <= 0 at both ends of the input range
    // [0, vmax] (fp32, the folded W1', b1' the kernel evaluates; the fma is monotone in v, so
    // it is <= 0 in between) adds exactly +0 to every output: dropping it changes no bit.
    // BCH(63,45)'s trained message MLP has one such unit.  load() puts the live units into the
    // first slots in their original order and counts them (nlive, wave-uniform); eval_n<NU> runs
    // the first NU slots.  The caller picks NU ONCE, above its iteration loop (the resident
    // kernel's switch on nlive): a branch on nlive inside every call cost more than the unit
    // saved (BCH -0.3 %, LDPC -5 %, profiles/r05/experiments/ab_r05d.txt).
    int nlive;
    __device__ __forceinline__ void load(const float* w, float vmax, float in_scale = 1.f,
                                         float in_bias = 0.f, float out_scale = 1.f) {
        // live mask (bit k: unit k).  A unit's folded weights do not depend on its slot.
        uint32_t lm = 0;
#pragma unroll
        for (int k = 0; k < 10; ++k) {
            const float w1 = w[k] * in_scale, b1 = __builtin_fmaf(w[k], in_bias, w[10 + k]);
            const bool live = !(b1 <= 0.f && __builtin_fmaf(vmax, w1, b1) <= 0.f);
            lm |= (live ? 1u : 0u) << k;
        }
        uint32_t rem = (uint32_t)__builtin_amdgcn_readfirstlane((int)lm);
        nlive = __builtin_popcount(rem);
        // slot j <- unit k, or zero weights (clamp(0) * 0: exact +0 when evaluated)
        auto fold = [&](int j, int k, bool has) {
            const float w1 = w[k] * in_scale, b1 = __builtin_fmaf(w[k], in_bias, w[10 + k]);
            int e;
            frexpf(fabsf(w1) * vmax + fabsf(b1), &e);
            const float c2 = has ? uniform(ldexpf(w[20 + k] * out_scale, e)) : 0.f;
            w1b[j] = has ? f32x2{uniform(ldexpf(w1, -e)), uniform(ldexpf(b1, -e))} : f32x2{0.f, 0.f};
            if (j & 1) w2[j >> 1].y = c2; else w2[j >> 1].x = c2;
            if (j == 0) w20b = f32x2{c2, uniform(w[30] * out_scale)};
        };
        if (rem == 0x3ffu) {
            // every unit live (the usual case): slot k = unit k, all reads at constant offsets and
            // independent of each other
#pragma unroll
            for (int k = 0; k < 10; ++k) fold(k, k, true);
        } else {
            // slot j takes the j-th live unit (the lowest set bit of what is left of the mask), read
            // at a wave-uniform index: a few scalar ops per slot, and no folded per-unit values
            // held in registers for a select matrix (the kernels sit at their 128-VGPR limit);
            // the slots past nlive get zero weights
#pragma unroll
            for (int j = 0; j < 10; ++j) {
                const bool has = rem != 0;
                const int k = has ? __builtin_ctz(rem) : 0;
                rem &= rem - 1;
                fold(j, k, has);
            }
        }
    }
    // the first NU slots (NU in {10, 9, 8}; exact for nlive <= NU: the slots past nlive hold
    // zero weights)
    template <int NU>
    __device__ __forceinline__ f32x2 eval_n(f32x2 u) const {
        static_assert(NU >= 8 && NU <= 10, "Mlp10Pair::eval_n: 8, 9 or 10 units");
#if GNND_MLP_ONEASM
        // the whole MLP as ONE asm block: hipcc's hazard recognizer assumes an op_sel dst
        // forwarding hazard between consecutive inline-asm VALU blocks and puts an s_nop 0
        // before every one that reads the previous block's result (one per unit); inside a block
        // the packed FMAs are ordinary interlocked VALU dependencies (no trans ops, no DPP, no
        // dst op_sel).  Layer 1 of unit k+1 is issued before unit k's layer-2 FMA (same
        // accumulation order: b2, then units 0..NU-1 — identical bits).
        f32x2 acc, h0, h1;
        if constexpr (NU == 10) {
        asm("v_pk_fma_f32 %1, %3, %4, %4 op_sel:[0,0,1] op_sel_hi:[1,0,1] clamp\n\t"
            "v_pk_fma_f32 %2, %3, %5, %5 op_sel:[0,0,1] op_sel_hi:[1,0,1] clamp\n\t"
            "v_pk_fma_f32 %0, %1, %14, %14 op_sel:[0,0,1] op_sel_hi:[1,0,1]\n\t"
            "v_pk_fma_f32 %1, %3, %6, %6 op_sel:[0,0,1] op_sel_hi:[1,0,1] clamp\n\t"
            "v_pk_fma_f32 %0, %2, %15, %0 op_sel:[0,1,0] op_sel_hi:[1,1,1]\n\t"
            "v_pk_fma_f32 %2, %3, %7, %7 op_sel:[0,0,1] op_sel_hi:[1,0,1] clamp\n\t"
            "v_pk_fma_f32 %0, %1, %16, %0 op_sel_hi:[1,0,1]\n\t"
            "v_pk_fma_f32 %1, %3, %8, %8 op_sel:[0,0,1] op_sel_hi:[1,0,1] clamp\n\t"
            "v_pk_fma_f32 %0, %2, %16, %0 op_sel:[0,1,0] op_sel_hi:[1,1,1]\n\t"
            "v_pk_fma_f32 %2, %3, %9, %9 op_sel:[0,0,1] op_sel_hi:[1,0,1] clamp\n\t"
            "v_pk_fma_f32 %0, %1, %17, %0 op_sel_hi:[1,0,1]\n\t"
            "v_pk_fma_f32 %1, %3, %10, %10 op_sel:[0,0,1] op_sel_hi:[1,0,1] clamp\n\t"
            "v_pk_fma_f32 %0, %2, %17, %0 op_sel:[0,1,0] op_sel_hi:[1,1,1]\n\t"
            "v_pk_fma_f32 %2, %3, %11, %11 op_sel:[0,0,1] op_sel_hi:[1,0,1] clamp\n\t"
            "v_pk_fma_f32 %0, %1, %18, %0 op_sel_hi:[1,0,1]\n\t"
            "v_pk_fma_f32 %1, %3, %12, %12 op_sel:[0,0,1] op_sel_hi:[1,0,1] clamp\n\t"
            "v_pk_fma_f32 %0, %2, %18, %0 op_sel:[0,1,0] op_sel_hi:[1,1,1]\n\t"
            "v_pk_fma_f32 %2, %3, %13, %13 op_sel:[0,0,1] op_sel_hi:[1,0,1] clamp\n\t"
            "v_pk_fma_f32 %0, %1, %19, %0 op_sel_hi:[1,0,1]\n\t"
            "v_pk_fma_f32 %0, %2, %19, %0 op_sel:[0,1,0] op_sel_hi:[1,1,1]"
            : "=&v"(acc), "=&v"(h0), "=&v"(h1)
            : "v"(u), "s"(w1b[0]), "s"(w1b[1]), "s"(w1b[2]), "s"(w1b[3]), "s"(w1b[4]),
              "s"(w1b[5]), "s"(w1b[6]), "s"(w1b[7]), "s"(w1b[8]), "s"(w1b[9]), "s"(w20b),
              "s"(w2[0]), "s"(w2[1]), "s"(w2[2]), "s"(w2[3]), "s"(w2[4]));
        } else if constexpr (NU == 9) {
            // (same operand numbering: %13 = w1b[9] and the high half of %19 stay unread)
            asm("v_pk_fma_f32 %1, %3, %4, %4 op_sel:[0,0,1] op_sel_hi:[1,0,1] clamp\n\t"
                "v_pk_fma_f32 %2, %3, %5, %5 op_sel:[0,0,1] op_sel_hi:[1,0,1] clamp\n\t"
                "v_pk_fma_f32 %0, %1, %14, %14 op_sel:[0,0,1] op_sel_hi:[1,0,1]\n\t"
                "v_pk_fma_f32 %1, %3, %6, %6 op_sel:[0,0,1] op_sel_hi:[1,0,1] clamp\n\t"
                "v_pk_fma_f32 %0, %2, %15, %0 op_sel:[0,1,0] op_sel_hi:[1,1,1]\n\t"
                "v_pk_fma_f32 %2, %3, %7, %7 op_sel:[0,0,1] op_sel_hi:[1,0,1] clamp\n\t"
                "v_pk_fma_f32 %0, %1, %16, %0 op_sel_hi:[1,0,1]\n\t"
                "v_pk_fma_f32 %1, %3, %8, %8 op_sel:[0,0,1] op_sel_hi:[1,0,1] clamp\n\t"
                "v_pk_fma_f32 %0, %2, %16, %0 op_sel:[0,1,0] op_sel_hi:[1,1,1]\n\t"
                "v_pk_fma_f32 %2, %3, %9, %9 op_sel:[0,0,1] op_sel_hi:[1,0,1] clamp\n\t"
                "v_pk_fma_f32 %0, %1, %17, %0 op_sel_hi:[1,0,1]\n\t"
                "v_pk_fma_f32 %1, %3, %10, %10 op_sel:[0,0,1] op_sel_hi:[1,0,1] clamp\n\t"
                "v_pk_fma_f32 %0, %2, %17, %0 op_sel:[0,1,0] op_sel_hi:[1,1,1]\n\t"
                "v_pk_fma_f32 %2, %3, %11, %11 op_sel:[0,0,1] op_sel_hi:[1,0,1] clamp\n\t"
                "v_pk_fma_f32 %0, %1, %18, %0 op_sel_hi:[1,0,1]\n\t"
                "v_pk_fma_f32 %1, %3, %12, %12 op_sel:[0,0,1] op_sel_hi:[1,0,1] clamp\n\t"
                "v_pk_fma_f32 %0, %2, %18, %0 op_sel:[0,1,0] op_sel_hi:[1,1,1]\n\t"
                "v_pk_fma_f32 %0, %1, %19, %0 op_sel_hi:[1,0,1]"
                : "=&v"(acc), "=&v"(h0), "=&v"(h1)
                : "v"(u), "s"(w1b[0]), "s"(w1b[1]), "s"(w1b[2]), "s"(w1b[3]), "s"(w1b[4]),
                  "s"(w1b[5]), "s"(w1b[6]), "s"(w1b[7]), "s"(w1b[8]), "s"(w1b[9]), "s"(w20b),
                  "s"(w2[0]), "s"(w2[1]), "s"(w2[2]), "s"(w2[3]), "s"(w2[4]));
        } else {
            // (%12, %13 = w1b[8], w1b[9] and %19 = w2[4] stay unread)
            asm("v_pk_fma_f32 %1, %3, %4, %4 op_sel:[0,0,1] op_sel_hi:[1,0,1] clamp\n\t"
                "v_pk_fma_f32 %2, %3, %5, %5 op_sel:[0,0,1] op_sel_hi:[1,0,1] clamp\n\t"
                "v_pk_fma_f32 %0, %1, %14, %14 op_sel:[0,0,1] op_sel_hi:[1,0,1]\n\t"
                "v_pk_fma_f32 %1, %3, %6, %6 op_sel:[0,0,1] op_sel_hi:[1,0,1] clamp\n\t"
                "v_pk_fma_f32 %0, %2, %15, %0 op_sel:[0,1,0] op_sel_hi:[1,1,1]\n\t"
                "v_pk_fma_f32 %2, %3, %7, %7 op_sel:[0,0,1] op_sel_hi:[1,0,1] clamp\n\t"
                "v_pk_fma_f32 %0, %1, %16, %0 op_sel_hi:[1,0,1]\n\t"
                "v_pk_fma_f32 %1, %3, %8, %8 op_sel:[0,0,1] op_sel_hi:[1,0,1] clamp\n\t"
                "v_pk_fma_f32 %0, %2, %16, %0 op_sel:[0,1,0] op_sel_hi:[1,1,1]\n\t"
                "v_pk_fma_f32 %2, %3, %9, %9 op_sel:[0,0,1] op_sel_hi:[1,0,1] clamp\n\t"
                "v_pk_fma_f32 %0, %1, %17, %0 op_sel_hi:[1,0,1]\n\t"
                "v_pk_fma_f32 %1, %3, %10, %10 op_sel:[0,0,1] op_sel_hi:[1,0,1] clamp\n\t"
                "v_pk_fma_f32 %0, %2, %17, %0 op_sel:[0,1,0] op_sel_hi:[1,1,1]\n\t"
                "v_pk_fma_f32 %2, %3, %11, %11 op_sel:[0,0,1] op_sel_hi:[1,0,1] clamp\n\t"
                "v_pk_fma_f32 %0, %1, %18, %0 op_sel_hi:[1,0,1]\n\t"
                "v_pk_fma_f32 %0, %2, %18, %0 op_sel:[0,1,0] op_sel_hi:[1,1,1]"
                : "=&v"(acc), "=&v"(h0), "=&v"(h1)
                : "v"(u), "s"(w1b[0]), "s"(w1b[1]), "s"(w1b[2]), "s"(w1b[3]), "s"(w1b[4]),
                  "s"(w1b[5]), "s"(w1b[6]), "s"(w1b[7]), "s"(w1b[8]), "s"(w1b[9]), "s"(w20b),
                  "s"(w2[0]), "s"(w2[1]), "s"(w2[2]), "s"(w2[3]), "s"(w2[4]));
        }
        return acc;
#else
        f32x2 h, acc;
        asm("v_pk_fma_f32 %0, %1, %2, %2 op_sel:[0,0,1] op_sel_hi:[1,0,1] clamp"
            : "=v"(h) : "v"(u), "s"(w1b[0]));
        acc = pk_fma_sb(h, w20b);
#pragma unroll
        for (int k = 1; k < NU; ++k) {
            asm("v_pk_fma_f32 %0, %1, %2, %2 op_sel:[0,0,1] op_sel_hi:[1,0,1] clamp"
                : "=v"(h) : "v"(u), "s"(w1b[k]));
            acc = (k & 1) ? pk_fma_hi(h, w2[k >> 1], acc) : pk_fma_lo(h, w2[k >> 1], acc);
        }
        return acc;
#endif
    }
    __device__ __forceinline__ f32x2 operator()(f32x2 u) const { return eval_n<10>(u); }
    // N edge pairs at once, unit-major: the N accumulation chains interleave, so no packed
    // FMA waits on the one just issued (same per-pair operation order: identical bits)
    template <int N>
    __device__ __forceinline__ void batch(const f32x2 (&u)[N], f32x2 (&acc)[N]) const {
        f32x2 h[N];
#pragma unroll
        for (int i = 0; i < N; ++i)
            asm("v_pk_fma_f32 %0, %1, %2, %2 op_sel:[0,0,1] op_sel_hi:[1,0,1] clamp"
                : "=v"(h[i]) : "v"(u[i]), "s"(w1b[0]));
#pragma unroll
        for (int i = 0; i < N; ++i) acc[i] = pk_fma_sb(h[i], w20b);
#pragma unroll
        for (int k = 1; k < 10; ++k) {
#pragma unroll
            for (int i = 0; i < N; ++i)
                asm("v_pk_fma_f32 %0, %1, %2, %2 op_sel:[0,0,1] op_sel_hi:[1,0,1] clamp"
                    : "=v"(h[i]) : "v"(u[i]), "s"(w1b[k]));
#pragma unroll
            for (int i = 0; i < N; ++i)
                acc[i] = (k & 1) ? pk_fma_hi(h[i], w2[k >> 1], acc[i]) : pk_fma_lo(h[i], w2[k >> 1], acc[i]);
        }
    }
};

// ---------------------------------------------------------------------------------------
// CGNNI / QGNNI message MLP as an exact piecewise-linear table (fp32 resident kernel,
// GNND_MLP_PWL).  The MLP (Linear(1,10) -> ReLU -> Linear(10,1),
// classical/CGNNI.py:238-242, quantum/QGNNI.py:207-214) of one scalar u,
//   f(u) = b2 + sum_k W2_k relu(W1_k u + b1_k),
// is linear between its <= 10 knots kappa_k = -b1_k / W1_k.  gnnd_prepare_weights (fp32)
// appends it as a table (pwl_build_kernel): the knots inside [-31, 31] (|u| <= dc - 1 <= 31)
// span [lo, hi], cut into the fewest K <= 32 equal cells holding at most two knots each (the
// trained weights: BCH 12 cells, LDPC 28, toric QGNNI 12); a cell stores its linear part and
// its knots' relu terms {alpha, beta, gamma1, kappa1, gamma2, kappa2} (the end cells extend to
// -inf / +inf).  The decoder maps each entry to its own input v = R_c - r_e (u = A v + B,
// A = -2, B = G R - 1, the output x log2 e: Mlp10Pair's folding) when it stages the table in
// LDS, so an edge costs an index (fma, cvt, med3, address), one 24-byte LDS entry and 5 FMAs
// (two clamped: relu of a 2^-p scaled difference, 2^p >= G R) instead of 20 packed FMAs per
// edge pair; the same function, rounded differently (the 1e-7 level).  No K <= 32: ok = 0 and
// the kernel keeps Mlp10Pair.
// ---------------------------------------------------------------------------------------
// MEASURED AND NOT KEPT (default 0; -DGNND_MLP_PWL=1 builds it): the table costs two LDS
// reads per edge (24 bytes), and the register-resident kernel's LDS pipe, shared by the CU's
// four SIMDs, is the tighter resource: same-box A/B (profiles/r06/experiments/ab_r06g_pwl.txt)
// BCH 142.5 -> 121.8 M cw/s with the unit fallback compiled in, 124.2 M without it; LDPC 22.0
// -> 16.7 / 17.4 M.  The ten packed unit FMAs with their weights in SGPRs stay.
#ifndef GNND_MLP_PWL
#define GNND_MLP_PWL 0                // 1: the piecewise-linear table (A/B builds)
#endif
constexpr int kPwlMaxCells = 32;
constexpr int kPwlEntry = 8;                                      // floats per cell (6 used)
constexpr size_t kPwlBytes = (size_t)kPwlMaxCells * kPwlEntry * 4;
constexpr int kPwlOff = 64;          // floats: prepared fp32 CGNNI / QGNNI = [62 | pad | hdr | cells]
constexpr int kPwlHdr = 8;           // {ok, K, s, t0, 0...}: cell = clamp(int(u s + t0), 0, K - 1)
constexpr int kGnnPreparedF32 = kPwlOff + kPwlHdr + kPwlMaxCells * kPwlEntry;   // 328
constexpr float kPwlUmax = 31.f;
// w = the plain 62 weights (message MLP at kMlp10Msg), prep = the prepared buffer; one wave.
// The cells' span [lo, hi] runs between two of the knots (the outermost ones may be left to
// the end cells, which extend to -inf / +inf and hold at most two knots like the others): the
// wave tries lo = the 1st..3rd smallest and hi = the 1st..3rd largest knot with K = 1..32 cells
// and keeps the fewest cells (then the first such pair)
__global__ void __launch_bounds__(64) pwl_build_kernel(const float* __restrict__ w, float* __restrict__ prep) {
    const float* m = w + kMlp10Msg;
    float* hdr = prep + kPwlOff;
    float* tab = hdr + kPwlHdr;
    const int tid = threadIdx.x;
    double a[10], c[10], kap[10], ks[10];
    bool in[10];
    int n = 0;
    for (int k = 0; k < 10; ++k) {
        a[k] = (double)m[k];
        c[k] = (double)m[10 + k];
        kap[k] = a[k] != 0.0 ? -c[k] / a[k] : 0.0;
        in[k] = a[k] != 0.0 && fabs(kap[k]) < kPwlUmax;
        if (in[k]) {                                           // insertion into the sorted knots
            int i = n++;
            while (i > 0 && ks[i - 1] > kap[k]) { ks[i] = ks[i - 1]; --i; }
            ks[i] = kap[k];
        }
    }
    auto cell = [&](double x, double lo, double span, int K) {
        const double r = span > 0.0 ? (x - lo) / span * K : 0.0;
        return r < 0.0 ? 0 : (r >= K ? K - 1 : (int)r);
    };
    // combo = (i, j, K): lo = ks[i], hi = ks[n - 1 - j]
    int best = 1 << 30;
    for (int cb = tid; cb < 9 * kPwlMaxCells; cb += 64) {
        const int K = cb / 9 + 1, i = cb % 9 / 3, j = cb % 3;
        if (n == 0 || i > n - 1 - j) continue;
        const double lo = ks[i], span = ks[n - 1 - j] - lo;
        bool fit = true;
        for (int x = 0; x < n && fit; ++x) {
            int cnt = 0;
            const int cx = cell(ks[x], lo, span, K);
            for (int y = 0; y < n; ++y) cnt += cell(ks[y], lo, span, K) == cx;
            fit = cnt <= 2;
        }
        if (fit && cb < best) best = cb;
    }
    for (int o = 1; o < 64; o <<= 1) best = min(best, __shfl_xor(best, o));
    if (n == 0) best = 0;                                      // no knot: one linear cell
    const bool ok = best < (1 << 30);
    const int K = ok ? best / 9 + 1 : 1;
    const double lo = ok && n ? ks[best % 9 / 3] : 0.0;
    const double span = ok && n ? ks[n - 1 - best % 3] - lo : 0.0;
    if (tid == 0) {
        hdr[0] = ok ? 1.f : 0.f;
        hdr[1] = (float)K;
        hdr[2] = span > 0.0 ? (float)(K / span) : 0.f;
        hdr[3] = span > 0.0 ? (float)(-lo * (K / span)) : 0.f;
        for (int i = 4; i < kPwlHdr; ++i) hdr[i] = 0.f;
        prep[62] = prep[63] = 0.f;
    }
    if (ok && tid < kPwlMaxCells) {
        double al = (double)m[30], be = 0.0, ga[2] = {0.0, 0.0}, ka[2] = {0.0, 0.0};
        int nk = 0;
        for (int k = 0; k < 10; ++k) {
            const int ci = in[k] ? cell(kap[k], lo, span, K) : -1;
            const double w2 = (double)m[20 + k];
            bool lin;                                          // active as a linear term
            if (ci == tid && nk < 2) {                         // the knot's relu term here
                ga[nk] = w2 * fabs(a[k]);
                ka[nk] = kap[k];
                ++nk;
                lin = a[k] < 0.0;                              // relu(-x) = -x + relu(x)
            } else if (ci >= 0) {
                lin = (a[k] > 0.0) == (ci < tid);
            } else {
                lin = a[k] != 0.0 ? (a[k] > 0.0) == (kap[k] < 0.0) : c[k] > 0.0;   // sign at u = 0
            }
            if (lin) { al = fma(w2, c[k], al); be = fma(w2, a[k], be); }
        }
        float* e = tab + tid * kPwlEntry;
        e[0] = (float)al; e[1] = (float)be;
        e[2] = (float)ga[0]; e[3] = (float)ka[0];
        e[4] = (float)ga[1]; e[5] = (float)ka[1];
        e[6] = 0.f; e[7] = 0.f;
    }
}
struct Pwl {
    int ok, K;
    float s, t0, sc;     // v-domain cell = clamp(int(v s + t0), 0, K - 1); sc = 2^-p
};
// the decoder's v-domain copy of the prepared table (u = A v + B, output x O), entries by
// threads < K; the caller's barrier orders them before use
__device__ Pwl pwl_stage(const float* __restrict__ prep, float* __restrict__ tab, float vmax, float A,
                         float B, float O, int tid) {
    const float* hdr = prep + kPwlOff;
    Pwl p;
    p.ok = (int)hdr[0];
    p.K = (int)hdr[1];
    int e2 = 0;
    frexpf(vmax, &e2);                                         // 2^e2 > vmax
    p.sc = ldexpf(1.f, -e2);
    const double s = hdr[2], t0 = hdr[3];
    p.s = (float)(A * s);                                      // cell from v: (A v + B) s + t0
    p.t0 = (float)fma((double)B, s, t0);
    if (p.ok && tid < p.K) {
        const float* e = hdr + kPwlHdr + tid * kPwlEntry;
        double al = e[0] + (double)e[1] * B, be = (double)e[1] * A;
        double g[2], kv[2];
        for (int j = 0; j < 2; ++j) {
            // gamma relu(u - kappa) = gamma relu(A (v - kv)), kv = (kappa - B) / A
            const double ga = e[2 + 2 * j], kap = e[3 + 2 * j];
            kv[j] = (kap - B) / A;
            g[j] = ga * fabs((double)A);
            if (A < 0.f) { al = fma(g[j], kv[j], al); be -= g[j]; }   // |A| relu(kv - v)
        }
        float* d = tab + tid * kPwlEntry;
        d[0] = (float)(al * O);
        d[1] = (float)(be * O);
        d[2] = (float)(g[0] * O / p.sc);
        d[3] = (float)(-kv[0] * p.sc);
        d[4] = (float)(g[1] * O / p.sc);
        d[5] = (float)(-kv[1] * p.sc);
        d[6] = 0.f; d[7] = 0.f;
    }
    return p;
}
__device__ __forceinline__ float pwl_eval(const float* tab, const Pwl& p, float v) {
    int k = (int)__builtin_fmaf(v, p.s, p.t0);
    k = k < 0 ? 0 : (k >= p.K ? p.K - 1 : k);
    const float* e = tab + k * kPwlEntry;
    const float4 e0 = *(const float4*)e;
    const float2 e1 = *(const float2*)(e + 4);
    float y = __builtin_fmaf(e0.y, v, e0.x);
    y = __builtin_fmaf(e0.z, __builtin_amdgcn_fmed3f(__builtin_fmaf(v, p.sc, e0.w), 0.f, 1.f), y);
    return __builtin_fmaf(e1.x, __builtin_amdgcn_fmed3f(__builtin_fmaf(v, p.sc, e1.y), 0.f, 1.f), y);
}
__device__ __forceinline__ f32x2 pwl_eval2(const float* tab, const Pwl& p, f32x2 v) {
    return f32x2{pwl_eval(tab, p, v.x), pwl_eval(tab, p, v.y)};
}
// the fp32 GNN message MLP's piecewise-linear table into the prepared buffer (w may alias prep)
int launch_pwl_build(const float* w, float* prep, hipStream_t st) {
    pwl_build_kernel<<<1, 64, 0, st>>>(w, prep);
    GNND_LAUNCH_CHECK();
    return GNND_OK;
}

// The unit sum in a FIXED order independent of how the units are spread over lanes: chain j
// (0..7) accumulates units k = 8i + j (i ascending), chain 0 starting from the linear part,
// and the MLP value is ((c0 + c1) + (c2 + c3)) + ((c4 + c5) + (c6 + c7)).  A call evaluates
// NC consecutive chains from J0 and returns their sum in that tree (NC = 8: the whole MLP;
// NC = 4 / 2 / 1: a half / quarter / eighth, the unit-split small-batch kernel combining the
// other waves' parts through LDS), so every split gives the same bits.  TWO: the 2-input MLP
// (u0 -> W1a', u1 -> W1b').  wg: the MLP's prepared weights in global memory (uniform
// address: scalar loads; J0 is a template argument so the weight offsets stay compile-time).
template <int NC, int J0, bool TWO>
__device__ __forceinline__ f32x2 mlp128_chains(const float* __restrict__ wg, V24Lin lin,
                                               f32x2 u0, f32x2 u1) {
    const f32x2* wb = (const f32x2*)wg;                      // {W1b'_k, b1'_k}
    const f32x2* wa = (const f32x2*)(wg + 256);              // W1a' pairs (TWO)
    const f32x2* w2 = (const f32x2*)(wg + (TWO ? 384 : 256));
    f32x2 c[NC];
#pragma unroll
    for (int jj = 0; jj < NC; ++jj) c[jj] = f32x2{0.f, 0.f};
    if constexpr (J0 == 0) {
        if constexpr (TWO)
            c[0] = __builtin_elementwise_fma(u0, f32x2{lin.a0, lin.a0},
                       __builtin_elementwise_fma(u1, f32x2{lin.a1, lin.a1}, f32x2{lin.b, lin.b}));
        else
            c[0] = __builtin_elementwise_fma(u0, f32x2{lin.a0, lin.a0}, f32x2{lin.b, lin.b});
    }
    constexpr int kUnroll = 8 / NC;                          // 8 units per loop trip
#pragma unroll kUnroll
    for (int i = 0; i < 16; ++i) {
        static_for<NC>([&](auto jc) {
            constexpr int j = J0 + decltype(jc)::value;         // chain (unit k = 8i + j)
            const int k = 8 * i + j;
            f32x2 h;
            if constexpr (TWO) {
                const f32x2 a = wa[k >> 1];
                h = (j & 1) ? pk_fma_hi(u0, a, pk_fma_sb(u1, wb[k])) : pk_fma_lo(u0, a, pk_fma_sb(u1, wb[k]));
            } else {
                h = pk_fma_sb(u0, wb[k]);
            }
            f32x2& cj = c[decltype(jc)::value];
            cj = (j & 1) ? pk_fma_hi(softplus_tail2(h), w2[k >> 1], cj)
                         : pk_fma_lo(softplus_tail2(h), w2[k >> 1], cj);
        });
    }
    if constexpr (NC == 8) return ((c[0] + c[1]) + (c[2] + c[3])) + ((c[4] + c[5]) + (c[6] + c[7]));
    else if constexpr (NC == 4) return (c[0] + c[1]) + (c[2] + c[3]);
    else if constexpr (NC == 2) return c[0] + c[1];
    else return c[0];
}
__device__ __forceinline__ f32x2 mlp128_sp2(const float* __restrict__ wg, V24Lin lin,
                                            f32x2 u) {
    return mlp128_chains<8, 0, false>(wg, lin, u, u);
}
__device__ __forceinline__ f32x2 mlp128x2_sp2(const float* __restrict__ wg, V24Lin lin,
                                              f32x2 u0, f32x2 u1) {
    return mlp128_chains<8, 0, true>(wg, lin, u0, u1);
}
// item lanes per workgroup of the unit-split streaming kernel: 256, except US = 8 (128 item
// lanes x 8 waves each = 1024 threads; taken when a codeword's items fit 128 lanes)
template <int US> constexpr int unit_split_lanes() { return US == 8 ? 128 : GNND_BLOCK; }
// unit-split evaluation (decode_kernel US > 1): wave-uniform `sub` selects this wave's
// chains; the US partial sums meet in LDS (buf = [US][IL] f32x2, IL = unit_split_lanes, one of
// two buffers used alternately so one barrier per call suffices) and every wave combines them
// in the tree above.  All threads of the workgroup must call it (barrier).  idle
// (wave-uniform): the wave holds no live work item (its result is never stored) and skips the
// units, so the SIMDs' issue goes to the live item waves only.
template <int US, bool TWO>
__device__ __forceinline__ f32x2 mlp128_split(const float* __restrict__ wg, V24Lin lin,
                                              f32x2 u0, f32x2 u1, int sub, f32x2* buf, int itid,
                                              bool idle, PhaseProf* pf = nullptr, int mk = 0) {
    (void)pf; (void)mk;
    constexpr int IL = unit_split_lanes<US>();
    f32x2 p = {0.f, 0.f};
    if constexpr (US == 1) {
        if (!idle) p = mlp128_chains<8, 0, TWO>(wg, lin, u0, u1);
        return p;
    } else {
        static_assert(US == 2 || US == 4 || US == 8, "unit split 1, 2, 4 or 8");
        constexpr int NC = 8 / US;
        if (!idle) {
            switch (sub) {
                case 0: p = mlp128_chains<NC, 0, TWO>(wg, lin, u0, u1); break;
                case 1: p = mlp128_chains<NC, NC, TWO>(wg, lin, u0, u1); break;
                case 2: if constexpr (US >= 4) p = mlp128_chains<NC, (2 * NC) & 7, TWO>(wg, lin, u0, u1); break;
                case 3: if constexpr (US >= 4) p = mlp128_chains<NC, (3 * NC) & 7, TWO>(wg, lin, u0, u1); break;
                case 4: if constexpr (US == 8) p = mlp128_chains<1, 4, TWO>(wg, lin, u0, u1); break;
                case 5: if constexpr (US == 8) p = mlp128_chains<1, 5, TWO>(wg, lin, u0, u1); break;
                case 6: if constexpr (US == 8) p = mlp128_chains<1, 6, TWO>(wg, lin, u0, u1); break;
                default: if constexpr (US == 8) p = mlp128_chains<1, 7, TWO>(wg, lin, u0, u1); break;
            }
        }
#ifdef GNND_PHASE_PROF
        if (pf) pf->mark(mk);
#endif
        buf[sub * IL + itid] = p;
        __syncthreads();
        f32x2 r;
        if constexpr (US == 2) r = buf[itid] + buf[IL + itid];
        else if constexpr (US == 4)
            r = (buf[itid] + buf[IL + itid]) + (buf[2 * IL + itid] + buf[3 * IL + itid]);
        else
            r = ((buf[itid] + buf[IL + itid]) + (buf[2 * IL + itid] + buf[3 * IL + itid])) +
                ((buf[4 * IL + itid] + buf[5 * IL + itid]) + (buf[6 * IL + itid] + buf[7 * IL + itid]));
#ifdef GNND_PHASE_PROF
        if (pf) pf->mark(mk + 1);
#endif
        return r;
    }
}
// Unit-PAIR form of the fp32 MLPs (decode_kernel on an R = 1 slot plan, the small batches of
// the training steps): ONE edge per lane and the two halves of every packed op carrying two
// hidden units, k = 8i + 2p and k + 1 — chains 2p and 2p + 1 of the fixed order above, each
// half accumulating its chain exactly as mlp128_chains does for one edge (same FMA per edge and
// unit, chain 0 from the linear part), and pair p's value c.x + c.y = c[2p] + c[2p + 1] enters
// the same tree: every form gives the same bits.  With a toric component's 192 edges on 192
// lanes the unit split's item waves are FULL (the edge-pair form puts 96 pairs on 128 lanes).
// Weights: the workgroup's LDS copy in pair-major order (UpairLds, staged from the prepared
// layout): entry e = 16 p + i holds {W'_k, W'_k+1, b'_k, b'_k+1} (2-input: the W1b' weights),
// then [64] {w2'_k, w2'_k+1} and (2-input) [64] {W1a'_k, W1a'_k+1}: broadcast LDS reads, every
// operand of the packed FMAs a VGPR pair (the SGPR pairs of the edge-pair form hold one unit).
struct UpairLds {
    static constexpr int kL1 = 0, kW2 = 256, kWA = 384;          // float offsets in an MLP block
    static constexpr int kMlp0 = 0, kMlp1 = 512, kMlp2 = 896, kFloats = 1280;   // ggc1, ggc2, mlp
};
template <int NP, int P0, bool TWO, bool FAIR = false>
__device__ __forceinline__ float mlp128_upair(const float* wl, V24Lin lin, float u0, float u1) {
    const f32x4* l1 = (const f32x4*)(wl + UpairLds::kL1);
    const f32x2* w2 = (const f32x2*)(wl + UpairLds::kW2);
    const f32x2* wa = (const f32x2*)(wl + UpairLds::kWA);
    const f32x2 U0 = {u0, u0}, U1 = {u1, u1};
    f32x2 c[NP];
#pragma unroll
    for (int q = 0; q < NP; ++q) c[q] = f32x2{0.f, 0.f};
    if constexpr (P0 == 0)
        c[0].x = TWO ? __builtin_fmaf(u0, lin.a0, __builtin_fmaf(u1, lin.a1, lin.b))
                     : __builtin_fmaf(u0, lin.a0, lin.b);
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        if constexpr (FAIR) {
            if (i == 0) __builtin_amdgcn_s_setprio(3);
            if (i == 6) __builtin_amdgcn_s_setprio(2);
            if (i == 11) __builtin_amdgcn_s_setprio(1);
        }
#pragma unroll
        for (int q = 0; q < NP; ++q) {
            const int e = (P0 + q) * 16 + i;
            const f32x4 L = l1[e];
            const f32x2 w = {L.x, L.y}, b = {L.z, L.w};
            f32x2 h;
            if constexpr (TWO) h = __builtin_elementwise_fma(U0, wa[e], __builtin_elementwise_fma(U1, w, b));
            else h = __builtin_elementwise_fma(U0, w, b);
            c[q] = __builtin_elementwise_fma(softplus_tail2(h), w2[e], c[q]);
        }
    }
    if constexpr (FAIR) __builtin_amdgcn_s_setprio(0);
    if constexpr (NP == 4)
        return ((c[0].x + c[0].y) + (c[1].x + c[1].y)) + ((c[2].x + c[2].y) + (c[3].x + c[3].y));
    else if constexpr (NP == 2) return (c[0].x + c[0].y) + (c[1].x + c[1].y);
    else return c[0].x + c[0].y;
}
// unit-split evaluation of the unit-pair form (as mlp128_split: wave `sub` evaluates pairs
// [sub NP, (sub + 1) NP), the partials meet in buf = [US][IL] floats, one of two buffers used
// alternately; every thread must call it; idle waves skip the units)
template <int US, bool TWO>
__device__ __forceinline__ float mlp128_upair_split(const float* wl, V24Lin lin, float u0, float u1,
                                                    int sub, float* buf, int itid, bool idle) {
    constexpr int IL = GNND_BLOCK;
    if constexpr (US == 1) {
        return idle ? 0.f : mlp128_upair<4, 0, TWO>(wl, lin, u0, u1);
    } else {
        static_assert(US == 2 || US == 4, "unit-pair split 1, 2 or 4");
        constexpr int NP = 4 / US;
        float p = 0.f;
        if (!idle) {
            constexpr bool F = GNND_FWD_FAIR;
            switch (sub) {
                case 0: p = mlp128_upair<NP, 0, TWO, F>(wl, lin, u0, u1); break;
                case 1: p = mlp128_upair<NP, NP, TWO, F>(wl, lin, u0, u1); break;
                case 2: if constexpr (US == 4) p = mlp128_upair<1, 2, TWO, F>(wl, lin, u0, u1); break;
                default: if constexpr (US == 4) p = mlp128_upair<1, 3, TWO, F>(wl, lin, u0, u1); break;
            }
        }
        buf[sub * IL + itid] = p;
        __syncthreads();
        if constexpr (US == 2) return buf[itid] + buf[IL + itid];
        else return (buf[itid] + buf[IL + itid]) + (buf[2 * IL + itid] + buf[3 * IL + itid]);
    }
}
// stage the three MLPs' pair-major LDS blocks from the prepared fp32 V24 weights (gnnd_decode.hip
// prepare_v24_f32_kernel layout): one entry per thread (workgroups have >= 256 threads)
__device__ __forceinline__ void stage_upair(const float* __restrict__ w, float* s, int tid) {
    if (tid < 3 * 64) {
        const int idx = tid;
        const int m = idx >> 6, e = idx & 63, k = 8 * (e & 15) + 2 * (e >> 4);
        const float* src = w + (m == 0 ? kV24Ggc1 : m == 1 ? kV24Ggc2 : kV24Mlp);
        float* d = s + (m == 0 ? UpairLds::kMlp0 : m == 1 ? UpairLds::kMlp1 : UpairLds::kMlp2);
        ((f32x4*)(d + UpairLds::kL1))[e] = f32x4{src[2 * k], src[2 * k + 2], src[2 * k + 1], src[2 * k + 3]};
        const int o2 = m == 0 ? 384 : 256;
        ((f32x2*)(d + UpairLds::kW2))[e] = f32x2{src[o2 + k], src[o2 + k + 1]};
        if (m == 0) ((f32x2*)(d + UpairLds::kWA))[e] = f32x2{src[256 + k], src[256 + k + 1]};
    }
}
// linear parts, identical in every thread: a fixed-order 128-term dot product spread over the
// wave's lanes (lane l: units l and l + 64, then the group_sum_c<64> butterfly, whose result
// is the same bits in every lane and wave) — one vector-load latency instead of a serial chain
// of scalar loads and 128 dependent FMAs per thread.  All 64 lanes must call it.
__device__ __forceinline__ float wave_dot128(const float* __restrict__ a, int sa,
                                             const float* __restrict__ b, int sb) {
    const int l = threadIdx.x & 63;
    const float p = __builtin_fmaf(a[(l + 64) * sa], b[(l + 64) * sb], a[l * sa] * b[l * sb]);
    return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(
                                         __builtin_bit_cast(int, group_sum_c<64>(p))));
}
__device__ __forceinline__ V24Lin v24_lin1(const float* __restrict__ wg) {
    const float a = wave_dot128(wg + 256, 1, wg, 2);
    const float b = wave_dot128(wg + 256, 1, wg + 1, 2);
    return V24Lin{0.5f * a, 0.f, __builtin_fmaf(0.5f, b, wg[384])};
}
__device__ __forceinline__ V24Lin v24_lin2(const float* __restrict__ wg) {
    const float a0 = wave_dot128(wg + 384, 1, wg + 256, 1);
    const float a1 = wave_dot128(wg + 384, 1, wg, 2);
    const float b = wave_dot128(wg + 384, 1, wg + 1, 2);
    return V24Lin{0.5f * a0, 0.5f * a1, __builtin_fmaf(0.5f, b, wg[512])};
}
struct V24F32 {            // fp32 V24 weights of the streaming kernel
    const float* __restrict__ g;
    V24Lin l1, l2, l3;     // ggc1.mlp, ggc2.mlp, mlp
};

// ---------------------------------------------------------------------------------------
// the fused kernel
// ---------------------------------------------------------------------------------------
template <typename T> struct alignas(2 * sizeof(T)) SumX {
    T s;   // S_v = sum of the variable's incoming c->v messages
    T x;   // x_v (prior / LLR)
};

// S_v = sum_{k in [k0, ke)} mb[vslot[k]] in k (= reference index_add) order.  The slot
// indices and the messages are fetched eight at a time (independent LDS reads in flight,
// clamped addresses, masked adds) instead of one dependent read pair per edge.
template <typename T>
__device__ __forceinline__ T var_sum(const T* mb, const int* vslot, int k0, int ke, int nslot = 1 << 30) {
    T s = T(0);
    for (int k = k0; k < ke; k += 8) {
        int idx[8];
        T val[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) idx[j] = GNND_DIDX(vslot[min(k + j, ke - 1)], nslot, GNND_DBG_SLOT);
#pragma unroll
        for (int j = 0; j < 8; ++j) val[j] = mb[idx[j]];
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (k + j < ke) s += val[j];
    }
    return s;
}


// S_v = sum_k fl(wk[k] * mb[vslot[k]]) in k order (NBP: the messages are weighted before
// the variable aggregation, neural_BP.py:248)
template <typename T>
__device__ __forceinline__ T var_sum_w(const T* mb, const int* vslot, int k0, int ke,
                                       const T* __restrict__ wk) {
    T s = T(0);
    for (int k = k0; k < ke; ++k) s += mb[vslot[k]] * wk[k];
    return s;
}

// ---------------------------------------------------------------------------------------
// per-edge model math shared by both kernels
// ---------------------------------------------------------------------------------------
// ---------------------------------------------------------------------------------------
// fp32 BP check-node math (classical/BP.py:101-116, quantum/BP.py:103-117) on the native
// v_exp_f32 / v_log_f32 / v_rcp_f32, in the BASE-2 log domain: the check sums carry
// log2|t| instead of ln|t| (exp2 of the base-2 sum is the same exp of the natural sum), so
// no ln2 rescaling sits between the transcendental ops.
//   tanh(z), z = min(|a|, 10)/2:  odd Taylor polynomial to z^9 for z < 0.3 (error < 2e-8
//   relative), (1 - e)/(1 + e) with e = 2^(-2 z log2 e) above (1 - e >= 0.45: ~2 ulp).
// Accuracy is a few ulp of the libm forms; classical BP in fp32 is ill-conditioned near
// its clamps (tests/test_gpu_parity.py conditioning test) for any two fp32
// implementations alike.
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ float bp_log2tanh_f32(float a, float lo) {
    const float z = 0.5f * fminf(fabsf(a), 10.f);
    const float z2 = z * z;
    float tp = __builtin_fmaf(z2, 62.f / 2835.f, -17.f / 315.f);
    tp = __builtin_fmaf(z2, tp, 2.f / 15.f);
    tp = __builtin_fmaf(z2, tp, -1.f / 3.f);
    tp = __builtin_fmaf(z2 * z, tp, z);
    const float e = __builtin_amdgcn_exp2f(z * (-2.f * kLog2e));
    const float te = (1.f - e) * __builtin_amdgcn_rcpf(1.f + e);
    const float t = z < 0.3f ? tp : te;
    return __builtin_amdgcn_logf(fmaxf(t, lo));
}
// m from the base-2 leave-one-out sum lam2 and the sign count n (CBP: log((1+p)/(1-p)),
// QBP: log(1+p) - log(1-p)), p = clamp(2^lam2 cos(pi n), +-hi)
template <bool QUANTUM>
__device__ __forceinline__ float bp_msg_f32(float lam2, float n, float hi) {
    const float p = g_clamp(__builtin_amdgcn_exp2f(lam2) * cos_pi(n), -hi, hi);
    if constexpr (QUANTUM)
        return kLn2 * (__builtin_amdgcn_logf(1.f + p) - __builtin_amdgcn_logf(1.f - p));
    else
        return kLn2 * __builtin_amdgcn_logf((1.f + p) * __builtin_amdgcn_rcpf(1.f - p));
}

// the same two functions on TWO edges (the paired check step of the resident kernel):
// every non-transcendental op is one packed VALU op for both; per half the arithmetic is
// identical to the scalar forms above.  The sign (-1)^n of an integer-valued count n is
// 1 - 2 (n - 2 floor(n / 2)) (torch.cos(pi n) rounds to exactly +-1 there too).
__device__ __forceinline__ f32x2 bp_log2tanh_f32x2(f32x2 a, float lo) {
    const f32x2 z = f32x2{fminf(fabsf(a.x), 10.f), fminf(fabsf(a.y), 10.f)} * 0.5f;
    const f32x2 z2 = z * z;
    f32x2 tp = __builtin_elementwise_fma(z2, f32x2{62.f / 2835.f, 62.f / 2835.f},
                                         f32x2{-17.f / 315.f, -17.f / 315.f});
    tp = __builtin_elementwise_fma(z2, tp, f32x2{2.f / 15.f, 2.f / 15.f});
    tp = __builtin_elementwise_fma(z2, tp, f32x2{-1.f / 3.f, -1.f / 3.f});
    tp = __builtin_elementwise_fma(z2 * z, tp, z);
    const f32x2 ea = z * (-2.f * kLog2e);
    const f32x2 e = {__builtin_amdgcn_exp2f(ea.x), __builtin_amdgcn_exp2f(ea.y)};
    const f32x2 d = f32x2{1.f, 1.f} + e;
    const f32x2 te = (f32x2{1.f, 1.f} - e) * f32x2{__builtin_amdgcn_rcpf(d.x), __builtin_amdgcn_rcpf(d.y)};
    const f32x2 t = {z.x < 0.3f ? tp.x : te.x, z.y < 0.3f ? tp.y : te.y};
    return f32x2{__builtin_amdgcn_logf(fmaxf(t.x, lo)), __builtin_amdgcn_logf(fmaxf(t.y, lo))};
}
template <bool QUANTUM>
__device__ __forceinline__ f32x2 bp_msg_f32x2(f32x2 lam2, f32x2 n, float hi) {
    const f32x2 h = n * 0.5f;
    const f32x2 par = __builtin_elementwise_fma(f32x2{__builtin_floorf(h.x), __builtin_floorf(h.y)},
                                                f32x2{-2.f, -2.f}, n);
    const f32x2 sgn = __builtin_elementwise_fma(par, f32x2{-2.f, -2.f}, f32x2{1.f, 1.f});
    f32x2 p = f32x2{__builtin_amdgcn_exp2f(lam2.x), __builtin_amdgcn_exp2f(lam2.y)} * sgn;
    p = f32x2{__builtin_amdgcn_fmed3f(p.x, -hi, hi), __builtin_amdgcn_fmed3f(p.y, -hi, hi)};
    const f32x2 up = f32x2{1.f, 1.f} + p, dn = f32x2{1.f, 1.f} - p;
    if constexpr (QUANTUM)
        return (f32x2{__builtin_amdgcn_logf(up.x), __builtin_amdgcn_logf(up.y)} -
                f32x2{__builtin_amdgcn_logf(dn.x), __builtin_amdgcn_logf(dn.y)}) * kLn2;
    else {
        const f32x2 q = up * f32x2{__builtin_amdgcn_rcpf(dn.x), __builtin_amdgcn_rcpf(dn.y)};
        return f32x2{__builtin_amdgcn_logf(q.x), __builtin_amdgcn_logf(q.y)} * kLn2;
    }
}

// PRODUCT form of the same check step (the paired resident kernel): exp(S_c(log|t|) -
// log|t_e|) = prod_{e' != e} |t_e'|, so the check node multiplies the clamped magnitudes
// max(|t|, lo) (padding slots: 1) and the leave-one-out value is prod * rcp(|t_e|) — one
// v_rcp_f32 per edge in place of a v_log_f32 and a v_exp_f32, and no log/exp round trip
// (the product of <= dc factors in [lo, 1] keeps ~dc ulp relative error where the log sum
// of magnitudes up to |log2 lo| keeps ~dc ulp of THAT sum, amplified by exp2).  Products
// below the fp32 range flush to 0 exactly where the reference's exp(sum) underflows.
__device__ __forceinline__ f32x2 bp_abstanh_f32x2(f32x2 a, float lo) {
    const f32x2 z = f32x2{fminf(fabsf(a.x), 10.f), fminf(fabsf(a.y), 10.f)} * 0.5f;
    const f32x2 z2 = z * z;
    f32x2 tp = __builtin_elementwise_fma(z2, f32x2{62.f / 2835.f, 62.f / 2835.f},
                                         f32x2{-17.f / 315.f, -17.f / 315.f});
    tp = __builtin_elementwise_fma(z2, tp, f32x2{2.f / 15.f, 2.f / 15.f});
    tp = __builtin_elementwise_fma(z2, tp, f32x2{-1.f / 3.f, -1.f / 3.f});
    tp = __builtin_elementwise_fma(z2 * z, tp, z);
    const f32x2 ea = z * (-2.f * kLog2e);
    const f32x2 e = {__builtin_amdgcn_exp2f(ea.x), __builtin_amdgcn_exp2f(ea.y)};
    const f32x2 d = f32x2{1.f, 1.f} + e;
    const f32x2 te = (f32x2{1.f, 1.f} - e) * f32x2{__builtin_amdgcn_rcpf(d.x), __builtin_amdgcn_rcpf(d.y)};
    const f32x2 t = {z.x < 0.3f ? tp.x : te.x, z.y < 0.3f ? tp.y : te.y};
    return f32x2{fmaxf(t.x, lo), fmaxf(t.y, lo)};
}
// m from the leave-one-out magnitude product q and the sign count n
template <bool QUANTUM>
__device__ __forceinline__ f32x2 bp_msg_prod_f32x2(f32x2 q, f32x2 n, float hi) {
    const f32x2 h = n * 0.5f;
    const f32x2 par = __builtin_elementwise_fma(f32x2{__builtin_floorf(h.x), __builtin_floorf(h.y)},
                                                f32x2{-2.f, -2.f}, n);
    const f32x2 sgn = __builtin_elementwise_fma(par, f32x2{-2.f, -2.f}, f32x2{1.f, 1.f});
    f32x2 p = q * sgn;
    p = f32x2{__builtin_amdgcn_fmed3f(p.x, -hi, hi), __builtin_amdgcn_fmed3f(p.y, -hi, hi)};
    const f32x2 up = f32x2{1.f, 1.f} + p, dn = f32x2{1.f, 1.f} - p;
    if constexpr (QUANTUM)
        return (f32x2{__builtin_amdgcn_logf(up.x), __builtin_amdgcn_logf(up.y)} -
                f32x2{__builtin_amdgcn_logf(dn.x), __builtin_amdgcn_logf(dn.y)}) * kLn2;
    else {
        const f32x2 r = up * f32x2{__builtin_amdgcn_rcpf(dn.x), __builtin_amdgcn_rcpf(dn.y)};
        return f32x2{__builtin_amdgcn_logf(r.x), __builtin_amdgcn_logf(r.y)} * kLn2;
    }
}
// RATIO form of the fp32 BP check step (the paired resident kernel, GNND_BP_RATIO): with the
// state in base-2 units (a' = a log2 e) and t_e = tanh(a_e/2) = n_e / d_e, n_e = sign(a)(1 - E),
// d_e = 1 + E, E = 2^-z, z = clamp(|a'|, zmin, zmax) (the reference's clamp(a, -10, 10) and
// its |t| >= lo floor, both on t's argument), the check node forms N = prod n and D = prod d
// (signed numerators carry the sign count: no (-1)^n parity), and the leave-one-out value is
// p_e = (N / n_e) / (D / d_e), so the message
//     m'_e = log2((1 + p_e) / (1 - p_e)) = log2|D n_e + N d_e| - log2|D n_e - N d_e|
// (CBP log((1+p)/(1-p)), QBP log(1+p) - log(1-p): the same function, in base 2) takes two
// v_log_f32 and no reciprocal: 3 transcendentals per edge (exp, 2 log) instead of the product
// form's 5 (exp and rcp for tanh, the leave-one-out rcp, rcp and log for atanh).  |p_e| <= tanh(5)
// ^(dc - 1) < 1 for every check of degree >= 2, so the reference's p clamp (1 - 1e-7 / 1 - 1e-12)
// never binds and the denominators never vanish (plans with a degree-1 check keep the product
// form: make_plan).  n_e != 0 by the z floor; products of tiny factors may underflow, exactly
// where the true leave-one-out value is below the fp32 range anyway (m'_e -> 0, never NaN).
// zmin = 1e-7 * 2 / ln 2 puts t's floor at the reference's 1e-7 (CBP; QBP's 1e-20 floor is
// below fp32's resolution of 1 - E: its t floor is 1e-7 too, a message change below 3e-7).
// The fp64 resident kernel (the quantum scripts' dtype) runs the same form in natural units
// with n = -expm1(-z), d = 2 + expm1(-z) (no cancellation: both floors exact, z >= 2 lo) and
// the libm-free fp64 log (decode_resident_kernel, kRatio64): exp and two logs per edge
// instead of tanh (expm1 and a division), log, exp, cos_pi and two logs.
constexpr float kBpZmin = 2.8853900817779268e-07f;        // 2e-7 log2 e
constexpr float kBpZmax = 14.426950408889634f;             // 10 log2 e
#ifndef GNND_BP_RATIO
#define GNND_BP_RATIO 1      // 0: the product form (A/B builds)
#endif
__device__ __forceinline__ f32x2 bp_ratio_msg(f32x2 N, f32x2 D, f32x2 n, f32x2 d) {
    const f32x2 A = D * n, Bv = N * d;
    const f32x2 up = A + Bv, dn = A - Bv;
    return f32x2{__builtin_amdgcn_logf(fabsf(up.x)), __builtin_amdgcn_logf(fabsf(up.y))} -
           f32x2{__builtin_amdgcn_logf(fabsf(dn.x)), __builtin_amdgcn_logf(fabsf(dn.y))};
}
__device__ __forceinline__ f32x2 rcp2(f32x2 v) {
    return f32x2{__builtin_amdgcn_rcpf(v.x), __builtin_amdgcn_rcpf(v.y)};
}

template <int MODEL, typename T> struct EdgeMath {
    static constexpr bool BP = ModelTraits<MODEL>::bp;
    static constexpr bool kFastBP = sizeof(T) == 4 && (MODEL == GNND_CBP || MODEL == GNND_QBP);
    // v->c message update and c->v pre-op: a_e = (S_v - m_e) + x_v -> t_e (+ BP sign flag)
    // (fp32 V24 runs the paired-edge path of decode_kernel instead)
    __device__ static __forceinline__ T pre(T ext, T xv, const T* __restrict__ wv, T& cc,
                                            const T* tab = nullptr) {
        cc = T(0);
        if constexpr (kFastBP) {
            const float a = ext + xv;
            cc = a < 0.f ? 1.f : 0.f;          // tanh(clamp(a)/2) < 0 exactly when a < 0
            return bp_log2tanh_f32(a, MODEL == GNND_QBP ? 1e-20f : 1e-7f);
        } else if constexpr (BP) {
            T a = ext + xv;
            T th = g_tanh(g_clamp(a, T(-10), T(10)) / T(2));
            cc = th < T(0) ? T(1) : T(0);
            const T lo = MODEL == GNND_QBP ? cst<T>(1e-20) : cst<T>(1e-7);
            return g_log(g_clamp(g_abs(th), lo, cst<T>(1e10)));
        } else {
            return tanh_half_fast(ext + xv);
        }
    }
    // c->v update: u = S_c - t_e (BP: Lambda), n2 = leave-one-out sign count (BP)
    __device__ static __forceinline__ T post(T u, T n2, T sc, T mprev, const Mlp10F32& mlp,
                                             const T* s_w, const T* __restrict__ wv,
                                             const T* tab = nullptr) {
        if constexpr (MODEL == GNND_QGNNI || MODEL == GNND_CGNNI) {
            T y;
            if constexpr (sizeof(T) == 4) y = mlp(u);
            else y = mlp10_relu(s_w + kMlp10Msg, u);
            return (MODEL == GNND_QGNNI ? y * sc : y) + mprev;
        } else if constexpr (kFastBP) {
            if constexpr (MODEL == GNND_QBP)
                return bp_msg_f32<true>(u, n2 + (1.f - sc) / 2.f, cst<float>(1 - 1e-12));
            else
                return bp_msg_f32<false>(u, n2, cst<float>(1 - 1e-7));
        } else {
            T n = n2;
            if constexpr (MODEL == GNND_QBP) n = n + (T(1) - sc) / T(2);
            const T hi = MODEL == GNND_QBP ? cst<T>(1 - 1e-12) : cst<T>(1 - 1e-7);
            T p = g_clamp(g_exp(u) * cos_pi(n), -hi, hi);
            if constexpr (MODEL == GNND_QBP) return g_log(T(1) + p) - g_log(T(1) - p);
            else return g_log((T(1) + p) / (T(1) - p));
        }
    }
    // readout of one variable from r = S_v(+x_v)
    __device__ static __forceinline__ T readout(T r, const T* s_w) {
        if constexpr (MODEL == GNND_CGNNI)
            return g_clamp(sigmoid_ref(-mlp10_relu(s_w + kMlp10Out, r)), cst<T>(1e-7), cst<T>(1 - 1e-7));
        else if constexpr (MODEL == GNND_QGNNI)
            return sigmoid_ref(-mlp10_relu(s_w + kMlp10Out, r));
        else if constexpr (MODEL == GNND_CBP)
            return g_clamp(sigmoid_ref(-r), cst<T>(1e-7), cst<T>(1 - 1e-7));
        else
            return sigmoid_ref(-r);
    }
};

// ---------------------------------------------------------------------------------------
// streaming kernel (any model; V24 and graphs too large for the resident kernel)
// ---------------------------------------------------------------------------------------
// Per iteration (two workgroup barriers):
//  step 1  lanes = (codeword, check, lane-in-group): each lane owns R edge slots of its
//          check (G lanes per check, consecutive and aligned inside the wave).  For every
//          owned edge it forms the v->c message a_e = (S_v - m_e) + x_v from LDS, applies
//          the v->c update and the c->v pre-op, sums the check with a G-lane butterfly
//          (no LDS, no barrier), then writes m_e = update(S_c - t_e, s_c) (+ m_e) back.
//          Messages are stored in SLOT order (check-major, lane-contiguous).
//  step 2  threads = (codeword, variable): S_v = sum of m over the variable's edges in
//          the reference's index_add order (gathered through vslot).
// Training tape of the streaming kernel (decoder_v2_4, TAPE = true): per iteration and edge
// (reference edge order) the v->c MLP input ext = S_v - m, the tanh output t and the c->v
// MLP input u = S_c - t; and the final messages m^T.  Everything gnnd_train_bwd needs.
template <typename T> struct TapeView {
    T* ext;   // [iters][B][E]
    T* u;     // [iters][B][E]
    T* t;     // [iters][B][E]
    T* mT;    // [B][E]
    // optional (y non-null): decoder_v2_4's syndrome loss computed in the forward's epilogue
    // (gnnd_train_fwd_loss: unit-split small batches) -> d loss / d out and the per-codeword
    // (and component) losses, the same terms and summation orders as the reverse pass's
    // fused loss (gnnd_train.hip BwdLoss)
    const T* y;               // [B*V] labels
    const uint32_t* lmask;    // [V] logical-row bit masks (whole graph's variables)
    int nl, logical_only, ncomp;
    T* gp;                    // [B*V] d loss / d out
    T* loss_b;                // [B * ncomp]
};
// wave all-reduce through the row/bank DPP butterfly and lane 63 (the reverse pass's wave_sum:
// the forward's loss sums use the same operations so the losses are the same bits)
__device__ __forceinline__ float fwd_wave_sum(float v) {
    auto mv = [](float x, auto ctl) {
        constexpr int C = decltype(ctl)::value;
        return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), C & 0xfff,
                                                          (C >> 12) & 0xf, 0xf, false));
    };
    v += mv(v, std::integral_constant<int, 0xB1 | (0xf << 12)>{});
    v += mv(v, std::integral_constant<int, 0x4E | (0xf << 12)>{});
    v += mv(v, std::integral_constant<int, 0x141 | (0xf << 12)>{});
    v += mv(v, std::integral_constant<int, 0x140 | (0xf << 12)>{});
    v += mv(v, std::integral_constant<int, 0x142 | (0xa << 12)>{});
    v += mv(v, std::integral_constant<int, 0x143 | (0xc << 12)>{});
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}
__device__ __forceinline__ double fwd_wave_sum(double v) {
    auto mv = [](double x, auto ctl) {
        constexpr int C = decltype(ctl)::value;
        const long long b = __double_as_longlong(x);
        const int lo = __builtin_amdgcn_update_dpp(0, (int)b, C & 0xfff, (C >> 12) & 0xf, 0xf, false);
        const int hi = __builtin_amdgcn_update_dpp(0, (int)(b >> 32), C & 0xfff, (C >> 12) & 0xf, 0xf, false);
        return __longlong_as_double(((long long)hi << 32) | (unsigned)lo);
    };
    v += mv(v, std::integral_constant<int, 0xB1 | (0xf << 12)>{});
    v += mv(v, std::integral_constant<int, 0x4E | (0xf << 12)>{});
    v += mv(v, std::integral_constant<int, 0x141 | (0xf << 12)>{});
    v += mv(v, std::integral_constant<int, 0x140 | (0xf << 12)>{});
    v += mv(v, std::integral_constant<int, 0x142 | (0xa << 12)>{});
    v += mv(v, std::integral_constant<int, 0x143 | (0xc << 12)>{});
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_readlane((int)b, 63), hi = __builtin_amdgcn_readlane((int)(b >> 32), 63);
    return __longlong_as_double(((long long)hi << 32) | (unsigned)lo);
}

// US (unit split, fp32 decoder_v2_4 small batches): US waves share each wave of work items,
// each evaluating a quarter / half of every 128-hidden MLP's units (mlp128_split), so a
// latency-bound batch of a few codewords per workgroup keeps 4 / 2 times as many waves busy.
// Split graphs (gnnd_graph::comp, `views` non-null): blocks [k*cblk, (k+1)*cblk) decode
// component k of every codeword, each block a tile of CW codewords of that component's graph
// views[k]; the component's rows are addressed through its GraphView addressing fields.
// WIDE (US = 1 only): WIDE x 256 work-item lanes per workgroup, so several waves' worth of items
// share one copy of the workgroup's LDS tables (fp64 decoder_v2_4: the 33 KB Softplus table)
// IW3 (unit split only): rounds of 192 work-item lanes (three item waves x US) instead of 256 --
// a workgroup with one toric-7 component-codeword (192 edges, one per lane) then has no item
// wave without work (launched with 192 US threads; the launch bound and thus the register
// allocation stay those of the 256-lane form)
template <int MODEL, typename T, int R, bool TAPE = false, int US = 1, int WIDE = 1, bool IW3 = false>
__global__ void __launch_bounds__(unit_split_lanes<US>() * US * WIDE)
decode_kernel(GraphView g0, const T* __restrict__ w, int nw, const T* __restrict__ x,
              T* __restrict__ out, int64_t B, int iters, int CW, FastDiv dItem, FastDiv dV,
              FastDiv dN, TapeView<T> tape, const GraphView* __restrict__ views, int cblk) {
    using M = EdgeMath<MODEL, T>;
    constexpr bool BP = ModelTraits<MODEL>::bp;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    GNND_PPROF(pf);
    GNND_PSTART(pf, blockIdx.x == 0 && threadIdx.x < 64);
    int blk = blockIdx.x, comp = 0;
    GraphView g = g0;
    if (views) {                       // uniform: component k of the split graph
        const int k = blk / cblk;
        g = views[k];
        blk -= k * cblk;
        comp = k;
    }
    const int V = g.V, C = g.C, E = g.E, N = g.N, G = g.G, logG = g.logG;
    const int tid = threadIdx.x;
    static_assert(WIDE == 1 || US == 1, "wide workgroups: no unit split");
    static_assert(!IW3 || (US > 1 && US < 8), "192-lane rounds: unit split 2 or 4");
    // ILB: the partial-sum buffers' row stride (the unit-split MLPs index them by it)
    constexpr int ILB = unit_split_lanes<US>() * WIDE;
    constexpr int IL = IW3 ? 192 : ILB;                // work-item lanes
    constexpr int NT = IL * US;
    static_assert(US == 1 || (MODEL == GNND_V24 && sizeof(T) == 4 && R <= 2) ||
                      (MODEL == GNND_V24 && sizeof(T) == 8 && US <= 4),
                  "unit split: decoder_v2_4 (fp32: one slot pair per lane; fp64: US <= 4)");
    // work-item lane (0..255) and the wave's unit chunk: waves w = US i + sub share item wave i
    const int sub = US > 1 ? __builtin_amdgcn_readfirstlane((tid >> 6) % US) : 0;
    const int itid = US > 1 ? ((tid >> 6) / US) * 64 + (tid & 63) : tid;

    // fp64 V24: the Softplus table (gnnd_common.h kSpTab, indexed per lane) at LDS byte 0,
    // then the three MLPs' layer-1 biases [3][128]
    constexpr bool kTab = MODEL == GNND_V24 && sizeof(T) == 8;
    T* s_w = (T*)smem;
    size_t off = ((size_t)nw * sizeof(T) + 15) & ~(size_t)15;
    T* s_tab = nullptr;
    T* s_bias = nullptr;
    T* s_lin = nullptr;        // [3][4] {A, B, C, 0} per MLP (mlp_lin), after the biases
    T* s_ctab = nullptr;           // [ctab_entries(max_dc)][kCtabNC] check-MLP table entries
    const int Rc = g.max_dc > 1 ? g.max_dc - 1 : 0, R8 = kCtabInv * Rc;
    constexpr bool kCtab = MODEL == GNND_V24 && GNND_V24_CTAB;
    if constexpr (kCtab && sizeof(T) == 4) {          // fp32 V24: the table at LDS byte 0
        s_ctab = (T*)smem;
        off = ((size_t)ctab_entries(g.max_dc) * kCtabNC * 4 + 15) & ~(size_t)15;
    }
    if constexpr (kTab) {
        s_tab = (T*)smem;
        s_bias = s_tab + kV24F64TabDoubles;
        s_lin = s_bias + 3 * 128;
        s_ctab = s_lin + 16;
        off = (size_t)(kV24F64TabDoubles + 3 * 128 + 16) * 8 +
              (GNND_V24_CTAB ? (size_t)ctab_entries(g.max_dc) * kCtabNC * 8 : 0);
        if (tid < 64) {            // wave 0: fixed-order 128-term dot products (same in every block)
            for (int m = 0; m < 3; ++m) {
                const T* wm = w + (m == 0 ? kV24Ggc1 : m == 1 ? kV24Ggc2 : kV24Mlp);
                const int o2 = m == 0 ? 384 : 256;
                for (int q = 0; q < 3; ++q) {
                    const int oa = q == 0 ? 0 : q == 1 ? 128 : (m == 0 ? 256 : 128);
                    T v = T(0);
                    if (q != 1 || m == 0) {
                        const T pl = fma(wm[o2 + tid + 64], wm[oa + tid + 64], wm[o2 + tid] * wm[oa + tid]);
                        v = group_sum_c<64>(pl) * T(0.5);
                    }
                    if (tid == 0) s_lin[4 * m + q] = v;
                }
                // the pre-activation bound's weight factor (mlp_wave_big): a 64-lane max
                const T* b1p = wm + (m == 0 ? 256 : 128);
                T wmx = T(0);
                for (int k = tid; k < 128; k += 64)
                    wmx = fmax(wmx, fabs(wm[k]) + (m == 0 ? fabs(wm[128 + k]) : T(0)) + fabs(b1p[k]));
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) wmx = fmax(wmx, __shfl_xor(wmx, o));
                if (tid == 0) s_lin[4 * m + 3] = wmx;
            }
        }
        for (int i = tid; i < kV24F64TabDoubles; i += NT) s_tab[i] = v24_f64_tab_entry(i);
        for (int i = tid; i < 3 * 128; i += NT) {
            const int m = i >> 7, k = i & 127;
            s_bias[i] = w[m == 0 ? kV24Ggc1 + 256 + k : (m == 1 ? kV24Ggc2 : kV24Mlp) + 128 + k];
        }
    }
    // the check-side MLP's table entries |c_j| <= R from the prepared weights (uniform verdict)
    bool ctab_ok = false;
    if constexpr (kCtab) {
        ctab_ok = ctab_valid(w, Rc);
        if (ctab_ok) {
            constexpr int kV = 16 / sizeof(T);            // values per 16-byte move
            const uint4* src = (const uint4*)(w + kV24CtabOff + (size_t)(kCtabInv * kCtabRcap - R8) * kCtabNC);
            for (int i = tid; i < ctab_entries(g.max_dc) * kCtabNC / kV; i += NT) ((uint4*)s_ctab)[i] = src[i];
        }
    }
    const int nslot = C * G * R;
    uint32_t* s_slot = (uint32_t*)(smem + off);
    int* s_vptr = (int*)(s_slot + nslot);
    int* s_vslot = s_vptr + V + 1;
    off += (((size_t)nslot + V + 1 + E) * 4 + 15) & ~(size_t)15;
    T* s_m = (T*)(smem + off);                             // [CW][nslot] c->v messages
    SumX<T>* s_sx = (SumX<T>*)(s_m + (size_t)CW * nslot);  // [CW][V]  {S_v, x_v}
    T* s_xc = (T*)(s_sx + (size_t)CW * V);                 // [CW][C]  check-row features
    constexpr bool kV24F32 = MODEL == GNND_V24 && sizeof(T) == 4;
    constexpr bool kV24F64 = MODEL == GNND_V24 && sizeof(T) == 8;
    // fp64 V24: [CW] the codeword's channel-prior table (offset into w, -1: none; vtab_eval)
    int* s_vto = (int*)(s_xc + (size_t)CW * C);
    // unit split: two [US][IL] f32x2 buffers for the MLP partial sums (8-byte aligned)
    // (offset arithmetic on the __shared__ base keeps the LDS address space: ds_* accesses,
    // not flat ones as through an integer cast of the pointer)
    f32x2* s_part = (f32x2*)(smem + ((((char*)(s_vto + (kV24F64 ? CW : 0)) - smem) + 7) & ~(ptrdiff_t)7));
    // channel-prior tables of the variable-side MLP (fp64 V24 decodes with one wave per item
    // group: the unit-split and training-tape forms evaluate the units)
    int n_pt = 0;
    if constexpr (kV24F64 && US == 1 && !TAPE) n_pt = (int)w[kV24PriorHdr];
    // fp32 V24 on the R = 1 slot plan (B <= 4096): the unit-pair MLPs (mlp128_upair), their
    // pair-major weights staged in LDS after the unit split's partial-sum buffers
    constexpr bool kUP = kV24F32 && R == 1 && US <= 4;
    float* s_up = (float*)(smem + ((((char*)(s_part + (US > 1 ? 2 * US * ILB : 0))) - smem) + 15 & ~(ptrdiff_t)15));
    if constexpr (kUP) stage_upair((const float*)w, s_up, tid);
    double* s_pd = (double*)s_part;                        // fp64 unit split: [2][US][256]
    // fp64 unit split: the three MLPs' chain-major weights [3][128] (16-byte aligned) after it
    WcmEntry* s_wcm = (WcmEntry*)(smem + ((((char*)(s_pd + 2 * US * GNND_BLOCK) - smem) + 15) & ~(ptrdiff_t)15));
    if constexpr (MODEL == GNND_V24 && sizeof(T) == 8 && US > 1 && GNND_F64_SPTAB) {
        for (int i = tid; i < 3 * 128; i += NT) {     // entry 32 j + i of MLP m: unit k = 4 i + j
            const int m = i >> 7, pos = i & 127, k = 4 * (pos & 31) + (pos >> 5);
            const T* wm = w + (m == 0 ? kV24Ggc1 : m == 1 ? kV24Ggc2 : kV24Mlp);
            WcmEntry e;
            e.w1a = wm[k];
            e.w1b = m == 0 ? wm[128 + k] : 0.0;
            e.b1 = wm[(m == 0 ? 256 : 128) + k];
            e.w2 = wm[(m == 0 ? 384 : 256) + k];
            s_wcm[i] = e;
        }
    }
    // Tiles: tile = blk, blk + grid, ... below cblk (the launch's tiles per component).  A
    // persistent launch (launch_decode: fp64 decoder_v2_4 at large batches, one workgroup per
    // resident slot) runs several, paying the per-workgroup prologue above -- the Softplus
    // table, the check-MLP table -- once per slot instead of once per tile; every other launch
    // has one tile per workgroup (split graphs: exactly one).
    for (int tile = blk; tile < cblk; tile += views ? cblk : (int)gridDim.x) {
    const int64_t b0 = (int64_t)tile * CW;
    const int nb = (int)((B - b0) < CW ? (B - b0) : CW);
    // fp32 decoder_v2_4 reads its weights through the scalar cache only (no LDS copy); with
    // every table and the tile's rows within one element per thread (small batches: one
    // component-codeword per workgroup) all global loads are issued before any LDS store, so
    // their latencies overlap instead of one loop after another
    const bool one = kV24F32 && nslot <= NT && V + 1 <= NT && E <= NT && nb * N <= NT;
    if (one) {
        const int i = tid;
        const uint32_t a_sl = i < nslot ? g.slot_ve[i] : 0u;
        const int a_vp = i <= V ? g.var_ptr[i] : 0;
        const int a_vs = i < E ? g.vslot[i] : 0;
        const int bx = fdiv(i < nb * N ? i : 0, dN), nx = (i < nb * N ? i : 0) - bx * N;
        const T* xr = x + (size_t)(b0 + bx) * g.xs;
        const T a_x = i < nb * N ? (nx < V ? xr[g.xv0 + nx] : xr[g.xc0 + nx - V]) : T(0);
        if (i < nslot) s_slot[i] = a_sl;
        if (i <= V) s_vptr[i] = a_vp;
        if (i < E) s_vslot[i] = a_vs;
        if (i < nb * N) {
            if (nx < V) s_sx[bx * V + nx] = SumX<T>{T(0), a_x};
            else s_xc[bx * C + nx - V] = a_x;
        }
    } else {
        if constexpr (!kV24F32)
            for (int i = tid; i < nw; i += NT) s_w[i] = w[i];
        for (int i = tid; i < nslot; i += NT) s_slot[i] = g.slot_ve[i];   // v | e << 16
        for (int i = tid; i <= V; i += NT) s_vptr[i] = g.var_ptr[i];
        for (int i = tid; i < E; i += NT) s_vslot[i] = g.vslot[i];
        // the tile's rows (whole graph: one contiguous run of nb*N values)
        for (int i = tid; i < nb * N; i += NT) {
            int b = fdiv(i, dN), n = i - b * N;
            const T* xr = x + (size_t)(b0 + b) * g.xs;
            if (n < V) s_sx[b * V + n] = SumX<T>{T(0), xr[g.xv0 + n]};
            else s_xc[b * C + n - V] = xr[g.xc0 + n - V];
            if constexpr (kV24F64) {
                if (n_pt > 0 && n == 0) {     // the table whose prior is the codeword's first x_v
                    const long long xb = __double_as_longlong((double)xr[g.xv0]);
                    int to = -1;
                    for (int t = 0; t < n_pt; ++t)
                        if (__double_as_longlong((double)w[kV24PriorOff + (size_t)t * kVtStride]) == xb) {
                            to = kV24PriorOff + t * kVtStride;
                            break;
                        }
                    s_vto[b] = to;
                }
            }
        }
    }
    for (int i = tid; i < nb * nslot; i += NT) s_m[i] = T(0);
    __syncthreads();

    // 128-hidden weights stream through the scalar cache into SGPRs (uniform addresses):
    // no LDS traffic, one SGPR operand per packed FMA.  Broadcast ds_read_b128 of the same
    // weights from LDS costs 4 LDS cycles per 4 floats per wave and saturated the LDS pipe.
    const T* __restrict__ wv = w;
    V24F32 v24{(const float*)w, {}, {}, {}};
    if constexpr (kV24F32) {
        v24.l1 = v24_lin2((const float*)w + kV24Ggc1);
        v24.l2 = v24_lin1((const float*)w + kV24Ggc2);
        v24.l3 = v24_lin1((const float*)w + kV24Mlp);
    }
    Mlp10F32 mlp_msg;   // 10-hidden message MLP weights live in VGPRs for the whole decode
    if constexpr (sizeof(T) == 4 && (MODEL == GNND_CGNNI || MODEL == GNND_QGNNI))
        mlp_msg.load((const float*)s_w + kMlp10Msg, (float)g.max_dc);
    constexpr bool WBP = ModelTraits<MODEL>::wbp;
    const WbpW<MODEL, T> ww{w, E, iters};
    T alpha = T(0);
    if constexpr (WBP) alpha = ww.alpha();

    const int IC = C * G;               // work items (lanes) per codeword
    const int nItem = nb * IC;          // a multiple of G: groups never straddle the end
    const int nV = nb * V;
    // the syndrome loss in the epilogue (gnnd_train_fwd_loss): labels and logical masks of the
    // first element per thread are loaded now, their latency hidden behind the iterations
    constexpr bool kFLoss = kV24F32 && TAPE && US > 1;
    const bool floss = kFLoss && tape.y != nullptr;
    T ypre = T(0);
    uint32_t lmpre = 0u;
    if (floss) {
        if (tid < nV) {
            const int b = fdiv(tid, dV), v = tid - b * V;
            ypre = tape.y[(size_t)(b0 + b) * g.os + g.o0 + v];
        }
        if (tid < V && tape.nl > 0) lmpre = tape.lmask[g.o0 + tid];
    }
    // unit-split small batches (one round of items): each lane's slots are fixed for the whole
    // decode, so it gathers its variables' messages itself (indices and x_v kept in registers,
    // summed in var_ptr order = var_sum's order: the same S_v bits) and the variable-sum step
    // and its barrier go (the unit split's barriers order this iteration's gathers before its
    // message writes)
    constexpr bool kGath = kV24F32 && US > 1;
    constexpr int kGDv = 4;
#ifdef GNND_NO_GATHER
    const bool gath = false;
#else
    const bool gath = kGath && g.max_dv <= kGDv && nItem <= IL;
#endif
    int gidx[kGath ? R : 1][kGDv], gcnt[kGath ? R : 1];
    float gx[kGath ? R : 1];
    if constexpr (kGath) {
        if (gath) {
            const int fc = itid < nItem ? itid : nItem - 1;
            const int b = fdiv(fc, dItem), rem = fc - b * IC;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const uint32_t sv = s_slot[rem * R + r];
                const int v = (int)(sv & 0xffffu);
                const int k0 = s_vptr[v], ke = s_vptr[v + 1];
                gcnt[r] = (int)(sv >> 16) != E ? ke - k0 : 0;
#pragma unroll
                for (int j = 0; j < kGDv; ++j) gidx[r][j] = b * nslot + s_vslot[min(k0 + j, ke - 1)];
                gx[r] = s_sx[b * V + v].x;
            }
        }
    }
    GNND_PMARK(pf, 11);
    // fp64 unit split: the partial-sum buffer of the next mlp128d_split call (the two buffers
    // alternate call by call, so a buffer is rewritten only after a barrier that follows every
    // read of its previous contents)
    int pbuf = 0;
    // fp64 decoder_v2_4 with channel-prior tables (one slot per item): TWO work items per lane per
    // pass (rounds f0 and f0 + IL), their LDS reads, table fetches and check-MLP entries issued
    // together -- the variable-side MLP is one L2 round trip per edge, and one item per lane left
    // the waves waiting on it (SQ_WAIT_ANY 0.60, profiles/pmc_classes_v24_toric_5_T15_f64_ptab)
#ifndef GNND_PT_ITEMS
#define GNND_PT_ITEMS 2            // work items per lane per pass (2 or 3; 3 measured slower:
#endif                             // 147 VGPRs = 3 waves per SIMD, or spills at 128 -- r06m)
    constexpr bool kPt2 = kV24F64 && US == 1 && !TAPE && R == 1;
    const bool pt2 = kPt2 && n_pt > 0;
    for (int it = 0; it < iters; ++it) {
        if constexpr (kPt2) {
            // one pass: items i = 0 .. NI-1 of rounds f0 + i IL; a wave whose later rounds hold no
            // live item runs the instantiation with fewer items (no work on clamped copies)
            auto pass_n = [&](int f0, auto nC) {
                constexpr int NI = decltype(nC)::value;
                bool act[NI], val[NI], need[NI], hit[NI];
                int bI[NI], rem[NI];
                T* mb[NI];
                T mv[NI], ext[NI], xs[NI], sc[NI], a[NI], tv[NI], y[NI];
                const double* tb[NI];
                VtCell cell[NI];
                const bool idle0 = __builtin_amdgcn_readfirstlane(f0 + (itid & ~63)) >= nItem;
#pragma unroll
                for (int i = 0; i < NI; ++i) {
                    const int f = f0 + i * IL + itid;
                    act[i] = f < nItem;
                    const int fc = act[i] ? f : nItem - 1;
                    bI[i] = fdiv(fc, dItem);
                    rem[i] = fc - bI[i] * IC;
                    const uint32_t sv = s_slot[rem[i]];
                    mb[i] = s_m + bI[i] * nslot + rem[i];
                    val[i] = (int)(sv >> 16) != E;
                    mv[i] = *mb[i];
                    const SumX<T> p = s_sx[bI[i] * V + GNND_DIDX((int)(sv & 0xffffu), V, GNND_DBG_VAR)];
                    ext[i] = p.s - mv[i];
                    xs[i] = p.x;
                    const int vto = s_vto[bI[i]];
                    tb[i] = (const double*)wv + (vto >= 0 ? vto : kV24PriorOff);
                }
#pragma unroll
                for (int i = 0; i < NI; ++i) cell[i] = vtab_fetch<kVtInvG, true>(tb[i], ext[i]);
#pragma unroll
                for (int i = 0; i < NI; ++i) sc[i] = s_xc[bI[i] * C + (rem[i] >> logG)];
                // (a hit gives t = tanh(ggc1.mlp/2) itself; the units give the MLP output)
#pragma unroll
                for (int i = 0; i < NI; ++i) {
                    a[i] = T(0);
                    hit[i] = vtab_finish<kVtInvG, true>(tb[i], cell[i], ext[i], xs[i], a[i]);
                    need[i] = act[i] && val[i] && !hit[i];
                }
                // (the wave evaluates the 128 units where a live lane's (u, x_v) has no table)
#pragma unroll
                for (int i = 0; i < NI; ++i) {
                    if (__builtin_amdgcn_ballot_w64(need[i]) != 0) {
                        const T a2 = mlp128d_split<1, true>(wv + kV24Ggc1, s_bias, ext[i], xs[i], 0, s_pd, itid,
                                                            i == 0 ? idle0 : false, s_tab, s_lin, s_wcm);
                        if (need[i]) a[i] = a2;
                    }
                }
#pragma unroll
                for (int i = 0; i < NI; ++i) {
                    tv[i] = val[i] ? (hit[i] ? a[i] : tanh_half_fast(a[i])) : T(0);
                    const T Sc = group_sum(tv[i], G);
                    a[i] = Sc - tv[i];                       // the check-side MLP's input u
                }
                if (ctab_ok) {               // (uniform)
#pragma unroll
                    for (int i = 0; i < NI; ++i) y[i] = ctab_eval(s_ctab, a[i], R8);
                } else {
#pragma unroll
                    for (int i = 0; i < NI; ++i)
                        y[i] = mlp128d_split<1, false>(wv + kV24Ggc2, s_bias + 128, a[i], a[i], 0, s_pd, itid,
                                                       i == 0 ? idle0 : false, s_tab, s_lin + 4, s_wcm + 128);
                }
#pragma unroll
                for (int i = 0; i < NI; ++i)
                    if (act[i]) *mb[i] = y[i] * sc[i] + mv[i];
            };
            constexpr int kNI = GNND_PT_ITEMS;
            for (int f0 = 0; f0 < (pt2 ? nItem : 0); f0 += kNI * IL) {
                // live rounds in this wave's pass (uniform)
                int live = 1;
                for (int i = 1; i < kNI; ++i)
                    live += __builtin_amdgcn_readfirstlane(f0 + i * IL + (itid & ~63)) < nItem ? 1 : 0;
                if constexpr (kNI >= 3) {
                    if (live == 3) { pass_n(f0, std::integral_constant<int, 3>{}); continue; }
                }
                if (live == 2) pass_n(f0, std::integral_constant<int, 2>{});
                else pass_n(f0, std::integral_constant<int, 1>{});
            }
        }
        for (int f0 = 0; f0 < (pt2 ? 0 : nItem); f0 += IL) {
            const int f = f0 + itid;
            const bool act = f < nItem;
            const bool own = act && sub == 0;            // the unit-split waves' writer
            // no live item in this wave (last round of a partial tile): skip the 128-unit MLPs
            const bool widle = __builtin_amdgcn_readfirstlane(f0 + (itid & ~63)) >= nItem;
            const int fc = act ? f : nItem - 1;          // idle groups compute on a copy
            const int b = fdiv(fc, dItem);
            const int rem = fc - b * IC;
            const int c = rem >> logG;
            const uint32_t* sl = s_slot + rem * R;       // (c*G + g)*R
            T* mb = s_m + b * nslot + rem * R;           // this lane's R message slots
            const SumX<T>* sxb = s_sx + b * V;
            T mv[R], tv[R], cf[R];
            T tsum = T(0), csum = T(0);
            if constexpr (kV24F32) {
                // slots in pairs through the two-edge MLP (odd R: the last pair repeats)
                float ext[R], xs[R];
                bool val[R];
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const uint32_t sv = sl[r];
                    val[r] = (int)(sv >> 16) != E;
                    mv[r] = mb[r];
                    if constexpr (kGath) {
                        if (gath) {
                            float m[kGDv];
#pragma unroll
                            for (int j = 0; j < kGDv; ++j) m[j] = s_m[gidx[r][j]];
                            float S = 0.f;
#pragma unroll
                            for (int j = 0; j < kGDv; ++j)
                                if (j < gcnt[r]) S += m[j];
                            ext[r] = S - mv[r];
                            xs[r] = gx[r];
                            continue;
                        }
                    }
                    const SumX<T> p = sxb[sv & 0xffffu];
                    ext[r] = p.s - mv[r];
                    xs[r] = p.x;
                }
                GNND_PMARK(pf, 0);
                if constexpr (kUP) {
                    // one edge per lane, two hidden units per packed op (with the check MLP on its
                    // table the var MLP's two partial-sum buffers alternate call by call)
                    float* pb = (float*)(s_part + (ctab_ok && (pbuf++ & 1) ? US * ILB : 0));
                    const float a = mlp128_upair_split<US, true>(s_up + UpairLds::kMlp0, v24.l1, ext[0], xs[0],
                                                                 sub, pb, itid, widle);
                    tv[0] = val[0] ? tanh_half_fast(a) : 0.f;
                } else {
#pragma unroll
                    for (int r = 0; r < R; r += 2) {
                        const int r1 = r + 1 < R ? r + 1 : r;
                        f32x2* pb = s_part + (ctab_ok && (pbuf++ & 1) ? US * ILB : 0);
                        const f32x2 a = mlp128_split<US, true>(v24.g + kV24Ggc1, v24.l1, f32x2{ext[r], ext[r1]},
                                                               f32x2{xs[r], xs[r1]}, sub, pb, itid, widle
                                                               GNND_PARG(pf, 1));
                        tv[r] = val[r] ? tanh_half_fast(a.x) : 0.f;
                        if (r + 1 < R) tv[r + 1] = val[r + 1] ? tanh_half_fast(a.y) : 0.f;
                    }
                }
                if constexpr (TAPE) {
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        const int e = (int)(sl[r] >> 16);
                        if (own && e != E) {
                            const size_t row = ((size_t)it * B + b0 + b) * g.es + g.e0 + e;
                            tape.ext[row] = ext[r];
                            tape.t[row] = tv[r];
                        }
                    }
                }
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    cf[r] = T(0);
                    tsum += tv[r];
                }
            } else if constexpr (kV24F64) {
                // the reference dtype: one slot at a time through the fp64 chain-form MLP (unit
                // split over US waves at small batches; partial-sum buffer = call index & 1)
                T ext[R], xs[R];
                bool val[R];
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const uint32_t sv = sl[r];
                    val[r] = (int)(sv >> 16) != E;
                    mv[r] = mb[r];
                    const SumX<T> p = sxb[GNND_DIDX((int)(sv & 0xffffu), V, GNND_DBG_VAR)];
                    ext[r] = p.s - mv[r];
                    xs[r] = p.x;
                }
                const int vto = n_pt > 0 ? s_vto[b] : -1;
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    T a = T(0);
                    // the channel-prior table where this lane's (u, x_v) has one; the wave
                    // evaluates the 128 units when any live lane has none (those lanes keep them)
                    bool need = n_pt == 0 || (act && val[r]);
                    // (no table for the codeword's first prior: table 0, whose key then decides --
                    // a variable whose x_v is table 0's prior is covered by it all the same)
                    // (a hit gives t = tanh(ggc1.mlp/2) itself; the units give the MLP output)
                    const bool hit = n_pt > 0 && vtab_eval<kVtInvG, true>(
                                                     (const double*)wv + (vto >= 0 ? vto : kV24PriorOff), ext[r], xs[r], a);
                    if (hit) need = false;
                    if (n_pt == 0 || __builtin_amdgcn_ballot_w64(need) != 0) {
                        const T a2 = mlp128d_split<US, true>(wv + kV24Ggc1, s_bias, ext[r], xs[r], sub,
                                                             s_pd + (pbuf++ & 1) * US * GNND_BLOCK, itid, widle,
                                                             s_tab, s_lin, s_wcm);
                        if (need) a = a2;
                    }
                    tv[r] = val[r] ? (hit ? a : tanh_half_fast(a)) : T(0);
                    cf[r] = T(0);
                    tsum += tv[r];
                    if constexpr (TAPE) {
                        if (own && val[r]) {
                            const size_t row = ((size_t)it * B + b0 + b) * g.es + g.e0 + (int)(sl[r] >> 16);
                            tape.ext[row] = ext[r];
                            tape.t[row] = tv[r];
                        }
                    }
                }
            } else if constexpr (WBP) {
                // v->c with this iteration's per-edge weights, then the BP pre-op
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const uint32_t sv = sl[r];
                    const int e = (int)(sv >> 16);
                    const bool valid = e != E;
                    const int ec = valid ? e : 0;
                    mv[r] = mb[r];
                    const SumX<T> p = sxb[sv & 0xffffu];
                    T a;
                    if constexpr (MODEL == GNND_NBP)   // LOO_v(W m) + x_v W_p  (neural_BP.py:248-260)
                        a = (p.s - mv[r] * ww.msg(it, ec)) + p.x * ww.prior(it, ec);
                    else                               // (LOO_v(m) + x_v) W  (decoder_v1_0.py:248-251)
                        a = ((p.s - mv[r]) + p.x) * ww.chk(it, ec);
                    T cc;
                    const T L = wbp_L(a, cc);
                    tv[r] = valid ? L : T(0);
                    cf[r] = valid ? cc : T(0);
                    tsum += tv[r];
                    csum += cf[r];
                }
            } else {
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const uint32_t sv = sl[r];
                    const bool valid = (int)(sv >> 16) != E;
                    mv[r] = mb[r];
                    const SumX<T> p = sxb[GNND_DIDX((int)(sv & 0xffffu), V, GNND_DBG_VAR)];  // padding: variable 0
                    T cc;
                    T t = M::pre(p.s - mv[r], p.x, wv, cc, s_tab);
                    tv[r] = valid ? t : T(0);
                    cf[r] = valid ? cc : T(0);
                    tsum += tv[r];
                    if constexpr (BP) csum += cf[r];
                    if constexpr (TAPE) {
                        if (act && valid) {
                            const size_t row = ((size_t)it * B + b0 + b) * g.es + g.e0 + (int)(sv >> 16);
                            tape.ext[row] = p.s - mv[r];
                            tape.t[row] = t;
                        }
                    }
                }
            }
            const T Sc = group_sum(tsum, G);
            T Sc2 = T(0);
            if constexpr (BP) Sc2 = group_sum(csum, G);
            const T sc = s_xc[b * C + c];
            T mn[R];
            if constexpr (TAPE) {
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const int e = (int)(sl[r] >> 16);
                    if (own && e != E) tape.u[((size_t)it * B + b0 + b) * g.es + g.e0 + e] = Sc - tv[r];
                }
            }
            if constexpr (kUP) {
                GNND_PMARK(pf, 3);
                const float u = Sc - tv[0];
                const float y = ctab_ok ? ctab_eval(s_ctab, u, R8)   // (uniform: every split wave)
                                        : mlp128_upair_split<US, false>(s_up + UpairLds::kMlp1, v24.l2, u, u, sub,
                                                                        (float*)(s_part + US * ILB), itid, widle);
                mn[0] = y * sc + mv[0];
            } else if constexpr (kV24F32) {
                GNND_PMARK(pf, 3);
#pragma unroll
                for (int r = 0; r < R; r += 2) {
                    const int r1 = r + 1 < R ? r + 1 : r;
                    const f32x2 uu = {Sc - tv[r], Sc - tv[r1]};
                    const f32x2 y = ctab_ok ? f32x2{ctab_eval(s_ctab, uu.x, R8), ctab_eval(s_ctab, uu.y, R8)}
                                            : mlp128_split<US, false>(v24.g + kV24Ggc2, v24.l2, uu, uu, sub,
                                                                      s_part + US * ILB, itid, widle GNND_PARG(pf, 4));
                    mn[r] = y.x * sc + mv[r];
                    if (r + 1 < R) mn[r + 1] = y.y * sc + mv[r + 1];
                }
            } else if constexpr (kV24F64) {
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const T u = Sc - tv[r];
                    T y;
                    if (ctab_ok)                 // (uniform) every unit-split wave evaluates it
                        y = ctab_eval(s_ctab, u, R8);
                    else
                        y = mlp128d_split<US, false>(wv + kV24Ggc2, s_bias + 128, u, u, sub,
                                                     s_pd + (pbuf++ & 1) * US * GNND_BLOCK, itid,
                                                     widle, s_tab, s_lin + 4, s_wcm + 128);
                    mn[r] = y * sc + mv[r];
                }
            } else if constexpr (WBP) {
#pragma unroll
                for (int r = 0; r < R; ++r)   // m = BP(.) + m_prev @ alpha  (neural_BP.py:304)
                    mn[r] = wbp_out(Sc - tv[r], Sc2 - cf[r], sc) + mv[r] * alpha;
            } else {
#pragma unroll
                for (int r = 0; r < R; ++r)   // every slot computes; padding slots are never read
                    mn[r] = M::post(Sc - tv[r], Sc2 - cf[r], sc, mv[r], mlp_msg, s_w, wv, s_tab);
            }
            if (own) {
#pragma unroll
                for (int r = 0; r < R; ++r) mb[r] = mn[r];
            }
            GNND_PMARK(pf, 6);
        }
        __syncthreads();
        GNND_PMARK(pf, 7);
        if (it + 1 == iters) break;
        if (gath) continue;                 // (uniform) the lanes gather S_v themselves
        for (int f = tid; f < nV; f += NT) {
            const int b = fdiv(f, dV), v = f - b * V;
            if constexpr (MODEL == GNND_NBP)   // S_v of the next layer's weighted messages
                s_sx[f].s = var_sum_w(s_m + b * nslot, s_vslot, s_vptr[v], s_vptr[v + 1],
                                      w + (size_t)2 * (it + 1) * E);
            else
                s_sx[f].s = var_sum(s_m + b * nslot, s_vslot, s_vptr[v], s_vptr[v + 1]);
        }
        GNND_PMARK(pf, 8);
        __syncthreads();
        GNND_PMARK(pf, 9);
    }

    if constexpr (TAPE) {
        for (int f = tid; f < nb * nslot; f += NT) {
            const int b = f / nslot, sl = f - b * nslot;
            const int e = (int)(s_slot[sl] >> 16);
            if (e != E) tape.mT[(size_t)(b0 + b) * g.es + g.e0 + e] = s_m[f];
        }
    }
    if constexpr (MODEL == GNND_V24) {
        // per-edge MLP_o(m_e), then variable sums (decoder_v2_4.py:291-292)
        if constexpr (kUP) {
            // unit pairs: item lane itid evaluates message f0 + itid (the US waves sharing it a
            // pair group each); the two partial-sum buffers alternate between rounds
            const int n = nb * nslot;
            int rb = 0;
            for (int f0 = 0; f0 < n; f0 += IL, rb ^= 1) {
                const int f = f0 + itid;
                const bool widle = __builtin_amdgcn_readfirstlane(f0 + (itid & ~63)) >= n;
                const float m = s_m[f < n ? f : n - 1];
                const float y = mlp128_upair_split<US, false>(s_up + UpairLds::kMlp2, v24.l3, m, m, sub,
                                                              (float*)(s_part + rb * US * ILB), itid, widle);
                if (sub == 0 && f < n) s_m[f] = y;
            }
        } else if constexpr (kV24F32 && US > 1) {
            // unit split here too: item lane itid evaluates slot pair f0 + 2 itid, the US waves
            // sharing it a chain group each (same bits as the whole MLP in one lane); the two
            // partial-sum buffers alternate between rounds (one barrier per round)
            const int n = nb * nslot;
            int rb = 0;
            for (int f0 = 0; f0 < n; f0 += 2 * IL, rb ^= 1) {
                const int f = f0 + 2 * itid;
                const bool widle = __builtin_amdgcn_readfirstlane(f0 + 2 * (itid & ~63)) >= n;
                const int fa = f < n ? f : n - 1;
                const int f1 = fa + 1 < n ? fa + 1 : fa;
                const f32x2 m2 = {s_m[fa], s_m[f1]};
                const f32x2 y = mlp128_split<US, false>(v24.g + kV24Mlp, v24.l3, m2, m2, sub,
                                                        s_part + rb * US * ILB, itid, widle);
                if (sub == 0 && f < n) {
                    s_m[f] = y.x;
                    if (f + 1 < n) s_m[f + 1] = y.y;
                }
            }
        } else if constexpr (kV24F32) {
            const int n = nb * nslot;
            for (int f = 2 * tid; f < n; f += 2 * NT) {
                const int f1 = f + 1 < n ? f + 1 : f;
                const f32x2 y = mlp128_sp2(v24.g + kV24Mlp, v24.l3, f32x2{s_m[f], s_m[f1]});
                s_m[f] = y.x;
                if (f + 1 < n) s_m[f + 1] = y.y;
            }
        } else if constexpr (US > 1) {
            // fp64 unit split: item lane itid evaluates message f0 + itid, the US waves a chain
            // group each (the same bits as the whole MLP in one lane)
            const int n = nb * nslot;
            int rb = 0;
            for (int f0 = 0; f0 < n; f0 += IL, rb ^= 1) {
                const int f = f0 + itid;
                const bool widle = __builtin_amdgcn_readfirstlane(f0 + (itid & ~63)) >= n;
                const T m = s_m[f < n ? f : n - 1];
                const T y = mlp128d_split<US, false>(wv + kV24Mlp, s_bias + 256, m, m, sub,
                                                     s_pd + rb * US * GNND_BLOCK, itid, widle, s_tab,
                                                     s_lin + 8, s_wcm + 256);
                if (sub == 0 && f < n) s_m[f] = y;   // (lanes read only their own message)
            }
        } else if (n_pt > 0 && w[kV24PriorHdr + 1] != T(0)) {     // (uniform) the readout table
            const double* rt = (const double*)wv + kV24PriorOff + (size_t)n_pt * kVtStride;
            const int n = nb * nslot;
            for (int f0 = 0; f0 < n; f0 += NT) {
                const int f = f0 + tid;
                const T m = s_m[f < n ? f : n - 1];
                T y = T(0);
                bool need = f < n;
                if (vtab_eval<kVtInvR, false>(rt, m, 0.0, y)) need = false;   // (f >= n: need false)
                if (__builtin_amdgcn_ballot_w64(need) != 0) {
                    const T y2 = mlp128_sp(wv + kV24Mlp, s_bias + 256, m, s_tab, s_lin + 8);
                    if (need) y = y2;
                }
                if (f < n) s_m[f] = y;
            }
        } else {
            for (int f = tid; f < nb * nslot; f += NT) s_m[f] = mlp128_sp(wv + kV24Mlp, s_bias + 256, s_m[f], s_tab, s_lin + 8);
        }
        __syncthreads();
    }
    for (int f = tid; f < nV; f += NT) {
        const int b = fdiv(f, dV), v = f - b * V;
        const size_t orow = (size_t)(b0 + b) * g.os + g.o0 + v;
        if constexpr (MODEL == GNND_NBP) {
            // sum_v(m W) + sum_v(x_v W_p)  (neural_BP.py:307-312), each in edge order
            const int k0 = s_vptr[v], ke = s_vptr[v + 1];
            const T s1 = var_sum_w(s_m + b * nslot, s_vslot, k0, ke, w + (size_t)2 * iters * E);
            const T xv = s_sx[f].x;
            T s2 = T(0);
            for (int k = k0; k < ke; ++k) s2 += xv * ww.out_p(k);
            out[orow] = sigmoid_ref(-(s1 + s2));
        } else {
            const T s = var_sum(s_m + b * nslot, s_vslot, s_vptr[v], s_vptr[v + 1]);
            const T pr = M::readout(s + s_sx[f].x, s_w);
            out[orow] = pr;
            // (the unit split's partial-sum buffers are free after the readout MLP's barrier)
            if constexpr (kFLoss)
                if (floss) ((T*)s_part)[f] = (f < NT ? ypre : tape.y[orow]) + pr;
        }
    }
    if constexpr (kFLoss) {
        if (floss) {
            // quantum/decoder_v2_4.py:297-317 on this tile (one component of each codeword when
            // split): s = y + p; check rows (slot order = cedge order) and logical rows
            // (variables ascending) -> |sin| terms and d|sin(pi/2 s_r)| / d s_r; d loss / d p_v
            // over v's edges in var_ptr order, then its logical rows — the reverse pass's fused
            // loss (gnnd_train.hip) term by term, so d out and the losses are the same bits
            const int nr = C + tape.nl, GR = G * R;
            T* s_ls = (T*)s_part;                          // [nb][V] y + p
            T* s_lg = s_ls + (size_t)nb * V;               // [nb][nr] row gradients
            T* s_lt = s_lg + (size_t)nb * nr;              // [nb][nr] row terms
            uint32_t* s_lm = (uint32_t*)(s_lt + (size_t)nb * nr);   // [V]
            for (int v = tid; v < V; v += NT)
                s_lm[v] = v < NT ? lmpre : (tape.nl > 0 ? tape.lmask[g.o0 + v] : 0u);
            __syncthreads();
            const T kPi = T(M_PI);
            for (int i = tid; i < nb * nr; i += NT) {
                const int b = i / nr, r = i - b * nr;
                T sr = T(0);
                if (r < C) {
                    for (int j = 0; j < GR; ++j) {
                        const uint32_t sv = s_slot[r * GR + j];
                        if ((int)(sv >> 16) != E) sr += s_ls[b * V + (int)(sv & 0xffffu)];
                    }
                } else {
                    const int l = r - C;
                    for (int v = 0; v < V; ++v)
                        if ((s_lm[v] >> l) & 1u) sr += s_ls[b * V + v];
                }
                const T xr = sr * kPi / T(2);
                const T sn = sin(xr);
                const T gr = (sn > T(0) ? T(1) : sn < T(0) ? T(-1) : T(0)) * cos(xr) * (kPi / T(2));
                const bool on = r >= C || !tape.logical_only;
                s_lg[i] = on ? gr : T(0);
                s_lt[i] = on ? (sn < T(0) ? -sn : sn) : T(0);
            }
            __syncthreads();
            for (int f = tid; f < nV; f += NT) {
                const int b = fdiv(f, dV), v = f - b * V;
                T d = T(0);
                for (int k = s_vptr[v]; k < s_vptr[v + 1]; ++k) d += s_lg[b * nr + s_vslot[k] / GR];
                const uint32_t m = s_lm[v];
                for (int l = 0; l < tape.nl; ++l)
                    if ((m >> l) & 1u) d += s_lg[b * nr + C + l];
                tape.gp[(size_t)(b0 + b) * g.os + g.o0 + v] = d;
            }
            const int wv = tid >> 6, lane = tid & 63;
            for (int b = wv; b < nb; b += NT / 64) {     // the codeword's loss, fixed order
                T t = T(0);
                for (int r = lane; r < nr; r += 64) t += s_lt[b * nr + r];
                t = fwd_wave_sum(t);
                if (lane == 0) tape.loss_b[(size_t)(b0 + b) * tape.ncomp + comp] = t;
            }
        }
    }
    GNND_PMARK(pf, 10);
    __syncthreads();                 // (the next tile restages the rows this one read)
    }
    GNND_PREPORT(pf, TAPE ? "fwd_tape" : "fwd", US, iters);
}

// HBM storage type of x / out.  GNND_BF16 keeps the inputs and outputs in bf16 (half the
// I/O bytes) while every LDS value, register and operation stays fp32: loads widen exactly
// (bf16 -> fp32 is a 16-bit shift), stores round to nearest even.
struct bf16_t {
    uint16_t u;
};
template <typename T> __device__ __forceinline__ T io_ld(T v) { return v; }
__device__ __forceinline__ float io_ld(bf16_t v) { return __uint_as_float((uint32_t)v.u << 16); }
template <typename TI, typename T> __device__ __forceinline__ TI io_st(T v) {
    if constexpr (std::is_same_v<TI, bf16_t>) {
        uint32_t u = __float_as_uint((float)v);
        u += 0x7fffu + ((u >> 16) & 1u);                 // round to nearest even (finite v)
        return bf16_t{(uint16_t)(u >> 16)};
    } else {
        return (TI)v;
    }
}

// sum of dp >= 1 consecutive LDS values in order; dp wave-uniform, so the trip counts and
// remainder tests are scalar branches and every lane runs unmasked
template <typename T> __device__ __forceinline__ T var_sum_uniform(const T* mp, int dp) {
    T s = mp[0];
    int k = 1;
    for (; k + 4 <= dp; k += 4) {
        const T a0 = mp[k], a1 = mp[k + 1], a2 = mp[k + 2], a3 = mp[k + 3];
        s += a0; s += a1; s += a2; s += a3;
    }
    if (k + 2 <= dp) {
        const T a0 = mp[k], a1 = mp[k + 1];
        s += a0; s += a1;
        k += 2;
    }
    if (k < dp) s += mp[k];
    return s;
}

// two variables' sums at once (wave-uniform degrees da, db): their common part in one loop of
// independent reads and adds (twice the LDS reads in flight of var_sum_uniform's chain), then
// each one's tail.  Every sum is still accumulated strictly in position order: the same bits.
template <typename T>
__device__ __forceinline__ void var_sum_uniform2(const T* ma, int da, const T* mb, int db, T& sa, T& sb) {
    T a = ma[0], b = mb[0];
    const int dm = da < db ? da : db;
    int k = 1;
    for (; k + 4 <= dm; k += 4) {
        const T a0 = ma[k], a1 = ma[k + 1], a2 = ma[k + 2], a3 = ma[k + 3];
        const T b0 = mb[k], b1 = mb[k + 1], b2 = mb[k + 2], b3 = mb[k + 3];
        a += a0; b += b0; a += a1; b += b1; a += a2; b += b2; a += a3; b += b3;
    }
    auto tail = [&](const T* mp, int dp, T s) {
        int j = k;
        for (; j + 4 <= dp; j += 4) {
            const T c0 = mp[j], c1 = mp[j + 1], c2 = mp[j + 2], c3 = mp[j + 3];
            s += c0; s += c1; s += c2; s += c3;
        }
        if (j + 2 <= dp) {
            const T c0 = mp[j], c1 = mp[j + 1];
            s += c0; s += c1;
            j += 2;
        }
        if (j < dp) s += mp[j];
        return s;
    };
    sa = tail(ma, da, a);
    sb = tail(mb, db, b);
}

// ---------------------------------------------------------------------------------------
// resident kernel (light models: CGNNI, QGNNI, CBP, QBP)
// ---------------------------------------------------------------------------------------
// Same two-phase iteration, but every lane keeps the c->v messages of its QMAX work
// items in registers for the whole decode, together with the items' slot entries
// (variable, edge) and check feature.  Step 1 therefore touches LDS only to read
// {S_v, x_v} and to publish m_e in VARIABLE-major order (E + 1 per codeword, the extra
// slot absorbs padding writes), and step 2 sums contiguous rows with no indirection.
#ifndef GNND_VAR_PRIO
#define GNND_VAR_PRIO 2            // s_setprio of the variable-sum step (0: off, A/B builds)
#endif
#ifndef GNND_RESIDENT_WAVES
#define GNND_RESIDENT_WAVES 4      // min waves per SIMD: 4 -> <= 128 VGPRs (tuning builds vary it)
#endif
// PADR: trailing slots per lane that may be padding (0: none, 1: only the last, R: any;
// gnnd_graph fills each check's lanes in order, so padding is always trailing)
template <int MODEL, typename T, int G, int R, int QMAX, int PADR, typename TI = T>
__global__ void __launch_bounds__(GNND_BLOCK, GNND_RESIDENT_WAVES)
decode_resident_kernel(GraphView g, const T* __restrict__ w, int nw, const TI* __restrict__ x,
                       TI* __restrict__ out, int64_t B, int iters, int CW, FastDiv dItem,
                       FastDiv dV, FastDiv dN, TapeView<T>) {
    using M = EdgeMath<MODEL, T>;
    constexpr bool BP = ModelTraits<MODEL>::bp;
    // fp32 GNN models keep x_v pre-scaled by log2(e) so the v->c pre-op is one FMA into
    // the base-2 tanh (tanh_half_base2); the readout re-reads the unscaled x_v from HBM.
    constexpr bool kBase2 = sizeof(T) == 4 && (MODEL == GNND_CGNNI || MODEL == GNND_QGNNI);
    // fp32 GNN and BP models run the check step on edge PAIRS (packed VALU, see below)
    constexpr bool kPairBP = sizeof(T) == 4 && (MODEL == GNND_CBP || MODEL == GNND_QBP ||
                                                MODEL == GNND_NBP || MODEL == GNND_V10 ||
                                                MODEL == GNND_V22);
    constexpr bool kPair = kBase2 || kPairBP;
    // plain fp32 BP (CBP, QBP): the check step multiplies magnitudes (bp_abstanh_f32x2)
#ifndef GNND_BP_LOGSUM
    constexpr bool kProd = kPairBP && !ModelTraits<MODEL>::wbp;
#else
    constexpr bool kProd = false;
#endif
    // ... in RATIO form (GNND_BP_RATIO, default): no per-edge tanh division, leave-one-out
    // reciprocal or atanh quotient; messages and x in base-2 units (bp_ratio below)
    constexpr bool kRatio = kProd && GNND_BP_RATIO;
    // fp64 plain BP (the quantum scripts' dtype) in the same ratio form, natural units, with the
    // cancellation-free expm1: n = -expm1(-z), d = 2 + expm1(-z) (bp_ratio64 below)
    constexpr bool kRatio64 = sizeof(T) == 8 && (MODEL == GNND_CBP || MODEL == GNND_QBP) && GNND_BP_RATIO;
    // x and messages held in base-2 units (x' = x log2 e): the GNN models' tanh pre-op and the
    // ratio-form BP check step start from 2^(-a')
    constexpr bool kB2 = kBase2 || kRatio;
    // T layout (paired GNN and plain-BP models): LDS keeps ONE value per variable,
    // T_v = S_v + x_v (base-2 scaled for the GNN models: messages m' = m log2 e, so
    // T'_v = S'_v + x'_v), refreshed by the variable-sum step, plus x_v itself for that
    // refresh; the check step's v->c argument a_e = T_v - m_e is one packed subtract per
    // edge pair.  The GNN check step then works in the sigmoid domain: r_e = 1/(1 + 2^a'_e)
    // = (1 - tanh(a_e/2))/2, check sum R = sum_slots r (padding slots r = 1/2, i.e. t = 0),
    // leave-one-out u_e = (G R_slots - 1) - 2 (R - r_e) with the affine map folded into the
    // message MLP's first layer and log2 e into its second (Mlp10Pair::load).  Weighted BP
    // keeps {S_v, x_v} (its per-edge weights act on S and x separately).
    constexpr bool WBP0 = ModelTraits<MODEL>::wbp;
    constexpr bool kTX = kPair && !WBP0;
    constexpr int kLogG = G == 1 ? 0 : G == 2 ? 1 : G == 4 ? 2 : G == 8 ? 3 : G == 16 ? 4 : G == 32 ? 5 : 6;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int V = g.V, C = g.C, E = g.E, N = g.N;
    const int E1 = g.P1;                  // message positions per codeword (layout stride)
    const int spare = g.spare;            // position padding slots and idle items write
    // T layout: codeword b's T_v at b * TS + tpos(v) (tpos in the slot tables' low halves and
    // vlay .y's high half; gnnd_graph.hip place_t_rows); {S_v, x_v} rows stay b * V + v
    const int TS = kTX ? g.ts : V;
    const int tid = threadIdx.x;

    T* s_w = (T*)smem;
    size_t off = ((size_t)nw * sizeof(T) + 15) & ~(size_t)15;
    // fp32 GNN models: the message MLP's piecewise-linear table (pwl_build) after the weights
    float* s_pwl = (float*)(smem + off);
    if constexpr (kBase2 && GNND_MLP_PWL) off += kPwlBytes;
    uint2* s_vord = (uint2*)(smem + off);
    off += ((size_t)V * 8 + 15) & ~(size_t)15;
    T* s_m = (T*)(smem + off);                             // [CW][E+1] messages, var-major
    SumX<T>* s_sx = (SumX<T>*)(s_m + (((size_t)CW * E1 + 1) & ~(size_t)1));  // [CW][V]
    T* s_xc = (T*)(s_sx + (size_t)CW * V);                 // [CW][C]  check-row features
    // kTX: [CW][V] T_v in place of {S_v, x_v}; x_v lives in the message layout
    // (gnnd_graph::rlayx: the last position of each variable's run)
    float* s_t = (float*)s_sx;
    if constexpr (kTX) s_xc = (T*)(s_t + (size_t)CW * TS);

    for (int i = tid; i < nw; i += GNND_BLOCK) s_w[i] = w[i];
    for (int i = tid; i < V; i += GNND_BLOCK) s_vord[i] = g.vlay[i];
    const int64_t b0 = (int64_t)blockIdx.x * CW;
    const int nb = (int)((B - b0) < CW ? (B - b0) : CW);
    const TI* xg = x + b0 * N;
    for (int i = tid; i < nb * N; i += GNND_BLOCK) {
        int b = fdiv(i, dN), n = i - b * N;
        if (n < V) {
            if constexpr (!kTX) {                       // (T layout: below, in var_ord order)
                const T xv = io_ld(xg[i]);
                s_sx[b * V + n] = SumX<T>{T(0), kB2 ? xv * T(kLog2e) : xv};
            }
        } else {
            s_xc[b * C + n - V] = io_ld(xg[i]);
        }
    }
    // padded layouts: the positions past a variable's degree are read by the variable sums
    // and never written, so they must hold 0 (s + 0 == s)
    if (kTX || g.vgroup > 1)
        for (int i = tid; i < CW * E1; i += GNND_BLOCK) s_m[i] = T(0);
    __syncthreads();
    if constexpr (kTX) {
        // T_v = 0 + x_v at its T row, and x_v into the last position of its message run (after
        // the padded messages: S + 0 + x_v)
        for (int i = tid; i < nb * V; i += GNND_BLOCK) {
            const int b = fdiv(i, dV), j = i - b * V;
            const uint2 o = s_vord[j];
            const int v = GNND_DIDX((int)(o.x & 0xffffu), V, GNND_DBG_VAR);
            const T xv = io_ld(xg[b * N + v]);
            const T xs = kB2 ? xv * T(kLog2e) : xv;
            s_t[b * TS + GNND_DIDX((int)(o.y >> 16), TS, GNND_DBG_VAR)] = xs;
            s_m[b * E1 + GNND_DIDX((int)(o.y & 0xffffu) + (int)(o.x >> 16) - 1, E1, GNND_DBG_LDS_POS)] = xs;
        }
        __syncthreads();
    }

    Mlp10F32 mlp_msg;   // scalar-path form (unused: fp32 GNN models run the paired step)
    if constexpr (sizeof(T) == 4 && !kPair && (MODEL == GNND_CGNNI || MODEL == GNND_QGNNI))
        mlp_msg.load((const float*)s_w + kMlp10Msg, (float)g.max_dc);
    // weighted BP: per-edge tables read through the cache; LDS carries the messages the
    // variable sums need (NBP: already weighted by the next layer's W, or the readout W)
    constexpr bool WBP = ModelTraits<MODEL>::wbp;
    const WbpW<MODEL, T> ww{w, E, iters};
    T alpha = T(0);
    if constexpr (WBP) alpha = ww.alpha();

    // ---- per-lane resident state.  Item f = tid + q*256 -> (check c, codeword b, lane g)
    // with g fastest and the CODEWORD next: a wave's 8 check groups are 8 codewords of one
    // check, so their {S_v, x_v} reads and message writes land on different LDS banks
    // (codeword strides V and E+1 are odd).  dItem divides by CW here.  Items of codewords
    // b >= nb (partial last tile) or checks c >= C compute on clamped copies and, like
    // padding slots, store into the spare slot E of their codeword: the item loop is
    // straight-line code.
    uint32_t ve[QMAX][R];      // v | e << 16 (padding and idle items: e = E)
    T m[QMAX][R];
    T sc[QMAX];
    int cb[QMAX];              // codeword of the item
    // fp32 GNN models run the check step on item PAIRS (2j, 2j+1): slot r of both items
    // rides the two halves of packed VALU ops (v_pk_add/fma_f32), so every non-
    // transcendental op covers two edges.  An odd last item pairs with itself (identical
    // arithmetic in every position: batch-independent bits).  m2 holds the pairs' messages.
    constexpr int QP = kPair ? QMAX / 2 : 1;              // item pairs
    constexpr bool kSolo = kPair && (QMAX & 1);           // odd last item: slot pairs
    constexpr int RP = (R + 1) / 2;
    f32x2 m2[QP][R];           // m2[j][r] = {m of item 2j, m of item 2j+1} at slot r
    f32x2 ms[RP];              // solo item: {slot 2i, slot 2i+1} (odd R: last pairs itself)
    f32x2 sc2[QP];
    Mlp10Pair mlp2;
    if constexpr (kBase2)      // input v = R - r_e: u = (G R_slots - 1) - 2 v; output x log2 e
        mlp2.load((const float*)s_w + kMlp10Msg, (float)(G * R), -2.f, (float)(G * R - 1), kLog2e);
    // the same function as a piecewise-linear table (pwl_stage: uniform ok, K and scales from
    // the prepared weights, the graph's v-domain entries in LDS)
    Pwl pwl{0, 1, 0.f, 0.f, 1.f};
    if constexpr (kBase2 && GNND_MLP_PWL) {
        pwl = pwl_stage((const float*)w, s_pwl, (float)(G * R), -2.f, (float)(G * R - 1), kLog2e, tid);
        __syncthreads();
    }
    // The per-lane state set-up and the T iterations, as a force-inlined generic lambda over NU =
    // the message-MLP units the check step evaluates (Mlp10Pair::eval_n<NU>): the fp32 GNN
    // models instantiate it per live-unit count and pick one by a wave-uniform switch below, so
    // the hot straight-line code carries no branch on the count.  The set-up is inside because a
    // switch between it and the loops made the register allocator spill ~40 of its values across
    // the switch (188 bytes of scratch per lane on the headline plan).  Every other model has the
    // one NU = 10 body.  (The body keeps the kernel's indentation.)
    auto run_iters = [&](auto nuc) __attribute__((always_inline)) {
    constexpr int NU = decltype(nuc)::value;
#pragma unroll
    for (int q = 0; q < QMAX; ++q) {
        const int f = tid + q * GNND_BLOCK;
        const int gi = f >> kLogG;
        const int c = fdiv(gi, dItem);
        const int b = gi - c * CW;
        const bool act = c < C && b < nb;
        const int cc = c < C ? c : C - 1, bb = b < nb ? b : nb - 1;
        const int rem = cc * G + (f & (G - 1));
        sc[q] = s_xc[bb * C + cc];
        // ratio-form QBP: the syndrome's sign factor cos(pi (1 - s_c) / 2) of quantum/BP.py:112
        // (+-1 for s_c = +-1) multiplies the check's numerator product
        if constexpr (kRatio && MODEL == GNND_QBP) sc[q] = cosf(3.14159265358979f * 0.5f * (1.f - (float)sc[q]));
        if constexpr (kRatio64 && MODEL == GNND_QBP) sc[q] = cos_pi((T(1) - sc[q]) / T(2));
        cb[q] = bb;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const uint32_t sv = g.slot_ve[rem * R + r];
            ve[q][r] = act ? sv : ((sv & 0xffffu) | ((uint32_t)spare << 16));
            m[q][r] = T(0);
        }
    }
    if constexpr (kPair) {
#pragma unroll
        for (int j = 0; j < QP; ++j) {
            sc2[j] = f32x2{(float)sc[2 * j], (float)sc[2 * j + 1]};
#pragma unroll
            for (int r = 0; r < R; ++r) m2[j][r] = f32x2{0.f, 0.f};
        }
#pragma unroll
        for (int i = 0; i < RP; ++i) ms[i] = f32x2{0.f, 0.f};
    }

    // variable-sum step mapping (see below): lane-invariant when CW divides the block
    const bool vfixed = GNND_BLOCK % CW == 0;
    const int vb = tid % CW, vi0 = tid / CW, vstep = GNND_BLOCK / CW;
    const bool vact = vb < nb;
    const int vmbase = vb * E1, vsbase = vb * V, vtbase = vb * TS;
    // a wave covers 64 / CW consecutive var_ord entries per step: uniform when the layout
    // pads each such group to one degree (weighted BP keeps the identity layout: its
    // per-edge weight tables are indexed by edge id)
    const bool vuni = !WBP && vfixed && g.vgroup * CW >= 64;
#ifndef GNND_VAR_CACHE
#define GNND_VAR_CACHE 1          // cache the first var_ord entries (r05d A/B: 0.4637 -> 0.4595 ms)
#endif
#ifndef GNND_VAR_CACHE_N
#define GNND_VAR_CACHE_N 2         // cached entries per lane (4 spilled the 128-VGPR kernel)
#endif
    // the uniform variable step's first kVC var_ord entries of this lane (loop-invariant over the
    // iterations): message-run base, T row position and the wave-uniform padded degree, so an
    // iteration's variable sums start with the message reads instead of an LDS round trip for the
    // entry and its decode
#ifndef GNND_VAR_CACHE_NL
#define GNND_VAR_CACHE_NL 5        // ... for fp32 plans with <= 64 item-state VGPRs (Q (2R + 2)):
#endif                             // r05n A/B LDPC CGNNI +1.1 %, toric QGNNI +1.4 %, QBP +2.3 %
    constexpr bool kLightRegs = sizeof(T) == 4 && QMAX * (2 * R + 2) <= 64;
    constexpr int kVC = GNND_VAR_CACHE ? (kLightRegs ? GNND_VAR_CACHE_NL : GNND_VAR_CACHE_N) : 0;
    // one VGPR per entry: message-run position (vmbase included, < 2^16: the tile's LDS message
    // block) | T row position << 16; the padded degree in an SGPR
    uint32_t vc_mt[kVC > 0 ? kVC : 1];
    int vc_dp[kVC > 0 ? kVC : 1];
    if constexpr (kVC > 0) {
#pragma unroll
        for (int k = 0; k < kVC; ++k) {
            const int i = vi0 + k * vstep;
            const uint2 o = s_vord[i < V ? i : V - 1];
            vc_mt[k] = (uint32_t)(vmbase + (int)(o.y & 0xffffu)) | (o.y & 0xffff0000u);
            vc_dp[k] = __builtin_amdgcn_readfirstlane((int)(o.x >> 16));
        }
    }

    for (int it = 0; it < iters; ++it) {
        if constexpr (kPair) {
            // check-node pre-op of two edges.  GNN: tanh(a/2) in base 2, 1 - 2 / (1 + 2^a'),
            // a' = (S - m) log2e + x'.  BP: {log2|tanh(a/2)|, [a < 0]}, a = (S - m) + x.
            // {S_v, x_v} arrive as one ds_read_b64 per edge; the leave-one-out and the
            // prior are added by scalar ops (packing them would need moves into {S_a, S_b}
            // / {x_a, x_b} pairs), the rest of the chain is packed
            auto pre2v = [&](SumX<T> pa, SumX<T> pb, uint32_t sa, uint32_t sb, f32x2 mprev,
                             int ra, int rb, f32x2& cc) {
                f32x2 t;
                if constexpr (kBase2) {
                    const f32x2 a = {__builtin_fmaf(pa.s - mprev.x, kLog2e, pa.x),
                                     __builtin_fmaf(pb.s - mprev.y, kLog2e, pb.x)};
                    f32x2 e = {__builtin_amdgcn_exp2f(a.x), __builtin_amdgcn_exp2f(a.y)};
                    e = e + f32x2{1.f, 1.f};
                    const f32x2 rc = {__builtin_amdgcn_rcpf(e.x), __builtin_amdgcn_rcpf(e.y)};
                    t = __builtin_elementwise_fma(rc, f32x2{-2.f, -2.f}, f32x2{1.f, 1.f});
                    cc = f32x2{0.f, 0.f};
                } else if constexpr (WBP) {
                    // weighted BP: the edge's iteration weights (identity layout: position =
                    // reference edge id) read through the cache
                    const int ea = (int)(sa >> 16), eb = (int)(sb >> 16);
                    const int xa = ea < E ? ea : 0, xb = eb < E ? eb : 0;
                    f32x2 a;
                    if constexpr (MODEL == GNND_NBP || MODEL == GNND_V22)
                        a = f32x2{(pa.s - mprev.x * ww.msg(it, xa)) + pa.x * ww.prior(it, xa),
                                  (pb.s - mprev.y * ww.msg(it, xb)) + pb.x * ww.prior(it, xb)};
                    else
                        a = f32x2{((pa.s - mprev.x) + pa.x) * ww.chk(it, xa),
                                  ((pb.s - mprev.y) + pb.x) * ww.chk(it, xb)};
                    t = wbp_L2(a, cc);
                } else {
                    const f32x2 a = {(pa.s - mprev.x) + pa.x, (pb.s - mprev.y) + pb.x};
                    cc = f32x2{a.x < 0.f ? 1.f : 0.f, a.y < 0.f ? 1.f : 0.f};
                    t = bp_log2tanh_f32x2(a, MODEL == GNND_QBP ? 1e-20f : 1e-7f);
                }
                if constexpr (PADR > 0) {   // padding slot: position == spare
                    if (ra >= R - PADR && sa >= ((uint32_t)spare << 16)) { t.x = 0.f; cc.x = 0.f; }
                    if (rb >= R - PADR && sb >= ((uint32_t)spare << 16)) { t.y = 0.f; cc.y = 0.f; }
                }
                return t;
            };
            // T layout: a = T - m for both edges in one packed subtract.  GNN: r = 1/(1 + 2^a')
            // (padding slots r = 1/2); BP: {log2|tanh(a/2)|, [a < 0]} (padding 0)
            auto pre2t = [&](f32x2 tt, uint32_t sa, uint32_t sb, f32x2 mprev, int ra, int rb,
                             f32x2& cc) {
                const f32x2 a = tt - mprev;
                f32x2 t;
                float pad = 0.f;
                if constexpr (kBase2) {
                    f32x2 e = {__builtin_amdgcn_exp2f(a.x), __builtin_amdgcn_exp2f(a.y)};
                    e = e + f32x2{1.f, 1.f};
                    t = f32x2{__builtin_amdgcn_rcpf(e.x), __builtin_amdgcn_rcpf(e.y)};
                    cc = f32x2{0.f, 0.f};
                    pad = 0.5f;
                } else if constexpr (kProd) {
                    cc = f32x2{a.x < 0.f ? 1.f : 0.f, a.y < 0.f ? 1.f : 0.f};
                    t = bp_abstanh_f32x2(a, MODEL == GNND_QBP ? 1e-20f : 1e-7f);
                    pad = 1.f;
                } else {
                    cc = f32x2{a.x < 0.f ? 1.f : 0.f, a.y < 0.f ? 1.f : 0.f};
                    t = bp_log2tanh_f32x2(a, MODEL == GNND_QBP ? 1e-20f : 1e-7f);
                }
                if constexpr (PADR > 0) {   // padding slot: position == spare
                    if (ra >= R - PADR && sa >= ((uint32_t)spare << 16)) { t.x = pad; cc.x = 0.f; }
                    if (rb >= R - PADR && sb >= ((uint32_t)spare << 16)) { t.y = pad; cc.y = 0.f; }
                }
                return t;
            };
            auto pre2 = [&](uint32_t sa, uint32_t sb, int ca, int cbb, f32x2 mprev, int ra, int rb,
                            f32x2& cc) {
                if constexpr (kTX)
                    return pre2t(f32x2{s_t[ca * TS + (int)(sa & 0xffffu)], s_t[cbb * TS + (int)(sb & 0xffffu)]},
                                 sa, sb, mprev, ra, rb, cc);
                else
                    return pre2v(s_sx[ca * V + (int)(sa & 0xffffu)], s_sx[cbb * V + (int)(sb & 0xffffu)],
                                 sa, sb, mprev, ra, rb, cc);
            };
            // per-slot operand of the paired pre-op: T_v of both edges (T layout) or the two
            // {S_v, x_v}
            using PX = std::conditional_t<kTX, f32x2, SumX<T>[2]>;
            // {S_v, x_v} of an item pair's slots (issued one pair ahead: LDS reads cannot move
            // above the previous pair's message writes by themselves, the compiler cannot
            // tell the two arrays apart)
            auto load_pair = [&](int j, PX (&px)[R]) {
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    // (T layout: row stride TS, the slot's low half is tpos(v))
                    const int ia = cb[2 * j] * TS + GNND_DIDX((int)(ve[2 * j][r] & 0xffffu), TS, GNND_DBG_VAR);
                    const int ib = cb[2 * j + 1] * TS + GNND_DIDX((int)(ve[2 * j + 1][r] & 0xffffu), TS, GNND_DBG_VAR);
                    if constexpr (kTX) {
#ifdef GNND_DIAG_TV_LINEAR
                        // diagnostic build only (wrong results): lane-linear, conflict-free T reads
                        (void)ia; (void)ib;
                        px[r] = f32x2{s_t[(int)(threadIdx.x & 63)], s_t[64 + (int)(threadIdx.x & 63)]};
#else
                        px[r] = f32x2{s_t[ia], s_t[ib]};
#endif
                    } else {
                        px[r][0] = s_sx[ia];
                        px[r][1] = s_sx[ib];
                    }
                }
            };
            // c->v update of two edges from the leave-one-out sums u (and sign counts n)
            auto post2 = [&](f32x2 u, f32x2 n, f32x2 scp, f32x2 mprev) {
                if constexpr (kBase2) {
#ifdef GNND_MLP_PWL_ONLY
                    const f32x2 y = pwl_eval2(s_pwl, pwl, u);          // (A/B: no unit fallback)
#else
                    const f32x2 y = pwl.ok ? pwl_eval2(s_pwl, pwl, u) : mlp2.template eval_n<NU>(u);
#endif
                    if constexpr (MODEL == GNND_QGNNI) return __builtin_elementwise_fma(y, scp, mprev);
                    else return y + mprev;
                } else if constexpr (WBP) {
                    return __builtin_elementwise_fma(mprev, f32x2{(float)alpha, (float)alpha},
                                                     wbp_out2(u, n, scp));
                } else if constexpr (MODEL == GNND_QBP) {
                    const f32x2 nq = __builtin_elementwise_fma(f32x2{1.f, 1.f} - scp, f32x2{0.5f, 0.5f}, n);
                    if constexpr (kProd) return bp_msg_prod_f32x2<true>(u, nq, cst<float>(1 - 1e-12));
                    else return bp_msg_f32x2<true>(u, nq, cst<float>(1 - 1e-12));
                } else {
                    if constexpr (kProd) return bp_msg_prod_f32x2<false>(u, n, cst<float>(1 - 1e-7));
                    else return bp_msg_f32x2<false>(u, n, cst<float>(1 - 1e-7));
                }
            };
            // NBP publishes m already weighted by the next layer's W (or the readout W) for
            // the variable sums (neural_BP.py:248); 1 otherwise (x 1.0 is exact)
            auto wnext = [&](uint32_t sv) -> float {
                if constexpr (MODEL == GNND_NBP) {
                    const int e = (int)(sv >> 16), ec = e < E ? e : 0;
                    return it + 1 < iters ? ww.msg(it + 1, ec) : ww.out_w(ec);
                } else {
                    return 1.f;
                }
            };
            // ratio-form fp32 BP (kRatio): per slot the signed numerator n = sign(a)(1 - E) and
            // the denominator d = 1 + E of t = tanh(a/2) (E = 2^-z, z = |a'| clamped to
            // [kBpZmin, kBpZmax]); padding slots n = d = 1
            auto nd2 = [&](f32x2 tt, uint32_t sa, uint32_t sb, f32x2 mprev, int ra, int rb, f32x2& n,
                           f32x2& d) {
                const f32x2 a = tt - mprev;
                const f32x2 e = {__builtin_amdgcn_exp2f(-__builtin_amdgcn_fmed3f(fabsf(a.x), kBpZmin, kBpZmax)),
                                 __builtin_amdgcn_exp2f(-__builtin_amdgcn_fmed3f(fabsf(a.y), kBpZmin, kBpZmax))};
                n = f32x2{1.f, 1.f} - e;
                d = f32x2{1.f, 1.f} + e;
                n = f32x2{__builtin_copysignf(n.x, a.x), __builtin_copysignf(n.y, a.y)};
                if constexpr (PADR > 0) {
                    if (ra >= R - PADR && sa >= ((uint32_t)spare << 16)) { n.x = 1.f; d.x = 1.f; }
                    if (rb >= R - PADR && sb >= ((uint32_t)spare << 16)) { n.y = 1.f; d.y = 1.f; }
                }
            };
            // item pair (2j, 2j + 1)
            auto pair_step = [&](auto jc, const PX (&px)[R]) {
                constexpr int j = decltype(jc)::value;
                const int qa = 2 * j, qb = 2 * j + 1;
                if constexpr (kRatio) {
                    // the check's products N = sc prod n, D = prod d (G-lane product butterflies)
                    // and per edge m' = log2|(D n_e + N d_e) / (D n_e - N d_e)| (bp_ratio_msg)
                    f32x2 nv[R], dv[R], Np, Dp;
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        nd2(px[r], ve[qa][r], ve[qb][r], m2[j][r], r, r, nv[r], dv[r]);
                        Np = r == 0 ? nv[0] : Np * nv[r];
                        Dp = r == 0 ? dv[0] : Dp * dv[r];
                    }
                    Np = f32x2{group_prod_c<G>(Np.x), group_prod_c<G>(Np.y)};
                    Dp = f32x2{group_prod_c<G>(Dp.x), group_prod_c<G>(Dp.y)};
                    if constexpr (MODEL == GNND_QBP) Np = Np * sc2[j];
                    T* mra = s_m + cb[qa] * E1;
                    T* mrb = s_m + cb[qb] * E1;
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        m2[j][r] = bp_ratio_msg(Np, Dp, nv[r], dv[r]);
                        mra[GNND_DIDX((int)(ve[qa][r] >> 16), E1, GNND_DBG_LDS_POS)] = m2[j][r].x;
                        mrb[GNND_DIDX((int)(ve[qb][r] >> 16), E1, GNND_DBG_LDS_POS)] = m2[j][r].y;
                    }
                    return;
                }
                f32x2 tv[R], cv[R], tsum, csum;
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    if constexpr (kTX)
                        tv[r] = pre2t(px[r], ve[qa][r], ve[qb][r], m2[j][r], r, r, cv[r]);
                    else
                        tv[r] = pre2v(px[r][0], px[r][1], ve[qa][r], ve[qb][r], m2[j][r], r, r, cv[r]);
                    if constexpr (kProd) tsum = r == 0 ? tv[0] : tsum * tv[r];
                    else tsum = r == 0 ? tv[0] : tsum + tv[r];
                    if constexpr (kPairBP) csum = r == 0 ? cv[0] : csum + cv[r];
                }
                f32x2 Sc;
                if constexpr (kProd) Sc = f32x2{group_prod_c<G>(tsum.x), group_prod_c<G>(tsum.y)};
                else Sc = f32x2{group_sum_c<G>(tsum.x), group_sum_c<G>(tsum.y)};
                f32x2 Sc2 = {0.f, 0.f};
                if constexpr (kPairBP) Sc2 = f32x2{group_sum_c<G>(csum.x), group_sum_c<G>(csum.y)};
                T* mba = s_m + cb[qa] * E1;
                T* mbb = s_m + cb[qb] * E1;
#ifdef GNND_MLP_BATCH
                if constexpr (kBase2) {
                    // the pair's R message MLPs unit-major (Mlp10Pair::batch)
                    f32x2 u[R], y[R];
#pragma unroll
                    for (int r = 0; r < R; ++r) u[r] = Sc - tv[r];
                    mlp2.template batch<R>(u, y);
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        if constexpr (MODEL == GNND_QGNNI) m2[j][r] = __builtin_elementwise_fma(y[r], sc2[j], m2[j][r]);
                        else m2[j][r] = y[r] + m2[j][r];
                        mba[GNND_DIDX((int)(ve[qa][r] >> 16), E1, GNND_DBG_LDS_POS)] = m2[j][r].x;
                        mbb[GNND_DIDX((int)(ve[qb][r] >> 16), E1, GNND_DBG_LDS_POS)] = m2[j][r].y;
                    }
                    return;
                }
#endif
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    m2[j][r] = post2(kProd ? Sc * rcp2(tv[r]) : Sc - tv[r], Sc2 - cv[r], sc2[j], m2[j][r]);
#ifdef GNND_DIAG_MSG_LINEAR
                    // diagnostic build only (wrong results): lane-linear, conflict-free message writes
                    (void)mba; (void)mbb;
                    s_m[(int)(threadIdx.x & 63)] = m2[j][r].x * wnext(ve[qa][r]);
                    s_m[64 + (int)(threadIdx.x & 63)] = m2[j][r].y * wnext(ve[qb][r]);
#else
                    mba[GNND_DIDX((int)(ve[qa][r] >> 16), E1, GNND_DBG_LDS_POS)] = m2[j][r].x * wnext(ve[qa][r]);
                    mbb[GNND_DIDX((int)(ve[qb][r] >> 16), E1, GNND_DBG_LDS_POS)] = m2[j][r].y * wnext(ve[qb][r]);
#endif
                }
            };
            // one item with its slots in pairs (the same per-edge arithmetic as pair_step:
            // bitwise-identical messages)
            auto solo_step = [&](auto qc, f32x2* msp) {
                constexpr int q = decltype(qc)::value;
                if constexpr (kRatio) {
                    f32x2 nv[RP], dv[RP];
                    float Np = 1.f, Dp = 1.f;
#pragma unroll
                    for (int i = 0; i < RP; ++i) {
                        const int r0 = 2 * i, r1 = 2 * i + 1 < R ? 2 * i + 1 : 2 * i;
                        const f32x2 tt = {s_t[cb[q] * TS + (int)(ve[q][r0] & 0xffffu)],
                                          s_t[cb[q] * TS + (int)(ve[q][r1] & 0xffffu)]};
                        nd2(tt, ve[q][r0], ve[q][r1], msp[i], r0, r1, nv[i], dv[i]);
                        Np = i == 0 ? nv[0].x : Np * nv[i].x;
                        Dp = i == 0 ? dv[0].x : Dp * dv[i].x;
                        if (2 * i + 1 < R) {
                            Np = Np * nv[i].y;
                            Dp = Dp * dv[i].y;
                        }
                    }
                    Np = group_prod_c<G>(Np);
                    Dp = group_prod_c<G>(Dp);
                    if constexpr (MODEL == GNND_QBP) Np = Np * (float)sc[q];
                    T* mb = s_m + cb[q] * E1;
#pragma unroll
                    for (int i = 0; i < RP; ++i) {
                        const int r0 = 2 * i, r1 = 2 * i + 1 < R ? 2 * i + 1 : 2 * i;
                        msp[i] = bp_ratio_msg(f32x2{Np, Np}, f32x2{Dp, Dp}, nv[i], dv[i]);
                        mb[GNND_DIDX((int)(ve[q][r0] >> 16), E1, GNND_DBG_LDS_POS)] = msp[i].x;
                        if (r1 != r0) mb[GNND_DIDX((int)(ve[q][r1] >> 16), E1, GNND_DBG_LDS_POS)] = msp[i].y;
                    }
                    return;
                }
                f32x2 tv[RP], cv[RP];
                float tsum = 0.f, csum = 0.f;
#pragma unroll
                for (int i = 0; i < RP; ++i) {
                    const int r0 = 2 * i, r1 = 2 * i + 1 < R ? 2 * i + 1 : 2 * i;
                    tv[i] = pre2(ve[q][r0], ve[q][r1], cb[q], cb[q], msp[i], r0, r1, cv[i]);
                    if constexpr (kProd) {
                        tsum = i == 0 ? tv[0].x : tsum * tv[i].x;
                        if (2 * i + 1 < R) tsum = tsum * tv[i].y;
                    } else {
                        tsum = i == 0 ? tv[0].x : tsum + tv[i].x;
                        if (2 * i + 1 < R) tsum = tsum + tv[i].y;
                    }
                    if constexpr (kPairBP) {
                        csum = i == 0 ? cv[0].x : csum + cv[i].x;
                        if (2 * i + 1 < R) csum = csum + cv[i].y;
                    }
                }
                const float Sc = kProd ? group_prod_c<G>(tsum) : group_sum_c<G>(tsum);
                float Sc2 = 0.f;
                if constexpr (kPairBP) Sc2 = group_sum_c<G>(csum);
                T* mb = s_m + cb[q] * E1;
#pragma unroll
                for (int i = 0; i < RP; ++i) {
                    const int r0 = 2 * i, r1 = 2 * i + 1 < R ? 2 * i + 1 : 2 * i;
                    msp[i] = post2(kProd ? f32x2{Sc, Sc} * rcp2(tv[i]) : f32x2{Sc, Sc} - tv[i],
                                  f32x2{Sc2, Sc2} - cv[i],
                                  f32x2{(float)sc[q], (float)sc[q]}, msp[i]);
                    mb[GNND_DIDX((int)(ve[q][r0] >> 16), E1, GNND_DBG_LDS_POS)] = msp[i].x * wnext(ve[q][r0]);
                    if (r1 != r0) mb[GNND_DIDX((int)(ve[q][r1] >> 16), E1, GNND_DBG_LDS_POS)] = msp[i].y * wnext(ve[q][r1]);
                }
            };
            // waves whose last work item is idle (tile rounds not filled: LDPC 1 296 items
            // in 6 rounds) run the last item pair as the first item alone
            const bool last_item_live = (int)(__builtin_amdgcn_readfirstlane(tid) & ~63) +
                                        (QMAX - 1) * GNND_BLOCK < C * G * CW;
            // one-pair-ahead reads: measured +1.2 % on BCH CGNNI (4 item pairs per lane),
            // -1.3 % on LDPC CGNNI (3 pairs) and -0.7 % on C/BP (profiles/r01/experiments)
#ifndef GNND_NO_PAIR_PREFETCH
            constexpr bool kAhead = kBase2 && QP >= 4;
#else
            constexpr bool kAhead = false;
#endif
            PX pxa[R], pxb[R];                  // current / next pair's operands
            if constexpr (kAhead) load_pair(0, pxa);
            static_for<QP>([&](auto jc) {
                constexpr int j = decltype(jc)::value;
                PX (&cur)[R] = (j & 1) ? pxb : pxa;
                PX (&nxt)[R] = (j & 1) ? pxa : pxb;
                if constexpr (kAhead) {
                    if constexpr (j + 1 < QP) load_pair(j + 1, nxt);
                } else {
                    load_pair(j, cur);
                }
                if constexpr (!kSolo && j == QP - 1) {
                    if (!last_item_live) {
                        f32x2 tmp[RP];
#pragma unroll
                        for (int i = 0; i < RP; ++i) {
                            const int r1 = 2 * i + 1 < R ? 2 * i + 1 : 2 * i;
                            tmp[i] = f32x2{m2[j][2 * i].x, m2[j][r1].x};
                        }
                        solo_step(std::integral_constant<int, 2 * j>{}, tmp);
#pragma unroll
                        for (int i = 0; i < RP; ++i) {
                            m2[j][2 * i].x = tmp[i].x;
                            if (2 * i + 1 < R) m2[j][2 * i + 1].x = tmp[i].y;
                        }
                        return;
                    }
                }
                pair_step(jc, cur);
            });
            if constexpr (kSolo) solo_step(std::integral_constant<int, QMAX - 1>{}, ms);
        } else
#pragma unroll
        for (int q = 0; q < QMAX; ++q) {
            T tv[R], cf[R];
            T tsum = T(0), csum = T(0);
            GNND_DCHECK(cb[q] < CW, GNND_DBG_GRID);
            const SumX<T>* sxb = s_sx + cb[q] * V;
            if constexpr (kRatio64) {
                // fp64 ratio form (bp_ratio64): t_e = n_e / d_e, the check's N = s prod n,
                // D = prod d, m_e = log|D n_e + N d_e| - log|D n_e - N d_e|
                T nv[R], dv[R], Np = T(1), Dp = T(1);
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const uint32_t sv = ve[q][r];
                    const bool valid = !(PADR > 0 && r >= R - PADR) || (int)(sv >> 16) != spare;
                    const SumX<T> p = sxb[sv & 0xffffu];
                    const T a = (p.s - m[q][r]) + p.x;
                    const T z = fmin(fmax(fabs(a), MODEL == GNND_QBP ? 2e-20 : 2e-7), 10.0);
                    const T em = expm1_f64(-z);
                    nv[r] = valid ? (a < T(0) ? em : -em) : T(1);
                    dv[r] = valid ? T(2) + em : T(1);
                    Np = r == 0 ? nv[0] : Np * nv[r];
                    Dp = r == 0 ? dv[0] : Dp * dv[r];
                }
                Np = group_prod_c<G>(Np);
                Dp = group_prod_c<G>(Dp);
                if constexpr (MODEL == GNND_QBP) Np = Np * sc[q];
                T* mb = s_m + cb[q] * E1;
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const T A = Dp * nv[r], Bv = Np * dv[r];
                    m[q][r] = g_log(fabs(A + Bv)) - g_log(fabs(A - Bv));
                    mb[(int)(ve[q][r] >> 16)] = m[q][r];
                }
                continue;
            }
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const uint32_t sv = ve[q][r];
                const bool valid = !(PADR > 0 && r >= R - PADR) || (int)(sv >> 16) != spare;
                const SumX<T> p = sxb[sv & 0xffffu];
                T cc = T(0), t;
                if constexpr (kBase2) t = tanh_half_base2(__builtin_fmaf(p.s - m[q][r], kLog2e, p.x));
                else if constexpr (WBP) {
                    const int e = (int)(sv >> 16), ec = e < E ? e : 0;
                    T a;
                    if constexpr (MODEL == GNND_NBP || MODEL == GNND_V22)
                        a = (p.s - m[q][r] * ww.msg(it, ec)) + p.x * ww.prior(it, ec);
                    else
                        a = ((p.s - m[q][r]) + p.x) * ww.chk(it, ec);
                    t = wbp_L(a, cc);
                }
                else t = M::pre(p.s - m[q][r], p.x, w, cc);
                tv[r] = valid ? t : T(0);
                cf[r] = valid ? cc : T(0);
                // the first term starts the sum (0 + t == t: t is never -0)
                tsum = r == 0 ? tv[0] : tsum + tv[r];
                if constexpr (BP) csum = r == 0 ? cf[0] : csum + cf[r];
            }
            const T Sc = group_sum_c<G>(tsum);
            T Sc2 = T(0);
            if constexpr (BP) Sc2 = group_sum_c<G>(csum);
            T* mb = s_m + cb[q] * E1;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int e = (int)(ve[q][r] >> 16);
                if constexpr (WBP) {
                    m[q][r] = wbp_out(Sc - tv[r], Sc2 - cf[r], sc[q]) + m[q][r] * alpha;
                    if constexpr (MODEL == GNND_NBP) {
                        const int ec = e < E ? e : 0;
                        mb[e] = m[q][r] * (it + 1 < iters ? ww.msg(it + 1, ec) : ww.out_w(ec));
                    } else {
                        mb[e] = m[q][r];
                    }
                } else {
                    m[q][r] = M::post(Sc - tv[r], Sc2 - cf[r], sc[q], m[q][r], mlp_msg, s_w, w);
                    mb[e] = m[q][r];
                }
            }
        }
        __syncthreads();
        // the latency-bound variable-sum step first at the issue arbiter (its LDS read chains
        // start while other workgroups' waves fill the VALU; BCH CGNNI +0.5 %,
        // profiles/r03/experiments/headline_mlp_batch_prio_ab_r03l.txt)
        if constexpr (GNND_VAR_PRIO > 0) __builtin_amdgcn_s_setprio(GNND_VAR_PRIO);
        // variable sums, codeword fastest, variables in degree order (var_ord): a wave's
        // lanes sum 64 / CW variables of (nearly) the same degree for consecutive codewords
        // (odd stride E+1: no bank conflicts).  Edge (index_add) order within a variable;
        // two-value ds_read2 loads, four values in flight per step, no masking.
        const bool last = it + 1 == iters;
        // the variable step's result for variable v of codeword b (sum s of its messages):
        // last iteration -> readout (GNN T layout: s = S' base-2 scaled, S + x = s ln2 + x);
        // otherwise the check step's operand (T_v = s + x_v, or S_v of {S_v, x_v})
        auto var_out = [&](int b, int sbase, int tbase, int v, int tp, T s) {
            if (last) {
                T r;
                if constexpr (kTX && kB2) r = s * kLn2;             // (S' + x') ln2 = S + x
                else if constexpr (kTX) r = s;                       // S + x
                else r = s + (kBase2 ? io_ld(xg[b * N + v]) : s_sx[sbase + v].x);
                out[b0 * V + sbase + v] = io_st<TI>(M::readout(r, s_w));
            } else if constexpr (kTX) {
#ifdef GNND_DIAG_VAR_LINEAR
                s_t[(int)(threadIdx.x & 63)] = s;
                (void)tbase; (void)tp;
#else
                s_t[tbase + tp] = s;                                  // T_v = S_v + x_v
#endif
                (void)v;
            } else {
                s_sx[sbase + v].s = s;
            }
        };
        // one variable-item (codeword b, degree-order index i); mbase = b E1, sbase = b V,
        // tbase = b TS
        auto var_item = [&](int b, int i, int mbase, int sbase, int tbase) {
            const uint2 o = s_vord[i];
            const int v = (int)(o.x & 0xffffu), dv = (int)(o.x >> 16);
#ifdef GNND_DIAG_VAR_LINEAR
            // diagnostic build only (wrong results): lane-linear, conflict-free message-run reads
            const T* mp = s_m + (int)(threadIdx.x & 63);
            (void)mbase;
#else
            const T* mp = s_m + mbase + (int)(o.y & 0xffffu);
#endif
            if constexpr (MODEL == GNND_V22) {
                // decoder_v2_2.py:333-347: the check step publishes raw messages (identity
                // layout: positions = edge ids); the variable step forms the next layer's
                // S'_v = sum_e m_e W_{t+1}[e] (its v->c input, as in neural_BP) and the
                // iteration's readout sigmoid(-(sum_e m_e W[e] + sum_e x_v W_pr[e])), every
                // sum in edge (index_add) order
                const int e0 = (int)(o.y & 0xffffu);
                const T xv = s_sx[sbase + v].x;
                T sn = T(0), so = T(0), s2 = T(0);
                for (int k = 0; k < dv; ++k) {
                    const T mk = mp[k];
                    so += mk * ww.out_w(e0 + k);
                    s2 += xv * ww.out_p(e0 + k);
                    if (!last) sn += mk * ww.msg(it + 1, e0 + k);
                }
                out[(size_t)it * (size_t)B * V + (size_t)b0 * V + sbase + v] =
                    io_st<TI>(sigmoid_ref(-(so + s2)));
                if (!last) s_sx[sbase + v].s = sn;
                return;
            }
            T s = T(0);
            int k = 0;
            for (; k + 4 <= dv; k += 4) {
                const T a0 = mp[k], a1 = mp[k + 1], a2 = mp[k + 2], a3 = mp[k + 3];
                s += a0; s += a1; s += a2; s += a3;
            }
            if (dv & 2) {
                const T a0 = mp[k], a1 = mp[k + 1];
                s += a0; s += a1;
                k += 2;
            }
            if (dv & 1) s += mp[k];
            if constexpr (MODEL == GNND_NBP) {
                if (last) {   // + sum_v(x_v W_p)  (neural_BP.py:307-312)
                    const T xv = s_sx[sbase + v].x;
                    T s2 = T(0);
                    for (int j = 0; j < dv; ++j) s2 += xv * ww.out_p((int)(o.y & 0xffffu) + j);
                    out[b0 * V + sbase + v] = io_st<TI>(sigmoid_ref(-(s + s2)));
                    return;
                }
            }
            var_out(b, sbase, tbase, v, (int)(o.y >> 16), s);
        };
        if (vuni) {
            // padded layout (GraphView::vlay): the wave's vgroup variables share one padded
            // degree, so the sum is straight-line code selected by a wave-uniform switch —
            // no masks, no per-edge address or loop arithmetic.  Reference (index_add) order;
            // the padding zeros come last (s + 0 == s).
#ifndef GNND_VAR_PAIR
#define GNND_VAR_PAIR 0            // 1: the two cached entries' sums interleaved (A/B)
#endif
            if (vact && GNND_VAR_PAIR && kVC == 2 && vi0 + vstep < V) {
                // both cached entries (every lane has them: vi0 + vstep < V)
                const int va = (last || !kTX) ? (int)(s_vord[vi0].x & 0xffffu) : 0;
                const int vbb = (last || !kTX) ? (int)(s_vord[vi0 + vstep].x & 0xffffu) : 0;
                const int pa = (int)(vc_mt[0] & 0xffffu), ta = (int)(vc_mt[0] >> 16);
                constexpr int k1 = kVC > 1 ? 1 : 0;
                const int pb = (int)(vc_mt[k1] & 0xffffu), tb = (int)(vc_mt[k1] >> 16);
                T sa, sb;
                var_sum_uniform2(s_m + pa, vc_dp[0], s_m + pb, vc_dp[k1], sa, sb);
                var_out(vb, vsbase, vtbase, va, ta, sa);
                var_out(vb, vsbase, vtbase, vbb, tb, sb);
            } else if (vact) {
#pragma unroll
                for (int k = 0; k < kVC; ++k) {
                    const int i = vi0 + k * vstep;
                    if (i < V) {
                        // (v: the readout's output row in the last iteration; every iteration
                        // of the {S_v, x_v} layouts, whose S_v row it indexes)
                        const int v = (last || !kTX) ? (int)(s_vord[i].x & 0xffffu) : 0;
                        const int pm = (int)(vc_mt[k] & 0xffffu), pt = (int)(vc_mt[k] >> 16);
                        GNND_DCHECK(pm - vmbase + vc_dp[k] <= E1, GNND_DBG_LDS_POS);
                        var_out(vb, vsbase, vtbase, v, pt, var_sum_uniform(s_m + pm, vc_dp[k]));
                    }
                }
            }
            if (vact) {
                for (int i = vi0 + kVC * vstep; i < V; i += vstep) {
                    const uint2 o = s_vord[i];
                    const int dp = __builtin_amdgcn_readfirstlane((int)(o.x >> 16));
                    const int v = (int)(o.x & 0xffffu);
                    GNND_DCHECK(v < V && (int)(o.y & 0xffffu) + dp <= E1, GNND_DBG_LDS_POS);
                    var_out(vb, vsbase, vtbase, v, (int)(o.y >> 16),
                            var_sum_uniform(s_m + vmbase + (int)(o.y & 0xffffu), dp));
                }
            }
        } else if (vfixed) {
            // CW divides 256: f = tid + k 256 keeps f mod CW, so the lane's codeword and its
            // LDS bases are loop-invariant (no per-item division or 32-bit multiplies: those
            // are quarter-rate and cost as much as the sums themselves)
            if (vact)
                for (int i = vi0; i < V; i += vstep) var_item(vb, i, vmbase, vsbase, vtbase);
        } else {
            for (int f = tid; f < V * CW; f += GNND_BLOCK) {
                const int i = fdiv(f, dItem), b = f - i * CW;
                if (b >= nb) continue;
                var_item(b, i, b * E1, b * V, b * TS);
            }
        }
        if constexpr (GNND_VAR_PRIO > 0) __builtin_amdgcn_s_setprio(0);
        __syncthreads();
    }
    };
    // Plans with more than 64 item-state VGPRs only (the headline's Q = 9, R = 3).  The lighter
    // plans (LDPC Q = 6, R = 4; toric R = 4) spend their spare registers on five cached variable
    // entries (kLightRegs), and with three loop copies the allocator reloaded 10-18 spilled values
    // per iteration in their variable step; they keep the one 10-unit body, which is exact for
    // any live count (zero-weight tail).
    constexpr bool kSpecialize = kBase2 && GNND_MLP_SPECIALIZE && QMAX * (2 * R + 2) > 64;
    if constexpr (kSpecialize) {
        // one wave-uniform switch per kernel (nlive: readfirstlane in Mlp10Pair::load); fewer
        // than 8 live units run the NU = 8 body, whose zero-weight tail is exact
        switch (mlp2.nlive) {
            case 10: run_iters(std::integral_constant<int, 10>{}); break;
            case 9: run_iters(std::integral_constant<int, 9>{}); break;
            default: run_iters(std::integral_constant<int, 8>{}); break;
        }
    } else {
        run_iters(std::integral_constant<int, 10>{});
    }
    if (iters == 0 && MODEL != GNND_V22)        // (V22: zero iterations, empty readout list)
        for (int f = tid; f < nb * V; f += GNND_BLOCK) {
            const int b = fdiv(f, dV), v = f - b * V;
            if constexpr (MODEL == GNND_NBP) {
                T s2 = T(0);
                for (int k = g.var_ptr[v]; k < g.var_ptr[v + 1]; ++k) s2 += io_ld(xg[b * N + v]) * ww.out_p(k);
                out[b0 * V + f] = io_st<TI>(sigmoid_ref(-s2));
            } else {
                out[b0 * V + f] = io_st<TI>(M::readout(io_ld(xg[b * N + v]), s_w));
            }
        }
}

// graph-independent weight count (-1: unknown model, -2: depends on the graph and T)
int weights_count(int model) {
    switch (model) {
        case GNND_CGNNI: case GNND_QGNNI: return 62;
        case GNND_V24: return 1283;
        case GNND_CBP: case GNND_QBP: return 0;
        case GNND_NBP: case GNND_V10: case GNND_V22: return -2;
        case GNND_V30: return kV30Count;
        default: return -1;
    }
}
int64_t decode_weights_count(int model, int E, int iters) {
    if (model == GNND_NBP || model == GNND_V22) return 2 * (int64_t)E * iters + 2 * (int64_t)E + 1;
    if (model == GNND_V10) return (int64_t)E * iters + 1;
    return weights_count(model);
}
// weights staged in LDS by the decode kernels (decoder_v2_4 reads its weights through the scalar
// cache: none; its fp64 form stages tables and biases, counted in make_plan)
int lds_weights(int model) {
    const int n = weights_count(model);
    return n > 0 && model != GNND_V24 ? n : 0;
}

constexpr size_t kLdsMax = 160 * 1024;
constexpr int kResidentQ[] = {3, 6, 9, 12};   // instantiated work items per lane
constexpr int kResidentRegBudget = 88;          // Q * (2R + 2) state VGPRs (<= 128 total)

// LDS budget per workgroup: 40 KiB -> 4 workgroups (16 waves) per CU.  GNND_LDS_TARGET
// (bytes) overrides it for tuning sweeps; GNND_NO_RESIDENT=1 forces the streaming kernel.
bool lds_target_set() {                // GNND_LDS_TARGET given (A/B): it overrides every budget
    static const bool v = gnnd_tune_env("GNND_LDS_TARGET") != nullptr;
    return v;
}
size_t lds_target() {
    static size_t v = [] {
        const char* e = gnnd_tune_env("GNND_LDS_TARGET");
        long n = e ? atol(e) : 0;
        return n >= 4096 && n <= (long)kLdsMax ? (size_t)n : (size_t)(40 * 1024);
    }();
    return v;
}
// GNND_NO_F64_RESIDENT=1: fp64 light models on the streaming kernel (A/B)
bool f64_resident_disabled() {
    static bool v = [] {
        const char* e = gnnd_tune_env("GNND_NO_F64_RESIDENT");
        return e && e[0] == '1';
    }();
    return v;
}
bool resident_disabled() {
    static bool v = [] {
        const char* e = gnnd_tune_env("GNND_NO_RESIDENT");
        return e && e[0] == '1';
    }();
    return v;
}

// GNND_NO_VLAYOUT=1: resident kernel on the identity message layout (A/B measurements)
bool vlayout_disabled() {
    static bool v = [] {
        const char* e = gnnd_tune_env("GNND_NO_VLAYOUT");
        return e && e[0] == '1';
    }();
    return v;
}

struct Plan {
    const GraphView* view;   // slot plan the chosen kernel runs on (gnnd_graph::view/rview)
    bool resident;
    int cw;       // codewords per workgroup
    int q;        // work items per lane (resident)
    size_t lds;   // bytes of dynamic LDS
    int us = 1;   // unit split of the streaming kernel (fp32 decoder_v2_4, small batches)
    int wide = 1; // work-item lanes / 256 of the streaming kernel (fp64 decoder_v2_4, GNND_V24F64_WIDE)
    bool iw3 = false;  // unit split in rounds of 192 item lanes (decode_kernel IW3)
    int ncomp = 1;                       // split graph: components per codeword (streaming)
    const GraphView* dviews = nullptr;   // device [ncomp] views of the plan's kind
};

// The component split pays while a whole-codeword launch would leave CUs idle: below one
// codeword per CU (the latency-bound training steps and small decodes).  At larger batches the
// whole-graph workgroups already fill the chip and the split only doubles the per-codeword
// fixed costs (measured r03b: toric-7 training step B = 256 0.485 ms split vs 0.449 whole,
// B = 1024 1.63 vs 1.53; B = 128 0.285 vs 0.397).  GNND_SPLIT_ALWAYS=1 splits at every B.
int device_cus() {
    static int n = [] {
        int dev = 0, v = 0;
        if (hipGetDevice(&dev) != hipSuccess ||
            hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0) {
            (void)hipGetLastError();
            return 256;
        }
        return v;
    }();
    return n;
}
bool split_pays(int64_t B) {
    static bool always = [] {
        const char* e = gnnd_tune_env("GNND_SPLIT_ALWAYS");
        return e && e[0] == '1';
    }();
    return always || B < device_cus();
}
// GNND_NO_SPLIT=1: decode split graphs whole (A/B of the component split)
bool split_disabled() {
    static bool v = [] {
        const char* e = gnnd_tune_env("GNND_NO_SPLIT");
        return e && e[0] == '1';
    }();
    return v;
}

// GNND_V24_SPLIT=1|2|4|8 forces the fp32 decoder_v2_4 unit split (A/B); default by batch
// GNND_V24F64_US=2|4: fp64 decoder_v2_4 large batches (several codewords per workgroup) with
// the MLP units split over US waves as well (A/B; default 1)
int v24f64_us_big() {
    static int v = [] {
        const char* e = gnnd_tune_env("GNND_V24F64_US");
        const int n = e ? atoi(e) : 0;
        return n == 2 || n == 4 ? n : 1;
    }();
    return v;
}
// fp64 decoder_v2_4 large batches in workgroups of 512 work-item lanes, two per CU (make_plan;
// GNND_V24F64_WIDE = 1 / 4: 256 lanes three per CU / 1 024 lanes one per CU).  Same-box A/B
// (profiles/r05/experiments/ab_r05r_f64_wide.txt, config 3): 23.29 / 23.11 / 24.90 ms
int v24f64_wide() {
    static int v = [] {
        const char* e = gnnd_tune_env("GNND_V24F64_WIDE");
        const int n = e ? atoi(e) : 2;
        return n == 1 || n == 4 ? n : 2;
    }();
    return v;
}
// GNND_V24_UPAIR=0: fp32 decoder_v2_4 small batches on the R = 2 edge-pair plan (A/B of the
// unit-pair MLPs)
bool v24_upair_disabled() {
    static bool v = [] {
        const char* e = gnnd_tune_env("GNND_V24_UPAIR");
        return e && e[0] == '0';
    }();
    return v;
}
bool v24_iw3_disabled() {
    static bool v = [] {
        const char* e = gnnd_tune_env("GNND_V24_IW3");
        return e && e[0] == '0';
    }();
    return v;
}
int v24_split_forced() {
    static int v = [] {
        const char* e = gnnd_tune_env("GNND_V24_SPLIT");
        const int n = e ? atoi(e) : 0;
        return n == 1 || n == 2 || n == 4 || n == 8 ? n : 0;
    }();
    return v;
}

size_t align16(size_t n) { return (n + 15) & ~(size_t)15; }

// B = batch of the launch (plan queries without one assume a large batch)
int make_plan(int model, int dtype, const gnnd_graph* gr, Plan* p, int64_t B = INT64_MAX,
              bool allow_wide = true) {
    const size_t esz = dtype == GNND_F64 ? 8 : 4;
    const size_t wb = align16((size_t)lds_weights(model) * esz);
    const size_t target = lds_target();
    // light models may take the register-resident kernel; V24 and the GRU edge-state V30
    // run their own streaming kernels
    const bool light = model != GNND_V24 && model != GNND_V30;
    // fp64 (the quantum scripts' dtype): the same kernel with scalar math, fewer items per
    // lane (a double message takes two VGPRs) and twice the LDS budget (2 workgroups/CU).
    // Measured faster for the quantum models on the toric code (Q/BP +24 %, QGNNI +35 %,
    // decoder_v1_0 +11 %) and slower for the classical ones on BCH (-8..-10 %, whose
    // reference dtype is fp32 anyway): quantum models only.
    const bool quantum = model == GNND_QBP || model == GNND_QGNNI || model == GNND_NBP ||
                         model == GNND_V10 || model == GNND_V22;
    const bool f64res = dtype == GNND_F64 && quantum && !f64_resident_disabled();
    // (the ratio-form fp32 BP check step needs every check of degree >= 2: bp_ratio_msg)
    const bool ratio_bad = GNND_BP_RATIO && (model == GNND_CBP || model == GNND_QBP) && gr->min_dc < 2;
    if (light && (dtype == GNND_F32 || f64res) && gr->rview.G <= 16 && !resident_disabled() && !ratio_bad) {
        const GraphView& g = gr->rview;          // instantiated group sizes 1..16
        const size_t target = dtype == GNND_F64 ? 2 * lds_target() : lds_target();
        const int IC = g.C * g.G;
        // message layout for a tile of cw codewords: with cw | 256 a wave sums 64 / cw
        // consecutive var_ord entries per step, so the layout padded for that group size
        // makes its variable sums uniform (GraphView::vlay); weighted BP indexes per-edge
        // weights by edge id and keeps the identity layout
        const bool wbp = model == GNND_NBP || model == GNND_V10 || model == GNND_V22;
        // T-layout models (decode_resident_kernel kTX: the fp32 paired GNN / plain BP) run
        // on the x-augmented layouts (gnnd_graph::rlayx)
        const bool tx = dtype == GNND_F32 && !wbp;
        auto lay_of = [&](int cw) -> const GraphView* {
            const GraphView* lays = tx ? gr->rlayx : gr->rlay;
            if (!wbp && !vlayout_disabled() && GNND_BLOCK % cw == 0 && cw < 64) {
                int i = 0;
                while ((cw << i) < 64) ++i;
                if (lays[i].vlay) return &lays[i];
            }
            return &lays[0];
        };
        // resident layout: weights, var order, then [CW][P1] messages, [CW][V] {S, x},
        // [CW][C].  Pick (CW, Q) with Q in kResidentQ maximising lane utilisation
        // CW*IC / (Q*256), ties to the larger tile.
        // (+ the fp32 GNN message MLP's piecewise-linear table, pwl_stage)
        const size_t fixed = wb + align16((size_t)g.V * 8) +
                             (GNND_MLP_PWL && dtype == GNND_F32 && (model == GNND_CGNNI || model == GNND_QGNNI)
                                  ? kPwlBytes : 0);
        auto lds_of = [&](int cw) {     // messages, then {S_v, x_v} (T layout: T_v rows), x_c
            const GraphView* l = lay_of(cw);
            return fixed + esz * (((size_t)cw * l->P1 + 1) & ~(size_t)1) +
                   esz * ((size_t)cw * (tx ? (size_t)l->ts : 2 * (size_t)g.V) + (size_t)cw * g.C);
        };
        const bool tx_ok = !tx || gr->rlayx[0].vlay != nullptr;   // else: streaming kernel
        int best = 0, bestq = 0;
        double bestu = 0;
        static const int force_q = [] {
            const char* e = gnnd_tune_env("GNND_RESIDENT_Q");
            return e ? atoi(e) : 0;
        }();
        for (int q : kResidentQ) {
            if (dtype == GNND_F32 ? q * (2 * g.R + 2) > kResidentRegBudget
                                  : (q > 6 || q * (3 * g.R + 3) > kResidentRegBudget)) continue;
            if (force_q && q != force_q) continue;
            int cw = q * GNND_BLOCK / IC;               // largest tile that fits q items/lane
            if (cw > 64) cw = 64;
            while (cw > 1 && lds_of(cw) > target) --cw;
            if (cw < 1 || lds_of(cw) > kLdsMax || (cw * IC + GNND_BLOCK - 1) / GNND_BLOCK > q) continue;
            double u = (double)cw * IC / ((double)q * GNND_BLOCK);
            if (u > bestu + 1e-9 || (u > bestu - 1e-9 && cw > best)) { bestu = u; best = cw; bestq = q; }
        }
        if (best > 0 && bestu >= 0.5 && tx_ok) {
            p->view = lay_of(best);
            p->resident = true;
            p->cw = best;
            p->q = bestq;
            p->lds = lds_of(best);
            return GNND_OK;
        }
    }
    // streaming layout: weights, slot table, var_ptr, vslot, then [CW][nslot] messages,
    // [CW][V] {S, x}, [CW][C].  fp32 V24 runs its MLPs on slot PAIRS (two edges per packed
    // FMA): it takes the larger-R plan (toric dc = 4: G = 1, R = 4 instead of G = 4, R = 1)
    // (small batches: the R = 2 plan puts one edge pair per lane and the most lanes on a
    // codeword — the training step's latency-bound forward)
    const bool v24f32 = model == GNND_V24 && dtype == GNND_F32;
    // (B <= 4096 with a one-slot plan, toric: G = 4, R = 1): one edge per lane through the
    // unit-pair MLPs (mlp128_upair) — a component's edges fill whole item waves
    const bool upair = v24f32 && B <= 4096 && gr->view.R == 1 && !v24_upair_disabled();
    const GraphView& g = !v24f32 ? gr->view
                         : upair ? gr->view
                         : (B <= 4096 && gr->pview.R == 2) ? gr->pview : gr->rview;
    const size_t nslot = (size_t)g.C * g.G * g.R;
    // (fp64 V24: Softplus table, biases, linear parts, then the check-MLP table entries; fp32
    // V24: the check-MLP table entries)
    const size_t tab = model == GNND_V24 && dtype == GNND_F64
                           ? (size_t)(kV24F64TabDoubles + 3 * 128 + 16) * 8 +
                                 (GNND_V24_CTAB ? (size_t)ctab_entries(g.max_dc) * kCtabNC * 8 : 0)
                       : model == GNND_V24 && GNND_V24_CTAB
                           ? align16((size_t)ctab_entries(g.max_dc) * kCtabNC * 4)
                           : 0;
    // (decode_kernel stages the unit-pair weights whenever fp32 V24 runs a one-slot plan, kUP:
    // reserve them for every such plan, not only for the upair choice above — ADVICE r05)
    const bool up_lds = v24f32 && g.R == 1;
    const size_t fixed0 = wb + align16((nslot + g.V + 1 + g.E) * 4) + tab +
                          (up_lds ? (size_t)UpairLds::kFloats * 4 + 16 : 0);
    const bool v24f64 = model == GNND_V24 && dtype == GNND_F64;
    // (+ fp64 V24: the codeword's channel-prior table offset, s_vto, and its alignment)
    const size_t fixed = fixed0 + (v24f64 ? 16 : 0);
    const size_t per = esz * (nslot + 2 * (size_t)g.V + g.C) + (v24f64 ? 4 : 0);
    if (fixed + per > kLdsMax) return GNND_ERR_UNSUPPORTED;
    // fp64 decoder_v2_4 stages its 33 KB Softplus table per workgroup: a third of the CU's LDS
    // per 256-lane workgroup (3 per CU; toric-5: 4 codewords, 3 full item rounds; the default
    // 512-lane form below: half, 2 per CU, 8 codewords).  Same-box A/B
    // (profiles/r04/experiments/v24_f64_shapes_ab_r04g.txt): 2.24 M cw/s vs 1.96 M at 80 KB
    // (2 per CU), 2.17 M with the units split over 2 waves, 1.74 M over 4
#ifndef GNND_V24F64_LDS
#define GNND_V24F64_LDS (GNND_F64_SPTAB ? (kLdsMax / 3) & ~(size_t)15 : 0)
#endif
    size_t tgt = model == GNND_V24 && dtype == GNND_F64 && GNND_V24F64_LDS && !lds_target_set()
                     ? (size_t)GNND_V24F64_LDS : target;
    // (larger graphs, e.g. toric-7 at 7 KB per codeword: where a third of the LDS holds fewer
    // than two codewords, half of it: 2 workgroups per CU, several codewords each)
    if (tgt == (size_t)GNND_V24F64_LDS && tgt != target && fixed + 2 * per > tgt)
        tgt = (kLdsMax / 2) & ~(size_t)15;
    const int us_big = model == GNND_V24 && dtype == GNND_F64 && g.R <= 2 ? v24f64_us_big() : 1;
    const size_t bufb = us_big > 1 ? (size_t)2 * us_big * GNND_BLOCK * 8 + 8 : 0;
    // fp64 decoder_v2_4 at large batches (v24f64_wide: 2 by default): workgroups of 512 / 1 024
    // work-item lanes at a half / all of the CU's LDS, so one copy of the Softplus table serves
    // 8 / 16 waves (4 per SIMD instead of 3)
    int wide = 1;
    if (allow_wide && model == GNND_V24 && dtype == GNND_F64 && us_big == 1 &&
        tgt == (size_t)GNND_V24F64_LDS && tgt != target) {
        wide = v24f64_wide();
        if (wide > 1) tgt = (kLdsMax / (4 / wide)) & ~(size_t)15;
    }
    const size_t lanes = (size_t)GNND_BLOCK * wide;
    size_t n = fixed + bufb + per >= tgt ? 1 : (tgt - fixed - bufb) / per;
    if (n > 64) n = 64;
    // step-1 lane utilisation: the tile's C*G work items run in rounds of 256 lanes; among
    // tiles down to half the LDS-limited size take the one wasting the fewest lanes (ties:
    // larger).  toric-5 V24 fp32 (C*G = 48): 19 -> 16 codewords (3 full rounds, and 4
    // workgroups per CU instead of 3)
    // (fp64 V24 wide plans with channel-prior tables run two rounds per pass (kPt2); choosing the
    // tile by round-pair utilisation instead -- toric-5: 10 codewords, 0.94 of two passes, for 8 =
    // 3 rounds -- measured 1.8182 vs 1.8325 ms at B = 65 536 (noise) and moved B = 4 096 off the
    // wide form, 0.155 -> 0.208 ms: not kept)
    {
        const size_t IC = (size_t)g.C * g.G;
        const size_t span = lanes;
        size_t best = n;
        double bu = 0;
        for (size_t c = n; c >= 1 && 2 * c >= n; --c) {
            const size_t items = c * IC, rounds = (items + span - 1) / span;
            const double u = (double)items / (double)(rounds * span);
            if (u > bu + 1e-9) { bu = u; best = c; }
        }
        n = best;
    }
    // small batches (training steps, latency-bound decodes): at least ~2 workgroups per CU
    // before grouping codewords (B = 128 -> one codeword per workgroup, 128 workgroups)
    if ((int64_t)n * 512 > B) {
        if (wide > 1) return make_plan(model, dtype, gr, p, B, false);
        n = (size_t)(B / 512 > 1 ? B / 512 : 1);
    }
    p->view = &g;
    p->resident = false;
    p->cw = (int)n;
    p->q = 0;
    p->lds = fixed + n * per;
    p->wide = wide;
    // fp32 decoder_v2_4 at one codeword per workgroup (training steps, small decodes) is
    // latency-bound: one wave per SIMD walks 128 hidden units per edge pair.  Split the units
    // over US waves (B <= 256: 4, one 16-wave workgroup per CU; B <= 512: 2; US = 8 runs 128
    // item lanes (1024 threads) when a codeword's items fit them).  The partial sums must fit.
    p->us = 1;
    if (v24f32 && n == 1 && g.R <= 2) {
        const int forced = v24_split_forced();
        const bool fit128 = (size_t)g.C * g.G <= 128;
        // (US = 8 measured slower than 4 on the split toric-7 step, r03c: 0.283 vs 0.276 ms at
        // B = 128 -- the per-item overhead repeats in every split wave; forced only)
        int us = forced ? forced : B <= 256 ? 4 : B <= 512 ? 2 : 1;
        if (us == 8 && (!fit128 || upair)) us = 4;      // (unit pairs: US <= 4)
        const size_t il = us == 8 ? 128 : GNND_BLOCK;
        if (us > 1 && align16(p->lds) + (size_t)2 * us * il * 8 + 8 <= kLdsMax) {
            p->us = us;
            p->lds = align16(p->lds) + (size_t)2 * us * il * 8 + 8;
        }
    }
    // fp64 decoder_v2_4 (the reference dtype) the same way: one slot per lane (R <= 2 plans;
    // toric: G = 4, R = 1), the 128 units of every MLP over US = 4 (B <= 256) / 2 (B <= 512)
    // waves in four fixed chains (mlp128d_split)
    if (model == GNND_V24 && dtype == GNND_F64 && (n == 1 || us_big > 1) && g.R <= 2) {
        const int forced = v24_split_forced();
        int us = forced ? forced : n > 1 ? us_big : B <= 256 ? 4 : B <= 512 ? 2 : 1;
        if (us > 4) us = 4;
        // (+ the chain-major weights of the three MLPs, 16-byte aligned: mlp128d_chains_cm)
        const size_t wcm = GNND_F64_SPTAB ? (size_t)3 * 128 * sizeof(WcmEntry) + 16 : 0;
        if (us > 1 && align16(p->lds) + (size_t)2 * us * GNND_BLOCK * 8 + 8 + wcm <= kLdsMax) {
            p->us = us;
            p->lds = align16(p->lds) + (size_t)2 * us * GNND_BLOCK * 8 + 8 + wcm;
        }
    }
    // unit split with a tile of 129..192 work items (toric-7: one component-codeword of 192
    // edges, one per lane): rounds of three item waves, so no item wave (and none of its US - 1
    // unit-split partners) sits at the barriers without work -- a quarter of the 256-lane
    // form's waves
    if ((p->us == 2 || p->us == 4) && !v24_iw3_disabled()) {
        const size_t items = n * (size_t)g.C * g.G;
        p->iw3 = items > 128 && items <= 192;
    }
    return GNND_OK;
}

// The launch plan, split over the graph's components where that applies: decoder_v2_4's
// streaming kernel on a split graph (gnnd_graph::comp) decodes each component of a codeword in
// its own workgroup(s); the plan is made for component 0 (all components share its shape and
// slot plans) at the launch's B * ncomp component-codewords.
// allow_wide = false: the training forward (TAPE), whose decode_kernel instantiation runs 256
// work-item lanes, is planned for 256-lane workgroups (a WIDE plan's tile and LDS
// target would leave it at two workgroups per CU)
int plan_for(int model, int dtype, const gnnd_graph* g, Plan* p, int64_t B = INT64_MAX,
             bool allow_wide = true) {
    if (model == GNND_V24 && g->ncomp > 1 && g->dcomp && !g->nosplit && !split_disabled() &&
        split_pays(B)) {
        const int K = g->ncomp;
        const gnnd_graph* c0 = g->comp[0];
        const int64_t BK = B > INT64_MAX / K ? INT64_MAX : B * K;
        const int rc = make_plan(model, dtype, c0, p, BK, allow_wide);
        if (rc != GNND_OK) return rc;
        if (!p->resident) {
            const int kind = p->view == &c0->view ? 0 : p->view == &c0->rview ? 1 : 2;
            if (kind == 2 && p->view != &c0->pview) return GNND_ERR_UNSUPPORTED;
            p->ncomp = K;
            p->dviews = g->dcomp + (size_t)kind * K;
            return GNND_OK;
        }
    }
    return make_plan(model, dtype, g, p, B, allow_wide);
}

template <int MODEL, typename T, int R, typename TI = T>
int launch_decode(const Plan& p, const void* w, const void* x, void* out, int64_t B,
                  int iters, hipStream_t st, TapeView<T> tape = {}) {
    const GraphView& g = *p.view;
    int64_t blocks = (B + p.cw - 1) / p.cw;
    if (blocks > 0x7fffffff) return GNND_ERR_UNSUPPORTED;
    const int nw = lds_weights(MODEL);
    const FastDiv dI = make_fastdiv(p.resident ? p.cw : g.C * g.G);
    const FastDiv dV = make_fastdiv(g.V), dN = make_fastdiv(g.N);
    auto go = [&](auto kern, int us = 1) -> int {
        if (p.lds > 64 * 1024)
            GNND_HIP_CHECK(hipFuncSetAttribute((const void*)kern,
                                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds));
        kern<<<(unsigned)blocks, GNND_BLOCK * us, p.lds, st>>>(g, (const T*)w, nw, (const TI*)x, (TI*)out,
                                                               B, iters, p.cw, dI, dV, dN, tape);
        GNND_LAUNCH_CHECK();
        return GNND_OK;
    };
    // the streaming kernel: every component of a split graph in the same launch
    // persist: one workgroup per resident slot (occupancy x CUs), each looping over tiles
    // (decode_kernel's tile loop); split graphs never
    auto go_s = [&](auto kern, int us = 1, int wide = 1, bool persist = false, bool iw3 = false) -> int {
        if (p.lds > 64 * 1024)
            GNND_HIP_CHECK(hipFuncSetAttribute((const void*)kern,
                                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds));
        int64_t grid = blocks * p.ncomp;
        if (grid > 0x7fffffff) return GNND_ERR_UNSUPPORTED;
        const int il = iw3 ? 192 : (us == 8 ? 128 : GNND_BLOCK) * wide;  // decode_kernel's IL
        if (persist && p.ncomp == 1) {
            int per_cu = 0;
            GNND_HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, il * us, p.lds));
            const int64_t slots = (int64_t)(per_cu > 0 ? per_cu : 1) * device_cus();
            if (grid > slots) grid = slots;
        }
        kern<<<(unsigned)grid, il * us, p.lds, st>>>(g, (const T*)w, nw, (const TI*)x, (TI*)out,
                                                             B, iters, p.cw, dI, dV, dN, tape,
                                                             p.ncomp > 1 ? p.dviews : nullptr,
                                                             (int)blocks);
        GNND_LAUNCH_CHECK();
        return GNND_OK;
    };
    if constexpr (MODEL != GNND_V24) {
        if (p.resident) {
            auto by_q = [&](auto gtag, auto ptag) -> int {
                constexpr int G = decltype(gtag)::value;
                constexpr int P = decltype(ptag)::value;
                switch (p.q) {
                    case 3: return go(decode_resident_kernel<MODEL, T, G, R, 3, P, TI>);
                    case 6: return go(decode_resident_kernel<MODEL, T, G, R, 6, P, TI>);
                    case 9: if constexpr (R <= 3 && sizeof(T) == 4) return go(decode_resident_kernel<MODEL, T, G, R, 9, P, TI>);
                            break;
                    case 12: if constexpr (R <= 2 && sizeof(T) == 4) return go(decode_resident_kernel<MODEL, T, G, R, 12, P, TI>);
                             break;
                }
                return GNND_ERR_UNSUPPORTED;
            };
            auto by_g = [&](auto ptag) -> int {
                switch (g.G) {
                    case 1: return by_q(std::integral_constant<int, 1>{}, ptag);
                    case 2: return by_q(std::integral_constant<int, 2>{}, ptag);
                    case 4: return by_q(std::integral_constant<int, 4>{}, ptag);
                    case 8: return by_q(std::integral_constant<int, 8>{}, ptag);
                    case 16: return by_q(std::integral_constant<int, 16>{}, ptag);
                }
                return GNND_ERR_UNSUPPORTED;
            };
            if (!g.padded) return by_g(std::integral_constant<int, 0>{});
            if (g.padr == 1) return by_g(std::integral_constant<int, 1>{});
            return by_g(std::integral_constant<int, R>{});
        }
    }
    if constexpr (!std::is_same_v<TI, T> || MODEL == GNND_V22) {
        // bf16 I/O and decoder_v2_2's per-iteration readout: register-resident plans only
        return GNND_ERR_UNSUPPORTED;
    } else {
        if constexpr (MODEL == GNND_V24 && R <= 2) {
            if (p.iw3 && p.us == 4)
                return tape.ext ? go_s(decode_kernel<MODEL, T, R, true, 4, 1, true>, 4, 1, false, true)
                                : go_s(decode_kernel<MODEL, T, R, false, 4, 1, true>, 4, 1, false, true);
            if (p.iw3 && p.us == 2)
                return tape.ext ? go_s(decode_kernel<MODEL, T, R, true, 2, 1, true>, 2, 1, false, true)
                                : go_s(decode_kernel<MODEL, T, R, false, 2, 1, true>, 2, 1, false, true);
        }
        if constexpr (MODEL == GNND_V24 && sizeof(T) == 4 && R <= 2) {
            if (p.us == 8) return tape.ext ? go_s(decode_kernel<MODEL, T, R, true, 8>, 8)
                                           : go_s(decode_kernel<MODEL, T, R, false, 8>, 8);
            if (p.us == 4) return tape.ext ? go_s(decode_kernel<MODEL, T, R, true, 4>, 4)
                                           : go_s(decode_kernel<MODEL, T, R, false, 4>, 4);
            if (p.us == 2) return tape.ext ? go_s(decode_kernel<MODEL, T, R, true, 2>, 2)
                                           : go_s(decode_kernel<MODEL, T, R, false, 2>, 2);
        }
        if constexpr (MODEL == GNND_V24 && sizeof(T) == 8 && R <= 2) {
            if (p.us == 4) return tape.ext ? go_s(decode_kernel<MODEL, T, R, true, 4>, 4)
                                           : go_s(decode_kernel<MODEL, T, R, false, 4>, 4);
            if (p.us == 2) return tape.ext ? go_s(decode_kernel<MODEL, T, R, true, 2>, 2)
                                           : go_s(decode_kernel<MODEL, T, R, false, 2>, 2);
        }
        if (p.us != 1) return GNND_ERR_UNSUPPORTED;
        if constexpr (MODEL == GNND_V24)
            if (tape.ext) return go_s(decode_kernel<MODEL, T, R, true>);
        // fp64 decoder_v2_4 decodes run persistent (their prologue builds two LDS tables)
        constexpr bool kPersist = MODEL == GNND_V24 && sizeof(T) == 8;
        if constexpr (MODEL == GNND_V24 && sizeof(T) == 8 && R <= 2) {
            // (the plan's tile fits any lane count: WIDE only changes the rounds' width)
            if (p.wide == 2) return go_s(decode_kernel<MODEL, T, R, false, 1, 2>, 1, 2, kPersist);
            if (p.wide == 4) return go_s(decode_kernel<MODEL, T, R, false, 1, 4>, 1, 4, kPersist);
        }
        return go_s(decode_kernel<MODEL, T, R>, 1, 1, kPersist);
    }
}


// floss (gnnd_train_fwd_loss): the syndrome loss in the forward's epilogue; only fp32 V24
// unit-split plans (small batches) whose component split matches the reverse pass's
// (need_ncomp: the reverse pass's components per codeword) and whose partial-sum buffers
// hold the loss arrays; UNSUPPORTED otherwise (the caller keeps the reverse pass's loss)
struct FwdLoss {
    const void* y;
    const uint32_t* lmask;
    int nl, logical_only, need_ncomp;
    void* gp;
    void* loss_b;
};
template <int MODEL, typename T, typename TI = T>
int launch_decode_r(const gnnd_graph* g, const void* w, const void* x, void* out, int64_t B,
                    int iters, hipStream_t st, void* tape_base = nullptr,
                    const FwdLoss* floss = nullptr) {
    Plan p;
    int rc = plan_for(MODEL, sizeof(T) == 8 ? GNND_F64 : GNND_F32, g, &p, B, tape_base == nullptr);
    if (rc != GNND_OK) return rc;
    if (tape_base && p.wide != 1) return GNND_ERR_UNSUPPORTED;   // (planned without WIDE above)
    TapeView<T> tape{};
    if (tape_base) {                        // [ext | u | t] x [iters][B][E], then mT [B][E]
        if (p.resident) return GNND_ERR_UNSUPPORTED;
        const size_t n = (size_t)iters * B * g->view.E;
        T* base = (T*)tape_base;
        tape = TapeView<T>{base, base + n, base + 2 * n, base + 3 * n};
    }
    if (floss) {
        if (MODEL != GNND_V24 || sizeof(T) != 4 || !tape_base || p.us < 2 ||
            p.ncomp != floss->need_ncomp)
            return GNND_ERR_UNSUPPORTED;
        const GraphView& v = *p.view;
        const int il = p.us == 8 ? 128 : GNND_BLOCK;
        const size_t need = sizeof(T) * (size_t)p.cw * (v.V + 2 * (size_t)(v.C + floss->nl)) + 4 * (size_t)v.V;
        if (need > (size_t)2 * p.us * il * 8) return GNND_ERR_UNSUPPORTED;
        tape.y = (const T*)floss->y;
        tape.lmask = floss->lmask;
        tape.nl = floss->nl;
        tape.logical_only = floss->logical_only;
        tape.ncomp = p.ncomp;
        tape.gp = (T*)floss->gp;
        tape.loss_b = (T*)floss->loss_b;
    }
    switch (p.view->R) {
        case 1: return launch_decode<MODEL, T, 1, TI>(p, w, x, out, B, iters, st, tape);
        case 2: return launch_decode<MODEL, T, 2, TI>(p, w, x, out, B, iters, st, tape);
        case 3: return launch_decode<MODEL, T, 3, TI>(p, w, x, out, B, iters, st, tape);
        case 4: return launch_decode<MODEL, T, 4, TI>(p, w, x, out, B, iters, st, tape);
    }
    return GNND_ERR_UNSUPPORTED;
}

template <int MODEL>
int launch_model(const gnnd_graph* g, int dtype, const void* w, const void* x, void* out,
                 int64_t B, int iters, hipStream_t st) {
    if (dtype == GNND_F32) return launch_decode_r<MODEL, float>(g, w, x, out, B, iters, st);
    if (dtype == GNND_BF16) {      // bf16 x / out, fp32 arithmetic: the classical fp32 models
        if constexpr (MODEL == GNND_CGNNI || MODEL == GNND_CBP)
            return launch_decode_r<MODEL, float, bf16_t>(g, w, x, out, B, iters, st);
        return GNND_ERR_UNSUPPORTED;
    }
    return launch_decode_r<MODEL, double>(g, w, x, out, B, iters, st);
}

}  // namespace

// per-model launchers (one translation unit each, compiled in parallel)
int gnnd_launch_v24(const gnnd_graph*, int, const void*, const void*, void*, int64_t, int, hipStream_t);
// forward with the training tape (gnnd_train.hip)
int gnnd_launch_v24_tape(const gnnd_graph*, int, const void*, const void*, void*, int64_t, int,
                         void*, hipStream_t);
// ... with decoder_v2_4's syndrome loss in the epilogue (y, logical masks, n_logical,
// logical_only, the reverse pass's components per codeword) -> d loss / d out, losses
int gnnd_launch_v24_tape_loss(const gnnd_graph*, int, const void*, const void*, void*, int64_t, int,
                              void*, const void*, const uint32_t*, int, int, int, void*, void*,
                              hipStream_t);
int gnnd_launch_qgnni(const gnnd_graph*, int, const void*, const void*, void*, int64_t, int, hipStream_t);
int gnnd_launch_qbp(const gnnd_graph*, int, const void*, const void*, void*, int64_t, int, hipStream_t);
int gnnd_launch_cgnni(const gnnd_graph*, int, const void*, const void*, void*, int64_t, int, hipStream_t);
int gnnd_launch_cbp(const gnnd_graph*, int, const void*, const void*, void*, int64_t, int, hipStream_t);
int gnnd_launch_nbp(const gnnd_graph*, int, const void*, const void*, void*, int64_t, int, hipStream_t);
int gnnd_launch_v10(const gnnd_graph*, int, const void*, const void*, void*, int64_t, int, hipStream_t);
int gnnd_launch_v30(const gnnd_graph*, int, const void*, const void*, void*, int64_t, int, hipStream_t);
// decoder_v3_0 training (gnnd_decode_v30.hip): the forward with its tape
// ([B][T + 1][2][nslot] states of the plan's slot layout) and the reverse pass to one gradient
// row [137] per workgroup (gnnd_v30_train_rows of them)
int64_t gnnd_v30_tape_elems(const gnnd_graph*, int64_t, int);
int64_t gnnd_v30_train_rows(int64_t);
int gnnd_launch_v30_tape(const gnnd_graph*, int, const void*, const void*, void*, int64_t, int,
                         void*, hipStream_t);
int gnnd_launch_v30_bwd(const gnnd_graph*, int, const void*, const void*, const void*,
                        const void*, const void*, void*, int64_t, int64_t, int, hipStream_t);
// weighted-BP training (gnnd_train_wbp.hip, models NBP, V22 and V10, fp64): the same tape shape and
// one gradient row [2 E T + 2 E + 1] per workgroup
int64_t gnnd_wbp_tape_elems(const gnnd_graph*, int64_t, int);
int64_t gnnd_wbp_train_rows(int64_t);
int64_t gnnd_wbp_weights(const gnnd_graph*, int, int);
int gnnd_launch_wbp_tape(const gnnd_graph*, int, const void*, const void*, void*, int64_t, int,
                         void*, hipStream_t);
int gnnd_launch_wbp_bwd(const gnnd_graph*, int, const void*, const void*, const void*,
                        const void*, const void*, void*, int64_t, int64_t, int, hipStream_t);
int gnnd_launch_v22(const gnnd_graph*, int, const void*, const void*, void*, int64_t, int, hipStream_t);
// CGNNI / QGNNI training (gnnd_train_gnn.hip): the forward with its tape ([B][T][nslot] tanh
// outputs of the view's slot plan, then [B][V] readout inputs) and the reverse pass to one
// gradient row [62] per workgroup (gnnd_gnn_train_rows of them)
int64_t gnnd_gnn_tape_elems(const gnnd_graph*, int64_t, int);
int64_t gnnd_gnn_train_rows(int64_t);
int gnnd_launch_gnn_tape(const gnnd_graph*, int, int, const void*, const void*, void*, int64_t, int,
                         void*, hipStream_t);
int gnnd_launch_gnn_bwd(const gnnd_graph*, int, int, const void*, const void*, const void*,
                        const void*, void*, int64_t, int64_t, int, hipStream_t);

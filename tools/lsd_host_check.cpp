// Stand-alone check of the localized-statistics host mirrors
// (gnn-decode_amd/csrc/gnnd_lsd_host.h) for host sanitizers: reads case files written by
// tools/lsd_host_sanitize.sh
//   kind(0 lsd / 1 bplsd) V C E B dtype(0 f32 / 1 f64) base bits, E edges "v c", B*N x values and,
//   for kind 0, B*V pred values (C99 hex literals: exact), then
//   kind 0: B*V expected ehat bits, B expected statuses, rounds, cluster and column counts;
//   kind 1: alpha beta iters, then B*V expected ehat bits and B expected bp statuses.
// Kind 0 runs gnnd_lsd_host_checked with every output, with the optional outputs null, and
// gnnd_lsd_gated_host_checked with a gate over sentinel-filled outputs, with and without llr, and
// compares exactly.  Kind 1 runs gnnd_bplsd_host_checked and compares ehat and the min-sum status,
// and the other outputs with gnnd_minsum_host_checked and gnnd_lsd_gated_host_checked composed by
// hand.  Plain C++17, no HIP, no GPU.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../gnn-decode_amd/csrc/gnnd_lsd_host.h"

struct Case {
    int kind, V, C, dtype, base, bits;
    long E, B;
};

template <typename T>
static bool read_reals(FILE* f, std::vector<T>& a) {
    double d;
    for (auto& v : a) {
        if (fscanf(f, "%la", &d) != 1) return false;
        v = (T)d;
    }
    return true;
}

template <typename T>
static int run_lsd(FILE* f, const Case& k, const std::vector<int64_t>& var,
                   const std::vector<int64_t>& chk) {
    const size_t nv = (size_t)k.B * k.V;
    std::vector<T> x((size_t)k.B * (k.V + k.C)), pred(nv), ehat(nv), ehat2(nv), llr(nv);
    if (!read_reals(f, x) || !read_reals(f, pred)) return 2;
    std::vector<int32_t> ints[4], gate(k.B);
    for (auto& a : ints) a.resize(k.B);
    int rc = gnnd_lsd_host_checked(var.data(), chk.data(), k.E, k.V, k.C, k.dtype, x.data(),
                                   pred.data(), k.base, k.bits, ehat.data(), ints[0].data(),
                                   ints[1].data(), ints[2].data(), ints[3].data(), k.B);
    if (rc != GNND_OK) { fprintf(stderr, "gnnd_lsd_host: status %d\n", rc); return 1; }
    rc = gnnd_lsd_host_checked(var.data(), chk.data(), k.E, k.V, k.C, k.dtype, x.data(),
                               pred.data(), k.base, k.bits, ehat2.data(), nullptr, nullptr, nullptr,
                               nullptr, k.B);
    if (rc != GNND_OK) { fprintf(stderr, "gnnd_lsd_host (null outputs): status %d\n", rc); return 1; }
    long bad = memcmp(ehat.data(), ehat2.data(), nv * sizeof(T)) != 0;
    for (long b = 0; b < k.B; ++b) gate[b] = b % 3 == 1 ? 0 : (int32_t)(b + 1);
    for (size_t i = 0; i < nv; ++i) llr[i] = (i % 5 < 2) ? T(-1) : T(0.5);
    for (int with_llr = 0; with_llr <= 1; ++with_llr) {
        std::vector<T> ehat3(nv, T(7));
        std::vector<int32_t> gated[4];
        for (auto& a : gated) a.assign(k.B, 7);
        rc = gnnd_lsd_gated_host_checked(var.data(), chk.data(), k.E, k.V, k.C, k.dtype, x.data(),
                                         pred.data(), with_llr ? llr.data() : nullptr, gate.data(),
                                         k.base, k.bits, ehat3.data(), gated[0].data(),
                                         gated[1].data(), gated[2].data(), gated[3].data(), k.B);
        if (rc != GNND_OK) { fprintf(stderr, "gnnd_lsd_gated_host: status %d\n", rc); return 1; }
        for (long b = 0; b < k.B; ++b) {
            for (int v = 0; v < k.V; ++v) {
                const size_t i = (size_t)b * k.V + v;
                const bool h = with_llr ? llr[i] < T(0) : pred[i] > T(0.5);
                bad += ehat3[i] != (gate[b] ? ehat[i] : h ? T(1) : T(0));
            }
            for (int j = 0; j < 4; ++j) bad += gated[j][b] != (gate[b] ? ints[j][b] : 0);
        }
    }
    for (size_t i = 0; i < nv; ++i) {
        int want;
        if (fscanf(f, "%d", &want) != 1) return 2;
        bad += ehat[i] != (T)want;
    }
    long unsolved = 0;
    for (int j = 0; j < 4; ++j)
        for (long b = 0; b < k.B; ++b) {
            int want;
            if (fscanf(f, "%d", &want) != 1) return 2;
            bad += ints[j][b] != want;
            unsolved += j == 0 && want != 0;
        }
    printf("lsd V %d C %d B %ld dtype %d base %d bits %d: %ld mismatches, %ld codewords without a "
           "solution\n", k.V, k.C, k.B, k.dtype, k.base, k.bits, bad, unsolved);
    return bad != 0;
}

template <typename T>
static int run_bplsd(FILE* f, const Case& k, const std::vector<int64_t>& var,
                     const std::vector<int64_t>& chk) {
    const size_t nv = (size_t)k.B * k.V;
    std::vector<T> x((size_t)k.B * (k.V + k.C));
    if (!read_reals(f, x)) return 2;
    double alpha, beta;
    int iters;
    if (fscanf(f, "%la %la %d", &alpha, &beta, &iters) != 3) return 2;
    std::vector<T> ehat(nv), pred(nv), llr(nv), pred2(nv), llr2(nv), ehat2(nv);
    std::vector<int32_t> a[6], b2[6];          // iters, bp status, status, rounds, nclus, ncols
    for (auto& v : a) v.resize(k.B);
    for (auto& v : b2) v.resize(k.B);
    int rc = gnnd_bplsd_host_checked(var.data(), chk.data(), k.E, k.V, k.C, k.dtype, x.data(), alpha,
                                     beta, iters, 1, k.base, k.bits, pred.data(), llr.data(),
                                     a[0].data(), a[1].data(), ehat.data(), a[2].data(), a[3].data(),
                                     a[4].data(), a[5].data(), k.B);
    if (rc != GNND_OK) { fprintf(stderr, "gnnd_bplsd_host: status %d\n", rc); return 1; }
    rc = gnnd_minsum_host_checked(var.data(), chk.data(), k.E, k.V, k.C, k.dtype, x.data(), alpha,
                                  beta, iters, 1, pred2.data(), llr2.data(), b2[0].data(),
                                  b2[1].data(), k.B, true);
    if (rc != GNND_OK) { fprintf(stderr, "gnnd_minsum_host: status %d\n", rc); return 1; }
    rc = gnnd_lsd_gated_host_checked(var.data(), chk.data(), k.E, k.V, k.C, k.dtype, x.data(),
                                     pred2.data(), llr2.data(), b2[1].data(), k.base, k.bits,
                                     ehat2.data(), b2[2].data(), b2[3].data(), b2[4].data(),
                                     b2[5].data(), k.B);
    if (rc != GNND_OK) { fprintf(stderr, "gnnd_lsd_gated_host (by hand): status %d\n", rc); return 1; }
    long bad = memcmp(ehat.data(), ehat2.data(), nv * sizeof(T)) != 0;
    bad += memcmp(llr.data(), llr2.data(), nv * sizeof(T)) != 0;
    bad += memcmp(pred.data(), pred2.data(), nv * sizeof(T)) != 0;
    for (int j = 0; j < 6; ++j) bad += a[j] != b2[j];
    rc = gnnd_bplsd_host_checked(var.data(), chk.data(), k.E, k.V, k.C, k.dtype, x.data(), alpha,
                                 beta, iters, 1, k.base, k.bits, pred2.data(), llr2.data(), nullptr,
                                 b2[1].data(), ehat2.data(), nullptr, nullptr, nullptr, nullptr, k.B);
    if (rc != GNND_OK) { fprintf(stderr, "gnnd_bplsd_host (null outputs): status %d\n", rc); return 1; }
    bad += memcmp(ehat.data(), ehat2.data(), nv * sizeof(T)) != 0;
    for (size_t i = 0; i < nv; ++i) {
        int want;
        if (fscanf(f, "%d", &want) != 1) return 2;
        bad += ehat[i] != (T)want;
    }
    long unsolved = 0;
    for (long b = 0; b < k.B; ++b) {
        int want;
        if (fscanf(f, "%d", &want) != 1) return 2;
        bad += a[1][b] != want;
        unsolved += want != 0;
    }
    printf("bplsd V %d C %d B %ld dtype %d base %d bits %d: %ld mismatches, %ld codewords left to "
           "lsd\n", k.V, k.C, k.B, k.dtype, k.base, k.bits, bad, unsolved);
    return bad != 0;
}

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: %s CASE_FILE...\n", argv[0]); return 2; }
    for (int a = 1; a < argc; ++a) {
        FILE* f = fopen(argv[a], "r");
        if (!f) { perror(argv[a]); return 2; }
        Case k;
        if (fscanf(f, "%d %d %d %ld %ld %d %d %d", &k.kind, &k.V, &k.C, &k.E, &k.B, &k.dtype,
                   &k.base, &k.bits) != 8)
            return 2;
        std::vector<int64_t> var(k.E), chk(k.E);
        for (long e = 0; e < k.E; ++e) {
            long v, c;
            if (fscanf(f, "%ld %ld", &v, &c) != 2) return 2;
            var[e] = v;
            chk[e] = c;
        }
        int rc;
        if (k.kind == 0)
            rc = k.dtype == GNND_F32 ? run_lsd<float>(f, k, var, chk) : run_lsd<double>(f, k, var, chk);
        else
            rc = k.dtype == GNND_F32 ? run_bplsd<float>(f, k, var, chk)
                                     : run_bplsd<double>(f, k, var, chk);
        fclose(f);
        if (rc) return rc;
    }
    return 0;
}

// Stand-alone check of the weighted union-find and belief-find host mirrors
// (gnn-decode_amd/csrc/gnnd_ufw_host.h) for host sanitizers: reads case files written by
// tools/ufw_host_sanitize.sh
//   kind(0 ufw / 1 belief-find) V C E B dtype(0 f32 / 1 f64) has_llr scale wmax, E edges "v c",
//   B*N x values and, with has_llr, B*V llr values (C99 hex literals: exact), then
//   kind 0: B*V expected ehat bits, B expected rounds, statuses, full-edge counts and events;
//   kind 1: alpha beta iters, then B*V expected ehat bits and B expected bp statuses.
// Kind 0 runs gnnd_ufw_host_checked with every output, with the optional outputs null, and with a
// gate over sentinel-filled outputs in both pass-through modes, and compares exactly.  Kind 1 runs
// gnnd_belief_find_host_checked and compares ehat and the min-sum status, and the other outputs
// with gnnd_minsum_host_checked and gnnd_ufw_host_checked composed by hand.
// Plain C++17, no HIP, no GPU.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../gnn-decode_amd/csrc/gnnd_ufw_host.h"

struct Case {
    int kind, V, C, dtype, has_llr, wmax;
    long E, B;
    double scale;
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
static int run_ufw(FILE* f, const Case& k, const std::vector<int64_t>& var,
                   const std::vector<int64_t>& chk) {
    const size_t nv = (size_t)k.B * k.V;
    std::vector<T> x((size_t)k.B * (k.V + k.C)), llr(k.has_llr ? nv : 0), ehat(nv), ehat2(nv);
    if (!read_reals(f, x) || !read_reals(f, llr)) return 2;
    const T* lp = k.has_llr ? llr.data() : nullptr;
    std::vector<int32_t> ints[4], gate(k.B);
    for (auto& a : ints) a.resize(k.B);
    int rc = gnnd_ufw_host_checked(var.data(), chk.data(), k.E, k.V, k.C, k.dtype, x.data(), lp,
                                   k.scale, k.wmax, nullptr, 0, ehat.data(), ints[0].data(),
                                   ints[1].data(), ints[2].data(), ints[3].data(), k.B);
    if (rc != GNND_OK) { fprintf(stderr, "gnnd_ufw_host: status %d\n", rc); return 1; }
    rc = gnnd_ufw_host_checked(var.data(), chk.data(), k.E, k.V, k.C, k.dtype, x.data(), lp,
                               k.scale, k.wmax, nullptr, 0, ehat2.data(), nullptr, nullptr, nullptr,
                               nullptr, k.B);
    if (rc != GNND_OK) { fprintf(stderr, "gnnd_ufw_host (null outputs): status %d\n", rc); return 1; }
    long bad = memcmp(ehat.data(), ehat2.data(), nv * sizeof(T)) != 0;
    for (long b = 0; b < k.B; ++b) gate[b] = b % 3 == 1 ? 0 : (int32_t)(b + 1);
    for (int pass = 0; pass <= k.has_llr; ++pass) {
        std::vector<T> ehat3(nv, T(7));
        std::vector<int32_t> gated[4];
        for (auto& a : gated) a.assign(k.B, 7);
        rc = gnnd_ufw_host_checked(var.data(), chk.data(), k.E, k.V, k.C, k.dtype, x.data(), lp,
                                   k.scale, k.wmax, gate.data(), pass, ehat3.data(),
                                   gated[0].data(), gated[1].data(), gated[2].data(),
                                   gated[3].data(), k.B);
        if (rc != GNND_OK) { fprintf(stderr, "gnnd_ufw_host (gated): status %d\n", rc); return 1; }
        for (long b = 0; b < k.B; ++b) {
            for (int v = 0; v < k.V; ++v) {
                const size_t i = (size_t)b * k.V + v;
                const T want = gate[b] ? ehat[i] : pass ? (llr[i] < T(0) ? T(1) : T(0)) : T(7);
                bad += ehat3[i] != want;
            }
            for (int j = 0; j < 4; ++j)
                bad += gated[j][b] != (gate[b] ? ints[j][b] : pass ? 0 : 7);
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
            unsolved += j == 1 && want != 0;
        }
    printf("ufw V %d C %d B %ld dtype %d llr %d: %ld mismatches, %ld codewords without a solution\n",
           k.V, k.C, k.B, k.dtype, k.has_llr, bad, unsolved);
    return bad != 0;
}

template <typename T>
static int run_belief_find(FILE* f, const Case& k, const std::vector<int64_t>& var,
                           const std::vector<int64_t>& chk) {
    const size_t nv = (size_t)k.B * k.V;
    std::vector<T> x((size_t)k.B * (k.V + k.C));
    if (!read_reals(f, x)) return 2;
    double alpha, beta;
    int iters;
    if (fscanf(f, "%la %la %d", &alpha, &beta, &iters) != 3) return 2;
    std::vector<T> ehat(nv), pred(nv), llr(nv), pred2(nv), llr2(nv), ehat2(nv);
    std::vector<int32_t> a[6], b2[6];
    for (auto& v : a) v.resize(k.B);
    for (auto& v : b2) v.resize(k.B);
    // a: iters, bp status, status, rounds, nfull, events
    int rc = gnnd_belief_find_host_checked(var.data(), chk.data(), k.E, k.V, k.C, k.dtype, x.data(),
                                           alpha, beta, iters, 1, k.scale, k.wmax, pred.data(),
                                           llr.data(), a[0].data(), a[1].data(), ehat.data(),
                                           a[2].data(), a[3].data(), a[4].data(), a[5].data(), k.B);
    if (rc != GNND_OK) { fprintf(stderr, "gnnd_belief_find_host: status %d\n", rc); return 1; }
    rc = gnnd_minsum_host_checked(var.data(), chk.data(), k.E, k.V, k.C, k.dtype, x.data(), alpha,
                                  beta, iters, 1, pred2.data(), llr2.data(), b2[0].data(),
                                  b2[1].data(), k.B, true);
    if (rc != GNND_OK) { fprintf(stderr, "gnnd_minsum_host: status %d\n", rc); return 1; }
    rc = gnnd_ufw_host_checked(var.data(), chk.data(), k.E, k.V, k.C, k.dtype, x.data(), llr2.data(),
                               k.scale, k.wmax, b2[1].data(), 1, ehat2.data(), b2[3].data(),
                               b2[2].data(), b2[4].data(), b2[5].data(), k.B);
    if (rc != GNND_OK) { fprintf(stderr, "gnnd_ufw_host (by hand): status %d\n", rc); return 1; }
    long bad = memcmp(ehat.data(), ehat2.data(), nv * sizeof(T)) != 0;
    bad += memcmp(llr.data(), llr2.data(), nv * sizeof(T)) != 0;
    bad += memcmp(pred.data(), pred2.data(), nv * sizeof(T)) != 0;
    for (int j = 0; j < 6; ++j) bad += a[j] != b2[j];
    rc = gnnd_belief_find_host_checked(var.data(), chk.data(), k.E, k.V, k.C, k.dtype, x.data(),
                                       alpha, beta, iters, 1, k.scale, k.wmax, pred2.data(),
                                       llr2.data(), nullptr, b2[1].data(), ehat2.data(), nullptr,
                                       nullptr, nullptr, nullptr, k.B);
    if (rc != GNND_OK) { fprintf(stderr, "gnnd_belief_find_host (null outputs): status %d\n", rc); return 1; }
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
    printf("belief-find V %d C %d B %ld dtype %d: %ld mismatches, %ld codewords left to ufw\n", k.V,
           k.C, k.B, k.dtype, bad, unsolved);
    return bad != 0;
}

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: %s CASE_FILE...\n", argv[0]); return 2; }
    for (int a = 1; a < argc; ++a) {
        FILE* f = fopen(argv[a], "r");
        if (!f) { perror(argv[a]); return 2; }
        Case k;
        if (fscanf(f, "%d %d %d %ld %ld %d %d %la %d", &k.kind, &k.V, &k.C, &k.E, &k.B, &k.dtype,
                   &k.has_llr, &k.scale, &k.wmax) != 9)
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
            rc = k.dtype == GNND_F32 ? run_ufw<float>(f, k, var, chk) : run_ufw<double>(f, k, var, chk);
        else
            rc = k.dtype == GNND_F32 ? run_belief_find<float>(f, k, var, chk)
                                     : run_belief_find<double>(f, k, var, chk);
        fclose(f);
        if (rc) return rc;
    }
    return 0;
}

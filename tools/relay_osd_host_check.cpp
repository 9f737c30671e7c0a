// Stand-alone check of the soft relay and relay+OSD host mirrors
// (gnn-decode_amd/csrc/gnnd_relay_host.h) for host sanitizers: reads case files written by
// tools/relay_osd_host_sanitize.sh
//   V C E B dtype(0 f32 / 1 f64) legs iters0 iters_leg stop_after alpha beta soft base method
//   order, E edges "v c", B*N x values, legs*V gammas, B*V expected soft values, B*V expected llr
//   values, then B expected iteration counts, statuses, legs and solution counts
// (floating-point values as C99 hex literals: exact), runs gnnd_relay_soft_host_checked with every
// output and with the optional outputs null, compares soft / llr / the integers bit for bit with
// the file, then runs gnnd_relay_osd_host_checked and compares it with the soft mirror followed
// by gnnd_osd_gated_host_checked, with and without its optional outputs, and checks the
// guarantees: a solved codeword keeps relay's solution with choice -1, every status-0 estimate
// satisfies the syndrome.  Plain C++17, no HIP, no GPU.  Build with -ffp-contract=off.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../gnn-decode_amd/csrc/gnnd_relay_host.h"

struct Case {
    int V, C, dtype, legs, iters0, iters_leg, S, soft, base, method, order;
    long E, B;
    double alpha, beta;
    std::vector<int64_t> var, chk;
};

template <typename T>
static long differ(const std::vector<T>& a, const std::vector<T>& b) {
    return a.size() != b.size() || memcmp(a.data(), b.data(), a.size() * sizeof(T)) != 0;
}

template <typename T>
static int run(FILE* f, const Case& k) {
    const int V = k.V, C = k.C;
    const long B = k.B;
    const size_t BV = (size_t)B * V;
    std::vector<T> x((size_t)B * (V + C)), gam((size_t)k.legs * V);
    std::vector<T> pred(BV), soft(BV), ehat(BV), llr(BV), pred2(BV), ehat2(BV);
    std::vector<int32_t> ints[4];
    for (auto& a : ints) a.resize(B);
    double d;
    for (auto& v : x) { if (fscanf(f, "%la", &d) != 1) return 2; v = (T)d; }
    for (auto& v : gam) { if (fscanf(f, "%la", &d) != 1) return 2; v = (T)d; }
    const int64_t *var = k.var.data(), *chk = k.chk.data();
    int rc = gnnd_relay_soft_host_checked(var, chk, k.E, V, C, k.dtype, x.data(), gam.data(), k.legs,
                                          k.iters0, k.iters_leg, k.S, k.alpha, k.beta, k.soft,
                                          pred.data(), soft.data(), ehat.data(), llr.data(),
                                          ints[0].data(), ints[1].data(), ints[2].data(),
                                          ints[3].data(), B);
    if (rc != GNND_OK) { fprintf(stderr, "gnnd_relay_soft_host: status %d\n", rc); return 1; }
    rc = gnnd_relay_soft_host_checked(var, chk, k.E, V, C, k.dtype, x.data(), gam.data(), k.legs,
                                      k.iters0, k.iters_leg, k.S, k.alpha, k.beta, k.soft,
                                      pred2.data(), nullptr, ehat2.data(), nullptr, nullptr, nullptr,
                                      nullptr, nullptr, B);
    if (rc != GNND_OK) { fprintf(stderr, "gnnd_relay_soft_host (null outputs): status %d\n", rc); return 1; }
    long bad = differ(pred, pred2) + differ(ehat, ehat2);
    for (size_t i = 0; i < BV; ++i) {
        if (fscanf(f, "%la", &d) != 1) return 2;
        const T w = (T)d;
        bad += memcmp(&soft[i], &w, sizeof(T)) != 0;         // bit for bit: -0.0 is not 0.0
    }
    for (size_t i = 0; i < BV; ++i) {
        if (fscanf(f, "%la", &d) != 1) return 2;
        const T w = (T)d;
        bad += memcmp(&llr[i], &w, sizeof(T)) != 0;
        bad += ehat[i] != (w < T(0) ? T(1) : T(0));
    }
    int want;
    for (auto& a : ints)
        for (auto& v : a) { if (fscanf(f, "%d", &want) != 1) return 2; bad += v != want; }

    // the composition: the soft mirror's outputs through gnnd_osd_gated_host
    std::vector<T> o_ehat(BV), r_pred(BV), r_llr(BV), r_ehat(BV), n_pred(BV), n_llr(BV), n_ehat(BV);
    std::vector<int32_t> o_status(B), o_choice(B), r_ints[4], r_status(B), r_choice(B), n_gate(B),
        n_status(B);
    for (auto& a : r_ints) a.resize(B);
    rc = gnnd_osd_gated_host_checked(var, chk, k.E, V, C, k.dtype, x.data(), pred.data(), llr.data(),
                                     ints[1].data(), k.base, k.method, k.order, o_ehat.data(),
                                     o_status.data(), o_choice.data(), B);
    if (rc != GNND_OK) { fprintf(stderr, "gnnd_osd_gated_host: status %d\n", rc); return 1; }
    rc = gnnd_relay_osd_host_checked(var, chk, k.E, V, C, k.dtype, x.data(), gam.data(), k.legs,
                                     k.iters0, k.iters_leg, k.S, k.alpha, k.beta, k.soft, k.base,
                                     k.method, k.order, r_pred.data(), r_llr.data(),
                                     r_ints[0].data(), r_ints[1].data(), r_ints[2].data(),
                                     r_ints[3].data(), r_ehat.data(), r_status.data(),
                                     r_choice.data(), B);
    if (rc != GNND_OK) { fprintf(stderr, "gnnd_relay_osd_host: status %d\n", rc); return 1; }
    rc = gnnd_relay_osd_host_checked(var, chk, k.E, V, C, k.dtype, x.data(), gam.data(), k.legs,
                                     k.iters0, k.iters_leg, k.S, k.alpha, k.beta, k.soft, k.base,
                                     k.method, k.order, n_pred.data(), n_llr.data(), nullptr,
                                     n_gate.data(), nullptr, nullptr, n_ehat.data(), n_status.data(),
                                     nullptr, B);
    if (rc != GNND_OK) { fprintf(stderr, "gnnd_relay_osd_host (null outputs): status %d\n", rc); return 1; }
    bad += differ(r_pred, pred) + differ(r_llr, llr) + differ(r_ehat, o_ehat);
    bad += differ(r_status, o_status) + differ(r_choice, o_choice);
    for (int i = 0; i < 4; ++i) bad += differ(r_ints[i], ints[i]);
    bad += differ(n_pred, pred) + differ(n_llr, llr) + differ(n_ehat, o_ehat);
    bad += differ(n_gate, ints[1]) + differ(n_status, o_status);
    long gated = 0;
    for (long b = 0; b < B; ++b) {
        const T* e = &r_ehat[(size_t)b * V];
        if (r_ints[1][b] == 0) {                            // solved: relay's own solution
            bad += r_choice[b] != -1 || r_status[b] != 0;
            bad += memcmp(e, &ehat[(size_t)b * V], V * sizeof(T)) != 0;
        } else {
            ++gated;
        }
        if (r_status[b] != 0) continue;
        std::vector<int> par(C);
        for (int c = 0; c < C; ++c) par[c] = x[(size_t)b * (V + C) + V + c] < T(0);
        for (long i = 0; i < k.E; ++i) par[chk[i]] ^= e[var[i]] != T(0);
        for (int c = 0; c < C; ++c) bad += par[c];
    }
    printf("V %d C %d B %ld dtype %d legs %d iters %d/%d S %d soft %d: %ld gated, %ld mismatches\n",
           V, C, B, k.dtype, k.legs, k.iters0, k.iters_leg, k.S, k.soft, gated, bad);
    return bad != 0;
}

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: %s CASE_FILE...\n", argv[0]); return 2; }
    for (int a = 1; a < argc; ++a) {
        FILE* f = fopen(argv[a], "r");
        if (!f) { perror(argv[a]); return 2; }
        Case k;
        if (fscanf(f, "%d %d %ld %ld %d %d %d %d %d %la %la %d %d %d %d", &k.V, &k.C, &k.E, &k.B,
                   &k.dtype, &k.legs, &k.iters0, &k.iters_leg, &k.S, &k.alpha, &k.beta, &k.soft,
                   &k.base, &k.method, &k.order) != 15) return 2;
        k.var.resize(k.E);
        k.chk.resize(k.E);
        for (long e = 0; e < k.E; ++e) {
            long v, c;
            if (fscanf(f, "%ld %ld", &v, &c) != 2) return 2;
            k.var[e] = v;
            k.chk[e] = c;
        }
        const int rc = k.dtype == GNND_F32 ? run<float>(f, k) : run<double>(f, k);
        fclose(f);
        if (rc) return rc;
    }
    return 0;
}

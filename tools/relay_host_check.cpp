// Stand-alone check of the relay host mirror (gnn-decode_amd/csrc/gnnd_relay_host.h) for host
// sanitizers: reads case files written by tools/relay_host_sanitize.sh
//   V C E B dtype(0 f32 / 1 f64) legs iters0 iters_leg stop_after alpha beta, E edges "v c",
//   B*N x values, legs*V gammas, B*V expected llr values, then B expected iteration counts,
//   statuses, legs and solution counts
// (floating-point values as C99 hex literals: exact), runs gnnd_relay_host_checked with every
// output and with the optional outputs null, and compares bit for bit (ehat against llr < 0).
// Plain C++17, no HIP, no GPU.  Build with -ffp-contract=off (c * l + g * M is three roundings).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../gnn-decode_amd/csrc/gnnd_relay_host.h"

template <typename T>
static int run(FILE* f, int V, int C, long E, long B, int dtype, int legs, int iters0, int iters_leg,
               int S, double alpha, double beta, const std::vector<int64_t>& var,
               const std::vector<int64_t>& chk) {
    std::vector<T> x((size_t)B * (V + C)), gam((size_t)legs * V), ehat((size_t)B * V),
        llr((size_t)B * V), ehat2((size_t)B * V);
    std::vector<int32_t> ints[4];
    for (auto& a : ints) a.resize(B);
    double d;
    for (auto& v : x) { if (fscanf(f, "%la", &d) != 1) return 2; v = (T)d; }
    for (auto& v : gam) { if (fscanf(f, "%la", &d) != 1) return 2; v = (T)d; }
    int rc = gnnd_relay_host_checked(var.data(), chk.data(), E, V, C, dtype, x.data(), gam.data(),
                                     legs, iters0, iters_leg, S, alpha, beta, ehat.data(),
                                     llr.data(), ints[0].data(), ints[1].data(), ints[2].data(),
                                     ints[3].data(), B);
    if (rc != GNND_OK) { fprintf(stderr, "gnnd_relay_host: status %d\n", rc); return 1; }
    rc = gnnd_relay_host_checked(var.data(), chk.data(), E, V, C, dtype, x.data(), gam.data(), legs,
                                 iters0, iters_leg, S, alpha, beta, ehat2.data(), nullptr, nullptr,
                                 nullptr, nullptr, nullptr, B);
    if (rc != GNND_OK) { fprintf(stderr, "gnnd_relay_host (null outputs): status %d\n", rc); return 1; }
    long bad = memcmp(ehat.data(), ehat2.data(), ehat.size() * sizeof(T)) != 0;
    for (size_t i = 0; i < llr.size(); ++i) {
        if (fscanf(f, "%la", &d) != 1) return 2;
        const T w = (T)d;
        bad += memcmp(&llr[i], &w, sizeof(T)) != 0;          // bit for bit: -0.0 is not 0.0
        bad += ehat[i] != (w < T(0) ? T(1) : T(0));
    }
    int want;
    for (auto& a : ints)
        for (auto& v : a) { if (fscanf(f, "%d", &want) != 1) return 2; bad += v != want; }
    printf("V %d C %d B %ld dtype %d legs %d iters %d/%d S %d: %ld mismatches\n", V, C, B, dtype,
           legs, iters0, iters_leg, S, bad);
    return bad != 0;
}

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: %s CASE_FILE...\n", argv[0]); return 2; }
    for (int a = 1; a < argc; ++a) {
        FILE* f = fopen(argv[a], "r");
        if (!f) { perror(argv[a]); return 2; }
        int V, C, dtype, legs, iters0, iters_leg, S;
        long E, B;
        double alpha, beta;
        if (fscanf(f, "%d %d %ld %ld %d %d %d %d %d %la %la", &V, &C, &E, &B, &dtype, &legs, &iters0,
                   &iters_leg, &S, &alpha, &beta) != 11) return 2;
        std::vector<int64_t> var(E), chk(E);
        for (long e = 0; e < E; ++e) {
            long v, c;
            if (fscanf(f, "%ld %ld", &v, &c) != 2) return 2;
            var[e] = v;
            chk[e] = c;
        }
        const int rc = dtype == GNND_F32 ? run<float>(f, V, C, E, B, dtype, legs, iters0, iters_leg, S,
                                                      alpha, beta, var, chk)
                                         : run<double>(f, V, C, E, B, dtype, legs, iters0, iters_leg,
                                                       S, alpha, beta, var, chk);
        fclose(f);
        if (rc) return rc;
    }
    return 0;
}

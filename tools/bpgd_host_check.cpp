// Stand-alone check of the guided-decimation host mirror (gnn-decode_amd/csrc/gnnd_bpgd_host.h) for
// host sanitizers: reads case files written by tools/bpgd_host_sanitize.sh
//   V C E B dtype(0 f32 / 1 f64) iters0 iters_round rounds per_round pick clamp alpha beta,
//   E edges "v c", B*N x values, B*V expected llr values, then B expected iteration counts,
//   statuses and decimation counts
// (floating-point values as C99 hex literals: exact), runs gnnd_bpgd_host_checked with every output
// and with the optional outputs null, and compares bit for bit (ehat against llr < 0, pred only
// for being a probability).  Plain C++17, no HIP, no GPU.  Build with -ffp-contract=off (a * m - b
// is two roundings).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../gnn-decode_amd/csrc/gnnd_bpgd_host.h"

struct Case {
    int V, C, dtype, iters0, iters_round, rounds, per_round, pick;
    long E, B;
    double clamp, alpha, beta;
};

template <typename T>
static int run(FILE* f, const Case& k, const std::vector<int64_t>& var,
               const std::vector<int64_t>& chk) {
    const size_t nv = (size_t)k.B * k.V;
    std::vector<T> x((size_t)k.B * (k.V + k.C)), ehat(nv), llr(nv), pred(nv), ehat2(nv);
    std::vector<int32_t> ints[3];
    for (auto& a : ints) a.resize(k.B);
    double d;
    for (auto& v : x) { if (fscanf(f, "%la", &d) != 1) return 2; v = (T)d; }
    int rc = gnnd_bpgd_host_checked(var.data(), chk.data(), k.E, k.V, k.C, k.dtype, x.data(),
                                    k.alpha, k.beta, k.iters0, k.iters_round, k.rounds, k.per_round,
                                    k.pick, k.clamp, ehat.data(), llr.data(), pred.data(),
                                    ints[0].data(), ints[1].data(), ints[2].data(), k.B);
    if (rc != GNND_OK) { fprintf(stderr, "gnnd_bpgd_host: status %d\n", rc); return 1; }
    rc = gnnd_bpgd_host_checked(var.data(), chk.data(), k.E, k.V, k.C, k.dtype, x.data(), k.alpha,
                                k.beta, k.iters0, k.iters_round, k.rounds, k.per_round, k.pick,
                                k.clamp, ehat2.data(), nullptr, nullptr, nullptr, nullptr, nullptr,
                                k.B);
    if (rc != GNND_OK) { fprintf(stderr, "gnnd_bpgd_host (null outputs): status %d\n", rc); return 1; }
    long bad = memcmp(ehat.data(), ehat2.data(), nv * sizeof(T)) != 0;
    for (size_t i = 0; i < nv; ++i) {
        if (fscanf(f, "%la", &d) != 1) return 2;
        const T w = (T)d;
        bad += memcmp(&llr[i], &w, sizeof(T)) != 0;          // bit for bit: -0.0 is not 0.0
        bad += ehat[i] != (w < T(0) ? T(1) : T(0));
        bad += !(pred[i] >= T(0) && pred[i] <= T(1));
    }
    int want;
    long full = 0;
    for (int j = 0; j < 3; ++j)
        for (auto& v : ints[j]) {
            if (fscanf(f, "%d", &want) != 1) return 2;
            bad += v != want;
            full += j == 2 && v == k.V;
        }
    printf("V %d C %d B %ld dtype %d iters %d/%d rounds %d x %d pick %d: %ld mismatches, %ld "
           "codewords fully decimated\n", k.V, k.C, k.B, k.dtype, k.iters0, k.iters_round, k.rounds,
           k.per_round, k.pick, bad, full);
    return bad != 0;
}

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: %s CASE_FILE...\n", argv[0]); return 2; }
    for (int a = 1; a < argc; ++a) {
        FILE* f = fopen(argv[a], "r");
        if (!f) { perror(argv[a]); return 2; }
        Case k;
        if (fscanf(f, "%d %d %ld %ld %d %d %d %d %d %d %la %la %la", &k.V, &k.C, &k.E, &k.B,
                   &k.dtype, &k.iters0, &k.iters_round, &k.rounds, &k.per_round, &k.pick, &k.clamp,
                   &k.alpha, &k.beta) != 13) return 2;
        std::vector<int64_t> var(k.E), chk(k.E);
        for (long e = 0; e < k.E; ++e) {
            long v, c;
            if (fscanf(f, "%ld %ld", &v, &c) != 2) return 2;
            var[e] = v;
            chk[e] = c;
        }
        const int rc = k.dtype == GNND_F32 ? run<float>(f, k, var, chk) : run<double>(f, k, var, chk);
        fclose(f);
        if (rc) return rc;
    }
    return 0;
}

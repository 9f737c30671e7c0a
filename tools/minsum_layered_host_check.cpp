// Stand-alone check of the layered min-sum host mirror
// (gnn-decode_amd/csrc/gnnd_minsum_layered_host.h) for host sanitizers: reads case files written
// by tools/minsum_layered_host_sanitize.sh
//   V C E B dtype(0 f32 / 1 f64) alpha beta iters early_stop, E edges "v c", B*N x values,
//   B*V expected llr values, B expected iteration counts, B expected statuses
// (floating-point values as C99 hex literals: exact), runs gnnd_minsum_layered_host_checked with
// every output and with the optional outputs null, compares bit for bit, and runs
// gnnd_bposd_layered_host_checked on the same input (its llr / iteration counts / statuses are the
// min-sum stage's; every estimate with status 0 must satisfy the syndrome).  Plain C++17, no HIP,
// no GPU.  Build with -ffp-contract=off (the contract's a * m - b is two roundings).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../gnn-decode_amd/csrc/gnnd_minsum_layered_host.h"

template <typename T>
static int run(FILE* f, int V, int C, long E, long B, int dtype, double alpha, double beta,
               int iters, int early, const std::vector<int64_t>& var,
               const std::vector<int64_t>& chk) {
    std::vector<T> x((size_t)B * (V + C)), out((size_t)B * V), llr((size_t)B * V), out2((size_t)B * V);
    std::vector<int32_t> its(B), status(B);
    double d;
    for (auto& v : x) { if (fscanf(f, "%la", &d) != 1) return 2; v = (T)d; }
    int rc = gnnd_minsum_layered_host_checked(var.data(), chk.data(), E, V, C, dtype, x.data(), alpha, beta,
                                      iters, early, out.data(), llr.data(), its.data(),
                                      status.data(), B);
    if (rc != GNND_OK) { fprintf(stderr, "gnnd_minsum_layered_host: status %d\n", rc); return 1; }
    rc = gnnd_minsum_layered_host_checked(var.data(), chk.data(), E, V, C, dtype, x.data(), alpha, beta,
                                  iters, early, out2.data(), nullptr, nullptr, nullptr, B);
    if (rc != GNND_OK) { fprintf(stderr, "gnnd_minsum_layered_host (null outputs): status %d\n", rc); return 1; }
    long bad = memcmp(out.data(), out2.data(), out.size() * sizeof(T)) != 0;
    int want;
    for (auto& v : llr) {
        if (fscanf(f, "%la", &d) != 1) return 2;
        const T w = (T)d;
        bad += memcmp(&v, &w, sizeof(T)) != 0;              // bit for bit: -0.0 is not 0.0
    }
    for (auto& v : its) { if (fscanf(f, "%d", &want) != 1) return 2; bad += v != want; }
    for (auto& v : status) { if (fscanf(f, "%d", &want) != 1) return 2; bad += v != want; }
    // the one-call decoder: the same min-sum stage, then the gated OSD
    std::vector<T> pred((size_t)B * V), llr2((size_t)B * V), ehat((size_t)B * V);
    std::vector<int32_t> its2(B), bp(B), ost(B), choice(B);
    rc = gnnd_bposd_layered_host_checked(var.data(), chk.data(), E, V, C, dtype, x.data(), alpha,
                                         beta, iters, early, GNND_OSD_BASE_ZERO, GNND_OSD_CS, 10,
                                         pred.data(), llr2.data(), its2.data(), bp.data(),
                                         ehat.data(), ost.data(), choice.data(), B);
    if (rc != GNND_OK) { fprintf(stderr, "gnnd_bposd_layered_host: status %d\n", rc); return 1; }
    bad += memcmp(llr2.data(), llr.data(), llr.size() * sizeof(T)) != 0;
    bad += its2 != its;
    bad += bp != status;
    for (long b = 0; b < B; ++b) {
        if (ost[b] != 0) continue;
        std::vector<int> syn(C, 0);
        for (long e = 0; e < E; ++e)
            syn[chk[e]] ^= (int)(ehat[(size_t)b * V + var[e]] != T(0));
        for (int c = 0; c < C; ++c) bad += syn[c] != (int)(x[(size_t)b * (V + C) + V + c] < T(0));
    }
    printf("V %d C %d B %ld dtype %d alpha %g beta %g iters %d early %d: %ld mismatches\n", V, C, B,
           dtype, alpha, beta, iters, early, bad);
    return bad != 0;
}

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: %s CASE_FILE...\n", argv[0]); return 2; }
    for (int a = 1; a < argc; ++a) {
        FILE* f = fopen(argv[a], "r");
        if (!f) { perror(argv[a]); return 2; }
        int V, C, dtype, iters, early;
        long E, B;
        double alpha, beta;
        if (fscanf(f, "%d %d %ld %ld %d %la %la %d %d", &V, &C, &E, &B, &dtype, &alpha, &beta,
                   &iters, &early) != 9) return 2;
        std::vector<int64_t> var(E), chk(E);
        for (long e = 0; e < E; ++e) {
            long v, c;
            if (fscanf(f, "%ld %ld", &v, &c) != 2) return 2;
            var[e] = v;
            chk[e] = c;
        }
        const int rc = dtype == GNND_F32
                           ? run<float>(f, V, C, E, B, dtype, alpha, beta, iters, early, var, chk)
                           : run<double>(f, V, C, E, B, dtype, alpha, beta, iters, early, var, chk);
        fclose(f);
        if (rc) return rc;
    }
    return 0;
}

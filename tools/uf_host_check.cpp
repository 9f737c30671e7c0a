// Stand-alone check of the union-find host mirror (gnn-decode_amd/csrc/gnnd_uf_host.h) for host
// sanitizers: reads case files written by tools/uf_host_sanitize.sh
//   V C E B dtype(0 f32 / 1 f64) N, E edges "v c", 2 V expected endpoints, B*N x values (C99 hex
//   literals: exact), B*V expected ehat bits, then B expected rounds, statuses and full-edge counts,
// runs gnnd_graph_matching_host_checked and gnnd_uf_host_checked with every output, with the
// optional outputs null, and with a gate over sentinel-filled outputs, and compares exactly.
// Plain C++17, no HIP, no GPU.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../gnn-decode_amd/csrc/gnnd_uf_host.h"

struct Case {
    int V, C, dtype, N;
    long E, B;
};

template <typename T>
static int run(FILE* f, const Case& k, const std::vector<int64_t>& var,
               const std::vector<int64_t>& chk) {
    const size_t nv = (size_t)k.B * k.V;
    std::vector<T> x((size_t)k.B * (k.V + k.C)), ehat(nv), ehat2(nv), ehat3(nv, T(7));
    std::vector<int32_t> ints[3], gated[3], gate(k.B);
    for (auto& a : ints) a.resize(k.B);
    for (auto& a : gated) a.assign(k.B, 7);
    double d;
    for (auto& v : x) { if (fscanf(f, "%la", &d) != 1) return 2; v = (T)d; }
    int rc = gnnd_uf_host_checked(var.data(), chk.data(), k.E, k.V, k.C, k.dtype, x.data(), nullptr,
                                  ehat.data(), ints[0].data(), ints[1].data(), ints[2].data(), k.B);
    if (rc != GNND_OK) { fprintf(stderr, "gnnd_uf_host: status %d\n", rc); return 1; }
    rc = gnnd_uf_host_checked(var.data(), chk.data(), k.E, k.V, k.C, k.dtype, x.data(), nullptr,
                              ehat2.data(), nullptr, nullptr, nullptr, k.B);
    if (rc != GNND_OK) { fprintf(stderr, "gnnd_uf_host (null outputs): status %d\n", rc); return 1; }
    for (long b = 0; b < k.B; ++b) gate[b] = b % 3 == 1 ? 0 : (int32_t)(b + 1);
    rc = gnnd_uf_host_checked(var.data(), chk.data(), k.E, k.V, k.C, k.dtype, x.data(), gate.data(),
                              ehat3.data(), gated[0].data(), gated[1].data(), gated[2].data(), k.B);
    if (rc != GNND_OK) { fprintf(stderr, "gnnd_uf_host (gated): status %d\n", rc); return 1; }
    long bad = memcmp(ehat.data(), ehat2.data(), nv * sizeof(T)) != 0;
    for (long b = 0; b < k.B; ++b)
        for (int v = 0; v < k.V; ++v) {
            int want;
            if (fscanf(f, "%d", &want) != 1) return 2;
            const size_t i = (size_t)b * k.V + v;
            bad += ehat[i] != (T)want;
            bad += ehat3[i] != (gate[b] ? (T)want : T(7));
        }
    long unsolved = 0;
    for (int j = 0; j < 3; ++j)
        for (long b = 0; b < k.B; ++b) {
            int want;
            if (fscanf(f, "%d", &want) != 1) return 2;
            bad += ints[j][b] != want;
            bad += gated[j][b] != (gate[b] ? want : 7);
            unsolved += j == 1 && want != 0;
        }
    printf("V %d C %d N %d B %ld dtype %d: %ld mismatches, %ld codewords without a solution\n", k.V,
           k.C, k.N, k.B, k.dtype, bad, unsolved);
    return bad != 0;
}

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: %s CASE_FILE...\n", argv[0]); return 2; }
    for (int a = 1; a < argc; ++a) {
        FILE* f = fopen(argv[a], "r");
        if (!f) { perror(argv[a]); return 2; }
        Case k;
        if (fscanf(f, "%d %d %ld %ld %d %d", &k.V, &k.C, &k.E, &k.B, &k.dtype, &k.N) != 6) return 2;
        std::vector<int64_t> var(k.E), chk(k.E);
        for (long e = 0; e < k.E; ++e) {
            long v, c;
            if (fscanf(f, "%ld %ld", &v, &c) != 2) return 2;
            var[e] = v;
            chk[e] = c;
        }
        int32_t n = 0;
        std::vector<int32_t> ends(2 * (size_t)k.V);
        int rc = gnnd_graph_matching_host_checked(var.data(), chk.data(), k.E, k.V, k.C, &n,
                                                  ends.data());
        if (rc != GNND_OK || n != k.N) {
            fprintf(stderr, "gnnd_graph_matching_host: status %d, N %d (expected %d)\n", rc, n, k.N);
            return 1;
        }
        for (auto& got : ends) {
            int want;
            if (fscanf(f, "%d", &want) != 1) return 2;
            if (got != want) { fprintf(stderr, "endpoint mismatch in %s\n", argv[a]); return 1; }
        }
        rc = k.dtype == GNND_F32 ? run<float>(f, k, var, chk) : run<double>(f, k, var, chk);
        fclose(f);
        if (rc) return rc;
    }
    return 0;
}

// Stand-alone check of the OSD host mirror (gnn-decode_amd/csrc/gnnd_osd_host.h) for host
// sanitizers: reads one case file written by tools/osd_host_sanitize.sh
//   V C E B base dtype(0 f32 / 1 f64) method(0 osd0 / 1 cs / 2 e) order, E edges "v c",
//   B*N x values, B*V pred values, B*V expected ehat bits, B expected statuses, B expected choices
// runs gnnd_osd_host_checked (and for method 0 gnnd_osd0_host_checked as well) and compares bit
// for bit.  Plain C++17, no HIP, no GPU.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../gnn-decode_amd/csrc/gnnd_osd_host.h"

template <typename T>
static int run(FILE* f, int V, int C, long E, long B, int base, int dtype, int method, int order,
               const std::vector<int64_t>& var, const std::vector<int64_t>& chk) {
    std::vector<T> x((size_t)B * (V + C)), p((size_t)B * V), ehat((size_t)B * V);
    std::vector<int32_t> status(B), choice(B);
    double d;
    for (auto& v : x) { if (fscanf(f, "%lf", &d) != 1) return 2; v = (T)d; }
    for (auto& v : p) { if (fscanf(f, "%lf", &d) != 1) return 2; v = (T)d; }
    const int rc = gnnd_osd_host_checked(var.data(), chk.data(), E, V, C, dtype, x.data(), p.data(),
                                         base, method, order, ehat.data(), status.data(),
                                         choice.data(), B);
    if (rc != GNND_OK) { fprintf(stderr, "gnnd_osd_host: status %d\n", rc); return 1; }
    long bad = 0;
    int want;
    for (auto& v : ehat) { if (fscanf(f, "%d", &want) != 1) return 2; bad += v != (T)want; }
    for (auto& v : status) { if (fscanf(f, "%d", &want) != 1) return 2; bad += v != want; }
    for (auto& v : choice) { if (fscanf(f, "%d", &want) != 1) return 2; bad += v != want; }
    if (method == GNND_OSD_0) {         // the OSD-0 entry point and a null choice: the same bits
        std::vector<T> e0((size_t)B * V), e1((size_t)B * V);
        std::vector<int32_t> s0(B), s1(B);
        if (gnnd_osd0_host_checked(var.data(), chk.data(), E, V, C, dtype, x.data(), p.data(), base,
                                   e0.data(), s0.data(), B) != GNND_OK) return 1;
        if (gnnd_osd_host_checked(var.data(), chk.data(), E, V, C, dtype, x.data(), p.data(), base,
                                  method, order, e1.data(), s1.data(), nullptr, B) != GNND_OK) return 1;
        bad += e0 != ehat || s0 != status || e1 != ehat || s1 != status;
    }
    printf("V %d C %d B %ld base %d dtype %d method %d order %d: %ld mismatches\n", V, C, B, base,
           dtype, method, order, bad);
    return bad != 0;
}

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: %s CASE_FILE...\n", argv[0]); return 2; }
    for (int a = 1; a < argc; ++a) {
        FILE* f = fopen(argv[a], "r");
        if (!f) { perror(argv[a]); return 2; }
        int V, C, base, dtype, method, order;
        long E, B;
        if (fscanf(f, "%d %d %ld %ld %d %d %d %d", &V, &C, &E, &B, &base, &dtype, &method,
                   &order) != 8) return 2;
        std::vector<int64_t> var(E), chk(E);
        for (long e = 0; e < E; ++e) {
            long v, c;
            if (fscanf(f, "%ld %ld", &v, &c) != 2) return 2;
            var[e] = v;
            chk[e] = c;
        }
        const int rc =
            dtype == GNND_F32 ? run<float>(f, V, C, E, B, base, dtype, method, order, var, chk)
                         : run<double>(f, V, C, E, B, base, dtype, method, order, var, chk);
        fclose(f);
        if (rc) return rc;
    }
    return 0;
}

// Stand-alone check of the gated-OSD and BP+OSD host mirrors (gnn-decode_amd/csrc/gnnd_osd_host.h,
// gnnd_bposd_host.h) for host sanitizers: reads case files written by tools/bposd_host_sanitize.sh
//   G V C E B dtype(0 f32 / 1 f64) base method order has_llr, E edges "v c", B*N x values, B*V pred
//     values, B*V llr values (if has_llr), B gate values, then the expected B*V ehat (0 / 1), B
//     statuses and B choices of the numpy statement: gnnd_osd_gated_host_checked, with and without
//     the optional choice array, compared exactly;
//   P V C E B dtype base method order alpha beta iters early_stop, E edges, B*N x values, then the
//     expected B*V llr values, B iteration counts and B min-sum statuses: gnnd_bposd_host_checked;
//     llr / iters / bp_status compared bit for bit, and of the estimate (whose OSD stage orders by
//     the library's own soft output) the contract's guarantees: rows with bp_status 0 are
//     (llr < 0) with choice -1, and every row with status 0 satisfies the syndrome.
// (floating-point values as C99 hex literals: exact).  Plain C++17, no HIP, no GPU.  Build with
// -ffp-contract=off (the min-sum contract).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../gnn-decode_amd/csrc/gnnd_bposd_host.h"

template <typename T>
static bool read_values(FILE* f, std::vector<T>& v) {
    double d;
    for (auto& e : v) {
        if (fscanf(f, "%la", &d) != 1) return false;
        e = (T)d;
    }
    return true;
}

static bool read_ints(FILE* f, std::vector<int32_t>& v) {
    int d;
    for (auto& e : v) {
        if (fscanf(f, "%d", &d) != 1) return false;
        e = d;
    }
    return true;
}

template <typename T>
static int run_gated(FILE* f, int V, int C, long E, long B, int dtype, int base, int method,
                     int order, int has_llr, const std::vector<int64_t>& var,
                     const std::vector<int64_t>& chk) {
    std::vector<T> x((size_t)B * (V + C)), pred((size_t)B * V), llr(has_llr ? (size_t)B * V : 0);
    std::vector<T> ehat((size_t)B * V), ehat2((size_t)B * V);
    std::vector<int32_t> gate(B), status(B), status2(B), choice(B), w_e((size_t)B * V), w_s(B), w_c(B);
    if (!read_values(f, x) || !read_values(f, pred) || !read_values(f, llr) || !read_ints(f, gate) ||
        !read_ints(f, w_e) || !read_ints(f, w_s) || !read_ints(f, w_c))
        return 2;
    const T* lp = has_llr ? llr.data() : nullptr;
    int rc = gnnd_osd_gated_host_checked(var.data(), chk.data(), E, V, C, dtype, x.data(), pred.data(),
                                         lp, gate.data(), base, method, order, ehat.data(),
                                         status.data(), choice.data(), B);
    if (rc != GNND_OK) { fprintf(stderr, "gnnd_osd_gated_host: status %d\n", rc); return 1; }
    rc = gnnd_osd_gated_host_checked(var.data(), chk.data(), E, V, C, dtype, x.data(), pred.data(), lp,
                                     gate.data(), base, method, order, ehat2.data(), status2.data(),
                                     nullptr, B);
    if (rc != GNND_OK) { fprintf(stderr, "gnnd_osd_gated_host (no choice): status %d\n", rc); return 1; }
    long bad = memcmp(ehat.data(), ehat2.data(), ehat.size() * sizeof(T)) != 0;
    bad += memcmp(status.data(), status2.data(), status.size() * sizeof(int32_t)) != 0;
    for (size_t i = 0; i < ehat.size(); ++i) bad += ehat[i] != (T)w_e[i];
    for (long b = 0; b < B; ++b) bad += (status[b] != w_s[b]) + (choice[b] != w_c[b]);
    printf("gated V %d C %d B %ld dtype %d base %d method %d order %d llr %d: %ld mismatches\n", V, C,
           B, dtype, base, method, order, has_llr, bad);
    return bad != 0;
}

template <typename T>
static int run_bposd(FILE* f, int V, int C, long E, long B, int dtype, int base, int method,
                     int order, double alpha, double beta, int iters, int early,
                     const std::vector<int64_t>& var, const std::vector<int64_t>& chk) {
    const int N = V + C;
    std::vector<T> x((size_t)B * N), w_llr((size_t)B * V);
    std::vector<T> pred((size_t)B * V), llr((size_t)B * V), ehat((size_t)B * V);
    std::vector<int32_t> its(B), bp(B), status(B), choice(B), w_its(B), w_bp(B);
    if (!read_values(f, x) || !read_values(f, w_llr) || !read_ints(f, w_its) || !read_ints(f, w_bp))
        return 2;
    const int rc = gnnd_bposd_host_checked(var.data(), chk.data(), E, V, C, dtype, x.data(), alpha,
                                           beta, iters, early, base, method, order, pred.data(),
                                           llr.data(), its.data(), bp.data(), ehat.data(),
                                           status.data(), choice.data(), B);
    if (rc != GNND_OK) { fprintf(stderr, "gnnd_bposd_host: status %d\n", rc); return 1; }
    long bad = memcmp(llr.data(), w_llr.data(), llr.size() * sizeof(T)) != 0;   // -0.0 is not 0.0
    for (long b = 0; b < B; ++b) bad += (its[b] != w_its[b]) + (bp[b] != w_bp[b]);
    for (long b = 0; b < B; ++b) {
        if (bp[b] == 0) {
            bad += choice[b] != -1 || status[b] != 0;
            for (int v = 0; v < V; ++v) bad += ehat[b * V + v] != (llr[b * V + v] < T(0) ? T(1) : T(0));
        }
        if (status[b] != 0) continue;
        std::vector<int> par(C);
        for (int c = 0; c < C; ++c) par[c] = x[b * N + V + c] < T(0);
        for (long e = 0; e < E; ++e) par[chk[e]] ^= ehat[b * V + var[e]] != T(0);
        for (int c = 0; c < C; ++c) bad += par[c];
    }
    printf("bposd V %d C %d B %ld dtype %d base %d method %d order %d: %ld mismatches\n", V, C, B,
           dtype, base, method, order, bad);
    return bad != 0;
}

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: %s CASE_FILE...\n", argv[0]); return 2; }
    for (int a = 1; a < argc; ++a) {
        FILE* f = fopen(argv[a], "r");
        if (!f) { perror(argv[a]); return 2; }
        char kind;
        int V, C, dtype, base, method, order;
        long E, B;
        if (fscanf(f, " %c %d %d %ld %ld %d %d %d %d", &kind, &V, &C, &E, &B, &dtype, &base, &method,
                   &order) != 9) return 2;
        int has_llr = 0, iters = 0, early = 0;
        double alpha = 0, beta = 0;
        if (kind == 'G') {
            if (fscanf(f, "%d", &has_llr) != 1) return 2;
        } else if (kind != 'P' || fscanf(f, "%la %la %d %d", &alpha, &beta, &iters, &early) != 4) {
            return 2;
        }
        std::vector<int64_t> var(E), chk(E);
        for (long e = 0; e < E; ++e) {
            long v, c;
            if (fscanf(f, "%ld %ld", &v, &c) != 2) return 2;
            var[e] = v;
            chk[e] = c;
        }
        int rc;
        if (kind == 'G')
            rc = dtype == GNND_F32
                     ? run_gated<float>(f, V, C, E, B, dtype, base, method, order, has_llr, var, chk)
                     : run_gated<double>(f, V, C, E, B, dtype, base, method, order, has_llr, var, chk);
        else
            rc = dtype == GNND_F32 ? run_bposd<float>(f, V, C, E, B, dtype, base, method, order, alpha,
                                                      beta, iters, early, var, chk)
                                   : run_bposd<double>(f, V, C, E, B, dtype, base, method, order,
                                                       alpha, beta, iters, early, var, chk);
        fclose(f);
        if (rc) return rc;
    }
    return 0;
}

// gnnd_graph.hip — single-codeword Tanner graph descriptor + misc C-ABI entry points.
//
// The reference rebuilds a batched int64 edge_index per batch (PyG collation,
// quantum/decoder_v2_4.py:161-183, 205-206) and re-reads it in every scatter/gather
// (:136-144).  Every codeword shares one H, so libgnnd keeps ONE small CSR/CSC of H
// (quantum/decoder_v2_4.py:164-165: H.to_sparse()._indices(), sorted by (v, c)) and the
// kernels derive batched node/edge ids in closed form.
#include "gnnd_common.h"
#include "gnnd_minsum_layered_host.h"   // the layer rule (gnnd_layers_build), shared with the mirror
#include "gnnd_uf_host.h"               // the decoding-graph rule (gnnd_uf_graph_build), likewise
#include <stdlib.h>
#include <string.h>
#include <vector>
#include <algorithm>
#include <cmath>
#include <cstdio>

static thread_local int g_last_hip_error = 0;

int set_hip_error(hipError_t e) {
    g_last_hip_error = (int)e;
    return GNND_ERR_HIP;
}

extern "C" int gnnd_last_hip_error(void) { return g_last_hip_error; }

GNND_DEBUG_TU(graph)

extern "C" int gnnd_version(void) { return GNND_VERSION; }

extern "C" const char* gnnd_status_string(int s) {
    switch (s) {
        case GNND_OK: return "ok";
        case GNND_ERR_INVALID_ARG: return "invalid argument";
        case GNND_ERR_HIP: return "HIP runtime error";
        case GNND_ERR_UNSUPPORTED: return "unsupported configuration";
        case GNND_ERR_GRAPH: return "invalid Tanner graph (edges must be unique and sorted by (v, c))";
        case GNND_ERR_ALLOC: return "device allocation failed";
        default: return "unknown status";
    }
}

namespace {

struct SlotPlan {
    int G = 0, R = 0, padded = 0, padr = 0;
    std::vector<uint32_t> slot, slot_ve;
    std::vector<int> vslot;
};
struct Layout {
    bool ok = false;
    int P = 0;
    std::vector<int> vlay, slot;     // [2V] {v | dpad << 16, pos}, [nsr] v | pos << 16
    int ts = 0;                      // x layouts: T row stride and positions (place_t_rows);
    std::vector<int> tpos;           // vlay .y high half and slot low half hold tpos(v)
};
// everything gnnd_graph_create uploads, built on the host (also checked by
// gnnd_graph_validate_host without a device)
struct HostTables {
    int V = 0, C = 0, E = 0, max_dv = 0, max_dc = 0, min_dc = 0, nints = 0, ord_off = 0, nsr = 0;
    int plan_off[3] = {0, 0, 0};
    SlotPlan plans[3];
    Layout lays[7], laysx[7];
    int lay_off[7] = {0}, layx_off[7] = {0};
    std::vector<int> table;
};

// GNND_NO_SLOT_SPREAD=1: the x-augmented layouts keep the slot plan's edge order (A/B)
bool slot_spread_disabled() {
    static bool v = [] {
        const char* e = gnnd_tune_env("GNND_NO_SLOT_SPREAD");
        return e && e[0] == '1';
    }();
    return v;
}

// LDS bank spreading of the register-resident kernel's message stores (decode_resident_kernel
// on an x-augmented layout for a tile of cw codewords).  Work item f = (c * cw + b) * G + g
// (check c, codeword b, group lane g); a 32-lane half of a wave is one LDS bank group, and the
// check step stores slot r of its items with one ds_write_b32 at b * P1 + pos(edge) (padding
// slots at the spare position P).  Cycles of a group = distinct addresses on its busiest bank
// (32 banks, MI355X_MICROARCH.md §LDS).  A check's edges may sit in any of its real slots: the
// variable sums keep edge order and the check sum is the same sum in another order, so each
// check's edges are redistributed over its slot rows r by a deterministic annealing (fixed
// seed: the same tables for the same graph) that minimises the summed cycles.  BCH(63,45),
// cw = 16: 648 -> ~490 store cycles per tile iteration (tools/t_perm.py models the same).
// slot[c * G * R + k] = v | pos << 16 for k < deg(c); padding (k >= deg) stays trailing.
void spread_check_slots(int C, int G, int R, int cw, int P, const std::vector<int>& cdeg,
                        std::vector<int>& slot) {
    const int GR = G * R, P1 = (P + 1) | 1;
    const long items = (long)C * cw * G;
    const int nh = (int)((items + 31) / 32);
    if (nh <= 0 || cw < 1) return;
    // group (h, r): lanes f in [32 h, 32 h + 32) of slot row r
    std::vector<std::vector<int>> cr_groups((size_t)C * R);     // (c, r) -> groups containing it
    for (int h = 0; h < nh; ++h) {
        int last = -1;
        for (int f = 32 * h; f < 32 * h + 32 && f < items; ++f) {
            const int c = (f / G) / cw;
            if (c == last) continue;
            last = c;
            for (int r = 0; r < R; ++r) cr_groups[(size_t)c * R + r].push_back(h * R + r);
        }
    }
    auto group_cost = [&](int grp) {
        const int h = grp / R, r = grp % R;
        int addr[32], n = 0;
        for (int f = 32 * h; f < 32 * h + 32 && f < items; ++f) {
            const int gi = f / G, g = f % G, c = gi / cw, b = gi % cw;
            const int k = g * R + r;
            const int pos = k < cdeg[c] ? (int)((uint32_t)slot[(size_t)c * GR + k] >> 16) : P;
            const int a = b * P1 + pos;
            bool dup = false;
            for (int i = 0; i < n && !dup; ++i) dup = addr[i] == a;
            if (!dup) addr[n++] = a;
        }
        int cnt[32] = {0}, m = 0;
        for (int i = 0; i < n; ++i) m = std::max(m, ++cnt[addr[i] & 31]);
        return m;
    };
    std::vector<int> gcost((size_t)nh * R);
    long cur = 0;
    for (int i = 0; i < nh * R; ++i) cur += gcost[i] = group_cost(i);
    const long init_cost = cur;
    std::vector<int> best = slot;
    long bestc = cur;
    uint64_t s = 0x9E3779B97F4A7C15ull;
    auto rnd = [&](uint64_t n) {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        return (uint64_t)(s >> 33) % n;
    };
    // (bounded: graph creation stays in the milliseconds for the framework's codes)
    const long iters = std::min(20L * C * GR, 20000L);
    std::vector<int> touched, nc;
    for (long it = 0; it < iters; ++it) {
        const int c = (int)rnd(C), d = cdeg[c];
        if (d < 2) continue;
        const int k1 = (int)rnd(d), k2 = (int)rnd(d);
        if (k1 % R == k2 % R) continue;                  // same slot row: same costs
        const size_t base = (size_t)c * GR;
        std::swap(slot[base + k1], slot[base + k2]);
        touched.clear();
        for (int r : {k1 % R, k2 % R})
            for (int grp : cr_groups[(size_t)c * R + r]) touched.push_back(grp);
        long delta = 0;
        nc.resize(touched.size());
        for (size_t i = 0; i < touched.size(); ++i) {
            nc[i] = group_cost(touched[i]);
            delta += nc[i] - gcost[touched[i]];
        }
        const double temp = 2.0 * (1.0 - (double)it / iters) + 0.05;
        const double u = (double)rnd(1u << 30) / (double)(1u << 30);
        if (delta <= 0 || u < exp(-(double)delta / temp)) {
            for (size_t i = 0; i < touched.size(); ++i) gcost[touched[i]] = nc[i];
            cur += delta;
            if (cur < bestc) { bestc = cur; best = slot; }
        } else {
            std::swap(slot[base + k1], slot[base + k2]);
        }
    }
    slot = best;
    static const bool log = [] {
        const char* e = gnnd_tune_env("GNND_SLOT_SPREAD_LOG");
        return e && e[0] == '1';
    }();
    if (log) {
        fprintf(stderr, "gnnd slot spread: C=%d G=%d R=%d cw=%d P1=%d store cycles per tile "
                        "iteration %ld -> %ld\n", C, G, R, cw, P1, init_cost, bestc);
    }
}

// GNND_NO_TPERM=1: the x layouts keep T rows in variable order (ts = V, tpos(v) = v) (A/B)
bool tperm_disabled() {
    static bool v = [] {
        const char* e = gnnd_tune_env("GNND_NO_TPERM");
        return e && e[0] == '1';
    }();
    return v;
}

// Placement of the resident fp32 kernel's T rows (T_v of codeword b at b * ts + tpos(v)) for
// a tile of cw codewords, after spread_check_slots fixed the slot rows: the check step gathers
// T_v of slot row r with one ds_read_b32 per item round (lanes f = (c * cw + b) * G + g), the
// variable step writes T_v of 256 / cw consecutive var_ord entries x cw codewords per row of
// lanes (lane t: codeword t % cw, entry t / cw).  Cycles of a 32-lane group = distinct
// addresses on its busiest bank.  For each candidate stride (V, and the next ones = 8, 24, 16
// mod 32 and odd) a deterministic annealing over the positions (swaps, moves into free
// positions) minimises the summed cycles; the best stride wins (ties: the smaller).
// BCH(63,45), cw = 16: gathers 432 -> ~350, writes ~63 -> ~70 cycles per tile iteration.
void place_t_rows(int C, int G, int R, int cw, int V, const std::vector<int>& vord,
                  const std::vector<int>& cdeg, const std::vector<int>& slot, int& ts_out,
                  std::vector<int>& tpos_out) {
    const int GR = G * R;
    const long items = (long)C * cw * G;
    const int nh = (int)((items + 31) / 32);
    // groups: (stride b, variable) lanes; gathers then variable-step writes
    std::vector<std::vector<std::pair<int, int>>> grp;
    for (int h = 0; h < nh; ++h)
        for (int r = 0; r < R; ++r) {
            std::vector<std::pair<int, int>> L;
            for (int f = 32 * h; f < 32 * h + 32 && f < items; ++f) {
                const int gi = f / G, g = f % G, c = gi / cw, b = gi % cw, k = g * R + r;
                const int v = k < cdeg[c] ? (slot[(size_t)c * GR + k] & 0xffff) : 0;
                L.push_back({b, v});
            }
            grp.push_back(L);
        }
    if (cw <= 32 && 256 % cw == 0) {
        const int per = 256 / cw;                       // var_ord entries per block row
        for (int i0 = 0; i0 < V; i0 += per)
            for (int h = 0; h < 8; ++h) {               // 8 half-waves of the 256 lanes
                std::vector<std::pair<int, int>> L;
                for (int t = 32 * h; t < 32 * h + 32; ++t) {
                    const int i = i0 + t / cw;
                    if (i < V) L.push_back({t % cw, vord[i]});
                }
                if (!L.empty()) grp.push_back(L);
            }
    }
    const int ng = (int)grp.size();
    std::vector<std::vector<int>> of_var(V);
    for (int q = 0; q < ng; ++q) {
        int last = -1;
        std::vector<int> vs;
        for (auto& bv : grp[q]) vs.push_back(bv.second);
        std::sort(vs.begin(), vs.end());
        for (int v : vs)
            if (v != last) { of_var[v].push_back(q); last = v; }
    }
    auto cost_of = [&](int q, int ts, const std::vector<int>& tp) {
        int addr[32], n = 0;
        for (auto& bv : grp[q]) {
            const int a = bv.first * ts + tp[bv.second];
            bool dup = false;
            for (int i = 0; i < n && !dup; ++i) dup = addr[i] == a;
            if (!dup) addr[n++] = a;
        }
        int cnt[32] = {0}, m = 0;
        for (int i = 0; i < n; ++i) m = std::max(m, ++cnt[addr[i] & 31]);
        return m;
    };
    std::vector<int> cands = {V};
    for (int want : {8, 24, 1}) {
        int t = V + 1;
        while (want == 1 ? (t % 2 == 0) : (t % 32 != want)) ++t;
        cands.push_back(t);
    }
    long best_total = -1;
    for (int ts : cands) {
        std::vector<int> tp(V), pos_owner(ts, -1);
        for (int v = 0; v < V; ++v) { tp[v] = v; pos_owner[v] = v; }
        std::vector<int> gc(ng);
        long cur = 0;
        for (int q = 0; q < ng; ++q) cur += gc[q] = cost_of(q, ts, tp);
        long bestc = cur;
        std::vector<int> best = tp;
        uint64_t s = 0x2545F4914F6CDD1Dull ^ (uint64_t)ts;
        auto rnd = [&](uint64_t n) {
            s = s * 6364136223846793005ull + 1442695040888963407ull;
            return (uint64_t)(s >> 33) % n;
        };
        const long iters = std::min(40L * V, 10000L);
        std::vector<int> touched, nc;
        for (long it = 0; it < iters; ++it) {
            const int a = (int)rnd(V);
            const int p2 = (int)rnd(ts);                 // target position: swap with its owner
            const int b = pos_owner[p2];
            if (b == a) continue;
            const int pa = tp[a];
            tp[a] = p2;
            if (b >= 0) tp[b] = pa;
            touched.clear();
            for (int q : of_var[a]) touched.push_back(q);
            if (b >= 0) for (int q : of_var[b]) touched.push_back(q);
            std::sort(touched.begin(), touched.end());
            touched.erase(std::unique(touched.begin(), touched.end()), touched.end());
            long delta = 0;
            nc.resize(touched.size());
            for (size_t i = 0; i < touched.size(); ++i) {
                nc[i] = cost_of(touched[i], ts, tp);
                delta += nc[i] - gc[touched[i]];
            }
            const double temp = 2.0 * (1.0 - (double)it / iters) + 0.05;
            const double u = (double)rnd(1u << 30) / (double)(1u << 30);
            if (delta <= 0 || u < exp(-(double)delta / temp)) {
                for (size_t i = 0; i < touched.size(); ++i) gc[touched[i]] = nc[i];
                cur += delta;
                pos_owner[p2] = a;
                pos_owner[pa] = b;
                if (cur < bestc) { bestc = cur; best = tp; }
            } else {
                tp[a] = pa;
                if (b >= 0) tp[b] = p2;
            }
        }
        if (best_total < 0 || bestc < best_total) {
            best_total = bestc;
            ts_out = ts;
            tpos_out = best;
        }
    }
    static const bool log = [] {
        const char* e = gnnd_tune_env("GNND_SLOT_SPREAD_LOG");
        return e && e[0] == '1';
    }();
    if (log) {
        std::vector<int> id(V);
        for (int v = 0; v < V; ++v) id[v] = v;
        long c0 = 0;
        for (int q = 0; q < ng; ++q) c0 += cost_of(q, V, id);
        fprintf(stderr, "gnnd t rows: C=%d G=%d R=%d cw=%d gather+write cycles per tile iteration "
                        "%ld (ts = V) -> %ld (ts = %d)\n", C, G, R, cw, c0, best_total, ts_out);
    }
}

int build_tables(const int64_t* h_var, const int64_t* h_chk, int64_t num_edges, int32_t V,
                 int32_t C, HostTables& T) {
    if (!h_var || !h_chk || num_edges <= 0 || V <= 0 || C <= 0) return GNND_ERR_INVALID_ARG;
    // 16-bit packing of v, c and edge ids (E itself marks padding); bounds every degree
    if (V > 65535 || C > 65535 || num_edges > 65535) return GNND_ERR_UNSUPPORTED;
    const int E = (int)num_edges;
    std::vector<uint32_t> evc(E);
    std::vector<int> vptr(V + 1, 0), cptr(C + 1, 0), cedge(E);
    for (int e = 0; e < E; ++e) {
        int64_t v = h_var[e], c = h_chk[e];
        if (v < 0 || v >= V || c < 0 || c >= C) return GNND_ERR_GRAPH;
        if (e > 0) {   // strictly increasing (v, c): coalesced sparse-index order
            int64_t pv = h_var[e - 1], pc = h_chk[e - 1];
            if (v < pv || (v == pv && c <= pc)) return GNND_ERR_GRAPH;
        }
        evc[e] = (uint32_t)v | ((uint32_t)c << 16);
        vptr[v + 1]++;
        cptr[c + 1]++;
    }
    int max_dv = 0, max_dc = 0;
    for (int v = 0; v < V; ++v) { max_dv = vptr[v + 1] > max_dv ? vptr[v + 1] : max_dv; vptr[v + 1] += vptr[v]; }
    int min_dc = C > 0 ? cptr[1] : 0;
    for (int c = 0; c < C; ++c) {
        max_dc = cptr[c + 1] > max_dc ? cptr[c + 1] : max_dc;
        min_dc = cptr[c + 1] < min_dc ? cptr[c + 1] : min_dc;
        cptr[c + 1] += cptr[c];
    }
    {
        std::vector<int> fill(cptr.begin(), cptr.end() - 1);
        for (int e = 0; e < E; ++e) cedge[fill[h_chk[e]]++] = e;   // increasing e per check
    }
    // check-group plans: R slots per lane, G (power of two) lanes per check, minimal padding.
    // Two tie-breaks between equal-slot plans: the streaming kernel prefers the smaller R
    // (more lanes per check: V24's heavy per-edge MLPs spread over more lanes; measured
    // toric-5 V24 fp32 5.1 vs 4.8 M cw/s), the register-resident kernel the larger R (fewer
    // butterfly steps per edge: toric QGNNI 147 -> 159 M cw/s, LDPC CGNNI 12.7 -> 13.9 M).
    // GNND_GROUP_R forces R in both (tuning sweeps) when it yields G <= 64.
    static const int force_r = [] {
        const char* e = gnnd_tune_env("GNND_GROUP_R");
        return e ? atoi(e) : 0;
    }();
    // tie preference: 0 = smaller R, 1 = larger R, 2 = R = 2 (the paired-edge fp32 V24
    // path at small batches: one edge pair per lane, most lanes per codeword)
    auto build_plan = [&](int pref, SlotPlan& sp) -> bool {
        long best = -1;
        for (int R = 1; R <= 4; ++R) {
            int need = (max_dc + R - 1) / R, G = 1;
            while (G < need) G <<= 1;
            if (G > 64) continue;
            long slots = (long)C * G * R;
            if (force_r == R) { best = slots; sp.G = G; sp.R = R; break; }
            const bool tie_wins = pref == 1 || (pref == 2 && R == 2);
            if (best < 0 || slots < best || (tie_wins && slots == best)) {
                best = slots; sp.G = G; sp.R = R;
            }
        }
        if (best < 0) return false;     // check degree > 256
        const int ns = C * sp.G * sp.R;
        sp.slot.assign(ns, GNND_SLOT_PAD);
        sp.slot_ve.assign(ns, (uint32_t)E << 16);   // padding: v 0, dummy edge E
        sp.vslot.assign(E, 0);
        sp.padded = 0;
        for (int c = 0; c < C; ++c) {
            sp.padded |= (cptr[c + 1] - cptr[c]) != sp.G * sp.R;
            sp.padr = std::max(sp.padr, std::min(sp.R, sp.G * sp.R - (cptr[c + 1] - cptr[c])));
            for (int k = cptr[c], i = 0; k < cptr[c + 1]; ++k, ++i) {
                int e = cedge[k];
                int pos = c * sp.G * sp.R + i;
                sp.slot[pos] = evc[e] & 0xffffu;
                sp.slot_ve[pos] = (evc[e] & 0xffffu) | ((uint32_t)e << 16);
                sp.vslot[e] = pos;
            }
        }
        return true;
    };
    SlotPlan* plans = T.plans;
    for (int i = 0; i < 3; ++i)
        if (!build_plan(i, plans[i])) return GNND_ERR_UNSUPPORTED;

    std::vector<int> vord(V);
    for (int v = 0; v < V; ++v) vord[v] = v;
    std::stable_sort(vord.begin(), vord.end(), [&](int a, int b) {
        return vptr[a + 1] - vptr[a] < vptr[b + 1] - vptr[b];
    });

    const int nints = graph_table_ints(V, C, E);
    int* plan_off = T.plan_off;
    int off = nints;
    for (int i = 0; i < 3; ++i) {
        plan_off[i] = off;
        off += 2 * (int)plans[i].slot.size() + E;
    }
    const int ord_off = (off + 1) & ~1;     // uint2 alignment
    // padded variable-major message layouts of the resident kernel (GraphView::vlay), one per
    // wave group size 2^i, i = 1..6: groups of 2^i consecutive var_ord entries share the
    // group's largest degree; positions run in var_ord order.  The x-augmented variants
    // (i = 0..6) give every variable one more position after its padded messages for x_v.
    const int nsr = (int)plans[1].slot.size();
    auto build_layout = [&](int gs, bool with_x, Layout& L) {
        std::vector<int> epos(E);
        L.vlay.assign(2 * V, 0);
        int pos = 0;
        for (int j0 = 0; j0 < V; j0 += gs) {
            const int j1 = std::min(V, j0 + gs);
            int dpad = 0;
            for (int j = j0; j < j1; ++j) dpad = std::max(dpad, vptr[vord[j] + 1] - vptr[vord[j]]);
            if (with_x) ++dpad;              // the x_v position, last in the variable's run
            for (int j = j0; j < j1; ++j) {
                const int v = vord[j];
                L.vlay[2 * j] = v | (dpad << 16);
                L.vlay[2 * j + 1] = pos;
                for (int e = vptr[v]; e < vptr[v + 1]; ++e) epos[e] = pos + (e - vptr[v]);
                pos += dpad;
            }
        }
        L.P = pos;
        if (pos >= 65535) return;            // positions travel in 16 bits
        L.ok = true;
        L.slot.assign(nsr, pos << 16);       // padding: variable 0, the spare position P
        for (int k = 0; k < nsr; ++k) {
            const uint32_t sv = plans[1].slot_ve[k];
            const int e = (int)(sv >> 16);
            if (e < E) L.slot[k] = (int)(sv & 0xffffu) | (epos[e] << 16);
        }
        // x-augmented layouts of the register-resident fp32 kernel (tiles of cw = 64 / gs
        // codewords): each check's edges over its slot rows for conflict-free-er message stores
        // (group sizes the register-resident kernel instantiates: G <= 16)
        // (tiles the plan can take: cw * C * G items within kResidentQ's largest 12 per lane)
        const bool tile_ok = (long)(64 / gs) * C * plans[1].G <= 12L * 256;
        if (with_x && gs >= 2 && gs <= 32 && plans[1].G <= 16 && tile_ok && !slot_spread_disabled()) {
            std::vector<int> cdeg(C);
            for (int c = 0; c < C; ++c) cdeg[c] = cptr[c + 1] - cptr[c];
            spread_check_slots(C, plans[1].G, plans[1].R, 64 / gs, pos, cdeg, L.slot);
        }
        L.ts = V;
        L.tpos.resize(V);
        for (int v = 0; v < V; ++v) L.tpos[v] = v;
        if (with_x && gs >= 2 && gs <= 32 && plans[1].G <= 16 && tile_ok && !tperm_disabled()) {
            std::vector<int> cdeg(C), vo(V);
            for (int c = 0; c < C; ++c) cdeg[c] = cptr[c + 1] - cptr[c];
            for (int j = 0; j < V; ++j) vo[j] = L.vlay[2 * j] & 0xffff;
            place_t_rows(C, plans[1].G, plans[1].R, 64 / gs, V, vo, cdeg, L.slot, L.ts, L.tpos);
        }
        if (with_x) {       // positions travel in 16 bits: ts <= 65535
            for (int j = 0; j < V; ++j) L.vlay[2 * j + 1] |= L.tpos[L.vlay[2 * j] & 0xffff] << 16;
            for (int k = 0; k < nsr; ++k)
                L.slot[k] = (L.slot[k] & ~0xffff) | L.tpos[L.slot[k] & 0xffff];
        }
    };
    Layout* lays = T.lays;
    Layout* laysx = T.laysx;
    int* lay_off = T.lay_off;
    int* layx_off = T.layx_off;
    off = ord_off + 2 * V;
    for (int i = 0; i < 7; ++i) {
        for (int x = 0; x < 2; ++x) {
            if (i == 0 && !x) continue;      // identity layout: positions = edge ids
            Layout& L = x ? laysx[i] : lays[i];
            build_layout(1 << i, x != 0, L);
            if (!L.ok) continue;
            (x ? layx_off : lay_off)[i] = off;
            off = (off + 2 * V + nsr + 1) & ~1;  // uint2 alignment of the next layout
        }
    }
    std::vector<int>& table = T.table;
    table.assign(off, 0);
    memcpy(table.data(), evc.data(), sizeof(int) * E);
    memcpy(table.data() + E, vptr.data(), sizeof(int) * (V + 1));
    memcpy(table.data() + E + V + 1, cptr.data(), sizeof(int) * (C + 1));
    memcpy(table.data() + E + V + 1 + C + 1, cedge.data(), sizeof(int) * E);
    for (int i = 0; i < 3; ++i) {
        const int ns = (int)plans[i].slot.size();
        memcpy(table.data() + plan_off[i], plans[i].slot.data(), sizeof(int) * ns);
        memcpy(table.data() + plan_off[i] + ns, plans[i].vslot.data(), sizeof(int) * E);
        memcpy(table.data() + plan_off[i] + ns + E, plans[i].slot_ve.data(), sizeof(int) * ns);
    }
    for (int i = 0; i < V; ++i) {
        const int v = vord[i];
        table[ord_off + 2 * i] = v | ((vptr[v + 1] - vptr[v]) << 16);
        table[ord_off + 2 * i + 1] = vptr[v];
    }
    for (int i = 0; i < 7; ++i)
        for (int x = 0; x < 2; ++x) {
            const Layout& L = x ? laysx[i] : lays[i];
            if (!L.ok) continue;
            const int o = (x ? layx_off : lay_off)[i];
            memcpy(table.data() + o, L.vlay.data(), sizeof(int) * 2 * V);
            memcpy(table.data() + o + 2 * V, L.slot.data(), sizeof(int) * nsr);
        }

    T.V = V; T.C = C; T.E = E; T.max_dv = max_dv; T.max_dc = max_dc; T.min_dc = min_dc;
    T.nints = nints; T.ord_off = ord_off; T.nsr = nsr;
    return GNND_OK;
}

// Structural invariants of the host tables (the device kernels index with them unchecked):
// every edge sits in exactly one slot of its check, in edge order, padding trailing; every
// layout gives each variable a disjoint run holding its edges first (then zero padding and,
// for the x-augmented layouts, the x_v position last), and its slot table points at them.
int check_tables(const HostTables& T, int32_t* report) {
    const int E = T.E, V = T.V, C = T.C;
    const std::vector<int>& t = T.table;
    const int* vptr = t.data() + E;
    const int* cptr = vptr + V + 1;
    const int* cedge = cptr + C + 1;
    int fails = 0, nlay = 0;
    for (int p = 0; p < 3; ++p) {
        const SlotPlan& sp = T.plans[p];
        const int GR = sp.G * sp.R;
        if ((int)sp.slot_ve.size() != C * GR) { ++fails; continue; }
        for (int c = 0; c < C; ++c) {
            const int deg = cptr[c + 1] - cptr[c];
            if (deg > GR) ++fails;
            for (int i = 0; i < GR; ++i) {
                const int e = (int)(sp.slot_ve[c * GR + i] >> 16);
                if (i < deg) {
                    if (e != cedge[cptr[c] + i] || sp.vslot[e] != c * GR + i) ++fails;
                    if ((int)(sp.slot_ve[c * GR + i] & 0xffffu) != (int)(t[e] & 0xffff)) ++fails;
                } else if (e != E) {
                    ++fails;
                }
            }
            // lanes fill in order: a lane's padding is trailing and at most padr slots
            for (int gi = 0; gi < sp.G; ++gi) {
                int pad = 0;
                for (int r = 0; r < sp.R; ++r) {
                    const bool isp = (int)(sp.slot_ve[c * GR + gi * sp.R + r] >> 16) == E;
                    if (!isp && pad) ++fails;
                    pad += isp;
                }
                if (pad > sp.padr) ++fails;
            }
        }
    }
    for (int x = 0; x < 2; ++x)
        for (int i = x ? 0 : 1; i < 7; ++i) {
            const Layout& L = x ? T.laysx[i] : T.lays[i];
            if (!L.ok) continue;
            ++nlay;
            std::vector<int> owner(L.P + 1, -1), epos(E, -1);
            int expect = 0;
            // x layouts: T row positions, a one-to-one map into [0, ts)
            const bool tx = x != 0;
            const int ts = tx ? L.ts : V;
            if (tx) {
                std::vector<int> used(ts > 0 ? ts : 1, 0);
                if ((int)L.tpos.size() != V || ts < V || ts > 65535) ++fails;
                else
                    for (int v = 0; v < V; ++v)
                        if (L.tpos[v] < 0 || L.tpos[v] >= ts || used[L.tpos[v]]++) ++fails;
            }
            auto tp = [&](int v) { return tx && (int)L.tpos.size() == V ? L.tpos[v] : v; };
            for (int j = 0; j < V; ++j) {
                const int v = L.vlay[2 * j] & 0xffff, dpad = (int)((uint32_t)L.vlay[2 * j] >> 16);
                const int pos = L.vlay[2 * j + 1] & 0xffff;
                if (((uint32_t)L.vlay[2 * j + 1] >> 16) != (uint32_t)(tx ? tp(v) : 0)) ++fails;
                const int deg = vptr[v + 1] - vptr[v];
                if (pos != expect || dpad < deg + x || pos + dpad > L.P) { ++fails; continue; }
                expect = pos + dpad;
                for (int k = 0; k < dpad; ++k) {
                    if (owner[pos + k] != -1) ++fails;
                    owner[pos + k] = v;
                }
                for (int e = vptr[v]; e < vptr[v + 1]; ++e) epos[e] = pos + (e - vptr[v]);
            }
            if (expect != L.P) ++fails;
            // the slot table: per check, its edges in some order (the x layouts spread them over
            // the slot rows, spread_check_slots), each once, as {variable, position}; padding
            // trailing at the spare position
            const SlotPlan& sp = T.plans[1];
            const int GR = sp.G * sp.R;
            std::vector<int> epos_inv(L.P + 1, -1), seen(E, 0);
            for (int e = 0; e < E; ++e)
                if (epos[e] >= 0) epos_inv[epos[e]] = e;
            for (int c = 0; c < C; ++c) {
                const int deg = cptr[c + 1] - cptr[c];
                for (int k = 0; k < GR; ++k) {
                    const uint32_t sl = (uint32_t)L.slot[c * GR + k];
                    const int pos = (int)(sl >> 16);
                    if (k >= deg) {
                        if (pos != L.P) ++fails;
                        continue;
                    }
                    const int e = pos <= L.P ? epos_inv[pos] : -1;
                    if (e < 0 || (int)(t[e] >> 16) != c || (int)(sl & 0xffffu) != tp((int)(t[e] & 0xffff)) ||
                        seen[e]++)
                        ++fails;
                }
            }
        }
    if (report) {
        report[0] = 3;
        report[1] = nlay;
        report[2] = E;
        report[3] = fails;
    }
    return fails ? GNND_ERR_GRAPH : GNND_OK;
}

}  // namespace

// Build every table gnnd_graph_create would upload, on the host only, and check their
// invariants (no device needed: CPU tests and the host sanitizer build run this).
// report[4] = {slot plans checked, layouts checked, edges, failures}.
extern "C" int gnnd_graph_validate_host(const int64_t* h_var, const int64_t* h_chk,
                                        int64_t num_edges, int32_t V, int32_t C,
                                        int32_t* h_report4) {
    HostTables T;
    const int rc = build_tables(h_var, h_chk, num_edges, V, C, T);
    if (rc != GNND_OK) return rc;
    return check_tables(T, h_report4);
}

namespace {

// one graph without component analysis (gnnd_graph_create adds it)
int create_single(const int64_t* h_var, const int64_t* h_chk, int64_t num_edges, int32_t V,
                  int32_t C, gnnd_graph** out) {
    *out = nullptr;
    HostTables T;
    const int rc = build_tables(h_var, h_chk, num_edges, V, C, T);
    if (rc != GNND_OK) return rc;
    const int E = T.E, max_dv = T.max_dv, max_dc = T.max_dc, nints = T.nints, ord_off = T.ord_off;
    const std::vector<int>& table = T.table;
    const SlotPlan* plans = T.plans;
    const Layout* lays = T.lays;
    const Layout* laysx = T.laysx;
    const int* plan_off = T.plan_off;
    const int* lay_off = T.lay_off;
    const int* layx_off = T.layx_off;
    gnnd_graph* g = (gnnd_graph*)calloc(1, sizeof(gnnd_graph));
    if (!g) return GNND_ERR_ALLOC;
    hipError_t err = hipMalloc(&g->dev, sizeof(int) * table.size());
    if (err != hipSuccess) { free(g); set_hip_error(err); return GNND_ERR_ALLOC; }
    err = hipMemcpy(g->dev, table.data(), sizeof(int) * table.size(), hipMemcpyHostToDevice);
    if (err != hipSuccess) { (void)hipFree(g->dev); free(g); return set_hip_error(err); }
    int* d = (int*)g->dev;
    g->table_bytes = sizeof(int) * (size_t)nints;
    GraphView& gv = g->view;
    gv.V = V; gv.C = C; gv.E = E; gv.N = V + C;
    gv.max_dv = max_dv; gv.max_dc = max_dc;
    gv.edge_vc = (const uint32_t*)d;
    gv.var_ptr = d + E;
    gv.chk_ptr = d + E + V + 1;
    gv.chk_edge = d + E + V + 1 + C + 1;
    gv.var_ord = (const uint2*)(d + ord_off);
    gv.xs = V + C; gv.xv0 = 0; gv.xc0 = V; gv.os = V; gv.o0 = 0; gv.es = E; gv.e0 = 0;
    gv.ts = V;
    g->ncomp = 1;
    g->min_dc = T.min_dc;
    g->rview = gv;
    g->pview = gv;
    for (int i = 0; i < 3; ++i) {
        GraphView& pv = i == 0 ? g->view : i == 1 ? g->rview : g->pview;
        const int ns = (int)plans[i].slot.size();
        pv.G = plans[i].G; pv.R = plans[i].R;
        pv.padded = plans[i].padded;
        pv.padr = plans[i].padr;
        pv.logG = 0;
        while ((1 << pv.logG) < pv.G) ++pv.logG;
        pv.slot = (const uint32_t*)(d + plan_off[i]);
        pv.vslot = d + plan_off[i] + ns;
        pv.slot_ve = (const uint32_t*)(d + plan_off[i] + ns + E);
        pv.vlay = gv.var_ord;               // identity layout: positions = edge ids
        pv.vgroup = 1; pv.spare = E; pv.P1 = E + 1;
    }
    for (int i = 0; i < 7; ++i) {
        for (int x = 0; x < 2; ++x) {
            GraphView& lv = x ? g->rlayx[i] : g->rlay[i];
            const Layout& L = x ? laysx[i] : lays[i];
            lv = g->rview;
            if (i == 0 && !x) continue;
            lv.vgroup = 1 << i;
            if (!L.ok) { lv.vlay = nullptr; continue; }
            const int o = (x ? layx_off : lay_off)[i];
            lv.vlay = (const uint2*)(d + o);
            lv.slot_ve = (const uint32_t*)(d + o + 2 * V);
            lv.spare = L.P;
            lv.P1 = (L.P + 1) | 1;          // odd codeword stride, spare slot included
            lv.ts = x ? L.ts : V;
        }
    }
    // layered schedule (gnnd_minsum_layered): the greedy layers, kept beside the views
    {
        const int* cptr = table.data() + E + V + 1;
        const int* cedge = cptr + C + 1;
        std::vector<int> cvar(E), layer_of, layer_tab, layer_chk;
        for (int i = 0; i < E; ++i) cvar[i] = (int)((uint32_t)table[cedge[i]] & 0xffffu);
        g->nlayers = gnnd_layers_build(V, C, cptr, cvar.data(), layer_of);
        gnnd_layers_order(C, g->nlayers, layer_of, layer_tab, layer_chk);
        for (int k = 0; k < g->nlayers; ++k)
            g->max_layer = std::max(g->max_layer, layer_tab[k + 1] - layer_tab[k]);
        layer_tab.insert(layer_tab.end(), layer_chk.begin(), layer_chk.end());
        g->layer_of = (int*)malloc(sizeof(int) * (size_t)C);
        if (!g->layer_of) { (void)hipFree(g->dev); free(g); return GNND_ERR_ALLOC; }
        memcpy(g->layer_of, layer_of.data(), sizeof(int) * (size_t)C);
        err = hipMalloc((void**)&g->layer_dev, sizeof(int) * layer_tab.size());
        if (err == hipSuccess) {
            err = hipMemcpy(g->layer_dev, layer_tab.data(), sizeof(int) * layer_tab.size(),
                            hipMemcpyHostToDevice);
            if (err != hipSuccess) (void)hipFree(g->layer_dev);
        }
        if (err != hipSuccess) {
            (void)hipFree(g->dev);
            free(g->layer_of);
            free(g);
            return set_hip_error(err);
        }
    }
    *out = g;
    return GNND_OK;
}

int destroy_graph(gnnd_graph* g) {
    hipError_t err = hipSuccess;
    for (int k = 0; k < g->ncomp && g->ncomp > 1; ++k)
        if (g->comp[k]) {
            const int rc = destroy_graph(g->comp[k]);
            if (rc != GNND_OK && err == hipSuccess) err = (hipError_t)gnnd_last_hip_error();
        }
    if (g->dcomp) {
        const hipError_t e = hipFree(g->dcomp);
        if (err == hipSuccess) err = e;
    }
    const hipError_t el = hipFree(g->layer_dev);
    if (err == hipSuccess) err = el;
    free(g->layer_of);
    const hipError_t eu = hipFree(g->uf_dev);
    if (err == hipSuccess) err = eu;
    free(g->uf_ends);
    const hipError_t e = hipFree(g->dev);
    if (err == hipSuccess) err = e;
    free(g);
    return err == hipSuccess ? GNND_OK : set_hip_error(err);
}

bool same_plan(const GraphView& a, const GraphView& b) {
    return a.V == b.V && a.C == b.C && a.E == b.E && a.max_dv == b.max_dv &&
           a.max_dc == b.max_dc && a.G == b.G && a.R == b.R && a.padded == b.padded &&
           a.padr == b.padr;
}

// Connected components of the Tanner graph (union-find over variables through checks).
// The split is kept only when there are 2..kMaxComp components, each a contiguous variable
// range with a contiguous check range (so its edges are contiguous in the (v, c) order too),
// all of one shape and slot plan: then every component decodes as an independent codeword
// of a smaller graph, in its own workgroup.  The toric code (quantum/error_generate.py:39-132,
// H = [[H_x, 0], [0, H_z]] up to the removed rows) splits into its X and Z halves.
void split_components(gnnd_graph* g, const int64_t* h_var, const int64_t* h_chk) {
    const int V = g->view.V, C = g->view.C, E = g->view.E;
    std::vector<int> par(V);
    for (int v = 0; v < V; ++v) par[v] = v;
    auto find = [&](int v) {
        while (par[v] != v) v = par[v] = par[par[v]];
        return v;
    };
    std::vector<int> cfirst(C, -1);
    for (int e = 0; e < E; ++e) {
        const int v = (int)h_var[e], c = (int)h_chk[e];
        if (cfirst[c] < 0) { cfirst[c] = v; continue; }
        const int a = find(v), b = find(cfirst[c]);
        if (a != b) par[a < b ? b : a] = a < b ? a : b;     // root = smallest variable
    }
    // components in order of their first variable; contiguity: variable v's root changes
    // only at component boundaries
    std::vector<int> vstart;
    for (int v = 0; v < V; ++v)
        if (find(v) == v) vstart.push_back(v);
    const int K = (int)vstart.size();
    if (K < 2 || K > kMaxComp || V % K) return;
    for (int v = 0; v < V; ++v) {
        int k = (int)(std::upper_bound(vstart.begin(), vstart.end(), v) - vstart.begin()) - 1;
        if (find(v) != vstart[k]) return;                     // not a contiguous range
    }
    const int Vk = V / K;
    for (int k = 0; k < K; ++k)
        if (vstart[k] != k * Vk) return;                      // unequal sizes
    if (C % K || E % K) return;
    const int Ck = C / K, Ek = E / K;
    for (int c = 0; c < C; ++c)                               // check ranges contiguous, ordered
        if (cfirst[c] < 0 || cfirst[c] / Vk != c / Ck) return;
    for (int k = 0; k < K; ++k)                               // edge ranges (sorted by v)
        if ((int)h_var[k * Ek] / Vk != k || (int)h_var[k * Ek + Ek - 1] / Vk != k) return;
    gnnd_graph* comp[kMaxComp] = {};
    std::vector<int64_t> sv(Ek), sc(Ek);
    bool ok = true;
    for (int k = 0; k < K && ok; ++k) {
        for (int i = 0; i < Ek; ++i) {
            sv[i] = h_var[k * Ek + i] - (int64_t)k * Vk;
            sc[i] = h_chk[k * Ek + i] - (int64_t)k * Ck;
        }
        ok = create_single(sv.data(), sc.data(), Ek, Vk, Ck, &comp[k]) == GNND_OK;
        if (ok && k > 0)
            ok = same_plan(comp[k]->view, comp[0]->view) && same_plan(comp[k]->rview, comp[0]->rview) &&
                 same_plan(comp[k]->pview, comp[0]->pview);
    }
    std::vector<GraphView> dv(3 * (size_t)K);
    if (ok) {
        for (int k = 0; k < K; ++k) {
            gnnd_graph* ck = comp[k];
            auto patch = [&](GraphView& v) {
                v.xs = V + C; v.xv0 = k * Vk; v.xc0 = V + k * Ck;
                v.os = V; v.o0 = k * Vk;
                v.es = E; v.e0 = k * Ek;
            };
            patch(ck->view); patch(ck->rview); patch(ck->pview);
            for (int i = 0; i < 7; ++i) { patch(ck->rlay[i]); patch(ck->rlayx[i]); }
            dv[k] = ck->view;
            dv[K + k] = ck->rview;
            dv[2 * K + k] = ck->pview;
        }
        ok = hipMalloc(&g->dcomp, sizeof(GraphView) * dv.size()) == hipSuccess;
        if (ok && hipMemcpy(g->dcomp, dv.data(), sizeof(GraphView) * dv.size(),
                            hipMemcpyHostToDevice) != hipSuccess) {
            (void)hipFree(g->dcomp);
            ok = false;
        }
        if (!ok) g->dcomp = nullptr;
    }
    if (!ok) {
        for (int k = 0; k < K; ++k)
            if (comp[k]) destroy_graph(comp[k]);
        (void)hipGetLastError();
        return;
    }
    g->ncomp = K;
    for (int k = 0; k < K; ++k) g->comp[k] = comp[k];
}

// The decoding graph of gnnd_uf, for a matchable graph: the endpoint and virtual-vertex tables on
// the device, the endpoints on the host too.  Any other graph keeps uf_nvert == 0 (gnnd_uf and
// gnnd_graph_matching then refuse it); a failed allocation or copy is an error of the create call.
int attach_matching(gnnd_graph* g, const int64_t* h_var, const int64_t* h_chk) {
    const int V = g->view.V, C = g->view.C;
    GnndUfGraph ug;
    if (gnnd_uf_graph_build(h_var, h_chk, g->view.E, V, C, ug) != GNND_OK) return GNND_OK;
    std::vector<int> tab(ug.ends);
    tab.insert(tab.end(), ug.cvirt.begin(), ug.cvirt.end());
    g->uf_ends = (int*)malloc(sizeof(int) * 2 * (size_t)V);
    if (!g->uf_ends) return GNND_ERR_ALLOC;
    memcpy(g->uf_ends, ug.ends.data(), sizeof(int) * 2 * (size_t)V);
    hipError_t err = hipMalloc((void**)&g->uf_dev, sizeof(int) * tab.size());
    if (err != hipSuccess) { g->uf_dev = nullptr; set_hip_error(err); return GNND_ERR_ALLOC; }
    err = hipMemcpy(g->uf_dev, tab.data(), sizeof(int) * tab.size(), hipMemcpyHostToDevice);
    if (err != hipSuccess) return set_hip_error(err);
    g->uf_nvert = ug.N;
    return GNND_OK;
}

}  // namespace

extern "C" int gnnd_graph_create(const int64_t* h_var, const int64_t* h_chk, int64_t num_edges,
                                 int32_t V, int32_t C, gnnd_graph** out) {
    if (!out) return GNND_ERR_INVALID_ARG;
    const int rc = create_single(h_var, h_chk, num_edges, V, C, out);
    if (rc != GNND_OK) return rc;
    split_components(*out, h_var, h_chk);
    const int mrc = attach_matching(*out, h_var, h_chk);
    if (mrc != GNND_OK) {
        destroy_graph(*out);
        *out = nullptr;
        return mrc;
    }
    return GNND_OK;
}

extern "C" int gnnd_graph_destroy(gnnd_graph* g) {
    if (!g) return GNND_ERR_INVALID_ARG;
    return destroy_graph(g);
}

extern "C" int gnnd_graph_components(const gnnd_graph* g, int32_t* h_ncomp) {
    if (!g || !h_ncomp) return GNND_ERR_INVALID_ARG;
    *h_ncomp = g->ncomp;
    return GNND_OK;
}

extern "C" int gnnd_graph_layers(const gnnd_graph* g, int32_t* h_nlayers,
                                 int32_t* h_layer_of_check) {
    if (!g || !h_nlayers) return GNND_ERR_INVALID_ARG;
    *h_nlayers = g->nlayers;
    if (h_layer_of_check)
        for (int c = 0; c < g->view.C; ++c) h_layer_of_check[c] = g->layer_of[c];
    return GNND_OK;
}

extern "C" int gnnd_graph_layers_host(const int64_t* h_var, const int64_t* h_chk,
                                      int64_t num_edges, int32_t V, int32_t C, int32_t* h_nlayers,
                                      int32_t* h_layer_of_check) {
    return gnnd_graph_layers_host_checked(h_var, h_chk, num_edges, V, C, h_nlayers,
                                          h_layer_of_check);
}

extern "C" int gnnd_graph_matching(const gnnd_graph* g, int32_t* h_nvert, int32_t* h_endpoints) {
    if (!g || !h_nvert) return GNND_ERR_INVALID_ARG;
    if (g->uf_nvert == 0) return GNND_ERR_UNSUPPORTED;
    *h_nvert = g->uf_nvert;
    if (h_endpoints)
        for (int i = 0; i < 2 * g->view.V; ++i) h_endpoints[i] = g->uf_ends[i];
    return GNND_OK;
}

extern "C" int gnnd_graph_matching_host(const int64_t* h_var, const int64_t* h_chk,
                                        int64_t num_edges, int32_t V, int32_t C, int32_t* h_nvert,
                                        int32_t* h_endpoints) {
    return gnnd_graph_matching_host_checked(h_var, h_chk, num_edges, V, C, h_nvert, h_endpoints);
}

extern "C" int gnnd_graph_set_split(gnnd_graph* g, int32_t enable) {
    if (!g) return GNND_ERR_INVALID_ARG;
    g->nosplit = enable ? 0 : 1;
    return GNND_OK;
}

extern "C" int gnnd_graph_dims(const gnnd_graph* g, int32_t* d) {
    if (!g || !d) return GNND_ERR_INVALID_ARG;
    d[0] = g->view.V; d[1] = g->view.C; d[2] = g->view.E; d[3] = g->view.N;
    d[4] = g->view.max_dv; d[5] = g->view.max_dc;
    return GNND_OK;
}

// one thread per batched edge column; any mismatch clears the flag (flag pre-set to 1)
__global__ void __launch_bounds__(GNND_BLOCK)
check_tiled_kernel(GraphView g, const int64_t* __restrict__ ei, int64_t stride, int64_t nE,
                   int64_t shift, int32_t* flag) {
    int64_t i = (int64_t)blockIdx.x * GNND_BLOCK + threadIdx.x;
    if (i >= nE) return;
    int64_t b = i / g.E;
    int e = (int)(i - b * g.E);
    uint32_t vc = g.edge_vc[e];
    int64_t base = b * g.N;
    bool ok = ei[i] == base + (int64_t)(vc & 0xffffu) &&
              ei[stride + i] == base + shift + (int64_t)(vc >> 16);
    if (!ok) *flag = 0;   // benign race: every writer stores 0
}

__global__ void set_flag_kernel(int32_t* flag, int32_t v) { *flag = v; }

extern "C" int gnnd_check_tiled(const gnnd_graph* g, const int64_t* d_ei, int64_t row_stride,
                                int64_t nE, int64_t batch, int64_t chk_shift, int32_t* d_flag,
                                void* stream) {
    if (!g || !d_ei || !d_flag || batch < 0 || row_stride < nE) return GNND_ERR_INVALID_ARG;
    hipStream_t st = (hipStream_t)stream;
    const bool shape_ok = nE == batch * (int64_t)g->view.E;
    set_flag_kernel<<<1, 1, 0, st>>>(d_flag, shape_ok ? 1 : 0);
    GNND_LAUNCH_CHECK();
    if (!shape_ok || nE == 0) return GNND_OK;
    int64_t blocks = (nE + GNND_BLOCK - 1) / GNND_BLOCK;
    check_tiled_kernel<<<(unsigned)blocks, GNND_BLOCK, 0, st>>>(g->view, d_ei, row_stride, nE,
                                                                 chk_shift, d_flag);
    GNND_LAUNCH_CHECK();
    return GNND_OK;
}

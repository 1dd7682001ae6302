// Layout, launch plan and staging of the Monte-Carlo SIR calls (gnode_sir_plan.h); gnode_sir.hip holds the kernels and the calls.
#include "gnode_sir_plan.h"
#include <algorithm>
#include <cmath>
#include <cstdio>

static size_t al(size_t x) { return (x + 255) / 256 * 256; }

static size_t frontier_bitmap_bytes(int n) { return 3 * ((((size_t)n + 31) / 32 + 3) & ~(size_t)3) * 4; }   // ever-infected + spent + recovered
// list elements in LDS: current + next frontier [n] each, long rows [as many as the graph has, padded to 8]
static size_t frontier_list_bytes(int n, int n_big) { return 2 * (2 * (size_t)n + (((size_t)n_big + 7) & ~(size_t)7)); }
// static_lds (here and below): what the instance keeps in static LDS beyond the few counters every instance has -- e.g. the SCORE
// instances' tallies (kSirScoreLds) -- so that the same 48 KiB hold the lists AND the tallies
bool frontier_lists_in_lds(int n, int n_big, size_t static_lds) {
    return n <= 65536 && frontier_bitmap_bytes(n) + frontier_list_bytes(n, n_big) + static_lds <= 48 * 1024;
}
// + 1 KB of coin queue per wave (the DYNAMIC bytes: static_lds only moves the boundary of the lists)
size_t frontier_lds_bytes(int n, int n_big, int threads, size_t static_lds) {
    return frontier_bitmap_bytes(n) + (size_t)(threads / 64) * 1024 + (frontier_lists_in_lds(n, n_big, static_lds) ? frontier_list_bytes(n, n_big) : 0);
}
// Workgroup size and workgroups per CU (the LDS decides how many fit).  Measured, 10 000 x 20 (2 000 x 30 at epinions size),
// beta 0.3 / 0.05, ms:            16 waves per CU    24 waves      32 waves
//   fb-social size (256 threads)        --           2.90 / 4.12   3.26 / 4.14
//   wiki-vote size (512 threads)    9.8 / 28.0       8.2 / 22.5    9.3 / 25.1
//   epinions size  (512 threads)        --          29.5 / 36.8   35.7 / 41.9     (256 threads x 5: 37.1 / 46.8)
// -- past 24 waves the resident trajectories thrash each other's rows in the L2, below it the waits are exposed.  So: 256
// threads for small graphs, 512 otherwise (1 024 when the LDS leaves fewer than 16 waves), at most GN_SIR_WAVES waves per CU.
#ifndef GN_SIR_WAVES
#define GN_SIR_WAVES 24
#endif
#ifndef GN_SIR_THREADS
#define GN_SIR_THREADS 0
#endif
int frontier_threads(int n, int n_big, int* per_cu_out, size_t static_lds) {
    for (int threads = GN_SIR_THREADS ? GN_SIR_THREADS : (n < 4096 ? 256 : 512); ; threads *= 2) {
        int per_cu = (int)std::max<size_t>(1, std::min<size_t>(8, (160 * 1024) / (frontier_lds_bytes(n, n_big, threads, static_lds) + 64 + static_lds)));
        if (per_cu * (threads / 64) >= 16 || threads == 1024 || GN_SIR_THREADS) {
            per_cu = std::max(1, std::min(per_cu, GN_SIR_WAVES / (threads / 64)));
            *per_cu_out = per_cu;
            return threads;
        }
    }
}

SirLaunch sir_launch_plan(int n, int n_bigrow, int num_cu, int64_t sims, bool edge_scan, size_t static_lds) {
    int per_cu = 1;
    const int threads = frontier_threads(n, n_bigrow, &per_cu, static_lds);
    const size_t fl = frontier_lds_bytes(n, n_bigrow, threads, static_lds), lds = (size_t)2 * n;
    if (fl + static_lds <= kLdsStateLimit && !edge_scan) {
        // frontier-driven walk.  Workgroups per CU by LDS, at least 16 waves per CU
        const int64_t grid = std::min<int64_t>(sims, (int64_t)num_cu * per_cu);
        if (frontier_lists_in_lds(n, n_bigrow, static_lds)) return {SIR_FRONTIER_LDS, threads, (int)grid, fl};
        return {SIR_FRONTIER_MEM, threads, (int)std::min<int64_t>(grid, kFrontierGlobalGrid), fl};
    }
    if (lds + static_lds <= kLdsStateLimit) {
        // edge-parallel scan, node state in LDS: 256 threads for small graphs, 1024 when the state allows one workgroup per CU
        per_cu = (int)std::max<size_t>(1, std::min<size_t>(8, (160 * 1024) / std::max<size_t>(lds + static_lds, 1)));
        return {SIR_SCAN_LDS, per_cu >= 4 ? 256 : (per_cu >= 2 ? 512 : 1024), (int)std::min<int64_t>(sims, (int64_t)num_cu * per_cu), lds};
    }
    return {SIR_SCAN_MEM, 256, (int)std::min<int64_t>(sims, 2048), 0};
}

SirLayout sir_layout(int n, int64_t nnz, int n_bigrow, int T, size_t static_lds) {
    SirLayout L;
    L.hist = 0;
    L.seeds = L.hist + al((size_t)2 * T * n * sizeof(uint32_t));
    L.rows = L.seeds + al(4096 * sizeof(int32_t));
    L.tail = L.rows + al((size_t)std::max<int64_t>(nnz, 1) * sizeof(int32_t));
    size_t tail = 0;
    if ((size_t)2 * n + static_lds > kLdsStateLimit) tail = (size_t)2048 * 2 * n;
    if (!frontier_lists_in_lds(n, n_bigrow, static_lds)) tail = std::max(tail, (size_t)kFrontierGlobalGrid * 3 * n * sizeof(int32_t));
    L.thr = L.bytes[SIR_SCALAR] = L.tail + al(tail);
    const size_t per_node = al((size_t)2 * n * sizeof(unsigned long long));
    L.bytes[SIR_NODES] = L.thr + per_node;
    L.start = L.bytes[SIR_EDGES] = L.thr + al(((size_t)std::max<int64_t>(nnz, 0) + (size_t)n) * sizeof(unsigned long long));
    L.bytes[SIR_INIT] = L.start + per_node;
    return L;
}

unsigned long long coin_threshold(double p) {
    return (unsigned long long)std::min(4294967296.0, std::max(0.0, std::floor(p * 4294967296.0)));
}

static SirThresholds refused(const char* msg) { SirThresholds t; t.error = msg; return t; }   // nothing staged, only the message
#define refuse(...) (snprintf(buf, sizeof buf, __VA_ARGS__), refused(buf))

SirThresholds sir_stage(const char* who, int n, int64_t nnz, const SirRates& r, const int32_t* restate_col, const double* init) {
    SirThresholds t;
    char buf[256];
    const int32_t* col = r.form == SIR_NODES ? restate_col : nullptr;
    const auto prob = [](double p) { return p >= 0.0 && p <= 1.0; };   // (a NaN fails both comparisons)
    if (r.form == SIR_SCALAR) {
        if (!prob(r.beta) || !prob(r.gamma)) return refuse("%s: beta = %g, gamma = %g are not both in [0,1]", who, r.beta, r.gamma);
        t.tb = coin_threshold(r.beta); t.tg = coin_threshold(r.gamma);
    } else {
        const size_t nb = (r.form == SIR_EDGES || col) ? (size_t)nnz : (size_t)n;   // infection thresholds in front of the recovery ones
        t.rates.resize(nb + n);
        if (r.form == SIR_EDGES) {
            for (size_t p = 0; p < nb; ++p) {
                if (!prob(r.w_edges[p])) return refuse("%s: the weight at CSR position %zu, %g, is not in [0,1]", who, p, r.w_edges[p]);
                t.rates[p] = coin_threshold(r.w_edges[p]);
            }
        } else {
            for (int v = 0; v < n; ++v)
                if (!prob(r.beta_nodes[v])) return refuse("%s: beta[%d] = %g is not in [0,1]", who, v, r.beta_nodes[v]);
            for (size_t p = 0; p < nb; ++p) t.rates[p] = coin_threshold(r.beta_nodes[col ? col[p] : (int)p]);
        }
        for (int v = 0; v < n; ++v) {
            const double gv = r.gamma_nodes ? r.gamma_nodes[v] : r.gamma;
            if (!prob(gv)) return refuse("%s: gamma[%d] = %g is not in [0,1]", who, v, gv);
            t.rates[nb + v] = coin_threshold(gv);
        }
    }
    if (init) {
        t.start.resize((size_t)2 * n);
        for (int v = 0; v < n; ++v) {
            const double* p = init + (size_t)3 * v;
            for (int c = 0; c < 3; ++c)
                if (!prob(p[c])) return refuse("%s: init[%d][%d] = %g is not in [0,1]", who, v, c, p[c]);
            if (!(std::fabs(p[0] + p[1] + p[2] - 1.0) <= 1e-6)) return refuse("%s: the row of node %d sums to %.9g, not 1", who, v, p[0] + p[1] + p[2]);
            t.start[v] = coin_threshold(p[0]);
            t.start[(size_t)n + v] = coin_threshold(p[2]);
        }
    }
    return t;
}

SirScheduleLayout sir_schedule_layout(int n, int64_t nnz, int n_bigrow, int T, int P, size_t static_lds) {
    SirScheduleLayout L;
    static_cast<SirLayout&>(L) = sir_layout(n, nnz, n_bigrow, T, static_lds);
    const size_t tables = (size_t)std::max(P, 1) * ((size_t)std::max<int64_t>(nnz, 0) + (size_t)n);
    L.start = L.thr + al(tables * sizeof(unsigned long long));
    L.phase = L.start + al((size_t)2 * n * sizeof(unsigned long long));
    L.total = L.phase + al((size_t)std::max(T, 1) * sizeof(int32_t));
    return L;
}

SirThresholds sir_stage_schedule(const char* who, int n, int64_t nnz, int T, int P, const int32_t* phase, const double* w, const double* gamma,
                                 const double* init) {
    char buf[256];
    const auto prob = [](double p) { return p >= 0.0 && p <= 1.0; };   // (a NaN fails both comparisons)
    if (P < 1) return refuse("%s: a schedule has at least one phase (P = %d)", who, P);
    for (int t = 1; t < T; ++t)
        if (phase[t] < 0 || phase[t] >= P) return refuse("%s: phase[%d] = %d is not in [0, %d)", who, t, phase[t], P);
    SirRates none;                                                     // the start alone, through the one place that checks it
    SirThresholds t = sir_stage(who, n, nnz, none, nullptr, init);
    if (!t.error.empty()) return t;
    const size_t ne = (size_t)std::max<int64_t>(nnz, 0);
    t.tb = t.tg = 0;
    t.rates.resize((size_t)P * (ne + n));
    for (int p = 0; p < P; ++p) {
        for (size_t q = 0; q < ne; ++q) {
            const double x = w[(size_t)p * ne + q];
            if (!prob(x)) return refuse("%s: phase %d: the weight at CSR position %zu, %g, is not in [0,1]", who, p, q, x);
            t.rates[(size_t)p * ne + q] = coin_threshold(x);
        }
        for (int v = 0; v < n; ++v) {
            const double x = gamma[(size_t)p * n + v];
            if (!prob(x)) return refuse("%s: phase %d: gamma[%d] = %g is not in [0,1]", who, p, v, x);
            t.rates[(size_t)P * ne + (size_t)p * n + v] = coin_threshold(x);
        }
    }
    return t;
}

static SirSweepLayout sweep_layout(int n, int64_t nnz, int n_bigrow, int T, int P, int L, int C, size_t static_lds) {
    const SirScheduleLayout S = sir_schedule_layout(n, nnz, n_bigrow, T, P, static_lds);
    const size_t ids = al((size_t)std::max(C, 1) * sizeof(int32_t));
    SirSweepLayout W;
    W.rows = 0;                                                    // (S.rows is where the histogram and the seed list end)
    W.tail = S.tail - S.rows;
    W.thr = S.thr - S.rows;
    W.start = S.start - S.rows;
    W.phase = S.phase - S.rows;
    W.cand = W.phase + al((size_t)std::max(L, 1) * sizeof(int32_t));
    W.shifts = W.cand + ids;
    W.total = W.shifts + ids;
    return W;
}
SirSweepLayout sir_sweep_layout(int n, int64_t nnz, int n_bigrow, int T, int P, int L, int C) { return sweep_layout(n, nnz, n_bigrow, T, P, L, C, 0); }

SirThresholds sir_stage_sweep(const char* who, int n, int64_t nnz, int T, int P, int L, const int32_t* phase, const double* w,
                              const double* gamma, const double* init, int C, const int32_t* shifts) {
    char buf[256];
    if (L < T) return refuse("%s: the phase row holds L = %d entries, fewer than T = %d", who, L, T);
    for (int c = 0; shifts && c < C; ++c)
        if (shifts[c] < 0 || (int64_t)shifts[c] + T > L)
            return refuse("%s: shifts[%d] = %d: a shift is >= 0 with shift + T <= L (T = %d, L = %d)", who, c, shifts[c], T, L);
    return sir_stage_schedule(who, n, nnz, L, P, phase, w, gamma, init);
}

SirScoreLayout sir_score_layout(int n, int64_t nnz, int n_bigrow, int T, int P, int L, int C, int O) {
    SirScoreLayout W;
    static_cast<SirSweepLayout&>(W) = sweep_layout(n, nnz, n_bigrow, T, P, L, C, kSirScoreLds);
    const size_t table = al((size_t)std::max(O, 1) * sizeof(int32_t));
    W.obs = W.total;
    W.marked = W.obs + al((size_t)std::max(O, 1) * (size_t)n);
    W.seen = W.marked + table;
    W.total = W.seen + table;
    return W;
}

// The checks the scored sweeps share, each a refusal (the message; empty: accepted).  O things (`what`: snapshots, evidence sets)
// per call, as many as the kernels' static LDS has room for ...
static std::string bad_sets(const char* who, int O, const char* what) {
    char buf[256];
    if (O >= 1 && O <= GN_SIR_SCORE_MAXO) return std::string();
    snprintf(buf, sizeof buf, "%s: O = %d %s: 1 to %d in one call", who, O, what, GN_SIR_SCORE_MAXO);
    return buf;
}
// ... and an output array of d0 * d1 * d2 * d3 cells, which the kernels index below 2^31
static bool cells_fit(int d0, int d1, int d2, int d3) {
    return (double)d0 * (double)std::max(d1, 1) * (double)std::max(d2, 1) * (double)std::max(d3, 1) < 2147483648.0;
}
static std::string bad_hist(const char* who, int O, int C, int T, int bins) {
    char buf[256];
    if (cells_fit(O, C, T, bins + 1)) return std::string();
    snprintf(buf, sizeof buf, "%s: the histogram [O = %d][C = %d][T = %d][bins + 1 = %d] has 2^31 cells or more", who, O, C, T, bins + 1);
    return buf;
}

SirScoreStaged sir_stage_score(const char* who, int n, int64_t nnz, int T, int P, int L, const int32_t* phase, const double* w,
                               const double* gamma, const double* init, int C, const int32_t* shifts, const int8_t* obs, int O, int measure,
                               int bins) {
    char buf[256];
    std::string bad;
    SirScoreStaged s;                                                  // (a refusal: nothing staged, only thr.error)
#define refuse_score(...) (s.thr = refuse(__VA_ARGS__), s)
    if (!(bad = bad_sets(who, O, "snapshots")).empty()) return refuse_score("%s", bad.c_str());
    if (bins < 1 || bins > 4096) return refuse_score("%s: bins = %d is not in [1, 4096]", who, bins);
    if (measure != 0 && measure != 1) return refuse_score("%s: measure %d is neither 0 (jaccard) nor 1 (match)", who, measure);
    if (!(bad = bad_hist(who, O, C, T, bins)).empty()) return refuse_score("%s", bad.c_str());
    std::vector<int32_t> marked((size_t)O, 0), seen((size_t)O, 0);
    for (int o = 0; o < O; ++o) {
        for (int v = 0; v < n; ++v) {
            const int x = obs[(size_t)o * n + v];
            if (x < -1 || x > 2) return refuse_score("%s: obs[%d][%d] = %d is not a code in [-1, 2]", who, o, v, x);
            seen[o] += x >= 0; marked[o] += x >= 1;
        }
        if (seen[o] == 0) return refuse_score("%s: snapshot %d observes no node", who, o);
    }
#undef refuse_score
    s.thr = sir_stage_sweep(who, n, nnz, T, P, L, phase, w, gamma, init, C, shifts);
    if (!s.thr.error.empty()) return s;
    s.obs.resize((size_t)n * O);                                       // node-major: an event reads its O codes from one place
    for (int o = 0; o < O; ++o)
        for (int v = 0; v < n; ++v) s.obs[(size_t)v * O + o] = obs[(size_t)o * n + v];
    s.marked = std::move(marked); s.seen = std::move(seen);
    return s;
}
template <class V> static SirUpload upload(size_t at, const V& v) { return {at, v.data(), v.size() * sizeof(v[0])}; }
std::vector<SirUpload> SirScoreStaged::uploads(const SirScoreLayout& W) const { return {upload(W.obs, obs), upload(W.marked, marked), upload(W.seen, seen)}; }

// the sweep's layout under `static_lds`, then the records of a timed call (sir_timed_layout, sir_post_layout)
static SirTimedLayout record_layout(int n, int64_t nnz, int n_bigrow, int T, int P, int L, int C, int O, int R, size_t static_lds) {
    SirTimedLayout W;
    static_cast<SirSweepLayout&>(W) = sweep_layout(n, nnz, n_bigrow, T, P, L, C, static_lds);
    const size_t table = al((size_t)std::max(O, 1) * sizeof(int32_t));
    W.rec_ptr = W.total;
    W.rec = W.rec_ptr + al(((size_t)n + 1) * sizeof(int32_t));
    W.zeros = W.rec + al((size_t)std::max(R, 1) * sizeof(uint32_t));
    W.records = W.zeros + table;
    W.total = W.records + table;
    return W;
}
SirTimedLayout sir_timed_layout(int n, int64_t nnz, int n_bigrow, int T, int P, int L, int C, int O, int R) {
    return record_layout(n, nnz, n_bigrow, T, P, L, C, O, R, kSirTimedLds);
}

// The records of a timed call (sir_stage_timed, sir_stage_post), in two halves around the sweep's own staging.  The checks: R >= 1,
// every set in [0, O), node in [0, n), kind in [0, 4] and offset <= 0, every set holding a record; they count zeros[o],
// records[o] and, in ptr[v + 1], the records of node v.  A refusal (the message; empty: accepted) names the offending index.
static std::string check_records(const char* who, int n, const int32_t* rec_set, const int32_t* rec_node, const int32_t* rec_offset,
                                 const int32_t* rec_kind, int R, int O, std::vector<int32_t>& zeros, std::vector<int32_t>& records,
                                 std::vector<int32_t>& ptr) {
    char buf[256];
#define refuse_rec(...) (snprintf(buf, sizeof buf, __VA_ARGS__), std::string(buf))
    if (R < 1) return refuse_rec("%s: R = %d records: at least one", who, R);
    zeros.assign((size_t)O, 0); records.assign((size_t)O, 0); ptr.assign((size_t)n + 1, 0);
    for (int i = 0; i < R; ++i) {
        if (rec_set[i] < 0 || rec_set[i] >= O) return refuse_rec("%s: rec_set[%d] = %d is not in [0, %d)", who, i, rec_set[i], O);
        if (rec_node[i] < 0 || rec_node[i] >= n) return refuse_rec("%s: rec_node[%d] = %d is not in [0, %d)", who, i, rec_node[i], n);
        if (rec_kind[i] < 0 || rec_kind[i] > 4) return refuse_rec("%s: rec_kind[%d] = %d is not a kind in [0, 4]", who, i, rec_kind[i]);
        if (rec_offset[i] > 0) return refuse_rec("%s: rec_offset[%d] = %d is after now: offsets are <= 0", who, i, rec_offset[i]);
        ++records[rec_set[i]]; zeros[rec_set[i]] += rec_kind[i] == 0; ++ptr[(size_t)rec_node[i] + 1];
    }
    for (int o = 0; o < O; ++o)
        if (records[o] == 0) return refuse_rec("%s: evidence set %d holds no record", who, o);
#undef refuse_rec
    return std::string();
}
// The sort: by node, a node's records in the order given, one word each -- set | kind << 4 | min(-offset, T) << 8.
static void sort_records(int n, int T, const int32_t* rec_set, const int32_t* rec_node, const int32_t* rec_offset, const int32_t* rec_kind, int R,
                         std::vector<int32_t>& ptr, SirTimedStaged& s) {
    for (int v = 0; v < n; ++v) ptr[(size_t)v + 1] += ptr[v];
    std::vector<int32_t> at(ptr.begin(), ptr.end() - 1);
    s.rec.resize((size_t)R);
    for (int i = 0; i < R; ++i) {
        const int64_t back = std::min<int64_t>(-(int64_t)rec_offset[i], std::max(T, 0));   // (at T or beyond: never reached)
        s.rec[(size_t)at[rec_node[i]]++] = (uint32_t)rec_set[i] | (uint32_t)rec_kind[i] << 4 | (uint32_t)back << 8;
    }
    s.rec_ptr = std::move(ptr);
}
// The sequence both timed calls end in: the records' checks, the sweep's own staging, the sort.
static void stage_records(const char* who, int n, int64_t nnz, int T, int P, int L, const int32_t* phase, const double* w, const double* gamma,
                          const double* init, int C, const int32_t* shifts, const int32_t* rec_set, const int32_t* rec_node,
                          const int32_t* rec_offset, const int32_t* rec_kind, int R, int O, SirTimedStaged& s) {
    std::vector<int32_t> zeros, records, ptr;
    const std::string bad = check_records(who, n, rec_set, rec_node, rec_offset, rec_kind, R, O, zeros, records, ptr);
    if (!bad.empty()) { s.thr = refused(bad.c_str()); return; }
    s.thr = sir_stage_sweep(who, n, nnz, T, P, L, phase, w, gamma, init, C, shifts);
    if (!s.thr.error.empty()) return;
    sort_records(n, T, rec_set, rec_node, rec_offset, rec_kind, R, ptr, s);
    s.zeros = std::move(zeros); s.records = std::move(records);
}
std::vector<SirUpload> SirTimedStaged::uploads(const SirTimedLayout& W) const {
    return {upload(W.rec_ptr, rec_ptr), upload(W.rec, rec), upload(W.zeros, zeros), upload(W.records, records)};
}

SirTimedStaged sir_stage_timed(const char* who, int n, int64_t nnz, int T, int P, int L, const int32_t* phase, const double* w,
                               const double* gamma, const double* init, int C, const int32_t* shifts, const int32_t* rec_set,
                               const int32_t* rec_node, const int32_t* rec_offset, const int32_t* rec_kind, int R, int O, int bins) {
    char buf[256];
    std::string bad;
    SirTimedStaged s;                                                  // (a refusal: nothing staged, only thr.error)
#define refuse_timed(...) (s.thr = refuse(__VA_ARGS__), s)
    if (!(bad = bad_sets(who, O, "evidence sets")).empty()) return refuse_timed("%s", bad.c_str());
    if ((int64_t)O * std::max(T, 1) > GN_SIR_TIMED_CELLS)
        return refuse_timed("%s: O = %d sets x T = %d steps are more than the %d cells of the difference array", who, O, T, GN_SIR_TIMED_CELLS);
    if (bins < 1 || bins > 4096) return refuse_timed("%s: bins = %d is not in [1, 4096]", who, bins);
    if (!(bad = bad_hist(who, O, C, T, bins)).empty()) return refuse_timed("%s", bad.c_str());
#undef refuse_timed
    stage_records(who, n, nnz, T, P, L, phase, w, gamma, init, C, shifts, rec_set, rec_node, rec_offset, rec_kind, R, O, s);
    return s;
}

SirPostLayout sir_post_layout(int n, int64_t nnz, int n_bigrow, int T, int P, int L, int C, int O, int R, int H) {
    SirPostLayout W;
    static_cast<SirTimedLayout&>(W) = record_layout(n, nnz, n_bigrow, T, P, L, C, O, R, kSirPostLds);
    W.horizons = W.total;
    W.total = W.horizons + al((size_t)std::max(H, 1) * sizeof(int32_t));
    return W;
}

SirPostStaged sir_stage_post(const char* who, int n, int64_t nnz, int T, int P, int L, const int32_t* phase, const double* w,
                             const double* gamma, const double* init, int C, const int32_t* shifts, const int32_t* rec_set,
                             const int32_t* rec_node, const int32_t* rec_offset, const int32_t* rec_kind, int R, int O, int now,
                             const int32_t* horizons, int H) {
    char buf[256];
    std::string bad;
    SirPostStaged s;                                                   // (a refusal: nothing staged, only thr.error)
#define refuse_post(...) (s.thr = refuse(__VA_ARGS__), s)
    if (!(bad = bad_sets(who, O, "evidence sets")).empty()) return refuse_post("%s", bad.c_str());
    if (now < 0 || now >= T) return refuse_post("%s: now = %d is not in [0, T = %d)", who, now, T);
    if (H < 1 || H > GN_SIR_POST_MAXH) return refuse_post("%s: H = %d horizons: 1 to %d in one call", who, H, GN_SIR_POST_MAXH);
    for (int j = 0; j < H; ++j) {
        if (horizons[j] < 0) return refuse_post("%s: horizons[%d] = %d is before now: horizons are >= 0", who, j, horizons[j]);
        if (j > 0 && horizons[j] <= horizons[j - 1]) return refuse_post("%s: horizons[%d] = %d does not ascend from horizons[%d] = %d", who, j, horizons[j], j - 1, horizons[j - 1]);
        if ((int64_t)now + horizons[j] > (int64_t)T - 1) return refuse_post("%s: horizons[%d] = %d: now + horizon = %lld is past the last step T - 1 = %d", who, j, horizons[j], (long long)now + horizons[j], T - 1);
    }
    if (!cells_fit(O, H, 2, n)) return refuse_post("%s: the counts [O = %d][H = %d][2][n = %d] have 2^31 cells or more", who, O, H, n);
#undef refuse_post
    stage_records(who, n, nnz, T, P, L, phase, w, gamma, init, C, shifts, rec_set, rec_node, rec_offset, rec_kind, R, O, s);
    if (s.thr.error.empty()) s.horizons.assign(horizons, horizons + H);
    return s;
}
SirPostStaged sir_stage_strata(const char* who, int n, int64_t nnz, int T, int P, int L, const int32_t* phase, const double* w,
                               const double* gamma, const double* init, int C, const int32_t* shifts, const int32_t* rec_set,
                               const int32_t* rec_node, const int32_t* rec_offset, const int32_t* rec_kind, int R, int O, int now,
                               const int32_t* horizons, int H, int mismatches) {
    char buf[256];
    SirPostStaged s;                                                   // (a refusal: nothing staged, only thr.error)
#define refuse_strata(...) (s = SirPostStaged(), s.thr = refuse(__VA_ARGS__), s)
    if (mismatches < 0 || mismatches > GN_SIR_POST_MAXD - 1)
        return refuse_strata("%s: mismatches = %d is not in [0, %d]", who, mismatches, GN_SIR_POST_MAXD - 1);
    s = sir_stage_post(who, n, nnz, T, P, L, phase, w, gamma, init, C, shifts, rec_set, rec_node, rec_offset, rec_kind, R, O, now, horizons, H);
    if (!s.thr.error.empty()) return s;
    const int D = mismatches + 1;                                      // (O, H and n have passed the posterior's checks)
    if (!cells_fit(O * D, H, 2, n))
        return refuse_strata("%s: the counts [O = %d][D = %d][H = %d][2][n = %d] have 2^31 cells or more", who, O, D, H, n);
#undef refuse_strata
    return s;
}
std::vector<SirUpload> SirPostStaged::uploads(const SirPostLayout& W) const {
    std::vector<SirUpload> up = SirTimedStaged::uploads(W);
    up.push_back(upload(W.horizons, horizons));
    return up;
}

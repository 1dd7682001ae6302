// The graph handle's plan and the per-call plans of the persistent launches (see gnode_graph_plan.h).  Host arithmetic only.
#include "gnode_graph_plan.h"
#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <functional>
#include <queue>

static std::string fmt(const char* f, ...) {
    char buf[256];
    va_list ap;
    va_start(ap, f);
    vsnprintf(buf, sizeof buf, f, ap);
    va_end(ap);
    return buf;
}

// Hub rows: rows longer than GN_HUB_T, their neighbour lists cut into segments of <= HUB_SEG edges (uniform work items).
static void plan_hubs(GnGraphPlan& P, const int32_t* rowptr, int32_t n) {
    P.hubidx.assign((size_t)n, -1);
    P.hub_seg_ptr.assign(1, 0);
    for (int32_t r = 0; r < n; ++r) {
        const int32_t lo = rowptr[r], hi = rowptr[r + 1];
        if (hi - lo <= GN_HUB_T) continue;
        P.hubidx[r] = P.n_hub++;
        for (int32_t e = lo; e < hi; e += HUB_SEG) {
            P.seg_lo.push_back(e);
            P.seg_hi.push_back(std::min(hi, e + HUB_SEG));
        }
        P.hub_seg_ptr.push_back((int32_t)P.seg_lo.size());
    }
    P.n_seg = (int32_t)P.seg_lo.size();
    if (P.n_hub == 0) { P.hubidx.clear(); P.hub_seg_ptr.clear(); }
}

// Row maps of k_pers64 for 1 / 2 / 4 tiles per workgroup.  Rows are sorted by length (longest first, ties by id) and dealt
// longest-processing-time first: each row goes to the workgroup with the fewest EDGES so far that still has a slot.
static void plan_pers64(GnGraphPlan& P, const int32_t* rowptr, int32_t n) {
    if (n > kPersMaxRows) return;
    std::vector<int32_t> order((size_t)n);
    for (int32_t r = 0; r < n; ++r) order[r] = r;
    auto deg = [&](int32_t r) { return rowptr[r + 1] - rowptr[r]; };
    std::stable_sort(order.begin(), order.end(), [&](int32_t x, int32_t y) { return deg(x) > deg(y); });
    for (int i = 0; i < 3; ++i) {
        const int nt = 1 << i, per_wg = 16 * nt, wgs = (n + per_wg - 1) / per_wg;
        std::vector<int32_t> map((size_t)wgs * per_wg, -1);
        // A step waits for its busiest workgroup, whose gather time follows the rows it has to read -- hub rows included, their
        // segments are summed by the owner's workgroup.  The two biggest hubs never share a workgroup, the workgroup of a big
        // hub gets short ordinary rows, and a workgroup's rows come out in descending length, so the four rows of a wave are
        // of neighbouring lengths (a wave issues loads as far as its longest row needs).
        std::vector<int> fill((size_t)wgs, 0);
        int32_t nh = 0;
        while (nh < n && deg(order[nh]) > GN_HUB_T) ++nh;
        if ((long)nh > (long)wgs * per_wg / 2) { continue; }   // (half the slots hubs: not a graph for this path)
        {
            typedef std::pair<long, int> WL;                   // (edges so far, workgroup)
            std::priority_queue<WL, std::vector<WL>, std::greater<WL>> heap;
            for (int wg = 0; wg < wgs; ++wg) heap.push(WL(0, wg));
            for (int32_t r = 0; r < n; ++r) {                  // (the heap cannot run dry: wgs * per_wg >= n)
                const WL w = heap.top();
                heap.pop();
                map[(size_t)w.second * per_wg + fill[w.second]++] = order[r];
                if (fill[w.second] < per_wg) heap.push(WL(w.first + std::max(1, deg(order[r])), w.second));
            }
        }
        // hub rows: the segments of a workgroup's hubs are summed by that workgroup's own lane groups (partials through LDS),
        // dealt to the lane groups with the least gather work so far; a hub's partial slots are consecutive, in segment order
        std::vector<int32_t> hub((size_t)wgs * per_wg * 2, 0), segptr((size_t)wgs * per_wg * 2, 0), items;
        int max_slots = 0, max_items = 0;
        bool ok = true;
        for (int wg = 0; wg < wgs && ok; ++wg) {
            std::vector<long> load((size_t)per_wg, 0);
            std::vector<std::vector<int32_t>> mine((size_t)per_wg);
            int slots = 0;
            for (int s = 0; s < per_wg; ++s) {
                const int32_t r = map[(size_t)wg * per_wg + s];
                hub[((size_t)wg * per_wg + s) * 2] = -1;
                if (r >= 0 && deg(r) <= GN_HUB_T) load[s] = deg(r);
            }
            for (int s = 0; s < per_wg; ++s) {
                const int32_t r = map[(size_t)wg * per_wg + s];
                if (r < 0 || deg(r) <= GN_HUB_T) continue;
                const int32_t lo = rowptr[r], hi = rowptr[r + 1];
                hub[((size_t)wg * per_wg + s) * 2] = slots;
                hub[((size_t)wg * per_wg + s) * 2 + 1] = (hi - lo + HUB_SEG - 1) / HUB_SEG;
                for (int32_t e = lo; e < hi; e += HUB_SEG) {
                    int best = 0;
                    for (int t = 1; t < per_wg; ++t) if (load[t] < load[best]) best = t;
                    load[best] += HUB_SEG;
                    mine[best].push_back(e); mine[best].push_back(std::min(hi, e + HUB_SEG)); mine[best].push_back(slots++); mine[best].push_back(0);
                }
            }
            if (slots > PERS_MAX_PARTIALS) ok = false;
            for (int s = 0; s < per_wg; ++s) { if ((int)(mine[s].size() / 4) > PERS_MAX_ITEMS) ok = false; max_items = std::max(max_items, (int)(mine[s].size() / 4)); }
            max_slots = std::max(max_slots, slots);
            for (int s = 0; s < per_wg; ++s) {
                segptr[((size_t)wg * per_wg + s) * 2] = (int32_t)(items.size() / 4);
                segptr[((size_t)wg * per_wg + s) * 2 + 1] = (int32_t)(mine[s].size() / 4);
                items.insert(items.end(), mine[s].begin(), mine[s].end());
            }
        }
        if (!ok) continue;                                  // this tile count is not available for this graph (the per-call plan skips it)
        GnPers64Maps& M = P.pers[i];
        M.present = true;
        M.map.swap(map); M.hub.swap(hub); M.segptr.swap(segptr); M.items.swap(items);
        M.lds = max_slots;
        M.max_items = max_items;
    }
}

// Row maps of k_persg for workgroups of 1 .. 4 waves (a wave holds 64 / LPR rows: 32 at H = 8): rows are dealt longest first,
// in snake order, to the sample's workgroups -- real node numberings put the big nodes next to each other, and one workgroup
// owning them all would need their segments' ids in its LDS and set every step's duration.  (Edge-balanced dealing -- each row
// to the workgroup with the fewest edges so far, what plan_pers64 does -- measured worse here: heavy-tailed wiki-vote size
// 0.32 -> 0.37 ms; a hub's segments are spread over the workgroup's lane groups, an ordinary row is one lane group's serial
// chain, and the snake gives every workgroup the same number of rows from every length class.)
static void plan_persg(GnGraphPlan& P, const int32_t* rowptr, int32_t n) {
    for (int vi = 0; vi < 3; ++vi) for (int nw = 0; nw < 4; ++nw) { P.pgoff[vi][nw] = -1; P.pgids[vi][nw] = P.pgsegs[vi][nw] = 0; }
    if ((long)n > 256L * 128) return;                        // never fits one resident grid
    // every row, longest first (hub rows lead), dealt in snake order: each workgroup gets its share of the long rows AND of the
    // neighbour ids -- what a step waits for is the busiest workgroup's gather
    std::vector<int> order(n);
    auto deg = [&](int i) { return rowptr[i + 1] - rowptr[i]; };
    for (int i = 0; i < n; ++i) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return deg(x) > deg(y); });
    std::vector<int32_t>& all = P.pgmap;
    for (int vi = 0; vi < 3; ++vi)
    for (int nw = 1; nw <= 4; ++nw) {
        const int gpw = (32 >> vi) * nw, wps = (n + gpw - 1) / gpw;
        if (wps > 256) continue;
        std::vector<std::vector<int>> own(wps);
        for (size_t h = 0; h < order.size(); ++h) {            // snake order: 0 .. wps-1, wps-1 .. 0, ...
            const size_t lap = h / wps, pos = h % wps;
            own[(lap & 1) ? wps - 1 - pos : pos].push_back(order[h]);
        }
        bool ok = true;
        for (int w = 0; w < wps; ++w) if ((int)own[w].size() > gpw) ok = false;     // (cannot happen: wps * gpw >= n)
        if (!ok) continue;
        const size_t off = all.size();
        all.resize(off + (size_t)wps * gpw, -1);
        long best_i = 0, best_s = 0;
        for (int ww = 0; ww < wps; ++ww) {
            long ci = 0, cs = 0;
            for (size_t k = 0; k < own[ww].size(); ++k) {
                const int i = own[ww][k], d = deg(i);
                all[off + (size_t)ww * gpw + k] = i;
                if (P.n_hub > 0 && d > GN_HUB_T) cs += (d + HUB_SEG - 1) / HUB_SEG; else ci += d;
            }
            best_i = std::max(best_i, ci); best_s = std::max(best_s, cs);
        }
        P.pgoff[vi][nw - 1] = (int32_t)off;
        P.pgids[vi][nw - 1] = (int32_t)std::min<long>(best_i, 1L << 30);
        P.pgsegs[vi][nw - 1] = (int32_t)std::min<long>(best_s, 1L << 30);
    }
}

// position of column c in row r of a CSR whose rows hold ascending columns, or -1 when (r, c) is no entry
static int32_t csr_position(const int32_t* rowptr, const int32_t* col, int32_t r, int32_t c) {
    int32_t lo = rowptr[r], hi = rowptr[r + 1] - 1;
    while (lo <= hi) {
        const int32_t mid = (lo + hi) >> 1, x = col[mid];
        if (x == c) return mid;
        if (x < c) lo = mid + 1; else hi = mid - 1;
    }
    return -1;
}

// src and rev of every CSR position (gnode_graph_plan.h); `symmetric` follows from rev.  rev[p] is csr_position's answer for
// (col[p], src[p]).  Where every row's columns ascend strictly -- every graph the project makes -- a merge gives that answer
// without searching: the questions put to row v come with ascending u (rows are visited in order, and v stands once in each),
// so `next[v]` only ever moves forward over row v.  One pass over the entries then, which is what keeps gnode_graph_create's
// cost near what it was (a search per entry: 14 ns each measured, 2.5 ms more per handle at fb-social size).
static void plan_edge_tables(GnGraphPlan& P, const int32_t* rowptr, const int32_t* col, int32_t n) {
    const size_t nnz = (size_t)rowptr[n];
    P.src.resize(nnz);
    P.rev.resize(nnz);
    bool ascending = true;
    for (int32_t u = 0; u < n; ++u)
        for (int32_t p = rowptr[u]; p < rowptr[u + 1]; ++p) {
            P.src[p] = u;
            if (p > rowptr[u] && col[p] <= col[p - 1]) ascending = false;
        }
    std::vector<int32_t> next;
    if (ascending) next.assign(rowptr, rowptr + n);
    for (int32_t u = 0; u < n; ++u)
        for (int32_t p = rowptr[u]; p < rowptr[u + 1]; ++p) {
            const int32_t v = col[p];
            int32_t r;
            if (ascending) {
                int32_t& c = next[v];
                while (c < rowptr[v + 1] && col[c] < u) ++c;
                r = c < rowptr[v + 1] && col[c] == u ? c : -1;
            } else r = csr_position(rowptr, col, v, u);
            P.rev[p] = r;
            if (r < 0) P.symmetric = false;
        }
}

GnGraphPlan gn_plan_graph(const int32_t* rowptr, const int32_t* col, int32_t n, int64_t nnz) {
    GnGraphPlan P;
    if (!(rowptr[0] == 0 && rowptr[n] == nnz)) { P.error = "gnode_graph_create: rowptr[0] != 0 or rowptr[n] != nnz"; return P; }
    for (int32_t i = 0; i < n; ++i) {
        const int32_t d = rowptr[i + 1] - rowptr[i];
        if (!(d >= 0)) { P.error = fmt("gnode_graph_create: rowptr not monotone at %d", i); return P; }
        P.max_degree = d > P.max_degree ? d : P.max_degree;
        P.n_bigrow += d > GN_SIR_BIGROW;
    }
    for (int64_t e = 0; e < nnz; ++e)
        if (!(col[e] >= 0 && col[e] < n)) { P.error = fmt("gnode_graph_create: col[%lld]=%d out of range", (long long)e, col[e]); return P; }
    P.rowhdr.assign((size_t)n * 20, 0);
    for (int32_t r = 0; r < n; ++r) {
        const int32_t lo = rowptr[r], hi = rowptr[r + 1];
        P.rowhdr[(size_t)r * 20] = lo; P.rowhdr[(size_t)r * 20 + 1] = hi;
        for (int32_t k = 0; k < 16 && lo + k < hi; ++k) P.rowhdr[(size_t)r * 20 + 4 + k] = col[lo + k];
    }
    plan_hubs(P, rowptr, n);
    plan_pers64(P, rowptr, n);
    plan_persg(P, rowptr, n);
    plan_edge_tables(P, rowptr, col, n);
    return P;
}

GnGraphInfo gn_graph_info(const GnGraphPlan& plan, int32_t n, int32_t num_cu) {
    GnGraphInfo g{};
    g.n = n; g.num_cu = num_cu; g.n_hub = plan.n_hub;
    for (int i = 0; i < 3; ++i) { g.pers[i] = plan.pers[i].present; g.persitems[i] = plan.pers[i].max_items; }
    for (int vi = 0; vi < 3; ++vi)
        for (int nw = 0; nw < 4; ++nw) { g.pgoff[vi][nw] = plan.pgoff[vi][nw]; g.pgids[vi][nw] = plan.pgids[vi][nw]; g.pgsegs[vi][nw] = plan.pgsegs[vi][nw]; }
    return g;
}

// --------------------------------------------------------------------------- per-call plans
bool gn_pers64_plan(const GnGraphInfo& g, long B, int n_steps, PersPlan* p) {
    if (n_steps < 1 || n_steps > 128 || B < 1) return false;
    const int n_xcc = 8;
    if (g.num_cu < 64 || g.num_cu % n_xcc) return false;
    const int slots = g.num_cu / n_xcc;
    if ((long)B * g.n >= (1L << 24)) return false;
    // the smallest tile count that holds the batch -- except that a graph whose biggest hub would give a lane group TWO segment
    // sums per step (a second ~2 us round of 32-row gathers every step) takes the next tile count when that halves the rounds
    // (fb-social size with a 738-edge row, B = 1: 8.7 -> 7.x us per step at 32 instead of 16 rows per workgroup)
    bool have = false;
    for (int nt = 1; nt <= 4; nt *= 2) {
        const int vi = nt == 1 ? 0 : nt == 2 ? 1 : 2;
        if (!g.pers[vi]) continue;      // graph too large, or its hub rows need too many partial slots
        const int wgs = (g.n + 16 * nt - 1) / (16 * nt);
        PersPlan q;
        q.nt = nt; q.wgs = wgs; q.n_xcc = n_xcc; q.slots = slots;
        if (wgs <= slots) { q.span = 1; q.gpx = std::min(slots / wgs, PERS_FLAG_WORDS / 32 / n_xcc); q.per = wgs; q.concurrent = n_xcc * q.gpx; }   // (one 32-word flag line per group)
        else {
            int span = 2;
            while (span < n_xcc && wgs > span * slots) span *= 2;
            if (wgs > span * slots) continue;
            q.span = span; q.gpx = 1; q.per = (wgs + span - 1) / span; q.concurrent = n_xcc / span;
        }
        if (q.concurrent < B) continue;
        q.rounds = 1;
        q.fstride = (wgs + 31) / 32 * 32;
        if ((long)q.concurrent * q.fstride > PERS_FLAG_WORDS) continue;
        if (!have) { *p = q; have = true; if (g.persitems[vi] <= 1) return true; continue; }
        if (nt <= 2 && g.persitems[vi] < g.persitems[p->nt == 1 ? 0 : 1]) { *p = q; if (g.persitems[vi] <= 1) return true; }
    }
    return have;
}

// The adjoint sweep's plan: 1 or 2 tiles per workgroup only (its per-row state -- adjoint, gradient accumulators, the interval's
// own rows -- does not fit the 128 registers a 1024-thread workgroup leaves), up to 2 consecutive launches (measured: 4 launches
// at 600 nodes x 32 samples lose to one launch per interval)
bool gn_pers_bwd64_plan(const GnGraphInfo& g, long B, int n_steps, PersPlan* p) {
    if (n_steps < 2 || n_steps > 127 || B < 1) return false;
    for (long conc = B; conc >= 1; conc = (conc + 1) / 2) {
        PersPlan q;
        if (gn_pers64_plan(g, conc, n_steps, &q) && q.nt <= 2 && (B + q.concurrent - 1) / q.concurrent <= 2 && q.wgs <= BWD_NWG) { *p = q; return true; }
        if (conc == 1) break;
    }
    return false;
}

size_t pg_lds_bytes(int H, int idcap, int segcap) {
    const size_t need = sizeof(float) * ((size_t)2 * H * H + idcap + (size_t)2 * segcap * H + (size_t)segcap * 34 + 8);
    // >= 84 KB: one workgroup per CU; the adjoint's final reduction borrows 64 KB behind the two weight copies
    return std::max<size_t>(need, std::max<size_t>(84 * 1024, sizeof(float) * 2 * H * H + 64 * 1024 + 64));
}

// The fewest rows per workgroup (most CUs) that still leaves every workgroup of the batch resident, one per CU: what a step
// waits for is its busiest CU's gather, and that is bound by the CU's rate of cache-line requests (a 32-byte row is a request
// of its own: ~1.3 ns each measured, 128 rows x 22 neighbours = 3.7 us) -- so spread the rows over as many CUs as there are.
bool gn_persg_plan(const GnGraphInfo& g, long rows, int H, int n_steps, PersgPlan* p) {
    const int vi = H == 8 ? 0 : H == 16 ? 1 : H == 32 ? 2 : -1;
    if (vi < 0 || n_steps < 1 || n_steps > 127) return false;
    if ((long)rows * H * 4 >= (1L << 31) - (1L << 17)) return false;    // 32-bit table offsets below PS_OOB
    for (int nw = 1; nw <= 4; ++nw) {
        if (g.pgoff[vi][nw - 1] < 0) continue;                     // (every variant of a graph without row maps)
        const int gpw = (32 >> vi) * nw, wps = (g.n + gpw - 1) / gpw;
        const long wgs = (rows / g.n) * wps;
        if (wgs > std::min(g.num_cu, 256)) continue;              // one workgroup per CU, all resident; pers_wait sweeps 256 flags
        const int idcap = (g.pgids[vi][nw - 1] + 3) & ~3, segcap = std::max(4, (g.pgsegs[vi][nw - 1] + 3) & ~3);
        const size_t need = sizeof(float) * ((size_t)2 * H * H + idcap + (size_t)2 * segcap * H + (size_t)segcap * 34 + 8);
        if (need > 150 * 1024) continue;
        if (p) { p->wgs = (int)wgs; p->wps = wps; p->nw = nw; p->map_off = g.pgoff[vi][nw - 1]; p->idcap = idcap; p->segcap = segcap; p->lds = pg_lds_bytes(H, idcap, segcap); }
        return true;
    }
    return false;
}

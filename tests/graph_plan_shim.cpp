// extern "C" face of csrc/gnode_graph_plan.cpp for tests/test_graph_plan.py (ctypes): plan a CSR, read every scalar and array of the
// plan, run the per-call planners for a given CU count.
#include "gnode_graph_plan.h"

extern "C" {
void* gp_plan(const int32_t* rowptr, const int32_t* col, int32_t n, int64_t nnz) { return new GnGraphPlan(gn_plan_graph(rowptr, col, n, nnz)); }
const char* gp_error(void* h) { return ((GnGraphPlan*)h)->error.c_str(); }
void gp_free(void* h) { delete (GnGraphPlan*)h; }

// max_degree, n_bigrow, n_hub, n_seg | present[3] | lds[3] | max_items[3] | pgoff[12] | pgids[12] | pgsegs[12]
void gp_scalars(void* h, int32_t* o) {
    const GnGraphPlan& P = *(GnGraphPlan*)h;
    int k = 0;
    o[k++] = P.max_degree; o[k++] = P.n_bigrow; o[k++] = P.n_hub; o[k++] = P.n_seg;
    for (int i = 0; i < 3; ++i) o[k++] = P.pers[i].present;
    for (int i = 0; i < 3; ++i) o[k++] = P.pers[i].lds;
    for (int i = 0; i < 3; ++i) o[k++] = P.pers[i].max_items;
    for (int i = 0; i < 12; ++i) o[k++] = P.pgoff[i / 4][i % 4];
    for (int i = 0; i < 12; ++i) o[k++] = P.pgids[i / 4][i % 4];
    for (int i = 0; i < 12; ++i) o[k++] = P.pgsegs[i / 4][i % 4];
}

// 0 rowhdr, 1 hubidx, 2 seg_lo, 3 seg_hi, 4 hub_seg_ptr, 5 pgmap, 6 + 4 i + {0 map, 1 hub, 2 segptr, 3 items} of variant i;
// *len = -1 for the arrays of an absent variant
const int32_t* gp_array(void* h, int which, int64_t* len) {
    const GnGraphPlan& P = *(GnGraphPlan*)h;
    const std::vector<int32_t>* v;
    if (which < 6) v = which == 0 ? &P.rowhdr : which == 1 ? &P.hubidx : which == 2 ? &P.seg_lo : which == 3 ? &P.seg_hi : which == 4 ? &P.hub_seg_ptr : &P.pgmap;
    else {
        const GnPers64Maps& M = P.pers[(which - 6) / 4];
        const int j = (which - 6) % 4;
        if (!M.present) { *len = -1; return nullptr; }
        v = j == 0 ? &M.map : j == 1 ? &M.hub : j == 2 ? &M.segptr : &M.items;
    }
    *len = (int64_t)v->size();
    return v->data();
}

// the edge tables, apart from gp_array (tests/golden/graph_plan_parent.json has no entry for them): 0 src, 1 rev
const int32_t* gp_edge_table(void* h, int which, int64_t* len) {
    const GnGraphPlan& P = *(GnGraphPlan*)h;
    const std::vector<int32_t>& v = which == 0 ? P.src : P.rev;
    *len = (int64_t)v.size();
    return v.data();
}
int gp_symmetric(void* h) { return ((GnGraphPlan*)h)->symmetric; }

static int put(bool ok, const PersPlan& q, int32_t* o) {
    if (!ok) return 0;
    const int f[10] = {q.nt, q.wgs, q.span, q.gpx, q.per, q.slots, q.n_xcc, q.rounds, q.concurrent, q.fstride};
    for (int i = 0; i < 10; ++i) o[i] = f[i];
    return 1;
}
int gp_pers64_plan(void* h, int num_cu, long B, int n_steps, int32_t* o) {
    const GnGraphPlan& P = *(GnGraphPlan*)h;
    PersPlan q{};
    return put(gn_pers64_plan(gn_graph_info(P, (int32_t)(P.rowhdr.size() / 20), num_cu), B, n_steps, &q), q, o);
}
int gp_pers_bwd64_plan(void* h, int num_cu, long B, int n_steps, int32_t* o) {
    const GnGraphPlan& P = *(GnGraphPlan*)h;
    PersPlan q{};
    return put(gn_pers_bwd64_plan(gn_graph_info(P, (int32_t)(P.rowhdr.size() / 20), num_cu), B, n_steps, &q), q, o);
}
int gp_persg_plan(void* h, int num_cu, long rows, int H, int n_steps, int64_t* o) {
    const GnGraphPlan& P = *(GnGraphPlan*)h;
    PersgPlan q{};
    if (!gn_persg_plan(gn_graph_info(P, (int32_t)(P.rowhdr.size() / 20), num_cu), rows, H, n_steps, &q)) return 0;
    const int64_t f[7] = {q.wgs, q.wps, q.nw, q.map_off, q.idcap, q.segcap, (int64_t)q.lds};
    for (int i = 0; i < 7; ++i) o[i] = f[i];
    return 1;
}
// GN_HUB_T, HUB_SEG, PERS_MAX_ITEMS, PERS_MAX_PARTIALS, kPersMaxRows, GN_SIR_BIGROW
int gp_const(int w) { return w == 0 ? GN_HUB_T : w == 1 ? HUB_SEG : w == 2 ? PERS_MAX_ITEMS : w == 3 ? PERS_MAX_PARTIALS : w == 4 ? kPersMaxRows : GN_SIR_BIGROW; }
}

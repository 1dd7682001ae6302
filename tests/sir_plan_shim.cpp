// extern "C" face of csrc/gnode_sir_plan.cpp for tests/test_sir_plan.py (ctypes): one case's layout and launch plan as a row of
// integers, coin_threshold, and the staging function.  With -DSIR_PLAN_MAIN it is a program instead: it reads a case file and
// prints the rows tests/golden/make_sir_plan_parent.cpp prints, then stages a few inputs (the sanitizer build's subject).
#include "gnode_sir_plan.h"
#include <cstdio>
#include <cstring>

extern "C" {
// five workspace sizes (scalar, nodes, edges, init, traj) | offsets of seeds, row expansion, tail, rate and start thresholds |
// lists_in_lds, frontier threads, per CU, LDS bytes | path, grid, threads, dynamic LDS of the launch
void sp_case(int n, int64_t nnz, int nb, int T, int cu, int64_t sims, int edge_scan, int64_t* o) {
    const SirLayout L = sir_layout(n, nnz, nb, T);
    int per_cu = 1;
    const int threads = frontier_threads(n, nb, &per_cu);
    const SirLaunch P = sir_launch_plan(n, nb, cu, sims, edge_scan != 0);
    const int64_t row[18] = {(int64_t)L.bytes[SIR_SCALAR], (int64_t)L.bytes[SIR_NODES], (int64_t)L.bytes[SIR_EDGES], (int64_t)L.bytes[SIR_INIT],
                             (int64_t)L.bytes[SIR_NODES], (int64_t)L.seeds, (int64_t)L.rows, (int64_t)L.tail, (int64_t)L.thr, (int64_t)L.start,
                             frontier_lists_in_lds(n, nb), threads, per_cu, (int64_t)frontier_lds_bytes(n, nb, threads),
                             (int64_t)P.path, P.grid, P.threads, (int64_t)P.lds};
    memcpy(o, row, sizeof row);
}
unsigned long long sp_coin(double p) { return coin_threshold(p); }

// the error text ("" = accepted); scalars[2], rates[n_rates], start[n_start] receive the thresholds (room for nnz + n and 2n)
const char* sp_stage(int n, int64_t nnz, int form, double beta, double gamma, const double* bn, const double* gn, const double* w,
                     const int32_t* col, const double* init, unsigned long long* scalars, unsigned long long* rates, int64_t* n_rates,
                     unsigned long long* start, int64_t* n_start) {
    static std::string err;
    SirRates r;
    r.form = form; r.beta = beta; r.gamma = gamma; r.beta_nodes = bn; r.gamma_nodes = gn; r.w_edges = w;
    const SirThresholds t = sir_stage("entry", n, nnz, r, col, init);
    scalars[0] = t.tb; scalars[1] = t.tg;
    *n_rates = (int64_t)t.rates.size(); *n_start = (int64_t)t.start.size();
    if (!t.rates.empty()) memcpy(rates, t.rates.data(), t.rates.size() * sizeof(unsigned long long));
    if (!t.start.empty()) memcpy(start, t.start.data(), t.start.size() * sizeof(unsigned long long));
    err = t.error;
    return err.c_str();
}
}

#ifdef SIR_PLAN_MAIN
int main(int argc, char** argv) {
    FILE* f = argc > 1 ? fopen(argv[1], "r") : nullptr;
    if (!f) return 2;
    long n, nnz, nb, T, cu, sims, es;
    while (fscanf(f, "%ld %ld %ld %ld %ld %ld %ld", &n, &nnz, &nb, &T, &cu, &sims, &es) == 7) {
        int64_t o[18];
        sp_case((int)n, nnz, (int)nb, (int)T, (int)cu, sims, (int)es, o);
        for (int i = 0; i < 18; ++i) printf("%lld%c", (long long)o[i], i == 17 ? '\n' : ' ');
    }
    fclose(f);
    const double ps[] = {0.0, 1.0, 0x1p-33, 1.0 - 0x1p-33, 0.3, 0x1p-32, 0.5};
    for (double p : ps) printf("coin %llu\n", coin_threshold(p));
    // staging: every rate form with and without a start, the restated per-node form, and a refusal of each kind
    const int sn = 5;
    const int32_t col[6] = {1, 0, 2, 1, 4, 3};
    double bn[5] = {0.1, 0.2, 0.3, 0.4, 0.5}, w[6] = {0.0, 1.0, 0.5, 0.25, 0.3, 0.7}, init[15];
    for (int v = 0; v < sn; ++v) { init[3 * v] = 0.5; init[3 * v + 1] = 0.25; init[3 * v + 2] = 0.25; }
    unsigned long long sc[2], rates[11], start[10];
    int64_t nr, ns;
    for (int form = 0; form < 3; ++form)
        for (int k = 0; k < 8; ++k) {
            double gn[5] = {0.5, 0.5, k & 4 ? 1.5 : 0.5, 0.5, 0.5};
            const char* e = sp_stage(sn, 6, form, 0.3, 0.2, bn, (k & 1) || form == 1 ? gn : nullptr, w, (k & 2) && form == 1 ? col : nullptr,
                                     (k & 2) ? init : nullptr, sc, rates, &nr, start, &ns);
            printf("stage %d %d: %lld %lld %s\n", form, k, (long long)nr, (long long)ns, e);
        }
    init[4] = 0.2500021;
    printf("stage: %s\n", sp_stage(sn, 6, 0, 0.3, 0.2, nullptr, nullptr, nullptr, nullptr, init, sc, rates, &nr, start, &ns));
    return 0;
}
#endif

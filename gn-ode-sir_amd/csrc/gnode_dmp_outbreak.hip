// Whom to immunise and where to seed (Lokhov, Saad 2017): the DMP recurrence of gnode_dmp.h from every candidate intervention on
// one outbreak, kept only as the expected size of each compartment over time -- gnode_dmp_outbreak_sizes_f32.
//
// The candidate sweep of gnode_dmp_sweep.h -- its two forms, kernels, workspace, preamble and launches -- with this unit's
// reader.  Candidate c's sample is DMP from the shared base start init[n][3] = (pS, pI, pR) per node with the triple of node
// cand[c] replaced: action 0 (seed) makes it (0, 1, 0), action 1 (immunise) makes it (0, 0, 1); an id outside the graph (-1 by
// convention) matches no node and gives the base start itself.  The recurrence is called as gnode_dmp.hip calls it for an
// `init` start (Pr_0 from the triple, phi_0 = Pi_0), so the fp32 marginals are gnode_dmp_batch_f32's bit for bit.  Three sums
// per candidate and step:
//   sizes[c][t][j] = sum_k (double)value[k] * (double)P^k_j(t),      j = 0 / 1 / 2 for S / I / R; value == null: 1 for every k
// (the product of two floats is exact in a double).
#include "gnode_dmp_sweep.h"

struct DmpOutbreakArgs : DmpSweepArgs {
    const float* init;                          // [n][3], the base start
    const float* value;                         // [n] or null
    int action;                                 // 0 seed, 1 immunise
    double* sizes;                              // [C][maxTime][3]
};
struct DmpOutbreakReader {
    using Args = DmpOutbreakArgs;
    struct Terms { double s, i, r; };
    static constexpr int W = 3;
    static constexpr bool kTiled = false;
    // the start of node k in the sample of candidate `cand`: the base triple, or the action's where k is the candidate
    static __device__ __forceinline__ void start(const Args& a, int k, int cand, float& ps0, float& pi0, float& pr0) {
        const bool hit = k == cand;
        const float seeded = a.action == 0 ? 1.0f : 0.0f;
        ps0 = hit ? 0.0f : a.init[(size_t)k * 3];
        pi0 = hit ? seeded : a.init[(size_t)k * 3 + 1];
        pr0 = hit ? 1.0f - seeded : a.init[(size_t)k * 3 + 2];
    }
    // ... and its Ps_0 alone, which is all that the steps after the first read of it: 0 under either action
    static __device__ __forceinline__ float ps0(const Args& a, int k, int cand) { return k == cand ? 0.0f : a.init[(size_t)k * 3]; }
    static __device__ __forceinline__ Terms terms(const Args& a, int k, float ps, float pi, float pr, float, float) {
        const double v = a.value ? (double)a.value[k] : 1.0;
        return {v * (double)ps, v * (double)pi, v * (double)pr};
    }
    static __device__ __forceinline__ double pick(const Args&, const Terms& l, int, int j0, int w) {
        return j0 + w == 0 ? l.s : j0 + w == 1 ? l.i : l.r;
    }
    static __device__ __forceinline__ double* out(const Args& a, size_t ct, size_t j) { return a.sizes + (ct * 3 + j); }
};

extern "C" size_t gnode_dmp_outbreak_lds_bytes(gnode_graph_t g) { return dmp_sweep_lds_bytes<DmpOutbreakReader>(g); }
int gn_dmp_outbreak_set_attributes() { return dmp_sweep_set_attributes<DmpOutbreakReader>(); }
extern "C" size_t gnode_dmp_outbreak_workspace_bytes(gnode_graph_t g, int32_t C, int32_t maxTime) {
    return dmp_sweep_workspace_bytes<DmpOutbreakReader>(g, C, maxTime, 3);
}

// Nothing here waits on the host: the call only enqueues work.
extern "C" int gnode_dmp_outbreak_sizes_f32(gnode_graph_t g, const float* weights, const float* gamma, const float* init,
                                            const int32_t* candidates, int32_t C, int32_t action, const float* value, int32_t maxTime,
                                            double* sizes, void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "gnode_dmp_outbreak_sizes_f32";
    if (int e = dmp_sweep_arguments(who, g, gamma && init && candidates && sizes && workspace, weights, maxTime, C)) return e;
    GN_CHECK_ARG(action == 0 || action == 1, "%s: action must be 0 (seed) or 1 (immunise) (got %d)", who, action);
    const DmpOutbreakArgs a = {{}, init, value, action, sizes};
    return dmp_sweep_run<DmpOutbreakReader>(who, "", g, weights, gamma, candidates, C, maxTime, 3, a, false, workspace, workspace_bytes, stream);
}

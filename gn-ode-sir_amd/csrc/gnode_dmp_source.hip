// Source inference from one snapshot (Lokhov, Mezard, Ohta, Zdeborova 2014): the DMP recurrence of gnode_dmp.h from every
// candidate source, scored by the mean-field likelihood of the observed states -- gnode_dmp_source_scores_f32.
//
// The candidate sweep of gnode_dmp_sweep.h -- its two forms, kernels, workspace, preamble and launches -- with this unit's
// reader: candidate c's sample is DMP from the one-hot seed state (1 - [k == cand_c], [k == cand_c], 0) (DmpOneHotStart), and
// at every step the node pass forms for obs[k] in {0, 1, 2}
//   log((double)min(max(p, floor), 1.0f)),      p = Ps / Pi / Pr by obs[k]
// (dmp_source_term of gnode_dmp.h), and any other obs[k] contributes nothing (so no device value indexes anything).  The clamp is
// fp32: Pi = 1 - Ps - Pr can round below 0, Ps can exceed 1 by the 1e-10 offset, and a node outside the t-ball of the candidate
// has probability exactly 0.  One sum per candidate and step:
//   scores[c][t] = sum_k term_k.
#include "gnode_dmp_sweep.h"

struct DmpSourceArgs : DmpSweepArgs {
    const int32_t* obs;                         // [n]
    float floor;
    double* scores;                             // [C][maxTime]
};
struct DmpSourceReader : DmpOneHotStart {
    using Args = DmpSourceArgs;
    using Rates = DmpConstantRates;
    using Terms = double;
    static constexpr int W = 1;
    static constexpr bool kTiled = false;
    static __device__ __forceinline__ Terms terms(const Args& a, int k, float ps, float pi, float pr, float, float) {
        return dmp_source_term(a.obs[k], ps, pi, pr, a.floor);
    }
    static __device__ __forceinline__ double pick(const Args&, const Terms& l, int, int, int) { return l; }
    static __device__ __forceinline__ double* out(const Args& a, size_t ct, size_t) { return a.scores + ct; }
};

extern "C" size_t gnode_dmp_source_lds_bytes(gnode_graph_t g) { return dmp_sweep_lds_bytes<DmpSourceReader>(g); }
int gn_dmp_source_set_attributes() { return dmp_sweep_set_attributes<DmpSourceReader>(); }
extern "C" size_t gnode_dmp_source_workspace_bytes(gnode_graph_t g, int32_t C, int32_t maxTime) {
    return dmp_sweep_workspace_bytes<DmpSourceReader>(g, C, maxTime, 1);
}

extern "C" int gnode_dmp_source_scores_f32(gnode_graph_t g, const float* weights, const float* gamma, const int32_t* candidates, int32_t C,
                                           const int32_t* obs, float floor, int32_t maxTime, double* scores, void* workspace,
                                           size_t workspace_bytes, void* stream) {
    const char* who = "gnode_dmp_source_scores_f32";
    if (int e = dmp_sweep_arguments(who, g, gamma && candidates && obs && scores && workspace, weights, maxTime, C)) return e;
    GN_CHECK_ARG(floor > 0.0f && floor <= 1.0f, "%s: floor must be in (0, 1] (got %g)", who, (double)floor);      // (a NaN fails it)
    const DmpSourceArgs a = {{}, obs, floor, scores};
    // (wait_first: nothing waits on the host here: only the documented contract (include/gnode.h) keeps it)
    return dmp_sweep_run<DmpSourceReader>(who, "", g, weights, gamma, candidates, C, maxTime, 1, a, true, workspace, workspace_bytes, stream);
}

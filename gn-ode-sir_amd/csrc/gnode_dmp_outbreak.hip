// Whom to immunise and where to seed (Lokhov, Saad 2017): the DMP recurrence of gnode_dmp.h from every candidate intervention on
// one outbreak, kept only as the expected size of each compartment over time -- gnode_dmp_outbreak_sizes_f32.
//
// The candidate sweep of gnode_dmp_sweep.h -- its two forms, kernels, workspace, preamble and launches -- with the outbreak
// reader (DmpOutbreakReader, in the header: gnode_dmp_outbreak_schedule.hip shares it).  Candidate c's sample is DMP from the shared base start init[n][3] = (pS, pI, pR) per node with the triple of node
// cand[c] replaced: action 0 (seed) makes it (0, 1, 0), action 1 (immunise) makes it (0, 0, 1); an id outside the graph (-1 by
// convention) matches no node and gives the base start itself.  The recurrence is called as gnode_dmp.hip calls it for an
// `init` start (Pr_0 from the triple, phi_0 = Pi_0), so the fp32 marginals are gnode_dmp_batch_f32's bit for bit.  Three sums
// per candidate and step:
//   sizes[c][t][j] = sum_k (double)value[k] * (double)P^k_j(t),      j = 0 / 1 / 2 for S / I / R; value == null: 1 for every k
// (the product of two floats is exact in a double).
#include "gnode_dmp_sweep.h"

extern "C" size_t gnode_dmp_outbreak_lds_bytes(gnode_graph_t g) { return dmp_sweep_lds_bytes<DmpOutbreakReader>(g); }
int gn_dmp_outbreak_set_attributes() { return dmp_sweep_set_attributes<DmpOutbreakReader>(); }
extern "C" size_t gnode_dmp_outbreak_workspace_bytes(gnode_graph_t g, int32_t C, int32_t maxTime) {
    return dmp_sweep_workspace_bytes<DmpOutbreakReader>(g, C, maxTime, 3);
}

// Nothing here waits on the host: the call only enqueues work.
extern "C" int gnode_dmp_outbreak_sizes_f32(gnode_graph_t g, const float* weights, const float* gamma, const float* init,
                                            const int32_t* candidates, int32_t C, int32_t action, const float* value, int32_t maxTime,
                                            double* sizes, void* workspace, size_t workspace_bytes, void* stream) {
    return dmp_outbreak_sizes<DmpOutbreakReader>("gnode_dmp_outbreak_sizes_f32", g, weights, gamma, init, candidates, C, action, value, maxTime,
                                                 sizes, workspace, workspace_bytes, stream);
}

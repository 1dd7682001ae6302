// DMP with rates that change over time -- gnode_dmp_batch_schedule_f32.
//
// gnode_dmp_batch.h's forward under DmpBatchScheduledRates: P tables of weights and of recovery probabilities per sample and a
// phase row that names, per step, which of them governs it.  Step t = 1 .. maxTime-1 leads from state t-1 to state t under tables
// p = phase[t]:
//   theta_1     = (1 - w^{phase[1]} phi_0) + 1e-10                               dmp_edge_start with step 1's weights
//   node pass t   Pr_t = Pr_{t-1} + gamma^p Pi_{t-1};  Ps_t, Pi_t as ever       dmp_node_update with step t's gamma
//   edge pass t   phi_t = (1 - w^p)(1 - gamma^p_src) phi_{t-1} - (Ps_e(t) - Ps_e(t-1))
//                 theta_{t+1} = theta_t - w^{phase[t+1]} phi_t                   dmp_edge_update with two weights
// phi_t is the probability that the source is infected and has neither transmitted nor recovered up to step t: what happened
// DURING step t, under step t's tables.  theta_{t+1} - theta_t is the probability of a transmission during step t + 1: the next
// step's weight.  The edge pass runs only when t + 1 < maxTime, so phase[t + 1] exists wherever it is read.  The arithmetic is
// gnode_dmp.h's and nothing else, so one phase -- or several holding equal tables -- returns gnode_dmp_batch_f32's bits.
#include "gnode_dmp_batch.h"

using DmpScheduled = DmpBatchScheduledRates;

int gn_dmp_schedule_set_attributes() { return dmp_batch_set_attributes<DmpScheduled>(); }

extern "C" size_t gnode_dmp_batch_schedule_workspace_bytes(gnode_graph_t g, int32_t B, int32_t maxTime) {
    return g && B >= 1 && maxTime >= 2 ? dmp_carve<DmpScheduled>(g, (size_t)B, (size_t)maxTime, !dmp_batch_one_workgroup(g), false, nullptr).bytes
                                       : 0;
}

// Synchronises the stream after staging the phase row (and while validating the tables) and again before returning.
extern "C" int gnode_dmp_batch_schedule_f32(gnode_graph_t g, const float* weights, int64_t w_stride, const float* gamma, int64_t gamma_stride,
                                            const int32_t* phase_host, int32_t P, const float* init, int32_t B, int32_t maxTime, float* out,
                                            void* workspace, size_t workspace_bytes, void* stream) {
    const DmpSchedule schedule = {phase_host, P};
    GN_CHECK_ARG(init, "gnode_dmp_batch_schedule_f32: null pointer");
    return dmp_run<DmpScheduled>("gnode_dmp_batch_schedule_f32", g, weights, (long)w_stride, gamma, (long)gamma_stride, init, nullptr, 0, B,
                                 maxTime, out, false, workspace, workspace_bytes, stream, schedule);
}

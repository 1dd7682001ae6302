// The reverse sweep of DMP with rates that change over time -- gnode_dmp_batch_schedule_backward_f32: the gradient of
// sum(grad_out * out) with respect to each phase's weights and recovery probabilities and to the start, where `out` is what
// gnode_dmp_batch_schedule_f32 returned.
//
// gnode_dmp_batch.h's reverse sweep under DmpBatchScheduledRates, which knows which table each step's adjoint belongs to (the
// header tells it pass by pass): theta_{t+1}'s weight gradient goes to step t + 1's table, phi_t's to step t's, and a phase no
// step names keeps the zeros the entry wrote.  The tape runs the scheduled forward's own arithmetic, so it holds the forward's
// bits.  One phase, or several holding equal tables summed over the phases, is gnode_dmp_batch_backward_f32's sweep.
#include "gnode_dmp_batch.h"

using DmpScheduled = DmpBatchScheduledRates;

int gn_dmp_schedule_bwd_set_attributes() { return dmp_grad_set_attributes<DmpScheduled>(); }

extern "C" size_t gnode_dmp_batch_schedule_backward_workspace_bytes(gnode_graph_t g, int32_t B, int32_t maxTime) {
    return g && B >= 1 && maxTime >= 2 ? dmp_grad_carve<DmpScheduled>(g, (size_t)B, (size_t)maxTime, !dmp_grad_one_workgroup(g), nullptr).bytes
                                       : 0;
}

// Synchronises the stream after staging the phase row (and while validating the tables) and again before returning.
extern "C" int gnode_dmp_batch_schedule_backward_f32(gnode_graph_t g, const float* weights, int64_t w_stride, const float* gamma,
                                                     int64_t gamma_stride, const int32_t* phase_host, int32_t P, const float* init, int32_t B,
                                                     int32_t maxTime, const float* out, const float* grad_out, float* grad_w,
                                                     float* grad_gamma, float* grad_init, void* workspace, size_t workspace_bytes,
                                                     void* stream) {
    const DmpSchedule schedule = {phase_host, P};
    return dmp_grad_run<DmpScheduled>("gnode_dmp_batch_schedule_backward_f32", g, weights, (long)w_stride, gamma, (long)gamma_stride, init, B,
                                      maxTime, out, grad_out, grad_w, grad_gamma, grad_init, false, workspace, workspace_bytes, stream,
                                      schedule);
}

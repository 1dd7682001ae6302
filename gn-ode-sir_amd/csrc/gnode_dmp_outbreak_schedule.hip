// Whom to immunise and where to seed when the rates change over time -- gnode_dmp_outbreak_sizes_schedule_f32.
//
// gnode_dmp_outbreak.hip's reader, DmpOutbreakReader, with the scheduled rates of gnode_dmp_sweep.h (DmpScheduled): P tables of
// weights and of recovery probabilities, a phase row stated in calendar steps, and per sample a candidate id and a SHIFT.  Step
// t = 1 .. maxTime - 1 of sample j is governed by phase[shift[j] + t]: shift 0 for everybody is "the schedule counts from the
// outbreak's start", and the candidate -1 (no change) with the shifts 0 .. K - 1 is "what does each step of delay cost".  The
// recurrence is gnode_dmp_batch_schedule_f32's from the candidate's start, under the row phase[shift : shift + maxTime], bit for
// bit; with one phase, or several of equal tables, the sizes are gnode_dmp_outbreak_sizes_f32's.
#include "gnode_dmp_sweep.h"

using DmpOutbreakScheduled = DmpScheduled<DmpOutbreakReader>;

int gn_dmp_outbreak_schedule_set_attributes() { return dmp_sweep_set_attributes<DmpOutbreakScheduled>(); }
extern "C" size_t gnode_dmp_outbreak_schedule_workspace_bytes(gnode_graph_t g, int32_t C, int32_t maxTime, int32_t L) {
    return dmp_sweep_schedule_workspace_bytes<DmpOutbreakScheduled>(g, C, maxTime, 3, L);
}

// Synchronises the stream once, after staging the phase row and the shifts (and while validating the tables).
extern "C" int gnode_dmp_outbreak_sizes_schedule_f32(gnode_graph_t g, const float* weights, const float* gamma, const int32_t* phase_host,
                                                     int32_t P, int32_t L, const float* init, const int32_t* candidates,
                                                     const int32_t* shifts_host, int32_t C, int32_t action, const float* value, int32_t maxTime,
                                                     double* sizes, void* workspace, size_t workspace_bytes, void* stream) {
    const DmpSweepSchedule schedule = {phase_host, P, L, shifts_host};
    return dmp_outbreak_sizes<DmpOutbreakScheduled>("gnode_dmp_outbreak_sizes_schedule_f32", g, weights, gamma, init, candidates, C, action, value,
                                                    maxTime, sizes, workspace, workspace_bytes, stream, &schedule);
}

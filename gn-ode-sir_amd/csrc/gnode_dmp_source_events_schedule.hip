// Source inference under rates that change over time -- gnode_dmp_source_events_scores_schedule_f32.
//
// gnode_dmp_source_events.hip's reader, DmpRowsReader<DmpEventTerms>, with the scheduled rates of gnode_dmp_sweep.h
// (DmpScheduled): P tables of weights and of recovery probabilities, a phase row stated in CALENDAR steps, and per sample a
// candidate id and a SHIFT.  Step t = 1 .. maxTime - 1 of sample j is governed by phase[shift[j] + t]: a hypothesis "c started
// tau steps before the snapshot of calendar step D" is the sample (c, D - tau) read at t = tau.  The recurrence is
// gnode_dmp_batch_schedule_f32's from the one-hot start, under the row phase[shift : shift + maxTime], bit for bit; with one
// phase, or several of equal tables, every row is gnode_dmp_source_events_scores_f32's.  A row of codes -1 .. 2 is the
// snapshot and batch entries' row, so this one instance serves all three under a schedule.
#include "gnode_dmp_sweep.h"

using DmpEventsScheduled = DmpScheduled<DmpRowsReader<DmpEventTerms>>;

int gn_dmp_source_events_schedule_set_attributes() { return dmp_sweep_set_attributes<DmpEventsScheduled>(); }
extern "C" size_t gnode_dmp_source_events_schedule_workspace_bytes(gnode_graph_t g, int32_t C, int32_t R, int32_t maxTime, int32_t L) {
    return dmp_sweep_schedule_workspace_bytes<DmpEventsScheduled>(g, C, maxTime, R, L);
}

extern "C" int gnode_dmp_source_events_scores_schedule_f32(gnode_graph_t g, const float* weights, const float* gamma,
                                                           const int32_t* phase_host, int32_t P, int32_t L, const int32_t* candidates,
                                                           const int32_t* shifts_host, int32_t C, const int8_t* rows, int32_t R, float floor,
                                                           int32_t maxTime, double* scores, int64_t score_stride, void* workspace,
                                                           size_t workspace_bytes, void* stream) {
    const DmpSweepSchedule schedule = {phase_host, P, L, shifts_host};
    return dmp_rows_scores<DmpEventTerms, DmpEventsScheduled>("gnode_dmp_source_events_scores_schedule_f32", "R", g, weights, gamma, candidates,
                                                              C, rows, R, floor, maxTime, scores, score_stride, workspace, workspace_bytes,
                                                              stream, &schedule);
}

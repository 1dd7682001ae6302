// Source inference from time-stamped evidence in one DMP pass -- gnode_dmp_source_events_scores_f32.
//
// gnode_dmp_source_batch.hip scores O snapshots: rows of STATES at one common step.  Outbreak data is events -- the step at which
// a node was infected, the step at which it recovered -- and DMP gives those too: node k becomes infected AT step t with
// probability Ps_k(t-1) - Ps_k(t) and recovers AT step t with probability Pr_k(t) - Pr_k(t-1).  The sweep's node pass
// (gnode_dmp_sweep.h) hands both previous values to its reader: Pr(t-1) is the pr_prev its update reads, Ps(t-1) is
// ps0 * P_old[k] on the product it is about to overwrite (ps0 itself at t = 1, where no product exists yet), and before the
// start Ps(-1) = 1, Pr(-1) = 0.  So a row code may be 3 ("infected at this step") or 4 ("recovered at this step") next to
// 0 / 1 / 2: this unit is the rows-of-codes reader (DmpRowsReader) with the FIVE possible terms, computed once per node and
// step (dmp_source_event_logs of gnode_dmp.h), of which every row selects one, or 0.0 (dmp_source_event_pick).  The contract:
//   scores[r * score_stride + c * maxTime + t]; a row whose codes are all outside 3 / 4 is bit for bit
//   gnode_dmp_source_batch_scores_f32's row, and so gnode_dmp_source_scores_f32's table for that row alone:
// the first three of the five are that unit's doubles, and everything else is the same sweep.
#include "gnode_dmp_sweep.h"

extern "C" int gnode_dmp_source_events_tile(gnode_graph_t g) { return dmp_rows_tile<DmpEventTerms>(g); }
int gn_dmp_source_events_set_attributes() { return dmp_sweep_set_attributes<DmpRowsReader<DmpEventTerms>>(); }
extern "C" size_t gnode_dmp_source_events_workspace_bytes(gnode_graph_t g, int32_t C, int32_t R, int32_t maxTime) {
    return dmp_sweep_workspace_bytes<DmpRowsReader<DmpEventTerms>>(g, C, maxTime, R);
}

extern "C" int gnode_dmp_source_events_scores_f32(gnode_graph_t g, const float* weights, const float* gamma, const int32_t* candidates,
                                                  int32_t C, const int8_t* rows, int32_t R, float floor, int32_t maxTime, double* scores,
                                                  int64_t score_stride, void* workspace, size_t workspace_bytes, void* stream) {
    return dmp_rows_scores<DmpEventTerms>("gnode_dmp_source_events_scores_f32", "R", g, weights, gamma, candidates, C, rows, R, floor, maxTime,
                                          scores, score_stride, workspace, workspace_bytes, stream);
}

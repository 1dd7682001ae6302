// Source inference from MANY snapshots in one DMP pass -- gnode_dmp_source_batch_scores_f32.
//
// gnode_dmp_source.hip scores one snapshot: a candidate's marginals Ps, Pi, Pr do not depend on the observation, and only the
// last instructions of its node pass read obs.  Here O snapshots obs[O][n] (int8) are scored where the node pass holds the
// marginals in registers: the rows-of-codes reader of gnode_dmp_sweep.h (DmpRowsReader, with its tile, its entry and the sweep
// behind them) with this unit's terms -- per node and step the three possible terms log((double)min(max(p, floor), 1.0f)),
// p = Ps / Pi / Pr, computed once (dmp_source_logs of gnode_dmp.h), of which every observation selects one, or 0.0
// (dmp_source_pick).  The contract:
//   scores[o * score_stride + c * maxTime + t]  is bit for bit what gnode_dmp_source_scores_f32 writes at [c][t] for obs[o] alone.
// That holds because both are the one sweep: the form is chosen by the same predicate (a tiled reader needs room for one sum,
// as the solo reader does), the launch shapes are the same, and every observation's sum is taken in the same order.
#include "gnode_dmp_sweep.h"

struct DmpSnapshotTerms {
    using Logs = DmpSourceLogs;
    static __device__ __forceinline__ Logs logs(float ps, float pi, float pr, float, float, float floor) { return dmp_source_logs(ps, pi, pr, floor); }
    static __device__ __forceinline__ double pick(int o, const Logs& l) { return dmp_source_pick(o, l); }
};

extern "C" int gnode_dmp_source_batch_tile(gnode_graph_t g) { return dmp_rows_tile<DmpSnapshotTerms>(g); }
int gn_dmp_source_batch_set_attributes() { return dmp_sweep_set_attributes<DmpRowsReader<DmpSnapshotTerms>>(); }
extern "C" size_t gnode_dmp_source_batch_workspace_bytes(gnode_graph_t g, int32_t C, int32_t O, int32_t maxTime) {
    return dmp_sweep_workspace_bytes<DmpRowsReader<DmpSnapshotTerms>>(g, C, maxTime, O);
}

extern "C" int gnode_dmp_source_batch_scores_f32(gnode_graph_t g, const float* weights, const float* gamma, const int32_t* candidates,
                                                 int32_t C, const int8_t* obs, int32_t O, float floor, int32_t maxTime, double* scores,
                                                 int64_t score_stride, void* workspace, size_t workspace_bytes, void* stream) {
    return dmp_rows_scores<DmpSnapshotTerms>("gnode_dmp_source_batch_scores_f32", "O", g, weights, gamma, candidates, C, obs, O, floor, maxTime,
                                             scores, score_stride, workspace, workspace_bytes, stream);
}

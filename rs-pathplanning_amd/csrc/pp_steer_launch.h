// pp_steer_launch.h — the host launch layer of the steer round (steer_prep_kernel, then
// steer_walk_kernel), implemented in pp_k_steer.hip, the one unit that compiles those kernels.
// The window, check_finish, query-batch and RRT* units run the round on their own tasks through
// these functions.  Internal to the kernel units (the C API goes through pp_kernels.h).
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>

#include "pp_types.h"

namespace ppamd {

// Which steer_walk_kernel a subsystem runs (its register budget kMinW and whether S segments are
// classified analytically, kS) and how many of its workgroups share a CU at most:
//   kWalkWindow      <kWalkMinWWindow, kS false>, 4 per CU   the window pipeline
//   kWalkBatchPlan   <kWalkMinWBatch, true>, 4               check_finish's rounds of a query batch
//   kWalkBatchBig    <kWalkMinWBatch, true>, 2               a query-batch step of >= kBigStepTasks
//   kWalkBatchSmall  <kWalkMinWBatch - 1, true>, 2           a smaller query-batch step
//   kWalkStar        <kWalkMinWStar, true>, 4                the RRT* rounds and goal connection
// (2 per CU: the query batch's walk runs beside the other sub-batch stream's kernels.)
enum WalkProfile : int {
    kWalkWindow = 0,
    kWalkBatchPlan,
    kWalkBatchBig,
    kWalkBatchSmall,
    kWalkStar
};

constexpr int kWalkMaxWG = 768;  // 3 resident workgroups per CU

// The walk's persistent grid for the profile's kernel on this scene: CUs x resident workgroups
// per CU (the occupancy API's figure, capped by the profile), cached per (profile, device, LDS
// image size, scene kind).
int walk_grid_cap(WalkProfile p, const SceneDev& sc);

// The most workgroups a walk of the profile is launched with.
inline int walk_grid_limit(WalkProfile p, const SceneDev& sc) {
    return std::min(kWalkMaxWG, walk_grid_cap(p, sc));
}
// The walk's grid for `tasks` tasks, one per wave, under a limit.
inline int walk_blocks(int tasks, int limit) {
    return std::min((tasks + kWalkThreads / 64 - 1) / (kWalkThreads / 64), limit);
}

// steer_walk_kernel over a task set on stream s (the profile's instantiation for the scene)
void launch_walk(WalkProfile p, hipStream_t s, int blocks, DevState* st, const SceneDev& sc,
                 const PrepRec* rec, CandEntry* cand, int* status, const int* cand_cnt, int* pend,
                 long long* wg_points);

// steer_prep_kernel over a window's snapshot and candidate tasks
void launch_prep_window(hipStream_t s, int blocks, const DevState* st, const SceneDev& sc,
                        const double* wsx, const double* wsy, const double* snap_pose,
                        CandEntry* cand, PrepRec* rec, double* snap_yaw);
// ... and over explicit (child, parent pose) tasks: yaw[t] the child's heading, cost (optional)
// the edge's Dubins cost, ext (optional) RRT*'s own-yaw children and cull limits
void launch_prep_tasks(hipStream_t s, int blocks, const DevState* st, const SceneDev& sc,
                       PrepRec* rec, double* yaw, const SteerTask* tasks, double* cost = nullptr,
                       const StarTaskExt* ext = nullptr);

}  // namespace ppamd

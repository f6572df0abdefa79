// pp_chain_dev.h — the chains of poses whose consecutive pairs are a planned path's Dubins edges,
// shared by the line kernels (pp_k_finish.hip: check_finish, cf_line_kernel, paths_kernel) and
// the segment export (pp_k_segments.hip): a pose, a node's ancestor path, and the two pose providers.
#pragma once

#include <hip/hip_runtime.h>

#include "pp_types.h"

namespace ppamd {

struct CfPose {
    double x, y, yaw;
};

// A node's ancestor path root first into path[0, D) (NodeIter, rrt.rs:253-265, reversed), by the
// calling wave (lane 0 follows the parents, then the lanes reverse it); -1 past kCfMaxDepth.
__device__ inline int cf_path(const TreeDev& tr, int node, int* __restrict__ path,
                              int cap = kCfMaxDepth) {
    const int lane = __lane_id();
    int d = 0;
    if (lane == 0) {
        int c = node;
        while (c >= 0 && d < cap) {
            path[d++] = c;
            c = tr.parent[c];
        }
        if (c >= 0) d = -1;
    }
    d = __shfl(d, 0);
    __builtin_amdgcn_wave_barrier();
    if (d > 0)
        for (int i = lane; i < d / 2; i += 64) {
            const int t = path[i];
            path[i] = path[d - 1 - i];
            path[d - 1 - i] = t;
        }
    __builtin_amdgcn_wave_barrier();
    return d;
}

// The pose providers: pose(j), j = 0 .. edges(), edge e runs from pose(e) to pose(e + 1).
//   CfChainPoses    finalize's chain (check_finish_kernel's pose(j)): the goal, optimize's copies,
//                   the tree path down to the root; the root contributes no point
//   StarChainPoses  pp_star_path's chain: the goal with its own yaw, then the stored poses of the
//                   node, its parent, ..., the root (a rewired node keeps its pose, so no edge
//                   uses compute_yaw); the root's point ends the forward line
//   CsrChainPoses   the same over a caller-supplied chain of tree nodes (below)
struct CfChainPoses {
    static constexpr bool kRootPoint = false;  // finalize: the root contributes no point
    static constexpr bool kGoalNoneOk = false;
    TreeDev tr;
    const int* path;
    const int* pos;
    int D, s, ps;
    double gx, gy, gyaw;
    __device__ CfChainPoses(const TreeDev& t, const int* path_, int D_, const int* o,
                            const int* pos_, const double* goal)
        : tr(t), path(path_), pos(pos_), D(D_), s(o[1]), gx(goal[0]), gy(goal[1]), gyaw(goal[2]) {
        ps = s > 0 ? pos[s - 1] : D - 1;
    }
    __device__ int edges() const { return 1 + s + ps; }
    __device__ CfPose pose(int j) const {
        if (j == 0) return CfPose{gx, gy, gyaw};  // (a batch's goal: gyaw_opt == gyaw)
        if (j <= s) {
            const int i = j - 1;
            const int here = path[i == 0 ? D - 1 : pos[i - 1]];
            const int to = path[pos[i]];
            const double x = tr.x[here], y = tr.y[here];
            return CfPose{x, y, atan2(tr.y[to] - y, tr.x[to] - x)};  // Node::new (compute_yaw)
        }
        const int node = path[ps - (j - s - 1)];
        return CfPose{tr.x[node], tr.y[node], tr.yaw[node]};
    }
};

struct StarChainPoses {
    static constexpr bool kRootPoint = true;
    static constexpr bool kGoalNoneOk = true;  // a goal edge without a word: ok 0, an empty row
    TreeDev tr;
    const int* path;
    int D;
    double gx, gy, gyaw;
    __device__ StarChainPoses(const TreeDev& t, const int* path_, int D_, const int*, const int*,
                              const double* goal)
        : tr(t), path(path_), D(D_), gx(goal[0]), gy(goal[1]), gyaw(goal[2]) {}
    __device__ int edges() const { return D; }  // the goal edge, then node -> parent down to the root
    __device__ CfPose pose(int j) const {
        if (j == 0) return CfPose{gx, gy, gyaw};
        const int node = path[D - j];
        return CfPose{tr.x[node], tr.y[node], tr.yaw[node]};
    }
};

// pp_star_chain_segments' chain: the goal with its own yaw, then the stored poses of the caller's
// nodes in the caller's order (path[0] the node after the goal, path[D - 1] the root) — a
// shortened path's edges skip tree nodes, so the chain is given, not walked
struct CsrChainPoses {
    static constexpr bool kRootPoint = true;
    static constexpr bool kGoalNoneOk = true;
    TreeDev tr;
    const int* path;
    int D;
    double gx, gy, gyaw;
    __device__ CsrChainPoses(const TreeDev& t, const int* path_, int D_, const int*, const int*,
                             const double* goal)
        : tr(t), path(path_), D(D_), gx(goal[0]), gy(goal[1]), gyaw(goal[2]) {}
    __device__ int edges() const { return D; }
    __device__ CfPose pose(int j) const {
        if (j == 0) return CfPose{gx, gy, gyaw};
        const int node = path[j - 1];
        return CfPose{tr.x[node], tr.y[node], tr.yaw[node]};
    }
};

}  // namespace ppamd

// Row field of a goal pose (include/dgdm_hip.h, dgdm_guidance_goal_field): for every row of the cond_fn grid the signed, windowed
// direction from the row's pose to the goal of its (chain, finger), times the chain's weights - the per-row seed of the trunk's backward
// pass for chains with use_rowcoef == DGDM_OBJ_ROWFIELD.  A positive entry rewards motion toward the goal (the roll-out's convention:
// state += logits * scale).
// One thread per row; every entry is evaluated in float64 from float32 inputs (the handle's own grids, the caller's goals) and rounded
// once, in operations no compiler may fuse (a difference, a quotient, a clamp, one product), so a float64 restatement reproduces the bits.
#include "common.h"
#include "trunk.h"

namespace dgdm {

__global__ __launch_bounds__(256) void goal_field_kernel(const float *__restrict__ ori_grid, const float *__restrict__ pos_grid,
                                                          const float *__restrict__ goals, const DgdmGoalSpec *__restrict__ specs, int B, int G,
                                                          int P, int64_t R, int64_t total, float *__restrict__ field) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int chain = (int)(i / R);
    const int64_t r = i - (int64_t)chain * R;                 // r = cell * B + b, cell = (g * P + px) * P + py
    const int b = (int)(r % B);
    const int cell = (int)(r / B);
    const int py = cell % P, px = (cell / P) % P, g = cell / (P * P);
    const DgdmGoalSpec sp = specs[chain];
    const float *goal = goals + ((size_t)chain * B + b) * 3;
    double u[3];
    u[0] = (double)goal[0] - (double)ori_grid[g];
    if (u[0] > 1.0) u[0] -= 2.0;                              // the shorter way round: ori is theta / pi - 1, period 2
    if (u[0] < -1.0) u[0] += 2.0;
    u[1] = (double)goal[1] - (double)pos_grid[px];
    u[2] = (double)goal[2] - (double)pos_grid[py];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const double h = (double)(j == 0 ? sp.ori_window : sp.pos_window);
        double s;
        if (sp.profile == 0) {
            const double a = fabs(u[j]);
            s = (a > 0.0 && a <= h) ? (u[j] > 0.0 ? 1.0 : -1.0) : 0.0;
        } else {
            s = fmin(fmax(u[j] / h, -1.0), 1.0);
        }
        field[i * 3 + j] = (float)((double)sp.weight[j] * s);
    }
}

int goal_field_build(const float *ori_grid, const float *pos_grid, const float *goals, const DgdmGoalSpec *specs, int n_chains, int B, int G, int P,
                     float *field, hipStream_t s) {
    if (!ori_grid || !pos_grid || !goals || !specs || !field || n_chains <= 0 || B <= 0 || G <= 0 || P <= 0) return DGDM_EINVAL;
    const int64_t R = (int64_t)B * G * P * P, total = R * n_chains;
    hipLaunchKernelGGL(goal_field_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, ori_grid, pos_grid, goals, specs, B, G, P, R, total,
                       field);
    DGDM_HIP_CHECK(hipGetLastError());
    return DGDM_OK;
}

}  // namespace dgdm

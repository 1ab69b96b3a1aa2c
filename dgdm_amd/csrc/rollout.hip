// Predicted roll-outs (dgdm_guidance_rollout): the dynamics model's output fed back into its pose input, K interactions per start
// orientation - what the reference's simulator does by closing the gripper 40 times (dynamics/sim_test_mj.py:161-185,
// sim_test_mj_3d.py:154-176), with the model in MuJoCo's place.  After the first interaction every (chain, finger, orientation) row
// has a pose of its own, so layer 1's pose term can no longer be one table row per cell: rollout_pose_table_kernel makes it per row,
// once per interaction, straight in the operand layout of the forward-only f16x3 trunk (trunk_f16l.hip, ROWPOSE), and
// rollout_update_kernel applies the logits to the state.  The state is float64; the model sees it rounded once to float32, as the
// reference model's float32 inputs are.  Nothing here returns to the host: a roll-out is K x (pose table, trunk, update) on one stream.
#include "common.h"
#include "trunk.h"

// The update's products and sums are rounded one by one (the contract states them that way); explicit fma() calls are unaffected.
#pragma clang fp contract(off)

namespace dgdm {

namespace {
struct Scale3 { double v[3]; };
constexpr int RO_LD = 260;        // row stride of the staged 32 x 256 block: float4-aligned, rows spread over the LDS banks
}  // namespace

__global__ void rollout_start_kernel(const float *__restrict__ ori_grid, int B, int G, int64_t total, double *__restrict__ state,
                                     int32_t *__restrict__ left, double *__restrict__ traj0) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;      // row of [n_chains][G][B]
    if (i >= total) return;
    const int g = (int)((i / B) % G);
    const double o = (double)ori_grid[g];
    state[3 * i] = o; state[3 * i + 1] = 0.0; state[3 * i + 2] = 0.0;
    left[i] = -1;
    if (traj0) { traj0[3 * i] = o; traj0[3 * i + 1] = 0.0; traj0[3 * i + 2] = 0.0; }
}

int rollout_start(const float *ori_grid, int n_chains, int B, int G, double *state, int32_t *left, double *traj0, hipStream_t s) {
    const int64_t total = (int64_t)n_chains * B * G;
    if (total <= 0) return DGDM_OK;
    hipLaunchKernelGGL(rollout_start_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, ori_grid, B, G, total, state, left, traj0);
    DGDM_HIP_CHECK(hipGetLastError());
    return DGDM_OK;
}

// One workgroup per trunk tile = 32 orientations of one finger of one chain.  Per row: the 27-wide embedding as pose_embed_kernel
// computes it (smallnet.hip), contracted with w1p_wt [27][W1] as linear64_kernel does for the sweep's pose table (an ascending-k fma
// chain in float64 from zero, one rounding to float32): for a row that holds a sweep pose the same bits as ptab_sweep.  A thread owns
// one output column of a 256-column pass for all 32 rows; the block is staged in LDS and leaves as the float4s of tile_table's layout.
template <int W1>
__global__ __launch_bounds__(256) void rollout_pose_table_kernel(const double *__restrict__ state, const double *__restrict__ w1p_wt, int B, int G,
                                                                 int tiles_per_b, float4 *__restrict__ tiles, float *__restrict__ pmax) {
    constexpr int WB = W1 / 32, NPASS = W1 / 256;
    __shared__ double emb[32][27];
    __shared__ __attribute__((aligned(16))) float sm[32 * RO_LD];
    const int t = threadIdx.x;
    const int tile = blockIdx.x;
    const int per_chain = B * tiles_per_b;
    const int chain = tile / per_chain;
    const int rem = tile - chain * per_chain;
    const int b = rem / tiles_per_b;
    const int gt = rem - b * tiles_per_b;
    if (t < 32) {
        const int g = min(gt * 32 + t, G - 1);                // a finger's padding rows repeat its last valid row
        const double *st = state + ((size_t)chain * B * G + (size_t)g * B + b) * 3;
        const float o = (float)st[0], px = (float)st[1], py = (float)st[2];
        float e[27];
        e[0] = o;
        e[9] = px; e[10] = py;
        float f = 1.f;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            e[1 + 2 * k] = sinf(o * f);
            e[2 + 2 * k] = cosf(o * f);
            e[11 + 4 * k] = sinf(px * f); e[12 + 4 * k] = sinf(py * f);
            e[13 + 4 * k] = cosf(px * f); e[14 + 4 * k] = cosf(py * f);
            f *= 2.f;
        }
#pragma unroll
        for (int k = 0; k < 27; ++k) emb[t][k] = (double)e[k];
    }
    __syncthreads();
    float rowmax = 0.f;                                       // of row t >> 3, kept by the thread with (t & 7) == 0
#pragma unroll 1
    for (int pass = 0; pass < NPASS; ++pass) {
        const int n = pass * 256 + t;
        double w[27];
#pragma unroll
        for (int k = 0; k < 27; ++k) w[k] = w1p_wt[(size_t)k * W1 + n];
#pragma unroll 4
        for (int r = 0; r < 32; ++r) {
            double acc = 0.0;
#pragma unroll
            for (int k = 0; k < 27; ++k) acc = fma(emb[r][k], w[k], acc);
            sm[r * RO_LD + t] = (float)acc;
        }
        __syncthreads();
        for (int i = t; i < 8 * 4 * 64; i += 256) {
            const int lane = i & 63, q = (i >> 6) & 3, ol = i >> 8;
            const int nr = lane & 31, h = lane >> 5;
            tiles[(((size_t)tile * WB + pass * 8 + ol) * 4 + q) * 64 + lane] = *reinterpret_cast<const float4 *>(&sm[nr * RO_LD + 32 * ol + 8 * q + 4 * h]);
        }
        if (pmax) {
            const int row = t >> 3, seg = t & 7;
            float m = 0.f;
            for (int i = 0; i < 32; ++i) m = fmaxf(m, fabsf(sm[row * RO_LD + seg * 32 + ((i + t) & 31)]));
            m = fmaxf(m, __shfl_xor(m, 1)); m = fmaxf(m, __shfl_xor(m, 2)); m = fmaxf(m, __shfl_xor(m, 4));
            rowmax = fmaxf(rowmax, m);
        }
        __syncthreads();
    }
    if (pmax && (t & 7) == 0) pmax[(size_t)tile * 32 + (t >> 3)] = rowmax;
}

int rollout_pose_table(const double *state, const double *w1p_wt, int W1, int n_chains, int B, int G, float *tiles, float *pmax, hipStream_t s) {
    if (!state || !w1p_wt || !tiles || (W1 != 256 && W1 != 512) || B <= 0 || G <= 0) return DGDM_EINVAL;
    const int tpb = (G + 31) / 32;
    const int ntiles = n_chains * B * tpb;
    if (ntiles <= 0) return DGDM_OK;
    if (W1 == 256)
        hipLaunchKernelGGL(rollout_pose_table_kernel<256>, dim3(ntiles), dim3(256), 0, s, state, w1p_wt, B, G, tpb, reinterpret_cast<float4 *>(tiles), pmax);
    else
        hipLaunchKernelGGL(rollout_pose_table_kernel<512>, dim3(ntiles), dim3(256), 0, s, state, w1p_wt, B, G, tpb, reinterpret_cast<float4 *>(tiles), pmax);
    DGDM_HIP_CHECK(hipGetLastError());
    return DGDM_OK;
}

// ori <- ori + l0 scale0, brought back into [-1, 1] (what subtracting / adding 2 while outside gives: the multiple of 2 is taken in
// one step, exact for every |ori| < 2^53, so that no value - infinite or huge - can keep a loop running; values inside, +-1 included,
// are left alone); pos <- pos + l scale, not clamped.  NaN fails every comparison and stays; inf - inf makes an infinite ori NaN.
__global__ void rollout_update_kernel(const float *__restrict__ logits, Scale3 sc, int k, int64_t rows, double *__restrict__ state,
                                      int32_t *__restrict__ left, double *__restrict__ traj_next, double *__restrict__ final_state,
                                      float *__restrict__ first_logits) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows) return;
    const float l0 = logits[3 * i], l1 = logits[3 * i + 1], l2 = logits[3 * i + 2];
    double o = state[3 * i], x = state[3 * i + 1], y = state[3 * i + 2];
    const double d0 = (double)l0 * sc.v[0], d1 = (double)l1 * sc.v[1], d2 = (double)l2 * sc.v[2];
    o = o + d0;
    if (o > 1.0) o = o - 2.0 * ceil((o - 1.0) * 0.5);
    else if (o < -1.0) o = o + 2.0 * ceil((-o - 1.0) * 0.5);
    x = x + d1;
    y = y + d2;
    state[3 * i] = o; state[3 * i + 1] = x; state[3 * i + 2] = y;
    if (left[i] < 0 && (fabs(x) > 1.0 || fabs(y) > 1.0)) left[i] = k;
    if (traj_next) { traj_next[3 * i] = o; traj_next[3 * i + 1] = x; traj_next[3 * i + 2] = y; }
    if (final_state) { final_state[3 * i] = o; final_state[3 * i + 1] = x; final_state[3 * i + 2] = y; }
    if (first_logits) { first_logits[3 * i] = l0; first_logits[3 * i + 1] = l1; first_logits[3 * i + 2] = l2; }
}

int rollout_update(const float *logits, const double scale[3], int k, int64_t rows, double *state, int32_t *left, double *traj_next,
                   double *final_state, float *first_logits, hipStream_t s) {
    if (!logits || !scale || !state || !left) return DGDM_EINVAL;
    if (rows <= 0) return DGDM_OK;
    Scale3 sc;
    for (int j = 0; j < 3; ++j) sc.v[j] = scale[j];
    hipLaunchKernelGGL(rollout_update_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, s, logits, sc, k, rows, state, left, traj_next,
                       final_state, first_logits);
    DGDM_HIP_CHECK(hipGetLastError());
    return DGDM_OK;
}

}  // namespace dgdm

// Tally of forward-only dynamics logits per (chain, finger): the joint class histogram and four sums that dgdm_guidance_score returns.
// Classes as generator/diffusion.py:532 and dynamics/sim_test_mj.py:198-200 assign them: 2 above the threshold, 0 below its negative,
// 1 between.  The job is small (a finger has G P^2 cells, 9000 at the largest grid in use): one workgroup per (chain, finger), the
// histogram in LDS on integer atomics (integer addition is exact in any order), the sums in double precision in a FIXED order - every
// thread its own cells in ascending order, an xor butterfly across the wave, the four wave totals added by thread 0 - so the results are
// the same bits run to run.  No float atomics anywhere.
#include "common.h"
#include "trunk.h"

namespace dgdm {

namespace {
struct Thr3 { float v[3]; };

__device__ __forceinline__ int class_of(float l, float thr) { return l > thr ? 2 : (l < -thr ? 0 : 1); }
}  // namespace

__global__ __launch_bounds__(256) void score_tally_kernel(const float *__restrict__ logits, int B, int C, Thr3 thr, int32_t *__restrict__ counts,
                                                           float *__restrict__ sums) {
    __shared__ int hist[27];
    __shared__ double part[4][4];                             // [wave][sum]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int chain = blockIdx.x / B, b = blockIdx.x - chain * B;
    if (tid < 27) hist[tid] = 0;
    __syncthreads();
    const float *rows = logits + ((size_t)chain * B * C + b) * 3;          // the finger's cell c: row c * B + b of its chain
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (int c = tid; c < C; c += 256) {
        const float *l = rows + (size_t)c * B * 3;
        const float d0 = l[0], d1 = l[1], d2 = l[2];
        atomicAdd(&hist[(class_of(d0, thr.v[0]) * 3 + class_of(d1, thr.v[1])) * 3 + class_of(d2, thr.v[2])], 1);
        s[0] += d0; s[1] += fabsf(d0); s[2] += d1; s[3] += d2;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s[k] += __shfl_xor(s[k], o);
        if (lane == 0) part[wave][k] = s[k];
    }
    __syncthreads();
    if (tid < 27) counts[(size_t)blockIdx.x * 27 + tid] = hist[tid];
    if (tid < 4) sums[(size_t)blockIdx.x * 4 + tid] = (float)(((part[0][tid] + part[1][tid]) + part[2][tid]) + part[3][tid]);
}

int score_tally(const float *logits, int n_chains, int B, int C, const float thr[3], int32_t *counts, float *sums, hipStream_t s) {
    if (!logits || !counts || !sums || n_chains <= 0 || B <= 0 || C <= 0) return DGDM_EINVAL;
    Thr3 t;
    for (int k = 0; k < 3; ++k) t.v[k] = thr[k];
    hipLaunchKernelGGL(score_tally_kernel, dim3((unsigned)(n_chains * B)), dim3(256), 0, s, logits, B, C, t, counts, sums);
    DGDM_HIP_CHECK(hipGetLastError());
    return DGDM_OK;
}

}  // namespace dgdm

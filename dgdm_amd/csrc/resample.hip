// Resampling the fingers of a chain by predicted objective (include/dgdm_hip.h: dgdm_guidance_objective_values, dgdm_chain_resample,
// dgdm_resample_uniform).  Three small kernels, everything that decides anything in float64 and in a FIXED order:
//   objective_values_kernel  one wave per (chain, finger): every lane its own cells in ascending order, an xor butterfly across the wave
//                            (the fixed shape of score.hip's sums), lane 0 stores - the same bits run to run, no atomics;
//   resample_kernel          one lane per chain walks its B fingers in ascending order, which makes the recipe's order literal
//                            (B <= 64 in every shipped configuration; a chain's whole job is a few hundred float64 operations);
//   gather_kernel            x_out[k][j] = x[k][a_j] as bit copies, one thread per entry, coalesced on both sides.
// The input of the first is 12 B per row and is read once; none of the three is worth more machinery than that.
#include "common.h"
#include "philox.h"
#include "trunk.h"
#include <cmath>

namespace dgdm {

namespace {

// numpy.random.Philox(key=[seed, key], counter=[0, step_index, 1, 0]).random_raw()'s output 0 (numpy counts up before a block), top 53 bits
__device__ __forceinline__ double resample_uniform(uint64_t seed, uint64_t key, uint64_t step_index) {
    const U64x4 r = philox4x64_10(U64x4{{1, step_index, 1, 0}}, seed, key);
    return (double)(r.v[0] >> 11) * 0x1.0p-53;
}

__global__ __launch_bounds__(64) void objective_values_kernel(const float *__restrict__ logits, const TrunkObjective *__restrict__ obj,
                                                              const float *__restrict__ rowcoef, const float *__restrict__ rowfield, int B, int C,
                                                              double *__restrict__ values) {
    const int lane = threadIdx.x;
    const int chain = blockIdx.x / B, b = blockIdx.x - chain * B;
    const TrunkObjective o = obj[chain];
    const size_t R = (size_t)B * C;
    double lin[3], quad[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) { lin[j] = (double)o.lin[j]; quad[j] = (double)o.quad[j]; }
    double v = 0.0;
    for (int c = lane; c < C; c += 64) {
        const size_t r = (size_t)chain * R + (size_t)c * B + b;          // the finger's cell c: row c * B + b of its chain
        const float *l = logits + r * 3;
        const double d[3] = {(double)l[0], (double)l[1], (double)l[2]};
        double t = 0.0;
#pragma unroll
        for (int j = 0; j < 3; ++j) t += lin[j] * d[j] + quad[j] * d[j] * d[j];
        if (o.use_rowcoef == 1) t += (double)rowcoef[r] * d[0];
        if (o.use_rowcoef == DGDM_OBJ_ROWFIELD) {
            const float *f = rowfield + r * 3;
#pragma unroll
            for (int j = 0; j < 3; ++j) t += (double)f[j] * d[j];
        }
        v += t;
    }
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) v += __shfl_xor(v, s);
    if (lane == 0) values[blockIdx.x] = v;
}

struct ResampleArgs {
    const double *values;      // [n_grad * nc][B]
    int n_grad, nc, B;
    double beta, ess_frac;
    uint64_t seed, step_index;
    const uint64_t *keys;      // [nc]
    double *logw, *vprev;      // [nc][B] in / out
    int32_t *anc;              // [nc][B]
    double *ess;               // [nc]
    int32_t *did;              // [nc]
};

__global__ __launch_bounds__(64) void resample_kernel(ResampleArgs a) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= a.nc) return;
    const int B = a.B;
    double *logw = a.logw + (size_t)k * B, *vprev = a.vprev + (size_t)k * B;
    int32_t *anc = a.anc + (size_t)k * B;
    const double ninf = -HUGE_VAL;
    // 1, 2: the potential of every finger and its incremental weight; 3: the largest log weight
    double m = ninf;
    for (int b = 0; b < B; ++b) {
        double sum = 0.0;
        for (int j = 0; j < a.n_grad; ++j) sum += a.values[((size_t)j * a.nc + k) * B + b];
        const double v = a.beta * (sum / (double)a.n_grad);
        double lw;
        if (isfinite(v)) {
            lw = logw[b] + (v - vprev[b]);
            vprev[b] = v;
        } else {
            lw = ninf;
        }
        logw[b] = lw;
        if (lw > m) m = lw;
        anc[b] = b;
    }
    if (!(m > ninf)) {                                             // nothing to weigh: every value of this step was non-finite
        for (int b = 0; b < B; ++b) logw[b] = 0.0;
        a.ess[k] = 0.0;
        a.did[k] = 0;
        return;
    }
    // 4: normalised weights (recomputed where needed: exp of the same argument is the same value) and the effective sample size
    double s = 0.0;
    for (int b = 0; b < B; ++b) s += exp(logw[b] - m);
    double s2 = 0.0;
    for (int b = 0; b < B; ++b) { const double w = exp(logw[b] - m) / s; s2 += w * w; }
    const double ess = 1.0 / s2;
    a.ess[k] = ess;
    if (!(ess < a.ess_frac * (double)B)) { a.did[k] = 0; return; }            // 6: ancestors stay the identity, logw is kept
    // 5: systematic resampling.  p_j ascends with j and cum_b with b, so one pointer walks the fingers: a_j = #{b : cum_b <= p_j}
    const double u = resample_uniform(a.seed, a.keys[k], a.step_index);
    int b = 0;
    double cum = exp(logw[0] - m) / s;                            // cum_b of the finger the pointer stands on
    for (int j = 0; j < B; ++j) {
        const double p = (u + (double)j) / (double)B;
        while (b < B && cum <= p) {
            ++b;
            if (b < B) cum += exp(logw[b] - m) / s;
        }
        anc[j] = b < B - 1 ? b : B - 1;
    }
    // vprev[j] = vprev_old[a_j] in place: a_j never descends, so the slots with a_j >= j can be filled in ascending order (what they read
    // lies at or behind them, untouched) and then the slots with a_j < j in descending order (a slot they read was either not written
    // or written with a_j' == j', i.e. unchanged)
    for (int j = 0; j < B; ++j) if (anc[j] >= j) vprev[j] = vprev[anc[j]];
    for (int j = B - 1; j >= 0; --j) if (anc[j] < j) vprev[j] = vprev[anc[j]];
    for (int j = 0; j < B; ++j) logw[j] = 0.0;
    a.did[k] = 1;
}

__global__ void gather_kernel(const uint32_t *__restrict__ x, const int32_t *__restrict__ anc, int B, int L, int64_t n, uint32_t *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t row = i / L;                                    // k * B + j
    const int l = (int)(i - row * L);
    const int64_t k = row / B;
    int a = anc[row];
    a = a < 0 ? 0 : (a >= B ? B - 1 : a);                         // the ancestors are this call's own; the clamp costs nothing
    out[i] = x[(k * B + a) * L + l];
}

__global__ void resample_uniform_kernel(uint64_t seed, const uint64_t *__restrict__ keys, uint64_t step_index, int n, double *__restrict__ u) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) u[i] = resample_uniform(seed, keys[i], step_index);
}

}  // namespace

int objective_values_launch(const float *logits, const TrunkObjective *obj, const float *rowcoef, const float *rowfield, int n_chains, int B, int C,
                            double *values, hipStream_t s) {
    if (!logits || !obj || !values || n_chains <= 0 || B <= 0 || C <= 0) return DGDM_EINVAL;
    hipLaunchKernelGGL(objective_values_kernel, dim3((unsigned)(n_chains * B)), dim3(64), 0, s, logits, obj, rowcoef, rowfield, B, C, values);
    DGDM_HIP_CHECK(hipGetLastError());
    return DGDM_OK;
}

}  // namespace dgdm

extern "C" int dgdm_chain_resample(const float *x_dev, const double *values_dev, int n_chains, int B, int L, int n_grad, double beta_per_cell,
                                   double ess_frac, uint64_t seed, const uint64_t *chain_keys_dev, int64_t step_index, double *logw_dev,
                                   double *vprev_dev, float *x_out_dev, int32_t *ancestors_dev, double *ess_dev, int32_t *did_dev, void *stream) {
    DGDM_REQUIRE(x_dev && values_dev && chain_keys_dev && logw_dev && vprev_dev && x_out_dev && ancestors_dev && ess_dev && did_dev, DGDM_EINVAL,
                 "dgdm_chain_resample: null argument");
    DGDM_REQUIRE(n_chains >= 1 && B >= 1 && L >= 1 && n_grad >= 1 && step_index >= 0, DGDM_EINVAL,
                 "dgdm_chain_resample: n_chains %d, B %d, L %d, n_grad %d, step_index %lld (each at least 1, the step index at least 0)", n_chains, B, L,
                 n_grad, (long long)step_index);
    const int64_t n = (int64_t)n_chains * B * L;
    DGDM_REQUIRE((int64_t)n_chains * B <= INT32_MAX && (int64_t)n_chains * B * n_grad <= INT32_MAX && (n + 255) / 256 <= INT32_MAX, DGDM_EINVAL,
                 "dgdm_chain_resample: %d chains of %d x %d entries are more than one launch covers", n_chains, B, L);
    DGDM_REQUIRE(x_out_dev + n <= x_dev || x_dev + n <= x_out_dev, DGDM_EINVAL, "dgdm_chain_resample: x_out_dev overlaps x_dev");
    DGDM_REQUIRE(logw_dev != vprev_dev, DGDM_EINVAL, "dgdm_chain_resample: logw_dev and vprev_dev are one buffer");
    hipStream_t s = (hipStream_t)stream;
    dgdm::ResampleArgs a{values_dev, n_grad, n_chains, B, beta_per_cell, ess_frac, seed, (uint64_t)step_index, chain_keys_dev, logw_dev, vprev_dev,
                         ancestors_dev, ess_dev, did_dev};
    hipLaunchKernelGGL(dgdm::resample_kernel, dim3((unsigned)((n_chains + 63) / 64)), dim3(64), 0, s, a);
    DGDM_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(dgdm::gather_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, reinterpret_cast<const uint32_t *>(x_dev), ancestors_dev, B,
                       L, n, reinterpret_cast<uint32_t *>(x_out_dev));
    DGDM_HIP_CHECK(hipGetLastError());
    return DGDM_OK;
}

extern "C" int dgdm_resample_uniform(uint64_t seed, const uint64_t *chain_keys_dev, int n_chains, int64_t step_index, double *u_dev, void *stream) {
    DGDM_REQUIRE(chain_keys_dev && u_dev, DGDM_EINVAL, "dgdm_resample_uniform: null argument");
    DGDM_REQUIRE(n_chains >= 0 && step_index >= 0, DGDM_EINVAL, "dgdm_resample_uniform: negative argument");
    if (n_chains == 0) return DGDM_OK;
    hipLaunchKernelGGL(dgdm::resample_uniform_kernel, dim3((unsigned)((n_chains + 63) / 64)), dim3(64), 0, (hipStream_t)stream, seed, chain_keys_dev,
                       (uint64_t)step_index, n_chains, u_dev);
    DGDM_HIP_CHECK(hipGetLastError());
    return DGDM_OK;
}

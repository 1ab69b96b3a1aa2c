// Condition rows of the eps-net from the dynamics model's opinion of a finger (dgdm_guidance_label / dgdm_guidance_label_settled, the
// runners in guidance_api.hip): the replication of one batch of fingers over the objects' chains, and the two reductions that turn what
// dgdm_guidance_score / dgdm_guidance_rollout leave per (chain, finger) into the row's columns (include/dgdm_hip.h states them).  As in
// score.hip: integer sums exact, everything else in float64 in a FIXED order - one thread owns one (finger, object) or one (finger,
// block of the row) and walks its terms in ascending order, so the bits do not depend on the launch geometry - one division and one
// rounding to float32 per value, no float atomics.  The work is tiny beside the trunk (a finger has G orientations and n_objects <= 256).
#include "common.h"
#include "trunk.h"

// c*c + s*s and px*px + py*py are two products and a sum, each rounded on its own (numpy's arithmetic)
#pragma clang fp contract(off)

namespace dgdm {

// dst [n_chains][B][L]: every chain the block of fingers first .. first + B - 1, the rows past the last finger copies of finger N - 1
__global__ void label_replicate_kernel(const float *__restrict__ fingers, int64_t N, int64_t first, int B, int L, int64_t total, float *__restrict__ dst) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int l = (int)(i % L);
    const int b = (int)((i / L) % B);
    const int64_t f = first + b < N ? first + b : N - 1;
    dst[i] = fingers[f * L + l];
}

int label_replicate(const float *fingers, int64_t N, int64_t first, int n_chains, int B, int L, float *dst, hipStream_t s) {
    if (!fingers || !dst || N < 1 || first < 0 || first >= N || n_chains <= 0 || B <= 0 || L <= 0) return DGDM_EINVAL;
    const int64_t total = (int64_t)n_chains * B * L;
    hipLaunchKernelGGL(label_replicate_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, fingers, N, first, B, L, total, dst);
    DGDM_HIP_CHECK(hipGetLastError());
    return DGDM_OK;
}

// One thread per (finger of the batch, block of the row): MEAN has one block over all M objects, PER_OBJECT M blocks of one object.
__global__ void label_tally_kernel(const int32_t *__restrict__ counts, const float *__restrict__ sums, int M, int B, int nvalid, int64_t cells,
                                   int per_object, float *__restrict__ rows, int64_t row_stride, int64_t object_stride) {
    const int nblk = per_object ? M : 1;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nvalid * nblk) return;
    const int b = i / nblk, blk = i - b * nblk;
    const int m0 = per_object ? blk : 0, m1 = per_object ? blk + 1 : M;
    int64_t k[6] = {0, 0, 0, 0, 0, 0};
    double sm[4] = {0.0, 0.0, 0.0, 0.0};
    for (int m = m0; m < m1; ++m) {
        const int32_t *c = counts + ((size_t)m * B + b) * 27;
        for (int bin = 0; bin < 27; ++bin) {
            const int64_t v = c[bin];
            const int c0 = bin / 9, c1 = (bin / 3) % 3, c2 = bin % 3;
            if (c0 == 0) k[0] += v;
            if (c0 == 2) k[1] += v;
            if (c1 == 0) k[2] += v;
            if (c1 == 2) k[3] += v;
            if (c2 == 0) k[4] += v;
            if (c2 == 2) k[5] += v;
        }
        const float *sp = sums + ((size_t)m * B + b) * 4;
        for (int j = 0; j < 4; ++j) sm[j] += (double)sp[j];
    }
    const double den = (double)((int64_t)(m1 - m0) * cells);
    float *out = rows + (size_t)b * row_stride + (per_object ? (size_t)blk * object_stride : 0);
    for (int j = 0; j < 6; ++j) out[j] = (float)((double)k[j] / den);
    for (int j = 0; j < 4; ++j) out[6 + j] = (float)(sm[j] / den);
}

int label_tally(const int32_t *counts, const float *sums, int M, int B, int nvalid, int64_t cells, int per_object, float *rows, int64_t row_stride,
                int64_t object_stride, hipStream_t s) {
    if (!counts || !sums || !rows || M <= 0 || B <= 0 || nvalid <= 0 || nvalid > B || cells <= 0) return DGDM_EINVAL;
    const int n = nvalid * (per_object ? M : 1);
    hipLaunchKernelGGL(label_tally_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, s, counts, sums, M, B, nvalid, cells, per_object, rows, row_stride,
                       object_stride);
    DGDM_HIP_CHECK(hipGetLastError());
    return DGDM_OK;
}

// Per (finger, object): c, s, rho, p, fl and whether a state was not finite -> per_obj [B][M][6] doubles, g ascending
__global__ void label_settled_object_kernel(const double *__restrict__ final_state, const int32_t *__restrict__ left, int M, int B, int G, int nvalid,
                                            double *__restrict__ per_obj) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nvalid * M) return;
    const int b = i / M, m = i - b * M;
    double c = 0.0, s = 0.0, p = 0.0;
    int inside = 0;
    bool bad = false;
    for (int g = 0; g < G; ++g) {
        const size_t r = (size_t)m * B * G + (size_t)g * B + b;
        const double o = final_state[3 * r], px = final_state[3 * r + 1], py = final_state[3 * r + 2];
        bad = bad || !(isfinite(o) && isfinite(px) && isfinite(py));
        const double theta = M_PI * (o + 1.0);
        c += cos(theta);
        s += sin(theta);
        p += sqrt(px * px + py * py);
        inside += left[r] >= 0 ? 1 : 0;
    }
    const double dg = (double)G;
    c = c / dg; s = s / dg; p = p / dg;
    double *o = per_obj + ((size_t)b * M + m) * 6;
    o[0] = sqrt(c * c + s * s); o[1] = c; o[2] = s; o[3] = p; o[4] = (double)inside / dg; o[5] = bad ? 1.0 : 0.0;
}

// Per (finger, block): MEAN the average over m ascending, PER_OBJECT the object's own values; one rounding to float32
__global__ void label_settled_rows_kernel(const double *__restrict__ per_obj, int M, int nvalid, int per_object, float *__restrict__ rows,
                                          int64_t row_stride, int64_t object_stride) {
    const int nblk = per_object ? M : 1;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nvalid * nblk) return;
    const int b = i / nblk, blk = i - b * nblk;
    const int m0 = per_object ? blk : 0, m1 = per_object ? blk + 1 : M;
    double v[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    bool bad = false;
    for (int m = m0; m < m1; ++m) {
        const double *o = per_obj + ((size_t)b * M + m) * 6;
        for (int j = 0; j < 5; ++j) v[j] += o[j];
        bad = bad || o[5] != 0.0;
    }
    const double den = (double)(m1 - m0);
    float *out = rows + (size_t)b * row_stride + (per_object ? (size_t)blk * object_stride : 0);
    for (int j = 0; j < 5; ++j) out[j] = (j < 4 && bad) ? __builtin_nanf("") : (float)(v[j] / den);
}

int label_settled(const double *final_state, const int32_t *left, int M, int B, int G, int nvalid, int per_object, double *per_obj, float *rows,
                  int64_t row_stride, int64_t object_stride, hipStream_t s) {
    if (!final_state || !left || !per_obj || !rows || M <= 0 || B <= 0 || G <= 0 || nvalid <= 0 || nvalid > B) return DGDM_EINVAL;
    const int n1 = nvalid * M, n2 = nvalid * (per_object ? M : 1);
    hipLaunchKernelGGL(label_settled_object_kernel, dim3((unsigned)((n1 + 63) / 64)), dim3(64), 0, s, final_state, left, M, B, G, nvalid, per_obj);
    hipLaunchKernelGGL(label_settled_rows_kernel, dim3((unsigned)((n2 + 63) / 64)), dim3(64), 0, s, per_obj, M, nvalid, per_object, rows, row_stride,
                       object_stride);
    DGDM_HIP_CHECK(hipGetLastError());
    return DGDM_OK;
}

}  // namespace dgdm

// Device-resident dynamics-training data (dgdm_dynamics_batch_rows, dgdm_class_agreement): the row tensors that
// dynamics/main.py:21-35 builds on the host for every batch - each sample's control ordinates and object replicated over its pose
// cells, its pose grid and scores copied - written by ONE launch from the store's device arrays and a list of sample indices, and the
// three-class agreement counts of main.py:37-39 as integers.  Pure copies and integer counts: every result is exact and independent of
// the launch geometry.
#include "common.h"

#include <algorithm>

namespace dgdm {
namespace {

// One output tensor as `n_outer` runs; run o = the rows of the batch slots o * n_inner .. + n_inner - 1, one after the other (W floats
// each), that sequence repeated `reps` times.  A row is read from its store item [K][D] transposed: element kk = item[kk % K][d0 + kk / K].
//   2-D ctrl (rows, L):    n_outer = nb, n_inner = 1, reps = cells, item [L][2], d0 = 1 (the y ordinate), W = L
//   2-D obj  (rows, 2 V):  the same with item [2 V][1], W = 2 V
//   3-D ctrl (rows, 3, L): n_outer = 1, n_inner = nb, reps = cells (row = cell * nb + slot, main.py:29-31), item [L][3], W = 3 L; obj alike
//   score / ori / pos:     n_outer = nb, n_inner = 1, reps = 1, item [cells * width][1]: a sample's whole grid is one "row"
struct RowTask {
    const float   *src;
    float         *out;
    const int64_t *items;          // device [nb]: the store item each batch slot reads
    unsigned n_outer, n_inner, reps, W, K, D, d0;
    unsigned len;                  // n_inner * W * reps: floats per run
    unsigned blocks_per_run, first_block;
};
constexpr int N_TASKS = 5;
struct RowTasks { RowTask t[N_TASKS]; };

// A thread owns one 16-byte-aligned group of four output floats and stores it whole; a group that straddles the start or the end of a
// run (row widths that are no multiple of four, outputs that do not start on a 16-byte boundary) is stored float by float, each run
// writing its own floats only.
__global__ __launch_bounds__(256) void batch_rows_kernel(RowTasks a) {
    unsigned b = blockIdx.x;
    RowTask t = a.t[0];
#pragma unroll
    for (int q = 1; q < N_TASKS; ++q)
        if (b >= a.t[q].first_block) t = a.t[q];
    b -= t.first_block;
    const unsigned outer = b / t.blocks_per_run, bl = b % t.blocks_per_run;
    if (outer >= t.n_outer) return;
    const size_t base = (size_t)outer * t.len;
    const unsigned mis = (unsigned)(((reinterpret_cast<uintptr_t>(t.out) >> 2) + base) & 3);      // floats past a 16-byte boundary
    const long long j0 = 4ll * ((long long)bl * 256 + threadIdx.x) - mis;                         // this thread's floats of the run: j0 .. j0 + 3
    const long long lo = j0 < 0 ? 0 : j0, hi = j0 + 4 < (long long)t.len ? j0 + 4 : (long long)t.len;
    if (lo >= hi) return;
    const unsigned P = t.n_inner * t.W;
    const unsigned p = (unsigned)lo % P;
    unsigned slot = p / t.W, kk = p % t.W, d = kk / t.K, k = kk % t.K;
    const int64_t *items = t.items + (size_t)outer * t.n_inner;
    const float *row = t.src + (size_t)items[slot] * t.K * t.D + t.d0;
    float v[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const long long e = j0 + q;
        v[q] = 0.f;
        if (e >= lo && e < hi) {
            v[q] = row[k * t.D + d];
            ++kk;
            if (++k == t.K) { k = 0; ++d; }
            if (kk == t.W) {
                kk = k = d = 0;
                if (++slot == t.n_inner) slot = 0;
                row = t.src + (size_t)items[slot] * t.K * t.D + t.d0;
            }
        }
    }
    float *o = t.out + base + j0;
    if (hi - lo == 4) {
        *reinterpret_cast<float4 *>(o) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (j0 + q >= lo && j0 + q < hi) o[q] = v[q];
    }
}

// Column j of agree: the rows whose class (v > t) - (v < -t) is the same for score and pred; a NaN is in the middle class on both
// sides, as in torch.  Integer sums: the order of the atomic additions does not matter.
__global__ __launch_bounds__(256) void class_agreement_kernel(const float *__restrict__ score, const float *__restrict__ pred, int64_t rows,
                                                              float t0, float t1, float t2, unsigned long long *agree) {
    __shared__ int part[4][3];
    const float thr[3] = {t0, t1, t2};
    int c[3] = {0, 0, 0};
    for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < rows; r += (int64_t)gridDim.x * 256) {
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const float s = score[3 * r + j], p = pred[3 * r + j];
            const int cs = (int)(s > thr[j]) - (int)(s < -thr[j]), cp = (int)(p > thr[j]) - (int)(p < -thr[j]);
            c[j] += cs == cp;
        }
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        for (int off = 32; off > 0; off >>= 1) c[j] += __shfl_down(c[j], off, 64);
        if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6][j] = c[j];
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        const int n = part[0][threadIdx.x] + part[1][threadIdx.x] + part[2][threadIdx.x] + part[3][threadIdx.x];
        if (n) atomicAdd(agree + threadIdx.x, (unsigned long long)n);
    }
}

}  // namespace
}  // namespace dgdm

using namespace dgdm;

extern "C" int dgdm_dynamics_batch_rows(const DgdmDynamicsStore *st, const int64_t *sample_ids_host, int nb, int64_t *ids_dev, float *ctrl_dev,
                                        float *obj_dev, float *score_dev, float *ori_dev, float *pos_dev, void *stream) {
    const char *fn = "dgdm_dynamics_batch_rows";
    DGDM_REQUIRE(st && sample_ids_host && ids_dev && ctrl_dev && obj_dev && score_dev && ori_dev && pos_dev, DGDM_EINVAL, "%s: null argument", fn);
    DGDM_REQUIRE(st->ctrl_dev && st->object_dev && st->scores_dev && st->ori_dev && st->pos_dev, DGDM_EINVAL, "%s: null store array", fn);
    DGDM_REQUIRE(st->n_samples >= 1 && st->n_objects >= 1 && st->cells >= 1 && st->n_ctrl >= 1 && st->n_object_points >= 1 && nb >= 1, DGDM_EINVAL,
                 "%s: samples %lld, objects %lld, cells %d, control points %d, object points %d, batch %d: all must be positive", fn,
                 (long long)st->n_samples, (long long)st->n_objects, st->cells, st->n_ctrl, st->n_object_points, nb);
    DGDM_REQUIRE(st->object_of_sample_host || st->n_objects == st->n_samples, DGDM_EINVAL, "%s: %lld objects for %lld samples and no object_of_sample_host", fn,
                 (long long)st->n_objects, (long long)st->n_samples);
    for (const void *p : {(const void *)ids_dev, (const void *)ctrl_dev, (const void *)obj_dev, (const void *)score_dev, (const void *)ori_dev, (const void *)pos_dev})
        DGDM_REQUIRE((reinterpret_cast<uintptr_t>(p) & 3) == 0, DGDM_EINVAL, "%s: an output is not 4-byte aligned", fn);
    // every index is checked here, before anything is enqueued: the kernel reads store rows by them
    std::vector<int64_t> ids(2 * (size_t)nb);
    for (int i = 0; i < nb; ++i) {
        const int64_t s = sample_ids_host[i];
        DGDM_REQUIRE(s >= 0 && s < st->n_samples, DGDM_EINVAL, "%s: sample index %lld (batch slot %d) outside the store's %lld samples", fn, (long long)s, i,
                     (long long)st->n_samples);
        const int64_t o = st->object_of_sample_host ? (int64_t)st->object_of_sample_host[s] : s;
        DGDM_REQUIRE(o >= 0 && o < st->n_objects, DGDM_EINVAL, "%s: sample %lld names object %lld of %lld", fn, (long long)s, (long long)o, (long long)st->n_objects);
        ids[i] = s;
        ids[nb + i] = o;
    }
    const bool d3 = st->fingers_3d != 0;
    const int64_t cells = st->cells, L = st->n_ctrl, V = st->n_object_points;
    struct Spec { const float *src; float *out; bool object; int64_t K, D, d0, W; bool replicated; };
    const Spec specs[N_TASKS] = {
        {st->ctrl_dev, ctrl_dev, false, L, d3 ? 3 : 2, d3 ? 0 : 1, d3 ? 3 * L : L, true},
        {st->object_dev, obj_dev, true, d3 ? V : 2 * V, d3 ? 3 : 1, 0, d3 ? 3 * V : 2 * V, true},
        {st->scores_dev, score_dev, false, cells * 3, 1, 0, cells * 3, false},
        {st->ori_dev, ori_dev, false, cells, 1, 0, cells, false},
        {st->pos_dev, pos_dev, false, cells * 2, 1, 0, cells * 2, false},
    };
    RowTasks a;
    int64_t blocks = 0;
    for (int q = 0; q < N_TASKS; ++q) {
        const Spec &sp = specs[q];
        const int64_t n_inner = sp.replicated && d3 ? nb : 1, n_outer = sp.replicated && d3 ? 1 : nb, reps = sp.replicated ? cells : 1;
        const int64_t len = n_inner * sp.W * reps;
        DGDM_REQUIRE(sp.W < (1ll << 30) && len < (1ll << 31) - 8, DGDM_EINVAL, "%s: a run of %lld floats (output %d) is beyond the kernel's 32-bit run index", fn,
                     (long long)len, q);
        RowTask &t = a.t[q];
        t.src = sp.src; t.out = sp.out; t.items = ids_dev + (sp.object ? nb : 0);
        t.n_outer = (unsigned)n_outer; t.n_inner = (unsigned)n_inner; t.reps = (unsigned)reps;
        t.W = (unsigned)sp.W; t.K = (unsigned)sp.K; t.D = (unsigned)sp.D; t.d0 = (unsigned)sp.d0;
        t.len = (unsigned)len;
        t.blocks_per_run = (unsigned)(((len + 6) / 4 + 255) / 256);      // threads: one per group of four, the run's start up to 3 floats into its first
        t.first_block = (unsigned)blocks;
        blocks += n_outer * (int64_t)t.blocks_per_run;
        DGDM_REQUIRE(blocks < (1ll << 31), DGDM_EINVAL, "%s: %lld workgroups", fn, (long long)blocks);
    }
    hipStream_t s = (hipStream_t)stream;
    DGDM_HIP_CHECK(hipMemcpyAsync(ids_dev, ids.data(), sizeof(int64_t) * ids.size(), hipMemcpyHostToDevice, s));      // pageable: staged before return
    hipLaunchKernelGGL(batch_rows_kernel, dim3((unsigned)blocks), dim3(256), 0, s, a);
    DGDM_HIP_CHECK(hipGetLastError());
    return DGDM_OK;
}

extern "C" int dgdm_class_agreement(const float *score_dev, const float *pred_dev, int64_t rows, const float thr[3], int64_t *agree_dev, void *stream) {
    const char *fn = "dgdm_class_agreement";
    DGDM_REQUIRE(thr && agree_dev && rows >= 0 && (rows == 0 || (score_dev && pred_dev)), DGDM_EINVAL, "%s: null argument or %lld rows", fn, (long long)rows);
    DGDM_REQUIRE((reinterpret_cast<uintptr_t>(agree_dev) & 7) == 0, DGDM_EINVAL, "%s: agree_dev is not 8-byte aligned", fn);
    hipStream_t s = (hipStream_t)stream;
    DGDM_HIP_CHECK(hipMemsetAsync(agree_dev, 0, 3 * sizeof(int64_t), s));
    if (rows == 0) return DGDM_OK;
    const unsigned grid = (unsigned)std::min<int64_t>((rows + 255) / 256, 2048);
    hipLaunchKernelGGL(class_agreement_kernel, dim3(grid), dim3(256), 0, s, score_dev, pred_dev, rows, thr[0], thr[1], thr[2],
                       reinterpret_cast<unsigned long long *>(agree_dev));
    DGDM_HIP_CHECK(hipGetLastError());
    return DGDM_OK;
}

// Small per-finger / per-cell pieces around the trunk: encoders, embeddings, first-layer tables,
// the fold of the tile partials and the backward pass through the gripper encoder.
// All of these touch O(B) or O(cells) rows (KBs..MBs) against the trunk's O(B*cells) rows.
#include "common.h"
#include "smallnet.h"
#include "philox.h"
#include <algorithm>

// No implicit a*b+c -> fma contraction in this file: the scheduler update, FPS and ball-query distances must round
// like the reference's separate float32 ops (HIP's __fmul_rn/__fadd_rn are plain * and + and would be contracted).
// Explicit fmaf() calls are unaffected.
#pragma clang fp contract(off)

namespace dgdm {

// ------------------------------------------------------------------------------------------------
// Y[r][n] = act( sum_k X[r][k] * WT[k][n] + bias[n] + rowbias[r / rb_div][n] ) (+ Y[r][n] if accumulate)
// WT is the weight stored [in][out] ("kn"), so a wave reads 64 consecutive outputs per k.
// The k loop is an in-order fmaf chain per output, like a sequential dot product.
// RB rows per workgroup (8 for a handful of rows, 32 otherwise: every weight value loaded from L2 feeds RB fmas); the k loop
// runs four at a time - four weight loads in flight, the activations as one ds_read_b128 per row - with the same ascending-k
// fmaf order per output as a one-at-a-time loop, so the result does not depend on RB or the unrolling.
template <int ACT, int RB>
__global__ __launch_bounds__(256) void linear_kernel(const float *__restrict__ X, int ldx, const float *__restrict__ WT,
                                                     const float *__restrict__ bias, const float *__restrict__ rowbias,
                                                     int rb_div, float *__restrict__ Y, int ldy, int rows, int K, int N,
                                                     int accumulate) {
    constexpr int KC = 128;
    __shared__ __attribute__((aligned(16))) float xs[RB][KC];
    const int r0 = blockIdx.x * RB;
    const int n = blockIdx.y * 256 + threadIdx.x;
    const int nn = min(n, N - 1);                       // out-of-range columns compute a copy of the last one and drop it
    float acc[RB];
#pragma unroll
    for (int r = 0; r < RB; ++r) acc[r] = 0.f;
    for (int k0 = 0; k0 < K; k0 += KC) {
        const int kc = min(KC, K - k0);
        __syncthreads();
        for (int i = threadIdx.x; i < RB * KC; i += 256) {
            const int r = i / KC, k = i - r * KC;
            xs[r][k] = (r0 + r < rows && k < kc) ? X[(size_t)(r0 + r) * ldx + k0 + k] : 0.f;
        }
        __syncthreads();
        const float *wp = WT + (size_t)k0 * N + nn;
        for (int k = 0; k < kc; k += 4) {
            // k + j >= kc only in the last group of a K that is not a multiple of 4: x is zero there, w is read from a valid row
            const float w0 = wp[(size_t)k * N], w1 = wp[(size_t)min(k + 1, kc - 1) * N], w2 = wp[(size_t)min(k + 2, kc - 1) * N],
                        w3 = wp[(size_t)min(k + 3, kc - 1) * N];
#pragma unroll
            for (int r = 0; r < RB; ++r) {
                const float4 x = *reinterpret_cast<const float4 *>(&xs[r][k]);
                acc[r] = fmaf(x.w, w3, fmaf(x.z, w2, fmaf(x.y, w1, fmaf(x.x, w0, acc[r]))));
            }
        }
    }
    if (n >= N) return;
    const float bn = bias ? bias[n] : 0.f;
#pragma unroll
    for (int r = 0; r < RB; ++r) {
        if (r0 + r >= rows) break;
        float v = acc[r] + bn;
        if (rowbias) v += rowbias[(size_t)((r0 + r) / rb_div) * N + n];
        if (accumulate) v += Y[(size_t)(r0 + r) * ldy + n];
        if (ACT == ACT_RELU) v = fmaxf(v, 0.f);
        if (ACT == ACT_SILU) v = v / (1.f + expf(-v));
        Y[(size_t)(r0 + r) * ldy + n] = v;
    }
}

template <int RB>
static void linear_launch(const float *X, int ldx, const float *WT, const float *bias, const float *rowbias, int rb_div, float *Y, int ldy,
                          int rows, int K, int N, int act, bool accumulate, hipStream_t s) {
    dim3 grid((rows + RB - 1) / RB, (N + 255) / 256);
    if (act == ACT_NONE)
        hipLaunchKernelGGL((linear_kernel<ACT_NONE, RB>), grid, dim3(256), 0, s, X, ldx, WT, bias, rowbias, rb_div, Y, ldy, rows, K, N, (int)accumulate);
    else if (act == ACT_RELU)
        hipLaunchKernelGGL((linear_kernel<ACT_RELU, RB>), grid, dim3(256), 0, s, X, ldx, WT, bias, rowbias, rb_div, Y, ldy, rows, K, N, (int)accumulate);
    else
        hipLaunchKernelGGL((linear_kernel<ACT_SILU, RB>), grid, dim3(256), 0, s, X, ldx, WT, bias, rowbias, rb_div, Y, ldy, rows, K, N, (int)accumulate);
}

int linear(const float *X, int ldx, const float *WT, const float *bias, const float *rowbias, int rb_div, float *Y, int ldy,
           int rows, int K, int N, int act, bool accumulate, hipStream_t s) {
    if (rows <= 0) return DGDM_OK;
    if (rows >= 64) linear_launch<32>(X, ldx, WT, bias, rowbias, rb_div, Y, ldy, rows, K, N, act, accumulate, s);
    else linear_launch<8>(X, ldx, WT, bias, rowbias, rb_div, Y, ldy, rows, K, N, act, accumulate, s);
    DGDM_HIP_CHECK(hipGetLastError());
    return DGDM_OK;
}

// ------------------------------------------------------------------------------------------------
// get_embedder(d, 4): [x, sin(2^k x), cos(2^k x)]_{k=0..3}  (dynamics/profile_forward_2d.py:10-56)
// pose = cat(embed(ori) [9], embed(pos) [18])  (profile_forward_2d.py:149-151) -> out[rows][27]
__global__ void pose_embed_kernel(const float *__restrict__ ori, const float *__restrict__ pos, float *__restrict__ out, int rows) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= rows) return;
    const float o = ori[r], px = pos[2 * r], py = pos[2 * r + 1];
    float *e = out + (size_t)r * 27;
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
}

__global__ void tile_table_kernel(const float *__restrict__ T, int rows, int W, float4 *__restrict__ out, int64_t total) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;      // one float4 of the output
    if (e >= total) return;
    const int lane = (int)(e & 63), n = lane & 31, h = lane >> 5;
    const int64_t t = e >> 6;
    const int q = (int)(t & 3);
    const int wb = W / 32;
    const int o = (int)((t >> 2) % wb);
    const int64_t g = (t >> 2) / wb;
    const int64_t r = min((int64_t)32 * g + n, (int64_t)rows - 1);
    out[e] = *reinterpret_cast<const float4 *>(T + r * W + 32 * o + 8 * q + 4 * h);
}

int tile_table(const float *T, int rows, int W, float *out, hipStream_t s) {
    const int64_t total = (int64_t)((rows + 31) / 32) * (W / 32) * 4 * 64;
    hipLaunchKernelGGL(tile_table_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, T, rows, W, reinterpret_cast<float4 *>(out), total);
    DGDM_HIP_CHECK(hipGetLastError());
    return DGDM_OK;
}

int pose_embed(const float *ori, const float *pos, float *out, int rows, hipStream_t s) {
    if (rows <= 0) return DGDM_OK;
    hipLaunchKernelGGL(pose_embed_kernel, dim3((rows + 255) / 256), dim3(256), 0, s, ori, pos, out, rows);
    DGDM_HIP_CHECK(hipGetLastError());
    return DGDM_OK;
}

// timestep_embedding(t, dim): [cos(t f_i) | sin(t f_i)], f_i from the host (profile_forward_2d.py:58-76)
__global__ void time_embed_kernel(const float *__restrict__ t, float t_scalar, const float *__restrict__ freqs, float *__restrict__ out,
                                  int rows, int half) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows * half) return;
    const int r = i / half, j = i - r * half;
    const float a = (t ? t[r] : t_scalar) * freqs[j];
    out[(size_t)r * 2 * half + j] = cosf(a);
    out[(size_t)r * 2 * half + half + j] = sinf(a);
}

int time_embed(const float *t_dev, float t_scalar, const float *freqs, float *out, int rows, int half, hipStream_t s) {
    if (rows <= 0) return DGDM_OK;
    hipLaunchKernelGGL(time_embed_kernel, dim3((rows * half + 255) / 256), dim3(256), 0, s, t_dev, t_scalar, freqs, out, rows, half);
    DGDM_HIP_CHECK(hipGetLastError());
    return DGDM_OK;
}

// ------------------------------------------------------------------------------------------------
// Backward tail of cond_fn for one finger of one chain (what autograd does after the trunk,
// generator/diffusion.py:498,504): fold the tile partials over cells, then go back through
// W1'[:, ctrl part], gripper_encoder.2, ReLU, gripper_encoder.0 (profile_forward_2d.py:103-107,148).
template <int W1>
__global__ __launch_bounds__(256) void dyn_post_kernel(const float *__restrict__ partial, int tiles_per_b,
                                                       const float *__restrict__ w1c /*[W1][256]*/,
                                                       const float *__restrict__ g2w /*[256][256]*/,
                                                       const float *__restrict__ g0w /*[256][L]*/,
                                                       const float *__restrict__ V /*[rows][256] relu(g0 x + b)*/,
                                                       float *__restrict__ grad /*[rows][L]*/, int L) {
    __shared__ float da[W1];
    __shared__ float v1[256];
    __shared__ float v2[256];
    const int row = blockIdx.x, t = threadIdx.x;
    for (int f = t; f < W1; f += 256) {
        const float *src = partial + (size_t)row * tiles_per_b * W1 + f;
        float acc = 0.f;
        for (int ct = 0; ct < tiles_per_b; ++ct) acc += src[(size_t)ct * W1];
        da[f] = acc;
    }
    __syncthreads();
    float acc = 0.f;
    for (int f = 0; f < W1; ++f) acc = fmaf(w1c[(size_t)f * 256 + t], da[f], acc);
    v1[t] = acc;
    __syncthreads();
    acc = 0.f;
    for (int f = 0; f < 256; ++f) acc = fmaf(g2w[(size_t)f * 256 + t], v1[f], acc);
    v2[t] = V[(size_t)row * 256 + t] > 0.f ? acc : 0.f;
    __syncthreads();
    if (t < L) {
        acc = 0.f;
        for (int f = 0; f < 256; ++f) acc = fmaf(g0w[(size_t)f * L + t], v2[f], acc);
        grad[(size_t)row * L + t] = acc;
    }
}

int dyn_post(int W1, const float *partial, int tiles_per_b, const float *w1c, const float *g2w, const float *g0w, const float *V,
             float *grad, int rows, int L, hipStream_t s) {
    if (rows <= 0) return DGDM_OK;
    DGDM_REQUIRE(L <= 256, DGDM_EINVAL, "params_ch %d > 256 not supported", L);
    if (W1 == 256)
        hipLaunchKernelGGL(dyn_post_kernel<256>, dim3(rows), dim3(256), 0, s, partial, tiles_per_b, w1c, g2w, g0w, V, grad, L);
    else
        hipLaunchKernelGGL(dyn_post_kernel<512>, dim3(rows), dim3(256), 0, s, partial, tiles_per_b, w1c, g2w, g0w, V, grad, L);
    DGDM_HIP_CHECK(hipGetLastError());
    return DGDM_OK;
}

// ------------------------------------------------------------------------------------------------
// Float64 versions of the per-finger / per-cell / per-object stages (smallnet.h).  Sizes are KBs..MBs: a thread per output column,
// RB rows per workgroup, X staged in LDS as doubles.
template <int ACT, int RB>
__global__ __launch_bounds__(256) void linear64_kernel(const float *__restrict__ Xf, const double *__restrict__ Xd, int ldx,
                                                       const double *__restrict__ WT, const double *__restrict__ bias,
                                                       const double *__restrict__ rowbias, int rb_div, double *__restrict__ Yd,
                                                       float *__restrict__ Yf, int ldy, int rows, int K, int N) {
    constexpr int KC = 64, KU = KC / 2;
    __shared__ double xs[RB][KC];
    const int r0 = blockIdx.x * RB;
    const int n = blockIdx.y * 256 + threadIdx.x;
    const int nn = min(n, N - 1);
    double acc[RB];
#pragma unroll
    for (int r = 0; r < RB; ++r) acc[r] = 0.0;
    for (int k0 = 0; k0 < K; k0 += KC) {
        const int kc = min(KC, K - k0);
        const double *wp = WT + (size_t)k0 * N + nn;
        double w0[KU], w1[KU];
#pragma unroll
        for (int j = 0; j < KU; ++j) w0[j] = wp[(size_t)min(j, kc - 1) * N];
        __syncthreads();
        for (int i = threadIdx.x; i < RB * KC; i += 256) {
            const int r = i / KC, k = i - r * KC;
            double v = 0.0;
            if (r0 + r < rows && k < kc) v = Xd ? Xd[(size_t)(r0 + r) * ldx + k0 + k] : (double)Xf[(size_t)(r0 + r) * ldx + k0 + k];
            xs[r][k] = v;
        }
        __syncthreads();
        // the loop is L2-latency bound: the chunk's first KU weights are loaded above, beside the staging of X, its other KU before
        // the first half's fma chain - up to 64 loads in flight per thread; the fma order (k ascending, one accumulator per output) is
        // that of a one-at-a-time loop
        if (kc > KU) {
#pragma unroll
            for (int j = 0; j < KU; ++j) w1[j] = wp[(size_t)min(KU + j, kc - 1) * N];
        }
#pragma unroll
        for (int j = 0; j < KU; ++j) {
            if (j < kc) {
#pragma unroll
                for (int r = 0; r < RB; ++r) acc[r] = fma(xs[r][j], w0[j], acc[r]);
            }
        }
        if (kc > KU) {
#pragma unroll
            for (int j = 0; j < KU; ++j) {
                if (KU + j < kc) {
#pragma unroll
                    for (int r = 0; r < RB; ++r) acc[r] = fma(xs[r][KU + j], w1[j], acc[r]);
                }
            }
        }
    }
    if (n >= N) return;
    const double bn = bias ? bias[n] : 0.0;
#pragma unroll
    for (int r = 0; r < RB; ++r) {
        if (r0 + r >= rows) break;
        double v = acc[r] + bn;
        if (rowbias) v += rowbias[(size_t)((r0 + r) / rb_div) * N + n];
        if (ACT == ACT_RELU) v = fmax(v, 0.0);
        if (ACT == ACT_SILU) v = v / (1.0 + exp(-v));
        if (Yd) Yd[(size_t)(r0 + r) * ldy + n] = v;
        if (Yf) Yf[(size_t)(r0 + r) * ldy + n] = (float)v;
    }
}

int linear64(const float *Xf, const double *Xd, int ldx, const double *WT, const double *bias, const double *rowbias, int rb_div,
             double *Yd, float *Yf, int ldy, int rows, int K, int N, int act, hipStream_t s) {
    if (rows <= 0) return DGDM_OK;
    constexpr int RB = 8;
    dim3 grid((rows + RB - 1) / RB, (N + 255) / 256);
    if (act == ACT_NONE)
        hipLaunchKernelGGL((linear64_kernel<ACT_NONE, RB>), grid, dim3(256), 0, s, Xf, Xd, ldx, WT, bias, rowbias, rb_div, Yd, Yf, ldy, rows, K, N);
    else if (act == ACT_RELU)
        hipLaunchKernelGGL((linear64_kernel<ACT_RELU, RB>), grid, dim3(256), 0, s, Xf, Xd, ldx, WT, bias, rowbias, rb_div, Yd, Yf, ldy, rows, K, N);
    else
        hipLaunchKernelGGL((linear64_kernel<ACT_SILU, RB>), grid, dim3(256), 0, s, Xf, Xd, ldx, WT, bias, rowbias, rb_div, Yd, Yf, ldy, rows, K, N);
    DGDM_HIP_CHECK(hipGetLastError());
    return DGDM_OK;
}

__global__ void gather_add64_kernel(const double *__restrict__ a, const int *__restrict__ idx, const double *__restrict__ b,
                                    double *__restrict__ out, int groups, int N) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= groups * N) return;
    const int g = i / N, n = i - g * N;
    out[i] = a[(size_t)idx[g] * N + n] + b[n];
}

int gather_add64(const double *a, const int *idx, const double *b, double *out, int groups, int N, hipStream_t s) {
    if (groups <= 0) return DGDM_OK;
    hipLaunchKernelGGL(gather_add64_kernel, dim3((groups * N + 255) / 256), dim3(256), 0, s, a, idx, b, out, groups, N);
    DGDM_HIP_CHECK(hipGetLastError());
    return DGDM_OK;
}

// cond_fn's backward tail in float64 for RB fingers per workgroup.  A finger alone reads all three weight matrices (1.6 MB at W1 = 512)
// from L2 for 1024 dependent fmas per thread: 1024 fingers made that 1.7 GB of L2 traffic per call, in groups of eight loads.  Here
// every weight value loaded feeds RB fmas (as in linear64_kernel), U loads are issued per step and the next step's before this
// step's fma chains.  Each output still has its one accumulator and takes its terms in ascending f, so the result does not depend
// on RB or U; no dot product is split across threads.
template <int W1, int RB>
__global__ __launch_bounds__(256) void dyn_post64_kernel(const float *__restrict__ partial, int tiles_per_b,
                                                         const double *__restrict__ w1c /*[W1][256]*/,
                                                         const double *__restrict__ g2w /*[256][256]*/,
                                                         const double *__restrict__ g0w /*[256][L]*/,
                                                         const double *__restrict__ V /*[rows][256] relu(g0 x + b)*/,
                                                         float *__restrict__ grad /*[rows][L]*/, int rows, int L) {
    __shared__ __attribute__((aligned(16))) double da[W1][RB];
    __shared__ __attribute__((aligned(16))) double v1[256][RB];
    __shared__ __attribute__((aligned(16))) double v2[256][RB];
    const int r0 = blockIdx.x * RB, t = threadIdx.x;
    // the fold over the cell tiles: twelve partials of a feature loaded before their adds (ct ascending, as a one-at-a-time loop adds
    // them); rows past the end fold a copy of the last row and are dropped at the store
    constexpr int CU = 12;
    for (int i = t; i < RB * W1; i += 256) {
        const int r = i / W1, f = i - r * W1;
        const float *src = partial + (size_t)min(r0 + r, rows - 1) * tiles_per_b * W1 + f;
        double acc = 0.0;
        for (int c0 = 0; c0 < tiles_per_b; c0 += CU) {
            float pv[CU];
#pragma unroll
            for (int j = 0; j < CU; ++j) pv[j] = src[(size_t)min(c0 + j, tiles_per_b - 1) * W1];
#pragma unroll
            for (int j = 0; j < CU; ++j)
                if (c0 + j < tiles_per_b) acc += (double)pv[j];
        }
        da[f][r] = acc;
    }
    __syncthreads();
    // acc[r] = sum_f w[f][t] x[f][r]  (F a multiple of 2 U)
    constexpr int U = 16;
    auto dot = [&](const double *__restrict__ w, int ld, const double (*x)[RB], int F, double (&acc)[RB]) {
        double wa[U], wb[U];
#pragma unroll
        for (int r = 0; r < RB; ++r) acc[r] = 0.0;
#pragma unroll
        for (int j = 0; j < U; ++j) wa[j] = w[(size_t)j * ld + t];
        for (int f = 0; f < F; f += 2 * U) {
#pragma unroll
            for (int j = 0; j < U; ++j) wb[j] = w[(size_t)(f + U + j) * ld + t];
#pragma unroll
            for (int j = 0; j < U; ++j)
#pragma unroll
                for (int r = 0; r < RB; ++r) acc[r] = fma(wa[j], x[f + j][r], acc[r]);
            if (f + 2 * U < F) {
#pragma unroll
                for (int j = 0; j < U; ++j) wa[j] = w[(size_t)(f + 2 * U + j) * ld + t];
            }
#pragma unroll
            for (int j = 0; j < U; ++j)
#pragma unroll
                for (int r = 0; r < RB; ++r) acc[r] = fma(wb[j], x[f + U + j][r], acc[r]);
        }
    };
    static_assert(W1 % (2 * U) == 0 && 256 % (2 * U) == 0, "dyn_post64_kernel: dot product lengths are multiples of 2 U");
    double acc[RB];
    dot(w1c, 256, da, W1, acc);
#pragma unroll
    for (int r = 0; r < RB; ++r) v1[t][r] = acc[r];
    __syncthreads();
    dot(g2w, 256, v1, 256, acc);
#pragma unroll
    for (int r = 0; r < RB; ++r) v2[t][r] = V[(size_t)min(r0 + r, rows - 1) * 256 + t] > 0.0 ? acc[r] : 0.0;
    __syncthreads();
    if (t < L) {
        dot(g0w, L, v2, 256, acc);
#pragma unroll
        for (int r = 0; r < RB; ++r)
            if (r0 + r < rows) grad[(size_t)(r0 + r) * L + t] = (float)acc[r];
    }
}

int dyn_post64(int W1, const float *partial, int tiles_per_b, const double *w1c, const double *g2w, const double *g0w, const double *V64,
               float *grad, int rows, int L, hipStream_t s) {
    if (rows <= 0) return DGDM_OK;
    DGDM_REQUIRE(L <= 256, DGDM_EINVAL, "params_ch %d > 256 not supported", L);
    constexpr int RB = 4;       // 1024 fingers (32 chains of 32): one workgroup per CU
    const dim3 grid((rows + RB - 1) / RB);
    if (W1 == 256)
        hipLaunchKernelGGL((dyn_post64_kernel<256, RB>), grid, dim3(256), 0, s, partial, tiles_per_b, w1c, g2w, g0w, V64, grad, rows, L);
    else
        hipLaunchKernelGGL((dyn_post64_kernel<512, RB>), grid, dim3(256), 0, s, partial, tiles_per_b, w1c, g2w, g0w, V64, grad, rows, L);
    DGDM_HIP_CHECK(hipGetLastError());
    return DGDM_OK;
}

// ------------------------------------------------------------------------------------------------
// a13/a14: guidance combine + DDIM(eta=0, clip) step, elementwise (see dgdm_hip.h).  BOUNDED: the clip of the predicted clean sample is
// per entry, [lo, hi] of entry i % period, instead of clip_sample=True's [-1, 1] (editing a design); the plain instantiation neither forms
// the index nor reads lo / hi.  Everything but the clamp's operands is one sequence, so lo = -1, hi = 1 gives the plain step's bits;
// lo == hi pins x0, and with sap = 1, sbp = 0 (the last step) the output is that value exactly.
// NOISY (eta > 0): out = sap x0 + dir eps + sigma z, with sbp holding dir; z is noise[i] or the keyed normal of dgdm_hip.h.  The
// instantiations without it never form the chain index or touch StepNoise.
struct StepNoise {
    float sigma;
    const float *noise;             // explicit z, or nullptr: the keyed normal
    uint64_t seed;
    const uint64_t *chain_keys;     // [n / per_chain]
    uint64_t step_index;
    int64_t per_chain;
};

// The recipe of include/dgdm_hip.h: element e of the chain keyed (seed, key) at step_index -> a standard normal, float64 until the end.
__device__ inline float keyed_normal(uint64_t seed, uint64_t key, uint64_t step_index, uint64_t e) {
    const U64x4 r = philox4x64_10(U64x4{{e / 2 + 1, step_index, 0, 0}}, seed, key);
    const int lane = 2 * (int)(e & 1);
    const double u1 = (double)((r.v[lane] >> 11) + 1) * 0x1.0p-53, u2 = (double)(r.v[lane + 1] >> 11) * 0x1.0p-53;
    return (float)(sqrt(-2.0 * log(u1)) * cos(6.283185307179586 * u2));
}

template <bool BOUNDED, bool NOISY>
__global__ void ddim_step_kernel(const float *__restrict__ x, const float *__restrict__ eps, const float *__restrict__ grad,
                                 int n_grad, float *__restrict__ out, int64_t n, float sa, float sb, float sap, float sbp,
                                 float scale, const float *__restrict__ lo, const float *__restrict__ hi, int64_t period, StepNoise nz) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float cl = -1.f, ch = 1.f;
    if constexpr (BOUNDED) {
        const int64_t j = i % period;
        cl = lo[j];
        ch = hi[j];
    }
    float e = eps[i];
    if (grad) {
        float g = grad[i];
        if (n_grad > 1) {                       // grad = 0.0; grad += g_k; grad /= n   (diffusion.py:640-644)
            g = 0.f + g;
            for (int k = 1; k < n_grad; ++k) g += grad[(size_t)k * n + i];
            g = g / (float)n_grad;
        }
        e = sub_rn(e, mul_rn(mul_rn(sb, g), scale));           // eps - (sqrt(1-abar) * grad) * scale, unfused
    }
    float x0 = __fdiv_rn(sub_rn(x[i], mul_rn(sb, e)), sa);        // (x - sqrt(1-abar) eps) / sqrt(abar)
    x0 = fminf(fmaxf(x0, cl), ch);
    if constexpr (NOISY) {
        const int64_t c = i / nz.per_chain;
        const float z = nz.noise ? nz.noise[i] : keyed_normal(nz.seed, nz.chain_keys[c], nz.step_index, (uint64_t)(i - c * nz.per_chain));
        out[i] = add_rn(add_rn(mul_rn(sap, x0), mul_rn(sbp, e)), mul_rn(nz.sigma, z));
    } else {
        out[i] = add_rn(mul_rn(sap, x0), mul_rn(sbp, e));
    }
}

__global__ void step_noise_kernel(uint64_t seed, const uint64_t *__restrict__ chain_keys, uint64_t step_index, int64_t per_chain, int64_t n,
                                  float *__restrict__ z) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t c = i / per_chain;
    z[i] = keyed_normal(seed, chain_keys[c], step_index, (uint64_t)(i - c * per_chain));
}

__global__ void add_noise_kernel(const float *__restrict__ x0, const float *__restrict__ noise, float *__restrict__ out, int64_t n,
                                 float sa, float sb) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = add_rn(mul_rn(sa, x0[i]), mul_rn(sb, noise[i]));
}

// The predicted clean sample ddim_step_kernel forms, on its own: the unguided eps, the [-1, 1] clip, the same helpers in the same order.
__global__ void pred_x0_kernel(const float *__restrict__ x, const float *__restrict__ eps, float *__restrict__ out, int64_t n, float sa, float sb) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = fminf(fmaxf(__fdiv_rn(sub_rn(x[i], mul_rn(sb, eps[i])), sa), -1.f), 1.f);
}

}  // namespace dgdm

// lo_dev == nullptr: the plain step; nz == nullptr or sigma == 0: the eta = 0 instantiations.  bytes: what prof_end books for the stage.
static int ddim_step_launch(const float *x_dev, const float *eps_dev, const float *grad_dev, int n_grad, float *x_next_dev, int64_t n, float sa,
                            float sb, float sap, float sbp, float scale, const float *lo_dev, const float *hi_dev, int64_t period, double bytes,
                            hipStream_t s, const dgdm::StepNoise *nz = nullptr) {
    if (n == 0) return DGDM_OK;
    const dim3 grid((unsigned)((n + 255) / 256));
    const dgdm::StepNoise none{};
    dgdm::prof_begin(s, DGDM_STAGE_DDIM);
    if (nz && nz->sigma != 0.f) {
        if (lo_dev)
            hipLaunchKernelGGL((dgdm::ddim_step_kernel<true, true>), grid, dim3(256), 0, s, x_dev, eps_dev, grad_dev, n_grad, x_next_dev, n, sa, sb, sap,
                               sbp, scale, lo_dev, hi_dev, period, *nz);
        else
            hipLaunchKernelGGL((dgdm::ddim_step_kernel<false, true>), grid, dim3(256), 0, s, x_dev, eps_dev, grad_dev, n_grad, x_next_dev, n, sa, sb, sap,
                               sbp, scale, nullptr, nullptr, (int64_t)0, *nz);
    } else if (lo_dev)
        hipLaunchKernelGGL((dgdm::ddim_step_kernel<true, false>), grid, dim3(256), 0, s, x_dev, eps_dev, grad_dev, n_grad, x_next_dev, n, sa, sb, sap, sbp,
                           scale, lo_dev, hi_dev, period, none);
    else
        hipLaunchKernelGGL((dgdm::ddim_step_kernel<false, false>), grid, dim3(256), 0, s, x_dev, eps_dev, grad_dev, n_grad, x_next_dev, n, sa, sb, sap, sbp,
                           scale, nullptr, nullptr, (int64_t)0, none);
    dgdm::prof_end(s, DGDM_STAGE_DDIM, bytes);
    DGDM_HIP_CHECK(hipGetLastError());
    return DGDM_OK;
}

extern "C" int dgdm_ddim_guided_step(const float *x_dev, const float *eps_dev, const float *grad_dev, int n_grad, float *x_next_dev,
                                     int64_t n, float sqrt_abar_t, float sqrt_1m_abar_t, float sqrt_abar_prev,
                                     float sqrt_1m_abar_prev, float guidance_scale, void *stream) {
    DGDM_REQUIRE(x_dev && eps_dev && x_next_dev && n >= 0, DGDM_EINVAL, "dgdm_ddim_guided_step: null argument");
    return ddim_step_launch(x_dev, eps_dev, grad_dev, n_grad, x_next_dev, n, sqrt_abar_t, sqrt_1m_abar_t, sqrt_abar_prev, sqrt_1m_abar_prev,
                            guidance_scale, nullptr, nullptr, 0, (double)n * 4.0 * (3 + n_grad), (hipStream_t)stream);
}

extern "C" int dgdm_ddim_guided_step_bounded(const float *x_dev, const float *eps_dev, const float *grad_dev, int n_grad, float *x_next_dev,
                                             int64_t n, float sqrt_abar_t, float sqrt_1m_abar_t, float sqrt_abar_prev,
                                             float sqrt_1m_abar_prev, float guidance_scale, const float *lo_dev, const float *hi_dev,
                                             int64_t period, void *stream) {
    DGDM_REQUIRE(x_dev && eps_dev && x_next_dev && n >= 0, DGDM_EINVAL, "dgdm_ddim_guided_step_bounded: null argument");
    DGDM_REQUIRE(lo_dev && hi_dev, DGDM_EINVAL, "dgdm_ddim_guided_step_bounded: needs both lo and hi");
    DGDM_REQUIRE(period > 0 && n % period == 0, DGDM_EINVAL, "dgdm_ddim_guided_step_bounded: period %lld does not divide n = %lld", (long long)period,
                 (long long)n);
    return ddim_step_launch(x_dev, eps_dev, grad_dev, n_grad, x_next_dev, n, sqrt_abar_t, sqrt_1m_abar_t, sqrt_abar_prev, sqrt_1m_abar_prev,
                            guidance_scale, lo_dev, hi_dev, period, (double)n * 4.0 * (5 + n_grad), (hipStream_t)stream);
}

extern "C" int dgdm_ddim_guided_step_noisy(const float *x_dev, const float *eps_dev, const float *grad_dev, int n_grad, float *x_next_dev, int64_t n,
                                           float sqrt_abar_t, float sqrt_1m_abar_t, float sqrt_abar_prev, float dir, float guidance_scale,
                                           const float *lo_dev, const float *hi_dev, int64_t period, float sigma, const float *noise_dev,
                                           uint64_t seed, const uint64_t *chain_keys_dev, int64_t step_index, int64_t per_chain, void *stream) {
    const char *fn = "dgdm_ddim_guided_step_noisy";
    DGDM_REQUIRE(x_dev && eps_dev && x_next_dev && n >= 0, DGDM_EINVAL, "%s: null argument", fn);
    DGDM_REQUIRE(!lo_dev == !hi_dev, DGDM_EINVAL, "%s: lo and hi come together or not at all", fn);
    DGDM_REQUIRE(!lo_dev || (period > 0 && n % period == 0), DGDM_EINVAL, "%s: period %lld does not divide n = %lld", fn, (long long)period, (long long)n);
    DGDM_REQUIRE(sigma >= 0.f && sigma <= 3.0e38f, DGDM_EINVAL, "%s: sigma %g is not a finite non-negative number", fn, (double)sigma);
    if (sigma != 0.f && !noise_dev) {
        DGDM_REQUIRE(chain_keys_dev, DGDM_EINVAL, "%s: sigma > 0 needs noise_dev or chain_keys_dev", fn);
        DGDM_REQUIRE(step_index >= 0, DGDM_EINVAL, "%s: step_index %lld is negative", fn, (long long)step_index);
        DGDM_REQUIRE(per_chain > 0 && n % per_chain == 0, DGDM_EINVAL, "%s: per_chain %lld does not divide n = %lld", fn, (long long)per_chain, (long long)n);
    }
    // with explicit noise the chain index is formed but never used: any positive per_chain will do
    const dgdm::StepNoise nz{sigma, noise_dev, seed, chain_keys_dev, (uint64_t)step_index, noise_dev ? std::max<int64_t>(1, n) : per_chain};
    return ddim_step_launch(x_dev, eps_dev, grad_dev, n_grad, x_next_dev, n, sqrt_abar_t, sqrt_1m_abar_t, sqrt_abar_prev, dir, guidance_scale, lo_dev,
                            hi_dev, period, (double)n * 4.0 * ((lo_dev ? 5 : 3) + n_grad + (noise_dev && sigma != 0.f ? 1 : 0)), (hipStream_t)stream, &nz);
}

extern "C" int dgdm_ddim_step_noise(uint64_t seed, const uint64_t *chain_keys_dev, int n_chains, int64_t step_index, int64_t per_chain, float *z_dev,
                                    void *stream) {
    DGDM_REQUIRE(chain_keys_dev && z_dev, DGDM_EINVAL, "dgdm_ddim_step_noise: null argument");
    DGDM_REQUIRE(n_chains >= 0 && per_chain >= 0 && step_index >= 0, DGDM_EINVAL, "dgdm_ddim_step_noise: negative argument");
    const int64_t n = (int64_t)n_chains * per_chain;
    if (n == 0) return DGDM_OK;
    hipLaunchKernelGGL(dgdm::step_noise_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, seed, chain_keys_dev,
                       (uint64_t)step_index, per_chain, n, z_dev);
    DGDM_HIP_CHECK(hipGetLastError());
    return DGDM_OK;
}

extern "C" int dgdm_ddim_add_noise(const float *x0_dev, const float *noise_dev, float *out_dev, int64_t n, float sqrt_abar,
                                   float sqrt_1m_abar, void *stream) {
    DGDM_REQUIRE(x0_dev && noise_dev && out_dev && n >= 0, DGDM_EINVAL, "dgdm_ddim_add_noise: null argument");
    if (n == 0) return DGDM_OK;
    hipLaunchKernelGGL(dgdm::add_noise_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x0_dev, noise_dev,
                       out_dev, n, sqrt_abar, sqrt_1m_abar);
    DGDM_HIP_CHECK(hipGetLastError());
    return DGDM_OK;
}

extern "C" int dgdm_ddim_pred_x0(const float *x_dev, const float *eps_dev, float *out_dev, int64_t n, float sqrt_abar_t, float sqrt_1m_abar_t,
                                 void *stream) {
    DGDM_REQUIRE(x_dev && eps_dev && out_dev && n >= 0, DGDM_EINVAL, "dgdm_ddim_pred_x0: null argument");
    if (n == 0) return DGDM_OK;
    hipLaunchKernelGGL(dgdm::pred_x0_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x_dev, eps_dev, out_dev, n,
                       sqrt_abar_t, sqrt_1m_abar_t);
    DGDM_HIP_CHECK(hipGetLastError());
    return DGDM_OK;
}

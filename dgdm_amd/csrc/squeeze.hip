// Squeeze simulator: a model-free, frictionless, quasi-static parallel-jaw squeeze of a polygon by two finger surfaces, tabulated on a
// (theta, x) grid.  The contract, exact in float64 and int32, is include/dgdm_hip.h "squeeze simulator" (DESIGN.md §4.1d);
// tests/squeeze_oracle.py is its CPU oracle, which these kernels reproduce bit for bit.
//
// Launches of dgdm_squeeze_map per chunk of pairs, all on the caller's stream, no host wait in between:
//   1. table_kernel     one workgroup per (pair, theta): the two surfaces and the rotated vertices staged in LDS once, lanes on the x
//                       cells; each lane walks the vertices (set A) and the finger samples under each edge (set B) and keeps the two
//                       minima in registers - no atomics, no cross-lane reduction;
//   2. successor_kernel one thread per cell: the (2R + 1)^2 - 1 neighbours of S in the contract's visiting order;
//   3. apply_kernel / square_kernel, ceil(log2(cells)) rounds of pointer doubling, int32 only: round r holds succ^(2^r); the k-th
//                       successor collects the rounds of k's set bits, the last square is the fixed point;
//   4. lookup_kernel    one thread per (pair, start): snap, read the two maps, y and flags.
// This file is compiled with -ffp-contract=off (build.py): no operation of the contract is fused.
#include "common.h"
#include <cmath>

namespace dgdm {
namespace {

constexpr int TABLE_THREADS = 256;
constexpr int MAX_SURFACE = 1024, MAX_VERTS = 1024;     // (2 m + 2 nv) doubles of LDS: 32 KB at the limits
constexpr double TWO_PI = 6.283185307179586;

struct Grid {
    int T, X, R, m, nv;
    double x_half, dx, hl, h, travel_max;
};

// touch_l / touch_r / S [pairs][T][X] of this chunk.  Grid: (T, pairs) workgroups.
__global__ __launch_bounds__(TABLE_THREADS) void table_kernel(Grid g, const double *surfaces, const double *objects, const int32_t *pairs,
                                                              const double *rot, double *touch_l, double *touch_r, double *S) {
    extern __shared__ double lds[];
    double *sL = lds, *sU = lds + g.m, *sRx = lds + 2 * g.m, *sRy = sRx + g.nv;
    const int a = blockIdx.x, p = blockIdx.y;
    const double *sf = surfaces + (int64_t)pairs[2 * p] * 2 * g.m;
    const double *ov = objects + (int64_t)pairs[2 * p + 1] * 2 * g.nv;
    const double c = rot[2 * a], s = rot[2 * a + 1];
    for (int i = threadIdx.x; i < g.m; i += TABLE_THREADS) {
        sL[i] = sf[i];
        sU[i] = sf[g.m + i];
    }
    for (int i = threadIdx.x; i < g.nv; i += TABLE_THREADS) {
        const double vx = ov[2 * i], vy = ov[2 * i + 1];
        sRx[i] = c * vx - s * vy;
        sRy[i] = s * vx + c * vy;
    }
    __syncthreads();
    const double hl = g.hl, h = g.h, inf = INFINITY;
    const double jA = (double)(g.m - 2), jB = (double)(g.m - 1);
    for (int b = threadIdx.x; b < g.X; b += TABLE_THREADS) {
        const double xg = -g.x_half + (double)b * g.dx;
        double gl = inf, gu = inf;
        // t = (x + hl) / h of a vertex serves set A and, x -> t being monotone, both ends of the two edges' sample ranges:
        // (min(xa, xb) + hl) / h is the smaller of the two t, bit for bit - one quotient per vertex instead of three
        double px = sRx[0] + xg, py = sRy[0];
        double t = (px + hl) / h;
        for (int i = 0; i < g.nv; ++i) {
            const int i1 = i + 1 == g.nv ? 0 : i + 1;
            const double qx = sRx[i1] + xg, qy = sRy[i1];
            const double tq = (qx + hl) / h;
            if (px >= -hl && px <= hl) {                                   // set A: this vertex against the interpolated surfaces
                const double jf = fmin(floor(t), jA);
                const int j = (int)jf;                                     // 0 .. m - 2: t >= 0
                const double f = t - jf;
                const double l0 = sL[j], u0 = sU[j];
                const double lp = l0 + f * (sL[j + 1] - l0);
                const double up = u0 + f * (sU[j + 1] - u0);
                gl = fmin(gl, py - lp);
                gu = fmin(gu, up - py);
            }
            if (px != qx) {                                                // set B: the finger samples under the edge P -> Q
                const double j0 = fmax(ceil(fmin(t, tq)), 0.0);
                const double j1 = fmin(floor(fmax(t, tq)), jB);
                if (j0 <= j1) {                                            // both in 0 .. m - 1 then (false for a NaN)
                    const double slope = (qy - py) / (qx - px);
                    const int je = (int)j1;
                    for (int j = (int)j0; j <= je; ++j) {
                        const double uj = -hl + (double)j * h;
                        const double ye = py + (uj - px) * slope;
                        gl = fmin(gl, ye - sL[j]);
                        gu = fmin(gu, sU[j] - ye);
                    }
                }
            }
            px = qx;
            py = qy;
            t = tq;
        }
        const int64_t o = ((int64_t)p * g.T + a) * g.X + b;
        touch_l[o] = gl;
        touch_r[o] = gu;
        S[o] = (gl + gu) / 2.0;
    }
}

// succ [pairs][cells]: the neighbour with the greatest S, visited in ascending (|db|, |da|, da, db), replaced on strictly greater only.
__global__ void successor_kernel(Grid g, const double *S, int32_t *succ) {
    const int cells = g.T * g.X;
    const int cell = blockIdx.x * blockDim.x + threadIdx.x;
    if (cell >= cells) return;
    const double *Sp = S + (int64_t)blockIdx.y * cells;
    const int a = cell / g.X, b = cell - a * g.X;
    double best = Sp[cell];
    int arg = cell;
    if (!(best >= g.travel_max)) {
        for (int adb = 0; adb <= g.R; ++adb)
            for (int ada = 0; ada <= g.R; ++ada)
                for (int sa = 0; sa < (ada ? 2 : 1); ++sa)
                    for (int sb = 0; sb < (adb ? 2 : 1); ++sb) {
                        const int da = sa ? ada : -ada, db = sb ? adb : -adb;
                        const int b2 = b + db;
                        if ((ada | adb) == 0 || b2 < 0 || b2 >= g.X) continue;
                        int a2 = (a + da) % g.T;
                        if (a2 < 0) a2 += g.T;
                        const int c2 = a2 * g.X + b2;
                        const double v = Sp[c2];
                        if (v > best) { best = v; arg = c2; }
                    }
    }
    succ[(int64_t)blockIdx.y * cells + cell] = arg;
}

__global__ void iota_kernel(int cells, int32_t *out) {
    const int cell = blockIdx.x * blockDim.x + threadIdx.x;
    if (cell < cells) out[(int64_t)blockIdx.y * cells + cell] = cell;
}

// res = power o res (res is read and written by its own thread only)
__global__ void apply_kernel(int cells, const int32_t *power, int32_t *res) {
    const int cell = blockIdx.x * blockDim.x + threadIdx.x;
    if (cell >= cells) return;
    const int64_t o = (int64_t)blockIdx.y * cells;
    res[o + cell] = power[o + res[o + cell]];
}

// out = in o in
__global__ void square_kernel(int cells, const int32_t *in, int32_t *out) {
    const int cell = blockIdx.x * blockDim.x + threadIdx.x;
    if (cell >= cells) return;
    const int64_t o = (int64_t)blockIdx.y * cells;
    out[o + cell] = in[o + in[o + cell]];
}

__device__ double pose_y(double y0, double tl, double tr, double S, double tm) {
    if (S < tm) return (tr - tl) / 2.0;
    const double lo = tm - tl, hi = tr - tm;
    double y = y0;
    if (y < lo) y = lo;
    if (y > hi) y = hi;
    return y;
}

// Per (pair, start): cells (start, closed, settled), y (closed, settled), flags.  `pair0`: the chunk's first pair in the outputs.
__global__ void lookup_kernel(Grid g, const double *starts, int n_starts, const double *touch_l, const double *touch_r, const double *S,
                              const int32_t *kth, const int32_t *fix, int pair0, int32_t *cells_out, double *y_out, int32_t *flags_out) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= n_starts) return;
    const int cells = g.T * g.X;
    const int64_t o = (int64_t)blockIdx.y * cells;
    const double th = starts[3 * n], x0 = starts[3 * n + 1], y0 = starts[3 * n + 2];
    const double dth = TWO_PI / (double)g.T;
    const double q = floor(th / dth + 0.5);
    const double v = q - (double)g.T * floor(q / (double)g.T);
    const int a = (v >= 0.0 && v < (double)g.T) ? (int)v : 0;
    double w = floor((x0 + g.x_half) / g.dx + 0.5);
    if (!(w >= 0.0)) w = 0.0;
    if (!(w <= (double)(g.X - 1))) w = (double)(g.X - 1);
    const int c0 = a * g.X + (int)w;
    const int ck = kth[o + c0], cf = fix[o + c0];
    const int bf = cf % g.X;
    const int64_t r = (int64_t)(pair0 + blockIdx.y) * n_starts + n;
    cells_out[3 * r] = c0;
    cells_out[3 * r + 1] = ck;
    cells_out[3 * r + 2] = cf;
    y_out[2 * r] = pose_y(y0, touch_l[o + ck], touch_r[o + ck], S[o + ck], g.travel_max);
    y_out[2 * r + 1] = pose_y(y0, touch_l[o + cf], touch_r[o + cf], S[o + cf], g.travel_max);
    flags_out[r] = (S[o + c0] >= g.travel_max ? 1 : 0) | (S[o + cf] >= g.travel_max ? 2 : 0) | ((bf == 0 || bf == g.X - 1) ? 4 : 0);
}

inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// workspace of a chunk of n pairs: [pairs | touch_l | touch_r | S | succ | ping | pong | kth]
struct Layout { size_t pairs, tl, tr, S, succ, ping, pong, kth, bytes; };
Layout layout(int64_t cells, int64_t n) {
    Layout L;
    const size_t d = align256(sizeof(double) * (size_t)(cells * n)), i = align256(sizeof(int32_t) * (size_t)(cells * n));
    L.pairs = 0;
    L.tl = align256(sizeof(int32_t) * 2 * (size_t)n);
    L.tr = L.tl + d;
    L.S = L.tr + d;
    L.succ = L.S + d;
    L.ping = L.succ + i;
    L.pong = L.ping + i;
    L.kth = L.pong + i;
    L.bytes = L.kth + i;
    return L;
}

constexpr int MAX_CHUNK = 65535;      // the pair index is the launch grid's y

int check_config(const DgdmSqueezeConfig *c, const char *fn) {
    DGDM_REQUIRE(c, DGDM_EINVAL, "%s: null config", fn);
    DGDM_REQUIRE(c->theta_cells >= 1 && c->x_cells >= 2, DGDM_EINVAL, "%s: grid of %d x %d cells (need theta_cells >= 1, x_cells >= 2)", fn,
                 c->theta_cells, c->x_cells);
    DGDM_REQUIRE((int64_t)c->theta_cells * c->x_cells <= (int64_t)1 << 30, DGDM_EINVAL, "%s: grid of %d x %d cells exceeds 2^30", fn,
                 c->theta_cells, c->x_cells);
    DGDM_REQUIRE(c->window >= 1 && c->window <= 64, DGDM_EINVAL, "%s: window %d (need 1 .. 64)", fn, c->window);
    DGDM_REQUIRE(c->closing_steps >= 0, DGDM_EINVAL, "%s: closing_steps %d is negative", fn, c->closing_steps);
    DGDM_REQUIRE(std::isfinite(c->x_half) && c->x_half > 0.0, DGDM_EINVAL, "%s: x_half %g (need finite, > 0)", fn, c->x_half);
    DGDM_REQUIRE(std::isfinite(c->travel_max), DGDM_EINVAL, "%s: travel_max %g is not finite", fn, c->travel_max);
    DGDM_REQUIRE(std::isfinite(c->finger_half_len) && c->finger_half_len > 0.0, DGDM_EINVAL, "%s: finger_half_len %g (need finite, > 0)", fn,
                 c->finger_half_len);
    return DGDM_OK;
}

}  // namespace
}  // namespace dgdm

using namespace dgdm;

extern "C" int64_t dgdm_squeeze_workspace_bytes(const DgdmSqueezeConfig *cfg, int chunk_pairs) {
    if (check_config(cfg, "dgdm_squeeze_workspace_bytes")) return DGDM_EINVAL;
    DGDM_REQUIRE(chunk_pairs >= 1 && chunk_pairs <= MAX_CHUNK, DGDM_EINVAL, "dgdm_squeeze_workspace_bytes: %d pairs per chunk (need 1 .. %d)",
                 chunk_pairs, MAX_CHUNK);
    return (int64_t)layout((int64_t)cfg->theta_cells * cfg->x_cells, chunk_pairs).bytes;
}

extern "C" int dgdm_squeeze_map(const DgdmSqueezeConfig *cfg, const double *surfaces_dev, int n_fingers, int num_points,
                                const double *objects_dev, int n_objects, int num_vertices, const int32_t *pairs_host, int n_pairs,
                                const double *rot_dev, const double *starts_dev, int n_starts, int32_t *cells_dev, double *y_dev,
                                int32_t *flags_dev, double *table_s_dev, double *touch_l_dev, double *touch_r_dev, int32_t *succ_dev,
                                void *workspace_dev, int64_t workspace_bytes, void *stream) {
    const char *fn = "dgdm_squeeze_map";
    int rc = check_config(cfg, fn);
    if (rc) return rc;
    DGDM_REQUIRE(surfaces_dev && objects_dev && pairs_host && rot_dev && workspace_dev, DGDM_EINVAL, "%s: null argument", fn);
    DGDM_REQUIRE(n_fingers >= 1 && n_objects >= 1 && n_pairs >= 1, DGDM_EINVAL, "%s: %d fingers, %d objects, %d pairs (need >= 1 each)", fn,
                 n_fingers, n_objects, n_pairs);
    DGDM_REQUIRE(num_points >= 2 && num_points <= MAX_SURFACE, DGDM_EINVAL, "%s: %d surface samples (need 2 .. %d)", fn, num_points, MAX_SURFACE);
    DGDM_REQUIRE(num_vertices >= 3 && num_vertices <= MAX_VERTS, DGDM_EINVAL, "%s: %d vertices (need 3 .. %d)", fn, num_vertices, MAX_VERTS);
    DGDM_REQUIRE(n_starts >= 0, DGDM_EINVAL, "%s: %d starts", fn, n_starts);
    DGDM_REQUIRE(n_starts == 0 || (starts_dev && cells_dev && y_dev && flags_dev), DGDM_EINVAL, "%s: %d starts need starts_dev and the three outputs",
                 fn, n_starts);
    for (int p = 0; p < n_pairs; ++p)
        DGDM_REQUIRE(pairs_host[2 * p] >= 0 && pairs_host[2 * p] < n_fingers && pairs_host[2 * p + 1] >= 0 && pairs_host[2 * p + 1] < n_objects,
                     DGDM_EINVAL, "%s: pair %d = (finger %d, object %d) outside %d fingers x %d objects", fn, p, pairs_host[2 * p],
                     pairs_host[2 * p + 1], n_fingers, n_objects);
    const int64_t cells = (int64_t)cfg->theta_cells * cfg->x_cells;
    DGDM_REQUIRE(workspace_bytes >= (int64_t)layout(cells, 1).bytes, DGDM_EINVAL,
                 "%s: workspace of %lld bytes holds no pair, one needs %lld (dgdm_squeeze_workspace_bytes)", fn, (long long)workspace_bytes,
                 (long long)layout(cells, 1).bytes);
    int64_t chunk = std::min<int64_t>(std::min<int64_t>(n_pairs, MAX_CHUNK), workspace_bytes / (int64_t)layout(cells, 1).bytes + 1);
    while (chunk > 1 && (int64_t)layout(cells, chunk).bytes > workspace_bytes) --chunk;

    Grid g;
    g.T = cfg->theta_cells;
    g.X = cfg->x_cells;
    g.R = cfg->window;
    g.m = num_points;
    g.nv = num_vertices;
    g.x_half = cfg->x_half;
    g.dx = 2.0 * cfg->x_half / (double)(cfg->x_cells - 1);
    g.hl = cfg->finger_half_len;
    g.h = 2.0 * cfg->finger_half_len / (double)(num_points - 1);
    g.travel_max = cfg->travel_max;
    int rounds = 0;
    while (((int64_t)1 << rounds) < cells) ++rounds;                     // ceil(log2(cells)): no path is longer than cells - 1 steps
    const bool k_settles = rounds < 31 && (int64_t)cfg->closing_steps >= ((int64_t)1 << rounds);

    const Layout L = layout(cells, chunk);
    uint8_t *ws = static_cast<uint8_t *>(workspace_dev);
    int32_t *pairs = reinterpret_cast<int32_t *>(ws + L.pairs);
    double *tl = reinterpret_cast<double *>(ws + L.tl), *tr = reinterpret_cast<double *>(ws + L.tr), *S = reinterpret_cast<double *>(ws + L.S);
    int32_t *succ = reinterpret_cast<int32_t *>(ws + L.succ), *kth = reinterpret_cast<int32_t *>(ws + L.kth);
    int32_t *buf[2] = {reinterpret_cast<int32_t *>(ws + L.ping), reinterpret_cast<int32_t *>(ws + L.pong)};
    hipStream_t s = (hipStream_t)stream;
    const size_t lds = sizeof(double) * (size_t)(2 * g.m + 2 * g.nv);
    const unsigned cb = (unsigned)((cells + 255) / 256);
    for (int64_t p0 = 0; p0 < n_pairs; p0 += chunk) {
        const unsigned n = (unsigned)std::min<int64_t>(chunk, n_pairs - p0);
        DGDM_HIP_CHECK(hipMemcpyAsync(pairs, pairs_host + 2 * p0, sizeof(int32_t) * 2 * n, hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(table_kernel, dim3((unsigned)g.T, n), dim3(TABLE_THREADS), lds, s, g, surfaces_dev, objects_dev, pairs, rot_dev, tl, tr, S);
        DGDM_HIP_CHECK(hipGetLastError());
        hipLaunchKernelGGL(successor_kernel, dim3(cb, n), dim3(256), 0, s, g, S, succ);
        DGDM_HIP_CHECK(hipGetLastError());
        hipLaunchKernelGGL(iota_kernel, dim3(cb, n), dim3(256), 0, s, (int)cells, kth);
        DGDM_HIP_CHECK(hipGetLastError());
        const int32_t *power = succ;
        for (int r = 0; r < rounds; ++r) {
            if (!k_settles && ((cfg->closing_steps >> r) & 1)) {
                hipLaunchKernelGGL(apply_kernel, dim3(cb, n), dim3(256), 0, s, (int)cells, power, kth);
                DGDM_HIP_CHECK(hipGetLastError());
            }
            hipLaunchKernelGGL(square_kernel, dim3(cb, n), dim3(256), 0, s, (int)cells, power, buf[r & 1]);
            DGDM_HIP_CHECK(hipGetLastError());
            power = buf[r & 1];
        }
        const int32_t *fix = power;                                      // succ^(2^rounds): every path has ended
        const int32_t *closed = k_settles ? fix : kth;
        if (n_starts > 0) {
            hipLaunchKernelGGL(lookup_kernel, dim3((unsigned)((n_starts + 255) / 256), n), dim3(256), 0, s, g, starts_dev, n_starts, tl, tr, S, closed,
                               fix, (int)p0, cells_dev, y_dev, flags_dev);
            DGDM_HIP_CHECK(hipGetLastError());
        }
        const size_t off = (size_t)p0 * cells, cnt = (size_t)n * cells;
        if (table_s_dev) DGDM_HIP_CHECK(hipMemcpyAsync(table_s_dev + off, S, sizeof(double) * cnt, hipMemcpyDeviceToDevice, s));
        if (touch_l_dev) DGDM_HIP_CHECK(hipMemcpyAsync(touch_l_dev + off, tl, sizeof(double) * cnt, hipMemcpyDeviceToDevice, s));
        if (touch_r_dev) DGDM_HIP_CHECK(hipMemcpyAsync(touch_r_dev + off, tr, sizeof(double) * cnt, hipMemcpyDeviceToDevice, s));
        if (succ_dev) DGDM_HIP_CHECK(hipMemcpyAsync(succ_dev + off, succ, sizeof(int32_t) * cnt, hipMemcpyDeviceToDevice, s));
    }
    DGDM_HIP_CHECK(hipStreamSynchronize(s));        // the pair list's host buffer belongs to the caller
    return DGDM_OK;
}

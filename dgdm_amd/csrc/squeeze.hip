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
// dgdm_squeeze_map_friction (include/dgdm_hip.h "squeeze simulator with Coulomb friction"; tests/squeeze_friction_oracle.py is its CPU
// oracle) runs the same launches with table_kernel<true>, which also fills the chunk's jam table: a jammed cell is its own successor
// (successor_kernel) and raises the flags 8 / 16 (lookup_kernel).  table_kernel<false> is dgdm_squeeze_map's kernel, instruction for
// instruction what it was before the template.
// dgdm_squeeze_map_3d (3-D fingers: the same contract on the horizontal planes of the finger grid, include/dgdm_hip.h "squeeze
// simulator, 3-D fingers") runs the same chunk loop (run_chunks) with table3d_kernel in table_kernel's place; dgdm_squeeze_slice cuts
// the object meshes into the per-level segment lists it reads.  Their kernels are described where they stand, below.
// dgdm_squeeze_map_3d_friction (include/dgdm_hip.h "squeeze simulator, 3-D fingers, with Coulomb friction"; tests/squeeze3d_friction_oracle.py
// is its CPU oracle) is dgdm_squeeze_map_3d with table3d_kernel<true>, which also fills the chunk's jam table by a 3-D antipodal test on
// the two contacts' points and normals; dgdm_squeeze_slice_normals is the slicer that also emits the crossing triangles' normals it reads.
// table3d_kernel<false> is dgdm_squeeze_map_3d's kernel, instruction for instruction what it was before the template.
// Host side: a map entry checks the sizes of its own inputs, then check_map_args checks what all three take alike (config, shared
// pointers, counts, starts and outputs, pair range, a workspace of at least one pair), then the entry checks what its own arrays hold.
// run_chunks alone decides how many pairs a workspace holds and where a chunk's tables lie; the 3-D entry's extra block (gx, level
// offsets) is the workspace's first bytes, so its place does not depend on the chunk size.  workspace_bytes_of is the one sum behind the
// three *_workspace_bytes entries.
// dgdm_squeeze_label (include/dgdm_hip.h "squeeze-simulator labels") is a fourth map entry behind the same front end: it hands run_chunks a
// consumer, which reduces each chunk's tables to condition rows where lookup_kernel would write per-start outputs, and fixes the chunk at
// whole fingers, since a row is made of all of a finger's pairs.
// dgdm_squeeze_label_3d (include/dgdm_hip.h "squeeze-simulator labels, 3-D fingers") is the fifth: the label entry's consumer behind the 3-D
// entry's inputs, both entries' checks (label_front, check_slices), and table3d_fingers_kernel for the chunk's tables, which shares the
// finger-independent work of table3d_kernel among a block of fingers and gives that kernel's tables bit for bit.
// dgdm_squeeze_values_3d (include/dgdm_hip.h "squeeze objective of 3-D fingers") is the sixth: groups of consecutive fingers on one object
// each, table3d_fingers_kernel over the groups for the chunk's tables, and values3d_pair_kernel as the consumer, which sums the objective
// per pair from the tables where lookup_kernel and squeeze_values_kernel would go through cells and y; chunks are whole groups.
// This file is compiled with -ffp-contract=off (build.py): no operation of the contract is fused.
#include "common.h"
#include <cmath>
#include <type_traits>

namespace dgdm {
namespace {

constexpr int TABLE_THREADS = 256;
constexpr int MAX_SURFACE = 1024, MAX_VERTS = 1024;     // (2 m + 2 nv) doubles of LDS: 32 KB at the limits
constexpr double TWO_PI = 6.283185307179586;

struct Grid {
    int T, X, R, m, nv;
    double x_half, dx, hl, h, travel_max;
};

// The contact `code` of one jaw (UPPER: the upper one), rebuilt after the walk by the walk's own operations in the walk's own order, so
// that every bit is the candidate's: its point c on the object and its unnormalised normal n from the jaw into the object (the header's
// table).  sF: that jaw's surface; code in 0 .. nv + nv m - 1.
template <bool UPPER>
__device__ __forceinline__ void contact_of(const Grid &g, const double *sF, const double *sRx, const double *sRy, double xg, int code, double &cx,
                                           double &cy, double &nx, double &ny) {
    if (code < g.nv) {                                                     // set A: vertex `code` on the segment j, j + 1
        const double px = sRx[code] + xg;
        const double t = (px + g.hl) / g.h;
        const int j = (int)fmin(floor(t), (double)(g.m - 2));
        const double d = sF[j + 1] - sF[j];
        cx = px;
        cy = sRy[code];
        nx = UPPER ? d : -d;
        ny = UPPER ? -g.h : g.h;
    } else {                                                               // set B: finger sample j under the edge (i, i + 1)
        const int r = code - g.nv, i = r / g.m, j = r - i * g.m, i1 = i + 1 == g.nv ? 0 : i + 1;
        const double px = sRx[i] + xg, py = sRy[i], qx = sRx[i1] + xg, qy = sRy[i1];
        const double ex = qx - px, ey = qy - py;
        const double slope = ey / ex;
        const double uj = -g.hl + (double)j * g.h;
        cx = uj;
        cy = py + (uj - px) * slope;
        const bool flip = (ex > 0.0) == UPPER;                             // lower: (-ey, ex) if ex > 0, else (ey, -ex); upper: its negative
        nx = flip ? ey : -ey;
        ny = flip ? -ex : ex;
    }
}

// touch_l / touch_r / S [pairs][T][X] of this chunk.  Grid: (T, pairs) workgroups.  FRICTION (dgdm_squeeze_map_friction): each lane also
// keeps, per jaw, the code of the first candidate to attain the least gap - two ints beside the two minima, one compare and one select per
// candidate - and after the walk rebuilds the two contacts from their codes (contact_of) and evaluates the jam test once; jam
// [pairs][T][X], contact [pairs][T][X][2] or null.  The false instantiation reads none of the last three arguments.
template <bool FRICTION>
__global__ __launch_bounds__(TABLE_THREADS) void table_kernel(Grid g, const double *surfaces, const double *objects, const int32_t *pairs,
                                                              const double *rot, double *touch_l, double *touch_r, double *S, double mu,
                                                              int32_t *jam, int32_t *contact) {
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
        [[maybe_unused]] int kl = -1, ku = -1;                             // FRICTION: the two contacts' codes
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
                if constexpr (FRICTION) {                                  // the first candidate to attain the least gap: strictly less only
                    kl = py - lp < gl ? i : kl;
                    ku = up - py < gu ? i : ku;
                }
                gl = fmin(gl, py - lp);
                gu = fmin(gu, up - py);
            }
            if (px != qx) {                                                // set B: the finger samples under the edge P -> Q
                const double j0 = fmax(ceil(fmin(t, tq)), 0.0);
                const double j1 = fmin(floor(fmax(t, tq)), jB);
                if (j0 <= j1) {                                            // both in 0 .. m - 1 then (false for a NaN)
                    const double slope = (qy - py) / (qx - px);
                    const int je = (int)j1;
                    [[maybe_unused]] const int kb = g.nv + i * g.m;        // FRICTION: the code of (edge i, sample 0)
                    for (int j = (int)j0; j <= je; ++j) {
                        const double uj = -hl + (double)j * h;
                        const double ye = py + (uj - px) * slope;
                        if constexpr (FRICTION) {
                            kl = ye - sL[j] < gl ? kb + j : kl;
                            ku = sU[j] - ye < gu ? kb + j : ku;
                        }
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
        if constexpr (FRICTION) {
            const double Sc = (gl + gu) / 2.0;
            int jm = 0;
            if (kl >= 0 && ku >= 0) {
                double clx, cly, nlx, nly, crx, cry, nrx, nry;
                contact_of<false>(g, sL, sRx, sRy, xg, kl, clx, cly, nlx, nly);
                contact_of<true>(g, sU, sRx, sRy, xg, ku, crx, cry, nrx, nry);
                const double ddx = crx - clx, ddy = cry - cly;
                const double dot_l = nlx * ddx + nly * ddy, crs_l = nlx * ddy - nly * ddx;
                const double dot_u = -(nrx * ddx + nry * ddy), crs_u = nrx * ddy - nry * ddx;
                jm = (mu > 0.0 && Sc < g.travel_max && dot_l > 0.0 && dot_u > 0.0 && fabs(crs_l) <= mu * dot_l && fabs(crs_u) <= mu * dot_u) ? 1 : 0;
            }
            jam[o] = jm;
            if (contact) {
                contact[2 * o] = kl;
                contact[2 * o + 1] = ku;
            }
        }
    }
}

// succ [pairs][cells]: the neighbour with the greatest S, visited in ascending (|db|, |da|, da, db), replaced on strictly greater only.
// jam [pairs][cells] or null (frictionless): a jammed cell is its own successor.
__global__ void successor_kernel(Grid g, const double *S, const int32_t *jam, int32_t *succ) {
    const int cells = g.T * g.X;
    const int cell = blockIdx.x * blockDim.x + threadIdx.x;
    if (cell >= cells) return;
    const double *Sp = S + (int64_t)blockIdx.y * cells;
    const int a = cell / g.X, b = cell - a * g.X;
    double best = Sp[cell];
    int arg = cell;
    const bool jammed = jam && jam[(int64_t)blockIdx.y * cells + cell] != 0;
    if (!(best >= g.travel_max) && !jammed) {
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

// The cell a start (theta0, x0) snaps to: the nearest, halves up, theta modulo 2 pi, x clamped; a non-finite start lands on cell 0.
__device__ __forceinline__ int snap_cell(const Grid &g, double th, double x0) {
    const double dth = TWO_PI / (double)g.T;
    const double q = floor(th / dth + 0.5);
    const double v = q - (double)g.T * floor(q / (double)g.T);
    const int a = (v >= 0.0 && v < (double)g.T) ? (int)v : 0;
    double w = floor((x0 + g.x_half) / g.dx + 0.5);
    if (!(w >= 0.0)) w = 0.0;
    if (!(w <= (double)(g.X - 1))) w = (double)(g.X - 1);
    return a * g.X + (int)w;
}

// Per (pair, start): cells (start, closed, settled), y (closed, settled), flags.  `pair0`: the chunk's first pair in the outputs.
// jam [pairs][cells] or null (frictionless): flags 8 (the start cell is jammed) and 16 (the settled cell is).
__global__ void lookup_kernel(Grid g, const double *starts, int n_starts, const double *touch_l, const double *touch_r, const double *S,
                              const int32_t *jam, const int32_t *kth, const int32_t *fix, int pair0, int32_t *cells_out, double *y_out,
                              int32_t *flags_out) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= n_starts) return;
    const int cells = g.T * g.X;
    const int64_t o = (int64_t)blockIdx.y * cells;
    const double th = starts[3 * n], x0 = starts[3 * n + 1], y0 = starts[3 * n + 2];
    const int c0 = snap_cell(g, th, x0);
    const int ck = kth[o + c0], cf = fix[o + c0];
    const int bf = cf % g.X;
    const int64_t r = (int64_t)(pair0 + blockIdx.y) * n_starts + n;
    cells_out[3 * r] = c0;
    cells_out[3 * r + 1] = ck;
    cells_out[3 * r + 2] = cf;
    y_out[2 * r] = pose_y(y0, touch_l[o + ck], touch_r[o + ck], S[o + ck], g.travel_max);
    y_out[2 * r + 1] = pose_y(y0, touch_l[o + cf], touch_r[o + cf], S[o + cf], g.travel_max);
    int fl = (S[o + c0] >= g.travel_max ? 1 : 0) | (S[o + cf] >= g.travel_max ? 2 : 0) | ((bf == 0 || bf == g.X - 1) ? 4 : 0);
    if (jam) fl |= (jam[o + c0] ? 8 : 0) | (jam[o + cf] ? 16 : 0);
    flags_out[r] = fl;
}

// The objective's value of every pair from its map (include/dgdm_hip.h, dgdm_squeeze_objective_values): one wave per pair, every lane its
// own starts in ascending order, an xor butterfly across the wave, lane 0 stores - the fixed shape of resample.hip's
// objective_values_kernel, the same bits run to run.  The cells are only taken apart, never used as an index.
struct ValueGrid {
    int T, X, n_starts, B;
    double dth, dx, std0, std1, std2;
};

__global__ __launch_bounds__(64) void squeeze_values_kernel(ValueGrid g, const int32_t *__restrict__ cells, const double *__restrict__ y,
                                                            const double *__restrict__ starts, const DgdmObjective *__restrict__ obj,
                                                            const float *__restrict__ rowcoef, double *__restrict__ values) {
    const int lane = threadIdx.x;
    const int64_t p = blockIdx.x;
    const int64_t group = p / g.B;
    const int b = (int)(p - group * g.B);
    const DgdmObjective o = obj[group];
    double lin[3], quad[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) { lin[j] = (double)o.lin[j]; quad[j] = (double)o.quad[j]; }
    double v = 0.0;
    for (int n = lane; n < g.n_starts; n += 64) {
        const int64_t r = p * g.n_starts + n;
        const int c0 = cells[3 * r], c1 = cells[3 * r + 1];
        const int a0 = c0 / g.X, b0 = c0 % g.X, a1 = c1 / g.X, b1 = c1 % g.X;
        int64_t da = (int64_t)a1 - a0;
        if (2 * da > g.T) da -= g.T;                                      // squeeze.fold's strict rule: +-T / 2 stays
        if (2 * da < -(int64_t)g.T) da += g.T;
        const double d0 = ((double)da * g.dth) / g.std0;
        const double d1 = ((double)(b1 - b0) * g.dx) / g.std1;
        const double d2 = (y[2 * r] - starts[3 * n + 2]) / g.std2;
        double t = ((lin[0] * d0 + quad[0] * (d0 * d0)) + (lin[1] * d1 + quad[1] * (d1 * d1))) + (lin[2] * d2 + quad[2] * (d2 * d2));
        if (o.use_rowcoef == 1) t += (double)rowcoef[(group * g.n_starts + n) * g.B + b] * d0;
        v += t;
    }
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) v += __shfl_xor(v, s);
    if (lane == 0) values[p] = v;
}

// dgdm_squeeze_values_3d's consumer (include/dgdm_hip.h "squeeze objective of 3-D fingers"): squeeze_values_kernel's sum straight from a
// chunk's tables, in lookup_kernel's place - no per-start row is stored.  Grid: one workgroup of one wave per pair of the chunk, `pair0`
// the chunk's first pair of the call (a whole group's), `obj` the chunk's groups.  Per start lookup_kernel's steps (the snap, the closed
// cell, pose_y at it), then squeeze_values_kernel's expressions in its order.  The cells are taken apart only after closed[] has been
// read at the snapped index; they index nothing else.
__global__ __launch_bounds__(64) void values3d_pair_kernel(Grid g, ValueGrid vg, const double *__restrict__ starts, const double *__restrict__ touch_l,
                                                           const double *__restrict__ touch_r, const double *__restrict__ S,
                                                           const int32_t *__restrict__ closed, const DgdmObjective *__restrict__ obj,
                                                           const float *__restrict__ rowcoef, int64_t pair0, double *__restrict__ values) {
    const int lane = threadIdx.x;
    const int64_t tab = (int64_t)blockIdx.x * g.T * g.X;
    const int64_t p = pair0 + blockIdx.x;
    const int64_t group = p / vg.B;
    const int b = (int)(p - group * vg.B);
    const DgdmObjective o = obj[group - pair0 / vg.B];
    double lin[3], quad[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) { lin[j] = (double)o.lin[j]; quad[j] = (double)o.quad[j]; }
    double v = 0.0;
    for (int n = lane; n < vg.n_starts; n += 64) {
        const double th = starts[3 * (int64_t)n], x0 = starts[3 * (int64_t)n + 1], y0 = starts[3 * (int64_t)n + 2];
        const int c0 = snap_cell(g, th, x0);
        const int c1 = closed[tab + c0];
        const double yc = pose_y(y0, touch_l[tab + c1], touch_r[tab + c1], S[tab + c1], g.travel_max);
        const int a0 = c0 / vg.X, b0 = c0 % vg.X, a1 = c1 / vg.X, b1 = c1 % vg.X;
        int64_t da = (int64_t)a1 - a0;
        if (2 * da > vg.T) da -= vg.T;                                    // squeeze.fold's strict rule: +-T / 2 stays
        if (2 * da < -(int64_t)vg.T) da += vg.T;
        const double d0 = ((double)da * vg.dth) / vg.std0;
        const double d1 = ((double)(b1 - b0) * vg.dx) / vg.std1;
        const double d2 = (yc - y0) / vg.std2;
        double t = ((lin[0] * d0 + quad[0] * (d0 * d0)) + (lin[1] * d1 + quad[1] * (d1 * d1))) + (lin[2] * d2 + quad[2] * (d2 * d2));
        if (o.use_rowcoef == 1) t += (double)rowcoef[(group * vg.n_starts + n) * vg.B + b] * d0;
        v += t;
    }
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) v += __shfl_xor(v, s);
    if (lane == 0) values[p] = v;
}

// ---------------------------------------------------------------------------------------------------------------- labels: condition rows
// dgdm_squeeze_label (include/dgdm_hip.h "squeeze-simulator labels"; tests/squeeze_label_oracle.py is the CPU oracle): the chunk loop's
// consumer in lookup_kernel's place.  Per chunk, straight from the chunk's tables, no per-start row is stored:
//   label_pair_kernel   one wave per pair: every lane its own starts in ascending order (snap, the two maps, y - lookup_kernel's steps),
//                       class counts, flag counts and the sums in registers, an xor butterfly across the wave, lane 0 stores the pair's
//                       partials - squeeze_values_kernel's shape, the same bits run to run;
//   label_rows_kernel   one thread per finger: its pairs' partials, objects ascending, to the row's blocks.
struct LabelGrid {
    int n_tally, n_settle, M, layout, column_offset, object_stride;
    int64_t row_stride;
    double dth, thr[3], std[3], pos_norm;
};

struct PairPart {
    double sum[4];          // d0, |d0|, d1, d2 over the tally starts
    double settle[3];       // cos, sin, r over the settle starts
    int32_t cls[6];         // e0 class 0 / 2, e1 class 0 / 2, e2 class 0 / 2
    int32_t flag[3];        // tally starts with flag 1, 2, 4
    int32_t left, bad, pad; // settle starts out of range; any non-finite y_settled
};

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) v += __shfl_xor(v, s);
    return v;
}

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) v += __shfl_xor(v, s);
    return v;
}

// Grid: one workgroup of one wave per pair of the chunk.  closed / fix [pairs][cells]: the one-closing and the settled map.
__global__ __launch_bounds__(64) void label_pair_kernel(Grid g, LabelGrid lg, const double *__restrict__ starts, const double *__restrict__ rot,
                                                        const double *__restrict__ touch_l, const double *__restrict__ touch_r,
                                                        const double *__restrict__ S, const int32_t *__restrict__ closed,
                                                        const int32_t *__restrict__ fix, PairPart *__restrict__ part) {
    const int lane = threadIdx.x;
    const int64_t o = (int64_t)blockIdx.x * g.T * g.X;
    double sum[4] = {0.0, 0.0, 0.0, 0.0};
    int cls[6] = {0, 0, 0, 0, 0, 0}, flag[3] = {0, 0, 0};
    for (int n = lane; n < lg.n_tally; n += 64) {
        const double th = starts[3 * (int64_t)n], x0 = starts[3 * (int64_t)n + 1], y0 = starts[3 * (int64_t)n + 2];
        const int c0 = snap_cell(g, th, x0);
        const int ck = closed[o + c0], cf = fix[o + c0];
        const int a0 = c0 / g.X, b0 = c0 % g.X, a1 = ck / g.X, b1 = ck % g.X, bf = cf % g.X;
        int64_t da = (int64_t)a1 - a0;
        if (2 * da > g.T) da -= g.T;                                      // squeeze.fold's strict rule: +-T / 2 stays
        if (2 * da < -(int64_t)g.T) da += g.T;
        double e[3];
        e[0] = (double)da * lg.dth;
        e[1] = (double)(b1 - b0) * g.dx;
        e[2] = pose_y(y0, touch_l[o + ck], touch_r[o + ck], S[o + ck], g.travel_max) - y0;
#pragma unroll
        for (int j = 0; j < 3; ++j) {                                      // class 2 first: squeeze_metric's where(d > thr, 2, where(d < -thr, 0, 1))
            const bool hi = e[j] > lg.thr[j];
            cls[2 * j] += (!hi && e[j] < -lg.thr[j]) ? 1 : 0;
            cls[2 * j + 1] += hi ? 1 : 0;
        }
        const double d0 = e[0] / lg.std[0];
        sum[0] += d0;
        sum[1] += fabs(d0);
        sum[2] += e[1] / lg.std[1];
        sum[3] += e[2] / lg.std[2];
        flag[0] += S[o + c0] >= g.travel_max ? 1 : 0;
        flag[1] += S[o + cf] >= g.travel_max ? 1 : 0;
        flag[2] += (bf == 0 || bf == g.X - 1) ? 1 : 0;
    }
    double settle[3] = {0.0, 0.0, 0.0};
    int left = 0, bad = 0;
    for (int q = lane; q < lg.n_settle; q += 64) {
        const int64_t n = (int64_t)lg.n_tally + q;
        const double th = starts[3 * n], x0 = starts[3 * n + 1], y0 = starts[3 * n + 2];
        const int cf = fix[o + snap_cell(g, th, x0)];
        const int as = cf / g.X, bs = cf % g.X;
        const double ys = pose_y(y0, touch_l[o + cf], touch_r[o + cf], S[o + cf], g.travel_max);
        const double xs = -g.x_half + (double)bs * g.dx;
        const double px = xs / lg.pos_norm, py = ys / lg.pos_norm;
        settle[0] += rot[2 * as];
        settle[1] += rot[2 * as + 1];
        settle[2] += sqrt(px * px + py * py);
        left += (bs == 0 || bs == g.X - 1 || fabs(px) > 1.0 || fabs(py) > 1.0) ? 1 : 0;
        bad |= isfinite(ys) ? 0 : 1;
    }
    PairPart r;
#pragma unroll
    for (int j = 0; j < 4; ++j) r.sum[j] = wave_sum(sum[j]);
#pragma unroll
    for (int j = 0; j < 3; ++j) r.settle[j] = wave_sum(settle[j]);
#pragma unroll
    for (int j = 0; j < 6; ++j) r.cls[j] = wave_sum(cls[j]);
#pragma unroll
    for (int j = 0; j < 3; ++j) r.flag[j] = wave_sum(flag[j]);
    r.left = wave_sum(left);
    r.bad = wave_sum(bad);
    r.pad = 0;
    if (lane == 0) part[blockIdx.x] = r;
}

// One thread per finger of the chunk (`finger0`: the chunk's first finger): its M pairs' partials to the row's blocks, and the flag counts.
__global__ void label_rows_kernel(LabelGrid lg, const PairPart *__restrict__ part, int n_fingers, int64_t finger0, float *__restrict__ rows,
                                  int32_t *__restrict__ counts) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= n_fingers) return;
    const PairPart *pp = part + (int64_t)f * lg.M;
    float *row = rows + (finger0 + f) * lg.row_stride + lg.column_offset;
    const int blocks = lg.layout == DGDM_LABEL_PER_OBJECT ? lg.M : 1, per = lg.layout == DGDM_LABEL_PER_OBJECT ? 1 : lg.M;
    const double G = (double)lg.n_settle, Mp = (double)per, nn = (double)((int64_t)per * lg.n_tally);
    for (int blk = 0; blk < blocks; ++blk) {
        float *dst = row + (int64_t)blk * lg.object_stride;                // MEAN: one block, blk = 0
        int64_t K[6] = {0, 0, 0, 0, 0, 0};
        double s[4] = {0.0, 0.0, 0.0, 0.0}, v[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
        for (int k = blk * per; k < (blk + 1) * per; ++k) {
            const PairPart &p = pp[k];
            for (int j = 0; j < 6; ++j) K[j] += p.cls[j];
            for (int j = 0; j < 4; ++j) s[j] += p.sum[j];
            if (lg.n_settle > 0) {
                double c = p.settle[0] / G, sn = p.settle[1] / G;
                double rho = sqrt(c * c + sn * sn), off = p.settle[2] / G;
                if (p.bad) rho = c = sn = off = NAN;
                v[0] += rho;
                v[1] += c;
                v[2] += sn;
                v[3] += off;
                v[4] += (double)p.left / G;
            }
        }
        for (int j = 0; j < 6; ++j) dst[j] = (float)((double)K[j] / nn);
        for (int j = 0; j < 4; ++j) dst[6 + j] = (float)(s[j] / nn);
        if (lg.n_settle > 0)
            for (int j = 0; j < 5; ++j) dst[DGDM_LABEL_TALLY_COLS + j] = (float)(v[j] / Mp);
    }
    if (counts) {
        int32_t c[3] = {0, 0, 0};
        for (int k = 0; k < lg.M; ++k)
            for (int j = 0; j < 3; ++j) c[j] += pp[k].flag[j];
        for (int j = 0; j < 3; ++j) counts[3 * (finger0 + f) + j] = c[j];
    }
}

inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// workspace of a chunk of n pairs: [pairs | touch_l | touch_r | S | succ | ping | pong | kth] and, with friction, [jam] behind them
struct Layout { size_t pairs, tl, tr, S, succ, ping, pong, kth, jam, bytes; };
Layout layout(int64_t cells, int64_t n, bool friction = false) {
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
    L.jam = L.kth + i;
    L.bytes = L.jam + (friction ? i : 0);
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

Grid grid_of(const DgdmSqueezeConfig *cfg) {
    Grid g = {};
    g.T = cfg->theta_cells;
    g.X = cfg->x_cells;
    g.R = cfg->window;
    g.x_half = cfg->x_half;
    g.dx = 2.0 * cfg->x_half / (double)(cfg->x_cells - 1);
    g.travel_max = cfg->travel_max;
    return g;
}

// The three *_workspace_bytes entries: a chunk of chunk_pairs pairs and the `extra` bytes the entry keeps in front of it.
int64_t workspace_bytes_of(const char *fn, const DgdmSqueezeConfig *cfg, int chunk_pairs, bool friction, size_t extra) {
    if (check_config(cfg, fn)) return DGDM_EINVAL;
    DGDM_REQUIRE(chunk_pairs >= 1 && chunk_pairs <= MAX_CHUNK, DGDM_EINVAL, "%s: %d pairs per chunk (need 1 .. %d)", fn, chunk_pairs, MAX_CHUNK);
    return (int64_t)(extra + layout((int64_t)cfg->theta_cells * cfg->x_cells, chunk_pairs, friction).bytes);
}

struct Outputs {
    int32_t *cells;
    double *y;
    int32_t *flags;
    double *S, *tl, *tr;
    int32_t *succ;
    int32_t *jam;       // friction only
};

// What every map entry checks alike, after the checks on its own inputs: the config, the pointers all entries take, the counts, the
// starts and their outputs, the pair range, and that the workspace holds the entry's `extra` bytes and one pair's chunk.  `own`: the
// entry's own pointers are all set.  `count_objects`: the 2-D entries name n_objects in the counts' message; the 3-D entry has checked
// it with its sizes.  `bytes_fn`: the entry that sizes this workspace, for the message.
int check_map_args(const char *fn, const DgdmSqueezeConfig *cfg, bool own, bool count_objects, int n_fingers, int n_objects,
                   const int32_t *pairs_host, int n_pairs, const double *starts_dev, int n_starts, const Outputs &out, const void *workspace_dev,
                   int64_t workspace_bytes, bool friction, size_t extra, const char *bytes_fn) {
    int rc = check_config(cfg, fn);
    if (rc) return rc;
    DGDM_REQUIRE(own && pairs_host && workspace_dev, DGDM_EINVAL, "%s: null argument", fn);
    if (count_objects)
        DGDM_REQUIRE(n_fingers >= 1 && n_objects >= 1 && n_pairs >= 1, DGDM_EINVAL, "%s: %d fingers, %d objects, %d pairs (need >= 1 each)", fn,
                     n_fingers, n_objects, n_pairs);
    else
        DGDM_REQUIRE(n_fingers >= 1 && n_pairs >= 1, DGDM_EINVAL, "%s: %d fingers, %d pairs (need >= 1 each)", fn, n_fingers, n_pairs);
    DGDM_REQUIRE(n_starts >= 0, DGDM_EINVAL, "%s: %d starts", fn, n_starts);
    DGDM_REQUIRE(n_starts == 0 || (starts_dev && out.cells && out.y && out.flags), DGDM_EINVAL, "%s: %d starts need starts_dev and the three outputs",
                 fn, n_starts);
    for (int p = 0; p < n_pairs; ++p)
        DGDM_REQUIRE(pairs_host[2 * p] >= 0 && pairs_host[2 * p] < n_fingers && pairs_host[2 * p + 1] >= 0 && pairs_host[2 * p + 1] < n_objects,
                     DGDM_EINVAL, "%s: pair %d = (finger %d, object %d) outside %d fingers x %d objects", fn, p, pairs_host[2 * p],
                     pairs_host[2 * p + 1], n_fingers, n_objects);
    const int64_t one = (int64_t)(extra + layout((int64_t)cfg->theta_cells * cfg->x_cells, 1, friction).bytes);
    DGDM_REQUIRE(workspace_bytes >= one, DGDM_EINVAL, "%s: workspace of %lld bytes holds no pair, one needs %lld (%s)", fn,
                 (long long)workspace_bytes, (long long)one, bytes_fn);
    return DGDM_OK;
}

// The chunk loop of all entries: as many pairs per chunk as the workspace's `bytes` hold (the caller has checked that one fits);
// `table(n, p0, pairs, tl, tr, S, jam, stream)` launches the entry's table kernel for the chunk's n pairs from pair p0 on, whose (finger,
// object) are at `pairs`.  `friction`: the chunk holds a jam table, which the table kernel fills and the successors and the flags read.
// `consume(n, p0, tl, tr, S, closed, fix, stream)`, optional: an entry's own reduction of the chunk, launched where lookup_kernel stands
// (which still runs when there are starts); an entry that passes one also passes `fixed`, the pairs per chunk it has sized its own
// buffers and the workspace for.  The map entries pass neither: their launches are what they were.
struct NoConsumer {};
template <class Table, class Consume = NoConsumer>
int run_chunks(const DgdmSqueezeConfig *cfg, const Grid &g, const int32_t *pairs_host, int n_pairs, const double *starts_dev, int n_starts,
               const Outputs &out, void *workspace_dev, int64_t bytes, hipStream_t s, bool friction, Table table, Consume consume = Consume(),
               int64_t fixed = 0) {
    const int64_t cells = (int64_t)g.T * g.X;
    int64_t chunk = std::min<int64_t>(std::min<int64_t>(n_pairs, MAX_CHUNK), bytes / (int64_t)layout(cells, 1, friction).bytes + 1);
    while (chunk > 1 && (int64_t)layout(cells, chunk, friction).bytes > bytes) --chunk;
    if (fixed > 0) chunk = std::min<int64_t>(n_pairs, fixed);
    int rounds = 0;
    while (((int64_t)1 << rounds) < cells) ++rounds;                     // ceil(log2(cells)): no path is longer than cells - 1 steps
    const bool k_settles = rounds < 31 && (int64_t)cfg->closing_steps >= ((int64_t)1 << rounds);

    const Layout L = layout(cells, chunk, friction);
    uint8_t *ws = static_cast<uint8_t *>(workspace_dev);
    int32_t *jam = friction ? reinterpret_cast<int32_t *>(ws + L.jam) : nullptr;
    int32_t *pairs = reinterpret_cast<int32_t *>(ws + L.pairs);
    double *tl = reinterpret_cast<double *>(ws + L.tl), *tr = reinterpret_cast<double *>(ws + L.tr), *S = reinterpret_cast<double *>(ws + L.S);
    int32_t *succ = reinterpret_cast<int32_t *>(ws + L.succ), *kth = reinterpret_cast<int32_t *>(ws + L.kth);
    int32_t *buf[2] = {reinterpret_cast<int32_t *>(ws + L.ping), reinterpret_cast<int32_t *>(ws + L.pong)};
    const unsigned cb = (unsigned)((cells + 255) / 256);
    for (int64_t p0 = 0; p0 < n_pairs; p0 += chunk) {
        const unsigned n = (unsigned)std::min<int64_t>(chunk, n_pairs - p0);
        DGDM_HIP_CHECK(hipMemcpyAsync(pairs, pairs_host + 2 * p0, sizeof(int32_t) * 2 * n, hipMemcpyHostToDevice, s));
        table(n, p0, pairs, tl, tr, S, jam, s);
        DGDM_HIP_CHECK(hipGetLastError());
        hipLaunchKernelGGL(successor_kernel, dim3(cb, n), dim3(256), 0, s, g, S, (const int32_t *)jam, succ);
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
            hipLaunchKernelGGL(lookup_kernel, dim3((unsigned)((n_starts + 255) / 256), n), dim3(256), 0, s, g, starts_dev, n_starts, tl, tr, S,
                               (const int32_t *)jam, closed, fix, (int)p0, out.cells, out.y, out.flags);
            DGDM_HIP_CHECK(hipGetLastError());
        }
        if constexpr (!std::is_same<Consume, NoConsumer>::value) {
            consume(n, p0, tl, tr, S, closed, fix, s);
            DGDM_HIP_CHECK(hipGetLastError());
        }
        const size_t off = (size_t)p0 * cells, cnt = (size_t)n * cells;
        if (out.S) DGDM_HIP_CHECK(hipMemcpyAsync(out.S + off, S, sizeof(double) * cnt, hipMemcpyDeviceToDevice, s));
        if (out.tl) DGDM_HIP_CHECK(hipMemcpyAsync(out.tl + off, tl, sizeof(double) * cnt, hipMemcpyDeviceToDevice, s));
        if (out.tr) DGDM_HIP_CHECK(hipMemcpyAsync(out.tr + off, tr, sizeof(double) * cnt, hipMemcpyDeviceToDevice, s));
        if (out.succ) DGDM_HIP_CHECK(hipMemcpyAsync(out.succ + off, succ, sizeof(int32_t) * cnt, hipMemcpyDeviceToDevice, s));
        if (jam && out.jam) DGDM_HIP_CHECK(hipMemcpyAsync(out.jam + off, jam, sizeof(int32_t) * cnt, hipMemcpyDeviceToDevice, s));
    }
    DGDM_HIP_CHECK(hipStreamSynchronize(s));        // the pair list's host buffer belongs to the caller
    return DGDM_OK;
}

// ---------------------------------------------------------------------------------------------------------------- 3-D: a sliced squeeze
// include/dgdm_hip.h "squeeze simulator, 3-D fingers"; tests/squeeze3d_oracle.py is the CPU oracle.
//   slice_kernel<false / true>  one workgroup per (level, object): the count pass and, after the host's scan of the n_objects x mv
//                       counts, the emit pass - a block scan of the crossing flags per 256 triangles keeps the triangle order;
//   table3d_kernel      one workgroup per (pair, theta), lanes on the x cells (table_kernel's layout): the pair's 2 mv mu surface doubles,
//                       gx and the object's level offsets staged in LDS once, the rotated segments in tiles of SEG_TILE; each lane
//                       carries its two minima in registers across tiles - no atomics, no cross-lane reduction.
// SEG_TILE = 1024 segments x 4 doubles = 32 KB: with the 16 KB of surfaces at the limits a workgroup stays under 50 KB, three per CU in
// the 160 KB of LDS; a larger tile saves two barriers per 1024 segments, which the ~100 float64 operations per segment and lane dwarf.
constexpr int SEG_TILE = 1024;
constexpr int MAX_MU = 128, MAX_MV = 512, MAX_SURFACE_3D = 1024, MAX_LEVELS = 1024;

struct Grid3 {
    int T, X, mu, mv;
    double x_half, dx;
};

template <bool EMIT>
__global__ __launch_bounds__(256) void slice_kernel(const double *verts, const int32_t *tris, const int64_t *vert_off, const int64_t *tri_off,
                                                    const double *gz, int mv, int32_t *counts, const int32_t *seg_off, double *segments,
                                                    double *normals) {
    __shared__ int sc[256];
    const int j = blockIdx.x, o = blockIdx.y, tid = threadIdx.x;
    const double z = gz[j];
    const double *V = verts + 3 * vert_off[o];
    const int32_t *F = tris + 3 * tri_off[o];
    const int nt = (int)(tri_off[o + 1] - tri_off[o]);
    int base = 0;                                                          // EMIT: segments of earlier rounds; else this thread's count
    for (int t0 = 0; t0 < nt; t0 += 256) {
        const int t = t0 + tid;
        int v[3] = {0, 0, 0};
        bool up[3] = {false, false, false};
        bool cross = false;
        if (t < nt) {
            for (int e = 0; e < 3; ++e) {
                v[e] = F[3 * t + e];
                up[e] = V[3 * v[e] + 2] >= z;
            }
            const int nup = (int)up[0] + (int)up[1] + (int)up[2];
            cross = nup != 0 && nup != 3;
        }
        if (!EMIT) {
            base += cross ? 1 : 0;
            continue;
        }
        sc[tid] = cross ? 1 : 0;                                           // inclusive scan of the flags: the triangle order is kept
        __syncthreads();
        for (int off = 1; off < 256; off <<= 1) {
            const int add = tid >= off ? sc[tid - off] : 0;
            __syncthreads();
            sc[tid] += add;
            __syncthreads();
        }
        const int incl = sc[tid], total = sc[255];
        __syncthreads();
        if (cross) {
            double pt[4];
            int n = 0;
            for (int e = 0; e < 3; ++e) {
                const int e1 = e == 2 ? 0 : e + 1;
                if (up[e] == up[e1]) continue;
                const double *D = V + 3 * (up[e] ? v[e1] : v[e]), *W = V + 3 * (up[e] ? v[e] : v[e1]);
                const double r = (z - D[2]) / (W[2] - D[2]);
                pt[n++] = D[0] + r * (W[0] - D[0]);
                pt[n++] = D[1] + r * (W[1] - D[1]);
            }
            double *dst = segments + 4 * ((int64_t)seg_off[o * (mv + 1) + j] + base + incl - 1);
            for (int q = 0; q < 4; ++q) dst[q] = pt[q];
            if (normals) {                                                 // dgdm_squeeze_slice_normals: N = (V1 - V0) x (V2 - V0), as the header writes it
                const double *V0 = V + 3 * v[0], *V1 = V + 3 * v[1], *V2 = V + 3 * v[2];
                const double ex = V1[0] - V0[0], ey = V1[1] - V0[1], ez = V1[2] - V0[2];
                const double fx = V2[0] - V0[0], fy = V2[1] - V0[1], fz = V2[2] - V0[2];
                double *nd = normals + 3 * ((int64_t)seg_off[o * (mv + 1) + j] + base + incl - 1);
                nd[0] = ey * fz - ez * fy;
                nd[1] = ez * fx - ex * fz;
                nd[2] = ex * fy - ey * fx;
            }
        }
        base += total;
    }
    if (!EMIT) {
        sc[tid] = base;
        __syncthreads();
        for (int off = 128; off > 0; off >>= 1) {
            if (tid < off) sc[tid] += sc[tid + off];
            __syncthreads();
        }
        if (tid == 0) counts[o * mv + j] = sc[0];
    }
}

// the greatest i with gx[i] <= x, -1 when there is none (or x is a NaN): comparisons only
__device__ __forceinline__ int last_le(const double *gx, int mu, double x) {
    int lo = -1, hi = mu;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (gx[mid] <= x) lo = mid; else hi = mid;
    }
    return lo;
}

// The contact `code` of one jaw (UPPER: the upper one) of a 3-D cell, rebuilt after the walk by the walk's own operations in the walk's own
// order (include/dgdm_hip.h "squeeze simulator, 3-D fingers, with Coulomb friction"): the winner's segment and, for set B, its triangle's
// normal are read from global memory and rotated again, so every bit is the candidate's.  sF: that jaw's surface [mv][mu] in LDS; sG, sOff:
// the abscissae and the object's level offsets in LDS; s0 = sOff[0]; code in 0 .. (segments of the object) (mu + 2) - 1.
template <bool UPPER>
__device__ __forceinline__ void contact3d_of(const Grid3 &g, const double *sF, const double *sG, const int32_t *sOff, const double *gz,
                                             const double *segments, const double *normals, int s0, double c, double s, double xg, int code,
                                             double &cx, double &cy, double &cz, double &nx, double &ny, double &nz) {
    const int mu = g.mu, w = mu + 2, si = code / w, k = code - si * w, t = s0 + si;
    int j = 0;
    while (t >= sOff[j + 1]) ++j;                                          // t < sOff[mv]: j stays below mv
    const double *sg = segments + 4 * (int64_t)t;
    const double ax = sg[0], ay = sg[1], bx = sg[2], by = sg[3];
    const double px = (c * ax - s * ay) + xg, py = s * ax + c * ay, qx = (c * bx - s * by) + xg, qy = s * bx + c * by;
    cz = gz[j];
    if (k < 2) {                                                           // set A: P or Q on the jaw's patch i, i + 1 of level j
        const double ex = k ? qx : px;
        const int i = max(min(last_le(sG, mu, ex), mu - 2), 0);
        const double g0 = sG[i], hx = sG[i + 1] - g0, f = (ex - g0) / hx;
        const double *Fj = sF + j * mu;
        const double dF = Fj[i + 1] - Fj[i];
        double hz = 1.0, sz = 0.0;                                         // mv = 1: no z slope
        if (g.mv > 1) {
            const int jm = max(j - 1, 0), jp = min(j + 1, g.mv - 1);
            const double *Fm = sF + jm * mu, *Fp = sF + jp * mu;
            const double m0 = Fm[i], p0 = Fp[i];
            const double fm = m0 + f * (Fm[i + 1] - m0), fp = p0 + f * (Fp[i + 1] - p0);
            hz = gz[jp] - gz[jm];
            sz = (fp - fm) * hx;
        }
        cx = ex;
        cy = k ? qy : py;
        nx = UPPER ? dF * hz : -dF * hz;
        ny = UPPER ? -(hx * hz) : hx * hz;
        nz = g.mv > 1 ? (UPPER ? sz : -sz) : 0.0;
    } else {                                                               // set B: abscissa k - 2 under the segment, the triangle's normal
        const int i = k - 2;
        const double slope = (qy - py) / (qx - px);
        const double *N = normals + 3 * (int64_t)t;
        const double rx = c * N[0] - s * N[1], ry = s * N[0] + c * N[1], rz = N[2];
        const bool flip = UPPER ? ry > 0.0 : ry < 0.0;                     // lower: n_y > 0, upper: n_y < 0, whatever the mesh's winding
        cx = sG[i];
        cy = py + (sG[i] - px) * slope;
        nx = flip ? -rx : rx;
        ny = flip ? -ry : ry;
        nz = flip ? -rz : rz;
    }
}

// touch_l / touch_r / S [pairs][T][X] of this chunk.  Grid: (T, pairs) workgroups.  FRICTION (dgdm_squeeze_map_3d_friction): each lane also
// keeps, per jaw, the code of the first candidate to attain the least gap - two ints beside the two minima, one compare and one select per
// candidate - and after the walk rebuilds the two contacts from their codes (contact3d_of) and evaluates the 3-D jam test once per cell;
// jam [pairs][T][X], contact [pairs][T][X][2] or null.  The false instantiation reads none of the last six arguments and is
// dgdm_squeeze_map_3d's kernel, instruction for instruction what it was before the template.
template <bool FRICTION>
__global__ __launch_bounds__(TABLE_THREADS) void table3d_kernel(Grid3 g, const double *surfaces, const double *gx, const double *segments,
                                                                const int32_t *seg_offsets, const int32_t *pairs, const double *rot,
                                                                double *touch_l, double *touch_r, double *S, const double *gz,
                                                                const double *normals, double fmu, double travel_max, int32_t *jam,
                                                                int32_t *contact) {
    extern __shared__ double lds[];
    const int ms = g.mv * g.mu, mu = g.mu, tid = threadIdx.x;
    double *sL = lds, *sU = lds + ms, *sG = lds + 2 * ms, *sSeg = sG + mu;
    int32_t *sOff = reinterpret_cast<int32_t *>(sSeg + 4 * SEG_TILE);
    const int a = blockIdx.x, p = blockIdx.y;
    const double *sf = surfaces + (int64_t)pairs[2 * p] * 2 * ms;
    const int32_t *off = seg_offsets + (int64_t)pairs[2 * p + 1] * (g.mv + 1);
    const double c = rot[2 * a], s = rot[2 * a + 1];
    for (int i = tid; i < 2 * ms; i += TABLE_THREADS) sL[i] = sf[i];       // L then U, as the pair holds them
    for (int i = tid; i < mu; i += TABLE_THREADS) sG[i] = gx[i];
    for (int i = tid; i <= g.mv; i += TABLE_THREADS) sOff[i] = off[i];
    __syncthreads();
    const int s0 = sOff[0], s1 = sOff[g.mv];
    const double glast = sG[mu - 1], inf = INFINITY;
    for (int b0 = 0; b0 < g.X; b0 += TABLE_THREADS) {
        const int b = b0 + tid;
        const double xg = -g.x_half + (double)b * g.dx;
        double gl = inf, gu = inf;
        [[maybe_unused]] int kl = -1, ku = -1;                             // FRICTION: the two contacts' codes
        int j = 0;                                                         // the level of the segment at hand: they come level-sorted
        for (int t0 = s0; t0 < s1; t0 += SEG_TILE) {
            const int n = min(SEG_TILE, s1 - t0);
            __syncthreads();                                               // the tile before has been read by every lane
            for (int k = tid; k < n; k += TABLE_THREADS) {
                const double *sg = segments + 4 * (int64_t)(t0 + k);
                const double ax = sg[0], ay = sg[1], bx = sg[2], by = sg[3];
                sSeg[4 * k] = c * ax - s * ay;
                sSeg[4 * k + 1] = s * ax + c * ay;
                sSeg[4 * k + 2] = c * bx - s * by;
                sSeg[4 * k + 3] = s * bx + c * by;
            }
            __syncthreads();
            if (b >= g.X) continue;
            for (int k = 0; k < n; ++k) {
                while (t0 + k >= sOff[j + 1]) ++j;                         // t0 + k < s1 = sOff[mv]: j stays below mv
                const double *Lj = sL + j * mu, *Uj = sU + j * mu;
                const double px = sSeg[4 * k] + xg, py = sSeg[4 * k + 1], qx = sSeg[4 * k + 2] + xg, qy = sSeg[4 * k + 3];
                // one search per endpoint serves set A and, gx being ascending, both ends of set B's range of abscissae
                const int ip = last_le(sG, mu, px), iq = last_le(sG, mu, qx);
                [[maybe_unused]] const int kc = (t0 + k - s0) * (mu + 2);  // FRICTION: the code of (this segment, P)
                if (ip >= 0 && px <= glast) {                              // set A: P against the interpolated profiles
                    const int i = min(ip, mu - 2);
                    const double g0 = sG[i], f = (px - g0) / (sG[i + 1] - g0);
                    const double l0 = Lj[i], u0 = Uj[i];
                    const double lp = l0 + f * (Lj[i + 1] - l0);
                    const double up = u0 + f * (Uj[i + 1] - u0);
                    if constexpr (FRICTION) {                              // the first candidate to attain the least gap: strictly less only
                        kl = py - lp < gl ? kc : kl;
                        ku = up - py < gu ? kc : ku;
                    }
                    gl = fmin(gl, py - lp);
                    gu = fmin(gu, up - py);
                }
                if (iq >= 0 && qx <= glast) {                              // set A: Q
                    const int i = min(iq, mu - 2);
                    const double g0 = sG[i], f = (qx - g0) / (sG[i + 1] - g0);
                    const double l0 = Lj[i], u0 = Uj[i];
                    const double lp = l0 + f * (Lj[i + 1] - l0);
                    const double up = u0 + f * (Uj[i + 1] - u0);
                    if constexpr (FRICTION) {
                        kl = qy - lp < gl ? kc + 1 : kl;
                        ku = up - qy < gu ? kc + 1 : ku;
                    }
                    gl = fmin(gl, qy - lp);
                    gu = fmin(gu, up - qy);
                }
                if (px < qx || qx < px) {                                  // set B: the abscissae under the segment (false for a NaN)
                    const bool fwd = px < qx;
                    const int ilo = fwd ? ip : iq, ihi = fwd ? iq : ip;
                    const double xlo = fwd ? px : qx;
                    const int i0 = (ilo >= 0 && sG[ilo] == xlo) ? ilo : ilo + 1;
                    if (i0 <= ihi) {
                        const double slope = (qy - py) / (qx - px);
                        for (int i = i0; i <= ihi; ++i) {
                            const double ye = py + (sG[i] - px) * slope;
                            if constexpr (FRICTION) {
                                kl = ye - Lj[i] < gl ? kc + 2 + i : kl;
                                ku = Uj[i] - ye < gu ? kc + 2 + i : ku;
                            }
                            gl = fmin(gl, ye - Lj[i]);
                            gu = fmin(gu, Uj[i] - ye);
                        }
                    }
                }
            }
        }
        if (b < g.X) {
            const int64_t o = ((int64_t)p * g.T + a) * g.X + b;
            touch_l[o] = gl;
            touch_r[o] = gu;
            S[o] = (gl + gu) / 2.0;
            if constexpr (FRICTION) {
                const double Sc = (gl + gu) / 2.0;
                int jm = 0;
                if (kl >= 0 && ku >= 0) {
                    double clx, cly, clz, nlx, nly, nlz, cux, cuy, cuz, nux, nuy, nuz;
                    contact3d_of<false>(g, sL, sG, sOff, gz, segments, normals, s0, c, s, xg, kl, clx, cly, clz, nlx, nly, nlz);
                    contact3d_of<true>(g, sU, sG, sOff, gz, segments, normals, s0, c, s, xg, ku, cux, cuy, cuz, nux, nuy, nuz);
                    const double ddx = cux - clx, ddy = cuy - cly, ddz = cuz - clz;
                    const double a_l = nlx * ddx + nly * ddy + nlz * ddz;
                    const double wlx = nly * ddz - nlz * ddy, wly = nlz * ddx - nlx * ddz, wlz = nlx * ddy - nly * ddx;
                    const double q_l = wlx * wlx + wly * wly + wlz * wlz;
                    const double a_u = -(nux * ddx + nuy * ddy + nuz * ddz);
                    const double wux = nuy * ddz - nuz * ddy, wuy = nuz * ddx - nux * ddz, wuz = nux * ddy - nuy * ddx;
                    const double q_u = wux * wux + wuy * wuy + wuz * wuz;
                    const double ml = fmu * a_l, mr = fmu * a_u;
                    jm = (fmu > 0.0 && Sc < travel_max && a_l > 0.0 && a_u > 0.0 && q_l <= ml * ml && q_u <= mr * mr) ? 1 : 0;
                }
                jam[o] = jm;
                if (contact) {
                    contact[2 * o] = kl;
                    contact[2 * o + 1] = ku;
                }
            }
        }
    }
}

// table3d_kernel's tables for a chunk of whole fingers x M objects (dgdm_squeeze_label_3d; pair f * M + k of the chunk is its finger f on
// object k, as that entry lists them), with what does not read the finger done once per block of FB fingers.  Grid: (T, M, blocks of FB
// fingers) workgroups, lanes on the x cells.  Per (segment, lane) the two searches, set A's i and f, set B's range and slope and each
// abscissa's ye are evaluated once; the loops over the block's fingers hold only the contract's operations on that finger's profiles, and
// each finger's two minima stay in registers.  Every finger sees its candidates in table3d_kernel's order (P, Q, then the abscissae
// ascending, segment by segment), so its three tables are table3d_kernel's bit for bit.  A tail block runs the same loops under the
// uniform bound nfb < FB and reads no finger past the chunk.  dgdm_squeeze_values_3d launches the same body over groups of `batch`
// consecutive fingers on one object each, pair k * batch + b of the chunk (the strides ks, fs at the kernel, below).
// LDS: the current level's profiles of the block only, restaged when the level changes - the segments come level-sorted and the level
// loop is uniform across the workgroup, so the barriers in it are legal.  sP[i][f] = (L_j[i], U_j[i]) of finger f as one 16-byte pair,
// entries LABEL3_ENTRY = 2 FB + 2 doubles apart: a lane's reads of the entries i and i + 1 of all FB fingers are 2 FB ds_read_b128 of one
// contiguous run, and the 16 bytes of padding put the entries i .. i + 15, which one ds_read_b128 service group of 16 (non-contiguous)
// lanes may span, on 16 distinct quarters of the 64 banks (entry stride 144 B at FB = 8: i * 36 mod 64 is a different multiple of 4 for
// 16 consecutive i; lanes on one entry read one address, a broadcast).  Bytes, FB = 8: mu * 144 (profiles) + 8 mu (gx) + 16384 (a tile
// of FSEG_TILE = 512 rotated segments) + 4 (mv + 1) (level offsets) = 3600 + 200 + 16384 + 104 = 20288 at 25 x 25; at the limits
// mu = 128 (mv = 8): 18432 + 1024 + 16384 + 36 = 35876, and mu = 2 (mv = 512): 288 + 16 + 16384 + 2052 = 18740.  Whole surfaces of the
// block would be 16 KB per finger at the limits, 128 KB for FB = 8: one workgroup per CU.
constexpr int LABEL3_FB = 8, FSEG_TILE = 512;
constexpr int LABEL3_ENTRY = 2 * LABEL3_FB + 2;

template <int FB, bool TAIL>
__device__ __forceinline__ void table3d_fingers_body(const Grid3 &g, int ks, int fs, int nfb, const double *surfaces, const double *gx,
                                                     const double *segments, const int32_t *seg_offsets, const int32_t *pairs, const double *rot,
                                                     double *touch_l, double *touch_r, double *S, double *lds) {
    constexpr int ENTRY = 2 * FB + 2;
    const int ms = g.mv * g.mu, mu = g.mu, tid = threadIdx.x;
    double *sP = lds, *sG = lds + mu * ENTRY, *sSeg = sG + mu;
    int32_t *sOff = reinterpret_cast<int32_t *>(sSeg + 4 * FSEG_TILE);
    const int a = blockIdx.x, k = blockIdx.y;
    const int64_t pr0 = (int64_t)blockIdx.z * FB * fs + (int64_t)k * ks;   // the block's first pair of the chunk; finger f's is fs f further on
    const double *sf = surfaces + (int64_t)pairs[2 * pr0] * 2 * ms;        // the chunk's fingers are consecutive: finger f's is 2 ms f further on
    const int32_t *off = seg_offsets + (int64_t)pairs[2 * pr0 + 1] * (g.mv + 1);
    const double c = rot[2 * a], s = rot[2 * a + 1];
    for (int i = tid; i < mu; i += TABLE_THREADS) sG[i] = gx[i];
    for (int i = tid; i <= g.mv; i += TABLE_THREADS) sOff[i] = off[i];
    __syncthreads();
    const double glast = sG[mu - 1], inf = INFINITY;
    for (int b0 = 0; b0 < g.X; b0 += TABLE_THREADS) {
        const int b = b0 + tid;
        const double xg = -g.x_half + (double)b * g.dx;
        double gl[FB], gu[FB];
#pragma unroll
        for (int f = 0; f < FB; ++f) gl[f] = gu[f] = inf;
        for (int j = 0; j < g.mv; ++j) {
            const int s0 = sOff[j], s1 = sOff[j + 1];
            if (s0 == s1) continue;                                        // uniform: an empty level stages nothing
            __syncthreads();                                               // the level and the tile before have been read by every lane
            for (int e = tid; e < nfb * 2 * mu; e += TABLE_THREADS) {      // L_j then U_j of finger f, as the finger holds them
                const int f = e / (2 * mu), r = e - f * 2 * mu, u = r >= mu ? 1 : 0, i = r - u * mu;
                sP[i * ENTRY + 2 * f + u] = sf[(int64_t)f * 2 * ms + (int64_t)u * ms + j * mu + i];
            }
            for (int t0 = s0; t0 < s1; t0 += FSEG_TILE) {
                const int n = min(FSEG_TILE, s1 - t0);
                if (t0 > s0) __syncthreads();
                for (int q = tid; q < n; q += TABLE_THREADS) {
                    const double *sg = segments + 4 * (int64_t)(t0 + q);
                    const double ax = sg[0], ay = sg[1], bx = sg[2], by = sg[3];
                    sSeg[4 * q] = c * ax - s * ay;
                    sSeg[4 * q + 1] = s * ax + c * ay;
                    sSeg[4 * q + 2] = c * bx - s * by;
                    sSeg[4 * q + 3] = s * bx + c * by;
                }
                __syncthreads();
                if (b >= g.X) continue;
                for (int q = 0; q < n; ++q) {
                    const double px = sSeg[4 * q] + xg, py = sSeg[4 * q + 1], qx = sSeg[4 * q + 2] + xg, qy = sSeg[4 * q + 3];
                    const int ip = last_le(sG, mu, px), iq = last_le(sG, mu, qx);
#pragma unroll
                    for (int end = 0; end < 2; ++end) {                    // set A: P, then Q
                        const int ie = end ? iq : ip;
                        const double ex = end ? qx : px, ey = end ? qy : py;
                        if (ie >= 0 && ex <= glast) {
                            const int i = min(ie, mu - 2);
                            const double g0 = sG[i], fr = (ex - g0) / (sG[i + 1] - g0);
                            const double2 *e0 = reinterpret_cast<const double2 *>(sP + i * ENTRY), *e1 = e0 + ENTRY / 2;
#pragma unroll
                            for (int f = 0; f < FB; ++f) {
                                if (TAIL && f >= nfb) break;
                                const double2 v0 = e0[f], v1 = e1[f];
                                const double lp = v0.x + fr * (v1.x - v0.x);
                                const double up = v0.y + fr * (v1.y - v0.y);
                                gl[f] = fmin(gl[f], ey - lp);
                                gu[f] = fmin(gu[f], up - ey);
                            }
                        }
                    }
                    if (px < qx || qx < px) {                              // set B
                        const bool fwd = px < qx;
                        const int ilo = fwd ? ip : iq, ihi = fwd ? iq : ip;
                        const double xlo = fwd ? px : qx;
                        const int i0 = (ilo >= 0 && sG[ilo] == xlo) ? ilo : ilo + 1;
                        if (i0 <= ihi) {
                            const double slope = (qy - py) / (qx - px);
                            for (int i = i0; i <= ihi; ++i) {
                                const double ye = py + (sG[i] - px) * slope;
                                const double2 *e0 = reinterpret_cast<const double2 *>(sP + i * ENTRY);
#pragma unroll
                                for (int f = 0; f < FB; ++f) {
                                    if (TAIL && f >= nfb) break;
                                    const double2 v = e0[f];
                                    gl[f] = fmin(gl[f], ye - v.x);
                                    gu[f] = fmin(gu[f], v.y - ye);
                                }
                            }
                        }
                    }
                }
            }
        }
        if (b < g.X) {
#pragma unroll
            for (int f = 0; f < FB; ++f) {
                if (f >= nfb) break;
                const int64_t o = ((pr0 + (int64_t)f * fs) * g.T + a) * g.X + b;
                touch_l[o] = gl[f];
                touch_r[o] = gu[f];
                S[o] = (gl[f] + gu[f]) / 2.0;
            }
        }
    }
}

// `nf`: the fingers that meet one object (the grid's y) - the label's: the chunk's; the groups form's: a group's.  (ks, fs): the pair
// strides of the grid's y and of a finger - the label's finger-major chunk is (1, M), dgdm_squeeze_values_3d's group-major one (batch, 1);
// either way a block's fingers are consecutive in `surfaces` and the loops are the same.  The branch on a full block is uniform across
// the grid's z.
__global__ __launch_bounds__(TABLE_THREADS) void table3d_fingers_kernel(Grid3 g, int ks, int fs, int nf, const double *surfaces, const double *gx,
                                                                        const double *segments, const int32_t *seg_offsets, const int32_t *pairs,
                                                                        const double *rot, double *touch_l, double *touch_r, double *S) {
    extern __shared__ __align__(16) double lds16[];
    const int nfb = min(LABEL3_FB, nf - (int)blockIdx.z * LABEL3_FB);
    if (nfb == LABEL3_FB)
        table3d_fingers_body<LABEL3_FB, false>(g, ks, fs, nfb, surfaces, gx, segments, seg_offsets, pairs, rot, touch_l, touch_r, S, lds16);
    else
        table3d_fingers_body<LABEL3_FB, true>(g, ks, fs, nfb, surfaces, gx, segments, seg_offsets, pairs, rot, touch_l, touch_r, S, lds16);
}

// the 3-D entry's workspace: gx [mu] and the level offsets [n_objects][mv + 1] in front, wherever the chunks are cut, then the chunk's
// layout (run_chunks gets what lies behind the block)
struct Extra3 { size_t gx, off, gz, bytes; };
Extra3 extra3(int mu, int mv, int n_objects, bool with_gz = false) {      // with_gz (the friction entry): the levels gz [mv] behind the two
    Extra3 e;
    e.gx = 0;
    e.off = align256(sizeof(double) * (size_t)mu);
    e.gz = e.off + align256(sizeof(int32_t) * (size_t)n_objects * (size_t)(mv + 1));
    e.bytes = e.gz + (with_gz ? align256(sizeof(double) * (size_t)mv) : 0);
    return e;
}

int check_sizes_3d(int mu, int mv, int n_objects, const char *fn) {
    DGDM_REQUIRE(mu >= 2 && mu <= MAX_MU, DGDM_EINVAL, "%s: %d abscissae (need 2 .. %d)", fn, mu, MAX_MU);
    DGDM_REQUIRE(mv >= 1 && mv <= MAX_MV, DGDM_EINVAL, "%s: %d levels (need 1 .. %d)", fn, mv, MAX_MV);
    DGDM_REQUIRE(mu * mv <= MAX_SURFACE_3D, DGDM_EINVAL, "%s: %d x %d surface samples (need at most %d)", fn, mv, mu, MAX_SURFACE_3D);
    DGDM_REQUIRE(n_objects >= 1 && n_objects <= (1 << 20), DGDM_EINVAL, "%s: %d objects (need 1 .. 2^20)", fn, n_objects);
    return DGDM_OK;
}

int check_ascending(const double *v, int n, const char *what, const char *fn) {
    for (int i = 0; i < n; ++i) {
        DGDM_REQUIRE(std::isfinite(v[i]), DGDM_EINVAL, "%s: %s[%d] = %g is not finite", fn, what, i, v[i]);
        DGDM_REQUIRE(i == 0 || v[i] > v[i - 1], DGDM_EINVAL, "%s: %s is not strictly ascending at %d (%g after %g)", fn, what, i, v[i], v[i - 1]);
    }
    return DGDM_OK;
}

}  // namespace
}  // namespace dgdm

using namespace dgdm;

extern "C" int64_t dgdm_squeeze_workspace_bytes(const DgdmSqueezeConfig *cfg, int chunk_pairs) {
    return workspace_bytes_of("dgdm_squeeze_workspace_bytes", cfg, chunk_pairs, false, 0);
}

// table_kernel<friction> for the n pairs of a chunk (g.m, g.nv, g.hl and g.h set).  Without friction mu, jam and contact are unused.
static void launch_table(bool friction, const Grid &g, const double *surfaces_dev, const double *objects_dev, const int32_t *pairs,
                         const double *rot_dev, double *tl, double *tr, double *S, double mu, int32_t *jam, int32_t *contact, unsigned n,
                         hipStream_t s) {
    const size_t lds = sizeof(double) * (size_t)(2 * g.m + 2 * g.nv);
    if (friction)
        hipLaunchKernelGGL(table_kernel<true>, dim3((unsigned)g.T, n), dim3(TABLE_THREADS), lds, s, g, surfaces_dev, objects_dev, pairs, rot_dev, tl, tr,
                           S, mu, jam, contact);
    else
        hipLaunchKernelGGL(table_kernel<false>, dim3((unsigned)g.T, n), dim3(TABLE_THREADS), lds, s, g, surfaces_dev, objects_dev, pairs, rot_dev, tl, tr,
                           S, 0.0, (int32_t *)nullptr, (int32_t *)nullptr);
}

// What the 2-D entries refuse of their own sizes, and the grid made of them once the config has been checked.
static int check_sizes_2d(const char *fn, int num_points, int num_vertices) {
    DGDM_REQUIRE(num_points >= 2 && num_points <= MAX_SURFACE, DGDM_EINVAL, "%s: %d surface samples (need 2 .. %d)", fn, num_points, MAX_SURFACE);
    DGDM_REQUIRE(num_vertices >= 3 && num_vertices <= MAX_VERTS, DGDM_EINVAL, "%s: %d vertices (need 3 .. %d)", fn, num_vertices, MAX_VERTS);
    return DGDM_OK;
}

static Grid grid_2d(const DgdmSqueezeConfig *cfg, int num_points, int num_vertices) {
    Grid g = grid_of(cfg);
    g.m = num_points;
    g.nv = num_vertices;
    g.hl = cfg->finger_half_len;
    g.h = 2.0 * cfg->finger_half_len / (double)(num_points - 1);
    return g;
}

// The body of dgdm_squeeze_map (friction = false: mu, jam_dev and contact_dev unused) and dgdm_squeeze_map_friction.
static int squeeze_map_common(const char *fn, bool friction, double mu, const DgdmSqueezeConfig *cfg, const double *surfaces_dev, int n_fingers,
                              int num_points, const double *objects_dev, int n_objects, int num_vertices, const int32_t *pairs_host, int n_pairs,
                              const double *rot_dev, const double *starts_dev, int n_starts, int32_t *cells_dev, double *y_dev, int32_t *flags_dev,
                              double *table_s_dev, double *touch_l_dev, double *touch_r_dev, int32_t *succ_dev, int32_t *jam_dev,
                              int32_t *contact_dev, void *workspace_dev, int64_t workspace_bytes, void *stream) {
    DGDM_REQUIRE(!friction || (std::isfinite(mu) && mu >= 0.0), DGDM_EINVAL, "%s: friction coefficient %g (need finite, >= 0)", fn, mu);
    int rc = check_sizes_2d(fn, num_points, num_vertices);
    if (rc) return rc;
    Outputs out = {cells_dev, y_dev, flags_dev, table_s_dev, touch_l_dev, touch_r_dev, succ_dev, jam_dev};
    if ((rc = check_map_args(fn, cfg, surfaces_dev && objects_dev && rot_dev, true, n_fingers, n_objects, pairs_host, n_pairs, starts_dev, n_starts, out,
                             workspace_dev, workspace_bytes, friction, 0,
                             friction ? "dgdm_squeeze_friction_workspace_bytes" : "dgdm_squeeze_workspace_bytes")))
        return rc;
    const int64_t cells = (int64_t)cfg->theta_cells * cfg->x_cells;
    const Grid g = grid_2d(cfg, num_points, num_vertices);
    return run_chunks(cfg, g, pairs_host, n_pairs, starts_dev, n_starts, out, workspace_dev, workspace_bytes, (hipStream_t)stream, friction,
                      [&](unsigned n, int64_t p0, const int32_t *pairs, double *tl, double *tr, double *S, int32_t *jam, hipStream_t s) {
                          launch_table(friction, g, surfaces_dev, objects_dev, pairs, rot_dev, tl, tr, S, mu, jam,
                                       contact_dev ? contact_dev + 2 * p0 * cells : nullptr, n, s);
                      });
}

extern "C" int dgdm_squeeze_map(const DgdmSqueezeConfig *cfg, const double *surfaces_dev, int n_fingers, int num_points,
                                const double *objects_dev, int n_objects, int num_vertices, const int32_t *pairs_host, int n_pairs,
                                const double *rot_dev, const double *starts_dev, int n_starts, int32_t *cells_dev, double *y_dev,
                                int32_t *flags_dev, double *table_s_dev, double *touch_l_dev, double *touch_r_dev, int32_t *succ_dev,
                                void *workspace_dev, int64_t workspace_bytes, void *stream) {
    return squeeze_map_common("dgdm_squeeze_map", false, 0.0, cfg, surfaces_dev, n_fingers, num_points, objects_dev, n_objects, num_vertices,
                              pairs_host, n_pairs, rot_dev, starts_dev, n_starts, cells_dev, y_dev, flags_dev, table_s_dev, touch_l_dev, touch_r_dev,
                              succ_dev, nullptr, nullptr, workspace_dev, workspace_bytes, stream);
}

extern "C" int64_t dgdm_squeeze_friction_workspace_bytes(const DgdmSqueezeConfig *cfg, int chunk_pairs) {
    return workspace_bytes_of("dgdm_squeeze_friction_workspace_bytes", cfg, chunk_pairs, true, 0);
}

extern "C" int dgdm_squeeze_map_friction(const DgdmSqueezeConfig *cfg, const double *surfaces_dev, int n_fingers, int num_points,
                                         const double *objects_dev, int n_objects, int num_vertices, const int32_t *pairs_host, int n_pairs,
                                         const double *rot_dev, const double *starts_dev, int n_starts, int32_t *cells_dev, double *y_dev,
                                         int32_t *flags_dev, double *table_s_dev, double *touch_l_dev, double *touch_r_dev, int32_t *succ_dev,
                                         void *workspace_dev, int64_t workspace_bytes, void *stream, double mu, int32_t *jam_dev,
                                         int32_t *contact_dev) {
    return squeeze_map_common("dgdm_squeeze_map_friction", true, mu, cfg, surfaces_dev, n_fingers, num_points, objects_dev, n_objects,
                              num_vertices, pairs_host, n_pairs, rot_dev, starts_dev, n_starts, cells_dev, y_dev, flags_dev, table_s_dev,
                              touch_l_dev, touch_r_dev, succ_dev, jam_dev, contact_dev, workspace_dev, workspace_bytes, stream);
}

// The label entry's partial sums lie in front of the chunk's tables, one PairPart per pair of the chunk.
static size_t label_extra(int64_t chunk_pairs) { return align256(sizeof(PairPart) * (size_t)chunk_pairs); }

static int check_label_objects(const char *fn, int n_objects) {
    DGDM_REQUIRE(n_objects >= 1 && n_objects <= MAX_CHUNK, DGDM_EINVAL, "%s: %d objects per finger (need 1 .. %d)", fn, n_objects, MAX_CHUNK);
    return DGDM_OK;
}

extern "C" int64_t dgdm_squeeze_label_workspace_bytes(const DgdmSqueezeConfig *cfg, int chunk_fingers, int n_objects, int friction) {
    const char *fn = "dgdm_squeeze_label_workspace_bytes";
    if (check_label_objects(fn, n_objects)) return DGDM_EINVAL;
    DGDM_REQUIRE(chunk_fingers >= 1 && (int64_t)chunk_fingers * n_objects <= MAX_CHUNK, DGDM_EINVAL,
                 "%s: %d fingers of %d objects per chunk (need >= 1 finger, at most %d pairs)", fn, chunk_fingers, n_objects, MAX_CHUNK);
    const int chunk_pairs = chunk_fingers * n_objects;
    return workspace_bytes_of(fn, cfg, chunk_pairs, friction != 0, label_extra(chunk_pairs));
}

// What both label entries check alike of the arguments they share, after the sizes of their own inputs and before check_map_args: on
// DGDM_OK `lg` holds all but dth (the config is checked later) and `pairs` the finger-major list, pair f * M + k = (f, objects_host[k]).
static int label_front(const char *fn, int n_fingers, int n_bank, const int32_t *objects_host, int n_objects, const double *starts_dev, int n_tally,
                       int n_settle, const double threshold[3], const double score_std[3], double pos_norm, int row_layout, const float *rows_dev,
                       int64_t row_stride, int column_offset, int object_stride, LabelGrid &lg, std::vector<int32_t> &pairs) {
    DGDM_REQUIRE(objects_host && threshold && score_std && rows_dev && starts_dev, DGDM_EINVAL, "%s: null argument", fn);
    DGDM_REQUIRE(n_fingers >= 1 && n_bank >= 1, DGDM_EINVAL, "%s: %d fingers, a bank of %d objects (need >= 1 each)", fn, n_fingers, n_bank);
    DGDM_REQUIRE((int64_t)n_fingers * n_objects <= INT32_MAX, DGDM_EINVAL, "%s: %d fingers x %d objects exceed 2^31 - 1 pairs", fn, n_fingers, n_objects);
    for (int k = 0; k < n_objects; ++k)
        DGDM_REQUIRE(objects_host[k] >= 0 && objects_host[k] < n_bank, DGDM_EINVAL, "%s: object %d = %d outside the bank of %d", fn, k, objects_host[k],
                     n_bank);
    DGDM_REQUIRE(n_tally >= 1 && n_settle >= 0 && (int64_t)n_tally + n_settle <= INT32_MAX, DGDM_EINVAL,
                 "%s: %d tally and %d settle starts (need n_tally >= 1, n_settle >= 0)", fn, n_tally, n_settle);
    DGDM_REQUIRE((int64_t)n_objects * n_tally <= INT32_MAX, DGDM_EINVAL, "%s: %d objects x %d tally starts exceed 2^31 - 1", fn, n_objects, n_tally);
    for (int j = 0; j < 3; ++j) {
        DGDM_REQUIRE(std::isfinite(score_std[j]) && score_std[j] > 0.0, DGDM_EINVAL, "%s: score_std[%d] = %g (need finite, > 0)", fn, j, score_std[j]);
        DGDM_REQUIRE(std::isfinite(threshold[j]) && threshold[j] >= 0.0, DGDM_EINVAL, "%s: threshold[%d] = %g (need finite, >= 0)", fn, j, threshold[j]);
    }
    DGDM_REQUIRE(std::isfinite(pos_norm) && pos_norm > 0.0, DGDM_EINVAL, "%s: pos_norm %g (need finite, > 0)", fn, pos_norm);
    DGDM_REQUIRE(row_layout == DGDM_LABEL_MEAN || row_layout == DGDM_LABEL_PER_OBJECT, DGDM_EINVAL, "%s: unknown layout %d", fn, row_layout);
    const int cols = DGDM_LABEL_TALLY_COLS + (n_settle > 0 ? DGDM_LABEL_SETTLED_COLS : 0);
    const bool per_object = row_layout == DGDM_LABEL_PER_OBJECT;
    DGDM_REQUIRE(column_offset >= 0, DGDM_EINVAL, "%s: column_offset %d is negative", fn, column_offset);
    DGDM_REQUIRE(!per_object || object_stride >= cols, DGDM_EINVAL, "%s: object_stride %d holds no block of %d columns", fn, object_stride, cols);
    const int64_t width = (int64_t)column_offset + (per_object ? (int64_t)(n_objects - 1) * object_stride : 0) + cols;
    DGDM_REQUIRE(row_stride >= width, DGDM_EINVAL, "%s: row_stride %lld holds no row of %lld floats", fn, (long long)row_stride, (long long)width);
    lg = {};
    lg.n_tally = n_tally;
    lg.n_settle = n_settle;
    lg.M = n_objects;
    lg.layout = row_layout;
    lg.column_offset = column_offset;
    lg.object_stride = per_object ? object_stride : 0;
    lg.row_stride = row_stride;
    for (int j = 0; j < 3; ++j) { lg.thr[j] = threshold[j]; lg.std[j] = score_std[j]; }
    lg.pos_norm = pos_norm;
    pairs.resize((size_t)2 * n_fingers * n_objects);
    for (int f = 0; f < n_fingers; ++f)
        for (int k = 0; k < n_objects; ++k) {
            pairs[2 * ((size_t)f * n_objects + k)] = f;
            pairs[2 * ((size_t)f * n_objects + k) + 1] = objects_host[k];
        }
    return DGDM_OK;
}

// Whole fingers only: the most fingers whose partials and tables a workspace holds behind the `front` bytes the entry keeps ahead of them.
static int label_chunk_fingers(const char *fn, const char *bytes_fn, const DgdmSqueezeConfig *cfg, int n_fingers, int n_objects, bool friction,
                               int64_t workspace_bytes, size_t front, int64_t &fingers) {
    const int64_t cells = (int64_t)cfg->theta_cells * cfg->x_cells;
    auto need = [&](int64_t f) { return (int64_t)(front + label_extra(f * n_objects) + layout(cells, f * n_objects, friction).bytes); };
    DGDM_REQUIRE(workspace_bytes >= need(1), DGDM_EINVAL, "%s: workspace of %lld bytes holds no finger of %d objects, one needs %lld (%s)", fn,
                 (long long)workspace_bytes, n_objects, (long long)need(1), bytes_fn);
    fingers = 1;
    int64_t over = std::min<int64_t>(n_fingers, MAX_CHUNK / n_objects) + 1;                   // need() does not fall: bisect [fingers, over)
    while (over - fingers > 1) {
        const int64_t mid = fingers + (over - fingers) / 2;
        if (need(mid) <= workspace_bytes) fingers = mid; else over = mid;
    }
    return DGDM_OK;
}

// The label entries' consumer: a chunk's n pairs (whole fingers, the first one pair p0's) from its tables to rows and counts.
static void launch_label(const Grid &g, const LabelGrid &lg, unsigned n, int64_t p0, const double *starts_dev, const double *rot_dev, const double *tl,
                         const double *tr, const double *S, const int32_t *closed, const int32_t *fix, PairPart *part, float *rows_dev,
                         int32_t *counts_dev, hipStream_t s) {
    const int nf = (int)(n / (unsigned)lg.M);
    hipLaunchKernelGGL(label_pair_kernel, dim3(n), dim3(64), 0, s, g, lg, starts_dev, rot_dev, tl, tr, S, closed, fix, part);
    hipLaunchKernelGGL(label_rows_kernel, dim3((unsigned)((nf + 63) / 64)), dim3(64), 0, s, lg, (const PairPart *)part, nf, p0 / lg.M, rows_dev,
                       counts_dev);
}

extern "C" int dgdm_squeeze_label(const DgdmSqueezeConfig *cfg, const double *surfaces_dev, int n_fingers, int num_points, const double *bank_dev,
                                  int n_bank, int num_vertices, const int32_t *objects_host, int n_objects, const double *rot_dev,
                                  const double *starts_dev, int n_tally, int n_settle, double mu, const double threshold[3],
                                  const double score_std[3], double pos_norm, int row_layout, float *rows_dev, int64_t row_stride, int column_offset,
                                  int object_stride, int32_t *counts_dev, void *workspace_dev, int64_t workspace_bytes, void *stream) {
    const char *fn = "dgdm_squeeze_label";
    const char *bytes_fn = "dgdm_squeeze_label_workspace_bytes";
    DGDM_REQUIRE(std::isfinite(mu) && mu >= 0.0, DGDM_EINVAL, "%s: friction coefficient %g (need finite, >= 0)", fn, mu);
    int rc = check_sizes_2d(fn, num_points, num_vertices);
    if (rc || (rc = check_label_objects(fn, n_objects))) return rc;
    LabelGrid lg;
    std::vector<int32_t> pairs;
    if ((rc = label_front(fn, n_fingers, n_bank, objects_host, n_objects, starts_dev, n_tally, n_settle, threshold, score_std, pos_norm, row_layout,
                          rows_dev, row_stride, column_offset, object_stride, lg, pairs)))
        return rc;
    const bool friction = mu > 0.0;
    const int n_pairs = n_fingers * n_objects;
    const Outputs out = {};
    if ((rc = check_map_args(fn, cfg, surfaces_dev && bank_dev && rot_dev, true, n_fingers, n_bank, pairs.data(), n_pairs, nullptr, 0, out, workspace_dev,
                             workspace_bytes, friction, label_extra(1), bytes_fn)))
        return rc;
    int64_t fingers;
    if ((rc = label_chunk_fingers(fn, bytes_fn, cfg, n_fingers, n_objects, friction, workspace_bytes, 0, fingers))) return rc;
    const int64_t cap = fingers * n_objects;
    const size_t extra = label_extra(cap);

    const Grid g = grid_2d(cfg, num_points, num_vertices);
    lg.dth = TWO_PI / (double)g.T;
    uint8_t *ws = static_cast<uint8_t *>(workspace_dev);                  // the partials in front, the chunk's tables behind them
    PairPart *part = reinterpret_cast<PairPart *>(ws);
    return run_chunks(
        cfg, g, pairs.data(), n_pairs, nullptr, 0, out, ws + extra, workspace_bytes - (int64_t)extra, (hipStream_t)stream, friction,
        [&](unsigned n, int64_t, const int32_t *prs, double *tl, double *tr, double *S, int32_t *jam, hipStream_t s) {
            launch_table(friction, g, surfaces_dev, bank_dev, prs, rot_dev, tl, tr, S, mu, jam, nullptr, n, s);
        },
        [&](unsigned n, int64_t p0, const double *tl, const double *tr, const double *S, const int32_t *closed, const int32_t *fix, hipStream_t s) {
            launch_label(g, lg, n, p0, starts_dev, rot_dev, tl, tr, S, closed, fix, part, rows_dev, counts_dev, s);
        },
        cap);
}

extern "C" int dgdm_squeeze_objective_values(const DgdmSqueezeConfig *cfg, const int32_t *cells_dev, const double *y_dev, const double *starts_dev,
                                             int n_pairs, int n_starts, int B, const DgdmObjective *objectives_host, const float *rowcoef_dev,
                                             const double score_std[3], double *values_dev, void *stream) {
    const char *fn = "dgdm_squeeze_objective_values";
    int rc = check_config(cfg, fn);
    if (rc) return rc;
    DGDM_REQUIRE(cells_dev && y_dev && starts_dev && objectives_host && score_std && values_dev, DGDM_EINVAL, "%s: null argument", fn);
    DGDM_REQUIRE(B >= 1 && n_starts >= 1 && n_pairs >= 0 && n_pairs % B == 0, DGDM_EINVAL,
                 "%s: %d pairs of %d starts in groups of %d (need B >= 1, n_starts >= 1, whole groups)", fn, n_pairs, n_starts, B);
    for (int j = 0; j < 3; ++j)
        DGDM_REQUIRE(std::isfinite(score_std[j]) && score_std[j] > 0.0, DGDM_EINVAL, "%s: score_std[%d] = %g (need finite, > 0)", fn, j, score_std[j]);
    const int groups = n_pairs / B;
    for (int i = 0; i < groups; ++i) {
        const int u = objectives_host[i].use_rowcoef;
        DGDM_REQUIRE(u != DGDM_OBJ_ROWFIELD, DGDM_EINVAL, "%s: objective %d reads a row field; goal fields have no squeeze form", fn, i);
        DGDM_REQUIRE(u == 0 || u == 1, DGDM_EINVAL, "%s: objective %d has use_rowcoef %d", fn, i, u);
        DGDM_REQUIRE(u == 0 || rowcoef_dev, DGDM_EINVAL, "%s: objective %d uses rowcoef, rowcoef_dev is null", fn, i);
    }
    if (n_pairs == 0) return DGDM_OK;
    hipStream_t s = (hipStream_t)stream;
    DevBuf obj;
    if ((rc = obj.alloc(sizeof(DgdmObjective) * (size_t)groups))) return rc;
    DGDM_HIP_CHECK(hipMemcpyAsync(obj.p, objectives_host, sizeof(DgdmObjective) * (size_t)groups, hipMemcpyHostToDevice, s));
    const Grid g = grid_of(cfg);
    const ValueGrid vg = {g.T, g.X, n_starts, B, TWO_PI / (double)g.T, g.dx, score_std[0], score_std[1], score_std[2]};
    hipLaunchKernelGGL(squeeze_values_kernel, dim3((unsigned)n_pairs), dim3(64), 0, s, vg, cells_dev, y_dev, starts_dev, obj.as<DgdmObjective>(),
                       rowcoef_dev, values_dev);
    DGDM_HIP_CHECK(hipGetLastError());
    DGDM_HIP_CHECK(hipStreamSynchronize(s));        // the objectives' host array and their device copy belong to this call
    return DGDM_OK;
}

// The body of dgdm_squeeze_slice (with_normals = false: normals_dev unused) and dgdm_squeeze_slice_normals.
static int slice_common(const char *fn, bool with_normals, const double *verts_host, const int64_t *vert_offsets_host, const int32_t *tris_host,
                        const int64_t *tri_offsets_host, int n_objects, const double *gz_host, int mv, double *segments_dev, int64_t capacity,
                        int32_t *seg_offsets_host, int64_t *n_segments_host, void *stream, double *normals_dev) {
    DGDM_REQUIRE(verts_host && vert_offsets_host && tris_host && tri_offsets_host && gz_host && seg_offsets_host && n_segments_host, DGDM_EINVAL,
                 "%s: null argument", fn);
    DGDM_REQUIRE(n_objects >= 1 && n_objects <= 65535, DGDM_EINVAL, "%s: %d objects (need 1 .. 65535)", fn, n_objects);
    DGDM_REQUIRE(mv >= 1 && mv <= MAX_LEVELS, DGDM_EINVAL, "%s: %d levels (need 1 .. %d)", fn, mv, MAX_LEVELS);
    DGDM_REQUIRE(capacity >= 0 && (segments_dev || capacity == 0), DGDM_EINVAL, "%s: capacity %lld with%s segments_dev", fn, (long long)capacity,
                 segments_dev ? "" : " no");
    DGDM_REQUIRE(!with_normals || normals_dev || !segments_dev, DGDM_EINVAL, "%s: segments_dev with no normals_dev", fn);
    int rc = check_ascending(gz_host, mv, "gz", fn);
    if (rc) return rc;
    DGDM_REQUIRE(vert_offsets_host[0] == 0 && tri_offsets_host[0] == 0, DGDM_EINVAL, "%s: offsets start at %lld and %lld (need 0)", fn,
                 (long long)vert_offsets_host[0], (long long)tri_offsets_host[0]);
    for (int o = 0; o < n_objects; ++o) {
        const int64_t nv = vert_offsets_host[o + 1] - vert_offsets_host[o], nt = tri_offsets_host[o + 1] - tri_offsets_host[o];
        DGDM_REQUIRE(nv >= 1 && nt >= 0, DGDM_EINVAL, "%s: mesh %d has %lld vertices and %lld triangles", fn, o, (long long)nv, (long long)nt);
        DGDM_REQUIRE(vert_offsets_host[o + 1] <= INT32_MAX && tri_offsets_host[o + 1] <= INT32_MAX, DGDM_EINVAL,
                     "%s: more than 2^31 - 1 vertices or triangles", fn);
        const double *V = verts_host + 3 * vert_offsets_host[o];
        for (int64_t i = 0; i < 3 * nv; ++i)
            DGDM_REQUIRE(std::isfinite(V[i]), DGDM_EINVAL, "%s: mesh %d, vertex %lld is not finite", fn, o, (long long)(i / 3));
        const int32_t *F = tris_host + 3 * tri_offsets_host[o];
        for (int64_t i = 0; i < 3 * nt; ++i)
            DGDM_REQUIRE(F[i] >= 0 && F[i] < nv, DGDM_EINVAL, "%s: mesh %d, triangle %lld names vertex %d of %lld", fn, o, (long long)(i / 3), F[i],
                         (long long)nv);
    }
    const int64_t nv_all = vert_offsets_host[n_objects], nt_all = tri_offsets_host[n_objects];
    hipStream_t s = (hipStream_t)stream;
    DevBuf verts, tris, voff, toff, gz, counts, offs;
    const size_t no1 = (size_t)n_objects + 1, nl = (size_t)n_objects * mv, nl1 = (size_t)n_objects * (mv + 1);
    if ((rc = verts.alloc(sizeof(double) * 3 * (size_t)nv_all)) || (rc = tris.alloc(sizeof(int32_t) * 3 * (size_t)std::max<int64_t>(nt_all, 1))) ||
        (rc = voff.alloc(sizeof(int64_t) * no1)) || (rc = toff.alloc(sizeof(int64_t) * no1)) || (rc = gz.alloc(sizeof(double) * mv)) ||
        (rc = counts.alloc(sizeof(int32_t) * nl)) || (rc = offs.alloc(sizeof(int32_t) * nl1)))
        return rc;
    DGDM_HIP_CHECK(hipMemcpyAsync(verts.p, verts_host, sizeof(double) * 3 * (size_t)nv_all, hipMemcpyHostToDevice, s));
    if (nt_all > 0) DGDM_HIP_CHECK(hipMemcpyAsync(tris.p, tris_host, sizeof(int32_t) * 3 * (size_t)nt_all, hipMemcpyHostToDevice, s));
    DGDM_HIP_CHECK(hipMemcpyAsync(voff.p, vert_offsets_host, sizeof(int64_t) * no1, hipMemcpyHostToDevice, s));
    DGDM_HIP_CHECK(hipMemcpyAsync(toff.p, tri_offsets_host, sizeof(int64_t) * no1, hipMemcpyHostToDevice, s));
    DGDM_HIP_CHECK(hipMemcpyAsync(gz.p, gz_host, sizeof(double) * mv, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(slice_kernel<false>, dim3((unsigned)mv, (unsigned)n_objects), dim3(256), 0, s, verts.as<double>(), tris.as<int32_t>(),
                       voff.as<int64_t>(), toff.as<int64_t>(), gz.as<double>(), mv, counts.as<int32_t>(), (const int32_t *)nullptr, (double *)nullptr,
                       (double *)nullptr);
    DGDM_HIP_CHECK(hipGetLastError());
    std::vector<int32_t> cnt(nl);
    DGDM_HIP_CHECK(hipMemcpyAsync(cnt.data(), counts.p, sizeof(int32_t) * nl, hipMemcpyDeviceToHost, s));
    DGDM_HIP_CHECK(hipStreamSynchronize(s));
    int64_t total = 0;                                                     // the scan: n_objects x mv counts, on the host
    for (int o = 0; o < n_objects; ++o) {
        for (int j = 0; j < mv; ++j) {
            DGDM_REQUIRE(total <= INT32_MAX, DGDM_EINVAL, "%s: more than 2^31 - 1 segments", fn);
            seg_offsets_host[(size_t)o * (mv + 1) + j] = (int32_t)total;
            total += cnt[(size_t)o * mv + j];
        }
        DGDM_REQUIRE(total <= INT32_MAX, DGDM_EINVAL, "%s: more than 2^31 - 1 segments", fn);
        seg_offsets_host[(size_t)o * (mv + 1) + mv] = (int32_t)total;
    }
    *n_segments_host = total;
    if (!segments_dev && capacity == 0) return DGDM_OK;                    // count only
    DGDM_REQUIRE(capacity >= total, DGDM_EINVAL, "%s: capacity of %lld segments, %lld needed", fn, (long long)capacity, (long long)total);
    if (total == 0) return DGDM_OK;
    DGDM_HIP_CHECK(hipMemcpyAsync(offs.p, seg_offsets_host, sizeof(int32_t) * nl1, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(slice_kernel<true>, dim3((unsigned)mv, (unsigned)n_objects), dim3(256), 0, s, verts.as<double>(), tris.as<int32_t>(),
                       voff.as<int64_t>(), toff.as<int64_t>(), gz.as<double>(), mv, (int32_t *)nullptr, offs.as<int32_t>(), segments_dev,
                       with_normals ? normals_dev : (double *)nullptr);
    DGDM_HIP_CHECK(hipGetLastError());
    DGDM_HIP_CHECK(hipStreamSynchronize(s));
    return DGDM_OK;
}

extern "C" int dgdm_squeeze_slice(const double *verts_host, const int64_t *vert_offsets_host, const int32_t *tris_host,
                                  const int64_t *tri_offsets_host, int n_objects, const double *gz_host, int mv, double *segments_dev,
                                  int64_t capacity, int32_t *seg_offsets_host, int64_t *n_segments_host, void *stream) {
    return slice_common("dgdm_squeeze_slice", false, verts_host, vert_offsets_host, tris_host, tri_offsets_host, n_objects, gz_host, mv, segments_dev,
                        capacity, seg_offsets_host, n_segments_host, stream, nullptr);
}

extern "C" int dgdm_squeeze_slice_normals(const double *verts_host, const int64_t *vert_offsets_host, const int32_t *tris_host,
                                          const int64_t *tri_offsets_host, int n_objects, const double *gz_host, int mv, double *segments_dev,
                                          int64_t capacity, int32_t *seg_offsets_host, int64_t *n_segments_host, void *stream,
                                          double *normals_dev) {
    return slice_common("dgdm_squeeze_slice_normals", true, verts_host, vert_offsets_host, tris_host, tri_offsets_host, n_objects, gz_host, mv,
                        segments_dev, capacity, seg_offsets_host, n_segments_host, stream, normals_dev);
}

// What the two 3-D entries check of the slices they are handed, and how they put gx and the level offsets into the workspace's first
// bytes (extra3).
static int check_slices(const char *fn, const double *segments_dev, int64_t n_segments, const int32_t *seg_offsets_host, int n_objects, int mv) {
    DGDM_REQUIRE(n_segments >= 0 && n_segments <= INT32_MAX && (segments_dev || n_segments == 0), DGDM_EINVAL, "%s: %lld segments with%s segments_dev",
                 fn, (long long)n_segments, segments_dev ? "" : " no");
    const size_t nl1 = (size_t)n_objects * (size_t)(mv + 1);
    DGDM_REQUIRE(seg_offsets_host[0] == 0, DGDM_EINVAL, "%s: seg_offsets start at %d (need 0)", fn, seg_offsets_host[0]);
    for (size_t i = 1; i < nl1; ++i)
        DGDM_REQUIRE(seg_offsets_host[i] >= seg_offsets_host[i - 1], DGDM_EINVAL, "%s: seg_offsets descend at %lld (%d after %d)", fn, (long long)i,
                     seg_offsets_host[i], seg_offsets_host[i - 1]);
    DGDM_REQUIRE(seg_offsets_host[nl1 - 1] <= n_segments, DGDM_EINVAL, "%s: seg_offsets end at %d, past the %lld segments", fn,
                 seg_offsets_host[nl1 - 1], (long long)n_segments);
    return DGDM_OK;
}

static int upload_extra3(const Extra3 &e, uint8_t *ws, const double *gx_host, int mu, const int32_t *seg_offsets_host, int n_objects, int mv,
                         hipStream_t s, double *&gx, int32_t *&offs) {
    gx = reinterpret_cast<double *>(ws + e.gx);
    offs = reinterpret_cast<int32_t *>(ws + e.off);
    DGDM_HIP_CHECK(hipMemcpyAsync(gx, gx_host, sizeof(double) * mu, hipMemcpyHostToDevice, s));
    DGDM_HIP_CHECK(hipMemcpyAsync(offs, seg_offsets_host, sizeof(int32_t) * (size_t)n_objects * (size_t)(mv + 1), hipMemcpyHostToDevice, s));
    return DGDM_OK;
}

extern "C" int64_t dgdm_squeeze_map_3d_workspace_bytes(const DgdmSqueezeConfig *cfg, int chunk_pairs, int mu, int mv, int n_objects) {
    const char *fn = "dgdm_squeeze_map_3d_workspace_bytes";
    if (check_sizes_3d(mu, mv, n_objects, fn)) return DGDM_EINVAL;
    return workspace_bytes_of(fn, cfg, chunk_pairs, false, extra3(mu, mv, n_objects).bytes);
}

// The body of dgdm_squeeze_map_3d (friction = false: gz_host, normals_dev, fmu, jam_dev and contact_dev unused) and
// dgdm_squeeze_map_3d_friction.
static int squeeze_map_3d_common(const char *fn, const char *bytes_fn, bool friction, const DgdmSqueezeConfig *cfg, const double *surfaces_dev,
                                 int n_fingers, const double *gx_host, int mu, int mv, const double *segments_dev, int64_t n_segments,
                                 const int32_t *seg_offsets_host, int n_objects, const int32_t *pairs_host, int n_pairs, const double *rot_dev,
                                 const double *starts_dev, int n_starts, int32_t *cells_dev, double *y_dev, int32_t *flags_dev, double *table_s_dev,
                                 double *touch_l_dev, double *touch_r_dev, int32_t *succ_dev, void *workspace_dev, int64_t workspace_bytes,
                                 void *stream, const double *gz_host, const double *normals_dev, double fmu, int32_t *jam_dev,
                                 int32_t *contact_dev) {
    int rc = check_sizes_3d(mu, mv, n_objects, fn);
    if (rc) return rc;
    DGDM_REQUIRE(!friction || (std::isfinite(fmu) && fmu >= 0.0), DGDM_EINVAL, "%s: friction coefficient %g (need finite, >= 0)", fn, fmu);
    const Extra3 e = extra3(mu, mv, n_objects, friction);
    Outputs out = {cells_dev, y_dev, flags_dev, table_s_dev, touch_l_dev, touch_r_dev, succ_dev, friction ? jam_dev : nullptr};
    if ((rc = check_map_args(fn, cfg, surfaces_dev && gx_host && seg_offsets_host && rot_dev && (!friction || gz_host), false, n_fingers, n_objects,
                             pairs_host, n_pairs, starts_dev, n_starts, out, workspace_dev, workspace_bytes, friction, e.bytes, bytes_fn)) ||
        (rc = check_ascending(gx_host, mu, "gx", fn)))
        return rc;
    if ((rc = check_slices(fn, segments_dev, n_segments, seg_offsets_host, n_objects, mv))) return rc;
    if (friction) {
        if ((rc = check_ascending(gz_host, mv, "gz", fn))) return rc;
        DGDM_REQUIRE(normals_dev || n_segments == 0, DGDM_EINVAL, "%s: %lld segments with no normals_dev", fn, (long long)n_segments);
        for (int o = 0; o < n_objects; ++o) {                              // a contact's code s (mu + 2) + k stays an int32
            const int64_t ns = (int64_t)seg_offsets_host[(size_t)o * (mv + 1) + mv] - seg_offsets_host[(size_t)o * (mv + 1)];
            DGDM_REQUIRE(ns * (mu + 2) <= INT32_MAX, DGDM_EINVAL, "%s: object %d has %lld segments, contact codes of %d abscissae pass 2^31 - 1", fn, o,
                         (long long)ns, mu);
        }
    }
    uint8_t *ws = static_cast<uint8_t *>(workspace_dev);                  // the extra block in front, the chunks' tables behind it
    hipStream_t s = (hipStream_t)stream;
    double *gx, *gz = nullptr;
    int32_t *offs;
    if ((rc = upload_extra3(e, ws, gx_host, mu, seg_offsets_host, n_objects, mv, s, gx, offs))) return rc;
    if (friction) {
        gz = reinterpret_cast<double *>(ws + e.gz);
        DGDM_HIP_CHECK(hipMemcpyAsync(gz, gz_host, sizeof(double) * mv, hipMemcpyHostToDevice, s));
    }
    const Grid g = grid_of(cfg);
    Grid3 g3 = {g.T, g.X, mu, mv, g.x_half, g.dx};
    const int64_t cells = (int64_t)g.T * g.X;
    const size_t lds = sizeof(double) * (size_t)(2 * mu * mv + mu + 4 * SEG_TILE) + sizeof(int32_t) * (size_t)(mv + 1);
    return run_chunks(cfg, g, pairs_host, n_pairs, starts_dev, n_starts, out, ws + e.bytes, workspace_bytes - (int64_t)e.bytes, s, friction,
                      [&](unsigned n, int64_t p0, const int32_t *pairs, double *tl, double *tr, double *S, int32_t *jam, hipStream_t st) {
                          if (friction)
                              hipLaunchKernelGGL(table3d_kernel<true>, dim3((unsigned)g3.T, n), dim3(TABLE_THREADS), lds, st, g3, surfaces_dev, gx,
                                                 segments_dev, offs, pairs, rot_dev, tl, tr, S, (const double *)gz, normals_dev, fmu, g.travel_max, jam,
                                                 contact_dev ? contact_dev + 2 * p0 * cells : nullptr);
                          else
                              hipLaunchKernelGGL(table3d_kernel<false>, dim3((unsigned)g3.T, n), dim3(TABLE_THREADS), lds, st, g3, surfaces_dev, gx,
                                                 segments_dev, offs, pairs, rot_dev, tl, tr, S, (const double *)nullptr, (const double *)nullptr, 0.0,
                                                 0.0, (int32_t *)nullptr, (int32_t *)nullptr);
                      });
}

extern "C" int dgdm_squeeze_map_3d(const DgdmSqueezeConfig *cfg, const double *surfaces_dev, int n_fingers, const double *gx_host, int mu, int mv,
                                   const double *segments_dev, int64_t n_segments, const int32_t *seg_offsets_host, int n_objects,
                                   const int32_t *pairs_host, int n_pairs, const double *rot_dev, const double *starts_dev, int n_starts,
                                   int32_t *cells_dev, double *y_dev, int32_t *flags_dev, double *table_s_dev, double *touch_l_dev,
                                   double *touch_r_dev, int32_t *succ_dev, void *workspace_dev, int64_t workspace_bytes, void *stream) {
    return squeeze_map_3d_common("dgdm_squeeze_map_3d", "dgdm_squeeze_map_3d_workspace_bytes", false, cfg, surfaces_dev, n_fingers, gx_host, mu, mv,
                                 segments_dev, n_segments, seg_offsets_host, n_objects, pairs_host, n_pairs, rot_dev, starts_dev, n_starts, cells_dev,
                                 y_dev, flags_dev, table_s_dev, touch_l_dev, touch_r_dev, succ_dev, workspace_dev, workspace_bytes, stream, nullptr,
                                 nullptr, 0.0, nullptr, nullptr);
}

extern "C" int64_t dgdm_squeeze_map_3d_friction_workspace_bytes(const DgdmSqueezeConfig *cfg, int chunk_pairs, int mu, int mv, int n_objects) {
    const char *fn = "dgdm_squeeze_map_3d_friction_workspace_bytes";
    if (check_sizes_3d(mu, mv, n_objects, fn)) return DGDM_EINVAL;
    return workspace_bytes_of(fn, cfg, chunk_pairs, true, extra3(mu, mv, n_objects, true).bytes);
}

extern "C" int dgdm_squeeze_map_3d_friction(const DgdmSqueezeConfig *cfg, const double *surfaces_dev, int n_fingers, const double *gx_host, int mu,
                                            int mv, const double *segments_dev, int64_t n_segments, const int32_t *seg_offsets_host, int n_objects,
                                            const int32_t *pairs_host, int n_pairs, const double *rot_dev, const double *starts_dev, int n_starts,
                                            int32_t *cells_dev, double *y_dev, int32_t *flags_dev, double *table_s_dev, double *touch_l_dev,
                                            double *touch_r_dev, int32_t *succ_dev, void *workspace_dev, int64_t workspace_bytes, void *stream,
                                            const double *gz_host, const double *normals_dev, double friction, int32_t *jam_dev,
                                            int32_t *contact_dev) {
    return squeeze_map_3d_common("dgdm_squeeze_map_3d_friction", "dgdm_squeeze_map_3d_friction_workspace_bytes", true, cfg, surfaces_dev, n_fingers,
                                 gx_host, mu, mv, segments_dev, n_segments, seg_offsets_host, n_objects, pairs_host, n_pairs, rot_dev, starts_dev,
                                 n_starts, cells_dev, y_dev, flags_dev, table_s_dev, touch_l_dev, touch_r_dev, succ_dev, workspace_dev, workspace_bytes,
                                 stream, gz_host, normals_dev, friction, jam_dev, contact_dev);
}

extern "C" int64_t dgdm_squeeze_label_3d_workspace_bytes(const DgdmSqueezeConfig *cfg, int chunk_fingers, int n_objects, int mu, int mv, int n_bank) {
    const char *fn = "dgdm_squeeze_label_3d_workspace_bytes";
    if (check_sizes_3d(mu, mv, n_bank, fn) || check_label_objects(fn, n_objects)) return DGDM_EINVAL;
    DGDM_REQUIRE(chunk_fingers >= 1 && (int64_t)chunk_fingers * n_objects <= MAX_CHUNK, DGDM_EINVAL,
                 "%s: %d fingers of %d objects per chunk (need >= 1 finger, at most %d pairs)", fn, chunk_fingers, n_objects, MAX_CHUNK);
    const int chunk_pairs = chunk_fingers * n_objects;
    return workspace_bytes_of(fn, cfg, chunk_pairs, false, extra3(mu, mv, n_bank).bytes + label_extra(chunk_pairs));
}

extern "C" int dgdm_squeeze_label_3d(const DgdmSqueezeConfig *cfg, const double *surfaces_dev, int n_fingers, const double *gx_host, int mu, int mv,
                                     const double *segments_dev, int64_t n_segments, const int32_t *seg_offsets_host, int n_bank,
                                     const int32_t *objects_host, int n_objects, const double *rot_dev, const double *starts_dev, int n_tally,
                                     int n_settle, const double threshold[3], const double score_std[3], double pos_norm, int row_layout,
                                     float *rows_dev, int64_t row_stride, int column_offset, int object_stride, int32_t *counts_dev,
                                     double *table_s_dev, double *touch_l_dev, double *touch_r_dev, void *workspace_dev, int64_t workspace_bytes,
                                     void *stream) {
    const char *fn = "dgdm_squeeze_label_3d";
    const char *bytes_fn = "dgdm_squeeze_label_3d_workspace_bytes";
    int rc = check_sizes_3d(mu, mv, n_bank, fn);
    if (rc || (rc = check_label_objects(fn, n_objects))) return rc;
    LabelGrid lg;
    std::vector<int32_t> pairs;
    if ((rc = label_front(fn, n_fingers, n_bank, objects_host, n_objects, starts_dev, n_tally, n_settle, threshold, score_std, pos_norm, row_layout,
                          rows_dev, row_stride, column_offset, object_stride, lg, pairs)))
        return rc;
    const int n_pairs = n_fingers * n_objects;
    const Extra3 e = extra3(mu, mv, n_bank);
    Outputs out = {};
    out.S = table_s_dev;
    out.tl = touch_l_dev;
    out.tr = touch_r_dev;
    if ((rc = check_map_args(fn, cfg, surfaces_dev && gx_host && seg_offsets_host && rot_dev, false, n_fingers, n_bank, pairs.data(), n_pairs, nullptr, 0,
                             out, workspace_dev, workspace_bytes, false, e.bytes + label_extra(1), bytes_fn)) ||
        (rc = check_ascending(gx_host, mu, "gx", fn)) || (rc = check_slices(fn, segments_dev, n_segments, seg_offsets_host, n_bank, mv)))
        return rc;
    int64_t fingers;
    if ((rc = label_chunk_fingers(fn, bytes_fn, cfg, n_fingers, n_objects, false, workspace_bytes, e.bytes, fingers))) return rc;
    const int64_t cap = fingers * n_objects;
    const size_t front = e.bytes + label_extra(cap);                      // gx and the offsets, then the partials, then the chunk's tables

    uint8_t *ws = static_cast<uint8_t *>(workspace_dev);
    hipStream_t s = (hipStream_t)stream;
    double *gx;
    int32_t *offs;
    if ((rc = upload_extra3(e, ws, gx_host, mu, seg_offsets_host, n_bank, mv, s, gx, offs))) return rc;
    PairPart *part = reinterpret_cast<PairPart *>(ws + e.bytes);
    const Grid g = grid_of(cfg);
    lg.dth = TWO_PI / (double)g.T;
    Grid3 g3 = {g.T, g.X, mu, mv, g.x_half, g.dx};
    const size_t lds = sizeof(double) * (size_t)(mu * LABEL3_ENTRY + mu + 4 * FSEG_TILE) + sizeof(int32_t) * (size_t)(mv + 1);
    return run_chunks(
        cfg, g, pairs.data(), n_pairs, nullptr, 0, out, ws + front, workspace_bytes - (int64_t)front, s, false,
        [&](unsigned n, int64_t, const int32_t *prs, double *tl, double *tr, double *S, int32_t *, hipStream_t st) {
            const int nf = (int)(n / (unsigned)n_objects);                // cap and n_pairs are whole fingers: so is every chunk
            hipLaunchKernelGGL(table3d_fingers_kernel, dim3((unsigned)g3.T, (unsigned)n_objects, (unsigned)((nf + LABEL3_FB - 1) / LABEL3_FB)),
                               dim3(TABLE_THREADS), lds, st, g3, 1, n_objects, nf, surfaces_dev, gx, segments_dev, offs, prs, rot_dev, tl, tr, S);
        },
        [&](unsigned n, int64_t p0, const double *tl, const double *tr, const double *S, const int32_t *closed, const int32_t *fix, hipStream_t st) {
            launch_label(g, lg, n, p0, starts_dev, rot_dev, tl, tr, S, closed, fix, part, rows_dev, counts_dev, st);
        },
        cap);
}

// dgdm_squeeze_values_3d's workspace: gx and the level offsets (extra3), then the chunk's objectives, then the chunk's tables.
static size_t values_extra(int64_t chunk_groups) { return align256(sizeof(DgdmObjective) * (size_t)chunk_groups); }

extern "C" int64_t dgdm_squeeze_values_3d_workspace_bytes(const DgdmSqueezeConfig *cfg, int chunk_groups, int batch, int mu, int mv, int n_bank) {
    const char *fn = "dgdm_squeeze_values_3d_workspace_bytes";
    if (check_sizes_3d(mu, mv, n_bank, fn)) return DGDM_EINVAL;
    DGDM_REQUIRE(batch >= 1 && chunk_groups >= 1 && (int64_t)chunk_groups * batch <= MAX_CHUNK, DGDM_EINVAL,
                 "%s: %d groups of %d fingers per chunk (need >= 1 each, at most %d pairs)", fn, chunk_groups, batch, MAX_CHUNK);
    return workspace_bytes_of(fn, cfg, chunk_groups * batch, false, extra3(mu, mv, n_bank).bytes + values_extra(chunk_groups));
}

extern "C" int dgdm_squeeze_values_3d(const DgdmSqueezeConfig *cfg, const double *surfaces_dev, int n_fingers, const double *gx_host, int mu, int mv,
                                      const double *segments_dev, int64_t n_segments, const int32_t *seg_offsets_host, int n_bank,
                                      const double *rot_dev, const double *starts_dev, int n_starts, int n_groups, int batch,
                                      const int32_t *group_first_host, const DgdmObjective *objectives_host, const float *rowcoef_dev,
                                      const double score_std[3], double *values_dev, double *table_s_dev, double *touch_l_dev,
                                      double *touch_r_dev, void *workspace_dev, int64_t workspace_bytes, void *stream) {
    const char *fn = "dgdm_squeeze_values_3d";
    const char *bytes_fn = "dgdm_squeeze_values_3d_workspace_bytes";
    int rc = check_sizes_3d(mu, mv, n_bank, fn);
    if (rc) return rc;
    DGDM_REQUIRE(group_first_host && objectives_host && score_std && values_dev && starts_dev, DGDM_EINVAL, "%s: null argument", fn);
    DGDM_REQUIRE(n_fingers >= 1 && n_groups >= 1 && batch >= 1 && n_starts >= 1, DGDM_EINVAL,
                 "%s: %d fingers, %d groups of %d fingers, %d starts (need >= 1 each)", fn, n_fingers, n_groups, batch, n_starts);
    DGDM_REQUIRE(batch <= MAX_CHUNK, DGDM_EINVAL, "%s: a group of %d fingers exceeds a chunk's %d pairs", fn, batch, MAX_CHUNK);
    DGDM_REQUIRE((int64_t)n_groups * batch <= INT32_MAX, DGDM_EINVAL, "%s: %d groups x %d fingers exceed 2^31 - 1 pairs", fn, n_groups, batch);
    for (int j = 0; j < 3; ++j)
        DGDM_REQUIRE(std::isfinite(score_std[j]) && score_std[j] > 0.0, DGDM_EINVAL, "%s: score_std[%d] = %g (need finite, > 0)", fn, j, score_std[j]);
    for (int i = 0; i < n_groups; ++i) {
        const int u = objectives_host[i].use_rowcoef, first = group_first_host[i], ob = objectives_host[i].object;
        DGDM_REQUIRE(u != DGDM_OBJ_ROWFIELD, DGDM_EINVAL, "%s: objective %d reads a row field; goal fields have no squeeze form", fn, i);
        DGDM_REQUIRE(u == 0 || u == 1, DGDM_EINVAL, "%s: objective %d has use_rowcoef %d", fn, i, u);
        DGDM_REQUIRE(u == 0 || rowcoef_dev, DGDM_EINVAL, "%s: objective %d uses rowcoef, rowcoef_dev is null", fn, i);
        DGDM_REQUIRE(first >= 0 && (int64_t)first + batch <= n_fingers, DGDM_EINVAL, "%s: group %d = fingers %d .. %lld of %d", fn, i, first,
                     (long long)first + batch - 1, n_fingers);
        DGDM_REQUIRE(ob >= 0 && ob < n_bank, DGDM_EINVAL, "%s: group %d names object %d outside the bank of %d", fn, i, ob, n_bank);
    }
    const int n_pairs = n_groups * batch;
    std::vector<int32_t> pairs((size_t)2 * n_pairs);                       // group-major: pair g * batch + b = (group_first[g] + b, its object)
    for (int i = 0; i < n_groups; ++i)
        for (int b = 0; b < batch; ++b) {
            pairs[2 * ((size_t)i * batch + b)] = group_first_host[i] + b;
            pairs[2 * ((size_t)i * batch + b) + 1] = objectives_host[i].object;
        }
    const Extra3 e = extra3(mu, mv, n_bank);
    Outputs out = {};
    out.S = table_s_dev;
    out.tl = touch_l_dev;
    out.tr = touch_r_dev;
    if ((rc = check_map_args(fn, cfg, surfaces_dev && gx_host && seg_offsets_host && rot_dev, false, n_fingers, n_bank, pairs.data(), n_pairs, nullptr, 0,
                             out, workspace_dev, workspace_bytes, false, e.bytes + values_extra(1), bytes_fn)) ||
        (rc = check_ascending(gx_host, mu, "gx", fn)) || (rc = check_slices(fn, segments_dev, n_segments, seg_offsets_host, n_bank, mv)))
        return rc;
    const int64_t cells = (int64_t)cfg->theta_cells * cfg->x_cells;
    auto need = [&](int64_t gr) { return (int64_t)(e.bytes + values_extra(gr) + layout(cells, gr * batch).bytes); };
    DGDM_REQUIRE(workspace_bytes >= need(1), DGDM_EINVAL, "%s: workspace of %lld bytes holds no group of %d fingers, one needs %lld (%s)", fn,
                 (long long)workspace_bytes, batch, (long long)need(1), bytes_fn);
    int64_t groups = 1, over = std::min<int64_t>(n_groups, MAX_CHUNK / batch) + 1;            // need() does not fall: bisect [groups, over)
    while (over - groups > 1) {
        const int64_t mid = groups + (over - groups) / 2;
        if (need(mid) <= workspace_bytes) groups = mid; else over = mid;
    }
    const int64_t cap = groups * batch;                                   // whole groups: a block of fingers never straddles two chunks
    const size_t front = e.bytes + values_extra(groups);

    uint8_t *ws = static_cast<uint8_t *>(workspace_dev);
    hipStream_t s = (hipStream_t)stream;
    double *gx;
    int32_t *offs;
    if ((rc = upload_extra3(e, ws, gx_host, mu, seg_offsets_host, n_bank, mv, s, gx, offs))) return rc;
    DgdmObjective *obj = reinterpret_cast<DgdmObjective *>(ws + e.bytes);
    const Grid g = grid_of(cfg);
    const ValueGrid vg = {g.T, g.X, n_starts, batch, TWO_PI / (double)g.T, g.dx, score_std[0], score_std[1], score_std[2]};
    Grid3 g3 = {g.T, g.X, mu, mv, g.x_half, g.dx};
    const size_t lds = sizeof(double) * (size_t)(mu * LABEL3_ENTRY + mu + 4 * FSEG_TILE) + sizeof(int32_t) * (size_t)(mv + 1);
    int copy_rc = DGDM_OK;
    rc = run_chunks(
        cfg, g, pairs.data(), n_pairs, nullptr, 0, out, ws + front, workspace_bytes - (int64_t)front, s, false,
        [&](unsigned n, int64_t, const int32_t *prs, double *tl, double *tr, double *S, int32_t *, hipStream_t st) {
            const unsigned ng = n / (unsigned)batch;                       // cap and n_pairs are whole groups: so is every chunk
            hipLaunchKernelGGL(table3d_fingers_kernel, dim3((unsigned)g3.T, ng, (unsigned)((batch + LABEL3_FB - 1) / LABEL3_FB)), dim3(TABLE_THREADS),
                               lds, st, g3, batch, 1, batch, surfaces_dev, gx, segments_dev, offs, prs, rot_dev, tl, tr, S);
        },
        [&](unsigned n, int64_t p0, const double *tl, const double *tr, const double *S, const int32_t *closed, const int32_t *, hipStream_t st) {
            if (hipMemcpyAsync(obj, objectives_host + p0 / batch, sizeof(DgdmObjective) * (size_t)(n / (unsigned)batch), hipMemcpyHostToDevice, st) !=
                hipSuccess) {
                copy_rc = DGDM_EHIP;
                return;
            }
            hipLaunchKernelGGL(values3d_pair_kernel, dim3(n), dim3(64), 0, st, g, vg, starts_dev, tl, tr, S, closed, (const DgdmObjective *)obj,
                               rowcoef_dev, p0, values_dev);
        },
        cap);
    return rc ? rc : copy_rc;
}

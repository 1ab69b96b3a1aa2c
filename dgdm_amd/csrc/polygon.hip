// Triangulation and convex decomposition of closed rings of integer points: what the reference gets from `triangle` (constrained
// Delaunay faces of the icon contour, assets/icon_process.py:62-92) and from an external V-HACD run on the extruded mesh
// (sim/sim_2d.py:103-111), as an exact-integer contract of this project's own (include/dgdm_hip.h "integer rings", DESIGN.md §4.5d;
// tests/polygon_oracle.py is its CPU oracle).  Every predicate is a cross or dot product of coordinate differences in int64
// (coordinates in [0, 32767]: |product| < 2^33); no float appears in this file.
//
// Launches, on the caller's stream:
//   1. range_kernel     one thread per coordinate: any value outside [0, 32767] raises a flag the host reads back (DGDM_EINVAL before
//                       the rings are touched);
//   2. polygon_kernel   one wave per ring, everything in LDS:
//        clean          keep[i] = p[i] != p[i - 1], compacted with ballots; one trailing point equal to the first dropped;
//        status         doubled area by a wave sum; the O(M^2) edge-pair test with edge e wave-uniform and 64 partner edges a step;
//        ear clipping   M - 3 rounds; a lane tests the candidates lane, lane + 64, ... (up to four at n = 256) against every current
//                       vertex (LDS broadcast reads); a ballot per 64 candidates and its lowest set bit (highest, in a reversed ring)
//                       pick the ear with the smallest original index; lane 0 unlinks it and records the triangle and its twins;
//        pieces         Hertel-Mehlhorn on half-edge next / previous tables by lane 0 (M - 3 dependent steps), the faces collected by
//                       lane 0 into LDS, every output row written by the whole wave with its padding.
// A ring's result is a function of its own n points only: nothing is shared between waves.
// LDS per wave (one wave per workgroup): 2 x 1024 B coordinates, 4 x 512 B index / link / edge tables, 256 B alive flags,
// 4 x 1524 B half-edge tables (origin, twin, next, previous) = 10 404 B (10 496 B allocated); 53 VGPRs, no scratch.
#include "common.h"

namespace dgdm {
namespace {

constexpr int MAX_N = 256;                 // points per ring
constexpr int MAX_H = 3 * (MAX_N - 2);     // half-edges of a triangulation
constexpr int32_t MAX_COORD = 32767;
enum { ST_OK = 0, ST_FEW = 1, ST_AREA = 2, ST_SIMPLE = 3, ST_EAR = 4 };

struct PolygonOut {
    int32_t *status, *count, *ring;
    int64_t *area2;
    int32_t *tris, *piece_count, *piece_off, *piece_idx;
};

__device__ __forceinline__ int64_t cross3(int ax, int ay, int bx, int by, int cx, int cy) {
    return (int64_t)(bx - ax) * (cy - ay) - (int64_t)(by - ay) * (cx - ax);
}

__device__ __forceinline__ bool within(int a, int b, int c) { return min(a, b) <= c && c <= max(a, b); }

// the closed segments a b and c d share a point
__device__ bool segments_touch(int ax, int ay, int bx, int by, int cx, int cy, int dx, int dy) {
    const int64_t d1 = cross3(cx, cy, dx, dy, ax, ay), d2 = cross3(cx, cy, dx, dy, bx, by);
    const int64_t d3 = cross3(ax, ay, bx, by, cx, cy), d4 = cross3(ax, ay, bx, by, dx, dy);
    if (((d1 > 0 && d2 < 0) || (d1 < 0 && d2 > 0)) && ((d3 > 0 && d4 < 0) || (d3 < 0 && d4 > 0))) return true;
    if (d1 == 0 && within(cx, dx, ax) && within(cy, dy, ay)) return true;
    if (d2 == 0 && within(cx, dx, bx) && within(cy, dy, by)) return true;
    if (d3 == 0 && within(ax, bx, cx) && within(ay, by, cy)) return true;
    if (d4 == 0 && within(ax, bx, dx) && within(ay, by, dy)) return true;
    return false;
}

__device__ __forceinline__ int64_t wave_sum(int64_t v) {
    for (int off = 32; off; off >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, off), hi = (uint32_t)__shfl_xor((int)(v >> 32), off);
        v += (int64_t)(((uint64_t)hi << 32) | lo);
    }
    return v;
}

__global__ void range_kernel(const int32_t *p, int64_t count, int32_t *flag) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool bad = g < count && (uint32_t)p[g] > (uint32_t)MAX_COORD;
    if (__ballot(bad) && (threadIdx.x & 63) == 0) atomicOr(flag, 1);
}

// points [batch][n][2]; one workgroup of one wave per ring.  Every pointer of o but status may be null.
__global__ __launch_bounds__(64) void polygon_kernel(const int32_t *points, int n, PolygonOut o) {
    __shared__ int32_t px[MAX_N], py[MAX_N];                         // the cleaned ring, in working order from the reversal on
    __shared__ int16_t oid[MAX_N];                                   // original index of working position w
    __shared__ int16_t nx[MAX_N], pv[MAX_N];                         // the current polygon as a doubly linked ring
    __shared__ int16_t eout[MAX_N];                                  // half-edge on the far side of the edge w -> nx[w] (-1: an input edge)
    __shared__ uint8_t alive[MAX_N];
    __shared__ int16_t org[MAX_H], twin[MAX_H], hn[MAX_H], hp[MAX_H];   // half-edge 3 t + k leaves vertex k of triangle t
    const int lane = threadIdx.x;
    const int64_t b = blockIdx.x;
    const int32_t *p = points + b * n * 2;
    const int chunks_n = (n + 63) >> 6;

    // ---- clean
    int M = 0;
    for (int c = 0; c < chunks_n; ++c) {
        const int i = 64 * c + lane;
        bool keep = false;
        int x = 0, y = 0;
        if (i < n) {
            x = p[2 * i];
            y = p[2 * i + 1];
            keep = i == 0 || x != p[2 * i - 2] || y != p[2 * i - 1];
        }
        const uint64_t mask = __ballot(keep);
        if (keep) {
            const int w = M + __popcll(mask & ((1ull << lane) - 1));
            px[w] = x;
            py[w] = y;
            oid[w] = (int16_t)i;
        }
        M += __popcll(mask);
    }
    __syncthreads();
    while (M > 1 && px[M - 1] == px[0] && py[M - 1] == py[0]) --M;
    if (o.ring)
        for (int k = lane; k < n; k += 64) o.ring[b * n + k] = k < M ? oid[k] : -1;

    // ---- status
    int status = ST_OK;
    int64_t a2 = 0;
    if (M < 3) {
        status = ST_FEW;
    } else {
        int64_t part = 0;
        for (int k = lane; k < M; k += 64) {
            const int k1 = k + 1 == M ? 0 : k + 1;
            part += (int64_t)px[k] * py[k1] - (int64_t)px[k1] * py[k];
        }
        a2 = wave_sum(part);
        if (a2 == 0) {
            status = ST_AREA;
        } else {
            bool bad = false;
            for (int k = lane; k < M; k += 64) {                     // adjacent edges folding back
                const int k1 = k + 1 >= M ? k + 1 - M : k + 1, k2 = k + 2 >= M ? k + 2 - M : k + 2;
                const int64_t ux = px[k1] - px[k], uy = py[k1] - py[k], vx = px[k2] - px[k1], vy = py[k2] - py[k1];
                bad |= ux * vy - uy * vx == 0 && ux * vx + uy * vy < 0;
            }
            for (int e = 0; e + 2 < M; ++e) {                        // edge e against the non-adjacent edges after it
                const int ax = px[e], ay = py[e], bx = px[e + 1], by = py[e + 1];
                for (int f = e + 2 + lane; f < M; f += 64) {
                    if (e == 0 && f == M - 1) continue;
                    const int f1 = f + 1 == M ? 0 : f + 1;
                    bad |= segments_touch(ax, ay, bx, by, px[f], py[f], px[f1], py[f1]);
                }
            }
            if (__ballot(bad)) status = ST_SIMPLE;
        }
    }

    int T = 0;
    if (status == ST_OK) {
        // ---- the working order: counter-clockwise
        const bool rev = a2 < 0;
        __syncthreads();
        if (rev) {
            for (int k = lane; k < M / 2; k += 64) {
                const int q = M - 1 - k;
                const int32_t tx = px[k], ty = py[k];
                const int16_t ti = oid[k];
                px[k] = px[q]; py[k] = py[q]; oid[k] = oid[q];
                px[q] = tx; py[q] = ty; oid[q] = ti;
            }
        }
        __syncthreads();
        for (int k = lane; k < M; k += 64) {
            nx[k] = (int16_t)(k + 1 == M ? 0 : k + 1);
            pv[k] = (int16_t)(k == 0 ? M - 1 : k - 1);
            eout[k] = -1;
            alive[k] = 1;
        }
        __syncthreads();

        // ---- ear clipping
        const int chunks = (M + 63) >> 6;
        int anchor = 0;                                              // a vertex that is still in the polygon
        for (int m = M; m > 3; --m) {
            int tip = -1;
            for (int cc = 0; cc < chunks && tip < 0; ++cc) {
                const int c = rev ? chunks - 1 - cc : cc;            // a reversed ring: original indices fall as positions rise
                const int j = 64 * c + lane;
                bool ear = false;
                if (j < M && alive[j]) {
                    const int i = pv[j], l = nx[j];
                    const int ax = px[i], ay = py[i], bx = px[j], by = py[j], cx = px[l], cy = py[l];
                    if (cross3(ax, ay, bx, by, cx, cy) > 0) {
                        ear = true;
                        for (int v = 0; v < M; ++v) {
                            if (!alive[v] || v == i || v == j || v == l) continue;
                            const int vx = px[v], vy = py[v];
                            if (cross3(ax, ay, bx, by, vx, vy) >= 0 && cross3(bx, by, cx, cy, vx, vy) >= 0 && cross3(cx, cy, ax, ay, vx, vy) >= 0) {
                                ear = false;
                                break;
                            }
                        }
                    }
                }
                const uint64_t mask = __ballot(ear);
                if (mask) tip = 64 * c + (rev ? 63 - __builtin_clzll(mask) : __builtin_ctzll(mask));
            }
            if (tip < 0) {
                status = ST_EAR;
                break;
            }
            const int i = pv[tip], l = nx[tip];
            __syncthreads();
            if (lane == 0) {
                const int h = 3 * T;
                org[h] = (int16_t)i; org[h + 1] = (int16_t)tip; org[h + 2] = (int16_t)l;
                const int e0 = eout[i], e1 = eout[tip];
                twin[h] = (int16_t)e0; twin[h + 1] = (int16_t)e1; twin[h + 2] = -1;
                if (e0 >= 0) twin[e0] = (int16_t)h;
                if (e1 >= 0) twin[e1] = (int16_t)(h + 1);
                eout[i] = (int16_t)(h + 2);                           // the new edge i -> l has the diagonal l -> i behind it
                nx[i] = (int16_t)l;
                pv[l] = (int16_t)i;
                alive[tip] = 0;
            }
            anchor = i;
            ++T;
            __syncthreads();
        }
        if (status == ST_OK) {                                       // the last three: tip = the smallest original index
            if (lane == 0) {
                int j = anchor;
                const int u = nx[j], w = nx[u];
                if (oid[u] < oid[j]) j = u;
                if (oid[w] < oid[j]) j = w;
                const int h = 3 * T;
                auto leave = [&](int k, int v) {                    // half-edge h + k leaves v along the polygon edge v -> nx[v]
                    org[h + k] = (int16_t)v;
                    const int e = eout[v];
                    twin[h + k] = (int16_t)e;
                    if (e >= 0) twin[e] = (int16_t)(h + k);
                };
                leave(0, pv[j]);
                leave(1, j);
                leave(2, nx[j]);
            }
            ++T;
            __syncthreads();
        }
    }
    if (status != ST_OK) T = 0;

    if (lane == 0) {
        o.status[b] = status;
        if (o.count) o.count[b] = M;
        if (o.area2) o.area2[b] = status == ST_FEW ? 0 : a2;
    }
    if (o.tris) {
        int32_t *out = o.tris + b * 3 * (n - 2);
        for (int k = lane; k < 3 * (n - 2); k += 64) out[k] = k < 3 * T ? oid[org[k]] : -1;
    }
    if (!o.piece_count) return;

    // ---- convex pieces
    int pieces = 0;
    if (T > 0) {
        for (int h = lane; h < 3 * T; h += 64) {
            const int t3 = h - h % 3;
            hn[h] = (int16_t)(t3 + (h + 1) % 3);
            hp[h] = (int16_t)(t3 + (h + 2) % 3);
        }
        __syncthreads();
        if (lane == 0) {
            for (int t = T - 2; t >= 0; --t) {                       // diagonal t: l -> i of triangle t and its twin i -> l
                const int h = 3 * t + 2, g = twin[h];
                if (g < 0) continue;                                  // every diagonal has a far side; an index is never formed from -1
                const int vi = org[g], vl = org[h];
                const int x = org[hp[g]], y = org[hn[hn[h]]], x2 = org[hp[h]], y2 = org[hn[hn[g]]];
                if (cross3(px[x], py[x], px[vi], py[vi], px[y], py[y]) >= 0 && cross3(px[x2], py[x2], px[vl], py[vl], px[y2], py[y2]) >= 0) {
                    const int a = hp[g], bb = hn[h], c = hp[h], d = hn[g];
                    hn[a] = (int16_t)bb; hp[bb] = (int16_t)a;
                    hn[c] = (int16_t)d; hp[d] = (int16_t)c;
                    hn[h] = -1; hn[g] = -1;
                }
            }
            // the faces, by lowest half-edge; twin and eout are free by now: the index list and the offsets are staged in them
            int off = 0;
            for (int h = 0; h < 3 * T; ++h) {
                if (hn[h] < 0) continue;
                eout[pieces++] = (int16_t)off;
                int e = h;
                while (hn[e] >= 0 && off < 3 * T) {
                    twin[off++] = oid[org[e]];
                    const int nxt = hn[e];
                    hn[e] = -1;
                    e = nxt;
                }
            }
            eout[pieces] = (int16_t)off;
        }
        __syncthreads();
        pieces = __shfl(pieces, 0);
    }
    if (lane == 0) o.piece_count[b] = pieces;
    const int total = pieces ? eout[pieces] : 0;
    for (int k = lane; k < n - 1; k += 64) o.piece_off[b * (n - 1) + k] = pieces && k <= pieces ? eout[k] : -1;
    for (int k = lane; k < 3 * (n - 2); k += 64) o.piece_idx[b * 3 * (n - 2) + k] = k < total ? twin[k] : -1;
}

int run(const char *fn, const int32_t *points_dev, int batch, int n, const PolygonOut &o, bool pieces, void *stream) {
    DGDM_REQUIRE(batch >= 1, DGDM_EINVAL, "%s: %d rings (need >= 1)", fn, batch);
    DGDM_REQUIRE(n >= 3 && n <= MAX_N, DGDM_EINVAL, "%s: %d points per ring (need 3 .. %d)", fn, n, MAX_N);
    DGDM_REQUIRE(points_dev && o.status, DGDM_EINVAL, "%s: null argument", fn);
    DGDM_REQUIRE(pieces ? o.piece_count && o.piece_off && o.piece_idx : o.count && o.ring && o.area2 && o.tris, DGDM_EINVAL,
                 "%s: null argument", fn);
    hipStream_t s = (hipStream_t)stream;
    const int64_t coords = (int64_t)batch * n * 2;
    int32_t flag = 0;
    DGDM_HIP_CHECK(hipMemsetAsync(o.status, 0, sizeof(int32_t), s));            // status[0] serves as the flag until the rings are run
    hipLaunchKernelGGL(range_kernel, dim3((unsigned)((coords + 255) / 256)), dim3(256), 0, s, points_dev, coords, o.status);
    DGDM_HIP_CHECK(hipGetLastError());
    DGDM_HIP_CHECK(hipMemcpyAsync(&flag, o.status, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    DGDM_HIP_CHECK(hipStreamSynchronize(s));
    DGDM_REQUIRE(!flag, DGDM_EINVAL, "%s: a coordinate outside [0, %d]", fn, MAX_COORD);
    hipLaunchKernelGGL(polygon_kernel, dim3((unsigned)batch), dim3(64), 0, s, points_dev, n, o);
    DGDM_HIP_CHECK(hipGetLastError());
    return DGDM_OK;
}

}  // namespace
}  // namespace dgdm

using namespace dgdm;

extern "C" int dgdm_polygon_triangulate(const int32_t *points_dev, int batch, int n, int32_t *status_dev, int32_t *count_dev, int32_t *ring_dev,
                                        int64_t *area2_dev, int32_t *triangles_dev, void *stream) {
    return run("dgdm_polygon_triangulate", points_dev, batch, n,
               PolygonOut{status_dev, count_dev, ring_dev, area2_dev, triangles_dev, nullptr, nullptr, nullptr}, false, stream);
}

extern "C" int dgdm_polygon_convex_pieces(const int32_t *points_dev, int batch, int n, int32_t *status_dev, int32_t *count_dev, int32_t *ring_dev,
                                          int64_t *area2_dev, int32_t *triangles_dev, int32_t *piece_count_dev, int32_t *piece_offsets_dev,
                                          int32_t *piece_index_dev, void *stream) {
    return run("dgdm_polygon_convex_pieces", points_dev, batch, n,
               PolygonOut{status_dev, count_dev, ring_dev, area2_dev, triangles_dev, piece_count_dev, piece_offsets_dev, piece_index_dev}, true,
               stream);
}

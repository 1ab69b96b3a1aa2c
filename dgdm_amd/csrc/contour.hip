// Object contours from icon images: the reference's assets/icon_process.py:extract_contours (cv2.resize to 128 x 128, BGR2GRAY,
// threshold 240 inverted, findContours RETR_EXTERNAL + CHAIN_APPROX_SIMPLE, the longest by arcLength, resample_contour, int32,
// rescale), which generator/train.py:111-124 applies to the Icons-50 test ids.  The contract, exact in integers and float64, is
// DESIGN.md "Object contours from icon images"; tests/icon_oracle.py is its CPU oracle.
//
// Launches, all on the caller's stream:
//   dgdm_icon_trace
//     1. binarise_kernel    one thread per output pixel (one workgroup per output row): resize taps, grey, threshold; two wave64
//                           ballots make the row's 128-bit mask;
//     2. trace_kernel       one wave per image: the framed 130 x 130 label image in LDS, candidates found with ballots over the row,
//                           one lane follows each outer border (marks as OpenCV sets them) and keeps the longest; the call reads the
//                           point counts back (one stream synchronisation) so that the caller sizes the point buffer exactly.
//   dgdm_icon_fetch_contours
//     3. fetch_kernel       one thread per image: the winner traced again from its start on the mask (the path depends on zero /
//                           non-zero only, so it is pass 2's), its points written.
//   dgdm_contour_resample (also the public resample_contour for caller-supplied contours)
//     4. cumlen_kernel      one thread per contour: the running sum of the segment lengths, strictly sequential as np.cumsum;
//     5. resample_kernel    one thread per output point: linspace, np.interp's search and formula, truncation, optional rescale.
// This file is compiled with -ffp-contract=off (build.py): no operation of the contract is fused.
#include "common.h"
#include <algorithm>
#include <cmath>
#include <cstring>

namespace dgdm {
namespace {

constexpr int SIZE = 128;                 // the reference resizes every icon to 128 x 128
constexpr int FW = SIZE + 2;              // framed by one pixel of background
constexpr int MASK_WORDS = SIZE * 2;      // 128 rows of two 64-bit words
constexpr int8_t MARK_POS = 2, MARK_NEG = -126;   // OpenCV's nbd and nbd | -128 for 8-bit images

__constant__ int8_t kDX[8] = {1, 1, 0, -1, -1, -1, 0, 1};
__constant__ int8_t kDY[8] = {0, -1, -1, -1, 0, 1, 1, 1};

// ------------------------------------------------------------------------------------------------------------------ binarise
struct Tap { int s0, s1, w0, w1; };

// INTER_LINEAR fixed-point tap of output index d for a source extent n.  scale = 1 / (128 / n), as OpenCV forms it.
__device__ Tap linear_tap(int d, int n) {
    const double scale = 1.0 / ((double)SIZE / (double)n);
    float f = (float)(((double)d + 0.5) * scale - 0.5);
    int s = (int)floorf(f);
    f = f - (float)s;
    if (s < 0) { s = 0; f = 0.f; }
    if (s >= n - 1) { s = n - 1; f = 0.f; }
    Tap t;
    t.s0 = s;
    t.s1 = min(s + 1, n - 1);
    t.w0 = (int)rintf((1.f - f) * 2048.f);
    t.w1 = (int)rintf(f * 2048.f);
    return t;
}

// images [M][H][W][C] uint8, channel 0 blue -> mask [M][128][2] uint64 (bit x of row y: pixel (x, y) is foreground).
// Grid: M * 128 workgroups of 128 threads; thread x of workgroup (m, y) is output pixel (x, y) of image m.
__global__ __launch_bounds__(SIZE) void binarise_kernel(const uint8_t *images, int H, int W, int C, uint64_t *mask) {
    const int y = blockIdx.x % SIZE, x = threadIdx.x;
    const int64_t m = blockIdx.x / SIZE;
    const uint8_t *img = images + m * (int64_t)H * W * C;
    int v[3];
    if (H == SIZE && W == SIZE) {                                    // cv2.resize copies
        const uint8_t *p = img + ((int64_t)y * W + x) * C;
        for (int c = 0; c < 3; ++c) v[c] = p[c];
    } else if (H == 2 * SIZE && W == 2 * SIZE) {                     // INTER_LINEAR at a factor of exactly 2: the area path
        const uint8_t *p = img + ((int64_t)(2 * y) * W + 2 * x) * C, *q = p + (int64_t)W * C;
        for (int c = 0; c < 3; ++c) v[c] = (p[c] + p[C + c] + q[c] + q[C + c] + 2) >> 2;
    } else {
        const Tap tx = linear_tap(x, W), ty = linear_tap(y, H);
        const uint8_t *r0 = img + (int64_t)ty.s0 * W * C, *r1 = img + (int64_t)ty.s1 * W * C;
        for (int c = 0; c < 3; ++c) {
            const int h0 = r0[tx.s0 * C + c] * tx.w0 + r0[tx.s1 * C + c] * tx.w1;
            const int h1 = r1[tx.s0 * C + c] * tx.w0 + r1[tx.s1 * C + c] * tx.w1;
            // OpenCV's vector vertical pass: >> 4 to int16, the high halves of the products, rounding shift by 2
            const int t = ((((h0 >> 4) * ty.w0) >> 16) + (((h1 >> 4) * ty.w1) >> 16) + 2) >> 2;
            v[c] = min(max(t, 0), 255);
        }
    }
    const int Y = (1868 * v[0] + 9617 * v[1] + 4899 * v[2] + 8192) >> 14;
    const uint64_t word = __ballot(Y <= 240);
    if ((threadIdx.x & 63) == 0) mask[(m * SIZE + y) * 2 + (threadIdx.x >> 6)] = word;
}

// ------------------------------------------------------------------------------------------------------------------ border following
// The label image seen by the border follower, in framed coordinates (the frame is background).
struct LdsLabels {                   // pass 1: OpenCV's marks live in LDS
    int8_t *lab;
    __device__ bool fg(int x, int y) const { return lab[y * FW + x] != 0; }
    __device__ void mark(int x, int y, bool right_bound) {
        int8_t &p = lab[y * FW + x];
        if (right_bound) p = MARK_NEG;
        else if (p == 1) p = MARK_POS;
    }
};

struct MaskLabels {                  // pass 2: zero / non-zero straight from the mask, nothing marked
    const uint64_t *mask;            // one image, [128][2]
    __device__ bool fg(int x, int y) const {
        if (x < 1 || x > SIZE || y < 1 || y > SIZE) return false;
        return (mask[(y - 1) * 2 + ((x - 1) >> 6)] >> ((x - 1) & 63)) & 1;
    }
    __device__ void mark(int, int, bool) {}
};

// A border visits each of its pixels at most four times: a trace that has not closed after this many steps is a bug, reported as
// such instead of looping on.
constexpr int64_t MAX_STEPS = 4 * (int64_t)SIZE * SIZE + 8;

// icvFetchContour of the outer border that starts at framed (x0, y0), CHAIN_APPROX_SIMPLE: emit(x, y) gets each point in image
// coordinates, in order.  False if the trace did not close within MAX_STEPS.
template <class Labels, class Emit>
__device__ bool follow(Labels &L, int x0, int y0, Emit &emit) {
    int s = 4, x1 = x0, y1 = y0;
    do {                                                 // backward search from direction 4: 3, 2, 1, 0, 7, 6, 5
        s = (s - 1) & 7;
        x1 = x0 + kDX[s];
        y1 = y0 + kDY[s];
    } while (!L.fg(x1, y1) && s != 4);
    if (s == 4) {                                        // no foreground neighbour: a one-point contour
        L.mark(x0, y0, true);
        emit(x0 - 1, y0 - 1);
        return true;
    }
    int x3 = x0, y3 = y0, prev_s = s ^ 4;
    for (int64_t step = 0; step < MAX_STEPS; ++step) {
        const int s_end = s;
        int x4, y4;
        do {                                             // counter-clockwise from s_end + 1; the pixel we came from ends it at the latest
            ++s;
            x4 = x3 + kDX[s & 7];
            y4 = y3 + kDY[s & 7];
        } while (s < 15 && !L.fg(x4, y4));               // OpenCV's bound (s_end + 8 at most)
        s &= 7;
        L.mark(x3, y3, (unsigned)(s - 1) < (unsigned)s_end);   // the search passed direction 0: right neighbour background
        if (s != prev_s) {
            emit(x3 - 1, y3 - 1);
            prev_s = s;
        }
        if (x4 == x0 && y4 == y0 && x3 == x1 && y3 == y1) return true;
        x3 = x4;
        y3 = y4;
        s = (s + 4) & 7;
    }
    return false;
}

// cv2.arcLength(closed) of the emitted points: float32 segment lengths summed in double.  Every term is a float >= 1 (a multiple of
// 2^-23) and the sum stays far below 2^30, so the double sum is exact in any order: the closing segment is added last here.
struct ArcLength {
    double len = 0.0;
    int64_t k = 0;
    int fx = 0, fy = 0, px = 0, py = 0;
    __device__ void seg(int x, int y) {
        const float dx = (float)(x - px), dy = (float)(y - py);
        len += (double)__fsqrt_rn(dx * dx + dy * dy);
    }
    __device__ void operator()(int x, int y) {
        if (k == 0) { fx = x; fy = y; } else seg(x, y);
        px = x;
        py = y;
        ++k;
    }
    __device__ double closed() { if (k > 1) seg(fx, fy); return len; }
};

struct Writer {
    int32_t *out;
    int64_t k = 0, cap;
    __device__ void operator()(int x, int y) {
        if (k < cap) { out[2 * k] = x; out[2 * k + 1] = y; }
        ++k;
    }
};

struct TraceRec {
    double len;          // arc length of the winner (-1: no contour)
    int64_t k;           // its point count
    int32_t x, y;        // its start pixel, framed coordinates
    int32_t n;           // external contours found
    int32_t bad;         // a trace did not close (a bug)
};

// One wave per image: cvFindNextContour's raster scan in RETR_EXTERNAL mode over the framed labels in LDS.  The scan's state (prev,
// lnbd) is wave-uniform; the change points of a row come from two ballots and are walked in order; a trace (lane 0) changes labels of
// the row, so the ballots are taken again behind it.
__global__ __launch_bounds__(64) void trace_kernel(const uint64_t *mask, TraceRec *rec) {
    __shared__ int8_t lab[FW * FW];
    __shared__ TraceRec best;
    const int lane = threadIdx.x;
    const uint64_t *mk = mask + (int64_t)blockIdx.x * MASK_WORDS;
    for (int i = lane; i < FW * FW; i += 64) {
        const int y = i / FW, x = i - y * FW;
        int8_t v = 0;
        if (y >= 1 && y <= SIZE && x >= 1 && x <= SIZE) v = (int8_t)((mk[(y - 1) * 2 + ((x - 1) >> 6)] >> ((x - 1) & 63)) & 1);
        lab[i] = v;
    }
    if (lane == 0) best = TraceRec{-1.0, 0, 0, 0, 0, 0};
    __syncthreads();
    LdsLabels L{lab};
    for (int y = 1; y <= SIZE; ++y) {
        const int8_t *row = lab + y * FW;
        int lnbd = 0;                                         // label of the last marked pixel passed (column 0: the frame)
        int from = 1;
        bool rescan = true;
        while (rescan) {
            rescan = false;
            // change points x in [from, 128]: row[x] != row[x - 1]
            uint64_t c0 = __ballot(lane + 1 >= from && row[lane + 1] != row[lane]);
            uint64_t c1 = __ballot(lane + 65 >= from && row[lane + 65] != row[lane + 64]);
            while (c0 | c1) {
                int x;
                if (c0) { x = 1 + __builtin_ctzll(c0); c0 &= c0 - 1; }
                else { x = 65 + __builtin_ctzll(c1); c1 &= c1 - 1; }
                const int p = row[x], prev = row[x - 1];
                if (prev == 0 && p == 1) {                    // outer border candidate
                    if (lnbd <= 0) {                          // not inside a traced component
                        if (lane == 0) {
                            ArcLength a;
                            if (!follow(L, x, y, a)) best.bad = 1;
                            const double len = a.closed();
                            ++best.n;
                            if (len >= best.len) { best.len = len; best.k = a.k; best.x = x; best.y = y; }   // a tie: the later one
                        }
                        __syncthreads();
                        lnbd = row[x];
                        from = x + 1;
                        rescan = true;
                        break;
                    }
                } else if (p == 0 && prev >= 1 && (prev & -2)) { // hole border candidate: never traced, lnbd moves to its left pixel
                    lnbd = prev;
                }
                if (p & -2) lnbd = p;
            }
        }
    }
    if (lane == 0) rec[blockIdx.x] = best;
}

__global__ void fetch_kernel(const uint64_t *mask, const TraceRec *rec, const int64_t *offsets, int M, int32_t *points, int32_t *bad) {
    const int m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= M) return;
    const TraceRec r = rec[m];
    MaskLabels L{mask + (int64_t)m * MASK_WORDS};
    Writer w{points + 2 * offsets[m], 0, offsets[m + 1] - offsets[m]};
    if (!follow(L, r.x, r.y, w) || w.k != w.cap) bad[m] = 1;
}

// ------------------------------------------------------------------------------------------------------------------ resample
// c = np.cumsum of [0, |p1 - p0|, |p2 - p1|, ...]: sqrt of the integer squared distance in float64, summed strictly in order.
__global__ void cumlen_kernel(const int32_t *points, const int64_t *offsets, int M, double *cum) {
    const int m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= M) return;
    const int64_t o = offsets[m], K = offsets[m + 1] - o;
    const int32_t *p = points + 2 * o;
    double c = 0.0;
    cum[o] = 0.0;
    for (int64_t i = 1; i < K; ++i) {
        const int64_t dx = (int64_t)p[2 * i] - p[2 * i - 2], dy = (int64_t)p[2 * i + 1] - p[2 * i - 1];
        c = c + __dsqrt_rn((double)(dx * dx + dy * dy));
        cum[o + i] = c;
    }
}

// out[m][j] = (int32) np.interp(u_j, c, p[:, 0|1]) with u = np.linspace(0, L, n); rescale: / 128 * 0.1 - 0.05 in float64.
__global__ void resample_kernel(const int32_t *points, const int64_t *offsets, const double *cum, int M, int n, int rescale, void *out) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= (int64_t)M * n) return;
    const int m = (int)(g / n), j = (int)(g - (int64_t)m * n);
    const int64_t o = offsets[m], K = offsets[m + 1] - o;
    const int32_t *p = points + 2 * o;
    const double *c = cum + o;
    const double L = c[K - 1];
    double u = 0.0;
    if (n > 1) {
        const double step = L / (double)(n - 1);
        u = step != 0.0 ? (double)j * step : 0.0;       // linspace: j * step; for step == 0, (j / (n - 1)) * L = 0
        if (j == n - 1) u = L;
    }
    // np.interp: the largest i with c[i] <= u (u >= 0 = c[0], u <= L)
    int64_t lo = 0, hi = K - 1;
    while (lo < hi) {
        const int64_t mid = hi - (hi - lo) / 2;
        if (c[mid] <= u) lo = mid; else hi = mid - 1;
    }
    int32_t r[2];
    for (int a = 0; a < 2; ++a) {
        const double f0 = (double)p[2 * lo + a];
        double v = f0;
        if (lo < K - 1 && c[lo] != u) {
            const double slope = ((double)p[2 * lo + 2 + a] - f0) / (c[lo + 1] - c[lo]);
            v = slope * (u - c[lo]) + f0;
        }
        r[a] = (int32_t)v;                              // astype(np.int32): truncation toward zero
    }
    if (rescale) {
        double *o2 = static_cast<double *>(out) + 2 * g;
        for (int a = 0; a < 2; ++a) o2[a] = (double)r[a] / 128.0 * 0.1 - 0.05;
    } else {
        int32_t *o2 = static_cast<int32_t *>(out) + 2 * g;
        o2[0] = r[0];
        o2[1] = r[1];
    }
}

inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// dgdm_icon_trace workspace: [mask | records | fetch flags]
struct IconLayout { size_t mask, rec, bad, bytes; };
IconLayout icon_layout(int M) {
    IconLayout L;
    L.mask = 0;
    L.rec = align256(sizeof(uint64_t) * MASK_WORDS * (size_t)M);
    L.bad = L.rec + align256(sizeof(TraceRec) * (size_t)M);
    L.bytes = L.bad + align256(sizeof(int32_t) * (size_t)M);
    return L;
}

// dgdm_icon_fetch_contours / dgdm_contour_resample workspace: [offsets | cumulative lengths]
struct ResampleLayout { size_t off, cum, bytes; };
ResampleLayout resample_layout(int M, int64_t total) {
    ResampleLayout L;
    L.off = 0;
    L.cum = align256(sizeof(int64_t) * (size_t)(M + 1));
    L.bytes = L.cum + align256(sizeof(double) * (size_t)total);
    return L;
}

constexpr int MAX_IMAGES = (int)(UINT32_MAX / SIZE / SIZE);    // binarise_kernel's grid has M * 128 * 128 threads

int check_offsets(const int64_t *off, int M, const char *fn, bool nonempty) {
    DGDM_REQUIRE(off && M >= 1, DGDM_EINVAL, "%s: need at least one contour and its offsets", fn);
    DGDM_REQUIRE(off[0] == 0, DGDM_EINVAL, "%s: offsets must start at 0", fn);
    for (int m = 0; m < M; ++m) {
        DGDM_REQUIRE(off[m + 1] >= off[m], DGDM_EINVAL, "%s: offsets of contour %d decrease", fn, m);
        DGDM_REQUIRE(!nonempty || off[m + 1] > off[m], DGDM_EINVAL, "%s: contour %d has no points", fn, m);
    }
    return DGDM_OK;
}

}  // namespace
}  // namespace dgdm

using namespace dgdm;

extern "C" int64_t dgdm_icon_workspace_bytes(int num_images) {
    DGDM_REQUIRE(num_images >= 1 && num_images <= MAX_IMAGES, DGDM_EINVAL, "dgdm_icon_workspace_bytes: %d images (need 1 .. %d)", num_images,
                 MAX_IMAGES);
    return (int64_t)icon_layout(num_images).bytes;
}

extern "C" int dgdm_icon_trace(const uint8_t *images_dev, int num_images, int height, int width, int channels, void *workspace_dev,
                               int64_t workspace_bytes, int64_t *num_points_host, void *stream) {
    const char *fn = "dgdm_icon_trace";
    DGDM_REQUIRE(images_dev && workspace_dev && num_points_host, DGDM_EINVAL, "%s: null argument", fn);
    DGDM_REQUIRE(num_images >= 1 && num_images <= MAX_IMAGES, DGDM_EINVAL, "%s: %d images (need 1 .. %d)", fn, num_images, MAX_IMAGES);
    DGDM_REQUIRE(height >= 1 && width >= 1, DGDM_EINVAL, "%s: image size %d x %d", fn, height, width);
    DGDM_REQUIRE(channels == 3 || channels == 4, DGDM_EINVAL, "%s: %d channels (need 3: BGR, or 4: BGRA)", fn, channels);
    DGDM_REQUIRE((int64_t)height * width * channels <= INT32_MAX, DGDM_EINVAL, "%s: image of %d x %d x %d bytes is too large", fn, height,
                 width, channels);
    const IconLayout L = icon_layout(num_images);
    DGDM_REQUIRE(workspace_bytes >= (int64_t)L.bytes, DGDM_EINVAL, "%s: workspace of %lld bytes, need %lld (dgdm_icon_workspace_bytes)", fn,
                 (long long)workspace_bytes, (long long)L.bytes);
    uint8_t *ws = static_cast<uint8_t *>(workspace_dev);
    uint64_t *mask = reinterpret_cast<uint64_t *>(ws + L.mask);
    TraceRec *rec = reinterpret_cast<TraceRec *>(ws + L.rec);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(binarise_kernel, dim3((unsigned)num_images * SIZE), dim3(SIZE), 0, s, images_dev, height, width, channels, mask);
    DGDM_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(trace_kernel, dim3((unsigned)num_images), dim3(64), 0, s, mask, rec);
    DGDM_HIP_CHECK(hipGetLastError());
    std::vector<TraceRec> R(num_images);
    DGDM_HIP_CHECK(hipMemcpyAsync(R.data(), rec, sizeof(TraceRec) * num_images, hipMemcpyDeviceToHost, s));
    DGDM_HIP_CHECK(hipStreamSynchronize(s));
    for (int m = 0; m < num_images; ++m) {
        DGDM_REQUIRE(!R[m].bad, DGDM_EINVAL, "%s: image %d: internal error, a border trace did not close", fn, m);
        DGDM_REQUIRE(R[m].n > 0, DGDM_EINVAL, "%s: image %d has no pixel with grey level <= 240 after the resize to 128 x 128 (no contour)", fn, m);
        num_points_host[m] = R[m].k;
    }
    return DGDM_OK;
}

extern "C" int dgdm_icon_fetch_contours(void *workspace_dev, int64_t workspace_bytes, int num_images, const int64_t *offsets_host,
                                        int32_t *points_dev, void *resample_workspace_dev, int64_t resample_workspace_bytes, void *stream) {
    const char *fn = "dgdm_icon_fetch_contours";
    DGDM_REQUIRE(workspace_dev && points_dev && resample_workspace_dev, DGDM_EINVAL, "%s: null argument", fn);
    DGDM_REQUIRE(num_images >= 1 && num_images <= MAX_IMAGES, DGDM_EINVAL, "%s: %d images (need 1 .. %d)", fn, num_images, MAX_IMAGES);
    int rc = check_offsets(offsets_host, num_images, fn, true);
    if (rc) return rc;
    const IconLayout L = icon_layout(num_images);
    DGDM_REQUIRE(workspace_bytes >= (int64_t)L.bytes, DGDM_EINVAL, "%s: workspace of %lld bytes, need %lld (dgdm_icon_workspace_bytes)", fn,
                 (long long)workspace_bytes, (long long)L.bytes);
    const ResampleLayout R = resample_layout(num_images, offsets_host[num_images]);
    DGDM_REQUIRE(resample_workspace_bytes >= (int64_t)R.bytes, DGDM_EINVAL,
                 "%s: resample workspace of %lld bytes, need %lld (dgdm_contour_resample_workspace_bytes)", fn, (long long)resample_workspace_bytes,
                 (long long)R.bytes);
    uint8_t *ws = static_cast<uint8_t *>(workspace_dev);
    int32_t *bad = reinterpret_cast<int32_t *>(ws + L.bad);
    int64_t *off = reinterpret_cast<int64_t *>(static_cast<uint8_t *>(resample_workspace_dev) + R.off);
    hipStream_t s = (hipStream_t)stream;
    DGDM_HIP_CHECK(hipMemcpyAsync(off, offsets_host, sizeof(int64_t) * (num_images + 1), hipMemcpyHostToDevice, s));
    DGDM_HIP_CHECK(hipMemsetAsync(bad, 0, sizeof(int32_t) * num_images, s));
    hipLaunchKernelGGL(fetch_kernel, dim3((unsigned)((num_images + 63) / 64)), dim3(64), 0, s, reinterpret_cast<const uint64_t *>(ws + L.mask),
                       reinterpret_cast<const TraceRec *>(ws + L.rec), off, num_images, points_dev, bad);
    DGDM_HIP_CHECK(hipGetLastError());
    std::vector<int32_t> B(num_images);
    DGDM_HIP_CHECK(hipMemcpyAsync(B.data(), bad, sizeof(int32_t) * num_images, hipMemcpyDeviceToHost, s));
    DGDM_HIP_CHECK(hipStreamSynchronize(s));        // also: the offsets' host buffer belongs to the caller, who may free it on return
    for (int m = 0; m < num_images; ++m)
        DGDM_REQUIRE(!B[m], DGDM_EINVAL, "%s: image %d: internal error, the winner's trace differs from the counting pass (offsets from "
                     "dgdm_icon_trace?)", fn, m);
    return DGDM_OK;
}

extern "C" int64_t dgdm_contour_resample_workspace_bytes(const int64_t *offsets_host, int num_contours) {
    if (check_offsets(offsets_host, num_contours, "dgdm_contour_resample_workspace_bytes", false)) return DGDM_EINVAL;
    return (int64_t)resample_layout(num_contours, offsets_host[num_contours]).bytes;
}

extern "C" int dgdm_contour_resample(const int32_t *points_dev, const int64_t *offsets_host, int num_contours, int num_out, int rescale,
                                     void *out_dev, void *workspace_dev, int64_t workspace_bytes, void *stream) {
    const char *fn = "dgdm_contour_resample";
    DGDM_REQUIRE(points_dev && out_dev && workspace_dev, DGDM_EINVAL, "%s: null argument", fn);
    int rc = check_offsets(offsets_host, num_contours, fn, true);
    if (rc) return rc;
    DGDM_REQUIRE(num_out >= 1, DGDM_EINVAL, "%s: num_points %d (need >= 1)", fn, num_out);
    DGDM_REQUIRE((int64_t)num_contours * num_out <= (int64_t)UINT32_MAX - 255, DGDM_EINVAL, "%s: %d x %d points exceed the launch grid", fn,
                 num_contours, num_out);
    const ResampleLayout L = resample_layout(num_contours, offsets_host[num_contours]);
    DGDM_REQUIRE(workspace_bytes >= (int64_t)L.bytes, DGDM_EINVAL, "%s: workspace of %lld bytes, need %lld (dgdm_contour_resample_workspace_bytes)",
                 fn, (long long)workspace_bytes, (long long)L.bytes);
    uint8_t *ws = static_cast<uint8_t *>(workspace_dev);
    int64_t *off = reinterpret_cast<int64_t *>(ws + L.off);
    double *cum = reinterpret_cast<double *>(ws + L.cum);
    hipStream_t s = (hipStream_t)stream;
    DGDM_HIP_CHECK(hipMemcpyAsync(off, offsets_host, sizeof(int64_t) * (num_contours + 1), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(cumlen_kernel, dim3((unsigned)((num_contours + 63) / 64)), dim3(64), 0, s, points_dev, off, num_contours, cum);
    DGDM_HIP_CHECK(hipGetLastError());
    const int64_t n_out = (int64_t)num_contours * num_out;
    hipLaunchKernelGGL(resample_kernel, dim3((unsigned)((n_out + 255) / 256)), dim3(256), 0, s, points_dev, off, cum, num_contours, num_out, rescale,
                       out_dev);
    DGDM_HIP_CHECK(hipGetLastError());
    DGDM_HIP_CHECK(hipStreamSynchronize(s));        // the offsets' host buffer belongs to the caller
    return DGDM_OK;
}

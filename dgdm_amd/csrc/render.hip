// Pictures of meshes: a batched z-buffer triangle rasteriser.  It stands where the reference calls MuJoCo's renderer
// (sim/render_mesh.py:render_mesh / render_object_mesh, dynamics/sim_test_mj_3d.py:99-106, 218-225); MuJoCo's lighting is not reproduced.
// The contract, exact in integers and unfused float32 operations, is include/dgdm_hip.h "mesh rendering" and DESIGN.md §4.5e;
// tests/render_oracle.py is its CPU statement.
//
// Launches of dgdm_render_meshes, all on the caller's stream (instances in view order, a view's triangles = its instances' in order):
//   1. project_kernel   one thread per (instance, vertex): the four row sums, three divisions, the snap to 1/256 pixel;
//   2. setup_kernel     one thread per (instance, triangle): index check, rejection, orientation, flat shade -> one 48-byte record;
//   3. raster_kernel    one workgroup per (view, 16 x 16 tile), one pixel per lane: the view's records in chunks of 256, each lane
//                       tests one record's bounding box against the tile, the survivors are compacted into LDS in index order
//                       (ballot + mbcnt), every lane walks the list.  Strictly-smaller depth wins, so order decides ties; every pixel
//                       of the image is written by exactly one lane: no atomics on the image, nothing to clear.
// The call reads one flag back (a triangle index outside its mesh): one stream synchronisation.
// This file is compiled with -ffp-contract=off (build.py): no operation of the contract is fused.
#include "common.h"
#include <algorithm>
#include <cmath>
#include <cstring>
#include <numeric>

namespace dgdm {
namespace {

constexpr int TILE = 16;                  // raster_kernel: 16 x 16 pixels, 256 lanes
constexpr int CHUNK = 256;                // records tested per pass, one per lane
constexpr int MAX_SIZE = 2048;            // W, H
constexpr int SUB = 256;                  // sub-pixel units per pixel (8 bits)
constexpr float SNAP_LIMIT = 1048576.f;   // |X|, |Y| < 2^20

struct Instance {                         // device copy of one instance, in view order
    float m[16];                          // row-major model -> (pixel x, pixel y, depth, w)
    float eye[3];                         // the eye in the instance's model frame
    float rgb[3];
    int32_t id, view;
    int32_t v0, nv;                       // its mesh: first vertex (row of verts), vertex count
    int32_t t0, nt;                       //           first triangle (row of tris), triangle count
};

struct Snapped { int32_t X, Y; float zs; int32_t ok; };       // 16 bytes: what project_kernel writes per (instance, vertex)

struct TriRec {                           // 48 bytes = three 16-byte loads
    int32_t x0, y0, x1, y1;
    int32_t x2, y2; float z0, z1;
    float z2; int32_t id; uint32_t rgb; int32_t live;
};
static_assert(sizeof(TriRec) == 48 && sizeof(Snapped) == 16, "record sizes");

// the instance that owns row g of a table with prefix offsets off[0 .. n]: the largest i with off[i] <= g
__device__ int owner(const int32_t *off, int n, int g) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = hi - (hi - lo) / 2;
        if (off[mid] <= g) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__global__ __launch_bounds__(256) void project_kernel(const float *verts, const Instance *inst, const int32_t *pv_off, int n_inst, int total,
                                                      Snapped *out) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= total) return;
    const int i = owner(pv_off, n_inst, g);
    const Instance &I = inst[i];
    const float *p = verts + 3 * (int64_t)(I.v0 + (g - pv_off[i]));
    const float x = p[0], y = p[1], z = p[2];
    float c[4];
    for (int r = 0; r < 4; ++r) c[r] = ((I.m[4 * r] * x + I.m[4 * r + 1] * y) + I.m[4 * r + 2] * z) + I.m[4 * r + 3];
    const float px = c[0] / c[3], py = c[1] / c[3], zs = c[2] / c[3];
    const float fx = rintf(px * (float)SUB), fy = rintf(py * (float)SUB);
    // !(a < b) is also true for a NaN
    const bool bad = !(c[3] > 0.f) || !(fabsf(c[3]) < INFINITY) || !(fabsf(fx) < SNAP_LIMIT) || !(fabsf(fy) < SNAP_LIMIT) || !(fabsf(zs) < INFINITY);
    Snapped s;
    s.X = bad ? 0 : (int32_t)fx;
    s.Y = bad ? 0 : (int32_t)fy;
    s.zs = zs;
    s.ok = bad ? 0 : 1;
    out[g] = s;
}

// s = 0.3 + 0.7 |n . d| / sqrt(|n|^2 |d|^2) in model coordinates, the triangle's vertices in file order; 0.3 for a degenerate one
__device__ float shade(const float *a, const float *b, const float *c, const float *eye) {
    const float e1[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]}, e2[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
    const float n[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
    float d[3];
    for (int k = 0; k < 3; ++k) d[k] = eye[k] - ((a[k] + b[k]) + c[k]) / 3.f;
    const float dot = (n[0] * d[0] + n[1] * d[1]) + n[2] * d[2];
    const float nn = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2], dd = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2];
    const float q = __fsqrt_rn(nn * dd);
    if (!(q > 0.f) || !(q < INFINITY)) return 0.3f;
    return 0.3f + 0.7f * fminf(fabsf(dot) / q, 1.f);
}

__global__ __launch_bounds__(256) void setup_kernel(const float *verts, const int32_t *tris, const Instance *inst, const int32_t *pv_off,
                                                    const int32_t *tr_off, int n_inst, int total, const Snapped *snapped, int want_rgb,
                                                    TriRec *rec, int32_t *rejected, int32_t *bad_index) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= total) return;
    const int i = owner(tr_off, n_inst, g);
    const Instance &I = inst[i];
    const int32_t *t = tris + 3 * (int64_t)(I.t0 + (g - tr_off[i]));
    const int i0 = t[0], i1 = t[1], i2 = t[2];
    TriRec R;
    memset(&R, 0, sizeof(R));
    if ((unsigned)i0 >= (unsigned)I.nv || (unsigned)i1 >= (unsigned)I.nv || (unsigned)i2 >= (unsigned)I.nv) {
        *bad_index = 1;                                    // every writer writes 1
        rec[g] = R;
        return;
    }
    const Snapped a = snapped[pv_off[i] + i0], b = snapped[pv_off[i] + i1], c = snapped[pv_off[i] + i2];
    if (!(a.ok && b.ok && c.ok)) {
        atomicAdd(rejected + I.view, 1);                   // an integer count: the same in any order
        rec[g] = R;
        return;
    }
    const int64_t A = (int64_t)(b.X - a.X) * (c.Y - a.Y) - (int64_t)(b.Y - a.Y) * (c.X - a.X);
    if (A == 0) {
        rec[g] = R;
        return;
    }
    const Snapped &v1 = A > 0 ? b : c, &v2 = A > 0 ? c : b;
    R.x0 = a.X; R.y0 = a.Y; R.z0 = a.zs;
    R.x1 = v1.X; R.y1 = v1.Y; R.z1 = v1.zs;
    R.x2 = v2.X; R.y2 = v2.Y; R.z2 = v2.zs;
    R.id = I.id;
    R.live = 1;
    if (want_rgb) {
        const float *V = verts + 3 * (int64_t)I.v0;
        const float s = shade(V + 3 * i0, V + 3 * i1, V + 3 * i2, I.eye);
        uint32_t packed = 0;
        for (int k = 0; k < 3; ++k) {
            const float v = rintf((I.rgb[k] * s) * 255.f);
            packed |= (uint32_t)fminf(fmaxf(v, 0.f), 255.f) << (8 * k);
        }
        R.rgb = packed;
    }
    rec[g] = R;
}

// E of sample (px, py) for the edge a -> b, and whether the sample is on the triangle's side of it (DESIGN.md §4.5e "coverage")
__device__ __forceinline__ bool edge(int xa, int ya, int xb, int yb, int px, int py, int64_t *E) {
    const int dx = xb - xa, dy = yb - ya;
    const int64_t e = (int64_t)dx * (py - ya) - (int64_t)dy * (px - xa);
    *E = e;
    return e > 0 || (e == 0 && (dy < 0 || (dy == 0 && dx > 0)));
}

// Grid (tiles_x * tiles_y, n_views), 256 lanes: lane = (ty << 4) | tx is pixel (16 tile_x + tx, 16 tile_y + ty) of view blockIdx.y.
__global__ __launch_bounds__(CHUNK) void raster_kernel(const TriRec *rec, const int32_t *view_tri, int W, int H, int tiles_x, int32_t *ids,
                                                       float *depth, uint8_t *rgb) {
    __shared__ int4 s_rec[CHUNK * 3];
    __shared__ int s_cnt[CHUNK / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int view = blockIdx.y;
    const int tile_x = blockIdx.x % tiles_x, tile_y = blockIdx.x / tiles_x;
    const int i = tile_x * TILE + (tid & (TILE - 1)), j = tile_y * TILE + (tid >> 4);
    const int px = SUB * i + SUB / 2, py = SUB * j + SUB / 2;
    // the tile's samples, in sub-pixel units (only those inside the image matter)
    const int sx_lo = SUB * (tile_x * TILE) + SUB / 2, sx_hi = SUB * min(tile_x * TILE + TILE - 1, W - 1) + SUB / 2;
    const int sy_lo = SUB * (tile_y * TILE) + SUB / 2, sy_hi = SUB * min(tile_y * TILE + TILE - 1, H - 1) + SUB / 2;
    const int begin = view_tri[view], end = view_tri[view + 1];
    float best_z = INFINITY;
    int32_t best_id = -1;
    uint32_t best_rgb = 0x00FFFFFFu;
    const int4 *rec4 = reinterpret_cast<const int4 *>(rec);
    for (int base = begin; base < end; base += CHUNK) {
        const int g = base + tid;
        int4 r0 = make_int4(0, 0, 0, 0), r1 = r0, r2 = r0;
        bool keep = false;
        if (g < end) {
            r0 = rec4[3 * (int64_t)g];
            r1 = rec4[3 * (int64_t)g + 1];
            r2 = rec4[3 * (int64_t)g + 2];
            const int x_lo = min(r0.x, min(r0.z, r1.x)), x_hi = max(r0.x, max(r0.z, r1.x));
            const int y_lo = min(r0.y, min(r0.w, r1.y)), y_hi = max(r0.y, max(r0.w, r1.y));
            keep = r2.w != 0 && x_lo <= sx_hi && x_hi >= sx_lo && y_lo <= sy_hi && y_hi >= sy_lo;
        }
        const uint64_t mask = __ballot(keep);
        const int rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0));
        if (lane == 0) s_cnt[wave] = __popcll(mask);
        __syncthreads();
        int before = 0, total = 0;
        for (int w = 0; w < CHUNK / 64; ++w) {
            const int c = s_cnt[w];
            before += w < wave ? c : 0;
            total += c;
        }
        if (keep) {
            const int k = before + rank;                  // < CHUNK: at most one survivor per lane
            s_rec[3 * k] = r0;
            s_rec[3 * k + 1] = r1;
            s_rec[3 * k + 2] = r2;
        }
        __syncthreads();
        for (int k = 0; k < total; ++k) {
            const int4 a = s_rec[3 * k], b = s_rec[3 * k + 1], c = s_rec[3 * k + 2];
            const int x0 = a.x, y0 = a.y, x1 = a.z, y1 = a.w, x2 = b.x, y2 = b.y;
            int64_t e01, e12, e20;
            const bool in01 = edge(x0, y0, x1, y1, px, py, &e01), in12 = edge(x1, y1, x2, y2, px, py, &e12), in20 = edge(x2, y2, x0, y0, px, py, &e20);
            if (in01 && in12 && in20) {
                const int64_t A = (int64_t)(x1 - x0) * (y2 - y0) - (int64_t)(y1 - y0) * (x2 - x0);
                const float z0 = __int_as_float(b.z), z1 = __int_as_float(b.w), z2 = __int_as_float(c.x);
                const float fA = (float)A, b1 = (float)e20 / fA, b2 = (float)e01 / fA;
                const float z = (z0 + b1 * (z1 - z0)) + b2 * (z2 - z0);
                if (z < best_z) {                          // strictly: at equal depth the earlier record stays
                    best_z = z;
                    best_id = c.y;
                    best_rgb = (uint32_t)c.z;
                }
            }
        }
        __syncthreads();                                   // s_rec / s_cnt are rewritten by the next chunk
    }
    if (i < W && j < H) {
        const int64_t o = ((int64_t)view * H + j) * W + i;
        ids[o] = best_id;
        depth[o] = best_z;
        if (rgb) {
            rgb[3 * o] = (uint8_t)(best_rgb & 255u);
            rgb[3 * o + 1] = (uint8_t)((best_rgb >> 8) & 255u);
            rgb[3 * o + 2] = (uint8_t)((best_rgb >> 16) & 255u);
        }
    }
}

inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// workspace: [instances | vertex prefix | triangle prefix | view triangle ranges | bad-index flag | snapped vertices | records]
struct Layout { size_t inst, pv_off, tr_off, view_tri, bad, snapped, rec, bytes; int64_t n_pv, n_tr; };

// Checks the mesh tables and the instances' mesh indices; fills the totals.
int layout(const int64_t *vo, const int64_t *to, int n_meshes, const int32_t *inst_mesh, int n_inst, int n_views, const char *fn, Layout *L) {
    DGDM_REQUIRE(vo && to && n_meshes >= 1, DGDM_EINVAL, "%s: need at least one mesh and both offset tables", fn);
    DGDM_REQUIRE(inst_mesh && n_inst >= 1, DGDM_EINVAL, "%s: need at least one instance", fn);
    DGDM_REQUIRE(n_views >= 1 && n_views <= 65535, DGDM_EINVAL, "%s: %d views (need 1 .. 65535)", fn, n_views);
    DGDM_REQUIRE(vo[0] == 0 && to[0] == 0, DGDM_EINVAL, "%s: offsets must start at 0", fn);
    for (int m = 0; m < n_meshes; ++m)
        DGDM_REQUIRE(vo[m + 1] >= vo[m] && to[m + 1] >= to[m], DGDM_EINVAL, "%s: offsets of mesh %d decrease", fn, m);
    DGDM_REQUIRE(vo[n_meshes] <= INT32_MAX / 4 && to[n_meshes] <= INT32_MAX / 4, DGDM_EINVAL, "%s: mesh tables too large", fn);
    int64_t n_pv = 0, n_tr = 0;
    for (int i = 0; i < n_inst; ++i) {
        const int m = inst_mesh[i];
        DGDM_REQUIRE(m >= 0 && m < n_meshes, DGDM_EINVAL, "%s: instance %d: mesh index %d outside 0 .. %d", fn, i, m, n_meshes - 1);
        n_pv += vo[m + 1] - vo[m];
        n_tr += to[m + 1] - to[m];
    }
    DGDM_REQUIRE(n_pv <= INT32_MAX / 4 && n_tr <= INT32_MAX / 4, DGDM_EINVAL, "%s: %lld instance vertices and %lld instance triangles are too many",
                 fn, (long long)n_pv, (long long)n_tr);
    L->n_pv = n_pv;
    L->n_tr = n_tr;
    L->inst = 0;
    L->pv_off = align256(sizeof(Instance) * (size_t)n_inst);
    L->tr_off = L->pv_off + align256(sizeof(int32_t) * (size_t)(n_inst + 1));
    L->view_tri = L->tr_off + align256(sizeof(int32_t) * (size_t)(n_inst + 1));
    L->bad = L->view_tri + align256(sizeof(int32_t) * (size_t)(n_views + 1));
    L->snapped = L->bad + align256(sizeof(int32_t));
    L->rec = L->snapped + align256(sizeof(Snapped) * (size_t)n_pv);
    L->bytes = L->rec + align256(sizeof(TriRec) * (size_t)n_tr);
    return DGDM_OK;
}

}  // namespace
}  // namespace dgdm

using namespace dgdm;

extern "C" int64_t dgdm_render_workspace_bytes(const int64_t *vert_offsets_host, const int64_t *tri_offsets_host, int n_meshes,
                                               const int32_t *inst_mesh_host, int n_inst, int n_views) {
    Layout L;
    if (layout(vert_offsets_host, tri_offsets_host, n_meshes, inst_mesh_host, n_inst, n_views, "dgdm_render_workspace_bytes", &L)) return DGDM_EINVAL;
    return (int64_t)L.bytes;
}

extern "C" int dgdm_render_meshes(const float *verts_dev, const int32_t *tris_dev, const int64_t *vert_offsets_host, const int64_t *tri_offsets_host,
                                  int n_meshes, const int32_t *inst_view_host, const int32_t *inst_mesh_host, const float *inst_matrix_host,
                                  const int32_t *inst_id_host, const float *inst_rgb_host, const float *inst_eye_host, int n_inst, int n_views,
                                  int width, int height, int32_t *ids_dev, float *depth_dev, uint8_t *rgb_dev, int32_t *rejected_dev,
                                  int32_t *snapped_dev, void *workspace_dev, int64_t workspace_bytes, void *stream) {
    const char *fn = "dgdm_render_meshes";
    DGDM_REQUIRE(verts_dev && tris_dev && ids_dev && depth_dev && rejected_dev && workspace_dev, DGDM_EINVAL, "%s: null argument", fn);
    DGDM_REQUIRE(inst_view_host && inst_matrix_host && inst_id_host, DGDM_EINVAL, "%s: null instance table", fn);
    DGDM_REQUIRE(!rgb_dev || (inst_rgb_host && inst_eye_host), DGDM_EINVAL, "%s: an rgb image needs the instances' colours and eyes", fn);
    DGDM_REQUIRE(width >= 1 && width <= MAX_SIZE && height >= 1 && height <= MAX_SIZE, DGDM_EINVAL, "%s: image of %d x %d (need 1 .. %d each)", fn,
                 width, height, MAX_SIZE);
    Layout L;
    int rc = layout(vert_offsets_host, tri_offsets_host, n_meshes, inst_mesh_host, n_inst, n_views, fn, &L);
    if (rc) return rc;
    DGDM_REQUIRE(workspace_bytes >= (int64_t)L.bytes, DGDM_EINVAL, "%s: workspace of %lld bytes, need %lld (dgdm_render_workspace_bytes)", fn,
                 (long long)workspace_bytes, (long long)L.bytes);
    for (int i = 0; i < n_inst; ++i)
        DGDM_REQUIRE(inst_view_host[i] >= 0 && inst_view_host[i] < n_views, DGDM_EINVAL, "%s: instance %d: view index %d outside 0 .. %d", fn, i,
                     inst_view_host[i], n_views - 1);
    // view order, the caller's order within a view: it decides ties
    std::vector<int> order(n_inst);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return inst_view_host[a] < inst_view_host[b]; });
    std::vector<Instance> inst(n_inst);
    std::vector<int32_t> pv_off(n_inst + 1, 0), tr_off(n_inst + 1, 0), view_tri(n_views + 1, 0);
    for (int k = 0; k < n_inst; ++k) {
        const int i = order[k], m = inst_mesh_host[i];
        Instance &I = inst[k];
        memcpy(I.m, inst_matrix_host + 16 * (size_t)i, sizeof(I.m));
        for (int c = 0; c < 3; ++c) {
            I.eye[c] = rgb_dev ? inst_eye_host[3 * (size_t)i + c] : 0.f;
            I.rgb[c] = rgb_dev ? inst_rgb_host[3 * (size_t)i + c] : 0.f;
        }
        I.id = inst_id_host[i];
        I.view = inst_view_host[i];
        I.v0 = (int32_t)vert_offsets_host[m];
        I.nv = (int32_t)(vert_offsets_host[m + 1] - vert_offsets_host[m]);
        I.t0 = (int32_t)tri_offsets_host[m];
        I.nt = (int32_t)(tri_offsets_host[m + 1] - tri_offsets_host[m]);
        pv_off[k + 1] = pv_off[k] + I.nv;
        tr_off[k + 1] = tr_off[k] + I.nt;
        view_tri[I.view + 1] += I.nt;
    }
    for (int v = 0; v < n_views; ++v) view_tri[v + 1] += view_tri[v];
    uint8_t *ws = static_cast<uint8_t *>(workspace_dev);
    Instance *d_inst = reinterpret_cast<Instance *>(ws + L.inst);
    int32_t *d_pv = reinterpret_cast<int32_t *>(ws + L.pv_off), *d_tr = reinterpret_cast<int32_t *>(ws + L.tr_off);
    int32_t *d_vt = reinterpret_cast<int32_t *>(ws + L.view_tri), *d_bad = reinterpret_cast<int32_t *>(ws + L.bad);
    Snapped *d_snap = reinterpret_cast<Snapped *>(ws + L.snapped);
    TriRec *d_rec = reinterpret_cast<TriRec *>(ws + L.rec);
    hipStream_t s = (hipStream_t)stream;
    // pageable host vectors: hipMemcpyAsync from them returns once the data is staged, and the call synchronises before they die
    DGDM_HIP_CHECK(hipMemcpyAsync(d_inst, inst.data(), sizeof(Instance) * n_inst, hipMemcpyHostToDevice, s));
    DGDM_HIP_CHECK(hipMemcpyAsync(d_pv, pv_off.data(), sizeof(int32_t) * (n_inst + 1), hipMemcpyHostToDevice, s));
    DGDM_HIP_CHECK(hipMemcpyAsync(d_tr, tr_off.data(), sizeof(int32_t) * (n_inst + 1), hipMemcpyHostToDevice, s));
    DGDM_HIP_CHECK(hipMemcpyAsync(d_vt, view_tri.data(), sizeof(int32_t) * (n_views + 1), hipMemcpyHostToDevice, s));
    DGDM_HIP_CHECK(hipMemsetAsync(d_bad, 0, sizeof(int32_t), s));
    DGDM_HIP_CHECK(hipMemsetAsync(rejected_dev, 0, sizeof(int32_t) * n_views, s));
    if (L.n_pv > 0) {
        hipLaunchKernelGGL(project_kernel, dim3((unsigned)((L.n_pv + 255) / 256)), dim3(256), 0, s, verts_dev, d_inst, d_pv, n_inst, (int)L.n_pv,
                           d_snap);
        DGDM_HIP_CHECK(hipGetLastError());
    }
    if (L.n_tr > 0) {
        hipLaunchKernelGGL(setup_kernel, dim3((unsigned)((L.n_tr + 255) / 256)), dim3(256), 0, s, verts_dev, tris_dev, d_inst, d_pv, d_tr, n_inst,
                           (int)L.n_tr, d_snap, rgb_dev ? 1 : 0, d_rec, rejected_dev, d_bad);
        DGDM_HIP_CHECK(hipGetLastError());
    }
    const int tiles_x = (width + TILE - 1) / TILE, tiles_y = (height + TILE - 1) / TILE;
    hipLaunchKernelGGL(raster_kernel, dim3((unsigned)(tiles_x * tiles_y), (unsigned)n_views), dim3(CHUNK), 0, s, d_rec, d_vt, width, height, tiles_x,
                       ids_dev, depth_dev, rgb_dev);
    DGDM_HIP_CHECK(hipGetLastError());
    if (snapped_dev && L.n_pv > 0) {
        // debug: row (view-ordered instance, vertex) = X, Y, the bits of zs, 1 when the vertex is kept
        DGDM_HIP_CHECK(hipMemcpyAsync(snapped_dev, d_snap, sizeof(Snapped) * (size_t)L.n_pv, hipMemcpyDeviceToDevice, s));
    }
    int32_t bad = 0;
    DGDM_HIP_CHECK(hipMemcpyAsync(&bad, d_bad, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    DGDM_HIP_CHECK(hipStreamSynchronize(s));
    DGDM_REQUIRE(!bad, DGDM_EINVAL, "%s: a triangle names a vertex outside its mesh (indices are local to the mesh, 0-based)", fn);
    return DGDM_OK;
}

// Designed fingers as watertight triangle meshes: the step after the decode (decode.hip), where the reference builds a trimesh per
// finger on the host (assets/finger_sampler.py:7-36 generate_finger_shape, assets/finger_3d.py:38-57 generate_3d_finger_mesh), exports
// it (save_gripper :52-64, save_3d_gripper :69-80) and hands the file to V-HACD for the collision pieces (dynamics/sim_test_mj.py:57-83).
//
//   topology   host, constant per (kind, n), cached: the triangle tables of include/dgdm_hip.h "finger meshes";
//   vertices   device, one thread per base point: the decoded ring / sheet (the expression of decode.h, so bit for bit the decode's
//              output) and its shifted copies, the shifts plain float32 adds;
//   statistics device, one wave per mesh: signed volume, area, smallest triangle area, count of triangles below an area epsilon - all
//              float64, lane partials folded by shuffles in a fixed order (no atomics: the result depends on the mesh alone);
//   pieces     device, one wave per finger: an exact convex decomposition of the same finger at a coarser resolution (sheared boxes between
//              knots of the ring / triangular prisms over the knot cells of the sheet) and how far the full-resolution base lies from it;
//   OBJ writer host.
// The kernels move a few kilobytes per finger; nothing here is tuned.
#include "common.h"
#include "decode.h"
#include <cerrno>
#include <cmath>
#include <cstring>
#include <map>
#include <mutex>

namespace dgdm {
namespace {

constexpr int WAVE = 64;

// ------------------------------------------------------------------------------------------------------------------ topology
inline void put_tri(std::vector<int32_t> &t, int64_t a, int64_t b, int64_t c) {
    t.push_back((int32_t)a); t.push_back((int32_t)b); t.push_back((int32_t)c);
}
inline void put_quad(std::vector<int32_t> &t, int64_t a, int64_t b, int64_t c, int64_t d) {      // (a, b, c), (a, c, d)
    put_tri(t, a, b, c);
    put_tri(t, a, c, d);
}

// local vertices of a 2-D piece: rings 0..3 at the lower knot, then rings 0..3 at the upper knot; the six quads of the full mesh for i = 0
std::vector<int32_t> piece2d_faces() {
    std::vector<int32_t> t;
    put_quad(t, 0, 4, 7, 3);     // left   (the curve side, -y)
    put_quad(t, 2, 6, 5, 1);     // right  (+y)
    put_quad(t, 3, 2, 1, 0);     // front  (-x)
    put_quad(t, 4, 5, 6, 7);     // back   (+x)
    put_quad(t, 2, 3, 7, 6);     // top    (+z)
    put_quad(t, 1, 5, 4, 0);     // bottom (-z)
    return t;
}

// local vertices of a 3-D piece: the triangle (0, 1, 2) on the sheet, (3, 4, 5) the same corners on the shifted sheet
std::vector<int32_t> piece3d_faces() {
    std::vector<int32_t> t;
    put_tri(t, 0, 1, 2);         // -y cap
    put_tri(t, 3, 5, 4);         // +y cap
    put_quad(t, 1, 0, 3, 4);
    put_quad(t, 2, 1, 4, 5);
    put_quad(t, 0, 2, 5, 3);
    return t;
}

std::vector<int32_t> mesh2d_faces(int64_t n) {
    std::vector<int32_t> t;
    t.reserve((size_t)(6 * (4 * (n - 1) + 2)));
    for (int64_t i = 0; i + 1 < n; ++i) put_quad(t, i, i + 1, i + 3 * n + 1, i + 3 * n);                     // left
    for (int64_t i = 0; i + 1 < n; ++i) put_quad(t, i + 2 * n, i + 2 * n + 1, i + n + 1, i + n);             // right
    put_quad(t, 3 * n, 2 * n, n, 0);                                                                        // front
    put_quad(t, n - 1, 2 * n - 1, 3 * n - 1, 4 * n - 1);                                                    // back
    for (int64_t i = 0; i + 1 < n; ++i) put_quad(t, i + 2 * n, i + 3 * n, i + 3 * n + 1, i + 2 * n + 1);     // top
    for (int64_t i = 0; i + 1 < n; ++i) put_quad(t, i + n, i + n + 1, i + 1, i);                             // bottom
    return t;
}

std::vector<int32_t> mesh3d_faces(int64_t n) {
    const int64_t N = n * n;
    std::vector<int32_t> t;
    t.reserve((size_t)(3 * (4 * (n - 1) * (n - 1) + 8 * (n - 1))));
    for (int side = 0; side < 2; ++side)
        for (int64_t a = 0; a + 1 < n; ++a)
            for (int64_t b = 0; b + 1 < n; ++b) {
                const int64_t p00 = a * n + b, p01 = p00 + 1, p10 = p00 + n, p11 = p10 + 1;
                if (side == 0) { put_tri(t, p00, p10, p11); put_tri(t, p00, p11, p01); }
                else { put_tri(t, N + p00, N + p11, N + p10); put_tri(t, N + p00, N + p01, N + p11); }
            }
    // the boundary loop: u = 0 with v rising, v = 1 with u rising, u = 1 with v falling, v = 0 with u falling
    std::vector<int64_t> loop;
    for (int64_t b = 0; b + 1 < n; ++b) loop.push_back(b);
    for (int64_t a = 0; a + 1 < n; ++a) loop.push_back(a * n + n - 1);
    for (int64_t b = n - 1; b > 0; --b) loop.push_back((n - 1) * n + b);
    for (int64_t a = n - 1; a > 0; --a) loop.push_back(a * n);
    for (size_t k = 0; k < loop.size(); ++k) {
        const int64_t c = loop[k], d = loop[(k + 1) % loop.size()];
        put_tri(t, c, d, d + N);
        put_tri(t, c, d + N, c + N);
    }
    return t;
}

std::mutex g_mu;
std::map<std::pair<int, int>, std::vector<int32_t>> g_faces;     // (kind, n) -> [T][3]

int mesh_counts(int kind, int n, int64_t *verts, int64_t *tris, const char *fn) {
    const bool piece = kind == DGDM_FINGER_PIECE_2D || kind == DGDM_FINGER_PIECE_3D;
    DGDM_REQUIRE(kind == DGDM_FINGER_MESH_2D || kind == DGDM_FINGER_MESH_3D || piece, DGDM_EINVAL,
                 "%s: kind %d (2: extruded 2-D finger, 3: 3-D finger, 12 / 13: one collision piece of either)", fn, kind);
    DGDM_REQUIRE(piece || n >= 2, DGDM_EINVAL, "%s: resolution %d (a mesh needs at least 2 points per direction)", fn, n);
    // int32 vertex indices: 4 n (2-D) and 2 n^2 (3-D) must stay below 2^31
    DGDM_REQUIRE(piece || (kind == DGDM_FINGER_MESH_2D ? n <= (1 << 28) : n <= 32767), DGDM_EINVAL, "%s: resolution %d too large for int32 indices", fn, n);
    const int64_t m = n - 1;
    switch (kind) {
    case DGDM_FINGER_MESH_2D: *verts = 4 * (int64_t)n; *tris = 2 * (4 * m + 2); break;
    case DGDM_FINGER_MESH_3D: *verts = 2 * (int64_t)n * n; *tris = 4 * m * m + 8 * m; break;
    case DGDM_FINGER_PIECE_2D: *verts = 8; *tris = 12; break;
    default: *verts = 6; *tris = 8; break;
    }
    return DGDM_OK;
}

// knot j of `pieces` over n samples: floor(j (n - 1) / pieces + 1/2)
__host__ __device__ inline int knot(int j, int n, int pieces) { return (int)((2 * (int64_t)j * (n - 1) + pieces) / (2 * (int64_t)pieces)); }

// ------------------------------------------------------------------------------------------------------------------ vertices
// verts [b][finger][4 n][3]: ring r of point p at row r n + p
__global__ void vertices2d_kernel(const float *__restrict__ samples, int B, int K, int n, const float *__restrict__ mat,
                                  const float *__restrict__ fixed, float scale, float offset, float width, float height, float *__restrict__ verts) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (int64_t)B * 2 * n) return;
    const int p = (int)(e % n);
    const int64_t bf = e / n;                          // b * 2 + finger
    const float x = fixed[p];
    const float y = decode_y(samples + bf * K, mat + (size_t)p * K, K, scale, offset);
    const float yw = add_rn(y, width), z0 = 0.f, z1 = height;                 // 0 + height
    float *o = verts + (bf * 4 * n + p) * 3;
    const int64_t ring = (int64_t)n * 3;
    o[0] = x; o[1] = y; o[2] = z0;
    o[ring] = x; o[ring + 1] = yw; o[ring + 2] = z0;
    o[2 * ring] = x; o[2 * ring + 1] = yw; o[2 * ring + 2] = z1;
    o[3 * ring] = x; o[3 * ring + 1] = y; o[3 * ring + 2] = z1;
}

// verts [b][finger][2 N][3], N = n^2: the sheet, then the sheet + width in y
__global__ void vertices3d_kernel(const float *__restrict__ samples, int B, int K, int N, const float *__restrict__ mat,
                                  const float *__restrict__ fixed, float scale, float offset, float width, float *__restrict__ verts) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (int64_t)B * 2 * N) return;
    const int p = (int)(e % N);
    const int64_t bf = e / N;
    const float x = fixed[2 * p], z = fixed[2 * p + 1];
    const float y = decode_y(samples + bf * K, mat + (size_t)p * K, K, scale, offset);
    float *o = verts + (bf * 2 * N + p) * 3;
    const int64_t sheet = (int64_t)N * 3;
    o[0] = x; o[1] = y; o[2] = z;
    o[sheet] = x; o[sheet + 1] = add_rn(y, width); o[sheet + 2] = z;
}

// ------------------------------------------------------------------------------------------------------------------ statistics
__device__ inline double wave_sum(double v) {
    for (int off = WAVE / 2; off > 0; off >>= 1) v += __shfl_down(v, off, WAVE);
    return v;
}
__device__ inline double wave_min(double v) {
    for (int off = WAVE / 2; off > 0; off >>= 1) v = fmin(v, __shfl_down(v, off, WAVE));
    return v;
}
__device__ inline double wave_max(double v) {
    for (int off = WAVE / 2; off > 0; off >>= 1) v = fmax(v, __shfl_down(v, off, WAVE));
    return v;
}

// one wave per mesh; lane l takes triangles l, l + 64, ... in order, then the 64 partials fold by halves
__global__ __launch_bounds__(WAVE) void stats_kernel(const float *__restrict__ verts, const int32_t *__restrict__ tris, int V, int T, double eps,
                                                     double *__restrict__ stats) {
    const int64_t mesh = blockIdx.x;
    const float *v = verts + mesh * V * 3;
    double vol = 0.0, area = 0.0, amin = INFINITY, small = 0.0, bad = 0.0;
    for (int t = threadIdx.x; t < T; t += WAVE) {
        const int32_t i0 = tris[3 * t], i1 = tris[3 * t + 1], i2 = tris[3 * t + 2];
        if (i0 < 0 || i1 < 0 || i2 < 0 || i0 >= V || i1 >= V || i2 >= V) { bad = 1.0; continue; }
        const double ax = v[3 * i0], ay = v[3 * i0 + 1], az = v[3 * i0 + 2];
        const double bx = v[3 * i1], by = v[3 * i1 + 1], bz = v[3 * i1 + 2];
        const double cx = v[3 * i2], cy = v[3 * i2 + 1], cz = v[3 * i2 + 2];
        // a . (b x c) / 6: the signed volume of the tetrahedron (origin, a, b, c)
        vol += (ax * (by * cz - bz * cy) + ay * (bz * cx - bx * cz) + az * (bx * cy - by * cx)) / 6.0;
        const double ux = bx - ax, uy = by - ay, uz = bz - az, wx = cx - ax, wy = cy - ay, wz = cz - az;
        const double nx = uy * wz - uz * wy, ny = uz * wx - ux * wz, nz = ux * wy - uy * wx;
        const double a = 0.5 * sqrt(nx * nx + ny * ny + nz * nz);
        area += a;
        amin = fmin(amin, a);
        if (a < eps) small += 1.0;
    }
    vol = wave_sum(vol); area = wave_sum(area); amin = wave_min(amin); small = wave_sum(small); bad = wave_max(bad);
    if (threadIdx.x == 0) {
        double *o = stats + mesh * 4;
        const bool ok = bad == 0.0;          // a triangle index outside the mesh: the mesh has no statistics
        o[0] = ok ? vol : NAN; o[1] = ok ? area : NAN; o[2] = ok ? amin : NAN; o[3] = ok ? small : NAN;
    }
}

// ------------------------------------------------------------------------------------------------------------------ pieces
__device__ inline void copy3(float *dst, const float *src) { dst[0] = src[0]; dst[1] = src[1]; dst[2] = src[2]; }

// one wave per finger; lane l takes pieces l, l + 64, ...: its 8 corners and the ring-0 samples strictly between its knots
__global__ __launch_bounds__(WAVE) void pieces2d_kernel(const float *__restrict__ verts, int n, int P, float *__restrict__ out, double *__restrict__ chord) {
    const int64_t bf = blockIdx.x;
    const float *v = verts + bf * 4 * n * 3;
    float *o = out + bf * P * 8 * 3;
    double err = 0.0;
    for (int k = threadIdx.x; k < P; k += WAVE) {
        const int i0 = knot(k, n, P), i1 = knot(k + 1, n, P);
        for (int r = 0; r < 4; ++r) {
            copy3(o + ((int64_t)k * 8 + r) * 3, v + ((int64_t)r * n + i0) * 3);
            copy3(o + ((int64_t)k * 8 + 4 + r) * 3, v + ((int64_t)r * n + i1) * 3);
        }
        const double x0 = v[3 * (int64_t)i0], y0 = v[3 * (int64_t)i0 + 1], x1 = v[3 * (int64_t)i1], y1 = v[3 * (int64_t)i1 + 1];
        for (int i = i0 + 1; i < i1; ++i) {
            const double x = v[3 * (int64_t)i], y = v[3 * (int64_t)i + 1];
            err = fmax(err, fabs(y - (y0 + (y1 - y0) * ((x - x0) / (x1 - x0)))));
        }
    }
    err = wave_max(err);
    if (threadIdx.x == 0) chord[bf] = err;
}

// one wave per finger; lane l takes knot cells l, l + 64, ... (cell = j pv + l): two prisms and the sheet samples the cell owns
__global__ __launch_bounds__(WAVE) void pieces3d_kernel(const float *__restrict__ verts, int n, int pu, int pv, float *__restrict__ out,
                                                        double *__restrict__ chord) {
    const int64_t bf = blockIdx.x, N = (int64_t)n * n;
    const float *v = verts + bf * 2 * N * 3;
    float *o = out + bf * 2 * pu * pv * 6 * 3;
    double err = 0.0;
    for (int c = threadIdx.x; c < pu * pv; c += WAVE) {
        const int j = c / pv, l = c - j * pv;
        const int a0 = knot(j, n, pu), a1 = knot(j + 1, n, pu), b0 = knot(l, n, pv), b1 = knot(l + 1, n, pv);
        const int64_t q00 = (int64_t)a0 * n + b0, q10 = (int64_t)a1 * n + b0, q11 = (int64_t)a1 * n + b1, q01 = (int64_t)a0 * n + b1;
        const int64_t corner[2][3] = {{q00, q10, q11}, {q00, q11, q01}};
        for (int h = 0; h < 2; ++h)
            for (int k = 0; k < 3; ++k) {
                float *dst = o + (((int64_t)2 * c + h) * 6 + k) * 3;
                copy3(dst, v + corner[h][k] * 3);
                copy3(dst + 9, v + (N + corner[h][k]) * 3);
            }
        const double x0 = v[3 * q00], z0 = v[3 * q00 + 2], x1 = v[3 * q10], z1 = v[3 * q01 + 2];
        const double y00 = v[3 * q00 + 1], y10 = v[3 * q10 + 1], y11 = v[3 * q11 + 1], y01 = v[3 * q01 + 1];
        const int a_end = j == pu - 1 ? a1 : a1 - 1, b_end = l == pv - 1 ? b1 : b1 - 1;      // the last cell of a row / column owns its far edge
        for (int a = a0; a <= a_end; ++a)
            for (int b = b0; b <= b_end; ++b) {
                if ((a == a0 || a == a1) && (b == b0 || b == b1)) continue;                 // a knot: on the coarse surface by construction
                const float *q = v + ((int64_t)a * n + b) * 3;
                const double s = ((double)q[0] - x0) / (x1 - x0), t = ((double)q[2] - z0) / (z1 - z0);
                const double yl = s >= t ? y00 + s * (y10 - y00) + t * (y11 - y10) : y00 + t * (y01 - y00) + s * (y11 - y01);
                err = fmax(err, fabs((double)q[1] - yl));
            }
    }
    err = wave_max(err);
    if (threadIdx.x == 0) chord[bf] = err;
}

}  // namespace
}  // namespace dgdm

using namespace dgdm;

extern "C" int dgdm_finger_mesh_counts(int kind, int n, int64_t *verts, int64_t *tris) {
    DGDM_REQUIRE(verts && tris, DGDM_EINVAL, "dgdm_finger_mesh_counts: null argument");
    return mesh_counts(kind, n, verts, tris, "dgdm_finger_mesh_counts");
}

extern "C" int dgdm_finger_mesh_faces(int kind, int n, int32_t *tris_host) {
    DGDM_REQUIRE(tris_host, DGDM_EINVAL, "dgdm_finger_mesh_faces: null argument");
    int64_t V, T;
    int rc = mesh_counts(kind, n, &V, &T, "dgdm_finger_mesh_faces");
    if (rc) return rc;
    if (kind == DGDM_FINGER_PIECE_2D || kind == DGDM_FINGER_PIECE_3D) n = 0;
    std::lock_guard<std::mutex> lk(g_mu);
    auto key = std::make_pair(kind, n);
    auto it = g_faces.find(key);
    if (it == g_faces.end()) {
        std::vector<int32_t> t = kind == DGDM_FINGER_MESH_2D ? mesh2d_faces(n) : kind == DGDM_FINGER_MESH_3D ? mesh3d_faces(n)
                                 : kind == DGDM_FINGER_PIECE_2D ? piece2d_faces() : piece3d_faces();
        DGDM_REQUIRE((int64_t)t.size() == 3 * T, DGDM_EINVAL, "dgdm_finger_mesh_faces: built %lld triangles, expected %lld", (long long)(t.size() / 3), (long long)T);
        it = g_faces.emplace(key, std::move(t)).first;
    }
    memcpy(tris_host, it->second.data(), it->second.size() * sizeof(int32_t));
    return DGDM_OK;
}

extern "C" int dgdm_finger_mesh_vertices_2d(const float *samples_dev, int batch, int num_ctrl, int num_points, float scale, float offset,
                                            float width, float height, float *verts_dev, void *stream) {
    DGDM_REQUIRE(samples_dev && verts_dev && batch >= 0, DGDM_EINVAL, "dgdm_finger_mesh_vertices_2d: null argument");
    DGDM_REQUIRE(num_ctrl >= 8 && num_ctrl % 2 == 0 && num_points >= 2 && num_points <= (1 << 28), DGDM_EINVAL,
                 "dgdm_finger_mesh_vertices_2d: %d control values (need an even number >= 8: not-a-knot needs 4 knots per finger), %d points (a mesh needs >= 2)",
                 num_ctrl, num_points);
    DGDM_REQUIRE(std::isfinite(width) && std::isfinite(height) && width > 0.f && height > 0.f, DGDM_EINVAL,
                 "dgdm_finger_mesh_vertices_2d: width %g, height %g (need both > 0)", (double)width, (double)height);
    if (batch == 0) return DGDM_OK;
    DecodeTable *t = nullptr;
    int rc;
    if ((rc = decode_table(2, num_ctrl / 2, num_points, &t))) return rc;
    const int64_t n = (int64_t)batch * 2 * t->npts;
    DGDM_REQUIRE((n + 255) / 256 <= (int64_t)INT32_MAX, DGDM_EINVAL, "dgdm_finger_mesh_vertices_2d: %lld points exceed the launch grid", (long long)n);
    hipLaunchKernelGGL(vertices2d_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, samples_dev, batch, t->K, t->npts,
                       t->mat.as<float>(), t->fixed.as<float>(), scale, offset, width, height, verts_dev);
    DGDM_HIP_CHECK(hipGetLastError());
    return DGDM_OK;
}

extern "C" int dgdm_finger_mesh_vertices_3d(const float *samples_dev, int batch, int num_ctrl, int sample_size, float scale, float offset,
                                            float width, float *verts_dev, void *stream) {
    DGDM_REQUIRE(samples_dev && verts_dev && batch >= 0, DGDM_EINVAL, "dgdm_finger_mesh_vertices_3d: null argument");
    DGDM_REQUIRE(num_ctrl == 42 && sample_size >= 2 && sample_size <= 32767, DGDM_EINVAL,
                 "dgdm_finger_mesh_vertices_3d: %d control values (the reference's net is 2 fingers x 7 x 3 = 42), sample_size %d (a mesh needs >= 2)",
                 num_ctrl, sample_size);
    DGDM_REQUIRE(std::isfinite(width) && width > 0.f, DGDM_EINVAL, "dgdm_finger_mesh_vertices_3d: width %g (need > 0)", (double)width);
    if (batch == 0) return DGDM_OK;
    DecodeTable *t = nullptr;
    int rc;
    if ((rc = decode_table(3, 21, sample_size, &t))) return rc;
    const int64_t n = (int64_t)batch * 2 * t->npts;
    DGDM_REQUIRE((n + 255) / 256 <= (int64_t)INT32_MAX, DGDM_EINVAL, "dgdm_finger_mesh_vertices_3d: %lld points exceed the launch grid", (long long)n);
    hipLaunchKernelGGL(vertices3d_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, samples_dev, batch, t->K, t->npts,
                       t->mat.as<float>(), t->fixed.as<float>(), scale, offset, width, verts_dev);
    DGDM_HIP_CHECK(hipGetLastError());
    return DGDM_OK;
}

extern "C" int dgdm_finger_mesh_stats(const float *verts_dev, const int32_t *tris_dev, int64_t meshes, int V, int T, double area_eps,
                                      double *stats_dev, void *stream) {
    DGDM_REQUIRE(verts_dev && tris_dev && stats_dev && meshes >= 0, DGDM_EINVAL, "dgdm_finger_mesh_stats: null argument");
    DGDM_REQUIRE(V >= 3 && T >= 1 && V <= INT32_MAX / 3 && T <= INT32_MAX / 3 && meshes <= INT32_MAX, DGDM_EINVAL,
                 "dgdm_finger_mesh_stats: %lld meshes of %d vertices and %d triangles", (long long)meshes, V, T);
    DGDM_REQUIRE(area_eps >= 0.0, DGDM_EINVAL, "dgdm_finger_mesh_stats: area epsilon %g (need >= 0)", area_eps);
    if (meshes == 0) return DGDM_OK;
    hipLaunchKernelGGL(stats_kernel, dim3((unsigned)meshes), dim3(WAVE), 0, (hipStream_t)stream, verts_dev, tris_dev, V, T, area_eps, stats_dev);
    DGDM_HIP_CHECK(hipGetLastError());
    return DGDM_OK;
}

extern "C" int dgdm_finger_pieces_2d(const float *verts_dev, int batch, int num_points, int pieces, float *out_dev, double *chord_err_dev, void *stream) {
    DGDM_REQUIRE(verts_dev && out_dev && chord_err_dev && batch >= 0, DGDM_EINVAL, "dgdm_finger_pieces_2d: null argument");
    DGDM_REQUIRE(num_points >= 2 && num_points <= (1 << 28), DGDM_EINVAL, "dgdm_finger_pieces_2d: %d points (a mesh needs >= 2)", num_points);
    DGDM_REQUIRE(pieces >= 1 && pieces <= num_points - 1, DGDM_EINVAL, "dgdm_finger_pieces_2d: %d pieces over %d segments (need 1 .. segments)", pieces,
                 num_points - 1);
    DGDM_REQUIRE(pieces <= 1000, DGDM_EINVAL, "dgdm_finger_pieces_2d: %d pieces (at most 1000: the files are numbered %%03d)", pieces);
    DGDM_REQUIRE(batch <= INT32_MAX / 2, DGDM_EINVAL, "dgdm_finger_pieces_2d: batch %d exceeds the launch grid", batch);
    if (batch == 0) return DGDM_OK;
    hipLaunchKernelGGL(pieces2d_kernel, dim3((unsigned)batch * 2), dim3(WAVE), 0, (hipStream_t)stream, verts_dev, num_points, pieces, out_dev, chord_err_dev);
    DGDM_HIP_CHECK(hipGetLastError());
    return DGDM_OK;
}

extern "C" int dgdm_finger_pieces_3d(const float *verts_dev, int batch, int sample_size, int pu, int pv, float *out_dev, double *chord_err_dev,
                                     void *stream) {
    DGDM_REQUIRE(verts_dev && out_dev && chord_err_dev && batch >= 0, DGDM_EINVAL, "dgdm_finger_pieces_3d: null argument");
    DGDM_REQUIRE(sample_size >= 2 && sample_size <= 32767, DGDM_EINVAL, "dgdm_finger_pieces_3d: sample_size %d (a mesh needs >= 2)", sample_size);
    DGDM_REQUIRE(pu >= 1 && pv >= 1 && pu <= sample_size - 1 && pv <= sample_size - 1, DGDM_EINVAL,
                 "dgdm_finger_pieces_3d: %d x %d knot cells over %d x %d sample cells (need 1 .. cells in each direction)", pu, pv, sample_size - 1,
                 sample_size - 1);
    DGDM_REQUIRE(2 * (int64_t)pu * pv <= 1000, DGDM_EINVAL, "dgdm_finger_pieces_3d: %lld pieces (at most 1000: the files are numbered %%03d)",
                 (long long)(2 * (int64_t)pu * pv));
    DGDM_REQUIRE(batch <= INT32_MAX / 2, DGDM_EINVAL, "dgdm_finger_pieces_3d: batch %d exceeds the launch grid", batch);
    if (batch == 0) return DGDM_OK;
    hipLaunchKernelGGL(pieces3d_kernel, dim3((unsigned)batch * 2), dim3(WAVE), 0, (hipStream_t)stream, verts_dev, sample_size, pu, pv, out_dev, chord_err_dev);
    DGDM_HIP_CHECK(hipGetLastError());
    return DGDM_OK;
}

extern "C" int dgdm_mesh_write_obj(const char *path, const float *verts_host, int64_t V, const int32_t *tris_host, int64_t T) {
    DGDM_REQUIRE(path && verts_host && tris_host, DGDM_EINVAL, "dgdm_mesh_write_obj: null argument");
    DGDM_REQUIRE(V >= 1 && T >= 1 && V <= INT32_MAX, DGDM_EINVAL, "dgdm_mesh_write_obj: %lld vertices, %lld triangles (need at least one of each)",
                 (long long)V, (long long)T);
    for (int64_t i = 0; i < 3 * T; ++i)
        DGDM_REQUIRE(tris_host[i] >= 0 && tris_host[i] < V, DGDM_EINVAL, "dgdm_mesh_write_obj: triangle %lld refers to vertex %d of %lld", (long long)(i / 3),
                     tris_host[i], (long long)V);
    std::string text;
    text.reserve((size_t)V * 48 + (size_t)T * 24);
    char line[128];
    for (int64_t i = 0; i < V; ++i) {        // 9 significant digits: the shortest count that names every binary32 value uniquely
        const int len = snprintf(line, sizeof line, "v %.9g %.9g %.9g\n", (double)verts_host[3 * i], (double)verts_host[3 * i + 1], (double)verts_host[3 * i + 2]);
        text.append(line, (size_t)len);
    }
    for (int64_t i = 0; i < T; ++i) {
        const int len = snprintf(line, sizeof line, "f %d %d %d\n", tris_host[3 * i] + 1, tris_host[3 * i + 1] + 1, tris_host[3 * i + 2] + 1);
        text.append(line, (size_t)len);
    }
    FILE *f = fopen(path, "wb");
    if (!f) {
        set_error("%s: cannot open for writing: %s", path, strerror(errno));
        return DGDM_EINVAL;
    }
    const bool ok = fwrite(text.data(), 1, text.size(), f) == text.size();
    if (fclose(f) != 0 || !ok) {
        set_error("%s: write error: %s", path, strerror(errno));
        return DGDM_EINVAL;
    }
    return DGDM_OK;
}

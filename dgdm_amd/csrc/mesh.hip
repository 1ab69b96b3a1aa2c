// Object point clouds from scanned meshes: the reference's sample_pts_from_mesh (dynamics/utils.py:14-18), called for the test objects
// of guided sampling (generator/train.py:100-109) and once per object name in dynamics training (dynamics/dataloader.py:57-63).
//
// Reader (host): OBJ vertex positions and triangles in file order (faces with more than three corners fan-triangulated).
// Sampler (device), after open3d's TriangleMesh::SamplePointsUniformlyImpl:
//   a_t = 0.5 |(v1 - v0) x (v2 - v0)|, A = sum a_t, cdf_t = running sum of a_t / A, n_t = round_half_away(cdf_t N);
//   triangle t owns the output points n_{t-1} <= p < n_t; point p = (1 - sqrt r1) v0 + sqrt r1 (1 - r2) v1 + sqrt r1 r2 v2.
// open3d draws r1, r2 from an unseeded global generator; here they are Philox4x64-10 outputs 2p and 2p + 1 under key
// (seed, mesh_key), so that a point depends on nothing but its mesh, its index and the key (DESIGN.md "Object clouds from meshes").
// Everything is float64.
//
// Launches of dgdm_mesh_sample_points, all on the caller's stream:
//   1. area_kernel      one workgroup per chunk of 1024 triangles (chunks start at each mesh's own first triangle): the areas and the
//                       chunk's total (the last element of the same block scan kernel 3 runs);
//   2. chunk_scan_kernel one thread per mesh: exclusive running sum of its chunk totals, in chunk order, and A;
//   3. count_kernel     one workgroup per chunk: the block scan again, + the chunk's prefix, / A, -> int64 n_t;
//   4. sample_kernel    one thread per (mesh, point): binary search for the owning triangle, Philox, barycentric point.
// 1-3 are the three phases of a reduce-then-scan: no workgroup waits for another, and the result depends on the mesh alone.  A is read
// back after 3 (the call synchronises once) so that a mesh without area fails before anything is sampled.
#include "common.h"
#include "philox.h"
#include <algorithm>
#include <cerrno>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <memory>

struct DgdmMesh {
    std::vector<double> verts;    // [V][3]
    std::vector<int32_t> tris;    // [T][3], 0-based
};

namespace dgdm {
namespace {

// ------------------------------------------------------------------------------------------------------------------ OBJ reader
struct LineReader {
    const char *path;
    int line = 0;
    int fail(const char *reason) {
        set_error("%s:%d: %s", path, line, reason);
        return DGDM_EINVAL;
    }
};

inline bool is_space(char c) { return c == ' ' || c == '\t' || c == '\r' || c == '\v' || c == '\f'; }

// Next whitespace-separated token of [*p, end): sets tok/len and advances *p; false at the end of the line.
bool next_token(const char **p, const char *end, const char **tok, size_t *len) {
    const char *s = *p;
    while (s < end && is_space(*s)) ++s;
    if (s == end) { *p = s; return false; }
    const char *e = s;
    while (e < end && !is_space(*e)) ++e;
    *tok = s; *len = (size_t)(e - s); *p = e;
    return true;
}

bool parse_double(const char *tok, size_t len, double *out) {
    char buf[128];
    if (len == 0 || len >= sizeof buf) return false;
    memcpy(buf, tok, len);
    buf[len] = 0;
    char *e = nullptr;
    errno = 0;
    *out = strtod(buf, &e);
    return e == buf + len && errno != ERANGE;
}

// The vertex index of a face token `i`, `i/j`, `i//k` or `i/j/k` (the texture / normal indices are not read).
bool parse_index(const char *tok, size_t len, long long *out) {
    char buf[64];
    size_t n = 0;
    while (n < len && tok[n] != '/') ++n;
    if (n == 0 || n >= sizeof buf) return false;
    memcpy(buf, tok, n);
    buf[n] = 0;
    char *e = nullptr;
    errno = 0;
    *out = strtoll(buf, &e, 10);
    return e == buf + n && errno != ERANGE;
}

int read_obj(const char *path, DgdmMesh *m) {
    LineReader r{path};
    FILE *f = fopen(path, "rb");
    if (!f) {
        set_error("%s: cannot open: %s", path, strerror(errno));
        return DGDM_EINVAL;
    }
    std::string text;
    char chunk[1 << 16];
    size_t got;
    while ((got = fread(chunk, 1, sizeof chunk, f)) > 0) text.append(chunk, got);
    const bool read_error = ferror(f) != 0;
    fclose(f);
    if (read_error) {
        set_error("%s: read error", path);
        return DGDM_EINVAL;
    }
    // positive indices may refer to vertices defined further down: checked against the final count, with the face's line
    std::vector<std::pair<long long, int>> forward;      // (largest index, line)
    std::vector<long long> face;
    const char *p = text.data(), *end = text.data() + text.size();
    while (p < end) {
        const char *eol = (const char *)memchr(p, '\n', (size_t)(end - p));
        if (!eol) eol = end;
        ++r.line;
        const char *q = p, *tok;
        size_t len;
        p = eol < end ? eol + 1 : end;
        if (!next_token(&q, eol, &tok, &len) || tok[0] == '#') continue;
        if (len == 1 && tok[0] == 'v') {
            double x[3];
            for (int k = 0; k < 3; ++k) {
                if (!next_token(&q, eol, &tok, &len)) return r.fail("vertex with fewer than 3 coordinates");
                if (!parse_double(tok, len, &x[k])) return r.fail("unparsable number");
            }
            m->verts.insert(m->verts.end(), x, x + 3);            // trailing w or colour values are ignored
        } else if (len == 1 && tok[0] == 'f') {
            const long long nv = (long long)(m->verts.size() / 3);
            face.clear();
            long long hi = -1;
            while (next_token(&q, eol, &tok, &len) && tok[0] != '#') {
                long long i;
                if (!parse_index(tok, len, &i)) return r.fail("unparsable number");
                if (i == 0) return r.fail("vertex index 0 (OBJ indices start at 1)");
                if (i < 0) {
                    if (-i > nv) return r.fail("relative vertex index out of range");
                    i = nv + i;
                } else {
                    i -= 1;
                    if (i > INT32_MAX - 1) return r.fail("vertex index out of range");
                    if (i >= nv && i > hi) hi = i;
                }
                face.push_back(i);
            }
            if (face.size() < 3) return r.fail("face with fewer than 3 vertices");
            if (hi >= 0) forward.emplace_back(hi, r.line);
            for (size_t k = 1; k + 1 < face.size(); ++k) {       // fan: (v0, vk, vk+1)
                m->tris.push_back((int32_t)face[0]);
                m->tris.push_back((int32_t)face[k]);
                m->tris.push_back((int32_t)face[k + 1]);
            }
        }
        // every other statement (vt, vn, vp, o, g, s, usemtl, mtllib, l, p, ...) is ignored
    }
    const long long nv = (long long)(m->verts.size() / 3);
    for (auto &fw : forward)
        if (fw.first >= nv) {
            r.line = fw.second;
            return r.fail("vertex index out of range");
        }
    if (m->tris.empty()) {
        set_error("%s:%d: no faces", path, r.line);
        return DGDM_EINVAL;
    }
    return DGDM_OK;
}

// ------------------------------------------------------------------------------------------------------------------ sampler
constexpr int SCAN_THREADS = 256, SCAN_ITEMS = 4, CHUNK = SCAN_THREADS * SCAN_ITEMS;

// Inclusive scan of the 1024 values a workgroup holds (4 consecutive values per thread), in a fixed order: every thread's own four
// serially, then Hillis-Steele over the 256 thread totals.  Kernels 1 and 3 both call it, so the chunk total of kernel 1 is bit for bit
// the last inclusive value of kernel 3 and the counts never decrease across a chunk boundary.
__device__ void block_scan(double v[SCAN_ITEMS], double *lds) {
    for (int j = 1; j < SCAN_ITEMS; ++j) v[j] += v[j - 1];
    const int tid = threadIdx.x;
    double x = v[SCAN_ITEMS - 1];
    lds[tid] = x;
    __syncthreads();
    for (int off = 1; off < SCAN_THREADS; off <<= 1) {
        const double y = tid >= off ? lds[tid - off] : 0.0;
        __syncthreads();
        x += y;
        lds[tid] = x;
        __syncthreads();
    }
    const double before = tid > 0 ? lds[tid - 1] : 0.0;
    for (int j = 0; j < SCAN_ITEMS; ++j) v[j] += before;
}

struct ChunkDesc {
    int64_t first;    // global index of the chunk's first triangle
    int32_t count;    // triangles in the chunk (<= CHUNK)
    int32_t mesh;
};

__device__ double tri_area(const double *verts, const int32_t *tris, int64_t vo, int64_t nv, int64_t t, int32_t *bad) {
    const int32_t i0 = tris[3 * t], i1 = tris[3 * t + 1], i2 = tris[3 * t + 2];
    if (i0 < 0 || i1 < 0 || i2 < 0 || i0 >= nv || i1 >= nv || i2 >= nv) {
        *bad = 1;
        return 0.0;
    }
    const double *a = verts + 3 * (vo + i0), *b = verts + 3 * (vo + i1), *c = verts + 3 * (vo + i2);
    const double ux = b[0] - a[0], uy = b[1] - a[1], uz = b[2] - a[2];
    const double wx = c[0] - a[0], wy = c[1] - a[1], wz = c[2] - a[2];
    const double cx = uy * wz - uz * wy, cy = uz * wx - ux * wz, cz = ux * wy - uy * wx;
    return 0.5 * sqrt(cx * cx + cy * cy + cz * cz);
}

__global__ __launch_bounds__(SCAN_THREADS) void area_kernel(const double *verts, const int32_t *tris, const int64_t *vert_off,
                                                            const ChunkDesc *chunks, double *area, double *chunk_total, int32_t *bad) {
    __shared__ double lds[SCAN_THREADS];
    const ChunkDesc c = chunks[blockIdx.x];
    const int64_t vo = vert_off[c.mesh], nv = vert_off[c.mesh + 1] - vo;
    double v[SCAN_ITEMS];
    for (int j = 0; j < SCAN_ITEMS; ++j) {
        const int k = threadIdx.x * SCAN_ITEMS + j;
        v[j] = 0.0;
        if (k < c.count) {
            v[j] = tri_area(verts, tris, vo, nv, c.first + k, bad + c.mesh);
            area[c.first + k] = v[j];
        }
    }
    block_scan(v, lds);
    if (threadIdx.x == SCAN_THREADS - 1) chunk_total[blockIdx.x] = v[SCAN_ITEMS - 1];
}

__global__ void chunk_scan_kernel(const int64_t *chunk_off, int n_meshes, double *chunk_prefix, const double *chunk_total, double *total) {
    const int m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= n_meshes) return;
    double s = 0.0;
    for (int64_t c = chunk_off[m]; c < chunk_off[m + 1]; ++c) {
        chunk_prefix[c] = s;
        s += chunk_total[c];
    }
    total[m] = s;
}

__global__ __launch_bounds__(SCAN_THREADS) void count_kernel(const ChunkDesc *chunks, const double *area, const double *chunk_prefix,
                                                             const double *total, double n_points, int64_t *counts) {
    __shared__ double lds[SCAN_THREADS];
    const ChunkDesc c = chunks[blockIdx.x];
    double v[SCAN_ITEMS];
    for (int j = 0; j < SCAN_ITEMS; ++j) {
        const int k = threadIdx.x * SCAN_ITEMS + j;
        v[j] = k < c.count ? area[c.first + k] : 0.0;
    }
    block_scan(v, lds);
    const double A = total[c.mesh], P = chunk_prefix[blockIdx.x];
    for (int j = 0; j < SCAN_ITEMS; ++j) {
        const int k = threadIdx.x * SCAN_ITEMS + j;
        if (k < c.count) counts[c.first + k] = A > 0.0 ? (int64_t)round((P + v[j]) / A * n_points) : 0;
    }
}

// Philox4x64-10: philox.h, shared with the scheduler step's noise.
__global__ void sample_kernel(const double *verts, const int32_t *tris, const int64_t *vert_off, const int64_t *tri_off, const uint64_t *keys,
                              uint64_t seed, const int64_t *counts, int64_t n_points, int64_t total, double *out) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= total) return;
    const int64_t m = g / n_points, p = g - m * n_points;
    // owner: the first triangle of the mesh whose count exceeds p (counts never decrease; the last one is n_points)
    int64_t lo = tri_off[m], hi = tri_off[m + 1] - 1;
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (counts[mid] > p) hi = mid; else lo = mid + 1;
    }
    // numpy.random.Philox(key=[seed, key]).random_raw() outputs 2p, 2p + 1: block counter p / 2 + 1 (numpy counts up before a block)
    const U64x4 r = philox4x64_10(U64x4{{(uint64_t)(p / 2) + 1, 0, 0, 0}}, seed, keys[m]);
    const int lane = 2 * (int)(p & 1);
    const double r1 = (double)(r.v[lane] >> 11) * 0x1.0p-53, r2 = (double)(r.v[lane + 1] >> 11) * 0x1.0p-53;
    const double s = sqrt(r1), a = 1.0 - s, b = s * (1.0 - r2), c = s * r2;
    const int64_t vo = vert_off[m];
    const double *v0 = verts + 3 * (vo + tris[3 * lo]), *v1 = verts + 3 * (vo + tris[3 * lo + 1]), *v2 = verts + 3 * (vo + tris[3 * lo + 2]);
    double *o = out + 3 * g;
    for (int k = 0; k < 3; ++k) o[k] = a * v0[k] + b * v1[k] + c * v2[k];
}

// Workspace layout for a batch (each piece 256-byte aligned).
struct Layout {
    size_t area, counts, chunks, chunk_total, chunk_prefix, chunk_off, vert_off, tri_off, keys, total, bad, bytes;
};

inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

Layout layout(int64_t n_tris, int64_t n_chunks, int n_meshes) {
    Layout L;
    size_t o = 0;
    auto put = [&](size_t bytes) { const size_t at = o; o = align256(o + bytes); return at; };
    L.area = put(sizeof(double) * n_tris);
    L.counts = put(sizeof(int64_t) * n_tris);
    L.chunk_total = put(sizeof(double) * n_chunks);
    L.chunk_prefix = put(sizeof(double) * n_chunks);
    L.total = put(sizeof(double) * n_meshes);
    L.bad = put(sizeof(int32_t) * n_meshes);
    // uploaded from the host in one copy: chunks .. keys are contiguous
    L.chunks = put(sizeof(ChunkDesc) * n_chunks);
    L.chunk_off = put(sizeof(int64_t) * (n_meshes + 1));
    L.vert_off = put(sizeof(int64_t) * (n_meshes + 1));
    L.tri_off = put(sizeof(int64_t) * (n_meshes + 1));
    L.keys = put(sizeof(uint64_t) * n_meshes);
    L.bytes = o;
    return L;
}

int check_offsets(const int64_t *tri_off, int n_meshes, int64_t *n_chunks, const char *fn) {
    DGDM_REQUIRE(tri_off && n_meshes >= 1, DGDM_EINVAL, "%s: need at least one mesh and its triangle offsets", fn);
    DGDM_REQUIRE(tri_off[0] == 0, DGDM_EINVAL, "%s: triangle offsets must start at 0", fn);
    int64_t c = 0;
    for (int m = 0; m < n_meshes; ++m) {
        DGDM_REQUIRE(tri_off[m + 1] >= tri_off[m], DGDM_EINVAL, "%s: triangle offsets of mesh %d decrease", fn, m);
        c += (tri_off[m + 1] - tri_off[m] + CHUNK - 1) / CHUNK;
    }
    *n_chunks = c;
    return DGDM_OK;
}

}  // namespace
}  // namespace dgdm

using namespace dgdm;

extern "C" int dgdm_mesh_read_obj(const char *path, DgdmMesh **out) {
    DGDM_REQUIRE(path && out, DGDM_EINVAL, "dgdm_mesh_read_obj: null argument");
    *out = nullptr;
    std::unique_ptr<DgdmMesh> m(new DgdmMesh);
    int rc = read_obj(path, m.get());
    if (rc) return rc;
    *out = m.release();
    return DGDM_OK;
}

extern "C" int64_t dgdm_mesh_num_vertices(const DgdmMesh *m) { return m ? (int64_t)(m->verts.size() / 3) : -1; }
extern "C" int64_t dgdm_mesh_num_triangles(const DgdmMesh *m) { return m ? (int64_t)(m->tris.size() / 3) : -1; }

extern "C" int dgdm_mesh_copy(const DgdmMesh *m, double *verts_host, int32_t *tris_host) {
    DGDM_REQUIRE(m && verts_host && tris_host, DGDM_EINVAL, "dgdm_mesh_copy: null argument");
    memcpy(verts_host, m->verts.data(), m->verts.size() * sizeof(double));
    memcpy(tris_host, m->tris.data(), m->tris.size() * sizeof(int32_t));
    return DGDM_OK;
}

extern "C" void dgdm_mesh_destroy(DgdmMesh *m) { delete m; }

extern "C" int64_t dgdm_mesh_sample_workspace_bytes(const int64_t *tri_offsets_host, int num_meshes) {
    int64_t n_chunks = 0;
    if (check_offsets(tri_offsets_host, num_meshes, &n_chunks, "dgdm_mesh_sample_workspace_bytes")) return DGDM_EINVAL;
    return (int64_t)layout(tri_offsets_host[num_meshes], n_chunks, num_meshes).bytes;
}

extern "C" int dgdm_mesh_sample_points(const double *verts_dev, const int32_t *tris_dev, const int64_t *vert_offsets_host,
                                       const int64_t *tri_offsets_host, int num_meshes, uint64_t seed, const uint64_t *keys_host,
                                       int64_t num_points, double *out_dev, void *workspace_dev, int64_t workspace_bytes, void *stream) {
    const char *fn = "dgdm_mesh_sample_points";
    int64_t n_chunks = 0;
    int rc = check_offsets(tri_offsets_host, num_meshes, &n_chunks, fn);
    if (rc) return rc;
    DGDM_REQUIRE(verts_dev && tris_dev && vert_offsets_host && keys_host && out_dev && workspace_dev, DGDM_EINVAL, "%s: null argument", fn);
    DGDM_REQUIRE(num_points >= 1, DGDM_EINVAL, "%s: num_points %lld (need >= 1)", fn, (long long)num_points);
    DGDM_REQUIRE(vert_offsets_host[0] == 0, DGDM_EINVAL, "%s: vertex offsets must start at 0", fn);
    for (int m = 0; m < num_meshes; ++m)
        DGDM_REQUIRE(vert_offsets_host[m + 1] >= vert_offsets_host[m], DGDM_EINVAL, "%s: vertex offsets of mesh %d decrease", fn, m);
    const int64_t n_tris = tri_offsets_host[num_meshes];
    const Layout L = layout(n_tris, n_chunks, num_meshes);
    DGDM_REQUIRE(workspace_bytes >= (int64_t)L.bytes, DGDM_EINVAL, "%s: workspace of %lld bytes, need %lld (dgdm_mesh_sample_workspace_bytes)", fn,
                 (long long)workspace_bytes, (long long)L.bytes);
    // a launch has fewer than 2^32 threads
    DGDM_REQUIRE(n_chunks <= (int64_t)(UINT32_MAX / SCAN_THREADS) && num_points <= (int64_t)(UINT32_MAX - 255) / num_meshes, DGDM_EINVAL,
                 "%s: %lld chunks / %d x %lld points exceed the launch grid", fn, (long long)n_chunks, num_meshes, (long long)num_points);
    // descriptors: host image of [chunks .. keys], one upload
    std::vector<uint8_t> host(L.bytes - L.chunks, 0);
    {
        ChunkDesc *cd = reinterpret_cast<ChunkDesc *>(host.data());
        int64_t *coff = reinterpret_cast<int64_t *>(host.data() + (L.chunk_off - L.chunks));
        int64_t c = 0;
        for (int m = 0; m < num_meshes; ++m) {
            coff[m] = c;
            for (int64_t t = tri_offsets_host[m]; t < tri_offsets_host[m + 1]; t += CHUNK)
                cd[c++] = ChunkDesc{t, (int32_t)std::min<int64_t>(CHUNK, tri_offsets_host[m + 1] - t), m};
        }
        coff[num_meshes] = c;
        memcpy(host.data() + (L.vert_off - L.chunks), vert_offsets_host, sizeof(int64_t) * (num_meshes + 1));
        memcpy(host.data() + (L.tri_off - L.chunks), tri_offsets_host, sizeof(int64_t) * (num_meshes + 1));
        memcpy(host.data() + (L.keys - L.chunks), keys_host, sizeof(uint64_t) * num_meshes);
    }
    uint8_t *ws = static_cast<uint8_t *>(workspace_dev);
    hipStream_t s = (hipStream_t)stream;
    double *area = reinterpret_cast<double *>(ws + L.area), *chunk_total = reinterpret_cast<double *>(ws + L.chunk_total);
    double *chunk_prefix = reinterpret_cast<double *>(ws + L.chunk_prefix), *total = reinterpret_cast<double *>(ws + L.total);
    int64_t *counts = reinterpret_cast<int64_t *>(ws + L.counts);
    int32_t *bad = reinterpret_cast<int32_t *>(ws + L.bad);
    const ChunkDesc *chunks = reinterpret_cast<const ChunkDesc *>(ws + L.chunks);
    const int64_t *chunk_off = reinterpret_cast<const int64_t *>(ws + L.chunk_off), *vert_off = reinterpret_cast<const int64_t *>(ws + L.vert_off);
    const int64_t *tri_off = reinterpret_cast<const int64_t *>(ws + L.tri_off);
    const uint64_t *keys = reinterpret_cast<const uint64_t *>(ws + L.keys);
    DGDM_HIP_CHECK(hipMemcpyAsync(ws + L.chunks, host.data(), host.size(), hipMemcpyHostToDevice, s));
    DGDM_HIP_CHECK(hipMemsetAsync(bad, 0, sizeof(int32_t) * num_meshes, s));
    if (n_chunks > 0) {
        hipLaunchKernelGGL(area_kernel, dim3((unsigned)n_chunks), dim3(SCAN_THREADS), 0, s, verts_dev, tris_dev, vert_off, chunks, area, chunk_total, bad);
        DGDM_HIP_CHECK(hipGetLastError());
    }
    hipLaunchKernelGGL(chunk_scan_kernel, dim3((unsigned)((num_meshes + 63) / 64)), dim3(64), 0, s, chunk_off, num_meshes, chunk_prefix, chunk_total, total);
    DGDM_HIP_CHECK(hipGetLastError());
    if (n_chunks > 0) {
        hipLaunchKernelGGL(count_kernel, dim3((unsigned)n_chunks), dim3(SCAN_THREADS), 0, s, chunks, area, chunk_prefix, total, (double)num_points, counts);
        DGDM_HIP_CHECK(hipGetLastError());
    }
    // every mesh must have triangles with valid indices and a positive area before anything is sampled (open3d raises on A <= 0 too)
    std::vector<double> A(num_meshes);
    std::vector<int32_t> B(num_meshes);
    DGDM_HIP_CHECK(hipMemcpyAsync(A.data(), total, sizeof(double) * num_meshes, hipMemcpyDeviceToHost, s));
    DGDM_HIP_CHECK(hipMemcpyAsync(B.data(), bad, sizeof(int32_t) * num_meshes, hipMemcpyDeviceToHost, s));
    DGDM_HIP_CHECK(hipStreamSynchronize(s));
    for (int m = 0; m < num_meshes; ++m) {
        DGDM_REQUIRE(!B[m], DGDM_EINVAL, "%s: mesh %d has a triangle whose vertex index is outside its %lld vertices", fn, m,
                     (long long)(vert_offsets_host[m + 1] - vert_offsets_host[m]));
        DGDM_REQUIRE(A[m] > 0.0, DGDM_EINVAL, "%s: mesh %d has surface area %g (%lld triangles); it must be > 0", fn, m, A[m],
                     (long long)(tri_offsets_host[m + 1] - tri_offsets_host[m]));
    }
    const int64_t n_out = (int64_t)num_meshes * num_points;
    hipLaunchKernelGGL(sample_kernel, dim3((unsigned)((n_out + 255) / 256)), dim3(256), 0, s, verts_dev, tris_dev, vert_off, tri_off, keys, seed,
                       counts, num_points, n_out, out_dev);
    DGDM_HIP_CHECK(hipGetLastError());
    return DGDM_OK;
}

// plan_chain_rows (dgdm_amd/csrc/row_plan.h) under the host sanitizers: a stand-alone program, no GPU and no Python.
//
//   hipcc --offload-arch=gfx950 -std=c++17 -g -Xarch_host -fsanitize=address,undefined -fsanitize=address,undefined \
//         dgdm_amd/csrc/row_plan.hip scripts/row_plan_sanitize.cpp -o row_plan_sanitize && ./row_plan_sanitize
//
// Runs the cases of tests/test_host_logic.py::test_row_plan_* (each checked against std::stable_sort) and prints "ok"; a sanitizer
// report or a wrong plan ends it with a non-zero status.
#include "../dgdm_amd/csrc/row_plan.h"
#include "../include/dgdm_hip.h"
#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <random>
#include <vector>

static char last_error[512];
namespace dgdm {
void set_error(const char *fmt, ...) {       // host_util.hip's, which the program does not link
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(last_error, sizeof last_error, fmt, ap);
    va_end(ap);
}
}  // namespace dgdm

#define EXPECT(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: %s failed (%s)\n", __FILE__, __LINE__, #cond, last_error); exit(1); } } while (0)

struct Case { int n_chains; int64_t rows; int n_calls; int64_t pad; int64_t sub; int N; bool need_order; };

static std::vector<int64_t> draws(const Case &c, std::mt19937 &rng) {
    const int64_t stride = c.n_calls > 1 ? (int64_t)c.n_chains * 2 * c.rows + c.pad : 0;
    std::vector<int64_t> s((size_t)((c.n_calls - 1) * stride + c.n_chains * 2 * c.rows), -1);      // exactly what the plan may read
    for (int k = 0; k < c.n_calls; ++k)
        for (int ch = 0; ch < c.n_chains; ++ch) {
            int64_t *call = s.data() + k * stride + ch * 2 * c.rows;
            for (int64_t r0 = 0; r0 < c.rows; r0 += c.sub) {
                const int64_t n = std::min(c.sub, c.rows - r0);
                for (int64_t i = 0; i < n; ++i) {
                    call[2 * r0 + i] = rng() % c.N;
                    call[2 * r0 + n + i] = rng() % 4 == 0 ? 511 : rng() % 512;      // the top value often: repeated pairs
                }
            }
        }
    return s;
}

static void run(const Case &c, std::mt19937 &rng) {
    const std::vector<int64_t> s = draws(c, rng);
    const int64_t stride = c.n_calls > 1 ? (int64_t)c.n_chains * 2 * c.rows + c.pad : 0, rt = c.rows * c.n_calls;
    // exact-size outputs: a write past any of them is the sanitizer's to find
    std::vector<int> pairs((size_t)c.n_chains * rt * 2, -7), order(c.need_order ? (size_t)c.n_chains * rt : 0, -7),
        goff(c.need_order ? (size_t)c.n_chains * (c.N + 1) : 0, -7);
    EXPECT(dgdm::plan_chain_rows(s.data(), c.n_chains, c.rows, c.n_calls, stride, c.sub, c.N, c.need_order, pairs.data(),
                                 c.need_order ? order.data() : nullptr, c.need_order ? goff.data() : nullptr) == DGDM_OK);
    for (int ch = 0; ch < c.n_chains; ++ch) {
        const int *p = pairs.data() + (size_t)ch * rt * 2;
        for (int k = 0; k < c.n_calls; ++k)
            for (int64_t r0 = 0; r0 < c.rows; r0 += c.sub) {
                const int64_t n = std::min(c.sub, c.rows - r0);
                const int64_t *call = s.data() + k * stride + ch * 2 * c.rows + 2 * r0;
                for (int64_t i = 0; i < n; ++i) EXPECT(p[2 * (k * c.rows + r0 + i)] == call[i] && p[2 * (k * c.rows + r0 + i) + 1] == call[n + i]);
            }
        if (!c.need_order) continue;
        std::vector<int> idx((size_t)rt);
        std::iota(idx.begin(), idx.end(), 0);
        std::stable_sort(idx.begin(), idx.end(), [&](int a, int b) { return p[2 * a] != p[2 * b] ? p[2 * a] < p[2 * b] : p[2 * a + 1] < p[2 * b + 1]; });
        const int *o = order.data() + (size_t)ch * rt, *g = goff.data() + (size_t)ch * (c.N + 1);
        for (int64_t i = 0; i < rt; ++i) EXPECT(o[i] == (idx[i] | (p[2 * idx[i] + 1] << 22)));
        for (int v = 0; v <= c.N; ++v) {
            int64_t below = 0;
            for (int64_t r = 0; r < rt; ++r) below += p[2 * r] < v;
            EXPECT(g[v] == below);
        }
    }
}

int main() {
    std::mt19937 rng(5);
    run({2, 7, 1, 0, 3, 5, true}, rng);              // a short last sub-batch, repeated pairs, an empty group, s2 = 511
    run({2, 7, 2, 5, 3, 5, true}, rng);              // two calls, blocks further apart than the chains need
    run({2, 7, 2, 5, 3, 5, false}, rng);             // the pairs alone: no order, no offsets (null)
    run({1, 1, 1, 0, 1, 1, true}, rng);              // one row, one point
    run({3, 50, 1, 0, 512, 1024, true}, rng);        // the largest cloud; a sub-batch longer than the call
    run({4, 40000, 1, 0, 512, 512, true}, rng);      // the threaded branch (2 threads)
    // refusals: nothing out of range is used as an index
    const Case small{1, 7, 1, 0, 3, 5, true};
    const int64_t bad[3][2] = {{1, -1}, {1, 5}, {4, 512}};
    for (const auto &b : bad) {
        std::vector<int64_t> s = draws(small, rng);
        s[(size_t)b[0]] = b[1];
        std::vector<int> pairs(14), order(7), goff(6);
        EXPECT(dgdm::plan_chain_rows(s.data(), 1, 7, 1, 0, 3, 5, true, pairs.data(), order.data(), goff.data()) == DGDM_EINVAL);
        EXPECT(!strcmp(last_error, "FPS start out of range (sa1 must be in [0, 5), sa2 in [0, 512))"));
    }
    int64_t none = 0;
    int nothing = 0;                                 // the limit is refused before anything is read or written
    EXPECT(dgdm::plan_chain_rows(&none, 1, (int64_t)1 << 21, 2, (int64_t)1 << 22, 512, 5, true, &nothing, &nothing, &nothing) == DGDM_EINVAL);
    EXPECT(!strcmp(last_error, "4194304 rows per chain in one gather launch (limit 4194303)"));
    puts("ok");
    return 0;
}

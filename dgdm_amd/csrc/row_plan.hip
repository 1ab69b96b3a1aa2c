// plan_chain_rows (row_plan.h) and its host-only test entry.
#include "row_plan.h"
#include "common.h"
#include <algorithm>
#include <atomic>
#include <cstring>
#include <thread>

namespace dgdm {

int check_row_plan(int64_t rt, bool need_order) {
    DGDM_REQUIRE(!need_order || rt <= ROW_PLAN_MAX_ROWS, DGDM_EINVAL, "%lld rows per chain in one gather launch (limit %lld)", (long long)rt,
                 (long long)ROW_PLAN_MAX_ROWS);
    return DGDM_OK;
}

int plan_chain_rows(const int64_t *starts_host, int n_chains, int64_t rows, int n_calls, int64_t call_stride, int64_t sb, int N, bool need_order,
                    int *dst, int *ord, int *goff) {
    const int64_t rt = rows * n_calls;                         // rows per chain
    int rc;
    if ((rc = check_row_plan(rt, need_order))) return rc;
    // per chain: int64 draws -> (s1, s2) int32 pairs in row order; rows sorted by s1 (counting sort) so that the rows of one
    // variant gather from the same Z slab; group offsets
    std::atomic<int> bad{0};
    auto work = [&](int c0, int c1) {
        std::vector<int> cnt(N + 1), cnt2(513), tmp;
        for (int c = c0; c < c1; ++c) {
            int *d = dst + (size_t)c * 2 * rt;
            for (int k = 0; k < n_calls; ++k) {
                const int64_t *src = starts_host + (size_t)k * call_stride + (size_t)c * 2 * rows;
                int *dk = d + 2 * (size_t)k * rows;
                for (int64_t r0 = 0; r0 < rows; r0 += sb) {
                    const int64_t n = std::min(sb, rows - r0);
                    const int64_t *s1 = src + 2 * r0, *s2 = s1 + n;
                    for (int64_t i = 0; i < n; ++i) {
                        const int64_t a = s1[i], b = s2[i];
                        if (!(a >= 0 && a < N && b >= 0 && b < 512)) { bad.store(1); return; }
                        dk[2 * (r0 + i)] = (int)a; dk[2 * (r0 + i) + 1] = (int)b;
                    }
                }
            }
            if (!need_order) continue;                      // embedding-table path: rows are looked up where they are
            // rows sorted by (s1, s2): two stable counting sorts, s2 first.  Rows of one variant s1 gather from the same Z slab, and
            // rows that share both draws are the same row (xobj_rows_kernel computes a run of them once)
            int *o = ord + (size_t)c * rt;
            tmp.resize((size_t)rt);
            std::fill(cnt2.begin(), cnt2.end(), 0);
            for (int64_t r = 0; r < rt; ++r) ++cnt2[d[2 * r + 1] + 1];
            for (int k = 0; k < 512; ++k) cnt2[k + 1] += cnt2[k];
            for (int64_t r = 0; r < rt; ++r) tmp[cnt2[d[2 * r + 1]]++] = (int)r;
            std::fill(cnt.begin(), cnt.end(), 0);
            for (int64_t r = 0; r < rt; ++r) ++cnt[d[2 * r] + 1];
            for (int k = 0; k < N; ++k) cnt[k + 1] += cnt[k];
            memcpy(goff + (size_t)c * (N + 1), cnt.data(), sizeof(int) * (N + 1));
            for (int64_t i = 0; i < rt; ++i) { const int r = tmp[i]; o[cnt[d[2 * r]]++] = r | (d[2 * r + 1] << 22); }      // row id | s2 << 22
        }
    };
    const int hw = (int)std::max(2u, std::thread::hardware_concurrency());
    const int nthreads = (int)std::min<int64_t>(std::min(16, hw / 2), std::max<int64_t>(1, std::min<int64_t>(n_chains, (int64_t)n_chains * rt / 65536)));
    if (nthreads <= 1) {
        work(0, n_chains);
    } else {
        std::vector<std::thread> pool;
        for (int t = 0; t < nthreads; ++t) pool.emplace_back(work, (int)((int64_t)n_chains * t / nthreads), (int)((int64_t)n_chains * (t + 1) / nthreads));
        for (auto &th : pool) th.join();
    }
    DGDM_REQUIRE(!bad.load(), DGDM_EINVAL, "FPS start out of range (sa1 must be in [0, %d), sa2 in [0, 512))", N);
    return DGDM_OK;
}

}  // namespace dgdm

extern "C" int dgdm_debug_row_plan(const int64_t *starts_host, int n_chains, int64_t rows, int n_calls, int64_t call_stride, int64_t sub_batch,
                                   int num_object_points, int need_order, int32_t *pairs_out, int32_t *order_out, int32_t *group_off_out) {
    DGDM_REQUIRE(starts_host && pairs_out && (!need_order || (order_out && group_off_out)), DGDM_EINVAL, "dgdm_debug_row_plan: null argument");
    DGDM_REQUIRE(n_chains > 0 && rows > 0 && n_calls > 0 && call_stride >= 0 && sub_batch > 0 && num_object_points > 0 && num_object_points <= 1024,
                 DGDM_EINVAL, "dgdm_debug_row_plan: bad argument");
    return dgdm::plan_chain_rows(starts_host, n_chains, rows, n_calls, call_stride, sub_batch, num_object_points, need_order != 0, pairs_out, order_out,
                                 group_off_out);
}

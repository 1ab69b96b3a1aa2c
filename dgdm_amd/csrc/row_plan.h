// The row plan of a 3-D gather launch: a pure host function (no HIP call, no handle state).
#pragma once
#include <stdint.h>

namespace dgdm {

// a sorted row packs `row | s2 << 22`: a launch holds fewer than 2^22 rows per chain
constexpr int64_t ROW_PLAN_MAX_ROWS = ((int64_t)1 << 22) - 1;

// The FPS start draws of `n_calls` classifier calls per chain -> what the gather kernels read.
//   in:  call k of chain c at starts_host + k * call_stride + c * 2 * rows, in the reference's draw order: per sub-batch of up to
//        `sub_batch` rows, that sub-batch's sa1 draws (each in [0, N)), then its sa2 draws (each in [0, 512))
//   pairs_out [n_chains][n_calls * rows][2]: (s1, s2) per row; a chain's rows of all calls form one run, row k * rows + r
//   need_order: order_out [n_chains][n_calls * rows]: the chain's rows sorted by (s1, s2), rows with equal draws in row order, each as
//        row | s2 << 22; group_off_out [n_chains][N + 1]: where the rows of each s1 start in that list ([N] = their number).
//        Without need_order neither is touched.
// Chains are independent: min(16, hardware threads / 2, n_chains, n_chains * n_calls * rows / 65536) host threads share them.
// DGDM_EINVAL (and the message) for a draw out of range, or - with need_order - more than ROW_PLAN_MAX_ROWS rows per chain.
int check_row_plan(int64_t rows_per_chain, bool need_order);      // the limit alone: what a caller refuses before it allocates for the plan
int plan_chain_rows(const int64_t *starts_host, int n_chains, int64_t rows, int n_calls, int64_t call_stride, int64_t sub_batch, int N,
                    bool need_order, int *pairs_out, int *order_out, int *group_off_out);

}  // namespace dgdm

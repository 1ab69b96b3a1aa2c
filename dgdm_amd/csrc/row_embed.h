// The rows of a 3-D classifier call: FPS start draws -> PointNet++ embeddings the trunk can read.
#pragma once
#include "object_tables.h"

namespace dgdm {

class RowEmbedder;

// The embeddings of `n_calls` classifier calls at once: afterwards call k reads rows [k * rows_per_call, (k + 1) * rows_per_call)
// of every chain.  tab: index rows into per-chain tables (the objects' embedding tables, or the group gather's mix of M0 and gathered
// rows), else materialised rows; used16: bf16 rows
struct Embedded {
    bool tab = false, used16 = false;
    int l1 = 0;           // tab, float32: the chains whose layer-1 tables the embedder holds (the tabled front of the f16x3 gradient trunk)
    int64_t rows_per_chain = 0;
    void point(TrunkParams *p, const RowEmbedder &r, int call, int64_t rows_per_call) const;      // points the trunk at call `call`'s rows
};

// Owns the per-row device buffers, the pinned staging block and the upload stream of a handle, and reads the store's tables.
//
// Ordering rules, all of them kept here:
//  - the host fills the staging block only after staging.ev: the previous copy out of it has finished.
//  - the copies of a call run on the upload stream behind `up_consumed` (the last readers of the device buffers, recorded on the
//    launch stream at the end of embed_rows), and the launch stream waits for `up_ready` behind them.  Where the gathers start
//    beside a build in flight the copies go on the launch stream itself (upload_starts has why).
//  - every way through embed_rows ends with the launch stream joined to the store's build, an error half way through the early
//    gathers included: the trunk's reads of M0 / L1Z through the pointer arrays are covered, and nothing enqueued is left un-joined.
//    Ahead of the join run only the index kernel (behind tables_started) and the per-object gathers (each behind object_done).
class RowEmbedder {
public:
    explicit RowEmbedder(ObjectStore3D &st) : store(st) {}
    RowEmbedder(const RowEmbedder &) = delete;
    RowEmbedder &operator=(const RowEmbedder &) = delete;
    // buffers for max_chains chains of rows_per_chain rows (they grow when a call brings more rows)
    int init(int num_object_points, int64_t sub_batch_size, int max_chains, int64_t rows_per_chain);
    // set at create, and by the test hook dgdm_guidance_debug_fps_path
    int serial = 0;                 // DGDM_SERIAL_STEP (guidance.h)
    bool l1tab = true;              // DGDM_L1TAB
    bool xtab_enabled = true;       // modes 1-3 read materialised rows (per-step gather kernels) instead of the embedding table
    int xobj_mode = 0;              // 0 = group kernel where possible, 2 = per-row table kernel (xobj_fast_kernel)
    bool force_slow_xobj = false;   // always run the per-row FPS kernel
    // the embedding tables may serve the rows (modes 1-3 force the gather kernels)
    bool tables_wanted() const { return xtab_enabled && !force_slow_xobj && xobj_mode == 0; }
    // The embeddings of the rows of `n_calls` consecutive classifier calls.  They depend on the FPS start draws and the objects only - not
    // on x - so a whole denoise loop's (or roll-out's) worth can be made before its first step: one upload and ONE gather launch whose
    // (chain, s1) groups hold the rows of all the calls (the variant's slab is staged once for five times the rows; beside a table build
    // still in flight the launch is cut by object, each part behind its object's tables: run_xobj), or - when every chain's object has
    // its embedding table in the wanted format (float32, or bf16 operand-order rows: want16) - one index kernel.
    // trunk_bf16: the trunk that will read the rows is the bf16 one (it has no float32 table form)
    int embed_rows(const int *objidx_host, int n_chains, const int64_t *starts_host, int64_t rows_per_call, int n_calls, int64_t call_stride,
                   bool want16, bool trunk_bf16, Embedded *e, hipStream_t s);

private:
    friend struct Embedded;
    // the gather of an object's rows starts behind its tables: only where a build off the stream has still to be joined (afterwards,
    // and on tables built earlier, one launch over all chains as ever)
    bool gather_early(hipStream_t s) const { return !(serial & 9) && !prof_on() && store.gather_early(s); }
    int ensure_rows(int n_chains, int64_t rows_per_chain);      // grows the per-row device buffers and the pinned staging area
    // starts of `n_calls` classifier calls per chain (row_plan.h has the layouts) -> starts / order / groupoff
    int upload_starts(const int64_t *starts_host, int n_chains, int64_t rows, hipStream_t s, bool need_order, int n_calls, int64_t call_stride,
                      bool on_launch_stream);
    // The layer-1 tables of the chains in of_chain (null: the chain does not read its object's float32 M0) and the chain list -> l1ptrs;
    // *n_tabled: how many chains have a table (0: nothing was uploaded)
    int fill_l1ptrs(const std::vector<const ObjectTables *> &of_chain, int *n_tabled, hipStream_t s);
    // what the trunk reads the chains through: per-chain lookup info and table bases go up and the index kernel runs (it reads fps1
    // and the draws only); fill_l1ptrs for m0_of, before (l1_first) or behind the two uploads
    int index_rows(const std::vector<XidxChain> &xc, const std::vector<const void *> &base, const std::vector<const ObjectTables *> &m0_of,
                   bool l1_first, int64_t rows, int *l1, hipStream_t s);
    // the rows' indices into the embedding tables (every chain's object has its table in the wanted format): no per-step gather runs at all
    int use_xtab(const int *objidx_host, int n_chains, int64_t rows, bool want16, int *l1, hipStream_t s);
    // via_tab: the group kernel gathered only the chains that need it (see there) and the trunk reads every chain through xtabptrs / xidx
    // l1: the number of chains whose layer-1 tables went into l1ptrs
    int run_xobj(const int *objidx_host, int n_chains, int64_t rows, bool want16, bool trunk_bf16, bool *used16, bool *via_tab, int *l1, hipStream_t s);

    ObjectStore3D &store;
    int N = 0, max_chains = 0;
    int64_t sub_batch = 0;
    DevBuf xobj, xobj16;                     // materialised rows [chains][rows][256] float32 / [128] bf16 dwords (run_xobj alone writes them)
    DevBuf starts, order, groupoff;          // the row plan on the device
    DevBuf xchains, todo;                    // the gather kernels' chains, and their list of tie-flagged rows + its counter
    int64_t todo_capacity = 0;
    DevBuf xidx, xidxchains, xtabptrs;       // embedding-table path: row index per reference row, per-chain lookup info, per-chain table base pointers
    // layer-1 tables of the f16x3 gradient trunk (ObjectTables::L1Z / L1K): beside xtabptrs, [2][max_chains] pointers - a chain's
    // L1Z and L1K where its table is its object's float32 M0 and the object has them, else null - and behind them the chain list
    // [max_chains] ints, those chains first (trunk.h TrunkParams::chainlist)
    DevBuf l1ptrs;
    PinnedBuf staging;                       // [pairs | order | group offsets] of a call
    Stream cstream;                          // uploads go through their own stream: the copy engine works beside the kernels of the launch stream
    Event up_ready, up_consumed;
};

}  // namespace dgdm

// Diffusion.cond_fn / get_convergence_centers (generator/diffusion.py:473-539) for batches of chains,
// and the PointNet++-backed forward entry points.
#include "common.h"
#include "models.h"
#include <algorithm>
#include <cmath>
#include <cstring>
#include <unordered_map>
#include <atomic>
#include <thread>

using namespace dgdm;

namespace {

// torch.linspace(start, end, steps) for float32 on CPU: symmetric evaluation around the midpoint
std::vector<float> linspace_f32(float start, float end, int steps) {
    std::vector<float> v(steps);
    if (steps == 1) { v[0] = start; return v; }
    const float step = (end - start) / (float)(steps - 1);
    const int half = steps / 2;
    for (int i = 0; i < steps; ++i) v[i] = i < half ? start + step * (float)i : end - step * (float)(steps - i - 1);
    return v;
}

struct ObjectTables {       // 3-D, per object
    // slices of the guidance handle's pools (the FPS tables of all objects are built by one launch each)
    const float *xyz = nullptr;   // [N][3]
    const int   *fps1 = nullptr;  // [N][512]
    const int   *fps2 = nullptr;  // [N][128] FPS(128) sequence by start point
    const int   *flags = nullptr; // [N] that sequence is order-dependent (exact distance tie / coordinates exhausted)
    DevBuf Z;               // [N][N][256]
    bool   fast_ok = false; // no flag set: rows can take their centres from fps2 instead of running FPS
    int *crowded = nullptr, *clist = nullptr;   // [N] int, [N + 1] int (clist[N] = count): centres whose ball query truncates (pointnet.hip crowd_kernel); pool slices
    DevBuf M0, cl2, cnt2;   // [N][256] float, [N][128] int, [N] int: variant-independent part of the sa3 max (pointnet.hip m0_kernel)
    DevBuf cl2s;            // [N][128] cl2 as positions in clist (xtab_kernel)
    DevBuf cl2o;            // [N][2][128] u16: cl2 as byte offsets into xobj_rows_kernel's LDS slab (scaled for the build's mode: has16), even / odd slots first
    DevBuf pcf;             // [N][512] per (s1, s2): sa2's start point, its list length, its tie flag (pointnet.hip pcf_kernel)
    DevBuf X, X16;          // [N][N][256] float32 / [N][N][128] bf16 dwords: the finished embedding per (s1, start point) (pointnet.hip xtab_kernel)
    bool   has_x = false, has_x16 = false;
    int    ncr = 0;         // number of crowded centres (read back by set_objects)
    DevBuf Z16, M0_16;      // bf16 operand-order copies, built when the handle is in bf16 mode at set_objects time
    bool   has16 = false;
    // [N][512] float, [N] int: layer 1's object part of the f16x3 trunk for the rows M0[q] - the scaled accumulators and the row's scale
    // exponent (trunk.h TrunkParams::l1z / l1k).  Written by set_objects' float32 build for an object without crowded centres (the
    // kernel looks at the device-side count); has_l1: the last build launched it, so the table is current whenever ncr == 0
    DevBuf L1Z, L1K;
    bool   has_l1 = false;
};

// A pose table of the trunk's first layer and the rows it spans: the cond_fn grid (G * P * P cells) or the orientation sweep (G cells)
struct PoseGrid {
    DevBuf tab, tiled;      // [cells][W1]; the same tiled for the trunk kernels (smallnet.h tile_table)
    DevBuf pmax;            // [cells] largest magnitude of a cell's row of tab (trunk_f16l.hip: f16 scale of 3-D layer 2's input); cond_fn grid only
    int cells = 0, tiles_per_b = 0;
    int64_t rows = 0;       // rows per chain: B * cells
};

}  // namespace

struct DgdmGuidance {
    DgdmDynamics *m = nullptr;
    DgdmGuidanceConfig cfg{};
    int B = 0;
    PoseGrid grid, sweep;                        // cond_fn grid, orientation sweep
    DevBuf objpart;                              // 2-D: [max_objects][W1] doubles
    DevBuf objtmp;                               // 2-D: scratch of set_objects (the object encoder's hidden layer, [n_objects][512] doubles)
    std::vector<std::unique_ptr<ObjectTables>> tables;   // 3-D
    bool bf16 = false;                           // contractions of the trunk on bf16 MFMA (dgdm_guidance_set_contraction_dtype)
    bool f32_mfma = false;                       // float32 mode on the k-ordered float32 MFMA chain (trunk.hip) instead of the f16x3 form (trunk_f16l.hip)
    static constexpr int NBUILD = 3;             // most objects whose tables are built concurrently (own stream + 0.5 GB of temporaries each)
    DevBuf pool_crowded, pool_clist, pool_off, pool_pairs, pool_rank, pool_F1, pool_U;   // [n_objects] x the light build stages' outputs (built by one launch per stage)
    DevBuf pool_xyz, pool_fps1, pool_fps2, pool_flags, pool_ncr;   // [n_objects] x per-object FPS tables (ObjectTables point into these), crowded-centre counts
    DevBuf pool_fps1t;                              // float32 build: [n_objects] x fps1 by position [64][N] x 16 B (l2sel_kernel reads it with the variants on its lanes)
    DevBuf tmpY[NBUILD], tmpL2[NBUILD], vlist;      // 3-D table-build temporaries of the heavy stages (per build stream)
    DevBuf tmpShare[NBUILD];                        // float32 build: the selection stage's outputs (pointnet.h L2Share), carved out of one buffer
    hipStream_t bstream[NBUILD] = {};
    hipEvent_t bev[NBUILD] = {}, bstart = nullptr, pooled = nullptr, ldone = nullptr;      // pooled: the objects' coordinates are in the pool; ldone: the batched light build stages
    // V, genc, chainbias, timepart: float64 (smallnet.h linear64: per-finger / per-chain quantities are evaluated in double precision,
    // so the A table carries one float32 rounding); ttmp64: scratch of the time encoder
    DevBuf V, genc, atab, chainbias, timepart, ttmp, ttmp64, partial, objdev, objidx, xobj, xobj16, starts, order, xchains, todo, groupoff;
    DevBuf loopx[2], loopeps, loopgrad, loopxrep, loopts;      // workspace of dgdm_guided_chains_run
    DevBuf loopeps1;                                           // ... step 0's one eps-net evaluation [B][L], replicated into loopeps
    DevBuf loopkeys;                                           // ... the chains' noise keys [n_chains] uint64 (eta > 0)
    std::vector<uint64_t> loopkeys_host;                       // ... what loopkeys holds
    DevBuf loopcond, loopx2, loopeps2;                         // ... with a condition: [cond rows | zero rows], and the doubled batch of the classifier-free mix
    DevBuf scorelogits;                      // dgdm_guidance_score: the logits when the caller does not want them
    DevBuf valobj;                           // dgdm_guidance_objective_values: the device copy of the call's objectives
    // dgdm_guidance_rollout: the sweep's orientations [G] (built with the handle), and its scratch, grown on demand: the state
    // [n][B*G][3] doubles, one interaction's logits, the per-row pose operand tiles [ntiles][W1*32] and (3-D) their row maxima [ntiles][32]
    DevBuf sweep_ori, rollstate, rolllogits, rolltiles, rollpmax;
    // dgdm_guidance_set_row_field: the caller's field [rowfield_chains][R][3] (kept, not copied) for chains with use_rowcoef == DGDM_OBJ_ROWFIELD;
    // dgdm_guidance_goal_field: the position grid [P] beside sweep_ori, and the device copy of the call's specs
    const float *rowfield = nullptr;
    int rowfield_chains = 0;
    DevBuf pos_lin, goalspecs;
    // dgdm_guidance_label / _label_settled: the batch replicated over the objects' chains [M][B][L], score's counts and sums, the
    // roll-out's final state, first logits and left, the per-(finger, object) settled values
    DevBuf labelx, labelcounts, labelsums, labelfinal, labelfirst, labelleft, labelobj;
    int rolltiles_chains = 0;                // chains the tiles of the last roll-out cover (dgdm_guidance_debug_rollout_table)
    DevBuf xidx, xidxchains, xtabptrs;       // embedding-table path: row index per reference row, per-chain lookup info, per-chain table base pointers
    // layer-1 tables of the f16x3 gradient trunk (ObjectTables::L1Z / L1K).  l1ptrs: beside xtabptrs, [2][max_chains] pointers - a chain's
    // L1Z and L1K where its table is its object's float32 M0 and the object has them, else null - and behind them the chain list
    // [max_chains] ints, those chains first (trunk.h TrunkParams::chainlist); l1objs: set_objects' per-object pointer arrays.
    // l1tab = DGDM_L1TAB, read at create: 0 builds no table, every chain takes the trunk's general front (same-binary reference, A/B)
    DevBuf l1ptrs, l1objs;
    bool l1tab = true;
    int fill_l1ptrs(const std::vector<const ObjectTables *> &of_chain, int *n_tabled, hipStream_t s);
    bool xtab_enabled = true;       // test hook: modes 1-3 read materialised rows (per-step gather kernels) instead of the embedding table
    int xtab_policy = 0;            // 0: build the embedding tables once the objects have served more than XTAB_AFTER cond_fn calls; 1: at set_objects (test hook mode 5)
    int grads_since_set = 0;
    static constexpr int XTAB_AFTER = 5;
    int l2_gather_mode = 0;         // test hook (mode 4): build the sa2 features of the crowded centres with l2_kernel's global gathers
    int xobj_mode = 0;              // test hook: 0 = group kernel where possible, 2 = per-row table kernel (xobj_fast_kernel)
    int n_objects = 0;
    bool force_slow_xobj = false;   // test hook: always run the per-row FPS kernel
    void *pinned = nullptr; size_t pinned_bytes = 0; hipEvent_t pinned_ev = nullptr;
    int64_t todo_capacity = 0;
    // uploads of the start indices go through their own stream (the copy engine works beside the kernels of the launch stream):
    // up_ready orders the consumers behind the copy, up_consumed the next copy behind the last reader of the device buffers
    // set_objects' read-back (tie flags, crowded-centre counts) lands in pinned memory behind rb_ev and is only waited for when its
    // values are first needed - the host converts and uploads the first step's start indices while the tables are still being built.
    // A build off the caller's stream copies them as soon as both exist (behind the FPS tables and crowd_ev, the first light stage):
    // the host then plans the gather while the heavy stages still run.  ro_ev is the END of the build (behind the last heavy stage
    // and the layer-1 tables): join_tables, the next set_objects and the destructor order themselves by it, never by rb_ev.
    int *ro_host = nullptr; size_t ro_ints = 0; hipEvent_t ro_ev = nullptr, rb_ev = nullptr, crowd_ev = nullptr; bool ro_pending = false;
    std::vector<hipEvent_t> odone;      // odone[i]: object i's tables are complete (the end of build_object on its build stream); created once, re-recorded by every build
    int finish_objects();
    hipStream_t cstream = nullptr; hipEvent_t up_ready = nullptr, up_consumed = nullptr; bool consumed_recorded = false;
    // Step schedule.  The 3-D table build runs on the build streams alone and ends in ro_ev on bstream[0]; the first
    // call that reads the tables on a stream makes that stream wait for it (join_tables).  Inside the denoise loop the eps-net runs on
    // bstream[0] (idle by then) beside common_pre and is joined in front of the trunk.  serial = DGDM_SERIAL_STEP, read at create:
    // 1 everything on the caller's stream, in the order of the data dependencies (also while dgdm_prof_enable is on: the stage events
    // assume one stream); for measuring the parts apart, 2 = only the table build stays on the caller's stream, 4 = only the eps-net does,
    // 8 = only the gather stays behind the END of the build (one launch behind join_tables) instead of starting object by object
    int serial = 0;
    bool tables_off_stream() const { return !(serial & 3) && !prof_on(); }
    bool eps_beside() const { return !(serial & 5) && !prof_on(); }
    bool hoist_x_only() const { return !(serial & 1) && !prof_on(); }
    // the gather of an object's rows starts behind odone[object]: only where a build off the stream has still to be joined (afterwards,
    // and on tables built earlier, one launch over all chains as ever)
    bool gather_early(hipStream_t s) const { return !(serial & 9) && !prof_on() && built_off_stream && (join_pending || s != joined_stream); }
    bool built_off_stream = false, join_pending = false, built_once = false;
    hipStream_t joined_stream = nullptr;
    hipEvent_t fork_ev = nullptr, side_ev = nullptr;
    int join_tables(hipStream_t s) {
        if (!built_off_stream || (!join_pending && s == joined_stream)) return DGDM_OK;
        DGDM_HIP_CHECK(hipStreamWaitEvent(s, ro_ev, 0));
        join_pending = false; joined_stream = s;
        return DGDM_OK;
    }
    int side_stream(hipStream_t *side) {
        if (!bstream[0]) DGDM_HIP_CHECK(hipStreamCreateWithFlags(&bstream[0], hipStreamNonBlocking));
        if (!fork_ev) DGDM_HIP_CHECK(hipEventCreateWithFlags(&fork_ev, hipEventDisableTiming));
        if (!side_ev) DGDM_HIP_CHECK(hipEventCreateWithFlags(&side_ev, hipEventDisableTiming));
        *side = bstream[0];
        return DGDM_OK;
    }
    ~DgdmGuidance() {
        for (int i = 0; i < NBUILD; ++i)
            if (bstream[i]) (void)hipStreamSynchronize(bstream[i]);      // a build nobody joined may still be writing the buffers freed below
        if (fork_ev) (void)hipEventDestroy(fork_ev);
        if (side_ev) (void)hipEventDestroy(side_ev);
        if (pinned) (void)hipHostFree(pinned);
        if (pinned_ev) (void)hipEventDestroy(pinned_ev);
        if (ro_host) (void)hipHostFree(ro_host);
        if (ro_ev) (void)hipEventDestroy(ro_ev);
        if (rb_ev) (void)hipEventDestroy(rb_ev);
        if (crowd_ev) (void)hipEventDestroy(crowd_ev);
        for (hipEvent_t e : odone) (void)hipEventDestroy(e);
        if (cstream) (void)hipStreamDestroy(cstream);
        if (up_ready) (void)hipEventDestroy(up_ready);
        if (up_consumed) (void)hipEventDestroy(up_consumed);
        for (int i = 0; i < NBUILD; ++i) {
            if (bstream[i]) (void)hipStreamDestroy(bstream[i]);
            if (bev[i]) (void)hipEventDestroy(bev[i]);
        }
        if (bstart) (void)hipEventDestroy(bstart);
        if (ldone) (void)hipEventDestroy(ldone);
        if (pooled) (void)hipEventDestroy(pooled);
    }
    int build_pose_table(const std::vector<float> &ori, const std::vector<float> &pos, PoseGrid *dst, hipStream_t s);
    // the first-layer tables and the shape of a launch over `g` for n_chains chains
    void set_grid(dgdm::TrunkParams *p, const PoseGrid &g, int n_chains) const;
    int check_objects(const int *oidx, int n_chains) const;
    // test hook (dgdm_guidance_debug_fps_path): the embedding tables may serve the rows (modes 1-3 force the gather kernels)
    bool tables_wanted() const { return xtab_enabled && !force_slow_xobj && xobj_mode == 0; }
    int common_pre(const float *x_dev, float t_scaled, const int *objidx_host, int n_chains, hipStream_t s);
    // starts of `n_calls` classifier calls per chain: call k of chain c at starts_host + k * call_stride + c * 2 * rows; on the device the
    // chain's rows of all calls form one run of n_calls * rows rows (row k * rows + r)
    int upload_starts(const int64_t *starts_host, int n_chains, int64_t rows, hipStream_t s, bool need_order = true, int n_calls = 1,
                      int64_t call_stride = 0, bool on_launch_stream = false);
    int ensure_rows(int n_chains, int64_t rows_per_chain);      // grows the per-row device buffers and the pinned staging area
    // the rows' indices into the embedding tables (every chain's object has its table in the wanted format): no per-step gather runs at all
    int use_xtab(const int *objidx_host, int n_chains, int64_t rows, bool want16, int *l1, hipStream_t s);
    int build_object(int oi, int slot, hipStream_t s);
    int build_xtab(int oi, hipStream_t s);
    // via_tab: the group kernel gathered only the chains that need it (see there) and the trunk reads every chain through xtabptrs / xidx
    // l1: the number of chains whose layer-1 tables went into l1ptrs
    int run_xobj(const int *objidx_host, int n_chains, int64_t rows, bool want16, bool *used16, bool *via_tab, int *l1, hipStream_t s);
    // the embeddings of `n_calls` classifier calls at once (3-D): afterwards call k reads rows [k * rows_per_call, (k + 1) * rows_per_call)
    // of every chain.  tab: index rows into per-chain tables (the objects' embedding tables, or run_xobj's mix of M0 and gathered rows), else
    // materialised rows; used16: bf16 rows
    struct Embedded {
        bool tab = false, used16 = false;
        int l1 = 0;           // tab, float32: the chains whose layer-1 tables l1ptrs holds (the tabled front of the f16x3 gradient trunk)
        int64_t rows_per_chain = 0;
        void point(dgdm::TrunkParams *p, const DgdmGuidance &g, int call, int64_t rows_per_call) const;
    };
    int embed_rows(const int *objidx_host, int n_chains, const int64_t *starts_host, int64_t rows_per_call, int n_calls, int64_t call_stride,
                   bool want16, Embedded *e, hipStream_t s);
    // cond_fn's: the rows of the cond_fn grid in the handle's arithmetic, counted towards the XTAB_AFTER policy, one `xobj` profiling region
    int embed(const int *objidx_host, int n_chains, const int64_t *starts_host, int n_calls, int64_t call_stride, Embedded *e, hipStream_t s);
    // what cond_fn's gradient and its forward-only scoring share, up to the trunk launch: common_pre, 3-D: the rows' embeddings (`emb` /
    // `call` as guidance_grad takes them), and the trunk parameters of the cond_fn grid in the float32 form (the caller swaps the weight
    // streams for its arithmetic and adds its outputs)
    // pre_done: the caller has already enqueued common_pre for this x and timestep (the denoise loop does, ahead of the tables' join)
    int trunk_front(int kind, const float *x_dev, int timestep, const int *objidx_host, const int64_t *starts_host, int n_chains, const Embedded *emb,
                    int call, dgdm::TrunkParams *p, hipStream_t s, bool pre_done = false);
};

int DgdmGuidance::build_pose_table(const std::vector<float> &ori, const std::vector<float> &pos, PoseGrid *dst, hipStream_t s) {
    const int n = (int)ori.size(), W1 = m->W1;
    dst->cells = n; dst->tiles_per_b = (n + 31) / 32; dst->rows = (int64_t)B * n;
    DevBuf d_ori, d_pos, d_emb;
    int rc;
    if ((rc = d_ori.upload(ori.data(), sizeof(float) * n))) return rc;
    if ((rc = d_pos.upload(pos.data(), sizeof(float) * 2 * n))) return rc;
    if ((rc = d_emb.alloc(sizeof(float) * 27 * n))) return rc;
    if ((rc = dst->tab.alloc(sizeof(float) * (size_t)W1 * n))) return rc;
    if ((rc = pose_embed(d_ori.as<float>(), d_pos.as<float>(), d_emb.as<float>(), n, s))) return rc;
    if ((rc = linear64(d_emb.as<float>(), nullptr, 27, m->blob64.at(m->off64.w1p_wt), nullptr, nullptr, 1, nullptr, dst->tab.as<float>(), W1, n, 27, W1, ACT_NONE, s))) return rc;
    if ((rc = dst->tiled.alloc(sizeof(float) * (size_t)W1 * dst->tiles_per_b * 32))) return rc;
    if ((rc = tile_table(dst->tab.as<float>(), n, W1, dst->tiled.as<float>(), s))) return rc;
    DGDM_HIP_CHECK(hipStreamSynchronize(s));     // temporaries die here
    return DGDM_OK;
}

void DgdmGuidance::set_grid(TrunkParams *p, const PoseGrid &g, int n_chains) const {
    p->Atab = atab.as<float>(); p->Ptab = g.tab.as<float>(); p->PtabT = g.tiled.as<float>(); p->Pmax = g.pmax.as<float>();
    p->B = B; p->C = g.cells; p->tiles_per_b = g.tiles_per_b; p->ntiles = n_chains * B * g.tiles_per_b; p->R = g.rows;
    p->xstride = g.rows;                         // 3-D: Embedded::point, afterwards
}

int DgdmGuidance::check_objects(const int *oidx, int n_chains) const {
    DGDM_REQUIRE(n_objects > 0, DGDM_EINVAL, "dgdm_guidance_set_objects has not been called");
    for (int i = 0; i < n_chains; ++i)
        DGDM_REQUIRE(oidx[i] >= 0 && oidx[i] < n_objects, DGDM_EINVAL, "chain %d refers to object %d of %d", i, oidx[i], n_objects);
    return DGDM_OK;
}

extern "C" int dgdm_guidance_create(DgdmGuidance **out, DgdmDynamics *model, const DgdmGuidanceConfig *cfg) {
    DGDM_REQUIRE(out && model && cfg, DGDM_EINVAL, "dgdm_guidance_create: null argument");
    DGDM_REQUIRE(cfg->batch > 0 && cfg->grid_size > 0 && cfg->num_pos > 0 && cfg->max_chains > 0 && cfg->num_train_timesteps > 0,
                 DGDM_EINVAL, "dgdm_guidance_create: bad config");
    DGDM_REQUIRE(cfg->max_chains <= DGDM_MAX_CHAINS, DGDM_EINVAL, "max_chains %d > %d", cfg->max_chains, DGDM_MAX_CHAINS);
    if (model->kind == 3) {
        DGDM_REQUIRE(cfg->sub_batch_size > 0, DGDM_EINVAL, "3-D guidance needs sub_batch_size (it partitions the FPS start draws)");
        DGDM_REQUIRE(cfg->num_object_points > 0 && cfg->num_object_points <= 1024, DGDM_EINVAL, "object clouds of %d points unsupported (1..1024)", cfg->num_object_points);
    } else {
        DGDM_REQUIRE(2 * cfg->num_object_points == model->object_ch, DGDM_EINVAL, "2*num_object_points (%d) != object_ch (%d)", 2 * cfg->num_object_points, model->object_ch);
    }
    std::unique_ptr<DgdmGuidance> g(new DgdmGuidance());
    g->m = model; g->cfg = *cfg;
    g->B = cfg->batch;
    if (const char *e = getenv("DGDM_SERIAL_STEP")) g->serial = atoi(e);      // test hook: the serial step schedule
    if (const char *e = getenv("DGDM_L1TAB")) g->l1tab = atoi(e) != 0;        // test hook: 0 = no layer-1 tables, the trunk's general front everywhere
    const int G = cfg->grid_size, P = cfg->num_pos, C = G * P * P;
    // pose grid: torch.meshgrid(linspace(ori), linspace(-1,1,P), linspace(-1,1,P)) 'ij' -> cell = (g*P + px)*P + py  (diffusion.py:478)
    const std::vector<float> lo = linspace_f32(cfg->ori_lo, cfg->ori_hi, G), lp = linspace_f32(-1.f, 1.f, P);
    std::vector<float> ori(C), pos(2 * (size_t)C);
    for (int gi = 0; gi < G; ++gi)
        for (int a = 0; a < P; ++a)
            for (int b = 0; b < P; ++b) {
                const int c = (gi * P + a) * P + b;
                ori[c] = lo[gi]; pos[2 * c] = lp[a]; pos[2 * c + 1] = lp[b];
            }
    int rc;
    if ((rc = g->build_pose_table(ori, pos, &g->grid, nullptr))) return rc;
    {   // per-cell magnitude bound of the pose table (built once: the pose grid is fixed)
        std::vector<float> tab((size_t)C * model->W1), mx(C, 0.f);
        DGDM_HIP_CHECK(hipMemcpy(tab.data(), g->grid.tab.p, tab.size() * sizeof(float), hipMemcpyDeviceToHost));
        for (int c = 0; c < C; ++c)
            for (int j = 0; j < model->W1; ++j) mx[c] = std::max(mx[c], std::fabs(tab[(size_t)c * model->W1 + j]));
        if ((rc = g->grid.pmax.upload(mx.data(), mx.size() * sizeof(float)))) return rc;
    }
    std::vector<float> pos0(2 * (size_t)G, 0.f);                          // get_convergence_centers: pos = 0 (:511)
    if ((rc = g->build_pose_table(lo, pos0, &g->sweep, nullptr))) return rc;
    if ((rc = g->sweep_ori.upload(lo.data(), lo.size() * sizeof(float)))) return rc;
    if ((rc = g->pos_lin.upload(lp.data(), lp.size() * sizeof(float)))) return rc;
    const int W1 = model->W1, nc = cfg->max_chains;
    const size_t rows = (size_t)nc * g->B;
    const int64_t R = g->grid.rows;
    if ((rc = g->V.alloc(rows * 256 * 8)) || (rc = g->genc.alloc(rows * 256 * 8)) || (rc = g->atab.alloc(rows * W1 * 4)) ||
        (rc = g->chainbias.alloc((size_t)nc * W1 * 8)) || (rc = g->timepart.alloc((size_t)W1 * 8)) || (rc = g->ttmp.alloc(768 * 4)) ||
        (rc = g->ttmp64.alloc(512 * 8)) ||
        (rc = g->partial.alloc(rows * g->grid.tiles_per_b * W1 * 4)) || (rc = g->objdev.alloc(sizeof(TrunkObjective) * nc)) ||
        (rc = g->objidx.alloc(sizeof(int) * nc)))
        return rc;
    if (model->kind == 2) {
        if ((rc = g->objpart.alloc((size_t)std::max(1, cfg->max_objects) * W1 * 8))) return rc;
    } else {
        if ((rc = g->starts.alloc((size_t)nc * R * 2 * sizeof(int))) ||
            (rc = g->order.alloc((size_t)nc * R * sizeof(int))) || (rc = g->xchains.alloc(sizeof(XobjChain) * nc)) ||
            (rc = g->todo.alloc(((size_t)nc * R + 1) * sizeof(int))))
            return rc;
        g->todo_capacity = (int64_t)nc * R;
        g->pinned_bytes = ((size_t)nc * R * 3 + (size_t)nc * (cfg->num_object_points + 1)) * sizeof(int);
        if ((rc = g->groupoff.alloc((size_t)nc * (cfg->num_object_points + 1) * sizeof(int))) || (rc = g->xidx.alloc((size_t)nc * R * sizeof(int))) ||
            (rc = g->xidxchains.alloc(sizeof(XidxChain) * nc)) || (rc = g->xtabptrs.alloc(sizeof(void *) * nc)) ||
            (rc = g->l1ptrs.alloc(sizeof(void *) * 3 * nc)))
            return rc;
        DGDM_HIP_CHECK(hipHostMalloc(&g->pinned, g->pinned_bytes, hipHostMallocDefault));
        DGDM_HIP_CHECK(hipEventCreateWithFlags(&g->pinned_ev, hipEventDisableTiming));
    }
    *out = g.release();
    return DGDM_OK;
}

extern "C" void dgdm_guidance_destroy(DgdmGuidance *g) { delete g; }

extern "C" int dgdm_guidance_set_contraction_dtype(DgdmGuidance *g, int dtype) {
    DGDM_REQUIRE(g, DGDM_EINVAL, "dgdm_guidance_set_contraction_dtype: null handle");
    DGDM_REQUIRE(dtype >= DGDM_DTYPE_F32 && dtype <= DGDM_DTYPE_F32_F16X3, DGDM_EINVAL,
                 "contraction dtype %d unsupported (0 = f32 (default form), 1 = bf16, 2 = f32 on the float32 MFMA, 3 = f32 as 3 f16 products = the default form)", dtype);
    g->bf16 = dtype == DGDM_DTYPE_BF16;
    g->f32_mfma = dtype == DGDM_DTYPE_F32_MFMA;
    return DGDM_OK;
}

extern "C" int dgdm_guidance_debug_fps_path(DgdmGuidance *g, int force_per_row, int32_t *out_fast_ok) {
    DGDM_REQUIRE(g, DGDM_EINVAL, "dgdm_guidance_debug_fps_path: null handle");
    g->force_slow_xobj = force_per_row == 1;            // 1: every row runs its own FPS; 2: per-row table kernel; 0: default (group kernel)
    g->xobj_mode = force_per_row == 2 ? 2 : 0;
    g->l2_gather_mode = force_per_row == 4 ? 1 : 0;     // takes effect at the next dgdm_guidance_set_objects
    g->xtab_enabled = force_per_row == 0 || force_per_row == 4 || force_per_row == 5;      // modes 1-3 read materialised rows; 3 = the group gather kernel
    g->xtab_policy = force_per_row == 5 ? 1 : 0;         // 5: the next set_objects builds the embedding tables right away
    if (force_per_row == 3) g->xobj_mode = 0;
    if (out_fast_ok) {
        int rc = g->finish_objects();
        if (rc) return rc;
        for (int i = 0; i < g->n_objects && i < (int)g->tables.size(); ++i) out_fast_ok[i] = g->tables[i]->fast_ok ? 1 : 0;
    }
    return DGDM_OK;
}
// d objective / d (scaled z1) -> d objective / d z1: x 2^e_j per column (the trunk is equilibrated by exact powers of two, models_api.hip TrunkEquil)
__global__ void partials_true_units_kernel(float *p, const float *unit, size_t n, int W1) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] *= unit[i % W1];
}
// Test hook: the per-tile partial sums of d objective / d z1 the last dgdm_dyn{2,3}d_guidance_grad call left behind
// ([n_chains * B * tiles_per_b][W1], tile = (chain * B + b) * tiles_per_b + cell tile; a tile is 32 consecutive pose cells of one finger).
extern "C" int dgdm_guidance_debug_partials(DgdmGuidance *g, int n_chains, float *out_dev, int32_t *tiles_per_finger, int32_t *width, void *stream) {
    DGDM_REQUIRE(g && n_chains > 0 && n_chains <= g->cfg.max_chains, DGDM_EINVAL, "dgdm_guidance_debug_partials: bad argument");
    if (tiles_per_finger) *tiles_per_finger = g->grid.tiles_per_b;
    if (width) *width = g->m->W1;
    if (out_dev) {
        const size_t n = (size_t)n_chains * g->B * g->grid.tiles_per_b * g->m->W1;
        DGDM_HIP_CHECK(hipMemcpyAsync(out_dev, g->partial.p, n * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
        hipLaunchKernelGGL(partials_true_units_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, out_dev, g->m->z1_unit.as<float>(), n, g->m->W1);
        DGDM_HIP_CHECK(hipGetLastError());
    }
    return DGDM_OK;
}
extern "C" int64_t dgdm_guidance_rows(const DgdmGuidance *g) { return g ? g->grid.rows : 0; }
extern "C" int64_t dgdm_guidance_starts_per_call(const DgdmGuidance *g) { return (g && g->m->kind == 3) ? 2 * g->grid.rows : 0; }

// ------------------------------------------------------------------------------------------------ objects
int DgdmGuidance::build_object(int oi, int slot, hipStream_t s) {
    const int N = cfg.num_object_points;
    ObjectTables &t = *tables[oi];
    const PnWeights w = m->pn();
    int rc;
    if ((rc = t.Z.alloc((size_t)N * N * 256 * 4)) ||
        (rc = t.M0.alloc((size_t)N * 256 * 4)) || (rc = t.cl2.alloc((size_t)N * 128 * sizeof(int))) || (rc = t.cnt2.alloc((size_t)N * sizeof(int))) ||
        (rc = t.cl2s.alloc((size_t)N * 128 * sizeof(int))) || (rc = t.cl2o.alloc((size_t)N * 256 * sizeof(unsigned short))) ||
        (rc = t.pcf.alloc((size_t)N * 512 * sizeof(int))))
        return rc;
    t.has16 = bf16;
    if (bf16 && ((rc = t.Z16.alloc((size_t)N * N * 128 * 4)) || (rc = t.M0_16.alloc((size_t)N * 128 * 4)))) return rc;
    uint32_t *z16 = bf16 ? t.Z16.as<uint32_t>() : nullptr;
    DevBuf &tY = tmpY[slot], &tL2 = tmpL2[slot];
    if ((rc = tY.alloc((size_t)N * N * 256 * 4)) || (rc = tL2.alloc((size_t)N * N * 256 * 4))) return rc;
    const float *xyz = t.xyz;                                                                                  // T1: set_objects, batched
    // crowded flags / pair lists (crowd_kernel, nbr_fill_kernel), T2 (sa1) and T3 (U): set_objects, one launch per stage for all objects
    const int *off = pool_off.as<int>() + (size_t)oi * (N + 1), *pairs = pool_pairs.as<int>() + (size_t)oi * N * N;
    const short *rank = pool_rank.as<short>() + (size_t)oi * N * N;
    const char *U = static_cast<const char *>(pool_U.p) + (size_t)oi * N * 128 * (bf16 ? 4 : 8);      // float32 rows in bf16 mode, float64 otherwise
    if (bf16) {
        // bf16 mode: the sa3 contraction (T6) runs on the bf16 matrix pipe and rounds its input, so T4 writes and T5 reduces bf16
        // rows (the temporaries tY / tL2 are simply used at half size); the stages in front of it stay float32
        if ((rc = pn_pairs(xyz, N, reinterpret_cast<const float *>(U), w, pairs, off, tY.as<float>(), tY.as<uint32_t>(), s))) return rc;   // T4
        if ((rc = pn_l2(xyz, N, w, t.fps1, vlist.as<int>(), N, tY.as<float>(), tL2.as<float>(), t.clist, t.clist + N,
                        off, rank, true, s, l2_gather_mode ? 0 : 1))) return rc;                   // T5
        if ((rc = pn_z16(xyz, N, N, w, tL2.as<uint32_t>(), t.Z.as<float>(), z16, t.clist, t.clist + N, s))) return rc;          // T6
    } else {
        // float32 mode (the parity path): every contraction of the build accumulates in float64 and each table entry is rounded once
        // (pointnet64.hip); the max stages (T5, T7) are exact as they are
        const PnWeights64 w64 = m->pn64();
        if ((rc = pn_pairs64(xyz, N, reinterpret_cast<const double *>(U), w64, pairs, off, tY.as<float>(), s))) return rc;                 // T4
        // T5 / T6 of the crowded centres once per DISTINCT first-64 selection: Z[v][c] depends on v only through which points of c's ball
        // come first in fps1[v], and many variants select the same set.  The test hook's dense build (l2_gather_mode) and clouds the
        // crowded-centre kernel does not take (N > 512) compute every (variant, centre) row from its own L2 row.
        const bool shared = !l2_gather_mode && N <= 512;
        L2Share sh{};
        if (shared) {
            const size_t NN = (size_t)N * N;
            if ((rc = tmpShare[slot].alloc(NN * 64 + NN + NN * sizeof(short) + NN * sizeof(int) + (2 * (size_t)N + 4) * sizeof(int)))) return rc;
            char *b = static_cast<char *>(tmpShare[slot].p);
            sh.sel = reinterpret_cast<unsigned char *>(b); b += NN * 64;
            sh.items = reinterpret_cast<int *>(b); b += NN * sizeof(int);
            sh.coff = reinterpret_cast<int *>(b); b += N * sizeof(int);
            sh.ccnt = reinterpret_cast<int *>(b); b += N * sizeof(int);
            sh.nitems = reinterpret_cast<int *>(b); b += 4 * sizeof(int);
            sh.rep = reinterpret_cast<short *>(b); b += NN * sizeof(short);
            sh.cnt = reinterpret_cast<unsigned char *>(b);
            sh.fps1t = pool_fps1t.as<uint4>() + (size_t)oi * N * 64;
        }
        if ((rc = pn_l2(xyz, N, w, t.fps1, vlist.as<int>(), N, tY.as<float>(), tL2.as<float>(), t.clist, t.clist + N,
                        off, rank, false, s, shared ? 1 : 0, shared ? &sh : nullptr))) return rc;  // T5
        if ((rc = pn_z64(xyz, N, N, w64, tL2.as<float>(), t.Z.as<float>(), t.clist, t.clist + N, s, sh.items, sh.nitems))) return rc;   // T6
        if (shared && N > 1 && (rc = pn_zfill(N, N, t.Z.as<float>(), t.clist, t.clist + N, sh.rep, s))) return rc;
    }
    if ((rc = pn_m0(t.fps2, t.crowded, N, t.Z.as<float>(), t.M0.as<float>(), t.cl2.as<int>(), t.cnt2.as<int>(), z16,
                    bf16 ? t.M0_16.as<uint32_t>() : nullptr, t.clist, t.clist + N, t.cl2s.as<int>(), t.cl2o.as<unsigned short>(), s))) return rc;          // T7
    if ((rc = pn_pcf(t.fps1, t.cnt2.as<int>(), t.flags, N, t.pcf.as<int>(), s))) return rc;
    t.has_x = t.has_x16 = false;
    return xtab_policy == 1 ? build_xtab(oi, s) : DGDM_OK;       // eager only on request: see guidance_grad for when it pays
}

// T8: the embedding table of object oi in the format the trunk of the object's build mode reads (float32 for the parity path, bf16
// operand-order rows when the object was built in bf16 mode)
int DgdmGuidance::build_xtab(int oi, hipStream_t s) {
    const int N = cfg.num_object_points;
    ObjectTables &t = *tables[oi];
    if (N < 128) return DGDM_OK;
    const bool b16 = t.has16;
    int rc;
    if (b16) { if ((rc = t.X16.alloc((size_t)N * N * 128 * 4))) return rc; }
    else if ((rc = t.X.alloc((size_t)N * N * 256 * 4))) return rc;
    XtabObj xo{};
    xo.xyz = t.xyz; xo.fps1 = t.fps1; xo.Z = t.Z.as<float>(); xo.M0 = t.M0.as<float>();
    xo.Z16 = b16 ? t.Z16.as<uint32_t>() : nullptr; xo.M0_16 = b16 ? t.M0_16.as<uint32_t>() : nullptr;
    xo.clist = t.clist; xo.ncr = t.clist + N; xo.cl2s = t.cl2s.as<int>(); xo.cnt2 = t.cnt2.as<int>(); xo.flags = t.flags;
    xo.crowded = t.crowded; xo.X = b16 ? nullptr : t.X.as<float>(); xo.X16 = b16 ? t.X16.as<uint32_t>() : nullptr; xo.N = N;
    if ((rc = pn_xtab(xo, b16, s))) return rc;
    (b16 ? t.has_x16 : t.has_x) = true;
    return DGDM_OK;
}

extern "C" int dgdm_guidance_set_objects(DgdmGuidance *g, const float *objects_dev, int n_objects, void *stream) {
    DGDM_REQUIRE(g && objects_dev && n_objects > 0, DGDM_EINVAL, "dgdm_guidance_set_objects: bad argument");
    DGDM_REQUIRE(n_objects <= std::max(1, g->cfg.max_objects), DGDM_EINVAL, "%d objects > max_objects %d", n_objects, g->cfg.max_objects);
    hipStream_t s = (hipStream_t)stream;
    int rc;
    prof_begin(s, DGDM_STAGE_TABLES);
    if (g->m->kind == 2) {
        // (a grow-only member, not a local: a local's hipFree - and the synchronize that had to precede it - stalled the host behind
        //  the previous batch's chains at every call)
        if ((rc = g->objtmp.alloc((size_t)n_objects * 512 * 8))) return rc;
        if ((rc = g->m->object_part_2d64(objects_dev, g->objtmp.as<double>(), g->objpart.as<double>(), n_objects, s))) return rc;
        prof_end(s, DGDM_STAGE_TABLES, 0.0);
    } else {
        while ((int)g->tables.size() < n_objects) g->tables.emplace_back(new ObjectTables());
        const int N = g->cfg.num_object_points;
        if (g->vlist.bytes < (size_t)N * sizeof(int)) {
            std::vector<int> v(N);
            for (int i = 0; i < N; ++i) v[i] = i;
            if ((rc = g->vlist.upload(v.data(), sizeof(int) * N))) return rc;
        }
        // objects are independent: build them round-robin on a few side streams so the latency-bound stages (FPS: 512
        // dependent iterations on 128 workgroups) of one object overlap the bandwidth/MFMA-bound stages of the others
        const int nb = std::min<int>(DgdmGuidance::NBUILD, n_objects);
        // off the caller's stream (step schedule): only the copy of the coordinates stays on `s`; the FPS tables go to
        // the last build stream (a second one even for a single object: they run beside the light stages), and what reads the tables
        // later waits for the build's end (join_tables)
        const bool off = g->tables_off_stream();
        const int ns = off ? std::max(nb, 2) : nb;
        if (!off && (rc = g->join_tables(s))) return rc;      // an earlier build off this stream that nobody has joined yet
        if (!g->bstart) DGDM_HIP_CHECK(hipEventCreateWithFlags(&g->bstart, hipEventDisableTiming));
        if (!g->ldone) DGDM_HIP_CHECK(hipEventCreateWithFlags(&g->ldone, hipEventDisableTiming));
        for (int i = 0; i < ns; ++i) {
            if (!g->bstream[i]) DGDM_HIP_CHECK(hipStreamCreateWithFlags(&g->bstream[i], hipStreamNonBlocking));
            if (!g->bev[i]) DGDM_HIP_CHECK(hipEventCreateWithFlags(&g->bev[i], hipEventDisableTiming));
        }
        // T1 for every object at once (stream `fs` below): fps1[obj][start][512], fps2[obj][start point][128] + tie flags
        const size_t no = (size_t)n_objects;
        if ((rc = g->pool_xyz.alloc(no * N * 3 * 4)) || (rc = g->pool_fps1.alloc(no * N * 512 * sizeof(int))) ||
            (rc = g->pool_fps2.alloc(no * N * 128 * sizeof(int))) || (rc = g->pool_flags.alloc(no * N * sizeof(int))) ||
            (rc = g->pool_ncr.alloc(no * sizeof(int))) || (rc = g->pool_crowded.alloc(no * N * sizeof(int))) ||
            (rc = g->pool_clist.alloc(no * (N + 1) * sizeof(int))) || (rc = g->pool_off.alloc(no * (N + 1) * sizeof(int))) ||
            (rc = g->pool_pairs.alloc(no * N * N * sizeof(int))) || (rc = g->pool_rank.alloc(no * N * N * sizeof(short))) ||
            (rc = g->pool_F1.alloc(no * N * 128 * 8)) || (rc = g->pool_U.alloc(no * N * 128 * 8)) ||
            (rc = g->pool_fps1t.alloc(no * N * 64 * sizeof(uint4))))
            return rc;
        // the layer-1 tables of the f16x3 gradient trunk (built at the end, below): the float32 build's, for clouds the M0-only path serves.
        // Their pointer arrays [M0 | L1Z | L1K][max_objects] go up in front of `pooled`, which every build stream waits for (the buffers
        // never move - N and max_objects are the handle's - so a build still in flight reads the same values)
        const bool l1 = g->l1tab && !g->bf16 && N >= 128;
        const size_t l1mo = (size_t)std::max(1, g->cfg.max_objects);
        if (l1) {
            std::vector<const void *> ptrs(3 * l1mo, nullptr);
            for (int i = 0; i < (int)g->tables.size(); ++i) {
                ObjectTables &t = *g->tables[i];
                if ((rc = t.M0.alloc((size_t)N * 256 * 4)) || (rc = t.L1Z.alloc((size_t)N * 512 * 4)) || (rc = t.L1K.alloc((size_t)N * sizeof(int)))) return rc;
                ptrs[i] = t.M0.p; ptrs[l1mo + i] = t.L1Z.p; ptrs[2 * l1mo + i] = t.L1K.p;
            }
            if ((rc = g->l1objs.alloc(sizeof(void *) * ptrs.size()))) return rc;
            DGDM_HIP_CHECK(hipMemcpyAsync(g->l1objs.p, ptrs.data(), sizeof(void *) * ptrs.size(), hipMemcpyHostToDevice, s));      // pageable: staged before return
        }
        for (int i = 0; i < n_objects; ++i) g->tables[i]->has_l1 = l1;
        if (!g->pooled) DGDM_HIP_CHECK(hipEventCreateWithFlags(&g->pooled, hipEventDisableTiming));
        DGDM_HIP_CHECK(hipMemcpyAsync(g->pool_xyz.p, objects_dev, no * N * 3 * 4, hipMemcpyDeviceToDevice, s));
        DGDM_HIP_CHECK(hipEventRecord(g->pooled, s));
        hipStream_t fs = s;
        if (off) {
            // `pooled` lies behind everything the previous chains enqueued on `s` (their side-stream work is joined into `s` before
            // they return), so the build may overwrite the tables they read; a previous build nobody joined has ended at ro_ev
            fs = g->bstream[ns - 1];
            for (int i = 1; i < ns; ++i) {
                DGDM_HIP_CHECK(hipStreamWaitEvent(g->bstream[i], g->pooled, 0));
                if (g->built_once) DGDM_HIP_CHECK(hipStreamWaitEvent(g->bstream[i], g->ro_ev, 0));
            }
        }
        // sa2's FPS table is the first 128 columns of sa1's (same clouds, same starts): one pass writes both and the tie flags
        if ((rc = pn_fps_tables(g->pool_xyz.as<float>(), N, N, g->pool_fps1.as<int>(), g->pool_fps2.as<int>(), g->pool_flags.as<int>(), fs, n_objects)))
            return rc;
        // the float32 build's selection stage reads the table by position (variants on its lanes): a transposed copy behind it
        if (!g->bf16 && !g->l2_gather_mode && N <= 512 &&
            (rc = pn_fps_transpose(g->pool_fps1.as<int>(), N, g->pool_fps1t.as<uint4>(), fs, n_objects))) return rc;
        DGDM_HIP_CHECK(hipEventRecord(g->bstart, fs));
        // per-object completion events and the pinned target of the read-back (a copy of an earlier build into the old block has ended
        // at rb_ev before the block goes)
        while ((int)g->odone.size() < n_objects) {
            hipEvent_t e = nullptr;
            DGDM_HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
            g->odone.push_back(e);
        }
        if (!g->rb_ev) DGDM_HIP_CHECK(hipEventCreateWithFlags(&g->rb_ev, hipEventDisableTiming));
        if (!g->crowd_ev) DGDM_HIP_CHECK(hipEventCreateWithFlags(&g->crowd_ev, hipEventDisableTiming));
        const size_t ro_need = no * N + no;
        if (ro_need > g->ro_ints) {
            if (g->ro_host) { DGDM_HIP_CHECK(hipEventSynchronize(g->rb_ev)); DGDM_HIP_CHECK(hipHostFree(g->ro_host)); }
            g->ro_host = nullptr; g->ro_ints = 0;
            DGDM_HIP_CHECK(hipHostMalloc(reinterpret_cast<void **>(&g->ro_host), ro_need * sizeof(int), hipHostMallocDefault));
            g->ro_ints = ro_need;
        }
        for (int i = 0; i < n_objects; ++i) {
            ObjectTables &t = *g->tables[i];
            t.xyz = g->pool_xyz.as<float>() + (size_t)i * N * 3; t.fps1 = g->pool_fps1.as<int>() + (size_t)i * N * 512;
            t.fps2 = g->pool_fps2.as<int>() + (size_t)i * N * 128; t.flags = g->pool_flags.as<int>() + (size_t)i * N;
            t.crowded = g->pool_crowded.as<int>() + (size_t)i * N; t.clist = g->pool_clist.as<int>() + (size_t)i * (N + 1);
        }
        // the light, latency-bound stages - crowded flags + pair lists, T2 (sa1 features), T3 (U = sa2's first layer on the features) -
        // for ALL objects in one launch each (per object they are 1 .. 512 small workgroups: 130-500 us of a build stream each, a third
        // of its time), on the first build stream, beside the FPS tables; the heavy per-object stages (T4 .. T7) follow on the build streams
        {
            hipStream_t ls = g->bstream[0];
            DGDM_HIP_CHECK(hipStreamWaitEvent(ls, g->pooled, 0));          // the objects' coordinates are in the pool
            const PnWeights w = g->m->pn();
            if ((rc = pn_crowd(g->pool_xyz.as<float>(), N, w, g->pool_crowded.as<int>(), g->pool_clist.as<int>(), g->pool_clist.as<int>() + N,
                               g->pool_off.as<int>(), g->pool_pairs.as<int>(), g->pool_rank.as<short>(), ls, g->pool_ncr.as<int>(), n_objects)))
                return rc;
            DGDM_HIP_CHECK(hipEventRecord(g->crowd_ev, ls));               // the crowded-centre counts exist
            if (g->bf16) {
                if ((rc = pn_sa1(g->pool_xyz.as<float>(), N, w, g->pool_F1.as<float>(), ls, n_objects))) return rc;                                   // T2
                if ((rc = linear(g->pool_F1.as<float>(), 128, w.sa2_wf_t, w.sa2_b0, nullptr, 1, g->pool_U.as<float>(), 128, n_objects * N, 128, 128,
                                 ACT_NONE, false, ls))) return rc;                                                                                 // T3
            } else {
                const PnWeights64 w64 = g->m->pn64();
                if ((rc = pn_sa1_64(g->pool_xyz.as<float>(), N, w.r1sq, w64, g->pool_F1.as<double>(), ls, n_objects))) return rc;                      // T2
                if ((rc = linear64(nullptr, g->pool_F1.as<double>(), 128, w64.sa2_wf_t, w64.sa2_b0, nullptr, 1, g->pool_U.as<double>(), nullptr, 128,
                                   n_objects * N, 128, 128, ACT_NONE, ls))) return rc;                                                             // T3
            }
            DGDM_HIP_CHECK(hipEventRecord(g->ldone, ls));
        }
        // which objects may use the table of FPS(128) sequences (no order-dependent selection anywhere); crowded-centre counts: copied
        // to pinned memory behind rb_ev, read by finish_objects() when first needed.  Off the caller's stream they go as soon as both
        // exist: on the FPS stream right behind the tables (pool_flags) and behind the first light stage (pool_ncr), in front of that
        // stream's heavy stages - the host can plan the chains' gathers while those run
        auto read_back = [&](hipStream_t rs) -> int {
            DGDM_HIP_CHECK(hipMemcpyAsync(g->ro_host, g->pool_flags.p, sizeof(int) * no * N, hipMemcpyDeviceToHost, rs));
            DGDM_HIP_CHECK(hipMemcpyAsync(g->ro_host + no * N, g->pool_ncr.p, sizeof(int) * no, hipMemcpyDeviceToHost, rs));
            DGDM_HIP_CHECK(hipEventRecord(g->rb_ev, rs));
            return DGDM_OK;
        };
        if (off) {
            DGDM_HIP_CHECK(hipStreamWaitEvent(fs, g->crowd_ev, 0));
            if ((rc = read_back(fs))) return rc;
        }
        for (int i = 0; i < nb; ++i) {       // the heavy stages need the FPS tables (bstart) and the light stages' outputs
            DGDM_HIP_CHECK(hipStreamWaitEvent(g->bstream[i], g->bstart, 0));
            DGDM_HIP_CHECK(hipStreamWaitEvent(g->bstream[i], g->ldone, 0));
        }
        for (int i = 0; i < n_objects; ++i) {
            if ((rc = g->build_object(i, i % nb, g->bstream[i % nb]))) return rc;
            // the object's tables are complete: the gather of its chains' rows may start (run_xobj).  The stream waited for bstart and
            // ldone, so the pool's parts of the object (fps1, clist, ..) are covered too
            DGDM_HIP_CHECK(hipEventRecord(g->odone[i], g->bstream[i % nb]));
        }
        // the build's end: on the caller's stream, or (off it) on bstream[0], which has the FPS stream behind it through bstart
        hipStream_t es = off ? g->bstream[0] : s;
        for (int i = off ? 1 : 0; i < nb; ++i) {
            DGDM_HIP_CHECK(hipEventRecord(g->bev[i], g->bstream[i]));
            DGDM_HIP_CHECK(hipStreamWaitEvent(es, g->bev[i], 0));
        }
        // every object's M0 and crowded count exist: the layer-1 tables of the uncrowded ones, all objects in one launch (in front of ro_ev:
        // join_tables covers it)
        if (l1) {
            void *const *po = g->l1objs.as<void *>();
            if ((rc = trunk_f16l_l1_tables(reinterpret_cast<const float *const *>(po), g->pool_ncr.as<int>(), reinterpret_cast<float *const *>(po + l1mo),
                                           reinterpret_cast<int *const *>(po + 2 * l1mo), N, n_objects, g->m->fwdh(), es))) return rc;
        }
        prof_end(s, DGDM_STAGE_TABLES, 0.0);
        if (!off && (rc = read_back(es))) return rc;
        // ro_ev: the END of the build (join_tables, the next build, the destructor), whatever the place of the read-back.  It has the
        // early read-back behind it as well (long complete by then): the next build's, possibly on another stream, cannot overtake it
        if (off) DGDM_HIP_CHECK(hipStreamWaitEvent(es, g->rb_ev, 0));
        if (!g->ro_ev) DGDM_HIP_CHECK(hipEventCreateWithFlags(&g->ro_ev, hipEventDisableTiming));
        DGDM_HIP_CHECK(hipEventRecord(g->ro_ev, es));
        g->ro_pending = true;
        g->built_once = true; g->built_off_stream = off; g->join_pending = off;
    }
    g->n_objects = n_objects;
    g->grads_since_set = 0;
    return DGDM_OK;
}

// ------------------------------------------------------------------------------------------------ shared front end
// V/genc from x, timepart(t), chain bias (2-D: object part + time part), A table.
int DgdmGuidance::common_pre(const float *x_dev, float t_scaled, const int *objidx_host, int n_chains, hipStream_t s) {
    const int rows = n_chains * B, W1 = m->W1;
    int rc;
    if ((rc = m->gripper_forward64(x_dev, m->L, V.as<double>(), genc.as<double>(), rows, s))) return rc;
    if ((rc = m->time_part64(t_scaled, ttmp.as<float>(), ttmp64.as<double>(), timepart.as<double>(), s))) return rc;
    if (m->kind == 2) {
        DGDM_HIP_CHECK(hipMemcpyAsync(objidx.p, objidx_host, sizeof(int) * n_chains, hipMemcpyHostToDevice, s));   // pageable: staged before return
        if ((rc = gather_add64(objpart.as<double>(), objidx.as<int>(), timepart.as<double>(), chainbias.as<double>(), n_chains, W1, s))) return rc;
        return linear64(nullptr, genc.as<double>(), 256, m->blob64.at(m->off64.w1c_wt), nullptr, chainbias.as<double>(), B, nullptr, atab.as<float>(), W1, rows, 256, W1,
                        ACT_NONE, s);
    }
    return linear64(nullptr, genc.as<double>(), 256, m->blob64.at(m->off64.w1c_wt), timepart.as<double>(), nullptr, 1, nullptr, atab.as<float>(), W1, rows, 256, W1,
                    ACT_NONE, s);
}

// Reference draw order per chain: for each sub-batch i, sa1's torch.randint(rows_i) then sa2's  ->  device [chain][row][2]
int DgdmGuidance::finish_objects() {
    if (!ro_pending) return DGDM_OK;
    DGDM_HIP_CHECK(hipEventSynchronize(rb_ev));      // the read-back alone: the build may still be running
    const int N = cfg.num_object_points;
    for (int i = 0; i < n_objects; ++i) {
        bool ok = N >= 128;
        for (int k = 0; k < N; ++k) ok = ok && ro_host[(size_t)i * N + k] == 0;
        tables[i]->fast_ok = ok;
        tables[i]->ncr = ro_host[(size_t)n_objects * N + i];
    }
    ro_pending = false;
    return DGDM_OK;
}

int DgdmGuidance::ensure_rows(int n_chains, int64_t rows_per_chain) {
    const int N = cfg.num_object_points;
    const size_t nr = (size_t)n_chains * rows_per_chain;
    int rc;
    // (the embedding rows themselves - xobj / xobj16, 1 KiB / 512 B per row - are allocated by run_xobj, the only path that writes them:
    // with the embedding tables X[s1][q] in place a call gathers nothing)
    if ((rc = starts.alloc(nr * 2 * sizeof(int))) || (rc = order.alloc(nr * sizeof(int))) ||
        (rc = todo.alloc((nr + 1) * sizeof(int))) || (rc = xidx.alloc(nr * sizeof(int))))
        return rc;
    todo_capacity = (int64_t)nr;
    const size_t need = (nr * 3 + (size_t)n_chains * (N + 1)) * sizeof(int);
    if (need > pinned_bytes) {
        if (pinned) { DGDM_HIP_CHECK(hipEventSynchronize(pinned_ev)); DGDM_HIP_CHECK(hipHostFree(pinned)); pinned = nullptr; pinned_bytes = 0; }
        DGDM_HIP_CHECK(hipHostMalloc(&pinned, need, hipHostMallocDefault));
        pinned_bytes = need;
    }
    return DGDM_OK;
}

int DgdmGuidance::upload_starts(const int64_t *starts_host, int n_chains, int64_t rows, hipStream_t s, bool need_order, int n_calls,
                                int64_t call_stride, bool on_launch_stream) {
    const int N = cfg.num_object_points;
    const int64_t sb = cfg.sub_batch_size;
    const int64_t rt = rows * n_calls;                         // rows per chain on the device
    int rc;
    DGDM_REQUIRE(!need_order || rt < ((int64_t)1 << 22), DGDM_EINVAL, "%lld rows per chain in one gather launch (limit 4194303)", (long long)rt);
    if ((rc = ensure_rows(n_chains, rt))) return rc;
    DGDM_HIP_CHECK(hipEventSynchronize(pinned_ev));            // previous copy out of the staging buffer has finished
    int *dst = static_cast<int *>(pinned);
    int *ord = dst + (size_t)n_chains * 2 * rt;
    int *goff = ord + (size_t)n_chains * rt;                   // [n_chains][N+1]: where each s1-group starts in the chain's sorted rows
    // per chain: int64 draws -> (s1, s2) int32 pairs in row order; rows sorted by s1 (counting sort) so that the rows of one
    // variant gather from the same Z slab; group offsets.  Chains are independent: a few host threads share them.
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
    if (!cstream) {
        DGDM_HIP_CHECK(hipStreamCreateWithFlags(&cstream, hipStreamNonBlocking));
        DGDM_HIP_CHECK(hipEventCreateWithFlags(&up_ready, hipEventDisableTiming));
        DGDM_HIP_CHECK(hipEventCreateWithFlags(&up_consumed, hipEventDisableTiming));
    }
    // the copy may start as soon as the previous readers of the device buffers (the last gather / index kernel on the launch stream)
    // are done - not behind everything queued on the launch stream since.
    // on_launch_stream (the gathers start beside a table build still in flight, run_xobj): the copies go on `s` itself.  The process
    // has more streams than hardware queues, and up_ready's marker on the upload stream was seen to come out only behind the LAST
    // kernel of the build stream whose queue it shares - the gathers then started at the build's end whatever they waited for
    // (DESIGN.md 4.3b).  `s` has nothing else to run until the build ends, so the copy costs the gathers' start, not the step.
    hipStream_t us = on_launch_stream ? s : cstream;
    if (consumed_recorded) DGDM_HIP_CHECK(hipStreamWaitEvent(us, up_consumed, 0));
    if (need_order) {         // what the gathers read first
        DGDM_HIP_CHECK(hipMemcpyAsync(order.p, ord, (size_t)n_chains * rt * sizeof(int), hipMemcpyHostToDevice, us));
        DGDM_HIP_CHECK(hipMemcpyAsync(groupoff.p, goff, (size_t)n_chains * (N + 1) * sizeof(int), hipMemcpyHostToDevice, us));
    }
    DGDM_HIP_CHECK(hipMemcpyAsync(starts.p, pinned, (size_t)n_chains * rt * 2 * sizeof(int), hipMemcpyHostToDevice, us));
    DGDM_HIP_CHECK(hipEventRecord(pinned_ev, us));
    if (!on_launch_stream) {
        DGDM_HIP_CHECK(hipEventRecord(up_ready, cstream));
        DGDM_HIP_CHECK(hipStreamWaitEvent(s, up_ready, 0));
    }
    return DGDM_OK;
}

// The layer-1 tables of the chains in of_chain (null: the chain does not read its object's float32 M0) and the chain list -> l1ptrs;
// *n_tabled: how many chains have a table (0: nothing was uploaded)
int DgdmGuidance::fill_l1ptrs(const std::vector<const ObjectTables *> &of_chain, int *n_tabled, hipStream_t s) {
    const int nc = cfg.max_chains;
    std::vector<const void *> ptrs(3 * (size_t)nc, nullptr);                       // [L1Z | L1K][nc] pointers, then the chain list [nc] ints
    int *list = reinterpret_cast<int *>(ptrs.data() + 2 * (size_t)nc);
    std::vector<int> rest;
    int nt = 0;
    for (size_t i = 0; i < of_chain.size(); ++i) {
        const ObjectTables *t = of_chain[i];
        if (!t || !l1tab || !t->has_l1 || t->ncr != 0) { rest.push_back((int)i); continue; }
        ptrs[i] = t->L1Z.p; ptrs[nc + i] = t->L1K.p;
        list[nt++] = (int)i;
    }
    std::copy(rest.begin(), rest.end(), list + nt);
    *n_tabled = nt;
    if (nt) DGDM_HIP_CHECK(hipMemcpyAsync(l1ptrs.p, ptrs.data(), sizeof(void *) * ptrs.size(), hipMemcpyHostToDevice, s));      // pageable: staged before return
    return DGDM_OK;
}

int DgdmGuidance::use_xtab(const int *objidx_host, int n_chains, int64_t rows, bool want16, int *l1, hipStream_t s) {
    std::vector<XidxChain> xc(n_chains);
    std::vector<const void *> base(n_chains);
    std::vector<const ObjectTables *> m0_of(n_chains, nullptr);      // chains that read their object's float32 M0
    for (int i = 0; i < n_chains; ++i) {
        const ObjectTables &t = *tables[objidx_host[i]];
        xc[i].fps1 = t.fps1; xc[i].N = cfg.num_object_points; xc[i].m0_only = t.ncr == 0;
        // an object without crowded centres has X[s1][q] = M0[q]: its table is M0 itself (xtab_kernel wrote nothing)
        base[i] = want16 ? (t.ncr == 0 ? (const void *)t.M0_16.p : (const void *)t.X16.p) : (t.ncr == 0 ? (const void *)t.M0.p : (const void *)t.X.p);
        if (!want16 && t.ncr == 0) m0_of[i] = &t;
    }
    int rc;
    if ((rc = fill_l1ptrs(m0_of, l1, s))) return rc;
    DGDM_HIP_CHECK(hipMemcpyAsync(xidxchains.p, xc.data(), sizeof(XidxChain) * n_chains, hipMemcpyHostToDevice, s));      // pageable: staged before return
    DGDM_HIP_CHECK(hipMemcpyAsync(xtabptrs.p, base.data(), sizeof(void *) * n_chains, hipMemcpyHostToDevice, s));
    return pn_xidx(xidxchains.as<XidxChain>(), starts.as<int>(), rows, n_chains, xidx.as<int>(), s);
}

int DgdmGuidance::run_xobj(const int *objidx_host, int n_chains, int64_t rows, bool want16, bool *used16, bool *via_tab, int *l1, hipStream_t s) {
    *via_tab = false;
    *l1 = 0;
    std::vector<XobjChain> ch(n_chains);
    for (int i = 0; i < n_chains; ++i) {
        const ObjectTables &t = *tables[objidx_host[i]];
        ch[i].xyz = t.xyz; ch[i].fps1 = t.fps1; ch[i].slot_of_start = nullptr; ch[i].Z = t.Z.as<float>();
        ch[i].fps2 = t.fps2; ch[i].flags = t.flags; ch[i].crowded = t.crowded; ch[i].N = cfg.num_object_points;
        ch[i].M0 = t.M0.as<float>(); ch[i].cl2 = t.cl2.as<int>(); ch[i].cnt2 = t.cnt2.as<int>();
        ch[i].Z16 = t.has16 ? t.Z16.as<uint32_t>() : nullptr; ch[i].M0_16 = t.has16 ? t.M0_16.as<uint32_t>() : nullptr;
        want16 = want16 && t.has16;          // bf16 rows only if every chain's object was built with its bf16 tables
    }
    {   // grow-only buffers (a run's embeds have the same size, or shrink at its tail: no reallocation under kernels in flight)
        const size_t nrows = (size_t)n_chains * rows;
        int rc = want16 ? xobj16.alloc(nrows * 512) : xobj.alloc(nrows * 256 * 4);
        if (rc) return rc;
    }
    *used16 = want16;
    XobjParams xp{};
    xp.chains = xchains.as<XobjChain>(); xp.starts = starts.as<int>(); xp.order = order.as<int>(); xp.xobj = xobj.as<float>();
    xp.xobj16 = want16 ? xobj16.as<uint32_t>() : nullptr;
    xp.R = rows; xp.total_rows = rows * n_chains; xp.use_table = force_slow_xobj ? 0 : 1;
    xp.todo = todo.as<int>(); xp.todo_count = todo.as<int>() + todo_capacity; xp.todo_capacity = todo_capacity;
    bool all_fast = true;
    for (int i = 0; i < n_chains; ++i) all_fast = all_fast && tables[objidx_host[i]]->fast_ok;
    // group kernel: every chain needs its tables and a slab chunk that fits LDS (it handles tie-flagged start points itself)
    bool groups = !force_slow_xobj && xobj_mode == 0 && cfg.num_object_points >= 128;
    for (int i = 0; i < n_chains && groups; ++i) {
        const ObjectTables &t = *tables[objidx_host[i]];
        const int lpr = xobj_rows_lpr(t.ncr, want16);
        groups = lpr > 0 && want16 == t.has16;     // the slot offsets are scaled for the build's mode
        ch[i].clist = t.clist; ch[i].cl2s = t.cl2s.as<int>(); ch[i].cl2o = t.cl2o.as<unsigned short>(); ch[i].pcf = t.pcf.as<int>(); ch[i].ncr = t.ncr; ch[i].lpr = lpr;
    }
    // only the group kernel's launches start ahead of the build's end (below); everything else reads the tables behind the join
    const bool early = groups && gather_early(s);
    if (!early) {
        int rc = join_tables(s);
        if (rc) return rc;
    }
    DGDM_HIP_CHECK(hipMemcpyAsync(xchains.p, ch.data(), sizeof(XobjChain) * n_chains, hipMemcpyHostToDevice, s));     // pageable: staged before return
    if (groups) {
        // A chain whose object has no crowded centre and no tie-flagged start has M0[q] as the embedding of every row (use_xtab): it gets no
        // work items and its block of xobj is never written.  The trunk then reads EVERY chain of the launch through a table and a row
        // index: such a chain M0 at q = fps1[s1][s2], a gathered chain its own block of xobj at the row's number.  Not when the test hook
        // asks for materialised rows (modes 1-3), nor for the bf16 trunk on float32 rows (it has no float32 table form).
        const bool by_index = tables_wanted() && (want16 || !bf16);
        std::vector<int> rank;
        std::vector<XidxChain> xc(n_chains);
        std::vector<const void *> base(n_chains);
        std::vector<const ObjectTables *> m0_of(n_chains, nullptr);      // chains that read their object's float32 M0
        for (int i = 0; i < n_chains; ++i) {
            const ObjectTables &t = *tables[objidx_host[i]];
            const bool m0_only = by_index && t.ncr == 0 && t.fast_ok;
            if (!m0_only) rank.push_back(i);
            if (m0_only && !want16) m0_of[i] = &t;
            xc[i].fps1 = m0_only ? t.fps1 : nullptr; xc[i].N = cfg.num_object_points; xc[i].m0_only = 1;
            base[i] = m0_only ? (want16 ? (const void *)t.M0_16.p : (const void *)t.M0.p)
                              : (want16 ? (const void *)(xobj16.as<uint32_t>() + (size_t)i * rows * 128) : (const void *)(xobj.as<float>() + (size_t)i * rows * 256));
        }
        xp.group_off = groupoff.as<int>(); xp.nchain = n_chains; xp.group_N = cfg.num_object_points; xp.use_table = 1;
        auto index = [&]() -> int {          // what the trunk reads the chains through; the index kernel reads fps1 and the draws only
            int rc;
            *via_tab = true;
            DGDM_HIP_CHECK(hipMemcpyAsync(xidxchains.p, xc.data(), sizeof(XidxChain) * n_chains, hipMemcpyHostToDevice, s));      // pageable: staged before return
            DGDM_HIP_CHECK(hipMemcpyAsync(xtabptrs.p, base.data(), sizeof(void *) * n_chains, hipMemcpyHostToDevice, s));
            if ((rc = fill_l1ptrs(m0_of, l1, s))) return rc;
            return pn_xidx(xidxchains.as<XidxChain>(), starts.as<int>(), rows, n_chains, xidx.as<int>(), s);
        };
        int rc;
        if (!early) {                        // one launch over all chains behind the joined build
            xp.total_items = (int)rank.size() * xp.group_N;
            std::stable_sort(rank.begin(), rank.end(), [&](int a, int b) { return ch[a].ncr > ch[b].ncr; });
            for (size_t i = 0; i < rank.size(); ++i) xp.chain_of_rank[i] = (unsigned char)rank[i];
            if ((rc = pn_xobj_groups(xp, s)) || !by_index) return rc;
            return index();
        }
        // Step schedule: the build is still running on its streams and `s` has not joined it.  A chain's rows are gathered
        // from its own object's tables alone, so they start behind that object's odone and run beside the float64 stages of the objects
        // still being built: one launch per object with gathered chains, in the order in which the builds end (object index order, round-
        // robin over the build streams).  All of them are on `s`, so what is recorded on `s` afterwards lies behind every gather:
        // up_consumed (embed_rows), the next set_objects' `pooled` (it may overwrite tables and pool), the previous run's trunk that
        // read xobj lies in front.  The launches append to ONE list of tie-flagged rows, emptied once; those rows (they read the
        // tables of any chain), and the trunk's reads of M0 / L1Z, come behind join_tables(s) - which is reached on every way out,
        // an error half way included, so that nothing enqueued here is left un-joined.
        auto gathers = [&]() -> int {
            int rc;
            if (by_index) {                  // the index kernel needs the FPS tables, nothing of the heavy stages
                DGDM_HIP_CHECK(hipStreamWaitEvent(s, bstart, 0));
                if ((rc = index())) return rc;
            }
            if (rank.empty()) return DGDM_OK;
            if ((rc = pn_xobj_groups_begin(xp, s))) return rc;
            for (int o = 0; o < n_objects; ++o) {
                int n = 0;                   // (the chains of one object have the same ncr: no heaviest-first order within a launch)
                for (int c : rank)
                    if (objidx_host[c] == o) xp.chain_of_rank[n++] = (unsigned char)c;
                if (!n) continue;
                xp.total_items = n * xp.group_N;
                DGDM_HIP_CHECK(hipStreamWaitEvent(s, odone[o], 0));
                if ((rc = pn_xobj_groups_rows(xp, s))) return rc;
            }
            return DGDM_OK;
        };
        rc = gathers();
        const int jrc = join_tables(s);
        if (rc || jrc) return rc ? rc : jrc;
        return rank.empty() ? DGDM_OK : pn_xobj_groups_ties(xp, s);
    }
    return pn_xobj(xp, all_fast, s);
}

// The PointNet++ embeddings of the rows of `n_calls` consecutive classifier calls (3-D).  They depend on the FPS start draws and the
// objects only - not on x - so a whole denoise loop's (or roll-out's) worth can be made before its first step: one upload and ONE gather
// launch whose (chain, s1) groups hold the rows of all the calls (the variant's slab is staged once for five times the rows; beside a
// table build still in flight the launch is cut by object, each part behind its object's tables: run_xobj), or - when
// every chain's object has its embedding table in the wanted format (float32, or bf16 operand-order rows: want16) - one index kernel.
// Call k then reads rows [k * rows_per_call, (k + 1) * rows_per_call) of every chain (Embedded::point).
int DgdmGuidance::embed_rows(const int *oidx, int n_chains, const int64_t *starts_host, int64_t rows_per_call, int n_calls, int64_t call_stride,
                             bool want16, Embedded *e, hipStream_t s) {
    bool tab = tables_wanted();
    for (int i = 0; i < n_chains && tab; ++i) tab = want16 ? tables[oidx[i]]->has_x16 : tables[oidx[i]]->has_x;   // else: built in the other format, or not at all
    const int64_t rt = rows_per_call * n_calls;
    int rc;
    // Every reader of the tables joins the build (join_tables) in front of its first read: the embedding-table path here, run_xobj
    // where its kernels need the whole build (its per-object gathers start earlier, see there), embed() in front of a build_xtab.  Every
    // way through this function ends joined, so the trunk's reads of M0 / L1Z through xtabptrs / l1ptrs are covered.
    if (tab && (rc = join_tables(s))) return rc;
    if ((rc = upload_starts(starts_host, n_chains, rows_per_call, s, !tab, n_calls, call_stride, !tab && gather_early(s)))) return rc;     // host work: overlaps a table build still in flight
    if ((rc = finish_objects())) return rc;
    e->tab = tab; e->used16 = want16; e->rows_per_chain = rt;
    if ((rc = tab ? use_xtab(oidx, n_chains, rt, want16, &e->l1, s) : run_xobj(oidx, n_chains, rt, want16, &e->used16, &e->tab, &e->l1, s))) return rc;
    DGDM_HIP_CHECK(hipEventRecord(up_consumed, s));          // the index buffers may be overwritten once these kernels are through
    consumed_recorded = true;
    return DGDM_OK;
}

// Points the trunk at call `call`'s rows of the run
void DgdmGuidance::Embedded::point(TrunkParams *p, const DgdmGuidance &g, int call, int64_t rows_per_call) const {
    const size_t row0 = (size_t)call * rows_per_call;
    p->xstride = rows_per_chain;
    if (tab) {
        p->xidx = g.xidx.as<int>() + row0;
        if (used16) p->xtab16 = g.xtabptrs.as<const uint32_t *>();
        else p->xtab = g.xtabptrs.as<const float *>();
        if (l1 && !used16) {                     // read by the f16x3 gradient trunk alone
            p->l1z = g.l1ptrs.as<const float *>();
            p->l1k = g.l1ptrs.as<const int *>() + g.cfg.max_chains;
            p->chainlist = reinterpret_cast<const int *>(g.l1ptrs.as<const void *>() + 2 * (size_t)g.cfg.max_chains);
            p->n_tabled = l1;
        }
    } else {
        p->xobj = g.xobj.as<float>() + row0 * 256;
        p->xobj16 = used16 ? g.xobj16.as<uint32_t>() + row0 * 128 : nullptr;
    }
}

int DgdmGuidance::embed(const int *oidx, int n_chains, const int64_t *starts_host, int n_calls, int64_t call_stride, Embedded *e, hipStream_t s) {
    DGDM_REQUIRE(starts_host, DGDM_EINVAL, "3-D guidance needs the FPS start indices");
    int rc;
    if (prof_on() && (rc = join_tables(s))) return rc;      // the stage's events bracket the gather, not a wait for the build
    prof_begin(s, DGDM_STAGE_XOBJ);
    // The table X[s1][q] of an object costs about what 7 cond_fn calls spend gathering its rows (it holds all 262 144 (s1, q)
    // pairs; one call touches 36 000 of them): it pays as soon as the objects serve more than one 5-step chain - the
    // reference's validation sweep runs 12 objectives x 5 steps (+ the multi-object chains) on the same objects - and it would
    // cost 2 % when every pair brings its own object (bench.py).  So it is built when the call count says the objects are being
    // reused: when the calls since set_objects pass XTAB_AFTER.
    if (tables_wanted()) {
        const bool crosses = grads_since_set <= XTAB_AFTER && grads_since_set + n_calls > XTAB_AFTER;
        grads_since_set += n_calls;
        if (crosses && (rc = join_tables(s))) return rc;      // build_xtab reads the finished tables
        if (crosses)
            for (int i = 0; i < n_objects; ++i) {
                ObjectTables &t = *tables[i];
                if (!(t.has16 ? t.has_x16 : t.has_x) && (rc = build_xtab(i, s))) return rc;
            }
    }
    if ((rc = embed_rows(oidx, n_chains, starts_host, grid.rows, n_calls, call_stride, bf16, e, s))) return rc;
    prof_end(s, DGDM_STAGE_XOBJ, 0.0);
    return DGDM_OK;
}

int DgdmGuidance::trunk_front(int kind, const float *x_dev, int timestep, const int *oidx, const int64_t *starts_host, int n_chains, const Embedded *emb,
                              int call, TrunkParams *pp, hipStream_t s, bool pre_done) {
    const float t_scaled = (float)timestep / (float)cfg.num_train_timesteps;      // timesteps.float() / T  (diffusion.py:487,496)
    int rc;
    if ((rc = check_objects(oidx, n_chains))) return rc;
    if (!pre_done) {
        prof_begin(s, DGDM_STAGE_GUIDE_MISC);
        if ((rc = common_pre(x_dev, t_scaled, oidx, n_chains, s))) return rc;
        prof_end(s, DGDM_STAGE_GUIDE_MISC, 0.0);
    }
    m->fill_trunk(pp);
    set_grid(pp, grid, n_chains);
    if (kind == 3) {
        Embedded own;
        if (!emb) {
            if ((rc = embed(oidx, n_chains, starts_host, 1, 0, &own, s))) return rc;
            emb = &own;
            call = 0;
        }
        emb->point(pp, *this, call, grid.rows);
    }
    return DGDM_OK;
}

// What a launch's objectives need of the per-row inputs, checked before anything is enqueued: the trunk reads rowcoef / field rows of
// chain i without looking again
static int check_objectives(const DgdmGuidance *g, const DgdmObjective *objectives, const float *rowcoef_dev, int n_chains) {
    for (int i = 0; i < n_chains; ++i) {
        const int u = objectives[i].use_rowcoef;
        DGDM_REQUIRE(u >= 0 && u <= DGDM_OBJ_ROWFIELD, DGDM_EINVAL, "chain %d: use_rowcoef %d (0, 1 or %d)", i, u, DGDM_OBJ_ROWFIELD);
        DGDM_REQUIRE(u != 1 || rowcoef_dev, DGDM_EINVAL, "chain %d uses rowcoef but rowcoef_dev is null", i);
        if (u == DGDM_OBJ_ROWFIELD) {
            DGDM_REQUIRE(g->rowfield, DGDM_EINVAL, "chain %d uses the row field but none is set (dgdm_guidance_set_row_field)", i);
            DGDM_REQUIRE(i < g->rowfield_chains, DGDM_EINVAL, "chain %d uses the row field, which was set for %d chains", i, g->rowfield_chains);
        }
    }
    return DGDM_OK;
}

// cond_fn for n_chains chains.  3-D: `emb` = the embeddings made by DgdmGuidance::embed for a run of calls, `call` = which of them this is;
// emb == nullptr: this call's own (starts_host = its draws).
static int guidance_grad(DgdmGuidance *g, int kind, const float *x_dev, int timestep, const DgdmObjective *objectives, const float *rowcoef_dev,
                         const int64_t *starts_host, int n_chains, float *grad_dev, hipStream_t s, const DgdmGuidance::Embedded *emb = nullptr,
                         int call = 0, bool pre_done = false) {
    DGDM_REQUIRE(g && x_dev && objectives && grad_dev, DGDM_EINVAL, "guidance_grad: null argument");
    if (g->m->kind != kind) { set_error("model type not supported: %d-D entry point on a %d-D model", kind, g->m->kind); return DGDM_EMODE; }
    DGDM_REQUIRE(n_chains > 0 && n_chains <= g->cfg.max_chains, DGDM_EINVAL, "n_chains %d outside 1..%d", n_chains, g->cfg.max_chains);
    int rc;
    if ((rc = check_objectives(g, objectives, rowcoef_dev, n_chains))) return rc;
    std::vector<int> oidx(n_chains);
    std::vector<TrunkObjective> tob(n_chains);
    for (int i = 0; i < n_chains; ++i) {
        oidx[i] = objectives[i].object;
        for (int j = 0; j < 3; ++j) { tob[i].lin[j] = objectives[i].lin[j]; tob[i].quad[j] = objectives[i].quad[j]; }
        tob[i].use_rowcoef = objectives[i].use_rowcoef; tob[i].pad = 0;
    }
    TrunkParams p;
    if ((rc = g->trunk_front(kind, x_dev, timestep, oidx.data(), starts_host, n_chains, emb, call, &p, s, pre_done))) return rc;
    DGDM_HIP_CHECK(hipMemcpyAsync(g->objdev.p, tob.data(), sizeof(TrunkObjective) * n_chains, hipMemcpyHostToDevice, s));
    p.obj = g->objdev.as<TrunkObjective>(); p.rowcoef = rowcoef_dev; p.rowfield = g->rowfield;
    p.partial = g->partial.as<float>();
    if (g->bf16) {
        g->m->fill_trunk_bf16(&p);       // only the two weight streams differ
        if ((rc = trunk_bf16_launch(kind, p, s))) return rc;
    } else if (g->f32_mfma) {
        if ((rc = trunk_launch(kind, false, false, p, s))) return rc;
    } else {
        TrunkF16Scales sc;
        g->m->fill_trunk_f16(&p, &sc);   // only the two weight streams differ (+ their scale exponents)
        if ((rc = trunk_f16l_launch(kind, TrunkF16Mode::Grad, p, sc, s))) return rc;
    }
    prof_begin(s, DGDM_STAGE_GUIDE_MISC);
    rc = dyn_post64(g->m->W1, g->partial.as<float>(), g->grid.tiles_per_b, g->m->blob64.at(g->m->off64.w1c_w), g->m->blob64.at(g->m->off64.g2_w),
                    g->m->blob64.at(g->m->off64.g0_w), g->V.as<double>(), grad_dev, n_chains * g->B, g->m->L, s);
    prof_end(s, DGDM_STAGE_GUIDE_MISC, 0.0);
    return rc;
}

extern "C" int dgdm_dyn2d_guidance_grad(DgdmGuidance *g, const float *x_dev, int timestep, const DgdmObjective *objectives,
                                        const float *rowcoef_dev, int n_chains, float *grad_dev, void *stream) {
    return guidance_grad(g, 2, x_dev, timestep, objectives, rowcoef_dev, nullptr, n_chains, grad_dev, (hipStream_t)stream);
}

extern "C" int dgdm_dyn3d_guidance_grad(DgdmGuidance *g, const float *x_dev, int timestep, const DgdmObjective *objectives,
                                        const float *rowcoef_dev, const int64_t *starts_host, int n_chains, float *grad_dev, void *stream) {
    return guidance_grad(g, 3, x_dev, timestep, objectives, rowcoef_dev, starts_host, n_chains, grad_dev, (hipStream_t)stream);
}

extern "C" int dgdm_guidance_set_row_field(DgdmGuidance *g, const float *field_dev, int n_chains, void *stream) {
    (void)stream;                                             // nothing is enqueued: the pointer is kept and read by later launches
    DGDM_REQUIRE(g, DGDM_EINVAL, "dgdm_guidance_set_row_field: null handle");
    if (!field_dev) { g->rowfield = nullptr; g->rowfield_chains = 0; return DGDM_OK; }
    DGDM_REQUIRE(n_chains > 0 && n_chains <= g->cfg.max_chains, DGDM_EINVAL, "dgdm_guidance_set_row_field: n_chains %d outside 1..%d", n_chains,
                 g->cfg.max_chains);
    g->rowfield = field_dev; g->rowfield_chains = n_chains;
    return DGDM_OK;
}

extern "C" int dgdm_guidance_goal_field(DgdmGuidance *g, const float *goals_dev, const DgdmGoalSpec *specs_host, int n_chains, float *field_dev,
                                        void *stream) {
    DGDM_REQUIRE(g && goals_dev && specs_host && field_dev, DGDM_EINVAL, "dgdm_guidance_goal_field: null argument");
    DGDM_REQUIRE(n_chains > 0 && n_chains <= g->cfg.max_chains, DGDM_EINVAL, "dgdm_guidance_goal_field: n_chains %d outside 1..%d", n_chains,
                 g->cfg.max_chains);
    hipStream_t s = (hipStream_t)stream;
    for (int i = 0; i < n_chains; ++i) {
        const DgdmGoalSpec &q = specs_host[i];
        DGDM_REQUIRE(q.ori_window > 0.f && q.ori_window <= 1.f, DGDM_EINVAL, "goal %d: ori_window %g outside (0, 1]", i, (double)q.ori_window);
        DGDM_REQUIRE(q.pos_window > 0.f && std::isfinite(q.pos_window), DGDM_EINVAL, "goal %d: pos_window %g is not a positive number", i, (double)q.pos_window);
        DGDM_REQUIRE(q.profile == 0 || q.profile == 1, DGDM_EINVAL, "goal %d: profile %d (0 sign, 1 linear)", i, q.profile);
        for (int j = 0; j < 3; ++j) DGDM_REQUIRE(std::isfinite(q.weight[j]), DGDM_EINVAL, "goal %d: weight %d is not finite", i, j);
    }
    // the goals may come from a device-side sweep: they are read back once to refuse a non-finite one (the builder is not a hot path)
    std::vector<float> goals((size_t)n_chains * g->B * 3);
    DGDM_HIP_CHECK(hipMemcpyAsync(goals.data(), goals_dev, goals.size() * sizeof(float), hipMemcpyDeviceToHost, s));
    DGDM_HIP_CHECK(hipStreamSynchronize(s));
    for (size_t k = 0; k < goals.size(); ++k)
        DGDM_REQUIRE(std::isfinite(goals[k]), DGDM_EINVAL, "goal %d, finger %d: coordinate %d is not finite", (int)(k / ((size_t)g->B * 3)),
                     (int)(k / 3 % g->B), (int)(k % 3));
    int rc;
    if ((rc = g->goalspecs.alloc(sizeof(DgdmGoalSpec) * g->cfg.max_chains))) return rc;
    DGDM_HIP_CHECK(hipMemcpyAsync(g->goalspecs.p, specs_host, sizeof(DgdmGoalSpec) * n_chains, hipMemcpyHostToDevice, s));
    return goal_field_build(g->sweep_ori.as<float>(), g->pos_lin.as<float>(), goals_dev, g->goalspecs.as<DgdmGoalSpec>(), n_chains, g->B,
                            g->cfg.grid_size, g->cfg.num_pos, field_dev, s);
}

// Diffusion.cond_fn's forward half (generator/diffusion.py:473-504 up to the classifier's output) and the classes of :506-532 on it.
extern "C" int dgdm_guidance_score(DgdmGuidance *g, const float *x_dev, int timestep, const int32_t *object_of_chain, const int64_t *starts_host,
                                   const float thr[3], int n_chains, float *logits_dev, int32_t *counts_dev, float *sums_dev, void *stream) {
    DGDM_REQUIRE(g && x_dev && object_of_chain && thr && counts_dev && sums_dev, DGDM_EINVAL, "dgdm_guidance_score: null argument");
    DGDM_REQUIRE(!g->bf16, DGDM_EINVAL, "dgdm_guidance_score: the bf16 trunk has no forward-only form (contraction dtypes f32 / f32_f16x3 / f32_mfma)");
    hipStream_t s = (hipStream_t)stream;
    const int kind = g->m->kind;
    DGDM_REQUIRE(kind == 2 || starts_host, DGDM_EINVAL, "3-D scoring needs the FPS start indices");
    DGDM_REQUIRE(n_chains > 0 && n_chains <= g->cfg.max_chains, DGDM_EINVAL, "n_chains %d outside 1..%d", n_chains, g->cfg.max_chains);
    int rc;
    if (!logits_dev) {
        if ((rc = g->scorelogits.alloc((size_t)n_chains * g->grid.rows * 3 * sizeof(float)))) return rc;
        logits_dev = g->scorelogits.as<float>();
    }
    const std::vector<int> oidx(object_of_chain, object_of_chain + n_chains);
    TrunkParams p;
    if ((rc = g->trunk_front(kind, x_dev, timestep, oidx.data(), starts_host, n_chains, nullptr, 0, &p, s))) return rc;
    p.logits = logits_dev;
    if (g->f32_mfma) {
        if ((rc = trunk_launch(kind, false, true, p, s))) return rc;
    } else {
        TrunkF16Scales sc;
        g->m->fill_trunk_f16(&p, &sc);
        if ((rc = trunk_f16l_launch(kind, TrunkF16Mode::Forward, p, sc, s))) return rc;
    }
    return score_tally(logits_dev, n_chains, g->B, g->grid.cells, thr, counts_dev, sums_dev, s);
}

extern "C" int dgdm_guidance_objective_values(DgdmGuidance *g, const float *logits_dev, const DgdmObjective *objectives, const float *rowcoef_dev,
                                              int n_chains, double *values_dev, void *stream) {
    DGDM_REQUIRE(g && logits_dev && objectives && values_dev, DGDM_EINVAL, "dgdm_guidance_objective_values: null argument");
    DGDM_REQUIRE(n_chains > 0 && n_chains <= g->cfg.max_chains, DGDM_EINVAL, "n_chains %d outside 1..%d", n_chains, g->cfg.max_chains);
    int rc;
    if ((rc = check_objectives(g, objectives, rowcoef_dev, n_chains))) return rc;
    hipStream_t s = (hipStream_t)stream;
    std::vector<TrunkObjective> tob(n_chains);
    for (int i = 0; i < n_chains; ++i) {
        for (int j = 0; j < 3; ++j) { tob[i].lin[j] = objectives[i].lin[j]; tob[i].quad[j] = objectives[i].quad[j]; }
        tob[i].use_rowcoef = objectives[i].use_rowcoef; tob[i].pad = 0;
    }
    if ((rc = g->valobj.alloc(sizeof(TrunkObjective) * g->cfg.max_chains))) return rc;
    DGDM_HIP_CHECK(hipMemcpyAsync(g->valobj.p, tob.data(), sizeof(TrunkObjective) * n_chains, hipMemcpyHostToDevice, s));
    return objective_values_launch(logits_dev, g->valobj.as<TrunkObjective>(), rowcoef_dev, g->rowfield, n_chains, g->B, g->grid.cells, values_dev, s);
}

// ================================================================================================ the denoise loop as one call
namespace {
__global__ void fill_i32_kernel(int *p, int v, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = v;
}
__global__ void repeat_rows_kernel(const float *__restrict__ src, float *__restrict__ dst, int64_t n_src, int reps) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_src * reps) dst[i] = src[i % n_src];
}
// classifier-free guidance: eps_u + w (eps_c - eps_u), every operation rounded on its own (common.h add_rn / mul_rn: never contracted into an fma)
__global__ void cfg_mix_kernel(const float *ec, const float *eu, float w, float *out, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float u = eu[i];
    out[i] = add_rn(u, mul_rn(w, sub_rn(ec[i], u)));
}
}  // namespace

extern "C" int dgdm_cfg_mix(const float *eps_c_dev, const float *eps_u_dev, float w, float *out_dev, int64_t numel, void *stream) {
    DGDM_REQUIRE(eps_c_dev && eps_u_dev && out_dev && numel >= 0, DGDM_EINVAL, "dgdm_cfg_mix: bad argument");
    if (numel == 0) return DGDM_OK;
    hipLaunchKernelGGL(cfg_mix_kernel, dim3((unsigned)((numel + 255) / 256)), dim3(256), 0, (hipStream_t)stream, eps_c_dev, eps_u_dev, w, out_dev, numel);
    DGDM_HIP_CHECK(hipGetLastError());
    return DGDM_OK;
}

extern "C" int dgdm_guided_chains_run(DgdmUnet1d *unet, DgdmGuidance *g, const float *noise_dev, int n_chains, int n_grad,
                                      const DgdmObjective *objectives, const float *rowcoef_dev, const int64_t *starts_host,
                                      const int32_t *timesteps, const float *coef, const float *scales, int n_steps, float *x_out_dev,
                                      void *stream) {
    return dgdm_guided_chains_run_cond(unet, g, noise_dev, n_chains, n_grad, objectives, rowcoef_dev, starts_host, timesteps, coef, scales, n_steps, x_out_dev,
                                       nullptr, 0, 1.f, stream);
}

extern "C" int dgdm_guided_chains_run_cond(DgdmUnet1d *unet, DgdmGuidance *g, const float *noise_dev, int n_chains, int n_grad,
                                           const DgdmObjective *objectives, const float *rowcoef_dev, const int64_t *starts_host,
                                           const int32_t *timesteps, const float *coef, const float *scales, int n_steps, float *x_out_dev,
                                           const float *global_cond_dev, int64_t cond_chain_stride, float cfg_weight, void *stream) {
    return dgdm_guided_chains_run_bounded(unet, g, noise_dev, n_chains, n_grad, objectives, rowcoef_dev, starts_host, timesteps, coef, scales, n_steps, x_out_dev,
                                          global_cond_dev, cond_chain_stride, cfg_weight, nullptr, nullptr, stream);
}

extern "C" int dgdm_guided_chains_run_bounded(DgdmUnet1d *unet, DgdmGuidance *g, const float *noise_dev, int n_chains, int n_grad,
                                              const DgdmObjective *objectives, const float *rowcoef_dev, const int64_t *starts_host,
                                              const int32_t *timesteps, const float *coef, const float *scales, int n_steps, float *x_out_dev,
                                              const float *global_cond_dev, int64_t cond_chain_stride, float cfg_weight, const float *lo_dev,
                                              const float *hi_dev, void *stream) {
    return dgdm_guided_chains_run_noisy(unet, g, noise_dev, n_chains, n_grad, objectives, rowcoef_dev, starts_host, timesteps, coef, scales, n_steps, x_out_dev,
                                        global_cond_dev, cond_chain_stride, cfg_weight, lo_dev, hi_dev, nullptr, 0, nullptr, stream);
}

// The single body of the four entries.  lo_dev / hi_dev: per-entry clip of the predicted clean sample ([B][L], one block for all chains)
// in place of [-1, 1]; both NULL: the plain step.  eta_coef: (sigma, dir) per step, NULL: sigma = 0 - then, and at every step whose
// sigma is 0, the step is the eta = 0 launch of old.
extern "C" int dgdm_guided_chains_run_noisy(DgdmUnet1d *unet, DgdmGuidance *g, const float *noise_dev, int n_chains, int n_grad,
                                            const DgdmObjective *objectives, const float *rowcoef_dev, const int64_t *starts_host,
                                            const int32_t *timesteps, const float *coef, const float *scales, int n_steps, float *x_out_dev,
                                            const float *global_cond_dev, int64_t cond_chain_stride, float cfg_weight, const float *lo_dev,
                                            const float *hi_dev, const float *eta_coef, uint64_t seed, const uint64_t *chain_keys, void *stream) {
    DGDM_REQUIRE(unet && g && noise_dev && objectives && timesteps && coef && scales && x_out_dev, DGDM_EINVAL, "dgdm_guided_chains_run: null argument");
    DGDM_REQUIRE(!lo_dev == !hi_dev, DGDM_EINVAL, "dgdm_guided_chains_run_bounded: lo and hi come together or not at all");
    DGDM_REQUIRE(n_chains > 0 && n_grad > 0 && n_chains * n_grad <= g->cfg.max_chains && n_steps > 0, DGDM_EINVAL,
                 "dgdm_guided_chains_run: %d chains x %d gradients outside 1..%d", n_chains, n_grad, g->cfg.max_chains);
    hipStream_t s = (hipStream_t)stream;
    const int B = g->B, L = g->m->L, kind = g->m->kind;
    const size_t per_chain = (size_t)B * L, nx = per_chain * n_chains, ng = nx * n_grad;
    DGDM_REQUIRE(kind == 2 || starts_host, DGDM_EINVAL, "3-D guidance needs the FPS start indices");
    const int gc = dgdm_unet1d_global_cond_dim(unet);
    DGDM_REQUIRE(gc == 0 || global_cond_dev, DGDM_EINVAL, "dgdm_guided_chains_run: the eps-net has global_cond_dim %d and needs a condition", gc);
    DGDM_REQUIRE(cfg_weight == cfg_weight && std::fabs(cfg_weight) <= 3.0e38f, DGDM_EINVAL, "dgdm_guided_chains_run: cfg_weight is not finite");
    const bool conditional = gc > 0;
    DGDM_REQUIRE(!conditional || cond_chain_stride == 0 || cond_chain_stride == (int64_t)B * gc, DGDM_EINVAL,
                 "dgdm_guided_chains_run: cond_chain_stride %lld is neither 0 (one [B][%d] block for all chains) nor B * gc = %lld", (long long)cond_chain_stride, gc,
                 (long long)B * gc);
    const bool per_chain_cond = conditional && cond_chain_stride != 0 && n_chains > 1;
    // what the eps-net evaluates: 1 the condition rows, 0 the all-zero rows, 2 both in one call of twice the samples, mixed afterwards
    const int cfg = !conditional ? 1 : cfg_weight == 1.f ? 1 : cfg_weight == 0.f ? 0 : 2;
    int rc;
    if ((rc = check_objectives(g, objectives, rowcoef_dev, n_chains * n_grad))) return rc;      // before the first launch of the loop
    bool noisy = false;
    for (int si = 0; eta_coef && si < n_steps; ++si) {
        const float sg = eta_coef[2 * si], dr = eta_coef[2 * si + 1];
        DGDM_REQUIRE(sg >= 0.f && sg <= 3.0e38f && dr == dr, DGDM_EINVAL, "dgdm_guided_chains_run_noisy: step %d has sigma %g, dir %g", si, (double)sg, (double)dr);
        noisy = noisy || sg != 0.f;
    }
    const uint64_t *keys_dev = nullptr;
    if (noisy) {         // the chains' keys: uploaded when they differ from what the handle holds (then the stream is waited for once,
                         // so the host copy is not touched again while a copy may be reading it); a repeated run uploads nothing
        std::vector<uint64_t> keys(n_chains);
        for (int c = 0; c < n_chains; ++c) keys[c] = chain_keys ? chain_keys[c] : (uint64_t)c;
        if (keys != g->loopkeys_host || !g->loopkeys.p) {
            g->loopkeys_host.clear();
            if ((rc = g->loopkeys.alloc(sizeof(uint64_t) * n_chains))) return rc;
            DGDM_HIP_CHECK(hipMemcpyAsync(g->loopkeys.p, keys.data(), sizeof(uint64_t) * n_chains, hipMemcpyHostToDevice, (hipStream_t)stream));
            DGDM_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
            g->loopkeys_host = keys;
        }
        keys_dev = g->loopkeys.as<uint64_t>();
    }
    if ((rc = g->loopx[0].alloc(nx * 4)) || (rc = g->loopx[1].alloc(nx * 4)) || (rc = g->loopeps.alloc(nx * 4)) || (rc = g->loopgrad.alloc(ng * 4)) ||
        (rc = g->loopxrep.alloc(ng * 4)) || (rc = g->loopts.alloc((size_t)2 * n_chains * B * sizeof(int))))
        return rc;
    // condition rows of all n_chains * B samples, then as many all-zero rows (the unconditional half of the classifier-free mix)
    const size_t ncond = (size_t)n_chains * B * gc;
    const float *cond_rows = nullptr, *zero_rows = nullptr;
    if (conditional) {
        if ((rc = g->loopcond.alloc(2 * ncond * 4))) return rc;
        float *cr = g->loopcond.as<float>();
        if (cond_chain_stride == 0) hipLaunchKernelGGL(repeat_rows_kernel, dim3((unsigned)((ncond + 255) / 256)), dim3(256), 0, s, global_cond_dev, cr, (int64_t)B * gc, n_chains);
        else DGDM_HIP_CHECK(hipMemcpyAsync(cr, global_cond_dev, ncond * 4, hipMemcpyDeviceToDevice, s));
        DGDM_HIP_CHECK(hipMemsetAsync(cr + ncond, 0, ncond * 4, s));
        cond_rows = cr; zero_rows = cr + ncond;
        if (cfg == 2 && ((rc = g->loopx2.alloc(2 * nx * 4)) || (rc = g->loopeps2.alloc(2 * nx * 4)))) return rc;
    }
    // every chain starts from the same noise (generator/diffusion.py:570)
    hipLaunchKernelGGL(repeat_rows_kernel, dim3((unsigned)((nx + 255) / 256)), dim3(256), 0, s, noise_dev, g->loopx[0].as<float>(), (int64_t)per_chain, n_chains);
    bool same_scale = true;
    for (int c = 1; c < n_chains; ++c) same_scale = same_scale && scales[c] == scales[0];
    const int64_t spc = kind == 3 ? 2 * g->grid.rows : 0;
    // 3-D: the embeddings of the rows depend on the draws and the objects, not on x, so those of ALL the steps are made before the
    // first one, in one upload and one gather launch: the (chain, s1) groups then hold n_steps times the rows per slab staged (and
    // per slab read from HBM), and more of them are equal rows computed once.  The host's conversion and sort of the draws runs
    // while the objects' tables are still being built (embed() waits for them only after the host work).  (A gather launch holds
    // fewer than 2^22 rows per chain - the sorted row list packs s2 beside the row id - so a longer run is embedded in groups of
    // `cpe` calls, each before its first step.)
    DgdmGuidance::Embedded emb;
    std::vector<int> oidx(n_chains * n_grad);
    const int64_t call_stride = (int64_t)n_chains * n_grad * spc;
    int cpe = kind == 3 ? (int)std::min<int64_t>(n_steps, std::max<int64_t>(1, (((int64_t)1 << 22) - 1) / std::max<int64_t>(1, g->grid.rows))) : n_steps;
    if (const char *e = getenv("DGDM_EMBED_CALLS")) cpe = std::max(1, std::min(cpe, atoi(e)));      // test hook: calls per gather launch
    // the embeddings and common_pre are made here, ahead of guidance_grad's own check
    for (int i = 0; i < n_chains * n_grad; ++i) oidx[i] = objectives[i].object;
    if ((rc = g->check_objects(oidx.data(), n_chains * n_grad))) return rc;
    DGDM_REQUIRE(same_scale || n_grad == 1, DGDM_EINVAL, "per-chain guidance scales with averaged gradients are not supported");
    // Step schedule.  eps-net and cond_fn both depend on x_t alone, so the eps-net (with its timestep fill,
    // classifier-free copies and mix, and step 0's replication) runs on bstream[0] beside common_pre's latency-bound float64 kernels,
    // between two events: fork_ev on `s` once x_t is final, side_ev on the side stream, which `s` waits for in front of the trunk (beside
    // the trunk itself the eps-net costs the trunk what it saves: DESIGN.md 4.3b) - every call's side work is joined into `s` before
    // the call returns.  A 3-D step 0 stays on `s`: the side stream may still be building the tables.  What reads no table - all of
    // the above and common_pre - is enqueued BEFORE the step's embed(), which joins `s` to the build: step 0 runs it beside the build.
    const bool hoist = g->hoist_x_only(), beside = g->eps_beside();
    hipStream_t side = s;
    if (beside && (rc = g->side_stream(&side))) return rc;
    if ((rc = g->loopeps1.alloc(per_chain * 4))) return rc;
    auto step = [&](int si) -> int {
        int rc;
        float *x = g->loopx[si & 1].as<float>(), *xn = (si + 1 == n_steps) ? x_out_dev : g->loopx[(si + 1) & 1].as<float>();
        const int t = timesteps[si];
        const bool embed_due = kind == 3 && si % cpe == 0;
        if (embed_due && !hoist &&
            (rc = g->embed(oidx.data(), n_chains * n_grad, starts_host + (size_t)si * call_stride, std::min(cpe, n_steps - si), call_stride, &emb, s))) return rc;
        // eps-net: at the first step all chains hold the same B fingers - one evaluation, replicated (same input, same bits) - unless
        // every chain has condition rows of its own
        const int nb = (si == 0 && n_chains > 1 && !per_chain_cond) ? B : n_chains * B;
        const int ne = cfg == 2 ? 2 * nb : nb;
        const bool fork = beside && !(kind == 3 && si == 0);
        const hipStream_t es = fork ? side : s;        // the eps-net's stream
        if (fork) {
            DGDM_HIP_CHECK(hipEventRecord(g->fork_ev, s));
            DGDM_HIP_CHECK(hipStreamWaitEvent(es, g->fork_ev, 0));
        }
        // one evaluation for all chains lands in a buffer of its own and is replicated from there (loopgrad, the scratch of old, is
        // cond_fn's output on the other stream)
        float *eps_dst = nb != n_chains * B ? g->loopeps1.as<float>() : g->loopeps.as<float>();
        hipLaunchKernelGGL(fill_i32_kernel, dim3((ne + 255) / 256), dim3(256), 0, es, g->loopts.as<int>(), t, ne);
        if (cfg == 2) {
            // [x | x] with [condition rows | zero rows] in one call (large runs land in the batched form), then the mix
            const size_t n = (size_t)nb * L, nc = (size_t)nb * gc;
            float *x2 = g->loopx2.as<float>(), *e2 = g->loopeps2.as<float>(), *c2 = g->loopcond.as<float>();
            DGDM_HIP_CHECK(hipMemcpyAsync(x2, x, n * 4, hipMemcpyDeviceToDevice, es));
            DGDM_HIP_CHECK(hipMemcpyAsync(x2 + n, x, n * 4, hipMemcpyDeviceToDevice, es));
            // the zero half has to follow the nb condition rows directly: at full size it does (loopcond's layout), at step 0's B rows it is moved up
            if (nc != ncond) DGDM_HIP_CHECK(hipMemsetAsync(c2 + nc, 0, nc * 4, es));
            if ((rc = dgdm_unet1d_forward_cond(unet, x2, g->loopts.as<int>(), c2, e2, 2 * nb, L, es))) return rc;
            if (nc != ncond) {       // restore chain 1's rows for the steps that follow
                if (cond_chain_stride == 0) hipLaunchKernelGGL(repeat_rows_kernel, dim3((unsigned)((ncond + 255) / 256)), dim3(256), 0, es, global_cond_dev, c2, (int64_t)B * gc, n_chains);
                else DGDM_HIP_CHECK(hipMemcpyAsync(c2, global_cond_dev, ncond * 4, hipMemcpyDeviceToDevice, es));
            }
            if ((rc = dgdm_cfg_mix(e2, e2 + n, cfg_weight, eps_dst, (int64_t)n, es))) return rc;
        } else if ((rc = dgdm_unet1d_forward_cond(unet, x, g->loopts.as<int>(), cfg == 0 ? zero_rows : cond_rows, eps_dst, nb, L, es))) return rc;
        if (nb != n_chains * B)
            hipLaunchKernelGGL(repeat_rows_kernel, dim3((unsigned)((nx + 255) / 256)), dim3(256), 0, es, eps_dst, g->loopeps.as<float>(), (int64_t)per_chain, n_chains);
        if (fork) DGDM_HIP_CHECK(hipEventRecord(g->side_ev, es));
        // cond_fn for the n_grad * n_chains gradient chains (object-major: gradient j of chain k is chain j * n_chains + k), x repeated
        const float *xg = x;
        if (n_grad > 1) {
            hipLaunchKernelGGL(repeat_rows_kernel, dim3((unsigned)((ng + 255) / 256)), dim3(256), 0, s, x, g->loopxrep.as<float>(), (int64_t)nx, n_grad);
            xg = g->loopxrep.as<float>();
        }
        if (hoist) {
            if ((rc = g->common_pre(xg, (float)t / (float)g->cfg.num_train_timesteps, oidx.data(), n_chains * n_grad, s))) return rc;
            if (embed_due &&
                (rc = g->embed(oidx.data(), n_chains * n_grad, starts_host + (size_t)si * call_stride, std::min(cpe, n_steps - si), call_stride, &emb, s))) return rc;
        }
        if (fork) DGDM_HIP_CHECK(hipStreamWaitEvent(s, g->side_ev, 0));
        if ((rc = guidance_grad(g, kind, xg, t, objectives, rowcoef_dev, nullptr, n_chains * n_grad, g->loopgrad.as<float>(), s,
                                kind == 3 ? &emb : nullptr, si % cpe, hoist))) return rc;
        const float *cf = coef + 4 * si;
        const float sigma = eta_coef ? eta_coef[2 * si] : 0.f;
        // the scheduler step over n entries, whole chains, from offset `off`; with bounds, their [B][L] block repeats for every chain
        auto ddim = [&](size_t off, int ngr, int64_t n, float scale) -> int {
            const float *e = g->loopeps.as<float>() + off, *gr = g->loopgrad.as<float>() + off;
            if (sigma != 0.f)
                return dgdm_ddim_guided_step_noisy(x + off, e, gr, ngr, xn + off, n, cf[0], cf[1], cf[2], eta_coef[2 * si + 1], scale, lo_dev, hi_dev,
                                                   (int64_t)per_chain, sigma, nullptr, seed, keys_dev + off / per_chain, si, (int64_t)per_chain, s);
            if (lo_dev)
                return dgdm_ddim_guided_step_bounded(x + off, e, gr, ngr, xn + off, n, cf[0], cf[1], cf[2], cf[3], scale, lo_dev, hi_dev, (int64_t)per_chain, s);
            return dgdm_ddim_guided_step(x + off, e, gr, ngr, xn + off, n, cf[0], cf[1], cf[2], cf[3], scale, s);
        };
        if (same_scale) {
            if ((rc = ddim(0, n_grad, (int64_t)nx, scales[0]))) return rc;
        } else {
            for (int c = 0; c < n_chains; ++c)
                if ((rc = ddim(c * per_chain, 1, (int64_t)per_chain, scales[c]))) return rc;
        }
        return DGDM_OK;
    };
    for (int si = 0; si < n_steps; ++si)
        if ((rc = step(si))) {
            if (beside) {       // a step that failed half way: what it left on the side stream is joined all the same
                (void)hipEventRecord(g->side_ev, side);
                (void)hipStreamWaitEvent(s, g->side_ev, 0);
            }
            return rc;
        }
    DGDM_HIP_CHECK(hipGetLastError());
    return DGDM_OK;
}

extern "C" int dgdm_guidance_orientation_sweep(DgdmGuidance *g, const float *x_dev, const int32_t *object_of_chain, const int64_t *starts_host,
                                               int n_chains, float *logits_dev, void *stream) {
    DGDM_REQUIRE(g && x_dev && object_of_chain && logits_dev, DGDM_EINVAL, "dgdm_guidance_orientation_sweep: null argument");
    DGDM_REQUIRE(n_chains > 0 && n_chains <= g->cfg.max_chains, DGDM_EINVAL, "n_chains %d outside 1..%d", n_chains, g->cfg.max_chains);
    hipStream_t s = (hipStream_t)stream;
    const int kind = g->m->kind;
    int rc;
    if ((rc = g->check_objects(object_of_chain, n_chains))) return rc;
    if ((rc = g->common_pre(x_dev, 0.f, object_of_chain, n_chains, s))) return rc;       // timesteps = zeros (:515,521)
    TrunkParams p;
    g->m->fill_trunk(&p);
    g->set_grid(&p, g->sweep, n_chains);
    if (kind == 3) {
        DGDM_REQUIRE(starts_host, DGDM_EINVAL, "3-D sweep needs the FPS start indices");
        // the sweep stays float32: table rows when the float32 tables exist, the gather kernels otherwise (e.g. a bf16-mode handle)
        DgdmGuidance::Embedded emb;
        if ((rc = g->embed_rows(object_of_chain, n_chains, starts_host, g->sweep.rows, 1, 0, false, &emb, s))) return rc;
        emb.point(&p, *g, 0, g->sweep.rows);
    }
    p.logits = logits_dev;
    return trunk_launch(kind, false, true, p, s);
}

// ================================================================================================ predicted roll-outs
// K interactions of the dynamics model with itself from the sweep's poses (include/dgdm_hip.h).  x and t = 0 do not change, so the
// per-finger table (common_pre) is built once; 3-D: the embeddings of the rows of all K classifier calls are made before the first
// interaction, as dgdm_guided_chains_run does for its steps (one upload, one gather launch or one index kernel), and call k reads rows
// [k * Rs, (k + 1) * Rs) of every chain.  Then K x (per-row pose tiles, forward-only f16x3 trunk, state update) on the caller's
// stream: no copy to the host and no host wait in between.
extern "C" int dgdm_guidance_rollout(DgdmGuidance *g, const float *x_dev, const int32_t *object_of_chain, const int64_t *starts_host,
                                     const double scale[3], int n_interactions, int n_chains, double *final_dev, float *first_logits_dev,
                                     int32_t *left_dev, double *traj_pose_dev, float *traj_logits_dev, void *stream) {
    DGDM_REQUIRE(g && x_dev && object_of_chain && scale && final_dev && first_logits_dev && left_dev, DGDM_EINVAL, "dgdm_guidance_rollout: null argument");
    DGDM_REQUIRE(!g->bf16, DGDM_EINVAL, "dgdm_guidance_rollout: the bf16 trunk has no forward-only form (contraction dtypes f32 / f32_f16x3)");
    DGDM_REQUIRE(!g->f32_mfma, DGDM_EINVAL, "dgdm_guidance_rollout: the float32 MFMA trunk has no per-row pose form (contraction dtypes f32 / f32_f16x3)");
    DGDM_REQUIRE(n_interactions >= 1, DGDM_EINVAL, "dgdm_guidance_rollout: %d interactions (at least 1)", n_interactions);
    DGDM_REQUIRE(n_chains > 0 && n_chains <= g->cfg.max_chains, DGDM_EINVAL, "n_chains %d outside 1..%d", n_chains, g->cfg.max_chains);
    int rc;
    if ((rc = g->check_objects(object_of_chain, n_chains))) return rc;
    hipStream_t s = (hipStream_t)stream;
    const int kind = g->m->kind, K = n_interactions, W1 = g->m->W1, G = g->sweep.cells;
    DGDM_REQUIRE(kind == 2 || starts_host, DGDM_EINVAL, "3-D roll-out needs the FPS start indices");
    const int64_t Rs = g->sweep.rows, rows = (int64_t)n_chains * Rs;
    const int ntiles = n_chains * g->B * g->sweep.tiles_per_b;
    if ((rc = g->rollstate.alloc((size_t)rows * 3 * sizeof(double))) || (rc = g->rolltiles.alloc((size_t)ntiles * 32 * W1 * sizeof(float))) ||
        (kind == 3 && (rc = g->rollpmax.alloc((size_t)ntiles * 32 * sizeof(float)))) ||
        (!traj_logits_dev && (rc = g->rolllogits.alloc((size_t)rows * 3 * sizeof(float)))))
        return rc;
    if ((rc = g->common_pre(x_dev, 0.f, object_of_chain, n_chains, s))) return rc;       // t = 0, as the sweep
    TrunkParams p;
    g->m->fill_trunk(&p);
    // float32 embeddings through the sweep's path: table rows when the float32 tables exist, the gather kernels otherwise
    DgdmGuidance::Embedded emb;
    if (kind == 3 && (rc = g->embed_rows(object_of_chain, n_chains, starts_host, Rs, K, (int64_t)n_chains * 2 * Rs, false, &emb, s))) return rc;
    TrunkF16Scales sc;
    g->m->fill_trunk_f16(&p, &sc);
    g->set_grid(&p, g->sweep, n_chains);
    p.Ptab = nullptr; p.PtabT = g->rolltiles.as<float>(); p.Pmax = kind == 3 ? g->rollpmax.as<float>() : nullptr;       // a pose per row
    double *state = g->rollstate.as<double>();
    if ((rc = rollout_start(g->sweep_ori.as<float>(), n_chains, g->B, G, state, left_dev, traj_pose_dev, s))) return rc;
    g->rolltiles_chains = n_chains;
    for (int k = 0; k < K; ++k) {
        if ((rc = rollout_pose_table(state, g->m->blob64.at(g->m->off64.w1p_wt), W1, n_chains, g->B, G, g->rolltiles.as<float>(), p.Pmax ? g->rollpmax.as<float>() : nullptr, s)))
            return rc;
        p.logits = traj_logits_dev ? traj_logits_dev + (size_t)k * rows * 3 : g->rolllogits.as<float>();
        if (kind == 3) emb.point(&p, *g, k, Rs);
        if ((rc = trunk_f16l_launch(kind, TrunkF16Mode::ForwardRowPose, p, sc, s))) return rc;
        if ((rc = rollout_update(p.logits, scale, k, rows, state, left_dev, traj_pose_dev ? traj_pose_dev + (size_t)(k + 1) * rows * 3 : nullptr,
                                 k == K - 1 ? final_dev : nullptr, k == 0 ? first_logits_dev : nullptr, s)))
            return rc;
    }
    return DGDM_OK;
}

// ================================================================================================ condition rows
// One pass over a set of fingers (include/dgdm_hip.h): per batch a replication copy, dgdm_guidance_score / dgdm_guidance_rollout on the
// handle's scratch, and label.hip's reduction into the caller's rows - all on the caller's stream, which orders the batches' reuse of
// the scratch.  Everything is checked here before the first launch; the trunk is the two calls' own.
namespace {
int label_check(const char *what, DgdmGuidance *g, const float *fingers_dev, int64_t n_fingers, const int32_t *objects_host, int n_objects,
                const int64_t *starts_host, int layout, const float *rows_dev, int64_t row_stride, int64_t object_stride, int cols) {
    DGDM_REQUIRE(g && fingers_dev && objects_host && rows_dev, DGDM_EINVAL, "%s: null argument", what);
    DGDM_REQUIRE(n_fingers >= 1, DGDM_EINVAL, "%s: %lld fingers (at least 1)", what, (long long)n_fingers);
    DGDM_REQUIRE(!g->bf16, DGDM_EINVAL, "%s: the bf16 trunk has no forward-only form (contraction dtypes f32 / f32_f16x3 / f32_mfma)", what);
    DGDM_REQUIRE(n_objects > 0 && n_objects <= g->cfg.max_chains, DGDM_EINVAL, "%s: n_objects %d outside 1..%d", what, n_objects, g->cfg.max_chains);
    DGDM_REQUIRE(layout == DGDM_LABEL_MEAN || layout == DGDM_LABEL_PER_OBJECT, DGDM_EINVAL, "%s: layout %d (0 mean, 1 per object)", what, layout);
    if (layout == DGDM_LABEL_PER_OBJECT) {
        DGDM_REQUIRE(object_stride >= cols, DGDM_EINVAL, "%s: object_stride %lld holds no block of %d columns", what, (long long)object_stride, cols);
        DGDM_REQUIRE(row_stride >= (int64_t)(n_objects - 1) * object_stride + cols, DGDM_EINVAL, "%s: row_stride %lld holds no %d blocks %lld apart", what,
                     (long long)row_stride, n_objects, (long long)object_stride);
    } else {
        DGDM_REQUIRE(row_stride >= cols, DGDM_EINVAL, "%s: row_stride %lld holds no %d columns", what, (long long)row_stride, cols);
    }
    DGDM_REQUIRE(g->m->kind == 2 || starts_host, DGDM_EINVAL, "%s: 3-D labelling needs the FPS start indices", what);
    return g->check_objects(objects_host, n_objects);
}
}  // namespace

extern "C" int dgdm_guidance_label(DgdmGuidance *g, const float *fingers_dev, int64_t n_fingers, const int32_t *objects_host, int n_objects,
                                   int timestep, const float thr[3], const int64_t *starts_host, int layout, float *rows_dev, int64_t row_stride,
                                   int64_t object_stride, void *stream) {
    int rc;
    if ((rc = label_check("dgdm_guidance_label", g, fingers_dev, n_fingers, objects_host, n_objects, starts_host, layout, rows_dev, row_stride,
                          object_stride, DGDM_LABEL_TALLY_COLS)))
        return rc;
    DGDM_REQUIRE(thr, DGDM_EINVAL, "dgdm_guidance_label: null argument");
    hipStream_t s = (hipStream_t)stream;
    const int B = g->B, L = g->m->L, M = n_objects;
    if ((rc = g->labelx.alloc((size_t)M * B * L * sizeof(float))) || (rc = g->labelcounts.alloc((size_t)M * B * 27 * sizeof(int32_t))) ||
        (rc = g->labelsums.alloc((size_t)M * B * 4 * sizeof(float))))
        return rc;
    const int64_t per_batch = (int64_t)M * dgdm_guidance_starts_per_call(g);
    for (int64_t first = 0, k = 0; first < n_fingers; first += B, ++k) {
        const int nvalid = (int)std::min<int64_t>(B, n_fingers - first);
        if ((rc = label_replicate(fingers_dev, n_fingers, first, M, B, L, g->labelx.as<float>(), s))) return rc;
        if ((rc = dgdm_guidance_score(g, g->labelx.as<float>(), timestep, objects_host, starts_host ? starts_host + k * per_batch : nullptr, thr, M, nullptr,
                                      g->labelcounts.as<int32_t>(), g->labelsums.as<float>(), s)))
            return rc;
        if ((rc = label_tally(g->labelcounts.as<int32_t>(), g->labelsums.as<float>(), M, B, nvalid, g->grid.cells, layout == DGDM_LABEL_PER_OBJECT,
                              rows_dev + first * row_stride, row_stride, object_stride, s)))
            return rc;
    }
    return DGDM_OK;
}

extern "C" int dgdm_guidance_label_settled(DgdmGuidance *g, const float *fingers_dev, int64_t n_fingers, const int32_t *objects_host, int n_objects,
                                           const double scale[3], int n_interactions, const int64_t *starts_host, int layout, float *rows_dev,
                                           int64_t row_stride, int64_t object_stride, void *stream) {
    int rc;
    if ((rc = label_check("dgdm_guidance_label_settled", g, fingers_dev, n_fingers, objects_host, n_objects, starts_host, layout, rows_dev, row_stride,
                          object_stride, DGDM_LABEL_SETTLED_COLS)))
        return rc;
    DGDM_REQUIRE(scale, DGDM_EINVAL, "dgdm_guidance_label_settled: null argument");
    DGDM_REQUIRE(!g->f32_mfma, DGDM_EINVAL, "dgdm_guidance_label_settled: the float32 MFMA trunk has no per-row pose form (contraction dtypes f32 / f32_f16x3)");
    DGDM_REQUIRE(n_interactions >= 1, DGDM_EINVAL, "dgdm_guidance_label_settled: %d interactions (at least 1)", n_interactions);
    hipStream_t s = (hipStream_t)stream;
    const int B = g->B, L = g->m->L, M = n_objects, G = g->sweep.cells;
    const size_t rows = (size_t)M * g->sweep.rows;
    if ((rc = g->labelx.alloc((size_t)M * B * L * sizeof(float))) || (rc = g->labelfinal.alloc(rows * 3 * sizeof(double))) ||
        (rc = g->labelfirst.alloc(rows * 3 * sizeof(float))) || (rc = g->labelleft.alloc(rows * sizeof(int32_t))) ||
        (rc = g->labelobj.alloc((size_t)B * M * 6 * sizeof(double))))
        return rc;
    const int64_t per_batch = g->m->kind == 3 ? (int64_t)n_interactions * M * 2 * g->sweep.rows : 0;
    for (int64_t first = 0, k = 0; first < n_fingers; first += B, ++k) {
        const int nvalid = (int)std::min<int64_t>(B, n_fingers - first);
        if ((rc = label_replicate(fingers_dev, n_fingers, first, M, B, L, g->labelx.as<float>(), s))) return rc;
        if ((rc = dgdm_guidance_rollout(g, g->labelx.as<float>(), objects_host, starts_host ? starts_host + k * per_batch : nullptr, scale, n_interactions, M,
                                        g->labelfinal.as<double>(), g->labelfirst.as<float>(), g->labelleft.as<int32_t>(), nullptr, nullptr, s)))
            return rc;
        if ((rc = label_settled(g->labelfinal.as<double>(), g->labelleft.as<int32_t>(), M, B, G, nvalid, layout == DGDM_LABEL_PER_OBJECT,
                                g->labelobj.as<double>(), rows_dev + first * row_stride, row_stride, object_stride, s)))
            return rc;
    }
    return DGDM_OK;
}

// Test hook: the pose operand tiles the last dgdm_guidance_rollout call left behind (its LAST interaction's: call it with one
// interaction to see the start poses') -> rollout_tiles_dev [n_chains * B * tiles_per_finger][W1 * 32], tile = (chain * B + b) *
// tiles_per_finger + orientation tile, and the sweep's own table in the same layout -> sweep_tiles_dev [tiles_per_finger][W1 * 32].
extern "C" int dgdm_guidance_debug_rollout_table(DgdmGuidance *g, int n_chains, float *rollout_tiles_dev, float *sweep_tiles_dev,
                                                 int32_t *tiles_per_finger, int32_t *width, void *stream) {
    DGDM_REQUIRE(g && n_chains > 0 && n_chains <= g->cfg.max_chains, DGDM_EINVAL, "dgdm_guidance_debug_rollout_table: bad argument");
    if (tiles_per_finger) *tiles_per_finger = g->sweep.tiles_per_b;
    if (width) *width = g->m->W1;
    const size_t per_tile = (size_t)g->m->W1 * 32 * sizeof(float);
    if (rollout_tiles_dev) {
        DGDM_REQUIRE(n_chains <= g->rolltiles_chains, DGDM_EINVAL, "dgdm_guidance_debug_rollout_table: the last roll-out had %d chains", g->rolltiles_chains);
        DGDM_HIP_CHECK(hipMemcpyAsync(rollout_tiles_dev, g->rolltiles.p, (size_t)n_chains * g->B * g->sweep.tiles_per_b * per_tile, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    }
    if (sweep_tiles_dev)
        DGDM_HIP_CHECK(hipMemcpyAsync(sweep_tiles_dev, g->sweep.tiled.p, (size_t)g->sweep.tiles_per_b * per_tile, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return DGDM_OK;
}

// ================================================================================================ PointNet++ on arbitrary rows
namespace {

struct CloudGroup { std::vector<int> rows; };

// Runs the table pipeline for every distinct cloud among `rows` clouds and writes emb_dev [rows][256].
int pointnet_rows(DgdmDynamics *m, const float *xyz_dev /*[rows][3][N]*/, const int64_t *s1, const int64_t *s2, float *emb_dev, int rows,
                  int N, hipStream_t s) {
    DGDM_REQUIRE(N > 0 && N <= 1024, DGDM_EINVAL, "clouds of %d points unsupported (1..1024)", N);
    std::vector<float> host((size_t)rows * 3 * N);
    DGDM_HIP_CHECK(hipMemcpyAsync(host.data(), xyz_dev, host.size() * 4, hipMemcpyDeviceToHost, s));
    DGDM_HIP_CHECK(hipStreamSynchronize(s));
    // group bit-identical clouds (cond_fn hands 512 replicas of one cloud per call, diffusion.py:491)
    std::unordered_map<std::string, int> seen;
    std::vector<CloudGroup> groups;
    std::vector<int> rep;
    for (int r = 0; r < rows; ++r) {
        std::string key(reinterpret_cast<const char *>(host.data() + (size_t)r * 3 * N), (size_t)3 * N * 4);
        auto it = seen.find(key);
        int gid;
        if (it == seen.end()) {
            gid = (int)groups.size();
            seen.emplace(std::move(key), gid);
            groups.emplace_back();
            rep.push_back(r);
        } else {
            gid = it->second;
        }
        groups[gid].rows.push_back(r);
    }
    const PnWeights w = m->pn();
    DevBuf xyz, fps1, F1, U, Y, L2, Z, vlist, slotmap, starts, chains, out, crowded, clist, poff, pairs, prank;
    int rc;
    const PnWeights64 w64 = m->pn64();
    if ((rc = xyz.alloc((size_t)N * 12)) || (rc = fps1.alloc((size_t)N * 512 * 4)) || (rc = F1.alloc((size_t)N * 128 * 8)) || (rc = U.alloc((size_t)N * 128 * 8)) ||
        (rc = Y.alloc((size_t)N * N * 1024)) || (rc = chains.alloc(sizeof(XobjChain))) || (rc = crowded.alloc((size_t)N * 4)) ||
        (rc = clist.alloc((size_t)(N + 1) * 4)) || (rc = poff.alloc((size_t)(N + 1) * 4)) || (rc = pairs.alloc((size_t)N * N * 4)) ||
        (rc = prank.alloc((size_t)N * N * 2)))
        return rc;
    for (size_t gi = 0; gi < groups.size(); ++gi) {
        const std::vector<int> &rws = groups[gi].rows;
        std::vector<float> pts((size_t)N * 3);
        const float *src = host.data() + (size_t)rep[gi] * 3 * N;
        for (int i = 0; i < N; ++i) { pts[3 * i] = src[i]; pts[3 * i + 1] = src[N + i]; pts[3 * i + 2] = src[2 * N + i]; }
        std::vector<int> slot_of(N, -1), vl, st(2 * rws.size());
        for (size_t k = 0; k < rws.size(); ++k) {
            const int64_t a = s1[rws[k]], b = s2[rws[k]];
            DGDM_REQUIRE(a >= 0 && a < N && b >= 0 && b < 512, DGDM_EINVAL, "FPS start out of range");
            if (slot_of[a] < 0) { slot_of[a] = (int)vl.size(); vl.push_back((int)a); }
            st[2 * k] = (int)a; st[2 * k + 1] = (int)b;
        }
        const int nv = (int)vl.size();
        if ((rc = xyz.upload(pts.data(), pts.size() * 4)) || (rc = vlist.upload(vl.data(), vl.size() * 4)) ||
            (rc = slotmap.upload(slot_of.data(), slot_of.size() * 4)) || (rc = starts.upload(st.data(), st.size() * 4)) ||
            (rc = L2.alloc((size_t)nv * N * 1024)) || (rc = Z.alloc((size_t)nv * N * 1024)) || (rc = out.alloc(rws.size() * 1024)))
            return rc;
        const float *x = xyz.as<float>();
        if ((rc = pn_fps_table(x, N, N, 512, fps1.as<int>(), nullptr, s))) return rc;
        if ((rc = pn_sa1_64(x, N, w.r1sq, w64, F1.as<double>(), s))) return rc;
        if ((rc = linear64(nullptr, F1.as<double>(), 128, w64.sa2_wf_t, w64.sa2_b0, nullptr, 1, U.as<double>(), nullptr, 128, N, 128, 128, ACT_NONE, s))) return rc;
        if ((rc = pn_crowd(x, N, w, crowded.as<int>(), clist.as<int>(), clist.as<int>() + N, poff.as<int>(), pairs.as<int>(), prank.as<short>(), s))) return rc;
        if ((rc = pn_pairs64(x, N, U.as<double>(), w64, pairs.as<int>(), poff.as<int>(), Y.as<float>(), s))) return rc;
        if ((rc = pn_l2(x, N, w, fps1.as<int>(), vlist.as<int>(), nv, Y.as<float>(), L2.as<float>(), clist.as<int>(), clist.as<int>() + N,
                        poff.as<int>(), prank.as<short>(), false, s))) return rc;
        if ((rc = pn_z64(x, N, nv, w64, L2.as<float>(), Z.as<float>(), clist.as<int>(), clist.as<int>() + N, s))) return rc;
        XobjChain ch{};
        ch.xyz = x; ch.fps1 = fps1.as<int>(); ch.slot_of_start = slotmap.as<int>(); ch.Z = Z.as<float>(); ch.fps2 = nullptr; ch.flags = nullptr; ch.crowded = crowded.as<int>(); ch.N = N;
        DGDM_HIP_CHECK(hipMemcpyAsync(chains.p, &ch, sizeof ch, hipMemcpyHostToDevice, s));
        XobjParams xp{};
        xp.chains = chains.as<XobjChain>(); xp.starts = starts.as<int>(); xp.xobj = out.as<float>(); xp.R = (int64_t)rws.size(); xp.total_rows = xp.R;
        if ((rc = pn_xobj(xp, false, s))) return rc;
        // scatter the group's rows back
        bool contiguous = true;
        for (size_t k = 1; k < rws.size(); ++k) contiguous = contiguous && rws[k] == rws[k - 1] + 1;
        if (contiguous) {
            DGDM_HIP_CHECK(hipMemcpyAsync(emb_dev + (size_t)rws[0] * 256, out.p, rws.size() * 1024, hipMemcpyDeviceToDevice, s));
        } else {
            for (size_t k = 0; k < rws.size(); ++k)
                DGDM_HIP_CHECK(hipMemcpyAsync(emb_dev + (size_t)rws[k] * 256, out.as<float>() + k * 256, 1024, hipMemcpyDeviceToDevice, s));
        }
        DGDM_HIP_CHECK(hipStreamSynchronize(s));     // per-group buffers are reused by the next group
    }
    return DGDM_OK;
}

}  // namespace

extern "C" int dgdm_pointnet2_forward(DgdmDynamics *m, const float *xyz_dev, const int64_t *start_sa1_host, const int64_t *start_sa2_host,
                                      float *emb_dev, int rows, int N, void *stream) {
    DGDM_REQUIRE(m && xyz_dev && start_sa1_host && start_sa2_host && emb_dev && rows >= 0, DGDM_EINVAL, "dgdm_pointnet2_forward: bad argument");
    if (m->kind != 3) { set_error("model type not supported: PointNet++ belongs to the 3-D model"); return DGDM_EMODE; }
    if (rows == 0) return DGDM_OK;
    return pointnet_rows(m, xyz_dev, start_sa1_host, start_sa2_host, emb_dev, rows, N, (hipStream_t)stream);
}

extern "C" int dgdm_dyn3d_forward(DgdmDynamics *m, const float *x_ctrl, const float *x_ori, const float *x_pos, const float *t,
                                  const float *xyz, const int64_t *start_sa1_host, const int64_t *start_sa2_host, float *logits, int rows,
                                  int N, void *stream) {
    DGDM_REQUIRE(m && x_ctrl && x_ori && x_pos && t && xyz && start_sa1_host && start_sa2_host && logits && rows >= 0, DGDM_EINVAL,
                 "dgdm_dyn3d_forward: bad argument");
    if (m->kind != 3) { set_error("model type not supported: dgdm_dyn3d_forward on a 2-D model"); return DGDM_EMODE; }
    if (rows == 0) return DGDM_OK;
    hipStream_t s = (hipStream_t)stream;
    int rc;
    // workspace: V, GENC [rows][256] | pose [rows][32] | tmp [rows][768] | z1 [rows][512] | xobj [rows][256]
    const size_t need = (size_t)rows * (256 + 256 + 32 + 768 + 512 + 256) * sizeof(float);
    if ((rc = m->ws.alloc(need))) return rc;
    float *V = m->ws.as<float>(), *genc = V + (size_t)rows * 256, *pose = genc + (size_t)rows * 256, *tmp = pose + (size_t)rows * 32,
          *z1 = tmp + (size_t)rows * 768, *xo = z1 + (size_t)rows * 512;
    if ((rc = pointnet_rows(m, xyz, start_sa1_host, start_sa2_host, xo, rows, N, s))) return rc;
    if ((rc = m->time_part(t, 0.f, tmp, z1, rows, s))) return rc;
    // x_ctrl[:, 1, :]  (profile_forward_3d.py:78): rows of length L at stride 3L, offset L
    if ((rc = m->gripper_forward(x_ctrl + m->L, 3 * m->L, V, genc, rows, s))) return rc;
    if ((rc = linear(genc, 256, m->blob.at(m->off.w1c_wt), nullptr, nullptr, 1, z1, 512, rows, 256, 512, ACT_NONE, true, s))) return rc;
    if ((rc = pose_embed(x_ori, x_pos, pose, rows, s))) return rc;
    if ((rc = linear(pose, 27, m->blob.at(m->off.w1p_wt), nullptr, nullptr, 1, z1, 512, rows, 27, 512, ACT_NONE, true, s))) return rc;
    TrunkParams p;
    m->fill_trunk(&p);
    p.Atab = z1; p.xobj = xo; p.logits = logits; p.C = rows; p.R = rows; p.xstride = rows; p.B = 1; p.tiles_per_b = 1; p.ntiles = (rows + 31) / 32;
    return trunk_launch(3, true, true, p, s);
}

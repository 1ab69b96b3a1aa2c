// The guidance handle (internal): Diffusion.cond_fn / get_convergence_centers (generator/diffusion.py:473-539) for batches of chains.
// guidance_api.hip has the handle and its entry points, guidance_chains.hip the denoise loop on top of them.
#pragma once
#include "common.h"
#include "models.h"
#include "object_tables.h"
#include "row_embed.h"

namespace dgdm {
// A pose table of the trunk's first layer and the rows it spans: the cond_fn grid (G * P * P cells) or the orientation sweep (G cells)
struct PoseGrid {
    DevBuf tab, tiled;      // [cells][W1]; the same tiled for the trunk kernels (smallnet.h tile_table)
    DevBuf pmax;            // [cells] largest magnitude of a cell's row of tab (trunk_f16l.hip: f16 scale of 3-D layer 2's input); cond_fn grid only
    int cells = 0, tiles_per_b = 0;
    int64_t rows = 0;       // rows per chain: B * cells
};
}  // namespace dgdm

struct DgdmGuidance {
    using DevBuf = dgdm::DevBuf;
    using PoseGrid = dgdm::PoseGrid;
    using Embedded = dgdm::Embedded;
    DgdmDynamics *m = nullptr;
    DgdmGuidanceConfig cfg{};
    int B = 0;
    PoseGrid grid, sweep;                        // cond_fn grid, orientation sweep
    DevBuf objpart;                              // 2-D: [max_objects][W1] doubles
    DevBuf objtmp;                               // 2-D: scratch of set_objects (the object encoder's hidden layer, [n_objects][512] doubles)
    bool bf16 = false;                           // contractions of the trunk on bf16 MFMA (dgdm_guidance_set_contraction_dtype)
    bool f32_mfma = false;                       // float32 mode on the k-ordered float32 MFMA chain (trunk.hip) instead of the f16x3 form (trunk_f16l.hip)
    // V, genc, chainbias, timepart: float64 (smallnet.h linear64: per-finger / per-chain quantities are evaluated in double precision,
    // so the A table carries one float32 rounding); ttmp64: scratch of the time encoder
    DevBuf V, genc, atab, chainbias, timepart, ttmp, ttmp64, partial, objdev, objidx;
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
    // l1tab = DGDM_L1TAB, read at create: 0 builds no layer-1 table (ObjectTables::L1Z / L1K), every chain takes the trunk's general
    // front (same-binary reference, A/B)
    bool l1tab = true;
    int xtab_policy = 0;            // 0: build the embedding tables once the objects have served more than XTAB_AFTER cond_fn calls; 1: at set_objects (test hook mode 5)
    int grads_since_set = 0;
    static constexpr int XTAB_AFTER = 5;
    int l2_gather_mode = 0;         // test hook (mode 4): build the sa2 features of the crowded centres with l2_kernel's global gathers
    int n_objects = 0;
    // Step schedule.  The 3-D table build runs on the store's build streams alone; the first call that reads the tables
    // on a stream makes that stream wait for its end (ObjectStore3D::join).  Inside the denoise loop the eps-net runs on the store's first
    // stream (idle by then) beside common_pre and is joined in front of the trunk.  serial = DGDM_SERIAL_STEP, read at create:
    // 1 everything on the caller's stream, in the order of the data dependencies (also while dgdm_prof_enable is on: the stage events
    // assume one stream); for measuring the parts apart, 2 = only the table build stays on the caller's stream, 4 = only the eps-net does,
    // 8 = only the gather stays behind the END of the build (one launch behind the join) instead of starting object by object
    int serial = 0;
    bool tables_off_stream() const { return !(serial & 3) && !dgdm::prof_on(); }
    bool eps_beside() const { return !(serial & 5) && !dgdm::prof_on(); }
    bool hoist_x_only() const { return !(serial & 1) && !dgdm::prof_on(); }
    dgdm::Event fork_ev, side_ev;            // the denoise loop's fork to and join from the side stream
    // 3-D: the rows of a call, and the objects' tables.  The store comes last: its destructor, which waits for the build streams (the
    // side stream among them), runs before any other member of the handle is released
    dgdm::RowEmbedder rows{store};
    dgdm::ObjectStore3D store;

    int build_pose_table(const std::vector<float> &ori, const std::vector<float> &pos, PoseGrid *dst, hipStream_t s);
    // the first-layer tables and the shape of a launch over `g` for n_chains chains
    void set_grid(dgdm::TrunkParams *p, const PoseGrid &g, int n_chains) const;
    int check_objects(const int *oidx, int n_chains) const;
    // n_chains in 1..max_chains, else "<what>n_chains %d outside 1..%d": `what` is the entry point's prefix, if it has one
    int check_chains(const char *what, int n_chains) const;
    int common_pre(const float *x_dev, float t_scaled, const int *objidx_host, int n_chains, hipStream_t s);
    // cond_fn's embeddings (3-D): the rows of the cond_fn grid in the handle's arithmetic, counted towards the XTAB_AFTER policy, one
    // `xobj` profiling region
    int embed(const int *objidx_host, int n_chains, const int64_t *starts_host, int n_calls, int64_t call_stride, Embedded *e, hipStream_t s);
    // what cond_fn's gradient and its forward-only scoring share, up to the trunk launch: common_pre, 3-D: the rows' embeddings (`emb` /
    // `call` as guidance_grad takes them), and the trunk parameters of the cond_fn grid in the float32 form (the caller swaps
    // the weight streams for its arithmetic and adds its outputs)
    // pre_done: the caller has already enqueued common_pre for this x and timestep (the denoise loop does, ahead of the tables' join)
    int trunk_front(int kind, const float *x_dev, int timestep, const int *objidx_host, const int64_t *starts_host, int n_chains, const Embedded *emb,
                    int call, dgdm::TrunkParams *p, hipStream_t s, bool pre_done = false);
};

namespace dgdm {
// What a launch's objectives need of the per-row inputs, checked before anything is enqueued: the trunk reads rowcoef / field rows of
// chain i without looking again
int check_objectives(const DgdmGuidance *g, const DgdmObjective *objectives, const float *rowcoef_dev, int n_chains);
// cond_fn for n_chains chains.  3-D: `emb` = the embeddings made by DgdmGuidance::embed for a run of calls, `call` = which of them this is;
// emb == nullptr: this call's own (starts_host = its draws).
int guidance_grad(DgdmGuidance *g, int kind, const float *x_dev, int timestep, const DgdmObjective *objectives, const float *rowcoef_dev,
                  const int64_t *starts_host, int n_chains, float *grad_dev, hipStream_t s, const Embedded *emb = nullptr, int call = 0,
                  bool pre_done = false);
}  // namespace dgdm

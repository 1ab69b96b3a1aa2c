#pragma once
#include "common.h"

namespace dgdm {

struct TrunkObjective {   // device copy of DgdmObjective (object index not needed on the device)
    float lin[3];
    float quad[3];
    int   use_rowcoef;        // 0: lin / quad; 1: d0's seed is rowcoef[r]; 2 (DGDM_OBJ_ROWFIELD): lin / quad + rowfield[r][j]
    int   pad;
};

struct TrunkParams {
    // 256 -> 256 layers (trunk layers 2..8 for 2-D, 3..8 for 3-D), BatchNorm folded
    const float  *bf[8];      // folded biases
    int           n_mid;
    // continuous weight streams (mfma_chain.h stream_cont), in consumption order:
    //   forward : [3-D: 16 x (W1o block (32 entries) | W2' column block (32 entries))] then the n_mid images of W'
    //   backward: the n_mid images of W'^T, LAST layer first, [3-D: then the 16 blocks of W2'^T]
    const float4 *Wfwd, *Wbwd;
    unsigned      fwd_bytes, bwd_bytes;
    const float  *Wout;       // [3][256] row-major
    const float  *bout;       // [3]
    // 3-D only
    const float  *b2;         // folded bias of layer 2
    const float  *xobj;       // [nchain][R][256]  PointNet++ embedding per reference row
    const uint32_t *xobj16;   // bf16 trunk only: the same rows in bf16 operand order [nchain][R][128 dwords] (mfma_chain.h), or null
    // table mode, 3-D: instead of materialised rows, the per-object embedding tables (pointnet.h xtab): row r of chain c is
    // xtab[c] + xidx[c * R + r] * 256 floats (xtab16: * 128 dwords).  Null: read xobj / xobj16.
    const float *const *xtab;
    const uint32_t *const *xtab16;
    const int    *xidx;
    int64_t       xstride;    // rows per chain in xobj / xobj16 / xidx (>= R: a launch may read one denoise step's rows out of buffers that hold all steps')
    // layer 1's object part from a table (trunk_f16l.hip, the gradient kernel only; table mode): l1z[c] / l1k[c] = the tables of chain c's
    // object - [N][512] scaled layer-1 accumulators and [N] row scale exponents of the rows M0[q], indexed by xidx like xtab[c] - or null
    // for a chain without one.  l1z null: no chain has one.  Wfwd_nl1: the forward f16 stream without its layer-1 entries.
    // chainlist (device): the launch's chains, the n_tabled ones with a table first - trunk_f16l_launch runs the tabled instantiation
    // over those and the general one over the rest.  chains: what a kernel reads - the list its tiles run along (tile t belongs to
    // chains[t / (B * tiles_per_b)]), null: all chains in order; set by the launcher
    const float *const *l1z;
    const int   *const *l1k;
    const float4 *Wfwd_nl1;
    unsigned      fwd_nl1_bytes;
    const int    *chainlist;
    int           n_tabled;
    const int    *chains;
    // first-layer tables
    const float  *Atab;       // table mode: [nchain*B][W1]; rows mode: [rows][W1]
    const float  *Ptab;       // [C][W1]  (table mode)
    const float  *PtabT;      // the same, tiled per 32 cells in operand layout (smallnet.h tile_table); per-row pose mode (TrunkF16Mode::ForwardRowPose): one tile per trunk tile, [ntiles][W1 / 32][4][64] float4
    const float  *Pmax;       // [C] largest magnitude of a cell's row of Ptab (trunk_f16l.hip: the f16 scale of 3-D layer 2's input); may be null elsewhere; per-row pose mode: [ntiles][32], one value per tile row, padding rows included
    const TrunkObjective *obj;// [nchain]
    const float  *rowcoef;    // [nchain][R] or null
    const float  *rowfield;   // [nchain][R][3] or null: read for chains with use_rowcoef == 2 only (the host checks that it covers them)
    float        *partial;    // [ntiles][W1]
    float        *logits;     // fwd-only: [nchain][R][3]
    int           B, C, tiles_per_b, ntiles;
    int64_t       R;          // rows per chain (B*C in table mode, rows in rows mode)
};

// Algorithmic FLOPs of one trunk launch, whichever arithmetic carries it (DESIGN_HISTORY.md §5; what the `trunk` profiling stage
// reports): MFMA layers only, real rows only (the last cell tile of a finger is padded to 32: 1125 cells -> 36 tiles = 1152 issued rows)
inline double trunk_flops(int kind, const TrunkParams &p, bool rows_mode, bool fwd_only) {
    const double rows = rows_mode ? (double)p.R : (double)(p.ntiles / (p.tiles_per_b > 0 ? p.tiles_per_b : 1)) * p.C;
    const double mid = 2.0 * 256 * 256 * p.n_mid;
    double per_row = (kind == 3) ? (2.0 * 256 * 512 * 2 + mid) : mid;
    if (!fwd_only) per_row += (kind == 3) ? (2.0 * 256 * 512 + mid) : mid;
    return rows * per_row;
}

// kind: 2 | 3.  rows_mode: first-layer pre-activations given per row (general forward API).
int trunk_launch(int kind, bool rows_mode, bool fwd_only, const TrunkParams &p, hipStream_t s);

// float32 contractions as three f16 MFMA products on two-way split, power-of-two scaled operands (trunk_f16l.hip): table mode, forward +
// backward.  p.Wfwd / p.Wbwd point at the f16 streams (DgdmDynamics::fill_trunk_f16), sc carries the weight matrices' scale exponents.
struct TrunkF16Scales {
    int ew_mid[8];            // 256 -> 256 stack layer l (the same for W and its transpose)
    int ew_l1, ew_l2;         // 3-D: layer 1's object-embedding columns; layer 2 (the same for its transpose, the last layer back)
    float l1_norm1;           // 3-D: largest absolute row sum of layer 1's object-embedding columns (bounds a row of layer 1 from its input)
};
// (the weight stream is shared by the workgroup's four waves through LDS: trunk_f16l.hip)
// Grad: forward + backward.
// Forward: the forward half alone: the logits of every valid row to p.logits [nchain][R][3]; p.Wbwd, p.obj, p.rowcoef and p.partial are
// not read.
// ForwardRowPose: the same with a pose per ROW instead of per cell (dgdm_guidance_rollout): p.PtabT = one operand tile per trunk tile,
// [ntiles][W1 / 32][4][64] float4 in tile_table's layout (tile = (chain * B + finger) * tiles_per_b + cell tile), p.Pmax (3-D) =
// [ntiles][32], padding rows included; p.Ptab is not read.
enum class TrunkF16Mode { Grad, Forward, ForwardRowPose };
int trunk_f16l_launch(int kind, TrunkF16Mode mode, const TrunkParams &p, const TrunkF16Scales &sc, hipStream_t s);
// The layer-1 tables (TrunkParams::l1z / l1k) of n_objects 3-D objects in one launch: object i's rows are m0[i] [N][256]; an object whose
// ncr[i] (device: its crowded-centre count) is not zero is skipped.  Wfwd: the full forward f16 stream.  The same code on the same
// operands as the trunk's front: entry [q] holds the bits a tile row with the embedding M0[q] gets there.
int trunk_f16l_l1_tables(const float *const *m0, const int *ncr, float *const *l1z, int *const *l1k, int N, int n_objects, const float4 *Wfwd,
                         hipStream_t s);

// Roll-out steps around that trunk (rollout.hip).  State [n_chains][B * G][3] doubles = (ori, pos_x, pos_y) in the model's normalised
// units, row r = g * B + b.
// rollout_start: state = (ori_grid[g], 0, 0); left = -1; a copy of the state to traj0 when it is not null.
int rollout_start(const float *ori_grid, int n_chains, int B, int G, double *state, int32_t *left, double *traj0, hipStream_t s);
// rollout_pose_table: the state rounded to float32 -> layer 1's pose term per row (the 27-wide embedding of pose_embed_kernel times
// w1p_wt [27][W1] in float64, rounded once), written as the trunk's operand tiles; a finger's padding rows repeat its last valid row.
// pmax (3-D, else null): [ntiles][32] largest magnitude of each row.
int rollout_pose_table(const double *state, const double *w1p_wt, int W1, int n_chains, int B, int G, float *tiles, float *pmax, hipStream_t s);
// rollout_update: state += logits * scale (each product and sum rounded on its own), ori wrapped into [-1, 1]; left[r] = k the first
// time |pos| leaves 1; copies: the new state to traj_next / final, the logits to first_logits, where those are not null.
int rollout_update(const float *logits, const double scale[3], int k, int64_t rows, double *state, int32_t *left, double *traj_next,
                   double *final_state, float *first_logits, hipStream_t s);

// Per (chain, finger) tally of forward-only logits [n_chains][B * C][3] (row = cell * B + finger; score.hip): the joint class histogram
// counts [n_chains][B][27] (bin = (class of d0 * 3 + class of d1) * 3 + class of d2; class 2 if l > thr, 0 if l < -thr, else 1) and
// sums [n_chains][B][4] = sum d0, sum |d0|, sum d1, sum d2.  Fixed reduction order: the same bits every run.
int score_tally(const float *logits, int n_chains, int B, int C, const float thr[3], int32_t *counts, float *sums, hipStream_t s);

// The objective's VALUE per (chain, finger) from forward-only logits (resample.hip; the formula is the header's, dgdm_guidance_objective_values):
// logits [n_chains][B * C][3], obj [n_chains] on the device, rowcoef [n_chains][B * C] / rowfield [n_chains][B * C][3] read only for the
// chains that use them (the caller checks that they cover those) -> values [n_chains][B] float64.
int objective_values_launch(const float *logits, const TrunkObjective *obj, const float *rowcoef, const float *rowfield, int n_chains, int B, int C,
                            double *values, hipStream_t s);

// Condition rows (label.hip; the columns are the header's, dgdm_guidance_label / dgdm_guidance_label_settled).
// label_replicate: dst [n_chains][B][L] = fingers first .. first + B - 1 of [N][L] for every chain, past the end copies of finger N - 1.
int label_replicate(const float *fingers, int64_t N, int64_t first, int n_chains, int B, int L, float *dst, hipStream_t s);
// label_tally: score_tally's counts / sums of M chains -> the 10 tally columns of the batch's first nvalid fingers; rows points at the
// first of them.  per_object: M blocks object_stride apart, else one block over all M chains.
int label_tally(const int32_t *counts, const float *sums, int M, int B, int nvalid, int64_t cells, int per_object, float *rows, int64_t row_stride,
                int64_t object_stride, hipStream_t s);
// label_settled: a roll-out's final state [M][B * G][3] and left [M][B * G] -> the 5 settled columns; per_obj: scratch [B][M][6] doubles.
int label_settled(const double *final_state, const int32_t *left, int M, int B, int G, int nvalid, int per_object, double *per_obj, float *rows,
                  int64_t row_stride, int64_t object_stride, hipStream_t s);

// Goal field (goal.hip): field [n_chains][R][3], row r = cell * B + b, cell = (g * P + px) * P + py, from the float32 grids ori_grid [G] /
// pos_grid [P], the goals [n_chains][B][3] and one (validated) spec per chain, all on the device; the definitions are the header's.
int goal_field_build(const float *ori_grid, const float *pos_grid, const float *goals, const DgdmGoalSpec *specs, int n_chains, int B, int G, int P,
                     float *field, hipStream_t s);

// bf16-contraction variant (trunk_bf16.hip): table mode, forward + backward only.  p.Wfwd / p.Wbwd point at the bf16 streams
// (DgdmDynamics::fill_trunk_bf16); everything else in TrunkParams means the same.
int trunk_bf16_launch(int kind, const TrunkParams &p, hipStream_t s);

}  // namespace dgdm

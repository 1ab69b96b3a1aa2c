// Diffusion.cond_fn / get_convergence_centers (generator/diffusion.py:473-539) for batches of chains: the guidance handle, its
// gradient, scores, fields, orientation sweep, roll-outs and labels.  (3-D objects: object_tables.hip; the rows of a 3-D call:
// row_embed.hip; the denoise loop: guidance_chains.hip.)
#include "guidance.h"
#include <algorithm>
#include <cmath>
#include <cstdlib>

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

// the trunk's form of the chains' objectives
std::vector<TrunkObjective> to_trunk_objectives(const DgdmObjective *objectives, int n_chains) {
    std::vector<TrunkObjective> tob(n_chains);
    for (int i = 0; i < n_chains; ++i) {
        for (int j = 0; j < 3; ++j) { tob[i].lin[j] = objectives[i].lin[j]; tob[i].quad[j] = objectives[i].quad[j]; }
        tob[i].use_rowcoef = objectives[i].use_rowcoef; tob[i].pad = 0;
    }
    return tob;
}

}  // namespace

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

int DgdmGuidance::check_chains(const char *what, int n_chains) const {
    DGDM_REQUIRE(n_chains > 0 && n_chains <= cfg.max_chains, DGDM_EINVAL, "%sn_chains %d outside 1..%d", what, n_chains, cfg.max_chains);
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
    if ((rc = g->V.alloc(rows * 256 * 8)) || (rc = g->genc.alloc(rows * 256 * 8)) || (rc = g->atab.alloc(rows * W1 * 4)) ||
        (rc = g->chainbias.alloc((size_t)nc * W1 * 8)) || (rc = g->timepart.alloc((size_t)W1 * 8)) || (rc = g->ttmp.alloc(768 * 4)) ||
        (rc = g->ttmp64.alloc(512 * 8)) ||
        (rc = g->partial.alloc(rows * g->grid.tiles_per_b * W1 * 4)) || (rc = g->objdev.alloc(sizeof(TrunkObjective) * nc)) ||
        (rc = g->objidx.alloc(sizeof(int) * nc)))
        return rc;
    if (model->kind == 2) {
        if ((rc = g->objpart.alloc((size_t)std::max(1, cfg->max_objects) * W1 * 8))) return rc;
    } else {
        g->store.init(model, cfg->num_object_points, cfg->max_objects);
        g->rows.serial = g->serial; g->rows.l1tab = g->l1tab;
        if ((rc = g->rows.init(cfg->num_object_points, cfg->sub_batch_size, nc, g->grid.rows))) return rc;
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
    g->rows.force_slow_xobj = force_per_row == 1;       // 1: every row runs its own FPS; 2: per-row table kernel; 0: default (group kernel)
    g->rows.xobj_mode = force_per_row == 2 ? 2 : 0;     // (3 = the group gather kernel)
    g->l2_gather_mode = force_per_row == 4 ? 1 : 0;     // takes effect at the next dgdm_guidance_set_objects
    g->rows.xtab_enabled = force_per_row == 0 || force_per_row == 4 || force_per_row == 5;      // modes 1-3 read materialised rows
    g->xtab_policy = force_per_row == 5 ? 1 : 0;         // 5: the next set_objects builds the embedding tables right away
    if (out_fast_ok) {
        int rc = g->store.finish();
        if (rc) return rc;
        for (int i = 0; i < g->n_objects && i < g->store.size(); ++i) out_fast_ok[i] = g->store[i].fast_ok ? 1 : 0;
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
extern "C" int dgdm_guidance_set_objects(DgdmGuidance *g, const float *objects_dev, int n_objects, void *stream) {
    DGDM_REQUIRE(g && objects_dev && n_objects > 0, DGDM_EINVAL, "dgdm_guidance_set_objects: bad argument");
    DGDM_REQUIRE(n_objects <= std::max(1, g->cfg.max_objects), DGDM_EINVAL, "%d objects > max_objects %d", n_objects, g->cfg.max_objects);
    hipStream_t s = (hipStream_t)stream;
    int rc;
    if (g->m->kind == 2) {
        prof_begin(s, DGDM_STAGE_TABLES);
        // (a grow-only member, not a local: a local's hipFree - and the synchronize that had to precede it - stalled the host behind
        //  the previous batch's chains at every call)
        if ((rc = g->objtmp.alloc((size_t)n_objects * 512 * 8))) return rc;
        if ((rc = g->m->object_part_2d64(objects_dev, g->objtmp.as<double>(), g->objpart.as<double>(), n_objects, s))) return rc;
        prof_end(s, DGDM_STAGE_TABLES, 0.0);
    } else {
        BuildOptions o;
        o.bf16 = g->bf16; o.l2_gather = g->l2_gather_mode != 0; o.eager_xtab = g->xtab_policy == 1; o.l1tab = g->l1tab;
        o.off_stream = g->tables_off_stream();
        if ((rc = g->store.build(objects_dev, n_objects, o, s))) return rc;
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

int DgdmGuidance::embed(const int *oidx, int n_chains, const int64_t *starts_host, int n_calls, int64_t call_stride, Embedded *e, hipStream_t s) {
    DGDM_REQUIRE(starts_host, DGDM_EINVAL, "3-D guidance needs the FPS start indices");
    int rc;
    if (prof_on() && (rc = store.join(s))) return rc;      // the stage's events bracket the gather, not a wait for the build
    prof_begin(s, DGDM_STAGE_XOBJ);
    // The table X[s1][q] of an object costs about what 7 cond_fn calls spend gathering its rows (it holds all 262 144 (s1, q)
    // pairs; one call touches 36 000 of them): it pays as soon as the objects serve more than one 5-step chain - the
    // reference's validation sweep runs 12 objectives x 5 steps (+ the multi-object chains) on the same objects - and it would
    // cost 2 % when every pair brings its own object (bench.py).  So it is built when the call count says the objects are being
    // reused: when the calls since set_objects pass XTAB_AFTER.
    if (rows.tables_wanted()) {
        const bool crosses = grads_since_set <= XTAB_AFTER && grads_since_set + n_calls > XTAB_AFTER;
        grads_since_set += n_calls;
        if (crosses && (rc = store.join(s))) return rc;      // build_xtab reads the finished tables
        if (crosses)
            for (int i = 0; i < n_objects; ++i) {
                const ObjectTables &t = store[i];
                if (!(t.has16 ? t.has_x16 : t.has_x) && (rc = store.build_xtab(i, s))) return rc;
            }
    }
    if ((rc = rows.embed_rows(oidx, n_chains, starts_host, grid.rows, n_calls, call_stride, bf16, bf16, e, s))) return rc;
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
        emb->point(pp, rows, call, grid.rows);
    }
    return DGDM_OK;
}

int dgdm::check_objectives(const DgdmGuidance *g, const DgdmObjective *objectives, const float *rowcoef_dev, int n_chains) {
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

int dgdm::guidance_grad(DgdmGuidance *g, int kind, const float *x_dev, int timestep, const DgdmObjective *objectives, const float *rowcoef_dev,
                        const int64_t *starts_host, int n_chains, float *grad_dev, hipStream_t s, const Embedded *emb, int call, bool pre_done) {
    DGDM_REQUIRE(g && x_dev && objectives && grad_dev, DGDM_EINVAL, "guidance_grad: null argument");
    if (g->m->kind != kind) { set_error("model type not supported: %d-D entry point on a %d-D model", kind, g->m->kind); return DGDM_EMODE; }
    int rc;
    if ((rc = g->check_chains("", n_chains)) || (rc = check_objectives(g, objectives, rowcoef_dev, n_chains))) return rc;
    std::vector<int> oidx(n_chains);
    for (int i = 0; i < n_chains; ++i) oidx[i] = objectives[i].object;
    const std::vector<TrunkObjective> tob = to_trunk_objectives(objectives, n_chains);
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
    int rc;
    if ((rc = g->check_chains("dgdm_guidance_set_row_field: ", n_chains))) return rc;
    g->rowfield = field_dev; g->rowfield_chains = n_chains;
    return DGDM_OK;
}

extern "C" int dgdm_guidance_goal_field(DgdmGuidance *g, const float *goals_dev, const DgdmGoalSpec *specs_host, int n_chains, float *field_dev,
                                        void *stream) {
    DGDM_REQUIRE(g && goals_dev && specs_host && field_dev, DGDM_EINVAL, "dgdm_guidance_goal_field: null argument");
    int rc;
    if ((rc = g->check_chains("dgdm_guidance_goal_field: ", n_chains))) return rc;
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
    int rc;
    if ((rc = g->check_chains("", n_chains))) return rc;
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
    int rc;
    if ((rc = g->check_chains("", n_chains)) || (rc = check_objectives(g, objectives, rowcoef_dev, n_chains))) return rc;
    hipStream_t s = (hipStream_t)stream;
    const std::vector<TrunkObjective> tob = to_trunk_objectives(objectives, n_chains);
    if ((rc = g->valobj.alloc(sizeof(TrunkObjective) * g->cfg.max_chains))) return rc;
    DGDM_HIP_CHECK(hipMemcpyAsync(g->valobj.p, tob.data(), sizeof(TrunkObjective) * n_chains, hipMemcpyHostToDevice, s));
    return objective_values_launch(logits_dev, g->valobj.as<TrunkObjective>(), rowcoef_dev, g->rowfield, n_chains, g->B, g->grid.cells, values_dev, s);
}

extern "C" int dgdm_guidance_orientation_sweep(DgdmGuidance *g, const float *x_dev, const int32_t *object_of_chain, const int64_t *starts_host,
                                               int n_chains, float *logits_dev, void *stream) {
    DGDM_REQUIRE(g && x_dev && object_of_chain && logits_dev, DGDM_EINVAL, "dgdm_guidance_orientation_sweep: null argument");
    hipStream_t s = (hipStream_t)stream;
    const int kind = g->m->kind;
    int rc;
    if ((rc = g->check_chains("", n_chains)) || (rc = g->check_objects(object_of_chain, n_chains))) return rc;
    if ((rc = g->common_pre(x_dev, 0.f, object_of_chain, n_chains, s))) return rc;       // timesteps = zeros (:515,521)
    TrunkParams p;
    g->m->fill_trunk(&p);
    g->set_grid(&p, g->sweep, n_chains);
    if (kind == 3) {
        DGDM_REQUIRE(starts_host, DGDM_EINVAL, "3-D sweep needs the FPS start indices");
        // the sweep stays float32: table rows when the float32 tables exist, the gather kernels otherwise (e.g. a bf16-mode handle)
        DgdmGuidance::Embedded emb;
        if ((rc = g->rows.embed_rows(object_of_chain, n_chains, starts_host, g->sweep.rows, 1, 0, false, g->bf16, &emb, s))) return rc;
        emb.point(&p, g->rows, 0, g->sweep.rows);
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
    int rc;
    if ((rc = g->check_chains("", n_chains)) || (rc = g->check_objects(object_of_chain, n_chains))) return rc;
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
    if (kind == 3 && (rc = g->rows.embed_rows(object_of_chain, n_chains, starts_host, Rs, K, (int64_t)n_chains * 2 * Rs, false, g->bf16, &emb, s))) return rc;
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
        if (kind == 3) emb.point(&p, g->rows, k, Rs);
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

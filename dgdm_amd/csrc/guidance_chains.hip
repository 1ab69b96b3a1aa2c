// The denoise loop as one call: dgdm_guided_chains_run* on a guidance handle (guidance.h) and an eps-net, and dgdm_cfg_mix.
#include "guidance.h"
#include <algorithm>
#include <cmath>
#include <cstdlib>

using namespace dgdm;

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
    // classifier-free copies and mix, and step 0's replication) runs on the object store's first build stream beside common_pre's
    // latency-bound float64 kernels, between two events: fork_ev on `s` once x_t is final, side_ev on the side stream, which `s` waits
    // for in front of the trunk (beside the trunk itself the eps-net costs the trunk what it saves: DESIGN.md 4.3b) - every call's
    // side work is joined into `s` before the call returns.  A 3-D step 0 stays on `s`: the side stream may still be building the
    // tables.  What reads no table - all of the above and common_pre - is enqueued BEFORE the step's embed(), which joins `s` to the
    // build: step 0 runs it beside the build.
    const bool hoist = g->hoist_x_only(), beside = g->eps_beside();
    hipStream_t side = s;
    if (beside && (rc = g->store.first_stream(&side))) return rc;
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
        if (fork && ((rc = g->fork_ev.record(s)) || (rc = g->fork_ev.wait(es)))) return rc;
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
        if (fork && (rc = g->side_ev.record(es))) return rc;
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
        if (fork && (rc = g->side_ev.wait(s))) return rc;
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
                (void)g->side_ev.record(side);
                (void)g->side_ev.wait(s);
            }
            return rc;
        }
    DGDM_HIP_CHECK(hipGetLastError());
    return DGDM_OK;
}

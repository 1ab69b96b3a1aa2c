/*
 * dgdm_hip.h - C-ABI of the MI355X (gfx950) guided-sampling library, libdgdm_hip.so.
 *
 * The reference (real-stanford/dgdm @ 2024_08_07) has no FFI layer: its hot path is Python
 * calling torch.nn modules.  This header is the boundary the replacement sits behind.  Each
 * entry point names the reference interface it stands in for (paths relative to the
 * reference tree); INTEGRATION.md shows the ctypes binding a maintainer adds on the
 * reference side.  Plain C types only: device pointers, sizes, a hipStream_t passed as void*.
 *
 * Conventions
 *  - every function returns 0 on success, a negative DGDM_E* code otherwise;
 *    dgdm_last_error() gives the message (thread-local).  The Python shim turns the codes into
 *    the reference's exceptions (ValueError('opt obj not supported'), ...).
 *  - "dev" pointers are HIP device memory owned by the caller; "host" pointers are ordinary
 *    memory.  Model handles own their packed weights and workspaces in device memory.
 *  - all floating point is IEEE binary32; timesteps / point indices are int64 on the host side
 *    (as in the reference) and int32 on the device side.
 *  - launches go to the stream given; nothing here synchronises unless documented.
 */
#ifndef DGDM_HIP_H
#define DGDM_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DGDM_OK            0
#define DGDM_EINVAL       -1   /* bad argument / unsupported shape                          */
#define DGDM_EKEY         -2   /* state_dict key missing or wrong size                      */
#define DGDM_EHIP         -3   /* HIP runtime error (message carries hipGetErrorString)     */
#define DGDM_EOBJECTIVE   -4   /* 'opt obj not supported'   (generator/diffusion.py:470)    */
#define DGDM_EMODE        -5   /* 'model type not supported' (generator/diffusion.py:502)   */
#define DGDM_ENODEVICE    -6   /* no gfx950 device visible                                  */

/* One host tensor of a reference-format state_dict (torch layout, contiguous). */
/* contraction dtypes of dgdm_unet1d_set_contraction_dtype / dgdm_guidance_set_contraction_dtype */
enum { DGDM_DTYPE_F32 = 0, DGDM_DTYPE_BF16 = 1, DGDM_DTYPE_F32_MFMA = 2, DGDM_DTYPE_F32_F16X3 = 3 };      /* (4, the six-bf16-product form of rounds 3-5, is retired: DGDM_EINVAL) */

typedef struct DgdmTensor {
    const char *name;     /* e.g. "linears.3.weight", "module."-prefix already stripped     */
    const void *data;     /* host memory                                                    */
    int64_t     numel;
    int32_t     dtype;    /* 0 = float32, 1 = int64                                         */
} DgdmTensor;

typedef struct DgdmUnet1d   DgdmUnet1d;    /* generator/diffusion_utils.py:123 ConditionalUnet1D        */
typedef struct DgdmDynamics DgdmDynamics;  /* dynamics/profile_forward_{2d,3d}.py ProfileForward{2,3}DModel */
typedef struct DgdmGuidance DgdmGuidance;  /* state of Diffusion.cond_fn for a batch of chains           */

/* Objective of Diffusion.deltas_to_objective (generator/diffusion.py:430-471) in gradient form:
 *   d objective / d delta_j = lin[j] + 2*quad[j]*delta_j                     (all but 'convergence')
 * 'convergence' sets use_rowcoef: d objective / d delta_0 of reference row r is rowcoef[r],
 * the signed multiplicity of r in the slicer() windows (dynamics/metrics.py:32-38), built by
 * dgdm_convergence_rowcoef().
 * use_rowcoef == DGDM_OBJ_ROWFIELD adds a per-row term for all three outputs instead:
 *   d objective / d delta_j of row r = lin[j] + 2*quad[j]*delta_j + field[r][j]
 * with the field given to dgdm_guidance_set_row_field() (with lin = quad = 0 the seed is the field
 * value itself, bit for bit).                                                                   */
#define DGDM_OBJ_ROWFIELD 2
typedef struct DgdmObjective {
    float   lin[3];
    float   quad[3];
    int32_t use_rowcoef;  /* 0: lin / quad only; 1: rowcoef ('convergence'); DGDM_OBJ_ROWFIELD       */
    int32_t object;       /* index into the object bank given to dgdm_guidance_set_objects      */
} DgdmObjective;

/* ------------------------------------------------------------------ library */
int         dgdm_version(void);
const char *dgdm_last_error(void);
/* 0 when device `ordinal` exists and is gfx950; selects it for this thread. */
int         dgdm_device_init(int ordinal);
/* Fills *out (lin/quad/use_rowcoef) for a reference objective name; DGDM_EOBJECTIVE otherwise. */
int         dgdm_objective_from_name(const char *opt_obj, DgdmObjective *out);

/* ------------------------------------------------------------------ a7: noise-prediction net
 * ConditionalUnet1D(input_dim=1, global_cond_dim, down_dims, diffusion_step_embed_dim,
 * kernel_size=5, n_groups=8)  (generator/diffusion_utils.py:124-236).  global_cond_dim (0..256) is read from the state dict: the
 * in_features of every `*.cond_encoder.1.weight` minus step_embed_dim; the eight blocks must agree (DGDM_EINVAL names the tensor).
 *
 * Accepted domain (everything else is DGDM_EINVAL from the host code, before any launch; tests/test_gpu_unet_shapes.py runs it):
 *   n_down          2 (down_dims = {d0, d1}); kernel_size 5; input_dim 1
 *   d0, d1          multiples of 128 (16-channel MFMA tiles, accumulation chunks of 128 input channels); d0 == d1 is allowed
 *   n_groups        >= 1 and a divisor of both widths
 *   step_embed_dim  even, 4 ... 64 (widths that are no multiple of 8 are padded with zero weight rows; above 64 the float32 chains of
 *                   the step encoder no longer hold 1e-6 against float64)
 *   L (forward)     even, 2 ... 64, and one sample's activations must fit the 160 KiB LDS.  With CPx = x + 8, L2 = L / 2:
 *                     floats = max((L+4) CP(d0), (L2+4) CP(2 d1)) + 3 max((L+4) CP(d0), (L2+4) CP(d1)) + 16 max(d0, d1)
 *                              + pad8(step_embed_dim) + max(4 step_embed_dim, pad8(global_cond_dim)) + L + 23,   4 floats <= 163840.
 *                   Largest L: 46 for (128, 256), 64 for (128, 128), 28 for (256, 256), 26 for (128, 384), 16 for (256, 512).
 *                   The default arithmetic (three f16 products) needs 64 + 256 (L + 4) bytes more for its split slabs; where only that
 *                   does not fit - (128, 256): L = 44, 46; (128, 128): 60 ... 64; (256, 256): 28; (128, 384): 26 - the float32 MFMA chain runs instead
 *                   and dgdm_unet1d_effective_form says so.
 *   batched form    (large batches) only for (128, 256) and step_embed_dim <= 32; other nets run the per-sample kernel at every B.  */
int dgdm_unet1d_create(DgdmUnet1d **out, const DgdmTensor *state_dict, int n_tensors,
                       const int32_t *down_dims, int n_down, int step_embed_dim, int kernel_size, int n_groups);
void dgdm_unet1d_destroy(DgdmUnet1d *m);
int dgdm_unet1d_global_cond_dim(const DgdmUnet1d *m);      /* negative: null handle */
/* ConditionalUnet1D.forward (diffusion_utils.py:238-285): sample_dev [B][L] (input_dim 1),
 * timestep_dev [B] int32 (one per sample), eps_dev [B][L].                                      */
int dgdm_unet1d_forward(DgdmUnet1d *m, const float *sample_dev, const int32_t *timestep_dev, float *eps_dev,
                        int B, int L, void *stream);
/* The same with global_cond (diffusion_utils.py:254-257): global_cond_dev [B][global_cond_dim], one row per sample.  Every block's
 * FiLM vector is Linear(Mish(cat(step embedding, global_cond row))), float32 in every contraction mode.  With global_cond_dim 0 the
 * condition is ignored (NULL: the call above, bit for bit); with global_cond_dim > 0 a NULL condition - and so dgdm_unet1d_forward -
 * is DGDM_EINVAL, before anything is launched.                                                                                    */
int dgdm_unet1d_forward_cond(DgdmUnet1d *m, const float *sample_dev, const int32_t *timestep_dev, const float *global_cond_dev,
                             float *eps_dev, int B, int L, void *stream);
/* Classifier-free guidance mix, elementwise: out = eps_u + w * (eps_c - eps_u), the three float32 operations each rounded on its own
 * (no fused multiply-add).  out may be either input.                                                                              */
int dgdm_cfg_mix(const float *eps_c_dev, const float *eps_u_dev, float w, float *out_dev, int64_t numel, void *stream);
/* Arithmetic of the convolutions with more than one input and output channel.  DGDM_DTYPE_F32 (default, the parity path):
 * float32-grade on the f16 matrix pipe - every float32 product as three f16 MFMA products on operands scaled by exact powers of two
 * (per convolution's weights, per sample and convolution input) and split in two f16 pieces, float32 accumulation (DESIGN_HISTORY.md 4.2;
 * closer to float64 than the float32 MFMA chain).  DGDM_DTYPE_F32_F16X3 selects the same form; DGDM_DTYPE_F32_MFMA the float32 MFMA
 * chain (also used where the split form's LDS slabs do not fit: L = 44, 46);
 * DGDM_DTYPE_BF16: weights and activations entering those convolutions rounded to bf16, float32 accumulation (BASELINE configs[4]).
 * GroupNorm, Mish, FiLM, residual adds, the Linear layers and the single-channel first/last convolutions are float32 in every mode.   */
int dgdm_unet1d_set_contraction_dtype(DgdmUnet1d *m, int dtype);
/* What a dgdm_unet1d_forward call with B samples of L control points actually runs: the DGDM_DTYPE_* of its convolutions
 * (DGDM_DTYPE_F32_F16X3, DGDM_DTYPE_F32_MFMA - also where the split form's slabs do not fit the LDS - or DGDM_DTYPE_BF16), + 16 when the
 * layer-by-layer batched form is used (large batches; the same bits as the per-sample kernel).  Negative: bad argument.  Depends on the
 * handle's global_cond_dim: up to 128 the condition row shares LDS the step encoder has finished with, beyond that it adds to the footprint. */
int dgdm_unet1d_effective_form(const DgdmUnet1d *m, int B, int L);

/* ------------------------------------------------------------------ a13/a14: scheduler step
 * noise_pred - sqrt(1-abar_t)*grad*scale  (generator/diffusion.py:575,645) followed by
 * DDIMScheduler.step(eta=0, clip_sample=True).prev_sample (diffusers 0.11.1; call sites
 * diffusion.py:201,256,576,647).  grad_dev may be NULL (unguided loops :193-201, :249-256).
 * grad_dev holds n_grad stacked gradients [n_grad][n]; their mean is used
 * (guided_sample_multi_object :640-644).  The four square roots are float32 values computed
 * by the host scheduler exactly as the reference computes them.                                 */
int dgdm_ddim_guided_step(const float *x_dev, const float *eps_dev, const float *grad_dev, int n_grad,
                          float *x_next_dev, int64_t n, float sqrt_abar_t, float sqrt_1m_abar_t,
                          float sqrt_abar_prev, float sqrt_1m_abar_prev, float guidance_scale, void *stream);
/* Editing a design: dgdm_ddim_guided_step with the clip of the predicted clean sample per entry,
 * x0 = min(max(x0, lo[i % period]), hi[i % period]), instead of clip_sample=True's [-1, 1].  lo = -1, hi = 1 is that step bit for bit;
 * lo == hi == v pins an entry: its predicted clean value is v at every step, its noisy state sqrt(abar_prev) v + sqrt(1-abar_prev) eps
 * stays a consistent DDIM state for the eps-net, and after the last step (sqrt(abar_prev) = 1, sqrt(1-abar_prev) = 0) it is exactly v;
 * lo = max(-1, d-u), hi = min(1, d+u) is a band of half-width u around a design d.  An edit starts from add_noise(design, noise, t)
 * and runs the schedule's last steps: the move the reference's first validation loop makes with its data (generator/diffusion.py:184-201).
 * The per-entry clip itself is this project's own: the reference has no counterpart to pin it to.
 * lo_dev / hi_dev [period] float32, period > 0 divides n (period = B*L: one block shared by all chains); a NULL bound, period <= 0 or
 * a period that does not divide n: DGDM_EINVAL before anything is launched.  Precondition, not checked on the device:
 * -1 <= lo <= hi <= 1, finite (any finite bounds are safe: they are only operands of the clamp).                                   */
int dgdm_ddim_guided_step_bounded(const float *x_dev, const float *eps_dev, const float *grad_dev, int n_grad, float *x_next_dev, int64_t n,
                                  float sqrt_abar_t, float sqrt_1m_abar_t, float sqrt_abar_prev, float sqrt_1m_abar_prev, float guidance_scale,
                                  const float *lo_dev, const float *hi_dev, int64_t period, void *stream);
/* The stochastic step, eta > 0 (extends dgdm_ddim_guided_step / _bounded; diffusers 0.11.1 DDIMScheduler.step(eta, variance_noise),
 * restated from the published algorithm - parity unpinned, as the eta = 0 step):
 *   x_prev = sqrt_abar_prev * clip(x0) + dir * eps + sigma * z,  rounded as add(add(mul, mul), mul), nothing fused;
 *   sigma = eta * sqrt((1 - abar_prev) / (1 - abar_t) * (1 - abar_t / abar_prev)),  dir = sqrt(1 - abar_prev - sigma^2)   (host, float32).
 * lo_dev == hi_dev == NULL: the [-1, 1] clip; both given: the per-entry clip of _bounded (period as there).
 * z is noise_dev[i] when noise_dev is given (diffusers' variance_noise), otherwise the keyed device normal below.
 * sigma == 0 launches the eta = 0 kernel with sqrt_1m_abar_prev = dir: bit for bit dgdm_ddim_guided_step / _bounded.
 *
 * The keyed normal (THE recipe: tests/step_noise_oracle.py states the same text in numpy).  Entry i of the step belongs to chain
 * c = i / per_chain and is element e = i % per_chain of it (per_chain > 0 divides n; chain_keys_dev [n / per_chain] uint64, device):
 *   r0, r1 = raw outputs 2e, 2e + 1 of numpy.random.Philox(key=[seed, chain_keys[c]], counter=[0, step_index, 0, 0]).random_raw():
 *            Philox4x64-10, block counter (e / 2 + 1, step_index, 0, 0) (numpy counts up before a block), lanes 2 (e & 1), 2 (e & 1) + 1;
 *   u1 = ((r0 >> 11) + 1) * 2^-53  in (0, 1],   u2 = (r1 >> 11) * 2^-53  in [0, 1);
 *   z  = (float)( sqrt(-2 ln u1) * cos(6.283185307179586 * u2) )    every operation float64, one rounding to float32 at the end.
 * z depends on (seed, chain key, step_index, e) only - not on the chain's place in the launch, the launch geometry, the rank or how a
 * run is split into calls.  |z| <= sqrt(2 * 53 ln 2) < 8.6: always finite.                                                            */
int dgdm_ddim_guided_step_noisy(const float *x_dev, const float *eps_dev, const float *grad_dev, int n_grad, float *x_next_dev, int64_t n,
                                float sqrt_abar_t, float sqrt_1m_abar_t, float sqrt_abar_prev, float dir, float guidance_scale,
                                const float *lo_dev, const float *hi_dev, int64_t period, float sigma, const float *noise_dev,
                                uint64_t seed, const uint64_t *chain_keys_dev, int64_t step_index, int64_t per_chain, void *stream);
/* Debug / test entry: the z values of the recipe above -> z_dev [n_chains][per_chain] float32. */
int dgdm_ddim_step_noise(uint64_t seed, const uint64_t *chain_keys_dev, int n_chains, int64_t step_index, int64_t per_chain, float *z_dev,
                         void *stream);
/* DDIMScheduler.add_noise (diffusion.py:145,185): out = sqrt_abar*x0 + sqrt_1m_abar*noise */
int dgdm_ddim_add_noise(const float *x0_dev, const float *noise_dev, float *out_dev, int64_t n,
                        float sqrt_abar, float sqrt_1m_abar, void *stream);
/* The predicted clean sample the DDIM steps above form, on its own, from the unguided eps and with clip_sample's [-1, 1]:
 *   out = fmin(fmax(fdiv_rn(sub_rn(x, mul_rn(sqrt_1m_abar_t, eps)), sqrt_abar_t), -1), 1)    float32, elementwise, nothing fused
 * - the bits dgdm_ddim_guided_step's x0 has when grad_dev is NULL.  A NaN passes through as fmaxf / fminf give it.  n >= 0; a NULL
 * pointer is DGDM_EINVAL.                                                                                                          */
int dgdm_ddim_pred_x0(const float *x_dev, const float *eps_dev, float *out_dev, int64_t n, float sqrt_abar_t, float sqrt_1m_abar_t,
                      void *stream);

/* ------------------------------------------------------------------ a8-a12: dynamics models
 * kind 2: ProfileForward2DModel(W=256, params_ch, object_ch) (dynamics/profile_forward_2d.py:78-135)
 * kind 3: ProfileForward3DModel(W=256, params_ch)            (dynamics/profile_forward_3d.py:13-65)
 * BatchNorm layers are folded with their running statistics (the reference runs the classifier
 * in eval mode with frozen parameters: generator/train.py:91-92).
 *
 * Accepted domain (tests/test_gpu_grad_shapes.py runs its edges through the guidance gradient): kind 2 or 3 (else DGDM_EMODE);
 * params_ch 1..256 (else DGDM_EINVAL); object_ch: kind 2 any size, it has to be the
 * input width of the state dict's object_encoder.0 (a tensor of another size is DGDM_EKEY, like a missing one); kind 3 ignores it.
 * The hidden width is the reference's W = 256.                                                                                       */
int dgdm_dynamics_create(DgdmDynamics **out, int kind, const DgdmTensor *state_dict, int n_tensors,
                         int params_ch, int object_ch);
void dgdm_dynamics_destroy(DgdmDynamics *m);

/* ProfileForward2DModel.forward (profile_forward_2d.py:137-156) on `rows` arbitrary rows:
 * x_ctrl [rows][params_ch], x_ori [rows][1], x_pos [rows][2], t [rows] (already divided by
 * num_train_timesteps, as cond_fn passes it), object [rows][object_ch] -> logits [rows][3].     */
int dgdm_dyn2d_forward(DgdmDynamics *m, const float *x_ctrl_dev, const float *x_ori_dev, const float *x_pos_dev,
                       const float *t_dev, const float *object_dev, float *logits_dev, int rows, void *stream);

/* PointNet2.forward (dynamics/models/pointnet2.py:21-32): xyz_dev [rows][3][N] (channel-major, as
 * the reference passes it), FPS start indices of sa1 and sa2 for every row (the values
 * torch.randint draws at pointnet2_utils.py:83) in host memory -> emb_dev [rows][256].
 * Rows holding bit-identical clouds share the per-cloud work.                                   */
int dgdm_pointnet2_forward(DgdmDynamics *m, const float *xyz_dev, const int64_t *start_sa1_host,
                           const int64_t *start_sa2_host, float *emb_dev, int rows, int N, void *stream);

/* ProfileForward3DModel.forward (profile_forward_3d.py:67-86): x_ctrl [rows][3][params_ch]
 * (only channel 1 is read, :78), object xyz [rows][3][N], FPS starts as above.                  */
int dgdm_dyn3d_forward(DgdmDynamics *m, const float *x_ctrl_dev, const float *x_ori_dev, const float *x_pos_dev,
                       const float *t_dev, const float *xyz_dev, const int64_t *start_sa1_host,
                       const int64_t *start_sa2_host, float *logits_dev, int rows, int N, void *stream);

/* The index functions of dynamics/models/pointnet2_utils.py on their own, for arbitrary batches of clouds (the guided path reads
 * per-object tables built by the same device code instead; these exist so that the reference's names run on the device and can be
 * compared one to one).  Indices are int32 on the device.
 *   farthest_point_sample(xyz, npoint)        :71-92   xyz_dev [B][N][3] (N <= 1024); start_host [B] = the torch.randint draw of :83
 *   query_ball_point(radius, nsample, xyz, new_xyz) :95-115   radius_squared = float32(radius ** 2); out [B][S][nsample], first
 *                                             in-radius indices in ascending order, padded with the first (N if the ball is empty)
 *   square_distance(src, dst)                 :27-48   out [B][S][N], the expanded form in the reference's operation order
 *   index_points(points, idx)                 :51-68   points [B][N][C], idx [B][M] -> out [B][M][C]; an index outside [0, N) (where
 *                                                      the reference's indexing raises) yields NaN; empty inputs give empty results  */
int dgdm_farthest_point_sample(const float *xyz_dev, const int64_t *start_host, int B, int N, int npoint, int32_t *out_dev, void *stream);
int dgdm_query_ball_point(float radius_squared, int nsample, const float *xyz_dev, const float *new_xyz_dev, int B, int N, int S,
                          int32_t *out_dev, void *stream);
int dgdm_square_distance(const float *src_dev, const float *dst_dev, int B, int S, int N, float *out_dev, void *stream);
int dgdm_index_points(const float *points_dev, const int32_t *idx_dev, int B, int N, int M, int C, float *out_dev, void *stream);
/* PointNetSetAbstraction.forward on its own (pointnet2_utils.py:184-210, eval mode): after sample_and_group (the functions above) the shared
 * MLP is applied to the grouped rows layer by layer - y = act(x W^T + b) with the eval-mode BatchNorm folded into W, b by the caller;
 * wt_dev [K][N] (W transposed), x_dev [rows][ldx], y_dev [rows][ldy], act 0 none / 1 ReLU / 2 SiLU - and the result is reduced with the
 * max over each group's nsample rows (:206): x_dev [groups][nsample][C] -> out_dev [groups][C].                                       */
int dgdm_linear_act(const float *x_dev, int ldx, const float *wt_dev, const float *bias_dev, float *y_dev, int ldy, int rows, int K, int N,
                    int act, void *stream);
int dgdm_group_max(const float *x_dev, int64_t groups, int nsample, int C, float *out_dev, void *stream);
/* Test hooks: the float64 stages around the trunk on the caller's operands.  dgdm_debug_linear64: y = act(x wt + bias), all doubles,
 * wt_dev [K][N].  dgdm_debug_dyn_post64: cond_fn's backward tail for `rows` fingers - partial_dev [rows][tiles_per_b][W1] float32 summed
 * over the tiles, then through w1c_dev [W1][256], g2w_dev [256][256], the ReLU mask of V_dev [rows][256] and g0w_dev [256][L] ->
 * grad_dev [rows][L] float32; every dot product one ascending chain of float64 fmas.                                                  */
int dgdm_debug_linear64(const double *x_dev, int ldx, const double *wt_dev, const double *bias_dev, double *y_dev, int ldy, int rows, int K,
                        int N, int act, void *stream);
int dgdm_debug_dyn_post64(int W1, const float *partial_dev, int tiles_per_b, const double *w1c_dev, const double *g2w_dev,
                          const double *g0w_dev, const double *V_dev, float *grad_dev, int rows, int L, void *stream);

/* ------------------------------------------------------------------ a4-a6: guidance gradient
 * One DgdmGuidance serves up to max_chains independent chains (object x objective pairs) that
 * share B fingers, the (grid_size, num_pos, ori_range) pose grid and the timestep; each chain
 * has its own x [B][L].  This is Diffusion.cond_fn (generator/diffusion.py:473-504) with the
 * R = B*grid_size*num_pos^2 replicated rows evaluated without materialising them.              */
typedef struct DgdmGuidanceConfig {
    int32_t batch;            /* B fingers per chain                                            */
    int32_t grid_size;        /* G  (--grid_size)                                               */
    int32_t num_pos;          /* P  (--num_pos)                                                 */
    float   ori_lo, ori_hi;   /* ori_range                                                      */
    int32_t max_chains;
    int32_t num_train_timesteps;
    int32_t sub_batch_size;   /* 3-D: --sub_bs; it fixes which rows share a torch.randint call  */
    int32_t num_object_points;/* 3-D: N points per object cloud; 2-D: vertices per contour      */
    int32_t max_objects;
} DgdmGuidanceConfig;

/* Accepted domain (everything else is DGDM_EINVAL from the host code, and no handle; tests/test_gpu_grad_shapes.py holds the gradient and
 * the logits to the oracle in float64 at its edges - one row, one cell, a cell count that is no multiple of a 32-row tile, params_ch 1 and
 * 256, 256 chains, the first and the last timestep):
 *   batch, grid_size, num_pos      any positive value (a one-cell grid takes ori_lo and position -1, as torch.linspace with one step does)
 *   ori_lo, ori_hi                 any pair, equal or descending included: linspace(ori_lo, ori_hi, grid_size)
 *   max_chains                     1..256 (DGDM_MAX_CHAINS); a call takes n_chains in 1..max_chains
 *   num_train_timesteps            any positive value; a call's timestep enters as float32(timestep) / float32(num_train_timesteps)
 *   sub_batch_size                 3-D: any positive value, larger than the row count included; 2-D: not read
 *   num_object_points              2-D: object_ch / 2 of the model; 3-D: 1..1024 - N = 512 is the only cloud size the test suite holds to
 *                                  the oracle
 *   max_objects                    values below 1 count as 1; an objective's object index is held to the objects set, at every call   */
int  dgdm_guidance_create(DgdmGuidance **out, DgdmDynamics *model, const DgdmGuidanceConfig *cfg);
void dgdm_guidance_destroy(DgdmGuidance *g);
/* Arithmetic of the trunk contractions inside dgdm_dyn{2,3}d_guidance_grad.  DGDM_DTYPE_F32 (default, the parity path) =
 * DGDM_DTYPE_F32_F16X3: float32 operands as two f16 pieces each after exact power-of-two scaling (per weight matrix, per tile row),
 * three f16 MFMAs per product with float32 accumulation (csrc/trunk_f16l.hip: 1.9e-7 rms of a 256-term contraction vs float64;
 * DESIGN_HISTORY.md 4.12).  DGDM_DTYPE_F32_MFMA: the k-ordered
 * float32 fma chain itself (v_mfma_f32_32x32x2_f32; 2.0e-7).  DGDM_DTYPE_BF16 (BASELINE configs[4]: "bf16 contractions, f32
 * accumulate"): weights and the activations/gradients entering a contraction rounded to bf16 (nearest even), float32 accumulation;
 * first-layer tables, biases, objective and row sums stay float32.  The reference has no such switch (it calls
 * torch.set_float32_matmul_precision('high'), generator/diffusion.py:102, which is a no-op on its CPU path).          */
int  dgdm_guidance_set_contraction_dtype(DgdmGuidance *g, int dtype);
/* Objects the chains refer to.  2-D: objects_dev [n][num_vertices][2] (flattened to object_ch as
 * cond_fn does, diffusion.py:485).  3-D: objects_dev [n][N][3]; builds the per-object PointNet++
 * tables (DESIGN_HISTORY.md §4) on `stream`.                                                            */
int  dgdm_guidance_set_objects(DgdmGuidance *g, const float *objects_dev, int n_objects, void *stream);
/* Rows of the pose grid per chain: R = B * G * P * P (reference row r = cell*B + b). */
int64_t dgdm_guidance_rows(const DgdmGuidance *g);
/* 3-D only: number of int64 FPS start indices one cond_fn call consumes per chain (= 2*R:
 * for every sub-batch, sa1's draw then sa2's, pointnet2_utils.py:83 via diffusion.py:495-498). */
int64_t dgdm_guidance_starts_per_call(const DgdmGuidance *g);

/* Diffusion.cond_fn for n_chains chains at once.
 *   x_dev        [n_chains][B][L]       current samples
 *   timestep     the (shared) integer diffusion timestep t; the model sees t/num_train_timesteps
 *   objectives   [n_chains] host array (objective + object index per chain)
 *   rowcoef_dev  [n_chains][R] or NULL  (only read for chains with use_rowcoef == 1)
 *   starts_host  3-D: [n_chains][starts_per_call] int64 in the order the reference draws them;
 *                2-D: NULL
 *   grad_dev     [n_chains][B][L]       d sum(objective) / d x                                 */
int dgdm_dyn2d_guidance_grad(DgdmGuidance *g, const float *x_dev, int timestep, const DgdmObjective *objectives,
                             const float *rowcoef_dev, int n_chains, float *grad_dev, void *stream);
int dgdm_dyn3d_guidance_grad(DgdmGuidance *g, const float *x_dev, int timestep, const DgdmObjective *objectives,
                             const float *rowcoef_dev, const int64_t *starts_host, int n_chains, float *grad_dev,
                             void *stream);

/* Row field: a per-row seed for all three outputs, for chains whose use_rowcoef == DGDM_OBJ_ROWFIELD (no counterpart in the reference,
 * whose objectives are one direction for every row, or 'convergence' on delta_0).
 * field_dev [n_chains][R][3] float32 (row r = cell*B + b as in cond_fn) or NULL to clear. The pointer is kept, not copied:
 * it must stay valid for every later grad / chains_run call on the handle. Read only for chains whose use_rowcoef == 2:
 *   d objective / d delta_j of row r of chain i = lin[j] + 2*quad[j]*delta_j + field[(i*R + r)*3 + j]
 * In dgdm_guided_chains_run, chain i runs over the n_grad * n_chains gradient chains in objectives[] order.
 * A chain with use_rowcoef == 2 while no field is set, or whose index is not below the n_chains given here, makes grad / chains_run
 * return DGDM_EINVAL before anything is launched.  All three contraction dtypes take it.                                              */
int dgdm_guidance_set_row_field(DgdmGuidance *g, const float *field_dev, int n_chains, void *stream);

/* Goal field: the row field that pulls every pose of the cond_fn grid toward a goal pose, built on the device.
 * goals_dev [n_chains][B][3] float32 = (ori, pos_x, pos_y) per finger in the model's normalised inputs (ori = theta/pi - 1, pos = m / 0.03);
 * specs_host [n_chains]; field_dev [n_chains][R][3].
 * Row r = cell*B + b, cell = (g*P + px)*P + py; ori[] / pos[] are the handle's own float32 grids (linspace(ori_range, G),
 * linspace(-1, 1, P)); everything below in float64:
 *   u0 = goal_ori - ori[g], minus 2 if > 1, plus 2 if < -1 (the shorter way round); u1 = goal_x - pos[px]; u2 = goal_y - pos[py]
 *   half-widths h0 = ori_window (0 < h0 <= 1), h1 = h2 = pos_window (> 0)
 *   profile 0 (sign):   s_j = sign(u_j) if 0 < |u_j| <= h_j, else 0        profile 1 (linear): s_j = clamp(u_j / h_j, -1, 1)
 *   field[r][j] = float32(weight[j] * s_j), the product formed in double and rounded once.
 * The sign is the roll-out's (state += logits * scale): a positive entry rewards motion toward the goal.  A window out of range, a
 * non-finite goal or weight, an unknown profile: DGDM_EINVAL.  Reads the goals back once (one stream synchronisation).             */
typedef struct DgdmGoalSpec { float weight[3]; float ori_window; float pos_window; int32_t profile; /* 0 sign, 1 linear */ } DgdmGoalSpec;
int dgdm_guidance_goal_field(DgdmGuidance *g, const float *goals_dev, const DgdmGoalSpec *specs_host, int n_chains, float *field_dev, void *stream);

/* Forward-only scoring on the cond_fn grid: Diffusion.cond_fn's forward half (generator/diffusion.py:473-504: the classifier on every
 * (finger, orientation, position) row at one timestep) and, per (chain, finger), the tally of the classes :506-532 assigns
 * (2 if l > thr[k], 0 if l < -thr[k], else 1; thr in the model's normalised units, threshold / std).
 *   object_of_chain [n_chains] host; starts_host (3-D) as dgdm_dyn3d_guidance_grad takes them, NULL in 2-D
 *   logits_dev  [n_chains][R][3], row r = cell * B + finger as in cond_fn; NULL: kept in the handle's scratch
 *   counts_dev  [n_chains][B][27] joint histogram, bin = (class of d0 * 3 + class of d1) * 3 + class of d2; each sums to G * P^2
 *   sums_dev    [n_chains][B][4]  sum d0, sum |d0|, sum d1, sum d2 over the finger's cells
 * Contraction dtypes f32 / f32_f16x3 (forward-only form of the f16x3 trunk) and f32_mfma; bf16: DGDM_EINVAL.  Bit-identical run to run;
 * leaves what dgdm_dyn{2,3}d_guidance_grad computes untouched.                                                                      */
int dgdm_guidance_score(DgdmGuidance *g, const float *x_dev, int timestep, const int32_t *object_of_chain,
                        const int64_t *starts_host, const float thr[3], int n_chains, float *logits_dev, int32_t *counts_dev,
                        float *sums_dev, void *stream);

/* ------------------------------------------------------------------ resampling fingers by predicted objective
 * The B fingers of a chain as particles of a stochastic run (eta > 0): weighted by the objective whose gradient guides the chain, the
 * promising ones copied over the poor ones, the keyed step noise parting the copies again.  No counterpart in the reference.
 *
 * The objective's VALUE per (chain, finger) (THE recipe: tests/resample_oracle.py states the same text in numpy).
 *   logits_dev  [n_chains][R][3] float32: what dgdm_guidance_score writes, row r = cell * B + b
 *   objectives  [n_chains] host; rowcoef_dev [n_chains][R] or NULL; the row field is the handle's (dgdm_guidance_set_row_field)
 *   values_dev  [n_chains][B] float64
 * For chain i and finger b, over the rows r with r % B == b, every delta widened to double, every product and sum in double:
 *   V = sum_rows [ sum_j (lin[j] * delta_j + quad[j] * delta_j^2) + (use_rowcoef == 1 ? rowcoef[i][r] * delta_0 : 0)
 *                  + (use_rowcoef == 2 ? sum_j field[i][r][j] * delta_j : 0) ]
 * Its derivative in delta is the gradient form of DgdmObjective above; for the reference's names it is
 * deltas_to_objective(...).sum() (generator/diffusion.py:430-471) over the rows that depend on finger b.
 * Validation as dgdm_dyn{2,3}d_guidance_grad: a chain that uses rowcoef without one, or the row field while none is set or one that
 * does not reach its index, is DGDM_EINVAL before anything is launched.  One wave per (chain, finger), a fixed reduction order:
 * bit-identical run to run.                                                                                                        */
int dgdm_guidance_objective_values(DgdmGuidance *g, const float *logits_dev, const DgdmObjective *objectives, const float *rowcoef_dev,
                                   int n_chains, double *values_dev, void *stream);

/* One weight / effective-sample-size / systematic-resampling step for n_chains chains of B fingers of L entries.
 *   x_dev [n_chains][B][L]; values_dev [n_grad * n_chains][B] float64, object-major as the gradients are; beta_per_cell: the caller's
 *   beta with 1 / (G P^2) folded in; ess_frac; seed, chain_keys_dev [n_chains] uint64 (device), step_index: the keys of the step noise
 *   in / out: logw_dev, vprev_dev [n_chains][B] float64 - the log weights and the last potentials of a run, zero at its start
 *   out: x_out_dev [n_chains][B][L] (must not overlap x_dev), ancestors_dev [n_chains][B] int32, ess_dev [n_chains] float64,
 *        did_dev [n_chains] int32
 * Per chain k, everything in float64 and in ascending finger order:
 *   1. v_b = beta_per_cell * mean_j values[j * n_chains + k][b]      (the sum in j order, then one division, as the gradients' mean)
 *   2. v_b not finite: logw_b = -inf.  Otherwise logw_b += v_b - vprev_b, then vprev_b = v_b.
 *   3. m = max_b logw_b.  m == -inf (every value non-finite): ancestors = identity, ess = 0, did = 0, logw = 0; done.
 *   4. w_b = exp(logw_b - m); s = sum w; w /= s; ess = 1 / sum w^2.
 *   5. ess < ess_frac * B: resample.  u = the uniform below; cum_b = the running sum of w; p_j = (u + j) / B;
 *      a_j = min(#{b : cum_b <= p_j}, B - 1); x_out[k][j] = x[k][a_j] (bit copies); vprev[j] = vprev_old[a_j]; logw = 0; did = 1.
 *   6. otherwise x_out = x, ancestors = identity, did = 0; logw is kept.
 * The uniform: raw output 0 of numpy.random.Philox(key=[seed, chain_keys[k]], counter=[0, step_index, 1, 0]), u = (r >> 11) * 2^-53
 * in [0, 1) - Philox4x64-10 block (1, step_index, 1, 0), lane 0.  The third counter word 1 keeps it clear of the step noise's blocks
 * (e / 2 + 1, step_index, 0, 0): u depends on (seed, key, step_index) only.
 * n_chains, B, L, n_grad >= 1, step_index >= 0, no NULL pointer, x_out_dev apart from x_dev: anything else is DGDM_EINVAL before a
 * launch.  One lane walks a chain's fingers (the order above is literal); the gather is a second, coalesced kernel over all entries.
 * Whatever the values hold, every ancestor lies in 0 .. B - 1.                                                                       */
int dgdm_chain_resample(const float *x_dev, const double *values_dev, int n_chains, int B, int L, int n_grad, double beta_per_cell,
                        double ess_frac, uint64_t seed, const uint64_t *chain_keys_dev, int64_t step_index, double *logw_dev, double *vprev_dev,
                        float *x_out_dev, int32_t *ancestors_dev, double *ess_dev, int32_t *did_dev, void *stream);
/* Debug / test entry: the uniform of the recipe above -> u_dev [n_chains] float64. */
int dgdm_resample_uniform(uint64_t seed, const uint64_t *chain_keys_dev, int n_chains, int64_t step_index, double *u_dev, void *stream);

/* The whole guided denoise loop in one call: Diffusion.guided_sample's loop body (generator/diffusion.py:570-576) for n_chains chains, or
 * guided_sample_multi_object's (:637-647) for n_chains chains that each average n_grad gradients - n_steps x [eps-net; cond_fn; guidance
 * combine; scheduler step] without returning to the host language in between.
 *   noise_dev    [B][L]             the start sample every chain begins from (:570)
 *   objectives   [n_grad * n_chains] host array, object-major: gradient j of chain k is entry j * n_chains + k (n_grad = 1: one per chain)
 *   rowcoef_dev  [n_grad * n_chains][R] or NULL
 *   starts_host  3-D: [n_steps][n_grad * n_chains][starts_per_call] int64 in the reference's draw order per gradient chain; 2-D: NULL
 *   timesteps    [n_steps] host; coef [n_steps][4] host = sqrt(abar_t), sqrt(1 - abar_t), sqrt(abar_prev), sqrt(1 - abar_prev) per step
 *   scales       [n_chains] host: the classifier scale of every chain (:549-560)
 *   x_out_dev    [n_chains][B][L]   the final samples
 * The first eps-net call is evaluated once for all chains (they all hold the start sample).  Equivalent, bit for bit, to calling
 * dgdm_unet1d_forward / dgdm_dyn{2,3}d_guidance_grad / dgdm_ddim_guided_step step by step.                                             */
int dgdm_guided_chains_run(DgdmUnet1d *unet, DgdmGuidance *g, const float *noise_dev, int n_chains, int n_grad,
                           const DgdmObjective *objectives, const float *rowcoef_dev, const int64_t *starts_host,
                           const int32_t *timesteps, const float *coef, const float *scales, int n_steps, float *x_out_dev, void *stream);
/* The same for a conditional eps-net (dgdm_guided_chains_run is this call with NULL, 0, 1).
 *   global_cond_dev    cond_chain_stride == 0: [B][gc], shared by all chains; == B * gc: [n_chains][B][gc]; anything else: DGDM_EINVAL
 *   cfg_weight         classifier-free guidance: eps = eps_u + w (eps_c - eps_u) (dgdm_cfg_mix), eps_u = the net on the all-zero condition
 *                      row.  w == 1 evaluates eps_c only (the plain conditional run), w == 0 eps_u only; otherwise both halves go through
 *                      ONE eps-net call of twice the samples.
 * The classifier-guidance term and the DDIM step follow as above.  With one shared condition block the first eps-net call is still
 * evaluated once for all chains; with per-chain conditions it covers all n_chains * B samples.  Equivalent, bit for bit, to calling
 * dgdm_unet1d_forward_cond / dgdm_cfg_mix / dgdm_dyn{2,3}d_guidance_grad / dgdm_ddim_guided_step step by step.                        */
int dgdm_guided_chains_run_cond(DgdmUnet1d *unet, DgdmGuidance *g, const float *noise_dev, int n_chains, int n_grad,
                                const DgdmObjective *objectives, const float *rowcoef_dev, const int64_t *starts_host,
                                const int32_t *timesteps, const float *coef, const float *scales, int n_steps, float *x_out_dev,
                                const float *global_cond_dev, int64_t cond_chain_stride, float cfg_weight, void *stream);
/* The same with every scheduler step bounded (dgdm_ddim_guided_step_bounded): lo_dev / hi_dev [B][L], one block shared by all chains
 * (period = B * L).  noise_dev is then the edit's start sample, add_noise(design, noise, timesteps[0]), and timesteps / coef the
 * schedule's last n_steps entries.  lo_dev == hi_dev == NULL is dgdm_guided_chains_run_cond; exactly one of them NULL: DGDM_EINVAL.
 * Equivalent, bit for bit, to the step-by-step composition above with dgdm_ddim_guided_step_bounded as its last call.               */
int dgdm_guided_chains_run_bounded(DgdmUnet1d *unet, DgdmGuidance *g, const float *noise_dev, int n_chains, int n_grad,
                                   const DgdmObjective *objectives, const float *rowcoef_dev, const int64_t *starts_host,
                                   const int32_t *timesteps, const float *coef, const float *scales, int n_steps, float *x_out_dev,
                                   const float *global_cond_dev, int64_t cond_chain_stride, float cfg_weight, const float *lo_dev,
                                   const float *hi_dev, void *stream);
/* The same with stochastic steps (dgdm_ddim_guided_step_noisy); the single body of the four entries.
 *   eta_coef    [n_steps][2] host = sigma, dir per step, or NULL: every step has sigma = 0, dir = coef[.][3] (dgdm_guided_chains_run_bounded)
 *   seed        the noise seed of the run
 *   chain_keys  [n_chains] host: chain k's step si draws the stream of key (seed, chain_keys[k]) at step_index si - the chain's global
 *               identity, so a run split over calls or ranks draws what the single call draws; NULL: 0 .. n_chains - 1
 * A step with sigma == 0 (the last one: abar_prev = 1) is the eta = 0 step.  Equivalent, bit for bit, to the step-by-step composition
 * with dgdm_ddim_guided_step_noisy as its last call.                                                                                 */
int dgdm_guided_chains_run_noisy(DgdmUnet1d *unet, DgdmGuidance *g, const float *noise_dev, int n_chains, int n_grad,
                                 const DgdmObjective *objectives, const float *rowcoef_dev, const int64_t *starts_host,
                                 const int32_t *timesteps, const float *coef, const float *scales, int n_steps, float *x_out_dev,
                                 const float *global_cond_dev, int64_t cond_chain_stride, float cfg_weight, const float *lo_dev,
                                 const float *hi_dev, const float *eta_coef, uint64_t seed, const uint64_t *chain_keys, void *stream);

/* Forward-only sweep of Diffusion.get_convergence_centers (diffusion.py:506-531): G orientations,
 * pos = 0, t = 0, rows r = g*B + b.  logits_dev [n_chains][B*G][3].  starts_host (3-D) holds
 * 2*B*G indices per chain in draw order with the sub_batch_size partition of :524-526.           */
int dgdm_guidance_orientation_sweep(DgdmGuidance *g, const float *x_dev, const int32_t *object_of_chain,
                                    const int64_t *starts_host, int n_chains, float *logits_dev, void *stream);

/* Predicted roll-outs: the dynamics model iterated on its own output, from the sweep's poses.  This stands where the reference's
 * simulator closes the gripper 40 times per start orientation (2-D: dynamics/sim_test_mj.py:161-185, 8000 steps with the gripper reset
 * every 200; 3-D: sim_test_mj_3d.py:154-176, 32000 steps, reset every 800) and reports the motion after the first closing and the
 * settled pose after the last; the roll-out itself is ours - the reference's are MuJoCo's.
 *   State per row (chain, finger b, start orientation g; r = g*B + b as the sweep): (ori, pos_x, pos_y) in float64, in the model's
 *   normalised inputs (ori = theta/pi - 1, pos = metres / 0.03; dynamics/dataloader.py:51-52).  Start: the sweep's poses,
 *   ori = linspace(ori_range)[g], pos = 0.  Interaction k = 0 .. K-1: the state rounded once to float32, the model evaluated at t = 0
 *   -> three float32 logits l; then, in double, each product and sum rounded on its own:
 *     ori += l0 * scale[0], brought back into [-1, 1] by multiples of 2 (values inside, +-1 included, are left alone);
 *     pos += l{1,2} * scale[{1,2}], NOT clamped: beyond |pos| = 1 the model extrapolates, and left[r] tells - the first k after which
 *     |pos_x| > 1 or |pos_y| > 1, -1 if never.
 *   A non-finite logit makes the row's state non-finite for good.  scale: the caller's std[0]/pi, std[1]/0.03, std[2]/0.03.
 *   starts_host  3-D: [K][n_chains][2*B*G] int64 - every interaction is a classifier call of its own, each with the sweep's layout and
 *                sub_batch_size partition, consecutive calls; 2-D: NULL
 *   final_dev [n][B*G][3] the state after interaction K-1; first_logits_dev [n][B*G][3] interaction 0's logits (= the sweep's poses
 *   through the f16x3 trunk); left_dev [n][B*G]; traj_pose_dev NULL or [K+1][n][B*G][3] (slot 0 = the start); traj_logits_dev NULL or
 *   [K][n][B*G][3].
 * All K interactions are enqueued on `stream`; nothing is copied to the host and the host does not wait between them.  Contraction
 * dtypes f32 / f32_f16x3 (forward-only f16x3 trunk with a pose per row); bf16 and f32_mfma: DGDM_EINVAL (neither trunk has that
 * form).  Bit-identical run to run; leaves what grad / score / orientation_sweep compute untouched.                                    */
int dgdm_guidance_rollout(DgdmGuidance *g, const float *x_dev, const int32_t *object_of_chain, const int64_t *starts_host,
                          const double scale[3], int n_interactions, int n_chains, double *final_dev, float *first_logits_dev,
                          int32_t *left_dev, double *traj_pose_dev, float *traj_logits_dev, void *stream);

/* Condition rows of the eps-net (global_cond) from the dynamics model: one pass that labels every finger of a set with what the model
 * predicts it does - the model's opinion, not a simulator's.  Two runners over the two calls above.
 * Batching (both).  fingers_dev [n_fingers][L] in sampler units, any n_fingers >= 1.  With B the handle's batch, batch k holds fingers
 *   k*B .. min((k+1)*B, N) - 1; the last batch is padded to B with copies of finger N - 1 (padding rows are computed and thrown away).
 *   Every batch is evaluated as n_objects chains that all hold the same [B][L] block (a small device copy replicates it), chain m facing
 *   object objects_host[m].  starts_host, 3-D: label [n_batches][n_objects][starts_per_call], settled [n_batches][K][n_objects][2*B*G] -
 *   each batch's slice exactly what dgdm_guidance_score / dgdm_guidance_rollout take, uploaded as they upload it; 2-D: NULL.  All batches
 *   are enqueued on `stream`; in 2-D the host does not wait between batches.  Scratch is the handle's; like score, the calls leave the
 *   results of dgdm_dyn{2,3}d_guidance_grad untouched.
 * Placement.  Row i starts at rows_dev + i*row_stride.  layout DGDM_LABEL_MEAN: the 10 (5) columns are written there.
 *   DGDM_LABEL_PER_OBJECT: object m's block starts m*object_stride floats further on (object_stride = 15 interleaves a tally and a
 *   settled block per object).  Floats of the row that belong to neither block are not written.
 * Tally columns (dgdm_guidance_label).  Row i holds, bit for bit, these functions of what dgdm_guidance_score returns for i's padded
 *   batch with the same thr, timestep, objects and start slice: per object m the histogram c_m[3][3][3] (bin = (class d0 * 3 + class d1)
 *   * 3 + class d2) and s_m[4]; n = G*P*P; M' = n_objects (MEAN) or 1 (PER_OBJECT).
 *     0 frac_clockwise (d0 class 0)   1 frac_counterclockwise (d0 class 2)   2 frac_up (d1 class 0)   3 frac_down (d1 class 2)
 *     4 frac_left (d2 class 0)        5 frac_right (d2 class 2)
 *       each float32(double(K) / double(M' * n)), K the marginal count summed in int64 over the block's objects;
 *     6 mean_rot   7 mean_abs_rot   8 mean_shift_x   9 mean_shift_y
 *       each float32((sum over m ascending of double(s_m[j])) / double(M' * n)), j = 0..3, in the model's normalised units.
 *   One IEEE division and one rounding per value.
 * Settled columns (dgdm_guidance_label_settled).  From what dgdm_guidance_rollout returns for the padded batch (final [M][B*G][3]
 *   float64 and left; finger b's rows are r = g*B + b), per object, everything in double with g ascending, no product fused into a sum:
 *     theta_g = M_PI * (ori_g + 1.0); c = (sum cos theta_g) / G; s = (sum sin theta_g) / G; rho = sqrt(c*c + s*s);
 *     p = (sum sqrt(px*px + py*py)) / G; fl = (count of left >= 0) / G
 *     0 settle_concentration = rho (1 when every start orientation settles at the same angle)   1 settle_cos = c   2 settle_sin = s
 *     3 settle_offset = p   4 left_range = fl
 *   MEAN: each per-object value summed over m ascending in double, divided by M', rounded once to float32.  A non-finite state of any
 *   of the block's rows makes columns 0-3 NaN.
 * DGDM_EINVAL before anything is launched: a NULL pointer or n_fingers < 1; n_objects outside 1..max_chains; an object index that is
 * not set; an unknown layout; row_stride / object_stride smaller than the columns they must hold; n_interactions < 1; a bf16 handle
 * (both calls); an f32_mfma handle for _settled (as rollout refuses it); 3-D without starts_host.                                     */
#define DGDM_LABEL_TALLY_COLS   10
#define DGDM_LABEL_SETTLED_COLS 5
enum { DGDM_LABEL_MEAN = 0, DGDM_LABEL_PER_OBJECT = 1 };
int dgdm_guidance_label(DgdmGuidance *g, const float *fingers_dev, int64_t n_fingers,
                        const int32_t *objects_host, int n_objects, int timestep, const float thr[3],
                        const int64_t *starts_host, int layout,
                        float *rows_dev, int64_t row_stride, int64_t object_stride, void *stream);
int dgdm_guidance_label_settled(DgdmGuidance *g, const float *fingers_dev, int64_t n_fingers,
                        const int32_t *objects_host, int n_objects, const double scale[3], int n_interactions,
                        const int64_t *starts_host, int layout,
                        float *rows_dev, int64_t row_stride, int64_t object_stride, void *stream);

/* Host helper for 'convergence': rowcoef_host[r] for one chain from its centers [B]
 * (deltas_to_objective :445-452 + slicer; `rows_in_call` is R for 2-D and the sub-batch
 * partition is applied for 3-D exactly as cond_fn :494-499 does).                               */
int dgdm_convergence_rowcoef(const int64_t *centers_host, int n_centers, int grid_size, int num_pos,
                             int64_t total_rows, int64_t sub_batch_size /* 0 = no sub-batching */, float *rowcoef_host);

/* Host-only test entry (no HIP call): the row plan of a 3-D gather launch, as the guidance handle makes it from the FPS start draws.
 *   in:  call k of chain c at starts_host + k * call_stride + c * 2 * rows, in the draw order of dgdm_dyn3d_guidance_grad's starts_host:
 *        per sub-batch of up to sub_batch_size rows, its sa1 draws (each in [0, num_object_points)), then its sa2 draws (in [0, 512))
 *   pairs_out [n_chains][n_calls * rows][2]: (s1, s2) per row; a chain's rows of all calls form one run, row k * rows + r
 *   need_order != 0: order_out [n_chains][n_calls * rows] - the chain's rows sorted by (s1, s2), rows with equal draws in row order,
 *        each as row | s2 << 22 - and group_off_out [n_chains][num_object_points + 1] - where the rows of each s1 start in that list
 *        ([num_object_points] = their number); need_order == 0: neither is touched (both may be NULL).
 * DGDM_EINVAL for a draw out of range, and with need_order for n_calls * rows >= 2^22 (the row id's bits below s2).                 */
int dgdm_debug_row_plan(const int64_t *starts_host, int n_chains, int64_t rows, int n_calls, int64_t call_stride, int64_t sub_batch_size,
                        int num_object_points, int need_order, int32_t *pairs_out, int32_t *order_out, int32_t *group_off_out);

/* ------------------------------------------------------------------ the path's random input: FPS start draws
 * farthest_point_sample draws its start index with torch.randint(0, N, (rows,)) on torch's CPU default generator
 * (dynamics/models/pointnet2_utils.py:83), twice per classifier call and sub-batch.  These host functions replay that generator
 * (at::mt19937; randint = output % range) on its own state blob - `state` is what torch.get_rng_state() / Generator.get_state()
 * returns (5056 bytes) - and advance the blob exactly as the torch calls would, so that the draws can be made (or skipped) from a
 * worker thread ahead of the launches and the blob handed back with torch.set_rng_state().                                    */
int dgdm_torch_rng_seed(uint8_t *state, int64_t state_bytes, uint64_t seed);             /* torch.Generator().manual_seed(seed)        */
int dgdm_torch_rng_randint(uint8_t *state, int64_t state_bytes, uint32_t high, int64_t n,
                           int64_t *out_host /* NULL: the n draws are skipped */);      /* torch.randint(0, high, (n,))               */
/* The draws of n_calls consecutive classifier calls over `rows` rows each (diffusion.py:495-498): per call and sub-batch of n rows,
 * sa1's n draws in [0, num_points) then sa2's n draws in [0, 512) - the starts_host layout of dgdm_dyn3d_guidance_grad.          */
int dgdm_torch_rng_fps_starts(uint8_t *state, int64_t state_bytes, int num_points, int64_t sub_batch_size, int64_t rows,
                              int64_t n_calls, int64_t *out_host /* NULL: skipped */,
                              int64_t out_call_stride /* elements between the outputs of consecutive calls; 0 = 2*rows */);

/* ------------------------------------------------------------------ (f) next: finger-geometry decode
 * What the reference does on the host, gripper by gripper, between the sampler and the simulator.  Both maps are linear in
 * the control values, so the library applies one constant matrix (built in double precision) to the whole batch on the device.
 *
 * 2-D  sim_test_batch (dynamics/sim_test_mj.py:257-262): y = 0.03 p - 0.015 over x = linspace(-0.12, 0.12, num_ctrl/2) for the
 *      left finger (first half of the control values) and the right one; generate_gripper / generate_finger_shape
 *      (assets/finger_sampler.py:7-12,39-51): scipy CubicSpline (not-a-knot) on linspace(x_0, x_last, num_points).
 *      samples_dev [batch][num_ctrl] -> curve_dev [batch][2 fingers][num_points][2] = (x, y) in metres.
 * 3-D  sim_test_batch_3d (dynamics/sim_test_mj_3d.py:236-237): y = 0.05 p - 0.05 on the 7 x 3 control net of
 *      generate_3d_ctrlpts (assets/finger_3d.py:77-81: x = linspace(-0.12, 0.12, 7), z = linspace(0, 0.12, 3), control point
 *      (i, j) = y[3 i + j]); generate_3d_finger_vertices (assets/finger_3d.py:60-68): geomdl BSpline.Surface of degree (3, 2),
 *      generate_knot_vector (clamped, uniform), sample_size x sample_size evaluation points in u-major order.
 *      samples_dev [batch][42] -> surface_dev [batch][2 fingers][sample_size^2][3] = (x, y, z) in metres.
 * The affine map from sampler units to metres is an argument (y = scale * p + offset): DGDM_DECODE_2D_* / DGDM_DECODE_3D_* are
 * the reference's constants; scale 1, offset 0 decodes control values that are already in metres.                              */
#define DGDM_DECODE_2D_SCALE 0.03f
#define DGDM_DECODE_2D_OFFSET (-0.015f)
#define DGDM_DECODE_3D_SCALE 0.05f
#define DGDM_DECODE_3D_OFFSET (-0.05f)
int dgdm_finger_decode_2d(const float *samples_dev, int batch, int num_ctrl, int num_points, float scale, float offset,
                          float *curve_dev, void *stream);
int dgdm_finger_decode_3d(const float *samples_dev, int batch, int num_ctrl, int sample_size, float scale, float offset,
                          float *surface_dev, void *stream);

/* ------------------------------------------------------------------ object point clouds from scanned meshes
 * sample_pts_from_mesh (dynamics/utils.py:14-18: open3d read_triangle_mesh + sample_points_uniformly), which the reference calls for
 * the test objects of guided sampling (generator/train.py:100-109) and once per object name in dynamics training
 * (dynamics/dataloader.py:57-63).  The sampling contract (DESIGN.md "Object clouds from meshes"), all in float64:
 *   a_t = 0.5 |(v1 - v0) x (v2 - v0)|, A = sum a_t (A <= 0: DGDM_EINVAL naming the mesh), cdf_t = running sum of a_t / A,
 *   n_t = round_half_away(cdf_t N); triangle t owns the output points n_{t-1} <= p < n_t (grouped by triangle in file order);
 *   point p: r1, r2 = the uniforms (u >> 11) * 2^-53 of raw outputs 2p, 2p + 1 of numpy.random.Philox(key=[seed, key]) (Philox4x64-10,
 *   block counter p / 2 + 1), a = 1 - sqrt r1, b = sqrt r1 (1 - r2), c = sqrt r1 r2, x = a v0 + b v1 + c v2.
 * A point depends on its mesh, its index, seed and key only - not on the other meshes of the batch or the launch geometry.        */
typedef struct DgdmMesh DgdmMesh;   /* vertex positions and triangles of one OBJ file (host memory) */
/* OBJ reader: `v x y z [...]` (trailing values ignored) and `f` with i, i/j, i//k, i/j/k tokens, negative = relative, faces of more than 3
 * corners fan-triangulated as (v0, vi, vi+1); every other statement ignored; CRLF accepted.  A bad index (0 or out of range), a face
 * with fewer than 3 vertices, an unparsable number or a file without faces: DGDM_EINVAL, dgdm_last_error() = "path:line: reason".
 * Thread-safe (no global state): several files may be read at once.                                                                  */
int     dgdm_mesh_read_obj(const char *path, DgdmMesh **out);
int64_t dgdm_mesh_num_vertices(const DgdmMesh *m);
int64_t dgdm_mesh_num_triangles(const DgdmMesh *m);
/* verts_host [num_vertices][3] float64, tris_host [num_triangles][3] int32 0-based, in file order */
int     dgdm_mesh_copy(const DgdmMesh *m, double *verts_host, int32_t *tris_host);
void    dgdm_mesh_destroy(DgdmMesh *m);
/* Bytes of device workspace dgdm_mesh_sample_points needs for this batch; negative: bad offsets. */
int64_t dgdm_mesh_sample_workspace_bytes(const int64_t *tri_offsets_host, int num_meshes);
/* A batch of meshes: verts_dev [V][3] float64 and tris_dev [T][3] int32 (indices local to their mesh) concatenated; mesh m is vertices
 * vert_offsets_host[m] .. [m+1] and triangles tri_offsets_host[m] .. [m+1] (both [num_meshes + 1], starting at 0); keys_host
 * [num_meshes] -> out_dev [num_meshes][num_points][3] float64.  Synchronises the stream once (after the per-mesh areas are known);
 * a mesh with no area or a vertex index outside its mesh fails the whole call with DGDM_EINVAL before anything is written to out_dev. */
int     dgdm_mesh_sample_points(const double *verts_dev, const int32_t *tris_dev, const int64_t *vert_offsets_host,
                                const int64_t *tri_offsets_host, int num_meshes, uint64_t seed, const uint64_t *keys_host,
                                int64_t num_points, double *out_dev, void *workspace_dev, int64_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------ finger meshes
 * The step after the decode: the reference builds a trimesh per finger on the host (assets/finger_sampler.py:7-36 generate_finger_shape,
 * assets/finger_3d.py:38-57 generate_3d_finger_mesh), exports fingerl.obj / fingerr.obj (save_gripper :52-64, save_3d_gripper :69-80) and runs
 * V-HACD on each file for the collision pieces (dynamics/sim_test_mj.py:57-103, sim_test_mj_3d.py:47-92).  Here the vertices, the per-mesh
 * statistics and the collision pieces are computed on the device for a whole batch; the topology is constant per (kind, n).
 *
 * Orientation rule, every table: triangles are 0-based and counter-clockwise seen from outside, so (v1 - v0) x (v2 - v0) points out of
 * the solid and the signed volume sum_t v0 . (v1 x v2) / 6 is positive.  A quad (a, b, c, d) is split as (a, b, c), (a, c, d).
 *
 * kind 2 (DGDM_FINGER_MESH_2D), n = num_points >= 2: 4 n vertices in four rings of n - the curve at z = 0, the curve + width in y at
 *   z = 0, the curve + width at z = height, the curve at z = height - and 2 (4 (n - 1) + 2) triangles from the reference's quads in its
 *   order (assets/finger_sampler.py:24-31), with i = 0 .. n - 2 inside a family:
 *     left (i, i+1, i+3n+1, i+3n), right (i+2n, i+2n+1, i+n+1, i+n), front (3n, 2n, n, 0), back (n-1, 2n-1, 3n-1, 4n-1),
 *     top (i+2n, i+3n, i+3n+1, i+2n+1), bottom (i+n, i+n+1, i+1, i).
 * kind 3 (DGDM_FINGER_MESH_3D), n = sample_size >= 2, N = n^2: 2 N vertices - the decoded sheet in u-major order (point (a, b) at a n + b),
 *   then the sheet + width in y - and 4 (n - 1)^2 + 8 (n - 1) triangles:
 *     sheet, cells (a, b) in a-major order, p00 = a n + b, p01 = p00 + 1, p10 = p00 + n, p11 = p10 + 1: (p00, p10, p11), (p00, p11, p01),
 *       normal toward -y;
 *     shifted sheet, same cell order: (N + p00, N + p11, N + p10), (N + p00, N + p01, N + p11);
 *     walls along the boundary loop c_0, c_1, ... (b = 0 .. n-2 at a = 0; a = 0 .. n-2 at b = n-1; b = n-1 .. 1 at a = n-1; a = n-1 .. 1 at
 *       b = 0), per edge (c, d = the next loop vertex): (c, d, d + N), (c, d + N, c + N).
 *   geomdl's own tessellation order is not reproduced (geomdl is not a dependency): this triangulation is the project's.
 * kind 12 / 13 (DGDM_FINGER_PIECE_2D / _3D), n not used: one collision piece, see dgdm_finger_pieces_2d / _3d.                          */
enum { DGDM_FINGER_MESH_2D = 2, DGDM_FINGER_MESH_3D = 3, DGDM_FINGER_PIECE_2D = 12, DGDM_FINGER_PIECE_3D = 13 };
/* Vertex and triangle counts of one mesh of this kind and resolution. */
int dgdm_finger_mesh_counts(int kind, int n, int64_t *verts, int64_t *tris);
/* tris_host [tris][3] int32.  Host code, built once per (kind, n) and kept. */
int dgdm_finger_mesh_faces(int kind, int n, int32_t *tris_host);
/* samples_dev as dgdm_finger_decode_2d / _3d take it -> verts_dev [batch][2 fingers][V][3] float32 in the vertex order above.  The base
 * ring / sheet is bit for bit what the decode writes (same tables, same fmaf order); y + width and z = 0 + height are single float32
 * additions.  Arguments are checked as the decode checks them, plus num_points / sample_size >= 2 and width, height > 0.              */
int dgdm_finger_mesh_vertices_2d(const float *samples_dev, int batch, int num_ctrl, int num_points, float scale, float offset,
                                 float width, float height, float *verts_dev, void *stream);
int dgdm_finger_mesh_vertices_3d(const float *samples_dev, int batch, int num_ctrl, int sample_size, float scale, float offset,
                                 float width, float *verts_dev, void *stream);
/* Per-mesh statistics of `meshes` meshes that share one triangle table: verts_dev [meshes][V][3] float32, tris_dev [T][3] int32 ->
 * stats_dev [meshes][4] float64 = signed volume (divergence theorem, sum_t v0 . (v1 x v2) / 6), surface area, smallest triangle area,
 * number of triangles whose area is below area_eps.  Everything is accumulated in float64 by one wave per mesh in a fixed order: the
 * result depends on the mesh alone.  A triangle index outside [0, V) makes all four values of that mesh NaN.
 * What trimesh's .volume / .area report, and what the exporter uses to refuse a degenerate finger.                                   */
int dgdm_finger_mesh_stats(const float *verts_dev, const int32_t *tris_dev, int64_t meshes, int V, int T, double area_eps,
                           double *stats_dev, void *stream);
/* Collision pieces, in place of the reference's external V-HACD call (TestVHACD -h 16 / -h 32: at most 16 hulls in 2-D, 32 in 3-D):
 * an exact convex decomposition of the same finger at a coarser resolution.  Knot j of p over n samples is the sample index
 * floor(j (n - 1) / p + 1/2), j = 0 .. p.
 * 2-D: verts_dev [batch][2][4 num_points][3] from dgdm_finger_mesh_vertices_2d -> out_dev [batch][2][pieces][8][3]: piece k is the sheared
 *   box between knots k and k + 1, its vertices rings 0..3 at knot k then rings 0..3 at knot k + 1, its 12 triangles kind 12.
 * 3-D: verts_dev [batch][2][2 sample_size^2][3] from dgdm_finger_mesh_vertices_3d -> out_dev [batch][2][2 pu pv][6][3]: knot cell (j, l) of
 *   the (pu + 1) x (pv + 1) knot grid, corners q00, q10 (next u knot), q11, q01, gives pieces 2 (j pv + l) and + 1: the triangles
 *   (q00, q10, q11) and (q00, q11, q01) swept by width in y, vertices the three sheet corners then the same corners of the shifted sheet,
 *   8 triangles kind 13.
 * Both kinds of piece are convex by construction.  pieces (pu, pv) must be 1 .. the number of segments (cells per direction) and a
 * finger has at most 1000 pieces (the files are numbered %03d): otherwise DGDM_EINVAL.
 * chord_err_dev [batch][2] float64: the largest |y| distance, in metres, between the full-resolution base ring / sheet vertices and the
 * coarse piece surface under them (linear between knots in 2-D; the two triangles of the knot cell in 3-D), exactly 0 when every
 * sample is a knot.  Reported, never thresholded.                                                                                   */
int dgdm_finger_pieces_2d(const float *verts_dev, int batch, int num_points, int pieces, float *out_dev, double *chord_err_dev, void *stream);
int dgdm_finger_pieces_3d(const float *verts_dev, int batch, int sample_size, int pu, int pv, float *out_dev, double *chord_err_dev,
                          void *stream);
/* OBJ writer (what trimesh's mesh.export(path) does for the reference): verts_host [V][3] float32 as `v` lines with %.9g, which names
 * every binary32 value uniquely, tris_host [T][3] int32 0-based as 1-based `f` lines.  dgdm_mesh_read_obj on the file returns the same
 * float32 values and triangles.  Host code, thread-safe.                                                                             */
int dgdm_mesh_write_obj(const char *path, const float *verts_host, int64_t V, const int32_t *tris_host, int64_t T);

/* ------------------------------------------------------------------ object contours from icon images
 * extract_contours (assets/icon_process.py: cv2.resize to 128 x 128, BGR2GRAY, threshold 240 inverted, findContours RETR_EXTERNAL +
 * CHAIN_APPROX_SIMPLE, the longest contour by arcLength, resample_contour, int32, rescale), which the reference applies to the
 * Icons-50 test ids (generator/train.py:111-124).  The contract, exact in integers and float64, is DESIGN.md "Object contours from
 * icon images".  An image's result depends on that image alone, whatever else is in the batch.  Three calls, on the caller's stream:
 *   dgdm_icon_trace           binarise + external contours: the winner's point count per image (synchronises once);
 *   dgdm_icon_fetch_contours  the winners' points into a buffer the caller sized from those counts (synchronises once);
 *   dgdm_contour_resample     resample_contour of each winner (or of any int32 contours: the reference's public resample_contour). */
/* Bytes of device workspace dgdm_icon_trace and dgdm_icon_fetch_contours need for num_images images; negative: bad count. */
int64_t dgdm_icon_workspace_bytes(int num_images);
/* images_dev [num_images][height][width][channels] uint8, channels 3 (BGR, channel 0 blue as cv2 reads it) or 4 (BGRA, alpha
 * ignored) -> num_points_host [num_images]: the point count of each image's longest external contour.  An image without a pixel of
 * grey level <= 240 after the resize has no contour: DGDM_EINVAL naming its index.                                                 */
int dgdm_icon_trace(const uint8_t *images_dev, int num_images, int height, int width, int channels, void *workspace_dev,
                    int64_t workspace_bytes, int64_t *num_points_host, void *stream);
/* After dgdm_icon_trace on the same workspace: image m's contour, as (x, y) int32 pixel pairs in cv2's order, into points_dev rows
 * offsets_host[m] .. [m+1] ([num_images + 1], starting at 0, the running sum of the counts).  resample_workspace_dev is
 * dgdm_contour_resample_workspace_bytes(offsets_host, num_images) bytes; it receives the offsets, and may be handed on to
 * dgdm_contour_resample with the same offsets.                                                                                    */
int dgdm_icon_fetch_contours(void *workspace_dev, int64_t workspace_bytes, int num_images, const int64_t *offsets_host,
                             int32_t *points_dev, void *resample_workspace_dev, int64_t resample_workspace_bytes, void *stream);
/* Bytes of device workspace dgdm_contour_resample needs for these contours; negative: bad offsets. */
int64_t dgdm_contour_resample_workspace_bytes(const int64_t *offsets_host, int num_contours);
/* resample_contour of each contour: points_dev [offsets_host[num_contours]][2] int32, contour m = rows offsets_host[m] .. [m+1]
 * (at least one point each) -> out_dev [num_contours][num_out][2], int32, or float64 c / 128 * 0.1 - 0.05 when rescale != 0.
 * Arc lengths: sqrt of the integer squared step in float64, summed in order (np.cumsum); u = np.linspace(0, L, num_out); np.interp;
 * truncation to int32.  Squares are taken in int64 (numpy squares int32 steps in int32: the same for steps below 46341).
 * Synchronises the stream once.                                                                                                    */
int dgdm_contour_resample(const int32_t *points_dev, const int64_t *offsets_host, int num_contours, int num_out, int rescale,
                          void *out_dev, void *workspace_dev, int64_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------ integer rings: triangulation and convex pieces
 * The step between an icon's contour and a simulator object: the reference extrudes the contour with `triangle`'s constrained Delaunay
 * faces as caps (assets/icon_process.py:62-92 generate_icon_mesh / save_icon_mesh) and decomposes the prism with an external V-HACD run
 * (sim/sim_2d.py:103-111 prepare_icon_object).  Neither is reproduced: this is the project's own contract, exact in integers, computed
 * by one wave per ring (csrc/polygon.hip).  DESIGN.md §4.5d; tests/polygon_oracle.py is the CPU statement.
 *
 * points_dev [batch][n][2] int32, 3 <= n <= 256, every coordinate in [0, 32767] - what dgdm_contour_resample writes without rescale;
 * anything else is DGDM_EINVAL before a ring is touched (the range is checked on the device: one stream synchronisation).  Every
 * predicate is a cross or dot product in int64.  A ring's result depends on that ring alone: the same bits alone, in any batch, at any
 * position.  Per ring:
 *   1. clean   a point equal to the point kept before it is dropped, then trailing points equal to the first.  count = M points remain,
 *              ring[k] = the original index of kept point k (-1 from k = M on).  Collinear points are kept.
 *   2. status  the first that applies: 1  M < 3;  2  the doubled signed area a2 = sum (x_i y_i+1 - x_i+1 y_i) is 0;  3  not simple - two
 *              non-adjacent closed edges share a point, or two adjacent edges fold back on each other (cross 0, dot < 0);  4  the ear
 *              rule below found no ear (no simple ring does this; reported instead of looping);  0 otherwise.  area2 carries its sign
 *              (0 for status 1).  A ring with status != 0 has no triangles and no pieces (-1 / count 0).
 *   3. triangulate  ear clipping in the working order, the kept points read so that a2 > 0 (backwards when a2 < 0).  A current vertex
 *              j with neighbours i, l is an ear when cross(p_i, p_j, p_l) > 0 and no other current vertex lies in the closed triangle
 *              (cross >= 0 on all three sides).  The ear whose tip has the smallest original index is clipped and (i, j, l) emitted, as
 *              original indices, until three vertices remain; they are emitted with the smallest original index as j.
 *              triangles [M - 2][3] in clip order (-1 beyond), all counter-clockwise in the working order; their doubled areas are
 *              positive and add up to |a2| exactly.
 *   4. convex pieces  Hertel-Mehlhorn on that triangulation: clip t < M - 3 created the diagonal (i, l); the diagonals are visited from
 *              the last created to the first, and one is removed when at both of its end points the two boundary edges that become
 *              neighbours turn left or go straight (cross >= 0).  The faces that remain are convex and tile the ring.
 *              piece_count; piece_offsets [n - 1] (piece q = piece_index[offsets[q] .. offsets[q + 1]), -1 beyond entry piece_count);
 *              piece_index [3 (n - 2)] original indices, counter-clockwise in the working order (-1 beyond).  Faces come in the order of
 *              their lowest half-edge (half-edge 3 t + k leaves vertex k of triangle t), each starting there.
 * dgdm_polygon_triangulate: steps 1-3.  dgdm_polygon_convex_pieces: steps 1-4 in the same launch; its count / ring / area2 / triangles
 * pointers may each be null.  Outputs: status_dev, count_dev, piece_count_dev [batch] int32; ring_dev [batch][n] int32; area2_dev [batch]
 * int64; triangles_dev [batch][n - 2][3] int32; piece_offsets_dev [batch][n - 1], piece_index_dev [batch][3 (n - 2)] int32.  All
 * fixed-stride: no workspace.                                                                                                       */
int dgdm_polygon_triangulate(const int32_t *points_dev, int batch, int n, int32_t *status_dev, int32_t *count_dev, int32_t *ring_dev,
                             int64_t *area2_dev, int32_t *triangles_dev, void *stream);
int dgdm_polygon_convex_pieces(const int32_t *points_dev, int batch, int n, int32_t *status_dev, int32_t *count_dev, int32_t *ring_dev,
                               int64_t *area2_dev, int32_t *triangles_dev, int32_t *piece_count_dev, int32_t *piece_offsets_dev,
                               int32_t *piece_index_dev, void *stream);

/* ------------------------------------------------------------------ mesh rendering
 * Where the reference evaluates a 3-D design with pictures (sim/render_mesh.py render_mesh / render_object_mesh through MuJoCo's OpenGL
 * renderer, dynamics/sim_test_mj_3d.py:99-106, 218-225) this library has a small batched z-buffer rasteriser (csrc/render.hip): one call
 * draws many views.  MuJoCo's renderer (lights, materials, shadows, the ground plane, anti-aliasing) is NOT reproduced and is unpinned;
 * this is the project's own contract, exact in integers and in unfused float32 operations.  DESIGN.md §4.5e; tests/render_oracle.py is
 * the CPU statement.
 *
 * Meshes: verts_dev [V][3] float32 and tris_dev [T][3] int32 (indices local to their mesh, 0-based) are n_meshes meshes concatenated;
 * mesh m = rows vert_offsets_host[m] .. [m + 1] and tri_offsets_host[m] .. [m + 1] (both int64, starting at 0).
 * Instances (host tables of n_inst rows): inst_view_host (0 .. n_views - 1), inst_mesh_host, inst_matrix_host [n_inst][16] float32
 * row-major, inst_id_host int32, inst_rgb_host [n_inst][3] base colour in [0, 1], inst_eye_host [n_inst][3] the eye in the instance's
 * model frame (the last two may be null without rgb_dev).  The matrix m maps model coordinates straight to pixel coordinates and depth
 * (viewport x projection x view x model); callers compose it in float64 and round once.
 *   projection  per (instance, vertex), float32, nothing fused:  c_r = ((m_r0 x + m_r1 y) + m_r2 z) + m_r3,  r = 0 .. 3;
 *               px = c_0 / c_3, py = c_1 / c_3, zs = c_2 / c_3, one IEEE division each;  X = (int32) rintf(px * 256), Y likewise:
 *               8 sub-pixel bits, ties to even.
 *   rejection   a vertex is bad when c_3 <= 0 or not finite, zs is not finite, or |rintf(px * 256)| or |rintf(py * 256)| is not below
 *               2^20 (a NaN anywhere ends here).  A triangle with a bad vertex is dropped whole and counted in rejected[view].  There is
 *               no near-plane clipping.
 *   coverage    int64.  A = (x1 - x0)(y2 - y0) - (y1 - y0)(x2 - x0) on the snapped vertices in file order; A == 0 draws nothing; A < 0
 *               swaps v1 and v2 (two-sided: OBJ winding is not trusted).  Pixel (i, j) samples at (256 i + 128, 256 j + 128) = (sx, sy).
 *               For the edges a -> b = v0 -> v1, v1 -> v2, v2 -> v0 with (dx, dy) = b - a:  E = dx (sy - ya) - dy (sx - xa).  The pixel
 *               is covered iff all three E >= 0, where E == 0 counts only when dy < 0, or dy == 0 and dx > 0.  Triangles that share an
 *               edge therefore cover each sample on it exactly once.
 *   depth       float32, nothing fused:  b1 = (float)E_20 / (float)A,  b2 = (float)E_01 / (float)A,
 *               z = (z0 + b1 (z1 - z0)) + b2 (z2 - z0)  with z_k the zs of (swapped) vertex k.  The smaller z wins; at equal z the
 *               earlier instance of the view (caller's order), then the lower triangle index.
 *   shading     rgb only, flat per triangle, float32, nothing fused, in model coordinates with the vertices a, b, c in file order:
 *               n = (b - a) x (c - a), each component p q - r s;  d = eye - ((a + b) + c) / 3;  dot = (n_x d_x + n_y d_y) + n_z d_z,
 *               |n|^2 and |d|^2 summed likewise;  q = sqrt(|n|^2 |d|^2);  s = 0.3 + 0.7 min(|dot| / q, 1), or 0.3 when q is 0 or not
 *               finite;  channel = (uint8) rintf((base s) 255), clamped to 0 .. 255.  (For a rigid model matrix this is the world-space
 *               |n . v| of the unit normal and the unit direction from the centroid to the eye.)
 * Outputs: ids_dev [n_views][height][width] int32, the id of the instance seen, -1 where nothing is drawn; depth_dev float32, +inf there;
 * rgb_dev (may be null) [n_views][height][width][3] uint8, white there; rejected_dev [n_views] int32.  snapped_dev (debug, may be null):
 * [instance vertices][4] int32 rows X, Y, the bits of zs, 1 = kept, instances in view order (the caller's order within a view).
 * A view's result depends on that view's instances alone, whatever else is in the batch.  1 <= width, height <= 2048, n_views <= 65535.
 * DGDM_EINVAL: bad offsets, a mesh or view index out of range, a size out of range, a triangle index outside its mesh (found on the
 * device; the images are then undefined).  Synchronises the stream once.                                                          */
/* Bytes of device workspace dgdm_render_meshes needs; negative: bad tables. */
int64_t dgdm_render_workspace_bytes(const int64_t *vert_offsets_host, const int64_t *tri_offsets_host, int n_meshes,
                                    const int32_t *inst_mesh_host, int n_inst, int n_views);
int dgdm_render_meshes(const float *verts_dev, const int32_t *tris_dev, const int64_t *vert_offsets_host, const int64_t *tri_offsets_host,
                       int n_meshes, const int32_t *inst_view_host, const int32_t *inst_mesh_host, const float *inst_matrix_host,
                       const int32_t *inst_id_host, const float *inst_rgb_host, const float *inst_eye_host, int n_inst, int n_views,
                       int width, int height, int32_t *ids_dev, float *depth_dev, uint8_t *rgb_dev, int32_t *rejected_dev,
                       int32_t *snapped_dev, void *workspace_dev, int64_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------ squeeze simulator (csrc/squeeze.hip)
 * A model-free 2-D closing simulator: a frictionless, quasi-static parallel-jaw squeeze of an object contour by two finger surfaces.  It
 * is this project's own idealisation, not the reference's MuJoCo scene (friction 1.0, soft position actuators: assets/finger_sampler.py:
 * 154-177), and is pinned by closed-form results of frictionless squeezing and by tests/squeeze_oracle.py, which the device reproduces
 * bit for bit.  All arithmetic is float64; every product, sum and quotient below is rounded on its own, in the order written; no
 * transcendental function is evaluated on the device.
 *
 * Inputs.  surfaces_dev [n_fingers][2][m]: the lower (L) and upper (U) jaw surface of each finger pair in the world frame at jaw
 *   travel 0, sampled at u_j = -hl + j h, h = 2 hl / (m - 1), hl = finger_half_len.  objects_dev [n_objects][nv][2]: closed polygons in
 *   metres about their own origin, either winding.  rot_dev [theta_cells][2] = (cos, sin) of theta_a = 2 pi a / theta_cells, made by the
 *   caller.  pairs_host [n_pairs][2] int32 = (finger, object), HOST memory.  starts_dev [n_starts][3] = (theta0, x0, y0), shared by all
 *   pairs.
 * Cell (a, b): the pose theta_a, x_b = -x_half + b dx, dx = 2 x_half / (x_cells - 1), the object at y = 0;
 *   P_i = (c vx_i - s vy_i + x_b, s vx_i + c vy_i).  Two candidate sets, for both jaws:
 *   A  the vertices with -hl <= P_ix <= hl:  t = (P_ix + hl) / h, j = min(floor t, m - 2), f = t - j, Lp = L_j + f (L_{j+1} - L_j), Up
 *      likewise; gaps P_iy - Lp and Up - P_iy;
 *   B  for every edge (P_i, P_{i+1}), cyclic, with xa != xb, the finger samples j0 = max(ceil((min(xa, xb) + hl) / h), 0) <= j <=
 *      j1 = min(floor((max(xa, xb) + hl) / h), m - 1):  ye = ya + (u_j - xa) ((yb - ya) / (xb - xa)); gaps ye - L_j and U_j - ye.
 *   touch_l = the least lower gap, touch_r = the least upper gap (+inf for an empty set): both functions are piecewise linear, so the
 *   two sets hold the exact minimum, and a minimum does not depend on the order it is taken in.  S = (touch_l + touch_r) / 2 is the
 *   common jaw travel at which both jaws touch.
 * Motion.  Two jaws under a constant closing force are a potential -2 F S; overdamped and frictionless, the object climbs S.  A jaw that
 *   touches alone carries the object along y without turning it (an assumption of this model, not a result).
 *   Successor of a cell: itself (a fixed point) if S >= travel_max - the jaws are fully closed and the object is loose; +inf included.
 *   Otherwise the candidates (da, db), |da|, |db| <= window, not both 0, a + da modulo theta_cells, b + db outside 0 .. x_cells - 1
 *   dropped, are visited in ascending (|db|, |da|, da, db); the best starts at the cell's own S and is replaced on strictly greater only
 *   (so a pure rotation wins a tie).  S rises strictly along a path: no cycles.
 *   One closing = the closing_steps-th successor (or the fixed point if reached first); settled = the fixed point.  Both by pointer
 *   doubling over ceil(log2(cells)) rounds on the device, no host wait in between.
 *   A start snaps to the nearest cell:  a = floor(theta0 / (2 pi / theta_cells) + 0.5) modulo theta_cells,
 *   b = floor((x0 + x_half) / dx + 0.5) clamped to 0 .. x_cells - 1 (halves round up; a non-finite start lands on cell 0).
 *   y at a reached cell: (touch_r - touch_l) / 2 if S < travel_max, else y0 clamped to [travel_max - touch_l, touch_r - travel_max].
 *   Flags per start: 1 = loose at the start cell; 2 = the path ended on a cell with S >= travel_max; 4 = settled on b = 0 or
 *   b = x_cells - 1, where the table's x range cut the path.
 * Known limit: a ridge of S oblique to the grid can stall the climb early; `window` widens the directions it can take - a mitigation,
 *   not a cure.  window and closing_steps are untuned.
 * Outputs, device memory: cells_dev [n_pairs][n_starts][3] int32 = the start, closed and settled cell (a x_cells + b);
 *   y_dev [n_pairs][n_starts][2] = y at the closed and the settled cell; flags_dev [n_pairs][n_starts] int32 (n_starts = 0: all
 *   may be null).  Optional (null = not wanted): table_s_dev, touch_l_dev, touch_r_dev [n_pairs][theta_cells][x_cells] float64 and
 *   succ_dev [n_pairs][theta_cells x_cells] int32.
 * Pairs are processed in chunks of as many as workspace_bytes holds (dgdm_squeeze_workspace_bytes(cfg, chunk_pairs); at least one).
 * Every argument is validated before any launch: DGDM_EINVAL for theta_cells < 1, x_cells < 2, more than 2^30 cells, window outside
 * 1 .. 64, closing_steps < 0, non-finite or non-positive x_half / finger_half_len, a non-finite travel_max, m outside 2 .. 1024, nv
 * outside 3 .. 1024, a pair index out of range, a null required pointer, a workspace too small for one pair.  Synchronises the stream
 * once, at the end (the pair list is the caller's).                                                                                   */
typedef struct DgdmSqueezeConfig {
    int32_t theta_cells;        /* 720 */
    int32_t x_cells;            /* 241 */
    int32_t window;             /* R: 2 */
    int32_t closing_steps;      /* k: 6 */
    double  x_half;             /* 0.06 */
    double  travel_max;         /* 0.1 */
    double  finger_half_len;    /* hl: 0.12 */
} DgdmSqueezeConfig;
/* Bytes of device workspace for chunks of chunk_pairs pairs; negative: bad config. */
int64_t dgdm_squeeze_workspace_bytes(const DgdmSqueezeConfig *cfg, int chunk_pairs);
int dgdm_squeeze_map(const DgdmSqueezeConfig *cfg, const double *surfaces_dev, int n_fingers, int num_points, const double *objects_dev,
                     int n_objects, int num_vertices, const int32_t *pairs_host, int n_pairs, const double *rot_dev,
                     const double *starts_dev, int n_starts, int32_t *cells_dev, double *y_dev, int32_t *flags_dev, double *table_s_dev,
                     double *touch_l_dev, double *touch_r_dev, int32_t *succ_dev, void *workspace_dev, int64_t workspace_bytes,
                     void *stream);

/* ------------------------------------------------------------------ squeeze simulator with Coulomb friction (csrc/squeeze.hip,
 * DESIGN.md §4.1d "friction")
 * dgdm_squeeze_map with a friction coefficient mu between the jaws and the object, as an antipodal jamming rule.  It is this project's
 * own model, stated exactly here, pinned to nothing in MuJoCo and claiming nothing about it; tests/squeeze_friction_oracle.py restates
 * it in numpy float64 and the device reproduces that bit for bit.  2-D only.
 * The model.  Friction decides WHETHER the object moves, not WHERE.  A cell in which both jaws touch and whose two contacts can hold the
 *   object against any squeezing force - the line through the two contact points lies inside both friction cones (the two-contact
 *   antipodal condition) - is JAMMED, and a jammed cell is a fixed point.  Every other cell moves by the frictionless rule above, the
 *   climb of S: that a part which slides, slides where it would without friction is an ASSUMPTION of this model, not a result.  No
 *   friction with the support plane, no jaw compliance.
 * Contacts.  The candidates of a cell are visited for i = 0 .. nv - 1 in this order: the set-A candidate of vertex i, if
 *   -hl <= P_ix <= hl; then the set-B candidates of the edge (P_i, P_{i+1}), j ascending from j0 to j1.  The lower and the upper contact
 *   are tracked independently: each starts as "none" with the running least gap +inf and is replaced by a candidate whose gap is
 *   strictly less than the running least gap of its side before that candidate - so each is the first candidate to attain the least
 *   gap, and a NaN gap replaces nothing.  touch_l, touch_r and S are dgdm_squeeze_map's, bit for bit.
 *   A contact is a point c on the object (in the cell's pose, the object at y = 0) and an unnormalised normal n from the jaw into the
 *   object.  With (px, py) = P_i, (qx, qy) = P_{i+1}, e = (qx - px, qy - py), ye as above (its slope is e_y / e_x) and j of set A as
 *   above:
 *     lower, set A:  c = (P_ix, P_iy)   n = (-(L_{j+1} - L_j), h)
 *     lower, set B:  c = (u_j, ye)      n = (-e_y, e_x) if e_x > 0, else (e_y, -e_x)
 *     upper, set A:  c = (P_ix, P_iy)   n = (U_{j+1} - U_j, -h)
 *     upper, set B:  c = (u_j, ye)      n = (e_y, -e_x) if e_x > 0, else (-e_y, e_x)
 *   The code of a contact: i for set A, nv + i m + j for set B, -1 for none.
 * Jam test, float64, every product, sum and difference rounded on its own in the order written, no transcendental function and no
 *   normalisation (l: the lower contact, r: the upper):
 *     dx = c_rx - c_lx;   dy = c_ry - c_ly
 *     dot_l = n_lx dx + n_ly dy;       crs_l = n_lx dy - n_ly dx
 *     dot_u = -(n_rx dx + n_ry dy);    crs_u = n_rx dy - n_ry dx
 *     jam = both contacts exist && mu > 0 && S < travel_max && dot_l > 0 && dot_u > 0
 *           && fabs(crs_l) <= mu dot_l && fabs(crs_u) <= mu dot_u                      (any NaN: not jammed)
 *   mu = 0 jams nothing: the maps are dgdm_squeeze_map's bit for bit, jam is all 0, the contacts are still reported.
 * Motion.  A jammed cell is its own successor, exactly as a cell with S >= travel_max is.  Everything else - the successor order, the
 *   pointer doubling, the snap, y, closing_steps as "the k-th successor or the fixed point if reached first" - is dgdm_squeeze_map's.
 *   Flags: 1, 2 and 4 as there; 8 = the start cell is jammed; 16 = the settled cell is jammed.
 * Arguments: dgdm_squeeze_map's, then mu, then two optional outputs (null = not wanted), device memory: jam_dev
 *   [n_pairs][theta_cells][x_cells] int32 (0 / 1) and contact_dev [n_pairs][theta_cells][x_cells][2] int32 = the code of the lower and of
 *   the upper contact.  The jam table of a chunk lives in the workspace: dgdm_squeeze_friction_workspace_bytes(cfg, chunk_pairs) (negative:
 *   bad config) is this entry's size function; at least one pair must fit.
 * DGDM_EINVAL before any launch: a non-finite or negative mu, and everything dgdm_squeeze_map refuses.  Synchronises the stream once,
 * at the end.                                                                                                                          */
int64_t dgdm_squeeze_friction_workspace_bytes(const DgdmSqueezeConfig *cfg, int chunk_pairs);
int dgdm_squeeze_map_friction(const DgdmSqueezeConfig *cfg, const double *surfaces_dev, int n_fingers, int num_points,
                              const double *objects_dev, int n_objects, int num_vertices, const int32_t *pairs_host, int n_pairs,
                              const double *rot_dev, const double *starts_dev, int n_starts, int32_t *cells_dev, double *y_dev,
                              int32_t *flags_dev, double *table_s_dev, double *touch_l_dev, double *touch_r_dev, int32_t *succ_dev,
                              void *workspace_dev, int64_t workspace_bytes, void *stream, double mu, int32_t *jam_dev, int32_t *contact_dev);

/* ------------------------------------------------------------------ squeeze-simulator labels (csrc/squeeze.hip, DESIGN.md §4.1b
 * "source: squeeze")
 * Condition rows of the eps-net (global_cond) from the squeeze simulator: dgdm_guidance_label's and dgdm_guidance_label_settled's columns
 * made of the squeeze model's closings, with no dynamics model anywhere.  This project's own mechanism, 2-D only; frictionless unless
 * mu > 0; k, R, mu and the thresholds are untuned for squeeze deltas; nothing is claimed about MuJoCo.  tests/squeeze_label_oracle.py
 * restates the text below in numpy float64 and the device reproduces it (bit for bit, but for the two columns that pass through sqrt).
 * The per-start outputs of the map are never written: each chunk's tables are reduced to rows on the device.
 * Inputs.  cfg, surfaces_dev [n_fingers][2][m], objects_dev (the bank) [n_bank][nv][2], rot_dev: dgdm_squeeze_map's.  objects_host
 *   [n_objects] int32 indices into the bank, HOST.  The pairs are implied, finger-major: pair f * n_objects + k is (finger f, object
 *   objects_host[k]).  starts_dev [n_tally + n_settle][3] = (theta0, x0, y0): the first n_tally starts are tallied after one closing,
 *   the last n_settle are followed until they settle; n_settle = 0 writes the tally columns only.  mu = 0: dgdm_squeeze_map's tables;
 *   mu > 0: dgdm_squeeze_map_friction's (a jammed cell is its own successor) - the rows of mu = 0 are the frictionless rows bit for bit.
 * Everything below is float64, every product, sum and quotient rounded on its own, in the order written; no transcendental function is
 * evaluated on the device.  T = theta_cells, X = x_cells, dx = 2 x_half / (X - 1), tm = travel_max.
 * Tally start n < n_tally of a pair.  c0 = the snapped start cell, ck = the closed cell (the closing_steps-th successor), cf = the
 *   settled cell, y_closed = y at ck: all dgdm_squeeze_map's.  a = cell / X, b = cell % X;  da = a_k - a_0 as an integer,
 *   2 da > T: da -= T;  2 da < -T: da += T   (dgdm_squeeze_objective_values' fold);
 *     e0 = (double)da * (6.283185307179586 / T)        radians
 *     e1 = (double)(b_k - b_0) * dx                    metres
 *     e2 = y_closed - y0                               metres
 *   class of e_j: 2 if e_j > threshold[j], else 0 if e_j < -threshold[j], else 1 (a NaN: 1) - sim.squeeze.squeeze_metric's rule on raw
 *   radians and metres;  d0 = e0 / score_std[0], d1 = e1 / score_std[1], d2 = e2 / score_std[2].
 *   Per pair, one wave of 64 lanes: lane l takes n = l, l + 64, ... in ascending order, counting the six classes below in int32 and
 *   adding the four terms d0, fabs(d0), d1, d2 to four sums that start at 0.0; then v += shfl_xor(v, s) for s = 32, 16, .., 1 (the shape
 *   of dgdm_squeeze_objective_values).  This gives the pair's counts c[6] and sums s[4].
 * Settle start g < n_settle (start n_tally + g) of a pair, (a_s, b_s) = cf's:  (cos_g, sin_g) = rot_dev[a_s];
 *     x_s = -x_half + (double)b_s * dx;   px = x_s / pos_norm;   py = y_settled / pos_norm;   r_g = sqrt(px px + py py)
 *     out_g = b_s == 0 or b_s == X - 1 (flag 4) or fabs(px) > 1 or fabs(py) > 1
 *   Per pair the same wave shape over g gives sum cos, sum sin, sum r (from 0.0) and the count of out_g; with G = (double)n_settle:
 *     c = (sum cos) / G;  s = (sum sin) / G;  rho = sqrt(c c + s s);  offset = (sum r) / G;  left = (double)count / G
 *   A non-finite y_settled at any g makes rho, c, s and offset of that pair NaN.
 * Rows.  Row f starts at rows_dev + f row_stride + column_offset.  layout DGDM_LABEL_MEAN: one block there, over all n_objects pairs of
 *   the finger, M' = n_objects.  DGDM_LABEL_PER_OBJECT: object k's block starts k object_stride floats further on and holds pair k
 *   alone, M' = 1.  A block, its pairs k ascending, n' = (int64)M' n_tally:
 *     0 frac_clockwise (e0 class 0)   1 frac_counterclockwise (e0 class 2)   2 frac_up (e1 class 0)   3 frac_down (e1 class 2)
 *     4 frac_left (e2 class 0)        5 frac_right (e2 class 2)
 *       each float32((double)K / (double)n'), K the class count summed in int64 over the block's pairs;
 *     6 mean_rot   7 mean_abs_rot   8 mean_shift_x   9 mean_shift_y
 *       each float32((0.0 + s_k0[j] + s_k1[j] + ...) / (double)n'), j = 0 .. 3: the dynamics model's normalised units;
 *     10 settle_concentration   11 settle_cos   12 settle_sin   13 settle_offset   14 left_range     (n_settle > 0 only)
 *       each float32((0.0 + v_k0 + v_k1 + ...) / (double)M') of the pairs' rho, c, s, offset, left.
 *   Floats of the row that belong to no block are not written.
 * counts_dev [n_fingers][3] int32 or NULL: per finger the number of tally (pair, start)s with flag 1 (loose at the start cell), flag 2
 *   (ended loose) and flag 4 (settled on the edge of the x range).
 * Chunks hold whole fingers only: the workspace holds the tables of as many fingers' pairs as fit it and their partial sums
 *   (dgdm_squeeze_label_workspace_bytes(cfg, chunk_fingers, n_objects, friction != 0); negative: bad arguments); the chunking does not
 *   change a bit of the rows.
 * DGDM_EINVAL before any launch: everything dgdm_squeeze_map(_friction) refuses; n_objects < 1 or more than 65535; an object index
 *   outside the bank; n_tally < 1; n_settle < 0; n_objects n_tally or n_fingers n_objects beyond 2^31 - 1; a non-finite or non-positive
 *   score_std or pos_norm; a non-finite or negative threshold; an unknown layout; column_offset < 0; object_stride (PER_OBJECT) or
 *   row_stride smaller than the columns they must hold; a workspace too small for one finger.  Synchronises the stream once, at the end. */
int64_t dgdm_squeeze_label_workspace_bytes(const DgdmSqueezeConfig *cfg, int chunk_fingers, int n_objects, int friction);
int dgdm_squeeze_label(const DgdmSqueezeConfig *cfg, const double *surfaces_dev, int n_fingers, int num_points, const double *bank_dev,
                       int n_bank, int num_vertices, const int32_t *objects_host, int n_objects, const double *rot_dev,
                       const double *starts_dev, int n_tally, int n_settle, double mu, const double threshold[3],
                       const double score_std[3], double pos_norm, int layout, float *rows_dev, int64_t row_stride, int column_offset,
                       int object_stride, int32_t *counts_dev, void *workspace_dev, int64_t workspace_bytes, void *stream);

/* The objective's VALUE per (pair) from a squeeze map: what dgdm_guidance_objective_values makes of the dynamics model's logits, made
 * of the squeeze model's one-closing deltas instead - a second opinion for resampling.  This project's own mechanism:
 * no counterpart in the reference, frictionless; the 3-D fingers' form is dgdm_squeeze_values_3d, below.  THE recipe (tests/resample_squeeze_oracle.py states the same text in numpy).
 *   cells_dev  [n_pairs][n_starts][3] int32, y_dev [n_pairs][n_starts][2] float64: as dgdm_squeeze_map writes them
 *   starts_dev [n_starts][3] float64: the starts of that map (y0 is read)
 *   pair p belongs to group p / B and is finger p % B of it;  objectives_host [n_pairs / B], HOST
 *   rowcoef_dev [n_pairs / B][n_starts * B] float32 or NULL, read at [group][n * B + p % B] - the guidance row cell * B + b
 *   score_std[3]: the theta, x, y entries of the dataset's SCORE_STD (radians, metres, metres);  values_dev [n_pairs] float64
 * For pair p and start n, everything float64, every product, sum and quotient rounded on its own, in the order written:
 *   a = cell / x_cells, b = cell % x_cells of the start cell and of the closed cell;  da = a_closed - a_start as an integer,
 *   2 da > T: da -= T;  2 da < -T: da += T   (T = theta_cells; +-T / 2 is kept: the strict rule of continuous_signed_delta)
 *   d0 = ((double)da * (6.283185307179586 / T)) / std0
 *   d1 = ((double)(b_closed - b_start) * (2 x_half / (x_cells - 1))) / std1
 *   d2 = (y[p][n][0] - starts[n][2]) / std2
 *   t  = ((l0 d0 + q0 (d0 d0)) + (l1 d1 + q1 (d1 d1))) + (l2 d2 + q2 (d2 d2)),   lin / quad widened to double;
 *        use_rowcoef == 1: t = t + (double)rowcoef * d0
 * - the delta order (theta, x, y) and the units (each over its SCORE_STD entry) of the dynamics model's outputs and of the dataset
 * files sim_2d.py writes.  V[p] = sum_n t: one wave of 64 lanes per pair, lane l adds n = l, l + 64, ... in ascending order from 0.0,
 * then v += shfl_xor(v, s) for s = 32, 16, .., 1, lane 0 stores: bit-identical run to run.
 * DGDM_EINVAL before any launch: use_rowcoef == DGDM_OBJ_ROWFIELD (goal fields have no squeeze form) or any value other than 0 / 1,
 * use_rowcoef == 1 with a NULL rowcoef_dev, n_pairs % B != 0, n_pairs < 0, B < 1, n_starts < 1, a non-finite or non-positive
 * score_std, a bad cfg by dgdm_squeeze_map's rules, a NULL required pointer.  Synchronises the stream once, at the end (the
 * objectives are the caller's).                                                                                                      */
int dgdm_squeeze_objective_values(const DgdmSqueezeConfig *cfg, const int32_t *cells_dev, const double *y_dev, const double *starts_dev,
                                  int n_pairs, int n_starts, int B, const DgdmObjective *objectives_host, const float *rowcoef_dev,
                                  const double score_std[3], double *values_dev, void *stream);

/* ------------------------------------------------------------------ squeeze simulator, 3-D fingers: a sliced squeeze (csrc/squeeze.hip,
 * DESIGN.md §4.1d "3-D form")
 * The same model for the 3-D scene (assets/finger_3d.py:110-177, sim/sim_3d.py:127-158): the object stands on a plane, is turned about z
 * and placed in x; two jaws close along y; a jaw's face is a surface over (x, z).  Like the 2-D form it is this project's own
 * idealisation, pinned to nothing in MuJoCo and claiming nothing about it; tests/squeeze3d_oracle.py restates it in numpy float64 and the
 * device reproduces that bit for bit.  All arithmetic is float64; every product, sum and quotient below is rounded on its own, in the
 * order written; no transcendental function is evaluated on the device.
 *
 * Model.  Object and jaws are compared on the mv horizontal planes z = gz[j] only.  On each plane the 2-D contract applies unchanged:
 *   the object is the cross-section of its mesh there, an unordered soup of segments; the jaws are that level's two profiles,
 *   piecewise linear on the abscissae gx[0 .. mu - 1] (strictly ascending, NOT uniform).  A cell's touch_l / touch_r is the least gap
 *   over all levels.  Known limit: what lies between two levels (5 mm for a 25 x 25 finger grid over 0.12 m) is not seen - a ledge,
 *   rim or tip that falls between two planes does not touch, and the jaws' faces between their own sample rows do not either.  This
 *   is the model's stated resolution, not an error bound.  The object does not tilt, lift or slide in z.
 *
 * dgdm_squeeze_slice.  n_objects meshes, HOST memory: verts_host [sum nv][3] float64 in metres, tris_host [sum nt][3] int32 indexing
 *   their own mesh's vertices from 0, vert_offsets_host / tri_offsets_host [n_objects + 1] int64 (first 0, ascending); gz_host [mv]
 *   strictly ascending.  They are uploaded; the slicing runs on the device in three passes (count, scan, emit).
 *   1. vertex i is UP at level j iff V_iz >= gz_j;  2. triangle t crosses level j iff its vertices are neither all up nor all down;
 *   3. a crossing triangle has exactly two edges whose ends differ.  For such an edge, D = its down end and W = its up end, whichever
 *      way the triangle lists them (so the two triangles that share an edge make identical bits):
 *        r = (gz_j - D_z) / (W_z - D_z),  point = (D_x + r (W_x - D_x), D_y + r (W_y - D_y));
 *   4. the segment is (first point, second point) in the triangle's edge order (v0 v1, v1 v2, v2 v0);
 *   5. segments_dev [n][4] = (A_x, A_y, B_x, B_y), listed by (object, level, triangle index ascending);  seg_offsets_host
 *      [n_objects][mv + 1] int32, HOST: level j of object o is segments seg_offsets[o][j] .. seg_offsets[o][j + 1] - 1 of the one
 *      list, seg_offsets[o][mv] = seg_offsets[o + 1][0];
 *   6. a vertex exactly on a level gives zero-length or touching segments.  They stay: set A handles them, set B skips P_x == Q_x.
 *   *n_segments_host receives the number of segments.  segments_dev == null with capacity 0 counts only (DGDM_OK).  A capacity smaller
 *   than the count returns DGDM_EINVAL after the count pass, with the count needed in *n_segments_host and nothing emitted.
 *   Validated before any launch (DGDM_EINVAL): null pointers, n_objects outside 1 .. 65535, mv outside 1 .. 1024, gz not strictly ascending or
 *   non-finite, offsets not starting at 0 or descending, a mesh with no vertex, a non-finite vertex, a triangle index outside its
 *   mesh, more than 2^31 - 1 vertices or triangles in all.  Synchronises the stream.
 *
 * dgdm_squeeze_map_3d.  surfaces_dev [n_fingers][2][mv][mu]: the lower (L) and upper (U) jaw face in the world frame at jaw travel 0,
 *   L_j[i] at (gx_i, gz_j).  gx_host [mu], HOST.  segments_dev / seg_offsets_host as dgdm_squeeze_slice made them for the same gz
 *   (finite coordinates).  pairs_host [n_pairs][2] = (finger, object), HOST.  rot_dev, starts_dev and cfg as dgdm_squeeze_map;
 *   cfg->finger_half_len is checked as there and is otherwise UNUSED here (gx says where the samples are).
 *   Cell (a, b), level j, segment (A, B) of that level:  P = (c A_x - s A_y + x_b, s A_x + c A_y), Q likewise from B.
 *   A  for each of P and Q with gx_0 <= P_x <= gx_{mu-1}:  i = the greatest index with gx_i <= P_x, capped at mu - 2;
 *      f = (P_x - gx_i) / (gx_{i+1} - gx_i);  Lp = L_j[i] + f (L_j[i+1] - L_j[i]), Up likewise;  gaps P_y - Lp and Up - P_y.  Only
 *      comparisons choose i, so any search gives the same bits;
 *   B  if P_x != Q_x:  slope = (Q_y - P_y) / (Q_x - P_x);  for every i with min(P_x, Q_x) <= gx_i <= max(P_x, Q_x):
 *      ye = P_y + (gx_i - P_x) slope;  gaps ye - L_j[i] and U_j[i] - ye.
 *   touch_l / touch_r = the least lower / upper gap over levels and segments, +inf when there is none;  S = (touch_l + touch_r) / 2.
 *   Everything after S - successors, one closing, settled, snap, y, flags, the outputs and the chunking - is dgdm_squeeze_map's
 *   contract verbatim.
 *   Validated before any launch (DGDM_EINVAL): cfg as dgdm_squeeze_map, null required pointers, mu outside 2 .. 128, mv outside
 *   1 .. 512, mu mv > 1024 (the pair's 2 mv mu surface doubles stay in 16 KB of LDS), gx not strictly ascending or non-finite,
 *   seg_offsets not starting at 0, descending or passing n_segments, a pair index out of range, n_fingers / n_pairs < 1, n_objects outside 1 .. 2^20,
 *   a workspace too small for one pair (dgdm_squeeze_map_3d_workspace_bytes).  Synchronises the stream once, at the end.                */
int dgdm_squeeze_slice(const double *verts_host, const int64_t *vert_offsets_host, const int32_t *tris_host, const int64_t *tri_offsets_host,
                       int n_objects, const double *gz_host, int mv, double *segments_dev, int64_t capacity, int32_t *seg_offsets_host,
                       int64_t *n_segments_host, void *stream);
/* Bytes of device workspace for chunks of chunk_pairs pairs; negative: bad config or sizes. */
int64_t dgdm_squeeze_map_3d_workspace_bytes(const DgdmSqueezeConfig *cfg, int chunk_pairs, int mu, int mv, int n_objects);
int dgdm_squeeze_map_3d(const DgdmSqueezeConfig *cfg, const double *surfaces_dev, int n_fingers, const double *gx_host, int mu, int mv,
                        const double *segments_dev, int64_t n_segments, const int32_t *seg_offsets_host, int n_objects,
                        const int32_t *pairs_host, int n_pairs, const double *rot_dev, const double *starts_dev, int n_starts,
                        int32_t *cells_dev, double *y_dev, int32_t *flags_dev, double *table_s_dev, double *touch_l_dev,
                        double *touch_r_dev, int32_t *succ_dev, void *workspace_dev, int64_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------ squeeze simulator, 3-D fingers, with Coulomb friction
 * (csrc/squeeze.hip, DESIGN.md §4.1d "3-D friction")
 * dgdm_squeeze_map_3d with a friction coefficient between the jaws and the object, as a 3-D antipodal jamming rule on 3-D contact points
 * and 3-D normals: the jaw's surface normal including its z slope, and the mesh triangle's own normal.  It is a different rule from
 * dgdm_squeeze_map_friction's per-plane one, not a port of it, and like the rest of the squeeze family it is this project's own model,
 * stated exactly here, pinned to nothing in MuJoCo and claiming nothing about it; the coefficient is untuned.
 * tests/squeeze3d_friction_oracle.py restates it in numpy float64 and the device reproduces that bit for bit.
 * The model.  Friction decides WHETHER a cell moves, not WHERE.  touch_l, touch_r and S are dgdm_squeeze_map_3d's, bit for bit.  A cell
 *   whose two contacts can hold the object against any squeezing force - the line through the two contact points lies inside both
 *   friction cones - is JAMMED, and a jammed cell is its own successor.  ASSUMPTIONS of this model, not results: two point contacts; a
 *   free cell moves by the frictionless rule; the object still neither tilts, lifts nor slides in z, so a z component of the contact
 *   force can only jam or not jam; the jaw's z slope is a difference over neighbouring sample rows, so it is blind between planes, as the
 *   sliced squeeze is.  No friction with the support plane, no sliding rule under friction.
 * Contacts.  Per cell and jaw the contact is the first candidate to attain the least gap in this visiting order, replaced on strictly
 *   less only (a NaN gap replaces nothing): the object's segments in list order (level by level, as dgdm_squeeze_slice lists them), and
 *   per segment P (set A), Q (set A), then the set-B abscissae i ascending.  The code of a contact is the int32
 *       s (mu + 2) + k,    s = the segment's index within its object (its place in the list minus seg_offsets[o][0]),
 *                          k = 0 for P, 1 for Q, 2 + i for abscissa i;   -1 = none.
 *   The level j of segment s comes from the object's offsets.  The point c and the unnormalised normal n (from the jaw into the object)
 *   of a contact are rebuilt from its code by the operations of dgdm_squeeze_map_3d's cell text, in its order, so P, Q, i, f, slope and
 *   ye below are the candidate's own bits:
 *   point   set A: (P_x, P_y, gz[j]) (Q likewise);   set B: (gx[i], ye, gz[j]).
 *   normal  set A, the jaw's surface at (P_x, level j), i and f of set A:
 *             hx = gx[i+1] - gx[i];  j- = max(j - 1, 0), j+ = min(j + 1, mv - 1);  hz = gz[j+] - gz[j-];
 *             Lp- = L_{j-}[i] + f (L_{j-}[i+1] - L_{j-}[i]), Lp+ likewise on row j+, Up-, Up+ likewise;
 *             lower: n = (-(L_j[i+1] - L_j[i]) hz,  hx hz,  -(Lp+ - Lp-) hx)
 *             upper: n = ( (U_j[i+1] - U_j[i]) hz, -(hx hz),  (Up+ - Up-) hx)
 *             mv = 1: hz = 1 and n_z = 0.  With the z terms zero this is the 2-D rule's (-d, h) and (d, -h).
 *           set B, the object's face: N = the crossing triangle's normal in the object frame (dgdm_squeeze_slice_normals, below);
 *             r = (c N_x - s N_y,  s N_x + c N_y,  N_z) with the cell's (c, s);  n = -r (all three components) if the y component has the
 *             wrong sign - the lower jaw flips iff r_y < 0, the upper iff r_y > 0 - else n = r.  Mesh winding is therefore irrelevant; a
 *             degenerate triangle gives n = 0 and jams nothing.
 * Jam test, float64, every product, sum and difference rounded on its own in the order written (sums left to right), no normalisation,
 *   no sqrt, no transcendental function (l: the lower contact, u: the upper):
 *     d = c_u - c_l (three differences)
 *     per jaw:  a = n_x d_x + n_y d_y + n_z d_z;   w = (n_y d_z - n_z d_y,  n_z d_x - n_x d_z,  n_x d_y - n_y d_x);
 *               q = w_x w_x + w_y w_y + w_z w_z;      a_l = a of the lower jaw,  a_u = -(a of the upper jaw)
 *     jam = both contacts exist && friction > 0 && S < travel_max && a_l > 0 && a_u > 0
 *           && q_l <= (friction a_l)(friction a_l) && q_u <= (friction a_u)(friction a_u)          (any NaN: not jammed)
 *   friction = 0 jams nothing: every output is dgdm_squeeze_map_3d's bit for bit, jam is all 0, the contacts are still reported.
 * Motion.  A jammed cell is its own successor; everything after the jam table is dgdm_squeeze_map_friction's contract: flags 1, 2, 4 as
 *   dgdm_squeeze_map, 8 = the start cell is jammed, 16 = the settled cell is jammed.
 *
 * dgdm_squeeze_slice_normals.  dgdm_squeeze_slice, which also emits normals_dev [capacity][3], in the same segment order: for the
 *   crossing triangle (V0, V1, V2) of a segment, e = V1 - V0, g = V2 - V0 (three differences each),
 *     N = (e_y g_z - e_z g_y,  e_z g_x - e_x g_z,  e_x g_y - e_y g_x).
 *   The segments and offsets are dgdm_squeeze_slice's bit for bit.  normals_dev may be null only where segments_dev may (count only).
 *
 * dgdm_squeeze_map_3d_friction.  dgdm_squeeze_map_3d's arguments, then gz_host [mv] (HOST, the levels the meshes were sliced on),
 *   normals_dev [n_segments][3], friction, and two optional outputs (null = not wanted), device memory: jam_dev [n_pairs][T][X] int32
 *   (0 / 1) and contact_dev [n_pairs][T][X][2] int32 = the code of the lower and of the upper contact.  The jam table of a chunk lives in
 *   the workspace: dgdm_squeeze_map_3d_friction_workspace_bytes(cfg, chunk_pairs, mu, mv, n_objects) (negative: bad config or sizes) is
 *   this entry's size function; at least one pair must fit.
 *   DGDM_EINVAL before any launch: everything dgdm_squeeze_map_3d refuses; a null gz_host; gz not strictly ascending or non-finite; null
 *   normals_dev with n_segments > 0; a negative or non-finite friction; an object with so many segments that a code would pass
 *   2^31 - 1 (segments (mu + 2) > 2^31 - 1).  Synchronises the stream once, at the end.                                                 */
int dgdm_squeeze_slice_normals(const double *verts_host, const int64_t *vert_offsets_host, const int32_t *tris_host,
                               const int64_t *tri_offsets_host, int n_objects, const double *gz_host, int mv, double *segments_dev,
                               int64_t capacity, int32_t *seg_offsets_host, int64_t *n_segments_host, void *stream, double *normals_dev);
int64_t dgdm_squeeze_map_3d_friction_workspace_bytes(const DgdmSqueezeConfig *cfg, int chunk_pairs, int mu, int mv, int n_objects);
int dgdm_squeeze_map_3d_friction(const DgdmSqueezeConfig *cfg, const double *surfaces_dev, int n_fingers, const double *gx_host, int mu,
                                 int mv, const double *segments_dev, int64_t n_segments, const int32_t *seg_offsets_host, int n_objects,
                                 const int32_t *pairs_host, int n_pairs, const double *rot_dev, const double *starts_dev, int n_starts,
                                 int32_t *cells_dev, double *y_dev, int32_t *flags_dev, double *table_s_dev, double *touch_l_dev,
                                 double *touch_r_dev, int32_t *succ_dev, void *workspace_dev, int64_t workspace_bytes, void *stream,
                                 const double *gz_host, const double *normals_dev, double friction, int32_t *jam_dev, int32_t *contact_dev);

/* ------------------------------------------------------------------ squeeze-simulator labels, 3-D fingers (csrc/squeeze.hip, DESIGN.md
 * §4.1b "source: squeeze_3d")
 * dgdm_squeeze_label with dgdm_squeeze_map_3d's inputs: condition rows of 3-D fingers from the sliced squeeze.  The contract is those two
 * entries' and nothing else: the tables touch_l / touch_r / S of pair f * n_objects + k = (finger f, object objects_host[k]) are
 * dgdm_squeeze_map_3d's for that pair, bit for bit; everything from the tables to rows_dev and counts_dev - successors, closing, settling,
 * the tally and settle starts, the columns, the layouts, row_stride / column_offset / object_stride, the whole-finger chunks - is
 * dgdm_squeeze_label's text verbatim with these tables where the 2-D ones stood.  The composition of tests/squeeze3d_oracle.py and
 * tests/squeeze_label_oracle.py is the CPU oracle.  The same caveats hold: this project's own idealisation, blind between two levels,
 * frictionless (friction has no sliced form: there is no mu argument), k, R and the thresholds untuned, nothing claimed about MuJoCo.
 * What is new:
 *   seg_offsets_host [n_bank][mv + 1] describes the bank of sliced meshes; objects_host [n_objects] indexes that bank (repeats allowed).
 *   table_s_dev / touch_l_dev / touch_r_dev [n_fingers n_objects][T][X] float64 or NULL (not wanted): the tables of every pair, in pair
 *   order - they exist so that the tables can be compared with dgdm_squeeze_map_3d's, which rows of counts and means cannot be.
 *   The tables are made for a block of fingers at a time (what does not read the finger is evaluated once per block); every finger
 *   still sees its candidates in dgdm_squeeze_map_3d's order, so neither the blocks nor the chunks change a bit.
 *   Workspace: dgdm_squeeze_label_3d_workspace_bytes(cfg, chunk_fingers, n_objects, mu, mv, n_bank) (negative: bad arguments) holds gx
 *   and the level offsets, then chunk_fingers n_objects partial sums, then that chunk's tables.
 * DGDM_EINVAL before any launch: everything dgdm_squeeze_map_3d refuses (n_bank in n_objects' place there), and everything
 *   dgdm_squeeze_label refuses that concerns neither friction nor the 2-D sizes.  Synchronises the stream once, at the end.             */
int64_t dgdm_squeeze_label_3d_workspace_bytes(const DgdmSqueezeConfig *cfg, int chunk_fingers, int n_objects, int mu, int mv, int n_bank);
int dgdm_squeeze_label_3d(const DgdmSqueezeConfig *cfg, const double *surfaces_dev, int n_fingers, const double *gx_host, int mu, int mv,
                          const double *segments_dev, int64_t n_segments, const int32_t *seg_offsets_host, int n_bank,
                          const int32_t *objects_host, int n_objects, const double *rot_dev, const double *starts_dev, int n_tally,
                          int n_settle, const double threshold[3], const double score_std[3], double pos_norm, int layout, float *rows_dev,
                          int64_t row_stride, int column_offset, int object_stride, int32_t *counts_dev, double *table_s_dev,
                          double *touch_l_dev, double *touch_r_dev, void *workspace_dev, int64_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------ squeeze objective of 3-D fingers (csrc/squeeze.hip, DESIGN.md §4.3e
 * "potential: squeeze_3d")
 * The objective's VALUE per (finger of a chain, the chain's object) from the sliced squeeze: the potential of a resampling step for 3-D
 * fingers.  The contract is two existing entries' and nothing else: values_dev[g * batch + b] is, bit for bit, what
 *   dgdm_squeeze_map_3d on the pairs (group_first_host[g] + b, objectives_host[g].object), listed group-major, with the same starts, then
 *   dgdm_squeeze_objective_values on its cells / y with B = batch and the same objectives, rowcoef and score_std
 * give; the composition of tests/squeeze3d_oracle.py and tests/resample_squeeze_oracle.py is the CPU oracle.  No per-start output is
 * stored: a chunk's tables are reduced where dgdm_squeeze_map_3d would write cells and y.  The same caveats hold: this project's own
 * idealisation, blind between two levels of the finger grid, frictionless, k, R and the table size untuned, nothing claimed about
 * MuJoCo or about real checkpoints.
 *   cfg, surfaces_dev [n_fingers][2][mv][mu], gx_host, segments_dev / seg_offsets_host [n_bank][mv + 1], rot_dev, starts_dev
 *   [n_starts][3]: dgdm_squeeze_map_3d's.  Group g is the `batch` consecutive fingers group_first_host[g] .. + batch - 1 against the
 *   object objectives_host[g].object of the bank; two groups may name the same fingers (one chain weighed on several objects).
 *   objectives_host [n_groups], rowcoef_dev [n_groups][n_starts * batch] float32 or NULL, score_std[3]: dgdm_squeeze_objective_values'.
 *   values_dev [n_groups * batch] float64.  table_s_dev / touch_l_dev / touch_r_dev [n_groups * batch][T][X] float64 or NULL (not
 *   wanted): the tables of every pair in pair order, dgdm_squeeze_map_3d's bit for bit - they exist so that tests can compare them.
 *   The tables are made for blocks of 8 fingers of a group at a time, as dgdm_squeeze_label_3d makes them (what does not read the
 *   finger is evaluated once per block; every finger still sees its candidates in dgdm_squeeze_map_3d's order).  Chunks are whole
 *   groups; neither the blocks nor the chunks change a bit.  Workspace: dgdm_squeeze_values_3d_workspace_bytes(cfg, chunk_groups,
 *   batch, mu, mv, n_bank) (negative: bad arguments) holds gx and the level offsets, chunk_groups objectives, then that chunk's tables.
 * DGDM_EINVAL before any launch: everything dgdm_squeeze_map_3d refuses (n_bank in n_objects' place); everything
 *   dgdm_squeeze_objective_values refuses (a row-field objective, use_rowcoef == 1 without rowcoef_dev, a bad score_std, n_starts < 1);
 *   batch < 1, n_groups < 1, a group or a chunk of more than 65535 pairs; a group that reaches past n_fingers; an object outside the
 *   bank; a workspace too small for one group.  Synchronises the stream once, at the end (the host arrays are the caller's).           */
int64_t dgdm_squeeze_values_3d_workspace_bytes(const DgdmSqueezeConfig *cfg, int chunk_groups, int batch, int mu, int mv, int n_bank);
int dgdm_squeeze_values_3d(const DgdmSqueezeConfig *cfg, const double *surfaces_dev, int n_fingers, const double *gx_host, int mu, int mv,
                           const double *segments_dev, int64_t n_segments, const int32_t *seg_offsets_host, int n_bank, const double *rot_dev,
                           const double *starts_dev, int n_starts, int n_groups, int batch, const int32_t *group_first_host,
                           const DgdmObjective *objectives_host, const float *rowcoef_dev, const double score_std[3], double *values_dev,
                           double *table_s_dev, double *touch_l_dev, double *touch_r_dev, void *workspace_dev, int64_t workspace_bytes,
                           void *stream);

/* ------------------------------------------------------------------ measurement hooks
 * When enabled, the launches of every stage of the path are bracketed by hipEvents on the stream they are launched on.
 * dgdm_prof_read_stage synchronises those events and returns, for one stage, the number of bracketed regions, their total
 * milliseconds and the algorithmic work they covered (FLOPs for the MFMA-bound stages, 0 where the host cannot know it).
 * dgdm_prof_read = dgdm_prof_read_stage(DGDM_STAGE_TRUNK): the dominant kernel (DESIGN_HISTORY.md §5).                               */
enum {
    DGDM_STAGE_TRUNK = 0,   /* trunk_kernel / trunk_bf16_kernel: fused dynamics trunk forward + backward (work = FLOPs, real rows only) */
    DGDM_STAGE_UNET,        /* unet_kernel: one eps-net forward (work = useful FLOPs)                                          */
    DGDM_STAGE_XOBJ,        /* 3-D: FPS-start upload + per-row PointNet++ embedding gather (xobj kernels)                      */
    DGDM_STAGE_TABLES,      /* dgdm_guidance_set_objects: per-object PointNet++ tables (3-D) / object encoder (2-D)            */
    DGDM_STAGE_GUIDE_MISC,  /* small kernels of cond_fn around the trunk: encoders, first-layer tables, partial-sum fold       */
    DGDM_STAGE_DDIM,        /* guidance combine + scheduler step                                                               */
    DGDM_STAGE_COUNT
};
int dgdm_prof_enable(int on);
/* Test hook (3-D): where a reference row's PointNet++ embedding comes from (DESIGN_HISTORY.md §4.3) - mode 0: default: one workgroup per
 * (chain, s1) group with the variant's crowded-centre rows staged in LDS, until the objects of the last dgdm_guidance_set_objects have
 * served more than 5 guidance calls; from then on the per-object embedding table X[s1][start point] (built at that moment) and no gather
 * kernel at all; 5: the NEXT set_objects builds the embedding tables right away; 3: always the group kernel; 2: the per-row table kernel;
 * 1: every row runs its own FPS(128) instead of reading the per-object table of order-independent sequences; 4: like 0, and the NEXT
 * set_objects builds the crowded centres' sa2 features with per-(variant, centre) global gathers instead of the LDS-staged kernel.
 * Results must be identical.  Also reports, per object of the bank, whether the table of FPS(128) sequences is admissible
 * (out_fast_ok[n_objects], may be NULL).                                                                                                */
int dgdm_guidance_debug_fps_path(DgdmGuidance *g, int mode, int32_t *out_fast_ok);
/* Test hook: the per-tile partial sums of d objective / d z1 (z1 = the first trunk layer's pre-activation, BatchNorm folded) that the
 * last dgdm_dyn{2,3}d_guidance_grad call produced: out_dev [n_chains * B * tiles_per_finger][width], tile index
 * (chain * B + b) * tiles_per_finger + t = cells 32 t .. 32 t + 31 of finger b.  A ReLU whose float32 pre-activation has the other sign
 * than in exact arithmetic changes exactly one tile, which is what tests/test_gpu_fullgrid.py looks at.  out_dev may be NULL (sizes only). */
int dgdm_guidance_debug_partials(DgdmGuidance *g, int n_chains, float *out_dev, int32_t *tiles_per_finger, int32_t *width, void *stream);
/* Test hook: layer 1's pose term as the last dgdm_guidance_rollout call left it - its LAST interaction's rows (a call with one
 * interaction shows the start poses') - in the trunk's operand tiles: rollout_tiles_dev [n_chains * B * tiles_per_finger][width * 32],
 * tile (chain * B + b) * tiles_per_finger + t = orientations 32 t .. 32 t + 31 of finger b; and the orientation sweep's own table in the
 * same layout, sweep_tiles_dev [tiles_per_finger][width * 32].  At the start poses every tile (chain, b, t) must equal the sweep's tile
 * t bit for bit, padding rows included.  Either pointer may be NULL (sizes only).                                                      */
int dgdm_guidance_debug_rollout_table(DgdmGuidance *g, int n_chains, float *rollout_tiles_dev, float *sweep_tiles_dev,
                                      int32_t *tiles_per_finger, int32_t *width, void *stream);
int dgdm_prof_read(int64_t *launches, double *total_ms, double *total_flops);
int dgdm_prof_read_stage(int stage, int64_t *launches, double *total_ms, double *total_work);
/* Unit-test hook for the register-resident MFMA chain (csrc/mfma_chain.h): one 32-row tile through one 256 -> 256 layer,
 * Y = X W^T + bias.  W_host [256][256] row-major, bias_host [256] (host memory); X_dev, Y_dev [32][256] (device).  Synchronises. */
int dgdm_debug_chain_layer(const float *W_host, const float *bias_host, const float *X_dev, float *Y_dev, void *stream);

/* Test hook for the index work of PointNet++ on ONE cloud xyz_dev [N][3] (128 <= N <= 1024), through the same device code as the
 * production kernels; every output is int32 device memory; synchronises.
 *   fps512_dev [N][512], fps128_dev [N][128]: farthest_point_sample (dynamics/models/pointnet2_utils.py:71-92) from every start index
 *                                             (row v = the sequence torch.randint's draw v would give);
 *   fps128_flags_dev [N]: 1 = that 128-sequence met an exact distance tie between different coordinates (it is then order-dependent
 *                                             and the production path re-runs FPS per row instead of using the table);
 *   ball1_dev [N][32]: query_ball_point(0.2, 32, xyz, centre = point p) (pointnet2_utils.py:95-115), padded with the first index;
 *   ball2_dev [N][64] + ball2_count_dev [N]: query_ball_point(0.4, 64, ...) for centre point c when the candidates are scanned in the
 *                                             order perm_dev[0..perm_len) (sa2 sees the cloud re-ordered by sa1's FPS); entries past the
 *                                             count are -1 (the reference pads with the first);
 *   crowded_dev [N]: 1 = more than 64 points in that ball (DESIGN_HISTORY.md 4.3).                                                          */
int dgdm_debug_pointnet_indices(DgdmDynamics *m, const float *xyz_dev, int N, const int32_t *perm_dev, int perm_len,
                                int32_t *fps512_dev, int32_t *fps128_dev, int32_t *fps128_flags_dev, int32_t *ball1_dev,
                                int32_t *ball2_dev, int32_t *ball2_count_dev, int32_t *crowded_dev, void *stream);

/* ------------------------------------------------------------------ (f) rank 4: training the 2-D dynamics model
 * Trainer (dynamics/trainer.py:16-106) for ProfileForward2DModel: parameters, gradients and torch.optim.Adam state
 * (trainer.py:46: betas (0.9, 0.95), weight_decay) live on the device.  state_dict: the model's tensors ("module."-prefix
 * stripped), BatchNorm running statistics included.                                                                        */
typedef struct DgdmTrainer2d DgdmTrainer2d;
int dgdm_trainer2d_create(DgdmTrainer2d **out, const DgdmTensor *state_dict, int n_tensors, int params_ch, int object_ch,
                          float beta1, float beta2, float eps, float weight_decay);
void dgdm_trainer2d_destroy(DgdmTrainer2d *m);
/* Trainer.step (trainer.py:53-103, the branch without sub-batches) on `rows` rows when train != 0: noisy control points
 * sqrt_abar[r]*ctrl + sqrt_1m_abar[r]*noise (DDIMScheduler.add_noise, :75-79; noise_dev null = ctrl as given), model forward in
 * training mode (BatchNorm1d batch statistics; running statistics updated), loss = nn.MSELoss()(pred, score), backward, one Adam
 * update with learning rate lr.  train == 0 is Trainer.inference (:108-146): eval-mode forward (running statistics) and the loss,
 * nothing is updated.  t_dev [rows] = timesteps / num_train_timesteps (:80).  pred_dev [rows][3]; loss_host (optional) receives
 * the loss and makes the call synchronous, like loss.item().  Deterministic: same inputs, same bits.                              */
int dgdm_trainer2d_step(DgdmTrainer2d *m, const float *ctrl_dev, const float *noise_dev, const float *sqrt_abar_dev,
                        const float *sqrt_1m_abar_dev, const float *t_dev, const float *ori_dev, const float *pos_dev,
                        const float *object_dev, const float *score_dev, int64_t rows, float lr, int train, float *pred_dev,
                        float *loss_host, void *stream);
/* Optional hints for the NEXT dgdm_trainer2d_step / _forward_backward call only: which encoder inputs repeat over the rows.  The
 * result is the same function of the inputs (only the float32 summation order of the two encoders' gradients changes); the time and
 * object encoders then run on their distinct inputs instead of on every row (1.15 M rows -> 15 and 128 at the shipped configuration).
 *   t_index_dev [rows] + t_values_dev [n_t], n_t <= 32: row r's t is t_values[t_index[r]] (t_dev of the step call is then ignored);
 *   rows_per_object > 1: object_dev's rows come in runs of that many identical rows (dynamics/main.py:34 builds them so); rows must
 *                        be a multiple of it, otherwise the hint is ignored.                                                        */
typedef struct DgdmTrainGroups {
    const int32_t *t_index_dev;
    const float   *t_values_dev;
    int32_t        n_t;
    int32_t        rows_per_object;
} DgdmTrainGroups;
int dgdm_trainer2d_set_groups(DgdmTrainer2d *m, const DgdmTrainGroups *g);

/* Data-parallel training, one process per GPU (replaces nn.DataParallel around the model, dynamics/trainer.py:41-43, whose replicas
 * each normalise with the batch statistics of THEIR chunk and whose gradients add up on the source device):
 *   dgdm_trainer2d_forward_backward  this rank's `rows` of a batch of `total_rows`: forward in training mode on these rows' statistics,
 *                                    d loss / d pred = 2 (pred - score) / (3 total_rows), backward; no update.  *loss_host = this rank's
 *                                    share of the loss (the shares add up to the batch loss).
 *   dgdm_trainer2d_gradients         the flat gradient buffer (dgdm_trainer2d_gradient_count floats, layout private to the library:
 *                                    only elementwise reductions are meaningful) device -> flat_dev, or flat_dev -> device (to_trainer);
 *                                    between the two calls: all-reduce(sum) over RCCL.
 *   dgdm_trainer2d_apply             one Adam update from the gradient buffer.
 * dgdm_trainer2d_step == forward_backward(rows, rows) + apply.                                                                      */
int dgdm_trainer2d_forward_backward(DgdmTrainer2d *m, const float *ctrl_dev, const float *noise_dev, const float *sqrt_abar_dev,
                                    const float *sqrt_1m_abar_dev, const float *t_dev, const float *ori_dev, const float *pos_dev,
                                    const float *object_dev, const float *score_dev, int64_t rows, int64_t total_rows, float *pred_dev,
                                    float *loss_host, void *stream);
int64_t dgdm_trainer2d_gradient_count(const DgdmTrainer2d *m);
int dgdm_trainer2d_gradients(DgdmTrainer2d *m, float *flat_dev, int64_t numel, int to_trainer, void *stream);
int dgdm_trainer2d_apply(DgdmTrainer2d *m, float lr, void *stream);
/* BatchNorm running statistics, 8 x [mean | var] x 256 floats, device -> flat_dev or flat_dev -> device (to_trainer): every rank updates
 * them from its own chunk; nn.DataParallel keeps replica 0's, so rank 0's are broadcast to the others after each data-parallel step.   */
int dgdm_trainer2d_running_stats(DgdmTrainer2d *m, float *flat_dev, int64_t numel, int to_trainer, void *stream);
/* Copies into the host buffers of `tensors` (matched by name; data is written despite the const): which = 0 the state_dict
 * (parameters + running statistics: Trainer.save_checkpoint, trainer.py:105-106), 1 the gradients of the last step, 2 / 3 Adam's
 * exp_avg / exp_avg_sq.                                                                                                           */
int dgdm_trainer2d_export(DgdmTrainer2d *m, int which, DgdmTensor *tensors, int n_tensors);
int64_t dgdm_trainer2d_steps(const DgdmTrainer2d *m);      /* training steps taken = BatchNorm's num_batches_tracked increment */

/* ------------------------------------------------------------------ training from a device-resident dataset (csrc/dataset.hip)
 * The training set's samples as device arrays, read from their files once (dgdm_amd/dynamics/device_dataset.py), float32 as
 * DynamicsDataset.__getitem__ returns them:
 *   ctrl_dev   [n_samples][n_ctrl][2] (3-D: [..][3]); scores_dev [n_samples][cells][3]; ori_dev [n_samples][cells]; pos_dev [n_samples][cells][2]
 *   object_dev [n_objects][n_object_points][2] (3-D: [..][3]); object_of_sample_host [n_samples] (HOST memory): the object of each sample,
 *              NULL = sample s has object s (2-D: every file carries its own contour; 3-D: one cloud per object name).                */
typedef struct DgdmDynamicsStore {
    const float   *ctrl_dev, *object_dev, *scores_dev, *ori_dev, *pos_dev;
    const int32_t *object_of_sample_host;
    int64_t        n_samples, n_objects;
    int32_t        cells, n_ctrl, n_object_points, fingers_3d;
} DgdmDynamicsStore;
/* batch_rows of dynamics/main.py:21-35 on the device: the five row tensors of the batch made of samples sample_ids_host[0 .. nb) (any
 * order, repeats allowed), R = nb * cells rows, one launch, values copied bit for bit.
 *   2-D (main.py:33-35), row r = i * cells + c for batch slot i, cell c:
 *     ctrl_dev [R][n_ctrl] = the y ordinates ctrl[s_i][k][1]; obj_dev [R][2 n_object_points] = object[s_i] flattened
 *   3-D (main.py:29-32), cell-major as the reference concatenates them, row r = c * nb + i:
 *     ctrl_dev [R][3][n_ctrl], ctrl[r][d][k] = ctrl[s_i][k][d]; obj_dev [R][3][n_object_points] alike
 *   both: score_dev [R][3], ori_dev [R], pos_dev [R][2] sample-major, r = i * cells + c.
 * ids_dev: [2 nb] int64 of device workspace.  Every index (and the object it names) is checked against the store on the host before
 * anything is enqueued: DGDM_EINVAL.  Row widths need not be multiples of four.                                                        */
int dgdm_dynamics_batch_rows(const DgdmDynamicsStore *store, const int64_t *sample_ids_host, int nb, int64_t *ids_dev, float *ctrl_dev,
                             float *obj_dev, float *score_dev, float *ori_dev, float *pos_dev, void *stream);
/* class_accuracy of dynamics/main.py:37-42 as counts: agree_dev[j] (int64 [3], overwritten) = the rows r of score_dev, pred_dev [rows][3]
 * with (s > thr[j]) - (s < -thr[j]) == (p > thr[j]) - (p < -thr[j]), s = score[r][j], p = pred[r][j] - torch's comparisons, so a NaN is in
 * the middle class on both sides.  thr: host.  Exact integers, independent of the launch geometry.                                     */
int dgdm_class_agreement(const float *score_dev, const float *pred_dev, int64_t rows, const float thr[3], int64_t *agree_dev, void *stream);

/* ------------------------------------------------------------------ (f) rank 4: training the eps-net
 * Diffusion.get_stats / training_step (generator/diffusion.py:126-177) for the ConditionalUnet1D of generator/train.py:80
 * (generator/diffusion_utils.py:123-285; input_dim 1, down_dims [128, 256], kernel 5, 8 groups), torch.optim.Adam
 * (diffusion.py:711-714) and the EMA copy of diffusers' EMAModel (diffusion.py:716-724).  Parameters, gradients, both Adam moments and the
 * EMA copy live on the device in the state_dict's own tensor layouts (keys as ConditionalUnet1D.state_dict() gives them).
 * global_cond_dim is read from the state dict as in dgdm_unet1d_create.
 * Accepted domain (else DGDM_EINVAL; tests/test_gpu_unet_train.py): n_down 2 with down_dims {128, 256}, kernel_size 5, n_groups 8 (the
 * GroupNorm kernels are written for these); num_points even, 2 ... 512 (rows per sample num_points + 8 and num_points / 2 + 4, general
 * in num_points); diffusion_step_embed_dim a multiple of 4, 4 ... 64 (the GEMMs read aligned float4 windows of the [B][dsed] tensors;
 * K is rounded up to 16 inside the weight images, zero rows against whatever finite values the window runs into).                  */
typedef struct DgdmUnetTrainer DgdmUnetTrainer;
int dgdm_unet_trainer_create(DgdmUnetTrainer **out, const DgdmTensor *state_dict, int n_tensors, int num_points, const int32_t *down_dims,
                             int n_down, int diffusion_step_embed_dim, int kernel_size, int n_groups, float beta1, float beta2, float eps,
                             float weight_decay);
void dgdm_unet_trainer_destroy(DgdmUnetTrainer *m);
/* One training step on `samples` samples: noisy = sqrt_abar[s] * x0 + sqrt_1m_abar[s] * noise (DDIMScheduler.add_noise, :144-148),
 * noise_pred = eps-net(noisy, timesteps) (:151-160), loss = F.mse_loss(noise_pred, noise) (:164), backward, one Adam update with
 * learning rate lr.  x0_dev, noise_dev [samples][num_points]; sqrt_abar_dev, sqrt_1m_abar_dev [samples]; timesteps_dev [samples]
 * int64; pred_dev (optional) [samples][num_points] receives noise_pred; loss_host (optional) receives the loss and makes the call
 * synchronous, like loss.item().  Deterministic: same inputs, same bits.                                                           */
int dgdm_unet_trainer_step(DgdmUnetTrainer *m, const float *x0_dev, const float *noise_dev, const float *sqrt_abar_dev,
                           const float *sqrt_1m_abar_dev, const int64_t *timesteps_dev, int samples, float lr, float *pred_dev,
                           float *loss_host, void *stream);
/* The same without the update: forward (+ backward when backward != 0) on this rank's `samples` of a batch of `total_samples`
 * (d loss / d pred = 2 (pred - noise) / (total_samples num_points); *loss_host = this rank's share of the batch loss).  With
 * dgdm_unet_trainer_gradients (flat gradient buffer device -> flat_dev, or flat_dev -> device scaled by `scale` when to_trainer) and
 * dgdm_unet_trainer_apply (one Adam update) this is data-parallel training, one process per GPU, with an RCCL all-reduce in between
 * (Lightning's DDP averages the ranks' gradients: total_samples = samples, scale = 1 / world).                                      */
int dgdm_unet_trainer_forward_backward(DgdmUnetTrainer *m, const float *x0_dev, const float *noise_dev, const float *sqrt_abar_dev,
                                       const float *sqrt_1m_abar_dev, const int64_t *timesteps_dev, int samples, int64_t total_samples,
                                       int backward, float *pred_dev, float *loss_host, void *stream);
/* The two calls above for a conditional eps-net: global_cond_dev [samples][global_cond_dim] goes, after Mish, into every cond_encoder
 * next to the step embedding; weight and bias gradients cover all step_embed_dim + global_cond_dim columns, the condition itself is
 * data (no gradient).  The calls above are these with NULL; a handle with global_cond_dim > 0 needs a condition (DGDM_EINVAL).       */
int dgdm_unet_trainer_step_cond(DgdmUnetTrainer *m, const float *x0_dev, const float *noise_dev, const float *sqrt_abar_dev,
                                const float *sqrt_1m_abar_dev, const int64_t *timesteps_dev, const float *global_cond_dev, int samples,
                                float lr, float *pred_dev, float *loss_host, void *stream);
int dgdm_unet_trainer_forward_backward_cond(DgdmUnetTrainer *m, const float *x0_dev, const float *noise_dev, const float *sqrt_abar_dev,
                                            const float *sqrt_1m_abar_dev, const int64_t *timesteps_dev, const float *global_cond_dev,
                                            int samples, int64_t total_samples, int backward, float *pred_dev, float *loss_host,
                                            void *stream);
int dgdm_unet_trainer_global_cond_dim(const DgdmUnetTrainer *m);
int64_t dgdm_unet_trainer_gradient_count(const DgdmUnetTrainer *m);
int dgdm_unet_trainer_gradients(DgdmUnetTrainer *m, float *flat_dev, int64_t numel, int to_trainer, float scale, void *stream);
int dgdm_unet_trainer_apply(DgdmUnetTrainer *m, float lr, void *stream);
/* EMAModel.step (diffusers 0.11.1, called from on_train_batch_end, diffusion.py:716-720): ema = ema * decay + one_minus_decay * param
 * for every parameter; the decay schedule (power, update_after_step) is the caller's.                                              */
int dgdm_unet_trainer_ema_step(DgdmUnetTrainer *m, float decay, float one_minus_decay, void *stream);
/* which = 0 parameters, 1 gradients of the last backward, 2 / 3 Adam's exp_avg / exp_avg_sq, 4 the EMA copy; tensors are matched by
 * name and written (export: data is written despite the const) or read (import; adam_steps >= 0 also sets Adam's step count -
 * resuming from a checkpoint).                                                                                                      */
int dgdm_unet_trainer_export(DgdmUnetTrainer *m, int which, DgdmTensor *tensors, int n_tensors);
int dgdm_unet_trainer_import(DgdmUnetTrainer *m, int which, const DgdmTensor *tensors, int n_tensors, int64_t adam_steps);
int64_t dgdm_unet_trainer_steps(const DgdmUnetTrainer *m);      /* Adam updates taken */

/* ------------------------------------------------------------------ (f) rank 4: training the 3-D dynamics model
 * Trainer.step / Trainer.inference (dynamics/trainer.py:53-146) for ProfileForward3DModel (dynamics/profile_forward_3d.py:13-86):
 * PointNet++ (dynamics/models/pointnet2.py:11-32, pointnet2_utils.py:169-210) with BatchNorm2d in TRAINING mode, the trunk with
 * BatchNorm1d batch statistics, nn.MSELoss, backward with every weight gradient, torch.optim.Adam (trainer.py:46) - evaluated as
 * written, one row = one (control points, pose, cloud) item.  state_dict: the model's tensors ("module."-prefix stripped),
 * running statistics included; time_encoder (constructed, never called by forward) is carried unchanged.                           */
typedef struct DgdmTrainer3d DgdmTrainer3d;
int dgdm_trainer3d_create(DgdmTrainer3d **out, const DgdmTensor *state_dict, int n_tensors, int params_ch, int num_object_points,
                          float beta1, float beta2, float eps, float weight_decay);
void dgdm_trainer3d_destroy(DgdmTrainer3d *m);
/* One forward / backward / optimizer.step() of the loop body of trainer.py:83-92 (one slice of --use_sub_batch; the whole batch when
 * it is not sub-batched) when train != 0; train == 0: Trainer.inference's eval-mode forward + loss (:108-146).
 *   ctrl1_dev [rows][params_ch]   channel 1 of the control points, the only one the model reads (profile_forward_3d.py:77) and the
 *                                 only one trainer.py:68 adds noise to: noisy = sqrt_abar[r] * ctrl1 + sqrt_1m_abar[r] * noise (null: as given)
 *   t_dev [rows] = timesteps / num_train_timesteps (:80); ori_dev [rows][1]; pos_dev [rows][2]; score_dev [rows][3]
 *   xyz_dev [rows][num_object_points][3]  the clouds, point-major (the model's (rows, 3, N) input transposed)
 *   start_sa1_host / start_sa2_host [rows] int64: the FPS start draws of pointnet2_utils.py:83 for sa1 and sa2, in the order the
 *                                 reference makes them (torch.randint on the CPU generator, sa1 then sa2, per forward)
 * pred_dev (optional) [rows][3]; loss_host (optional) receives the loss and makes the call synchronous.  Deterministic.
 * Memory: 68 MB of activations and gradients per row (PointNet++ as written): rows <= 4096.                                        */
int dgdm_trainer3d_step(DgdmTrainer3d *m, const float *ctrl1_dev, const float *noise_dev, const float *sqrt_abar_dev,
                        const float *sqrt_1m_abar_dev, const float *t_dev, const float *ori_dev, const float *pos_dev, const float *xyz_dev,
                        const int64_t *start_sa1_host, const int64_t *start_sa2_host, const float *score_dev, int64_t rows, float lr,
                        int train, float *pred_dev, float *loss_host, void *stream);
/* Data-parallel training, one process per GPU, with nn.DataParallel's semantics (dynamics/trainer.py:41-43 wraps the 3-D model as well):
 *   dgdm_trainer3d_forward_backward  this rank's `rows` of a batch (or --use_sub_batch slice) of `total_rows`: forward in training mode on
 *                                    these rows' batch statistics (running statistics updated), loss share sum / (3 total_rows), backward;
 *                                    no update
 *   dgdm_trainer3d_gradients         the flat gradient buffer (dgdm_trainer3d_gradient_count floats, layout private to the library) read
 *                                    (to_trainer = 0) or written back after the all-reduce (1)
 *   dgdm_trainer3d_apply             one Adam update from the gradient buffer
 *   dgdm_trainer3d_running_stats     BatchNorm running means / variances of all 13 layers as one flat buffer
 *                                    (dgdm_trainer3d_running_stats_count floats): rank 0's are broadcast after every step
 * dgdm_trainer3d_step(train = 1) == forward_backward(rows, rows) + apply.                                                              */
int dgdm_trainer3d_forward_backward(DgdmTrainer3d *m, const float *ctrl1_dev, const float *noise_dev, const float *sqrt_abar_dev,
                                    const float *sqrt_1m_abar_dev, const float *t_dev, const float *ori_dev, const float *pos_dev,
                                    const float *xyz_dev, const int64_t *start_sa1_host, const int64_t *start_sa2_host, const float *score_dev,
                                    int64_t rows, int64_t total_rows, float *pred_dev, float *loss_host, void *stream);
int64_t dgdm_trainer3d_gradient_count(const DgdmTrainer3d *m);
int dgdm_trainer3d_gradients(DgdmTrainer3d *m, float *flat_dev, int64_t numel, int to_trainer, void *stream);
int dgdm_trainer3d_apply(DgdmTrainer3d *m, float lr, void *stream);
int64_t dgdm_trainer3d_running_stats_count(const DgdmTrainer3d *m);
int dgdm_trainer3d_running_stats(DgdmTrainer3d *m, float *flat_dev, int64_t numel, int to_trainer, void *stream);
/* which = 0 the state_dict (parameters + running statistics), 1 gradients of the last step, 2 / 3 Adam's exp_avg / exp_avg_sq */
int dgdm_trainer3d_export(DgdmTrainer3d *m, int which, DgdmTensor *tensors, int n_tensors);
int64_t dgdm_trainer3d_steps(const DgdmTrainer3d *m);      /* training steps taken = num_batches_tracked increment */
/* Test hook: an intermediate tensor of the last call, `count` 32-bit words device -> out_dev.  which: 0 trunk input [rows][800] =
 * [object embedding 256 | gripper 256 | pose 27 | time 256 | 0 x 5], 1 sa1 output [rows*512][128], 2 sa2 output [rows*128][256],
 * 3 sa1 grouped coordinates [rows*512*32][4], 4 sa1 first conv [..][64], 5 sa1 centres [rows][512][3], 6 sa1 FPS indices (int32),
 * 7 sa1 ball lists (int32), 8 gradient of the trunk input [rows][800], 9 predictions [rows][4].                                    */
int dgdm_trainer3d_debug_read(DgdmTrainer3d *m, int which, void *out_dev, int64_t count, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* DGDM_HIP_H */

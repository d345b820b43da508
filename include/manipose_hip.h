/* manipose_hip.h -- C ABI of libmanipose_hip.so: the MI355X (gfx950) implementation of ManiPose's
 * data-parallel 2D->3D lifting hot path.
 *
 * The reference (cedricrommel/manipose @ 2025-01-17) is pure Python/PyTorch and has NO native interface;
 * its "plugin API" for this path is the nn.Module contract of hpe/mh_so3_hpe/architectures.
 * This header is the boundary a binding for that contract attaches to (ctypes stub: INTEGRATION.md; the
 * in-tree binding is manipose_amd/_lib.py).  Each entry point names the reference code it replaces
 * (paths relative to the reference root).
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no torch types.  All data pointers are DEVICE pointers to
 *     contiguous fp32 buffers unless stated otherwise; `stream` is a hipStream_t (NULL = default stream).
 *   - every function returns 0 on success, non-zero on error (1 bad argument, 2 HIP runtime error,
 *     3 bad state); mp_last_error() returns the message of the last failure on the calling thread.
 *   - calls only ENQUEUE work on `stream`; nothing synchronises the host except mp_prof_collect().
 *   - token layout everywhere: row m = (b*T + t)*J + j of a (B, T, J, C) activation.
 *   - pose layout: (B, K, T, 17, 3); scores: (B, K, T[, 1]); targets: (B, T, 17, 3)  (reference layouts).
 */
#ifndef MANIPOSE_HIP_H
#define MANIPOSE_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MP_ABI_VERSION 8

int mp_abi_version(void);
const char* mp_last_error(void);

/* ------------------------------------------------------------------------------------------------
 * Stand-alone operators (the HBM-bound kernels of the path; also used by the roofline harness)
 * ---------------------------------------------------------------------------------------------- */

/* PoseDecoder.forward: architectures/pose_decoder.py:32-55 = _compute_rotation_mats (:57-83,
 * utils/rotation_tools.py:35-57) + build_t_pose_from_bone_lengths (:98-120) + forward_kinematics
 * (utils/forward_kinematics.py:6-48), root at the origin (rmcl_manifold_mix_ste.py:92).
 *   rot6d  : (K, B*T*17, rot_stride) head output, channels 0..rot_dim-1 are the rotation representation (rot_stride >= rot_dim)
 *   rot_dim: 6 = two 3-vectors, Gram-Schmidt (rotation_tools.py:35-57); 4 = two 2-vectors -> R_theta R_phi
 *            (rotation_tools.py:60-116; conf/config.yaml:47 model.rot_dim)
 *   lengths: (B, 16) segment lengths;  poses: (B, K, T, 17, 3) */
int mp_fk_decode_fwd(const float* rot6d, int rot_stride, int rot_dim, const float* lengths, float* poses, int B, int K, int T,
                     void* stream);
/* gradient of the above: d_rot6d has rot6d's layout (channels >= rot_dim untouched); d_len_pose: (B*K*T, 16)
 * per-pose segment-length gradients (summed over a window's poses by mp_bones_mean_bwd). */
int mp_fk_decode_bwd(const float* rot6d, int rot_stride, int rot_dim, const float* lengths, const float* d_poses, float* d_rot6d,
                     float* d_len_pose, int B, int K, int T, void* stream);

/* Multi-hypothesis training loss with its gradient, metrics/losses.py:104-170 + :75-101 +
 * metrics/regularizations.py:160-174 assembled like make_loss/compute_and_acc_loss
 * (hpe/main_h36m_lifting.py:101-209).  terms (device, 4 floats) = wloss, score_reg, vloss, sreg (already
 * weighted; total = their sum).  argmin (device int32 (B,T)) / d_poses / d_scores may be NULL.
 * scratch: >= 4*ceil(B*T/256) floats; with >= 4*ceil(B*T/48) the kernel runs on more, shorter-lived workgroups (same results up to the order of the
 * final sum). */
typedef struct mp_loss_config {
  float rmcl_score_reg; /* beta, conf/config.yaml:36 (0.1) */
  float vel_loss;       /* conf/config.yaml:33 (2.0) */
  float smooth_reg;     /* conf/config.yaml:34 (0.5) */
  int w_loss;           /* conf/config.yaml:32: 1 = weight joints by STANDARD_H36M_WEIGHTS (losses.py:6-8); 0 = unweighted; 2 = joint_weights below */
  int sq_loss;          /* conf/config.yaml:31: squared distances in the WTA and velocity terms (losses.py:46-72,96-97,110-116) */
  float joint_weights[17]; /* w_loss == 2: the caller's per-joint weights (the `weights` argument of losses.py:14-43,104-138, regularizations.py:160-174) */
} mp_loss_config;
int mp_wta_loss(const float* poses, const float* scores, const float* target, const mp_loss_config* cfg, float* terms,
                int32_t* argmin, float* d_poses, float* d_scores, int B, int K, int T, float* scratch,
                int64_t scratch_floats, void* stream);
/* single-hypothesis variant (ManifoldMixSTE, make_loss :113-127): terms (3 floats) = wloss, vloss, sreg */
int mp_single_loss(const float* poses, const float* target, const mp_loss_config* cfg, float* terms, float* d_poses,
                   int B, int T, float* scratch, int64_t scratch_floats, void* stream);

/* The rigid_seg_reg term of make_loss (hpe/main_h36m_lifting.py:170-177): weight * segments_time_consistency(pred.permute(0,3,2,1),
 * skeleton, mode="sum") (metrics/regularizations.py:8-45, metrics/utils.py:4-20) = weight * sum over windows and the 16 bones of the
 * unbiased variance over time of the bone length, for (B, T, 17, 3) predictions of the single-hypothesis models.  term: 1 device float;
 * d_poses (may be NULL): the gradient is ADDED to it (the other loss terms' gradient is already there).  scratch >= B floats. */
int mp_rigid_segments_loss(const float* poses, float weight, float* term, float* d_poses, int B, int T, float* scratch,
                           int64_t scratch_floats, void* stream);

/* RMCLManifoldMixSTE.aggregate (rmcl_manifold_mix_ste.py:141-185): mode 0 "weighted_ave", 1 "best_score",
 * 2 "oracle" (needs target).  out: (B, T, 17, 3). */
int mp_aggregate(const float* poses, const float* scores, const float* target, int mode, float* out, int B, int K, int T,
                 void* stream);
/* mpjpe_error(mode="sum") (metrics/mean_joint_errors.py:31-36): out_sum (device, 1 float) = sum of the
 * per-joint L2 errors of n_joints joints.  scratch >= 4*min(ceil(n/256),1024)+4 floats. */
int mp_mpjpe_sum(const float* pred, const float* target, int64_t n_joints, float* out_sum, float* scratch,
                 int64_t scratch_floats, void* stream);

/* torch.optim.Adam(lr, weight_decay) update (hpe/main_h36m_lifting.py:234-238), fused over a flat buffer.
 * grad_scale multiplies the gradient first (1/world_size after a sum all-reduce). step counts from 1. */
int mp_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, int step, float lr,
                 float beta1, float beta2, float eps, float weight_decay, float grad_scale, void* stream);

/* The same with per-element multipliers of the learning rate and of the weight decay (flat buffers in the parameter layout):
 * mup.optim.MuAdam as the reference builds it under model.mup (hpe/main_h36m_lifting.py:227-232) - parameters with two width
 * dimensions train with lr / width_mult and weight_decay * width_mult. */
int mp_adam_step_scaled(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, int step, float lr, float beta1,
                        float beta2, float eps, float weight_decay, float grad_scale, const float* lr_mult, const float* wd_mult, void* stream);

/* Building blocks exposed for unit parity tests (same kernels the model engine launches). */
int mp_layernorm_fwd(const float* x, const float* gamma, const float* beta, float eps, float* y, float* stats, int M, int C,
                     void* stream);
/* scratch: >= 1024 * 2 * C floats (per-workgroup dgamma/dbeta partials, reduced deterministically) */
int mp_layernorm_bwd(const float* dy, const float* x, const float* stats, const float* gamma, const float* dskip, float* dx,
                     float* dgamma, float* dbeta, int M, int C, float* scratch, int64_t scratch_floats, void* stream);
/* y = x W^T + b (nn.Linear); epilogue 0 none, 1 GELU (z receives gelu'(x W^T + b), which is all the backward needs), 2 residual: y = r + y */
int mp_linear_fwd(const float* x, const float* W, const float* b, float* y, float* z, const float* r, int M, int N, int K,
                  int epilogue, void* stream);
/* dx = dy W ; dW += dy^T x ; db += colsum(dy).  slab >= workspace reported by mp_linear_bwd_slab_floats */
int64_t mp_linear_bwd_slab_floats(int N, int K);
int mp_linear_bwd(const float* dy, const float* x, const float* W, float* dx, float* dW, float* db, int M, int N, int K,
                  float* slab, int64_t slab_floats, void* stream);
/* bf16 matrix-core variants (precision 1 of the engine).  x, W, dy are bf16 unless *_f32 says fp32; y/z bf16, dx fp32
 * or bf16 (dx_f32); r and the residual output y of epilogue 2 are fp32; dW/db fp32 (accumulated). */
int mp_linear_fwd_bf16(const void* x, const void* W, const float* b, void* y, void* z, const float* r, int M, int N, int K,
                       int epilogue, void* stream);
int mp_linear_bwd_bf16(const void* dy, int dy_f32, const void* x, const void* W, void* dx, int dx_f32, float* dW, float* db,
                       int M, int N, int K, float* slab, int64_t slab_floats, void* stream);
/* Attention core of Attention.forward (architectures/mix_ste.py:271-279) on a fused qkv buffer (M, 3C).
 * temporal = 0: attends over the J tokens of a frame; 1: over the T frames of a joint. */
int mp_attention_fwd(const float* qkv, float* out, float* lse, int temporal, int B, int T, int J, int C, int H, void* stream);
int mp_attention_bwd(const float* qkv, const float* out, const float* d_out, const float* lse, float* delta, float* d_qkv,
                     int temporal, int B, int T, int J, int C, int H, void* stream);

/* bf16 storage variants of the two calls above (temporal: MFMA kernels when T <= 256 and head dim in {64, 16}) */
int mp_attention_fwd_bf16(const void* qkv, void* out, float* lse, int temporal, int B, int T, int J, int C, int H, void* stream);
int mp_attention_bwd_bf16(const void* qkv, const void* out, const void* d_out, const float* lse, float* delta, void* d_qkv,
                          int temporal, int B, int T, int J, int C, int H, void* stream);

/* Split precision "bf16x3" (precision 2 of the engine): a value x is carried as two bf16 numbers hi = bf16(x), lo = bf16(x - hi)
 * in two planes of the same shape, and every product a*b of a Linear layer (architectures/mix_ste.py:216-222,257-261,280-281) or of
 * the attention core (:271-279) is evaluated as a_lo*b_hi + a_hi*b_lo + a_hi*b_hi on the bf16 matrix cores with fp32 accumulation:
 * 16 significand bits per operand, which keeps the model within the 1e-4 m MPJPE bound of the fp32 reference at matrix-core speed.
 * mp_split_bf16: fp32 -> (hi, lo) planes (n a multiple of 4). */
int mp_split_bf16(const float* src, void* hi, void* lo, int64_t n, void* stream);
/* y = x W^T + b on planar operands.  epilogue 0: y planar (y = hi plane, y_lo); 1: GELU, y planar and z = gelu'(pre-activation) as
 * plain bf16; 2: y = r + (x W^T + b) in fp32 (y_lo unused). */
int mp_linear_fwd_bf16x3(const void* x_hi, const void* x_lo, const void* W_hi, const void* W_lo, const float* b, void* y, void* y_lo,
                         void* z, const float* r, int M, int N, int K, int epilogue, void* stream);
/* The residual Linear of a Block from the third block on (architectures/mix_ste.py:352-368 inside ST_foward :157-173): the block input is
 * the shared post-norm of the previous block's output, x = LayerNorm(r_in) (Spatial_norm / Temporal_norm, eps folded into rstats), which
 * the engine never materialises - the epilogue recomputes it from r_in and its row statistics while adding the branch:
 *   y[m][n] = (r_in[m][n] - mean[m]) * rstd[m] * rgamma[n] + rbeta[n] + mask(m) * (x W^T + b)[m][n]        (fp32, N columns)
 * rstats: (M, 2) = (mean, rstd) per row; mask: DropPath multipliers per sample or NULL (mask_mode 1: sample = m / J, a spatial block's
 * (b, t); 2: sample = b * J + m % J, a temporal block's (b, j), with b = m / (T J)); r_in and y may not alias.  This is the same
 * kernel path mp_model_forward takes in precision 2 (persistent split-precision GEMM when the problem has >= 2 tiles per CU or
 * "gemm_persist_min_tiles" says so). */
int mp_linear_fwd_bf16x3_lnres(const void* x_hi, const void* x_lo, const void* W_hi, const void* W_lo, const float* b, float* y,
                               const float* r_in, const float* rstats, const float* rgamma, const float* rbeta, const float* mask, int mask_mode,
                               int T, int J, int M, int N, int K, void* stream);
/* The same Linear (architectures/mix_ste.py:216-222, 257-261) on the "f16f8" operand format - one fp16 product plus ONE block-scaled fp8
 * product per 64 reduction indices instead of three bf16 products.  A value v is carried as hi = fp16(v) (x16 / W16, row-major [rows][K])
 * and a correction plane of the same byte geometry (x8 / W8: 2 K bytes per row): for every four reduction indices 4 q .. 4 q + 3 the 8 bytes
 *   activation row:  4 x e4m3(2^11 (v - hi))  |  4 x e4m3(hi)
 *   weight row:      4 x e4m3(2^4 hi)         |  4 x e4m3(2^15 (v - hi))
 * so that the fp8 dot product of an activation row and a weight row is 2^15 (x_lo w_hi + x_hi w_lo).  y = x W^T + b in fp32.
 * N must be a multiple of 256, K of 64 (>= 128).  Two kernels serve it with the same bits: the persistent 256 x 256 one and a tiled 128 x 128
 * one (two workgroups per CU) that mp_gemm_plan picks for the token counts of a few windows.  The engine runs its qkv and fc1 forward GEMMs in this form with mp_model_config::f16f8 = 1,
 * the fc2 GEMM too with f16f8 = 2, and all four Linear layers of a block with f16f8 = 3 (the default of the training configuration). */
/* fp32 -> the two planes of that format for a matrix whose rows are multiples of 64 elements long (n = rows * K elements; hi16: n fp16
 * values, corr8: 2 n bytes); weight != 0 selects the weight form of the correction rows. */
int mp_split_f16f8(const float* src, void* hi16, void* corr8, int64_t n, int weight, void* stream);
int mp_linear_fwd_f16f8(const void* x16, const void* x8, const void* W16, const void* W8, const float* b, float* y, int M, int N, int K,
                        void* stream);
/* attention core on a planar fused qkv buffer, planar output.  scratch: 4*M*C floats, needed only where no MFMA kernel covers the
 * shape (spatial: 16 <= J <= 32 tokens, head dim 64 or 16, <= 8 heads; temporal: T <= 256, head dim 64 or 16); NULL otherwise. */
int mp_attention_fwd_bf16x3(const void* qkv_hi, const void* qkv_lo, void* out_hi, void* out_lo, float* lse, float* scratch, int temporal,
                            int B, int T, int J, int C, int H, void* stream);
/* The other forms of the f16f8 path (mp_model_config::f16f8 >= 1), each through the dispatcher the engine calls.
 * mp_linear_fwd_f16f8_ex: the Linear above with every epilogue.  epilogue 0 bias, 1 GELU (z: gelu'(pre-activation) as bf16, may be NULL),
 * 2 residual (y = LN(r_in) + mask * (x W^T + b) with rstats / rgamma / rbeta as in mp_linear_fwd_bf16x3_lnres, or y = r_in + mask * (..)
 * when they are NULL; rscale must be 0 or 1).  out_form 0: y fp32 (epilogues 0, 2); 1: planar bf16, y = hi plane, y_lo = lo plane
 * (epilogues 0, 1); 2: y = fp16 plane, y_lo = correction plane of the activation form (epilogue 1).  Other combinations: MP_ERR_ARG. */
int mp_linear_fwd_f16f8_ex(const void* x16, const void* x8, const void* W16, const void* W8, const float* b, void* y, void* y_lo, void* z,
                           const float* r_in, const float* rstats, const float* rgamma, const float* rbeta, const float* mask, int mask_mode,
                           float rscale, int T, int J, int M, int N, int K, int epilogue, int out_form, void* stream);
/* The fused LayerNorm forward of the engine: stage 1 (g1 non-NULL) x1 = LN(x; g1, b1, eps1) [+ pos[t]] (fp32, x1 may be NULL: not stored),
 * stats1 = (mean, rstd) per row; stage 2 (g2 non-NULL) y2 = LN(stage-1 output or x; g2, b2, eps2) in out_mode 0 fp32, 1 bf16, 2 planar bf16
 * (y2_lo the lo plane), 3 f16f8 (y2 the fp16 plane, y2_lo the correction plane; y2_b16 an optional bf16 copy).  C <= 1024. */
int mp_layernorm_fwd_ex(const float* x, int M, int C, const float* g1, const float* b1, float eps1, const float* pos, int T, int J, float* x1,
                        float* stats1, const float* g2, const float* b2, float eps2, void* y2, void* y2_lo, void* y2_b16, float* stats2, int out_mode,
                        void* stream);
/* mp_attention_fwd_bf16x3 with out_form 1: the output as f16f8 planes (out_hi = fp16 plane, out_lo = correction plane; head dim 64) */
int mp_attention_fwd_bf16x3_ex(const void* qkv_hi, const void* qkv_lo, void* out_hi, void* out_lo, float* lse, float* scratch, int temporal,
                               int B, int T, int J, int C, int H, int out_form, void* stream);
/* mp_attention_bwd_bf16 with out_f16 = 1: O is the fp16 plane of an f16f8 output (temporal MFMA backward only; MP_ERR_ARG elsewhere) */
int mp_attention_bwd_bf16_ex(const void* qkv, const void* out, const void* d_out, const float* lse, float* delta, void* d_qkv, int temporal, int B,
                             int T, int J, int C, int H, int out_f16, void* stream);
/* The three calls above in the forms only a model reaches otherwise.  qk_scale: the softmax scale (mp_model_config::qk_scale; muP: 1 / head_dim),
 * 0 = head_dim ** -0.5.  grad_scale (backward; NULL = bf16 outputs): the 8-float gradient-scale block {S, 1 / S, -, 1, clamped (u32), non-finite
 * (u32), -, -} of an f16_backward model on the device - dQ / dK / dV leave as fp16 of S x value, stores beyond +-65504 are clamped, non-finite ones
 * written as 0, and both are counted in the block.  Only the MFMA backward kernels have that store: MP_ERR_ARG for a shape the row kernels serve. */
int mp_attention_fwd_bf16_scale_ex(const void* qkv, void* out, float* lse, int temporal, int B, int T, int J, int C, int H, float qk_scale,
                                   void* stream);
int mp_attention_bwd_bf16_scale_ex(const void* qkv, const void* out, const void* d_out, const float* lse, float* delta, void* d_qkv, int temporal,
                                   int B, int T, int J, int C, int H, int out_f16, float qk_scale, const float* grad_scale, void* stream);
int mp_attention_fwd_bf16x3_scale_ex(const void* qkv_hi, const void* qkv_lo, void* out_hi, void* out_lo, float* lse, float* scratch, int temporal,
                                     int B, int T, int J, int C, int H, int out_form, float qk_scale, void* stream);
/* Backward GEMMs of the f16f8 layers.  dgrad (dx non-NULL): dx = dy W (bf16 out), times z = gelu' (bf16) when z is non-NULL; f16 = 1: dy and W
 * are fp16; gout non-NULL (device address): dx is written as saturating fp16 of *gout x value, clamped at +-65504, non-finite values as 0,
 * counted in gsat[0] (clamped) and gsat[1] (non-finite), which are added to.  Weight gradient (dW non-NULL): dW += dy^T x, db += colsum(dy);
 * f16 = 1: dy and x fp16, the sums multiplied by *oscale (device address); x_f16 = 1: dy bf16, x fp16 rounded to bf16; slab as mp_linear_bwd_bf16. */
int mp_linear_bwd_f16(const void* dy, const void* x, const void* W, void* dx, const void* z, const float* gout, uint32_t* gsat, float* dW, float* db,
                      int M, int N, int K, int f16, int x_f16, const float* oscale, float* slab, int64_t slab_floats, void* stream);
/* The LayerNorm backward forms of the engine's backbone backward.  mp_layernorm_bwd_ex: dx = rs * dskip + LN'(dy) (dskip may be NULL; dx may
 * alias dy or dskip, as in the engine); dy fp32 or (dy_bf16) bf16.  dx_b16 (may be NULL): a 2-byte copy of dx times the DropPath multiplier
 * of its row (mask, mask_mode 1 / 2 as in mp_linear_fwd_bf16x3_lnres; M a multiple of T*J), bf16, or with copy_f16 the saturating fp16 of
 * dx * mask * gsc[0] (clamped at +-65504, non-finite as 0, counted in the uint32 words gsc[4] / gsc[5], which are added to).  gsc: the
 * engine's 8-float gradient-scale block {S, 1/S, ..}; dy_scaled multiplies dy by gsc[1] on load.  dgamma / dbeta are ACCUMULATED into;
 * scratch >= 1024 * 2 * C floats; C <= 1024.  param_stream (may be NULL): the reduction of the partial sums into dgamma / dbeta runs on that
 * stream, ordered behind the row kernel by an event (the caller keeps scratch until it has run).
 * mp_layernorm_bwd2_ex: the fused pair t = rs * dskip + LN1'(dy1) with x1 = LN0(x0; stats0, gamma0, beta0) recomputed in fp32, then
 * dx = LN0'(t); dgamma1 / dbeta1 / dgamma0 / dbeta0 accumulated; C <= 512, scratch >= 1024 * 4 * C floats, dskip and beta0 required.
 * mp_scale_rows_ex: out = mask(m) * g (the fp32-precision DropPath of a branch gradient), fp32 or (out_bf16) bf16.  Bad arguments: MP_ERR_ARG
 * before any launch. */
int mp_layernorm_bwd_ex(const void* dy, int dy_bf16, const float* x, const float* stats, const float* gamma, const float* dskip, float rs, float* dx,
                        void* dx_b16, const float* mask, int mask_mode, int T, int J, float* gsc, int dy_scaled, int copy_f16, float* dgamma,
                        float* dbeta, int M, int C, float* scratch, int64_t scratch_floats, void* param_stream, void* stream);
int mp_layernorm_bwd2_ex(const void* dy1, int dy_bf16, const float* stats1, const float* gamma1, const float* dskip, float rs, const float* x0,
                         const float* stats0, const float* gamma0, const float* beta0, float* dx, void* dx_b16, const float* mask, int mask_mode, int T,
                         int J, float* gsc, int dy_scaled, int copy_f16, float* dgamma1, float* dbeta1, float* dgamma0, float* dbeta0, int M, int C,
                         float* scratch, int64_t scratch_floats, void* param_stream, void* stream);
int mp_scale_rows_ex(const float* g, const float* mask, int mask_mode, void* out, int out_bf16, int M, int C, int T, int J, void* stream);

/* The kernels at the two ends of the network, each through the engine's own launcher, all fp32.  Bad arguments (null pointers, non-positive
 * dimensions, the limits named below, short scratch): MP_ERR_ARG before any launch.  Every gradient of a parameter is ACCUMULATED into.
 * Input embedding of the rotation backbone (mix_ste.py:134-138): out[m][c] = W[c][0] x[m][0] + W[c][1] x[m][1] + b[c] + spos[m % J][c];
 *   x [M][2], W [C][2], b [C], spos [J][C], out [M][C]; C % 4 == 0.  Backward: dW += g^T x, db += colsum(g), dspos[j] += sum of the rows m with
 *   m % J == j, over the M / J WHOLE frames only: rows past the last whole frame (M % J != 0) enter no sum.  J == 17 with C % 4 == 0 and M % 17 == 0
 *   runs the four-channel kernel, everything else the channel-per-thread kernel.  scratch: mp_embed_bwd_scratch_floats(C, J).
 * Input embedding of the bones net (manifold_mix_ste.py:133-150): out[f][o] = sum_i W[o][i] x[f][i] + b[o] + spos[o], IN == 34;
 *   x [BT][34], W [O][34], b, spos [O], out [BT][O].  Backward: dW += g^T x, db += colsum(g), dspos += colsum(g);
 *   scratch >= (min(32, BT) + 1) * O * 35 floats.
 * mp_tpos_grad_ex: dtpos[t][c] += sum_{b,j} g[((b T + t) J + j)][c]; g [B T J][C], dtpos [T][C]; C % 4 == 0 and J >= 4 (the kernel walks the
 *   (b, j) rows of a frame four at a time; a smaller J is refused, dtpos untouched). */
int mp_embed_fwd_ex(const float* x, const float* W, const float* b, const float* spos, float* out, int M, int C, int J, void* stream);
int64_t mp_embed_bwd_scratch_floats(int C, int J);
int mp_embed_bwd_ex(const float* g, const float* x, float* dW, float* db, float* dspos, int M, int C, int J, float* scratch, int64_t scratch_floats,
                    void* stream);
int mp_bones_embed_fwd_ex(const float* x, const float* W, const float* b, const float* spos, float* out, int BT, int IN, int O, void* stream);
int mp_bones_embed_bwd_ex(const float* g, const float* x, float* dW, float* db, float* dspos, int BT, int IN, int O, float* scratch,
                          int64_t scratch_floats, void* stream);
int mp_tpos_grad_ex(const float* g, float* dtpos, int B, int T, int J, int C, void* stream);
/* Score head (rmcl_manifold_mix_ste.py:291-298): logit[b][k][t] = sum_j w[k][j] headout[k][(b T + t) J + j][O - 1] + b[k], scores = softmax over k;
 *   headout [K][B T J][O], packed w [K][J], b [K], scores [B][K][T]; 1 <= K <= 8, 1 <= J <= 32.  Backward: dlogit = s (ds - sum_k s ds); channel
 *   O - 1 of dheadout is WRITTEN with dlogit w[k][j] (the other channels are not touched), dw[k][j] += sum_f dlogit emb, db[k] += sum_f dlogit;
 *   scratch: mp_scores_bwd_scratch_floats(K, B, T).  param_stream (may be NULL): the two parameter-gradient kernels run there, behind an event
 *   this call creates and destroys (the caller keeps scratch until that stream has run).
 * Bone lengths (manifold_mix_ste.py:154): lengths[b][s] = mean_t headout[(b T + t) S + s].  Backward: dlengths[b][s] (may be NULL; WRITTEN) = the
 *   sum over the KT decoded poses of window b of dlen_pose[(b KT + i) S + s], dheadout[(b T + t) S + s] = that sum / T; 1 <= S <= 32. */
int mp_scores_fwd_ex(const float* headout, const float* w, const float* b, int K, int O, float* scores, int B, int T, int J, void* stream);
int64_t mp_scores_bwd_scratch_floats(int K, int B, int T);
int mp_scores_bwd_ex(const float* headout, const float* scores, const float* d_scores, const float* w, const float* b, float* dw, float* db, int K,
                     int O, float* d_headout, int B, int T, int J, float* scratch, int64_t scratch_floats, void* param_stream, void* stream);
int mp_bones_mean_fwd_ex(const float* headout, float* lengths, int B, int T, int S, void* stream);
int mp_bones_mean_bwd_ex(const float* d_len_pose, int KT, float* d_lengths, float* d_headout, int B, int T, int S, void* stream);

/* K output heads, head k = LayerNorm(C, eps 1e-5) -> Linear(C, O)  (MCLHead stack, rmcl_manifold_mix_ste.py:291-298; MixSTE.head,
 * mix_ste.py:123-126), all fp32.  Packed parameters: gamma, beta [K][C]; W [K][O][C]; b [K][O].  out [K][M][O]; stats [M][2] (mean, rstd
 * of x, shared by the heads) and fold (mp_heads_fold_floats(C) floats: the LayerNorm affine folded into the weights) are written by the
 * forward and, with out, read by the backward.  impl 0 = the engine's choice (fp32 matrix cores when C is 128, 256 or 512 and K*O <= 48, row kernels
 * otherwise), 1 = row kernels, 2 = matrix cores (MP_ERR_ARG when the shape is not covered).
 * Backward: dx [M][C] is overwritten; dgamma, dbeta, dW, db are ACCUMULATED into.  scratch: mp_heads_bwd_scratch_floats(K, O, C). */
int64_t mp_heads_fold_floats(int C);
int64_t mp_heads_bwd_scratch_floats(int K, int O, int C);
int mp_heads_fwd(const float* x, const float* gamma, const float* beta, const float* W, const float* b, int K, int O, float* out, float* stats,
                 float* fold, int M, int C, int impl, void* stream);
int mp_heads_bwd(const float* x, const float* stats, const float* fold, const float* out, const float* gamma, const float* beta, const float* W,
                 const float* b, const float* d_out, float* dx, float* dgamma, float* dbeta, float* dW, float* db, int K, int O, int M, int C, int impl,
                 float* scratch, int64_t scratch_floats, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Model engine: RMCLManifoldMixSTE / ManifoldMixSTE forward + backward as one native launch sequence
 * (replaces RMCLManifoldMixSTE.forward, architectures/rmcl_manifold_mix_ste.py:83-106 and everything it
 * calls: mix_ste.py:128-173,216-222,255-282,352-368; manifold_mix_ste.py:75-88,139-154; pose_decoder.py)
 * ---------------------------------------------------------------------------------------------- */
typedef struct mp_model mp_model;

typedef struct mp_model_config {
  int arch;            /* 0 = "rmcl_manifold" (K heads + scores), 1 = "manifold" (single hypothesis), 2 = "mixste": the bare MixSTE
                        * regressor of main_h36m_lifting.py:617-628 (mix_ste.py:175-191; out_dim 3, no bones net, no decoder;
                        * state-dict keys without the "rotations_module." prefix) */
  int num_frame;       /* T  (cfg.data.seq_len) */
  int num_joints;      /* 17 */
  int num_bones;       /* 16 */
  int embed_dim_rot, depth_rot, num_heads_rot;
  int embed_dim_seg, depth_seg, num_heads_seg;
  int n_hyp;           /* K (ignored for arch 1) */
  float drop_path_rate;/* stochastic depth: linspace(0, rate, depth) per module (mix_ste.py:70) */
  int max_batch;       /* workspace is sized for this many windows; 0 = layout-only handle (no device memory) */
  int precision;       /* 0 = fp32 matrix cores; 1 = bf16 matrix cores / fp32 accumulate; 2 = "bf16x3": split-precision forward (planar hi/lo
                        * bf16 operands, three matrix-core products each: within the 1e-4 m MPJPE bound); the backward runs in bf16 on the hi
                        * planes unless f16_backward (below) moves the qkv / fc1 (/ fc2) layers of an f16f8 model to fp16 operands */
  int rot_rep_dim;     /* 6 (default when 0) or 4: rotation representation the heads emit (pose_decoder.py:22-31) */
  /* mu-parametrisation (model.mup, conf/config.yaml:52) and explicit attention scales; per backbone (rotations / segments), 0 = default:
   *   qk_scale      softmax scale of Attention (mix_ste.py:243-244): default head_dim^-0.5; muP 1 / head_dim
   *   resid_scale   Block.residual_scale (mix_ste.py:330,353-358): x = x * resid_scale + branch; default 1; muP 1 / sqrt(depth)
   *   readout_mult  multiplier on the input of the head's last Linear, mup.MuReadout (mix_ste.py:118-121, rmcl_manifold_mix_ste.py:278-285):
   *                 y = W (readout_mult * x) + b with readout_mult = output_mult / width_mult; default 1 */
  float qk_scale_rot, resid_scale_rot, readout_mult_rot;
  float qk_scale_seg, resid_scale_seg, readout_mult_seg;
  /* ABI v7: the numerics- and scheduling-affecting knobs of ONE model (they were process-wide options / environment variables up to v6;
   * the library reads no environment variable).  All 0 = the defaults.
   *   f16f8         precision 2 only, rotations net of a width that is a multiple of 256: 0 (default) = every Linear product as three bf16
   *                 products of bf16 hi / lo planes; 1 = the qkv and fc1 Linear layers read "f16f8" operands (mp_linear_fwd_f16f8: one fp16
   *                 product + one block-scaled fp8 correction product per 64 reduction indices); 2 = the fc2 layer as well (needs f16_backward);
   *                 3 (round 6; head dim 64, residual scale 1) = ALL FOUR Linear layers of a block: the attention kernels and the fc1 epilogue
   *                 write their outputs as f16f8 planes too, no bf16 copy of those activations exists, and the bf16 backward rounds the fp16
   *                 planes to bf16 where it reads them (weight-gradient GEMM fragments, the temporal attention backward's O); f16_backward
   *                 must be 0; a model that does not qualify (other head dims / widths, muP residual scale) runs as f16f8 = 0
   *   f16_backward  with f16f8 >= 1: 1 = the backward GEMMs of those layers run on fp16 operands - gradients carried as fp16 of S x value,
   *                 S a power of two chosen per backward on the device from the residual gradient at the top of the backbone, stores saturate at
   *                 +-65504 and are counted (mp_model_grad_health);
   *                 0 (default) = bf16 backward on a bf16 copy of those activations
   *   streams       bit 0 set: the segments net is enqueued on the caller's stream instead of the engine's side stream; bit 1 set: the
   *                 weight-gradient GEMMs likewise instead of the engine's third stream (debugging / single-queue profiles; results are
   *                 bit-identical either way) */
  int f16f8;
  int f16_backward;
  int streams;
  /* ABI v8.  debug: bit 0 = the stream-hazard check (below): every launch of mp_model_forward / mp_model_backward is declared to a host-side
   * tracker together with the events the engine records and waits on; costs host time only, changes no launch.  0 = off. */
  int debug;
} mp_model_config;

int mp_model_create(const mp_model_config* cfg, mp_model** out);
void mp_model_destroy(mp_model* m);
int64_t mp_model_workspace_bytes(const mp_model* m);

/* Flat parameter layout: parameter i (state-dict key `name`, reference naming) occupies
 * floats [offset, offset + numel) of the flat parameter buffer (offsets are 16-byte aligned; gaps are
 * padding).  The gradient buffer and the Adam moment buffers use the same layout. */
int mp_model_num_params(const mp_model* m);
int64_t mp_model_flat_size(const mp_model* m);
int mp_model_param_info(const mp_model* m, int index, char* name, int name_cap, int64_t* offset, int64_t* numel);

/* DropPath mask layout for a batch of B windows: branch i (name like "rotations_module.STEblocks.3.attn")
 * uses floats [offset, offset+count) of the mask buffer; values are 0 or 1/keep. */
int mp_model_num_mask_branches(const mp_model* m);
int mp_model_mask_info(const mp_model* m, int B, int index, char* name, int name_cap, int64_t* offset, int64_t* count,
                       float* keep_prob);
int64_t mp_model_mask_floats(const mp_model* m, int B);

/* forward: x (B, T, 17, 2) -> poses (B, K, T, 17, 3) [, scores (B, K, T, 1) for arch 0].
 * train is a bit set: bit 0 applies DropPath: masks = masks_override (device, layout above) if non-NULL, else drawn from
 * (seed, step); bit 1 (value 2) announces that NO mp_model_backward will follow this forward (torch.no_grad() evaluation): tensors that
 * only the backward reads are then not written, and mp_model_backward returns MP_ERR_STATE.  Otherwise the activations needed by
 * mp_model_backward are kept inside the model until the next forward. */
int mp_model_forward(mp_model* m, const float* flat_params, const float* x, int B, float* poses, float* scores, int train,
                     const float* masks_override, uint64_t seed, uint64_t step, void* stream);
/* backward of the LAST forward: d_poses (B,K,T,17,3), d_scores (B,K,T,1) or NULL; parameter gradients are
 * ACCUMULATED into flat_grads (zero it first for a fresh gradient). */
int mp_model_backward(mp_model* m, const float* flat_params, float* flat_grads, const float* d_poses, const float* d_scores,
                      void* stream);
/* Gradient buckets for overlapping the data-parallel exchange with the backward (the reference has no counterpart: it wraps the
 * model in nn.DataParallel, hpe/main_h36m_lifting.py:749-751).  Bucket i = the parameter gradients of layer i of the rotations net
 * (STEblocks.i and TTEblocks.i: one contiguous range [offset, offset + numel) of the flat gradient buffer, ~25 MB at full width).  The
 * backward finishes them from the last layer down; mp_model_grad_bucket_wait makes `stream` wait (device side, the host does not block)
 * until bucket `index` of the LAST mp_model_backward is final, so a collective enqueued on that stream afterwards runs while the rest of
 * the backward is still computing.  Everything outside the buckets (embeddings, shared norms, heads, the segments net) is final when the
 * stream mp_model_backward was given has passed the call. */
int mp_model_grad_bucket_count(const mp_model* m);
int mp_model_grad_bucket_info(const mp_model* m, int index, int64_t* offset, int64_t* numel);
int mp_model_grad_bucket_wait(mp_model* m, int index, void* stream);
/* Health of the scaled-fp16 gradient operands of the LAST mp_model_backward (f16_backward models; zeros otherwise): copies 4 floats to the
 * HOST after synchronising `stream`: out[0] = S, the power-of-two scale of that backward; out[1] = number of fp16 gradient elements that
 * hit the +-65504 clamp (stores saturate, they never write inf); out[2] = number of non-finite gradient elements met at those stores
 * (written as 0); out[3] = 1 / S (what consumers of the scaled operands multiply by).  A trainer that sees out[1] + out[2] > 0 should redo
 * the step with f16_backward off or skip it (manipose_amd/training.py sums the counters on the device, all-reduces the sum over the ranks and
 * raises / warns every health_interval steps - the steps since the last check were applied; health_interval = 1 stops on the first).  MP_ERR_STATE unless a completed mp_model_backward is
 * the last engine call (a forward, or a backward that failed midway, has overwritten what the counters described).
 * mp_model_grad_health_async: the same four values as floats into a DEVICE (or pinned host) buffer by an asynchronous copy on `stream`, no
 * host synchronisation - for a trainer that looks at the counters every N steps.  Cost, accepted: a backward of an f16_backward model reads the
 * residual-gradient stream of the heads once more on its main stream to choose S (one M x C fp32 pass, ~0.25 ms at the benchmark's batch) and
 * resets the counters there; the synchronous form blocks the host until `stream` is idle. */
int mp_model_grad_health(mp_model* m, float* out4_host, void* stream);
int mp_model_grad_health_async(mp_model* m, float* out4_device, void* stream);
/* Which of the engine's two extra streams the NEXT forward / backward calls use: the `streams` bit set of mp_model_config, changed on a live
 * model (bench.py times the kernel classes of the same model with every kernel on one queue).  Synchronises the engine's streams first. */
int mp_model_set_streams(mp_model* m, int streams);
/* Stream-hazard check (mp_model_config::debug bit 0; csrc/hazard.h): the engine runs its rotations net, its segments net and its weight-gradient
 * GEMMs on three streams ordered by events.  With the check on, every launch declares the byte ranges of the workspace / gradient buffers it
 * reads and writes and its stream, every event record / wait is mirrored, and a vector clock per stream decides for each pair of launches on
 * different streams that touch the same bytes (at least one writing) whether an event path orders them.  out4 = {launches declared, conflicting
 * cross-stream pairs found ORDERED, pairs found UNORDERED (violations), events recorded}; the first violations are written to `msg` as lines
 * of text (may be NULL).  Returns MP_ERR_STATE when the model was created without the debug bit. */
int mp_model_hazard_report(const mp_model* m, int64_t* out4, char* msg, int msg_cap);
/* The tracker by itself (no device involved; used by the CPU tests): streams and events are small integers. */
typedef struct mp_hazard mp_hazard;
mp_hazard* mp_hazard_create(void);
void mp_hazard_destroy(mp_hazard* h);
int mp_hazard_launch(mp_hazard* h, int stream, const char* name, int n, const int64_t* addr, const int64_t* bytes, const int* is_write);
int mp_hazard_record(mp_hazard* h, int event, int stream);
int mp_hazard_wait(mp_hazard* h, int stream, int event);
int mp_hazard_report(const mp_hazard* h, int64_t* out4, char* msg, int msg_cap);
/* intermediate outputs of the last forward (device pointers owned by the model): 0 = head output
 * (K, B*T*17, O), 1 = segment lengths (B, 16), 2 = the DropPath multipliers of the last train-mode forward (layout: mp_model_mask_info);
 * the fp32 residual stream block by block (blocks in execution order STE0, TTE0, STE1, ...; (B*T*N, C) each): 100 + 2 l = after the
 * attention branch of block l of the rotations net, 101 + 2 l = after its MLP branch, 99 = its embedding output; 300 + 2 l, 301 + 2 l,
 * 299 the same for the segments net; 500 / 501 / 502 = the 2-byte gradient operands dz (M x 2C) / dqkv (M x 3C) / residual-gradient copy (M x C) of the
 * LAST block the last backward differentiated (bf16, or scaled fp16 for dz / dqkv of an f16_backward model; numel counts floats = element pairs) */
int mp_model_peek(const mp_model* m, int which, const float** ptr, int64_t* numel);
/* copy `numel` floats of intermediate `which` into dst (device) on `stream` */
int mp_model_peek_copy(const mp_model* m, int which, float* dst, int64_t numel, void* stream);

/* per-kernel-class device timing (HIP events on the stream each kernel is launched on): classes 0 gemm_fwd, 1 gemm_dgrad,
 * 2 gemm_wgrad, 3 attention, 4 layernorm, 5 other partition the launches; class 6 gemm_persist is the SUBSET of classes 0/1 that
 * ran gemm_bf16_persist_kernel (the kernel with the largest share of a training step: its average launch time is what
 * rocprofv3 reports for that kernel name).  collect() synchronises the events, adds up elapsed ms / launch counts /
 * algorithmic FLOPs (and, for the forward / dgrad GEMM classes, algorithmic bytes: every operand read once, every output written
 * once) per class since the last reset and resets. */
#define MP_PROF_CLASSES 7
/* The Linear GEMM launches of the same interval by KIND = module * 12 + direction * 4 + layer (module 0 rotations / 1 segments net;
 * direction 0 forward, 1 dgrad, 2 weight gradient; layer 0 qkv, 1 proj, 2 fc1, 3 fc2: architectures/mix_ste.py:216-222,257-261,280-281):
 * what mp_prof_collect added up at its last call - elapsed ms, launches, how many of them ran gemm_bf16_persist_kernel, issued matrix-core
 * FLOPs, algorithmic bytes (forward / dgrad kinds) and 2 M N K - so that a forward instantiation running at 0.14 of the matrix peak is not
 * averaged with a dgrad running at 0.38.  Arrays of MP_PROF_KINDS entries; all but ms / launches may be NULL. */
#define MP_PROF_KINDS 24
int mp_prof_enable(mp_model* m, int on);
int mp_prof_collect(mp_model* m, double* ms, int64_t* launches, double* flops, double* bytes /* nullable: algorithmic bytes, GEMM classes */,
                    double* model_flops /* nullable: 2 M N K of the mathematical products; `flops` counts the matrix-core work issued, 3x that for the
                                         * split-precision forward */);
int mp_prof_kinds(const mp_model* m, double* ms, int64_t* launches, int64_t* persist_launches, double* flops, double* bytes, double* model_flops);

/* GPU-resident PoseSequenceGenerator (hpe/mh_so3_hpe/data/generators.py:44-219) + PoseFlip
 * (hpe/mh_so3_hpe/augmentations/transforms.py:7-28, functional.py:7-31): cuts B windows of T frames out of pose sequences stored
 * back to back in device memory.  poses_2d (Ntot,J,2), poses_3d (Ntot,J,3); seq_offset (S+1) device int64: first frame of each
 * sequence; win_seq / win_start (B) device int32: sequence and first frame (within it) of every window - the reference's
 * _map_index_to_pose / _map_index_to_frame entries or its random start; frames past the end of the sequence replicate its last
 * frame (the drop_last=False padding); win_flip (B) device bytes or null: windows to mirror (u / x negated, joint j read from
 * mirror[j]); mirror (J) HOST int32.  mask2d (B,T,J) device floats or null: multipliers of the 2-D input (the occlusion patterns
 * of generators.py:171-216); noise2d (B,T,J,2) or null: noise added to the 2-D input before the mask (miss_type "noisy").
 * Outputs X (B,T,J,2), y (B,T,J,3). */
int mp_gather_windows(const float* poses_2d, const float* poses_3d, const int64_t* seq_offset, int S, const int32_t* win_seq,
                      const int32_t* win_start, const uint8_t* win_flip, const int32_t* mirror, const float* mask2d, const float* noise2d,
                      int B, int T, int J, float* X, float* y, void* stream);

/* Sequence lifting: one 3-D pose per frame of whole 2-D keypoint sequences - the reference's lift_action (hpe/eval_utils.py:226-253, used by
 * hpe/viz.py:84-91): windows with drop_last=False replicate padding (hpe/mh_so3_hpe/data/generators.py:93-104,135-154), the flip-TTA evaluation
 * loop (eval_utils.py:84-142), predictions flattened to (windows * T, 17, 3) or, with return_hyps, (windows * T, K, 17, 4) with the score in the
 * fourth channel.  Here the windows may also overlap (stride < T).
 * mp_lift_windows_2d: mp_gather_windows for sequences that have no 3-D side - X (B,T,J,2) only, same tables, flags and padding.
 * mp_lift_merge: the output side in one pass.  poses (F*W, K, T, J, 3) and scores (F*W, K, T[, 1]) as mp_model_forward leaves them (scores may be
 * null when K == 1); F = 2 with tta != 0: windows W .. 2W-1 are the mirrored copies of windows 0 .. W-1.  win_seq / win_start (W) device int32 and
 * seq_offset (S+1) device int64 as for mp_gather_windows; h_win_seq / h_win_start / h_seq_offset: HOST copies of the three tables, checked before
 * anything is launched - windows sorted by sequence and then by start, every window starting inside its sequence, every frame of every sequence
 * covered by a window (otherwise MP_ERR_ARG; a seq_offset that describes the padded lengths keeps the padded frames).  mirror (J) HOST int32.
 * Per output frame f, over the windows w that cover it (win_start <= f < win_start + T), in increasing w:
 *   p_w = sum_k score * pose (agg 0, "weighted_ave") or the pose of the first maximal score (agg 1, "best_score"; mp_aggregate's tie rule);
 *   with tta, p_w = (p_w(window w) + unflip(p_w(window W + w))) / 2, unflip = x negated and joint j read from mirror[j], the mirrored half
 *   aggregated with its own scores;
 *   blend 0 "mean": out = mean of p_w; blend 1 "center": p_w of the window whose centre frame win_start + (T-1)/2 is nearest to f (the lower w on a
 *   tie), no averaging.
 * out (Ntot, J, 3) = scale * that (scale 1: metres).  hyps (Ntot, K, J, 4) or null: every hypothesis (times scale) and its score (never scaled) of
 * the un-mirrored windows, blended over the windows by the same rule.  Gather, fixed summation order, no atomics: identical bits on every call. */
int mp_lift_windows_2d(const float* poses_2d, const int64_t* seq_offset, int S, const int32_t* win_seq, const int32_t* win_start,
                       const uint8_t* win_flip, const int32_t* mirror, int B, int T, int J, float* X, void* stream);
int mp_lift_merge(const float* poses, const float* scores, int W, int K, int T, int J, int tta, const int32_t* win_seq,
                  const int32_t* win_start, const int64_t* seq_offset, int S, const int32_t* h_win_seq, const int32_t* h_win_start,
                  const int64_t* h_seq_offset, const int32_t* mirror, int agg, int blend, float scale, float* out, float* hyps,
                  void* stream);

/* Rigid lifting: one skeleton per lifted sequence.  The model's hypotheses of a window share their bone lengths; what mp_lift_merge emits does not
 * (weighted_ave averages poses that differ in rotation, blend "mean" averages windows whose lengths differ, and every window predicts its own
 * lengths), so a lifted sequence has a non-zero MPSCE (segments_time_consistency, hpe/mh_so3_hpe/metrics/regularizations.py:8-60).  The reference
 * has no counterpart (hpe/viz.py renders the hypotheses as they come).  parents (J) HOST int32: parents[0] = -1, 0 <= parents[j] < j (parents
 * precede their children), 2 <= J <= 32, otherwise MP_ERR_ARG before anything is launched; bone b = j - 1 joins joint j to parents[j]
 * (Skeleton.bones order, the layout of the model's (B, 16) lengths).
 * mp_lift_rigid: poses (Ntot, inner, J, C) device floats, C = 3 (poses) or 4 (hypotheses; channel 3, the score, is neither read nor written),
 * updated IN PLACE; seq_offset (S + 1) device int64 as for mp_lift_merge: frame g belongs to the last sequence s with seq_offset[s] <= g and is
 * re-assembled with row s of lengths (S, J - 1) device floats.  Per pose p, in fp32:  q[0] = p[0];  for j = 1 .. J-1:  d = p[j] - p[parents[j]]
 * (the INPUT positions), n = sqrtf(d . d), u = d / n if n > 0 and finite, otherwise the u of the bone of parents[j] ((0, 0, 1) when parents[j] is
 * the root);  q[j] = q[parents[j]] + lengths[s][j-1] u.  sqrtf and the division are correctly rounded.  One lane owns one pose and holds it in
 * registers, so nothing it stores is read again.
 * mp_bone_length_means: lengths (S, J - 1) = per sequence the mean over its frames of the bone lengths of poses (Ntot, J, 3); seq_real (S) device
 * int64 or null: only the first min(seq_real[s], frames of s) frames of sequence s count (a sequence kept with its replicate-padded frames);
 * a sequence without frames gets lengths 0, and no frame at or beyond Ntot is read whatever the device tables say.
 * Differences, square roots and sums in fp64, rounded to fp32 once; one workgroup per sequence, fixed summation order, no atomics: identical bits
 * on every call.  Neither call synchronises. */
int mp_lift_rigid(float* poses, int64_t Ntot, int inner, int J, int C, const int64_t* seq_offset, int S, const float* lengths,
                  const int32_t* parents, void* stream);
int mp_bone_length_means(const float* poses, int64_t Ntot, int J, const int64_t* seq_offset, const int64_t* seq_real, int S, const int32_t* parents,
                         float* lengths, void* stream);

/* Placing lifted sequences in the scene.  What mp_lift_merge / mp_lift_rigid leave is root-relative and in the camera's frame; the reference's
 * consumer of lift_action rotates it into the world and puts it on the floor first (hpe/viz.py:93-98: camera_to_world(prediction, R, t = 0), then
 * z -= min z), and its data/camera.py ships the H36M camera model (project_to_2d).  Conventions of mp_lift_rigid: poses (Ntot, inner, J, C) device
 * floats, C = 3 or 4 (channel 3, a hypothesis' score, is neither read nor written), 2 <= J <= 32, seq_offset (S + 1) device int64: frame g belongs
 * to the last sequence s with seq_offset[s] <= g; one lane owns one pose.  All arithmetic between the float32 loads and the float32 stores is fp64.
 * A null pointer, C outside {3, 4}, J outside 2..32, Ntot / inner / S <= 0 or S > Ntot, or more poses than one grid holds: MP_ERR_ARG before
 * anything is launched.  Neither call synchronises.
 * mp_lift_place (poses read only): per pose the root translation t that fits the 2-D keypoints kp (Ntot, J, 2) of its frame (normalised screen
 * coordinates, shared by the frame's `inner` poses) under the pinhole part of the camera intr (S, 9) = (fx, fy, cx, cy, k1, k2, k3, p1, p2) of its
 * sequence, and the reprojection error of the placed pose.  weights (J) device floats or null (all ones); a joint of weight 0 is skipped.  With
 * a_j = (u_j - cx) / fx, b_j = (v_j - cy) / fy, ex_j = X_j - a_j Z_j, ey_j = Y_j - b_j Z_j, t minimises
 * sum_j w_j [(ex_j + tx - a_j tz)^2 + (ey_j + ty - b_j tz)^2]: with W = sum w, A = sum w a, B = sum w b, Q = sum w (a^2 + b^2) (sums in joint order)
 *   [[W, 0, -A], [0, W, -B], [-A, -B, Q]] t = [-sum w ex, -sum w ey, sum w (a ex + b ey)],
 * solved as  D = W Q - A^2 - B^2,  tz = (W sum w (a ex + b ey) - A sum w ex - B sum w ey) / D,  tx = (A tz - sum w ex) / W,  ty = (B tz - sum w ey) / W.
 * reproj = sum_j w_j d_j / W, d_j the distance between (u_j, v_j) and pi(P_j), P_j = (X_j, Y_j, Z_j) + t; distort = 1: pi is project_to_2d
 * (XX = clamp(P.xy / P.z, -1, 1), r2 = |XX|^2, XXX = XX (1 + k1 r2 + k2 r2^2 + k3 r2^3 + p . XX) + p r2, pi = f XXX + c); distort = 0: pi is
 * project_to_2d_linear (f XX + c, the clamp included).  Normalised screen units: times res_w / 2 gives pixels.
 * traj (Ntot, inner, 3) and reproj (Ntot, inner) floats, ok (Ntot, inner) bytes.  ok = 0 with t = (0, 0, 0) and reproj = 0: W <= 0, a non-finite sum,
 * or D <= 1e-9 W Q (D / (W Q) lies in [0, 1]; 0: all weighted keypoints coincide).  ok = 0 with t and reproj stored as computed: a weighted joint
 * with Z_j + tz <= 0.  Otherwise ok = 1.  A pose's result depends on no other pose.
 * The call is mp_lift_place_refine (below) with start = start_ok = steps = null and iters = 0: one kernel serves both.
 * mp_lift_world (poses updated IN PLACE): every joint p <- qrot(q_s, p + traj) + trans_s,  qrot(q, v) = v + 2 (w (q_xyz x v) + q_xyz x (q_xyz x v))
 * (the reference's qrot, data/quaternion.py:6-20: q is not normalised); quat (S, 4) = (w, x, y, z); traj (Ntot, inner, 3) or null, trans (S, 3) or
 * null: with both null this is camera_to_world(., R, t = 0).  floor_mode 0: nothing more.  1: after the float32 results are stored, floor[s] (S floats,
 * written) = the minimum stored z over every frame, inner index and joint of sequence s (fminf: a NaN is passed over), and every z of the sequence
 * becomes the ONE float32 difference z - floor[s]; scratch holds at least S * MP_LIFT_WORLD_SHARES floats (one partial minimum per workgroup, merged
 * in a fixed order; no atomics: identical bits on every call).  2: z - floor[s] with the caller's floor (read; scratch may be null). */
#define MP_LIFT_WORLD_SHARES 16
int mp_lift_place(const float* poses, int64_t Ntot, int inner, int J, int C, const float* kp, const int64_t* seq_offset, int S, const float* intr,
                  const float* weights, int distort, float* traj, float* reproj, uint8_t* ok, void* stream);
int mp_lift_world(float* poses, int64_t Ntot, int inner, int J, int C, const float* traj, const int64_t* seq_offset, int S, const float* quat,
                  const float* trans, int floor_mode, float* floor, float* scratch, int64_t scratch_floats, void* stream);

/* Refining placed root trajectories under the FULL camera model.  mp_lift_place fits t with the pinhole part of the camera (linear in t) and
 * measures the error with the full one; mp_lift_place_refine starts from that fit, or from a given trajectory, and takes up to `iters` undamped
 * Gauss-Newton steps on  F(t) = sum_j w_j |pi(p_j + t) - u_j|^2,  pi as for mp_lift_place by `distort`.  The reference has no counterpart.  The
 * conventions, checks and MP_ERR_ARG cases of mp_lift_place apply (poses read only); in addition 0 <= iters <= MP_LIFT_REFINE_MAXITERS, start
 * (Ntot, inner, 3) device floats or null, start_ok (Ntot, inner) device bytes or null (it needs start), steps (Ntot, inner) device bytes or null.
 * Per pose, in fp64 between the float32 loads and stores, joints of weight 0 never looked at, every sum in joint order:
 * 1. Start.  start null: t, ok and the degenerate rule of mp_lift_place (ok = 0, t = 0, reproj = 0, steps = 0 for a degenerate fit).  start given:
 *    t = start[i]; if start_ok[i] == 0, t is not finite or sum w is not > 0: t is stored as it came in, bit for bit, reproj = 0, ok = 0, steps = 0.
 * 2. Evaluation at t, one pass over the joints:  P = p_j + t,  q = P.xy / P.z,  x = clamp(q, -1, 1),  s_x, s_y = 1 where -1 <= q <= 1 else 0 (the
 *    derivative of the clamp),  r_j = pi(P) - u_j,  and the 2 x 3 Jacobian  J_j = diag(f) d(px, py)/d(x, y) d(x, y)/dt  with
 *    dx/dt = s_x (1/Z, 0, -q_x/Z),  dy/dt = s_y (0, 1/Z, -q_y/Z);  distort = 0: d(px, py)/d(x, y) is the identity;  distort = 1: with m the bracket
 *    of project_to_2d,  dm = k1 + 2 k2 r2 + 3 k3 r2^2,  m_x = 2 x dm + p1,  m_y = 2 y dm + p2:
 *    dpx/dx = m + x m_x + 2 p1 x,  dpx/dy = x m_y + 2 p1 y,  dpy/dx = y m_x + 2 p2 x,  dpy/dy = m + y m_y + 2 p2 y.
 *    Sums:  F = sum w |r|^2,  E = sum w |r|,  W = sum w,  H = sum w J^T J,  g = sum w J^T r,  deep = every weighted Z > 0.
 * 3. Steps.  If the first evaluation has deep false or F not finite: ok = 0, t and E / W stored as computed, no step (mp_lift_place's rule for a
 *    joint behind the camera).  Otherwise for k = 1 .. iters:  det H by cofactors,  d = -adj(H) g / det;  the step is taken iff det and
 *    H00 H11 H22 are finite,  det > 1e-12 H00 H11 H22  (the ratio lies in [0, 1] for a positive semi-definite H),  t' = t + d is finite, the
 *    evaluation at t' has deep true, and  F' <= (1 + 1e-6) F.  On the first step not taken the iteration ends and t stays.  No convergence test
 *    and no damping: the start lies centimetres from the minimum, where Gauss-Newton converges in about three steps; the 1e-6 slack keeps
 *    rounding from deciding at the minimum, where F' / F is 1.
 * 4. Store.  traj = (float) t,  reproj = (float)(E / W) at the final t,  ok = 1,  steps = steps taken.
 * iters = 0 with start null IS mp_lift_place: that entry point makes exactly this call (steps null), so the two share every bit by construction.
 * iters = 0 with start given: the reprojection error of a given trajectory.
 * One lane owns one pose and a pose depends on no other pose; no atomics: identical bits on every call.  The call does not synchronise. */
#define MP_LIFT_REFINE_MAXITERS 16
int mp_lift_place_refine(const float* poses, int64_t Ntot, int inner, int J, int C, const float* kp, const int64_t* seq_offset, int S, const float* intr,
                         const float* weights, int distort, const float* start, const uint8_t* start_ok, int iters, float* traj, float* reproj,
                         uint8_t* ok, uint8_t* steps, void* stream);

/* Joint rotations of lifted poses: the inverse of the decoder's forward kinematics on the poses the pipeline emits.  The reference has no
 * counterpart.  poses (Ntot, inner, J, C) device floats, read only, C = 3 or 4 (channel 3 is not read), 2 <= J <= 32; seq_offset (S + 1) device
 * int64 (read by MP_LIFT_ROT_CONTINUOUS alone, every sequence's frames clamped to 0 .. Ntot-1); parents (J) HOST int32, parents[0] = -1,
 * 0 <= parents[j] < j; rest (J, 3) HOST floats, row j >= 1 the T-pose direction of the bone parents[j] -> j (the skeleton's t_pose_operators),
 * normalised here in fp64, row 0 ignored; a zero or non-finite row is MP_ERR_ARG.  Outputs: quat (Ntot, inner, J, 4) device floats (w, x, y, z),
 * 16-byte aligned; rot6d (Ntot, inner, J, 6) device floats or null: columns 0 then 1 of the matrix of q[j] (fp64 q), what mp_fk_decode_fwd takes;
 * ok (Ntot, inner) device bytes; a zero component of q[j] or rot6d is stored as +0.  The FK convention is the decoder's: Rw[0] = R[0], Rw[j] = Rw[parent] R[j], p[j] = p[parent] + Rw[j] (len_j
 * rest_j), so fk(q, measured lengths) is the pose again.  Per pose, on its own, fp64 between the float32 loads and stores:
 * 1. Bones.  b_j = p_j - p_parent is GOOD if its six coordinates are finite and |b_j| > 1e-12; then d_j = b_j / |b_j|.  If any coordinate of the
 *    pose is not finite: every quaternion is (1, 0, 0, 0) and ok = 0.
 * 2. Reference children of the root, chosen on the host: a = the lowest child of joint 0, b = the lowest child of joint 0 with
 *    |rest_a x rest_b| > 1e-6, or none (H36M: a = 1, the right hip, +x; b = 7, the spine, +y).
 * 3. Root.  E = [e1, e2, e1 x e2], e1 = rest_a, e2 = unit(rest_b - (rest_b . e1) e1); F the same frame of d_a, d_b; Rw[0] = F E^T.  Fallbacks with
 *    ok = 0: d_b not good or |d_b - (d_b . f1) f1| <= 1e-9: Rw[0] = arc(rest_a -> d_a); d_a not good either: identity.  No b: arc(rest_a -> d_a),
 *    ok untouched.  q[0] is the unit quaternion of Rw[0], taken from the largest of 4w^2 = 1 + tr, 4x^2 = 1 + m00 - m11 - m22, 4y^2, 4z^2 (the
 *    first on a tie), normalised, with the sign that makes its first non-zero component positive.
 * 4. Joints j = 1 .. J-1:  u = Rw[parent]^T d_j,  q[j] = arc(rest_j -> u),  Rw[j] = Rw[parent] q[j];  arc(r -> u) = normalize(1 + r . u, r x u),
 *    the shortest, twist-free rotation; where 1 + r . u < 1e-12 it is the half turn (0, n), n = unit(e_k - (e_k . r) r), k the coordinate where
 *    |r| is smallest (the lowest on a tie), n's first non-zero component positive, and ok = 0.  A bone that is not good: q[j] = (1, 0, 0, 0),
 *    ok = 0.
 * 5. MP_LIFT_ROT_CONTINUOUS, per (sequence, inner index, joint) over the sequence's frames f0 .. f1-1: with c[g] the float32 quaternion as stored
 *    by 1-4, flip[f0] = 0, flip[g] = flip[g-1] XOR (dot(c[g], c[g-1]) < 0) (the dot in fp64), and -c[g] is stored where flip[g]; rot6d is
 *    not touched, a frame no sequence holds keeps c[g].  An exclusive-or prefix over integer flags: the result does not depend on how the frames
 *    are cut into chunks.
 * The twist about a bone is zero by construction: a convention, not a measurement.  No atomics, a fixed order: identical bits on every call; a
 * pose's result of 1-4 depends on no other pose, a sequence's signs on no other sequence.  The call does not synchronise. */
#define MP_LIFT_ROT_CONTINUOUS 1
int mp_lift_rotations(const float* poses, int64_t Ntot, int inner, int J, int C, const int64_t* seq_offset, int S, const int32_t* parents,
                      const float* rest, int flags, float* quat, float* rot6d, uint8_t* ok, void* stream);

/* Smoothing lifted sequences in time: a weighted local polynomial fit (Savitzky-Golay with validity weights) along the frames of a sequence, which
 * also fills frames that have no valid value of their own.  The reference has no counterpart.  in / out (Ntot, inner, M, C) device floats, out of
 * place; C = 3 or 4, 1 <= M <= 32 (M = 1, C = 3: a trajectory; M = J: poses or hypotheses); valid and filled (Ntot, inner) device bytes, either may
 * be null (null valid: every frame is valid); seq_offset (S + 1) device int64 as for mp_lift_rigid, its entries clamped to 0 .. Ntot.
 * Per frame g of sequence s = frames [f0, f1), inner index i, with radius R, degree deg, taper:
 *   taps tau in [-R, R] with f0 <= g + tau < f1 (a window never crosses a sequence boundary and is never padded);
 *   w_tau = k(tau) [valid[g + tau, i] != 0],  k = 1 (taper 0, "uniform") or (1 - (tau / (R + 1))^2)^2 (taper 1, "biweight");
 *   n = taps with w_tau > 0.  n = 0: every float of the frame is copied bit for bit and filled = 0; otherwise filled = 1 and
 *   d = min(deg, n - 1), or d = 0 when no valid tap has tau <= 0 or none has tau >= 0 (not bracketed: held constant, never extrapolated);
 *   u_tau = tau / R;  for each channel c < 3 of each of the M items out = p(0), p the polynomial of degree d that minimises
 *   sum_tau w_tau (p(u_tau) - y_tau)^2:  out = sum_tau c_tau y_tau,  c_tau = w_tau (a0 + a1 u_tau + a2 u_tau^2),  (a0, a1, a2) the first row of
 *   the inverse of the (d + 1) x (d + 1) normal matrix [sum w u^(j+k)].  c_tau is computed once per (g, i) and shared by the M x 3 channels.
 *   Channel 3 of C = 4 (a hypothesis' score) is copied bit for bit.
 * All arithmetic between the float32 loads and the one float32 store is fp64; sums run over the valid taps in increasing tau; no atomics: identical
 * bits on every call.  A non-finite value on a valid tap gives IEEE results in the windows that hold it; an invalid tap's value is never looked at.
 * MP_ERR_ARG before anything is launched: in, out or seq_offset null; in and out overlapping; radius outside 1..MP_LIFT_SMOOTH_MAXR, degree outside
 * 0..2, taper outside 0..1; M outside 1..32, C outside {3, 4}; Ntot, inner or S <= 0, S > Ntot; more work than one grid holds.  The call does not
 * synchronise. */
#define MP_LIFT_SMOOTH_MAXR 64
int mp_lift_smooth(const float* in, float* out, int64_t Ntot, int inner, int M, int C, const uint8_t* valid, const int64_t* seq_offset, int S,
                   int radius, int degree, int taper, uint8_t* filled, void* stream);

/* Lifting a sequence along ONE hypothesis path: per frame exactly one of the model's K hypotheses, chosen jointly over the whole sequence - the
 * maximum a posteriori path of a hidden Markov model whose states are the hypotheses, found with the Viterbi algorithm.  Nothing is averaged (every
 * emitted pose is one the model made, on its manifold) and nothing is chosen frame by frame (mp_lift_merge's "best_score" jumps from head to head
 * whenever two scores cross).  The reference has no counterpart: its aggregate is per frame.
 * hyps (Ntot, K, J, 4) device floats as mp_lift_merge emits them: xyz in the poses' unit, the hypothesis' score replicated in channel 3 (read from
 * joint 0); 1 <= K <= 8, 2 <= J <= 32; seq_offset (S + 1) device int64 as for mp_lift_rigid, its entries clamped to 0 .. Ntot.  Everything between
 * the float32 loads and the stores is fp64.  Per sequence with frames [f0, f1):
 *   unary cost       U[g][k] = -log(s), s the score of (g, k); a score that is not > 1e-12 (zero, negative, NaN) is taken as 1e-12;
 *   transition cost  for g > f0, from state a at g - 1 to state b at g:
 *                    D[g][a][b] = (1 / (2 sigma^2)) ((sum_j |x[g][b][j] - x[g-1][a][j]|^2) / J) + (a != b ? switch_cost : 0),
 *                    the sum in joint order, then channel order; sigma > 0 in the poses' unit (+inf: the factor is exactly 0), switch_cost >= 0 and
 *                    finite; a transition cost that is not finite (a NaN coordinate) is taken as 1e30;
 *   forward pass     f[f0][k] = U[f0][k];  f[g][b] = min_a (f[g-1][a] + D[g][a][b]) + U[g][b], the back-pointer the FIRST (lowest) arg-min a;
 *   end, backtrack   the last frame takes the first arg-min of f[f1-1][.], the frames before it follow the back-pointers.
 * path (Ntot) bytes: the chosen hypothesis of every frame; out (Ntot, J, 3) or null: out[g] = hyps[g][path[g]][:, :3], copied bit for bit; cost (S)
 * doubles or null: f at the chosen end state.  A sequence of one frame takes the first arg-min of its unary costs; an empty clamped range writes
 * cost[s] = 0 and nothing else; a frame that no sequence's clamped range holds is not written.  hyps is not modified.
 * scratch: at least mp_lift_path_scratch_floats(Ntot, K) floats = Ntot (8 K^2 + 9 K) bytes (D, U and the back-pointers), 8-byte aligned.  The backtrack
 * walks the back-pointers out of LDS, MP_LIFT_PATH_CHUNK frames at a time.  No atomics, fixed order of operations: identical bits on every call, and a
 * sequence's results do not depend on the other sequences of the call.
 * MP_ERR_ARG before anything is launched: hyps, path, seq_offset or scratch null; K outside 1..8; J outside 2..32; Ntot or S <= 0, S > Ntot; sigma not
 * > 0; switch_cost negative or not finite; scratch too small or misaligned.  The call does not synchronise. */
#define MP_LIFT_PATH_CHUNK 512
int64_t mp_lift_path_scratch_floats(int64_t Ntot, int K);
int mp_lift_path(const float* hyps, int64_t Ntot, int K, int J, const int64_t* seq_offset, int S, float sigma, float switch_cost, uint8_t* path,
                 float* out, double* cost, float* scratch, int64_t scratch_floats, void* stream);

/* Scoring a lift against ground truth, per sequence: what the lifting stages emit (merged, smoothed, re-assembled or selected poses, hypotheses,
 * fitted trajectories) held against the 3-D sequences of the dataset - the sums behind MPJPE, its root mean square, the velocity and acceleration
 * errors, P-MPJPE (the reference's p_mpjpe, hpe/mh_so3_hpe/metrics/mean_joint_errors.py:148-189), per-joint errors and bone-length statistics.  The
 * evaluation loop (mp_pose_metrics) scores windows per batch item; this scores sequences of any length, never across a sequence boundary.
 * pred (Ntot, inner, M, C) device floats, C = 3 or 4 (channel 3, a hypothesis' score, is not read); gt (Ntot, M, 3), shared by the inner poses of a
 * frame; valid (Ntot, inner) bytes or null (every frame is valid); seq_offset (S + 1) device int64 as for mp_lift_rigid, its entries clamped to
 * 0 .. Ntot; parents (M) HOST ints, parents[0] = -1 and parents before children, or null (no bone statistics); 1 <= M <= 32 (M = 1: a root
 * trajectory); pred_scale, gt_scale finite and > 0; flags: bit 0 = root-relative, bit 1 = Procrustes (needs M >= 3).  Everything between the float32
 * loads and the stores is fp64, without contraction into fused multiply-adds.  For one sequence with frames [f0, f1) and one inner index i:
 *   P[g][j] = pred_scale * (double)pred, G[g][j] = gt_scale * (double)gt; with bit 0, joint 0 of the same pose is subtracted from every joint of P,
 *   and likewise of G;
 *   a frame is COUNTED if valid is null or non-zero there and all 3 M coordinates of P and of G are finite; a frame that is not counted contributes
 *   to nothing, and its frame_err is -1;
 *   e[g][j] = sqrt(|P[g][j] - G[g][j]|^2), the squares added in channel order;  frame_err[g][i] = (float)(sum_j e[g][j] / M), j in order.
 * rows (S, inner, mp_lift_score_row_doubles(M)) doubles:
 *   [0] counted frames   [1] sum_g sum_j e   [2] sum_g sum_j e^2
 *   [3] pairs (g-1, g), both in the sequence and counted   [4] over them sum_j |(P[g] - P[g-1]) - (G[g] - G[g-1])|
 *   [5] triples (g-2, g-1, g), all in the sequence and counted   [6] over them sum_j |(P[g] - 2 P[g-1] + P[g-2]) - (G[g] - 2 G[g-1] + G[g-2])|
 *   [7] bit 1: sum_g sum_j of the error after the similarity alignment (scale, proper rotation, translation) of P[g] onto G[g], else 0: Horn's closed
 *       form as in mp_procrustes_errors, in fp64, the cyclic Jacobi sweeps run until the off-diagonal mass is at most 2^-52 times the matrix norm
 *       (30 sweeps at most)
 *   [8] counted frames the alignment skipped (the centred P or the centred G has zero squared norm); they add nothing to [7]
 *   [9, 9 + M) per joint sum_g e[g][j]
 *   [9 + M + 3 (b - 1) + {0, 1, 2}], b = 1 .. M - 1, with L = |P[b] - P[parents[b]]| and LG likewise of G: sum L, sum L^2, sum |LG - L|; zeros with
 *       null parents.
 * A velocity or acceleration term never crosses a sequence boundary; a sequence whose clamped range is empty gets an all-zero row.  frame_err
 * (Ntot, inner) floats or null; a frame that no sequence's clamped range holds is not written.
 * Schedule: MP_LIFT_SCORE_SHARES workgroups per (sequence, inner), each on a contiguous slice of the sequence's own range (a whole number of tiles),
 * each writing one partial row to scratch (the alignment, one lane per pose, in a kernel of its own on the same slices); a last kernel adds the shares
 * in share order.  No atomics; the order of every sum depends on the
 * sequence's own frames only: identical bits on every call, and a sequence scored alone has the bits it has in a call with others.
 * scratch: at least mp_lift_score_scratch_doubles(S, inner, M) doubles = S inner MP_LIFT_SCORE_SHARES row doubles, 8-byte aligned.
 * MP_ERR_ARG before anything is launched: pred, gt, seq_offset, rows or scratch null; C not 3 or 4; M outside 1..32; Procrustes with M < 3; Ntot,
 * inner or S <= 0, S > Ntot; flags outside 0..3; a scale that is not finite and > 0; a parent table that breaks the order; scratch too small or
 * misaligned.  The call does not synchronise. */
#define MP_LIFT_SCORE_SHARES 32
int mp_lift_score_row_doubles(int M);                    /* 9 + M + 3 (M - 1) */
int64_t mp_lift_score_scratch_doubles(int S, int inner, int M);
int mp_lift_score(const float* pred, int64_t Ntot, int inner, int M, int C, const float* gt, const uint8_t* valid, const int64_t* seq_offset, int S,
                  const int32_t* parents, double pred_scale, double gt_scale, int flags, double* rows, float* frame_err, double* scratch,
                  int64_t scratch_doubles, void* stream);

/* Fusing the camera views of a take: Human3.6M records every motion with four calibrated cameras at once, and a second camera sees the first one's
 * depth axis as an image axis - the views resolve each other's ambiguity, in the choice of a hypothesis and in the depth of the root.  The reference
 * has no counterpart.  A TAKE is a group of up to V views of one motion, 1 <= V <= MP_LIFT_FUSE_MAXV, all with the same number of frames; the views
 * of all takes lie side by side: a per-view array is (V, Ftot, ...), Ftot the sum of the takes' frame counts.  take_offset (G + 1) device int64 is
 * used like seq_offset (frame f belongs to the last take g with take_offset[g] <= f; entries clamped to 0 .. Ftot).  valid (V, Ftot) device bytes
 * or null (every view is valid): a take with fewer than V views marks the missing ones 0 in all of its frames; an invalid view's data is never
 * looked at.  Per-take camera tables, device floats: quat (G, V, 4) = (w, x, y, z), trans (G, V, 3), intr (G, V, 9) as for mp_lift_place.  A view
 * whose |q|^2 is not finite or < 1e-12 counts as invalid in every frame of its take.  R is the rotation matrix of q / |q|, normalised in fp64
 * (mp_lift_world keeps the dataset's quaternion un-normalised, as the reference's qrot does; H36M's are unit to 6e-8); camera to world is
 * x_world = R x_cam + T.  quat null: R is the identity, nothing is multiplied and the differences are exact.  Everything between the float32 loads
 * and the float32 stores is fp64; no atomics, fixed orders: identical bits on every call; a frame's result depends on no other frame; neither
 * call synchronises.
 * mp_lift_fuse: hyps (V, Ftot, K, J, C) read only, 1 <= K <= MP_LIFT_FUSE_MAXK, 2 <= J <= 32, C = 3 or 4 (channel 3 of joint 0: the hypothesis'
 * score; C = 3: every unary cost is 0); sigma > 0 in the poses' unit (+inf: the pair factor is exactly 0); score_weight >= 0 and finite.  Per
 * frame f of take g:
 * 1. Rotate.  w[v][k][j] = R_gv (x[v][f][k][j] - x[v][f][k][0]): root-relative, placed or floored poses may be passed.
 * 2. Pair cost, views a < b:  d(a, i; b, l) = (sum_j |w[a][i][j] - w[b][l][j]|^2) / J, the sum in joint order, then channel order; a d that is not
 *    finite is taken as 1e30.
 * 3. Unary cost.  u(v, k) = -log(s); an s that is not > 1e-12 is taken as 1e-12 (mp_lift_path's rule).
 * 4. Combinations c = (k_v) over the frame's valid views:  E(c) = (1 / (2 sigma^2)) sum_{a < b valid} d(a, k_a; b, k_b) + score_weight sum_{v valid}
 *    u(v, k_v), the pairs in lexicographic order of (a, b), then the unary terms in view order.  The choice is the FIRST minimum in lexicographic
 *    order of c, view 0 most significant (at most 8^4 = 4096 combinations).
 * 5. pose[f][j] = (sum_{v valid} w[v][k_v][j]) / n in view order, n the number of valid views; joint 0 is stored as +0.
 * 6. spread[f] = sqrt(sum_v sum_j |w[v][k_v][j] - pose64[f][j]|^2 / (n J)), in the poses' unit: how well the views agree.
 * 7. cost[f] = E;  choice[f][v] = k_v, 255 for an invalid view;  ok[f] = 1, 0 if E >= 1e30.  n = 0: pose 0, every choice 255, cost = spread = 0, ok = 0.
 * pose (Ftot, J, 3) floats, root-relative in the world's orientation; choice (Ftot, V) bytes; cost, spread (Ftot) floats; ok (Ftot) bytes.
 * MP_ERR_ARG before anything is launched: hyps, take_offset or an output null; V, K, J or C out of range; Ftot or G <= 0, G > Ftot; sigma not > 0;
 * score_weight negative or not finite; more frames than one grid holds.
 * mp_lift_fuse_place: ONE world root per frame from all views.  pose (Ftot, J, 3) as mp_lift_fuse wrote it, kp (V, Ftot, J, 2) normalised screen
 * coordinates, weights (J) or null, distort and 0 <= iters <= MP_LIFT_REFINE_MAXITERS as for mp_lift_place_refine.  Joint j seen by view v with the
 * root at r is the camera-space point P = R^T (pose_j + r - T_v).
 * 1. Start, linear under the pinhole part: with a, b as for mp_lift_place and rho_x, rho_y, rho_z the rows of R^T,  m_x = rho_x - a rho_z,
 *    m_y = rho_y - b rho_z,  H = sum_v sum_j w_j (m_x m_x^T + m_y m_y^T),  h = sum w_j (m_x (m_x . (T_v - pose_j)) + m_y (m_y . (T_v - pose_j))),
 *    over the valid views in order, then the joints in order, a joint of weight 0 skipped;  r = adj(H) h / det by cofactors.  Degenerate - no valid
 *    view, sum w not > 0, a non-finite sum, det not > 1e-12 H00 H11 H22, r not finite:  ok = 0, root = 0, reproj = 0, steps = 0.
 * 2. Evaluation and steps: steps 2 to 4 of mp_lift_place_refine with F, E, W, H, g and deep summed over the valid views, then the joints; the
 *    Jacobian with respect to r is J_j R^T; the acceptance rule and its constants are the same; deep asks every weighted joint of every valid view
 *    to lie in front of its camera.
 * 3. root (Ftot, 3) floats;  reproj (V, Ftot) floats: view v's own E_v / W_v at the final r (its weighted mean distance, as mp_lift_place_refine's
 *    reproj), 0 for an invalid view;  ok (Ftot) bytes;  steps (Ftot) bytes or null.
 * One lane owns one frame.  MP_ERR_ARG: those of mp_lift_place_refine, and pose, kp, take_offset, trans or intr null, V outside 1..4, G out of range. */
#define MP_LIFT_FUSE_MAXV 4
#define MP_LIFT_FUSE_MAXK 8
int mp_lift_fuse(const float* hyps, int V, int64_t Ftot, int K, int J, int C, const uint8_t* valid, const int64_t* take_offset, int G, const float* quat,
                 float sigma, float score_weight, float* pose, uint8_t* choice, float* cost, float* spread, uint8_t* ok, void* stream);
int mp_lift_fuse_place(const float* pose, const float* kp, int V, int64_t Ftot, int J, const uint8_t* valid, const int64_t* take_offset, int G,
                       const float* quat, const float* trans, const float* intr, const float* weights, int distort, int iters, float* root,
                       float* reproj, uint8_t* ok, uint8_t* steps, void* stream);

/* Fusing the views of a take ALONG TIME: one hypothesis per view and frame, chosen jointly over the views AND over the whole take.  mp_lift_fuse
 * decides every frame on its own, so an ambiguity that all views share - a left/right-mirrored body is consistent in every camera, the pair cost
 * cannot reject it - is taken in every frame where its score happens to be higher, and the fused motion flickers; mp_lift_path removes that
 * flicker for one view.  This is the Viterbi path over the COMBINATIONS of a take: K^V states, at most 4096.  The conventions are mp_lift_fuse's:
 * takes, take_offset (entries clamped to 0 .. Ftot), valid, quat and its fp64 normalisation, a view with a zero quaternion counts as invalid;
 * fp64 between the float32 loads and the float32 stores, without contraction into fused multiply-adds; no atomics, fixed orders: identical bits
 * on every call; a take's result does not depend on the other takes of the call; the call does not synchronise.  Not measured on real data.
 * hyps (V, Ftot, K, J, C) read only, 1 <= V <= MP_LIFT_FUSE_MAXV, 1 <= K <= MP_LIFT_FUSE_MAXK, 2 <= J <= 32, C = 3 or 4; sigma and score_weight as
 * for mp_lift_fuse; path_sigma > 0 in the poses' unit (+inf: the motion factor is exactly 0); switch_cost >= 0 and finite.
 * A STATE is c = (k_0 .. k_{V-1}), every view a digit 0 .. K - 1, view 0 most significant; it always has V digits.  For frame g of a take with
 * frames [f0, f1):
 * 1. w, d(a, i; b, l), u(v, k): exactly steps 1 to 3 of mp_lift_fuse (for C = 3, u = 0).
 * 2. Frame cost  E_g(c) = (1 / (2 sigma^2)) sum_{a < b valid at g} d(a, k_a; b, k_b) + score_weight sum_{v valid at g} u(v, k_v), step 4 of
 *    mp_lift_fuse with its order of additions.  A view invalid at g contributes nothing: its digit is free.  No valid view: E_g = 0.
 * 3. Transition of view v from a at g - 1 to b at g:
 *    t_v(g; a -> b) = (1 / (2 path_sigma^2)) ((sum_j |w[v][g][b][j] - w[v][g-1][a][j]|^2) / J) + (a != b ? switch_cost : 0), the sum in joint
 *    order, then channel order; a value that is not finite is taken as 1e30; if view v is invalid at g or at g - 1, t_v = 0 for every (a, b): a
 *    view's chain is cut across a gap.
 * 4. Forward pass, STAGED per view (the transition is a sum over the views; the staged order of additions is the definition):
 *    f[f0][c] = E_f0(c);  for g > f0:  h_0 = f[g-1];  for v = 0 .. V - 1:  h_{v+1}[c with digit v = b] = min_a (h_v[c with digit v = a] +
 *    t_v(g; a -> b)), the back-pointer digit bp_v[g][c] the FIRST (lowest) arg-min a;  f[g][c] = h_V[c] + E_g(c).  This is min over all
 *    predecessor states of f[g-1][c'] + sum_v t_v up to the rounding of another order of additions, in V K^(V+1) operations instead of K^(2V).
 * 5. End and backtrack.  The last frame takes the first minimum of f[f1-1][.] in lexicographic order; from g to g - 1 the back-pointer digits are
 *    applied for v = V - 1 down to 0, c_v <- bp_v[g][c] with c updated in between (the inverse of the staging).  path_cost[take] (double) = f at
 *    the chosen end state; an empty clamped range writes path_cost = 0 and nothing else.
 * 6. Emit, per frame with its chosen c, steps 5 to 7 of mp_lift_fuse over the views valid at the frame: pose (Ftot, J, 3) the mean in view order,
 *    joint 0 stored as +0; spread (Ftot); cost[f] = (float)E_f(c); choice (Ftot, V) bytes, 255 for a view invalid at f (whatever its free digit);
 *    ok[f] = 1, 0 if E_f(c) >= 1e30; no valid view: pose, cost and spread 0, every choice 255, ok 0.  A frame outside every take's clamped range
 *    is not written.
 * With path_sigma = +inf and switch_cost = 0 the choice is mp_lift_fuse's wherever its minimum is unique; with V = 1, quat null, score_weight = 1
 * and joint 0 at the origin the path and path_cost are mp_lift_path's.
 * scratch: at least mp_lift_fuse_path_scratch_bytes(V, Ftot, K) bytes = Ftot (8 R + 2 K^V + 2) rounded up to 8, R = (V (V - 1) / 2 + V) K^2 + V K
 * (per frame the row of pair, transition and unary tables in doubles, one 16-bit word of V 3-bit back-pointer digits per state, the chosen state),
 * 8-byte aligned; 0 for arguments out of range.  The backtrack walks the back-pointers out of LDS, at most MP_LIFT_FUSE_PATH_CHUNK frames at a
 * time.
 * MP_ERR_ARG before anything is launched: those of mp_lift_fuse; path_sigma not > 0; switch_cost negative or not finite; path_cost null; scratch
 * null, too small or misaligned. */
#define MP_LIFT_FUSE_PATH_CHUNK 512
int64_t mp_lift_fuse_path_scratch_bytes(int V, int64_t Ftot, int K);
int mp_lift_fuse_path(const float* hyps, int V, int64_t Ftot, int K, int J, int C, const uint8_t* valid, const int64_t* take_offset, int G,
                      const float* quat, float sigma, float score_weight, float path_sigma, float switch_cost, float* pose, uint8_t* choice, float* cost,
                      float* spread, uint8_t* ok, double* path_cost, void* scratch, int64_t scratch_bytes, void* stream);

/* Aligning the views of a take WITHOUT extrinsics: mp_lift_fuse, mp_lift_fuse_place and mp_lift_fuse_path stand on every camera's calibrated
 * orientation and position; this estimates them from the lifted poses themselves, up to the choice of a reference view.  Two views of one motion
 * give, per frame, the same root-relative body in two camera frames: they differ by ONE rotation for the whole take, and their placed roots
 * (mp_lift_place[_refine]) by that rotation and ONE translation.  The rotation is Horn's closed form over all frames of the take, re-weighted
 * (single views do produce depth-mirrored bodies: mp_lift_fuse exists because of them).  The conventions are mp_lift_fuse's: takes, take_offset
 * (entries clamped to 0 .. Ftot), valid (V, Ftot) bytes or null, 1 <= V <= MP_LIFT_FUSE_MAXV; fp64 between the float32 loads and the float32
 * stores, without contraction into fused multiply-adds; no atomics, fixed orders: identical bits on every call; a take's result does not depend
 * on the other takes of the call; the call does not synchronise.  Not measured on real data.
 * poses (V, Ftot, J, C) read only, C = 3 or 4 (channel 3 is not read), 2 <= J <= 32: one pose per view and frame in that view's camera frame;
 * traj (V, Ftot, 3) floats and traj_ok (V, Ftot) bytes, or both null: the views' camera-space roots; sigma > 0 in the poses' unit (+inf: every
 * weight is exactly 1); 0 <= iters <= MP_LIFT_ALIGN_MAXITERS.  Per take g with frames [f0, f1):
 * 1. b[v][f][j] = x[v][f][j] - x[v][f][0].
 * 2. The reference view r is the lowest view with at least one valid frame in the take.  Its row: quat = (1, 0, 0, 0), trans = 0, rms = 0,
 *    trans_rms = 0, used = its valid frames, ok = 1.  A take without such a view writes, for every view, quat = (1, 0, 0, 0), zeros and ok = 0.
 * 3. Frame f is USED for view v if it is valid in v and in r and all 3 J coordinates of both poses are finite.
 * 4. M = sum_f w_f S_f over the used frames,  S_f = sum_j b[v][f][j] b[r][f][j]^T (row: view v's channel, column: the reference's), joints in
 *    order;  w_f = 1 in the first pass.  Horn's symmetric 4x4 N(M) as mp_lift_score's alignment forms it; its dominant eigenvector by cyclic Jacobi
 *    sweeps until off(N) <= 2^-52 |N|_F (30 at most), normalised;  q is canonical: w >= 0, and if w == 0 the first non-zero component is positive.
 * 5. iters times, with R = R(q):  e_f = (sum_j |b[r][f][j] - R b[v][f][j]|^2) / J,  w_f = 1 / (1 + e_f / sigma^2)^2, then step 4 again.
 * 6. Degenerate: no used frame; sum w not > 0; one of the ten sums not finite; the dominant eigenvalue not > 0 (all at any solve);
 *    (lambda_1 - lambda_2) <= 1e-9 |lambda_1| at the last solve.  Then ok = 0, quat = (1, 0, 0, 0), trans = 0, rms = 0, trans_rms = 0.
 * 7. rms[g][v] = sqrt(sum_f w_f e_f / sum_f w_f), e_f at the final q, w_f the weights of the last solve (1 for iters = 0);  used[g][v] = the
 *    number of used frames (also in a degenerate row).
 * 8. With traj: over the used frames with traj_ok set in v and in r,  d_f = traj[r][f] - R traj[v][f],  T = sum w_f d_f / sum w_f,
 *    trans_rms = sqrt(sum w_f |d_f - T|^2 / sum w_f) in a pass of its own after T, the weights those of step 7.  No such frame, sum w not > 0 or
 *    a sum that is not finite: T = 0, trans_rms = 0 and ok keeps bit 0 only.  ok is a byte: bit 0 the rotation, bit 1 the translation.
 * 9. x_ref = R_v x_v + T_v, mp_lift_fuse's camera-to-world with the reference view's frame as the world: quat and trans can be passed on as they are.
 * One workgroup of 256 lanes per (take, view): a lane sums the frames f0 + lane, f0 + lane + 256, ... in order, the lanes' sums are added by a
 * butterfly within a wave and the four waves' in wave order, every lane solves the 4x4 problem; the passes (iters + 2, with traj iters + 4)
 * follow one another inside the workgroup.
 * quat (G, V, 4), rms (G, V) floats, used (G, V) int32, ok (G, V) bytes; trans (G, V, 3) and trans_rms (G, V) floats, needed with traj, else they
 * may be null (given without traj they are written as zeros).
 * MP_ERR_ARG before anything is launched: poses, take_offset, quat, rms, used or ok null; V, J or C out of range; Ftot or G <= 0, G > Ftot,
 * Ftot or G V > 2^31 - 1; sigma not > 0; iters out of range; exactly one of traj and traj_ok null; trans or trans_rms null while traj is given. */
#define MP_LIFT_ALIGN_MAXITERS 8
int mp_lift_align_views(const float* poses, int V, int64_t Ftot, int J, int C, const uint8_t* valid, const int64_t* take_offset, int G,
                        const float* traj, const uint8_t* traj_ok, float sigma, int iters, float* quat, float* trans, float* rms, float* trans_rms,
                        int32_t* used, uint8_t* ok, void* stream);

/* Synchronising the views of a take IN TIME: every operator above assumes that frame f of every view shows the same instant.  Cameras that were
 * never calibrated against each other were not gen-locked either: their views start a few frames apart, often by a fraction of a frame.  This
 * estimates every view's lag against a reference view from the lifted poses themselves, before any camera is known, and mp_lift_shift_views puts
 * a per-view array on the reference's clock.  The signal is the distance of every joint from the root: it does not depend on the camera's
 * orientation, and mirroring the camera's z - the lifter's depth ambiguity - leaves it untouched.  (Joint speeds, the obvious alternative, failed
 * by tens of frames at 10 mm of noise in a numpy prototype.)  The conventions are mp_lift_align_views': takes, take_offset (entries clamped to
 * 0 .. Ftot), valid (V, Ftot) bytes or null, 1 <= V <= MP_LIFT_FUSE_MAXV; fp64 between the float32 loads and the float32 stores, without
 * contraction into fused multiply-adds; no atomics, fixed orders: identical bits on every call; a take's result does not depend on the other
 * takes of the call; the call does not synchronise.  Not measured on real data.
 * poses (V, Ftot, J, C) read only, C = 3 or 4 (channel 3 is not read), 2 <= J <= 32: one pose per view and frame in that view's camera frame;
 * 0 <= max_lag <= MP_LIFT_SYNC_MAXLAG, written L; min_overlap >= 1; sigma > 0 in the poses' unit (+inf: plain squares).  Per take g with frames
 * [f0, f1):
 * 1. d[v][f][j] = |x[v][f][j] - x[v][f][0]|, j = 1 .. J - 1: the square root of the squared differences added in channel order.  Frame f is
 *    USABLE in view v if it is valid there and all 3 J coordinates are finite.
 * 2. used[g][v] = the number of usable frames;  m[v][j] = the mean of d over them (lane l of 256 sums the take's frames l, l + 256, .. in order, the
 *    lanes' sums are added by a butterfly within a wave and the four waves' in wave order);  s[v][f][j] = d - m.  The mean is removed so that a view whose lifter sees the body slightly larger does not pay
 *    for it at every lag.
 * 3. The reference view r is the lowest view with a usable frame.  Its row: lag = 0, lag_int = 0, a curve of zeros, contrast = 0, ok = 1.  A take
 *    without such a view writes zeros and ok = 0 for every view.
 * 4. For a view v != r and a lag d in -L .. L the PAIRS are the frames f with f and f + d both inside the take, r usable at f and v usable at
 *    f + d; n(d) is their number.  n(d) < min_overlap: the lag is INELIGIBLE and curve[d] = +inf.  Else
 *    e_f = (sum_j (s[v][f+d][j] - s[r][f][j])^2) / (J - 1), joints in order, and  curve[d] = (sum_f e_f / (1 + e_f / sigma^2)) / n(d); with sigma = +inf every
 *    term is exactly e_f.  The order of the sum: the take's n frames are cut into chunks of max(256, 64 ceil(n / 4096)) frames; slot s of 16 sums
 *    a chunk's frames s, s + 16, .. in order, the 16 sums are added in order, then the chunks' sums in order.  A value
 *    that is not finite makes the lag ineligible.
 * 5. d* is the eligible lag with the smallest curve value; ties go to the smaller |d|, then to the positive lag.  No eligible lag: ok = 0,
 *    lag = 0, lag_int = 0, contrast = 0.
 * 6. The sub-frame part, in fp64 from the fp64 curve values c: if |d*| < L, both neighbours are eligible and
 *    den = c[d*-1] - 2 c[d*] + c[d*+1] > 0, then delta = clamp(0.5 (c[d*-1] - c[d*+1]) / den, -0.5, 0.5); otherwise delta = 0.
 *    lag = float32(d* + delta), lag_int = d*.  The parabola is biased: on noise-free synthetic views the estimate was off by up to 0.08 frame.
 * 7. ok is a byte: bit 0 a lag was estimated, bit 1 the minimum is interior (step 6's conditions held; without it the true lag may lie outside
 *    the search range).  contrast = 1 - c[d*] / (the mean of the eligible curve values, summed in lag order by 64 lanes and a butterfly), and 0
 *    where that mean is not > 0.
 * 8. Meaning: frame f + lag of view v shows what frame f of the reference shows.
 * lag, contrast (G, V) floats; lag_int, used (G, V) int32; curve (G, V, 2 L + 1) floats, lag d at d + L; ok (G, V) bytes.
 * scratch: at least mp_lift_sync_views_scratch_bytes(V, Ftot, J) bytes = V Ftot (8 (J - 1) + 80 + 1) rounded up to 8 (the signals; per take,
 * lag and chunk a sum and a number of pairs - a take of n frames has at most 2 n - 1 lags with a pair, and fewer than 5 n such entries -; the
 * usable bytes), 8-byte aligned; 0 for arguments out of range.
 * Three kernels: one workgroup per (take, view) writes s and the usable bytes; one workgroup per (take, view, block of 16 lags, chunk) stages
 * tiles of 64 reference rows and the view's 79 rows that pair with them in LDS; one wave per (take, view) adds the chunks and takes the minimum.
 * MP_ERR_ARG before anything is launched: poses, take_offset or an output null; V, J or C out of range; Ftot or G <= 0, G > Ftot, Ftot or
 * G V > 2^31 - 1; max_lag or min_overlap out of range; sigma not > 0; scratch null, misaligned or too small.
 * mp_lift_shift_views: in and out (V, Ftot, M) are rows of M floats per frame, 1 <= M <= MP_LIFT_SHIFT_MAXM; they must not overlap.  lag (G, V)
 * device floats.  Per take, view and frame f:  p = (f - f0) + lag in fp64.
 * mode 0, nearest: i = floor(p + 0.5); the row is a copy, bit for bit, of frame f0 + i where i is inside the take and valid there.
 * mode 1, linear: i = floor(p), a = p - i; with a == 0 the row is a copy of frame f0 + i; otherwise frames i and i + 1 must both be inside the
 * take and valid, and out = (1 - a) x_i + a x_{i+1}: two products and one sum in fp64, not contracted, rounded once.
 * A frame without a result gets zeros and valid_out = 0, a frame with one valid_out = 1; so does every frame no take holds.  A lag that is not
 * finite invalidates the whole view of that take.  A lag of 0 reproduces in at the valid frames and valid (as 0 / 1) exactly.
 * MP_ERR_ARG before anything is launched: in, take_offset, lag, out or valid_out null; V or M out of range; Ftot or G <= 0, G > Ftot; an
 * unknown mode; in and out overlapping; more floats than one grid holds. */
#define MP_LIFT_SYNC_MAXLAG 256
#define MP_LIFT_SHIFT_MAXM 1048576
int64_t mp_lift_sync_views_scratch_bytes(int V, int64_t Ftot, int J);
int mp_lift_sync_views(const float* poses, int V, int64_t Ftot, int J, int C, const uint8_t* valid, const int64_t* take_offset, int G,
                       int max_lag, int min_overlap, float sigma, float* lag, int32_t* lag_int, float* curve, float* contrast,
                       int32_t* used, uint8_t* ok, void* scratch, int64_t scratch_bytes, void* stream);
int mp_lift_shift_views(const float* in, int V, int64_t Ftot, int64_t M, const uint8_t* valid, const int64_t* take_offset, int G,
                        const float* lag, int mode, float* out, uint8_t* valid_out, void* stream);

/* Bundle-adjusting a take's cameras: mp_lift_align_views gives the extrinsics in closed form from the lifted poses and the per-view roots, and the
 * 2-D keypoints - the only measured quantity - decide nothing about them.  This is the joint Gauss-Newton refinement of all free cameras and all
 * per-frame world roots of a take on the robust reprojection error, the roots eliminated by a Schur complement.  The reference has no counterpart.
 * The conventions are mp_lift_fuse_place's: takes, take_offset (G + 1, entries clamped to 0 .. Ftot), valid (V, Ftot) bytes or null,
 * 1 <= V <= MP_LIFT_FUSE_MAXV, 2 <= J <= 32, quat (G, V, 4), trans (G, V, 3), intr (G, V, 9), R the matrix of q / |q| normalised in fp64, a view whose
 * |q|^2 is not finite or < 1e-12 counts as invalid, x_world = R x_cam + T, weights (J) or null, distort as for mp_lift_place_refine; fp64 between
 * the float32 loads and the float32 stores, without contraction into fused multiply-adds; no atomics, fixed orders: identical bits on every call;
 * a take's result does not depend on the other takes of the call; the call does not synchronise.  Not measured on real data.
 * Read only: pose (Ftot, J, 3) the fused root-relative world pose; root (Ftot, 3) and root_ok (Ftot) bytes or null; kp (V, Ftot, J, 2); the camera
 * tables; fixed (G, V) bytes or null; sigma > 0 in normalised screen units (+inf: every robust factor is exactly 1); 0 <= iters <=
 * MP_LIFT_BUNDLE_MAXITERS.  Per take g with frames [f0, f1):
 * 1. Observations.  (v, f) is USED if view v is valid at f (its valid byte and its quaternion), root_ok is null or non-zero at f, the root and
 *    all 3 J coordinates of the pose are finite, and both coordinates of every keypoint of view v whose joint has a non-zero weight are finite.
 *    A frame with no used observation is outside the problem: its root is copied through bit for bit.  used[g][v] = the used frames of view v.
 * 2. Gauge.  A view is FIXED if fixed[g][v] != 0; with fixed null the fixed view is the lowest view with a used frame (mp_lift_align_views'
 *    reference).  The FREE views are the views that are not fixed and have a used frame, in view order (their slots k = 0, 1, ..); a view that is
 *    not fixed and has no used frame is outside the problem and copied through.  A take with no fixed view that has a used frame, or with no free
 *    view, evaluates only: steps = 0, ok as step 5 finds it, reproj and cost written (start = end), cameras and roots copied through.  A fixed
 *    view's quat and trans are copied through bit for bit in every case.
 * 3. Residuals.  State in fp64: per view the unit quaternion q and T, per used frame the root r; at the start q = quat / |quat|, T = trans,
 *    r = root.  P = R(q)^T (pose_j + r - T).  The projection, the clamp, its derivative and the 2x3 Jacobian J_pi with respect to P are exactly
 *    step 2 of mp_lift_place_refine.  With res = (du, dv) and e = du^2 + dv^2:  t = 1 + e / sigma^2,  rho = e / t,  omega = 1 / t^2
 *    (mp_lift_align_views' weight).  F = sum w_j rho over the used observations: views in order, within a view the joints in order - per frame, then
 *    the frames in increasing order.  Per view E_v = sum w_j sqrt(e), W_v = sum w_j likewise; E_v / W_v is the view's weighted mean distance, as
 *    mp_lift_fuse_place's reproj.  A joint of weight 0 is skipped.  deep: every weighted joint of every used observation has Z > 0.
 * 4. Parameters.  A frame's root moves by dr, with Jacobian J_r = J_pi R^T.  A free camera moves by a left perturbation of the camera-space point,
 *    P' = exp([w]x) P + tau, with Jacobian J_c = J_pi [-[P]x | I] (2x6, the rotation first).  Applied to the world-to-camera pair
 *    (R^T, -R^T T) <- (exp([w]x) R^T, exp([w]x) (-R^T T) + tau) with the exact rotation of w, which in (q, T) reads
 *    q <- q * conj(q_w),  q_w = (cos(th / 2), sin(th / 2) w / th) with th = |w|, and for th^2 <= 1e-16 the small-angle branch q_w = (1, w / 2);
 *    the product is normalised and made canonical by mp_lift_align_views' sign rule (w >= 0, and if w == 0 the first non-zero component is
 *    positive; a zero comes out as +0);  then T <- T - R(q) tau with the new q.
 * 5. One step, normal equations with the weights w_j omega.  Per used frame, views in order, joints in order:  U_f = sum J_r^T J_r (3x3),
 *    b_f = sum J_r^T res, and per free view used at f  W_fv = sum J_r^T J_c (3x6), A_fv = sum J_c^T J_c (6x6), a_fv = sum J_c^T res.  U_f^-1 by
 *    cofactors with mp_lift_place_refine's test, det finite and > 1e-12 U00 U11 U22.  The reduced system over the free views' slots:
 *    S = sum_f (blockdiag(A_f) - W_f^T (U_f^-1 W_f)),  s = sum_f (a_f - W_f^T (U_f^-1 b_f)), each frame's term formed first, then the frames added
 *    in increasing order.  S = L L^T by Cholesky (row by row) in fp64; a pivot that is not finite and > 1e-12 times its diagonal entry of S means
 *    "no step".  dc = -S^-1 s;  dr_f = -(U_f^-1 b_f + sum_k (U_f^-1 W_fk) dc_k), slots in order.  The candidate is the state moved by (dc, dr).
 *    The step is taken iff every U_f and the factorisation pass, dc and the candidate cameras are finite, deep holds at the candidate and
 *    F' <= (1 + 1e-6) F (a non-finite candidate root gives a non-finite F', which is not taken).  On the first step not taken the take's iteration
 *    ends and its state stays.  If the first evaluation is not deep or F is not finite: ok = 0, everything copied through, steps = 0, reproj and
 *    cost as evaluated (start = end); otherwise ok = 1.  At most iters steps.
 * 6. Outputs.  quat_out (G, V, 4), trans_out (G, V, 3) floats: while steps = 0 the inputs bit for bit, else a free view's (q, T) rounded to
 *    float32 (q unit and canonical), every other view copied through;  root_out (Ftot, 3): a used frame's r rounded to float32 (bit for bit the
 *    input while steps = 0), every other frame of the call copied through;  reproj (G, V, 2) floats: E_v / W_v at the start and at the end, 0 for a
 *    view with no used frame;  cost (G, 2) doubles: F at the start and at the end;  steps (G), ok (G) bytes;  used (G, V) int32.
 * Schedule: one lane per frame evaluates, forms the frame's blocks view by view and writes its term of S and s (at most 171 + 18 doubles) to the
 * scratch; one workgroup per take sums the terms, lane e entry e, frames in increasing order, then decides, factorises and forms the candidate
 * cameras; the next pass of the frame kernel applies dc and its own dr at its head.  iters + 1 passes, launched in a fixed sequence.
 * scratch: at least mp_lift_bundle_views_scratch_bytes(V, Ftot) bytes = 3056 Ftot (per frame: 200 doubles of its row, 118 of blocks kept between
 * the passes, 64 of a take's state), 8-byte aligned; 0 for arguments out of range.
 * MP_ERR_ARG before anything is launched: an input or output pointer null (root_ok, valid, fixed, weights may be null); V or J out of range; Ftot or
 * G <= 0, G > Ftot, Ftot > 2^31 - 1; distort not 0 or 1; sigma not > 0; iters out of range; scratch null, too small or misaligned. */
#define MP_LIFT_BUNDLE_MAXITERS 8
int64_t mp_lift_bundle_views_scratch_bytes(int V, int64_t Ftot);
int mp_lift_bundle_views(const float* pose, const float* root, const uint8_t* root_ok, const float* kp, int V, int64_t Ftot, int J, const uint8_t* valid,
                         const int64_t* take_offset, int G, const float* quat, const float* trans, const float* intr, const uint8_t* fixed,
                         const float* weights, int distort, float sigma, int iters, float* quat_out, float* trans_out, float* root_out, float* reproj,
                         double* cost, uint8_t* steps, uint8_t* ok, int32_t* used, void* scratch, int64_t scratch_bytes, void* stream);

/* Calibrating a take on its keypoints: mp_lift_bundle_views holds the fused pose fixed as structure and reads the focal lengths from a calibration,
 * so whatever the lifter got wrong - a scale error above all - goes into the cameras.  This is the full bundle adjustment of a take: every joint of
 * every used frame is a free 3-D point, every free camera has its six pose parameters, every view with a used frame one focal factor, all fitted
 * to the 2-D keypoints by undamped Gauss-Newton steps, the points eliminated one by one by a Schur complement.  The start enters only as a weak
 * prior on the points.  The reference has no counterpart.  The conventions are mp_lift_bundle_views': takes, take_offset, valid, quat (G, V, 4),
 * trans (G, V, 3), intr (G, V, 9), fixed (G, V) bytes or null, weights (J) or null, distort, sigma; fp64 between the float32 loads and the float32
 * stores, without contraction; no atomics, fixed orders: identical bits on every call; a take's result does not depend on the other takes of the
 * call; the call does not synchronise.  Not measured on real data.
 * WHY AT LEAST TWO VIEWS: from one view's lifted poses the focal length is a linear fit once the per-frame (f tx, f ty, tz) are eliminated - exact on
 * noise-free poses, but what is left as regressor is only the perspective part of the body (about 16 mm), below a lifter's error: in float64 on
 * 3000 synthetic frames, true f = 2.29, keypoint noise 0.002, 20 mm of pose noise gave f = 1.53 .. 1.60 and 45 mm gave 0.66 .. 0.74.
 * WHY prior > 0: the keypoints leave one gauge freedom, the scale of points and camera positions together; with prior = 0 the reduced system's
 * condition number is 1e17 and the points drift (0.35 m in the float64 prototype); with prior 1e-3 it was 2.4e6 .. 2.4e7.
 * Read only: start (Ftot, J, 3) world points (the fused pose plus its root); start_ok (Ftot) bytes or null; kp (V, Ftot, J, 2); the camera tables;
 * focal 0 or 1; prior finite and > 0; 0 <= iters <= MP_LIFT_CALIBRATE_MAXITERS.  Per take g with frames [f0, f1):
 * 1. Observations.  mp_lift_bundle_views' step 1 with "the root and the pose are finite" replaced by "all 3 J coordinates of start are finite"
 *    and root_ok by start_ok.  A frame with no used observation is outside the problem.  used[g][v] = the used frames of view v.
 * 2. Gauge.  FIXED and FREE views as in mp_lift_bundle_views' step 2 (no fixed view with a used frame, or no free view: no camera moves); the free
 *    views' slots k = 0, 1, .. own the columns 6 k .. 6 k + 5 of the reduced system.  With focal = 1 every view with a used frame, fixed ones
 *    included, has a focal factor g_v, starting at 1; their columns follow the cameras' in view order: N <= 22 columns.  The take ITERATES iff
 *    N >= 1 and at least two views have a used frame; otherwise it evaluates only: steps = 0, everything copied through, reproj and cost written
 *    (start = end).
 * 3. Residuals.  State in fp64: per view q, T (as in mp_lift_bundle_views) and g_v, per used frame and joint the point X_fj, starting at start.
 *    P = R(q)^T (X - T); the projection of mp_lift_bundle_views' step 3 with fx = g_v fx0, fy = g_v fy0 (the products in fp64; the principal
 *    point and the distortion coefficients stay); res, e, t, rho, omega as there.  A joint of weight 0 is skipped: no camera sees it and it stays
 *    at start.  Per frame and view F_fv = sum_j w_j rho, E_fv = sum_j w_j sqrt(e), W_fv = sum_j w_j, joints in order;  P_f = sum_j w_j
 *    ((dx^2 + dy^2) + dz^2) with d = X_fj - start_fj;  F_f = (sum_v F_fv, the used views in order) + prior P_f;  F, E_v, W_v: the frames in
 *    increasing order.  deep as in mp_lift_bundle_views.
 * 4. Parameters.  A point moves by dX with Jacobian J_x = J_pi R^T; a free camera as in mp_lift_bundle_views' step 4 (J_c, 2x6, and its update);
 *    a focal factor moves additively, g <- g + dg, with the Jacobian column J_g = ((res + keypoint) - (cx, cy)) / g, which is (pi(P) - c) / g for
 *    either value of distort, pi(P) taken back from the residual.
 * 5. One step.  Per point, with the weights w_j omega over the views that use the frame, in view order:  U = prior w_j I + sum J_x^T J_x,
 *    b = prior w_j (X - start) + sum J_x^T res (the prior's term first), W = the 3 x N matrix whose columns of view v are w_j omega J_x^T [J_c | J_g]
 *    (zero for a view that does not use the frame or has no such column), a likewise from [J_c | J_g]^T res, and A_rc = w_j omega (J_r . J_c) where
 *    columns r and c belong to the same view, else 0.  U^-1 by cofactors with mp_lift_place_refine's test.  The point's term of the reduced system is
 *    S_rc = A_rc - W_r^T (U^-1 W_c) for c <= r and s_c = a_c - W_c^T (U^-1 b), every product of three summed as (p0 + p1) + p2; the terms are added
 *    to zero, a frame's joints in order, then the frames in increasing order.  S = L L^T, the pivot test, dc = -S^-1 s as in mp_lift_bundle_views;
 *    dX = -(U^-1 b + sum_c (U^-1 W)_c dc_c), columns in order.  The candidate is the state moved by (dc, dX).  The step is taken iff every U and
 *    the factorisation pass, dc and the candidate cameras are finite, every candidate g is finite and > 0, deep holds at the candidate and
 *    F' <= (1 + 1e-6) F.  The first step not taken ends the take's iteration and its state stays.  If the first evaluation is not deep or F is not
 *    finite: ok = 0, everything copied through, steps = 0; otherwise ok = 1.  At most iters steps.
 * 6. Outputs.  quat_out, trans_out, reproj, cost, steps, ok, used as mp_lift_bundle_views writes them.  intr_out (G, V, 9): while steps = 0 intr bit
 *    for bit, else fx, fy of a view with a focal factor are (float)(g fx0), (float)(g fy0) and the other entries copied.  points (Ftot, J, 3): a
 *    used frame's weighted joints rounded to float32 (start's bits while steps = 0), everything else copied from start bit for bit.
 * Schedule: one lane per frame goes through the frame's points one by one, the point's blocks by column in lane-private LDS, and adds each point's
 * term of S and s (at most 253 + 22 doubles) to the frame's row in the scratch; one workgroup per take sums the rows, lane e entry e, frames in
 * increasing order, then decides, factorises and forms the candidate cameras and focal factors; the next pass of the frame kernel applies dc and
 * its own dX at its head.  iters + 1 passes, launched in a fixed sequence.
 * scratch: at least mp_lift_calibrate_views_scratch_bytes(V, Ftot, J) bytes = 8 Ftot (286 + 1 + 75 J + 96), 8-byte aligned; 0 for arguments out
 * of range.
 * MP_ERR_ARG before anything is launched: what mp_lift_bundle_views rejects (start_ok, valid, fixed, weights may be null), focal not 0 or 1, prior
 * not finite or not > 0. */
#define MP_LIFT_CALIBRATE_MAXITERS 8
int64_t mp_lift_calibrate_views_scratch_bytes(int V, int64_t Ftot, int J);
int mp_lift_calibrate_views(const float* start, const uint8_t* start_ok, const float* kp, int V, int64_t Ftot, int J, const uint8_t* valid,
                            const int64_t* take_offset, int G, const float* quat, const float* trans, const float* intr, const uint8_t* fixed,
                            const float* weights, int focal, int distort, float sigma, float prior, int iters, float* quat_out, float* trans_out,
                            float* intr_out, float* points, float* reproj, double* cost, uint8_t* steps, uint8_t* ok, int32_t* used, void* scratch,
                            int64_t scratch_bytes, void* stream);

/* Triangulating a fused take's joints on the 2-D keypoints: after mp_lift_fuse, mp_lift_fuse_place and mp_lift_bundle_views the keypoints - the only
 * measured quantity - decide the root (three numbers per frame) and the cameras; the body is still the mean of one lifted hypothesis per view,
 * though every joint is seen by up to four cameras.  Here every joint of every frame becomes a world point of its own, triangulated from its
 * observations; the fused pose plus root chooses the start where the linear system cannot, stands in where fewer than two cameras see the joint,
 * and may pull (prior).  The reference has no counterpart.  The conventions are mp_lift_fuse_place's: takes, take_offset (G + 1, entries clamped
 * to 0 .. Ftot), valid (V, Ftot) bytes or null, 1 <= V <= MP_LIFT_FUSE_MAXV, 2 <= J <= 32, quat (G, V, 4), trans (G, V, 3), intr (G, V, 9), R the matrix
 * of q / |q| normalised in fp64, a view whose |q|^2 is not finite or < 1e-12 counts as invalid in its take, the camera-space point of the world point
 * X is P = R^T (X - T_v), distort as for mp_lift_place_refine, 0 <= iters <= MP_LIFT_REFINE_MAXITERS; fp64 between the float32 loads and the
 * float32 stores, without contraction into fused multiply-adds; no atomics, fixed orders: identical bits on every call; an item depends on no
 * other item; the call does not synchronise.  Not measured on real data.
 * Read only: pose (Ftot, J, 3) as mp_lift_fuse wrote it; root (Ftot, 3) and root_ok (Ftot) bytes or null; kp (V, Ftot, J, 2); kp_weight (V, Ftot, J)
 * floats or null (every weight 1): a weight per observation, the detector's confidence or an occlusion mask; the camera tables; sigma > 0 in
 * normalised screen units (+inf: every robust factor is exactly 1); prior >= 0 and finite.  Per item (frame f of take g, joint j):
 * 1. Prior point.  X0 = pose[f][j] + root[f];  USABLE iff root_ok is null or non-zero at f and the three coordinates of X0 are finite.
 * 2. Observations.  View v is an observation iff it counts at the frame (its valid byte and its take's quaternion), both coordinates of its
 *    keypoint are finite and its weight w_v is finite and > 0 (a zero, negative or non-finite weight: not observed, no error; an invalid view's
 *    keypoint and weight are never looked at).  n = the number of observations; every sum below runs over them in view order.
 * 3. Linear start, under the pinhole part as step 1 of mp_lift_fuse_place: with a = (u - cx) / fx, b = (v - cy) / fy and rho_x, rho_y, rho_z the
 *    rows of R^T,  m_x = rho_x - a rho_z,  m_y = rho_y - b rho_z,  H = sum w_v (m_x m_x^T + m_y m_y^T),  h = sum w_v (m_x (m_x . T_v) + m_y (m_y . T_v)),
 *    X = adj(H) h / det by cofactors.  If n >= 2, det and H00 H11 H22 are finite, det > 1e-12 H00 H11 H22 and X is finite, X is the start and the
 *    item is TRIANGULATED; otherwise the start is X0 if usable; otherwise the item FAILS: points = 0, err = 0, ok = 0, steps = 0 (views as step 2).
 * 4. Evaluation at X.  Per observation the projection, the clamp, its derivative and the 2x3 Jacobian J_pi with respect to P are exactly step 2
 *    of mp_lift_place_refine; with (du, dv) the residual and e = du^2 + dv^2:  t = 1 + e / sigma^2,  rho = e / t,  omega = 1 / t^2
 *    (mp_lift_bundle_views' form).  F = sum w_v rho,  E = sum w_v sqrt(e),  W = sum w_v,  H = sum (w_v omega) (J_pi R^T)^T (J_pi R^T),
 *    g = sum (w_v omega) (J_pi R^T)^T (du, dv),  deep = every observation's Z > 0;  then, iff prior > 0 and X0 is usable, F += prior |X - X0|^2,
 *    H += prior I, g += prior (X - X0).  If the triangulated start is not deep and X0 is usable, the item starts once more from X0 and is no
 *    longer triangulated.  A start that is not deep, or whose F is not finite, fails as in step 3.
 * 5. Steps.  Up to iters undamped Gauss-Newton steps X' = X - adj(H) g / det under the tests of mp_lift_place_refine (det and H00 H11 H22 finite,
 *    det > 1e-12 H00 H11 H22, X' finite); X' is taken iff it is deep and F' <= (1 + 1e-6) F.  The first step not taken ends the item and its state
 *    stays.  With one observation and prior = 0, H has rank 2: the step is refused and the joint stays at X0 - the intended fallback; with no
 *    observation and prior = 0 likewise (H = 0).  (With no observation and prior > 0 the steps are taken and move nothing: at X0, g = 0 and F = 0.)
 * 6. points (Ftot, J, 3) floats: X;  err (Ftot, J) floats: E / W at the final X, the weighted mean reprojection distance (0 when n = 0);
 *    views (Ftot, J) bytes: bit v set iff view v was an observation;  ok (Ftot, J) bytes: bit 0 a finite result, bit 1 triangulated;
 *    steps (Ftot, J) bytes or null: the steps taken.  A frame outside every take's clamped range is not written.
 * One lane owns one item, items in f J + j order.
 * MP_ERR_ARG before anything is launched: an input or output pointer null (valid, root_ok, kp_weight, steps may be null); V or J out of range;
 * Ftot or G <= 0, G > Ftot; distort not 0 or 1; iters out of range; sigma not > 0; prior negative or not finite; more items than one grid holds. */
int mp_lift_triangulate(const float* pose, const float* root, const uint8_t* root_ok, const float* kp, const float* kp_weight, int V, int64_t Ftot,
                        int J, const uint8_t* valid, const int64_t* take_offset, int G, const float* quat, const float* trans, const float* intr,
                        int distort, float sigma, float prior, int iters, float* points, float* err, uint8_t* views, uint8_t* ok, uint8_t* steps,
                        void* stream);

/* Fitting ONE SKELETON to a fused take's keypoints.  mp_lift_triangulate leaves 17 points per frame, not a body: bone lengths change from frame
 * to frame, a joint that fewer than two cameras see falls back to the lifted pose, nothing ties a joint to its neighbours.  mp_lift_rigid gives
 * constant bones by keeping every bone's direction and re-assembling the pose bone by bone: the keypoints have no say, and an error in the hip's
 * direction moves the whole leg.  Here a frame's pose IS the root and one unit direction per bone of a fixed bone table, and these
 * U = 3 + 2 (J - 1) unknowns are fitted to the keypoints of all joints at once by undamped Gauss-Newton steps.  The reference has no counterpart.
 * The conventions are mp_lift_triangulate's: takes, take_offset (G + 1, entries clamped to 0 .. Ftot), valid (V, Ftot) bytes or null, kp
 * (V, Ftot, J, 2), kp_weight (V, Ftot, J) or null, 1 <= V <= MP_LIFT_FUSE_MAXV, quat (G, V, 4), trans (G, V, 3), intr (G, V, 9), R the matrix of
 * q / |q| normalised in fp64, a view whose |q|^2 is not finite or < 1e-12 counts as invalid in its take, P = R^T (X - T_v), distort, sigma > 0 in
 * normalised screen units (+inf: every robust factor is exactly 1), prior >= 0 and finite, 0 <= iters <= MP_LIFT_REFINE_MAXITERS; fp64 between the
 * float32 loads and the float32 stores, without contraction into fused multiply-adds, a sum a + b + c is (a + b) + c; no atomics, fixed orders:
 * identical bits on every call; a frame depends on no other frame; the call neither synchronises nor modifies its inputs.  Not measured on real data.
 * Read only: start (Ftot, J, 3) world points, the pose to start from and to be pulled towards; start_ok (Ftot) bytes or null; lengths (G, J - 1)
 * device floats, one bone table per take; parents (J) HOST int32 with mp_lift_rigid's conditions (parents[0] = -1, 0 <= parents[j] < j), bone
 * b = j - 1 joins joint j to parents[j]; 2 <= J <= 32.  Per frame f of take g:
 *  0. Not fitted.  If start_ok[f] is 0, a start coordinate is not finite, or a length of the take's row is not finite or not > 0:  pose = 0,
 *     err = 0, ok = 0, steps = 0.
 *  1. Start.  r = start[0].  For j = 1 .. J-1:  v = start[j] - start[parent],  n = sqrt(v . v);  d_b = v / n where n is finite and > 1e-12;
 *     otherwise d_b is the direction of the parent's bone ((0, 0, 1) under the root; decided in joint order) and bit 1 of ok is cleared.
 *  2. Observations.  Rule 2 of mp_lift_triangulate: view v counts by its valid byte and its take's quaternion; (v, j) is an observation where
 *     both keypoint coordinates and the weight are finite and the weight is > 0.  An invalid view's data is never looked at.
 *  3. Evaluation at (r, d).  p[0] = r,  p[j] = p[parent] + L_b d_b in joint order.  Per joint j over its observations in view order, rule 4 of
 *     mp_lift_triangulate at X = p[j]: camera point, deep (Z > 0), projection with its Jacobian, e = du^2 + dv^2, t = 1 + e / sigma^2, W_j += w,
 *     E_j += w sqrt(e), F_j += w (e / t), and S_j (3x3), g_j the normal equations of the 2x3 Jacobian J_pi R^T with weight w (1 / t^2); then, iff
 *     prior > 0, the pull: F_j += prior |p_j - start_j|^2, the diagonal of S_j += prior, g_j += prior (p_j - start_j).  F, E and W of the frame
 *     are the sums over the joints in joint order; deep asks every observation of every joint.
 *  4. Subtree sums.  T_j = S_j, h_j = g_j;  for j = J-1 down to 1:  T_parent += T_j,  h_parent += h_j.
 *  5. Tangent bases.  e = the unit axis of the coordinate where |d_b| is smallest, the lowest on a tie (step 4 of mp_lift_rotations);
 *     e1 = u / |u| with u = e - (e . d_b) d_b,  e2 = d_b x e1,  B_b = L_b [e1 e2] (3x2).
 *  6. The system of the U unknowns, the root's three and then (alpha_b, beta_b) per bone in bone order, p_j moving by B_b (alpha_b, beta_b) for
 *     every bone b between the root and j:  H_rr = T_0, right side h_0;  M_b = T_{b+1} B_b,  H_{r,b} = M_b;  H_{a,b} = B_a^T M_b for every bone a
 *     that is b or lies on the path from the root to b, 0 for every other pair;  the right side of bone b is B_b^T h_{b+1}.  This is
 *     sum_j J_j^T S_j J_j with the dense 3 x U Jacobian J_j of p_j, which is never formed.
 *  7. The solve.  H = C C^T, the lower factor:  entry (i, k) is H_ik minus the products C_im C_km for m = 0 .. k-1, one subtraction at a time in
 *     that order, over C_kk; a pivot (the diagonal entry before its square root) that is not finite or not > 1e-12 H_kk means NO STEP.
 *     Forward substitution  y_i = (b_i - sum_{k < i} C_ik y_k) / C_ii, i ascending, and back substitution
 *     delta_i = (y_i - sum_{k > i} C_ki delta_k) / C_ii, i descending, both sums one subtraction at a time with k ascending.
 *  8. The candidate.  r' = r - delta_r;  t_b = (d_b - delta_alpha e1) - delta_beta e2,  d'_b = t_b / |t_b| (|t_b| >= 1: nothing can vanish).  A
 *     non-finite number in r' or d' ends the frame's steps.
 *  9. Accept.  mp_lift_place_refine's rule: the candidate stands iff it is deep and F' <= (1 + 1e-6) F.  The steps end at the first refusal, at a
 *     failed pivot, or after iters.  If the start itself is not deep, or its F is not finite, the frame has NO RESULT: pose = 0, err = 0, steps =
 *     0, bit 0 of ok stays clear, bit 1 keeps what step 1 found.
 * 10. pose (Ftot, J, 3) floats: p;  err (Ftot, 2) floats: E / W, the weighted mean reprojection distance of the frame, at the rigid start and at
 *     the result (0 where nothing is observed);  ok (Ftot) bytes: bit 0 a finite result, bit 1 every bone of the start had a direction of its
 *     own;  steps (Ftot) bytes or null.  A frame outside every take's clamped range is not written.
 * With iters = 0 the result is the rigid start: mp_lift_rigid's rule applied to start in fp64.  With no observation and prior = 0, H = 0: no
 * step.  One 64-lane workgroup owns one frame; lane j evaluates joint j; the system lives in LDS.
 * MP_ERR_ARG before anything is launched: an input or output pointer null (start_ok, kp_weight, valid, steps may be null); V or J out of range;
 * Ftot or G <= 0, G > Ftot, Ftot > 2^31 - 1; a parent table that breaks its conditions; distort not 0 or 1; iters out of range; sigma not > 0;
 * prior negative or not finite. */
int mp_lift_fit_skeleton(const float* start, const uint8_t* start_ok, const float* kp, const float* kp_weight, int V, int64_t Ftot, int J,
                         const uint8_t* valid, const int64_t* take_offset, int G, const float* quat, const float* trans, const float* intr,
                         const float* lengths, const int32_t* parents, int distort, float sigma, float prior, int iters, float* pose, float* err,
                         uint8_t* ok, uint8_t* steps, void* stream);

/* Fitting a fused take's skeleton ALONG TIME.  mp_lift_fit_skeleton fits every frame on its own: every frame keeps its own keypoint noise, and the
 * fitted body jitters.  Here the frames of a take share one cost - the frames' own costs plus smooth times the squared second differences of
 * the joint positions - which sweeps over the frames lower, one Gauss-Newton step of a frame at a time with its neighbours held.  The 19 inputs,
 * the conventions, the checks and the numeric rules are mp_lift_fit_skeleton's: fp64 between the float32 loads and the float32 stores, no
 * contraction, a sum a + b + c is (a + b) + c, no atomics, fixed orders, identical bits on every call, inputs untouched, no synchronisation.
 * smooth >= 0 and finite: the weight of a squared second difference in square metres against the cost's normalised screen units squared;
 * 0 <= sweeps <= MP_LIFT_SKELETON_MAXSWEEPS.  scratch: device memory, 8-byte aligned, of at least
 * mp_lift_fit_skeleton_smooth_scratch_bytes(Ftot, J) = 48 Ftot J bytes (0 for arguments out of range); its contents after the call are not
 * specified.  Not measured on real data; smooth = 0.1 and 8 sweeps, the bindings' defaults, are untuned and come from a synthetic motion.
 * STAGE A.  Every frame is fitted by rules 0 to 10 of mp_lift_fit_skeleton: pose, err[:, 0:2], ok and steps are that function's bits.  The
 *   frame's state (r, d) and its positions p stay in fp64 in scratch and never make a float32 round trip between visits.  A frame is USABLE iff
 *   bit 0 of its ok is set.  err[:, 2] = err[:, 1], moves = 0.
 * STAGE B, iff smooth > 0 and sweeps > 0.  The cost of a take is the sum of its usable frames' F (rule 3, the pull towards the start included)
 *   plus  smooth sum_s sum_j |p_j(s-1) - 2 p_j(s) + p_j(s+1)|^2  over every take-local frame index s whose frames s-1, s, s+1 all lie in the
 *   take (its clamped range) and are all usable: a term never crosses a take's border or an unusable frame.
 *  S1. The stencil of frame t.  t appears in the terms centred at t-1 (coefficient 1), t (-2) and t+1 (1).  With u(k) = frame k lies in the take
 *     and is usable:  a = u(t-2) and u(t-1),  b = u(t-1) and u(t+1),  c = u(t+1) and u(t+2)  say which of them exist, and
 *     W_t = a + 4 b + c, one of 0, 1, 4, 5, 6.  With the other frames held, the terms that exist are  smooth W_t sum_j |p_j - q_j|^2  plus a
 *     constant, where per coordinate, with c1- = 2 a + 2 b, c1+ = 2 b + 2 c, c2- = a, c2+ = c (each 0, 1, 2 or 4),
 *       q_j = ((c1- p_j(t-1) + c1+ p_j(t+1)) - (c2- p_j(t-2) + c2+ p_j(t+2))) / W_t
 *     in exactly this order; a frame whose coefficient is 0 is not read and counts as 0.  The full stencil gives
 *     q = (4 (p(t-1) + p(t+1)) - (p(t-2) + p(t+2))) / 6  (the products are exact), b alone the midpoint of t-1 and t+1, a alone 2 p(t-1) - p(t-2).
 *  S2. The order of the visits.  For sweep = 0 .. sweeps-1, for colour = 0, 1, 2: every usable frame t of every take with
 *     (t - the take's first frame) mod 3 = colour and W_t > 0 is visited.  A visited frame reads frames t+-1 and t+-2, which have other colours:
 *     the visits of a colour are independent, and the result does not depend on their order.
 *  S3. A visit is ONE step of rules 3 to 9 from the frame's current state.  Rule 3 is evaluated with a second pull, added after the pull towards
 *     the start and exactly as that one is, with lambda = (double)smooth * W_t:  F_j += lambda |p_j - q_j|^2 (the squares summed (x + y) + z),
 *     the diagonal of S_j += lambda,  g_j += lambda (p_j - q_j).  If the state's evaluation is not deep or its F is not finite, a pivot fails
 *     (rule 7), the candidate is not finite (rule 8), or the candidate is refused (rule 9: it stands iff it is deep and F' <= (1 + 1e-6) F, on
 *     this conditional cost, so the take's cost never rises by more than that slack), the frame's state stays and the frame is visited again
 *     in the next sweep.  An accepted candidate becomes the state; pose and err[:, 2] are written from it, moves += 1.
 * Outputs: pose (Ftot, J, 3) floats: p after the last sweep;  err (Ftot, 3) floats: E / W at the rigid start, after stage A, and at the result
 * (the pulls do not enter E / W);  ok (Ftot), steps (Ftot) bytes or null: stage A's;  moves (Ftot) bytes or null: the accepted visits.  With
 * smooth = 0 or sweeps = 0, pose, err[:, 0:2], ok and steps are bit for bit mp_lift_fit_skeleton's.  A frame outside every take's clamped range is
 * not written.  Stage A is one launch, stage B 3 sweeps launches, one 64-lane workgroup a frame in each.
 * MP_ERR_ARG before anything is launched: what mp_lift_fit_skeleton refuses; smooth negative or not finite; sweeps out of range; scratch null,
 * not 8-byte aligned or smaller than mp_lift_fit_skeleton_smooth_scratch_bytes. */
#define MP_LIFT_SKELETON_MAXSWEEPS 64
int64_t mp_lift_fit_skeleton_smooth_scratch_bytes(int64_t Ftot, int J);
int mp_lift_fit_skeleton_smooth(const float* start, const uint8_t* start_ok, const float* kp, const float* kp_weight, int V, int64_t Ftot, int J,
                                const uint8_t* valid, const int64_t* take_offset, int G, const float* quat, const float* trans, const float* intr,
                                const float* lengths, const int32_t* parents, int distort, float sigma, float prior, int iters, float smooth,
                                int sweeps, float* pose, float* err, uint8_t* ok, uint8_t* steps, uint8_t* moves, void* scratch,
                                int64_t scratch_bytes, void* stream);

/* Standing a take on its floor: contacts, ground plane, foot skate.  Every operator above either reads which way is up from a calibration
 * (mp_lift_world's quaternion, its floor "the lowest joint on z = 0") or has no up at all (a camera's frame, the frame of estimated cameras).
 * The motion carries it: a foot that stands still is standing on something, and over a sequence those points span the floor.  This estimates, per
 * sequence, which frames each foot is in contact, the plane through the contact points - robustly, with the body's mean axis as a weak prior - the
 * rotation and shift that stand the sequence on z = foot_height, each foot's height over the plane, and how far the feet slide while in contact
 * (the foot skate: a quality measure that needs neither 3-D ground truth nor a calibration).  The reference has no counterpart.  The layout is the
 * per-sequence operators': seq_offset (S + 1) device int64, entries clamped to 0 .. Ntot, sequence s = frames [f0, f1); valid (Ntot) bytes or null;
 * fp64 between the float32 loads and the float32 stores, without contraction into fused multiply-adds; no atomics, fixed orders: identical bits on
 * every call; a sequence's result does not depend on the other sequences of the call; the call does not synchronise.  The defaults the Python layer
 * passes (radius 2, speed 0.01, sigma 0.03, prior 0.05, iters 5) are untuned.  Not measured on real data.
 * points (Ntot, J, C) read only, C = 3 or 4 (channel 3 is not read), 2 <= J <= 32: absolute joint positions in ANY rigid frame, a camera's or a
 * world; feet: nf joint indices, 1 <= nf <= MP_LIFT_GROUND_MAXFEET (host table); axis_from != axis_to: two joints whose difference points up the
 * body (pelvis, thorax); radius r in 1 .. MP_LIFT_GROUND_MAXRADIUS frames; speed > 0 in the points' unit per frame; sigma > 0 in that unit (+inf:
 * every weight is exactly 1); prior >= 0 in that unit; 0 <= iters <= MP_LIFT_GROUND_MAXITERS; foot_height in that unit.  Frame f is GOOD if
 * valid[f] != 0 (valid null: every frame); a joint of a frame is FINITE if its three coordinates are.
 * A. Contacts, per frame f and foot k with joint j = feet[k]: contact[f][k] = 1 if f - r >= f0 and f + r < f1, the frames f - r, f, f + r are
 *    good, p[.][j] is finite in all three, and with d = p[f+r][j] - p[f-r][j]:  (dx^2 + dy^2) + dz^2 <= ((2 r) speed)^2, the threshold formed in
 *    fp64 from the float32 speed.  Else 0 - the first and last r frames of a sequence, and a frame that no sequence holds, included.
 * B. Body axis: B = sum over the good frames f with p[f][axis_to] and p[f][axis_from] finite, in frame order, of d / |d|, d = p[f][axis_to] -
 *    p[f][axis_from]; a term with |d| < 1e-12 is passed over.  |B| < 1e-12 (or no term): the sequence has NO AXIS; else b = B / |B|.
 * C. The plane, iters + 1 solves over the contact points x_i = p[f][feet[k]] (frames in order, within a frame the feet in order); used = their
 *    number.  Solve 0: w_i = 1.  Solve t > 0: r_i = ((n . x_i) - offset) under the plane of solve t - 1, w_i = 1 / (1 + r_i^2 / sigma^2)^2.  A solve
 *    takes two passes:  W = sum w_i,  m = (sum w_i x_i) / W;  then C = sum w_i (x_i - m)(x_i - m)^T.  A = C - prior^2 W b b^T, the second term only
 *    with an axis and prior > 0: of the planes the data leave open - two ankles in place span a line - it picks the one most perpendicular to the
 *    body; with contacts spread over decimetres the data outweigh prior = 0.05 by orders of magnitude.  A's eigenvalues a1 <= a2 <= a3 and the
 *    eigenvector of a1 come from the symmetric 4x4 Jacobi of mp_lift_align_views on s I - A, s = tr C + prior^2 W, padded with a zero row and
 *    column (positive semidefinite; its eigenvalues are s - a).  n = that vector, normalised; with an axis and n . b != 0 its sign is the one
 *    with n . b > 0 (ok bit 1); else the first non-zero component is positive (bit 1 clear).  offset = n . m.
 *    NO PLANE: used < 3; at any solve W not > 0, a sum, m or s not finite, or  a2 - a1 <= 1e-9 max(|a1|, |a3|).
 * D. Per sequence: normal (S, 3) = n;  offset (S);  quat (S, 4) = the shortest rotation taking n onto +z, normalize(1 + n_z, n_y, -n_x, 0), and
 *    (0, 1, 0, 0) where 1 + n_z < 1e-12 - its w is never negative: canonical;  trans (S, 3) = (0, 0, foot_height - offset): with mp_lift_world's
 *    convention p' = qrot(quat, p) + trans a contact foot ends at z = foot_height, the heading and the horizontal origin stay the input frame's;
 *    rms (S) = sqrt(sum w_i r_i^2 / sum w_i), r_i under the final plane, w_i the weights of the last solve (1 for iters = 0);
 *    gap (S) = (a2 - a1) / (a3 - a1) of the last solve, 0 where a3 == a1: near 0 the contact points lie on a line and the prior or noise chose
 *    the plane, near 1 they are spread evenly;  used (S) int32;  ok (S) bytes: bit 0 a plane exists, bit 1 the body axis decided its up side.
 *    Without a plane: normal = (0, 0, 1), quat = (1, 0, 0, 0), offset, trans, rms, gap zero, ok = 0; contact, used, skate, skate_pairs all the same.
 * E. height (Ntot, nf) = (n . p[f][feet[k]]) - offset for a good frame with that joint finite in a sequence with a plane, else 0.
 *    skate (S) = the mean over the contact pairs - contact[f][k] and contact[f+1][k], both frames in the sequence - of |d - (n . d) n|,
 *    d = p[f+1][feet[k]] - p[f][feet[k]]: the in-plane length of the step, in the points' unit per frame; without a plane |d|.  0 where there is
 *    no pair.  skate_pairs (S) int32 = their number.
 * Two launches: one lane per (frame, foot) for A; one workgroup of 256 lanes per sequence for the rest - a lane sums the frames f0 + lane,
 * f0 + lane + 256, ... in order, the lanes' sums are added by a butterfly within a wave and the four waves' in wave order, every lane solves the
 * eigenproblem; the 2 (iters + 1) + 1 passes follow one another inside the workgroup.  No scratch memory.
 * MP_ERR_ARG before anything is launched: J, C, Ntot or S out of range (S > Ntot, Ntot nf > 2^31 - 1); points, seq_offset, feet or an output null;
 * nf out of range; a foot or an axis joint outside 0 .. J - 1; axis_from == axis_to; radius or iters out of range; speed not > 0 or not finite;
 * sigma not > 0; prior negative or not finite; foot_height not finite. */
#define MP_LIFT_GROUND_MAXFEET 4
#define MP_LIFT_GROUND_MAXRADIUS 8
#define MP_LIFT_GROUND_MAXITERS 8
int mp_lift_ground(const float* points, int64_t Ntot, int J, int C, const uint8_t* valid, const int64_t* seq_offset, int S, const int32_t* feet, int nf,
                   int axis_from, int axis_to, int radius, float speed, float sigma, float prior, int iters, float foot_height, float* normal,
                   float* offset, float* quat, float* trans, float* rms, float* gap, int32_t* used, uint8_t* ok, uint8_t* contact, float* height,
                   float* skate, int32_t* skate_pairs, void* stream);

/* Pinning a take's feet where they stand: leg IK on contacts.  mp_lift_ground measures how far a foot slides while it stands and moves nothing;
 * this removes the slide.  A foot in a stance run is pinned to ONE anchor point, the swing frames before and after a run are eased into and out of
 * the pin, optionally the anchors are put on the estimated floor and swing feet kept above it, and each leg is re-posed by analytic two-bone IK with
 * the frame's OWN thigh and shank lengths (a rigid sequence stays rigid); the hip and the rest of the body do not move.  The reference has no
 * counterpart.  The layout and the conventions are mp_lift_ground's: seq_offset (S + 1) device int64 clamped to 0 .. Ntot, valid (Ntot) bytes or
 * null, fp64 between the float32 loads and the float32 stores without contraction, no atomics, fixed orders (identical bits on every call), a
 * sequence's result independent of the other sequences of the call, no synchronisation.  The defaults the Python layer passes (blend 5,
 * stretch 1) are untuned.  Not measured on real data.
 * points (Ntot, J, C) read only, C = 3 or 4, 2 <= J <= 32: absolute joint positions in any rigid frame;  contact (Ntot, nf) bytes: what
 * mp_lift_ground wrote, or the caller's own;  legs (nf, 3) HOST int32, 1 <= nf <= MP_LIFT_GROUND_MAXFEET: (hip, knee, ankle) of every foot, the
 * 3 nf joints all different;  normal (S, 3), offset (S), plane_ok (S) bytes: all three or none, the floor n . x = offset; sequence s HAS A FLOOR if
 * they are given, bit 0 of plane_ok[s] is set and n and offset are finite (n is taken as a unit vector, as mp_lift_ground writes it);
 * blend B in 0 .. MP_LIFT_FOOTLOCK_MAXBLEND frames;  0 < stretch <= 1 (a float32, used in fp64).  Frame f is GOOD if valid[f] != 0 (valid null:
 * every frame), HELD if it lies in [f0, f1) of the last sequence s with seq_offset[s] <= f; a joint is FINITE if its three coordinates are.
 * seq_offset MUST NOT DECREASE (the per-sequence operators' shared assumption: the clamp keeps every access inside the Ntot frames whatever the table
 * holds, but sequences that overlap would have two waves write the same frames, and which sequence holds a frame would be undefined).
 * |v| = sqrt((vx^2 + vy^2) + vz^2), a . b = (ax bx + ay by) + az bz, h / k / a = hip / knee / ankle of leg k in the input.
 * A. Frame f, foot k is LOCKABLE if f is held and good, contact[f][k] != 0 and h, k, a are finite in f.  A RUN is a maximal stretch of consecutive
 *    lockable frames of one foot inside one sequence.  run[f][k] = the run's length inside it, 0 elsewhere; runs[s][k] = the foot's runs in s.
 * B. The run's ANCHOR = (sum of a over its frames) / length in fp64 (the sum's order is the kernel's: a tree inside every 64 frames counted from
 *    f0, the blocks in order); with a floor then A - ((n . A) - offset) n; then ROUNDED TO float32, once: the float32 is the anchor everywhere below.
 * C. The target t of every held, good (f, k) with h, k, a finite.  In a run: t = the anchor (flags bit 0).  Else t = a, and with fa the last frame
 *    of the nearest run before f and fb the first frame of the nearest run after f in the sequence (either may be missing), L = min(B + 1, fb - fa)
 *    if both exist, else B + 1:  w_prev = 1 - (f - fa) / L,  w_next = 1 - (fb - f) / L,  s(w) = (w w)(3 - 2 w);  where w_prev > 0:
 *    t = t + s(w_prev) (anchor(fa) - a[fa]);  then where w_next > 0:  t = t + s(w_next) (anchor(fb) - a[fb]);  bit 1 if either weight is > 0.
 *    (A run further than B frames away carries no weight, so B frames each way are searched.)  With a floor, outside runs: hh = (n . t) - offset;
 *    if hh < 0:  t = t - hh n  (bit 3).
 * D. Leg IK.  l1 = |k - h|, l2 = |a - k|, d = t - h, D = |d|.  l1, l2 or D below 1e-12: flags = 32 ALONE, target and moved 0, the leg keeps its
 *    bits.  Dmin = |l1 - l2|, Dmax = max(stretch (l1 + l2), Dmin), u = d / D.  D > Dmax: D' = Dmax, else D < Dmin: D' = Dmin, either way
 *    t' = h + u D' (bit 2); else D' = D, t' = t.  WHERE t' == a IN ALL THREE COORDINATES THE LEG KEEPS ITS BITS (moved 0, target a): a foot that
 *    is where it belongs is not re-posed, and without contacts out is points bit for bit.  Else the pole b = (k - h) - ((k - h) . u) u; if
 *    |b| < 1e-9 l1:  b = e - u_i u, e the unit axis i of u's smallest |component|, the first on a tie (bit 4).  x = ((D'^2 + l1^2) - l2^2) / (2 D'),
 *    y = sqrt(max(0, l1^2 - x^2)),  knee' = (h + x u) + y (b / |b|),  ankle' = t' as it is stored (not h + D' u recomputed: without a reach clamp
 *    every frame of a run carries the same ankle bits).  target = t';  moved = |ankle' - a| of the stored float32 ankle'.
 * E. out: every float of points, channel 3 included; only the knee and ankle of the legs D re-posed differ.  A frame that is not held or not
 *    good, and a foot with a leg joint that is not finite, keep their bits, with target, moved and flags 0 (run 0 too for a frame not held).
 * One copy and three launches: one WAVE per (sequence, foot) walks the frames in blocks of 64 - the lockable bits' ballot gives the run borders, a
 * segmented scan and a carry in uniform registers the sums; forward it leaves length and anchor at each run's last frame, backward it spreads
 * them over the run (run, target); then one lane per (frame, foot), first the frames outside runs (they read anchors of run frames, write their
 * own), then the frames inside (they read and write their own): no lane reads what another writes.  No scratch memory.
 * MP_ERR_ARG before anything is launched: J, C, Ntot or S out of range (S > Ntot, Ntot nf > 2^31 - 1); points, contact, seq_offset, legs or an
 * output null; out == points; nf out of range; a leg joint outside 0 .. J - 1 or named twice (in a leg or by two legs: two lanes would write it);
 * blend out of range; stretch not in (0, 1]; normal, offset, plane_ok neither all given nor all null. */
#define MP_LIFT_FOOTLOCK_MAXBLEND 32
int mp_lift_footlock(const float* points, int64_t Ntot, int J, int C, const uint8_t* valid, const int64_t* seq_offset, int S, const uint8_t* contact,
                     const int32_t* legs, int nf, const float* normal, const float* offset, const uint8_t* plane_ok, int blend, float stretch,
                     float* out, int32_t* run, float* target, float* moved, uint8_t* flags, int32_t* runs, void* stream);

/* Forward kinematics of (root, quaternions, bone lengths): the inverse of mp_lift_rotations, in the decoder's convention as that entry point states
 * it.  The reference has no counterpart.  quat (Ntot, inner, J, 4) device floats (w, x, y, z), 16-byte aligned, 2 <= J <= 32; root (Ntot, inner, 3)
 * device floats or null (the origin); lengths device floats: (S, J - 1), one row per sequence, frame g taking the row of the last s with
 * seq_offset[s] <= g (always inside 0 .. S-1, whatever the device table holds; seq_offset (S + 1) device int64), or with MP_LIFT_FK_POSE_LENGTHS
 * (Ntot, inner, J - 1), one row per pose (seq_offset and S are then not read: without mp_lift_rigid only each frame's own measured lengths close the
 * loop); parents (J) and rest (J, 3) HOST tables exactly as mp_lift_rotations takes them (parents[0] = -1, 0 <= parents[j] < j; rest row j >= 1
 * normalised here in fp64, row 0 ignored, a zero or non-finite row is MP_ERR_ARG).  Outputs: poses (Ntot, inner, J, 3) device floats, ok
 * (Ntot, inner) device bytes.  Per pose, on its own, fp64 between the float32 loads and stores:
 * 1. Every quaternion must be USABLE: n2 = |q|^2 in fp64 finite and >= 1e-12 (the rule of a take's quaternions everywhere in this library).  If one
 *    of the pose's J is not: every joint gets the root's float32 bits (+0 without a root) and ok = 0.
 * 2. Otherwise u[j] = q[j] / sqrt(n2[j]);  Rw[0] = u[0],  Rw[j] = Rw[parent] u[j];  p[0] = root,  p[j] = p[parent] + Rw[j] (len_j rest_j) for
 *    j = 1 .. J-1 in order;  poses[j] = (float) p[j],  ok = 1.  len_j is used as it is stored (a negative or non-finite length gives IEEE results).
 * mp_lift_fk(mp_lift_rotations(p), the measured lengths of p, p[0]) is p again to float32 rounding.  One lane per (pose, joint); a lane fetches its
 * parent's world rotation (a quaternion) and position by wavefront shuffles, level by level.  No atomics, no LDS, a fixed order: identical bits on
 * every call; a pose depends on no other pose.  The call does not synchronise.
 * MP_ERR_ARG before anything is launched: quat, lengths, rest, parents, poses or ok null; seq_offset null without MP_LIFT_FK_POSE_LENGTHS; another
 * flag; J, Ntot, inner or S out of range (S > Ntot); quat not 16-byte aligned; poses overlapping quat; a bad parent table or rest row; more work
 * than one grid holds. */
#define MP_LIFT_FK_POSE_LENGTHS 1
int mp_lift_fk(const float* quat, const float* root, const float* lengths, int64_t Ntot, int inner, int J, const int64_t* seq_offset, int S,
               const int32_t* parents, const float* rest, int flags, float* poses, uint8_t* ok, void* stream);

/* A take resampled in time on its rotations: every output frame samples its sequence at a fractional input time, on SO(3) for the joints and
 * linearly for the root, by interpolation (radius 0) or by mp_lift_smooth's weighted local polynomial evaluated at that time (radius >= 1).  What
 * comes out is again (root, quat), so with mp_lift_fk and the take's ONE bone table the retimed positions have exactly the take's bones - averaging
 * or interpolating POSITIONS shortens a bone by 1 - cos(theta / 2) at the midpoint of two directions theta apart.  The reference has no counterpart.
 * quat (Ntot, inner, J, 4) device floats (w, x, y, z), 2 <= J <= 32; root (Ntot, inner, 3) or null; valid (Ntot, inner) bytes or null (every frame
 * valid); seq_offset (S + 1) device int64, the input frames [f0, f1) of every sequence clamped to 0 .. Ntot (n = f1 - f0); out_offset (S + 1) device
 * int64, its output frames, clamped to 0 .. Mtot; clock (S, 3) device DOUBLES (start, num, den), num and den holding integers (output and input
 * frames per unit of time); radius R in 0 .. MP_LIFT_SMOOTH_MAXR, degree 0..2, taper 0 (uniform) or 1 (biweight).  Outputs: quat_out
 * (Mtot, inner, J, 4), root_out (Mtot, inner, 3) (null exactly when root is), ok and taps (Mtot, inner) bytes.  quat and quat_out 16-byte aligned.
 * Output frame g belongs to the last sequence s with out_offset[s] <= g (always inside 0 .. S-1).  If g lies outside that sequence's clamped output
 * range, or n = 0: identity quaternions (1, 0, 0, 0), root 0, ok = 0, taps = 0.  Otherwise with h = g - (the sequence's first output frame):
 *   t = start + (h den) / num  in fp64 (the product an exact integer, ONE division; num <= 0 or NaN counts as 1), in input frames from f0;
 *   t is clamped into [0, n - 1] (a NaN to 0), and ok gets the value 2 added where it was.
 * log(r): s = |r.xyz|; 0 where s == 0, else 2 atan2(s, r.w) r.xyz / s.   exp(v): a = |v|; (1, 0, 0, 0) where a == 0, else (cos(a / 2),
 * sin(a / 2) v / a).   u(k) = q_k / |q_k| in fp64.
 * R = 0, interpolation.  k = floor(t), al = t - k.
 *   al == 0 exactly (every integer t, t = n - 1 included): frame k is copied BIT FOR BIT, its quaternions as stored and its root; ok = (valid[k] != 0),
 *   taps = 1.  With start = 0 and num = den the operator is the identity on every valid frame, bit for bit.
 *   Otherwise (k + 1 <= n - 1) both frames must be valid; if not: identities, root 0, ok = 0, taps = 0 - nothing is filled in this mode.  Else
 *   a = u(k), b = u(k + 1) negated where dot(a, b) < 0,  q = a exp(al log(conj(a) b)): the short-way slerp, in the hemisphere of q_k as stored, so
 *   a sign-continuous track stays one;  root = (1 - al) r_k + al r_(k+1);  ok = 1, taps = 2.
 * R >= 1, fit.  The taps are the frames k in 0 .. n-1 with |k - t| <= R and valid[k] != 0, cnt of them (taps = cnt).  cnt = 0: identities, root 0,
 *   ok = 0.  Else ok = 1 and  u_k = (k - t) / R,  w_k = 1 (uniform) or (1 - ((k - t) / (R + 1))^2)^2 (biweight);  d = min(degree, cnt - 1), or d = 0
 *   when no tap has k <= t or none has k >= t (not bracketed: held, never extrapolated);  c_k = w_k (a0 + a1 u_k + a2 u_k^2), (a0, a1, a2) the first
 *   row of the inverse of the (d + 1) x (d + 1) normal matrix [sum w u^(i+j)] by cofactors, exactly mp_lift_smooth's with its integer tau replaced by
 *   k - t; all sums over the taps in increasing k; c_k is computed once per (output frame, inner index) and shared by the root and the J joints.
 *   k* = the tap nearest to t, the lower one on a tie.  Per joint:  v_k = log(conj(u(k*)) (+-u(k))), the sign that makes dot(u(k*), +-u(k)) >= 0;
 *   q = u(k*) exp(sum_k c_k v_k).  Per root coordinate: sum_k c_k r_k (at an integer t mp_lift_smooth's sum).  A rotation at constant angular
 *   velocity about a fixed axis is reproduced for degree >= 1 (its v_k are linear in k); two taps with degree 1 are the slerp above.
 * All arithmetic between the float32 loads and stores is fp64; a computed zero component is stored as +0.  A non-finite or zero quaternion on a
 * valid tap gives IEEE results in the output frames that read it; an invalid tap's value never enters the arithmetic.  clock and out_offset are
 * device data no host check sees: whatever they hold, nothing outside the arrays is read or written (seq_offset and out_offset MUST NOT DECREASE for
 * the result to be the one stated here: which sequence holds a frame is found by bisection).  One lane per (output pose, joint); no atomics,
 * no LDS, fixed orders: identical bits on every call; a sequence's result does not depend on the other sequences.  The call does not synchronise.
 * MP_ERR_ARG before anything is launched: quat, seq_offset, out_offset, clock, quat_out, ok or taps null; root and root_out not both null or both
 * given; an output overlapping an input or another output; radius, degree, taper, J, Ntot, Mtot, inner or S out of range (S > Ntot); quat or
 * quat_out not 16-byte aligned; more work than one grid holds. */
int mp_lift_retime(const float* quat, const float* root, const uint8_t* valid, int64_t Ntot, int inner, int J, const int64_t* seq_offset,
                   const int64_t* out_offset, const double* clock, int S, int64_t Mtot, int radius, int degree, int taper, float* quat_out,
                   float* root_out, uint8_t* ok, uint8_t* taps, void* stream);

/* Euler channels of a take's joint rotations, for export as a BONE-CENTRED joint hierarchy (BVH, manipose_amd/bvh.py): bone j >= 1 gets a node that
 * sits at its PARENT joint, carries exactly q[j] and has its child end len_j rest_j away, so the node's world rotation is the decoder's Rw[j] and
 * every joint position comes out as mp_lift_fk's, with no approximation and no twist estimate.  The reference has no counterpart.
 * quat (Ntot, inner, J, 4) device floats (w, x, y, z), 16-byte aligned, 2 <= J <= 32; root (Ntot, inner, 3) or null; valid (Ntot, inner) bytes or
 * null (every frame valid); seq_offset (S + 1) device int64, a sequence's frames [f0, f1) clamped to 0 .. Ntot as in mp_lift_retime, frame g
 * belonging to the last s with seq_offset[s] <= g (always inside 0 .. S-1); basis (S, 4) and shift (S, 3) device floats or both null (identity,
 * zero): a rigid transform per sequence in mp_lift_world's convention, p' = qrot(basis, p) + shift; scale a finite float > 0; order 0..5 for XYZ,
 * XZY, YXZ, YZX, ZXY, ZYX; flags 0 or MP_LIFT_EULER_CONTINUOUS.  Outputs: angles (Ntot, inner, J, 3) floats, DEGREES in channel order; pos
 * (Ntot, inner, 3), null exactly when root is; ok (Ntot, inner) bytes.
 * FIRST PASS, per pose, on its own; all arithmetic between the float32 loads and stores is fp64 with contraction off.  A quaternion is USABLE where
 * n2 = |q|^2 is finite and >= 1e-12.  If one of the pose's J quaternions is not usable, or valid of the frame is 0, or basis of its sequence is
 * not usable: every angle +0, pos +0, ok = 0.  Otherwise u[j] = q[j] / sqrt(n2[j]); u[0] := unit(basis) u[0] (the quaternion product, basis on
 * the LEFT); R the matrix of u[j] (1 - 2 (y^2 + z^2), 2 (x y - w z), ... row-major).  The order names the axes (i, j, k), s = +1 where
 * (j - i) mod 3 == 1, else -1; the angles (al, be, ga) satisfy R = R_i(al) R_j(be) R_k(ga), the channel convention of BVH:
 *   c2 = R[j][k]^2 + R[k][k]^2;  be = asin(clamp(s R[i][k], -1, 1));
 *   regular, c2 >= 1e-12:  al = atan2(-s R[j][k], R[k][k]),  ga = atan2(-s R[i][j], R[i][i]);
 *   gimbal,  c2 <  1e-12:  al = atan2(s R[k][j], R[j][j]),   ga = 0,  and ok gets 2 added (once per pose, whichever joint it was).
 * pos = (float)(scale * (qrot(unit(basis), root) + shift)), qrot by the matrix of unit(basis), row sums left to right.  An angle is multiplied by
 * 57.29577951308232 (the double nearest to 180 / pi) and rounded to float32 once; a float32 zero, -0 of a negative value that underflowed included,
 * is stored as +0 (angles and pos, in both passes); ok = 1 (or 3).
 * SECOND PASS, MP_LIFT_EULER_CONTINUOUS: per track (sequence, inner index, joint) over the sequence's clamped frames, decided ON THE FLOAT32 ANGLES
 * AS THE FIRST PASS STORED THEM, in fp64, so that the rule applied to the first pass's output gives the second pass's bits.  c[g] the stored triple;
 * T(x) = (x0 + 180, 180 - x1, x2 + 180), the other Euler solution of the same rotation;  w(x) = x - 360 floor((x + 180) / 360), in [-180, 180);
 * d(x, y) = (|w(x0 - y0)| + |w(x1 - y1)|) + |w(x2 - y2)|.  The PREDECESSOR g' of frame g is the last frame before g in the sequence with
 * ok != 0; a frame with ok = 0 keeps its zeros and is transparent.
 *   branch: no predecessor: flip[g] = 0; else flip[g] = flip[g'] XOR (d(c[g], T(c[g'])) < d(c[g], c[g'])).  d is unchanged when T is applied to
 *     both arguments, so this is the greedy choice "the solution nearer to what was chosen for the frame before", as a prefix parity.
 *   e[g] = flip[g] ? T(c[g]) : c[g].
 *   turns, per channel: no predecessor: W[g] = 0; else W[g] = W[g'] - rint((e[g] - e[g']) / 360), rint rounding a tie to even.
 *   stored: (float)(e[g] + 360 W[g]), the sum in fp64 (a zero as +0).
 * Both scans are integer, exact and associative: the result does not depend on how the frames are cut into chunks; a sequence's result depends on
 * no other sequence; identical bits on every call.  One lane per (pose, joint), then one wave per track, 64 frames at a time; no atomics, no LDS.
 * seq_offset is device data no host check sees: whatever it holds, nothing outside the arrays is read or written (it MUST NOT DECREASE for the
 * result to be the one stated here).  The call does not synchronise.
 * MP_ERR_ARG before anything is launched: quat, seq_offset, angles or ok null; root and pos not both null or both given; basis and shift not both
 * null or both given; order, flags, scale, J, Ntot, inner or S out of range (S > Ntot); quat not 16-byte aligned; an output overlapping an input
 * or another output; more work than one grid holds. */
#define MP_LIFT_EULER_CONTINUOUS 1
int mp_lift_euler(const float* quat, const float* root, const uint8_t* valid, int64_t Ntot, int inner, int J, const int64_t* seq_offset, int S,
                  const float* basis, const float* shift, float scale, int order, int flags, float* angles, float* pos, uint8_t* ok, void* stream);

/* Dataset ingest: the raw arrays of the reference's on-disk formats -> the resident sequences mp_gather_windows reads.
 * mp_ingest_pose3d: raw (frames_raw, raw_joints, 3) device floats; frames (N) device int32 or null (null: the first N raw frames;
 * otherwise the raw frame of every output frame - temporal stride, valid-frame selection); joint_map (J <= 32) HOST int32 or null:
 * raw joint of every output joint.  out[n][j] = (T(raw[map[j]] - raw[root_raw]) - T(raw[map[root_out]])) / divisor, where a negative
 * root index drops its term and T is the world-to-camera transform qrot(qinverse(orientation), . - translation) when
 * orientation (4, w-first, HOST) / translation (3, HOST) are given, identity when both are null.
 *   Human3.6M (hpe/mh_so3_hpe/data/h36m_lifting.py:620-660 joint selection; data/utils.py:29-58 read_3d_data;
 *   data/camera.py:24-28; data/quaternion.py:6-31): map = the 17 kept joints, camera given, root_raw -1, root_out 0, divisor 1.
 *   MPI-INF-3DHP (data/dataset_3dhp.py:153-176,185-203): map = MAP_H36M_TO_MPI_JOINTS, no camera, root_raw 14, root_out -1,
 *   divisor 1000, frames = the valid test frames.
 * mp_ingest_pose2d: raw (frames_raw, raw_joints, raw_channels >= 2) pixel keypoints -> out (N, J, 2) = X / w * 2 - [1, h / w]
 * (data/camera.py:9-14 as called by data/utils.py:9-26 and dataset_3dhp.py:170-175,212-224; the subtraction runs in double as in
 * the reference, where a float64 list is subtracted from the float32 array). */
int mp_ingest_pose3d(const float* raw, int raw_joints, const int32_t* frames, int64_t N, const int32_t* joint_map, int J,
                     const float* orientation, const float* translation, int root_raw, int root_out, float divisor, float* out,
                     void* stream);
int mp_ingest_pose2d(const float* raw, int raw_joints, int raw_channels, const int32_t* frames, int64_t N, const int32_t* joint_map,
                     int J, float res_w, float res_h, float* out, void* stream);

/* Evaluation analytics of pose sequences in one pass over the frames (17-joint H36M / 3DHP tree compiled in): the running sums
 * behind mpjpe_error / mse_error / jointwise_error / segments_len_err (hpe/mh_so3_hpe/metrics/mean_joint_errors.py:31-130),
 * sagittal_symmetry(_per_bone) and segments_time_consistency(_per_bone) (metrics/regularizations.py:8-157), the evaluation form of
 * mean_velocity_error (metrics/losses.py:75-101) and keypoint_3d_pck / keypoint_3d_auc (metrics/pck.py:92-199; alignment 'none',
 * or 'scale' with scale_align = 1).  pred / gt are addressed through ELEMENT strides of (b, t, j, c), so the reference's
 * (B,3,J,L) permutations need no copy; gt (and its strides) may be null for the prediction-only metrics; mask: (B,L,J) bytes or null.
 * out: (B, mp_pose_metrics_row_floats()) sums per batch item, laid out as
 *   [0] sum ||e||  [1] sum ||e||^2  [2] sum_pairs |l-r|  [3] sum_pairs (l-r)^2  [4] sum_bones |gt-pred|  [5] sum_bones (gt-pred)
 *   [6] #(||e|| < pck_threshold)  [7] sum_j #(AUC thresholds i*auc_max/(auc_steps-1) above ||e||)  [8] #visible joints
 *   [9] sum ||d_t pred - d_t gt||  [10] the same squared  [11] frames;
 *   then per bone k (16): sum (len-len0), sum (len-len0)^2, sum |gt-pred|, sum (gt-pred);  per left/right pair (6): sum |l-r|,
 *   sum (l-r)^2;  per joint (17): sum ||e||, sum ||e||^2.   len0: (B,16) bone lengths of frame 0 (the shift of the variance sums).
 * scratch: >= B * ceil(L/128) * row_floats floats. */
int mp_pose_metrics_row_floats(void);
/* segments_len_err(..., mode="no_agg") (metrics/mean_joint_errors.py:83-130): out (B*L, 16) = ground-truth minus predicted bone length per
 * frame and bone (absolute value unless signed_diff); strides as in mp_pose_metrics. */
int mp_bone_length_table(const float* pred, const int64_t* pred_strides, const float* gt, const int64_t* gt_strides, int B, int L, int signed_diff,
                         float* out, void* stream);
int mp_pose_metrics(const float* pred, const int64_t* pred_strides, const float* gt, const int64_t* gt_strides, const uint8_t* mask, int B,
                    int L, int J, float pred_scale, float gt_scale, float pck_threshold, float auc_max, int auc_steps, int scale_align,
                    float* out, float* len0, float* scratch, int64_t scratch_floats, void* stream);

/* The evaluation quantities that are not sums (17-joint tree compiled in; bone k = (joint k+1, its parent)): per bone the smallest and the
 * largest length over all B*L frames (segments_max_strech_per_bone, metrics/regularizations.py:63-74), the largest |len(f) - len(f-1)| with
 * the index of the FIRST difference that attains it (segments_max_diff_strech_per_bone, :77-94; torch.max(dim) returns the first maximum),
 * and the sums over all frames and joints of |gt - pred| per coordinate (coordwise_error, metrics/mean_joint_errors.py:133-141).  pred / gt
 * are addressed through element strides of (b, t, j, c) as in mp_pose_metrics; a length is sqrtf(dx^2 + dy^2 + dz^2) of the scaled
 * coordinates.  gt, gt_strides and coord_sums (3 floats) may be null together.
 * chain = 0: differences inside every batch item only, index b (L-1) + t of the difference between frames t and t+1 of item b - the
 *   reference function on a (B,3,J,L) tensor.
 * chain = 1: the B*L frames are ONE sequence (the last frame of item b is followed by frame 0 of item b+1: the reference's (1,3,J,B*L)
 *   reshape, main_h36m_lifting.py:1061-1085); the difference between frames f-1 and f has index frame_base + f - 1; with prev_len (16 floats
 *   on the device, or null) frame 0 is differenced against it.  last_len (16 floats) receives the bone lengths of the last frame: pass it
 *   as prev_len of the next call, with frame_base advanced by B*L, and a sequence can be fed in pieces with the result of one call.
 * Outputs, on the device: min_len, max_len, max_delta (16 floats each), max_delta_idx (16 int64); without any difference (one frame and no
 * prev_len, or chain = 0 with L = 1) max_delta is -1 and the index -1.  Deterministic (no atomics): the same bits in every run.
 * scratch: >= mp_bone_extremes_scratch_floats(B*L) floats, 8-byte aligned. */
int64_t mp_bone_extremes_scratch_floats(int64_t frames);
int mp_bone_extremes(const float* pred, const int64_t* pred_strides, const float* gt, const int64_t* gt_strides, int B, int L, int J,
                     float pred_scale, float gt_scale, int chain, const float* prev_len, int64_t frame_base, float* min_len, float* max_len,
                     float* max_delta, int64_t* max_delta_idx, float* coord_sums, float* last_len, float* scratch, int64_t scratch_floats,
                     void* stream);

/* The multi-hypothesis study of K hypotheses, their scores and the target in one pass (17 joints): what the reference's follow-up scripts
 * compute on the host from all_pred_hyps.pkl - calc_jbest_mpjpe / calc_jbest_pose (hpe/useful_aux_scripts/eval_baselines.py:451-481), the
 * error against the number of hypotheses (plot_nhyps_lineplot.py), the per-joint spread (inspect_multimodality.py) - and the oracle /
 * best_score / weighted_ave aggregations of RMCLManifoldMixSTE.aggregate (rmcl_manifold_mix_ste.py:141-185) with mpjpe_error, without
 * test-time augmentation.  poses (B,K,T,17,3), scores (B,K,T), target (B,T,17,3), contiguous; 1 <= K <= 8, T >= 1, B*T < 2^31.
 * Per frame, with q_k = pose_scale * p_k and g = target_scale * target:  e[k][j] = ||q_k[j] - g[j]|| (sqrtf of the scaled coordinates),
 * E[k] = sum_j e[k][j];  k* = the FIRST arg-min of E (torch.min), k_s = the FIRST arg-max of the score; the score order is descending,
 * equal scores in the order of their indices; per joint the FIRST arg-min over k of e[k][j] wins.
 * sums: mp_hypothesis_stats_row_floats() floats, every entry a sum over the B*T frames:
 *   [0] frames  [1] E[k_s] (pseudo-oracle)  [2] E[k*] (oracle, "P-Best")  [3] sum_j min_k e[k][j] (J-Best)
 *   [4] sum_j ||sum_k s_k q_k[j] - g[j]|| (weighted average)  [5] s[k*]  [6] s[k_s]
 *   [7] 2 / (K (K-1)) sum_{k<k'} sum_j ||q_k[j] - q_k'[j]|| (mean pairwise distance; 0 for K = 1)
 *   [8,16) top-m: min of E over the m best-scored hypotheses, m = 1..K, slots K.. are 0 ([8] = [1], [8+K-1] = [2], the same bits)
 *   [16,33) per joint: min_k e[k][j]    [33,50) per joint: sqrt(sum_k s_k ||q_k[j] - w[j]||^2), w = sum_k s_k q_k
 *   [50,58) per head k: s_k (slots K.. are 0).
 * counts: mp_hypothesis_stats_row_counts() int64, exact:
 *   [0] frames with k_s == k*   [1,9) place of k* in the score order (0 = best-scored)   [9,17) k*   [17,25) k_s
 *   [25,33) (frame, joint) pairs whose per-joint winner is head k.
 * jbest_pose (B,T,17,3) or null: per joint the three input floats of the winning hypothesis, UNSCALED (the bits of `poses`);
 * jbest_idx (B,T,17) bytes or null: that hypothesis.  Deterministic (no atomics): the same bits in every run.
 * scratch: >= mp_hypothesis_stats_scratch_floats(B*T) floats; counts 8-byte aligned. */
int64_t mp_hypothesis_stats_scratch_floats(int64_t frames);
int mp_hypothesis_stats_row_floats(void);
int mp_hypothesis_stats_row_counts(void);
int mp_hypothesis_stats(const float* poses, const float* scores, const float* target, int B, int K, int T, float pose_scale, float target_scale,
                        float* sums, int64_t* counts, float* jbest_pose, uint8_t* jbest_idx, float* scratch, int64_t scratch_floats,
                        void* stream);

/* Procrustes-aligned errors: per frame the similarity transform (scale, proper rotation, translation) taking the predicted joints onto
 * the target ones in the least-squares sense - p_mpjpe (hpe/mh_so3_hpe/metrics/mean_joint_errors.py:148-189, batched numpy SVD on the
 * host in the reference) and the 'procrustes' alignment of keypoint_3d_pck / keypoint_3d_auc (metrics/pck.py:5-60,127-131) - solved on
 * the device with Horn's quaternion closed form (thread per frame, 4x4 Jacobi).  pred, gt: (N,17,3) contiguous; mask (N,17) bytes or
 * null.  out[5]: sum of aligned per-joint errors, #(error < pck_threshold), sum of AUC threshold counts, #visible joints, frames.
 * scratch: >= 5 * ceil(N/256) floats. */
int mp_procrustes_errors(const float* pred, const float* gt, const uint8_t* mask, int64_t N, int J, float pred_scale, float gt_scale,
                         float pck_threshold, float auc_max, int auc_steps, float* out, float* scratch, int64_t scratch_floats, void* stream);

/* test / tuning hooks (no reference counterpart; process-wide, they select between kernels that the GPU tests hold to the same results):
 * "gemm_small_tile" (1 = 128x128 GEMM tiles everywhere), "gemm_persist_min_tiles" (output-tile count from which the persistent GEMM
 * kernels are used; 0 = default), "gemm_persist_mode" (0 tiled kernels only, 1 = default: persistent kernel where it applies),
 * "gemm_persist_wgs" (workgroups = CUs the persistent GEMMs occupy; 0 = default: all), "gemm_tile" (0 = default: mp_gemm_plan's planner
 * chooses the tile; 128 / 256 = that tile wherever the operand form has it - "gemm_small_tile" never applied to f16f8, this does; any other
 * value: MP_ERR_ARG), "attn_two_phase" (0 = the one-strip-at-a-time
 * split-precision temporal attention forward for every shape; 1 = default: the two-phase kernel for head dim 64 and T > 128),
 * "heads_mfma" (0 = row kernels for the output heads, 1 = default: matrix cores wherever covered, 2 = only from 16 outputs up).
 * Everything that changes a model's arithmetic or stream use is a field of mp_model_config. */
int mp_set_option(const char* name, int value);
/* Which GEMM kernel serves a Linear of M tokens, N outputs and K inputs (the planner every launch goes through; host-only, no HIP call when
 * cus > 0; cus == 0 asks the current device for its CU count).  form: 0 bf16, 1 bf16x3, 8 f16f8, 16 fp16; epilogue: 0 bias, 1 GELU, 2 residual,
 * 3 gelu'-multiplying dgrad, 4 weight-gradient slabs (the layouts are the engine's for that epilogue).
 * out = {tile (128 or 256), persistent (0 / 1), workgroups, tiles = ceil(M / tile) * ceil(N / tile)}.  The 256 x 256 tile runs one 8-wave workgroup
 * per CU, the 128 x 128 tile two 4-wave ones: the planner compares ceil(tiles256 / cus) rounds of cost 4 with ceil(tiles128 / (2 cus)) rounds of
 * the measured cost c of a small tile and takes the small tile only where the large one leaves CUs idle - the batch sizes
 * of a few windows.  It honours the "gemm_*" options.  A shape no kernel of that form serves (f16f8: N % 256, K % 64, K >= 128): MP_ERR_ARG. */
int mp_gemm_plan(int M, int N, int K, int form, int epilogue, int cus, int out[4]);
/* Process-wide counts of GEMM launches since the last reset, by kernel family: out = {persistent 256 x 256, tiled 256 x 256, tiled 128 x 128}.
 * Plain host counters (no device work); reset != 0 zeroes them after reading.  Tests use it to prove which kernel ran. */
int mp_gemm_launch_counts(int64_t out[3], int reset);

#ifdef __cplusplus
}
#endif
#endif /* MANIPOSE_HIP_H */

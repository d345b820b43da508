// extern "C" shims of the stand-alone operators declared in include/manipose_hip.h
#include <string.h>
#include "common.h"
#include "kernels.h"
#include "../../include/manipose_hip.h"

namespace mp {
const char* last_error();
long wgrad_f32_slab_floats(int Mtok, int Nout, int Kin);
}
using namespace mp;

static LossCfg to_cfg(const mp_loss_config* c) {
  LossCfg l;
  l.beta = c->rmcl_score_reg; l.vel_w = c->vel_loss; l.smooth_w = c->smooth_reg; l.use_joint_weights = c->w_loss; l.squared = c->sq_loss;
  for (int j = 0; j < 17; ++j) l.joint_weights[j] = c->joint_weights[j];
  return l;
}

// The ten attention entry points: check, fill the argument block (kernels.h AttnArgs), call.  `who` names the entry point in the messages; a
// plain entry point is its _ex / _scale_ex form at the defaults, which pass those forms' further checks.
static int attention_fwd(const char* who, int form, const void* qkv, void* out, float* lse, int temporal, int B, int T, int J, int C, int H,
                         float qk_scale, void* stream) {
  MP_CHECK(qkv && out && (!temporal || lse), MP_ERR_ARG, "%s: null pointer", who);
  MP_CHECK(qk_scale >= 0.f && qk_scale <= 3.0e38f, MP_ERR_ARG, "%s: qk_scale must be finite and >= 0 (0 = head_dim ** -0.5)", who);
  AttnArgs a = {};
  a.qkv = qkv; a.out = out; a.lse = lse; a.B = B; a.T = T; a.J = J; a.C = C; a.H = H; a.form = form; a.scale = qk_scale;
  return attn_fwd(a, temporal, (hipStream_t)stream);
}
static int attention_bwd(const char* who, int form, const void* qkv, const void* out, const void* d_out, const float* lse, float* delta, void* d_qkv,
                         int temporal, int B, int T, int J, int C, int H, int out_f16, float qk_scale, const float* grad_scale, void* stream) {
  MP_CHECK(qkv && d_out && d_qkv && (!temporal || (out && lse && delta)), MP_ERR_ARG, "%s: null pointer", who);
  MP_CHECK(!out_f16 || temporal, MP_ERR_ARG, "%s: only the temporal backward reads O", who);
  MP_CHECK(qk_scale >= 0.f && qk_scale <= 3.0e38f, MP_ERR_ARG, "%s: qk_scale must be finite and >= 0 (0 = head_dim ** -0.5)", who);
  if (grad_scale != nullptr) {      // the row kernels know no fp16 store (attn_bwd refuses too; this message names the shape as the caller gave it)
    const bool mfma = H > 0 && C % H == 0 && C % 8 == 0 && (temporal ? attn_tmfma_supported(T, C / H) : attn_smfma_supported(J, C / H, H));
    MP_CHECK(mfma, MP_ERR_ARG, "%s: scaled fp16 gradients need an MFMA backward (temporal %d, T=%d J=%d C=%d H=%d)", who, temporal, T, J, C, H);
  }
  AttnArgs a = {};
  a.qkv = qkv; a.out = const_cast<void*>(out); a.dout = d_out; a.dqkv = d_qkv; a.lse = const_cast<float*>(lse); a.delta = delta;
  a.B = B; a.T = T; a.J = J; a.C = C; a.H = H; a.form = form; a.scale = qk_scale; a.grad_f16 = grad_scale; a.out_f16 = out_f16;
  return attn_bwd(a, temporal, (hipStream_t)stream);
}
static int attention_fwd_x3(const char* who, const char* bad, const void* qkv_hi, const void* qkv_lo, void* out_hi, void* out_lo, float* lse, float* scratch,
                            int temporal, int B, int T, int J, int C, int H, int out_form, float qk_scale, void* stream) {
  MP_CHECK(qkv_hi && qkv_lo && out_hi && out_lo && (!temporal || lse) && (out_form == 0 || out_form == 1), MP_ERR_ARG, "%s: %s", who, bad);
  MP_CHECK(qk_scale >= 0.f && qk_scale <= 3.0e38f, MP_ERR_ARG, "%s: qk_scale must be finite and >= 0 (0 = head_dim ** -0.5)", who);
  AttnArgs a = {};
  a.qkv = qkv_hi; a.qkv_lo = qkv_lo; a.out = out_hi; a.out_lo = out_lo; a.lse = lse; a.scratch = scratch;
  a.B = B; a.T = T; a.J = J; a.C = C; a.H = H; a.form = ATTN_BF16X3; a.scale = qk_scale; a.out_f16f8 = out_form;
  return attn_fwd(a, temporal, (hipStream_t)stream);
}

extern "C" {

int mp_abi_version(void) { return MP_ABI_VERSION; }
const char* mp_last_error(void) { return mp::last_error(); }

int mp_fk_decode_fwd(const float* rot6d, int rot_stride, int rot_dim, const float* lengths, float* poses, int B, int K, int T,
                     void* stream) {
  MP_CHECK(rot6d && lengths && poses, MP_ERR_ARG, "mp_fk_decode_fwd: null pointer");
  return fk_decode_fwd(rot6d, rot_stride, rot_dim, lengths, poses, B, K, T, (hipStream_t)stream);
}
int mp_fk_decode_bwd(const float* rot6d, int rot_stride, int rot_dim, const float* lengths, const float* d_poses, float* d_rot6d,
                     float* d_len_pose, int B, int K, int T, void* stream) {
  MP_CHECK(rot6d && lengths && d_poses && d_rot6d && d_len_pose, MP_ERR_ARG, "mp_fk_decode_bwd: null pointer");
  return fk_decode_bwd(rot6d, rot_stride, rot_dim, lengths, d_poses, d_rot6d, d_len_pose, B, K, T, (hipStream_t)stream);
}

int mp_wta_loss(const float* poses, const float* scores, const float* target, const mp_loss_config* cfg, float* terms,
                int32_t* argmin, float* d_poses, float* d_scores, int B, int K, int T, float* scratch, int64_t scratch_floats,
                void* stream) {
  MP_CHECK(poses && scores && target && cfg && terms && scratch, MP_ERR_ARG, "mp_wta_loss: null pointer");
  return wta_loss(poses, scores, target, to_cfg(cfg), terms, argmin, d_poses, d_scores, B, K, T, scratch, scratch_floats,
                  (hipStream_t)stream);
}
int mp_single_loss(const float* poses, const float* target, const mp_loss_config* cfg, float* terms, float* d_poses, int B, int T,
                   float* scratch, int64_t scratch_floats, void* stream) {
  MP_CHECK(poses && target && cfg && terms && scratch, MP_ERR_ARG, "mp_single_loss: null pointer");
  return single_loss(poses, target, to_cfg(cfg), terms, d_poses, B, T, scratch, scratch_floats, (hipStream_t)stream);
}
int mp_rigid_segments_loss(const float* poses, float weight, float* term, float* d_poses, int B, int T, float* scratch, int64_t scratch_floats,
                           void* stream) {
  return rigid_segments_loss(poses, weight, term, d_poses, B, T, scratch, (long)scratch_floats, (hipStream_t)stream);
}

int mp_aggregate(const float* poses, const float* scores, const float* target, int mode, float* out, int B, int K, int T,
                 void* stream) {
  MP_CHECK(poses && out, MP_ERR_ARG, "mp_aggregate: null pointer");
  return aggregate_poses(poses, scores, target, mode, out, B, K, T, (hipStream_t)stream);
}
int mp_mpjpe_sum(const float* pred, const float* target, int64_t n_joints, float* out_sum, float* scratch, int64_t scratch_floats,
                 void* stream) {
  MP_CHECK(pred && target && out_sum && scratch && n_joints > 0, MP_ERR_ARG, "mp_mpjpe_sum: bad argument");
  return mpjpe_sum(pred, target, n_joints, out_sum, scratch, scratch_floats, (hipStream_t)stream);
}
int mp_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, int step, float lr, float beta1,
                 float beta2, float eps, float weight_decay, float grad_scale, void* stream) {
  MP_CHECK(params && grads && exp_avg && exp_avg_sq && n > 0, MP_ERR_ARG, "mp_adam_step: bad argument");
  return adam_step(params, grads, exp_avg, exp_avg_sq, n, step, lr, beta1, beta2, eps, weight_decay, grad_scale,
                   (hipStream_t)stream);
}

int mp_adam_step_scaled(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, int step, float lr, float beta1,
                        float beta2, float eps, float weight_decay, float grad_scale, const float* lr_mult, const float* wd_mult, void* stream) {
  MP_CHECK(params && grads && exp_avg && exp_avg_sq && lr_mult && wd_mult && n > 0, MP_ERR_ARG, "mp_adam_step_scaled: bad argument");
  return adam_step(params, grads, exp_avg, exp_avg_sq, n, step, lr, beta1, beta2, eps, weight_decay, grad_scale, (hipStream_t)stream, lr_mult,
                   wd_mult);
}

int mp_layernorm_fwd(const float* x, const float* gamma, const float* beta, float eps, float* y, float* stats, int M, int C,
                     void* stream) {
  MP_CHECK(x && gamma && beta && y && stats, MP_ERR_ARG, "mp_layernorm_fwd: null pointer");
  LnFwdArgs a = {};
  a.x = x; a.M = M; a.C = C; a.g2 = gamma; a.b2 = beta; a.eps2 = eps; a.y2 = y; a.stats2 = stats;
  return ln_fwd(a, 0, (hipStream_t)stream);
}
int mp_layernorm_bwd(const float* dy, const float* x, const float* stats, const float* gamma, const float* dskip, float* dx,
                     float* dgamma, float* dbeta, int M, int C, float* scratch, int64_t scratch_floats, void* stream) {
  MP_CHECK(dy && x && stats && gamma && dx && dgamma && dbeta && scratch, MP_ERR_ARG, "mp_layernorm_bwd: null pointer");
  return ln_bwd(dy, 0, x, stats, gamma, dskip, dx, nullptr, nullptr, 0, 1, 1, dgamma, dbeta, M, C, scratch, scratch_floats, (hipStream_t)stream);
}

int mp_linear_fwd(const float* x, const float* W, const float* b, float* y, float* z, const float* r, int M, int N, int K,
                  int epilogue, void* stream) {
  MP_CHECK(x && W && y, MP_ERR_ARG, "mp_linear_fwd: null pointer");
  MP_CHECK(epilogue >= 0 && epilogue <= 2, MP_ERR_ARG, "mp_linear_fwd: epilogue %d", epilogue);
  MP_CHECK(epilogue != 1 || z, MP_ERR_ARG, "mp_linear_fwd: GELU epilogue needs z");
  MP_CHECK(epilogue != 2 || r, MP_ERR_ARG, "mp_linear_fwd: residual epilogue needs r");
  GemmF32Args g = {};
  g.A = x; g.lda = K; g.B = W; g.ldb = K; g.C = y; g.ldc = N; g.M = M; g.N = N; g.K = K; g.bias = b; g.Z = z; g.R = r;
  return gemm_f32(0, 0, epilogue == 0 ? EPI_BIAS : (epilogue == 1 ? EPI_BIAS_GELU : EPI_BIAS_RESID), g, (hipStream_t)stream);
}
int64_t mp_linear_bwd_slab_floats(int N, int K) { return wgrad_f32_slab_floats(0, N, K) + (int64_t)N * K + N; }
int mp_linear_bwd(const float* dy, const float* x, const float* W, float* dx, float* dW, float* db, int M, int N, int K,
                  float* slab, int64_t slab_floats, void* stream) {
  MP_CHECK(dy && x && W && dW && slab, MP_ERR_ARG, "mp_linear_bwd: null pointer");
  if (dx) {
    GemmF32Args g = {};
    g.A = dy; g.lda = N; g.B = W; g.ldb = K; g.C = dx; g.ldc = K; g.M = M; g.N = K; g.K = N;
    int rc = gemm_f32(0, 1, EPI_BIAS, g, (hipStream_t)stream);
    if (rc) return rc;
  }
  return wgrad_f32(dy, N, x, K, M, N, K, dW, db, slab, slab_floats, (hipStream_t)stream);
}

int mp_linear_fwd_bf16(const void* x, const void* W, const float* b, void* y, void* z, const float* r, int M, int N, int K,
                       int epilogue, void* stream) {
  MP_CHECK(x && W && y && epilogue >= 0 && epilogue <= 2, MP_ERR_ARG, "mp_linear_fwd_bf16: bad argument");
  MP_CHECK((epilogue != 1 || z) && (epilogue != 2 || r), MP_ERR_ARG, "mp_linear_fwd_bf16: epilogue operand missing");
  GemmB16Args g = {};
  g.A = x; g.lda = K; g.B = W; g.ldb = K; g.C = y; g.ldc = N; g.M = M; g.N = N; g.K = K; g.bias = b; g.Z = z; g.R = r;
  const int epi = epilogue == 0 ? EPI_BIAS : (epilogue == 1 ? EPI_BIAS_GELU : EPI_BIAS_RESID);
  return gemm_bf16(g, 0, 0, 0, epilogue == 2, epi, (hipStream_t)stream);
}
int mp_linear_bwd_bf16(const void* dy, int dy_f32, const void* x, const void* W, void* dx, int dx_f32, float* dW, float* db,
                       int M, int N, int K, float* slab, int64_t slab_floats, void* stream) {
  MP_CHECK(dy && x && W && dW && slab, MP_ERR_ARG, "mp_linear_bwd_bf16: null pointer");
  if (dx) {
    GemmB16Args g = {};
    g.A = dy; g.lda = N; g.B = W; g.ldb = K; g.C = dx; g.ldc = K; g.M = M; g.N = K; g.K = N;
    int rc = gemm_bf16(g, dy_f32, 0, 1, dx_f32, EPI_BIAS, (hipStream_t)stream);
    if (rc) return rc;
  }
  return wgrad_bf16(dy, dy_f32, N, (const bf16*)x, K, M, N, K, dW, db, slab, slab_floats, (hipStream_t)stream);
}

int mp_attention_fwd(const float* qkv, float* out, float* lse, int temporal, int B, int T, int J, int C, int H, void* stream) {
  return attention_fwd("mp_attention_fwd", ATTN_F32, qkv, out, lse, temporal, B, T, J, C, H, 0.f, stream);
}
int mp_attention_bwd(const float* qkv, const float* out, const float* d_out, const float* lse, float* delta, float* d_qkv,
                     int temporal, int B, int T, int J, int C, int H, void* stream) {
  return attention_bwd("mp_attention_bwd", ATTN_F32, qkv, out, d_out, lse, delta, d_qkv, temporal, B, T, J, C, H, 0, 0.f, nullptr, stream);
}

int mp_attention_fwd_bf16(const void* qkv, void* out, float* lse, int temporal, int B, int T, int J, int C, int H, void* stream) {
  return attention_fwd("mp_attention_fwd_bf16", ATTN_BF16, qkv, out, lse, temporal, B, T, J, C, H, 0.f, stream);
}
int mp_attention_bwd_bf16(const void* qkv, const void* out, const void* d_out, const float* lse, float* delta, void* d_qkv,
                          int temporal, int B, int T, int J, int C, int H, void* stream) {
  return attention_bwd("mp_attention_bwd_bf16", ATTN_BF16, qkv, out, d_out, lse, delta, d_qkv, temporal, B, T, J, C, H, 0, 0.f, nullptr, stream);
}

/* split precision ("bf16x3"): planar hi/lo bf16 operands, three matrix-core products per k-tile */
int mp_split_bf16(const float* src, void* hi, void* lo, int64_t n, void* stream) {
  MP_CHECK(src && hi && lo && n > 0, MP_ERR_ARG, "mp_split_bf16: bad argument");
  return split_planes(src, (bf16*)hi, (bf16*)lo, (long)n, (hipStream_t)stream);
}
int mp_linear_fwd_bf16x3(const void* x_hi, const void* x_lo, const void* W_hi, const void* W_lo, const float* b, void* y, void* y_lo,
                         void* z, const float* r, int M, int N, int K, int epilogue, void* stream) {
  MP_CHECK(x_hi && x_lo && W_hi && W_lo && y && epilogue >= 0 && epilogue <= 2, MP_ERR_ARG, "mp_linear_fwd_bf16x3: bad argument");
  MP_CHECK((epilogue == 2 || y_lo) && (epilogue != 1 || z) && (epilogue != 2 || r), MP_ERR_ARG, "mp_linear_fwd_bf16x3: epilogue operand missing");
  GemmB16Args g = {};
  g.A = x_hi; g.A_lo = x_lo; g.lda = K; g.B = W_hi; g.B_lo = W_lo; g.ldb = K; g.C = y; g.C_lo = y_lo; g.ldc = N; g.M = M; g.N = N; g.K = K;
  g.bias = b; g.Z = z; g.R = r;
  const int epi = epilogue == 0 ? EPI_BIAS : (epilogue == 1 ? EPI_BIAS_GELU : EPI_BIAS_RESID);
  return gemm_bf16x3(g, epilogue == 2, epi, (hipStream_t)stream);
}
int mp_linear_fwd_bf16x3_lnres(const void* x_hi, const void* x_lo, const void* W_hi, const void* W_lo, const float* b, float* y,
                               const float* r_in, const float* rstats, const float* rgamma, const float* rbeta, const float* mask, int mask_mode,
                               int T, int J, int M, int N, int K, void* stream) {
  MP_CHECK(x_hi && x_lo && W_hi && W_lo && y && r_in && rstats && rgamma && rbeta, MP_ERR_ARG, "mp_linear_fwd_bf16x3_lnres: null argument");
  MP_CHECK(mask == nullptr || ((mask_mode == 1 || mask_mode == 2) && T > 0 && J > 0 && M % (T * J) == 0), MP_ERR_ARG,
           "mp_linear_fwd_bf16x3_lnres: a DropPath mask needs mask_mode 1 or 2 and M a multiple of T*J");
  MP_CHECK(y != r_in, MP_ERR_ARG, "mp_linear_fwd_bf16x3_lnres: y and r_in may not alias");
  GemmB16Args g = {};
  g.A = x_hi; g.A_lo = x_lo; g.lda = K; g.B = W_hi; g.B_lo = W_lo; g.ldb = K; g.C = y; g.ldc = N; g.M = M; g.N = N; g.K = K;
  g.bias = b; g.R = r_in; g.rstats = rstats; g.rgamma = rgamma; g.rbeta = rbeta;
  g.mask = mask; g.mask_mode = mask ? mask_mode : 0; g.T = T; g.J = J;
  return gemm_bf16x3(g, 1, EPI_BIAS_RESID, (hipStream_t)stream);
}
int mp_split_f16f8(const float* src, void* hi16, void* corr8, int64_t n, int weight, void* stream) {
  MP_CHECK(src && hi16 && corr8 && n > 0 && n % 64 == 0, MP_ERR_ARG, "mp_split_f16f8: bad argument (n must be a multiple of 64)");
  return cast_to_f16f8(src, hi16, corr8, (long)n, weight, (hipStream_t)stream);
}
int mp_linear_fwd_f16f8(const void* x16, const void* x8, const void* W16, const void* W8, const float* b, float* y, int M, int N, int K,
                        void* stream) {
  MP_CHECK(x16 && x8 && W16 && W8 && y, MP_ERR_ARG, "mp_linear_fwd_f16f8: null argument");
  GemmB16Args g = {};
  g.A = x16; g.A_lo = x8; g.lda = K; g.B = W16; g.B_lo = W8; g.ldb = K; g.C = y; g.ldc = N; g.M = M; g.N = N; g.K = K; g.bias = b;
  return gemm_f16f8(g, 1, EPI_BIAS, (hipStream_t)stream);
}
int mp_attention_fwd_bf16x3(const void* qkv_hi, const void* qkv_lo, void* out_hi, void* out_lo, float* lse, float* scratch, int temporal,
                            int B, int T, int J, int C, int H, void* stream) {
  return attention_fwd_x3("mp_attention_fwd_bf16x3", "null pointer", qkv_hi, qkv_lo, out_hi, out_lo, lse, scratch, temporal, B, T, J, C, H, 0, 0.f, stream);
}

/* unit-test entry points of the f16f8 forms the engine launches (include/manipose_hip.h): each fills the argument block engine.hip fills
 * and calls the same dispatcher */
int mp_linear_fwd_f16f8_ex(const void* x16, const void* x8, const void* W16, const void* W8, const float* b, void* y, void* y_lo, void* z,
                           const float* r_in, const float* rstats, const float* rgamma, const float* rbeta, const float* mask, int mask_mode,
                           float rscale, int T, int J, int M, int N, int K, int epilogue, int out_form, void* stream) {
  MP_CHECK(x16 && x8 && W16 && W8 && y, MP_ERR_ARG, "mp_linear_fwd_f16f8_ex: null argument");
  MP_CHECK(epilogue >= 0 && epilogue <= 2 && out_form >= 0 && out_form <= 2, MP_ERR_ARG, "mp_linear_fwd_f16f8_ex: epilogue %d, out_form %d", epilogue,
           out_form);
  MP_CHECK(mask == nullptr || ((mask_mode == 1 || mask_mode == 2) && T > 0 && J > 0 && M % (T * J) == 0), MP_ERR_ARG,
           "mp_linear_fwd_f16f8_ex: a DropPath mask needs mask_mode 1 or 2 and M a multiple of T*J");
  MP_CHECK(epilogue != 2 || (r_in && y != r_in), MP_ERR_ARG, "mp_linear_fwd_f16f8_ex: the residual epilogue needs r_in, not aliased with y");
  GemmB16Args g = {};
  g.A = x16; g.A_lo = x8; g.lda = K; g.B = W16; g.B_lo = W8; g.ldb = K; g.C = y; g.C_lo = y_lo; g.ldc = N; g.M = M; g.N = N; g.K = K; g.bias = b;
  g.Z = z; g.R = r_in; g.rstats = rstats; g.rgamma = rgamma; g.rbeta = rbeta; g.mask = mask; g.mask_mode = mask ? mask_mode : 0; g.T = T; g.J = J;
  g.rscale = rscale; g.out_f16f8 = out_form == 2 ? 1 : 0;
  const int epi = epilogue == 0 ? EPI_BIAS : (epilogue == 1 ? EPI_BIAS_GELU : EPI_BIAS_RESID);
  return gemm_f16f8(g, out_form == 0 ? 1 : 0, epi, (hipStream_t)stream);
}
int mp_layernorm_fwd_ex(const float* x, int M, int C, const float* g1, const float* b1, float eps1, const float* pos, int T, int J, float* x1,
                        float* stats1, const float* g2, const float* b2, float eps2, void* y2, void* y2_lo, void* y2_b16, float* stats2, int out_mode,
                        void* stream) {
  MP_CHECK(x && M > 0 && out_mode >= 0 && out_mode <= 3, MP_ERR_ARG, "mp_layernorm_fwd_ex: bad argument");
  MP_CHECK(!g1 || (b1 && stats1 && (!pos || (T > 0 && J > 0))), MP_ERR_ARG, "mp_layernorm_fwd_ex: stage 1 needs b1, stats1 (and T, J with pos)");
  MP_CHECK(!g2 || (b2 && y2 && stats2), MP_ERR_ARG, "mp_layernorm_fwd_ex: stage 2 needs b2, y2 and stats2");
  MP_CHECK(!y2_b16 || out_mode == 3, MP_ERR_ARG, "mp_layernorm_fwd_ex: the bf16 copy belongs to out mode 3");
  LnFwdArgs a = {};
  a.x = x; a.M = M; a.C = C;
  a.g1 = g1; a.b1 = b1; a.eps1 = eps1; a.pos = pos; a.T = T; a.J = J; a.x1 = x1; a.stats1 = stats1;
  a.g2 = g2; a.b2 = b2; a.eps2 = eps2; a.y2 = y2; a.y2_lo = y2_lo; a.y2_b16 = y2_b16; a.stats2 = stats2;
  return ln_fwd(a, out_mode, (hipStream_t)stream);
}
int mp_attention_fwd_bf16x3_ex(const void* qkv_hi, const void* qkv_lo, void* out_hi, void* out_lo, float* lse, float* scratch, int temporal,
                               int B, int T, int J, int C, int H, int out_form, void* stream) {
  return attention_fwd_x3("mp_attention_fwd_bf16x3_ex", "bad argument", qkv_hi, qkv_lo, out_hi, out_lo, lse, scratch, temporal, B, T, J, C, H, out_form, 0.f,
                          stream);
}
int mp_attention_bwd_bf16_ex(const void* qkv, const void* out, const void* d_out, const float* lse, float* delta, void* d_qkv, int temporal, int B,
                             int T, int J, int C, int H, int out_f16, void* stream) {
  return attention_bwd("mp_attention_bwd_bf16_ex", ATTN_BF16, qkv, out, d_out, lse, delta, d_qkv, temporal, B, T, J, C, H, out_f16, 0.f, nullptr, stream);
}
/* the attention forms only the engine reaches: a softmax scale of its own and the scaled-fp16 gradient stores of the MFMA backward kernels */
int mp_attention_fwd_bf16_scale_ex(const void* qkv, void* out, float* lse, int temporal, int B, int T, int J, int C, int H, float qk_scale,
                                   void* stream) {
  return attention_fwd("mp_attention_fwd_bf16_scale_ex", ATTN_BF16, qkv, out, lse, temporal, B, T, J, C, H, qk_scale, stream);
}
int mp_attention_bwd_bf16_scale_ex(const void* qkv, const void* out, const void* d_out, const float* lse, float* delta, void* d_qkv, int temporal,
                                   int B, int T, int J, int C, int H, int out_f16, float qk_scale, const float* grad_scale, void* stream) {
  return attention_bwd("mp_attention_bwd_bf16_scale_ex", ATTN_BF16, qkv, out, d_out, lse, delta, d_qkv, temporal, B, T, J, C, H, out_f16, qk_scale, grad_scale,
                       stream);
}
int mp_attention_fwd_bf16x3_scale_ex(const void* qkv_hi, const void* qkv_lo, void* out_hi, void* out_lo, float* lse, float* scratch, int temporal,
                                     int B, int T, int J, int C, int H, int out_form, float qk_scale, void* stream) {
  return attention_fwd_x3("mp_attention_fwd_bf16x3_scale_ex", "bad argument", qkv_hi, qkv_lo, out_hi, out_lo, lse, scratch, temporal, B, T, J, C, H, out_form,
                          qk_scale, stream);
}
int mp_linear_bwd_f16(const void* dy, const void* x, const void* W, void* dx, const void* z, const float* gout, uint32_t* gsat, float* dW, float* db,
                      int M, int N, int K, int f16, int x_f16, const float* oscale, float* slab, int64_t slab_floats, void* stream) {
  MP_CHECK(dy && (dx || dW), MP_ERR_ARG, "mp_linear_bwd_f16: nothing to compute");
  MP_CHECK(!f16 || !x_f16, MP_ERR_ARG, "mp_linear_bwd_f16: f16 and x_f16 are exclusive");
  if (dx) {
    MP_CHECK(W, MP_ERR_ARG, "mp_linear_bwd_f16: dgrad without W");
    GemmB16Args g = {};
    g.A = dy; g.lda = N; g.B = W; g.ldb = K; g.C = dx; g.ldc = K; g.M = M; g.N = K; g.K = N; g.Z = const_cast<void*>(z);
    g.f16 = f16; g.gout = gout; g.gsat = gout != nullptr ? gsat : nullptr;
    int rc = gemm_bf16(g, 0, 0, 1, 0, z ? EPI_DGELU : EPI_BIAS, (hipStream_t)stream);
    if (rc) return rc;
  }
  if (dW) {
    MP_CHECK(x && slab && (!f16 || oscale), MP_ERR_ARG, "mp_linear_bwd_f16: weight gradient without x / slab (or oscale with f16)");
    return wgrad_bf16(dy, 0, N, (const bf16*)x, K, M, N, K, dW, db, slab, (long)slab_floats, (hipStream_t)stream, f16, oscale, x_f16);
  }
  return MP_OK;
}

/* unit-test entry points of the LayerNorm backward forms the engine launches (include/manipose_hip.h): the same dispatchers with every argument
 * engine.hip fills.  gsc is the engine's 8-float gradient-scale block (grad_scale): dy_scaled passes gsc + 1 (1 / S) as dy_scale, copy_f16 passes
 * gsc (S, counters in gsc[4..5]) as b16_gs.  A non-null param_stream runs the parameter-gradient reduction there, behind an event this file owns
 * (the engine's ev_heads). */
static int ln_bwd_common(const char* who, const float* mask, int mask_mode, int M, int T, int J, void* dx_b16, const float* gsc, int dy_scaled,
                         int copy_f16, hipEvent_t* ev, void* param_stream) {
  MP_CHECK(mask == nullptr || mask_mode == 1 || mask_mode == 2, MP_ERR_ARG, "%s: a DropPath mask needs mask_mode 1 or 2 (got %d)", who, mask_mode);
  MP_CHECK(mask == nullptr || (T > 0 && J > 0 && M % (T * J) == 0), MP_ERR_ARG, "%s: a DropPath mask needs M=%d a multiple of T*J (T=%d, J=%d)", who, M,
           T, J);
  MP_CHECK(!copy_f16 || dx_b16, MP_ERR_ARG, "%s: copy_f16 without dx_b16", who);
  MP_CHECK((!dy_scaled && !copy_f16) || gsc, MP_ERR_ARG, "%s: dy_scaled / copy_f16 need the gsc block", who);
  *ev = nullptr;
  if (param_stream != nullptr) {
    static hipEvent_t own = nullptr;
    if (own == nullptr && hipEventCreateWithFlags(&own, hipEventDisableTiming) != hipSuccess) {
      own = nullptr;
      MP_CHECK(false, MP_ERR_HIP, "%s: could not create the parameter-stream event", who);
    }
    *ev = own;
  }
  return MP_OK;
}
int mp_layernorm_bwd_ex(const void* dy, int dy_bf16, const float* x, const float* stats, const float* gamma, const float* dskip, float rs, float* dx,
                        void* dx_b16, const float* mask, int mask_mode, int T, int J, float* gsc, int dy_scaled, int copy_f16, float* dgamma,
                        float* dbeta, int M, int C, float* scratch, int64_t scratch_floats, void* param_stream, void* stream) {
  MP_CHECK(dy && x && stats && gamma && dx && dgamma && dbeta && scratch && M > 0, MP_ERR_ARG, "mp_layernorm_bwd_ex: null pointer");
  MP_CHECK(C > 0 && C % 4 == 0 && C <= 1024, MP_ERR_ARG, "mp_layernorm_bwd_ex: C=%d unsupported", C);
  MP_CHECK(scratch_floats >= 1024L * 2 * C, MP_ERR_ARG, "mp_layernorm_bwd_ex: scratch needs 1024 * 2 * C floats");
  hipEvent_t ev = nullptr;
  if (int rc = ln_bwd_common("mp_layernorm_bwd_ex", mask, mask_mode, M, T, J, dx_b16, gsc, dy_scaled, copy_f16, &ev, param_stream)) return rc;
  return ln_bwd(dy, dy_bf16, x, stats, gamma, dskip, dx, dx_b16, mask, mask ? mask_mode : 0, T, J, dgamma, dbeta, M, C, scratch, (long)scratch_floats,
                (hipStream_t)stream, (hipStream_t)param_stream, ev, rs, dy_scaled ? gsc + 1 : nullptr, copy_f16 ? gsc : nullptr);
}
int mp_layernorm_bwd2_ex(const void* dy1, int dy_bf16, const float* stats1, const float* gamma1, const float* dskip, float rs, const float* x0,
                         const float* stats0, const float* gamma0, const float* beta0, float* dx, void* dx_b16, const float* mask, int mask_mode, int T,
                         int J, float* gsc, int dy_scaled, int copy_f16, float* dgamma1, float* dbeta1, float* dgamma0, float* dbeta0, int M, int C,
                         float* scratch, int64_t scratch_floats, void* param_stream, void* stream) {
  MP_CHECK(dy1 && stats1 && gamma1 && x0 && stats0 && gamma0 && dx && dgamma1 && dbeta1 && dgamma0 && dbeta0 && scratch && M > 0, MP_ERR_ARG,
           "mp_layernorm_bwd2_ex: null pointer");
  MP_CHECK(beta0, MP_ERR_ARG, "mp_layernorm_bwd2_ex: x1 is recomputed from x0, beta0 is required");
  MP_CHECK(dskip, MP_ERR_ARG, "mp_layernorm_bwd2_ex: the fused form always adds the skip gradient (dskip is required)");
  MP_CHECK(C > 0 && C % 4 == 0 && C <= 512, MP_ERR_ARG, "mp_layernorm_bwd2_ex: C=%d unsupported", C);
  MP_CHECK(scratch_floats >= 1024L * 4 * C, MP_ERR_ARG, "mp_layernorm_bwd2_ex: scratch needs 1024 * 4 * C floats");
  hipEvent_t ev = nullptr;
  if (int rc = ln_bwd_common("mp_layernorm_bwd2_ex", mask, mask_mode, M, T, J, dx_b16, gsc, dy_scaled, copy_f16, &ev, param_stream)) return rc;
  return ln_bwd2(dy1, dy_bf16, nullptr, stats1, gamma1, dskip, x0, stats0, gamma0, beta0, dx, dx_b16, mask, mask ? mask_mode : 0, T, J, dgamma1, dbeta1,
                 dgamma0, dbeta0, M, C, scratch, (long)scratch_floats, (hipStream_t)stream, (hipStream_t)param_stream, ev, rs,
                 dy_scaled ? gsc + 1 : nullptr, copy_f16 ? gsc : nullptr);
}
int mp_scale_rows_ex(const float* g, const float* mask, int mask_mode, void* out, int out_bf16, int M, int C, int T, int J, void* stream) {
  MP_CHECK(g && mask && out && M > 0, MP_ERR_ARG, "mp_scale_rows_ex: null pointer");
  MP_CHECK(C > 0 && C % 4 == 0, MP_ERR_ARG, "mp_scale_rows_ex: C=%d unsupported", C);
  MP_CHECK(mask_mode == 1 || mask_mode == 2, MP_ERR_ARG, "mp_scale_rows_ex: mask_mode %d (1 or 2)", mask_mode);
  MP_CHECK(T > 0 && J > 0 && M % (T * J) == 0, MP_ERR_ARG, "mp_scale_rows_ex: M=%d is not a multiple of T*J (T=%d, J=%d)", M, T, J);
  return scale_rows(g, mask, mask_mode, out, out_bf16, M, C, T, J, (hipStream_t)stream);
}

/* unit-test entry points of the kernels at the two ends of the network (include/manipose_hip.h): the launchers' unstated limits are checked
 * here, everything else is the engine's call */
int mp_embed_fwd_ex(const float* x, const float* W, const float* b, const float* spos, float* out, int M, int C, int J, void* stream) {
  MP_CHECK(x && W && b && spos && out, MP_ERR_ARG, "mp_embed_fwd_ex: null pointer");
  MP_CHECK(M > 0 && J > 0 && C > 0 && C % 4 == 0, MP_ERR_ARG, "mp_embed_fwd_ex: M=%d C=%d J=%d unsupported (positive, C %% 4 == 0)", M, C, J);
  return embed_fwd(x, W, b, spos, out, M, C, J, (hipStream_t)stream);
}
int64_t mp_embed_bwd_scratch_floats(int C, int J) { return (C > 0 && J > 0) ? (int64_t)embed_bwd_scratch_floats(C, J) : 0; }
/* M % J != 0: the launcher takes the channel-per-thread kernel (also for J == 17) and sums the M / J whole frames only */
int mp_embed_bwd_ex(const float* g, const float* x, float* dW, float* db, float* dspos, int M, int C, int J, float* scratch, int64_t scratch_floats,
                    void* stream) {
  MP_CHECK(g && x && dW && db && dspos && scratch, MP_ERR_ARG, "mp_embed_bwd_ex: null pointer");
  MP_CHECK(M > 0 && J > 0 && C > 0 && C % 4 == 0, MP_ERR_ARG, "mp_embed_bwd_ex: M=%d C=%d J=%d unsupported (positive, C %% 4 == 0)", M, C, J);
  MP_CHECK(scratch_floats >= embed_bwd_scratch_floats(C, J), MP_ERR_ARG, "mp_embed_bwd_ex: scratch needs mp_embed_bwd_scratch_floats(C, J) floats");
  return embed_bwd(g, x, dW, db, dspos, M, C, J, scratch, (long)scratch_floats, (hipStream_t)stream);
}
int mp_bones_embed_fwd_ex(const float* x, const float* W, const float* b, const float* spos, float* out, int BT, int IN, int O, void* stream) {
  MP_CHECK(x && W && b && spos && out, MP_ERR_ARG, "mp_bones_embed_fwd_ex: null pointer");
  MP_CHECK(BT > 0 && O > 0 && IN == 34, MP_ERR_ARG, "mp_bones_embed_fwd_ex: BT=%d IN=%d O=%d unsupported (positive, IN == 34)", BT, IN, O);
  return bones_embed_fwd(x, W, b, spos, out, BT, IN, O, (hipStream_t)stream);
}
int mp_bones_embed_bwd_ex(const float* g, const float* x, float* dW, float* db, float* dspos, int BT, int IN, int O, float* scratch,
                          int64_t scratch_floats, void* stream) {
  MP_CHECK(g && x && dW && db && dspos && scratch, MP_ERR_ARG, "mp_bones_embed_bwd_ex: null pointer");
  MP_CHECK(BT > 0 && O > 0 && IN == 34, MP_ERR_ARG, "mp_bones_embed_bwd_ex: BT=%d IN=%d O=%d unsupported (positive, IN == 34)", BT, IN, O);
  MP_CHECK(scratch_floats >= (int64_t)((BT < 32 ? BT : 32) + 1) * O * 35, MP_ERR_ARG, "mp_bones_embed_bwd_ex: scratch needs (min(32, BT) + 1) * O * 35 floats");
  return bones_embed_bwd(g, x, dW, db, dspos, BT, IN, O, scratch, (long)scratch_floats, (hipStream_t)stream);
}
int mp_tpos_grad_ex(const float* g, float* dtpos, int B, int T, int J, int C, void* stream) {
  MP_CHECK(g && dtpos, MP_ERR_ARG, "mp_tpos_grad_ex: null pointer");
  MP_CHECK(B > 0 && T > 0 && J > 0 && C > 0, MP_ERR_ARG, "mp_tpos_grad_ex: B=%d T=%d J=%d C=%d must be positive", B, T, J, C);
  return tpos_grad(g, dtpos, B, T, J, C, (hipStream_t)stream);      // refuses C % 4 != 0 and J < 4 itself
}

static int score_dims(const char* who, int K, int O, int B, int T, int J) {
  MP_CHECK(K >= 1 && K <= 8 && J >= 1 && J <= 32, MP_ERR_ARG, "%s: K=%d J=%d unsupported (1 <= K <= 8, 1 <= J <= 32)", who, K, J);
  MP_CHECK(O > 0 && B > 0 && T > 0, MP_ERR_ARG, "%s: O=%d B=%d T=%d must be positive", who, O, B, T);
  return MP_OK;
}
int mp_scores_fwd_ex(const float* headout, const float* w, const float* b, int K, int O, float* scores, int B, int T, int J, void* stream) {
  MP_CHECK(headout && w && b && scores, MP_ERR_ARG, "mp_scores_fwd_ex: null pointer");
  if (int rc = score_dims("mp_scores_fwd_ex", K, O, B, T, J)) return rc;
  ScoreParams p = {};
  for (int k = 0; k < K; ++k) { p.w[k] = w + (long)k * J; p.b[k] = b + k; }
  return scores_fwd(headout, p, K, O, scores, B, T, J, (hipStream_t)stream);
}
int64_t mp_scores_bwd_scratch_floats(int K, int B, int T) { return (K > 0 && B > 0 && T > 0) ? (int64_t)scores_bwd_scratch_floats(K, B, T) : 0; }
int mp_scores_bwd_ex(const float* headout, const float* scores, const float* d_scores, const float* w, const float* b, float* dw, float* db, int K,
                     int O, float* d_headout, int B, int T, int J, float* scratch, int64_t scratch_floats, void* param_stream, void* stream) {
  MP_CHECK(headout && scores && d_scores && w && b && dw && db && d_headout && scratch, MP_ERR_ARG, "mp_scores_bwd_ex: null pointer");
  if (int rc = score_dims("mp_scores_bwd_ex", K, O, B, T, J)) return rc;
  MP_CHECK(scratch_floats >= scores_bwd_scratch_floats(K, B, T), MP_ERR_ARG, "mp_scores_bwd_ex: scratch needs mp_scores_bwd_scratch_floats(K, B, T) floats");
  ScoreParams p = {};
  ScoreGrads gp = {};
  for (int k = 0; k < K; ++k) { p.w[k] = w + (long)k * J; p.b[k] = b + k; gp.w[k] = dw + (long)k * J; gp.b[k] = db + k; }
  hipEvent_t ev = nullptr;
  if (param_stream != nullptr) MP_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
  const int rc = scores_bwd(headout, scores, d_scores, p, gp, K, O, d_headout, B, T, J, scratch, (long)scratch_floats, (hipStream_t)stream,
                            (hipStream_t)param_stream, ev);
  if (ev != nullptr) (void)hipEventDestroy(ev);      // the wait already enqueued on param_stream keeps what it needs
  return rc;
}
int mp_bones_mean_fwd_ex(const float* headout, float* lengths, int B, int T, int S, void* stream) {
  MP_CHECK(headout && lengths, MP_ERR_ARG, "mp_bones_mean_fwd_ex: null pointer");
  MP_CHECK(B > 0 && T > 0 && S >= 1 && S <= 32, MP_ERR_ARG, "mp_bones_mean_fwd_ex: B=%d T=%d S=%d unsupported (positive, S <= 32)", B, T, S);
  return bones_mean_fwd(headout, lengths, B, T, S, (hipStream_t)stream);
}
int mp_bones_mean_bwd_ex(const float* d_len_pose, int KT, float* d_lengths, float* d_headout, int B, int T, int S, void* stream) {
  MP_CHECK(d_len_pose && d_headout, MP_ERR_ARG, "mp_bones_mean_bwd_ex: null pointer");
  MP_CHECK(B > 0 && T > 0 && KT > 0 && S >= 1 && S <= 32, MP_ERR_ARG, "mp_bones_mean_bwd_ex: B=%d T=%d KT=%d S=%d unsupported (positive, S <= 32)", B, T,
           KT, S);
  return bones_mean_bwd(d_len_pose, KT, d_lengths, d_headout, B, T, S, (hipStream_t)stream);
}

static int heads_pick(int impl, int K, int O, int C, const char* who, bool* mfma) {
  MP_CHECK(impl >= 0 && impl <= 2, MP_ERR_ARG, "%s: impl %d", who, impl);
  MP_CHECK(K >= 1 && K <= 8 && O >= 1, MP_ERR_ARG, "%s: K=%d O=%d unsupported", who, K, O);
  *mfma = impl == 2 || (impl == 0 && heads_use_mfma(K, O, C));
  MP_CHECK(!*mfma || heads_mfma_supported(K, O, C), MP_ERR_ARG, "%s: K=%d O=%d C=%d not covered by the matrix-core heads", who, K, O, C);
  return MP_OK;
}
int64_t mp_heads_fold_floats(int C) { return heads_fold_floats(C); }
int64_t mp_heads_bwd_scratch_floats(int K, int O, int C) { return 512L * K * ((long)O * C + O + 2 * C) + 256L * heads_fold_floats(C); }
int mp_heads_fwd(const float* x, const float* gamma, const float* beta, const float* W, const float* b, int K, int O, float* out, float* stats,
                 float* fold, int M, int C, int impl, void* stream) {
  MP_CHECK(x && gamma && beta && W && b && out && stats && fold && M > 0, MP_ERR_ARG, "mp_heads_fwd: bad argument");
  bool mfma = false;
  if (int rc = heads_pick(impl, K, O, C, "mp_heads_fwd", &mfma)) return rc;
  HeadParams p = {};
  for (int k = 0; k < K; ++k) { p.gamma[k] = gamma + (long)k * C; p.beta[k] = beta + (long)k * C; p.W[k] = W + (long)k * O * C; p.b[k] = b + (long)k * O; }
  return mfma ? heads_fwd_mfma(x, p, K, O, out, stats, M, C, fold, (hipStream_t)stream) : heads_fwd(x, p, K, O, out, stats, M, C, (hipStream_t)stream);
}
int mp_heads_bwd(const float* x, const float* stats, const float* fold, const float* out, const float* gamma, const float* beta, const float* W,
                 const float* b, const float* d_out, float* dx, float* dgamma, float* dbeta, float* dW, float* db, int K, int O, int M, int C, int impl,
                 float* scratch, int64_t scratch_floats, void* stream) {
  MP_CHECK(x && stats && fold && out && gamma && beta && W && b && d_out && dx && dgamma && dbeta && dW && db && scratch && M > 0, MP_ERR_ARG,
           "mp_heads_bwd: bad argument");
  bool mfma = false;
  if (int rc = heads_pick(impl, K, O, C, "mp_heads_bwd", &mfma)) return rc;
  HeadParams p = {};
  HeadGrads g = {};
  for (int k = 0; k < K; ++k) {
    p.gamma[k] = gamma + (long)k * C; p.beta[k] = beta + (long)k * C; p.W[k] = W + (long)k * O * C; p.b[k] = b + (long)k * O;
    g.gamma[k] = dgamma + (long)k * C; g.beta[k] = dbeta + (long)k * C; g.W[k] = dW + (long)k * O * C; g.b[k] = db + (long)k * O;
  }
  return mfma ? heads_bwd_mfma(x, stats, fold, out, p, g, K, O, d_out, dx, M, C, scratch, scratch_floats, (hipStream_t)stream, nullptr)
              : heads_bwd(x, stats, p, g, K, O, d_out, dx, M, C, scratch, scratch_floats, (hipStream_t)stream);
}

int mp_gather_windows(const float* poses_2d, const float* poses_3d, const int64_t* seq_offset, int S, const int32_t* win_seq,
                      const int32_t* win_start, const uint8_t* win_flip, const int32_t* mirror, const float* mask2d, const float* noise2d,
                      int B, int T, int J, float* X, float* y, void* stream) {
  static_assert(sizeof(long) == sizeof(int64_t), "LP64");
  return gather_windows(poses_2d, poses_3d, (const long*)seq_offset, S, win_seq, win_start, win_flip, mirror, mask2d, noise2d, B, T, J,
                        X, y, (hipStream_t)stream);
}

int mp_ingest_pose3d(const float* raw, int raw_joints, const int32_t* frames, int64_t N, const int32_t* joint_map, int J,
                     const float* orientation, const float* translation, int root_raw, int root_out, float divisor, float* out,
                     void* stream) {
  return ingest_pose3d(raw, raw_joints, frames, (long)N, joint_map, J, orientation, translation, root_raw, root_out, divisor, out,
                       (hipStream_t)stream);
}

int mp_ingest_pose2d(const float* raw, int raw_joints, int raw_channels, const int32_t* frames, int64_t N, const int32_t* joint_map,
                     int J, float res_w, float res_h, float* out, void* stream) {
  return ingest_pose2d(raw, raw_joints, raw_channels, frames, (long)N, joint_map, J, res_w, res_h, out, (hipStream_t)stream);
}

int mp_procrustes_errors(const float* pred, const float* gt, const uint8_t* mask, int64_t N, int J, float pred_scale, float gt_scale,
                         float pck_threshold, float auc_max, int auc_steps, float* out, float* scratch, int64_t scratch_floats, void* stream) {
  return procrustes_errors(pred, gt, mask, (long)N, J, pred_scale, gt_scale, pck_threshold, auc_max, auc_steps, 1, out, scratch,
                           (long)scratch_floats, (hipStream_t)stream);
}

int mp_pose_metrics_row_floats(void) { return pose_metrics_row_floats(); }
int mp_bone_length_table(const float* pred, const int64_t* pred_strides, const float* gt, const int64_t* gt_strides, int B, int L, int signed_diff,
                         float* out, void* stream) {
  MP_CHECK(pred && pred_strides && gt && gt_strides && out, MP_ERR_ARG, "mp_bone_length_table: null pointer");
  long ps[4], gs[4];
  for (int i = 0; i < 4; ++i) { ps[i] = (long)pred_strides[i]; gs[i] = (long)gt_strides[i]; }
  return bone_length_table(pred, ps, gt, gs, B, L, signed_diff, out, (hipStream_t)stream);
}
int mp_pose_metrics(const float* pred, const int64_t* pred_strides, const float* gt, const int64_t* gt_strides, const uint8_t* mask, int B,
                    int L, int J, float pred_scale, float gt_scale, float pck_threshold, float auc_max, int auc_steps, int scale_align,
                    float* out, float* len0, float* scratch, int64_t scratch_floats, void* stream) {
  MP_CHECK(pred && pred_strides && out && len0 && scratch, MP_ERR_ARG, "mp_pose_metrics: null pointer");
  long ps[4], gs[4] = {0, 0, 0, 0};
  for (int i = 0; i < 4; ++i) { ps[i] = (long)pred_strides[i]; if (gt_strides) gs[i] = (long)gt_strides[i]; }
  return pose_metrics(pred, ps, gt, gt_strides ? gs : nullptr, mask, B, L, J, pred_scale, gt_scale, pck_threshold, auc_max, auc_steps,
                      scale_align, out, len0, scratch, (long)scratch_floats, (hipStream_t)stream);
}

int64_t mp_bone_extremes_scratch_floats(int64_t frames) { return (int64_t)bone_extremes_scratch_floats((long)frames); }
int mp_bone_extremes(const float* pred, const int64_t* pred_strides, const float* gt, const int64_t* gt_strides, int B, int L, int J,
                     float pred_scale, float gt_scale, int chain, const float* prev_len, int64_t frame_base, float* min_len, float* max_len,
                     float* max_delta, int64_t* max_delta_idx, float* coord_sums, float* last_len, float* scratch, int64_t scratch_floats,
                     void* stream) {
  MP_CHECK(pred && pred_strides, MP_ERR_ARG, "mp_bone_extremes: null pointer");
  long ps[4], gs[4] = {0, 0, 0, 0};
  for (int i = 0; i < 4; ++i) { ps[i] = (long)pred_strides[i]; if (gt_strides) gs[i] = (long)gt_strides[i]; }
  return bone_extremes(pred, ps, gt, gt_strides ? gs : nullptr, B, L, J, pred_scale, gt_scale, chain, prev_len, (long)frame_base, min_len,
                       max_len, max_delta, reinterpret_cast<long*>(max_delta_idx), coord_sums, last_len, scratch, (long)scratch_floats,
                       (hipStream_t)stream);
}

int64_t mp_hypothesis_stats_scratch_floats(int64_t frames) { return (int64_t)hypothesis_stats_scratch_floats((long)frames); }
int mp_hypothesis_stats_row_floats(void) { return hypothesis_stats_row_floats(); }
int mp_hypothesis_stats_row_counts(void) { return hypothesis_stats_row_counts(); }
int mp_hypothesis_stats(const float* poses, const float* scores, const float* target, int B, int K, int T, float pose_scale, float target_scale,
                        float* sums, int64_t* counts, float* jbest_pose, uint8_t* jbest_idx, float* scratch, int64_t scratch_floats,
                        void* stream) {
  return hypothesis_stats(poses, scores, target, B, K, T, pose_scale, target_scale, sums, reinterpret_cast<long*>(counts), jbest_pose, jbest_idx,
                          scratch, (long)scratch_floats, (hipStream_t)stream);
}

/* test / tuning hooks (include/manipose_hip.h): process-wide selectors between kernels that are tested to agree; everything that changes a
 * model's arithmetic or its stream use is a field of mp_model_config */
int mp_gemm_plan(int M, int N, int K, int form, int epilogue, int cus, int out[4]) {
  MP_CHECK(out, MP_ERR_ARG, "mp_gemm_plan: null out");
  MP_CHECK(M > 0 && N > 0 && K > 0 && cus >= 0, MP_ERR_ARG, "mp_gemm_plan: bad shape M=%d N=%d K=%d cus=%d", M, N, K, cus);
  MP_CHECK(form == GEMM_FORM_BF16 || form == GEMM_FORM_BF16X3 || form == GEMM_FORM_F16F8 || form == GEMM_FORM_F16, MP_ERR_ARG,
           "mp_gemm_plan: form %d (0 bf16, 1 bf16x3, 8 f16f8, 16 fp16)", form);
  MP_CHECK(epilogue >= EPI_BIAS && epilogue <= EPI_SLAB, MP_ERR_ARG, "mp_gemm_plan: epilogue %d", epilogue);
  if (cus == 0) cus = gemm_device_cus();
  MP_CHECK(cus > 0, MP_ERR_HIP, "mp_gemm_plan: no device to ask for its CU count");
  // the layouts the engine uses for that epilogue: forward "N","N" (lda = ldb = K); gelu'-multiplying dgrad "N","T" (ldb = N); weight
  // gradient "T","T" (one split)
  const bool wgrad = epilogue == EPI_SLAB, dgrad = epilogue == EPI_DGELU;
  const GemmPlanIn in = {M, N, K, form, epilogue, wgrad ? 1 : 0, (wgrad || dgrad) ? 1 : 0, 1, wgrad ? (long)M : (long)K, (wgrad || dgrad) ? (long)N : (long)K, 1.0f, cus};
  const GemmPlan pl = gemm_plan(in);
  MP_CHECK(pl.tile != 0, MP_ERR_ARG, "mp_gemm_plan: no kernel of form %d serves M=%d N=%d K=%d with epilogue %d", form, M, N, K, epilogue);
  out[0] = pl.tile; out[1] = pl.persistent; out[2] = pl.workgroups; out[3] = pl.tiles;
  return MP_OK;
}
int mp_gemm_launch_counts(int64_t out[3], int reset) {
  MP_CHECK(out, MP_ERR_ARG, "mp_gemm_launch_counts: null out");
  long long c[3];
  gemm_launch_counts(c, reset);
  for (int i = 0; i < 3; ++i) out[i] = (int64_t)c[i];
  return MP_OK;
}
int mp_set_option(const char* name, int value) {
  MP_CHECK(name, MP_ERR_ARG, "mp_set_option: null name");
  if (!strcmp(name, "gemm_small_tile")) { gemm_bf16_force_small_tile(value != 0); return MP_OK; }
  if (!strcmp(name, "gemm_persist_min_tiles")) { gemm_bf16_persist_min_tiles(value); return MP_OK; }
  if (!strcmp(name, "gemm_persist_mode")) { gemm_bf16_persist_mode(value); return MP_OK; }
  if (!strcmp(name, "gemm_persist_wgs")) { gemm_bf16_persist_wgs(value); return MP_OK; }
  if (!strcmp(name, "gemm_tile")) {
    MP_CHECK(gemm_bf16_tile(value) == MP_OK, MP_ERR_ARG, "mp_set_option: gemm_tile is 0 (planner), 128 or 256, not %d", value);
    return MP_OK;
  }
  if (!strcmp(name, "attn_two_phase")) { attn_two_phase(value); return MP_OK; }
  if (!strcmp(name, "heads_mfma")) { heads_mfma_mode(value); return MP_OK; }
  MP_CHECK(false, MP_ERR_ARG, "mp_set_option: unknown option '%s' (side_streams / f16f8_inputs became mp_model_config::streams / f16f8 in ABI v7)", name);
}

}  // extern "C"

// The multi-hypothesis study of the reference's follow-up scripts, in one pass over K hypotheses, their scores and the target:
//   calc_jbest_mpjpe / calc_jbest_pose      hpe/useful_aux_scripts/eval_baselines.py:451-481   (per joint the hypothesis closest to the target)
//   oracle / best_score / weighted_ave      architectures/rmcl_manifold_mix_ste.py:141-185 + mpjpe_error, without test-time augmentation
//   error against the number of hypotheses  plot_nhyps_lineplot.py   (best of the m best-scored hypotheses, m = 1..K)
//   per-joint spread of the hypotheses      inspect_multimodality.py
// plus what a user needs to judge the scoring head: the score of the oracle hypothesis, its place in the score order, how often every head
// wins by error, by score and per joint, and every head's score mass (include/manipose_hip.h, mp_hypothesis_stats, has the row layouts).
// Wave mapping as wta_loss.hip: a LANE PER JOINT, three consecutive frames per wave (51 of 64 lanes), so that a wave's loads are the whole
// 204-byte rows of its frames.  K is a template parameter: the K distances, pose errors, scores and ranks of a lane stay in registers (a
// private array indexed by a runtime k would live in scratch memory).  What belongs to a frame and not to a joint is kept by the lane whose
// joint number equals the slot's index (head k, rank r and top-(m = k + 1) on lane k of the frame's group): a compare, never a dynamic index.
// A workgroup owns HS_FPB consecutive frames and writes ONE record; a second kernel adds the records in block order (floats in double, counts
// in int64).  No atomics, and every sum has a fixed order (lane, group, wave, block): two runs give the same bits.  Counts are integers from the lane up.
#include "common.h"
#include "kernels.h"

namespace mp {

constexpr int HS_J = 17, HS_KMAX = 8;
constexpr int HS_FPB = 48;                     // frames per workgroup: four waves x 12 frames, three at a time
constexpr int HS_NWV = 4;
// float row (and the float part of a record; word 0, the frame count, is filled in by the finalize kernel)
constexpr int HS_BEST = 1, HS_ORACLE = 2, HS_JBEST = 3, HS_WAVE = 4, HS_S_ORACLE = 5, HS_S_MAX = 6, HS_PAIR = 7, HS_TOPM = 8, HS_JB_JOINT = 16,
              HS_SPREAD = 33, HS_MASS = 50, HS_NF = 58;
// count row (int32 words HS_NF.. of a record, int64 in the result)
constexpr int HS_AGREE = 0, HS_ORANK = 1, HS_PBEST = 9, HS_SHEAD = 17, HS_JHEAD = 25, HS_NI = 33;
constexpr int HS_REC = HS_NF + HS_NI + 1;      // 92 words

struct HsArgs {
  const float* poses; const float* scores; const float* target;
  long N;                                      // B * T frames
  int T;
  float pose_scale, target_scale;
  float* jbest_pose; unsigned char* jbest_idx;
};

__device__ __forceinline__ int wave_sum_i(int v) {
  v += __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xf, 0xf, false);
  v += __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xf, 0xf, false);
  v += __builtin_amdgcn_update_dpp(0, v, 0x141, 0xf, 0xf, false);
  v += __builtin_amdgcn_update_dpp(0, v, 0x140, 0xf, 0xf, false);
  v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xa, 0xf, false);
  v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xc, 0xf, false);
  return __builtin_amdgcn_readlane(v, 63);
}

// sum over the 17 lanes of a frame's group, valid in the group's first lane (wta_loss.hip, group17_sum)
__device__ __forceinline__ float hs_group_sum(float v, int j) {
#pragma unroll
  for (int d = 16; d >= 1; d >>= 1) {
    const float o = __shfl_down(v, d, 64);
    if (j < d && j + d < HS_J) v += o;
  }
  return v;
}
// the three groups of a wave folded onto lanes 0..16, in group order
__device__ __forceinline__ float hs_fold(float v) { return (v + __shfl_down(v, HS_J, 64)) + __shfl_down(v, 2 * HS_J, 64); }
__device__ __forceinline__ int hs_fold(int v) { return (v + __shfl_down(v, HS_J, 64)) + __shfl_down(v, 2 * HS_J, 64); }

template <int K>
__global__ __launch_bounds__(256) void hypothesis_stats_kernel(HsArgs a, unsigned* __restrict__ partial) {
  __shared__ unsigned s_rec[HS_NWV][HS_REC];
  constexpr int J = HS_J;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int slot = lane / J, j = lane - slot * J;                 // lanes 51-63: slot 3, idle
  const bool lane_on = slot < 3;
  const int src = min(slot, 2) * J;                               // the group's first lane
  constexpr int per_wave = HS_FPB / HS_NWV;
  const long f_begin = (long)blockIdx.x * HS_FPB + wave * per_wave, f_end = min(f_begin + per_wave, a.N);
  const float inf = __builtin_inff();
  const float pair_w = K > 1 ? 2.0f / (float)(K * (K - 1)) : 0.f;
  float a_jb = 0.f, a_spread = 0.f, a_topm = 0.f, a_mass = 0.f, a_misc = 0.f, a_wave = 0.f, a_pair = 0.f;
  int c_pbest = 0, c_shead = 0, c_orank = 0, c_agree = 0;
  int c_jhead[K];                                                 // wave-uniform (ballot counts)
#pragma unroll
  for (int k = 0; k < K; ++k) c_jhead[k] = 0;
  for (int s_ = 0; s_ < per_wave; s_ += 3) {                      // (wave-uniform trip count: the shuffles below see every lane)
    const long f0 = f_begin + s_;
    if (f0 >= f_end) break;                                       // wave-uniform
    const long f = f0 + slot;
    const bool valid = lane_on && f < f_end;
    const long fc = valid ? f : f_begin;                          // idle lanes read a valid frame and contribute nothing
    const long b = fc / a.T;
    const int t = (int)(fc - b * a.T);
    const int jc = lane_on ? j : 0;
    const float* gr = a.target + fc * (J * 3) + 3 * jc;
    const float g0 = a.target_scale * gr[0], g1 = a.target_scale * gr[1], g2 = a.target_scale * gr[2];
    float q[K][3], e[K], E[K], s[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const long row = (b * K + k) * a.T + t;
      const float* pr = a.poses + row * (J * 3) + 3 * jc;
      q[k][0] = a.pose_scale * pr[0]; q[k][1] = a.pose_scale * pr[1]; q[k][2] = a.pose_scale * pr[2];
      s[k] = a.scores[row];
      const float dx = q[k][0] - g0, dy = q[k][1] - g1, dz = q[k][2] - g2;
      e[k] = sqrtf(dx * dx + dy * dy + dz * dz);
      E[k] = __shfl(hs_group_sum(e[k], j), src, 64);              // the frame's pose error, in every lane of its group
    }
    // ---- the winners: first arg-min of the pose error, first arg-max of the score, first arg-min of this joint's distance ----
    int ko = 0, ks = 0, kj = 0;
    float Eo = E[0], sm = s[0], ej = e[0];
#pragma unroll
    for (int k = 1; k < K; ++k) {
      if (E[k] < Eo) { Eo = E[k]; ko = k; }
      if (s[k] > sm) { sm = s[k]; ks = k; }
      if (e[k] < ej) { ej = e[k]; kj = k; }
    }
    // ---- place of every hypothesis in the descending score order, ties to the smaller index ----
    int rank[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
      int r = 0;
#pragma unroll
      for (int i = 0; i < K; ++i)
        if (i != k) r += (s[i] > s[k] || (s[i] == s[k] && i < k)) ? 1 : 0;
      rank[k] = r;
    }
    float Es = E[0], so = s[0], s_own = s[0], tm = inf;
    int ro = rank[0];
#pragma unroll
    for (int k = 0; k < K; ++k) {
      if (k == ks) Es = E[k];
      if (k == ko) { so = s[k]; ro = rank[k]; }
      if (k == j) s_own = s[k];
      if (rank[k] <= j) tm = fminf(tm, E[k]);                     // lane j: best of the j + 1 best-scored hypotheses
    }
    // ---- weighted average, spread about it, mean pairwise distance: this joint ----
    float w0 = 0.f, w1 = 0.f, w2 = 0.f;
#pragma unroll
    for (int k = 0; k < K; ++k) { w0 += q[k][0] * s[k]; w1 += q[k][1] * s[k]; w2 += q[k][2] * s[k]; }
    float var = 0.f, pd = 0.f;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const float dx = q[k][0] - w0, dy = q[k][1] - w1, dz = q[k][2] - w2;
      var += s[k] * (dx * dx + dy * dy + dz * dz);
#pragma unroll
      for (int i = k + 1; i < K; ++i) {
        const float ux = q[k][0] - q[i][0], uy = q[k][1] - q[i][1], uz = q[k][2] - q[i][2];
        pd += sqrtf(ux * ux + uy * uy + uz * uz);
      }
    }
    const float wx = w0 - g0, wy = w1 - g1, wz = w2 - g2;
    if (valid) {
      a_jb += ej;
      a_spread += sqrtf(var);
      a_wave += sqrtf(wx * wx + wy * wy + wz * wz);
      a_pair += pair_w * pd;
      if (j < K) {
        a_topm += tm;
        a_mass += s_own;
        c_pbest += (j == ko) ? 1 : 0;
        c_shead += (j == ks) ? 1 : 0;
        c_orank += (j == ro) ? 1 : 0;
      }
      a_misc += j == 0 ? Es : j == 1 ? Eo : j == 2 ? so : j == 3 ? sm : 0.f;
      c_agree += (j == 0 && ko == ks) ? 1 : 0;
      if (a.jbest_idx != nullptr) a.jbest_idx[f * J + j] = (unsigned char)kj;
      if (a.jbest_pose != nullptr) {                              // the winner's input bits, unscaled
        const float* pr = a.poses + ((b * K + kj) * a.T + t) * (J * 3) + 3 * j;
        float* o = a.jbest_pose + f * (J * 3) + 3 * j;
        o[0] = pr[0]; o[1] = pr[1]; o[2] = pr[2];
      }
    }
#pragma unroll
    for (int k = 0; k < K; ++k) c_jhead[k] += __popcll(__ballot(valid && kj == k));
  }
  // ---- one record per workgroup: inside a wave by shuffle / DPP, across the waves through LDS, in wave order ----
  const float t_jb = hs_fold(a_jb), t_spread = hs_fold(a_spread), t_topm = hs_fold(a_topm), t_mass = hs_fold(a_mass), t_misc = hs_fold(a_misc);
  const int t_pbest = hs_fold(c_pbest), t_shead = hs_fold(c_shead), t_orank = hs_fold(c_orank);
  const float t_wave = wave_sum(lane_on ? a_wave : 0.f), t_pair = wave_sum(lane_on ? a_pair : 0.f);
  const int t_agree = wave_sum_i(lane_on ? c_agree : 0);
  unsigned* r = s_rec[wave];
  if (lane < J) {
    r[HS_JB_JOINT + lane] = __float_as_uint(t_jb);
    r[HS_SPREAD + lane] = __float_as_uint(t_spread);
  }
  if (lane < HS_KMAX) {                                          // slots K.. stay 0: nothing was added to them
    r[HS_TOPM + lane] = __float_as_uint(t_topm);
    r[HS_MASS + lane] = __float_as_uint(t_mass);
    r[HS_NF + HS_ORANK + lane] = (unsigned)t_orank;
    r[HS_NF + HS_PBEST + lane] = (unsigned)t_pbest;
    r[HS_NF + HS_SHEAD + lane] = (unsigned)t_shead;
    int cj = 0;
#pragma unroll
    for (int k = 0; k < K; ++k) cj = lane == k ? c_jhead[k] : cj;
    r[HS_NF + HS_JHEAD + lane] = (unsigned)cj;
  }
  if (lane < 4) r[lane == 0 ? HS_BEST : lane == 1 ? HS_ORACLE : lane == 2 ? HS_S_ORACLE : HS_S_MAX] = __float_as_uint(t_misc);
  if (lane == 0) {
    r[0] = 0u; r[HS_JBEST] = 0u; r[HS_REC - 1] = 0u;              // frames / the J-Best total: finalize kernel
    r[HS_WAVE] = __float_as_uint(t_wave);
    r[HS_PAIR] = __float_as_uint(t_pair);
    r[HS_NF + HS_AGREE] = (unsigned)t_agree;
  }
  __syncthreads();
  const int v = threadIdx.x;
  if (v < HS_REC) {
    unsigned out;
    if (v < HS_NF) {
      float x = __uint_as_float(s_rec[0][v]);
      for (int w = 1; w < HS_NWV; ++w) x += __uint_as_float(s_rec[w][v]);
      out = __float_as_uint(x);
    } else {
      out = s_rec[0][v];
      for (int w = 1; w < HS_NWV; ++w) out += s_rec[w][v];
    }
    partial[(long)blockIdx.x * HS_REC + v] = out;
  }
}

// Adds the records in block order: thread v owns word v of the rows (floats in double, counts in int64); the J-Best total is the sum of its
// 17 per-joint sums, the frame count comes from the shape.
__global__ __launch_bounds__(128) void hypothesis_stats_finalize_kernel(const unsigned* __restrict__ partial, int blocks, long frames,
                                                                        float* __restrict__ sums, long* __restrict__ counts) {
  __shared__ double s_joint[HS_J];
  const int v = threadIdx.x;
  if (v < HS_NF) {
    double x = 0.0;
    for (int r = 0; r < blocks; ++r) x += (double)__uint_as_float(partial[(long)r * HS_REC + v]);
    if (v >= HS_JB_JOINT && v < HS_JB_JOINT + HS_J) s_joint[v - HS_JB_JOINT] = x;
    if (v == 0) sums[0] = (float)frames;
    else if (v != HS_JBEST) sums[v] = (float)x;
  } else if (v < HS_NF + HS_NI) {
    long c = 0;
    for (int r = 0; r < blocks; ++r) c += (long)partial[(long)r * HS_REC + v];
    counts[v - HS_NF] = c;
  }
  __syncthreads();
  if (v == HS_JBEST) {
    double x = 0.0;
    for (int jj = 0; jj < HS_J; ++jj) x += s_joint[jj];
    sums[HS_JBEST] = (float)x;
  }
}

long hypothesis_stats_scratch_floats(long frames) { return (long)cdiv(frames > 0 ? frames : 1, HS_FPB) * HS_REC; }
int hypothesis_stats_row_floats() { return HS_NF; }
int hypothesis_stats_row_counts() { return HS_NI; }

int hypothesis_stats(const float* poses, const float* scores, const float* target, int B, int K, int T, float pose_scale, float target_scale,
                     float* sums, long* counts, float* jbest_pose, unsigned char* jbest_idx, float* scratch, long scratch_floats,
                     hipStream_t st) {
  MP_CHECK(poses && scores && target && sums && counts && scratch, MP_ERR_ARG, "hypothesis_stats: null pointer");
  MP_CHECK(B > 0 && K >= 1 && K <= HS_KMAX && T >= 1 && (long)B * T < (1L << 31), MP_ERR_ARG,
           "hypothesis_stats: B=%d K=%d T=%d unsupported (K <= %d, T >= 1)", B, K, T, HS_KMAX);
  MP_CHECK(((uintptr_t)counts & 7) == 0, MP_ERR_ARG, "hypothesis_stats: counts must be 8-byte aligned");
  HsArgs a = {};
  a.poses = poses; a.scores = scores; a.target = target;
  a.N = (long)B * T; a.T = T;
  a.pose_scale = pose_scale; a.target_scale = target_scale;
  a.jbest_pose = jbest_pose; a.jbest_idx = jbest_idx;
  const int blocks = cdiv(a.N, HS_FPB);
  MP_CHECK(scratch_floats >= (long)blocks * HS_REC, MP_ERR_ARG, "hypothesis_stats: scratch too small (%ld < %ld)", scratch_floats,
           (long)blocks * HS_REC);
  unsigned* partial = reinterpret_cast<unsigned*>(scratch);
  switch (K) {
#define HS_CASE(KK) \
    case KK: hipLaunchKernelGGL(hypothesis_stats_kernel<KK>, dim3(blocks), dim3(256), 0, st, a, partial); break;
    HS_CASE(1) HS_CASE(2) HS_CASE(3) HS_CASE(4) HS_CASE(5) HS_CASE(6) HS_CASE(7) HS_CASE(8)
#undef HS_CASE
  }
  MP_LAUNCH_CHECK();
  hipLaunchKernelGGL(hypothesis_stats_finalize_kernel, dim3(1), dim3(128), 0, st, partial, blocks, a.N, sums, counts);
  MP_LAUNCH_CHECK();
  return MP_OK;
}

}  // namespace mp

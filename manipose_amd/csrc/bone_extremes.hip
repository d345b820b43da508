// The evaluation quantities of predicted pose sequences that are NOT sums (the rest of pose_metrics.hip):
//   segments_max_strech_per_bone        hpe/mh_so3_hpe/metrics/regularizations.py:63-74   (min / max length of every bone over all frames)
//   segments_max_diff_strech_per_bone   regularizations.py:77-94   (largest frame-to-frame jump of every bone length, and where it is)
//   coordwise_error                     metrics/mean_joint_errors.py:133-141   (sum of |gt - pred| per coordinate; a sum, but not one of pose_metrics')
// One thread per frame of the flattened (B*L) frame list reads its 17 x 3 coordinates through the caller's element strides (as
// pose_metrics.hip: the reference's (B,3,J,L) views need no copy), forms the 16 bone lengths and leaves them in LDS, where its successor
// finds them; thread 0 of a block computes the frame ahead of the block as well (the same loop body a second time: the same bits as
// the block that owns that frame).  Values are reduced with DPP inside a wave, through LDS across the 4 waves, into ONE record per block;
// a second kernel merges the records.  No atomics: the result is the same bits in every run, and among equal jumps the smallest index wins
// (torch.max(dim) returns the first maximum) - indices grow with the frame number, so "first lane, first wave, first block" is that rule.
#include "common.h"
#include "kernels.h"

namespace mp {

constexpr int BX_J = 17, BX_NB = 16, BX_FR = 256, BX_NWV = BX_FR / 64, BX_PITCH = BX_NB + 1;      // LDS row pitch 17 dwords: odd, no bank conflicts
__device__ constexpr int BX_PARENT[BX_J] = {-1, 0, 1, 2, 0, 4, 5, 0, 7, 8, 9, 8, 11, 12, 8, 14, 15};     // pose_metrics.hip PM_PARENT
// per-block record, in floats: [0,16) min  [16,32) max  [32,48) largest jump (-1: none)  [48,51) sum |gt - pred| per coordinate  [51] unused
// [52,84) the 16 int64 indices of the largest jumps (byte offset 208: 8-byte aligned, as is the record size)
constexpr int BX_OMIN = 0, BX_OMAX = 16, BX_OJMP = 32, BX_OSUM = 48, BX_OIDX = 52, BX_REC = 84;

struct BxArgs {
  const float* pred; long ps[4];         // element strides of (b, t, j, c)
  const float* gt; long gs[4];           // nullable
  const float* prev_len;                 // nullable: bone lengths of the frame ahead of frame 0 (chain only)
  long N, frame_base;                    // N = B * L frames
  int L, chain;
  float pred_scale, gt_scale;
};

__device__ __forceinline__ float wave_min(float v) { return -wave_max(-v); }

// index of the difference between frames f - 1 and f
__device__ __forceinline__ long bx_index(const BxArgs& a, long f) {
  if (a.chain) return a.frame_base + f - 1;
  const long b = f / a.L;
  return b * (a.L - 1) + (f - b * a.L) - 1;
}

__global__ __launch_bounds__(BX_FR) void bone_extremes_kernel(BxArgs a, float* __restrict__ partial, float* __restrict__ last_len) {
  __shared__ float lens[(BX_FR + 1) * BX_PITCH];      // row r + 1 = the block's frame r, row 0 = the frame ahead of the block
  __shared__ float w_min[BX_NWV][BX_NB], w_max[BX_NWV][BX_NB], w_jmp[BX_NWV][BX_NB], w_sum[BX_NWV][3];
  __shared__ int w_first[BX_NWV][BX_NB];              // frame offset inside the block of a wave's first largest jump
  constexpr int J = BX_J, NB = BX_NB;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const long f0 = (long)blockIdx.x * BX_FR, f = f0 + tid;
  const bool live = f < a.N;
  const long b = live ? f / a.L : 0;
  const int t = (int)(f - b * a.L);
  // has this frame a predecessor to be differenced with, and is it a frame of this call (else: prev_len)?
  const bool in_call = live && f > 0 && (a.chain || t > 0);
  const bool from_prev = live && f == 0 && a.chain && a.prev_len != nullptr;
  float x[J][3], len[NB];
  // offset -1 (thread 0 only): the frame ahead of the block, into row 0.  ONE loop body for both frames, so that a length has the same bits
  // wherever it is computed.
  const int first = !live ? 1 : (tid == 0 && in_call) ? -1 : 0;
#pragma unroll 1
  for (int o = first; o <= 0; ++o) {
    const long g = f + o, gb = g / a.L, gt_ = g - gb * a.L;
    const float* base = a.pred + gb * a.ps[0] + gt_ * a.ps[1];
#pragma unroll
    for (int j = 0; j < J; ++j) {
      x[j][0] = a.pred_scale * base[j * a.ps[2]];
      x[j][1] = a.pred_scale * base[j * a.ps[2] + a.ps[3]];
      x[j][2] = a.pred_scale * base[j * a.ps[2] + 2 * a.ps[3]];
    }
#pragma unroll
    for (int k = 0; k < NB; ++k) {
      const int j = k + 1, p = BX_PARENT[k + 1];
      const float dx = x[j][0] - x[p][0], dy = x[j][1] - x[p][1], dz = x[j][2] - x[p][2];
      len[k] = sqrtf(dx * dx + dy * dy + dz * dz);
      lens[(tid + 1 + o) * BX_PITCH + k] = len[k];
    }
  }
  if (from_prev)
    for (int k = 0; k < NB; ++k) lens[k] = a.prev_len[k];
  if (live && f == a.N - 1)
    for (int k = 0; k < NB; ++k) last_len[k] = len[k];
  // sum |gt - pred| per coordinate over the joints of this frame
  float cs[3] = {0.f, 0.f, 0.f};
  if (live && a.gt != nullptr) {
    const float* base = a.gt + b * a.gs[0] + t * a.gs[1];
#pragma unroll
    for (int j = 0; j < J; ++j)
#pragma unroll
      for (int c = 0; c < 3; ++c) cs[c] += fabsf(a.gt_scale * base[j * a.gs[2] + c * a.gs[3]] - x[j][c]);
  }
  __syncthreads();                         // every frame's lengths are in LDS
  const bool has_diff = in_call || from_prev;
  const float inf = __builtin_inff();
#pragma unroll
  for (int k = 0; k < NB; ++k) {
    const float mn = wave_min(live ? len[k] : inf), mx = wave_max(live ? len[k] : -inf);
    const float d = has_diff ? fabsf(len[k] - lens[tid * BX_PITCH + k]) : -1.f;
    const float md = wave_max(d);
    const float fl = wave_min((has_diff && d == md) ? (float)lane : 64.f);        // first lane that holds the wave's largest jump
    if (lane == 0) {
      w_min[wv][k] = mn; w_max[wv][k] = mx; w_jmp[wv][k] = md;
      w_first[wv][k] = wv * 64 + (int)fl;
    }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float s = wave_sum(cs[c]);
    if (lane == 0) w_sum[wv][c] = s;
  }
  __syncthreads();
  float* rec = partial + (long)blockIdx.x * BX_REC;
  if (tid < NB) {
    float mn = w_min[0][tid], mx = w_max[0][tid], md = w_jmp[0][tid];
    int at = w_first[0][tid];
    for (int w = 1; w < BX_NWV; ++w) {
      mn = fminf(mn, w_min[w][tid]);
      mx = fmaxf(mx, w_max[w][tid]);
      if (w_jmp[w][tid] > md) { md = w_jmp[w][tid]; at = w_first[w][tid]; }      // strictly larger: the earlier wave keeps a tie
    }
    rec[BX_OMIN + tid] = mn; rec[BX_OMAX + tid] = mx; rec[BX_OJMP + tid] = md;
    reinterpret_cast<long*>(rec + BX_OIDX)[tid] = md >= 0.f ? bx_index(a, f0 + at) : -1;
  } else if (tid < NB + 3) {
    const int c = tid - NB;
    float s = w_sum[0][c];
    for (int w = 1; w < BX_NWV; ++w) s += w_sum[w][c];
    rec[BX_OSUM + c] = s;
  }
}

// Merges the block records in block order.  4 waves; wave w takes bones 4 w .. 4 w + 3: its lanes stride over the records (each lane's own
// records come in rising order, so "strictly larger" keeps its first), then the wave's largest value and, among the lanes that hold it, the
// lowest record number (exact in fp32: < 2^24 records) decide - that lane writes its index.  Thread c < 3 adds the coordinate sums in
// double, in record order.
__global__ __launch_bounds__(256) void bone_extremes_finalize_kernel(const float* __restrict__ partial, int blocks, float* __restrict__ min_len,
                                                                     float* __restrict__ max_len, float* __restrict__ max_delta,
                                                                     long* __restrict__ max_delta_idx, float* __restrict__ coord_sums) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const float inf = __builtin_inff();
  for (int q = 0; q < 4; ++q) {
    const int k = 4 * wv + q;
    float mn = inf, mx = -inf, md = -1.f, at = 16777216.f;
    long idx = -1;
    for (int r = lane; r < blocks; r += 64) {
      const float* rec = partial + (long)r * BX_REC;
      mn = fminf(mn, rec[BX_OMIN + k]);
      mx = fmaxf(mx, rec[BX_OMAX + k]);
      if (rec[BX_OJMP + k] > md) { md = rec[BX_OJMP + k]; at = (float)r; idx = reinterpret_cast<const long*>(rec + BX_OIDX)[k]; }
    }
    mn = wave_min(mn); mx = wave_max(mx);
    const float best = wave_max(md);
    const float who = wave_min((md == best && md >= 0.f) ? at : 16777216.f);
    if (lane == 0) {
      min_len[k] = mn; max_len[k] = mx; max_delta[k] = best;
      if (best < 0.f) max_delta_idx[k] = -1;
    }
    if (best >= 0.f && md == best && at == who) max_delta_idx[k] = idx;      // one lane: record numbers are distinct
  }
  if (coord_sums != nullptr && threadIdx.x < 3) {
    double s = 0.0;
    for (int r = 0; r < blocks; ++r) s += (double)partial[(long)r * BX_REC + BX_OSUM + threadIdx.x];
    coord_sums[threadIdx.x] = (float)s;
  }
}

long bone_extremes_scratch_floats(long frames) { return (long)cdiv(frames, BX_FR) * BX_REC; }

int bone_extremes(const float* pred, const long* ps, const float* gt, const long* gs, int B, int L, int J, float pred_scale, float gt_scale,
                  int chain, const float* prev_len, long frame_base, float* min_len, float* max_len, float* max_delta, long* max_delta_idx,
                  float* coord_sums, float* last_len, float* scratch, long scratch_floats, hipStream_t st) {
  MP_CHECK(pred && ps && min_len && max_len && max_delta && max_delta_idx && last_len && scratch, MP_ERR_ARG, "bone_extremes: null pointer");
  MP_CHECK(J == BX_J, MP_ERR_ARG, "bone_extremes: %d joints; the 17-joint H36M / 3DHP tree is compiled in", J);
  MP_CHECK(B > 0 && L > 0 && (long)B * L < (1L << 31), MP_ERR_ARG, "bone_extremes: B=%d L=%d", B, L);
  MP_CHECK(gt == nullptr || (gs != nullptr && coord_sums != nullptr), MP_ERR_ARG, "bone_extremes: target without strides or without coord_sums");
  MP_CHECK(((uintptr_t)scratch & 7) == 0, MP_ERR_ARG, "bone_extremes: scratch must be 8-byte aligned");
  BxArgs a = {};
  a.pred = pred; a.gt = gt; a.prev_len = chain ? prev_len : nullptr;
  for (int i = 0; i < 4; ++i) { a.ps[i] = ps[i]; a.gs[i] = gt ? gs[i] : 0; }
  a.N = (long)B * L; a.frame_base = frame_base; a.L = L; a.chain = chain != 0;
  a.pred_scale = pred_scale; a.gt_scale = gt_scale;
  const int blocks = cdiv(a.N, BX_FR);
  MP_CHECK(scratch_floats >= (long)blocks * BX_REC, MP_ERR_ARG, "bone_extremes: scratch too small (%ld < %ld)", scratch_floats, (long)blocks * BX_REC);
  hipLaunchKernelGGL(bone_extremes_kernel, dim3(blocks), dim3(BX_FR), 0, st, a, scratch, last_len);
  MP_LAUNCH_CHECK();
  hipLaunchKernelGGL(bone_extremes_finalize_kernel, dim3(1), dim3(256), 0, st, scratch, blocks, min_len, max_len, max_delta, max_delta_idx,
                     gt ? coord_sums : nullptr);
  MP_LAUNCH_CHECK();
  return MP_OK;
}

}  // namespace mp

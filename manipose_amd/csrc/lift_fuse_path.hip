// Fusing the camera views of a take ALONG TIME (include/manipose_hip.h: mp_lift_fuse_path): one hypothesis per view and frame, chosen jointly over
// the views (as mp_lift_fuse) AND over the whole take (as mp_lift_path) - the Viterbi path through the K^V combinations of a frame, at most 4096
// states.  The transition is a sum over the views, so the forward step is STAGED per view (V K^(V+1) operations a frame, not K^(2V)); the staged
// order of additions is the rule.  tests/lift_fuse_path_ref.py states it in float64.  Three kernels on one stream:
//   tables: fully parallel over frames.  ONE WORKGROUP OWNS A TILE of TF consecutive frames and rotates them plus the frame before the tile into
//           LDS, once per (frame, view, hypothesis, joint); then one lane owns one entry of the frame's row in the scratch:
//             [pair costs d (V (V - 1) / 2, K, K) | transitions t (V, K, K), a-major | unary costs u (V, K)]   doubles,
//           an entry that belongs to a view invalid at the frame (for t: at the frame or the one before) written as +0, which adds nothing to a
//           sum: the scan needs no masks.  t at the first frame of a take is computed against whatever frame lies before it and never read.
//   scan:   ONE WORKGROUP PER TAKE, one instantiation per K with one state per lane (K^V <= 1024, the workgroup K^V lanes rounded up to whole waves)
//           and three with four (K = 6, 7, 8 at V = 4: up to 4096 states on at most 1024 lanes).  A lane keeps the digits of its states packed in a register (3 bits a view); the state
//           vector lives in LDS twice, stage v reads one copy with stride K^(V-1-v) doubles and writes the other, ONE barrier per stage.  Banks:
//           the K reads of a lane's group differ by the stride; across the 32 lanes of a half-wave, at the last stage (stride 1) K neighbours
//           read one address (a broadcast) and the groups lie K doubles apart - for K = 5 and 8 the 7 and 4 addresses fall on different 8-byte
//           banks - and at the earlier stages runs of consecutive lanes read consecutive doubles; the write is linear.  The last stage adds the
//           frame cost, formed from the row's tables in mp_lift_fuse's order.  The next frame's row is loaded into registers at the head of a
//           frame and stored to the other row buffer before the frame's last barrier.  Back-pointers: one 16-bit word per state and frame.  The
//           backtrack stages them into the LDS the forward pass has left, at most MP_LIFT_FUSE_PATH_CHUNK frames at a time, one lane walks
//           the chunk (the digits kept apart: no division), all lanes store the path.
//   emit:   ONE LANE OWNS ONE FRAME: the frame cost of the chosen state from the row, in the scan's order (the same bits); the views' rotations
//           re-made in registers (the view loop is unrolled: nothing is indexed at run time), mean and spread in joint order, views in order.
// The rotation and the view test are lift_geom.h's, shared with lift_fuse.hip (compiled here without contraction: the header is included after
// the pragma); mp_lift_fuse's emit step is restated for one lane per frame.
// Everything between the float32 loads and the stores is fp64 without contraction; a take's frames are its CLAMPED range and every digit read
// back is clamped to K - 1, so whatever the device table holds nothing outside the arrays is touched.  No atomics: identical bits on every call.
#include <algorithm>

#include "lift_common.h"

#pragma clang fp contract(off)
#include "lift_geom.h"                    // after the pragma: the shared code takes this file's mode

namespace mp {

constexpr int FP_MAXV = MP_LIFT_FUSE_MAXV, FP_MAXK = MP_LIFT_FUSE_MAXK;
constexpr int FP_CHUNK = MP_LIFT_FUSE_PATH_CHUNK;                      // frames of a backtrack chunk at most
constexpr int FP_PRE = 4;                                              // doubles of the next row a lane holds in flight (rows <= 4 x lanes: host check)
constexpr double FP_BIG = 1e30;
constexpr long FP_TILE_LDS = 60 * 1024;                                // the tables kernel's rotated frames
constexpr long FP_SCAN_MIN_LDS = 32 * 1024;                            // the scan's main region at least: what a backtrack chunk gets
static_assert(FP_MAXV == 4 && FP_MAXK <= 8, "3 bits a view, 4 views: 12 bits of a 16-bit back-pointer word");
static_assert(FP_CHUNK >= 1 && FP_CHUNK <= 1024, "the path of a chunk lives in LDS");

struct FusePathArgs {
  const float* hyps;             // (V, Ftot, K, J, C)
  const unsigned char* valid;    // (V, Ftot) or null
  const long* take_offset;       // (G + 1) device
  const float* quat;             // (G, V, 4) device or null
  double* rows;                  // (Ftot, R) scratch
  unsigned short* bp;            // (Ftot, S) scratch: back-pointer words
  unsigned short* path;          // (Ftot) scratch: the chosen state
  float* pose;                   // (Ftot, J, 3)
  unsigned char* choice;         // (Ftot, V)
  float* cost;                   // (Ftot)
  float* spread;                 // (Ftot)
  unsigned char* ok;             // (Ftot)
  double* path_cost;             // (G) or null
  long Ftot;
  double pair_factor, score_weight, path_factor, switch_cost;          // 1 / (2 sigma^2), score_weight, 1 / (2 path_sigma^2), switch_cost
  int V, K, J, C, G;
  int S, NP, R;                  // K^V states, V (V - 1) / 2 pairs, doubles of a row
  int TF, frame_doubles;         // tables: frames of a tile, doubles of a rotated frame in LDS
  int lds_main, chunk;           // scan: bytes of its main LDS region, frames of a backtrack chunk
};

__global__ __launch_bounds__(POSE_THREADS) void lift_fuse_path_tables_kernel(FusePathArgs A) {
  extern __shared__ __attribute__((aligned(16))) unsigned char fpt_lds[];
  const int V = A.V, K = A.K, J = A.J, C = A.C, TF = A.TF, KK = K * K, R = A.R, VKJ = V * K * J;
  const int tid = threadIdx.x;
  const long t0 = (long)blockIdx.x * TF;
  double* fr = (double*)fpt_lds;                                       // [TF + 1][frame_doubles]: slot h is frame t0 - 1 + h
  int* vok = (int*)(fr + (long)(TF + 1) * A.frame_doubles);            // [TF + 1][FP_MAXV]
  if (tid < (TF + 1) * FP_MAXV) {                                      // (TF <= 8: 36 lanes at most)
    const int h = tid / FP_MAXV, v = tid % FP_MAXV;
    const long gf = t0 - 1 + h;
    int good = 0;
    if (v < V && gf >= 0 && gf < A.Ftot) {
      const int g = lift_seq_of(A.take_offset, A.G, gf);
      if (lift_view_ok(A.valid, A.quat, V, A.Ftot, gf, g, v)) {
        Rot3 Q;
        lift_rot3(A.quat != nullptr ? A.quat + ((long)g * V + v) * 4 : nullptr, Q);
        double* r = fr + (long)h * A.frame_doubles + v * 9;
        r[0] = Q.r00; r[1] = Q.r01; r[2] = Q.r02; r[3] = Q.r10; r[4] = Q.r11; r[5] = Q.r12; r[6] = Q.r20; r[7] = Q.r21; r[8] = Q.r22;
        good = 1;
      }
    }
    vok[tid] = good;
  }
  __syncthreads();
  // 1. rotate, and the unary costs of the tile's own frames
  for (int idx = tid; idx < (TF + 1) * VKJ; idx += POSE_THREADS) {
    const int h = idx / VKJ, it = idx - h * VKJ, v = it / (K * J), k = (it / J) % K, j = it % J;
    const long gf = t0 - 1 + h;
    const bool good = vok[h * FP_MAXV + v] != 0;                        // (0 for a frame outside 0 .. Ftot - 1)
    double u = 0.0;
    if (good) {                                                         // an invalid view's data is never looked at
      const float* x0 = A.hyps + (((long)v * A.Ftot + gf) * K + k) * J * C;
      const float* xj = x0 + j * C;
      const double dx = (double)xj[0] - (double)x0[0], dy = (double)xj[1] - (double)x0[1], dz = (double)xj[2] - (double)x0[2];
      double* w = fr + (long)h * A.frame_doubles + FP_MAXV * 9 + (long)it * 3;
      if (A.quat != nullptr) {
        const double* r = fr + (long)h * A.frame_doubles + v * 9;
        w[0] = r[0] * dx + r[1] * dy + r[2] * dz;
        w[1] = r[3] * dx + r[4] * dy + r[5] * dz;
        w[2] = r[6] * dx + r[7] * dy + r[8] * dz;
      } else {
        w[0] = dx; w[1] = dy; w[2] = dz;                                // nothing is multiplied: the differences are exact
      }
      if (j == 0 && C == 4) {
        double s = x0[3];
        if (!(s > 1e-12)) s = 1e-12;
        u = -log(s);
      }
    }
    if (j == 0 && h >= 1 && gf < A.Ftot) A.rows[gf * R + (long)(A.NP + V) * KK + v * K + k] = u;
  }
  __syncthreads();
  // 2. pair costs of the tile's frames
  for (int idx = tid; idx < TF * A.NP * KK; idx += POSE_THREADS) {
    const int t = idx / (A.NP * KK), e = idx - t * (A.NP * KK), p = e / KK, i = (e / K) % K, l = e % K;
    const long g = t0 + t;
    if (g >= A.Ftot) break;
    int a = 0, b = 1;                                                   // pair p in lexicographic order of (a, b), a < b < V
    for (int q = 0; q < p; ++q) { if (++b == V) { ++a; b = a + 1; } }
    double d = 0.0;
    if (vok[(t + 1) * FP_MAXV + a] && vok[(t + 1) * FP_MAXV + b]) {
      const double* wa = fr + (long)(t + 1) * A.frame_doubles + FP_MAXV * 9 + (long)(a * K + i) * J * 3;
      const double* wb = fr + (long)(t + 1) * A.frame_doubles + FP_MAXV * 9 + (long)(b * K + l) * J * 3;
      double s = 0.0;
      for (int j = 0; j < J; ++j) {                                     // joint order, then channel order
        const double ex = wa[j * 3] - wb[j * 3], ey = wa[j * 3 + 1] - wb[j * 3 + 1], ez = wa[j * 3 + 2] - wb[j * 3 + 2];
        s += ex * ex; s += ey * ey; s += ez * ez;
      }
      d = s / (double)J;
      if (!__builtin_isfinite(d)) d = FP_BIG;
    }
    A.rows[g * R + e] = d;
  }
  // 3. transitions of every view from the frame before
  for (int idx = tid; idx < TF * V * KK; idx += POSE_THREADS) {
    const int t = idx / (V * KK), e = idx - t * (V * KK), v = e / KK, a = (e / K) % K, b = e % K;
    const long g = t0 + t;
    if (g >= A.Ftot) break;
    double d = 0.0;
    if (vok[(t + 1) * FP_MAXV + v] && vok[t * FP_MAXV + v]) {           // (the view's chain is cut across a gap)
      const double* wb = fr + (long)(t + 1) * A.frame_doubles + FP_MAXV * 9 + (long)(v * K + b) * J * 3;
      const double* wa = fr + (long)t * A.frame_doubles + FP_MAXV * 9 + (long)(v * K + a) * J * 3;
      double s = 0.0;
      for (int j = 0; j < J; ++j) {
        const double ex = wb[j * 3] - wa[j * 3], ey = wb[j * 3 + 1] - wa[j * 3 + 1], ez = wb[j * 3 + 2] - wa[j * 3 + 2];
        s += ex * ex; s += ey * ey; s += ez * ez;
      }
      d = A.path_factor * (s / (double)J) + (a != b ? A.switch_cost : 0.0);
      if (!__builtin_isfinite(d)) d = FP_BIG;
    }
    A.rows[g * R + (long)A.NP * KK + e] = d;
  }
}

// E(c) of the state whose digits are packed in dg, from a frame's row: the pairs in lexicographic order, then the unary terms in view order
__device__ __forceinline__ double fp_frame_cost(const double* row, int dg, int V, int K, int NP, double pair_factor, double score_weight) {
  const int KK = K * K;
  double pairs = 0.0, unary = 0.0;
  int p = 0;
#pragma unroll
  for (int a = 0; a < FP_MAXV; ++a)
#pragma unroll
    for (int b = a + 1; b < FP_MAXV; ++b)
      if (b < V) { pairs += row[p * KK + ((dg >> (3 * a)) & 7) * K + ((dg >> (3 * b)) & 7)]; ++p; }
#pragma unroll
  for (int v = 0; v < FP_MAXV; ++v)
    if (v < V) unary += row[(NP + V) * KK + v * K + ((dg >> (3 * v)) & 7)];
  return pair_factor * pairs + score_weight * unary;
}

// NS: states a lane owns, c = tid + i blockDim.x.  K is a template argument: the loop over a is unrolled to exactly K steps, so a stage's 2 K LDS
// reads are issued together and the stage waits for one round trip, not K
template <int NS, int K>
__global__ __launch_bounds__(1024) void lift_fuse_path_scan_kernel(FusePathArgs A) {
  extern __shared__ __attribute__((aligned(16))) unsigned char fps_lds[];
  const int V = A.V, S = A.S, R = A.R, NP = A.NP;
  constexpr int KK = K * K;
  const int tid = threadIdx.x, NT = blockDim.x, lane = tid & 63, wave = tid >> 6;
  double* hb = (double*)fps_lds;                                       // [2][S] the state vector, twice
  double* rb = hb + 2 * S;                                             // [2][R] the current and the next frame's row
  double* redv = (double*)(fps_lds + A.lds_main);                      // [16] a wave's minimum
  int* redc = (int*)(redv + 16);                                       // [16] and its state
  unsigned short* pl = (unsigned short*)(redc + 16);                   // [FP_CHUNK] the path of a backtrack chunk
  const int take = blockIdx.x;
  const FrameRange r = lift_seq_frames(A.take_offset, take, A.Ftot);
  if (r.f1 <= r.f0) {
    if (tid == 0 && A.path_cost != nullptr) A.path_cost[take] = 0.0;
    return;
  }
  int st[FP_MAXV];                                                     // K^(V-1-v), view 0 most significant (every use below is unrolled)
  {
    int s = 1;
#pragma unroll
    for (int v = FP_MAXV - 1; v >= 0; --v) {
      st[v] = 0;
      if (v < V) { st[v] = s; s *= K; }
    }
  }
  int dg[NS];
#pragma unroll
  for (int i = 0; i < NS; ++i) {
    const int c = tid + i * NT;
    dg[i] = 0;
    if (c < S) {
#pragma unroll
      for (int v = 0; v < FP_MAXV; ++v)
        if (v < V) dg[i] |= ((c / st[v]) % K) << (3 * v);
    }
  }

  for (int idx = tid; idx < R; idx += NT) rb[idx] = A.rows[r.f0 * R + idx];
  __syncthreads();
#pragma unroll
  for (int i = 0; i < NS; ++i) {
    const int c = tid + i * NT;
    if (c < S) hb[c] = fp_frame_cost(rb, dg[i], V, K, NP, A.pair_factor, A.score_weight);
  }
  if (r.f0 + 1 < r.f1)
    for (int idx = tid; idx < R; idx += NT) rb[R + idx] = A.rows[(r.f0 + 1) * R + idx];
  __syncthreads();

  int hc = 0, rc = 1;                                                  // the buffers that hold f[g - 1] and row g
  for (long g = r.f0 + 1; g < r.f1; ++g) {
    double pre[FP_PRE];                                                // row g + 1, on its way while frame g is worked through
    const bool more = g + 1 < r.f1;
#pragma unroll
    for (int i = 0; i < FP_PRE; ++i) {
      const int idx = i * NT + tid;
      pre[i] = (more && idx < R) ? A.rows[(g + 1) * R + idx] : 0.0;
    }
    const double* row = rb + rc * R;
    int bpw[NS];
    double Eg[NS];                                                     // the frame cost of the lane's states: read now, added at the last stage
#pragma unroll
    for (int i = 0; i < NS; ++i) {
      bpw[i] = 0;
      Eg[i] = tid + i * NT < S ? fp_frame_cost(row, dg[i], V, K, NP, A.pair_factor, A.score_weight) : 0.0;
    }
#pragma unroll
    for (int v = 0; v < FP_MAXV; ++v) {
      if (v < V) {                                                      // (uniform: every lane meets the barrier)
        const double* hin = hb + hc * S;
        double* hout = hb + (hc ^ 1) * S;
        const double* T = row + (NP + v) * KK;
#pragma unroll
        for (int i = 0; i < NS; ++i) {
          const int c = tid + i * NT;
          if (c < S) {
            const int b = (dg[i] >> (3 * v)) & 7;
            const double* hg = hin + (c - b * st[v]);
            double best = __builtin_inf();
            int arg = 0;
#pragma unroll
            for (int a = 0; a < K; ++a) {
              const double val = hg[a * st[v]] + T[a * K + b];
              if (val < best) { best = val; arg = a; }                  // the FIRST arg-min
            }
            if (v == V - 1) best = best + Eg[i];
            hout[c] = best;
            bpw[i] |= arg << (3 * v);
          }
        }
        if (v == V - 1 && more) {
#pragma unroll
          for (int i = 0; i < FP_PRE; ++i) {
            const int idx = i * NT + tid;
            if (idx < R) rb[(rc ^ 1) * R + idx] = pre[i];               // (that buffer's last readers passed the barrier that ended frame g - 1)
          }
        }
        __syncthreads();
        hc ^= 1;
      }
    }
#pragma unroll
    for (int i = 0; i < NS; ++i) {
      const int c = tid + i * NT;
      if (c < S) A.bp[g * S + c] = (unsigned short)bpw[i];
    }
    rc ^= 1;
  }

  // the end state: the first minimum of f in lexicographic order (a lane's own states increase; then lowest cost, then lowest state)
  const double* hf = hb + hc * S;
  double best = __builtin_inf();
  int bc = 0x7fffffff;
#pragma unroll
  for (int i = 0; i < NS; ++i) {
    const int c = tid + i * NT;
    if (c < S) {
      const double v = hf[c];
      if (bc == 0x7fffffff || v < best) { best = v; bc = c; }
    }
  }
  for (int off = 32; off > 0; off >>= 1) {
    const double oe = __shfl_xor(best, off);
    const int oc = __shfl_xor(bc, off);
    if (oc != 0x7fffffff && (bc == 0x7fffffff || oe < best || (oe == best && oc < bc))) { best = oe; bc = oc; }
  }
  if (lane == 0) { redv[wave] = best; redc[wave] = bc; }
  __threadfence();                                                     // (the back-pointers other lanes wrote are read below)
  __syncthreads();
  int d0 = 0, d1 = 0, d2 = 0, d3 = 0;                                  // lane 0: the digits of the state, kept apart
  if (tid == 0) {
    const int waves = (NT + 63) >> 6;
    for (int w = 1; w < waves; ++w) {
      const double oe = redv[w];
      const int oc = redc[w];
      if (oc != 0x7fffffff && (bc == 0x7fffffff || oe < best || (oe == best && oc < bc))) { best = oe; bc = oc; }
    }
    bc = min(bc, S - 1);
    if (A.path_cost != nullptr) A.path_cost[take] = best;
    if (V > 0) d0 = (bc / st[0]) % K;
    if (V > 1) d1 = (bc / st[1]) % K;
    if (V > 2) d2 = (bc / st[2]) % K;
    if (V > 3) d3 = (bc / st[3]) % K;
  }
  __syncthreads();                                                     // (every lane is done with hb: the chunks overwrite it)

  // backtrack, from the last chunk to the first; the words of frame g name the state at g - 1, those of f0 do not exist
  unsigned short* bpl = (unsigned short*)fps_lds;                      // [chunk][S]
  const int CH = A.chunk;
  for (long c1 = r.f1; c1 > r.f0; c1 -= CH) {
    const long b0 = max(c1 - CH, r.f0);
    const int n = (int)(c1 - b0);
    for (int idx = (b0 == r.f0 ? S : 0) + tid; idx < n * S; idx += NT) bpl[idx] = A.bp[b0 * S + idx];
    __syncthreads();
    if (tid == 0) {
      const int km = K - 1;
      for (int t = n - 1; t >= 0; --t) {
        pl[t] = (unsigned short)(d0 * st[0] + d1 * st[1] + d2 * st[2] + d3 * st[3]);
        if (b0 + t > r.f0) {                                            // the inverse of the staging: view V - 1 first, the state updated in between
          const unsigned short* wt = bpl + (long)t * S;
          if (V > 3) d3 = min((wt[d0 * st[0] + d1 * st[1] + d2 * st[2] + d3 * st[3]] >> 9) & 7, km);
          if (V > 2) d2 = min((wt[d0 * st[0] + d1 * st[1] + d2 * st[2] + d3 * st[3]] >> 6) & 7, km);
          if (V > 1) d1 = min((wt[d0 * st[0] + d1 * st[1] + d2 * st[2] + d3 * st[3]] >> 3) & 7, km);
          d0 = min(wt[d0 * st[0] + d1 * st[1] + d2 * st[2] + d3 * st[3]] & 7, km);
        }
      }
    }
    __syncthreads();
    for (int t = tid; t < n; t += NT) A.path[b0 + t] = pl[t];
    __syncthreads();
  }
}

__global__ __launch_bounds__(64) void lift_fuse_path_emit_kernel(FusePathArgs A) {
  const int V = A.V, K = A.K, J = A.J, C = A.C;
  const long f = (long)blockIdx.x * 64 + threadIdx.x;
  if (f >= A.Ftot) return;
  const int g = lift_seq_of(A.take_offset, A.G, f);
  const FrameRange r = lift_seq_frames(A.take_offset, g, A.Ftot);
  if (f < r.f0 || f >= r.f1) return;                                    // a frame no take holds has no path
  int c = min((int)A.path[f], A.S - 1), dg = 0, mask = 0, n = 0;
#pragma unroll
  for (int v = FP_MAXV - 1; v >= 0; --v)
    if (v < V) {
      dg |= (c % K) << (3 * v);
      c /= K;
      if (lift_view_ok(A.valid, A.quat, V, A.Ftot, f, g, v)) { mask |= 1 << v; ++n; }
    }
  if (n == 0) {
    for (int it = 0; it < J * 3; ++it) A.pose[f * J * 3 + it] = 0.f;
    for (int v = 0; v < V; ++v) A.choice[f * V + v] = 255;
    A.cost[f] = 0.f; A.spread[f] = 0.f; A.ok[f] = 0;
    return;
  }
  const double E = fp_frame_cost(A.rows + f * A.R, dg, V, K, A.NP, A.pair_factor, A.score_weight);
  Rot3 Q[FP_MAXV];
  const float* x[FP_MAXV];
#pragma unroll
  for (int v = 0; v < FP_MAXV; ++v) {
    x[v] = nullptr;
    if (v < V && ((mask >> v) & 1)) {
      lift_rot3(A.quat != nullptr ? A.quat + ((long)g * V + v) * 4 : nullptr, Q[v]);
      x[v] = A.hyps + (((long)v * A.Ftot + f) * K + ((dg >> (3 * v)) & 7)) * J * C;
    }
  }
  double dev = 0.0;
  for (int j = 0; j < J; ++j) {
    double wx[FP_MAXV], wy[FP_MAXV], wz[FP_MAXV], sx = 0.0, sy = 0.0, sz = 0.0;
#pragma unroll
    for (int v = 0; v < FP_MAXV; ++v) {
      wx[v] = 0.0; wy[v] = 0.0; wz[v] = 0.0;
      if (x[v] != nullptr) {
        const double dx = (double)x[v][j * C] - (double)x[v][0], dy = (double)x[v][j * C + 1] - (double)x[v][1],
                     dz = (double)x[v][j * C + 2] - (double)x[v][2];
        if (A.quat != nullptr) {
          wx[v] = Q[v].r00 * dx + Q[v].r01 * dy + Q[v].r02 * dz;
          wy[v] = Q[v].r10 * dx + Q[v].r11 * dy + Q[v].r12 * dz;
          wz[v] = Q[v].r20 * dx + Q[v].r21 * dy + Q[v].r22 * dz;
        } else {
          wx[v] = dx; wy[v] = dy; wz[v] = dz;
        }
        sx += wx[v]; sy += wy[v]; sz += wz[v];                          // the sum in view order
      }
    }
    const double mx = sx / (double)n, my = sy / (double)n, mz = sz / (double)n;
#pragma unroll
    for (int v = 0; v < FP_MAXV; ++v)
      if (x[v] != nullptr) {
        const double ex = wx[v] - mx, ey = wy[v] - my, ez = wz[v] - mz;
        dev += ex * ex; dev += ey * ey; dev += ez * ez;
      }
    float* o = A.pose + (f * J + j) * 3;
    o[0] = j == 0 ? 0.f : (float)mx; o[1] = j == 0 ? 0.f : (float)my; o[2] = j == 0 ? 0.f : (float)mz;      // joint 0 is stored as +0
  }
#pragma unroll
  for (int v = 0; v < FP_MAXV; ++v)
    if (v < V) A.choice[f * V + v] = ((mask >> v) & 1) ? (unsigned char)((dg >> (3 * v)) & 7) : (unsigned char)255;
  A.cost[f] = (float)E;
  A.spread[f] = (float)sqrt(dev / ((double)n * (double)J));
  A.ok[f] = E >= FP_BIG ? 0 : 1;
}

struct FpShape { int S, NP, R; };
static FpShape fp_shape(int V, int K) {
  int S = 1;
  for (int v = 0; v < V; ++v) S *= K;
  const int NP = V * (V - 1) / 2;
  return {S, NP, (NP + V) * K * K + V * K};
}

static long fp_scratch_bytes(int V, long Ftot, int K) {
  const FpShape s = fp_shape(V, K);
  return (Ftot * (8L * s.R + 2L * s.S + 2L) + 7) & ~7L;                 // rows, back-pointer words, the path
}

}  // namespace mp
using namespace mp;

extern "C" {

int64_t mp_lift_fuse_path_scratch_bytes(int V, int64_t Ftot, int K) {
  if (V < 1 || V > FP_MAXV || K < 1 || K > FP_MAXK || Ftot <= 0 || Ftot > (1L << 40)) return 0;
  return fp_scratch_bytes(V, (long)Ftot, K);
}

int mp_lift_fuse_path(const float* hyps, int V, int64_t Ftot, int K, int J, int C, const uint8_t* valid, const int64_t* take_offset, int G,
                      const float* quat, float sigma, float score_weight, float path_sigma, float switch_cost, float* pose, uint8_t* choice, float* cost,
                      float* spread, uint8_t* ok, double* path_cost, void* scratch, int64_t scratch_bytes, void* stream) {
  static_assert(sizeof(long) == sizeof(int64_t), "LP64");
  MP_CHECK(hyps && take_offset && pose && choice && cost && spread && ok && path_cost && scratch, MP_ERR_ARG, "mp_lift_fuse_path: null pointer");
  if (int rc = lift_take_shape("mp_lift_fuse_path", V, (long)Ftot, J, G)) return rc;
  MP_CHECK(K >= 1 && K <= FP_MAXK, MP_ERR_ARG, "mp_lift_fuse_path: K=%d outside 1..%d", K, FP_MAXK);
  MP_CHECK(C == 3 || C == 4, MP_ERR_ARG, "mp_lift_fuse_path: C=%d (3: poses, 4: hypotheses with their score)", C);
  MP_CHECK(sigma > 0.f, MP_ERR_ARG, "mp_lift_fuse_path: sigma=%g must be > 0 (inf: the pair factor is 0)", (double)sigma);
  MP_CHECK(score_weight >= 0.f && __builtin_isfinite(score_weight), MP_ERR_ARG, "mp_lift_fuse_path: score_weight=%g must be finite and >= 0",
           (double)score_weight);
  MP_CHECK(path_sigma > 0.f, MP_ERR_ARG, "mp_lift_fuse_path: path_sigma=%g must be > 0 (inf: the motion factor is 0)", (double)path_sigma);
  MP_CHECK(switch_cost >= 0.f && __builtin_isfinite(switch_cost), MP_ERR_ARG, "mp_lift_fuse_path: switch_cost=%g must be finite and >= 0",
           (double)switch_cost);
  MP_CHECK(Ftot <= (1L << 40), MP_ERR_ARG, "mp_lift_fuse_path: %ld frames: too many for one launch", (long)Ftot);
  MP_CHECK(scratch_bytes >= fp_scratch_bytes(V, (long)Ftot, K), MP_ERR_ARG, "mp_lift_fuse_path: scratch too small (%ld bytes, %ld needed)",
           (long)scratch_bytes, fp_scratch_bytes(V, (long)Ftot, K));
  MP_CHECK(((uintptr_t)scratch & 7) == 0, MP_ERR_ARG, "mp_lift_fuse_path: scratch must be 8-byte aligned");
  const FpShape s = fp_shape(V, K);
  FusePathArgs a = {};
  a.hyps = hyps; a.valid = valid; a.take_offset = (const long*)take_offset; a.quat = quat;
  a.rows = (double*)scratch; a.bp = (unsigned short*)(a.rows + (long)Ftot * s.R); a.path = a.bp + (long)Ftot * s.S;
  a.pose = pose; a.choice = choice; a.cost = cost; a.spread = spread; a.ok = ok; a.path_cost = path_cost; a.Ftot = (long)Ftot;
  a.pair_factor = 1.0 / (2.0 * (double)sigma * (double)sigma);          // (sigma = +inf: exactly 0)
  a.score_weight = (double)score_weight;
  a.path_factor = 1.0 / (2.0 * (double)path_sigma * (double)path_sigma);
  a.switch_cost = (double)switch_cost;
  a.V = V; a.K = K; a.J = J; a.C = C; a.G = G; a.S = s.S; a.NP = s.NP; a.R = s.R;
  // tables: as many frames a tile as fit beside the frame before it (at 4 x 8 x 32 one: 24 KB a rotated frame)
  a.frame_doubles = FP_MAXV * 9 + V * K * J * 3;
  a.TF = (int)std::max(1L, std::min(8L, FP_TILE_LDS / (8L * a.frame_doubles) - 1));
  const size_t tile_lds = (size_t)(a.TF + 1) * a.frame_doubles * 8 + (size_t)(a.TF + 1) * FP_MAXV * sizeof(int);
  const long tiles = ((long)Ftot + a.TF - 1) / a.TF, blocks = ((long)Ftot + 63) / 64;
  MP_CHECK(tiles <= 0x7fffffffL && blocks <= 0x7fffffffL, MP_ERR_ARG, "mp_lift_fuse_path: %ld frames: too many for one launch", (long)Ftot);
  // scan: one state a lane up to 1024 states, four beyond; whole waves
  const int per = s.S <= 1024 ? 1 : 4;
  const int lanes = (((s.S + per - 1) / per + 63) / 64) * 64;
  MP_CHECK(lanes <= 1024 && s.R <= FP_PRE * lanes, MP_ERR_ARG, "mp_lift_fuse_path: V=%d K=%d: %d lanes for rows of %d doubles", V, K, lanes, s.R);
  a.lds_main = (int)std::max((long)(2 * s.S + 2 * s.R) * 8, FP_SCAN_MIN_LDS);
  a.chunk = std::max(1, std::min(FP_CHUNK, a.lds_main / (2 * s.S)));
  const size_t scan_lds = (size_t)a.lds_main + 16 * sizeof(double) + 16 * sizeof(int) + FP_CHUNK * sizeof(unsigned short);
  // (more than 64 KB of LDS only with four states a lane: 77 KB at 4 x 8, the two state vectors are 64 KB)
#define MP_FP_SCAN(ns, k)                                                                                                                            \
  case k:                                                                                                                                            \
    if (scan_lds > 64 * 1024)                                                                                                                        \
      MP_HIP(hipFuncSetAttribute((const void*)lift_fuse_path_scan_kernel<ns, k>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));           \
    hipLaunchKernelGGL((lift_fuse_path_scan_kernel<ns, k>), dim3((unsigned)G), dim3(lanes), scan_lds, (hipStream_t)stream, a);                       \
    break;
  hipLaunchKernelGGL(lift_fuse_path_tables_kernel, dim3((unsigned)tiles), dim3(POSE_THREADS), tile_lds, (hipStream_t)stream, a);
  MP_LAUNCH_CHECK();
  if (per == 1) {
    switch (K) { MP_FP_SCAN(1, 1) MP_FP_SCAN(1, 2) MP_FP_SCAN(1, 3) MP_FP_SCAN(1, 4) MP_FP_SCAN(1, 5) MP_FP_SCAN(1, 6) MP_FP_SCAN(1, 7) MP_FP_SCAN(1, 8) }
  } else {
    switch (K) { MP_FP_SCAN(4, 6) MP_FP_SCAN(4, 7) MP_FP_SCAN(4, 8) }      // (K^V > 1024 needs V = 4 and K >= 6)
  }
#undef MP_FP_SCAN
  MP_LAUNCH_CHECK();
  hipLaunchKernelGGL(lift_fuse_path_emit_kernel, dim3((unsigned)blocks), dim3(64), 0, (hipStream_t)stream, a);
  MP_LAUNCH_CHECK();
  return MP_OK;
}

}  // extern "C"

// Scoring a lift against ground truth, per sequence (include/manipose_hip.h: mp_lift_score has the rule): the sums behind MPJPE, its root mean
// square, velocity and acceleration errors, P-MPJPE, per-joint errors and bone-length statistics of (Ntot, inner, M, C) poses against (Ntot, M, 3)
// targets.  Three kernels on one stream:
//   score:    MP_LIFT_SCORE_SHARES WORKGROUPS PER (sequence, inner), share k on the k-th contiguous slice of the sequence's own clamped range (a
//             whole number of tiles, so a slice's tiling depends on the sequence's length only).  A workgroup walks its slice in tiles of TF frames
//             and stages a tile plus the two frames before it of pred and gt into LDS (consecutive lanes on consecutive floats); one lane per staged
//             frame decides whether the frame is counted; ONE LANE OWNS ONE (frame, joint) and keeps its seven sums in registers over the tiles;
//             one lane per frame adds the frame's joint errors in joint order (frame_err) and counts frames, pairs and triples.  At the end
//             the lanes' sums are added through LDS in a fixed order (frames of the tile, then joints) and the share's partial row goes to scratch.
//   align:    (flag bit 1) one wave64 workgroup per share, on the same slices, in tiles of 64 frames (32 above 17 joints): ONE LANE OWNS ONE
//             POSE and aligns it (Horn's closed form, the pose read from LDS joint by joint, the 4x4 eigenproblem by cyclic Jacobi sweeps in
//             registers); a kernel of its own, so that 64 lanes of a wave align and not the 15 frame lanes of a score tile, and so that the
//             Jacobi's registers are not the score kernel's.  It fills slots 7 and 8 of the partial rows.
//   finalize: one workgroup per (sequence, inner), one lane per slot: the shares added in share order.
// Everything between the float32 loads and the stores is fp64, without contraction into fused multiply-adds.  A sequence's frames are its CLAMPED
// range (lift_seq_frames): whatever the device table holds, no frame outside 0 .. Ntot - 1 is touched.  No atomics, fixed order: identical bits on
// every call, and a sequence's row does not depend on the other sequences of the call.
#include "lift_common.h"

#pragma clang fp contract(off)
#include "lift_geom.h"                    // after the pragma: the shared code takes this file's mode

namespace mp {

constexpr int SCORE_MAXM = LIFT_MAXJ;
constexpr int SCORE_MAXTF = 64;                  // frames of a tile at most (M <= 4); 256 / M otherwise: 15 at M = 17, 8 at M = 32
constexpr int SCORE_SUMS = 7;                    // per (frame, joint) lane: e, e^2, velocity, acceleration, L, L^2, |LG - L|

struct ScoreArgs {
  const float* pred;             // (Ntot, inner, M, C)
  const float* gt;               // (Ntot, M, 3)
  const unsigned char* valid;    // (Ntot, inner) or null
  const long* seq_offset;        // (S + 1) device
  double* rows;                  // (S, inner, R)
  float* frame_err;              // (Ntot, inner) or null
  double* scratch;               // (S, inner, SHARES, R) partial rows
  long Ntot;
  double ps, gs;                 // pred_scale, gt_scale
  unsigned long parent[4];       // parent of joint j: byte j & 7 of word j >> 3 (selected, never indexed: the arguments stay in scalar registers)
  int inner, M, C, S, TF, AF, R, flags, bones;
};

__host__ __device__ static inline int score_tile_frames(int M) { return min(SCORE_MAXTF, POSE_THREADS / M); }
static inline int score_align_frames(int M) { return M > 17 ? 32 : 64; }          // poses of the alignment kernel's tile: 30.8 KiB of LDS at most

// joint j of a staged pose (C floats per joint), scaled, minus its root with rr
__device__ __forceinline__ void score_point(const float* x, int C, int j, double sc, bool rr, double (&p)[3]) {
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    p[c] = sc * (double)x[j * C + c];
    if (rr) p[c] = p[c] - sc * (double)x[c];
  }
}

__device__ __forceinline__ double score_norm3(double x, double y, double z) { return sqrt((x * x + y * y) + z * z); }

// sum_j |a R (y_j - my) + mx - x_j| of the similarity transform that takes the pose y (xp) onto x (xg) best; false: a centred pose is a point
__device__ __forceinline__ bool score_align(const float* xp, const float* xg, int M, int C, double ps, double gs, bool rr, double& err) {
  double mx[3] = {0, 0, 0}, my[3] = {0, 0, 0};
#pragma unroll 1
  for (int j = 0; j < M; ++j) {
    double x[3], y[3];
    score_point(xg, 3, j, gs, rr, x);
    score_point(xp, C, j, ps, rr, y);
#pragma unroll
    for (int c = 0; c < 3; ++c) { mx[c] += x[c]; my[c] += y[c]; }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) { mx[c] = mx[c] / (double)M; my[c] = my[c] / (double)M; }
  double h[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};          // h[r][c] = sum_j y0_j[r] x0_j[c]
  double nx = 0.0, ny = 0.0;
#pragma unroll 1
  for (int j = 0; j < M; ++j) {
    double x[3], y[3];
    score_point(xg, 3, j, gs, rr, x);
    score_point(xp, C, j, ps, rr, y);
#pragma unroll
    for (int c = 0; c < 3; ++c) { x[c] -= mx[c]; y[c] -= my[c]; nx += x[c] * x[c]; ny += y[c] * y[c]; }
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 3; ++c) h[r][c] += y[r] * x[c];
  }
  if (!(nx > 0.0) || !(ny > 0.0)) return false;
  // Horn's N for the rotation taking y0 onto x0 (quaternion w, x, y, z), as in procrustes.hip
  double n[4][4];
  n[0][0] = h[0][0] + h[1][1] + h[2][2];
  n[0][1] = n[1][0] = h[1][2] - h[2][1];
  n[0][2] = n[2][0] = h[2][0] - h[0][2];
  n[0][3] = n[3][0] = h[0][1] - h[1][0];
  n[1][1] = h[0][0] - h[1][1] - h[2][2];
  n[1][2] = n[2][1] = h[0][1] + h[1][0];
  n[1][3] = n[3][1] = h[2][0] + h[0][2];
  n[2][2] = -h[0][0] + h[1][1] - h[2][2];
  n[2][3] = n[3][2] = h[1][2] + h[2][1];
  n[3][3] = -h[0][0] - h[1][1] + h[2][2];
  double q[4], lam, lam2;                        // (the second eigenvalue is not used here)
  lift_eig4(n, q, lam, lam2);
  const double qn = 1.0 / sqrt((q[0] * q[0] + q[1] * q[1]) + (q[2] * q[2] + q[3] * q[3]));
  const double w = q[0] * qn, qx = q[1] * qn, qy = q[2] * qn, qz = q[3] * qn;
  double R[3][3];                               // x0 ~ a R y0
  R[0][0] = 1 - 2 * (qy * qy + qz * qz); R[0][1] = 2 * (qx * qy - w * qz);     R[0][2] = 2 * (qx * qz + w * qy);
  R[1][0] = 2 * (qx * qy + w * qz);     R[1][1] = 1 - 2 * (qx * qx + qz * qz); R[1][2] = 2 * (qy * qz - w * qx);
  R[2][0] = 2 * (qx * qz - w * qy);     R[2][1] = 2 * (qy * qz + w * qx);     R[2][2] = 1 - 2 * (qx * qx + qy * qy);
  const double sc = lam / ny;                   // trace(S) normX / normY of the reference's normalised form
  double sum = 0.0;
#pragma unroll 1
  for (int j = 0; j < M; ++j) {
    double x[3], y[3], d[3];
    score_point(xg, 3, j, gs, rr, x);
    score_point(xp, C, j, ps, rr, y);
#pragma unroll
    for (int c = 0; c < 3; ++c) y[c] -= my[c];
#pragma unroll
    for (int r = 0; r < 3; ++r) d[r] = (sc * ((R[r][0] * y[0] + R[r][1] * y[1]) + R[r][2] * y[2]) + mx[r]) - x[r];
    sum += score_norm3(d[0], d[1], d[2]);
  }
  err = sum;
  return true;
}

__global__ __launch_bounds__(POSE_THREADS) void lift_score_kernel(ScoreArgs A) {
  extern __shared__ __attribute__((aligned(16))) unsigned char score_lds[];
  const int M = A.M, C = A.C, TF = A.TF, WP = M * C, WG = M * 3;
  double* dbuf = (double*)score_lds;                                   // [TF M]: a value per (frame, joint) lane
  double* col = dbuf + TF * M;                                         // [SCORE_SUMS][M]: the lanes' sums added over the frames of the tile
  double* fr = col + SCORE_SUMS * M;                                   // [3][TF]: the frame lanes' counts
  float* xp = (float*)(fr + 3 * TF);                                   // [TF + 2][WP]: row h is frame tile0 - 2 + h
  float* xg = xp + (TF + 2) * WP;                                      // [TF + 2][WG]
  int* flag = (int*)(xg + (TF + 2) * WG);                              // [TF + 2]: the staged frame is in the sequence and counted
  const int tid = threadIdx.x;
  const int k = (int)(blockIdx.x % MP_LIFT_SCORE_SHARES);
  const long si = blockIdx.x / MP_LIFT_SCORE_SHARES;
  const int i = (int)(si % A.inner), s = (int)(si / A.inner);
  const bool rr = (A.flags & 1) != 0;
  const FrameRange r = lift_seq_frames(A.seq_offset, s, A.Ntot);
  const long n = r.f1 - r.f0;
  const long per = ((n + MP_LIFT_SCORE_SHARES - 1) / MP_LIFT_SCORE_SHARES + TF - 1) / TF * TF;     // frames of a share: whole tiles
  const long a0 = min(r.f0 + k * per, r.f1), a1 = min(a0 + per, r.f1);

  const int t = tid / M, j = tid - t * M;
  const bool act = t < TF;
  int pj = -1;                                                         // the joint's parent; -1: no bone
  if (A.bones && j >= 1) {
    const int wsel = j >> 3;
    const unsigned long w = wsel == 0 ? A.parent[0] : wsel == 1 ? A.parent[1] : wsel == 2 ? A.parent[2] : A.parent[3];
    pj = (int)((w >> ((j & 7) * 8)) & 0xff);
  }
  double acc[SCORE_SUMS] = {0, 0, 0, 0, 0, 0, 0};
  double cnt0 = 0.0, cnt3 = 0.0, cnt5 = 0.0;                           // of the frame lanes (tid < TF)

  for (long tile0 = a0; tile0 < a1; tile0 += TF) {
    for (int idx = tid; idx < (TF + 2) * WP; idx += POSE_THREADS) {
      const int h = idx / WP;
      const long g = tile0 - 2 + h;
      if (g >= r.f0 && g < a1) xp[idx] = A.pred[(g * A.inner + i) * WP + (idx - h * WP)];
    }
    for (int idx = tid; idx < (TF + 2) * WG; idx += POSE_THREADS) {
      const int h = idx / WG;
      const long g = tile0 - 2 + h;
      if (g >= r.f0 && g < a1) xg[idx] = A.gt[g * WG + (idx - h * WG)];
    }
    __syncthreads();
    if (tid < TF + 2) {
      const long g = tile0 - 2 + tid;
      bool ok = g >= r.f0 && g < a1 && (A.valid == nullptr || A.valid[g * A.inner + i] != 0);
      if (ok) {
#pragma unroll 1
        for (int jj = 0; jj < M; ++jj) {
          double p[3], q[3];
          score_point(xp + tid * WP, C, jj, A.ps, rr, p);
          score_point(xg + tid * WG, 3, jj, A.gs, rr, q);
          ok = ok && __builtin_isfinite((p[0] + p[1]) + p[2]) && __builtin_isfinite((q[0] + q[1]) + q[2]);
        }
      }
      flag[tid] = ok ? 1 : 0;
    }
    __syncthreads();
    double e = 0.0;
    if (act && flag[t + 2]) {
      const float* p2 = xp + (t + 2) * WP;
      const float* g2 = xg + (t + 2) * WG;
      double P[3], G[3];
      score_point(p2, C, j, A.ps, rr, P);
      score_point(g2, 3, j, A.gs, rr, G);
      e = score_norm3(P[0] - G[0], P[1] - G[1], P[2] - G[2]);
      acc[0] += e;
      acc[1] += e * e;
      if (flag[t + 1]) {
        double P1[3], G1[3];
        score_point(p2 - WP, C, j, A.ps, rr, P1);
        score_point(g2 - WG, 3, j, A.gs, rr, G1);
        acc[2] += score_norm3((P[0] - P1[0]) - (G[0] - G1[0]), (P[1] - P1[1]) - (G[1] - G1[1]), (P[2] - P1[2]) - (G[2] - G1[2]));
        if (flag[t]) {
          double P0[3], G0[3], d[3];
          score_point(p2 - 2 * WP, C, j, A.ps, rr, P0);
          score_point(g2 - 2 * WG, 3, j, A.gs, rr, G0);
#pragma unroll
          for (int c = 0; c < 3; ++c) d[c] = ((P[c] - 2.0 * P1[c]) + P0[c]) - ((G[c] - 2.0 * G1[c]) + G0[c]);
          acc[3] += score_norm3(d[0], d[1], d[2]);
        }
      }
      if (pj >= 0) {
        double Pp[3], Gp[3];
        score_point(p2, C, pj, A.ps, rr, Pp);
        score_point(g2, 3, pj, A.gs, rr, Gp);
        const double L = score_norm3(P[0] - Pp[0], P[1] - Pp[1], P[2] - Pp[2]);
        const double LG = score_norm3(G[0] - Gp[0], G[1] - Gp[1], G[2] - Gp[2]);
        acc[4] += L;
        acc[5] += L * L;
        acc[6] += fabs(LG - L);
      }
    }
    if (act) dbuf[tid] = e;
    __syncthreads();
    if (tid < TF && tile0 + tid < a1) {
      const long g = tile0 + tid;
      float fe = -1.f;
      if (flag[tid + 2]) {
        double sum = 0.0;
        for (int jj = 0; jj < M; ++jj) sum += dbuf[tid * M + jj];
        fe = (float)(sum / (double)M);
        cnt0 += 1.0;
        if (flag[tid + 1]) {
          cnt3 += 1.0;
          if (flag[tid]) cnt5 += 1.0;
        }
      }
      if (A.frame_err != nullptr) A.frame_err[g * A.inner + i] = fe;
    }
    __syncthreads();
  }

  // the share's partial row: the lanes' sums over the frames of the tile (t in order), then over the joints (j in order)
#pragma unroll
  for (int q = 0; q < SCORE_SUMS; ++q) {
    if (act) dbuf[tid] = acc[q];
    __syncthreads();
    if (tid < M) {
      double sum = 0.0;
      for (int tt = 0; tt < TF; ++tt) sum += dbuf[tt * M + tid];
      col[q * M + tid] = sum;
    }
    __syncthreads();
  }
  if (tid < TF) {
    fr[tid] = cnt0; fr[TF + tid] = cnt3; fr[2 * TF + tid] = cnt5;
  }
  __syncthreads();
  double* prow = A.scratch + (long)blockIdx.x * A.R;
  if (tid < M) {
    prow[9 + tid] = col[tid];
    if (tid >= 1) {
#pragma unroll
      for (int c = 0; c < 3; ++c) prow[9 + M + 3 * (tid - 1) + c] = col[(4 + c) * M + tid];
    }
  }
  if (tid >= 64 && tid < 64 + 9) {                                     // (another wave than the one that stores the joints' slots)
    const int slot = tid - 64;
    const bool frame = slot == 0 || slot == 3 || slot == 5;
    const double* src = frame ? fr + (slot == 0 ? 0 : slot == 3 ? 1 : 2) * TF
                              : col + (slot == 1 ? 0 : slot == 2 ? 1 : slot == 4 ? 2 : 3) * M;
    const int cnt = slot >= 7 ? 0 : frame ? TF : M;                    // (slots 7 and 8 are the alignment kernel's: zero without it)
    double sum = 0.0;
    for (int u = 0; u < cnt; ++u) sum += src[u];
    prow[slot] = sum;
  }
}

// Slots 7 and 8 of the partial rows (flag bit 1): ONE WAVE64 WORKGROUP per share, on the slice the score kernel gives that share, in tiles of AF
// frames; ONE LANE OWNS ONE POSE, decides whether its frame is counted and aligns it, reading the pose from LDS joint by joint.  The lanes' sums
// are added in lane order.  Runs after the score kernel on the same stream and overwrites the zeros that one left in the two slots.
__global__ __launch_bounds__(64) void lift_score_align_kernel(ScoreArgs A) {
  extern __shared__ __attribute__((aligned(16))) unsigned char score_lds[];
  const int M = A.M, C = A.C, TF = A.TF, AF = A.AF, WP = M * C, WG = M * 3;
  double* red = (double*)score_lds;                                    // [2][64]
  float* xp = (float*)(red + 128);                                     // [AF][WP]
  float* xg = xp + AF * WP;                                            // [AF][WG]
  const int lane = threadIdx.x;
  const int k = (int)(blockIdx.x % MP_LIFT_SCORE_SHARES);
  const long si = blockIdx.x / MP_LIFT_SCORE_SHARES;
  const int i = (int)(si % A.inner), s = (int)(si / A.inner);
  const bool rr = (A.flags & 1) != 0;
  const FrameRange r = lift_seq_frames(A.seq_offset, s, A.Ntot);
  const long n = r.f1 - r.f0;
  const long per = ((n + MP_LIFT_SCORE_SHARES - 1) / MP_LIFT_SCORE_SHARES + TF - 1) / TF * TF;     // (the score kernel's slices)
  const long a0 = min(r.f0 + k * per, r.f1), a1 = min(a0 + per, r.f1);
  double sum7 = 0.0, cnt8 = 0.0;
  for (long tile0 = a0; tile0 < a1; tile0 += AF) {
    const int nf = (int)min((long)AF, a1 - tile0);
    for (int idx = lane; idx < nf * WP; idx += 64) {
      const int h = idx / WP;
      xp[idx] = A.pred[((tile0 + h) * A.inner + i) * WP + (idx - h * WP)];
    }
    for (int idx = lane; idx < nf * WG; idx += 64) xg[idx] = A.gt[tile0 * WG + idx];
    __syncthreads();
    if (lane < nf) {
      const long g = tile0 + lane;
      bool ok = A.valid == nullptr || A.valid[g * A.inner + i] != 0;
      if (ok) {
#pragma unroll 1
        for (int jj = 0; jj < M; ++jj) {
          double p[3], q[3];
          score_point(xp + lane * WP, C, jj, A.ps, rr, p);
          score_point(xg + lane * WG, 3, jj, A.gs, rr, q);
          ok = ok && __builtin_isfinite((p[0] + p[1]) + p[2]) && __builtin_isfinite((q[0] + q[1]) + q[2]);
        }
      }
      if (ok) {
        double err = 0.0;
        if (score_align(xp + lane * WP, xg + lane * WG, M, C, A.ps, A.gs, rr, err)) sum7 += err;
        else cnt8 += 1.0;
      }
    }
    __syncthreads();
  }
  red[lane] = sum7;
  red[64 + lane] = cnt8;
  __syncthreads();
  if (lane < 2) {
    double sum = 0.0;
    for (int u = 0; u < 64; ++u) sum += red[lane * 64 + u];
    A.scratch[(long)blockIdx.x * A.R + 7 + lane] = sum;
  }
}

__global__ __launch_bounds__(POSE_THREADS) void lift_score_finalize_kernel(ScoreArgs A) {
  const int slot = threadIdx.x;
  if (slot >= A.R) return;
  const double* p = A.scratch + (long)blockIdx.x * MP_LIFT_SCORE_SHARES * A.R + slot;
  double sum = 0.0;
  for (int k = 0; k < MP_LIFT_SCORE_SHARES; ++k) sum += p[(long)k * A.R];
  A.rows[(long)blockIdx.x * A.R + slot] = sum;
}

static size_t score_lds_bytes(int M, int C, int TF) {
  return sizeof(double) * ((size_t)TF * M + SCORE_SUMS * M + 3 * TF) + sizeof(float) * (size_t)(TF + 2) * M * (C + 3) + sizeof(int) * (TF + 2);
}

}  // namespace mp
using namespace mp;

extern "C" {

int mp_lift_score_row_doubles(int M) { return M >= 1 && M <= SCORE_MAXM ? 9 + M + 3 * (M - 1) : 0; }

int64_t mp_lift_score_scratch_doubles(int S, int inner, int M) {
  if (S <= 0 || inner <= 0 || M < 1 || M > SCORE_MAXM) return 0;
  return (int64_t)S * inner * MP_LIFT_SCORE_SHARES * mp_lift_score_row_doubles(M);
}

int mp_lift_score(const float* pred, int64_t Ntot, int inner, int M, int C, const float* gt, const uint8_t* valid, const int64_t* seq_offset, int S,
                  const int32_t* parents, double pred_scale, double gt_scale, int flags, double* rows, float* frame_err, double* scratch,
                  int64_t scratch_doubles, void* stream) {
  static_assert(sizeof(long) == sizeof(int64_t), "LP64");
  static_assert(POSE_THREADS >= 64 + 9 && POSE_THREADS >= SCORE_MAXTF + 2 && POSE_THREADS >= 6 + 4 * SCORE_MAXM, "lane roles of lift_score_kernel");
  MP_CHECK(pred && gt && seq_offset && rows && scratch, MP_ERR_ARG, "mp_lift_score: null pointer");
  MP_CHECK(C == 3 || C == 4, MP_ERR_ARG, "mp_lift_score: C=%d (3: poses, 4: hypotheses with their score)", C);
  MP_CHECK(M >= 1 && M <= SCORE_MAXM, MP_ERR_ARG, "mp_lift_score: M=%d outside 1..%d", M, SCORE_MAXM);
  MP_CHECK(flags >= 0 && flags <= 3, MP_ERR_ARG, "mp_lift_score: flags=%d outside 0..3 (bit 0 root-relative, bit 1 Procrustes)", flags);
  MP_CHECK(!(flags & 2) || M >= 3, MP_ERR_ARG, "mp_lift_score: Procrustes alignment needs M >= 3 joints, got M=%d", M);
  MP_CHECK(Ntot > 0 && inner > 0 && S > 0 && (long)S <= Ntot, MP_ERR_ARG, "mp_lift_score: Ntot=%ld inner=%d S=%d out of range", (long)Ntot, inner, S);
  MP_CHECK(Ntot <= (1L << 40) / ((long)inner * M * 4), MP_ERR_ARG, "mp_lift_score: %ld frames of %d poses: too many for one launch", (long)Ntot, inner);
  MP_CHECK((long)S * inner <= 0x7fffffffL / MP_LIFT_SCORE_SHARES, MP_ERR_ARG, "mp_lift_score: S=%d inner=%d: too many for one launch", S, inner);
  MP_CHECK(pred_scale > 0.0 && pred_scale <= 1.7976931348623157e308 && gt_scale > 0.0 && gt_scale <= 1.7976931348623157e308, MP_ERR_ARG,
           "mp_lift_score: scale pred=%g gt=%g must be finite and > 0", pred_scale, gt_scale);
  ScoreArgs A = {};
  if (parents != nullptr) {
    MP_CHECK(parents[0] == -1, MP_ERR_ARG, "mp_lift_score: parents[0] = %d: joint 0 must be the root (-1)", parents[0]);
    for (int j = 1; j < M; ++j) {
      MP_CHECK(parents[j] >= 0 && parents[j] < j, MP_ERR_ARG, "mp_lift_score: parents[%d] = %d: parents precede their children", j, parents[j]);
      A.parent[j >> 3] |= (unsigned long)parents[j] << ((j & 7) * 8);
    }
    A.bones = 1;
  }
  MP_CHECK(scratch_doubles >= mp_lift_score_scratch_doubles(S, inner, M), MP_ERR_ARG, "mp_lift_score: scratch too small (%ld doubles, %ld needed)",
           (long)scratch_doubles, (long)mp_lift_score_scratch_doubles(S, inner, M));
  MP_CHECK(((uintptr_t)scratch & 7) == 0 && ((uintptr_t)rows & 7) == 0, MP_ERR_ARG, "mp_lift_score: rows and scratch must be 8-byte aligned");
  A.pred = pred; A.gt = gt; A.valid = valid; A.seq_offset = (const long*)seq_offset; A.rows = rows; A.frame_err = frame_err; A.scratch = scratch;
  A.Ntot = Ntot; A.ps = pred_scale; A.gs = gt_scale;
  A.inner = inner; A.M = M; A.C = C; A.S = S; A.TF = score_tile_frames(M); A.AF = score_align_frames(M); A.R = mp_lift_score_row_doubles(M); A.flags = flags;
  const unsigned groups = (unsigned)((long)S * inner);
  const size_t lds = score_lds_bytes(M, C, A.TF);                                  // 12.7 KiB at most (M = 32, C = 4)
  hipLaunchKernelGGL(lift_score_kernel, dim3(groups * MP_LIFT_SCORE_SHARES), dim3(POSE_THREADS), lds, (hipStream_t)stream, A);
  MP_LAUNCH_CHECK();
  if (flags & 2) {
    const size_t alds = 128 * sizeof(double) + sizeof(float) * (size_t)A.AF * M * (C + 3);       // 30.8 KiB at most (M = 17, C = 4)
    hipLaunchKernelGGL(lift_score_align_kernel, dim3(groups * MP_LIFT_SCORE_SHARES), dim3(64), alds, (hipStream_t)stream, A);
    MP_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(lift_score_finalize_kernel, dim3(groups), dim3(POSE_THREADS), 0, (hipStream_t)stream, A);
  MP_LAUNCH_CHECK();
  return MP_OK;
}

}  // extern "C"

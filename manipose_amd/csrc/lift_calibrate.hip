// Calibrating a take on its keypoints (include/manipose_hip.h: mp_lift_calibrate_views has the rule).  mp_lift_bundle_views refines the cameras'
// extrinsics and takes the fused pose as given structure; the intrinsics are read from a calibration file.  This is the full bundle adjustment:
// every joint of every used frame is a free 3-D point, every free camera has its six pose parameters, every view one focal factor, all fitted to
// the keypoints, the start entering as a weak prior on the points (which pins the scale).  The points are eliminated one by one by a Schur
// complement: per point a 3x3 inverse and its coupling to at most 22 camera parameters, per take one reduced system, summed in a fixed order.
// tests/lift_calibrate_ref.py states the rule in float64.
//
// FIVE KERNELS, launched in a fixed sequence on one stream (lift_bundle.hip's scheme), no grid-wide barrier and no synchronisation:
//   cal_mask_kernel     one lane per frame: which views observe the frame, start copied into points and (as doubles) into the scratch, the row zeroed
//   cal_init_kernel     one workgroup per take: used[g][v], the gauge, the camera and focal slots, the column tables, the take's state
//   cal_frame_kernel    one lane per frame, pass p = 0 .. iters: at its head the frame's points take the candidate of pass p - 1 and form their own,
//                       X - U^-1 (b + W dc); then the lane goes JOINT BY JOINT: all views of the joint evaluated at the candidate, the point's U, b
//                       and its W (3 x N), a and Jacobian rows by COLUMN of the reduced system in LDS (indexed at run time: a view's slot decides
//                       the column), U^-1 by cofactors, U^-1 b and U^-1 W kept in the scratch for the next head, and the point's term of S
//                       (lower triangle, packed by rows) and of s added to the frame's row - joints in order
//   cal_take_kernel     one workgroup per take, pass p: lane e sums entry e of the take's rows in frame order; lane 0 decides on the candidate,
//                       writes the take's outputs, factorises S in LDS and forms the next candidate cameras and focal factors
//   cal_final_kernel    one lane per frame: the points that stand
// The LDS of the frame kernel is lane-private ([item][lane]: no bank conflicts, no barrier): 148 doubles per lane, 74 KiB per workgroup.  The
// frame's row and the frame-private scratch are laid out item-major (item * Ftot + f: consecutive lanes touch consecutive doubles) - the row is
// read and written 275 times per joint; CAL_ROW_FRAME_MAJOR builds the other layout (lift_bundle.hip's), kept for the measurement in DESIGN.md.
// Everything between the float32 loads and the float32 stores is fp64, without contraction; no atomics, fixed orders: identical bits on every call.
#include "lift_common.h"

#pragma clang fp contract(off)
#include "lift_geom.h"                    // after the pragma: the shared code takes this file's mode

namespace mp {

constexpr int CAL_MAXV = MP_LIFT_FUSE_MAXV;
constexpr int CAL_N = 6 * (CAL_MAXV - 1) + CAL_MAXV;    // unknowns of the reduced system at most: three free cameras, four focal factors
constexpr int CAL_THREADS = 64;                         // lanes of a workgroup of the per-frame kernels
constexpr int CAL_TAKE_THREADS = 256;
// a frame's row: [0, 253) S, [253, 275) s, F, the joints not in front of their camera, E_v (4), W_v (4), the U that failed its test
constexpr int CROW_S = 0, CROW_G = CAL_N * (CAL_N + 1) / 2, CROW_F = CROW_G + CAL_N, CROW_DEEP = CROW_F + 1, CROW_E = CROW_DEEP + 1,
              CROW_W = CROW_E + CAL_MAXV, CROW_U = CROW_W + CAL_MAXV, CAL_ROW = CROW_U + 1;
static_assert(CAL_N == 22 && CAL_ROW == 286, "the row");
// a frame's private items: the mask, then per joint: the point that stands (3), the candidate (3), U^-1 b (3), U^-1 W (3 x CAL_N, column-major)
constexpr int CPRIV_MASK = 0, CPRIV_JOINT = 1, CPJ_CUR = 0, CPJ_CAND = 3, CPJ_YB = 6, CPJ_Y = 9, CAL_PJ = CPJ_Y + 3 * CAL_N;
// a take's state
constexpr int CTS_STOP = 0, CTS_STEPS = 1, CTS_USE_CAND = 2, CTS_N = 3, CTS_ITERATE = 4, CTS_F = 5, CTS_NFREE = 6, CTS_SLOT = 8, CTS_VIEW = 12,
              CTS_FSLOT = 16, CTS_CAM = 20, CTS_COLV = 52, CTS_DC = 74, CAL_TS = 96;
static_assert(CTS_CAM + 8 * CAL_MAXV <= CTS_COLV && CTS_COLV + CAL_N <= CTS_DC && CTS_DC + CAL_N <= CAL_TS, "the take's state");
constexpr double CAL_PIVOT = 1e-12, CAL_SLACK = 1e-6, CAL_SMALL = 1e-16;

#ifdef CAL_ROW_FRAME_MAJOR
#define CAL_ROW_AT(A, f, e) (A).rows[(f) * CAL_ROW + (e)]
#else
#define CAL_ROW_AT(A, f, e) (A).rows[(long)(e) * (A).Ftot + (f)]
#endif

struct CalArgs {
  const float* start;            // (Ftot, J, 3)
  const unsigned char* start_ok; // (Ftot) or null
  const float* kp;               // (V, Ftot, J, 2)
  const unsigned char* valid;    // (V, Ftot) or null
  const long* take_offset;       // (G + 1) device
  const float* quat;             // (G, V, 4)
  const float* trans;            // (G, V, 3)
  const float* intr;             // (G, V, 9)
  const unsigned char* fixed;    // (G, V) or null
  const float* weights;          // (J) or null
  float* quat_out;               // (G, V, 4)
  float* trans_out;              // (G, V, 3)
  float* intr_out;               // (G, V, 9)
  float* points;                 // (Ftot, J, 3)
  float* reproj;                 // (G, V, 2)
  double* cost;                  // (G, 2)
  unsigned char* steps;          // (G)
  unsigned char* ok;             // (G)
  int* used;                     // (G, V)
  double* rows;                  // CAL_ROW x Ftot
  double* priv;                  // (1 + J CAL_PJ) x Ftot
  double* state;                 // (G, CAL_TS)
  long Ftot;
  double sigma2, prior;
  int V, J, G, distort, focal, iters;
};

// 1. of the rule: the views that observe frame f, start into points and into the scratch, the frame's row zeroed
__global__ __launch_bounds__(CAL_THREADS) void cal_mask_kernel(CalArgs A) {
  const long f = (long)blockIdx.x * CAL_THREADS + threadIdx.x;
  if (f >= A.Ftot) return;
  const long Ftot = A.Ftot;
  const int V = A.V, J = A.J;
  const int g = lift_seq_of(A.take_offset, A.G, f);
  const FrameRange fr = lift_seq_frames(A.take_offset, g, Ftot);
  const float* X = A.start + f * J * 3;
  double* pv = A.priv + f;
  bool good = f >= fr.f0 && f < fr.f1 && (A.start_ok == nullptr || A.start_ok[f] != 0);
#pragma unroll 1
  for (int j = 0; j < J; ++j) {
    const float x0 = X[j * 3], x1 = X[j * 3 + 1], x2 = X[j * 3 + 2];
    good = good && __builtin_isfinite(((double)x0 + (double)x1) + (double)x2);
    float* out = A.points + (f * J + j) * 3;
    out[0] = x0; out[1] = x1; out[2] = x2;
    double* pj = pv + (long)(CPRIV_JOINT + j * CAL_PJ) * Ftot;
    pj[(long)(CPJ_CUR + 0) * Ftot] = x0; pj[(long)(CPJ_CUR + 1) * Ftot] = x1; pj[(long)(CPJ_CUR + 2) * Ftot] = x2;
    pj[(long)(CPJ_CAND + 0) * Ftot] = x0; pj[(long)(CPJ_CAND + 1) * Ftot] = x1; pj[(long)(CPJ_CAND + 2) * Ftot] = x2;
  }
  int mask = 0;
  if (good) {
#pragma unroll 1
    for (int v = 0; v < V; ++v) {
      if (A.valid != nullptr && A.valid[(long)v * Ftot + f] == 0) continue;
      if (!lift_quat_ok(A.quat + ((long)g * V + v) * 4)) continue;
      const float* U = A.kp + ((long)v * Ftot + f) * J * 2;
      bool fin = true;
#pragma unroll 1
      for (int j = 0; j < J; ++j)
        if (A.weights == nullptr || A.weights[j] != 0.f) fin = fin && __builtin_isfinite((double)U[2 * j] + (double)U[2 * j + 1]);
      if (fin) mask |= 1 << v;
    }
  }
  pv[(long)CPRIV_MASK * Ftot] = (double)mask;
#pragma unroll 1
  for (int e = 0; e < CAL_ROW; ++e) CAL_ROW_AT(A, f, e) = 0.0;
}

// 2. of the rule: the used frames of every view, the gauge, the slots, the take's state
__global__ __launch_bounds__(CAL_TAKE_THREADS) void cal_init_kernel(CalArgs A) {
  __shared__ int counts[CAL_TAKE_THREADS / 64][CAL_MAXV];
  const int g = blockIdx.x, V = A.V;
  const FrameRange fr = lift_seq_frames(A.take_offset, g, A.Ftot);
  int c0 = 0, c1 = 0, c2 = 0, c3 = 0;
#pragma unroll 1
  for (long f = fr.f0 + threadIdx.x; f < fr.f1; f += CAL_TAKE_THREADS) {
    const int mask = (int)A.priv[(long)CPRIV_MASK * A.Ftot + f];
    c0 += mask & 1; c1 += (mask >> 1) & 1; c2 += (mask >> 2) & 1; c3 += (mask >> 3) & 1;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {                             // (integers: exact in any order)
    c0 += __shfl_xor(c0, off); c1 += __shfl_xor(c1, off); c2 += __shfl_xor(c2, off); c3 += __shfl_xor(c3, off);
  }
  if ((threadIdx.x & 63) == 0) {
    int* c = counts[threadIdx.x >> 6];
    c[0] = c0; c[1] = c1; c[2] = c2; c[3] = c3;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  double* ts = A.state + (long)g * CAL_TS;
  int lowest = -1, n = 0, seen = 0;
  bool anchored = false;
  for (int v = 0; v < V; ++v) {
    const int u = (counts[0][v] + counts[1][v]) + (counts[2][v] + counts[3][v]);
    A.used[(long)g * V + v] = u;
    if (u > 0 && lowest < 0) lowest = v;
    if (u > 0) ++seen;
  }
  for (int v = 0; v < CAL_MAXV; ++v) { ts[CTS_SLOT + v] = -1.0; ts[CTS_VIEW + v] = -1.0; ts[CTS_FSLOT + v] = -1.0; }
  for (int v = 0; v < V; ++v) {
    const int u = A.used[(long)g * V + v];
    const bool fix = A.fixed != nullptr ? A.fixed[(long)g * V + v] != 0 : v == lowest;
    if (fix) anchored = anchored || u > 0;
    else if (u > 0) { ts[CTS_SLOT + v] = (double)n; ts[CTS_VIEW + n] = (double)v; ++n; }
  }
  if (!(anchored && n > 0)) {                                          // mp_lift_bundle_views' gauge: no camera moves
    n = 0;
    for (int v = 0; v < CAL_MAXV; ++v) { ts[CTS_SLOT + v] = -1.0; ts[CTS_VIEW + v] = -1.0; }
  }
  int N = 6 * n;
  for (int i = 0; i < CAL_N; ++i) { ts[CTS_COLV + i] = -1.0; ts[CTS_DC + i] = 0.0; }
  for (int k = 0; k < n; ++k)
    for (int i = 0; i < 6; ++i) ts[CTS_COLV + 6 * k + i] = ts[CTS_VIEW + k];
  if (A.focal)
    for (int v = 0; v < V; ++v)
      if (A.used[(long)g * V + v] > 0) { ts[CTS_FSLOT + v] = (double)N; ts[CTS_COLV + N] = (double)v; ++N; }
  ts[CTS_STOP] = 0.0; ts[CTS_STEPS] = 0.0; ts[CTS_USE_CAND] = 0.0; ts[CTS_N] = (double)N; ts[CTS_ITERATE] = (N > 0 && seen >= 2) ? 1.0 : 0.0;
  ts[CTS_F] = 0.0; ts[CTS_NFREE] = (double)n; ts[7] = 0.0;
  for (int v = 0; v < CAL_MAXV; ++v) {
    double* cam = ts + CTS_CAM + 8 * v;
    cam[0] = 1.0; cam[1] = 0.0; cam[2] = 0.0; cam[3] = 0.0; cam[4] = 0.0; cam[5] = 0.0; cam[6] = 0.0; cam[7] = 1.0;
    double n2;
    if (v < V && lift_quat_ok(A.quat + ((long)g * V + v) * 4, n2)) {
      const float* q = A.quat + ((long)g * V + v) * 4;
      const float* T = A.trans + ((long)g * V + v) * 3;
      const double nn = sqrt(n2);
      cam[0] = (double)q[0] / nn; cam[1] = (double)q[1] / nn; cam[2] = (double)q[2] / nn; cam[3] = (double)q[3] / nn;
      cam[4] = T[0]; cam[5] = T[1]; cam[6] = T[2];
    }
  }
}

// pass p of a frame: its candidate points, the evaluation of every view at the candidate, its row of the reduced system
__global__ __launch_bounds__(CAL_THREADS) void cal_frame_kernel(CalArgs A, int p) {
  __shared__ double sW[3 * CAL_N][CAL_THREADS];                        // the point's W by column: rows x, y, z
  __shared__ double sJ0[CAL_N][CAL_THREADS], sJ1[CAL_N][CAL_THREADS];  // the two rows of the Jacobian with respect to a column's parameter
  __shared__ double sA[CAL_N][CAL_THREADS];                            // a by column
  __shared__ double sT[CAL_MAXV][CAL_THREADS];                         // w_j omega of a view's observation of the point
  __shared__ double sE[CAL_MAXV][CAL_THREADS], sS[CAL_MAXV][CAL_THREADS], sF[CAL_MAXV][CAL_THREADS];   // a view's E, W and F of the frame
  const int t = threadIdx.x;
  const long f = (long)blockIdx.x * CAL_THREADS + t;
  if (f >= A.Ftot) return;
  const long Ftot = A.Ftot;
  const int V = A.V, J = A.J;
  const int g = lift_seq_of(A.take_offset, A.G, f);
  const double* ts = A.state + (long)g * CAL_TS;
  if (ts[CTS_STOP] != 0.0) return;
  double* pv = A.priv + f;                                              // item i of this frame: pv[i * Ftot]
  const int mask = (int)pv[(long)CPRIV_MASK * Ftot];
  if (mask == 0) return;
  const int N = (int)ts[CTS_N];
  const bool jac = p < A.iters && ts[CTS_ITERATE] != 0.0;
  if (p > 0) {
    // the take still runs: the candidate of pass p - 1 was taken.  The next: X - (U^-1 b + sum_c (U^-1 W)_c dc_c), columns in order
#pragma unroll 1
    for (int j = 0; j < J; ++j) {
      if (A.weights != nullptr && A.weights[j] == 0.f) continue;
      double* pj = pv + (long)(CPRIV_JOINT + j * CAL_PJ) * Ftot;
      double x = pj[(long)(CPJ_CAND + 0) * Ftot], y = pj[(long)(CPJ_CAND + 1) * Ftot], z = pj[(long)(CPJ_CAND + 2) * Ftot];
      pj[(long)(CPJ_CUR + 0) * Ftot] = x; pj[(long)(CPJ_CUR + 1) * Ftot] = y; pj[(long)(CPJ_CUR + 2) * Ftot] = z;
      double dx = pj[(long)(CPJ_YB + 0) * Ftot], dy = pj[(long)(CPJ_YB + 1) * Ftot], dz = pj[(long)(CPJ_YB + 2) * Ftot];
#pragma unroll 1
      for (int c = 0; c < N; ++c) {
        const double* Y = pj + (long)(CPJ_Y + 3 * c) * Ftot;
        const double d = ts[CTS_DC + c];
        dx += Y[0] * d; dy += Y[Ftot] * d; dz += Y[2 * Ftot] * d;
      }
      x = x - dx; y = y - dy; z = z - dz;
      pj[(long)(CPJ_CAND + 0) * Ftot] = x; pj[(long)(CPJ_CAND + 1) * Ftot] = y; pj[(long)(CPJ_CAND + 2) * Ftot] = z;
    }
  }
  if (jac) {
#pragma unroll 1
    for (int e = CROW_S; e < CROW_F; ++e) CAL_ROW_AT(A, f, e) = 0.0;
  }
#pragma unroll
  for (int v = 0; v < CAL_MAXV; ++v) { sE[v][t] = 0.0; sS[v][t] = 0.0; sF[v][t] = 0.0; }
  const float* S0 = A.start + f * J * 3;
  double Pf = 0.0, notdeep = 0.0, ufail = 0.0;
#pragma unroll 1
  for (int j = 0; j < J; ++j) {                                         // the frame's points one by one
    const double w = A.weights != nullptr ? (double)A.weights[j] : 1.0;
    if (w == 0.0) continue;
    double* pj = pv + (long)(CPRIV_JOINT + j * CAL_PJ) * Ftot;
    const double x = pj[(long)(CPJ_CAND + 0) * Ftot], y = pj[(long)(CPJ_CAND + 1) * Ftot], z = pj[(long)(CPJ_CAND + 2) * Ftot];
    const double ex = x - (double)S0[j * 3], ey = y - (double)S0[j * 3 + 1], ez = z - (double)S0[j * 3 + 2];
    Pf += w * ((ex * ex + ey * ey) + ez * ez);
    LiftNormal3 n = {};
    if (jac) {
      const double pw = A.prior * w;
      n.H00 = pw; n.H11 = pw; n.H22 = pw;
      n.g0 = pw * ex; n.g1 = pw * ey; n.g2 = pw * ez;
#pragma unroll 1
      for (int c = 0; c < N; ++c) { sW[c][t] = 0.0; sW[CAL_N + c][t] = 0.0; sW[2 * CAL_N + c][t] = 0.0; sJ0[c][t] = 0.0; sJ1[c][t] = 0.0; sA[c][t] = 0.0; }
#pragma unroll
      for (int v = 0; v < CAL_MAXV; ++v) sT[v][t] = 0.0;
    }
#pragma unroll 1
    for (int v = 0; v < V; ++v) {
      if (!((mask >> v) & 1)) continue;
      const double* cq = ts + CTS_CAM + 8 * v;
      const Rot3 R = lift_rot3(cq[0], cq[1], cq[2], cq[3]);
      const double gf = cq[7];
      LiftCam cam = lift_cam(A.intr + ((long)g * V + v) * 9);
      cam.fx = gf * cam.fx; cam.fy = gf * cam.fy;
      const float* Uk = A.kp + (((long)v * Ftot + f) * J + j) * 2;
      const double wx = x - cq[4], wy = y - cq[5], wz = z - cq[6];
      const double X = R.r00 * wx + R.r10 * wy + R.r20 * wz, Y = R.r01 * wx + R.r11 * wy + R.r21 * wz, Z = R.r02 * wx + R.r12 * wy + R.r22 * wz;
      if (!(Z > 0.0)) notdeep = 1.0;
      const LiftProj pr = jac ? lift_project<true>(X, Y, Z, Uk, cam, A.distort) : lift_project<false>(X, Y, Z, Uk, cam, A.distort);
      const double du = pr.du, dv = pr.dv;
      const double e = du * du + dv * dv;
      const double tt = 1.0 + e / A.sigma2;                             // (sigma = +inf: exactly 1)
      sS[v][t] += w;
      sE[v][t] += w * sqrt(e);
      sF[v][t] += w * (e / tt);
      if (!jac) continue;
      const double wt = w * (1.0 / (tt * tt));
      const double c00 = pr.c00, c01 = pr.c01, c02 = pr.c02, c10 = pr.c10, c11 = pr.c11, c12 = pr.c12;
      const double j00 = c00 * R.r00 + c01 * R.r01 + c02 * R.r02, j01 = c00 * R.r10 + c01 * R.r11 + c02 * R.r12,
                   j02 = c00 * R.r20 + c01 * R.r21 + c02 * R.r22;      // J_pi R^T: with respect to the point
      const double j10 = c10 * R.r00 + c11 * R.r01 + c12 * R.r02, j11 = c10 * R.r10 + c11 * R.r11 + c12 * R.r12,
                   j12 = c10 * R.r20 + c11 * R.r21 + c12 * R.r22;
      lift_normal3_add(n, wt, du, dv, j00, j01, j02, j10, j11, j12);
      sT[v][t] = wt;
      const int slot = (int)ts[CTS_SLOT + v], fslot = (int)ts[CTS_FSLOT + v];
      if (slot >= 0) {
        // J_pi [-[P]x | I]: with respect to the camera's (omega, tau)
        const double jc0[6] = {c02 * Y - c01 * Z, c00 * Z - c02 * X, c01 * X - c00 * Y, c00, c01, c02};
        const double jc1[6] = {c12 * Y - c11 * Z, c10 * Z - c12 * X, c11 * X - c10 * Y, c10, c11, c12};
#pragma unroll
        for (int i = 0; i < 6; ++i) {
          const int c = 6 * slot + i;
          sJ0[c][t] = jc0[i]; sJ1[c][t] = jc1[i];
          sA[c][t] = wt * (jc0[i] * du + jc1[i] * dv);
          sW[c][t] = wt * (j00 * jc0[i] + j10 * jc1[i]);
          sW[CAL_N + c][t] = wt * (j01 * jc0[i] + j11 * jc1[i]);
          sW[2 * CAL_N + c][t] = wt * (j02 * jc0[i] + j12 * jc1[i]);
        }
      }
      if (fslot >= 0) {
        // (pi(P) - c) / g, pi(P) taken back from the residual: with respect to the view's focal factor
        const double g0 = ((du + (double)Uk[0]) - cam.cx) / gf, g1 = ((dv + (double)Uk[1]) - cam.cy) / gf;
        sJ0[fslot][t] = g0; sJ1[fslot][t] = g1;
        sA[fslot][t] = wt * (g0 * du + g1 * dv);
        sW[fslot][t] = wt * (j00 * g0 + j10 * g1);
        sW[CAL_N + fslot][t] = wt * (j01 * g0 + j11 * g1);
        sW[2 * CAL_N + fslot][t] = wt * (j02 * g0 + j12 * g1);
      }
    }
    if (!jac) continue;
    LiftAdj3 a;
    if (!lift_adj3(n, a)) { ufail = 1.0; continue; }
    const double i00 = a.c00 / a.det, i01 = a.c01 / a.det, i02 = a.c02 / a.det, i11 = a.c11 / a.det, i12 = a.c12 / a.det, i22 = a.c22 / a.det;
    const double y0 = (i00 * n.g0 + i01 * n.g1) + i02 * n.g2, y1 = (i01 * n.g0 + i11 * n.g1) + i12 * n.g2, y2 = (i02 * n.g0 + i12 * n.g1) + i22 * n.g2;
    pj[(long)(CPJ_YB + 0) * Ftot] = y0; pj[(long)(CPJ_YB + 1) * Ftot] = y1; pj[(long)(CPJ_YB + 2) * Ftot] = y2;
#pragma unroll 1
    for (int c = 0; c < N; ++c) {                                       // U^-1 W, and s_c += a_c - W_c^T U^-1 b
      const double w0 = sW[c][t], w1 = sW[CAL_N + c][t], w2 = sW[2 * CAL_N + c][t];
      double* Yp = pj + (long)(CPJ_Y + 3 * c) * Ftot;
      Yp[0] = (i00 * w0 + i01 * w1) + i02 * w2;
      Yp[Ftot] = (i01 * w0 + i11 * w1) + i12 * w2;
      Yp[2 * Ftot] = (i02 * w0 + i12 * w1) + i22 * w2;
      const double term = sA[c][t] - ((w0 * y0 + w1 * y1) + w2 * y2);
      CAL_ROW_AT(A, f, CROW_G + c) = CAL_ROW_AT(A, f, CROW_G + c) + term;
    }
#pragma unroll 1
    for (int r = 0; r < N; ++r) {                                       // S_rc += [same view] A_rc - W_r^T (U^-1 W_c), c <= r
      const double r0 = sW[r][t], r1 = sW[CAL_N + r][t], r2 = sW[2 * CAL_N + r][t], jr0 = sJ0[r][t], jr1 = sJ1[r][t];
      const int vr = (int)ts[CTS_COLV + r];
      const double wr = sT[vr][t];
#pragma unroll 1
      for (int c = 0; c <= r; ++c) {
        const double w0 = sW[c][t], w1 = sW[CAL_N + c][t], w2 = sW[2 * CAL_N + c][t];
        const double q0 = (i00 * w0 + i01 * w1) + i02 * w2, q1 = (i01 * w0 + i11 * w1) + i12 * w2, q2 = (i02 * w0 + i12 * w1) + i22 * w2;
        const double prod = (r0 * q0 + r1 * q1) + r2 * q2;
        const double blk = (int)ts[CTS_COLV + c] == vr ? wr * (jr0 * sJ0[c][t] + jr1 * sJ1[c][t]) : 0.0;
        const int e = CROW_S + r * (r + 1) / 2 + c;
        CAL_ROW_AT(A, f, e) = CAL_ROW_AT(A, f, e) + (blk - prod);
      }
    }
  }
  double F = 0.0;
#pragma unroll
  for (int v = 0; v < CAL_MAXV; ++v) {
    if (v < V && ((mask >> v) & 1)) {
      F += sF[v][t];
      CAL_ROW_AT(A, f, CROW_E + v) = sE[v][t];
      CAL_ROW_AT(A, f, CROW_W + v) = sS[v][t];
    }
  }
  CAL_ROW_AT(A, f, CROW_F) = F + A.prior * Pf;
  CAL_ROW_AT(A, f, CROW_DEEP) = notdeep;
  CAL_ROW_AT(A, f, CROW_U) = ufail;
}

// the take's outputs from its state: cameras and intrinsics (copied through while no step was taken), reproj and cost at the end (start: pass 0 only)
__device__ void cal_write(const CalArgs& A, int g, const double* ts, const double* sum, bool start, int ok) {
  const int V = A.V, steps = (int)ts[CTS_STEPS];
  for (int v = 0; v < V; ++v) {
    const long gv = (long)g * V + v;
    const bool moved = steps > 0 && ts[CTS_SLOT + v] >= 0.0, scaled = steps > 0 && ts[CTS_FSLOT + v] >= 0.0;
    const double* cam = ts + CTS_CAM + 8 * v;
    for (int c = 0; c < 4; ++c) A.quat_out[gv * 4 + c] = moved ? (float)cam[c] : A.quat[gv * 4 + c];
    for (int c = 0; c < 3; ++c) A.trans_out[gv * 3 + c] = moved ? (float)cam[4 + c] : A.trans[gv * 3 + c];
    for (int c = 0; c < 9; ++c) A.intr_out[gv * 9 + c] = (scaled && c < 2) ? (float)(cam[7] * (double)A.intr[gv * 9 + c]) : A.intr[gv * 9 + c];
    const float err = A.used[gv] > 0 ? (float)(sum[CROW_E + v] / sum[CROW_W + v]) : 0.f;
    if (start) A.reproj[gv * 2] = err;
    A.reproj[gv * 2 + 1] = err;
  }
  if (start) A.cost[(long)g * 2] = sum[CROW_F];
  A.cost[(long)g * 2 + 1] = sum[CROW_F];
  A.steps[g] = (unsigned char)steps;
  A.ok[g] = (unsigned char)ok;
}

// pass p of a take: the rows summed in frame order, the decision on the candidate, the next step
__global__ __launch_bounds__(CAL_TAKE_THREADS) void cal_take_kernel(CalArgs A, int p) {
  __shared__ double sum[CAL_ROW];
  __shared__ double L[CAL_N][CAL_N];
  __shared__ double x[CAL_N];
  __shared__ double cand[CAL_MAXV][8];
  const int g = blockIdx.x;
  double* ts = A.state + (long)g * CAL_TS;
  if (ts[CTS_STOP] != 0.0) return;                                      // (uniform; written by lane 0 of this take's workgroup of an earlier pass only)
  const FrameRange fr = lift_seq_frames(A.take_offset, g, A.Ftot);
#pragma unroll 1
  for (int e = threadIdx.x; e < CAL_ROW; e += CAL_TAKE_THREADS) {
    double acc = 0.0;
#pragma unroll 16
    for (long f = fr.f0; f < fr.f1; ++f) acc += CAL_ROW_AT(A, f, e);    // frames in increasing order (a frame outside the problem holds zeros)
    sum[e] = acc;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  const double Fn = sum[CROW_F];
  const bool deep = sum[CROW_DEEP] == 0.0;
  if (p == 0) {
    if (!(deep && __builtin_isfinite(Fn))) {                            // nothing to start from
      ts[CTS_STOP] = 1.0;
      cal_write(A, g, ts, sum, true, 0);
      return;
    }
  } else {
    if (!(deep && Fn <= (1.0 + CAL_SLACK) * ts[CTS_F])) {               // (a NaN cost is not taken either) the state stays, and so do the outputs
      ts[CTS_STOP] = 1.0;
      ts[CTS_USE_CAND] = 0.0;
      return;
    }
    ts[CTS_STEPS] = ts[CTS_STEPS] + 1.0;
  }
  ts[CTS_F] = Fn;
  ts[CTS_USE_CAND] = 1.0;
  cal_write(A, g, ts, sum, p == 0, 1);
  ts[CTS_STOP] = 1.0;                                                   // (cleared below where a next candidate exists)
  if (p >= A.iters || ts[CTS_ITERATE] == 0.0 || sum[CROW_U] != 0.0) return;
  // S = L L^T, a pivot must be > 1e-12 times its diagonal entry of S
  const int N = (int)ts[CTS_N], nfree = (int)ts[CTS_NFREE];
  for (int i = 0; i < N; ++i) {
    for (int j = 0; j <= i; ++j) {
      double s = sum[CROW_S + i * (i + 1) / 2 + j];
      for (int k = 0; k < j; ++k) s -= L[i][k] * L[j][k];
      if (i == j) {
        if (!(__builtin_isfinite(s) && s > CAL_PIVOT * sum[CROW_S + i * (i + 1) / 2 + i])) return;
        L[i][i] = sqrt(s);
      } else {
        L[i][j] = s / L[j][j];
      }
    }
  }
  for (int i = 0; i < N; ++i) {                                         // L y = s
    double s = sum[CROW_G + i];
    for (int k = 0; k < i; ++k) s -= L[i][k] * x[k];
    x[i] = s / L[i][i];
  }
  for (int i = N - 1; i >= 0; --i) {                                    // L^T z = y;  dc = -z
    double s = x[i];
    for (int k = i + 1; k < N; ++k) s -= L[k][i] * x[k];
    x[i] = s / L[i][i];
  }
  bool finite = true;
  for (int i = 0; i < N; ++i) { x[i] = 0.0 - x[i]; finite = finite && __builtin_isfinite(x[i]); }
  if (!finite) return;
  // the candidate cameras, step 4 of mp_lift_bundle_views: q <- q * conj(q_w), T <- T - R(q) tau
  for (int k = 0; k < nfree; ++k) {
    const double* cam = ts + CTS_CAM + 8 * (int)ts[CTS_VIEW + k];
    const double wx = x[6 * k], wy = x[6 * k + 1], wz = x[6 * k + 2];
    const double th2 = (wx * wx + wy * wy) + wz * wz;
    double bw = 1.0, bs = 0.5;                                          // q_w = (cos(th / 2), sin(th / 2) w / th);  th^2 <= 1e-16: (1, w / 2)
    if (th2 > CAL_SMALL) {
      const double th = sqrt(th2);
      double sn;
      sincos(0.5 * th, &sn, &bw);
      bs = sn / th;
    }
    const double bx = 0.0 - bs * wx, by = 0.0 - bs * wy, bz = 0.0 - bs * wz;          // the conjugate
    const double aw = cam[0], ax = cam[1], ay = cam[2], az = cam[3];
    double q0 = ((aw * bw - ax * bx) - ay * by) - az * bz, q1 = ((aw * bx + ax * bw) + ay * bz) - az * by;
    double q2 = ((aw * by - ax * bz) + ay * bw) + az * bx, q3 = ((aw * bz + ax * by) - ay * bx) + az * bw;
    const double nn = sqrt((q0 * q0 + q1 * q1) + (q2 * q2 + q3 * q3));
    q0 = q0 / nn; q1 = q1 / nn; q2 = q2 / nn; q3 = q3 / nn;
    if (q0 < 0.0 || (q0 == 0.0 && (q1 < 0.0 || (q1 == 0.0 && (q2 < 0.0 || (q2 == 0.0 && q3 < 0.0)))))) {
      q0 = 0.0 - q0; q1 = 0.0 - q1; q2 = 0.0 - q2; q3 = 0.0 - q3;      // canonical, mp_lift_align_views' rule (0 - x: a zero comes out as +0)
    }
    const Rot3 R = lift_rot3(q0, q1, q2, q3);
    const double tx = x[6 * k + 3], ty = x[6 * k + 4], tz = x[6 * k + 5];
    double* c = cand[k];
    c[0] = q0; c[1] = q1; c[2] = q2; c[3] = q3;
    c[4] = cam[4] - ((R.r00 * tx + R.r01 * ty) + R.r02 * tz);
    c[5] = cam[5] - ((R.r10 * tx + R.r11 * ty) + R.r12 * tz);
    c[6] = cam[6] - ((R.r20 * tx + R.r21 * ty) + R.r22 * tz);
    for (int i = 0; i < 7; ++i) finite = finite && __builtin_isfinite(c[i]);
  }
  // the candidate focal factors: additive, finite and > 0
  for (int v = 0; v < A.V; ++v) {
    const int fs = (int)ts[CTS_FSLOT + v];
    if (fs < 0) continue;
    const double gn = ts[CTS_CAM + 8 * v + 7] + x[fs];
    finite = finite && __builtin_isfinite(gn) && gn > 0.0;
  }
  if (!finite) return;
  for (int k = 0; k < nfree; ++k) {
    double* cam = ts + CTS_CAM + 8 * (int)ts[CTS_VIEW + k];
    for (int i = 0; i < 7; ++i) cam[i] = cand[k][i];
  }
  for (int v = 0; v < A.V; ++v) {
    const int fs = (int)ts[CTS_FSLOT + v];
    if (fs >= 0) ts[CTS_CAM + 8 * v + 7] = ts[CTS_CAM + 8 * v + 7] + x[fs];
  }
  for (int i = 0; i < N; ++i) ts[CTS_DC + i] = x[i];
  ts[CTS_STOP] = 0.0;
}

// the points that stand: the candidate if the last decision on it was to take it
__global__ __launch_bounds__(CAL_THREADS) void cal_final_kernel(CalArgs A) {
  const long f = (long)blockIdx.x * CAL_THREADS + threadIdx.x;
  if (f >= A.Ftot) return;
  const long Ftot = A.Ftot;
  if ((int)A.priv[(long)CPRIV_MASK * Ftot + f] == 0) return;            // outside the problem: copied through by cal_mask_kernel
  const int g = lift_seq_of(A.take_offset, A.G, f);
  const int base = A.state[(long)g * CAL_TS + CTS_USE_CAND] != 0.0 ? CPJ_CAND : CPJ_CUR;
#pragma unroll 1
  for (int j = 0; j < A.J; ++j) {
    if (A.weights != nullptr && A.weights[j] == 0.f) continue;          // (no camera sees it: it stays at start)
    const double* pj = A.priv + f + (long)(CPRIV_JOINT + j * CAL_PJ) * Ftot;
#pragma unroll
    for (int c = 0; c < 3; ++c) A.points[(f * A.J + j) * 3 + c] = (float)pj[(long)(base + c) * Ftot];
  }
}

}  // namespace mp
using namespace mp;

extern "C" {

int64_t mp_lift_calibrate_views_scratch_bytes(int V, int64_t Ftot, int J) {
  if (V < 1 || V > CAL_MAXV || Ftot <= 0 || Ftot > 0x7fffffffL || J < 2 || J > LIFT_MAXJ) return 0;
  return (int64_t)Ftot * (CAL_ROW + 1 + (int64_t)J * CAL_PJ + CAL_TS) * 8;
}

int mp_lift_calibrate_views(const float* start, const uint8_t* start_ok, const float* kp, int V, int64_t Ftot, int J, const uint8_t* valid,
                            const int64_t* take_offset, int G, const float* quat, const float* trans, const float* intr, const uint8_t* fixed,
                            const float* weights, int focal, int distort, float sigma, float prior, int iters, float* quat_out, float* trans_out,
                            float* intr_out, float* points, float* reproj, double* cost, uint8_t* steps, uint8_t* ok, int32_t* used, void* scratch,
                            int64_t scratch_bytes, void* stream) {
  static_assert(sizeof(long) == sizeof(int64_t), "LP64");
  MP_CHECK(start && kp && take_offset && quat && trans && intr, MP_ERR_ARG, "mp_lift_calibrate_views: null input");
  MP_CHECK(quat_out && trans_out && intr_out && points && reproj && cost && steps && ok && used, MP_ERR_ARG, "mp_lift_calibrate_views: null output");
  if (int rc = lift_take_shape("mp_lift_calibrate_views", V, (long)Ftot, J, G)) return rc;
  MP_CHECK(Ftot <= 0x7fffffffL, MP_ERR_ARG, "mp_lift_calibrate_views: Ftot=%ld G=%d out of range", (long)Ftot, G);
  MP_CHECK(focal == 0 || focal == 1, MP_ERR_ARG, "mp_lift_calibrate_views: focal=%d (0: the focal lengths are held, 1: one factor per view)", focal);
  MP_CHECK(distort == 0 || distort == 1, MP_ERR_ARG, "mp_lift_calibrate_views: distort=%d (0: project_to_2d_linear, 1: project_to_2d)", distort);
  MP_CHECK(sigma > 0.f, MP_ERR_ARG, "mp_lift_calibrate_views: sigma=%g must be > 0 (inf: every robust factor is 1)", (double)sigma);
  MP_CHECK(prior > 0.f && prior <= 3.402823466e38f, MP_ERR_ARG,
           "mp_lift_calibrate_views: prior=%g must be finite and > 0 (without it the keypoints leave the scale free)", (double)prior);
  MP_CHECK(iters >= 0 && iters <= MP_LIFT_CALIBRATE_MAXITERS, MP_ERR_ARG, "mp_lift_calibrate_views: iters=%d outside 0..%d", iters,
           MP_LIFT_CALIBRATE_MAXITERS);
  const int64_t need = mp_lift_calibrate_views_scratch_bytes(V, Ftot, J);
  MP_CHECK(scratch != nullptr && scratch_bytes >= need && ((uintptr_t)scratch & 7) == 0, MP_ERR_ARG,
           "mp_lift_calibrate_views: scratch null, misaligned or %ld bytes where %ld are needed", (long)scratch_bytes, (long)need);
  CalArgs a = {};
  a.start = start; a.start_ok = start_ok; a.kp = kp; a.valid = valid; a.take_offset = (const long*)take_offset;
  a.quat = quat; a.trans = trans; a.intr = intr; a.fixed = fixed; a.weights = weights;
  a.quat_out = quat_out; a.trans_out = trans_out; a.intr_out = intr_out; a.points = points; a.reproj = reproj; a.cost = cost; a.steps = steps; a.ok = ok;
  a.used = used;
  a.rows = (double*)scratch;
  a.priv = a.rows + (long)Ftot * CAL_ROW;
  a.state = a.priv + (long)Ftot * (1 + (long)J * CAL_PJ);
  a.Ftot = (long)Ftot; a.sigma2 = (double)sigma * (double)sigma; a.prior = (double)prior;
  a.V = V; a.J = J; a.G = G; a.distort = distort; a.focal = focal; a.iters = iters;
  const dim3 frames((unsigned)(((long)Ftot + CAL_THREADS - 1) / CAL_THREADS)), takes((unsigned)G);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(cal_mask_kernel, frames, dim3(CAL_THREADS), 0, s, a);
  hipLaunchKernelGGL(cal_init_kernel, takes, dim3(CAL_TAKE_THREADS), 0, s, a);
  for (int p = 0; p <= iters; ++p) {
    hipLaunchKernelGGL(cal_frame_kernel, frames, dim3(CAL_THREADS), 0, s, a, p);
    hipLaunchKernelGGL(cal_take_kernel, takes, dim3(CAL_TAKE_THREADS), 0, s, a, p);
  }
  hipLaunchKernelGGL(cal_final_kernel, frames, dim3(CAL_THREADS), 0, s, a);
  MP_LAUNCH_CHECK();
  return MP_OK;
}

}  // extern "C"

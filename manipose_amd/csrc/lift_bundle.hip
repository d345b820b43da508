// Bundle-adjusting a take's cameras (include/manipose_hip.h: mp_lift_bundle_views has the rule).  mp_lift_align_views gives a take's extrinsics in
// closed form from the lifted poses and the per-view roots; the 2-D keypoints - the only measured quantity - have no say in them.  This is the joint
// Gauss-Newton step over all free cameras (6 parameters each, at most 3) and all per-frame roots (3 each) on the robust reprojection error, the roots
// eliminated by a Schur complement: per frame a 3x3 inverse and its coupling blocks, per take one reduced system of at most 18 unknowns, summed over
// the frames in frame order.  tests/lift_bundle_ref.py states the rule in float64.
//
// FIVE KERNELS, launched in a fixed sequence on one stream, no grid-wide barrier and no synchronisation:
//   bundle_mask_kernel    one lane per frame: which views observe the frame (a bit mask), the root into the scratch, the frame's row zeroed
//   bundle_init_kernel    one workgroup per take: used[g][v] (integer counts: exact in any order), the gauge, the free views' slots, the take's state
//   bundle_frame_kernel   one lane per frame, pass p = 0 .. iters: at its head the frame takes the candidate of pass p - 1 (running means accepted) and
//                         forms its own, r - U^-1 (b + W dc); then it evaluates all views at the candidate and writes ONE ROW of BUNDLE_ROW doubles: its
//                         share of the reduced system S (lower triangle, packed by rows), of s, of F, of every view's E and W and two fault counts
//   bundle_take_kernel    one workgroup per take, pass p: lane e sums entry e of the take's rows in frame order (consecutive lanes read consecutive
//                         doubles); lane 0 then decides on the candidate, writes the take's outputs, factorises S in LDS and forms the next candidate
//   bundle_final_kernel   one lane per frame: the root that stands
// A take that has stopped is skipped by every later kernel (its state word says so).  A lane's blocks - 21 + 6 + 18 doubles per free view, 6 + 3 of
// the root - do not fit at once for three views: the lane goes VIEW BY VIEW, parks W_v in the scratch, inverts U when all views are in, and comes
// back for U^-1 W_v and the products W_k^T U^-1 W_l pair by pair.  Every register array is indexed by unrolled constants; what is indexed at run time
// (a view's slot, the reduced system during the factorisation) lives in global memory or LDS.  The frame-private scratch is laid out item-major
// (item * Ftot + f: consecutive lanes touch consecutive doubles), the rows frame-major (what the take kernel reads whole).
// Everything between the float32 loads and the float32 stores is fp64, without contraction; no atomics, fixed orders: identical bits on every call.
#include "lift_common.h"

#pragma clang fp contract(off)
#include "lift_geom.h"                    // after the pragma: the shared code takes this file's mode

namespace mp {

constexpr int BUNDLE_MAXV = MP_LIFT_FUSE_MAXV;
constexpr int BUNDLE_FREE = BUNDLE_MAXV - 1;            // free views at most: one view of a take that moves is fixed
constexpr int BUNDLE_N = 6 * BUNDLE_FREE;               // unknowns of the reduced system at most
constexpr int BUNDLE_THREADS = 64;                      // lanes of a workgroup of the per-frame kernels
constexpr int BUNDLE_TAKE_THREADS = 256;
// a frame's row: [0, 171) S, [171, 189) s, F, the joints not in front of their camera, E_v (4), W_v (4), the U that failed its test
constexpr int ROW_S = 0, ROW_G = BUNDLE_N * (BUNDLE_N + 1) / 2, ROW_F = ROW_G + BUNDLE_N, ROW_DEEP = ROW_F + 1, ROW_E = ROW_DEEP + 1,
              ROW_W = ROW_E + BUNDLE_MAXV, ROW_U = ROW_W + BUNDLE_MAXV, BUNDLE_ROW = ROW_U + 1;
static_assert(BUNDLE_ROW == 200 && BUNDLE_ROW <= BUNDLE_TAKE_THREADS, "one lane per entry of a row");
// a frame's private items: per slot W (18) and U^-1 W (18), then U^-1 b, the root that stands, the candidate, the mask
constexpr int PRIV_W = 0, PRIV_Y = 18, PRIV_SLOT = 36, PRIV_YB = PRIV_SLOT * BUNDLE_FREE, PRIV_CUR = PRIV_YB + 3, PRIV_CAND = PRIV_CUR + 3,
              PRIV_MASK = PRIV_CAND + 3, BUNDLE_PRIV = PRIV_MASK + 1;
// a take's state
constexpr int TS_STOP = 0, TS_STEPS = 1, TS_USE_CAND = 2, TS_N = 3, TS_GAUGE = 4, TS_F = 5, TS_SLOT = 6, TS_VIEW = 10, TS_CAM = 16, TS_DC = 44,
              BUNDLE_TS = 64;
static_assert(TS_CAM + 7 * BUNDLE_MAXV <= TS_DC && TS_DC + BUNDLE_N <= BUNDLE_TS, "the take's state");
constexpr long BUNDLE_FRAME_DOUBLES = BUNDLE_ROW + BUNDLE_PRIV + BUNDLE_TS;     // (a take has at least one frame or no state to keep)
constexpr double BUNDLE_DET = 1e-12, BUNDLE_PIVOT = 1e-12, BUNDLE_SLACK = 1e-6, BUNDLE_SMALL = 1e-16;

struct BundleArgs {
  const float* pose;             // (Ftot, J, 3)
  const float* root;             // (Ftot, 3)
  const unsigned char* root_ok;  // (Ftot) or null
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
  float* root_out;               // (Ftot, 3)
  float* reproj;                 // (G, V, 2)
  double* cost;                  // (G, 2)
  unsigned char* steps;          // (G)
  unsigned char* ok;             // (G)
  int* used;                     // (G, V)
  double* rows;                  // (Ftot, BUNDLE_ROW)
  double* priv;                  // (BUNDLE_PRIV, Ftot)
  double* state;                 // (G, BUNDLE_TS)
  long Ftot;
  double sigma2;
  int V, J, G, distort, iters;
};

__device__ __forceinline__ bool bundle_finite3(const float* x) { return __builtin_isfinite(((double)x[0] + (double)x[1]) + (double)x[2]); }

// 1. of the rule: the views that observe frame f, the frame's root into the scratch and into root_out, its row zeroed
__global__ __launch_bounds__(BUNDLE_THREADS) void bundle_mask_kernel(BundleArgs A) {
  const long f = (long)blockIdx.x * BUNDLE_THREADS + threadIdx.x;
  if (f >= A.Ftot) return;
  const int V = A.V, J = A.J;
  const int g = lift_seq_of(A.take_offset, A.G, f);
  const FrameRange fr = lift_seq_frames(A.take_offset, g, A.Ftot);
  const float* r = A.root + f * 3;
  const float r0 = r[0], r1 = r[1], r2 = r[2];
  A.root_out[f * 3] = r0; A.root_out[f * 3 + 1] = r1; A.root_out[f * 3 + 2] = r2;
  int mask = 0;
  bool good = f >= fr.f0 && f < fr.f1 && (A.root_ok == nullptr || A.root_ok[f] != 0) && bundle_finite3(r);
  if (good) {
    const float* P = A.pose + f * J * 3;
#pragma unroll 1
    for (int j = 0; j < J; ++j) good = good && bundle_finite3(P + j * 3);
  }
  if (good) {
#pragma unroll 1
    for (int v = 0; v < V; ++v) {
      if (A.valid != nullptr && A.valid[(long)v * A.Ftot + f] == 0) continue;
      if (!lift_quat_ok(A.quat + ((long)g * V + v) * 4)) continue;
      const float* U = A.kp + ((long)v * A.Ftot + f) * J * 2;
      bool fin = true;
#pragma unroll 1
      for (int j = 0; j < J; ++j)
        if (A.weights == nullptr || A.weights[j] != 0.f) fin = fin && __builtin_isfinite((double)U[2 * j] + (double)U[2 * j + 1]);
      if (fin) mask |= 1 << v;
    }
  }
  A.priv[(long)PRIV_MASK * A.Ftot + f] = (double)mask;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const double rc = c == 0 ? (double)r0 : (c == 1 ? (double)r1 : (double)r2);
    A.priv[(long)(PRIV_CUR + c) * A.Ftot + f] = rc;
    A.priv[(long)(PRIV_CAND + c) * A.Ftot + f] = rc;
  }
  double* row = A.rows + f * BUNDLE_ROW;
#pragma unroll 1
  for (int e = 0; e < BUNDLE_ROW; ++e) row[e] = 0.0;
}

// 2. of the rule: the used frames of every view, the gauge, the take's state
__global__ __launch_bounds__(BUNDLE_TAKE_THREADS) void bundle_init_kernel(BundleArgs A) {
  __shared__ int counts[BUNDLE_TAKE_THREADS / 64][BUNDLE_MAXV];
  const int g = blockIdx.x, V = A.V;
  const FrameRange fr = lift_seq_frames(A.take_offset, g, A.Ftot);
  int c0 = 0, c1 = 0, c2 = 0, c3 = 0;
#pragma unroll 1
  for (long f = fr.f0 + threadIdx.x; f < fr.f1; f += BUNDLE_TAKE_THREADS) {
    const int mask = (int)A.priv[(long)PRIV_MASK * A.Ftot + f];
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
  double* ts = A.state + (long)g * BUNDLE_TS;
  int lowest = -1, n = 0;
  bool anchored = false;
  for (int v = 0; v < V; ++v) {
    const int u = (counts[0][v] + counts[1][v]) + (counts[2][v] + counts[3][v]);
    A.used[(long)g * V + v] = u;
    if (u > 0 && lowest < 0) lowest = v;
  }
  for (int v = 0; v < BUNDLE_MAXV; ++v) ts[TS_SLOT + v] = -1.0;
  for (int k = 0; k < BUNDLE_MAXV; ++k) ts[TS_VIEW + k] = -1.0;
  for (int v = 0; v < V; ++v) {
    const int u = A.used[(long)g * V + v];
    const bool fix = A.fixed != nullptr ? A.fixed[(long)g * V + v] != 0 : v == lowest;
    if (fix) anchored = anchored || u > 0;
    else if (u > 0) { ts[TS_SLOT + v] = (double)n; ts[TS_VIEW + n] = (double)v; ++n; }
  }
  const bool gauge = anchored && n > 0;                                 // (then n <= V - 1 <= 3)
  if (!gauge) {
    n = 0;
    for (int v = 0; v < BUNDLE_MAXV; ++v) ts[TS_SLOT + v] = -1.0;
  }
  ts[TS_STOP] = 0.0; ts[TS_STEPS] = 0.0; ts[TS_USE_CAND] = 0.0; ts[TS_N] = (double)n; ts[TS_GAUGE] = gauge ? 1.0 : 0.0; ts[TS_F] = 0.0;
  for (int v = 0; v < BUNDLE_MAXV; ++v) {
    double* cam = ts + TS_CAM + 7 * v;
    cam[0] = 1.0; cam[1] = 0.0; cam[2] = 0.0; cam[3] = 0.0; cam[4] = 0.0; cam[5] = 0.0; cam[6] = 0.0;
    double n2;
    if (v < V && lift_quat_ok(A.quat + ((long)g * V + v) * 4, n2)) {
      const float* q = A.quat + ((long)g * V + v) * 4;
      const float* T = A.trans + ((long)g * V + v) * 3;
      const double nn = sqrt(n2);
      cam[0] = (double)q[0] / nn; cam[1] = (double)q[1] / nn; cam[2] = (double)q[2] / nn; cam[3] = (double)q[3] / nn;
      cam[4] = T[0]; cam[5] = T[1]; cam[6] = T[2];
    }
  }
  for (int i = 0; i < BUNDLE_N; ++i) ts[TS_DC + i] = 0.0;
}

// pass p of a frame: 4. and 5. its candidate root, 3. the evaluation of every view at the candidate, 5. its row of the reduced system.
// The joint loop keeps its OWN statement of the camera model, the root's normal equations and their cofactor inverse (lift_geom.h's
// lift_project, LiftNormal3 and lift_adj3 word for word): through the shared functions this kernel, at 250 VGPRs, kept its bits, registers and
// fp64 opcode counts but was scheduled differently and ran 1 to 3 % slower in every pass with a Jacobian.  A change to the camera model or to
// the 1e-12 rule in lift_geom.h is made here as well; tests/test_gpu_lift_bundle.py holds this copy to the float64 statement.
__global__ __launch_bounds__(BUNDLE_THREADS) void bundle_frame_kernel(BundleArgs A, int p) {
  const long f = (long)blockIdx.x * BUNDLE_THREADS + threadIdx.x;
  if (f >= A.Ftot) return;
  const long Ftot = A.Ftot;
  const int V = A.V, J = A.J;
  const int g = lift_seq_of(A.take_offset, A.G, f);
  const double* ts = A.state + (long)g * BUNDLE_TS;
  if (ts[TS_STOP] != 0.0) return;
  double* pv = A.priv + f;                                              // item i of this frame: pv[i * Ftot]
  const int mask = (int)pv[(long)PRIV_MASK * Ftot];
  if (mask == 0) return;
  const int n = (int)ts[TS_N];
  const bool jac = p < A.iters;
  double rx = pv[(long)PRIV_CAND * Ftot], ry = pv[(long)(PRIV_CAND + 1) * Ftot], rz = pv[(long)(PRIV_CAND + 2) * Ftot];
  if (p > 0) {
    // the take still runs: the candidate of pass p - 1 was taken.  The next: r - (U^-1 b + sum_k (U^-1 W_k) dc_k), slots in order, columns in order
    pv[(long)PRIV_CUR * Ftot] = rx; pv[(long)(PRIV_CUR + 1) * Ftot] = ry; pv[(long)(PRIV_CUR + 2) * Ftot] = rz;
    double dx = pv[(long)PRIV_YB * Ftot], dy = pv[(long)(PRIV_YB + 1) * Ftot], dz = pv[(long)(PRIV_YB + 2) * Ftot];
#pragma unroll 1
    for (int k = 0; k < n; ++k) {
      if (!((mask >> (int)ts[TS_VIEW + k]) & 1)) continue;
      const double* Y = pv + (long)(PRIV_SLOT * k + PRIV_Y) * Ftot;
      const double* dc = ts + TS_DC + 6 * k;
#pragma unroll
      for (int c = 0; c < 6; ++c) {
        dx += Y[(long)c * Ftot] * dc[c]; dy += Y[(long)(6 + c) * Ftot] * dc[c]; dz += Y[(long)(12 + c) * Ftot] * dc[c];
      }
    }
    rx = rx - dx; ry = ry - dy; rz = rz - dz;
    pv[(long)PRIV_CAND * Ftot] = rx; pv[(long)(PRIV_CAND + 1) * Ftot] = ry; pv[(long)(PRIV_CAND + 2) * Ftot] = rz;
  }
  double* row = A.rows + f * BUNDLE_ROW;
  const float* P = A.pose + f * J * 3;
  double U00 = 0.0, U01 = 0.0, U02 = 0.0, U11 = 0.0, U12 = 0.0, U22 = 0.0, b0 = 0.0, b1 = 0.0, b2 = 0.0, F = 0.0, notdeep = 0.0;
#pragma unroll 1
  for (int v = 0; v < V; ++v) {
    if (!((mask >> v) & 1)) continue;                                   // (its E, W and blocks stay the zeros of bundle_mask_kernel)
    const double* cq = ts + TS_CAM + 7 * v;
    const Rot3 R = lift_rot3(cq[0], cq[1], cq[2], cq[3]);
    const float* cam = A.intr + ((long)g * V + v) * 9;
    const float* Uk = A.kp + ((long)v * Ftot + f) * J * 2;
    const double fx = cam[0], fy = cam[1], cx = cam[2], cy = cam[3], k1 = cam[4], k2 = cam[5], k3 = cam[6], p1 = cam[7], p2 = cam[8];
    const double ox = rx - cq[4], oy = ry - cq[5], oz = rz - cq[6];
    const int slot = (int)ts[TS_SLOT + v];
    const bool cams = jac && slot >= 0;
    double E = 0.0, W = 0.0;
    double Am[21], am[6], Wm[18];
#pragma unroll
    for (int i = 0; i < 21; ++i) Am[i] = 0.0;
#pragma unroll
    for (int i = 0; i < 6; ++i) am[i] = 0.0;
#pragma unroll
    for (int i = 0; i < 18; ++i) Wm[i] = 0.0;
#pragma unroll 1
    for (int j = 0; j < J; ++j) {                                       // sums in joint order
      const double w = A.weights != nullptr ? (double)A.weights[j] : 1.0;
      if (w == 0.0) continue;
      const double wx = (double)P[j * 3] + ox, wy = (double)P[j * 3 + 1] + oy, wz = (double)P[j * 3 + 2] + oz;
      const double X = R.r00 * wx + R.r10 * wy + R.r20 * wz, Y = R.r01 * wx + R.r11 * wy + R.r21 * wz, Z = R.r02 * wx + R.r12 * wy + R.r22 * wz;
      if (!(Z > 0.0)) notdeep = 1.0;
      const double qx = X / Z, qy = Y / Z;
      const double xx = lift_clamp1(qx), yy = lift_clamp1(qy);
      double px = xx, py = yy;
      double a = 1.0, b = 0.0, c = 0.0, d = 1.0;                        // d(px, py) / d(x, y)
      if (A.distort) {
        const double r2 = xx * xx + yy * yy;
        const double m = 1.0 + (k1 * r2 + k2 * (r2 * r2) + k3 * (r2 * r2 * r2)) + (p1 * xx + p2 * yy);
        px = xx * m + p1 * r2;
        py = yy * m + p2 * r2;
        const double dm = k1 + 2.0 * k2 * r2 + 3.0 * k3 * (r2 * r2);
        const double mx = 2.0 * xx * dm + p1, my = 2.0 * yy * dm + p2;
        a = m + xx * mx + 2.0 * p1 * xx;
        b = xx * my + 2.0 * p1 * yy;
        c = yy * mx + 2.0 * p2 * xx;
        d = m + yy * my + 2.0 * p2 * yy;
      }
      const double du = fx * px + cx - (double)Uk[2 * j], dv = fy * py + cy - (double)Uk[2 * j + 1];
      const double e = du * du + dv * dv;
      const double t = 1.0 + e / A.sigma2;                              // (sigma = +inf: exactly 1)
      W += w;
      E += w * sqrt(e);
      F += w * (e / t);
      if (!jac) continue;
      const double wt = w * (1.0 / (t * t));
      const double sx = (qx >= -1.0 && qx <= 1.0) ? 1.0 : 0.0, sy = (qy >= -1.0 && qy <= 1.0) ? 1.0 : 0.0;   // the derivative of the clamp
      const double iz = 1.0 / Z;
      const double xz = sx * iz, yz = sy * iz, xq = sx * (-qx / Z), yq = sy * (-qy / Z);
      const double c00 = fx * (a * xz), c01 = fx * (b * yz), c02 = fx * (a * xq + b * yq);                  // J_pi: with respect to the camera-space point
      const double c10 = fy * (c * xz), c11 = fy * (d * yz), c12 = fy * (c * xq + d * yq);
      const double j00 = c00 * R.r00 + c01 * R.r01 + c02 * R.r02, j01 = c00 * R.r10 + c01 * R.r11 + c02 * R.r12,
                   j02 = c00 * R.r20 + c01 * R.r21 + c02 * R.r22;                                            // J_pi R^T: with respect to the root
      const double j10 = c10 * R.r00 + c11 * R.r01 + c12 * R.r02, j11 = c10 * R.r10 + c11 * R.r11 + c12 * R.r12,
                   j12 = c10 * R.r20 + c11 * R.r21 + c12 * R.r22;
      U00 += wt * (j00 * j00 + j10 * j10);
      U01 += wt * (j00 * j01 + j10 * j11);
      U02 += wt * (j00 * j02 + j10 * j12);
      U11 += wt * (j01 * j01 + j11 * j11);
      U12 += wt * (j01 * j02 + j11 * j12);
      U22 += wt * (j02 * j02 + j12 * j12);
      b0 += wt * (j00 * du + j10 * dv);
      b1 += wt * (j01 * du + j11 * dv);
      b2 += wt * (j02 * du + j12 * dv);
      if (!cams) continue;
      // J_pi [-[P]x | I]: with respect to the camera's (omega, tau)
      const double jc0[6] = {c02 * Y - c01 * Z, c00 * Z - c02 * X, c01 * X - c00 * Y, c00, c01, c02};
      const double jc1[6] = {c12 * Y - c11 * Z, c10 * Z - c12 * X, c11 * X - c10 * Y, c10, c11, c12};
      const double jr0[3] = {j00, j01, j02}, jr1[3] = {j10, j11, j12};
#pragma unroll
      for (int i = 0; i < 6; ++i) {
#pragma unroll
        for (int l = 0; l <= i; ++l) Am[i * (i + 1) / 2 + l] += wt * (jc0[i] * jc0[l] + jc1[i] * jc1[l]);
        am[i] += wt * (jc0[i] * du + jc1[i] * dv);
#pragma unroll
        for (int r = 0; r < 3; ++r) Wm[r * 6 + i] += wt * (jr0[r] * jc0[i] + jr1[r] * jc1[i]);
      }
    }
    row[ROW_E + v] = E;
    row[ROW_W + v] = W;
    if (cams) {
      double* Wp = pv + (long)(PRIV_SLOT * slot + PRIV_W) * Ftot;
#pragma unroll
      for (int i = 0; i < 18; ++i) Wp[(long)i * Ftot] = Wm[i];
      const int o = 6 * slot;
#pragma unroll
      for (int i = 0; i < 6; ++i) {
#pragma unroll
        for (int l = 0; l <= i; ++l) row[ROW_S + (o + i) * (o + i + 1) / 2 + o + l] = Am[i * (i + 1) / 2 + l];
        row[ROW_G + o + i] = am[i];
      }
    }
  }
  row[ROW_F] = F;
  row[ROW_DEEP] = notdeep;
  if (!jac) return;
  // U^-1 by cofactors, mp_lift_place_refine's test
  const double c00 = U11 * U22 - U12 * U12, c01 = U02 * U12 - U01 * U22, c02 = U01 * U12 - U02 * U11;
  const double det = U00 * c00 + U01 * c01 + U02 * c02, scale = U00 * U11 * U22;
  if (!(__builtin_isfinite(det) && __builtin_isfinite(scale) && det > BUNDLE_DET * scale)) { row[ROW_U] = 1.0; return; }
  row[ROW_U] = 0.0;
  const double c11 = U00 * U22 - U02 * U02, c12 = U01 * U02 - U00 * U12, c22 = U00 * U11 - U01 * U01;
  const double i00 = c00 / det, i01 = c01 / det, i02 = c02 / det, i11 = c11 / det, i12 = c12 / det, i22 = c22 / det;
  const double y0 = (i00 * b0 + i01 * b1) + i02 * b2, y1 = (i01 * b0 + i11 * b1) + i12 * b2, y2 = (i02 * b0 + i12 * b1) + i22 * b2;
  pv[(long)PRIV_YB * Ftot] = y0; pv[(long)(PRIV_YB + 1) * Ftot] = y1; pv[(long)(PRIV_YB + 2) * Ftot] = y2;
#pragma unroll 1
  for (int k = 0; k < n; ++k) {                                         // U^-1 W_k, and s_k = a_k - W_k^T U^-1 b
    if (!((mask >> (int)ts[TS_VIEW + k]) & 1)) continue;
    const double* Wp = pv + (long)(PRIV_SLOT * k + PRIV_W) * Ftot;
    double* Yp = pv + (long)(PRIV_SLOT * k + PRIV_Y) * Ftot;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      const double w0 = Wp[(long)i * Ftot], w1 = Wp[(long)(6 + i) * Ftot], w2 = Wp[(long)(12 + i) * Ftot];
      Yp[(long)i * Ftot] = (i00 * w0 + i01 * w1) + i02 * w2;
      Yp[(long)(6 + i) * Ftot] = (i01 * w0 + i11 * w1) + i12 * w2;
      Yp[(long)(12 + i) * Ftot] = (i02 * w0 + i12 * w1) + i22 * w2;
      row[ROW_G + 6 * k + i] = row[ROW_G + 6 * k + i] - ((w0 * y0 + w1 * y1) + w2 * y2);
    }
  }
#pragma unroll 1
  for (int k = 0; k < n; ++k) {                                         // S_kl = [k == l] A_k - W_k^T (U^-1 W_l), l <= k
    if (!((mask >> (int)ts[TS_VIEW + k]) & 1)) continue;
    const double* Wp = pv + (long)(PRIV_SLOT * k + PRIV_W) * Ftot;
    double Wk[18];
#pragma unroll
    for (int i = 0; i < 18; ++i) Wk[i] = Wp[(long)i * Ftot];
#pragma unroll 1
    for (int l = 0; l <= k; ++l) {
      if (!((mask >> (int)ts[TS_VIEW + l]) & 1)) continue;
      const double* Yp = pv + (long)(PRIV_SLOT * l + PRIV_Y) * Ftot;
      double Yl[18];
#pragma unroll
      for (int i = 0; i < 18; ++i) Yl[i] = Yp[(long)i * Ftot];
#pragma unroll
      for (int i = 0; i < 6; ++i) {
        const int ri = 6 * k + i;
#pragma unroll
        for (int c = 0; c < 6; ++c) {
          const double prod = (Wk[i] * Yl[c] + Wk[6 + i] * Yl[6 + c]) + Wk[12 + i] * Yl[12 + c];
          double* at = row + ROW_S + ri * (ri + 1) / 2 + 6 * l + c;
          if (k != l) *at = 0.0 - prod;
          else if (c <= i) *at = *at - prod;
        }
      }
    }
  }
}

// the take's outputs from its state: the cameras (copied through while no step was taken), reproj and cost at the end (start: pass 0 only)
__device__ void bundle_write(const BundleArgs& A, int g, const double* ts, const double* sum, bool start, int ok) {
  const int V = A.V, steps = (int)ts[TS_STEPS];
  for (int v = 0; v < V; ++v) {
    const long gv = (long)g * V + v;
    const bool moved = steps > 0 && ts[TS_SLOT + v] >= 0.0;
    const double* cam = ts + TS_CAM + 7 * v;
    for (int c = 0; c < 4; ++c) A.quat_out[gv * 4 + c] = moved ? (float)cam[c] : A.quat[gv * 4 + c];
    for (int c = 0; c < 3; ++c) A.trans_out[gv * 3 + c] = moved ? (float)cam[4 + c] : A.trans[gv * 3 + c];
    const float err = A.used[gv] > 0 ? (float)(sum[ROW_E + v] / sum[ROW_W + v]) : 0.f;
    if (start) A.reproj[gv * 2] = err;
    A.reproj[gv * 2 + 1] = err;
  }
  if (start) A.cost[(long)g * 2] = sum[ROW_F];
  A.cost[(long)g * 2 + 1] = sum[ROW_F];
  A.steps[g] = (unsigned char)steps;
  A.ok[g] = (unsigned char)ok;
}

// pass p of a take: the rows summed in frame order, the decision on the candidate, the next step
__global__ __launch_bounds__(BUNDLE_TAKE_THREADS) void bundle_take_kernel(BundleArgs A, int p) {
  __shared__ double sum[BUNDLE_ROW];
  __shared__ double L[BUNDLE_N][BUNDLE_N];
  __shared__ double x[BUNDLE_N];
  __shared__ double cand[BUNDLE_FREE][7];
  const int g = blockIdx.x;
  double* ts = A.state + (long)g * BUNDLE_TS;
  if (ts[TS_STOP] != 0.0) return;                                       // (uniform; written by lane 0 of this take's workgroup of an earlier pass only)
  const FrameRange fr = lift_seq_frames(A.take_offset, g, A.Ftot);
  if (threadIdx.x < BUNDLE_ROW) {
    const double* col = A.rows + threadIdx.x;
    double acc = 0.0;
#pragma unroll 16
    for (long f = fr.f0; f < fr.f1; ++f) acc += col[f * BUNDLE_ROW];    // frames in increasing order (a frame outside the problem holds zeros)
    sum[threadIdx.x] = acc;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  const double Fn = sum[ROW_F];
  const bool deep = sum[ROW_DEEP] == 0.0;
  if (p == 0) {
    if (!(deep && __builtin_isfinite(Fn))) {                            // nothing to start from
      ts[TS_STOP] = 1.0;
      bundle_write(A, g, ts, sum, true, 0);
      return;
    }
  } else {
    if (!(deep && Fn <= (1.0 + BUNDLE_SLACK) * ts[TS_F])) {             // (a NaN cost is not taken either) the state stays, and so do the outputs
      ts[TS_STOP] = 1.0;
      ts[TS_USE_CAND] = 0.0;
      return;
    }
    ts[TS_STEPS] = ts[TS_STEPS] + 1.0;
  }
  ts[TS_F] = Fn;
  ts[TS_USE_CAND] = 1.0;
  bundle_write(A, g, ts, sum, p == 0, 1);
  ts[TS_STOP] = 1.0;                                                    // (cleared below where a next candidate exists)
  if (p >= A.iters || ts[TS_GAUGE] == 0.0 || sum[ROW_U] != 0.0) return;
  // S = L L^T, a pivot must be > 1e-12 times its diagonal entry of S
  const int N = 6 * (int)ts[TS_N];
  for (int i = 0; i < N; ++i) {
    for (int j = 0; j <= i; ++j) {
      double s = sum[ROW_S + i * (i + 1) / 2 + j];
      for (int k = 0; k < j; ++k) s -= L[i][k] * L[j][k];
      if (i == j) {
        if (!(__builtin_isfinite(s) && s > BUNDLE_PIVOT * sum[ROW_S + i * (i + 1) / 2 + i])) return;
        L[i][i] = sqrt(s);
      } else {
        L[i][j] = s / L[j][j];
      }
    }
  }
  for (int i = 0; i < N; ++i) {                                         // L y = s
    double s = sum[ROW_G + i];
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
  // 4. the candidate cameras: (R^T, -R^T T) <- (exp([w]x) R^T, exp([w]x) (-R^T T) + tau), which is q <- q * conj(q_w), T <- T - R(q) tau
  for (int k = 0; k < N / 6; ++k) {
    const double* cam = ts + TS_CAM + 7 * (int)ts[TS_VIEW + k];
    const double wx = x[6 * k], wy = x[6 * k + 1], wz = x[6 * k + 2];
    const double th2 = (wx * wx + wy * wy) + wz * wz;
    double bw = 1.0, bs = 0.5;                                          // q_w = (cos(th / 2), sin(th / 2) w / th);  th^2 <= 1e-16: (1, w / 2)
    if (th2 > BUNDLE_SMALL) {
      const double th = sqrt(th2);
      double sn;
      sincos(0.5 * th, &sn, &bw);                                       // (one argument reduction for both)
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
  if (!finite) return;
  for (int k = 0; k < N / 6; ++k) {
    double* cam = ts + TS_CAM + 7 * (int)ts[TS_VIEW + k];
    for (int i = 0; i < 7; ++i) cam[i] = cand[k][i];
  }
  for (int i = 0; i < N; ++i) ts[TS_DC + i] = x[i];
  ts[TS_STOP] = 0.0;
}

// 6. the root that stands: the candidate if the last decision on it was to take it
__global__ __launch_bounds__(BUNDLE_THREADS) void bundle_final_kernel(BundleArgs A) {
  const long f = (long)blockIdx.x * BUNDLE_THREADS + threadIdx.x;
  if (f >= A.Ftot) return;
  if ((int)A.priv[(long)PRIV_MASK * A.Ftot + f] == 0) return;           // outside the problem: copied through by bundle_mask_kernel
  const int g = lift_seq_of(A.take_offset, A.G, f);
  const int base = A.state[(long)g * BUNDLE_TS + TS_USE_CAND] != 0.0 ? PRIV_CAND : PRIV_CUR;
#pragma unroll
  for (int c = 0; c < 3; ++c) A.root_out[f * 3 + c] = (float)A.priv[(long)(base + c) * A.Ftot + f];
}

}  // namespace mp
using namespace mp;

extern "C" {

int64_t mp_lift_bundle_views_scratch_bytes(int V, int64_t Ftot) {
  if (V < 1 || V > BUNDLE_MAXV || Ftot <= 0 || Ftot > 0x7fffffffL) return 0;
  return (int64_t)Ftot * BUNDLE_FRAME_DOUBLES * 8;
}

int mp_lift_bundle_views(const float* pose, const float* root, const uint8_t* root_ok, const float* kp, int V, int64_t Ftot, int J, const uint8_t* valid,
                         const int64_t* take_offset, int G, const float* quat, const float* trans, const float* intr, const uint8_t* fixed,
                         const float* weights, int distort, float sigma, int iters, float* quat_out, float* trans_out, float* root_out, float* reproj,
                         double* cost, uint8_t* steps, uint8_t* ok, int32_t* used, void* scratch, int64_t scratch_bytes, void* stream) {
  static_assert(sizeof(long) == sizeof(int64_t), "LP64");
  MP_CHECK(pose && root && kp && take_offset && quat && trans && intr, MP_ERR_ARG, "mp_lift_bundle_views: null input");
  MP_CHECK(quat_out && trans_out && root_out && reproj && cost && steps && ok && used, MP_ERR_ARG, "mp_lift_bundle_views: null output");
  if (int rc = lift_take_shape("mp_lift_bundle_views", V, (long)Ftot, J, G)) return rc;
  MP_CHECK(Ftot <= 0x7fffffffL, MP_ERR_ARG, "mp_lift_bundle_views: Ftot=%ld G=%d out of range", (long)Ftot, G);
  MP_CHECK(distort == 0 || distort == 1, MP_ERR_ARG, "mp_lift_bundle_views: distort=%d (0: project_to_2d_linear, 1: project_to_2d)", distort);
  MP_CHECK(sigma > 0.f, MP_ERR_ARG, "mp_lift_bundle_views: sigma=%g must be > 0 (inf: every robust factor is 1)", (double)sigma);
  MP_CHECK(iters >= 0 && iters <= MP_LIFT_BUNDLE_MAXITERS, MP_ERR_ARG, "mp_lift_bundle_views: iters=%d outside 0..%d", iters, MP_LIFT_BUNDLE_MAXITERS);
  const int64_t need = mp_lift_bundle_views_scratch_bytes(V, Ftot);
  MP_CHECK(scratch != nullptr && scratch_bytes >= need && ((uintptr_t)scratch & 7) == 0, MP_ERR_ARG,
           "mp_lift_bundle_views: scratch null, misaligned or %ld bytes where %ld are needed", (long)scratch_bytes, (long)need);
  BundleArgs a = {};
  a.pose = pose; a.root = root; a.root_ok = root_ok; a.kp = kp; a.valid = valid; a.take_offset = (const long*)take_offset;
  a.quat = quat; a.trans = trans; a.intr = intr; a.fixed = fixed; a.weights = weights;
  a.quat_out = quat_out; a.trans_out = trans_out; a.root_out = root_out; a.reproj = reproj; a.cost = cost; a.steps = steps; a.ok = ok; a.used = used;
  a.rows = (double*)scratch;
  a.priv = a.rows + (long)Ftot * BUNDLE_ROW;
  a.state = a.priv + (long)Ftot * BUNDLE_PRIV;
  a.Ftot = (long)Ftot; a.sigma2 = (double)sigma * (double)sigma;
  a.V = V; a.J = J; a.G = G; a.distort = distort; a.iters = iters;
  const dim3 frames((unsigned)(((long)Ftot + BUNDLE_THREADS - 1) / BUNDLE_THREADS)), takes((unsigned)G);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(bundle_mask_kernel, frames, dim3(BUNDLE_THREADS), 0, s, a);
  hipLaunchKernelGGL(bundle_init_kernel, takes, dim3(BUNDLE_TAKE_THREADS), 0, s, a);
  for (int p = 0; p <= iters; ++p) {
    hipLaunchKernelGGL(bundle_frame_kernel, frames, dim3(BUNDLE_THREADS), 0, s, a, p);
    hipLaunchKernelGGL(bundle_take_kernel, takes, dim3(BUNDLE_TAKE_THREADS), 0, s, a, p);
  }
  hipLaunchKernelGGL(bundle_final_kernel, frames, dim3(BUNDLE_THREADS), 0, s, a);
  MP_LAUNCH_CHECK();
  return MP_OK;
}

}  // extern "C"

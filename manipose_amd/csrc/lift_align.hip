// Aligning the views of a take without extrinsics (include/manipose_hip.h: mp_lift_align_views has the rule).  Every view's lifted poses are
// root-relative bodies in that camera's frame, so a view and the take's reference view differ by ONE rotation for the whole take: Horn's closed
// form over all used frames, re-weighted `iters` times with a Geman-McClure-like weight per frame (a depth-mirrored body is an outlier of the
// whole frame, not of a joint), then - with placed roots - one translation.  tests/lift_align_ref.py states the rule in float64.
//
// ONE WORKGROUP OF 256 LANES OWNS ONE (take, view).  A lane walks the frames f0 + lane, f0 + lane + 256, ... in order and keeps its eleven sums
// (9 of M, sum w, the count) in registers: the arrays below are indexed by unrolled constants only, nothing lands in scratch.  The lanes' sums
// are added by an xor butterfly within a wave - an addition is commutative, so all 64 lanes hold the same bits - and the four waves' sums through
// LDS in wave order, (w0 + w1) + (w2 + w3); EVERY lane then solves the 4x4 eigenproblem (cyclic Jacobi in registers: lift_geom.h's lift_eig4,
// shared with lift_score.hip) on identical inputs, so the branches on its result are uniform
// and the next pass has its rotation without a broadcast.  The passes follow one another inside the workgroup: no grid-wide synchronisation.
// A pass reads both views' poses again (iters + 2 passes, with a trajectory iters + 4): a frame's J C floats are contiguous, consecutive lanes
// are J C floats apart, every cache line fetched is used whole.  It runs once per take and sits on one CU; no rate is claimed for it.
// Everything between the float32 loads and the float32 stores is fp64, without contraction; no atomics, fixed orders: identical bits on every call.
#include "lift_common.h"

#pragma clang fp contract(off)
#include "lift_geom.h"                    // after the pragma: the shared code takes this file's mode

namespace mp {

constexpr int ALIGN_MAXV = MP_LIFT_FUSE_MAXV;
constexpr int ALIGN_THREADS = 256, ALIGN_WAVES = ALIGN_THREADS / 64;
constexpr int ALIGN_SUMS = 11;                   // of a pass: 9 of M, sum w, the used frames (fewer in the later passes)
constexpr double ALIGN_GAP = 1e-9;               // (lambda_1 - lambda_2) <= ALIGN_GAP |lambda_1|: the rotation is not determined

struct AlignArgs {
  const float* poses;            // (V, Ftot, J, C)
  const unsigned char* valid;    // (V, Ftot) or null
  const long* take_offset;       // (G + 1) device
  const float* traj;             // (V, Ftot, 3) or null
  const unsigned char* traj_ok;  // (V, Ftot) or null
  float* quat;                   // (G, V, 4)
  float* trans;                  // (G, V, 3) or null
  float* rms;                    // (G, V)
  float* trans_rms;              // (G, V) or null
  int* used;                     // (G, V)
  unsigned char* ok;             // (G, V)
  long Ftot;
  double sigma2;                 // sigma^2 (+inf: every weight is exactly 1)
  int V, J, C, G, iters;
};

// the lanes' sums added: a butterfly within the wave, then the waves in order; every lane returns with the workgroup's sums
__device__ __forceinline__ void align_reduce(double (&x)[ALIGN_SUMS], double* lds) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
#pragma unroll
    for (int k = 0; k < ALIGN_SUMS; ++k) x[k] += __shfl_xor(x[k], off);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();                                                      // (the readers of the reduction before are done)
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < ALIGN_SUMS; ++k) lds[wave * ALIGN_SUMS + k] = x[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < ALIGN_SUMS; ++k)
    x[k] = (lds[k] + lds[ALIGN_SUMS + k]) + (lds[2 * ALIGN_SUMS + k] + lds[3 * ALIGN_SUMS + k]);
}

// step 4 on the workgroup's sums s (9 of M, sum w): the canonical unit quaternion; false: degenerate (the gap is judged by the caller)
__device__ __forceinline__ bool align_solve(const double (&s)[ALIGN_SUMS], double (&q)[4], double& lam1, double& lam2) {
  bool finite = true;
#pragma unroll
  for (int k = 0; k < 10; ++k) finite = finite && __builtin_isfinite(s[k]);
  if (!finite || !(s[9] > 0.0)) return false;
  // h[r][c] = s[3 r + c] = sum w b_v[r] b_ref[c]: Horn's N for the rotation taking b_v onto b_ref (quaternion w, x, y, z)
  double n[4][4];
  n[0][0] = s[0] + s[4] + s[8];
  n[0][1] = n[1][0] = s[5] - s[7];
  n[0][2] = n[2][0] = s[6] - s[2];
  n[0][3] = n[3][0] = s[1] - s[3];
  n[1][1] = s[0] - s[4] - s[8];
  n[1][2] = n[2][1] = s[1] + s[3];
  n[1][3] = n[3][1] = s[6] + s[2];
  n[2][2] = -s[0] + s[4] - s[8];
  n[2][3] = n[3][2] = s[5] + s[7];
  n[3][3] = -s[0] - s[4] + s[8];
  lift_eig4(n, q, lam1, lam2);
  if (!(lam1 > 0.0)) return false;
  const double qn = 1.0 / sqrt((q[0] * q[0] + q[1] * q[1]) + (q[2] * q[2] + q[3] * q[3]));
#pragma unroll
  for (int k = 0; k < 4; ++k) q[k] = q[k] * qn;
  const bool flip = q[0] < 0.0 || (q[0] == 0.0 && (q[1] < 0.0 || (q[1] == 0.0 && (q[2] < 0.0 || (q[2] == 0.0 && q[3] < 0.0)))));
  if (flip) {
#pragma unroll
    for (int k = 0; k < 4; ++k) q[k] = 0.0 - q[k];                      // (0 - x: a zero component comes out as +0)
  }
  return __builtin_isfinite((q[0] + q[1]) + (q[2] + q[3]));
}

// |b_ref - R b_v|^2, channel order
__device__ __forceinline__ double align_res2(const Rot3& R, double vx, double vy, double vz, double rx, double ry, double rz) {
  const double ex = rx - ((R.r00 * vx + R.r01 * vy) + R.r02 * vz);
  const double ey = ry - ((R.r10 * vx + R.r11 * vy) + R.r12 * vz);
  const double ez = rz - ((R.r20 * vx + R.r21 * vy) + R.r22 * vz);
  return (ex * ex + ey * ey) + ez * ez;
}

// One pass of this lane over its frames of view v against the reference r.  weighted: w_f from e_f under Rw, else 1.
// MODE 0: acc[0..8] += w S_f, acc[9] += w, acc[10] += 1          (steps 4 and 5)
// MODE 1: acc[0] += w e_f under Rf, acc[1] += w                   (step 7)
// MODE 2: acc[0..2] += w d_f, acc[3] += w, d_f under Rf           (step 8: T)
// MODE 3: acc[0] += w |d_f - T|^2, acc[1] += w                    (step 8: trans_rms)
template <int MODE>
__device__ __forceinline__ void align_pass(const AlignArgs& A, int v, int r, long f0, long f1, bool weighted, const Rot3& Rw, const Rot3& Rf,
                                           double Tx, double Ty, double Tz, double (&acc)[ALIGN_SUMS]) {
  const int J = A.J, C = A.C;
#pragma unroll
  for (int k = 0; k < ALIGN_SUMS; ++k) acc[k] = 0.0;
#pragma unroll 1
  for (long f = f0 + threadIdx.x; f < f1; f += ALIGN_THREADS) {
    const long fv = (long)v * A.Ftot + f, fr = (long)r * A.Ftot + f;
    if (A.valid != nullptr && !(A.valid[fv] != 0 && A.valid[fr] != 0)) continue;
    if (MODE >= 2 && !(A.traj_ok[fv] != 0 && A.traj_ok[fr] != 0)) continue;
    const float* xv = A.poses + fv * J * C;
    const float* xr = A.poses + fr * J * C;
    const double v0x = xv[0], v0y = xv[1], v0z = xv[2], r0x = xr[0], r0y = xr[1], r0z = xr[2];
    bool finite = __builtin_isfinite((v0x + v0y) + v0z) && __builtin_isfinite((r0x + r0y) + r0z);   // (a sum of float32 values in fp64 cannot overflow)
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0, s4 = 0.0, s5 = 0.0, s6 = 0.0, s7 = 0.0, s8 = 0.0, ew = 0.0, ef = 0.0;
#pragma unroll 1
    for (int j = 1; j < J; ++j) {                                       // (joint 0: b = 0 exactly, it adds nothing)
      const double ax = xv[j * C], ay = xv[j * C + 1], az = xv[j * C + 2];
      const double cx = xr[j * C], cy = xr[j * C + 1], cz = xr[j * C + 2];
      finite = finite && __builtin_isfinite((ax + ay) + az) && __builtin_isfinite((cx + cy) + cz);
      const double vx = ax - v0x, vy = ay - v0y, vz = az - v0z, rx = cx - r0x, ry = cy - r0y, rz = cz - r0z;
      if (weighted) ew += align_res2(Rw, vx, vy, vz, rx, ry, rz);
      if (MODE == 0) {
        s0 += vx * rx; s1 += vx * ry; s2 += vx * rz;
        s3 += vy * rx; s4 += vy * ry; s5 += vy * rz;
        s6 += vz * rx; s7 += vz * ry; s8 += vz * rz;
      }
      if (MODE == 1) ef += align_res2(Rf, vx, vy, vz, rx, ry, rz);
    }
    if (!finite) continue;
    double w = 1.0;
    if (weighted) {
      const double t = 1.0 + (ew / (double)J) / A.sigma2;
      w = 1.0 / (t * t);
    }
    if (MODE == 0) {
      acc[0] += w * s0; acc[1] += w * s1; acc[2] += w * s2;
      acc[3] += w * s3; acc[4] += w * s4; acc[5] += w * s5;
      acc[6] += w * s6; acc[7] += w * s7; acc[8] += w * s8;
      acc[9] += w;
      acc[10] += 1.0;
    }
    if (MODE == 1) {
      acc[0] += w * (ef / (double)J);
      acc[1] += w;
    }
    if (MODE >= 2) {
      const float* tv = A.traj + fv * 3;
      const float* tr = A.traj + fr * 3;
      const double px = tv[0], py = tv[1], pz = tv[2];
      const double dx = (double)tr[0] - ((Rf.r00 * px + Rf.r01 * py) + Rf.r02 * pz);
      const double dy = (double)tr[1] - ((Rf.r10 * px + Rf.r11 * py) + Rf.r12 * pz);
      const double dz = (double)tr[2] - ((Rf.r20 * px + Rf.r21 * py) + Rf.r22 * pz);
      if (MODE == 2) {
        acc[0] += w * dx; acc[1] += w * dy; acc[2] += w * dz;
        acc[3] += w;
      } else {
        const double ux = dx - Tx, uy = dy - Ty, uz = dz - Tz;
        acc[0] += w * ((ux * ux + uy * uy) + uz * uz);
        acc[1] += w;
      }
    }
  }
}

// the row of (take, view): lane 0 of the workgroup stores it
__device__ __forceinline__ void align_store(const AlignArgs& A, long row, const double (&q)[4], double Tx, double Ty, double Tz, double rms, double trms,
                                            int used, int ok) {
  if (threadIdx.x != 0) return;
  A.quat[row * 4] = (float)q[0]; A.quat[row * 4 + 1] = (float)q[1]; A.quat[row * 4 + 2] = (float)q[2]; A.quat[row * 4 + 3] = (float)q[3];
  if (A.trans != nullptr) { A.trans[row * 3] = (float)Tx; A.trans[row * 3 + 1] = (float)Ty; A.trans[row * 3 + 2] = (float)Tz; }
  A.rms[row] = (float)rms;
  if (A.trans_rms != nullptr) A.trans_rms[row] = (float)trms;
  A.used[row] = used;
  A.ok[row] = (unsigned char)ok;
}

__global__ __launch_bounds__(ALIGN_THREADS) void lift_align_kernel(AlignArgs A) {
  __shared__ double lds[ALIGN_WAVES * ALIGN_SUMS];
  const int V = A.V;
  const int g = (int)(blockIdx.x / V), v = (int)(blockIdx.x % V);
  const long row = blockIdx.x;
  const FrameRange fr = lift_seq_frames(A.take_offset, g, A.Ftot);
  const double unit[4] = {1.0, 0.0, 0.0, 0.0};
  double acc[ALIGN_SUMS];

  // 2. the reference view: the valid frames of every view of the take, counted
#pragma unroll
  for (int k = 0; k < ALIGN_SUMS; ++k) acc[k] = 0.0;
#pragma unroll 1
  for (long f = fr.f0 + threadIdx.x; f < fr.f1; f += ALIGN_THREADS) {
#pragma unroll
    for (int u = 0; u < ALIGN_MAXV; ++u)
      if (u < V && (A.valid == nullptr || A.valid[(long)u * A.Ftot + f] != 0)) acc[u] += 1.0;
  }
  align_reduce(acc, lds);
  int r = -1, rcount = 0;
#pragma unroll
  for (int u = ALIGN_MAXV - 1; u >= 0; --u)
    if (acc[u] > 0.0) { r = u; rcount = (int)acc[u]; }
  if (r < 0) { align_store(A, row, unit, 0.0, 0.0, 0.0, 0.0, 0.0, 0, 0); return; }           // (uniform: every lane holds the same sums)
  if (v == r) { align_store(A, row, unit, 0.0, 0.0, 0.0, 0.0, 0.0, rcount, 1); return; }

  // 4., 5. the rotation
  Rot3 Rw = lift_rot3(1.0, 0.0, 0.0, 0.0), Rf = Rw;
  double q[4], lam1 = 0.0, lam2 = 0.0;
  align_pass<0>(A, v, r, fr.f0, fr.f1, false, Rw, Rf, 0.0, 0.0, 0.0, acc);
  align_reduce(acc, lds);
  const int used = (int)acc[10];
  bool good = used > 0 && align_solve(acc, q, lam1, lam2);
#pragma unroll 1
  for (int it = 0; good && it < A.iters; ++it) {
    Rw = lift_rot3(q[0], q[1], q[2], q[3]);
    align_pass<0>(A, v, r, fr.f0, fr.f1, true, Rw, Rf, 0.0, 0.0, 0.0, acc);
    align_reduce(acc, lds);
    good = align_solve(acc, q, lam1, lam2);
  }
  if (good && (lam1 - lam2) <= ALIGN_GAP * fabs(lam1)) good = false;
  if (!good) { align_store(A, row, unit, 0.0, 0.0, 0.0, 0.0, 0.0, used, 0); return; }

  // 7. the residual at the final q under the weights of the last solve
  const bool weighted = A.iters > 0;
  Rf = lift_rot3(q[0], q[1], q[2], q[3]);
  align_pass<1>(A, v, r, fr.f0, fr.f1, weighted, Rw, Rf, 0.0, 0.0, 0.0, acc);
  align_reduce(acc, lds);
  const double rms = sqrt(acc[0] / acc[1]);

  // 8. the translation
  double Tx = 0.0, Ty = 0.0, Tz = 0.0, trms = 0.0;
  int ok = 1;
  if (A.traj != nullptr) {
    align_pass<2>(A, v, r, fr.f0, fr.f1, weighted, Rw, Rf, 0.0, 0.0, 0.0, acc);
    align_reduce(acc, lds);
    const double sw = acc[3];
    const double tx = acc[0] / sw, ty = acc[1] / sw, tz = acc[2] / sw;
    if (sw > 0.0 && __builtin_isfinite(sw) && __builtin_isfinite((tx + ty) + tz)) {
      align_pass<3>(A, v, r, fr.f0, fr.f1, weighted, Rw, Rf, tx, ty, tz, acc);
      align_reduce(acc, lds);
      const double t2 = acc[0] / acc[1];
      if (__builtin_isfinite(t2)) { Tx = tx; Ty = ty; Tz = tz; trms = sqrt(t2); ok = 3; }
    }
  }
  align_store(A, row, q, Tx, Ty, Tz, rms, trms, used, ok);
}

}  // namespace mp
using namespace mp;

extern "C" {

int mp_lift_align_views(const float* poses, int V, int64_t Ftot, int J, int C, const uint8_t* valid, const int64_t* take_offset, int G,
                        const float* traj, const uint8_t* traj_ok, float sigma, int iters, float* quat, float* trans, float* rms, float* trans_rms,
                        int32_t* used, uint8_t* ok, void* stream) {
  static_assert(sizeof(long) == sizeof(int64_t), "LP64");
  MP_CHECK(poses && take_offset && quat && rms && used && ok, MP_ERR_ARG, "mp_lift_align_views: null pointer");
  if (int rc = lift_take_shape("mp_lift_align_views", V, (long)Ftot, J, G)) return rc;
  MP_CHECK(C == 3 || C == 4, MP_ERR_ARG, "mp_lift_align_views: C=%d (3: poses, 4: hypotheses with their score)", C);
  MP_CHECK(Ftot <= 0x7fffffffL, MP_ERR_ARG, "mp_lift_align_views: Ftot=%ld G=%d out of range", (long)Ftot, G);
  MP_CHECK((long)G * V <= 0x7fffffffL, MP_ERR_ARG, "mp_lift_align_views: G=%d takes of %d views: too many for one launch", G, V);
  MP_CHECK(sigma > 0.f, MP_ERR_ARG, "mp_lift_align_views: sigma=%g must be > 0 (inf: every weight is 1)", (double)sigma);
  MP_CHECK(iters >= 0 && iters <= MP_LIFT_ALIGN_MAXITERS, MP_ERR_ARG, "mp_lift_align_views: iters=%d outside 0..%d", iters, MP_LIFT_ALIGN_MAXITERS);
  MP_CHECK((traj == nullptr) == (traj_ok == nullptr), MP_ERR_ARG, "mp_lift_align_views: traj and traj_ok come together");
  MP_CHECK(traj == nullptr || (trans != nullptr && trans_rms != nullptr), MP_ERR_ARG, "mp_lift_align_views: traj given, trans or trans_rms null");
  AlignArgs a = {};
  a.poses = poses; a.valid = valid; a.take_offset = (const long*)take_offset; a.traj = traj; a.traj_ok = traj_ok;
  a.quat = quat; a.trans = trans; a.rms = rms; a.trans_rms = trans_rms; a.used = used; a.ok = ok;
  a.Ftot = (long)Ftot; a.sigma2 = (double)sigma * (double)sigma;
  a.V = V; a.J = J; a.C = C; a.G = G; a.iters = iters;
  hipLaunchKernelGGL(lift_align_kernel, dim3((unsigned)((long)G * V)), dim3(ALIGN_THREADS), 0, (hipStream_t)stream, a);
  MP_LAUNCH_CHECK();
  return MP_OK;
}

}  // extern "C"

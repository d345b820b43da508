// The geometry the multi-view lifting kernels share (lift_place.hip, lift_fuse.hip, lift_fuse_path.hip, lift_align.hip, lift_bundle.hip,
// lift_calibrate.hip, lift_score.hip): a camera's rotation from its quaternion and the test whether a take's quaternion is usable, the H36M camera model with its
// analytic Jacobian, the Gauss-Newton sums with their 3x3 solve by cofactors and accept rule, and the cyclic Jacobi on a symmetric 4x4.  ONE COPY:
// the camera model, the 1e-12 rules and the sweep limit change here or nowhere.  tests/golden/lift_place_bits.npz and lift_geom_bits.npz pin
// the bits of every kernel that includes this file.  (One loop keeps a copy of its own, for speed: bundle_frame_kernel's joint loop in
// lift_bundle.hip states the projection, the normal equations and the cofactor inverse itself; the reason is written there.)
// CONTRACTION: this header carries no `#pragma clang fp contract` of its own, so its code takes the mode of the file that includes it at the
// point of inclusion.  lift_place.hip and lift_fuse.hip compile with the default (fused multiply-adds); lift_fuse_path.hip, lift_align.hip,
// lift_bundle.hip, lift_calibrate.hip and lift_score.hip state `#pragma clang fp contract(off)` and MUST include this header AFTER that line - included before it,
// the shared code would fuse and their bits would move.
// Everything is fp64 and __device__ __forceinline__; nothing is indexed at run time (every array below is indexed by unrolled constants).
#pragma once
#include "lift_common.h"
#include "../../include/manipose_hip.h"

namespace mp {

constexpr int LIFT_EIG4_SWEEPS = 30;             // Jacobi sweeps at most (quadratic convergence: 6 to 8 in practice)

// ---- rotation --------------------------------------------------------------------------------------------------------------------------------
struct Rot3 { double r00, r01, r02, r10, r11, r12, r20, r21, r22; };

// the matrix of the unit quaternion (w, x, y, z)
__device__ __forceinline__ Rot3 lift_rot3(double w, double x, double y, double z) {
  Rot3 R;
  R.r00 = 1.0 - 2.0 * (y * y + z * z); R.r01 = 2.0 * (x * y - w * z);       R.r02 = 2.0 * (x * z + w * y);
  R.r10 = 2.0 * (x * y + w * z);       R.r11 = 1.0 - 2.0 * (x * x + z * z); R.r12 = 2.0 * (y * z - w * x);
  R.r20 = 2.0 * (x * z - w * y);       R.r21 = 2.0 * (y * z + w * x);       R.r22 = 1.0 - 2.0 * (x * x + y * y);
  return R;
}

// is a take's float32 quaternion usable: n2 = |q|^2 in fp64 is finite and >= 1e-12
__device__ __forceinline__ bool lift_quat_ok(const float* q, double& n2) {
  const double w = q[0], x = q[1], y = q[2], z = q[3];
  n2 = w * w + x * x + y * y + z * z;
  return __builtin_isfinite(n2) && n2 >= 1e-12;
}
__device__ __forceinline__ bool lift_quat_ok(const float* q) {
  double n2;
  return lift_quat_ok(q, n2);
}

// the matrix of q / |q|, normalised in fp64; false (and the identity) where q fails lift_quat_ok; q null: the identity
__device__ __forceinline__ bool lift_rot3(const float* q, Rot3& R) {
  R = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
  if (q == nullptr) return true;
  double n2;
  if (!lift_quat_ok(q, n2)) return false;
  const double n = sqrt(n2);
  R = lift_rot3((double)q[0] / n, (double)q[1] / n, (double)q[2] / n, (double)q[3] / n);
  return true;
}

// view v of frame f of take g counts: its byte of valid (V, Ftot) and its take's quaternion in quat (G, V, 4); either table may be null
__device__ __forceinline__ bool lift_view_ok(const unsigned char* valid, const float* quat, int V, long Ftot, long f, int g, int v) {
  bool good = valid == nullptr || valid[(long)v * Ftot + f] != 0;
  if (good && quat != nullptr) good = lift_quat_ok(quat + ((long)g * V + v) * 4);
  return good;
}

// bit v: view v of frame f counts
__device__ __forceinline__ int lift_view_mask(const unsigned char* valid, const float* quat, int V, long Ftot, long f, int g) {
  int mask = 0;
  for (int v = 0; v < V; ++v)
    if (lift_view_ok(valid, quat, V, Ftot, f, g, v)) mask |= 1 << v;
  return mask;
}

// ---- the camera model ------------------------------------------------------------------------------------------------------------------------
// torch.clamp(x, -1, 1): a NaN stays a NaN
__device__ __forceinline__ double lift_clamp1(double x) { return x < -1.0 ? -1.0 : (x > 1.0 ? 1.0 : x); }

struct LiftCam { double fx, fy, cx, cy, k1, k2, k3, p1, p2; };
__device__ __forceinline__ LiftCam lift_cam(const float* c) { return {c[0], c[1], c[2], c[3], c[4], c[5], c[6], c[7], c[8]}; }

// the residual (du, dv) of a joint and, with JAC, c = d(du, dv) / d(X, Y, Z); without it c stays zero
struct LiftProj { double du, dv, c00, c01, c02, c10, c11, c12; };

// The camera-space point (X, Y, Z) against its keypoint U (2 floats): perspective divide, clamp to +-1, with `distort` the radial and tangential
// terms (the reference's project_to_2d; without: project_to_2d_linear), focal length and centre.  The caller judges Z > 0.
template <bool JAC>
__device__ __forceinline__ LiftProj lift_project(double X, double Y, double Z, const float* U, const LiftCam& cam, int distort) {
  const double fx = cam.fx, fy = cam.fy, cx = cam.cx, cy = cam.cy, k1 = cam.k1, k2 = cam.k2, k3 = cam.k3, p1 = cam.p1, p2 = cam.p2;
  const double qx = X / Z, qy = Y / Z;
  const double xx = lift_clamp1(qx), yy = lift_clamp1(qy);
  double px = xx, py = yy;
  double a = 1.0, b = 0.0, c = 0.0, d = 1.0;                            // d(px, py) / d(x, y)
  if (distort) {
    const double r2 = xx * xx + yy * yy;
    const double m = 1.0 + (k1 * r2 + k2 * (r2 * r2) + k3 * (r2 * r2 * r2)) + (p1 * xx + p2 * yy);
    px = xx * m + p1 * r2;
    py = yy * m + p2 * r2;
    if (JAC) {
      const double dm = k1 + 2.0 * k2 * r2 + 3.0 * k3 * (r2 * r2);
      const double mx = 2.0 * xx * dm + p1, my = 2.0 * yy * dm + p2;
      a = m + xx * mx + 2.0 * p1 * xx;
      b = xx * my + 2.0 * p1 * yy;
      c = yy * mx + 2.0 * p2 * xx;
      d = m + yy * my + 2.0 * p2 * yy;
    }
  }
  LiftProj r = {};
  r.du = fx * px + cx - (double)U[0];
  r.dv = fy * py + cy - (double)U[1];
  if (JAC) {
    const double sx = (qx >= -1.0 && qx <= 1.0) ? 1.0 : 0.0, sy = (qy >= -1.0 && qy <= 1.0) ? 1.0 : 0.0;   // the derivative of the clamp
    const double iz = 1.0 / Z;
    const double xz = sx * iz, yz = sy * iz, xq = sx * (-qx / Z), yq = sy * (-qy / Z);   // dx/dP = (xz, 0, xq), dy/dP = (0, yz, yq)
    r.c00 = fx * (a * xz); r.c01 = fx * (b * yz); r.c02 = fx * (a * xq + b * yq);
    r.c10 = fy * (c * xz); r.c11 = fy * (d * yz); r.c12 = fy * (c * xq + d * yq);
  }
  return r;
}

// ---- Gauss-Newton on three unknowns ------------------------------------------------------------------------------------------------------------
// H = sum w J^T J (upper triangle) and g = sum w J^T r of 2 x 3 Jacobians J and residuals r
struct LiftNormal3 { double H00, H01, H02, H11, H12, H22, g0, g1, g2; };

// one term: weight w, residual (du, dv), Jacobian rows (j00, j01, j02) and (j10, j11, j12)
__device__ __forceinline__ void lift_normal3_add(LiftNormal3& n, double w, double du, double dv, double j00, double j01, double j02, double j10,
                                                 double j11, double j12) {
  n.H00 += w * (j00 * j00 + j10 * j10);
  n.H01 += w * (j00 * j01 + j10 * j11);
  n.H02 += w * (j00 * j02 + j10 * j12);
  n.H11 += w * (j01 * j01 + j11 * j11);
  n.H12 += w * (j01 * j02 + j11 * j12);
  n.H22 += w * (j02 * j02 + j12 * j12);
  n.g0 += w * (j00 * du + j10 * dv);
  n.g1 += w * (j01 * du + j11 * dv);
  n.g2 += w * (j02 * du + j12 * dv);
}

// adj(H) (upper triangle) and det H of the symmetric 3x3 by cofactors
struct LiftAdj3 { double c00, c01, c02, c11, c12, c22, det; };

// false where H is degenerate - the rule of every fit here: det and H00 H11 H22 finite and det > 1e-12 H00 H11 H22
__device__ __forceinline__ bool lift_adj3(const LiftNormal3& n, LiftAdj3& a) {
  a.c00 = n.H11 * n.H22 - n.H12 * n.H12; a.c01 = n.H02 * n.H12 - n.H01 * n.H22; a.c02 = n.H01 * n.H12 - n.H02 * n.H11;
  a.det = n.H00 * a.c00 + n.H01 * a.c01 + n.H02 * a.c02;
  const double scale = n.H00 * n.H11 * n.H22;
  a.c11 = n.H00 * n.H22 - n.H02 * n.H02; a.c12 = n.H01 * n.H02 - n.H00 * n.H12; a.c22 = n.H00 * n.H11 - n.H01 * n.H01;
  return __builtin_isfinite(a.det) && __builtin_isfinite(scale) && a.det > 1e-12 * scale;
}

// x = adj(H) g / det
__device__ __forceinline__ void lift_adj3_solve(const LiftAdj3& a, double g0, double g1, double g2, double& x0, double& x1, double& x2) {
  x0 = (a.c00 * g0 + a.c01 * g1 + a.c02 * g2) / a.det;
  x1 = (a.c01 * g0 + a.c11 * g1 + a.c12 * g2) / a.det;
  x2 = (a.c02 * g0 + a.c12 * g1 + a.c22 * g2) / a.det;
}

// what one pass over the weighted joints at a translation gives: F = sum w |r|^2, E = sum w |r|, W = sum w, the normal equations,
// deep = every weighted Z > 0
struct LiftGN {
  double F, E, W;
  LiftNormal3 n;
  bool deep;
};
__device__ __forceinline__ LiftGN lift_gn_start() {
  LiftGN e = {};
  e.deep = true;
  return e;
}

// a joint of weight w: its projection pr and the rows of its Jacobian with respect to the unknown (JAC = false leaves H and g at zero)
template <bool JAC>
__device__ __forceinline__ void lift_gn_add(LiftGN& e, double w, const LiftProj& pr, double j00, double j01, double j02, double j10, double j11,
                                            double j12) {
  const double rr = pr.du * pr.du + pr.dv * pr.dv;
  e.W += w;
  e.E += w * sqrt(rr);
  e.F += w * rr;
  if (JAC) lift_normal3_add(e.n, w, pr.du, pr.dv, j00, j01, j02, j10, j11, j12);
}

// the undamped step from t: t - adj(H) g / det; false where H is degenerate or the step is not finite
__device__ __forceinline__ bool lift_gn_step(const LiftGN& e, double tx, double ty, double tz, double& nx, double& ny, double& nz) {
  LiftAdj3 a;
  if (!lift_adj3(e.n, a)) return false;
  double d0, d1, d2;
  lift_adj3_solve(a, e.n.g0, e.n.g1, e.n.g2, d0, d1, d2);
  nx = tx - d0; ny = ty - d1; nz = tz - d2;
  return __builtin_isfinite(nx) && __builtin_isfinite(ny) && __builtin_isfinite(nz);
}

// the step from e to n is taken: every weighted joint in front of its camera, the cost not above (1 + 1e-6) times the one before
// (a NaN cost is not taken either)
__device__ __forceinline__ bool lift_gn_accept(const LiftGN& n, const LiftGN& e) { return n.deep && n.F <= (1.0 + 1e-6) * e.F; }

// ---- the symmetric 4x4 eigenproblem ----------------------------------------------------------------------------------------------------------
// the two largest eigenvalues lam1 >= lam2 of a symmetric 4x4 matrix and the eigenvector q of lam1: cyclic Jacobi sweeps until
// off(A) <= 2^-52 |A|_F.  a is overwritten.
__device__ __forceinline__ void lift_eig4(double (&a)[4][4], double (&q)[4], double& lam1, double& lam2) {
  double v[4][4] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}, {0, 0, 0, 1}};
#pragma unroll 1
  for (int sweep = 0; sweep < LIFT_EIG4_SWEEPS; ++sweep) {
    double off2 = 0.0, diag2 = 0.0;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      diag2 += a[p][p] * a[p][p];
#pragma unroll
      for (int r = p + 1; r < 4; ++r) off2 += 2.0 * (a[p][r] * a[p][r]);
    }
    if (off2 <= 0x1p-104 * (off2 + diag2)) break;
#pragma unroll
    for (int p = 0; p < 3; ++p)
#pragma unroll
      for (int r = p + 1; r < 4; ++r) {
        // (no branch: a pair that needs no rotation, or whose theta overflows, gets t = 0, c = 1, s = 0, which leaves every entry's bits alone)
        const double apq = a[p][r];
        const double theta = (a[r][r] - a[p][p]) / (2.0 * apq);
        const double t = apq != 0.0 ? copysign(1.0, theta) / (fabs(theta) + sqrt(theta * theta + 1.0)) : 0.0;
        const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
        for (int k = 0; k < 4; ++k) {            // A <- A J (columns p, r)
          const double akp = a[k][p], akr = a[k][r];
          a[k][p] = c * akp - s * akr;
          a[k][r] = s * akp + c * akr;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {            // A <- J^T A (rows p, r)
          const double apk = a[p][k], ark = a[r][k];
          a[p][k] = c * apk - s * ark;
          a[r][k] = s * apk + c * ark;
        }
        a[p][r] = a[r][p] = t != 0.0 ? 0.0 : a[p][r];   // (what the rotation was built for)
#pragma unroll
        for (int k = 0; k < 4; ++k) {            // V <- V J
          const double vkp = v[k][p], vkr = v[k][r];
          v[k][p] = c * vkp - s * vkr;
          v[k][r] = s * vkp + c * vkr;
        }
      }
  }
  int best = 0;
  lam1 = a[0][0];
#pragma unroll
  for (int k = 1; k < 4; ++k)
    if (a[k][k] > lam1) { lam1 = a[k][k]; best = k; }
  lam2 = -__builtin_inf();
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (k != best && a[k][k] > lam2) lam2 = a[k][k];
#pragma unroll
  for (int k = 0; k < 4; ++k) q[k] = best == 0 ? v[k][0] : best == 1 ? v[k][1] : best == 2 ? v[k][2] : v[k][3];
}

// ---- host ------------------------------------------------------------------------------------------------------------------------------------
// the shape every multi-view entry point checks: V views of Ftot frames of J joints in G takes
static int lift_take_shape(const char* who, int V, long Ftot, int J, int G) {
  MP_CHECK(V >= 1 && V <= MP_LIFT_FUSE_MAXV, MP_ERR_ARG, "%s: V=%d outside 1..%d", who, V, MP_LIFT_FUSE_MAXV);
  MP_CHECK(J >= 2 && J <= LIFT_MAXJ, MP_ERR_ARG, "%s: J=%d outside 2..%d", who, J, LIFT_MAXJ);
  MP_CHECK(Ftot > 0 && G > 0 && (long)G <= Ftot, MP_ERR_ARG, "%s: Ftot=%ld G=%d out of range", who, Ftot, G);
  return MP_OK;
}

}  // namespace mp

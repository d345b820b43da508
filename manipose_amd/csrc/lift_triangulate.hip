// Triangulating a fused take's joints on the 2-D keypoints (include/manipose_hip.h: mp_lift_triangulate has the rule).  mp_lift_fuse gives a take's
// body as the mean of one lifted hypothesis per view and mp_lift_fuse_place one world root per frame: the keypoints - the only measured quantity -
// decide three numbers per frame.  Here every joint of every frame is a world point of its own, seen by up to 4 calibrated cameras: the linear
// pinhole triangulation over its observations as a start (the fused pose plus root where fewer than two cameras see the joint, or the linear
// system is degenerate), then undamped Gauss-Newton steps on the robust reprojection error under the full camera model, with an optional pull
// towards the fused pose plus root.  tests/lift_triangulate_ref.py states the rule in float64.
//
// ONE LANE OWNS ONE (frame, joint) ITEM, items in f * J + j order: consecutive lanes store consecutive floats of points, err, views, ok, steps.
// A view's rotation matrix is re-made from its quaternion at the head of every pass, as lift_fuse_place_kernel does, and its weight and keypoint
// are loaded again (a cache hit), so nothing sits in a register array at all; the view loops are unrolled to MP_LIFT_FUSE_MAXV.  One loop holds
// the start, the restart and the steps, so the evaluation - four views of a projection with its Jacobian - is in the kernel once.  The rotation,
// the view test, the projection with its Jacobian, the normal equations, the 3x3 solve by cofactors and the accept rule are lift_geom.h's.
// Everything between the float32 loads and the float32 stores is fp64, without contraction; no atomics, fixed orders: identical bits on every call.
#include "lift_common.h"

#pragma clang fp contract(off)
#include "lift_geom.h"                    // after the pragma: the shared code takes this file's mode

namespace mp {

constexpr int TRI_MAXV = MP_LIFT_FUSE_MAXV;
constexpr int TRI_THREADS = 64;                // lanes of a workgroup: one wave, as lift_fuse_place_kernel

struct TriArgs {
  const float* pose;             // (Ftot, J, 3)
  const float* root;             // (Ftot, 3)
  const unsigned char* root_ok;  // (Ftot) or null
  const float* kp;               // (V, Ftot, J, 2)
  const float* kp_weight;        // (V, Ftot, J) or null
  const unsigned char* valid;    // (V, Ftot) or null
  const long* take_offset;       // (G + 1) device
  const float* quat;             // (G, V, 4)
  const float* trans;            // (G, V, 3)
  const float* intr;             // (G, V, 9)
  float* points;                 // (Ftot, J, 3)
  float* err;                    // (Ftot, J)
  unsigned char* views;          // (Ftot, J)
  unsigned char* ok;             // (Ftot, J)
  unsigned char* steps;          // (Ftot, J) or null
  long Ftot;
  double sigma2, prior;
  int V, J, G, distort, iters;
};

// 4. of the rule at the world point (x, y, z): the sums over the observations in view order, then the prior's terms
template <bool JAC>
__device__ __forceinline__ LiftGN tri_eval(const TriArgs& A, long f, int j, int g, int mask, double x, double y, double z, bool pull, double x0,
                                           double y0, double z0) {
  LiftGN e = lift_gn_start();
#pragma unroll
  for (int v = 0; v < TRI_MAXV; ++v) {
    if (!((mask >> v) & 1)) continue;                                   // (mask holds no bit at or above V)
    const long gv = (long)g * A.V + v;
    const long o = ((long)v * A.Ftot + f) * A.J + j;
    Rot3 R;
    lift_rot3(A.quat + gv * 4, R);
    const LiftCam K = lift_cam(A.intr + gv * 9);
    const float* T = A.trans + gv * 3;
    const double w = A.kp_weight != nullptr ? (double)A.kp_weight[o] : 1.0;
    const double wx = x - (double)T[0], wy = y - (double)T[1], wz = z - (double)T[2];
    const double X = R.r00 * wx + R.r10 * wy + R.r20 * wz, Y = R.r01 * wx + R.r11 * wy + R.r21 * wz, Z = R.r02 * wx + R.r12 * wy + R.r22 * wz;
    if (!(Z > 0.0)) e.deep = false;
    const LiftProj pr = lift_project<JAC>(X, Y, Z, A.kp + o * 2, K, A.distort);
    const double ee = pr.du * pr.du + pr.dv * pr.dv;
    const double t = 1.0 + ee / A.sigma2;                               // (sigma = +inf: exactly 1)
    e.W += w;
    e.E += w * sqrt(ee);
    e.F += w * (ee / t);
    if (JAC) {
      const double wt = w * (1.0 / (t * t));
      const double j00 = pr.c00 * R.r00 + pr.c01 * R.r01 + pr.c02 * R.r02, j01 = pr.c00 * R.r10 + pr.c01 * R.r11 + pr.c02 * R.r12,
                   j02 = pr.c00 * R.r20 + pr.c01 * R.r21 + pr.c02 * R.r22;                                // J_pi R^T: with respect to the world point
      const double j10 = pr.c10 * R.r00 + pr.c11 * R.r01 + pr.c12 * R.r02, j11 = pr.c10 * R.r10 + pr.c11 * R.r11 + pr.c12 * R.r12,
                   j12 = pr.c10 * R.r20 + pr.c11 * R.r21 + pr.c12 * R.r22;
      lift_normal3_add(e.n, wt, pr.du, pr.dv, j00, j01, j02, j10, j11, j12);
    }
  }
  if (pull) {
    const double dx = x - x0, dy = y - y0, dz = z - z0;
    e.F += A.prior * ((dx * dx + dy * dy) + dz * dz);
    if (JAC) {
      e.n.H00 += A.prior; e.n.H11 += A.prior; e.n.H22 += A.prior;
      e.n.g0 += A.prior * dx; e.n.g1 += A.prior * dy; e.n.g2 += A.prior * dz;
    }
  }
  return e;
}

// JAC = false: the launch of iters = 0, which takes no step and needs no Jacobian (F, E, W and deep have the same bits either way)
template <bool JAC>
__global__ __launch_bounds__(TRI_THREADS) void lift_triangulate_kernel(TriArgs A) {
  const long item = (long)blockIdx.x * TRI_THREADS + threadIdx.x;
  if (item >= A.Ftot * A.J) return;
  const long f = item / A.J;
  const int j = (int)(item - f * A.J);
  const int g = lift_seq_of(A.take_offset, A.G, f);
  const FrameRange fr = lift_seq_frames(A.take_offset, g, A.Ftot);
  if (f < fr.f0 || f >= fr.f1) return;                                  // a frame no take holds is left unwritten
  // 1. the prior point
  const float* P = A.pose + item * 3;
  const float* r = A.root + f * 3;
  const double x0 = (double)P[0] + (double)r[0], y0 = (double)P[1] + (double)r[1], z0 = (double)P[2] + (double)r[2];
  const bool usable = (A.root_ok == nullptr || A.root_ok[f] != 0) && __builtin_isfinite(x0) && __builtin_isfinite(y0) && __builtin_isfinite(z0);
  const bool pull = A.prior > 0.0 && usable;
  // 2. the observations, 3. the linear start over them
  int mask = 0, n = 0;
  LiftNormal3 lin = {};
#pragma unroll
  for (int v = 0; v < TRI_MAXV; ++v) {
    if (v >= A.V || !lift_view_ok(A.valid, A.quat, A.V, A.Ftot, f, g, v)) continue;      // an invalid view's data is never looked at
    const long gv = (long)g * A.V + v;
    const long o = ((long)v * A.Ftot + f) * A.J + j;
    const double ku = A.kp[o * 2], kv = A.kp[o * 2 + 1];
    const double w = A.kp_weight != nullptr ? (double)A.kp_weight[o] : 1.0;
    if (!(__builtin_isfinite(ku) && __builtin_isfinite(kv) && __builtin_isfinite(w) && w > 0.0)) continue;
    mask |= 1 << v;
    ++n;
    Rot3 R;
    lift_rot3(A.quat + gv * 4, R);
    const float* cam = A.intr + gv * 9;
    const float* T = A.trans + gv * 3;
    const double fx = cam[0], fy = cam[1], cx = cam[2], cy = cam[3], Tx = T[0], Ty = T[1], Tz = T[2];
    const double a = (ku - cx) / fx, b = (kv - cy) / fy;
    // rows of R^T are columns of R: rho_x = (r00, r10, r20), rho_y = (r01, r11, r21), rho_z = (r02, r12, r22)
    const double mx0 = R.r00 - a * R.r02, mx1 = R.r10 - a * R.r12, mx2 = R.r20 - a * R.r22;
    const double my0 = R.r01 - b * R.r02, my1 = R.r11 - b * R.r12, my2 = R.r21 - b * R.r22;
    const double sx = mx0 * Tx + mx1 * Ty + mx2 * Tz, sy = my0 * Tx + my1 * Ty + my2 * Tz;
    lift_normal3_add(lin, w, sx, sy, mx0, mx1, mx2, my0, my1, my2);
  }
  double cx = x0, cy = y0, cz = z0;                                     // the candidate: the point the next pass evaluates
  bool tri = false;
  if (n >= 2) {
    LiftAdj3 adj;
    if (lift_adj3(lin, adj)) {
      double tx, ty, tz;
      lift_adj3_solve(adj, lin.g0, lin.g1, lin.g2, tx, ty, tz);
      if (__builtin_isfinite(tx) && __builtin_isfinite(ty) && __builtin_isfinite(tz)) { cx = tx; cy = ty; cz = tz; tri = true; }
    }
  }
  // 4., 5. one loop: the start, once more from the prior point where the triangulated start is behind a camera, then the steps
  double x = 0.0, y = 0.0, z = 0.0;
  LiftGN e = lift_gn_start();
  bool have = false;
  unsigned char taken = 0;
  if (tri || usable) {
#pragma unroll 1
    for (;;) {
      const LiftGN c = tri_eval<JAC>(A, f, j, g, mask, cx, cy, cz, pull, x0, y0, z0);
      if (!have) {
        if (!c.deep && tri && usable) { cx = x0; cy = y0; cz = z0; tri = false; continue; }
        if (!(c.deep && __builtin_isfinite(c.F))) { tri = false; break; }
        have = true;
      } else {
        if (!lift_gn_accept(c, e)) break;
        ++taken;
      }
      x = cx; y = cy; z = cz; e = c;
      if ((int)taken >= A.iters) break;
      if (!lift_gn_step(e, x, y, z, cx, cy, cz)) break;
    }
  }
  // 6.
  A.points[item * 3] = (float)x; A.points[item * 3 + 1] = (float)y; A.points[item * 3 + 2] = (float)z;
  A.err[item] = (have && n > 0) ? (float)(e.E / e.W) : 0.f;
  A.views[item] = (unsigned char)mask;
  A.ok[item] = have ? (unsigned char)(1 | (tri ? 2 : 0)) : (unsigned char)0;
  if (A.steps != nullptr) A.steps[item] = taken;
}

}  // namespace mp
using namespace mp;

extern "C" {

int mp_lift_triangulate(const float* pose, const float* root, const uint8_t* root_ok, const float* kp, const float* kp_weight, int V, int64_t Ftot,
                        int J, const uint8_t* valid, const int64_t* take_offset, int G, const float* quat, const float* trans, const float* intr,
                        int distort, float sigma, float prior, int iters, float* points, float* err, uint8_t* views, uint8_t* ok, uint8_t* steps,
                        void* stream) {
  static_assert(sizeof(long) == sizeof(int64_t), "LP64");
  MP_CHECK(pose && root && kp && take_offset && quat && trans && intr, MP_ERR_ARG, "mp_lift_triangulate: null input");
  MP_CHECK(points && err && views && ok, MP_ERR_ARG, "mp_lift_triangulate: null output");
  if (int rc = lift_take_shape("mp_lift_triangulate", V, (long)Ftot, J, G)) return rc;
  MP_CHECK(distort == 0 || distort == 1, MP_ERR_ARG, "mp_lift_triangulate: distort=%d (0: project_to_2d_linear, 1: project_to_2d)", distort);
  MP_CHECK(iters >= 0 && iters <= MP_LIFT_REFINE_MAXITERS, MP_ERR_ARG, "mp_lift_triangulate: iters=%d outside 0..%d", iters, MP_LIFT_REFINE_MAXITERS);
  MP_CHECK(sigma > 0.f, MP_ERR_ARG, "mp_lift_triangulate: sigma=%g must be > 0 (inf: every robust factor is 1)", (double)sigma);
  MP_CHECK(prior >= 0.f && __builtin_isfinite(prior), MP_ERR_ARG, "mp_lift_triangulate: prior=%g must be finite and >= 0", (double)prior);
  MP_CHECK((long)Ftot <= 0x7fffffffL * (long)TRI_THREADS / J, MP_ERR_ARG, "mp_lift_triangulate: %ld frames of %d joints: too many for one launch",
           (long)Ftot, J);
  const long blocks = ((long)Ftot * J + TRI_THREADS - 1) / TRI_THREADS;
  MP_CHECK(blocks <= 0x7fffffffL, MP_ERR_ARG, "mp_lift_triangulate: %ld items: too many for one launch", (long)Ftot * J);
  TriArgs a = {};
  a.pose = pose; a.root = root; a.root_ok = root_ok; a.kp = kp; a.kp_weight = kp_weight; a.valid = valid; a.take_offset = (const long*)take_offset;
  a.quat = quat; a.trans = trans; a.intr = intr; a.points = points; a.err = err; a.views = views; a.ok = ok; a.steps = steps;
  a.Ftot = (long)Ftot; a.sigma2 = (double)sigma * (double)sigma; a.prior = (double)prior;
  a.V = V; a.J = J; a.G = G; a.distort = distort; a.iters = iters;
  if (iters > 0)
    hipLaunchKernelGGL(lift_triangulate_kernel<true>, dim3((unsigned)blocks), dim3(TRI_THREADS), 0, (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL(lift_triangulate_kernel<false>, dim3((unsigned)blocks), dim3(TRI_THREADS), 0, (hipStream_t)stream, a);
  MP_LAUNCH_CHECK();
  return MP_OK;
}

}  // extern "C"

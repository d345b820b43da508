// Fusing the camera views of a take (include/manipose_hip.h: mp_lift_fuse, mp_lift_fuse_place).  A take is one motion seen by up to 4 calibrated
// cameras at once; the lifting pipeline gives every view K hypotheses per frame, root-relative and in that camera's frame.  mp_lift_fuse rotates
// them into the world's orientation, chooses ONE hypothesis per view JOINTLY - the combination whose members agree best with each other, the
// scores as a prior - and emits their mean; mp_lift_fuse_place then finds the ONE world root whose projection into every view meets that view's
// 2-D keypoints: the linear pinhole fit over all views as a start, then undamped Gauss-Newton steps under the full camera model, with the rule and
// the constants of mp_lift_place_refine.  The rules are in the header; tests/lift_fuse_ref.py states them in float64.
//
// mp_lift_fuse: ONE WAVE OWNS ONE FRAME, up to FUSE_WAVES frames per workgroup, each with its own slice of dynamic LDS: the views' rotation
// matrices, the rotated hypotheses (V K J 3 doubles: 8 KB at 4 x 5 x 17), the unary costs and the cross-view pair table (at most 6 K^2 doubles).
// The lanes split the (view, hypothesis, joint) items of the rotation, then the (pair, i, l) entries of the pair table, then the K^n combinations
// (at most 4096: 64 per lane, each lane in increasing order, strict <), and a butterfly arg-min - lowest cost, then lowest combination - leaves
// every lane with the frame's choice.  The workgroup barriers are reached by every wave, whether its frame exists or not.
// mp_lift_fuse_place: ONE LANE OWNS ONE FRAME, as in lift_place_refine_kernel; a view's rotation matrix is re-made from its quaternion at the head
// of every pass (a few dozen operations against J joints of five divisions and a square root), so nothing sits in a register array indexed at
// run time.  The rotation, the view test, the per-joint projection with its Jacobian, the Gauss-Newton sums and the 3x3 solve are lift_geom.h's,
// shared with lift_place.hip: here the Jacobian is taken through R^T.
// Everything between the float32 loads and the float32 stores is fp64; no atomics, fixed orders: identical bits on every call.
#include "lift_geom.h"

namespace mp {

constexpr int FUSE_MAXV = MP_LIFT_FUSE_MAXV, FUSE_MAXK = MP_LIFT_FUSE_MAXK;
constexpr int FUSE_WAVES = 4;                  // frames of a workgroup at most (fewer where their LDS would pass 64 KB)
constexpr int FUSE_PLACE_THREADS = 64;         // lanes of a workgroup of the place kernel: one wave, as lift_place_refine_kernel
constexpr double FUSE_BIG = 1e30;              // a pair cost that is not finite
constexpr long FUSE_LDS_LIMIT = 64 * 1024;

struct FuseArgs {
  const float* hyps;             // (V, Ftot, K, J, C)
  const unsigned char* valid;    // (V, Ftot) or null
  const long* take_offset;       // (G + 1) device
  const float* quat;             // (G, V, 4) device or null
  float* pose;                   // (Ftot, J, 3)
  unsigned char* choice;         // (Ftot, V)
  float* cost;                   // (Ftot)
  float* spread;                 // (Ftot)
  unsigned char* ok;             // (Ftot)
  long Ftot;
  double pair_factor, score_weight;   // 1 / (2 sigma^2), score_weight
  int V, K, J, C, G, waves, frame_doubles;
};

// pair (a, b), a < b, in lexicographic order: its row in the pair table
__device__ __forceinline__ int fuse_pair_index(int a, int b) { return a * (2 * FUSE_MAXV - a - 1) / 2 + (b - a - 1); }

__global__ __launch_bounds__(FUSE_WAVES * 64) void lift_fuse_kernel(FuseArgs A) {
  extern __shared__ double fuse_lds[];
  const int V = A.V, K = A.K, J = A.J, C = A.C;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long f = (long)blockIdx.x * A.waves + wave;
  const bool live = f < A.Ftot;                                         // (a wave without a frame still meets the barriers)
  double* Rm = fuse_lds + (long)wave * A.frame_doubles;                 // V x 9
  double* Wr = Rm + FUSE_MAXV * 9;                                      // (V, K, J, 3) rotated hypotheses
  double* U = Wr + V * K * J * 3;                                       // (V, K) unary costs
  double* D = U + V * K;                                                // (6, K, K) pair costs
  int g = 0, mask = 0;
  if (live) {
    g = lift_seq_of(A.take_offset, A.G, f);
    mask = lift_view_mask(A.valid, A.quat, V, A.Ftot, f, g);
    if (lane < V && ((mask >> lane) & 1)) {
      Rot3 R;
      lift_rot3(A.quat != nullptr ? A.quat + ((long)g * V + lane) * 4 : nullptr, R);
      double* r = Rm + lane * 9;
      r[0] = R.r00; r[1] = R.r01; r[2] = R.r02; r[3] = R.r10; r[4] = R.r11; r[5] = R.r12; r[6] = R.r20; r[7] = R.r21; r[8] = R.r22;
    }
  }
  __syncthreads();
  if (live) {                                                           // 1. rotate, 3. unary costs
    for (int it = lane; it < V * K * J; it += 64) {
      const int v = it / (K * J), k = (it / J) % K, j = it % J;
      if (!((mask >> v) & 1)) continue;                                 // an invalid view's data is never looked at
      const float* x0 = A.hyps + (((long)v * A.Ftot + f) * K + k) * J * C;
      const float* xj = x0 + j * C;
      const double dx = (double)xj[0] - (double)x0[0], dy = (double)xj[1] - (double)x0[1], dz = (double)xj[2] - (double)x0[2];
      double* w = Wr + (long)it * 3;
      if (A.quat != nullptr) {
        const double* r = Rm + v * 9;
        w[0] = r[0] * dx + r[1] * dy + r[2] * dz;
        w[1] = r[3] * dx + r[4] * dy + r[5] * dz;
        w[2] = r[6] * dx + r[7] * dy + r[8] * dz;
      } else {
        w[0] = dx; w[1] = dy; w[2] = dz;                                // nothing is multiplied: the differences are exact
      }
      if (j == 0) {
        double u = 0.0;
        if (C == 4) {
          double s = x0[3];
          if (!(s > 1e-12)) s = 1e-12;
          u = -log(s);
        }
        U[v * K + k] = u;
      }
    }
  }
  __syncthreads();
  if (live) {                                                           // 2. pair costs
    const int KK = K * K;
    for (int it = lane; it < 6 * KK; it += 64) {
      const int p = it / KK, i = (it / K) % K, l = it % K;
      const int a = p < 3 ? 0 : (p < 5 ? 1 : 2), b = p < 3 ? p + 1 : (p < 5 ? p - 1 : 3);     // (0,1) (0,2) (0,3) (1,2) (1,3) (2,3)
      if (b >= V || !((mask >> a) & 1) || !((mask >> b) & 1)) continue;
      const double* wa = Wr + (long)(a * K + i) * J * 3;
      const double* wb = Wr + (long)(b * K + l) * J * 3;
      double s = 0.0;
      for (int j = 0; j < J; ++j) {                                     // joint order, then channel order
        const double ex = wa[j * 3] - wb[j * 3], ey = wa[j * 3 + 1] - wb[j * 3 + 1], ez = wa[j * 3 + 2] - wb[j * 3 + 2];
        s += ex * ex; s += ey * ey; s += ez * ez;
      }
      double d = s / (double)J;
      if (!__builtin_isfinite(d)) d = FUSE_BIG;
      D[it] = d;
    }
  }
  __syncthreads();
  if (!live) return;                                                    // (no barrier below)
  int n = 0, total = 1;
  for (int v = 0; v < V; ++v) if ((mask >> v) & 1) { ++n; total *= K; }
  if (n == 0) {
    for (int it = lane; it < J * 3; it += 64) A.pose[f * J * 3 + it] = 0.f;
    if (lane < V) A.choice[f * V + lane] = 255;
    if (lane == 0) { A.cost[f] = 0.f; A.spread[f] = 0.f; A.ok[f] = 0; }
    return;
  }
  // 4. the combinations: c counts through the valid views' hypotheses, view 0 most significant; this lane takes c = lane, lane + 64, ...
  double best = __builtin_inf();
  int bc = 0x7fffffff;
  for (int c = lane; c < total; c += 64) {
    int kv[FUSE_MAXV] = {0, 0, 0, 0};
    int rest = c;
#pragma unroll
    for (int v = FUSE_MAXV - 1; v >= 0; --v)
      if (v < V && ((mask >> v) & 1)) { kv[v] = rest % K; rest /= K; }
    double pairs = 0.0, unary = 0.0;
#pragma unroll
    for (int a = 0; a < FUSE_MAXV; ++a)
#pragma unroll
      for (int b = a + 1; b < FUSE_MAXV; ++b)
        if (b < V && ((mask >> a) & 1) && ((mask >> b) & 1)) pairs += D[(fuse_pair_index(a, b) * K + kv[a]) * K + kv[b]];
#pragma unroll
    for (int v = 0; v < FUSE_MAXV; ++v)
      if (v < V && ((mask >> v) & 1)) unary += U[v * K + kv[v]];
    const double E = A.pair_factor * pairs + A.score_weight * unary;
    if (bc == 0x7fffffff || E < best) { best = E; bc = c; }            // the first minimum of this lane's own, increasing c
  }
  for (int off = 32; off > 0; off >>= 1) {                              // arg-min: lowest cost, then lowest combination
    const double oe = __shfl_xor(best, off);
    const int oc = __shfl_xor(bc, off);
    if (oc != 0x7fffffff && (bc == 0x7fffffff || oe < best || (oe == best && oc < bc))) { best = oe; bc = oc; }
  }
  int kv[FUSE_MAXV] = {0, 0, 0, 0};
  {
    int rest = bc;
#pragma unroll
    for (int v = FUSE_MAXV - 1; v >= 0; --v)
      if (v < V && ((mask >> v) & 1)) { kv[v] = rest % K; rest /= K; }
  }
  // 5. the mean of the chosen hypotheses, 6. their spread about it
  double dev = 0.0;
  for (int it = lane; it < J * 3; it += 64) {
    double sum = 0.0;
#pragma unroll
    for (int v = 0; v < FUSE_MAXV; ++v)
      if (v < V && ((mask >> v) & 1)) sum += Wr[(long)(v * K + kv[v]) * J * 3 + it];
    const double mean = sum / (double)n;
#pragma unroll
    for (int v = 0; v < FUSE_MAXV; ++v)
      if (v < V && ((mask >> v) & 1)) {
        const double e = Wr[(long)(v * K + kv[v]) * J * 3 + it] - mean;
        dev += e * e;
      }
    A.pose[f * J * 3 + it] = it < 3 ? 0.f : (float)mean;                // joint 0 is stored as +0
  }
  for (int off = 32; off > 0; off >>= 1) dev += __shfl_xor(dev, off);   // (a fixed tree: identical bits on every call)
  if (lane < V) {
    unsigned char k = 255;
#pragma unroll
    for (int v = 0; v < FUSE_MAXV; ++v)
      if (v == lane && ((mask >> v) & 1)) k = (unsigned char)kv[v];
    A.choice[f * V + lane] = k;
  }
  if (lane == 0) {
    A.cost[f] = (float)best;
    A.spread[f] = (float)sqrt(dev / ((double)n * (double)J));
    A.ok[f] = best >= FUSE_BIG ? 0 : 1;
  }
}

struct FusePlaceArgs {
  const float* pose;             // (Ftot, J, 3)
  const float* kp;               // (V, Ftot, J, 2)
  const unsigned char* valid;    // (V, Ftot) or null
  const long* take_offset;       // (G + 1) device
  const float* quat;             // (G, V, 4) device or null
  const float* trans;            // (G, V, 3) device
  const float* intr;             // (G, V, 9) device
  const float* weights;          // (J) device or null
  float* root;                   // (Ftot, 3)
  float* reproj;                 // (V, Ftot)
  unsigned char* ok;             // (Ftot)
  unsigned char* steps;          // (Ftot) or null
  long Ftot;
  int V, J, G, distort, iters;
};

// view `cam` (its row of the take's tables) added to e: P = R^T (pose_j + r - T), the projection's Jacobian taken through R^T
template <bool JAC>
__device__ __forceinline__ void fuse_eval_view(LiftGN& e, const float* P, const float* U, const float* weights, int J, int distort, const float* q,
                                               const float* T, const float* cam, double rx, double ry, double rz) {
  Rot3 R;
  lift_rot3(q, R);
  const LiftCam K = lift_cam(cam);
  const double ox = rx - (double)T[0], oy = ry - (double)T[1], oz = rz - (double)T[2];
  for (int j = 0; j < J; ++j) {                                         // sums in joint order
    const double w = weights != nullptr ? (double)weights[j] : 1.0;
    if (w == 0.0) continue;
    const double wx = (double)P[j * 3] + ox, wy = (double)P[j * 3 + 1] + oy, wz = (double)P[j * 3 + 2] + oz;
    const double X = R.r00 * wx + R.r10 * wy + R.r20 * wz, Y = R.r01 * wx + R.r11 * wy + R.r21 * wz, Z = R.r02 * wx + R.r12 * wy + R.r22 * wz;
    if (!(Z > 0.0)) e.deep = false;
    const LiftProj pr = lift_project<JAC>(X, Y, Z, U + 2 * j, K, distort);
    const double j00 = pr.c00 * R.r00 + pr.c01 * R.r01 + pr.c02 * R.r02, j01 = pr.c00 * R.r10 + pr.c01 * R.r11 + pr.c02 * R.r12,
                 j02 = pr.c00 * R.r20 + pr.c01 * R.r21 + pr.c02 * R.r22;                                  // J_j R^T: with respect to r
    const double j10 = pr.c10 * R.r00 + pr.c11 * R.r01 + pr.c12 * R.r02, j11 = pr.c10 * R.r10 + pr.c11 * R.r11 + pr.c12 * R.r12,
                 j12 = pr.c10 * R.r20 + pr.c11 * R.r21 + pr.c12 * R.r22;
    lift_gn_add<JAC>(e, w, pr, j00, j01, j02, j10, j11, j12);
  }
}

// the sums over the valid views in order, then the joints in order
template <bool JAC>
__device__ __forceinline__ LiftGN fuse_eval(const FusePlaceArgs& A, long f, int g, int mask, double rx, double ry, double rz) {
  LiftGN e = lift_gn_start();
  for (int v = 0; v < A.V; ++v) {
    if (!((mask >> v) & 1)) continue;
    const long gv = (long)g * A.V + v;
    fuse_eval_view<JAC>(e, A.pose + f * A.J * 3, A.kp + ((long)v * A.Ftot + f) * A.J * 2, A.weights, A.J, A.distort,
                        A.quat != nullptr ? A.quat + gv * 4 : nullptr, A.trans + gv * 3, A.intr + gv * 9, rx, ry, rz);
  }
  return e;
}

__global__ __launch_bounds__(FUSE_PLACE_THREADS) void lift_fuse_place_kernel(FusePlaceArgs A) {
  const int V = A.V, J = A.J;
  const long f = (long)blockIdx.x * FUSE_PLACE_THREADS + threadIdx.x;
  if (f >= A.Ftot) return;
  const int g = lift_seq_of(A.take_offset, A.G, f);
  const int mask = lift_view_mask(A.valid, A.quat, V, A.Ftot, f, g);
  const float* P = A.pose + f * J * 3;
  // 1. the linear pinhole fit over all valid views
  LiftNormal3 lin = {};
  double W = 0.0;
  for (int v = 0; v < V; ++v) {
    if (!((mask >> v) & 1)) continue;
    const long gv = (long)g * V + v;
    Rot3 R;
    lift_rot3(A.quat != nullptr ? A.quat + gv * 4 : nullptr, R);
    const float* cam = A.intr + gv * 9;
    const float* T = A.trans + gv * 3;
    const float* U = A.kp + ((long)v * A.Ftot + f) * J * 2;
    const double fx = cam[0], fy = cam[1], cx = cam[2], cy = cam[3], Tx = T[0], Ty = T[1], Tz = T[2];
    for (int j = 0; j < J; ++j) {
      const double w = A.weights != nullptr ? (double)A.weights[j] : 1.0;
      if (w == 0.0) continue;
      const double a = ((double)U[2 * j] - cx) / fx, b = ((double)U[2 * j + 1] - cy) / fy;
      // rows of R^T are columns of R: rho_x = (r00, r10, r20), rho_y = (r01, r11, r21), rho_z = (r02, r12, r22)
      const double mx0 = R.r00 - a * R.r02, mx1 = R.r10 - a * R.r12, mx2 = R.r20 - a * R.r22;
      const double my0 = R.r01 - b * R.r02, my1 = R.r11 - b * R.r12, my2 = R.r21 - b * R.r22;
      const double c0 = Tx - (double)P[j * 3], c1 = Ty - (double)P[j * 3 + 1], c2 = Tz - (double)P[j * 3 + 2];
      const double sx = mx0 * c0 + mx1 * c1 + mx2 * c2, sy = my0 * c0 + my1 * c1 + my2 * c2;
      W += w;
      lift_normal3_add(lin, w, sx, sy, mx0, mx1, mx2, my0, my1, my2);
    }
  }
  double rx = 0.0, ry = 0.0, rz = 0.0;
  bool have = false;
  {
    LiftAdj3 adj;
    const bool solvable = lift_adj3(lin, adj);
    const bool finite = __builtin_isfinite(W) && __builtin_isfinite(lin.H00) && __builtin_isfinite(lin.H01) && __builtin_isfinite(lin.H02) &&
                        __builtin_isfinite(lin.H11) && __builtin_isfinite(lin.H12) && __builtin_isfinite(lin.H22) && __builtin_isfinite(lin.g0) &&
                        __builtin_isfinite(lin.g1) && __builtin_isfinite(lin.g2);
    if (mask != 0 && W > 0.0 && finite && solvable) {
      lift_adj3_solve(adj, lin.g0, lin.g1, lin.g2, rx, ry, rz);
      have = __builtin_isfinite(rx) && __builtin_isfinite(ry) && __builtin_isfinite(rz);
      if (!have) { rx = 0.0; ry = 0.0; rz = 0.0; }
    }
  }
  unsigned char ok = 0, taken = 0;
  if (have) {                                                           // 2., 3. of mp_lift_place_refine
    LiftGN e = A.iters > 0 ? fuse_eval<true>(A, f, g, mask, rx, ry, rz) : fuse_eval<false>(A, f, g, mask, rx, ry, rz);
    if (e.deep && __builtin_isfinite(e.F)) {
      ok = 1;
      for (int k = 0; k < A.iters; ++k) {
        double nx, ny, nz;
        if (!lift_gn_step(e, rx, ry, rz, nx, ny, nz)) break;
        const LiftGN n = fuse_eval<true>(A, f, g, mask, nx, ny, nz);
        if (!lift_gn_accept(n, e)) break;
        rx = nx; ry = ny; rz = nz; e = n; ++taken;
      }
    }
  }
  A.root[f * 3] = (float)rx; A.root[f * 3 + 1] = (float)ry; A.root[f * 3 + 2] = (float)rz;
  for (int v = 0; v < V; ++v) {                                         // 4. every view's own error at the final root
    double err = 0.0;
    if (have && ((mask >> v) & 1)) {
      const long gv = (long)g * V + v;
      LiftGN e = lift_gn_start();
      fuse_eval_view<false>(e, P, A.kp + ((long)v * A.Ftot + f) * J * 2, A.weights, J, A.distort, A.quat != nullptr ? A.quat + gv * 4 : nullptr,
                            A.trans + gv * 3, A.intr + gv * 9, rx, ry, rz);
      err = e.E / e.W;
    }
    A.reproj[(long)v * A.Ftot + f] = (float)err;
  }
  A.ok[f] = ok;
  if (A.steps != nullptr) A.steps[f] = taken;
}

}  // namespace mp
using namespace mp;

extern "C" {

int mp_lift_fuse(const float* hyps, int V, int64_t Ftot, int K, int J, int C, const uint8_t* valid, const int64_t* take_offset, int G, const float* quat,
                 float sigma, float score_weight, float* pose, uint8_t* choice, float* cost, float* spread, uint8_t* ok, void* stream) {
  static_assert(sizeof(long) == sizeof(int64_t), "LP64");
  MP_CHECK(hyps && take_offset && pose && choice && cost && spread && ok, MP_ERR_ARG, "mp_lift_fuse: null pointer");
  if (int rc = lift_take_shape("mp_lift_fuse", V, (long)Ftot, J, G)) return rc;
  MP_CHECK(K >= 1 && K <= FUSE_MAXK, MP_ERR_ARG, "mp_lift_fuse: K=%d outside 1..%d", K, FUSE_MAXK);
  MP_CHECK(C == 3 || C == 4, MP_ERR_ARG, "mp_lift_fuse: C=%d (3: poses, 4: hypotheses with their score)", C);
  MP_CHECK(sigma > 0.f, MP_ERR_ARG, "mp_lift_fuse: sigma=%g must be > 0 (inf: the pair factor is 0)", (double)sigma);
  MP_CHECK(score_weight >= 0.f && __builtin_isfinite(score_weight), MP_ERR_ARG, "mp_lift_fuse: score_weight=%g must be finite and >= 0",
           (double)score_weight);
  const int frame_doubles = FUSE_MAXV * 9 + V * K * J * 3 + V * K + 6 * K * K;
  int waves = FUSE_WAVES;
  while (waves > 1 && (long)waves * frame_doubles * 8 > FUSE_LDS_LIMIT) waves >>= 1;     // (at 4 x 8 x 32: 28 KB a frame, two frames a workgroup)
  const long blocks = ((long)Ftot + waves - 1) / waves;
  MP_CHECK(blocks <= 0x7fffffffL, MP_ERR_ARG, "mp_lift_fuse: %ld frames: too many for one launch", (long)Ftot);
  FuseArgs a = {};
  a.hyps = hyps; a.valid = valid; a.take_offset = (const long*)take_offset; a.quat = quat;
  a.pose = pose; a.choice = choice; a.cost = cost; a.spread = spread; a.ok = ok; a.Ftot = (long)Ftot;
  a.pair_factor = 1.0 / (2.0 * (double)sigma * (double)sigma);          // (sigma = +inf: exactly 0)
  a.score_weight = (double)score_weight;
  a.V = V; a.K = K; a.J = J; a.C = C; a.G = G; a.waves = waves; a.frame_doubles = frame_doubles;
  hipLaunchKernelGGL(lift_fuse_kernel, dim3((unsigned)blocks), dim3(waves * 64), (size_t)waves * frame_doubles * 8, (hipStream_t)stream, a);
  MP_LAUNCH_CHECK();
  return MP_OK;
}

int mp_lift_fuse_place(const float* pose, const float* kp, int V, int64_t Ftot, int J, const uint8_t* valid, const int64_t* take_offset, int G,
                       const float* quat, const float* trans, const float* intr, const float* weights, int distort, int iters, float* root,
                       float* reproj, uint8_t* ok, uint8_t* steps, void* stream) {
  MP_CHECK(pose && kp && take_offset && trans && intr && root && reproj && ok, MP_ERR_ARG, "mp_lift_fuse_place: null pointer");
  if (int rc = lift_take_shape("mp_lift_fuse_place", V, (long)Ftot, J, G)) return rc;
  MP_CHECK(distort == 0 || distort == 1, MP_ERR_ARG, "mp_lift_fuse_place: distort=%d (0: project_to_2d_linear, 1: project_to_2d)", distort);
  MP_CHECK(iters >= 0 && iters <= MP_LIFT_REFINE_MAXITERS, MP_ERR_ARG, "mp_lift_fuse_place: iters=%d outside 0..%d", iters, MP_LIFT_REFINE_MAXITERS);
  const long blocks = ((long)Ftot + FUSE_PLACE_THREADS - 1) / FUSE_PLACE_THREADS;
  MP_CHECK(blocks <= 0x7fffffffL, MP_ERR_ARG, "mp_lift_fuse_place: %ld frames: too many for one launch", (long)Ftot);
  FusePlaceArgs a = {};
  a.pose = pose; a.kp = kp; a.valid = valid; a.take_offset = (const long*)take_offset; a.quat = quat; a.trans = trans; a.intr = intr;
  a.weights = weights; a.root = root; a.reproj = reproj; a.ok = ok; a.steps = steps; a.Ftot = (long)Ftot;
  a.V = V; a.J = J; a.G = G; a.distort = distort; a.iters = iters;
  hipLaunchKernelGGL(lift_fuse_place_kernel, dim3((unsigned)blocks), dim3(FUSE_PLACE_THREADS), 0, (hipStream_t)stream, a);
  MP_LAUNCH_CHECK();
  return MP_OK;
}

}  // extern "C"

// Standing a take on its floor (include/manipose_hip.h: mp_lift_ground has the rule).  Feet that stand still are standing on something: a foot is
// in CONTACT in a frame where its central difference over +- radius frames is slow, the contact points of a sequence span its floor, and the plane
// through them - the eigenvector of the smallest eigenvalue of their weighted scatter, re-weighted `iters` times so that a slow foot held in the air
// is shed, with the body's mean axis as a weak prior that decides the planes two ankles in place leave open and the side that is up - gives the
// rotation and the shift that stand the sequence on z = foot_height.  The same pass reports each foot's height over the plane and how far the feet
// slide while in contact.  tests/lift_ground_ref.py states the rule in float64.
//
// TWO KERNELS.  ground_contact_kernel: one lane per (frame, foot); a frame's J C floats are contiguous, a lane reads three joints of three frames.
// ground_plane_kernel: ONE WORKGROUP OF 256 LANES OWNS ONE SEQUENCE, the shape of lift_align.hip's kernel.  A lane walks the frames f0 + lane,
// f0 + lane + 256, ... in order, within a frame the feet in order, and keeps its eight sums in registers: the arrays below are indexed by unrolled
// constants only, nothing lands in scratch.  The lanes' sums are added by an xor butterfly within a wave - all 64 lanes hold the same bits - and the
// four waves' sums through LDS in wave order, (w0 + w1) + (w2 + w3); EVERY lane then solves the eigenproblem (lift_geom.h's lift_eig4 on s I - A,
// padded with a zero row and column) on identical sums, so the branches on its result are uniform and the next pass has its plane without a
// broadcast.  The passes follow one another inside the workgroup, 2 (iters + 1) + 1 of them: no grid-wide synchronisation, no scratch memory.
// Everything between the float32 loads and the float32 stores is fp64, without contraction; no atomics, fixed orders: identical bits on every call.
#include "lift_common.h"

#pragma clang fp contract(off)
#include "lift_geom.h"                    // after the pragma: the shared code takes this file's mode

namespace mp {

constexpr int GROUND_THREADS = 256, GROUND_WAVES = GROUND_THREADS / 64;
constexpr int GROUND_MAXF = MP_LIFT_GROUND_MAXFEET;
constexpr int GROUND_SUMS = 8;                   // of a pass at most: sum w, 3 of sum w x, the count, 3 of the axis
constexpr double GROUND_GAP = 1e-9;              // (a2 - a1) <= GROUND_GAP max(|a1|, |a3|): the points do not span a plane
constexpr double GROUND_TINY = 1e-12;            // a direction shorter than this has none

struct GroundArgs {
  const float* points;           // (Ntot, J, C)
  const unsigned char* valid;    // (Ntot) or null
  const long* seq_offset;        // (S + 1) device
  unsigned char* contact;        // (Ntot, nf)
  float* height;                 // (Ntot, nf)
  float* normal;                 // (S, 3)
  float* offset;                 // (S)
  float* quat;                   // (S, 4)
  float* trans;                  // (S, 3)
  float* rms;                    // (S)
  float* gap;                    // (S)
  float* skate;                  // (S)
  int* used;                     // (S)
  int* skate_pairs;              // (S)
  unsigned char* ok;             // (S)
  long Ntot;
  double thr2;                   // (2 radius speed)^2
  double sigma2;                 // sigma^2 (+inf: every weight is exactly 1)
  double prior2;                 // prior^2
  double foot_height;
  int J, C, S, nf, radius, iters, axis_from, axis_to;
  signed char feet[GROUND_MAXF];
};

struct GroundPlane { double nx, ny, nz, off; };

// joint j of frame f in fp64; false where a coordinate is not finite
__device__ __forceinline__ bool ground_load(const GroundArgs& A, long f, int j, double& x, double& y, double& z) {
  const float* p = A.points + (f * A.J + j) * A.C;
  x = p[0]; y = p[1]; z = p[2];
  return __builtin_isfinite((x + y) + z);                               // (a sum of float32 values in fp64 cannot overflow)
}

__device__ __forceinline__ bool ground_valid(const GroundArgs& A, long f) { return A.valid == nullptr || A.valid[f] != 0; }

// step A: one lane per (frame, foot).  It also clears the foot's height: a frame that no sequence holds keeps the zero.
__global__ __launch_bounds__(GROUND_THREADS) void ground_contact_kernel(GroundArgs A) {
  const long i = (long)blockIdx.x * GROUND_THREADS + threadIdx.x;
  if (i >= A.Ntot * A.nf) return;
  const long f = i / A.nf;
  const int k = (int)(i % A.nf);
  int j = A.feet[0];
#pragma unroll
  for (int u = 1; u < GROUND_MAXF; ++u)
    if (u == k) j = A.feet[u];
  const FrameRange fr = lift_seq_frames(A.seq_offset, lift_seq_of(A.seq_offset, A.S, f), A.Ntot);
  const long r = A.radius;
  int c = 0;
  if (f - r >= fr.f0 && f + r < fr.f1 && ground_valid(A, f - r) && ground_valid(A, f) && ground_valid(A, f + r)) {
    double ax, ay, az, bx, by, bz, mx, my, mz;
    const bool fa = ground_load(A, f - r, j, ax, ay, az), fm = ground_load(A, f, j, mx, my, mz), fb = ground_load(A, f + r, j, bx, by, bz);
    const double dx = bx - ax, dy = by - ay, dz = bz - az;
    c = (fa && fm && fb && (dx * dx + dy * dy) + dz * dz <= A.thr2) ? 1 : 0;
  }
  A.contact[i] = (unsigned char)c;
  A.height[i] = 0.f;
}

// the lanes' sums added: a butterfly within the wave, then the waves in order; every lane returns with the workgroup's sums
__device__ __forceinline__ void ground_reduce(double (&x)[GROUND_SUMS], double* lds) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
#pragma unroll
    for (int k = 0; k < GROUND_SUMS; ++k) x[k] += __shfl_xor(x[k], off);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();                                                      // (the readers of the reduction before are done)
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < GROUND_SUMS; ++k) lds[wave * GROUND_SUMS + k] = x[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < GROUND_SUMS; ++k)
    x[k] = (lds[k] + lds[GROUND_SUMS + k]) + (lds[2 * GROUND_SUMS + k] + lds[3 * GROUND_SUMS + k]);
}

// the weight of a contact point under the plane of the solve before: 1 / (1 + r^2 / sigma^2)^2
__device__ __forceinline__ double ground_weight(const GroundArgs& A, const GroundPlane& P, double x, double y, double z) {
  const double r = ((P.nx * x + P.ny * y) + P.nz * z) - P.off;
  const double t = 1.0 + (r * r) / A.sigma2;
  return 1.0 / (t * t);
}

// One pass of this lane over the contact points of its frames.  weighted: w under the plane Pw, else 1.
// MODE 0: acc[0] += w, acc[1..3] += w x, acc[4] += 1; with `axis` also acc[5..7] += unit(p[to] - p[from]) per valid, finite frame   (step B, W, m)
// MODE 1: acc[0..5] += w (x - m)(x - m)^T, upper triangle by rows                                                                      (the scatter)
template <int MODE>
__device__ __forceinline__ void ground_pass(const GroundArgs& A, long f0, long f1, bool weighted, const GroundPlane& Pw, bool axis, double mx, double my,
                                            double mz, double (&acc)[GROUND_SUMS]) {
  const int nf = A.nf;
#pragma unroll
  for (int k = 0; k < GROUND_SUMS; ++k) acc[k] = 0.0;
#pragma unroll 1
  for (long f = f0 + threadIdx.x; f < f1; f += GROUND_THREADS) {
    if (MODE == 0 && axis && ground_valid(A, f)) {
      double ax, ay, az, bx, by, bz;
      const bool fa = ground_load(A, f, A.axis_from, ax, ay, az), fb = ground_load(A, f, A.axis_to, bx, by, bz);
      const double dx = bx - ax, dy = by - ay, dz = bz - az;
      const double d = sqrt((dx * dx + dy * dy) + dz * dz);
      if (fa && fb && d >= GROUND_TINY) { acc[5] += dx / d; acc[6] += dy / d; acc[7] += dz / d; }
    }
#pragma unroll
    for (int k = 0; k < GROUND_MAXF; ++k) {
      if (k >= nf || A.contact[f * nf + k] == 0) continue;
      double x, y, z;
      ground_load(A, f, A.feet[k], x, y, z);                            // (a contact is finite)
      const double w = weighted ? ground_weight(A, Pw, x, y, z) : 1.0;
      if (MODE == 0) {
        acc[0] += w; acc[1] += w * x; acc[2] += w * y; acc[3] += w * z;
        acc[4] += 1.0;
      } else {
        const double ux = x - mx, uy = y - my, uz = z - mz;
        acc[0] += w * (ux * ux); acc[1] += w * (ux * uy); acc[2] += w * (ux * uz);
        acc[3] += w * (uy * uy); acc[4] += w * (uy * uz); acc[5] += w * (uz * uz);
      }
    }
  }
}

// step C on the workgroup's sums: W, the mean m, the scatter c (upper triangle by rows), the axis b or none.  The plane, the eigenvalue differences
// d21 = a2 - a1 and d31 = a3 - a1, and whether the axis decided the side; false: no plane.
__device__ __forceinline__ bool ground_solve(const GroundArgs& A, double W, double mx, double my, double mz, const double (&c)[GROUND_SUMS], bool has_axis,
                                             double bx, double by, double bz, GroundPlane& P, double& d21, double& d31, bool& sided) {
  bool finite = __builtin_isfinite(W) && __builtin_isfinite((mx + my) + mz);
#pragma unroll
  for (int k = 0; k < 6; ++k) finite = finite && __builtin_isfinite(c[k]);
  if (!finite || !(W > 0.0)) return false;
  const bool pull = has_axis && A.prior2 > 0.0;
  const double pw = pull ? A.prior2 * W : 0.0;
  double a00 = c[0], a01 = c[1], a02 = c[2], a11 = c[3], a12 = c[4], a22 = c[5];
  if (pull) {
    a00 = a00 - pw * (bx * bx); a01 = a01 - pw * (bx * by); a02 = a02 - pw * (bx * bz);
    a11 = a11 - pw * (by * by); a12 = a12 - pw * (by * bz); a22 = a22 - pw * (bz * bz);
  }
  const double s = ((c[0] + c[3]) + c[5]) + A.prior2 * W;                // s I - A is positive semidefinite: its dominant eigenvector is A's smallest
  double m[4][4];
  m[0][0] = s - a00; m[1][1] = s - a11; m[2][2] = s - a22; m[3][3] = 0.0;
  m[0][1] = m[1][0] = 0.0 - a01; m[0][2] = m[2][0] = 0.0 - a02; m[1][2] = m[2][1] = 0.0 - a12;
  m[0][3] = m[3][0] = 0.0; m[1][3] = m[3][1] = 0.0; m[2][3] = m[3][2] = 0.0;
  double q[4], l1, l2;
  lift_eig4(m, q, l1, l2);                                              // (the padded row and column stay as they are: every rotation with them is the identity)
  const double e0 = m[0][0], e1 = m[1][1], e2 = m[2][2];
  const double hi = fmax(fmax(e0, e1), e2), lo = fmin(fmin(e0, e1), e2);
  const double mid = fmax(fmin(e0, e1), fmin(fmax(e0, e1), e2));
  d21 = hi - mid; d31 = hi - lo;
  const double a1 = s - hi, a3 = s - lo;
  if (!__builtin_isfinite(s) || !(q[3] == 0.0) || !(d21 > GROUND_GAP * fmax(fabs(a1), fabs(a3)))) return false;
  const double qn = 1.0 / sqrt((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]);
  double nx = q[0] * qn + 0.0, ny = q[1] * qn + 0.0, nz = q[2] * qn + 0.0;   // (+ 0: a zero component comes out as +0)
  const double d = has_axis ? (nx * bx + ny * by) + nz * bz : 0.0;
  sided = has_axis && d != 0.0;
  const bool flip = sided ? d < 0.0 : (nx < 0.0 || (nx == 0.0 && (ny < 0.0 || (ny == 0.0 && nz < 0.0))));
  if (flip) { nx = 0.0 - nx; ny = 0.0 - ny; nz = 0.0 - nz; }            // (0 - x: a zero component comes out as +0)
  P.nx = nx; P.ny = ny; P.nz = nz;
  P.off = ((nx * mx + ny * my) + nz * mz) + 0.0;                        // (+ 0: a zero offset comes out as +0)
  return __builtin_isfinite(((nx + ny) + nz) + P.off);
}

__global__ __launch_bounds__(GROUND_THREADS) void ground_plane_kernel(GroundArgs A) {
  __shared__ double lds[GROUND_WAVES * GROUND_SUMS];
  const int s = blockIdx.x, nf = A.nf;
  const FrameRange fr = lift_seq_frames(A.seq_offset, s, A.Ntot);
  double acc[GROUND_SUMS];
  GroundPlane P = {0.0, 0.0, 1.0, 0.0}, Pw = P;                         // the plane of the last solve, and of the one before (its weights)
  double d21 = 0.0, d31 = 0.0, bx = 0.0, by = 0.0, bz = 0.0;
  bool has_axis = false, sided = false, good = true;
  int used = 0;

  // steps B and C: iters + 1 solves of two passes each
#pragma unroll 1
  for (int it = 0; good && it <= A.iters; ++it) {
    Pw = P;
    ground_pass<0>(A, fr.f0, fr.f1, it > 0, Pw, it == 0, 0.0, 0.0, 0.0, acc);
    ground_reduce(acc, lds);
    if (it == 0) {
      used = (int)acc[4];
      const double bn = sqrt((acc[5] * acc[5] + acc[6] * acc[6]) + acc[7] * acc[7]);
      has_axis = __builtin_isfinite(bn) && bn >= GROUND_TINY;
      if (has_axis) { bx = acc[5] / bn; by = acc[6] / bn; bz = acc[7] / bn; }
    }
    const double W = acc[0], mx = acc[1] / W, my = acc[2] / W, mz = acc[3] / W;
    good = used >= 3 && W > 0.0 && __builtin_isfinite(W) && __builtin_isfinite((mx + my) + mz);
    if (!good) break;                                                   // (uniform: every lane holds the same sums)
    ground_pass<1>(A, fr.f0, fr.f1, it > 0, Pw, false, mx, my, mz, acc);
    ground_reduce(acc, lds);
    good = ground_solve(A, W, mx, my, mz, acc, has_axis, bx, by, bz, P, d21, d31, sided);
  }

  // step E: the residual under the weights of the last solve, the feet's heights, the skate
  const bool weighted = good && A.iters > 0;
#pragma unroll
  for (int k = 0; k < GROUND_SUMS; ++k) acc[k] = 0.0;
#pragma unroll 1
  for (long f = fr.f0 + threadIdx.x; f < fr.f1; f += GROUND_THREADS) {
    const bool vf = ground_valid(A, f);
#pragma unroll
    for (int k = 0; k < GROUND_MAXF; ++k) {
      if (k >= nf) continue;
      double x = 0.0, y = 0.0, z = 0.0;
      const bool fin = vf && ground_load(A, f, A.feet[k], x, y, z);
      double h = 0.0;
      if (fin && good) h = (((P.nx * x + P.ny * y) + P.nz * z) - P.off) + 0.0;
      A.height[f * nf + k] = (float)h;
      if (A.contact[f * nf + k] == 0) continue;
      if (good) {
        const double w = weighted ? ground_weight(A, Pw, x, y, z) : 1.0;
        acc[0] += w * (h * h);
        acc[1] += w;
      }
      if (f + 1 < fr.f1 && A.contact[(f + 1) * nf + k] != 0) {
        double x1, y1, z1;
        ground_load(A, f + 1, A.feet[k], x1, y1, z1);
        double dx = x1 - x, dy = y1 - y, dz = z1 - z;
        if (good) {                                                     // the part of the step in the plane; without a plane the whole step
          const double dn = (P.nx * dx + P.ny * dy) + P.nz * dz;
          dx = dx - dn * P.nx; dy = dy - dn * P.ny; dz = dz - dn * P.nz;
        }
        acc[2] += sqrt((dx * dx + dy * dy) + dz * dz);
        acc[3] += 1.0;
      }
    }
  }
  ground_reduce(acc, lds);
  if (threadIdx.x != 0) return;
  A.used[s] = used;
  A.skate_pairs[s] = (int)acc[3];
  A.skate[s] = acc[3] > 0.0 ? (float)(acc[2] / acc[3]) : 0.f;
  if (!good) {
    A.normal[s * 3] = 0.f; A.normal[s * 3 + 1] = 0.f; A.normal[s * 3 + 2] = 1.f;
    A.quat[s * 4] = 1.f; A.quat[s * 4 + 1] = 0.f; A.quat[s * 4 + 2] = 0.f; A.quat[s * 4 + 3] = 0.f;
    A.trans[s * 3] = 0.f; A.trans[s * 3 + 1] = 0.f; A.trans[s * 3 + 2] = 0.f;
    A.offset[s] = 0.f; A.rms[s] = 0.f; A.gap[s] = 0.f; A.ok[s] = 0;
    return;
  }
  A.normal[s * 3] = (float)P.nx; A.normal[s * 3 + 1] = (float)P.ny; A.normal[s * 3 + 2] = (float)P.nz;
  A.offset[s] = (float)P.off;
  double qw = 1.0 + P.nz, qx = P.ny, qy = 0.0 - P.nx;
  if (qw < GROUND_TINY) { qw = 0.0; qx = 1.0; qy = 0.0; }
  else {
    const double qn = 1.0 / sqrt((qw * qw + qx * qx) + qy * qy);
    qw = qw * qn; qx = qx * qn; qy = qy * qn;
  }
  A.quat[s * 4] = (float)qw; A.quat[s * 4 + 1] = (float)qx; A.quat[s * 4 + 2] = (float)qy; A.quat[s * 4 + 3] = 0.f;
  A.trans[s * 3] = 0.f; A.trans[s * 3 + 1] = 0.f; A.trans[s * 3 + 2] = (float)(A.foot_height - P.off);
  A.rms[s] = (float)sqrt(acc[0] / acc[1]);                               // (sum w is the W > 0 of the last solve)
  A.gap[s] = d31 > 0.0 ? (float)(d21 / d31) : 0.f;
  A.ok[s] = (unsigned char)(sided ? 3 : 1);
}

}  // namespace mp
using namespace mp;

extern "C" {

int mp_lift_ground(const float* points, int64_t Ntot, int J, int C, const uint8_t* valid, const int64_t* seq_offset, int S, const int32_t* feet, int nf,
                   int axis_from, int axis_to, int radius, float speed, float sigma, float prior, int iters, float foot_height, float* normal,
                   float* offset, float* quat, float* trans, float* rms, float* gap, int32_t* used, uint8_t* ok, uint8_t* contact, float* height,
                   float* skate, int32_t* skate_pairs, void* stream) {
  static_assert(sizeof(long) == sizeof(int64_t), "LP64");
  long blocks = 0;
  if (int rc = lift_pose_shape("mp_lift_ground", (long)Ntot, 1, J, C, S, &blocks)) return rc;
  MP_CHECK(points && seq_offset, MP_ERR_ARG, "mp_lift_ground: points or seq_offset null");
  MP_CHECK(normal && offset && quat && trans && rms && gap && used && ok && contact && height && skate && skate_pairs, MP_ERR_ARG,
           "mp_lift_ground: null output (normal, offset, quat, trans, rms, gap, used, ok, contact, height, skate, skate_pairs are all written)");
  MP_CHECK(feet != nullptr, MP_ERR_ARG, "mp_lift_ground: null feet table");
  MP_CHECK(nf >= 1 && nf <= MP_LIFT_GROUND_MAXFEET, MP_ERR_ARG, "mp_lift_ground: nf=%d feet outside 1..%d", nf, MP_LIFT_GROUND_MAXFEET);
  for (int k = 0; k < nf; ++k) MP_CHECK(feet[k] >= 0 && feet[k] < J, MP_ERR_ARG, "mp_lift_ground: feet[%d] = %d outside 0..%d", k, feet[k], J - 1);
  MP_CHECK(axis_from >= 0 && axis_from < J && axis_to >= 0 && axis_to < J, MP_ERR_ARG, "mp_lift_ground: axis_from=%d axis_to=%d outside 0..%d", axis_from,
           axis_to, J - 1);
  MP_CHECK(axis_from != axis_to, MP_ERR_ARG, "mp_lift_ground: axis_from == axis_to = %d: two joints span the body's axis", axis_from);
  MP_CHECK(radius >= 1 && radius <= MP_LIFT_GROUND_MAXRADIUS, MP_ERR_ARG, "mp_lift_ground: radius=%d outside 1..%d", radius, MP_LIFT_GROUND_MAXRADIUS);
  MP_CHECK(iters >= 0 && iters <= MP_LIFT_GROUND_MAXITERS, MP_ERR_ARG, "mp_lift_ground: iters=%d outside 0..%d", iters, MP_LIFT_GROUND_MAXITERS);
  MP_CHECK(speed > 0.f && __builtin_isfinite(speed), MP_ERR_ARG, "mp_lift_ground: speed=%g must be finite and > 0", (double)speed);
  MP_CHECK(sigma > 0.f, MP_ERR_ARG, "mp_lift_ground: sigma=%g must be > 0 (inf: every weight is 1)", (double)sigma);
  MP_CHECK(prior >= 0.f && __builtin_isfinite(prior), MP_ERR_ARG, "mp_lift_ground: prior=%g must be finite and >= 0", (double)prior);
  MP_CHECK(__builtin_isfinite(foot_height), MP_ERR_ARG, "mp_lift_ground: foot_height=%g must be finite", (double)foot_height);
  MP_CHECK((long)Ntot * nf <= 0x7fffffffL, MP_ERR_ARG, "mp_lift_ground: Ntot=%ld frames of %d feet: too many for one launch", (long)Ntot, nf);
  GroundArgs a = {};
  a.points = points; a.valid = valid; a.seq_offset = (const long*)seq_offset; a.contact = contact; a.height = height; a.normal = normal;
  a.offset = offset; a.quat = quat; a.trans = trans; a.rms = rms; a.gap = gap; a.skate = skate; a.used = used; a.skate_pairs = skate_pairs; a.ok = ok;
  a.Ntot = (long)Ntot;
  const double thr = (2.0 * (double)radius) * (double)speed;
  a.thr2 = thr * thr;
  a.sigma2 = (double)sigma * (double)sigma;
  a.prior2 = (double)prior * (double)prior;
  a.foot_height = (double)foot_height;
  a.J = J; a.C = C; a.S = S; a.nf = nf; a.radius = radius; a.iters = iters; a.axis_from = axis_from; a.axis_to = axis_to;
  for (int k = 0; k < GROUND_MAXF; ++k) a.feet[k] = (signed char)feet[k < nf ? k : 0];
  const long lanes = (long)Ntot * nf;
  hipLaunchKernelGGL(ground_contact_kernel, dim3((unsigned)((lanes + GROUND_THREADS - 1) / GROUND_THREADS)), dim3(GROUND_THREADS), 0, (hipStream_t)stream, a);
  MP_LAUNCH_CHECK();
  hipLaunchKernelGGL(ground_plane_kernel, dim3((unsigned)S), dim3(GROUND_THREADS), 0, (hipStream_t)stream, a);
  MP_LAUNCH_CHECK();
  return MP_OK;
}

}  // extern "C"

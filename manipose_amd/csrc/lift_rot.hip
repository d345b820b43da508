// Joint rotations of lifted poses (include/manipose_hip.h: mp_lift_rotations): the inverse of the decoder's forward kinematics (fk_decode.hip:
// Rw[0] = R[0], Rw[j] = Rw[parent] R[j], p[j] = p[parent] + Rw[j] (len_j rest_j)) on the poses the lifting pipeline emits.  Per pose the root
// orientation from the frame its two reference bones span, then per joint the shortest-arc (twist-free) rotation that turns the bone's T-pose
// direction into its measured direction as the parent sees it.  The reference has no counterpart (its hpe/viz.py draws positions).
//
// lift_rot_kernel: ONE LANE OWNS ONE (pose, joint), 64 / J poses per wave (3 for the 17-joint tree, 2 for 32 joints), as fk_decode.hip maps its
// lanes, and like there the tree is walked level by level: a lane of depth d fetches its parent's WORLD rotation, a unit quaternion of 4 doubles,
// from the parent's lane with wavefront shuffles, so no world rotation is ever indexed at run time in a per-lane array (which would live in
// scratch memory) and none touches memory at all.  The lane's own tables (parent, depth, T-pose direction, the axis of its half-turn) are picked
// from the kernel arguments by a chain of selects over compile-time indices.  "Any coordinate of the pose is not finite" and "every joint is
// regular" are wave ballots masked to the pose's lanes: no LDS, no atomics, a fixed order, identical bits on every call.  Everything between the
// float32 loads and the float32 stores is fp64 (sqrt and the divisions correctly rounded).  The stores are one 16-byte quaternion per lane at
// consecutive addresses; the loads are 12-byte pieces 4 C bytes apart.  Nothing here reads seq_offset: a pose's result depends on no other pose.
//
// lift_rot_sign_kernel (MP_LIFT_ROT_CONTINUOUS): ONE WAVE OWNS ONE TRACK (sequence, inner index, joint) and walks its frames 64 at a time: lane l
// loads the stored float32 quaternion of frame f0 + 64 c + l, gets its predecessor's from lane l - 1 (lane 0: from lane 63 of the chunk before,
// kept in registers as it was STORED by the first kernel, so flipping in place has no read-after-write hazard), votes "dot < 0", and the
// exclusive-or prefix of the votes is the parity of the ballot below and including the lane, exclusive-or the carry of the chunks before - integer
// work, exact, the same whatever the chunking.  A lane's loads are 16 bytes 16 inner J bytes apart (the neighbouring tracks' waves use the rest
// of the lines at about the same time).  A wave walks its chunks one after the other: on 3000 frames x 5 hypotheses as ONE sequence (47 chunks) this
// kernel adds 30 us to the first kernel's 20 us, cut into 16 sequences 7 us (tools/lift_bench.py --rotations).
#include "lift_common.h"
#include "../../include/manipose_hip.h"

namespace mp {

struct RotArgs {
  const float* poses;            // (Ntot, inner, J, C), read only
  float* quat;                   // (Ntot, inner, J, 4)
  float* rot6d;                  // (Ntot, inner, J, 6) or null
  unsigned char* ok;             // (Ntot, inner)
  long npose;                    // Ntot * inner
  int J, C, ppw, levels;         // poses per wave (64 / J), depth of the tree
  int a, b;                      // the root's reference children (b = -1: none)
  double E[3][3];                // rows e1, e2, e3 of the T-pose frame (e1 = rest[a])
  double pia[3];                 // the half-turn axis of rest[a], canonical sign
  double rest[LIFT_MAXJ][3];     // unit T-pose directions (row 0 unused)
  double piax[LIFT_MAXJ][3];     // per joint: the half-turn axis of a bone exactly opposite its rest direction, canonical sign
  signed char parent[LIFT_MAXJ];
  signed char depth[LIFT_MAXJ];
};

struct Q4 { double w, x, y, z; };

__device__ __forceinline__ Q4 qmul(const Q4& a, const Q4& b) {
  return {a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z, a.w * b.x + a.x * b.w + a.y * b.z - a.z * b.y,
          a.w * b.y - a.x * b.z + a.y * b.w + a.z * b.x, a.w * b.z + a.x * b.y - a.y * b.x + a.z * b.w};
}

// R(q)^T v for a unit quaternion: v + w t + qv x t with qv = -(x, y, z), t = 2 qv x v  (exactly v for q = (1, 0, 0, 0))
__device__ __forceinline__ void qrot_inv(const Q4& q, const double* v, double* o) {
  const double ax = -q.x, ay = -q.y, az = -q.z;
  const double tx = 2.0 * (ay * v[2] - az * v[1]), ty = 2.0 * (az * v[0] - ax * v[2]), tz = 2.0 * (ax * v[1] - ay * v[0]);
  o[0] = v[0] + q.w * tx + (ay * tz - az * ty);
  o[1] = v[1] + q.w * ty + (az * tx - ax * tz);
  o[2] = v[2] + q.w * tz + (ax * ty - ay * tx);
}

__device__ __forceinline__ bool finite3(const float* p) { return fabsf(p[0]) <= 3.4028235e38f && fabsf(p[1]) <= 3.4028235e38f && fabsf(p[2]) <= 3.4028235e38f; }

// the unit direction of the bone c -> p; false: not good (a non-finite coordinate, or not longer than 1e-12)
__device__ __forceinline__ bool bone_dir(const float* p, const float* c, double* d) {
  const double bx = (double)c[0] - (double)p[0], by = (double)c[1] - (double)p[1], bz = (double)c[2] - (double)p[2];
  const double n = sqrt(bx * bx + by * by + bz * bz);
  const bool good = finite3(p) && finite3(c) && n > 1e-12;
  d[0] = good ? bx / n : 0.0; d[1] = good ? by / n : 0.0; d[2] = good ? bz / n : 0.0;
  return good;
}

// the shortest arc r -> u (both unit): normalize(1 + r . u, r x u); a half turn about `pi` (false is returned) where 1 + r . u < 1e-12
__device__ __forceinline__ bool arc(const double* r, const double* u, const double* pi, Q4& q) {
  const double w = 1.0 + (r[0] * u[0] + r[1] * u[1] + r[2] * u[2]);
  if (w < 1e-12) { q = {0.0, pi[0], pi[1], pi[2]}; return false; }
  const double cx = r[1] * u[2] - r[2] * u[1], cy = r[2] * u[0] - r[0] * u[2], cz = r[0] * u[1] - r[1] * u[0];
  const double n = sqrt(w * w + cx * cx + cy * cy + cz * cz);
  q = {w / n, cx / n, cy / n, cz / n};
  return true;
}

// the unit quaternion of a rotation matrix (row-major), from the largest of 4 w^2, 4 x^2, 4 y^2, 4 z^2 (the first on a tie), normalised, with the
// sign that makes its first non-zero component positive
__device__ __forceinline__ Q4 quat_of(const double (&m)[3][3]) {
  const double tw = 1.0 + m[0][0] + m[1][1] + m[2][2], tx = 1.0 + m[0][0] - m[1][1] - m[2][2], ty = 1.0 - m[0][0] + m[1][1] - m[2][2],
               tz = 1.0 - m[0][0] - m[1][1] + m[2][2];
  Q4 q;
  if (tw >= tx && tw >= ty && tw >= tz) {
    const double s = 2.0 * sqrt(tw);
    q = {0.25 * s, (m[2][1] - m[1][2]) / s, (m[0][2] - m[2][0]) / s, (m[1][0] - m[0][1]) / s};
  } else if (tx >= ty && tx >= tz) {
    const double s = 2.0 * sqrt(tx);
    q = {(m[2][1] - m[1][2]) / s, 0.25 * s, (m[0][1] + m[1][0]) / s, (m[0][2] + m[2][0]) / s};
  } else if (ty >= tz) {
    const double s = 2.0 * sqrt(ty);
    q = {(m[0][2] - m[2][0]) / s, (m[0][1] + m[1][0]) / s, 0.25 * s, (m[1][2] + m[2][1]) / s};
  } else {
    const double s = 2.0 * sqrt(tz);
    q = {(m[1][0] - m[0][1]) / s, (m[0][2] + m[2][0]) / s, (m[1][2] + m[2][1]) / s, 0.25 * s};
  }
  const double n = sqrt(q.w * q.w + q.x * q.x + q.y * q.y + q.z * q.z);
  const double lead = q.w != 0.0 ? q.w : q.x != 0.0 ? q.x : q.y != 0.0 ? q.y : q.z;
  const double sg = lead < 0.0 ? -n : n;
  return {q.w / sg, q.x / sg, q.y / sg, q.z / sg};
}

__device__ __forceinline__ void load3(const float* p, bool on, float* o) {
  o[0] = on ? p[0] : 0.f; o[1] = on ? p[1] : 0.f; o[2] = on ? p[2] : 0.f;
}

__global__ __launch_bounds__(POSE_THREADS) void lift_rot_kernel(RotArgs A) {
  const int lane = threadIdx.x & 63, J = A.J;
  const long wave = (long)blockIdx.x * (POSE_THREADS / 64) + (threadIdx.x >> 6);
  const int slot = lane / J;
  const int j = lane - slot * J;
  const long n = wave * A.ppw + slot;                                  // pose (frame, inner index)
  const bool valid = slot < A.ppw && n < A.npose;
  // this lane's rows of the tables: selects over compile-time indices (a run-time index into the arguments would copy them to scratch)
  int par = 0, depth = 0;
  double rest[3] = {0.0, 0.0, 0.0}, piax[3] = {0.0, 0.0, 0.0};
#pragma unroll
  for (int k = 1; k < LIFT_MAXJ; ++k) {
    if (j == k) {
      par = A.parent[k]; depth = A.depth[k];
      rest[0] = A.rest[k][0]; rest[1] = A.rest[k][1]; rest[2] = A.rest[k][2];
      piax[0] = A.piax[k][0]; piax[1] = A.piax[k][1]; piax[2] = A.piax[k][2];
    }
  }
  const int plane = valid ? slot * J + par : lane;                     // the parent's lane (the root and idle lanes: their own)
  const unsigned long long mine = valid ? ((1ull << J) - 1ull) << (slot * J) : 0ull;        // the lanes of this pose (J <= 32)
  const float* base = A.poses + (valid ? n : 0) * J * A.C;
  float pj[3], pp[3];
  load3(base + j * A.C, valid, pj);
  load3(base + par * A.C, valid, pp);
  const bool pose_bad = (__ballot(valid && !finite3(pj)) & mine) != 0ull;
  bool regular = true;
  double d[3];
  const bool good = bone_dir(pp, pj, d);                               // (the root: a bone of length 0, never used)
  Q4 q = {1.0, 0.0, 0.0, 0.0}, Rw = q;
  if (j == 0) {                                                        // the root: the frame of its two reference bones against the T-pose frame
    float pa[3], pb[3];
    double da[3], db[3] = {0.0, 0.0, 0.0};
    load3(base + A.a * A.C, valid, pa);
    load3(base + max(A.b, 0) * A.C, valid, pb);
    const bool ga = bone_dir(pj, pa, da);
    const bool gb = A.b >= 0 && bone_dir(pj, pb, db);
    const double s = db[0] * da[0] + db[1] * da[1] + db[2] * da[2];
    const double tx = db[0] - s * da[0], ty = db[1] - s * da[1], tz = db[2] - s * da[2];
    const double tn = sqrt(tx * tx + ty * ty + tz * tz);
    if (ga && gb && tn > 1e-9) {
      const double f2[3] = {tx / tn, ty / tn, tz / tn};
      const double f3[3] = {da[1] * f2[2] - da[2] * f2[1], da[2] * f2[0] - da[0] * f2[2], da[0] * f2[1] - da[1] * f2[0]};
      double m[3][3];
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) m[r][c] = da[r] * A.E[0][c] + f2[r] * A.E[1][c] + f3[r] * A.E[2][c];
      q = quat_of(m);
    } else if (ga) {
      regular = arc(A.E[0], da, A.pia, q) && A.b < 0;                  // without a second reference bone the arc is the rule, not a fallback
    } else {
      regular = false;
    }
    Rw = q;
  }
  for (int lv = 1; lv <= A.levels; ++lv) {                             // parents hand their world rotation down, level by level
    const Q4 P = {__shfl(Rw.w, plane, 64), __shfl(Rw.x, plane, 64), __shfl(Rw.y, plane, 64), __shfl(Rw.z, plane, 64)};
    if (depth == lv) {
      if (good) {
        double u[3];
        qrot_inv(P, d, u);
        regular = arc(rest, u, piax, q);
        Rw = qmul(P, q);
      } else {
        regular = false;
        Rw = P;
      }
    }
  }
  if (pose_bad) { q = {1.0, 0.0, 0.0, 0.0}; regular = false; }
  const bool all_regular = (__ballot(valid && !regular) & mine) == 0ull;
  if (!valid) return;
  float* o = A.quat + (n * J + j) * 4;
  q = {q.w + 0.0, q.x + 0.0, q.y + 0.0, q.z + 0.0};                    // a zero component is +0
  *reinterpret_cast<float4*>(o) = make_float4((float)q.w, (float)q.x, (float)q.y, (float)q.z);
  if (A.rot6d != nullptr) {                                            // columns 0 and 1 of the matrix of q (zeros: +0)
    float* r = A.rot6d + (n * J + j) * 6;
    r[0] = (float)(1.0 - 2.0 * (q.y * q.y + q.z * q.z) + 0.0); r[1] = (float)(2.0 * (q.x * q.y + q.w * q.z) + 0.0);
    r[2] = (float)(2.0 * (q.x * q.z - q.w * q.y) + 0.0); r[3] = (float)(2.0 * (q.x * q.y - q.w * q.z) + 0.0);
    r[4] = (float)(1.0 - 2.0 * (q.x * q.x + q.z * q.z) + 0.0); r[5] = (float)(2.0 * (q.y * q.z + q.w * q.x) + 0.0);
  }
  if (j == 0) A.ok[n] = all_regular ? 1 : 0;
}

struct RotSignArgs {
  float* quat;                   // (Ntot, inner, J, 4), the canonical quaternions, signs flipped in place
  const long* seq_offset;        // (S + 1) device
  long Ntot, tracks;             // tracks = S * inner * J
  int inner, J;
};

__global__ __launch_bounds__(POSE_THREADS) void lift_rot_sign_kernel(RotSignArgs A) {
  const int lane = threadIdx.x & 63;
  const long track = (long)blockIdx.x * (POSE_THREADS / 64) + (threadIdx.x >> 6);      // wave-uniform
  if (track >= A.tracks) return;
  const long per = (long)A.inner * A.J;
  const int s = (int)(track / per);
  const long ij = track - (long)s * per;                               // inner index * J + joint
  const FrameRange r = lift_seq_frames(A.seq_offset, s, A.Ntot);
  unsigned carry = 0u;                                                 // flip of the last frame of the chunk before
  float4 last = make_float4(0.f, 0.f, 0.f, 0.f);                       // ... and its canonical quaternion
  for (long c0 = r.f0; c0 < r.f1; c0 += 64) {
    const long g = c0 + lane;
    const bool on = g < r.f1;
    float4* at = reinterpret_cast<float4*>(A.quat + ((on ? g : r.f0) * per + ij) * 4);
    const float4 c = *at;
    float4 p = make_float4(__shfl_up(c.x, 1, 64), __shfl_up(c.y, 1, 64), __shfl_up(c.z, 1, 64), __shfl_up(c.w, 1, 64));
    if (lane == 0) p = last;
    const double dot = (double)c.x * (double)p.x + (double)c.y * (double)p.y + (double)c.z * (double)p.z + (double)c.w * (double)p.w;
    const unsigned long long votes = __ballot(on && g > r.f0 && dot < 0.0);
    const unsigned flip = (unsigned)(__popcll(votes & (~0ull >> (63 - lane))) & 1) ^ carry;
    if (on && flip) *at = make_float4(-c.x, -c.y, -c.z, -c.w);
    carry ^= (unsigned)(__popcll(votes) & 1);
    last = make_float4(__shfl(c.x, 63, 64), __shfl(c.y, 63, 64), __shfl(c.z, 63, 64), __shfl(c.w, 63, 64));
  }
}

static bool unit3(const float* v, double* o) {                         // fp64 normalisation of a host row; false: non-finite or zero
  const double x = v[0], y = v[1], z = v[2], n = std::sqrt(x * x + y * y + z * z);
  if (!(n > 0.0) || !(n <= 1.0e300)) return false;
  o[0] = x / n; o[1] = y / n; o[2] = z / n;
  return true;
}

// the half-turn axis of a unit direction r: unit(e_k - (e_k . r) r), k the coordinate where |r| is smallest (the lowest on a tie), with the sign
// that makes its first non-zero component positive
static void half_turn_axis(const double* r, double* o) {
  int k = 0;
  for (int c = 1; c < 3; ++c) if (std::fabs(r[c]) < std::fabs(r[k])) k = c;
  double v[3];
  for (int c = 0; c < 3; ++c) v[c] = (c == k ? 1.0 : 0.0) - r[k] * r[c];
  const double n = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
  const double lead = v[0] != 0.0 ? v[0] : v[1] != 0.0 ? v[1] : v[2];
  const double sg = lead < 0.0 ? -n : n;
  for (int c = 0; c < 3; ++c) o[c] = v[c] / sg;
}

}  // namespace mp
using namespace mp;

extern "C" {

int mp_lift_rotations(const float* poses, int64_t Ntot, int inner, int J, int C, const int64_t* seq_offset, int S, const int32_t* parents,
                      const float* rest, int flags, float* quat, float* rot6d, uint8_t* ok, void* stream) {
  static_assert(sizeof(long) == sizeof(int64_t), "LP64");
  MP_CHECK(poses && seq_offset && parents && rest && quat && ok, MP_ERR_ARG, "mp_lift_rotations: null pointer");
  long blocks = 0;
  if (int rc = lift_pose_shape("mp_lift_rotations", (long)Ntot, inner, J, C, S, &blocks)) return rc;
  MP_CHECK(((uintptr_t)quat & 15) == 0, MP_ERR_ARG, "mp_lift_rotations: quat is not 16-byte aligned (a quaternion is stored in one piece)");
  MP_CHECK((flags & ~MP_LIFT_ROT_CONTINUOUS) == 0, MP_ERR_ARG, "mp_lift_rotations: flags=%d (0 or MP_LIFT_ROT_CONTINUOUS)", flags);
  RotArgs a = {};
  MP_CHECK(parents[0] == -1, MP_ERR_ARG, "mp_lift_rotations: parents[0] = %d: joint 0 must be the root (-1)", parents[0]);
  a.parent[0] = 0; a.depth[0] = 0;
  for (int j = 1; j < J; ++j) {
    MP_CHECK(parents[j] >= 0 && parents[j] < j, MP_ERR_ARG, "mp_lift_rotations: parents[%d] = %d: parents precede their children", j, parents[j]);
    MP_CHECK(unit3(rest + 3 * j, a.rest[j]), MP_ERR_ARG, "mp_lift_rotations: rest[%d] is zero or not finite: a bone needs a T-pose direction", j);
    a.parent[j] = (signed char)parents[j];
    a.depth[j] = (signed char)(a.depth[parents[j]] + 1);
    if (a.depth[j] > a.levels) a.levels = a.depth[j];
    half_turn_axis(a.rest[j], a.piax[j]);
  }
  // the root's reference children: a the lowest child of joint 0, b the lowest one whose T-pose direction is not parallel to a's (-1: none)
  a.a = a.b = -1;
  for (int j = 1; j < J && a.a < 0; ++j) if (parents[j] == 0) a.a = j;        // (joint 1 always is one: parents[1] = 0)
  const double* e1 = a.rest[a.a];
  for (int j = a.a + 1; j < J && a.b < 0; ++j) {
    if (parents[j] != 0) continue;
    const double* r = a.rest[j];
    const double cx = e1[1] * r[2] - e1[2] * r[1], cy = e1[2] * r[0] - e1[0] * r[2], cz = e1[0] * r[1] - e1[1] * r[0];
    if (std::sqrt(cx * cx + cy * cy + cz * cz) > 1e-6) a.b = j;
  }
  for (int c = 0; c < 3; ++c) { a.E[0][c] = e1[c]; a.pia[c] = a.piax[a.a][c]; }
  if (a.b >= 0) {
    const double* r = a.rest[a.b];
    const double s = r[0] * e1[0] + r[1] * e1[1] + r[2] * e1[2];
    double t[3] = {r[0] - s * e1[0], r[1] - s * e1[1], r[2] - s * e1[2]};
    const double n = std::sqrt(t[0] * t[0] + t[1] * t[1] + t[2] * t[2]);
    for (int c = 0; c < 3; ++c) a.E[1][c] = t[c] / n;
    a.E[2][0] = e1[1] * a.E[1][2] - e1[2] * a.E[1][1];
    a.E[2][1] = e1[2] * a.E[1][0] - e1[0] * a.E[1][2];
    a.E[2][2] = e1[0] * a.E[1][1] - e1[1] * a.E[1][0];
  }
  a.poses = poses; a.quat = quat; a.rot6d = rot6d; a.ok = ok; a.npose = (long)Ntot * inner; a.J = J; a.C = C; a.ppw = 64 / J;
  const long per_block = (long)a.ppw * (POSE_THREADS / 64);
  const long grid = (a.npose + per_block - 1) / per_block;
  MP_CHECK(grid <= 0x7fffffffL, MP_ERR_ARG, "mp_lift_rotations: %ld poses of %d joints: too many for one launch", a.npose, J);
  RotSignArgs g = {};
  g.quat = quat; g.seq_offset = (const long*)seq_offset; g.Ntot = Ntot; g.inner = inner; g.J = J; g.tracks = (long)S * inner * J;
  const long sign_grid = (g.tracks + POSE_THREADS / 64 - 1) / (POSE_THREADS / 64);
  MP_CHECK(sign_grid <= 0x7fffffffL, MP_ERR_ARG, "mp_lift_rotations: %ld tracks: too many for one launch", g.tracks);
  hipLaunchKernelGGL(lift_rot_kernel, dim3((unsigned)grid), dim3(POSE_THREADS), 0, (hipStream_t)stream, a);
  MP_LAUNCH_CHECK();
  if (flags & MP_LIFT_ROT_CONTINUOUS) {
    hipLaunchKernelGGL(lift_rot_sign_kernel, dim3((unsigned)sign_grid), dim3(POSE_THREADS), 0, (hipStream_t)stream, g);
    MP_LAUNCH_CHECK();
  }
  return MP_OK;
}

}  // extern "C"

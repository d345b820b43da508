// Forward kinematics of (root, quaternions, bone lengths) (include/manipose_hip.h: mp_lift_fk has the rule): the inverse of mp_lift_rotations, in the
// decoder's convention Rw[0] = q[0], Rw[j] = Rw[parent] q[j], p[0] = root, p[j] = p[parent] + len_j Rw[j] rest_j.  The reference has no counterpart
// (its decoder takes 6-D rotations in the window layout: fk_decode.hip).  tests/lift_retime_ref.py states the rule in float64 with 3 x 3 matrices.
//
// lift_fk_kernel: ONE LANE OWNS ONE (pose, joint), 64 / J poses per wave, the mapping and the level-by-level walk of lift_rot_kernel (lift_rot.hip):
// a lane of depth d fetches its parent's WORLD rotation (a unit quaternion, 4 doubles) and its parent's POSITION (3 doubles) from the parent's lane
// with wavefront shuffles, so neither is ever indexed at run time in a per-lane array (which would live in scratch memory) and neither touches
// memory.  The lane's own rows of the tables (parent, depth, T-pose direction) are picked from the kernel arguments by a chain of selects over
// compile-time indices.  "A quaternion of the pose is not usable" is a wave ballot masked to the pose's lanes: no LDS, no atomics, a fixed order,
// identical bits on every call.  Everything between the float32 loads and stores is fp64.  A lane loads one 16-byte quaternion at consecutive
// addresses, one length (per sequence: the pose's lanes read one row; its sequence by lift_seq_of, always inside 0 .. S-1) and the pose's root
// (the same 12 bytes for all lanes of a pose: a broadcast), and stores 12 bytes at consecutive addresses.
// Compiler's figures (hipcc --offload-arch=gfx950 -O3 -Rpass-analysis=kernel-resource-usage): 54 VGPRs, 32 SGPRs, scratch 0 bytes, no spills, no LDS.
// On an MI355X a take of 3000 frames takes 14 us, a launch's latency (tools/lift_bench.py --retime).
#include "lift_geom.h"

namespace mp {

struct FkArgs {
  const float* quat;             // (Ntot, inner, J, 4)
  const float* root;             // (Ntot, inner, 3) or null
  const float* lengths;          // (S, J - 1), or (Ntot, inner, J - 1) with per_pose
  const long* seq_offset;        // (S + 1) device; not read with per_pose
  float* poses;                  // (Ntot, inner, J, 3)
  unsigned char* ok;             // (Ntot, inner)
  long npose;                    // Ntot * inner
  int inner, J, S, ppw, levels, per_pose;
  double rest[LIFT_MAXJ][3];     // unit T-pose directions (row 0 unused)
  signed char parent[LIFT_MAXJ];
  signed char depth[LIFT_MAXJ];
};

struct Q4 { double w, x, y, z; };

__device__ __forceinline__ Q4 qmul(const Q4& a, const Q4& b) {
  return {a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z, a.w * b.x + a.x * b.w + a.y * b.z - a.z * b.y,
          a.w * b.y - a.x * b.z + a.y * b.w + a.z * b.x, a.w * b.z + a.x * b.y - a.y * b.x + a.z * b.w};
}

// R(q) v for a unit quaternion: v + w t + qv x t with t = 2 qv x v  (exactly v for q = (1, 0, 0, 0))
__device__ __forceinline__ void qrot(const Q4& q, const double* v, double* o) {
  const double tx = 2.0 * (q.y * v[2] - q.z * v[1]), ty = 2.0 * (q.z * v[0] - q.x * v[2]), tz = 2.0 * (q.x * v[1] - q.y * v[0]);
  o[0] = v[0] + q.w * tx + (q.y * tz - q.z * ty);
  o[1] = v[1] + q.w * ty + (q.z * tx - q.x * tz);
  o[2] = v[2] + q.w * tz + (q.x * ty - q.y * tx);
}

__global__ __launch_bounds__(POSE_THREADS) void lift_fk_kernel(FkArgs A) {
  const int lane = threadIdx.x & 63, J = A.J;
  const long wave = (long)blockIdx.x * (POSE_THREADS / 64) + (threadIdx.x >> 6);
  const int slot = lane / J;
  const int j = lane - slot * J;
  const long n = wave * A.ppw + slot;                                  // pose (frame, inner index)
  const bool valid = slot < A.ppw && n < A.npose;
  // this lane's rows of the tables: selects over compile-time indices (a run-time index into the arguments would copy them to scratch)
  int par = 0, depth = 0;
  double rest[3] = {0.0, 0.0, 0.0};
#pragma unroll
  for (int k = 1; k < LIFT_MAXJ; ++k) {
    if (j == k) {
      par = A.parent[k]; depth = A.depth[k];
      rest[0] = A.rest[k][0]; rest[1] = A.rest[k][1]; rest[2] = A.rest[k][2];
    }
  }
  const int plane = valid ? slot * J + par : lane;                     // the parent's lane (the root and idle lanes: their own)
  const unsigned long long mine = valid ? ((1ull << J) - 1ull) << (slot * J) : 0ull;        // the lanes of this pose (J <= 32)
  const long at = valid ? n : 0;
  const float4 c = valid ? *reinterpret_cast<const float4*>(A.quat + (at * J + j) * 4) : make_float4(1.f, 0.f, 0.f, 0.f);
  const float cq[4] = {c.x, c.y, c.z, c.w};
  double n2;
  const bool good = lift_quat_ok(cq, n2);
  const bool pose_bad = (__ballot(valid && !good) & mine) != 0ull;
  const double nq = good ? sqrt(n2) : 1.0;
  const Q4 q = good ? Q4{(double)c.x / nq, (double)c.y / nq, (double)c.z / nq, (double)c.w / nq} : Q4{1.0, 0.0, 0.0, 0.0};
  float r32[3] = {0.f, 0.f, 0.f};
  if (valid && A.root != nullptr) { r32[0] = A.root[at * 3]; r32[1] = A.root[at * 3 + 1]; r32[2] = A.root[at * 3 + 2]; }
  double len = 0.0;
  if (valid && j > 0) {
    const long row = A.per_pose ? at : (long)lift_seq_of(A.seq_offset, A.S, at / A.inner);
    len = (double)A.lengths[row * (J - 1) + (j - 1)];
  }
  const double v[3] = {len * rest[0], len * rest[1], len * rest[2]};
  Q4 Rw = q;
  double p[3] = {(double)r32[0], (double)r32[1], (double)r32[2]};
  for (int lv = 1; lv <= A.levels; ++lv) {                             // parents hand their world rotation and position down, level by level
    const Q4 P = {__shfl(Rw.w, plane, 64), __shfl(Rw.x, plane, 64), __shfl(Rw.y, plane, 64), __shfl(Rw.z, plane, 64)};
    const double pp[3] = {__shfl(p[0], plane, 64), __shfl(p[1], plane, 64), __shfl(p[2], plane, 64)};
    if (depth == lv) {
      Rw = qmul(P, q);
      double o[3];
      qrot(Rw, v, o);
      p[0] = pp[0] + o[0]; p[1] = pp[1] + o[1]; p[2] = pp[2] + o[2];
    }
  }
  if (!valid) return;
  float* o = A.poses + (at * J + j) * 3;
  if (pose_bad) {                                                      // every joint on the root, its bits
    o[0] = r32[0]; o[1] = r32[1]; o[2] = r32[2];
  } else {
    o[0] = (float)p[0]; o[1] = (float)p[1]; o[2] = (float)p[2];
  }
  if (j == 0) A.ok[at] = pose_bad ? 0 : 1;
}

static bool fk_unit3(const float* v, double* o) {                      // fp64 normalisation of a host row; false: non-finite or zero
  const double x = v[0], y = v[1], z = v[2], n = std::sqrt(x * x + y * y + z * z);
  if (!(n > 0.0) || !(n <= 1.0e300)) return false;
  o[0] = x / n; o[1] = y / n; o[2] = z / n;
  return true;
}

}  // namespace mp
using namespace mp;

extern "C" {

int mp_lift_fk(const float* quat, const float* root, const float* lengths, int64_t Ntot, int inner, int J, const int64_t* seq_offset, int S,
               const int32_t* parents, const float* rest, int flags, float* poses, uint8_t* ok, void* stream) {
  static_assert(sizeof(long) == sizeof(int64_t), "LP64");
  MP_CHECK(quat && lengths && rest && poses && ok, MP_ERR_ARG, "mp_lift_fk: null pointer (quat, lengths, rest, poses and ok are all needed)");
  MP_CHECK((flags & ~MP_LIFT_FK_POSE_LENGTHS) == 0, MP_ERR_ARG, "mp_lift_fk: flags=%d (0 or MP_LIFT_FK_POSE_LENGTHS)", flags);
  const bool per_pose = (flags & MP_LIFT_FK_POSE_LENGTHS) != 0;
  MP_CHECK(per_pose || seq_offset != nullptr, MP_ERR_ARG, "mp_lift_fk: null seq_offset (a length table per sequence needs the sequences)");
  long blocks = 0;
  if (int rc = lift_pose_shape("mp_lift_fk", (long)Ntot, inner, J, 3, per_pose ? 1 : S, &blocks)) return rc;
  MP_CHECK(((uintptr_t)quat & 15) == 0, MP_ERR_ARG, "mp_lift_fk: quat is not 16-byte aligned (a quaternion is loaded in one piece)");
  FkArgs a = {};
  if (int rc = rigid_parents("mp_lift_fk", parents, J, a.parent)) return rc;
  a.parent[0] = 0; a.depth[0] = 0;
  for (int j = 1; j < J; ++j) {
    MP_CHECK(fk_unit3(rest + 3 * j, a.rest[j]), MP_ERR_ARG, "mp_lift_fk: rest[%d] is zero or not finite: a bone needs a T-pose direction", j);
    a.depth[j] = (signed char)(a.depth[parents[j]] + 1);
    if (a.depth[j] > a.levels) a.levels = a.depth[j];
  }
  const uintptr_t po = (uintptr_t)poses, pe = po + (uintptr_t)Ntot * inner * J * 3 * sizeof(float);
  const uintptr_t qo = (uintptr_t)quat, qe = qo + (uintptr_t)Ntot * inner * J * 4 * sizeof(float);
  MP_CHECK(pe <= qo || qe <= po, MP_ERR_ARG, "mp_lift_fk: poses and quat overlap (the call is out of place)");
  a.quat = quat; a.root = root; a.lengths = lengths; a.seq_offset = (const long*)seq_offset; a.poses = poses; a.ok = ok;
  a.npose = (long)Ntot * inner; a.inner = inner; a.J = J; a.S = S; a.ppw = 64 / J; a.per_pose = per_pose ? 1 : 0;
  const long per_block = (long)a.ppw * (POSE_THREADS / 64);
  const long grid = (a.npose + per_block - 1) / per_block;
  MP_CHECK(grid <= 0x7fffffffL, MP_ERR_ARG, "mp_lift_fk: %ld poses of %d joints: too many for one launch", a.npose, J);
  hipLaunchKernelGGL(lift_fk_kernel, dim3((unsigned)grid), dim3(POSE_THREADS), 0, (hipStream_t)stream, a);
  MP_LAUNCH_CHECK();
  return MP_OK;
}

}  // extern "C"

// The pose layout the lifting kernels share (lift.hip, lift_rigid.hip, lift_place.hip): poses are (Ntot, inner, J, C) floats, C = 3 or 4 (channel 3
// is a hypothesis' score), the Ntot frames belong to S sequences whose first frames are the device table seq_offset (S + 1), and in the pose
// kernels ONE LANE OWNS ONE POSE: lane i of the grid has frame i / inner.
#pragma once
#include "common.h"

namespace mp {

constexpr int LIFT_MAXJ = 32;        // joints of a skeleton: parent / mirror tables travel in the kernel arguments
constexpr int POSE_THREADS = 256;    // lanes of a workgroup of the pose kernels

// the sequence of frame g: last s with seq_offset[s] <= g (always inside 0 .. S-1, whatever the device table holds)
__device__ __forceinline__ int lift_seq_of(const long* seq_offset, int S, long g) {
  int lo = 0, hi = S - 1;
  while (lo < hi) {
    const int m = (lo + hi + 1) >> 1;
    if (seq_offset[m] <= g) lo = m; else hi = m - 1;
  }
  return lo;
}

// frames [f0, f1) of sequence s.  The offsets are device data no host check has seen: clamped to the Ntot frames the caller vouches for, so no
// frame outside the poses is touched
struct FrameRange { long f0, f1; };
__device__ __forceinline__ FrameRange lift_seq_frames(const long* seq_offset, int s, long Ntot) {
  const long f0 = min(max(seq_offset[s], 0L), Ntot);
  return {f0, min(max(seq_offset[s + 1], f0), Ntot)};
}

// host: the shape of (Ntot, inner, J, C) poses in S sequences, and the workgroups of a one-lane-per-pose launch over them
static int lift_pose_shape(const char* who, long Ntot, int inner, int J, int C, int S, long* blocks) {
  MP_CHECK(C == 3 || C == 4, MP_ERR_ARG, "%s: C=%d (3: poses, 4: hypotheses with their score)", who, C);
  MP_CHECK(J >= 2 && J <= LIFT_MAXJ, MP_ERR_ARG, "%s: J=%d outside 2..%d", who, J, LIFT_MAXJ);
  MP_CHECK(Ntot > 0 && inner > 0 && S > 0 && (long)S <= Ntot, MP_ERR_ARG, "%s: Ntot=%ld inner=%d S=%d out of range", who, Ntot, inner, S);
  MP_CHECK(Ntot <= 0x7fffffffL * (long)POSE_THREADS / inner, MP_ERR_ARG, "%s: %ld frames of %d poses: too many for one launch", who, Ntot, inner);
  *blocks = (Ntot * inner + POSE_THREADS - 1) / POSE_THREADS;
  MP_CHECK(*blocks <= 0x7fffffffL, MP_ERR_ARG, "%s: %ld poses: too many for one launch", who, Ntot * inner);
  return MP_OK;
}

// host: a skeleton's parent table (J) copied into a kernel's arguments: parents precede children, exactly one root (joint 0)
static int rigid_parents(const char* who, const int* parents, int J, signed char* dst) {
  MP_CHECK(parents != nullptr, MP_ERR_ARG, "%s: null parent table", who);
  MP_CHECK(J >= 2 && J <= LIFT_MAXJ, MP_ERR_ARG, "%s: J=%d outside 2..%d", who, J, LIFT_MAXJ);
  MP_CHECK(parents[0] == -1, MP_ERR_ARG, "%s: parents[0] = %d: joint 0 must be the root (-1)", who, parents[0]);
  for (int j = 1; j < J; ++j) {
    MP_CHECK(parents[j] >= 0 && parents[j] < j, MP_ERR_ARG, "%s: parents[%d] = %d: parents precede their children", who, j, parents[j]);
    dst[j] = (signed char)parents[j];
  }
  dst[0] = -1;
  return MP_OK;
}

}  // namespace mp

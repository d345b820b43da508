// Rigid lifting (include/manipose_hip.h: mp_lift_rigid, mp_bone_length_means): after mp_lift_merge every sequence gets ONE table of J - 1 bone
// lengths, and every pose it emitted - the merged pose and every hypothesis - is re-assembled along its own bone directions with those lengths.
// The reference has no counterpart (its hpe/viz.py renders the hypotheses as they come); the quantity this holds at zero is the MPSCE its test
// pass reports (segments_time_consistency, hpe/mh_so3_hpe/metrics/regularizations.py:8-60).
//
// lift_rigid_kernel: ONE LANE OWNS ONE POSE.  It loads all J x 3 coordinates into registers before it stores anything, so updating the pose in
// place has no read-after-write hazard, and walks the tree three times over that one register array:
//   1. j = J-1 .. 1:  a[j] <- p[j] - p[parent[j]]          (children first: parents precede children, so p[parent] is still the INPUT position)
//   2. j = 1 .. J-1:  a[j] <- a[j] / sqrtf(a[j] . a[j]), or for a bone of length 0 / non-finite length the direction of the parent's bone
//                     ((0, 0, 1) under the root), which step 2 has already left in a[parent[j]]
//   3. j = 1 .. J-1:  a[j] <- a[parent[j]] + L[j-1] a[j]     (a[parent] is already the OUTPUT position; a[0], the root, was never touched)
// The parent table is a kernel argument (wave-uniform); a[parent[j]] is a chain of selects over the compile-time indices k < j, because a
// register array indexed at run time would live in scratch memory.  sqrtf and the division are the correctly rounded ones (no v_rsq).
// A pose is (C = 3 or 4) x J floats; channel 3 (the score of a hypothesis) is neither read nor written.  A lane's loads are 12-byte pieces
// 4 C J bytes apart from its neighbours': every byte of the lines is used, but over 3 J instructions, not one - the whole workload is a few
// MB (3000 frames x 5 hypotheses x 272 B), nobody has measured it, and no rate is claimed.
//
// bone_length_means_kernel: one workgroup per sequence.  Thread t adds up the bone lengths of frames t, t + 256, ... of its sequence in fp64
// (differences, dot product and square root in fp64 too), the 64 lanes of a wave are added in a fixed butterfly order, the 4 waves in wave
// order: a fixed summation order and no atomics, identical bits on every call.
#include "lift_common.h"
#include "../../include/manipose_hip.h"

namespace mp {

struct RigidArgs {
  float* poses;                  // (Ntot, inner, J, C), updated in place
  const long* seq_offset;        // (S + 1) device
  const float* lengths;          // (S, J - 1) device
  long npose;                    // Ntot * inner
  int inner, J, C, S;
  signed char parent[LIFT_MAXJ];
};

// a[par] for par < j: selects over compile-time indices (par is wave-uniform)
template <int JT>
__device__ __forceinline__ void rigid_pick(const float (&a)[JT][3], int j, int par, float& x, float& y, float& z) {
  x = a[0][0]; y = a[0][1]; z = a[0][2];
#pragma unroll
  for (int k = 1; k < JT - 1; ++k) {
    if (k < j && par == k) { x = a[k][0]; y = a[k][1]; z = a[k][2]; }
  }
}

template <int JT>
__global__ __launch_bounds__(POSE_THREADS) void lift_rigid_kernel(RigidArgs A) {
  const long i = (long)blockIdx.x * POSE_THREADS + threadIdx.x;        // pose (frame, inner index)
  if (i >= A.npose) return;
  const long g = i / A.inner;                                          // frame
  const int s = lift_seq_of(A.seq_offset, A.S, g);
  const float* L = A.lengths + (long)s * (A.J - 1);
  float* base = A.poses + i * A.J * A.C;
  float a[JT][3];
#pragma unroll
  for (int j = 0; j < JT; ++j) {
    if (j < A.J) {
      a[j][0] = base[j * A.C]; a[j][1] = base[j * A.C + 1]; a[j][2] = base[j * A.C + 2];
    } else {
      a[j][0] = a[j][1] = a[j][2] = 0.f;
    }
  }
#pragma unroll
  for (int j = JT - 1; j >= 1; --j) {
    if (j < A.J) {
      float px, py, pz;
      rigid_pick<JT>(a, j, A.parent[j], px, py, pz);
      a[j][0] -= px; a[j][1] -= py; a[j][2] -= pz;
    }
  }
#pragma unroll
  for (int j = 1; j < JT; ++j) {
    if (j < A.J) {
      const int par = A.parent[j];
      float ux, uy, uz;
      rigid_pick<JT>(a, j, par, ux, uy, uz);                           // the parent's direction; the root has none
      if (par == 0) { ux = 0.f; uy = 0.f; uz = 1.f; }
      const float n = sqrtf(a[j][0] * a[j][0] + a[j][1] * a[j][1] + a[j][2] * a[j][2]);
      if (n > 0.f && n <= 3.0e38f) { ux = a[j][0] / n; uy = a[j][1] / n; uz = a[j][2] / n; }      // (false for a NaN too)
      a[j][0] = ux; a[j][1] = uy; a[j][2] = uz;
    }
  }
  // (a[0] holds the root POSITION during step 2; no lane reads it as a direction: par == 0 takes (0, 0, 1))
#pragma unroll
  for (int j = 1; j < JT; ++j) {
    if (j < A.J) {
      float qx, qy, qz;
      rigid_pick<JT>(a, j, A.parent[j], qx, qy, qz);
      const float len = L[j - 1];
      a[j][0] = qx + len * a[j][0]; a[j][1] = qy + len * a[j][1]; a[j][2] = qz + len * a[j][2];
      base[j * A.C] = a[j][0]; base[j * A.C + 1] = a[j][1]; base[j * A.C + 2] = a[j][2];
    }
  }
}

struct BoneMeanArgs {
  const float* poses;            // (Ntot, J, 3)
  const long* seq_offset;        // (S + 1) device
  const long* seq_real;          // (S) device or null: frames of the sequence that count (the first seq_real[s] of them)
  float* lengths;                // (S, J - 1)
  long Ntot;
  int J;
  signed char parent[LIFT_MAXJ];
};

__device__ __forceinline__ double wave_sum_f64(double v) {             // fixed butterfly: the same order on every call
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}

__global__ __launch_bounds__(POSE_THREADS) void bone_length_means_kernel(BoneMeanArgs A) {
  __shared__ double part[POSE_THREADS / 64][LIFT_MAXJ];
  const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const FrameRange r = lift_seq_frames(A.seq_offset, s, A.Ntot);
  const long f0 = r.f0, len = r.f1 - f0;
  long n = A.seq_real != nullptr ? A.seq_real[s] : len;
  n = n < len ? n : len;                                               // never past the sequence's own frames
  const int J3 = A.J * 3;
  for (int b = 0; b < A.J - 1; ++b) {                                  // one bone at a time: no per-thread array, the frame rows stay in L1 / L2
    const int j = b + 1, p = A.parent[j];
    double acc = 0.0;
    for (long f = tid; f < n; f += POSE_THREADS) {
      const float* r = A.poses + (f0 + f) * J3;
      const double dx = (double)r[j * 3] - (double)r[p * 3], dy = (double)r[j * 3 + 1] - (double)r[p * 3 + 1],
                   dz = (double)r[j * 3 + 2] - (double)r[p * 3 + 2];
      acc += sqrt(dx * dx + dy * dy + dz * dz);
    }
    acc = wave_sum_f64(acc);
    if (lane == 0) part[wv][b] = acc;
  }
  __syncthreads();
  if (tid < A.J - 1) {
    double t = part[0][tid];
    for (int w = 1; w < POSE_THREADS / 64; ++w) t += part[w][tid];
    A.lengths[(long)s * (A.J - 1) + tid] = n > 0 ? (float)(t / (double)n) : 0.f;
  }
}

}  // namespace mp
using namespace mp;

extern "C" {

int mp_lift_rigid(float* poses, int64_t Ntot, int inner, int J, int C, const int64_t* seq_offset, int S, const float* lengths,
                  const int32_t* parents, void* stream) {
  static_assert(sizeof(long) == sizeof(int64_t), "LP64");
  MP_CHECK(poses && seq_offset && lengths, MP_ERR_ARG, "mp_lift_rigid: null pointer");
  long blocks = 0;
  if (int rc = lift_pose_shape("mp_lift_rigid", (long)Ntot, inner, J, C, S, &blocks)) return rc;
  RigidArgs a = {};
  if (int rc = rigid_parents("mp_lift_rigid", parents, J, a.parent)) return rc;
  a.poses = poses; a.seq_offset = (const long*)seq_offset; a.lengths = lengths; a.npose = (long)Ntot * inner;
  a.inner = inner; a.J = J; a.C = C; a.S = S;
  if (J <= 17) hipLaunchKernelGGL(lift_rigid_kernel<17>, dim3((unsigned)blocks), dim3(POSE_THREADS), 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(lift_rigid_kernel<LIFT_MAXJ>, dim3((unsigned)blocks), dim3(POSE_THREADS), 0, (hipStream_t)stream, a);
  MP_LAUNCH_CHECK();
  return MP_OK;
}

int mp_bone_length_means(const float* poses, int64_t Ntot, int J, const int64_t* seq_offset, const int64_t* seq_real, int S, const int32_t* parents,
                         float* lengths, void* stream) {
  MP_CHECK(poses && seq_offset && lengths, MP_ERR_ARG, "mp_bone_length_means: null pointer");
  MP_CHECK(S > 0 && Ntot > 0, MP_ERR_ARG, "mp_bone_length_means: Ntot=%ld S=%d out of range", (long)Ntot, S);
  BoneMeanArgs a = {};
  if (int rc = rigid_parents("mp_bone_length_means", parents, J, a.parent)) return rc;
  a.poses = poses; a.seq_offset = (const long*)seq_offset; a.seq_real = (const long*)seq_real; a.lengths = lengths; a.Ntot = Ntot;
  a.J = J;
  hipLaunchKernelGGL(bone_length_means_kernel, dim3((unsigned)S), dim3(POSE_THREADS), 0, (hipStream_t)stream, a);
  MP_LAUNCH_CHECK();
  return MP_OK;
}

}  // extern "C"

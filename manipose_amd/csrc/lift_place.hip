// Placing lifted sequences in the scene (include/manipose_hip.h: mp_lift_place, mp_lift_world): what mp_lift_merge / mp_lift_rigid leave is
// root-relative and in the camera's frame.  mp_lift_place fits, per pose, the root translation whose pinhole projection meets the sequence's own
// 2-D keypoints, and reports the reprojection error under the full H36M camera model (the reference's project_to_2d,
// hpe/mh_so3_hpe/data/camera.py:35-70; project_to_2d_linear :73-95); mp_lift_world is the reference's camera_to_world (:31-32, qrot of
// data/quaternion.py:6-20) with the fitted translation added first, and the floor line of its prepare_prediction_for_viz (z -= min z).
//
// ONE LANE OWNS ONE POSE, as in lift_rigid.hip; a pose is (C = 3 or 4) x J floats and channel 3 (a hypothesis' score) is neither read nor
// written.  Everything between the float32 loads and the float32 stores is fp64: 17 joints and a few dozen operations per pose, so the only
// error against a float64 statement on the same inputs is the final rounding (the fit's condition number is a few hundred; a float32 solve of
// the same construction misses by 2e-5 m).  The joints are read twice (sums, then reprojection) instead of being kept in a register array.
// The workload is a few MB (3000 frames x 5 hypotheses x 272 B), nobody has measured it, and no rate is claimed.
//
// Floor (mode 1): the minimum is taken from the STORED float32 values by a second kernel - MP_LIFT_WORLD_SHARES workgroups per sequence, each
// over one contiguous share of the sequence's poses, DPP inside a wave, LDS across the 4 waves, one partial per workgroup - and the third
// kernel merges a sequence's partials in share order, subtracts, and writes floor[s].  No atomics: the same bits on every call.
#include "lift_common.h"
#include "../../include/manipose_hip.h"

namespace mp {

constexpr int FLOOR_SHARES = MP_LIFT_WORLD_SHARES;

// torch.clamp(x, -1, 1): a NaN stays a NaN
__device__ __forceinline__ double place_clamp1(double x) { return x < -1.0 ? -1.0 : (x > 1.0 ? 1.0 : x); }

struct PlaceArgs {
  const float* poses;            // (Ntot, inner, J, C)
  const float* kp;               // (Ntot, J, 2)
  const long* seq_offset;        // (S + 1) device
  const float* intr;             // (S, 9) device
  const float* weights;          // (J) device or null
  float* traj;                   // (Ntot, inner, 3)
  float* reproj;                 // (Ntot, inner)
  unsigned char* ok;             // (Ntot, inner)
  long npose;                    // Ntot * inner
  int inner, J, C, S, distort;
};

__global__ __launch_bounds__(POSE_THREADS) void lift_place_kernel(PlaceArgs A) {
  const long i = (long)blockIdx.x * POSE_THREADS + threadIdx.x;        // pose (frame, inner index)
  if (i >= A.npose) return;
  const long g = i / A.inner;                                          // frame
  const int s = lift_seq_of(A.seq_offset, A.S, g);
  const float* cam = A.intr + (long)s * 9;
  const double fx = cam[0], fy = cam[1], cx = cam[2], cy = cam[3];
  const float* P = A.poses + i * A.J * A.C;
  const float* U = A.kp + g * A.J * 2;
  double W = 0.0, Sa = 0.0, Sb = 0.0, Q = 0.0, Sx = 0.0, Sy = 0.0, Sc = 0.0;
  for (int j = 0; j < A.J; ++j) {                                      // sums in joint order
    const double w = A.weights != nullptr ? (double)A.weights[j] : 1.0;
    if (w == 0.0) continue;                                            // a joint of weight 0 is not looked at
    const double X = P[j * A.C], Y = P[j * A.C + 1], Z = P[j * A.C + 2];
    const double a = ((double)U[2 * j] - cx) / fx, b = ((double)U[2 * j + 1] - cy) / fy;
    const double ex = X - a * Z, ey = Y - b * Z;
    W += w; Sa += w * a; Sb += w * b; Q += w * (a * a + b * b);
    Sx += w * ex; Sy += w * ey; Sc += w * (a * ex + b * ey);
  }
  // [[W, 0, -Sa], [0, W, -Sb], [-Sa, -Sb, Q]] t = [-Sx, -Sy, Sc]; its determinant is W (W Q - Sa^2 - Sb^2)
  const double WQ = W * Q, det = WQ - Sa * Sa - Sb * Sb;
  const bool finite = __builtin_isfinite(W) && __builtin_isfinite(Sa) && __builtin_isfinite(Sb) && __builtin_isfinite(Q) && __builtin_isfinite(Sx) &&
                      __builtin_isfinite(Sy) && __builtin_isfinite(Sc);
  double tx = 0.0, ty = 0.0, tz = 0.0, err = 0.0;
  unsigned char ok = 0;
  if (W > 0.0 && finite && det > 1e-9 * WQ) {
    tz = (W * Sc - Sa * Sx - Sb * Sy) / det;
    tx = (Sa * tz - Sx) / W;
    ty = (Sb * tz - Sy) / W;
    const double k1 = cam[4], k2 = cam[5], k3 = cam[6], p1 = cam[7], p2 = cam[8];
    ok = 1;
    for (int j = 0; j < A.J; ++j) {
      const double w = A.weights != nullptr ? (double)A.weights[j] : 1.0;
      if (w == 0.0) continue;
      const double X = (double)P[j * A.C] + tx, Y = (double)P[j * A.C + 1] + ty, Z = (double)P[j * A.C + 2] + tz;
      if (!(Z > 0.0)) ok = 0;                                          // behind the camera: t and the error are stored as computed
      const double xx = place_clamp1(X / Z), yy = place_clamp1(Y / Z);
      double px = xx, py = yy;
      if (A.distort) {
        const double r2 = xx * xx + yy * yy;
        const double m = 1.0 + (k1 * r2 + k2 * (r2 * r2) + k3 * (r2 * r2 * r2)) + (p1 * xx + p2 * yy);
        px = xx * m + p1 * r2;
        py = yy * m + p2 * r2;
      }
      const double du = fx * px + cx - (double)U[2 * j], dv = fy * py + cy - (double)U[2 * j + 1];
      err += w * sqrt(du * du + dv * dv);
    }
    err /= W;
  }
  A.traj[i * 3] = (float)tx; A.traj[i * 3 + 1] = (float)ty; A.traj[i * 3 + 2] = (float)tz;
  A.reproj[i] = (float)err;
  A.ok[i] = ok;
}

struct WorldArgs {
  float* poses;                  // (Ntot, inner, J, C), updated in place
  const float* traj;             // (Ntot, inner, 3) or null
  const long* seq_offset;        // (S + 1) device
  const float* quat;             // (S, 4) device, (w, x, y, z)
  const float* trans;            // (S, 3) device or null
  float* floor;                  // (S) device: read in mode 2, written in mode 1
  float* partial;                // (S, FLOOR_SHARES) device, mode 1
  long npose, Ntot;
  int inner, J, C, S, floor_mode;
};

// p <- qrot(q, p + traj) + trans; mode 2 also subtracts the caller's floor from the float32 z it would have stored
__global__ __launch_bounds__(POSE_THREADS) void lift_world_kernel(WorldArgs A) {
  const long i = (long)blockIdx.x * POSE_THREADS + threadIdx.x;
  if (i >= A.npose) return;
  const int s = lift_seq_of(A.seq_offset, A.S, i / A.inner);
  const float* q = A.quat + (long)s * 4;
  const double qw = q[0], qx = q[1], qy = q[2], qz = q[3];
  const bool move = A.traj != nullptr, shift = A.trans != nullptr;
  const double ax = move ? (double)A.traj[i * 3] : 0.0, ay = move ? (double)A.traj[i * 3 + 1] : 0.0, az = move ? (double)A.traj[i * 3 + 2] : 0.0;
  const double bx = shift ? (double)A.trans[s * 3] : 0.0, by = shift ? (double)A.trans[s * 3 + 1] : 0.0, bz = shift ? (double)A.trans[s * 3 + 2] : 0.0;
  const float fl = A.floor_mode == 2 ? A.floor[s] : 0.f;
  float* base = A.poses + i * A.J * A.C;
  for (int j = 0; j < A.J; ++j) {
    double vx = base[j * A.C], vy = base[j * A.C + 1], vz = base[j * A.C + 2];
    if (move) { vx += ax; vy += ay; vz += az; }
    const double ux = qy * vz - qz * vy, uy = qz * vx - qx * vz, uz = qx * vy - qy * vx;           // q_xyz x v
    const double wx = qy * uz - qz * uy, wy = qz * ux - qx * uz, wz = qx * uy - qy * ux;           // q_xyz x (q_xyz x v)
    double rx = vx + 2.0 * (qw * ux + wx), ry = vy + 2.0 * (qw * uy + wy), rz = vz + 2.0 * (qw * uz + wz);
    if (shift) { rx += bx; ry += by; rz += bz; }
    float z = (float)rz;
    if (A.floor_mode == 2) z = z - fl;
    base[j * A.C] = (float)rx; base[j * A.C + 1] = (float)ry; base[j * A.C + 2] = z;
  }
}

// workgroup (c, s): the minimum stored z over share c of the poses of sequence s (+inf for an empty share)
__global__ __launch_bounds__(POSE_THREADS) void floor_partial_kernel(WorldArgs A) {
  __shared__ float w_min[POSE_THREADS / 64];
  const int c = blockIdx.x % FLOOR_SHARES, s = blockIdx.x / FLOOR_SHARES, tid = threadIdx.x;
  const FrameRange r = lift_seq_frames(A.seq_offset, s, A.Ntot);
  const long f0 = r.f0, f1 = r.f1;
  const long n = (f1 - f0) * A.inner, per = (n + FLOOR_SHARES - 1) / FLOOR_SHARES;
  const long p0 = f0 * A.inner + min((long)c * per, n), p1 = f0 * A.inner + min((long)(c + 1) * per, n);
  float m = __builtin_inff();
  for (long p = p0 + tid; p < p1; p += POSE_THREADS) {
    const float* base = A.poses + p * A.J * A.C;
    for (int j = 0; j < A.J; ++j) m = fminf(m, base[j * A.C + 2]);
  }
  m = -wave_max(-m);
  if ((tid & 63) == 0) w_min[tid >> 6] = m;
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < POSE_THREADS / 64; ++w) m = fminf(m, w_min[w]);
    A.partial[(long)s * FLOOR_SHARES + c] = m;
  }
}

__device__ __forceinline__ float floor_merge(const float* partial, int s) {
  float m = partial[(long)s * FLOOR_SHARES];
  for (int c = 1; c < FLOOR_SHARES; ++c) m = fminf(m, partial[(long)s * FLOOR_SHARES + c]);       // in share order
  return m;
}

// z <- z - floor[s], one float32 subtraction; mode 1: floor[s] is the merge of the sequence's partials, written by lane s of the grid
__global__ __launch_bounds__(POSE_THREADS) void floor_apply_kernel(WorldArgs A) {
  const long i = (long)blockIdx.x * POSE_THREADS + threadIdx.x;
  if (i >= A.npose) return;
  const int s = lift_seq_of(A.seq_offset, A.S, i / A.inner);
  const float fl = A.floor_mode == 1 ? floor_merge(A.partial, s) : A.floor[s];
  float* base = A.poses + i * A.J * A.C;
  for (int j = 0; j < A.J; ++j) base[j * A.C + 2] = base[j * A.C + 2] - fl;
  if (A.floor_mode == 1 && i < A.S) A.floor[i] = floor_merge(A.partial, (int)i);                  // (S <= Ntot <= npose: every sequence has its lane)
}

}  // namespace mp
using namespace mp;

extern "C" {

int mp_lift_place(const float* poses, int64_t Ntot, int inner, int J, int C, const float* kp, const int64_t* seq_offset, int S, const float* intr,
                  const float* weights, int distort, float* traj, float* reproj, uint8_t* ok, void* stream) {
  static_assert(sizeof(long) == sizeof(int64_t), "LP64");
  MP_CHECK(poses && kp && seq_offset && intr && traj && reproj && ok, MP_ERR_ARG, "mp_lift_place: null pointer");
  MP_CHECK(distort == 0 || distort == 1, MP_ERR_ARG, "mp_lift_place: distort=%d (0: project_to_2d_linear, 1: project_to_2d)", distort);
  long blocks = 0;
  if (int rc = lift_pose_shape("mp_lift_place", (long)Ntot, inner, J, C, S, &blocks)) return rc;
  PlaceArgs a = {};
  a.poses = poses; a.kp = kp; a.seq_offset = (const long*)seq_offset; a.intr = intr; a.weights = weights;
  a.traj = traj; a.reproj = reproj; a.ok = ok; a.npose = (long)Ntot * inner;
  a.inner = inner; a.J = J; a.C = C; a.S = S; a.distort = distort;
  hipLaunchKernelGGL(lift_place_kernel, dim3((unsigned)blocks), dim3(POSE_THREADS), 0, (hipStream_t)stream, a);
  MP_LAUNCH_CHECK();
  return MP_OK;
}

int mp_lift_world(float* poses, int64_t Ntot, int inner, int J, int C, const float* traj, const int64_t* seq_offset, int S, const float* quat,
                  const float* trans, int floor_mode, float* floor, float* scratch, int64_t scratch_floats, void* stream) {
  MP_CHECK(poses && seq_offset && quat, MP_ERR_ARG, "mp_lift_world: null pointer");
  MP_CHECK(floor_mode >= 0 && floor_mode <= 2, MP_ERR_ARG, "mp_lift_world: floor_mode=%d (0 none, 1 compute, 2 given)", floor_mode);
  MP_CHECK(floor_mode == 0 || floor != nullptr, MP_ERR_ARG, "mp_lift_world: floor_mode=%d without a floor table: null pointer", floor_mode);
  long blocks = 0;
  if (int rc = lift_pose_shape("mp_lift_world", (long)Ntot, inner, J, C, S, &blocks)) return rc;
  MP_CHECK(floor_mode != 1 || (scratch != nullptr && scratch_floats >= (int64_t)S * FLOOR_SHARES), MP_ERR_ARG,
           "mp_lift_world: floor_mode=1 needs %ld scratch floats (S * MP_LIFT_WORLD_SHARES), got %ld", (long)S * FLOOR_SHARES,
           scratch ? (long)scratch_floats : 0L);
  MP_CHECK(floor_mode != 1 || S <= 0x7fffffff / FLOOR_SHARES, MP_ERR_ARG, "mp_lift_world: floor_mode=1 with S=%d sequences: too many for one launch", S);
  WorldArgs a = {};
  a.poses = poses; a.traj = traj; a.seq_offset = (const long*)seq_offset; a.quat = quat; a.trans = trans; a.floor = floor;
  a.partial = scratch; a.npose = (long)Ntot * inner; a.Ntot = Ntot;
  a.inner = inner; a.J = J; a.C = C; a.S = S; a.floor_mode = floor_mode;
  hipLaunchKernelGGL(lift_world_kernel, dim3((unsigned)blocks), dim3(POSE_THREADS), 0, (hipStream_t)stream, a);
  MP_LAUNCH_CHECK();
  if (floor_mode == 1) {
    hipLaunchKernelGGL(floor_partial_kernel, dim3((unsigned)S * FLOOR_SHARES), dim3(POSE_THREADS), 0, (hipStream_t)stream, a);
    MP_LAUNCH_CHECK();
    hipLaunchKernelGGL(floor_apply_kernel, dim3((unsigned)blocks), dim3(POSE_THREADS), 0, (hipStream_t)stream, a);
    MP_LAUNCH_CHECK();
  }
  return MP_OK;
}

}  // extern "C"

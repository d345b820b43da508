// Placing lifted sequences in the scene (include/manipose_hip.h: mp_lift_place, mp_lift_place_refine, mp_lift_world): what mp_lift_merge /
// mp_lift_rigid leave is root-relative and in the camera's frame.  The fit kernel finds, per pose, the root translation whose pinhole projection
// meets the sequence's own 2-D keypoints - that fit is linear in t - and reports the reprojection error under the full H36M camera model (the
// reference's project_to_2d, hpe/mh_so3_hpe/data/camera.py:35-70; project_to_2d_linear :73-95); mp_lift_world is the reference's camera_to_world
// (:31-32, qrot of data/quaternion.py:6-20) with the fitted translation added first, and the floor line of its prepare_prediction_for_viz
// (z -= min z).
//
// ONE FIT KERNEL serves both entry points: mp_lift_place is mp_lift_place_refine with start = start_ok = steps = null and iters = 0.  Under the
// H36M calibration (k1 ~ -0.2, k2 ~ 0.25) the pinhole fit and the full model disagree by centimetres of depth, so from that fit (or from a given
// trajectory) the kernel takes up to `iters` undamped Gauss-Newton steps on the weighted squared reprojection error of the FULL projection, with the
// analytic 2 x 3 Jacobian per joint and a 3 x 3 solve by cofactors.  With iters = 0 it is the linear fit alone (start null) or the pure reprojection
// of a given trajectory (start given).  The rule is in the header; tests/lift_place_ref.py and tests/lift_refine_ref.py state it in float64.
//
// ONE LANE OWNS ONE POSE, as in lift_rigid.hip; a pose is (C = 3 or 4) x J floats and channel 3 (a hypothesis' score) is neither read nor
// written.  Everything between the float32 loads and the float32 stores is fp64: 17 joints and a few dozen operations per pose and pass, so the
// only error against a float64 statement on the same inputs is the final rounding (the linear fit's condition number is a few hundred; a float32
// solve of the same construction misses by 2e-5 m).  Sums run in joint order; a pose depends on no other pose; no atomics: the same bits on every
// call.  The fit kernel runs in workgroups of one wave and reads a pose's joints iters + 2 times (the linear sums, the first evaluation, one
// evaluation per step) straight from global memory, where a lane sits J C floats (204 or 272 bytes) from its neighbour; nothing is kept in a
// register array indexed at run time.  Copying the workgroup's 64 poses and their frames' keypoints into LDS first (consecutive lanes on
// consecutive floats, odd rows, as lift_score_align_kernel does) was built and measured on an MI355X on 3000 frames x 5 hypotheses (4 MB of poses,
// which stay in L2): staged 18.4 / 47.8 / 90.7 us at iters 0 / 3 / 8, this form 15.8 / 42.6 / 88.8 us, this form in workgroups of 256 lanes
// 15.4 / 47.9 / 99.4 us.  Staging does not pay: the time goes to the fp64 arithmetic of a pass (five divisions and a square root per joint), not to
// the loads.  (mp_lift_place once had a kernel of its own, the linear fit and one error pass in workgroups of 256 lanes: into outputs allocated
// once it took 14.9 us on the same poses, this kernel at iters = 0 takes 11.7 us - 59 workgroups against 235 on 256 CUs.  One kernel is also one
// place to change the camera model and the degenerate-fit rule.  DESIGN.md, "Refining the placement", has both measurements.)  The camera model, the
// Gauss-Newton sums, the 3x3 solve and the accept rule are lift_geom.h's, shared with lift_fuse.hip and lift_bundle.hip.
//
// Floor (mode 1): the minimum is taken from the STORED float32 values by a second kernel - MP_LIFT_WORLD_SHARES workgroups per sequence, each
// over one contiguous share of the sequence's poses, DPP inside a wave, LDS across the 4 waves, one partial per workgroup - and the third
// kernel merges a sequence's partials in share order, subtracts, and writes floor[s].  No atomics: the same bits on every call.
#include "lift_geom.h"

namespace mp {

constexpr int FLOOR_SHARES = MP_LIFT_WORLD_SHARES;
constexpr int REFINE_THREADS = 64;   // lanes of a workgroup of the fit kernel: one wave (235 workgroups for 15,000 poses; 256 lanes measured slower)

struct RefineArgs {
  const float* poses;            // (Ntot, inner, J, C)
  const float* kp;               // (Ntot, J, 2)
  const long* seq_offset;        // (S + 1) device
  const float* intr;             // (S, 9) device
  const float* weights;          // (J) device or null
  const float* start;            // (Ntot, inner, 3) or null: the linear fit
  const unsigned char* start_ok; // (Ntot, inner) or null
  float* traj;                   // (Ntot, inner, 3)
  float* reproj;                 // (Ntot, inner)
  unsigned char* ok;             // (Ntot, inner)
  unsigned char* steps;          // (Ntot, inner) or null
  long npose;                    // Ntot * inner
  int inner, J, C, S, distort, iters;
};

// one pass over the weighted joints of a pose at the translation t: the camera's frame is the pose's, so the Jacobian with respect to t is the
// projection's own.  P: the lane's pose (J rows of C floats), U: its frame's keypoints (J rows of 2 floats).  JAC = false leaves H and g at zero
// (iters = 0: the reprojection error alone)
template <bool JAC>
__device__ __forceinline__ LiftGN refine_eval(const float* P, const float* U, const float* weights, int J, int C, int distort, const LiftCam& cam,
                                              double tx, double ty, double tz) {
  LiftGN e = lift_gn_start();
  for (int j = 0; j < J; ++j) {                                        // sums in joint order
    const double w = weights != nullptr ? (double)weights[j] : 1.0;
    if (w == 0.0) continue;                                            // a joint of weight 0 is not looked at
    const double X = (double)P[j * C] + tx, Y = (double)P[j * C + 1] + ty, Z = (double)P[j * C + 2] + tz;
    if (!(Z > 0.0)) e.deep = false;
    const LiftProj pr = lift_project<JAC>(X, Y, Z, U + 2 * j, cam, distort);
    lift_gn_add<JAC>(e, w, pr, pr.c00, pr.c01, pr.c02, pr.c10, pr.c11, pr.c12);
  }
  return e;
}

__global__ __launch_bounds__(REFINE_THREADS) void lift_place_refine_kernel(RefineArgs A) {
  const int J = A.J, C = A.C;
  const long i = (long)blockIdx.x * REFINE_THREADS + threadIdx.x;      // pose (frame, inner index)
  if (i >= A.npose) return;
  const long g = i / A.inner;                                          // frame
  const int s = lift_seq_of(A.seq_offset, A.S, g);
  const float* cam = A.intr + (long)s * 9;
  const LiftCam K = lift_cam(cam);
  const float* P = A.poses + i * J * C;
  const float* U = A.kp + g * J * 2;
  double tx = 0.0, ty = 0.0, tz = 0.0;
  bool have = false;                                                   // a translation to evaluate at
  if (A.start == nullptr) {                                            // the linear fit
    const double fx = K.fx, fy = K.fy, cx = K.cx, cy = K.cy;
    double W = 0.0, Sa = 0.0, Sb = 0.0, Q = 0.0, Sx = 0.0, Sy = 0.0, Sc = 0.0;
    for (int j = 0; j < J; ++j) {                                      // sums in joint order
      const double w = A.weights != nullptr ? (double)A.weights[j] : 1.0;
      if (w == 0.0) continue;
      const double X = P[j * C], Y = P[j * C + 1], Z = P[j * C + 2];
      const double a = ((double)U[2 * j] - cx) / fx, b = ((double)U[2 * j + 1] - cy) / fy;
      const double ex = X - a * Z, ey = Y - b * Z;
      W += w; Sa += w * a; Sb += w * b; Q += w * (a * a + b * b);
      Sx += w * ex; Sy += w * ey; Sc += w * (a * ex + b * ey);
    }
    const double WQ = W * Q, det = WQ - Sa * Sa - Sb * Sb;
    const bool finite = __builtin_isfinite(W) && __builtin_isfinite(Sa) && __builtin_isfinite(Sb) && __builtin_isfinite(Q) && __builtin_isfinite(Sx) &&
                        __builtin_isfinite(Sy) && __builtin_isfinite(Sc);
    if (W > 0.0 && finite && det > 1e-9 * WQ) {
      tz = (W * Sc - Sa * Sx - Sb * Sy) / det;
      tx = (Sa * tz - Sx) / W;
      ty = (Sb * tz - Sy) / W;
      have = true;
    }
  } else {
    const float sx = A.start[i * 3], sy = A.start[i * 3 + 1], sz = A.start[i * 3 + 2];
    tx = sx; ty = sy; tz = sz;
    have = (A.start_ok == nullptr || A.start_ok[i] != 0) && __builtin_isfinite(tx) && __builtin_isfinite(ty) && __builtin_isfinite(tz);
    if (have) {                                                        // ... and a weighted joint to evaluate it on
      double W = 0.0;
      for (int j = 0; j < J; ++j) W += A.weights != nullptr ? (double)A.weights[j] : 1.0;
      have = W > 0.0;
    }
    if (!have) {                                                       // copied through, bit for bit
      A.traj[i * 3] = sx; A.traj[i * 3 + 1] = sy; A.traj[i * 3 + 2] = sz;
    }
  }
  unsigned char ok = 0, taken = 0;
  double err = 0.0;
  if (have) {
    LiftGN e = A.iters > 0 ? refine_eval<true>(P, U, A.weights, J, C, A.distort, K, tx, ty, tz)
                           : refine_eval<false>(P, U, A.weights, J, C, A.distort, K, tx, ty, tz);
    if (e.deep && __builtin_isfinite(e.F)) {
      ok = 1;
      for (int k = 0; k < A.iters; ++k) {
        double nx, ny, nz;                                             // t + d, d = -adj(H) g / det
        if (!lift_gn_step(e, tx, ty, tz, nx, ny, nz)) break;
        const LiftGN n = refine_eval<true>(P, U, A.weights, J, C, A.distort, K, nx, ny, nz);
        if (!lift_gn_accept(n, e)) break;
        tx = nx; ty = ny; tz = nz; e = n; ++taken;
      }
    }
    err = e.E / e.W;
    A.traj[i * 3] = (float)tx; A.traj[i * 3 + 1] = (float)ty; A.traj[i * 3 + 2] = (float)tz;
  } else if (A.start == nullptr) {
    A.traj[i * 3] = 0.f; A.traj[i * 3 + 1] = 0.f; A.traj[i * 3 + 2] = 0.f;
  }
  A.reproj[i] = (float)err;
  A.ok[i] = ok;
  if (A.steps != nullptr) A.steps[i] = taken;
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

// the one launcher of the fit kernel; `who` is the entry point, in whose name the arguments are refused
static int lift_place_launch(const char* who, const float* poses, int64_t Ntot, int inner, int J, int C, const float* kp, const int64_t* seq_offset, int S,
                             const float* intr, const float* weights, int distort, const float* start, const uint8_t* start_ok, int iters, float* traj,
                             float* reproj, uint8_t* ok, uint8_t* steps, void* stream) {
  static_assert(sizeof(long) == sizeof(int64_t), "LP64");
  MP_CHECK(poses && kp && seq_offset && intr && traj && reproj && ok, MP_ERR_ARG, "%s: null pointer", who);
  MP_CHECK(distort == 0 || distort == 1, MP_ERR_ARG, "%s: distort=%d (0: project_to_2d_linear, 1: project_to_2d)", who, distort);
  MP_CHECK(iters >= 0 && iters <= MP_LIFT_REFINE_MAXITERS, MP_ERR_ARG, "%s: iters=%d outside 0..%d", who, iters, MP_LIFT_REFINE_MAXITERS);
  MP_CHECK(start_ok == nullptr || start != nullptr, MP_ERR_ARG, "%s: start_ok without start: null pointer", who);
  long blocks = 0;
  if (int rc = lift_pose_shape(who, (long)Ntot, inner, J, C, S, &blocks)) return rc;
  blocks = (Ntot * inner + REFINE_THREADS - 1) / REFINE_THREADS;
  MP_CHECK(blocks <= 0x7fffffffL, MP_ERR_ARG, "%s: %ld poses: too many for one launch", who, (long)Ntot * inner);
  RefineArgs a = {};
  a.poses = poses; a.kp = kp; a.seq_offset = (const long*)seq_offset; a.intr = intr; a.weights = weights; a.start = start; a.start_ok = start_ok;
  a.traj = traj; a.reproj = reproj; a.ok = ok; a.steps = steps; a.npose = (long)Ntot * inner;
  a.inner = inner; a.J = J; a.C = C; a.S = S; a.distort = distort; a.iters = iters;
  hipLaunchKernelGGL(lift_place_refine_kernel, dim3((unsigned)blocks), dim3(REFINE_THREADS), 0, (hipStream_t)stream, a);
  MP_LAUNCH_CHECK();
  return MP_OK;
}

}  // namespace mp
using namespace mp;

extern "C" {

int mp_lift_place(const float* poses, int64_t Ntot, int inner, int J, int C, const float* kp, const int64_t* seq_offset, int S, const float* intr,
                  const float* weights, int distort, float* traj, float* reproj, uint8_t* ok, void* stream) {
  return lift_place_launch("mp_lift_place", poses, Ntot, inner, J, C, kp, seq_offset, S, intr, weights, distort, nullptr, nullptr, 0, traj, reproj, ok,
                           nullptr, stream);
}

int mp_lift_place_refine(const float* poses, int64_t Ntot, int inner, int J, int C, const float* kp, const int64_t* seq_offset, int S, const float* intr,
                         const float* weights, int distort, const float* start, const uint8_t* start_ok, int iters, float* traj, float* reproj,
                         uint8_t* ok, uint8_t* steps, void* stream) {
  return lift_place_launch("mp_lift_place_refine", poses, Ntot, inner, J, C, kp, seq_offset, S, intr, weights, distort, start, start_ok, iters, traj,
                           reproj, ok, steps, stream);
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

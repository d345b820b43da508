// Pinning a take's feet where they stand (include/manipose_hip.h: mp_lift_footlock has the rule).  A foot in a stance run - consecutive frames in
// contact - is pinned to the run's anchor, the mean of its ankle positions (put on the floor where one is given); the swing frames within `blend`
// frames of a run are eased into and out of the pin; each leg is then re-posed by analytic two-bone IK with the frame's own thigh and shank lengths.
// tests/lift_footlock_ref.py states the rule in float64.
//
// THE CHOSEN SHAPE: ONE COPY AND THREE LAUNCHES.  out = points by a device-to-device copy on the stream.  footlock_runs_kernel: ONE WAVE OWNS ONE
// (SEQUENCE, FOOT) and walks its frames in blocks of 64, twice.  Forward: the ballot of the lockable bits gives a block's run borders, a segmented
// Hillis-Steele scan over the lanes the sums inside it, and a carry in uniform registers (sum, length of the run that crosses the block's end) joins
// the blocks; the lane of a run's LAST frame (the next block's first bit is known: the blocks are loaded one ahead) stores the run's length and its
// float32 anchor there, every other lane a marker.  Backward: a lane takes length and anchor from its run's last frame - inside the block from memory,
// beyond it from the carry - and stores them at its own.  No lane ever walks a run: a person standing still for 3000 frames costs 47 blocks.
// footlock_pose_kernel<false>, then <true>: one lane per (frame, foot); first the frames OUTSIDE runs, which search `blend` frames each way for a
// run, read its anchor and the ankle under it and write their own target; then the frames INSIDE, which read and write their own.  Split in two
// launches because a reach-clamped frame of a run overwrites its anchor with its clamped target: no lane reads what a lane of its launch writes.
// The leg tables are read through unrolled selects, no array is indexed by a variable.  Resource report (hipcc -Rpass-analysis=kernel-resource-usage,
// gfx950): footlock_runs_kernel 72 VGPRs, footlock_pose_kernel<false> 56, <true> 58; scratch 0 bytes, no spills, no LDS.
// Everything between the float32 loads and the float32 stores is fp64, without contraction; no atomics, fixed orders: identical bits on every call.
#include "lift_common.h"

#pragma clang fp contract(off)
#include "lift_geom.h"                    // after the pragma: the shared code takes this file's mode

namespace mp {

constexpr int LOCK_THREADS = 256;
constexpr int LOCK_MAXF = MP_LIFT_GROUND_MAXFEET;
constexpr double LOCK_TINY = 1e-12;              // a bone or a reach shorter than this has no direction
constexpr double LOCK_POLE = 1e-9;               // |b| < LOCK_POLE l1: the knee lies on the hip-ankle line, the pole comes from an axis

struct LockArgs {
  const float* points;           // (Ntot, J, C)
  const unsigned char* valid;    // (Ntot) or null
  const long* seq_offset;        // (S + 1) device
  const unsigned char* contact;  // (Ntot, nf)
  const float* normal;           // (S, 3) or null
  const float* offset;           // (S)
  const unsigned char* plane_ok; // (S)
  float* out;                    // (Ntot, J, C), holds a copy of points
  int* run;                      // (Ntot, nf)
  float* target;                 // (Ntot, nf, 3)
  float* moved;                  // (Ntot, nf)
  unsigned char* flags;          // (Ntot, nf)
  int* runs;                     // (S, nf)
  long Ntot;
  double stretch;
  int J, C, S, nf, blend;
  signed char hip[LOCK_MAXF], knee[LOCK_MAXF], ankle[LOCK_MAXF];
};

struct LockPlane { double nx, ny, nz, off; bool has; };

__device__ __forceinline__ int lock_pick(const signed char (&t)[LOCK_MAXF], int k) {
  int j = t[0];
#pragma unroll
  for (int u = 1; u < LOCK_MAXF; ++u)
    if (u == k) j = t[u];
  return j;
}

// joint j of frame f in fp64; false where a coordinate is not finite
__device__ __forceinline__ bool lock_load(const LockArgs& A, long f, int j, double& x, double& y, double& z) {
  const float* p = A.points + (f * A.J + j) * A.C;
  x = p[0]; y = p[1]; z = p[2];
  return __builtin_isfinite((x + y) + z);                               // (a sum of float32 values in fp64 cannot overflow)
}

__device__ __forceinline__ bool lock_valid(const LockArgs& A, long f) { return A.valid == nullptr || A.valid[f] != 0; }

__device__ __forceinline__ double lock_norm(double x, double y, double z) { return sqrt((x * x + y * y) + z * z); }

__device__ __forceinline__ LockPlane lock_plane(const LockArgs& A, int s) {
  LockPlane P = {0.0, 0.0, 1.0, 0.0, false};
  if (A.normal == nullptr || (A.plane_ok[s] & 1) == 0) return P;
  P.nx = A.normal[s * 3]; P.ny = A.normal[s * 3 + 1]; P.nz = A.normal[s * 3 + 2]; P.off = A.offset[s];
  P.has = __builtin_isfinite(((P.nx + P.ny) + P.nz) + P.off);
  return P;
}

// step A's bit of frame f (inside [f0, f1) or not) and, where it is set, the ankle
__device__ __forceinline__ bool lock_bit(const LockArgs& A, long f, long f1, int k, int hj, int kj, int aj, double& x, double& y, double& z) {
  x = 0.0; y = 0.0; z = 0.0;
  if (f >= f1 || !lock_valid(A, f) || A.contact[f * A.nf + k] == 0) return false;
  double hx, hy, hz, kx, ky, kz;
  const bool fh = lock_load(A, f, hj, hx, hy, hz), fk = lock_load(A, f, kj, kx, ky, kz), fa = lock_load(A, f, aj, x, y, z);
  if (fh && fk && fa) return true;
  x = 0.0; y = 0.0; z = 0.0;
  return false;
}

// steps A and B: one wave per (sequence, foot)
__global__ __launch_bounds__(64) void footlock_runs_kernel(LockArgs A) {
  const int nf = A.nf, s = blockIdx.x / nf, k = blockIdx.x % nf, lane = threadIdx.x;
  const int hj = lock_pick(A.hip, k), kj = lock_pick(A.knee, k), aj = lock_pick(A.ankle, k);
  const FrameRange fr = lift_seq_frames(A.seq_offset, s, A.Ntot);
  const LockPlane P = lock_plane(A, s);
  const long blocks = (fr.f1 - fr.f0 + 63) / 64;
  const unsigned long long below = (1ull << lane) - 1ull;

  // forward: the sums, and length and anchor at each run's last frame
  double cx = 0.0, cy = 0.0, cz = 0.0;                                    // the carry: the run that reaches the block's first frame from before
  int clen = 0, nruns = 0;
  double nx, ny, nz;
  bool nlock = lock_bit(A, fr.f0 + lane, fr.f1, k, hj, kj, aj, nx, ny, nz);
#pragma unroll 1
  for (long c = 0; c < blocks; ++c) {
    const long f = fr.f0 + c * 64 + lane;
    const bool lock = nlock;
    double x = nx, y = ny, z = nz;
    nlock = lock_bit(A, f + 64, fr.f1, k, hj, kj, aj, nx, ny, nz);        // the block after this one (past f1: no bit)
    const unsigned long long m = __ballot(lock), mn = __ballot(nlock);
    const unsigned long long zb = ~m & below;                            // the frames of the block before this lane's that are not lockable
    const int start = zb ? 64 - __builtin_clzll(zb) : 0;                  // the first lane of this lane's segment
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const double vx = __shfl_up(x, off), vy = __shfl_up(y, off), vz = __shfl_up(z, off);
      if (lane - off >= start) { x += vx; y += vy; z += vz; }
    }
    int len = lane - start + 1;
    if (start == 0 && clen > 0) { x = cx + x; y = cy + y; z = cz + z; len += clen; }
    const bool next = lane < 63 ? ((m >> (lane + 1)) & 1ull) != 0ull : (mn & 1ull) != 0ull;
    if (f < fr.f1) {
      const long i = f * nf + k;
      if (lock && !next) {                                                // the run's last frame
        double ax = x / (double)len, ay = y / (double)len, az = z / (double)len;
        if (P.has) {
          const double h = ((P.nx * ax + P.ny * ay) + P.nz * az) - P.off;
          ax = ax - h * P.nx; ay = ay - h * P.ny; az = az - h * P.nz;
        }
        A.run[i] = len;
        A.target[i * 3] = (float)ax; A.target[i * 3 + 1] = (float)ay; A.target[i * 3 + 2] = (float)az;
      } else {
        A.run[i] = lock ? 1 : 0;                                          // a marker; the sweep back replaces it
      }
    }
    nruns += __popcll(m & ~(m << 1) & ~(clen > 0 ? 1ull : 0ull));         // runs that start in this block
    const double lx = __shfl(x, 63), ly = __shfl(y, 63), lz = __shfl(z, 63);
    const int ll = __shfl(len, 63);
    const bool on = (m >> 63) != 0ull;                                    // (uniform)
    cx = on ? lx : 0.0; cy = on ? ly : 0.0; cz = on ? lz : 0.0; clen = on ? ll : 0;
  }
  if (lane == 0) A.runs[s * nf + k] = nruns;
  __threadfence_block();
  __syncthreads();                                                        // the stores at the runs' last frames are visible to the wave

  // backward: every frame of a run takes length and anchor from the run's last frame
  float bx = 0.f, by = 0.f, bz = 0.f;                                     // the carry: the run that reaches past the block's last frame
  int blen = 0;
  const unsigned long long above = lane < 63 ? ~((2ull << lane) - 1ull) : 0ull;
#pragma unroll 1
  for (long c = blocks - 1; c >= 0; --c) {
    const long f = fr.f0 + c * 64 + lane, i = f * nf + k;
    const bool lock = f < fr.f1 && A.run[i] > 0;
    const unsigned long long m = __ballot(lock);
    const unsigned long long za = ~m & above;                            // the frames of the block after this lane's that are not lockable
    const int last = za ? __builtin_ctzll(za) - 1 : 63;                   // the last lane of this lane's segment
    int len = 0;
    float ax = 0.f, ay = 0.f, az = 0.f;
    if (lock) {
      if (last == 63 && blen > 0) { len = blen; ax = bx; ay = by; az = bz; }
      else {
        const long e = (fr.f0 + c * 64 + last) * nf + k;                  // (a lockable frame of this block: inside [f0, f1))
        len = A.run[e]; ax = A.target[e * 3]; ay = A.target[e * 3 + 1]; az = A.target[e * 3 + 2];
      }
    }
    if (lock) {                                                           // (a lane rewrites its own frame alone, a run's last lane what it holds)
      A.run[i] = len;
      A.target[i * 3] = ax; A.target[i * 3 + 1] = ay; A.target[i * 3 + 2] = az;
    }
    blen = __shfl(len, 0); bx = __shfl(ax, 0); by = __shfl(ay, 0); bz = __shfl(az, 0);      // (len = 0 where the block's first frame is in no run)
  }
}

// steps C to E: one lane per (frame, foot).  RUNS = false: the frames outside runs, and what is cleared; RUNS = true: the frames inside runs.
template <bool RUNS>
__global__ __launch_bounds__(LOCK_THREADS) void footlock_pose_kernel(LockArgs A) {
  const long i = (long)blockIdx.x * LOCK_THREADS + threadIdx.x;
  const int nf = A.nf;
  if (i >= A.Ntot * nf) return;
  const long f = i / nf;
  const int k = (int)(i % nf);
  const int s = lift_seq_of(A.seq_offset, A.S, f);
  const FrameRange fr = lift_seq_frames(A.seq_offset, s, A.Ntot);
  const bool held = f >= fr.f0 && f < fr.f1;
  if (!held) {
    if (!RUNS) { A.run[i] = 0; A.target[i * 3] = 0.f; A.target[i * 3 + 1] = 0.f; A.target[i * 3 + 2] = 0.f; A.moved[i] = 0.f; A.flags[i] = 0; }
    return;
  }
  if ((A.run[i] > 0) != RUNS) return;
  const int hj = lock_pick(A.hip, k), kj = lock_pick(A.knee, k), aj = lock_pick(A.ankle, k);
  double hx, hy, hz, kx, ky, kz, ax, ay, az;
  bool fin = lock_valid(A, f);
  if (fin) {
    const bool fh = lock_load(A, f, hj, hx, hy, hz), fk = lock_load(A, f, kj, kx, ky, kz), fa = lock_load(A, f, aj, ax, ay, az);
    fin = fh && fk && fa;
  }
  if (!fin) {                                                             // (never a frame of a run)
    A.target[i * 3] = 0.f; A.target[i * 3 + 1] = 0.f; A.target[i * 3 + 2] = 0.f; A.moved[i] = 0.f; A.flags[i] = 0;
    return;
  }
  const LockPlane P = lock_plane(A, s);
  int flags = 0;
  double tx = ax, ty = ay, tz = az;

  // step C
  if (RUNS) {
    tx = A.target[i * 3]; ty = A.target[i * 3 + 1]; tz = A.target[i * 3 + 2];
    flags = 1;
  } else {
    long fa = -1, fb = -1;
    const long lo = max(fr.f0, f - A.blend), hi = min(fr.f1 - 1, f + A.blend);
#pragma unroll 1
    for (long g = f - 1; g >= lo; --g)
      if (A.run[g * nf + k] > 0) { fa = g; break; }
#pragma unroll 1
    for (long g = f + 1; g <= hi; ++g)
      if (A.run[g * nf + k] > 0) { fb = g; break; }
    long L = (long)A.blend + 1;
    if (fa >= 0 && fb >= 0) L = min(L, fb - fa);
    if (fa >= 0) {
      const double w = 1.0 - (double)(f - fa) / (double)L;
      if (w > 0.0) {
        double px, py, pz;
        lock_load(A, fa, aj, px, py, pz);                                 // (a frame of a run: finite)
        const long e = fa * nf + k;
        const double sw = (w * w) * (3.0 - 2.0 * w);
        tx = tx + sw * ((double)A.target[e * 3] - px); ty = ty + sw * ((double)A.target[e * 3 + 1] - py); tz = tz + sw * ((double)A.target[e * 3 + 2] - pz);
        flags |= 2;
      }
    }
    if (fb >= 0) {
      const double w = 1.0 - (double)(fb - f) / (double)L;
      if (w > 0.0) {
        double px, py, pz;
        lock_load(A, fb, aj, px, py, pz);
        const long e = fb * nf + k;
        const double sw = (w * w) * (3.0 - 2.0 * w);
        tx = tx + sw * ((double)A.target[e * 3] - px); ty = ty + sw * ((double)A.target[e * 3 + 1] - py); tz = tz + sw * ((double)A.target[e * 3 + 2] - pz);
        flags |= 2;
      }
    }
    if (P.has) {
      const double h = ((P.nx * tx + P.ny * ty) + P.nz * tz) - P.off;
      if (h < 0.0) { tx = tx - h * P.nx; ty = ty - h * P.ny; tz = tz - h * P.nz; flags |= 8; }
    }
  }

  // step D
  const double l1 = lock_norm(kx - hx, ky - hy, kz - hz), l2 = lock_norm(ax - kx, ay - ky, az - kz);
  const double dx = tx - hx, dy = ty - hy, dz = tz - hz;
  const double D = lock_norm(dx, dy, dz);
  if (l1 < LOCK_TINY || l2 < LOCK_TINY || D < LOCK_TINY) {
    A.target[i * 3] = 0.f; A.target[i * 3 + 1] = 0.f; A.target[i * 3 + 2] = 0.f; A.moved[i] = 0.f; A.flags[i] = 32;
    return;
  }
  const double Dmin = fabs(l1 - l2), Dmax = fmax(A.stretch * (l1 + l2), Dmin);
  const double ux = dx / D, uy = dy / D, uz = dz / D;
  double Dc = D;
  if (D > Dmax) { Dc = Dmax; flags |= 4; }
  else if (D < Dmin) { Dc = Dmin; flags |= 4; }
  if (flags & 4) { tx = hx + ux * Dc; ty = hy + uy * Dc; tz = hz + uz * Dc; }
  const float sx = (float)tx, sy = (float)ty, sz = (float)tz;             // ankle' as it is stored
  A.target[i * 3] = sx; A.target[i * 3 + 1] = sy; A.target[i * 3 + 2] = sz;
  if (tx == ax && ty == ay && tz == az) {                                 // the foot is where it belongs: the leg keeps its bits
    A.moved[i] = 0.f; A.flags[i] = (unsigned char)flags;
    return;
  }
  const double ex = kx - hx, ey = ky - hy, ez = kz - hz;
  const double eu = (ex * ux + ey * uy) + ez * uz;
  double bx = ex - eu * ux, by = ey - eu * uy, bz = ez - eu * uz;
  double bn = lock_norm(bx, by, bz);
  if (bn < LOCK_POLE * l1) {
    const double mx = fabs(ux), my = fabs(uy), mz = fabs(uz);
    const int axis = (mx <= my && mx <= mz) ? 0 : (my <= mz ? 1 : 2);
    const double ui = axis == 0 ? ux : (axis == 1 ? uy : uz);
    bx = (axis == 0 ? 1.0 : 0.0) - ui * ux; by = (axis == 1 ? 1.0 : 0.0) - ui * uy; bz = (axis == 2 ? 1.0 : 0.0) - ui * uz;
    bn = lock_norm(bx, by, bz);
    flags |= 16;
  }
  const double x = ((Dc * Dc + l1 * l1) - l2 * l2) / (2.0 * Dc);
  const double y = sqrt(fmax(0.0, l1 * l1 - x * x));
  const double nkx = (hx + x * ux) + y * (bx / bn), nky = (hy + x * uy) + y * (by / bn), nkz = (hz + x * uz) + y * (bz / bn);
  float* ok = A.out + (f * A.J + kj) * A.C;
  float* oa = A.out + (f * A.J + aj) * A.C;
  ok[0] = (float)nkx; ok[1] = (float)nky; ok[2] = (float)nkz;
  oa[0] = sx; oa[1] = sy; oa[2] = sz;
  A.moved[i] = (float)lock_norm((double)sx - ax, (double)sy - ay, (double)sz - az);
  A.flags[i] = (unsigned char)flags;
}

}  // namespace mp
using namespace mp;

extern "C" {

int mp_lift_footlock(const float* points, int64_t Ntot, int J, int C, const uint8_t* valid, const int64_t* seq_offset, int S, const uint8_t* contact,
                     const int32_t* legs, int nf, const float* normal, const float* offset, const uint8_t* plane_ok, int blend, float stretch,
                     float* out, int32_t* run, float* target, float* moved, uint8_t* flags, int32_t* runs, void* stream) {
  static_assert(sizeof(long) == sizeof(int64_t), "LP64");
  long blocks = 0;
  if (int rc = lift_pose_shape("mp_lift_footlock", (long)Ntot, 1, J, C, S, &blocks)) return rc;
  MP_CHECK(points && seq_offset && contact, MP_ERR_ARG, "mp_lift_footlock: points, contact or seq_offset null");
  MP_CHECK(out && run && target && moved && flags && runs, MP_ERR_ARG,
           "mp_lift_footlock: null output (out, run, target, moved, flags, runs are all written)");
  MP_CHECK(out != points, MP_ERR_ARG, "mp_lift_footlock: out == points: the operator works out of place");
  MP_CHECK(legs != nullptr, MP_ERR_ARG, "mp_lift_footlock: null legs table");
  MP_CHECK(nf >= 1 && nf <= MP_LIFT_GROUND_MAXFEET, MP_ERR_ARG, "mp_lift_footlock: nf=%d feet outside 1..%d", nf, MP_LIFT_GROUND_MAXFEET);
  for (int k = 0; k < 3 * nf; ++k) {
    MP_CHECK(legs[k] >= 0 && legs[k] < J, MP_ERR_ARG, "mp_lift_footlock: legs[%d][%d] = %d outside 0..%d", k / 3, k % 3, legs[k], J - 1);
    for (int q = 0; q < k; ++q)
      MP_CHECK(legs[q] != legs[k], MP_ERR_ARG, "mp_lift_footlock: joint %d named twice, legs[%d][%d] and legs[%d][%d]: a leg is three joints, and no two legs share one",
               legs[k], q / 3, q % 3, k / 3, k % 3);
  }
  MP_CHECK((normal != nullptr) == (offset != nullptr) && (normal != nullptr) == (plane_ok != nullptr), MP_ERR_ARG,
           "mp_lift_footlock: normal, offset and plane_ok describe the floor together: all three or none");
  MP_CHECK(blend >= 0 && blend <= MP_LIFT_FOOTLOCK_MAXBLEND, MP_ERR_ARG, "mp_lift_footlock: blend=%d outside 0..%d", blend, MP_LIFT_FOOTLOCK_MAXBLEND);
  MP_CHECK(stretch > 0.f && stretch <= 1.f, MP_ERR_ARG, "mp_lift_footlock: stretch=%g outside (0, 1]", (double)stretch);
  MP_CHECK((long)Ntot * nf <= 0x7fffffffL, MP_ERR_ARG, "mp_lift_footlock: Ntot=%ld frames of %d feet: too many for one launch", (long)Ntot, nf);
  LockArgs a = {};
  a.points = points; a.valid = valid; a.seq_offset = (const long*)seq_offset; a.contact = contact; a.normal = normal; a.offset = offset;
  a.plane_ok = plane_ok; a.out = out; a.run = run; a.target = target; a.moved = moved; a.flags = flags; a.runs = runs;
  a.Ntot = (long)Ntot; a.stretch = (double)stretch;
  a.J = J; a.C = C; a.S = S; a.nf = nf; a.blend = blend;
  for (int k = 0; k < LOCK_MAXF; ++k) {
    const int q = k < nf ? k : 0;
    a.hip[k] = (signed char)legs[3 * q]; a.knee[k] = (signed char)legs[3 * q + 1]; a.ankle[k] = (signed char)legs[3 * q + 2];
  }
  hipStream_t st = (hipStream_t)stream;
  MP_HIP(hipMemcpyAsync(out, points, sizeof(float) * (size_t)Ntot * J * C, hipMemcpyDeviceToDevice, st));
  hipLaunchKernelGGL(footlock_runs_kernel, dim3((unsigned)(S * nf)), dim3(64), 0, st, a);
  MP_LAUNCH_CHECK();
  const long lanes = (long)Ntot * nf;
  const dim3 grid((unsigned)((lanes + LOCK_THREADS - 1) / LOCK_THREADS));
  hipLaunchKernelGGL(footlock_pose_kernel<false>, grid, dim3(LOCK_THREADS), 0, st, a);
  MP_LAUNCH_CHECK();
  hipLaunchKernelGGL(footlock_pose_kernel<true>, grid, dim3(LOCK_THREADS), 0, st, a);
  MP_LAUNCH_CHECK();
  return MP_OK;
}

}  // extern "C"

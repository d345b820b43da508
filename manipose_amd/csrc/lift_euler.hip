// Euler channels of a take's joint rotations, for export as a joint hierarchy (include/manipose_hip.h: mp_lift_euler has the rule): per (pose, joint)
// the three Tait-Bryan angles of q[j] in one of the six channel orders, in degrees, the root's rotation and position re-expressed by a rigid
// transform per sequence; then, with MP_LIFT_EULER_CONTINUOUS, every (sequence, inner index, joint) track made continuous in time - the other Euler
// solution of the same rotation where it lies nearer to the frame before, and whole turns added.  The reference has no counterpart.
// tests/lift_euler_ref.py states the rule in float64 with explicit loops and a sequential walk.
//
// lift_euler_kernel: ONE LANE OWNS ONE (pose, joint), 64 / J poses per wave, lift_rot_kernel's mapping, but with no tree walk: the rotations are
// local already.  A lane loads its 16-byte quaternion (consecutive lanes consecutive addresses) and stores 12 bytes of angles; the lane of joint 0
// alone reads the frame's validity byte, its sequence's basis and shift and the root, and writes pos and ok.  "A quaternion of the pose is not
// usable" (with the joint-0 lane's "the frame is invalid or the basis is unusable") and "a joint is in the gimbal case" are wave ballots masked to
// the pose's lanes.  The entries of the matrix that the channel order names are picked by chains of selects over the order's three (wave-uniform)
// axes on SCALARS, never by an index into a per-lane array or a struct held by reference (the compiler turns that into an indexed load from 80
// bytes of scratch memory a lane).
//
// lift_euler_unwrap_kernel (MP_LIFT_EULER_CONTINUOUS): ONE WAVE OWNS ONE TRACK and walks its frames 64 at a time, as lift_rot_sign_kernel does:
// lane l holds frame f0 + 64 c + l's stored triple and its ok byte; the ballot of the ok bits and the highest set bit below the lane name the
// predecessor's lane (none below: the last ok frame of the chunks before, carried in wave-uniform registers AS IT WAS STORED by the first kernel,
// so rewriting in place has no read-after-write hazard).  The branch is the exclusive-or prefix of the votes "the other solution of the
// predecessor is nearer", the turns a prefix sum of integers (six shuffle steps): both exact and associative, so the result cannot depend on the
// chunking.  Why one wave per track and not one per (sequence, inner index) looping over the joints: a lane's 12 bytes are 12 J inner bytes from
// its neighbour's either way, so either layout touches the same cache lines; per track the J waves of a pose's joints run at about the same time
// and share those lines out of the L2, and a take of ONE sequence still gives J inner waves to the device instead of inner.  No rate is claimed
// for that choice: tools/lift_bench.py --bvh is the measurement.
// Compiler's figures (hipcc --offload-arch=gfx950 -O3 -Rpass-analysis=kernel-resource-usage): lift_euler_kernel 52 VGPRs, 88 SGPRs;
// lift_euler_unwrap_kernel 64 VGPRs, 46 SGPRs; both scratch 0 bytes, no spills, no LDS.
// No atomics, no LDS, fixed orders: identical bits on every call.  Everything between the float32 loads and stores is fp64, contraction off.
// Whatever seq_offset holds: a frame's sequence lies in 0 .. S-1 (lift_seq_of) and a track's frames are clamped to 0 .. Ntot (lift_seq_frames).
#pragma clang fp contract(off)
#include "lift_geom.h"

namespace mp {

constexpr double EULER_DEG = 57.29577951308232;          // the double nearest to 180 / pi

struct EulerArgs {
  const float* quat;             // (Ntot, inner, J, 4)
  const float* root;             // (Ntot, inner, 3) or null
  const unsigned char* valid;    // (Ntot, inner) or null
  const long* seq_offset;        // (S + 1) device
  const float* basis;            // (S, 4) or null
  const float* shift;            // (S, 3) or null
  float* angles;                 // (Ntot, inner, J, 3)
  float* pos;                    // (Ntot, inner, 3) or null
  unsigned char* ok;             // (Ntot, inner)
  long Ntot, npose;              // npose = Ntot * inner
  double scale;
  int inner, J, S, ppw;
  int ai, aj, ak;                // the order's axes
  double sg;                     // +1 where (aj - ai) mod 3 == 1, else -1
};

// lift_geom.h's rule of a usable quaternion on loaded components: n2 = |q|^2 in fp64 finite and >= 1e-12
__device__ __forceinline__ double euler_norm2(float qw, float qx, float qy, float qz) {
  const double w = qw, x = qx, y = qy, z = qz;
  return w * w + x * x + y * y + z * z;
}
__device__ __forceinline__ bool euler_usable(double n2) { return __builtin_isfinite(n2) && n2 >= 1e-12; }

// row r of a matrix given in scalars, and entry c of a row, by selects (r, c wave-uniform)
struct Row3 { double c0, c1, c2; };
__device__ __forceinline__ Row3 euler_row(double r00, double r01, double r02, double r10, double r11, double r12, double r20, double r21, double r22, int r) {
  return {r == 0 ? r00 : r == 1 ? r10 : r20, r == 0 ? r01 : r == 1 ? r11 : r21, r == 0 ? r02 : r == 1 ? r12 : r22};
}
__device__ __forceinline__ double euler_col(const Row3 v, int c) { return c == 0 ? v.c0 : c == 1 ? v.c1 : v.c2; }

__global__ __launch_bounds__(POSE_THREADS) void lift_euler_kernel(EulerArgs A) {
  const int lane = threadIdx.x & 63, J = A.J;
  const long wave = (long)blockIdx.x * (POSE_THREADS / 64) + (threadIdx.x >> 6);
  const int slot = lane / J;
  const int j = lane - slot * J;
  const long n = wave * A.ppw + slot;                                  // pose (frame, inner index)
  const bool on = slot < A.ppw && n < A.npose;
  const unsigned long long mine = on ? ((1ull << J) - 1ull) << (slot * J) : 0ull;        // the lanes of this pose (J <= 32)
  const float4 c = on ? *reinterpret_cast<const float4*>(A.quat + (n * J + j) * 4) : make_float4(1.f, 0.f, 0.f, 0.f);
  const double n2 = euler_norm2(c.x, c.y, c.z, c.w);
  bool bad = !euler_usable(n2);
  const double nq = sqrt(n2);
  double w = (double)c.x / nq, x = (double)c.y / nq, y = (double)c.z / nq, z = (double)c.w / nq;
  double px = 0.0, py = 0.0, pz = 0.0;
  if (on && j == 0) {                                                  // the root: the frame's validity, its sequence's transform, the position
    const long g = n / A.inner;
    if (A.valid != nullptr && A.valid[n] == 0) bad = true;
    Rot3 B = lift_rot3(1.0, 0.0, 0.0, 0.0);
    double tx = 0.0, ty = 0.0, tz = 0.0;
    if (A.basis != nullptr) {
      const int s = lift_seq_of(A.seq_offset, A.S, g);
      const float* bp = A.basis + (long)s * 4;                         // (four loads: only quat is known to be 16-byte aligned)
      const float4 b = make_float4(bp[0], bp[1], bp[2], bp[3]);
      const double b2 = euler_norm2(b.x, b.y, b.z, b.w);
      if (euler_usable(b2)) {
        const double nb = sqrt(b2);
        const double bw = (double)b.x / nb, bx = (double)b.y / nb, by = (double)b.z / nb, bz = (double)b.w / nb;
        B = lift_rot3(bw, bx, by, bz);
        const double mw = bw * w - bx * x - by * y - bz * z, mx = bw * x + bx * w + by * z - bz * y;      // unit(basis) u[0]
        const double my = bw * y - bx * z + by * w + bz * x, mz = bw * z + bx * y - by * x + bz * w;
        w = mw; x = mx; y = my; z = mz;
      } else {
        bad = true;
      }
      tx = A.shift[(long)s * 3]; ty = A.shift[(long)s * 3 + 1]; tz = A.shift[(long)s * 3 + 2];
    }
    if (A.root != nullptr) {
      const double r0 = A.root[n * 3], r1 = A.root[n * 3 + 1], r2 = A.root[n * 3 + 2];
      px = A.scale * ((B.r00 * r0 + B.r01 * r1 + B.r02 * r2) + tx);
      py = A.scale * ((B.r10 * r0 + B.r11 * r1 + B.r12 * r2) + ty);
      pz = A.scale * ((B.r20 * r0 + B.r21 * r1 + B.r22 * r2) + tz);
    }
  }
  const bool pose_bad = (__ballot(on && bad) & mine) != 0ull;
  // the matrix of (w, x, y, z), lift_rot3's expressions, in scalars: rows i, j, k of it, then their entries, by selects
  const double m00 = 1.0 - 2.0 * (y * y + z * z), m01 = 2.0 * (x * y - w * z), m02 = 2.0 * (x * z + w * y);
  const double m10 = 2.0 * (x * y + w * z), m11 = 1.0 - 2.0 * (x * x + z * z), m12 = 2.0 * (y * z - w * x);
  const double m20 = 2.0 * (x * z - w * y), m21 = 2.0 * (y * z + w * x), m22 = 1.0 - 2.0 * (x * x + y * y);
  const int ai = A.ai, aj = A.aj, ak = A.ak;
  const double s = A.sg;
  const Row3 ri = euler_row(m00, m01, m02, m10, m11, m12, m20, m21, m22, ai), rj = euler_row(m00, m01, m02, m10, m11, m12, m20, m21, m22, aj),
             rk = euler_row(m00, m01, m02, m10, m11, m12, m20, m21, m22, ak);
  const double Rik = euler_col(ri, ak), Rjk = euler_col(rj, ak), Rkk = euler_col(rk, ak);
  const double c2 = Rjk * Rjk + Rkk * Rkk;
  const bool gimbal = c2 < 1e-12;
  const double be = asin(lift_clamp1(s * Rik));
  double al, ga;
  if (!gimbal) {
    al = atan2(-s * Rjk, Rkk);
    ga = atan2(-s * euler_col(ri, aj), euler_col(ri, ai));
  } else {
    al = atan2(s * euler_col(rk, aj), euler_col(rj, aj));
    ga = 0.0;
  }
  const bool any_gimbal = (__ballot(on && !pose_bad && gimbal) & mine) != 0ull;
  if (!on) return;
  float* o = A.angles + (n * J + j) * 3;
  o[0] = pose_bad ? 0.f : (float)(al * EULER_DEG) + 0.f;               // a zero is +0, one the rounding to float32 made too
  o[1] = pose_bad ? 0.f : (float)(be * EULER_DEG) + 0.f;
  o[2] = pose_bad ? 0.f : (float)(ga * EULER_DEG) + 0.f;
  if (j == 0) {
    if (A.pos != nullptr) {
      A.pos[n * 3] = pose_bad ? 0.f : (float)px + 0.f;
      A.pos[n * 3 + 1] = pose_bad ? 0.f : (float)py + 0.f;
      A.pos[n * 3 + 2] = pose_bad ? 0.f : (float)pz + 0.f;
    }
    A.ok[n] = pose_bad ? 0 : (any_gimbal ? 3 : 1);
  }
}

struct EulerUnwrapArgs {
  float* angles;                 // (Ntot, inner, J, 3), the canonical angles, rewritten in place
  const unsigned char* ok;       // (Ntot, inner), as the first kernel wrote it
  const long* seq_offset;        // (S + 1) device
  long Ntot, tracks;             // tracks = S * inner * J
  int inner, J;
};

// x wrapped into [-180, 180)
__device__ __forceinline__ double euler_wrap(double x) { return x - 360.0 * floor((x + 180.0) / 360.0); }

// d(x, y) = sum_i |w(x_i - y_i)|, summed in the order of the channels
__device__ __forceinline__ double euler_dist(double x0, double x1, double x2, double y0, double y1, double y2) {
  return (fabs(euler_wrap(x0 - y0)) + fabs(euler_wrap(x1 - y1))) + fabs(euler_wrap(x2 - y2));
}

__device__ __forceinline__ int euler_scan(int v, int lane) {           // the inclusive prefix sum over the wave's lanes
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int u = __shfl_up(v, d, 64);
    if (lane >= d) v += u;
  }
  return v;
}

__global__ __launch_bounds__(POSE_THREADS) void lift_euler_unwrap_kernel(EulerUnwrapArgs A) {
  const int lane = threadIdx.x & 63;
  const long track = (long)blockIdx.x * (POSE_THREADS / 64) + (threadIdx.x >> 6);      // wave-uniform
  if (track >= A.tracks) return;
  const long per = (long)A.inner * A.J;
  const int s = (int)(track / per);
  const long ij = track - (long)s * per;                               // inner index * J + joint
  const long i = ij / A.J;
  const FrameRange r = lift_seq_frames(A.seq_offset, s, A.Ntot);
  // the last ok frame of the chunks before: whether there is one, its stored triple, its branch and its turns
  bool has = false;
  float l0 = 0.f, l1 = 0.f, l2 = 0.f;
  int lflip = 0, W0 = 0, W1 = 0, W2 = 0;
  for (long c0 = r.f0; c0 < r.f1; c0 += 64) {
    const long g = c0 + lane;
    const bool in = g < r.f1;
    float* at = A.angles + ((in ? g : r.f0) * per + ij) * 3;
    const bool live = in && A.ok[(in ? g : r.f0) * A.inner + i] != 0;
    const float c_0 = at[0], c_1 = at[1], c_2 = at[2];
    const unsigned long long mask = __ballot(live);
    if (mask == 0ull) continue;                                        // (uniform) a chunk without a result is transparent
    const unsigned long long below = mask & ((1ull << lane) - 1ull);
    const int pl = below != 0ull ? 63 - __clzll((long long)below) : lane;      // the predecessor's lane (none below: this lane, replaced by the carry)
    const bool pred = below != 0ull || has;
    float p0 = __shfl(c_0, pl, 64), p1 = __shfl(c_1, pl, 64), p2 = __shfl(c_2, pl, 64);
    if (below == 0ull) { p0 = l0; p1 = l1; p2 = l2; }
    const double x0 = c_0, x1 = c_1, x2 = c_2, y0 = p0, y1 = p1, y2 = p2;
    const double ty0 = y0 + 180.0, ty1 = 180.0 - y1, ty2 = y2 + 180.0;  // T(c[g'])
    const bool vote = live && pred && euler_dist(x0, x1, x2, ty0, ty1, ty2) < euler_dist(x0, x1, x2, y0, y1, y2);
    const unsigned long long votes = __ballot(vote);
    const int flip = (__popcll(votes & (~0ull >> (63 - lane))) & 1) ^ lflip;
    int pflip = __shfl(flip, pl, 64);
    if (below == 0ull) pflip = lflip;
    const double e0 = flip ? x0 + 180.0 : x0, e1 = flip ? 180.0 - x1 : x1, e2 = flip ? x2 + 180.0 : x2;
    const double q0 = pflip ? ty0 : y0, q1 = pflip ? ty1 : y1, q2 = pflip ? ty2 : y2;      // e[g']
    const bool step = live && pred;
    const int t0 = euler_scan(step ? -(int)rint((e0 - q0) / 360.0) : 0, lane) + W0;
    const int t1 = euler_scan(step ? -(int)rint((e1 - q1) / 360.0) : 0, lane) + W1;
    const int t2 = euler_scan(step ? -(int)rint((e2 - q2) / 360.0) : 0, lane) + W2;
    if (live) {
      at[0] = (float)(e0 + 360.0 * (double)t0) + 0.f;
      at[1] = (float)(e1 + 360.0 * (double)t1) + 0.f;
      at[2] = (float)(e2 + 360.0 * (double)t2) + 0.f;
    }
    const int ll = 63 - __clzll((long long)mask);                      // the chunk's last ok frame (uniform)
    l0 = __shfl(c_0, ll, 64); l1 = __shfl(c_1, ll, 64); l2 = __shfl(c_2, ll, 64);
    lflip = __shfl(flip, ll, 64);
    W0 = __shfl(t0, ll, 64); W1 = __shfl(t1, ll, 64); W2 = __shfl(t2, ll, 64);
    has = true;
  }
}

static bool euler_apart(const void* a, uintptr_t na, const void* b, uintptr_t nb) {      // two byte ranges do not overlap (a null one: apart)
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return a == nullptr || b == nullptr || x + na <= y || y + nb <= x;
}

}  // namespace mp
using namespace mp;

extern "C" {

int mp_lift_euler(const float* quat, const float* root, const uint8_t* valid, int64_t Ntot, int inner, int J, const int64_t* seq_offset, int S,
                  const float* basis, const float* shift, float scale, int order, int flags, float* angles, float* pos, uint8_t* ok, void* stream) {
  static_assert(sizeof(long) == sizeof(int64_t), "LP64");
  MP_CHECK(quat && seq_offset && angles && ok, MP_ERR_ARG, "mp_lift_euler: null pointer (quat, seq_offset, angles and ok are all needed)");
  MP_CHECK((root == nullptr) == (pos == nullptr), MP_ERR_ARG, "mp_lift_euler: root and pos go together: both or neither");
  MP_CHECK((basis == nullptr) == (shift == nullptr), MP_ERR_ARG, "mp_lift_euler: basis and shift go together: both or neither");
  MP_CHECK(order >= 0 && order <= 5, MP_ERR_ARG, "mp_lift_euler: order=%d outside 0..5 (XYZ, XZY, YXZ, YZX, ZXY, ZYX)", order);
  MP_CHECK((flags & ~MP_LIFT_EULER_CONTINUOUS) == 0, MP_ERR_ARG, "mp_lift_euler: flags=%d (0 or MP_LIFT_EULER_CONTINUOUS)", flags);
  MP_CHECK(scale > 0.f && scale <= 3.4028235e38f, MP_ERR_ARG, "mp_lift_euler: scale=%g must be finite and > 0", (double)scale);
  long blocks = 0;
  if (int rc = lift_pose_shape("mp_lift_euler", (long)Ntot, inner, J, 3, S, &blocks)) return rc;
  MP_CHECK(((uintptr_t)quat & 15) == 0, MP_ERR_ARG, "mp_lift_euler: quat is not 16-byte aligned (a quaternion is loaded in one piece)");
  const uintptr_t np = (uintptr_t)Ntot * inner;
  const void* ins[6] = {quat, root, valid, seq_offset, basis, shift};
  const uintptr_t in_bytes[6] = {np * J * 16, np * 12, np, ((uintptr_t)S + 1) * 8, (uintptr_t)S * 16, (uintptr_t)S * 12};
  const void* outs[3] = {angles, pos, ok};
  const uintptr_t out_bytes[3] = {np * J * 12, np * 12, np};
  for (int a = 0; a < 3; ++a) {
    for (int b = 0; b < 6; ++b)
      MP_CHECK(euler_apart(outs[a], out_bytes[a], ins[b], in_bytes[b]), MP_ERR_ARG, "mp_lift_euler: an output overlaps an input (the call is out of place)");
    for (int b = 0; b < a; ++b)
      MP_CHECK(euler_apart(outs[a], out_bytes[a], outs[b], out_bytes[b]), MP_ERR_ARG, "mp_lift_euler: two outputs overlap");
  }
  static const int AX[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
  EulerArgs A = {};
  A.quat = quat; A.root = root; A.valid = valid; A.seq_offset = (const long*)seq_offset; A.basis = basis; A.shift = shift;
  A.angles = angles; A.pos = pos; A.ok = ok; A.Ntot = Ntot; A.npose = (long)Ntot * inner; A.scale = (double)scale;
  A.inner = inner; A.J = J; A.S = S; A.ppw = 64 / J;
  A.ai = AX[order][0]; A.aj = AX[order][1]; A.ak = AX[order][2];
  A.sg = (A.aj - A.ai + 3) % 3 == 1 ? 1.0 : -1.0;
  const long per_block = (long)A.ppw * (POSE_THREADS / 64);
  const long grid = (A.npose + per_block - 1) / per_block;
  MP_CHECK(grid <= 0x7fffffffL, MP_ERR_ARG, "mp_lift_euler: %ld poses of %d joints: too many for one launch", A.npose, J);
  EulerUnwrapArgs U = {};
  U.angles = angles; U.ok = ok; U.seq_offset = (const long*)seq_offset; U.Ntot = Ntot; U.inner = inner; U.J = J; U.tracks = (long)S * inner * J;
  const long unwrap_grid = (U.tracks + POSE_THREADS / 64 - 1) / (POSE_THREADS / 64);
  MP_CHECK(unwrap_grid <= 0x7fffffffL, MP_ERR_ARG, "mp_lift_euler: %ld tracks: too many for one launch", U.tracks);
  hipLaunchKernelGGL(lift_euler_kernel, dim3((unsigned)grid), dim3(POSE_THREADS), 0, (hipStream_t)stream, A);
  MP_LAUNCH_CHECK();
  if (flags & MP_LIFT_EULER_CONTINUOUS) {
    hipLaunchKernelGGL(lift_euler_unwrap_kernel, dim3((unsigned)unwrap_grid), dim3(POSE_THREADS), 0, (hipStream_t)stream, U);
    MP_LAUNCH_CHECK();
  }
  return MP_OK;
}

}  // extern "C"

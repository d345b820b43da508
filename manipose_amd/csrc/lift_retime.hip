// A take resampled in time on its rotations (include/manipose_hip.h: mp_lift_retime has the rule): every output frame samples its sequence at a
// fractional input time t, by the short-way slerp of the two frames around t (radius 0) or by mp_lift_smooth's weighted local polynomial, fitted in
// the tangent space of the valid frame nearest to t and evaluated at t (radius >= 1); the root trajectory goes through the same coefficients.  The
// reference has no counterpart.  tests/lift_retime_ref.py states the rule in float64 with explicit loops.
//
// lift_retime_kernel: ONE LANE OWNS ONE (output pose, joint), 64 / J output poses per wave, lift_rot_kernel's mapping; the lane of joint 0 also owns
// the pose's root, ok and taps.  Why not lift_smooth_kernel's LDS tile: that kernel stages TF + 2R input frames per TF output frames because its
// output frames ARE its input frames; here the output frames of a tile map to a span of input frames that depends on the device clock table (a
// third of a frame to three frames per output frame, another span for every sequence inside the tile), so a tile's span is not known on the host
// and LDS would have to be sized for the worst.  Read from global memory instead a lane loads ONE 16-byte quaternion per tap, consecutive lanes
// consecutive addresses (a pose's J lanes read 16 J contiguous bytes), and an input frame is read by the 2R + 1 output frames around it out of the
// L2, which holds a whole take (3000 frames x 17 joints x 16 bytes = 0.8 MB).  Bytes requested per output pose: (2R + 1)(16 J + 12 + 1); no rate
// is claimed for that choice beyond what tools/lift_bench.py --retime printed (a take of 3000 frames 18 us at radius 0 and 4,
// 158 us at radius 64, where the fp64 logarithm per (tap, joint), not the bytes, is the cost, and mp_lift_smooth on the same array takes 102 us).
// Compiler's figures (hipcc --offload-arch=gfx950 -O3 -Rpass-analysis=kernel-resource-usage): 158 VGPRs, 72 SGPRs, scratch 0 bytes, no spills, no LDS.
// The fit's per-pose work is done ONCE per (output frame, inner index): the joint-0 lane walks the validity bytes of the window and forms the
// moments, the degree, the first row of the inverse normal matrix and the reference tap, and hands them to the pose's lanes by wavefront shuffles;
// then the window is walked in chunks of J taps - lane e of the pose computes tap e's coefficient c_k, and the chunk's J coefficients reach all
// lanes by shuffles from lane e in turn, in increasing k: c_k is computed once and shared by the root and all J joints.  Loop bounds are uniform
// over the wave (the chunks of 2R + 1 taps); loads are predicated.  No LDS, no atomics, fixed orders: identical bits on every call.  Everything
// between the float32 loads and stores is fp64.
// Whatever the device tables hold: the sequence of an output frame lies in 0 .. S-1 (lift_seq_of), both frame ranges are clamped to their arrays
// (lift_seq_frames), t is clamped into [0, n - 1] by comparisons a NaN fails, and taps lie in [0, n - 1]: no access outside the arrays.
#include "lift_geom.h"

namespace mp {

struct RetimeArgs {
  const float* quat;             // (Ntot, inner, J, 4)
  const float* root;             // (Ntot, inner, 3) or null
  const unsigned char* valid;    // (Ntot, inner) or null
  const long* seq_offset;        // (S + 1) device: the input frames
  const long* out_offset;        // (S + 1) device: the output frames
  const double* clock;           // (S, 3) device: start, num, den
  float* quat_out;               // (Mtot, inner, J, 4)
  float* root_out;               // (Mtot, inner, 3) or null
  unsigned char* ok;             // (Mtot, inner)
  unsigned char* taps;           // (Mtot, inner)
  long Ntot, Mtot, npose;        // npose = Mtot * inner
  int inner, J, S, ppw, R, deg, taper, chunks;      // chunks of J taps that cover 2R + 1
};

struct Q4 { double w, x, y, z; };

__device__ __forceinline__ Q4 qmul(const Q4& a, const Q4& b) {
  return {a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z, a.w * b.x + a.x * b.w + a.y * b.z - a.z * b.y,
          a.w * b.y - a.x * b.z + a.y * b.w + a.z * b.x, a.w * b.z + a.x * b.y - a.y * b.x + a.z * b.w};
}

// q / |q| in fp64 of a stored quaternion (a zero or non-finite one gives IEEE results)
__device__ __forceinline__ Q4 unit_of(const float4& c) {
  const double w = c.x, x = c.y, y = c.z, z = c.w, n = sqrt(w * w + x * x + y * y + z * z);
  return {w / n, x / n, y / n, z / n};
}

// log(conj(a) . +-b), the sign aligning b with a (negated where dot(a, b) < 0): s = |r.xyz|, 0 where s == 0, else 2 atan2(s, r.w) r.xyz / s
__device__ __forceinline__ void rel_log(const Q4& a, Q4 b, double* v) {
  if (a.w * b.w + a.x * b.x + a.y * b.y + a.z * b.z < 0.0) b = {-b.w, -b.x, -b.y, -b.z};
  const Q4 r = qmul({a.w, -a.x, -a.y, -a.z}, b);
  const double s = sqrt(r.x * r.x + r.y * r.y + r.z * r.z);
  const double f = s == 0.0 ? 0.0 : 2.0 * atan2(s, r.w) / s;
  v[0] = s == 0.0 ? 0.0 : f * r.x; v[1] = s == 0.0 ? 0.0 : f * r.y; v[2] = s == 0.0 ? 0.0 : f * r.z;
}

// a . exp(v): exp(v) = (1, 0, 0, 0) where |v| == 0, else (cos(|v| / 2), sin(|v| / 2) v / |v|)
__device__ __forceinline__ Q4 mul_exp(const Q4& a, const double* v) {
  const double n = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
  if (n == 0.0) return a;
  double sn, cs;
  sincos(0.5 * n, &sn, &cs);
  const double g = sn / n;
  return qmul(a, {cs, g * v[0], g * v[1], g * v[2]});
}

__device__ __forceinline__ double retime_taper(double dk, int R, int taper) {      // dk = k - t
  if (taper == 0) return 1.0;
  const double r = dk / (double)(R + 1), q = 1.0 - r * r;
  return q * q;
}

__device__ __forceinline__ float4 store_of(const Q4& q) {                // a zero component is +0
  return make_float4((float)(q.w + 0.0), (float)(q.x + 0.0), (float)(q.y + 0.0), (float)(q.z + 0.0));
}

__global__ __launch_bounds__(POSE_THREADS) void lift_retime_kernel(RetimeArgs A) {
  const int lane = threadIdx.x & 63, J = A.J, R = A.R;
  const long wave = (long)blockIdx.x * (POSE_THREADS / 64) + (threadIdx.x >> 6);
  const int slot = lane / J;
  const int j = lane - slot * J;
  const long m = wave * A.ppw + slot;                                  // output pose (output frame, inner index)
  const bool on = slot < A.ppw && m < A.npose;
  const int first = on ? slot * J : lane;                              // the pose's joint-0 lane
  const long hg = on ? m / A.inner : 0;
  const int i = on ? (int)(m - hg * A.inner) : 0;
  // the frame's sequence, its place in it and its time: every lane of the pose computes the same few numbers
  const int s = lift_seq_of(A.out_offset, A.S, hg);
  const FrameRange o = lift_seq_frames(A.out_offset, s, A.Mtot), f = lift_seq_frames(A.seq_offset, s, A.Ntot);
  const long n = f.f1 - f.f0;
  const bool held = on && hg >= o.f0 && hg < o.f1 && n > 0;            // (an output frame no sequence holds, or of an empty sequence: no result)
  const double start = A.clock[s * 3], num0 = A.clock[s * 3 + 1], den = A.clock[s * 3 + 2];
  const double num = num0 > 0.0 ? num0 : 1.0;
  double t = start + ((double)(hg - o.f0) * den) / num;
  const double last = (double)(held ? n - 1 : 0);
  const bool clamped = !(t >= 0.0 && t <= last);
  if (!(t >= 0.0)) t = 0.0;                                            // (a NaN too)
  if (t > last) t = last;
  const long per = (long)A.inner * J;
  const float* qin = A.quat + ((held ? f.f0 : 0) * per + (long)i * J + j) * 4;     // + k per 4: this lane's quaternion of frame k of the sequence
  const float* rin = A.root != nullptr ? A.root + ((held ? f.f0 : 0) * A.inner + i) * 3 : nullptr;
  const unsigned char* vin = A.valid != nullptr ? A.valid + (held ? f.f0 : 0) * A.inner + i : nullptr;
  float4 q_store = make_float4(1.f, 0.f, 0.f, 0.f);
  float r_store[3] = {0.f, 0.f, 0.f};
  int result = 0, used = 0;

  if (R == 0) {
    const long k = (long)floor(t);
    const double al = t - (double)k;
    if (held && al == 0.0) {                                           // an input frame: its bits
      q_store = *reinterpret_cast<const float4*>(qin + k * per * 4);
      if (j == 0 && rin != nullptr) { r_store[0] = rin[k * A.inner * 3]; r_store[1] = rin[k * A.inner * 3 + 1]; r_store[2] = rin[k * A.inner * 3 + 2]; }
      result = vin == nullptr || vin[k * A.inner] != 0;
      used = 1;
    } else if (held && (vin == nullptr || (vin[k * A.inner] != 0 && vin[(k + 1) * A.inner] != 0))) {       // (al > 0: k + 1 <= n - 1)
      const Q4 a = unit_of(*reinterpret_cast<const float4*>(qin + k * per * 4));
      const Q4 b = unit_of(*reinterpret_cast<const float4*>(qin + (k + 1) * per * 4));
      double v[3];
      rel_log(a, b, v);
      v[0] *= al; v[1] *= al; v[2] *= al;
      q_store = store_of(mul_exp(a, v));
      if (j == 0 && rin != nullptr) {
#pragma unroll
        for (int c = 0; c < 3; ++c)
          r_store[c] = (float)(((1.0 - al) * (double)rin[k * A.inner * 3 + c] + al * (double)rin[(k + 1) * A.inner * 3 + c]) + 0.0);
      }
      result = 1;
      used = 2;
    }
  } else {
    // the window: valid frames k of the sequence with |k - t| <= R
    long lo = (long)ceil(t - (double)R), hi = (long)floor(t + (double)R);
    lo = max(lo, 0L);
    hi = held ? min(hi, n - 1) : -1;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0;
    long kstar = 0;
    int cnt = 0;
    if (held && j == 0) {                                              // once per (output frame, inner index)
      double S0 = 0.0, S1 = 0.0, S2 = 0.0, S3 = 0.0, S4 = 0.0, best = 1.0e300;
      bool left = false, right = false;
      for (long k = lo; k <= hi; ++k) {
        if (vin != nullptr && vin[k * A.inner] == 0) continue;
        const double dk = (double)k - t;
        const double w = retime_taper(dk, R, A.taper), u = dk / (double)R, wu = w * u, wu2 = wu * u;
        ++cnt;
        left = left || dk <= 0.0;
        right = right || dk >= 0.0;
        if (fabs(dk) < best) { best = fabs(dk); kstar = k; }            // the nearest, the lower one on a tie
        S0 += w; S1 += wu; S2 += wu2; S3 += wu2 * u; S4 += wu2 * u * u;
      }
      int d = min(A.deg, cnt - 1);
      if (!(left && right)) d = 0;                                     // not bracketed by valid data: held constant, never extrapolated
      if (cnt > 0) {
        if (d <= 0) {
          a0 = 1.0 / S0;
        } else if (d == 1) {
          const double det = S0 * S2 - S1 * S1;
          a0 = S2 / det; a1 = -S1 / det;
        } else {
          const double c0 = S2 * S4 - S3 * S3, c1 = S1 * S4 - S2 * S3, c2 = S1 * S3 - S2 * S2;
          const double det = S0 * c0 - S1 * c1 + S2 * c2;
          a0 = c0 / det; a1 = -c1 / det; a2 = c2 / det;
        }
      }
    }
    a0 = __shfl(a0, first, 64); a1 = __shfl(a1, first, 64); a2 = __shfl(a2, first, 64);
    kstar = __shfl(kstar, first, 64);
    cnt = __shfl(cnt, first, 64);
    const bool fit = held && cnt > 0;
    const Q4 ref = fit ? unit_of(*reinterpret_cast<const float4*>(qin + kstar * per * 4)) : Q4{1.0, 0.0, 0.0, 0.0};
    double acc[3] = {0.0, 0.0, 0.0}, racc[3] = {0.0, 0.0, 0.0};
    for (int ch = 0; ch < A.chunks; ++ch) {
      const long kmine = lo + (long)ch * J + j;                        // lane e of the pose: tap e of the chunk
      int use_mine = 0;
      double c_mine = 0.0;
      if (fit && kmine <= hi && (vin == nullptr || vin[kmine * A.inner] != 0)) {
        const double dk = (double)kmine - t, u = dk / (double)R;
        use_mine = 1;
        c_mine = retime_taper(dk, R, A.taper) * (a0 + u * (a1 + u * a2));
      }
      for (int e = 0; e < J; ++e) {
        const int src = on ? first + e : lane;                         // (an idle lane reads itself: its flag is never set)
        const int use = __shfl(use_mine, src, 64);
        const double c = __shfl(c_mine, src, 64);
        if (use) {                                                     // (only lanes of a pose with a fit see a set flag)
          const long k = lo + (long)ch * J + e;
          double v[3];
          rel_log(ref, unit_of(*reinterpret_cast<const float4*>(qin + k * per * 4)), v);
          acc[0] += c * v[0]; acc[1] += c * v[1]; acc[2] += c * v[2];
          if (j == 0 && rin != nullptr) {
#pragma unroll
            for (int x = 0; x < 3; ++x) racc[x] += c * (double)rin[k * A.inner * 3 + x];
          }
        }
      }
    }
    if (fit) {
      q_store = store_of(mul_exp(ref, acc));
      r_store[0] = (float)(racc[0] + 0.0); r_store[1] = (float)(racc[1] + 0.0); r_store[2] = (float)(racc[2] + 0.0);
      result = 1;
      used = cnt;
    }
  }
  if (!on) return;
  *reinterpret_cast<float4*>(A.quat_out + (m * J + j) * 4) = q_store;
  if (j == 0) {
    if (A.root_out != nullptr) { A.root_out[m * 3] = r_store[0]; A.root_out[m * 3 + 1] = r_store[1]; A.root_out[m * 3 + 2] = r_store[2]; }
    A.ok[m] = (unsigned char)((result ? 1 : 0) | (held && clamped ? 2 : 0));
    A.taps[m] = (unsigned char)used;
  }
}

static bool retime_apart(const void* a, uintptr_t na, const void* b, uintptr_t nb) {      // two byte ranges do not overlap (a null one: apart)
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return a == nullptr || b == nullptr || x + na <= y || y + nb <= x;
}

}  // namespace mp
using namespace mp;

extern "C" {

int mp_lift_retime(const float* quat, const float* root, const uint8_t* valid, int64_t Ntot, int inner, int J, const int64_t* seq_offset,
                   const int64_t* out_offset, const double* clock, int S, int64_t Mtot, int radius, int degree, int taper, float* quat_out,
                   float* root_out, uint8_t* ok, uint8_t* taps, void* stream) {
  static_assert(sizeof(long) == sizeof(int64_t), "LP64");
  MP_CHECK(quat && seq_offset && out_offset && clock, MP_ERR_ARG, "mp_lift_retime: null pointer (quat, seq_offset, out_offset and clock are all needed)");
  MP_CHECK(quat_out && ok && taps, MP_ERR_ARG, "mp_lift_retime: null output (quat_out, ok and taps are all written)");
  MP_CHECK((root == nullptr) == (root_out == nullptr), MP_ERR_ARG, "mp_lift_retime: root and root_out go together: both or neither");
  MP_CHECK(radius >= 0 && radius <= MP_LIFT_SMOOTH_MAXR, MP_ERR_ARG, "mp_lift_retime: radius=%d outside 0..%d", radius, MP_LIFT_SMOOTH_MAXR);
  MP_CHECK(degree >= 0 && degree <= 2, MP_ERR_ARG, "mp_lift_retime: degree=%d outside 0..2", degree);
  MP_CHECK(taper == 0 || taper == 1, MP_ERR_ARG, "mp_lift_retime: taper=%d (0: uniform, 1: biweight)", taper);
  long blocks = 0;
  if (int rc = lift_pose_shape("mp_lift_retime", (long)Ntot, inner, J, 3, S, &blocks)) return rc;
  MP_CHECK(Mtot > 0 && Mtot <= 0x7fffffffL * (long)POSE_THREADS / inner, MP_ERR_ARG, "mp_lift_retime: Mtot=%ld output frames of %d poses out of range",
           (long)Mtot, inner);
  MP_CHECK((((uintptr_t)quat | (uintptr_t)quat_out) & 15) == 0, MP_ERR_ARG, "mp_lift_retime: quat or quat_out is not 16-byte aligned (a quaternion moves in one piece)");
  const uintptr_t nin = (uintptr_t)Ntot * inner, nout = (uintptr_t)Mtot * inner;
  const void* ins[3] = {quat, root, valid};
  const uintptr_t in_bytes[3] = {nin * J * 16, nin * 12, nin};
  const void* outs[4] = {quat_out, root_out, ok, taps};
  const uintptr_t out_bytes[4] = {nout * J * 16, nout * 12, nout, nout};
  for (int a = 0; a < 4; ++a) {
    for (int b = 0; b < 3; ++b)
      MP_CHECK(retime_apart(outs[a], out_bytes[a], ins[b], in_bytes[b]), MP_ERR_ARG, "mp_lift_retime: an output overlaps an input (the call is out of place)");
    for (int b = 0; b < a; ++b)
      MP_CHECK(retime_apart(outs[a], out_bytes[a], outs[b], out_bytes[b]), MP_ERR_ARG, "mp_lift_retime: two outputs overlap");
  }
  RetimeArgs A = {};
  A.quat = quat; A.root = root; A.valid = valid; A.seq_offset = (const long*)seq_offset; A.out_offset = (const long*)out_offset; A.clock = clock;
  A.quat_out = quat_out; A.root_out = root_out; A.ok = ok; A.taps = taps; A.Ntot = Ntot; A.Mtot = Mtot; A.npose = (long)Mtot * inner;
  A.inner = inner; A.J = J; A.S = S; A.ppw = 64 / J; A.R = radius; A.deg = degree; A.taper = taper; A.chunks = (2 * radius + 1 + J - 1) / J;
  const long per_block = (long)A.ppw * (POSE_THREADS / 64);
  const long grid = (A.npose + per_block - 1) / per_block;
  MP_CHECK(grid <= 0x7fffffffL, MP_ERR_ARG, "mp_lift_retime: %ld output poses of %d joints: too many for one launch", A.npose, J);
  hipLaunchKernelGGL(lift_retime_kernel, dim3((unsigned)grid), dim3(POSE_THREADS), 0, (hipStream_t)stream, A);
  MP_LAUNCH_CHECK();
  return MP_OK;
}

}  // extern "C"

// Smoothing lifted sequences in time (include/manipose_hip.h: mp_lift_smooth): a weighted local polynomial fit along the frames of a sequence -
// Savitzky-Golay with validity weights - of every coordinate of (Ntot, inner, M, C) floats; frames without a valid value of their own are filled
// from their neighbours.  The reference has no counterpart (its hpe/viz.py renders the frames as they come).
//
// ONE WORKGROUP OWNS A TILE of TF consecutive frames of ONE inner index (frames by their number in the array: a sequence boundary may lie inside
// a tile; every frame looks up its own sequence).  A frame of one inner index is a contiguous run of W = M C floats.
//   stage:    the tile and its R-frame halos, frames t0 - R .. t0 + TF + R - 1 (those inside 0 .. Ntot-1), go to LDS as (TF + 2R, W) floats,
//             consecutive lanes on consecutive floats of a run, and their validity bytes as (TF + 2R) bytes
//   phase 1a: lane t < TF owns frame t0 + t: its sequence, the taps lo .. hi that stay inside the sequence, the moments S_k = sum w u^k (k = 0..4,
//             taps in increasing order), the number of valid taps, the degree, and the first row (a0, a1, a2) of the inverse of the normal
//             matrix [[S0, S1, S2], [S1, S2, S3], [S2, S3, S4]] (its leading 1x1 / 2x2 block for degree 0 / 1), by cofactors; writes `filled`
//   phase 1b: all lanes: the tap coefficients c[t][tau] = w_tau (a0 + a1 u + a2 u^2), 0 on a tap that is invalid or outside the sequence - once
//             per (frame, inner index), shared by the frame's W floats
//   phase 2:  consecutive lanes on consecutive floats of a frame: out = sum over the valid taps, in increasing order, of c[t][tau] y[t + tau];
//             reads of c are LDS broadcasts, reads of y are conflict-free.  A frame without a valid tap, and channel 3 of C = 4, are copied.
// Everything between the float32 loads and the one float32 store is fp64.  The taps of a frame lie in [g - R, g + R] AND inside the clamped
// frame range of its sequence (lift_seq_frames), so whatever the device table holds, only staged frames inside 0 .. Ntot-1 are read.
// Fixed summation order, no atomics: identical bits on every call.
//
// LDS: 8 TF (2R + 1) + 24 TF bytes of coefficients, 4 (TF + 2R) W of frames, 12 TF + (TF + 2R) of tables.  The host picks TF = 64, 32 or 16: the
// largest that stays within 64 KiB, otherwise 16 - the largest case (R = 64, M = 32, C = 4) then takes 88.8 KiB of the 160.  The workload is a
// few MB; tools/lift_bench.py --place times it next to mp_lift_rigid on the same arrays, and no rate is claimed.
#include "lift_common.h"
#include "../../include/manipose_hip.h"

namespace mp {

constexpr int SMOOTH_MAXR = MP_LIFT_SMOOTH_MAXR;
constexpr int SMOOTH_MAXM = 32;

struct SmoothArgs {
  const float* in;               // (Ntot, inner, M, C)
  float* out;                    // (Ntot, inner, M, C)
  const unsigned char* valid;    // (Ntot, inner) or null
  unsigned char* filled;         // (Ntot, inner) or null
  const long* seq_offset;        // (S + 1) device
  long Ntot;
  int inner, W, C, S, R, deg, taper, TF;
};

// k(tau): 1 (uniform) or the biweight (1 - (tau / (R + 1))^2)^2, positive on every tap
__device__ __forceinline__ double smooth_taper(int tau, int R, int taper) {
  if (taper == 0) return 1.0;
  const double r = (double)tau / (double)(R + 1), q = 1.0 - r * r;
  return q * q;
}

__host__ __device__ static inline long smooth_lds_bytes(int TF, int R, int W) {
  const long NT = 2 * R + 1, H = TF + 2 * R;
  return 8L * TF * NT + 24L * TF + 4L * H * W + 12L * TF + H;
}

__global__ __launch_bounds__(POSE_THREADS) void lift_smooth_kernel(SmoothArgs A) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smooth_lds[];
  const int R = A.R, TF = A.TF, W = A.W, NT = 2 * R + 1, H = TF + 2 * R;
  double* coef = (double*)smooth_lds;                                  // [TF][NT]
  double* poly = coef + TF * NT;                                       // [TF][3]
  float* y = (float*)(poly + TF * 3);                                  // [H][W]: row h is frame t0 - R + h
  int* lo = (int*)(y + H * W);                                         // [TF] first and last tap inside the sequence,
  int* hi = lo + TF;
  int* cnt = hi + TF;                                                  // [TF] valid taps among them
  unsigned char* vld = (unsigned char*)(cnt + TF);                     // [H]
  const int tid = threadIdx.x;
  const long tile = blockIdx.x / A.inner;
  const int i = blockIdx.x % A.inner;
  const long t0 = tile * TF;

  for (int idx = tid; idx < H * W; idx += POSE_THREADS) {
    const int h = idx / W, e = idx - h * W;
    const long gf = t0 - R + h;
    if (gf >= 0 && gf < A.Ntot) y[idx] = A.in[(gf * A.inner + i) * W + e];
  }
  for (int h = tid; h < H; h += POSE_THREADS) {
    const long gf = t0 - R + h;
    unsigned char v = 0;
    if (gf >= 0 && gf < A.Ntot) v = A.valid != nullptr ? (A.valid[gf * A.inner + i] != 0) : 1;
    vld[h] = v;
  }
  __syncthreads();

  if (tid < TF) {
    const long g = t0 + tid;
    int l = 1, h = 0, n = 0;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0;
    if (g < A.Ntot) {
      const int s = lift_seq_of(A.seq_offset, A.S, g);
      const FrameRange r = lift_seq_frames(A.seq_offset, s, A.Ntot);
      l = (int)min(max(r.f0 - g, (long)-R), (long)R + 1);               // taps stay inside [g - R, g + R]: inside the staged rows
      h = (int)max(min(r.f1 - 1 - g, (long)R), (long)-R - 1);
      double S0 = 0.0, S1 = 0.0, S2 = 0.0, S3 = 0.0, S4 = 0.0;
      bool left = false, right = false;
      for (int tau = l; tau <= h; ++tau) {
        if (!vld[tid + R + tau]) continue;
        const double w = smooth_taper(tau, R, A.taper), u = (double)tau / (double)R, wu = w * u, wu2 = wu * u;
        ++n;
        left = left || tau <= 0;
        right = right || tau >= 0;
        S0 += w; S1 += wu; S2 += wu2; S3 += wu2 * u; S4 += wu2 * u * u;
      }
      int d = min(A.deg, n - 1);
      if (!(left && right)) d = 0;                                     // not bracketed by valid data: held constant, never extrapolated
      if (n > 0) {
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
      if (A.filled != nullptr) A.filled[g * A.inner + i] = n > 0 ? 1 : 0;
    }
    lo[tid] = l; hi[tid] = h; cnt[tid] = n;
    poly[tid * 3] = a0; poly[tid * 3 + 1] = a1; poly[tid * 3 + 2] = a2;
  }
  __syncthreads();

  for (int idx = tid; idx < TF * NT; idx += POSE_THREADS) {
    const int t = idx / NT, tau = idx - t * NT - R;
    double c = 0.0;
    if (tau >= lo[t] && tau <= hi[t] && vld[t + R + tau]) {
      const double u = (double)tau / (double)R;
      c = smooth_taper(tau, R, A.taper) * (poly[t * 3] + u * (poly[t * 3 + 1] + u * poly[t * 3 + 2]));
    }
    coef[idx] = c;
  }
  __syncthreads();

  for (int idx = tid; idx < TF * W; idx += POSE_THREADS) {
    const int t = idx / W, e = idx - t * W;
    const long g = t0 + t;
    if (g >= A.Ntot) break;
    float o = y[(t + R) * W + e];                                      // no valid tap, or a score: the input's bits
    if (cnt[t] > 0 && !(A.C == 4 && (e & 3) == 3)) {
      const double* c = coef + t * NT + R;
      double acc = 0.0;
      for (int tau = lo[t]; tau <= hi[t]; ++tau) {
        if (vld[t + R + tau]) acc += c[tau] * (double)y[(t + R + tau) * W + e];
      }
      o = (float)acc;
    }
    A.out[(g * A.inner + i) * W + e] = o;
  }
}

}  // namespace mp
using namespace mp;

extern "C" {

int mp_lift_smooth(const float* in, float* out, int64_t Ntot, int inner, int M, int C, const uint8_t* valid, const int64_t* seq_offset, int S,
                   int radius, int degree, int taper, uint8_t* filled, void* stream) {
  static_assert(sizeof(long) == sizeof(int64_t), "LP64");
  MP_CHECK(in && out && seq_offset, MP_ERR_ARG, "mp_lift_smooth: null pointer");
  MP_CHECK(C == 3 || C == 4, MP_ERR_ARG, "mp_lift_smooth: C=%d (3: coordinates, 4: hypotheses with their score)", C);
  MP_CHECK(M >= 1 && M <= SMOOTH_MAXM, MP_ERR_ARG, "mp_lift_smooth: M=%d outside 1..%d", M, SMOOTH_MAXM);
  MP_CHECK(radius >= 1 && radius <= SMOOTH_MAXR, MP_ERR_ARG, "mp_lift_smooth: radius=%d outside 1..%d", radius, SMOOTH_MAXR);
  MP_CHECK(degree >= 0 && degree <= 2, MP_ERR_ARG, "mp_lift_smooth: degree=%d outside 0..2", degree);
  MP_CHECK(taper == 0 || taper == 1, MP_ERR_ARG, "mp_lift_smooth: taper=%d (0: uniform, 1: biweight)", taper);
  MP_CHECK(Ntot > 0 && inner > 0 && S > 0 && (long)S <= Ntot, MP_ERR_ARG, "mp_lift_smooth: Ntot=%ld inner=%d S=%d out of range", (long)Ntot, inner, S);
  const int W = M * C;
  int TF = 16;
  for (int t = 64; t > 16; t >>= 1) {
    if (smooth_lds_bytes(t, radius, W) <= 64 * 1024) { TF = t; break; }
  }
  MP_CHECK(Ntot <= 0x7fffffffL * TF / inner, MP_ERR_ARG, "mp_lift_smooth: %ld frames of %d: too many for one launch", (long)Ntot, inner);
  const long blocks = ((long)Ntot + TF - 1) / TF * inner;
  MP_CHECK(blocks <= 0x7fffffffL, MP_ERR_ARG, "mp_lift_smooth: %ld tiles: too many for one launch", blocks);
  const uintptr_t a = (uintptr_t)in, b = (uintptr_t)out, bytes = (uintptr_t)Ntot * (uintptr_t)inner * (uintptr_t)W * sizeof(float);
  MP_CHECK(a + bytes <= b || b + bytes <= a, MP_ERR_ARG, "mp_lift_smooth: in and out overlap (the call is out of place)");
  const long lds = smooth_lds_bytes(TF, radius, W);
  if (lds > 64 * 1024) MP_HIP(hipFuncSetAttribute((const void*)lift_smooth_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  SmoothArgs A = {};
  A.in = in; A.out = out; A.valid = valid; A.filled = filled; A.seq_offset = (const long*)seq_offset; A.Ntot = Ntot;
  A.inner = inner; A.W = W; A.C = C; A.S = S; A.R = radius; A.deg = degree; A.taper = taper; A.TF = TF;
  hipLaunchKernelGGL(lift_smooth_kernel, dim3((unsigned)blocks), dim3(POSE_THREADS), (size_t)lds, (hipStream_t)stream, A);
  MP_LAUNCH_CHECK();
  return MP_OK;
}

}  // extern "C"

// Lifting a sequence along ONE hypothesis path (include/manipose_hip.h: mp_lift_path): per frame exactly one of the model's K hypotheses, chosen
// jointly over the whole sequence - the maximum a posteriori path of a hidden Markov model whose states are the hypotheses, found with the Viterbi
// algorithm.  The reference has no counterpart (its aggregate is per frame).  Three kernels on one stream:
//   cost:   fully parallel over frames.  ONE WORKGROUP OWNS A TILE of TF consecutive frames and stages them plus the frame before the tile into LDS
//           (consecutive lanes on consecutive floats of hyps); one lane owns one (g, a, b) and writes D[g][a][b], the cost of stepping from
//           hypothesis a of frame g - 1 to hypothesis b of frame g; the first K lanes of a frame write the unary costs U[g][k].  Row g of the scratch
//           is [D (K K doubles, a-major), U (K doubles)].  D at the first frame of a sequence is computed against whatever frame lies before it
//           (0 at frame 0) and never read.
//   scan:   ONE WAVE64 WORKGROUP PER SEQUENCE (one instantiation per K).  Every lane holds f of state min(lane, K - 1) in a register and reads f_prev[a]
//           with v_readlane, a in increasing order, while the next frame's row is already on its way from LDS to registers; the rows of the next
//           SCAN_FRAMES frames are loaded into registers by all 64 lanes before the frames of the current chunk are worked through and stored to
//           the other LDS buffer afterwards.  Back-pointers go to the scratch as (Ntot, K) bytes.  The
//           backtrack stages them into LDS MP_LIFT_PATH_CHUNK frames at a time, one lane walks the chunk out of LDS, and all lanes store its path.
//   gather: consecutive lanes on consecutive floats of out: out[g] = hyps[g][path[g]][:, :3], bit for bit.
// Everything between the float32 loads and the stores is fp64, without contraction into fused multiply-adds.  A sequence's frames are its CLAMPED
// range (lift_seq_frames), and a state read from the back-pointers or the path is clamped to K - 1, so whatever the device table holds (overlapping
// sequences included) no frame outside 0 .. Ntot - 1 and no hypothesis outside 0 .. K - 1 is touched.  No atomics, fixed order: identical bits on every call.
#include "lift_common.h"
#include "../../include/manipose_hip.h"

#pragma clang fp contract(off)

namespace mp {

constexpr int PATH_MAXK = 8;
constexpr int SCAN_FRAMES = 16;                                                   // frames per prefetched chunk of the forward pass
constexpr int SCAN_ROW = PATH_MAXK * PATH_MAXK + PATH_MAXK;                       // doubles of a frame's row at K = 8
static_assert(MP_LIFT_PATH_CHUNK >= 1 && MP_LIFT_PATH_CHUNK <= 1024, "the backtrack's chunk lives in LDS");

struct PathArgs {
  const float* hyps;             // (Ntot, K, J, 4)
  const long* seq_offset;        // (S + 1) device
  double* rows;                  // (Ntot, K K + K): D, then U
  unsigned char* bp;             // (Ntot, K) back-pointers
  unsigned char* path;           // (Ntot)
  float* out;                    // (Ntot, J, 3) or null
  double* cost;                  // (S) or null
  long Ntot;
  double fac, sw;                // 1 / (2 sigma^2), switch_cost
  int K, J, S, TF;
};

__host__ __device__ static inline int path_tile_frames(int K) { return max(8, min(32, 256 / (K * K))); }

__global__ __launch_bounds__(POSE_THREADS) void lift_path_cost_kernel(PathArgs A) {
  extern __shared__ __attribute__((aligned(16))) unsigned char path_lds[];
  float* y = (float*)path_lds;                                         // [TF + 1][W]: row h is frame t0 - 1 + h
  const int K = A.K, J = A.J, TF = A.TF, W = K * J * 4, KK = K * K, R = KK + K;
  const int tid = threadIdx.x;
  const long t0 = (long)blockIdx.x * TF;

  for (int idx = tid; idx < (TF + 1) * W; idx += POSE_THREADS) {
    const int h = idx / W;
    const long gf = t0 - 1 + h;
    if (gf >= 0 && gf < A.Ntot) y[idx] = A.hyps[gf * W + (idx - h * W)];
  }
  __syncthreads();

  for (int idx = tid; idx < TF * KK; idx += POSE_THREADS) {
    const int t = idx / KK, ab = idx - t * KK, a = ab / K, b = ab - a * K;
    const long g = t0 + t;
    if (g >= A.Ntot) break;
    double d = 0.0;
    if (g > 0) {
      const float* xb = y + (t + 1) * W + b * J * 4;
      const float* xa = y + t * W + a * J * 4;
      double sum = 0.0;
      for (int j = 0; j < J; ++j) {
        for (int c = 0; c < 3; ++c) {
          const double e = (double)xb[j * 4 + c] - (double)xa[j * 4 + c];
          sum += e * e;
        }
      }
      d = A.fac * (sum / (double)J) + (a != b ? A.sw : 0.0);
      if (!__builtin_isfinite(d)) d = 1e30;
    }
    A.rows[g * R + ab] = d;
  }
  for (int idx = tid; idx < TF * K; idx += POSE_THREADS) {
    const int t = idx / K, k = idx - t * K;
    const long g = t0 + t;
    if (g >= A.Ntot) break;
    double s = (double)y[(t + 1) * W + k * J * 4 + 3];
    if (!(s > 1e-12)) s = 1e-12;
    A.rows[g * R + KK + k] = -log(s);
  }
}

// v of lane `lane` (wave-uniform) as a wave-uniform value
__device__ __forceinline__ double readlane_d(double v, int lane) {
  const long u = __double_as_longlong(v);
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(u & 0xffffffffL), lane);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(u >> 32), lane);
  return __longlong_as_double((long)(((unsigned long)hi << 32) | lo));
}

// K is a template argument: the loop over a is unrolled to exactly K steps and a frame's K + 1 row values sit in registers
template <int K>
__global__ __launch_bounds__(64) void lift_path_scan_kernel(PathArgs A) {
  __shared__ double buf[2][SCAN_FRAMES * SCAN_ROW];
  __shared__ unsigned char bpl[MP_LIFT_PATH_CHUNK * PATH_MAXK];
  __shared__ unsigned char pl[MP_LIFT_PATH_CHUNK];
  constexpr int KK = K * K, R = KK + K;
  constexpr int SCAN_PRE = (SCAN_FRAMES * R + 63) / 64;                // doubles a lane holds of a chunk in flight
  const int s = blockIdx.x, lane = threadIdx.x;
  const int b = min(lane, K - 1);                                      // lanes K .. 63 repeat state K - 1: no divergence, every lane's f is defined
  const FrameRange r = lift_seq_frames(A.seq_offset, s, A.Ntot);
  if (r.f1 <= r.f0) {
    if (lane == 0 && A.cost != nullptr) A.cost[s] = 0.0;
    return;
  }
  double f = A.rows[r.f0 * R + KK + b];

  // forward pass over frames f0 + 1 .. f1 - 1 in chunks of SCAN_FRAMES; the chunk at c0 holds rows c0 .. c0 + nf - 1
  double pre[SCAN_PRE];
  long c0 = r.f0 + 1;
  int cur = 0;
  {
    const int n = c0 < r.f1 ? (int)min((long)SCAN_FRAMES, r.f1 - c0) * R : 0;
#pragma unroll
    for (int i = 0; i < SCAN_PRE; ++i) {
      const int idx = i * 64 + lane;
      if (idx < n) buf[0][idx] = A.rows[c0 * R + idx];
    }
  }
  __syncthreads();
  for (; c0 < r.f1; c0 += SCAN_FRAMES) {
    const int nf = (int)min((long)SCAN_FRAMES, r.f1 - c0);
    const long nx = c0 + SCAN_FRAMES;
    const int nn = nx < r.f1 ? (int)min((long)SCAN_FRAMES, r.f1 - nx) * R : 0;
#pragma unroll
    for (int i = 0; i < SCAN_PRE; ++i) {
      const int idx = i * 64 + lane;
      pre[i] = idx < nn ? A.rows[nx * R + idx] : 0.0;
    }
    // the row of frame t + 1 is read from LDS while frame t is worked on: the chain f -> f is readlane, add, compare only
    double d[K], u;
#pragma unroll
    for (int a = 0; a < K; ++a) d[a] = buf[cur][a * K + b];
    u = buf[cur][KK + b];
    for (int t = 0; t < nf; ++t) {
      const double* nrow = buf[cur] + min(t + 1, SCAN_FRAMES - 1) * R;   // (past the chunk's last frame: a row that is read and not used)
      double dn[K];
#pragma unroll
      for (int a = 0; a < K; ++a) dn[a] = nrow[a * K + b];
      const double un = nrow[KK + b];
      double best = __builtin_inf();
      int arg = 0;
#pragma unroll
      for (int a = 0; a < K; ++a) {
        const double c = readlane_d(f, a) + d[a];
        if (c < best) { best = c; arg = a; }
      }
      f = best + u;
      if (lane < K) A.bp[(c0 + t) * K + lane] = (unsigned char)arg;
#pragma unroll
      for (int a = 0; a < K; ++a) d[a] = dn[a];
      u = un;
    }
#pragma unroll
    for (int i = 0; i < SCAN_PRE; ++i) {
      const int idx = i * 64 + lane;
      if (idx < nn) buf[cur ^ 1][idx] = pre[i];
    }
    __syncthreads();
    cur ^= 1;
  }

  // the end state: the first arg-min of f
  double best = readlane_d(f, 0);
  int state = 0;
#pragma unroll
  for (int k = 1; k < K; ++k) {
    const double v = readlane_d(f, k);
    if (v < best) { best = v; state = k; }
  }
  if (lane == 0 && A.cost != nullptr) A.cost[s] = best;

  // backtrack, from the last chunk to the first; the back-pointers of frame g name the state at g - 1, those of f0 do not exist
  __threadfence();
  __syncthreads();
  for (long c1 = r.f1; c1 > r.f0; c1 -= MP_LIFT_PATH_CHUNK) {
    const long b0 = max(c1 - MP_LIFT_PATH_CHUNK, r.f0);
    const int n = (int)(c1 - b0);
    for (int idx = (b0 == r.f0 ? K : 0) + lane; idx < n * K; idx += 64) bpl[idx] = A.bp[b0 * K + idx];
    __syncthreads();
    if (lane == 0) {
      for (int t = n - 1; t >= 0; --t) {
        pl[t] = (unsigned char)state;
        if (b0 + t > r.f0) state = min((int)bpl[t * K + state], K - 1);
      }
    }
    __syncthreads();
    for (int t = lane; t < n; t += 64) A.path[b0 + t] = pl[t];
    __syncthreads();
  }
}

__global__ __launch_bounds__(POSE_THREADS) void lift_path_gather_kernel(PathArgs A) {
  const int J3 = A.J * 3;
  const long idx = (long)blockIdx.x * POSE_THREADS + threadIdx.x;
  if (idx >= A.Ntot * J3) return;
  const long g = idx / J3;
  const int e = (int)(idx - g * J3), j = e / 3, c = e - j * 3;
  const int s = lift_seq_of(A.seq_offset, A.S, g);
  const FrameRange r = lift_seq_frames(A.seq_offset, s, A.Ntot);
  if (g < r.f0 || g >= r.f1) return;                                   // a frame no sequence holds has no path
  const int k = min((int)A.path[g], A.K - 1);
  A.out[idx] = A.hyps[((g * A.K + k) * A.J + j) * 4 + c];
}

static long path_scratch_bytes(long Ntot, int K) { return Ntot * (8L * K * K + 9L * K); }

}  // namespace mp
using namespace mp;

extern "C" {

int64_t mp_lift_path_scratch_floats(int64_t Ntot, int K) {
  if (Ntot <= 0 || Ntot > (1L << 40) || K < 1 || K > PATH_MAXK) return 0;
  return (path_scratch_bytes(Ntot, K) + 3) / 4;
}

int mp_lift_path(const float* hyps, int64_t Ntot, int K, int J, const int64_t* seq_offset, int S, float sigma, float switch_cost, uint8_t* path,
                 float* out, double* cost, float* scratch, int64_t scratch_floats, void* stream) {
  static_assert(sizeof(long) == sizeof(int64_t), "LP64");
  MP_CHECK(hyps && path && seq_offset && scratch, MP_ERR_ARG, "mp_lift_path: null pointer");
  MP_CHECK(K >= 1 && K <= PATH_MAXK, MP_ERR_ARG, "mp_lift_path: K=%d outside 1..%d", K, PATH_MAXK);
  MP_CHECK(J >= 2 && J <= LIFT_MAXJ, MP_ERR_ARG, "mp_lift_path: J=%d outside 2..%d", J, LIFT_MAXJ);
  MP_CHECK(Ntot > 0 && S > 0 && (long)S <= Ntot, MP_ERR_ARG, "mp_lift_path: Ntot=%ld S=%d out of range", (long)Ntot, S);
  MP_CHECK(Ntot <= (1L << 40) / (J * 3), MP_ERR_ARG, "mp_lift_path: %ld frames: too many for one launch", (long)Ntot);
  MP_CHECK(sigma > 0.f, MP_ERR_ARG, "mp_lift_path: sigma=%g must be > 0 (+inf is allowed)", (double)sigma);
  MP_CHECK(switch_cost >= 0.f && switch_cost <= 3.4028234e38f, MP_ERR_ARG, "mp_lift_path: switch_cost=%g must be finite and >= 0", (double)switch_cost);
  MP_CHECK(scratch_floats >= mp_lift_path_scratch_floats(Ntot, K), MP_ERR_ARG, "mp_lift_path: scratch too small (%ld floats, %ld needed)",
           (long)scratch_floats, (long)mp_lift_path_scratch_floats(Ntot, K));
  MP_CHECK(((uintptr_t)scratch & 7) == 0, MP_ERR_ARG, "mp_lift_path: scratch must be 8-byte aligned");
  PathArgs A = {};
  A.hyps = hyps; A.seq_offset = (const long*)seq_offset; A.rows = (double*)scratch; A.bp = (unsigned char*)(A.rows + (long)Ntot * (K * K + K));
  A.path = path; A.out = out; A.cost = cost; A.Ntot = Ntot;
  A.fac = 1.0 / (2.0 * (double)sigma * (double)sigma); A.sw = (double)switch_cost;
  A.K = K; A.J = J; A.S = S; A.TF = path_tile_frames(K);
  const long tiles = ((long)Ntot + A.TF - 1) / A.TF, blocks = ((long)Ntot * J * 3 + POSE_THREADS - 1) / POSE_THREADS;
  MP_CHECK(tiles <= 0x7fffffffL && blocks <= 0x7fffffffL, MP_ERR_ARG, "mp_lift_path: %ld frames: too many for one launch", (long)Ntot);
  const size_t lds = (size_t)(A.TF + 1) * K * J * 4 * sizeof(float);               // 43.5 KiB at most (K = 3, J = 32)
  hipLaunchKernelGGL(lift_path_cost_kernel, dim3((unsigned)tiles), dim3(POSE_THREADS), lds, (hipStream_t)stream, A);
  MP_LAUNCH_CHECK();
  switch (K) {
#define MP_PATH_SCAN(k) case k: hipLaunchKernelGGL(lift_path_scan_kernel<k>, dim3((unsigned)S), dim3(64), 0, (hipStream_t)stream, A); break;
    MP_PATH_SCAN(1) MP_PATH_SCAN(2) MP_PATH_SCAN(3) MP_PATH_SCAN(4) MP_PATH_SCAN(5) MP_PATH_SCAN(6) MP_PATH_SCAN(7) MP_PATH_SCAN(8)
#undef MP_PATH_SCAN
  }
  MP_LAUNCH_CHECK();
  if (out != nullptr) {
    hipLaunchKernelGGL(lift_path_gather_kernel, dim3((unsigned)blocks), dim3(POSE_THREADS), 0, (hipStream_t)stream, A);
    MP_LAUNCH_CHECK();
  }
  return MP_OK;
}

}  // extern "C"

// Synchronising the views of a take in time (include/manipose_hip.h: mp_lift_sync_views and mp_lift_shift_views have the rules).  A view's signal
// is the distance of every joint from the root, mean removed: it does not know the camera's orientation and not the lifter's depth mirror.  A view's
// lag against the take's reference view is the minimum over d in -L .. L of a robust mean squared difference of the two signals, refined by a
// parabola through the minimum and its neighbours.  tests/lift_sync_ref.py states both rules in float64.
//
// THREE KERNELS on one stream.  sync_signal_kernel, one workgroup of 256 lanes per (take, view): the distances and the usable bytes go to scratch,
// a lane sums the distances of its own frames in registers, the lanes' sums are added by a butterfly and the waves' in order, the means are
// subtracted in place.  (Its first form summed the means with 8 lanes per joint, each walking every 8th frame out of scratch: 375 dependent
// loads in a row on a take of 3000 frames, 540 of the call's 560 us; this form was measured against it, DESIGN.md has both.)
// sync_curve_kernel, one workgroup per (take, view, block of 16 lags, chunk of 256 or more frames): a tile of 64 reference rows and the 79 rows
// of the view that the block's lags pair with them are staged in LDS, so a reference row read once from memory serves 16 lags and a view's row up to 16 pairs; lane
// (lag k, slot s) sums the chunk's frames s, s + 16, ... of its lag in order, the 16 slots are added in order; rows are padded to an odd number
// of doubles, so the 16 slots of a wave read 16 different bank pairs, and the 4 lags of a wave that share a slot read the reference row as a
// broadcast.  A chunk's sum and pairs go to scratch.  (Without the chunks a take of 3000 frames was 47 tiles one after the other in each of its
// workgroups, load, barrier, sum, barrier: 440 us whatever the range; DESIGN.md has both forms' times.)  sync_pick_kernel, one wave per (take,
// view): the chunks' sums added in order and divided, the curve stored, the minimum under the tie rule by a butterfly (a total order: every lane
// ends with the same lag), the mean of the eligible values by lane sums in lag order and the butterfly, the parabola.
// mp_lift_shift_views is one lane per float.  Everything between the float32 loads and the float32 stores is fp64, without contraction; no
// atomics, fixed orders: identical bits on every call.
#include "lift_common.h"

#pragma clang fp contract(off)
#include "lift_geom.h"                    // after the pragma: the shared code takes this file's mode

namespace mp {

constexpr int SYNC_MAXV = MP_LIFT_FUSE_MAXV;
constexpr int SYNC_THREADS = 256;
constexpr int SYNC_MAXD = LIFT_MAXJ - 1;           // distances of a frame at most
constexpr int SYNC_LAGS = 16, SYNC_SLOTS = 16;    // of a curve workgroup: lags of a block, lanes of a lag
constexpr int SYNC_TILE = 64;                     // reference frames staged at a time
constexpr int SYNC_VROWS = SYNC_TILE + SYNC_LAGS - 1;
constexpr int SYNC_CHUNK = 256, SYNC_MAXCHUNKS = 64;   // frames of a chunk at least (sync_chunk_len), chunks of a take at most
constexpr int SYNC_ENTRIES = 5;                   // (sum, pairs) entries of the scratch per frame and view (sync_partial)
constexpr int SYNC_STRIDE = 31;                   // doubles of a staged row at most: (J - 1) | 1, J <= 32

struct SyncArgs {
  const float* poses;            // (V, Ftot, J, C)
  const unsigned char* valid;    // (V, Ftot) or null
  const long* take_offset;       // (G + 1) device
  double* sig;                   // scratch (V, Ftot, J - 1): d, then s
  double* partial;               // scratch (V, Ftot, SYNC_ENTRIES, 2): per take, lag and chunk the sum and the pairs (sync_partial)
  unsigned char* usable;         // scratch (V, Ftot)
  float* lag;                    // (G, V)
  int* lag_int;                  // (G, V)
  float* curve;                  // (G, V, 2 L + 1)
  float* contrast;               // (G, V)
  int* used;                     // (G, V)
  unsigned char* ok;             // (G, V)
  long Ftot;
  double sigma2;                 // sigma^2 (+inf: every term is e_f)
  int V, J, C, G, L, min_overlap;
};

// steps 1 and 2: the signal of (take, view) and its usable frames.  A lane walks the frames f0 + lane, f0 + lane + 256, ... in order and keeps the
// J - 1 sums of its frames' distances in registers (the arrays are indexed by unrolled constants only); the lanes' sums are added by an xor
// butterfly within a wave and the four waves' through LDS in wave order, (w0 + w1) + (w2 + w3), as lift_align.hip does; then every lane takes
// the means off the rows it wrote itself.
__global__ __launch_bounds__(SYNC_THREADS) void sync_signal_kernel(SyncArgs A) {
  __shared__ double part[SYNC_THREADS / 64][SYNC_MAXD];
  __shared__ double mean[SYNC_MAXD];
  __shared__ int count[SYNC_THREADS / 64];
  const int V = A.V, J = A.J, C = A.C, D = J - 1;
  const int g = (int)(blockIdx.x / V), v = (int)(blockIdx.x % V);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const FrameRange fr = lift_seq_frames(A.take_offset, g, A.Ftot);
  double acc[SYNC_MAXD];
#pragma unroll
  for (int j = 0; j < SYNC_MAXD; ++j) acc[j] = 0.0;
  int mine = 0;
#pragma unroll 1
  for (long f = fr.f0 + threadIdx.x; f < fr.f1; f += SYNC_THREADS) {
    const long fv = (long)v * A.Ftot + f;
    bool use = A.valid == nullptr || A.valid[fv] != 0;
    if (use) {
      const float* x = A.poses + fv * J * C;
      const double x0 = x[0], y0 = x[1], z0 = x[2];
      bool finite = __builtin_isfinite((x0 + y0) + z0);                   // (a sum of float32 values in fp64 cannot overflow)
      double d[SYNC_MAXD];
#pragma unroll
      for (int j = 0; j < SYNC_MAXD; ++j) {
        if (j < D) {
          const double ax = x[(j + 1) * C], ay = x[(j + 1) * C + 1], az = x[(j + 1) * C + 2];
          finite = finite && __builtin_isfinite((ax + ay) + az);
          const double bx = ax - x0, by = ay - y0, bz = az - z0;
          d[j] = sqrt((bx * bx + by * by) + bz * bz);
        }
      }
      use = finite;
      if (use) {
#pragma unroll
        for (int j = 0; j < SYNC_MAXD; ++j) {
          if (j < D) { acc[j] += d[j]; A.sig[fv * D + j] = d[j]; }
        }
      }
    }
    A.usable[fv] = use ? 1 : 0;
    mine += use ? 1 : 0;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    mine += __shfl_xor(mine, off);
#pragma unroll
    for (int j = 0; j < SYNC_MAXD; ++j)
      if (j < D) acc[j] += __shfl_xor(acc[j], off);
  }
  if (lane == 0) {
    count[wave] = mine;
#pragma unroll
    for (int j = 0; j < SYNC_MAXD; ++j)
      if (j < D) part[wave][j] = acc[j];
  }
  __syncthreads();
  const int n = (count[0] + count[1]) + (count[2] + count[3]);
  if (threadIdx.x == 0) A.used[blockIdx.x] = n;
  if ((int)threadIdx.x < D) {
    const double sum = (part[0][threadIdx.x] + part[1][threadIdx.x]) + (part[2][threadIdx.x] + part[3][threadIdx.x]);
    mean[threadIdx.x] = n > 0 ? sum / (double)n : 0.0;
  }
  __syncthreads();
#pragma unroll 1
  for (long f = fr.f0 + threadIdx.x; f < fr.f1; f += SYNC_THREADS) {      // (the rows this lane wrote itself)
    const long fv = (long)v * A.Ftot + f;
    const bool use = A.usable[fv] != 0;
#pragma unroll
    for (int j = 0; j < SYNC_MAXD; ++j) {
      if (j < D) A.sig[fv * D + j] = use ? A.sig[fv * D + j] - mean[j] : 0.0;      // (an unusable frame's row is never paired; it holds no NaN either)
    }
  }
}

// the reference view of take g: the lowest view with a usable frame, -1 if there is none (sync_signal_kernel has written used)
__device__ __forceinline__ int sync_reference(const SyncArgs& A, int g) {
  int r = -1;
#pragma unroll
  for (int u = SYNC_MAXV - 1; u >= 0; --u)
    if (u < A.V && A.used[(long)g * A.V + u] > 0) r = u;
  return r;
}

// The chunks of a take of n frames: its frames are cut into runs of len = max(256, 64 ceil(n / 4096)) frames, 64 at most; the cut depends on n
// alone, so a take's sums are added in the same order whatever stands beside it
__device__ __forceinline__ long sync_chunk_len(long n) { return max((long)SYNC_CHUNK, (n + 4095) / 4096 * 64); }

// where the (sum, pairs) of (take at f0 with n frames, view, lag d, chunk c) lies in the scratch: 5 entries per frame and view hold every take's
// (2 reach + 1) chunks entries, reach = min(L, n - 1): with one chunk that is 2 n - 1 at most, with more 513 (n / 256 + 1) < 5 n
__device__ __forceinline__ double* sync_partial(const SyncArgs& A, int v, long f0, int reach, int chunks, int d, int c) {
  return A.partial + (((long)v * A.Ftot + f0) * SYNC_ENTRIES + (long)(d + reach) * chunks + c) * 2;
}

// step 4: the sums of (take, view) at the 16 lags of a block over one chunk of the take's frames
__global__ __launch_bounds__(SYNC_THREADS) void sync_curve_kernel(SyncArgs A) {
  __shared__ double ref_rows[SYNC_TILE * SYNC_STRIDE];
  __shared__ double view_rows[SYNC_VROWS * SYNC_STRIDE];
  __shared__ unsigned char ref_use[SYNC_TILE], view_use[SYNC_VROWS];
  __shared__ double part[SYNC_LAGS][SYNC_SLOTS];
  __shared__ int pairs[SYNC_LAGS][SYNC_SLOTS];
  const int V = A.V, D = A.J - 1, L = A.L;
  const int g = (int)(blockIdx.x / V), v = (int)(blockIdx.x % V);
  const int k = threadIdx.x / SYNC_SLOTS, slot = threadIdx.x % SYNC_SLOTS;
  const int lag0 = -L + (int)blockIdx.y * SYNC_LAGS, d = lag0 + k;
  const FrameRange fr = lift_seq_frames(A.take_offset, g, A.Ftot);
  const long n = fr.f1 - fr.f0, len = sync_chunk_len(n);
  const int chunks = (int)((n + len - 1) / len), chunk = (int)blockIdx.z;
  const int reach = (int)min((long)L, n - 1);                             // lags beyond it pair no frames
  const int r = sync_reference(A, g);
  if (r < 0 || v == r || chunk >= chunks || lag0 > reach || lag0 + SYNC_LAGS - 1 < -reach) return;      // (uniform) nothing to sum here
  const long c0 = fr.f0 + (long)chunk * len, c1 = min(c0 + len, fr.f1);
  const int stride = D | 1;
  const double* sr = A.sig + (long)r * A.Ftot * D;
  const double* sv = A.sig + (long)v * A.Ftot * D;
  const unsigned char* ur = A.usable + (long)r * A.Ftot;
  const unsigned char* uv = A.usable + (long)v * A.Ftot;
  double acc = 0.0;
  int cnt = 0;
#pragma unroll 1
  for (long t0 = c0; t0 < c1; t0 += SYNC_TILE) {
    __syncthreads();                                                      // (the readers of the tile before are done)
    for (int i = threadIdx.x; i < SYNC_TILE * D; i += SYNC_THREADS) {
      const int row = i / D, col = i % D;
      const long f = t0 + row;
      ref_rows[row * stride + col] = f < c1 ? sr[f * D + col] : 0.0;
    }
    for (int i = threadIdx.x; i < SYNC_VROWS * D; i += SYNC_THREADS) {
      const int row = i / D, col = i % D;
      const long f = t0 + lag0 + row;
      view_rows[row * stride + col] = (f >= fr.f0 && f < fr.f1) ? sv[f * D + col] : 0.0;
    }
    if (threadIdx.x < SYNC_TILE) {
      const long f = t0 + threadIdx.x;
      ref_use[threadIdx.x] = f < c1 ? ur[f] : 0;
    }
    if (threadIdx.x < SYNC_VROWS) {
      const long f = t0 + lag0 + threadIdx.x;
      view_use[threadIdx.x] = (f >= fr.f0 && f < fr.f1) ? uv[f] : 0;
    }
    __syncthreads();
#pragma unroll 1
    for (int fl = slot; fl < SYNC_TILE; fl += SYNC_SLOTS) {
      if (ref_use[fl] == 0 || view_use[fl + k] == 0) continue;
      const double* a = view_rows + (fl + k) * stride;
      const double* b = ref_rows + fl * stride;
      double e = 0.0;
#pragma unroll 1
      for (int j = 0; j < D; ++j) {
        const double t = a[j] - b[j];
        e += t * t;
      }
      e = e / (double)D;
      acc += e / (1.0 + e / A.sigma2);
      cnt += 1;
    }
  }
  part[k][slot] = acc;
  pairs[k][slot] = cnt;
  __syncthreads();
  if (slot == 0 && d >= -reach && d <= reach) {
    double sum = 0.0;
    int nd = 0;
#pragma unroll
    for (int s = 0; s < SYNC_SLOTS; ++s) { sum += part[k][s]; nd += pairs[k][s]; }
    double* p = sync_partial(A, v, fr.f0, reach, chunks, d, chunk);
    p[0] = sum;
    p[1] = (double)nd;
  }
}

// the fp64 curve value of lag d, |d| <= reach: the chunks' sums and pairs added in chunk order; +inf where the lag is ineligible
__device__ __forceinline__ double sync_value(const SyncArgs& A, int v, long f0, int reach, int chunks, int d) {
  const double* p = sync_partial(A, v, f0, reach, chunks, d, 0);
  double sum = 0.0, nd = 0.0;
#pragma unroll 1
  for (int c = 0; c < chunks; ++c) { sum += p[2 * c]; nd += p[2 * c + 1]; }
  if (!(nd >= (double)A.min_overlap)) return __builtin_inf();
  const double c = sum / nd;
  return __builtin_isfinite(c) ? c : __builtin_inf();
}

// the order of step 5 among eligible lags: the smaller value, then the smaller |d|, then the positive lag
__device__ __forceinline__ bool sync_before(double ca, int da, double cb, int db) {
  if (ca != cb) return ca < cb;
  const int aa = da < 0 ? -da : da, ab = db < 0 ? -db : db;
  if (aa != ab) return aa < ab;
  return da > db;
}

// steps 3 to 7: the row of (take, view) and its curve; one wave
__global__ __launch_bounds__(64) void sync_pick_kernel(SyncArgs A) {
  const int V = A.V, L = A.L, width = 2 * L + 1;
  const int g = (int)(blockIdx.x / V), v = (int)(blockIdx.x % V), lane = threadIdx.x;
  const long row = blockIdx.x;
  const FrameRange fr = lift_seq_frames(A.take_offset, g, A.Ftot);
  const long n = fr.f1 - fr.f0, len = sync_chunk_len(n);
  const int chunks = (int)((n + len - 1) / len);
  const int r = sync_reference(A, g);
  float* out = A.curve + row * width;
  if (r < 0 || v == r) {                                                  // (uniform) the reference view's row, and a take without one
    for (int i = lane; i < width; i += 64) out[i] = 0.f;
    if (lane == 0) { A.lag[row] = 0.f; A.lag_int[row] = 0; A.contrast[row] = 0.f; A.ok[row] = r < 0 ? 0 : 1; }
    return;
  }
  const int reach = (int)min((long)L, n - 1);
  const double inf = __builtin_inf();
  double best = inf, sum = 0.0;
  int best_d = 0, eligible = 0;
#pragma unroll 1
  for (int d = -L + lane; d <= L; d += 64) {
    const double c = (d >= -reach && d <= reach) ? sync_value(A, v, fr.f0, reach, chunks, d) : inf;
    out[d + L] = (float)c;
    if (c < inf) {
      if (eligible == 0 || sync_before(c, d, best, best_d)) { best = c; best_d = d; }
      sum += c;
      eligible += 1;
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const double oc = __shfl_xor(best, off), os = __shfl_xor(sum, off);
    const int od = __shfl_xor(best_d, off), oe = __shfl_xor(eligible, off);
    if (oe > 0 && (eligible == 0 || sync_before(oc, od, best, best_d))) { best = oc; best_d = od; }
    sum += os;
    eligible += oe;
  }
  if (lane != 0) return;
  if (eligible == 0) { A.lag[row] = 0.f; A.lag_int[row] = 0; A.contrast[row] = 0.f; A.ok[row] = 0; return; }
  double delta = 0.0;
  int ok = 1;
  if (best_d > -reach && best_d < reach) {                                // (reach <= L: |d*| < L, and both neighbours have sums)
    const double lo = sync_value(A, v, fr.f0, reach, chunks, best_d - 1), hi = sync_value(A, v, fr.f0, reach, chunks, best_d + 1);
    const double den = (lo - 2.0 * best) + hi;
    if (lo < inf && hi < inf && den > 0.0) {
      delta = 0.5 * (lo - hi) / den;
      delta = delta < -0.5 ? -0.5 : (delta > 0.5 ? 0.5 : delta);
      ok = 3;
    }
  }
  const double mean = sum / (double)eligible;
  A.lag[row] = (float)((double)best_d + delta);
  A.lag_int[row] = best_d;
  A.contrast[row] = mean > 0.0 ? (float)(1.0 - best / mean) : 0.f;
  A.ok[row] = (unsigned char)ok;
}

struct ShiftArgs {
  const float* in;               // (V, Ftot, M)
  const unsigned char* valid;    // (V, Ftot) or null
  const long* take_offset;       // (G + 1) device
  const float* lag;              // (G, V) device
  float* out;                    // (V, Ftot, M)
  unsigned char* valid_out;      // (V, Ftot)
  long Ftot, M, total;           // total = V Ftot M
  int V, G, mode;
};

__global__ __launch_bounds__(SYNC_THREADS) void sync_shift_kernel(ShiftArgs A) {
  const long idx = (long)blockIdx.x * SYNC_THREADS + threadIdx.x;
  if (idx >= A.total) return;
  const long row = idx / A.M, m = idx % A.M;
  const int v = (int)(row / A.Ftot);
  const long f = row % A.Ftot;
  const int g = lift_seq_of(A.take_offset, A.G, f);
  const FrameRange fr = lift_seq_frames(A.take_offset, g, A.Ftot);
  float res = 0.f;
  unsigned char have = 0;
  if (f >= fr.f0 && f < fr.f1) {
    const double n = (double)(fr.f1 - fr.f0), lag = (double)A.lag[(long)g * A.V + v];
    if (__builtin_isfinite(lag)) {
      const double p = (double)(f - fr.f0) + lag;
      const double i = A.mode == 0 ? floor(p + 0.5) : floor(p);
      const double a = A.mode == 0 ? 0.0 : p - i;
      const bool two = a != 0.0;
      if (i >= 0.0 && i + (two ? 1.0 : 0.0) < n) {                        // (compared as doubles: a huge lag never becomes an index)
        const long fi = (long)v * A.Ftot + fr.f0 + (long)i;
        if (A.valid == nullptr || (A.valid[fi] != 0 && (!two || A.valid[fi + 1] != 0))) {
          have = 1;
          if (two) res = (float)((1.0 - a) * (double)A.in[fi * A.M + m] + a * (double)A.in[(fi + 1) * A.M + m]);
          else res = __uint_as_float(reinterpret_cast<const unsigned int*>(A.in)[fi * A.M + m]);      // a copy of the bits
        }
      }
    }
  }
  A.out[idx] = res;
  if (m == 0) A.valid_out[row] = have;
}

// host: the byte offsets of the scratch parts; the total
static long sync_scratch(int V, long Ftot, int J, long* partial, long* usable) {
  const long rows = (long)V * Ftot;
  *partial = rows * (J - 1) * 8;
  *usable = *partial + rows * SYNC_ENTRIES * 16;
  return (*usable + rows + 7) / 8 * 8;
}

}  // namespace mp
using namespace mp;

extern "C" {

int64_t mp_lift_sync_views_scratch_bytes(int V, int64_t Ftot, int J) {
  if (V < 1 || V > MP_LIFT_FUSE_MAXV || J < 2 || J > LIFT_MAXJ || Ftot <= 0 || Ftot > 0x7fffffffL) return 0;
  long a, b;
  return sync_scratch(V, (long)Ftot, J, &a, &b);
}

int mp_lift_sync_views(const float* poses, int V, int64_t Ftot, int J, int C, const uint8_t* valid, const int64_t* take_offset, int G,
                       int max_lag, int min_overlap, float sigma, float* lag, int32_t* lag_int, float* curve, float* contrast,
                       int32_t* used, uint8_t* ok, void* scratch, int64_t scratch_bytes, void* stream) {
  static_assert(sizeof(long) == sizeof(int64_t), "LP64");
  MP_CHECK(poses && take_offset && lag && lag_int && curve && contrast && used && ok, MP_ERR_ARG, "mp_lift_sync_views: null pointer");
  if (int rc = lift_take_shape("mp_lift_sync_views", V, (long)Ftot, J, G)) return rc;
  MP_CHECK(C == 3 || C == 4, MP_ERR_ARG, "mp_lift_sync_views: C=%d (3: poses, 4: hypotheses with their score)", C);
  MP_CHECK(Ftot <= 0x7fffffffL, MP_ERR_ARG, "mp_lift_sync_views: Ftot=%ld G=%d out of range", (long)Ftot, G);
  MP_CHECK((long)G * V <= 0x7fffffffL, MP_ERR_ARG, "mp_lift_sync_views: G=%d takes of %d views: too many for one launch", G, V);
  MP_CHECK(max_lag >= 0 && max_lag <= MP_LIFT_SYNC_MAXLAG, MP_ERR_ARG, "mp_lift_sync_views: max_lag=%d outside 0..%d", max_lag, MP_LIFT_SYNC_MAXLAG);
  MP_CHECK(min_overlap >= 1, MP_ERR_ARG, "mp_lift_sync_views: min_overlap=%d must be >= 1", min_overlap);
  MP_CHECK(sigma > 0.f, MP_ERR_ARG, "mp_lift_sync_views: sigma=%g must be > 0 (inf: plain squares)", (double)sigma);
  long at_curve, at_usable;
  const long need = sync_scratch(V, (long)Ftot, J, &at_curve, &at_usable);
  MP_CHECK(scratch != nullptr && scratch_bytes >= need && ((uintptr_t)scratch & 7) == 0, MP_ERR_ARG,
           "mp_lift_sync_views: scratch null, misaligned or too small: %ld bytes given, %ld needed", (long)scratch_bytes, need);
  SyncArgs a = {};
  a.poses = poses; a.valid = valid; a.take_offset = (const long*)take_offset;
  a.sig = (double*)scratch; a.partial = (double*)((char*)scratch + at_curve); a.usable = (unsigned char*)scratch + at_usable;
  a.lag = lag; a.lag_int = lag_int; a.curve = curve; a.contrast = contrast; a.used = used; a.ok = ok;
  a.Ftot = (long)Ftot; a.sigma2 = (double)sigma * (double)sigma;
  a.V = V; a.J = J; a.C = C; a.G = G; a.L = max_lag; a.min_overlap = min_overlap;
  const unsigned rows = (unsigned)((long)G * V), blocks = (unsigned)((2 * max_lag + 1 + SYNC_LAGS - 1) / SYNC_LAGS);
  hipLaunchKernelGGL(sync_signal_kernel, dim3(rows), dim3(SYNC_THREADS), 0, (hipStream_t)stream, a);
  MP_LAUNCH_CHECK();
  const unsigned chunks = (unsigned)min((long)SYNC_MAXCHUNKS, ((long)Ftot + SYNC_CHUNK - 1) / SYNC_CHUNK);      // (of the longest take the call can hold)
  hipLaunchKernelGGL(sync_curve_kernel, dim3(rows, blocks, chunks), dim3(SYNC_THREADS), 0, (hipStream_t)stream, a);
  MP_LAUNCH_CHECK();
  hipLaunchKernelGGL(sync_pick_kernel, dim3(rows), dim3(64), 0, (hipStream_t)stream, a);
  MP_LAUNCH_CHECK();
  return MP_OK;
}

int mp_lift_shift_views(const float* in, int V, int64_t Ftot, int64_t M, const uint8_t* valid, const int64_t* take_offset, int G,
                        const float* lag, int mode, float* out, uint8_t* valid_out, void* stream) {
  MP_CHECK(in && take_offset && lag && out && valid_out, MP_ERR_ARG, "mp_lift_shift_views: null pointer");
  if (int rc = lift_take_shape("mp_lift_shift_views", V, (long)Ftot, 2, G)) return rc;
  MP_CHECK(Ftot <= 0x7fffffffL, MP_ERR_ARG, "mp_lift_shift_views: Ftot=%ld G=%d out of range", (long)Ftot, G);
  MP_CHECK(M >= 1 && M <= MP_LIFT_SHIFT_MAXM, MP_ERR_ARG, "mp_lift_shift_views: M=%ld outside 1..%d", (long)M, MP_LIFT_SHIFT_MAXM);
  MP_CHECK(mode == 0 || mode == 1, MP_ERR_ARG, "mp_lift_shift_views: mode=%d (0: nearest, 1: linear)", mode);
  const long total = (long)V * (long)Ftot * (long)M;
  const long blocks = (total + SYNC_THREADS - 1) / SYNC_THREADS;
  MP_CHECK(blocks <= 0x7fffffffL, MP_ERR_ARG, "mp_lift_shift_views: %ld floats: too many for one launch", total);
  const uintptr_t a0 = (uintptr_t)in, b0 = (uintptr_t)out, bytes = (uintptr_t)total * 4;
  MP_CHECK(a0 + bytes <= b0 || b0 + bytes <= a0, MP_ERR_ARG, "mp_lift_shift_views: in and out overlap");
  ShiftArgs a = {};
  a.in = in; a.valid = valid; a.take_offset = (const long*)take_offset; a.lag = lag; a.out = out; a.valid_out = valid_out;
  a.Ftot = (long)Ftot; a.M = (long)M; a.total = total; a.V = V; a.G = G; a.mode = mode;
  hipLaunchKernelGGL(sync_shift_kernel, dim3((unsigned)blocks), dim3(SYNC_THREADS), 0, (hipStream_t)stream, a);
  MP_LAUNCH_CHECK();
  return MP_OK;
}

}  // extern "C"

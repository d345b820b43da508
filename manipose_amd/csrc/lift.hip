// Sequence lifting, output side (include/manipose_hip.h: mp_lift_merge) and its 2-D-only input side (mp_lift_windows_2d).
//   reference: lift_action, hpe/eval_utils.py:226-253 (used by hpe/viz.py:84-91) = non-overlapping windows with drop_last=False replicate
//   padding (hpe/mh_so3_hpe/data/generators.py:93-104,135-154) + the flip-TTA evaluation loop (eval_utils.py:84-142) +
//   RMCLManifoldMixSTE.aggregate (rmcl_manifold_mix_ste.py:141-185), predictions flattened to (windows * T, 17, 3).
// lift_merge_kernel turns the model's hypotheses (F*W, K, T, J, 3) and scores (F*W, K, T) into ONE pose per real frame of every sequence:
// aggregation over the K hypotheses, the average with the un-mirrored prediction of the mirrored copy, and the blend over the windows
// that cover the frame, in one pass.  It GATHERS: the thread that owns output float (frame, j, c) walks the frame's covering windows in
// increasing w and the hypotheses in increasing k - a fixed summation order, no atomics, identical bits on every call.
// Lanes run over the contiguous (t, j, c) floats of a (window, k) plane, so a wave reads 256 consecutive bytes of a plane per load and
// writes 256 consecutive bytes of `out`; the mirror gather moves a lane within its frame's 204-byte row.  One workgroup owns
// 256 / (3 J) whole frames; one thread per frame first finds the covering windows in the tables (binary search over the windows in
// their sorted order, or arithmetic when the host found one uniform stride) and leaves them in LDS for the frame's 3 J lanes.
// Traffic: every hypothesis float the output needs is read once, 4 F K B per output float at stride = T; HBM-bound.
#include "lift_common.h"
#include "../../include/manipose_hip.h"

namespace mp {

constexpr int LIFT_MAXK = 8, LIFT_THREADS = 256;
struct LiftArgs {
  const float* poses; const float* scores;
  const long* seq_offset; const int* win_seq; const int* win_start;
  float* out; float* hyps;
  long Ntot;
  int W, K, T, J, F, agg, blend, stride;
  float scale;
  unsigned char mirror[LIFT_MAXJ];
};

// p_w of one half (original or mirrored) at window-half plane row `wh`, frame t, float i of the frame row
__device__ __forceinline__ float lift_aggregate(const LiftArgs& a, long wh, int t, int i, float sx) {
  const long TJ3 = (long)a.T * a.J * 3;
  const float* pr = a.poses + wh * a.K * TJ3 + (long)t * a.J * 3 + i;
  if (a.scores == nullptr) return sx * pr[0];                         // K == 1
  const float* sc = a.scores + wh * a.K * a.T + t;
  if (a.agg == 0) {
    float p = 0.f;
    for (int k = 0; k < a.K; ++k) p += sc[(long)k * a.T] * pr[k * TJ3];
    return sx * p;
  }
  int kb = 0;
  float best = -INFINITY;
  for (int k = 0; k < a.K; ++k) {                                      // first maximal score, as aggregate_kernel (wta_loss.hip)
    const float s = sc[(long)k * a.T];
    if (s > best) { best = s; kb = k; }
  }
  return sx * pr[kb * TJ3];
}

template <bool HYPS>
__global__ __launch_bounds__(LIFT_THREADS) void lift_merge_kernel(LiftArgs a) {
  __shared__ int s_lo[LIFT_THREADS / 3], s_hi[LIFT_THREADS / 3], s_f[LIFT_THREADS / 3];
  const int J3 = a.J * 3;
  const int fpb = LIFT_THREADS / J3;                                   // whole frames of this workgroup
  const long g0 = (long)blockIdx.x * fpb;
  if ((int)threadIdx.x < fpb && g0 + threadIdx.x < a.Ntot) {
    const long g = g0 + threadIdx.x;
    // hi = the last window that starts at or before frame g (windows are sorted by sequence, then start: their first frames
    // seq_offset[win_seq] + win_start increase with w); it belongs to g's sequence because every frame is covered (host check)
    int lo = 0, hi = a.W - 1;
    while (lo < hi) {
      const int m = (lo + hi + 1) >> 1;
      if (a.seq_offset[a.win_seq[m]] + a.win_start[m] <= g) lo = m; else hi = m - 1;
    }
    hi = lo;
    const int s = a.win_seq[hi];
    const int f = (int)(g - a.seq_offset[s]);
    if (a.stride > 0) {                                                // uniform stride: the first covering window by arithmetic
      const int first = f >= a.T ? (f - a.T) / a.stride + 1 : 0;
      lo = hi - (a.win_start[hi] / a.stride - first);
    } else {                                                           // from the tables: first window of s with start + T > f
      int l = 0, h = hi;
      while (l < h) {
        const int m = (l + h) >> 1;
        if (a.win_seq[m] == s && a.win_start[m] + a.T > f) h = m; else l = m + 1;
      }
      lo = l;
    }
    if (a.blend == 1) {                                                // "center": nearest window centre start + (T-1)/2, lower w on a tie
      int wb = lo, db = abs(2 * (f - a.win_start[lo]) - (a.T - 1));
      for (int w = lo + 1; w <= hi; ++w) {
        const int d = abs(2 * (f - a.win_start[w]) - (a.T - 1));
        if (d < db) { db = d; wb = w; }
      }
      lo = hi = wb;
    }
    s_lo[threadIdx.x] = lo; s_hi[threadIdx.x] = hi; s_f[threadIdx.x] = f;
  }
  __syncthreads();
  const int fl = threadIdx.x / J3, i = threadIdx.x - fl * J3;
  const long g = g0 + fl;
  if (fl >= fpb || g >= a.Ntot) return;
  const int lo = s_lo[fl], hi = s_hi[fl], f = s_f[fl];
  const int j = i / 3, c = i - 3 * j;
  const int im = a.mirror[j] * 3 + c;                                  // the same frame row, mirrored joint
  const float sx = c == 0 ? -1.f : 1.f;
  const long TJ3 = (long)a.T * J3;
  float acc = 0.f;
  float hy[LIFT_MAXK], hs[LIFT_MAXK];
  if (HYPS) {
#pragma unroll
    for (int k = 0; k < LIFT_MAXK; ++k) { hy[k] = 0.f; hs[k] = 0.f; }
  }
  for (int w = lo; w <= hi; ++w) {
    const int t = f - a.win_start[w];
    float p = lift_aggregate(a, w, t, i, 1.f);
    if (a.F == 2) p = 0.5f * (p + lift_aggregate(a, (long)a.W + w, t, im, sx));
    acc = w == lo ? p : acc + p;
    if (HYPS) {                                                        // the original pass only (return_hyps, eval_utils.py:226-253)
      const float* pr = a.poses + (long)w * a.K * TJ3 + (long)t * J3 + i;
      const float* sc = a.scores != nullptr ? a.scores + (long)w * a.K * a.T + t : nullptr;
#pragma unroll
      for (int k = 0; k < LIFT_MAXK; ++k) {
        if (k < a.K) {
          const float v = pr[k * TJ3], q = sc != nullptr ? sc[(long)k * a.T] : 1.f;
          hy[k] = w == lo ? v : hy[k] + v;
          hs[k] = w == lo ? q : hs[k] + q;
        }
      }
    }
  }
  const int n = hi - lo + 1;
  const float fn = (float)n;
  if (n > 1) acc = acc / fn;
  a.out[g * J3 + i] = acc * a.scale;
  if (HYPS) {
    float* ho = a.hyps + (g * a.K * a.J + j) * 4 + c;
#pragma unroll
    for (int k = 0; k < LIFT_MAXK; ++k) {
      if (k < a.K) {
        float v = hy[k], q = hs[k];
        if (n > 1) { v = v / fn; q = q / fn; }
        ho[(long)k * a.J * 4] = v * a.scale;
        if (c == 0) ho[(long)k * a.J * 4 + 3] = q;                     // scores are never scaled
      }
    }
  }
}

// 2-D-only window gather: gather_windows_kernel (windows.hip) without the 3-D targets a lifted video does not have
struct Lift2dArgs {
  const float* p2; const long* seq_offset; const int* win_seq; const int* win_start; const unsigned char* win_flip;
  float* X;
  int B, T, J;
  unsigned char mirror[LIFT_MAXJ];
};

__global__ __launch_bounds__(256) void lift_windows_2d_kernel(Lift2dArgs a) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;          // (w, t, j)
  const long n = (long)a.B * a.T * a.J;
  if (i >= n) return;
  const int j = (int)(i % a.J);
  const long wt = i / a.J;
  const int t = (int)(wt % a.T), w = (int)(wt / a.T);
  const int s = a.win_seq[w];
  const long f0 = a.seq_offset[s], len = a.seq_offset[s + 1] - f0;
  const long f = f0 + min((long)a.win_start[w] + t, len - 1);          // replicate the last frame past the end of the sequence
  const bool flip = a.win_flip != nullptr && a.win_flip[w] != 0;
  const int js = flip ? a.mirror[j] : j;
  const float2 u = *reinterpret_cast<const float2*>(a.p2 + (f * a.J + js) * 2);
  *reinterpret_cast<float2*>(a.X + i * 2) = make_float2(flip ? -u.x : u.x, u.y);
}

static int lift_mirror(const char* who, const int* mirror, int J, unsigned char* dst) {
  for (int j = 0; j < J; ++j) {
    const int m = mirror ? mirror[j] : j;
    MP_CHECK(m >= 0 && m < J, MP_ERR_ARG, "%s: mirror[%d] = %d out of range", who, j, m);
    dst[j] = (unsigned char)m;
  }
  return MP_OK;
}

}  // namespace mp
using namespace mp;

extern "C" {

int mp_lift_merge(const float* poses, const float* scores, int W, int K, int T, int J, int tta, const int32_t* win_seq,
                  const int32_t* win_start, const int64_t* seq_offset, int S, const int32_t* h_win_seq, const int32_t* h_win_start,
                  const int64_t* h_seq_offset, const int32_t* mirror, int agg, int blend, float scale, float* out, float* hyps,
                  void* stream) {
  static_assert(sizeof(long) == sizeof(int64_t), "LP64");
  MP_CHECK(poses && win_seq && win_start && seq_offset && h_win_seq && h_win_start && h_seq_offset && out, MP_ERR_ARG,
           "mp_lift_merge: null pointer");
  MP_CHECK(K >= 1 && K <= LIFT_MAXK, MP_ERR_ARG, "mp_lift_merge: K=%d outside 1..%d", K, LIFT_MAXK);
  MP_CHECK(J >= 1 && J <= LIFT_MAXJ, MP_ERR_ARG, "mp_lift_merge: J=%d outside 1..%d", J, LIFT_MAXJ);
  MP_CHECK(W > 0 && T > 0 && S > 0, MP_ERR_ARG, "mp_lift_merge: W=%d T=%d S=%d out of range", W, T, S);
  MP_CHECK(agg == 0 || agg == 1, MP_ERR_ARG, "mp_lift_merge: agg %d (0 weighted_ave, 1 best_score)", agg);
  MP_CHECK(blend == 0 || blend == 1, MP_ERR_ARG, "mp_lift_merge: blend %d (0 mean, 1 center)", blend);
  MP_CHECK(scores != nullptr || K == 1, MP_ERR_ARG, "mp_lift_merge: null scores with K=%d hypotheses", K);
  MP_CHECK(!tta || mirror != nullptr, MP_ERR_ARG, "mp_lift_merge: test-time augmentation without a joint mirror table");
  MP_CHECK((long)(tta ? 2 : 1) * W <= 0x7fffffffL / K, MP_ERR_ARG, "mp_lift_merge: %d windows of %d hypotheses: too many", W, K);
  // the tables, on their host copies: windows sorted by sequence then start, every start inside its sequence, every frame covered
  MP_CHECK(h_seq_offset[0] == 0, MP_ERR_ARG, "mp_lift_merge: seq_offset[0] = %ld, not 0", (long)h_seq_offset[0]);
  for (int s = 0; s < S; ++s)
    MP_CHECK(h_seq_offset[s + 1] > h_seq_offset[s] && h_seq_offset[s + 1] - h_seq_offset[s] <= 0x7fffffffL, MP_ERR_ARG,
             "mp_lift_merge: sequence %d has %ld frames", s, (long)(h_seq_offset[s + 1] - h_seq_offset[s]));
  int stride = -1;                                                     // -1 not seen yet, 0 not uniform
  int w = 0;
  for (int s = 0; s < S; ++s) {
    const long len = h_seq_offset[s + 1] - h_seq_offset[s];
    MP_CHECK(w < W && h_win_seq[w] == s, MP_ERR_ARG, "mp_lift_merge: a frame that no window covers (sequence %d frame 0%s)", s,
             w < W && h_win_seq[w] < s ? "; windows are not sorted by sequence" : "");
    MP_CHECK(h_win_start[w] == 0, MP_ERR_ARG, "mp_lift_merge: a frame that no window covers (sequence %d frame 0; its first window starts at %d)",
             s, h_win_start[w]);
    long covered = T;
    for (++w; w < W && h_win_seq[w] == s; ++w) {
      const int d = h_win_start[w] - h_win_start[w - 1];
      MP_CHECK(d > 0, MP_ERR_ARG, "mp_lift_merge: window %d does not start after window %d of sequence %d", w, w - 1, s);
      MP_CHECK(h_win_start[w] < len, MP_ERR_ARG, "mp_lift_merge: window %d starts at %d, past the %ld frames of sequence %d", w, h_win_start[w],
               len, s);
      MP_CHECK(h_win_start[w] <= covered, MP_ERR_ARG, "mp_lift_merge: a frame that no window covers (sequence %d frame %ld)", s, covered);
      covered = (long)h_win_start[w] + T;
      stride = stride < 0 ? d : (stride == d ? stride : 0);
    }
    MP_CHECK(covered >= len, MP_ERR_ARG, "mp_lift_merge: a frame that no window covers (sequence %d frame %ld)", s, covered);
  }
  MP_CHECK(w == W, MP_ERR_ARG, "mp_lift_merge: window %d names sequence %d (S=%d, windows sorted by sequence)", w, h_win_seq[w], S);
  LiftArgs a = {};
  a.poses = poses; a.scores = scores; a.seq_offset = (const long*)seq_offset; a.win_seq = win_seq; a.win_start = win_start;
  a.out = out; a.hyps = hyps; a.Ntot = (long)h_seq_offset[S];
  a.W = W; a.K = K; a.T = T; a.J = J; a.F = tta ? 2 : 1; a.agg = agg; a.blend = blend; a.stride = stride > 0 ? stride : 0; a.scale = scale;
  if (int rc = lift_mirror("mp_lift_merge", mirror, J, a.mirror)) return rc;
  const long blocks = (a.Ntot + LIFT_THREADS / (J * 3) - 1) / (LIFT_THREADS / (J * 3));
  MP_CHECK(blocks <= 0x7fffffffL, MP_ERR_ARG, "mp_lift_merge: %ld frames: too many for one launch", a.Ntot);
  if (hyps != nullptr) hipLaunchKernelGGL(lift_merge_kernel<true>, dim3((unsigned)blocks), dim3(LIFT_THREADS), 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(lift_merge_kernel<false>, dim3((unsigned)blocks), dim3(LIFT_THREADS), 0, (hipStream_t)stream, a);
  MP_LAUNCH_CHECK();
  return MP_OK;
}

int mp_lift_windows_2d(const float* poses_2d, const int64_t* seq_offset, int S, const int32_t* win_seq, const int32_t* win_start,
                       const uint8_t* win_flip, const int32_t* mirror, int B, int T, int J, float* X, void* stream) {
  MP_CHECK(poses_2d && seq_offset && win_seq && win_start && X, MP_ERR_ARG, "mp_lift_windows_2d: null pointer");
  MP_CHECK(B > 0 && T > 0 && S > 0 && J > 0 && J <= LIFT_MAXJ, MP_ERR_ARG, "mp_lift_windows_2d: B=%d T=%d S=%d J=%d out of range", B, T, S, J);
  MP_CHECK(win_flip == nullptr || mirror != nullptr, MP_ERR_ARG, "mp_lift_windows_2d: flip flags without a joint mirror table");
  Lift2dArgs a = {};
  a.p2 = poses_2d; a.seq_offset = (const long*)seq_offset; a.win_seq = win_seq; a.win_start = win_start; a.win_flip = win_flip;
  a.X = X; a.B = B; a.T = T; a.J = J;
  if (int rc = lift_mirror("mp_lift_windows_2d", mirror, J, a.mirror)) return rc;
  const long n = (long)B * T * J;
  hipLaunchKernelGGL(lift_windows_2d_kernel, dim3(cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, a);
  MP_LAUNCH_CHECK();
  return MP_OK;
}

}  // extern "C"

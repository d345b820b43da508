// Fitting a fused take's skeleton ALONG TIME (include/manipose_hip.h: mp_lift_fit_skeleton_smooth has the rule).  mp_lift_fit_skeleton fits every
// frame on its own, so every frame keeps its own keypoint noise and the fitted body jitters.  Here the frames of a take share one cost: the
// frames' own reprojection costs plus smooth times the squared second differences of the joint positions, and that cost is lowered by sweeps over
// the frames in three colours: in a visit a frame takes ONE Gauss-Newton step of mp_lift_fit_skeleton's rule with its neighbours held, on its
// own cost plus the pull smooth W_t |p_j - q_j|^2 that the smoothness terms reduce to.  tests/lift_skeleton_smooth_ref.py states the rule in float64.
//
// STAGE A is lift_skeleton.h's lift_fit_skeleton_kernel with STATE set: mp_lift_fit_skeleton's bits, and the frame's (r, d, p) kept in fp64 in the
// scratch buffer, 6 J doubles a frame.  STAGE B launches the visit kernel 3 x sweeps times, one launch a colour: one 64-lane workgroup a frame, as
// in stage A.  A frame of another colour, outside its take, without a result or without a smoothness term leaves before the first barrier;
// W_t comes from the ok bytes of frames t-2 .. t+2, which every lane reads alike.  Lane j forms q_j from the neighbours' fp64 positions; a visited
// frame reads frames t+-1 and t+-2, which have other colours, and writes only its own state: nothing is read and written in one launch.  The
// evaluation, the step and the accept rule are lift_skeleton.h's and lift_geom.h's.  No atomics, no register arrays, no scratch memory.
#include "lift_common.h"

#pragma clang fp contract(off)
#include "lift_geom.h"                    // after the pragma: the shared code takes this file's mode
#include "lift_skeleton.h"

namespace mp {

__global__ __launch_bounds__(SK_THREADS) void lift_skeleton_visit_kernel(SkelArgs A, double smooth, int colour) {
  __shared__ SkelLds L;
  const long f = blockIdx.x;
  const int lane = threadIdx.x, J = A.J, NB = J - 1;
  const int g = lift_seq_of(A.take_offset, A.G, f);
  const FrameRange fr = lift_seq_frames(A.take_offset, g, A.Ftot);
  if (f < fr.f0 || f >= fr.f1 || (int)((f - fr.f0) % 3) != colour) return;
  // the stencil: the terms centred at t-1, t, t+1 that exist (every lane alike)
  const bool u0 = (A.ok[f] & 1) != 0;
  const bool m2 = f - 2 >= fr.f0 && (A.ok[f - 2] & 1) != 0, m1 = f - 1 >= fr.f0 && (A.ok[f - 1] & 1) != 0;
  const bool p1 = f + 1 < fr.f1 && (A.ok[f + 1] & 1) != 0, p2 = f + 2 < fr.f1 && (A.ok[f + 2] & 1) != 0;
  const bool ta = m2 && m1, tb = m1 && p1, tc = p1 && p2;
  const int W = (ta ? 1 : 0) + (tb ? 4 : 0) + (tc ? 1 : 0);
  if (!u0 || W == 0) return;
  const double cm1 = (ta ? 2.0 : 0.0) + (tb ? 2.0 : 0.0), cp1 = (tb ? 2.0 : 0.0) + (tc ? 2.0 : 0.0), cm2 = ta ? 1.0 : 0.0, cp2 = tc ? 1.0 : 0.0;
  const long stride = 6L * J;
  double* mine = A.state + f * stride;
  SkelPull q = {smooth * (double)W, 0.0, 0.0, 0.0};
  double x0 = 0.0, y0 = 0.0, z0 = 0.0;
  if (lane < J) {
    const float* P = A.start + (f * J + lane) * 3;
    x0 = P[0]; y0 = P[1]; z0 = P[2];
    const double* at = mine + 3 + 3 * NB + 3 * lane;                    // p_j of this frame; a frame without a coefficient is not read and counts 0
    const double* a1 = at - stride; const double* b1 = at + stride; const double* a2 = at - 2 * stride; const double* b2 = at + 2 * stride;
    const bool hm1 = ta || tb, hp1 = tb || tc;
    q.x = ((cm1 * (hm1 ? a1[0] : 0.0) + cp1 * (hp1 ? b1[0] : 0.0)) - (cm2 * (ta ? a2[0] : 0.0) + cp2 * (tc ? b2[0] : 0.0))) / (double)W;
    q.y = ((cm1 * (hm1 ? a1[1] : 0.0) + cp1 * (hp1 ? b1[1] : 0.0)) - (cm2 * (ta ? a2[1] : 0.0) + cp2 * (tc ? b2[1] : 0.0))) / (double)W;
    q.z = ((cm1 * (hm1 ? a1[2] : 0.0) + cp1 * (hp1 ? b1[2] : 0.0)) - (cm2 * (ta ? a2[2] : 0.0) + cp2 * (tc ? b2[2] : 0.0))) / (double)W;
  }
  if (lane < NB) L.len[lane] = A.lengths[(long)g * NB + lane];
  skel_state<false>(L, 0, mine, J);                                     // the state in slot 0 (skel_eval opens with the barrier)
  const int mask = skel_observed(A, f, g);
  const bool seen = __any(mask != 0) != 0;
  // one step of rules 3 to 9 on the conditional cost
  const SkelCost k0 = skel_eval<true, true>(A, L, 0, f, g, mask, x0, y0, z0, q);
  if (!(k0.deep && __builtin_isfinite(k0.F))) return;
  if (!skel_step(A, L, 0, 1)) return;
  const SkelCost k1 = skel_eval<false, true>(A, L, 1, f, g, mask, x0, y0, z0, q);
  LiftGN e = lift_gn_start(), n = lift_gn_start();
  e.F = k0.F; e.deep = k0.deep;
  n.F = k1.F; n.deep = k1.deep;
  if (!lift_gn_accept(n, e)) return;
  __syncthreads();
  skel_state<true>(L, 1, mine, J);
  float* out = A.pose + f * J * 3;
  for (int i = lane; i < J * 3; i += SK_THREADS) out[i] = (float)L.p[1][i / 3][i % 3];
  if (lane == 0) {
    A.err[f * 3 + 2] = (float)(seen ? k1.E / k1.W : 0.0);
    if (A.moves != nullptr) A.moves[f] = (unsigned char)(A.moves[f] + 1);
  }
}

}  // namespace mp
using namespace mp;

extern "C" {

int64_t mp_lift_fit_skeleton_smooth_scratch_bytes(int64_t Ftot, int J) {
  if (J < 2 || J > LIFT_MAXJ || Ftot <= 0 || Ftot > 0x7fffffffL) return 0;
  return (int64_t)Ftot * 6 * J * 8;
}

int mp_lift_fit_skeleton_smooth(const float* start, const uint8_t* start_ok, const float* kp, const float* kp_weight, int V, int64_t Ftot, int J,
                                const uint8_t* valid, const int64_t* take_offset, int G, const float* quat, const float* trans, const float* intr,
                                const float* lengths, const int32_t* parents, int distort, float sigma, float prior, int iters, float smooth,
                                int sweeps, float* pose, float* err, uint8_t* ok, uint8_t* steps, uint8_t* moves, void* scratch,
                                int64_t scratch_bytes, void* stream) {
  SkelArgs a;
  if (int rc = skel_arguments("mp_lift_fit_skeleton_smooth", start, start_ok, kp, kp_weight, V, Ftot, J, valid, take_offset, G, quat, trans, intr, lengths,
                              parents, distort, sigma, prior, iters, pose, err, ok, steps, a))
    return rc;
  MP_CHECK(smooth >= 0.f && __builtin_isfinite(smooth), MP_ERR_ARG, "mp_lift_fit_skeleton_smooth: smooth=%g must be finite and >= 0", (double)smooth);
  MP_CHECK(sweeps >= 0 && sweeps <= MP_LIFT_SKELETON_MAXSWEEPS, MP_ERR_ARG, "mp_lift_fit_skeleton_smooth: sweeps=%d outside 0..%d", sweeps,
           MP_LIFT_SKELETON_MAXSWEEPS);
  const int64_t need = mp_lift_fit_skeleton_smooth_scratch_bytes(Ftot, J);
  MP_CHECK(scratch != nullptr && scratch_bytes >= need && ((uintptr_t)scratch & 7) == 0, MP_ERR_ARG,
           "mp_lift_fit_skeleton_smooth: scratch null, misaligned or %ld bytes where %ld are needed", (long)scratch_bytes, (long)need);
  a.state = (double*)scratch; a.moves = moves;
  const dim3 grid((unsigned)Ftot), block(SK_THREADS);
  if (iters > 0)
    hipLaunchKernelGGL((lift_fit_skeleton_kernel<true, true>), grid, block, 0, (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL((lift_fit_skeleton_kernel<false, true>), grid, block, 0, (hipStream_t)stream, a);
  MP_LAUNCH_CHECK();
  if (smooth > 0.f)
    for (int sweep = 0; sweep < sweeps; ++sweep)
      for (int colour = 0; colour < 3; ++colour) {
        hipLaunchKernelGGL(lift_skeleton_visit_kernel, grid, block, 0, (hipStream_t)stream, a, (double)smooth, colour);
        MP_LAUNCH_CHECK();
      }
  return MP_OK;
}

}  // extern "C"

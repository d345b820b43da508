// Fitting one skeleton to a fused take's keypoints (include/manipose_hip.h: mp_lift_fit_skeleton has the rule).  mp_lift_triangulate makes every
// joint of every frame a world point of its own: bone lengths change from frame to frame and nothing ties a joint to its neighbours;
// mp_lift_rigid gives constant bones by re-assembling the pose bone by bone, with no say of the keypoints.  Here a frame's pose is the root and one
// unit direction per bone of a FIXED bone table, and the 3 + 2 (J - 1) unknowns - the root, two tangent coordinates per direction - take undamped
// Gauss-Newton steps on the robust reprojection error of all joints under the full camera model, with a pull towards the start.
// tests/lift_skeleton_ref.py states the rule in float64.
//
// lift_skeleton.h has the device code - the evaluation, the step, the per-frame fit - and the host's argument checks: mp_lift_fit_skeleton_smooth
// (lift_skeleton_smooth.hip) runs the same fit as its first stage and the same step in its visits.
#include "lift_common.h"

#pragma clang fp contract(off)
#include "lift_geom.h"                    // after the pragma: the shared code takes this file's mode
#include "lift_skeleton.h"

using namespace mp;

extern "C" {

int mp_lift_fit_skeleton(const float* start, const uint8_t* start_ok, const float* kp, const float* kp_weight, int V, int64_t Ftot, int J,
                         const uint8_t* valid, const int64_t* take_offset, int G, const float* quat, const float* trans, const float* intr,
                         const float* lengths, const int32_t* parents, int distort, float sigma, float prior, int iters, float* pose, float* err,
                         uint8_t* ok, uint8_t* steps, void* stream) {
  SkelArgs a;
  if (int rc = skel_arguments("mp_lift_fit_skeleton", start, start_ok, kp, kp_weight, V, Ftot, J, valid, take_offset, G, quat, trans, intr, lengths, parents,
                              distort, sigma, prior, iters, pose, err, ok, steps, a))
    return rc;
  if (iters > 0)
    hipLaunchKernelGGL(lift_fit_skeleton_kernel<true>, dim3((unsigned)Ftot), dim3(SK_THREADS), 0, (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL(lift_fit_skeleton_kernel<false>, dim3((unsigned)Ftot), dim3(SK_THREADS), 0, (hipStream_t)stream, a);
  MP_LAUNCH_CHECK();
  return MP_OK;
}

}  // extern "C"

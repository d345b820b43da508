"""The take-level operators of lifting: the camera views of a take - V sequences of the same frames, one per camera - fused into one motion in one
world.  They are NOT stages of ``lift_sequences``' chain (lifting.py): they work on what it returns for the views, and hpe/_entry.py (``lift.fuse``)
cuts a group's sequences into takes and calls them.  ``fuse_views``: one hypothesis per view, chosen jointly, and their mean;
``fuse_views_path``: that choice made jointly over the whole take, a Viterbi path over the combinations, so that a hypothesis all views agree on -
a mirrored body - cannot make the fused motion flicker; ``place_views``: one world root per frame from all views; ``align_views``: the views'
extrinsics estimated from their lifted poses, for takes that were never calibrated; ``bundle_views``: those cameras and the roots refined jointly
on the reprojection error; ``calibrate_views``: cameras, focal lengths and every joint as a free point fitted to the keypoints;
``triangulate_views``: every joint of the fused take triangulated on the keypoints of the cameras that see it;
``fit_skeleton_views``: one skeleton of constant bones fitted to those keypoints, frame by frame; ``sync_views`` /
``shift_views``: the views' lags in time estimated from their poses, and any per-view array put on the reference view's clock.  Built
like lift_ops.py: a public function composes lift_args' checks (``_fuse_front`` and ``_take_front`` are the
fronts two of them share), then uploads and calls its private launcher, which allocates the outputs and goes through ``_launch``.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np
import torch

from . import _lib, lift_args
from .lift_ops import PATH_SIGMA, PATH_SWITCH, REFINE_MAXITERS, _host_f32, _launch, _parents_c, _seq_table, _skeleton_of, camera_table

FUSE_MAXV, FUSE_MAXK = 4, 8  # MP_LIFT_FUSE_MAXV, MP_LIFT_FUSE_MAXK of include/manipose_hip.h: views of a take, hypotheses of a view
FUSE_SIGMA, FUSE_SCORE_WEIGHT = 0.02, 1.0    # defaults of fuse_views: the views' disagreement in metres (not tuned), the weight of -log(score)


def _fuse_quat(orientation, G, V):
    """(G, V, 4) float32 host quaternions, (V, 4) standing for one take; a zero quaternion is refused here (the kernel would ignore the view)"""
    h = _host_f32(orientation, (G, V, 4), "orientation", row=(V, 4) if G == 1 else None)
    if not ((h.astype(np.float64) ** 2).sum(-1) >= 1e-12).all():
        raise ValueError("orientation holds a zero quaternion: mark a missing view in valid and give it any unit quaternion")
    return h


def _fuse_outputs(hyps):
    """what mp_lift_fuse and mp_lift_fuse_path both write: (pose (Ftot, J, 3), choice (Ftot, V), cost, spread, ok (Ftot)), uninitialised"""
    V, ftot, _, J, _ = (int(v) for v in hyps.shape)
    dev = hyps.device
    return (torch.empty(ftot, J, 3, dtype=torch.float32, device=dev), torch.empty(ftot, V, dtype=torch.uint8, device=dev),
            torch.empty(ftot, dtype=torch.float32, device=dev), torch.empty(ftot, dtype=torch.float32, device=dev),
            torch.empty(ftot, dtype=torch.uint8, device=dev))


def _fuse(lib, hyps, valid, d_off, G, d_quat, sigma, score_weight):
    """``mp_lift_fuse`` on hyps (V, Ftot, K, J, C): (pose, choice, cost, spread, ok), new tensors"""
    V, ftot, K, J, ch = (int(v) for v in hyps.shape)
    pose, choice, cost, spread, ok = _fuse_outputs(hyps)
    if ftot > 0:
        _launch(hyps.device, "mp_lift_fuse", _lib.ptr(hyps), V, ftot, K, J, ch, _lib.ptr(valid), _lib.ptr(d_off), G, _lib.ptr(d_quat), float(sigma),
                float(score_weight), _lib.ptr(pose), _lib.ptr(choice), _lib.ptr(cost), _lib.ptr(spread), _lib.ptr(ok))
    return pose, choice, cost, spread, ok


def _fuse_place(lib, pose, kp, valid, d_off, G, d_quat, d_trans, d_intr, d_w, distort, iters):
    """``mp_lift_fuse_place`` on pose (Ftot, J, 3), kp (V, Ftot, J, 2): (root, reproj, ok, steps), new tensors"""
    V, ftot, J = int(kp.shape[0]), int(kp.shape[1]), int(kp.shape[2])
    dev = pose.device
    root = torch.empty(ftot, 3, dtype=torch.float32, device=dev)
    reproj = torch.empty(V, ftot, dtype=torch.float32, device=dev)
    ok = torch.empty(ftot, dtype=torch.uint8, device=dev)
    steps = torch.empty(ftot, dtype=torch.uint8, device=dev)
    if ftot > 0:
        _launch(dev, "mp_lift_fuse_place", _lib.ptr(pose), _lib.ptr(kp), V, ftot, J, _lib.ptr(valid), _lib.ptr(d_off), G, _lib.ptr(d_quat),
                _lib.ptr(d_trans), _lib.ptr(d_intr), _lib.ptr(d_w), int(bool(distort)), int(iters), _lib.ptr(root), _lib.ptr(reproj), _lib.ptr(ok),
                _lib.ptr(steps))
    return root, reproj, ok, steps


def _fuse_front(who, hyps, orientation, valid, take_offset):
    """what fuse_views and fuse_views_path do between their options and their launch: the checks of hyps, valid and orientation, the refusal of CPU
    tensors, the uploads: (valid, d_off, G, d_quat)"""
    if torch.is_tensor(hyps):
        lift_args.hyps5(hyps, FUSE_MAXV, FUSE_MAXK)       # (the ValueErrors come before the refusal of a CPU tensor)
        V, ftot = int(hyps.shape[0]), int(hyps.shape[1])
        lift_args.mask(valid, (V, ftot), "valid")
        h_quat = _fuse_quat(orientation, lift_args.take_count(take_offset), V) if orientation is not None else None
    lift_args.need_device(who, hyps, optional=(valid,))
    valid = valid.contiguous() if valid is not None else None
    d_off, G = _seq_table(take_offset, ftot, hyps.device)
    return valid, d_off, G, torch.from_numpy(h_quat).to(hyps.device) if h_quat is not None else None


def fuse_views(hyps, orientation=None, valid=None, take_offset=None, sigma=FUSE_SIGMA, score_weight=FUSE_SCORE_WEIGHT):
    """``mp_lift_fuse`` on device tensors: the camera views of a take fused into one pose per frame.  ``hyps`` (V, Ftot, K, J, 3 | 4) float32, the
    K hypotheses of each of V <= 4 views of the same frames, each in its camera's frame (channel 3 of joint 0: the hypothesis' score; without it
    every hypothesis is equally likely); ``orientation`` (G, V, 4) or, for one take, (V, 4) camera quaternions (w, x, y, z), tensor or array,
    normalised in the kernel, or None: the views are in the world's orientation already; ``valid`` (V, Ftot) uint8 device tensor or None: 0 where a
    view is missing (a take with fewer than V views: all of its frames); ``take_offset`` (G + 1): first frame of every take, HOST table or device
    int64 tensor (default: one take).  Per frame the ONE combination of a hypothesis per valid view is chosen that minimises
    sum_{a < b} mean_j |w_a - w_b|^2 / (2 sigma^2) + score_weight sum_v -log(score_v), w the root-relative hypothesis rotated into the world - the
    first minimum in lexicographic order - and the chosen hypotheses are averaged (include/manipose_hip.h has the rule).  ``sigma`` > 0 in the
    poses' unit (inf: the views do not see each other and every view takes its best score), ``score_weight`` >= 0.  Returns ``(pose (Ftot, J, 3)
    root-relative in the world's orientation, choice (Ftot, V) uint8 (255: invalid view), cost (Ftot), spread (Ftot) the chosen hypotheses' RMS
    distance from their mean, ok (Ftot) uint8)``, new device tensors.  hyps is not modified; identical bits on every call."""
    lift_args.sigma_pair(sigma, score_weight, ("sigma", "score_weight"))
    valid, d_off, G, d_quat = _fuse_front("fuse_views", hyps, orientation, valid, take_offset)
    return _fuse(_lib.load(), hyps, valid, d_off, G, d_quat, sigma, score_weight)


def _fuse_path(lib, hyps, valid, d_off, G, d_quat, sigma, score_weight, path_sigma, switch_cost):
    """``mp_lift_fuse_path`` on hyps (V, Ftot, K, J, C): (pose, choice, cost, spread, ok, path_cost (G,) float64), new tensors"""
    V, ftot, K, J, ch = (int(v) for v in hyps.shape)
    dev = hyps.device
    pose, choice, cost, spread, ok = _fuse_outputs(hyps)
    path_cost = torch.zeros(G, dtype=torch.float64, device=dev)
    if ftot > 0:
        n = int(lib.mp_lift_fuse_path_scratch_bytes(V, ftot, K))
        scratch = torch.empty(n // 8, dtype=torch.float64, device=dev)
        _launch(dev, "mp_lift_fuse_path", _lib.ptr(hyps), V, ftot, K, J, ch, _lib.ptr(valid), _lib.ptr(d_off), G, _lib.ptr(d_quat), float(sigma),
                float(score_weight), float(path_sigma), float(switch_cost), _lib.ptr(pose), _lib.ptr(choice), _lib.ptr(cost), _lib.ptr(spread),
                _lib.ptr(ok), _lib.ptr(path_cost), _lib.ptr(scratch), n)
    return pose, choice, cost, spread, ok, path_cost


def fuse_views_path(hyps, orientation=None, valid=None, take_offset=None, sigma=FUSE_SIGMA, score_weight=FUSE_SCORE_WEIGHT, path_sigma=PATH_SIGMA,
                    switch_cost=PATH_SWITCH):
    """``mp_lift_fuse_path`` on device tensors: the camera views of a take fused along time.  The arguments are ``fuse_views``'; the choice is not
    made frame by frame but jointly over the whole take: the cheapest PATH through the combinations (one hypothesis per view: K^V states, at most
    4096) under ``fuse_views``' cost per frame and, per view, ``select_path``'s cost per step - mean_j |w_b[j] - w_a[j]|^2 / (2 path_sigma^2) +
    (switch_cost if a != b) from hypothesis a of a frame to hypothesis b of the next, w the rotated root-relative hypothesis; by the Viterbi
    algorithm in fp64, staged per view, ties to the first combination (include/manipose_hip.h has the rule).  ``fuse_views`` takes a hypothesis
    that all views agree on - a left/right-mirrored body - in every frame where its score is higher, and the fused motion flickers; the path does
    not jump.  A view missing at a frame (``valid``) has no say there and its chain is cut.  ``path_sigma`` > 0 in the poses' unit (inf: steps cost
    nothing, and with switch_cost = 0 the choice is ``fuse_views``'), ``switch_cost`` >= 0.  Returns ``(pose, choice, cost, spread, ok, path_cost
    (G,) float64: the cost of every take's path)``, the first five as ``fuse_views`` returns them, new device tensors.  A frame that no take of
    ``take_offset`` holds is left unwritten.  hyps is not modified; identical bits on every call.  Not measured on real data."""
    lift_args.sigma_pair(sigma, score_weight, ("sigma", "score_weight"))
    lift_args.sigma_pair(path_sigma, switch_cost, ("path_sigma", "switch_cost"))
    valid, d_off, G, d_quat = _fuse_front("fuse_views_path", hyps, orientation, valid, take_offset)
    return _fuse_path(_lib.load(), hyps, valid, d_off, G, d_quat, sigma, score_weight, path_sigma, switch_cost)


def _take_cameras(cameras, V):
    """cameras[take][view] (camera_table's forms, None: a missing view) -> host (intr (G, V, 9), quat (G, V, 4), trans (G, V, 3), present (G, V) bool);
    a missing view gets the identity camera, which is never read"""
    if isinstance(cameras, dict) or not hasattr(cameras, "__len__") or len(cameras) == 0:
        raise ValueError("cameras must be a nested list [take][view] of cameras (None: a missing view)")
    G = len(cameras)
    intr, quat, trans = np.zeros((G, V, 9), np.float32), np.zeros((G, V, 4), np.float32), np.zeros((G, V, 3), np.float32)
    present = np.zeros((G, V), bool)
    intr[..., 0:2], quat[..., 0] = 1.0, 1.0
    for g, take in enumerate(cameras):
        if isinstance(take, dict) or not hasattr(take, "__len__") or len(take) != V:
            raise ValueError(f"cameras[{g}] must list {V} views (None: a missing view)")
        for v, cam in enumerate(take):
            if cam is None:
                continue
            try:
                i, q, t = camera_table([cam])
            except ValueError as e:
                raise ValueError(f"take {g}, view {v}: {e}") from None
            if not float((q.astype(np.float64) ** 2).sum()) >= 1e-12:
                raise ValueError(f"take {g}, view {v}: zero quaternion")
            intr[g, v], quat[g, v], trans[g, v], present[g, v] = i[0], q[0], t[0], True
    return intr, quat, trans, present


def _take_front(who, pose, keypoints_2d, cameras, valid, take_offset, weights, roots=None, ok_name="root_ok"):
    """What place_views and bundle_views do before their uploads: the checks of the take's pose, keypoints, masks, cameras and weights - with ``roots`` =
    (root, root_ok, fixed) also of bundle_views' three, each where bundle_views has always checked it (a root of None: there is none, and the mask
    of the frames goes by ``ok_name``) -, the refusal of CPU tensors, the offsets'
    upload, and the mask that makes a missing view (None in ``cameras``) invalid in every frame of its take: (valid, d_off, G, (intr, quat, trans,
    present) host tables, h_w, h_fixed)"""
    root, root_ok, fixed = roots if roots is not None else (None, None, None)
    given = (pose, keypoints_2d) if root is None else (pose, root, keypoints_2d)
    if all(torch.is_tensor(t) for t in given):
        V, ftot, J = lift_args.take_pose_keypoints(pose, keypoints_2d, FUSE_MAXV, root)
        lift_args.mask(valid, (V, ftot), "valid")
        lift_args.mask(root_ok, (ftot,), ok_name, bare=True)
        cams = _take_cameras(cameras, V)
        G, present = cams[0].shape[0], cams[3]
        h_fixed = None
        if fixed is not None:
            h_fixed = np.asarray(fixed.detach().cpu().numpy() if torch.is_tensor(fixed) else fixed)
            if h_fixed.shape == (V,) and G == 1:
                h_fixed = h_fixed.reshape(1, V)
            if h_fixed.shape != (G, V) or h_fixed.dtype.kind not in "biu":
                raise ValueError(f"fixed must be a table ({G}, {V}) of flags, got {h_fixed.shape} {h_fixed.dtype}")
            h_fixed = np.ascontiguousarray(h_fixed != 0, dtype=np.uint8)
        h_w = _host_f32(weights, (J,), "weights", nonneg=True) if weights is not None else None
    lift_args.need_device(who, *given, optional=(valid, root_ok))
    dev = pose.device
    valid = valid.contiguous() if valid is not None else None
    d_off, G_off = _seq_table(take_offset, ftot, dev)
    if G_off != G:
        raise ValueError(f"cameras lists {G} takes, take_offset {G_off}")
    if not present.all():                                  # a missing view is invalid in every frame of its take
        off = d_off.cpu().numpy().clip(0, ftot)
        mask = np.ones((V, ftot), np.uint8)
        for g, v in zip(*np.nonzero(~present)):
            mask[v, off[g]:max(off[g], off[g + 1])] = 0
        mask = torch.from_numpy(mask).to(dev)
        valid = mask if valid is None else valid & mask
    return valid, d_off, G, cams, h_w, h_fixed


def place_views(pose, keypoints_2d, cameras, valid=None, take_offset=None, weights=None, distort=True, refine=3, return_steps=False):
    """``mp_lift_fuse_place`` on device tensors: ONE world root per frame from all views of its take.  ``pose`` (Ftot, J, 3) float32, root-relative
    in the world's orientation, as ``fuse_views`` returns it; ``keypoints_2d`` (V, Ftot, J, 2) float32, every view's keypoints in normalised screen
    coordinates; ``cameras``: nested list [take][view] of cameras in ``camera_table``'s forms (a dict of ``h36m_cameras()`` with its
    ``translation``, or ``fetch()``'s 16 numbers), None for a view the take does not have; ``valid`` (V, Ftot) uint8 device tensor or None;
    ``take_offset`` (G + 1) as for ``fuse_views``; ``weights`` (J) or None.  The root starts at the linear fit of all views' pinhole projections
    (condition number about 6 with H36M's four cameras, against 6e2 for one view) and takes up to ``refine`` (0..16) Gauss-Newton steps under the
    camera model ``distort`` names, with ``place_poses``' acceptance rule.  Returns ``(root (Ftot, 3), reproj (V, Ftot): every view's own mean
    reprojection error at the root, 0 for an invalid view, ok (Ftot) uint8[, steps (Ftot) uint8])``."""
    if not lift_args.is_int_in(refine, 0, REFINE_MAXITERS):
        raise ValueError(f"refine counts Gauss-Newton steps, an integer in 0..{REFINE_MAXITERS} (0: the linear fit alone), got {refine!r}")
    valid, d_off, G, (intr, quat, trans, _), h_w, _ = _take_front("place_views", pose, keypoints_2d, cameras, valid, take_offset, weights)
    dev = pose.device
    res = _fuse_place(_lib.load(), pose, keypoints_2d.contiguous(), valid, d_off, G, torch.from_numpy(quat).to(dev), torch.from_numpy(trans).to(dev),
                      torch.from_numpy(intr).to(dev), torch.from_numpy(h_w).to(dev) if h_w is not None else None, distort, refine)
    return res if return_steps else res[:3]


ALIGN_MAXITERS = 8           # MP_LIFT_ALIGN_MAXITERS of include/manipose_hip.h: re-weightings mp_lift_align_views takes at most
ALIGN_SIGMA, ALIGN_ITERS = 0.05, 5           # defaults of align_views: the scale of a frame's residual in metres, the re-weightings (not tuned)
# What align_views returns: quat (G, V, 4), trans (G, V, 3) or None, rms (G, V), trans_rms (G, V) or None float32, used (G, V) int32, ok (G, V) uint8
ViewAlignment = namedtuple("ViewAlignment", "quat trans rms trans_rms used ok")


def _quat_matrix(q):
    """the rotation matrix of q / |q| (w, x, y, z) in float64"""
    w, x, y, z = np.asarray(q, np.float64) / np.linalg.norm(np.asarray(q, np.float64))
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def _align_compose(quat, trans, ok, ref_quat, ref_trans):
    """mp_lift_align_views' rows (G, V, ..) in the reference views' frames -> in the worlds of the reference views' known extrinsics, on the host
    in float64: q = q_ref * q_v (q_ref normalised), T = R_ref T_v + T_ref.  A row whose ok lacks bit 0 is left as it is; the translation is composed
    where ok has bit 1 and for the reference view itself, the lowest view of a take with bit 0 (its T_v = 0 is known); elsewhere it stays 0.
    Returns float32 (quat, trans or None); q stays canonical (w >= 0, else the first non-zero component positive)."""
    q64, ok = np.asarray(quat, np.float64).copy(), np.asarray(ok)
    t64 = np.asarray(trans, np.float64).copy() if trans is not None else None
    for g in range(q64.shape[0]):
        a = np.asarray(ref_quat[g], np.float64)
        a = a / np.linalg.norm(a)
        R = _quat_matrix(a)
        rot = np.nonzero(ok[g] & 1)[0]
        for v in rot:
            b = q64[g, v]
            q = np.array([a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3], a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                          a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1], a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0]])
            nz = q[np.nonzero(q)[0][:1]]
            q64[g, v] = -q if nz.size and nz[0] < 0 else q
            if t64 is not None and (ok[g, v] & 2 or v == rot[0]):
                t64[g, v] = R @ t64[g, v] + np.asarray(ref_trans[g], np.float64)
    return q64.astype(np.float32), t64.astype(np.float32) if t64 is not None else None


def _align(lib, poses, valid, d_off, G, traj, traj_ok, sigma, iters):
    """``mp_lift_align_views`` on poses (V, Ftot, J, C): a ViewAlignment of new tensors"""
    V, ftot, J, ch = (int(v) for v in poses.shape)
    dev = poses.device
    quat = torch.zeros(G, V, 4, dtype=torch.float32, device=dev)
    quat[..., 0] = 1.0
    trans = torch.zeros(G, V, 3, dtype=torch.float32, device=dev) if traj is not None else None
    rms = torch.zeros(G, V, dtype=torch.float32, device=dev)
    trans_rms = torch.zeros(G, V, dtype=torch.float32, device=dev) if traj is not None else None
    used = torch.zeros(G, V, dtype=torch.int32, device=dev)
    ok = torch.zeros(G, V, dtype=torch.uint8, device=dev)
    if ftot > 0:
        _launch(dev, "mp_lift_align_views", _lib.ptr(poses), V, ftot, J, ch, _lib.ptr(valid), _lib.ptr(d_off), G, _lib.ptr(traj), _lib.ptr(traj_ok),
                float(sigma), int(iters), _lib.ptr(quat), _lib.ptr(trans), _lib.ptr(rms), _lib.ptr(trans_rms), _lib.ptr(used), _lib.ptr(ok))
    return ViewAlignment(quat, trans, rms, trans_rms, used, ok)


def align_views(poses, valid=None, take_offset=None, traj=None, traj_ok=None, sigma=ALIGN_SIGMA, iters=ALIGN_ITERS, reference=None):
    """``mp_lift_align_views`` on device tensors: the extrinsics of a take's views estimated from their lifted poses, for takes whose cameras
    were never calibrated against each other.  ``poses`` (V, Ftot, J, 3 | 4) float32, one pose per view and frame in that view's camera frame
    (channel 3 is not read); ``valid`` (V, Ftot) uint8 device tensor or None; ``take_offset`` (G + 1) as for ``fuse_views``; ``traj`` (V, Ftot, 3)
    float32 and ``traj_ok`` (V, Ftot) uint8, both or neither: the views' camera-space roots as ``place_poses`` returns them.  Per take the lowest
    view with a valid frame is the reference; every other view's rotation onto it is Horn's closed form over the root-relative poses of all
    frames valid in both, re-weighted ``iters`` (0..8) times with w = 1 / (1 + e / sigma^2)^2, e a frame's mean squared residual - a depth-mirrored
    body loses its say; ``sigma`` > 0 in the poses' unit (inf: plain Horn) - and, with ``traj``, its translation the weighted mean of
    traj_ref - R traj_v (include/manipose_hip.h has the rule).  The defaults are not tuned.  x_ref = R_v x_v + T_v: ``quat`` and ``trans`` are
    ``fuse_views``' and ``place_views``' extrinsics with the reference view's frame as the world.  ``reference``: per take one camera in
    ``camera_table``'s forms (a list of G; one camera alone for one take), the known extrinsics of the reference view: the result is composed on
    the host in float64 into that world, q = q_ref * q_v, T = R_ref T_v + T_ref (this waits for the kernel).  Returns a ``ViewAlignment``:
    ``(quat (G, V, 4), trans (G, V, 3) or None, rms (G, V): the weighted RMS residual of the poses, trans_rms (G, V) or None: that of the
    roots - a monocular depth scale error shows here -, used (G, V) int32: the frames used, ok (G, V) uint8: bit 0 the rotation, bit 1 the
    translation)``, new device tensors; a degenerate row is the identity with ok = 0.  Inputs are not modified; identical bits on every call.
    Not measured on real data."""
    if not lift_args.is_number(sigma) or not float(sigma) > 0:
        raise ValueError(f"sigma must be a number > 0 (inf: every frame weighs 1), got {sigma!r}")
    if not lift_args.is_int_in(iters, 0, ALIGN_MAXITERS):
        raise ValueError(f"iters counts re-weightings, an integer in 0..{ALIGN_MAXITERS} (0: plain Horn), got {iters!r}")
    if (traj is None) != (traj_ok is None):
        raise ValueError("traj and traj_ok come together: the views' roots and where they were fitted")
    if torch.is_tensor(poses):
        lift_args.view_poses4(poses, FUSE_MAXV)
        V, ftot = int(poses.shape[0]), int(poses.shape[1])
        lift_args.mask(valid, (V, ftot), "valid")
        if traj is not None:
            lift_args.f32(traj, (V, ftot, 3), "traj")       # (made contiguous below: any strides)
            lift_args.mask(traj_ok, (V, ftot), "traj_ok", bare=True)
        G = lift_args.take_count(take_offset)
        if reference is not None:
            single = isinstance(reference, dict) or torch.is_tensor(reference) or (hasattr(reference, "ndim") and getattr(reference, "ndim", 0) == 1)
            _, ref_quat, ref_trans = camera_table([reference] if single else reference)
            if ref_quat.shape[0] != G:
                raise ValueError(f"reference lists {ref_quat.shape[0]} cameras, take_offset {G} takes")
            if not ((ref_quat.astype(np.float64) ** 2).sum(-1) >= 1e-12).all():
                raise ValueError("reference holds a zero quaternion")
    lift_args.need_device("align_views", poses, optional=(valid, traj, traj_ok))
    valid = valid.contiguous() if valid is not None else None
    d_off, G = _seq_table(take_offset, ftot, poses.device)
    res = _align(_lib.load(), poses, valid, d_off, G, traj.contiguous() if traj is not None else None,
                 traj_ok.contiguous() if traj_ok is not None else None, sigma, iters)
    if reference is None:
        return res
    q, t = _align_compose(res.quat.cpu().numpy(), res.trans.cpu().numpy() if res.trans is not None else None, res.ok.cpu().numpy(), ref_quat, ref_trans)
    return res._replace(quat=torch.from_numpy(q).to(poses.device), trans=torch.from_numpy(t).to(poses.device) if t is not None else None)


SYNC_MAXLAG, SHIFT_MAXM = 256, 1 << 20       # MP_LIFT_SYNC_MAXLAG, MP_LIFT_SHIFT_MAXM of include/manipose_hip.h
# defaults of sync_views: the search range and the fewest pairs of a lag in frames, the robust scale in metres (not tuned, not measured on real data)
SYNC_MAX_LAG, SYNC_MIN_OVERLAP, SYNC_SIGMA = 32, 16, 0.05
SHIFT_MODES = {"nearest": 0, "linear": 1}
# What sync_views returns: lag, contrast (G, V) float32, lag_int, used (G, V) int32, curve (G, V, 2 max_lag + 1) float32, ok (G, V) uint8
ViewSync = namedtuple("ViewSync", "lag lag_int curve contrast used ok")


def _sync(lib, poses, valid, d_off, G, max_lag, min_overlap, sigma):
    """``mp_lift_sync_views`` on poses (V, Ftot, J, C): a ViewSync of new tensors"""
    V, ftot, J, ch = (int(v) for v in poses.shape)
    dev = poses.device
    lag, contrast = torch.zeros(G, V, dtype=torch.float32, device=dev), torch.zeros(G, V, dtype=torch.float32, device=dev)
    lag_int, used = torch.zeros(G, V, dtype=torch.int32, device=dev), torch.zeros(G, V, dtype=torch.int32, device=dev)
    curve = torch.zeros(G, V, 2 * int(max_lag) + 1, dtype=torch.float32, device=dev)
    ok = torch.zeros(G, V, dtype=torch.uint8, device=dev)
    if ftot > 0:
        n = int(lib.mp_lift_sync_views_scratch_bytes(V, ftot, J))
        scratch = torch.empty(n // 8, dtype=torch.float64, device=dev)
        _launch(dev, "mp_lift_sync_views", _lib.ptr(poses), V, ftot, J, ch, _lib.ptr(valid), _lib.ptr(d_off), G, int(max_lag), int(min_overlap),
                float(sigma), _lib.ptr(lag), _lib.ptr(lag_int), _lib.ptr(curve), _lib.ptr(contrast), _lib.ptr(used), _lib.ptr(ok), _lib.ptr(scratch), n)
    return ViewSync(lag, lag_int, curve, contrast, used, ok)


def sync_views(poses, valid=None, take_offset=None, max_lag=SYNC_MAX_LAG, min_overlap=SYNC_MIN_OVERLAP, sigma=SYNC_SIGMA):
    """``mp_lift_sync_views`` on device tensors: the lag IN TIME of every view of a take against a reference view, estimated from the lifted poses
    themselves, for cameras that were not gen-locked - every other take-level operator assumes that frame f of every view shows the same instant.
    ``poses`` (V, Ftot, J, 3 | 4) float32, one pose per view and frame in that view's camera frame (channel 3 is not read); ``valid`` (V, Ftot)
    uint8 device tensor or None; ``take_offset`` (G + 1) as for ``fuse_views``.  A view's signal is the distance of every joint from the root, its
    mean over the take removed: it knows neither the camera's orientation nor the lifter's depth mirror.  Per take the lowest view with a usable
    frame is the reference; for every other view and every lag d in -``max_lag`` .. ``max_lag`` (0..256) with at least ``min_overlap`` (>= 1) pairs
    of frames the curve is the mean of e / (1 + e / sigma^2), e the mean squared difference of the two signals at frames f + d and f; ``sigma`` > 0
    in the poses' unit (inf: plain squares).  The lag is the curve's minimum (ties: the smaller |d|, then the positive lag) plus the vertex of the
    parabola through it and its neighbours, clamped to half a frame (include/manipose_hip.h has the rule; the parabola is biased by up to 0.08 frame
    on noise-free synthetic views).  The defaults are not tuned.  Frame f + lag of view v shows what frame f of the reference shows: ``shift_views``
    with these lags puts a per-view array on the reference's clock.  Returns a ``ViewSync``: ``(lag (G, V) float32, lag_int (G, V) int32: the
    minimum's lag, curve (G, V, 2 max_lag + 1) float32 (+inf: too few pairs), contrast (G, V) float32: 1 - minimum / mean of the curve, used (G, V)
    int32: the usable frames, ok (G, V) uint8: bit 0 a lag was estimated, bit 1 the minimum is interior - without it the true lag may lie outside the
    range)``, new device tensors; the reference's row is zeros with ok = 1.  Inputs are not modified; identical bits on every call.  Not measured
    on real data."""
    if not lift_args.is_int_in(max_lag, 0, SYNC_MAXLAG):
        raise ValueError(f"max_lag is the search range in frames, an integer in 0..{SYNC_MAXLAG}, got {max_lag!r}")
    if not lift_args.is_int_in(min_overlap, 1, 2 ** 31 - 1):
        raise ValueError(f"min_overlap counts the pairs of frames a lag needs, an integer >= 1, got {min_overlap!r}")
    if not lift_args.is_number(sigma) or not float(np.float32(sigma)) > 0:
        raise ValueError(f"sigma must be a number > 0 (inf: plain squares), got {sigma!r}")
    if torch.is_tensor(poses):
        lift_args.view_poses4(poses, FUSE_MAXV)
        V, ftot = int(poses.shape[0]), int(poses.shape[1])
        lift_args.mask(valid, (V, ftot), "valid")
    lift_args.need_device("sync_views", poses, optional=(valid,))
    valid = valid.contiguous() if valid is not None else None
    d_off, G = _seq_table(take_offset, ftot, poses.device)
    return _sync(_lib.load(), poses, valid, d_off, G, max_lag, min_overlap, sigma)


def _shift(lib, x, valid, d_off, G, d_lag, mode):
    """``mp_lift_shift_views`` on x (V, Ftot, ...) contiguous: (out like x, valid_out (V, Ftot) uint8), new tensors"""
    V, ftot = int(x.shape[0]), int(x.shape[1])
    M = int(x.numel()) // max(V * ftot, 1)
    out = torch.zeros_like(x)
    valid_out = torch.zeros(V, ftot, dtype=torch.uint8, device=x.device)
    if ftot > 0:
        _launch(x.device, "mp_lift_shift_views", _lib.ptr(x), V, ftot, M, _lib.ptr(valid), _lib.ptr(d_off), G, _lib.ptr(d_lag), int(mode), _lib.ptr(out),
                _lib.ptr(valid_out))
    return out, valid_out


def shift_views(x, lag, valid=None, take_offset=None, mode="linear"):
    """``mp_lift_shift_views`` on device tensors: a per-view array put on the reference view's clock.  ``x`` (V, Ftot, ...) float32, anything per
    view and frame - poses, hypotheses, keypoints, roots; ``lag`` (G, V) or, for one take, (V,): ``sync_views``' lags in frames, device tensor, host
    tensor or array (a lag that is not finite invalidates its view); ``valid`` (V, Ftot) uint8 device tensor or None; ``take_offset`` (G + 1) as for
    ``fuse_views``.  Frame f of the result shows frame p = f + lag of the view, counted inside its take: ``mode="nearest"`` copies the frame
    nearest to p, bit for bit; ``mode="linear"`` interpolates between the two frames around p in fp64 (a p that is a whole number: a copy) -
    every float of a row with the same float of the next row, so hypothesis k of a frame with hypothesis k of the next, scores included: the
    heads' identity over time is assumed, not guaranteed, and ``nearest`` avoids the question.  A frame whose source lies outside the take or is not
    valid is zeros with ``valid_out`` 0.  A lag of 0 reproduces ``x`` at the valid frames and ``valid`` exactly.  Returns ``(out like x, valid_out
    (V, Ftot) uint8)``, new device tensors.  Inputs are not modified; identical bits on every call."""
    if mode not in SHIFT_MODES:
        raise ValueError(f"mode must be nearest or linear, got {mode!r}")
    if torch.is_tensor(x):
        if x.dim() < 2 or x.dtype != torch.float32 or not 1 <= int(x.shape[0]) <= FUSE_MAXV:
            raise ValueError(f"x must be float32 (V <= {FUSE_MAXV}, Ftot, ...), got {tuple(x.shape)} {x.dtype}")
        V, ftot = int(x.shape[0]), int(x.shape[1])
        M = int(np.prod([int(s) for s in x.shape[2:]], dtype=np.int64))
        if not 1 <= M <= SHIFT_MAXM:
            raise ValueError(f"x holds {M} floats per frame: 1..{SHIFT_MAXM} expected")
        lift_args.mask(valid, (V, ftot), "valid")
        G = lift_args.take_count(take_offset)
        h_lag = lag
        if not (torch.is_tensor(lag) and lag.is_cuda):
            h = lag.detach().cpu().numpy() if torch.is_tensor(lag) else np.asarray(lag)
            h = h.reshape(1, V) if h.shape == (V,) and G == 1 else h
            if h.dtype.kind not in "fiu" or h.shape != (G, V):
                raise ValueError(f"lag must be ({G}, {V}) numbers, got shape {tuple(h.shape)} {h.dtype}")
            h_lag = np.array(h, dtype=np.float32, order="C")
        else:
            lag2 = lag.reshape(1, V) if tuple(lag.shape) == (V,) and G == 1 else lag
            lift_args.f32(lag2, (G, V), "lag")
            h_lag = lag2.contiguous()
    lift_args.need_device("shift_views", x, optional=(valid,))
    d_lag = h_lag if torch.is_tensor(h_lag) else torch.from_numpy(h_lag).to(x.device)
    d_off, G = _seq_table(take_offset, ftot, x.device)
    return _shift(_lib.load(), x.contiguous(), valid.contiguous() if valid is not None else None, d_off, G, d_lag, SHIFT_MODES[mode])


BUNDLE_MAXITERS = 8          # MP_LIFT_BUNDLE_MAXITERS of include/manipose_hip.h: Gauss-Newton steps mp_lift_bundle_views takes at most
BUNDLE_SIGMA, BUNDLE_ITERS = 0.05, 3         # defaults of bundle_views: the robust scale in normalised screen units, the steps (not tuned)
# What bundle_views returns: cameras: place_views' nested list [take][view] with the refined extrinsics; quat (G, V, 4), trans (G, V, 3), root (Ftot, 3),
# reproj (G, V, 2) float32, cost (G, 2) float64, steps, ok (G) uint8, used (G, V) int32
ViewBundle = namedtuple("ViewBundle", "cameras quat trans root reproj cost steps ok used")


def _bundle(lib, pose, root, root_ok, kp, valid, d_off, G, d_quat, d_trans, d_intr, d_fixed, d_w, distort, sigma, iters):
    """``mp_lift_bundle_views``: (quat, trans, root, reproj, cost, steps, ok, used), new tensors"""
    V, ftot, J = int(kp.shape[0]), int(kp.shape[1]), int(kp.shape[2])
    dev = pose.device
    quat, trans = d_quat.clone(), d_trans.clone()
    out_root = root.clone()
    reproj = torch.zeros(G, V, 2, dtype=torch.float32, device=dev)
    cost = torch.zeros(G, 2, dtype=torch.float64, device=dev)
    steps, ok = torch.zeros(G, dtype=torch.uint8, device=dev), torch.zeros(G, dtype=torch.uint8, device=dev)
    used = torch.zeros(G, V, dtype=torch.int32, device=dev)
    if ftot > 0:
        n = int(lib.mp_lift_bundle_views_scratch_bytes(V, ftot))
        scratch = torch.empty(n // 8, dtype=torch.float64, device=dev)
        _launch(dev, "mp_lift_bundle_views", _lib.ptr(pose), _lib.ptr(root), _lib.ptr(root_ok), _lib.ptr(kp), V, ftot, J, _lib.ptr(valid), _lib.ptr(d_off),
                G, _lib.ptr(d_quat), _lib.ptr(d_trans), _lib.ptr(d_intr), _lib.ptr(d_fixed), _lib.ptr(d_w), int(bool(distort)), float(sigma), int(iters),
                _lib.ptr(quat), _lib.ptr(trans), _lib.ptr(out_root), _lib.ptr(reproj), _lib.ptr(cost), _lib.ptr(steps), _lib.ptr(ok), _lib.ptr(used),
                _lib.ptr(scratch), n)
    return quat, trans, out_root, reproj, cost, steps, ok, used


def bundle_views(pose, root, keypoints_2d, cameras, valid=None, take_offset=None, root_ok=None, fixed=None, weights=None, distort=True,
                 sigma=BUNDLE_SIGMA, iters=BUNDLE_ITERS):
    """``mp_lift_bundle_views`` on device tensors: a take's cameras and world roots refined JOINTLY on the reprojection error - the bundle adjustment
    behind ``align_views``' closed form, in which the 2-D keypoints have no say.  ``pose`` (Ftot, J, 3) float32 as ``fuse_views`` returns it,
    ``root`` (Ftot, 3) float32 and ``root_ok`` (Ftot) uint8 or None as ``place_views`` returns them, ``keypoints_2d`` (V, Ftot, J, 2), ``cameras``,
    ``valid``, ``take_offset``, ``weights`` and ``distort`` as for ``place_views``; ``fixed`` (G, V) or, for one take, (V,): non-zero where a view's
    extrinsics are held (host table; None: the lowest view of every take that observes a frame).  Up to ``iters`` (0..8) undamped Gauss-Newton steps
    over all free cameras (6 parameters each: a left perturbation of the camera-space point, P' = exp([w]x) P + tau) and all roots, the roots
    eliminated by a Schur complement, on sum w_j rho(|res|^2) with rho(e) = e / (1 + e / sigma^2); ``sigma`` > 0 in normalised screen units (inf:
    plain least squares); a step is taken while the cost does not rise (``place_poses``' rule; include/manipose_hip.h has the rule in full).  The
    defaults are not tuned.  Returns a ``ViewBundle``: ``(cameras: the nested list with the refined extrinsics, to be passed on to place_views
    (this waits for the kernel), quat (G, V, 4), trans (G, V, 3), root (Ftot, 3), reproj (G, V, 2): every view's weighted mean reprojection error
    at the start and at the end, cost (G, 2) float64, steps (G) uint8, ok (G) uint8: 0 where the start could not be evaluated (a joint behind a
    camera), used (G, V) int32: the frames a view observes)``, new device tensors.  A fixed view, and every view of a take that took no step, is
    copied through bit for bit.  Inputs are not modified; identical bits on every call.  Not measured on real data."""
    if not lift_args.is_number(sigma) or not float(sigma) > 0:
        raise ValueError(f"sigma must be a number > 0 in normalised screen units (inf: no robust weight), got {sigma!r}")
    if not lift_args.is_int_in(iters, 0, BUNDLE_MAXITERS):
        raise ValueError(f"iters counts Gauss-Newton steps, an integer in 0..{BUNDLE_MAXITERS} (0: the evaluation alone), got {iters!r}")
    valid, d_off, G, (intr, quat, trans, present), h_w, h_fixed = _take_front("bundle_views", pose, keypoints_2d, cameras, valid, take_offset, weights,
                                                                             roots=(root, root_ok, fixed))
    dev, V = pose.device, int(keypoints_2d.shape[0])
    res = _bundle(_lib.load(), pose, root.contiguous(), root_ok.contiguous() if root_ok is not None else None, keypoints_2d.contiguous(), valid, d_off, G,
                  torch.from_numpy(quat).to(dev), torch.from_numpy(trans).to(dev), torch.from_numpy(intr).to(dev),
                  torch.from_numpy(h_fixed).to(dev) if h_fixed is not None else None, torch.from_numpy(h_w).to(dev) if h_w is not None else None,
                  distort, sigma, iters)
    q, t = res[0].cpu().numpy(), res[1].cpu().numpy()
    nested = [[np.concatenate([intr[g, v], q[g, v], t[g, v]]) if present[g, v] else None for v in range(V)] for g in range(G)]
    return ViewBundle(nested, *res)


CALIBRATE_MAXITERS = 8       # MP_LIFT_CALIBRATE_MAXITERS of include/manipose_hip.h
CALIBRATE_SIGMA, CALIBRATE_PRIOR, CALIBRATE_ITERS = 0.05, 1e-3, 3          # defaults of calibrate_views (the float64 prototype's; not tuned)
# What calibrate_views returns: cameras: the nested list [take][view] with the new intrinsics and extrinsics; quat (G, V, 4), trans (G, V, 3),
# intr (G, V, 9), points (Ftot, J, 3), reproj (G, V, 2) float32, cost (G, 2) float64, steps, ok (G) uint8, used (G, V) int32
ViewCalibration = namedtuple("ViewCalibration", "cameras quat trans intr points reproj cost steps ok used")


def _calibrate(lib, points, points_ok, kp, valid, d_off, G, d_quat, d_trans, d_intr, d_fixed, d_w, focal, distort, sigma, prior, iters):
    """``mp_lift_calibrate_views``: (quat, trans, intr, points, reproj, cost, steps, ok, used), new tensors"""
    V, ftot, J = int(kp.shape[0]), int(kp.shape[1]), int(kp.shape[2])
    dev = points.device
    quat, trans, intr = d_quat.clone(), d_trans.clone(), d_intr.clone()
    out = points.clone()
    reproj = torch.zeros(G, V, 2, dtype=torch.float32, device=dev)
    cost = torch.zeros(G, 2, dtype=torch.float64, device=dev)
    steps, ok = torch.zeros(G, dtype=torch.uint8, device=dev), torch.zeros(G, dtype=torch.uint8, device=dev)
    used = torch.zeros(G, V, dtype=torch.int32, device=dev)
    if ftot > 0:
        n = int(lib.mp_lift_calibrate_views_scratch_bytes(V, ftot, J))
        scratch = torch.empty(n // 8, dtype=torch.float64, device=dev)
        _launch(dev, "mp_lift_calibrate_views", _lib.ptr(points), _lib.ptr(points_ok), _lib.ptr(kp), V, ftot, J, _lib.ptr(valid), _lib.ptr(d_off), G,
                _lib.ptr(d_quat), _lib.ptr(d_trans), _lib.ptr(d_intr), _lib.ptr(d_fixed), _lib.ptr(d_w), int(bool(focal)), int(bool(distort)),
                float(sigma), float(prior), int(iters), _lib.ptr(quat), _lib.ptr(trans), _lib.ptr(intr), _lib.ptr(out), _lib.ptr(reproj), _lib.ptr(cost),
                _lib.ptr(steps), _lib.ptr(ok), _lib.ptr(used), _lib.ptr(scratch), n)
    return quat, trans, intr, out, reproj, cost, steps, ok, used


def calibrate_views(points, keypoints_2d, cameras, valid=None, take_offset=None, points_ok=None, fixed=None, weights=None, distort=True, focal=True,
                    sigma=CALIBRATE_SIGMA, prior=CALIBRATE_PRIOR, iters=CALIBRATE_ITERS):
    """``mp_lift_calibrate_views`` on device tensors: a take CALIBRATED on its keypoints - the full bundle adjustment behind ``bundle_views``, which
    holds the fused pose fixed and reads the focal lengths from a calibration.  ``points`` (Ftot, J, 3) float32 world points, the fused pose plus
    its root, and ``points_ok`` (Ftot) uint8 or None; ``keypoints_2d`` (V, Ftot, J, 2), ``cameras``, ``valid``, ``take_offset``, ``fixed``,
    ``weights`` and ``distort`` as for ``bundle_views``.  Every joint of every used frame is a free point, every free camera has its six pose
    parameters and, with ``focal``, every view that observes a frame - the fixed ones too - one factor g on its focal lengths (fx, fy) = g (fx0, fy0);
    up to ``iters`` (0..8) undamped Gauss-Newton steps on sum w_j rho(|res|^2) + prior sum w_j |X - start|^2, the points eliminated one by one by a
    Schur complement (include/manipose_hip.h has the rule in full).  ``sigma`` > 0 in normalised screen units (inf: plain least squares);
    ``prior`` > 0: the keypoints leave the scale of points and camera positions free, and the pull towards the start pins it.  A take needs two
    views that observe a frame (one view's poses do not decide its focal length); otherwise it is evaluated and copied through.  The defaults are
    a float64 prototype's, not tuned.  Returns a ``ViewCalibration``: ``(cameras: the nested list with the new intrinsics and extrinsics, to be
    passed on (this waits for the kernel), quat (G, V, 4), trans (G, V, 3), intr (G, V, 9), points (Ftot, J, 3), reproj (G, V, 2), cost (G, 2)
    float64, steps (G) uint8, ok (G) uint8, used (G, V) int32)``, new device tensors.  Every view of a take that took no step is copied through bit
    for bit.  Inputs are not modified; identical bits on every call.  Not measured on real data."""
    lift_args.robust_scale(sigma)
    lift_args.prior_pull(prior)
    lift_args.step_count(iters, CALIBRATE_MAXITERS)
    valid, d_off, G, (intr, quat, trans, present), h_w, h_fixed = _take_front("calibrate_views", points, keypoints_2d, cameras, valid, take_offset, weights,
                                                                             roots=(None, points_ok, fixed), ok_name="points_ok")
    dev, V = points.device, int(keypoints_2d.shape[0])
    res = _calibrate(_lib.load(), points, points_ok.contiguous() if points_ok is not None else None, keypoints_2d.contiguous(), valid, d_off, G,
                     torch.from_numpy(quat).to(dev), torch.from_numpy(trans).to(dev), torch.from_numpy(intr).to(dev),
                     torch.from_numpy(h_fixed).to(dev) if h_fixed is not None else None, torch.from_numpy(h_w).to(dev) if h_w is not None else None,
                     focal, distort, sigma, prior, iters)
    q, t, k = res[0].cpu().numpy(), res[1].cpu().numpy(), res[2].cpu().numpy()
    nested = [[np.concatenate([k[g, v], q[g, v], t[g, v]]) if present[g, v] else None for v in range(V)] for g in range(G)]
    return ViewCalibration(nested, *res)


TRIANGULATE_SIGMA, TRIANGULATE_PRIOR, TRIANGULATE_STEPS = float("inf"), 0.0, 3          # defaults of triangulate_views (not tuned)
# What triangulate_views returns: points (Ftot, J, 3), err (Ftot, J) float32, views, ok, steps (Ftot, J) uint8
ViewTriangulation = namedtuple("ViewTriangulation", "points err views ok steps")


def _triangulate(lib, pose, root, root_ok, kp, kp_weight, valid, d_off, G, d_quat, d_trans, d_intr, distort, sigma, prior, iters):
    """``mp_lift_triangulate`` on pose (Ftot, J, 3), root (Ftot, 3), kp (V, Ftot, J, 2): a ViewTriangulation of new tensors (zeros where no take
    holds a frame)"""
    V, ftot, J = int(kp.shape[0]), int(kp.shape[1]), int(kp.shape[2])
    dev = pose.device
    points = torch.zeros(ftot, J, 3, dtype=torch.float32, device=dev)
    err = torch.zeros(ftot, J, dtype=torch.float32, device=dev)
    views, ok, steps = (torch.zeros(ftot, J, dtype=torch.uint8, device=dev) for _ in range(3))
    if ftot > 0:
        _launch(dev, "mp_lift_triangulate", _lib.ptr(pose), _lib.ptr(root), _lib.ptr(root_ok), _lib.ptr(kp), _lib.ptr(kp_weight), V, ftot, J,
                _lib.ptr(valid), _lib.ptr(d_off), G, _lib.ptr(d_quat), _lib.ptr(d_trans), _lib.ptr(d_intr), int(bool(distort)), float(sigma),
                float(prior), int(iters), _lib.ptr(points), _lib.ptr(err), _lib.ptr(views), _lib.ptr(ok), _lib.ptr(steps))
    return ViewTriangulation(points, err, views, ok, steps)


def triangulate_views(pose, root, keypoints_2d, cameras, valid=None, take_offset=None, root_ok=None, kp_weight=None, distort=True,
                      sigma=TRIANGULATE_SIGMA, prior=TRIANGULATE_PRIOR, refine=TRIANGULATE_STEPS):
    """``mp_lift_triangulate`` on device tensors: every joint of a fused take TRIANGULATED on the 2-D keypoints of the cameras that see it - after
    ``fuse_views`` and ``place_views`` the keypoints decide one root per frame and the body is the mean of the views' lifted hypotheses.  ``pose``
    (Ftot, J, 3) float32 as ``fuse_views`` returns it, ``root`` (Ftot, 3) float32 and ``root_ok`` (Ftot) uint8 or None as ``place_views`` returns
    them, ``keypoints_2d`` (V, Ftot, J, 2), ``cameras``, ``valid``, ``take_offset`` and ``distort`` as for ``place_views``; ``kp_weight``
    (V, Ftot, J) float32 device tensor or None (every weight 1): a weight per observation - the detector's confidence, an occlusion mask; a
    weight that is 0, negative or not finite means "not observed".  Per joint the start is the linear pinhole triangulation over its
    observations; with fewer than two, or a degenerate system, it is the prior point pose + root.  Then up to ``refine`` (0..16) undamped
    Gauss-Newton steps on sum w rho(|res|^2) + prior |X - (pose + root)|^2 under the camera model ``distort`` names, rho(e) = e / (1 + e / sigma^2);
    ``sigma`` > 0 in normalised screen units (inf: plain least squares), ``prior`` >= 0 (0: no pull; a joint one camera sees then stays at the
    prior point); a step is taken while the cost does not rise (``place_poses``' rule; include/manipose_hip.h has the rule in full).  The
    defaults are not tuned.  Returns a ``ViewTriangulation``: ``(points (Ftot, J, 3) world positions, err (Ftot, J): the weighted mean
    reprojection distance of the joint's observations, views (Ftot, J) uint8: bit v set where view v observed the joint, ok (Ftot, J) uint8: bit 0
    a finite result, bit 1 triangulated (not started from the prior point), steps (Ftot, J) uint8)``, new device tensors; an item without a result
    is 0 with ok = 0.  Inputs are not modified; identical bits on every call.  Not measured on real data."""
    lift_args.robust_scale(sigma)
    lift_args.prior_weight(prior)
    if not lift_args.is_int_in(refine, 0, REFINE_MAXITERS):
        raise ValueError(f"refine counts Gauss-Newton steps, an integer in 0..{REFINE_MAXITERS} (0: the start alone), got {refine!r}")
    if all(torch.is_tensor(t) for t in (pose, root, keypoints_2d)):
        lift_args.take_pose_keypoints(pose, keypoints_2d, FUSE_MAXV, root)
        lift_args.keypoint_weights(kp_weight, tuple(keypoints_2d.shape[:3]))
    valid, d_off, G, (intr, quat, trans, _), _, _ = _take_front("triangulate_views", pose, keypoints_2d, cameras, valid, take_offset, None,
                                                                roots=(root, root_ok, None))
    lift_args.need_device("triangulate_views", pose, optional=(kp_weight,))
    dev = pose.device
    return _triangulate(_lib.load(), pose, root.contiguous(), root_ok.contiguous() if root_ok is not None else None, keypoints_2d.contiguous(),
                        kp_weight.contiguous() if kp_weight is not None else None, valid, d_off, G, torch.from_numpy(quat).to(dev),
                        torch.from_numpy(trans).to(dev), torch.from_numpy(intr).to(dev), distort, sigma, prior, refine)


# defaults of fit_skeleton_views (not tuned).  The pull of 1e-4 keeps a frame with an unseen limb solvable: it weighs a 1 cm move at 1e-8 against
# 4e-6 for one keypoint at noise 0.002
SKELETON_SIGMA, SKELETON_PRIOR, SKELETON_STEPS = float("inf"), 1e-4, 3
# What fit_skeleton_views returns: pose (Ftot, J, 3), err (Ftot, 2) float32, ok, steps (Ftot) uint8, lengths (G, J - 1) float32: the bone tables used
ViewSkeleton = namedtuple("ViewSkeleton", "pose err ok steps lengths")


def _fit_skeleton(lib, start, start_ok, kp, kp_weight, valid, d_off, G, d_quat, d_trans, d_intr, d_lengths, parents, distort, sigma, prior, iters):
    """``mp_lift_fit_skeleton`` on start (Ftot, J, 3), kp (V, Ftot, J, 2), lengths (G, J - 1): (pose, err, ok, steps), new tensors (zeros where no
    take holds a frame)"""
    V, ftot, J = int(kp.shape[0]), int(kp.shape[1]), int(kp.shape[2])
    dev = start.device
    pose = torch.zeros(ftot, J, 3, dtype=torch.float32, device=dev)
    err = torch.zeros(ftot, 2, dtype=torch.float32, device=dev)
    ok, steps = (torch.zeros(ftot, dtype=torch.uint8, device=dev) for _ in range(2))
    if ftot > 0:
        _launch(dev, "mp_lift_fit_skeleton", _lib.ptr(start), _lib.ptr(start_ok), _lib.ptr(kp), _lib.ptr(kp_weight), V, ftot, J, _lib.ptr(valid),
                _lib.ptr(d_off), G, _lib.ptr(d_quat), _lib.ptr(d_trans), _lib.ptr(d_intr), _lib.ptr(d_lengths), parents, int(bool(distort)), float(sigma),
                float(prior), int(iters), _lib.ptr(pose), _lib.ptr(err), _lib.ptr(ok), _lib.ptr(steps))
    return pose, err, ok, steps


# defaults of fit_skeleton_views' smoothing along time (not tuned: taken from a synthetic motion), and the entry point's bound on the sweeps
SKELETON_SMOOTH, SKELETON_SWEEPS, SKELETON_MAXSWEEPS = 0.0, 8, 64
# What fit_skeleton_views returns with smooth > 0: err is (Ftot, 3), its third column the result's; moves (Ftot) uint8: the accepted visits
ViewSkeletonSmooth = namedtuple("ViewSkeletonSmooth", "pose err ok steps lengths moves")


def _fit_skeleton_smooth(lib, start, start_ok, kp, kp_weight, valid, d_off, G, d_quat, d_trans, d_intr, d_lengths, parents, distort, sigma, prior, iters,
                         smooth, sweeps):
    """``mp_lift_fit_skeleton_smooth`` on ``_fit_skeleton``'s arguments: (pose, err (Ftot, 3), ok, steps, moves), new tensors (zeros where no take
    holds a frame)"""
    V, ftot, J = int(kp.shape[0]), int(kp.shape[1]), int(kp.shape[2])
    dev = start.device
    pose = torch.zeros(ftot, J, 3, dtype=torch.float32, device=dev)
    err = torch.zeros(ftot, 3, dtype=torch.float32, device=dev)
    ok, steps, moves = (torch.zeros(ftot, dtype=torch.uint8, device=dev) for _ in range(3))
    if ftot > 0:
        n = int(lib.mp_lift_fit_skeleton_smooth_scratch_bytes(ftot, J))
        scratch = torch.empty(n // 8, dtype=torch.float64, device=dev)
        _launch(dev, "mp_lift_fit_skeleton_smooth", _lib.ptr(start), _lib.ptr(start_ok), _lib.ptr(kp), _lib.ptr(kp_weight), V, ftot, J, _lib.ptr(valid),
                _lib.ptr(d_off), G, _lib.ptr(d_quat), _lib.ptr(d_trans), _lib.ptr(d_intr), _lib.ptr(d_lengths), parents, int(bool(distort)), float(sigma),
                float(prior), int(iters), float(smooth), int(sweeps), _lib.ptr(pose), _lib.ptr(err), _lib.ptr(ok), _lib.ptr(steps), _lib.ptr(moves),
                _lib.ptr(scratch), n)
    return pose, err, ok, steps, moves


def _median_bones(start, start_ok, d_off, G, parents):
    """(G, J - 1) float32: per take and bone the median over the take's start_ok frames of the start's bone lengths (torch's median: the lower of
    two middle values); a take without such a frame gets NaN, which mp_lift_fit_skeleton does not fit"""
    ftot, J = int(start.shape[0]), int(start.shape[1])
    par = torch.tensor(list(parents)[1:], dtype=torch.int64, device=start.device)
    bones = (start[:, 1:].double() - start[:, par].double()).norm(dim=-1)
    use = torch.isfinite(bones).all(dim=1)
    if start_ok is not None:
        use &= start_ok != 0
    off = d_off.cpu().clamp(0, ftot).tolist()
    out = torch.full((G, J - 1), float("nan"), dtype=torch.float32, device=start.device)
    for g in range(G):
        rows = bones[off[g]:max(off[g], off[g + 1])][use[off[g]:max(off[g], off[g + 1])]]
        if rows.shape[0]:
            out[g] = rows.median(dim=0).values.float()
    return out


def fit_skeleton_views(start, keypoints_2d, cameras, lengths=None, valid=None, take_offset=None, start_ok=None, kp_weight=None, skeleton=None,
                       distort=True, sigma=SKELETON_SIGMA, prior=SKELETON_PRIOR, refine=SKELETON_STEPS, smooth=SKELETON_SMOOTH, sweeps=SKELETON_SWEEPS):
    """``mp_lift_fit_skeleton`` on device tensors: ONE SKELETON fitted to a fused take's keypoints.  ``triangulate_views`` leaves a cloud of points
    per frame, with bone lengths that change from frame to frame; ``project_rigid`` makes bones constant but re-assembles the pose bone by bone,
    without asking the keypoints.  Here a frame's pose is its root and one unit direction per bone of a fixed bone table, fitted to the keypoints
    of all joints at once.  ``start`` (Ftot, J, 3) float32 WORLD joints - the triangulated points, or the fused pose plus root -, the pose to start
    from and to be pulled towards; ``start_ok`` (Ftot) uint8 or None: 0 where a frame is not to be fitted; ``keypoints_2d`` (V, Ftot, J, 2),
    ``cameras``, ``valid``, ``take_offset``, ``kp_weight`` and ``distort`` as for ``triangulate_views``; ``lengths`` (G, J - 1) or (J - 1,), tensor
    or array, in the poses' unit: one bone table per take, or None: per take and bone the median over the take's ``start_ok`` frames of the
    start's bone lengths; ``skeleton``: default the 17-joint H36M tree.  The start is made rigid as ``project_rigid`` does (each bone's direction
    kept, a bone without one taking its parent's); then up to ``refine`` (0..16) undamped Gauss-Newton steps over the root and two tangent
    coordinates per bone direction on sum w rho(|res|^2) + prior sum_j |p_j - start_j|^2, rho(e) = e / (1 + e / sigma^2); ``sigma`` > 0 in
    normalised screen units (inf: plain least squares), ``prior`` >= 0; a step is taken while the cost does not rise (``place_poses``' rule;
    include/manipose_hip.h has the rule in full).  The defaults are not tuned: the pull of 1e-4 only keeps a frame with an unseen limb solvable.
    Returns a ``ViewSkeleton``: ``(pose (Ftot, J, 3) world joints with the table's bone lengths, err (Ftot, 2): the frame's weighted mean
    reprojection distance at the rigid start and at the result, ok (Ftot) uint8: bit 0 a finite result, bit 1 every bone of the start had a
    direction of its own, steps (Ftot) uint8, lengths (G, J - 1): the tables used)``, new device tensors; a frame without a result is 0 with
    bit 0 of ok clear.  Inputs are not modified; identical bits on every call.  Not measured on real data.

    ``smooth`` > 0 fits the take ALONG TIME (``mp_lift_fit_skeleton_smooth``): after the fit above, ``sweeps`` (0..64) sweeps over the frames
    lower the frames' costs plus ``smooth`` times the squared second differences of the joint positions, a frame at a time taking one
    Gauss-Newton step with its neighbours held (the terms never cross a take's border or a frame without a result).  It then returns a
    ``ViewSkeletonSmooth``: ``err`` is (Ftot, 3), its third column the distance at the smoothed result, and ``moves (Ftot) uint8``, the accepted
    visits, follows ``lengths``.  With ``smooth=0`` (the default) the call and its result are what they are without the two arguments.
    ``smooth=0.1`` with 8 sweeps is what a synthetic motion suggested; neither is tuned."""
    lift_args.robust_scale(sigma)
    lift_args.prior_weight(prior)
    lift_args.smooth_weight(smooth)
    lift_args.sweep_count(sweeps, SKELETON_MAXSWEEPS)
    if not lift_args.is_int_in(refine, 0, REFINE_MAXITERS):
        raise ValueError(f"refine counts Gauss-Newton steps, an integer in 0..{REFINE_MAXITERS} (0: the rigid start alone), got {refine!r}")
    h_len = parents = None
    if all(torch.is_tensor(t) for t in (start, keypoints_2d)):
        _, _, J = lift_args.take_pose_keypoints(start, keypoints_2d, FUSE_MAXV)
        lift_args.keypoint_weights(kp_weight, tuple(keypoints_2d.shape[:3]))
        parents = _parents_c(_skeleton_of(skeleton=skeleton), J)
        if lengths is not None:
            G = lift_args.take_count(take_offset)
            h_len = _host_f32(lengths, (G, J - 1), "lengths", row=(J - 1,))      # (a length that is not > 0: the kernel does not fit its take)
    valid, d_off, G, (intr, quat, trans, _), _, _ = _take_front("fit_skeleton_views", start, keypoints_2d, cameras, valid, take_offset, None,
                                                                roots=(None, start_ok, None), ok_name="start_ok")
    lift_args.need_device("fit_skeleton_views", start, optional=(kp_weight,))
    dev = start.device
    start_ok = start_ok.contiguous() if start_ok is not None else None
    d_len = torch.from_numpy(h_len).to(dev) if h_len is not None else _median_bones(start, start_ok, d_off, G, parents)
    args = (_lib.load(), start, start_ok, keypoints_2d.contiguous(), kp_weight.contiguous() if kp_weight is not None else None, valid, d_off, G,
            torch.from_numpy(quat).to(dev), torch.from_numpy(trans).to(dev), torch.from_numpy(intr).to(dev), d_len, parents, distort, sigma, prior, refine)
    if float(smooth) > 0:
        pose, err, ok, steps, moves = _fit_skeleton_smooth(*args, smooth, sweeps)
        return ViewSkeletonSmooth(pose, err, ok, steps, d_len, moves)
    return ViewSkeleton(*_fit_skeleton(*args), d_len)

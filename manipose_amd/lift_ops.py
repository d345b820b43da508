"""The per-sequence operators of lifting: what one kernel of the library does to the frames of sequences laid end to end, as a public function
on device tensors (``project_rigid``, ``pose_rotations``, ``smooth_poses`` ...) and as the private launcher behind it (``_rigid``, ``_rotations``,
``_smooth`` ...), which ``lift_sequences``' stages (lifting.py) call on their own buffers.  A public function checks its arguments with lift_args'
vocabulary - the ValueErrors first, then ``need_device``'s refusal of CPU tensors (``_poses4``, for project_rigid, place_poses and to_world, refuses
before it looks at the shape, as those three always have) - uploads its tables and calls its launcher; a launcher allocates its outputs, and where
there is a frame goes through ``_launch``, the one way into the library.

Rigid lifting (``rigid=True``, off by default): the merged poses of a sequence do not share their bone lengths (averaged hypotheses, blended
windows, one length prediction per window), so after the merge every sequence gets ONE table of J - 1 bone lengths - the model's own
(``"model"``), the mean lengths of the merged poses (``"measured"``, ``mp_bone_length_means``) or the caller's - and ``mp_lift_rigid``
re-assembles every emitted pose and hypothesis along its own bone directions with them (include/manipose_hip.h has the definition).

Placing (``place`` / ``frame="world"`` / ``floor``, all off by default): the merged poses are root-relative and in the camera's frame.  With
the sequences' cameras (``camera_table``) ``mp_lift_place`` fits, per pose and per hypothesis, the root translation whose pinhole projection meets
the 2-D keypoints the pose was lifted from, and reports the reprojection error under the full H36M camera model; ``mp_lift_world`` rotates
everything into the world frame (the reference's ``camera_to_world``, hpe/viz.py:93-98) and, with ``floor``, puts the sequence on z = 0.

Refining the placement (``place_refine``, Gauss-Newton steps, 0 = off, the default): the fit above uses the pinhole part of the camera only, because
that fit is linear in the translation, while the H36M cameras distort (k1 ~ -0.2, k2 ~ 0.25): on noise-free keypoints made with the full model the
linear fit misses the true root by up to 0.17 m, almost all of it depth.  ``mp_lift_place_refine`` starts from the linear fit and takes up to
``place_refine`` undamped Gauss-Newton steps on the squared reprojection error of the FULL projection (include/manipose_hip.h has the rule); three
steps recover the translation of that construction to the float32 rounding of its keypoints.  The same entry point with zero steps and a given
trajectory is ``reproject_poses``.  What this does to accuracy on real H36M data has not been measured (no dataset here).

Joint rotations (``rotations``, off by default): every stage here emits joint POSITIONS, while the model decodes (6-D rotation per joint, segment
lengths) by forward kinematics.  ``mp_lift_rotations`` is the inverse on the poses as they are emitted: per pose the root orientation from the
frame the hip and the spine span, per joint the shortest-arc (twist-free) rotation that turns the bone's T-pose direction into its measured one
(include/manipose_hip.h has the rule), as unit quaternions (w, x, y, z) that are sign-continuous along every sequence, and as the 6-D form the
decoder takes.  ``pose_rotations`` is the public form.  No accuracy of these rotations on real data has been measured (no dataset here).

Smoothing in time (``smooth_poses`` / ``smooth_traj``, radii, 0 = off, the default): every stage above treats every frame on its own.
``mp_lift_smooth`` fits, per frame and coordinate, a polynomial of degree ``smooth_degree`` to the frames within the radius that belong to the same
sequence and are valid (Savitzky-Golay with validity weights; include/manipose_hip.h has the rule) and stores its value at the frame.  The merged
poses and the hypotheses are smoothed BEFORE the rigid stage (bone lengths stay constant, and placing fits the trajectory to the poses that are
emitted); the fitted root trajectories AFTER ``mp_lift_place`` and before ``mp_lift_world``, with the fit's ``ok`` as validity, so a frame whose fit
was degenerate is filled from its neighbours.  Whether this lowers MPJPE / MPJVE on real data has not been measured (no dataset here).

One hypothesis path (``agg="path"``): ``weighted_ave`` averages K poses that share their bone lengths but differ in rotation (the result lies off
the manifold the model stays on), and ``best_score`` keeps a real hypothesis in every frame but chooses each frame on its own, so the sequence jumps
from head to head whenever two scores cross.  ``mp_lift_path`` emits exactly one of the model's own hypotheses per frame, chosen jointly over the
whole sequence: the most probable path of a hidden Markov model whose states are the hypotheses (unary cost -log score, transition cost the mean
squared joint step over 2 sigma^2 plus a cost per switch), found with the Viterbi algorithm (include/manipose_hip.h has the rule).  It runs right
after the merge, on the hypotheses of the un-mirrored pass, and every later stage starts from the selected poses.  Whether it lowers MPJPE / MPJVE
on real data has not been measured (no dataset here), and the default sigma is not tuned.

Scoring (``targets`` / ``return_score``, off by default): ``mp_lift_score`` holds what the stages emit against the dataset's 3-D sequences, per
sequence and on the device - MPJPE, P-MPJPE, velocity and acceleration errors, per-joint errors, bone-length statistics, and the trajectory's error
with ``place`` (include/manipose_hip.h has the rule; ``score_poses`` / ``score_traj`` are the stand-alone forms).  It is the instrument for the
sentences above that say "has not been measured"; no number is claimed here.

Standing a sequence on its floor (``estimate_ground``, off everywhere by default): placing and the world frame read which way is up from a calibration.
``mp_lift_ground`` takes it from the motion: a foot that stands still is standing on something, the contact points of a sequence span its floor, and the
plane through them - robustly, the body's mean axis a weak prior - gives the rotation and shift ``to_world`` applies, each foot's height over the plane and
the foot skate, how far the feet slide while in contact (include/manipose_hip.h has the rule).  It reads ABSOLUTE positions (poses plus trajectory) in any
rigid frame and moves nothing.  The defaults are untuned and nothing has been measured on real data (no dataset here).

Pinning the feet (``lock_feet``, off everywhere by default): ``mp_lift_footlock`` removes the slide the ground estimate measures.  A foot in a stance run
is pinned to the mean of its ankle positions (on the estimated floor where a ``Ground`` is handed over), the swing frames around a run are eased into
and out of the pin, and each leg is re-posed by analytic two-bone IK with the frame's own bone lengths; hips and the rest of the body keep their bits
(include/manipose_hip.h has the rule).  The defaults are untuned and nothing has been measured on real data (no dataset here).

Retiming on the rotations (``retime_rotations`` / ``smooth_rotations`` / ``pose_from_rotations``, off everywhere by default): with ``rotations`` the
product is the triple (root trajectory, quat, bones), and every operator above that works along time works on joint positions, where averaging or
interpolating shortens the bones.  ``mp_lift_retime`` resamples the triple at any frame rate, or smooths it at its own, on SO(3) - the short-way slerp
of the two frames around a sample, or ``mp_lift_smooth``'s local polynomial in the tangent space of the nearest valid frame - and ``mp_lift_fk``, the
inverse of ``mp_lift_rotations``, turns it back into positions on exactly the take's bone table (include/manipose_hip.h has both rules).  The defaults
are untuned and nothing has been measured on real data (no dataset here).

Export (``euler_from_rotations``, off everywhere by default): ``mp_lift_euler`` turns the triple's rotations into Euler channels in degrees, in any
of the six channel orders, re-expressed by a rigid transform per sequence (the estimated floor, an up-axis turn) and made continuous in time; with
the bone-centred hierarchy of ``manipose_amd.bvh`` (every bone a node at its parent joint that carries exactly q[j]) they are a BVH file whose joint
positions are ``pose_from_rotations``' (include/manipose_hip.h has the rule).  Nothing has been measured on real data (no dataset here).
"""
from __future__ import annotations

import ctypes as C
from collections import namedtuple

import numpy as np
import torch

from . import _lib
from . import lift_args

TAPER = {"uniform": 0, "biweight": 1}
SMOOTH_MAXR = 64             # MP_LIFT_SMOOTH_MAXR of include/manipose_hip.h
PATH_MAXK = 8                # hypotheses mp_lift_path takes
PATH_SIGMA, PATH_SWITCH = 0.02, 0.0      # defaults of agg="path": the step's standard deviation in metres (not tuned), the cost of a switch


def _launch(dev, name, *call):
    """The one way into the library: entry point ``name`` on ``call`` and, last, the current stream of ``dev``; its status is checked under its name.
    (Every launcher keeps its leading ``lib`` argument, though only those that size a scratch buffer read it: the tests' and the bench's call
    lines stay as they are.)"""
    with torch.cuda.device(dev):
        _lib.check(getattr(_lib.load(), name)(*call, _lib.stream_ptr()), name)


def _skeleton_of(model=None, skeleton=None):
    """``skeleton`` if given, else the model's own, else the 17-joint H36M tree (MixSTE carries none)"""
    from .data import h36m_skeleton
    if skeleton is not None:
        return skeleton
    return model.decoder.skeleton if model is not None and hasattr(model, "decoder") else h36m_skeleton()


def _parents_c(sk, J):
    par = [int(p) for p in sk.parents]
    if par[0] != -1 or any(not 0 <= p < j for j, p in enumerate(par) if j):
        raise ValueError("rigid lifting: joint 0 must be the root and parents must precede their children")
    if len(par) != J:
        raise ValueError(f"{J} joints, but the skeleton has {len(par)}")
    return (C.c_int32 * J)(*par)


def _host_f32(a, shape, what, row=None, nonneg=False):
    """A per-sequence table (tensor or array) as float32 numpy of ``shape``, after its dtype, shape and finiteness were checked on the host; a
    copy: the caller's table is never aliased.  A table of shape ``row`` is one row for every sequence; ``nonneg`` also refuses negative entries."""
    h = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    got = h.shape
    if row is not None and h.shape == row:
        h = np.broadcast_to(h, shape)
    if h.dtype.kind not in "fiu" or h.shape != shape:
        raise ValueError(f"{what} must be {shape}{'' if row is None else f' or {row}'} numbers, got shape {tuple(got)} {h.dtype}")
    h = np.array(h, dtype=np.float32, order="C")
    if not np.isfinite(h).all() or (nonneg and (h < 0).any()):
        raise ValueError(f"{what} must be finite{' and non-negative' if nonneg else ''}")
    return h


def _device_f32(a, dev, shape, what, row=None, nonneg=False):
    return torch.from_numpy(_host_f32(a, shape, what, row, nonneg)).to(dev)


def _device_i64(a, dev):
    if torch.is_tensor(a):
        return a.to(dev, torch.int64).contiguous()
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).to(dev)


def _seq_table(seq_offset, ntot, dev):
    d_off = _device_i64(seq_offset if seq_offset is not None else [0, ntot], dev)
    if d_off.dim() != 1 or d_off.numel() < 2:
        raise ValueError("seq_offset must hold S + 1 >= 2 frame numbers")
    return d_off, int(d_off.numel()) - 1


def _poses4(poses, who):
    """the 4-D view of device poses; for the functions that refuse a CPU tensor before they look at its shape"""
    lift_args.need_device(who, poses)
    return lift_args.poses4(poses)


def _rigid(lib, poses4, d_off, S, d_lengths, parents):
    ntot, inner, J, ch = (int(v) for v in poses4.shape)
    _launch(poses4.device, "mp_lift_rigid", _lib.ptr(poses4), ntot, inner, J, ch, _lib.ptr(d_off), S, _lib.ptr(d_lengths), parents)


def bone_length_means(poses, seq_offset=None, real_frames=None, skeleton=None):
    """``mp_bone_length_means``: (S, J - 1) mean bone lengths per sequence of the device tensor poses (Ntot, J, 3); ``seq_offset`` (S + 1) HOST
    table or device int64 tensor (default: one sequence); ``real_frames`` (S) or None: only the first that many frames of a sequence count."""
    if poses.dim() != 3 or poses.shape[2] != 3 or poses.dtype != torch.float32:
        raise ValueError(f"poses must be float32 (Ntot, J, 3), got {tuple(poses.shape)} {poses.dtype}")
    dev, J = poses.device, int(poses.shape[1])
    parents = _parents_c(_skeleton_of(skeleton=skeleton), J)
    d_off, S = _seq_table(seq_offset, int(poses.shape[0]), dev)
    d_real = _device_i64(real_frames, dev) if real_frames is not None else None
    if d_real is not None and int(d_real.numel()) != S:
        raise ValueError(f"real_frames must have {S} entries")
    out = torch.empty(S, J - 1, dtype=torch.float32, device=dev)
    _launch(dev, "mp_bone_length_means", _lib.ptr(poses), int(poses.shape[0]), J, _lib.ptr(d_off), _lib.ptr(d_real), S, parents, _lib.ptr(out))
    return out


def project_rigid(poses, lengths, seq_offset=None, skeleton=None):
    """``mp_lift_rigid`` on a device tensor, IN PLACE (and returned): poses (Ntot, J, 3), or (Ntot, inner, J, C) with C = 3 or 4 (channel 3, a
    hypothesis' score, is left alone).  Every pose keeps its root and its bone directions and gets the bone lengths of its sequence:
    ``lengths`` (S, J - 1) or (J - 1,), tensor or array, in the unit of the poses; ``seq_offset`` (S + 1): first frame of every sequence, HOST
    table or device int64 tensor (default: all frames are one sequence).  A bone of length zero takes its parent bone's direction, (0, 0, 1)
    under the root.  ``skeleton``: default the 17-joint H36M tree."""
    p4 = _poses4(poses, "project_rigid")
    ntot, J = int(p4.shape[0]), int(p4.shape[2])
    parents = _parents_c(_skeleton_of(skeleton=skeleton), J)
    d_off, S = _seq_table(seq_offset, ntot, poses.device)
    table = _device_f32(lengths, poses.device, (S, J - 1), "lengths", row=(J - 1,), nonneg=True)
    if ntot > 0:
        _rigid(_lib.load(), p4, d_off, S, table, parents)
    return poses


ROT_CONTINUOUS = 1           # MP_LIFT_ROT_CONTINUOUS of include/manipose_hip.h


def _rest_c(sk, J):
    """The (J, 3) T-pose directions of a skeleton's ``t_pose_operators`` (joint -> direction of the bone parent -> joint; the root has none) as a C
    float table, row 0 zero; ValueError for a missing, non-finite or zero direction (the entry point normalises them)"""
    ops = getattr(sk, "t_pose_operators", None)
    if ops is None:
        raise ValueError("joint rotations need the skeleton's t_pose_operators: the T-pose direction of every bone")
    rest = np.zeros((J, 3), dtype=np.float32)
    for j in range(1, J):
        try:
            v = ops[j]
        except (KeyError, IndexError):
            raise ValueError(f"t_pose_operators has no direction for joint {j}") from None
        v = v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)
        if v.shape != (3,) or v.dtype.kind not in "fiu":
            raise ValueError(f"t_pose_operators[{j}] must be 3 numbers, got shape {tuple(v.shape)} {v.dtype}")
        with np.errstate(over="ignore"):
            v = v.astype(np.float32)
        if not np.isfinite(v).all() or not (v != 0).any():
            raise ValueError(f"t_pose_operators[{j}] = {v.tolist()}: a T-pose direction must be finite and not zero")
        rest[j] = v
    return (C.c_float * (3 * J))(*rest.ravel().tolist())


def _rotations(lib, p4, d_off, S, parents, rest, continuous=True, want_rot6d=False):
    """``mp_lift_rotations`` on p4 (Ntot, inner, J, C): (quat (Ntot, inner, J, 4), ok (Ntot, inner) uint8, rot6d (Ntot, inner, J, 6) or None), new
    tensors; p4 is read only"""
    ntot, inner, J, ch = (int(v) for v in p4.shape)
    dev = p4.device
    quat = torch.empty(ntot, inner, J, 4, dtype=torch.float32, device=dev)
    ok = torch.empty(ntot, inner, dtype=torch.uint8, device=dev)
    rot6d = torch.empty(ntot, inner, J, 6, dtype=torch.float32, device=dev) if want_rot6d else None
    if ntot > 0:
        _launch(dev, "mp_lift_rotations", _lib.ptr(p4), ntot, inner, J, ch, _lib.ptr(d_off), S, parents, rest, ROT_CONTINUOUS if continuous else 0,
                _lib.ptr(quat), _lib.ptr(rot6d), _lib.ptr(ok))
    return quat, ok, rot6d


def pose_rotations(poses, seq_offset=None, skeleton=None, continuous=True, return_rot6d=False):
    """``mp_lift_rotations`` on a device tensor, OUT of place: the joint rotations that, with each pose's own bone lengths and root position, ARE the
    pose under the decoder's forward kinematics (Rw[0] = R[0], Rw[j] = Rw[parent] R[j], p[j] = p[parent] + Rw[j] (len_j rest_j)).  ``poses``
    (Ntot, J, 3) or (Ntot, inner, J, 3 | 4) float32 (channel 3, a hypothesis' score, is not read); ``skeleton``: anything with ``parents`` and
    ``t_pose_operators`` (default, for J = 17 only: the H36M tree); ``seq_offset`` (S + 1): first frame of every sequence, HOST table or device
    int64 tensor (default: one sequence), used by ``continuous`` alone.  Returns ``(quat, ok)`` and with ``return_rot6d`` also ``rot6d``: quat
    (Ntot[, inner], J, 4) float32 unit quaternions (w, x, y, z), quat[:, 0] the root's orientation (the frame of the bones to its first child and to
    its first child in another direction - H36M: right hip and spine - against the T-pose's), quat[:, j] the shortest-arc rotation of bone j in
    its parent's frame: the twist about a bone is zero by construction, a convention and not a measurement.  ok (Ntot[, inner]) uint8: 0 where a
    bone has no direction (length 0, a non-finite coordinate: identity; any non-finite coordinate makes the whole pose identities), lies exactly
    opposite its T-pose direction (a half turn about a fixed axis) or the root's two bones are collinear.  rot6d (Ntot[, inner], J, 6): columns 0
    then 1 of each quaternion's matrix, what ``torch.ops.manipose.fk_decode`` / ``mp_fk_decode_fwd`` take.  A quaternion's sign is the one that
    makes its first non-zero component positive; with ``continuous`` it is then flipped along every (sequence, inner index, joint) track wherever
    that keeps consecutive frames in one hemisphere (dot >= 0), so the track can be filtered or interpolated; rot6d does not depend on the sign.
    fp64 inside, identical bits on every call (include/manipose_hip.h has the rule)."""
    if torch.is_tensor(poses):
        lift_args.poses4(poses)
        J = int(poses.shape[-2])
        if skeleton is None and J != 17:
            raise ValueError(f"poses have {J} joints: the default skeleton is the 17-joint H36M tree; pass a skeleton with parents and t_pose_operators")
        sk = _skeleton_of(skeleton=skeleton)
        parents, rest = _parents_c(sk, J), _rest_c(sk, J)
    p4 = _poses4(poses, "pose_rotations")
    d_off, S = _seq_table(seq_offset, int(p4.shape[0]), poses.device)
    quat, ok, rot6d = _rotations(_lib.load(), p4, d_off, S, parents, rest, bool(continuous), bool(return_rot6d))
    res = (quat, ok, rot6d) if return_rot6d else (quat, ok)
    return tuple(r[:, 0] for r in res) if poses.dim() == 3 else res


def _smooth_options(radius, degree, taper):
    if not lift_args.is_int_in(radius, 1, SMOOTH_MAXR):
        raise ValueError(f"radius must be an integer in 1..{SMOOTH_MAXR}, got {radius!r}")
    if not lift_args.is_int_in(degree, 0, 2):
        raise ValueError(f"degree must be 0, 1 or 2, got {degree!r}")
    if taper not in TAPER:
        raise ValueError(f"taper must be one of {sorted(TAPER)}, got {taper!r}")


def _smooth(lib, x4, valid, d_off, S, radius, degree, taper, want_filled=False):
    """``mp_lift_smooth`` on x4 (Ntot, inner, M, C) with valid (Ntot, inner) uint8 or None: (a new tensor, filled (Ntot, inner) uint8 or None)"""
    ntot, inner, M, ch = (int(v) for v in x4.shape)
    out = torch.empty_like(x4)
    filled = torch.empty(ntot, inner, dtype=torch.uint8, device=x4.device) if want_filled else None
    if ntot > 0:
        _launch(x4.device, "mp_lift_smooth", _lib.ptr(x4), _lib.ptr(out), ntot, inner, M, ch, _lib.ptr(valid), _lib.ptr(d_off), S, int(radius), int(degree),
                TAPER[taper], _lib.ptr(filled))
    return out, filled


def smooth_poses(poses, seq_offset=None, radius=4, degree=2, taper="uniform"):
    """``mp_lift_smooth`` on a device tensor, OUT of place: poses (Ntot, J, 3) or (Ntot, inner, J, 3 | 4) float32 (channel 3, a hypothesis' score,
    is copied) -> a new tensor of the same shape in which every coordinate of frame g is p(0) of the polynomial p of degree ``degree`` (0..2)
    fitted by least squares to the frames g - radius .. g + radius of the same sequence (radius 1..64; at the ends of a sequence the window is
    shorter, never padded, and the degree falls to the number of frames - 1), in the variable (frame - g) / radius.  ``taper``: "uniform"
    (all taps weigh 1: the classical Savitzky-Golay filter) or "biweight" ((1 - (tau / (radius + 1))^2)^2).  ``seq_offset`` (S + 1): first frame
    of every sequence, HOST table or device int64 tensor (default: one sequence).  Every frame counts as valid; fp64 inside, identical bits on
    every call."""
    _smooth_options(radius, degree, taper)
    if torch.is_tensor(poses):
        lift_args.poses4(poses)                          # (the ValueErrors come before the refusal of a CPU tensor)
    p4 = _poses4(poses, "smooth_poses")
    d_off, S = _seq_table(seq_offset, int(p4.shape[0]), poses.device)
    return _smooth(_lib.load(), p4, None, d_off, S, radius, degree, taper)[0].view(poses.shape)


def smooth_traj(traj, ok=None, seq_offset=None, radius=4, degree=2, taper="uniform"):
    """``mp_lift_smooth`` on root trajectories, OUT of place: traj (Ntot, 3) or (Ntot, inner, 3) float32 device tensor as ``place_poses`` returns it,
    ``ok`` uint8 of shape (Ntot[, inner]) or None (every frame is valid): a frame with ok = 0 does not enter any fit, and gets the value the fit
    through its valid neighbours has at it - constant where valid frames lie on one side only.  Returns ``(smoothed, filled)``: filled uint8
    (Ntot[, inner]) is 0 where no frame within the radius in the same sequence is valid; such a frame keeps its input bits.  The other arguments
    as for ``smooth_poses``."""
    _smooth_options(radius, degree, taper)
    if torch.is_tensor(traj):
        lift_args.traj3(traj)
        lift_args.mask(ok, traj.shape[:-1], "ok")
    lift_args.need_device("smooth_traj", traj, optional=(ok,))
    ntot = int(traj.shape[0])
    d_off, S = _seq_table(seq_offset, ntot, traj.device)
    out, filled = _smooth(_lib.load(), traj.view(ntot, -1, 1, 3), None if ok is None else ok.contiguous().view(ntot, -1), d_off, S, radius, degree,
                          taper, want_filled=True)
    return out.view(traj.shape), filled.view(traj.shape[:-1])


def _path(lib, hyps, d_off, S, sigma, switch_cost):
    """``mp_lift_path`` on hyps (Ntot, K, J, 4): (poses (Ntot, J, 3), path (Ntot,) uint8, cost (S,) float64), new tensors"""
    ntot, K, J, _ = (int(v) for v in hyps.shape)
    dev = hyps.device
    out = torch.empty(ntot, J, 3, dtype=torch.float32, device=dev)
    path = torch.empty(ntot, dtype=torch.uint8, device=dev)
    cost = torch.zeros(S, dtype=torch.float64, device=dev)
    if ntot > 0:
        n = int(lib.mp_lift_path_scratch_floats(ntot, K))
        scratch = torch.empty(n, dtype=torch.float32, device=dev)
        _launch(dev, "mp_lift_path", _lib.ptr(hyps), ntot, K, J, _lib.ptr(d_off), S, float(sigma), float(switch_cost), _lib.ptr(path), _lib.ptr(out),
                _lib.ptr(cost), _lib.ptr(scratch), n)
    return out, path, cost


def select_path(hyps, seq_offset=None, sigma=PATH_SIGMA, switch_cost=PATH_SWITCH):
    """``mp_lift_path`` on a device tensor: hyps (Ntot, K, J, 4) float32 as ``lift_sequences(return_hyps=True)`` returns them (xyz, and the
    hypothesis' score in channel 3), K in 1..8 -> ``(poses (Ntot, J, 3), path (Ntot,) uint8, cost (S,) float64)``, new device tensors: per frame
    exactly one hypothesis, poses[g] = hyps[g, path[g], :, :3] bit for bit, the path being the cheapest one through the sequence under the unary cost
    -log(score) (a score that is not > 1e-12 counts as 1e-12) and, from hypothesis a of a frame to hypothesis b of the next, the transition cost
    mean_j |x_b[j] - x_a[j]|^2 / (2 sigma^2) + (switch_cost if a != b): the maximum a posteriori path of that hidden Markov model, by the Viterbi
    algorithm in fp64, ties to the lowest index.  ``sigma`` > 0 in the unit of the hypotheses (inf: steps cost nothing, and with switch_cost = 0 the
    path is the best score of every frame); ``switch_cost`` >= 0.  ``seq_offset`` (S + 1): first frame of every sequence, HOST table or device int64
    tensor (default: one sequence); a path never crosses a sequence boundary, and a frame that no sequence of the table holds is left unwritten.  ``cost``: the cost of each sequence's path.  hyps is not modified;
    identical bits on every call."""
    lift_args.sigma_pair(sigma, switch_cost, ("sigma", "switch_cost"))
    if torch.is_tensor(hyps):
        lift_args.hyps4(hyps, PATH_MAXK)                 # (the ValueErrors come before the refusal of a CPU tensor)
    lift_args.need_device("select_path", hyps)
    d_off, S = _seq_table(seq_offset, int(hyps.shape[0]), hyps.device)
    return _path(_lib.load(), hyps, d_off, S, sigma, switch_cost)


SCORE_SHARES = 32            # MP_LIFT_SCORE_SHARES of include/manipose_hip.h: partial rows per (sequence, inner) in mp_lift_score's scratch
SCORE_ROOT_RELATIVE, SCORE_PROCRUSTES = 1, 2     # mp_lift_score's flags
# What score_poses returns: device float64 tensors of shape (S,), or (S, inner) for 4-D poses; per_joint (.., M); bone_* (.., M - 1) or None without a
# skeleton; rows: mp_lift_score's raw sums (.., 9 + M + 3 (M - 1)); frame_err (Ntot[, inner]) float32 with return_frames, else None
PoseScore = namedtuple("PoseScore", "frames mpjpe rmse mpjve accel p_mpjpe per_joint bone_mean bone_std bone_err rows frame_err")
# What score_traj returns: (S,) or (S, inner) device float64 tensors
TrajScore = namedtuple("TrajScore", "frames ate rmse velocity accel")


def _score(lib, p4, gt, valid, d_off, S, parents, pred_scale, gt_scale, flags, want_frames=False):
    """``mp_lift_score`` on p4 (Ntot, inner, M, C) against gt (Ntot, M, 3), valid (Ntot, inner) uint8 or None: (rows (S, inner, R) float64, frame_err
    (Ntot, inner) float32 or None), new tensors.  A frame that no sequence holds keeps frame_err = -1."""
    ntot, inner, M, ch = (int(v) for v in p4.shape)
    dev = p4.device
    rows = torch.zeros(S, inner, 6 + 4 * M, dtype=torch.float64, device=dev)
    frame_err = torch.full((ntot, inner), -1.0, dtype=torch.float32, device=dev) if want_frames else None
    if ntot > 0:
        n = int(lib.mp_lift_score_scratch_doubles(S, inner, M))
        scratch = torch.empty(n, dtype=torch.float64, device=dev)
        _launch(dev, "mp_lift_score", _lib.ptr(p4), ntot, inner, M, ch, _lib.ptr(gt), _lib.ptr(valid), _lib.ptr(d_off), S, parents, float(pred_scale),
                float(gt_scale), int(flags), _lib.ptr(rows), _lib.ptr(frame_err), _lib.ptr(scratch), n)
    return rows, frame_err


def _ratio(num, den):
    """num / den in float64, NaN where the count den is 0"""
    return torch.where(den > 0, num / den.clamp(min=1.0), torch.full_like(num, float("nan")))


def _pose_record(rows, M, procrustes, bones, frame_err=None):
    """mp_lift_score's rows (.., R) as a PoseScore"""
    n, nm = rows[..., 0], rows[..., 0] * M
    bone_mean = bone_std = bone_err = None
    if bones:
        b = rows[..., 9 + M:].reshape(*rows.shape[:-1], M - 1, 3)
        cnt = n.unsqueeze(-1).expand(b.shape[:-1])
        bone_mean, bone_err = _ratio(b[..., 0], cnt), _ratio(b[..., 2], cnt)
        bone_std = torch.sqrt((_ratio(b[..., 1], cnt) - bone_mean * bone_mean).clamp(min=0.0))      # (NaN stays NaN under clamp)
    p = _ratio(rows[..., 7], (n - rows[..., 8]) * M) if procrustes else torch.full_like(n, float("nan"))
    return PoseScore(n, _ratio(rows[..., 1], nm), torch.sqrt(_ratio(rows[..., 2], nm)), _ratio(rows[..., 4], rows[..., 3] * M),
                     _ratio(rows[..., 6], rows[..., 5] * M), p, _ratio(rows[..., 9:9 + M], n.unsqueeze(-1).expand(*n.shape, M)), bone_mean, bone_std,
                     bone_err, rows, frame_err)


def score_poses(poses, target, seq_offset=None, valid=None, skeleton=None, root_relative=False, procrustes=True, pose_scale=1.0, target_scale=1.0,
                return_frames=False):
    """``mp_lift_score`` on device tensors: lifted poses against ground truth, per sequence.  ``poses`` (Ntot, J, 3) or (Ntot, inner, J, 3 | 4) float32
    (channel 3, a hypothesis' score, is not read); ``target`` (Ntot, J, 3) float32, shared by the ``inner`` poses of a frame; ``seq_offset`` (S + 1):
    first frame of every sequence, HOST table or device int64 tensor (default: one sequence); ``valid`` uint8 (Ntot[, inner]) or None (every frame is
    valid).  With P = pose_scale * poses and G = target_scale * target in fp64 (``root_relative``: joint 0 of the same pose subtracted from both), a
    frame is COUNTED if it is valid and all its coordinates of P and G are finite, and e[g][j] = |P[g][j] - G[g][j]|.  Returns a ``PoseScore`` of
    device float64 tensors of shape (S,) - (S, inner) for 4-D poses: ``frames`` counted; ``mpjpe`` the mean of e; ``rmse`` the root of the mean of
    e^2; ``mpjve`` the mean over the pairs of consecutive counted frames of |(P[g] - P[g-1]) - (G[g] - G[g-1])|; ``accel`` the same of the second
    differences over triples; ``p_mpjpe`` (``procrustes``, needs J >= 3; NaN without it) the mean of e after the similarity alignment of every P[g]
    onto G[g], the reference's p_mpjpe, over the counted frames whose centred poses are not single points; ``per_joint`` (.., J); ``bone_mean``,
    ``bone_std`` (population standard deviation over the frames) and ``bone_err`` (mean |target's length - pose's length|), each (.., J - 1), of
    the bones of ``skeleton`` (default: the 17-joint H36M tree for 17 joints, else None: no bone statistics); ``rows``: the kernel's raw sums
    (include/manipose_hip.h has the slots); ``frame_err`` (Ntot[, inner]) float32 with ``return_frames``: the mean of e over the joints, -1 for a
    frame that is not counted or that no sequence holds.  A ratio whose count is 0 is NaN.  No term crosses a sequence boundary; fp64 inside,
    identical bits on every call."""
    if not all(lift_args.is_number(v) and np.isfinite(float(v)) and float(v) > 0 for v in (pose_scale, target_scale)):
        raise ValueError(f"pose_scale and target_scale must be finite numbers > 0, got {pose_scale!r}, {target_scale!r}")
    parents = None
    if torch.is_tensor(poses):
        p4 = lift_args.poses4(poses)                     # (the ValueErrors come before the refusal of a CPU tensor)
        ntot, inner, J = int(p4.shape[0]), int(p4.shape[1]), int(p4.shape[2])
        lift_args.f32(target, (ntot, J, 3), "target", contiguous=True)
        lift_args.mask(valid, poses.shape[:-2], "valid")
        if procrustes and J < 3:
            raise ValueError(f"procrustes=True aligns poses of at least 3 joints, got {J}")
        if skeleton is not None or J == 17:
            parents = _parents_c(_skeleton_of(skeleton=skeleton), J)
    lift_args.need_device("score_poses", poses, target, optional=(valid,))
    d_off, S = _seq_table(seq_offset, ntot, poses.device)
    flags = (SCORE_ROOT_RELATIVE if root_relative else 0) | (SCORE_PROCRUSTES if procrustes else 0)
    rows, fe = _score(_lib.load(), p4, target, None if valid is None else valid.contiguous().view(ntot, inner), d_off, S, parents, pose_scale,
                      target_scale, flags, return_frames)
    if poses.dim() == 3:
        rows, fe = rows[:, 0], (fe[:, 0] if fe is not None else None)
    return _pose_record(rows, J, bool(procrustes), parents is not None, fe)


def score_traj(traj, target, ok=None, seq_offset=None):
    """``mp_lift_score`` on root trajectories (its M = 1 form: no alignment, no bones): ``traj`` (Ntot, 3) or (Ntot, inner, 3) float32 device tensor
    as ``place_poses`` returns it, ``target`` (Ntot, 3) float32 in the same unit, ``ok`` uint8 (Ntot[, inner]) or None: a frame with ok = 0 or a
    non-finite coordinate is not counted.  Returns a ``TrajScore`` of device float64 tensors (S,) or (S, inner): ``frames`` counted, ``ate`` the mean
    distance, ``rmse`` the root of the mean squared distance, ``velocity`` / ``accel`` the mean norms of the first / second differences of the error
    over consecutive counted frames of one sequence.  A ratio whose count is 0 is NaN.  ``seq_offset`` as for ``score_poses``."""
    if torch.is_tensor(traj):
        lift_args.traj3(traj)
        lift_args.f32(target, (int(traj.shape[0]), 3), "target", contiguous=True)
        lift_args.mask(ok, traj.shape[:-1], "ok")
    lift_args.need_device("score_traj", traj, target, optional=(ok,))
    ntot = int(traj.shape[0])
    d_off, S = _seq_table(seq_offset, ntot, traj.device)
    rows = _score(_lib.load(), traj.view(ntot, -1, 1, 3), target.view(ntot, 1, 3), None if ok is None else ok.contiguous().view(ntot, -1), d_off, S, None,
                  1.0, 1.0, 0)[0]
    return _traj_record(rows[:, 0] if traj.dim() == 2 else rows)


def _traj_record(rows):
    n = rows[..., 0]
    return TrajScore(n, _ratio(rows[..., 1], n), torch.sqrt(_ratio(rows[..., 2], n)), _ratio(rows[..., 4], rows[..., 3]), _ratio(rows[..., 6], rows[..., 5]))


GROUND_MAXFEET, GROUND_MAXRADIUS, GROUND_MAXITERS = 4, 8, 8      # MP_LIFT_GROUND_* of include/manipose_hip.h
# What estimate_ground returns, device tensors: per sequence normal (S, 3), offset (S), quat (S, 4), trans (S, 3), rms (S), gap (S) float32, used (S)
# int32, ok (S) uint8; per frame and foot contact (Ntot, nf) uint8, height (Ntot, nf) float32; skate (S) float32, skate_pairs (S) int32
Ground = namedtuple("Ground", "normal offset quat trans rms gap used ok contact height skate skate_pairs")


def _ground(lib, points, valid, d_off, S, feet, axis, radius, speed, sigma, prior, iters, foot_height):
    """``mp_lift_ground`` on points (Ntot, J, C) with valid (Ntot) uint8 or None: a ``Ground`` of new tensors"""
    ntot, J, ch = (int(v) for v in points.shape)
    dev, nf = points.device, len(feet)
    f32s = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)
    i32s = lambda *shape: torch.empty(*shape, dtype=torch.int32, device=dev)
    g = Ground(f32s(S, 3), f32s(S), f32s(S, 4), f32s(S, 3), f32s(S), f32s(S), i32s(S), torch.empty(S, dtype=torch.uint8, device=dev),
               torch.empty(ntot, nf, dtype=torch.uint8, device=dev), f32s(ntot, nf), f32s(S), i32s(S))
    _launch(dev, "mp_lift_ground", _lib.ptr(points), ntot, J, ch, _lib.ptr(valid), _lib.ptr(d_off), S, (C.c_int32 * nf)(*feet), nf, axis[0], axis[1],
            int(radius), float(speed), float(sigma), float(prior), int(iters), float(foot_height), *(_lib.ptr(t) for t in g))
    return g


def estimate_ground(points, seq_offset=None, valid=None, feet=(3, 6), axis=(0, 8), radius=2, speed=0.01, sigma=0.03, prior=0.05, iters=5,
                    foot_height=0.0):
    """``mp_lift_ground`` on device tensors: which way is up and where the floor is, from the motion itself.  ``points`` (Ntot, J, 3 | 4) float32:
    ABSOLUTE joint positions (poses plus their root trajectory) in any rigid frame, a camera's or a world (channel 3 is not read); ``seq_offset``
    (S + 1): first frame of every sequence, HOST table or device int64 tensor (default: one sequence); ``valid`` uint8 (Ntot) or None.  ``feet``:
    1..4 joint indices (default the H36M ankles), ``axis``: two joints whose difference points up the body (default pelvis, thorax).  A foot is in
    CONTACT in frame f where its central difference over f - radius .. f + radius (radius 1..8, all three frames valid, finite and in one
    sequence) is at most ``speed`` per frame; the plane through a sequence's contact points is the smallest eigenvector of their scatter,
    re-weighted ``iters`` times (0..8) with 1 / (1 + r^2 / sigma^2)^2 so that a slow foot held in the air is shed (``sigma`` = inf: no weight), and
    pulled by ``prior`` (a length; 0: off) towards the plane perpendicular to the body's mean axis - what decides a sequence whose feet never move,
    two points that span a line.  The axis also decides which side is up.  include/manipose_hip.h has the rule.  Returns a ``Ground`` of new device
    tensors: ``normal`` (S, 3), ``offset`` (S) = normal . a point of the plane, ``quat`` (S, 4) the shortest rotation taking the normal onto +z and
    ``trans`` (S, 3) = (0, 0, foot_height - offset): ``to_world(points, g.quat, translation=g.trans, seq_offset=...)`` stands every sequence up with
    its contact feet at z = ``foot_height``, heading and horizontal origin unchanged; ``rms`` (S) the weighted RMS distance of the contact points from
    the plane; ``gap`` (S) in 0..1, (a2 - a1) / (a3 - a1) of the scatter's eigenvalues: near 0 the contacts lie on a line and the prior chose the
    plane; ``used`` (S) int32 contact points; ``ok`` (S) uint8: bit 0 a plane exists (else normal (0, 0, 1), quat (1, 0, 0, 0), zeros), bit 1 the
    body axis decided the up side; ``contact`` (Ntot, nf) uint8; ``height`` (Ntot, nf) each foot's height over the plane; ``skate`` (S) the mean
    in-plane step of a foot between two consecutive frames in contact, per frame, and ``skate_pairs`` (S) int32 the number of such pairs.  points is
    not modified; fp64 inside, identical bits on every call.  The defaults are untuned, and nothing here has been measured on real data."""
    lift_args.ground_options(radius, speed, sigma, prior, iters, foot_height, GROUND_MAXRADIUS, GROUND_MAXITERS)
    ntot, J = lift_args.points3(points)                  # (the ValueErrors come before the refusal of a CPU tensor)
    feet, axis = lift_args.ground_joints(feet, axis, J, GROUND_MAXFEET)
    lift_args.mask(valid, (ntot,), "valid")
    if ntot < 1:
        raise ValueError("points hold no frame")
    shape = None if seq_offset is None else tuple(seq_offset.shape if torch.is_tensor(seq_offset) else np.shape(seq_offset))
    if shape is not None and (len(shape) != 1 or shape[0] < 2 or shape[0] - 1 > ntot):
        raise ValueError(f"seq_offset must hold S + 1 >= 2 frame numbers, S <= {ntot} frames, got shape {shape}")
    lift_args.need_device("estimate_ground", points, optional=(valid,))
    d_off, S = _seq_table(seq_offset, ntot, points.device)
    return _ground(_lib.load(), points, None if valid is None else valid.contiguous(), d_off, S, feet, axis, radius, speed, sigma, prior, iters,
                   foot_height)


FOOTLOCK_MAXBLEND = 32       # MP_LIFT_FOOTLOCK_MAXBLEND of include/manipose_hip.h
H36M_LEGS = ((1, 2, 3), (4, 5, 6))      # (hip, knee, ankle) of the right and the left leg of the 17-joint H36M tree
# What lock_feet returns, device tensors: points (Ntot, J, C) float32; per frame and foot run (Ntot, nf) int32, target (Ntot, nf, 3), moved (Ntot, nf)
# float32, flags (Ntot, nf) uint8; per sequence runs (S, nf) int32, skate (S) float32, skate_pairs (S) int32
FootLock = namedtuple("FootLock", "points run target moved flags runs skate skate_pairs")


def _footlock(lib, points, contact, valid, d_off, S, legs, floor, blend, stretch):
    """``mp_lift_footlock`` on points (Ntot, J, C), contact (Ntot, nf) uint8, valid (Ntot) uint8 or None, floor (normal, offset, ok) or None: (out, run,
    target, moved, flags, runs), new tensors"""
    ntot, J, ch = (int(v) for v in points.shape)
    dev, nf = points.device, len(legs)
    res = (torch.empty_like(points), torch.empty(ntot, nf, dtype=torch.int32, device=dev), torch.empty(ntot, nf, 3, dtype=torch.float32, device=dev),
           torch.empty(ntot, nf, dtype=torch.float32, device=dev), torch.empty(ntot, nf, dtype=torch.uint8, device=dev),
           torch.empty(S, nf, dtype=torch.int32, device=dev))
    normal, offset, ok = floor if floor is not None else (None, None, None)
    _launch(dev, "mp_lift_footlock", _lib.ptr(points), ntot, J, ch, _lib.ptr(valid), _lib.ptr(d_off), S, _lib.ptr(contact),
            (C.c_int32 * (3 * nf))(*(j for leg in legs for j in leg)), nf, _lib.ptr(normal), _lib.ptr(offset), _lib.ptr(ok), int(blend), float(stretch),
            *(_lib.ptr(t) for t in res))
    return res


def _skate(points, contact, valid, d_off, S, ankles, floor):
    """The foot skate of ``points`` over the contact pairs of ``contact``, as mp_lift_ground reports it, with plain torch on the device: per sequence the
    mean over the pairs (contact[f][k] and contact[f + 1][k], both frames in the sequence, valid and the ankle finite: what mp_lift_ground's own
    contacts always are) of the ankle's step, its part in the plane where the sequence has one, in fp64 -> (skate (S) float32, 0 without a pair,
    skate_pairs (S) int32).  Every sequence is summed on its own, in frame order (``torch.segment_reduce`` over the sequences' frames): no atomics,
    nothing is read back to the host."""
    ntot, dev = int(points.shape[0]), points.device
    bounds = torch.cummax(d_off.clamp(0, ntot), dim=0)[0]                # (first frames that do not decrease: every frame in one segment at most)
    frame = torch.arange(ntot, device=dev)
    seq = (torch.searchsorted(bounds, frame, right=True) - 1).clamp(0, S - 1)
    held = (frame >= bounds[seq]) & (frame < bounds[seq + 1])
    a = points[:, list(ankles), :3].double()
    good = held if valid is None else held & (valid != 0)
    touch = (contact != 0) & good[:, None] & torch.isfinite(a).all(dim=2)
    pair = (seq[:-1] == seq[1:])[:, None] & touch[:-1] & touch[1:]
    d = a[1:] - a[:-1]                                                   # (Ntot - 1, nf, 3)
    if floor is not None:
        n = floor[0].double()[seq[:-1]]                                  # (Ntot - 1, 3)
        has = ((floor[2][seq[:-1]] & 1) != 0) & torch.isfinite(n).all(dim=1) & torch.isfinite(floor[1][seq[:-1]])
        n = torch.where(has[:, None], n, torch.zeros_like(n))[:, None]   # (without a plane the whole step)
        d = d - (d * n).sum(dim=2, keepdim=True) * n
    zero = torch.zeros((), dtype=torch.float64, device=dev)
    per_frame = torch.zeros(ntot, 2, dtype=torch.float64, device=dev)    # a pair belongs to its first frame: (the feet's steps, their number)
    per_frame[:-1, 0] = torch.where(pair, d.norm(dim=2), zero).sum(dim=1)
    per_frame[:-1, 1] = pair.sum(dim=1).double()
    sums = torch.segment_reduce(per_frame, "sum", offsets=bounds, axis=0, unsafe=True)      # (S, 2); a count in fp64 is exact
    skate = torch.where(sums[:, 1] > 0, sums[:, 0] / sums[:, 1].clamp(min=1.0), zero)
    return skate.float(), sums[:, 1].int()


def lock_feet(points, contact, seq_offset=None, valid=None, legs=H36M_LEGS, ground=None, blend=5, stretch=1.0):
    """``mp_lift_footlock`` on device tensors: the feet pinned where they stand, by leg IK on the contacts.  ``points`` (Ntot, J, 3 | 4) float32: ABSOLUTE
    joint positions in any rigid frame (channel 3 is copied); ``contact`` (Ntot, nf) uint8: ``estimate_ground(...).contact``, or the caller's own;
    ``seq_offset`` (S + 1): first frame of every sequence, HOST table or device int64 tensor (default: one sequence); ``valid`` uint8 (Ntot) or None;
    ``legs``: 1..4 triples (hip, knee, ankle), no joint named twice (default the H36M legs, their ankles ``estimate_ground``'s default feet).
    A RUN is a maximal stretch of consecutive frames of one sequence in which a foot is in contact (the frame valid, the leg finite).  The foot is
    pinned to the run's anchor, the mean of its ankle positions; the frames within ``blend`` (0..32) frames of a run are eased into and out of the
    pin by a smoothstep, and between two runs closer than that the correction passes from one pin to the next.  ``ground``: a ``Ground`` of the same
    sequences or None; only its ``normal``, ``offset`` and ``ok`` are read: where a sequence has a plane the anchors are put on it and a swing foot
    below it is lifted onto it.  Every leg is then re-posed by analytic two-bone IK with the frame's own thigh and shank lengths, the knee on the side
    it was on; ``stretch`` in (0, 1] is the share of thigh + shank the leg may reach.  The hip and every other joint keep their bits, and so does a
    leg whose foot is already where it belongs.  include/manipose_hip.h has the rule.  Returns a ``FootLock`` of new device tensors: ``points``
    (Ntot, J, C); ``run`` (Ntot, nf) int32 the length of the run a frame lies in, else 0; ``target`` (Ntot, nf, 3) where the ankle was sent;
    ``moved`` (Ntot, nf) how far it went; ``flags`` (Ntot, nf) uint8: 1 pinned, 2 eased, 4 reach clamped, 8 lifted onto the floor, 16 straight leg (the
    knee's side comes from an axis), 32 a leg without length, left alone; ``runs`` (S, nf) int32 runs per foot; ``skate`` (S) float32 and
    ``skate_pairs`` (S) int32: the foot skate of the RETURNED points over the contact pairs of ``contact`` - the mean step of an ankle between two
    consecutive valid frames in contact with the ankle finite, its part in the plane where ``ground`` has one - comparable with ``Ground.skate`` of the
    input.  The inputs are not modified and nothing is read back to the host; fp64 inside, identical bits on every call.  The defaults are untuned,
    and nothing here has been measured on real data."""
    lift_args.footlock_options(blend, stretch, FOOTLOCK_MAXBLEND)
    ntot, J = lift_args.points3(points)                  # (the ValueErrors come before the refusal of a CPU tensor)
    legs = lift_args.leg_joints(legs, J, GROUND_MAXFEET)
    if contact is None:
        raise ValueError(f"contact must be a uint8 tensor of shape {(ntot, len(legs))}, got None")
    lift_args.mask(contact, (ntot, len(legs)), "contact")
    lift_args.mask(valid, (ntot,), "valid")
    if ntot < 1:
        raise ValueError("points hold no frame")
    shape = None if seq_offset is None else tuple(seq_offset.shape if torch.is_tensor(seq_offset) else np.shape(seq_offset))
    if shape is not None and (len(shape) != 1 or shape[0] < 2 or shape[0] - 1 > ntot):
        raise ValueError(f"seq_offset must hold S + 1 >= 2 frame numbers, S <= {ntot} frames, got shape {shape}")
    floor = lift_args.floor_record(ground, 1 if shape is None else shape[0] - 1)
    lift_args.need_device("lock_feet", points, contact, optional=(valid,) + (floor or ()))
    d_off, S = _seq_table(seq_offset, ntot, points.device)
    contact = contact.contiguous()
    floor = None if floor is None else tuple(t.contiguous() for t in floor)
    out, run, target, moved, flags, runs = _footlock(_lib.load(), points, contact, None if valid is None else valid.contiguous(), d_off, S, legs, floor,
                                                     blend, stretch)
    skate, pairs = _skate(out, contact, valid, d_off, S, [leg[2] for leg in legs], floor)
    return FootLock(out, run, target, moved, flags, runs, skate, pairs)


FK_POSE_LENGTHS = 1          # MP_LIFT_FK_POSE_LENGTHS of include/manipose_hip.h
# What retime_rotations returns, device tensors: quat (Mtot[, inner], J, 4) float32, root (Mtot[, inner], 3) float32 or None, ok and taps
# (Mtot[, inner]) uint8, seq_offset (S + 1) int64 the OUTPUT frames of every sequence, time (Mtot,) float64 the sampled input times
Retimed = namedtuple("Retimed", "quat root ok taps seq_offset time")


def _fk(lib, q4, root, d_lengths, d_off, S, parents, rest, per_pose):
    """``mp_lift_fk`` on q4 (Ntot, inner, J, 4), root (Ntot, inner, 3) or None, lengths (S, J - 1) or per pose (Ntot, inner, J - 1):
    (poses (Ntot, inner, J, 3), ok (Ntot, inner) uint8), new tensors"""
    ntot, inner, J, _ = (int(v) for v in q4.shape)
    dev = q4.device
    poses = torch.empty(ntot, inner, J, 3, dtype=torch.float32, device=dev)
    ok = torch.empty(ntot, inner, dtype=torch.uint8, device=dev)
    _launch(dev, "mp_lift_fk", _lib.ptr(q4), _lib.ptr(root), _lib.ptr(d_lengths), ntot, inner, J, _lib.ptr(d_off), S, parents, rest,
            FK_POSE_LENGTHS if per_pose else 0, _lib.ptr(poses), _lib.ptr(ok))
    return poses, ok


def pose_from_rotations(quat, bones, root=None, seq_offset=None, skeleton=None):
    """``mp_lift_fk`` on device tensors, the inverse of ``pose_rotations``: the joint positions of (root, quat, bones) under the decoder's forward
    kinematics (Rw[0] = q[0], Rw[j] = Rw[parent] q[j], p[0] = root, p[j] = p[parent] + bones[j - 1] Rw[j] rest_j).  ``quat`` (Ntot, J, 4) or
    (Ntot, inner, J, 4) float32 (w, x, y, z), normalised in fp64 before use; ``bones``: per SEQUENCE (S, J - 1) or (J - 1,), tensor or array, finite
    and non-negative (what ``lift_sequences(return_bones=True)`` returns), or per POSE a float32 device tensor (Ntot[, inner], J - 1) - without a
    rigid stage only each frame's own measured lengths give the pose back; ``root`` (Ntot[, inner], 3) float32 or None (the origin);
    ``seq_offset`` (S + 1): first frame of every sequence, HOST table or device int64 tensor (default: one sequence), read for per-sequence bones
    alone; ``skeleton``: anything with ``parents`` and ``t_pose_operators`` (default, for J = 17 only: the H36M tree).  Returns ``(poses, ok)``:
    poses (Ntot[, inner], J, 3) float32; ok (Ntot[, inner]) uint8, 0 where a quaternion of the pose is zero or not finite (|q|^2 < 1e-12): all its
    joints then sit on its root.  fp64 inside, identical bits on every call (include/manipose_hip.h has the rule)."""
    q4 = lift_args.quats4(quat)
    ntot, inner, J = (int(v) for v in q4.shape[:3])
    lead = tuple(quat.shape[:-2])
    if skeleton is None and J != 17:
        raise ValueError(f"quat has {J} joints: the default skeleton is the 17-joint H36M tree; pass a skeleton with parents and t_pose_operators")
    sk = _skeleton_of(skeleton=skeleton)
    parents, rest = _parents_c(sk, J), _rest_c(sk, J)
    if root is not None:
        lift_args.f32(root, lead + (3,), "root", contiguous=True)
    shape = None if seq_offset is None else tuple(seq_offset.shape if torch.is_tensor(seq_offset) else np.shape(seq_offset))
    if shape is not None and (len(shape) != 1 or shape[0] < 2 or shape[0] - 1 > ntot):
        raise ValueError(f"seq_offset must hold S + 1 >= 2 frame numbers, S <= {ntot} frames, got shape {shape}")
    S = 1 if shape is None else shape[0] - 1
    got = tuple(bones.shape) if torch.is_tensor(bones) else np.shape(bones)
    per_pose = got == lead + (J - 1,) and got not in ((S, J - 1), (J - 1,))
    if per_pose:
        lift_args.f32(bones, lead + (J - 1,), "bones (one row per pose)", contiguous=True)
        table = None
    else:
        table = _host_f32(bones, (S, J - 1), "bones", row=(J - 1,), nonneg=True)
    lift_args.need_device("pose_from_rotations", quat, optional=(root, bones if per_pose else None))
    d_off = None if per_pose else _seq_table(seq_offset, ntot, quat.device)[0]
    d_len = bones if per_pose else torch.from_numpy(table).to(quat.device)
    poses, ok = _fk(_lib.load(), q4, root, d_len, d_off, S, parents, rest, per_pose)
    return poses.view(lead + (J, 3)), ok.view(lead)


def _retime(lib, q4, root, valid, d_off, d_out, d_clock, S, mtot, radius, degree, taper):
    """``mp_lift_retime`` on q4 (Ntot, inner, J, 4), root (Ntot, inner, 3) or None, valid (Ntot, inner) uint8 or None and the device tables:
    (quat (Mtot, inner, J, 4), root (Mtot, inner, 3) or None, ok, taps (Mtot, inner) uint8), new tensors"""
    ntot, inner, J, _ = (int(v) for v in q4.shape)
    dev = q4.device
    quat = torch.empty(mtot, inner, J, 4, dtype=torch.float32, device=dev)
    rout = torch.empty(mtot, inner, 3, dtype=torch.float32, device=dev) if root is not None else None
    ok, taps = (torch.empty(mtot, inner, dtype=torch.uint8, device=dev) for _ in range(2))
    _launch(dev, "mp_lift_retime", _lib.ptr(q4), _lib.ptr(root), _lib.ptr(valid), ntot, inner, J, _lib.ptr(d_off), _lib.ptr(d_out), _lib.ptr(d_clock), S,
            mtot, int(radius), int(degree), TAPER[taper], _lib.ptr(quat), _lib.ptr(rout), _lib.ptr(ok), _lib.ptr(taps))
    return quat, rout, ok, taps


def retime_rotations(quat, root=None, valid=None, seq_offset=None, fps_in=1, fps_out=1, start=0.0, radius=0, degree=2, taper="uniform"):
    """``mp_lift_retime`` on device tensors: a take resampled in time on its rotations.  ``quat`` (Ntot, J, 4) or (Ntot, inner, J, 4) float32 as
    ``pose_rotations`` returns it (sign-continuous tracks stay sign-continuous); ``root`` (Ntot[, inner], 3) float32 or None; ``valid`` uint8
    (Ntot[, inner]) or None (every frame is valid); ``seq_offset`` (S + 1): first frame of every sequence, HOST table or device int64 tensor
    (default: one sequence; a device table is read back once, the output's frame counts are host numbers).  ``fps_in`` / ``fps_out``: positive
    integers, the input's and the output's frame rate; ``start`` >= 0 in input frames, one number or one per sequence.  Output frame h of a
    sequence of n frames samples it at t = start + h fps_in / fps_out; the sequence gets the M = floor((n - 1 - start) fps_out / fps_in) + 1 frames
    whose t does not pass its last frame.  ``radius`` 0: the short-way slerp of the two frames around t and the root between them linearly, both
    of which must be valid (nothing is filled); an integer t returns its frame's bits, so fps_in == fps_out with start 0 is the identity.
    ``radius`` 1..64: ``smooth_poses``' weighted local polynomial (``degree``, ``taper``) over the valid frames within ``radius`` of t, fitted in the
    tangent space of the frame nearest to t and evaluated at t - holes are filled, a window with valid frames on one side only is held constant;
    fps_in == fps_out then is smoothing in rotation space (``smooth_rotations``).  Returns a ``Retimed`` of new device tensors: ``quat``
    (Mtot[, inner], J, 4); ``root`` (Mtot[, inner], 3) or None; ``ok`` uint8: 1 a result (else identities and a zero root), + 2 where t had to be
    clamped into the sequence; ``taps`` uint8 the input frames the result was formed from; ``seq_offset`` (S + 1) int64 the output frames of every
    sequence; ``time`` (Mtot,) float64 every output frame's t.  ``pose_from_rotations(r.quat, bones, r.root, r.seq_offset)`` gives the retimed
    positions, on exactly the take's bone table.  fp64 inside, identical bits on every call (include/manipose_hip.h has the rule)."""
    lift_args.retime_options(fps_in, fps_out, radius, degree, taper, SMOOTH_MAXR, TAPER)
    q4 = lift_args.quats4(quat)
    ntot, inner, J = (int(v) for v in q4.shape[:3])
    lead = tuple(quat.shape[:-2])
    if root is not None:
        lift_args.f32(root, lead + (3,), "root", contiguous=True)
    lift_args.mask(valid, lead, "valid")
    on_device = torch.is_tensor(seq_offset) and seq_offset.is_cuda
    plan = None if on_device else lift_args.retime_plan(seq_offset.numpy() if torch.is_tensor(seq_offset) else seq_offset, ntot, fps_in, fps_out, start)
    lift_args.need_device("retime_rotations", quat, optional=(root, valid))
    if plan is None:
        plan = lift_args.retime_plan(seq_offset.cpu().numpy(), ntot, fps_in, fps_out, start)
    off, out_off, clock, time = plan
    dev, S, mtot = quat.device, int(off.size) - 1, int(out_off[-1])
    d_off, d_out = (torch.from_numpy(t).to(dev) for t in (off, out_off))
    got = _retime(_lib.load(), q4, None if root is None else root.view(ntot, inner, 3), None if valid is None else valid.contiguous().view(ntot, inner),
                  d_off, d_out, torch.from_numpy(clock).to(dev), S, mtot, radius, degree, taper)
    out_lead = (mtot,) + lead[1:]
    return Retimed(got[0].view(out_lead + (J, 4)), None if got[1] is None else got[1].view(out_lead + (3,)), got[2].view(out_lead), got[3].view(out_lead),
                   d_out, torch.from_numpy(time).to(dev))


def smooth_rotations(quat, root=None, valid=None, seq_offset=None, radius=4, degree=2, taper="uniform"):
    """Smoothing in rotation space: ``retime_rotations`` at the input's own frames (fps_in == fps_out, start 0) with ``radius`` 1..64 - the filter of
    ``smooth_poses`` on the rotations and the root instead of the joint positions, so the bones of ``pose_from_rotations`` on the result are the bone
    table's by construction.  Returns the same ``Retimed`` record (its seq_offset and time are the input's frames)."""
    _smooth_options(radius, degree, taper)
    return retime_rotations(quat, root, valid, seq_offset, 1, 1, 0.0, radius, degree, taper)


EULER_CONTINUOUS = 1         # MP_LIFT_EULER_CONTINUOUS of include/manipose_hip.h
EULER_ORDERS = ("XYZ", "XZY", "YXZ", "YZX", "ZXY", "ZYX")      # mp_lift_euler's order = the index
# What euler_from_rotations returns, device tensors: angles (Ntot[, inner], J, 3) float32 degrees in channel order, pos (Ntot[, inner], 3) float32
# or None, ok (Ntot[, inner]) uint8
Eulers = namedtuple("Eulers", "angles pos ok")


def _euler(lib, q4, root, valid, d_off, S, d_basis, d_shift, scale, order, continuous):
    """``mp_lift_euler`` on q4 (Ntot, inner, J, 4), root (Ntot, inner, 3) or None, valid (Ntot, inner) uint8 or None, basis (S, 4) and shift (S, 3)
    device tables or both None: (angles (Ntot, inner, J, 3), pos (Ntot, inner, 3) or None, ok (Ntot, inner) uint8), new tensors"""
    ntot, inner, J, _ = (int(v) for v in q4.shape)
    dev = q4.device
    angles = torch.empty(ntot, inner, J, 3, dtype=torch.float32, device=dev)
    pos = torch.empty(ntot, inner, 3, dtype=torch.float32, device=dev) if root is not None else None
    ok = torch.empty(ntot, inner, dtype=torch.uint8, device=dev)
    _launch(dev, "mp_lift_euler", _lib.ptr(q4), _lib.ptr(root), _lib.ptr(valid), ntot, inner, J, _lib.ptr(d_off), S, _lib.ptr(d_basis), _lib.ptr(d_shift),
            float(scale), EULER_ORDERS.index(order), EULER_CONTINUOUS if continuous else 0, _lib.ptr(angles), _lib.ptr(pos), _lib.ptr(ok))
    return angles, pos, ok


def euler_from_rotations(quat, root=None, valid=None, seq_offset=None, order="ZXY", continuous=True, basis=None, shift=None, scale=1.0):
    """``mp_lift_euler`` on device tensors: the Euler channels of a take's joint rotations, what ``manipose_amd.bvh.write_bvh`` writes.  ``quat``
    (Ntot, J, 4) or (Ntot, inner, J, 4) float32 (w, x, y, z) as ``pose_rotations`` or ``retime_rotations`` return it, normalised in fp64 before
    use; ``root`` (Ntot[, inner], 3) float32 or None; ``valid`` uint8 (Ntot[, inner]) or None (every frame is valid); ``seq_offset`` (S + 1): first
    frame of every sequence, HOST table or device int64 tensor (default: one sequence); ``order``: one of XYZ, XZY, YXZ, YZX, ZXY, ZYX - the
    angles (al, be, ga) of joint j satisfy R(q[j]) = R_i(al) R_j(be) R_k(ga), BVH's channel convention; ``basis`` (S, 4) or (4,) and ``shift``
    (S, 3) or (3,), tensors or arrays, finite, or None (identity, zero): a rigid transform per sequence in ``to_world``'s convention,
    p' = qrot(basis, p) + shift, applied to the root's rotation (on the left) and position - ``estimate_ground``'s quat and trans stand the take
    on its floor; ``scale`` > 0 multiplies the positions (100: centimetres).  ``continuous``: every (sequence, inner index, joint) track is then
    made continuous in time - where the other Euler solution of the same rotation, (al + 180, 180 - be, ga + 180), lies nearer to the frame before
    it is taken, and whole turns are added so that no channel jumps by more than 180 degrees between two frames with a result: a curve a tool can
    interpolate between its keys.  Returns an ``Eulers`` of new device tensors: ``angles`` (Ntot[, inner], J, 3) float32 DEGREES in channel
    order; ``pos`` (Ntot[, inner], 3) float32 or None; ``ok`` uint8: 0 where the frame is invalid or a quaternion of the pose (or the basis) is
    zero or not finite (|q|^2 < 1e-12) - angles and pos are then +0 and the frame is transparent to the continuity -, 1 a result, 3 a result with
    a joint in gimbal lock (be = +-90: ga is then 0 and al carries both).  fp64 inside, identical bits on every call (include/manipose_hip.h has
    the rule)."""
    lift_args.euler_options(order, scale, EULER_ORDERS)
    q4 = lift_args.quats4(quat)
    ntot, inner, J = (int(v) for v in q4.shape[:3])
    lead = tuple(quat.shape[:-2])
    if root is not None:
        lift_args.f32(root, lead + (3,), "root", contiguous=True)
    lift_args.mask(valid, lead, "valid")
    shape = None if seq_offset is None else tuple(seq_offset.shape if torch.is_tensor(seq_offset) else np.shape(seq_offset))
    if shape is not None and (len(shape) != 1 or shape[0] < 2 or shape[0] - 1 > ntot):
        raise ValueError(f"seq_offset must hold S + 1 >= 2 frame numbers, S <= {ntot} frames, got shape {shape}")
    S = 1 if shape is None else shape[0] - 1
    h_basis = h_shift = None
    if basis is not None or shift is not None:
        h_basis = _host_f32(basis if basis is not None else np.array([1.0, 0.0, 0.0, 0.0], np.float32), (S, 4), "basis", row=(4,))
        h_shift = _host_f32(shift if shift is not None else np.zeros(3, np.float32), (S, 3), "shift", row=(3,))
    lift_args.need_device("euler_from_rotations", quat, optional=(root, valid))
    dev = quat.device
    d_off = _seq_table(seq_offset, ntot, dev)[0]
    d_basis, d_shift = (None, None) if h_basis is None else (torch.from_numpy(h_basis).to(dev), torch.from_numpy(h_shift).to(dev))
    angles, pos, ok = _euler(_lib.load(), q4, None if root is None else root.view(ntot, inner, 3), None if valid is None else valid.contiguous().view(ntot, inner),
                             d_off, S, d_basis, d_shift, scale, order, bool(continuous))
    return Eulers(angles.view(lead + (J, 3)), None if pos is None else pos.view(lead + (3,)), ok.view(lead))


REFINE_MAXITERS = 16         # MP_LIFT_REFINE_MAXITERS of include/manipose_hip.h: Gauss-Newton steps mp_lift_place_refine takes at most
FLOOR_SHARES = 16            # MP_LIFT_WORLD_SHARES of include/manipose_hip.h: partial minima per sequence in mp_lift_world's scratch


def camera_table(cameras):
    """Per-sequence cameras as the float32 numpy tables the kernels read: ``intr`` (S, 9) = (fx, fy, cx, cy, k1, k2, k3, p1, p2) in normalised
    screen units, ``quat`` (S, 4) = (w, x, y, z), ``trans`` (S, 3) in metres.  ``cameras``: one entry per sequence, either a dict as
    ``h36m_cameras()`` gives (``intrinsic``, ``orientation``, optionally ``translation``: zeros when absent) or a 1-D array of at least 16
    numbers in ``fetch()``'s order (intrinsic 9, orientation 4, translation 3[, camera index]).  ValueError for a wrong shape or a non-finite entry."""
    if isinstance(cameras, dict) or (hasattr(cameras, "ndim") and getattr(cameras, "ndim", 0) == 1):
        raise ValueError("cameras must be a list with one camera per sequence (a dict or a 1-D array of >= 16 numbers each)")
    cams = list(cameras)
    if not cams:
        raise ValueError("cameras is empty: one camera per sequence expected")
    rows = np.zeros((len(cams), 16), dtype=np.float32)
    for s, cam in enumerate(cams):
        if isinstance(cam, dict):
            if "intrinsic" not in cam or "orientation" not in cam:
                raise ValueError(f"camera {s}: a camera dict needs 'intrinsic' (9) and 'orientation' (4)")
            parts = [np.asarray(cam["intrinsic"]), np.asarray(cam["orientation"]), np.asarray(cam.get("translation", np.zeros(3)))]
            for name, a, n in zip(("intrinsic", "orientation", "translation"), parts, (9, 4, 3)):
                if a.shape != (n,) or a.dtype.kind not in "fiu":
                    raise ValueError(f"camera {s}: '{name}' must be {n} numbers, got shape {a.shape} {a.dtype}")
            row = np.concatenate([a.astype(np.float64) for a in parts])
        else:
            a = cam.detach().cpu().numpy() if torch.is_tensor(cam) else np.asarray(cam)
            if a.ndim != 1 or a.shape[0] < 16 or a.dtype.kind not in "fiu":
                raise ValueError(f"camera {s}: expected a dict or a 1-D array of at least 16 numbers (intrinsic 9, orientation 4, translation 3), "
                                 f"got shape {a.shape} {a.dtype}")
            row = a[:16].astype(np.float64)
        if not np.isfinite(row).all():
            raise ValueError(f"camera {s}: non-finite entry")
        rows[s] = row
    return rows[:, :9].copy(), rows[:, 9:13].copy(), rows[:, 13:16].copy()


def _place_refine(lib, p4, kp, d_off, S, d_intr, d_w, distort, iters, start=None, start_ok=None):
    """``mp_lift_place_refine`` on p4 (Ntot, inner, J, C), the one launcher of the fit: (traj, reproj, ok, steps), new tensors; start (Ntot, inner, 3)
    or None: the linear fit (with iters = 0: what ``mp_lift_place`` computes, by the same kernel), start_ok (Ntot, inner) uint8 or None"""
    ntot, inner, J, ch = (int(v) for v in p4.shape)
    dev = p4.device
    traj = torch.empty(ntot, inner, 3, dtype=torch.float32, device=dev)
    reproj = torch.empty(ntot, inner, dtype=torch.float32, device=dev)
    ok = torch.empty(ntot, inner, dtype=torch.uint8, device=dev)
    steps = torch.empty(ntot, inner, dtype=torch.uint8, device=dev)
    if ntot > 0:
        _launch(dev, "mp_lift_place_refine", _lib.ptr(p4), ntot, inner, J, ch, _lib.ptr(kp), _lib.ptr(d_off), S, _lib.ptr(d_intr), _lib.ptr(d_w),
                int(bool(distort)), _lib.ptr(start), _lib.ptr(start_ok), int(iters), _lib.ptr(traj), _lib.ptr(reproj), _lib.ptr(ok), _lib.ptr(steps))
    return traj, reproj, ok, steps


def _world(lib, p4, traj, d_off, S, d_quat, d_trans, floor_mode=0, d_floor=None):
    ntot, inner, J, ch = (int(v) for v in p4.shape)
    if ntot == 0:
        return
    scratch = torch.empty(S * FLOOR_SHARES, dtype=torch.float32, device=p4.device) if floor_mode == 1 else None
    _launch(p4.device, "mp_lift_world", _lib.ptr(p4), ntot, inner, J, ch, _lib.ptr(traj), _lib.ptr(d_off), S, _lib.ptr(d_quat), _lib.ptr(d_trans),
            int(floor_mode), _lib.ptr(d_floor), _lib.ptr(scratch), S * FLOOR_SHARES if floor_mode == 1 else 0)


def _place_inputs(poses, keypoints_2d, intrinsics, seq_offset, weights, who):
    """the checks and uploads place_poses and reproject_poses share: (p4, keypoints, d_off, S, d_intr, d_w)"""
    p4 = _poses4(poses, who)
    dev, ntot, J = poses.device, int(p4.shape[0]), int(p4.shape[2])
    lift_args.need_device(who, keypoints_2d)
    lift_args.f32(keypoints_2d, (ntot, J, 2), "keypoints_2d", plain=True)
    d_off, S = _seq_table(seq_offset, ntot, dev)
    d_intr = _device_f32(intrinsics, dev, (S, 9), "intrinsics", row=(9,) if S == 1 else None)
    d_w = _device_f32(weights, dev, (J,), "weights", nonneg=True) if weights is not None else None
    return p4, keypoints_2d.contiguous(), d_off, S, d_intr, d_w


def place_poses(poses, keypoints_2d, intrinsics, seq_offset=None, weights=None, distort=True, refine=0, return_steps=False):
    """``mp_lift_place`` on device tensors: per pose the root translation that fits the frame's 2-D keypoints, and the reprojection error.
    ``poses`` (Ntot, J, 3) or (Ntot, inner, J, 3 | 4) float32 (channel 3, a hypothesis' score, is not read); ``keypoints_2d`` (Ntot, J, 2) in
    normalised screen coordinates, shared by the ``inner`` poses of a frame; ``intrinsics`` (S, 9) or (9,), tensor or array, as
    ``camera_table`` / ``h36m_cameras()[s][i]["intrinsic"]``; ``seq_offset`` (S + 1): first frame of every sequence, HOST table or device int64
    tensor (default: one sequence); ``weights`` (J) non-negative or None (all ones; a joint of weight 0 is skipped).  The fit uses the pinhole
    part of the camera; the error the full model (``distort=True``, the reference's project_to_2d) or project_to_2d_linear, in normalised screen
    units (times res_w / 2: pixels).  Returns ``traj`` (Ntot[, inner], 3) in the poses' unit, ``reproj`` (Ntot[, inner]), ``ok`` uint8: 0 where the
    fit is degenerate (no weight, a non-finite input, all keypoints on one spot: traj and reproj are 0) or puts a joint behind the camera.
    ``refine`` (0..16, default 0: the linear fit alone, ``mp_lift_place``): ``mp_lift_place_refine`` starts from that fit and takes up to that many
    undamped Gauss-Newton steps on the weighted squared reprojection error of the projection ``distort`` names - the fit then uses the model the
    error is measured with; a step is taken only while the normal matrix is regular, the translation stays finite and in front of the camera, and
    the cost does not rise (include/manipose_hip.h has the rule); ``reproj`` is the error at the refined translation.  ``return_steps`` appends
    ``steps`` uint8 (Ntot[, inner]): the steps taken (0 everywhere without ``refine``)."""
    if not lift_args.is_int_in(refine, 0, REFINE_MAXITERS):
        raise ValueError(f"refine counts Gauss-Newton steps, an integer in 0..{REFINE_MAXITERS} (0: the linear fit alone), got {refine!r}")
    p4, kp, d_off, S, d_intr, d_w = _place_inputs(poses, keypoints_2d, intrinsics, seq_offset, weights, "place_poses")
    res = _place_refine(_lib.load(), p4, kp, d_off, S, d_intr, d_w, distort, refine)[:4 if return_steps else 3]
    return tuple(r[:, 0] for r in res) if poses.dim() == 3 else tuple(res)


def reproject_poses(poses, traj, keypoints_2d, intrinsics, ok=None, seq_offset=None, weights=None, distort=True):
    """``mp_lift_place_refine`` with zero steps on a GIVEN trajectory: the reprojection error of poses placed at ``traj`` - a smoothed trajectory,
    a ground-truth one, another method's.  ``traj`` (Ntot[, inner], 3) float32 device tensor shaped like ``place_poses`` returns it, ``ok`` uint8
    (Ntot[, inner]) or None (every frame is given); the other arguments as for ``place_poses``.  Returns ``(reproj, ok)``: reproj (Ntot[, inner])
    float32 in normalised screen units, the weighted mean distance between the keypoints and the projection of pose + traj; ok uint8, 0 with
    reproj = 0 where ``ok`` was 0 or traj is not finite, 0 with reproj as computed where a joint lies behind the camera or the error is not
    finite, else 1."""
    if torch.is_tensor(poses) and torch.is_tensor(traj):
        lift_args.poses4(poses)
        lift_args.f32(traj, tuple(poses.shape[:-2]) + (3,), "traj", plain=True)
        lift_args.mask(ok, traj.shape[:-1], "ok")
    lift_args.need_device("reproject_poses", traj, optional=(ok,))
    p4, kp, d_off, S, d_intr, d_w = _place_inputs(poses, keypoints_2d, intrinsics, seq_offset, weights, "reproject_poses")
    _, reproj, good, _ = _place_refine(_lib.load(), p4, kp, d_off, S, d_intr, d_w, distort, 0, traj.contiguous(), None if ok is None else ok.contiguous())
    return (reproj[:, 0], good[:, 0]) if poses.dim() == 3 else (reproj, good)


def to_world(poses, orientation, translation=None, traj=None, seq_offset=None, floor=False):
    """``mp_lift_world`` on a device tensor, IN PLACE (and returned): every joint p <- qrot(q_s, p + traj) + t_s.  ``poses`` (Ntot, J, 3) or
    (Ntot, inner, J, 3 | 4) (channel 3 is left alone); ``orientation`` (S, 4) or (4,) quaternions (w, x, y, z) as the dataset stores them (not
    normalised here, like the reference's qrot); ``translation`` (S, 3) / (3,) or None; ``traj`` (Ntot[, inner], 3) device tensor as
    ``place_poses`` returns it, or None - with both None this is the reference's camera_to_world(., R, t = 0); ``seq_offset`` as for
    ``place_poses``.  ``floor=True``: every sequence's lowest joint is put on z = 0 and ``(poses, offsets)`` is returned, offsets (S,) = the
    minimum z subtracted; ``floor`` = a tensor or array (S,): those offsets are subtracted instead (one scene for several arrays)."""
    p4 = _poses4(poses, "to_world")
    dev, ntot = poses.device, int(p4.shape[0])
    d_off, S = _seq_table(seq_offset, ntot, dev)
    d_quat = _device_f32(orientation, dev, (S, 4), "orientation", row=(4,) if S == 1 else None)
    d_trans = _device_f32(translation, dev, (S, 3), "translation", row=(3,) if S == 1 else None) if translation is not None else None
    if traj is not None:
        lift_args.need_device("to_world", traj)
        lift_args.f32(traj, tuple(poses.shape[:-2]) + (3,), "traj", plain=True)
        traj = traj.contiguous()
    mode = 1 if floor is True else 0 if floor is False or floor is None else 2          # mp_lift_world's floor_mode: measure, none, given
    d_floor = None if mode == 0 else torch.empty(S, dtype=torch.float32, device=dev) if mode == 1 else \
        _device_f32(floor, dev, (S,), "floor", row=() if S == 1 else None)
    _world(_lib.load(), p4, traj, d_off, S, d_quat, d_trans, mode, d_floor)
    return (poses, d_floor) if mode == 1 else poses

"""Whole-sequence lifting: 2-D keypoints ``(N, 17, 2)`` of any length in, one 3-D pose per frame out.

Counterpart of the reference's ``lift_action`` (hpe/eval_utils.py:226-253, used by hpe/viz.py:84-91): windows with the
``drop_last=False`` replicate padding of its generator (hpe/mh_so3_hpe/data/generators.py:93-104,135-154), the flip test-time
augmentation of its evaluation loop (eval_utils.py:84-142) and the flattening of the predictions - here with windows that may
overlap (``stride < T``) and everything on the device: the raw keypoints are uploaded once, ``mp_lift_windows_2d`` cuts the
(mirrored) windows, the engine runs its no-backward forward, and ONE kernel (``mp_lift_merge``) aggregates the hypotheses, undoes
the mirroring and blends the windows that cover a frame, reading every hypothesis once.

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

Scheduling: a sequence is lifted on its own - its windows are cut into forwards of ``batch`` (``2 * batch`` with TTA), all of them
stay resident until the sequence is merged, and no forward mixes two sequences.  A frame's covering windows are therefore always
resident when it is merged (no partial sum is ever carried), and a sequence's result does not depend on what else is lifted with
it: the engine's GEMM tile plan depends on the batch, so a window's bits do.

Structure: ``lift_sequences`` is a chain of private stages - ``_check_options`` (every argument error, then an immutable record of resolved
options), ``_upload`` (keypoints, window tables, offsets and output buffers, once), ``_lift_one`` per sequence (forwards and ONE merge),
``_path_stage``, ``_smooth_poses_stage``, ``_rigid_stage``, ``_score_stage`` (with ``targets``), ``_place_stage`` (with ``_smooth_traj_stage``, ``_reproj_smooth_stage`` and ``_score_traj_stage`` between its fit and its world transform), ``_rotations_stage`` (last, on the poses as emitted), ``_per_sequence`` - whose result is ONE record, ``_Lifted``, with the fields poses, hyps, bones, place, path, score, rotations.  The
public function turns the record into its documented list / tuple in one place; ``lift_action`` and hpe/_entry.py read the fields by name.
Placing has ONE launcher, ``_place_refine``, as the library has one fit kernel: ``place_poses``, ``reproject_poses`` and ``_place_stage`` all go
through it, and zero steps from the linear fit is what ``mp_lift_place`` computes.
Fusing the camera views of a take (``fuse_views_path``: ``fuse_views``' choice made jointly over the whole take, a Viterbi path over the combinations,
so that a hypothesis all views agree on - a mirrored body - cannot make the fused motion flicker; ``fuse_views``: one hypothesis per view, chosen jointly, and their mean; ``place_views``: one world root per frame
from all views) is NOT a stage of the chain: they work on what ``lift_sequences`` returns for the views, and hpe/_entry.py (``lift.fuse``) cuts a
group's sequences into takes and calls them.
"""
from __future__ import annotations

import ctypes as C
from collections import namedtuple
from typing import Sequence, Tuple

import numpy as np
import torch

from . import _lib

AGG = {"weighted_ave": 0, "best_score": 1}
BLEND = {"mean": 0, "center": 1}
TAPER = {"uniform": 0, "biweight": 1}
SMOOTH_MAXR = 64             # MP_LIFT_SMOOTH_MAXR of include/manipose_hip.h
PATH_MAXK = 8                # hypotheses mp_lift_path takes
PATH_SIGMA, PATH_SWITCH = 0.02, 0.0      # defaults of agg="path": the step's standard deviation in metres (not tuned), the cost of a switch


def plan_windows(lengths: Sequence[int], T: int, stride: int) -> Tuple[np.ndarray, np.ndarray]:
    """(win_seq, win_start) int32 tables of the windows that cover sequences of ``lengths`` frames: per sequence of N frames
    ``1 + ceil(max(0, N - T) / stride)`` windows at starts 0, stride, 2 stride, ...  ``stride == T`` gives the reference's
    ``_map_index_to_pose`` / ``_map_index_to_frame`` for ``drop_last=False`` (generators.py:93-104)."""
    T, stride = int(T), int(stride)
    if T < 1 or not 1 <= stride <= T:
        raise ValueError(f"plan_windows: stride {stride} outside 1..T (T={T})")
    seq, start = [], []
    for s, n in enumerate(lengths):
        n = int(n)
        if n < 1:
            raise ValueError(f"plan_windows: sequence {s} has {n} frames")
        nw = 1 + -(-max(0, n - T) // stride)
        seq.append(np.full(nw, s, dtype=np.int32))
        start.append(np.arange(nw, dtype=np.int32) * np.int32(stride))
    if not seq:
        return np.zeros(0, np.int32), np.zeros(0, np.int32)
    return np.concatenate(seq), np.concatenate(start)


def _model_shape(model):
    cfg = getattr(model, "_engine_cfg", None)
    if cfg is None:
        raise RuntimeError("manipose_amd: lift_sequences needs a MixSTE, ManifoldMixSTE or RMCLManifoldMixSTE model")
    from .architectures import RMCLManifoldMixSTE
    return int(cfg["num_frame"]), int(cfg["num_joints"]), int(model.n_hyp) if isinstance(model, RMCLManifoldMixSTE) else 1


def _skeleton_of(model=None, skeleton=None):
    """``skeleton`` if given, else the model's own, else the 17-joint H36M tree (MixSTE carries none)"""
    from .data import h36m_skeleton
    if skeleton is not None:
        return skeleton
    return model.decoder.skeleton if model is not None and hasattr(model, "decoder") else h36m_skeleton()


def _mirror(model, J):
    sk = _skeleton_of(model)
    m = list(range(J))
    for l, r in zip(sk.joints_left, sk.joints_right):
        m[l], m[r] = r, l
    return (C.c_int32 * J)(*m)


def _i32p(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


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
    if not torch.is_tensor(poses) or not poses.is_cuda:
        raise RuntimeError(f"manipose_amd: {who} takes device tensors; there is no CPU fallback")
    return _poses4_shape(poses)


def _poses4_shape(poses):
    p4 = poses.unsqueeze(1) if poses.dim() == 3 else poses
    if p4.dim() != 4 or p4.shape[3] not in (3, 4) or (poses.dim() == 3 and poses.shape[2] != 3) or poses.dtype != torch.float32 \
            or not poses.is_contiguous():
        raise ValueError(f"poses must be contiguous float32 (Ntot, J, 3) or (Ntot, inner, J, 3 | 4), got {tuple(poses.shape)} {poses.dtype}")
    if not 2 <= int(p4.shape[2]) <= 32:
        raise ValueError(f"poses have {int(p4.shape[2])} joints: 2..32 expected")
    return p4


def _rigid(lib, poses4, d_off, S, d_lengths, parents):
    ntot, inner, J, ch = (int(v) for v in poses4.shape)
    with torch.cuda.device(poses4.device):
        _lib.check(lib.mp_lift_rigid(_lib.ptr(poses4), ntot, inner, J, ch, _lib.ptr(d_off), S, _lib.ptr(d_lengths), parents, _lib.stream_ptr()),
                   "mp_lift_rigid")


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
    with torch.cuda.device(dev):
        _lib.check(_lib.load().mp_bone_length_means(_lib.ptr(poses), int(poses.shape[0]), J, _lib.ptr(d_off), _lib.ptr(d_real), S, parents, _lib.ptr(out), _lib.stream_ptr()),
                   "mp_bone_length_means")
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
        with torch.cuda.device(dev):
            _lib.check(lib.mp_lift_rotations(_lib.ptr(p4), ntot, inner, J, ch, _lib.ptr(d_off), S, parents, rest, ROT_CONTINUOUS if continuous else 0,
                                             _lib.ptr(quat), _lib.ptr(rot6d), _lib.ptr(ok), _lib.stream_ptr()), "mp_lift_rotations")
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
        _poses4_shape(poses)
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


def _is_radius(r, lowest):
    return isinstance(r, (int, np.integer)) and not isinstance(r, (bool, np.bool_)) and lowest <= int(r) <= SMOOTH_MAXR


def _smooth_options(radius, degree, taper):
    if not _is_radius(radius, 1):
        raise ValueError(f"radius must be an integer in 1..{SMOOTH_MAXR}, got {radius!r}")
    if not isinstance(degree, (int, np.integer)) or isinstance(degree, (bool, np.bool_)) or not 0 <= int(degree) <= 2:
        raise ValueError(f"degree must be 0, 1 or 2, got {degree!r}")
    if taper not in TAPER:
        raise ValueError(f"taper must be one of {sorted(TAPER)}, got {taper!r}")


def _smooth(lib, x4, valid, d_off, S, radius, degree, taper, want_filled=False):
    """``mp_lift_smooth`` on x4 (Ntot, inner, M, C) with valid (Ntot, inner) uint8 or None: (a new tensor, filled (Ntot, inner) uint8 or None)"""
    ntot, inner, M, ch = (int(v) for v in x4.shape)
    out = torch.empty_like(x4)
    filled = torch.empty(ntot, inner, dtype=torch.uint8, device=x4.device) if want_filled else None
    if ntot > 0:
        with torch.cuda.device(x4.device):
            _lib.check(lib.mp_lift_smooth(_lib.ptr(x4), _lib.ptr(out), ntot, inner, M, ch, _lib.ptr(valid), _lib.ptr(d_off), S, int(radius), int(degree),
                                          TAPER[taper], _lib.ptr(filled), _lib.stream_ptr()), "mp_lift_smooth")
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
        _poses4_shape(poses)                             # (the ValueErrors come before the refusal of a CPU tensor)
    p4 = _poses4(poses, "smooth_poses")
    d_off, S = _seq_table(seq_offset, int(p4.shape[0]), poses.device)
    return _smooth(_lib.load(), p4, None, d_off, S, radius, degree, taper)[0].view(poses.shape)


def _traj_shape(traj):
    if traj.dim() not in (2, 3) or traj.shape[-1] != 3 or traj.dtype != torch.float32 or not traj.is_contiguous():
        raise ValueError(f"traj must be contiguous float32 (Ntot, 3) or (Ntot, inner, 3), got {tuple(traj.shape)} {traj.dtype}")


def smooth_traj(traj, ok=None, seq_offset=None, radius=4, degree=2, taper="uniform"):
    """``mp_lift_smooth`` on root trajectories, OUT of place: traj (Ntot, 3) or (Ntot, inner, 3) float32 device tensor as ``place_poses`` returns it,
    ``ok`` uint8 of shape (Ntot[, inner]) or None (every frame is valid): a frame with ok = 0 does not enter any fit, and gets the value the fit
    through its valid neighbours has at it - constant where valid frames lie on one side only.  Returns ``(smoothed, filled)``: filled uint8
    (Ntot[, inner]) is 0 where no frame within the radius in the same sequence is valid; such a frame keeps its input bits.  The other arguments
    as for ``smooth_poses``."""
    _smooth_options(radius, degree, taper)
    if torch.is_tensor(traj):
        _traj_shape(traj)
        if ok is not None and (not torch.is_tensor(ok) or tuple(ok.shape) != tuple(traj.shape[:-1]) or ok.dtype != torch.uint8):
            raise ValueError(f"ok must be a uint8 tensor of shape {tuple(traj.shape[:-1])}, got "
                             f"{(tuple(ok.shape), ok.dtype) if torch.is_tensor(ok) else type(ok).__name__}")
    if not torch.is_tensor(traj) or not traj.is_cuda or (ok is not None and not ok.is_cuda):
        raise RuntimeError("manipose_amd: smooth_traj takes device tensors; there is no CPU fallback")
    ntot = int(traj.shape[0])
    d_off, S = _seq_table(seq_offset, ntot, traj.device)
    out, filled = _smooth(_lib.load(), traj.view(ntot, -1, 1, 3), None if ok is None else ok.contiguous().view(ntot, -1), d_off, S, radius, degree,
                          taper, want_filled=True)
    return out.view(traj.shape), filled.view(traj.shape[:-1])


def _path_options(sigma, switch_cost, names=("sigma", "switch_cost")):
    for v in (sigma, switch_cost):
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)):
            raise ValueError(f"{names[0]} and {names[1]} are numbers, got {v!r}")
    if not float(np.float32(sigma)) > 0:                     # (as the kernel takes it: a float32; +inf is allowed)
        raise ValueError(f"{names[0]} must be > 0 (inf: the step costs nothing), got {sigma!r}")
    if not 0 <= float(switch_cost) <= float(np.finfo(np.float32).max):
        raise ValueError(f"{names[1]} must be finite and >= 0, got {switch_cost!r}")


def _hyps4_shape(hyps):
    if hyps.dim() != 4 or hyps.shape[3] != 4 or hyps.dtype != torch.float32 or not hyps.is_contiguous():
        raise ValueError(f"hyps must be contiguous float32 (Ntot, K, J, 4), got {tuple(hyps.shape)} {hyps.dtype}")
    if not 1 <= int(hyps.shape[1]) <= PATH_MAXK:
        raise ValueError(f"hyps have {int(hyps.shape[1])} hypotheses: 1..{PATH_MAXK} expected")
    if not 2 <= int(hyps.shape[2]) <= 32:
        raise ValueError(f"hyps have {int(hyps.shape[2])} joints: 2..32 expected")
    return hyps


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
        with torch.cuda.device(dev):
            _lib.check(lib.mp_lift_path(_lib.ptr(hyps), ntot, K, J, _lib.ptr(d_off), S, float(sigma), float(switch_cost), _lib.ptr(path), _lib.ptr(out),
                                        _lib.ptr(cost), _lib.ptr(scratch), n, _lib.stream_ptr()), "mp_lift_path")
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
    _path_options(sigma, switch_cost)
    if torch.is_tensor(hyps):
        _hyps4_shape(hyps)                               # (the ValueErrors come before the refusal of a CPU tensor)
    if not torch.is_tensor(hyps) or not hyps.is_cuda:
        raise RuntimeError("manipose_amd: select_path takes device tensors; there is no CPU fallback")
    d_off, S = _seq_table(seq_offset, int(hyps.shape[0]), hyps.device)
    return _path(_lib.load(), hyps, d_off, S, sigma, switch_cost)


SCORE_SHARES = 32            # MP_LIFT_SCORE_SHARES of include/manipose_hip.h: partial rows per (sequence, inner) in mp_lift_score's scratch
SCORE_ROOT_RELATIVE, SCORE_PROCRUSTES = 1, 2     # mp_lift_score's flags
# What score_poses returns: device float64 tensors of shape (S,), or (S, inner) for 4-D poses; per_joint (.., M); bone_* (.., M - 1) or None without a
# skeleton; rows: mp_lift_score's raw sums (.., 9 + M + 3 (M - 1)); frame_err (Ntot[, inner]) float32 with return_frames, else None
PoseScore = namedtuple("PoseScore", "frames mpjpe rmse mpjve accel p_mpjpe per_joint bone_mean bone_std bone_err rows frame_err")
# What score_traj returns: (S,) or (S, inner) device float64 tensors
TrajScore = namedtuple("TrajScore", "frames ate rmse velocity accel")


def _is_scale(v):
    return isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, (bool, np.bool_)) and np.isfinite(float(v)) and float(v) > 0


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
        with torch.cuda.device(dev):
            _lib.check(lib.mp_lift_score(_lib.ptr(p4), ntot, inner, M, ch, _lib.ptr(gt), _lib.ptr(valid), _lib.ptr(d_off), S, parents, float(pred_scale),
                                         float(gt_scale), int(flags), _lib.ptr(rows), _lib.ptr(frame_err), _lib.ptr(scratch), n, _lib.stream_ptr()),
                       "mp_lift_score")
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


def _score_valid(valid, shape, name):
    if valid is not None and (not torch.is_tensor(valid) or tuple(valid.shape) != tuple(shape) or valid.dtype != torch.uint8):
        raise ValueError(f"{name} must be a uint8 tensor of shape {tuple(shape)}, got "
                         f"{(tuple(valid.shape), valid.dtype) if torch.is_tensor(valid) else type(valid).__name__}")


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
    if not _is_scale(pose_scale) or not _is_scale(target_scale):
        raise ValueError(f"pose_scale and target_scale must be finite numbers > 0, got {pose_scale!r}, {target_scale!r}")
    parents = None
    if torch.is_tensor(poses):
        p4 = _poses4_shape(poses)                        # (the ValueErrors come before the refusal of a CPU tensor)
        ntot, inner, J = int(p4.shape[0]), int(p4.shape[1]), int(p4.shape[2])
        if not torch.is_tensor(target) or tuple(target.shape) != (ntot, J, 3) or target.dtype != torch.float32 or not target.is_contiguous():
            raise ValueError(f"target must be a contiguous float32 tensor ({ntot}, {J}, 3), got "
                             f"{(tuple(target.shape), target.dtype) if torch.is_tensor(target) else type(target).__name__}")
        _score_valid(valid, poses.shape[:-2], "valid")
        if procrustes and J < 3:
            raise ValueError(f"procrustes=True aligns poses of at least 3 joints, got {J}")
        if skeleton is not None or J == 17:
            parents = _parents_c(_skeleton_of(skeleton=skeleton), J)
    if not torch.is_tensor(poses) or not poses.is_cuda or not target.is_cuda or (valid is not None and not valid.is_cuda):
        raise RuntimeError("manipose_amd: score_poses takes device tensors; there is no CPU fallback")
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
        _traj_shape(traj)
        if not torch.is_tensor(target) or tuple(target.shape) != (int(traj.shape[0]), 3) or target.dtype != torch.float32 or not target.is_contiguous():
            raise ValueError(f"target must be a contiguous float32 tensor ({int(traj.shape[0])}, 3), got "
                             f"{(tuple(target.shape), target.dtype) if torch.is_tensor(target) else type(target).__name__}")
        _score_valid(ok, traj.shape[:-1], "ok")
    if not torch.is_tensor(traj) or not traj.is_cuda or not target.is_cuda or (ok is not None and not ok.is_cuda):
        raise RuntimeError("manipose_amd: score_traj takes device tensors; there is no CPU fallback")
    ntot = int(traj.shape[0])
    d_off, S = _seq_table(seq_offset, ntot, traj.device)
    rows = _score(_lib.load(), traj.view(ntot, -1, 1, 3), target.view(ntot, 1, 3), None if ok is None else ok.contiguous().view(ntot, -1), d_off, S, None,
                  1.0, 1.0, 0)[0]
    return _traj_record(rows[:, 0] if traj.dim() == 2 else rows)


def _traj_record(rows):
    n = rows[..., 0]
    return TrajScore(n, _ratio(rows[..., 1], n), torch.sqrt(_ratio(rows[..., 2], n)), _ratio(rows[..., 4], rows[..., 3]), _ratio(rows[..., 6], rows[..., 5]))


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


def _is_iters(n):
    return isinstance(n, (int, np.integer)) and not isinstance(n, (bool, np.bool_)) and 0 <= int(n) <= REFINE_MAXITERS


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
        with torch.cuda.device(dev):
            _lib.check(lib.mp_lift_place_refine(_lib.ptr(p4), ntot, inner, J, ch, _lib.ptr(kp), _lib.ptr(d_off), S, _lib.ptr(d_intr), _lib.ptr(d_w),
                                                int(bool(distort)), _lib.ptr(start), _lib.ptr(start_ok), int(iters), _lib.ptr(traj), _lib.ptr(reproj),
                                                _lib.ptr(ok), _lib.ptr(steps), _lib.stream_ptr()), "mp_lift_place_refine")
    return traj, reproj, ok, steps


def _world(lib, p4, traj, d_off, S, d_quat, d_trans, floor_mode=0, d_floor=None):
    ntot, inner, J, ch = (int(v) for v in p4.shape)
    if ntot == 0:
        return
    scratch = torch.empty(S * FLOOR_SHARES, dtype=torch.float32, device=p4.device) if floor_mode == 1 else None
    with torch.cuda.device(p4.device):
        _lib.check(lib.mp_lift_world(_lib.ptr(p4), ntot, inner, J, ch, _lib.ptr(traj), _lib.ptr(d_off), S, _lib.ptr(d_quat), _lib.ptr(d_trans),
                                     int(floor_mode), _lib.ptr(d_floor), _lib.ptr(scratch), S * FLOOR_SHARES if floor_mode == 1 else 0,
                                     _lib.stream_ptr()), "mp_lift_world")


def _place_inputs(poses, keypoints_2d, intrinsics, seq_offset, weights, who):
    """the checks and uploads place_poses and reproject_poses share: (p4, keypoints, d_off, S, d_intr, d_w)"""
    p4 = _poses4(poses, who)
    dev, ntot, J = poses.device, int(p4.shape[0]), int(p4.shape[2])
    if not torch.is_tensor(keypoints_2d) or not keypoints_2d.is_cuda:
        raise RuntimeError(f"manipose_amd: {who} takes device tensors; there is no CPU fallback")
    if tuple(keypoints_2d.shape) != (ntot, J, 2) or keypoints_2d.dtype != torch.float32:
        raise ValueError(f"keypoints_2d must be float32 ({ntot}, {J}, 2), got {tuple(keypoints_2d.shape)} {keypoints_2d.dtype}")
    d_off, S = _seq_table(seq_offset, ntot, dev)
    d_intr = _device_f32(intrinsics, dev, (S, 9), "intrinsics", row=(9,) if S == 1 else None)
    d_w = _device_f32(weights, dev, (J,), "weights", nonneg=True) if weights is not None else None
    return p4, keypoints_2d.contiguous(), d_off, S, d_intr, d_w


def _traj_of_poses(traj, poses):
    if tuple(traj.shape) != tuple(poses.shape[:-2]) + (3,) or traj.dtype != torch.float32:
        raise ValueError(f"traj must be float32 {tuple(poses.shape[:-2]) + (3,)}, got {tuple(traj.shape)} {traj.dtype}")


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
    if not _is_iters(refine):
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
        _poses4_shape(poses)
        _traj_of_poses(traj, poses)
        _score_valid(ok, traj.shape[:-1], "ok")
    if not torch.is_tensor(traj) or not traj.is_cuda or (ok is not None and not ok.is_cuda):
        raise RuntimeError("manipose_amd: reproject_poses takes device tensors; there is no CPU fallback")
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
        if not torch.is_tensor(traj) or not traj.is_cuda:
            raise RuntimeError("manipose_amd: to_world takes device tensors; there is no CPU fallback")
        _traj_of_poses(traj, poses)
        traj = traj.contiguous()
    if floor is True:
        d_floor = torch.empty(S, dtype=torch.float32, device=dev)
        _world(_lib.load(), p4, traj, d_off, S, d_quat, d_trans, 1, d_floor)
        return poses, d_floor
    if floor is False or floor is None:
        _world(_lib.load(), p4, traj, d_off, S, d_quat, d_trans)
        return poses
    d_floor = _device_f32(floor, dev, (S,), "floor", row=() if S == 1 else None)
    _world(_lib.load(), p4, traj, d_off, S, d_quat, d_trans, 2, d_floor)
    return poses


FUSE_MAXV, FUSE_MAXK = 4, 8  # MP_LIFT_FUSE_MAXV, MP_LIFT_FUSE_MAXK of include/manipose_hip.h: views of a take, hypotheses of a view
FUSE_SIGMA, FUSE_SCORE_WEIGHT = 0.02, 1.0    # defaults of fuse_views: the views' disagreement in metres (not tuned), the weight of -log(score)


def _fuse_options(sigma, score_weight, names=("sigma", "score_weight")):
    _path_options(sigma, score_weight, names)              # the same two rules: sigma > 0 (inf allowed), the other finite and >= 0


def _fuse_quat(orientation, G, V):
    """(G, V, 4) float32 host quaternions, (V, 4) standing for one take; a zero quaternion is refused here (the kernel would ignore the view)"""
    h = _host_f32(orientation, (G, V, 4), "orientation", row=(V, 4) if G == 1 else None)
    if not ((h.astype(np.float64) ** 2).sum(-1) >= 1e-12).all():
        raise ValueError("orientation holds a zero quaternion: mark a missing view in valid and give it any unit quaternion")
    return h


def _fuse_valid(valid, V, ftot, who):
    if valid is None:
        return None
    _score_valid(valid, (V, ftot), "valid")
    if not valid.is_cuda:
        raise RuntimeError(f"manipose_amd: {who} takes device tensors; there is no CPU fallback")
    return valid.contiguous()


def _fuse(lib, hyps, valid, d_off, G, d_quat, sigma, score_weight):
    """``mp_lift_fuse`` on hyps (V, Ftot, K, J, C): (pose, choice, cost, spread, ok), new tensors"""
    V, ftot, K, J, ch = (int(v) for v in hyps.shape)
    dev = hyps.device
    pose = torch.empty(ftot, J, 3, dtype=torch.float32, device=dev)
    choice = torch.empty(ftot, V, dtype=torch.uint8, device=dev)
    cost = torch.empty(ftot, dtype=torch.float32, device=dev)
    spread = torch.empty(ftot, dtype=torch.float32, device=dev)
    ok = torch.empty(ftot, dtype=torch.uint8, device=dev)
    if ftot > 0:
        with torch.cuda.device(dev):
            _lib.check(lib.mp_lift_fuse(_lib.ptr(hyps), V, ftot, K, J, ch, _lib.ptr(valid), _lib.ptr(d_off), G, _lib.ptr(d_quat), float(sigma),
                                        float(score_weight), _lib.ptr(pose), _lib.ptr(choice), _lib.ptr(cost), _lib.ptr(spread), _lib.ptr(ok),
                                        _lib.stream_ptr()), "mp_lift_fuse")
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
        with torch.cuda.device(dev):
            _lib.check(lib.mp_lift_fuse_place(_lib.ptr(pose), _lib.ptr(kp), V, ftot, J, _lib.ptr(valid), _lib.ptr(d_off), G, _lib.ptr(d_quat),
                                              _lib.ptr(d_trans), _lib.ptr(d_intr), _lib.ptr(d_w), int(bool(distort)), int(iters), _lib.ptr(root),
                                              _lib.ptr(reproj), _lib.ptr(ok), _lib.ptr(steps), _lib.stream_ptr()), "mp_lift_fuse_place")
    return root, reproj, ok, steps


def _fuse_hyps_shape(hyps):
    if hyps.dim() != 5 or hyps.shape[4] not in (3, 4) or hyps.dtype != torch.float32 or not hyps.is_contiguous():
        raise ValueError(f"hyps must be contiguous float32 (V, Ftot, K, J, 3 | 4), got {tuple(hyps.shape)} {hyps.dtype}")
    V, _, K, J, _ = (int(v) for v in hyps.shape)
    if not 1 <= V <= FUSE_MAXV:
        raise ValueError(f"hyps have {V} views: 1..{FUSE_MAXV} expected")
    if not 1 <= K <= FUSE_MAXK:
        raise ValueError(f"hyps have {K} hypotheses: 1..{FUSE_MAXK} expected")
    if not 2 <= J <= 32:
        raise ValueError(f"hyps have {J} joints: 2..32 expected")


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
    _fuse_options(sigma, score_weight)
    if torch.is_tensor(hyps):
        _fuse_hyps_shape(hyps)                            # (the ValueErrors come before the refusal of a CPU tensor)
        V, ftot = int(hyps.shape[0]), int(hyps.shape[1])
        _score_valid(valid, (V, ftot), "valid")
        G = 1 if take_offset is None else max(int(take_offset.numel() if torch.is_tensor(take_offset) else np.asarray(take_offset).size) - 1, 1)
        h_quat = _fuse_quat(orientation, G, V) if orientation is not None else None
    if not torch.is_tensor(hyps) or not hyps.is_cuda:
        raise RuntimeError("manipose_amd: fuse_views takes device tensors; there is no CPU fallback")
    valid = _fuse_valid(valid, V, ftot, "fuse_views")
    d_off, G = _seq_table(take_offset, ftot, hyps.device)
    d_quat = torch.from_numpy(h_quat).to(hyps.device) if h_quat is not None else None
    return _fuse(_lib.load(), hyps, valid, d_off, G, d_quat, sigma, score_weight)


def _fuse_path(lib, hyps, valid, d_off, G, d_quat, sigma, score_weight, path_sigma, switch_cost):
    """``mp_lift_fuse_path`` on hyps (V, Ftot, K, J, C): (pose, choice, cost, spread, ok, path_cost (G,) float64), new tensors"""
    V, ftot, K, J, ch = (int(v) for v in hyps.shape)
    dev = hyps.device
    pose = torch.empty(ftot, J, 3, dtype=torch.float32, device=dev)
    choice = torch.empty(ftot, V, dtype=torch.uint8, device=dev)
    cost = torch.empty(ftot, dtype=torch.float32, device=dev)
    spread = torch.empty(ftot, dtype=torch.float32, device=dev)
    ok = torch.empty(ftot, dtype=torch.uint8, device=dev)
    path_cost = torch.zeros(G, dtype=torch.float64, device=dev)
    if ftot > 0:
        n = int(lib.mp_lift_fuse_path_scratch_bytes(V, ftot, K))
        scratch = torch.empty(n // 8, dtype=torch.float64, device=dev)
        with torch.cuda.device(dev):
            _lib.check(lib.mp_lift_fuse_path(_lib.ptr(hyps), V, ftot, K, J, ch, _lib.ptr(valid), _lib.ptr(d_off), G, _lib.ptr(d_quat), float(sigma),
                                             float(score_weight), float(path_sigma), float(switch_cost), _lib.ptr(pose), _lib.ptr(choice),
                                             _lib.ptr(cost), _lib.ptr(spread), _lib.ptr(ok), _lib.ptr(path_cost), _lib.ptr(scratch), n,
                                             _lib.stream_ptr()), "mp_lift_fuse_path")
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
    _fuse_options(sigma, score_weight)
    _path_options(path_sigma, switch_cost, ("path_sigma", "switch_cost"))
    if torch.is_tensor(hyps):
        _fuse_hyps_shape(hyps)                            # (the ValueErrors come before the refusal of a CPU tensor)
        V, ftot = int(hyps.shape[0]), int(hyps.shape[1])
        _score_valid(valid, (V, ftot), "valid")
        G = 1 if take_offset is None else max(int(take_offset.numel() if torch.is_tensor(take_offset) else np.asarray(take_offset).size) - 1, 1)
        h_quat = _fuse_quat(orientation, G, V) if orientation is not None else None
    if not torch.is_tensor(hyps) or not hyps.is_cuda:
        raise RuntimeError("manipose_amd: fuse_views_path takes device tensors; there is no CPU fallback")
    valid = _fuse_valid(valid, V, ftot, "fuse_views_path")
    d_off, G = _seq_table(take_offset, ftot, hyps.device)
    d_quat = torch.from_numpy(h_quat).to(hyps.device) if h_quat is not None else None
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


def place_views(pose, keypoints_2d, cameras, valid=None, take_offset=None, weights=None, distort=True, refine=3, return_steps=False):
    """``mp_lift_fuse_place`` on device tensors: ONE world root per frame from all views of its take.  ``pose`` (Ftot, J, 3) float32, root-relative
    in the world's orientation, as ``fuse_views`` returns it; ``keypoints_2d`` (V, Ftot, J, 2) float32, every view's keypoints in normalised screen
    coordinates; ``cameras``: nested list [take][view] of cameras in ``camera_table``'s forms (a dict of ``h36m_cameras()`` with its
    ``translation``, or ``fetch()``'s 16 numbers), None for a view the take does not have; ``valid`` (V, Ftot) uint8 device tensor or None;
    ``take_offset`` (G + 1) as for ``fuse_views``; ``weights`` (J) or None.  The root starts at the linear fit of all views' pinhole projections
    (condition number about 6 with H36M's four cameras, against 6e2 for one view) and takes up to ``refine`` (0..16) Gauss-Newton steps under the
    camera model ``distort`` names, with ``place_poses``' acceptance rule.  Returns ``(root (Ftot, 3), reproj (V, Ftot): every view's own mean
    reprojection error at the root, 0 for an invalid view, ok (Ftot) uint8[, steps (Ftot) uint8])``."""
    if not _is_iters(refine):
        raise ValueError(f"refine counts Gauss-Newton steps, an integer in 0..{REFINE_MAXITERS} (0: the linear fit alone), got {refine!r}")
    if torch.is_tensor(pose) and torch.is_tensor(keypoints_2d):
        if pose.dim() != 3 or pose.shape[2] != 3 or pose.dtype != torch.float32 or not pose.is_contiguous() or not 2 <= int(pose.shape[1]) <= 32:
            raise ValueError(f"pose must be contiguous float32 (Ftot, J, 3) with 2..32 joints, got {tuple(pose.shape)} {pose.dtype}")
        ftot, J = int(pose.shape[0]), int(pose.shape[1])
        kp = keypoints_2d
        if kp.dim() != 4 or not 1 <= int(kp.shape[0]) <= FUSE_MAXV or tuple(kp.shape[1:]) != (ftot, J, 2) or kp.dtype != torch.float32:
            raise ValueError(f"keypoints_2d must be float32 (V <= {FUSE_MAXV}, {ftot}, {J}, 2), got {tuple(kp.shape)} {kp.dtype}")
        V = int(kp.shape[0])
        if valid is not None:
            _score_valid(valid, (V, ftot), "valid")
        intr, quat, trans, present = _take_cameras(cameras, V)
        h_w = _host_f32(weights, (J,), "weights", nonneg=True) if weights is not None else None
    if not torch.is_tensor(pose) or not pose.is_cuda or not torch.is_tensor(keypoints_2d) or not keypoints_2d.is_cuda:
        raise RuntimeError("manipose_amd: place_views takes device tensors; there is no CPU fallback")
    dev = pose.device
    valid = _fuse_valid(valid, V, ftot, "place_views")
    d_off, G = _seq_table(take_offset, ftot, dev)
    if G != intr.shape[0]:
        raise ValueError(f"cameras lists {intr.shape[0]} takes, take_offset {G}")
    if not present.all():                                  # a missing view is invalid in every frame of its take
        off = d_off.cpu().numpy().clip(0, ftot)
        mask = np.ones((V, ftot), np.uint8)
        for g, v in zip(*np.nonzero(~present)):
            mask[v, off[g]:max(off[g], off[g + 1])] = 0
        mask = torch.from_numpy(mask).to(dev)
        valid = mask if valid is None else valid & mask
    res = _fuse_place(_lib.load(), pose, keypoints_2d.contiguous(), valid, d_off, G, torch.from_numpy(quat).to(dev), torch.from_numpy(trans).to(dev),
                      torch.from_numpy(intr).to(dev), torch.from_numpy(h_w).to(dev) if h_w is not None else None, distort, refine)
    return res if return_steps else res[:3]


ALIGN_MAXITERS = 8           # MP_LIFT_ALIGN_MAXITERS of include/manipose_hip.h: re-weightings mp_lift_align_views takes at most
ALIGN_SIGMA, ALIGN_ITERS = 0.05, 5           # defaults of align_views: the scale of a frame's residual in metres, the re-weightings (not tuned)
# What align_views returns: quat (G, V, 4), trans (G, V, 3) or None, rms (G, V), trans_rms (G, V) or None float32, used (G, V) int32, ok (G, V) uint8
ViewAlignment = namedtuple("ViewAlignment", "quat trans rms trans_rms used ok")


def _align_options(sigma, iters):
    if isinstance(sigma, (bool, np.bool_)) or not isinstance(sigma, (int, float, np.integer, np.floating)) or not float(sigma) > 0:
        raise ValueError(f"sigma must be a number > 0 (inf: every frame weighs 1), got {sigma!r}")
    if not isinstance(iters, (int, np.integer)) or isinstance(iters, (bool, np.bool_)) or not 0 <= int(iters) <= ALIGN_MAXITERS:
        raise ValueError(f"iters counts re-weightings, an integer in 0..{ALIGN_MAXITERS} (0: plain Horn), got {iters!r}")


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
        with torch.cuda.device(dev):
            _lib.check(lib.mp_lift_align_views(_lib.ptr(poses), V, ftot, J, ch, _lib.ptr(valid), _lib.ptr(d_off), G, _lib.ptr(traj), _lib.ptr(traj_ok),
                                               float(sigma), int(iters), _lib.ptr(quat), _lib.ptr(trans), _lib.ptr(rms), _lib.ptr(trans_rms),
                                               _lib.ptr(used), _lib.ptr(ok), _lib.stream_ptr()), "mp_lift_align_views")
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
    _align_options(sigma, iters)
    if (traj is None) != (traj_ok is None):
        raise ValueError("traj and traj_ok come together: the views' roots and where they were fitted")
    if torch.is_tensor(poses):
        if poses.dim() != 4 or poses.shape[3] not in (3, 4) or poses.dtype != torch.float32 or not poses.is_contiguous():
            raise ValueError(f"poses must be contiguous float32 (V, Ftot, J, 3 | 4), got {tuple(poses.shape)} {poses.dtype}")
        V, ftot, J = (int(v) for v in poses.shape[:3])
        if not 1 <= V <= FUSE_MAXV:
            raise ValueError(f"poses have {V} views: 1..{FUSE_MAXV} expected")
        if not 2 <= J <= 32:
            raise ValueError(f"poses have {J} joints: 2..32 expected")
        _score_valid(valid, (V, ftot), "valid")
        if traj is not None:
            if not torch.is_tensor(traj) or tuple(traj.shape) != (V, ftot, 3) or traj.dtype != torch.float32:
                raise ValueError(f"traj must be a float32 tensor ({V}, {ftot}, 3), got "
                                 f"{(tuple(traj.shape), traj.dtype) if torch.is_tensor(traj) else type(traj).__name__}")
            if traj_ok is None or not torch.is_tensor(traj_ok):
                raise ValueError(f"traj_ok must be a uint8 tensor of shape ({V}, {ftot})")
            _score_valid(traj_ok, (V, ftot), "traj_ok")
        G = 1 if take_offset is None else max(int(take_offset.numel() if torch.is_tensor(take_offset) else np.asarray(take_offset).size) - 1, 1)
        if reference is not None:
            single = isinstance(reference, dict) or torch.is_tensor(reference) or (hasattr(reference, "ndim") and getattr(reference, "ndim", 0) == 1)
            _, ref_quat, ref_trans = camera_table([reference] if single else reference)
            if ref_quat.shape[0] != G:
                raise ValueError(f"reference lists {ref_quat.shape[0]} cameras, take_offset {G} takes")
            if not ((ref_quat.astype(np.float64) ** 2).sum(-1) >= 1e-12).all():
                raise ValueError("reference holds a zero quaternion")
    if not torch.is_tensor(poses) or not poses.is_cuda or (traj is not None and not (traj.is_cuda and traj_ok.is_cuda)):
        raise RuntimeError("manipose_amd: align_views takes device tensors; there is no CPU fallback")
    valid = _fuse_valid(valid, V, ftot, "align_views")
    d_off, G = _seq_table(take_offset, ftot, poses.device)
    res = _align(_lib.load(), poses, valid, d_off, G, traj.contiguous() if traj is not None else None,
                 traj_ok.contiguous() if traj_ok is not None else None, sigma, iters)
    if reference is None:
        return res
    q, t = _align_compose(res.quat.cpu().numpy(), res.trans.cpu().numpy() if res.trans is not None else None, res.ok.cpu().numpy(), ref_quat, ref_trans)
    return res._replace(quat=torch.from_numpy(q).to(poses.device), trans=torch.from_numpy(t).to(poses.device) if t is not None else None)


BUNDLE_MAXITERS = 8          # MP_LIFT_BUNDLE_MAXITERS of include/manipose_hip.h: Gauss-Newton steps mp_lift_bundle_views takes at most
BUNDLE_SIGMA, BUNDLE_ITERS = 0.05, 3         # defaults of bundle_views: the robust scale in normalised screen units, the steps (not tuned)
# What bundle_views returns: cameras: place_views' nested list [take][view] with the refined extrinsics; quat (G, V, 4), trans (G, V, 3), root (Ftot, 3),
# reproj (G, V, 2) float32, cost (G, 2) float64, steps, ok (G) uint8, used (G, V) int32
ViewBundle = namedtuple("ViewBundle", "cameras quat trans root reproj cost steps ok used")


def _bundle_options(sigma, iters):
    if isinstance(sigma, (bool, np.bool_)) or not isinstance(sigma, (int, float, np.integer, np.floating)) or not float(sigma) > 0:
        raise ValueError(f"sigma must be a number > 0 in normalised screen units (inf: no robust weight), got {sigma!r}")
    if not isinstance(iters, (int, np.integer)) or isinstance(iters, (bool, np.bool_)) or not 0 <= int(iters) <= BUNDLE_MAXITERS:
        raise ValueError(f"iters counts Gauss-Newton steps, an integer in 0..{BUNDLE_MAXITERS} (0: the evaluation alone), got {iters!r}")


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
        with torch.cuda.device(dev):
            _lib.check(lib.mp_lift_bundle_views(_lib.ptr(pose), _lib.ptr(root), _lib.ptr(root_ok), _lib.ptr(kp), V, ftot, J, _lib.ptr(valid), _lib.ptr(d_off),
                                                G, _lib.ptr(d_quat), _lib.ptr(d_trans), _lib.ptr(d_intr), _lib.ptr(d_fixed), _lib.ptr(d_w), int(bool(distort)),
                                                float(sigma), int(iters), _lib.ptr(quat), _lib.ptr(trans), _lib.ptr(out_root), _lib.ptr(reproj),
                                                _lib.ptr(cost), _lib.ptr(steps), _lib.ptr(ok), _lib.ptr(used), _lib.ptr(scratch), n, _lib.stream_ptr()),
                       "mp_lift_bundle_views")
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
    _bundle_options(sigma, iters)
    tensors = torch.is_tensor(pose) and torch.is_tensor(root) and torch.is_tensor(keypoints_2d)
    if tensors:
        if pose.dim() != 3 or pose.shape[2] != 3 or pose.dtype != torch.float32 or not pose.is_contiguous() or not 2 <= int(pose.shape[1]) <= 32:
            raise ValueError(f"pose must be contiguous float32 (Ftot, J, 3) with 2..32 joints, got {tuple(pose.shape)} {pose.dtype}")
        ftot, J = int(pose.shape[0]), int(pose.shape[1])
        if tuple(root.shape) != (ftot, 3) or root.dtype != torch.float32:
            raise ValueError(f"root must be float32 ({ftot}, 3), got {tuple(root.shape)} {root.dtype}")
        kp = keypoints_2d
        if kp.dim() != 4 or not 1 <= int(kp.shape[0]) <= FUSE_MAXV or tuple(kp.shape[1:]) != (ftot, J, 2) or kp.dtype != torch.float32:
            raise ValueError(f"keypoints_2d must be float32 (V <= {FUSE_MAXV}, {ftot}, {J}, 2), got {tuple(kp.shape)} {kp.dtype}")
        V = int(kp.shape[0])
        if valid is not None:
            _score_valid(valid, (V, ftot), "valid")
        if root_ok is not None:
            if not torch.is_tensor(root_ok):
                raise ValueError(f"root_ok must be a uint8 tensor of shape ({ftot},)")
            _score_valid(root_ok, (ftot,), "root_ok")
        intr, quat, trans, present = _take_cameras(cameras, V)
        G = intr.shape[0]
        h_fixed = None
        if fixed is not None:
            h_fixed = np.asarray(fixed.detach().cpu().numpy() if torch.is_tensor(fixed) else fixed)
            if h_fixed.shape == (V,) and G == 1:
                h_fixed = h_fixed.reshape(1, V)
            if h_fixed.shape != (G, V) or h_fixed.dtype.kind not in "biu":
                raise ValueError(f"fixed must be a table ({G}, {V}) of flags, got {h_fixed.shape} {h_fixed.dtype}")
            h_fixed = np.ascontiguousarray(h_fixed != 0, dtype=np.uint8)
        h_w = _host_f32(weights, (J,), "weights", nonneg=True) if weights is not None else None
    if not tensors or not (pose.is_cuda and root.is_cuda and keypoints_2d.is_cuda) or (root_ok is not None and not root_ok.is_cuda):
        raise RuntimeError("manipose_amd: bundle_views takes device tensors; there is no CPU fallback")
    dev = pose.device
    valid = _fuse_valid(valid, V, ftot, "bundle_views")
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
    res = _bundle(_lib.load(), pose, root.contiguous(), root_ok.contiguous() if root_ok is not None else None, keypoints_2d.contiguous(), valid, d_off, G,
                  torch.from_numpy(quat).to(dev), torch.from_numpy(trans).to(dev), torch.from_numpy(intr).to(dev),
                  torch.from_numpy(h_fixed).to(dev) if h_fixed is not None else None, torch.from_numpy(h_w).to(dev) if h_w is not None else None,
                  distort, sigma, iters)
    q, t = res[0].cpu().numpy(), res[1].cpu().numpy()
    nested = [[np.concatenate([intr[g, v], q[g, v], t[g, v]]) if present[g, v] else None for v in range(V)] for g in range(G)]
    return ViewBundle(nested, *res)


def merge_windows(poses, scores, win_seq, win_start, seq_offset, *, T, tta, mirror, agg="weighted_ave", blend="mean", scale=1.0,
                  return_hyps=False, out=None, hyps=None, device_tables=None):
    """``mp_lift_merge`` on device tensors: poses (F*W, K, T, J, 3), scores (F*W, K, T, 1) or None (K == 1); win_seq / win_start (W)
    and seq_offset (S + 1) HOST numpy tables (uploaded here unless ``device_tables`` = their device copies is given).
    Returns (out (Ntot, J, 3), hyps (Ntot, K, J, 4) or None)."""
    if agg not in AGG:
        raise ValueError(f"agg must be one of {sorted(AGG)}, got {agg!r} ('oracle' needs ground truth: hpe/_entry.py::evaluate)")
    if blend not in BLEND:
        raise ValueError(f"blend must be one of {sorted(BLEND)}, got {blend!r}")
    lib = _lib.load()
    F = 2 if tta else 1
    h_seq = np.ascontiguousarray(win_seq, dtype=np.int32)
    h_start = np.ascontiguousarray(win_start, dtype=np.int32)
    h_off = np.ascontiguousarray(seq_offset, dtype=np.int64)
    W, S = int(h_seq.size), int(h_off.size) - 1
    K, J = int(poses.shape[1]), int(poses.shape[3])
    assert poses.shape[0] == F * W and poses.shape[2] == T and poses.shape[4] == 3, "poses must be (F*W, K, T, J, 3)"
    dev = poses.device
    if device_tables is None:
        device_tables = (torch.from_numpy(h_seq).to(dev), torch.from_numpy(h_start).to(dev), torch.from_numpy(h_off).to(dev))
    d_seq, d_start, d_off = device_tables
    ntot = int(h_off[-1]) if S >= 0 and h_off.size else 0
    if out is None:
        out = torch.empty(ntot, J, 3, dtype=torch.float32, device=dev)
    if return_hyps and hyps is None:
        hyps = torch.empty(ntot, K, J, 4, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.mp_lift_merge(_lib.ptr(poses), _lib.ptr(scores), W, K, int(T), J, int(bool(tta)), _lib.ptr(d_seq), _lib.ptr(d_start),
                                     _lib.ptr(d_off), S, _i32p(h_seq), _i32p(h_start), h_off.ctypes.data_as(C.POINTER(C.c_int64)), mirror,
                                     AGG[agg], BLEND[blend], float(scale), _lib.ptr(out), _lib.ptr(hyps) if return_hyps else None,
                                     _lib.stream_ptr()), "mp_lift_merge")
    return out, (hyps if return_hyps else None)


# What a lift was asked for, checked and resolved by _check_options; no stage after it validates anything.  seqs: the 2-D sequences;
# cam_tables: camera_table(cameras) with place / world; lengths: "model", "measured" or "table" with rigid, and table: the caller's checked
# (S, J - 1) one; skeleton, parents: the model's, with rigid; windows: plan_windows' (win_seq, win_start)
# smooth_poses, smooth_traj: the two radii (0: off), smooth_degree, smooth_taper: shared by both; agg: "path" included, path_sigma (metres),
# path_switch, return_path: its options; targets: the checked (N_i, J, 3) ground truth in metres or None, return_score; place_refine: Gauss-Newton
# steps after the linear fit (0: none); rotations, rotations_continuous, return_rotations and rot_tables: the (parents, rest) C tables of the stage
_Options = namedtuple("_Options", "seqs tta agg blend scale return_hyps keep_padding rigid symmetric return_bones place world floor return_place "
                                  "smooth_poses smooth_traj smooth_degree smooth_taper path_sigma path_switch return_path cam_tables T J K lengths table skeleton parents "
                                  "windows batch dev targets return_score place_refine rotations rotations_continuous return_rotations rot_tables",
                      defaults=(None,) * 11 + (None, False, 0, False, True, False, None))
# Everything the kernels of a lift read, uploaded once by _upload, and the buffers they write.  p2: (sum N_i, J, 2) keypoints of all sequences,
# lens: N_i; out_lens: frames emitted per sequence (whole windows with keep_padding), out_off: their (S + 1) offsets in out_all (., J, 3) and
# hyp_all (., K, J, 4); gt: (sum N_i, J, 3) targets of all sequences in metres, joint 0 (the root's position) as given; first: (S + 1) first window of every sequence; merge_off (S, 2), h_zero / d_zero: the offsets (0, out_lens[s]) and the
# win_seq (zeros) of a one-sequence merge; bone_mirror (lengths="model"): bone of joint j <- bone of joint mirror[j]; d_*: device copies
_Plan = namedtuple("_Plan", "p2 lens out_lens out_off first win_start merge_off h_zero d_off d_merge_off d_seq d_start d_zero d_flip mirror "
                            "bone_mirror out_all hyp_all gt", defaults=(None,))
# What _lift_sequences returns: per-sequence lists of the poses, the hypotheses, the bone tables, the place dicts, the (path, cost) pairs, the score
# dicts and the rotation dicts; a field that was not asked for is None
_Lifted = namedtuple("_Lifted", "poses hyps bones place path score rotations", defaults=(None,) * 6)
SCORE_FIELDS = ("frames", "mpjpe", "rmse", "mpjve", "accel", "p_mpjpe", "per_joint", "bone_mean", "bone_std", "bone_err")   # of a score dict


def _check_options(model, poses_2d, *, stride=None, tta=True, agg="weighted_ave", blend="mean", return_hyps=False, batch=None, scale=1.0,
                   keep_padding=False, rigid=False, lengths=None, symmetric=False, return_bones=False, cameras=None, place=False, frame="camera",
                   floor=False, return_place=False, smooth_poses=0, smooth_traj=0, smooth_degree=2, smooth_taper="uniform", path_sigma=PATH_SIGMA,
                   path_switch=PATH_SWITCH, return_path=False, targets=None, return_score=False, place_refine=0, rotations=False,
                   rotations_continuous=True, return_rotations=False):
    """Every argument error of ``lift_sequences``, in a fixed order and before anything touches a device: the ValueErrors first, the "no CPU
    fallback" RuntimeErrors last.  No sequences: the record ends after ``return_place``."""
    if not rigid and (lengths is not None or symmetric or return_bones):
        raise ValueError("lengths, symmetric and return_bones describe rigid lifting: pass rigid=True")
    if frame not in ("camera", "world"):
        raise ValueError(f"frame must be 'camera' or 'world', got {frame!r}")
    if not isinstance(place, (bool, np.bool_)) or not isinstance(floor, (bool, np.bool_)):
        raise ValueError("place and floor are switches (True / False); to_world takes given floor offsets")
    world = frame == "world"
    if place and cameras is None:
        raise ValueError("place=True needs cameras: one camera per sequence (camera_table)")
    if world and cameras is None:
        raise ValueError("frame='world' needs cameras: one camera per sequence (camera_table)")
    if floor and not world:
        raise ValueError("floor=True puts the world frame's z on the floor: pass frame='world'")
    if cameras is not None and not (place or world):
        raise ValueError("cameras describe place=True and frame='world': pass one of them")
    if return_place and not (place or floor):
        raise ValueError("return_place returns what place=True (and floor=True) computed: pass place=True")
    if (place or world) and keep_padding:
        raise ValueError("place / frame='world' with keep_padding=True: padded frames have no keypoints of their own")
    if not _is_iters(place_refine):
        raise ValueError(f"place_refine counts Gauss-Newton steps, an integer in 0..{REFINE_MAXITERS} (0: off), got {place_refine!r}")
    if int(place_refine) > 0 and not place:
        raise ValueError("place_refine refines the trajectory that place=True fits: pass place=True")
    if not all(isinstance(v, (bool, np.bool_)) for v in (rotations, rotations_continuous, return_rotations)):
        raise ValueError("rotations, rotations_continuous and return_rotations are switches (True / False)")
    if not rotations and (return_rotations or not rotations_continuous):
        raise ValueError("rotations_continuous and return_rotations describe the joint rotations: pass rotations=True")
    if rotations and keep_padding:
        raise ValueError("rotations with keep_padding=True: padded frames repeat the last frame and would enter the sign-continuous tracks")
    for name, r in (("smooth_poses", smooth_poses), ("smooth_traj", smooth_traj)):
        if not _is_radius(r, 0):
            raise ValueError(f"{name} is a radius in frames, an integer in 0..{SMOOTH_MAXR} (0: off), got {r!r}")
    smoothing = int(smooth_poses) > 0 or int(smooth_traj) > 0
    if not smoothing and (smooth_degree != 2 or smooth_taper != "uniform"):
        raise ValueError("smooth_degree and smooth_taper describe smoothing: pass smooth_poses or smooth_traj (a radius > 0)")
    if smoothing:
        _smooth_options(max(int(smooth_poses), int(smooth_traj)), smooth_degree, smooth_taper)
    if int(smooth_traj) > 0 and not place:
        raise ValueError("smooth_traj smooths the trajectory that place=True fits: pass place=True")
    if smoothing and keep_padding:
        raise ValueError("smooth_poses / smooth_traj with keep_padding=True: padded frames repeat the last frame and would enter the fits")
    if agg == "path":
        _path_options(path_sigma, path_switch, ("path_sigma", "path_switch"))
        if tta:
            raise ValueError("agg='path' with tta=True: the path runs through the hypotheses of the un-mirrored pass, and head k of a mirrored input "
                             "is not head k of the plain one, so the mirrored pass has nothing to add to them: pass tta=False")
        if keep_padding:
            raise ValueError("agg='path' with keep_padding=True: padded frames repeat the last frame and would enter the path")
    elif return_path or isinstance(path_sigma, bool) or isinstance(path_switch, bool) or path_sigma != PATH_SIGMA or path_switch != PATH_SWITCH:
        raise ValueError("path_sigma, path_switch and return_path describe the hypothesis path: pass agg='path'")
    single = torch.is_tensor(poses_2d) or isinstance(poses_2d, np.ndarray)
    seqs = [poses_2d] if single else list(poses_2d)
    if return_score and targets is None:
        raise ValueError("return_score returns the score against ground truth: pass targets (one (N, J, 3) array per sequence)")
    if targets is not None:
        if keep_padding:
            raise ValueError("targets with keep_padding=True: padded frames have no ground truth of their own")
        targets = [targets] if torch.is_tensor(targets) or isinstance(targets, np.ndarray) else list(targets)
        if len(targets) != len(seqs):
            raise ValueError(f"targets: {len(targets)} arrays for {len(seqs)} sequences")
        for i, (t, q) in enumerate(zip(targets, seqs)):
            h = t if torch.is_tensor(t) else np.asarray(t)                   # (a device tensor stays where it is: only its shape is looked at)
            numbers = (h.dtype.is_floating_point or h.dtype in (torch.int32, torch.int64)) if torch.is_tensor(t) else h.dtype.kind in "fiu"
            want = (int(q.shape[0]), int(q.shape[1]), 3) if getattr(q, "ndim", 0) == 3 else None
            if not numbers or want is None or tuple(h.shape) != want:
                raise ValueError(f"targets[{i}] must be {want if want else '(N, J, 3)'} numbers like its sequence, got shape {tuple(h.shape)} {h.dtype}")
            targets[i] = h
    opt = _Options(seqs, tta, agg, blend, scale, bool(return_hyps), keep_padding, rigid, symmetric, bool(return_bones), place, world, floor,
                   bool(return_place), int(smooth_poses), int(smooth_traj), int(smooth_degree), smooth_taper, float(path_sigma), float(path_switch),
                   bool(return_path), targets=targets, return_score=bool(return_score), place_refine=int(place_refine), rotations=bool(rotations),
                   rotations_continuous=bool(rotations_continuous), return_rotations=bool(return_rotations))
    if not seqs:
        return opt
    cam_tables = None
    if place or world:
        cam_tables = camera_table(cameras)
        if cam_tables[0].shape[0] != len(seqs):
            raise ValueError(f"cameras: {cam_tables[0].shape[0]} cameras for {len(seqs)} sequences")
    T, J, K = _model_shape(model)
    if agg == "path" and not 2 <= K <= PATH_MAXK:
        raise ValueError(f"agg='path' chooses among a model's hypotheses: this model has {K} (2..{PATH_MAXK} expected)")
    table = sk = parents = None
    if rigid:
        mixste = getattr(model, "_arch", None) == "mixste"
        if lengths is None:
            lengths = "measured" if mixste else "model"
        if isinstance(lengths, str):
            if lengths not in ("model", "measured"):
                raise ValueError(f"lengths must be None, 'model', 'measured' or a table, got {lengths!r}")
            if lengths == "model" and mixste:
                raise ValueError("lengths='model': MixSTE predicts no bone lengths; use 'measured' or pass a table")
        else:
            table, lengths = _host_f32(lengths, (len(seqs), J - 1), "lengths", row=(J - 1,), nonneg=True), "table"
        sk = _skeleton_of(model)
        parents = _parents_c(sk, J)
    rot_tables = None
    if rotations:                                    # the tree and the T-pose the model decodes with (MixSTE carries none: the H36M ones)
        rot_sk = _skeleton_of(model)
        rot_tables = (_parents_c(rot_sk, J), _rest_c(rot_sk, J))
    stride = T if stride is None else int(stride)
    if (agg not in AGG and agg != "path") or blend not in BLEND:
        raise ValueError(f"agg in {sorted(AGG) + ['path']} and blend in {sorted(BLEND)} expected, got {agg!r}, {blend!r}")
    if keep_padding and stride != T:
        raise ValueError("keep_padding describes the reference's non-overlapping windows: stride must be T")
    for s in seqs:
        if s.ndim != 3 or s.shape[1] != J or s.shape[2] != 2:
            raise ValueError(f"every sequence must be (N, {J}, 2), got {tuple(s.shape)}")
    windows = plan_windows([int(s.shape[0]) for s in seqs], T, stride)       # (its own ValueErrors: the stride, a sequence without frames)
    params = list(model.parameters())
    if not params or not params[0].is_cuda:
        raise RuntimeError("manipose_amd: lift_sequences needs the model on a ROCm device; there is no CPU fallback")
    for s in seqs:
        if torch.is_tensor(s) and not s.is_cuda:
            raise RuntimeError("manipose_amd: lift_sequences takes device tensors or numpy arrays (got a CPU tensor); there is no CPU fallback")
    if batch is None:
        batch = (int(getattr(model, "max_batch_hint", 0)) // (2 if tta else 1)) or 16
    return opt._replace(cam_tables=cam_tables, T=T, J=J, K=K, lengths=lengths, table=table, skeleton=sk, parents=parents, rot_tables=rot_tables,
                        windows=windows, batch=max(1, int(batch)), dev=params[0].device)


def _upload(model, opt):
    """The 2-D keypoints, the window tables and the offsets of all sequences go to the device once, up front; the output buffers are allocated."""
    dev, T, J, seqs = opt.dev, opt.T, opt.J, opt.seqs
    lens = [int(s.shape[0]) for s in seqs]
    win_seq, win_start = opt.windows
    first = np.concatenate([[0], np.cumsum(np.bincount(win_seq, minlength=len(lens)))]).astype(np.int64)     # first window of every sequence
    if all(torch.is_tensor(s) for s in seqs):
        p2 = torch.cat([s.to(dev, torch.float32) for s in seqs], dim=0).contiguous()
    else:
        host = [s.detach().cpu().numpy() if torch.is_tensor(s) else np.asarray(s) for s in seqs]
        p2 = torch.from_numpy(np.concatenate([h.astype(np.float32, copy=False) for h in host], axis=0)).to(dev).contiguous()
    off = np.zeros(len(lens) + 1, dtype=np.int64)
    off[1:] = np.cumsum(lens)
    out_lens = [int(first[s + 1] - first[s]) * T if opt.keep_padding else lens[s] for s in range(len(lens))]
    out_off = np.zeros(len(lens) + 1, dtype=np.int64)
    out_off[1:] = np.cumsum(out_lens)
    merge_off = np.zeros((len(lens), 2), dtype=np.int64)
    merge_off[:, 1] = out_lens
    d_off, d_merge_off = torch.from_numpy(off).to(dev), torch.from_numpy(merge_off).to(dev)
    d_seq, d_start = torch.from_numpy(win_seq).to(dev), torch.from_numpy(win_start).to(dev)
    max_nw = int(np.max(first[1:] - first[:-1]))
    d_zero = torch.zeros(max_nw, dtype=torch.int32, device=dev)
    d_flip = torch.ones(opt.batch, dtype=torch.uint8, device=dev)
    mirror = _mirror(model, J)
    bone_mirror = torch.tensor([int(mirror[j]) - 1 for j in range(1, J)], device=dev) if opt.lengths == "model" else None
    out_all = torch.empty(sum(out_lens), J, 3, dtype=torch.float32, device=dev)
    hyp_all = torch.empty(sum(out_lens), opt.K, J, 4, dtype=torch.float32, device=dev) if opt.return_hyps or opt.agg == "path" else None
    return _Plan(p2=p2, lens=lens, out_lens=out_lens, out_off=out_off, first=first, win_start=win_start, merge_off=merge_off,
                 h_zero=np.zeros(max_nw, dtype=np.int32), d_off=d_off, d_merge_off=d_merge_off, d_seq=d_seq, d_start=d_start, d_zero=d_zero,
                 d_flip=d_flip, mirror=mirror, bone_mirror=bone_mirror, out_all=out_all, hyp_all=hyp_all,
                 gt=_upload_targets(opt.targets, dev) if opt.return_score else None)


def _upload_targets(targets, dev):
    if all(torch.is_tensor(t) for t in targets):
        return torch.cat([t.to(dev, torch.float32) for t in targets], dim=0).contiguous()
    host = [t.detach().cpu().numpy() if torch.is_tensor(t) else t for t in targets]
    return torch.from_numpy(np.concatenate([h.astype(np.float32, copy=False) for h in host], axis=0)).to(dev).contiguous()


def _lift_one(model, opt, plan, s, model_rows):
    """Sequence ``s`` on its own: its windows in forwards of ``batch`` (the mirrored copies of a forward's windows follow them, as evaluate()
    batches them; no forward mixes two sequences), every forward's hypotheses staged until all are there, then ONE merge into the sequence's
    rows of ``out_all`` / ``hyp_all``.  ``lengths="model"``: the bone lengths every forward left in the engine are appended to ``model_rows``."""
    lib, dev, T, J, K, tta = _lib.load(), opt.dev, opt.T, opt.J, opt.K, opt.tta
    F = 2 if tta else 1
    a0, nw = int(plan.first[s]), int(plan.first[s + 1] - plan.first[s])
    buf_p = buf_s = None
    for a in range(0, nw, opt.batch):
        n = min(opt.batch, nw - a)
        X = torch.empty(F * n, T, J, 2, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            for h in range(F):
                _lib.check(lib.mp_lift_windows_2d(_lib.ptr(plan.p2), _lib.ptr(plan.d_off), len(plan.lens), _lib.ptr(plan.d_seq[a0 + a:]),
                                                  _lib.ptr(plan.d_start[a0 + a:]), _lib.ptr(plan.d_flip) if h else None, plan.mirror, n, T, J,
                                                  _lib.ptr(X[h * n:]), _lib.stream_ptr()), "mp_lift_windows_2d")
        res = model(X)
        poses, scores = res if isinstance(res, tuple) else (res, None)
        poses = poses.reshape(F * n, K, T, J, 3)
        if opt.lengths == "model":                   # the (F n, J - 1) lengths this forward left in the engine
            lw = model._engine.peek(1).view(F * n, J - 1).abs()
            model_rows.append((lw[:n] + lw[n:][:, plan.bone_mirror]) / 2 if tta else lw)
        if n == nw:                                  # the whole sequence in one forward: merged where the engine left it
            buf_p, buf_s = poses, scores
            break
        if buf_p is None:
            buf_p = torch.empty(F * nw, K, T, J, 3, dtype=torch.float32, device=dev)
            buf_s = torch.empty(F * nw, K, T, 1, dtype=torch.float32, device=dev) if scores is not None else None
        for h in range(F):
            buf_p[h * nw + a:h * nw + a + n] = poses[h * n:(h + 1) * n]
            if scores is not None:
                buf_s[h * nw + a:h * nw + a + n] = scores[h * n:(h + 1) * n]
    o0, o1 = int(plan.out_off[s]), int(plan.out_off[s + 1])
    hyps_on = plan.hyp_all is not None               # asked for, or what agg="path" chooses from (the merged poses are then replaced: _path_stage)
    merge_windows(buf_p, buf_s, plan.h_zero[:nw], plan.win_start[a0:a0 + nw], plan.merge_off[s], T=T, tta=tta, mirror=plan.mirror,
                  agg="weighted_ave" if opt.agg == "path" else opt.agg, blend=opt.blend, scale=opt.scale, return_hyps=hyps_on, out=plan.out_all[o0:o1],
                  hyps=plan.hyp_all[o0:o1] if hyps_on else None,
                  device_tables=(plan.d_zero[:nw], plan.d_start[a0:a0 + nw], plan.d_merge_off[s]))


def _path_stage(opt, plan):
    """``agg="path"``: ONE call chooses every sequence's path through its merged hypotheses (``path_sigma`` is in metres, the hypotheses in the
    poses' unit); the selected poses replace the merged ones, and the hypotheses stay in the plan only if they were asked for.  Returns the plan
    and the (path (Ntot,), cost (S,)) of all sequences.  (No padded frames here: ``d_off`` describes ``hyp_all``.)"""
    out, path, cost = _path(_lib.load(), plan.hyp_all, plan.d_off, len(plan.lens), opt.path_sigma * float(opt.scale), opt.path_switch)
    return plan._replace(out_all=out, hyp_all=plan.hyp_all if opt.return_hyps else None), (path, cost)


def _smooth_poses_stage(opt, plan):
    """The merged poses and, with ``return_hyps``, the hypotheses (hypothesis k is a track over time; its scores are untouched) smoothed along
    the frames of their sequence; every frame is valid.  ``mp_lift_smooth`` is out of place: returns the plan with the new buffers.  (No padded
    frames here: ``d_off`` describes ``out_all``.)"""
    lib, S, args = _lib.load(), len(plan.lens), (opt.smooth_poses, opt.smooth_degree, opt.smooth_taper)
    out = _smooth(lib, plan.out_all.unsqueeze(1), None, plan.d_off, S, *args)[0][:, 0]
    hyps = _smooth(lib, plan.hyp_all, None, plan.d_off, S, *args)[0] if opt.return_hyps else None
    return plan._replace(out_all=out, hyp_all=hyps)


def _smooth_traj_stage(opt, plan, placed):
    """The fitted trajectories of the merged poses and of the hypotheses smoothed along the frames of their sequence with the fit's ``ok`` as
    validity: ``traj`` / ``hyps_traj`` become the smoothed ones (which the world stage uses), the fitted ones stay as ``traj_fit`` /
    ``hyps_traj_fit``, and ``filled`` / ``hyps_filled`` say where a value could be given; ``ok`` and ``reproj`` stay what the fit reported."""
    lib, S, ntot = _lib.load(), len(plan.lens), int(plan.out_all.shape[0])
    for pre in ("", "hyps_") if opt.return_hyps else ("",):
        fit, ok = placed[pre + "traj"], placed[pre + "ok"]
        out, filled = _smooth(lib, fit.view(ntot, -1, 1, 3), ok.view(ntot, -1), plan.d_off, S, opt.smooth_traj, opt.smooth_degree, opt.smooth_taper,
                              want_filled=True)
        placed[pre + "traj_fit"], placed[pre + "traj"], placed[pre + "filled"] = fit, out.view(fit.shape), filled.view(ok.shape)


def _reproj_smooth_stage(opt, plan, placed, d_intr):
    """``place_refine`` with ``smooth_traj``: the reprojection error of the smoothed trajectories over their ``filled`` frames, under the full camera
    model (``reproj`` stays the error at the fitted translation): ``reproj_smooth`` / ``hyps_reproj_smooth``, 0 where nothing was filled in."""
    lib, S, ntot = _lib.load(), len(plan.lens), int(plan.out_all.shape[0])
    for pre, p4 in (("", plan.out_all.unsqueeze(1)), ("hyps_", plan.hyp_all)) if opt.return_hyps else (("", plan.out_all.unsqueeze(1)),):
        traj, filled = placed[pre + "traj"], placed[pre + "filled"]
        err = _place_refine(lib, p4, plan.p2, plan.d_off, S, d_intr, None, True, 0, traj.contiguous().view(ntot, -1, 3),
                            filled.contiguous().view(ntot, -1))[1]
        placed[pre + "reproj_smooth"] = err.view(filled.shape)


def _rigid_stage(opt, plan, model_rows):
    """One (J - 1) table of bone lengths per sequence, and every merged pose and hypothesis re-assembled with it, in place.  Returns the
    (S, J - 1) tables in metres."""
    dev, S, sk, scale = opt.dev, len(plan.lens), opt.skeleton, float(opt.scale)
    d_out_off = torch.from_numpy(plan.out_off).to(dev)
    if opt.lengths == "model":                       # plain mean over each sequence's windows, in window order
        rows = torch.cat(model_rows, dim=0)
        bones = torch.stack([rows[int(plan.first[s]):int(plan.first[s + 1])].mean(dim=0) for s in range(S)])
    elif opt.lengths == "measured":                  # of the merged poses, which mp_lift_merge has already multiplied by scale
        bones = bone_length_means(plan.out_all, d_out_off, real_frames=np.asarray(plan.lens, dtype=np.int64) if opt.keep_padding else None, skeleton=sk)
        if scale != 1.0:
            bones = bones / scale
    else:
        bones = torch.from_numpy(opt.table).to(dev)
    if opt.symmetric:
        bl, br = list(sk.bones_left), list(sk.bones_right)
        mean = (bones[:, bl] + bones[:, br]) / 2
        bones = bones.clone()
        bones[:, bl] = mean
        bones[:, br] = mean
    used = (bones * scale).contiguous()
    _rigid(_lib.load(), plan.out_all.unsqueeze(1), d_out_off, S, used, opt.parents)
    if opt.return_hyps:
        _rigid(_lib.load(), plan.hyp_all, d_out_off, S, used, opt.parents)
    return bones


def _score_stage(opt, plan, model):
    """The emitted poses and, with ``return_hyps``, every hypothesis against the targets with joint 0 zeroed (the poses are root-relative; joint 0 of
    a target holds the root's position), ``pred_scale = 1 / scale``: every number in metres.  After the rigid stage and before placing: what follows
    moves a pose rigidly, so the score is that of the placed pose and of the world frame's too.  Returns the dict of PoseScore fields of all
    sequences ((S,) tensors; under "hyps" the same of the hypotheses, (S, K), and "oracle_mpjpe" (S,): the mean over the frames with a counted
    hypothesis of min_k frame_err - plain torch on the device).  (No padded frames here: ``d_off`` describes ``out_all``.)"""
    lib, S, J, inv = _lib.load(), len(plan.lens), opt.J, 1.0 / float(opt.scale)
    parents = _parents_c(_skeleton_of(model), J)
    gt = plan.gt.clone()
    gt[:, 0] = 0.0
    flags = SCORE_PROCRUSTES
    rec = _pose_record(_score(lib, plan.out_all.unsqueeze(1), gt, None, plan.d_off, S, parents, inv, 1.0, flags)[0][:, 0], J, True, True)
    score = {f: getattr(rec, f) for f in SCORE_FIELDS}
    if opt.return_hyps:
        rows, fe = _score(lib, plan.hyp_all, gt, None, plan.d_off, S, parents, inv, 1.0, flags, want_frames=True)
        hrec = _pose_record(rows, J, True, True)
        score["hyps"] = {f: getattr(hrec, f) for f in SCORE_FIELDS}
        best = torch.where(fe >= 0, fe.double(), torch.full_like(fe, float("inf"), dtype=torch.float64)).min(dim=1).values
        seen = torch.isfinite(best)
        per = [(b[m].mean() if bool(m.any()) else b.new_full((), float("nan"))) for b, m in zip(torch.split(best, plan.out_lens), torch.split(seen, plan.out_lens))]
        score["oracle_mpjpe"] = torch.stack(per)
    return score


def _score_traj_stage(opt, plan, placed, score):
    """The trajectory the world stage uses (smoothed with ``smooth_traj``) against the targets' joint 0, in metres; a frame counts where the fit was
    ``ok`` or, smoothed, where a value could be ``filled`` in."""
    valid = placed["filled"] if opt.smooth_traj else placed["ok"]
    ntot = int(plan.out_all.shape[0])
    rows = _score(_lib.load(), placed["traj"].contiguous().view(ntot, 1, 1, 3), plan.gt[:, :1].contiguous(), valid.contiguous().view(ntot, 1), plan.d_off,
                  len(plan.lens), None, 1.0 / float(opt.scale), 1.0, 0)[0][:, 0]
    score["traj"] = dict(_traj_record(rows)._asdict())


def _place_stage(opt, plan, score=None):
    """The root trajectories of the merged poses and the hypotheses (``place``), then both into the world frame, in place, the hypotheses on
    the merged poses' floor (``world``).  No padded frames here: a frame of ``out_all`` is the frame of ``p2`` with the same number.  Returns
    the dict of per-frame results and the (S,) floor offsets or None."""
    lib, dev, S, out4 = _lib.load(), opt.dev, len(plan.lens), plan.out_all.unsqueeze(1)
    d_intr, d_quat = torch.from_numpy(opt.cam_tables[0]).to(dev), torch.from_numpy(opt.cam_tables[1]).to(dev)
    d_trans = torch.from_numpy(opt.cam_tables[2] * np.float32(opt.scale)).to(dev) if opt.place else None
    placed, d_floor = {}, None
    if opt.place:
        keys = ("traj", "reproj", "ok", "steps") if opt.place_refine else ("traj", "reproj", "ok")      # (zip stops at the keys: no steps without refine)
        fit = lambda p4: _place_refine(lib, p4, plan.p2, plan.d_off, S, d_intr, None, True, opt.place_refine)     # the linear fit, then Gauss-Newton steps
        placed.update((k, t[:, 0]) for k, t in zip(keys, fit(out4)))
        if opt.return_hyps:
            placed.update(("hyps_" + k, t) for k, t in zip(keys, fit(plan.hyp_all)))
        if opt.smooth_traj:
            _smooth_traj_stage(opt, plan, placed)
            if opt.place_refine:
                _reproj_smooth_stage(opt, plan, placed, d_intr)
        if score is not None:
            _score_traj_stage(opt, plan, placed, score)
    if opt.world:
        d_floor = torch.empty(S, dtype=torch.float32, device=dev) if opt.floor else None
        _world(lib, out4, placed["traj"].unsqueeze(1).contiguous() if opt.place else None, plan.d_off, S, d_quat, d_trans, 1 if opt.floor else 0,
               d_floor)
        if opt.return_hyps:
            _world(lib, plan.hyp_all, placed.get("hyps_traj"), plan.d_off, S, d_quat, d_trans, 2 if opt.floor else 0, d_floor)
    return placed, d_floor


def _rotations_stage(opt, plan):
    """The joint rotations of the poses AS EMITTED - after path, smoothing, rigid and place / world, so with ``frame="world"`` the root quaternion is
    in the world frame; local rotations do not care - and, with ``return_hyps``, of every hypothesis: the dict quat (Ntot, J, 4), ok (Ntot,) and
    hyps_quat (Ntot, K, J, 4), hyps_ok (Ntot, K) of all sequences.  The poses are read only.  (No padded frames here: ``d_off`` describes
    ``out_all``.)"""
    lib, S, (parents, rest) = _lib.load(), len(plan.lens), opt.rot_tables
    quat, ok, _ = _rotations(lib, plan.out_all.unsqueeze(1), plan.d_off, S, parents, rest, opt.rotations_continuous)
    rot = {"quat": quat[:, 0], "ok": ok[:, 0]}
    if opt.return_hyps:
        rot["hyps_quat"], rot["hyps_ok"], _ = _rotations(lib, plan.hyp_all, plan.d_off, S, parents, rest, opt.rotations_continuous)
    return rot


def _cut_score(score, s):
    return {k: (_cut_score(v, s) if isinstance(v, dict) else v[s]) for k, v in score.items()}


def _per_sequence(opt, plan, bones, placed, d_floor, chosen=None, score=None, rot=None):
    """the buffers of all sequences cut into the per-sequence lists of ``_Lifted``"""
    info = None
    if opt.return_place:
        per_seq = {k: torch.split(v, plan.out_lens, dim=0) for k, v in placed.items()}
        info = [dict({k: v[i] for k, v in per_seq.items()}, **({"floor": d_floor[i]} if opt.floor else {})) for i in range(len(plan.lens))]
    turns = None
    if opt.return_rotations:
        per_seq = {k: torch.split(v, plan.out_lens, dim=0) for k, v in rot.items()}
        turns = [{k: v[i] for k, v in per_seq.items()} for i in range(len(plan.lens))]
    return _Lifted(list(torch.split(plan.out_all, plan.out_lens, dim=0)),
                   list(torch.split(plan.hyp_all, plan.out_lens, dim=0)) if opt.return_hyps else None,
                   list(bones.unbind(0)) if opt.return_bones else None, info,
                   list(zip(torch.split(chosen[0], plan.out_lens, dim=0), chosen[1].unbind(0))) if opt.return_path else None,
                   [_cut_score(score, s) for s in range(len(plan.lens))] if opt.return_score else None, turns)


@torch.no_grad()
def _lift_sequences(model, poses_2d, **options):
    """``lift_sequences`` with its results by name (``_Lifted``): check options -> upload -> every sequence lifted on its own ->
    hypothesis path -> smoothed poses -> rigid stage -> score -> place (-> smoothed trajectories -> their score) / world / floor stage -> joint rotations -> per-sequence lists."""
    opt = _check_options(model, poses_2d, **options)
    if not opt.seqs:
        return _Lifted([], *([] if wanted else None for wanted in (opt.return_hyps, opt.return_bones, opt.return_place, opt.return_path,
                                                                   opt.return_score, opt.return_rotations)))
    plan = _upload(model, opt)
    model_rows = []
    was_training = model.training
    model.eval()
    try:
        for s in range(len(plan.lens)):
            _lift_one(model, opt, plan, s, model_rows)
    finally:
        model.train(was_training)
    chosen = None
    if opt.agg == "path":
        plan, chosen = _path_stage(opt, plan)
    if opt.smooth_poses:
        plan = _smooth_poses_stage(opt, plan)
    bones = _rigid_stage(opt, plan, model_rows) if opt.rigid else None
    score = _score_stage(opt, plan, model) if opt.return_score else None
    placed, d_floor = _place_stage(opt, plan, score) if opt.place or opt.world else (None, None)
    rot = _rotations_stage(opt, plan) if opt.rotations else None
    return _per_sequence(opt, plan, bones, placed, d_floor, chosen, score, rot)


def lift_sequences(model, poses_2d, *, stride=None, tta=True, agg="weighted_ave", blend="mean", return_hyps=False, batch=None, scale=1.0,
                   keep_padding=False, rigid=False, lengths=None, symmetric=False, return_bones=False, cameras=None, place=False, frame="camera",
                   floor=False, return_place=False, smooth_poses=0, smooth_traj=0, smooth_degree=2, smooth_taper="uniform", path_sigma=PATH_SIGMA,
                   path_switch=PATH_SWITCH, return_path=False, targets=None, return_score=False, place_refine=0, rotations=False,
                   rotations_continuous=True, return_rotations=False):
    """One 3-D pose per frame of every sequence.  ``poses_2d``: a list of (N_i, 17, 2) device tensors or numpy arrays (or one such
    array); returns a list of (N_i, 17, 3) device tensors, and with ``return_hyps`` also a list of (N_i, K, 17, 4) (every hypothesis
    and its score, from the un-mirrored pass).  ``stride`` (default T: non-overlapping windows) in 1..T; ``blend`` "mean" averages the
    windows that cover a frame, "center" takes the one whose centre is nearest; ``batch`` windows per forward (``2 * batch`` with
    TTA; default: the model's ``max_batch_hint`` or 16).  ``keep_padding`` (stride == T only) also returns the replicate-padded
    frames of the last window, as the reference's lift_action does.

    ``rigid`` (default off: nothing changes by a bit): every sequence is re-assembled with ONE table of J - 1 bone lengths - each emitted pose and,
    with ``return_hyps``, each hypothesis keeps its root and its bone directions (``project_rigid``).  ``lengths``: "model" = the mean over the
    sequence's windows of the lengths the model predicted (with TTA the mirrored copy's, left and right swapped back, averaged in), the
    default of the two manifold models; "measured" = the mean bone lengths of the sequence's merged poses over its real frames, the default of
    MixSTE, which predicts none; or an (S, J - 1) / (J - 1,) table in metres.  ``symmetric`` replaces every left / right pair of the table
    by its mean.  ``return_bones`` appends the list of (J - 1,) tables used, in metres (``scale`` multiplies poses and lengths alike).

    Placing (all off by default: nothing changes by a bit), after the merge and the rigid stage.  ``cameras``: one camera per sequence
    (``camera_table``).  ``place``: ``mp_lift_place`` fits the root translation of every merged pose and, with ``return_hyps``, of every
    hypothesis (each its own) to the sequence's 2-D keypoints; ``return_place`` appends a list of per-sequence dicts ``traj`` (N, 3), ``reproj``
    (N,), ``ok`` (N,) uint8 and with hypotheses ``hyps_traj`` (N, K, 3), ``hyps_reproj`` (N, K), ``hyps_ok`` (N, K) - and ``floor`` (a scalar)
    when ``floor`` is on, the only key without ``place``; the results come in the order poses, hyps, bones, place.  ``frame="world"``:
    ``mp_lift_world`` rotates the merged poses and the hypotheses by the camera's orientation; with ``place`` their trajectories are added
    first and the camera's translation (times ``scale``, so ``traj`` and the world poses are in the poses' unit) afterwards, without it the
    rotation alone (the reference's prepare_prediction_for_viz before its floor line).  ``floor`` (needs ``frame="world"``): every sequence's
    lowest merged joint is put on z = 0, and the SAME offset is subtracted from the hypotheses - merged pose and hypotheses stand in one scene
    (the reference floors each array on its own).  Not with ``keep_padding``: padded frames have no keypoints of their own.

    Refining the placement (``place_refine=0``, the default: nothing changes by a bit, and no dict gains a key; needs ``place``): an integer in
    0..16, the undamped Gauss-Newton steps ``mp_lift_place_refine`` takes from the linear fit on the reprojection error of the FULL camera model
    (``place_poses(refine=)`` has the rule), for the merged poses and, with ``return_hyps``, for every hypothesis.  ``traj`` / ``hyps_traj`` are then
    the refined trajectories - which ``smooth_traj``, the score's ``traj`` and the world frame use unchanged - ``reproj`` the error at them, and the
    place dicts gain ``steps`` / ``hyps_steps`` (uint8: steps taken); with ``smooth_traj`` also ``reproj_smooth`` / ``hyps_reproj_smooth``, the
    reprojection error of the smoothed trajectory where ``filled`` is 1 (0 elsewhere).  Three steps suffice on the H36M cameras.

    Smoothing in time (both off by default: nothing changes by a bit): ``smooth_poses`` and ``smooth_traj`` are radii in frames, 0..64, 0 = off;
    ``smooth_degree`` (0..2) and ``smooth_taper`` ("uniform" | "biweight") are shared by both and need one of them (``smooth_poses()`` has the
    rule: a least-squares polynomial over the frames within the radius, inside the sequence).  ``smooth_poses``: the merged poses and, with
    ``return_hyps``, every hypothesis as a track over time (scores untouched) are smoothed after the merge and BEFORE the rigid stage, so bone
    lengths stay constant and placing fits the poses that are emitted.  ``smooth_traj`` (needs ``place``): the fitted trajectories are smoothed
    after the fit and before the world frame, with the fit's ``ok`` as validity: a frame with ok = 0 (``traj`` = 0) is filled from its valid
    neighbours.  The place dicts then hold the smoothed ``traj`` / ``hyps_traj`` (what the world frame uses) and gain ``traj_fit`` /
    ``hyps_traj_fit`` (the fitted values, bit for bit) and ``filled`` / ``hyps_filled`` (uint8; 0: no valid frame within the radius, the fitted
    value is kept); ``ok`` and ``reproj`` stay what the fit reported (the reprojection error of the smoothed trajectory comes with ``place_refine``).  Not with
    ``keep_padding``.

    One hypothesis path (``agg="path"``; with the default ``agg`` nothing changes by a bit): instead of averaging the K hypotheses of a frame
    ("weighted_ave": a pose off the model's manifold) or taking every frame's best score on its own ("best_score": jumps from head to head), every
    frame gets exactly ONE of the model's hypotheses, chosen jointly over the sequence (``select_path()`` has the rule: unary cost -log score,
    transition cost mean squared joint step / (2 ``path_sigma``^2) + ``path_switch`` per change of head, cheapest path by the Viterbi algorithm).
    ``path_sigma`` > 0 is in metres (``scale`` multiplies it like the poses; the default 0.02 is not tuned), ``path_switch`` >= 0.  The stage runs
    right after the merge and before ``smooth_poses``: merge -> path -> smooth poses -> rigid -> place -> smooth trajectories -> world, each later
    stage starting from the selected poses (so bone lengths are the model's own until something smooths them).  ``return_path`` appends a list of
    per-sequence ``(path (N,) uint8, cost)`` pairs, cost a float64 scalar tensor; the results come in the order poses, hyps, bones, place, path.
    The hypotheses are those ``return_hyps`` returns (the un-mirrored pass), so ``tta`` must be False: head k of a mirrored input is not head k
    of the plain one.  Needs a model of 2..8 hypotheses; not with ``keep_padding``.

    Scoring against ground truth (``targets=None``, the default: nothing changes by a bit).  ``targets``: one (N_i, J, 3) array per sequence in metres,
    as the dataset's ``fetch()`` prepares them: joint 0 holds the root's position in the camera's frame, the other joints are relative to the root.
    ``return_score`` appends one dict per sequence (the results come in the order poses, hyps, bones, place, path, score): ``score_poses()``'s
    ``frames``, ``mpjpe``, ``rmse``, ``mpjve``, ``accel``, ``p_mpjpe``, ``per_joint`` (J), ``bone_mean``, ``bone_std``, ``bone_err`` (J - 1), float64
    device tensors in metres, of the poses that are emitted - after the path, the smoothing and the rigid stage, before placing, which moves poses
    rigidly - against the targets with joint 0 zeroed (``scale`` is divided out).  With ``return_hyps`` the key ``hyps`` holds the same fields of
    every hypothesis ((K,), (K, J), (K, J - 1)) and ``oracle_mpjpe`` the mean over the frames of the best hypothesis' error.  With ``place`` the key
    ``traj`` holds ``score_traj()``'s ``frames``, ``ate``, ``rmse``, ``velocity``, ``accel`` of the trajectory the world frame uses (smoothed with
    ``smooth_traj``) against the targets' joint 0, over the frames whose fit is ``ok`` (``filled`` when smoothed).  Whether any option lowers these
    numbers on real data has not been measured here.  Not with ``keep_padding``.

    Joint rotations (``rotations=False``, the default: nothing changes by a bit, and no dict gains a key).  ``rotations``: ``mp_lift_rotations``
    (``pose_rotations()`` has the rule) runs LAST, on the poses as they are emitted - after the path, the smoothing, the rigid stage and placing / the
    world frame, so with ``frame="world"`` the root quaternion is in the world frame (local rotations do not care) - and, with ``return_hyps``, on
    every hypothesis; the poses are not modified.  ``return_rotations`` appends one dict per sequence (the results come in the order poses, hyps,
    bones, place, path, score, rotations): ``quat`` (N, J, 4) float32 unit quaternions (w, x, y, z), ``ok`` (N,) uint8, and with hypotheses
    ``hyps_quat`` (N, K, J, 4), ``hyps_ok`` (N, K).  ``rotations_continuous`` (default on) keeps every joint's quaternion track in one hemisphere
    from frame to frame within its sequence.  With ``rigid`` the triple (root trajectory or origin, ``quat``, ``bones``) reproduces the emitted poses
    through the decoder's forward kinematics; without ``rigid`` it reproduces them only with each frame's own measured bone lengths.  The twist about
    a bone is fixed at zero by construction: a convention, not a measurement, and what these rotations are worth on real data has not been measured
    here.  Not with ``keep_padding``."""
    res = _lift_sequences(model, poses_2d, stride=stride, tta=tta, agg=agg, blend=blend, return_hyps=return_hyps, batch=batch, scale=scale,
                          keep_padding=keep_padding, rigid=rigid, lengths=lengths, symmetric=symmetric, return_bones=return_bones, cameras=cameras,
                          place=place, frame=frame, floor=floor, return_place=return_place, smooth_poses=smooth_poses, smooth_traj=smooth_traj,
                          smooth_degree=smooth_degree, smooth_taper=smooth_taper, path_sigma=path_sigma, path_switch=path_switch,
                          return_path=return_path, targets=targets, return_score=return_score, place_refine=place_refine, rotations=rotations,
                          rotations_continuous=rotations_continuous, return_rotations=return_rotations)
    asked = [r for r in res if r is not None]                # in the order poses, hyps, bones, place, path, score, rotations
    return asked[0] if len(asked) == 1 else tuple(asked)


def lift_action(model, poses_2d, config, return_hyps=False) -> np.ndarray:
    """The reference-shaped wrapper (lift_action, hpe/eval_utils.py:226-253): non-overlapping windows, ``config.train.tta``, the padded
    frames of every sequence's last window kept; numpy (windows * T, 17, 3) in metres, or with ``return_hyps`` (multi-hypothesis
    models only, as in the reference) (windows * T, K, 17, 4) with the score in the fourth channel."""
    from .architectures import RMCLManifoldMixSTE
    tta = bool(config.train.tta) if hasattr(config, "train") else bool(config["train"]["tta"])
    hyps = bool(return_hyps) and isinstance(model, RMCLManifoldMixSTE)
    res = _lift_sequences(model, poses_2d, stride=None, tta=tta, return_hyps=hyps, keep_padding=True)
    return torch.cat(res.hyps if hyps else res.poses, dim=0).cpu().numpy()


__all__ = ["plan_windows", "merge_windows", "project_rigid", "bone_length_means", "camera_table", "place_poses", "reproject_poses", "pose_rotations", "to_world", "smooth_poses", "smooth_traj",
           "select_path", "score_poses", "score_traj", "fuse_views", "fuse_views_path", "place_views", "align_views", "bundle_views", "lift_sequences",
           "lift_action"]

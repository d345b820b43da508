"""The argument checks of the lifting bindings (lift_ops.py, lift_views.py, lifting.py, hpe/_entry.py), and nothing else: host code that looks
at types, shapes and dtypes.  Nothing here loads the library, allocates or reads a device tensor's contents.  Predicates (``is_*``) return a bool,
and their callers word the error; everything else raises - a ValueError, but for ``need_device``, the RuntimeError that refuses CPU tensors ("no
CPU fallback") and that an entry point raises after its ValueErrors.  A new entry point composes these and does not write its own."""
from __future__ import annotations

import numpy as np
import torch


def is_number(v):
    """an int or a float, numpy's included; a bool is not a number"""
    return isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, (bool, np.bool_))


def is_int_in(v, lowest, highest):
    """an integer (not a bool) in lowest..highest"""
    return isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_)) and lowest <= int(v) <= highest


def sigma_pair(sigma, other, names):
    """the rule of a (scale, cost) pair, under the callers' names: both numbers, sigma > 0 as the kernel takes it (a float32; +inf is allowed),
    the other finite and >= 0"""
    for v in (sigma, other):
        if not is_number(v):
            raise ValueError(f"{names[0]} and {names[1]} are numbers, got {v!r}")
    if not float(np.float32(sigma)) > 0:
        raise ValueError(f"{names[0]} must be > 0 (inf: the step costs nothing), got {sigma!r}")
    if not 0 <= float(other) <= float(np.finfo(np.float32).max):
        raise ValueError(f"{names[1]} must be finite and >= 0, got {other!r}")


def _got(t):
    return (tuple(t.shape), t.dtype) if torch.is_tensor(t) else type(t).__name__


def mask(m, shape, name, bare=False):
    """m is None or a uint8 tensor of ``shape``; ``bare``: what is no tensor at all is refused without saying what it is"""
    if m is None:
        return
    if bare and not torch.is_tensor(m):
        raise ValueError(f"{name} must be a uint8 tensor of shape {tuple(shape)}")
    if not torch.is_tensor(m) or tuple(m.shape) != tuple(shape) or m.dtype != torch.uint8:
        raise ValueError(f"{name} must be a uint8 tensor of shape {tuple(shape)}, got {_got(m)}")


def f32(t, shape, name, contiguous=False, plain=False):
    """t is a float32 tensor of ``shape``, ``contiguous`` where the kernel reads it as it is.  ``plain``: t is known to be a tensor, and the
    message is the short one"""
    shape = tuple(shape)
    if torch.is_tensor(t) and tuple(t.shape) == shape and t.dtype == torch.float32 and (t.is_contiguous() or not contiguous):
        return
    if plain:
        raise ValueError(f"{name} must be float32 {shape}, got {tuple(t.shape)} {t.dtype}")
    raise ValueError(f"{name} must be a {'contiguous ' if contiguous else ''}float32 tensor {shape}, got {_got(t)}")


def _count(name, n, noun, lowest, highest):
    if not lowest <= n <= highest:
        raise ValueError(f"{name} have {n} {noun}: {lowest}..{highest} expected")


def poses4(poses):
    """poses (Ntot, J, 3) or (Ntot, inner, J, 3 | 4), contiguous float32, 2..32 joints -> its 4-D view"""
    p4 = poses.unsqueeze(1) if poses.dim() == 3 else poses
    if p4.dim() != 4 or p4.shape[3] not in (3, 4) or (poses.dim() == 3 and poses.shape[2] != 3) or poses.dtype != torch.float32 \
            or not poses.is_contiguous():
        raise ValueError(f"poses must be contiguous float32 (Ntot, J, 3) or (Ntot, inner, J, 3 | 4), got {tuple(poses.shape)} {poses.dtype}")
    _count("poses", int(p4.shape[2]), "joints", 2, 32)
    return p4


def traj3(traj):
    if traj.dim() not in (2, 3) or traj.shape[-1] != 3 or traj.dtype != torch.float32 or not traj.is_contiguous():
        raise ValueError(f"traj must be contiguous float32 (Ntot, 3) or (Ntot, inner, 3), got {tuple(traj.shape)} {traj.dtype}")


def hyps4(hyps, maxk):
    if hyps.dim() != 4 or hyps.shape[3] != 4 or hyps.dtype != torch.float32 or not hyps.is_contiguous():
        raise ValueError(f"hyps must be contiguous float32 (Ntot, K, J, 4), got {tuple(hyps.shape)} {hyps.dtype}")
    _count("hyps", int(hyps.shape[1]), "hypotheses", 1, maxk)
    _count("hyps", int(hyps.shape[2]), "joints", 2, 32)


def hyps5(hyps, maxv, maxk):
    if hyps.dim() != 5 or hyps.shape[4] not in (3, 4) or hyps.dtype != torch.float32 or not hyps.is_contiguous():
        raise ValueError(f"hyps must be contiguous float32 (V, Ftot, K, J, 3 | 4), got {tuple(hyps.shape)} {hyps.dtype}")
    _count("hyps", int(hyps.shape[0]), "views", 1, maxv)
    _count("hyps", int(hyps.shape[2]), "hypotheses", 1, maxk)
    _count("hyps", int(hyps.shape[3]), "joints", 2, 32)


def view_poses4(poses, maxv):
    if poses.dim() != 4 or poses.shape[3] not in (3, 4) or poses.dtype != torch.float32 or not poses.is_contiguous():
        raise ValueError(f"poses must be contiguous float32 (V, Ftot, J, 3 | 4), got {tuple(poses.shape)} {poses.dtype}")
    _count("poses", int(poses.shape[0]), "views", 1, maxv)
    _count("poses", int(poses.shape[2]), "joints", 2, 32)


def take_pose_keypoints(pose, keypoints_2d, maxv, root=None):
    """pose (Ftot, J, 3) contiguous float32 with 2..32 joints, root (Ftot, 3) float32 if there is one, and keypoints_2d (V <= maxv, Ftot, J, 2)
    float32, all tensors -> (V, Ftot, J)"""
    if pose.dim() != 3 or pose.shape[2] != 3 or pose.dtype != torch.float32 or not pose.is_contiguous() or not 2 <= int(pose.shape[1]) <= 32:
        raise ValueError(f"pose must be contiguous float32 (Ftot, J, 3) with 2..32 joints, got {tuple(pose.shape)} {pose.dtype}")
    ftot, J, kp = int(pose.shape[0]), int(pose.shape[1]), keypoints_2d
    if root is not None:
        f32(root, (ftot, 3), "root", plain=True)
    if kp.dim() != 4 or not 1 <= int(kp.shape[0]) <= maxv or tuple(kp.shape[1:]) != (ftot, J, 2) or kp.dtype != torch.float32:
        raise ValueError(f"keypoints_2d must be float32 (V <= {maxv}, {ftot}, {J}, 2), got {tuple(kp.shape)} {kp.dtype}")
    return int(kp.shape[0]), ftot, J


def keypoint_weights(kp_weight, shape):
    """kp_weight is None or a float32 tensor (V, Ftot, J), a weight per observation (made contiguous by the caller: any strides)"""
    if kp_weight is not None:
        f32(kp_weight, shape, "kp_weight")


def robust_scale(sigma):
    """sigma is a number > 0 as the kernel takes it (a float32; +inf is allowed), in normalised screen units"""
    if not is_number(sigma) or not float(np.float32(sigma)) > 0:
        raise ValueError(f"sigma must be a number > 0 in normalised screen units (inf: no robust weight), got {sigma!r}")


def prior_weight(prior):
    """prior is a finite number >= 0 (a float32)"""
    if not is_number(prior) or not 0 <= float(prior) <= float(np.finfo(np.float32).max):
        raise ValueError(f"prior must be a finite number >= 0 (0: no pull towards the fused pose), got {prior!r}")


def prior_pull(prior):
    """prior is a finite number > 0 as the kernel takes it (a float32): the pull that pins what the keypoints leave free"""
    if not is_number(prior) or not 0 < float(np.float32(prior)) <= float(np.finfo(np.float32).max):
        raise ValueError(f"prior must be a finite number > 0 (the keypoints leave the scale free: without the pull the points drift), got {prior!r}")


def step_count(iters, highest):
    """iters is an integer in 0..highest"""
    if not is_int_in(iters, 0, highest):
        raise ValueError(f"iters counts Gauss-Newton steps, an integer in 0..{highest} (0: the evaluation alone), got {iters!r}")


def smooth_weight(smooth):
    """smooth is a finite number >= 0 (a float32): the weight of a squared second difference"""
    if not is_number(smooth) or not 0 <= float(smooth) <= float(np.finfo(np.float32).max):
        raise ValueError(f"smooth must be a finite number >= 0 (0: every frame fitted on its own), got {smooth!r}")


def sweep_count(sweeps, highest):
    """sweeps is an integer in 0..highest"""
    if not is_int_in(sweeps, 0, highest):
        raise ValueError(f"sweeps counts sweeps over a take's frames, an integer in 0..{highest} (0: every frame fitted on its own), got {sweeps!r}")


def points3(points):
    """points (Ntot, J, 3 | 4) contiguous float32 with 2..32 joints, a tensor -> (Ntot, J)"""
    if not torch.is_tensor(points) or points.dim() != 3 or points.shape[2] not in (3, 4) or points.dtype != torch.float32 or not points.is_contiguous():
        raise ValueError(f"points must be a contiguous float32 tensor (Ntot, J, 3 | 4), got {_got(points)}")
    _count("points", int(points.shape[1]), "joints", 2, 32)
    return int(points.shape[0]), int(points.shape[1])


def ground_joints(feet, axis, J, maxfeet):
    """feet: 1..maxfeet joint indices, axis: two different ones, all integers in 0..J-1 -> (feet, axis) as tuples of int"""
    try:
        feet, axis = tuple(feet), tuple(axis)
    except TypeError:
        raise ValueError(f"feet and axis are sequences of joint indices, got {feet!r}, {axis!r}") from None
    if not 1 <= len(feet) <= maxfeet or not all(is_int_in(j, 0, J - 1) for j in feet):
        raise ValueError(f"feet must be 1..{maxfeet} joint indices in 0..{J - 1}, got {feet!r}")
    if len(axis) != 2 or not all(is_int_in(j, 0, J - 1) for j in axis) or int(axis[0]) == int(axis[1]):
        raise ValueError(f"axis must be two different joint indices in 0..{J - 1} (from, to: up the body), got {axis!r}")
    return tuple(int(j) for j in feet), tuple(int(j) for j in axis)


def ground_options(radius, speed, sigma, prior, iters, foot_height, maxradius, maxiters):
    """the scalars of estimate_ground as the kernel takes them (float32): radius and iters integers in range, speed finite and > 0, sigma > 0 (+inf is
    allowed), prior finite and >= 0, foot_height finite"""
    big = float(np.finfo(np.float32).max)
    if not is_int_in(radius, 1, maxradius):
        raise ValueError(f"radius must be an integer in 1..{maxradius} frames, got {radius!r}")
    if not is_number(speed) or not 0 < float(np.float32(speed)) <= big:
        raise ValueError(f"speed must be a finite number > 0 (the points' unit per frame), got {speed!r}")
    if not is_number(sigma) or not float(np.float32(sigma)) > 0:
        raise ValueError(f"sigma must be a number > 0 in the points' unit (inf: no robust weight), got {sigma!r}")
    if not is_number(prior) or not 0 <= float(prior) <= big:
        raise ValueError(f"prior must be a finite number >= 0 (0: the body axis does not pull the plane), got {prior!r}")
    if not is_int_in(iters, 0, maxiters):
        raise ValueError(f"iters counts re-weighted solves, an integer in 0..{maxiters} (0: the plain fit alone), got {iters!r}")
    if not is_number(foot_height) or not abs(float(foot_height)) <= big:
        raise ValueError(f"foot_height must be a finite number, got {foot_height!r}")


def leg_joints(legs, J, maxfeet):
    """legs: 1..maxfeet triples (hip, knee, ankle) of integers in 0..J-1, no joint named twice -> a tuple of tuples of int"""
    try:
        legs = tuple(tuple(leg) for leg in legs)
    except TypeError:
        raise ValueError(f"legs is a sequence of (hip, knee, ankle) joint indices, got {legs!r}") from None
    if not 1 <= len(legs) <= maxfeet or not all(len(leg) == 3 and all(is_int_in(j, 0, J - 1) for j in leg) for leg in legs):
        raise ValueError(f"legs must be 1..{maxfeet} triples (hip, knee, ankle) of joint indices in 0..{J - 1}, got {legs!r}")
    named = [int(j) for leg in legs for j in leg]
    if len(set(named)) != len(named):
        raise ValueError(f"legs name a joint twice: a leg is three different joints, and no two legs share one, got {legs!r}")
    return tuple(tuple(int(j) for j in leg) for leg in legs)


def footlock_options(blend, stretch, maxblend):
    """the scalars of lock_feet as the kernel takes them: blend an integer in 0..maxblend frames, stretch a float32 in (0, 1]"""
    if not is_int_in(blend, 0, maxblend):
        raise ValueError(f"blend counts the frames of the ease into and out of a stance run, an integer in 0..{maxblend}, got {blend!r}")
    if not is_number(stretch) or not 0 < float(np.float32(stretch)) <= 1:
        raise ValueError(f"stretch is the share of thigh + shank a leg may reach, a number in (0, 1], got {stretch!r}")


def quats4(quat):
    """quat (Ntot, J, 4) or (Ntot, inner, J, 4), contiguous float32, 2..32 joints, at least one frame -> its 4-D view"""
    if not torch.is_tensor(quat) or quat.dim() not in (3, 4) or quat.shape[-1] != 4 or quat.dtype != torch.float32 or not quat.is_contiguous():
        raise ValueError(f"quat must be a contiguous float32 tensor (Ntot, J, 4) or (Ntot, inner, J, 4), got {_got(quat)}")
    _count("quat", int(quat.shape[-2]), "joints", 2, 32)
    if int(quat.shape[0]) < 1 or (quat.dim() == 4 and int(quat.shape[1]) < 1):
        raise ValueError(f"quat holds no frame, got {tuple(quat.shape)}")
    return quat.unsqueeze(1) if quat.dim() == 3 else quat


def retime_options(fps_in, fps_out, radius, degree, taper, maxradius, tapers):
    """the scalars of retime_rotations as the kernel takes them: both rates integers in 1..2^20 (frames times a rate stay exact in a float64),
    radius an integer in 0..maxradius (0: interpolation), degree 0..2, taper one of ``tapers``"""
    for name, v in (("fps_in", fps_in), ("fps_out", fps_out)):
        if not is_int_in(v, 1, 1 << 20):
            raise ValueError(f"{name} is a frame rate, an integer in 1..{1 << 20}, got {v!r}")
    if not is_int_in(radius, 0, maxradius):
        raise ValueError(f"radius must be an integer in 0..{maxradius} (0: interpolation between the two frames around a sample), got {radius!r}")
    if not is_int_in(degree, 0, 2):
        raise ValueError(f"degree must be 0, 1 or 2, got {degree!r}")
    if taper not in tapers:
        raise ValueError(f"taper must be one of {sorted(tapers)}, got {taper!r}")


def retime_plan(seq_offset, ntot, fps_in, fps_out, start):
    """The output frames of a retimed take, from HOST numbers alone.  ``seq_offset`` (S + 1) first input frames (None: one sequence of ``ntot``),
    not decreasing inside 0..ntot, no sequence empty; ``start`` one number or S of them, finite and >= 0, in input frames.  Output frame h of a
    sequence of n frames samples it at t = start + (h * fps_in) / fps_out - in float64 the product is exact and there is one division, the
    kernel's expression - and the sequence gets the M frames with t <= n - 1: for start = 0 in integers, M = ((n - 1) * fps_out) // fps_in + 1.
    Returns (in_offset (S + 1) int64, out_offset (S + 1) int64, clock (S, 3) float64 rows (start, fps_out, fps_in), time (Mtot,) float64)."""
    off = np.asarray([0, ntot] if seq_offset is None else seq_offset)
    if off.ndim != 1 or off.size < 2 or off.dtype.kind not in "iu":
        raise ValueError(f"seq_offset must hold S + 1 >= 2 integer frame numbers, got shape {off.shape} {off.dtype}")
    off = off.astype(np.int64)
    S = off.size - 1
    if off[0] < 0 or off[-1] > ntot or (np.diff(off) < 1).any():
        raise ValueError(f"seq_offset must increase inside 0..{ntot} (no sequence is empty), got {off.tolist()}")
    st = np.asarray(start, dtype=np.float64) if is_number(start) or isinstance(start, (list, tuple, np.ndarray)) else None
    if st is None or st.shape not in ((), (S,)) or not np.isfinite(st).all() or (st < 0).any():
        raise ValueError(f"start is the first sample in input frames, one finite number >= 0 or one per sequence ({S}), got {start!r}")
    st = np.broadcast_to(st, (S,)).astype(np.float64)
    num, den = float(fps_out), float(fps_in)
    counts, times = [], []
    for s in range(S):
        n = int(off[s + 1] - off[s])
        if st[s] > n - 1:
            raise ValueError(f"start = {st[s]!r} lies past the last frame of sequence {s} ({n} frames)")
        at = lambda h: st[s] + (float(h) * den) / num
        M = ((n - 1) * int(fps_out)) // int(fps_in) + 1 if st[s] == 0 else int(np.floor((n - 1 - st[s]) * num / den)) + 1
        while M > 1 and at(M - 1) > n - 1:
            M -= 1
        while at(M) <= n - 1:
            M += 1
        counts.append(M)
        times.append(st[s] + (np.arange(M, dtype=np.float64) * den) / num)
    out_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    clock = np.stack([st, np.full(S, num), np.full(S, den)], axis=1)
    return off, out_off, np.ascontiguousarray(clock), np.concatenate(times)


def euler_options(order, scale, orders):
    """the scalars of euler_from_rotations as the kernel takes them: order one of ``orders`` (the six channel orders), scale a number whose
    float32 is finite and > 0"""
    if not isinstance(order, str) or order not in orders:
        raise ValueError(f"order must be one of {list(orders)} (the rotation channels, first to last), got {order!r}")
    if not is_number(scale) or not 0 < float(np.float32(scale)) <= float(np.finfo(np.float32).max):
        raise ValueError(f"scale is the unit of the positions, a finite number > 0 (100: centimetres), got {scale!r}")


def floor_record(ground, S):
    """ground is None or carries ``normal`` (S, 3) float32, ``offset`` (S) float32 and ``ok`` (S) uint8 tensors (a ``Ground``) -> those three or None"""
    if ground is None:
        return None
    try:
        normal, offset, ok = ground.normal, ground.offset, ground.ok
    except AttributeError:
        raise ValueError(f"ground must be None or a Ground record (normal, offset, ok), got {type(ground).__name__}") from None
    f32(normal, (S, 3), "ground.normal")
    f32(offset, (S,), "ground.offset")
    if ok is None:
        raise ValueError(f"ground.ok must be a uint8 tensor of shape {(S,)}, got None")
    mask(ok, (S,), "ground.ok")
    return normal, offset, ok


def take_count(take_offset):
    """the G of a (G + 1) table of first frames, host or device, read from its size alone (None: one take)"""
    if take_offset is None:
        return 1
    return max(int(take_offset.numel() if torch.is_tensor(take_offset) else np.asarray(take_offset).size) - 1, 1)


def need_device(who, *tensors, optional=()):
    """the refusal of CPU inputs, after every ValueError: ``tensors`` are device tensors, and so is what is not None of ``optional``"""
    if not all(torch.is_tensor(t) and t.is_cuda for t in tensors) or not all(t.is_cuda for t in optional if t is not None):
        raise RuntimeError(f"manipose_amd: {who} takes device tensors; there is no CPU fallback")

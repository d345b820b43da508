"""Whole-sequence lifting: 2-D keypoints ``(N, 17, 2)`` of any length in, one 3-D pose per frame out.

Counterpart of the reference's ``lift_action`` (hpe/eval_utils.py:226-253, used by hpe/viz.py:84-91): windows with the
``drop_last=False`` replicate padding of its generator (hpe/mh_so3_hpe/data/generators.py:93-104,135-154), the flip test-time
augmentation of its evaluation loop (eval_utils.py:84-142) and the flattening of the predictions - here with windows that may
overlap (``stride < T``) and everything on the device: the raw keypoints are uploaded once, ``mp_lift_windows_2d`` cuts the
(mirrored) windows, the engine runs its no-backward forward, and ONE kernel (``mp_lift_merge``) aggregates the hypotheses, undoes
the mirroring and blends the windows that cover a frame, reading every hypothesis once.

The bindings come in three layers, each importing only the ones before it: lift_args.py (the argument checks), lift_ops.py (the per-sequence
operators and their launchers: rigid, rotations, smooth, path, score, place / reproject / world; its docstring describes each stage), lift_views.py
(the take-level operators on the views of a take: fuse, fuse-path, place-views, align, bundle, triangulate; they are NOT stages of the chain below but work
on what it returns) and this module, the pipeline - and the import surface: every public name of the other three is re-exported here.

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
"""
from __future__ import annotations

import ctypes as C
from collections import namedtuple
from typing import Sequence, Tuple

import numpy as np
import torch

from . import _lib, lift_args
from .lift_ops import (FLOOR_SHARES, PATH_MAXK, PATH_SIGMA, PATH_SWITCH, REFINE_MAXITERS, ROT_CONTINUOUS, SCORE_PROCRUSTES,  # noqa: F401
                       SCORE_ROOT_RELATIVE, SCORE_SHARES, SMOOTH_MAXR, TAPER, PoseScore, TrajScore, _host_f32, _launch, _parents_c, _path,
                       _place_refine, _pose_record, _rest_c, _rigid, _rotations, _score, _skeleton_of, _smooth, _smooth_options, _traj_record, _world,
                       GROUND_MAXFEET, GROUND_MAXITERS, GROUND_MAXRADIUS, Ground, estimate_ground, FOOTLOCK_MAXBLEND, FootLock, lock_feet,
                       FK_POSE_LENGTHS, Retimed, pose_from_rotations, retime_rotations, smooth_rotations,
                       EULER_CONTINUOUS, EULER_ORDERS, Eulers, euler_from_rotations,
                       bone_length_means, camera_table, place_poses, pose_rotations, project_rigid, reproject_poses, score_poses, score_traj,
                       select_path, smooth_poses, smooth_traj, to_world)
from .lift_views import (ALIGN_ITERS, ALIGN_MAXITERS, ALIGN_SIGMA, BUNDLE_ITERS, BUNDLE_MAXITERS, BUNDLE_SIGMA, CALIBRATE_ITERS, CALIBRATE_MAXITERS, CALIBRATE_PRIOR,
                         CALIBRATE_SIGMA, ViewCalibration, calibrate_views, FUSE_MAXK, FUSE_MAXV,  # noqa: F401
                         FUSE_SCORE_WEIGHT, FUSE_SIGMA, ViewAlignment, ViewBundle, ViewSync, SYNC_MAXLAG, SYNC_MAX_LAG, SYNC_MIN_OVERLAP, SYNC_SIGMA, sync_views, shift_views, ViewSkeleton, ViewSkeletonSmooth, ViewTriangulation, align_views, bundle_views, fuse_views, fuse_views_path,
                         fit_skeleton_views, place_views, triangulate_views)

AGG = {"weighted_ave": 0, "best_score": 1}
BLEND = {"mean": 0, "center": 1}


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


def _mirror(model, J):
    sk = _skeleton_of(model)
    m = list(range(J))
    for l, r in zip(sk.joints_left, sk.joints_right):
        m[l], m[r] = r, l
    return (C.c_int32 * J)(*m)


def _i32p(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def merge_windows(poses, scores, win_seq, win_start, seq_offset, *, T, tta, mirror, agg="weighted_ave", blend="mean", scale=1.0,
                  return_hyps=False, out=None, hyps=None, device_tables=None):
    """``mp_lift_merge`` on device tensors: poses (F*W, K, T, J, 3), scores (F*W, K, T, 1) or None (K == 1); win_seq / win_start (W)
    and seq_offset (S + 1) HOST numpy tables (uploaded here unless ``device_tables`` = their device copies is given).
    Returns (out (Ntot, J, 3), hyps (Ntot, K, J, 4) or None)."""
    if agg not in AGG:
        raise ValueError(f"agg must be one of {sorted(AGG)}, got {agg!r} ('oracle' needs ground truth: hpe/_entry.py::evaluate)")
    if blend not in BLEND:
        raise ValueError(f"blend must be one of {sorted(BLEND)}, got {blend!r}")
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
    _launch(dev, "mp_lift_merge", _lib.ptr(poses), _lib.ptr(scores), W, K, int(T), J, int(bool(tta)), _lib.ptr(d_seq), _lib.ptr(d_start), _lib.ptr(d_off),
            S, _i32p(h_seq), _i32p(h_start), h_off.ctypes.data_as(C.POINTER(C.c_int64)), mirror, AGG[agg], BLEND[blend], float(scale), _lib.ptr(out),
            _lib.ptr(hyps) if return_hyps else None)
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
    if not lift_args.is_int_in(place_refine, 0, REFINE_MAXITERS):
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
        if not lift_args.is_int_in(r, 0, SMOOTH_MAXR):
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
        lift_args.sigma_pair(path_sigma, path_switch, ("path_sigma", "path_switch"))
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
    dev, T, J, K, tta = opt.dev, opt.T, opt.J, opt.K, opt.tta
    F = 2 if tta else 1
    a0, nw = int(plan.first[s]), int(plan.first[s + 1] - plan.first[s])
    buf_p = buf_s = None
    for a in range(0, nw, opt.batch):
        n = min(opt.batch, nw - a)
        X = torch.empty(F * n, T, J, 2, dtype=torch.float32, device=dev)
        for h in range(F):
            _launch(dev, "mp_lift_windows_2d", _lib.ptr(plan.p2), _lib.ptr(plan.d_off), len(plan.lens), _lib.ptr(plan.d_seq[a0 + a:]),
                    _lib.ptr(plan.d_start[a0 + a:]), _lib.ptr(plan.d_flip) if h else None, plan.mirror, n, T, J, _lib.ptr(X[h * n:]))
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
           "select_path", "score_poses", "score_traj", "fuse_views", "fuse_views_path", "place_views", "align_views", "sync_views", "shift_views", "bundle_views", "calibrate_views", "triangulate_views", "fit_skeleton_views", "lift_sequences",
           "lift_action", "estimate_ground", "lock_feet", "pose_from_rotations", "retime_rotations", "smooth_rotations", "euler_from_rotations"]

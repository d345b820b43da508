"""The argument errors of the lifting bindings, word for word (no GPU): every row of CASES is a bad call with CPU tensors, a CPU model or an
argument list for hpe/_entry.py::run, and its exception type and complete message are held against tests/golden/lift_messages.json, which
tools/gen_golden_lift_messages.py recorded from this table at the commit before the bindings were cut into lift_args / lift_ops / lift_views /
lifting.  The table reaches every raise of those modules, of ``lifting._check_options`` and of the ``lift_*_options`` functions that can be reached
without a device; of the "no CPU fallback" refusals one per public function."""
import json
import os
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hpe"))
GOLD = os.path.join(ROOT, "tests", "golden", "lift_messages.json")

U8 = torch.uint8
P, P2J, H, H5 = torch.zeros(6, 17, 3), torch.zeros(6, 2, 3), torch.zeros(6, 3, 17, 4), torch.zeros(4, 6, 5, 17, 4)
TRAJ, KP, KPV, VP = torch.zeros(6, 3), torch.zeros(6, 17, 2), torch.zeros(4, 6, 17, 2), torch.zeros(4, 6, 17, 3)
INTR, ROOT3 = np.ones(9, np.float32), torch.zeros(6, 3)
SEQS = [np.zeros((12, 17, 2), np.float32), np.zeros((20, 17, 2), np.float32)]
PATH = dict(agg="path", tta=False)
_MODELS = {}


def _model(kind="rmcl"):
    """a CPU model: whatever passes the checks ends in the refusal of a model that is not on a device"""
    if kind not in _MODELS:
        from manipose_amd import ManifoldMixSTE, MixSTE, RMCLManifoldMixSTE, h36m_skeleton
        kw = dict(num_frame=9, embed_dim_rot=32, depth_rot=1, num_heads_rot=4, embed_dim_seg=16, depth_seg=1, num_heads_seg=4)
        _MODELS[kind] = (RMCLManifoldMixSTE(h36m_skeleton(), n_hyp=2, **kw) if kind == "rmcl" else ManifoldMixSTE(h36m_skeleton(), **kw)
                         if kind == "manifold" else MixSTE(num_frame=9, num_joints=17, in_chans=2, out_dim=3, embed_dim=32, depth=1, num_heads=4))
    return _MODELS[kind]


def _cams():
    from manipose_amd.data.ingest import h36m_cameras
    return list(h36m_cameras()["S11"])


def _quat():
    return np.stack([c["orientation"] for c in _cams()])


def _sk(**kw):
    from manipose_amd import h36m_skeleton
    return types.SimpleNamespace(**{"parents": [int(p) for p in h36m_skeleton().parents], **kw})


def _m():
    import manipose_amd
    from manipose_amd import lifting
    ns = types.SimpleNamespace(**{n: getattr(lifting, n) for n in lifting.__all__})
    assert all(getattr(manipose_amd, n) is getattr(lifting, n) for n in lifting.__all__ if hasattr(manipose_amd, n))
    return ns


def _lift(**kw):
    return _m().lift_sequences(_model(kw.pop("model", "rmcl")), kw.pop("seqs", SEQS), **kw)


def _run(*argv):
    from _entry import run
    return run(["run.train=false", "run.test=false"] + list(argv))


def _zero(q, v):
    q = q.copy()
    q[v] = 0
    return q


def _nan_cam():
    return np.concatenate([np.full(1, np.nan), np.ones(15)])


ON = ("run.lift=true", "lift.fuse=true")
u8 = lambda *shape: torch.ones(*shape, dtype=U8)                                                     # noqa: E731
nested = lambda: [_cams()]                                                                               # noqa: E731

CASES = {
    # lift_ops: the per-sequence operators
    "bone_length_means.shape": lambda m: m.bone_length_means(torch.zeros(6, 17, 2)),
    "bone_length_means.root": lambda m: m.bone_length_means(P, skeleton=types.SimpleNamespace(parents=[0] * 17)),
    "bone_length_means.joints": lambda m: m.bone_length_means(torch.zeros(6, 5, 3)),
    "bone_length_means.seq_offset": lambda m: m.bone_length_means(P, seq_offset=[6]),
    "bone_length_means.seq_offset_2d": lambda m: m.bone_length_means(P, seq_offset=np.zeros((2, 2), np.int64)),
    "bone_length_means.real_frames": lambda m: m.bone_length_means(P, real_frames=[1, 2]),
    "project_rigid.cpu": lambda m: m.project_rigid(P, np.ones(16)),
    "pose_rotations.shape": lambda m: m.pose_rotations(torch.zeros(6, 17, 2)),
    "pose_rotations.dtype": lambda m: m.pose_rotations(P.double()),
    "pose_rotations.joints": lambda m: m.pose_rotations(torch.zeros(6, 1, 3)),
    "pose_rotations.default_skeleton": lambda m: m.pose_rotations(torch.zeros(6, 5, 3)),
    "pose_rotations.no_t_pose": lambda m: m.pose_rotations(P, skeleton=_sk()),
    "pose_rotations.no_direction": lambda m: m.pose_rotations(P, skeleton=_sk(t_pose_operators={})),
    "pose_rotations.direction_shape": lambda m: m.pose_rotations(P, skeleton=_sk(t_pose_operators={j: np.ones(2) for j in range(17)})),
    "pose_rotations.direction_zero": lambda m: m.pose_rotations(P, skeleton=_sk(t_pose_operators={j: np.zeros(3) for j in range(17)})),
    "pose_rotations.cpu": lambda m: m.pose_rotations(P),
    "smooth_poses.radius_0": lambda m: m.smooth_poses(P, radius=0),
    "smooth_poses.radius_bool": lambda m: m.smooth_poses(P, radius=True),
    "smooth_poses.radius_65": lambda m: m.smooth_poses(P, radius=65),
    "smooth_poses.radius_float": lambda m: m.smooth_poses(P, radius=4.0),
    "smooth_poses.degree_3": lambda m: m.smooth_poses(P, degree=3),
    "smooth_poses.degree_bool": lambda m: m.smooth_poses(P, degree=False),
    "smooth_poses.taper": lambda m: m.smooth_poses(P, taper="gauss"),
    "smooth_poses.shape": lambda m: m.smooth_poses(torch.zeros(6, 2, 17, 5)),
    "smooth_poses.joints": lambda m: m.smooth_poses(torch.zeros(6, 2, 33, 3)),
    "smooth_poses.cpu": lambda m: m.smooth_poses(P, radius=np.int32(64), degree=0, taper="biweight"),
    "smooth_traj.radius": lambda m: m.smooth_traj(TRAJ, radius=0),
    "smooth_traj.shape": lambda m: m.smooth_traj(torch.zeros(6, 2)),
    "smooth_traj.ok_shape": lambda m: m.smooth_traj(TRAJ, ok=u8(5)),
    "smooth_traj.ok_dtype": lambda m: m.smooth_traj(TRAJ, ok=torch.ones(6)),
    "smooth_traj.ok_array": lambda m: m.smooth_traj(TRAJ, ok=np.ones(6, np.uint8)),
    "smooth_traj.cpu": lambda m: m.smooth_traj(TRAJ, ok=u8(6)),
    "select_path.numbers": lambda m: m.select_path(H, sigma="a"),
    "select_path.numbers_bool": lambda m: m.select_path(H, switch_cost=True),
    "select_path.sigma_0": lambda m: m.select_path(H, sigma=0),
    "select_path.sigma_nan": lambda m: m.select_path(H, sigma=float("nan")),
    "select_path.switch_negative": lambda m: m.select_path(H, switch_cost=-1),
    "select_path.switch_inf": lambda m: m.select_path(H, switch_cost=float("inf")),
    "select_path.shape": lambda m: m.select_path(torch.zeros(6, 3, 17, 3)),
    "select_path.hypotheses": lambda m: m.select_path(torch.zeros(6, 9, 17, 4)),
    "select_path.joints": lambda m: m.select_path(torch.zeros(6, 3, 1, 4)),
    "select_path.cpu": lambda m: m.select_path(H, sigma=float("inf"), switch_cost=np.float32(2)),
    "score_poses.scale_0": lambda m: m.score_poses(P, P, pose_scale=0),
    "score_poses.scale_bool": lambda m: m.score_poses(P, P, target_scale=True),
    "score_poses.scale_inf": lambda m: m.score_poses(P, P, target_scale=float("inf")),
    "score_poses.shape": lambda m: m.score_poses(torch.zeros(6, 17, 4), P),
    "score_poses.target_shape": lambda m: m.score_poses(P, torch.zeros(5, 17, 3)),
    "score_poses.target_array": lambda m: m.score_poses(P, P.numpy()),
    "score_poses.valid_shape": lambda m: m.score_poses(H, P, valid=u8(6)),
    "score_poses.valid_list": lambda m: m.score_poses(P, P, valid=[1] * 6),
    "score_poses.procrustes": lambda m: m.score_poses(P2J, P2J),
    "score_poses.skeleton": lambda m: m.score_poses(P2J, P2J, procrustes=False, skeleton=_sk()),
    "score_poses.cpu": lambda m: m.score_poses(H, P, valid=u8(6, 3)),
    "score_traj.shape": lambda m: m.score_traj(torch.zeros(6, 3, 2), TRAJ),
    "score_traj.target_shape": lambda m: m.score_traj(TRAJ, torch.zeros(6, 1, 3)),
    "score_traj.target_none": lambda m: m.score_traj(TRAJ, None),
    "score_traj.ok": lambda m: m.score_traj(torch.zeros(6, 2, 3), TRAJ, ok=u8(6)),
    "score_traj.cpu": lambda m: m.score_traj(TRAJ, TRAJ),
    "camera_table.dict": lambda m: m.camera_table(_cams()[0]),
    "camera_table.empty": lambda m: m.camera_table([]),
    "camera_table.keys": lambda m: m.camera_table([{"intrinsic": np.ones(9)}]),
    "camera_table.part": lambda m: m.camera_table([{"intrinsic": np.ones(8), "orientation": np.ones(4)}]),
    "camera_table.row": lambda m: m.camera_table([_cams()[0], np.ones(15)]),
    "camera_table.finite": lambda m: m.camera_table([_nan_cam()]),
    "place_poses.refine_17": lambda m: m.place_poses(P, KP, INTR, refine=17),
    "place_poses.refine_bool": lambda m: m.place_poses(P, KP, INTR, refine=True),
    "place_poses.cpu": lambda m: m.place_poses(P, KP, INTR, refine=np.int64(16)),
    "reproject_poses.shape": lambda m: m.reproject_poses(torch.zeros(6, 17, 5), TRAJ, KP, INTR),
    "reproject_poses.traj": lambda m: m.reproject_poses(H, TRAJ, KP, INTR),
    "reproject_poses.ok": lambda m: m.reproject_poses(H, torch.zeros(6, 3, 3), KP, INTR, ok=u8(6)),
    "reproject_poses.cpu": lambda m: m.reproject_poses(P, TRAJ, KP, INTR),
    "to_world.cpu": lambda m: m.to_world(P, np.ones(4)),
    # lift_views: the take-level operators
    "fuse_views.numbers": lambda m: m.fuse_views(H5, sigma="a"),
    "fuse_views.sigma": lambda m: m.fuse_views(H5, sigma=0),
    "fuse_views.score_weight": lambda m: m.fuse_views(H5, score_weight=-1),
    "fuse_views.shape": lambda m: m.fuse_views(H),
    "fuse_views.views": lambda m: m.fuse_views(torch.zeros(5, 6, 5, 17, 4)),
    "fuse_views.hypotheses": lambda m: m.fuse_views(torch.zeros(4, 6, 9, 17, 4)),
    "fuse_views.joints": lambda m: m.fuse_views(torch.zeros(4, 6, 5, 1, 4)),
    "fuse_views.valid": lambda m: m.fuse_views(H5, valid=u8(4, 5)),
    "fuse_views.orientation_shape": lambda m: m.fuse_views(H5, _quat()[:3]),
    "fuse_views.orientation_takes": lambda m: m.fuse_views(H5, _quat(), take_offset=[0, 2, 6]),
    "fuse_views.orientation_finite": lambda m: m.fuse_views(H5, _quat() * np.nan),
    "fuse_views.orientation_zero": lambda m: m.fuse_views(H5, _zero(_quat(), 2)),
    "fuse_views.cpu": lambda m: m.fuse_views(H5, np.stack([_quat(), _quat()]), u8(4, 6), torch.tensor([0, 2, 6]), sigma=float("inf"), score_weight=0),
    "fuse_views_path.numbers": lambda m: m.fuse_views_path(H5, sigma=None),
    "fuse_views_path.path_numbers": lambda m: m.fuse_views_path(H5, path_sigma="a"),
    "fuse_views_path.path_sigma": lambda m: m.fuse_views_path(H5, path_sigma=-1.0),
    "fuse_views_path.switch_cost": lambda m: m.fuse_views_path(H5, switch_cost=1e39),
    "fuse_views_path.shape": lambda m: m.fuse_views_path(H5.double()),
    "fuse_views_path.valid": lambda m: m.fuse_views_path(H5, valid=torch.ones(4, 6)),
    "fuse_views_path.orientation_zero": lambda m: m.fuse_views_path(H5, _zero(_quat(), 0)),
    "fuse_views_path.cpu": lambda m: m.fuse_views_path(H5, _quat()),
    "place_views.refine": lambda m: m.place_views(VP[0], KPV, nested(), refine=17),
    "place_views.pose": lambda m: m.place_views(torch.zeros(6, 17, 4), KPV, nested()),
    "place_views.pose_joints": lambda m: m.place_views(torch.zeros(6, 1, 3), torch.zeros(4, 6, 1, 2), nested()),
    "place_views.keypoints": lambda m: m.place_views(VP[0], torch.zeros(4, 5, 17, 2), nested()),
    "place_views.keypoints_views": lambda m: m.place_views(VP[0], torch.zeros(5, 6, 17, 2), nested()),
    "place_views.valid": lambda m: m.place_views(VP[0], KPV, nested(), valid=u8(6, 4)),
    "place_views.cameras": lambda m: m.place_views(VP[0], KPV, _cams()[0]),
    "place_views.cameras_empty": lambda m: m.place_views(VP[0], KPV, []),
    "place_views.cameras_views": lambda m: m.place_views(VP[0], KPV, [_cams()[:3]]),
    "place_views.camera": lambda m: m.place_views(VP[0], KPV, [[_cams()[0], {"intrinsic": np.zeros(9)}, None, None]]),
    "place_views.camera_zero": lambda m: m.place_views(VP[0], KPV, [[_cams()[0], dict(_cams()[1], orientation=np.zeros(4, np.float32)), None, None]]),
    "place_views.weights_shape": lambda m: m.place_views(VP[0], KPV, nested(), weights=np.ones(16)),
    "place_views.weights_negative": lambda m: m.place_views(VP[0], KPV, nested(), weights=-np.ones(17)),
    "place_views.cpu": lambda m: m.place_views(VP[0], KPV, [[_cams()[0], None, _cams()[2], None]], weights=np.ones(17), refine=0, return_steps=True),
    "place_views.cpu_array": lambda m: m.place_views(VP[0].numpy(), KPV, nested()),
    "align_views.sigma": lambda m: m.align_views(VP, sigma=0),
    "align_views.sigma_bool": lambda m: m.align_views(VP, sigma=True),
    "align_views.iters": lambda m: m.align_views(VP, iters=9),
    "align_views.iters_float": lambda m: m.align_views(VP, iters=2.0),
    "align_views.traj_alone": lambda m: m.align_views(VP, traj=torch.zeros(4, 6, 3)),
    "align_views.shape": lambda m: m.align_views(torch.zeros(4, 6, 17, 2)),
    "align_views.views": lambda m: m.align_views(torch.zeros(5, 6, 17, 3)),
    "align_views.joints": lambda m: m.align_views(torch.zeros(4, 6, 33, 3)),
    "align_views.valid": lambda m: m.align_views(VP, valid=u8(6, 4)),
    "align_views.traj_shape": lambda m: m.align_views(VP, traj=torch.zeros(4, 6, 2), traj_ok=u8(4, 6)),
    "align_views.traj_array": lambda m: m.align_views(VP, traj=np.zeros((4, 6, 3), np.float32), traj_ok=u8(4, 6)),
    "align_views.traj_ok_array": lambda m: m.align_views(VP, traj=torch.zeros(4, 6, 3), traj_ok=np.ones((4, 6), np.uint8)),
    "align_views.traj_ok_dtype": lambda m: m.align_views(VP, traj=torch.zeros(4, 6, 3), traj_ok=torch.ones(4, 6)),
    "align_views.reference_count": lambda m: m.align_views(VP, reference=_cams()[:2]),
    "align_views.reference_zero": lambda m: m.align_views(VP, reference=dict(_cams()[0], orientation=np.zeros(4, np.float32))),
    "align_views.reference_camera": lambda m: m.align_views(VP, reference=np.ones(15)),
    "align_views.cpu": lambda m: m.align_views(VP, u8(4, 6), [0, 2, 6], torch.zeros(4, 6, 3).transpose(0, 1).contiguous().transpose(0, 1), u8(4, 6),
                                               sigma=float("inf"), iters=0, reference=_cams()[:2]),
    "bundle_views.sigma": lambda m: m.bundle_views(VP[0], ROOT3, KPV, nested(), sigma=-1),
    "bundle_views.iters": lambda m: m.bundle_views(VP[0], ROOT3, KPV, nested(), iters=True),
    "bundle_views.pose": lambda m: m.bundle_views(VP[0].double(), ROOT3, KPV, nested()),
    "bundle_views.root": lambda m: m.bundle_views(VP[0], torch.zeros(5, 3), KPV, nested()),
    "bundle_views.keypoints": lambda m: m.bundle_views(VP[0], ROOT3, KPV.double(), nested()),
    "bundle_views.valid": lambda m: m.bundle_views(VP[0], ROOT3, KPV, nested(), valid=u8(4, 5)),
    "bundle_views.root_ok_array": lambda m: m.bundle_views(VP[0], ROOT3, KPV, nested(), root_ok=np.ones(6, np.uint8)),
    "bundle_views.root_ok_shape": lambda m: m.bundle_views(VP[0], ROOT3, KPV, nested(), root_ok=u8(6, 1)),
    "bundle_views.cameras": lambda m: m.bundle_views(VP[0], ROOT3, KPV, [_cams()[:2]]),
    "bundle_views.fixed_shape": lambda m: m.bundle_views(VP[0], ROOT3, KPV, nested(), fixed=[1, 0, 0]),
    "bundle_views.fixed_dtype": lambda m: m.bundle_views(VP[0], ROOT3, KPV, nested(), fixed=np.ones((1, 4))),
    "bundle_views.weights": lambda m: m.bundle_views(VP[0], ROOT3, KPV, nested(), weights=np.full(17, np.inf)),
    "bundle_views.cpu": lambda m: m.bundle_views(VP[0], ROOT3, KPV, [[_cams()[0], None, _cams()[2], None]], u8(4, 6), None, u8(6), [1, 0, 0, 0],
                                                 np.ones(17), sigma=float("inf"), iters=0),
    "bundle_views.cpu_array": lambda m: m.bundle_views(VP[0], ROOT3.numpy(), KPV, nested()),
    # lifting: the windows, the merge and lift_sequences' options, in _check_options' order
    "plan_windows.stride": lambda m: m.plan_windows([5], 9, 10),
    "plan_windows.frames": lambda m: m.plan_windows([5, 0], 9, 9),
    "merge_windows.agg": lambda m: m.merge_windows(None, None, [0], [0], [0, 9], T=9, tta=False, mirror=None, agg="path"),
    "merge_windows.blend": lambda m: m.merge_windows(None, None, [0], [0], [0, 9], T=9, tta=False, mirror=None, blend="median"),
    "lift_sequences.rigid_words": lambda m: _lift(symmetric=True),
    "lift_sequences.frame": lambda m: _lift(frame="floor"),
    "lift_sequences.switches": lambda m: _lift(place=1),
    "lift_sequences.place_cameras": lambda m: _lift(place=True),
    "lift_sequences.world_cameras": lambda m: _lift(frame="world"),
    "lift_sequences.floor_world": lambda m: _lift(floor=True),
    "lift_sequences.cameras_alone": lambda m: _lift(cameras=_cams()[:2]),
    "lift_sequences.return_place": lambda m: _lift(return_place=True),
    "lift_sequences.place_padding": lambda m: _lift(place=True, cameras=_cams()[:2], keep_padding=True),
    "lift_sequences.place_refine_17": lambda m: _lift(place_refine=17),
    "lift_sequences.place_refine_bool": lambda m: _lift(place_refine=True),
    "lift_sequences.place_refine_alone": lambda m: _lift(place_refine=2),
    "lift_sequences.rotations_switches": lambda m: _lift(rotations=1),
    "lift_sequences.rotations_words": lambda m: _lift(return_rotations=True),
    "lift_sequences.rotations_padding": lambda m: _lift(rotations=True, keep_padding=True),
    "lift_sequences.smooth_poses": lambda m: _lift(smooth_poses=65),
    "lift_sequences.smooth_traj": lambda m: _lift(smooth_traj=True),
    "lift_sequences.smooth_words": lambda m: _lift(smooth_degree=1),
    "lift_sequences.smooth_degree": lambda m: _lift(smooth_poses=2, smooth_degree=3),
    "lift_sequences.smooth_taper": lambda m: _lift(smooth_poses=2, smooth_taper="gauss"),
    "lift_sequences.smooth_traj_alone": lambda m: _lift(smooth_traj=2),
    "lift_sequences.smooth_padding": lambda m: _lift(smooth_poses=2, keep_padding=True),
    "lift_sequences.path_numbers": lambda m: _lift(path_sigma="0.02", **PATH),
    "lift_sequences.path_sigma": lambda m: _lift(path_sigma=0.0, **PATH),
    "lift_sequences.path_switch": lambda m: _lift(path_switch=float("inf"), **PATH),
    "lift_sequences.path_tta": lambda m: _lift(agg="path"),
    "lift_sequences.path_padding": lambda m: _lift(keep_padding=True, **PATH),
    "lift_sequences.path_words": lambda m: _lift(path_switch=1.0),
    "lift_sequences.path_words_bool": lambda m: _lift(path_sigma=True),
    "lift_sequences.return_score": lambda m: _lift(return_score=True),
    "lift_sequences.targets_padding": lambda m: _lift(targets=[np.zeros((12, 17, 3)), np.zeros((20, 17, 3))], keep_padding=True),
    "lift_sequences.targets_count": lambda m: _lift(targets=[np.zeros((12, 17, 3))]),
    "lift_sequences.targets_shape": lambda m: _lift(targets=[np.zeros((12, 17, 3)), np.zeros((19, 17, 3))]),
    "lift_sequences.targets_dtype": lambda m: _lift(targets=[torch.zeros(12, 17, 3), torch.zeros(20, 17, 3, dtype=torch.bool)]),
    "lift_sequences.cameras_count": lambda m: _lift(place=True, cameras=_cams()[:3]),
    "lift_sequences.cameras_camera": lambda m: _lift(place=True, cameras=[_cams()[0], np.ones(15)]),
    "lift_sequences.model": lambda m: m.lift_sequences(object(), SEQS),
    "lift_sequences.path_hypotheses": lambda m: _lift(model="manifold", **PATH),
    "lift_sequences.lengths_word": lambda m: _lift(rigid=True, lengths="mean"),
    "lift_sequences.lengths_mixste": lambda m: _lift(model="mixste", rigid=True, lengths="model"),
    "lift_sequences.lengths_shape": lambda m: _lift(rigid=True, lengths=np.ones((3, 16))),
    "lift_sequences.lengths_negative": lambda m: _lift(rigid=True, lengths=-np.ones(16)),
    "lift_sequences.agg": lambda m: _lift(agg="oracle"),
    "lift_sequences.blend": lambda m: _lift(blend="median"),
    "lift_sequences.padding_stride": lambda m: _lift(keep_padding=True, stride=3),
    "lift_sequences.sequence_shape": lambda m: _lift(seqs=[np.zeros((12, 16, 2), np.float32)]),
    "lift_sequences.stride": lambda m: _lift(stride=10),
    "lift_sequences.cpu": lambda m: _lift(rigid=True, symmetric=True, rotations=True, smooth_poses=2, place=True, cameras=_cams()[:2], frame="world", floor=True,
                                          place_refine=3, smooth_traj=3, return_hyps=True, targets=[np.zeros((12, 17, 3)), np.zeros((20, 17, 3))],
                                          path_sigma=0.05, path_switch=np.float32(1), return_path=True, **PATH),
    # hpe/_entry.py: the lift_*_options functions, in the order run() calls them
    "entry.place.frame": lambda m: _run("lift.frame=sky"),
    "entry.place.floor": lambda m: _run("lift.floor=true"),
    "entry.place.3dhp": lambda m: _run("lift.place=true", "+data=mpi_inf_3dhp"),
    "entry.smooth.radius": lambda m: _run("lift.smooth_poses=65"),
    "entry.smooth.radius_bool": lambda m: _run("lift.smooth_traj=true"),
    "entry.smooth.degree": lambda m: _run("lift.smooth_poses=2", "lift.smooth_degree=3"),
    "entry.smooth.degree_float": lambda m: _run("lift.smooth_poses=2", "lift.smooth_degree=1.0"),
    "entry.smooth.taper": lambda m: _run("lift.smooth_poses=2", "lift.smooth_taper=gauss"),
    "entry.smooth.words": lambda m: _run("lift.smooth_degree=1"),
    "entry.smooth.traj_alone": lambda m: _run("lift.smooth_traj=2"),
    "entry.refine.steps": lambda m: _run("lift.place_refine=17"),
    "entry.refine.steps_float": lambda m: _run("lift.place_refine=1.5"),
    "entry.refine.alone": lambda m: _run("lift.place_refine=2"),
    "entry.path.agg": lambda m: _run("lift.agg=oracle"),
    "entry.path.number": lambda m: _run("lift.path_sigma=big"),
    "entry.path.number_bool": lambda m: _run("lift.path_switch=true"),
    "entry.path.sigma": lambda m: _run("lift.path_sigma=0"),
    "entry.path.switch": lambda m: _run("lift.path_switch=-1"),
    "entry.path.words": lambda m: _run("lift.path_sigma=0.05"),
    "entry.path.tta": lambda m: _run("lift.agg=path"),
    "entry.path.model": lambda m: _run("lift.agg=path", "train.tta=false", "model.arch=mixste"),
    "entry.score.bool": lambda m: _run("lift.score=1"),
    "entry.score.alone": lambda m: _run("lift.score=true"),
    "entry.rotations.bool": lambda m: _run("lift.rotations=1"),
    "entry.rotations.alone": lambda m: _run("lift.rotations=true"),
    "entry.rotations.words": lambda m: _run("lift.rotations_continuous=false"),
    "entry.fuse.bool": lambda m: _run("lift.fuse=1"),
    "entry.fuse.number": lambda m: _run("lift.fuse_sigma=abc"),
    "entry.fuse.sigma": lambda m: _run("lift.fuse_sigma=0"),
    "entry.fuse.weight": lambda m: _run("lift.fuse_score_weight=-1"),
    "entry.fuse.refine": lambda m: _run("lift.fuse_refine=17"),
    "entry.fuse.refine_bool": lambda m: _run("lift.fuse_refine=true"),
    "entry.fuse.words": lambda m: _run("lift.fuse_score_weight=2"),
    "entry.fuse.alone": lambda m: _run("lift.fuse=true"),
    "entry.fuse.3dhp": lambda m: _run(*ON, "+data=mpi_inf_3dhp"),
    "entry.fuse.padding": lambda m: _run(*ON, "+lift.keep_padding=true"),
    "entry.fuse.model": lambda m: _run(*ON, "data.data_dir=/nowhere", "model.arch=mixste"),
    "entry.fuse.hypotheses": lambda m: _run(*ON, "multi_hyp.n_hyp=9"),
    "entry.fuse_path.bool": lambda m: _run("lift.fuse_path=1"),
    "entry.fuse_path.number": lambda m: _run("lift.fuse_path_switch=abc"),
    "entry.fuse_path.sigma": lambda m: _run("lift.fuse_path_sigma=0"),
    "entry.fuse_path.switch": lambda m: _run("lift.fuse_path_switch=-1"),
    "entry.fuse_path.words": lambda m: _run("lift.fuse_path_sigma=0.05"),
    "entry.fuse_path.alone": lambda m: _run("lift.fuse_path=true"),
    "entry.fuse_align.cameras": lambda m: _run("lift.fuse_cameras=guess"),
    "entry.fuse_align.number": lambda m: _run("lift.fuse_align_sigma=abc"),
    "entry.fuse_align.sigma": lambda m: _run("lift.fuse_align_sigma=0"),
    "entry.fuse_align.iters": lambda m: _run("lift.fuse_align_iters=9"),
    "entry.fuse_align.words": lambda m: _run("lift.fuse_align_iters=2"),
    "entry.fuse_align.alone": lambda m: _run("lift.fuse_cameras=estimate"),
    "entry.fuse_bundle.steps": lambda m: _run("lift.fuse_bundle=9"),
    "entry.fuse_bundle.steps_bool": lambda m: _run("lift.fuse_bundle=true"),
    "entry.fuse_bundle.number": lambda m: _run("lift.fuse_bundle_sigma=abc"),
    "entry.fuse_bundle.sigma": lambda m: _run("lift.fuse_bundle_sigma=0"),
    "entry.fuse_bundle.words": lambda m: _run("lift.fuse_bundle_sigma=0.1"),
    "entry.fuse_bundle.alone": lambda m: _run("lift.fuse_bundle=2"),
}


def provoke(name):
    """(exception type's name, complete message, the exception) of the row ``name``; AssertionError if the call returns"""
    try:
        CASES[name](_m())
    except (ValueError, RuntimeError) as e:
        return type(e).__name__, str(e), e
    raise AssertionError(f"{name}: the call was accepted")


def test_the_table_and_the_record_hold_the_same_rows():
    assert sorted(json.load(open(GOLD))) == sorted(CASES)


@pytest.mark.parametrize("name", sorted(CASES))
def test_exception_type_and_message_word_for_word(name):
    want = json.load(open(GOLD))[name]
    kind, message, _ = provoke(name)
    assert (kind, message) == (want["type"], want["message"])

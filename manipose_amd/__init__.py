"""manipose_amd: MI355X (gfx950)-native implementation of ManiPose's 2D->3D lifting hot path.

Host side in Python (the reference's nn.Module contract), compute in hand-written HIP kernels behind the C ABI of
include/manipose_hip.h (libmanipose_hip.so).  See DESIGN.md.
"""
from . import _lib  # noqa: F401
from .architectures import ManifoldMixSTE, MixSTE, RMCLManifoldMixSTE  # noqa: F401
from .data import Skeleton, h36m_skeleton  # noqa: F401
from .lifting import align_views, bundle_views, calibrate_views, camera_table, estimate_ground, euler_from_rotations, fit_skeleton_views, fuse_views, fuse_views_path, lift_action, lift_sequences, lock_feet, place_poses, place_views, plan_windows, pose_from_rotations, pose_rotations, project_rigid, reproject_poses, retime_rotations, score_poses, score_traj, select_path, shift_views, smooth_poses, smooth_rotations, smooth_traj, sync_views, to_world, triangulate_views  # noqa: F401

__version__ = "0.1.0"
from . import ops  # noqa: F401  (registers torch.ops.manipose.*)

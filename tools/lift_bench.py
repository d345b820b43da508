"""Output stage of sequence lifting, two forms on the same hypotheses and scores in one process (frames per second, HIP events):
  (a) the composition of existing ops the evaluation path uses (hpe/_entry.py::evaluate): mp_aggregate on the original half, clone +
      pose_flip of the mirrored hypotheses, mp_aggregate, average - "weighted_ave" only, and with "best_score" as evaluate computes both;
  (b) mp_lift_merge (one kernel).
Then lift_sequences end to end (gather + forward + merge) at the same batch.
    python tools/lift_bench.py [W=158] [T=243] [K=5] [precision=bf16x3] [reps=50]
    python tools/lift_bench.py --place [frames=3000] [K=5] [reps=50]
    python tools/lift_bench.py --path [frames=3000] [K=5] [reps=50]
    python tools/lift_bench.py --score [frames=3000] [K=5] [reps=50]
    python tools/lift_bench.py --rotations [frames=3000] [K=5] [reps=50]
    python tools/lift_bench.py --fuse [frames=3000] [K=5] [reps=200]
    python tools/lift_bench.py --fuse-path [frames=3000] [K=5] [reps=20]
    python tools/lift_bench.py --align [frames=3000] [reps=20]
    python tools/lift_bench.py --sync [frames=3000] [reps=20]
    python tools/lift_bench.py --bundle [frames=3000] [reps=20]
    python tools/lift_bench.py --calibrate [frames=3000] [reps=20]
    python tools/lift_bench.py --triangulate [frames=3000] [reps=20]
    python tools/lift_bench.py --skeleton [frames=3000] [reps=20]
    python tools/lift_bench.py --skeleton-smooth [frames=3000] [reps=20]
    python tools/lift_bench.py --ground [frames=3000] [reps=20]
    python tools/lift_bench.py --footlock [frames=3000] [reps=20]
    python tools/lift_bench.py --retime [frames=3000] [reps=20]
    python tools/lift_bench.py --bvh [frames=3000] [reps=20]
--bvh times mp_lift_euler (the Euler channels a BVH file holds: one lane per (pose, joint), then with MP_LIFT_EULER_CONTINUOUS one wave per
(sequence, joint) track that walks its frames 64 at a time) through its private launcher on a spinning synthetic take of 17 joints with 10 % of the
frames invalid, a basis and a shift, order ZXY, as ONE sequence of `frames` frames and as 64 sequences of `frames` each: the first pass alone, both
passes, their difference (the second pass), and the bytes each must move at least once with the bandwidth that implies.
--retime times mp_lift_retime (a take resampled in time on its rotations: one lane per (output pose, joint)) and mp_lift_fk (the positions of
(root, quat, bones)) through their private launchers on a smooth synthetic take of 17 joints with 10 % of the frames invalid, as ONE take of
`frames` frames and as 64 sequences of `frames` / 10, at the rates 50 -> 50, 50 -> 30 and 50 -> 60 and the radii 0, 4 and 64; beside each time the
bytes the kernel requests and writes and the bandwidth that implies, and mp_lift_smooth on the same quaternion array at the same radius in the same
run (the operators have no predecessor: that is the figure to hold them against).
--footlock times mp_lift_footlock (the feet pinned on their contacts: a copy, the run kernel with one wave per (sequence, foot), the pose kernel
with one lane per (frame, foot) twice) through its private launcher on --ground's walkers, contacts and planes, as ONE take of `frames` frames and
as 64 sequences of `frames` / 10, at blend 0, 5 and 32, with and without the floor; beside each time the bytes the copy and the kernels must move
and the bandwidth that implies (the operator has no predecessor: there is no time to hold it against).
--ground times mp_lift_ground (contacts, ground plane and foot skate of a sequence: a contact kernel with one lane per (frame, foot) and a plane
kernel with one 256-lane workgroup per sequence, 2 (iters + 1) + 1 passes inside it) through its private launcher on synthetic walkers on a tilted
floor with 5 mm of noise, as ONE take of `frames` frames and as 64 sequences of `frames` / 10, at iters 0, 5 and 8, and prints how far the
normal is from the floor's.
--skeleton-smooth times mp_lift_fit_skeleton_smooth (a fused take's skeleton fitted along time: mp_lift_fit_skeleton's kernel as stage A, then three
launches a sweep, one per colour, each visited frame one Gauss-Newton step with its neighbours held) through its private launcher and through the
entry point into outputs allocated once, on --skeleton's scene and start, iters = 3, smooth = 0.1, at sweeps 1 and 8, as ONE take and cut into
16, next to mp_lift_fit_skeleton at iters 1 and 3 on the same scene in the same process; a sweep's time is (8 sweeps - 1 sweep) / 7.
--skeleton times mp_lift_fit_skeleton (one skeleton of constant bones fitted to a fused take's keypoints: one kernel, one 64-lane workgroup per
frame, the system of 35 unknowns in LDS) through its private launcher on --fuse's scene, the start that scene's triangulated joints
(mp_lift_triangulate, 3 steps), the bone table the start's median, sigma = inf, the default pull, at iters 0, 1 and 3, as ONE take and cut
into 16, next to mp_lift_triangulate's time for the same frames.
--triangulate times mp_lift_triangulate (every joint of a fused take triangulated on the 2-D keypoints: one kernel, one lane per (frame, joint))
through its private launcher on --fuse's scene - 4 views x `frames` frames of 17 joints, pinhole keypoints with 0.01 of noise, the lifted pose
0.03 m N(0, 1) off, the roots fitted by mp_lift_fuse_place - at iters 0, 1 and 3, as ONE take and cut into 16, next to mp_lift_fuse_place's time
for the same frames.
--calibrate times mp_lift_calibrate_views (a take calibrated on its keypoints: per pass one kernel with a lane per frame, which goes through the
frame's 17 points one by one, and one with a workgroup per take, iters + 1 passes) through its private launcher on --bundle's scene as ONE take,
the start the fused pose at its placed root, every view's focal lengths started 10, -10, 7 and -8 % off S11's, prior 1e-3, sigma 0.05, at iters
0, 1 and 3, beside mp_lift_bundle_views at the same iters on the same take - the yardstick - and prints the focal errors before and after.
--bundle times mp_lift_bundle_views (the bundle adjustment of a take's cameras and roots on the 2-D keypoints: per pass one kernel with a lane per
frame and one with a workgroup per take, iters + 1 passes) through its private launcher on --fuse's scene - 4 views x `frames` frames of 17 joints,
pinhole keypoints with 0.01 of noise - with the cameras of views 1..3 started 0.3 degrees and 0.15 m off S11's calibration and the roots fitted
under them by mp_lift_fuse_place, as ONE take and cut into 16, and prints how far the cameras are from the calibration before and after.
--sync times mp_lift_sync_views (a take's views synchronised in time: a signal kernel with one workgroup per (take, view), a curve kernel with one
workgroup per (take, view, block of 16 lags), a pick kernel with one wave per (take, view)) through its private launcher on 4 views x `frames`
frames of 17 joints of a smooth synthetic motion with lags of 0, 3, -7.5 and 12.25 frames, at max_lag 0 (the signal and pick kernels and an
all-but-empty curve kernel), 32 and 256, as ONE take and cut into 16, and mp_lift_shift_views in both modes on the poses (51 floats a frame) and
on hypotheses (5 x 17 x 4 floats a frame), each beside the bytes its passes must move at least once.
--align times mp_lift_align_views (a take's extrinsics from its views' poses: one workgroup per (take, view), iters + 2 passes over the poses, with
a trajectory iters + 4) through its private launcher on --fuse's scene - 4 views x `frames` frames of 17 joints, in 30 % of the frames of views 1..3
the hypothesis moved along the depth axis - as ONE take and cut into 16, and prints how far the estimate is from S11's calibration.
--fuse-path times mp_lift_fuse_path (the views' hypotheses chosen jointly over the whole take: tables, scan and emit kernels) through its private
launcher on --fuse's scene - 4 views x `frames` frames x K hypotheses - as ONE take (the scan is one workgroup walking the frames in order: the serial
case) and cut into 16, next to mp_lift_fuse on the same scene.
--fuse times mp_lift_fuse (one hypothesis per view chosen jointly over S11's four cameras, and their mean) and mp_lift_fuse_place (one world root
per frame from all views, at iters 0 and 3) through their private launchers on 4 views x `frames` frames x K hypotheses of ONE take, next to
mp_lift_path on one view's hypotheses of the same frames, for scale.
--place times only the two kernels that put a lifted sequence in the scene (mp_lift_place: root translation and reprojection error of every
hypothesis; mp_lift_world: world frame, with and without the floor) on `frames` frames x K hypotheses of one sequence with S11's first camera,
and then, in the same process, mp_lift_smooth (radius 4 and 32, degree 2, uniform) on the merged poses (frames, 17, 3), the hypotheses
(frames, K, 17, 4) and the trajectories (frames, K, 3) next to its yardstick mp_lift_rigid on the same arrays (which reads and writes the same
bytes once; it needs 2 joints, so the trajectory has none): both times, their ratio and the bytes/s of "read once, write once".  Between the two,
mp_lift_place_refine (Gauss-Newton steps under the full camera model) at iters 0, 3 and 8 and as the pure reprojection of a given trajectory,
through the private launcher on tables uploaded once; its iters = 0 row is what mp_lift_place runs (one kernel serves both) and the yardstick of the
others.  One row before them calls mp_lift_place itself into outputs allocated once: the kernel without the launcher's allocations.
--path times mp_lift_path (one hypothesis per frame, chosen over the whole sequence: cost, scan and gather kernels) through its private launcher
on `frames` frames x K hypotheses of 17 joints, as ONE sequence (the scan is one wave: the serial case) and cut into 16, next to mp_lift_rigid
on the same hypotheses.
--score times mp_lift_score (the score of lifted poses against ground truth: score, alignment and finalize kernels) through its private launcher
on `frames` frames x K hypotheses of 17 joints with bones, with and without the Procrustes alignment, as ONE sequence and cut into 16, and on the
(frames, K, 3) trajectories, next to mp_lift_rigid on the same hypotheses.
--rotations times mp_lift_rotations (the joint rotations of lifted poses: the rotation kernel and, with the continuity flag, the sign kernel) through
its private launcher on `frames` frames x K hypotheses of 17 joints, canonical signs alone and sign-continuous as ONE sequence and cut into 16,
with and without rot6d, next to mp_lift_rigid on the same hypotheses."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from manipose_amd import RMCLManifoldMixSTE, h36m_skeleton, lift_sequences, plan_windows
from manipose_amd.augmentations import pose_flip
from manipose_amd.lifting import _mirror, merge_windows



def timed_us(fn, reps):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(reps):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / reps * 1e3


def place_bench(argv):
    from manipose_amd import camera_table, place_poses, to_world
    from manipose_amd.data.ingest import h36m_cameras
    frames = int(argv[0]) if len(argv) > 0 else 3000
    K = int(argv[1]) if len(argv) > 1 else 5
    reps = int(argv[2]) if len(argv) > 2 else 50
    assert torch.cuda.is_available(), "needs an MI355X"
    intr, quat, trans = camera_table(h36m_cameras()["S11"][:1])
    g = torch.Generator(device="cuda").manual_seed(1)
    hyps = 0.3 * torch.randn(frames, K, 17, 4, device="cuda", generator=g)
    hyps[:, 1:, :, :3] = hyps[:, :1, :, :3] + 0.05 * torch.randn(frames, K - 1, 17, 3, device="cuda", generator=g)      # hypotheses of ONE frame
    hyps[:, :, 0, :3] = 0
    centre = torch.tensor([0.0, 0.0, 5.0], device="cuda")
    P = hyps[:, 0, :, :3] + centre
    kp = (torch.from_numpy(intr[0, 0:2]).cuda() * P[..., :2] / P[..., 2:3] + torch.from_numpy(intr[0, 2:4]).cuda()).contiguous()
    traj, _, ok = place_poses(hyps, kp, intr)
    print(f"--place: {frames} frames x {K} hypotheses, {hyps.numel() * 4 / 1e6:.2f} MB of poses; ok on {ok.float().mean().item():.3f} of them", flush=True)
    work = hyps.clone()
    for name, fn in (("mp_lift_place (full camera model)", lambda: place_poses(hyps, kp, intr)),
                     ("mp_lift_place (linear projection)", lambda: place_poses(hyps, kp, intr, distort=False)),
                     ("mp_lift_world", lambda: to_world(work, quat, trans, traj)),
                     ("mp_lift_world + floor (3 kernels)", lambda: to_world(work, quat, trans, traj, floor=True))):
        us = timed_us(fn, reps)            # (the public functions: their table uploads are inside the time)
        print(f"{name}: {us:,.1f} us  {frames * K / us:,.2f} M poses/s", flush=True)
    refine_bench(hyps, kp, intr, reps)
    smooth_bench(hyps, traj, reps)


def refine_bench(hyps, kp, intr, reps):
    """mp_lift_place_refine through its private launcher on tables uploaded once; ratios against its iters = 0 row, which is mp_lift_place's kernel
    and arguments (the allocation of the outputs from torch's caching allocator is inside every time)"""
    from manipose_amd import _lib
    from manipose_amd.lifting import _place_refine
    lib, dev, frames, K = _lib.load(), hyps.device, int(hyps.shape[0]), int(hyps.shape[1])
    d_off = torch.tensor([0, frames], dtype=torch.int64, device=dev)
    d_intr = torch.from_numpy(intr).to(dev)
    print(f"mp_lift_place_refine on {frames} x {K} poses (full camera model), {reps} launches each after 5 of warm-up; ratios against iters=0:", flush=True)
    out = _place_refine(lib, hyps, kp, d_off, 1, d_intr, None, True, 0)
    us = timed_us(lambda: lib.mp_lift_place(_lib.ptr(hyps), frames, K, 17, 4, _lib.ptr(kp), _lib.ptr(d_off), 1, _lib.ptr(d_intr), None, 1, _lib.ptr(out[0]),
                                            _lib.ptr(out[1]), _lib.ptr(out[2]), _lib.stream_ptr()), reps)
    print(f"mp_lift_place into outputs allocated once (the kernel alone: a row below that is not well above it is bound by its allocations): {us:,.1f} us", flush=True)
    base = None
    for iters in (0, 3, 8):
        us = timed_us(lambda: _place_refine(lib, hyps, kp, d_off, 1, d_intr, None, True, iters), reps)
        base = us if base is None else base
        steps = _place_refine(lib, hyps, kp, d_off, 1, d_intr, None, True, iters)[3].float().mean().item()
        print(f"mp_lift_place_refine iters={iters}: {us:,.1f} us  {frames * K / us:,.2f} M poses/s, ratio {us / base:.2f}; {steps:.2f} steps taken per pose",
              flush=True)
    traj, _, ok, _ = _place_refine(lib, hyps, kp, d_off, 1, d_intr, None, True, 3)
    us = timed_us(lambda: _place_refine(lib, hyps, kp, d_off, 1, d_intr, None, True, 0, traj, ok), reps)
    print(f"mp_lift_place_refine iters=0 on a given trajectory (reprojection alone): {us:,.1f} us, ratio {us / base:.2f}", flush=True)


def smooth_bench(hyps, traj, reps):
    """mp_lift_smooth and mp_lift_rigid through their private launchers on tables uploaded once: kernel against kernel"""
    from manipose_amd import _lib
    from manipose_amd.lifting import _parents_c, _rigid, _skeleton_of, _smooth
    lib, dev, frames = _lib.load(), hyps.device, int(hyps.shape[0])
    d_off = torch.tensor([0, frames], dtype=torch.int64, device=dev)
    lengths = torch.full((1, 16), 0.25, device=dev)
    parents = _parents_c(_skeleton_of(), 17)
    merged = hyps[:, :1, :, :3].contiguous()                              # (frames, 1, 17, 3)
    arrays = (("poses", merged), ("hypotheses", hyps.clone()), ("trajectory", traj.reshape(frames, -1, 1, 3).contiguous()))
    print(f"mp_lift_smooth (degree 2, uniform) against mp_lift_rigid on the same arrays, {reps} launches each after 5 of warm-up:", flush=True)
    for name, x in arrays:
        moved = 2 * x.numel() * 4                                         # read once, write once
        rigid_us = timed_us(lambda: _rigid(lib, x, d_off, 1, lengths, parents), reps) if x.shape[2] >= 2 else None
        for R in (4, 32):
            us = timed_us(lambda: _smooth(lib, x, None, d_off, 1, R, 2, "uniform"), reps)
            against = f"mp_lift_rigid {rigid_us:,.1f} us ({moved / rigid_us / 1e3:,.1f} GB/s), ratio {us / rigid_us:.2f}" if rigid_us else \
                "mp_lift_rigid needs 2 joints: no yardstick"
            print(f"mp_lift_smooth {name} {tuple(x.shape)} R={R}: {us:,.1f} us  {moved / us / 1e3:,.1f} GB/s of the {moved / 1e6:.2f} MB read once + written once; "
                  f"{against}", flush=True)


def path_bench(argv):
    from manipose_amd import _lib
    from manipose_amd.lifting import _parents_c, _path, _rigid, _skeleton_of
    frames = int(argv[0]) if len(argv) > 0 else 3000
    K = int(argv[1]) if len(argv) > 1 else 5
    reps = int(argv[2]) if len(argv) > 2 else 50
    assert torch.cuda.is_available(), "needs an MI355X"
    lib = _lib.load()
    g = torch.Generator(device="cuda").manual_seed(1)
    f = torch.arange(frames, device="cuda", dtype=torch.float32)[:, None, None, None]
    hyps = torch.empty(frames, K, 17, 4, device="cuda")
    hyps[..., :3] = 0.3 * torch.sin(f / 9.0 + torch.rand(1, 1, 17, 3, device="cuda", generator=g) * 6.28) \
        + 0.03 * torch.randn(1, K, 17, 3, device="cuda", generator=g) + 0.01 * torch.randn(frames, K, 17, 3, device="cuda", generator=g)
    hyps[..., 3] = torch.softmax(1.5 * torch.randn(frames, K, device="cuda", generator=g), dim=1)[:, :, None]
    lengths, parents = torch.full((1, 16), 0.25, device="cuda"), _parents_c(_skeleton_of(), 17)
    one = torch.tensor([0, frames], dtype=torch.int64, device="cuda")
    print(f"--path: {frames} frames x {K} hypotheses, {hyps.numel() * 4 / 1e6:.2f} MB of hypotheses, scratch {frames * (8 * K * K + 9 * K) / 1e6:.2f} MB; "
          f"{reps} calls each after 5 of warm-up (the output and scratch allocations are inside the time)", flush=True)
    for S in (1, 16):
        d_off = torch.linspace(0, frames, S + 1, device="cuda").round().to(torch.int64)
        us = timed_us(lambda: _path(lib, hyps, d_off, S, 0.02, 0.0), reps)
        path = _path(lib, hyps, d_off, S, 0.02, 0.0)[1]
        switches = int((path[1:] != path[:-1]).sum().item())
        print(f"mp_lift_path, {S} sequence(s): {us:,.1f} us  {frames / us:,.2f} M frames/s; {switches} switches", flush=True)
    work = hyps.clone()
    us = timed_us(lambda: _rigid(lib, work, one, 1, lengths, parents), reps)
    print(f"mp_lift_rigid on the same hypotheses: {us:,.1f} us", flush=True)


def score_bench(argv):
    from manipose_amd import _lib
    from manipose_amd.lifting import SCORE_PROCRUSTES, _parents_c, _rigid, _score, _skeleton_of
    frames = int(argv[0]) if len(argv) > 0 else 3000
    K = int(argv[1]) if len(argv) > 1 else 5
    reps = int(argv[2]) if len(argv) > 2 else 50
    assert torch.cuda.is_available(), "needs an MI355X"
    lib = _lib.load()
    g = torch.Generator(device="cuda").manual_seed(1)
    gt = 0.3 * torch.randn(frames, 17, 3, device="cuda", generator=g)
    hyps = torch.rand(frames, K, 17, 4, device="cuda", generator=g)
    hyps[..., :3] = 0.9 * gt[:, None] + 0.05 * torch.randn(frames, K, 17, 3, device="cuda", generator=g)
    traj, root = hyps[:, :, :1, :3].contiguous(), gt[:, :1].contiguous()
    lengths, parents = torch.full((1, 16), 0.25, device="cuda"), _parents_c(_skeleton_of(), 17)
    print(f"--score: {frames} frames x {K} hypotheses, {hyps.numel() * 4 / 1e6:.2f} MB of hypotheses; {reps} calls each after 5 of warm-up (the output and "
          f"scratch allocations are inside the time)", flush=True)
    for S in (1, 16):
        d_off = torch.linspace(0, frames, S + 1, device="cuda").round().to(torch.int64)
        for name, flags in (("sums and alignment", SCORE_PROCRUSTES), ("sums only", 0)):
            us = timed_us(lambda: _score(lib, hyps, gt, None, d_off, S, parents, 1.0, 1.0, flags, want_frames=True), reps)
            print(f"mp_lift_score, {S} sequence(s), {name}: {us:,.1f} us  {frames * K / us:,.2f} M poses/s", flush=True)
        us = timed_us(lambda: _score(lib, traj, root, None, d_off, S, None, 1.0, 1.0, 0), reps)
        print(f"mp_lift_score, {S} sequence(s), trajectories (M = 1): {us:,.1f} us  {frames * K / us:,.2f} M poses/s", flush=True)
    work = hyps.clone()
    us = timed_us(lambda: _rigid(lib, work, torch.tensor([0, frames], dtype=torch.int64, device="cuda"), 1, lengths, parents), reps)
    print(f"mp_lift_rigid on the same hypotheses: {us:,.1f} us", flush=True)


def rotations_bench(argv):
    from manipose_amd import _lib
    from manipose_amd.lifting import _parents_c, _rest_c, _rigid, _rotations, _skeleton_of
    frames = int(argv[0]) if len(argv) > 0 else 3000
    K = int(argv[1]) if len(argv) > 1 else 5
    reps = int(argv[2]) if len(argv) > 2 else 50
    assert torch.cuda.is_available(), "needs an MI355X"
    lib = _lib.load()
    g = torch.Generator(device="cuda").manual_seed(1)
    hyps = torch.rand(frames, K, 17, 4, device="cuda", generator=g)
    hyps[..., :3] = 0.3 * torch.randn(frames, K, 17, 3, device="cuda", generator=g)
    lengths, parents, rest = torch.full((1, 16), 0.25, device="cuda"), _parents_c(_skeleton_of(), 17), _rest_c(_skeleton_of(), 17)
    one = torch.tensor([0, frames], dtype=torch.int64, device="cuda")
    moved = hyps.numel() * 4 + frames * K * (17 * 16 + 1)
    print(f"--rotations: {frames} frames x {K} hypotheses, {hyps.numel() * 4 / 1e6:.2f} MB of hypotheses read, {frames * K * 17 * 16 / 1e6:.2f} MB of quaternions "
          f"written; {reps} calls each after 5 of warm-up (the output allocations are inside the time)", flush=True)
    us = timed_us(lambda: _rotations(lib, hyps, one, 1, parents, rest, False), reps)
    print(f"mp_lift_rotations, canonical signs (one kernel): {us:,.1f} us  {frames * K / us:,.2f} M poses/s, {moved / us / 1e3:,.1f} GB/s of the "
          f"{moved / 1e6:.2f} MB it must move", flush=True)
    us = timed_us(lambda: _rotations(lib, hyps, one, 1, parents, rest, False, True), reps)
    print(f"mp_lift_rotations, canonical signs, with rot6d: {us:,.1f} us  {frames * K / us:,.2f} M poses/s", flush=True)
    for S in (1, 16):
        d_off = torch.linspace(0, frames, S + 1, device="cuda").round().to(torch.int64)
        us = timed_us(lambda: _rotations(lib, hyps, d_off, S, parents, rest, True), reps)
        print(f"mp_lift_rotations, sign-continuous, {S} sequence(s) (two kernels): {us:,.1f} us  {frames * K / us:,.2f} M poses/s", flush=True)
    work = hyps.clone()
    us = timed_us(lambda: _rigid(lib, work, one, 1, lengths, parents), reps)
    print(f"mp_lift_rigid on the same hypotheses: {us:,.1f} us", flush=True)


def fuse_scene(frames, K):
    """--fuse's scene: (lib, V, (quat, trans, intr), pose, hyps (V, frames, K, 17, 4), kp) on S11's four cameras"""
    from manipose_amd import _lib
    from manipose_amd.data.ingest import h36m_cameras
    assert torch.cuda.is_available(), "needs an MI355X"
    lib, V = _lib.load(), 4
    cams = h36m_cameras()["S11"]
    quat, trans, intr = (torch.from_numpy(np.stack([c[k] for c in cams])[None].astype(np.float32)).cuda() for k in ("orientation", "translation", "intrinsic"))
    qn = quat[0] / quat[0].norm(dim=1, keepdim=True)
    w, x, y, z = qn.unbind(1)
    R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y), 2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                     2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], dim=1).view(V, 3, 3)
    g = torch.Generator(device="cuda").manual_seed(1)
    pose = 0.3 * torch.randn(frames, 17, 3, device="cuda", generator=g)
    pose[:, 0] = 0
    root = torch.cat([2 * torch.rand(frames, 2, device="cuda", generator=g) - 1, 0.8 + 0.2 * torch.rand(frames, 1, device="cuda", generator=g)], dim=1)
    cam = torch.einsum("fjc,vcd->vfjd", pose, R)                          # R^T p: every view's camera-frame pose
    hyps = torch.empty(V, frames, K, 17, 4, device="cuda")
    hyps[..., :3] = cam[:, :, None] + 0.005 * torch.randn(V, frames, K, 17, 3, device="cuda", generator=g)
    hyps[:, :, 1:, :, 2] += 0.08 * torch.randn(V, frames, K - 1, 17, device="cuda", generator=g)      # all but one moved along the camera's depth axis
    hyps[..., 3] = torch.softmax(1.5 * torch.randn(V, frames, K, device="cuda", generator=g), dim=2)[..., None]
    P = torch.einsum("vfjc,vcd->vfjd", (pose + root[:, None])[None] - trans[0][:, None, None], R)
    kp = (intr[0, :, None, None, 0:2] * P[..., :2] / P[..., 2:3] + intr[0, :, None, None, 2:4] + 0.01 * torch.randn(V, frames, 17, 2, device="cuda", generator=g)).contiguous()
    return lib, V, (quat, trans, intr), pose, hyps, kp


def fuse_bench(argv):
    from manipose_amd import _lib
    from manipose_amd.data.ingest import h36m_cameras
    from manipose_amd.lift_ops import _path
    from manipose_amd.lift_views import _fuse, _fuse_place
    frames = int(argv[0]) if len(argv) > 0 else 3000
    K = int(argv[1]) if len(argv) > 1 else 5
    reps = int(argv[2]) if len(argv) > 2 else 200
    lib, V, (quat, trans, intr), pose, hyps, kp = fuse_scene(frames, K)
    one = torch.tensor([0, frames], dtype=torch.int64, device="cuda")
    fused = _fuse(lib, hyps, None, one, 1, quat, 0.02, 1.0)
    print(f"--fuse: {V} views x {frames} frames x {K} hypotheses, {hyps.numel() * 4 / 1e6:.2f} MB of hypotheses, {K ** V} combinations a frame; {reps} calls each "
          f"after 5 of warm-up (the output allocations are inside the time); hypothesis 0 chosen in {(fused[1] == 0).float().mean().item():.3f} of the views",
          flush=True)
    us = timed_us(lambda: _fuse(lib, hyps, None, one, 1, quat, 0.02, 1.0), reps)
    print(f"mp_lift_fuse: {us:,.1f} us  {frames / us:,.2f} M frames/s", flush=True)
    for iters in (0, 3):
        us = timed_us(lambda: _fuse_place(lib, fused[0], kp, None, one, 1, quat, trans, intr, None, True, iters), reps)
        steps = _fuse_place(lib, fused[0], kp, None, one, 1, quat, trans, intr, None, True, iters)[3].float().mean().item()
        print(f"mp_lift_fuse_place iters={iters}: {us:,.1f} us  {frames / us:,.2f} M frames/s; {steps:.2f} steps taken per frame", flush=True)
    us = timed_us(lambda: _path(lib, hyps[0], one, 1, 0.02, 0.0), reps)
    print(f"mp_lift_path on one view's {frames} frames x {K} hypotheses, for scale: {us:,.1f} us", flush=True)


def fuse_path_bench(argv):
    from manipose_amd.lift_views import _fuse, _fuse_path
    frames = int(argv[0]) if len(argv) > 0 else 3000
    K = int(argv[1]) if len(argv) > 1 else 5
    reps = int(argv[2]) if len(argv) > 2 else 20
    lib, V, (quat, _, _), _, hyps, _ = fuse_scene(frames, K)
    print(f"--fuse-path: {V} views x {frames} frames x {K} hypotheses, {K ** V} states a frame, {lib.mp_lift_fuse_path_scratch_bytes(V, frames, K) / 1e6:.2f} MB of "
          f"scratch; {reps} calls each after 5 of warm-up (the allocations of outputs and scratch are inside the time)", flush=True)
    for G in (1, 16):
        off = torch.tensor([frames * i // G for i in range(G + 1)], dtype=torch.int64, device="cuda")
        q = quat.expand(G, V, 4).contiguous()
        res = _fuse_path(lib, hyps, None, off, G, q, 0.02, 1.0, 0.02, 0.0)
        per = _fuse(lib, hyps, None, off, G, q, 0.02, 1.0)
        us = timed_us(lambda: _fuse_path(lib, hyps, None, off, G, q, 0.02, 1.0, 0.02, 0.0), reps)
        print(f"mp_lift_fuse_path, {G} take(s): {us:,.1f} us  {frames / us:,.3f} M frames/s  {us / (frames / G) * 1e3:,.0f} ns per frame of a take; choice differs from "
              f"mp_lift_fuse's in {(res[1] != per[1]).any(dim=1).float().mean().item():.3f} of the frames", flush=True)
    one = torch.tensor([0, frames], dtype=torch.int64, device="cuda")
    us = timed_us(lambda: _fuse(lib, hyps, None, one, 1, quat, 0.02, 1.0), 10 * reps)
    print(f"mp_lift_fuse on the same scene, for scale: {us:,.1f} us", flush=True)


def align_bench(argv):
    from manipose_amd import align_views
    from manipose_amd.data.ingest import h36m_cameras
    from manipose_amd.lift_views import _align
    frames = int(argv[0]) if len(argv) > 0 else 3000
    reps = int(argv[1]) if len(argv) > 1 else 20
    lib, V, (quat, trans, _), _, hyps, _ = fuse_scene(frames, 2)
    g = torch.Generator(device="cuda").manual_seed(2)
    swap = torch.rand(V, frames, device="cuda", generator=g) < 0.3           # 30 % of a view's frames take the hypothesis moved along the depth axis
    swap[0] = False
    poses = torch.where(swap[:, :, None, None], hyps[:, :, 1], hyps[:, :, 0]).contiguous()
    qn = quat[0] / quat[0].norm(dim=1, keepdim=True)
    w, x, y, z = qn.unbind(1)
    R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y), 2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                     2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], dim=1).view(V, 3, 3)
    root = torch.cat([2 * torch.rand(frames, 2, device="cuda", generator=g) - 1, 0.8 + 0.2 * torch.rand(frames, 1, device="cuda", generator=g)], dim=1)
    traj = torch.einsum("vfc,vcd->vfd", root[None] - trans[0][:, None], R).contiguous()      # R^T (root - T): every view's camera-space root
    traj_ok = torch.ones(V, frames, dtype=torch.uint8, device="cuda")
    print(f"--align: {V} views x {frames} frames x 17 joints, {poses.numel() * 4 / 1e6:.2f} MB of poses, 30 % of the frames of views 1..3 moved along the depth axis "
          f"(sigma 0.08 m); {reps} calls each after 5 of warm-up (the output allocations are inside the time)", flush=True)
    cams = h36m_cameras()["S11"]
    for iters in (0, 5):
        got = align_views(poses, None, None, traj, traj_ok, 0.05, iters, reference=cams[0])
        a, b = qn.double().cpu().numpy(), got.quat[0].double().cpu().numpy()     # the angle of conj(a) b by the arc tangent: accurate at small angles
        vec = a[:, :1] * b[:, 1:] - b[:, :1] * a[:, 1:] - np.cross(a[:, 1:], b[:, 1:])
        deg = np.degrees(2.0 * np.arctan2(np.linalg.norm(vec, axis=1), np.abs((a * b).sum(axis=1))))
        print(f"iters={iters}: off S11's calibration by {', '.join(f'{x:.3f}' for x in deg[1:])} degrees and "
              f"{', '.join(f'{d * 1e3:.1f}' for d in (got.trans[0] - trans[0]).norm(dim=1).tolist()[1:])} mm; rms {', '.join(f'{r * 1e3:.1f}' for r in got.rms[0].tolist()[1:])} mm",
              flush=True)
    for G in (1, 16):
        off = torch.tensor([frames * i // G for i in range(G + 1)], dtype=torch.int64, device="cuda")
        for iters, with_traj in ((0, False), (5, False), (5, True), (8, True)):
            t, k = (traj, traj_ok) if with_traj else (None, None)
            us = timed_us(lambda: _align(lib, poses, None, off, G, t, k, 0.05, iters), reps)
            passes = iters + (4 if with_traj else 2)
            print(f"mp_lift_align_views, {G} take(s), iters={iters}, {'with' if with_traj else 'no'} traj: {us:,.1f} us  {passes} passes, {us / passes:,.1f} us a pass", flush=True)


def sync_bench(argv):
    from manipose_amd import _lib, sync_views
    from manipose_amd.lift_views import _shift, _sync
    frames = int(argv[0]) if len(argv) > 0 else 3000
    reps = int(argv[1]) if len(argv) > 1 else 20
    assert torch.cuda.is_available(), "needs an MI355X"
    lib, V, J, K = _lib.load(), 4, 17, 5
    true = torch.tensor([0.0, 3.0, -7.5, 12.25], device="cuda")
    g = torch.Generator(device="cuda").manual_seed(3)
    rnd = lambda *shape: torch.rand(*shape, device="cuda", generator=g)
    rest, amp = 0.3 * torch.randn(J, 3, device="cuda", generator=g), 0.1 * torch.randn(4, J, 3, device="cuda", generator=g)
    freq, phase = 2 * np.pi / (20 + 100 * rnd(4, J, 3)), 2 * np.pi * rnd(4, J, 3)
    time = torch.arange(frames, device="cuda")[None, :] - true[:, None]                              # frame f of view v shows time f - lag_v
    body = rest + (amp * torch.sin(freq * time[:, :, None, None, None] + phase)).sum(dim=2)          # (V, frames, J, 3): a motion smooth in time
    body[:, :, 0] = 0
    poses = torch.empty_like(body)
    for v in range(V):                                                                               # every view in a camera frame of its own, 10 mm of noise
        q = torch.randn(4, device="cuda", generator=g)
        w, x, y, z = (q / q.norm()).tolist()
        R = torch.tensor([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                          [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]], device="cuda")
        poses[v] = body[v] @ R.T + 0.01 * torch.randn(frames, J, 3, device="cuda", generator=g)
    poses = poses.contiguous()
    hyps = torch.randn(V, frames, K, J, 4, device="cuda", generator=g)
    sig_mb = (poses.numel() * 4 + V * frames * (J - 1) * 8) / 1e6
    pair_mb = (V - 1) * 2 * frames * (J - 1) * 8 / 1e6
    print(f"--sync: {V} views x {frames} frames x {J} joints, {poses.numel() * 4 / 1e6:.2f} MB of poses; {reps} calls each after 5 of warm-up (the output and "
          f"scratch allocations are inside the time).  At least once: the signal kernel reads the poses and writes the signals ({sig_mb:.2f} MB), the curve "
          f"kernel reads a view's and the reference's signals per view ({pair_mb:.2f} MB)", flush=True)
    got = sync_views(poses)
    print(f"defaults: lags {', '.join(f'{x:.3f}' for x in got.lag[0].tolist())} (true {', '.join(f'{x:g}' for x in true.tolist())}), contrast "
          f"{', '.join(f'{x:.2f}' for x in got.contrast[0].tolist())}, ok {got.ok[0].tolist()}", flush=True)
    for G in (1, 16):
        off = torch.tensor([frames * i // G for i in range(G + 1)], dtype=torch.int64, device="cuda")
        for L in (0, 32, 256):
            us = timed_us(lambda: _sync(lib, poses, None, off, G, L, 16, 0.05), reps)
            terms = (2 * L + 1) * frames * (J - 1) * (V - 1)
            print(f"mp_lift_sync_views, {G} take(s), max_lag={L}: {us:,.1f} us  {2 * L + 1} lags, at most {terms / 1e6:,.1f} M terms, {terms / us / 1e3:,.2f} G terms/s; "
                  f"{(sig_mb + pair_mb) / us * 1e3:,.1f} GB/s of the bytes to move once", flush=True)
    one = torch.tensor([0, frames], dtype=torch.int64, device="cuda")
    for name, x in (("poses (51 floats a frame)", poses), ("hypotheses (340 floats a frame)", hyps)):
        for mode, code in (("nearest", 0), ("linear", 1)):
            us = timed_us(lambda: _shift(lib, x, None, one, 1, got.lag, code), reps)
            mb = 2 * x.numel() * 4 / 1e6
            print(f"mp_lift_shift_views, {mode}, {name}: {us:,.1f} us  read once, write once {mb:.2f} MB: {mb / us * 1e3:,.1f} GB/s", flush=True)


def bundle_bench(argv):
    from manipose_amd.lift_views import _bundle, _fuse_place
    frames = int(argv[0]) if len(argv) > 0 else 3000
    reps = int(argv[1]) if len(argv) > 1 else 20
    lib, V, (quat, trans, intr), pose, _, kp = fuse_scene(frames, 2)
    g = np.random.default_rng(3)
    qn = (quat[0] / quat[0].norm(dim=1, keepdim=True)).double().cpu().numpy()
    q0, t0 = qn.copy(), trans[0].double().cpu().numpy()
    for v in range(1, V):                                                 # views 1..3 start 0.3 degrees and 0.15 m off
        axis, d = g.standard_normal(3), g.standard_normal(3)
        h = 0.5 * np.radians(0.3)
        b = np.concatenate([[np.cos(h)], np.sin(h) * axis / np.linalg.norm(axis)])
        a = qn[v]
        q0[v] = [a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3], a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                 a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1], a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0]]
        t0[v] += 0.15 * d / np.linalg.norm(d)

    def off_by(q, t):
        a, b = qn, q.double().cpu().numpy()
        vec = a[:, :1] * b[:, 1:] - b[:, :1] * a[:, 1:] - np.cross(a[:, 1:], b[:, 1:])
        deg = np.degrees(2.0 * np.arctan2(np.linalg.norm(vec, axis=1), np.abs((a * b).sum(axis=1))))
        return (f"{', '.join(f'{x:.4f}' for x in deg[1:])} degrees and "
                f"{', '.join(f'{x * 1e3:.2f}' for x in (t - trans[0]).norm(dim=1).tolist()[1:])} mm")

    print(f"--bundle: {V} views x {frames} frames x 17 joints, pinhole keypoints with 0.01 of noise, sigma = inf; {reps} calls each after 5 of warm-up "
          f"(the allocations of outputs and scratch are inside the time)", flush=True)
    fixed = torch.tensor([[1, 0, 0, 0]], dtype=torch.uint8, device="cuda")
    for G in (1, 16):
        off = torch.tensor([frames * i // G for i in range(G + 1)], dtype=torch.int64, device="cuda")
        q = torch.from_numpy(q0.astype(np.float32)).cuda().expand(G, V, 4).contiguous()
        t = torch.from_numpy(t0.astype(np.float32)).cuda().expand(G, V, 3).contiguous()
        k = intr.expand(G, V, 9).contiguous()
        root, _, ok, _ = _fuse_place(lib, pose, kp, None, off, G, q, t, k, None, False, 3)
        call = lambda iters: _bundle(lib, pose, root, ok, kp, None, off, G, q, t, k, fixed.expand(G, V).contiguous(), None, False, float("inf"), iters)
        if G == 1:
            print(f"start: off S11's calibration by {off_by(q[0], t[0])}", flush=True)
        for iters in (0, 1, 3, 8):
            res = call(iters)
            us = timed_us(lambda: call(iters), reps)
            print(f"mp_lift_bundle_views, {G} take(s), iters={iters}: {us:,.1f} us  {iters + 1} passes, {us / (iters + 1):,.1f} us a pass; take 0: {int(res[5][0])} steps, "
                  f"cost {res[4][0, 0].item():.4f} -> {res[4][0, 1].item():.4f}, off by {off_by(res[0][0], res[1][0])}", flush=True)


def calibrate_bench(argv):
    from manipose_amd.lift_views import _bundle, _calibrate, _fuse_place
    frames = int(argv[0]) if len(argv) > 0 else 3000
    reps = int(argv[1]) if len(argv) > 1 else 20
    lib, V, (quat, trans, intr), pose, _, kp = fuse_scene(frames, 2)
    g = np.random.default_rng(3)
    q0 = (quat[0] / quat[0].norm(dim=1, keepdim=True)).double().cpu().numpy()
    t0 = trans[0].double().cpu().numpy()
    for v in range(1, V):                                                 # views 1..3 start 0.3 degrees and 0.15 m off, as in --bundle
        axis, d = g.standard_normal(3), g.standard_normal(3)
        h = 0.5 * np.radians(0.3)
        b = np.concatenate([[np.cos(h)], np.sin(h) * axis / np.linalg.norm(axis)])
        a = q0[v].copy()
        q0[v] = [a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3], a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                 a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1], a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0]]
        t0[v] += 0.15 * d / np.linalg.norm(d)
    print(f"--calibrate: {V} views x {frames} frames x 17 joints, ONE take, pinhole keypoints with 0.01 of noise, prior 1e-3, sigma 0.05; {reps} calls each "
          f"after 5 of warm-up (the allocations of outputs and scratch are inside the time); synthetic data", flush=True)
    fixed = torch.tensor([[1, 0, 0, 0]], dtype=torch.uint8, device="cuda")
    off = torch.tensor([0, frames], dtype=torch.int64, device="cuda")
    q = torch.from_numpy(q0.astype(np.float32)).cuda().reshape(1, V, 4).contiguous()
    t = torch.from_numpy(t0.astype(np.float32)).cuda().reshape(1, V, 3).contiguous()
    k = intr.reshape(1, V, 9).clone()
    root, _, ok, _ = _fuse_place(lib, pose, kp, None, off, 1, q, t, k, None, False, 3)
    start = (pose + root[:, None]).contiguous()
    k0 = k.clone()
    k0[0, :, :2] *= torch.tensor([1.10, 0.90, 1.07, 0.92], device="cuda")[:V, None]
    err = lambda x: ", ".join(f"{e:.4f}" for e in (x[0, :, 0] / k[0, :, 0] - 1).abs().tolist())
    print(f"start: focal lengths off S11's by {err(k0)}", flush=True)
    for iters in (0, 1, 3):
        cal = lambda: _calibrate(lib, start, ok, kp, None, off, 1, q, t, k0, fixed, None, True, False, 0.05, 1e-3, iters)
        bun = lambda: _bundle(lib, pose, root, ok, kp, None, off, 1, q, t, k, fixed, None, False, 0.05, iters)
        res = cal()
        us, us_b = timed_us(cal, reps), timed_us(bun, reps)
        print(f"mp_lift_calibrate_views, iters={iters}: {us:,.1f} us  {iters + 1} passes, {us / (iters + 1):,.1f} us a pass; {int(res[6][0])} steps, cost "
              f"{res[5][0, 0].item():.4f} -> {res[5][0, 1].item():.4f}, focal lengths off by {err(res[2])};  mp_lift_bundle_views, iters={iters}: {us_b:,.1f} us "
              f"({us / us_b:.2f} x)", flush=True)


def triangulate_bench(argv):
    from manipose_amd import _lib
    from manipose_amd.lift_ops import _launch
    from manipose_amd.lift_views import _fuse_place, _triangulate
    frames = int(argv[0]) if len(argv) > 0 else 3000
    reps = int(argv[1]) if len(argv) > 1 else 20
    lib, V, (quat, trans, intr), pose, _, kp = fuse_scene(frames, 2)
    g = torch.Generator(device="cuda").manual_seed(4)
    lifted = pose + 0.03 * torch.randn(frames, 17, 3, device="cuda", generator=g)      # the lifted body: 0.03 m N(0, 1) off per coordinate
    lifted[:, 0] = 0
    print(f"--triangulate: {V} views x {frames} frames x 17 joints = {frames * 17} items, pinhole keypoints with 0.01 of noise, the lifted pose 0.03 m N(0, 1) off, "
          f"sigma = inf, prior = 0; {reps} calls each after 5 of warm-up (the output allocations are inside the time)", flush=True)
    for G in (1, 16):
        off = torch.tensor([frames * i // G for i in range(G + 1)], dtype=torch.int64, device="cuda")
        q, t, k = quat.expand(G, V, 4).contiguous(), trans.expand(G, V, 3).contiguous(), intr.expand(G, V, 9).contiguous()
        place = lambda: _fuse_place(lib, lifted, kp, None, off, G, q, t, k, None, False, 3)
        root, _, ok, _ = place()
        us = timed_us(place, reps)
        print(f"mp_lift_fuse_place, {G} take(s), iters=3, on the same frames: {us:,.1f} us", flush=True)
        for iters in (0, 1, 3):
            call = lambda: _triangulate(lib, lifted, root, ok, kp, None, None, off, G, q, t, k, False, float("inf"), 0.0, iters)
            res = call()
            us = timed_us(call, reps)
            moved = (res.points - (lifted + root[:, None])).norm(dim=2).mean().item()
            direct = lambda: _launch(res.points.device, "mp_lift_triangulate", _lib.ptr(lifted), _lib.ptr(root), _lib.ptr(ok), _lib.ptr(kp), None, V, frames, 17, None,
                                     _lib.ptr(off), G, _lib.ptr(q), _lib.ptr(t), _lib.ptr(k), 0, float("inf"), 0.0, iters, _lib.ptr(res.points), _lib.ptr(res.err),
                                     _lib.ptr(res.views), _lib.ptr(res.ok), _lib.ptr(res.steps))
            alone = timed_us(direct, reps)                                # the entry point into outputs allocated once: the kernel without the launcher's five fills
            print(f"mp_lift_triangulate, {G} take(s), iters={iters}: {us:,.1f} us ({alone:,.1f} us into outputs allocated once)  {frames * 17 / us:,.2f} M items/s; {res.steps.float().mean().item():.2f} steps an item, "
                  f"{(res.ok == 3).float().mean().item():.3f} triangulated, mean reprojection {res.err.mean().item():.5f}, {moved * 1e3:.1f} mm from the lifted pose plus root "
                  f"and {(res.points - (pose + root[:, None])).norm(dim=2).mean().item() * 1e3:.1f} mm from the true pose plus the fitted root", flush=True)


def skeleton_bench(argv):
    from manipose_amd import _lib
    from manipose_amd.lift_ops import _launch, _parents_c, _skeleton_of
    from manipose_amd.lift_views import SKELETON_PRIOR, _fit_skeleton, _fuse_place, _median_bones, _triangulate
    frames = int(argv[0]) if len(argv) > 0 else 3000
    reps = int(argv[1]) if len(argv) > 1 else 20
    lib, V, (quat, trans, intr), pose, _, kp = fuse_scene(frames, 2)
    g = torch.Generator(device="cuda").manual_seed(4)
    lifted = pose + 0.03 * torch.randn(frames, 17, 3, device="cuda", generator=g)      # the lifted body: 0.03 m N(0, 1) off per coordinate
    lifted[:, 0] = 0
    parents = _parents_c(_skeleton_of(), 17)
    print(f"--skeleton: {V} views x {frames} frames x 17 joints, one workgroup a frame, pinhole keypoints with 0.01 of noise, the start the triangulated joints, "
          f"the median bone table, sigma = inf, prior = {SKELETON_PRIOR}; {reps} calls each after 5 of warm-up (the output allocations are inside the time)", flush=True)
    for G in (1, 16):
        off = torch.tensor([frames * i // G for i in range(G + 1)], dtype=torch.int64, device="cuda")
        q, t, k = quat.expand(G, V, 4).contiguous(), trans.expand(G, V, 3).contiguous(), intr.expand(G, V, 9).contiguous()
        root, _, ok, _ = _fuse_place(lib, lifted, kp, None, off, G, q, t, k, None, False, 3)
        tri = lambda: _triangulate(lib, lifted, root, ok, kp, None, None, off, G, q, t, k, False, float("inf"), 0.0, 3)
        start = tri().points
        print(f"mp_lift_triangulate, {G} take(s), iters=3, on the same frames: {timed_us(tri, reps):,.1f} us", flush=True)
        table = _median_bones(start, None, off, G, [int(p) for p in parents])
        for iters in (0, 1, 3):
            call = lambda: _fit_skeleton(lib, start, None, kp, None, None, off, G, q, t, k, table, parents, False, float("inf"), SKELETON_PRIOR, iters)
            res = call()
            us = timed_us(call, reps)
            direct = lambda: _launch(start.device, "mp_lift_fit_skeleton", _lib.ptr(start), None, _lib.ptr(kp), None, V, frames, 17, None, _lib.ptr(off), G,
                                     _lib.ptr(q), _lib.ptr(t), _lib.ptr(k), _lib.ptr(table), parents, 0, float("inf"), float(SKELETON_PRIOR), iters, _lib.ptr(res[0]),
                                     _lib.ptr(res[1]), _lib.ptr(res[2]), _lib.ptr(res[3]))
            alone = timed_us(direct, reps)                                # the entry point into outputs allocated once: the kernel without the launcher's four fills
            print(f"mp_lift_fit_skeleton, {G} take(s), iters={iters}: {us:,.1f} us ({alone:,.1f} us into outputs allocated once: {alone * 1e3 / frames:,.1f} ns a frame); "
                  f"{res[3].float().mean().item():.2f} steps a frame, {(res[2] == 3).float().mean().item():.3f} with a result, mean reprojection "
                  f"{res[1][:, 0].mean().item():.5f} -> {res[1][:, 1].mean().item():.5f}, {(res[0] - start).norm(dim=2).mean().item() * 1e3:.1f} mm from the start", flush=True)


def skeleton_smooth_bench(argv):
    from manipose_amd import _lib
    from manipose_amd.lift_ops import _launch, _parents_c, _skeleton_of
    from manipose_amd.lift_views import SKELETON_PRIOR, _fit_skeleton, _fit_skeleton_smooth, _fuse_place, _median_bones, _triangulate
    frames = int(argv[0]) if len(argv) > 0 else 3000
    reps = int(argv[1]) if len(argv) > 1 else 20
    lib, V, (quat, trans, intr), pose, _, kp = fuse_scene(frames, 2)
    g = torch.Generator(device="cuda").manual_seed(4)
    lifted = pose + 0.03 * torch.randn(frames, 17, 3, device="cuda", generator=g)      # the lifted body: 0.03 m N(0, 1) off per coordinate
    lifted[:, 0] = 0
    parents = _parents_c(_skeleton_of(), 17)
    smooth = 0.1
    print(f"--skeleton-smooth: {V} views x {frames} frames x 17 joints, one workgroup a frame, --skeleton's scene and start, the median bone table, sigma = inf, "
          f"prior = {SKELETON_PRIOR}, iters = 3, smooth = {smooth}; {reps} calls each after 5 of warm-up (the output allocations are inside the first time)", flush=True)
    for G in (1, 16):
        off = torch.tensor([frames * i // G for i in range(G + 1)], dtype=torch.int64, device="cuda")
        q, t, k = quat.expand(G, V, 4).contiguous(), trans.expand(G, V, 3).contiguous(), intr.expand(G, V, 9).contiguous()
        root, _, ok, _ = _fuse_place(lib, lifted, kp, None, off, G, q, t, k, None, False, 3)
        start = _triangulate(lib, lifted, root, ok, kp, None, None, off, G, q, t, k, False, float("inf"), 0.0, 3).points
        table = _median_bones(start, None, off, G, [int(p) for p in parents])
        base = {}
        for iters in (1, 3):
            res = _fit_skeleton(lib, start, None, kp, None, None, off, G, q, t, k, table, parents, False, float("inf"), SKELETON_PRIOR, iters)
            direct = lambda: _launch(start.device, "mp_lift_fit_skeleton", _lib.ptr(start), None, _lib.ptr(kp), None, V, frames, 17, None, _lib.ptr(off), G,
                                     _lib.ptr(q), _lib.ptr(t), _lib.ptr(k), _lib.ptr(table), parents, 0, float("inf"), float(SKELETON_PRIOR), iters, _lib.ptr(res[0]),
                                     _lib.ptr(res[1]), _lib.ptr(res[2]), _lib.ptr(res[3]))
            base[iters] = timed_us(direct, reps)
            print(f"mp_lift_fit_skeleton, {G} take(s), iters={iters}: {base[iters]:,.1f} us into outputs allocated once", flush=True)
        alone = {}
        for sweeps in (1, 8):
            call = lambda: _fit_skeleton_smooth(lib, start, None, kp, None, None, off, G, q, t, k, table, parents, False, float("inf"), SKELETON_PRIOR, 3, smooth, sweeps)
            res = call()
            us = timed_us(call, reps)
            n = int(lib.mp_lift_fit_skeleton_smooth_scratch_bytes(frames, 17))
            scratch = torch.empty(n // 8, dtype=torch.float64, device="cuda")
            direct = lambda: _launch(start.device, "mp_lift_fit_skeleton_smooth", _lib.ptr(start), None, _lib.ptr(kp), None, V, frames, 17, None, _lib.ptr(off), G,
                                     _lib.ptr(q), _lib.ptr(t), _lib.ptr(k), _lib.ptr(table), parents, 0, float("inf"), float(SKELETON_PRIOR), 3, smooth, sweeps,
                                     _lib.ptr(res[0]), _lib.ptr(res[1]), _lib.ptr(res[2]), _lib.ptr(res[3]), _lib.ptr(res[4]), _lib.ptr(scratch), n)
            alone[sweeps] = timed_us(direct, reps)
            sd = lambda p: (p[:-2] - 2 * p[1:-1] + p[2:]).norm(dim=2).mean().item() * 1e3
            print(f"mp_lift_fit_skeleton_smooth, {G} take(s), sweeps={sweeps}: {us:,.1f} us ({alone[sweeps]:,.1f} us into outputs allocated once); "
                  f"{res[4].float().mean().item():.2f} accepted visits a frame, mean reprojection {res[1][:, 1].mean().item():.5f} -> {res[1][:, 2].mean().item():.5f}, "
                  f"mean second difference {sd(res[0]):.2f} mm a frame^2 (the start's {sd(start):.2f})", flush=True)
        sweep = (alone[8] - alone[1]) / 7
        print(f"  one sweep (three launches), {G} take(s): {sweep:,.1f} us = {sweep / base[1]:.2f} x the iters=1 call, {sweep / base[3]:.2f} x the iters=3 call; "
              f"stage A and one sweep together {alone[1]:,.1f} us", flush=True)


def ground_walker(n, seed):
    """a walker on a tilted floor: a 40-frame step cycle, 60 % stance, 5 mm of noise, 17 joints"""
    g = np.random.default_rng(seed)
    f = np.arange(n)
    pts = np.zeros((n, 17, 3))
    for k, j in enumerate((3, 6)):
        c, t = np.divmod(f + 20 * k, 40)
        u = np.clip((t - 23) / 17.0, 0.0, 1.0)
        e = 0.5 - 0.5 * np.cos(np.pi * u)
        pts[:, j] = np.stack([0.6 * (c + e) + 0.3 * k, np.full(n, 0.2 * k - 0.1) + 0.5 * np.sin(0.4 * (c + e)), 0.12 * np.sin(np.pi * u)], axis=1)
    centre = 0.5 * (pts[:, 3] + pts[:, 6]) * [1, 1, 0]
    pts[:, [0, 1, 2, 4, 5, 7, 9, 10, 11, 12, 13, 14, 15, 16]] = (centre + [0, 0, 0.9])[:, None] + 0.25 * g.standard_normal((14, 3))
    pts[:, 0], pts[:, 8] = centre + [0, 0, 0.9], centre + [0, 0, 1.4]
    pts += 0.005 * g.standard_normal(pts.shape)
    a, b = 0.4, -0.3                                                   # a tilt of the floor: about x, then about y
    R = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]]) @ np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    return (pts @ R.T + [1.0, -2.0, 3.0]).astype(np.float32), R[:, 2]


def ground_scenes(lib, S, n):
    """S walkers of n frames laid end to end and mp_lift_ground on them at the defaults: (the walkers, points, seq_offset, a launcher by iters)"""
    from manipose_amd.lift_ops import _ground
    scenes = [ground_walker(n, 100 * S + s) for s in range(S)]
    pts = torch.from_numpy(np.concatenate([p for p, _ in scenes])).cuda()
    off = torch.tensor([n * s for s in range(S + 1)], dtype=torch.int64, device="cuda")
    return scenes, pts, off, lambda iters=5: _ground(lib, pts, None, off, S, (3, 6), (0, 8), 2, 0.01, 0.03, 0.05, iters, 0.0)


def ground_bench(argv):
    from manipose_amd import _lib
    frames = int(argv[0]) if len(argv) > 0 else 3000
    reps = int(argv[1]) if len(argv) > 1 else 20
    lib = _lib.load()
    print(f"--ground: walkers of 17 joints on a tilted floor, 5 mm of noise, the defaults (radius 2, speed 0.01, sigma 0.03, prior 0.05, iters 5: 13 passes); "
          f"{reps} calls each after 5 of warm-up (the output allocations are inside the time)", flush=True)
    for S, n in ((1, frames), (64, max(frames // 10, 1))):
        scenes, pts, off, run = ground_scenes(lib, S, n)
        got = run()
        torch.cuda.synchronize()
        cos = np.clip((got.normal.double().cpu().numpy() * np.stack([u for _, u in scenes])).sum(axis=1), -1, 1)
        print(f"{S} sequence(s) of {n} frames: ok {sorted(set(got.ok.tolist()))}, {int(got.used.sum())} contacts, the normal off the floor's by at most "
              f"{np.degrees(np.arccos(cos)).max():.3f} degrees, rms {1e3 * float(got.rms.max()):.2f} mm, skate {1e3 * float(got.skate.max()):.2f} mm a frame", flush=True)
        for iters in (0, 5, 8):
            us = timed_us(lambda: run(iters), reps)
            print(f"mp_lift_ground, {S} sequence(s) of {n} frames, iters={iters}: {us:,.1f} us  (contact kernel + {2 * (iters + 1) + 1} passes of the plane kernel)", flush=True)


def footlock_bench(argv):
    from manipose_amd import _lib
    from manipose_amd.lift_ops import _footlock
    frames = int(argv[0]) if len(argv) > 0 else 3000
    reps = int(argv[1]) if len(argv) > 1 else 20
    lib = _lib.load()
    print(f"--footlock: --ground's walkers of 17 joints, their contacts and planes under the ground defaults, legs (1, 2, 3) and (4, 5, 6), stretch 1; "
          f"{reps} calls each after 5 of warm-up (the output allocations are inside the time)", flush=True)
    for S, n in ((1, frames), (64, max(frames // 10, 1))):
        _, pts, off, run = ground_scenes(lib, S, n)
        got = run()
        torch.cuda.synchronize()
        legs, floor = ((1, 2, 3), (4, 5, 6)), (got.normal, got.offset, got.ok)
        lock = lambda blend=5, fl=floor: _footlock(lib, pts, got.contact, None, off, S, legs, fl, blend, 1.0)
        out, runlen, target, moved, flags, runs = lock()
        torch.cuda.synchronize()
        n_lock = int((flags & 1 != 0).sum())
        # what must move, per frame: the copy reads and writes J C floats; per (frame, foot) the run kernel reads contact (1 byte) and writes run (4)
        # twice over, and where the foot is lockable reads three joints (36) and reads and writes the anchor (12 + 12); the pose kernel reads
        # run (4, in both launches), three joints (36) and, in a run, the anchor (12), and writes target, moved, flags (17) and two joints (24)
        nf, total = 2, S * n
        nbytes = total * 2 * 17 * 3 * 4 + total * nf * (1 + 4 + 4 + 4) + n_lock * (36 + 24) + total * nf * (8 + 36 + 17 + 24) + n_lock * 12
        print(f"{S} sequence(s) of {n} frames: {int(runs.sum())} runs, {n_lock} of {total * nf} (frame, foot)s pinned, {int((flags & 2 != 0).sum())} eased, "
              f"{int((flags & 4 != 0).sum())} reach clamped, {int((flags & 8 != 0).sum())} lifted onto the floor; the longest run {int(runlen.max())} frames, "
              f"an ankle moved by {1e3 * float(moved.max()):.1f} mm at most; {nbytes / 1e6:.2f} MB must move", flush=True)
        for blend, fl, word in ((0, floor, "floor"), (5, floor, "floor"), (32, floor, "floor"), (5, None, "no floor")):
            us = timed_us(lambda: lock(blend, fl), reps)
            print(f"mp_lift_footlock, {S} sequence(s) of {n} frames, blend={blend}, {word}: {us:,.1f} us  (a copy and three launches; {nbytes / 1e6:.2f} MB: "
                  f"{nbytes / us / 1e3:,.1f} GB/s)", flush=True)


def retime_bench(argv):
    from manipose_amd import _lib
    from manipose_amd import lift_args
    from manipose_amd.lift_ops import _fk, _parents_c, _rest_c, _retime, _skeleton_of, _smooth
    frames = int(argv[0]) if len(argv) > 0 else 3000
    reps = int(argv[1]) if len(argv) > 1 else 20
    lib = _lib.load()
    J = 17
    sk = _skeleton_of()
    parents, rest = _parents_c(sk, J), _rest_c(sk, J)
    print(f"--retime: a smooth synthetic take of {J} joints (every joint turns at up to 0.03 rad a frame), 10 % of the frames invalid, degree 2, biweight; "
          f"{reps} calls each after 5 of warm-up (the output allocations are inside the time)", flush=True)
    for S, n in ((1, frames), (64, max(frames // 10, 1))):
        g = np.random.default_rng(S)
        t = np.arange(n, dtype=np.float64)[None, :, None]
        axis = g.standard_normal((S, 1, J, 3))
        axis /= np.sqrt((axis * axis).sum(-1))[..., None]
        ang = 0.5 * (g.uniform(-0.03, 0.03, (S, 1, J)) * t + 0.2 * np.sin(g.uniform(0.02, 0.08, (S, 1, J)) * t))
        q = np.concatenate([np.cos(ang)[..., None], np.sin(ang)[..., None] * axis], axis=-1).reshape(S * n, 1, J, 4).astype(np.float32)
        quat = torch.from_numpy(q).cuda()
        root = torch.from_numpy(g.standard_normal((S * n, 1, 3)).astype(np.float32)).cuda()
        valid = torch.from_numpy((g.uniform(size=(S * n, 1)) > 0.1).astype(np.uint8)).cuda()
        bones = torch.from_numpy(g.uniform(0.1, 0.5, (S, J - 1)).astype(np.float32)).cuda()
        seq = [n * s for s in range(S + 1)]
        for fps_out in (50, 30, 60):
            off, out_off, clock, _ = lift_args.retime_plan(seq, S * n, 50, fps_out, 0.0)
            d_off, d_out, d_clock = (torch.from_numpy(a).cuda() for a in (off, out_off, clock))
            mtot = int(out_off[-1])
            for R in (0, 4, 64):
                call = lambda: _retime(lib, quat, root, valid, d_off, d_out, d_clock, S, mtot, R, 2, "biweight")
                got = call()
                torch.cuda.synchronize()
                taps = int(got[3].sum())
                # requested per tap: a validity byte, a root (12) and J quaternions (16 J); for R >= 1 the validity bytes of the window twice over
                # (the moments, then the coefficients) and the reference frame's quaternions; written per output pose: 16 J + 12 + 2
                nbytes = taps * (1 + 12 + 16 * J) + mtot * (16 * J + 12 + 2) + (mtot * (2 * (2 * R + 1) + 16 * J) if R else 0)
                us = timed_us(call, reps)
                line = (f"mp_lift_retime, {S} sequence(s) of {n} frames, 50 -> {fps_out} fps ({mtot} output frames), radius={R}: {us:,.1f} us  ({taps / mtot:.1f} taps a "
                        f"frame, {int((got[2] & 1 == 0).sum())} frames without a result; {nbytes / 1e6:.2f} MB requested and written: {nbytes / us / 1e3:,.1f} GB/s)")
                if R and fps_out == 50:
                    sm = timed_us(lambda: _smooth(lib, quat, valid, d_off, S, R, 2, "biweight"), reps)
                    line += f"; mp_lift_smooth on the same quaternions as (Ntot, 1, {J}, 4) values, radius={R}: {sm:,.1f} us"
                print(line, flush=True)
            fk = lambda: _fk(lib, got[0], got[1], bones, d_out, S, parents, rest, False)
            fk()
            us = timed_us(fk, reps)
            nbytes = mtot * (16 * J + 12 + 4 * (J - 1) + 12 * J + 1)
            print(f"mp_lift_fk, {S} sequence(s), {mtot} frames (the retimed take at {fps_out} fps): {us:,.1f} us  ({nbytes / 1e6:.2f} MB read and written: "
                  f"{nbytes / us / 1e3:,.1f} GB/s)", flush=True)


def bvh_bench(argv):
    from manipose_amd import _lib
    from manipose_amd.lift_ops import _euler
    frames = int(argv[0]) if len(argv) > 0 else 3000
    reps = int(argv[1]) if len(argv) > 1 else 20
    lib = _lib.load()
    J = 17
    print(f"--bvh: a synthetic take of {J} joints, every joint spinning at up to 0.25 rad a frame (the angles cross their branch cuts every few frames), "
          f"10 % of the frames invalid, order ZXY, scale 100, a basis and a shift per sequence; {reps} calls each after 5 of warm-up (the output "
          f"allocations are inside the time)", flush=True)
    for S, n in ((1, frames), (64, frames)):
        g = np.random.default_rng(S)
        t = np.arange(n, dtype=np.float64)[None, :, None]
        axis = g.standard_normal((S, 1, J, 3))
        axis /= np.sqrt((axis * axis).sum(-1))[..., None]
        ang = 0.5 * (g.uniform(-0.25, 0.25, (S, 1, J)) * t + g.uniform(0, 6, (S, 1, J)))
        q = np.concatenate([np.cos(ang)[..., None], np.sin(ang)[..., None] * axis], axis=-1).reshape(S * n, 1, J, 4).astype(np.float32)
        quat = torch.from_numpy(q).cuda()
        root = torch.from_numpy(g.standard_normal((S * n, 1, 3)).astype(np.float32)).cuda()
        valid = torch.from_numpy((g.uniform(size=(S * n, 1)) > 0.1).astype(np.uint8)).cuda()
        b = g.standard_normal((S, 4))
        basis = torch.from_numpy((b / np.sqrt((b * b).sum(-1))[:, None]).astype(np.float32)).cuda()
        shift = torch.from_numpy(g.standard_normal((S, 3)).astype(np.float32)).cuda()
        d_off = torch.tensor([n * s for s in range(S + 1)], dtype=torch.int64).cuda()
        one = lambda: _euler(lib, quat, root, valid, d_off, S, basis, shift, 100.0, "ZXY", False)
        both = lambda: _euler(lib, quat, root, valid, d_off, S, basis, shift, 100.0, "ZXY", True)
        got = both()
        torch.cuda.synchronize()
        live = int((got[2] != 0).sum())
        first = S * n * (16 * J + 12 + 1 + 12 * J + 12 + 1)              # quaternions, root, valid in; angles, pos, ok out
        second = S * n * (12 * J + J) + live * 12 * J                    # angles and (once per joint's wave) ok in; the frames with a result out
        us1, us2 = timed_us(one, reps), timed_us(both, reps)
        print(f"mp_lift_euler, {S} sequence(s) of {n} frames, first pass: {us1:,.1f} us  ({first / 1e6:.2f} MB: {first / us1 / 1e3:,.1f} GB/s); both passes: "
              f"{us2:,.1f} us; the second pass ({S * J} tracks, {-(-n // 64)} chunks each): {us2 - us1:,.1f} us  ({second / 1e6:.2f} MB: "
              f"{second / max(us2 - us1, 1e-9) / 1e3:,.1f} GB/s); {S * n - live} frames without a result, largest |angle| {float(got[0].abs().max()):,.0f} degrees",
              flush=True)


if "--bvh" in sys.argv:
    bvh_bench([a for a in sys.argv[1:] if a != "--bvh"])
    sys.exit(0)
if "--retime" in sys.argv:
    retime_bench([a for a in sys.argv[1:] if a != "--retime"])
    sys.exit(0)
if "--footlock" in sys.argv:
    footlock_bench([a for a in sys.argv[1:] if a != "--footlock"])
    sys.exit(0)
if "--ground" in sys.argv:
    ground_bench([a for a in sys.argv[1:] if a != "--ground"])
    sys.exit(0)
if "--skeleton-smooth" in sys.argv:
    skeleton_smooth_bench([a for a in sys.argv[1:] if a != "--skeleton-smooth"])
    sys.exit(0)
if "--skeleton" in sys.argv:
    skeleton_bench([a for a in sys.argv[1:] if a != "--skeleton"])
    sys.exit(0)
if "--calibrate" in sys.argv:
    calibrate_bench([a for a in sys.argv[1:] if a != "--calibrate"])
    sys.exit(0)
if "--triangulate" in sys.argv:
    triangulate_bench([a for a in sys.argv[1:] if a != "--triangulate"])
    sys.exit(0)
if "--bundle" in sys.argv:
    bundle_bench([a for a in sys.argv[1:] if a != "--bundle"])
    sys.exit(0)
if "--sync" in sys.argv:
    sync_bench([a for a in sys.argv[1:] if a != "--sync"])
    sys.exit(0)
if "--align" in sys.argv:
    align_bench([a for a in sys.argv[1:] if a != "--align"])
    sys.exit(0)
if "--fuse-path" in sys.argv:
    fuse_path_bench([a for a in sys.argv[1:] if a != "--fuse-path"])
    sys.exit(0)
if "--fuse" in sys.argv:
    fuse_bench([a for a in sys.argv[1:] if a != "--fuse"])
    sys.exit(0)
if "--rotations" in sys.argv:
    rotations_bench([a for a in sys.argv[1:] if a != "--rotations"])
    sys.exit(0)
if "--score" in sys.argv:
    score_bench([a for a in sys.argv[1:] if a != "--score"])
    sys.exit(0)
if "--path" in sys.argv:
    path_bench([a for a in sys.argv[1:] if a != "--path"])
    sys.exit(0)
if "--place" in sys.argv:
    place_bench([a for a in sys.argv[1:] if a != "--place"])
    sys.exit(0)
W = int(sys.argv[1]) if len(sys.argv) > 1 else 158
T = int(sys.argv[2]) if len(sys.argv) > 2 else 243
K = int(sys.argv[3]) if len(sys.argv) > 3 else 5
prec = sys.argv[4] if len(sys.argv) > 4 else "bf16x3"
reps = int(sys.argv[5]) if len(sys.argv) > 5 else 50
assert torch.cuda.is_available(), "needs an MI355X"
sk = h36m_skeleton()
torch.manual_seed(0)
model = RMCLManifoldMixSTE(sk, num_frame=T, n_hyp=K, drop_path_rate=0.1)
model.precision = prec
model.max_batch_hint = 2 * W
model = model.cuda().eval()
g = torch.Generator(device="cuda").manual_seed(1)
poses = 0.3 * torch.randn(2 * W, K, T, 17, 3, device="cuda", generator=g)
scores = torch.softmax(torch.randn(2 * W, K, T, 1, device="cuda", generator=g), dim=1).contiguous()
N = W * T
win_seq, win_start = plan_windows([N], T, T)
off = np.array([0, N], dtype=np.int64)
tables = tuple(torch.from_numpy(a).cuda() for a in (win_seq, win_start, off))
mirror = _mirror(model, 17)
out = torch.empty(N, 17, 3, device="cuda")


def composition(best):
    pred = model.aggregate(poses[:W], scores[:W], "weighted_ave")
    hyp_f = pose_flip((poses[W:].clone(),), sk)[0]
    pred = (pred + model.aggregate(hyp_f, scores[W:], "weighted_ave")) / 2
    if best:
        b = (model.aggregate(poses[:W], scores[:W], "best_score") + model.aggregate(hyp_f, scores[W:], "best_score")) / 2
        return pred, b
    return pred


def merge(agg="weighted_ave"):
    return merge_windows(poses, scores, win_seq, win_start, off, T=T, tta=True, mirror=mirror, agg=agg, out=out, device_tables=tables)[0]


def timed(fn):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(reps):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / reps


a = composition(False).reshape(N, 17, 3)
b = merge().clone()
print(f"W={W} T={T} K={K} TTA on, stride=T, {N} frames; max |composition - merge| = {(a - b).abs().max().item():.2e}", flush=True)
must = 2 * W * K * T * (51 + 1) * 4 + N * 51 * 4           # every hypothesis and score read once, every output float written once
rows = (("(a) composition, weighted_ave", lambda: composition(False)), ("(a) composition, weighted_ave + best_score (evaluate)", lambda: composition(True)),
        ("(b) mp_lift_merge, weighted_ave", merge), ("(b) mp_lift_merge x2, weighted_ave + best_score", lambda: (merge(), merge("best_score"))))
for name, fn in rows:
    ms = timed(fn)
    extra = f", {must / ms / 1e6:,.0f} GB/s of the {must / 1e6:.1f} MB it must move" if name.startswith("(b) mp_lift_merge,") else ""
    print(f"{name}: {ms * 1e3:,.1f} us  {N / ms / 1e3:,.2f} M frames/s{extra}", flush=True)
# end to end: one sequence of W windows, lifted at the bench's batch
p2 = (0.3 * torch.randn(N, 17, 2, device="cuda", generator=g)).clamp(-1, 1)
lift_sequences(model, [p2], batch=W)
torch.cuda.synchronize()
ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
n_e2e = 3
ev[0].record()
for _ in range(n_e2e):
    lift_sequences(model, [p2], batch=W)
ev[1].record()
torch.cuda.synchronize()
ms = ev[0].elapsed_time(ev[1]) / n_e2e
print(f"lift_sequences end to end ({prec}, batch {W}, TTA on): {ms:,.1f} ms per {N} frames = {N / ms * 1e3:,.0f} frames/s", flush=True)

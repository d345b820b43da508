"""Refining placed root trajectories under the full camera model, the host side (no GPU): the float64 statement of the rule (lift_refine_ref.py)
against central differences, against its own optimality condition and against an independent damped minimiser; what the feature is for (the
linear fit's depth bias on noise-free keypoints of the full model, and its removal); the decision margins of every scene the GPU tests use; the
new entry point in the places that declare it, the config key, and the argument errors that are raised before anything touches a device."""
import os
import re
import shlex
import sys

import numpy as np
import pytest
import torch

import lift_place_ref as place
import lift_refine_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hpe"))


def test_zero_steps_are_the_linear_fit():
    intr = ref.s11_intrinsics()
    poses, kp, _, off = ref.distorted_scene([1, 7, 5], 3, 4, intr, seed=0, noise=0.01)
    for distort in (True, False):
        for weights in (None, np.where(np.arange(17) % 3 == 0, 0.0, 1.0)):
            want = place.place_all(poses, kp, intr, off, weights, distort)
            got = ref.refine_all(poses, kp, intr, off, weights, distort, iters=0)
            assert all(np.array_equal(a, b) for a, b in zip(got[:3], want)) and not got[3].any() and want[2].all()
    pose, k = poses[3, 0], kp[3]
    for bad in (ref.refine_one(pose, k, intr[1], np.zeros(17), iters=4), ref.refine_one(pose, np.broadcast_to(k[3], (17, 2)), intr[1], iters=4)):
        assert np.array_equal(bad[0], np.zeros(3)) and bad[1:] == (0.0, 0, 0)                     # a degenerate fit: all zeros, no step
    behind = pose.copy()
    behind[5, 2] = -40.0
    t, err, ok, steps = ref.refine_one(behind, k, intr[1], iters=4)
    want = place.place_one(behind, k, intr[1])
    assert ok == 0 and steps == 0 and np.array_equal(t, want[0]) and err == want[1] and want[2] == 0       # stored as computed, no step


def test_the_jacobian_matches_central_differences():
    intr = ref.s11_intrinsics()[0].astype(np.float64)
    g = np.random.default_rng(3)
    points = np.concatenate([g.uniform(-1, 1, (40, 2)) * 3.0, g.uniform(3, 7, (40, 1))], axis=1)
    points = np.concatenate([points, [[6.0, 0.5, 4.0], [0.5, -7.0, 4.0], [9.0, 9.0, 5.0]]])      # x clamped, y clamped, both
    assert (np.abs(points[-3:, :2] / points[-3:, 2:3]) > 1).sum() == 4
    worst, h = 0.0, 1e-5
    for distort in (True, False):
        for P in points:
            J = ref.jacobian(P, intr, distort)
            num = np.stack([(place.project(P + h * e, intr, distort) - place.project(P - h * e, intr, distort)) / (2 * h) for e in np.eye(3)], axis=1)
            worst = max(worst, np.abs(J - num).max() / max(1.0, np.abs(num).max()))
    print(f"\n[jacobian vs central differences] worst relative difference {worst:.2e} (bound 1e-7)")
    assert worst <= 1e-7
    J = ref.jacobian(points[-3], intr)                                                            # x clamped: no derivative through x
    assert J[0, 0] == 0 and J[1, 0] == 0 and np.abs(J[:, 1]).max() > 0 and np.array_equal(ref.jacobian(points[-1], intr), np.zeros((2, 3)))


def _cost(pose, kp, intr, t):
    return float((((place.project(pose[:, :3].astype(np.float64) + t, intr, True) - kp) ** 2).sum()))


def _damped_minimiser(pose, kp, intr, t0):
    """Levenberg-Marquardt with a numerical Jacobian of lift_place_ref.project: independent of the statement's Jacobian, steps and acceptance rule"""
    t, lam, f = np.array(t0, np.float64), 1e-3, _cost(pose, kp, intr, t0)
    for _ in range(200):
        r = (place.project(pose[:, :3].astype(np.float64) + t, intr, True) - kp).ravel()
        h = 1e-6
        Jn = np.stack([((place.project(pose[:, :3].astype(np.float64) + t + h * e, intr, True)
                         - place.project(pose[:, :3].astype(np.float64) + t - h * e, intr, True)) / (2 * h)).ravel() for e in np.eye(3)], axis=1)
        A, b = Jn.T @ Jn, Jn.T @ r
        d = np.linalg.solve(A + lam * np.diag(np.diag(A)), -b)
        f2 = _cost(pose, kp, intr, t + d)
        if f2 <= f:
            t, f, lam = t + d, f2, max(lam / 10, 1e-15)
        else:
            lam *= 10
        if np.abs(d).max() < 1e-13:
            break
    return t


def test_the_converged_translation_is_a_minimum():
    intr = ref.s11_intrinsics()
    poses, kp, _, off = ref.distorted_scene([6, 6], 1, 3, intr[:2], seed=21, noise=0.01)
    worst_g = worst_t = 0.0
    for n in range(12):
        cam = intr[n // 6].astype(np.float64)
        t, err, ok, steps = ref.refine_one(poses[n, 0], kp[n], cam, iters=8)
        assert ok == 1 and steps == 8
        e = ref.evaluate(poses[n, 0], kp[n], cam, np.ones(17), True, t)
        gnorm, hnorm = np.abs(e["g"]).max(), np.abs(np.array(e["H"])).max()
        worst_g = max(worst_g, gnorm / (hnorm * np.abs(t).max()))
        assert gnorm <= 1e-9 * hnorm * np.abs(t).max()                                            # the optimality condition |g| <= 1e-9 |H| |t|
        other = _damped_minimiser(poses[n, 0], kp[n].astype(np.float64), cam, place.place_one(poses[n, 0], kp[n], cam)[0])
        worst_t = max(worst_t, np.abs(t - other).max())
    print(f"\n[converged] worst |g| / (|H| |t|) = {worst_g:.2e} (bound 1e-9), worst |t - damped minimiser| = {worst_t:.2e} m (bound 1e-9)")
    assert worst_t <= 1e-9


def test_the_linear_fit_is_biased_under_the_full_camera_and_three_steps_remove_it():
    """What the feature is for.  Checked when written: the linear fit misses by 0.171 m, three steps by 2.1e-7 m (the float32 rounding of the keypoints)."""
    poses, kp, t_true, off = ref.recovery_scene()
    intr = ref.s11_intrinsics()
    lin = place.place_all(poses[:, 0], kp, intr, off)
    miss_lin = np.abs(lin[0] - t_true).max()
    trace = []
    got = ref.refine_all(poses[:, 0], kp, intr, off, iters=3, trace=trace)
    miss = np.abs(got[0] - t_true).max()
    sizes = [max(d["step"] for d in trace if d["kind"] == "cost")]
    print(f"\n[recovery] linear fit misses by {miss_lin:.3f} m (mean reprojection error {lin[1].mean():.2e}); 3 steps: {miss:.2e} m, reprojection error "
          f"{got[1].max():.2e}; largest step {sizes[0]:.2e} m")
    assert lin[2].all() and miss_lin >= 0.1
    assert got[2].all() and (got[3] == 3).all() and miss <= 2e-6 and got[1].max() <= 1e-6


def _margins(tag, trace, worst):
    cost, det = ref.margins(trace)
    print(f"[margins] {tag}: cost decisions at least {cost:.2e} relative from their threshold, det / (H00 H11 H22) at least {det:.2e}")
    assert cost >= 1e-9 and det >= 1e-6, tag
    worst[0], worst[1] = min(worst[0], cost), min(worst[1], det)


def test_margins_of_the_gpu_inputs():
    """Every accept / reject decision the statement takes on the scenes of test_gpu_lift_refine.py lies far enough from its threshold that fp64
    contraction differences between the kernel and numpy cannot flip it.  The decisions of a run of 16 steps contain those of 1 and of 4."""
    intr = ref.s11_intrinsics()
    worst = [np.inf, np.inf]
    print()
    for inner, ch in ((1, 3), (1, 4), (5, 3), (5, 4)):
        poses, kp, _, off = ref.fp64_scene(inner, ch)
        for distort in (True, False):
            trace = []
            ref.refine_all(poses, kp, intr, off, None, distort, iters=16, trace=trace)
            _margins(f"fp64 scene inner={inner} C={ch} distort={int(distort)}", trace, worst)
    poses, kp, _, off = ref.recovery_scene()
    trace = []
    ref.refine_all(poses, kp, intr, off, iters=3, trace=trace)
    _margins("recovery scene", trace, worst)
    poses, kp, _, off = ref.small_scene()
    keep = np.arange(17) % 3 != 0
    trace = []
    four = ref.refine_all(poses, kp, intr, off, np.where(keep, 1.0, 0.0), iters=4, trace=trace)
    ref.refine_all(poses, kp, intr, off, np.random.default_rng(9).uniform(0.25, 4.0, 17).astype(np.float32), iters=4, trace=trace)
    four = ref.refine_all(poses, kp, intr, off, iters=4, trace=trace)
    ref.refine_all(poses, kp, intr, off, iters=2, start=four[0].astype(np.float32), trace=trace)
    _margins("small scene: weights, 4 steps, warm start", trace, worst)
    lin = place.place_all(poses, kp, intr, off)
    trace = []
    got = ref.refine_all(poses, kp, intr, off, iters=6, start=ref.overshoot_start(lin[0]), trace=trace)
    _margins("small scene: overshooting start", trace, worst)
    rising = [d for d in trace if d["kind"] == "cost" and not d["taken"] and d["deep"]]
    print(f"[margins] overshooting start: {len(rising)} steps refused for a rising cost alone, F' / F from {min(d['value'] / d['threshold'] for d in rising):.2f}")
    assert rising and (got[3] == 0).any() and (got[3] == 6).any()
    clean_p, clean_k, bad_p, bad_k, intr1 = ref.guards_scene()
    trace = []
    ref.refine_all(clean_p, clean_k, intr1, iters=4, trace=trace)
    _margins("guards scene, clean", trace, worst)
    trace = []
    ref.refine_all(np.delete(bad_p, ref.CLAMPED, axis=0), np.delete(bad_k, ref.CLAMPED, axis=0), intr1, iters=4, trace=trace)
    _margins("guards scene, spoiled, without the clamped frame", trace, worst)
    for i in range(2):                                                    # the clamped frame is built to make H = 0: checked for exactly that
        trace = []
        t, err, ok, steps = ref.refine_one(bad_p[ref.CLAMPED, i], bad_k[ref.CLAMPED], intr1[0], iters=4, trace=trace)
        q = (bad_p[ref.CLAMPED, i, :, :2] + t[:2]) / (bad_p[ref.CLAMPED, i, :, 2:3] + t[2])
        assert (q > 1).all() and ok == 1 and steps == 0 and np.isfinite(err)
        assert [d["kind"] for d in trace] == ["eval", "det"] and not np.array(trace[0]["H"]).any() and not np.array(trace[0]["g"]).any()
        assert trace[1]["value"] == 0 and trace[1]["scale"] == 0
    print(f"[margins] over all scenes: cost {worst[0]:.2e} (needed 1e-9), det ratio {worst[1]:.2e} (needed 1e-6)")


def test_new_abi_symbol_is_declared_everywhere():
    from manipose_amd import _lib, lifting
    import manipose_amd
    header = open(_lib.HEADER_PATH).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "mp_lift_place_refine" in _lib.declared_symbols() and len(_lib._SIGNATURES["mp_lift_place_refine"][1]) == 19
    assert "lib.mp_lift_place_refine.argtypes" in doc
    assert _lib.ABI_VERSION == 8 and int(re.search(r"#define MP_ABI_VERSION (\d+)", header).group(1)) == 8        # purely additive
    assert int(re.search(r"#define MP_LIFT_REFINE_MAXITERS (\d+)", header).group(1)) == lifting.REFINE_MAXITERS == ref.MAXITERS
    assert manipose_amd.reproject_poses is lifting.reproject_poses and "reproject_poses" in lifting.__all__
    assert os.path.exists(os.path.join(ROOT, "manipose_amd", "csrc", "lift_place.hip"))
    if os.path.exists(_lib.LIB_PATH):
        assert hasattr(_lib.load(), "mp_lift_place_refine")


def test_config_key_parses_a_typo_fails_and_the_readme_command_parses():
    from _entry import LIFT_SUFFIXES, lift_place_options, lift_refine_options, load_config, run
    cfg = load_config([])
    assert cfg.lift.place_refine == 0 and lift_refine_options(cfg) == 0
    cfg = load_config(["lift.place=true", "lift.place_refine=3"])
    assert lift_refine_options(cfg) == 3
    with pytest.raises(SystemExit):
        load_config(["lift.place_refien=3"])
    for argv, word in ((["lift.place_refine=3"], "set lift.place=true"), (["lift.place=true", "lift.place_refine=17"], "0..16"),
                       (["lift.place=true", "lift.place_refine=-1"], "0..16"), (["lift.place=true", "lift.place_refine=2.5"], "0..16"),
                       (["lift.place=true", "lift.place_refine=true"], "0..16"), (["+data=mpi_inf_3dhp", "lift.place=true", "lift.place_refine=3"], "carry none")):
        with pytest.raises(ValueError, match=word):
            run(["run.train=false", "run.test=false", "run.lift=true"] + argv)        # (a run that got further would need a device)
    assert all(s in LIFT_SUFFIXES for s in ("__steps", "__hyps_steps", "__reproj_smooth", "__hyps_reproj_smooth"))
    lines = [l for l in open(os.path.join(ROOT, "README.md")).read().splitlines() if l.startswith("python hpe/") and "lift.place_refine=" in l]
    assert len(lines) == 1
    cfg = load_config(shlex.split(lines[0].split("#")[0])[2:])
    assert cfg.run.lift is True and lift_place_options(cfg)[0] is True and lift_refine_options(cfg) == 3


def test_argument_errors_are_value_errors_before_any_device_work():
    """The calls are given CPU tensors and a CPU model: had the arguments been accepted, they would have ended in the RuntimeError that refuses them
    ("no CPU fallback"), which is what the valid calls at the end do."""
    from manipose_amd import RMCLManifoldMixSTE, h36m_skeleton, lift_sequences, place_poses, reproject_poses
    from manipose_amd.data.ingest import h36m_cameras
    model = RMCLManifoldMixSTE(h36m_skeleton(), num_frame=9, embed_dim_rot=32, depth_rot=1, num_heads_rot=4, embed_dim_seg=16, depth_seg=1, num_heads_seg=4,
                               n_hyp=2)
    seqs = [np.zeros((12, 17, 2), np.float32), np.zeros((20, 17, 2), np.float32)]
    cams = h36m_cameras()["S11"][:2]
    for kw, word in ((dict(place_refine=3), "place_refine refines"), (dict(place_refine=3, frame="world", cameras=cams), "place_refine refines"),
                     (dict(place_refine=17, place=True, cameras=cams), "0..16"), (dict(place_refine=-1, place=True, cameras=cams), "0..16"),
                     (dict(place_refine=True, place=True, cameras=cams), "0..16"), (dict(place_refine=2.0, place=True, cameras=cams), "0..16")):
        with pytest.raises(ValueError, match=word):
            lift_sequences(model, seqs, **kw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        lift_sequences(model, seqs, place=True, place_refine=3, cameras=cams, smooth_traj=4, return_place=True)
    intr = cams[0]["intrinsic"]
    poses, kp, traj = torch.zeros(4, 17, 3), torch.zeros(4, 17, 2), torch.zeros(4, 3)
    for n in (17, -1, 1.5, True):
        with pytest.raises(ValueError, match="0..16"):
            place_poses(poses, kp, intr, refine=n)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        place_poses(poses, kp, intr, refine=3, return_steps=True)
    for bad_traj, bad_ok, word in ((torch.zeros(4, 2), None, "traj must be"), (torch.zeros(4, 3, dtype=torch.float64), None, "traj must be"),
                                   (traj, torch.zeros(4), "ok must be"), (traj, torch.zeros(3, dtype=torch.uint8), "ok must be")):
        with pytest.raises(ValueError, match=word):
            reproject_poses(poses, bad_traj, kp, intr, bad_ok)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        reproject_poses(poses, traj, kp, intr, torch.ones(4, dtype=torch.uint8))

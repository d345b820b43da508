"""Calibrating a take on its keypoints, the parts that need no device: the float64 statement of mp_lift_calibrate_views' rule
(lift_calibrate_ref.py) against a dense solve of the full normal equations, its Jacobians - the focal column included - against central
differences, the conditions under which the device test (test_gpu_lift_calibrate.py) claims its bounds (every decision's margin, the reduced
system's condition number), the recovery claim on the committed scene, the takes that are evaluated only, the argument checks and the
declarations."""
import os
import re

import numpy as np
import pytest
import torch

import lift_bundle_ref as bundle
import lift_calibrate_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _take(sc, g=0, focal=True, fixed=None, **kw):
    """(Take, q, T, gf, X, free, fslot, colv) of take g of a scene at its start"""
    inp = ref.inputs(sc, **kw)
    sl = slice(int(sc["off"][g]), int(sc["off"][g + 1]))
    tk = ref.make_take(inp["start"], inp["kp"], inp["quat"][g], inp.get("valid"), inp.get("start_ok"), inp.get("weights"), inp["intr"][g],
                       inp.get("distort", True), inp.get("sigma", ref.SIGMA), inp.get("prior", ref.PRIOR), sl)
    q = [ref.unit(inp["quat"][g, v]) for v in range(tk.V)]
    T = [inp["trans"][g, v].astype(np.float64) for v in range(tk.V)]
    free, fslot, colv, iterates = ref.columns(tk.used.sum(axis=1), fixed, focal)
    assert iterates
    return tk, q, T, [1.0] * tk.V, tk.start.copy(), free, fslot, colv


@pytest.mark.parametrize("V,focal,weights", [(4, True, None), (3, True, ref.WEIGHTS[:7]), (2, False, None)])
def test_the_schur_step_is_the_dense_gauss_newton_step(V, focal, weights):
    """eliminating the points one by one and solving the reduced system gives the step of the full system: cameras, focal factors and points"""
    sc = ref.scene(V, 7, [6], seed=500 + V)
    valid = np.ones((V, 6), np.uint8)
    valid[V - 1, 2] = 0                                                   # a frame one view does not observe
    tk, q, T, gf, X, free, fslot, colv = _take(sc, focal=focal, valid=valid, weights=weights)
    dc, dX = ref.schur_step(tk, q, T, gf, X, free, fslot, colv)
    dc2, dX2 = ref.dense_step(tk, q, T, gf, X, free, fslot)
    assert len(dc) == 6 * (V - 1) + (V if focal else 0)
    assert np.abs(dc - dc2).max() <= 1e-7 * np.abs(dc2).max() and np.abs(dX - dX2).max() <= 1e-7 * np.abs(dX2).max()
    if weights is not None:
        assert (dX[:, np.asarray(weights) == 0] == 0).all()              # a joint of weight 0 stays at start


@pytest.mark.parametrize("distort", [True, False])
def test_the_jacobians_against_central_differences(distort):
    """every column of the dense Jacobian - camera, FOCAL and point - is the central difference of the residuals under the rule's own update:
    the camera moved by move_camera (the left perturbation), the focal factor added to, the point added to"""
    sc = ref.scene(3, 4, [2], seed=510)
    tk, q, T, gf, X, free, fslot, colv = _take(sc, sigma=float("inf"), distort=distort)
    gf = [1.05, 0.97, 1.02]                                               # (away from 1: the division by g counts)
    r0, Jm, (N, frames, joints, seen) = ref.jacobian(tk, q, T, gf, X, free, fslot)
    assert N == 15 and np.abs(r0[seen] - ref.residuals(tk, q, T, gf, X)).max() == 0
    J = Jm[seen]
    h = 1e-6
    worst = 0.0
    for c in range(Jm.shape[1]):
        side = []
        for s in (h, -h):
            qn, Tn, gn, Xn = list(q), list(T), list(gf), X.copy()
            if c < 6 * len(free):
                d = np.zeros(6)
                d[c % 6] = s
                qn[free[c // 6]], Tn[free[c // 6]] = bundle.move_camera(q[free[c // 6]], T[free[c // 6]], d)
            elif c < N:
                gn[fslot.index(c)] += s
            else:
                a, rest = divmod(c - N, 3 * len(joints))
                Xn[frames[a], joints[rest // 3], rest % 3] += s
            side.append(ref.residuals(tk, qn, Tn, gn, Xn))
        fd = (side[0] - side[1]) / (2 * h)
        worst = max(worst, np.abs(fd - J[:, c]).max() / max(1.0, np.abs(J[:, c]).max()))
    assert worst <= 1e-7, worst                                           # (h^2 times the third derivative, and rounding / h)


def test_every_compared_scene_is_decided_and_conditioned():
    """the device is held to the statement within a float32 store only where every decision is at least MARGIN_MIN from its threshold and the
    reduced system's condition number, which amplifies what the library's sine and cosine differ by, is at most 1e8 (1e8 x 1e-16 against 2^-24)"""
    worst = 0.0
    for tag, inp, want, trace in ref.cases():
        assert ref.margin(trace) >= ref.MARGIN_MIN, (tag, ref.margin(trace))
        assert ref.worst_cond(trace) <= ref.COND_MAX, (tag, ref.worst_cond(trace))
        worst = max(worst, ref.worst_cond(trace))
    for V in (4, 2):
        trace = []
        ref.calibrate(trace=trace, **ref.inputs(ref.recovery(V)))
        assert ref.margin(trace) >= ref.MARGIN_MIN and ref.worst_cond(trace) <= ref.COND_MAX
        worst = max(worst, ref.worst_cond(trace))
    print("worst condition number", worst)
    tags = " ".join(t for t, *_ in ref.cases())
    assert all(f"F={n} " in tags for n in (1, 5, 65, 257)) and "V=3 J=5" in tags and "V=2 J=17" in tags and "V=4 J=17" in tags


def test_recovery_on_the_committed_scene():
    """S11's four cameras, 200 frames, 17 joints in smooth motion, seed 11 (lift_calibrate_ref.RECOVERY): keypoint noise 0.002, the start's focal
    lengths 10, 10, 7 and 8 % off, the free cameras 0.02 rad and 5 cm off per component, the points 62 mm off on average; prior 1e-3, sigma 0.05,
    three steps.  Measured with the float64 statement (no device, synthetic data - nothing here is measured on real data):
      four views: focal errors 0.100, 0.100, 0.070, 0.080 -> 0.0127, 0.0017, 0.0070, 0.0064; mean point error 61.9 -> 12.6 mm; cost 17.52 -> 0.0837;
                  condition number 4.8e6, 1.6e6, 1.6e6
      two views:  focal errors 0.100, 0.100 -> 0.0039, 0.0089; mean point error 68.7 -> 14.7 mm; cost 6.42 -> 0.0318; condition number 1.7e6
    The claim: every view's focal error ends below a quarter of its start, and the mean point error falls."""
    for V in (4, 2):
        sc = ref.recovery(V)
        out = ref.calibrate(**ref.inputs(sc))
        e0, e1 = ref.focal_errors(sc["intr"], sc), ref.focal_errors(out["intr"], sc)
        p0, p1 = ref.point_error(sc["start"], sc), ref.point_error(out["points"], sc)
        print(V, "views: focal", e0, "->", e1, "points", p0, "->", p1, "cost", out["cost"])
        assert out["steps"][0] == 3 and out["ok"][0] == 1
        assert (e1 < 0.25 * e0).all() and p1 < p0 and out["cost"][0, 1] < out["cost"][0, 0]
        assert np.array_equal(out["intr"][0][:, 2:], sc["intr"][0][:, 2:].astype(np.float64))        # the centre and the distortion stay
        assert np.array_equal(out["quat"][0, 0], sc["quat"][0, 0]) and np.array_equal(out["trans"][0, 0], sc["trans"][0, 0])     # the first view is held
        assert np.allclose(out["intr"][0][:, 1] / sc["intr"][0][:, 1], out["intr"][0][:, 0] / sc["intr"][0][:, 0], rtol=1e-15)    # one factor per view


def test_a_single_view_and_a_take_without_parameters_are_evaluated_only():
    sc = ref.scene(4, 17, [9], seed=520)
    inp = ref.inputs(sc)
    one = np.zeros((4, 9), np.uint8)
    one[2] = 1
    copied = lambda o: all(np.array_equal(o[k], np.asarray(inp[s]).astype(np.float64).reshape(o[k].shape))
                           for k, s in (("quat", "quat"), ("trans", "trans"), ("intr", "intr"), ("points", "start")))
    for kw in (dict(valid=one), dict(valid=one, fixed=np.zeros((1, 4), np.uint8)),             # one view: its poses do not decide its focal length
               dict(focal=False, fixed=np.ones((1, 4), np.uint8)),                             # no parameter: the prior alone
               dict(focal=False, fixed=np.zeros((1, 4), np.uint8))):                           # no fixed view, focal held: no camera moves
        out = ref.calibrate(**dict(inp, **kw))
        assert out["steps"][0] == 0 and out["ok"][0] == 1 and copied(out), kw
        assert out["cost"][0, 0] == out["cost"][0, 1] > 0 and np.array_equal(out["reproj"][0][:, 0], out["reproj"][0][:, 1])
    held = ref.calibrate(**dict(inp, fixed=np.ones((1, 4), np.uint8)))                         # every view fixed, the focal factors free: it iterates
    assert held["steps"][0] == 3 and np.array_equal(held["quat"], np.asarray(inp["quat"], np.float64)) and not np.array_equal(held["intr"][0][:, 0], inp["intr"][0][:, 0])
    nothing = ref.calibrate(**dict(inp, iters=0))
    assert nothing["steps"][0] == 0 and copied(nothing)


def test_the_argument_checks_come_before_the_device():
    from manipose_amd import calibrate_views
    pts, kp = torch.zeros(6, 5, 3), torch.zeros(3, 6, 5, 2)
    cams = [[np.concatenate([[1.1, 1.1, 0, 0, 0, 0, 0, 0, 0], [1, 0, 0, 0], [0, 0, 0]]) for _ in range(3)]]
    for bad in (0, 0.0, -1e-3, float("nan"), float("inf"), None, True, "1"):
        with pytest.raises(ValueError, match="prior must be a finite number > 0"):
            calibrate_views(pts, kp, cams, prior=bad)
    for bad in (0, -1.0, float("nan"), None):
        with pytest.raises(ValueError, match="sigma must be a number > 0"):
            calibrate_views(pts, kp, cams, sigma=bad)
    for bad in (-1, 9, 2.0, True):
        with pytest.raises(ValueError, match=r"iters counts Gauss-Newton steps, an integer in 0\.\.8"):
            calibrate_views(pts, kp, cams, iters=bad)
    with pytest.raises(ValueError, match="pose must be contiguous float32"):
        calibrate_views(torch.zeros(6, 5, 2), kp, cams)
    with pytest.raises(ValueError, match="points_ok must be a uint8 tensor"):
        calibrate_views(pts, kp, cams, points_ok=np.ones(6, np.uint8))
    with pytest.raises(ValueError, match="fixed must be a table"):
        calibrate_views(pts, kp, cams, fixed=np.ones((2, 3), np.uint8))
    with pytest.raises(RuntimeError, match="calibrate_views takes device tensors; there is no CPU fallback"):
        calibrate_views(pts, kp, cams)


def test_new_abi_symbol_is_declared_everywhere():
    from manipose_amd import _lib, lifting
    import manipose_amd
    header = open(_lib.HEADER_PATH).read()
    assert {"mp_lift_calibrate_views", "mp_lift_calibrate_views_scratch_bytes"} <= set(_lib.declared_symbols())
    assert len(_lib._SIGNATURES["mp_lift_calibrate_views"][1]) == 31 and len(_lib._SIGNATURES["mp_lift_calibrate_views_scratch_bytes"][1]) == 3
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "lib.mp_lift_calibrate_views.argtypes" in integration and "lib.mp_lift_calibrate_views_scratch_bytes.argtypes" in integration
    assert _lib.ABI_VERSION == 8 and int(re.search(r"#define MP_ABI_VERSION (\d+)", header).group(1)) == 8        # purely additive
    assert int(re.search(r"#define MP_LIFT_CALIBRATE_MAXITERS (\d+)", header).group(1)) == lifting.CALIBRATE_MAXITERS == ref.MAXITERS == 8
    assert manipose_amd.calibrate_views is lifting.calibrate_views and "calibrate_views" in lifting.__all__
    assert (lifting.CALIBRATE_SIGMA, lifting.CALIBRATE_PRIOR, lifting.CALIBRATE_ITERS) == (ref.SIGMA, ref.PRIOR, 3)
    assert lifting.ViewCalibration._fields == ("cameras", "quat", "trans", "intr", "points", "reproj", "cost", "steps", "ok", "used")
    assert os.path.exists(os.path.join(ROOT, "manipose_amd", "csrc", "lift_calibrate.hip"))
    for name in ("README.md", "DESIGN.md"):
        assert "mp_lift_calibrate_views" in open(os.path.join(ROOT, name)).read()
    if os.path.exists(_lib.LIB_PATH):
        lib = _lib.load()
        assert lib.mp_lift_calibrate_views_scratch_bytes(4, 10, 17) == 10 * 8 * (286 + 1 + 75 * 17 + 96)
        assert lib.mp_lift_calibrate_views_scratch_bytes(5, 10, 17) == 0 and lib.mp_lift_calibrate_views_scratch_bytes(4, 0, 17) == 0 and \
            lib.mp_lift_calibrate_views_scratch_bytes(4, 10, 1) == 0 and lib.mp_lift_calibrate_views_scratch_bytes(4, 10, 33) == 0


def test_config_keys_parse_and_the_option_errors_come_before_the_model():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "hpe"))
    from _entry import CALIBRATE_KEYS, LIFT_SUFFIXES, lift_fuse_calibrate_options, load_config, run, start_focal_cameras
    cfg = load_config([])
    assert cfg.lift.fuse_calibrate == 0 and lift_fuse_calibrate_options(cfg) == (0, 0.05, 0.001, True, 0.0)
    on = ["run.lift=true", "lift.hyps=true", "lift.fuse=true", "lift.fuse_cameras=estimate"]
    assert lift_fuse_calibrate_options(load_config(on)) == (0, 0.05, 0.001, True, 0.0)
    assert lift_fuse_calibrate_options(load_config(on + ["lift.fuse_calibrate=3"])) == (3, 0.05, 0.001, True, 0.0)
    assert lift_fuse_calibrate_options(load_config(on + ["lift.fuse_calibrate=8", "lift.fuse_calibrate_sigma=0.2", "lift.fuse_calibrate_prior=0.01",
                                                         "lift.fuse_calibrate_focal=false", "lift.fuse_calibrate_start_focal=2.2"])) == (8, 0.2, 0.01, False, 2.2)
    assert lift_fuse_calibrate_options(load_config(on + ["lift.fuse_calibrate_start_focal=2.2"])) == (0, 0.05, 0.001, True, 2.2)
    assert all(k in LIFT_SUFFIXES for k in CALIBRATE_KEYS) and "__cam_quat_bundle" in LIFT_SUFFIXES
    for argv, message in (
            (on + ["lift.fuse_calibrate=9"], "lift.fuse_calibrate counts Gauss-Newton steps, an integer in 0..8 (0: off), got 9"),
            (on + ["lift.fuse_calibrate=-1"], "lift.fuse_calibrate counts Gauss-Newton steps, an integer in 0..8 (0: off), got -1"),
            (on + ["lift.fuse_calibrate=true"], "lift.fuse_calibrate counts Gauss-Newton steps, an integer in 0..8 (0: off), got True"),
            (on + ["lift.fuse_calibrate=3", "lift.fuse_calibrate_sigma=0"], "lift.fuse_calibrate_sigma must be > 0"),
            (on + ["lift.fuse_calibrate=3", "lift.fuse_calibrate_prior=0"], "lift.fuse_calibrate_prior must be a finite number > 0"),
            (on + ["lift.fuse_calibrate=3", "lift.fuse_calibrate_prior=-0.001"], "lift.fuse_calibrate_prior must be a finite number > 0"),
            (on + ["lift.fuse_calibrate=3", "lift.fuse_calibrate_prior=.inf"], "lift.fuse_calibrate_prior must be a finite number > 0"),
            (on + ["lift.fuse_calibrate=3", "lift.fuse_calibrate_focal=1"], "lift.fuse_calibrate_focal must be true or false, got 1"),
            (on + ["lift.fuse_calibrate_start_focal=-1"], "lift.fuse_calibrate_start_focal is a focal length in normalised screen units"),
            (on + ["lift.fuse_calibrate_prior=0.01"], "describe the calibration of a take on its keypoints: set lift.fuse_calibrate=N"),
            (on + ["lift.fuse_calibrate_focal=false"], "describe the calibration of a take on its keypoints: set lift.fuse_calibrate=N"),
            (on[:3] + ["lift.fuse_calibrate=3"], "lift.fuse_calibrate refines the cameras that lift.fuse_cameras=estimate estimates"),
            (on[:3] + ["lift.fuse_calibrate_start_focal=2.2"], "lift.fuse_calibrate_start_focal replaces the intrinsics of a run that estimates its cameras")):
        with pytest.raises(ValueError) as err:
            lift_fuse_calibrate_options(load_config(argv))
        assert message in str(err.value), (argv, str(err.value))
        with pytest.raises(ValueError) as err:                            # run() raises it before anything is built (no device is asked for)
            run(argv)
        assert message in str(err.value)
    from manipose_amd.data.ingest import h36m_cameras
    s11 = h36m_cameras()["S11"][:2]
    rows = start_focal_cameras([s11[0], np.concatenate([s11[1]["intrinsic"], s11[1]["orientation"], s11[1]["translation"], [1]])], 2.2)
    assert rows[0].shape == (16,) and rows[1].shape == (17,) and rows[1][16] == 1 and all(r.dtype == np.float32 for r in rows)
    assert all(r[:9].tolist() == [np.float32(2.2)] * 2 + [0] * 7 for r in rows)
    assert np.array_equal(rows[0][9:13], np.asarray(s11[0]["orientation"], np.float32)) and np.array_equal(rows[1][13:16], np.asarray(s11[1]["translation"], np.float32))

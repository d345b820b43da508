"""Aligning a take's views without extrinsics, the parts that need no device: the float64 statement of mp_lift_align_views' rule
(lift_align_ref.py) against plain Horn, its degenerate rules, the canonical sign, align_views' composition with a reference camera, the
recovery claim on a committed seed, the conditioning of the device test's scenes, the option checks of hpe/_entry.py and the declarations."""
import os
import re
import sys

import numpy as np
import pytest
import torch

import lift_align_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hpe"))


def _kabsch(bv, br):
    """the rotation taking bv onto br best, by the singular value decomposition: an independent route to Horn's answer"""
    U, _, Vt = np.linalg.svd(np.einsum("fja,fjc->ac", bv, br))
    d = np.sign(np.linalg.det(Vt.T @ U.T))
    return Vt.T @ np.diag([1.0, 1.0, d]) @ U.T


def test_iters_0_is_plain_horn_and_sigma_inf_is_iters_0_exactly():
    sc = ref.scene(4, 17, [40, 25], seed=3, mirrored=0.3)
    plain = ref.align(sc["poses"], None, sc["off"], sc["traj"], sc["traj_ok"], iters=0)
    x = sc["poses"].astype(np.float64)
    for g in range(2):
        sl = slice(int(sc["off"][g]), int(sc["off"][g + 1]))
        for v in range(1, 4):
            R = _kabsch(x[v, sl] - x[v, sl, :1], x[0, sl] - x[0, sl, :1])
            assert np.abs(ref.quat_matrix(plain["quat"][g, v]) - R).max() < 1e-12
            d = x[0, sl, 0] - x[v, sl, 0] @ R.T                                # joint 0 is the trajectory, up to its float32 rounding
            assert np.abs(plain["trans"][g, v] - d.mean(0)).max() < 1e-6
    blind = ref.align(sc["poses"], None, sc["off"], sc["traj"], sc["traj_ok"], sigma=float("inf"), iters=5)
    assert all(np.array_equal(blind[k], plain[k]) for k in plain)
    robust = ref.align(sc["poses"], None, sc["off"], sc["traj"], sc["traj_ok"])
    assert not np.array_equal(robust["quat"], plain["quat"])
    assert (plain["ok"] == [[1, 3, 3, 3]] * 2).all() and (plain["used"] == [[40] * 4, [25] * 4]).all()


def test_the_canonical_sign():
    assert np.array_equal(ref.canonical([0.0, -1.0, 0.0, 0.0]), [0, 1, 0, 0]) and np.array_equal(ref.canonical([-0.0, 0.0, -2.0, 1.0]), [0, 0, 2, -1])
    assert np.array_equal(ref.canonical([0.5, -0.5, -0.5, -0.5]), [0.5, -0.5, -0.5, -0.5]) and not np.signbit(ref.canonical([0.0, -1.0, 0.0, 0.0])).any()
    # a take seen by two cameras exactly half a turn apart: joints on the axes (M and N are diagonal, nothing is rounded), w = 0 exactly
    body = np.array([[0, 0, 0], [1, 0, 0], [0, 2, 0], [0, 0, 3], [-2, 0, 0]], np.float32)
    for axis, flip in enumerate(([1, -1, -1], [-1, 1, -1], [-1, -1, 1])):
        poses = np.stack([np.tile(body, (3, 1, 1)), np.tile(body * np.array(flip, np.float32), (3, 1, 1))])
        got = ref.align(poses, iters=2)
        want = np.zeros(4)
        want[1 + axis] = 1.0
        assert np.array_equal(got["quat"][0, 1], want) and not np.signbit(got["quat"][0, 1]).any() and got["ok"][0, 1] == 1
        assert got["rms"][0, 1] == 0 and got["gap"][0, 1] >= ref.GAP_MIN


def test_every_degenerate_rule():
    sc = ref.scene(3, 5, [12], seed=5)
    fill = lambda r, g, v: (np.array_equal(r["quat"][g, v], [1, 0, 0, 0]) and not r["trans"][g, v].any() and r["rms"][g, v] == 0
                            and r["trans_rms"][g, v] == 0 and r["ok"][g, v] == 0)
    args = (sc["off"], sc["traj"], sc["traj_ok"])
    none = ref.align(sc["poses"], np.zeros((3, 12), np.uint8), *args)     # no view has a valid frame: ok = 0 rows, used 0
    assert all(fill(none, 0, v) for v in range(3)) and not none["used"].any()
    valid = np.ones((3, 12), np.uint8)
    valid[0], valid[1, :6], valid[2, 6:] = 0, 0, 0                        # view 0 missing: view 1 is the reference; views 1 and 2 share no frame
    r = ref.align(sc["poses"], valid, *args)
    assert fill(r, 0, 0) and r["used"][0].tolist() == [0, 6, 0] and r["ok"][0].tolist() == [0, 1, 0] and fill(r, 0, 2)
    nan = sc["poses"].copy()
    nan[1, :, 2, 0] = np.nan                                              # every frame of view 1 has a NaN: no used frame
    r = ref.align(nan, None, *args)
    assert fill(r, 0, 1) and r["used"][0].tolist() == [12, 0, 12] and r["ok"][0, 2] == 3
    flat = sc["poses"].copy()
    flat[1] = flat[1][:, :1]                                              # view 1: every joint at the root, M = 0: the dominant eigenvalue is not > 0
    r = ref.align(flat, None, *args)
    assert fill(r, 0, 1) and r["used"][0, 1] == 12
    line = np.zeros((2, 6, 4, 3), np.float32)
    line[0, :, 1:, 0], line[1, :, 1:, 1] = [1, 2, 3], [1, 2, 3]           # identical frames, collinear joints: the rotation about the line is free
    r = ref.align(line)
    assert fill(r, 0, 1) and r["used"][0].tolist() == [6, 6] and r["ok"][0, 0] == 1
    huge = np.zeros((2, 2, 3, 3), np.float32)                             # sum w not > 0: residuals so large against sigma that every weight is 0
    huge[0, 0, 1:], huge[0, 1, 1:] = [[3e38, 0, 0], [0, 3e38, 0]], [[0, 3e38, 0], [3e38, 0, 0]]
    huge[1, 0, 1:], huge[1, 1, 1:] = [[3e38, 0, 0], [0, 3e38, 0]], [[3e38, 0, 0], [0, -3e38, 0]]
    assert ref.align(huge, iters=0)["ok"][0, 1] == 1
    r = ref.align(huge, sigma=1e-40, iters=1)                           # (a denormal float32; (1 + e / sigma^2)^2 overflows)
    assert fill(r, 0, 1) and r["used"][0, 1] == 2
    # a sum that is not finite cannot come from float32 inputs (a used frame is finite and |x|^2 <= 1.2e77); the rule guards the solve itself
    assert ref.solve(np.full((3, 3), np.inf), 1.0)[0] is None and ref.solve(np.eye(3), float("nan"))[0] is None and ref.solve(np.eye(3), 0.0)[0] is None
    tok = sc["traj_ok"].copy()
    tok[2] = 0                                                            # traj_ok nowhere set in view 2: the rotation stands, ok keeps bit 0 only
    r = ref.align(sc["poses"], None, sc["off"], sc["traj"], tok)
    assert r["ok"][0].tolist() == [1, 3, 1] and not r["trans"][0, 2].any() and r["trans_rms"][0, 2] == 0 and r["rms"][0, 2] > 0


def test_composition_with_a_reference_camera():
    from manipose_amd.lift_views import _align_compose
    sc = ref.scene(4, 9, [20, 20], seed=9)
    valid = np.ones((4, 40), np.uint8)
    valid[0, 20:] = 0                                                     # take 1: view 1 is the reference
    tok = sc["traj_ok"].copy()
    tok[3, :20] = 0                                                       # take 0: view 3 has a rotation and no translation
    r = ref.align(sc["poses"], valid, sc["off"], sc["traj"], tok)
    assert r["ok"].tolist() == [[1, 3, 3, 1], [0, 1, 3, 3]]
    g = np.random.default_rng(2)
    ref_quat, ref_trans = 3.0 * g.standard_normal((2, 4)), g.standard_normal((2, 3))      # (not unit: normalised like the kernels' tables)
    q32, t32 = r["quat"].astype(np.float32), r["trans"].astype(np.float32)
    got_q, got_t = _align_compose(q32, t32, r["ok"], ref_quat, ref_trans)
    want_q, want_t = ref.compose(q32, t32, r["ok"], ref_quat, ref_trans)
    assert got_q.dtype == got_t.dtype == np.float32 and np.abs(got_q - want_q).max() <= 2.0 ** -23 and np.abs(got_t - want_t).max() <= 2.0 ** -22 * np.abs(want_t).max()
    assert np.array_equal(got_q[1, 0], [1, 0, 0, 0]) and not got_t[1, 0].any()            # a row without bit 0 stays
    assert not got_t[0, 3].any() and np.abs(got_t[0, 0] - ref_trans[0]).max() < 1e-6 and np.abs(got_t[1, 1] - ref_trans[1]).max() < 1e-6
    assert (got_q[..., 0] >= 0).all()
    x = g.standard_normal(3)                                              # x_world = R_ref (R_v x + T_v) + T_ref
    for gi, v in ((0, 1), (0, 2), (1, 2), (1, 3)):
        Rr = ref.quat_matrix(ref_quat[gi] / np.linalg.norm(ref_quat[gi]))
        want = Rr @ (ref.quat_matrix(q32[gi, v] / np.linalg.norm(q32[gi, v])) @ x + t32[gi, v]) + ref_trans[gi]
        assert np.abs(ref.quat_matrix(got_q[gi, v].astype(np.float64)) @ x + got_t[gi, v] - want).max() < 1e-5
    assert _align_compose(q32, None, r["ok"], ref_quat, ref_trans)[1] is None


def test_recovery_on_the_committed_seed():
    """60 frames, 17 joints, 4 views, noise 0.01 m, 30 % of the frames of views 1..3 depth-mirrored (lift_align_ref.RECOVERY, seed 7).  Measured
    with the float64 statement, degrees off the true rotation per view 1..3:
      plain Horn (iters = 0)                      3.54  1.23  2.44
      robust (iters = 5, sigma = 0.05 m)          0.068 0.098 0.038
      the same scene without mirrored frames      0.071 0.099 0.047   (plain Horn: the statement's own error under the noise)
    The claim: the robust estimate is closer than plain Horn in every view, and in every view within twice the error the statement makes on the
    scene without outliers.  A rotation off by an angle a moves the translation by at most a |root|, the roots' distance from the camera (here up
    to 7 m: 5 to 7 mm measured); the bound below is that plus a millimetre (trans_rms is about 1 mm: the roots carry no noise here)."""
    dirty, clean = ref.recovery()
    plain, _ = ref.errors_deg(dirty, iters=0)
    robust, res = ref.errors_deg(dirty, traj=dirty["traj"], traj_ok=dirty["traj_ok"], sigma=0.05, iters=5)
    own, _ = ref.errors_deg(clean, iters=0)
    print("plain", np.round(plain, 3), "robust", np.round(robust, 3), "without outliers", np.round(own, 3), "gap", np.round(res["gap"][0, 1:], 2))
    assert all(r < p for r, p in zip(robust, plain)) and all(r <= 2.0 * c for r, c in zip(robust, own))
    assert min(plain) > 1.0 and max(robust) < 0.1                        # (the figures of the docstring, loosely: the scene is what it says)
    assert (res["gap"][0, 1:] > 1.0).all() and (res["ok"][0] == [1, 3, 3, 3]).all()
    for v in range(1, 4):
        lever = np.linalg.norm(dirty["traj"][v], axis=1).max()
        assert np.linalg.norm(res["trans"][0, v] - dirty["trans"][0, v]) <= np.radians(robust[v - 1]) * lever + 1e-3


def test_the_device_tests_scenes_are_well_conditioned():
    """the device test claims its bounds where the gap is >= 0.1: every row of its cases that has a rotation is such a row"""
    seen = set()
    for tag, inp, want in ref.cases():
        rot = (want["ok"] & 1).astype(bool) & (want["rms"] > 0)           # (the reference views have no gap)
        assert (want["gap"][rot] >= ref.GAP_MIN).all(), (tag, want["gap"])
        seen |= set(want["ok"].ravel().tolist())
    assert seen == {0, 1, 3}
    frames = {int(inp["poses"].shape[1]) for _, inp, _ in ref.cases()}
    assert {1, 255, 256, 257, 600} <= frames and {2, 5, 17} <= {int(inp["poses"].shape[2]) for _, inp, _ in ref.cases()}


def test_new_abi_symbol_is_declared_everywhere():
    from manipose_amd import _lib, lifting
    import manipose_amd
    header = open(_lib.HEADER_PATH).read()
    assert "mp_lift_align_views" in _lib.declared_symbols() and len(_lib._SIGNATURES["mp_lift_align_views"][1]) == 19
    assert "lib.mp_lift_align_views.argtypes" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert _lib.ABI_VERSION == 8 and int(re.search(r"#define MP_ABI_VERSION (\d+)", header).group(1)) == 8        # purely additive
    assert int(re.search(r"#define MP_LIFT_ALIGN_MAXITERS (\d+)", header).group(1)) == lifting.ALIGN_MAXITERS == 8
    assert manipose_amd.align_views is lifting.align_views and "align_views" in lifting.__all__
    assert (lifting.ALIGN_SIGMA, lifting.ALIGN_ITERS) == (0.05, 5) and lifting.ViewAlignment._fields == ("quat", "trans", "rms", "trans_rms", "used", "ok")
    assert lifting._Lifted._fields == ("poses", "hyps", "bones", "place", "path", "score", "rotations")
    assert os.path.exists(os.path.join(ROOT, "manipose_amd", "csrc", "lift_align.hip"))
    for name in ("README.md", "DESIGN.md"):
        assert "mp_lift_align_views" in open(os.path.join(ROOT, name)).read()
    if os.path.exists(_lib.LIB_PATH):
        assert hasattr(_lib.load(), "mp_lift_align_views")


def test_config_keys_parse_and_an_estimate_without_the_fusion_fails():
    from _entry import LIFT_SUFFIXES, lift_fuse_align_options, lift_fuse_options, load_config, run
    cfg = load_config([])
    assert cfg.lift.fuse_cameras == "dataset" and lift_fuse_align_options(cfg) == (False, 0.05, 5) and lift_fuse_options(cfg) == (False, 0.02, 1.0, 3)
    on = ["run.lift=true", "lift.fuse=true", "lift.fuse_cameras=estimate"]
    assert lift_fuse_align_options(load_config(on + ["lift.fuse_align_sigma=0.1", "lift.fuse_align_iters=0"])) == (True, 0.1, 0)
    assert lift_fuse_align_options(load_config(on)) == (True, 0.05, 5)
    with pytest.raises(SystemExit):
        load_config(["lift.fuse_camera=estimate"])
    fused = ["run.lift=true", "lift.fuse=true"]
    for argv, word in ((fused + ["lift.fuse_cameras=guess"], "dataset or estimate"), (["run.lift=true", "lift.fuse_cameras=estimate"], "set lift.fuse=true"),
                       (["lift.fuse_cameras=estimate"], "set lift.fuse=true"), (fused + ["lift.fuse_align_sigma=0.1"], "set lift.fuse_cameras=estimate"),
                       (fused + ["lift.fuse_align_iters=2"], "set lift.fuse_cameras=estimate"), (on + ["lift.fuse_align_sigma=0"], "> 0"),
                       (on + ["lift.fuse_align_sigma=abc"], "is a number"), (on + ["lift.fuse_align_sigma=true"], "is a number"),
                       (on + ["lift.fuse_align_iters=9"], "0..8"), (on + ["lift.fuse_align_iters=-1"], "0..8"), (on + ["lift.fuse_align_iters=1.5"], "0..8"),
                       (on + ["+data=mpi_inf_3dhp"], "align_views")):
        with pytest.raises(ValueError, match=word):
            run(["run.train=false", "run.test=false"] + argv)                    # (a run that got further would need a device)
    assert all("__cam_" + s in LIFT_SUFFIXES for s in ("quat", "trans", "rms", "trans_rms", "used", "ok", "err_deg", "err_m"))


def test_argument_errors_are_value_errors_before_any_device_work():
    """The calls are given CPU tensors: had the arguments been accepted, they would have ended in the RuntimeError that refuses them ("no CPU
    fallback"), which is what the valid calls at the end do."""
    from manipose_amd import align_views
    poses, valid = torch.zeros(3, 6, 17, 3), torch.ones(3, 6, dtype=torch.uint8)
    traj, tok = torch.zeros(3, 6, 3), torch.ones(3, 6, dtype=torch.uint8)
    cam = np.concatenate([np.ones(9), [1, 0, 0, 0], np.zeros(3)])
    for kw, word in ((dict(poses=torch.zeros(6, 17, 3)), "poses must be"), (dict(poses=poses.double()), "poses must be"), (dict(poses=torch.zeros(5, 6, 17, 3)), "views"),
                     (dict(poses=torch.zeros(3, 6, 1, 3)), "joints"), (dict(poses=torch.zeros(3, 6, 17, 2)), "poses must be"), (dict(valid=valid[:2]), "valid must be"),
                     (dict(valid=valid.bool()), "valid must be"), (dict(traj=traj), "come together"), (dict(traj_ok=tok), "come together"),
                     (dict(traj=traj[:, :5], traj_ok=tok), "traj must be"), (dict(traj=traj.double(), traj_ok=tok), "traj must be"),
                     (dict(traj=traj, traj_ok=tok.float()), "traj_ok must be"), (dict(sigma=0), "sigma"), (dict(sigma=-1.0), "sigma"), (dict(sigma=float("nan")), "sigma"),
                     (dict(sigma="a"), "sigma"), (dict(sigma=True), "sigma"), (dict(iters=9), "iters"), (dict(iters=-1), "iters"), (dict(iters=1.5), "iters"),
                     (dict(iters=True), "iters"), (dict(reference=[cam, cam]), "2 cameras"), (dict(reference=[cam[:5]]), "camera 0"),
                     (dict(reference=np.concatenate([np.ones(9), np.zeros(7)])), "zero quaternion"),
                     (dict(take_offset=[0, 3, 6], reference=cam), "1 cameras")):
        with pytest.raises(ValueError, match=word):
            align_views(**dict(dict(poses=poses), **kw))
    for kw in (dict(), dict(valid=valid, traj=traj, traj_ok=tok, sigma=float("inf"), iters=0, reference=cam), dict(take_offset=[0, 3, 6], reference=[cam, cam])):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            align_views(poses, **kw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        align_views(np.zeros((3, 6, 17, 3), np.float32))

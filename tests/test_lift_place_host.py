"""Placing lifted sequences in the scene, the host side (no GPU): the numpy statement of the fit, the camera model and the world transform
(lift_place_ref.py) against numpy.linalg.lstsq and against the reference's own outputs (tests/golden/place.npz, tools/gen_golden_place.py),
camera_table, the new entry points of the C ABI in the places that declare them, the config keys, and every argument error of lift_sequences
and of the entry point, which are raised before anything touches a device."""
import os
import re
import shlex
import sys

import numpy as np
import pytest
import torch

import lift_place_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hpe"))


def _s11():
    from manipose_amd.data.ingest import h36m_cameras
    return h36m_cameras()["S11"]


def _lstsq(pose, kp, intr, w):
    """the stacked 2J x 3 system sqrt(w_j) [(1, 0, -a_j), (0, 1, -b_j)] t = -sqrt(w_j) (ex_j, ey_j)"""
    fx, fy, cx, cy = np.asarray(intr, np.float64)[:4]
    a, b = (kp[:, 0] - cx) / fx, (kp[:, 1] - cy) / fy
    ex, ey = pose[:, 0] - a * pose[:, 2], pose[:, 1] - b * pose[:, 2]
    r, one, zero = np.sqrt(w), np.ones_like(a), np.zeros_like(a)
    M = np.concatenate([r[:, None] * np.stack([one, zero, -a], 1), r[:, None] * np.stack([zero, one, -b], 1)])
    y = -np.concatenate([r * ex, r * ey])
    return np.linalg.lstsq(M, y, rcond=None)[0], np.linalg.cond(M)


def test_the_fit_is_the_least_squares_solution():
    cams = _s11()
    intr = np.stack([c["intrinsic"] for c in cams[:3]])
    poses, kp, t_true, off = ref.synthetic_scene([1, 7, 5], 5, 3, intr, seed=0)
    g = np.random.default_rng(1)
    worst = 0.0
    for weights in (None, g.uniform(0.5, 2.0, 17), np.where(np.arange(17) % 3 == 0, 0.0, 1.0)):
        traj, err, ok = ref.place_all(poses, kp, intr, off, weights)
        assert ok.all()
        w = np.ones(17) if weights is None else weights
        for s in range(3):
            for n in range(int(off[s]), int(off[s + 1])):
                for i in range(5):
                    keep = w != 0
                    t, cond = _lstsq(poses[n, i, keep].astype(np.float64), kp[n, keep].astype(np.float64), intr[s], w[keep])
                    worst = max(worst, np.abs(traj[n, i] - t).max())
                    assert cond < 1e3
    print(f"\n[fit vs lstsq] max |t - lstsq| = {worst:.2e} (bound 1e-12)")
    assert worst <= 1e-12
    # zero weights: the restatement on the remaining joints alone, exactly
    keep = np.arange(17) % 3 != 0
    a = ref.place_all(poses, kp, intr, off, np.where(keep, 1.0, 0.0))
    b = ref.place_all(poses[:, :, keep], kp[:, keep], intr, off)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    # the noise-free construction is recovered (float32 inputs: 2.6e-7 m measured for the first GPU test's construction)
    poses, kp, t_true, off = ref.synthetic_scene([20], 1, 3, intr[:1], seed=2, noise=0.0)
    traj, err, ok = ref.place_all(poses, kp, intr[:1], off, distort=False)
    assert ok.all() and np.abs(traj[:, 0] - t_true).max() <= 2e-6 and err.max() <= 1e-6


def test_the_degenerate_rule_of_the_statement():
    intr = _s11()[0]["intrinsic"]
    poses, kp, _, _ = ref.synthetic_scene([4], 1, 3, intr[None], seed=3)
    pose, k = poses[0, 0], kp[0]
    zero = (np.zeros(3), 0.0, 0)
    for got in (ref.place_one(pose, k, intr, np.zeros(17)), ref.place_one(pose, np.broadcast_to(k[3], (17, 2)), intr),
                ref.place_one(pose, np.where(np.arange(34).reshape(17, 2) == 9, np.nan, k), intr),
                ref.place_one(np.where(np.arange(51).reshape(17, 3) == 7, np.inf, pose), k, intr)):
        assert np.array_equal(got[0], zero[0]) and got[1] == 0.0 and got[2] == 0
    # a NaN keypoint at a joint of weight 0 is not looked at
    w = np.ones(17)
    w[4] = 0
    bad = k.copy()
    bad[4] = np.nan
    t, err, ok = ref.place_one(pose, bad, intr, w)
    assert ok == 1 and np.isfinite(t).all() and np.isfinite(err)
    # a pose deeper than its fitted distance: solved, stored as computed, ok = 0
    behind = pose.copy()
    behind[5, 2] = -40.0
    t, err, ok = ref.place_one(behind, k, intr)
    assert ok == 0 and np.isfinite(t).all() and np.isfinite(err) and behind[5, 2] + t[2] < 0 and (t != 0).all()


def test_the_statement_reproduces_the_references_outputs(golden_dir):
    z = np.load(os.path.join(golden_dir, "place.npz"))
    X, kp, intr, quat = z["X"], z["kp"], z["intr"], z["quat"]
    assert X.shape == (6, 5, 17, 3) and X.dtype == np.float64 and np.array_equal(X, X.astype(np.float32))       # float32 values
    assert (np.abs(X[..., :2] / X[..., 2:3]).max(axis=(1, 2, 3)) > 1).tolist() == [False] * 4 + [True] * 2       # the clamp is exercised
    t_fit = np.stack([np.stack([ref.place_one(X[n, i], kp[n], intr[n])[0] for i in range(5)]) for n in range(6)])
    assert np.array_equal(t_fit, z["t_fit"])
    worst = 0.0
    for tag, pts in (("", X), ("_fit", X + t_fit[:, :, None, :])):
        for n in range(6):
            worst = max(worst, np.abs(ref.project(pts[n], intr[n], True) - z["proj" + tag][n]).max(),
                        np.abs(ref.project(pts[n], intr[n], False) - z["proj_linear" + tag][n]).max())
    assert not np.allclose(z["proj"], z["proj_linear"], atol=1e-4)        # the distortion terms are not idle
    world = ref.world_all(X, quat, seq_offset=np.arange(7))
    worst = max(worst, np.abs(world - z["world"]).max())
    floored = world.copy()
    for n in range(6):
        floored[n, ..., 2] -= floored[n, ..., 2].min()
    worst = max(worst, np.abs(floored - z["world_floor"]).max())
    print(f"\n[statement vs place.npz] max |difference| = {worst:.2e} (bound 1e-12)")
    assert worst <= 1e-12
    for n in range(6):
        assert np.abs(z["world_floor"][n, ..., 2].min()) == 0.0
    # qrot does not normalise: a scaled quaternion gives another result, and the statement follows the formula
    v = X[0, 0]
    np.testing.assert_allclose(ref.qrot(2 * quat[0], v), v + 2 * (2 * quat[0, 0] * np.cross(2 * quat[0, 1:], v)
                                                                 + np.cross(2 * quat[0, 1:], np.cross(2 * quat[0, 1:], v))), rtol=0, atol=1e-12)
    np.testing.assert_allclose(ref.qrot([1, 0, 0, 0], v), v, rtol=0, atol=0)


def test_camera_table_accepts_both_forms_and_reports_its_errors():
    from manipose_amd import camera_table
    cams = _s11()
    as_dicts = camera_table(cams)
    vecs = [np.concatenate([c["intrinsic"], c["orientation"], c["translation"], np.array([i])]) for i, c in enumerate(cams)]       # fetch()'s rows
    as_vecs = camera_table(vecs)
    for a, b, shape in zip(as_dicts, as_vecs, ((4, 9), (4, 4), (4, 3))):
        assert a.shape == shape and a.dtype == np.float32 and np.array_equal(a, b)
    assert np.array_equal(as_dicts[0][2], cams[2]["intrinsic"]) and np.array_equal(as_dicts[1][1], cams[1]["orientation"])
    assert np.array_equal(as_dicts[2][3], cams[3]["translation"])
    mixed = camera_table([cams[0], vecs[1][:16], torch.from_numpy(vecs[2])])
    assert all(np.array_equal(m, a[:3]) for m, a in zip(mixed, as_dicts))
    no_t = {k: v for k, v in cams[0].items() if k != "translation"}
    assert np.array_equal(camera_table([no_t])[2], np.zeros((1, 3), np.float32))
    bad_quat = dict(cams[0], orientation=np.ones(3, np.float32))
    nan_vec = vecs[0].copy()
    nan_vec[11] = np.nan
    inf_dict = dict(cams[0], translation=np.array([0.0, np.inf, 0.0]))
    for bad, word in (([vecs[0][:15]], "at least 16"), ([np.zeros((4, 4))], "at least 16"), ([bad_quat], "'orientation' must be 4"),
                      ([{"intrinsic": cams[0]["intrinsic"]}], "needs 'intrinsic'"), ([nan_vec], "non-finite"), ([inf_dict], "non-finite"),
                      ([], "empty"), (cams[0], "one camera per sequence"), (vecs[0], "one camera per sequence"), (["abc"], "at least 16")):
        with pytest.raises(ValueError, match=word):
            camera_table(bad)


def test_new_abi_symbols_are_declared_everywhere():
    from manipose_amd import _lib, lifting
    import manipose_amd
    names = _lib.declared_symbols()
    header = open(_lib.HEADER_PATH).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for sym, nargs in (("mp_lift_place", 15), ("mp_lift_world", 15)):
        assert sym in names and sym in _lib._SIGNATURES and len(_lib._SIGNATURES[sym][1]) == nargs
        assert f"lib.{sym}.argtypes" in doc
    assert _lib.ABI_VERSION == 8 and int(re.search(r"#define MP_ABI_VERSION (\d+)", header).group(1)) == 8        # purely additive
    assert int(re.search(r"#define MP_LIFT_WORLD_SHARES (\d+)", header).group(1)) == lifting.FLOOR_SHARES
    for name in ("camera_table", "place_poses", "to_world"):
        assert getattr(manipose_amd, name) is getattr(lifting, name) and name in lifting.__all__
    assert os.path.exists(os.path.join(ROOT, "manipose_amd", "csrc", "lift_place.hip"))
    if os.path.exists(_lib.LIB_PATH):
        lib = _lib.load()
        assert hasattr(lib, "mp_lift_place") and hasattr(lib, "mp_lift_world")


def test_config_keys_parse_a_typo_fails_and_the_readme_command_parses():
    from _entry import lift_place_options, load_config
    cfg = load_config([])
    assert cfg.lift.place is False and cfg.lift.frame == "camera" and cfg.lift.floor is False
    assert lift_place_options(cfg) == (False, False, False)
    cfg = load_config(["lift.place=true", "lift.frame=world", "lift.floor=true"])
    assert cfg.lift.place is True and cfg.lift.frame == "world" and cfg.lift.floor is True
    assert lift_place_options(cfg) == (True, True, True)
    for typo in ("lift.plaec=true", "lift.frames=world", "lift.flor=true"):
        with pytest.raises(SystemExit):
            load_config([typo])
    lines = [l for l in open(os.path.join(ROOT, "README.md")).read().splitlines() if l.startswith("python hpe/") and "lift.place=true" in l]
    assert len(lines) == 1
    argv = shlex.split(lines[0].split("#")[0])[2:]
    cfg = load_config(argv)
    assert cfg.run.lift is True and lift_place_options(cfg) == (True, True, True)


def test_entry_point_errors_come_before_the_model_is_built():
    from _entry import lift_place_options, load_config, run
    for argv, word in ((["lift.frame=wrold"], "camera or world"), (["lift.floor=true"], "lift.frame=world"),
                       (["+data=mpi_inf_3dhp", "lift.place=true"], "carry none"), (["+data=mpi_inf_3dhp", "lift.frame=world"], "carry none")):
        with pytest.raises(ValueError, match=word):
            run(["run.train=false", "run.test=false", "run.lift=true"] + argv)        # (a run that got further would need a device)
    with pytest.raises(ValueError, match="carry none"):                               # the 3DHP script's own defaults
        lift_place_options(load_config(["lift.place=true"], {"data.dataset": "3dhp", "data.seq_len": 27, "data.keypoints": "gt"}))
    assert lift_place_options(load_config(["+data=mpi_inf_3dhp"])) == (False, False, False)


def _cpu_model():
    from manipose_amd import RMCLManifoldMixSTE, h36m_skeleton
    return RMCLManifoldMixSTE(h36m_skeleton(), num_frame=9, embed_dim_rot=32, depth_rot=1, num_heads_rot=4, embed_dim_seg=16, depth_seg=1,
                              num_heads_seg=4, n_hyp=2)


def test_argument_errors_are_value_errors_before_any_device_work():
    """Every call below is given a CPU model: had the arguments been accepted, the call would have ended in the RuntimeError that refuses a CPU
    model ("no CPU fallback"), which is what the valid calls at the end do."""
    from manipose_amd import lift_sequences, place_poses, to_world
    model = _cpu_model()
    seqs = [np.zeros((12, 17, 2), np.float32), np.zeros((20, 17, 2), np.float32)]
    cams = _s11()[:2]
    for kw, word in ((dict(place=True), "place=True needs cameras"), (dict(frame="world"), "frame='world' needs cameras"),
                     (dict(frame="World", cameras=cams), "frame must be"), (dict(floor=True), "frame='world'"),
                     (dict(floor=True, cameras=cams, place=True), "frame='world'"), (dict(cameras=cams), "cameras describe"),
                     (dict(return_place=True), "return_place"), (dict(return_place=True, cameras=cams, frame="world"), "return_place"),
                     (dict(place=True, cameras=cams, keep_padding=True), "keep_padding"), (dict(frame="world", cameras=cams, keep_padding=True), "keep_padding"),
                     (dict(place=True, cameras=_s11()[:3]), "3 cameras for 2 sequences"), (dict(place=True, cameras=cams[0]), "one camera per sequence"),
                     (dict(frame="world", cameras=[cams[0], np.zeros(9)]), "at least 16"),
                     (dict(frame="world", floor=np.zeros(2), cameras=cams), "switches"), (dict(place=1, cameras=cams), "switches")):
        with pytest.raises(ValueError, match=word):
            lift_sequences(model, seqs, **kw)
    for kw in (dict(place=True, cameras=cams), dict(frame="world", cameras=cams), dict(place=True, frame="world", floor=True, cameras=cams,
               return_place=True, return_hyps=True), dict(frame="world", floor=True, cameras=cams, return_place=True, rigid=True), dict()):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            lift_sequences(model, seqs, **kw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        place_poses(torch.zeros(4, 17, 3), torch.zeros(4, 17, 2), cams[0]["intrinsic"])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        to_world(torch.zeros(4, 17, 3), cams[0]["orientation"])

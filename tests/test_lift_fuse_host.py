"""Fusing the camera views of a take, the host side (no GPU): the float64 statement of both rules (lift_fuse_ref.py) against its own quadratic,
against lift_place_ref's single-view fit and against central differences; what the feature is for (the jointly chosen hypotheses against the
per-view best score, the root from four views against the root from one); the decision margins of every scene the GPU tests compare; the two new
entry points in the places that declare them, the config keys, and the argument errors that are raised before anything touches a device."""
import os
import re
import shlex
import sys

import numpy as np
import pytest
import torch

import lift_fuse_ref as ref
import lift_place_ref as place

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hpe"))


def test_the_linear_fit_minimises_its_quadratic_and_one_view_is_place_one():
    pose, kp, _, (quat, trans, intr), off = ref.place_scene(4, lens=[3], seed=1)
    cams = ref.take_cameras(quat, trans, intr, 0, 4)
    for w in (np.ones(17), ref.WEIGHTS.astype(np.float64)):
        for f in range(3):
            kps = [kp[v, f] for v in range(4)]
            H, h, _ = ref.linear_sums(pose[f], kps, cams, w)
            r = np.linalg.solve(H, h)
            got = ref.place_frame(pose[f], kps, cams, w, iters=0)[0]
            assert np.abs(got - r).max() <= 1e-12 * max(1.0, np.abs(r).max())                     # cofactors against LAPACK: cond(H) is about 6
            base = ref.linear_cost(pose[f], kps, cams, w, r)
            for d in np.eye(3):
                for s in (1e-3, -1e-3):
                    assert ref.linear_cost(pose[f], kps, cams, w, r + s * d) > base             # a strict minimum along every axis
    assert np.linalg.cond(H) < 10
    eye = [(np.eye(3), np.zeros(3), intr[0, 1].astype(np.float64))]                               # one view, the identity orientation: mp_lift_place
    poses, kp1, _, _ = place.synthetic_scene([5], 1, 3, intr[0, 1:2], seed=2)
    for f in range(5):
        want = place.place_one(poses[f, 0], kp1[f], intr[0, 1])
        got = ref.place_frame(poses[f, 0], [kp1[f]], eye, iters=0)
        assert np.abs(got[0] - want[0]).max() <= 1e-12 * np.abs(want[0]).max() and abs(got[1][0] - want[1]) <= 1e-12 and got[2] == want[2] == 1
        H, _, _ = ref.linear_sums(poses[f, 0], [kp1[f]], eye, np.ones(17))
    assert np.linalg.cond(H) > 100                                                                # one camera cannot see depth


def test_the_jacobian_matches_central_differences():
    quat, trans, intr = ref.s11_tables()
    g = np.random.default_rng(0)
    for v in range(4):
        R, T, K = ref.rotation(quat[0, v]), trans[0, v].astype(np.float64), intr[0, v].astype(np.float64)
        for distort in (True, False):
            for _ in range(5):
                p = np.concatenate([g.uniform(-1, 1, 2), g.uniform(0.2, 1.8, 1)])
                J = ref.jacobian_view(p, R, T, K, distort)
                num = np.zeros((2, 3))
                for c in range(3):
                    d = np.zeros(3)
                    d[c] = 1e-6
                    num[:, c] = (place.project((p + d - T) @ R, K, distort) - place.project((p - d - T) @ R, K, distort)) / 2e-6
                assert np.abs(J - num).max() <= 1e-8 * max(1.0, np.abs(J).max())


def test_the_views_choose_the_true_hypothesis_where_the_scores_cannot():
    sc = ref.recovery_scene()
    got = ref.fuse_all(sc["hyps"], sc["cams"][0], None, sc["off"])
    right = (got["choice"] == sc["truth"]).all(axis=1)
    by_score = (sc["hyps"][..., 0, 3].argmax(axis=-1).T == sc["truth"]).all(axis=1)                # the per-view first arg-max of the score
    print(f"[recovery] all four views right in {int(right.sum())} of 40 frames (smallest gap to the runner-up {got['gap'].min():.2f}); the per-view "
          f"best score in {int(by_score.sum())} of 40; fused pose within {np.abs(got['pose'] - sc['pose']).max():.2e} m of the true one")
    assert right.all() and got["gap"].min() >= 1.0 and got["ok"].all()
    assert by_score.sum() < 10
    assert np.abs(got["pose"] - sc["pose"]).max() <= 5e-3                                         # the mean of four hypotheses true to 1 mm
    blind = ref.fuse_all(sc["hyps"], sc["cams"][0], None, sc["off"], sigma=float("inf"))
    assert np.array_equal(blind["choice"], sc["hyps"][..., 0, 3].argmax(axis=-1).T)               # sigma = inf: every view on its own


def test_four_views_recover_the_root_one_view_cannot():
    sc = ref.recovery_scene()
    quat, trans, intr = sc["cams"]
    miss = []
    for iters, bound in enumerate(ref.ROOT_MISS):
        root, _, ok, steps = ref.place_all(sc["pose"], sc["kp"], quat, trans, intr, iters=iters)
        miss.append(np.linalg.norm(root - sc["root"], axis=1).max())
        assert ok.all() and (steps == iters).all() and miss[-1] <= bound, (iters, miss[-1])
    noisy = ref.recovery_scene(noise=0.01)
    four = np.linalg.norm(ref.place_all(noisy["pose"], noisy["kp"], quat, trans, intr, iters=3)[0] - noisy["root"], axis=1).max()
    single = []
    for v in range(4):
        valid = np.zeros((4, 40), np.uint8)
        valid[v] = 1
        root, _, ok, _ = ref.place_all(noisy["pose"], noisy["kp"], quat, trans, intr, valid=valid, iters=3)
        single.append(np.linalg.norm(root - noisy["root"], axis=1).max())
        assert ok.all() and four < single[-1] / 4
    print(f"[recovery] root miss after 0..3 steps: {', '.join(f'{m:.2e}' for m in miss)} m; keypoint noise 0.01: four views {four:.2e} m, one view "
          f"{', '.join(f'{m:.2e}' for m in single)} m")


def test_margins_of_the_gpu_inputs():
    """Every comparison scene of test_gpu_lift_fuse.py: the best combination leads the second by at least 1e-6 (1 + |E|), and every threshold
    decision of the root fit - det against 1e-12 H00 H11 H22, a weighted joint's depth against 0, F' / F - 1 against the slack 1e-6 - lies at least
    1e-3 (relative) from its threshold, so that fp64 contraction differences between the kernel and numpy cannot flip a choice, ok or steps."""
    worst = np.inf
    for tag, _, _, _, _, want in ref.fuse_cases():
        rel = want["gap"] / (1.0 + np.abs(want["cost"]))
        worst = min(worst, rel.min())
        assert rel.min() >= 1e-6, tag
    sc = ref.recovery_scene()
    got = ref.fuse_all(sc["hyps"], sc["cams"][0], None, sc["off"])
    assert (got["gap"] / (1.0 + np.abs(got["cost"]))).min() >= 1e-6
    print(f"[margins] mp_lift_fuse: E gap / (1 + |E|) at least {worst:.2e} over {len(ref.fuse_cases())} scenes")
    low = np.inf
    for case in ref.place_cases():
        m = ref.margin(case[-1])
        low = min(low, m)
        assert m >= 1e-3, case[0]
    trace = []
    ref.place_all(sc["pose"], sc["kp"], *sc["cams"], iters=3, trace=trace)
    assert ref.margin(trace) >= 1e-3
    print(f"[margins] mp_lift_fuse_place: every decision at least {min(low, ref.margin(trace)):.2e} from its threshold")


def test_the_degenerate_frames_are_what_they_were_built_for():
    pose, kp, cams, off, valid = ref.degenerate_place_scene()
    root, reproj, ok, steps = ref.place_all(pose, kp, *cams, valid, off, iters=3)
    assert ok[ref.BEHIND] == 0 and steps[ref.BEHIND] == 0 and np.abs(root[ref.BEHIND]).max() > 0 and reproj[:, ref.BEHIND].min() > 0
    assert ok[ref.NO_VIEW] == 0 and not root[ref.NO_VIEW].any() and not reproj[:, ref.NO_VIEW].any()
    clean = [f for f in range(8) if f not in (ref.BEHIND, ref.NO_VIEW)]
    assert ok[clean].all() and (steps[clean] == 3).all()                                          # ONE_SPOT too: four views' rays still meet
    trace = []
    ref.place_all(pose, kp, *cams, valid, off, iters=3, trace=trace)
    assert ref.margin(trace) >= 1e-3                                                              # (the scene is compared like the others)
    one = np.zeros((4, 8), np.uint8)                                                              # one view alone: all keypoints on one spot is degenerate
    one[0] = 1
    root1, reproj1, ok1, _ = ref.place_all(pose, kp, *cams, one, off, iters=3)
    assert ok1[ref.ONE_SPOT] == 0 and not root1[ref.ONE_SPOT].any() and not reproj1[:, ref.ONE_SPOT].any()


def test_new_abi_symbols_are_declared_everywhere():
    from manipose_amd import _lib, lifting
    import manipose_amd
    header = open(_lib.HEADER_PATH).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    declared = _lib.declared_symbols()
    assert "mp_lift_fuse" in declared and "mp_lift_fuse_place" in declared
    assert len(_lib._SIGNATURES["mp_lift_fuse"][1]) == 18 and len(_lib._SIGNATURES["mp_lift_fuse_place"][1]) == 19
    assert "lib.mp_lift_fuse.argtypes" in doc and "lib.mp_lift_fuse_place.argtypes" in doc
    assert _lib.ABI_VERSION == 8 and int(re.search(r"#define MP_ABI_VERSION (\d+)", header).group(1)) == 8        # purely additive
    assert int(re.search(r"#define MP_LIFT_FUSE_MAXV (\d+)", header).group(1)) == lifting.FUSE_MAXV == 4
    assert int(re.search(r"#define MP_LIFT_FUSE_MAXK (\d+)", header).group(1)) == lifting.FUSE_MAXK == 8
    for name in ("fuse_views", "place_views"):
        assert getattr(manipose_amd, name) is getattr(lifting, name) and name in lifting.__all__
    assert lifting._Lifted._fields == ("poses", "hyps", "bones", "place", "path", "score", "rotations")
    assert os.path.exists(os.path.join(ROOT, "manipose_amd", "csrc", "lift_fuse.hip"))
    if os.path.exists(_lib.LIB_PATH):
        assert hasattr(_lib.load(), "mp_lift_fuse") and hasattr(_lib.load(), "mp_lift_fuse_place")


def test_config_keys_parse_a_typo_fails_and_the_readme_command_parses():
    from _entry import LIFT_SUFFIXES, lift_fuse_options, load_config, run, split_takes
    cfg = load_config([])
    assert cfg.lift.fuse is False and lift_fuse_options(cfg) == (False, 0.02, 1.0, 3)
    cfg = load_config(["run.lift=true", "lift.fuse=true", "lift.fuse_sigma=0.05", "lift.fuse_score_weight=0", "lift.fuse_refine=5"])
    assert lift_fuse_options(cfg) == (True, 0.05, 0.0, 5)
    with pytest.raises(SystemExit):
        load_config(["lift.fuze=true"])
    on = ["run.lift=true", "lift.fuse=true"]
    for argv, word in ((["run.lift=true", "lift.fuse=1"], "true or false"), (["lift.fuse=true"], "set run.lift=true"),
                       (on + ["+data=mpi_inf_3dhp"], "carry none"), (on + ["data.data_dir=/nowhere", "model.arch=mixste"], "rmcl_manifold"),
                       (on + ["data.data_dir=/nowhere", "multi_hyp.n_hyp=1"], "rmcl_manifold"), (on + ["+lift.keep_padding=true"], "keep_padding"),
                       (["run.lift=true", "lift.fuse_sigma=0.05"], "set lift.fuse=true"), (["run.lift=true", "lift.fuse_score_weight=2"], "set lift.fuse=true"),
                       (["run.lift=true", "lift.fuse_refine=2"], "set lift.fuse=true"), (on + ["lift.fuse_sigma=0"], "> 0"),
                       (on + ["lift.fuse_sigma=abc"], "is a number"), (on + ["lift.fuse_score_weight=-1"], ">= 0"),
                       (on + ["lift.fuse_refine=17"], "0..16"), (on + ["lift.fuse_refine=1.5"], "0..16"), (on + ["lift.fuse_refine=true"], "0..16")):
        with pytest.raises(ValueError, match=word):
            run(["run.train=false", "run.test=false"] + argv)                    # (a run that got further would need a device)
    assert all(s in LIFT_SUFFIXES for s in ("__root", "__choice", "__spread", "__cost", "__views", "__ok", "__reproj", "__steps", "__floor"))
    cam = lambda i: np.concatenate([np.zeros(16), [i]])
    assert split_takes([cam(i) for i in (0, 1, 2, 3, 0, 1, 2)]) == [[0, 1, 2, 3], [4, 5, 6]]
    assert split_takes([cam(i) for i in (0, 2, 2, 1, 3)]) == [[0, 1], [2], [3, 4]]
    assert split_takes([{"intrinsic": 0}, {"intrinsic": 0}]) == [[0], [1]]       # no camera index: every sequence a take of its own
    lines = [l for l in open(os.path.join(ROOT, "README.md")).read().splitlines() if l.startswith("python hpe/") and "lift.fuse=" in l]
    assert len(lines) == 1
    cfg = load_config(shlex.split(lines[0].split("#")[0])[2:])
    assert cfg.run.lift is True and lift_fuse_options(cfg) == (True, 0.02, 1.0, 3)


def test_argument_errors_are_value_errors_before_any_device_work():
    """The calls are given CPU tensors: had the arguments been accepted, they would have ended in the RuntimeError that refuses them ("no CPU
    fallback"), which is what the valid calls at the end do."""
    from manipose_amd import fuse_views, place_views
    from manipose_amd.data.ingest import h36m_cameras
    cams = h36m_cameras()["S11"]
    hyps, quat = torch.zeros(4, 6, 5, 17, 4), np.stack([c["orientation"] for c in cams])
    for bad, word in ((torch.zeros(6, 5, 17, 4), "hyps must be"), (hyps.double(), "hyps must be"), (torch.zeros(5, 6, 5, 17, 4), "views"),
                      (torch.zeros(4, 6, 9, 17, 4), "hypotheses"), (torch.zeros(4, 6, 5, 1, 4), "joints"), (torch.zeros(4, 6, 5, 17, 2), "hyps must be")):
        with pytest.raises(ValueError, match=word):
            fuse_views(bad, quat)
    zero, nan = quat.copy(), quat.copy()
    zero[2], nan[1, 0] = 0, np.nan
    for kw, word in ((dict(orientation=zero), "zero quaternion"), (dict(orientation=nan), "finite"), (dict(orientation=quat[:3]), "orientation must be"),
                     (dict(valid=torch.ones(4, 5, dtype=torch.uint8)), "valid must be"), (dict(valid=torch.ones(4, 6)), "valid must be"),
                     (dict(sigma=0), "must be > 0"), (dict(sigma=float("nan")), "must be > 0"), (dict(sigma="a"), "numbers"),
                     (dict(score_weight=-1), ">= 0"), (dict(score_weight=float("inf")), ">= 0"), (dict(score_weight=True), "numbers")):
        with pytest.raises(ValueError, match=word):
            fuse_views(hyps, **{"orientation": quat, **kw})
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fuse_views(hyps, np.stack([quat, quat]), torch.ones(4, 6, dtype=torch.uint8), [0, 2, 6], sigma=float("inf"), score_weight=0)
    pose, kp, nested = torch.zeros(6, 17, 3), torch.zeros(4, 6, 17, 2), [list(cams)]
    no_q = dict(cams[1], orientation=np.zeros(4, np.float32))
    for args, kw, word in (((torch.zeros(6, 17, 4), kp, nested), {}, "pose must be"), ((pose, torch.zeros(4, 5, 17, 2), nested), {}, "keypoints_2d must be"),
                           ((pose, torch.zeros(5, 6, 17, 2), nested), {}, "keypoints_2d must be"), ((pose, kp, [list(cams[:3])]), {}, "must list 4 views"),
                           ((pose, kp, cams[0]), {}, "nested list"), ((pose, kp, [[cams[0], no_q, None, None]]), {}, "zero quaternion"),
                           ((pose, kp, [[cams[0], {"intrinsic": np.zeros(9)}, None, None]]), {}, "view 1"),
                           ((pose, kp, nested), dict(refine=17), "0..16"), ((pose, kp, nested), dict(refine=True), "0..16"),
                           ((pose, kp, nested), dict(weights=-np.ones(17)), "non-negative"), ((pose, kp, nested), dict(weights=np.ones(16)), "weights must be"),
                           ((pose, kp, nested), dict(valid=torch.ones(6, 4, dtype=torch.uint8)), "valid must be")):
        with pytest.raises(ValueError, match=word):
            place_views(*args, **kw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        place_views(pose, kp, [[cams[0], None, cams[2], None]], weights=np.ones(17), refine=0, return_steps=True)

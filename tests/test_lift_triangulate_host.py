"""Triangulating a fused take's joints, without a device: the float64 statement of mp_lift_triangulate's rule (lift_triangulate_ref.py) held against
central differences, against numpy's least squares and against every rule of the fallbacks; the margins of the scenes the device test compares;
the recovery claims on committed seeds; and what the new entry point needs declared around it."""
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

import lift_bundle_ref as bundle
import lift_triangulate_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hpe"))
INF = float("inf")


def _item(V=4, seed=500, f=1, j=3, weights=False):
    """(observations, X0, truth) of one item of a noisy scene"""
    sc = ref.scene(V, 5, [3], seed=seed)
    units = [[bundle.rotation(bundle.unit(sc["quat"][0, v])) for v in range(V)]]
    w = ref.weight_table(V, 3, 5, seed)[:, :, :] + np.float32(0.1) if weights else None
    obs = ref.observations(sc["kp"], w, None, units, sc["trans"].astype(np.float64), sc["intr"].astype(np.float64), 0, f, j)
    X0 = tuple(np.float64(sc["pose"][f, j, c]) + np.float64(sc["root"][f, c]) for c in range(3))
    return obs, X0, sc["truth"][f, j]


@pytest.mark.parametrize("distort", [False, True])
@pytest.mark.parametrize("sigma,prior", [(INF, 0.0), (0.05, 0.0), (0.004, 0.02)])
def test_jacobian_and_gradient_against_central_differences(distort, sigma, prior):
    """J_pi R^T against central differences of the residual, and g against half the central differences of F itself (rho' = omega, so
    dF/dX = 2 g, the prior's term included).  h = 1e-6 m: the truncation is O(h^2) of third derivatives of order 1 / Z^3 < 0.1, the rounding
    1e-16 / h = 1e-10; 1e-7 relative to the largest entry bounds both with room."""
    obs, X0, truth = _item(weights=True)
    X = np.asarray(truth) + np.array([0.02, -0.015, 0.01])
    sigma2 = np.float64(sigma) * np.float64(sigma)
    h = 1e-6
    for o in obs:
        _, rows, _, _ = ref.residual_jac(o, tuple(X), distort)
        num = np.zeros((2, 3))
        for c in range(3):
            d = np.zeros(3); d[c] = h
            (up, vp), _, _, _ = ref.residual_jac(o, tuple(X + d), distort)
            (um, vm), _, _, _ = ref.residual_jac(o, tuple(X - d), distort)
            num[:, c] = ((up - um) / (2 * h), (vp - vm) / (2 * h))
        J = np.array(rows, np.float64)
        assert np.abs(J - num).max() <= 1e-7 * np.abs(J).max()
    pull = prior > 0
    e = ref.evaluate(obs, tuple(X), sigma2, np.float64(prior), X0, pull, distort)
    grad = np.zeros(3)
    for c in range(3):
        d = np.zeros(3); d[c] = h
        grad[c] = (ref.evaluate(obs, tuple(X + d), sigma2, np.float64(prior), X0, pull, distort)["F"]
                   - ref.evaluate(obs, tuple(X - d), sigma2, np.float64(prior), X0, pull, distort)["F"]) / (2 * h)
    g = np.array(e["g"], np.float64)
    print("g", g, "dF/dX / 2", grad / 2)
    assert np.abs(g - grad / 2).max() <= 1e-7 * max(np.abs(g).max(), 1e-3)
    # H = sum (w omega) (J R^T)^T (J R^T) + prior I, formed with numpy from the same rows
    H = np.zeros((3, 3))
    for o in obs:
        (du, dv), rows, _, _ = ref.residual_jac(o, tuple(X), distort)
        t = 1.0 + (du * du + dv * dv) / sigma2
        J = np.array(rows, np.float64)
        H += float(o.w) / float(t * t) * J.T @ J
    H += prior * np.eye(3)
    got = np.array([[e["H"][0], e["H"][1], e["H"][2]], [e["H"][1], e["H"][3], e["H"][4]], [e["H"][2], e["H"][4], e["H"][5]]], np.float64)
    assert np.abs(got - H).max() <= 1e-12 * np.abs(H).max()


def test_sigma_inf_is_exactly_unweighted_and_prior_zero_drops_the_prior():
    obs, X0, truth = _item(weights=True)
    X = tuple(np.asarray(truth) + 0.01)
    e = ref.evaluate(obs, X, np.float64(INF) * np.float64(INF), np.float64(0), X0, False, True)
    F, H, g = np.float64(0), [np.float64(0)] * 6, [np.float64(0)] * 3
    for o in obs:                                                         # the same sums with no robust factor written at all
        (du, dv), (r0, r1), _, _ = ref.residual_jac(o, X, True)
        F += o.w * (du * du + dv * dv)
        ref.normal_add(H, g, o.w, du, dv, r0, r1)
    assert e["F"] == F and e["H"] == H and e["g"] == g                  # bit for bit
    far = (X0[0] + 1.0, X0[1] - 2.0, X0[2] + 0.5)
    a = ref.evaluate(obs, X, np.float64(0.0025), np.float64(0), X0, False, True)
    b = ref.evaluate(obs, X, np.float64(0.0025), np.float64(0), far, False, True)
    assert a["F"] == b["F"] and a["H"] == b["H"] and a["g"] == b["g"]   # prior = 0: X0 appears nowhere
    c = ref.evaluate(obs, X, np.float64(0.0025), np.float64(0.01), X0, True, True)
    assert c["F"] > a["F"] and c["H"][0] == a["H"][0] + 0.01 and c["H"][1] == a["H"][1]
    sc = ref.scene(4, 5, [3], seed=501)
    one = ref.triangulate(**ref.inputs(sc, sigma=INF))
    two = ref.triangulate(**ref.inputs(sc, sigma=1e30))                   # sigma^2 = 1e60 is finite, and 1 + e / 1e60 is 1 all the same
    assert np.array_equal(one["points"], two["points"]) and np.array_equal(one["steps"], two["steps"])


@pytest.mark.parametrize("V,weights", [(2, False), (3, True), (4, False), (4, True)])
def test_linear_start_against_numpy_least_squares(V, weights):
    for j in range(5):
        obs, _, truth = _item(V=V, seed=510 + V, j=j, weights=weights)
        H, h = ref.linear_sums(obs)
        det, scale, passed, x = ref.solve3(H, h)
        A, b = ref.linear_rows(obs)
        want = np.linalg.lstsq(A, b, rcond=None)[0]
        assert passed and np.abs(np.array(x, np.float64) - want).max() <= 1e-9
        assert np.linalg.norm(want - truth) < 0.05                        # (and it is the joint, to the keypoints' noise)


def test_every_rule_of_the_fallbacks():
    inp, trace = ref.constructed(), []
    got = ref.triangulate(trace=trace, **inp)
    X0 = inp["pose"].astype(np.float64) + inp["root"].astype(np.float64)[:, None]
    f = ref.NO_VIEW                                                       # n = 0, X0 usable: the prior point, nothing to step on
    assert (got["views"][f] == 0).all() and (got["ok"][f] == 1).all() and (got["steps"][f] == 0).all() and (got["err"][f] == 0).all()
    assert np.array_equal(got["points"][f], X0[f])
    f = ref.NOTHING                                                       # n = 0 and no usable X0: fails
    assert (got["ok"][f] == 0).all() and (got["points"][f] == 0).all() and (got["err"][f] == 0).all() and (got["steps"][f] == 0).all()
    f = ref.ONE_VIEW                                                      # n = 1, prior = 0: H has rank 2, stays at X0
    assert (got["views"][f] == 1).all() and (got["ok"][f] == 1).all() and (got["steps"][f] == 0).all() and np.array_equal(got["points"][f], X0[f])
    assert (got["err"][f] > 0).all()
    f = ref.NAN_KP                                                        # a NaN keypoint: that view is no observation
    assert (got["views"][f] == 0b1101).all() and (got["ok"][f] == 3).all()
    f = ref.WEIGHTS                                                       # a zero, a negative and a NaN weight: not observed, no error
    assert (got["views"][f] == 0b1000).all() and (got["ok"][f] == 1).all() and np.array_equal(got["points"][f], X0[f])
    f = ref.NO_ROOT                                                       # root_ok = 0 under four views: triangulated all the same
    assert (got["views"][f] == 15).all() and (got["ok"][f] == 3).all() and (got["steps"][f] == 3).all()
    f = ref.BEHIND                                                        # the linear start lies behind camera 0: once more from X0, bit 1 cleared
    assert (got["views"][f] == 3).all() and (got["ok"][f] == 1).all()
    for j in range(5):                                                    # per item: the triangulated start is not deep, the start from X0 is
        deep = [d["taken"] for d in trace if d["item"] == (f, j) and d["kind"] == "deep"]
        assert deep[:2] == [False, True]
    refused = [d for d in trace if d["item"][0] == f and d["kind"] == "cost"]
    assert len(refused) == 5 and not any(d["taken"] for d in refused)    # A REFUSED STEP: the cost would rise, the state stays
    assert (got["steps"][f] == 0).all() and np.array_equal(got["points"][f], X0[f])
    assert (got["ok"][ref.PLAIN] == 3).all() and (got["steps"][ref.PLAIN] == 3).all()
    # with a prior the one-view joints move towards their ray, and the frame without a root stays what it was (X0 unusable: no pull)
    pulled = ref.triangulate(**ref.constructed(prior=0.01))
    assert np.array_equal(pulled["points"][ref.NO_ROOT], got["points"][ref.NO_ROOT])
    for f in (ref.ONE_VIEW, ref.WEIGHTS):
        assert (pulled["steps"][f] > 0).all() and (pulled["ok"][f] == 1).all() and (pulled["err"][f] < 0.25 * got["err"][f]).all()
        assert (np.linalg.norm(pulled["points"][f] - X0[f], axis=1) > 1e-3).all()
    assert np.array_equal(pulled["points"][ref.NO_VIEW], X0[ref.NO_VIEW]) and (pulled["ok"][ref.NOTHING] == 0).all()
    # two views with identical cameras: a degenerate start, and with prior = 0 no step either
    inp, trace = ref.twins(), []
    got = ref.triangulate(trace=trace, **inp)
    assert (got["views"] == 3).all() and (got["ok"] == 1).all() and (got["steps"] == 0).all()
    assert np.array_equal(got["points"], inp["pose"].astype(np.float64) + inp["root"].astype(np.float64)[:, None])
    assert not any(d["taken"] for d in trace if d["kind"] in ("det0", "det")) and sum(d["kind"] == "det0" for d in trace) == 15
    # a zero quaternion: the view is invalid in its take
    got = ref.triangulate(**ref.zero_quaternion())
    assert (got["views"] == 0b110).all() and (got["ok"] == 3).all()
    # a frame no take holds is not written
    sc = ref.scene(2, 5, [6], seed=423)
    got = ref.triangulate(**ref.inputs(sc, take_offset=[1, 4]))
    assert got["written"].tolist() == [False, True, True, True, False, False] and (got["ok"][[0, 4, 5]] == 0).all() and (got["ok"][1:4] == 3).all()


def test_every_compared_scene_is_far_from_every_threshold():
    """what the device test relies on: every decision of every scene it compares with the statement is at least MARGIN_MIN of its slack from its
    threshold, so that rounding differences far below a float32 store cannot flip one"""
    for tag, _, want, trace in ref.cases():
        assert ref.margin(trace) >= ref.MARGIN_MIN, (tag, ref.margin(trace))
        assert want["written"].all()
    tags = " | ".join(c[0] for c in ref.cases())
    for word in ("F=1 V=4 J=17", "F=5 V=4", "F=16 V=2", "F=65 V=4", "F=257 V=4 J=2", "V=3 J=5", "V=1 J=17", "three takes", "iters=0", "iters=1", "iters=16",
                 "pinhole", "prior 0.01", "sigma=0.004", "view 2 missing", "weights with zeros"):
        assert word in tags, word
    for inp in (ref.constructed(), ref.constructed(0.01), ref.twins(), ref.zero_quaternion(), ref.inputs(ref.recovery(4, 0.002))):
        trace = []
        ref.triangulate(trace=trace, **inp)
        assert ref.margin(trace) >= ref.MARGIN_MIN
    both = [c for c in ref.cases() if "weights" in c[0]]                 # the weighted cases reach every kind of item
    assert all(set(np.unique(c[2]["ok"])) == {0, 1, 3} for c in both)


def test_recovery_on_the_committed_seeds():
    """the four claims, re-measured with the statement; each bound is twice the value measured (lift_triangulate_ref.py has them)"""
    sc = ref.recovery(4, 0.0)
    lifted = ref.lifted_errors(sc).mean()
    got = ref.triangulate(**ref.inputs(sc, iters=ref.RECOVERY_STEPS_4V))
    worst4 = ref.errors(got["points"], sc).max()
    print(f"claim 1: 4 views, {ref.RECOVERY_STEPS_4V} steps, noise-free: max {worst4:.3e} m (mean {ref.errors(got['points'], sc).mean():.3e}); lifted mean {lifted:.4f}")
    assert (got["ok"] == 3).all() and worst4 <= ref.RECOVERY_4V
    sc2 = ref.recovery(2, 0.0)
    got = ref.triangulate(**ref.inputs(sc2, iters=ref.RECOVERY_STEPS_2V))
    worst2 = ref.errors(got["points"], sc2).max()
    print(f"claim 1: 2 views, {ref.RECOVERY_STEPS_2V} steps, noise-free: max {worst2:.3e} m")
    assert (got["ok"] == 3).all() and worst2 <= ref.RECOVERY_2V
    noisy = ref.recovery(4, 0.002)
    got = ref.triangulate(**ref.inputs(noisy, iters=3))
    mean = ref.errors(got["points"], noisy).mean()
    print(f"claim 2: 4 views, noise 0.002, 3 steps: mean {mean:.5f} m against the lifted pose's {ref.lifted_errors(noisy).mean():.5f} m")
    assert mean < 0.25 * ref.lifted_errors(noisy).mean()
    one = ref.recovery(1, 0.002)
    got = ref.triangulate(**ref.inputs(one, iters=3, prior=ref.ONE_VIEW_PRIOR))
    mean = ref.errors(got["points"], one).mean()
    print(f"claim 3: 1 view, prior {ref.ONE_VIEW_PRIOR}, noise 0.002, 3 steps: mean {mean:.5f} m against the lifted pose's {ref.lifted_errors(one).mean():.5f} m")
    assert (got["ok"] == 1).all() and mean < ref.lifted_errors(one).mean()
    off = ref.recovery(4, 0.0, ref.ROOT_OFF)
    got = ref.triangulate(**ref.inputs(off, iters=ref.RECOVERY_STEPS_4V))
    worst = ref.errors(got["points"], off).max()
    print(f"claim 4: the root {ref.ROOT_OFF} m N(0, 1) off (prior points {ref.lifted_errors(off).mean():.3f} m off): max {worst:.3e} m")
    assert (got["ok"] == 3).all() and worst <= ref.RECOVERY_4V
    exact = ref.triangulate(**ref.inputs(sc, iters=ref.RECOVERY_STEPS_4V))
    assert np.array_equal(got["points"], exact["points"])                 # the start does not depend on X0 where the linear start stands


def test_new_abi_symbol_is_declared_everywhere():
    from manipose_amd import _lib, lifting
    import manipose_amd
    header = open(_lib.HEADER_PATH).read()
    assert "mp_lift_triangulate" in _lib.declared_symbols() and len(_lib._SIGNATURES["mp_lift_triangulate"][1]) == 24
    assert _lib.ABI_VERSION == 8 and int(re.search(r"#define MP_ABI_VERSION (\d+)", header).group(1)) == 8        # purely additive
    assert int(re.search(r"#define MP_LIFT_REFINE_MAXITERS (\d+)", header).group(1)) == lifting.REFINE_MAXITERS == ref.MAXITERS == 16
    assert manipose_amd.triangulate_views is lifting.triangulate_views and "triangulate_views" in lifting.__all__
    assert lifting.ViewTriangulation._fields == ("points", "err", "views", "ok", "steps")
    assert os.path.exists(os.path.join(ROOT, "manipose_amd", "csrc", "lift_triangulate.hip"))
    source = open(os.path.join(ROOT, "manipose_amd", "csrc", "lift_triangulate.hip")).read()
    assert source.index("#pragma clang fp contract(off)") < source.index('#include "lift_geom.h"')
    assert "lib.mp_lift_triangulate.argtypes" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ("README.md", "DESIGN.md"):
        text = open(os.path.join(ROOT, name)).read()
        assert "mp_lift_triangulate" in text and "lift.fuse_triangulate" in text
    config = open(os.path.join(ROOT, "hpe", "conf", "config.yaml")).read()
    assert all(k in config for k in ("fuse_triangulate:", "fuse_triangulate_steps:", "fuse_triangulate_sigma:", "fuse_triangulate_prior:"))
    assert "--triangulate" in open(os.path.join(ROOT, "tools", "lift_bench.py")).read()
    if os.path.exists(_lib.LIB_PATH):
        assert hasattr(_lib.load(), "mp_lift_triangulate")


def test_config_keys_parse_and_a_triangulation_without_a_fusion_fails():
    from _entry import LIFT_SUFFIXES, lift_fuse_triangulate_options, load_config, run
    cfg = load_config([])
    assert cfg.lift.fuse_triangulate is False and lift_fuse_triangulate_options(cfg) == (False, 3, INF, 0.0)
    on = ["run.lift=true", "lift.fuse=true"]
    assert lift_fuse_triangulate_options(load_config(on)) == (False, 3, INF, 0.0)
    assert lift_fuse_triangulate_options(load_config(on + ["lift.fuse_triangulate=true"])) == (True, 3, INF, 0.0)
    assert lift_fuse_triangulate_options(load_config(on + ["lift.fuse_triangulate=true", "lift.fuse_triangulate_steps=16", "lift.fuse_triangulate_sigma=0.05",
                                                           "lift.fuse_triangulate_prior=0.01"])) == (True, 16, 0.05, 0.01)
    assert lift_fuse_triangulate_options(load_config(on + ["lift.fuse_triangulate=true", "lift.fuse_triangulate_sigma=inf"]))[2] == INF
    with pytest.raises(SystemExit):
        load_config(["lift.fuse_triangulates=true"])
    tri = on + ["lift.fuse_triangulate=true"]
    for argv, word in ((["lift.fuse_triangulate=true"], "set lift.fuse=true"), (["run.lift=true", "lift.fuse_triangulate=true"], "set lift.fuse=true"),
                       (on + ["lift.fuse_triangulate_steps=2"], "set lift.fuse_triangulate=true"), (on + ["lift.fuse_triangulate_sigma=0.1"], "set lift.fuse_triangulate=true"),
                       (on + ["lift.fuse_triangulate_prior=0.1"], "set lift.fuse_triangulate=true"), (on + ["lift.fuse_triangulate=1"], "true or false"),
                       (tri + ["lift.fuse_triangulate_steps=17"], "0..16"), (tri + ["lift.fuse_triangulate_steps=-1"], "0..16"),
                       (tri + ["lift.fuse_triangulate_steps=1.5"], "0..16"), (tri + ["lift.fuse_triangulate_steps=true"], "0..16"),
                       (tri + ["lift.fuse_triangulate_sigma=0"], "> 0"), (tri + ["lift.fuse_triangulate_sigma=-1"], "> 0"),
                       (tri + ["lift.fuse_triangulate_sigma=abc"], "is a number"), (tri + ["lift.fuse_triangulate_prior=-0.1"], "finite and >= 0"),
                       (tri + ["lift.fuse_triangulate_prior=inf"], "finite and >= 0"), (tri + ["lift.fuse_triangulate_prior=true"], "is a number")):
        with pytest.raises(ValueError, match=word):
            run(["run.train=false", "run.test=false"] + argv)                    # (a run that got further would need a device)
    assert all(s in LIFT_SUFFIXES for s in ("__tri", "__tri_err", "__tri_views", "__tri_ok", "__tri_steps"))


def test_argument_errors_are_value_errors_before_any_device_work():
    """The calls are given CPU tensors: had the arguments been accepted, they would have ended in the RuntimeError that refuses them ("no CPU
    fallback"), which is what the valid calls at the end do."""
    from manipose_amd import triangulate_views
    pose, root, kp = torch.zeros(6, 17, 3), torch.zeros(6, 3), torch.zeros(3, 6, 17, 2)
    cam = np.concatenate([np.ones(9), [1, 0, 0, 0], np.zeros(3)])
    cams, ok, w = [[cam, cam, cam]], torch.ones(6, dtype=torch.uint8), torch.ones(3, 6, 17)
    base = dict(pose=pose, root=root, keypoints_2d=kp, cameras=cams)
    for kw, word in ((dict(pose=torch.zeros(6, 17, 2)), "pose must be"), (dict(pose=pose.double()), "pose must be"), (dict(root=torch.zeros(5, 3)), "root must be"),
                     (dict(root=root.double()), "root must be"), (dict(keypoints_2d=torch.zeros(5, 6, 17, 2)), "keypoints_2d"),
                     (dict(keypoints_2d=torch.zeros(3, 6, 16, 2)), "keypoints_2d"), (dict(valid=torch.ones(2, 6, dtype=torch.uint8)), "valid must be"),
                     (dict(root_ok=torch.ones(5, dtype=torch.uint8)), "root_ok must be"), (dict(root_ok=ok.bool()), "root_ok must be"),
                     (dict(kp_weight=torch.ones(3, 6, 16)), "kp_weight must be"), (dict(kp_weight=w.double()), "kp_weight must be"),
                     (dict(kp_weight=np.ones((3, 6, 17), np.float32)), "kp_weight must be"), (dict(kp_weight=torch.ones(6, 17)), "kp_weight must be"),
                     (dict(cameras=[[cam, cam]]), "3 views"), (dict(cameras=[[cam, np.concatenate([np.ones(9), np.zeros(7)]), cam]]), "zero quaternion"),
                     (dict(sigma=0), "sigma"), (dict(sigma=-1.0), "sigma"), (dict(sigma=float("nan")), "sigma"), (dict(sigma="a"), "sigma"), (dict(sigma=True), "sigma"),
                     (dict(prior=-0.1), "prior"), (dict(prior=INF), "prior"), (dict(prior=float("nan")), "prior"), (dict(prior="a"), "prior"), (dict(prior=True), "prior"),
                     (dict(refine=17), "refine"), (dict(refine=-1), "refine"), (dict(refine=1.5), "refine"), (dict(refine=True), "refine")):
        with pytest.raises(ValueError, match=word):
            triangulate_views(**dict(base, **kw))
    for kw in (dict(), dict(valid=torch.ones(3, 6, dtype=torch.uint8), root_ok=ok, kp_weight=w, distort=False, sigma=0.05, prior=0.01, refine=0),
               dict(cameras=[[cam, None, cam]])):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            triangulate_views(**dict(base, **kw))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        triangulate_views(np.zeros((6, 17, 3), np.float32), root, kp, cams)

"""Fitting one skeleton to a fused take's keypoints, without a device: the float64 statement of mp_lift_fit_skeleton's rule (lift_skeleton_ref.py)
held against central differences, against an independent dense assembly and numpy's solve, and against every rule of the fallbacks; the margins
of the scenes the device test compares; the recovery claims on the committed seed; and what the new entry point needs declared around it."""
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

import lift_skeleton_ref as ref
import lift_triangulate_ref as tri

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hpe"))
INF = float("inf")


def _take(V=4, J=17, n=3, seed=700, sigma=0.05, prior=1e-4, distort=True, parents=None, weights=False):
    """(Take, scene) of a noisy scene of n frames"""
    sc = ref.body_scene(V, J, [n], seed=seed, parents=parents)
    w = tri.weight_table(V, n, J, seed) + np.float32(0.1) if weights else None
    return ref.make_take(sc["start"], sc["kp"], sc["quat"][0], sc["trans"][0], sc["intr"][0], sc["lengths"][0], sc["parents"], kp_weight=w,
                         distort=distort, sigma=sigma, prior=prior), sc


def _one(tk, f):
    """the Take of frame f alone"""
    return ref.Take(tk.start[f:f + 1], tk.kp[:, f:f + 1], None if tk.w is None else tk.w[:, f:f + 1], tk.seen[:, f:f + 1], tk.R, tk.T, tk.intr, tk.L,
                    tk.parents, tk.distort, 1.0, 0.0)


@pytest.mark.parametrize("distort", [False, True])
@pytest.mark.parametrize("sigma,prior", [(INF, 0.0), (0.05, 1e-4), (0.004, 0.02)])
def test_jacobians_and_gradient_against_central_differences(distort, sigma, prior):
    """The assembly Jacobian - every joint with respect to the root and to (alpha_b, beta_b) of d_b -> unit(d_b + alpha e1 + beta e2) - and the
    right side against central differences: dp_j/dx against the dense 3 x U Jacobian, and the gradient of F against 2 rhs (rho' = omega, so
    dF/dx = 2 sum J^T g, the pull included).  h = 1e-6: truncation O(h^2) of derivatives of order 1, rounding 1e-16 / h = 1e-10; 1e-7 relative to
    the largest entry bounds both with room.  (The projection's own Jacobian is lift_triangulate_ref's, held against differences there; the
    gradient here goes through it once more.)"""
    tk, _ = _take(sigma=sigma, prior=prior, distort=distort, weights=True)
    tk.sigma2, tk.prior = np.float64(sigma) * np.float64(sigma), np.float64(prior)
    r, d, _, _ = ref.start_directions(tk)
    e = ref.evaluate(tk, r, d)
    _, _, _, e1, e2, H, rhs = ref.step_system(tk, e, d)
    f, h = 1, 1e-6
    one = _one(tk, f)
    one.sigma2, one.prior = tk.sigma2, tk.prior
    state = (r[f:f + 1], d[f:f + 1], e1[f:f + 1], e2[f:f + 1])
    Jm = ref.dense_jacobians(tk, e1, e2, f)
    num, grad = np.zeros((tk.J, 3, tk.U)), np.zeros(tk.U)
    for u in range(tk.U):
        x = np.zeros(tk.U); x[u] = h
        rp, dp = ref.moved(one, *state, x)
        rm, dm = ref.moved(one, *state, -x)
        ep, em = ref.evaluate(one, rp, dp, jac=False), ref.evaluate(one, rm, dm, jac=False)
        num[:, :, u] = (ep["p"][0] - em["p"][0]) / (2 * h)
        grad[u] = (ep["F"][0] - em["F"][0]) / (2 * h)
    assert np.abs(Jm - num).max() <= 1e-7 * np.abs(Jm).max()
    print("rhs", rhs[f][:5], "dF/dx / 2", grad[:5] / 2)
    assert np.abs(rhs[f] - grad / 2).max() <= 1e-7 * max(np.abs(rhs[f]).max(), 1e-3)


@pytest.mark.parametrize("V,J,parents", [(4, 17, None), (2, 17, None), (3, 5, None), (4, 2, None), (4, 32, ref.chain(32)), (4, 32, ref.star(32)), (1, 17, None)])
def test_tree_assembly_and_cholesky_against_the_dense_path(V, J, parents):
    """H and the right side assembled from the subtree sums against sum_j J_j^T S_j J_j with the dense 3 x U Jacobians, to 1e-12 relative; the
    Cholesky solve against numpy.linalg.solve of the dense system, to 1e-9 relative (the condition numbers stay below 1e7: printed)"""
    tk, _ = _take(V=V, J=J, seed=710 + V + J, parents=parents, weights=V > 2, prior=1e-4 if V > 1 else 0.01)
    r, d, _, _ = ref.start_directions(tk)
    e = ref.evaluate(tk, r, d)
    delta, passed, worst, e1, e2, H, rhs = ref.step_system(tk, e, d)
    assert passed.all()
    anc = ref.ancestors(tk.parents)
    for f in range(tk.n):
        Hd, bd, dd = ref.dense_system(tk, e, d, f)
        low = np.tril(H[f])
        assert np.array_equal(H[f], low)                                  # nothing above the diagonal
        assert np.abs(low + np.tril(H[f], -1).T - Hd).max() <= 1e-12 * np.abs(Hd).max()
        assert np.abs(rhs[f] - bd).max() <= 1e-12 * np.abs(bd).max()
        cond = np.linalg.cond(Hd)
        print(f"V={V} J={J} frame {f}: U={tk.U}, cond {cond:.3e}, smallest pivot ratio {worst[f]:.3e}")
        assert cond < 1e7 and np.abs(delta[f] - dd).max() <= 1e-9 * np.abs(dd).max()
        for a in range(J - 1):                                            # a pair of bones on different branches has an exactly zero block
            for b in range(a + 1, J - 1):
                if a not in anc[b]:
                    assert not H[f, 3 + 2 * b:5 + 2 * b, 3 + 2 * a:5 + 2 * a].any() and np.abs(Hd[3 + 2 * b:5 + 2 * b, 3 + 2 * a:5 + 2 * a]).max() <= 1e-12 * np.abs(Hd).max()
    if parents == ref.star(32):
        assert all(a == {b} for b, a in enumerate(anc))
    if parents == ref.chain(32):
        assert anc[30] == set(range(31)) and tk.U == 65


def test_cholesky_solve_alone():
    g = np.random.default_rng(720)
    for U in (1, 5, 35, 65):
        A = g.standard_normal((2, U, U + 3))
        H = A @ A.transpose(0, 2, 1)
        b = g.standard_normal((2, U))
        x, passed, worst = ref.cholesky_solve(np.tril(H), b)
        assert passed.all() and (worst > 0).all()
        for f in range(2):
            assert np.abs(x[f] - np.linalg.solve(H[f], b[f])).max() <= 1e-9 * np.abs(x[f]).max()
    H = np.tril(np.array([[[1.0, 1.0], [1.0, 1.0]], [[1.0, 0.0], [0.0, 1.0]]]))      # a singular system beside a regular one: decided per frame
    x, passed, worst = ref.cholesky_solve(H, np.ones((2, 2)))
    assert passed.tolist() == [False, True] and worst[0] == 0.0 and np.array_equal(x[1], [1.0, 1.0])


def test_sigma_inf_is_exactly_unweighted_and_prior_zero_drops_the_pull():
    tk, sc = _take(sigma=INF, prior=0.0, weights=True)
    r, d, _, _ = ref.start_directions(tk)
    e = ref.evaluate(tk, r, d)
    big = ref.make_take(sc["start"], sc["kp"], sc["quat"][0], sc["trans"][0], sc["intr"][0], sc["lengths"][0], sc["parents"], kp_weight=tk.w.astype(np.float32),
                        sigma=1e30, prior=0.0)                              # sigma^2 = 1e60 is finite, and 1 + e / 1e60 is 1 all the same
    e2 = ref.evaluate(big, r, d)
    assert all(np.array_equal(e[k], e2[k]) for k in ("F", "E", "W", "S", "g"))
    # the same sums with no robust factor written at all, for one joint of one frame
    f, j = 1, 5
    obs = tri.observations(sc["kp"], tk.w.astype(np.float32), None, [tk.R], tk.T[None], tk.intr[None], 0, f, j)
    F, H, g = np.float64(0), [np.float64(0)] * 6, [np.float64(0)] * 3
    for o in obs:
        (du, dv), (r0, r1), _, _ = tri.residual_jac(o, tuple(e["p"][f, j]), True)
        F += o.w * (du * du + dv * dv)
        tri.normal_add(H, g, o.w, du, dv, r0, r1)
    assert list(e["S"][f, j]) == H and list(e["g"][f, j]) == g            # bit for bit: per joint the evaluation is lift_triangulate_ref's
    moved = ref.make_take(sc["start"] + np.float32(0.5), sc["kp"], sc["quat"][0], sc["trans"][0], sc["intr"][0], sc["lengths"][0], sc["parents"],
                          kp_weight=tk.w.astype(np.float32), sigma=INF, prior=0.0)
    e3 = ref.evaluate(moved, r, d)
    assert all(np.array_equal(e[k], e3[k]) for k in ("F", "S", "g"))      # prior = 0: the start appears nowhere in the evaluation
    pulled = ref.make_take(sc["start"], sc["kp"], sc["quat"][0], sc["trans"][0], sc["intr"][0], sc["lengths"][0], sc["parents"], kp_weight=tk.w.astype(np.float32),
                           sigma=INF, prior=0.01)
    e4 = ref.evaluate(pulled, r, d)
    assert (e4["F"] > e["F"]).all() and np.array_equal(e4["S"][..., 0], e["S"][..., 0] + np.float64(np.float32(0.01))) and np.array_equal(e4["S"][..., 1], e["S"][..., 1])


def test_every_rule_of_the_fallbacks():
    inp, trace = ref.constructed(), []
    got = ref.fit(trace=trace, **inp)
    rigid = ref.rigid(inp["start"], inp["lengths"][0], inp["parents"])
    assert got["ok"].tolist() == [1, 1, 0, 0, 3, 2, 3] and got["written"].all()
    tk = ref.make_take(inp["start"], inp["kp"], inp["quat"][0], inp["trans"][0], inp["intr"][0], inp["lengths"][0], inp["parents"])
    with np.errstate(all="ignore"):
        _, d, own, _ = ref.start_directions(tk)
    f = ref.ZERO_ROOT_BONE                                                # joint 1 on the root: bone 0 takes (0, 0, 1), bit 1 cleared, fitted all the same
    assert np.array_equal(d[f, 0], [0.0, 0.0, 1.0]) and not own[f] and got["steps"][f] == 3
    f = ref.ZERO_DEEP_BONE                                                # joint 3 on joint 2: bone 2 takes bone 1's direction
    assert np.array_equal(d[f, 2], d[f, 1]) and not own[f] and got["steps"][f] == 3
    for f in (ref.NAN_START, ref.NOT_OK):                                 # rule 0: not fitted
        assert not got["pose"][f].any() and not got["err"][f].any() and got["steps"][f] == 0
    f = ref.NO_OBS                                                        # no observation, prior 0: H = 0, the first pivot fails, the rigid start is the result
    assert got["steps"][f] == 0 and np.array_equal(got["pose"][f], rigid[f]) and not got["err"][f].any()
    f = ref.BEHIND                                                        # rule 9: a start behind a camera has no result; bit 1 keeps what step 1 found
    assert not got["pose"][f].any() and not got["err"][f].any() and got["steps"][f] == 0 and got["ok"][f] == 2
    assert got["steps"][ref.PLAIN] == 3 and (got["err"][ref.PLAIN] > 0).all() and got["err"][ref.PLAIN, 1] < got["err"][ref.PLAIN, 0]
    pulled = ref.fit(**ref.constructed(prior=0.01))                       # with a pull the frame without observations is solvable: steps that move nothing
    assert pulled["steps"][ref.NO_OBS] == 3 and np.abs(pulled["pose"][ref.NO_OBS] - rigid[ref.NO_OBS]).max() < 0.05
    assert pulled["ok"].tolist() == got["ok"].tolist()
    bad = ref.fit(**ref.bad_lengths())                                    # a non-positive length: its take is not fitted, the other is
    assert not bad["ok"][:3].any() and not bad["pose"][:3].any() and (bad["ok"][3:] == 3).all()
    for spoil in (np.nan, np.inf, -0.1):
        inp2 = ref.bad_lengths()
        inp2["lengths"][0, 2] = spoil
        assert not ref.fit(**inp2)["ok"][:3].any()
    sc = ref.body_scene(2, 5, [6], seed=623)                              # a frame no take holds is not written
    got = ref.fit(**ref.inputs(sc, take_offset=[1, 4]))
    assert got["written"].tolist() == [False, True, True, True, False, False] and not got["ok"][[0, 4, 5]].any() and (got["ok"][1:4] == 3).all()
    # a refused step: from a far start under a hard robust scale the undamped step raises the cost and the state stays
    sc = ref.body_scene(2, 17, [4], seed=730, pose_noise=0.25)
    trace = []
    got = ref.fit(trace=trace, **ref.inputs(sc, sigma=0.001, prior=0.0, iters=5))
    print("a far start under sigma = 0.001: steps", got["steps"])
    assert (got["ok"] & 1).all() and (got["steps"] < 5).any()


def test_refine_zero_is_the_rigid_reassembly():
    for tag, inp, want, _ in ref.cases():
        if "iters=0" not in tag:
            continue
        for t in range(len(inp["take_offset"]) - 1):
            sl = slice(int(inp["take_offset"][t]), int(inp["take_offset"][t + 1]))
            rigid = ref.rigid(inp["start"][sl], inp["lengths"][t], inp["parents"])
            assert np.array_equal(want["pose"][sl], rigid) and not want["steps"][sl].any()      # mp_lift_rigid's rule in fp64, bit for bit
            assert np.array_equal(want["err"][sl, 0], want["err"][sl, 1])


def test_every_compared_scene_is_far_from_every_threshold():
    """what the device test relies on: every decision of every scene it compares with the statement is at least MARGIN_MIN of its slack from its
    threshold, so that rounding differences far below a float32 store cannot flip one"""
    for tag, _, want, trace in ref.cases():
        assert ref.margin(trace) >= ref.MARGIN_MIN, (tag, ref.margin(trace))
        assert want["written"].all()
    tags = " | ".join(c[0] for c in ref.cases())
    for word in ("F=1 V=4 J=17", "F=5 V=4", "F=65 V=2", "F=257 V=4 J=2", "V=3 J=5", "V=1 J=17", "J=32 chain", "J=32 star", "three takes", "iters=0", "iters=1",
                 "iters=16", "pinhole", "prior 0.01", "prior 0", "sigma=0.004", "view 2 missing", "weights with zeros"):
        assert word in tags, word
    noisy = ref.recovery(4, 0.002)
    for inp in (ref.constructed(), ref.constructed(0.01), ref.bad_lengths(), ref.inputs(noisy, start=ref.triangulated_start(noisy)),
                ref.inputs(ref.body_scene(2, 5, [6], seed=623), take_offset=[1, 4]), ref.inputs(ref.body_scene(3, 5, [6], seed=624))):
        trace = []
        ref.fit(trace=trace, **inp)
        assert ref.margin(trace) >= ref.MARGIN_MIN
    gaps = [c for c in ref.cases() if "gaps" in c[0]]                     # the cases with gaps hold frames that are not fitted
    assert gaps and all(set(np.unique(c[2]["ok"])) == {0, 3} for c in gaps)
    assert all(c[2]["steps"].max() == 16 for c in ref.cases() if "iters=16" in c[0])


def test_the_results_bones_are_the_table():
    for tag, inp, want, _ in ref.cases():
        off = inp["take_offset"]
        for t in range(len(off) - 1):
            sl = slice(int(off[t]), int(off[t + 1]))
            done = (want["ok"][sl] & 1) != 0
            bones = ref.bone_lengths(want["pose"][sl][done].astype(np.float32), inp["parents"])
            table = np.broadcast_to(inp["lengths"], (len(off) - 1, len(inp["parents"]) - 1))[t].astype(np.float64)
            # two float32 stores of coordinates below 8 m (half an ulp, 2^-22, each), three coordinates: sqrt(3) 2^-21
            assert np.abs(want["pose"]).max() < 8 and np.abs(bones - table).max() <= math.sqrt(3.0) * 2.0 ** -21, tag


def test_recovery_on_the_committed_seed():
    """the claims, re-measured with the statement (lift_skeleton_ref.py has the figures; every bound is twice the value measured)"""
    sc = ref.recovery(4, 0.0)
    got = ref.fit(**ref.inputs(sc))
    worst = ref.errors(got["pose"], sc).max()
    print(f"claim 1: 4 views, noise-free, {ref.DEFAULT_STEPS} steps from a start {ref.errors(sc['start'], sc).mean():.4f} m off: max {worst:.3e} m "
          f"(mean {ref.errors(got['pose'], sc).mean():.3e}), steps {np.bincount(got['steps'])}")
    assert (got["ok"] == 3).all() and worst <= ref.RECOVERY_4V
    for V in (4, 2):
        noisy = ref.recovery(V, 0.002)
        start = ref.triangulated_start(noisy)
        got = ref.fit(**ref.inputs(noisy, start=start))
        mean, before = ref.errors(got["pose"], noisy).mean(), ref.errors(start, noisy).mean()
        again = ref.errors(ref.rigid(start, noisy["lengths"][0], noisy["parents"]), noisy).mean()
        print(f"claim 2: {V} views, noise 0.002: the fit {mean:.5f} m, the triangulated start {before:.5f} m, re-assembled bone by bone {again:.5f} m")
        assert (got["ok"] == 3).all() and mean < before and mean < again
        if V == 4:
            table = ref.median_table(start, noisy["parents"])
            miss = np.abs(table - noisy["lengths"][0]).max()
            med = ref.fit(**ref.inputs(noisy, start=start, lengths=table[None]))
            print(f"claim 4 (recorded): the median table of that start misses the true table by at most {miss:.5f} m; the fit with it: "
                  f"{ref.errors(med['pose'], noisy).mean():.5f} m")
    one = ref.recovery(1, 0.002)
    got = ref.fit(**ref.inputs(one))
    mean, before = ref.errors(got["pose"], one).mean(), ref.errors(one["start"], one).mean()
    print(f"claim 3: 1 view, the default pull, noise 0.002: the fit {mean:.5f} m against the lifted start's {before:.5f} m, steps {np.bincount(got['steps'])}")
    assert (got["ok"] == 3).all() and mean < before


def test_new_abi_symbol_is_declared_everywhere():
    from manipose_amd import _lib, lifting, lift_views
    import manipose_amd
    header = open(_lib.HEADER_PATH).read()
    assert "mp_lift_fit_skeleton" in _lib.declared_symbols() and len(_lib._SIGNATURES["mp_lift_fit_skeleton"][1]) == 24
    assert _lib.ABI_VERSION == 8 and int(re.search(r"#define MP_ABI_VERSION (\d+)", header).group(1)) == 8        # purely additive
    assert int(re.search(r"#define MP_LIFT_REFINE_MAXITERS (\d+)", header).group(1)) == lifting.REFINE_MAXITERS == ref.MAXITERS == 16
    assert manipose_amd.fit_skeleton_views is lifting.fit_skeleton_views and "fit_skeleton_views" in lifting.__all__
    assert lifting.ViewSkeleton._fields == ("pose", "err", "ok", "steps", "lengths")
    assert (lift_views.SKELETON_SIGMA, lift_views.SKELETON_PRIOR, lift_views.SKELETON_STEPS) == (INF, ref.DEFAULT_PRIOR, ref.DEFAULT_STEPS)
    source = open(os.path.join(ROOT, "manipose_amd", "csrc", "lift_skeleton.hip")).read()
    assert source.index("#pragma clang fp contract(off)") < source.index('#include "lift_geom.h"')
    assert "lib.mp_lift_fit_skeleton.argtypes" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ("README.md", "DESIGN.md"):
        text = open(os.path.join(ROOT, name)).read()
        assert "mp_lift_fit_skeleton" in text and "lift.fuse_skeleton" in text
    config = open(os.path.join(ROOT, "hpe", "conf", "config.yaml")).read()
    assert all(k in config for k in ("fuse_skeleton:", "fuse_skeleton_steps:", "fuse_skeleton_sigma:", "fuse_skeleton_prior:"))
    assert "--skeleton" in open(os.path.join(ROOT, "tools", "lift_bench.py")).read()
    if os.path.exists(_lib.LIB_PATH):
        assert hasattr(_lib.load(), "mp_lift_fit_skeleton")


def test_config_keys_parse_and_a_skeleton_without_a_fusion_fails():
    from _entry import LIFT_SUFFIXES, lift_fuse_skeleton_options, load_config, run
    cfg = load_config([])
    assert cfg.lift.fuse_skeleton is False and lift_fuse_skeleton_options(cfg) == (False, 3, INF, 0.0001)
    on = ["run.lift=true", "lift.fuse=true"]
    assert lift_fuse_skeleton_options(load_config(on)) == (False, 3, INF, 0.0001)
    assert lift_fuse_skeleton_options(load_config(on + ["lift.fuse_skeleton=true"])) == (True, 3, INF, 0.0001)
    assert lift_fuse_skeleton_options(load_config(on + ["lift.fuse_skeleton=true", "lift.fuse_skeleton_steps=16", "lift.fuse_skeleton_sigma=0.05",
                                                        "lift.fuse_skeleton_prior=0"])) == (True, 16, 0.05, 0.0)
    assert lift_fuse_skeleton_options(load_config(on + ["lift.fuse_skeleton=true", "lift.fuse_skeleton_sigma=inf"]))[2] == INF
    with pytest.raises(SystemExit):
        load_config(["lift.fuse_skeletons=true"])
    sk = on + ["lift.fuse_skeleton=true"]
    for argv, word in ((["lift.fuse_skeleton=true"], "set lift.fuse=true"), (["run.lift=true", "lift.fuse_skeleton=true"], "set lift.fuse=true"),
                       (on + ["lift.fuse_skeleton_steps=2"], "describe the skeleton fit of a fused take: set lift.fuse_skeleton=true"),
                       (on + ["lift.fuse_skeleton_sigma=0.1"], "set lift.fuse_skeleton=true"), (on + ["lift.fuse_skeleton_prior=0.1"], "set lift.fuse_skeleton=true"),
                       (on + ["lift.fuse_skeleton=1"], "true or false"), (sk + ["lift.fuse_skeleton_steps=17"], "0..16"), (sk + ["lift.fuse_skeleton_steps=-1"], "0..16"),
                       (sk + ["lift.fuse_skeleton_steps=1.5"], "0..16"), (sk + ["lift.fuse_skeleton_steps=true"], "0..16"),
                       (sk + ["lift.fuse_skeleton_sigma=0"], "> 0"), (sk + ["lift.fuse_skeleton_sigma=-1"], "> 0"), (sk + ["lift.fuse_skeleton_sigma=abc"], "is a number"),
                       (sk + ["lift.fuse_skeleton_prior=-0.1"], "finite and >= 0"), (sk + ["lift.fuse_skeleton_prior=inf"], "finite and >= 0"),
                       (sk + ["lift.fuse_skeleton_prior=true"], "is a number")):
        with pytest.raises(ValueError, match=word):
            run(["run.train=false", "run.test=false"] + argv)                    # (a run that got further would need a device)
    assert all(s in LIFT_SUFFIXES for s in ("__skel", "__skel_bones", "__skel_err", "__skel_ok", "__skel_steps", "__skel_quat", "__skel_quat_ok"))


def test_argument_errors_are_value_errors_before_any_device_work():
    """The calls are given CPU tensors: had the arguments been accepted, they would have ended in the RuntimeError that refuses them ("no CPU
    fallback"), which is what the valid calls at the end do."""
    import types
    from manipose_amd import fit_skeleton_views
    start, kp = torch.zeros(6, 17, 3), torch.zeros(3, 6, 17, 2)
    cam = np.concatenate([np.ones(9), [1, 0, 0, 0], np.zeros(3)])
    cams, ok, w = [[cam, cam, cam]], torch.ones(6, dtype=torch.uint8), torch.ones(3, 6, 17)
    base = dict(start=start, keypoints_2d=kp, cameras=cams)
    five = types.SimpleNamespace(parents=[-1, 0, 1, 2, 0])
    for kw, word in ((dict(start=torch.zeros(6, 17, 2)), "pose must be"), (dict(start=start.double()), "pose must be"), (dict(start=torch.zeros(6, 33, 3)), "pose must be"),
                     (dict(keypoints_2d=torch.zeros(5, 6, 17, 2)), "keypoints_2d"), (dict(keypoints_2d=torch.zeros(3, 6, 16, 2)), "keypoints_2d"),
                     (dict(valid=torch.ones(2, 6, dtype=torch.uint8)), "valid must be"), (dict(start_ok=torch.ones(5, dtype=torch.uint8)), "start_ok must be"),
                     (dict(start_ok=ok.bool()), "start_ok must be"), (dict(kp_weight=torch.ones(3, 6, 16)), "kp_weight must be"),
                     (dict(kp_weight=w.double()), "kp_weight must be"), (dict(kp_weight=np.ones((3, 6, 17), np.float32)), "kp_weight must be"),
                     (dict(lengths=np.ones(15)), "lengths must be"), (dict(lengths=np.ones((2, 16))), "lengths must be"), (dict(lengths=np.full(16, np.nan)), "lengths must be finite"),
                     (dict(skeleton=five), "17 joints, but the skeleton has 5"), (dict(skeleton=types.SimpleNamespace(parents=[-1] + [3] * 16)), "parents must precede"),
                     (dict(cameras=[[cam, cam]]), "3 views"), (dict(cameras=[[cam, np.concatenate([np.ones(9), np.zeros(7)]), cam]]), "zero quaternion"),
                     (dict(sigma=0), "sigma"), (dict(sigma=-1.0), "sigma"), (dict(sigma=float("nan")), "sigma"), (dict(sigma="a"), "sigma"), (dict(sigma=True), "sigma"),
                     (dict(prior=-0.1), "prior"), (dict(prior=INF), "prior"), (dict(prior=float("nan")), "prior"), (dict(prior="a"), "prior"), (dict(prior=True), "prior"),
                     (dict(refine=17), "refine"), (dict(refine=-1), "refine"), (dict(refine=1.5), "refine"), (dict(refine=True), "refine")):
        with pytest.raises(ValueError, match=word):
            fit_skeleton_views(**dict(base, **kw))
    for kw in (dict(), dict(lengths=np.ones(16), valid=torch.ones(3, 6, dtype=torch.uint8), start_ok=ok, kp_weight=w, distort=False, sigma=0.05, prior=0.0, refine=0),
               dict(lengths=torch.ones(1, 16)), dict(cameras=[[cam, None, cam]])):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fit_skeleton_views(**dict(base, **kw))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fit_skeleton_views(np.zeros((6, 17, 3), np.float32), kp, cams)

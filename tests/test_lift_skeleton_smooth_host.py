"""Fitting a fused take's skeleton along time, without a device: the float64 statement of mp_lift_fit_skeleton_smooth's rule
(lift_skeleton_smooth_ref.py) held against the total cost summed directly over its terms, against central differences of that cost, and against
lift_skeleton_ref where the two must agree; the margins of the scenes the device test compares; the recovery claims on the committed seed; and
what the new entry point needs declared around it."""
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

import lift_bundle_ref as bundle
import lift_skeleton_ref as base
import lift_skeleton_smooth_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hpe"))
INF = float("inf")
KEYS = ("pose", "err", "ok", "steps", "moves")


def test_the_evaluation_with_the_one_pull_is_lift_skeleton_refs():
    for prior, sigma, distort in ((1e-4, INF, True), (0.0, 0.05, False), (0.02, 0.004, True)):
        sc = ref.motion_scene(3, 17, [4], seed=840)
        tk = base.make_take(sc["start"], sc["kp"], sc["quat"][0], sc["trans"][0], sc["intr"][0], sc["lengths"][0], sc["parents"], distort=distort, sigma=sigma, prior=prior)
        r, d, _, _ = base.start_directions(tk)
        for jac in (True, False):
            a, b = base.evaluate(tk, r, d, jac=jac), ref.evaluate(tk, r, d, ref.start_pull(tk), jac=jac)
            assert all(np.array_equal(a[k], b[k]) for k in a), (prior, jac)
        assert len(ref.start_pull(tk)) == (prior > 0)


def _usable_patterns():
    """(n, usable) of takes of 3, 4, 5 and 7 frames, whole and with an unusable frame inside"""
    out = []
    for n in (3, 4, 5, 7):
        out.append(np.ones(n, bool))
        for hole in range(n):
            u = np.ones(n, bool)
            u[hole] = False
            out.append(u)
    return out


def test_the_conditional_form_is_the_total_cost():
    """With the other frames held, the terms of the smoothness cost that hold frame t are W_t sum_j |p_j - q_j|^2 plus a constant: the change of
    the cost summed directly over its terms equals the change of the conditional form to 1e-12 relative, for every frame of every pattern; and
    W_t takes each of 0, 1, 4, 5, 6 somewhere"""
    g = np.random.default_rng(841)
    met, worst = set(), 0.0
    for usable in _usable_patterns():
        n = usable.size
        a, b, c, W = ref.stencil(usable)
        P = g.standard_normal((n, 5, 3))
        P[~usable] = np.nan                                                # an unusable frame's positions are never read
        for t in range(n):
            met.add(int(W[t]))
            if not usable[t]:
                assert W[t] == 0
                continue
            moved = P.copy()
            moved[t] = g.standard_normal((5, 3))
            direct = ref.prior_terms(moved, usable) - ref.prior_terms(P, usable)
            if W[t] == 0:
                assert direct == 0.0
                continue
            q = ref.target(P, np.array([t]), a, b, c)[0]
            cond = W[t] * (((moved[t] - q) ** 2).sum() - ((P[t] - q) ** 2).sum())
            worst = max(worst, abs(direct - cond) / abs(direct))
            assert abs(direct - cond) <= 1e-12 * abs(direct), (usable, t, direct, cond)
    print(f"W_t met: {sorted(met)}; the largest relative difference {worst:.2e}")
    assert met == {0, 1, 4, 5, 6}
    # the full stencil's expression, and the two one-sided ones
    P = g.standard_normal((5, 2, 3))
    a, b, c, W = ref.stencil(np.ones(5, bool))
    q = ref.target(P, np.arange(5), a, b, c)
    assert W.tolist() == [1, 5, 6, 5, 1] and np.array_equal(q[2], (4.0 * (P[1] + P[3]) - (P[0] + P[4])) / 6.0)
    assert np.array_equal(q[0], 2.0 * P[1] - P[2]) and np.array_equal(q[4], 2.0 * P[3] - P[2])
    assert np.array_equal(q[1], ((2.0 * P[0] + 4.0 * P[2]) - P[3]) / 5.0)
    a, b, c, W = ref.stencil(np.array([True, True, True, False, True]))
    assert W.tolist() == [1, 4, 1, 0, 0] and np.array_equal(ref.target(P, np.array([1]), a, b, c)[0], (2.0 * P[0] + 2.0 * P[2]) / 4.0)


def test_the_total_cost_never_rises_by_more_than_the_slack():
    """after every colour of every sweep the take's cost, summed directly, is at most (1 + 1e-6) times what it was (a colour's frames share no
    term, and a frame's conditional cost is at most its share of the total), up to the rounding of the sum itself"""
    for V, smooth, sigma in ((4, 0.1, INF), (2, 10.0, 0.05), (1, 0.1, INF)):
        sc = ref.motion_scene(V, 17, [7, 5], seed=842 + V)
        start, ok = ref.spoiled(sc, dead=[3], nan=[])                       # the take of 7 with a hole in the middle: W = 1 4 1 0 1 4 1
        costs = {}

        def watch(st, sweep, colour):
            costs.setdefault(id(st), []).append(st.cost(smooth))

        got = ref.fit(**ref.inputs(sc, start=start, start_ok=ok, smooth=smooth, sweeps=6, sigma=sigma, prior=0.01 if V == 1 else 1e-4, watch=watch))
        first = [st.cost(smooth) for st in ref.fit(**ref.inputs(sc, start=start, start_ok=ok, sweeps=0, sigma=sigma, prior=0.01 if V == 1 else 1e-4))["takes"]]
        for st, c0 in zip(got["takes"], first):
            seq = [c0] + costs[id(st)]
            print(f"V={V} smooth={smooth}: a take's cost {seq[0]:.6e} -> {seq[3]:.6e} (1 sweep) -> {seq[-1]:.6e} (6 sweeps)")
            assert all(b <= (1.0 + ref.COST_SLACK) * a + 1e-12 * a for a, b in zip(seq[:-1], seq[1:])) and seq[-1] < seq[0]
        assert got["moves"].any()


def test_smooth_zero_and_sweeps_zero_are_lift_skeleton_refs_fit():
    seen = 0
    for tag, inp, want, _ in ref.cases():
        if "three takes" not in tag and "chain" not in tag:
            continue
        plain = base.fit(**{k: v for k, v in inp.items() if k not in ("smooth", "sweeps")})
        for over in (dict(smooth=0.0), dict(sweeps=0), dict(smooth=1e-50)):      # (1e-50 is 0 as a float32)
            got = ref.fit(**dict(inp, **over))
            assert all(np.array_equal(got[k], plain[k]) for k in ("pose", "ok", "steps", "written")) and np.array_equal(got["err"][:, :2], plain["err"]), (tag, over)
            assert np.array_equal(got["err"][:, 2], got["err"][:, 1]) and not got["moves"].any()
        assert all(np.array_equal(want[k], plain[k]) for k in ("ok", "steps")) and np.array_equal(want["err"][:, :2], plain["err"])      # stage A's outputs stay
        seen += 1
    assert seen >= 10


def test_short_takes_and_takes_without_three_usable_frames_in_a_row_are_stage_a():
    sc = ref.motion_scene(4, 17, [1, 2, 8], seed=845)
    start, ok = ref.spoiled(sc, dead=[5, 8], nan=[10])                      # the take of 8: usable 1 1 0 1 1 0 1 0 - never three in a row
    inp = ref.inputs(sc, start=start, start_ok=ok, sweeps=3)
    got, plain = ref.fit(**inp), ref.fit(**dict(inp, sweeps=0))
    assert got["ok"].tolist() == [3, 3, 3, 3, 3, 0, 3, 3, 0, 3, 0]
    assert all(np.array_equal(got[k], plain[k]) for k in KEYS) and not got["moves"].any()
    assert all(not st.W.any() for st in got["takes"])
    three = ref.fit(**ref.inputs(ref.motion_scene(4, 17, [3], seed=846), sweeps=1))      # three frames: one term, W = (1, 4, 1)
    assert three["takes"][0].W.tolist() == [1, 4, 1] and three["moves"].tolist() == [1, 1, 1]


def _exact_take(V=2, J=5, n=7, seed=847):
    """a Take in float64 throughout - the kernel's float32 inputs would put 1e-7 of rounding into the keypoints: a body of constant directions
    whose root moves with constant velocity, keypoints the statement's own projection of it, the start the truth"""
    g = np.random.default_rng(seed)
    sc = ref.motion_scene(V, J, [n], seed=seed)
    tk = base.make_take(sc["start"], sc["kp"], sc["quat"][0], sc["trans"][0], sc["intr"][0], sc["lengths"][0], sc["parents"], prior=0.0)
    dirs = g.standard_normal((J - 1, 3))
    dirs /= np.linalg.norm(dirs, axis=-1, keepdims=True)
    r = np.array([0.1, -0.2, 0.9]) + np.arange(n)[:, None] * np.array([0.01, 0.005, 0.0])
    d = np.broadcast_to(dirs, (n, J - 1, 3)).copy()
    p = base.positions(tk, r, d)
    tk.start = p.copy()
    for v in range(V):
        w = p - tk.T[v]
        X, Y, Z = (w @ tk.R[v][:, i] for i in range(3))
        du, dv, _ = bundle.project_jac(X, Y, Z, np.zeros_like(X), np.zeros_like(X), tk.intr[v], tk.distort)
        tk.kp[v, :, :, 0], tk.kp[v, :, :, 1] = du, dv                      # the residual against a keypoint of 0 is the projection
    return tk, r, d, p


def test_a_body_in_uniform_motion_is_a_fixed_point():
    """constant velocity, constant directions, noise-free, started at the truth, prior 0: the second differences vanish and so does every frame's
    gradient; no visit's step reaches 1e-9 m"""
    tk, r, d, p = _exact_take()
    r0, d0, _, _ = base.start_directions(tk)
    assert np.abs(r0 - r).max() == 0 and np.abs(d0 - d).max() <= 1e-15
    st = ref.TakeState(tk, np.arange(tk.n), np.ones(tk.n, bool), r0.copy(), d0.copy(), base.positions(tk, r0, d0))
    largest = 0.0
    for sweep in range(3):
        for colour in range(3):
            T, moved, _, size = ref.sweep_take(st, 0.1, colour)
            largest = max(largest, float(size.max()))
    print(f"uniform motion: the largest step of 3 sweeps {largest:.2e} m, the positions moved by {np.abs(st.p - p).max():.2e} m")
    assert largest < 1e-9 and np.abs(st.p - p).max() < 1e-9


def _gradient(st, smooth, h=1e-6):
    """central differences of the take's total cost with respect to every unknown of every usable frame, in the tangent parametrisation around
    the state (lift_skeleton_ref.moved): (n, U)"""
    tk = st.tk
    e1, e2, _ = base.tangent_bases(tk, st.d)
    out = np.zeros((tk.n, tk.U))
    for t in np.flatnonzero(st.usable):
        one = ref.sub_take(tk, np.array([t]))
        for u in range(tk.U):
            side = []
            for sign in (1.0, -1.0):
                x = np.zeros(tk.U)
                x[u] = sign * h
                r2, d2 = base.moved(one, st.r[t:t + 1], st.d[t:t + 1], e1[t:t + 1], e2[t:t + 1], x)
                keep = st.r[t].copy(), st.d[t].copy(), st.p[t].copy()
                st.r[t], st.d[t], st.p[t] = r2[0], d2[0], base.positions(one, r2, d2)[0]
                side.append(st.cost(smooth))
                st.r[t], st.d[t], st.p[t] = keep
            out[t, u] = (side[0] - side[1]) / (2 * h)
    return out


def test_the_sweeps_reach_a_stationary_point_of_the_total_cost():
    """The sweeps solve the right problem: after STATIONARY's sweeps every central-difference derivative of the take's total cost - the frames'
    F plus smooth times the second differences, summed directly - is at most 1e-6 of the largest derivative at stage A's result.  h = 1e-6: the
    cost is about 1e-3 and rounds at 1e-19, so a difference quotient is good to 1e-13, six orders below the bound it is held to"""
    S = ref.STATIONARY
    sc = ref.motion_scene(S["V"], S["J"], list(S["lens"]), seed=S["seed"])
    inp = ref.inputs(sc, smooth=S["smooth"])
    before = ref.fit(**dict(inp, sweeps=0))["takes"][0]
    after = ref.fit(**dict(inp, sweeps=S["sweeps"]))
    g0, g1 = np.abs(_gradient(before, S["smooth"])).max(), np.abs(_gradient(after["takes"][0], S["smooth"])).max()
    print(f"the largest derivative of the total cost: {g0:.3e} at stage A's result, {g1:.3e} after {S['sweeps']} sweeps: ratio {g1 / g0:.2e} "
          f"(recorded: {ref.MEASURED_STATIONARY}); moves {after['moves']}")
    assert g1 <= 1e-6 * g0


def test_the_visits_of_one_colour_commute():
    for tag, inp, want, _ in ref.cases():
        if not ("start_ok" in tag or tag == "three takes" or tag.startswith("F=7 V=3")):
            continue
        for kw in (dict(reverse_colour=0), dict(reverse_colour=1), dict(reverse_colour=2), dict(order="forward"), dict(order="reverse")):
            got = ref.fit(**dict(inp, **kw))
            assert all(np.array_equal(got[k], want[k]) for k in KEYS), (tag, kw)


def test_recovery_on_the_committed_seed():
    """the claims, re-measured with the statement (lift_skeleton_smooth_ref.py has the figures; a bound on a mean is twice the value measured).
    Asserted outright at 4, 2 and 1 views with the default weight and sweeps: the smoothed fit's mean error and its mean second difference are
    below the per-frame fit's"""
    for V, record in ((4, ref.MEASURED_4V), (2, ref.MEASURED_2V)):
        sc, inp = ref.recovery(V), ref.recovery_inputs(V)
        got = ref.fit(**inp)
        plain = base.fit(**{k: v for k, v in inp.items()})
        err = (ref.errors(inp["start"], sc).mean(), ref.errors(plain["pose"], sc).mean(), ref.errors(got["pose"], sc).mean())
        sd = (ref.second_difference(plain["pose"]), ref.second_difference(got["pose"]), ref.second_difference(sc["truth"]))
        print(f"{V} views, noise 0.002, smooth {ref.DEFAULT_SMOOTH}, {ref.DEFAULT_SWEEPS} sweeps: the triangulated start {err[0]:.6f} m, the per-frame fit {err[1]:.6f} m, "
              f"the smoothed fit {err[2]:.6f} m; second difference {sd[0]:.6f} -> {sd[1]:.6f} m / frame^2 (the truth's {sd[2]:.6f}); moves {np.bincount(got['moves'])}")
        assert (got["ok"] == 3).all() and err[2] < err[1] and sd[1] < sd[0]
        assert err[2] <= 2 * record[0][2] and sd[1] <= 2 * record[1][1]
    sc, inp = ref.recovery(1), ref.recovery_inputs(1)
    got, more = ref.fit(**inp), ref.fit(**dict(inp, sweeps=4 * ref.DEFAULT_SWEEPS))
    plain = base.fit(**{k: v for k, v in inp.items()})
    err = (ref.errors(inp["start"], sc).mean(), ref.errors(plain["pose"], sc).mean(), ref.errors(got["pose"], sc).mean(), ref.errors(more["pose"], sc).mean())
    sd = (ref.second_difference(plain["pose"]), ref.second_difference(got["pose"]))
    print(f"1 view (still converging): the lifted start {err[0]:.6f} m, the per-frame fit {err[1]:.6f} m, {ref.DEFAULT_SWEEPS} sweeps {err[2]:.6f} m, "
          f"{4 * ref.DEFAULT_SWEEPS} sweeps {err[3]:.6f} m; second difference {sd[0]:.6f} -> {sd[1]:.6f} m / frame^2")
    assert (got["ok"] == 3).all() and err[2] < err[1] and sd[1] < sd[0]
    assert err[2] <= 2 * ref.MEASURED_1V[0][2] and err[3] <= 2 * ref.MEASURED_1V[0][3]


def test_every_compared_scene_is_far_from_every_threshold():
    """what the device test relies on: every decision of every scene it compares with the statement - stage A's and every visit's pivot, cost and
    depth decisions - is at least MARGIN_MIN of its slack from its threshold"""
    smallest = math.inf
    for tag, _, want, trace in ref.cases():
        assert ref.margin(trace) >= ref.MARGIN_MIN, (tag, ref.margin(trace))
        assert want["written"].all()
        smallest = min(smallest, ref.margin(trace))
    tags = " | ".join(c[0] for c in ref.cases())
    for word in ("F=1 V=4", "F=2 V=4", "F=3 V=4", "F=4 V=4", "F=5 V=4", "F=7 V=4", "F=65 V=2", "V=1 J=17", "V=3 J=5", "J=32 chain", "three takes", "sweeps=0", "sweeps=1",
                 "sweeps=2", "sweeps=5", "smooth=0", "smooth=10", "prior 0", "pinhole", "sigma 0.05", "start_ok 0 in the middle", "NaN at position 1",
                 "start_ok 0 at position 1", "NaN in the middle", "view 2 missing", "weights with zeros"):
        assert word in tags, word
    for inp in (ref.recovery_inputs(4), ref.inputs(ref.motion_scene(2, 5, [9], seed=823), take_offset=[1, 8], sweeps=2),
                ref.inputs(ref.motion_scene(3, 5, [6], seed=824), sweeps=2)):
        trace = []
        ref.fit(trace=trace, **inp)
        assert ref.margin(trace) >= ref.MARGIN_MIN
        smallest = min(smallest, ref.margin(trace))
    print(f"the smallest margin of a compared scene: {smallest:.4f} of its slack")
    kinds = {d["kind"] for c in ref.cases() for d in c[3]}
    assert kinds >= {"dir", "deep", "pivot", "cost"}
    gaps = [c for c in ref.cases() if "start_ok" in c[0]]                   # the cases with unusable frames: not fitted, never visited, never read
    assert len(gaps) == 2 and all(set(np.unique(c[2]["ok"])) == {0, 3} and not c[2]["moves"][c[2]["ok"] == 0].any() for c in gaps)
    assert any((c[2]["moves"] < c[1].get("sweeps", ref.DEFAULT_SWEEPS))[c[2]["ok"] == 3].any() for c in gaps)       # a usable frame with W = 0 beside a gap


def test_new_abi_symbols_are_declared_everywhere():
    from manipose_amd import _lib, lift_views, lifting
    header = open(_lib.HEADER_PATH).read()
    assert {"mp_lift_fit_skeleton_smooth", "mp_lift_fit_skeleton_smooth_scratch_bytes"} <= set(_lib.declared_symbols())
    res, args = _lib._SIGNATURES["mp_lift_fit_skeleton_smooth"]
    assert len(args) == 29 and args[:19] == _lib._SIGNATURES["mp_lift_fit_skeleton"][1][:19] and args[19:21] == [_lib.C.c_float, _lib.C.c_int]
    assert _lib._SIGNATURES["mp_lift_fit_skeleton_smooth_scratch_bytes"] == (_lib.C.c_int64, [_lib.C.c_int64, _lib.C.c_int])
    assert _lib.ABI_VERSION == 8 and int(re.search(r"#define MP_ABI_VERSION (\d+)", header).group(1)) == 8        # purely additive
    assert int(re.search(r"#define MP_LIFT_SKELETON_MAXSWEEPS (\d+)", header).group(1)) == lift_views.SKELETON_MAXSWEEPS == ref.MAXSWEEPS == 64
    assert (lift_views.SKELETON_SMOOTH, lift_views.SKELETON_SWEEPS) == (0.0, ref.DEFAULT_SWEEPS)
    assert lifting.ViewSkeletonSmooth._fields == ("pose", "err", "ok", "steps", "lengths", "moves") and lifting.ViewSkeleton._fields == lifting.ViewSkeletonSmooth._fields[:5]
    for word in ("q_j = ((c1- p_j(t-1) + c1+ p_j(t+1)) - (c2- p_j(t-2) + c2+ p_j(t+2))) / W_t", "q = (4 (p(t-1) + p(t+1)) - (p(t-2) + p(t+2))) / 6", "STAGE A", "STAGE B"):
        assert word in header, word
    for name in ("lift_skeleton.hip", "lift_skeleton_smooth.hip"):
        source = open(os.path.join(ROOT, "manipose_amd", "csrc", name)).read()
        assert source.index("#pragma clang fp contract(off)") < source.index('#include "lift_geom.h"') < source.index('#include "lift_skeleton.h"')
        assert "skel_step(" not in source.replace("skel_step(A, L, 0, 1)", "")      # the step is lift_skeleton.h's, not a copy
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "lib.mp_lift_fit_skeleton_smooth.argtypes" in text and "lib.mp_lift_fit_skeleton_smooth_scratch_bytes.argtypes" in text
    for name in ("README.md", "DESIGN.md"):
        text = open(os.path.join(ROOT, name)).read()
        assert "mp_lift_fit_skeleton_smooth" in text and "lift.fuse_skeleton_smooth" in text
    config = open(os.path.join(ROOT, "hpe", "conf", "config.yaml")).read()
    assert "fuse_skeleton_smooth: 0.0" in config and "fuse_skeleton_sweeps: 8" in config
    assert "--skeleton-smooth" in open(os.path.join(ROOT, "tools", "lift_bench.py")).read()
    if os.path.exists(_lib.LIB_PATH):
        assert hasattr(_lib.load(), "mp_lift_fit_skeleton_smooth") and hasattr(_lib.load(), "mp_lift_fit_skeleton_smooth_scratch_bytes")


def test_config_keys_parse_and_a_smoothing_without_a_skeleton_fails():
    from _entry import LIFT_SUFFIXES, lift_fuse_skeleton_options, lift_fuse_skeleton_smooth_options, load_config, run
    cfg = load_config([])
    assert cfg.lift.fuse_skeleton_smooth == 0.0 and cfg.lift.fuse_skeleton_sweeps == 8 and lift_fuse_skeleton_smooth_options(cfg) == (0.0, 8)
    sk = ["run.lift=true", "lift.fuse=true", "lift.fuse_skeleton=true"]
    assert lift_fuse_skeleton_smooth_options(load_config(sk)) == (0.0, 8) and lift_fuse_skeleton_options(load_config(sk)) == (True, 3, INF, 0.0001)
    assert lift_fuse_skeleton_smooth_options(load_config(sk + ["lift.fuse_skeleton_smooth=0.1"])) == (0.1, 8)
    assert lift_fuse_skeleton_smooth_options(load_config(sk + ["lift.fuse_skeleton_smooth=10", "lift.fuse_skeleton_sweeps=64"])) == (10.0, 64)
    assert lift_fuse_skeleton_smooth_options(load_config(sk + ["lift.fuse_skeleton_sweeps=0"])) == (0.0, 0)
    with pytest.raises(SystemExit):
        load_config(["lift.fuse_skeleton_smoothing=0.1"])
    on = ["run.lift=true", "lift.fuse=true"]
    for argv, word in ((["lift.fuse_skeleton_smooth=0.1"], "set lift.fuse_skeleton=true"), (on + ["lift.fuse_skeleton_smooth=0.1"], "set lift.fuse_skeleton=true"),
                       (on + ["lift.fuse_skeleton_sweeps=4"], "describe the skeleton fit of a fused take along time: set lift.fuse_skeleton=true"),
                       (sk + ["lift.fuse_skeleton_smooth=-0.1"], "finite and >= 0"), (sk + ["lift.fuse_skeleton_smooth=inf"], "finite and >= 0"),
                       (sk + ["lift.fuse_skeleton_smooth=nan"], "finite and >= 0"), (sk + ["lift.fuse_skeleton_smooth=true"], "is a number"),
                       (sk + ["lift.fuse_skeleton_smooth=abc"], "is a number"), (sk + ["lift.fuse_skeleton_sweeps=65"], "0..64"),
                       (sk + ["lift.fuse_skeleton_sweeps=-1"], "0..64"), (sk + ["lift.fuse_skeleton_sweeps=1.5"], "0..64"), (sk + ["lift.fuse_skeleton_sweeps=true"], "0..64")):
        with pytest.raises(ValueError, match=word):
            run(["run.train=false", "run.test=false"] + argv)                    # (a run that got further would need a device)
    assert "__skel_err_smooth" in LIFT_SUFFIXES and "__skel_moves" in LIFT_SUFFIXES


def test_argument_errors_are_value_errors_before_any_device_work():
    """The calls are given CPU tensors: had the arguments been accepted, they would have ended in the RuntimeError that refuses them ("no CPU
    fallback"), which is what the valid calls at the end do."""
    from manipose_amd import fit_skeleton_views
    start, kp = torch.zeros(6, 17, 3), torch.zeros(3, 6, 17, 2)
    cam = np.concatenate([np.ones(9), [1, 0, 0, 0], np.zeros(3)])
    base_kw = dict(start=start, keypoints_2d=kp, cameras=[[cam, cam, cam]])
    for kw, text in ((dict(smooth=-0.1), "smooth must be a finite number >= 0 (0: every frame fitted on its own), got -0.1"),
                     (dict(smooth=INF), "smooth must be a finite number >= 0 (0: every frame fitted on its own), got inf"),
                     (dict(smooth=float("nan")), "smooth must be a finite number >= 0"), (dict(smooth="a"), "smooth must be a finite number >= 0"),
                     (dict(smooth=True), "smooth must be a finite number >= 0"),
                     (dict(sweeps=65), "sweeps counts sweeps over a take's frames, an integer in 0..64 (0: every frame fitted on its own), got 65"),
                     (dict(sweeps=-1), "an integer in 0..64"), (dict(sweeps=1.5), "an integer in 0..64"), (dict(sweeps=True), "an integer in 0..64"),
                     (dict(smooth=0.1, sigma=0), "sigma must be"), (dict(smooth=0.1, refine=17), "refine counts")):
        with pytest.raises(ValueError, match=re.escape(text)):
            fit_skeleton_views(**dict(base_kw, **kw))
    for kw in (dict(smooth=0.1), dict(smooth=0.0, sweeps=0), dict(smooth=np.float32(10), sweeps=np.int64(64))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fit_skeleton_views(**dict(base_kw, **kw))

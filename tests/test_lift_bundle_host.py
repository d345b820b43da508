"""Bundle-adjusting a take's cameras, the parts that need no device: the float64 statement of mp_lift_bundle_views' rule (lift_bundle_ref.py)
against a dense solve of the full normal equations, its Jacobians against central differences, sigma = inf, what is copied through, the gauge
and the degenerate takes, the quaternion's sign rule, the recovery claims on committed seeds, the alternation the joint step replaces, the
decision margins of the device test's scenes, the option checks of hpe/_entry.py and the declarations."""
import os
import re
import sys

import numpy as np
import pytest
import torch

import lift_bundle_ref as ref
import lift_refine_ref as refine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hpe"))


def _take(sc, g=0, sigma=float("inf"), **kw):
    inp = ref.inputs(sc, **kw)
    sl = slice(int(sc["off"][g]), int(sc["off"][g + 1]))
    tk = ref.make_take(inp["pose"], inp["root"], inp["kp"], inp["quat"][g], inp.get("valid"), inp.get("root_ok"), inp.get("weights"), inp["intr"][g],
                       True, sigma, sl)
    q = [ref.unit(inp["quat"][g, v]) for v in range(tk.V)]
    T = [inp["trans"][g, v].astype(np.float64) for v in range(tk.V)]
    return tk, q, T


def test_the_projection_is_lift_refine_refs():
    """project_jac restates lift_refine_ref.evaluate for arrays: the same residual, cost and Jacobian at every point, clamped ones included"""
    g = np.random.default_rng(0)
    intr = refine.s11_intrinsics(1)[0]
    P = np.concatenate([g.uniform(-1, 1, (40, 2)), g.uniform(0.8, 6.0, (40, 1))], axis=1)
    P[:4, :2] *= 8.0                                                     # beyond the clamp
    kp = g.uniform(-1, 1, (40, 2))
    for distort in (True, False):
        du, dv, jac = ref.project_jac(P[:, 0], P[:, 1], P[:, 2], kp[:, 0], kp[:, 1], intr, distort)
        for n in range(40):
            e = refine.evaluate(P[n:n + 1], kp[n:n + 1], intr, [1.0], distort, np.zeros(3))
            assert e["F"] == du[n] * du[n] + dv[n] * dv[n]
            assert e["g"] == [jac[0][n] * du[n] + jac[3][n] * dv[n], jac[1][n] * du[n] + jac[4][n] * dv[n], jac[2][n] * du[n] + jac[5][n] * dv[n]]
            J = refine.jacobian(P[n], intr, distort)
            assert np.abs(J - np.array([[jac[0][n], jac[1][n], jac[2][n]], [jac[3][n], jac[4][n], jac[5][n]]])).max() <= 1e-12 * max(1.0, np.abs(J).max())


def test_the_camera_jacobian_against_central_differences():
    g = np.random.default_rng(1)
    intr = refine.s11_intrinsics(1)[0].astype(np.float64)
    h = 1e-6
    for n in range(20):
        P = np.array([g.uniform(-0.6, 0.6), g.uniform(-0.6, 0.6), g.uniform(2.0, 6.0)])
        _, _, jac = ref.project_jac(P[0], P[1], P[2], 0.0, 0.0, intr, True)
        rows = np.array(ref.camera_rows(jac, P[0], P[1], P[2]), np.float64)
        for c in range(6):
            side = []
            for s in (h, -h):
                d = np.zeros(6)
                d[c] = s
                th = np.linalg.norm(d[:3])                                # P' = exp([omega]x) P + tau by Rodrigues' formula, an independent route
                k = d[:3] / th if th > 0 else np.zeros(3)
                Pn = P * np.cos(th) + np.cross(k, P) * np.sin(th) + k * (k @ P) * (1 - np.cos(th)) + d[3:]
                du, dv, _ = ref.project_jac(Pn[0], Pn[1], Pn[2], 0.0, 0.0, intr, True)
                side.append(np.array([du, dv]))
            num = (side[0] - side[1]) / (2 * h)
            assert np.abs(num - rows[:, c]).max() <= 1e-7 * max(1.0, np.abs(rows[:, c]).max()), (n, c, num, rows[:, c])
    # ... and through the whole evaluation: a_v and b_f are half the gradient of F along move_camera's and the roots' own parametrisation
    sc = ref.scene(3, 5, [4], seed=40)
    for sigma in (float("inf"), 0.05):
        tk, q, T = _take(sc, sigma=sigma)
        e = ref.evaluate(tk, q, T, tk.root, True, [1, 2])
        for k, v in enumerate((1, 2)):
            for c in range(6):
                F = []
                for s in (h, -h):
                    d = np.zeros(6)
                    d[c] = s
                    qn, Tn = list(q), list(T)
                    qn[v], Tn[v] = ref.move_camera(q[v], T[v], d)
                    F.append(ref.cost_at(tk, qn, Tn, tk.root))
                want = 2.0 * e["am"][k][:, c].sum()
                assert abs((F[0] - F[1]) / (2 * h) - want) <= 1e-6 * max(1.0, abs(want)), (sigma, v, c)
        for c in range(3):
            r = [tk.root.copy(), tk.root.copy()]
            r[0][2, c] += h
            r[1][2, c] -= h
            want = 2.0 * e["b"][2, c]
            assert abs((ref.cost_at(tk, q, T, r[0]) - ref.cost_at(tk, q, T, r[1])) / (2 * h) - want) <= 1e-6 * max(1.0, abs(want))


def test_the_step_is_the_dense_solve_of_the_full_normal_equations():
    for V, J, F, seed, sigma in ((4, 17, 12, 41, float("inf")), (3, 5, 7, 42, 0.05), (2, 17, 1, 43, 0.05)):
        sc = ref.scene(V, J, [F], seed=seed)
        valid = np.ones((V, F), np.uint8)
        if F > 2:
            valid[1, 0], valid[V - 1, 2] = 0, 0                          # a free view that misses a frame
        tk, q, T = _take(sc, sigma=sigma, valid=valid)
        free = list(range(1, V))
        dc, dr = ref.schur_step(tk, q, T, tk.root, free)
        want_c, want_r = ref.dense_step(tk, q, T, tk.root, free)
        assert np.abs(dc - want_c).max() <= 1e-9 * np.abs(want_c).max() and np.abs(dr - want_r).max() <= 1e-9 * np.abs(want_r).max()


def test_sigma_inf_is_exactly_the_unweighted_problem():
    sc = ref.scene(3, 5, [9], seed=44)
    tk, q, T = _take(sc, sigma=float("inf"))
    e = ref.evaluate(tk, q, T, tk.root, True, [1, 2])
    plain = np.zeros(9)                                                  # sum w |res|^2 in the rule's order, no robust factor anywhere
    for v in range(3):
        R = ref.rotation(q[v])
        for j in range(5):
            w = tk.pose[:, j] + (tk.root - T[v])
            X, Y, Z = (R[0, c] * w[:, 0] + R[1, c] * w[:, 1] + R[2, c] * w[:, 2] for c in range(3))
            du, dv, _ = ref.project_jac(X, Y, Z, tk.kp[v, :, j, 0], tk.kp[v, :, j, 1], tk.intr[v], True)
            plain += 1.0 * (du * du + dv * dv)
    assert np.array_equal(e["Ff"], plain)
    a, b = ref.bundle(**ref.inputs(sc, sigma=float("inf"))), ref.bundle(**ref.inputs(sc, sigma=1e18))      # (a robust factor of 1 - 1e-36: rounds to 1)
    assert all(np.array_equal(a[k], b[k]) for k in a)
    c = ref.bundle(**ref.inputs(sc, sigma=0.01))
    assert not np.array_equal(a["quat"], c["quat"]) and c["cost"][0, 0] < a["cost"][0, 0]


def test_what_is_copied_through_is_copied_bit_for_bit():
    sc = ref.scene(4, 17, [6, 9], seed=45)
    inp = ref.inputs(sc, sigma=0.05)
    off = ref.bundle(**dict(inp, iters=0))
    assert np.array_equal(off["quat"], inp["quat"]) and np.array_equal(off["trans"], inp["trans"]) and np.array_equal(off["root"], inp["root"])
    assert off["steps"].tolist() == [0, 0] and off["ok"].tolist() == [1, 1] and np.array_equal(off["cost"][:, 0], off["cost"][:, 1]) and (off["cost"] > 0).all()
    fixed = np.array([[1, 0, 1, 0], [0, 1, 0, 0]], np.uint8)
    on = ref.bundle(**dict(inp, fixed=fixed))
    assert on["steps"].tolist() == [3, 3]
    for g, v in zip(*np.nonzero(fixed)):
        assert np.array_equal(on["quat"][g, v], inp["quat"][g, v]) and np.array_equal(on["trans"][g, v], inp["trans"][g, v])
    for g, v in zip(*np.nonzero(fixed == 0)):
        assert not np.array_equal(on["quat"][g, v], inp["quat"][g, v]) and abs(np.linalg.norm(on["quat"][g, v]) - 1) < 1e-15 and on["quat"][g, v, 0] >= 0
    root_ok = np.ones(15, np.uint8)
    root_ok[[2, 8]] = 0                                                   # a frame outside the problem keeps its root
    out = ref.bundle(**dict(inp, root_ok=root_ok))
    assert np.array_equal(out["root"][[2, 8]], inp["root"][[2, 8]]) and out["used"].tolist() == [[5] * 4, [8] * 4]
    assert not np.array_equal(out["root"][3], inp["root"][3])


def test_the_gauge_and_the_degenerate_takes():
    assert ref.gauge([5, 5, 5, 5], None) == ([1, 2, 3], True) and ref.gauge([0, 5, 5], None) == ([2], True)           # the lowest view with a used frame is held
    assert ref.gauge([5, 5, 5], [0, 0, 1]) == ([0, 1], True) and ref.gauge([5, 0, 5], [0, 0, 1]) == ([0], True)
    assert ref.gauge([5, 5, 5], [0, 0, 0]) == ([], False) and ref.gauge([5, 5, 5], [1, 1, 1]) == ([], False)         # no fixed view; no free view
    assert ref.gauge([5, 5, 0], [0, 0, 1]) == ([], False) and ref.gauge([0, 0, 0], None) == ([], False) and ref.gauge([7], None) == ([], False)
    sc = ref.scene(3, 5, [12], seed=31)
    inp = ref.inputs(sc, sigma=0.05)
    for fixed in (np.zeros((1, 3), np.uint8), np.ones((1, 3), np.uint8), np.array([[0, 0, 1]], np.uint8)):
        valid = np.ones((3, 12), np.uint8)
        valid[2] = fixed[0, 2] == 0                                      # (the third: the only fixed view observes nothing)
        r = ref.bundle(**dict(inp, fixed=fixed, valid=valid))
        assert r["steps"][0] == 0 and r["ok"][0] == 1 and np.array_equal(r["quat"], inp["quat"]) and np.array_equal(r["root"], inp["root"])
        assert r["cost"][0, 0] == r["cost"][0, 1] > 0 and np.array_equal(r["reproj"][..., 0], r["reproj"][..., 1])
    behind = dict(inp, pose=inp["pose"].copy())
    behind["pose"][5, 3] = (-40.0 * ref.rotation(ref.unit(inp["quat"][0, 0]))[:, 2]).astype(np.float32)
    r = ref.bundle(**behind)
    assert r["ok"][0] == 0 and r["steps"][0] == 0 and np.array_equal(r["quat"], inp["quat"]) and np.array_equal(r["root"], inp["root"])
    zero = dict(inp, quat=inp["quat"].copy())
    zero["quat"][0, 0] = 0
    r = ref.bundle(**zero)
    assert r["used"][0].tolist() == [0, 12, 12] and r["steps"][0] == 3 and np.array_equal(r["quat"][0, :2], zero["quat"][0, :2]) and r["reproj"][0, 0].tolist() == [0, 0]
    nan = dict(inp, quat=inp["quat"].copy())
    nan["quat"][0, 1, 2] = np.nan
    assert ref.bundle(**nan)["used"][0].tolist() == [12, 0, 12]
    empty = ref.bundle(**dict(inp, valid=np.zeros((3, 12), np.uint8)))   # nothing observed: F = 0 is evaluated, nothing moves
    assert empty["ok"][0] == 1 and empty["steps"][0] == 0 and not empty["cost"].any() and not empty["reproj"].any() and not empty["used"].any()
    # a step that would raise the cost is not taken, and the state stays: one frame, one camera 40 degrees and 1 m off, undamped
    far = ref.refused_scene()
    trace = []
    r = ref.bundle(trace=trace, **ref.inputs(far, iters=8))
    costs = [d for d in trace if d["kind"] == "cost"]
    assert [d["taken"] for d in costs] == [True, False] and r["steps"][0] == 1 and r["cost"][0, 1] < r["cost"][0, 0] and costs[1]["F"] > r["cost"][0, 1]
    assert all(d["taken"] for d in trace if d["kind"] != "cost") and ref.margin(trace) >= ref.MARGIN_MIN
    once = ref.bundle(**ref.inputs(far, iters=1))
    assert all(np.array_equal(once[k], r[k]) for k in r)                  # the state of the last step taken
    flat = ref.scene(2, 17, [3], seed=47)                                 # every joint at the root: a camera sees one point per frame, S is singular
    flat["pose"][:] = 0
    trace = []
    r = ref.bundle(trace=trace, **ref.inputs(flat))
    assert r["steps"][0] == 0 and r["ok"][0] == 1 and [d["kind"] for d in trace if not d["taken"]] in (["det"], ["pivot"])


def test_the_quaternion_sign_rule_and_the_small_angle_branch():
    T = np.array([1.0, 2.0, 3.0])
    for q, want in (([0.0, -1.0, 0.0, 0.0], [0, 1, 0, 0]), ([-0.0, 0.0, -0.6, 0.8], [0, 0, 0.6, -0.8]), ([-0.5, 0.5, 0.5, 0.5], [0.5, -0.5, -0.5, -0.5]),
                    ([0.5, -0.5, -0.5, -0.5], [0.5, -0.5, -0.5, -0.5])):
        got, Tn = ref.move_camera(np.array(q), T, np.zeros(6))
        assert np.abs(got - want).max() < 1e-15 and not np.signbit(got[got == 0]).any() and np.array_equal(Tn, T) and got[np.nonzero(got)[0][0]] > 0
    # half a turn about x from the identity: w = cos(pi / 2) rounds to 6e-17 > 0, the vector part keeps the sign of conj(q_w)
    got, _ = ref.move_camera(np.array([1.0, 0, 0, 0]), T, np.array([np.pi, 0, 0, 0, 0, 0]))
    assert got[0] >= 0 and abs(got[1] + 1) < 1e-15
    w = np.array([3e-9, -4e-9, 0.0])                                     # |w|^2 = 2.5e-17 <= 1e-16: q_w = (1, w / 2); the exact one differs by |w|^2 / 8
    small, _ = ref.move_camera(np.array([1.0, 0, 0, 0]), T, np.concatenate([w, np.zeros(3)]))
    assert np.abs(small - np.array([1.0, -1.5e-9, 2e-9, 0.0])).max() < 1e-16
    big, Tn = ref.move_camera(np.array([1.0, 0, 0, 0]), T, np.array([0.0, 0.0, np.pi / 2, 1.0, 0.0, 0.0]))
    # exp([w]x) = a quarter turn about z of the camera-space point: R' = R exp(-[w]x), and T' = T - R' tau
    assert np.abs(ref.rotation(big) - np.array([[0, 1, 0], [-1, 0, 0], [0, 0, 1.0]])).max() < 1e-15 and np.abs(Tn - (T - np.array([0.0, -1.0, 0.0]))).max() < 1e-15


def test_recovery_on_the_committed_seeds():
    """S11's four cameras, 60 frames, 17 joints, seed 7, views 1..3 start 0.3 degrees and 0.15 m off, the roots 0.05 m N(0, 1) (lift_bundle_ref.RECOVERY).
    Measured with the float64 statement:
      noise-free float32 keypoints    step 1: 0.008 - 0.030 degrees, 1.2 - 4.3 mm;  step 2: 1.4e-5 degrees, 2.1e-6 m, roots 1.4e-6 m;
                                      step 3: 1.2e-7 degrees, 1.5e-8 m, roots 1.6e-8 m, and no further (the keypoints' own rounding)
      0.002 keypoint noise            3 steps: 0.024 - 0.034 degrees, 2.1 - 4.8 mm, roots within 5.3 mm; the same after 8
      the alternation, 8 rounds       noise-free 0.037 - 0.082 degrees, 3.2 - 7.9 mm; with noise a cost of 0.031825 against the joint 0.031659
    The claims: the truth is reached in RECOVERY_STEPS = 3 steps within twice what was measured; with noise every free view ends closer to the truth
    in angle and in distance than it started; the alternation (resection <-> root fit, three Gauss-Newton steps each, 8 rounds) ends worse than 3
    joint steps in every view."""
    sc = ref.recovery(0.0)
    assert np.abs(sc["trans"]).max() < 8 and np.abs(sc["true_root"]).max() < 2          # what STORE_M and STORE_ROOT stand on
    trace = []
    res = ref.bundle(trace=trace, **ref.inputs(sc, iters=ref.RECOVERY_STEPS))
    deg, m = ref.camera_errors(res["quat"], res["trans"], sc)
    worst = np.abs(res["root"] - sc["true_root"]).max()
    cond = max(d["cond"] for d in trace if d["kind"] == "pivot")
    print("noise-free:", deg[1:], m[1:], worst, "condition number of S", cond)
    assert res["steps"][0] == ref.RECOVERY_STEPS and deg.max() <= ref.RECOVERY_DEG and m.max() <= ref.RECOVERY_M and worst <= ref.RECOVERY_ROOT
    assert deg.max() >= ref.RECOVERY_DEG / 4 and 5e3 < cond < 5e4      # (the bounds are twice what is measured, not more)
    tk, q, T = _take(sc)
    qa, Ta, ra = ref.alternate(tk, sc["quat"][0], sc["trans"][0], [1, 2, 3], rounds=8)
    da, ma = ref.camera_errors(np.array(qa)[None], np.array(Ta)[None], sc)
    print("alternation, noise-free:", da[1:], ma[1:])
    assert (da[1:] > 1e3 * deg[1:]).all() and (ma[1:] > 1e3 * m[1:]).all() and (da[1:] < 0.3).all()
    sc = ref.recovery(0.002)
    d0, m0 = ref.camera_errors(sc["quat"], sc["trans"], sc)
    res = ref.bundle(**ref.inputs(sc))
    deg, m = ref.camera_errors(res["quat"], res["trans"], sc)
    print("noise 0.002:", deg[1:], m[1:], np.abs(res["root"] - sc["true_root"]).max())
    assert res["steps"][0] == 3 and (deg[1:] < d0[1:]).all() and (m[1:] < m0[1:]).all() and deg.max() < 0.05 and m.max() < 0.006
    # with noise the truth is not the minimum; "worse" is: a higher cost, and in every view farther from where the joint steps converge
    tk, q, T = _take(sc)
    qa, Ta, ra = ref.alternate(tk, sc["quat"][0], sc["trans"][0], [1, 2, 3], rounds=8)
    end = ref.bundle(**ref.inputs(sc, iters=8))
    at = dict(true_quat=np.stack([[ref.unit(x) for x in end["quat"][0]]]), true_trans=end["trans"])
    da, ma = ref.camera_errors(np.array(qa)[None], np.array(Ta)[None], at)
    dj, mj = ref.camera_errors(res["quat"], res["trans"], at)
    print("from the converged cameras: alternation", da[1:], ma[1:], "3 joint steps", dj[1:], mj[1:])
    assert ref.cost_at(tk, qa, Ta, ra) > res["cost"][0, 1] and (da[1:] > dj[1:]).all() and (ma[1:] > mj[1:]).all()


def test_the_device_tests_scenes_decide_far_from_their_thresholds():
    seen = set()
    for tag, inp, want, trace in ref.cases():
        assert ref.margin(trace) >= ref.MARGIN_MIN, (tag, ref.margin(trace))
        assert all(d["taken"] for d in trace), tag                       # (no scene of the comparison rests on a refusal)
        assert want["ok"].all() and (want["cost"][:, 1] > 1e-6).all()    # F at the minimum is far above rounding
        seen |= {(int(inp["kp"].shape[0]), int(inp["kp"].shape[2]))}
    frames = {int(n) for _, inp, _, _ in ref.cases() for n in np.diff(inp["take_offset"])}
    assert {1, 5, 65, 257, 600} <= frames and {(4, 17), (3, 5), (2, 17)} <= seen
    assert {int(inp.get("iters", 3)) for _, inp, _, _ in ref.cases()} == {0, 1, 3, 8}
    for noise in (0.002,):
        trace = []
        ref.bundle(trace=trace, **ref.inputs(ref.recovery(noise)))
        assert ref.margin(trace) >= ref.MARGIN_MIN
    for sc, kw in ((ref.scene(3, 5, [12], seed=31), dict(sigma=0.05)), (ref.scene(3, 5, [6], seed=32), {})):       # the constructed takes' base scenes
        trace = []
        ref.bundle(trace=trace, **ref.inputs(sc, **kw))
        assert ref.margin(trace) >= ref.MARGIN_MIN


def test_new_abi_symbol_is_declared_everywhere():
    from manipose_amd import _lib, lifting
    import manipose_amd
    header = open(_lib.HEADER_PATH).read()
    assert {"mp_lift_bundle_views", "mp_lift_bundle_views_scratch_bytes"} <= set(_lib.declared_symbols())
    assert len(_lib._SIGNATURES["mp_lift_bundle_views"][1]) == 29 and len(_lib._SIGNATURES["mp_lift_bundle_views_scratch_bytes"][1]) == 2
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "lib.mp_lift_bundle_views.argtypes" in integration and "lib.mp_lift_bundle_views_scratch_bytes.argtypes" in integration
    assert _lib.ABI_VERSION == 8 and int(re.search(r"#define MP_ABI_VERSION (\d+)", header).group(1)) == 8        # purely additive
    assert int(re.search(r"#define MP_LIFT_BUNDLE_MAXITERS (\d+)", header).group(1)) == lifting.BUNDLE_MAXITERS == ref.MAXITERS == 8
    assert manipose_amd.bundle_views is lifting.bundle_views and "bundle_views" in lifting.__all__
    assert (lifting.BUNDLE_SIGMA, lifting.BUNDLE_ITERS) == (0.05, 3)
    assert lifting.ViewBundle._fields == ("cameras", "quat", "trans", "root", "reproj", "cost", "steps", "ok", "used")
    assert os.path.exists(os.path.join(ROOT, "manipose_amd", "csrc", "lift_bundle.hip"))
    for name in ("README.md", "DESIGN.md"):
        text = open(os.path.join(ROOT, name)).read()
        assert "mp_lift_bundle_views" in text and "lift.fuse_bundle" in text
    assert "--bundle" in open(os.path.join(ROOT, "tools", "lift_bench.py")).read()
    if os.path.exists(_lib.LIB_PATH):
        assert hasattr(_lib.load(), "mp_lift_bundle_views") and _lib.load().mp_lift_bundle_views_scratch_bytes(4, 10) == 10 * 3056


def test_config_keys_parse_and_a_bundle_without_estimated_cameras_fails():
    from _entry import BUNDLE_KEYS, LIFT_SUFFIXES, lift_fuse_bundle_options, load_config, run
    cfg = load_config([])
    assert cfg.lift.fuse_bundle == 0 and lift_fuse_bundle_options(cfg) == (0, 0.05)
    on = ["run.lift=true", "lift.fuse=true", "lift.fuse_cameras=estimate"]
    assert lift_fuse_bundle_options(load_config(on)) == (0, 0.05)
    assert lift_fuse_bundle_options(load_config(on + ["lift.fuse_bundle=3"])) == (3, 0.05)
    assert lift_fuse_bundle_options(load_config(on + ["lift.fuse_bundle=8", "lift.fuse_bundle_sigma=0.2"])) == (8, 0.2)
    with pytest.raises(SystemExit):
        load_config(["lift.fuse_bundles=3"])
    fused = ["run.lift=true", "lift.fuse=true"]
    for argv, word in ((fused + ["lift.fuse_bundle=3"], "set lift.fuse_cameras=estimate"), (["lift.fuse_bundle=1"], "set lift.fuse_cameras=estimate"),
                       (["run.lift=true", "lift.fuse_bundle=2"], "set lift.fuse_cameras=estimate"), (on + ["lift.fuse_bundle_sigma=0.1"], "set lift.fuse_bundle=N"),
                       (fused + ["lift.fuse_bundle_sigma=0.1"], "set lift.fuse_bundle=N"), (on + ["lift.fuse_bundle=9"], "0..8"), (on + ["lift.fuse_bundle=-1"], "0..8"),
                       (on + ["lift.fuse_bundle=1.5"], "0..8"), (on + ["lift.fuse_bundle=true"], "0..8"), (on + ["lift.fuse_bundle=3", "lift.fuse_bundle_sigma=0"], "> 0"),
                       (on + ["lift.fuse_bundle=3", "lift.fuse_bundle_sigma=abc"], "is a number"), (on + ["lift.fuse_bundle=3", "lift.fuse_bundle_sigma=true"], "is a number")):
        with pytest.raises(ValueError, match=word):
            run(["run.train=false", "run.test=false"] + argv)                    # (a run that got further would need a device)
    assert all("__cam_" + s in LIFT_SUFFIXES for s in BUNDLE_KEYS) and len(BUNDLE_KEYS) == 9


def test_argument_errors_are_value_errors_before_any_device_work():
    """The calls are given CPU tensors: had the arguments been accepted, they would have ended in the RuntimeError that refuses them ("no CPU
    fallback"), which is what the valid calls at the end do."""
    from manipose_amd import bundle_views
    pose, root, kp = torch.zeros(6, 17, 3), torch.zeros(6, 3), torch.zeros(3, 6, 17, 2)
    cam = np.concatenate([np.ones(9), [1, 0, 0, 0], np.zeros(3)])
    cams, ok = [[cam, cam, cam]], torch.ones(6, dtype=torch.uint8)
    base = dict(pose=pose, root=root, keypoints_2d=kp, cameras=cams)
    for kw, word in ((dict(pose=torch.zeros(6, 17, 2)), "pose must be"), (dict(pose=pose.double()), "pose must be"), (dict(pose=torch.zeros(6, 1, 3)), "pose must be"),
                     (dict(root=torch.zeros(5, 3)), "root must be"), (dict(root=root.double()), "root must be"), (dict(keypoints_2d=torch.zeros(5, 6, 17, 2)), "keypoints_2d"),
                     (dict(keypoints_2d=torch.zeros(3, 6, 16, 2)), "keypoints_2d"), (dict(valid=torch.ones(2, 6, dtype=torch.uint8)), "valid must be"),
                     (dict(valid=torch.ones(3, 6)), "valid must be"), (dict(root_ok=torch.ones(5, dtype=torch.uint8)), "root_ok must be"),
                     (dict(root_ok=np.ones(6, np.uint8)), "root_ok must be"), (dict(root_ok=ok.bool()), "root_ok must be"), (dict(cameras=[[cam, cam]]), "3 views"),
                     (dict(cameras={"view": cam}), "nested list"), (dict(cameras=[[cam, cam[:5], cam]]), "view 1"),
                     (dict(cameras=[[cam, np.concatenate([np.ones(9), np.zeros(7)]), cam]]), "zero quaternion"), (dict(fixed=[1, 0]), "fixed must be"),
                     (dict(fixed=[[1.0, 0, 0]]), "fixed must be"), (dict(fixed=np.ones((2, 3), np.uint8)), "fixed must be"), (dict(weights=np.ones(16)), "weights"),
                     (dict(weights=-np.ones(17)), "weights"), (dict(sigma=0), "sigma"), (dict(sigma=-1.0), "sigma"), (dict(sigma=float("nan")), "sigma"),
                     (dict(sigma="a"), "sigma"), (dict(sigma=True), "sigma"), (dict(iters=9), "iters"), (dict(iters=-1), "iters"), (dict(iters=1.5), "iters"),
                     (dict(iters=True), "iters")):
        with pytest.raises(ValueError, match=word):
            bundle_views(**dict(base, **kw))
    for kw in (dict(), dict(valid=torch.ones(3, 6, dtype=torch.uint8), root_ok=ok, fixed=[1, 0, 0], weights=np.ones(17), distort=False, sigma=float("inf"), iters=0),
               dict(cameras=[[cam, None, cam]], fixed=np.array([[0, 0, 1]]))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            bundle_views(**dict(base, **kw))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        bundle_views(np.zeros((6, 17, 3), np.float32), root, kp, cams)

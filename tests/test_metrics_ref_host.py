"""The fp64 references of tests/metrics_ref.py, verified without a GPU: they reproduce every output of the reference project's own metric
functions recorded in the `metrics` fixture (so the reference is the right function, independently of the kernels), no case is left out
of any comparison (every error of every case lies at least 64 u of its scale away from every PCK / AUC threshold, the planted ties are
exact in fp32, every non-special Procrustes frame stays below the conditioning cap), and the bound constants test_gpu_metric_kernels.py
asserts follow from the error of the same formulas evaluated in plain fp32 numpy on the CPU (ends_ref.bound_from: 4 x the worst
error / scale ratio over the GPU module's cases, rounded up to one significant digit, never below 1)."""
import numpy as np
import pytest

import metrics_ref as mr
from helpers import load_fixture

F32, F64 = np.float32, np.float64


def close(got, want, what, rtol=5e-6, atol=0.0):
    got, want = np.asarray(got, dtype=F64), np.asarray(want, dtype=F64)
    assert got.shape == want.shape or want.size == 1, (what, got.shape, want.shape)
    err = np.abs(got - want)
    assert (err <= rtol * np.abs(want) + atol).all(), f"{what}: error {err.max():.3g} against {np.abs(want).max():.3g}"


# ------------------------------------------------------------------------------------------------ the recorded outputs of the reference
@pytest.mark.parametrize("nm", ["pred", "rigid"])
def test_reference_reproduces_the_recorded_metrics_fixture(nm):
    """every key of the fixture.  The recorded values are fp32 results of the reference's torch / numpy code: 5e-6 relative; the variance
    of the rigid sequence is rounding noise of lengths ~250 mm in the recording (absolute floors 1e-6 mm^2 and 1e-3 mm, as in
    test_gpu_parity.py).  Percentages are counts: they must agree to within the recording's own fp32 rounding of the percentage, unless a
    joint lies within 64 u of a threshold (none does for `rigid`; the free prediction of the fixture is not settled, such joints are counted
    and allowed for)"""
    fx = load_fixture("metrics")
    x, gt, mask = fx[nm], fx["gt"], fx["mask"]
    B, L = x.shape[:2]
    n = B * L
    T = mr.pose_terms(x, gt, False)
    e, e2, dp, dp2, dl, plen = T["e"][0], T["e2"][0], T["sym"][0], T["sym2"][0], T["dl"][0], T["plen"][0]
    agg = {"average": np.mean, "sum": np.sum}
    vat, sat = (1e-6, 1e-3) if nm == "rigid" else (0.0, 0.0)
    for mode, f in agg.items():
        close(f(e), fx[f"{nm}.mpjpe.{mode}"], "mpjpe " + mode)
        close(f(e2), fx[f"{nm}.mse.{mode}"], "mse " + mode)
        close(f(e.reshape(n, 17), axis=0), fx[f"{nm}.jw_err.{mode}"], "jw_err " + mode)
        close(f(e2.reshape(n, 17), axis=0), fx[f"{nm}.jw_mse.{mode}"], "jw_mse " + mode)
        for sq, d in ((0, dp), (1, dp2)):
            close(f(d), fx[f"{nm}.sym.{mode}.{sq}"], f"sym {mode} {sq}")
            close(f(d.reshape(n, 6), axis=0), fx[f"{nm}.sym_per_bone.{mode}.{sq}"], f"sym_per_bone {mode} {sq}")
        abs_sum = np.abs(dl).sum() if mode == "sum" else np.abs(dl).mean()
        close(f(np.abs(dl)), fx[f"{nm}.len_err.{mode}.0"], "len_err unsigned " + mode)
        close(f(dl), fx[f"{nm}.len_err.{mode}.1"], "len_err signed " + mode, atol=5e-6 * abs_sum)      # a signed sum: the unsigned scale
    var = plen.var(1, ddof=1)                                  # (B, 16)
    std = np.sqrt(var)
    for mode, f in (("average", np.mean), ("sum", np.sum), ("min", np.min), ("max", np.max)):
        close(f(var), fx[f"{nm}.stc.{mode}"], "stc " + mode, atol=vat * (48 if mode == "sum" else 1))
    close(std.mean(), fx[f"{nm}.stc.std"], "stc std", atol=sat)
    close(var.mean(0), fx[f"{nm}.stc_per_bone.average"], "stc_per_bone average", atol=vat)
    close(var.sum(0), fx[f"{nm}.stc_per_bone.sum"], "stc_per_bone sum", atol=vat * 3)
    close(std.mean(0), fx[f"{nm}.stc_per_bone.std"], "stc_per_bone std", atol=sat)
    flat = plen.reshape(n, 16)
    close(np.sqrt(flat.var(0, ddof=1)).mean(), fx[f"{nm}.stc_flat.std"], "stc_flat std", atol=sat)
    nv = B * (L - 1) * 17
    close(T["vel"][0].sum() / nv, fx[f"{nm}.vel"], "vel")
    close(T["vel2"][0].sum() / (3 * nv), fx[f"{nm}.vel_sq"], "vel_sq")
    # the report of the accumulator on the same frames is the same function
    rep = mr.report_ref([(x, gt)])
    close(rep["mpjpe"][0], fx[f"{nm}.mpjpe.average"], "report mpjpe")
    close(rep["mpsce"][0], fx[f"{nm}.stc_flat.std"], "report mpsce", atol=sat)
    close(rep["mvjpe"][0], fx[f"{nm}.vel"], "report mvjpe")
    # counts
    xf, gf = x.reshape(1, n, 17, 3), gt.reshape(1, n, 17, 3)
    m = mask.reshape(1, n, 17)

    def percent(r, slot, den):
        return 100.0 * r["row"][0, slot] / den

    def near(r, thr):
        return int((mr.near_threshold(r["e"], r["e_scale"], thr, mr.MARGIN) & r["vis"]).sum())

    grid = mr.thresholds_of(150.0, 150.0, 31)
    for al in ("none", "scale"):
        r = mr.pose_metrics_ref(xf, gf, None, scale_align=(al == "scale"))
        k = near(r, grid)
        close(percent(r, 6, n * 17), fx[f"{nm}.pck.{al}"], "pck " + al, rtol=1e-6, atol=100.0 * k / (n * 17))
        close(percent(r, 7, 31 * n * 17), fx[f"{nm}.auc.{al}"], "auc " + al, rtol=1e-6, atol=100.0 * k / (31 * n * 17))
    r = mr.pose_metrics_ref(xf, gf, m)
    vis, k = m.sum(), near(r, grid)
    close(percent(r, 6, vis), fx[f"{nm}.pck.masked"], "pck masked", rtol=1e-6, atol=100.0 * k / vis)
    close(percent(r, 7, 31 * vis), fx[f"{nm}.auc.masked"], "auc masked", rtol=1e-6, atol=100.0 * k / (31 * vis))
    r = mr.pose_metrics_ref(xf, gf, None, pck_thr=80.0)
    close(percent(r, 6, n * 17), fx[f"{nm}.pck.thr80"], "pck 80", rtol=1e-6, atol=100.0 * near(r, np.array([80.0])) / (n * 17))
    for mk, key in ((None, ""), (m[0], ".masked")):
        p = mr.procrustes_ref(xf[0], gf[0], mk)
        k = int((mr.near_threshold(p["e"], p["e_scale"], grid, mr.MARGIN) & p["vis"]).sum())
        close(100.0 * p["out"][1] / p["out"][3], fx[f"{nm}.pck.procrustes{key}"], "pck procrustes" + key, rtol=1e-6, atol=100.0 * k / p["out"][3])
        if mk is None:
            close(100.0 * p["out"][2] / (31 * p["out"][3]), fx[f"{nm}.auc.procrustes"], "auc procrustes", rtol=1e-6, atol=100.0 * k / (31 * p["out"][3]))
            close(p["out"][0] / (n * 17), fx[f"{nm}.p_mpjpe"], "p_mpjpe", rtol=1e-5)
            # lambda_1 of Horn's N is trace(S) with the reflection fix, in the unnormalised units: a = lambda_1 / |y0|^2
            y0 = xf[0].astype(F64) - xf[0].astype(F64).mean(1, keepdims=True)
            close(p["lam1"] / (y0 ** 2).sum((1, 2)), p["a"], "Horn's lambda_1 against the SVD's scale", rtol=1e-10)


def test_layouts_address_the_frames_they_were_built_from():
    a = mr.skeleton_frames((3, 5), 1)[0]
    for form in ("contig", "perm", "pad"):
        s, off, st = mr.layout(a, form)
        assert np.array_equal(mr.gather(s, off, st, 3, 5), a) and int(np.isfinite(s).sum()) == a.size, form
    assert mr.layout(a, "contig")[2] == (5 * 51, 51, 3, 1) and mr.layout(a, "pad")[1] == 7
    assert mr.NV == 122 and len(mr.SLOT_KEYS) == mr.NV


# ------------------------------------------------------------------------------------------------ no case is left out
def _margin_ok(r, thr, planted, what):
    near = mr.near_threshold(r["e"], r["e_scale"], thr, mr.MARGIN)
    if planted is not None:
        near &= ~planted
    assert not near.any(), f"{what}: {int(near.sum())} errors within 64 u of a threshold"
    assert np.isfinite(r["e_scale"]).all(), what


@pytest.mark.parametrize("name", mr.POSE_CASES)
def test_every_pose_error_keeps_its_margin_from_every_threshold(name):
    c = mr.pose_case(name)
    for v in c["variants"]:
        if v["gt"]:
            r = mr.pose_metrics_ref(c["pred"], c["gt"], None, v["ps"], v["gs"], v["pck"], v["auc_max"], v["auc_steps"], v["align"])
            _margin_ok(r, mr.thresholds_of(v["pck"], v["auc_max"], v["auc_steps"]), c["planted"], f"{name} {mr.vname(v)}")
    if c["mask"].shape[1] >= 127:
        assert len({m.tobytes() for m in c["mask"]}) == c["mask"].shape[0], "every batch item has a mask of its own"
        assert (~c["mask"].any(-1)).any(1).all(), "every batch item has fully invisible frames"


def test_planted_ties_are_exact_in_fp32():
    """the subtraction pred - gt of the tie case is exact, the fp32 norm of the planted joint IS the threshold 5 i, the fp64 reference counts
    strictly: PCK does not count the tie, the AUC count is 30 - i"""
    c = mr.pose_case("ties")
    p, g = c["pred"], c["gt"]
    assert np.array_equal((p - g).astype(F64), p.astype(F64) - g.astype(F64))
    d = (p - g)[:, 0, mr.TIE_JOINT]
    e32 = np.sqrt((d * d).sum(-1, dtype=F32), dtype=F32)
    grid = mr.auc_grid(150.0, 31)
    assert np.array_equal(e32.astype(F64), grid) and np.array_equal(grid, 5.0 * np.arange(31))
    for thr in (150.0, 80.0):
        r = mr.pose_metrics_ref(p, g, None, pck_thr=thr)
        assert np.array_equal(r["e"][:, 0, mr.TIE_JOINT], grid)
        assert np.array_equal(r["row"][:, 6], 16 + (grid < thr)) and np.array_equal(r["row"][:, 7], 16 * 30 + (30 - np.arange(31)))
    assert mr.f32(0.15) / 30 != mr.f32(mr.f32(0.15) / 30)      # the grid of the metre cases: its step is no fp32 number


@pytest.mark.parametrize("N", mr.PROC_N)
def test_every_procrustes_frame_keeps_its_margin_and_stays_below_the_gap_cap(N):
    c = mr.procrustes_case(N)
    worst = 0.0
    for v in mr.PROC_VARIANTS:
        r = mr.procrustes_ref(c["pred"], c["gt"], None, pck_thr=v["pck"])
        _margin_ok(r, mr.thresholds_of(v["pck"], 150.0, 31), None, f"N={N} pck={v['pck']}")
        worst = max(worst, float(r["kappa"].max()))
    print(f"[metrics ref] Procrustes N={N}: largest 1 + lambda_1 / (lambda_1 - lambda_2) = {worst:.3g} (cap {mr.GAP_CAP:g})")
    assert worst < mr.GAP_CAP
    if N > 256:
        e = mr.procrustes_ref(c["pred"], c["gt"], None)["e"].sum(1)
        assert e[[255, 256, N - 1]].min() > 2.5 * np.median(e)          # the edge frames stand out


def test_special_procrustes_frames_carry_their_own_gap():
    names = [s["name"] for s in mr.procrustes_specials()]
    assert len(names) == len(set(names)) and 35 <= len(names) <= 45
    for s in mr.procrustes_specials():
        for thr in (150.0, 80.0):
            r = mr.procrustes_ref(s["pred"], s["gt"], None, s["ps"], s["gs"], pck_thr=thr, axis_free=s["axis_free"])
            _margin_ok(r, mr.thresholds_of(thr, 150.0, 31), None, s["name"])
        full = mr.procrustes_ref(s["pred"], s["gt"], None, s["ps"], s["gs"])
        print(f"[metrics ref] special frame {s['name']}: 1 + lambda_1 / gap = {r['kappa'][0]:.3g}, sum of aligned errors {r['out'][0]:.4g}")
        if s["name"].startswith("collinear"):
            assert full["gap"][0] < 1e-6 * full["lam1"][0] and r["kappa"][0] < 100          # lambda_1 == lambda_2 up to the fp32 rounding of the points
        if s["name"].startswith("similar"):
            assert r["out"][0] < 1e-2
        if s["name"].startswith("mirror"):          # the reflection fix is taken: the plain R = V U^T is improper
            x, y = s["gt"][0].astype(F64), s["pred"][0].astype(F64)
            U, _, Vt = np.linalg.svd((x - x.mean(0)).T @ (y - y.mean(0)))
            assert np.linalg.det(Vt.T @ U.T) < 0


def test_report_batches_keep_their_margins():
    for i, (p, g) in enumerate(mr.report_case()):
        for v in (mr.variant(), mr.variant(align=True), mr.variant(pck=80.0)):
            _margin_ok(mr.pose_metrics_ref(p, g, None, pck_thr=v["pck"], scale_align=v["align"]), mr.thresholds_of(v["pck"], 150.0, 31), None, f"batch {i}")
        for v in mr.PROC_VARIANTS:
            r = mr.procrustes_ref(p.reshape(-1, 17, 3), g.reshape(-1, 17, 3), None, pck_thr=v["pck"])
            _margin_ok(r, mr.thresholds_of(v["pck"], 150.0, 31), None, f"batch {i} procrustes")
            assert r["kappa"].max() < mr.GAP_CAP
    rigid = mr.report_case()[1][0]
    plen = mr.pose_terms(rigid, None, False)["plen"][0]
    assert np.abs(plen - plen[:, :1]).max() < 1e-3          # the rigid batch stayed rigid
    plen = mr.pose_terms(mr.pose_case("rigid_L257")["pred"], None, False)["plen"][0]
    assert np.abs(plen - plen[:, :1]).max() < 5e-3


# ------------------------------------------------------------------------------------------------ the bound constants
def _ratios():
    """key -> worst error / scale of the plain fp32 CPU evaluation over the cases of test_gpu_metric_kernels.py"""
    w = {}

    def add(key, got, want, scale):
        w[key] = max(w.get(key, 0.0), mr.worst(got, want, scale))

    for name in mr.POSE_CASES:
        c = mr.pose_case(name)
        for v in c["variants"]:
            a = (c["pred"], c["gt"] if v["gt"] else None, c["mask"] if v["mask"] else None, v["ps"], v["gs"], v["pck"], v["auc_max"], v["auc_steps"], v["align"])
            r64, r32 = mr.pose_metrics_ref(*a), mr.pose_metrics_ref(*a, dtype=F32)
            for key in set(mr.SLOT_KEYS) - {"count"}:
                s = [i for i, k in enumerate(mr.SLOT_KEYS) if k == key]
                add(mr.row_key(key, name, c["rigid"]), r32["row"][:, s], r64["row"][:, s], r64["row_scale"][:, s])
            add(mr.row_key("len0", name), r32["len0"], r64["len0"], r64["len0_scale"])
            if not v["gt"]:
                assert not r64["row"][:, mr.GT_SLOTS].any() and not r64["row_scale"][:, mr.GT_SLOTS].any()
        if name in ("frames_L2", "B3L257", "rigid_L257"):
            for signed in (0, 1):
                t64, t32 = mr.bone_table_ref(c["pred"], c["gt"], signed), mr.bone_table_ref(c["pred"], c["gt"], signed, F32)
                add("blt", t32[0], t64[0], t64[1])
    for N in mr.PROC_N:
        c = mr.procrustes_case(N)
        r = mr.procrustes_ref(c["pred"], c["gt"], None)
        for how in ("jacobi", "svd"):
            e = mr.procrustes_f32(c["pred"], c["gt"], how=how)
            add("pr_frame", e.sum(1, dtype=F32), r["e"].sum(1), r["e_scale"].sum(1) + r["e"].sum(1))
            add("pr_sum", e.sum(dtype=F32), r["out"][0], r["out_scale"])
            add("pr_joint", e, r["e"], r["e_scale"])
    for s in mr.procrustes_specials():
        r = mr.procrustes_ref(s["pred"], s["gt"], None, s["ps"], s["gs"], axis_free=s["axis_free"])
        for how in ("jacobi", "svd"):
            e = mr.procrustes_f32(s["pred"], s["gt"], s["ps"], s["gs"], how=how)
            add("pr_frame", e.sum(1, dtype=F32), r["e"].sum(1), r["e_scale"].sum(1) + r["e"].sum(1))
            add("pr_joint", e, r["e"], r["e_scale"])
    # bone_variance from the fp32 sums, per item of the three batches of the host-arithmetic test
    for (p, g), (_, L, rigid) in zip(mr.report_case(), mr.REPORT_BATCHES):
        r32 = mr.pose_metrics_ref(p, g, None, dtype=F32)
        s1, s2 = r32["row"][:, mr.OB:mr.OP:4].astype(F64), r32["row"][:, mr.OB + 1:mr.OP:4].astype(F64)
        var = np.maximum((s2 - s1 * s1 / L) / (L - 1), 0.0).astype(F32)
        want, scale = mr.item_variance_ref(p)
        add("bone_var_rigid" if rigid else "bone_var", var, want, scale)
    return w


def test_bound_constants_follow_from_the_fp32_cpu_evaluation():
    w = _ratios()
    for key in sorted(w):
        if key in mr.BOUNDS:
            print(f"[metrics ref] {key}: fp32 CPU worst error / scale {w[key]:.3g} u -> bound {mr.bound_from(w[key]):g} (asserted {mr.BOUNDS[key]:g})")
        else:
            print(f"[metrics ref] {key}: fp32 CPU worst error / scale {w[key]:.3g} u (not asserted on the device: no such output)")
    assert set(mr.BOUNDS) == set(w) - {"pr_joint"}, set(mr.BOUNDS) ^ set(w)
    for key, b in mr.BOUNDS.items():
        assert np.isfinite(w[key]) and b >= 4.0 * w[key] and b >= 1.0, (key, w[key], b)
        assert b <= 10.0 * mr.bound_from(w[key]), (key, w[key], b)          # and no looser than the rule gives, up to a digit

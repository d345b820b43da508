"""Kernel-level tests of the evaluation metrics - the numbers the project reports - each through its C entry point (include/manipose_hip.h):
mp_pose_metrics (pose_metrics_kernel<true,128>, the LDS-staged form taken for two plain contiguous tensors, pose_metrics_kernel<false,256>,
the strided gather form, pose_metrics_finalize_kernel), mp_bone_length_table (bone_length_table_kernel), mp_procrustes_errors
(procrustes_kernel, procrustes_finalize_kernel), and the host arithmetic of manipose_amd/metrics/analytics.py that turns their sums into
metrics (PoseAnalytics.bone_variance, AnalyticsAccumulator.add / add_procrustes / report, keypoint_3d_pck / keypoint_3d_auc, p_mpjpe).

Every entry of every output row is compared with fp64 of the exact fp32 inputs the kernel received (tests/metrics_ref.py: formulas and
scales), against that entry's own forward-error scale: per frame (rows of one or two frames: every batch item is its own workgroup) and per
batch item at the chunk edges of both forms, never one form against the other.  Counts (PCK, AUC, visible joints, frames) are compared for
equality: test_metrics_ref_host.py shows that every error of every case is at least 64 u of its scale away from every threshold (no case is
left out) and that the planted ties are exact in fp32.  Inputs live in storages that are NaN wherever no element lives, outputs start as NaN
(behind them a guard of sentinels that must survive), the scratch has exactly the documented minimum size.

Bound constants (metrics_ref.BOUNDS), in units of u = 2^-24 times the scale.  They are NOT fitted to the kernels: each is 4 x the worst
error / scale of the same formula evaluated in plain fp32 numpy on the CPU over this module's cases (the factor 4: another, equally valid
summation order and FMA contraction), rounded up to one significant digit, never below 1; test_metrics_ref_host.py measures the ratios:
    quantity        fp32 CPU ratio  bound     quantity         fp32 CPU ratio  bound     quantity         fp32 CPU ratio  bound
    err             1.09            5         err_sum          4.69            20        bone_d_rigid     0.274           2
    err2            1.13            5         err2_sum         3.2             20        bone_d2_rigid    0.208           1
    sym             0.592           3         sym_sum          0.316           2         blt              0.901           4
    sym2            0.596           3         sym2_sum         0.32            2         pr_frame         0.474           2
    len_abs         0.759           4         len_abs_sum      0.226           1         pr_sum           0.0128          1
    len_signed      0.759           4         len_signed_sum   0.22            1         bone_var         0.199           1
    vel             0.28            2         vel_sum          0.187           1         bone_var_rigid   0.184           1
    vel2            0.211           1         vel2_sum         0.085           1
    bone_d          0.68            3         bone_d_sum       0.517           3
    bone_d2         0.711           3         bone_d2_sum      0.378           2
    len0            1.1             5         len0_sum         1.05            5
The plain keys are the rows of one or two frames, `_sum` the rows of hundreds of frames (numpy adds the frames of a per-joint column one
after the other: its err_sum is the largest ratio), `_rigid` the shifted variance sums of the rigid sequence at a root offset of 5 m.
pr_frame is the sum of one frame's Procrustes-aligned errors (the larger of Horn's N with Jacobi sweeps run to convergence and of an fp32
SVD), its scale carries the conditioning 1 + lambda_1 / (lambda_1 - lambda_2) of the frame's rotation.
Every test prints its measured worst ratio next to the bound."""
import ctypes as C

import numpy as np
import pytest
import torch

import metrics_ref as mr
from test_gpu_model_ends import ERR_ARG, Buf, check, same_bits
from test_gpu_parity import st

pytestmark = pytest.mark.gpu
NV = mr.NV


class Worst:
    """the worst error / scale ratio of every quantity over the calls of one test; done() prints one line per quantity and asserts the bounds"""

    def __init__(self):
        self.r = {}

    def add(self, key, got, want, scale, what):
        ratio = mr.worst(got, want, scale)
        if key not in self.r or ratio > self.r[key][0]:
            self.r[key] = (ratio, what)

    def done(self, name, bounds=None):
        b = {k: (bounds or {}).get(k, mr.BOUNDS.get(k)) for k in self.r}
        for key, (ratio, what) in sorted(self.r.items()):
            print(f"[metric kernels] {name} {key}: worst error / scale {ratio:.3g} u (asserted <= {b[key]:g})  [{what}]")
        for key, (ratio, what) in self.r.items():
            assert ratio <= b[key], (name, key, what, ratio, b[key])


def cdiv(a, b):
    return (a + b - 1) // b


def host(buf):
    return buf.t.cpu().double().numpy()


class Frames:
    """a (B, L, 17, 3) array on the device in one of metrics_ref.layout's forms: pointer of element (0,0,0,0), element strides"""

    def __init__(self, a, form):
        s, off, strides = mr.layout(a, form)
        self.t = torch.from_numpy(s).cuda()
        self.p = self.t.data_ptr() + 4 * off
        self.s = (C.c_int64 * 4)(*strides)


def run_pm(lib, P, G, mask, B, L, v, short=0, over=()):
    """one mp_pose_metrics call with the scratch of the documented minimum size -> rc, out, len0 (Buf); `over` replaces single arguments"""
    out, len0 = Buf((B, NV)), Buf((B, mr.NB))
    n = max(B, 1) * cdiv(max(L, 1), 128) * NV
    scratch = Buf((n,))
    a = dict(pred=P.p, ps=P.s, gt=G.p if G is not None else None, gs=G.s if G is not None else None, mask=mask.data_ptr() if mask is not None else None,
             B=B, L=L, J=17, psc=v["ps"], gsc=v["gs"], pck=v["pck"], auc_max=v["auc_max"], steps=v["auc_steps"], align=int(v["align"]), out=out.p,
             len0=len0.p, scratch=scratch.p, n=n - short)
    a.update(over)
    rc = lib.mp_pose_metrics(a["pred"], a["ps"], a["gt"], a["gs"], a["mask"], a["B"], a["L"], a["J"], a["psc"], a["gsc"], a["pck"], a["auc_max"],
                             a["steps"], a["align"], a["out"], a["len0"], a["scratch"], a["n"], st())
    torch.cuda.synchronize()
    scratch.ok("pose_metrics scratch")
    return rc, out, len0


_REFS = {}


def pose_ref(name, v):
    """the fp64 rows of a case and variant, computed once"""
    key = (name, mr.vname(v))
    if key not in _REFS:
        c = mr.pose_case(name)
        _REFS[key] = mr.pose_metrics_ref(c["pred"], c["gt"] if v["gt"] else None, c["mask"] if v["mask"] else None, v["ps"], v["gs"], v["pck"],
                                         v["auc_max"], v["auc_steps"], v["align"])
    return _REFS[key]


def check_rows(w, name, rigid, out, len0, ref, has_gt, what):
    got, got0 = host(out), host(len0)
    out.ok(what), len0.ok(what)
    for key in set(mr.SLOT_KEYS) - {"count"}:
        s = [i for i, k in enumerate(mr.SLOT_KEYS) if k == key]
        w.add(mr.row_key(key, name, rigid), got[:, s], ref["row"][:, s], ref["row_scale"][:, s], what)
    w.add(mr.row_key("len0", name), got0, ref["len0"], ref["len0_scale"], what)
    cs = list(mr.COUNT_SLOTS)
    bad = np.argwhere(got[:, cs] != ref["row"][:, cs])
    assert bad.size == 0, f"{what}: counts (PCK, AUC, visible, frames) differ from fp64 at (item, slot) {bad[:5].tolist()}: " \
                          f"{got[:, cs][tuple(bad[0])]} against {ref['row'][:, cs][tuple(bad[0])]}"
    if not has_gt:
        assert not got[:, mr.GT_SLOTS].any(), f"{what}: a target-dependent entry is not 0 without a target"


def forms_of(v, edge):
    """(prediction form, target form) pairs: two plain contiguous tensors take the staged kernel; the same contiguous prediction with the
    target passed through a padded copy, the reference's (B,3,J,L) permutation, and offset / padded storages take the strided one"""
    if not v["gt"]:
        return [("contig", None), ("perm", None), ("pad", None)]
    return [("contig", "contig"), ("contig", "pad"), ("perm", "perm")] + ([] if edge else [("pad", "pad")])


def run_case(lib, name, edge):
    c = mr.pose_case(name)
    B, L = c["pred"].shape[:2]
    w = Worst()
    dev_p = {f: Frames(c["pred"], f) for f in ("contig", "perm", "pad")}
    dev_g = {f: Frames(c["gt"], f) for f in ("contig", "perm", "pad")}
    mask = torch.from_numpy(c["mask"]).cuda()
    for v in c["variants"]:
        ref = pose_ref(name, v)
        for fp, fg in forms_of(v, edge):
            what = f"{name} {mr.vname(v)} pred {fp} gt {fg}"
            a = (lib, dev_p[fp], dev_g[fg] if fg else None, mask if v["mask"] else None, B, L, v)
            rc, out, len0 = run_pm(*a)
            check(lib, rc, "mp_pose_metrics")
            check_rows(w, name, c["rigid"], out, len0, ref, v["gt"], what)
            if edge:
                rc, out2, len02 = run_pm(*a)
                check(lib, rc, "mp_pose_metrics")
                same_bits(out2.ok(what), out.t, what + ": second run")
                same_bits(len02.ok(what), len0.t, what + ": second run, len0")
    w.done(f"mp_pose_metrics {name}")


# ------------------------------------------------------------------------------------------------ mp_pose_metrics
@pytest.mark.parametrize("name", mr.FRAME_CASES)
def test_pose_metrics_rows_of_single_frames_and_frame_pairs(lib, name):
    """L = 1 and L = 2 with B = 70 items: every one of the 122 entries and the 16 len0 values of every row is one frame's (one frame pair's)
    value; both kernel forms, storage offset and padded strides, with and without target, mask and scale alignment, millimetres, metres with
    scales 1000 and metres on the inexact AUC grid 0.15 / 30; `ties`: e == threshold exactly (PCK's strict <, the AUC count 30 - i)"""
    run_case(lib, name, edge=False)


@pytest.mark.parametrize("name", mr.EDGE_CASES)
def test_pose_metrics_chunk_edges(lib, name):
    """L around the 128 frames of a staged and the 256 frames of a strided workgroup, B = 1 and 3 with a mask of its own for every item; the
    staged and the strided form of the same contiguous data each against fp64; the same bits in two runs"""
    run_case(lib, name, edge=True)


# ------------------------------------------------------------------------------------------------ mp_bone_length_table
@pytest.mark.parametrize("B,L", [(1, 1), (3, 85), (1, 256), (257, 1)])
def test_bone_length_table_per_element(lib, B, L):
    pred, gt = mr.skeleton_frames((B, L), 5000 + B * L)
    w = Worst()
    for fp, fg in (("contig", "contig"), ("perm", "perm"), ("pad", "contig")):
        P, G = Frames(pred, fp), Frames(gt, fg)
        for signed in (0, 1):
            what = f"B={B} L={L} pred {fp} gt {fg} signed={signed}"
            out = Buf((B * L, mr.NB))
            check(lib, lib.mp_bone_length_table(P.p, P.s, G.p, G.s, B, L, signed, out.p, st()), "mp_bone_length_table")
            torch.cuda.synchronize()
            want, scale = mr.bone_table_ref(pred, gt, signed)
            got = host(out)
            out.ok(what)
            w.add("blt", got, want, scale, what)
            assert signed or (got >= 0).all()
    w.done("mp_bone_length_table")


# ------------------------------------------------------------------------------------------------ mp_procrustes_errors
def run_pr(lib, pred, gt, mask, N, v, short=0, over=()):
    out = Buf((5,))
    n = 5 * cdiv(max(N, 1), 256)
    scratch = Buf((n,))
    a = dict(pred=pred.data_ptr(), gt=gt.data_ptr(), mask=mask.data_ptr() if mask is not None else None, N=N, J=17, psc=v["ps"], gsc=v["gs"],
             pck=v["pck"], auc_max=v["auc_max"], steps=v["auc_steps"], out=out.p, scratch=scratch.p, n=n - short)
    a.update(over)
    rc = lib.mp_procrustes_errors(a["pred"], a["gt"], a["mask"], a["N"], a["J"], a["psc"], a["gsc"], a["pck"], a["auc_max"], a["steps"], a["out"],
                                  a["scratch"], a["n"], st())
    torch.cuda.synchronize()
    scratch.ok("procrustes scratch")
    return rc, out


def test_procrustes_named_single_frames(lib):
    """N = 1 calls: out[0] is the frame's sum of aligned errors, within the frame's conditioned scale; out[1..4] are counts.  Generic frames,
    similar copies (error ~ 0: the absolute floor of the scale), mirror images (the reflection fix), planar and collinear sets, a pose 5 m
    from the origin, predictions 100 x too small / large, metres with scales 1000, frames of the `metrics` fixture"""
    w = Worst()
    for s in mr.procrustes_specials():
        pred, gt = torch.from_numpy(s["pred"]).cuda(), torch.from_numpy(s["gt"]).cuda()
        for thr in (150.0, 80.0):
            v = mr.variant(pck=thr, ps=s["ps"], gs=s["gs"])
            what = f"{s['name']} pck={thr:g}"
            rc, out = run_pr(lib, pred, gt, None, 1, v)
            check(lib, rc, "mp_procrustes_errors")
            r = mr.procrustes_ref(s["pred"], s["gt"], None, s["ps"], s["gs"], thr, axis_free=s["axis_free"])
            got = host(out)
            out.ok(what)
            w.add("pr_frame", got[0], r["out"][0], r["out_scale"], what)
            assert np.array_equal(got[1:], r["out"][1:]), f"{what}: counts {got[1:]} against {r['out'][1:]}"
    w.done("mp_procrustes_errors N=1")


@pytest.mark.parametrize("N", mr.PROC_N)
def test_procrustes_sums(lib, N):
    """N around the 256 frames of a workgroup, with and without a mask; frames 255, 256 and the last one carry a distinctly larger error;
    the mask changes only slots 1 - 3; the same bits in two runs"""
    c = mr.procrustes_case(N)
    pred, gt, mask = torch.from_numpy(c["pred"]).cuda(), torch.from_numpy(c["gt"]).cuda(), torch.from_numpy(c["mask"]).cuda()
    w = Worst()
    for v in mr.PROC_VARIANTS:
        outs = []
        for m, mh in ((None, None), (mask, c["mask"])):
            what = f"N={N} pck={v['pck']:g} mask={int(m is not None)}"
            rc, out = run_pr(lib, pred, gt, m, N, v)
            check(lib, rc, "mp_procrustes_errors")
            r = mr.procrustes_ref(c["pred"], c["gt"], mh, pck_thr=v["pck"])
            got = host(out)
            out.ok(what)
            w.add("pr_frame" if N == 1 else "pr_sum", got[0], r["out"][0], r["out_scale"], what)
            assert np.array_equal(got[1:], r["out"][1:]), f"{what}: counts {got[1:]} against {r['out'][1:]}"
            rc, out2 = run_pr(lib, pred, gt, m, N, v)
            same_bits(out2.ok(what), out.t, what + ": second run")
            outs.append(out)
        same_bits(outs[0].t[[0, 4]], outs[1].t[[0, 4]], f"N={N}: the mask changed the error sum or the frame count")
    w.done(f"mp_procrustes_errors N={N}")


# ------------------------------------------------------------------------------------------------ the host arithmetic
def test_accumulator_report_and_metric_functions_against_the_concatenated_frames(lib):
    """pose_analytics + AnalyticsAccumulator.add over three unequal batches (one of them rigid), add_procrustes, report(): every metric
    against fp64 of the concatenated frames (the variance of the concatenated sequence, not re-centred sums), bounds from the row bounds;
    bone_variance per item; keypoint_3d_pck / keypoint_3d_auc / p_mpjpe: the counts are those of fp64"""
    from manipose_amd.metrics import keypoint_3d_auc, keypoint_3d_pck, p_mpjpe
    from manipose_amd.metrics.analytics import AnalyticsAccumulator, pose_analytics, procrustes_sums
    batches = mr.report_case()
    acc, w = AnalyticsAccumulator(), Worst()
    for (p, g), (_, _, rigid) in zip(batches, mr.REPORT_BATCHES):
        pd, gd = torch.from_numpy(p).cuda(), torch.from_numpy(g).cuda()
        a = pose_analytics(pd, gd)
        acc.add(a)
        acc.add_procrustes(procrustes_sums(pd, gd))
        want, scale = mr.item_variance_ref(p)
        w.add("bone_var_rigid" if rigid else "bone_var", a.bone_variance().cpu().double().numpy(), want, scale, f"bone_variance rigid={int(rigid)}")
    rep, ref = acc.report(), mr.report_ref(batches)
    var_bound = max(mr.BOUNDS[k] for k in ("bone_d_sum", "bone_d2_sum", "bone_d_rigid", "bone_d2_rigid", "bone_var", "bone_var_rigid"))
    bounds = {}
    for name, (val, scale, key) in ref.items():
        if key == "count":
            assert abs(rep[name] - val) <= 1e-9, (name, rep[name], val)
            continue
        bounds[name] = var_bound if name.startswith("mpsce") else mr.BOUNDS[key if key.startswith("pr_") else key + "_sum"]
        w.add(name, np.asarray(rep[name], dtype=np.float64), val, scale, "report()")
    w.done("manipose_amd.metrics", bounds)
    # the reference-named functions, with a mask, on the frames of the first batch
    p, g = batches[0]
    n = p.shape[0] * p.shape[1]
    pf, gf = torch.from_numpy(p).cuda().reshape(n, 17, 3), torch.from_numpy(g).cuda().reshape(n, 17, 3)
    mask = mr.case_mask(1, n, 77)
    for al in ("none", "scale", "procrustes"):
        for thr in (150.0, 80.0):
            if al == "procrustes":
                r = mr.procrustes_ref(p.reshape(n, 17, 3), g.reshape(n, 17, 3), mask[0], pck_thr=thr)["out"]
                pck, auc = 100.0 * r[1] / r[3], 100.0 * r[2] / (31 * r[3])
            else:
                r = mr.pose_metrics_ref(p.reshape(1, n, 17, 3), g.reshape(1, n, 17, 3), mask, pck_thr=thr, scale_align=(al == "scale"))["row"][0]
                pck, auc = 100.0 * r[6] / r[8], 100.0 * r[7] / (31 * r[8])
            got = keypoint_3d_pck(pf, gf, mask[0], al, thr)
            assert abs(got - pck) <= 1e-9, (al, thr, got, pck)
        got = keypoint_3d_auc(pf, gf, mask[0], al)
        assert abs(got - auc) <= 1e-9, (al, got, auc)
    r = mr.procrustes_ref(p.reshape(n, 17, 3), g.reshape(n, 17, 3), None)
    got = p_mpjpe(torch.from_numpy(p).cuda(), torch.from_numpy(g).cuda())
    ratio = mr.worst(np.float64(got), r["out"][0] / (n * 17), r["out_scale"] / (n * 17))
    print(f"[metric kernels] p_mpjpe: worst error / scale {ratio:.3g} u (asserted <= {mr.BOUNDS['pr_sum']:g})")
    assert ratio <= mr.BOUNDS["pr_sum"]


def test_report_divides_the_auc_counts_by_the_steps_of_its_grid(lib):
    """an accumulator fed with another AUC grid than the default reports the mean over THAT grid's thresholds"""
    from manipose_amd.metrics.analytics import AnalyticsAccumulator, pose_analytics, procrustes_sums
    p, g = mr.report_case()[0]
    pd, gd = torch.from_numpy(p).cuda(), torch.from_numpy(g).cuda()
    acc = AnalyticsAccumulator(auc_steps=16)                       # 150 / 15 = 10 mm: a subset of the default grid, the margins hold
    acc.add(pose_analytics(pd, gd, auc_max=150.0, auc_steps=16))
    acc.add_procrustes(procrustes_sums(pd, gd, auc_max=150.0, auc_steps=16))
    ref = mr.report_ref([(p, g)], auc_steps=16)
    rep = acc.report()
    for k in ("auc", "auc_procrustes", "pck"):
        assert abs(rep[k] - ref[k][0]) <= 1e-9, (k, rep[k], ref[k][0])


# ------------------------------------------------------------------------------------------------ refusals
def test_pose_metrics_refusals_leave_every_output_untouched(lib):
    """every MP_CHECK of mp_pose_metrics and its launcher, each before any launch"""
    B, L = 2, 130
    pred, gt = mr.skeleton_frames((B, L), 6000)
    v = mr.variant()
    Pc, Gc, Gp = Frames(pred, "contig"), Frames(gt, "contig"), Frames(gt, "pad")
    # the launcher needs B ceil(L / 128) rows for the staged form and B ceil(L / 256) for the strided one: one float less than that is refused
    strided_short = B * cdiv(L, 128) * NV - B * cdiv(L, 256) * NV + 1
    bad = [dict(pred=None), dict(ps=None), dict(out=None), dict(len0=None), dict(scratch=None), dict(J=16), dict(J=18), dict(B=0), dict(B=-1),
           dict(L=0), dict(L=-3), dict(gs=None), dict(steps=1), dict(steps=0), dict(auc_max=0.0), dict(auc_max=-150.0), dict(short=1),
           dict(short=strided_short, G=Gp)]
    for kw in bad:
        kw = dict(kw)
        G = kw.pop("G", Gc)
        rc, out, len0 = run_pm(lib, Pc, G, None, B, L, v, short=kw.pop("short", 0), over=kw)
        assert rc == ERR_ARG and lib.mp_last_error(), kw
        if "out" not in kw:
            out.untouched(None, f"{kw}: out")
        if "len0" not in kw:
            len0.untouched(None, f"{kw}: len0")
    rc, out, len0 = run_pm(lib, Pc, Gp, None, B, L, v, short=strided_short - 1)       # the strided form with exactly its rows: accepted
    check(lib, rc, "mp_pose_metrics, strided form, exact scratch")
    assert lib.mp_pose_metrics_row_floats() == NV


def test_bone_length_table_and_procrustes_refusals_leave_every_output_untouched(lib):
    B, L = 2, 5
    pred, gt = mr.skeleton_frames((B, L), 6001)
    P, G = Frames(pred, "contig"), Frames(gt, "contig")
    for kw in (dict(pred=None), dict(ps=None), dict(gt=None), dict(gs=None), dict(out=None), dict(B=0), dict(L=0), dict(B=-2)):
        out = Buf((B * L, mr.NB))
        a = dict(pred=P.p, ps=P.s, gt=G.p, gs=G.s, B=B, L=L, out=out.p)
        a.update(kw)
        rc = lib.mp_bone_length_table(a["pred"], a["ps"], a["gt"], a["gs"], a["B"], a["L"], 1, a["out"], st())
        torch.cuda.synchronize()
        assert rc == ERR_ARG and lib.mp_last_error(), kw
        out.untouched(None, f"{kw}: table")
    N = 300
    p, g = (torch.from_numpy(a).cuda() for a in mr.skeleton_frames((N,), 6002))
    for kw in (dict(pred=None), dict(gt=None), dict(out=None), dict(scratch=None), dict(J=16), dict(N=0), dict(N=-1), dict(steps=1),
               dict(auc_max=0.0), dict(short=1)):
        kw = dict(kw)
        rc, out = run_pr(lib, p, g, None, N, mr.variant(), short=kw.pop("short", 0), over=kw)
        assert rc == ERR_ARG and lib.mp_last_error(), kw
        if "out" not in kw:
            out.untouched(None, f"{kw}: sums")

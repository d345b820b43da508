"""Kernel-level tests of what ends every training step and every evaluation, each through its C entry point (include/manipose_hip.h):
mp_wta_loss and mp_single_loss (wta_loss_kernel in both of its forms - 48 and 256 frames per workgroup, chosen by the scratch size - and
loss_finalize_kernel), mp_rigid_segments_loss (rigid_segments_kernel, rigid_finalize_kernel), mp_aggregate, mp_mpjpe_sum
(mpjpe_partial_kernel's grid-stride loop, the four-trip finalize) and mp_adam_step / mp_adam_step_scaled (adam_kernel<false / true>, the
float4 body and the scalar tail).

Every value is compared PER ELEMENT with fp64 of the exact fp32 inputs the kernel received, against that element's own forward-error scale
(tests/loss_ref.py: formulas and scales), never against a tensor-wide maximum and never against another form of the same kernel: a wrong
neighbour frame, a wrong sign at the last frame of a window, a winner taken from another lane group or a swapped beta cannot hide.  Inputs
come from seeded generators, outputs start as NaN (behind them a guard of sentinels that must survive), the rigid-segments gradient is
accumulated into a non-zero seed.  The winner of every frame is the fp64 winner: test_loss_ref_host.py shows that best and second best are
at least 64 u apart on every frame of every case (no frame is excluded); planted exact ties take the lowest index.

Bound constants (loss_ref.BOUNDS), in units of u = 2^-24 times the scale.  They are NOT fitted to the kernels: each is 4 x the worst
error / scale of the same formula evaluated in plain fp32 torch on the CPU over this module's cases (the factor 4: another, equally valid
summation order and FMA contraction), rounded up to one significant digit, never below 1; test_loss_ref_host.py measures the ratios:
    quantity             fp32 CPU ratio   bound        quantity             fp32 CPU ratio   bound
    wta_wloss            0.415            2            single_d_poses       0.917            4
    wta_score_reg        0.919            4            rigid_term           0.379            2
    wta_vloss            0.121            1            rigid_term_rigid     1120             5000
    wta_sreg             0.505            3            rigid_d_poses        1.89             8
    wta_d_poses          1.09             5            agg_weighted_ave     1.74             7
    wta_d_scores         1.14             5            mpjpe_sum            0.397            2
    single_wloss         0.56             3            adam_p               0.749            3
    single_vloss         0.102            1            adam_m               0.923            4
    single_sreg          0.191            1            adam_v               0.968            4
rigid_term_rigid is the term of the cases made of one rigid window (T = 255, 256, 257): its variance is all cancellation, the scale carries
the cancellation of the sums but not the roundings of the lengths, which the constant therefore carries (loss_ref.py, "rigid").
The BCE quantities carry no allowance for the device's logf: none was needed.  Every test prints its measured worst ratio next to the bound."""
import ctypes as C

import pytest
import torch

import loss_ref as lr
from test_gpu_model_ends import ERR_ARG, Buf, bits, check, dev, same_bits
from test_gpu_parity import st

pytestmark = pytest.mark.gpu


class Worst:
    """the worst error / scale ratio of every quantity over the calls of one test; done() prints one line per quantity and asserts the bounds"""

    def __init__(self):
        self.r = {}

    def add(self, key, got, ref, what):
        ratio = lr.worst(got, ref[0], ref[1])
        if key not in self.r or ratio > self.r[key][0]:
            self.r[key] = (ratio, what)

    def done(self, name):
        for key, (ratio, what) in self.r.items():
            print(f"[loss kernels] {name} {key}: worst error / scale {ratio:.3g} u (asserted <= {lr.BOUNDS[key]:g})  [{what}]")
        for key, (ratio, what) in self.r.items():
            assert ratio <= lr.BOUNDS[key], (name, key, what, ratio, lr.BOUNDS[key])


def loss_config(cfg, w_loss=None):
    from manipose_amd import _lib
    c = _lib.LossConfig(rmcl_score_reg=cfg["beta"], vel_loss=cfg["vel"], smooth_reg=cfg["smooth"], w_loss=cfg["w_loss"] if w_loss is None else w_loss,
                        sq_loss=int(cfg["squared"]))
    for j, w in enumerate(lr.CUSTOM_W):
        c.joint_weights[j] = w
    return c


def cdiv(a, b):
    return (a + b - 1) // b


def forms(frames):
    """(frames per workgroup, scratch floats) of the forms wta_loss_kernel can take at this frame count: the ABI's minimum scratch gives 256
    frames per workgroup, 4 ceil(frames / 48) floats give 48; up to 48 frames the two sizes are the same 4 floats and only the 48 form exists"""
    return [(48, 4 * cdiv(frames, 48))] + ([(256, 4 * cdiv(frames, 256))] if frames > 48 else [])


# ------------------------------------------------------------------------------------------------ mp_wta_loss
def run_wta(lib, dv, cfg, B, K, T, nscratch, want=(True, True, True), scratch_floats=None, scores=True, w_loss=None):
    """-> rc, terms, argmin, d_poses, d_scores (Buf; an output not wanted is passed as null and stays NaN)"""
    terms, am, dp, ds = Buf((4,)), Buf((B, T)), Buf((B, K, T, 17, 3)), Buf((B, K, T))
    scratch = Buf((nscratch,))
    c = loss_config(cfg, w_loss)
    rc = lib.mp_wta_loss(dv["poses"].data_ptr(), dv["scores"].data_ptr() if scores else None, dv["y"].data_ptr(), C.byref(c), terms.p,
                         am.p if want[0] else None, dp.p if want[1] else None, ds.p if want[2] else None, B, K, T, scratch.p,
                         nscratch if scratch_floats is None else scratch_floats, st())
    torch.cuda.synchronize()
    scratch.ok("wta scratch")
    return rc, terms, am, dp, ds


@pytest.mark.parametrize("B,K,T,modes", lr.WTA_CASES, ids=[f"B{c[0]}K{c[1]}T{c[2]}" for c in lr.WTA_CASES])
def test_wta_loss_terms_argmin_and_gradients_per_element(lib, B, K, T, modes):
    """both forms of the kernel, each against fp64: argmin on every frame, d_poses and d_scores per element, the four terms; a null argmin,
    d_poses or d_scores leaves the other outputs bit-identical"""
    d = lr.wta_case_inputs(B, K, T)
    dv = {k: dev(d[k]) for k in ("poses", "scores", "y")}
    w = Worst()
    for w_loss, squared in modes:
        cfg = lr.loss_cfg(w_loss, squared)
        ref = lr.wta_loss(d["poses"], d["scores"], d["y"], cfg)
        for fpb, n in forms(B * T):
            what = f"B={B} K={K} T={T} w_loss={w_loss} squared={int(squared)} fpb={fpb}"
            rc, terms, am, dp, ds = run_wta(lib, dv, cfg, B, K, T, n)
            check(lib, rc, "mp_wta_loss")
            got_am = bits(am.ok(what)).cpu().long()
            wrong = int((got_am != ref["argmin"]).sum())
            assert wrong == 0, f"{what}: argmin differs from fp64 on {wrong} frames"
            if d["tie"] is not None:
                assert bool((got_am[d["tie"]] == 1).all()), f"{what}: a planted tie of hypotheses 1 and 3 did not take index 1"
            w.add("wta_d_poses", dp.ok(what), ref["d_poses"], what)
            w.add("wta_d_scores", ds.ok(what), ref["d_scores"], what)
            t = terms.ok(what).cpu()
            for i, k in enumerate(lr.WTA_TERMS):
                w.add("wta_" + k, t[i], ref[k], what)
            for skip in range(3):
                want = tuple(i != skip for i in range(3))
                rc, terms2, am2, dp2, ds2 = run_wta(lib, dv, cfg, B, K, T, n, want=want)
                check(lib, rc, "mp_wta_loss with a null output")
                same_bits(terms2.ok(what), terms.t, f"{what}: terms, output {skip} null")
                for i, (a, b) in enumerate(((am2, am), (dp2, dp), (ds2, ds))):
                    if want[i]:
                        same_bits(a.ok(what), b.t, f"{what}: output {i}, output {skip} null")
                    else:
                        a.untouched(None, f"{what}: null output {i}")
    w.done("mp_wta_loss")


def test_wta_loss_refusals_leave_every_output_untouched(lib):
    B, K, T = 2, 5, 7
    cfg = lr.loss_cfg(1, False)
    bad = [dict(K=9), dict(T=1), dict(short=1), dict(w_loss=3), dict(scores=False)]
    for kw in bad:
        b, k, t = B, kw.get("K", K), kw.get("T", T)
        d = lr.wta_inputs(b, k, max(t, 2), 3)                                        # (buffers that would hold the call if it were let through)
        dv = {n: dev(d[n]) for n in ("poses", "scores", "y")}
        n = 4 * cdiv(b * t, 256)
        rc, terms, am, dp, ds = run_wta(lib, dv, cfg, b, k, t, n, scratch_floats=n - kw.get("short", 0), scores=kw.get("scores", True),
                                        w_loss=kw.get("w_loss"))
        assert rc == ERR_ARG and lib.mp_last_error(), kw
        for o, name in ((terms, "terms"), (am, "argmin"), (dp, "d_poses"), (ds, "d_scores")):
            o.untouched(None, f"{kw}: {name}")


# ------------------------------------------------------------------------------------------------ mp_single_loss
def run_single(lib, dv, cfg, B, T, nscratch, with_grad=True):
    terms, dp, scratch = Buf((3,)), Buf((B, T, 17, 3)), Buf((nscratch,))
    c = loss_config(cfg)
    rc = lib.mp_single_loss(dv["poses"].data_ptr(), dv["y"].data_ptr(), C.byref(c), terms.p, dp.p if with_grad else None, B, T, scratch.p, nscratch, st())
    torch.cuda.synchronize()
    scratch.ok("single scratch")
    return rc, terms, dp


@pytest.mark.parametrize("B,T", lr.SINGLE_CASES)
def test_single_loss_terms_and_gradient_per_element(lib, B, T):
    """three terms in the order wloss, vloss, sreg; with d_poses null the terms keep their bits"""
    d = lr.single_case_inputs(B, T)
    dv = {k: dev(d[k]) for k in ("poses", "y")}
    w = Worst()
    for squared in (False, True):
        cfg = lr.loss_cfg(1, squared)
        ref = lr.wta_loss(d["poses"][:, None], None, d["y"], cfg)
        for fpb, n in forms(B * T):
            what = f"B={B} T={T} squared={int(squared)} fpb={fpb}"
            rc, terms, dp = run_single(lib, dv, cfg, B, T, n)
            check(lib, rc, "mp_single_loss")
            w.add("single_d_poses", dp.ok(what), (ref["d_poses"][0][:, 0], ref["d_poses"][1][:, 0]), what)
            t = terms.ok(what).cpu()
            for i, k in enumerate(lr.SINGLE_TERMS):
                w.add("single_" + k, t[i], ref[k], what)
            rc, terms2, dp2 = run_single(lib, dv, cfg, B, T, n, with_grad=False)
            check(lib, rc, "mp_single_loss without d_poses")
            same_bits(terms2.ok(what), terms.t, f"{what}: terms without d_poses")
            dp2.untouched(None, f"{what}: null d_poses")
    w.done("mp_single_loss")


# ------------------------------------------------------------------------------------------------ mp_rigid_segments_loss
def run_rigid(lib, poses, weight, seed, B, T, with_grad=True, scratch_floats=None):
    term, dp, scratch = Buf((1,)), Buf((B, T, 17, 3), seed), Buf((B,))
    rc = lib.mp_rigid_segments_loss(poses.data_ptr(), weight, term.p, dp.p if with_grad else None, B, T, scratch.p,
                                    B if scratch_floats is None else scratch_floats, st())
    torch.cuda.synchronize()
    scratch.ok("rigid scratch")
    return rc, term, dp


@pytest.mark.parametrize("B,T", lr.RIGID_CASES)
def test_rigid_segments_term_and_accumulated_gradient_per_element(lib, B, T):
    """T around the 256 threads of a workgroup (the frame loop's second trip from 257 on), B = 257 windows (the finalize loop's second trip);
    rigid windows whose variance is nearly all cancellation, a bone of length exactly 0, an exactly constant window; the gradient is added
    to a non-zero seed; with d_poses null the term keeps its bits"""
    d = lr.rigid_case_inputs(B, T)
    what = f"B={B} T={T}"
    poses = dev(d["poses"])
    w = Worst()
    rc, term, dp = run_rigid(lib, poses, d["weight"], d["seed"], B, T)
    check(lib, rc, "mp_rigid_segments_loss")
    ref = lr.rigid_segments(d["poses"], d["weight"], d["seed"])
    w.add(lr.rigid_term_key(B, T), term.ok(what)[0], ref[0], what)
    w.add("rigid_d_poses", dp.ok(what), ref[1], what)
    rc, term2, dp2 = run_rigid(lib, poses, d["weight"], d["seed"], B, T, with_grad=False)
    check(lib, rc, "mp_rigid_segments_loss without d_poses")
    same_bits(term2.ok(what), term.t, f"{what}: term without d_poses")
    dp2.untouched(d["seed"], f"{what}: null d_poses")
    if (B, T) == (2, 3):      # the exactly constant window on its own: the variance is exactly 0 (the scale is 0: any other value fails)
        rc, term3, dp3 = run_rigid(lib, poses[1:].contiguous(), d["weight"], d["seed"][1:], 1, T)
        check(lib, rc, "mp_rigid_segments_loss, constant window")
        ref3 = lr.rigid_segments(d["poses"][1:], d["weight"], d["seed"][1:])
        assert float(ref3[0][1]) == 0.0
        w.add("rigid_term", term3.ok(what)[0], ref3[0], what + " constant window")
        w.add("rigid_d_poses", dp3.ok(what), ref3[1], what + " constant window")
    w.done("mp_rigid_segments_loss")


def test_rigid_segments_refusals(lib):
    d = lr.rigid_inputs(3, 4, 5)
    poses = dev(d["poses"])
    for T, nscratch in ((1, 3), (4, 2)):
        rc, term, dp = run_rigid(lib, poses, d["weight"], d["seed"], 3, T, scratch_floats=nscratch) if T == 4 else \
            run_rigid(lib, poses, d["weight"], d["seed"][:, :1], 3, 1)
        assert rc == ERR_ARG and lib.mp_last_error(), (T, nscratch)
        term.untouched(None, "term")
        dp.untouched(d["seed"] if T == 4 else d["seed"][:, :1], "d_poses")


# ------------------------------------------------------------------------------------------------ mp_aggregate
def run_aggregate(lib, dv, mode, B, K, T, scores=True, target=True):
    out = Buf((B, T, 17, 3))
    rc = lib.mp_aggregate(dv["poses"].data_ptr(), dv["scores"].data_ptr() if scores else None, dv["y"].data_ptr() if target else None, mode, out.p,
                          B, K, T, st())
    torch.cuda.synchronize()
    return rc, out


@pytest.mark.parametrize("B,T", lr.AGG_BT)
def test_aggregate_three_modes(lib, B, T):
    """weighted_ave per element; best_score and oracle: the output row is a bit-exact copy of the hypothesis fp64 picks (equal top scores and
    duplicated best hypotheses: the lowest index), and of no other hypothesis unless that one carries the same bits"""
    w = Worst()
    for K in lr.AGG_K:
        what = f"B={B} K={K} T={T}"
        d = lr.agg_case_inputs(B, K, T)
        dv = {k: dev(d[k]) for k in ("poses", "scores", "y")}
        rc, out = run_aggregate(lib, dv, 0, B, K, T, target=False)
        check(lib, rc, "mp_aggregate weighted_ave")
        w.add("agg_weighted_ave", out.ok(what), lr.aggregate(d["poses"], d["scores"], d["y"], 0), what)
        for mode, name, need in ((1, "best_score", dict(target=False)), (2, "oracle", dict(scores=False))):
            rc, out = run_aggregate(lib, dv, mode, B, K, T, **need)
            check(lib, rc, "mp_aggregate " + name)
            idx = lr.aggregate(d["poses"], d["scores"], d["y"], mode)[0]
            got = bits(out.ok(what).cpu())                                                     # (B, T, 17, 3)
            match = (bits(d["poses"]) == got[:, None]).all(-1).all(-1)                         # (B, K, T): hypotheses the output row equals bit for bit
            assert bool(match.any(1).all()), f"{what} {name}: an output row is no hypothesis of its frame"
            # the recovered index: the hypothesis fp64 picks where the row carries its bits (a planted duplicate carries them too), else the first match
            first = torch.where(match.gather(1, idx[:, None])[:, 0], idx, match.float().argmax(1))
            wrong = int((first != idx).sum())
            assert wrong == 0, f"{what} {name}: {wrong} frames carry another hypothesis than fp64 picks"
            assert bool((match.sum(1) == 1)[~d["tie_p"]].all()), f"{what} {name}: two hypotheses with the same bits outside the planted frames"
        if K >= 5:
            assert bool((lr.aggregate(d["poses"], d["scores"], d["y"], 1)[0][d["tie_s"]] == 1).all())
    w.done("mp_aggregate")


def test_aggregate_refusals(lib):
    B, K, T = 2, 5, 7
    d = lr.agg_case_inputs(B, K, T)
    dv = {k: dev(d[k]) for k in ("poses", "scores", "y")}
    for mode, need in ((3, {}), (-1, {}), (2, dict(target=False)), (0, dict(scores=False)), (1, dict(scores=False))):
        rc, out = run_aggregate(lib, dv, mode, B, K, T, **need)
        assert rc == ERR_ARG and lib.mp_last_error(), (mode, need)
        out.untouched(None, f"mode {mode} {need}")


# ------------------------------------------------------------------------------------------------ mp_mpjpe_sum
def mpjpe_scratch(n):
    return 4 * min(cdiv(n, 256), 1024) + 4


@pytest.mark.parametrize("n", lr.MPJPE_N)
def test_mpjpe_sum(lib, n):
    """1024 * 256 + 257 joints: the grid-stride loop of mpjpe_partial_kernel runs a second time and loss_finalize_kernel four times"""
    d = lr.mpjpe_case_inputs(n)
    pred, gt = dev(d["pred"]), dev(d["gt"])
    out, scratch = Buf((1,)), Buf((mpjpe_scratch(n),))
    check(lib, lib.mp_mpjpe_sum(pred.data_ptr(), gt.data_ptr(), n, out.p, scratch.p, mpjpe_scratch(n), st()), "mp_mpjpe_sum")
    torch.cuda.synchronize()
    scratch.ok("mpjpe scratch")
    w = Worst()
    w.add("mpjpe_sum", out.ok("sum")[0], lr.mpjpe_sum(d["pred"], d["gt"]), f"n={n}")
    w.done("mp_mpjpe_sum")
    out2 = Buf((1,))
    assert lib.mp_mpjpe_sum(pred.data_ptr(), gt.data_ptr(), n, out2.p, scratch.p, mpjpe_scratch(n) - 1, st()) == ERR_ARG
    torch.cuda.synchronize()
    out2.untouched(None, "sum of a refused call")


# ------------------------------------------------------------------------------------------------ mp_adam_step, mp_adam_step_scaled
def run_adam(lib, d, g_dev, step, wd, gscale, mults=None, lr_null=False, wd_null=False):
    """-> rc, p, m, v (Buf, updated in place); mults: None = mp_adam_step, (lr_mult, wd_mult) device tensors = mp_adam_step_scaled"""
    h = lr.ADAM_HYPER
    n = d["p"].numel()
    p, m, v = Buf((n,), d["p"]), Buf((n,), d["m"]), Buf((n,), d["v"])
    a = (p.p, g_dev.data_ptr(), m.p, v.p, n, step, h["lr"], h["beta1"], h["beta2"], h["eps"], wd, gscale)
    if mults is None:
        rc = lib.mp_adam_step(*a, st())
    else:
        rc = lib.mp_adam_step_scaled(*a, None if lr_null else mults[0].data_ptr(), None if wd_null else mults[1].data_ptr(), st())
    torch.cuda.synchronize()
    return rc, p, m, v


@pytest.mark.parametrize("n", lr.ADAM_N)
def test_adam_step_p_m_v_per_element(lib, n):
    """the float4 body and the scalar tail (n % 4 != 0, n < 4), steps 1 .. 100000 (the bias corrections), non-zero moments, weight decay, a
    gradient scale, and the multiplier form with multipliers that include 0 and with all multipliers 1 - each against fp64"""
    w = Worst()
    ones = torch.ones(n, device="cuda")
    for step in lr.ADAM_STEPS:
        d = lr.adam_case_inputs(n, step)
        g_dev, lm, wm = dev(d["g"]), dev(d["lr_mult"]), dev(d["wd_mult"])
        for wd, gs in lr.ADAM_WD_GS:
            for form, mults, kw in (("plain", None, {}), ("scaled", (lm, wm), dict(lr_mult=d["lr_mult"], wd_mult=d["wd_mult"])), ("scaled by 1", (ones, ones), {})):
                what = f"n={n} step={step} wd={wd:g} grad_scale={gs:g} {form}"
                rc, p, m, v = run_adam(lib, d, g_dev, step, wd, gs, mults)
                check(lib, rc, "mp_adam_step " + form)
                ref = lr.adam(*lr.adam_args(d, step, wd, gs), **kw)
                for k, buf, r in zip("pmv", (p, m, v), ref):
                    w.add("adam_" + k, buf.ok(f"{what}: {k}"), r, what)
    w.done("mp_adam_step")


def test_adam_refusals(lib):
    n, step = 5, 3
    d = lr.adam_case_inputs(n, step)
    g_dev, lm, wm = dev(d["g"]), dev(d["lr_mult"]), dev(d["wd_mult"])
    for kw in (dict(step=0), dict(step=0, mults=(lm, wm)), dict(mults=(lm, wm), lr_null=True), dict(mults=(lm, wm), wd_null=True)):
        rc, p, m, v = run_adam(lib, d, g_dev, kw.pop("step", step), 0.0, 1.0, **kw)
        assert rc == ERR_ARG and lib.mp_last_error(), kw
        for k, buf in zip("pmv", (p, m, v)):
            buf.untouched(d[k], f"{kw}: {k}")

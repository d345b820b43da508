"""The fp64 references of tests/loss_ref.py, verified without a GPU: they agree with the oracle (oracle/manipose_ref.py) evaluated in fp64 on
the same inputs to 1e-12 relative - values directly, the hand-written gradients against the oracle's autograd -, they reproduce the fixtures
loss.npz and loss_sq.npz, every input case keeps the winner margin (gap >= 64 u on every frame, no frame excluded), and the bound constants
test_gpu_loss_kernels.py asserts follow from the error of the same formulas evaluated in plain fp32 torch on the CPU (ends_ref.bound_from:
4 x the worst error / scale ratio over the GPU module's cases, rounded up to one significant digit, never below 1)."""
import os
import sys

import numpy as np
import pytest
import torch

import loss_ref as lr
from helpers import load_fixture

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import manipose_ref as orc  # noqa: E402

F32, F64 = torch.float32, torch.float64


def close(a, b, what, tol=1e-12):
    a, b = torch.as_tensor(a, dtype=F64), torch.as_tensor(b, dtype=F64)
    err = (a - b).abs().max().item()
    ref = b.abs().max().item()
    assert err <= tol * max(ref, 1e-300), f"{what}: {err:.3g} against {ref:.3g}"


def test_tables_match_the_oracle():
    assert lr.H36M_W == [float(w) for w in orc.STANDARD_H36M_WEIGHTS]
    assert list(zip(lr.BONE_J, lr.BONE_P)) == [tuple(b) for b in orc.H36M_BONES]


def _oracle_terms(p, s, y, cfg):
    """the four terms assembled from the oracle's loss functions, as rmcl_training_loss does, with any joint weights"""
    w = None if cfg["w_loss"] == 0 else lr.joint_weights(cfg).double()
    sq = cfg["squared"]
    return dict(wloss=orc.wta_l2_loss_and_activate_head(p, y, w, sq)[0].mean(), score_reg=orc.wta_with_scoring_loss(p, s, y, cfg["beta"], w, sq)[1],
                vloss=cfg["vel"] * orc.mean_velocity_error(p, y, axis=2, squared=sq), sreg=cfg["smooth"] * orc.smoothness_regularization(p, w, axis=2))


# ------------------------------------------------------------------------------------------------ against the oracle, fp64
@pytest.mark.parametrize("B,K,T", [(2, 5, 7), (1, 8, 49), (3, 1, 2)])
@pytest.mark.parametrize("w_loss,squared", lr.ALL_MODES)
def test_wta_loss_matches_the_oracle_and_its_autograd(B, K, T, w_loss, squared):
    d = lr.wta_inputs(B, K, T, 5 + B + K + T)
    # scores on a grid of 2^-12: 1 - s and s (1 - s) are exact in fp32, the oracle in fp64 sees the numbers the reference clamps
    d["scores"] = (torch.round(d["scores"] * 4096.0) / 4096.0).clamp(1.0 / 4096.0, 4095.0 / 4096.0)
    cfg = lr.loss_cfg(w_loss, squared)
    r = lr.wta_loss(d["poses"], d["scores"], d["y"], cfg)
    p, s = d["poses"].double().requires_grad_(True), d["scores"].double()[..., None].requires_grad_(True)
    terms = _oracle_terms(p, s, d["y"].double(), cfg)
    if w_loss < 2:
        _, named = orc.rmcl_training_loss(p, s, d["y"].double(), dict(w_loss=bool(w_loss), vel_loss=cfg["vel"], smooth_reg=cfg["smooth"],
                                                                     rmcl_score_reg=cfg["beta"], sq_loss=squared))
        for k in lr.WTA_TERMS:
            close(terms[k].detach(), named[k].detach(), "assembly " + k)
    for k in lr.WTA_TERMS:
        close(r[k][0], terms[k].detach(), k)
    gp, gs = torch.autograd.grad(sum(terms.values()), (p, s))
    close(r["d_poses"][0], gp, "d_poses")
    close(r["d_scores"][0], gs[..., 0], "d_scores")
    w = None if w_loss == 0 else lr.joint_weights(cfg).double()
    e = orc.weighted_mse_per_hyp(p, d["y"].double(), w) if squared else orc.weighted_mpjpe_per_hyp(p, d["y"].double(), w)
    close(r["e"], e.detach(), "per-hypothesis error")
    assert torch.equal(r["argmin"], e.argmin(1))
    for v in r.values():
        if isinstance(v, tuple):
            assert torch.isfinite(v[1]).all() and (v[1] >= 0).all()


@pytest.mark.parametrize("w_loss,squared", lr.ALL_MODES)
def test_single_loss_matches_the_oracle_and_its_autograd(w_loss, squared):
    B, T = 3, 50
    d = lr.single_case_inputs(B, T)
    cfg = lr.loss_cfg(w_loss, squared)
    r = lr.wta_loss(d["poses"][:, None], None, d["y"], cfg)
    assert "score_reg" not in r and "d_scores" not in r
    p, y = d["poses"].double().requires_grad_(True), d["y"].double()
    w = None if w_loss == 0 else lr.joint_weights(cfg).double()
    terms = dict(wloss=orc.weighted_mse_loss(p, y, w) if squared else orc.weighted_mpjpe_loss(p, y, w),
                 vloss=cfg["vel"] * orc.mean_velocity_error(p, y, axis=1, squared=squared), sreg=cfg["smooth"] * orc.smoothness_regularization(p, w, axis=1))
    if w_loss < 2:
        _, named = orc.manifold_training_loss(p, y, dict(w_loss=bool(w_loss), vel_loss=cfg["vel"], smooth_reg=cfg["smooth"], sq_loss=squared))
        for k in lr.SINGLE_TERMS:
            close(terms[k].detach(), named[k].detach(), "assembly " + k)
    for k in lr.SINGLE_TERMS:
        close(r[k][0], terms[k].detach(), k)
    gp, = torch.autograd.grad(sum(terms.values()), p)
    close(r["d_poses"][0][:, 0], gp, "d_poses")


def test_zero_norm_pieces_are_exactly_zero_and_planted_ties_take_the_lowest_index():
    B, K, T = lr.WTA_PLANTED
    d = lr.wta_case_inputs(B, K, T)
    p, y = d["poses"], d["y"]
    assert d["tie"].sum() == 3 and torch.equal(p[:, 1][d["tie"]], p[:, 3][d["tie"]])
    u = (p[:, :, 1:] - p[:, :, :-1]) - (y[:, 1:] - y[:, :-1])[:, None]
    assert ((u == 0).all(-1)).sum() == 3 and ((p - y[:, None] == 0).all(-1)).sum() == 4
    s = d["scores"]
    for v in (0.0, 1.0, 2.0 ** -30, 1.0 - 2.0 ** -24, 1e-40):
        assert (s == torch.tensor(v, dtype=F32)).any(), v
    assert 0 < float(torch.tensor(1e-40, dtype=F32)) < 2.0 ** -126
    for w_loss, squared in lr.ALL_MODES:
        r = lr.wta_loss(p, s, y, lr.loss_cfg(w_loss, squared))
        assert (r["argmin"][d["tie"]] == 1).all()
        # a joint of the winner that meets y, next to a step that is smooth only: the plain-mode winner piece is 0, the gradient is what the
        # neighbours give; every value is finite, the clamps included
        for k in lr.WTA_TERMS + ("d_poses", "d_scores"):
            assert torch.isfinite(r[k][0]).all() and torch.isfinite(r[k][1]).all(), k
        assert r["d_scores"][0].abs().max() >= 0.09 * 1e12 / (B * K * T)            # a winner at s = 0: beta / (B K T) / 1e-12


def test_rigid_segments_match_the_oracle_and_its_autograd():
    for B, T in ((1, 2), (2, 3), (2, 40), (3, 300)):
        g = lr.gen(B + T)
        x, seed = 0.5 * torch.randn(B, T, 17, 3, generator=g), torch.randn(B, T, 17, 3, generator=g)
        wgt = lr.f32(0.7)
        (term, _), (grad, _) = lr.rigid_segments(x, wgt, seed)
        p = x.double().requires_grad_(True)
        want = wgt * orc.segments_time_consistency(p.permute(0, 3, 2, 1), "sum")
        close(term, want.detach(), f"rigid term {B} {T}")
        gp, = torch.autograd.grad(want, p)
        close(grad - seed.double(), gp, f"rigid gradient {B} {T}", tol=1e-11)      # the sum with the seed rounds at |seed| 1e-16
    # the planted windows: an exactly constant window has variance exactly 0 and leaves the seed alone, a zero-length bone is skipped
    d = lr.rigid_case_inputs(2, 3)
    (term, ts), (grad, gs) = lr.rigid_segments(d["poses"][1:], d["weight"], d["seed"][1:])
    assert term == 0 and ts == 0 and torch.equal(grad, d["seed"][1:].double())
    (term, ts), (grad, gs) = lr.rigid_segments(d["poses"], d["weight"], d["seed"])
    assert torch.isfinite(grad).all() and torch.isfinite(gs).all() and term > 0
    ln = (d["poses"][0, :, 6] - d["poses"][0, :, 5]).norm(dim=-1)
    assert ln[1] == 0 and ln[0] > 0 and ln[2] > 0
    # a rigid window: bone lengths constant to 1e-6, a variance of 1e-12 per bone - nearly all cancellation in fp32
    d = lr.rigid_case_inputs(1, 256)
    (term, ts), _ = lr.rigid_segments(d["poses"], d["weight"], None)
    assert 0 < term < 1e-9 and term <= ts < 1e-8


def test_aggregate_and_mpjpe_match_the_oracle():
    for (B, T) in lr.AGG_BT:
        for K in lr.AGG_K:
            d = lr.agg_case_inputs(B, K, T)
            p, s, y = d["poses"].double(), d["scores"].double(), d["y"].double()
            close(lr.aggregate(d["poses"], d["scores"], d["y"], 0)[0], orc.aggregate(p, s[..., None], "weighted_ave"), "weighted_ave")
            i1 = lr.aggregate(d["poses"], d["scores"], d["y"], 1)[0]
            free = ~d["tie_s"]                                     # (on a planted tie torch's argmax / min need not take the lowest index)
            assert torch.equal(orc.poses_from_hyp_idx(p, i1)[free], orc.aggregate(p, s[..., None], "best_score")[free])
            i2, e = lr.aggregate(d["poses"], d["scores"], d["y"], 2)
            eo, po = orc.aggregate(p, None, "oracle", ground_truth=y)
            assert torch.equal(orc.poses_from_hyp_idx(p, i2), po)     # (a duplicated best hypothesis is the same pose under either index)
            close(e.min(1).values / 17.0, eo, "oracle error")
            assert (i1[d["tie_s"]] == 1).all() and (i2[d["tie_p"]] == 1).all()
            if K >= 5 and B * T >= 127:
                assert d["tie_s"].sum() == 2 and d["tie_p"].sum() == 2 and not (d["tie_s"] & d["tie_p"]).any()
                assert not torch.equal(d["poses"][:, 1][d["tie_s"]], d["poses"][:, 3][d["tie_s"]])
    for n in lr.MPJPE_N[:4]:
        d = lr.mpjpe_case_inputs(n)
        close(lr.mpjpe_sum(d["pred"], d["gt"])[0], orc.mpjpe_error(d["pred"].double(), d["gt"].double(), "sum"), "mpjpe")


@pytest.mark.parametrize("step", lr.ADAM_STEPS)
def test_adam_matches_the_oracle(step):
    h = lr.ADAM_HYPER
    for n in (5, 1025):
        d = lr.adam_case_inputs(n, step)
        p, g, m, v = (d[k].double() for k in ("p", "g", "m", "v"))
        for wd, gs in lr.ADAM_WD_GS:
            (p2, _), (m2, _), (v2, _) = lr.adam(*lr.adam_args(d, step, wd, gs))
            po, mo, vo = orc.adam_step(p, g * gs, m, v, step, h["lr"], h["beta1"], h["beta2"], h["eps"], wd)
            close(p2, po, "p")
            close(m2, mo, "m")
            close(v2, vo, "v")
            # multipliers: the decay enters the gradient as wd wd_mult p, the step is lr_mult times the plain one
            lm, wm = d["lr_mult"].double(), d["wd_mult"].double()
            (p2, _), (m2, _), (v2, _) = lr.adam(*lr.adam_args(d, step, wd, gs), lr_mult=d["lr_mult"], wd_mult=d["wd_mult"])
            po, mo, vo = orc.adam_step(p, g * gs + wd * wm * p, m, v, step, h["lr"], h["beta1"], h["beta2"], h["eps"], 0.0)
            close(p2, p - lm * (p - po), "p, multipliers", tol=1e-11)
            close(m2, mo, "m, multipliers")
            close(v2, vo, "v, multipliers")
        if n > 20:
            assert ((d["v"] == 0) & (d["g"] == 0)).any() and (d["lr_mult"] == 0).any() and (d["wd_mult"] == 0).any() and (d["m"] != 0).all()


# ------------------------------------------------------------------------------------------------ the fixtures, a third witness
@pytest.mark.parametrize("name,squared", [("loss", False), ("loss_sq", True)])
def test_reference_reproduces_the_loss_fixtures(name, squared):
    fx = load_fixture(name)
    poses, scores, y = (torch.as_tensor(np.ascontiguousarray(fx[k])) for k in ("poses", "scores", "y"))
    r = lr.wta_loss(poses, scores[..., 0], y, lr.loss_cfg(1, squared))
    np.testing.assert_allclose([float(r[k][0]) for k in lr.WTA_TERMS], fx["loss_terms"], rtol=2e-5)
    np.testing.assert_allclose(r["d_poses"][0].numpy(), fx["g_poses"], rtol=1e-4, atol=1e-8)
    np.testing.assert_allclose(r["d_scores"][0].numpy(), fx["g_scores"][..., 0], rtol=1e-4, atol=1e-8)
    if squared:
        assert np.array_equal(r["argmin"].numpy(), fx["wta_idx"])
        for nm, w_loss in (("w", 1), ("nw", 0)):
            r1 = lr.wta_loss(poses[:, :1], None, y, lr.loss_cfg(w_loss, True))
            np.testing.assert_allclose([float(r1[k][0]) for k in lr.SINGLE_TERMS], fx[f"single_{nm}.terms"], rtol=2e-5)
            np.testing.assert_allclose(r1["d_poses"][0][:, 0].numpy(), fx[f"single_{nm}.g"], rtol=1e-4, atol=1e-8)


# ------------------------------------------------------------------------------------------------ the winner margin
def test_every_case_keeps_the_winner_margin_with_no_frame_excluded():
    """gap >= 64 u on every frame of every case, in every mode the case runs in, and plain fp32 picks the fp64 winner everywhere; a frame with a
    planted exact tie is measured against the best hypothesis that is not the duplicate.  A seed that violates this is changed, no frame is
    ever excluded."""
    worst_gap = float("inf")
    for B, K, T, modes in lr.WTA_CASES:
        d = lr.wta_case_inputs(B, K, T)
        for w_loss, squared in modes:
            cfg = lr.loss_cfg(w_loss, squared)
            r, r32 = lr.wta_loss(d["poses"], d["scores"], d["y"], cfg), lr.wta_loss(d["poses"], d["scores"], d["y"], cfg, dtype=F32)
            gap = lr.winner_gap(r["e"], None if d["tie"] is None else (3, d["tie"]))
            assert gap.min() >= lr.MARGIN, (B, K, T, w_loss, squared, gap.min().item() / lr.U24)
            assert torch.equal(r["argmin"], r32["argmin"]), (B, K, T, w_loss, squared)
            worst_gap = min(worst_gap, gap.min().item())
    for B, T in lr.AGG_BT:
        for K in lr.AGG_K:
            d = lr.agg_case_inputs(B, K, T)
            i2, e = lr.aggregate(d["poses"], d["scores"], d["y"], 2)
            gap = lr.winner_gap(e, (3, d["tie_p"]))
            assert gap.min() >= lr.MARGIN, ("aggregate", B, K, T, gap.min().item() / lr.U24)
            assert torch.equal(i2, lr.aggregate(d["poses"], d["scores"], d["y"], 2, dtype=F32)[0])
            worst_gap = min(worst_gap, gap.min().item())
            top = d["scores"].double().topk(min(2, K), dim=1).values
            assert K == 1 or ((top[:, 0] > top[:, 1]) | d["tie_s"]).all()              # best_score compares fp32 numbers exactly: distinct is enough
    print(f"[loss kernels] smallest winner gap over all cases: {worst_gap / lr.U24:.3g} u (required >= 64)")


# ------------------------------------------------------------------------------------------------ the bound constants
def _fp32_ratios():
    """worst error / scale of the plain fp32 CPU evaluation of every quantity, over the cases of the GPU module"""
    r = {}

    def put(name, got, ref):
        r[name] = max(r.get(name, 0.0), lr.worst(got, ref[0], ref[1]))

    for B, K, T, modes in lr.WTA_CASES:
        d = lr.wta_case_inputs(B, K, T)
        for w_loss, squared in modes:
            cfg = lr.loss_cfg(w_loss, squared)
            ref, got = lr.wta_loss(d["poses"], d["scores"], d["y"], cfg), lr.wta_loss(d["poses"], d["scores"], d["y"], cfg, dtype=F32)
            for k in lr.WTA_TERMS + ("d_poses", "d_scores"):
                put("wta_" + k, got[k][0], ref[k])
    for B, T in lr.SINGLE_CASES:
        d = lr.single_case_inputs(B, T)
        for squared in (False, True):
            cfg = lr.loss_cfg(1, squared)
            ref, got = lr.wta_loss(d["poses"][:, None], None, d["y"], cfg), lr.wta_loss(d["poses"][:, None], None, d["y"], cfg, dtype=F32)
            for k in lr.SINGLE_TERMS + ("d_poses",):
                put("single_" + k, got[k][0], ref[k])
    for B, T in lr.RIGID_CASES:
        d = lr.rigid_case_inputs(B, T)
        ref, got = lr.rigid_segments(d["poses"], d["weight"], d["seed"]), lr.rigid_segments(d["poses"], d["weight"], d["seed"], dtype=F32)
        put(lr.rigid_term_key(B, T), got[0][0], ref[0])
        put("rigid_d_poses", got[1][0], ref[1])
    for B, T in lr.AGG_BT:
        for K in lr.AGG_K:
            d = lr.agg_case_inputs(B, K, T)
            put("agg_weighted_ave", lr.aggregate(d["poses"], d["scores"], d["y"], 0, dtype=F32)[0], lr.aggregate(d["poses"], d["scores"], d["y"], 0))
    for n in lr.MPJPE_N:
        d = lr.mpjpe_case_inputs(n)
        put("mpjpe_sum", lr.mpjpe_sum(d["pred"], d["gt"], dtype=F32)[0], lr.mpjpe_sum(d["pred"], d["gt"]))
    for n in lr.ADAM_N:
        for step in lr.ADAM_STEPS:
            d = lr.adam_case_inputs(n, step)
            for wd, gs in lr.ADAM_WD_GS:
                for kw in ({}, dict(lr_mult=d["lr_mult"], wd_mult=d["wd_mult"]), dict(lr_mult=torch.ones(n), wd_mult=torch.ones(n))):
                    a = lr.adam_args(d, step, wd, gs)
                    for k, got, ref in zip("pmv", lr.adam(*a, **kw, dtype=F32), lr.adam(*a, **kw)):
                        put("adam_" + k, got[0], ref)
    return r


def test_bound_constants_follow_from_the_fp32_cpu_error():
    ratios = _fp32_ratios()
    assert set(ratios) == set(lr.BOUNDS), sorted(set(ratios) ^ set(lr.BOUNDS))
    for name in sorted(ratios):
        need = lr.bound_from(ratios[name])
        print(f"[loss kernels] {name}: fp32 CPU worst error / scale {ratios[name]:.3g} -> bound {need:g} (asserted on the GPU: {lr.BOUNDS[name]:g})")
    for name, ratio in ratios.items():
        need = lr.bound_from(ratio)
        # the committed constant is the derived one; a CPU whose vector width sums in another order may move the ratio a little, never by 2
        assert need / 2 <= lr.BOUNDS[name] <= max(1.0, 2 * need), (name, ratio, need, lr.BOUNDS[name])

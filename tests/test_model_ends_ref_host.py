"""The fp64 references of tests/ends_ref.py, verified without a GPU: they agree with the oracle (oracle/manipose_ref.py) evaluated in fp64 on
the same inputs to 1e-12 relative, their analytic backward formulas agree with fp64 autograd, and the bound constants test_gpu_model_ends.py
asserts follow from the error of the same formulas evaluated in plain fp32 torch on the CPU (ends_ref.bound_from: 4 x the worst
error / scale ratio over the GPU module's shapes, rounded up to one significant digit, never below 1)."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

import ends_ref as er

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import manipose_ref as orc  # noqa: E402


def close(a, b, what, tol=1e-12):
    err = (a - b).abs().max().item()
    ref = b.abs().max().item()
    assert err <= tol * max(ref, 1e-300), f"{what}: {err:.3g} against {ref:.3g}"


def test_tables_match_the_oracle():
    assert er.PARENTS == list(orc.H36M_PARENTS)
    assert [list(map(float, o)) for o in er.TPOSE_OPS[1:]] == [list(map(float, orc.T_POSE_OPERATORS[j])) for j in range(1, 17)]


# ------------------------------------------------------------------------------------------------ against the oracle, fp64
def test_embeddings_match_the_oracle():
    M, C, J = 17 * 3, 32, 17
    d = er.embed_inputs(M, C, J, er.gen(1))
    want = F.linear(d["x"].double().reshape(3, J, 2), d["W"].double(), d["b"].double()) + d["spos"].double()     # mixste_backbone, STE_forward
    close(er.embed_fwd(d["x"], d["W"], d["b"], d["spos"], J)[0], want.reshape(M, C), "embed_fwd")
    d = er.bones_embed_inputs(5, 256, er.gen(2))
    z = F.linear(d["x"].double(), d["W"].double(), d["b"].double()).reshape(5, 16, 16) + d["spos"].double().reshape(16, 16)   # bones_forward + STE_forward
    close(er.bones_embed_fwd(d["x"], d["W"], d["b"], d["spos"])[0], z.reshape(5, 256), "bones_embed_fwd")


def test_score_head_matches_the_oracle():
    K, O, J, B, T = 3, 7, 17, 2, 5
    d = er.score_inputs(K, O, B, T, J, er.gen(3))
    (s, _), _ = er.scores_fwd(d["h"], d["w"], d["b"], B, T, J)
    z = d["h"].double().reshape(K, B, T, J, O)
    logits = [F.linear(z[k][..., -1], d["w"][k:k + 1].double(), d["b"][k:k + 1].double()) for k in range(K)]      # rmcl_rot_forward
    close(s, torch.stack(logits, dim=1).softmax(dim=1)[..., 0], "scores")
    hm = torch.randn(2 * 9 * 16, generator=er.gen(4))
    close(er.bones_mean_fwd(hm, 2, 9, 16)[0], hm.double().reshape(2, 9, 16, 1).mean(dim=1)[..., 0], "bones mean")      # bones_forward


@pytest.mark.parametrize("rot_dim,stride", er.FK_REPS)
def test_decoder_matches_the_oracle_and_its_autograd(rot_dim, stride):
    B, K, T = 2, 3, 4
    d = er.fk_inputs(B, K, T, rot_dim, stride, er.gen(5), zero_halves=False)      # the oracle's sqrt has no gradient at a zero half
    (poses, _), (drot, _), (dlen, _) = er.fk_reference(d["rot"], d["lengths"], d["dposes"], B, K, T, rot_dim)
    r = er._rows(d["rot"].double(), B, K, T, rot_dim).reshape(B * K * T, 17, rot_dim).clone().requires_grad_(True)
    bl = d["lengths"].double().reshape(B, 16, 1).clone().requires_grad_(True)
    want = orc.pose_decoder(r, bl).reshape(B, K, T, 17, 3)
    close(poses, want.detach(), "poses")
    assert (poses[..., 0, :] == 0).all()
    gr, gl = torch.autograd.grad(want, (r, bl), d["dposes"].double())
    close(er._rows(drot, B, K, T, rot_dim).reshape(-1, 17, rot_dim), gr, "drot")
    close(dlen.sum((1, 2)), gl[..., 0], "dlengths")


def test_decoder_clamp_branches_are_finite():
    B, K, T = 2, 5, 7
    for rot_dim, stride in er.FK_REPS:
        d = er.fk_inputs(B, K, T, rot_dim, stride, er.gen(6))
        h = rot_dim // 2
        r = d["rot"][..., :rot_dim]
        assert ((r[..., :h] == 0).all(-1) | (r[..., h:] == 0).all(-1)).sum() == 6
        for v, s in er.fk_reference(d["rot"], d["lengths"], d["dposes"], B, K, T, rot_dim):
            assert torch.isfinite(v).all() and torch.isfinite(s).all() and (s >= 0).all()


# ------------------------------------------------------------------------------------------------ analytic backward against fp64 autograd
def test_analytic_backwards_match_autograd():
    M, C, J = 17 * 4, 32, 17
    d = er.embed_inputs(M, C, J, er.gen(7))
    leaves = [d[k].double().clone().requires_grad_(True) for k in ("W", "b", "spos")]
    out = F.linear(d["x"].double(), leaves[0], leaves[1]) + leaves[2].repeat(4, 1)
    grads = torch.autograd.grad(out, leaves, d["g"].double())
    zero = [torch.zeros_like(t) for t in (d["sW"], d["sb"], d["sspos"])]
    for (got, _), want, name in zip(er.embed_bwd(d["g"], d["x"], J, *zero), grads, ("dW", "db", "dspos")):
        close(got, want, "embed " + name)
    d = er.bones_embed_inputs(9, 256, er.gen(8))
    leaves = [d[k].double().clone().requires_grad_(True) for k in ("W", "b", "spos")]
    grads = torch.autograd.grad(F.linear(d["x"].double(), leaves[0], leaves[1]) + leaves[2], leaves, d["g"].double())
    zero = [torch.zeros_like(t) for t in (d["sW"], d["sb"], d["sspos"])]
    for (got, _), want, name in zip(er.bones_embed_bwd(d["g"], d["x"], *zero), grads, ("dW", "db", "dspos")):
        close(got, want, "bones_embed " + name)
    B, T = 3, 5
    g = torch.randn(B * T * J, C, generator=er.gen(9))
    tp = torch.zeros(T, C, dtype=torch.float64, requires_grad=True)
    x = torch.zeros(B, J, T, C, dtype=torch.float64) + tp                                     # TTE_foward: x (B J, T, C) + Temporal_pos_embed
    want, = torch.autograd.grad(x, tp, g.double().reshape(B, T, J, C).permute(0, 2, 1, 3))
    close(er.tpos_grad(g, torch.zeros(T, C), B, T, J)[0], want, "tpos_grad")


def test_score_backward_matches_autograd():
    K, O, J, B, T = 5, 7, 17, 2, 9
    d = er.score_inputs(K, O, B, T, J, er.gen(10))
    h = d["h"].double().clone().requires_grad_(True)
    w, b = d["w"].double().clone().requires_grad_(True), d["b"].double().clone().requires_grad_(True)
    logit = (h[:, :, O - 1].reshape(K, B * T, J) * w[:, None, :]).sum(-1) + b[:, None]
    s = torch.softmax(logit, 0).reshape(K, B, T).permute(1, 0, 2)
    gh, gw, gb = torch.autograd.grad(s, (h, w, b), d["d"].double())
    zero = torch.zeros(K, J), torch.zeros(K)
    (dh, _), (dw, _), (db, _) = er.scores_bwd(d["h"], s.detach(), d["d"], d["w"], *zero, B, T, J)
    close(dh, gh[:, :, O - 1], "dheadout score channel")
    assert (gh[:, :, :O - 1] == 0).all()
    close(dw, gw, "dw")
    close(db, gb, "db")
    B, K, T, S = 3, 5, 9, 17                                                                 # bones_forward mean, lengths repeated over K T poses
    dlp = torch.randn(B * K * T, S, generator=er.gen(11))
    hh = torch.zeros(B, T, S, dtype=torch.float64, requires_grad=True)
    rep = hh.mean(1)[:, None, :].expand(B, K * T, S)
    want, = torch.autograd.grad(rep, hh, dlp.double().reshape(B, K * T, S))
    got, _ = er.bones_mean_bwd(dlp, B, K * T, S)
    close((got / T)[:, None, :].expand(B, T, S), want, "bones mean backward")


# ------------------------------------------------------------------------------------------------ the bound constants
def _fp32_ratios():
    """worst error / scale of the plain fp32 CPU evaluation of every quantity, over the shapes of the GPU module"""
    r = {}

    def put(name, got, ref, floor=0.0):
        r[name] = max(r.get(name, 0.0), er.worst(got, ref[0], ref[1], floor))

    def pairs(name, f, *a, names, floor=0.0):
        for n, got, ref in zip(names, f(*a, dtype=torch.float32), f(*a)):
            put(name + n, got[0], ref, floor)

    cases = [(17, 17 * f, C) for f in er.EMBED17_FRAMES for C in er.EMBED17_C] + er.EMBED_GENERIC
    for i, (J, M, C) in enumerate(cases):
        d = er.embed_inputs(M, C, J, er.gen(100 + i))
        a = (d["x"], d["W"], d["b"], d["spos"], J)
        put("embed_fwd", er.embed_fwd(*a, dtype=torch.float32)[0], er.embed_fwd(*a))
        pairs("embed_", er.embed_bwd, d["g"], d["x"], J, d["sW"], d["sb"], d["sspos"], names=("dW", "db", "dspos"))
    for i, (BT, O) in enumerate((bt, o) for bt in er.BONES_EMBED_BT for o in er.BONES_EMBED_O):
        d = er.bones_embed_inputs(BT, O, er.gen(200 + i))
        a = (d["x"], d["W"], d["b"], d["spos"])
        put("bones_embed_fwd", er.bones_embed_fwd(*a, dtype=torch.float32)[0], er.bones_embed_fwd(*a))
        pairs("bones_embed_", er.bones_embed_bwd, d["g"], d["x"], d["sW"], d["sb"], d["sspos"], names=("dW", "db", "dspos"))
    for i, (B, T, J, C) in enumerate(er.TPOS):
        g = er.gen(300 + i)
        gg, seed = torch.randn(B * T * J, C, generator=g), torch.randn(T, C, generator=g)
        put("tpos_grad", er.tpos_grad(gg, seed, B, T, J, dtype=torch.float32)[0], er.tpos_grad(gg, seed, B, T, J))
    for i, (K, O, J, B, T, pat) in enumerate(er.SCORES):
        d = er.score_inputs(K, O, B, T, J, er.gen(400 + i), pat)
        (s32, _), _ = er.scores_fwd(d["h"], d["w"], d["b"], B, T, J, dtype=torch.float32)
        (s, sc), _ = er.scores_fwd(d["h"], d["w"], d["b"], B, T, J)
        put("scores", s32, (s, sc), er.F32_TINY)      # an underflowing score (and a product with one, below) has no relative precision
        a = (d["h"], s32, d["d"], d["w"], d["sw"], d["sb"], B, T, J)
        pairs("scores_", er.scores_bwd, *a, names=("dheadout", "dw", "db"), floor=er.F32_TINY)
    for i, (B, K, T, S) in enumerate(er.BONES_MEAN):
        g = er.gen(500 + i)
        h, dlp = torch.randn(B * T * S, generator=g), torch.randn(B * K * T, S, generator=g)
        put("bones_mean_fwd", er.bones_mean_fwd(h, B, T, S, dtype=torch.float32)[0], er.bones_mean_fwd(h, B, T, S))
        put("bones_mean_bwd", er.bones_mean_bwd(dlp, B, K * T, S, dtype=torch.float32)[0], er.bones_mean_bwd(dlp, B, K * T, S))
    for i, ((B, K, T), (rd, stride)) in enumerate((s, f) for s in er.FK_BKT for f in er.FK_REPS):
        d = er.fk_inputs(B, K, T, rd, stride, er.gen(600 + i))
        a = (d["rot"], d["lengths"], d["dposes"], B, K, T, rd)
        for n, got, ref in zip(("poses", "drot", "dlen"), er.fk_reference(*a, dtype=torch.float32), er.fk_reference(*a)):
            put(f"fk{rd}_" + n, got[0], ref)
    return r


def test_bound_constants_follow_from_the_fp32_cpu_error():
    ratios = _fp32_ratios()
    assert set(ratios) == set(er.BOUNDS), sorted(set(ratios) ^ set(er.BOUNDS))
    for name in sorted(ratios):
        need = er.bound_from(ratios[name])
        print(f"[model ends] {name}: fp32 CPU worst error / scale {ratios[name]:.3g} -> bound {need:g} (asserted on the GPU: {er.BOUNDS[name]:g})")
    for name, ratio in ratios.items():
        need = er.bound_from(ratio)
        # the committed constant is the derived one; a CPU whose vector width sums in another order may move the ratio a little, never by 2
        assert need / 2 <= er.BOUNDS[name] <= max(1.0, 2 * need), (name, ratio, need, er.BOUNDS[name])

"""fp64 references of the kernels that end a training step and an evaluation - the fused WTA loss with its gradient (mp_wta_loss,
mp_single_loss), the rigid-segments term (mp_rigid_segments_loss), mp_aggregate, mp_mpjpe_sum and the Adam update (mp_adam_step,
mp_adam_step_scaled) - with per-element forward-error scales, and the seeded inputs the host and the GPU tests share (no GPU).

Every function takes the fp32 tensors exactly as the kernel receives them and a `dtype`: torch.float64 gives the reference, torch.float32 the
same formula in plain fp32 torch (test_loss_ref_host.py measures its error to derive the bound constants of test_gpu_loss_kernels.py).
A result is a pair (value, scale): an error is asserted per element as |got - value| <= C u scale, u = 2^-24.  The formulas are those of the
header comment of wta_loss.hip and of oracle/manipose_ref.py (test_loss_ref_host.py checks them against the oracle and its autograd).

Scales (absolute values of the pieces a result is summed from, plus the result; a quantity that is itself computed carries its own scale on):
  difference    d = p - y of two inputs: |d| (one rounding).  u = (p' - p) - (y' - y): |p' - p| + |y' - y| + |u|
  norm          n = |c| of a vector c whose components carry the scales e_c:   N = sum_c |c_c| e_c / n + n;  n^2:  sum_c 2 |c_c| e_c + n^2
  unit vector   coef c_c / n:   |coef| (e_c / n + |c_c| / n * N / n) + |piece|   (the division carries the relative error N / n of n);
                where n == 0 exactly the piece is 0 (torch.norm's subgradient; the kernel skips it)
  scalar terms  wloss, score_reg, vloss, sreg, the rigid term, the MPJPE sum:  sum of the addends' own scales + |sum|
                (an addend coef n has the scale |coef| N + |addend|; a BCE addend -log(.) bce: 2 |addend|)
  d_poses       winner piece + velocity pieces towards t+1 and t-1 + smoothness pieces towards both: the sum of the pieces' scales + |result|
  d_scores      bce (s - gt) / max(s (1 - s), 1e-12), on the fp32 s - gt and fp32 s (1 - s) the kernel forms:  2 |result|
                + 2^-125 / max(s (1 - s), 1e-12)  (bce (s - gt) underflows for a denormal score: one denormal spacing 2^-149 = u 2^-125, divided on)
  rigid         d = len - len(frame 0) per bone and frame; the variance of a bone (sum d^2 - (sum d)^2 / T) / (T - 1) carries its cancellation:
                (sum d^2 + (sum d)^2 / T) / (T - 1) + var.  The roundings of the lengths themselves (u len each, not u d) are not in the scale:
                where a skeleton is rigid they are all there is, and the plain fp32 evaluation is ~1000 u of this scale off.  So the term has
                two bound constants, each derived by the same rule from its own cases: `rigid_term` over the cases with ordinary windows,
                `rigid_term_rigid` over the cases that are one rigid window (rigid_term_key), where the constant carries that amplification
                gradient seed + sum_bones c (len - mean) / len * delta:   sum_bones |c| (|len| + |mean|) / len |delta| + |seed| + |result|
  aggregate     weighted_ave: sum_k |p_k s_k| + |out|;  best_score / oracle: the index, the output is a bit-exact copy of that hypothesis
  Adam          gr = g gscale + wd wd_mult p:  G = |g gscale| + 2 |wd wd_mult p| + |gr|;   m' = b1 m + (1 - b1) gr:  M = |b1 m| + (1 - b1) G + |m'|;
                v' = b2 v + (1 - b2) gr^2:  V = |b2 v| + (1 - b2) 2 |gr| G + |v'|;   den = sqrt(v') / sqrt(bc2) + eps;
                p' = p - upd, upd = lr / bc1 * lr_mult * m' / den:   |p| + lr / bc1 |lr_mult| (M + |m'| (1 + V / (2 v') * sqrt(v' / bc2) / den)) / den + |p'|

Winner margin: an fp32 kernel and fp64 may pick different winners only where two hypotheses are within rounding.  Every reference that
picks a winner also returns gap = (e2 - e1) / (e1 + e2) per frame (best and second best, fp64); test_loss_ref_host.py asserts
gap >= 64 u on every frame of every case (a planted exact tie is measured against the best hypothesis that is not its duplicate)."""
import math

import torch

from ends_ref import PARENTS, U24, bound_from, gen, worst  # noqa: F401  (re-exported: the two test modules take them from here)

NJ = 17
H36M_W = [1, 1, 2.5, 2.5, 1, 2.5, 2.5, 1, 1, 1, 1.5, 1.5, 4, 4, 1.5, 4, 4]
CUSTOM_W = [0.0, 1.0, 2.5, 0.5, 1.0, 3.0, 0.25, 1.0, 2.0, 1.0, 1.5, 0.75, 4.0, 0.0, 1.5, 4.0, 1.25]      # w_loss == 2: a 0 and unequal values
MARGIN = 64 * U24
F32_DENORM = 2.0 ** -125      # u x this = 2^-149, the spacing of the fp32 denormals: the absolute error of a product that underflows
F32 = torch.float32
F64 = torch.float64


def f32(x):
    """the fp32 value of a Python float (what the C ABI receives), as a Python float"""
    return float(torch.tensor(x, dtype=F32))


def loss_cfg(w_loss=1, squared=False, beta=0.1, vel=2.0, smooth=0.5):
    return dict(w_loss=w_loss, squared=bool(squared), beta=f32(beta), vel=f32(vel), smooth=f32(smooth))


def joint_weights(cfg):
    return torch.tensor({0: [1.0] * NJ, 1: H36M_W, 2: CUSTOM_W}[cfg["w_loss"]], dtype=F32)


def _consts(B, K, T, cfg, has_scores, dtype):
    """the four normalisations of loss_impl: exact in fp64, with the kernel's fp32 operations in fp32"""
    sq = cfg["squared"]
    if dtype == F64:
        return (1.0 / (B * T), cfg["beta"] / (B * K * T) if has_scores else 0.0, cfg["vel"] / (B * K * (T - 1) * NJ * (3 if sq else 1)),
                cfg["smooth"] / (B * K * (T - 1) * NJ * 3))
    t = lambda v: torch.tensor(float(v), dtype=F32)
    return (float(1.0 / (t(B) * t(T))), float(t(cfg["beta"]) / (t(B) * t(K) * t(T))) if has_scores else 0.0,
            float(t(cfg["vel"]) / (t(B) * t(K) * t(T - 1) * t(NJ) * t(3 if sq else 1))), float(t(cfg["smooth"]) / (t(B) * t(K) * t(T - 1) * t(NJ) * t(3))))


def _norm(c, ec):
    """n = |c| over the last axis, its square, and their scales (module docstring); where n == 0 the scale of n is 0"""
    n2 = (c * c).sum(-1)
    n = n2.sqrt()
    lin = (c.abs() * ec).sum(-1)
    pos = n > 0
    safe = torch.where(pos, n, torch.ones_like(n))
    return n, torch.where(pos, lin / safe + n, torch.zeros_like(n)), n2, 2.0 * lin + n2


def _unit_piece(coef, c, ec, n, n_s):
    """coef c / n per component and its scale; 0 where n == 0"""
    pos = (n > 0)[..., None]
    safe = torch.where(n > 0, n, torch.ones_like(n))[..., None]
    piece = torch.where(pos, coef * c / safe, torch.zeros_like(c))
    scale = torch.where(pos, coef.abs() * (ec / safe + c.abs() / safe * (n_s[..., None] / safe)) + piece.abs(), torch.zeros_like(c))
    return piece, scale


def _first_min(e, dim=1):
    """the minimum over `dim` and the LOWEST index that attains it (the kernels' strict `<`)"""
    e = e.movedim(dim, 0)
    best, kb = e[0].clone(), torch.zeros(e[0].shape, dtype=torch.long)
    for k in range(1, e.shape[0]):
        lt = e[k] < best
        best, kb = torch.where(lt, e[k], best), torch.where(lt, torch.full_like(kb, k), kb)
    return best, kb


def winner_gap(e, dup=None):
    """(e2 - e1) / (e1 + e2) per frame of e (B, K, T); dup = (k, frames (B, T) bool): hypothesis k is a planted bit-identical copy of a lower
    one on those frames and does not count as the second best there.  K == 1: inf."""
    e = e.double().clone()
    B, K, T = e.shape
    if K == 1:
        return torch.full((B, T), float("inf"), dtype=F64)
    if dup is not None:
        e[:, dup[0]][dup[1]] = float("inf")
    lo = e.topk(2, dim=1, largest=False).values
    return torch.where(torch.isinf(lo[:, 1]), torch.full((B, T), float("inf"), dtype=F64), (lo[:, 1] - lo[:, 0]) / (lo[:, 0] + lo[:, 1]))


# ------------------------------------------------------------------------------------------------ the fused loss
def wta_loss(poses, scores, y, cfg, dtype=F64):
    """poses (B, K, T, 17, 3), scores (B, K, T) or None (the single-hypothesis form: no BCE term, K = 1), y (B, T, 17, 3) ->
    dict(argmin (B, T), e (B, K, T), wloss / score_reg / vloss / sreg = (value, scale), d_poses = (value, scale), d_scores = (value, scale))"""
    B, K, T = poses.shape[:3]
    D, sq = dtype, cfg["squared"]
    wta, bce, vel, smooth = _consts(B, K, T, cfg, scores is not None, D)
    p, yy, w = poses.to(D), y.to(D), joint_weights(cfg).to(D)
    out = {}
    # ---- per-hypothesis distance, the winner
    diff = p - yy[:, None]
    e_diff = diff.abs()
    n, n_s, d2, d2_s = _norm(diff, e_diff)
    a, a_s = (w * d2, w * d2_s) if sq else (w * n, w * n_s)
    den = float(NJ * 3 if sq else NJ)
    e = a.sum(-1) / den
    best, kb = _first_min(e)
    out["argmin"], out["e"] = kb, e
    gt = torch.zeros(B, K, T, dtype=torch.bool).scatter_(1, kb[:, None], True)
    win = gt[..., None].to(D)
    wl = (best * wta).sum()
    out["wloss"] = (wl, (a_s * win).sum() / den * wta + wl.abs())
    # ---- scoring BCE and its gradient, on the fp32 s, 1 - s, s (1 - s) and s - gt of the kernel
    if scores is not None:
        s32 = scores.to(F32)
        om32, d32 = 1.0 - s32, s32 - gt.to(F32)
        den32 = (s32 * om32).clamp_min(torch.tensor(1e-12, dtype=F32))
        l1, l0 = s32.to(D).log().clamp_min(-100.0), om32.to(D).log().clamp_min(-100.0)
        add = -torch.where(gt, l1, l0) * bce
        sr = add.sum()
        out["score_reg"] = (sr, 2.0 * add.abs().sum() + sr.abs())
        ds = bce * d32.to(D) / den32.to(D)
        out["d_scores"] = (ds, 2.0 * ds.abs() + F32_DENORM / den32.to(D))
    # ---- velocity and smoothness over the T - 1 steps, all hypotheses
    s = p[:, :, 1:] - p[:, :, :-1]
    dy = (yy[:, 1:] - yy[:, :-1])[:, None]
    u = s - dy
    e_u = s.abs() + dy.abs() + u.abs()
    nv, nv_s, nv2, nv2_s = _norm(u, e_u)
    add = (nv2 if sq else nv) * vel
    vl = add.sum()
    out["vloss"] = (vl, ((nv2_s if sq else nv_s) * vel + add).sum() + vl.abs())
    add = w * (s * s).sum(-1) * smooth
    sg = add.sum()
    out["sreg"] = (sg, 4.0 * add.sum() + sg.abs())
    # ---- d_poses: winner piece, velocity and smoothness pieces towards t + 1 (subtracted at t) and t - 1 (added at t + 1)
    if sq:
        cw = (wta * (2.0 / (NJ * 3))) * w[:, None]
        wp = cw * diff * win[..., None]
        wp_s = 2.0 * wp.abs()
        vp = (2.0 * vel) * u
        vp_s = (2.0 * vel) * e_u + vp.abs()
    else:
        wp, wp_s = _unit_piece(((wta / NJ) * w)[:, None].expand_as(diff), diff, e_diff, n, n_s)
        wp, wp_s = wp * win[..., None], wp_s * win[..., None]
        vp, vp_s = _unit_piece(torch.full_like(u, vel), u, e_u, nv, nv_s)
    sp = (2.0 * smooth) * w[:, None] * s
    step, step_s = vp + sp, vp_s + 2.0 * sp.abs()
    g, g_s = wp.clone(), wp_s.clone()
    g[:, :, :-1] -= step
    g[:, :, 1:] += step
    g_s[:, :, :-1] += step_s
    g_s[:, :, 1:] += step_s
    out["d_poses"] = (g, g_s + g.abs())
    return out


WTA_TERMS = ("wloss", "score_reg", "vloss", "sreg")
SINGLE_TERMS = ("wloss", "vloss", "sreg")


# ------------------------------------------------------------------------------------------------ rigid segments
BONE_J = list(range(1, NJ))
BONE_P = PARENTS[1:]


def rigid_segments(poses, weight, seed, dtype=F64):
    """poses (B, T, 17, 3), weight (an fp32 value), seed (B, T, 17, 3) or None -> (term, scale), (seed + gradient, scale)"""
    B, T = poses.shape[:2]
    D = dtype
    x = poses.to(D)
    delta = x[:, :, BONE_J] - x[:, :, BONE_P]                                  # (B, T, 16, 3)
    ln = _norm(delta, delta.abs())[0]
    d = ln - ln[:, :1]
    u, v = d.sum(1), (d * d).sum(1)
    var = (v - u * u / T).clamp_min(0.0) / (T - 1)
    var_s = (v + u * u / T) / (T - 1) + var
    term = weight * var.sum()
    mean = ln[:, 0] + u / T
    c = (weight * 2.0 / (T - 1)) if D == F64 else float(torch.tensor(weight, dtype=F32) * 2.0 / torch.tensor(float(T - 1), dtype=F32))
    pos = ln > 0
    safe = torch.where(pos, ln, torch.ones_like(ln))
    sc = torch.where(pos, c * (ln - mean[:, None]) / safe, torch.zeros_like(ln))[..., None]
    piece = sc * delta
    piece_s = torch.where(pos, abs(c) * (ln.abs() + mean.abs()[:, None]) / safe, torch.zeros_like(ln))[..., None] * delta.abs()
    g = torch.zeros_like(x) if seed is None else seed.to(D).clone()
    g_s = g.abs()
    jj, pp = torch.tensor(BONE_J), torch.tensor(BONE_P)
    g.index_add_(2, jj, piece)
    g.index_add_(2, pp, -piece)
    g_s.index_add_(2, jj, piece_s)
    g_s.index_add_(2, pp, piece_s)
    return (term, abs(weight) * var_s.sum() + term.abs()), (g, g_s + g.abs())


# ------------------------------------------------------------------------------------------------ aggregation, MPJPE
def aggregate(poses, scores, y, mode, dtype=F64):
    """mode 0 weighted_ave -> (out (B, T, 17, 3), scale); 1 best_score / 2 oracle -> (index (B, T), e (B, K, T) or None)"""
    D = dtype
    p = poses.to(D)
    if mode == 0:
        terms = p * scores.to(D)[..., None, None]
        out = terms.sum(1)
        return out, terms.abs().sum(1) + out.abs()
    if mode == 1:
        return _first_min(-scores.to(D))[1], None
    diff = p - y.to(D)[:, None]
    e = _norm(diff, diff.abs())[0].sum(-1)
    return _first_min(e)[1], e


def mpjpe_sum(pred, target, dtype=F64):
    diff = (pred.to(dtype) - target.to(dtype)).reshape(-1, 3)
    n, n_s, _, _ = _norm(diff, diff.abs())
    tot = n.sum()
    return tot, n_s.sum() + tot.abs()


# ------------------------------------------------------------------------------------------------ Adam
def adam(p, g, m, v, step, lr, beta1, beta2, eps, wd, gscale, lr_mult=None, wd_mult=None, dtype=F64):
    """-> (p', scale), (m', scale), (v', scale); lr .. gscale are fp32 values.  lr / bc1 and 1 / sqrt(bc2) are formed in double and rounded
    to fp32 once, as adam_step does."""
    D = dtype
    p, g, m, v = (t.to(D) for t in (p, g, m, v))
    lm = torch.ones_like(p) if lr_mult is None else lr_mult.to(D)
    wm = torch.ones_like(p) if wd_mult is None else wd_mult.to(D)
    lrc, isb = lr / (1.0 - beta1 ** step), 1.0 / math.sqrt(1.0 - beta2 ** step)
    if D != F64:
        lrc, isb = f32(lrc), f32(isb)
    sc = lambda x: torch.tensor(x, dtype=D)
    ob1, ob2 = (sc(1.0) - sc(beta1)), (sc(1.0) - sc(beta2))                      # exact in both precisions (Sterbenz)
    wdp = (sc(wd) * wm) * p
    gr = g * sc(gscale) + wdp
    G = (g * gscale).abs() + 2.0 * wdp.abs() + gr.abs()
    m2 = sc(beta1) * m + ob1 * gr
    M = (beta1 * m).abs() + ob1 * G + m2.abs()
    v2 = sc(beta2) * v + ob2 * gr * gr
    V = (beta2 * v).abs() + ob2 * 2.0 * gr.abs() * G + v2.abs()
    root = v2.sqrt() * sc(isb)
    den = root + sc(eps)
    p2 = p - (sc(lrc) * lm) * (m2 / den)
    rel_den = torch.where(v2 > 0, 0.5 * V / torch.where(v2 > 0, v2, torch.ones_like(v2)), torch.zeros_like(v2)) * root / den
    P = p.abs() + (lrc * lm).abs() * (M + m2.abs() * (1.0 + rel_den)) / den + p2.abs()
    return (p2, P), (m2, M), (v2, V)


ADAM_HYPER = dict(lr=f32(4e-5), beta1=f32(0.9), beta2=f32(0.999), eps=f32(1e-8))


# ------------------------------------------------------------------------------------------------ seeded inputs
def wta_inputs(B, K, T, seed, planted=False):
    """y = 0.5 randn, poses = y + 0.05 randn, scores in (0, 1).  planted (the (2, 5, 7) case): exact ties of hypotheses 1 and 3 that win,
    p == y on joints of a winner, (p' - p) == (y' - y) exactly on three (k, t, j), and scores 0, 1, 2^-30, 1 - 2^-24 and a denormal.
    -> dict(poses, scores, y, tie (B, T) bool or None)"""
    g = gen(seed)
    y = 0.5 * torch.randn(B, T, NJ, 3, generator=g)
    exact = [(0, 2, 3, 5), (1, 0, 0, 16), (1, 4, 5, 0)] if planted else []         # (b, k, t, j): the step t -> t + 1
    for b, k, t, j in exact:
        y[b, t:t + 2, j] = torch.round(y[b, t:t + 2, j] * 1024.0) / 1024.0         # a few mantissa bits: every sum below is exact
    poses = y[:, None] + 0.05 * torch.randn(B, K, T, NJ, 3, generator=g)
    scores = torch.sigmoid(1.5 * torch.randn(B, K, T, generator=g))
    tie = None
    if planted:
        for b, k, t, j in exact:
            poses[b, k, t:t + 2, j] = y[b, t:t + 2, j] + 0.0625
        tie = torch.zeros(B, T, dtype=torch.bool)
        for b, t in [(0, 1), (0, 6), (1, 2)]:
            poses[b, 1, t] = y[b, t] + 0.01 * torch.randn(NJ, 3, generator=g)
            poses[b, 3, t] = poses[b, 1, t]
            tie[b, t] = True
        for k in (1, 3):                                                            # the winner of a tie frame (in every mode) meets y exactly on two joints
            for j in (3, 9):
                poses[0, k, 6, j] = y[0, 6, j]
        scores[0, 1, 1], scores[0, 3, 1] = 0.0, 1.0                                 # a winner at 0, a loser at 1: both logs clamp at -100
        scores[0, 1, 6], scores[0, 0, 6] = 1.0, 0.0
        scores[1, 0, 3], scores[1, 1, 3], scores[1, 2, 3] = 2.0 ** -30, 1.0 - 2.0 ** -24, 1e-40
        scores[1, 1, 2], scores[1, 3, 2] = 1e-40, 1.0 - 2.0 ** -24
    return dict(poses=poses.contiguous(), scores=scores.contiguous(), y=y, tie=tie)


def rigid_inputs(B, T, seed):
    """random poses; from T >= 255 on window 0 is a rigid skeleton (bone lengths constant up to the fp32 rounding of the joints) plus noise of
    1e-6: its variances are nearly all cancellation; with T == 3 one bone of window 0 has exactly zero length in frame 1 and window 1 (if
    there is one) is exactly constant.  -> dict(poses, seed, weight)"""
    g = gen(seed)
    x = 0.5 * torch.randn(B, T, NJ, 3, generator=g)
    if T >= 255:
        lens = 0.1 + 0.4 * torch.rand(NJ, generator=g, dtype=F64)
        dirs = torch.nn.functional.normalize(torch.randn(T, NJ, 3, generator=g, dtype=F64), dim=-1)
        pos = [torch.randn(T, 3, generator=g, dtype=F64)]
        for j in range(1, NJ):
            pos.append(pos[PARENTS[j]] + lens[j] * dirs[:, j])
        x[0] = (torch.stack(pos, 1) + 1e-6 * torch.randn(T, NJ, 3, generator=g, dtype=F64)).float()
    if T == 3:
        x[0, 1, 6] = x[0, 1, 5]                                                     # bone (6, 5) of frame 1: length exactly 0
        if B >= 2:
            x[1] = x[1, :1]
    return dict(poses=x.contiguous(), seed=torch.randn(B, T, NJ, 3, generator=g), weight=f32(0.7))


def aggregate_inputs(B, K, T, seed):
    """poses, scores (a softmax over K), y; from K >= 5 on, frames 0 and B T / 2 carry equal top scores on hypotheses 1 and 3 (whose poses
    differ) and frames B T - 1 and B T / 3 (where those are other frames) bit-identical best hypotheses 1 and 3
    -> dict(poses, scores, y, tie_s, tie_p (B, T) bool)"""
    g = gen(seed)
    y = 0.5 * torch.randn(B, T, NJ, 3, generator=g)
    poses = y[:, None] + 0.05 * torch.randn(B, K, T, NJ, 3, generator=g)
    scores = torch.softmax(torch.randn(B, K, T, generator=g), 1)
    tie_s, tie_p = torch.zeros(B, T, dtype=torch.bool), torch.zeros(B, T, dtype=torch.bool)
    if K >= 5:
        fs = {0, (B * T) // 2}
        for f in sorted(fs):
            b, t = divmod(f, T)
            scores[b, 1, t] = scores[b, 3, t] = scores[b, :, t].max() + 0.125
            tie_s[b, t] = True
        for f in sorted({B * T - 1, (B * T) // 3} - fs):
            b, t = divmod(f, T)
            poses[b, 1, t] = y[b, t] + 0.01 * torch.randn(NJ, 3, generator=g)
            poses[b, 3, t] = poses[b, 1, t]
            tie_p[b, t] = True
    return dict(poses=poses.contiguous(), scores=scores.contiguous(), y=y, tie_s=tie_s, tie_p=tie_p)


def mpjpe_inputs(n, seed):
    g = gen(seed)
    gt = 0.5 * torch.randn(n, 3, generator=g)
    return dict(pred=gt + 0.05 * torch.randn(n, 3, generator=g), gt=gt)


def adam_inputs(n, seed):
    """non-zero m, v >= 0 with exact zeros where g == 0 too, multipliers that include 0 and values != 1"""
    g = gen(seed)
    p, gr, m = torch.randn(n, generator=g), torch.randn(n, generator=g) * (0.25 + torch.rand(n, generator=g)), 0.1 * torch.randn(n, generator=g)
    v = (0.1 * torch.randn(n, generator=g)) ** 2
    zero = torch.arange(n) % 7 == 3
    v[zero], gr[zero] = 0.0, 0.0
    lm = torch.tensor([0.0, 0.5, 1.0, 2.0, 0.125])[torch.randint(0, 5, (n,), generator=g)]
    wm = torch.tensor([0.0, 1.0, 4.0, 0.25, 8.0])[torch.randint(0, 5, (n,), generator=g)]
    return dict(p=p, g=gr, m=m, v=v, lr_mult=lm, wd_mult=wm)


# ------------------------------------------------------------------------------------------------ cases shared by the two tests
# (B, K, T, forms, [(w_loss, squared)]): (1, 1, 2) every frame first or last; (2, 5, 7) T % 3 != 0, lane groups straddle windows, the planted edges;
# (1, 8, 49) K at its maximum, a full workgroup of 48 frames plus one; (2, 5, 145) two workgroups of 256 with a ragged second one, T % 3 == 1;
# (51, 2, 243) 259 partial rows at 48 frames per workgroup: the second trip of loss_finalize_kernel, at the production T
ALL_MODES = [(w, s) for w in (0, 1, 2) for s in (False, True)]
WTA_CASES = [(1, 1, 2, ALL_MODES), (2, 5, 7, ALL_MODES), (1, 8, 49, ALL_MODES), (2, 5, 145, ALL_MODES), (51, 2, 243, [(1, False)])]
WTA_PLANTED = (2, 5, 7)
SINGLE_CASES = [(1, 2), (3, 50), (51, 243)]
RIGID_CASES = [(1, 2), (2, 3), (1, 255), (1, 256), (1, 257), (2, 600), (257, 2)]
AGG_BT = [(1, 1), (1, 127), (2, 64), (3, 43), (3, 100)]
AGG_K = (1, 5, 8)
MPJPE_N = (1, 255, 256, 257, 1024 * 256 + 257)
ADAM_N = (1, 2, 3, 4, 5, 1023, 1025, 2051)
ADAM_STEPS = (1, 2, 1000, 100000)
ADAM_WD_GS = [(0.0, 1.0), (f32(1e-2), 1.0), (0.0, 0.125), (f32(1e-2), 0.125)]


def wta_case_inputs(B, K, T):
    return wta_inputs(B, K, T, 1000 * B + 10 * K + T + 1, planted=(B, K, T) == WTA_PLANTED)


def single_case_inputs(B, T):
    d = wta_inputs(B, 1, T, 77 * B + T)
    return dict(poses=d["poses"][:, 0].contiguous(), y=d["y"])


def rigid_term_key(B, T):
    """the bound constant of the term: the cases made of one rigid window have their own (module docstring)"""
    return "rigid_term_rigid" if B == 1 and T >= 255 else "rigid_term"


def rigid_case_inputs(B, T):
    return rigid_inputs(B, T, 1000 * B + T)


def agg_case_inputs(B, K, T):
    return aggregate_inputs(B, K, T, 100 * B + 10 * K + T + 1)


def mpjpe_case_inputs(n):
    return mpjpe_inputs(n, n)


def adam_case_inputs(n, step):
    return adam_inputs(n, n + step)


def adam_args(d, step, wd, gscale):
    return (d["p"], d["g"], d["m"], d["v"], step, ADAM_HYPER["lr"], ADAM_HYPER["beta1"], ADAM_HYPER["beta2"], ADAM_HYPER["eps"], wd, gscale)


# asserted bound constants, in units of u x the element's scale: bound_from() of the worst error / scale of the plain fp32 CPU evaluation
# over the cases above (the ratio in the comment; test_loss_ref_host.py measures it and checks the constant against it)
BOUNDS = {
    "wta_wloss": 2.0,          # 0.415
    "wta_score_reg": 4.0,      # 0.919
    "wta_vloss": 1.0,          # 0.121
    "wta_sreg": 3.0,           # 0.505
    "wta_d_poses": 5.0,        # 1.09
    "wta_d_scores": 5.0,       # 1.14
    "single_wloss": 3.0,       # 0.56
    "single_vloss": 1.0,       # 0.102
    "single_sreg": 1.0,        # 0.191
    "single_d_poses": 4.0,     # 0.917
    "rigid_term": 2.0,         # 0.379
    "rigid_term_rigid": 5000.0,  # 1.12e+03 (one rigid window: the roundings of the lengths against a variance that is all cancellation)
    "rigid_d_poses": 8.0,      # 1.89
    "agg_weighted_ave": 7.0,   # 1.74
    "mpjpe_sum": 2.0,          # 0.397
    "adam_p": 3.0,             # 0.749
    "adam_m": 4.0,             # 0.923
    "adam_v": 4.0,             # 0.968
}

"""fp64 references of the kernels at the two ends of the network - input embeddings, positional-embedding gradients, score head, bone means,
manifold decoder - with per-element forward-error scales, and the seeded inputs the host and the GPU tests share (no GPU).

Every function takes the fp32 tensors exactly as the kernel receives them and a `dtype`: torch.float64 gives the reference, torch.float32 the
same formula in plain fp32 torch (test_model_ends_ref_host.py measures its error to derive the bound constants of test_gpu_model_ends.py).
A result is a pair (value, scale): an error is asserted per element as |got - value| <= C u scale, u = 2^-24.

Scales (absolute values of the terms a result is summed from, plus the result; a quantity that is itself computed carries its own scale on):
  embeddings    out = W x + b + spos[j]: |w0 x0| + |w1 x1| + |b| + |spos| + |out| (bones: 34 products); sums dW, db, dspos accumulated into a
                seed: sum |terms| + |seed| + |result|
  tpos_grad     seed + sum_{b,j} g: sum |g| + |seed| + |result|
  scores        logit: E = sum_j |w e| + |b| + |logit|; score s_k: s_k (1 + 2 max_k' E_k') + s_k (expf, the division)
                backward, on the fp32 scores the kernel reads: dlogit = s (d - sum s d) has D = |s| (|d| + sum |s d| + |d - sum s d|) + |dlogit|;
                channel O - 1 of dheadout = dlogit w: |w| D + |dlogit w|; dw = seed + sum_f dlogit e: sum_f (D |e| + |dlogit e|) + |seed| + |dw|;
                db = seed + sum_f dlogit: sum_f (D + |dlogit|) + |seed| + |db|
  bone means    mean: sum_t |h| / T + |mean|; backward sum over the K T poses of a window: sum |.| + |sum|
  fk_decode     cond_a = 1 / sin(angle between the two 6-D halves of joint a) (1 for the 4-D representation and where a norm is clamped: the
                clamped formula is a division by the constant 1e-8): the cross product x x b cancels to |b| sin, so a rotation matrix R_a carries
                u cond_a per entry, and a world rotation Rw_i = prod R_a over the chain root .. i carries A_i = sum_{a in chain(i)} cond_a.
                position p_j = sum_{i in chain(j)} Rw_i off_i:   sum_{i in chain(j)} |len_i| A_i + |p_j|
  fk_decode backward (derived the same way).  G_i = the sum of dposes over the subtree of i (joint 0's own row is not read: the root is the
                constant 0), |G_i| <= Gabs_i = sum_{d in subtree(i)} ||dposes_d||_1.
                dlen_i = op_i . Rw_i^T G_i:   Gabs_i A_i + |dlen_i|
                The gradient of R_j is the sum over the bones i of its subtree of G_i off_i^T carried through rotations of chain(i), so its
                entries and their errors are bounded by W_j = sum_{i in subtree(j)} |len_i| Gabs_i A_i (A_i >= cond_j: an error u cond_j of z
                enters squared, once through A_i and once through the division by |x x b| below).  Gram-Schmidt backward, na = max(|a|, eps),
                nz = max(|x x b|, eps), kb = |b| / nz (= cond_j when nothing is clamped):
                    d a = (dx - x (x . dx)) / na, dx gathers b x dzc:   W_j (1 + kb) / na + |d a|
                    d b = dzc x x, dzc = (dz - z (z . dz)) / nz:         W_j / nz + |d b|
                4-D: each unit 2-vector c = r / n:   W_j / max(n, eps) + |d r|
"""
import torch

U24 = 2.0 ** -24
F32_TINY = 2.0 ** -126      # below it fp32 has no relative precision (and a device may flush to zero): the absolute floor of a score's bound
GS_EPS = float(torch.tensor(1e-8, dtype=torch.float32))      # GS_EPS of fk_decode.hip, an fp32 constant
NJ = 17
PARENTS = [-1, 0, 1, 2, 0, 4, 5, 0, 7, 8, 9, 8, 11, 12, 8, 14, 15]
TPOSE_OPS = [[0, 0, 0], [1, 0, 0], [0, -1, 0], [0, -1, 0], [-1, 0, 0], [0, -1, 0], [0, -1, 0], [0, 1, 0], [0, 1, 0], [0, 1, 0], [0, 1, 0],
             [-1, 0, 0], [-1, 0, 0], [-1, 0, 0], [1, 0, 0], [1, 0, 0], [1, 0, 0]]


def _chain_matrix():
    """anc[i][a] = 1 when a is i or an ancestor of i (the root included)"""
    anc = torch.zeros(NJ, NJ, dtype=torch.float64)
    for i in range(NJ):
        a = i
        while a >= 0:
            anc[i, a] = 1.0
            a = PARENTS[a]
    return anc


ANC = _chain_matrix()


def gen(seed):
    return torch.Generator().manual_seed(seed)


def worst(got, want, scale, floor=0.0):
    """largest |got - want| / (u scale + floor) over the elements; NaN / inf anywhere in got gives inf, and so does any error where the scale
    is 0 (an exact zero, such as the root joint, must come out exact)"""
    got = got.detach().cpu().double()
    if not torch.isfinite(got).all():
        return float("inf")
    err, den = (got - want).abs(), U24 * scale + floor
    ratio = torch.where(den > 0, err / den.clamp_min(1e-300), torch.where(err > 0, float("inf"), 0.0).to(err.dtype))
    return ratio.max().item() if got.numel() else 0.0


# ------------------------------------------------------------------------------------------------ embeddings
def embed_inputs(M, C, J, g):
    return dict(x=torch.randn(M, 2, generator=g), W=torch.randn(C, 2, generator=g), b=torch.randn(C, generator=g),
                spos=torch.randn(J, C, generator=g), g=torch.randn(M, C, generator=g) * (0.25 + torch.rand(M, 1, generator=g)),
                sW=torch.randn(C, 2, generator=g), sb=torch.randn(C, generator=g), sspos=torch.randn(J, C, generator=g))


def embed_fwd(x, W, b, spos, J, dtype=torch.float64):
    x, W, b, spos = (t.to(dtype) for t in (x, W, b, spos))
    p = spos[torch.arange(x.shape[0]) % J]
    t0, t1 = x[:, 0:1] * W[:, 0], x[:, 1:2] * W[:, 1]
    out = t0 + t1 + b + p
    return out, t0.abs() + t1.abs() + b.abs() + p.abs() + out.abs()


def embed_bwd(g, x, J, sW, sb, sspos, dtype=torch.float64):
    """the sums over the M // J whole frames (rows past the last whole frame enter no sum, as in the kernels)"""
    g, x, sW, sb, sspos = (t.to(dtype) for t in (g, x, sW, sb, sspos))
    n = (g.shape[0] // J) * J
    g, x = g[:n], x[:n]
    dW = sW + g.t() @ x
    db = sb + g.sum(0)
    gj = g.reshape(-1, J, g.shape[1])
    dsp = sspos + gj.sum(0)
    return (dW, g.abs().t() @ x.abs() + sW.abs() + dW.abs()), (db, g.abs().sum(0) + sb.abs() + db.abs()), \
        (dsp, gj.abs().sum(0) + sspos.abs() + dsp.abs())


def bones_embed_inputs(BT, O, g):
    return dict(x=torch.randn(BT, 34, generator=g), W=torch.randn(O, 34, generator=g), b=torch.randn(O, generator=g),
                spos=torch.randn(O, generator=g), g=torch.randn(BT, O, generator=g) * (0.25 + torch.rand(BT, 1, generator=g)),
                sW=torch.randn(O, 34, generator=g), sb=torch.randn(O, generator=g), sspos=torch.randn(O, generator=g))


def bones_embed_fwd(x, W, b, spos, dtype=torch.float64):
    x, W, b, spos = (t.to(dtype) for t in (x, W, b, spos))
    out = x @ W.t() + b + spos
    return out, x.abs() @ W.abs().t() + b.abs() + spos.abs() + out.abs()


def bones_embed_bwd(g, x, sW, sb, sspos, dtype=torch.float64):
    g, x, sW, sb, sspos = (t.to(dtype) for t in (g, x, sW, sb, sspos))
    dW = sW + g.t() @ x
    cs, acs = g.sum(0), g.abs().sum(0)
    db, dsp = sb + cs, sspos + cs
    return (dW, g.abs().t() @ x.abs() + sW.abs() + dW.abs()), (db, acs + sb.abs() + db.abs()), (dsp, acs + sspos.abs() + dsp.abs())


def tpos_grad(g, seed, B, T, J, dtype=torch.float64):
    g, seed = g.to(dtype), seed.to(dtype)
    g = g.reshape(B, T, J, -1)
    r = seed + g.sum((0, 2))
    return r, g.abs().sum((0, 2)) + seed.abs() + r.abs()


# ------------------------------------------------------------------------------------------------ scores
def score_inputs(K, O, B, T, J, g, pattern="ordinary"):
    """headout (K, B T J, O) with every channel drawn on its own; `equal`: the K heads carry the same score channel, weights and bias;
    `ahead`: head (f % K) of frame f leads every other head by 100 (the others underflow in the softmax)"""
    F = B * T
    h = torch.randn(K, F * J, O, generator=g)
    w = torch.randn(K, J, generator=g) * 0.5
    b = torch.randn(K, generator=g)
    if pattern == "equal":
        h[:, :, O - 1] = h[0, :, O - 1]
        w[:] = w[0]
        b[:] = b[0]
    if pattern == "ahead":
        # add 100 to the leader's logit through the bias-free part: shift its channel along w / |w|^2
        lead = torch.arange(F) % K
        e = h[:, :, O - 1].reshape(K, F, J)
        e[lead, torch.arange(F)] += 100.0 * w[lead] / (w[lead] ** 2).sum(1, keepdim=True)
        h[:, :, O - 1] = e.reshape(K, F * J)
    return dict(h=h.contiguous(), w=w, b=b, d=torch.randn(B, K, T, generator=g), sw=torch.randn(K, J, generator=g), sb=torch.randn(K, generator=g))


def scores_fwd(h, w, b, B, T, J, dtype=torch.float64):
    """-> (scores (B, K, T), scale), (logit (K, B T), E)"""
    K, _, O = h.shape
    e = h[:, :, O - 1].to(dtype).reshape(K, B * T, J)
    w, b = w.to(dtype), b.to(dtype)
    terms = e * w[:, None, :]
    logit = terms.sum(-1) + b[:, None]
    E = terms.abs().sum(-1) + b.abs()[:, None] + logit.abs()
    s = torch.softmax(logit, 0)
    sc = s * (1.0 + 2.0 * E.max(0, keepdim=True).values) + s
    lay = lambda t: t.reshape(K, B, T).permute(1, 0, 2).contiguous()
    return (lay(s), lay(sc)), (logit, E)


def scores_bwd(h, s, d, w, sw, sb, B, T, J, dtype=torch.float64):
    """s: the fp32 scores the kernel reads, d: dscores, both (B, K, T) -> (score channel of dheadout (K, B T J), dw (K, J), db (K)) with scales"""
    K, _, O = h.shape
    F = B * T
    e = h[:, :, O - 1].to(dtype).reshape(K, F, J)
    lay = lambda t: t.to(dtype).permute(1, 0, 2).reshape(K, F)
    s, d, w, sw, sb = lay(s), lay(d), w.to(dtype), sw.to(dtype), sb.to(dtype)
    dot = (s * d).sum(0, keepdim=True)
    dl = s * (d - dot)
    D = s.abs() * (d.abs() + (s * d).abs().sum(0, keepdim=True) + (d - dot).abs()) + dl.abs()
    dh = dl[:, :, None] * w[:, None, :]
    dh_s = D[:, :, None] * w.abs()[:, None, :] + dh.abs()
    dw = sw + (dl[:, :, None] * e).sum(1)
    dw_s = (D[:, :, None] * e.abs() + (dl[:, :, None] * e).abs()).sum(1) + sw.abs() + dw.abs()
    db = sb + dl.sum(1)
    db_s = (D + dl.abs()).sum(1) + sb.abs() + db.abs()
    return (dh.reshape(K, F * J), dh_s.reshape(K, F * J)), (dw, dw_s), (db, db_s)


# ------------------------------------------------------------------------------------------------ bone means
def bones_mean_fwd(h, B, T, S, dtype=torch.float64):
    h = h.to(dtype).reshape(B, T, S)
    m = h.sum(1) / T
    return m, h.abs().sum(1) / T + m.abs()


def bones_mean_bwd(dlp, B, KT, S, dtype=torch.float64):
    """-> dlengths (B, S) and its scale; dheadout[(b, t, s)] = dlengths / T"""
    dlp = dlp.to(dtype).reshape(B, KT, S)
    r = dlp.sum(1)
    return r, dlp.abs().sum(1) + r.abs()


# ------------------------------------------------------------------------------------------------ manifold decoder
def fk_inputs(B, K, T, rot_dim, stride, g, zero_halves=True):
    """rot (K, B T 17, stride) in the engine's row order (k, b, t, j), lengths (B, 16), dposes (B, K, T, 17, 3).  6-D: the halves have norms
    in [0.5, 2] and a mutual angle in [30, 150] degrees; 4-D: each 2-vector a norm in [0.5, 2].  Padding channels hold noise.  With
    zero_halves a few joints get an exactly zero half (the clamp branches)."""
    M = B * T * NJ
    n = K * M
    rot = torch.randn(K, M, stride, generator=g)
    if rot_dim == 6:
        u = torch.nn.functional.normalize(torch.randn(n, 3, generator=g, dtype=torch.float64), dim=1)
        v = torch.randn(n, 3, generator=g, dtype=torch.float64)
        v = torch.nn.functional.normalize(v - u * (u * v).sum(1, keepdim=True), dim=1)
        ang = torch.deg2rad(30.0 + 120.0 * torch.rand(n, 1, generator=g, dtype=torch.float64))
        na, nb = (0.5 + 1.5 * torch.rand(n, 1, generator=g, dtype=torch.float64) for _ in range(2))
        r = torch.cat([na * u, nb * (torch.cos(ang) * u + torch.sin(ang) * v)], 1)
    else:
        ang = 6.283185307179586 * torch.rand(n, 2, generator=g, dtype=torch.float64)
        nn = 0.5 + 1.5 * torch.rand(n, 2, generator=g, dtype=torch.float64)
        r = torch.stack([nn[:, 0] * torch.cos(ang[:, 0]), nn[:, 0] * torch.sin(ang[:, 0]), nn[:, 1] * torch.cos(ang[:, 1]),
                         nn[:, 1] * torch.sin(ang[:, 1])], 1)
    rot[:, :, :rot_dim] = r.float().reshape(K, M, rot_dim)
    if zero_halves and n >= 4 * NJ:
        h = rot_dim // 2
        flat = rot.reshape(n, stride)
        for i, row in enumerate(torch.randperm(n, generator=g)[:6].tolist()):
            flat[row, (i % 2) * h:(i % 2) * h + h] = 0.0
    lengths = 0.1 + 0.4 * torch.rand(B, NJ - 1, generator=g)
    dposes = torch.randn(B, K, T, NJ, 3, generator=g) * (0.25 + torch.rand(B, K, T, NJ, 1, generator=g))
    return dict(rot=rot.contiguous(), lengths=lengths, dposes=dposes)


def _cross(u, v):
    return torch.stack([u[..., 1] * v[..., 2] - u[..., 2] * v[..., 1], u[..., 2] * v[..., 0] - u[..., 0] * v[..., 2],
                        u[..., 0] * v[..., 1] - u[..., 1] * v[..., 0]], -1)


def _norm(v):
    return torch.linalg.vector_norm(v, dim=-1, keepdim=True)      # subgradient 0 at the zero vector, as the kernels' clamp branch


def rotations(r, rot_dim):
    """(..., rot_dim) -> (..., 3, 3) with the max(norm, 1e-8) clamps of fk_decode.hip"""
    if rot_dim == 6:
        a, b = r[..., :3], r[..., 3:6]
        x = a / _norm(a).clamp_min(GS_EPS)
        zc = _cross(x, b)
        z = zc / _norm(zc).clamp_min(GS_EPS)
        return torch.stack([x, _cross(z, x), z], -1)
    p, q = r[..., 0:2], r[..., 2:4]
    p, q = p / _norm(p).clamp_min(GS_EPS), q / _norm(q).clamp_min(GS_EPS)
    c1, s1, c2, s2 = p[..., 0], p[..., 1], q[..., 0], q[..., 1]
    zero = torch.zeros_like(c1)
    return torch.stack([torch.stack([s1, c1 * c2, -(c1 * s2)], -1), torch.stack([-c1, s1 * c2, -(s1 * s2)], -1),
                        torch.stack([zero, s2, c2], -1)], -2)


def _rows(rot, B, K, T, rot_dim):
    """engine rows (k, b, t, j) -> (B, K, T, 17, rot_dim)"""
    return rot[..., :rot_dim].reshape(K, B, T, NJ, rot_dim).permute(1, 0, 2, 3, 4)


def fk_forward(rot, lengths, B, K, T, rot_dim):
    """poses (B, K, T, 17, 3) in the dtype of rot; differentiable"""
    R = rotations(_rows(rot, B, K, T, rot_dim), rot_dim)
    ops = torch.tensor(TPOSE_OPS, dtype=rot.dtype)
    ln = torch.cat([torch.zeros(B, 1, dtype=rot.dtype), lengths], 1)
    off = (ops[None] * ln[:, :, None])[:, None, None]                      # (B, 1, 1, 17, 3)
    Rw, p = [R[..., 0, :, :]], [torch.zeros(B, K, T, 3, dtype=rot.dtype)]
    for j in range(1, NJ):
        pa = PARENTS[j]
        rw = Rw[pa] @ R[..., j, :, :]
        Rw.append(rw)
        p.append((rw @ off[..., j, :, None].expand(B, K, T, 3, 1))[..., 0] + p[pa])
    return torch.stack(p, -2)


def fk_reference(rot, lengths, dposes, B, K, T, rot_dim, dtype=torch.float64):
    """-> (poses, scale), (drot (K, M, rot_dim), scale), (dlen_pose (B, K, T, 16), scale); the backward is autograd of fk_forward"""
    rd = rot.to(dtype).clone().requires_grad_(True)
    lb = lengths.to(dtype)[:, None, None, :].expand(B, K, T, NJ - 1).clone().requires_grad_(True)     # a length per pose: dlen_pose
    R = rotations(_rows(rd, B, K, T, rot_dim), rot_dim)
    ops = torch.tensor(TPOSE_OPS, dtype=dtype)
    ln = torch.cat([torch.zeros(B, K, T, 1, dtype=dtype), lb], -1)
    off = ops * ln[..., None]
    Rw, p = [R[..., 0, :, :]], [torch.zeros(B, K, T, 3, dtype=dtype)]
    for j in range(1, NJ):
        rw = Rw[PARENTS[j]] @ R[..., j, :, :]
        Rw.append(rw)
        p.append((rw @ off[..., j, :, None])[..., 0] + p[PARENTS[j]])
    poses = torch.stack(p, -2)
    dp = dposes.to(dtype).clone()
    dp[..., 0, :] = 0.0                                                     # the root is the constant 0
    drot, dlen = torch.autograd.grad(poses, (rd, lb), dp)
    poses, drot = poses.detach(), drot[..., :rot_dim].detach()
    if dtype != torch.float64:
        return (poses, None), (drot, None), (dlen, None)
    # ---- scales (module docstring)
    r = _rows(rot.double(), B, K, T, rot_dim)
    anc = ANC
    if rot_dim == 6:
        a, b = r[..., :3], r[..., 3:6]
        na, nb = _norm(a)[..., 0], _norm(b)[..., 0]
        x = a / na.clamp_min(GS_EPS)[..., None]
        nz = _norm(_cross(x, b))[..., 0]
        ok = (na > GS_EPS) & (nz > GS_EPS)
        cond = torch.where(ok, nb / nz.clamp_min(GS_EPS), torch.ones_like(na))
    else:
        na, nb = _norm(r[..., 0:2])[..., 0], _norm(r[..., 2:4])[..., 0]
        cond = torch.ones_like(na)
    A = cond @ anc.t()                                                     # (B, K, T, 17): sum over chain(i)
    al = torch.cat([torch.zeros(B, 1, dtype=torch.float64), lengths.double().abs()], 1)[:, None, None, :]
    pose_s = ((al * A) @ anc.t())[..., None] + poses.abs()
    gabs = dp.abs().sum(-1) @ anc                                          # subtree sums
    dlen_s = (gabs * A)[..., 1:] + dlen.abs()
    W = (al * gabs * A) @ anc
    if rot_dim == 6:
        ina, inz = 1.0 / na.clamp_min(GS_EPS), 1.0 / nz.clamp_min(GS_EPS)
        sa, sb = W * (1.0 + nb * inz) * ina, W * inz
        s = torch.cat([sa[..., None].expand(*sa.shape, 3), sb[..., None].expand(*sb.shape, 3)], -1)
    else:
        sa, sb = W / na.clamp_min(GS_EPS), W / nb.clamp_min(GS_EPS)
        s = torch.cat([sa[..., None].expand(*sa.shape, 2), sb[..., None].expand(*sb.shape, 2)], -1)
    drot_s = s.permute(1, 0, 2, 3, 4).reshape(K, B * T * NJ, rot_dim) + drot.abs()
    return (poses, pose_s), (drot, drot_s), (dlen.detach(), dlen_s)


# ------------------------------------------------------------------------------------------------ shapes and bounds shared by the two tests
EMBED17_FRAMES = (1, 2, 3, 7, 513, 486)          # embed_bwd4_kernel<17>: 1 chunk with frame group 1 idle .. 256 chunks of 3 frames, 85 of them empty
EMBED17_C = (32, 128, 512, 516)                  # C / 4 = 129: a second column block with one live column
EMBED_GENERIC = [(16, 16 * f, C) for f in (1, 5, 129) for C in (32, 260)] + [(17, 17 * 5 + 3, 32)]      # (J, M, C); the last: M % 17 != 0
BONES_EMBED_BT = (1, 31, 32, 33, 65, 486)
BONES_EMBED_O = (256, 384, 512)
TPOS = [(1, 1, 17, 32), (2, 9, 17, 128), (3, 5, 16, 512), (2, 4, 4, 260), (1, 3, 5, 64)]               # (B, T, J, C)
TPOS_REFUSED = [(2, 5, 3, 32), (3, 2, 1, 32)]
# (K, O, J, B, T, pattern): B T = 1, 127, 128, 129, 486 and 24577 = 96 * 256 + 1 (one wrap of the scores_param_kernel stride)
SCORES = [(1, 7, 17, 1, 1, "ordinary"), (3, 7, 17, 1, 127, "ordinary"), (5, 5, 16, 2, 64, "ordinary"), (8, 1, 32, 3, 43, "ordinary"),
          (5, 7, 17, 2, 243, "ordinary"), (3, 5, 17, 7, 3511, "ordinary"), (8, 7, 32, 1, 127, "ordinary"), (5, 7, 17, 2, 243, "equal"),
          (8, 5, 16, 3, 43, "equal"), (5, 7, 17, 2, 243, "ahead"), (8, 1, 32, 3, 43, "ahead"), (3, 7, 17, 1, 127, "ahead")]
# (B, K, T, S): K T below 256 / S, not a multiple of 4 (256 / S), and 1215
BONES_MEAN = [(2, 1, 1, 16), (3, 5, 9, 17), (2, 5, 243, 16), (3, 1, 9, 32), (2, 5, 243, 32), (4, 1, 243, 17), (2, 5, 1, 32)]
FK_BKT = [(1, 1, 1), (2, 5, 7), (3, 4, 3), (2, 8, 27)]      # 70 poses: one live slot in the tail wave; 36: whole waves, not whole workgroups
FK_REPS = [(6, 6), (6, 7), (4, 4), (4, 5)]                   # (rot_dim, stride)


def bound_from(ratio):
    """the asserted constant of a quantity whose plain fp32 evaluation on the CPU has the worst error / scale `ratio`: 4 x ratio (another,
    equally valid summation order and FMA contraction), rounded up to one significant digit, never below 1"""
    import math
    v = 4.0 * ratio
    if v <= 1.0:
        return 1.0
    p = 10.0 ** math.floor(math.log10(v))
    return math.ceil(v / p - 1e-9) * p


# asserted bound constants, in units of u x the element's scale: bound_from() of the worst error / scale of the plain fp32 CPU evaluation
# over the shapes above (the ratio in the comment; test_model_ends_ref_host.py measures it and checks the constant against it)
BOUNDS = {
    "embed_fwd": 7.0,          # 1.69
    "embed_dW": 9.0,           # 2.13
    "embed_db": 7.0,           # 1.70
    "embed_dspos": 7.0,        # 1.60
    "bones_embed_fwd": 20.0,   # 3.31
    "bones_embed_dW": 20.0,    # 2.86
    "bones_embed_db": 6.0,     # 1.28
    "bones_embed_dspos": 5.0,  # 1.19
    "tpos_grad": 5.0,          # 1.04
    "scores": 5.0,             # 1.04
    "scores_dheadout": 6.0,    # 1.42
    "scores_dw": 2.0,          # 0.349
    "scores_db": 1.0,          # 0.161
    "bones_mean_fwd": 4.0,     # 0.997
    "bones_mean_bwd": 5.0,     # 1.14
    "fk6_poses": 5.0,          # 1.18
    "fk6_drot": 3.0,           # 0.602
    "fk6_dlen": 3.0,           # 0.704
    "fk4_poses": 5.0,          # 1.21
    "fk4_drot": 4.0,           # 0.864
    "fk4_dlen": 3.0,           # 0.748
}

"""Kernel-level tests of the two ends of the network, each through the C entry point that calls the engine's own launcher
(include/manipose_hip.h): embed_fwd / embed_bwd (embed_bwd4_kernel<17>, the generic embed_bwd_kernel, reduce_partials_kernel),
bones_embed_fwd / bones_embed_bwd, tpos_grad, scores_fwd / scores_bwd (scores_param_kernel, scores_param_fin_kernel, the parameter stream),
bones_mean_fwd / bones_mean_bwd, and fk_decode in the engine's layout (K hypotheses, rows (k, b, t, j), poses (b, k, t), strided channels).

Every value is compared PER ELEMENT with fp64 of the exact fp32 inputs the kernel received, against that element's own forward-error scale
(tests/ends_ref.py: formulas and scales), never against a tensor-wide maximum: one wrong frame, chunk or joint cannot hide.  Inputs come
from seeded generators, no value is shared between samples, frames, joints or heads, outputs start as NaN (behind them a guard of
sentinels that must survive), accumulated gradients start from non-zero seeds, and untouched channels are compared bit for bit.

Bound constants (ends_ref.BOUNDS), in units of u = 2^-24 times the scale.  They are NOT fitted to the kernels: each is 4 x the worst
error / scale of the same formula evaluated in plain fp32 torch on the CPU over this module's shapes (the factor 4: another, equally valid
summation order and FMA contraction), rounded up to one significant digit, never below 1; test_model_ends_ref_host.py measures the ratios:
    quantity             fp32 CPU ratio   bound        quantity             fp32 CPU ratio   bound
    embed_fwd            1.69             7            scores               1.04             5
    embed_dW             2.13             9            scores_dheadout      1.42             6
    embed_db             1.70             7            scores_dw            0.349            2
    embed_dspos          1.60             7            scores_db            0.161            1
    bones_embed_fwd      3.31             20           bones_mean_fwd       0.997            4
    bones_embed_dW       2.86             20           bones_mean_bwd       1.14             5
    bones_embed_db       1.28             6            fk6_poses / fk4      1.18 / 1.21      5 / 5
    bones_embed_dspos    1.19             5            fk6_drot / fk4       0.602 / 0.864    3 / 4
    tpos_grad            1.04             5            fk6_dlen / fk4       0.704 / 0.748    3 / 3
A score (and a product with one in the backward) additionally gets the absolute floor 2^-126: below the smallest normal fp32 has no
relative precision and a device may flush to zero.  Every test prints its measured worst ratio next to the bound."""
import pytest
import torch

import ends_ref as er
from test_gpu_parity import st

pytestmark = pytest.mark.gpu

ERR_ARG = 1
GUARD = 256
SENTINEL = 12345.678


def report(name, ratio, key):
    bound = er.BOUNDS[key]
    print(f"[model ends] {name}: worst error / scale {ratio:.3g} u (asserted <= {bound:g})")
    assert ratio <= bound, (name, ratio, bound)


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b, what):
    assert a.shape == b.shape, what
    bad = int((bits(a) != bits(b)).sum())
    assert bad == 0, f"{what}: {bad} elements differ"


class Buf:
    """a device buffer of `shape` followed by GUARD sentinel floats that no kernel may touch; `init`: None = NaN, a tensor = its values"""

    def __init__(self, shape, init=None):
        n = 1
        for s in shape:
            n *= s
        self.raw = torch.full((n + GUARD,), SENTINEL, device="cuda")
        self.t = self.raw[:n].view(*shape)
        if init is None:
            self.t.fill_(float("nan"))
        else:
            self.t.copy_(init)
        self.p = self.raw.data_ptr()

    def ok(self, what):
        assert bool((self.raw[-GUARD:] == torch.tensor(SENTINEL, device="cuda")).all()), f"{what}: wrote past its end"
        return self.t

    def untouched(self, init, what):
        self.ok(what)
        if init is None:
            assert bool(torch.isnan(self.t).all()), f"{what}: written by a refused call"
        else:
            same_bits(self.t, init.cuda(), f"{what}: changed by a refused call")


def dev(t):
    return t.cuda().contiguous()


def check(lib, rc, what):
    from manipose_amd import _lib
    _lib.check(rc, what)


# ------------------------------------------------------------------------------------------------ embeddings
def run_embed(lib, d, M, C, J, what):
    x, W, b, spos, g = (dev(d[k]) for k in ("x", "W", "b", "spos", "g"))
    out = Buf((M, C))
    check(lib, lib.mp_embed_fwd_ex(x.data_ptr(), W.data_ptr(), b.data_ptr(), spos.data_ptr(), out.p, M, C, J, st()), "mp_embed_fwd_ex")
    n = lib.mp_embed_bwd_scratch_floats(C, J)
    assert n == 256 * (3 + J) * C
    scratch = Buf((n,))
    res = []
    for _ in range(2):
        dW, db, dsp = Buf((C, 2), d["sW"]), Buf((C,), d["sb"]), Buf((J, C), d["sspos"])
        check(lib, lib.mp_embed_bwd_ex(g.data_ptr(), x.data_ptr(), dW.p, db.p, dsp.p, M, C, J, scratch.p, n, st()), "mp_embed_bwd_ex")
        torch.cuda.synchronize()
        res.append([t.ok(what).clone() for t in (dW, db, dsp)])
    scratch.ok(what + " scratch")
    for a, b2, k in zip(res[0], res[1], ("dW", "db", "dspos")):
        same_bits(a, b2, f"{what}: {k} of two calls")
    report(f"embed_fwd {what}", er.worst(out.ok(what), *er.embed_fwd(d["x"], d["W"], d["b"], d["spos"], J)), "embed_fwd")
    for got, ref, k in zip(res[0], er.embed_bwd(d["g"], d["x"], J, d["sW"], d["sb"], d["sspos"]), ("dW", "db", "dspos")):
        report(f"embed {k} {what}", er.worst(got, *ref), "embed_" + k)


@pytest.mark.parametrize("frames", er.EMBED17_FRAMES)
def test_embed_j17_four_channel_kernel(lib, frames):
    """embed_bwd4_kernel<17>: chunks = max(1, min(256, frames / 2)) of ceil(frames / chunks) frames, two frame groups per chunk."""
    for C in er.EMBED17_C:
        M = 17 * frames
        run_embed(lib, er.embed_inputs(M, C, 17, er.gen(1000 * frames + C)), M, C, 17, f"J=17 frames={frames} C={C}")


@pytest.mark.parametrize("J,M,C", er.EMBED_GENERIC)
def test_embed_generic_kernel(lib, J, M, C):
    """embed_bwd_kernel (a thread per channel); J = 17 with M % 17 != 0 takes it too and sums the whole frames only (the rows of the partial
    frame carry gradients eight times the others: adding any of them fails every sum)."""
    d = er.embed_inputs(M, C, J, er.gen(7 * M + C + J))
    if M % J:
        d["g"][(M // J) * J:] *= 8.0
    run_embed(lib, d, M, C, J, f"J={J} M={M} C={C}")


@pytest.mark.parametrize("BT", er.BONES_EMBED_BT)
def test_bones_embed(lib, BT):
    """bones_embed_fwd (32 frames per workgroup, the last one partial) and bones_embed_bwd (min(32, BT) chunks, reduce_partials_kernel twice)."""
    for O in er.BONES_EMBED_O:
        what = f"BT={BT} O={O}"
        d = er.bones_embed_inputs(BT, O, er.gen(31 * BT + O))
        x, W, b, spos, g = (dev(d[k]) for k in ("x", "W", "b", "spos", "g"))
        out = Buf((BT, O))
        check(lib, lib.mp_bones_embed_fwd_ex(x.data_ptr(), W.data_ptr(), b.data_ptr(), spos.data_ptr(), out.p, BT, 34, O, st()), "mp_bones_embed_fwd_ex")
        n = (min(32, BT) + 1) * O * 35
        scratch = Buf((n,))
        res = []
        for _ in range(2):
            dW, db, dsp = Buf((O, 34), d["sW"]), Buf((O,), d["sb"]), Buf((O,), d["sspos"])
            check(lib, lib.mp_bones_embed_bwd_ex(g.data_ptr(), x.data_ptr(), dW.p, db.p, dsp.p, BT, 34, O, scratch.p, n, st()), "mp_bones_embed_bwd_ex")
            torch.cuda.synchronize()
            res.append([t.ok(what).clone() for t in (dW, db, dsp)])
        scratch.ok(what + " scratch")
        for a, b2, k in zip(res[0], res[1], ("dW", "db", "dspos")):
            same_bits(a, b2, f"{what}: {k} of two calls")
        report(f"bones_embed_fwd {what}", er.worst(out.ok(what), *er.bones_embed_fwd(d["x"], d["W"], d["b"], d["spos"])), "bones_embed_fwd")
        for got, ref, k in zip(res[0], er.bones_embed_bwd(d["g"], d["x"], d["sW"], d["sb"], d["sspos"]), ("dW", "db", "dspos")):
            report(f"bones_embed {k} {what}", er.worst(got, *ref), "bones_embed_" + k)


# ------------------------------------------------------------------------------------------------ tpos_grad
@pytest.mark.parametrize("B,T,J,C", er.TPOS)
def test_tpos_grad(lib, B, T, J, C):
    g = er.gen(B + 10 * T + 100 * J + C)
    gg, seed = torch.randn(B * T * J, C, generator=g), torch.randn(T, C, generator=g)
    out = Buf((T, C), seed)
    check(lib, lib.mp_tpos_grad_ex(dev(gg).data_ptr(), out.p, B, T, J, C, st()), "mp_tpos_grad_ex")
    torch.cuda.synchronize()
    report(f"tpos_grad B={B} T={T} J={J} C={C}", er.worst(out.ok("dtpos"), *er.tpos_grad(gg, seed, B, T, J)), "tpos_grad")


@pytest.mark.parametrize("B,T,J,C", er.TPOS_REFUSED)
def test_tpos_grad_refuses_fewer_than_four_rows_per_frame(lib, B, T, J, C):
    """J < 4: row group 3 of the kernel would start past the frame.  The launcher refuses; dtpos keeps its bits (a wrong sum is never accepted:
    if the call is ever allowed, it has to give the exact sums)."""
    g = er.gen(J)
    gg, seed = torch.randn(B * T * J, C, generator=g), torch.randn(T, C, generator=g)
    out = Buf((T, C), seed)
    rc = lib.mp_tpos_grad_ex(dev(gg).data_ptr(), out.p, B, T, J, C, st())
    torch.cuda.synchronize()
    if rc == 0:
        report(f"tpos_grad J={J}", er.worst(out.ok("dtpos"), *er.tpos_grad(gg, seed, B, T, J)), "tpos_grad")
    else:
        assert rc == ERR_ARG and b"J=" in lib.mp_last_error()
        out.untouched(seed, "dtpos")


# ------------------------------------------------------------------------------------------------ scores
def run_scores_bwd(lib, d, dv, s_dev, K, O, B, T, J, init, pstream=None, scratch_floats=None):
    n = lib.mp_scores_bwd_scratch_floats(K, B, T)
    assert n == K * B * T + K * 96 * 33
    scratch = Buf((n,))
    dh, dw, db = Buf((K, B * T * J, O), init), Buf((K, J), d["sw"]), Buf((K,), d["sb"])
    rc = lib.mp_scores_bwd_ex(dv["h"].data_ptr(), s_dev.data_ptr(), dv["d"].data_ptr(), dv["w"].data_ptr(), dv["b"].data_ptr(), dw.p, db.p, K, O, dh.p,
                              B, T, J, scratch.p, n if scratch_floats is None else scratch_floats, pstream, st())
    torch.cuda.synchronize()
    scratch.ok("scores scratch")
    return rc, dh, dw, db


@pytest.mark.parametrize("K,O,J,B,T,pattern", er.SCORES)
def test_scores(lib, K, O, J, B, T, pattern):
    what = f"K={K} O={O} J={J} B={B} T={T} {pattern}"
    F = B * T
    d = er.score_inputs(K, O, B, T, J, er.gen(K + 10 * O + 100 * J + 1000 * F), pattern)
    dv = {k: dev(v) for k, v in d.items()}
    sc = Buf((B, K, T))
    check(lib, lib.mp_scores_fwd_ex(dv["h"].data_ptr(), dv["w"].data_ptr(), dv["b"].data_ptr(), K, O, sc.p, B, T, J, st()), "mp_scores_fwd_ex")
    torch.cuda.synchronize()
    s = sc.ok(what).cpu()
    (want, scale), _ = er.scores_fwd(d["h"], d["w"], d["b"], B, T, J)
    assert bool(torch.isfinite(s).all())
    report(f"scores {what}", er.worst(s, want, scale, er.F32_TINY), "scores")
    if pattern == "ahead":
        dev1 = (s.double().sum(1) - 1.0).abs().max().item()
        print(f"  sum of the scores: worst |sum - 1| {dev1 / er.U24:.3g} u (asserted <= K = {K})")
        assert dev1 <= K * er.U24
        lead = (torch.arange(F) % K).reshape(B, T)
        assert bool((s.argmax(1) == lead).all()) and (K == 1 or float(s.sum(1).sub(s.max(1).values).max()) < 1e-30)
    if pattern == "equal":
        assert bool((bits(s) == bits(s[:, :1].expand(B, K, T))).all()), "equal heads, different scores"
    # backward on the kernel's own fp32 scores; the other channels of dheadout hold noise that must survive bit for bit
    init = torch.randn(K, F * J, O, generator=er.gen(F))
    init[:, :, O - 1] = float("nan")
    rc, dh, dw, db = run_scores_bwd(lib, d, dv, sc.t, K, O, B, T, J, init)
    check(lib, rc, "mp_scores_bwd_ex")
    got = dh.ok(what).cpu()
    if O > 1:
        same_bits(got[:, :, :O - 1], init[:, :, :O - 1], f"{what}: channels of dheadout the score head does not own")
    refs = er.scores_bwd(d["h"], s, d["d"], d["w"], d["sw"], d["sb"], B, T, J)
    report(f"scores dheadout {what}", er.worst(got[:, :, O - 1], *refs[0], er.F32_TINY), "scores_dheadout")
    report(f"scores dw {what}", er.worst(dw.ok(what), *refs[1], er.F32_TINY), "scores_dw")
    report(f"scores db {what}", er.worst(db.ok(what), *refs[2], er.F32_TINY), "scores_db")
    # two calls, and a call whose parameter kernels run on a second stream, give the same bits
    side = torch.cuda.Stream()
    for name, ps in (("repeated", None), ("parameter stream", side.cuda_stream)):
        rc, dh2, dw2, db2 = run_scores_bwd(lib, d, dv, sc.t, K, O, B, T, J, init, pstream=ps)
        check(lib, rc, "mp_scores_bwd_ex")
        side.synchronize()
        same_bits(dh2.t[:, :, O - 1], dh.t[:, :, O - 1], f"{what}: dheadout, {name}")
        same_bits(dw2.ok(what), dw.t, f"{what}: dw, {name}")
        same_bits(db2.ok(what), db.t, f"{what}: db, {name}")


def test_scores_refusals(lib):
    """K = 9, J = 33 and a short scratch are refused before any launch: every output keeps its bits"""
    O, B, T = 3, 2, 5
    for K, J, short in ((9, 17, 0), (3, 33, 0), (3, 17, 1)):
        g = er.gen(K + J)
        d = dict(h=torch.randn(K, B * T * J, O, generator=g), w=torch.randn(K, J, generator=g), b=torch.randn(K, generator=g),
                 d=torch.randn(B, K, T, generator=g), sw=torch.randn(K, J, generator=g), sb=torch.randn(K, generator=g))
        dv = {k: dev(v) for k, v in d.items()}
        sc = Buf((B, K, T))
        if not short:
            assert lib.mp_scores_fwd_ex(dv["h"].data_ptr(), dv["w"].data_ptr(), dv["b"].data_ptr(), K, O, sc.p, B, T, J, st()) == ERR_ARG
            torch.cuda.synchronize()
            sc.untouched(None, f"scores K={K} J={J}")
        init = torch.randn(K, B * T * J, O, generator=g)
        s_in = dev(torch.softmax(torch.randn(B, K, T, generator=g), 1))
        n = K * B * T + K * 96 * 33
        rc, dh, dw, db = run_scores_bwd(lib, d, dv, s_in, K, O, B, T, J, init, scratch_floats=n - 1 if short else n)
        assert rc == ERR_ARG, (K, J, short)
        dh.untouched(init, "dheadout")
        dw.untouched(d["sw"], "dw")
        db.untouched(d["sb"], "db")
    assert lib.mp_scores_bwd_scratch_floats(9, 0, 5) == 0


# ------------------------------------------------------------------------------------------------ bone means
@pytest.mark.parametrize("B,K,T,S", er.BONES_MEAN)
def test_bones_mean(lib, B, K, T, S):
    what = f"B={B} K={K} T={T} S={S}"
    KT = K * T
    g = er.gen(B + 10 * K + 100 * T + 1000 * S)
    h, dlp = torch.randn(B * T * S, generator=g), torch.randn(B * KT, S, generator=g)
    ln = Buf((B, S))
    check(lib, lib.mp_bones_mean_fwd_ex(dev(h).data_ptr(), ln.p, B, T, S, st()), "mp_bones_mean_fwd_ex")
    torch.cuda.synchronize()
    report(f"bones_mean_fwd {what}", er.worst(ln.ok(what), *er.bones_mean_fwd(h, B, T, S)), "bones_mean_fwd")
    want, scale = er.bones_mean_bwd(dlp, B, KT, S)
    d_dlp = dev(dlp)
    dl, dh, dh0 = Buf((B, S)), Buf((B, T, S)), Buf((B, T, S))
    check(lib, lib.mp_bones_mean_bwd_ex(d_dlp.data_ptr(), KT, dl.p, dh.p, B, T, S, st()), "mp_bones_mean_bwd_ex")
    check(lib, lib.mp_bones_mean_bwd_ex(d_dlp.data_ptr(), KT, None, dh0.p, B, T, S, st()), "mp_bones_mean_bwd_ex (no dlengths)")     # the engine's form
    torch.cuda.synchronize()
    report(f"bones_mean_bwd dlengths {what}", er.worst(dl.ok(what), want, scale), "bones_mean_bwd")
    same_bits(dh.ok(what).cpu(), (dl.t.cpu() / torch.tensor(float(T)))[:, None, :].expand(B, T, S).contiguous(), f"{what}: dheadout != fp32(dlengths / T)")
    same_bits(dh0.ok(what), dh.t, f"{what}: dheadout without dlengths")
    report(f"bones_mean_bwd dheadout {what}", er.worst(dh0.t, (want / T)[:, None, :].expand(B, T, S), (scale / T)[:, None, :].expand(B, T, S)), "bones_mean_bwd")


# ------------------------------------------------------------------------------------------------ fk_decode, engine layout
@pytest.mark.parametrize("rot_dim,stride", er.FK_REPS)
@pytest.mark.parametrize("B,K,T", er.FK_BKT)
def test_fk_decode_engine_layout(lib, B, K, T, rot_dim, stride):
    """K hypotheses, rows (k, b, t, j) with `stride` channels, poses in (b, k, t) order, lengths per window; a few joints with an exactly zero
    half run the clamp branches (from 4 poses up).  Near-colinear halves stay out (test_gpu_parity.py explains why)."""
    what = f"B={B} K={K} T={T} rot {rot_dim}/{stride}"
    N, M = B * K * T, B * T * 17
    d = er.fk_inputs(B, K, T, rot_dim, stride, er.gen(N + 10 * rot_dim + stride))
    rot, lengths, dposes = dev(d["rot"]), dev(d["lengths"]), dev(d["dposes"])
    poses = Buf((B, K, T, 17, 3))
    check(lib, lib.mp_fk_decode_fwd(rot.data_ptr(), stride, rot_dim, lengths.data_ptr(), poses.p, B, K, T, st()), "mp_fk_decode_fwd")
    init = torch.randn(K, M, stride, generator=er.gen(N))
    drot, dlen = Buf((K, M, stride), init), Buf((N, 16))
    check(lib, lib.mp_fk_decode_bwd(rot.data_ptr(), stride, rot_dim, lengths.data_ptr(), dposes.data_ptr(), drot.p, dlen.p, B, K, T, st()), "mp_fk_decode_bwd")
    torch.cuda.synchronize()
    (p_ref, p_s), (r_ref, r_s), (l_ref, l_s) = er.fk_reference(d["rot"], d["lengths"], d["dposes"], B, K, T, rot_dim)
    p = poses.ok(what).cpu()
    assert bool((bits(p[..., 0, :]) == 0).all()), "the root joint is not exactly +0"
    key = f"fk{rot_dim}_"
    report(f"fk poses {what}", er.worst(p, p_ref, p_s), key + "poses")
    got = drot.ok(what).cpu()
    if stride > rot_dim:
        same_bits(got[..., rot_dim:], init[..., rot_dim:], f"{what}: padding channel of drot")
    report(f"fk drot {what}", er.worst(got[..., :rot_dim], r_ref, r_s), key + "drot")
    report(f"fk dlen_pose {what}", er.worst(dlen.ok(what).view(B, K, T, 16), l_ref, l_s), key + "dlen")


# ------------------------------------------------------------------------------------------------ refusals
def test_bad_arguments_are_refused_before_any_launch(lib):
    """every new entry point: null pointers, non-positive dimensions and the documented limits return MP_ERR_ARG and leave the outputs alone;
    the same calls with good arguments then run"""
    g = er.gen(99)
    M, C, J, BT, O = 34, 32, 17, 5, 256
    e, be = er.embed_inputs(M, C, J, g), er.bones_embed_inputs(BT, O, g)
    ev, bev = {k: dev(v) for k, v in e.items()}, {k: dev(v) for k, v in be.items()}
    n_e, n_b = lib.mp_embed_bwd_scratch_floats(C, J), (min(32, BT) + 1) * O * 35
    scratch = Buf((max(n_e, n_b),))
    B, T, S, KT = 2, 3, 16, 6
    hm, dlp, tg = dev(torch.randn(B * T * S, generator=g)), dev(torch.randn(B * KT, S, generator=g)), dev(torch.randn(B * T * J, C, generator=g))
    tseed = torch.randn(T, C, generator=g)
    outs = dict(out=Buf((M, C)), dW=Buf((C, 2), e["sW"]), db=Buf((C,), e["sb"]), dsp=Buf((J, C), e["sspos"]), bout=Buf((BT, O)),
                bdW=Buf((O, 34), be["sW"]), bdb=Buf((O,), be["sb"]), bdsp=Buf((O,), be["sspos"]), tp=Buf((T, C), tseed), ln=Buf((B, S)),
                dl=Buf((B, S)), dh=Buf((B, T, S)))
    inits = dict(out=None, dW=e["sW"], db=e["sb"], dsp=e["sspos"], bout=None, bdW=be["sW"], bdb=be["sb"], bdsp=be["sspos"], tp=tseed, ln=None,
                 dl=None, dh=None)
    K, SO = 3, 7
    sd = er.score_inputs(K, SO, B, T, J, g)
    sv = {k: dev(v) for k, v in sd.items()}
    s_in = torch.softmax(torch.randn(B, K, T, generator=g), 1)
    s_dev, dh_init = dev(s_in), torch.randn(K, B * T * J, SO, generator=g)
    n_s = lib.mp_scores_bwd_scratch_floats(K, B, T)
    sscratch = Buf((n_s,))
    outs.update(sc=Buf((B, K, T)), sdh=Buf((K, B * T * J, SO), dh_init), sdw=Buf((K, J), sd["sw"]), sdb=Buf((K,), sd["sb"]))
    inits.update(sc=None, sdh=dh_init, sdw=sd["sw"], sdb=sd["sb"])
    o = outs

    def scores_fwd(h=sv["h"].data_ptr(), sc=o["sc"].p, K=K, O=SO, B=B, T=T, J=J):
        return lib.mp_scores_fwd_ex(h, sv["w"].data_ptr(), sv["b"].data_ptr(), K, O, sc, B, T, J, st())

    def scores_bwd(s=s_dev.data_ptr(), dh=o["sdh"].p, K=K, O=SO, B=B, T=T, J=J, n=n_s, ps=None):
        return lib.mp_scores_bwd_ex(sv["h"].data_ptr(), s, sv["d"].data_ptr(), sv["w"].data_ptr(), sv["b"].data_ptr(), o["sdw"].p, o["sdb"].p, K, O, dh,
                                    B, T, J, sscratch.p, n, ps, st())

    def embed_fwd(x=ev["x"].data_ptr(), out=o["out"].p, M=M, C=C, J=J):
        return lib.mp_embed_fwd_ex(x, ev["W"].data_ptr(), ev["b"].data_ptr(), ev["spos"].data_ptr(), out, M, C, J, st())

    def embed_bwd(g_=ev["g"].data_ptr(), dW=o["dW"].p, M=M, C=C, J=J, sc=scratch.p, n=n_e):
        return lib.mp_embed_bwd_ex(g_, ev["x"].data_ptr(), dW, o["db"].p, o["dsp"].p, M, C, J, sc, n, st())

    def bones_fwd(x=bev["x"].data_ptr(), BT=BT, IN=34, O=O):
        return lib.mp_bones_embed_fwd_ex(x, bev["W"].data_ptr(), bev["b"].data_ptr(), bev["spos"].data_ptr(), o["bout"].p, BT, IN, O, st())

    def bones_bwd(dsp=o["bdsp"].p, BT=BT, IN=34, O=O, n=n_b):
        return lib.mp_bones_embed_bwd_ex(bev["g"].data_ptr(), bev["x"].data_ptr(), o["bdW"].p, o["bdb"].p, dsp, BT, IN, O, scratch.p, n, st())

    def tpos(g_=tg.data_ptr(), B=B, T=T, J=J, C=C):
        return lib.mp_tpos_grad_ex(g_, o["tp"].p, B, T, J, C, st())

    def mean_fwd(h=hm.data_ptr(), B=B, T=T, S=S):
        return lib.mp_bones_mean_fwd_ex(h, o["ln"].p, B, T, S, st())

    def mean_bwd(dh=o["dh"].p, KT=KT, B=B, T=T, S=S):
        return lib.mp_bones_mean_bwd_ex(dlp.data_ptr(), KT, o["dl"].p, dh, B, T, S, st())

    bad = [(embed_fwd, dict(x=None)), (embed_fwd, dict(out=None)), (embed_fwd, dict(M=0)), (embed_fwd, dict(C=30)), (embed_fwd, dict(C=0)),
           (embed_fwd, dict(J=0)), (embed_bwd, dict(g_=None)), (embed_bwd, dict(dW=None)), (embed_bwd, dict(sc=None)), (embed_bwd, dict(M=-1)),
           (embed_bwd, dict(C=30)), (embed_bwd, dict(J=0)), (embed_bwd, dict(n=n_e - 1)), (bones_fwd, dict(x=None)), (bones_fwd, dict(BT=0)),
           (bones_fwd, dict(IN=32)), (bones_fwd, dict(O=0)), (bones_bwd, dict(dsp=None)), (bones_bwd, dict(BT=0)), (bones_bwd, dict(IN=36)),
           (bones_bwd, dict(O=-256)), (bones_bwd, dict(n=n_b - 1)), (tpos, dict(g_=None)), (tpos, dict(B=0)), (tpos, dict(T=0)), (tpos, dict(J=3)),
           (tpos, dict(J=0)), (tpos, dict(C=30)), (tpos, dict(C=0)), (mean_fwd, dict(h=None)), (mean_fwd, dict(B=0)), (mean_fwd, dict(T=0)),
           (mean_fwd, dict(S=0)), (mean_fwd, dict(S=33)), (mean_bwd, dict(dh=None)), (mean_bwd, dict(KT=0)), (mean_bwd, dict(B=0)),
           (mean_bwd, dict(T=0)), (mean_bwd, dict(S=0)), (mean_bwd, dict(S=33)), (scores_fwd, dict(h=None)), (scores_fwd, dict(sc=None)),
           (scores_fwd, dict(K=0)), (scores_fwd, dict(K=9)), (scores_fwd, dict(O=0)), (scores_fwd, dict(B=0)), (scores_fwd, dict(T=0)),
           (scores_fwd, dict(J=0)), (scores_fwd, dict(J=33)), (scores_bwd, dict(s=None)), (scores_bwd, dict(dh=None)), (scores_bwd, dict(K=0)),
           (scores_bwd, dict(K=9)), (scores_bwd, dict(J=33)), (scores_bwd, dict(O=0)), (scores_bwd, dict(B=0)), (scores_bwd, dict(T=-1)),
           (scores_bwd, dict(n=n_s - 1)), (scores_bwd, dict(n=n_s - 1, ps=torch.cuda.Stream().cuda_stream))]
    for f, kw in bad:
        assert f(**kw) == ERR_ARG, (f.__name__, kw)
        assert lib.mp_last_error()
    assert lib.mp_embed_bwd_scratch_floats(0, 17) == 0 and lib.mp_embed_bwd_scratch_floats(32, 0) == 0
    torch.cuda.synchronize()
    for k, b in outs.items():
        b.untouched(inits[k], k)
    for f in (embed_fwd, embed_bwd, bones_fwd, bones_bwd, tpos, mean_fwd, mean_bwd, scores_fwd, scores_bwd):
        check(lib, f(), f.__name__)
    torch.cuda.synchronize()
    scratch.ok("scratch")
    sscratch.ok("scores scratch")
    report("scores after the refusals", er.worst(o["sc"].ok("sc"), *er.scores_fwd(sd["h"], sd["w"], sd["b"], B, T, J)[0], er.F32_TINY), "scores")
    report("scores dw after the refusals", er.worst(o["sdw"].ok("sdw"), *er.scores_bwd(sd["h"], s_in, sd["d"], sd["w"], sd["sw"], sd["sb"], B, T, J)[1]), "scores_dw")
    same_bits(o["sdh"].ok("sdh")[:, :, :SO - 1], dh_init[:, :, :SO - 1].cuda(), "channels of dheadout the score head does not own")
    report("embed_fwd after the refusals", er.worst(o["out"].ok("out"), *er.embed_fwd(e["x"], e["W"], e["b"], e["spos"], J)), "embed_fwd")
    report("embed dW after the refusals", er.worst(o["dW"].ok("dW"), *er.embed_bwd(e["g"], e["x"], J, e["sW"], e["sb"], e["sspos"])[0]), "embed_dW")
    report("bones_embed_fwd after the refusals", er.worst(o["bout"].ok("bout"), *er.bones_embed_fwd(be["x"], be["W"], be["b"], be["spos"])), "bones_embed_fwd")
    report("bones_embed dspos after the refusals", er.worst(o["bdsp"].ok("bdsp"), *er.bones_embed_bwd(be["g"], be["x"], be["sW"], be["sb"], be["sspos"])[2]),
           "bones_embed_dspos")
    report("tpos_grad after the refusals", er.worst(o["tp"].ok("tp"), *er.tpos_grad(tg.cpu(), tseed, B, T, J)), "tpos_grad")
    report("bones_mean_fwd after the refusals", er.worst(o["ln"].ok("ln"), *er.bones_mean_fwd(hm.cpu(), B, T, S)), "bones_mean_fwd")
    report("bones_mean_bwd after the refusals", er.worst(o["dl"].ok("dl"), *er.bones_mean_bwd(dlp.cpu(), B, KT, S)), "bones_mean_bwd")

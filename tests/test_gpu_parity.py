"""GPU parity tests: every HIP kernel and the whole model (forward, loss, backward, Adam) through the C ABI against
the CPU oracle (oracle/manipose_ref.py) and the committed golden fixtures.  Run with ``pytest -m gpu`` on an MI355X.

Tolerances: the path is fp32 end to end in the default (parity) precision; the north-star bound is 1e-4 m on MPJPE.
Kernel-level comparisons use rtol/atol a few fp32 ulps above the CPU oracle's own reassociation noise.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import manipose_ref as orc
from helpers import droppath_mask_names, fixture_masks, fixture_state, load_fixture

pytestmark = pytest.mark.gpu

MPJPE_TOL_M = 1e-4      # BASELINE.json north_star: outputs within 1e-4 on MPJPE


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def st():
    return torch.cuda.current_stream().cuda_stream


def close(got, want, rtol=1e-4, atol=1e-5, msg=""):
    np.testing.assert_allclose(got.detach().cpu().numpy() if torch.is_tensor(got) else got,
                               want.detach().cpu().numpy() if torch.is_tensor(want) else want, rtol=rtol, atol=atol,
                               err_msg=msg)


# --------------------------------------------------------------------------------------------- decoder
def test_fk_decode_forward_backward_vs_reference_fixture(lib):
    from manipose_amd import _lib
    fx = load_fixture("decoder")
    rot = dev(fx["rot6d"])                      # (B*L, 17, 6) rows ordered (b, l)
    B, L = 3, 7
    lengths = dev(fx["bones"].reshape(B, 16))
    poses = torch.empty(B, 1, L, 17, 3, device="cuda")
    _lib.check(lib.mp_fk_decode_fwd(rot.data_ptr(), 6, 6, lengths.data_ptr(), poses.data_ptr(), B, 1, L, st()))
    # pose 1 / joint 5 has EXACTLY colinear 6-D halves (x cross b == rounding noise): its frame, hence joints 5 and 6 of
    # that pose, is ill-conditioned (the reference's own value changes with the BLAS/FMA build) and is excluded.
    ok = np.ones((B * L, 17), dtype=bool)
    ok[1, 5:7] = False
    got_p = poses.view(B * L, 17, 3).cpu().numpy()
    np.testing.assert_allclose(got_p[ok], fx["poses"][ok], rtol=1e-5, atol=2e-6)
    assert bool((poses[..., 0, :] == 0).all())
    gp = dev(fx["gpos"]).view(B, 1, L, 17, 3).contiguous()
    drot = torch.zeros_like(rot)
    dlen = torch.zeros(B * L, 16, device="cuda")
    _lib.check(lib.mp_fk_decode_bwd(rot.data_ptr(), 6, 6, lengths.data_ptr(), gp.data_ptr(), drot.data_ptr(), dlen.data_ptr(),
                                    B, 1, L, st()))
    want = fx["g_rot6d"]
    finite = np.isfinite(want)                  # the reference's autograd yields NaN at the two degenerate joints
    assert (~finite).sum() == 12
    got = drot.cpu().numpy()
    assert np.isfinite(got).all()
    finite[1] = False                           # whole pose 1: gradients flow through the ill-conditioned frame
    np.testing.assert_allclose(got[finite], want[finite], rtol=2e-4, atol=2e-5)
    gb = dlen.view(B, L, 16).sum(1).cpu().numpy()
    okb = np.ones((B, 16), dtype=bool)
    okb[0, 4:6] = False                         # segment-length gradients of the two ill-conditioned joints (batch item 0)
    np.testing.assert_allclose(gb[okb], fx["g_bones"].reshape(B, 16)[okb], rtol=2e-4, atol=2e-5)


def test_custom_operators_registered_under_torch_ops_manipose(lib):
    """SURVEY 8b / north star "exposed as custom ops": torch.ops.manipose.* (manipose_amd/ops.py, torch.library.custom_op over the C ABI).
    fk_decode against the reference's decoder fixture, forward and - through autograd - backward; wta_loss against the reference's loss
    fixture incl. its gradient; adam_step against the reference Adam fixture; linear / layernorm / attention against torch's own operators
    with autograd on both sides; torch.library.opcheck (schema, fake-tensor shapes, autograd registration) on the differentiable ones."""
    import manipose_amd.ops  # noqa: F401
    fx = load_fixture("decoder")
    B, L = 3, 7
    rot = dev(fx["rot6d"]).view(1, B * L * 17, 6).clone().requires_grad_(True)      # (K = 1, B T 17, 6), rows (b, l, j)
    lengths = dev(fx["bones"].reshape(B, 16)).clone().requires_grad_(True)
    poses = torch.ops.manipose.fk_decode(rot, lengths, 1, L)
    ok = np.ones((B * L, 17), dtype=bool)
    ok[1, 5:7] = False                          # the fixture's ill-conditioned joints (see the C-ABI test above)
    np.testing.assert_allclose(poses.detach().view(B * L, 17, 3).cpu().numpy()[ok], fx["poses"][ok], rtol=1e-5, atol=2e-6)
    poses.backward(dev(fx["gpos"]).view(B, 1, L, 17, 3))
    want = fx["g_rot6d"]
    finite = np.isfinite(want)
    finite[1] = False
    np.testing.assert_allclose(rot.grad.view(B * L, 17, 6).cpu().numpy()[finite], want[finite], rtol=2e-4, atol=2e-5)
    okb = np.ones((B, 16), dtype=bool)
    okb[0, 4:6] = False
    np.testing.assert_allclose(lengths.grad.cpu().numpy()[okb], fx["g_bones"].reshape(B, 16)[okb], rtol=2e-4, atol=2e-5)
    with pytest.raises(NotImplementedError):    # registered for ROCm devices only: a CPU tensor is refused, there is no fallback
        torch.ops.manipose.fk_decode(rot.detach().cpu(), lengths.detach().cpu(), 1, L)
    torch.library.opcheck(torch.ops.manipose.fk_decode.default, (rot.detach().clone().requires_grad_(True), lengths.detach().clone(), 1, L),
                          test_utils=("test_schema", "test_faketensor", "test_autograd_registration"))
    # loss
    fl = load_fixture("loss")
    hyp, sc, y = (dev(fl[k]).clone() for k in ("poses", "scores", "y"))
    hyp.requires_grad_(True); sc.requires_grad_(True)
    terms, argmin, _, _ = torch.ops.manipose.wta_loss(hyp, sc, y, 0.1, 2.0, 0.5, 1, 0)
    terms.sum().backward()
    np.testing.assert_allclose(terms.detach().cpu().numpy(), fl["loss_terms"], rtol=2e-5)
    close(hyp.grad, fl["g_poses"], rtol=1e-4, atol=1e-8)
    close(sc.grad, fl["g_scores"], rtol=1e-4, atol=1e-8)
    _, oidx = orc.wta_l2_loss_and_activate_head(torch.from_numpy(fl["poses"]), torch.from_numpy(fl["y"]), torch.tensor(orc.STANDARD_H36M_WEIGHTS))
    assert torch.equal(argmin.long().cpu(), oidx.long())
    # Adam
    fa = load_fixture("rmcl_tiny")
    k0 = next(k[7:] for k in fa if k.startswith("adam1::"))
    p = dev(fa["w::" + k0]).clone().reshape(-1)
    m1, m2 = torch.zeros_like(p), torch.zeros_like(p)
    torch.ops.manipose.adam_step(p, dev(fa["g::" + k0]).reshape(-1), m1, m2, 1, 4e-5, 0.9, 0.999, 1e-8, 1e-6, 1.0)
    close(p, fa["adam1::" + k0].reshape(-1), rtol=1e-6, atol=1e-9)
    # linear / layernorm / attention against torch (autograd on both sides)
    gen = torch.Generator(device="cuda").manual_seed(0)
    x = torch.randn(300, 64, device="cuda", generator=gen, requires_grad=True)
    W = (torch.randn(96, 64, device="cuda", generator=gen) / 8).requires_grad_(True)
    b = torch.randn(96, device="cuda", generator=gen, requires_grad=True)
    for epi in (0, 1):
        y_, _ = torch.ops.manipose.linear(x, W, b, epi)
        ref = torch.nn.functional.linear(x, W, b)
        ref = torch.nn.functional.gelu(ref) if epi else ref
        close(y_, ref, rtol=1e-4, atol=1e-5)
        gy = torch.randn_like(ref)
        got = torch.autograd.grad(y_, (x, W, b), gy)
        wantg = torch.autograd.grad(ref, (x, W, b), gy)
        for a_, b_ in zip(got, wantg):
            close(a_, b_, rtol=2e-3, atol=2e-4)
    gam, bet = torch.rand(64, device="cuda", generator=gen) + 0.5, torch.randn(64, device="cuda", generator=gen)
    gam.requires_grad_(True); bet.requires_grad_(True)
    yl, _ = torch.ops.manipose.layernorm(x, gam, bet, 1e-6)
    refl = torch.nn.functional.layer_norm(x, (64,), gam, bet, 1e-6)
    close(yl, refl, rtol=1e-4, atol=1e-5)
    gl = torch.randn_like(refl)
    for a_, b_ in zip(torch.autograd.grad(yl, (x, gam, bet), gl), torch.autograd.grad(refl, (x, gam, bet), gl)):
        close(a_, b_, rtol=2e-3, atol=2e-4)
    Bq, Tq, Jq, Hq, Cq = 2, 9, 17, 4, 64
    qkv = torch.randn(Bq * Tq * Jq, 3 * Cq, device="cuda", generator=gen, requires_grad=True)
    for temporal in (False, True):
        out, _ = torch.ops.manipose.attention(qkv, temporal, Bq, Tq, Jq, Hq)
        q, k, v = (t.reshape(Bq, Tq, Jq, Hq, Cq // Hq) for t in qkv.split(Cq, dim=1))
        perm = (0, 1, 3, 2, 4) if not temporal else (0, 2, 3, 1, 4)             # (b, t, h, j, d) / (b, j, h, t, d): attend over the second-to-last axis
        qh, kh, vh = (t.permute(*perm) for t in (q, k, v))
        refa = torch.nn.functional.scaled_dot_product_attention(qh, kh, vh)
        refa = (refa.permute(0, 1, 3, 2, 4) if not temporal else refa.permute(0, 3, 1, 2, 4)).reshape(Bq * Tq * Jq, Cq)
        close(out, refa, rtol=1e-4, atol=1e-5)
        go = torch.randn_like(refa)
        close(torch.autograd.grad(out, qkv, go)[0], torch.autograd.grad(refa, qkv, go)[0], rtol=2e-3, atol=2e-4)


def test_fk_decode_known_answer_tpose_and_autograd_module(lib):
    from manipose_amd.architectures import PoseDecoder
    from manipose_amd.data import h36m_skeleton
    fx = load_fixture("decoder")
    dec = PoseDecoder(h36m_skeleton())
    ident = torch.tensor([1., 0, 0, 0, 1, 0], device="cuda").repeat(1, 17, 1)
    tp = dec(ident, dev(fx["tpose_lens"]), torch.zeros(1, 3, device="cuda"))
    close(tp, fx["tpose"], atol=1e-7)
    rot = dev(fx["rot6d"][2:]).requires_grad_(True)            # skip the rows holding the degenerate joints
    bl = dev(fx["bones"]).requires_grad_(True)
    rot_full = torch.cat([dev(fx["rot6d"][:2]), rot], 0)
    poses = dec(rot_full, bl)
    (poses * dev(fx["gpos"])).sum().backward()
    close(rot.grad, fx["g_rot6d"][2:], rtol=2e-4, atol=2e-5)
    okb = np.ones((3, 16, 1), dtype=bool)
    okb[0, 4:6] = False                         # see the ill-conditioned joints of pose 1 above
    np.testing.assert_allclose(bl.grad.cpu().numpy()[okb], fx["g_bones"][okb], rtol=2e-4, atol=2e-5)


# --------------------------------------------------------------------------------------------- loss
def test_wta_loss_terms_and_gradients_vs_reference_fixture(lib):
    from manipose_amd.metrics import rmcl_training_loss
    fx = load_fixture("loss")
    poses = dev(fx["poses"]).requires_grad_(True)
    scores = dev(fx["scores"]).requires_grad_(True)
    total, terms = rmcl_training_loss(poses, scores, dev(fx["y"]))
    total.backward()
    got = np.array([terms[k].item() for k in ("wloss", "score_reg", "vloss", "sreg")])
    np.testing.assert_allclose(got, fx["loss_terms"], rtol=2e-5)
    close(poses.grad, fx["g_poses"], rtol=1e-4, atol=1e-8)
    close(scores.grad, fx["g_scores"], rtol=1e-4, atol=1e-8)


def test_wta_loss_kernel_forms_by_scratch_size_and_ragged_frame_counts(lib):
    """mp_wta_loss through the C ABI on the fixture and on frame counts that do not fill the last wave / workgroup (a lane per joint, three frames per
    wave, shuffle sums over a frame's 17 lanes, winner broadcast by a shuffle): with the ABI's minimum scratch (256 frames per workgroup) and with
    >= 4 ceil(B T / 48) floats (48 frames per workgroup) - the same argmin, the same gradients bit for bit (they do not depend on the partial sums),
    terms equal to the oracle's.  The gradients themselves are checked per element against fp64, in each form, by tests/test_gpu_loss_kernels.py."""
    import ctypes as C
    from manipose_amd import _lib
    g = torch.Generator().manual_seed(9)
    for B, K, T in ((1, 1, 2), (2, 5, 7), (3, 3, 50), (5, 5, 243), (2, 8, 100)):
        poses = 0.3 * torch.randn(B, K, T, 17, 3, generator=g)
        y = 0.3 * torch.randn(B, T, 17, 3, generator=g)
        scores = torch.softmax(torch.randn(B, K, T, 1, generator=g), 1).contiguous()
        o_tot, o_terms = orc.rmcl_training_loss(poses, scores, y)
        cfg = _lib.LossConfig(rmcl_score_reg=0.1, vel_loss=2.0, smooth_reg=0.5, w_loss=1, sq_loss=0)
        dposes, dscores, dy = poses.cuda(), scores.cuda(), y.cuda()
        outs = []
        for fpb in (256, 48):
            terms = torch.zeros(4, device="cuda")
            dp, dsc = torch.full((B, K, T, 17, 3), float("nan"), device="cuda"), torch.full((B, K, T, 1), float("nan"), device="cuda")
            am = torch.full((B, T), -1, device="cuda", dtype=torch.int32)
            sc = torch.empty(4 * ((B * T + fpb - 1) // fpb), device="cuda")
            _lib.check(lib.mp_wta_loss(_lib.ptr(dposes), _lib.ptr(dscores), _lib.ptr(dy), C.byref(cfg), _lib.ptr(terms), _lib.ptr(am),
                                       _lib.ptr(dp), _lib.ptr(dsc), B, K, T, _lib.ptr(sc), sc.numel(), st()), "mp_wta_loss")
            torch.cuda.synchronize()
            np.testing.assert_allclose(terms.cpu().numpy(), [o_terms[k].item() for k in ("wloss", "score_reg", "vloss", "sreg")], rtol=2e-5, atol=1e-8)
            assert torch.isfinite(dp).all() and torch.isfinite(dsc).all() and int(am.min()) >= 0 and int(am.max()) < K
            outs.append((am.clone(), dp.clone(), dsc.clone()))
        assert all(torch.equal(u, v) for u, v in zip(outs[0], outs[1])), (B, K, T)
        want = ((poses - y[:, None]).norm(dim=-1) * torch.tensor(orc.STANDARD_H36M_WEIGHTS)).mean(-1).argmin(1)
        assert torch.equal(outs[0][0].cpu().long(), want), (B, K, T)


def test_reference_named_loss_functions(lib):
    from manipose_amd import metrics as M
    fx = load_fixture("loss")
    poses, scores, y = dev(fx["poses"]), dev(fx["scores"]), dev(fx["y"])
    w = M.STANDARD_H36M_WEIGHTS
    cp, cy = torch.from_numpy(fx["poses"]), torch.from_numpy(fx["y"])
    val, idx = M.wta_l2_loss_and_activate_head(poses, y, weights=w)
    oval, oidx = orc.wta_l2_loss_and_activate_head(cp, cy, w)
    assert torch.equal(idx.cpu(), oidx)
    close(val, oval, rtol=1e-5, atol=1e-7)
    close(M.mean_velocity_error(poses, y, axis=2), orc.mean_velocity_error(cp, cy, axis=2), rtol=1e-5)
    close(M.smoothness_regularization(poses, w, axis=2), orc.smoothness_regularization(cp, w, axis=2), rtol=1e-5)
    both, reg = M.wta_with_scoring_loss(poses, scores, y, beta=0.1, weights=w)
    oboth, oreg = orc.wta_with_scoring_loss(cp, torch.from_numpy(fx["scores"]), cy, 0.1, w)
    close(both, oboth, rtol=1e-5)
    close(reg, oreg, rtol=1e-5)
    close(M.mpjpe_error(poses[:, 0], y, "average"), orc.mpjpe_error(cp[:, 0], cy), rtol=1e-5)


# --------------------------------------------------------------------------------------------- building blocks
@pytest.mark.parametrize("M,C", [(37, 32), (306, 128), (4131, 512)])
def test_layernorm_forward_backward(lib, M, C):
    from manipose_amd import _lib
    g = torch.Generator().manual_seed(M + C)
    x = torch.randn(M, C, generator=g)
    gamma, beta = 1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    dy, dskip = torch.randn(M, C, generator=g), torch.randn(M, C, generator=g)
    xr = x.clone().requires_grad_(True)
    gr, br = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    y_ref = torch.nn.functional.layer_norm(xr, (C,), gr, br, 1e-6)
    (y_ref * dy).sum().backward()
    xd, y, stats = x.cuda(), torch.empty(M, C, device="cuda"), torch.empty(M, 2, device="cuda")
    gd, bd, dyd, dsd = gamma.cuda(), beta.cuda(), dy.cuda(), dskip.cuda()
    _lib.check(lib.mp_layernorm_fwd(xd.data_ptr(), gd.data_ptr(), bd.data_ptr(), 1e-6, y.data_ptr(),
                                    stats.data_ptr(), M, C, st()))
    close(y, y_ref, rtol=1e-5, atol=2e-6)
    dx = torch.empty(M, C, device="cuda")
    dg, db = torch.zeros(C, device="cuda"), torch.zeros(C, device="cuda")
    scratch = torch.empty(1024 * 2 * C + 16, device="cuda")       # LN-backward partials: 1024 workgroups x [dgamma | dbeta]
    _lib.check(lib.mp_layernorm_bwd(dyd.data_ptr(), xd.data_ptr(), stats.data_ptr(), gd.data_ptr(),
                                    dsd.data_ptr(), dx.data_ptr(), dg.data_ptr(), db.data_ptr(), M, C,
                                    scratch.data_ptr(), scratch.numel(), st()))
    close(dx, xr.grad + dskip, rtol=1e-4, atol=1e-5)
    close(dg, gr.grad, rtol=1e-4, atol=1e-4)
    close(db, br.grad, rtol=1e-4, atol=1e-4)


# K output heads = K x [LayerNorm(C, eps 1e-5) -> Linear(C, O)] (MCLHead stack, rmcl_manifold_mix_ste.py:291-298; MixSTE.head,
# mix_ste.py:123-126) against torch autograd on the CPU, for the row kernels (impl 1) and the fp32 matrix-core kernels (impl 2):
# ragged token counts (not a multiple of the 16-token MFMA tile, fewer tokens than one tile), both widths, 1..48 output columns.
@pytest.mark.parametrize("impl,K,O,C,M", [(1, 5, 7, 512, 1003), (2, 5, 7, 512, 1003), (2, 5, 7, 512, 7), (2, 1, 3, 512, 17 * 9 + 1), (2, 3, 7, 128, 77),
                                          (2, 6, 8, 128, 4131), (1, 1, 1, 128, 333), (2, 1, 1, 128, 333), (2, 2, 7, 512, 100), (2, 4, 7, 128, 1601),
                                          (2, 8, 5, 512, 2 * 243 * 17), (0, 5, 7, 512, 243 * 17), (0, 1, 1, 128, 243 * 16), (2, 5, 7, 256, 1500), (0, 1, 3, 256, 999)])
def test_output_heads_forward_backward(lib, impl, K, O, C, M):
    from manipose_amd import _lib
    g = torch.Generator().manual_seed(7 * M + K + O + C)
    x = 1.5 * torch.randn(M, C, generator=g) + 0.3
    gamma, beta = 1 + 0.1 * torch.randn(K, C, generator=g), 0.1 * torch.randn(K, C, generator=g)
    W, b = torch.randn(K, O, C, generator=g) / C ** 0.5, 0.1 * torch.randn(K, O, generator=g)
    dout = torch.randn(K, M, O, generator=g)
    ref = [t.clone().requires_grad_(True) for t in (x, gamma, beta, W, b)]
    y_ref = torch.stack([torch.nn.functional.linear(torch.nn.functional.layer_norm(ref[0], (C,), ref[1][k], ref[2][k], 1e-5), ref[3][k], ref[4][k])
                         for k in range(K)])
    (y_ref * dout).sum().backward()
    xd, gd, bd, Wd, bbd, dd = (t.cuda() for t in (x, gamma, beta, W, b, dout))
    out, stats = torch.empty(K, M, O, device="cuda"), torch.empty(M, 2, device="cuda")
    fold = torch.zeros(lib.mp_heads_fold_floats(C), device="cuda")
    _lib.check(lib.mp_heads_fwd(xd.data_ptr(), gd.data_ptr(), bd.data_ptr(), Wd.data_ptr(), bbd.data_ptr(), K, O, out.data_ptr(), stats.data_ptr(),
                                fold.data_ptr(), M, C, impl, st()))
    close(out, y_ref, rtol=1e-5, atol=5e-6)
    close(stats[:, 0], x.mean(1), rtol=1e-5, atol=1e-6)
    dx = torch.full((M, C), float("nan"), device="cuda")
    seed = [0.5 * torch.randn(t.shape, generator=g) for t in (gamma, beta, W, b)]       # parameter gradients are accumulated into
    grads = [t.cuda() for t in seed]
    scratch = torch.empty(lib.mp_heads_bwd_scratch_floats(K, O, C), device="cuda")
    _lib.check(lib.mp_heads_bwd(xd.data_ptr(), stats.data_ptr(), fold.data_ptr(), out.data_ptr(), gd.data_ptr(), bd.data_ptr(), Wd.data_ptr(),
                                bbd.data_ptr(), dd.data_ptr(), dx.data_ptr(), *[t.data_ptr() for t in grads], K, O, M, C, impl,
                                scratch.data_ptr(), scratch.numel(), st()))
    close(dx, ref[0].grad, rtol=1e-4, atol=2e-5)
    tol = 2e-4 * max(1.0, (M / 1000) ** 0.5)
    for got, s0, r in zip(grads, seed, ref[1:]):
        close(got, s0 + r.grad, rtol=1e-4, atol=tol)


def test_output_heads_reject_uncovered_shapes(lib):
    from manipose_amd import _lib
    t = torch.zeros(4096, device="cuda")
    for K, O, C in ((5, 7, 384), (7, 7, 512), (1, 9, 512)):        # width without a matrix-core instance; 49 > 48 columns; 9 outputs per head
        rc = lib.mp_heads_fwd(t.data_ptr(), t.data_ptr(), t.data_ptr(), t.data_ptr(), t.data_ptr(), K, O, t.data_ptr(), t.data_ptr(), t.data_ptr(), 4, C, 2, st())
        assert rc != 0 and b"matrix-core" in lib.mp_last_error(), (K, O, C, rc)
    assert lib.mp_heads_fwd(t.data_ptr(), t.data_ptr(), t.data_ptr(), t.data_ptr(), t.data_ptr(), 5, 7, t.data_ptr(), t.data_ptr(), t.data_ptr(), 4, 512, 3, st()) != 0


@pytest.mark.parametrize("M,N,K", [(306, 96, 32), (130, 48, 16), (4131, 1536, 512), (1000, 512, 1024)])
def test_linear_forward_epilogues_and_backward(lib, M, N, K):
    from manipose_amd import _lib
    g = torch.Generator().manual_seed(M + N + K)
    x, W, b = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) / K ** 0.5, torch.randn(N, generator=g)
    r, dy = torch.randn(M, N, generator=g), torch.randn(M, N, generator=g)
    xd, Wd, bd, rd, dyd = x.cuda(), W.cuda(), b.cuda(), r.cuda(), dy.cuda()
    ref = (x.double() @ W.double().T + b.double())
    tol = dict(rtol=2e-5, atol=2e-5 * max(1.0, (K / 64) ** 0.5))
    y = torch.empty(M, N, device="cuda")
    _lib.check(lib.mp_linear_fwd(xd.data_ptr(), Wd.data_ptr(), bd.data_ptr(), y.data_ptr(), None, None, M, N, K, 0, st()))
    close(y, ref.float(), **tol)
    z = torch.empty(M, N, device="cuda")
    _lib.check(lib.mp_linear_fwd(xd.data_ptr(), Wd.data_ptr(), bd.data_ptr(), y.data_ptr(), z.data_ptr(), None, M, N, K, 1, st()))
    refg = ref.clone().requires_grad_(True)
    torch.nn.functional.gelu(refg).sum().backward()
    close(z, refg.grad.float(), **tol)                   # z keeps gelu'(pre-activation)
    close(y, torch.nn.functional.gelu(ref).float(), **tol)
    _lib.check(lib.mp_linear_fwd(xd.data_ptr(), Wd.data_ptr(), bd.data_ptr(), y.data_ptr(), None, rd.data_ptr(), M, N, K, 2, st()))
    close(y, (ref + r.double()).float(), **tol)
    # backward: dx = dy W, dW += dy^T x (accumulating), db += colsum(dy)
    dx = torch.empty(M, K, device="cuda")
    dW, db = torch.ones(N, K, device="cuda"), torch.ones(N, device="cuda")
    slab = torch.empty(int(lib.mp_linear_bwd_slab_floats(N, K)), device="cuda")
    _lib.check(lib.mp_linear_bwd(dyd.data_ptr(), xd.data_ptr(), Wd.data_ptr(), dx.data_ptr(), dW.data_ptr(), db.data_ptr(),
                                 M, N, K, slab.data_ptr(), slab.numel(), st()))
    tolb = dict(rtol=5e-5, atol=5e-5 * max(1.0, (M / 64) ** 0.5))
    close(dx, (dy.double() @ W.double()).float(), rtol=5e-5, atol=5e-5 * max(1.0, (N / 64) ** 0.5))
    close(dW, (1 + dy.double().T @ x.double()).float(), **tolb)
    close(db, (1 + dy.double().sum(0)).float(), **tolb)


def _attn_ref(qkv, B, T, J, C, H, temporal):
    """mix_ste.py:255-279 restated on the (b,t,j) token layout for one fused qkv buffer."""
    d = C // H
    q, k, v = qkv.view(B, T, J, 3, H, d).unbind(3)                        # (B,T,J,H,d)
    if temporal:
        q, k, v = (t.permute(0, 2, 3, 1, 4) for t in (q, k, v))           # (B,J,H,T,d)
    else:
        q, k, v = (t.permute(0, 1, 3, 2, 4) for t in (q, k, v))           # (B,T,H,J,d)
    a = ((q @ k.transpose(-2, -1)) * d ** -0.5).softmax(-1) @ v
    a = a.permute(0, 3, 1, 2, 4) if temporal else a.permute(0, 1, 3, 2, 4)
    return a.reshape(B * T * J, C)


@pytest.mark.parametrize("temporal,B,T,J,C,H", [(0, 2, 9, 17, 32, 4), (0, 1, 27, 16, 128, 8), (0, 1, 5, 17, 512, 8),
                                                (1, 2, 9, 17, 32, 4), (1, 1, 27, 16, 128, 8), (1, 1, 243, 17, 64, 1),
                                                (1, 1, 243, 2, 512, 8), (1, 1, 300, 3, 16, 4)])
def test_attention_forward_backward(lib, temporal, B, T, J, C, H):
    from manipose_amd import _lib
    g = torch.Generator().manual_seed(T * 7 + C)
    M = B * T * J
    qkv = torch.randn(M, 3 * C, generator=g).requires_grad_(True)
    dout = torch.randn(M, C, generator=g)
    ref = _attn_ref(qkv, B, T, J, C, H, temporal)
    (ref * dout).sum().backward()
    qd = qkv.detach().cuda()
    out = torch.empty(M, C, device="cuda")
    lse = torch.empty(B * J * H * T, device="cuda")
    _lib.check(lib.mp_attention_fwd(qd.data_ptr(), out.data_ptr(), lse.data_ptr(), temporal, B, T, J, C, H, st()))
    close(out, ref, rtol=2e-5, atol=2e-6)
    dq = torch.zeros(M, 3 * C, device="cuda")
    delta = torch.empty(B * J * H * T, device="cuda")
    dod = dout.cuda()
    _lib.check(lib.mp_attention_bwd(qd.data_ptr(), out.data_ptr(), dod.data_ptr(), lse.data_ptr(), delta.data_ptr(),
                                    dq.data_ptr(), temporal, B, T, J, C, H, st()))
    close(dq, qkv.grad, rtol=1e-4, atol=2e-6)


def test_adam_step_vs_reference_fixture(lib):
    from manipose_amd import _lib
    fx = load_fixture("rmcl_tiny")
    for k in [k[7:] for k in fx if k.startswith("adam1::")]:
        p, g = dev(fx["w::" + k]).clone(), dev(fx["g::" + k])
        m, v = torch.zeros_like(p), torch.zeros_like(p)
        _lib.check(lib.mp_adam_step(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), 1, 4e-5, 0.9, 0.999,
                                    1e-8, 1e-6, 1.0, st()))
        close(p, fx["adam1::" + k], rtol=1e-6, atol=1e-9)


# --------------------------------------------------------------------------------------------- whole model
def _build(fx, drop_path_rate=0.0):
    from manipose_amd import ManifoldMixSTE, RMCLManifoldMixSTE, h36m_skeleton
    c = fx["cfg"]
    kw = dict(skeleton=h36m_skeleton(), num_frame=c["T"], embed_dim_rot=c["C_rot"], depth_rot=c["depth_rot"],
              num_heads_rot=c["heads_rot"], embed_dim_seg=c["C_seg"], depth_seg=c["depth_seg"], num_heads_seg=c["heads_seg"],
              drop_path_rate=drop_path_rate, rot_rep_dim=c.get("rot_dim", 6))
    model = RMCLManifoldMixSTE(n_hyp=c["n_hyp"], **kw) if c["n_hyp"] > 0 else ManifoldMixSTE(**kw)
    model.load_state_dict(fixture_state(fx), strict=True)
    return model.cuda()


def _check_grads(model, fx, rtol=2e-3, atol=2e-6):
    worst = ("", 0.0)
    for k, p in model.named_parameters():
        want = fx["g::" + k]
        got = p.grad.detach().cpu().numpy()
        assert got.shape == want.shape, k
        scale = np.abs(want).max() + 1e-12
        err = np.abs(got - want).max() / scale
        if err > worst[1]:
            worst = (k, err)
        np.testing.assert_allclose(got, want, rtol=rtol, atol=atol + 1e-4 * scale, err_msg=k)
    return worst


@pytest.mark.parametrize("name", ["rmcl_tiny", "rmcl_small"])
def test_rmcl_model_forward_loss_backward_vs_reference(lib, name):
    from manipose_amd.metrics import mpjpe_error, rmcl_training_loss
    fx = load_fixture(name)
    model = _build(fx).eval()
    X, y = dev(fx["X"]), dev(fx["y"])
    poses, scores = model(X)
    assert poses.shape == fx["poses"].shape and scores.shape == fx["scores"].shape
    mp = mpjpe_error(poses, dev(fx["poses"]), "average").item()
    assert mp <= MPJPE_TOL_M, f"MPJPE vs reference {mp:.3e} m"
    close(poses, fx["poses"], rtol=1e-4, atol=2e-5)
    close(scores, fx["scores"], rtol=1e-4, atol=1e-6)
    assert bool((poses[..., 0, :] == 0).all())
    close(scores.sum(1), torch.ones_like(scores.sum(1)), atol=1e-6)
    if "rot6d" in fx:                                         # intermediates: head output and segment lengths
        K, (B, T) = fx["cfg"]["n_hyp"], X.shape[:2]
        ho = model._engine.peek(0).view(K, B, T, 17, 7)
        close(ho[..., :6].permute(1, 0, 2, 3, 4), fx["rot6d"], rtol=1e-4, atol=2e-5)
        close(model._engine.peek(1).view(B, 16, 1), fx["bones"], rtol=1e-4, atol=2e-6)
    total, terms = rmcl_training_loss(poses, scores, y)
    got = np.array([terms[k].item() for k in ("wloss", "score_reg", "vloss", "sreg")])
    np.testing.assert_allclose(got, fx["loss_terms"], rtol=1e-4)
    total.backward()
    _check_grads(model, fx)
    # eval-time aggregation modes against the reference's outputs
    close(model.aggregate(poses, scores, "weighted_ave"), fx["agg_weighted"], rtol=1e-4, atol=2e-5)
    close(model.aggregate(poses, scores, "best_score"), fx["agg_best"], rtol=1e-4, atol=2e-5)
    oe, op = model.aggregate(poses, mode="oracle", ground_truth=y)
    close(op, fx["agg_oracle"], rtol=1e-4, atol=2e-5)
    close(oe, fx["agg_oracle_err"], rtol=1e-4, atol=2e-6)
    with pytest.raises(ValueError):
        model.aggregate(poses, scores, mode="median")


def test_manifold_single_hypothesis_model_vs_reference(lib):
    from manipose_amd.metrics import manifold_training_loss
    fx = load_fixture("manifold_k1")
    model = _build(fx).eval()
    pred = model(dev(fx["X"]))
    close(pred, fx["poses"], rtol=1e-4, atol=2e-5)
    total, terms = manifold_training_loss(pred, dev(fx["y"]))
    got = np.array([terms[k].item() for k in ("wloss", "vloss", "sreg")])
    np.testing.assert_allclose(got, fx["loss_terms"], rtol=1e-4)
    total.backward()
    _check_grads(model, fx)


def test_droppath_train_mode_with_injected_masks_vs_reference(lib):
    from manipose_amd.metrics import rmcl_training_loss
    fx = load_fixture("rmcl_tiny_droppath")
    model = _build(fx, drop_path_rate=float(fx["drop_path_rate"])).train()
    model.set_droppath_masks({k: v.cuda() for k, v in fixture_masks(fx).items()})
    poses, scores = model(dev(fx["X"]))
    close(poses, fx["poses"], rtol=1e-4, atol=2e-5)
    total, _ = rmcl_training_loss(poses, scores, dev(fx["y"]))
    np.testing.assert_allclose(total.item(), float(fx["loss_total"]), rtol=1e-4)
    total.backward()
    _check_grads(model, fx)


def test_droppath_engine_rng_statistics(lib):
    """Engine-drawn masks: eval == no drop; train differs from eval and the keep frequency matches the rate."""
    fx = load_fixture("rmcl_tiny")
    model = _build(fx, drop_path_rate=0.5)
    X = dev(np.tile(fx["X"], (16, 1, 1, 1)))
    with torch.no_grad():
        p_eval, _ = model.eval()(X)
        p_tr1, _ = model.train()(X)
        p_tr2, _ = model.train()(X)
    close(p_eval[:2], fx["poses"], rtol=1e-4, atol=2e-5)
    assert not torch.allclose(p_eval, p_tr1) and not torch.allclose(p_tr1, p_tr2)
    layout = model._engine.mask_layout(X.shape[0])
    assert [n for n, *_ in layout][:2] == ["rotations_module.STEblocks.0.attn", "rotations_module.STEblocks.0.mlp"]
    assert abs(layout[4][3] - 0.5) < 1e-6 and layout[0][3] == 1.0      # linspace(0, .5, 2) -> keep 1.0, 0.5
    # the masks the engine drew (timm DropPath semantics, mix_ste.py:8,334-336: Bernoulli(keep) / keep per sample of dim 0): values, empirical
    # keep frequency, a pure function of (seed, step), independent across steps
    fx2 = load_fixture("rmcl_tiny")
    big = _build(fx2, drop_path_rate=0.4).train()
    Xb = dev(np.tile(fx2["X"], (128, 1, 1, 1)))
    B = Xb.shape[0]
    with torch.no_grad():
        big._seed, big._step_counter = 7, 0
        big(Xb)
        m1 = big._engine.peek(2).clone()
        big(Xb)
        m2 = big._engine.peek(2).clone()
        big._step_counter = 0
        big(Xb)
        m1_again = big._engine.peek(2).clone()
    assert torch.equal(m1, m1_again) and not torch.equal(m1, m2)
    for name, off, cnt, keep in big._engine.mask_layout(B):
        seg = m1[off:off + cnt]
        if keep >= 1.0:
            assert bool((seg == 1).all()), name
            continue
        vals = torch.unique(seg)
        assert set(vals.tolist()) <= {0.0, float(np.float32(1.0 / keep))}, (name, vals)                 # 0 or 1 / keep
        freq = (seg > 0).float().mean().item()
        sigma = (keep * (1 - keep) / cnt) ** 0.5
        assert abs(freq - keep) < 5 * sigma + 1e-3, (name, freq, keep, cnt)                              # empirical keep frequency
        assert abs(seg.mean().item() - 1.0) < 5 * sigma / keep + 1e-2                                    # E[mask] = 1: the 1 / keep scaling


def test_full_size_model_T243_K5_vs_oracle_and_manifold_property(lib):
    """BASELINE config: T=243, J=17, K=5, C=512, depth 8 at B=1: MPJPE vs the CPU oracle <= 1e-4 m, parameter
    gradients vs the oracle's autograd, and the size-independent manifold property (exact segment lengths)."""
    from manipose_amd import RMCLManifoldMixSTE, h36m_skeleton
    from manipose_amd.metrics import mpjpe_error, rmcl_training_loss
    cfg = orc.FULL_CFG
    st_ = orc.make_state(cfg, seed=3)
    model = RMCLManifoldMixSTE(h36m_skeleton(), drop_path_rate=0.0)
    model.load_state_dict(st_, strict=True)
    model = model.cuda().eval()
    X, y = orc.synthetic_batch(1, 243, seed=42)
    poses, scores = model(X.cuda())
    req = {k: v.clone().requires_grad_(True) for k, v in st_.items()}
    o_poses, o_scores = orc.rmcl_manifold_forward(X, req, orc.oracle_cfg(cfg))
    mp = mpjpe_error(poses, o_poses.detach().cuda(), "average").item()
    assert mp <= MPJPE_TOL_M, f"full-size MPJPE vs oracle {mp:.3e} m"
    close(scores, o_scores.detach(), rtol=1e-3, atol=1e-5)
    total, terms = rmcl_training_loss(poses, scores, y.cuda())
    o_total, o_terms = orc.rmcl_training_loss(o_poses, o_scores, y)
    np.testing.assert_allclose(total.item(), o_total.item(), rtol=1e-4)
    total.backward()
    o_total.backward()
    bad = []
    for k, p in model.named_parameters():
        want = req[k].grad
        err = (p.grad.cpu() - want).abs().max().item() / (want.abs().max().item() + 1e-12)
        if err > 5e-3:
            bad.append((k, err))
    assert not bad, bad[:5]
    # manifold property at full size: every hypothesis/frame has exactly the predicted segment lengths
    par = torch.tensor(orc.H36M_PARENTS[1:], device="cuda")
    seg = (poses[..., 1:, :] - poses[..., par, :]).norm(dim=-1)
    lens = model._engine.peek(1).view(1, 1, 1, 16).abs()
    close(seg, lens.expand_as(seg), rtol=1e-4, atol=2e-6)


def test_two_forwards_before_one_backward_have_ordinary_autograd_semantics(lib):
    """SURVEY 8b "ordinary PyTorch semantics": l1 = f(model(x1)); l2 = f(model(x2)); (l1 + l2).backward() - the engine keeps the activations
    of its last forward only, so the backward of the first graph node re-runs that forward (deterministic: same bits, same DropPath masks)
    before differentiating it.  The accumulated gradient must equal the sum of the two separately computed gradients, in train mode with
    DropPath on, and a retained graph can be differentiated twice."""
    fx = load_fixture("rmcl_tiny")
    model = _build(fx, drop_path_rate=0.3).train()
    X = dev(fx["X"])
    X2 = (X.flip(0) * 0.9).contiguous()

    def grads_of(fn):
        model.zero_grad(set_to_none=True)
        model._step_counter = 0                         # the same DropPath stream positions in every variant
        fn()
        return {k: p.grad.detach().clone() for k, p in model.named_parameters()}

    def f(out):
        return out[0].square().mean() + out[1].square().mean()

    def separate():
        f(model(X)).backward()
        f(model(X2)).backward()

    def joint():
        l1 = f(model(X))
        l2 = f(model(X2))
        (l1 + l2).backward()
    a, b = grads_of(separate), grads_of(joint)
    for k in a:
        assert torch.equal(a[k], b[k]), k                # the re-run forward reproduces the original bits, so the sums are identical
    model.zero_grad(set_to_none=True)
    l = f(model(X))
    l.backward(retain_graph=True)
    g1 = {k: p.grad.detach().clone() for k, p in model.named_parameters()}
    with torch.no_grad():
        model(X2)                                       # an evaluation forward in between
    l.backward()
    for k, p in model.named_parameters():
        close(p.grad, 2 * g1[k], rtol=1e-6, atol=1e-12)


def test_cpu_tensor_is_refused_loudly(lib):
    fx = load_fixture("rmcl_tiny")
    model = _build(fx)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        model(torch.from_numpy(fx["X"]))


# --------------------------------------------------------------------------------------------- bf16 precision (throughput mode)
# measured drift of the bf16 matrix-core mode vs the fp32 reference: 3.1-3.5 mm (fixtures and full size);
# the bound is that + ~25 % margin, so a real accuracy regression of the bf16 kernels fails.  The mode that meets the north-star
# bound (1e-4 m) at matrix-core speed is "bf16x3" below.
BF16_MPJPE_TOL_M = 4.5e-3


@pytest.mark.parametrize("M,N,K", [(306, 96, 32), (130, 48, 16), (4131, 1536, 512), (1000, 512, 1024), (66100, 512, 512)])
def test_bf16_linear_forward_and_backward(lib, M, N, K):
    """bf16 MFMA GEMMs (N/T operand layouts incl. the hardware-transpose-read path) against an fp64 product of the SAME
    bf16-rounded operands: only accumulation order and output rounding differ."""
    _bf16_linear_case(lib, M, N, K)


def test_bf16_linear_tiled_kernels_on_the_persistent_kernel_shape(lib):
    """Same check on the large shape with the persistent kernel switched off (one tile per workgroup)."""
    from manipose_amd import _lib
    _lib.check(lib.mp_set_option(b"gemm_persist_mode", 0))
    try:
        _bf16_linear_case(lib, 66100, 512, 512)
    finally:
        _lib.check(lib.mp_set_option(b"gemm_persist_mode", 1))


def _bf16_linear_case(lib, M, N, K):
    from manipose_amd import _lib
    g = torch.Generator().manual_seed(M * 3 + N + K)
    x, W, b = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) / K ** 0.5, torch.randn(N, generator=g)
    r, dy = torch.randn(M, N, generator=g), torch.randn(M, N, generator=g)
    xb, Wb, dyb = x.bfloat16().cuda(), W.bfloat16().cuda(), dy.bfloat16().cuda()
    bd, rd, dyd = b.cuda(), r.cuda(), dy.cuda()
    ref = xb.double().cpu() @ Wb.double().cpu().T + b.double()
    y = torch.empty(M, N, device="cuda", dtype=torch.bfloat16)
    _lib.check(lib.mp_linear_fwd_bf16(xb.data_ptr(), Wb.data_ptr(), bd.data_ptr(), y.data_ptr(), None, None, M, N, K, 0, st()))
    close(y.float(), ref.float(), rtol=1e-2, atol=1e-2)
    z = torch.empty_like(y)
    _lib.check(lib.mp_linear_fwd_bf16(xb.data_ptr(), Wb.data_ptr(), bd.data_ptr(), y.data_ptr(), z.data_ptr(), None, M, N, K, 1, st()))
    refg = ref.clone().requires_grad_(True)
    torch.nn.functional.gelu(refg).sum().backward()
    close(z.float(), refg.grad.float(), rtol=1e-2, atol=1e-2)      # z keeps gelu'(pre-activation)
    close(y.float(), torch.nn.functional.gelu(ref).float(), rtol=1e-2, atol=1e-2)
    y32 = torch.empty(M, N, device="cuda")
    _lib.check(lib.mp_linear_fwd_bf16(xb.data_ptr(), Wb.data_ptr(), bd.data_ptr(), y32.data_ptr(), None, rd.data_ptr(), M, N, K, 2, st()))
    close(y32, (ref + r.double()).float(), rtol=1e-4, atol=1e-4 * max(1.0, (K / 64) ** 0.5))
    slab = torch.empty(int(lib.mp_linear_bwd_slab_floats(N, K)), device="cuda")
    for dy_f32 in (0, 1):
        dyin = dyd if dy_f32 else dyb
        dyr = (dyd.bfloat16() if dy_f32 else dyb).double().cpu()       # fp32 dY is rounded to bf16 while staging
        dx = torch.empty(M, K, device="cuda")
        dW, db = torch.ones(N, K, device="cuda"), torch.ones(N, device="cuda")
        _lib.check(lib.mp_linear_bwd_bf16(dyin.data_ptr(), dy_f32, xb.data_ptr(), Wb.data_ptr(), dx.data_ptr(), 1, dW.data_ptr(),
                                          db.data_ptr(), M, N, K, slab.data_ptr(), slab.numel(), st()))
        close(dx, (dyr @ Wb.double().cpu()).float(), rtol=1e-4, atol=1e-4 * max(1.0, (N / 64) ** 0.5))
        close(dW, (1 + dyr.T @ xb.double().cpu()).float(), rtol=1e-4, atol=2e-4 * max(1.0, (M / 64) ** 0.5))
        close(db, (1 + dyr.sum(0)).float(), rtol=1e-4, atol=2e-4 * max(1.0, (M / 64) ** 0.5))
    dxb = torch.empty(M, K, device="cuda", dtype=torch.bfloat16)
    dW, db = torch.zeros(N, K, device="cuda"), torch.zeros(N, device="cuda")
    _lib.check(lib.mp_linear_bwd_bf16(dyd.data_ptr(), 1, xb.data_ptr(), Wb.data_ptr(), dxb.data_ptr(), 0, dW.data_ptr(),
                                      db.data_ptr(), M, N, K, slab.data_ptr(), slab.numel(), st()))
    close(dxb.float(), (dyd.bfloat16().double().cpu() @ Wb.double().cpu()).float(), rtol=1e-2, atol=1e-2 * max(1.0, (N / 64) ** 0.5))


def _cos(a, b):
    a, b = a.double().reshape(-1), b.double().reshape(-1)
    return float((a @ b) / (a.norm() * b.norm() + 1e-30))


@pytest.mark.parametrize("name", ["rmcl_tiny", "rmcl_small"])
def test_bf16_precision_model_drift_vs_reference(lib, name):
    """Throughput precision (bf16 matrix cores, fp32 accumulate / residual stream / norms / softmax): drift vs the fp32
    reference is bounded and reported; gradients stay aligned with the reference's."""
    from manipose_amd.metrics import mpjpe_error, rmcl_training_loss
    fx = load_fixture(name)
    model = _build(fx)
    model.precision = "bf16"
    model = model.eval()
    poses, scores = model(dev(fx["X"]))
    mp = mpjpe_error(poses, dev(fx["poses"]), "average").item()
    print(f"\n[bf16 drift] {name}: MPJPE vs fp32 reference = {mp * 1e3:.4f} mm")
    assert mp <= BF16_MPJPE_TOL_M
    total, _ = rmcl_training_loss(poses, scores, dev(fx["y"]))
    assert abs(total.item() - float(fx["loss_total"])) <= 2e-2 * abs(float(fx["loss_total"]))
    total.backward()
    cs = {k: _cos(p.grad.cpu(), torch.from_numpy(fx["g::" + k])) for k, p in model.named_parameters()}
    worst = min(cs.items(), key=lambda kv: kv[1])
    print(f"[bf16 drift] {name}: worst gradient cosine {worst[1]:.5f} at {worst[0]}")
    assert worst[1] > 0.98, worst


@pytest.mark.parametrize("temporal,B,T,J,C,H", [(1, 2, 243, 3, 128, 2), (1, 1, 81, 17, 512, 8), (1, 2, 27, 16, 128, 8),
                                                (1, 1, 256, 2, 64, 1), (1, 1, 17, 2, 32, 2), (1, 1, 300, 2, 128, 2),
                                                (1, 2, 81, 3, 128, 8), (1, 1, 100, 2, 64, 4), (1, 1, 128, 2, 128, 2), (1, 3, 200, 2, 32, 2),
                                                (1, 3, 243, 17, 512, 8), (1, 30, 241, 3, 128, 2), (1, 2, 250, 2, 64, 1),
                                                (0, 1, 9, 17, 128, 2), (0, 2, 5, 17, 512, 8), (0, 1, 7, 16, 128, 8),
                                                (0, 1, 3, 17, 64, 4)])
def test_bf16_attention_forward_backward(lib, temporal, B, T, J, C, H):
    """bf16-storage attention (temporal: MFMA kernels for T <= 256 and head dim 64/16, VALU kernels otherwise) against the
    fp32 formula evaluated on the same bf16-rounded q/k/v and dO."""
    from manipose_amd import _lib
    g = torch.Generator().manual_seed(T * 11 + C)
    M = B * T * J
    qkv_b = torch.randn(M, 3 * C, generator=g).bfloat16()
    dout_b = torch.randn(M, C, generator=g).bfloat16()
    qkv = qkv_b.float().requires_grad_(True)
    ref = _attn_ref(qkv, B, T, J, C, H, temporal)
    (ref * dout_b.float()).sum().backward()
    qd, dod = qkv_b.cuda(), dout_b.cuda()
    out = torch.full((M, C), float("nan"), device="cuda", dtype=torch.bfloat16)      # (NaN, not zeros: an element never written must not read as a value)
    lse = torch.full((B * J * H * T,), float("nan"), device="cuda")
    _lib.check(lib.mp_attention_fwd_bf16(qd.data_ptr(), out.data_ptr(), lse.data_ptr(), temporal, B, T, J, C, H, st()))
    close(out.float(), ref, rtol=2e-2, atol=2e-2)
    dq = torch.full((M, 3 * C), float("nan"), device="cuda", dtype=torch.bfloat16)
    delta = torch.empty(B * J * H * T, device="cuda")
    _lib.check(lib.mp_attention_bwd_bf16(qd.data_ptr(), out.data_ptr(), dod.data_ptr(), lse.data_ptr(), delta.data_ptr(),
                                         dq.data_ptr(), temporal, B, T, J, C, H, st()))
    got, want = dq.float().cpu(), qkv.grad
    assert _cos(got, want) > 0.999, _cos(got, want)
    close(got, want, rtol=5e-2, atol=5e-2 * float(want.abs().max()))


def test_bf16_full_size_model_drift_vs_oracle(lib):
    """BASELINE config #3 (T=243 K=5 C=512 depth 8, bf16 matrix cores incl. the MFMA attention kernels) at B=1 against
    the fp32 CPU oracle: reports the MPJPE drift of the throughput precision and checks gradient alignment."""
    from manipose_amd import RMCLManifoldMixSTE, h36m_skeleton
    from manipose_amd.metrics import mpjpe_error, rmcl_training_loss
    cfg = orc.FULL_CFG
    st_ = orc.make_state(cfg, seed=3)
    model = RMCLManifoldMixSTE(h36m_skeleton(), drop_path_rate=0.0)
    model.load_state_dict(st_, strict=True)
    model.precision = "bf16"
    model = model.cuda().eval()
    X, y = orc.synthetic_batch(1, 243, seed=42)
    poses, scores = model(X.cuda())
    req = {k: v.clone().requires_grad_(True) for k, v in st_.items()}
    o_poses, o_scores = orc.rmcl_manifold_forward(X, req, orc.oracle_cfg(cfg))
    mp = mpjpe_error(poses, o_poses.detach().cuda(), "average").item()
    print(f"\n[bf16 drift] full size T=243 K=5: MPJPE vs fp32 oracle = {mp * 1e3:.4f} mm")
    assert mp <= BF16_MPJPE_TOL_M
    total, _ = rmcl_training_loss(poses, scores, y.cuda())
    o_total, _ = orc.rmcl_training_loss(o_poses, o_scores, y)
    assert abs(total.item() - o_total.item()) <= 2e-2 * abs(o_total.item())
    total.backward()
    o_total.backward()
    cs = {k: _cos(p.grad.cpu(), req[k].grad) for k, p in model.named_parameters()}
    worst = min(cs.items(), key=lambda kv: kv[1])
    mean = sum(cs.values()) / len(cs)
    print(f"[bf16 drift] full size: gradient cosine mean {mean:.5f}, worst {worst[1]:.5f} at {worst[0]}")
    assert worst[1] > 0.9 and mean > 0.99, (worst, mean)
    par = torch.tensor(orc.H36M_PARENTS[1:], device="cuda")
    seg = (poses[..., 1:, :] - poses[..., par, :]).norm(dim=-1)       # the manifold property is exact in any precision
    lens = model._engine.peek(1).view(1, 1, 1, 16).abs()
    close(seg, lens.expand_as(seg), rtol=1e-4, atol=2e-6)


def test_bf16_droppath_train_mode_with_injected_masks(lib):
    """Train-mode DropPath in the bf16 precision (mask scaling folded into GEMM epilogues and the LN-backward bf16 copy)."""
    from manipose_amd.metrics import mpjpe_error, rmcl_training_loss
    fx = load_fixture("rmcl_tiny_droppath")
    model = _build(fx, drop_path_rate=float(fx["drop_path_rate"]))
    model.precision = "bf16"
    model = model.train()
    model.set_droppath_masks({k: v.cuda() for k, v in fixture_masks(fx).items()})
    poses, scores = model(dev(fx["X"]))
    # keep = 0.5 doubles the surviving branches, so this fixture's poses (joints up to 1.3 m from the root) amplify the bf16
    # rounding noise: bound the drift relative to the mean joint distance instead of in absolute millimetres
    ref = dev(fx["poses"])
    rel = mpjpe_error(poses, ref, "average").item() / ref.norm(dim=-1).mean().item()
    assert rel <= 0.03, rel
    total, _ = rmcl_training_loss(poses, scores, dev(fx["y"]))
    assert abs(total.item() - float(fx["loss_total"])) <= 2e-2 * abs(float(fx["loss_total"]))
    total.backward()
    cs = {k: _cos(p.grad.cpu(), torch.from_numpy(fx["g::" + k])) for k, p in model.named_parameters()}
    worst = min(cs.items(), key=lambda kv: kv[1])
    assert worst[1] > 0.98, worst


def test_batched_flip_tta_matches_two_pass_reference_procedure(lib):
    """Eval with flip test-time augmentation (hpe/eval_utils.py:76-142): the batched single-pass version of the entry
    point equals the reference's two-pass procedure evaluated with the CPU oracle on the same weights."""
    import os, sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "hpe"))
    from _entry import evaluate
    from manipose_amd.augmentations import pose_flip
    from manipose_amd.data import h36m_skeleton
    fx = load_fixture("rmcl_small")
    model = _build(fx).eval()
    X, y = torch.from_numpy(fx["X"]), torch.from_numpy(fx["y"])
    got = evaluate(model, X.cuda(), y.cuda(), batch=2, tta=True)
    st_, cfg, sk = fixture_state(fx), orc.oracle_cfg(fx["cfg"]), h36m_skeleton()
    p0, s0 = orc.rmcl_manifold_forward(X, st_, cfg)
    p1, s1 = orc.rmcl_manifold_forward(pose_flip((X.clone(),), sk)[0], st_, cfg)
    pred = (orc.aggregate(p0, s0) + pose_flip((orc.aggregate(p1, s1),), sk)[0]) / 2
    want = 1000.0 * orc.mpjpe_error(pred, y).item()
    assert abs(got["mpjpe"] - want) <= 1e-3 * want + 0.05, (got, want)
    hyp_f = pose_flip((p1.clone(),), sk)[0]
    orac = (orc.aggregate(p0, mode="oracle", ground_truth=y)[1] + orc.aggregate(hyp_f, mode="oracle", ground_truth=y)[1]) / 2
    want_o = 1000.0 * orc.mpjpe_error(orac, y).item()
    assert abs(got["oracle_mpjpe"] - want_o) <= 1e-3 * want_o + 0.05, (got, want_o)


def test_bf16_persistent_gemm_path_matches_tiled_path(lib):
    """The persistent 256x256 GEMM kernel (used from 512 output tiles up, i.e. only at training batch sizes) forced on at
    small sizes: forward outputs and every gradient of the train-mode (DropPath masks injected) bf16 model must agree with
    the one-tile-per-workgroup kernels, which the fixtures above pin to the reference."""
    from manipose_amd import RMCLManifoldMixSTE, _lib, h36m_skeleton
    B, T = 6, 27
    outs = []
    for min_tiles in (0, 1):                              # tiled kernels (too few tiles for the default rule) / persistent kernel forced
        _lib.check(lib.mp_set_option(b"gemm_persist_min_tiles", min_tiles))
        try:
            torch.manual_seed(7)
            model = RMCLManifoldMixSTE(n_hyp=3, skeleton=h36m_skeleton(), num_frame=T, embed_dim_rot=256, depth_rot=2, num_heads_rot=4,
                                       embed_dim_seg=256, depth_seg=2, num_heads_seg=4, drop_path_rate=0.3).cuda().train()
            model.precision = "bf16"
            x = torch.randn(B, T, 17, 2, generator=torch.Generator().manual_seed(3)).cuda()
            model.flat_parameters()
            model._ensure_engine(B, x.device)
            gen = torch.Generator().manual_seed(11)
            model.set_droppath_masks({name: (torch.rand(cnt, generator=gen) > 0.3).float() / 0.7
                                      for name, _, cnt, _ in model._engine.mask_layout(B)})
            poses, scores = model(x)
            (poses.square().sum() + scores.square().sum()).backward()
            outs.append((poses.detach().clone(), scores.detach().clone(),
                         torch.cat([p.grad.reshape(-1) for p in model.parameters()]).clone()))
        finally:
            _lib.check(lib.mp_set_option(b"gemm_persist_min_tiles", 0))
    for o in outs[1:]:
        assert torch.isfinite(o[2]).all()
        close(outs[0][0], o[0], rtol=1e-5, atol=1e-5)
        close(outs[0][1], o[1], rtol=1e-5, atol=1e-5)
        assert _cos(outs[0][2], o[2]) > 0.99999
        assert (outs[0][2] - o[2]).abs().max() <= 1e-4 * outs[0][2].abs().max()


# --------------------------------------------------------------------------------- evaluation analytics
def _close_rel(got, want, rtol=2e-4, atol=0.0):
    got = got.detach().cpu().double().numpy() if isinstance(got, torch.Tensor) else np.asarray(got, dtype=np.float64)
    np.testing.assert_allclose(got, np.asarray(want, dtype=np.float64), rtol=rtol, atol=atol)


@pytest.mark.parametrize("nm", ["pred", "rigid"])
def test_consistency_metrics_match_reference_fixture(lib, nm):
    """segments_time_consistency / sagittal_symmetry / segments_len_err (+ per-bone forms) from the one-pass HIP kernel against
    the outputs of the reference's own functions; 'rigid' has constant bone lengths (time variance ~ rounding noise)."""
    from manipose_amd import h36m_skeleton
    from manipose_amd.metrics import (sagittal_symmetry, sagittal_symmetry_per_bone, segments_len_err, segments_time_consistency,
                                      segments_time_consistency_per_bone)
    fx, sk = load_fixture("metrics"), h36m_skeleton()
    jc = dev(fx[nm]).permute(0, 3, 2, 1)                  # (B, 3, J, L) view, read through its strides (no copy)
    gj = dev(fx["gt"]).permute(0, 3, 2, 1)
    # variance of lengths ~250 mm known to ~2e-5 mm: absolute floor for the rigid case
    vat, sat = (1e-6, 1e-3) if nm == "rigid" else (0.0, 0.0)
    for mode in ("average", "sum", "min", "max"):
        _close_rel(segments_time_consistency(jc, sk, mode), fx[f"{nm}.stc.{mode}"], atol=vat * (48 if mode == "sum" else 1))
    _close_rel(segments_time_consistency(jc, sk, "std"), fx[f"{nm}.stc.std"], atol=sat)
    for mode in ("average", "sum"):
        _close_rel(segments_time_consistency_per_bone(jc, sk, mode), fx[f"{nm}.stc_per_bone.{mode}"], atol=vat * 3)
    _close_rel(segments_time_consistency_per_bone(jc, sk, "std"), fx[f"{nm}.stc_per_bone.std"], atol=sat)
    flat = jc.permute(1, 2, 0, 3).reshape(1, 3, 17, -1)   # the evaluation call: batch flattened into time (903 frames, 4 chunks)
    _close_rel(segments_time_consistency(flat, sk, "std"), fx[f"{nm}.stc_flat.std"], atol=sat)
    for sq in (False, True):
        for mode in ("average", "sum"):
            _close_rel(sagittal_symmetry(jc, sk, mode, squared=sq), fx[f"{nm}.sym.{mode}.{int(sq)}"])
            _close_rel(sagittal_symmetry_per_bone(jc, sk, mode, squared=sq), fx[f"{nm}.sym_per_bone.{mode}.{int(sq)}"])
    for signed in (False, True):
        for mode in ("average", "sum"):
            want = fx[f"{nm}.len_err.{mode}.{int(signed)}"]
            # the signed sum cancels: bound it by the unsigned scale
            _close_rel(segments_len_err(jc, gj, sk, mode, signed=signed), want,
                       atol=2e-4 * abs(float(fx[f"{nm}.len_err.{mode}.0"])))
    with pytest.raises(ValueError):
        segments_time_consistency(jc, sk, "median")
    with pytest.raises(ValueError):
        sagittal_symmetry(jc, sk, "max")


@pytest.mark.parametrize("nm", ["pred", "rigid"])
def test_error_metrics_and_pck_auc_match_reference_fixture(lib, nm):
    from manipose_amd.metrics import (jointwise_error, jointwise_mse, keypoint_3d_auc, keypoint_3d_pck, mpjpe_error, mse_error,
                                      pose_analytics)
    fx = load_fixture("metrics")
    x, gt = dev(fx[nm]), dev(fx["gt"])
    for mode in ("average", "sum"):
        _close_rel(mpjpe_error(x, gt, mode), fx[f"{nm}.mpjpe.{mode}"])
        _close_rel(mse_error(x, gt, mode), fx[f"{nm}.mse.{mode}"])
        _close_rel(jointwise_error(x, gt, mode), fx[f"{nm}.jw_err.{mode}"])
        _close_rel(jointwise_mse(x, gt, mode), fx[f"{nm}.jw_mse.{mode}"])
    r = pose_analytics(x, gt)                               # velocity error sums: one pass, both forms
    n = x.shape[0] * (x.shape[1] - 1) * 17
    _close_rel(r.scalar(9) / n, fx[f"{nm}.vel"])
    _close_rel(r.scalar(10) / (3 * n), fx[f"{nm}.vel_sq"])
    xf, gf = x.reshape(-1, 17, 3), gt.reshape(-1, 17, 3)
    tol = 100.0 * 3 / (xf.shape[0] * 17)                   # at most a few joints within rounding of a threshold
    for al in ("none", "scale"):
        assert abs(keypoint_3d_pck(xf, gf, None, al, 150) - float(fx[f"{nm}.pck.{al}"])) <= tol
        assert abs(keypoint_3d_auc(xf, gf, None, al) - float(fx[f"{nm}.auc.{al}"])) <= tol
    assert abs(keypoint_3d_pck(xf.cpu().numpy(), gf.cpu().numpy(), fx["mask"], "none", 150) - float(fx[f"{nm}.pck.masked"])) <= 2 * tol
    assert abs(keypoint_3d_auc(xf, gf, fx["mask"], "none") - float(fx[f"{nm}.auc.masked"])) <= 2 * tol
    assert abs(keypoint_3d_pck(xf, gf, None, "none", 80) - float(fx[f"{nm}.pck.thr80"])) <= tol
    # Procrustes-aligned metrics: Horn's closed form on the device against the reference's numpy SVD
    from manipose_amd.metrics import p_mpjpe
    assert abs(p_mpjpe(x, gt) - float(fx[f"{nm}.p_mpjpe"])) <= 2e-4 * float(fx[f"{nm}.p_mpjpe"])
    assert abs(keypoint_3d_pck(xf, gf, None, "procrustes", 150) - float(fx[f"{nm}.pck.procrustes"])) <= tol
    assert abs(keypoint_3d_auc(xf, gf, None, "procrustes") - float(fx[f"{nm}.auc.procrustes"])) <= tol
    assert abs(keypoint_3d_pck(xf, gf, fx["mask"], "procrustes", 150) - float(fx[f"{nm}.pck.procrustes.masked"])) <= 2 * tol
    rot = torch.linalg.qr(torch.randn(3, 3, generator=torch.Generator().manual_seed(1)))[0].cuda()      # an exactly similar copy aligns to 0
    if torch.linalg.det(rot) < 0:
        rot[:, 0] *= -1
    assert p_mpjpe((0.37 * gt @ rot + 5.0), gt) <= 1e-3
    with pytest.raises(ValueError):
        keypoint_3d_auc(xf, gf, None, "affine")


def test_pose_analytics_refuses_cpu_tensors_and_foreign_skeletons(lib):
    from manipose_amd.data.skeleton import Skeleton, T_POSE_OPERATORS
    from manipose_amd.metrics import pose_analytics, sagittal_symmetry
    x = torch.zeros(1, 4, 17, 3)
    with pytest.raises(RuntimeError):
        pose_analytics(x)
    other = Skeleton([-1, 0, 1, 2, 0, 4, 5, 0, 7, 8, 9, 8, 11, 12, 8, 14, 14], [4, 5, 6, 11, 12, 13], [1, 2, 3, 14, 15, 16], T_POSE_OPERATORS)
    with pytest.raises(AssertionError):
        sagittal_symmetry(x.cuda().permute(0, 3, 2, 1), other, "average")


def test_evaluate_analytics_table_matches_oracle_on_the_flattened_sequence(lib):
    """hpe entry evaluate(analytics=True): the accumulated table (batches merged into ONE sequence like the reference's
    (1,3,J,B*L) reshape, shifted variance sums re-centred across batches) against the oracle restatement applied to the
    concatenated aggregated predictions."""
    import os, sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "hpe"))
    from _entry import evaluate
    fx = load_fixture("rmcl_small")
    model = _build(fx).eval()
    g = torch.Generator().manual_seed(21)
    X = torch.cat([torch.from_numpy(fx["X"]), 0.3 * torch.randn(3, 27, 17, 2, generator=g)]).cuda()
    y = torch.cat([torch.from_numpy(fx["y"]), 0.3 * torch.randn(3, 27, 17, 3, generator=g)]).cuda()
    y[:, :, 0] = 0
    got = evaluate(model, X, y, batch=2, tta=False, analytics=True)["analytics"]
    with torch.no_grad():
        poses, scores = model(X)
        pred = (model.aggregate(poses, scores, "weighted_ave") * 1000.0).cpu()
    gt = (y * 1000.0).cpu()
    jc, gj = pred.permute(0, 3, 2, 1), gt.permute(0, 3, 2, 1)
    flat = jc.permute(1, 2, 0, 3).reshape(1, 3, 17, -1)
    want = {"mpjpe": orc.mpjpe_error(pred, gt).item(), "mse": orc.mse_error(pred, gt).item(),
            "mpsse": orc.sagittal_symmetry(jc, "average", False).item(), "mpsce": orc.segments_time_consistency(flat, "std").item(),
            "seg_len_err": orc.segments_len_err(jc, gj, "average", False).item()}
    pck, auc = orc.keypoint_3d_pck_auc(pred.reshape(-1, 17, 3), gt.reshape(-1, 17, 3))
    for k, v in want.items():
        assert abs(got[k] - v) <= 2e-4 * abs(v) + 1e-3, (k, got[k], v)
    assert abs(got["pck"] - pck.item()) <= 0.2 and abs(got["auc"] - auc.item()) <= 0.2
    assert abs(got["err_var"] - (want["mse"] - want["mpjpe"] ** 2)) <= 1e-3 * want["mse"]
    assert abs(got["p_mpjpe"] - orc.p_mpjpe(pred, gt).item()) <= 2e-4 * got["p_mpjpe"] + 1e-3


# ------------------------------------------------------------------------------------ GPU-resident input pipeline
WINDOW_CASES = {"strided_drop": (False, True, False), "strided_pad": (False, False, False), "random_flip": (True, True, True),
                "strided_pad_flip": (False, False, True)}


@pytest.mark.parametrize("case", sorted(WINDOW_CASES))
def test_window_generator_is_bit_exact_with_the_reference_generator(lib, case):
    """PoseSequenceGenerator + PoseFlip on the device (one gather kernel per batch) against the windows the reference's generator
    produced item by item under the same torch seed: index tables, random starts, replicate padding, flip decisions, mirroring."""
    from manipose_amd import h36m_skeleton
    from manipose_amd.augmentations import PoseFlip
    from manipose_amd.data import PoseSequenceGenerator
    fx = load_fixture("windows")
    n = len(fx["lens"])
    p3, p2 = [fx[f"p3.{i}"] for i in range(n)], [fx[f"p2.{i}"] for i in range(n)]
    random_start, drop_last, flip = WINDOW_CASES[case]
    gen = PoseSequenceGenerator(p3, p2, None, seq_len=27, random_start=random_start, drop_last=drop_last,
                                transform=PoseFlip(h36m_skeleton(), 0.5) if flip else None)
    assert len(gen) == int(fx[f"{case}.len"])
    torch.manual_seed(2024)
    X, y = gen.batch(range(len(gen)))                      # one launch for the whole epoch
    assert torch.equal(X.cpu(), torch.from_numpy(fx[f"{case}.X"])) and torch.equal(y.cpu(), torch.from_numpy(fx[f"{case}.y"]))
    torch.manual_seed(2024)
    x0, y0 = gen[0]                                          # the reference's per-item interface
    assert torch.equal(x0.cpu(), torch.from_numpy(fx[f"{case}.X"][0])) and torch.equal(y0.cpu(), torch.from_numpy(fx[f"{case}.y"][0]))


def test_window_generator_properties_at_training_size(lib):
    """T = 243 windows out of long sequences: mirroring twice is the identity, un-flipped windows are verbatim slices, frames past the
    end of a sequence repeat its last frame; unsupported options fail loudly."""
    from manipose_amd import h36m_skeleton
    from manipose_amd.augmentations import PoseFlip, pose_flip
    from manipose_amd.data import PoseSequenceGenerator
    g = np.random.default_rng(5)
    lens = [3000, 1700, 2431]
    p3 = [g.normal(size=(n, 17, 3)).astype(np.float32) for n in lens]
    p2 = [g.normal(size=(n, 17, 2)).astype(np.float32) for n in lens]
    sk = h36m_skeleton()
    gen = PoseSequenceGenerator(p3, p2, None, seq_len=243, random_start=False, drop_last=False, transform=PoseFlip(sk, 0.5))
    assert len(gen) == sum(-(-n // 243) for n in lens)
    seq = torch.tensor([0, 0, 1, 2, 2], dtype=torch.int32)
    start = torch.tensor([0, 2916, 1500, 243, 2430], dtype=torch.int32)
    X, y = gen.gather(seq, start, torch.zeros(5, dtype=torch.uint8))
    Xf, yf = gen.gather(seq, start, torch.ones(5, dtype=torch.uint8))
    assert torch.equal(X[0].cpu(), torch.from_numpy(p2[0][:243])) and torch.equal(y[2, :200].cpu(), torch.from_numpy(p3[1][1500:1700]))
    assert torch.equal(y[1, :84].cpu(), torch.from_numpy(p3[0][2916:3000])) and bool((y[1, 84:] == y[1, 83]).all())     # replicate padding
    assert bool((y[4, 1:] == y[4, 0]).all())
    Xb, yb = pose_flip((Xf.clone(), yf.clone()), sk)       # mirroring the mirrored windows on the host side gives the originals back
    assert torch.equal(Xb, X) and torch.equal(yb, y)
    with pytest.raises(RuntimeError):
        PoseSequenceGenerator(p3, p2, None, seq_len=243, device="cpu")


def test_training_entry_runs_on_resident_sequences(lib, tmp_path, monkeypatch):
    """hpe/main_h36m_lifting.py (the reference's entry point and override grammar) end to end on a small model: windows drawn by the
    GPU-resident generator with flip augmentation, two training steps, validation, checkpoint, analytics table."""
    import os, sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "hpe"))
    from _entry import run
    monkeypatch.chdir(tmp_path)
    best = run(["train.epochs=1", "train.steps_per_epoch=2", "train.batch_size=4", "train.batch_size_test=2", "data.seq_len=27",
                "model.channels=64", "model.layers=2", "model.nheads=4", "model.channels_seg=32", "model.layers_seg=1",
                "model.nheads_seg=4", "multi_hyp.n_hyp=3", "data.synthetic_sequences=6", "run.test=true"])
    assert np.isfinite(best) and best < 1e9
    assert any(f.endswith(".pth") for _, _, fs in os.walk(tmp_path) for f in fs)
    # resume (run.checkpoint_model / run.checkpoint_params, main_h36m_lifting.py:225-285,755-761): weights, Adam moments, scheduler, epoch
    d = os.path.join(str(tmp_path), "default")
    for f in ("model_end.pth", "params_end.pth", "model_best_val.pth", "params_best_val.pth", "train_loss.npy", "valid_loss.npy"):
        assert os.path.exists(os.path.join(d, f)), f
    st = torch.load(os.path.join(d, "params_end.pth"), map_location="cpu")
    assert st["epoch"] == 1 and st["scheduler"]["kind"] == "plateau"
    opt_state = st["optimizer"]                                        # torch.optim.Adam's layout (interchangeable with the reference's files)
    assert float(opt_state["state"][0]["step"]) == 2 and opt_state["param_groups"][0]["lr"] == 4e-5 and len(opt_state["state"]) > 50
    best2 = run(["train.epochs=2", "train.steps_per_epoch=2", "train.batch_size=4", "train.batch_size_test=2", "data.seq_len=27",
                 "model.channels=64", "model.layers=2", "model.nheads=4", "model.channels_seg=32", "model.layers_seg=1",
                 "model.nheads_seg=4", "multi_hyp.n_hyp=3", "data.synthetic_sequences=6", "run.test=false", "run.experiment=resumed",
                 f"run.checkpoint_model={d}/model_end.pth", f"run.checkpoint_params={d}/params_end.pth", "train.mpjpe_epoch_interval=1"])
    st2 = torch.load(os.path.join(str(tmp_path), "resumed", "params_end.pth"), map_location="cpu")
    assert float(st2["optimizer"]["state"][0]["step"]) == 4 and np.isfinite(best2)    # one more epoch of two steps on top of the restored moments
    assert os.path.exists(os.path.join(str(tmp_path), "resumed", "model_best_mpjpe.pth"))


@pytest.mark.parametrize("mt", ["random", "random_left_arm_right_leg", "structured_joint", "structured_frame", "noisy", "all"])
def test_window_generator_occlusion_patterns_match_reference(lib, mt):
    """The generator's occlusion patterns (host-side numpy draws in the reference's order, applied by the gather kernel) against the
    reference's generator under the same torch / numpy seeds; bit-exact except 'noisy' (the reference's result is float64 there:
    one float32 ulp)."""
    from manipose_amd import h36m_skeleton
    from manipose_amd.augmentations import PoseFlip
    from manipose_amd.data import PoseSequenceGenerator
    fx = load_fixture("windows")
    n = len(fx["lens"])
    p3, p2 = [fx[f"p3.{i}"] for i in range(n)], [fx[f"p2.{i}"] for i in range(n)]
    gen = PoseSequenceGenerator(p3, p2, None, seq_len=27, random_start=True, drop_last=True, miss_type=mt, miss_rate=0.3,
                                noise_sigma=0.05, transform=PoseFlip(h36m_skeleton(), 0.5))
    torch.manual_seed(77)
    np.random.seed(99)
    X, y = gen.batch(range(len(gen)))
    assert torch.equal(y.cpu(), torch.from_numpy(fx[f"miss.{mt}.y"]))
    want = torch.from_numpy(fx[f"miss.{mt}.X"])
    if mt == "noisy":
        np.testing.assert_allclose(X.cpu().numpy(), want.numpy(), rtol=3e-7, atol=1e-7)
    else:
        assert torch.equal(X.cpu(), want.float())
    with pytest.raises(ValueError):
        PoseSequenceGenerator(p3, p2, None, seq_len=27, miss_type="checkerboard")


# ---------------------------------------------------------------------------------------------------------------------------------
# dataset ingest (the on-disk formats either side of the window generator): HIP kernels vs what the reference's loaders made of the
# same files (tests/golden/datasets.npz) and vs the oracle restatement
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,subjects,filt,stride", [("all", ["S1", "S9"], None, 1), ("walk_s2", ["S9", "S11"], ["walking"], 2),
                                                       ("s11_sit", ["S11"], ["sittingdown"], 1)])
def test_h36m_dataset_ingest_matches_reference_loaders(lib, raw_dataset_dir, case, subjects, filt, stride):
    from manipose_amd.data import Human36mDataset, create_2d_data, fetch, read_3d_data
    d, fx = raw_dataset_dir
    ds = read_3d_data(Human36mDataset(d + "/data_3d_h36m.npz", n_joints=17))
    kp = create_2d_data(d + "/data_2d_h36m_gt.npz", ds)
    p3, p2, actions, cams = fetch(subjects, ds, kp, filt, stride)
    assert len(p3) == len(p2) == int(fx[f"h36m.{case}.n"]) and actions == list(fx[f"h36m.{case}.actions"])
    assert list(ds.skeleton.parents) == list(fx["h36m.parents"]) and list(ds.skeleton.joints_left) == list(fx["h36m.joints_left"])
    worst = 0.0
    for i in range(len(p3)):
        assert p3[i].is_cuda and p2[i].is_cuda
        np.testing.assert_array_equal(p2[i].cpu().numpy(), fx[f"h36m.{case}.p2.{i}"])                 # bit-exact
        ref3 = fx[f"h36m.{case}.p3.{i}"]
        worst = max(worst, float(np.abs(p3[i].cpu().numpy() - ref3).max()))
        np.testing.assert_allclose(cams[i], fx[f"h36m.{case}.cam.{i}"], rtol=0, atol=0)
    assert worst <= 2e-6, worst        # metres; the reference's torch.cross may contract multiply-adds, the kernel does not
    print(f"h36m ingest {case}: {len(p3)} sequences, worst |d| = {worst:.2e} m")


@pytest.mark.parametrize("split", ["train", "test"])
def test_3dhp_dataset_ingest_matches_reference_loader_bit_exact(lib, raw_dataset_dir, split):
    from types import SimpleNamespace as NS
    from manipose_amd.data import Dataset3DHP
    d, fx = raw_dataset_dir
    cfg = NS(data=NS(dataset="3dhp", keypoints="gt", actions="*", seq_len=27), train=NS(flip_aug=True, batch_size=2, batch_size_test=2, tta=True))
    hp = Dataset3DHP(cfg, d + "/", train=(split == "train"))
    assert len(hp.poses) == len(hp.poses_2d) == int(fx[f"hp.{split}.n"])
    for i in range(len(hp.poses)):
        np.testing.assert_array_equal(hp.poses[i].cpu().numpy(), fx[f"hp.{split}.p3.{i}"])
        np.testing.assert_array_equal(hp.poses_2d[i].cpu().numpy(), fx[f"hp.{split}.p2.{i}"])


def test_ingested_sequences_feed_the_window_generator_without_leaving_the_device(lib, raw_dataset_dir):
    """files -> ingest kernels -> resident generator -> window kernel; windows equal slices of the reference loader's sequences."""
    from manipose_amd.data import Human36mDataset, PoseSequenceGenerator, create_2d_data, fetch, read_3d_data
    d, fx = raw_dataset_dir
    ds = read_3d_data(Human36mDataset(d + "/data_3d_h36m.npz"))
    p3, p2, _, cams = fetch(["S1", "S9"], ds, create_2d_data(d + "/data_2d_h36m_gt.npz", ds))
    gen = PoseSequenceGenerator(p3, p2, cams, seq_len=9, random_start=False, drop_last=True)
    X, y = gen.batch(list(range(len(gen))))
    n = 0
    for i in range(len(p3)):
        for k in range(p3[i].shape[0] // 9):
            np.testing.assert_array_equal(X[n].cpu().numpy(), fx[f"h36m.all.p2.{i}"][9 * k:9 * k + 9])
            assert np.abs(y[n].cpu().numpy() - fx[f"h36m.all.p3.{i}"][9 * k:9 * k + 9]).max() <= 2e-6
            n += 1
    assert n == len(gen) and torch.all(y[:, :, 0] == 0)


def test_ingest_argument_errors_are_reported(lib):
    from manipose_amd import _lib as L
    from manipose_amd.data.ingest import ingest_pose2d, ingest_pose3d
    raw = torch.zeros(4, 17, 3, device="cuda")
    with pytest.raises(RuntimeError):
        ingest_pose3d(raw, [0, 17])                                   # joint outside the raw array
    with pytest.raises(RuntimeError):
        ingest_pose3d(raw, list(range(17)), orientation=[1, 0, 0, 0])   # orientation without translation
    with pytest.raises(RuntimeError):
        ingest_pose2d(torch.zeros(4, 17, 2, device="cuda"), list(range(17)), 0, 1000)
    assert ingest_pose3d(raw[:0].contiguous(), list(range(17))).shape == (0, 17, 3)


@pytest.mark.parametrize("dataset", ["h36m", "3dhp"])
def test_training_entry_reads_the_reference_file_formats(lib, raw_dataset_dir, tmp_path, monkeypatch, capsys, dataset):
    """Entry point with data.data_dir: files in the reference's formats -> device ingest -> resident window generator -> one epoch
    over the shuffled windows, validation, checkpoint, per-action (H36M, subject S11) / whole-set (3DHP) test tables."""
    import os, sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "hpe"))
    from _entry import run
    d, _ = raw_dataset_dir
    monkeypatch.chdir(tmp_path)
    best = run(["train.epochs=1", "train.batch_size=4", "train.batch_size_test=3", "data.seq_len=9", f"data.data_dir={d}",
                "data.keypoints=gt", "model.channels=64", "model.layers=2", "model.nheads=4", "model.channels_seg=32",
                "model.layers_seg=1", "model.nheads_seg=4", "multi_hyp.n_hyp=3", "run.test=true", "train.mpjpe_epoch_interval=1"],
               extra_defaults={"data.dataset": dataset})
    out = capsys.readouterr().out
    assert np.isfinite(best) and best < 1e9
    assert ">>> Training dataset length:" in out and "epoch 0:" in out and "eval:" in out
    if dataset == "h36m":
        assert "test [walking]:" in out and "test [sittingdown]:" in out and "test [average over groups]:" in out   # S11's two takes
    else:
        assert "test [all]:" in out and "pck" in out.lower()
    assert any(f.endswith(".pth") for _, _, fs in os.walk(tmp_path) for f in fs)


def test_squared_loss_mode_vs_reference_fixture(lib):
    """train.sq_loss=True: squared WTA + velocity terms and their gradients, multi-hypothesis and single-hypothesis,
    against the reference's own loss functions (tests/golden/loss_sq.npz)."""
    from manipose_amd import metrics as M
    fx = load_fixture("loss_sq")
    poses = dev(fx["poses"]).requires_grad_(True)
    scores = dev(fx["scores"]).requires_grad_(True)
    y = dev(fx["y"])
    total, terms = M.rmcl_training_loss(poses, scores, y, sq_loss=True)
    total.backward()
    np.testing.assert_allclose([terms[k].item() for k in ("wloss", "score_reg", "vloss", "sreg")], fx["loss_terms"], rtol=2e-5)
    close(poses.grad, fx["g_poses"], rtol=1e-4, atol=1e-8)
    close(scores.grad, fx["g_scores"], rtol=1e-4, atol=1e-8)
    val, idx = M.wta_l2_loss_and_activate_head(poses.detach(), y, weights=M.STANDARD_H36M_WEIGHTS, squared=True)
    assert np.array_equal(idx.cpu().numpy(), fx["wta_idx"])
    close(val, fx["wta_vals"], rtol=1e-5, atol=1e-8)
    close(M.mean_velocity_error(poses.detach(), y, axis=2, squared=True) * 2.0, fx["loss_terms"][2], rtol=2e-5)
    for nm, w_loss in (("w", True), ("nw", False)):
        p1 = dev(fx["poses"][:, 0].copy()).requires_grad_(True)
        tot, t = M.manifold_training_loss(p1, y, w_loss=w_loss, sq_loss=True)
        tot.backward()
        np.testing.assert_allclose([t[k].item() for k in ("wloss", "vloss", "sreg")], fx[f"single_{nm}.terms"], rtol=2e-5)
        close(p1.grad, fx[f"single_{nm}.g"], rtol=1e-4, atol=1e-8)
    close(M.weighted_mse_loss(dev(fx["poses"][:, 0].copy()), y, weights=M.STANDARD_H36M_WEIGHTS), fx["single_w.terms"][0], rtol=2e-5)


# ---------------------------------------------------------------------------------------------------------------------------------
# model.rot_dim=4: 4-D rotation representation (rotation_tools.py:60-116) in the decoder kernel and the engine
# ---------------------------------------------------------------------------------------------------------------------------------
def test_rot4_fk_decode_forward_backward_vs_reference_fixture(lib):
    from manipose_amd import _lib, h36m_skeleton
    from manipose_amd.architectures.pose_decoder import PoseDecoder
    fx = load_fixture("decoder_rot4")
    B, L = 3, 7
    rot = dev(fx["rot4d"]).requires_grad_(True)
    bl = dev(fx["bones"]).requires_grad_(True)
    dec = PoseDecoder(h36m_skeleton(), rot_rep_dim=4)
    poses = dec(rot, bl, torch.zeros(B * L, 3, device="cuda"))
    close(poses, fx["poses"], rtol=1e-5, atol=2e-6)
    (poses * dev(fx["gpos"])).sum().backward()
    close(rot.grad, fx["g_rot4d"], rtol=2e-4, atol=2e-5)
    close(bl.grad, fx["g_bones"], rtol=2e-4, atol=2e-5)
    ident = torch.tensor([0.0, 1.0, 1.0, 0.0], device="cuda").repeat(1, 17, 1)
    close(dec(ident, dev(fx["tpose_lens"])), fx["tpose"], atol=1e-7)
    # strided C-ABI form the engine uses: 5 channels per joint (4-D rotation + score embedding), gradient leaves channel 4 alone
    wide = torch.zeros(B * L, 17, 5, device="cuda")
    wide[..., :4] = rot.detach()
    out = torch.empty(B, 1, L, 17, 3, device="cuda")
    _lib.check(lib.mp_fk_decode_fwd(wide.data_ptr(), 5, 4, bl.detach().reshape(B, 16).contiguous().data_ptr(), out.data_ptr(), B, 1, L, st()))
    close(out.view(B * L, 17, 3), fx["poses"], rtol=1e-5, atol=2e-6)
    assert lib.mp_fk_decode_fwd(wide.data_ptr(), 5, 5, bl.data_ptr(), out.data_ptr(), B, 1, L, st()) != 0      # only 4 and 6 exist


def test_rot4_models_vs_reference(lib):
    from manipose_amd.metrics import manifold_training_loss, rmcl_training_loss
    fx = load_fixture("rmcl_tiny_rot4")
    model = _build(fx).eval()
    assert model.rotations_module.head[0].prediction_head.weight.shape[0] == 5
    poses, scores = model(dev(fx["X"]))
    close(poses, fx["poses"], rtol=1e-4, atol=2e-5)
    close(scores, fx["scores"], rtol=1e-4, atol=1e-6)
    total, terms = rmcl_training_loss(poses, scores, dev(fx["y"]))
    np.testing.assert_allclose([terms[k].item() for k in ("wloss", "score_reg", "vloss", "sreg")], fx["loss_terms"], rtol=1e-4)
    total.backward()
    _check_grads(model, fx)
    fx = load_fixture("manifold_k1_rot4")
    model = _build(fx).eval()
    pred = model(dev(fx["X"]))
    close(pred, fx["poses"], rtol=1e-4, atol=2e-5)
    total, _ = manifold_training_loss(pred, dev(fx["y"]))
    np.testing.assert_allclose(total.item(), float(fx["loss_total"]), rtol=1e-4)
    total.backward()
    _check_grads(model, fx)


def test_rot4_bf16_engine_and_training_step(lib):
    """The 4-D variant on the bf16 engine through the fused trainer: finite loss that decreases over a few Adam steps."""
    from manipose_amd.training import LiftingTrainer
    fx = load_fixture("rmcl_tiny_rot4")
    model = _build(fx)
    model.precision = "bf16"
    model._engine = None
    tr = LiftingTrainer(model, lr=2e-3, sq_loss=True)
    X, y = dev(fx["X"]), dev(fx["y"])
    first = tr.train_step(X, y).sum().item()
    for _ in range(8):
        last = tr.train_step(X, y).sum().item()
    assert np.isfinite(first) and np.isfinite(last) and last < first


@pytest.mark.parametrize("precision", ["fp32", "bf16", "bf16x3"])
def test_config5_T81_K5_eval_mpjpe_pck_auc_vs_oracle(lib, precision):
    """BASELINE config #5 shape (MPI-INF-3DHP lifting: T=81, K=5, full width) through the evaluation path of the entry points
    (flip test-time augmentation batched into one forward, weighted-average / best-score / oracle aggregation, MPJPE in mm,
    3DPCK@150 mm / AUC, P-MPJPE) against the CPU oracle composing the same procedure (eval_utils.py:16-223, pck.py:92-199) on
    identical synthetic batches."""
    import os, sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "hpe"))
    from _entry import evaluate
    from manipose_amd import RMCLManifoldMixSTE, h36m_skeleton
    cfg = dict(orc.FULL_CFG, T=81)
    st_ = orc.make_state(cfg, seed=5)
    model = RMCLManifoldMixSTE(h36m_skeleton(), num_frame=81, drop_path_rate=0.0)
    model.load_state_dict(st_, strict=True)
    model.precision = precision
    model = model.cuda().eval()
    X, y = orc.synthetic_batch(2, 81, seed=7)
    y = 0.25 * y                                                   # errors around the 150 mm threshold, so PCK / AUC are informative
    res = evaluate(model, X.cuda(), y.cuda(), batch=2, tta=True, analytics=True)
    with torch.no_grad():
        ocfg = orc.oracle_cfg(cfg)
        p0, s0 = orc.rmcl_manifold_forward(X, st_, ocfg)
        p1, s1 = orc.rmcl_manifold_forward(orc.flip_pose(X), st_, ocfg)
        p1 = orc.flip_pose(p1)
        agg = (orc.aggregate(p0, s0, "weighted_ave") + orc.aggregate(p1, s1, "weighted_ave")) / 2
        best = (orc.aggregate(p0, s0, "best_score") + orc.aggregate(p1, s1, "best_score")) / 2
        orac = (orc.aggregate(p0, mode="oracle", ground_truth=y)[1] + orc.aggregate(p1, mode="oracle", ground_truth=y)[1]) / 2
        want = {"mpjpe": 1000 * orc.mpjpe_error(agg, y).item(), "ps_oracle_mpjpe": 1000 * orc.mpjpe_error(best, y).item(),
                "oracle_mpjpe": 1000 * orc.mpjpe_error(orac, y).item()}
        pck, auc = orc.keypoint_3d_pck_auc(1000 * agg.reshape(-1, 17, 3), 1000 * y.reshape(-1, 17, 3))
        pmp = 1000 * orc.p_mpjpe(agg.reshape(-1, 17, 3), y.reshape(-1, 17, 3)).item()
    tol_mm = 0.1 if precision != "bf16" else 10.0                   # north star: 0.1 mm (fp32 and the split precision); bf16: the documented drift bound
    for k, v in want.items():
        assert abs(res[k] - v) <= tol_mm, (k, res[k], v)
    a = res["analytics"]
    assert abs(a["mpjpe"] - want["mpjpe"]) <= tol_mm and abs(a["p_mpjpe"] - pmp) <= tol_mm
    tol_pct = 0.2 if precision != "bf16" else 5.0
    assert abs(a["pck"] - pck.item()) <= tol_pct and abs(a["auc"] - auc.item()) <= tol_pct, (a["pck"], pck.item(), a["auc"], auc.item())
    assert 1.0 < a["pck"] < 99.0
    print(f"T=81 K=5 {precision}: MPJPE {res['mpjpe']:.3f} mm (oracle {want['mpjpe']:.3f}), PCK {a['pck']:.2f} ({pck.item():.2f}), AUC {a['auc']:.2f} ({auc.item():.2f})")


# ---------------------------------------------------------------------------------------------------------------------------------
# model.arch=mixste: the bare MixSTE regressor of the reference's entry points (main_h36m_lifting.py:617-628) through the engine
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_bare_mixste_model_vs_reference(lib, precision):
    from manipose_amd import MixSTE
    from manipose_amd.metrics import manifold_training_loss, mpjpe_error
    fx = load_fixture("mixste_tiny")
    T, C, depth, heads = [int(v) for v in fx["cfg_mixste"]]
    model = MixSTE(num_frame=T, num_joints=17, in_chans=2, out_dim=3, embed_dim=C, depth=depth, num_heads=heads, drop_path_rate=0.0)
    assert sorted(model.state_dict().keys()) == sorted(k[3:] for k in fx if k.startswith("w::"))      # the reference's state-dict keys
    model.load_state_dict(fixture_state(fx), strict=True)
    model.precision = precision
    model = model.cuda().eval()
    pred = model(dev(fx["X"]))
    assert pred.shape == fx["poses"].shape
    total, terms = manifold_training_loss(pred, dev(fx["y"]))
    total.backward()
    if precision == "fp32":
        assert mpjpe_error(pred, dev(fx["poses"]), "average").item() <= MPJPE_TOL_M
        close(pred, fx["poses"], rtol=1e-4, atol=2e-5)
        np.testing.assert_allclose([terms[k].item() for k in ("wloss", "vloss", "sreg")], fx["loss_terms"], rtol=1e-4)
        _check_grads(model, fx)
    else:
        assert mpjpe_error(pred, dev(fx["poses"]), "average").item() <= 3e-2          # un-normalised regression output: bf16 operand rounding
        np.testing.assert_allclose(total.item(), float(fx["loss_total"]), rtol=3e-2)
    with pytest.raises(RuntimeError):
        model.STEblocks[0](pred)                          # blocks stay parameter containers


def test_bare_mixste_entry_point_trains(lib, tmp_path, monkeypatch, capsys):
    import os, sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "hpe"))
    from _entry import run
    monkeypatch.chdir(tmp_path)
    best = run(["model.arch=mixste", "train.epochs=1", "train.steps_per_epoch=2", "train.batch_size=4", "train.batch_size_test=2",
                "data.seq_len=27", "model.channels=64", "model.layers=2", "model.nheads=4", "data.synthetic_sequences=6", "run.test=true",
                "train.mpjpe_epoch_interval=1"])
    out = capsys.readouterr().out
    assert np.isfinite(best) and "epoch 0:" in out and "test [synthetic]:" in out and "mpjpe" in out


def test_rigid_segments_term_kernel_and_training_step_vs_reference(lib):
    """train.rigid_seg_reg (make_loss :170-177): the fused variance-of-bone-length kernel (value + gradient) against the reference's
    segments_time_consistency autograd, through the reference-named function, the C ABI's accumulate-into-d_poses form, and one trainer
    step of the bare MixSTE whose parameter gradients must equal those of the reference's 4-term total."""
    from manipose_amd import MixSTE, _lib, h36m_skeleton
    from manipose_amd.metrics.regularizations import segments_time_consistency
    from manipose_amd.training import LiftingTrainer
    fx = load_fixture("mixste_tiny")
    T, C, depth, heads = [int(v) for v in fx["cfg_mixste"]]
    pred = dev(fx["poses"]).requires_grad_(True)
    r = 0.7 * segments_time_consistency(pred.permute(0, 3, 2, 1), h36m_skeleton(), mode="sum")
    r.backward()
    np.testing.assert_allclose(r.item(), float(fx["rigid_term"]), rtol=2e-5)
    close(pred.grad, fx["rigid_g_pred"], rtol=2e-4, atol=1e-7)
    # non-differentiable (analytics) path of the same function agrees
    np.testing.assert_allclose(0.7 * segments_time_consistency(pred.detach().permute(0, 3, 2, 1), h36m_skeleton(), mode="sum").item(),
                               float(fx["rigid_term"]), rtol=1e-4)
    model = MixSTE(num_frame=T, num_joints=17, in_chans=2, out_dim=3, embed_dim=C, depth=depth, num_heads=heads, drop_path_rate=0.0)
    model.load_state_dict(fixture_state(fx), strict=True)
    model = model.cuda().eval()
    tr = LiftingTrainer(model, lr=0.0, weight_decay=0.0, rigid_seg_reg=0.7)
    terms = tr.train_step(dev(fx["X"]), dev(fx["y"]))
    np.testing.assert_allclose(terms.sum().item(), float(fx["rigid_total"]), rtol=1e-4)
    np.testing.assert_allclose(terms[3].item(), float(fx["rigid_term"]), rtol=1e-4)
    flat = tr.flat_grads
    for (name, off, n) in model.flat_layout():
        want = fx["g_rigid::" + name].reshape(-1)
        got = flat[off:off + n].cpu().numpy()
        scale = np.abs(want).max() + 1e-12
        np.testing.assert_allclose(got, want, rtol=2e-3, atol=2e-6 + 1e-4 * scale, err_msg=name)
    with pytest.raises(NotImplementedError):
        LiftingTrainer(_build(load_fixture("rmcl_tiny")), rigid_seg_reg=0.1)


def test_caller_facing_helpers_of_the_rmcl_model(lib):
    """concat_hyp_and_scores / poses_from_hyp_idx (rmcl_manifold_mix_ste.py:108-139, used by eval_utils.py) and the single-term loss
    functions the reference's make_loss calls, on the fixture's outputs."""
    from manipose_amd import metrics as M
    from manipose_amd.data.skeleton import assert_h36m
    fx = load_fixture("rmcl_tiny")
    model = _build(fx).eval()
    poses, scores = dev(fx["poses"]), dev(fx["scores"])
    B, K, T = poses.shape[:3]
    cat = model.concat_hyp_and_scores(poses, scores)
    assert cat.shape == (B, K, T, 17, 4) and torch.equal(cat[..., :3], poses) and torch.equal(cat[..., 3], scores.expand(B, K, T, 17))
    idx = torch.from_numpy(fx["wta_idx"]).cuda()
    picked = model.poses_from_hyp_idx(poses, idx)
    want = orc.poses_from_hyp_idx(torch.from_numpy(fx["poses"]), torch.from_numpy(fx["wta_idx"]))
    assert torch.equal(picked.cpu(), want)
    w = M.STANDARD_H36M_WEIGHTS
    close(M.weighted_mpjpe_loss(poses[:, 0], dev(fx["y"]), weights=w), orc.weighted_mpjpe_loss(torch.from_numpy(fx["poses"][:, 0]), torch.from_numpy(fx["y"]), w), rtol=1e-5)
    assert_h36m(model.decoder.skeleton)
    from manipose_amd.data import Skeleton, T_POSE_OPERATORS
    with pytest.raises(AssertionError):
        assert_h36m(Skeleton([-1, 0, 1, 2, 0, 4, 5, 0, 7, 8, 9, 8, 11, 12, 8, 14, 14], [4, 5, 6, 11, 12, 13], [1, 2, 3, 14, 15, 16], T_POSE_OPERATORS))


# --------------------------------------------------------------------------------------------- bf16x3: split precision (parity at matrix-core speed)
def _split(t):
    hi = t.bfloat16()
    lo = (t - hi.float()).bfloat16()
    return hi, lo


def _join(hi, lo):
    return hi.float() + lo.float()


@pytest.mark.parametrize("M,N,K", [(300, 96, 64), (1027, 512, 512), (4131, 1536, 512), (777, 512, 1024), (66100, 512, 512), (520, 128, 128),
                                   (64, 32, 32)])
def test_bf16x3_linear_forward_epilogues(lib, M, N, K):
    """Split-precision Linear forward (planar hi/lo bf16 operands, three MFMA products per k-tile; persistent, 256- and 128-tile
    kernels) against an fp64 product of the fp32 operands: 2^-16 operand precision instead of bf16's 2^-9."""
    from manipose_amd import _lib
    g = torch.Generator().manual_seed(M + N + K)
    x = torch.randn(M, K, generator=g)
    W = torch.randn(N, K, generator=g) / K ** 0.5
    b = torch.randn(N, generator=g)
    r = torch.randn(M, N, generator=g)
    xd, Wd = x.cuda(), W.cuda()
    xh, xl, Wh, Wl = (torch.empty(t.shape, device="cuda", dtype=torch.bfloat16) for t in (x, x, W, W))
    _lib.check(lib.mp_split_bf16(xd.data_ptr(), xh.data_ptr(), xl.data_ptr(), xd.numel(), st()))
    _lib.check(lib.mp_split_bf16(Wd.data_ptr(), Wh.data_ptr(), Wl.data_ptr(), Wd.numel(), st()))
    eh, el = _split(x)
    assert torch.equal(xh.cpu(), eh) and torch.equal(xl.cpu(), el)          # hi = bf16(x), lo = bf16(x - hi), bit for bit
    bd, rd = b.cuda(), r.cuda()
    pre = (x.double() @ W.double().t() + b.double())
    scale = float(pre.abs().max())
    yh, yl = torch.empty(M, N, device="cuda", dtype=torch.bfloat16), torch.empty(M, N, device="cuda", dtype=torch.bfloat16)
    _lib.check(lib.mp_linear_fwd_bf16x3(xh.data_ptr(), xl.data_ptr(), Wh.data_ptr(), Wl.data_ptr(), bd.data_ptr(), yh.data_ptr(), yl.data_ptr(),
                                        None, None, M, N, K, 0, st()))
    err = (_join(yh, yl).cpu().double() - pre).abs().max().item() / scale
    assert err < 4e-5, err                                                     # bf16 operands: ~4e-3
    z = torch.empty(M, N, device="cuda", dtype=torch.bfloat16)
    _lib.check(lib.mp_linear_fwd_bf16x3(xh.data_ptr(), xl.data_ptr(), Wh.data_ptr(), Wl.data_ptr(), bd.data_ptr(), yh.data_ptr(), yl.data_ptr(),
                                        z.data_ptr(), None, M, N, K, 1, st()))
    want = torch.nn.functional.gelu(pre)
    assert (_join(yh, yl).cpu().double() - want).abs().max().item() / scale < 4e-5
    pf = pre.float().requires_grad_(True)
    torch.nn.functional.gelu(pf).sum().backward()
    close(z.float(), pf.grad, rtol=1e-2, atol=1e-2)                          # gelu' is kept as plain bf16 (the backward is bf16)
    y32 = torch.empty(M, N, device="cuda")
    _lib.check(lib.mp_linear_fwd_bf16x3(xh.data_ptr(), xl.data_ptr(), Wh.data_ptr(), Wl.data_ptr(), bd.data_ptr(), y32.data_ptr(), None,
                                        None, rd.data_ptr(), M, N, K, 2, st()))
    assert (y32.cpu().double() - (pre + r.double())).abs().max().item() / scale < 4e-5


@pytest.mark.parametrize("M,N,K,wgs", [(300, 256, 128, 0), (1027, 768, 192, 8), (2049, 768, 320, 8), (777, 512, 1024, 0), (5000, 1536, 512, 16), (4131, 256, 128, 8)])
def test_bf16x3_persistent_loop_shapes(lib, M, N, K, wgs):
    """The persistent split-precision kernel's hand-scheduled loop (csrc/gemm_bf16.hip, kpipe_x3: k-tiles 0 .. nk-2 of a tile in one
    pipelined asm block, the last k-tile block by block) forced on at small sizes: two k-tiles (one pass of the loop), odd k-tile counts, 16
    k-tiles, one tile per workgroup (no next tile to prefetch) and several (few workgroups: the next tile's first k-tile is fetched during
    the last), ragged last row panel; all three epilogues against the fp64 product and against the tiled kernels."""
    from manipose_amd import _lib
    g = torch.Generator().manual_seed(M + N + K)
    x = torch.randn(M, K, generator=g)
    W = torch.randn(N, K, generator=g) / K ** 0.5
    b, r = torch.randn(N, generator=g), torch.randn(M, N, generator=g)
    xd, Wd, bd, rd = x.cuda(), W.cuda(), b.cuda(), r.cuda()
    xh, xl, Wh, Wl = (torch.empty(t.shape, device="cuda", dtype=torch.bfloat16) for t in (x, x, W, W))
    _lib.check(lib.mp_split_bf16(xd.data_ptr(), xh.data_ptr(), xl.data_ptr(), xd.numel(), st()))
    _lib.check(lib.mp_split_bf16(Wd.data_ptr(), Wh.data_ptr(), Wl.data_ptr(), Wd.numel(), st()))
    pre = x.double() @ W.double().t() + b.double()
    scale = float(pre.abs().max())
    res = {}
    for min_tiles in (1, 1 << 30):                   # persistent kernel forced / tiled kernels only
        _lib.check(lib.mp_set_option(b"gemm_persist_min_tiles", min_tiles))
        if wgs: _lib.check(lib.mp_set_option(b"gemm_persist_wgs", wgs))
        try:
            yh, yl = torch.full((M, N), float("nan"), device="cuda").bfloat16(), torch.full((M, N), float("nan"), device="cuda").bfloat16()
            _lib.check(lib.mp_linear_fwd_bf16x3(xh.data_ptr(), xl.data_ptr(), Wh.data_ptr(), Wl.data_ptr(), bd.data_ptr(), yh.data_ptr(), yl.data_ptr(),
                                                None, None, M, N, K, 0, st()))
            zh, zl, z = torch.empty_like(yh), torch.empty_like(yh), torch.empty_like(yh)
            _lib.check(lib.mp_linear_fwd_bf16x3(xh.data_ptr(), xl.data_ptr(), Wh.data_ptr(), Wl.data_ptr(), bd.data_ptr(), zh.data_ptr(), zl.data_ptr(),
                                                z.data_ptr(), None, M, N, K, 1, st()))
            y32 = torch.full((M, N), float("nan"), device="cuda")
            _lib.check(lib.mp_linear_fwd_bf16x3(xh.data_ptr(), xl.data_ptr(), Wh.data_ptr(), Wl.data_ptr(), bd.data_ptr(), y32.data_ptr(), None,
                                                None, rd.data_ptr(), M, N, K, 2, st()))
            torch.cuda.synchronize()
        finally:
            _lib.check(lib.mp_set_option(b"gemm_persist_min_tiles", 0))
            if wgs: _lib.check(lib.mp_set_option(b"gemm_persist_wgs", 0))
        assert (_join(yh, yl).cpu().double() - pre).abs().max().item() / scale < 4e-5, min_tiles
        assert (_join(zh, zl).cpu().double() - torch.nn.functional.gelu(pre)).abs().max().item() / scale < 4e-5, min_tiles
        assert (y32.cpu().double() - (pre + r.double())).abs().max().item() / scale < 4e-5, min_tiles
        res[min_tiles] = (yh.cpu(), yl.cpu(), zh.cpu(), zl.cpu(), z.cpu(), y32.cpu())
    p_, t_ = res[1], res[1 << 30]                    # (the 128-tile kernel sums in another order: agreement, not identity)
    assert (_join(p_[0], p_[1]) - _join(t_[0], t_[1])).abs().max().item() <= 2e-5 * scale
    assert (_join(p_[2], p_[3]) - _join(t_[2], t_[3])).abs().max().item() <= 2e-5 * scale
    assert (p_[5] - t_[5]).abs().max().item() <= 2e-5 * scale


def f16f8_planes(v, weight):
    """The "f16f8" operand format of include/manipose_hip.h (mp_linear_fwd_f16f8), built on the host: fp16 hi plane + the 8-bit correction
    plane (per four reduction indices: 4 e4m3 bytes | 4 e4m3 bytes).  Returns (hi, correction bytes, first half, second half)."""
    R, K = v.shape
    hi = v.half()
    lo = v - hi.float()
    f8 = lambda t: t.clamp(-448, 448).to(torch.float8_e4m3fn)
    first, second = (f8(hi.float() * 16), f8(lo * 2.0 ** 15)) if weight else (f8(lo * 2.0 ** 11), f8(hi.float()))
    cat = torch.stack([first.view(torch.uint8).view(R, K // 4, 4), second.view(torch.uint8).view(R, K // 4, 4)], dim=2).reshape(R, 2 * K)
    return hi.contiguous(), cat.contiguous(), first.double(), second.double()


@pytest.mark.gpu
@pytest.mark.parametrize("M,N,K", [(300, 256, 128), (1027, 512, 512), (4131, 1536, 512), (777, 512, 1024), (66100, 512, 512)])
def test_f16f8_linear_forward(lib, M, N, K):
    """Linear forward on fp16 hi planes + block-scaled fp8 correction planes (one fp16 and one 128-deep fp8 matrix-core product per 64
    reduction indices): (a) the kernel evaluates exactly the products of the rounded planes it is given (fp64 of the same
    planes, to fp32 accumulation error); (b) against the fp64 product of the fp32 operands it keeps ~2^-15 of the operand precision -
    a lone fp16 product: 2^-11."""
    from manipose_amd import _lib
    g = torch.Generator().manual_seed(M + N + K)
    x = torch.randn(M, K, generator=g)
    W = torch.randn(N, K, generator=g) / K ** 0.5
    b = torch.randn(N, generator=g)
    x16, x8, x_lo8, x_hi8 = f16f8_planes(x, False)
    W16, W8, W_hi8, W_lo8 = f16f8_planes(W, True)
    planes = x16.double() @ W16.double().t() + 2.0 ** -15 * (x_lo8 @ W_hi8.t() + x_hi8 @ W_lo8.t()) + b.double()
    pre = x.double() @ W.double().t() + b.double()
    scale = float(pre.abs().max())
    dx16, dx8, dW16, dW8, bd = x16.cuda(), x8.cuda(), W16.cuda(), W8.cuda(), b.cuda()
    y = torch.empty(M, N, device="cuda")
    _lib.check(lib.mp_linear_fwd_f16f8(dx16.data_ptr(), dx8.data_ptr(), dW16.data_ptr(), dW8.data_ptr(), bd.data_ptr(), y.data_ptr(), M, N, K, st()))
    got = y.cpu().double()
    assert (got - planes).abs().max().item() / scale < 2e-6, (got - planes).abs().max().item() / scale
    err = (got - pre).abs().max().item() / scale
    lone = (x16.double() @ W16.double().t() + b.double() - pre).abs().max().item() / scale
    print(f"f16f8 M={M} N={N} K={K}: max error / max |y| {err:.2e} (lone fp16 product {lone:.2e})")
    assert err < 4e-5 and err < lone / 8, (err, lone)
    with pytest.raises(RuntimeError):
        _lib.check(lib.mp_linear_fwd_f16f8(dx16.data_ptr(), dx8.data_ptr(), dW16.data_ptr(), dW8.data_ptr(), bd.data_ptr(), y.data_ptr(), M, N - 4, K, st()))
    # the device-side splitter writes the same planes, bit for bit (fp16 and e4m3 round to nearest even; +-448 clamp)
    for v, weight, want16, want8 in ((x, 0, x16, x8), (W, 1, W16, W8)):
        big = v.clone()
        big[0, :4] = torch.tensor([1000.0, -1000.0, 447.0, 3e-5]) * (1.0 if not weight else 1 / 16)       # clamp and subnormal cases
        b16, b8, _, _ = f16f8_planes(big, bool(weight))
        src = big.cuda()
        o16 = torch.empty(v.shape, device="cuda", dtype=torch.float16)
        o8 = torch.empty(v.shape[0], 2 * v.shape[1], device="cuda", dtype=torch.uint8)
        _lib.check(lib.mp_split_f16f8(src.data_ptr(), o16.data_ptr(), o8.data_ptr(), src.numel(), weight, st()))
        assert torch.equal(o16.cpu(), b16)
        assert torch.equal(o8.cpu(), b8), (o8.cpu() != b8).sum().item()


def _f16f8_model(state, kw, f16f8, f16_backward, train=False):
    from manipose_amd import RMCLManifoldMixSTE
    model = RMCLManifoldMixSTE(**kw)
    model.load_state_dict(state, strict=True)
    model.precision, model.f16f8, model.f16_backward = "bf16x3", f16f8, f16_backward
    model = model.cuda()
    return model.train() if train else model.eval()


def _grad_agreement(model, ref_grads):
    """worst cosine / largest relative norm deviation of the model's parameter gradients against a dict of reference gradients"""
    cos = min(torch.nn.functional.cosine_similarity(p.grad.cpu().reshape(-1).double(), ref_grads[k].reshape(-1).double(), dim=0).item()
              for k, p in model.named_parameters())
    dev = max(abs((p.grad.cpu().norm() / ref_grads[k].norm()).item() - 1.0) for k, p in model.named_parameters())
    return cos, dev


@pytest.mark.gpu
def test_f16f8_inputs_of_the_model_and_the_inference_flag(lib):
    """mp_model_config::f16f8 / f16_backward (ABI v7; per model, no process-wide state): the qkv / fc1 (level 2: fc2 too) Linear layers of a
    rotations net whose width is a multiple of 256 read "f16f8" operands, optionally with their backward on saturating scaled-fp16 operands.
    (a) every form stays inside the 1e-4 m bound of the CPU oracle and the forms differ (the fields really switch kernels), two models of
    different forms coexist in one process; (b) a forward under torch.no_grad() tells the engine that no backward follows (train bit 1) and
    gives the same bits; mp_model_backward refuses to run after it; (c) the fp16 backward's gradients have the oracle's direction and norm
    for losses scaled by 1e6, 1 and 1e-6 (measured: worst cosine 0.999994, norm within 4e-4; asserted with that margin, not two orders
    above it), nothing saturates (mp_model_grad_health); (d) invalid combinations are refused."""
    from manipose_amd import h36m_skeleton, _lib
    from manipose_amd.architectures.engine import LiftEngine
    T, C, H, K, B = 27, 256, 4, 3, 2
    cfg = dict(T=T, J=17, num_bones=16, C_rot=C, depth_rot=3, heads_rot=H, C_seg=32, depth_seg=1, heads_seg=4, n_hyp=K)
    state = orc.make_state(cfg, seed=11)
    X, y = orc.synthetic_batch(B, T, seed=12)
    with torch.no_grad():
        want, _ = orc.rmcl_manifold_forward(X, state, orc.oracle_cfg(cfg))
    kw = dict(skeleton=h36m_skeleton(), num_frame=T, embed_dim_rot=C, depth_rot=3, num_heads_rot=H, embed_dim_seg=32, depth_seg=1,
              num_heads_seg=4, drop_path_rate=0.0, n_hyp=K)
    req = {k: v.clone().requires_grad_(True) for k, v in state.items()}
    op, osc = orc.rmcl_manifold_forward(X, req, orc.oracle_cfg(cfg))
    (op.square().sum() + osc.square().sum()).backward()
    ref = {k: v.grad for k, v in req.items()}
    outs, models = {}, {}
    for form in ((0, False), (1, False), (1, True), (2, True), (3, False)):
        model = models[form] = _f16f8_model(state, kw, *form)       # all four stay alive: the forms are per-model state
        poses, scores = model(X.cuda())
        err = (poses.cpu() - want).norm(dim=-1).mean().item()
        print(f"f16f8={form[0]} f16_backward={form[1]}: MPJPE vs oracle {err:.2e} m")
        assert err <= 1e-4
        outs[form] = poses.detach().clone()
        with torch.no_grad():
            p2, s2 = model(X.cuda())
        assert torch.equal(p2, poses.detach()) and torch.equal(s2, scores.detach())
        g = torch.zeros_like(model._flat)
        rc = lib.mp_model_backward(model._engine.handle, _lib.ptr(model._flat), _lib.ptr(g), _lib.ptr(torch.zeros_like(p2)), None, _lib.stream_ptr())
        assert rc != 0                                     # the last forward announced that no backward follows
        for factor in (1e6, 1e-6, 1.0):
            model.zero_grad(set_to_none=True)
            pf, sf = model(X.cuda())
            (factor * (pf.square().sum() + sf.square().sum())).backward()
            cos, dev = _grad_agreement(model, {k: factor * v for k, v in ref.items()})
            health = model._engine.grad_health()
            print(f"  loss x {factor:g}: worst gradient cosine {cos:.6f}, largest norm deviation {dev:.1e}, health {health}")
            assert cos > 0.9999 and dev < 2e-3, (form, factor, cos, dev)
            assert health["saturated"] == 0 and health["non_finite"] == 0
            assert (health["scale"] > 0) == form[1]        # a scale exists exactly for the fp16-backward models
    assert torch.equal(outs[(1, False)], outs[(1, True)])                          # the backward's form does not touch the forward
    assert not torch.equal(outs[(0, False)], outs[(1, False)]) and not torch.equal(outs[(1, True)], outs[(2, True)])
    assert not torch.equal(outs[(3, False)], outs[(1, False)]) and not torch.equal(outs[(3, False)], outs[(2, True)])      # proj reads f16f8 operands too
    p_again, _ = models[(0, False)](X.cuda())                                      # ... and the first model still computes what it computed
    assert torch.equal(p_again.detach(), outs[(0, False)])
    base = dict(arch="rmcl_manifold", num_frame=T, num_joints=17, num_bones=16, embed_dim_rot=C, depth_rot=3, num_heads_rot=H, embed_dim_seg=32,
                depth_seg=1, num_heads_seg=4, n_hyp=K, drop_path_rate=0.0, max_batch=0)
    for bad in (dict(precision="bf16", f16f8=1), dict(precision="bf16x3", f16f8=0, f16_backward=True), dict(precision="bf16x3", f16f8=2, f16_backward=False),
                dict(precision="bf16x3", f16f8=3, f16_backward=True), dict(precision="bf16x3", f16f8=4)):
        with pytest.raises(RuntimeError):
            LiftEngine(**base, **bad)


@pytest.mark.gpu
def test_fp16_backward_gradient_window_at_full_width_and_after_training(lib):
    """Where the scaled-fp16 gradient operands of an f16_backward model sit in fp16's range (round-3 review: "nothing measures where the
    internal gradients sit relative to that window", all evidence at random-init weights).  Full width (C = 512, depth 8, 8 heads), T = 27:
    after the backward the engine's scratch still holds dz and dqkv of the LAST block it differentiated
    (STE0, the far end of the chain from where S was chosen: mp_model_peek 500 / 501).  Asserted at random init, after 200 optimisation steps
    with the reference's Adam settings at a 5x learning rate (weights that have really moved), and on a muP model:
    no store saturated or met a non-finite value, the largest stored magnitude leaves >= 2^4 of headroom; of the TRUE non-zero values of each
    operand (the same buffers of the bf16 backward of the same weights, which has fp32's exponent range) fewer than 2 % fall into
    fp16's subnormal range and fewer than 0.1 % flush to zero at the chosen S; and the parameter gradients are as close to the fp32 engine's
    (same weights) as those of the bf16 backward are."""
    from manipose_amd import RMCLManifoldMixSTE, h36m_skeleton
    from manipose_amd.training import LiftingTrainer
    T, B = 27, 8
    sk = h36m_skeleton()

    def window(model, tag, truth):
        """truth: the same three operands of the bf16 backward of the same weights (bf16 has fp32's exponent range: what is really there)"""
        eng = model._engine
        h = eng.grad_health()
        rep = {}
        for code, name in ((500, "dz"), (501, "dqkv")):
            v = eng.peek(code).view(torch.float16).float().abs()
            t = truth[name] * h["scale"]                # where the true values WOULD sit in the fp16 window
            nzt = t[t > 0]
            lost = ((nzt < 2.0 ** -24).float().mean().item() if nzt.numel() else 0.0, (nzt < 2.0 ** -14).float().mean().item() if nzt.numel() else 0.0)
            rep[name] = (v.max().item(), t.max().item(), lost[1], lost[0])
            assert torch.isfinite(v).all()
            assert v.max().item() <= 65504.0 / 16, (tag, name, v.max().item())
            # of the operand's TRUE non-zero values: fewer than 2 % may land in fp16's subnormal range, fewer than 0.1 % may flush to zero
            assert lost[1] < 0.02 and lost[0] < 0.001, (tag, name, rep[name])
        print(f"[fp16 window] {tag}: S = 2^{int(np.log2(h['scale']))}, " + "; ".join(f"{n}: amax {a:.3g} (true x S {b:.3g}), subnormal {u:.3%}, flushed {z:.3%}"
                                                                                       for n, (a, b, u, z) in rep.items()))
        assert h["saturated"] == 0 and h["non_finite"] == 0, (tag, h)

    def true_operands(model):
        return {name: model._engine.peek(code).view(torch.bfloat16).float().abs() for code, name in ((500, "dz"), (501, "dqkv"))}

    def one_backward(model, X, y):
        from manipose_amd.metrics import rmcl_training_loss
        model.zero_grad(set_to_none=True)
        p, s = model(X)
        total, _ = rmcl_training_loss(p, s, y)
        total.backward()
        return {k: q.grad.detach().cpu().clone() for k, q in model.named_parameters()}

    for mup in (False, True):
        torch.manual_seed(7)
        kw = dict(skeleton=sk, num_frame=T, n_hyp=5, drop_path_rate=0.0, mup=mup)
        m16 = RMCLManifoldMixSTE(**kw)
        if mup:                                   # base shapes as hpe/_entry.py derives them (widths 64 -> base, 128 -> delta), then the muP re-initialisation
            from manipose_amd.mup_lite import make_base_shapes, mu_init_params, set_base_shapes
            shapes = make_base_shapes(RMCLManifoldMixSTE(**dict(kw, embed_dim_rot=64, embed_dim_seg=64)),
                                      RMCLManifoldMixSTE(**dict(kw, embed_dim_rot=128, embed_dim_seg=128)))
            set_base_shapes(m16, shapes)
            mu_init_params(m16)
        lvl = 1 if mup else 2                 # level 2 (fc2 as well: the residual-gradient copy is fp16 too) needs a residual scale of 1
        m16.precision, m16.f16f8, m16.f16_backward = "bf16x3", lvl, True
        m16 = m16.cuda().train()
        g = torch.Generator(device="cuda").manual_seed(3)
        X = (0.3 * torch.randn(B, T, 17, 2, device="cuda", generator=g)).clamp(-1, 1)
        y = 0.3 * torch.randn(B, T, 17, 3, device="cuda", generator=g)
        y[:, :, 0] = 0
        stages = ("random init",) if mup else ("random init", "after 200 steps")
        for stage in stages:
            if stage != "random init":
                tr = LiftingTrainer(m16, lr=2e-4, weight_decay=1e-6, seed=1)
                first = last = None
                for i in range(200):
                    terms = tr.train_step(X, y)
                    if i == 0:
                        first = terms.sum().item()
                last = terms.sum().item()
                h = m16._engine.grad_health()
                print(f"[fp16 window] 200 steps: loss {first:.4f} -> {last:.4f}; last step's health {h}")
                assert last < first and h["saturated"] == 0 and h["non_finite"] == 0
            mb = RMCLManifoldMixSTE(**kw)
            if mup:
                set_base_shapes(mb, shapes, rescale_params=False)
            mb.load_state_dict(m16.state_dict(), strict=True)
            mb.precision, mb.f16f8, mb.f16_backward = "bf16x3", 1, False      # (level 1 + bf16 backward: the same forward for qkv / fc1; fc2's form differs at level 2)
            mb = mb.cuda().train()
            gb = one_backward(mb, X, y)
            truth = true_operands(mb)
            g16 = one_backward(m16, X, y)
            window(m16, ("muP, " if mup else "") + stage, truth)
            # both against the fp32 engine on the same weights: after training the batch loss sits near a minimum, the gradients are small
            # differences of large terms and ANY 8-11-bit backward loses digits - the fp16 backward must not lose more than the bf16 one
            m32 = RMCLManifoldMixSTE(**kw)
            if mup:
                set_base_shapes(m32, shapes, rescale_params=False)
            m32.load_state_dict(m16.state_dict(), strict=True)
            m32.precision = "fp32"
            m32 = m32.cuda().train()
            g32 = one_backward(m32, X, y)
            m32._engine = None
            del m32

            def worst_cos(g):
                return min(torch.nn.functional.cosine_similarity(g[k].reshape(-1).double(), g32[k].reshape(-1).double(), dim=0).item() for k in g
                           if g32[k].norm() > 0)
            c16, cb = worst_cos(g16), worst_cos(gb)
            print(f"[fp16 window] {'muP, ' if mup else ''}{stage}: worst parameter-gradient cosine against the fp32 engine: fp16 backward {c16:.6f}, bf16 backward {cb:.6f}")
            # At random init both backwards sit at 0.99999 (measured 0.999992 / 0.999989).  After the 200 steps the figure depends on WHERE the
            # trajectory ended: it moves with any reordering of fp32 sums in the backward (round 4 regrouped the LayerNorm backward's partial
            # sums: 0.9960 / 0.9922 on that trajectory, above 0.999 on the earlier one) - so the post-training claim is the relative one, the
            # fp16 backward loses no more than the bf16 backward does, with a floor well under both measurements
            assert c16 >= cb - 2e-4 and c16 > (0.9999 if stage == "random init" else 0.99), (stage, c16, cb)
            mb._engine = None
            del mb


@pytest.mark.gpu
def test_fp16_backward_saturates_instead_of_overflowing(lib):
    """Adversarial gradient scale (round-3 advice): the per-backward scale S is chosen from max(|d_poses|, |d_scores|) alone, so it can be
    wrong by orders of magnitude for the interior gradients.  (a) One d_poses element 1e4 x the rest under a SUMMED loss: S follows the
    outlier, the rest of the gradient sits 1e4 lower in the window - the parameter gradients must stay finite and keep the direction of the
    bf16 backward's.  (b) The converse: d_scores carries a huge value that contributes almost nothing to the interior (S is then far too
    SMALL for... no: too small a scale only loses precision); to force the OVERFLOW side the scale is pinned low by tiny d_poses while the
    score gradient - 2^40 larger after the score head's softmax - drives the interior: stores must clamp at +-65504 and be counted, no inf /
    NaN may reach the weight gradients."""
    from manipose_amd import h36m_skeleton, _lib
    T, C, H, K, B = 27, 256, 4, 3, 2
    cfg = dict(T=T, J=17, num_bones=16, C_rot=C, depth_rot=3, heads_rot=H, C_seg=32, depth_seg=1, heads_seg=4, n_hyp=K)
    state = orc.make_state(cfg, seed=21)
    X, _ = orc.synthetic_batch(B, T, seed=22)
    kw = dict(skeleton=h36m_skeleton(), num_frame=T, embed_dim_rot=C, depth_rot=3, num_heads_rot=H, embed_dim_seg=32, depth_seg=1,
              num_heads_seg=4, drop_path_rate=0.0, n_hyp=K)
    m16, mb = _f16f8_model(state, kw, 1, True), _f16f8_model(state, kw, 1, False)
    gen = torch.Generator(device="cuda").manual_seed(5)
    dp = torch.randn(B, K, T, 17, 3, device="cuda", generator=gen)
    dp[0, 1, 3, 5, 2] = 1e4 * dp.abs().max()                      # (a) one outlier joint sets S for the whole net
    ds = torch.randn(B, K, T, 1, device="cuda", generator=gen)
    grads = {}
    for tag, model in (("fp16", m16), ("bf16", mb)):
        model.zero_grad(set_to_none=True)
        p, s = model(X.cuda())
        torch.autograd.backward([p, s], [dp, ds])
        grads[tag] = {k: q.grad.detach().clone() for k, q in model.named_parameters()}
        assert all(torch.isfinite(v).all() for v in grads[tag].values()), tag
    h = m16._engine.grad_health()
    cos = min(torch.nn.functional.cosine_similarity(grads["fp16"][k].reshape(-1).double(), grads["bf16"][k].reshape(-1).double(), dim=0).item()
              for k in grads["fp16"] if grads["bf16"][k].norm() > 0)
    print(f"[adversarial] outlier x 1e4: S = {h['scale']:.3g}, saturated {h['saturated']}, non-finite {h['non_finite']}, worst cosine vs the bf16 backward {cos:.6f}")
    assert h["non_finite"] == 0 and cos > 0.999, (h, cos)
    # (b) overflow side: the loss gradient is tiny (S large), the interior is driven 1e9 harder through the score path
    dp2 = 1e-12 * torch.randn(B, K, T, 17, 3, device="cuda", generator=gen)
    ds2 = 1e-12 * torch.randn(B, K, T, 1, device="cuda", generator=gen)
    m16.zero_grad(set_to_none=True)
    p, s = m16(X.cuda())
    torch.autograd.backward([p, s], [dp2, ds2])
    h0 = m16._engine.grad_health()
    assert h0["saturated"] == 0                                   # a uniformly tiny gradient is what S is for
    with torch.no_grad():                                         # blow one score head up so that its logit gradient dwarfs the pose gradient
        for k, q in m16.named_parameters():
            if k.endswith("head.0.score_head.weight"):
                q.mul_(1e7)
    m16.zero_grad(set_to_none=True)
    p, s = m16(X.cuda())
    torch.autograd.backward([p, s], [dp2, 1e-12 * torch.ones_like(ds2)])
    h1 = m16._engine.grad_health()
    fin = all(torch.isfinite(q.grad).all() for q in m16.parameters())
    print(f"[adversarial] overflow side: S = {h1['scale']:.3g}, saturated {h1['saturated']}, non-finite {h1['non_finite']}, gradients finite: {fin}")
    assert fin, "an out-of-window interior gradient must clamp, never reach the weight gradients as inf / NaN"


@pytest.mark.parametrize("temporal,B,T,J,C,H", [(1, 2, 243, 3, 128, 2), (1, 1, 81, 17, 512, 8), (1, 2, 27, 16, 128, 8), (1, 1, 256, 2, 64, 1),
                                                (1, 1, 17, 2, 32, 2), (1, 1, 300, 2, 128, 2), (1, 1, 100, 2, 64, 4), (1, 3, 243, 17, 512, 8),
                                                (1, 2, 129, 5, 64, 1), (1, 40, 200, 3, 128, 2), (1, 1, 145, 2, 64, 1),
                                                (0, 1, 9, 17, 128, 2), (0, 2, 5, 17, 512, 8), (0, 1, 7, 16, 128, 8), (0, 1, 3, 17, 64, 4)])
def test_bf16x3_attention_forward(lib, temporal, B, T, J, C, H):
    """Split-precision attention forward (MFMA kernels with hi/lo images; fp32 route for the other shapes) against the fp32 formula
    on the fp32 q/k/v."""
    from manipose_amd import _lib
    g = torch.Generator().manual_seed(T * 13 + C)
    M = B * T * J
    qkv = torch.randn(M, 3 * C, generator=g)
    ref = _attn_ref(qkv, B, T, J, C, H, temporal)
    qd = qkv.cuda()
    qh, ql = torch.empty_like(qd, dtype=torch.bfloat16), torch.empty_like(qd, dtype=torch.bfloat16)
    _lib.check(lib.mp_split_bf16(qd.data_ptr(), qh.data_ptr(), ql.data_ptr(), qd.numel(), st()))
    oh, ol = torch.zeros(M, C, device="cuda", dtype=torch.bfloat16), torch.zeros(M, C, device="cuda", dtype=torch.bfloat16)
    lse = torch.zeros(B * J * H * T, device="cuda")
    scratch = torch.empty(4 * M * C, device="cuda")
    _lib.check(lib.mp_attention_fwd_bf16x3(qh.data_ptr(), ql.data_ptr(), oh.data_ptr(), ol.data_ptr(), lse.data_ptr(), scratch.data_ptr(),
                                           temporal, B, T, J, C, H, st()))
    err = (_join(oh, ol).cpu() - ref).abs().max().item() / float(ref.abs().max())
    assert err < 1e-4, err                                                     # bf16 kernels: ~1e-2
    if temporal and C // H == 64 and 128 < T <= 256:
        # this shape runs the two-phase kernel (K / V regions fetched by direct-to-LDS DMA, two strips per fragment read): the
        # one-strip-at-a-time kernel computes the same products in the same order: same log-sum-exp and hi plane bit for bit, lo plane up to
        # the contraction of (o * 1/sum - hi) into one fused multiply-add
        o2h, o2l, lse2 = torch.zeros_like(oh), torch.zeros_like(ol), torch.zeros_like(lse)
        _lib.check(lib.mp_set_option(b"attn_two_phase", 0))
        try:
            _lib.check(lib.mp_attention_fwd_bf16x3(qh.data_ptr(), ql.data_ptr(), o2h.data_ptr(), o2l.data_ptr(), lse2.data_ptr(), scratch.data_ptr(),
                                                   temporal, B, T, J, C, H, st()))
        finally:
            _lib.check(lib.mp_set_option(b"attn_two_phase", 1))
        assert torch.equal(oh, o2h) and torch.equal(lse, lse2)
        assert (_join(oh, ol) - _join(o2h, o2l)).abs().max().item() <= 1e-5 * float(ref.abs().max())      # one ulp of a lo plane


@pytest.mark.parametrize("name", ["rmcl_tiny", "rmcl_small"])
def test_bf16x3_model_meets_the_parity_bound_on_the_reference_fixtures(lib, name):
    """precision="bf16x3": forward within the north-star bound of the REFERENCE's outputs; loss within 1e-3; gradients (bf16 backward
    on the hi planes) aligned with the reference's."""
    from manipose_amd.metrics import mpjpe_error, rmcl_training_loss
    fx = load_fixture(name)
    model = _build(fx)
    model.precision = "bf16x3"
    model = model.eval()
    poses, scores = model(dev(fx["X"]))
    mp = mpjpe_error(poses, dev(fx["poses"]), "average").item()
    print(f"\n[bf16x3 drift] {name}: MPJPE vs fp32 reference = {mp * 1e3:.5f} mm")
    assert mp <= MPJPE_TOL_M
    close(scores, fx["scores"], rtol=1e-3, atol=1e-5)
    total, _ = rmcl_training_loss(poses, scores, dev(fx["y"]))
    assert abs(total.item() - float(fx["loss_total"])) <= 1e-3 * abs(float(fx["loss_total"]))
    total.backward()
    cs = {k: _cos(p.grad.cpu(), torch.from_numpy(fx["g::" + k])) for k, p in model.named_parameters()}
    worst = min(cs.items(), key=lambda kv: kv[1])
    print(f"[bf16x3 drift] {name}: worst gradient cosine {worst[1]:.5f} at {worst[0]}")
    assert worst[1] > 0.9995, worst            # measured 0.99998 - 0.99999 (bf16 backward on the hi planes)


@pytest.mark.parametrize("f16f8", [0, 3])
def test_bf16x3_full_size_model_meets_the_parity_bound(lib, f16f8):
    """BASELINE config #3 shape (T=243 K=5 C=512 depth 8) at B=1 and B=3 in the split precision against the fp32 CPU oracle:
    MPJPE <= 1e-4 m (the north-star bound), loss, gradient alignment, manifold property.  f16f8 = 3 (round 6): all four Linear layers of
    every block of the rotations net as one fp16 + one block-scaled fp8 product, the attention kernels and the GELU epilogue writing f16f8
    planes, the bf16 backward rounding the fp16 planes where it reads them - the same bounds."""
    from manipose_amd import RMCLManifoldMixSTE, h36m_skeleton
    from manipose_amd.metrics import mpjpe_error, rmcl_training_loss
    cfg = orc.FULL_CFG
    st_ = orc.make_state(cfg, seed=3)
    model = RMCLManifoldMixSTE(h36m_skeleton(), drop_path_rate=0.0)
    model.load_state_dict(st_, strict=True)
    model.precision, model.f16f8 = "bf16x3", f16f8
    model.max_batch_hint = 3
    model = model.cuda().eval()
    X, y = orc.synthetic_batch(3, 243, seed=42)
    with torch.no_grad():
        o3, _ = orc.rmcl_manifold_forward(X, st_, orc.oracle_cfg(cfg))
        p3, _ = model(X.cuda())
    mp3 = mpjpe_error(p3, o3.cuda(), "average").item()
    X, y = X[:1].contiguous(), y[:1].contiguous()
    poses, scores = model(X.cuda())
    req = {k: v.clone().requires_grad_(True) for k, v in st_.items()}
    o_poses, o_scores = orc.rmcl_manifold_forward(X, req, orc.oracle_cfg(cfg))
    mp = mpjpe_error(poses, o_poses.detach().cuda(), "average").item()
    print(f"\n[bf16x3 drift] full size T=243 K=5 f16f8={f16f8}: MPJPE vs fp32 oracle = {mp * 1e3:.5f} mm (B=1), {mp3 * 1e3:.5f} mm (B=3)")
    assert mp <= MPJPE_TOL_M and mp3 <= MPJPE_TOL_M
    close(scores, o_scores.detach(), rtol=1e-3, atol=1e-5)
    total, _ = rmcl_training_loss(poses, scores, y.cuda())
    o_total, _ = orc.rmcl_training_loss(o_poses, o_scores, y)
    assert abs(total.item() - o_total.item()) <= 1e-3 * abs(o_total.item())
    total.backward()
    o_total.backward()
    cs = {k: _cos(p.grad.cpu(), req[k].grad) for k, p in model.named_parameters()}
    worst = min(cs.items(), key=lambda kv: kv[1])
    mean = sum(cs.values()) / len(cs)
    wc, wck, _, wm, wmk = _grad_report(model.named_parameters(), {k: v.grad for k, v in req.items()})
    print(f"[bf16x3 drift] full size: gradient cosine mean {mean:.6f}, worst {worst[1]:.6f} at {worst[0]}; worst max-norm error {wm:.2e} at {wmk}")
    assert worst[1] > 0.9999 and mean > 0.99999, (worst, mean)      # measured: worst 0.999987, mean 0.999997
    assert wm < 2e-2, (wm, wmk)                                     # measured 4.7e-3 of the gradient's max-norm
    par = torch.tensor(orc.H36M_PARENTS[1:], device="cuda")
    seg = (poses[..., 1:, :] - poses[..., par, :]).norm(dim=-1)
    lens = model._engine.peek(1).view(1, 1, 1, 16).abs()
    close(seg, lens.expand_as(seg), rtol=1e-4, atol=2e-6)


_MASKED_FULL_SIZE = {}


def _masked_full_size_reference(layout):
    """The masked full-size case (FULL_CFG, B = 2, DropPath 0.1 with injected masks) and its CPU oracle forward, loss and gradients - computed
    once, shared by the precisions.  Masks: keep 0.9 (values 0 and 1/0.9), every branch drops a sample in each window, window 1 keeps the
    sample window 0 drops and drops another one."""
    if not _MASKED_FULL_SIZE:
        cfg = orc.FULL_CFG
        st_ = orc.make_state(cfg, seed=3)
        X, y = orc.synthetic_batch(2, 243, seed=42)
        gen = torch.Generator().manual_seed(17)
        masks = {}
        for name, _, cnt, keep in layout:
            if keep >= 1.0:
                continue
            m = (torch.rand(cnt, generator=gen) < 0.9).float() / 0.9
            half = cnt // 2
            m[1], m[half + 1], m[half + 3] = 0.0, 1.0 / 0.9, 0.0
            masks[name] = m
        assert sorted(masks) == sorted(droppath_mask_names(cfg, 0.1)), sorted(masks)
        req = {k: v.clone().requires_grad_(True) for k, v in st_.items()}
        o_poses, o_scores = orc.rmcl_manifold_forward(X, req, orc.oracle_cfg(cfg), masks=masks)
        o_total, _ = orc.rmcl_training_loss(o_poses, o_scores, y)
        o_total.backward()
        _MASKED_FULL_SIZE.update(st=st_, X=X, y=y, masks=masks, poses=o_poses.detach(), scores=o_scores.detach(), total=o_total.item(),
                                 grads={k: v.grad for k, v in req.items()})
    return _MASKED_FULL_SIZE


@pytest.mark.parametrize("precision,f16f8", [("fp32", 0), ("bf16x3", 0), ("bf16x3", 3)])
def test_full_size_model_with_droppath_masks_vs_oracle(lib, precision, f16f8):
    """The benchmarked training form: the full-size model (FULL_CFG) at B = 2 in train mode with DropPath 0.1 and injected masks in every
    branch of both nets, against the CPU oracle with the same masks - in fp32 and in the split precision with f16f8 = 0 and 3 (the timed
    form, whose wide blocks run the f16f8 kernels).  The bounds of the unmasked full-size tests."""
    from manipose_amd import RMCLManifoldMixSTE, h36m_skeleton
    from manipose_amd.metrics import mpjpe_error, rmcl_training_loss
    model = RMCLManifoldMixSTE(h36m_skeleton(), drop_path_rate=0.1)
    model.load_state_dict(orc.make_state(orc.FULL_CFG, seed=3), strict=True)
    model.precision, model.f16f8 = precision, f16f8
    model.max_batch_hint = 2
    model = model.cuda().train()
    model._ensure_engine(2, torch.device("cuda"))
    ref = _masked_full_size_reference(model._engine.mask_layout(2))
    model.set_droppath_masks({k: v.cuda() for k, v in ref["masks"].items()})
    poses, scores = model(ref["X"].cuda())
    total, _ = rmcl_training_loss(poses, scores, ref["y"].cuda())
    total.backward()
    mp = mpjpe_error(poses, ref["poses"].cuda(), "average").item()
    wc, wck, mean, wm, wmk = _grad_report(model.named_parameters(), ref["grads"])
    print(f"\n[masked full size] {precision} f16f8={f16f8}: MPJPE vs oracle {mp * 1e3:.5f} mm, loss {total.item():.6f} vs {ref['total']:.6f}, gradient "
          f"cosine mean {mean:.6f} worst {wc:.6f} ({wck}), worst max-norm error {wm:.2e} ({wmk})")
    assert mp <= MPJPE_TOL_M
    close(scores, ref["scores"], rtol=1e-3, atol=1e-5)
    assert abs(total.item() - ref["total"]) <= 1e-3 * abs(ref["total"])
    if precision == "fp32":
        _check_grads(model, {"g::" + k: v.numpy() for k, v in ref["grads"].items()})
    else:
        assert wc > 0.9999 and mean > 0.99999, (wc, wck, mean)
        assert wm < 2e-2, (wm, wmk)


def test_bf16x3_training_step_and_droppath(lib):
    """Train-mode DropPath (injected masks) in the split precision vs the reference fixture, then fused trainer steps whose loss
    falls."""
    from manipose_amd.metrics import mpjpe_error, rmcl_training_loss
    from manipose_amd.training import LiftingTrainer
    fx = load_fixture("rmcl_tiny_droppath")
    model = _build(fx, drop_path_rate=float(fx["drop_path_rate"]))
    model.precision = "bf16x3"
    model = model.train()
    model.set_droppath_masks({k: v.cuda() for k, v in fixture_masks(fx).items()})
    poses, scores = model(dev(fx["X"]))
    mp = mpjpe_error(poses, dev(fx["poses"]), "average").item()
    print(f"\n[bf16x3 drift] droppath fixture: {mp * 1e3:.5f} mm")
    assert mp <= MPJPE_TOL_M
    total, _ = rmcl_training_loss(poses, scores, dev(fx["y"]))
    np.testing.assert_allclose(total.item(), float(fx["loss_total"]), rtol=1e-3)
    model.set_droppath_masks(None)
    tr = LiftingTrainer(model, lr=1e-3, weight_decay=0.0, seed=1)
    X, y = dev(fx["X"]), dev(fx["y"])
    losses = [float(tr.train_step(X, y).sum().item()) for _ in range(8)]
    assert all(np.isfinite(losses)) and losses[-1] < losses[0], losses


def _grad_report(named_params, ref_grads):
    """(worst cosine, its key, mean cosine, worst max-norm error relative to the reference gradient's max-norm, its key)."""
    cs, mx = {}, {}
    for k, p in named_params:
        g, r = p.grad.detach().cpu().double(), ref_grads[k].double()
        cs[k] = _cos(g, r)
        mx[k] = float((g - r).abs().max() / (r.abs().max() + 1e-30))
    wc = min(cs.items(), key=lambda kv: kv[1])
    wm = max(mx.items(), key=lambda kv: kv[1])
    return wc[1], wc[0], sum(cs.values()) / len(cs), wm[1], wm[0]


@pytest.mark.parametrize("M,N,K,mode,T,J", [(66096, 512, 512, 1, 243, 17), (66096, 512, 1024, 2, 243, 17), (2754, 256, 256, 2, 27, 17), (2592, 128, 128, 1, 27, 16),
                                            (2754, 512, 512, 0, 27, 17), (12393, 512, 512, 0, 243, 17), (1001, 128, 128, 0, 7, 11), (1559, 256, 256, 0, 1559, 1),
                                            (3 * 243 * 16 + 48, 128, 256, 0, 243, 16)])
def test_bf16x3_residual_linear_with_recomputed_layernorm(lib, M, N, K, mode, T, J):
    """The residual Linear of a block from the third on (mix_ste.py:352-368 inside ST_foward :157-173) as the engine runs it in the split
    precision: y = LayerNorm(r_in) + DropPath-mask * (x W^T + b) with the LayerNorm recomputed in the GEMM epilogue from r_in and its row
    statistics - through mp_linear_fwd_bf16x3_lnres against the same expression in fp64.  Both the persistent kernel (forced from one
    tile up: the kernel the benchmark times) and the tiled kernels (256- and 128-wide tiles) are checked."""
    from manipose_amd import _lib
    g = torch.Generator().manual_seed(M + N + K + mode)
    x = torch.randn(M, K, generator=g)
    W = torch.randn(N, K, generator=g) / K ** 0.5
    b = torch.randn(N, generator=g)
    r_in = torch.randn(M, N, generator=g) * 2.0 + 0.3
    gamma, beta = 1.0 + 0.2 * torch.randn(N, generator=g), 0.1 * torch.randn(N, generator=g)
    mean = r_in.mean(1)
    rstd = (r_in.var(1, unbiased=False) + 1e-6).rsqrt()
    stats = torch.stack([mean, rstd], 1).contiguous()
    ns = {0: 0, 1: M // J, 2: (M // (T * J)) * J}[mode]
    mask = ((torch.rand(ns, generator=g) > 0.3).float() / 0.7) if mode else None
    rows = torch.arange(M)
    mrow = torch.ones(M) if mode == 0 else (mask[rows // J] if mode == 1 else mask[(rows // (T * J)) * J + rows % J])
    want = ((r_in.double() - mean.double()[:, None]) * rstd.double()[:, None] * gamma.double() + beta.double()
            + mrow.double()[:, None] * (x.double() @ W.double().t() + b.double()))
    scale = float(want.abs().max())
    xd, Wd = x.cuda(), W.cuda()
    xh, xl, Wh, Wl = (torch.empty(t.shape, device="cuda", dtype=torch.bfloat16) for t in (x, x, W, W))
    _lib.check(lib.mp_split_bf16(xd.data_ptr(), xh.data_ptr(), xl.data_ptr(), xd.numel(), st()))
    _lib.check(lib.mp_split_bf16(Wd.data_ptr(), Wh.data_ptr(), Wl.data_ptr(), Wd.numel(), st()))
    bd, rd, sd, gd, be = b.cuda(), r_in.cuda(), stats.cuda(), gamma.cuda(), beta.cuda()
    md = mask.cuda() if mask is not None else None
    for min_tiles in (1, 1 << 30):                   # persistent kernel forced / tiled kernels only
        _lib.check(lib.mp_set_option(b"gemm_persist_min_tiles", min_tiles))
        try:
            y = torch.full((M, N), float("nan"), device="cuda")
            _lib.check(lib.mp_linear_fwd_bf16x3_lnres(xh.data_ptr(), xl.data_ptr(), Wh.data_ptr(), Wl.data_ptr(), bd.data_ptr(), y.data_ptr(), rd.data_ptr(),
                                                      sd.data_ptr(), gd.data_ptr(), be.data_ptr(), md.data_ptr() if md is not None else None, mode, T, J,
                                                      M, N, K, st()), "mp_linear_fwd_bf16x3_lnres")
        finally:
            _lib.check(lib.mp_set_option(b"gemm_persist_min_tiles", 0))
        err = (y.cpu().double() - want).abs().max().item() / scale
        assert err < 4e-5, (min_tiles, err)                                     # bf16 operands: ~4e-3
    with pytest.raises(RuntimeError):                # y may not alias r_in
        _lib.check(lib.mp_linear_fwd_bf16x3_lnres(xh.data_ptr(), xl.data_ptr(), Wh.data_ptr(), Wl.data_ptr(), bd.data_ptr(), rd.data_ptr(), rd.data_ptr(),
                                                  sd.data_ptr(), gd.data_ptr(), be.data_ptr(), None, 0, T, J, M, N, K, st()), "alias")


@pytest.mark.parametrize("train", [False, True])
def test_bf16x3_persistent_kernels_inside_the_model_vs_oracle(lib, train):
    """The kernels the benchmark times - gemm_bf16_persist_kernel<.., SPLIT=1> with the bias, GELU and (recomputed-LayerNorm) residual
    epilogues, which the default rule only selects from 512 output tiles up - forced on (one tile is enough) inside a model wide and deep
    enough for them (C = 256, depth 3: the lazy block input / recomputed residual runs from the third block on), eval mode and train mode
    with injected DropPath masks, against the CPU ORACLE (not against the tiled kernels): MPJPE within the north-star bound, scores,
    loss, every parameter gradient.  The engine's own launch accounting proves the persistent kernel ran."""
    from manipose_amd import RMCLManifoldMixSTE, _lib, h36m_skeleton
    from manipose_amd.metrics import mpjpe_error, rmcl_training_loss
    cfg = dict(T=27, J=17, num_bones=16, C_rot=256, depth_rot=3, heads_rot=4, C_seg=256, depth_seg=2, heads_seg=4, n_hyp=3)
    B, rate = 6, 0.3
    st_ = orc.make_state(cfg, seed=21)
    X, y = orc.synthetic_batch(B, cfg["T"], seed=9)
    _lib.check(lib.mp_set_option(b"gemm_persist_min_tiles", 1))
    try:
        model = RMCLManifoldMixSTE(h36m_skeleton(), num_frame=cfg["T"], embed_dim_rot=256, depth_rot=3, num_heads_rot=4, embed_dim_seg=256,
                                   depth_seg=2, num_heads_seg=4, n_hyp=3, drop_path_rate=rate if train else 0.0)
        model.load_state_dict(st_, strict=True)
        model.precision = "bf16x3"
        model = model.cuda()
        model = model.train() if train else model.eval()
        model._ensure_engine(B, torch.device("cuda"))
        masks = None
        if train:
            gen = torch.Generator().manual_seed(11)
            masks = {name: (torch.rand(cnt, generator=gen) < keep).float() / keep for name, _, cnt, keep in model._engine.mask_layout(B) if keep < 1.0}
            model.set_droppath_masks({k: v.cuda() for k, v in masks.items()})
        model._engine.prof_enable(True)
        poses, scores = model(X.cuda())
        total, _ = rmcl_training_loss(poses, scores, y.cuda())
        total.backward()
        prof = model._engine.prof_collect()
        model._engine.prof_enable(False)
    finally:
        _lib.check(lib.mp_set_option(b"gemm_persist_min_tiles", 0))
    # 4 Linear layers x 2 blocks x depth, both backbones, forward; the dgrad launches of the backward on top
    n_fwd = 4 * 2 * (cfg["depth_rot"] + cfg["depth_seg"])
    assert prof["gemm_persist"]["launches"] >= n_fwd, prof["gemm_persist"]
    req = {k: v.clone().requires_grad_(True) for k, v in st_.items()}
    o_poses, o_scores = orc.rmcl_manifold_forward(X, req, orc.oracle_cfg(cfg), masks=masks)
    o_total, _ = orc.rmcl_training_loss(o_poses, o_scores, y)
    o_total.backward()
    mp = mpjpe_error(poses, o_poses.detach().cuda(), "average").item()
    wc, wck, mean, wm, wmk = _grad_report(model.named_parameters(), {k: v.grad for k, v in req.items()})
    print(f"\n[bf16x3 persistent] train={train}: MPJPE vs oracle {mp * 1e3:.5f} mm, loss {total.item():.6f} vs {o_total.item():.6f}, gradient cosine "
          f"mean {mean:.6f} worst {wc:.6f} ({wck}), worst max-norm error {wm:.2e} ({wmk}), persistent launches {prof['gemm_persist']['launches']}")
    assert mp <= MPJPE_TOL_M
    close(scores, o_scores.detach(), rtol=1e-3, atol=1e-5)
    assert abs(total.item() - o_total.item()) <= 1e-3 * abs(o_total.item())
    assert wc > 0.9999 and mean > 0.99999, (wc, wck, mean)          # measured: worst 0.999992, mean 0.999998
    assert wm < 2e-2, (wm, wmk)                     # measured 5e-3 (bf16 backward)


@pytest.mark.parametrize("precision,optimiser", [("fp32", "adam"), ("bf16x3", "adam"), ("fp32", "damped"), ("bf16x3", "damped"),
                                                 ("bf16x3@256", "damped"), ("bf16x3@256+f16", "damped"), ("bf16x3@256+f16", "adam")])
def test_ten_training_steps_follow_the_oracle_trajectory(lib, precision, optimiser):
    """The loop of train() (hpe/main_h36m_lifting.py:294-311) for ten optimisation steps - engine forward, fused loss, engine backward,
    fused Adam - against the oracle's own ten steps (autograd + orc.adam_step) from the same weights on the same batch, DropPath off:
    the loss of every step and, at the end, the two models' outputs on the batch.

    "adam" = the reference's optimiser settings (lr 4e-5, eps 1e-8).  Adam's first steps are lr * sign(g): a weight whose gradient is
    smaller than the rounding noise of the backward moves by the full lr in a noise-decided direction, so two correct implementations
    drift apart along loss-neutral directions however small their gradient difference is - the fp32 engine (gradients within 3e-4 of
    the oracle's) already ends 0.08 mm from the oracle after ten steps.  For the split precision (bf16 backward: gradients within 5e-3
    max-norm, cosine 0.99999) only the per-step LOSS is bounded there; the distance of the outputs is printed, not asserted.
    "damped" = the same kernel with eps = 1 (update ~ lr * m: the noise is not amplified): there the fp32 engine must end within the
    north-star bound of the oracle (measured 0.001 mm after the outputs moved 369 mm) and the split precision within 0.1 % of the distance
    the outputs travelled (measured 0.21 mm of 369 mm = 0.06 %: what a backward with 8-bit operands can hold) - the statement that the
    backward itself is right.
    "@256" = the rotations net 256 wide (head dim 64), where the persistent GEMMs (forced on), the MFMA attention kernels and - "+f16" -
    the f16f8 operand form with its scaled-fp16 backward (mp_model_config::f16f8 = 1, f16_backward = 1) are what runs: the optional
    backward goes through an optimiser trajectory against the oracle with the same asserted bounds."""
    from manipose_amd import RMCLManifoldMixSTE, h36m_skeleton
    from manipose_amd.metrics import mpjpe_error
    from manipose_amd.optim import FusedAdam
    from manipose_amd.training import LiftingTrainer
    from manipose_amd import _lib
    wide, f16 = "@256" in precision, precision.endswith("+f16")
    precision = precision.split("@")[0]
    Cr, Hr = (256, 4) if wide else (128, 8)
    cfg = dict(T=27, J=17, num_bones=16, C_rot=Cr, depth_rot=3, heads_rot=Hr, C_seg=64, depth_seg=2, heads_seg=4, n_hyp=3)
    B, steps, wd = 4, 10, 1e-6
    lr, eps = (4e-5, 1e-8) if optimiser == "adam" else (2e-3, 1.0)
    st_ = orc.make_state(cfg, seed=5)
    X, y = orc.synthetic_batch(B, cfg["T"], seed=13)
    model = RMCLManifoldMixSTE(h36m_skeleton(), num_frame=cfg["T"], embed_dim_rot=Cr, depth_rot=3, num_heads_rot=Hr, embed_dim_seg=64,
                               depth_seg=2, num_heads_seg=4, n_hyp=3, drop_path_rate=0.0)
    model.load_state_dict(st_, strict=True)
    model.precision = precision
    if f16:
        model.f16f8, model.f16_backward = 1, True
    model = model.cuda().train()
    tr = LiftingTrainer(model, lr=lr, weight_decay=wd, seed=1)
    tr.opt = FusedAdam(model, lr=lr, weight_decay=wd, eps=eps)
    Xd, yd = X.cuda(), y.cuda()
    if wide:
        _lib.check(lib.mp_set_option(b"gemm_persist_min_tiles", 1))
    try:
        if wide:
            model._ensure_engine(B, Xd.device)
            model._engine.prof_enable(True)
        got = [float(tr.train_step(Xd, yd).sum().item()) for _ in range(steps)]
        if wide:
            assert model._engine.prof_collect()["gemm_persist"]["launches"] > 0
            model._engine.prof_enable(False)
            h = model._engine.grad_health()
            assert h["saturated"] == 0 and h["non_finite"] == 0 and (h["scale"] > 0) == f16, h
    finally:
        if wide:
            _lib.check(lib.mp_set_option(b"gemm_persist_min_tiles", 0))
    w = {k: v.clone().requires_grad_(True) for k, v in st_.items()}
    m1 = {k: torch.zeros_like(v) for k, v in st_.items()}
    m2 = {k: torch.zeros_like(v) for k, v in st_.items()}
    want = []
    for i in range(steps):
        poses, scores = orc.rmcl_manifold_forward(X, w, orc.oracle_cfg(cfg))
        total, _ = orc.rmcl_training_loss(poses, scores, y)
        for v in w.values():
            v.grad = None
        total.backward()
        want.append(float(total.item()))
        with torch.no_grad():
            for k in w:
                pk, m1[k], m2[k] = orc.adam_step(w[k], w[k].grad, m1[k], m2[k], i + 1, lr=lr, eps=eps, weight_decay=wd)
                w[k].copy_(pk)
    rel = max(abs(a - b) / abs(b) for a, b in zip(got, want))
    with torch.no_grad():
        o_poses, o_scores = orc.rmcl_manifold_forward(X, w, orc.oracle_cfg(cfg))
        o_first, _ = orc.rmcl_manifold_forward(X, st_, orc.oracle_cfg(cfg))
        p, s = model.eval()(Xd)
    mp = mpjpe_error(p, o_poses.cuda(), "average").item()
    moved = (o_poses - o_first).norm(dim=-1).mean().item()
    dw = max(float((dict(model.named_parameters())[k].detach().cpu() - w[k].detach()).abs().max()) for k in w)
    print(f"\n[trajectory] {precision} / {optimiser}: loss {want[0]:.4f} -> {want[-1]:.4f}, worst per-step loss deviation {rel:.2e}, the oracle's "
          f"outputs moved {moved * 1e3:.2f} mm in {steps} steps, MPJPE between the two trained models {mp * 1e3:.5f} mm, largest weight difference {dw:.2e}")
    assert want[-1] < want[0]
    if optimiser == "adam":
        assert rel <= (1e-4 if precision == "fp32" else 5e-3), (got, want)
        if precision == "fp32":
            assert mp <= 2e-4, mp
    else:
        assert rel <= (1e-4 if precision == "fp32" else 1e-3), (got, want)
        assert mp <= (MPJPE_TOL_M if precision == "fp32" else 1e-3 * moved), (mp, moved)
        close(s, o_scores, rtol=2e-3, atol=2e-4 if precision == "bf16x3" else 2e-5)


@pytest.mark.parametrize("ntok,C", [(16, 128), (17, 512)])
def test_split_precision_linear_kernels_are_reproducible_at_scale(lib, ntok, C):
    """Run-to-run reproducibility of every split-precision Linear variant at a training-size token count, tiled and persistent kernels:
    the same launch three times must give the same BITS.  (Round 3: the tiled residual epilogue with the recomputed LayerNorm produced
    wrong values in ~1e-4 of the rows, different in every run - invisible at the row counts the parity tests use, 2 mm on the segment
    lengths at the benchmark's batch.  See the comment in gemm_bf16_glds_kernel's epilogue.)"""
    from manipose_amd import _lib
    M = 40 * 243 * ntok
    g = torch.Generator(device="cuda").manual_seed(ntok)
    shapes = (("qkv", 3 * C, C, 0), ("fc1", 2 * C, C, 1), ("proj", C, C, 2), ("fc2", C, 2 * C, 2), ("proj+ln", C, C, 3))
    for name, N, K, epi in shapes:
        x = torch.randn(M, K, device="cuda", generator=g)
        W = torch.randn(N, K, device="cuda", generator=g) / K ** 0.5
        b = torch.randn(N, device="cuda", generator=g)
        r = torch.randn(M, N, device="cuda", generator=g)
        stats = torch.stack([r.mean(1), (r.var(1, unbiased=False) + 1e-6).rsqrt()], 1).contiguous()
        gam, bet = torch.rand(N, device="cuda", generator=g) + 0.5, torch.randn(N, device="cuda", generator=g)
        xh, xl, Wh, Wl = (torch.empty(t.shape, device="cuda", dtype=torch.bfloat16) for t in (x, x, W, W))
        _lib.check(lib.mp_split_bf16(x.data_ptr(), xh.data_ptr(), xl.data_ptr(), x.numel(), st()))
        _lib.check(lib.mp_split_bf16(W.data_ptr(), Wh.data_ptr(), Wl.data_ptr(), W.numel(), st()))

        def run():
            if epi in (0, 1):
                yh, yl = torch.zeros(M, N, device="cuda", dtype=torch.bfloat16), torch.zeros(M, N, device="cuda", dtype=torch.bfloat16)
                z = torch.zeros(M, N, device="cuda", dtype=torch.bfloat16) if epi == 1 else None
                _lib.check(lib.mp_linear_fwd_bf16x3(xh.data_ptr(), xl.data_ptr(), Wh.data_ptr(), Wl.data_ptr(), b.data_ptr(), yh.data_ptr(), yl.data_ptr(),
                                                    z.data_ptr() if z is not None else None, None, M, N, K, epi, st()))
                return [yh.view(torch.int16), yl.view(torch.int16)] + ([z.view(torch.int16)] if z is not None else [])
            y = torch.zeros(M, N, device="cuda")
            if epi == 2:
                _lib.check(lib.mp_linear_fwd_bf16x3(xh.data_ptr(), xl.data_ptr(), Wh.data_ptr(), Wl.data_ptr(), b.data_ptr(), y.data_ptr(), None, None,
                                                    r.data_ptr(), M, N, K, 2, st()))
            else:
                _lib.check(lib.mp_linear_fwd_bf16x3_lnres(xh.data_ptr(), xl.data_ptr(), Wh.data_ptr(), Wl.data_ptr(), b.data_ptr(), y.data_ptr(), r.data_ptr(),
                                                          stats.data_ptr(), gam.data_ptr(), bet.data_ptr(), None, 0, 243, ntok, M, N, K, st()))
            return [y.view(torch.int32)]
        for mode in (0, 1):                          # tiled kernels only / persistent kernel where it applies
            _lib.check(lib.mp_set_option(b"gemm_persist_mode", mode))
            try:
                first = run()
                for _ in range(2):
                    again = run()
                    bad = sum(int((a != c).sum().item()) for a, c in zip(first, again))
                    assert bad == 0, f"{name} (N={N}, K={K}, persist_mode={mode}): {bad} elements differ between two identical launches"
            finally:
                _lib.check(lib.mp_set_option(b"gemm_persist_mode", 1))
        # the same Linear on "f16f8" operands (the hand-scheduled fp16 + block-scaled fp8 k-steps of round 6; persistent kernel only)
        if N % 256 == 0 and K % 64 == 0 and epi in (0, 1, 2):
            x16, W16 = torch.empty(M, K, device="cuda", dtype=torch.float16), torch.empty(N, K, device="cuda", dtype=torch.float16)
            x8, W8 = torch.empty(M, 2 * K, device="cuda", dtype=torch.uint8), torch.empty(N, 2 * K, device="cuda", dtype=torch.uint8)
            _lib.check(lib.mp_split_f16f8(x.data_ptr(), x16.data_ptr(), x8.data_ptr(), x.numel(), 0, st()))
            _lib.check(lib.mp_split_f16f8(W.data_ptr(), W16.data_ptr(), W8.data_ptr(), W.numel(), 1, st()))
            outs = []
            for _ in range(3):
                y = torch.zeros(M, N, device="cuda")
                _lib.check(lib.mp_linear_fwd_f16f8(x16.data_ptr(), x8.data_ptr(), W16.data_ptr(), W8.data_ptr(), b.data_ptr(), y.data_ptr(), M, N, K, st()))
                outs.append(y.view(torch.int32))
            bad = sum(int((outs[0] != o).sum().item()) for o in outs[1:])
            assert bad == 0, f"{name} f16f8 (N={N}, K={K}): {bad} elements differ between identical launches"


def test_bench_batch_of_158_windows_is_two_times_its_half(lib):
    """bench.py's default batch (158 windows per GPU since round 5: 652 698 tokens, 2.0 GB per qkv plane - close to what 31-bit byte offsets hold)
    through a size-independent property, the oracle being far too slow there: a batch made of two copies of a 79-window batch must give
    every window of the second copy the poses of the first BIT FOR BIT (and the first copy those of the 79-window batch alone), and - with the upstream gradients duplicated too - twice the parameter gradients
    of the 79-window batch, up to the summation order of the token sums (eval mode: no DropPath; full width, benchmarked precision)."""
    import gc
    from manipose_amd import RMCLManifoldMixSTE, h36m_skeleton
    gc.collect(); torch.cuda.empty_cache()
    H, B = 79, 158
    torch.manual_seed(42)
    model = RMCLManifoldMixSTE(h36m_skeleton(), num_frame=243, n_hyp=5, drop_path_rate=0.1)
    model.precision, model.f16f8 = "bf16x3", 3          # the benchmark's operand form since round 6
    model.max_batch_hint = B
    model = model.cuda().eval()
    X, _ = orc.synthetic_batch(H, 243, seed=11)
    X = X.cuda()
    X2 = torch.cat([X, X], 0).contiguous()
    model._ensure_engine(B, X.device)
    eng, flat = model._engine, model.flat_parameters()
    dp = torch.randn(H, 5, 243, 17, 3, device="cuda", generator=torch.Generator(device="cuda").manual_seed(3)) * 1e-3
    ds = torch.randn(H, 5, 243, 1, device="cuda", generator=torch.Generator(device="cuda").manual_seed(4)) * 1e-3

    def run(x, gp, gs):
        poses, scores = eng.forward(flat, x, train=False)
        poses, scores = poses.clone(), scores.clone()
        grads = torch.zeros_like(flat)
        eng.backward(flat, grads, gp, gs)
        torch.cuda.synchronize()
        return poses, scores, grads
    p1, s1, g1 = run(X, dp, ds)
    p2, s2, g2 = run(X2, torch.cat([dp, dp], 0).contiguous(), torch.cat([ds, ds], 0).contiguous())
    assert torch.isfinite(p2).all() and torch.isfinite(g2).all()
    for name, u, v in (("poses: first half of the 158 vs the 79 alone", p2[:H], p1), ("poses: second half vs first half of the 158", p2[H:], p2[:H]),
                       ("scores: first half vs alone", s2[:H], s1), ("scores: second half vs first half", s2[H:], s2[:H])):
        d = (u - v).abs().reshape(-1)
        nz = int((d > 0).sum())
        print(f"\n[158 = 2 x 79] {name}: {nz} of {d.numel()} values differ, mean {float(d.mean()):.3e}, 99.9 % {float(d.float().kthvalue(int(0.999 * d.numel())).values):.3e}, max {float(d.max()):.3e}")
        assert nz == 0, name      # (round 5: the GELU epilogue's lo plane used to differ by an ulp in the last 4 of a wave's 128 rows - csrc/common.h, split_bf16x2)
    rel = float((g2 - 2.0 * g1).abs().max() / (2.0 * g1).abs().max())
    cos = _cos(g2, g1)
    print(f"\n[158 = 2 x 79] gradients: max |g158 - 2 g79| / max |2 g79| = {rel:.2e}, cosine {cos:.8f}")
    assert rel < 2e-3 and cos > 0.999999, (rel, cos)
    del eng
    model._engine = None
    del model
    gc.collect(); torch.cuda.empty_cache()


def test_batch_beyond_the_2_gib_plane_boundary_vs_oracle_and_small_batch(lib):
    """172 windows of T=243 at full width in the benchmarked precision: 710 532 tokens, so each 2-byte plane of the fused qkv activation (and of
    its gradient) is 2.18 GB - past 2^31 bytes, which bench.py's default batch (158) stays 7 % under.  (a) Forward: parity windows placed in the
    FIRST, MIDDLE and LAST row of the batch against the fp32 CPU oracle (north-star bound), and bit-identical to the same windows run as a
    3-window batch (a window's result does not depend on its row).  (b) Backward: with upstream gradients on those three rows only, the
    parameter gradients of the 172-window step equal those of the 3-window step up to the summation order of the token sums - a wrong
    address past the boundary in any forward or backward kernel of the LAST row would show in either."""
    import gc
    from manipose_amd import RMCLManifoldMixSTE, h36m_skeleton
    gc.collect(); torch.cuda.empty_cache()
    B = 172
    torch.manual_seed(42)
    model = RMCLManifoldMixSTE(h36m_skeleton(), num_frame=243, n_hyp=5, drop_path_rate=0.1)
    with torch.no_grad():
        for n, p in model.named_parameters():
            if n.endswith("pos_embed"):
                p.normal_(0.0, 0.02)
    state = {k: v.detach().clone() for k, v in model.state_dict().items()}
    model.precision, model.f16f8 = "bf16x3", 3          # the benchmark's operand form since round 6
    model.max_batch_hint = B
    model = model.cuda().eval()
    assert 2 * B * 243 * 17 * 1536 > 2 ** 31
    Xp, _ = orc.synthetic_batch(3, 243, seed=21)
    with torch.no_grad():
        o_poses, o_scores = orc.rmcl_manifold_forward(Xp, state, orc.oracle_cfg(orc.FULL_CFG))
    Xb, _ = orc.synthetic_batch(B, 243, seed=22)
    rows = [0, B // 2, B - 1]
    Xb[rows] = Xp
    Xb, Xp = Xb.cuda(), Xp.cuda()
    model._ensure_engine(B, Xb.device)
    eng, flat = model._engine, model.flat_parameters()
    gen = torch.Generator(device="cuda").manual_seed(3)
    dp3 = torch.randn(3, 5, 243, 17, 3, device="cuda", generator=gen) * 1e-3
    ds3 = torch.randn(3, 5, 243, 1, device="cuda", generator=gen) * 1e-3
    dpB = torch.zeros(B, 5, 243, 17, 3, device="cuda")
    dsB = torch.zeros(B, 5, 243, 1, device="cuda")
    dpB[rows], dsB[rows] = dp3, ds3

    def run(x, gp, gs):
        poses, scores = eng.forward(flat, x, train=False)
        poses, scores = poses.clone(), scores.clone()
        grads = torch.zeros_like(flat)
        eng.backward(flat, grads, gp, gs)
        torch.cuda.synchronize()
        return poses, scores, grads
    from manipose_amd import _lib
    pB, sB, gB = run(Xb, dpB, dsB)
    _lib.check(lib.mp_set_option(b"gemm_persist_min_tiles", 1))      # the 3-window batch on the persistent GEMM kernels too (same epilogue code: same bits)
    try:
        p3, s3, g3 = run(Xp, dp3, ds3)
    finally:
        _lib.check(lib.mp_set_option(b"gemm_persist_min_tiles", 0))
    assert torch.isfinite(pB).all() and torch.isfinite(gB).all()
    mp = (pB[rows].cpu() - o_poses).norm(dim=-1).mean(dim=(1, 2, 3))
    print(f"\n[B=172, planes past 2^31 bytes] MPJPE vs oracle at rows {rows}: {[f'{v:.2e}' for v in mp.tolist()]} m; workspace {eng.workspace_bytes / 2**30:.1f} GiB")
    assert float(mp.max()) <= MPJPE_TOL_M and float((sB[rows].cpu() - o_scores).abs().max()) < 1e-3
    assert torch.equal(pB[rows], p3) and torch.equal(sB[rows], s3), "a window's forward depends on its row past the 2 GiB boundary"
    rel = float((gB - g3).abs().max() / g3.abs().max())
    cos = _cos(gB, g3)
    print(f"[B=172] gradients of the three live rows vs the 3-window step: max |dg| / max |g| = {rel:.2e}, cosine {cos:.8f}")
    assert rel < 2e-3 and cos > 0.999999, (rel, cos)
    del eng
    model._engine = None
    del model
    gc.collect(); torch.cuda.empty_cache()


@pytest.mark.parametrize("f16f8", [3, 0])
def test_training_step_is_bitwise_reproducible_and_batch_invariant(lib, f16f8):
    """The benchmarked precision at full width (T=243 K=5 C=512 depth 8) and a batch of 16 windows - persistent GEMMs, side streams,
    train-mode DropPath from the engine's counter-based stream: two identical steps must produce the same BITS (poses, scores, segment
    lengths, every gradient: the backward is deterministic by construction - fixed-order slab / partial reductions, no atomics), the
    forward of a window must not depend on the batch it sits in, and the kernel-family / stream choices may move a pose by rounding only.
    f16f8 = 3: the benchmark's operand form since round 6 (all four Linear layers as one fp16 + one fp8 product); 0: three bf16 products.
    The persistent path's GRADIENTS are held against an independent path too (round-5 advisory): the same training step on the tiled GEMM
    kernels, one queue."""
    from manipose_amd import RMCLManifoldMixSTE, _lib, h36m_skeleton
    B = 16
    torch.manual_seed(42)
    model = RMCLManifoldMixSTE(h36m_skeleton(), num_frame=243, n_hyp=5, drop_path_rate=0.1)
    with torch.no_grad():
        for n, p in model.named_parameters():
            if n.endswith("pos_embed"):
                p.normal_(0.0, 0.02)
    model.precision, model.f16f8 = "bf16x3", f16f8
    model.max_batch_hint = B
    model = model.cuda().train()
    X, y = orc.synthetic_batch(B, 243, seed=7)
    X = X.cuda()
    model._ensure_engine(B, X.device)
    eng, flat = model._engine, model.flat_parameters()
    dp = torch.randn(B, 5, 243, 17, 3, device="cuda", generator=torch.Generator(device="cuda").manual_seed(3)) * 1e-3
    ds = torch.randn(B, 5, 243, 1, device="cuda", generator=torch.Generator(device="cuda").manual_seed(4)) * 1e-3

    def step():
        poses, scores = eng.forward(flat, X, train=True, seed=5, step=9)
        lens = eng.peek(1).clone()
        grads = torch.zeros_like(flat)
        eng.backward(flat, grads, dp, ds)
        torch.cuda.synchronize()
        return poses.clone(), scores.clone(), lens, grads
    a, b = step(), step()
    for name, u, v in zip(("poses", "scores", "segment lengths", "gradients"), a, b):
        nd = int((u.view(torch.int32) != v.view(torch.int32)).sum().item())
        assert nd == 0, f"{name}: {nd} of {u.numel()} values differ between two identical training steps (max {float((u - v).abs().max()):.3e})"
    assert torch.isfinite(a[3]).all()
    # eval mode: a window alone, in the batch, and in the batch with the other kernel family / without the side stream
    model.eval()
    with torch.no_grad():
        full, _ = eng.forward(flat, X, train=False)
        full = full.clone()
        alone, _ = eng.forward(flat, X[5:7].contiguous(), train=False)
        alone = alone.clone()
        # the other kernel family on ONE queue: a second model on the same weights whose config switches the engine's extra streams off
        # (mp_model_config::streams, per model since ABI v7) while the process-wide hook selects the tiled GEMM kernels
        single = RMCLManifoldMixSTE(h36m_skeleton(), num_frame=243, n_hyp=5, drop_path_rate=0.1)
        single.load_state_dict(model.state_dict(), strict=True)
        single.precision, single.f16f8, single.side_stream, single.wgrad_stream, single.max_batch_hint = "bf16x3", f16f8, False, False, B
        single = single.cuda().eval()
        _lib.check(lib.mp_set_option(b"gemm_persist_mode", 0))
        try:
            plain, _ = single(X)
            plain = plain.clone()
            # the training step of `step()` above on this engine: tiled bf16 / bf16x3 GEMM kernels (the f16f8 forward GEMMs exist in the persistent
            # form only), every kernel on one queue - an independent path to the same gradients
            seng, sflat = single._engine, single.flat_parameters()
            seng.forward(sflat, X, train=True, seed=5, step=9)
            g_tiled = torch.zeros_like(sflat)
            seng.backward(sflat, g_tiled, dp, ds)
            torch.cuda.synchronize()
        finally:
            _lib.check(lib.mp_set_option(b"gemm_persist_mode", 1))
        assert single._engine.cfg.streams == 3 and eng.cfg.streams == 0
    rel_g = float((a[3] - g_tiled).abs().max() / g_tiled.abs().max())
    cos_g = _cos(a[3], g_tiled)
    print(f"\n[f16f8={f16f8}] gradients, persistent kernels + three queues vs tiled kernels on one queue: max |dg| / max |g| = {rel_g:.2e}, cosine {cos_g:.8f}")
    assert rel_g < 2e-3 and cos_g > 0.99999, (rel_g, cos_g)
    # B = 16 runs the persistent GEMMs in the rotations net, B = 2 the tiled ones: same products, different epilogue code -> rounding-level
    # differences only (a wrong row would be ~1 m off)
    d_alone = (full[5:7] - alone).norm(dim=-1)
    d_plain = (full - plain).norm(dim=-1)
    print(f"\n[batch invariance] window in a batch of {B} vs alone: mean {d_alone.mean().item():.2e} m max {d_alone.max().item():.2e}; persistent + side stream "
          f"vs tiled on one stream: mean {d_plain.mean().item():.2e} m max {d_plain.max().item():.2e}")
    assert d_alone.mean().item() < 2e-5 and d_plain.mean().item() < 2e-5, (d_alone.mean().item(), d_plain.mean().item())


def test_workspace_larger_than_the_device_memory_is_refused_cleanly(lib):
    """The activation arena is sized for max_batch windows (1.57 GiB per window at full width in the split precision: 124 GiB at the
    benchmark's 79).  A batch whose arena cannot be allocated must come back as an error of mp_model_create - code 2, a message naming the
    size - and leave the device usable; it must not crash or half-initialise a model."""
    import ctypes as C
    from manipose_amd import RMCLManifoldMixSTE, _lib, h36m_skeleton
    cfg = _lib.ModelConfig(arch=0, num_frame=243, num_joints=17, num_bones=16, embed_dim_rot=512, depth_rot=8, num_heads_rot=8, embed_dim_seg=128,
                           depth_seg=2, num_heads_seg=8, n_hyp=5, drop_path_rate=0.1, max_batch=400, precision=2, rot_rep_dim=6)
    h = C.c_void_p()
    rc = lib.mp_model_create(C.byref(cfg), C.byref(h))
    assert rc == 2 and not h.value, rc
    msg = lib.mp_last_error().decode()
    assert "hipMalloc" in msg and "bytes" in msg, msg
    need = int(msg.split("hipMalloc(")[1].split(" bytes")[0])
    assert need > torch.cuda.get_device_properties(0).total_memory                 # it was refused for the right reason
    # the Python mirror turns it into a RuntimeError, and the device still works afterwards
    model = RMCLManifoldMixSTE(h36m_skeleton(), num_frame=243, n_hyp=5)
    model.precision = "bf16x3"
    model.max_batch_hint = 400
    with pytest.raises(RuntimeError, match="hipMalloc"):
        model.cuda()(torch.zeros(400, 243, 17, 2, device="cuda"))
    del model
    small = RMCLManifoldMixSTE(h36m_skeleton(), num_frame=27, embed_dim_rot=64, depth_rot=1, num_heads_rot=4, embed_dim_seg=32, depth_seg=1, num_heads_seg=4,
                               n_hyp=2).cuda().eval()
    p, _ = small(torch.zeros(2, 27, 17, 2, device="cuda"))
    assert torch.isfinite(p).all()


def test_custom_joint_weights_and_no_agg_segment_table_vs_oracle(lib):
    """The `weights` argument of the reference's loss functions with arbitrary per-joint weights (losses.py:14-43,104-138,
    regularizations.py:160-174) and segments_len_err(mode="no_agg") (mean_joint_errors.py:83-130) against the oracle."""
    from manipose_amd import h36m_skeleton
    from manipose_amd.metrics import (segments_len_err, smoothness_regularization, weighted_mpjpe_loss, wta_l2_loss_and_activate_head,
                                      wta_with_scoring_loss)
    g = torch.Generator().manual_seed(5)
    B, K, T = 3, 4, 11
    hyp = torch.randn(B, K, T, 17, 3, generator=g)
    sc = torch.softmax(torch.randn(B, K, T, 1, generator=g), dim=1)
    y = torch.randn(B, T, 17, 3, generator=g)
    w = torch.rand(17, generator=g) * 3 + 0.1
    hd = hyp.cuda().requires_grad_(True)
    sd = sc.cuda().requires_grad_(True)
    tot, reg = wta_with_scoring_loss(hd, sd, y.cuda(), 0.1, weights=w)
    ho, so = hyp.clone().requires_grad_(True), sc.clone().requires_grad_(True)
    o_tot, o_reg = orc.wta_with_scoring_loss(ho, so, y, 0.1, weights=w)
    close(tot, o_tot.detach(), rtol=1e-5, atol=1e-6)
    tot.backward()
    o_tot.backward()
    close(hd.grad, ho.grad, rtol=1e-4, atol=1e-7)
    vals, idx = wta_l2_loss_and_activate_head(hyp.cuda(), y.cuda(), weights=w)
    o_vals, o_idx = orc.wta_l2_loss_and_activate_head(hyp, y, weights=w)
    assert torch.equal(idx.cpu(), o_idx)
    close(vals, o_vals, rtol=1e-5, atol=1e-6)
    close(smoothness_regularization(hyp.cuda(), w, axis=2), orc.smoothness_regularization(hyp, w, 2), rtol=1e-5)
    close(weighted_mpjpe_loss(hyp[:, 0].cuda().contiguous(), y.cuda(), w), orc.weighted_mpjpe_loss(hyp[:, 0], y, w), rtol=1e-5)
    # per-frame segment-length table on the reference's (B, 3, J, L) views
    pred, gt = hyp[:, 0].permute(0, 3, 2, 1), y.permute(0, 3, 2, 1)
    for signed in (True, False):
        got = segments_len_err(pred.cuda(), gt.cuda(), h36m_skeleton(), "no_agg", signed=signed)
        lp = orc.measure_bones_length(pred).permute(0, 2, 1).reshape(B * T, -1)
        lg = orc.measure_bones_length(gt).permute(0, 2, 1).reshape(B * T, -1)
        want = lg - lp if signed else (lg - lp).abs()
        assert got.shape == (B * T, 16)
        close(got, want, rtol=1e-5, atol=1e-6)


# --------------------------------------------------------------------------------------------- muP mode (model.mup=True)
@pytest.mark.parametrize("precision", ["fp32", "bf16x3", "bf16"])
@pytest.mark.parametrize("name", ["mup_manifold", "mup_rmcl"])
def test_mup_mode_models_vs_reference_fixture(lib, name, precision):
    """model.mup=True: attention scale 1 / head_dim, residual scale 1 / sqrt(depth) (the reference's own code, pinned by fixtures generated
    from it) and MuReadout heads (input multiplier 1 / width_mult from base shapes; third-party formula) through the engine."""
    from test_host_cpu import _mup_model
    from manipose_amd.metrics import manifold_training_loss, mpjpe_error, rmcl_training_loss
    fx = load_fixture(name)
    model = _mup_model(fx)
    model.precision = precision
    model = model.cuda().eval()
    X, y = dev(fx["X"]), dev(fx["y"])
    if fx["cfg"]["n_hyp"]:
        poses, scores = model(X)
        total, _ = rmcl_training_loss(poses, scores, y)
    else:
        poses = model(X)
        total, _ = manifold_training_loss(poses, y)
    mp = mpjpe_error(poses, dev(fx["poses"]), "average").item()
    print(f"\n[mup {name} {precision}] MPJPE vs reference {mp * 1e3:.5f} mm")
    assert mp <= (MPJPE_TOL_M if precision != "bf16" else BF16_MPJPE_TOL_M)
    total.backward()
    if precision == "fp32":
        close(poses, fx["poses"], rtol=1e-4, atol=2e-5)
        np.testing.assert_allclose(total.item(), float(fx["loss_total"]), rtol=1e-4)
        _check_grads(model, fx)
    else:
        cs = {k: _cos(p.grad.cpu(), torch.from_numpy(fx["g::" + k])) for k, p in model.named_parameters()}
        worst = min(cs.items(), key=lambda kv: kv[1])
        assert worst[1] > 0.98, worst


def test_mup_training_entry_and_muadam_step(lib, tmp_path, monkeypatch):
    """hpe/main_h36m_lifting.py model.mup=true: base shapes (64 / 27 vs 128 / 81 as main_h36m_lifting.py:681-693), muP re-initialisation,
    MuAdam multipliers in the fused Adam; one scaled Adam step against torch.optim.Adam with the same per-parameter groups."""
    import os, sys
    from manipose_amd.mup_lite import mup_lr_multipliers
    from manipose_amd.optim import FusedAdam
    from test_host_cpu import _mup_model
    fx = load_fixture("mup_manifold")
    model = _mup_model(fx).cuda()
    mult = mup_lr_multipliers(model)
    ref_params = {k: torch.from_numpy(fx["w::" + k]).clone().requires_grad_(True) for k in mult}
    groups = [{"params": [ref_params[k]], "lr": 1e-3 * lm, "weight_decay": 1e-2 * wm} for k, (lm, wm) in mult.items()]
    ref = torch.optim.Adam(groups, lr=1e-3, weight_decay=1e-2)
    for k, p in model.named_parameters():
        g = torch.from_numpy(fx["g::" + k])
        p.grad = g.cuda()
        ref_params[k].grad = g.clone()
    opt = FusedAdam(model, lr=1e-3, weight_decay=1e-2)
    opt.set_multipliers(mult)
    opt.step()
    ref.step()
    for k, p in model.named_parameters():
        close(p.detach(), ref_params[k].detach(), rtol=1e-5, atol=1e-7, msg=k)
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "hpe"))
    from _entry import run
    monkeypatch.chdir(tmp_path)
    best = run(["model.mup=true", "train.epochs=1", "train.steps_per_epoch=2", "train.batch_size=2", "train.batch_size_test=2", "data.seq_len=27",
                "model.channels=128", "model.layers=2", "model.nheads=4", "model.channels_seg=64", "model.layers_seg=1", "model.nheads_seg=4",
                "multi_hyp.n_hyp=2", "data.synthetic_sequences=4", "run.test=false", "model.arch=manifold"])
    assert np.isfinite(best)


def test_deep_bones_net_draws_more_than_48_droppath_branches(lib):
    """4 (layers + layers_seg) DropPath branches: 56 with layers=8, layers_seg=6 (the mask kernel takes 48 descriptors per launch)."""
    from manipose_amd import RMCLManifoldMixSTE, h36m_skeleton
    torch.manual_seed(3)
    model = RMCLManifoldMixSTE(h36m_skeleton(), num_frame=9, embed_dim_rot=32, depth_rot=8, num_heads_rot=4, embed_dim_seg=16, depth_seg=6,
                               num_heads_seg=4, n_hyp=2, drop_path_rate=0.3).cuda().train()
    X = torch.randn(4, 9, 17, 2, device="cuda")
    with torch.no_grad():
        poses, scores = model(X)
        masks = model._engine.peek(2)
    layout = model._engine.mask_layout(4)
    assert len(layout) == 56 and torch.isfinite(poses).all()
    for name, off, cnt, keep in layout[-4:]:                       # the last branches (beyond descriptor 48) were drawn, not left at zero
        seg = masks[off:off + cnt]
        assert set(torch.unique(seg).tolist()) <= {0.0, float(np.float32(1.0 / keep))} and cnt > 0, name
    assert bool((masks[layout[52][1]:layout[55][1] + layout[55][2]] > 0).any())


@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
def test_config2_T27_K1_single_hypothesis_full_width_vs_oracle(lib, precision):
    """BASELINE config #2: H36M lifting T=27 J=17 K=1 (ManifoldMixSTE) at FULL width (C=512, depth 8; bones net C=128, depth 2), B=3, against
    the fp32 CPU oracle: poses inside the north-star bound in fp32 and in the split precision, loss, parameter gradients."""
    from manipose_amd import ManifoldMixSTE, h36m_skeleton
    from manipose_amd.metrics import manifold_training_loss, mpjpe_error
    cfg = dict(orc.FULL_CFG, T=27, n_hyp=0)
    st_ = orc.make_state(cfg, seed=11)
    model = ManifoldMixSTE(h36m_skeleton(), num_frame=27, drop_path_rate=0.0)
    model.load_state_dict(st_, strict=True)
    model.precision = precision
    model = model.cuda().eval()
    X, y = orc.synthetic_batch(3, 27, seed=12)
    pred = model(X.cuda())
    req = {k: v.clone().requires_grad_(True) for k, v in st_.items()}
    o_pred = orc.manifold_forward(X, req, orc.oracle_cfg(cfg))
    mp = mpjpe_error(pred, o_pred.detach().cuda(), "average").item()
    print(f"\n[config #2 T=27 K=1 {precision}] MPJPE vs oracle {mp * 1e3:.5f} mm")
    assert mp <= MPJPE_TOL_M and pred.shape == (3, 27, 17, 3) and bool((pred[..., 0, :] == 0).all())
    total, _ = manifold_training_loss(pred, y.cuda())
    o_total, _ = orc.manifold_training_loss(o_pred, y)
    np.testing.assert_allclose(total.item(), o_total.item(), rtol=1e-4 if precision == "fp32" else 1e-3)
    total.backward()
    o_total.backward()
    if precision == "fp32":
        bad = [(k, ((p.grad.cpu() - req[k].grad).abs().max() / (req[k].grad.abs().max() + 1e-12)).item()) for k, p in model.named_parameters()]
        assert max(e for _, e in bad) <= 5e-3, sorted(bad, key=lambda t: -t[1])[:3]
    else:
        cs = [_cos(p.grad.cpu(), req[k].grad) for k, p in model.named_parameters() if req[k].grad.abs().max() > 0]
        print(f"\n[bf16x3 drift] config #2: worst gradient cosine {min(cs):.6f}")
        assert min(cs) > 0.9995, min(cs)


def test_stream_hazard_check_of_the_three_stream_engine(lib):
    """mp_model_config::debug bit 0 (csrc/hazard.h): every launch of a forward + backward declares its stream and the bytes it reads / writes, the
    engine's event records / waits are mirrored, and a vector clock per stream must find every conflicting cross-stream pair ordered - for the
    rotations net on the caller's stream, the segments net on the side stream and the weight gradients / parameter reductions on the third
    stream, in every precision, over two training steps (the second step's forward meets the first step's backward), with DropPath masks.
    Results are those of a model without the check."""
    from manipose_amd import RMCLManifoldMixSTE, h36m_skeleton
    from manipose_amd.metrics import rmcl_training_loss
    g = torch.Generator(device="cuda").manual_seed(5)
    X = (0.3 * torch.randn(3, 27, 17, 2, device="cuda", generator=g)).clamp(-1, 1)
    y = 0.3 * torch.randn(3, 27, 17, 3, device="cuda", generator=g)
    for precision in ("bf16x3", "bf16", "fp32"):
        grads = {}
        for check in (True, False):
            torch.manual_seed(11)
            m = RMCLManifoldMixSTE(h36m_skeleton(), num_frame=27, embed_dim_rot=128, depth_rot=3, num_heads_rot=8, embed_dim_seg=64, depth_seg=2,
                                   num_heads_seg=4, n_hyp=3, drop_path_rate=0.1)
            m.precision, m.hazard_check = precision, check
            m = m.cuda().train()
            for step in range(2):
                m.zero_grad(set_to_none=True)
                poses, scores = m(X)
                total, _ = rmcl_training_loss(poses, scores, y)
                total.backward()
            torch.cuda.synchronize()
            grads[check] = torch.cat([p.grad.reshape(-1) for p in m.parameters()]).clone()
            if check:
                rep = m._engine.hazard_report()
                assert rep["violations"] == 0, "\n".join(rep["messages"][:8])
                # the check did see the engine's concurrency: hundreds of launches, event edges, and conflicting cross-stream pairs that ARE ordered
                assert rep["launches"] > 300 and rep["events"] > 40 and rep["ordered_pairs"] > 100, rep
                print(precision, {k: v for k, v in rep.items() if k != "messages"})
            else:
                with pytest.raises(RuntimeError, match="debug bit 0"):
                    m._engine.hazard_report()
        assert torch.equal(grads[True], grads[False])
    # MuReadout (readout multiplier != 1): the heads' weight gradients land in a zeroed scratch (memset on the caller's stream) that the
    # parameter kernels fill on the weight-gradient stream and a flush adds to the gradient buffer - declared to the tracker since round 6
    from test_host_cpu import _mup_model
    from manipose_amd.metrics import rmcl_training_loss as rloss
    fx = load_fixture("mup_rmcl")
    mm = _mup_model(fx)
    mm.precision, mm.hazard_check = "bf16x3", True
    mm = mm.cuda().train()
    Xm, ym = dev(fx["X"]), dev(fx["y"])
    for step in range(2):
        mm.zero_grad(set_to_none=True)
        pm, sm = mm(Xm)
        rloss(pm, sm, ym)[0].backward()
    torch.cuda.synchronize()
    rep = mm._engine.hazard_report()
    assert rep["violations"] == 0, "\n".join(rep["messages"][:8])
    print("mup_rmcl bf16x3", {k: v for k, v in rep.items() if k != "messages"})


def test_backward_after_an_in_place_parameter_update_is_refused(lib):
    """autograd's saved-tensor version check for the fused module: the engine reads the parameters again in its backward (and in the re-run
    forward of a delayed backward), so an optimizer step or load_state_dict between a forward and its backward must raise, not yield the
    gradients of a different graph."""
    from manipose_amd import RMCLManifoldMixSTE, h36m_skeleton
    from manipose_amd.optim import FusedAdam
    torch.manual_seed(0)
    m = RMCLManifoldMixSTE(h36m_skeleton(), num_frame=9, embed_dim_rot=32, depth_rot=2, num_heads_rot=4, embed_dim_seg=16, depth_seg=1,
                           num_heads_seg=4, n_hyp=2, drop_path_rate=0.0).cuda().train()
    opt = FusedAdam(m, lr=1e-3)
    x = torch.randn(2, 9, 17, 2, device="cuda")
    p, s = m(x)
    p.square().sum().backward()
    opt.step()                                                   # ordinary order: fine
    p1, _ = m(x)
    opt.step()                                                   # fused update between the forward and its backward
    with pytest.raises(RuntimeError, match="modified in place"):
        p1.square().sum().backward()
    p2, _ = m(x)
    with torch.no_grad():
        next(m.parameters()).mul_(1.0)                           # torch-side in-place write (what load_state_dict does)
    with pytest.raises(RuntimeError, match="modified in place"):
        p2.square().sum().backward()
    p3, _ = m(x)
    p4, _ = m(x)                                                 # two forwards, delayed backward of the first with unchanged parameters: still fine
    (p3.square().sum() + p4.square().sum()).backward()


def test_trainer_reads_the_fp16_backward_health_counters(lib):
    """LiftingTrainer on an f16_backward model sums the saturation counters of every backward on the device and raises at its check interval
    when the fp16 gradient operands were clamped - driven here by a gradient scale far beyond the fp16 range (a loss weight of 1e9)."""
    from manipose_amd import RMCLManifoldMixSTE, h36m_skeleton
    from manipose_amd.training import LiftingTrainer
    torch.manual_seed(0)
    def build():
        m = RMCLManifoldMixSTE(h36m_skeleton(), num_frame=27, embed_dim_rot=256, depth_rot=2, num_heads_rot=4, embed_dim_seg=32, depth_seg=1,
                               num_heads_seg=4, n_hyp=2, drop_path_rate=0.0)
        m.precision, m.f16f8, m.f16_backward = "bf16x3", 1, True
        return m.cuda().train()
    X = (0.3 * torch.randn(4, 27, 17, 2, device="cuda")).clamp(-1, 1)
    y = 0.3 * torch.randn(4, 27, 17, 3, device="cuda")
    tr = LiftingTrainer(build(), lr=1e-5, health_interval=2)
    for _ in range(4):
        tr.train_step(X, y)                                      # healthy gradients: the per-backward scale keeps them inside fp16
    assert tr.saturation_events == 0
    # a backward whose interior gradients leave the window the scale was chosen for: the velocity term weighted 1e12 against a scale taken
    # from the residual gradient is still covered by S (S adapts) - so drive the counters directly through a non-finite target instead
    y_bad = y.clone(); y_bad[0, 0, 1, 0] = float("inf")
    tr2 = LiftingTrainer(build(), lr=1e-5, health_interval=1, on_saturation="raise")
    with pytest.raises(RuntimeError, match="fp16 gradient operands"):
        tr2.train_step(X, y_bad)
    tr3 = LiftingTrainer(build(), lr=1e-5, health_interval=1, on_saturation="warn")
    with pytest.warns(UserWarning, match="fp16 gradient operands"):
        tr3.train_step(X, y_bad)
    assert tr3.saturation_events > 0

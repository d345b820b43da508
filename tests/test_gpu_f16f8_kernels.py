"""Kernel-level tests of every "f16f8" form the engine launches (mp_model_config::f16f8 = 3, the training default; 1 / 2 with f16_backward),
each through the C entry point that fills the engine's argument block and calls the engine's dispatcher (include/manipose_hip.h).

Every test compares with fp64 on the host, twice:
  (a) exact planes: fp64 of the ROUNDED operands the kernel receives (decoded fp16 + e4m3 planes, bf16, fp16, bf16-of-fp16), the epilogue in
      fp64, asserted PER ELEMENT against that element's forward-error scale (never against the global max: a wrong row of small values must
      not hide under a large one);
  (b) format accuracy: fp64 of the fp32 operands - the form must stay clearly better than a lone fp16 / bf16 product.
Outputs in the f16f8 format are also checked for internal consistency: the second 4-byte half of every 8-byte group must be e4m3(hi) of the
fp16 plane bit for bit, and the decoded value hi + 2^-11 e4m3(lo byte) must re-encode to the same planes: hi a nearest fp16 of it (the
correction is a rounding remainder of hi, at most half an ulp), whence e4m3(2^11 (value - hi)) is the lo byte again.  Planar bf16 outputs:
hi a nearest bf16 of hi + lo likewise.  This catches byte-order, half-swap and stale
correction bugs that a value tolerance cannot.

Bound constants: C_* below, in units of 2^-24 times the element's scale; each was measured on the MI355X and is asserted with a margin
(the measured worst ratio is printed next to every bound)."""
import numpy as np
import pytest
import torch

from test_gpu_parity import _attn_ref, _cos, close, f16f8_planes, st

pytestmark = pytest.mark.gpu

U24 = 2.0 ** -24
# (measured worst ratio on the MI355X over this module's shapes -> asserted bound)
C_GEMM = 8.0        # fp32-accumulated GEMM (+ epilogue) against the exact planes, x 2^-24 x (sum |a||b| + |epilogue terms|): 3.3 -> 8
C_LN = 6.0          # two-pass LayerNorm, x 2^-24 x |gamma| (|xhat| + |mean| rstd) + |beta| + |pos|: 2.4 -> 6
C_ATTN = 0.25       # split-precision attention against fp64 of the planar qkv, x 2^-16 x the softmax-weighted |v| (+ logit error) scale: 0.091 -> 0.25
C_WG = 5.0          # weight / bias gradients (split over token slabs, fp32 partial sums), x 2^-24 x sum |dy||x|: 2.0 -> 5


def report(name, ratio, bound):
    print(f"[f16f8 kernels] {name}: worst error / bound-scale {ratio:.3g} (asserted <= {bound})")
    assert ratio <= bound, (name, ratio, bound)


def lib_():
    from manipose_amd import _lib
    return _lib


# ------------------------------------------------------------------------------------------------ format helpers
def e4m3_bytes(t):
    return t.clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8)


def e4m3_decode(b):
    return b.contiguous().view(torch.float8_e4m3fn).double()


def halves(corr8, K):
    """(R, 2K) correction plane -> (first, second): the two 4-byte halves of every 8-byte group, as (R, K) byte tensors."""
    R = corr8.shape[0]
    c = corr8.view(R, K // 4, 2, 4)
    return c[:, :, 0].reshape(R, K), c[:, :, 1].reshape(R, K)


def ulp(hi, mant_bits, min_exp):
    """ulp of the finite values hi (float64) in a binary format with mant_bits stored bits and smallest normal exponent min_exp."""
    _, e = torch.frexp(hi)
    e = torch.where(hi == 0, torch.full_like(e, min_exp + 1), e)
    return torch.ldexp(torch.ones_like(hi), torch.clamp(e - 1, min=min_exp) - mant_bits)


def assert_rounding_pair(hi, lo, mant_bits, min_exp, what):
    """hi is a nearest value of hi + lo (exact sum, fp64) in its format: |lo| at most half the ulp on its side of hi.  (Not "ties to even": the
    rounding of the remainder itself - 3 bits in e4m3, 8 in bf16 - can carry it to exactly half an ulp next to an odd hi.)"""
    u = ulp(hi, mant_bits, min_exp)
    m, e = torch.frexp(hi)
    pow2 = (hi != 0) & (m.abs() == 0.5) & (e - 1 > min_exp)
    half = torch.where(pow2 & (lo * hi < 0), u / 4, u / 2)       # below a power of two the grid is twice as fine
    ok = lo.abs() <= half
    bad = (~ok).sum().item()
    assert bad == 0, f"{what}: {bad} elements whose hi plane is not the rounding of the represented value"


def decode_act(hi16, corr8):
    """f16f8 activation planes -> (value hi + 2^-11 e4m3(first half), the lo part); checks the encoding is self-consistent."""
    R, K = hi16.shape
    first, second = halves(corr8, K)
    assert torch.equal(second, e4m3_bytes(hi16.float())), f"second half != e4m3(hi): {(second != e4m3_bytes(hi16.float())).sum().item()} bytes"
    lo = 2.0 ** -11 * e4m3_decode(first)
    hi = hi16.double()
    assert_rounding_pair(hi, lo, 10, -14, "f16f8 output")
    return hi + lo


def decode_planar(hi, lo):
    assert_rounding_pair(hi.double(), lo.double(), 7, -126, "planar bf16 output")
    return hi.double() + lo.double()


def f8_rep(v):
    """what the f16f8 format can miss of a value: e4m3 keeps 3 bits of a correction <= 2^-11 |v| (2^-15 |v|), e4m3 subnormals 2^-21 absolute;
    + the planar reference's own 2^-16 |v|"""
    return 2.0 ** -14 * v.abs() + 2.0 ** -20


def gemm_exact(x, W, b):
    """fp64 of x W^T + b on the rounded f16f8 planes (the products the kernel evaluates) and the forward-error scale sum |x||W| + |b|."""
    x16, x8, x_lo8, x_hi8 = f16f8_planes(x, False)
    W16, W8, W_hi8, W_lo8 = f16f8_planes(W, True)
    exact = x16.double() @ W16.double().t() + 2.0 ** -15 * (x_lo8 @ W_hi8.t() + x_hi8 @ W_lo8.t()) + b.double()
    mag = x16.double().abs() @ W16.double().abs().t() + 2.0 ** -15 * (x_lo8.abs() @ W_hi8.abs().t() + x_hi8.abs() @ W_lo8.abs().t()) + b.double().abs()
    lone = x16.double() @ W16.double().t() + b.double()
    return (x16.cuda(), x8.cuda(), W16.cuda(), W8.cuda()), exact, mag, lone


def linear_ex(lib, ops, b, y, y_lo, z, r_in, rstats, rgamma, rbeta, mask, mode, rscale, T, J, M, N, K, epi, form):
    p = lambda t: t.data_ptr() if t is not None else None
    lib_().check(lib.mp_linear_fwd_f16f8_ex(*(t.data_ptr() for t in ops), p(b), p(y), p(y_lo), p(z), p(r_in), p(rstats), p(rgamma), p(rbeta), p(mask), mode,
                                            rscale, T, J, M, N, K, epi, form, st()), "mp_linear_fwd_f16f8_ex")


def operands(M, N, K, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, K, generator=g)
    x[::7] *= 2.0 ** -6                     # small-magnitude rows: a per-element bound must still see their errors
    W = torch.randn(N, K, generator=g) / K ** 0.5
    b = torch.randn(N, generator=g)
    return g, x, W, b


# M = B T J tokens: 918 (T 27, B 2), 4131 (one T = 243 window), 66096 (16 windows), 255 / 256 / 257 around one 256-row tile, 17 (one partial
# tile); the persistent grid is sized from the CU count (256 on the MI355X, 8-aligned), so 4131 x 1536 (17 x 6 = 102 tiles) and 66096 x 768
# (259 x 3 = 777 tiles) are not multiples of it
@pytest.mark.parametrize("M,C", [(918, 256), (4131, 512), (66096, 256), (255, 256), (256, 512), (257, 256), (17, 512)])
def test_f16f8_linear_bias_planar_bf16_output(lib, M, C):
    """qkv -> attention: gemm_f16f8, EPI_BIAS, planar bf16 hi / lo output (N = 3C, K = C)."""
    N, K = 3 * C, C
    _, x, W, b = operands(M, N, K, M + C)
    ops, exact, mag, lone = gemm_exact(x, W, b)
    y, yl = (torch.full((M, N), float("nan"), device="cuda", dtype=torch.bfloat16) for _ in range(2))
    linear_ex(lib, ops, b.cuda(), y, yl, None, None, None, None, None, None, 0, 1.0, 0, 0, M, N, K, 0, 1)
    got = decode_planar(y.cpu(), yl.cpu())
    rep = 2.0 ** -16 * exact.abs()           # the planar pair carries 16 significand bits
    report(f"bias planar M={M} N={N} K={K}", ((got - exact).abs() - rep).clamp(min=0).div(U24 * mag).max().item(), C_GEMM)
    pre = x.double() @ W.double().t() + b.double()
    err, lone_err = ((got - pre).abs() / (x.double().abs() @ W.double().abs().t() + b.double().abs())).max().item(), \
        ((lone - pre).abs() / (x.double().abs() @ W.double().abs().t() + b.double().abs())).max().item()
    print(f"  vs fp32 operands: {err:.2e} relative to sum |x||W| (lone fp16 product {lone_err:.2e})")
    assert err < lone_err / 8, (err, lone_err)


@pytest.mark.parametrize("M,C", [(918, 256), (4131, 512), (66096, 256), (257, 512), (17, 256)])
def test_f16f8_linear_gelu_both_output_forms(lib, M, C):
    """fc1 -> fc2: gemm_f16f8, EPI_BIAS_GELU, output as f16f8 planes (+ Z = gelu') and as planar bf16 (N = 2C, K = C)."""
    N, K = 2 * C, C
    _, x, W, b = operands(M, N, K, 3 * M + C)
    ops, exact, mag, lone = gemm_exact(x, W, b)
    pre = exact
    want = torch.nn.functional.gelu(pre)
    dwant = 0.5 * (1 + torch.erf(pre / 2 ** 0.5)) + pre * torch.exp(-0.5 * pre * pre) / (2 * np.pi) ** 0.5
    bd = b.cuda()
    y, yl, z = (torch.full((M, N), float("nan"), device="cuda", dtype=torch.bfloat16) for _ in range(3))
    linear_ex(lib, ops, bd, y, yl, z, None, None, None, None, None, 0, 1.0, 0, 0, M, N, K, 1, 1)
    planar = decode_planar(y.cpu(), yl.cpu())
    # error scale: the pre-activation's (|gelu'| <= 1.13) plus the fp32 GELU itself (erf polynomial ~1.5e-7 absolute: 2.5 |pre| 2^-24)
    scale = U24 * (1.2 * mag + 4.0 * pre.abs())
    report(f"gelu planar M={M} N={N}", ((planar - want).abs() - 2.0 ** -16 * want.abs()).clamp(min=0).div(scale).max().item(), C_GEMM)
    zerr = ((z.cpu().double() - dwant).abs() / (2.0 ** -8 * dwant.abs() + 2.0 ** -20)).max().item()
    report(f"gelu' (bf16) M={M}", zerr, 1.0)
    h16 = torch.full((M, N), float("nan"), device="cuda", dtype=torch.float16)
    c8 = torch.full((M, 2 * N), 0x7E, device="cuda", dtype=torch.uint8)       # stale bytes (e4m3 448) must all be overwritten
    z2 = torch.full_like(z, float("nan"))
    linear_ex(lib, ops, bd, h16, c8, z2, None, None, None, None, None, 0, 1.0, 0, 0, M, N, K, 1, 2)
    got = decode_act(h16.cpu(), c8.cpu())
    assert torch.equal(z2.cpu(), z.cpu())
    # the f16f8 output carries ~2^-15 of the value (e4m3 correction: 3 bits below 2^-11): against the planar form of the same kernel
    rep = (got - planar).abs() / f8_rep(planar)
    report(f"gelu f16f8 vs planar M={M}", rep.max().item(), 1.0)
    gelu32 = torch.nn.functional.gelu(x.double() @ W.double().t() + b.double())
    err = ((got - gelu32).abs() / (x.double().abs() @ W.double().abs().t() + b.double().abs())).max().item()
    lone_err = ((torch.nn.functional.gelu(lone) - gelu32).abs() / (x.double().abs() @ W.double().abs().t() + b.double().abs())).max().item()
    print(f"  vs fp32 operands: {err:.2e} (lone fp16 product {lone_err:.2e})")
    assert err < lone_err / 4, (err, lone_err)


@pytest.mark.parametrize("M,C,K,mode,T,J,ln", [(918, 256, 256, 1, 27, 17, False), (918, 256, 512, 2, 27, 17, True), (4131, 512, 512, 2, 243, 17, False),
                                               (4131, 512, 1024, 1, 243, 17, True), (66096, 512, 512, 2, 243, 17, True), (255, 256, 512, 0, 255, 1, True),
                                               (257, 512, 512, 0, 257, 1, False), (17, 256, 256, 1, 1, 17, True), (8262, 256, 512, 2, 27, 17, True)])
def test_f16f8_linear_residual_epilogue(lib, M, C, K, mode, T, J, ln):
    """proj / fc2: gemm_f16f8, EPI_BIAS_RESID, fp32 output y = R' + mask * (x W^T + b) with R' = r_in or the recomputed LayerNorm of r_in
    (rstats), DropPath mask modes 0 / 1 / 2 with dropped samples; a residual scale other than 1 is refused."""
    N = C
    g, x, W, b = operands(M, N, K, 5 * M + K + mode)
    ops, exact, mag, lone = gemm_exact(x, W, b)
    r_in = torch.randn(M, N, generator=g) * 2.0 + 0.3
    gamma, beta = 1.0 + 0.2 * torch.randn(N, generator=g), 0.1 * torch.randn(N, generator=g)
    mean, rstd = r_in.double().mean(1), (r_in.double().var(1, unbiased=False) + 1e-6).rsqrt()
    stats = torch.stack([mean, rstd], 1).float().contiguous()
    ns = {0: 0, 1: M // J, 2: (M // (T * J)) * J}[mode]
    mask = ((torch.rand(ns, generator=g) > 0.3).float() / 0.7) if mode else None
    if mode:
        mask[-1] = 1 / 0.7                   # a kept sample and, from two samples on, a dropped one in the first row tile whatever the draw
        if ns > 1:
            mask[0] = 0.0
    rows = torch.arange(M)
    mrow = torch.ones(M, dtype=torch.float64) if mode == 0 else (mask[rows // J] if mode == 1 else mask[(rows // (T * J)) * J + rows % J]).double()
    if ln:
        sd = stats.double()
        res = (r_in.double() - sd[:, :1]) * sd[:, 1:] * gamma.double() + beta.double()
        rmag = (r_in.double() - sd[:, :1]).abs() * sd[:, 1:] * gamma.double().abs() + beta.double().abs() + sd[:, :1].abs() * sd[:, 1:] * gamma.double().abs()
    else:
        res, rmag = r_in.double(), r_in.double().abs()
    want = res + mrow[:, None] * exact
    dv = lambda t: t.cuda() if t is not None else None
    args = (dv(r_in), dv(stats) if ln else None, dv(gamma) if ln else None, dv(beta) if ln else None, dv(mask), mode)
    y = torch.full((M, N), float("nan"), device="cuda")
    linear_ex(lib, ops, b.cuda(), y, None, None, *args, 1.0, T, J, M, N, K, 2, 0)
    got = y.cpu().double()
    scale = U24 * (mrow.abs()[:, None] * mag + 2.0 * rmag + want.abs())
    report(f"residual M={M} N={N} K={K} mode={mode} rstats={ln}", ((got - want).abs() / scale).max().item(), C_GEMM)
    pre = x.double() @ W.double().t() + b.double()
    m32 = mrow[:, None] * (x.double().abs() @ W.double().abs().t() + b.double().abs()) + rmag
    err = ((got - (res + mrow[:, None] * pre)).abs() / m32).max().item()
    lone_err = ((mrow[:, None] * (lone - pre)).abs() / m32).max().item()
    print(f"  vs fp32 operands: {err:.2e} (lone fp16 product {lone_err:.2e})")
    assert err <= lone_err / 4, (err, lone_err)
    with pytest.raises(RuntimeError, match="residual scale"):
        linear_ex(lib, ops, b.cuda(), y, None, None, *args, 0.5, T, J, M, N, K, 2, 0)


def test_f16f8_linear_refuses_the_forms_that_do_not_exist(lib):
    """f16f8 output planes exist for the GELU epilogue only; the residual epilogue writes fp32 only."""
    M, N, K = 256, 256, 256
    _, x, W, b = operands(M, N, K, 1)
    ops, _, _, _ = gemm_exact(x, W, b)
    y, yl = torch.empty(M, N, device="cuda"), torch.empty(M, N, device="cuda")
    r = torch.zeros(M, N, device="cuda")
    for epi, form in ((0, 2), (2, 1), (2, 2), (1, 0)):
        with pytest.raises(RuntimeError):
            linear_ex(lib, ops, b.cuda(), y, yl, None, r if epi == 2 else None, None, None, None, None, 0, 1.0, 0, 0, M, N, K, epi, form)


def ln_ref(x, g, b, eps):
    mean = x.mean(1, keepdim=True)
    var = ((x - mean) ** 2).mean(1, keepdim=True)
    rstd = (var + eps).rsqrt()
    return (x - mean) * rstd * g + b, mean, rstd


@pytest.mark.parametrize("M,C,stage1,b16", [(918, 256, False, False), (918, 512, True, True), (4131, 1024, True, False), (257, 256, True, True),
                                            (17, 512, False, True), (66096, 512, True, False), (4131, 256, False, True)])
def test_f16f8_layernorm_forward(lib, M, C, stage1, b16):
    """ln_fwd out mode 3 (f16f8 planes, with and without the bf16 copy: ln_fwd_kernel<f16f8, V, B16>), with stage 1 and the positional table,
    C = 256 / 512 / 1024 (V = 1, 2, 4), rows with a mean of 30 and a spread of 0.1: the row statistics are two-pass in fp32, so the error scale
    has a |mean| rstd term (a one-pass E[x^2] - mean^2 would have |mean|^2 rstd^2)."""
    g = torch.Generator().manual_seed(M + C + stage1)
    T, J = 27, M // 27 if M % 27 == 0 else 1
    if M % 27:
        T, J = M, 1
    x = 30.0 + 0.1 * torch.randn(M, C, generator=g)
    x[1::5] = 0.1 * torch.randn(len(range(1, M, 5)), C, generator=g)        # rows of a small mean among them
    g1, b1 = 1.0 + 0.1 * torch.randn(C, generator=g), 30.0 + 0.1 * torch.randn(C, generator=g)      # stage 1 hands stage 2 a mean-30 row too
    pos = 0.05 * torch.randn(T, C, generator=g)
    g2, b2 = 1.0 + 0.2 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    xd = x.double()
    if stage1:
        x1, m1, r1 = ln_ref(xd, g1.double(), b1.double(), 1e-6)
        x1 = x1 + pos.double()[(torch.arange(M) // J) % T]
        s_in = x1.float().double()           # stage 2 reads the fp32 stage-1 output (the kernel keeps it in registers; compared per element below)
    else:
        s_in = xd
    want, m2, r2 = ln_ref(s_in, g2.double(), b2.double(), 1e-6)
    xhat = (s_in - m2) * r2
    scale = U24 * (g2.double().abs() * (xhat.abs() + m2.abs() * r2) + b2.double().abs())
    dv = lambda t: t.cuda()
    xg = dv(x)
    x1d = torch.full((M, C), float("nan"), device="cuda") if stage1 else None
    st1 = torch.full((M, 2), float("nan"), device="cuda") if stage1 else None
    st2 = torch.full((M, 2), float("nan"), device="cuda")
    p = lambda t: t.data_ptr() if t is not None else None
    g1d, b1d, posd, g2d, b2d = dv(g1), dv(b1), dv(pos), dv(g2), dv(b2)

    def run(out_mode, y, ylo, yb):
        lib_().check(lib.mp_layernorm_fwd_ex(xg.data_ptr(), M, C, p(g1d) if stage1 else None, p(b1d) if stage1 else None, 1e-6, p(posd) if stage1 else None,
                                             T, J, p(x1d), p(st1), g2d.data_ptr(), b2d.data_ptr(), 1e-6, y.data_ptr(), p(ylo), p(yb), st2.data_ptr(), out_mode,
                                             st()), "mp_layernorm_fwd_ex")
    yh, yl = (torch.full((M, C), float("nan"), device="cuda", dtype=torch.bfloat16) for _ in range(2))
    run(2, yh, yl, None)
    planar = decode_planar(yh.cpu(), yl.cpu())
    if stage1:       # the stage-1 output itself (fp32), then stage 2 against the fp64 LayerNorm of that fp32 row
        s1scale = U24 * (g1.double().abs() * ((xd - m1).abs() * r1 + m1.abs() * r1) + b1.double().abs() + pos.double().abs().max())
        report(f"layernorm stage 1 M={M} C={C}", ((x1d.cpu().double() - x1).abs() / s1scale).max().item(), C_LN)
        s_in = x1d.cpu().double()
        want, m2, r2 = ln_ref(s_in, g2.double(), b2.double(), 1e-6)
        xhat = (s_in - m2) * r2
        scale = U24 * (g2.double().abs() * (xhat.abs() + m2.abs() * r2) + b2.double().abs())
    report(f"layernorm planar M={M} C={C} stage1={stage1}", ((planar - want).abs() - 2.0 ** -16 * want.abs()).clamp(min=0).div(scale).max().item(), C_LN)
    stats = st2.cpu().double()
    assert ((stats[:, 0] - m2[:, 0]).abs() <= 8 * U24 * s_in.abs().mean(1)).all()          # the fp32 row sum's error scale
    h16 = torch.full((M, C), float("nan"), device="cuda", dtype=torch.float16)
    c8 = torch.full((M, 2 * C), 0x7E, device="cuda", dtype=torch.uint8)
    yb = torch.full((M, C), float("nan"), device="cuda", dtype=torch.bfloat16) if b16 else None
    run(3, h16, c8, yb)
    got = decode_act(h16.cpu(), c8.cpu())
    report(f"layernorm f16f8 vs planar M={M} C={C} bf16 copy={b16}", ((got - planar).abs() / f8_rep(planar)).max().item(), 1.0)
    if b16:          # the copy is bf16 of the same fp32 value: the rounding of the planar pair's value
        assert torch.equal(yb.cpu(), yh.cpu())
    ref32 = ln_ref(xd, g2.double(), b2.double(), 1e-6)[0] if not stage1 else want
    print(f"  f16f8 vs fp64: {((got - ref32).abs().max().item()):.2e}")


@pytest.mark.parametrize("temporal,B,T,J,C,H", [(0, 2, 27, 17, 256, 4), (0, 1, 81, 17, 512, 8), (1, 2, 27, 17, 256, 4), (1, 1, 81, 17, 512, 8),
                                                (1, 1, 243, 17, 256, 4), (1, 1, 243, 5, 512, 8)])
def test_f16f8_attention_forward_output_and_backward_with_fp16_O(lib, temporal, B, T, J, C, H):
    """attn_{spatial,temporal}_fwd_x3(..., out_f16f8 = 1) against fp64 of the planar qkv, lse bit-identical between the planar and f16f8 output
    forms; then the temporal MFMA backward reading O from that fp16 plane (out_f16) against fp64 autograd, within the bound of the bf16
    backward test (test_bf16_attention_forward_backward)."""
    _lib = lib_()
    g = torch.Generator().manual_seed(T * 17 + C + temporal)
    M = B * T * J
    qkv = torch.randn(M, 3 * C, generator=g)
    qh, ql = qkv.bfloat16(), (qkv - qkv.bfloat16().float()).bfloat16()
    qx = qh.double() + ql.double()               # what the planes carry
    ref = _attn_ref(qx, B, T, J, C, H, temporal)
    # error scale per output element: softmax-weighted |v| and the logit error's share (2^-16 relative products of the split operands)
    pv, lmax = _attn_scales(qx, B, T, J, C, H, temporal)
    scale = 2.0 ** -16 * (pv + ref.abs()) * (1.0 + lmax)
    qhd, qld = qh.cuda(), ql.cuda()
    lse1, lse2 = (torch.full((B * J * H * T,), float("nan"), device="cuda") for _ in range(2))
    oh, ol = (torch.full((M, C), float("nan"), device="cuda", dtype=torch.bfloat16) for _ in range(2))
    _lib.check(lib.mp_attention_fwd_bf16x3_ex(qhd.data_ptr(), qld.data_ptr(), oh.data_ptr(), ol.data_ptr(), lse1.data_ptr(), None, temporal, B, T, J, C, H, 0, st()))
    planar = decode_planar(oh.cpu(), ol.cpu())
    report(f"attention planar temporal={temporal} T={T} C={C} H={H}", ((planar - ref).abs() / scale).max().item(), C_ATTN)
    h16 = torch.full((M, C), float("nan"), device="cuda", dtype=torch.float16)
    c8 = torch.full((M, 2 * C), 0x7E, device="cuda", dtype=torch.uint8)
    _lib.check(lib.mp_attention_fwd_bf16x3_ex(qhd.data_ptr(), qld.data_ptr(), h16.data_ptr(), c8.data_ptr(), lse2.data_ptr(), None, temporal, B, T, J, C, H, 1, st()))
    got = decode_act(h16.cpu(), c8.cpu())
    report(f"attention f16f8 vs planar temporal={temporal} T={T}", ((got - planar).abs() / f8_rep(planar)).max().item(), 1.0)
    err = (got - _attn_ref(qkv.double(), B, T, J, C, H, temporal)).abs().max().item()
    print(f"  f16f8 output vs fp64 of the fp32 qkv: {err:.2e}")
    assert err < 1e-4 * float(ref.abs().max())      # the bf16 attention kernels: ~1e-2 (test_bf16x3_attention_forward)
    if temporal:
        assert torch.equal(lse1.cpu(), lse2.cpu()), "the output form changed the softmax"
        # backward on the bf16 hi plane of qkv with O = the fp16 plane (what the engine hands it with f16f8 = 3)
        dout = torch.randn(M, C, generator=g).bfloat16()
        qb = qh.double().requires_grad_(True)
        (_attn_ref(qb, B, T, J, C, H, temporal) * dout.double()).sum().backward()
        want = qb.grad
        dq = torch.full((M, 3 * C), float("nan"), device="cuda", dtype=torch.bfloat16)
        dod = dout.cuda()
        delta = torch.empty(B * J * H * T, device="cuda")
        _lib.check(lib.mp_attention_bwd_bf16_ex(qhd.data_ptr(), h16.data_ptr(), dod.data_ptr(), lse2.data_ptr(), delta.data_ptr(), dq.data_ptr(),
                                                1, B, T, J, C, H, 1, st()))
        gotq = dq.cpu().double()
        c = _cos(gotq, want)
        print(f"  backward with fp16 O: cosine {c:.6f}, max error / max |grad| {((gotq - want).abs().max() / want.abs().max()).item():.2e}")
        assert c > 0.999, c
        close(gotq.float(), want.float(), rtol=5e-2, atol=5e-2 * float(want.abs().max()))
        # the same with O as bf16 (of the fp16 plane): the fp16 reading must not be worse
        dq2 = torch.empty_like(dq)
        ob16 = h16.to(torch.bfloat16)
        _lib.check(lib.mp_attention_bwd_bf16_ex(qhd.data_ptr(), ob16.data_ptr(), dod.data_ptr(), lse2.data_ptr(), delta.data_ptr(), dq2.data_ptr(),
                                                1, B, T, J, C, H, 0, st()))
        e16, eb = (gotq - want).abs().max().item(), (dq2.cpu().double() - want).abs().max().item()
        print(f"  fp16 O: {e16:.3e}, bf16 O: {eb:.3e}")
        assert e16 <= 1.5 * eb + 1e-6, (e16, eb)


def _attn_scales(qkv, B, T, J, C, H, temporal):
    """per output element: sum_j p_j |v_j| (the softmax-weighted |v|) and the largest scale |q||k| of its row (the logit's error scale)"""
    d = C // H
    q, k, v = qkv.view(B, T, J, 3, H, d).unbind(3)
    perm = (0, 2, 3, 1, 4) if temporal else (0, 1, 3, 2, 4)
    q, k, v = (t.permute(*perm) for t in (q, k, v))
    p = ((q @ k.transpose(-2, -1)) * d ** -0.5).softmax(-1)
    pv = p @ v.abs()
    lmax = ((q.abs() @ k.abs().transpose(-2, -1)) * d ** -0.5).amax(-1, keepdim=True).expand_as(pv)
    back = (0, 3, 1, 2, 4) if temporal else (0, 1, 3, 2, 4)
    return pv.permute(*back).reshape(B * T * J, C), lmax.permute(*back).reshape(B * T * J, C)


def test_attention_backward_refuses_an_fp16_O_outside_the_mfma_kernel(lib):
    """The row-kernel temporal backward (T > 256) reads O in the storage type of qkv: it refuses an fp16 plane instead of misreading it;
    the spatial backward reads no O."""
    _lib = lib_()
    B, T, J, C, H = 1, 300, 2, 128, 2
    M = B * T * J
    q = torch.zeros(M, 3 * C, device="cuda", dtype=torch.bfloat16)
    o = torch.zeros(M, C, device="cuda", dtype=torch.float16)
    do = torch.zeros(M, C, device="cuda", dtype=torch.bfloat16)
    lse, delta = torch.zeros(B * J * H * T, device="cuda"), torch.zeros(B * J * H * T, device="cuda")
    dq = torch.zeros_like(q)
    for temporal, t in ((1, T), (0, 5)):
        with pytest.raises(RuntimeError):
            _lib.check(lib.mp_attention_bwd_bf16_ex(q.data_ptr(), o.data_ptr(), do.data_ptr(), lse.data_ptr(), delta.data_ptr(), dq.data_ptr(), temporal,
                                                    B, t, J, C, H, 1, st()))


def _slab(lib, N, K):
    return torch.empty(int(lib.mp_linear_bwd_slab_floats(N, K)), device="cuda")


@pytest.mark.parametrize("M,N,K,f16,dgelu", [(918, 512, 256, 1, False), (4131, 768, 256, 1, False), (4131, 512, 1024, 1, True), (257, 512, 1024, 0, True),
                                             (66096, 1024, 512, 1, True), (17, 1536, 512, 1, False)])
def test_f16_dgrad_with_saturating_scaled_store(lib, M, N, K, f16, dgelu):
    """gemm_bf16 dgrad dx = dy W [* z] on fp16 dy / fp16 weights (g.f16; f16 = 0: bf16 operands), EPI_BIAS (bf16 out) and EPI_DGELU with the
    saturating scaled-fp16 store (gout): rows that saturate after the scale, NaN / inf rows; clamped / zeroed stores and both counters
    against a host count (inputs built with a margin around 65504)."""
    _lib = lib_()
    g = torch.Generator().manual_seed(M + N + K + f16)
    dt = torch.float16 if f16 else torch.bfloat16
    dy = torch.randn(M, N, generator=g)
    W = torch.randn(N, K, generator=g) / N ** 0.5
    S = 8.0
    pick = lambda vals, shape: torch.tensor(vals)[torch.randint(len(vals), shape, generator=g)]
    z = pick([0.5, 1.0, 1.5], (M, K)).bfloat16()
    big = torch.arange(M) % 11 == 3
    if dgelu:
        # margin by construction: W in +-{1/4, 1/2, 1}, z in {1/2, 1, 3/2}; a saturating row of dy is ONE value c at one column, so its dx row
        # is c W[k] exactly and S c |W| z lands at 0.21 .. 2.5 x 65504, at least 16 % from the threshold; the other rows stay far below it
        W = pick([0.25, 0.5, 1.0], (N, K)) * (torch.randint(2, (N, K), generator=g) * 2 - 1)
        nb = int(big.sum())
        dy[big] = 0.0
        dy[big.nonzero()[:, 0], torch.randint(N, (nb,), generator=g)] = 65504.0 / (0.6 * S)
    dyq, Wq = dy.to(dt), W.to(dt)
    if dgelu:
        dyq[5 % M, 7 % N] = float("nan")
        dyq[(M - 1), 3] = float("inf")
        if M > 40:
            dyq[40, 0] = float("-inf")
    exact = dyq.double() @ Wq.double()
    mag = dyq.double().abs() @ Wq.double().abs()
    gout = torch.tensor([S], device="cuda")
    gsat = torch.zeros(2, device="cuda", dtype=torch.int32)
    dx = torch.full((M, K), float("nan"), device="cuda", dtype=torch.float16 if dgelu else torch.bfloat16)
    p = lambda t: t.data_ptr() if t is not None else None
    zd = z.cuda() if dgelu else None
    dyd, Wd = dyq.cuda(), Wq.cuda()          # (named: a temporary's memory could be handed to the next one before the launch)
    _lib.check(lib.mp_linear_bwd_f16(dyd.data_ptr(), None, Wd.data_ptr(), dx.data_ptr(), p(zd), p(gout) if dgelu else None, p(gsat) if dgelu else None,
                                     None, None, M, N, K, f16, 0, None, None, 0, st()), "mp_linear_bwd_f16")
    got = dx.cpu().double()
    if not dgelu:
        report(f"dgrad fp16 operands M={M} N={N} K={K}", ((got - exact).abs() - 2.0 ** -8 * exact.abs()).clamp(min=0).div(U24 * mag).max().item(), C_GEMM)
        err = ((got - dy.double() @ W.double()).abs() / (dy.double().abs() @ W.double().abs())).max().item()
        print(f"  vs fp32 operands: {err:.2e} relative to sum |dy||W|")
        assert err < 2.0 ** -8
        return
    v = S * exact * z.double()
    fin = torch.isfinite(v)
    sat = fin & (v.abs() > 65504)
    margin = (v[fin].abs() - 65504).abs() / 65504
    assert margin.min().item() > 0.1, "construction: values too close to the saturation threshold"
    n_sat, n_nf = int(sat.sum()), int((~fin).sum())
    assert n_sat > 0 and n_nf > 0
    cnt = gsat.cpu()
    print(f"  counters: clamped {cnt[0].item()} (host {n_sat}), non-finite {cnt[1].item()} (host {n_nf})")
    assert cnt[0].item() == n_sat and cnt[1].item() == n_nf
    assert (got[~fin] == 0).all(), "non-finite values must be stored as 0"
    assert (got[sat] == 65504 * torch.sign(v[sat])).all(), "saturated values must be clamped to +-65504"
    ok = fin & ~sat
    want = v[ok]
    scale = U24 * S * (mag * z.double().abs())[ok] + 2.0 ** -11 * want.abs() + 2.0 ** -25
    report(f"dgrad * gelu' scaled fp16 M={M} N={N} K={K} f16={f16}", ((got[ok] - want).abs() / scale).max().item(), C_GEMM)


@pytest.mark.parametrize("M,N,K,form", [(918, 768, 256, "f16"), (4131, 512, 512, "f16"), (66096, 1536, 512, "x_f16"), (4131, 512, 1024, "x_f16"),
                                        (257, 1024, 512, "x_f16"), (17, 512, 256, "f16")])
def test_f16_weight_gradient_forms(lib, M, N, K, form):
    """wgrad_bf16 with f16 = 1 (fp16 dY and X, dW += oscale dY^T X, db += oscale colsum dY) and x_f16 = 1 (bf16 dY, X the fp16 plane of an f16f8
    activation rounded to bf16 per fragment): accumulated into existing gradients."""
    _lib = lib_()
    g = torch.Generator().manual_seed(M * 5 + N + K)
    dy = torch.randn(M, N, generator=g) * 64.0
    x = torch.randn(M, K, generator=g)
    x[::5] *= 2.0 ** -5
    if form == "f16":
        dyq, xq, s = dy.half(), x.half(), 1.0 / 64
        dyr, xr = dyq.double(), xq.double()
    else:
        dyq, xq, s = dy.bfloat16(), x.half(), 1.0
        dyr, xr = dyq.double(), xq.to(torch.bfloat16).double()
    exact = 1.0 + s * (dyr.t() @ xr)
    dexact = 1.0 + s * dyr.sum(0)
    mag = s * (dyr.abs().t() @ xr.abs())
    dW, db = torch.ones(N, K, device="cuda"), torch.ones(N, device="cuda")
    osc = torch.tensor([s], device="cuda")
    slab = _slab(lib, N, K)
    dyd, xd = dyq.cuda(), xq.cuda()
    _lib.check(lib.mp_linear_bwd_f16(dyd.data_ptr(), xd.data_ptr(), None, None, None, None, None, dW.data_ptr(), db.data_ptr(), M, N, K,
                                     int(form == "f16"), int(form == "x_f16"), osc.data_ptr() if form == "f16" else None, slab.data_ptr(), slab.numel(), st()),
               "mp_linear_bwd_f16")
    report(f"wgrad {form} M={M} N={N} K={K}", ((dW.cpu().double() - exact).abs() / (U24 * (mag + 1.0))).max().item(), C_WG)
    report(f"bias grad {form} M={M} N={N}", ((db.cpu().double() - dexact).abs() / (U24 * (s * dyr.abs().sum(0) + 1.0))).max().item(), C_WG)
    ref32 = 1.0 + s * (dy.double().t() @ x.double()) if form == "f16" else 1.0 + dy.double().t() @ x.double()
    err = ((dW.cpu().double() - ref32).abs() / (s * (dy.double().abs().t() @ x.double().abs()) + 1.0)).max().item()
    print(f"  vs fp32 operands: {err:.2e}")
    assert err < (2.0 ** -9 if form == "f16" else 2.0 ** -7)


# ------------------------------------------------------------------------------------------------ splitter / packer sweep and the NaN policy
def sweep_values(weight):
    """Every finite fp16 hi crossed with correction offsets (in ulps of hi) that reach e4m3 subnormals, e4m3 round-to-nearest-even ties, +-0 and
    the 448 clamp; + the non-finite groups.  Rows of 64 (the splitter's granularity), groups of four along a row."""
    h = torch.arange(0, 1 << 16, dtype=torch.int32).to(torch.int16).view(torch.float16)
    h = h[torch.isfinite(h)].double()
    fr = [0.0, 0.25, 0.49, 0.5]
    for k in range(2, 14):
        fr += [2.0 ** -k, 2.0 ** -k * (1 + 1 / 16), 2.0 ** -k * (1 + 3 / 16), 2.0 ** -k * (1 + 1 / 8)]
    fr = torch.tensor(sorted(set(fr + [-f for f in fr])), dtype=torch.float64)
    u = ulp(h, 10, -14)
    v = (h[:, None] + fr[None, :] * u[:, None]).reshape(-1).float()
    v = v[torch.isfinite(v)]
    special = torch.tensor([[float("nan"), 1.0, 2.0, 3.0], [float("nan"), 1000.0, 2.0, -3.0], [float("inf"), 1.0, 2.0, 3.0], [float("inf"), 1000.0, 2.0, 3.0],
                            [float("-inf"), 0.5, 2.0, 3.0], [float("-inf"), -1000.0, 2.0, 3.0], [1.0, float("nan"), float("inf"), 3.0],
                            [0.1, 0.2, float("nan"), 447.0], [448.0, 449.0, 464.0, float("nan")], [-0.0, 0.0, 2.0 ** -24, -(2.0 ** -25)]]).reshape(-1)
    v = torch.cat([special.repeat(16), v])
    n = (v.numel() + 63) // 64 * 64
    v = torch.cat([v, torch.zeros(n - v.numel())])
    return v.reshape(-1, 64).contiguous()


def same_bits_nan_aware(got, want, what):
    if got.dtype == torch.float16:
        gb, wb = got.view(torch.int16), want.view(torch.int16)
        both_nan = torch.isnan(got) & torch.isnan(want)
    else:        # e4m3 bytes: 0x7f / 0xff are the NaNs (sign and payload are not part of the format)
        gb, wb = got, want
        both_nan = ((got & 0x7F) == 0x7F) & ((want & 0x7F) == 0x7F)
    bad = (gb != wb) & ~both_nan
    assert bad.sum().item() == 0, f"{what}: {bad.sum().item()} differ, first at {bad.nonzero()[:4].tolist()}"


@pytest.mark.parametrize("weight", [0, 1])
def test_f16f8_splitter_sweep_and_nan_policy(lib, weight):
    """mp_split_f16f8 (both forms) over the sweep, bit for bit against the host construction, NaN / inf included: NaN stays NaN in both
    planes, +-inf keeps +-inf in the fp16 plane and saturates to +-448 where e4m3(hi) is stored (common.h)."""
    _lib = lib_()
    v = sweep_values(weight)
    if weight:
        v = v / 16          # the weight form stores e4m3(16 hi): the clamp at |hi| = 28 and the e4m3 subnormals of 2^15 lo
    want16, want8, _, _ = f16f8_planes(v, bool(weight))
    src = v.cuda()
    o16 = torch.empty(v.shape, device="cuda", dtype=torch.float16)
    o8 = torch.empty(v.shape[0], 2 * v.shape[1], device="cuda", dtype=torch.uint8)
    _lib.check(lib.mp_split_f16f8(src.data_ptr(), o16.data_ptr(), o8.data_ptr(), src.numel(), weight, st()))
    same_bits_nan_aware(o16.cpu(), want16, "fp16 plane")
    same_bits_nan_aware(o8.cpu(), want8, "correction plane")
    nan_in = torch.isnan(v)
    assert torch.isnan(o16.cpu()[nan_in]).all()
    print(f"  {v.numel()} values ({int(nan_in.sum())} NaN, {int(torch.isinf(v).sum())} inf): identical bytes")


def test_f16f8_epilogue_packer_sweep(lib):
    """pack4_f16f8 (the epilogue packer of the LayerNorm, attention and GELU f16f8 outputs: a fast branch for groups within +-448 and a clamped
    one) through ln_fwd out mode 3 with gamma = 0, so that the row written is beta exactly: the sweep, NaN / inf alone in a group of four
    (fast branch) and next to a value above 448 (clamped branch), bit for bit against the host construction."""
    _lib = lib_()
    v = sweep_values(0).reshape(-1)
    v = torch.where(v == 0, torch.zeros_like(v), v)        # 0 x xhat + (-0) is +0: the LayerNorm's arithmetic cannot hand -0 to the packer
    C, M = 1024, 4
    v = torch.cat([v, torch.zeros((-v.numel()) % C)]).reshape(-1, C)
    x = torch.randn(M, C, generator=torch.Generator().manual_seed(1)).cuda()
    gam = torch.zeros(C, device="cuda")
    st2 = torch.empty(M, 2, device="cuda")
    vd = v.cuda()
    h16 = torch.empty(v.shape[0], M, C, device="cuda", dtype=torch.float16)
    c8 = torch.empty(v.shape[0], M, 2 * C, device="cuda", dtype=torch.uint8)
    for i in range(v.shape[0]):
        _lib.check(lib.mp_layernorm_fwd_ex(x.data_ptr(), M, C, None, None, 0.0, None, 0, 0, None, None, gam.data_ptr(), vd[i].data_ptr(), 1e-6,
                                           h16[i].data_ptr(), c8[i].data_ptr(), None, st2.data_ptr(), 3, st()))
    want16, want8, _, _ = f16f8_planes(v, False)
    got16, got8 = h16.cpu(), c8.cpu()
    for r in range(M):
        same_bits_nan_aware(got16[:, r], want16, f"packer fp16 plane, row {r}")
        same_bits_nan_aware(got8[:, r], want8, f"packer correction plane, row {r}")
    print(f"  {v.numel()} values through the LayerNorm epilogue packer: identical bytes")

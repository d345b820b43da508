"""Kernel-level tests of every LayerNorm backward form the backbone backward launches (engine.hip backbone_bwd_impl), DropPath masks included,
each through the C entry point that fills the engine's arguments and calls the engine's dispatcher (mp_layernorm_bwd_ex -> ln_bwd,
mp_layernorm_bwd2_ex -> ln_bwd2, mp_scale_rows_ex -> scale_rows; include/manipose_hip.h).

Every value is compared with fp64 of the exact inputs the kernel receives (a bf16 dy decoded exactly, the fp32 row statistics as stored),
PER ELEMENT against that element's forward-error scale - never against a global max, so that a wrong row of small values cannot hide under a
large one.  u = 2^-24; the scales, with d = g gamma, xhat = (x - mean) rstd, a = mean_c |d|, b = mean_c |d xhat| and e the error scale of
xhat in units of u (e = |xhat| + |mean| rstd: the fp32 subtraction and product; |mean| rstd is 300 for a row of mean 30 and spread 0.1):
  dx of ln_bwd:  dx = rs dskip + rstd (d - mean(d) - xhat mean(d xhat))
      u [rstd (|d| + a + |xhat| b + e b + |xhat| mean_c(|d| e)) + |rs dskip| + |dx|]
      (the rounding of d, of the two row sums and of the products; an xhat error e enters through xhat s2 and through s2 itself)
  ln_bwd2:  t = rs dskip + LN1'(dy1) on x1 = (x0 - mean0) rstd0 gamma0 + beta0, recomputed in fp32 - x1 carries its own error
      E1 = |gamma0| (|xhat0| + |mean0| rstd0) + |beta0| + |x1|, so xhat1 has e1 = |xhat1| + |mean1| rstd1 + rstd1 E1.  t has the scale
      S_t = [dx scale of stage 1 with e1] + |rs dskip| + |t|, which stage 0 carries: dx = LN0'(t) has the stage-0 scale with d = t gamma0 plus
      rstd0 (|gamma0| S_t + mean_c(|gamma0| S_t) + |xhat0| mean_c(|gamma0| S_t |xhat0|)).
  parameter gradients (accumulated into a seed s): dgamma: u (sum_m |g| e + |s| + |dgamma|), dbeta: u (sum_m |g| + |s| + |dbeta|); stage 0 of
      ln_bwd2: dgamma0: u (sum_m (|t| e0 + S_t |xhat0|) + ..), dbeta0: u (sum_m (|t| + S_t) + ..).
The 2-byte copies are checked bit for bit: bf16 copy == bf16(dx * mask[sample(row)]) of the kernel's own fp32 dx; fp16 copy == the
saturating fp16 of dx * (mask S) (product in the kernel's order; clamped at +-65504, non-finite as 0) with both counters equal to exact host
counts.  Every form runs with the aliasing the engine uses (dx == dy in the post-norm call, dx == dskip elsewhere) and must give the bits of a
non-aliased call; two calls give the same bits, and a call whose parameter-gradient reduction runs on a second stream gives them too.

Bound constants: C_* below, in units of u times the element's scale; each was measured on the MI355X and is asserted with a margin (the
measured worst ratio is printed next to every bound)."""
import pytest
import torch

from test_gpu_parity import st

pytestmark = pytest.mark.gpu

U24 = 2.0 ** -24
# (measured worst ratio on the MI355X over this module's shapes -> asserted bound)
C_DX = 4.0           # dx of ln_bwd: 1.69 -> 4
C_DX2 = 1.5          # dx of ln_bwd2 (the scale carries t's): 0.61 -> 1.5
C_PG = 4.0           # dgamma / dbeta of ln_bwd and of stage 1 of ln_bwd2 (per-wave sums, per-workgroup partial rows, reduce_partials_kernel): 1.6 -> 4
C_PG0 = 0.15         # dgamma0 / dbeta0 of ln_bwd2 (the scale carries t's): 0.052 -> 0.15
S_F16 = 256.0        # the gradient scale S of the fp16-copy forms: the x64 rows of dy saturate, no other row comes near 65504

# (M, C, T, J, B): partial rows min(ceil(M / 4), occupancy slots): 77 and 230 (not multiples of 64: the remainder loop of reduce_partials_kernel),
# the bones net at full size, C = 512 at one and at 16 windows (several rows per wave), one frame
SHAPES = [(306, 32, 9, 17, 2), (918, 64, 27, 17, 2), (8262, 128, 243, 17, 2), (8262, 512, 243, 17, 2), (66096, 512, 243, 17, 16), (17, 512, 1, 17, 1)]
MASKS = [(0, None), (1, 0.9), (2, 0.9), (1, 0.5), (2, 0.5)]


def report(name, ratio, bound):
    print(f"[layernorm backward] {name}: worst error / bound-scale {ratio:.3g} (asserted <= {bound})")
    assert ratio <= bound, (name, ratio, bound)


def lib_():
    from manipose_amd import _lib
    return _lib


def ref_device(M, C):
    return "cuda" if M * C > (1 << 22) else "cpu"       # fp64 on the device for the two largest shapes (host time)


def same_bits(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape, what
    if a.dtype in (torch.bfloat16, torch.float16):
        a, b = a.view(torch.int16), b.view(torch.int16)
    elif a.dtype == torch.float32:
        a, b = a.view(torch.int32), b.view(torch.int32)
    bad = int((a != b).sum())
    assert bad == 0, f"{what}: {bad} elements differ"


def droppath_mask(mode, keep, B, T, J, g):
    """Per-sample multipliers 0 / 1/keep (mode 1: B T samples (b, t); mode 2: B J samples (b, j)): every window has a dropped sample, at a
    place that differs between windows, and window b > 0 keeps the sample window 0 drops - a swapped sample index cannot pass."""
    n = T if mode == 1 else J
    m = (torch.rand(B, n, generator=g) < keep).float() / keep
    for b in range(B):
        if n > 1:
            m[b, (3 * b + 1) % n] = 0.0
        if b > 0 and n > 4:
            m[b, 1] = 1.0 / keep
    if n == 1:
        m[:] = 1.0 / keep
    return m.reshape(-1).contiguous()


def row_multiplier(mask, mode, M, T, J):
    rows = torch.arange(M, device=mask.device)
    mask = mask[:(M // J if mode == 1 else (M // (T * J)) * J)]
    return mask[rows // J] if mode == 1 else mask[(rows // (T * J)) * J + rows % J]


def gsc_block(S):
    """the engine's 8-float gradient-scale block: {S, 1/S, .., counters (uint32) in words 4, 5}"""
    g = torch.tensor([S, 1.0 / S, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0], device="cuda")
    g.view(torch.int32)[4:6] = 0
    return g


def saturating_f16(v):
    fin = v.abs() <= 3.0e38
    sat = fin & (v.abs() > 65504.0)
    return torch.where(fin, v.clamp(-65504.0, 65504.0), torch.zeros_like(v)).half(), int(sat.sum()), int((~fin).sum())


def rows_input(M, C, g):
    """rows of mean 30 and spread 0.1 mixed with rows of mean 0 (every fifth)"""
    x = 30.0 + 0.1 * torch.randn(M, C, generator=g)
    x[1::5] = 0.1 * torch.randn(len(range(1, M, 5)), C, generator=g)
    return x


def row_stats(x, eps=1e-6):
    xd = x.double()
    mean = xd.mean(1)
    return torch.stack([mean, ((xd - mean[:, None]) ** 2).mean(1).add(eps).rsqrt()], 1).float().contiguous()


def grad_input(M, C, g):
    """dy: unit rows, every seventh row 2^-6 of that, every 97th (from row 11) x64 - the rows that saturate the fp16 copy at S_F16"""
    dy = torch.randn(M, C, generator=g)
    dy[::7] *= 2.0 ** -6
    dy[11::97] *= 64.0
    return dy


def lnp_ref(g, xh, rstd, gam, e):
    """fp64 LN'(g) (without the skip term) and its error scale in units of u (module docstring); g, xh, e: (M, C), rstd: (M, 1)"""
    d = g * gam
    s1, s2 = d.mean(1, keepdim=True), (d * xh).mean(1, keepdim=True)
    core = rstd * (d - s1 - xh * s2)
    ad = d.abs()
    a, b = ad.mean(1, keepdim=True), (ad * xh.abs()).mean(1, keepdim=True)
    scale = rstd * (ad + a + xh.abs() * b + e * b + xh.abs() * (ad * e).mean(1, keepdim=True))
    return core, scale


def ratio(got, want, scale):
    return ((got.to(want.device).double() - want).abs() / (U24 * scale)).max().item()


def ptr(t):
    return t.data_ptr() if t is not None else None


class Case:
    """inputs of one shape on the device and their fp64 images on the reference device"""

    def __init__(self, M, C, T, J, B, seed):
        self.M, self.C, self.T, self.J, self.B = M, C, T, J, B
        g = torch.Generator().manual_seed(seed)
        self.g = g
        self.rd = ref_device(M, C)
        x = rows_input(M, C, g)
        self.stats = row_stats(x)
        self.gam = 1.0 + 0.2 * torch.randn(C, generator=g)
        self.beta = 30.0 + 0.1 * torch.randn(C, generator=g)      # (ln_bwd2: the shared post-norm hands norm1 a mean-30 row)
        self.dy = grad_input(M, C, g)
        self.skip = torch.randn(M, C, generator=g)
        self.seed = [0.5 + torch.randn(C, generator=g) for _ in range(4)]
        # each mask sits at the start of B (T + J) floats: an index computed with T and J swapped still reads inside the buffer
        self.masks = {}
        for mode, keep in MASKS[1:]:
            m = droppath_mask(mode, keep, B, T, J, g)
            self.masks[(mode, keep)] = torch.cat([m, torch.ones(B * (T + J) - m.numel())]).cuda()
        self.x = x
        dv = lambda t: t.cuda()
        self.d_x, self.d_stats, self.d_gam, self.d_beta, self.d_skip = dv(x), dv(self.stats), dv(self.gam), dv(self.beta), dv(self.skip)
        self.d_dy32 = dv(self.dy)
        self.d_dyb = self.d_dy32.bfloat16()
        self.d_dys = (self.d_dy32 * S_F16).bfloat16()           # dy carried as bf16 of S x value (dy_scaled: times 1/S on load)
        self.scratch = torch.empty(1024 * 4 * C, device="cuda")

    def r(self, t):
        return t.to(self.rd).double()


def dy_of(case, kind):
    return {"fp32": (case.d_dy32, 0, 0), "bf16": (case.d_dyb, 1, 0), "scaled": (case.d_dys, 1, 1)}[kind]


def dy_exact(case, kind):
    """fp64 of what the kernel multiplies: the fp32 dy, the decoded bf16, or the decoded bf16 of S dy times 1/S (a power of two: exact)"""
    return case.r(case.d_dy32) if kind == "fp32" else (case.r(case.d_dyb) if kind == "bf16" else case.r(case.d_dys) / S_F16)


# ln_bwd forms (engine.hip backbone_bwd_impl): name, dy, skip, rs, copy ("bf16", "f16" or None); the aliasing follows from skip: dx == dy in
# the post-norm call (no skip), dx == dskip otherwise
LN_BWD_FORMS = [
    ("post-norm (fp32 dy, dx == dy, masked bf16 copy)", "fp32", False, 1.0, "bf16"),
    ("norm2 (bf16 dy, dx == dskip, masked bf16 copy)", "bf16", True, 1.0, "bf16"),
    ("norm2 rs 0.7", "bf16", True, 0.7, "bf16"),
    ("norm1 at l < 2 (no copy)", "bf16", True, 0.7, None),
    ("fp32 precision (fp32 dy, dx == dskip, no copy)", "fp32", True, 1.0, None),
    ("post-norm, f16 copy", "fp32", False, 1.0, "f16"),
    ("norm2, dy_scaled", "scaled", True, 0.7, "bf16"),
    ("norm1, dy_scaled", "scaled", True, 1.0, None),
]


def run_ln_bwd(lib, case, dy_kind, skip, rs, copy, mask_key, alias, pstream=None):
    M, C = case.M, case.C
    dy, dy_bf16, scaled = dy_of(case, dy_kind)
    sk = case.d_skip if skip else None
    if alias:
        G = (case.d_skip if skip else dy).clone()
        dy_arg, sk_arg, dx = (dy, G, G) if skip else (G, None, G)
    else:
        dy_arg, sk_arg, dx = dy, sk, torch.full((M, C), float("nan"), device="cuda")
    out = None
    if copy:
        out = torch.full((M, C), float("nan"), device="cuda", dtype=torch.bfloat16 if copy == "bf16" else torch.float16)
    mode, keep = mask_key
    mask = case.masks[mask_key] if mode else None
    dg, db = case.seed[0].cuda(), case.seed[1].cuda()
    gsc = gsc_block(S_F16)
    rc = lib.mp_layernorm_bwd_ex(dy_arg.data_ptr(), dy_bf16, case.d_x.data_ptr(), case.d_stats.data_ptr(), case.d_gam.data_ptr(), ptr(sk_arg), rs,
                                 dx.data_ptr(), ptr(out), ptr(mask), mode, case.T, case.J, gsc.data_ptr(), scaled, int(copy == "f16"), dg.data_ptr(),
                                 db.data_ptr(), M, C, case.scratch.data_ptr(), case.scratch.numel(), pstream, st())
    lib_().check(rc, "mp_layernorm_bwd_ex")
    torch.cuda.synchronize()
    return dx, out, dg, db, gsc.view(torch.int32)[4:6].cpu().tolist()


def check_copy(case, dx, out, copy, mask_key, cnt, what):
    mode, _ = mask_key
    mrow = row_multiplier(case.masks[mask_key], mode, case.M, case.T, case.J) if mode else torch.ones(case.M, device="cuda")
    if copy == "bf16":
        same_bits(out, (dx * mrow[:, None]).bfloat16(), f"{what}: bf16 copy")
        assert cnt == [0, 0]
        return 0
    want, n_sat, n_nf = saturating_f16(dx * (mrow * S_F16)[:, None])
    same_bits(out, want, f"{what}: fp16 copy")
    assert cnt == [n_sat, n_nf], (what, cnt, n_sat, n_nf)
    return n_sat


@pytest.mark.parametrize("M,C,T,J,B", SHAPES + [(4131, 1024, 243, 17, 1)])
def test_ln_bwd_every_engine_form(lib, M, C, T, J, B):
    """ln_bwd in every form of the backbone backward, no mask and mode-1 / mode-2 masks at keep 0.9 and 0.5: dx and the parameter gradients
    against fp64 per element, the copies bit for bit, aliased == non-aliased, deterministic, parameter-stream reduction == single stream."""
    case = Case(M, C, T, J, B, 7 * M + C)
    xh32 = (case.r(case.x) - case.r(case.stats[:, :1])) * case.r(case.stats[:, 1:])
    mean, rstd = case.r(case.stats[:, :1]), case.r(case.stats[:, 1:])
    e = xh32.abs() + mean.abs() * rstd
    gam = case.r(case.gam)
    refs = {}
    sat_rows = 0
    for name, dy_kind, skip, rs, copy in LN_BWD_FORMS:
        if dy_kind not in refs:
            gd = dy_exact(case, dy_kind)
            core, scale = lnp_ref(gd, xh32, rstd, gam, e)
            refs[dy_kind] = (core, scale, (gd * xh32).sum(0), (gd.abs() * e).sum(0), gd.sum(0), gd.abs().sum(0))
        core, scale, dg_r, dg_s, db_r, db_s = refs[dy_kind]
        rsk = torch.tensor(rs, dtype=torch.float32).double().item()
        want = core + (rsk * case.r(case.skip) if skip else 0.0)
        full_scale = scale + ((rsk * case.r(case.skip)).abs() if skip else 0.0) + want.abs()
        first = None
        for mask_key in (MASKS if copy else MASKS[:1]):
            dx, out, dg, db, cnt = run_ln_bwd(lib, case, dy_kind, skip, rs, copy, mask_key, alias=False)
            dx2, out2, dg2, db2, cnt2 = run_ln_bwd(lib, case, dy_kind, skip, rs, copy, mask_key, alias=True)
            what = f"{name} M={M} C={C} mask={mask_key}"
            for a, b, k in ((dx, dx2, "dx"), (out, out2, "copy"), (dg, dg2, "dgamma"), (db, db2, "dbeta")):
                if a is not None:
                    same_bits(a, b, f"{what}: aliased call, {k}")
            assert cnt == cnt2
            if copy:
                sat_rows += check_copy(case, dx, out, copy, mask_key, cnt, what)
            if first is None:
                first = (dx, dg, db)
                report(f"dx, {name} M={M} C={C}", ratio(dx, want, full_scale), C_DX)
                sd0, sd1 = case.r(case.seed[0]), case.r(case.seed[1])
                report(f"dgamma, {name} M={M} C={C}", ratio(dg, sd0 + dg_r, dg_s + sd0.abs() + (sd0 + dg_r).abs()), C_PG)
                report(f"dbeta, {name} M={M} C={C}", ratio(db, sd1 + db_r, db_s + sd1.abs() + (sd1 + db_r).abs()), C_PG)
                # deterministic, and the same bits with the reduction on a second stream (the engine's weight-gradient stream)
                _, _, dg3, db3, _ = run_ln_bwd(lib, case, dy_kind, skip, rs, copy, mask_key, alias=False)
                side = torch.cuda.Stream()
                _, _, dg4, db4, _ = run_ln_bwd(lib, case, dy_kind, skip, rs, copy, mask_key, alias=True, pstream=side.cuda_stream)
                for a in (dg3, dg4):
                    same_bits(a, dg, f"{what}: dgamma, repeated / parameter stream")
                for a in (db3, db4):
                    same_bits(a, db, f"{what}: dbeta, repeated / parameter stream")
            else:       # the mask reaches the copy only
                same_bits(dx, first[0], f"{what}: dx changed with the mask")
                same_bits(dg, first[1], f"{what}: dgamma changed with the mask")
    if M > 11:
        assert sat_rows > 0, "the fp16-copy form saturated nothing"
        print(f"  fp16 copies: {sat_rows} clamped stores over the mask cases")


# ln_bwd2 forms: name, dy1, rs, copy
LN_BWD2_FORMS = [
    ("fp32 dy1, masked bf16 copy", "fp32", 1.0, "bf16"),
    ("bf16 dy1, masked bf16 copy, rs 0.7", "bf16", 0.7, "bf16"),
    ("bf16 dy1, no copy", "bf16", 1.0, None),
    ("fp32 dy1, no copy, rs 0.7", "fp32", 0.7, None),
    ("dy_scaled bf16 dy1, f16 copy, rs 0.7", "scaled", 0.7, "f16"),
    ("fp32 dy1, f16 copy", "fp32", 1.0, "f16"),
]


def run_ln_bwd2(lib, case, x0, stats0, stats1, dy_kind, rs, copy, mask_key, alias, pstream=None):
    M, C = case.M, case.C
    dy, dy_bf16, scaled = dy_of(case, dy_kind)
    if alias:
        G = case.d_skip.clone()
        sk, dx = G, G
    else:
        sk, dx = case.d_skip, torch.full((M, C), float("nan"), device="cuda")
    out = None
    if copy:
        out = torch.full((M, C), float("nan"), device="cuda", dtype=torch.bfloat16 if copy == "bf16" else torch.float16)
    mode, _ = mask_key
    mask = case.masks[mask_key] if mode else None
    pg = [s.cuda() for s in case.seed]
    gsc = gsc_block(S_F16)
    rc = lib.mp_layernorm_bwd2_ex(dy.data_ptr(), dy_bf16, stats1.data_ptr(), case.d_gam1.data_ptr(), sk.data_ptr(), rs, x0.data_ptr(), stats0.data_ptr(),
                                  case.d_gam.data_ptr(), case.d_beta.data_ptr(), dx.data_ptr(), ptr(out), ptr(mask), mode, case.T, case.J, gsc.data_ptr(),
                                  scaled, int(copy == "f16"), *(p.data_ptr() for p in pg), M, C, case.scratch.data_ptr(), case.scratch.numel(), pstream,
                                  st())
    lib_().check(rc, "mp_layernorm_bwd2_ex")
    torch.cuda.synchronize()
    return dx, out, pg, gsc.view(torch.int32)[4:6].cpu().tolist()


@pytest.mark.parametrize("M,C,T,J,B", SHAPES)
def test_ln_bwd2_every_engine_form(lib, M, C, T, J, B):
    """ln_bwd2 (norm1 of block l fused with the shared post-norm of block l - 1, x1 recomputed from x0 in fp32) in every form, no mask and
    mode-1 / mode-2 masks: dx and the four parameter gradients against fp64 per element (the stage-1 result t carried through stage 0 with its
    own scale), copies bit for bit, aliased == non-aliased, deterministic, parameter-stream reduction == single stream."""
    case = Case(M, C, T, J, B, 11 * M + C + 1)
    g = case.g
    case.gam1 = 1.0 + 0.2 * torch.randn(C, generator=g)
    case.d_gam1 = case.gam1.cuda()
    x0, stats0 = case.d_x, case.d_stats
    m0, r0 = case.r(stats0[:, :1]), case.r(stats0[:, 1:])
    xh0 = (case.r(x0) - m0) * r0
    gam0, b0, gam1 = case.r(case.gam), case.r(case.beta), case.r(case.gam1)
    x1 = xh0 * gam0 + b0                                                  # fp64 of the forward's expression on the exact x0
    E1 = gam0.abs() * (xh0.abs() + m0.abs() * r0) + b0.abs() + x1.abs()
    # stats1 as the forward stores them: of its fp32 x1 (= the kernel's recomputation, the same expression)
    x1_32 = ((x0 - stats0[:, :1]) * stats0[:, 1:] * case.d_gam + case.d_beta)
    stats1 = row_stats(x1_32)
    m1, r1 = case.r(stats1[:, :1]), case.r(stats1[:, 1:])
    xh1 = (x1 - m1) * r1
    e1 = xh1.abs() + m1.abs() * r1 + r1 * E1
    e0 = xh0.abs() + m0.abs() * r0
    sk = case.r(case.skip)
    sat = 0
    for name, dy_kind, rs, copy in LN_BWD2_FORMS:
        gd = dy_exact(case, dy_kind)
        core1, sc1 = lnp_ref(gd, xh1, r1, gam1, e1)
        rsk = torch.tensor(rs, dtype=torch.float32).double().item()
        t = core1 + rsk * sk
        St = sc1 + (rsk * sk).abs() + t.abs()
        core0, sc0 = lnp_ref(t, xh0, r0, gam0, e0)
        gS = gam0.abs() * St
        sc0 = sc0 + r0 * (gS + gS.mean(1, keepdim=True) + xh0.abs() * (gS * xh0.abs()).mean(1, keepdim=True)) + core0.abs()
        want_p = [(gd * xh1).sum(0), gd.sum(0), (t * xh0).sum(0), t.sum(0)]
        scale_p = [(gd.abs() * e1).sum(0), gd.abs().sum(0), (t.abs() * e0 + St * xh0.abs()).sum(0), (t.abs() + St).sum(0)]
        first = None
        for mask_key in (MASKS if copy else MASKS[:1]):
            dx, out, pg, cnt = run_ln_bwd2(lib, case, x0, stats0, stats1, dy_kind, rs, copy, mask_key, alias=False)
            dx2, out2, pg2, cnt2 = run_ln_bwd2(lib, case, x0, stats0, stats1, dy_kind, rs, copy, mask_key, alias=True)
            what = f"ln_bwd2 {name} M={M} C={C} mask={mask_key}"
            same_bits(dx, dx2, f"{what}: aliased call, dx")
            if out is not None:
                same_bits(out, out2, f"{what}: aliased call, copy")
            for k in range(4):
                same_bits(pg[k], pg2[k], f"{what}: aliased call, parameter gradient {k}")
            assert cnt == cnt2
            if copy:
                sat += check_copy(case, dx, out, copy, mask_key, cnt, what)
            if first is None:
                first = (dx, pg)
                report(f"dx, ln_bwd2 {name} M={M} C={C}", ratio(dx, core0, sc0), C_DX2)
                for k, nm in enumerate(("dgamma1", "dbeta1", "dgamma0", "dbeta0")):
                    s = case.r(case.seed[k])
                    report(f"{nm}, ln_bwd2 {name} M={M} C={C}", ratio(pg[k], s + want_p[k], scale_p[k] + s.abs() + (s + want_p[k]).abs()),
                           C_PG if k < 2 else C_PG0)
                _, _, pg3, _ = run_ln_bwd2(lib, case, x0, stats0, stats1, dy_kind, rs, copy, mask_key, alias=False)
                side = torch.cuda.Stream()
                _, _, pg4, _ = run_ln_bwd2(lib, case, x0, stats0, stats1, dy_kind, rs, copy, mask_key, alias=True, pstream=side.cuda_stream)
                for k in range(4):
                    same_bits(pg3[k], pg[k], f"{what}: parameter gradient {k}, repeated")
                    same_bits(pg4[k], pg[k], f"{what}: parameter gradient {k}, parameter stream")
            else:
                same_bits(dx, first[0], f"{what}: dx changed with the mask")
                for k in range(4):
                    same_bits(pg[k], first[1][k], f"{what}: parameter gradient {k} changed with the mask")
    if M > 11:
        assert sat > 0, "the fp16-copy forms saturated nothing"


@pytest.mark.parametrize("M,C,T,J,B", [SHAPES[0], SHAPES[2], SHAPES[4], SHAPES[5]])
def test_scale_rows_both_output_types(lib, M, C, T, J, B):
    """scale_rows (the fp32-precision DropPath of a branch gradient): out = mask(row) g, fp32 and bf16, bit for bit, modes 1 and 2."""
    g = torch.Generator().manual_seed(M + C)
    gd = grad_input(M, C, g).cuda()
    for mode, keep in MASKS[1:]:
        mask = droppath_mask(mode, keep, B, T, J, g).cuda()
        prod = gd * row_multiplier(mask, mode, M, T, J)[:, None]
        for out_bf16, dt in ((0, torch.float32), (1, torch.bfloat16)):
            out = torch.full((M, C), float("nan"), device="cuda", dtype=dt)
            lib_().check(lib.mp_scale_rows_ex(gd.data_ptr(), mask.data_ptr(), mode, out.data_ptr(), out_bf16, M, C, T, J, st()), "mp_scale_rows_ex")
            same_bits(out, prod.to(dt), f"scale_rows M={M} C={C} mode={mode} keep={keep} bf16={out_bf16}")


def test_layernorm_backward_entry_points_refuse_bad_arguments(lib):
    """Every refusal returns MP_ERR_ARG before any launch (the output keeps its sentinel)."""
    M, C, T, J = 306, 32, 9, 17
    z = lambda *s: torch.zeros(*s, device="cuda")
    dy, x, k, dx = z(M, C), z(M, C), z(M, C), torch.full((M, C), float("nan"), device="cuda")
    stats, gam, beta = z(M, 2), z(C), z(C)
    copy = torch.empty(M, C, device="cuda", dtype=torch.bfloat16)
    mask = torch.ones(2 * T + 2 * J, device="cuda")          # covers both modes' sample counts
    gsc = gsc_block(1.0)
    p = [z(C) for _ in range(4)]
    scr = z(1024 * 4 * C)

    def bwd(mask_=mask, mode=1, M_=M, C_=C, T_=T, out=copy, copy_f16=0, scratch_floats=1024 * 2 * C, gsc_=gsc):
        return lib.mp_layernorm_bwd_ex(dy.data_ptr(), 0, x.data_ptr(), stats.data_ptr(), gam.data_ptr(), k.data_ptr(), 1.0, dx.data_ptr(), ptr(out),
                                       ptr(mask_), mode, T_, J, ptr(gsc_), 0, copy_f16, p[0].data_ptr(), p[1].data_ptr(), M_, C_, scr.data_ptr(),
                                       scratch_floats, None, st())

    def bwd2(mask_=mask, mode=2, M_=M, C_=C, T_=T, out=copy, copy_f16=0, scratch_floats=1024 * 4 * C, beta_=beta):
        return lib.mp_layernorm_bwd2_ex(dy.data_ptr(), 0, stats.data_ptr(), gam.data_ptr(), k.data_ptr(), 1.0, x.data_ptr(), stats.data_ptr(),
                                        gam.data_ptr(), ptr(beta_), dx.data_ptr(), ptr(out), ptr(mask_), mode, T_, J, gsc.data_ptr(), 0, copy_f16,
                                        *(t.data_ptr() for t in p), M_, C_, scr.data_ptr(), scratch_floats, None, st())

    def rows(mode=1, M_=M, T_=T):
        return lib.mp_scale_rows_ex(k.data_ptr(), mask.data_ptr(), mode, dx.data_ptr(), 0, M_, C, T_, J, st())

    bad = {
        "ln_bwd mask_mode 0": bwd(mode=0), "ln_bwd mask_mode 3": bwd(mode=3), "ln_bwd M % (T J)": bwd(M_=M - J), "ln_bwd T = 0": bwd(T_=0),
        "ln_bwd copy_f16 without dx_b16": bwd(out=None, copy_f16=1), "ln_bwd copy_f16 without gsc": bwd(copy_f16=1, gsc_=None),
        "ln_bwd C % 4": bwd(mask_=None, C_=C - 2), "ln_bwd C > 1024": bwd(mask_=None, C_=1028), "ln_bwd scratch": bwd(scratch_floats=1024 * 2 * C - 1),
        "ln_bwd2 mask_mode 0": bwd2(mode=0), "ln_bwd2 mask_mode -1": bwd2(mode=-1), "ln_bwd2 M % (T J)": bwd2(M_=M - 1),
        "ln_bwd2 copy_f16 without dx_b16": bwd2(out=None, copy_f16=1), "ln_bwd2 C > 512": bwd2(mask_=None, C_=516),
        "ln_bwd2 without beta0": bwd2(beta_=None), "ln_bwd2 scratch": bwd2(scratch_floats=1024 * 4 * C - 1),
        "scale_rows mask_mode 0": rows(mode=0), "scale_rows M % (T J)": rows(M_=M - 17 * 3),
    }
    torch.cuda.synchronize()
    wrong = {k: v for k, v in bad.items() if v != 1}
    assert not wrong, wrong
    assert torch.isnan(dx).all(), "a refused call launched"
    assert bwd(mask_=None, mode=0) == 0 and bwd2() == 0 and rows() == 0          # the same calls with good arguments run
    torch.cuda.synchronize()

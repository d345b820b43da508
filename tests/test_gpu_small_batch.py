"""The small-batch GEMM configuration: the 128 x 128 tile of the f16f8 Linear (gemm_bf16_glds_kernel<.., BT = 128, SPLIT = 8>) and the planner
(mp_gemm_plan) that chooses tile and kernel from the shape and the CU count.

The condition these tests hold is IDENTITY, not a tolerance: the 128-wide tile performs, per output element, the persistent 256-wide kernel's
sequence of matrix-core accumulations (k-tiles ascending; fp16 chunk g, fp16 chunk g + 4, then the fp8 correction product) and runs the
persistent kernel's own epilogue code, so every output plane of every form is equal bit for bit - compared as integers, NaN payloads
included.  The fp64 accuracy of the 256-wide form is held by tests/test_gpu_f16f8_kernels.py; identity carries it over.  The model-level tests
then show that the planner's default path (tile 128 where the large tile leaves CUs idle: the reference's own batch sizes) gives the bits of
the large-tile path, and the oracle test that those bits are right.

mp_gemm_launch_counts proves which kernel ran; every test restores gemm_tile = 0."""
import ctypes as C

import pytest
import torch

import manipose_ref as orc
from test_gpu_parity import MPJPE_TOL_M, _cos, _grad_report, close, st

pytestmark = pytest.mark.gpu

TJ = {17: (1, 17), 128: (8, 16), 255: (15, 17), 257: (257, 1), 4131: (243, 17), 12393: (243, 17)}      # M = B T J for the DropPath masks
PAD = 130                                    # guard rows behind the M rows of every output: a kernel that stores its M-tail rows is caught
S32, S16 = 0x7FBADBAD, 0x7FBA                # "never written" patterns (NaNs no arithmetic here produces)


def _lib():
    from manipose_amd import _lib
    return _lib


def set_tile(lib, tile):
    _lib().check(lib.mp_set_option(b"gemm_tile", tile), "gemm_tile")


def counts(lib, reset=1):
    out = (C.c_int64 * 3)()
    _lib().check(lib.mp_gemm_launch_counts(out, reset))
    return list(out)


def ints(t):
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def guarded(M, N, dtype):
    """(M + PAD, N) buffer filled with the never-written pattern; the kernel sees the first M rows"""
    if dtype == torch.uint8:
        return torch.full((M + PAD, N), 0x7E, device="cuda", dtype=torch.uint8)
    if dtype == torch.float32:
        return torch.full((M + PAD, N), S32, device="cuda", dtype=torch.int32).view(torch.float32)
    return torch.full((M + PAD, N), S16, device="cuda", dtype=torch.int16).view(dtype)


def check_planes(M, a, b, what):
    """bit identity of two runs' output planes (lists of guarded buffers, None for absent planes), guard rows untouched, every element written"""
    for i, (p, q) in enumerate(zip(a, b)):
        if p is None:
            assert q is None
            continue
        pi, qi = ints(p), ints(q)
        diff = (pi[:M] != qi[:M]).sum().item()
        assert diff == 0, f"{what}: plane {i}: {diff} of {pi[:M].numel()} elements differ between the tiles"
        if p.dtype != torch.uint8:
            sent = S32 if p.element_size() == 4 else S16
            for r, name in ((pi, "128"), (qi, "256")):
                assert (r[:M] == sent).sum().item() == 0, f"{what}: plane {i}: tile {name} left elements unwritten"
                assert (r[M:] == sent).all().item(), f"{what}: plane {i}: tile {name} stored rows past M"
        else:
            for r, name in ((pi, "128"), (qi, "256")):
                assert (r[M:] == 0x7E).all().item(), f"{what}: plane {i}: tile {name} stored rows past M"


def f16f8_device_planes(lib, v, weight):
    """fp32 (rows, K) on the device -> (fp16 plane, correction plane) through the library's splitter"""
    hi = torch.empty(v.shape, device="cuda", dtype=torch.float16)
    c8 = torch.empty(v.shape[0], 2 * v.shape[1], device="cuda", dtype=torch.uint8)
    _lib().check(lib.mp_split_f16f8(v.data_ptr(), hi.data_ptr(), c8.data_ptr(), v.numel(), weight, st()))
    return hi, c8


def f16f8_case(M, N, K, seed, special=False):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, K, generator=g)
    x[::7] *= 2.0 ** -6
    W = torch.randn(N, K, generator=g) / K ** 0.5
    if special:                               # NaN / inf / beyond the e4m3 range, in the operands (tests/test_gpu_f16f8_kernels.py pins the format's policy)
        x[3, 5], x[M // 2, 17], x[M - 1, 0], x[5, 64], x[6, 70] = float("nan"), float("inf"), -float("inf"), 1000.0, -449.0
        W[7, 3], W[N - 1, K - 1] = 500.0, float("nan")
    b = torch.randn(N, generator=g)
    T, J = TJ[M]
    r_in = torch.randn(M, N, generator=g) * 2.0 + 0.3
    stats = torch.stack([r_in.double().mean(1), (r_in.double().var(1, unbiased=False) + 1e-6).rsqrt()], 1).float().contiguous()
    gamma, beta = 1.0 + 0.2 * torch.randn(N, generator=g), 0.1 * torch.randn(N, generator=g)
    masks = {0: None}
    for mode, ns in ((1, M // J), (2, (M // (T * J)) * J)):
        m = (torch.rand(ns, generator=g) > 0.3).float() / 0.7
        m[-1] = 1 / 0.7
        if ns > 1:
            m[0] = 0.0
        masks[mode] = m.cuda()
    return dict(x=x.cuda(), W=W.cuda(), b=b.cuda(), r_in=r_in.cuda(), stats=stats.cuda(), gamma=gamma.cuda(), beta=beta.cuda(), masks=masks, T=T, J=J)


# the five output forms gemm_f16f8 dispatches, as (name, epilogue, out_form, variants); a variant = (residual LayerNorm recomputed?, mask mode, z kept?)
FORMS = [("fp32 + bias", 0, 0, [(False, 0, False)]),
         ("fp32 + bias + residual", 2, 0, [(ln, mode, False) for ln in (False, True) for mode in (0, 1, 2)]),
         ("planar bf16 + bias", 0, 1, [(False, 0, False)]),
         ("planar bf16 + GELU", 1, 1, [(False, 0, False), (False, 0, True)]),
         ("f16f8 planes + GELU", 1, 2, [(False, 0, False), (False, 0, True)])]


def run_form(lib, c, ops, M, N, K, epi, form, ln, mode, keep_z):
    p = lambda t: t.data_ptr() if t is not None else None
    if form == 0:
        y, y_lo = guarded(M, N, torch.float32), None
    elif form == 1:
        y, y_lo = guarded(M, N, torch.bfloat16), guarded(M, N, torch.bfloat16)
    else:
        y, y_lo = guarded(M, N, torch.float16), guarded(M, 2 * N, torch.uint8)
    z = guarded(M, N, torch.bfloat16) if keep_z else None
    resid = epi == 2
    _lib().check(lib.mp_linear_fwd_f16f8_ex(*(t.data_ptr() for t in ops), p(c["b"]), p(y), p(y_lo), p(z), p(c["r_in"]) if resid else None,
                                            p(c["stats"]) if ln else None, p(c["gamma"]) if ln else None, p(c["beta"]) if ln else None,
                                            p(c["masks"][mode]) if resid else None, mode if resid else 0, 1.0, c["T"], c["J"], M, N, K, epi, form, st()),
                 "mp_linear_fwd_f16f8_ex")
    return [y, y_lo, z]


@pytest.mark.parametrize("N,K", [(1536, 512), (512, 512), (2048, 512), (512, 2048), (256, 128)])
@pytest.mark.parametrize("M", [17, 128, 255, 257, 4131, 12393])
def test_f16f8_tile_128_equals_tile_256_bit_for_bit(lib, M, N, K):
    """Every output form of the f16f8 Linear, tile 128 against tile 256 on the same operands: zero differing elements in y, y_lo and z (integer
    views).  The fp32 + bias form proves the accumulation order; the others that the 128-wide tile rounds its epilogue as the persistent kernel
    does.  M covers partial tiles of both sizes (17, 255, 257; 4131 = 32 x 128 + 35; 12393 = 96 x 128 + 105), one and three full windows; the
    residual form runs with and without the recomputed LayerNorm and with DropPath masks of mode 0 / 1 / 2 that drop samples; gelu' is kept (z) and
    not (NULL, inference).  One case carries NaN / inf / values beyond +-448 in its operands.  The launch counters show that the 128 run launched
    only tiled-128 kernels and the 256 run none."""
    special = (M, N, K) == (257, 512, 512)
    c = f16f8_case(M, N, K, 11 * M + N + K, special)
    ops = f16f8_device_planes(lib, c["x"], 0) + f16f8_device_planes(lib, c["W"], 1)
    try:
        for name, epi, form, variants in FORMS:
            for ln, mode, keep_z in variants:
                set_tile(lib, 128)
                counts(lib)
                a = run_form(lib, c, ops, M, N, K, epi, form, ln, mode, keep_z)
                ca = counts(lib)
                set_tile(lib, 256)
                b = run_form(lib, c, ops, M, N, K, epi, form, ln, mode, keep_z)
                cb = counts(lib)
                torch.cuda.synchronize()
                assert ca == [0, 0, 1], f"tile 128 launched {ca} (persistent 256, tiled 256, tiled 128)"
                assert cb == [1, 0, 0], f"tile 256 launched {cb}"
                check_planes(M, a, b, f"{name} M={M} N={N} K={K} rstats={ln} mask mode {mode} z={'kept' if keep_z else 'NULL'}")
        if special:
            assert torch.isnan(a[0][:M].float()).any().item(), "the special values did not reach the output"
    finally:
        set_tile(lib, 0)


def test_f16f8_tile_128_is_deterministic(lib):
    """Two identical launches of the 128-wide form give identical bits (residual form with masks and the f16f8-plane GELU form, three windows)."""
    M, N, K = 12393, 512, 512
    c = f16f8_case(M, N, K, 5)
    ops = f16f8_device_planes(lib, c["x"], 0) + f16f8_device_planes(lib, c["W"], 1)
    try:
        set_tile(lib, 128)
        for epi, form, ln, mode, keep_z in ((2, 0, True, 2, False), (1, 2, False, 0, True)):
            counts(lib)
            a = run_form(lib, c, ops, M, N, K, epi, form, ln, mode, keep_z)
            b = run_form(lib, c, ops, M, N, K, epi, form, ln, mode, keep_z)
            torch.cuda.synchronize()
            assert counts(lib) == [0, 0, 2]
            check_planes(M, a, b, f"repeat epi={epi} form={form}")
    finally:
        set_tile(lib, 0)


# ------------------------------------------------------------------------------------------------ the forms that gain selection
def _two_tiles(lib, run, want_128, want_256, what):
    try:
        set_tile(lib, 128)
        counts(lib)
        a = run()
        ca = counts(lib)
        set_tile(lib, 256)
        b = run()
        cb = counts(lib)
        torch.cuda.synchronize()
    finally:
        set_tile(lib, 0)
    assert ca == want_128, (what, ca)
    assert cb == want_256, (what, cb)
    for i, (p, q) in enumerate(zip(a, b)):
        diff = (ints(p) != ints(q)).sum().item()
        assert diff == 0, f"{what}: output {i}: {diff} elements differ between tile 128 and tile 256"


@pytest.mark.parametrize("N_out,K_in", [(1536, 512), (512, 512), (2048, 512), (512, 2048)])
def test_bf16_and_fp16_dgrad_tiles_agree_bit_for_bit(lib, N_out, K_in):
    """dx = dy W at M = 12393 (three windows: the tiled region, where the planner chooses between the two instantiations of one template): plain bf16
    dgrad, the gelu'-multiplying one, the fp16-operand one (mp_linear_bwd_f16) and mp_linear_bwd_bf16's dgrad with fp32 and bf16 dx."""
    M = 12393
    g = torch.Generator().manual_seed(N_out + K_in)
    dy32 = torch.randn(M, N_out, generator=g).cuda()
    W32 = (torch.randn(N_out, K_in, generator=g) / K_in ** 0.5).cuda()
    zb = torch.rand(M, K_in, generator=g).cuda().bfloat16()
    for f16 in (0, 1):
        dy, W = (dy32.half(), W32.half()) if f16 else (dy32.bfloat16(), W32.bfloat16())
        for z in (None, zb):
            def run():
                dx = torch.full((M, K_in), S16, device="cuda", dtype=torch.int16).view(torch.bfloat16)
                _lib().check(lib.mp_linear_bwd_f16(dy.data_ptr(), None, W.data_ptr(), dx.data_ptr(), z.data_ptr() if z is not None else None, None, None, None,
                                                   None, M, N_out, K_in, f16, 0, None, None, 0, st()), "mp_linear_bwd_f16")
                return [dx]
            _two_tiles(lib, run, [0, 0, 1], [0, 1, 0], f"dgrad f16={f16} dgelu={z is not None} {N_out}x{K_in}")
    x = torch.randn(M, K_in, generator=g).cuda().bfloat16()
    dy, W = dy32.bfloat16(), W32.bfloat16()
    slab = torch.empty(int(lib.mp_linear_bwd_slab_floats(N_out, K_in)), device="cuda")
    for dx_f32 in (0, 1):
        def run():
            dx = torch.zeros(M, K_in, device="cuda", dtype=torch.float32 if dx_f32 else torch.bfloat16)
            dW, db = torch.zeros(N_out, K_in, device="cuda"), torch.zeros(N_out, device="cuda")
            _lib().check(lib.mp_linear_bwd_bf16(dy.data_ptr(), 0, x.data_ptr(), W.data_ptr(), dx.data_ptr(), dx_f32, dW.data_ptr(), db.data_ptr(), M, N_out, K_in,
                                                slab.data_ptr(), slab.numel(), st()), "mp_linear_bwd_bf16")
            return [dx, dW, db]
        # (the weight gradient keeps the large tile under both settings: its split-K was laid out for it)
        _two_tiles(lib, run, [0, 1, 1], [0, 2, 0], f"mp_linear_bwd_bf16 dx_f32={dx_f32} {N_out}x{K_in}")


@pytest.mark.parametrize("N,K", [(1536, 512), (512, 512), (2048, 512), (512, 2048)])
def test_bf16x3_forward_tiles_agree_bit_for_bit(lib, N, K):
    """The split-precision forward (three bf16 products) at M = 12393, every epilogue, tile 128 against tile 256 of the tiled template."""
    M = 12393
    g = torch.Generator().manual_seed(N + 3 * K)
    x = torch.randn(M, K, generator=g).cuda()
    W = (torch.randn(N, K, generator=g) / K ** 0.5).cuda()
    b = torch.randn(N, generator=g).cuda()
    r = torch.randn(M, N, generator=g).cuda()

    def split(t):
        hi, lo = torch.empty_like(t, dtype=torch.bfloat16), torch.empty_like(t, dtype=torch.bfloat16)
        _lib().check(lib.mp_split_bf16(t.data_ptr(), hi.data_ptr(), lo.data_ptr(), t.numel(), st()))
        return hi, lo
    xh, xl = split(x)
    Wh, Wl = split(W)
    for epi in (0, 1, 2):
        def run():
            if epi == 2:
                y, yl, z = torch.zeros(M, N, device="cuda"), None, None
            else:
                y, yl = (torch.zeros(M, N, device="cuda", dtype=torch.bfloat16) for _ in range(2))
                z = torch.zeros(M, N, device="cuda", dtype=torch.bfloat16) if epi == 1 else None
            p = lambda t: t.data_ptr() if t is not None else None
            _lib().check(lib.mp_linear_fwd_bf16x3(p(xh), p(xl), p(Wh), p(Wl), p(b), p(y), p(yl), p(z), p(r) if epi == 2 else None, M, N, K, epi, st()),
                         "mp_linear_fwd_bf16x3")
            return [t for t in (y, yl, z) if t is not None]
        _two_tiles(lib, run, [0, 0, 1], [0, 1, 0], f"bf16x3 forward epilogue {epi} {N}x{K}")


# ------------------------------------------------------------------------------------------------ model level
def _full_model(f16f8, B, train):
    from manipose_amd import RMCLManifoldMixSTE, h36m_skeleton
    model = RMCLManifoldMixSTE(h36m_skeleton(), drop_path_rate=0.1 if train else 0.0)
    model.load_state_dict(orc.make_state(orc.FULL_CFG, seed=3), strict=True)
    model.precision, model.f16f8 = "bf16x3", f16f8
    model.max_batch_hint = B
    model = model.cuda()
    model = model.train() if train else model.eval()
    model._ensure_engine(B, torch.device("cuda"))
    return model


def _masks(layout, seed=17):
    """injected DropPath masks (keep 0.9), every branch dropping samples - the construction of the masked full-size parity test"""
    gen = torch.Generator().manual_seed(seed)
    masks = {}
    for name, _, cnt, keep in layout:
        if keep >= 1.0:
            continue
        m = (torch.rand(cnt, generator=gen) < 0.9).float() / 0.9
        half = cnt // 2
        m[1], m[half + 1] = 0.0, 1.0 / 0.9
        masks[name] = m
    return masks


def _train_step_bits(lib, model, X, y, masks):
    """forward (train mode, injected masks), loss, backward: poses, scores, the four loss terms and the flat gradient, plus the launch counts"""
    from manipose_amd.metrics import rmcl_training_loss
    model.zero_grad(set_to_none=True)
    model.set_droppath_masks({k: v.cuda() for k, v in masks.items()})
    counts(lib)
    poses, scores = model(X)
    total, terms = rmcl_training_loss(poses, scores, y)
    total.backward()
    torch.cuda.synchronize()
    n = counts(lib)
    flat = torch.cat([p.grad.reshape(-1) for _, p in model.named_parameters()])
    return [poses.detach().clone(), scores.detach().clone(), torch.stack([terms[k].detach() for k in ("wloss", "score_reg", "vloss", "sreg")]), flat.clone()], n


@pytest.mark.parametrize("f16f8,B", [(3, 3), (3, 1), (0, 3)])
def test_planner_path_gives_the_bits_of_the_large_tile_path(lib, f16f8, B):
    """Full-size model (T = 243, K = 5, C = 512, 8 layers), split precision, train-mode forward with injected DropPath masks + loss + backward at
    the reference's batch sizes: the planner (gemm_tile = 0) against the large tile everywhere (gemm_tile = 256).  Poses, scores, the four loss terms
    and the whole flat gradient are bit-identical, and the planner run did launch the 128-wide tile - more often than the 256 run, whose only
    128-wide launches are the narrow layers no large tile serves."""
    model = _full_model(f16f8, B, train=True)
    masks = _masks(model._engine.mask_layout(B))
    X, y = orc.synthetic_batch(B, 243, seed=42)
    X, y = X.cuda(), y.cuda()
    try:
        set_tile(lib, 0)
        a, na = _train_step_bits(lib, model, X, y, masks)
        set_tile(lib, 256)
        b, nb = _train_step_bits(lib, model, X, y, masks)
    finally:
        set_tile(lib, 0)
    print(f"\n[small batch] f16f8={f16f8} B={B}: launches (persistent 256, tiled 256, tiled 128) planner {na}, gemm_tile=256 {nb}")
    assert na[2] > 0 and na[2] > nb[2], (na, nb)
    for name, p, q in zip(("poses", "scores", "loss terms", "flat gradient"), a, b):
        diff = (ints(p) != ints(q)).sum().item()
        assert diff == 0, f"{name}: {diff} of {p.numel()} elements differ between the planner and gemm_tile = 256"


def test_planner_path_eval_forward_gives_the_bits_of_the_large_tile_path(lib):
    """Inference forward at B = 3 (no backward follows: the GELU epilogues get Z = NULL), planner against gemm_tile = 256."""
    model = _full_model(3, 3, train=False)
    X, _ = orc.synthetic_batch(3, 243, seed=42)
    X = X.cuda()
    out = {}
    try:
        for tile in (0, 256):
            set_tile(lib, tile)
            counts(lib)
            with torch.no_grad():
                poses, scores = model(X)
            torch.cuda.synchronize()
            out[tile] = (poses.clone(), scores.clone(), counts(lib))
    finally:
        set_tile(lib, 0)
    assert out[0][2][2] > out[256][2][2], (out[0][2], out[256][2])
    for i in range(2):
        assert (ints(out[0][i]) != ints(out[256][i])).sum().item() == 0


def test_planner_path_B3_vs_cpu_oracle(lib):
    """The default path of a drop-in user at the reference's default batch (B = 3, planner on) against the fp32 CPU oracle, with the bounds of the
    full-size parity tests at the timed precision: MPJPE <= 1e-4 m, loss to 1e-3, every parameter's gradient cosine > 0.9999."""
    from manipose_amd.metrics import mpjpe_error, rmcl_training_loss
    cfg = orc.FULL_CFG
    st_ = orc.make_state(cfg, seed=3)
    model = _full_model(3, 3, train=False)
    X, y = orc.synthetic_batch(3, 243, seed=42)
    set_tile(lib, 0)
    counts(lib)
    poses, scores = model(X.cuda())
    total, _ = rmcl_training_loss(poses, scores, y.cuda())
    total.backward()
    torch.cuda.synchronize()
    n = counts(lib)
    assert n[2] > 0, n
    req = {k: v.clone().requires_grad_(True) for k, v in st_.items()}
    o_poses, o_scores = orc.rmcl_manifold_forward(X, req, orc.oracle_cfg(cfg))
    o_total, _ = orc.rmcl_training_loss(o_poses, o_scores, y)
    o_total.backward()
    mp = mpjpe_error(poses, o_poses.detach().cuda(), "average").item()
    cs = {k: _cos(p.grad.cpu(), req[k].grad) for k, p in model.named_parameters()}
    worst = min(cs.items(), key=lambda kv: kv[1])
    wc, wck, mean, wm, wmk = _grad_report(model.named_parameters(), {k: v.grad for k, v in req.items()})
    print(f"\n[small batch] B=3 planner vs oracle: MPJPE {mp * 1e3:.5f} mm, loss {total.item():.6f} vs {o_total.item():.6f}, gradient cosine worst "
          f"{worst[1]:.6f} at {worst[0]}, mean {mean:.6f}; launches {n}")
    assert mp <= MPJPE_TOL_M
    close(scores, o_scores.detach(), rtol=1e-3, atol=1e-5)
    assert abs(total.item() - o_total.item()) <= 1e-3 * abs(o_total.item())
    assert worst[1] >= 0.9999, worst

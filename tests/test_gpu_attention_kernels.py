"""Kernel-level tests of every attention form, each through its C entry point (include/manipose_hip.h), against fp64 element by element.

The reference, the per-element error scales, the input families and what a bound of this module must reject are in tests/attn_ref.py and
tests/test_attn_check_host.py (the checker is itself tested there, on the CPU, with the constants below).  Every output element - none
excluded - is asserted against ITS OWN scale:  |got - fp64| <= C (unit m + 2^-24 ml), unit = 2^-8 for the bf16 forms and 2^-24 for the fp32
row kernels and for every log-sum-exp.  Outputs are pre-filled with NaN (an element the kernel never writes fails), inputs and outputs are
views into larger allocations whose guard rows hold NaN (inputs) or a sentinel that must be untouched afterwards (outputs), and the backward
is fed the kernel's own forward O and lse, as the engine feeds it.

Which kernel a shape reaches (attention.hip attn_fwd / attn_bwd, attention_mfma.hip attn_tmfma_supported / attn_smfma_supported /
attn_x3_needs_scratch) is restated in route() / x3_route() and asserted for every parametrisation that is about a kernel.

Constants (C_* below): the worst error / scale ratio measured on the MI355X over this module -> asserted at about 2.5 x, two digits; split per
form only where the measurements differ by more than a factor of two:
  lse  (2^-24, every form) ....... MFMA 2.65, bf16 rows 3.83, fp32 rows 3.41 -> 9.6      split precision (lo x lo dropped) 27.9 -> 70
  O    (2^-8, bf16 forms) ........ MFMA 1.75, rows 0.98 -> 4.4                           fp32 rows (2^-24) 3.29 -> 8.2
  dQ ............................. MFMA 0.585, rows 0.409 -> 1.5                         fp32 rows 1.16 -> 2.9
  dK ............................. MFMA 1.1 -> 2.8; bf16 rows 0.419 -> 1.0               fp32 rows 0.573 -> 1.4
  dV ............................. MFMA 1.82, rows 0.98 -> 4.6                           fp32 rows 1.91 -> 4.8
  delta (row kernels only) ....... bf16 rows 0.595 -> 1.5                                fp32 rows 1.05 -> 2.6
  split-precision O .............. C_ATTN = 0.25 of test_gpu_f16f8_kernels.py unchanged (0.239 at the worst here)
(the CPU rounding model of attn_ref.py had predicted O 1.5, dQ 0.49, dK 0.61, dV 1.9 for the MFMA kernels)
"""
import hashlib
import json
import os
import zlib

import numpy as np
import pytest
import torch

import attn_ref as ar
from test_gpu_f16f8_kernels import C_ATTN, decode_planar
from test_gpu_parity import st

pytestmark = pytest.mark.gpu

# (measured worst ratio on the MI355X over this module's shapes -> asserted bound; one constant for two forms wherever their measurements are
# within a factor of two of each other, the larger measurement then decides)
#   lse: 2^-24 (max_j scale |q| . |k_j| + |lse|); O: unit P |V|; dQ / dK: unit scale mag(dS) |K| / mag(dS)^T |Q|; dV: unit P^T |dO|;
#   delta: unit sum |dO| (P |V|); mag(dS) = P (|dO| |V|^T + sum |dO| (P |V|)); + 2^-24 x the logit-error share of each (attn_ref.py)
C_LSE = 9.6           # every form: mfma 2.65, bf16 rows 3.83, fp32 rows 3.41 -> 9.6
C_O = 4.4             # bf16 forms (unit 2^-8): mfma 1.75, rows 0.98 -> 4.4
C_DQ = 1.5            # bf16 forms: mfma 0.585, rows 0.409 -> 1.5
C_DK = 2.8            # bf16 MFMA kernels: 1.1 -> 2.8
C_DK_ROW = 1.0        # bf16 row kernels (fp32 arithmetic, one rounding at the store): 0.419 -> 1.0
C_DV = 4.6            # bf16 forms: mfma 1.82, rows 0.98 -> 4.6
C_DELTA_ROW = 1.5     # bf16 row kernels (delta from the stored bf16 O): 0.595 -> 1.5
BOUNDS = {
    "mfma": dict(lse=C_LSE, O=C_O, dq=C_DQ, dk=C_DK, dv=C_DV),
    "row_bf16": dict(lse=C_LSE, O=C_O, dq=C_DQ, dk=C_DK_ROW, dv=C_DV, delta=C_DELTA_ROW),
    # fp32 row kernels (unit 2^-24): O 3.29 -> 8.2, dQ 1.16 -> 2.9, dK 0.573 -> 1.4, dV 1.91 -> 4.8, delta 1.05 -> 2.6
    "row_f32": dict(lse=C_LSE, O=8.2, dq=2.9, dk=1.4, dv=4.8, delta=2.6),
}
# split-precision forward.  O: C_ATTN = 0.25 of test_gpu_f16f8_kernels.py, unchanged (measured here: 0.239 at the worst, spatial J = 16, C = 512).
# lse in 2^-24 units: the lo x lo products are left out (2^-18 of |q| . |k| at the most, 64 units): 27.9 -> 70
C_LSE_X3 = 70.0


def lib_():
    from manipose_amd import _lib
    return _lib


def check(name, form, ratios):
    """prints every worst ratio next to its bound, then asserts all of them"""
    b = BOUNDS[form]
    print(f"[attention kernels] {name} ({form}): " + ", ".join(f"{k} {v:.3g} (<= {b[k]})" for k, v in ratios.items()))
    bad = {k: (v, b[k]) for k, v in ratios.items() if not v <= b[k]}
    assert not bad, (name, form, bad)


# ------------------------------------------------------------------------------------------------ dispatch, restated
def route(storage, temporal, T, J, C, H):
    D = C // H
    if storage != "bf16" or C % 8:
        return "row"
    if temporal:
        return "mfma" if T <= 256 and D in (64, 16) else "row"
    return "mfma" if 16 <= J <= 32 and D in (64, 16) and 1 <= H <= 8 else "row"


def x3_route(temporal, T, J, C, H, two_phase=True):
    D = C // H
    if temporal:
        if not (T <= 256 and D in (64, 16) and C % 8 == 0):
            return "scratch"
        return "x3p" if D == 64 and T > 128 and two_phase and (2 * C) % 128 == 0 else "x3"
    ok = 16 <= J <= 32 and D in (64, 16) and 1 <= H <= 8 and C % 8 == 0 and 2 * J * (6 * C + 16) <= 160 * 1024 and J * (6 * C // 16) <= 7 * H * 64
    return "x3" if ok else "scratch"


# ------------------------------------------------------------------------------------------------ guarded buffers
SENT = -1234.0


class Buf:
    """a tensor that is a view into a larger allocation: two guard rows of its own width on each side (1-D: 8 elements), so that the
    16-byte alignment of its rows holds; input guards hold NaN, output guards a sentinel that untouched() looks for afterwards"""

    def __init__(self, shape, dtype, src=None):
        n = 1
        for s in shape:
            n *= s
        self.g = 2 * (shape[-1] if len(shape) > 1 else 4)
        assert (self.g * torch.empty(0, dtype=dtype).element_size()) % 16 == 0, (shape, dtype)
        self.full = torch.full((n + 2 * self.g,), float("nan") if src is not None else SENT, device="cuda", dtype=dtype)
        self.t = self.full[self.g:self.g + n].view(*shape)
        if src is not None:
            self.t.copy_(src.to(dtype))
        else:
            self.t.fill_(float("nan"))

    def ptr(self):
        return self.t.data_ptr()

    def untouched(self, what):
        lo, hi = self.full[:self.g].cpu(), self.full[-self.g:].cpu()
        want = torch.full_like(lo, SENT)
        assert torch.equal(lo, want) and torch.equal(hi, want), f"{what}: a guard row was written"


def ptr(b):
    return b.ptr() if b is not None else None


# ------------------------------------------------------------------------------------------------ runners
def run(lib, storage, temporal, B, T, J, C, H, qkv_t, dout_t, qk_scale=0.0, out_f16=0, gsc=None, backward=True):
    """forward (+ backward on the kernel's own O and lse) through the C entry points; returns the raw outputs on the host"""
    _lib = lib_()
    dt = torch.float32 if storage == "f32" else torch.bfloat16
    M, L = B * T * J, B * J * H * T
    qd, dod = Buf((M, 3 * C), dt, qkv_t), Buf((M, C), dt, dout_t)
    out = Buf((M, C), dt)
    lse = Buf((L,), torch.float32) if temporal else None
    ex = qk_scale != 0.0 or gsc is not None
    if storage == "f32":
        assert not ex and not out_f16
        _lib.check(lib.mp_attention_fwd(qd.ptr(), out.ptr(), ptr(lse), temporal, B, T, J, C, H, st()), "mp_attention_fwd")
    elif ex:
        _lib.check(lib.mp_attention_fwd_bf16_scale_ex(qd.ptr(), out.ptr(), ptr(lse), temporal, B, T, J, C, H, qk_scale, st()), "mp_attention_fwd_bf16_scale_ex")
    else:
        _lib.check(lib.mp_attention_fwd_bf16(qd.ptr(), out.ptr(), ptr(lse), temporal, B, T, J, C, H, st()), "mp_attention_fwd_bf16")
    res = dict(out=out.t.cpu(), lse=lse.t.cpu() if temporal else None)
    bufs = [("out", out), ("lse", lse)]
    if backward:
        o_in = Buf((M, C), torch.float16, out.t) if out_f16 else out
        delta = Buf((L,), torch.float32) if temporal else None
        dq = Buf((M, 3 * C), torch.float16 if gsc is not None else dt)
        if storage == "f32":
            _lib.check(lib.mp_attention_bwd(qd.ptr(), o_in.ptr(), dod.ptr(), ptr(lse), ptr(delta), dq.ptr(), temporal, B, T, J, C, H, st()), "mp_attention_bwd")
        elif ex:
            _lib.check(lib.mp_attention_bwd_bf16_scale_ex(qd.ptr(), o_in.ptr(), dod.ptr(), ptr(lse), ptr(delta), dq.ptr(), temporal, B, T, J, C, H, out_f16,
                                                          qk_scale, ptr(gsc), st()), "mp_attention_bwd_bf16_scale_ex")
        else:
            _lib.check(lib.mp_attention_bwd_bf16_ex(qd.ptr(), o_in.ptr(), dod.ptr(), ptr(lse), ptr(delta), dq.ptr(), temporal, B, T, J, C, H, out_f16, st()),
                       "mp_attention_bwd_bf16_ex")
        res.update(dqkv=dq.t.cpu(), delta=delta.t.cpu() if temporal else None)
        bufs += [("dqkv", dq), ("delta", delta)]
    torch.cuda.synchronize()
    for name, b in bufs:
        if b is not None:
            b.untouched(name)
    return res


def as_units(res, B, T, J, C, H, temporal, gscale=1.0):
    """raw outputs -> the quantities of attn_ref.reference, in units"""
    U = B * J * H if temporal else B * T * H
    got = dict(O=ar.to_units(res["out"].double(), B, T, J, H, temporal))
    if temporal:
        got["lse"] = res["lse"].double().reshape(U, T)
    if "dqkv" in res:
        dq, dk, dv = ar.split_qkv(res["dqkv"].double() / gscale, B, T, J, H, temporal)
        got.update(dq=dq, dk=dk, dv=dv)
        if temporal and not torch.isnan(res["delta"]).all():      # only the row kernels write delta; they write all of it
            got["delta"] = res["delta"].double().reshape(U, T)
    return got


def reference_of(qv, dv, B, T, J, C, H, temporal, scale=None):
    q, k, v = ar.split_qkv(qv, B, T, J, H, temporal)
    return ar.reference(q, k, v, ar.to_units(dv, B, T, J, H, temporal), (C // H) ** -0.5 if scale is None else scale)


def one_case(lib, family, storage, temporal, B, T, J, C, H, seed, qk_scale=0.0, out_f16=0, want_route=None):
    form = route(storage, temporal, T, J, C, H)
    if want_route is not None:
        assert form == want_route, (form, want_route)
    form = "mfma" if form == "mfma" else ("row_f32" if storage == "f32" else "row_bf16")
    scale = qk_scale if qk_scale else None
    (qv, qt), (dv, dt) = ar.make_inputs(family, B, T, J, C, H, temporal, storage, seed, scale=scale)
    ref = reference_of(qv, dv, B, T, J, C, H, temporal, scale)
    if family == "negative":
        assert ref[0]["S"].max().item() <= -8.0, ref[0]["S"].max().item()
    res = run(lib, storage, temporal, B, T, J, C, H, qt[0], dt[0], qk_scale=qk_scale, out_f16=out_f16)
    got = as_units(res, B, T, J, C, H, temporal)
    if form != "mfma" and temporal:
        assert "delta" in got, "the row kernels write delta"
    keys = ("lse", "O", "dq", "dk", "dv", "delta")
    r = ar.ratios(got, ref, ar.U24 if storage == "f32" else ar.U8, keys)
    name = f"{'temporal' if temporal else 'spatial'} {family} B={B} T={T} J={J} C={C} H={H}" + (f" scale={qk_scale:.4g}" if qk_scale else "") + \
        (" fp16 O" if out_f16 else "")
    check(name, form, r)
    return res, ref


# ------------------------------------------------------------------------------------------------ temporal MFMA, bf16
T_EDGES = (1, 15, 16, 17, 31, 32, 33, 64, 65, 81, 112, 113, 128, 129, 240, 241, 243, 255, 256)


@pytest.mark.parametrize("T", T_EDGES)
@pytest.mark.parametrize("D", [64, 16])
def test_temporal_mfma_forward_backward(lib, D, T):
    """attn_tmfma_fwd_kernel<D, 0> and attn_tmfma_bwd_kernel<D, NTC, false> (NTC = 16 for T > 240, else 0): 16-frame strips, the 32-frame
    rounding of the LDS images, (ntile + 1) / 2 forward waves up to 8 strips, the backward's 4 waves for 5-7 strips; b and j strides non-trivial.
    T = 1: dQ = dK = 0 and dV = dO in the reference, and the kernel within the bounds of that."""
    B, J, H = 2, 3, 2
    C = D * H
    families = ar.FAMILIES if T in (17, 81, 243) else ("randn", "negative")
    for i, family in enumerate(families):
        _, ref = one_case(lib, family, "bf16", 1, B, T, J, C, H, seed=1000 * i + T + D, want_route="mfma")
        if T == 1:
            (_, _), (dv, _) = ar.make_inputs(family, B, T, J, C, H, 1, "bf16", 1000 * i + T + D)
            assert ref[0]["dq"].abs().max() <= 1e-13 and ref[0]["dk"].abs().max() <= 1e-13      # (dP and delta: two summation orders of one sum)
            assert torch.equal(ref[0]["dv"], ar.to_units(dv, B, T, J, H, 1))


@pytest.mark.parametrize("T", [17, 243])
def test_temporal_mfma_backward_reads_O_from_the_fp16_plane(lib, T):
    """out_f16 = 1 (mp_model_config::f16f8 = 3): the same bounds"""
    for i, family in enumerate(("randn", "peaked", "negative")):
        one_case(lib, family, "bf16", 1, 2, T, 3, 128, 2, seed=77 + i + T, out_f16=1, want_route="mfma")


# ------------------------------------------------------------------------------------------------ temporal row kernels
@pytest.mark.parametrize("storage", ["f32", "bf16"])
@pytest.mark.parametrize("T,C,H", [(15, 64, 2), (16, 64, 2), (17, 64, 2), (81, 64, 2), (17, 8, 2), (17, 16, 2), (257, 128, 2), (300, 64, 1), (513, 64, 1)])
def test_temporal_row_kernels(lib, storage, T, C, H):
    """attn_temporal_fwd_kernel / attn_temporal_bwd_dq_kernel / attn_temporal_bwd_dkv_kernel<D, float | bf16>: head dim 32 (no MFMA form),
    4 and 8, and head dim 64 beyond 256 frames (grid.y blocks of 256 queries / keys); delta is compared too."""
    B, J = (2, 3) if T < 100 else (1, 2)
    for i, family in enumerate(("randn", "peaked", "negative")):
        one_case(lib, family, storage, 1, B, T, J, C, H, seed=31 * i + T + C, want_route="row")


# ------------------------------------------------------------------------------------------------ spatial MFMA, bf16
@pytest.mark.parametrize("J", [16, 17, 31, 32])
@pytest.mark.parametrize("D,H", [(64, 1), (64, 8), (16, 8)])
def test_spatial_mfma_forward_backward(lib, D, H, J):
    """attn_smfma_fwd_kernel<D> / attn_smfma_bwd_kernel<D, false>, 5 frames.  The padding lanes of the 32-token tiles hold clamped duplicates
    of the last token: under `negative` a duplicate that is not masked to exactly 0 takes a visible share of the row."""
    for i, family in enumerate(ar.FAMILIES):
        one_case(lib, family, "bf16", 0, 1, 5, J, D * H, H, seed=17 * i + J + D + H, want_route="mfma")


# ------------------------------------------------------------------------------------------------ spatial row kernels
@pytest.mark.parametrize("storage", ["f32", "bf16"])
@pytest.mark.parametrize("J,C,H", [(2, 64, 2), (15, 64, 2), (17, 64, 2), (17, 256, 16)])
def test_spatial_row_kernels(lib, storage, J, C, H):
    """attn_spatial_fwd_kernel / attn_spatial_bwd_kernel<WPB, float | bf16>: head dim 32, fewer than 16 tokens, and 16 heads (more than the
    8 waves of the MFMA form; 4 x 4.6 KB / 2 x 9.4 KB of LDS)"""
    for i, family in enumerate(("randn", "peaked", "negative")):
        one_case(lib, family, storage, 0, 1, 5, J, C, H, seed=13 * i + J + C, want_route="row")


@pytest.mark.parametrize("storage", ["f32", "bf16"])
def test_spatial_attention_refuses_more_than_32_tokens(lib, storage):
    """J = 33 is MP_ERR_ARG in both directions (the row kernels keep a token per lane of half a wave)"""
    _lib = lib_()
    B, T, J, C, H = 1, 2, 33, 64, 2
    dt = torch.float32 if storage == "f32" else torch.bfloat16
    q, o, dq = (torch.zeros(B * T * J, w, device="cuda", dtype=dt) for w in (3 * C, C, 3 * C))
    fwd, bwd = (lib.mp_attention_fwd, lib.mp_attention_bwd) if storage == "f32" else (lib.mp_attention_fwd_bf16, lib.mp_attention_bwd_bf16)
    with pytest.raises(RuntimeError, match="unsupported"):
        _lib.check(fwd(q.data_ptr(), o.data_ptr(), None, 0, B, T, J, C, H, st()))
    with pytest.raises(RuntimeError, match="unsupported"):
        _lib.check(bwd(q.data_ptr(), None, o.data_ptr(), None, None, dq.data_ptr(), 0, B, T, J, C, H, st()))


# ------------------------------------------------------------------------------------------------ split-precision forward
def x3_forward(lib, temporal, B, T, J, C, H, family, seed, qk_scale=0.0, want_route=None):
    """mp_attention_fwd_bf16x3_ex (planar output): O per element against C_ATTN x the split-precision scale, lse per element"""
    _lib = lib_()
    if want_route is not None:
        assert x3_route(temporal, T, J, C, H) == want_route, (x3_route(temporal, T, J, C, H), want_route)
    scale = qk_scale if qk_scale else None
    (qv, (qh, ql)), (dv, _) = ar.make_inputs(family, B, T, J, C, H, temporal, "planar", seed, scale=scale)
    ref = reference_of(qv, dv, B, T, J, C, H, temporal, scale)
    M, L = B * T * J, B * J * H * T
    qhd, qld = Buf((M, 3 * C), torch.bfloat16, qh), Buf((M, 3 * C), torch.bfloat16, ql)
    oh, ol = Buf((M, C), torch.bfloat16), Buf((M, C), torch.bfloat16)
    lse = Buf((L,), torch.float32) if temporal else None
    scratch = torch.empty(4 * M * C, device="cuda") if x3_route(temporal, T, J, C, H) == "scratch" else None
    sp = scratch.data_ptr() if scratch is not None else None
    if qk_scale:
        _lib.check(lib.mp_attention_fwd_bf16x3_scale_ex(qhd.ptr(), qld.ptr(), oh.ptr(), ol.ptr(), ptr(lse), sp, temporal, B, T, J, C, H, 0, qk_scale, st()))
    else:
        _lib.check(lib.mp_attention_fwd_bf16x3_ex(qhd.ptr(), qld.ptr(), oh.ptr(), ol.ptr(), ptr(lse), sp, temporal, B, T, J, C, H, 0, st()))
    torch.cuda.synchronize()
    for name, b in (("out_hi", oh), ("out_lo", ol), ("lse", lse)):
        if b is not None:
            b.untouched(name)
    got = ar.to_units(decode_planar(oh.t.cpu(), ol.t.cpu()), B, T, J, H, temporal)
    r = ((got - ref[0]["O"]).abs() / ar.x3_scale(ref))
    r = torch.where(torch.isfinite(got), r, torch.full_like(r, float("inf"))).max().item()
    name = f"[attention kernels] split precision {'temporal' if temporal else 'spatial'} {family} B={B} T={T} J={J} C={C} H={H}" + \
        (f" scale={qk_scale:.4g}" if qk_scale else "")
    rl = ar.ratios(dict(lse=lse.t.cpu().double()), ref, ar.U24, ("lse",))["lse"] if temporal else 0.0
    print(f"{name}: O {r:.3g} (<= {C_ATTN}), lse {rl:.3g} (<= {C_LSE_X3})")
    assert r <= C_ATTN and rl <= C_LSE_X3, (name, r, rl)
    return oh.t.cpu(), ol.t.cpu(), lse.t.cpu() if temporal else None


@pytest.mark.parametrize("T", [17, 81, 243])
def test_split_precision_temporal_head_dim_16(lib, T):
    """attn_tmfma_fwd_x3_kernel<16, FULL> (FULL: 16 key tiles, T > 240)"""
    for i, family in enumerate(("randn", "negative")):
        x3_forward(lib, 1, 2, T, 3, 32, 2, family, seed=5 * i + T, want_route="x3")


@pytest.mark.parametrize("T", [128, 129, 240, 241, 256])
def test_split_precision_temporal_head_dim_64_both_kernels(lib, T):
    """T <= 128: attn_tmfma_fwd_x3_kernel<64>; beyond: attn_tmfma_fwd_x3p_kernel<FULL> (two-phase) and, with the option off, the one-strip
    kernel again - same log-sum-exp and hi plane bit for bit (test_bf16x3_attention_forward), both within the bound here"""
    _lib = lib_()
    B, J, C, H = 2, 3, 128, 2
    for i, family in enumerate(("randn", "negative")):
        a = x3_forward(lib, 1, B, T, J, C, H, family, seed=9 * i + T, want_route="x3p" if T > 128 else "x3")
        _lib.check(lib.mp_set_option(b"attn_two_phase", 0))
        try:
            assert x3_route(1, T, J, C, H, two_phase=False) == "x3"
            b = x3_forward(lib, 1, B, T, J, C, H, family, seed=9 * i + T)
        finally:
            _lib.check(lib.mp_set_option(b"attn_two_phase", 1))
        assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2])


@pytest.mark.parametrize("J,C,H,want", [(16, 128, 8, "x3"), (31, 128, 8, "x3"), (32, 128, 8, "x3"), (16, 512, 8, "x3"), (17, 64, 1, "x3"),
                                        (31, 512, 8, "scratch"), (32, 64, 1, "scratch")])
def test_split_precision_spatial(lib, J, C, H, want):
    """attn_smfma_fwd_x3_kernel<16 | 64>; head dim 64 beyond 18 tokens does not fit the kernel's register prefetch (J 6C / 16 <= 7 H 64) and
    takes the fp32 route through the scratch (join_planes, attn_spatial_fwd_kernel<float>, split_planes)"""
    for i, family in enumerate(("randn", "negative")):
        x3_forward(lib, 0, 1, 5, J, C, H, family, seed=3 * i + J + C, want_route=want)


@pytest.mark.parametrize("form", ["x3", "x3p", "spatial"])
def test_split_precision_persistent_kernels_loop_over_more_units_than_workgroups(lib, form):
    """grid = min(units, CUs x per_cu): a unit count above the grid and no multiple of it, so that workgroups run different numbers of units
    (the prefetch of the next unit's images behind the last one included)"""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    if form == "x3":            # attn_tmfma_fwd_x3_kernel<16>: 6 KB of LDS, 4 workgroups per CU
        B, T, J, C, H = 1, 32, cus // 2 + 1, 128, 8
        assert B * J * H > 4 * cus and (B * J * H) % (4 * cus)
        x3_forward(lib, 1, B, T, J, C, H, "randn", seed=1, want_route="x3")
    elif form == "x3p":         # attn_tmfma_fwd_x3p_kernel<false>: one workgroup per CU
        B, T, J, C, H = 1, 129, cus // 2 + 1, 128, 2
        assert B * J * H > cus and (B * J * H) % cus
        x3_forward(lib, 1, B, T, J, C, H, "randn", seed=2, want_route="x3p")
    else:                       # attn_smfma_fwd_x3_kernel<16>: 26 KB of LDS, 4 workgroups per CU
        B, T, J, C, H = 1, 4 * cus + 7, 17, 128, 8
        x3_forward(lib, 0, B, T, J, C, H, "negative", seed=3, want_route="x3")


# ------------------------------------------------------------------------------------------------ unit independence
@pytest.mark.parametrize("temporal,T,J,C,H", [(1, 81, 3, 128, 2), (0, 5, 17, 128, 2)])
def test_units_are_independent_bit_for_bit(lib, temporal, T, J, C, H):
    """the results of batch item 0 do not change by a bit when item 1's inputs are replaced by other data (MFMA kernels, forward and backward)"""
    B = 2
    assert route("bf16", temporal, T, J, C, H) == "mfma"
    (_, (q1,)), (_, (d1,)) = ar.make_inputs("randn", B, T, J, C, H, temporal, "bf16", 11)
    (_, (q2,)), (_, (d2,)) = ar.make_inputs("peaked", B, T, J, C, H, temporal, "bf16", 12)
    n = T * J
    q2[:n], d2[:n] = q1[:n], d1[:n]
    a = run(lib, "bf16", temporal, B, T, J, C, H, q1, d1)
    b = run(lib, "bf16", temporal, B, T, J, C, H, q2, d2)
    assert torch.equal(a["out"][:n].view(torch.int16), b["out"][:n].view(torch.int16))
    assert torch.equal(a["dqkv"][:n].view(torch.int16), b["dqkv"][:n].view(torch.int16))
    assert not torch.equal(a["out"][n:].view(torch.int16), b["out"][n:].view(torch.int16))
    if temporal:
        nl = J * H * T
        assert torch.equal(a["lse"][:nl].view(torch.int32), b["lse"][:nl].view(torch.int32))


# ------------------------------------------------------------------------------------------------ softmax scale override
@pytest.mark.parametrize("temporal,T,J,C,H", [(1, 81, 3, 128, 2), (0, 5, 17, 128, 2), (1, 33, 3, 32, 2)])
@pytest.mark.parametrize("which", ["mup", "arbitrary"])
def test_softmax_scale_override(lib, which, temporal, T, J, C, H):
    """a softmax scale other than head_dim ** -0.5 (mp_model_config::qk_scale; muP: 1 / head_dim) through mp_attention_{fwd,bwd}_bf16_scale_ex
    and mp_attention_fwd_bf16x3_scale_ex: against the reference with THAT scale, within the same constants"""
    D = C // H
    qk = 1.0 / D if which == "mup" else 0.173
    for i, family in enumerate(("randn", "peaked")):
        one_case(lib, family, "bf16", temporal, 2, T, J, C, H, seed=41 + i + T, qk_scale=qk, want_route="mfma")
        x3_forward(lib, temporal, 2, T, J, C, H, family, seed=43 + i + T, qk_scale=qk, want_route="x3")
    # 0 = the default, and the override does not outlive its call
    one_case(lib, "randn", "bf16", temporal, 2, T, J, C, H, seed=5)


# ------------------------------------------------------------------------------------------------ scaled-fp16 gradient forms
def gsc_block(S):
    """the engine's gradient-scale block (elementwise.hip grad_scale_kernel): {S, 1 / S, scratch, 1, clamped (u32), non-finite (u32), -, -}"""
    b = Buf((8,), torch.float32, torch.tensor([S, 1.0 / S, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0]))
    return b


@pytest.mark.parametrize("temporal,T,J,C,H", [(1, 243, 2, 128, 2), (0, 5, 17, 128, 2)])
def test_fp16_gradient_forms(lib, temporal, T, J, C, H):
    """attn_tmfma_bwd_kernel<64, 16, true> / attn_smfma_bwd_kernel<64, true> (mp_model_config::f16_backward): dQ / dK / dV as fp16 of S x value.
    (a) a moderate S: stored / S within the bf16 form's bounds, both counters 0; (b) an S that lifts about a tenth of the elements over 65504:
    those hold +-65504, never inf, the clamped counter lies in the interval the reference allows (an element within its error bound of the
    threshold may fall either way) and in the much narrower one that the kernel's own values of (a) allow, the non-finite counter stays 0."""
    B = 1
    assert route("bf16", temporal, T, J, C, H) == "mfma"
    (qv, (qt,)), (dv, (dt,)) = ar.make_inputs("randn", B, T, J, C, H, temporal, "bf16", 7 + T)
    ref = reference_of(qv, dv, B, T, J, C, H, temporal)
    val, m, ml = ref
    want = ar.join_qkv(val["dq"], val["dk"], val["dv"], B, T, J, H, temporal)
    b = BOUNDS["mfma"]
    bound = ar.join_qkv(*(b[k] * (ar.U8 * m[k] + ar.U24 * ml[k]) for k in ("dq", "dk", "dv")), B, T, J, H, temporal)
    # (a)
    S = 16.0
    gsc = gsc_block(S)
    res = run(lib, "bf16", temporal, B, T, J, C, H, qt, dt, gsc=gsc)
    check(f"fp16 gradients S={S} temporal={temporal}", "mfma", ar.ratios(as_units(res, B, T, J, C, H, temporal, gscale=S), ref, ar.U8))
    own = res["dqkv"].double().abs() / S          # the kernel's own values to 2^-11 (fp16 of S x value, far above fp16's subnormals where it matters)
    cnt = gsc.t[4:6].cpu().view(torch.int32)
    assert cnt.tolist() == [0, 0], cnt
    assert torch.equal(gsc.t[:4].cpu(), torch.tensor([S, 1.0 / S, 0.0, 1.0]))
    # (b)
    q90 = want.abs().flatten().kthvalue(int(0.9 * want.numel())).values.item()
    S = 2.0 ** round(torch.log2(torch.tensor(65504.0 / q90)).item())
    gsc = gsc_block(S)
    res = run(lib, "bf16", temporal, B, T, J, C, H, qt, dt, gsc=gsc)
    got = res["dqkv"].double()
    assert torch.isfinite(got).all(), "a saturating store wrote inf / NaN"
    sure = S * (want.abs() - bound) > 65504.0
    free = S * (want.abs() + bound) < 65504.0
    maybe = ~sure & ~free
    n_sure, n_maybe = int(sure.sum()), int(maybe.sum())
    assert n_sure > 0.03 * want.numel(), (n_sure, n_maybe)
    assert (got[sure] == 65504.0 * torch.sign(want[sure])).all(), "an element beyond the fp16 range was not clamped"
    assert ((got[maybe].abs() == 65504.0) | ((got[maybe] / S - want[maybe]).abs() <= bound[maybe])).all()
    assert ((got[free] / S - want[free]).abs() <= bound[free]).all()
    cnt = gsc.t[4:6].cpu().view(torch.int32).tolist()
    n_clamped = int((got.abs() == 65504.0).sum())
    print(f"[attention kernels] fp16 gradients S={S:g} temporal={temporal}: clamped {cnt[0]} (reference: {n_sure} .. {n_sure + n_maybe}), non-finite {cnt[1]}")
    assert n_sure <= cnt[0] <= n_sure + n_maybe and cnt[1] == 0, (cnt, n_sure, n_maybe)
    assert cnt[0] <= n_clamped          # (an element that rounds to 65504 without exceeding it is stored as 65504 and not counted)
    # the reference's interval is as wide as the error bound at the threshold; the kernel's own values of run (a) pin the store itself: the same fp32
    # value times another power of two, known to fp16's 2^-11
    sure2, free2 = S * own * (1 - 2.0 ** -10) > 65504.0, S * own * (1 + 2.0 ** -10) < 65504.0
    n2, m2 = int(sure2.sum()), int((~sure2 & ~free2).sum())
    print(f"  against the kernel's own unsaturated values: {n2} .. {n2 + m2}")
    assert m2 < 0.05 * n2 and n2 <= cnt[0] <= n2 + m2, (cnt, n2, m2)
    assert (got[sure2].abs() == 65504.0).all() and ((got[free2].abs() / S - own[free2]).abs() <= 2.0 ** -10 * own[free2] + 2.0 ** -28).all()


def test_fp16_gradients_are_refused_where_a_row_kernel_would_write_bf16(lib):
    _lib = lib_()
    gsc = gsc_block(16.0)
    for temporal, T, J, C, H in ((1, 300, 2, 128, 2), (1, 17, 2, 64, 2), (0, 5, 15, 128, 2), (0, 5, 17, 256, 16)):
        assert route("bf16", temporal, T, J, C, H) == "row"
        M, L = 2 * T * J, 2 * J * H * T
        q, dq = (torch.zeros(M, 3 * C, device="cuda", dtype=torch.bfloat16) for _ in range(2))
        o, do = (torch.zeros(M, C, device="cuda", dtype=torch.bfloat16) for _ in range(2))
        lse, delta = torch.zeros(L, device="cuda"), torch.zeros(L, device="cuda")
        with pytest.raises(RuntimeError, match="MFMA backward"):
            _lib.check(lib.mp_attention_bwd_bf16_scale_ex(q.data_ptr(), o.data_ptr(), do.data_ptr(), lse.data_ptr(), delta.data_ptr(), dq.data_ptr(), temporal,
                                                          2, T, J, C, H, 0, 0.0, gsc.ptr(), st()))
    with pytest.raises(RuntimeError, match="qk_scale"):
        _lib.check(lib.mp_attention_fwd_bf16_scale_ex(q.data_ptr(), o.data_ptr(), lse.data_ptr(), 0, 2, 5, 17, 256, 16, -1.0, st()))


# ------------------------------------------------------------------------------------------------ softmax scale on the routes without an MFMA kernel
def other_scale(which, D):
    return 1.0 / D if which == "mup" else 0.173


@pytest.mark.parametrize("temporal,T,J,C,H", [(0, 5, 32, 64, 1), (1, 257, 2, 32, 2)])
@pytest.mark.parametrize("which", ["mup", "arbitrary"])
def test_softmax_scale_through_the_split_precision_fallback(lib, which, temporal, T, J, C, H):
    """mp_attention_fwd_bf16x3_scale_ex on shapes no MFMA kernel covers (spatial: head dim 64 beyond the register prefetch; temporal: T > 256):
    join_planes, the fp32 row kernel, split_planes - the fp32 launch has to run with the caller's scale.  Same bounds as every split-precision
    forward; then the default scale on the same shape: nothing outlives the call."""
    qk = other_scale(which, C // H)
    for i, family in enumerate(("randn", "peaked")):
        x3_forward(lib, temporal, 1, T, J, C, H, family, seed=61 + i + T, qk_scale=qk, want_route="scratch")
    x3_forward(lib, temporal, 1, T, J, C, H, "randn", seed=5, want_route="scratch")


@pytest.mark.parametrize("temporal,T,J,C,H", [(1, 17, 2, 64, 2), (0, 5, 15, 128, 2)])
@pytest.mark.parametrize("which", ["mup", "arbitrary"])
def test_softmax_scale_through_the_bf16_row_kernels(lib, which, temporal, T, J, C, H):
    """mp_attention_{fwd,bwd}_bf16_scale_ex where the bf16 row kernels run (temporal: head dim 32; spatial: 15 tokens), forward and backward,
    against the reference with THAT scale within the row kernels' constants; then the default scale again"""
    qk = other_scale(which, C // H)
    for i, family in enumerate(("randn", "peaked")):
        one_case(lib, family, "bf16", temporal, 2, T, J, C, H, seed=67 + i + T, qk_scale=qk, want_route="row")
    one_case(lib, "randn", "bf16", temporal, 2, T, J, C, H, seed=5, want_route="row")


# ------------------------------------------------------------------------------------------------ bits
# Every public attention entry point once per route it reaches, on inputs from a seeded numpy generator; the SHA-256 of every output tensor's
# bytes is compared with tests/golden/attn_bits.json (tools/gen_golden_attn_bits.py: the recording and the test run the same code).
GOLD_BITS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "attn_bits.json")
#               temporal, B, T, J, C, H
BITS_SHAPES = {
    "s_row": (0, 2, 5, 15, 64, 2),       # spatial, 15 tokens, head dim 32: row kernels; split precision: scratch
    "s_d16": (0, 2, 5, 17, 32, 2),       # spatial MFMA, head dim 16
    "s_d64": (0, 2, 5, 17, 128, 2),      # spatial MFMA, head dim 64
    "t_row": (1, 2, 17, 3, 64, 2),       # temporal, head dim 32: row kernels; split precision: scratch
    "t_d16": (1, 2, 17, 3, 32, 2),       # temporal MFMA, head dim 16
    "t_d64": (1, 2, 17, 3, 128, 2),      # temporal MFMA, head dim 64; split precision: the one-strip kernel
    "t_d16_full": (1, 1, 241, 2, 32, 2),     # the full-window backward (T > 240)
    "t_d64_full": (1, 1, 241, 2, 128, 2),    # ... and the two-phase split-precision forward (x3p)
}
BITS_ROUTES = {"s_row": ("row", "scratch"), "s_d16": ("mfma", "x3"), "s_d64": ("mfma", "x3"), "t_row": ("row", "scratch"), "t_d16": ("mfma", "x3"),
               "t_d64": ("mfma", "x3"), "t_d16_full": ("mfma", "x3"), "t_d64_full": ("mfma", "x3p")}
QK_BITS = 0.173


def bits_table():
    """(entry point, shape, options) rows: qk = softmax scale, form = out_form (1: f16f8 planes), o16 = out_f16, S = gradient-scale block"""
    rows = []
    for s, (route_, _) in BITS_ROUTES.items():
        mfma, temporal, d64 = route_ == "mfma", BITS_SHAPES[s][0], BITS_SHAPES[s][4] // BITS_SHAPES[s][5] == 64
        if not mfma:
            rows += [("mp_attention_fwd", s, {}), ("mp_attention_bwd", s, {})]
        rows += [("mp_attention_fwd_bf16", s, {}), ("mp_attention_bwd_bf16", s, {}), ("mp_attention_bwd_bf16_ex", s, {}),
                 ("mp_attention_fwd_bf16_scale_ex", s, dict(qk=QK_BITS)), ("mp_attention_bwd_bf16_scale_ex", s, dict(qk=QK_BITS)),
                 ("mp_attention_fwd_bf16x3", s, {}), ("mp_attention_fwd_bf16x3_ex", s, {}), ("mp_attention_fwd_bf16x3_scale_ex", s, dict(qk=QK_BITS))]
        if mfma:
            rows += [("mp_attention_bwd_bf16_scale_ex", s, dict(S=16.0)), ("mp_attention_bwd_bf16_scale_ex", s, dict(qk=QK_BITS, S=16.0))]
        if mfma and temporal:
            rows += [("mp_attention_bwd_bf16_ex", s, dict(o16=1)), ("mp_attention_bwd_bf16_scale_ex", s, dict(qk=QK_BITS, S=16.0, o16=1))]
        if mfma and d64:
            rows += [("mp_attention_fwd_bf16x3_ex", s, dict(form=1)), ("mp_attention_fwd_bf16x3_scale_ex", s, dict(qk=QK_BITS, form=1))]
    return rows


def bits_name(entry, shape, opt):
    return "/".join([entry, shape] + [f"{k}={opt[k]:g}" for k in sorted(opt)])


def bits_outputs(lib, entry, shape, opt):
    """{tensor name: host tensor} of one row; outputs are pre-filled with 0 (the MFMA backward leaves delta alone)"""
    _lib = lib_()
    temporal, B, T, J, C, H = BITS_SHAPES[shape]
    qk, form, o16, S = opt.get("qk", 0.0), opt.get("form", 0), opt.get("o16", 0), opt.get("S")
    assert B <= 2 and J <= 17 and C <= 128
    rng = np.random.default_rng(zlib.crc32(shape.encode()))
    M, L = B * T * J, B * J * H * T
    qkv = torch.from_numpy(rng.standard_normal((M, 3 * C), dtype=np.float32))
    dout = torch.from_numpy(rng.standard_normal((M, C), dtype=np.float32))
    f32 = entry in ("mp_attention_fwd", "mp_attention_bwd")
    dt = torch.float32 if f32 else torch.bfloat16

    def zeros(*shape_, dtype=dt):
        return torch.zeros(*shape_, device="cuda", dtype=dtype)

    lse = zeros(L, dtype=torch.float32)
    lp = lse.data_ptr() if temporal else None
    dims = (temporal, B, T, J, C, H)
    if "x3" in entry:
        assert x3_route(temporal, T, J, C, H) == BITS_ROUTES[shape][1]
        hi = qkv.bfloat16()
        lo = (qkv - hi.float()).bfloat16()
        hi, lo, oh, ol = hi.cuda(), lo.cuda(), zeros(M, C), zeros(M, C)
        scratch = zeros(4 * M * C, dtype=torch.float32) if BITS_ROUTES[shape][1] == "scratch" else None
        tail = {"mp_attention_fwd_bf16x3": (), "mp_attention_fwd_bf16x3_ex": (form,), "mp_attention_fwd_bf16x3_scale_ex": (form, qk)}[entry]
        _lib.check(getattr(lib, entry)(hi.data_ptr(), lo.data_ptr(), oh.data_ptr(), ol.data_ptr(), lp, scratch.data_ptr() if scratch is not None else None,
                                       *dims, *tail, st()), entry)
        outs = dict(out_hi=oh, out_lo=ol)
    else:
        assert route("f32" if f32 else "bf16", temporal, T, J, C, H) == ("row" if f32 else BITS_ROUTES[shape][0])
        q, do, out = qkv.to(dt).cuda(), dout.to(dt).cuda(), zeros(M, C)
        fwd = "mp_attention_fwd" if f32 else ("mp_attention_fwd_bf16_scale_ex" if entry.endswith("_scale_ex") else "mp_attention_fwd_bf16")
        _lib.check(getattr(lib, fwd)(q.data_ptr(), out.data_ptr(), lp, *dims, *((qk,) if fwd.endswith("_scale_ex") else ()), st()), fwd)
        outs = dict(out=out)
        if "_bwd" in entry:
            o_in = out.to(torch.float16) if o16 else out
            delta = zeros(L, dtype=torch.float32)
            dq = zeros(M, 3 * C, dtype=torch.float16 if S else dt)
            gsc = torch.tensor([S, 1.0 / S, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0], device="cuda") if S else None
            tail = {"mp_attention_bwd": (), "mp_attention_bwd_bf16": (), "mp_attention_bwd_bf16_ex": (o16,),
                    "mp_attention_bwd_bf16_scale_ex": (o16, qk, gsc.data_ptr() if S else None)}[entry]
            _lib.check(getattr(lib, entry)(q.data_ptr(), o_in.data_ptr(), do.data_ptr(), lp, delta.data_ptr() if temporal else None, dq.data_ptr(), *dims, *tail,
                                           st()), entry)
            outs = dict(dqkv=dq)
            if temporal:
                outs["delta"] = delta
            if S:
                outs["gsc"] = gsc
    if temporal and "_bwd" not in entry:
        outs["lse"] = lse
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in outs.items()}


def bits_digests(lib):
    """{row / tensor: {"shape": [...], "sha256": hex}} over bits_table()"""
    out = {}
    for entry, shape, opt in bits_table():
        for k, t in bits_outputs(lib, entry, shape, opt).items():
            raw = t.contiguous().view(torch.uint8).numpy().tobytes()
            out[bits_name(entry, shape, opt) + "/" + k] = {"shape": list(t.shape), "sha256": hashlib.sha256(raw).hexdigest()}
    return out


def test_every_entry_point_repeats_the_recorded_bits(lib):
    """the launchers changed, the kernels and what they are given did not: every output of every entry point on every route has the bytes it had
    at the commit the fixture was recorded at (tools/gen_golden_attn_bits.py)"""
    with open(GOLD_BITS) as f:
        want = json.load(f)
    got = bits_digests(lib)
    assert len({e for e, _, _ in bits_table()}) == 10
    assert sorted(got) == sorted(want), sorted(set(got) ^ set(want))
    bad = [k for k in sorted(want) if got[k] != want[k]]
    assert not bad, "entry point / shape / options / tensor with other bits than recorded: " + ", ".join(bad)

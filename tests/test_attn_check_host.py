"""The attention checker is itself tested (CPU): with the constants the GPU module asserts, a CPU model of a bf16 MFMA kernel (fp64 with bf16
rounding at the kernel's rounding points, attn_ref.model_bf16) passes for every input family, every subtly wrong variant of it is rejected,
and the two faults that the tolerances of test_bf16_attention_forward_backward accept stay on record as accepted by those tolerances."""
import numpy as np
import pytest
import torch

import attn_ref as ar
from test_gpu_attention_kernels import BOUNDS

SHAPES = [(T, D) for T in (17, 81, 243) for D in (16, 64)]
B, J, H = 1, 2, 2


def case(family, T, D, storage="bf16", seed=0):
    C = D * H
    (qv, _), (dv, _) = ar.make_inputs(family, B, T, J, C, H, 1, storage, seed + T + D)
    q, k, v = ar.split_qkv(qv, B, T, J, H, 1)
    do = ar.to_units(dv, B, T, J, H, 1)
    return q, k, v, do, D ** -0.5


def passes(r, keys=("lse", "O", "dq", "dk", "dv")):
    return all(r[k] <= BOUNDS["mfma"][k] for k in keys)


@pytest.mark.parametrize("family", ar.FAMILIES)
def test_the_rounding_model_of_a_bf16_kernel_passes(family):
    for T, D in SHAPES:
        q, k, v, do, scale = case(family, T, D)
        ref = ar.reference(q, k, v, do, scale)
        if family == "negative":
            assert ref[0]["S"].max().item() <= -8.0
            assert ref[0]["P"].amax(-1).max().item() < 0.9          # ... and no row is degenerate
        if family == "large":
            assert ref[0]["S"].abs().max().item() > (55.0 if T == 243 else 30.0)      # (a short window draws fewer logits)
        r = ar.ratios(ar.model_bf16(q, k, v, do, scale), ref, ar.U8)
        print(f"[attention checker] model {family} T={T} D={D}: " + ", ".join(f"{k} {x:.3g}" for k, x in r.items()))
        assert passes(r), (family, T, D, r)
        assert min(ref[1][k].min().item() for k in ("lse", "O", "dq", "dk", "dv")) > 0.0, "an error scale of 0"


@pytest.mark.parametrize("fault", ar.FAULTS)
def test_every_faulty_kernel_is_rejected(fault):
    rejected = []
    for family in ar.FAMILIES:
        for T, D in SHAPES:
            q, k, v, do, scale = case(family, T, D)
            r = ar.ratios(ar.model_bf16(q, k, v, do, scale, fault=fault), ar.reference(q, k, v, do, scale), ar.U8)
            if not passes(r):
                rejected.append((family, T, D))
            if fault == "pad_key":                        # by the log-sum-exp alone, at every shape and family
                assert not passes(r, ("lse",)), (family, T, D, r)
    print(f"[attention checker] {fault}: rejected at {len(rejected)} of {len(ar.FAMILIES) * len(SHAPES)} cases")
    assert rejected, fault


def _cos(a, b):
    a, b = a.reshape(-1), b.reshape(-1)
    return float((a @ b) / (a.norm() * b.norm() + 1e-30))


@pytest.mark.parametrize("fault", ["pad_key", "dq_x1.03"])
def test_the_old_tolerances_accept_what_this_checker_rejects(fault):
    """fp64 with one fault and NO rounding, compared as test_bf16_attention_forward_backward compares (randn inputs, forward rtol = atol = 2e-2,
    backward cos > 0.999 and atol = 5e-2 max |grad|): accepted at T = 243 and T = 81; rejected here."""
    rejected = []
    for T, D in ((243, 64), (81, 64), (243, 16)):
        q, k, v, do, scale = case("randn", T, D)
        ref = ar.reference(q, k, v, do, scale)
        got = ar.model_bf16(q, k, v, do, scale, fault=fault, rounding=False)
        np.testing.assert_allclose(got["O"].numpy(), ref[0]["O"].numpy(), rtol=2e-2, atol=2e-2)
        g = torch.cat([got[x] for x in ("dq", "dk", "dv")], -1)
        w = torch.cat([ref[0][x] for x in ("dq", "dk", "dv")], -1)
        assert _cos(g, w) > 0.999
        np.testing.assert_allclose(g.numpy(), w.numpy(), rtol=5e-2, atol=5e-2 * float(w.abs().max()))
        for family in ar.FAMILIES:      # the same fault at the same shapes, under this module's inputs and bounds
            q, k, v, do, scale = case(family, T, D)
            if not passes(ar.ratios(ar.model_bf16(q, k, v, do, scale, fault=fault, rounding=False), ar.reference(q, k, v, do, scale), ar.U8)):
                rejected.append((family, T, D))
    assert rejected, fault


def test_the_explicit_backward_formulas_agree_with_autograd():
    for temporal, T, Jn, D, scale in ((1, 33, 2, 16, None), (0, 3, 17, 64, None), (1, 81, 1, 8, 0.3)):
        C = D * H
        (qv, _), (dv, _) = ar.make_inputs("peaked", 2, T, Jn, C, H, temporal, "f32", 5, scale=scale)
        sc = D ** -0.5 if scale is None else scale
        x = qv.clone().requires_grad_(True)
        q, k, v = ar.split_qkv(x, 2, T, Jn, H, temporal)
        out = ar.from_units(((q @ k.transpose(-2, -1)) * sc).softmax(-1) @ v, 2, T, Jn, H, temporal)
        (out * dv).sum().backward()
        q, k, v = ar.split_qkv(qv, 2, T, Jn, H, temporal)
        val, _, _ = ar.reference(q, k, v, ar.to_units(dv, 2, T, Jn, H, temporal), sc)
        mine = ar.join_qkv(val["dq"], val["dk"], val["dv"], 2, T, Jn, H, temporal)
        assert (ar.from_units(val["O"], 2, T, Jn, H, temporal) - out.detach()).abs().max() <= 1e-12 * out.abs().max()
        assert (mine - x.grad).abs().max() <= 1e-12 * x.grad.abs().max()
        assert torch.allclose(val["lse"], torch.logsumexp(val["S"], -1))


def test_the_layout_helpers_are_the_parity_tests_layout():
    """to_units / from_units against _attn_ref of test_gpu_parity.py; the split-precision scale against _attn_scales of the f16f8 module"""
    from test_gpu_f16f8_kernels import _attn_scales
    from test_gpu_parity import _attn_ref
    for temporal in (0, 1):
        Bn, T, Jn, C, Hn = 2, 5, 3, 32, 2
        (qv, _), (dv, _) = ar.make_inputs("randn", Bn, T, Jn, C, Hn, temporal, "planar", 3)
        q, k, v = ar.split_qkv(qv, Bn, T, Jn, Hn, temporal)
        ref = ar.reference(q, k, v, ar.to_units(dv, Bn, T, Jn, Hn, temporal), (C // Hn) ** -0.5)
        want = _attn_ref(qv, Bn, T, Jn, C, Hn, temporal)
        assert (ar.from_units(ref[0]["O"], Bn, T, Jn, Hn, temporal) - want).abs().max() <= 1e-14
        pv, lmax = _attn_scales(qv, Bn, T, Jn, C, Hn, temporal)
        theirs = 2.0 ** -16 * (pv + want.abs()) * (1.0 + lmax)
        assert torch.allclose(ar.from_units(ar.x3_scale(ref), Bn, T, Jn, Hn, temporal), theirs, rtol=1e-12, atol=0)

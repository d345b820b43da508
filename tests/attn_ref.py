"""fp64 reference of the attention core, per-element forward-error scales, input families and a CPU model of a bf16 kernel (no GPU).

Everything works on "units": a (U, N, d) tensor per operand, U = the independent attention problems of a launch - (b, j, h) with N = T
tokens for the temporal layout, (b, t, h) with N = J tokens for the spatial one - cut out of the fused (M, 3C) qkv buffer of the token
layout m = (b T + t) J + j by to_units / from_units.  The temporal log-sum-exp of the kernels is lse[unit * T + t]: lse_flat().

Explicit formulas (reference()), on the values the kernel receives:
    S = scale Q K^T   lse = logsumexp(S)   P = exp(S - lse)   O = P V
    dP = dO V^T   delta = sum_d dO O   dS = P (dP - delta)   dQ = scale dS K   dK = scale dS^T Q   dV = P^T dO
Forward-error scales (same formulas on absolute values; `m`), and the share of each that the logits' own rounding moves (`ml`): a logit is
an fp32-accumulated sum of exactly represented products, so it carries 2^-24 lmax of absolute error, lmax = max_j scale |q| . |k_j|, whatever
the storage type, and P - with everything computed from it - moves by that RELATIVE amount.  An error is asserted per element as
    |got - want| <= C (unit m + 2^-24 ml),        unit = 2^-8 (bf16 operands / outputs) or 2^-24 (fp32),
so for the bf16 forms the second term is noise (2^-16 lmax) and for the fp32 row kernels it is what keeps `large` logits in the same bound.
"""
import math

import torch

U8, U24 = 2.0 ** -8, 2.0 ** -24
FAMILIES = ("randn", "peaked", "negative", "large")
FAULTS = ("pad_key", "dq_x1.03", "last_query", "dq_row_zero", "dk_no_scale")


# ------------------------------------------------------------------------------------------------ layout
def to_units(x, B, T, J, H, temporal):
    """(M, H d) -> (U, N, d)"""
    d = x.shape[1] // H
    x = x.reshape(B, T, J, H, d)
    x = x.permute(0, 2, 3, 1, 4) if temporal else x.permute(0, 1, 3, 2, 4)
    return x.reshape(-1, T if temporal else J, d)


def from_units(y, B, T, J, H, temporal):
    """(U, N, d) -> (M, H d)"""
    d = y.shape[-1]
    y = y.reshape(B, J, H, T, d).permute(0, 3, 1, 2, 4) if temporal else y.reshape(B, T, H, J, d).permute(0, 1, 3, 2, 4)
    return y.reshape(B * T * J, H * d)


def split_qkv(qkv, B, T, J, H, temporal):
    C = qkv.shape[1] // 3
    return tuple(to_units(qkv[:, i * C:(i + 1) * C], B, T, J, H, temporal) for i in range(3))


def join_qkv(dq, dk, dv, B, T, J, H, temporal):
    return torch.cat([from_units(t, B, T, J, H, temporal) for t in (dq, dk, dv)], 1)


def lse_flat(lse_units):
    """(U, N) -> the kernels' lse[unit * T + t] (temporal)"""
    return lse_units.reshape(-1)


# ------------------------------------------------------------------------------------------------ reference and scales
def reference(q, k, v, do, scale):
    """fp64 attention forward + backward on (U, N, d) operands; returns the values, the scales `m` and their logit shares `ml`."""
    q, k, v, do = (t.double() for t in (q, k, v, do))
    S = scale * q @ k.transpose(-2, -1)
    lse = torch.logsumexp(S, -1)
    P = torch.exp(S - lse[..., None])
    O = P @ v
    dP = do @ v.transpose(-2, -1)
    delta = (do * O).sum(-1)
    dS = P * (dP - delta[..., None])
    val = dict(S=S, lse=lse, P=P, O=O, delta=delta, dq=scale * dS @ k, dk=scale * dS.transpose(-2, -1) @ q, dv=P.transpose(-2, -1) @ do)
    lmax = (scale * q.abs() @ k.abs().transpose(-2, -1)).amax(-1)                       # (U, N): per query
    mO = P @ v.abs()
    # dS: the products of dP, and delta's - the cancellation in dP - delta, delta being formed from the stored (rounded) O
    mdS = P * (do.abs() @ v.abs().transpose(-2, -1) + (do.abs() * mO).sum(-1, keepdim=True))
    m = dict(lse=lmax + lse.abs(), O=mO, delta=(do.abs() * mO).sum(-1), dq=scale * mdS @ k.abs(), dk=scale * mdS.transpose(-2, -1) @ q.abs(),
             dv=P.transpose(-2, -1) @ do.abs())
    w = lmax[..., None]                                                                  # a query's logit error moves its row of P
    ml = dict(lse=torch.zeros_like(lse), O=w * mO, delta=lmax * m["delta"], dq=scale * (w * mdS) @ k.abs(),
              dk=scale * (w * mdS).transpose(-2, -1) @ q.abs(), dv=(w * P).transpose(-2, -1) @ do.abs())
    return val, m, ml


def ratios(got, ref, unit, keys=("lse", "O", "dq", "dk", "dv")):
    """worst |got - want| / (unit m + 2^-24 ml) per quantity over ALL elements (inf for a non-finite or missing element); lse always in 2^-24"""
    val, m, ml = ref
    out = {}
    for key in keys:
        if key not in got:
            continue
        g = got[key].double().reshape(val[key].shape)
        u = U24 if key == "lse" else unit
        r = (g - val[key]).abs() / (u * m[key] + U24 * ml[key])
        r = torch.where(torch.isfinite(g), r, torch.full_like(r, float("inf")))
        out[key] = r.max().item()
    return out


def x3_scale(ref):
    """the split-precision forward's error scale per output element (test_gpu_f16f8_kernels: 2^-16 (softmax-weighted |v| + |O|) (1 + lmax))"""
    val, m, _ = ref
    lmax = m["lse"] - val["lse"].abs()
    return 2.0 ** -16 * (m["O"] + val["O"].abs()) * (1.0 + lmax[..., None])


# ------------------------------------------------------------------------------------------------ inputs
def _storage(x, storage):
    """round to what the kernel receives; returns (fp64 value, tensors to upload)"""
    if storage == "f32":
        x = x.float()
        return x.double(), (x,)
    hi = x.float().bfloat16()
    if storage == "bf16":
        return hi.double(), (hi,)
    assert storage == "planar"
    lo = (x.float() - hi.float()).bfloat16()
    return hi.double() + lo.double(), (hi, lo)


def make_inputs(family, B, T, J, C, H, temporal, storage, seed, scale=None):
    """(qkv, dout) of one input family, rounded to the storage type BEFORE anything is computed from them:
    (qkv fp64 (M, 3C), upload tensors), (dout fp64 (M, C), upload tensors); storage "f32", "bf16" or "planar" (bf16 hi + lo; dout bf16)."""
    assert family in FAMILIES, family
    d = C // H
    scale = d ** -0.5 if scale is None else scale
    g = torch.Generator().manual_seed(seed)
    M = B * T * J
    qkv = torch.randn(M, 3 * C, generator=g)
    dout = torch.randn(M, C, generator=g)
    small = torch.arange(M) % 7 == 3                      # small-magnitude token rows: a per-element bound must still see their errors
    dout[small] *= 2.0 ** -4
    if family == "negative":
        # q = a s + noise, k = -b s + noise with a common sign vector s per head: every logit is -(scale d) a b + noise, a b in [1, 1.69] x 12 /
        # (scale d): all real logits in about [-21, -11], so a key that leaks in at score 0 carries e^11 times the mass of the row
        s = (torch.randint(2, (H, d), generator=g) * 2 - 1).float().reshape(1, C)
        base = math.sqrt(12.0 / (scale * d))
        a = base * (1.0 + 0.3 * torch.rand(M, 1, generator=g))
        b = base * (1.0 + 0.3 * torch.rand(M, 1, generator=g))
        noise = 0.05 * base
        qkv[:, :C] = a * s + noise * qkv[:, :C]
        qkv[:, C:2 * C] = -b * s + noise * qkv[:, C:2 * C]
        qkv[small, 2 * C:] *= 2.0 ** -4
    else:
        qkv[small] *= 2.0 ** -4
        if family == "peaked":
            qkv[:, :C] *= 4.0                             # logits of std ~4: a few keys carry the mass, dP - delta cancels
        elif family == "large":
            qkv[:, :C] *= 13.0                            # |logit| up to ~60: exp overflows without the max, underflows for most keys with it
        if scale != d ** -0.5:
            qkv[:, :C] *= d ** -0.5 / scale               # the same logits under another softmax scale
    qv, qt = _storage(qkv, storage)
    dv, dt = _storage(dout, "f32" if storage == "f32" else "bf16")
    return (qv, qt), (dv, dt)


# ------------------------------------------------------------------------------------------------ CPU model of a bf16 MFMA kernel
def _rb(x):
    return x.float().bfloat16().double()


def model_bf16(q, k, v, do, scale, fault=None, rounding=True):
    """fp64 with bf16 rounding at the rounding points of attn_tmfma_fwd / attn_tmfma_bwd (attention_mfma.hip):
      forward : e = exp(S - max) rounded to bf16 as the MFMA operand of e V (pack_acc), the row sum taken from the unrounded e, O stored as
                bf16((e V) / sum); lse from the unrounded sum;
      backward: P = exp(S - lse) and dS = P (dP - delta) rounded to bf16 as MFMA operands (pack_acc), delta from the STORED O, dQ / dK / dV
                stored as bf16.
    rounding = False: plain fp64 (an exact kernel).  fault: one of FAULTS - a subtly wrong kernel."""
    assert fault is None or fault in FAULTS, fault
    rb = _rb if rounding else (lambda x: x)
    q, k, v, do = (t.double() for t in (q, k, v, do))
    U, N, d = q.shape
    kk, vv = k, v
    if fault == "pad_key":                                # one zero-padded key (score 0, v = 0) takes part in the softmax
        kk = torch.cat([k, torch.zeros(U, 1, d, dtype=k.dtype)], 1)
        vv = torch.cat([v, torch.zeros(U, 1, d, dtype=v.dtype)], 1)
    S = scale * q @ kk.transpose(-2, -1)
    mx = S.amax(-1, keepdim=True)
    e = torch.exp(S - mx)
    den = e.sum(-1, keepdim=True)
    O = rb((rb(e) @ vv) / den)
    lse = (mx + torch.log(den))[..., 0]
    P = torch.exp(S - lse[..., None])
    dP = do @ vv.transpose(-2, -1)
    delta = (do * O).sum(-1)
    dS = P * (dP - delta[..., None])
    Pb, dSb = rb(P), rb(dS)
    dq = scale * dSb @ kk
    if fault == "dq_x1.03":
        dq = dq * 1.03
    if fault == "last_query":                             # the last query missing from dK / dV
        Pb, dSb = Pb[:, :-1], dSb[:, :-1]
        qq, dd = q[:, :-1], do[:, :-1]
    else:
        qq, dd = q, do
    dk = (1.0 if fault == "dk_no_scale" else scale) * dSb.transpose(-2, -1) @ qq
    dv = Pb.transpose(-2, -1) @ dd
    dq, dk, dv = rb(dq), rb(dk[:, :N]), rb(dv[:, :N])
    if fault == "dq_row_zero":                            # one token's dQ row never written
        dq = dq.clone()
        dq[:, N // 2] = 0.0
    return dict(lse=lse, O=O, dq=dq, dk=dk, dv=dv)

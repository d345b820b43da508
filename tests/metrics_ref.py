"""fp64 references of the evaluation-metric kernels - mp_pose_metrics (pose_metrics_kernel in its LDS-staged and its strided form,
pose_metrics_finalize_kernel), mp_bone_length_table and mp_procrustes_errors (procrustes_kernel, procrustes_finalize_kernel) - and of
the host arithmetic of manipose_amd/metrics/analytics.py, with per-entry forward-error scales, and the seeded inputs the host and the GPU
tests share (numpy only, no GPU).

Every function takes the fp32 arrays exactly as the kernel receives them and a `dtype`: numpy.float64 gives the reference, numpy.float32 the
same formula in plain fp32 numpy (test_metrics_ref_host.py measures its error to derive BOUNDS).  The two scales are applied in fp32
first, as the kernels do (x = fl(sc * raw)): those fp32 products are the exact inputs of everything below.  A result is a pair
(value, scale): an error is asserted per entry as |got - value| <= C u scale, u = 2^-24, C = BOUNDS[key].

Scales (absolute values of the pieces a result is formed from, plus the result; a quantity that is itself computed carries its scale on)
  difference    d = a - b of two inputs: |d| (one rounding); of two computed values: their scales + |d|
  norm          n = |c| of a vector c whose components carry e_c:  N = sum_c |c_c| e_c / n + n (sum_c e_c where n == 0);  n^2: 2 sum_c |c_c| e_c + n^2
  square        q^2 of a computed q with scale Q:  2 |q| Q + q^2 + u Q^2 (the second-order term is all there is where q == 0: frame 0's
                len - len0 is exactly 0 in the reference and a rounding of the coordinates in a kernel that scales by sc != 1)
  scale_align   f = <x, y> / <x, x> per frame:  F = |f| (sum |x y| / |<x, y>| + 2);  aligned coordinate f x:  |x| F + |f x|
  bone length   norm of x_j - x_parent;  joint error: norm of x_j - y_j;  velocity: norm of (x_t - x_t-1) - (y_t - y_t-1), components
                carrying |x_t - x_t-1| + |y_t - y_t-1| + |v| (+ the aligned coordinates' own scales)
  len0          the bone lengths of frame 0 of the UNALIGNED prediction.  The kernel forms them as sc (a - b), the frames' lengths from
                sc a - sc b: equal in exact arithmetic, a rounding of the coordinates apart in fp32.  The reference is |x_j - x_p| of
                x = fl(sc raw); with sc != 1 its components carry |x_j| + |x_p| (the cancellation), with sc == 1 only |d|
  shifted sums  d = len - len0:  D = N(len) + N(len0) + |d| - the cancellation in len - len0 is the lengths' own roundings;  d^2 by the square rule
  sums          over frames (and joints, bones, pairs):  sum of the addends' scales + sum of |addend| (the fp32 partial sums).  The signed
                bone sum therefore carries the unsigned sum
  counts        PCK: visible joints with e < threshold (strict: a tie is not counted);  AUC: per visible joint the number of grid values
                i auc_max / (auc_steps - 1), i = 0 .. auc_steps - 1, strictly above e (the grid in fp64 from the fp32 auc_max the ABI
                receives);  compared for equality - test_metrics_ref_host.py shows every error of every case is at least 64 u of its
                scale away from every threshold, except the planted ties, which are exact in fp32.  The grid value 0 is above no error in
                any arithmetic (no norm is negative), so it needs no margin
  variance      of a bone length over n frames from s1 = sum d, s2 = sum d^2:  (s2 - s1^2 / n) / (n - 1) carries
                (S2 + 2 |s1| S1 / n) / (n - 1) + var;  its root: that / (2 std) + std.  A rigid sequence has d of the size of the lengths'
                roundings: its sums are all rounding, the plain fp32 evaluation may be any multiple of that scale off, and such cases
                have bound keys of their own (`*_rigid`), derived by the same rule from their own cases

Procrustes (mp_procrustes_errors), per frame, x = target, y = prediction (17 x 3):  the reference's procedure (mean_joint_errors.py p_mpjpe)
in fp64: centre both, normalise both to Frobenius norm 1, H = X0^T Y0 = U S V^T (numpy.linalg.svd), R = V U^T, where det R < 0 flip the
sign of the last column of V and of the last singular value, a = trace(S) normX / normY, t = mx - a my R, aligned y' = a y R + t,
e_j = |y'_j - x_j|.  Scale of e_j:  the kernel centres in fp32 (an error of u (|x_j| + mean|x|) in x0_j, likewise y0_j), forms Horn's N
from H (entries known to u sum_j |y0_j||x0_j|, which the centring error raises to u (|x| / |x0|) lambda_1), takes N's dominant
eigenvector (perturbation theory: an error dN turns it by |dN| / (lambda_1 - lambda_2)) and lambda_1 itself (the scale a = lambda_1 /
|y0|^2).  The rotation error moves the aligned joint by a |y0_j| |dN| / (lambda_1 - lambda_2), the other errors by their own size, so
    S_j = (sum_c |x_jc| + mean_j |x_jc| + a (|y_jc| + mean_j |y_jc|)) (1 + lambda_1 / (lambda_1 - lambda_2)) + e_j,
the last factor being the conditioning of the rotation.  Non-special frames keep that factor below GAP_CAP (asserted on the CPU).
Where lambda_1 = lambda_2 the rotation is undetermined and the factor is infinite - but for these inputs the aligned errors do not depend
on the undetermined part, and the gap to the next DISTINCT eigenvalue (lambda_1 - lambda_3) takes its place (frames marked `axis_free`):
  * a collinear target: the optimum is free up to a rotation about the target's axis, which moves the aligned prediction on circles
    around that axis and leaves every joint's distance to its (on-axis) target unchanged;
  * a collinear prediction: a rotation about the prediction's own axis does not move the prediction at all.
A planar prediction makes the reflection fix immaterial (flipping V's last column acts along the prediction's normal, where it has no
extent); a planar target with a non-planar prediction maps the prediction's third direction to +/- the target's normal: every distance
is the same for both signs.  A prediction that is an exactly similar copy of the target has e = 0: its bound is the absolute floor u S_j.
"""
import functools
import os

import numpy as np

from ends_ref import PARENTS, U24, bound_from  # noqa: F401  (re-exported)

NJ, NB, NP, NS = 17, 16, 6, 12
OB, OP, OJ = NS, NS + 4 * NB, NS + 4 * NB + 2 * NP
NV = OJ + 2 * NJ
BJ, BP = np.arange(1, NJ), np.array(PARENTS[1:])
PAIR_L, PAIR_R = np.array([3, 4, 5, 10, 11, 12]), np.array([0, 1, 2, 13, 14, 15])        # bones of joints_left (4,5,6,11,12,13) / joints_right
F32, F64 = np.float32, np.float64
MARGIN = 64 * U24          # asserted distance of every error from every threshold, in units of its scale
SETTLE = 128 * U24         # the distance the generators establish
GAP_CAP = 8.0              # 1 + lambda_1 / (lambda_1 - lambda_2) of every non-special Procrustes frame stays below it
COUNT_SLOTS = (6, 7, 8, 11)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# bound key of every slot of a row
SLOT_KEYS = ["err", "err2", "sym", "sym2", "len_abs", "len_signed", "count", "count", "count", "vel", "vel2", "count"] + \
    ["bone_d", "bone_d2", "len_abs", "len_signed"] * NB + ["sym", "sym2"] * NP + ["err", "err2"] * NJ
GT_SLOTS = [0, 1, 4, 5, 6, 7, 8, 9, 10] + [OB + 4 * k + i for k in range(NB) for i in (2, 3)] + list(range(OJ, NV))   # 0 without a target

# asserted bound constants, in units of u x the entry's scale: bound_from() of the worst error / scale of the plain fp32 CPU evaluation over
# this module's cases (the ratio in the comment; test_metrics_ref_host.py measures it and checks the constant against it)
BOUNDS = {
    # rows of one or two frames (FRAME_CASES)
    "err": 5.0,             # 1.09
    "err2": 5.0,            # 1.13
    "sym": 3.0,             # 0.592
    "sym2": 3.0,            # 0.596
    "len_abs": 4.0,         # 0.759
    "len_signed": 4.0,      # 0.759
    "vel": 2.0,             # 0.28
    "vel2": 1.0,            # 0.211
    "bone_d": 3.0,          # 0.68
    "bone_d2": 3.0,         # 0.711
    "len0": 5.0,            # 1.1
    # rows of hundreds of frames (EDGE_CASES); numpy adds the frames of a per-joint column one after the other
    "err_sum": 20.0,        # 4.69
    "err2_sum": 20.0,       # 3.2
    "sym_sum": 2.0,         # 0.316
    "sym2_sum": 2.0,        # 0.32
    "len_abs_sum": 1.0,     # 0.226
    "len_signed_sum": 1.0,  # 0.22
    "vel_sum": 1.0,         # 0.187
    "vel2_sum": 1.0,        # 0.085
    "bone_d_sum": 3.0,      # 0.517
    "bone_d2_sum": 2.0,     # 0.378
    "len0_sum": 5.0,        # 1.05
    "bone_d_rigid": 2.0,    # 0.274   (the rigid sequence at a root offset of 5 m, T = 257)
    "bone_d2_rigid": 1.0,   # 0.208
    "blt": 4.0,             # 0.901
    "pr_frame": 2.0,        # 0.474   (the larger of the Jacobi and the SVD evaluation)
    "pr_sum": 1.0,          # 0.0128
    "bone_var": 1.0,        # 0.199   (PoseAnalytics.bone_variance from the fp32 sums)
    "bone_var_rigid": 1.0,  # 0.184
}


def row_key(key, case, rigid=False):
    """the bound key of a row entry of kind `key` in the pose case `case`: the per-frame cases (one or two frames per row), the chunk-edge cases
    (`_sum`: hundreds of frames per row) and the shifted sums of the rigid case (`_rigid`) each have constants derived from their own cases"""
    if rigid and key.startswith("bone_d"):
        return key + "_rigid"
    return key + "_sum" if case in EDGE_CASES else key


def f32(x):
    """the fp32 value of a Python float (what the C ABI receives), as a Python float"""
    return float(np.float32(x))


def worst(got, want, scale):
    """largest |got - want| / (u scale) over the entries; NaN / inf anywhere in got gives inf, and so does any error where the scale is 0"""
    got = np.asarray(got, dtype=F64)
    if got.size == 0:
        return 0.0
    if not np.isfinite(got).all():
        return float("inf")
    err, den = np.abs(got - want), U24 * np.asarray(scale, dtype=F64) * np.ones_like(got)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(den > 0, err / np.maximum(den, 1e-300), np.where(err > 0, np.inf, 0.0))
    return float(ratio.max())


# ------------------------------------------------------------------------------------------------ storage layouts
def layout(a, form):
    """(storage (1-D fp32, NaN wherever no element lives), offset, element strides of (b, t, j, c)) holding a (B, L, 17, 3) in one of the
    forms the entry points are called with: 'contig' (B,L,J,3); 'perm' the reference's (B,3,J,L) permutation; 'pad' a storage offset of 7
    floats, 5 floats per joint, one spare frame and 3 spare floats per batch item"""
    B, L = a.shape[:2]
    if form == "contig":
        off, st = 0, (L * NJ * 3, NJ * 3, 3, 1)
    elif form == "perm":
        off, st = 0, (3 * NJ * L, 1, L, NJ * L)
    else:
        off, st = 7, ((L + 1) * NJ * 5 + 3, NJ * 5, 5, 1)
    size = off + (B - 1) * st[0] + (L - 1) * st[1] + (NJ - 1) * st[2] + 2 * st[3] + 1
    s = np.full(size, np.nan, dtype=F32)
    gather(s, off, st, B, L, writable=True)[...] = a
    return s, off, st


def gather(storage, offset, strides, B, L, writable=False):
    """the (B, L, 17, 3) array the kernel addresses in `storage` through the element strides of (b, t, j, c) from `offset`"""
    v = np.lib.stride_tricks.as_strided(storage[offset:], shape=(B, L, NJ, 3), strides=tuple(4 * s for s in strides), writeable=writable)
    return v if writable else np.array(v)


def scaled(raw, sc):
    """fl(sc * raw): the kernel's first operation, in fp32"""
    return (np.float32(sc) * np.asarray(raw, dtype=F32)).astype(F32)


# ------------------------------------------------------------------------------------------------ mp_pose_metrics
def _norm(d, ed):
    n2 = (d * d).sum(-1)
    n = np.sqrt(n2)
    lin = (np.abs(d) * ed).sum(-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        N = np.where(n > 0, lin / np.where(n > 0, n, 1) + n, ed.sum(-1))
    return n, N, n2, 2 * lin + n2


def _sq_scale(q, Q):
    return 2 * np.abs(q) * Q + q * q + U24 * Q * Q


def _bones(z, ez):
    d = z[..., BJ, :] - z[..., BP, :]
    return _norm(d, ez[..., BJ, :] + ez[..., BP, :] + np.abs(d))[:2]


def auc_grid(auc_max, auc_steps):
    return np.arange(auc_steps, dtype=F64) * (F64(f32(auc_max)) / (auc_steps - 1))


def _tot(v, s, axes):
    return v.sum(axes), s.sum(axes) + np.abs(v).sum(axes)


def pose_terms(x32, y32, scale_align, D=F64):
    """per-frame quantities of the scaled fp32 frames x32 (prediction), y32 (target or None), each (B, L, 17, 3):
    dict name -> (value, scale); plen (B,L,16), e (B,L,17), vel (B,L) (0 at t = 0) ..."""
    x = x32.astype(D)
    ex = np.zeros_like(x)
    y = None if y32 is None else y32.astype(D)
    if y is not None and scale_align:
        pp, pg, apg = (x * x).sum((-1, -2)), (x * y).sum((-1, -2)), np.abs(x * y).sum((-1, -2))
        f = pg / pp
        F = np.abs(f) * (apg / np.abs(pg) + 2)
        xa = x * f[..., None, None]
        ex, x = np.abs(x) * F[..., None, None] + np.abs(xa), xa
    out = {}
    plen, Np = _bones(x, ex)
    out["plen"] = (plen, Np)
    dp = np.abs(plen[..., PAIR_L] - plen[..., PAIR_R])
    Sp = Np[..., PAIR_L] + Np[..., PAIR_R] + dp
    out["sym"], out["sym2"] = (dp, Sp), (dp * dp, _sq_scale(dp, Sp))
    if y is not None:
        glen, Ng = _bones(y, np.zeros_like(y))
        dl = glen - plen
        out["dl"] = (dl, Ng + Np + np.abs(dl))
        d = x - y
        e, Ne, e2, Ne2 = _norm(d, ex + np.abs(d))
        out["e"], out["e2"] = (e, Ne), (e2, Ne2)
        dx, dy = x[:, 1:] - x[:, :-1], y[:, 1:] - y[:, :-1]
        v = dx - dy
        n, N, n2, N2 = _norm(v, ex[:, 1:] + ex[:, :-1] + np.abs(dx) + np.abs(dy) + np.abs(v))
        z = np.zeros(x.shape[:1] + (1,), dtype=D)
        out["vel"] = tuple(np.concatenate([z, q.sum(-1)], 1) for q in (n, N + n))
        out["vel2"] = tuple(np.concatenate([z, q.sum(-1)], 1) for q in (n2, N2 + n2))
    return out


def len0_ref(x32, pred_scale, D=F64):
    """(B, 16) bone lengths of frame 0 of the unaligned scaled prediction and their scale (module docstring, len0)"""
    x = x32[:, 0].astype(D)
    d = x[..., BJ, :] - x[..., BP, :]
    ed = np.abs(d) + (0.0 if f32(pred_scale) == 1.0 else np.abs(x[..., BJ, :]) + np.abs(x[..., BP, :]))
    return _norm(d, ed)[:2]


def pose_metrics_ref(pred, gt, mask, pred_scale=1.0, gt_scale=1.0, pck_thr=150.0, auc_max=150.0, auc_steps=31, scale_align=False, dtype=F64):
    """pred, gt (or None): (B, L, 17, 3) fp32 as addressed by the kernel; mask (B, L, 17) or None ->
    dict(row (B, NV), row_scale, len0 (B, 16), len0_scale, e / e_scale (B, L, 17) or None, vis (B, L, 17) bool)"""
    D = dtype
    B, L = pred.shape[:2]
    x32 = scaled(pred, pred_scale)
    y32 = None if gt is None else scaled(gt, gt_scale)
    T = pose_terms(x32, y32, scale_align, D)
    l0, N0 = len0_ref(x32, pred_scale, D)
    row, sc = np.zeros((B, NV), dtype=D), np.zeros((B, NV), dtype=F64)

    def put(slot, vs, axes):
        row[:, slot], sc[:, slot] = _tot(vs[0], vs[1], axes)

    plen, Np = T["plen"]
    d0 = plen - l0[:, None]
    D0 = Np + N0[:, None] + np.abs(d0)
    put(slice(OB, OP, 4), (d0, D0), 1)
    put(slice(OB + 1, OP, 4), (d0 * d0, _sq_scale(d0, D0)), 1)
    put(2, T["sym"], (1, 2)); put(3, T["sym2"], (1, 2))
    put(slice(OP, OJ, 2), T["sym"], 1); put(slice(OP + 1, OJ, 2), T["sym2"], 1)
    row[:, 11] = L
    vis = np.ones((B, L, NJ), dtype=bool) if mask is None else np.asarray(mask).reshape(B, L, NJ) != 0
    res = dict(row=row, row_scale=sc, len0=l0, len0_scale=N0, e=None, e_scale=None, vis=vis)
    if gt is not None:
        dl, Sl = T["dl"]
        put(4, (np.abs(dl), Sl), (1, 2)); put(5, (dl, Sl), (1, 2))
        put(slice(OB + 2, OP, 4), (np.abs(dl), Sl), 1); put(slice(OB + 3, OP, 4), (dl, Sl), 1)
        put(0, T["e"], (1, 2)); put(1, T["e2"], (1, 2))
        put(slice(OJ, NV, 2), T["e"], 1); put(slice(OJ + 1, NV, 2), T["e2"], 1)
        put(9, T["vel"], 1); put(10, T["vel2"], 1)
        e = T["e"][0]
        row[:, 6] = ((e < F64(f32(pck_thr))) & vis).sum((1, 2))
        row[:, 7] = ((auc_grid(auc_max, auc_steps) > e[..., None]).sum(-1) * vis).sum((1, 2))
        row[:, 8] = vis.sum((1, 2))
        res["e"], res["e_scale"] = e, T["e"][1] + e
    return res


def bone_table_ref(pred, gt, signed, dtype=F64):
    """mp_bone_length_table: (B L, 16) target minus predicted bone length of the raw inputs (no scales), and its scale"""
    p, g = pred.astype(dtype), gt.astype(dtype)
    lp, Npp = _bones(p, np.zeros_like(p))
    lg, Ng = _bones(g, np.zeros_like(g))
    d = lg - lp
    return (d if signed else np.abs(d)).reshape(-1, NB), (Ng + Npp + np.abs(d)).reshape(-1, NB)


# ------------------------------------------------------------------------------------------------ mp_procrustes_errors
def horn_matrix(x0, y0):
    """Horn's N (.., 4, 4) for the rotation taking the centred prediction y0 onto the centred target x0 (quaternion w, x, y, z)"""
    h = np.einsum("...jr,...jc->...rc", y0, x0)
    n = np.zeros(h.shape[:-2] + (4, 4), dtype=h.dtype)
    n[..., 0, 0] = h[..., 0, 0] + h[..., 1, 1] + h[..., 2, 2]
    n[..., 1, 1] = h[..., 0, 0] - h[..., 1, 1] - h[..., 2, 2]
    n[..., 2, 2] = -h[..., 0, 0] + h[..., 1, 1] - h[..., 2, 2]
    n[..., 3, 3] = -h[..., 0, 0] - h[..., 1, 1] + h[..., 2, 2]
    for (a, b), v in (((0, 1), h[..., 1, 2] - h[..., 2, 1]), ((0, 2), h[..., 2, 0] - h[..., 0, 2]), ((0, 3), h[..., 0, 1] - h[..., 1, 0]),
                      ((1, 2), h[..., 0, 1] + h[..., 1, 0]), ((1, 3), h[..., 2, 0] + h[..., 0, 2]), ((2, 3), h[..., 1, 2] + h[..., 2, 1])):
        n[..., a, b] = n[..., b, a] = v
    return n


def _svd_align(x, y):
    """the reference's procedure on (N, 17, 3) arrays of any float type: aligned prediction, scale a"""
    mx, my = x.mean(1, keepdims=True), y.mean(1, keepdims=True)
    X0, Y0 = x - mx, y - my
    nX, nY = np.sqrt((X0 ** 2).sum((1, 2), keepdims=True)), np.sqrt((Y0 ** 2).sum((1, 2), keepdims=True))
    X0, Y0 = X0 / nX, Y0 / nY
    U, s, Vt = np.linalg.svd(np.matmul(X0.transpose(0, 2, 1), Y0))
    V = Vt.transpose(0, 2, 1).copy()
    sign = np.sign(np.linalg.det(np.matmul(V, U.transpose(0, 2, 1))))[:, None].astype(x.dtype)
    V[:, :, -1] *= sign
    s[:, -1] *= sign[:, 0]
    R = np.matmul(V, U.transpose(0, 2, 1))
    a = s.sum(1)[:, None, None] * nX / nY
    t = mx - a * np.matmul(my, R)
    return a * np.matmul(y, R) + t, a[:, 0, 0]


def thresholds_of(pck_thr, auc_max, auc_steps):
    """every threshold an error is compared with (the grid value 0 left out: module docstring, counts)"""
    return np.concatenate([[F64(f32(pck_thr))], auc_grid(auc_max, auc_steps)[1:]])


def procrustes_ref(pred, gt, mask, pred_scale=1.0, gt_scale=1.0, pck_thr=150.0, auc_max=150.0, auc_steps=31, axis_free=False):
    """pred, gt (N, 17, 3) fp32, mask (N, 17) or None -> dict(out (5,), out_scale (only [0] is not a count), e / e_scale (N, 17),
    gap (N,) = lambda_1 - lambda_2 of Horn's N (lambda_1 - lambda_3 with axis_free), kappa (N,) = 1 + lambda_1 / gap, lam1 (N,), a (N,))"""
    x, y = scaled(gt, gt_scale).astype(F64), scaled(pred, pred_scale).astype(F64)
    ya, a = _svd_align(x, y)
    e = np.sqrt(((ya - x) ** 2).sum(-1))
    w = np.linalg.eigvalsh(horn_matrix(x - x.mean(1, keepdims=True), y - y.mean(1, keepdims=True)))
    lam1 = w[:, -1]
    gap = lam1 - (w[:, -3] if axis_free else w[:, -2])
    with np.errstate(divide="ignore"):
        kappa = 1.0 + lam1 / gap
    mag = (np.abs(x) + np.abs(x).mean(1, keepdims=True)).sum(-1) + a[:, None] * (np.abs(y) + np.abs(y).mean(1, keepdims=True)).sum(-1)
    S = mag * kappa[:, None] + e
    vis = np.ones(e.shape, dtype=bool) if mask is None else np.asarray(mask).reshape(e.shape) != 0
    out = np.array([e.sum(), ((e < F64(f32(pck_thr))) & vis).sum(), ((auc_grid(auc_max, auc_steps) > e[..., None]).sum(-1) * vis).sum(), vis.sum(),
                    float(e.shape[0])])
    return dict(out=out, out_scale=S.sum() + e.sum(), e=e, e_scale=S, gap=gap, kappa=kappa, lam1=lam1, a=a, vis=vis)


def _jacobi_f32(n):
    """dominant eigenpair of (N, 4, 4) fp32 matrices: cyclic Jacobi sweeps in fp32 until no rotation is left to do (at most 30 sweeps)"""
    a = n.astype(F32).copy()
    v = np.broadcast_to(np.eye(4, dtype=F32), a.shape).copy()
    one = np.float32(1.0)
    with np.errstate(all="ignore"):
        for _ in range(30):
            off = np.sqrt(sum(a[:, p, r] ** 2 for p in range(3) for r in range(p + 1, 4)))
            if (off <= np.float32(2.0 ** -26) * np.abs(a[:, [0, 1, 2, 3], [0, 1, 2, 3]]).max(1)).all():
                break
            for p in range(3):
                for r in range(p + 1, 4):
                    apq = a[:, p, r]
                    nz = np.abs(apq) > 0
                    theta = (a[:, r, r] - a[:, p, p]) / (np.float32(2.0) * np.where(nz, apq, one))
                    t = np.copysign(one, theta) / (np.abs(theta) + np.sqrt(theta * theta + one))
                    c = np.where(nz, one / np.sqrt(t * t + one), one).astype(F32)
                    s = np.where(nz, t * c, np.float32(0.0)).astype(F32)
                    c1, s1 = c[:, None], s[:, None]
                    ap, ar = a[:, :, p].copy(), a[:, :, r].copy()
                    a[:, :, p], a[:, :, r] = c1 * ap - s1 * ar, s1 * ap + c1 * ar
                    ap, ar = a[:, p, :].copy(), a[:, r, :].copy()
                    a[:, p, :], a[:, r, :] = c1 * ap - s1 * ar, s1 * ap + c1 * ar
                    vp, vr = v[:, :, p].copy(), v[:, :, r].copy()
                    v[:, :, p], v[:, :, r] = c1 * vp - s1 * vr, s1 * vp + c1 * vr
    diag = a[:, [0, 1, 2, 3], [0, 1, 2, 3]]
    best = diag.argmax(1)
    idx = np.arange(a.shape[0])
    return v[idx, :, best], diag[idx, best]


def procrustes_f32(pred, gt, pred_scale=1.0, gt_scale=1.0, how="jacobi"):
    """(N, 17) aligned errors in plain fp32 on the CPU: 'jacobi' = Horn's N with cyclic Jacobi sweeps run to convergence and the
    kernel's assembly of the transform; 'svd' = the reference's procedure with an fp32 SVD"""
    x, y = scaled(gt, gt_scale), scaled(pred, pred_scale)
    if how == "svd":
        ya, _ = _svd_align(x, y)
        return np.sqrt(((ya - x) ** 2).sum(-1, dtype=F32))
    mx, my = x.mean(1, keepdims=True, dtype=F32), y.mean(1, keepdims=True, dtype=F32)
    x0, y0 = x - mx, y - my
    q, lam = _jacobi_f32(horn_matrix(x0, y0))
    q = q / np.sqrt((q * q).sum(1, keepdims=True))
    w, qx, qy, qz = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = np.stack([np.stack([1 - 2 * (qy * qy + qz * qz), 2 * (qx * qy - w * qz), 2 * (qx * qz + w * qy)], -1),
                  np.stack([2 * (qx * qy + w * qz), 1 - 2 * (qx * qx + qz * qz), 2 * (qy * qz - w * qx)], -1),
                  np.stack([2 * (qx * qz - w * qy), 2 * (qy * qz + w * qx), 1 - 2 * (qx * qx + qy * qy)], -1)], 1).astype(F32)
    sc = (lam / (y0 * y0).sum((1, 2), dtype=F32)).astype(F32)
    ya = sc[:, None, None] * np.einsum("nrc,njc->njr", R, y0) + mx
    return np.sqrt(((ya - x) ** 2).sum(-1, dtype=F32))


# ------------------------------------------------------------------------------------------------ AnalyticsAccumulator.report()
def _var_of(plen, Np, ref, Nref):
    """unbiased variance over axis 0 of the bone lengths plen (n, 16) from the sums shifted by ref (16,), its scale, and those of its root"""
    n = plen.shape[0]
    d = plen - ref
    Dd = Np + Nref + np.abs(d)
    s1, S1 = _tot(d, Dd, 0)
    s2, S2 = _tot(d * d, _sq_scale(d, Dd), 0)
    var = plen.var(0, ddof=1)
    Sv = (S2 + 2 * np.abs(s1) * S1 / n) / (n - 1) + var
    std = np.sqrt(var)
    with np.errstate(divide="ignore", invalid="ignore"):
        Ss = np.where(std > 0, Sv / (2 * np.where(std > 0, std, 1)), np.sqrt(U24 * Sv) / U24) + std
    return var, Sv, std, Ss


def item_variance_ref(pred):
    """PoseAnalytics.bone_variance(unbiased=True) of a (B, L, 17, 3) batch with scales 1: (B, 16) value, scale"""
    out = []
    for b in range(pred.shape[0]):
        plen, Np = _bones(pred[b].astype(F64), np.zeros(pred[b].shape))
        out.append(_var_of(plen, Np, plen[0], Np[0])[:2])
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def report_ref(batches, pck_thr=150.0, auc_max=150.0, auc_steps=31):
    """the metrics of AnalyticsAccumulator.report() in fp64 directly from the frames of `batches` = [(pred (B, L, 17, 3), gt)] (scales 1, no
    mask), concatenated into ONE sequence: name -> (value, scale, bound key)"""
    P = np.concatenate([b[0].reshape(-1, NJ, 3) for b in batches]).astype(F64)[None]
    G = np.concatenate([b[1].reshape(-1, NJ, 3) for b in batches]).astype(F64)[None]
    n = P.shape[1]
    T = pose_terms(P.astype(F32), G.astype(F32), False)
    mean = lambda vs, ax: (vs[0].mean(ax), (vs[1] + np.abs(vs[0])).mean(ax))
    out = {}
    e, Ne = T["e"]
    out["mpjpe"] = mean(T["e"], None) + ("err",)
    out["mse"] = mean(T["e2"], None) + ("err2",)
    mp, ms = out["mpjpe"], out["mse"]
    ev = ms[0] - mp[0] ** 2
    out["err_var"] = (ev, ms[1] + 2 * mp[0] * mp[1] + abs(ev), "err2")
    out["mpsse"] = mean(T["sym"], None) + ("sym",)
    out["seg_len_err"] = mean((np.abs(T["dl"][0]), T["dl"][1]), None) + ("len_abs",)
    thr = F64(f32(pck_thr))
    out["pck"] = (100.0 * (e < thr).sum() / e.size, 0.0, "count")
    out["auc"] = (100.0 * (auc_grid(auc_max, auc_steps) > e[..., None]).sum() / (auc_steps * e.size), 0.0, "count")
    jw, jw2 = mean(T["e"], (0, 1)), mean(T["e2"], (0, 1))
    out["jointwise_err"] = jw + ("err",)
    out["jw_err_var"] = (jw2[0] - jw[0] ** 2, jw2[1] + 2 * jw[0] * jw[1] + np.abs(jw2[0] - jw[0] ** 2), "err2")
    out["mpsse_per_pair"] = mean(T["sym"], (0, 1)) + ("sym",)
    plen, Np = T["plen"][0][0], T["plen"][1][0]
    var, Sv, std, Ss = _var_of(plen, Np, plen[0], Np[0])
    out["mpsce_per_bone"] = (std, Ss, "bone_d2")
    out["mpsce"] = (std.mean(), Ss.mean(), "bone_d2")
    vel = nvel = 0.0
    Svel = 0.0
    wstd, Swstd, nwin = np.zeros(NB), np.zeros(NB), 0
    for p, g in batches:
        t = pose_terms(p.astype(F32), g.astype(F32), False)
        vel, Svel, nvel = vel + t["vel"][0].sum(), Svel + t["vel"][1].sum() + t["vel"][0].sum(), nvel + p.shape[0] * (p.shape[1] - 1)
        if p.shape[1] > 1:
            for b in range(p.shape[0]):
                pl, Npl = t["plen"][0][b], t["plen"][1][b]
                _, _, s, Sstd = _var_of(pl, Npl, pl[0], Npl[0])
                wstd, Swstd, nwin = wstd + s, Swstd + Sstd + s, nwin + 1      # (+ s: the fp32 rounding of bone_variance's result)
    out["mvjpe"] = (vel / (nvel * NJ), Svel / (nvel * NJ), "vel")
    out["mpsce_per_bone_windows"] = (wstd / nwin, Swstd / nwin, "bone_d2")
    r = procrustes_ref(P[0].astype(F32), G[0].astype(F32), None, 1.0, 1.0, pck_thr, auc_max, auc_steps)
    out["p_mpjpe"] = (r["out"][0] / (n * NJ), r["out_scale"] / (n * NJ), "pr_sum")
    out["pck_procrustes"] = (100.0 * r["out"][1] / r["out"][3], 0.0, "count")
    out["auc_procrustes"] = (100.0 * r["out"][2] / (auc_steps * r["out"][3]), 0.0, "count")
    return out


# ------------------------------------------------------------------------------------------------ seeded inputs
def skeleton_frames(shape, seed, noise=60.0):
    """gt = 400 randn with the root at 0, pred = gt + noise randn (the construction of the `metrics` fixture), fp32 (*shape, 17, 3), millimetres"""
    g = np.random.default_rng(seed)
    gt = (400.0 * g.standard_normal(tuple(shape) + (NJ, 3))).astype(F32)
    gt[..., 0, :] = 0
    return (gt + (noise * g.standard_normal(gt.shape)).astype(F32)).astype(F32), gt


def case_mask(B, L, seed):
    """(B, L, 17) bytes: 80 % visible, different for every batch item, about one frame in eight fully invisible, visible bytes of any non-zero value"""
    g = np.random.default_rng(seed)
    m = (g.random((B, L, NJ)) > 0.2) & (g.random((B, L, 1)) > 0.125)
    if not m.any():
        m[0, 0, 1] = True
    return (m * g.integers(1, 256, m.shape)).astype(np.uint8)


def near_threshold(e, S, thr, margin):
    """(…, 17) bool: the error is closer than margin x its scale to one of the thresholds"""
    return (np.abs(e[..., None] - thr) < margin * S[..., None]).any(-1)


def pose_near(pred, gt, var, margin):
    r = pose_metrics_ref(pred, gt, None, var["ps"], var["gs"], var["pck"], var["auc_max"], var["auc_steps"], var["align"])
    return near_threshold(r["e"], r["e_scale"], thresholds_of(var["pck"], var["auc_max"], var["auc_steps"]), margin)


def proc_near(pred, gt, var, margin, axis_free=False):
    r = procrustes_ref(pred, gt, None, var["ps"], var["gs"], var["pck"], var["auc_max"], var["auc_steps"], axis_free)
    return near_threshold(r["e"], r["e_scale"], thresholds_of(var["pck"], var["auc_max"], var["auc_steps"]), margin)


def settle(pred, near, seed, skip=None):
    """move every predicted joint whose error lies within SETTLE of a threshold in any of the calls `near(pred)` evaluates by a fraction of
    a millimetre (2^-10 of the largest coordinate of the case) until none does; `skip`: planted joints that stay"""
    g = np.random.default_rng(seed)
    pred = pred.copy()
    step = F32(np.abs(pred).max() * 2.0 ** -10)
    for _ in range(40):
        bad = near(pred)
        if skip is not None:
            bad &= ~skip
        if not bad.any():
            return pred
        pred[bad] = (pred[bad] + step * g.standard_normal(pred[bad].shape).astype(F32)).astype(F32)
    raise AssertionError("settle: errors stay within the margin of a threshold")


def variant(gt=True, mask=False, align=False, pck=150.0, auc_max=150.0, auc_steps=31, ps=1.0, gs=1.0):
    return dict(gt=gt, mask=mask, align=align, pck=pck, auc_max=auc_max, auc_steps=auc_steps, ps=ps, gs=gs)


def vname(v):
    return f"gt={int(v['gt'])} mask={int(v['mask'])} align={int(v['align'])} pck={v['pck']:g} auc={v['auc_max']:g}/{v['auc_steps']} scales={v['ps']:g},{v['gs']:g}"


V_FULL = [variant(), variant(mask=True), variant(align=True), variant(mask=True, align=True), variant(gt=False), variant(mask=True, pck=80.0)]
V_METRES = [variant(ps=1000.0, gs=1000.0), variant(mask=True, align=True, ps=1000.0, gs=1000.0), variant(pck=0.15, auc_max=0.15),
            variant(mask=True, pck=0.08, auc_max=0.15), variant(align=True, pck=0.15, auc_max=0.15), variant(gt=False, ps=1000.0)]
V_PLAIN = [variant(), variant(mask=True), variant(gt=False)]
V_TIES = [variant(), variant(mask=True), variant(pck=80.0), variant(mask=True, pck=80.0)]

FRAME_CASES = ["frames_L1", "frames_L2", "metres_L1", "metres_L2", "ties"]                       # B = 70 (ties: 31) items of one or two frames
STAGED_L, STRIDED_L = (127, 128, 129, 257), (255, 256, 257, 513)
EDGE_CASES = [f"B{b}L{l}" for b in (1, 3) for l in sorted(set(STAGED_L + STRIDED_L))] + ["metres_B3L257", "spike_L257", "spike_L513", "rigid_L257"]
POSE_CASES = FRAME_CASES + EDGE_CASES
TIE_JOINT, SPIKE_JOINT = 5, 6


def rigid_frames(L, seed, offset=5000.0):
    """(1, L, 17, 3): constant bone lengths 200 .. 300 mm in random directions (the `metrics` fixture's walk down the tree), the root
    `offset` mm from the origin in every coordinate"""
    g = np.random.default_rng(seed)
    lens = 200.0 + 100.0 * g.random(NB)
    x = np.zeros((1, L, NJ, 3))
    x[:, :, 0] = offset
    for j in range(1, NJ):
        d = g.standard_normal((1, L, 3))
        x[:, :, j] = x[:, :, PARENTS[j]] + lens[j - 1] * d / np.linalg.norm(d, axis=-1, keepdims=True)
    return x.astype(F32)


@functools.lru_cache(maxsize=None)
def pose_case(name):
    """dict(pred, gt (B, L, 17, 3) fp32, mask (B, L, 17) uint8, variants, planted (B, L, 17) bool or None, rigid bool)"""
    seed = 1000 + POSE_CASES.index(name)
    planted, rigid = None, False
    if name == "ties":
        # integer millimetres: joint TIE_JOINT of item i is displaced by exactly 5 i (i = 0 .. 30: every grid value, 80 = 5 x 16 and 150 = 5 x 30
        # among them) along one axis, every other joint by (1, 1, 1): e == threshold holds exactly in fp32
        g = np.random.default_rng(seed)
        gt = g.integers(-600, 601, (31, 1, NJ, 3)).astype(F32)
        pred = gt + F32(1.0)
        pred[:, 0, TIE_JOINT] = gt[:, 0, TIE_JOINT]
        for i in range(31):
            pred[i, 0, TIE_JOINT, i % 3] += F32(5.0 * i)
        planted = np.zeros((31, 1, NJ), dtype=bool)
        planted[:, :, TIE_JOINT] = True
        variants = V_TIES
    elif name.startswith("spike"):
        # prediction == target except joint SPIKE_JOINT of the first frame of the second chunk (frame 128 of the staged form for L = 257,
        # frame 256 of the strided form for L = 513): every error sum and the whole velocity sum come from that frame and the one after it
        L = int(name.split("L")[1])
        _, gt = skeleton_frames((1, L), seed)
        pred = gt.copy()
        pred[0, 128 if L == 257 else 256, SPIKE_JOINT] += np.array([37.25, -61.5, 112.75], dtype=F32)
        variants = V_PLAIN
    elif name.startswith("rigid"):
        pred = rigid_frames(257, seed)
        gt = (skeleton_frames((1, 257), seed)[1] + F32(5000.0)).astype(F32)
        variants, rigid = V_PLAIN + [variant(align=True)], True
    else:
        metres = name.startswith("metres")
        if name.startswith(("frames", "metres_L")):
            B, L = 70, int(name[-1])
        elif metres:
            B, L = 3, 257
        else:
            B, L = int(name[1]), int(name.split("L")[1])
        pred, gt = skeleton_frames((B, L), seed)
        if metres:
            pred, gt = (pred / F32(1000.0)).astype(F32), (gt / F32(1000.0)).astype(F32)
        variants = V_METRES if metres else V_FULL
    vs = [v for v in variants if v["gt"]]
    if rigid:                                                               # the rigid prediction stays as it is: the target's joints move
        gt = settle(gt, lambda q: np.any([pose_near(pred, q, v, SETTLE) for v in vs], axis=0), seed)
    else:
        pred = settle(pred, lambda p: np.any([pose_near(p, gt, v, SETTLE) for v in vs], axis=0), seed, skip=planted)
    B, L = pred.shape[:2]
    return dict(pred=pred, gt=gt, mask=case_mask(B, L, seed + 500), variants=variants, planted=planted, rigid=rigid)


PROC_N = (1, 255, 256, 257, 600)
PROC_VARIANTS = [variant(), variant(pck=80.0)]


@functools.lru_cache(maxsize=None)
def procrustes_case(N):
    """dict(pred, gt (N, 17, 3), mask (N, 17)): random frames; frames 255, 256 and the last one carry five times the noise, so that a frame
    dropped or doubled at a workgroup edge moves the sum by far more than the bound"""
    seed = 2000 + N
    pred, gt = skeleton_frames((N,), seed)
    big = [f for f in (255, 256, N - 1) if 0 < f < N]
    for k, f in enumerate(big):
        pred[f] = (gt[f] + (300.0 + 40.0 * k) * np.random.default_rng(seed + 1 + k).standard_normal((NJ, 3))).astype(F32)
    pred = settle(pred, lambda p: np.any([proc_near(p, gt, v, SETTLE) for v in PROC_VARIANTS], axis=0), seed)
    return dict(pred=pred, gt=gt, mask=case_mask(1, N, seed + 500)[0])


def _rotation(g):
    q, _ = np.linalg.qr(g.standard_normal((3, 3)))
    if np.linalg.det(q) < 0:
        q[:, 0] *= -1
    return q


@functools.lru_cache(maxsize=None)
def procrustes_specials():
    """the named single frames: list of dict(name, pred, gt (1, 17, 3) fp32, ps, gs, axis_free)"""
    g = np.random.default_rng(3000)
    out = []

    def add(name, pred, gt, ps=1.0, gs=1.0, axis_free=False):
        pred, gt = np.asarray(pred, dtype=F32)[None], np.asarray(gt, dtype=F32)[None]
        var = variant(ps=ps, gs=gs)
        pred = settle(pred, lambda p: np.any([proc_near(p, gt, dict(var, pck=t), SETTLE, axis_free) for t in (150.0, 80.0)], axis=0), 3000 + len(out))
        out.append(dict(name=f"{name}{sum(o['name'].startswith(name) for o in out)}", pred=pred, gt=gt, ps=ps, gs=gs, axis_free=axis_free))

    for i in range(4):
        p, t = skeleton_frames((), 3100 + i)
        add("generic", p, t)
    for i, s in enumerate((0.37, 1.0, 2.5, 0.01, 40.0)):                     # a rotated, scaled and shifted copy of the target: aligned error ~ 0
        _, t = skeleton_frames((), 3110 + i)
        add("similar", ((t.astype(F64) - g.normal(0, 300, 3)) @ _rotation(g)) / s, t)
    for i in range(4):                                                        # a mirror image (x -> -x) of the target, a little noise: the reflection fix
        p, t = skeleton_frames((), 3120 + i, noise=20.0)
        add("mirror", p * np.array([-1.0, 1.0, 1.0]), t)
    for i in range(4):                                                        # target and prediction in one plane each (z = 0; the prediction's plane rotated)
        p, t = skeleton_frames((), 3130 + i)
        p[:, 2], t[:, 2] = 0, 0
        add("planar", p.astype(F64) @ _rotation(g) if i % 2 else p, t)
    for i in range(3):                                                        # all target joints on one line
        p, _ = skeleton_frames((), 3140 + i)
        d = g.standard_normal(3)
        add("collinear", p, g.normal(0, 300, 3) + (400.0 * g.standard_normal(NJ))[:, None] * d / np.linalg.norm(d), axis_free=True)
    for i in range(4):                                                        # 5 m from the origin: the centring cancels
        p, t = skeleton_frames((), 3150 + i)
        off = np.array([5000.0, -5000.0, 5000.0])[[i % 3, (i + 1) % 3, (i + 2) % 3]]
        add("far", p + off, t + off)
    for i, s in enumerate((0.01, 0.01, 100.0, 100.0)):                        # a prediction 100 x too small / too large
        p, t = skeleton_frames((), 3160 + i)
        add("misscaled", p.astype(F64) * s, t)
    for i in range(3):                                                        # metres with both scales 1000
        p, t = skeleton_frames((), 3170 + i)
        add("metres", p / F32(1000.0), t / F32(1000.0), 1000.0, 1000.0)
    fx = np.load(os.path.join(GOLDEN, "metrics.npz"))
    for i, (nm, b, f) in enumerate((("pred", 0, 0), ("pred", 1, 150), ("pred", 2, 300), ("pred", 0, 77), ("rigid", 0, 0), ("rigid", 1, 150),
                                    ("rigid", 2, 300), ("rigid", 1, 1))):
        add("fixture_" + nm, fx[nm][b, f], fx["gt"][b, f])
    return out


# the three unequal batches of the host-arithmetic test: (B, L) and whether the batch is rigid
REPORT_BATCHES = ((2, 40, False), (1, 97, True), (3, 23, False))


@functools.lru_cache(maxsize=None)
def report_case():
    """[(pred, gt)] of REPORT_BATCHES, millimetres, settled for the alignments none / scale / procrustes at the default thresholds and 80"""
    out = []
    for i, (B, L, rigid) in enumerate(REPORT_BATCHES):
        pred, gt = skeleton_frames((B, L), 4000 + i)
        if rigid:                                                           # a rigid prediction, the target 60 mm of noise around it
            pred = np.concatenate([rigid_frames(L, 4100 + i + b, offset=0.0) for b in range(B)])
            gt = (pred + (gt - skeleton_frames((B, L), 4000 + i)[0])).astype(F32)
        vs = [variant(), variant(align=True), variant(pck=80.0)]
        near = lambda p, q: np.any([pose_near(p, q, v, SETTLE) for v in vs] +
                                   [proc_near(p.reshape(-1, NJ, 3), q.reshape(-1, NJ, 3), v, SETTLE).reshape(p.shape[:3]) for v in PROC_VARIANTS], axis=0)
        if rigid:                                                           # the rigid prediction stays as it is: the target's joints move
            gt = settle(gt, lambda q: near(pred, q), 4000 + i)
        else:
            pred = settle(pred, lambda p: near(p, gt), 4000 + i)
        out.append((pred, gt))
    return out

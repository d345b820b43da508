"""mp_lift_align_views' rule (include/manipose_hip.h) stated in numpy float64, the seeded scenes its tests share, and their bounds.

The statement works on the float32 inputs the kernel gets and follows the header step by step; the 4x4 eigenproblem is numpy.linalg.eigh's.  It also
returns what the kernel does not: the relative eigenvalue gap (lambda_1 - lambda_2) / lambda_1 of the last solve, the condition of the rotation.
The device tests hold their bounds only where that gap is >= GAP_MIN."""
import functools

import numpy as np

GAP = 1e-9          # the header's degenerate rule: (lambda_1 - lambda_2) <= GAP |lambda_1|
GAP_MIN = 0.1       # the device tests' bounds are claimed for scenes at least this well conditioned
QUAT_TOL = 2.0 ** -23


def quat_matrix(q):
    w, x, y, z = np.asarray(q, np.float64)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def canonical(q):
    """w >= 0; if w == 0 the first non-zero component is positive"""
    q = np.asarray(q, np.float64)
    nz = np.nonzero(q)[0]
    return -q + 0.0 if nz.size and q[nz[0]] < 0 else q + 0.0


def horn_n(M):
    """Horn's symmetric 4x4 matrix of M[a][c] = sum b_v[a] b_ref[c] for the rotation taking b_v onto b_ref, quaternion (w, x, y, z)"""
    return np.array([[M[0, 0] + M[1, 1] + M[2, 2], M[1, 2] - M[2, 1], M[2, 0] - M[0, 2], M[0, 1] - M[1, 0]],
                     [M[1, 2] - M[2, 1], M[0, 0] - M[1, 1] - M[2, 2], M[0, 1] + M[1, 0], M[2, 0] + M[0, 2]],
                     [M[2, 0] - M[0, 2], M[0, 1] + M[1, 0], -M[0, 0] + M[1, 1] - M[2, 2], M[1, 2] + M[2, 1]],
                     [M[0, 1] - M[1, 0], M[2, 0] + M[0, 2], M[1, 2] + M[2, 1], -M[0, 0] - M[1, 1] + M[2, 2]]])


def solve(M, sw):
    """step 4 on the sums: (q canonical or None where degenerate, lambda_1, lambda_2)"""
    if not (np.isfinite(M).all() and np.isfinite(sw) and sw > 0):
        return None, 0.0, 0.0
    lam, vec = np.linalg.eigh(horn_n(M))
    if not lam[3] > 0:
        return None, lam[3], lam[2]
    q = vec[:, 3] / np.linalg.norm(vec[:, 3])
    return canonical(q), lam[3], lam[2]


def residual(bv, br, R):
    """e_f = (sum_j |b_ref - R b_v|^2) / J of (n, J, 3) bodies"""
    d = br - bv @ R.T
    return (d * d).sum(axis=(1, 2)) / bv.shape[1]


def weights(e, sigma):
    """w = 1 / (1 + e / sigma^2)^2, sigma the float32 number the entry point is given"""
    with np.errstate(over="ignore"):
        s2 = np.float64(np.float32(sigma)) * np.float64(np.float32(sigma))
        t = 1.0 + e / s2
        return 1.0 / (t * t)


DEGENERATE = dict(quat=np.array([1.0, 0, 0, 0]), trans=np.zeros(3), rms=0.0, trans_rms=0.0, ok=0, gap=0.0)


def align_view(xv, xr, both, sigma, iters, tv=None, tr=None, tok=None):
    """One view against the reference over a take: xv, xr (n, J, 3) float64, both (n,) bool: valid in both.  A dict of the row."""
    used = both & np.isfinite(xv).all(axis=(1, 2)) & np.isfinite(xr).all(axis=(1, 2))
    row = dict(DEGENERATE, used=int(used.sum()))
    if not used.any():
        return row
    bv, br = xv[used] - xv[used][:, :1], xr[used] - xr[used][:, :1]
    S = np.einsum("fja,fjc->fac", bv, br)
    w = np.ones(bv.shape[0])
    q, l1, l2 = solve((w[:, None, None] * S).sum(0), w.sum())
    for _ in range(iters):
        if q is None:
            return row
        w = weights(residual(bv, br, quat_matrix(q)), sigma)
        q, l1, l2 = solve((w[:, None, None] * S).sum(0), w.sum())
    if q is None or (l1 - l2) <= GAP * abs(l1):
        return row
    R = quat_matrix(q)
    row.update(quat=q, ok=1, gap=(l1 - l2) / l1, rms=float(np.sqrt((w * residual(bv, br, R)).sum() / w.sum())))
    if tv is not None:
        sel = tok[used]
        if sel.any():
            d, ws = (tr[used] - tv[used] @ R.T)[sel], w[sel]
            with np.errstate(all="ignore"):
                T = (ws[:, None] * d).sum(0) / ws.sum()
                t2 = (ws * ((d - T) ** 2).sum(1)).sum() / ws.sum()
            if ws.sum() > 0 and np.isfinite(ws.sum()) and np.isfinite(T).all() and np.isfinite(t2):
                row.update(trans=T, trans_rms=float(np.sqrt(t2)), ok=3)
    return row


def align(poses, valid=None, off=None, traj=None, traj_ok=None, sigma=0.05, iters=5):
    """The rule on float32 inputs: dict of quat (G, V, 4), trans (G, V, 3), rms, trans_rms, gap (G, V) float64, used (G, V) int32, ok (G, V) uint8.
    trans and trans_rms are zeros without traj."""
    V, ftot = poses.shape[:2]
    off = np.array([0, ftot]) if off is None else np.clip(np.asarray(off, np.int64), 0, ftot)
    G = len(off) - 1
    x = poses[..., :3].astype(np.float64)
    val = np.ones((V, ftot), bool) if valid is None else valid != 0
    out = dict(quat=np.tile([1.0, 0, 0, 0], (G, V, 1)), trans=np.zeros((G, V, 3)), rms=np.zeros((G, V)), trans_rms=np.zeros((G, V)),
               gap=np.zeros((G, V)), used=np.zeros((G, V), np.int32), ok=np.zeros((G, V), np.uint8))
    for g in range(G):
        sl = slice(int(off[g]), int(max(off[g], off[g + 1])))
        have = [v for v in range(V) if val[v, sl].any()]
        if not have:
            continue
        r = have[0]
        out["used"][g, r], out["ok"][g, r] = int(val[r, sl].sum()), 1
        for v in range(V):
            if v == r:
                continue
            kw = {}
            if traj is not None:
                kw = dict(tv=traj[v, sl].astype(np.float64), tr=traj[r, sl].astype(np.float64), tok=(traj_ok[v, sl] != 0) & (traj_ok[r, sl] != 0))
            row = align_view(x[v, sl], x[r, sl], val[v, sl] & val[r, sl], sigma, iters, **kw)
            for k, a in row.items():
                out[k][g, v] = a
    return out


def compose(quat, trans, ok, ref_quat, ref_trans):
    """align_views' reference= in float64, through rotation matrices: R = R_ref R_v (as a canonical quaternion), T = R_ref T_v + T_ref; the rows
    without bit 0 stay; T is composed where bit 1 is set and for the reference view (the lowest view of the take with bit 0)"""
    q, t = np.array(quat, np.float64), None if trans is None else np.array(trans, np.float64)
    for g in range(q.shape[0]):
        a = np.asarray(ref_quat[g], np.float64)
        Rr = quat_matrix(a / np.linalg.norm(a))
        rot = [v for v in range(q.shape[1]) if ok[g][v] & 1]
        for v in rot:
            q[g, v] = matrix_quat(Rr @ quat_matrix(q[g, v]))
            if t is not None and (ok[g][v] & 2 or v == rot[0]):
                t[g, v] = Rr @ t[g, v] + np.asarray(ref_trans[g], np.float64)
    return q, t


def matrix_quat(R):
    """the canonical unit quaternion of a rotation matrix: the dominant eigenvector of Horn's matrix of R^T"""
    lam, vec = np.linalg.eigh(horn_n(R.T))
    return canonical(vec[:, 3] / np.linalg.norm(vec[:, 3]))


def angle_deg(q, p):
    """the angle between two rotations given as unit quaternions, in degrees"""
    a, b = np.asarray(p, np.float64), np.asarray(q, np.float64)          # conj(p) q; the arc tangent is accurate at small angles, the arc cosine is not
    w = a @ b
    vec = a[0] * b[1:] - b[0] * a[1:] - np.cross(a[1:], b[1:])
    return float(np.degrees(2.0 * np.arctan2(np.linalg.norm(vec), abs(w))))


def random_rotation(g):
    q = g.standard_normal(4)
    return quat_matrix(q / np.linalg.norm(q))


def scene(V, J, lens, seed, noise=0.01, mirrored=0.0, C=3, size=0.3):
    """A seeded scene of G = len(lens) takes: per take random camera rotations Rc_v and positions t_v, per frame a random root-relative body
    (joint spread `size` metres) and a world root; view v sees x = Rc_v body + Gaussian noise, in a `mirrored` share of the frames of every view
    but the first its depth (camera z) negated - the lifter's mirror ambiguity.  Returns dict: poses (V, Ftot, J, C) float32 with joint 0 at
    the camera-space root (C = 4: channel 3 a score that must not be read), off (G + 1), traj (V, Ftot, 3), traj_ok (V, Ftot) all 1, and the
    truth quat (G, V, 4), trans (G, V, 3) with view 0 as the reference: x_0 = R_v x_v + T_v."""
    g = np.random.default_rng(seed)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    ftot = int(off[-1])
    poses = np.zeros((V, ftot, J, C), np.float32)
    traj = np.zeros((V, ftot, 3), np.float32)
    quat, trans = np.zeros((len(lens), V, 4)), np.zeros((len(lens), V, 3))
    for t, n in enumerate(lens):
        sl = slice(int(off[t]), int(off[t + 1]))
        body = size * g.standard_normal((n, J, 3))
        body[:, 0] = 0.0
        root = np.array([0.0, 0.0, 1.0]) + 0.5 * g.standard_normal((n, 3))
        Rc = [random_rotation(g) for _ in range(V)]
        tc = [np.array([0.0, 0.0, 4.0]) + 0.5 * g.standard_normal(3) for _ in range(V)]
        for v in range(V):
            b = body @ Rc[v].T + noise * g.standard_normal((n, J, 3))
            b[:, 0] = 0.0
            flip = (g.random(n) < mirrored) & (v > 0)                    # (drawn in any case: the scene without mirrored frames is the same scene)
            b[flip, :, 2] *= -1.0
            cam_root = root @ Rc[v].T + tc[v]
            traj[v, sl] = cam_root
            poses[v, sl, :, :3] = b + traj[v, sl][:, None].astype(np.float64)
            Rv = Rc[0] @ Rc[v].T
            quat[t, v], trans[t, v] = matrix_quat(Rv), tc[0] - Rv @ tc[v]
    if C == 4:
        poses[..., 3] = g.random((V, ftot, J)).astype(np.float32)
    return dict(poses=poses, off=off, traj=traj, traj_ok=np.ones((V, ftot), np.uint8), quat=quat, trans=trans)


def valid_table(V, off, seed, missing=None):
    """gaps in valid: about one frame in five of every view; `missing`: (take, view) pairs absent in all frames of the take"""
    g = np.random.default_rng(seed)
    valid = (g.random((V, int(off[-1]))) > 0.2).astype(np.uint8)
    for t, v in missing or ():
        valid[v, int(off[t]):int(off[t + 1])] = 0
    return valid


@functools.lru_cache(maxsize=None)
def cases():
    """(tag, inputs dict for align(), want) of the device test: the lane stride's edges in F, J = 2, 5, 17, V = 1, 2, 4 with a missing view, three
    takes in one call, gaps in valid, a NaN coordinate, C = 4, iters 0, 1, 8, sigma = inf, with and without traj"""
    out = []

    def add(tag, sc, traj=True, **kw):
        inp = dict(poses=sc["poses"], off=sc["off"], **kw)
        if traj:
            inp.update(traj=sc["traj"], traj_ok=kw.get("traj_ok", sc["traj_ok"]))
        out.append((tag, inp, align(**inp)))

    for n, (F, J, V) in enumerate(((1, 5, 2), (255, 2, 2), (256, 17, 4), (257, 5, 4), (600, 17, 2))):
        # (one frame alone has no traj: its trans_rms is |d - (w d) / w|, 0 up to fp64 noise, and an array of nothing but noise has no float32 ulp to
        # be held to; the one-frame take of "three takes" below has its translation compared, beside takes whose trans_rms is a number)
        add(f"F={F} J={J} V={V}", scene(V, J, [F], seed=100 + n, mirrored=0.25 if F > 1 else 0.0), traj=F > 1)
    add("V=1: the reference alone", scene(1, 5, [7], seed=110))
    sc = scene(4, 17, [1, 257, 40], seed=111, mirrored=0.3)
    add("three takes", sc)
    add("three takes, no traj", sc, traj=False)
    valid = valid_table(4, sc["off"], 112, missing=((1, 0), (2, 2)))
    tok = valid_table(4, sc["off"], 113)
    add("three takes, gaps in valid, view 0 missing in take 1, view 2 in take 2, gaps in traj_ok", sc, valid=valid, traj_ok=tok)
    nan = dict(sc, poses=sc["poses"].copy())
    nan["poses"][1, 5, 3, 1] = np.nan
    nan["poses"][0, 200, 0, 2] = np.inf                                 # (the root of a frame of the reference view)
    add("a NaN and an infinite coordinate", nan)
    sc4 = scene(4, 17, [1, 257, 40], seed=116, mirrored=0.3, C=4)
    add("C = 4", sc4)
    for iters in (0, 1, 8):
        add(f"iters={iters}", sc, iters=iters)
    add("sigma=inf", sc, sigma=float("inf"))
    add("sigma=0.02, 5 joints", scene(3, 5, [24, 24], seed=115, mirrored=0.25), sigma=0.02)
    return out


def close_quat(got, want):
    """every component within 2^-23 (both canonical)"""
    return np.abs(np.asarray(got, np.float64) - want) <= QUAT_TOL


def ulp_bound(want):
    """one float32 ulp of the largest magnitude in `want`"""
    return float(np.spacing(np.float32(np.abs(want).max()))) if np.size(want) else 0.0


# ---- the recovery scene --------------------------------------------------------------------------------------------------------------------
RECOVERY = dict(V=4, J=17, lens=(60,), seed=7, noise=0.01, mirrored=0.3)


@functools.lru_cache(maxsize=None)
def recovery():
    """60 frames, 17 joints, 4 views, noise 0.01 m, 30 % of the frames of views 1..3 depth-mirrored; and the same scene (same seed: the same
    cameras, bodies and noise up to the stream's position) without the mirrored frames.  Returns (dirty scene, clean scene)."""
    kw = dict(RECOVERY, lens=list(RECOVERY["lens"]))
    return scene(**kw), scene(**dict(kw, mirrored=0.0))


def errors_deg(sc, **kw):
    """per view 1..V-1 of take 0: the angle between the statement's rotation and the scene's true one"""
    res = align(sc["poses"], None, sc["off"], **kw)
    return [angle_deg(res["quat"][0, v], sc["quat"][0, v]) for v in range(1, sc["poses"].shape[0])], res

"""mp_lift_ground's rule (include/manipose_hip.h) stated in numpy float64, the seeded scenes its tests share, and their bounds.

The statement works on the float32 inputs the kernel gets and follows the header step by step.  The squared speed of step A is formed with the
kernel's operations in the kernel's order; every sum is numpy's, in numpy's order, and the eigenproblem is numpy's eigh on A itself (the kernel
runs a Jacobi on s I - A).  It also returns what the kernel does not: per sequence the eigenvalues of the last solve, n . b, the smallest relative
distance of a squared speed from the threshold, the scales the bounds are written in, and - with ``jitter`` - the same rule with every solve's
sums disturbed, from which ``amplification`` measures how far a relative error of the sums travels into each output.

The scene generator makes a WALKER ON A FLOOR: a 40-frame step cycle, 60 % of it stance with the ankle exactly still, a swing arc above the floor,
a pelvis and a thorax above the feet, the other joints hung on the pelvis; the whole scene is moved by a random rotation and a translation of a
few metres, so neither up nor the floor's height can be read from the coordinates."""
import functools

import numpy as np

U = 2.0 ** -53
SPEED_MARGIN = 1e-9   # |d^2 - thr^2| / thr^2 of every compared (frame, foot): both sides form d^2 with the same operations, a margin for good measure
GAP_MIN = 1e-4        # (a2 - a1) / (a3 - a1) of a compared row with a plane: an eigenvector moves by the matrix's error over the eigenvalue gap
FLAT_MAX = 1e-12      # (a2 - a1) / max(|a1|, |a3|) of a compared row that has no plane for want of a gap: nowhere near the rule's 1e-9
SIDE_MIN = 0.1        # |n . b| of a compared row whose side the axis decided
SEQ_LENS = (1, 5, 64, 257, 300)
# The recovery scene (300 frames, 5 mm of noise, 10 % hover frames), THE FLOAT64 STATEMENT ON THE CPU over the seeds 0..7: the RMS distance of the
# true stance positions from the estimated plane in metres, the angle to the true normal in degrees - measured 0.17 .. 0.75 mm and 0.016 .. 0.173
# degrees (seed by seed: 0.56, 0.75, 0.17, 0.32, 0.19, 0.66, 0.20, 0.35 mm; 0.041, 0.095, 0.028, 0.016, 0.042, 0.173, 0.043, 0.031 degrees); the
# bounds are twice the worst, for seeds not tried.  With prior = 0 the same scenes give at most 0.77 mm and 0.186 degrees: the data decide.
# A stand-still scene (5 mm of noise, three seeds): 0.010 .. 0.085 degrees with the default prior, 3.7 .. 62.9 degrees with prior = 0.
# Synthetic walkers; not a result on real data.
RECOVERY_SEEDS = tuple(range(8))
RECOVERY_BOUND = {"rms_m": 2 * 0.00075, "angle_deg": 2 * 0.173}


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(np.float32)).astype(np.float64)


def _unit_quat_rot(n):
    """step D: the shortest rotation taking n onto +z"""
    w = 1.0 + n[2]
    if w < 1e-12:
        return np.array([0.0, 1.0, 0.0, 0.0])
    q = np.array([w, n[1], 0.0 - n[0], 0.0])
    return q * (1.0 / np.sqrt((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]))


def qrot(q, v):
    """mp_lift_world's qrot"""
    u = q[1:]
    return v + 2.0 * (q[0] * np.cross(u, v) + np.cross(u, np.cross(u, v)))


def ground(points, off=None, valid=None, feet=(3, 6), axis=(0, 8), radius=2, speed=0.01, sigma=0.03, prior=0.05, iters=5, foot_height=0.0, jitter=None):
    """the rule on points (Ntot, J, C) float32 -> a dict of float64 / integer arrays under the kernel's names, plus ``eig`` (S, 3), ``side`` (S),
    ``speed_margin``, ``scale`` (S): the largest |coordinate| of a foot in a good, finite frame of the sequence, ``step`` (S): the longest step of a
    contact pair.  ``jitter`` = (generator, delta): every solve's m and C, and the axis, are disturbed by delta relative to scale, tr C and 1"""
    points = np.asarray(points)
    assert points.dtype == np.float32 and points.ndim == 3
    ntot, J, _ = points.shape
    off = np.array([0, ntot]) if off is None else np.asarray(off)
    S, nf, r = len(off) - 1, len(feet), int(radius)
    x = points[..., :3].astype(np.float64)
    good = np.ones(ntot, bool) if valid is None else np.asarray(valid) != 0
    finite = np.isfinite(x).all(axis=2)                                   # (Ntot, J)
    thr = (2.0 * r) * float(np.float32(speed))
    thr2 = thr * thr
    sigma2 = float(np.float32(sigma)) * float(np.float32(sigma))
    prior2 = float(np.float32(prior)) * float(np.float32(prior))
    fh = float(np.float32(foot_height))
    out = dict(normal=np.zeros((S, 3)), offset=np.zeros(S), quat=np.zeros((S, 4)), trans=np.zeros((S, 3)), rms=np.zeros(S), gap=np.zeros(S),
               used=np.zeros(S, np.int32), ok=np.zeros(S, np.uint8), contact=np.zeros((ntot, nf), np.uint8), height=np.zeros((ntot, nf)),
               skate=np.zeros(S), skate_pairs=np.zeros(S, np.int32), eig=np.zeros((S, 3)), side=np.zeros(S), scale=np.zeros(S), step=np.zeros(S))
    out["normal"][:, 2] = 1.0
    out["quat"][:, 0] = 1.0
    margin = np.inf
    for s in range(S):
        f0 = min(max(int(off[s]), 0), ntot)
        f1 = min(max(int(off[s + 1]), f0), ntot)
        n = f1 - f0
        p, g = x[f0:f1], good[f0:f1]
        contact = np.zeros((n, nf), bool)
        # A
        for k, j in enumerate(feet):
            fin = finite[f0:f1, j] & g
            if n > 2 * r:
                both = fin[r:n - r] & fin[:n - 2 * r] & fin[2 * r:]
                with np.errstate(invalid="ignore", over="ignore"):
                    d = p[2 * r:, j] - p[:n - 2 * r, j]
                    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
                    contact[r:n - r, k] = both & (d2 <= thr2)
                if both.any():
                    margin = min(margin, float(np.abs(d2[both] - thr2).min() / thr2))
        out["contact"][f0:f1] = contact
        # B
        fa = g & finite[f0:f1, axis[0]] & finite[f0:f1, axis[1]]
        b = None
        if fa.any():
            d = p[fa, axis[1]] - p[fa, axis[0]]
            dn = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
            keep = dn >= 1e-12
            B = (d[keep] / dn[keep, None]).sum(axis=0) if keep.any() else np.zeros(3)
            bn = np.sqrt((B[0] * B[0] + B[1] * B[1]) + B[2] * B[2])
            if np.isfinite(bn) and bn >= 1e-12:
                b = B / bn
                if jitter is not None:
                    b = b + jitter[1] * jitter[0].standard_normal(3)
                    b = b / np.linalg.norm(b)
        # C
        fi, ki = np.nonzero(contact)                                      # frames in order, within a frame the feet in order
        X = p[fi, np.asarray(feet)[ki]]
        used = len(X)
        out["used"][s] = used
        feetfin = g[:, None] & finite[f0:f1][:, list(feet)]
        scale = float(np.abs(p[:, list(feet)][feetfin]).max()) if feetfin.any() else 0.0
        out["scale"][s] = scale
        plane, nrm, offset, w = used >= 3, np.array([0.0, 0.0, 1.0]), 0.0, np.ones(used)
        eig, sided = np.zeros(3), False
        for it in range(iters + 1 if plane else 0):
            if it > 0:
                res = X @ nrm - offset
                t = 1.0 + (res * res) / sigma2
                w = 1.0 / (t * t)
            W = w.sum()
            if not (np.isfinite(W) and W > 0):
                plane = False
                break
            m = (w[:, None] * X).sum(axis=0) / W
            u = X - m
            Cm = np.einsum("i,ij,ik->jk", w, u, u)
            if jitter is not None:
                e = jitter[0].standard_normal((3, 3))
                m = m + jitter[1] * scale * jitter[0].standard_normal(3)
                Cm = Cm + jitter[1] * np.trace(Cm) * 0.5 * (e + e.T)
            A = Cm - prior2 * W * np.outer(b, b) if b is not None and prior2 > 0 else Cm
            if not (np.isfinite(A).all() and np.isfinite(m).all()):
                plane = False
                break
            eig, vec = np.linalg.eigh(A)
            if not eig[1] - eig[0] > 1e-9 * max(abs(eig[0]), abs(eig[2])):
                plane = False
                break
            nrm = vec[:, 0] / np.linalg.norm(vec[:, 0])
            side = float(nrm @ b) if b is not None else 0.0
            sided = side != 0.0
            if (side < 0) if sided else (nrm[np.nonzero(nrm)[0][0]] < 0):
                nrm = 0.0 - nrm
            offset = float(nrm @ m) + 0.0
        out["eig"][s], out["side"][s] = eig, (abs(float(nrm @ b)) if b is not None and plane else 0.0)
        # E: the skate, with or without a plane
        pair = contact[:-1] & contact[1:] if n > 1 else np.zeros((0, nf), bool)
        fi2, ki2 = np.nonzero(pair)
        out["skate_pairs"][s] = len(fi2)
        if len(fi2):
            jj = np.asarray(feet)[ki2]
            d = p[fi2 + 1, jj] - p[fi2, jj]
            out["step"][s] = float(np.linalg.norm(d, axis=1).max())
            if plane:
                d = d - (d @ nrm)[:, None] * nrm
            out["skate"][s] = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).sum() / len(fi2)
        if not plane:
            continue
        # D, E
        out["normal"][s], out["offset"][s], out["quat"][s] = nrm, offset, _unit_quat_rot(nrm)
        out["trans"][s] = (0.0, 0.0, fh - offset)
        res = X @ nrm - offset
        out["rms"][s] = np.sqrt((w * res * res).sum() / w.sum())
        out["gap"][s] = (eig[1] - eig[0]) / (eig[2] - eig[0]) if eig[2] > eig[0] else 0.0
        out["ok"][s] = 3 if sided else 1
        with np.errstate(invalid="ignore", over="ignore"):
            h = np.where(feetfin, (p[:, list(feet)] @ nrm - offset) + 0.0, 0.0)
        out["height"][f0:f1] = h
    out["speed_margin"] = margin
    return out


FLOATS = ("normal", "offset", "quat", "trans", "rms", "gap", "height", "skate")


def scales(want):
    """what each float output's error is measured in (the module docstring of test_gpu_lift_ground.py derives them): 1 for the unit vectors and the
    gap, the sequence's largest foot coordinate for the lengths along the normal, the longest contact step for the skate"""
    S = len(want["ok"])
    L = np.maximum(want["scale"], 1e-30)
    return dict(normal=np.ones((S, 1)), quat=np.ones((S, 1)), gap=np.ones(S), offset=L, trans=L[:, None], rms=L, skate=np.maximum(want["step"], 1e-30))


def frame_scale(want, off):
    """scale (S) spread over the frames (Ntot, 1)"""
    out = np.full((len(want["height"]), 1), 1e-30)
    for s in range(len(off) - 1):
        out[int(off[s]):int(off[s + 1])] = max(want["scale"][s], 1e-30)
    return out


def bound(key, want, off):
    """the largest |device - statement| of a float output: one float32 ulp of max(|want|, its scale)"""
    sc = frame_scale(want, off) if key == "height" else scales(want)[key]
    return ulp32(np.maximum(np.abs(want[key]), sc))


def amplification(inp, want, draws=3, delta=1e-9, seed=0):
    """How far a relative disturbance delta of every solve's sums travels: max over the float outputs and ``draws`` disturbed runs of
    |disturbed - want| / (its scale) / delta, over the rows with a plane.  (A sampled figure, not a worst case: the bound leaves it a factor.)"""
    g = np.random.default_rng(seed)
    worst = 0.0
    has = (want["ok"] & 1).astype(bool)
    for _ in range(draws):
        got = ground(inp["points"], inp["off"], inp.get("valid"), **inp["opts"], jitter=(g, delta))
        assert np.array_equal(got["ok"], want["ok"]) and np.array_equal(got["contact"], want["contact"])
        for key in FLOATS:
            sc = frame_scale(want, inp["off"]) if key == "height" else scales(want)[key]
            err = np.abs(got[key] - want[key]) / sc
            if key != "height":
                err = err[has]
            worst = max(worst, float(err.max()) / delta if err.size else 0.0)
    return worst


def sum_error(want):
    """the relative error of a solve's sums between two fp64 summations in different orders: N terms, each side at most N u of the sum of the
    absolute terms (the diagonal's are the sum itself, the others at most half the trace), three roundings per product, 6 entries: 8 N u"""
    return 8.0 * max(int(want["used"].max()), 1) * U


# ---- scenes ----------------------------------------------------------------------------------------------------------------------------------
CYCLE, STANCE = 40, 24


def _rotation(g):
    q = g.standard_normal(4)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def _foothold(side, c):
    """where foot `side` (-1, +1) stands in its cycle c: a gently curved path, a function of the cycle alone (the stance is exactly still)"""
    x = 0.6 * c + 0.3 * (side > 0)
    return np.array([x, 0.1 * side + 0.5 * np.sin(0.7 * x), 0.0])


def walker(seed, frames, J=17, feet=(3, 6), axis=(0, 8), noise=0.0, hover=0.0, still=False, invalid=0.0, poison=False, C=3, move=True):
    """A walker on the floor z = 0, moved by a random rotation and translation.  Returns a dict: points (frames, J, C) float32, valid (frames) uint8
    or None, normal (3) and offset: the true plane n . x = offset in the moved frame, stance (frames, nf) bool: the foot is exactly still on the
    floor, truth (frames, nf, 3) float64: the feet without noise in the moved frame.  ``hover``: that share of the frames, in one run, the last
    foot is held still 0.15 m above the floor; ``still``: nobody walks, the pelvis sways; ``invalid``: that share of the frames is marked invalid
    and, with ``poison``, filled with NaN - and a foot of some valid frames with an infinity."""
    g = np.random.default_rng(seed)
    nf = len(feet)
    pos = np.zeros((frames, J, 3))
    stance = np.zeros((frames, nf), bool)
    foot = np.zeros((frames, nf, 3))
    for k in range(nf):
        side, phase = (1 if k % 2 else -1) * (1 + k // 2), 20 * k
        for f in range(frames):
            c, t = divmod(f + phase, CYCLE)
            if still:
                foot[f, k], stance[f, k] = _foothold(side, 0), True
            elif t < STANCE:
                foot[f, k], stance[f, k] = _foothold(side, c), True
            else:
                u = (t - STANCE + 1) / (CYCLE - STANCE + 1)
                e = 0.5 - 0.5 * np.cos(np.pi * u)
                foot[f, k] = (1 - e) * _foothold(side, c) + e * _foothold(side, c + 1) + np.array([0, 0, 0.12 * np.sin(np.pi * u)])
    if hover > 0 and not still and frames >= 40:
        n, k = max(int(round(hover * frames)), 1), nf - 1
        a = int(g.integers(10, max(frames - n - 10, 11)))
        foot[a:a + n, k] = foot[a, k] * [1, 1, 0] + [0, 0, 0.15]
        stance[a:a + n, k] = False
    t = np.arange(frames)
    centre = foot.mean(axis=1) * [1, 1, 0] + np.stack([0.02 * np.sin(0.13 * t), 0.02 * np.cos(0.11 * t), 0 * t], 1)
    hang = 0.25 * g.standard_normal((J, 3)) + [0, 0, 0.9]
    pos[:] = centre[:, None] + hang[None]
    pos[:, axis[0]] = centre + [0, 0, 0.9]
    pos[:, axis[1]] = centre + [0, 0, 1.4] + np.stack([0.03 * np.sin(0.2 * t), 0.03 * np.sin(0.17 * t), 0 * t], 1)
    for k, j in enumerate(feet):
        pos[:, j] = foot[:, k]
    noisy = pos + noise * g.standard_normal(pos.shape)
    R, T = (_rotation(g), g.uniform(-3, 3, 3)) if move else (np.eye(3), np.zeros(3))
    pts = np.zeros((frames, J, C), np.float32)
    pts[..., :3] = (noisy @ R.T + T).astype(np.float32)
    if C == 4:
        pts[..., 3] = g.random((frames, J)).astype(np.float32)
    valid = None
    if invalid > 0:
        valid = (g.random(frames) >= invalid).astype(np.uint8)
        if poison:
            pts[valid == 0] = np.nan
            for f in g.choice(frames, size=max(frames // 50, 1), replace=False):
                pts[f, feet[int(g.integers(nf))], int(g.integers(3))] = np.inf
    return dict(points=pts, valid=valid, normal=R[:, 2].copy(), offset=float(R[:, 2] @ T), stance=stance, truth=foot @ R.T + T)


def take(seed, lens=SEQ_LENS, **kw):
    """sequences of walkers laid end to end, each with its own motion: (points, valid or None, off)"""
    ws = [walker(seed * 100 + i, n, **kw) for i, n in enumerate(lens)]
    valid = None if ws[0]["valid"] is None else np.concatenate([w["valid"] for w in ws])
    return np.concatenate([w["points"] for w in ws]), valid, np.concatenate([[0], np.cumsum(lens)])


DEFAULTS = dict(feet=(3, 6), axis=(0, 8), radius=2, speed=0.01, sigma=0.03, prior=0.05, iters=5, foot_height=0.0)


def _case(tag, seed, scene, **opts):
    o = dict(DEFAULTS, **opts)
    pts, valid, off = take(seed, feet=o["feet"], axis=o["axis"], **scene)
    inp = dict(points=pts, valid=valid, off=off, opts=o)
    return tag, inp, ground(pts, off, valid, **o)


@functools.lru_cache(maxsize=None)
def cases():
    """(tag, inputs, the statement's outputs): five sequences of 1, 5, 64, 257 and 300 frames in every call - no speed at all, shorter than a wave,
    the 256-lane stride and a remainder - over the joint counts, channels, feet, radii and the options that switch a part of the rule off"""
    noisy = dict(noise=0.002, hover=0.1, invalid=0.1, poison=True)
    return (
        _case("J=17 C=3, two feet, noise, hover, invalid frames poisoned", 1, noisy, foot_height=0.08),
        _case("J=5 C=4 feet (3, 4), radius 1", 2, dict(J=5, C=4, noise=0.001, hover=0.1), feet=(3, 4), axis=(0, 1), radius=1),
        _case("one foot, radius 3", 3, dict(noise=0.002, invalid=0.05, poison=True), feet=(3,), radius=3),
        _case("sigma = inf", 4, dict(noise=0.002, hover=0.1), sigma=float("inf")),
        _case("iters = 0", 5, dict(noise=0.002, hover=0.1), iters=0),
        _case("prior = 0", 6, dict(noise=0.002, hover=0.1), prior=0.0),
        _case("no noise, no mask, C=4", 7, dict(C=4)),
        _case("four feet, eight solves", 8, dict(noise=0.003, hover=0.05), feet=(3, 6, 13, 16), iters=8, speed=0.012),
    )


# ---- constructed rows: dyadic numbers, on which the kernel is exact ---------------------------------------------------------------------------
def dyadic_scene(frames=48, slide=0.0, flip=False):
    """Two feet (joints 3, 6) standing on z = 0 at dyadic positions, joint 0 at z = 1 and joint 8 at z = 2 above them; the first foot moves by
    ``slide`` (dyadic, along x) per frame.  ``flip``: the scene turned by exactly 180 degrees about x (y, z -> -y, -z)."""
    pts = np.zeros((frames, 17, 3), np.float32)
    pts[:, :, 0] = 0.5 * np.arange(17)[None]
    pts[:, :, 1] = 0.25
    pts[:, :, 2] = 1.5
    pts[:, 3] = (1.0, 0.5, 0.0)
    pts[:, 3, 0] += np.float32(slide) * np.arange(frames, dtype=np.float32)
    pts[:, 6] = (2.0, 1.75, 0.0)
    pts[:frames // 2, 6] = (0.25, 3.0, 0.0)                               # (the second foot takes one step: three holds, not on a line)
    pts[:, 0] = (1.0, 1.0, 1.0)
    pts[:, 8] = (1.0, 1.0, 2.0)
    if flip:
        pts[..., 1:] = -pts[..., 1:]
    return pts


# ---- recovery ----------------------------------------------------------------------------------------------------------------------------------
def recovery_scene(seed, noise=0.005, hover=0.1, still=False):
    return walker(1000 + seed, 300, noise=noise, hover=hover, still=still)


def recovery_error(scene, normal, offset):
    """(the RMS distance in metres of the scene's TRUE stance positions from the plane normal . x = offset, the angle in degrees between normal
    and the true one)"""
    pts = scene["truth"][scene["stance"]]
    d = pts @ np.asarray(normal, np.float64) - float(offset)
    cosine = float(np.clip(np.asarray(normal, np.float64) @ scene["normal"], -1, 1))
    return float(np.sqrt((d * d).mean())), float(np.degrees(np.arccos(cosine)))

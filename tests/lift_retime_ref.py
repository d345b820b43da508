"""Forward kinematics of (root, quaternions, bone lengths) and a take resampled in time on its rotations: the float64 numpy statements of
mp_lift_fk's and mp_lift_retime's rules (include/manipose_hip.h), written from the header's text and not from the kernels - world rotations are
3 x 3 matrices here (the kernel carries quaternions), the taps of a window are walked by explicit loops (the kernel hands coefficients round a
wavefront) - with the scenes and the cases the GPU tests run.

What lets a float32 bound stand: the sampled time t = start + (h den) / num is one exact product, one division and one addition of float64
numbers, the same IEEE operations on both sides, so floor(t), the window |k - t| <= R, the bracketing and the nearest tap are decided on identical
bits.  The one decision taken on rounded numbers is the hemisphere, dot(a, b) < 0: ``retime`` returns the least |dot| it met, and the largest
relative rotation angle, and test_lift_retime_host.py asserts |dot| >= 1e-6 and angle <= pi - 1e-3 on every case."""
import functools
from fractions import Fraction

import numpy as np

import lift_rot_ref as rot

TOL = 2.0 ** -23                # one unit in the last place of 1.0: both sides round the same component of a unit quaternion to float32
LENS = (1, 2, 3, 67, 130)       # a single frame, a pair, a triple, a sequence boundary inside a wave, and one past 128 frames
RATES = ((1, 1), (3, 5), (6, 5), (2, 1), (1, 3))         # (fps_out, fps_in) = (num, den)
MAXR = 64


# ---- mp_lift_fk ------------------------------------------------------------------------------------------------------------------------------
def seq_of(off, g):
    """the last s with off[s] <= g, inside 0 .. S-1"""
    S = len(off) - 1
    s = 0
    for k in range(S):
        if int(off[k]) <= g:
            s = k
    return s


def fk(quat, lengths, parents, rest, root=None, off=None):
    """The rule of mp_lift_fk on float32 quat (Ntot, inner, J, 4): (poses (Ntot, inner, J, 3) float64 BEFORE the final rounding, ok (Ntot, inner)
    uint8).  ``lengths`` (S, J - 1) with ``off`` (S + 1), or per pose (Ntot, inner, J - 1) with off None; root (Ntot, inner, 3) float32 or None."""
    tb = rot.tables(parents, rest)
    J, par, r = tb["J"], tb["parents"], tb["rest"]
    q32 = np.asarray(quat, np.float32)
    ntot, inner = q32.shape[:2]
    q = q32.astype(np.float64)
    L = np.asarray(lengths, np.float32).astype(np.float64)
    out = np.zeros((ntot, inner, J, 3))
    ok = np.zeros((ntot, inner), np.uint8)
    for g in range(ntot):
        row = None if off is None else seq_of(off, g)
        for i in range(inner):
            base = np.zeros(3) if root is None else np.asarray(root, np.float32)[g, i].astype(np.float64)
            with np.errstate(all="ignore"):
                n2 = (q[g, i] * q[g, i]).sum(-1)
            if not (np.isfinite(n2) & (n2 >= 1e-12)).all():
                out[g, i] = base
                continue
            u = q[g, i] / np.sqrt(n2)[:, None]
            M = rot.matrix(u)
            Rw, p = [M[0]], [base]
            lens = L[g, i] if off is None else L[row]
            for j in range(1, J):
                Rw.append(Rw[par[j]] @ M[j])
                p.append(p[par[j]] + Rw[j] @ (lens[j - 1] * r[j]))
            out[g, i] = np.stack(p)
            ok[g, i] = 1
    return out, ok


# ---- mp_lift_retime --------------------------------------------------------------------------------------------------------------------------
def qmul(a, b):
    aw, ax, ay, az = (a[..., k] for k in range(4))
    bw, bx, by, bz = (b[..., k] for k in range(4))
    return np.stack([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw], -1)


def conj(a):
    return a * np.array([1.0, -1.0, -1.0, -1.0])


def qlog(r):
    """s = |r.xyz|; 0 where s == 0, else 2 atan2(s, r.w) r.xyz / s"""
    s = np.sqrt((r[..., 1:] ** 2).sum(-1))
    with np.errstate(all="ignore"):
        f = np.where(s == 0, 0.0, 2.0 * np.arctan2(s, r[..., 0]) / s)
    return np.where((s == 0)[..., None], 0.0, f[..., None] * r[..., 1:])


def qexp(v):
    """a = |v|; (1, 0, 0, 0) where a == 0, else (cos(a / 2), sin(a / 2) v / a)"""
    a = np.sqrt((v * v).sum(-1))
    with np.errstate(all="ignore"):
        g = np.where(a == 0, 0.0, np.sin(0.5 * a) / a)
    return np.concatenate([np.where(a == 0, 1.0, np.cos(0.5 * a))[..., None], g[..., None] * v], -1)


def unit(q):
    with np.errstate(all="ignore"):
        return q / np.sqrt((q * q).sum(-1))[..., None]


def aligned_log(a, b, m):
    """log(conj(a) (+-b)), b negated where dot(a, b) < 0; m collects the least |dot| and the largest angle"""
    d = (a * b).sum(-1)
    b = np.where((d < 0)[..., None], -b, b)
    v = qlog(qmul(conj(a), b))
    if np.isfinite(d).all():
        m["dot"] = min(m["dot"], float(np.abs(d).min()))
        m["angle"] = max(m["angle"], float(np.sqrt((v * v).sum(-1)).max()))
    return v


def taper_of(dk, R, taper):
    if taper == 0:
        return 1.0
    r = dk / float(R + 1)
    q = 1.0 - r * r
    return q * q


def coefficients(ks, t, R, degree, taper):
    """(c_k of the valid taps ks (increasing), the reference tap k*): the first row of the inverse normal matrix by cofactors, sums in increasing k"""
    S0 = S1 = S2 = S3 = S4 = 0.0
    left = right = False
    best, kstar = np.inf, None
    for k in ks:
        dk = float(k) - t
        w, u = taper_of(dk, R, taper), dk / float(R)
        wu = w * u
        wu2 = wu * u
        left, right = left or dk <= 0, right or dk >= 0
        if abs(dk) < best:
            best, kstar = abs(dk), k
        S0, S1, S2, S3, S4 = S0 + w, S1 + wu, S2 + wu2, S3 + wu2 * u, S4 + wu2 * u * u
    d = min(degree, len(ks) - 1)
    if not (left and right):
        d = 0
    a0 = a1 = a2 = 0.0
    if d <= 0:
        a0 = 1.0 / S0
    elif d == 1:
        det = S0 * S2 - S1 * S1
        a0, a1 = S2 / det, -S1 / det
    else:
        c0, c1, c2 = S2 * S4 - S3 * S3, S1 * S4 - S2 * S3, S1 * S3 - S2 * S2
        det = S0 * c0 - S1 * c1 + S2 * c2
        a0, a1, a2 = c0 / det, -c1 / det, c2 / det
    c = []
    for k in ks:
        dk = float(k) - t
        u = dk / float(R)
        c.append(taper_of(dk, R, taper) * (a0 + u * (a1 + u * a2)))
    return c, kstar


def retime(quat, root, valid, off, out_off, clock, R, degree, taper, mtot=None, storage=np.float32):
    """The rule of mp_lift_retime on float32 quat (Ntot, inner, J, 4), root (Ntot, inner, 3) or None, valid (Ntot, inner) or None: a dict of quat
    (Mtot, inner, J, 4) and root (Mtot, inner, 3) float64 BEFORE the final rounding (copied frames: the input's float32 values), ok, taps uint8,
    copied (Mtot, inner) bool, time (Mtot,), and the margins dot / angle / window (the least distance of a |k - t| from R that is not 0).  ``storage``
    np.float64: the input is taken as it is, for the properties that hold in exact arithmetic."""
    q32 = np.asarray(quat, storage)
    ntot, inner, J = q32.shape[:3]
    q = q32.astype(np.float64)
    r = None if root is None else np.asarray(root, storage).astype(np.float64)
    mtot = int(out_off[-1]) if mtot is None else mtot
    ident = np.zeros((J, 4))
    ident[:, 0] = 1.0
    out_q = np.tile(ident, (mtot, inner, 1, 1))
    out_r = np.zeros((mtot, inner, 3))
    ok, taps = np.zeros((mtot, inner), np.uint8), np.zeros((mtot, inner), np.uint8)
    copied = np.zeros((mtot, inner), bool)
    time = np.zeros(mtot)
    m = dict(dot=np.inf, angle=0.0, window=np.inf)
    clamp = lambda v, lo, hi: min(max(int(v), lo), hi)
    for g in range(mtot):
        s = seq_of(out_off, g)                                       # the last sequence whose first output frame is not past g
        f0 = clamp(off[s], 0, ntot)
        f1 = clamp(off[s + 1], f0, ntot)
        o0 = clamp(out_off[s], 0, mtot)
        o1 = clamp(out_off[s + 1], o0, mtot)
        n = f1 - f0
        if not o0 <= g < o1 or n == 0:
            continue
        start, num, den = (float(v) for v in clock[s])
        if not num > 0:
            num = 1.0
        with np.errstate(all="ignore"):
            t = start + np.float64(float(g - o0) * den) / np.float64(num)
        t = float(t)
        clamped = not (0.0 <= t <= n - 1)
        t = 0.0 if not t >= 0.0 else min(t, float(n - 1))
        time[g] = t
        for i in range(inner):
            good = lambda k: valid is None or valid[f0 + k, i] != 0
            flag = 2 if clamped else 0
            if R == 0:
                k = int(np.floor(t))
                al = t - k
                if al == 0:
                    out_q[g, i] = q[f0 + k, i]
                    if r is not None:
                        out_r[g, i] = r[f0 + k, i]
                    ok[g, i], taps[g, i], copied[g, i] = (1 if good(k) else 0) | flag, 1, True
                elif good(k) and good(k + 1):
                    a, b = unit(q[f0 + k, i]), unit(q[f0 + k + 1, i])
                    out_q[g, i] = qmul(a, qexp(al * aligned_log(a, b, m)))
                    if r is not None:
                        out_r[g, i] = (1.0 - al) * r[f0 + k, i] + al * r[f0 + k + 1, i]
                    ok[g, i], taps[g, i] = 1 | flag, 2
                else:
                    ok[g, i] = flag
                continue
            ks = []
            for k in range(n):
                gap = abs(float(k) - t) - R
                if gap != 0:
                    m["window"] = min(m["window"], abs(gap))
                if gap <= 0 and good(k):
                    ks.append(k)
            if not ks:
                ok[g, i] = flag
                continue
            c, kstar = coefficients(ks, t, R, degree, taper)
            a = unit(q[f0 + kstar, i])
            acc, racc = np.zeros((J, 3)), np.zeros(3)
            for ck, k in zip(c, ks):
                acc = acc + ck * aligned_log(a, unit(q[f0 + k, i]), m)
                if r is not None:
                    racc = racc + ck * r[f0 + k, i]
            out_q[g, i] = qmul(a, qexp(acc))
            out_r[g, i] = racc
            ok[g, i], taps[g, i] = 1 | flag, len(ks)
    return dict(quat=out_q + 0.0, root=out_r + 0.0, ok=ok, taps=taps, copied=copied, time=time, margins=m)


def frame_count(n, num, den, start=0):
    """the output frames of a sequence of n frames: the h >= 0 with start + h den / num <= n - 1, in exact rational arithmetic"""
    room = Fraction(n - 1) - Fraction(start)
    if room < 0:
        return 0
    return int(room * num / den) + 1                                    # (int() of a non-negative Fraction is its floor)


def starts(lens, start):
    """one start per sequence: ``start``, and 0 for a sequence of a single frame (a start past the last frame is refused by the bindings)"""
    return [0.0 if n == 1 else float(start) for n in lens]


def plan(lens, num, den, start=0.0):
    """(off, out_off, clock) of sequences of ``lens`` frames laid end to end; ``start`` one number or one per sequence"""
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    st = [float(start)] * len(lens) if np.ndim(start) == 0 else [float(v) for v in start]
    counts = [frame_count(n, num, den, v) for n, v in zip(lens, st)]
    out_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    clock = np.array([[v, float(num), float(den)] for v in st])
    return off, out_off, clock


# ---- scenes ----------------------------------------------------------------------------------------------------------------------------------
def smooth_tracks(g, n, inner, J, speed=0.012, wobble=0.15):
    """(n, inner, J, 4) float64 unit quaternions of a smooth motion with bounded angular acceleration: every (inner, joint) track is
    q0 exp(axis_1 (w t + A sin(f t))) exp(axis_2 B sin(f2 t)), |w| <= speed rad a frame; sign-continuous by construction, then checked"""
    t = np.arange(n, dtype=np.float64)[:, None, None]
    q0 = rot._random_rotations(g, (inner, J), np.pi)
    ax = g.standard_normal((2, inner, J, 3))
    ax /= np.sqrt((ax * ax).sum(-1))[..., None]
    w = g.uniform(-speed, speed, (inner, J))
    f = g.uniform(0.02, 0.08, (2, inner, J))
    amp = g.uniform(0.0, wobble, (2, inner, J))
    th1 = w * t + amp[0] * np.sin(f[0] * t)
    th2 = amp[1] * np.sin(f[1] * t + 1.0)
    q = qmul(qmul(np.broadcast_to(q0, (n, inner, J, 4)), qexp(th1[..., None] * ax[0])), qexp(th2[..., None] * ax[1]))
    for k in range(1, n):                                                # (continuous in time: consecutive frames share a hemisphere)
        flip = (q[k] * q[k - 1]).sum(-1) < 0
        q[k] = np.where(flip[..., None], -q[k], q[k])
    return q


def smooth_root(g, n, inner):
    t = np.arange(n, dtype=np.float64)[:, None, None]
    return (g.uniform(-1, 1, (inner, 3)) + g.uniform(-0.01, 0.01, (inner, 3)) * t + 0.2 * np.sin(g.uniform(0.02, 0.1, (inner, 3)) * t)
            + np.array([0.0, 0.0, 4.0]))


def take(kind="h36m", inner=1, lens=LENS, holes="none", R=4, seed=0):
    """A scene: dict of quat (Ntot, inner, J, 4) float32 (each sequence a smooth motion of its own, scaled off the unit sphere a little: the
    operator normalises), root (Ntot, inner, 3) float32, valid (Ntot, inner) uint8 or None, lens, parents, rest.  ``holes``: "none" (valid None),
    "single" (every 7th frame of an inner index invalid, staggered) or "run" (as single, and frames 20 .. 20 + 2R + 2 of every sequence that long:
    a hole run longer than the window)."""
    parents, rest = rot.skeleton(kind)
    J = len(parents)
    g = np.random.default_rng(1000 + seed)
    ntot = int(sum(lens))
    q = np.concatenate([smooth_tracks(g, n, inner, J) for n in lens]) * g.uniform(0.8, 1.25, (ntot, inner, J, 1))
    r = np.concatenate([smooth_root(g, n, inner) for n in lens])
    valid = None
    if holes != "none":
        valid = np.ones((ntot, inner), np.uint8)
        for i in range(inner):
            valid[(3 + 2 * i) % 7::7, i] = 0
        if holes == "run":
            f0 = 0
            for n in lens:
                if n > 20:
                    valid[f0 + 20:min(f0 + 20 + 2 * R + 3, f0 + n)] = 0
                f0 += n
    return dict(quat=np.ascontiguousarray(q.astype(np.float32)), root=np.ascontiguousarray(r.astype(np.float32)), valid=valid, lens=tuple(lens),
                parents=parents, rest=rest, kind=kind)


def cases():
    """The cases the device is held to: (id, kind, inner, holes, (num, den), start, radius, degree, taper).  Between them: every length of LENS in
    every case, inner 1 and 5, J 17 / 2 / 32, every rate of RATES, start 0 and 0.25, radius 0 / 1 / 4 / 64, degree 0..2, both tapers, valid null,
    with single holes, and with a hole run longer than 2R + 1."""
    rows = [
        ("h36m", 1, "none", (1, 1), 0.0, 0, 2, 0), ("h36m", 5, "single", (3, 5), 0.0, 0, 2, 0), ("h36m", 1, "none", (6, 5), 0.25, 0, 2, 0),
        ("pair", 5, "none", (2, 1), 0.0, 0, 2, 0), ("chain", 1, "single", (1, 3), 0.25, 0, 2, 0),
        ("h36m", 1, "none", (1, 1), 0.0, 4, 2, 0), ("h36m", 5, "single", (3, 5), 0.0, 4, 2, 1), ("h36m", 1, "run", (6, 5), 0.25, 4, 1, 0),
        ("h36m", 5, "run", (2, 1), 0.0, 1, 2, 1), ("h36m", 1, "single", (1, 3), 0.0, 1, 0, 0), ("h36m", 1, "none", (3, 5), 0.25, 1, 1, 1),
        ("pair", 5, "single", (6, 5), 0.0, 4, 0, 1), ("pair", 1, "run", (1, 1), 0.0, 1, 1, 0), ("chain", 1, "none", (2, 1), 0.0, 4, 2, 0),
        ("chain", 5, "run", (3, 5), 0.0, 4, 1, 1), ("h36m", 1, "none", (1, 1), 0.0, 64, 2, 0), ("h36m", 1, "single", (3, 5), 0.25, 64, 1, 1),
        ("pair", 5, "run", (6, 5), 0.0, 64, 2, 1), ("chain", 1, "single", (1, 3), 0.0, 64, 0, 0), ("h36m", 5, "none", (2, 1), 0.25, 4, 2, 1),
    ]
    return [(f"{k}-i{i}-{h}-{r[0]}by{r[1]}-s{st}-R{R}-d{d}-t{tp}", k, i, h, r, st, R, d, tp) for k, i, h, r, st, R, d, tp in rows]


@functools.lru_cache(maxsize=None)
def solved(case_id):
    """a case's scene, its tables and the statement on it, computed once and left unchanged"""
    _, kind, inner, holes, (num, den), start, R, degree, taper = next(c for c in cases() if c[0] == case_id)
    sc = take(kind, inner, LENS, holes, max(R, 1), seed=len(case_id) + inner + R)
    off, out_off, clock = plan(sc["lens"], num, den, starts(sc["lens"], start))
    want = retime(sc["quat"], sc["root"], sc["valid"], off, out_off, clock, R, degree, taper)
    for a in (sc["quat"], sc["root"], want["quat"], want["root"], want["ok"], want["taps"]):
        a.setflags(write=False)
    return sc, (off, out_off, clock), want


def geodesic(a, b):
    """the angle between rotations a and b (unit quaternions, any sign), radians"""
    return 2.0 * np.arccos(np.clip(np.abs((a * b).sum(-1)), 0.0, 1.0))

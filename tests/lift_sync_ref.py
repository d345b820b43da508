"""mp_lift_sync_views' and mp_lift_shift_views' rules (include/manipose_hip.h) stated in numpy float64, the seeded scenes their tests share, and
their bounds.

The statement works on the float32 inputs the kernel gets and follows the header step by step; its sums are numpy's, in numpy's order.  It also
returns what the kernel does not: the fp64 curve, per row the relative margin of the best curve value below the runner-up and, where step 6
applies, den / c[d*].  The device tests hold lag_int and lag to the statement only where these are >= MARGIN_MIN and >= DEN_MIN.

The scene generator draws a motion that is SMOOTH IN TIME (a few sinusoids per joint coordinate): lift_align_ref.scene draws a new body per frame,
which has no lag to find."""
import functools

import numpy as np

MARGIN_MIN = 1e-9     # (runner-up - best) / runner-up of a compared row: the fp64 orders of summation differ by 1e-15 or so
DEN_MIN = 1e-4        # den / c[d*] of a compared row with a sub-frame part: delta's relative error is the curve's over this
FLOOR = 2.0 ** -48    # times the take's largest distance squared: below it a curve value is cancellation noise (test_gpu_lift_sync.py derives it)


def signals(poses, valid, off):
    """steps 1 and 2: (d - m (V, Ftot, J - 1) float64 with 0 at unusable frames, usable (V, Ftot) bool, used (G, V), dmax (G,): the largest
    distance of a usable frame of the take)"""
    V, ftot, J = poses.shape[:3]
    G = len(off) - 1
    x = poses[..., :3].astype(np.float64)
    b = x[:, :, 1:] - x[:, :, :1]
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.sqrt((b[..., 0] * b[..., 0] + b[..., 1] * b[..., 1]) + b[..., 2] * b[..., 2])
    usable = np.isfinite(x).all(axis=(2, 3)) & (np.ones((V, ftot), bool) if valid is None else valid != 0)
    s = np.zeros((V, ftot, J - 1))
    used, dmax = np.zeros((G, V), np.int32), np.zeros(G)
    inside = np.zeros(ftot, bool)
    for g in range(G):
        sl = slice(int(off[g]), int(max(off[g], off[g + 1])))
        inside[sl] = True
        for v in range(V):
            u = usable[v, sl]
            used[g, v] = int(u.sum())
            if u.any():
                dv = d[v, sl]
                s[v, sl][u] = dv[u] - dv[u].sum(axis=0) / int(u.sum())
                dmax[g] = max(dmax[g], float(dv[u].max()))
    return s, usable & inside, used, dmax


def curve_of(sv, uv, sr, ur, L, min_overlap, sigma2):
    """step 4 for one view against the reference over one take: sv, sr (n, J - 1), uv, ur (n,) bool -> (2 L + 1,) float64, +inf where ineligible"""
    n, D = sv.shape
    c = np.full(2 * L + 1, np.inf)
    for d in range(-L, L + 1):
        lo, hi = max(0, -d), min(n, n - d)                                 # f and f + d inside the take
        if hi <= lo:
            continue
        pair = ur[lo:hi] & uv[lo + d:hi + d]
        nd = int(pair.sum())
        if nd < min_overlap:
            continue
        t = sv[lo + d:hi + d][pair] - sr[lo:hi][pair]
        with np.errstate(over="ignore", invalid="ignore"):
            e = (t * t).sum(axis=1) / D
            val = (e / (1.0 + e / sigma2)).sum() / nd
        if np.isfinite(val):
            c[d + L] = val
    return c


def pick(c, L):
    """steps 5 to 7 on one fp64 curve: dict(lag float64, lag_int, contrast float64, ok, margin, den_ratio)"""
    row = dict(lag=0.0, lag_int=0, contrast=0.0, ok=0, margin=np.inf, den_ratio=np.inf)
    lags = np.arange(-L, L + 1)
    elig = np.isfinite(c)
    if not elig.any():
        return row
    order = sorted(lags[elig], key=lambda d: (c[d + L], abs(d), -d))
    best = int(order[0])
    cb = c[best + L]
    if len(order) > 1:
        ru = c[order[1] + L]
        row["margin"] = (ru - cb) / ru if ru > 0 else 0.0
    delta, ok = 0.0, 1
    if abs(best) < L and elig[best + L - 1] and elig[best + L + 1]:
        lo, hi = c[best + L - 1], c[best + L + 1]
        den = (lo - 2.0 * cb) + hi
        if den > 0:
            delta = min(max(0.5 * (lo - hi) / den, -0.5), 0.5)
            ok = 3
            row["den_ratio"] = den / cb if cb > 0 else np.inf
    mean = c[elig].sum() / int(elig.sum())
    row.update(lag=best + delta, lag_int=best, ok=ok, contrast=1.0 - cb / mean if mean > 0 else 0.0)
    return row


def sync(poses, valid=None, off=None, max_lag=32, min_overlap=16, sigma=0.05):
    """The rule on float32 inputs: dict of lag, contrast (G, V) float64, lag_int, used (G, V) int32, curve (G, V, 2 L + 1) float64, ok (G, V)
    uint8, and margin, den_ratio (G, V), dmax (G,) for the tests' conditions and floor."""
    V, ftot = poses.shape[:2]
    off = np.array([0, ftot]) if off is None else np.clip(np.asarray(off, np.int64), 0, ftot)
    G, L = len(off) - 1, int(max_lag)
    s, usable, used, dmax = signals(poses, valid, off)
    with np.errstate(over="ignore"):
        sigma2 = np.float64(np.float32(sigma)) * np.float64(np.float32(sigma))
    out = dict(lag=np.zeros((G, V)), lag_int=np.zeros((G, V), np.int32), curve=np.zeros((G, V, 2 * L + 1)), contrast=np.zeros((G, V)), used=used,
               ok=np.zeros((G, V), np.uint8), margin=np.full((G, V), np.inf), den_ratio=np.full((G, V), np.inf), dmax=dmax)
    for g in range(G):
        sl = slice(int(off[g]), int(max(off[g], off[g + 1])))
        have = [v for v in range(V) if used[g, v] > 0]
        if not have:
            continue
        r = have[0]
        out["ok"][g, r] = 1
        for v in range(V):
            if v == r:
                continue
            c = curve_of(s[v, sl], usable[v, sl], s[r, sl], usable[r, sl], L, int(min_overlap), sigma2)
            out["curve"][g, v] = c
            for k, a in pick(c, L).items():
                out[k][g, v] = a
    return out


def shift(x, lag, valid=None, off=None, mode="linear"):
    """mp_lift_shift_views on float32 x (V, Ftot, ...), lag (G, V) float32: (out float32 like x, valid_out (V, Ftot) uint8); the kernel's arithmetic"""
    V, ftot = x.shape[:2]
    off = np.array([0, ftot]) if off is None else np.clip(np.asarray(off, np.int64), 0, ftot)
    lag = np.asarray(lag, np.float32).reshape(len(off) - 1, V)
    rows = np.ascontiguousarray(x, np.float32).reshape(V, ftot, -1)
    out, vout = np.zeros_like(rows), np.zeros((V, ftot), np.uint8)
    val = np.ones((V, ftot), bool) if valid is None else valid != 0
    for g in range(len(off) - 1):
        f0, n = int(off[g]), int(max(off[g], off[g + 1])) - int(off[g])
        for v in range(V):
            if not np.isfinite(lag[g, v]):
                continue
            for f in range(n):
                p = np.float64(f) + np.float64(lag[g, v])
                i = np.floor(p + 0.5) if mode == "nearest" else np.floor(p)
                a = 0.0 if mode == "nearest" else p - i
                two = a != 0.0
                if not (i >= 0 and i + (1 if two else 0) < n):
                    continue
                i = int(i)
                if not (val[v, f0 + i] and (not two or val[v, f0 + i + 1])):
                    continue
                vout[v, f0 + f] = 1
                if two:
                    out[v, f0 + f] = ((1.0 - a) * rows[v, f0 + i].astype(np.float64) + a * rows[v, f0 + i + 1].astype(np.float64)).astype(np.float32)
                else:
                    out[v, f0 + f] = rows[v, f0 + i]
    return out.reshape(x.shape), vout


# ---- scenes --------------------------------------------------------------------------------------------------------------------------------
def random_rotation(g):
    q = g.standard_normal(4)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def scene(V, J, lens, seed, true_lag=None, noise=0.01, mirrored=0.0, outliers=0.0, C=3, size=0.3, waves=4):
    """A seeded scene of G = len(lens) takes with a motion that is smooth in time: per take every root-relative joint coordinate is a constant
    (joint spread `size` metres) plus `waves` sinusoids with periods of 20 to 120 frames and amplitudes of about 0.1 m, and the root walks on
    sinusoids of its own.  Frame f of view v shows the body at time f - true_lag[v] (frames; None: zeros) - so frame f + true_lag[v] of view v shows
    what frame f of a view without lag shows, the header's step 8 -, rotated by a random camera, plus Gaussian noise;
    in a `mirrored` share of the frames of every view but the first its depth (camera z) is negated - the lifter's mirror ambiguity - and an
    `outliers` share of the frames of every view is replaced by a gross outlier, a body of independent Gaussians.  Returns dict: poses
    (V, Ftot, J, C) float32 with joint 0 at the camera-space root (C = 4: channel 3 a score that must not be read), off (G + 1), traj (V, Ftot, 3),
    traj_ok (V, Ftot) all 1, lag (V,) the truth."""
    g = np.random.default_rng(seed)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    ftot = int(off[-1])
    lag = np.zeros(V) if true_lag is None else np.asarray(true_lag, np.float64)
    poses, traj = np.zeros((V, ftot, J, C), np.float32), np.zeros((V, ftot, 3), np.float32)
    for t, n in enumerate(lens):
        sl = slice(int(off[t]), int(off[t + 1]))
        rest = size * g.standard_normal((J, 3))
        amp = 0.1 * g.standard_normal((waves, J, 3))
        freq = 2.0 * np.pi / g.uniform(20.0, 120.0, (waves, J, 3))
        phase = g.uniform(0.0, 2.0 * np.pi, (waves, J, 3))
        r_amp, r_freq, r_phase = 0.5 * g.standard_normal((2, 3)), 2.0 * np.pi / g.uniform(60.0, 240.0, (2, 3)), g.uniform(0.0, 2.0 * np.pi, (2, 3))

        def body(time):
            b = rest + (amp * np.sin(freq * time[:, None, None, None] + phase)).sum(axis=1)
            b[:, 0] = 0.0
            return b, np.array([0.0, 0.0, 1.0]) + (r_amp * np.sin(r_freq * time[:, None, None] + r_phase)).sum(axis=1)

        for v in range(V):
            Rc, tc = random_rotation(g), np.array([0.0, 0.0, 4.0]) + 0.5 * g.standard_normal(3)
            b, root = body(np.arange(n, dtype=np.float64) - lag[v])
            b = b @ Rc.T + noise * g.standard_normal((n, J, 3))
            flip = (g.random(n) < mirrored) & (v > 0)                    # (drawn in any case: the scene without them is the same scene)
            b[flip, :, 2] *= -1.0
            gross = g.random(n) < outliers
            wild = size * g.standard_normal((n, J, 3))
            b[gross] = wild[gross]
            b[:, 0] = 0.0
            traj[v, sl] = root @ Rc.T + tc
            poses[v, sl, :, :3] = b + traj[v, sl][:, None].astype(np.float64)
    if C == 4:
        poses[..., 3] = g.random((V, ftot, J)).astype(np.float32)
    return dict(poses=poses, off=off, traj=traj, traj_ok=np.ones((V, ftot), np.uint8), lag=lag)


def valid_table(V, off, seed, missing=None):
    """gaps in valid: about one frame in five of every view; `missing`: (take, view) pairs absent in all frames of the take"""
    g = np.random.default_rng(seed)
    valid = (g.random((V, int(off[-1]))) > 0.2).astype(np.uint8)
    for t, v in missing or ():
        valid[v, int(off[t]):int(off[t + 1])] = 0
    return valid


@functools.lru_cache(maxsize=None)
def cases():
    """(tag, inputs dict for sync(), want) of the device test: take lengths 1, 255, 256, 257, 600 and 16500 (one chunk of the kernel's sums, two,
    three, and chunks of more than 256 frames), J = 2, 5, 17, V = 1 and V = 4 with a view
    missing from one take, three takes in one call with a single frame among them, gaps in valid, a NaN and an infinite coordinate, C = 4, max_lag 0,
    1, larger than the take, 256 on a 300-frame take, n(d) exactly min_overlap and one below it, sigma = inf"""
    out = []

    def add(tag, sc, **kw):
        inp = dict(poses=sc["poses"], off=sc["off"], **kw)
        out.append((tag, inp, sync(**inp)))

    for n, (F, J, V) in enumerate(((1, 5, 2), (255, 2, 2), (256, 17, 4), (257, 5, 4), (600, 17, 2))):
        add(f"F={F} J={J} V={V}", scene(V, J, [F], seed=200 + n, true_lag=[0, 3, -7.5, 12.25][:V], mirrored=0.25), min_overlap=1 if F == 1 else 16)
    add("V=1: the reference alone", scene(1, 5, [40], seed=210))
    # (a take of more than 16384 frames: the kernel's chunks grow beyond 256 frames there)
    add("F=16500 J=2 V=2, max_lag=2", scene(2, 2, [16500], seed=220, true_lag=[0, 1.25]), max_lag=2)
    sc = scene(4, 17, [1, 257, 40], seed=211, true_lag=[0, 2, -4.5, 6.25], mirrored=0.3, outliers=0.1)
    add("three takes", sc)
    valid = valid_table(4, sc["off"], 212, missing=((1, 0), (2, 2)))
    add("three takes, gaps in valid, view 0 missing in take 1, view 2 in take 2", sc, valid=valid)
    nan = dict(sc, poses=sc["poses"].copy())
    nan["poses"][1, 5, 3, 1] = np.nan
    nan["poses"][0, 200, 0, 2] = np.inf                                 # (the root of a frame of the reference view)
    add("a NaN and an infinite coordinate", nan)
    add("C = 4", scene(4, 17, [1, 257, 40], seed=216, true_lag=[0, 2, -4.5, 6.25], mirrored=0.3, C=4))
    for L in (0, 1):
        add(f"max_lag={L}", sc, max_lag=L)
    add("max_lag larger than the take: every lag ineligible", scene(3, 5, [12], seed=217), max_lag=40, min_overlap=13)
    add("max_lag=256 on a 300-frame take", scene(3, 17, [300], seed=218, true_lag=[0, 40.5, -100]), max_lag=256)
    short = scene(2, 5, [30], seed=219, true_lag=[0, 1.5])
    add("n(d) exactly min_overlap at |d| = 8", short, max_lag=12, min_overlap=22)             # n(d) = 30 - |d|
    add("n(d) one below min_overlap at |d| = 8", short, max_lag=12, min_overlap=23)
    add("sigma=inf", sc, sigma=float("inf"))
    add("sigma=0.01, min_overlap=1", scene(3, 5, [24, 24], seed=215, true_lag=[0, 1, -2.25]), sigma=0.01, min_overlap=1, max_lag=30)
    return out


def ulp32(x):
    """one float32 ulp of |x| (of the smallest normal number below it)"""
    return np.spacing(np.maximum(np.abs(np.asarray(x, np.float64)), np.finfo(np.float32).tiny).astype(np.float32)).astype(np.float64)


def curve_bound(want, dmax):
    """per value of a (.., 2 L + 1) fp64 curve of one take: one float32 ulp of max(|want|, FLOOR dmax^2)"""
    return ulp32(np.maximum(np.abs(np.where(np.isfinite(want), want, 0.0)), FLOOR * dmax * dmax))


# ---- the recovery scene --------------------------------------------------------------------------------------------------------------------
RECOVERY = dict(V=4, J=17, lens=(300,), seed=3, true_lag=(0.0, 3.0, -7.5, 12.25), noise=0.01, mirrored=0.2, outliers=0.1)
RECOVERY_BOUND = 0.5        # frames: what makes the nearest-frame shift the right one


@functools.lru_cache(maxsize=None)
def recovery():
    return scene(**dict(RECOVERY, lens=list(RECOVERY["lens"])))


# ---- constructed rows, compared exactly ------------------------------------------------------------------------------------------------------
def delayed_copy(n=40, delay=5, J=5):
    """Two views (2, n, J, 3) float32: joint j of the reference sits at root + (j + j b(f) / 8, 0, 0), b a triangle of height 6 over the frames
    10 .. 20 and 0 elsewhere, and view 1 is the reference delayed by `delay` frames (its frame f + delay is the reference's frame f; both hold the
    whole triangle).  Every distance is a small dyadic number: the sums, the means and the squared differences are exact in any order, both
    views have the same mean, and the curve at `delay` is exactly 0 (sigma = inf: every other value is exact too; J - 1 = 4 divides exactly)."""
    pad = abs(delay)
    b = np.zeros(n + 2 * pad)
    b[10 + pad:21 + pad] = [1, 2, 3, 4, 5, 6, 5, 4, 3, 2, 1]
    poses = np.zeros((2, n, J, 3), np.float32)
    poses[..., :] = [1.0, 2.0, 3.0]
    for v, shift_by in enumerate((0, delay)):
        for j in range(1, J):
            poses[v, :, j, 0] += j + j * b[pad - shift_by + np.arange(n)] / 8.0
    return poses


def static_pair(n=40):
    """Two views of a body that does not move: distances 5, 13 and 1 in view 0 and 10, 26 and 2 in view 1, exact"""
    poses = np.zeros((2, n, 4, 3), np.float32)
    poses[0, :, 1:] = [[3, 4, 0], [5, 0, 12], [0, 0, 1]]
    poses[1, :, 1:] = [[0, 6, 8], [10, 24, 0], [2, 0, 0]]
    return poses + np.float32(0.5)

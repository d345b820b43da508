"""numpy float64 statement of smoothing lifted sequences in time (manipose_amd/lifting.py: smooth_poses, smooth_traj; mp_lift_smooth), shared by
test_lift_smooth_host.py and test_gpu_lift_smooth.py: the rule of include/manipose_hip.h - a weighted local polynomial fit along the frames of a
sequence, Savitzky-Golay with validity weights - as a plain loop over frames and taps with normal equations, nothing else.  Our own code; the
reference has no counterpart."""
import numpy as np

from lift_place_ref import TOL, within, worst  # noqa: F401  (the lifting bound: |x - x64| <= 2^-23 max(1, |x64|))

TAPER = {"uniform": 0, "biweight": 1}


def taper_weight(tau, R, taper):
    """k(tau): 1 for "uniform", (1 - (tau / (R + 1))^2)^2 for "biweight" (positive on every tap)"""
    if TAPER[taper] == 0:
        return 1.0
    r = float(tau) / float(R + 1)
    q = 1.0 - r * r
    return q * q


def tap_coefficients(taus, R, deg, taper):
    """The valid taps ``taus`` (increasing integers in [-R, R], at least one) of one frame -> (c, d): out = sum_k c[k] y[taus[k]] is p(0) of the
    polynomial p of degree d that minimises sum w (p(u) - y)^2, u = tau / R; d = min(deg, n - 1), and 0 when the frame is not bracketed."""
    taus = [int(t) for t in taus]
    n = len(taus)
    d = min(int(deg), n - 1)
    if not (any(t <= 0 for t in taus) and any(t >= 0 for t in taus)):
        d = 0
    w = np.array([taper_weight(t, R, taper) for t in taus], np.float64)
    u = np.array([float(t) / float(R) for t in taus], np.float64)
    N = np.zeros((d + 1, d + 1))
    for j in range(d + 1):
        for k in range(d + 1):
            acc = 0.0
            for wt, ut in zip(w, u):                    # the normal matrix sum w u^(j + k), taps in increasing order
                acc += wt * ut ** (j + k)
            N[j, k] = acc
    e0 = np.zeros(d + 1)
    e0[0] = 1.0
    a = np.linalg.solve(N, e0)                          # first row of the inverse (N is symmetric)
    c = np.array([wt * sum(a[k] * ut ** k for k in range(d + 1)) for wt, ut in zip(w, u)])
    return c, d


def smooth_all(x, valid=None, seq_offset=None, radius=4, degree=2, taper="uniform", return_degree=False):
    """x (Ntot, inner, M, C) float32 or float64, valid (Ntot, inner) or None (all valid), seq_offset (S + 1) or None (one sequence) ->
    (out float64 of x's shape, filled uint8 (Ntot, inner)[, degree used int (Ntot, inner), -1 where filled = 0]).  A frame without a valid tap
    and channel 3 of C = 4 are the input's values."""
    x = np.asarray(x)
    assert x.ndim == 4 and x.shape[3] in (3, 4)
    ntot, inner = x.shape[:2]
    R = int(radius)
    off = [0, ntot] if seq_offset is None else [int(v) for v in seq_offset]
    ok = np.ones((ntot, inner), bool) if valid is None else np.asarray(valid) != 0
    x64 = x.astype(np.float64)
    out = x64.copy()
    filled = np.zeros((ntot, inner), np.uint8)
    used = np.full((ntot, inner), -1, np.int64)
    for s in range(len(off) - 1):
        f0, f1 = off[s], off[s + 1]
        for g in range(f0, f1):
            for i in range(inner):
                taus = [t for t in range(-R, R + 1) if f0 <= g + t < f1 and ok[g + t, i]]
                if not taus:
                    continue
                c, d = tap_coefficients(taus, R, degree, taper)
                acc = np.zeros(x.shape[2:], np.float64)[..., :3]
                for ck, t in zip(c, taus):              # taps in increasing order
                    acc = acc + ck * x64[g + t, i, :, :3]
                out[g, i, :, :3] = acc
                filled[g, i] = 1
                used[g, i] = d
    return (out, filled, used) if return_degree else (out, filled)


def lstsq_all(x, valid=None, seq_offset=None, radius=4, degree=2, taper="uniform"):
    """The same rule through numpy.linalg.lstsq on the stacked system sqrt(w) [1, u, u^2, ...] a = sqrt(w) y: an independent solve"""
    x = np.asarray(x)
    ntot, inner = x.shape[:2]
    R = int(radius)
    off = [0, ntot] if seq_offset is None else [int(v) for v in seq_offset]
    ok = np.ones((ntot, inner), bool) if valid is None else np.asarray(valid) != 0
    x64 = x.astype(np.float64)
    out = x64.copy()
    for s in range(len(off) - 1):
        f0, f1 = off[s], off[s + 1]
        for g in range(f0, f1):
            for i in range(inner):
                taus = np.array([t for t in range(-R, R + 1) if f0 <= g + t < f1 and ok[g + t, i]])
                if taus.size == 0:
                    continue
                d = min(int(degree), taus.size - 1)
                if not ((taus <= 0).any() and (taus >= 0).any()):
                    d = 0
                r = np.sqrt(np.array([taper_weight(t, R, taper) for t in taus]))
                A = r[:, None] * np.vander(taus / float(R), d + 1, increasing=True)
                Y = r[:, None] * x64[g + taus, i, :, :3].reshape(taus.size, -1)
                out[g, i, :, :3] = np.linalg.lstsq(A, Y, rcond=None)[0][0].reshape(-1, 3)
    return out


LENS = [1, 2, 70, 259]                                  # shorter than any window, a boundary inside a tile, a sequence longer than a tile
OFF = np.concatenate([[0], np.cumsum(LENS)]).astype(np.int64)
NTOT = int(OFF[-1])


def planted_valid(inner, R, deg, seed):
    """(NTOT, inner) uint8 validity of the tests: about 30 % random holes, and planted in EVERY inner index, in the sequences of 70 and 259 frames:
    an isolated hole; a gap at the first frames and one at the last frames of a sequence; a gap of 2R + 3 frames (its 3 middle frames
    have no valid tap: filled = 0), and for R <= 8 (where there is room) a frame whose window holds exactly ``deg`` valid taps."""
    g = np.random.default_rng(seed)
    v = (g.uniform(size=(NTOT, inner)) >= 0.3).astype(np.uint8)
    s2, s3, end = int(OFF[2]), int(OFF[3]), int(OFF[4])
    v[s2 + 30:s2 + 33] = 1                              # isolated hole
    v[s2 + 31] = 0
    v[s2:s2 + 3] = 0                                    # the sequence of 70 starts and ends with a gap
    v[s2 + 3] = 1
    v[s3 - 4:s3] = 0
    v[s3 - 5] = 1
    v[s3:s3 + 2] = 0                                    # so does the sequence of 259
    v[end - 3:end] = 0
    a = s3 + 20                                         # a gap of 2R + 3 frames inside the sequence of 259: its 3 middle frames have no valid tap
    b = min(a + 2 * R + 3, end - 8)
    v[a:b] = 0
    v[a - 1] = v[b] = 1
    # exactly `deg` valid taps around frame c: everything within R of it invalid except `deg` frames (deg = 0: see the long gap's middle)
    c = s3 + 200 if R <= 8 else None
    if c is not None and deg >= 1:
        v[c - R:c + R + 1] = 0
        v[c - 1] = 1
        if deg == 2:
            v[c + R] = 1
    return v


def smooth_inputs(inner, M, C, R, deg, seed):
    """float32 data (NTOT, inner, M, C) - a smooth curve per coordinate plus noise, of size about 1 - and the planted validity"""
    g = np.random.default_rng(seed)
    t = np.arange(NTOT, dtype=np.float64)[:, None, None, None]
    phase = g.uniform(0, 2 * np.pi, (1, inner, M, C))
    x = np.sin(t / 17.0 + phase) + 0.1 * g.standard_normal((NTOT, inner, M, C))
    return x.astype(np.float32), planted_valid(inner, R, deg, seed + 1)


def polynomial_inputs(inner, M, C, deg):
    """integer-valued polynomials of degree <= deg in the frame number of each sequence, exactly representable in float32 (|x| < 2^24)"""
    x = np.zeros((NTOT, inner, M, C), np.float32)
    for s in range(len(LENS)):
        f = (np.arange(LENS[s], dtype=np.float64) - LENS[s] // 2)[:, None, None, None]      # (centred: the values stay below 2^15)
        i = np.arange(inner, dtype=np.float64)[None, :, None, None]
        m = np.arange(M, dtype=np.float64)[None, None, :, None]
        c = np.arange(C, dtype=np.float64)[None, None, None, :]
        p = (3 + i - 2 * m + c) + (deg >= 1) * (5 - c - i) * f + (deg >= 2) * ((m + c) % 3 - 1) * f * f
        assert np.abs(p).max() < 2 ** 24
        x[OFF[s]:OFF[s + 1]] = p
    return x


# every (inner, M, C, R, deg, taper) the float64 test of test_gpu_lift_smooth.py runs (test_lift_smooth_host.py checks the statement on the same inputs); R = 64 with M = 32, C = 4 is among them
GPU_CASES = [(1, 1, 3, 1, 0, "uniform"), (1, 1, 3, 2, 2, "uniform"), (1, 1, 3, 8, 1, "biweight"), (1, 1, 3, 64, 2, "biweight"),
             (1, 17, 3, 2, 1, "biweight"), (1, 17, 3, 8, 2, "uniform"), (1, 17, 3, 64, 0, "uniform"),
             (1, 32, 4, 1, 2, "biweight"), (1, 32, 4, 64, 2, "uniform"),
             (5, 1, 3, 2, 0, "biweight"), (5, 1, 3, 8, 2, "uniform"),
             (5, 17, 3, 1, 1, "uniform"), (5, 17, 3, 8, 2, "biweight"),
             (5, 17, 4, 2, 2, "uniform"), (5, 17, 4, 64, 1, "biweight"),
             (5, 32, 4, 8, 0, "uniform"), (5, 32, 4, 64, 2, "biweight")]


def case_seed(case):
    inner, M, C, R, deg, taper = case
    return 1000 * inner + 10 * M + C + 100000 * R + 7 * deg + (3 if taper == "biweight" else 0)

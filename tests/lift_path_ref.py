"""The float64 statement of mp_lift_path's rule (include/manipose_hip.h) in numpy, what the tests derive from it, and their inputs.

The rule, per sequence with frames [f0, f1) of hyps (Ntot, K, J, 4) float32 (xyz, the score in channel 3):
  U[g][k] = -log(s), s the score of (g, k) read from joint 0; a score that is not > 1e-12 counts as 1e-12;
  D[g][a][b] = (1 / (2 sigma^2)) (sum_j |x[g][b][j] - x[g-1][a][j]|^2 / J) + (a != b ? switch_cost : 0), joint order then channel order, a cost that
  is not finite counts as 1e30;  f[f0] = U[f0];  f[g][b] = min_a (f[g-1][a] + D[g][a][b]) + U[g][b] with the FIRST arg-min as back-pointer; the
  end state is the first arg-min of f[f1-1], the rest follows the back-pointers.  sigma and switch_cost are the float32 values the C ABI carries.

`through` is the forward / backward table: for every (g, k) the cost of the cheapest path forced through state k at frame g.  Its minimum over k is
the optimum at every g.  The MARGIN of an input is the smallest through[g][k] over all k != path[g], minus the optimum: a computation whose costs are
off by less than half of it relative to the statement's must find the same path."""
import itertools

import numpy as np

TINY, HUGE = 1e-12, 1e30


def clamp_offsets(off, ntot):
    """(f0, f1) per sequence as lift_seq_frames clamps a table: entries into 0 .. ntot, an end never before its start"""
    off = [int(v) for v in off]
    out = []
    for s in range(len(off) - 1):
        f0 = min(max(off[s], 0), ntot)
        out.append((f0, min(max(off[s + 1], f0), ntot)))
    return out


def unary(hyps):
    """(N, K) float64"""
    s = hyps[:, :, 0, 3].astype(np.float64)
    with np.errstate(invalid="ignore"):
        s = np.where(s > TINY, s, TINY)
    return -np.log(s)


def transitions(hyps, sigma, switch_cost, reverse_joints=False):
    """(N, K, K) float64: D[g][a][b], row 0 zeros (never read).  The sum runs joint by joint, channel by channel, as the kernel's does."""
    N, K, J, _ = hyps.shape
    sigma, switch_cost = float(np.float32(sigma)), float(np.float32(switch_cost))
    x = hyps[..., :3].astype(np.float64)
    D = np.zeros((N, K, K))
    if N < 2:
        return D
    with np.errstate(invalid="ignore", over="ignore"):
        e = x[1:, None, :, :, :] - x[:-1, :, None, :, :]           # [g - 1][a][b][j][c]
        sq = e * e
        total = np.zeros((N - 1, K, K))
        for j in (range(J - 1, -1, -1) if reverse_joints else range(J)):
            for c in range(3):
                total = total + sq[..., j, c]
        fac = 1.0 / (2.0 * sigma * sigma)
        d = fac * (total / float(J)) + np.where(np.eye(K, dtype=bool), 0.0, switch_cost)
    D[1:] = np.where(np.isfinite(d), d, HUGE)
    return D


def viterbi(U, D):
    """(path (N,) uint8, cost, f (N, K)) of one sequence"""
    N, K = U.shape
    f = np.zeros((N, K))
    bp = np.zeros((N, K), np.int64)
    f[0] = U[0]
    for g in range(1, N):
        c = f[g - 1][:, None] + D[g]                               # [a][b]
        bp[g] = np.argmin(c, axis=0)                               # the first minimum
        f[g] = c[bp[g], np.arange(K)] + U[g]
    path = np.zeros(N, np.uint8)
    k = int(np.argmin(f[N - 1]))
    cost = float(f[N - 1][k])
    for g in range(N - 1, -1, -1):
        path[g] = k
        if g > 0:
            k = int(bp[g][k])
    return path, cost, f


def through(U, D):
    """(N, K): the cost of the cheapest path through (g, k) = forward[g][k] + backward[g][k]"""
    N, K = U.shape
    f = viterbi(U, D)[2]
    b = np.zeros((N, K))
    for g in range(N - 2, -1, -1):
        b[g] = np.min(D[g + 1] + (U[g + 1] + b[g + 1])[None, :], axis=1)
    return f + b


def select_all(hyps, off=None, sigma=0.02, switch_cost=0.0, reverse_joints=False):
    """The statement on (Ntot, K, J, 4) float32 hypotheses: (path (Ntot,) uint8, out (Ntot, J, 3) float32, cost (S,) float64, margin (S,), covered
    (Ntot,) bool); margin[s] is inf where no alternative exists (K = 1 or no frames)."""
    ntot, K = hyps.shape[:2]
    ranges = clamp_offsets(off if off is not None else [0, ntot], ntot)
    U, D = unary(hyps), transitions(hyps, sigma, switch_cost, reverse_joints)
    path = np.zeros(ntot, np.uint8)
    covered = np.zeros(ntot, bool)
    cost, margin = np.zeros(len(ranges)), np.full(len(ranges), np.inf)
    for s, (f0, f1) in enumerate(ranges):
        if f1 <= f0:
            continue
        p, c, _ = viterbi(U[f0:f1], D[f0:f1])
        path[f0:f1], cost[s], covered[f0:f1] = p, c, True
        if K > 1:
            t = through(U[f0:f1], D[f0:f1])
            t[np.arange(f1 - f0), p] = np.inf
            margin[s] = t.min() - c
    out = hyps[np.arange(ntot), path][:, :, :3].copy()
    return path, out, cost, margin, covered


def brute_force(U, D):
    """(path, cost) by enumerating all K^N paths, every path's cost summed in the order of the forward pass; the first minimum in lexicographic
    order is kept (the tests use inputs without ties)."""
    N, K = U.shape
    best, best_p = np.inf, None
    for p in itertools.product(range(K), repeat=N):
        c = U[0][p[0]]
        for g in range(1, N):
            c = (c + D[g][p[g - 1]][p[g]]) + U[g][p[g]]
        if c < best:
            best, best_p = c, p
    return np.asarray(best_p, np.uint8), float(best)


def switches(path, ranges):
    return [int((np.diff(path[f0:f1].astype(np.int64)) != 0).sum()) for f0, f1 in ranges]


def best_score(hyps):
    """the first arg-max of the float32 score per frame: what agg = "best_score" chooses"""
    return np.argmax(hyps[:, :, 0, 3], axis=1).astype(np.uint8)


# ---- inputs --------------------------------------------------------------------------------------------------------------------------------------
def path_inputs(lens, K, J, seed, spread=0.03, noise=0.01, logit_std=1.5):
    """(hyps (sum lens, K, J, 4) float32, off (S + 1) int64): a smooth track per sequence, plus an offset of size `spread` per hypothesis and joint
    that stays put over time, plus noise per frame; scores = softmax over K of logits N(0, logit_std^2), replicated over the joints."""
    g = np.random.default_rng(seed)
    chunks = []
    for n in lens:
        f = np.arange(n, dtype=np.float64)[:, None, None]
        phase = g.uniform(0, 2 * np.pi, (1, J, 3))
        track = 0.3 * np.sin(f / 9.0 + phase) + 0.1 * np.cos(f / 4.0 + 2 * phase)
        x = track[:, None] + spread * g.standard_normal((1, K, J, 3)) + noise * g.standard_normal((n, K, J, 3))
        logits = logit_std * g.standard_normal((n, K))
        p = np.exp(logits - logits.max(axis=1, keepdims=True))
        p = p / p.sum(axis=1, keepdims=True)
        h = np.empty((n, K, J, 4), np.float32)
        h[..., :3] = x
        h[..., 3] = p[:, :, None]
        chunks.append(h)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return np.concatenate(chunks, axis=0), off


# (lens, K, J, sigma, switch_cost, seed): several sequences per call, sequences of 1 and 2 frames among them; K = 1, 2, 5, 8 and the non-powers of two
# 3 and 5; J = 2, 17, 32; switch_cost 0 and > 0.  The last case's high switch cost makes the optimal paths constant.
GPU_CASES = [
    ((130, 1, 2, 61), 5, 17, 0.02, 0.0, 1),
    ((7, 300, 1), 8, 32, 0.02, 0.5, 2),
    ((2, 45, 1, 19), 3, 2, 0.005, 0.0, 3),
    ((33, 2, 70, 1), 2, 17, 0.1, 0.25, 4),
    ((1, 40, 3), 1, 17, 0.02, 0.0, 5),
    ((64, 1, 2, 90), 5, 32, 0.02, 50.0, 6),
]


def case_inputs(case):
    lens, K, J, sigma, switch_cost, seed = case
    return path_inputs(lens, K, J, seed)


def case_id(case):
    lens, K, J, sigma, switch_cost, seed = case
    return f"N{'+'.join(str(n) for n in lens)}-K{K}-J{J}-s{sigma}-w{switch_cost}"

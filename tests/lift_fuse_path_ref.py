"""float64 statement of fusing a take's views along time (manipose_amd/lifting.py: fuse_views_path; mp_lift_fuse_path), shared by
test_lift_fuse_path_host.py and test_gpu_lift_fuse_path.py: the rule of include/manipose_hip.h in plain numpy, nothing else, and the scenes both
files use.  Our own code.  The state vector of a frame is an array of shape (K,) * V, axis v the digit of view v; an operation on such an array is
the same IEEE operation on every state, so the staged recursion below adds and compares exactly what the rule says, in its order.  Rotation,
scenes and camera tables are lift_fuse_ref's."""
import functools
import itertools
import math

import numpy as np

from lift_fuse_ref import TAKES, fuse_scene, rotation, s11_tables, valid_table

BIG = 1e30
CHUNK = 512                                             # MP_LIFT_FUSE_PATH_CHUNK: frames of a backtrack chunk at most (the row prefetch is one frame deep)


def _offsets(take_offset, ftot):
    return [0, ftot] if take_offset is None else [int(v) for v in take_offset]


def frame_tables(x, rots, sigma, score_weight):
    """x (V, K, J, C) one frame's hypotheses, rots per view a matrix or None (invalid: its data is not looked at) -> (w: per view (K, J, 3) or None,
    E (K,) * V: the frame cost of every state, steps 1 to 4 of mp_lift_fuse in its order of additions, subs: pair costs replaced by 1e30)"""
    V, K, J, C = x.shape
    views = [v for v in range(V) if rots[v] is not None]
    w, u, subs = [None] * V, {}, 0
    with np.errstate(all="ignore"):
        for v in views:
            xv = np.asarray(x[v], np.float64)
            w[v] = (xv[:, :, :3] - xv[:, :1, :3]) @ rots[v].T
            u[v] = -np.log(np.where(xv[:, 0, 3] > 1e-12, xv[:, 0, 3], 1e-12)) if C == 4 else np.zeros(K)
        shape = lambda v: tuple(K if a == v else 1 for a in range(V))
        pairs = np.zeros((K,) * V)
        for a, b in itertools.combinations(views, 2):
            s = np.zeros((K, K))
            e = (w[a][:, None] - w[b][None]) ** 2                                 # (K, K, J, 3)
            for j in range(J):                                                    # joint order, then channel order
                for ch in range(3):
                    s = s + e[:, :, j, ch]
            d = s / J
            subs += int((~np.isfinite(d)).sum())
            d = np.where(np.isfinite(d), d, BIG)
            pairs = pairs + d.reshape(tuple(K if ax in (a, b) else 1 for ax in range(V)))      # lexicographic order of (a, b)
        unary = np.zeros((K,) * V)
        for v in views:
            unary = unary + u[v].reshape(shape(v))
        E = (1.0 / (2.0 * float(sigma) * float(sigma))) * pairs + float(score_weight) * unary
    return w, E, subs


def transition(wa, wb, path_sigma, switch_cost, K):
    """t_v[a][b] from hypothesis a of the frame before (wa (K, J, 3)) to hypothesis b of the frame (wb); zeros if either is None (a gap)"""
    if wa is None or wb is None:
        return np.zeros((K, K)), 0
    J = wa.shape[1]
    with np.errstate(all="ignore"):
        e = (wb[None] - wa[:, None]) ** 2                                         # [a][b]
        s = np.zeros((K, K))
        for j in range(J):
            for ch in range(3):
                s = s + e[:, :, j, ch]
        t = (1.0 / (2.0 * float(path_sigma) * float(path_sigma))) * (s / J) + np.where(np.eye(K) == 1, 0.0, float(switch_cost))
    return np.where(np.isfinite(t), t, BIG), int((~np.isfinite(t)).sum())


def take_tables(x, rots, sigma, score_weight, path_sigma, switch_cost):
    """x (V, n, K, J, C) one take, rots[g][v] -> (w[g][v], E[g] (K,) * V, T[g][v] (K, K) for g >= 1 (T[0] is None), substitutions by 1e30)"""
    V, n, K = x.shape[:3]
    w, E, T, subs = [], [], [None], 0
    for g in range(n):
        wg, Eg, s = frame_tables(x[:, g], rots[g], sigma, score_weight)
        w.append(wg); E.append(Eg); subs += s
        if g:
            row = []
            for v in range(V):
                t, s = transition(w[g - 1][v], wg[v], path_sigma, switch_cost, K)
                row.append(t); subs += s
            T.append(row)
    return w, E, T, subs


def _stage(h, t, v, V, back=False):
    """forward: out[.. b ..] = min_a (h[.. a ..] + t[a][b]) over axis v, with the first arg-min; back: out[.. a ..] = min_b (h[.. b ..] + t[a][b])"""
    K = t.shape[0]
    hv = np.moveaxis(h, v, -1)                                                    # (..., a)
    cand = hv[..., :, None] + t if not back else hv[..., None, :] + t             # (..., a, b)
    axis = -2 if not back else -1
    arg = cand.argmin(axis=axis)                                                  # numpy's argmin is the first one
    out = np.take_along_axis(cand, np.expand_dims(arg, axis), axis=axis).squeeze(axis)
    return np.moveaxis(out, -1, v), np.moveaxis(arg, -1, v)


def viterbi(E, T):
    """steps 4 and 5: -> (path (n, V) ints, cost, fwd list of f[g])"""
    V, n = E[0].ndim, len(E)
    f, bps = [E[0]], [None]
    for g in range(1, n):
        h, bp = f[-1], []
        for v in range(V):
            h, arg = _stage(h, T[g][v], v, V)
            bp.append(arg)
        f.append(h + E[g])
        bps.append(bp)
    end = int(f[-1].reshape(-1).argmin())                                         # the first minimum in lexicographic order
    c = list(np.unravel_index(end, E[0].shape))
    cost, path = float(f[-1].reshape(-1)[end]), [None] * n
    for g in range(n - 1, -1, -1):
        path[g] = list(c)
        if g:
            for v in range(V - 1, -1, -1):                                        # the inverse of the staging
                c[v] = int(bps[g][v][tuple(c)])
    return np.array(path, np.int64).reshape(n, V), cost, f


def backward(E, T):
    """bwd[g][c]: the cheapest continuation after state c at frame g (full states, any order of the views: used for the margin only)"""
    V, n = E[0].ndim, len(E)
    bwd = [None] * n
    bwd[n - 1] = np.zeros_like(E[0])
    for g in range(n - 2, -1, -1):
        m = bwd[g + 1] + E[g + 1]
        for v in range(V - 1, -1, -1):
            m, _ = _stage(m, T[g + 1][v], v, V, back=True)
        bwd[g] = m
    return bwd


def exhaustive(E, T):
    """the minimum over ALL paths of sum_g E_g(c_g) + sum_g sum_v t_v (plain left-to-right sums)"""
    V, n, K = E[0].ndim, len(E), E[0].shape[0]
    best = math.inf
    states = list(itertools.product(range(K), repeat=V))
    for p in itertools.product(states, repeat=n):
        s = float(E[0][p[0]])
        for g in range(1, n):
            for v in range(V):
                s += float(T[g][v][p[g - 1][v], p[g][v]])
            s += float(E[g][p[g]])
        best = min(best, s)
    return best


def path_all(hyps, quat=None, valid=None, take_offset=None, sigma=0.02, score_weight=1.0, path_sigma=0.02, switch_cost=0.0):
    """hyps (V, Ftot, K, J, C), quat (G, V, 4) or None, valid (V, Ftot) or None -> dict of pose (Ftot, J, 3), choice (Ftot, V) uint8, cost, spread, ok
    (Ftot), written (Ftot) bool, path_cost (G,), margin (G,): the best path that differs from the chosen one in a valid digit of some frame, minus
    the best (inf without an alternative), subs: table entries that were replaced by 1e30"""
    hyps = np.asarray(hyps)
    V, ftot, K, J, C = hyps.shape
    off = _offsets(take_offset, ftot)
    G = len(off) - 1
    sigma, score_weight, path_sigma, switch_cost = (float(np.float32(v)) for v in (sigma, score_weight, path_sigma, switch_cost))    # the C ABI's floats
    out = dict(pose=np.zeros((ftot, J, 3)), choice=np.zeros((ftot, V), np.uint8), cost=np.zeros(ftot), spread=np.zeros(ftot), ok=np.zeros(ftot, np.uint8),
               written=np.zeros(ftot, bool), path_cost=np.zeros(G), margin=np.full(G, math.inf), subs=0)
    for t in range(G):
        f0 = min(max(off[t], 0), ftot)
        f1 = min(max(off[t + 1], f0), ftot)
        if f1 <= f0:
            continue
        rots = []
        for f in range(f0, f1):
            rots.append([rotation(None if quat is None else quat[t][v]) if (valid is None or valid[v][f]) else None for v in range(V)])
        w, E, T, subs = take_tables(hyps[:, f0:f1], rots, sigma, score_weight, path_sigma, switch_cost)
        path, cost, fwd = viterbi(E, T)
        bwd = backward(E, T)
        out["path_cost"][t], out["subs"] = cost, out["subs"] + subs
        for g in range(f1 - f0):
            f, views = f0 + g, [v for v in range(V) if rots[g][v] is not None]
            out["written"][f] = True
            out["choice"][f] = 255
            if not views:
                continue
            c = tuple(path[g])
            through = fwd[g] + bwd[g]
            same = np.ones((K,) * V, bool)                                        # the states whose VALID digits are the chosen ones
            for v in views:
                same &= (np.arange(K) == c[v]).reshape(tuple(K if a == v else 1 for a in range(V)))
            if (~same).any():
                out["margin"][t] = min(out["margin"][t], float(through[~same].min()) - cost)
            total = np.zeros((J, 3))
            for v in views:
                total = total + w[g][v][c[v]]
            pose = total / len(views)
            dev = 0.0
            for v in views:
                dev += float(((w[g][v][c[v]] - pose) ** 2).sum())
            pose[0] = 0.0
            for v in views:
                out["choice"][f, v] = c[v]
            out["pose"][f], out["cost"][f], out["spread"][f] = pose, float(E[g][c]), math.sqrt(dev / (len(views) * J))
            out["ok"][f] = 0 if E[g][c] >= BIG else 1
    return out


def scratch_bytes(V, ftot, K):
    """mp_lift_fuse_path_scratch_bytes: per frame the row of tables in doubles, a 16-bit word per state, the chosen state; rounded up to 8"""
    R = (V * (V - 1) // 2 + V) * K * K + V * K
    return (ftot * (8 * R + 2 * K ** V + 2) + 7) // 8 * 8


# ---- the scenes -------------------------------------------------------------------------------------------------------------------------------
def mirror_scene(seed=0, frames=60, K=5):
    """The scene the feature is for: S11's four cameras, one take; the true world pose 0.3 N(0, 1) moves 4 mm (RMS) per joint and frame.  Every
    frame and view holds the true pose to 1 mm, its MIRRORED copy (world x negated: consistent in every camera, so the pair cost cannot reject
    it) to 1 mm, and K - 2 distractors moved 0.08 N(0, 1) along the camera's depth axis.  The indices of the true and the mirrored hypothesis are
    drawn per view and re-drawn every 15 frames.  In 24 of the 60 frames (0.4 of them, drawn) the mirrored copy is scored 0.6 and the true pose
    0.2, in the others the other way round; a distractor is scored 0.05.  Returns dict(hyps (4, frames, K, 17, 4) float32, quat (1, 4, 4), off,
    truth (frames, 4) uint8, flipped (frames,) bool: the frames whose scores favour the mirrored copy)."""
    g = np.random.default_rng(seed)
    V, J = 4, 17
    quat = s11_tables(V, 1)[0]
    world = np.zeros((frames, J, 3))
    world[0] = 0.3 * g.standard_normal((J, 3))
    for f in range(1, frames):
        world[f] = world[f - 1] + 0.004 / math.sqrt(3.0) * g.standard_normal((J, 3))
    world -= world[:, :1]
    mirrored = world * np.array([-1.0, 1.0, 1.0])
    flipped = np.zeros(frames, bool)
    flipped[g.permutation(frames)[:round(0.4 * frames)]] = True
    truth = np.zeros((frames, V), np.uint8)
    hyps = np.zeros((V, frames, K, J, 4), np.float32)
    for v in range(V):
        R = rotation(quat[0, v])
        for f in range(frames):
            if f % 15 == 0:
                it, im = (int(i) for i in g.permutation(K)[:2])
            truth[f, v] = it
            for k in range(K):
                if k == it:
                    x, s = world[f] @ R + 0.001 * g.standard_normal((J, 3)), 0.2 if flipped[f] else 0.6
                elif k == im:
                    x, s = mirrored[f] @ R + 0.001 * g.standard_normal((J, 3)), 0.6 if flipped[f] else 0.2
                else:
                    x, s = world[f] @ R + 0.005 * g.standard_normal((J, 3)), 0.05
                    x[:, 2] += 0.08 * g.standard_normal(J)
                hyps[v, f, k, :, :3], hyps[v, f, k, :, 3] = x, s
    return dict(hyps=hyps, quat=quat, off=np.array([0, frames], np.int64), truth=truth, flipped=flipped)


PATH_CASES = [(4, 5, 4), (3, 2, 3), (1, 5, 4), (2, 8, 4)]     # (V, K, C)
SETTINGS = [(0.2, 0.0), (0.5, 1.5)]                           # (path_sigma, switch_cost): fuse_scene draws every frame anew, 0.3 m between frames
LONG = 1100                                                   # frames of the long take: two chunks of 512 and 76 more


@functools.lru_cache(maxsize=None)
def path_cases():
    """Every comparison scene of mp_lift_fuse_path and the statement's answer, computed once: list of (tag, hyps, quat, valid, take_offset, path_sigma,
    switch_cost, want).  Per (V, K, C) on takes of 1, 6 and 37 frames: with and without quaternions, with and without a valid table, at both
    settings (J = 17 with quaternions, J = 5 without: a second joint count); (4, 8, 4), all 4096 states, on one take of 12 frames; (2, 2, 4) on one
    take of LONG frames."""
    cases = []
    for n, (V, K, C) in enumerate(PATH_CASES):
        for with_quat in (True, False):
            for masked in (True, False):
                for m, (ps, sw) in enumerate(SETTINGS):
                    hyps, quat, off = fuse_scene(V, K, C, 17 if with_quat else 5, seed=100 + 10 * n + m, with_quat=with_quat)
                    valid = valid_table(V, off, n) if masked else None
                    cases.append((f"V={V} K={K} C={C} quat={int(with_quat)} valid={int(masked)} path_sigma={ps} switch={sw}", hyps, quat, valid, off, ps, sw))
    hyps, quat, off = fuse_scene(4, 8, 4, 17, lens=[12], seed=199)
    cases.append(("V=4 K=8 C=4 Ftot=12", hyps, quat, None, off, 0.2, 0.0))
    hyps, quat, off = fuse_scene(2, 2, 4, 3, lens=[LONG], seed=198)
    cases.append((f"V=2 K=2 C=4 Ftot={LONG}", hyps, quat, None, off, 0.5, 0.5))
    return [c + (path_all(c[1], c[2], c[3], c[4], path_sigma=c[5], switch_cost=c[6]),) for c in cases]

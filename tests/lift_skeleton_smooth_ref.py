"""mp_lift_fit_skeleton_smooth's rule (include/manipose_hip.h) stated in numpy float64, the seeded scenes its tests share, and their bounds.

Stage A, the per-frame fit, and every piece of a Gauss-Newton step - the subtree sums, the tangent bases, the tree-assembled system, the Cholesky
solve, the candidate - are lift_skeleton_ref's, imported and not restated.  This file adds the stencil of the second differences (S1), the order
of the visits (S2) and the visit (S3).  A visit's evaluation takes a LIST of pulls where lift_skeleton_ref.evaluate has the one towards the
start; with that one pull it gives lift_skeleton_ref.evaluate's bits (test_lift_skeleton_smooth_host.py holds it to that).  The frames a colour
visits are independent, so the statement visits them as one array, every operation elementwise as in lift_skeleton_ref; order="forward" and
order="reverse" visit them one at a time instead, which gives the same bits.  The trace of decisions covers the visits: the smallest Z / |P| of
both evaluations ("deep"), every pivot ("pivot") and F' / F - 1 against the slack ("cost")."""
import copy
import functools
import math

import numpy as np

import lift_fuse_ref as fuse
import lift_skeleton_ref as base

F64 = np.float64
MAXSWEEPS = 64                                          # MP_LIFT_SKELETON_MAXSWEEPS
DEFAULT_SMOOTH, DEFAULT_SWEEPS = 0.1, 8                 # fit_skeleton_views' defaults (untuned: taken from the synthetic motion below)
MARGIN_MIN, COST_SLACK, PIVOT_FLOOR = base.MARGIN_MIN, base.COST_SLACK, base.PIVOT_FLOOR
within_store = base.within_store


# ---- S1: the stencil -------------------------------------------------------------------------------------------------------------------------
def stencil(usable):
    """usable (n) bool over a take's frames -> (a, b, c) bool (n): the terms centred at t-1, t, t+1 exist, and W (n) int = a + 4 b + c"""
    usable = np.asarray(usable, bool)
    u = np.concatenate([[False, False], usable, [False, False]])
    m2, m1, p1, p2 = u[:-4], u[1:-3], u[3:-1], u[4:]
    a, b, c = m2 & m1 & usable, m1 & p1 & usable, p1 & p2 & usable
    return a, b, c, a * 1 + b * 4 + c * 1


def target(P, T, a, b, c):
    """q (len(T), J, 3) of the frames T (take-local indices) from the positions P (n, J, 3):
    ((c1- p(t-1) + c1+ p(t+1)) - (c2- p(t-2) + c2+ p(t+2))) / W in this order; a frame whose coefficient is 0 is not read and counts 0"""
    T = np.asarray(T, np.int64)
    n = P.shape[0]

    def at(k, on):
        return np.where(on[:, None, None], P[np.clip(T + k, 0, n - 1)], 0.0)

    aT, bT, cT = a[T], b[T], c[T]
    cm1, cp1, cm2, cp2 = 2.0 * aT + 2.0 * bT, 2.0 * bT + 2.0 * cT, 1.0 * aT, 1.0 * cT
    W = (aT * 1 + bT * 4 + cT * 1).astype(F64)
    e = lambda v: v[:, None, None]
    with np.errstate(all="ignore"):
        return ((e(cm1) * at(-1, aT | bT) + e(cp1) * at(1, bT | cT)) - (e(cm2) * at(-2, aT) + e(cp2) * at(2, cT))) / e(W)


def prior_terms(P, usable):
    """the smoothness cost without its weight, summed directly over its terms: sum_s sum_j |p_j(s-1) - 2 p_j(s) + p_j(s+1)|^2 over the s whose
    three frames are usable"""
    total = F64(0)
    for s in range(1, P.shape[0] - 1):
        if usable[s - 1] and usable[s] and usable[s + 1]:
            dd = P[s - 1] - 2.0 * P[s] + P[s + 1]
            total += (dd * dd).sum()
    return total


# ---- S3: the evaluation with its pulls, and the visit ------------------------------------------------------------------------------------------
def evaluate(tk, r, d, pulls, jac=True):
    """rule 3 at (r, d) with a list of pulls (weight: a number or (n), target (n, J, 3)), each added as the pull towards the start is: the keys
    of lift_skeleton_ref.evaluate"""
    import lift_bundle_ref as bundle
    n, J = tk.n, tk.J
    p = base.positions(tk, r, d)
    S, g = np.zeros((n, J, 6)), np.zeros((n, J, 3))
    F, E, W = np.zeros(n), np.zeros(n), np.zeros(n)
    deep, minz = np.ones(n, bool), np.full(n, math.inf)
    with np.errstate(all="ignore"):
        for j in range(J):
            Fj, Ej, Wj = np.zeros(n), np.zeros(n), np.zeros(n)
            x, y, z = p[:, j, 0], p[:, j, 1], p[:, j, 2]
            for v in range(tk.V):
                on = tk.obs[v, :, j]
                if not on.any():
                    continue
                R, T = tk.R[v], tk.T[v]
                w = tk.w[v, :, j] if tk.w is not None else np.ones(n)
                wx, wy, wz = x - T[0], y - T[1], z - T[2]
                X = R[0, 0] * wx + R[1, 0] * wy + R[2, 0] * wz
                Y = R[0, 1] * wx + R[1, 1] * wy + R[2, 1] * wz
                Z = R[0, 2] * wx + R[1, 2] * wy + R[2, 2] * wz
                deep &= ~(on & ~(Z > 0.0))
                ratio = np.nan_to_num(Z / np.sqrt(X * X + Y * Y + Z * Z), nan=-math.inf)
                minz = np.where(on, np.minimum(minz, ratio), minz)
                du, dv, (c00, c01, c02, c10, c11, c12) = bundle.project_jac(X, Y, Z, tk.kp[v, :, j, 0], tk.kp[v, :, j, 1], tk.intr[v], tk.distort)
                ee = du * du + dv * dv
                t = 1.0 + ee / tk.sigma2
                Wj = np.where(on, Wj + w, Wj)
                Ej = np.where(on, Ej + w * np.sqrt(ee), Ej)
                Fj = np.where(on, Fj + w * (ee / t), Fj)
                if not jac:
                    continue
                wt = w * (1.0 / (t * t))
                j00, j01, j02 = (c00 * R[0, 0] + c01 * R[0, 1] + c02 * R[0, 2], c00 * R[1, 0] + c01 * R[1, 1] + c02 * R[1, 2],
                                 c00 * R[2, 0] + c01 * R[2, 1] + c02 * R[2, 2])
                j10, j11, j12 = (c10 * R[0, 0] + c11 * R[0, 1] + c12 * R[0, 2], c10 * R[1, 0] + c11 * R[1, 1] + c12 * R[1, 2],
                                 c10 * R[2, 0] + c11 * R[2, 1] + c12 * R[2, 2])
                terms = (wt * (j00 * j00 + j10 * j10), wt * (j00 * j01 + j10 * j11), wt * (j00 * j02 + j10 * j12), wt * (j01 * j01 + j11 * j11),
                         wt * (j01 * j02 + j11 * j12), wt * (j02 * j02 + j12 * j12))
                for k, term in enumerate(terms):
                    S[:, j, k] = np.where(on, S[:, j, k] + term, S[:, j, k])
                for k, term in enumerate((wt * (j00 * du + j10 * dv), wt * (j01 * du + j11 * dv), wt * (j02 * du + j12 * dv))):
                    g[:, j, k] = np.where(on, g[:, j, k] + term, g[:, j, k])
            for lam, q in pulls:
                dx, dy, dz = x - q[:, j, 0], y - q[:, j, 1], z - q[:, j, 2]
                Fj = Fj + lam * ((dx * dx + dy * dy) + dz * dz)
                if jac:
                    S[:, j, 0] += lam; S[:, j, 3] += lam; S[:, j, 5] += lam
                    g[:, j, 0] += lam * dx; g[:, j, 1] += lam * dy; g[:, j, 2] += lam * dz
            F, E, W = F + Fj, E + Ej, W + Wj
    return dict(p=p, F=F, E=E, W=W, deep=deep, minz=minz, S=S, g=g)


def start_pull(tk):
    """the pull towards the start as a list of pulls: rule 3's `iff prior > 0`"""
    return [(tk.prior, tk.start)] if tk.prior > 0.0 else []


def sub_take(tk, rows):
    """the Take of the frames rows of tk"""
    s = copy.copy(tk)
    s.start, s.kp, s.seen, s.obs = tk.start[rows], tk.kp[:, rows], tk.seen[:, rows], tk.obs[:, rows]
    s.w = None if tk.w is None else tk.w[:, rows]
    s.n = len(rows)
    return s


def visit(tk, r, d, lam, q, note=lambda **kw: None):
    """S3 for the frames of tk at once: one step from (r, d) on the frames' cost plus lam |p - q|^2 -> (moved (n) bool, r', d', the candidate's
    evaluation, the largest |delta| of the step in metres (n): the root's move and L_b times the tangent move of every bone)"""
    pulls = start_pull(tk) + [(lam, q)]
    seen = tk.obs.any(axis=(0, 2))
    e = evaluate(tk, r, d, pulls, jac=True)
    note(kind="deep", margin=np.where(seen, np.abs(e["minz"]), math.inf))
    live = e["deep"] & np.isfinite(e["F"])
    delta, passed, worst, e1, e2, _, _ = base.step_system(tk, e, d)
    with np.errstate(all="ignore"):
        note(kind="pivot", margin=np.where(live & np.isfinite(worst), np.abs(worst - PIVOT_FLOOR) / PIVOT_FLOOR, math.inf))
    live &= passed
    r2, d2, finite = base.candidate(tk, r, d, e1, e2, delta)
    live &= finite
    n = evaluate(tk, r2, d2, pulls, jac=False)
    with np.errstate(all="ignore"):
        good = n["deep"] & (n["F"] <= (1.0 + COST_SLACK) * e["F"])
        note(kind="deep", margin=np.where(live & seen, np.abs(n["minz"]), math.inf))
        trivial = (e["F"] == 0) & (n["F"] == 0)
        note(kind="cost", margin=np.where(live & ~trivial, np.abs(n["F"] / e["F"] - 1.0 - COST_SLACK) / COST_SLACK, math.inf))
        size = np.abs(delta).copy()
        size[:, 3:] *= np.repeat(tk.L, 2)[None, :]
    live &= good
    return live, np.where(live[:, None], r2, r), np.where(live[:, None, None], d2, d), n, size.max(axis=1)


class TakeState:
    """one take between the visits: tk the Take of ALL its frames (an unusable frame's rows are never evaluated), frames their global indices,
    usable (n), the stencil, and the fp64 state r (n, 3), d (n, B, 3), p (n, J, 3)"""

    def __init__(self, tk, frames, usable, r, d, p):
        self.tk, self.frames, self.usable, self.r, self.d, self.p = tk, frames, usable, r, d, p
        self.a, self.b, self.c, self.W = stencil(usable)

    def cost(self, smooth):
        """the take's total cost: the usable frames' F, the pull towards the start included, plus smooth times the terms summed directly"""
        rows = np.flatnonzero(self.usable)
        sub = sub_take(self.tk, rows)
        F = evaluate(sub, self.r[rows], self.d[rows], start_pull(sub), jac=False)["F"]
        return math.fsum(F) + F64(np.float32(smooth)) * prior_terms(self.p, self.usable)


def sweep_take(st, smooth, colour, note=lambda **kw: None, order="batch"):
    """S2 for one colour of one take: every usable frame t with t mod 3 = colour and W_t > 0 is visited; returns (the visited rows, moved, the
    candidates' evaluation or None, the steps' sizes)"""
    smooth = F64(np.float32(smooth))
    T = np.array([t for t in range(st.tk.n) if t % 3 == colour and st.usable[t] and st.W[t] > 0], np.int64)
    if T.size == 0:
        return T, np.zeros(0, bool), None, np.zeros(0)
    groups = [T] if order == "batch" else [T[i:i + 1] for i in (range(T.size) if order == "forward" else range(T.size - 1, -1, -1))]
    moved, size, evals = np.zeros(st.tk.n, bool), np.zeros(st.tk.n), {}
    for rows in groups:
        q = target(st.p, rows, st.a, st.b, st.c)
        lam = smooth * st.W[rows].astype(F64)
        mv, r2, d2, n, sz = visit(sub_take(st.tk, rows), st.r[rows], st.d[rows], lam, q, lambda **kw: note(**dict(kw, frames=st.frames[rows])))
        st.r[rows], st.d[rows] = r2, d2
        st.p[rows] = np.where(mv[:, None, None], n["p"], st.p[rows])
        moved[rows], size[rows] = mv, sz
        for i, t in enumerate(rows):
            evals[int(t)] = (n["E"][i], n["W"][i])
    return T, moved[T], evals, size[T]


def fit(start, kp, quat, trans, intr, lengths, parents=None, valid=None, take_offset=None, start_ok=None, kp_weight=None, distort=True,
        sigma=float("inf"), prior=base.DEFAULT_PRIOR, iters=base.DEFAULT_STEPS, smooth=DEFAULT_SMOOTH, sweeps=DEFAULT_SWEEPS, trace=None,
        order="batch", reverse_colour=None, watch=None):
    """The rule on float32 inputs: dict of pose (Ftot, J, 3), err (Ftot, 3) float64, ok, steps, moves (Ftot) uint8, written (Ftot) bool, takes: the
    TakeState of every take that holds a frame, and largest_step: the largest step of any visit in metres.  order: how a colour's frames are
    visited ("batch": as one array; "forward", "reverse": one at a time); reverse_colour: that colour alone is visited in reverse order, one at a
    time; watch(take state, sweep, colour) is called after every colour of every take."""
    import lift_triangulate_ref as tri
    start, kp = np.asarray(start, np.float32), np.asarray(kp, np.float32)
    V, ftot, J = kp.shape[:3]
    parents = base.tree(J) if parents is None else tuple(int(p) for p in parents)
    raw = [0, ftot] if take_offset is None else [int(v) for v in take_offset]
    G = len(raw) - 1
    quat, trans, intr = (np.asarray(a).reshape(G, V, -1) for a in (quat, trans, intr))
    lengths = np.broadcast_to(np.asarray(lengths, np.float32), (G, J - 1))
    out = dict(pose=np.zeros((ftot, J, 3)), err=np.zeros((ftot, 3)), ok=np.zeros(ftot, np.uint8), steps=np.zeros(ftot, np.uint8),
               moves=np.zeros(ftot, np.uint8), written=np.zeros(ftot, bool), takes=[], largest_step=0.0)
    where = [tri.take_of(raw, ftot, f) for f in range(ftot)]
    for g in range(G):
        idx = np.array([f for f in range(ftot) if where[f] == (g, True)], dtype=np.int64)
        if idx.size == 0:
            continue
        out["written"][idx] = True
        with np.errstate(invalid="ignore"):
            L = lengths[g].astype(F64)
            fitted = np.isfinite(start[idx]).all(axis=(1, 2)) & bool(np.isfinite(L).all() and (L > 0).all())
        if start_ok is not None:
            fitted &= np.asarray(start_ok)[idx] != 0
        tk = base.make_take(start[idx], kp[:, idx], quat[g], trans[g], intr[g], lengths[g], parents, None if valid is None else np.asarray(valid)[:, idx],
                            None if kp_weight is None else np.asarray(kp_weight)[:, idx], distort, sigma, prior)
        n = idx.size
        st = TakeState(tk, idx, np.zeros(n, bool), np.full((n, 3), np.nan), np.full((n, J - 1, 3), np.nan), np.full((n, J, 3), np.nan))
        rows = np.flatnonzero(fitted)
        if rows.size:                                                       # stage A: lift_skeleton_ref's fit of the fitted frames
            note = (lambda rows=rows, **kw: trace.append(dict(kw, frames=idx[rows]))) if trace is not None else (lambda **kw: None)
            res = base.fit_take(sub_take(tk, rows), int(iters), note)
            for k in ("pose", "ok", "steps"):
                out[k][idx[rows]] = res[k]
            out["err"][idx[rows], :2] = res["err"]
            out["err"][idx[rows], 2] = res["err"][:, 1]
            have = (res["ok"] & 1) != 0
            st.usable[rows] = have
            st.r[rows[have]], st.d[rows[have]], st.p[rows[have]] = res["r"][have], res["d"][have], res["pose"][have]
            st.a, st.b, st.c, st.W = stencil(st.usable)
        out["takes"].append(st)
    if not (F64(np.float32(smooth)) > 0 and sweeps > 0):
        return out
    note = (lambda **kw: trace.append(kw)) if trace is not None else (lambda **kw: None)
    for sweep in range(int(sweeps)):
        for colour in range(3):
            for st in out["takes"]:
                seen = st.tk.obs.any(axis=(0, 2))
                T, moved, evals, size = sweep_take(st, smooth, colour, note, "reverse" if reverse_colour == colour else order)
                if T.size:
                    out["largest_step"] = max(out["largest_step"], float(size.max()))
                for t, mv in zip(T, moved):
                    if mv:
                        f = st.frames[t]
                        E, W = evals[int(t)]
                        with np.errstate(all="ignore"):
                            out["err"][f, 2] = E / W if seen[t] else 0.0
                        out["moves"][f] += 1
                        out["pose"][f] = st.p[t]
                if watch is not None:
                    watch(st, sweep, colour)
    return out


margin = base.margin


# ---- the scenes --------------------------------------------------------------------------------------------------------------------------------
def motion_scene(V, J, lens, seed, noise=0.002, pose_noise=0.03, parents=None, amp=0.35):
    """A body that MOVES SMOOTHLY: constant bones (lift_skeleton_ref.bone_table, take t's 4 t per cent larger), every bone's direction
    unit(base + amp_i sin(2 pi t / period_i + phase_i)) per coordinate i with |amp_i| <= amp (0.35: the vector before normalising is at least
    1 - 0.35 sqrt(3) = 0.39 long, no direction passes near zero) and periods of 30 to 90 frames, the root walking a circle of 0.5 m in 120 frames
    at 0.9 m; t counts from each take's first frame.  S11's first V cameras, the full camera model, keypoint noise N(0, 1) noise; the START every
    coordinate off by pose_noise N(0, 1).  Returns lift_skeleton_ref.body_scene's dict."""
    g = np.random.default_rng(seed)
    parents = base.tree(J) if parents is None else tuple(parents)
    ftot, G = int(sum(lens)), len(lens)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    quat, trans, intr = fuse.s11_tables(V, G)
    tables = np.stack([base.bone_table(J, seed + t) * np.float32(1.0 + 0.04 * t) for t in range(G)]).astype(np.float32)
    truth, kp = np.zeros((ftot, J, 3)), np.zeros((V, ftot, J, 2), np.float32)
    for t in range(G):
        rest = g.standard_normal((J - 1, 3))
        rest /= np.linalg.norm(rest, axis=-1, keepdims=True)
        amps, period, phase = g.uniform(-amp, amp, (J - 1, 3)), g.uniform(30, 90, (J - 1, 3)), g.uniform(0, 2 * math.pi, (J - 1, 3))
        turn = g.uniform(0, 2 * math.pi)
        for f in range(int(off[t]), int(off[t + 1])):
            s = f - int(off[t])
            dirs = rest + amps * np.sin(2 * math.pi * s / period + phase)
            dirs /= np.linalg.norm(dirs, axis=-1, keepdims=True)
            truth[f, 0] = (0.5 * math.cos(2 * math.pi * s / 120 + turn), 0.5 * math.sin(2 * math.pi * s / 120 + turn), 0.9 + 0.02 * math.sin(2 * math.pi * s / 40))
            for j in range(1, J):
                truth[f, j] = truth[f, parents[j]] + float(tables[t, j - 1]) * dirs[j - 1]
            for v in range(V):
                kp[v, f] = (fuse.project_view(truth[f], np.zeros(3), fuse.rotation(quat[t, v]), trans[t, v], intr[t, v], True)
                            + noise * g.standard_normal((J, 2))).astype(np.float32)
    start = (truth + pose_noise * g.standard_normal(truth.shape)).astype(np.float32)
    return dict(start=start, kp=kp, quat=quat, trans=trans, intr=intr, lengths=tables, off=off, parents=parents, truth=truth)


inputs, errors = base.inputs, base.errors


def second_difference(pose, off=None):
    """the mean over frames and joints of |p(t-1) - 2 p(t) + p(t+1)| in metres per frame^2, inside every take"""
    pose = np.asarray(pose, F64)
    off = [0, pose.shape[0]] if off is None else [int(v) for v in off]
    parts = [np.linalg.norm(pose[a:b - 2] - 2 * pose[a + 1:b - 1] + pose[a + 2:b], axis=-1).ravel() for a, b in zip(off[:-1], off[1:]) if b - a >= 3]
    return float(np.concatenate(parts).mean())


RECOVERY = dict(J=17, lens=(120,), seed=7, noise=0.002)


@functools.lru_cache(maxsize=None)
def recovery(V=4):
    """the committed motion scene: S11's cameras, one take of 120 frames, 17 joints, keypoint noise 0.002, the start 0.03 m N(0, 1) off"""
    return motion_scene(V, RECOVERY["J"], list(RECOVERY["lens"]), RECOVERY["seed"], noise=RECOVERY["noise"])


@functools.lru_cache(maxsize=None)
def recovery_inputs(V=4):
    """the arguments of fit() on the recovery scene: with 2 and 4 views the start is the triangulated joints (lift_triangulate_ref's statement, as a
    fused take hands them on), with 1 view the lifted start and lift_skeleton_ref's one-view pull of 0.01"""
    sc = recovery(V)
    if V == 1:
        return inputs(sc, prior=0.01)
    return inputs(sc, start=base.triangulated_start(sc))


# What the statement reaches on the committed seed with the default weight and sweeps (0.1, 8), measured in fp64 (test_lift_skeleton_smooth_host.py
# prints each figure before it asserts); any bound is TWICE the measured value, the project's convention.  Per number of views: mean joint error in
# metres of (the start, the per-frame fit = stage A, the smoothed fit), and the mean second difference in metres per frame^2 of (the per-frame fit,
# the smoothed fit, the truth).  Asserted outright: smoothed < per-frame, for the error and for the second difference.
MEASURED_4V = ((5.532e-3, 4.171e-3, 2.608e-3), (1.0569e-2, 3.821e-3, 2.067e-3))
MEASURED_2V = ((8.137e-3, 6.127e-3, 3.594e-3), (1.4953e-2, 3.648e-3, 2.067e-3))
# 1 view: STILL CONVERGING after the default sweeps - the keypoints do not fix depth, and the sweeps remove low frequencies slowly: (the start, the
# per-frame fit, after 8 sweeps, after 32 sweeps) and the second differences of (the per-frame fit, 8 sweeps)
MEASURED_1V = ((4.7625e-2, 1.5900e-2, 9.256e-3, 7.595e-3), (3.8634e-2, 4.116e-3))
# The sweeps solve the right problem (test_the_sweeps_reach_a_stationary_point): on STATIONARY's scene after STATIONARY["sweeps"] sweeps the largest
# central-difference derivative of the total cost is this fraction of the largest at stage A's result (the claim: at most 1e-6)
STATIONARY = dict(V=2, J=5, lens=(6,), seed=31, smooth=0.1, sweeps=64)
MEASURED_STATIONARY = 1.85e-9      # (3.63e-2 at stage A's result, 6.73e-11 after 64 sweeps; 32 sweeps leave 1.7e-5, 128 reach the differences' own noise)


# ---- the device test's cases -------------------------------------------------------------------------------------------------------------------
def spoiled(sc, dead, nan):
    """(start, start_ok) of a scene with start_ok = 0 at the frames dead and a NaN start coordinate at the frames nan"""
    start, ok = sc["start"].copy(), np.ones(sc["start"].shape[0], np.uint8)
    ok[list(dead)] = 0
    for f in nan:
        start[f, 1, 2] = np.nan
    return start, ok


@functools.lru_cache(maxsize=None)
def cases():
    """(tag, inputs of fit(), want, trace) of the device test (the smallest margin of a decision met in them and in the device test's other scenes:
    0.92 of its slack, a depth test's): takes of 1, 2, 3, 4, 5, 7 and 65 frames; three takes of 4, 5 and 7 frames in one
    call (colours are take-local); an unusable frame (start_ok 0, and a NaN start) in the middle and at position 1; (V, J) = (4, 17), (2, 17),
    (1, 17), (3, 5) and J = 32 as a chain; four views with one missing; kp_weight with zeros; sweeps 0, 1, 2, 5; smooth 0, 0.1 and 10; prior 0 and
    1e-4; sigma inf and 0.05; pinhole and distorted.  Noisy keypoints: F at the minimum is far above rounding."""
    import lift_triangulate_ref as tri
    out = []

    def add(tag, sc, **kw):
        inp, trace = inputs(sc, **kw), []
        out.append((tag, inp, fit(trace=trace, **inp), trace))

    for k, F in enumerate((1, 2, 3, 4, 5, 7)):
        add(f"F={F} V=4 J=17", motion_scene(4, 17, [F], seed=800 + k), sweeps=2)
    add("F=65 V=2 J=17, sigma 0.05, sweeps 5", motion_scene(2, 17, [65], seed=806), sigma=0.05, sweeps=5)
    add("F=7 V=1 J=17, prior 0.01", motion_scene(1, 17, [7], seed=807), prior=0.01, sweeps=2)
    add("F=7 V=3 J=5", motion_scene(3, 5, [7], seed=808), sweeps=2, sigma=0.05)
    add("F=5 J=32 chain", motion_scene(4, 32, [5], seed=809, parents=base.chain(32)), sweeps=2, iters=2)
    sc = motion_scene(4, 17, [4, 5, 7], seed=810)
    add("three takes", sc)
    for sweeps in (0, 1, 2, 5):
        add(f"three takes, sweeps={sweeps}", sc, sweeps=sweeps, sigma=0.05)
    add("three takes, smooth=0", sc, smooth=0.0)
    add("three takes, smooth=10", sc, smooth=10.0, sweeps=2)
    add("three takes, prior 0, pinhole", sc, prior=0.0, distort=False, sweeps=2)
    add("three takes, iters=0", sc, iters=0, sweeps=2)
    valid = np.ones((4, 16), np.uint8)
    valid[2, 4:9] = 0                                                       # take 1: four views with one missing
    w = tri.weight_table(4, 16, 17, 812)
    start, ok = spoiled(sc, dead=[12], nan=[5])                             # take 2's middle (its frame 3) not ok; take 1's frame 1 a NaN start
    add("three takes, start_ok 0 in the middle, NaN at position 1, view 2 missing in take 1", sc, start=start, start_ok=ok, valid=valid, sweeps=2)
    start, ok = spoiled(sc, dead=[10], nan=[6])                             # take 2's frame 1 not ok; take 1's middle (its frame 2) a NaN start
    add("three takes, start_ok 0 at position 1, NaN in the middle, weights with zeros", sc, start=start, start_ok=ok, kp_weight=w, sweeps=2, sigma=0.05)
    return out

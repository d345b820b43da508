"""mp_lift_calibrate_views' rule (include/manipose_hip.h) stated in numpy float64, the seeded scenes its tests share, and their bounds.

The statement works on the float32 inputs the kernel gets and follows the header step by step: per point plain arithmetic in the rule's order,
written once for all frames of a take (numpy elementwise: every frame sees the operations a scalar loop would give it); a frame's joints are
added in order, a take's frames by numpy.cumsum (a sequential scan).  The rotation, the quaternion test, the projection with its Jacobian, the
camera update, the gauge and the Cholesky solve are lift_bundle_ref's, as the rule says.  The statement also returns what the kernel does not: a
trace of every decision with its distance from the threshold, and the reduced system's 2-norm condition number of every step."""
import functools
import math

import numpy as np

import lift_bundle_ref as bundle
import lift_fuse_ref as fuse

MAXITERS = 8                                            # MP_LIFT_CALIBRATE_MAXITERS
MAXN = 22
DET_FLOOR, COST_SLACK = bundle.DET_FLOOR, bundle.COST_SLACK
STORE_TOL, COST_TOL, MARGIN_MIN = bundle.STORE_TOL, bundle.COST_TOL, bundle.MARGIN_MIN
COND_MAX = 1e8                                          # every compared scene's reduced system, every step: a condition of the device test's bound
SIGMA, PRIOR = 0.05, 1e-3                               # the prototype's values, calibrate_views' defaults
rotation, unit, within_store, margin = bundle.rotation, bundle.unit, bundle.within_store, bundle.margin


class Take:
    """one take's float32 inputs as float64 arrays: start (n, J, 3), kp (V, n, J, 2), used (V, n) bool, w (J), intr (V, 9)"""

    def __init__(self, start, kp, used, w, intr, distort, sigma, prior):
        self.start, self.kp, self.used, self.w, self.intr = start, kp, used, w, intr
        self.distort = bool(distort)
        s = np.float64(np.float32(sigma))
        with np.errstate(over="ignore"):
            self.sigma2 = s * s
        self.prior = float(np.float64(np.float32(prior)))
        self.V, self.n, self.J = kp.shape[0], start.shape[0], start.shape[1]
        self.inside = used.any(axis=0)                      # the frames of the problem


def columns(used_count, fixed_row, focal):
    """2.: (free views in order, fslot per view (-1: none), the view of every column, whether the take iterates)"""
    V = len(used_count)
    free, _ = bundle.gauge(used_count, fixed_row)
    colv = [v for v in free for _ in range(6)]
    fslot = [-1] * V
    if focal:
        for v in range(V):
            if used_count[v] > 0:
                fslot[v] = len(colv)
                colv.append(v)
    return free, fslot, colv, bool(len(colv) > 0 and sum(1 for u in used_count if u > 0) >= 2)


def evaluate(tk, q, T, gf, X, jac=True, free=(), fslot=None, colv=()):
    """3. and 5. at the state (q[v], T[v], gf[v], X (n, J, 3)): dict of Ff (n), F, deep, minz, E (V), W (V) and, with jac, per weighted joint
    yb[j] (n, 3) and Y[j] (3, N, n), the frames' terms Sf (n, N, N) (lower triangle) and sf (n, N), passed (every U), ratio (the smallest
    det / (U00 U11 U22))"""
    n, J, V, N = tk.n, tk.J, tk.V, len(colv)
    fslot = [-1] * V if fslot is None else fslot
    inside = tk.inside
    Fv, Ev, Wv = np.zeros((V, n)), np.zeros((V, n)), np.zeros((V, n))
    Pf = np.zeros(n)
    out = dict(deep=True, minz=math.inf, yb={}, Y={}, Sf=np.zeros((n, N, N)), sf=np.zeros((n, N)), passed=True, ratio=math.inf)
    colv_a = np.asarray(colv, int)
    same = colv_a[:, None] == colv_a[None, :] if N else np.zeros((0, 0), bool)
    with np.errstate(all="ignore"):
        for j in range(J):
            wj = float(tk.w[j])
            if wj == 0.0:
                continue
            x, y, z = X[:, j, 0], X[:, j, 1], X[:, j, 2]
            ex, ey, ez = x - tk.start[:, j, 0], y - tk.start[:, j, 1], z - tk.start[:, j, 2]
            Pf = Pf + wj * ((ex * ex + ey * ey) + ez * ez)
            pw = tk.prior * wj
            H00, H11, H22 = np.full(n, pw), np.full(n, pw), np.full(n, pw)
            H01, H02, H12 = np.zeros(n), np.zeros(n), np.zeros(n)
            g0, g1, g2 = pw * ex, pw * ey, pw * ez
            Wc, J0, J1, ac, wtv = np.zeros((3, N, n)), np.zeros((N, n)), np.zeros((N, n)), np.zeros((N, n)), np.zeros((V, n))
            for v in range(V):
                m = tk.used[v]
                if not m.any():
                    continue
                R = rotation(q[v])
                intr = np.array(tk.intr[v], np.float64)
                cx, cy = float(intr[2]), float(intr[3])
                intr[0], intr[1] = gf[v] * intr[0], gf[v] * intr[1]
                wx, wy, wz = x - T[v][0], y - T[v][1], z - T[v][2]
                Xc = R[0, 0] * wx + R[1, 0] * wy + R[2, 0] * wz
                Yc = R[0, 1] * wx + R[1, 1] * wy + R[2, 1] * wz
                Zc = R[0, 2] * wx + R[1, 2] * wy + R[2, 2] * wz
                if not (Zc[m] > 0.0).all():
                    out["deep"] = False
                out["minz"] = min(out["minz"], float(np.nan_to_num((Zc / np.sqrt(Xc * Xc + Yc * Yc + Zc * Zc))[m], nan=-math.inf).min()))
                ku, kv = tk.kp[v, :, j, 0], tk.kp[v, :, j, 1]
                du, dv, (c00, c01, c02, c10, c11, c12) = bundle.project_jac(Xc, Yc, Zc, ku, kv, intr, tk.distort)
                e = du * du + dv * dv
                t = 1.0 + e / tk.sigma2
                Wv[v] = np.where(m, Wv[v] + wj, Wv[v])
                Ev[v] = np.where(m, Ev[v] + wj * np.sqrt(e), Ev[v])
                Fv[v] = np.where(m, Fv[v] + wj * (e / t), Fv[v])
                if not jac:
                    continue
                wt = wj * (1.0 / (t * t))
                j00, j01, j02 = (c00 * R[0, 0] + c01 * R[0, 1] + c02 * R[0, 2], c00 * R[1, 0] + c01 * R[1, 1] + c02 * R[1, 2],
                                 c00 * R[2, 0] + c01 * R[2, 1] + c02 * R[2, 2])
                j10, j11, j12 = (c10 * R[0, 0] + c11 * R[0, 1] + c12 * R[0, 2], c10 * R[1, 0] + c11 * R[1, 1] + c12 * R[1, 2],
                                 c10 * R[2, 0] + c11 * R[2, 1] + c12 * R[2, 2])
                H00 = np.where(m, H00 + wt * (j00 * j00 + j10 * j10), H00); H01 = np.where(m, H01 + wt * (j00 * j01 + j10 * j11), H01)
                H02 = np.where(m, H02 + wt * (j00 * j02 + j10 * j12), H02); H11 = np.where(m, H11 + wt * (j01 * j01 + j11 * j11), H11)
                H12 = np.where(m, H12 + wt * (j01 * j02 + j11 * j12), H12); H22 = np.where(m, H22 + wt * (j02 * j02 + j12 * j12), H22)
                g0 = np.where(m, g0 + wt * (j00 * du + j10 * dv), g0); g1 = np.where(m, g1 + wt * (j01 * du + j11 * dv), g1)
                g2 = np.where(m, g2 + wt * (j02 * du + j12 * dv), g2)
                wtv[v] = np.where(m, wt, 0.0)
                rows = []
                if v in free:
                    jc0, jc1 = bundle.camera_rows((c00, c01, c02, c10, c11, c12), Xc, Yc, Zc)
                    rows += [(6 * list(free).index(v) + i, jc0[i], jc1[i]) for i in range(6)]
                if fslot[v] >= 0:
                    rows.append((fslot[v], ((du + ku) - cx) / gf[v], ((dv + kv) - cy) / gf[v]))
                for c, a0, a1 in rows:
                    J0[c], J1[c] = np.where(m, a0, 0.0), np.where(m, a1, 0.0)
                    ac[c] = np.where(m, wt * (a0 * du + a1 * dv), 0.0)
                    Wc[0, c] = np.where(m, wt * (j00 * a0 + j10 * a1), 0.0)
                    Wc[1, c] = np.where(m, wt * (j01 * a0 + j11 * a1), 0.0)
                    Wc[2, c] = np.where(m, wt * (j02 * a0 + j12 * a1), 0.0)
            if not jac:
                continue
            c00, c01, c02 = H11 * H22 - H12 * H12, H02 * H12 - H01 * H22, H01 * H12 - H02 * H11
            det, scale = H00 * c00 + H01 * c01 + H02 * c02, H00 * H11 * H22
            good = np.isfinite(det) & np.isfinite(scale) & (det > DET_FLOOR * scale)
            if inside.any():
                out["ratio"] = min(out["ratio"], float(np.nan_to_num((det / scale)[inside], nan=-math.inf).min()))
            if not good[inside].all():
                out["passed"] = False
                continue
            c11, c12, c22 = H00 * H22 - H02 * H02, H01 * H02 - H00 * H12, H00 * H11 - H01 * H01
            i00, i01, i02, i11, i12, i22 = c00 / det, c01 / det, c02 / det, c11 / det, c12 / det, c22 / det
            y0, y1, y2 = (i00 * g0 + i01 * g1) + i02 * g2, (i01 * g0 + i11 * g1) + i12 * g2, (i02 * g0 + i12 * g1) + i22 * g2
            Q = np.stack([(i00 * Wc[0] + i01 * Wc[1]) + i02 * Wc[2], (i01 * Wc[0] + i11 * Wc[1]) + i12 * Wc[2],
                          (i02 * Wc[0] + i12 * Wc[1]) + i22 * Wc[2]])                          # U^-1 W: (3, N, n)
            out["yb"][j], out["Y"][j] = np.stack([y0, y1, y2], axis=1), Q
            sterm = ac - ((Wc[0] * y0 + Wc[1] * y1) + Wc[2] * y2)                               # (N, n)
            prod = (Wc[0][:, None] * Q[0][None] + Wc[1][:, None] * Q[1][None]) + Wc[2][:, None] * Q[2][None]      # (N, N, n): rows r, columns c
            blk = np.where(same[:, :, None], wtv[colv_a][:, None] * (J0[:, None] * J0[None] + J1[:, None] * J1[None]), 0.0) if N else prod
            keep = inside[:, None]
            out["sf"] = out["sf"] + np.where(keep, sterm.T, 0.0)
            out["Sf"] = out["Sf"] + np.where(keep[:, :, None], np.transpose(blk - prod, (2, 0, 1)), 0.0)
        Ff = np.zeros(n)
        for v in range(V):
            Ff = np.where(tk.used[v], Ff + Fv[v], Ff)
        Ff = np.where(inside, Ff + tk.prior * Pf, 0.0)
        out["Ff"] = Ff
        out["F"] = float(np.cumsum(Ff)[-1]) if n else 0.0
        out["E"] = np.array([float(np.cumsum(np.where(tk.used[v], Ev[v], 0.0))[-1]) if n else 0.0 for v in range(V)])
        out["W"] = np.array([float(np.cumsum(np.where(tk.used[v], Wv[v], 0.0))[-1]) if n else 0.0 for v in range(V)])
    return out


def reduced(e):
    """(S (N, N) symmetric, s (N)) of an evaluation: the frames' terms in increasing order"""
    Sf, sf = e["Sf"], e["sf"]
    with np.errstate(all="ignore"):
        S = np.cumsum(Sf, axis=0)[-1] if len(Sf) else np.zeros(Sf.shape[1:])
        s = np.cumsum(sf, axis=0)[-1] if len(sf) else np.zeros(sf.shape[1:])
    return np.tril(S) + np.tril(S, -1).T, s


def move_points(tk, X, e, dc):
    """dX = -(U^-1 b + sum_c (U^-1 W)_c dc_c), columns in order, of every weighted joint of the frames of the problem"""
    Xn = X.copy()
    with np.errstate(all="ignore"):
        for j, yb in e["yb"].items():
            d = yb.copy()
            Y = e["Y"][j]
            for c in range(len(dc)):
                d[:, 0] += Y[0, c] * dc[c]; d[:, 1] += Y[1, c] * dc[c]; d[:, 2] += Y[2, c] * dc[c]
            Xn[:, j] = np.where(tk.inside[:, None], X[:, j] - d, X[:, j])
    return Xn


def calibrate_take(tk, quat32, trans32, fixed_row, focal, iters, trace=None):
    """one take: dict of quat (V, 4), trans (V, 3), intr (V, 9), points (n, J, 3), reproj (V, 2), cost (2), steps, ok, used (V)"""
    V = tk.V
    used = tk.used.sum(axis=1).astype(np.int32)
    q = [unit(quat32[v]) if unit(quat32[v]) is not None else np.array([1.0, 0, 0, 0]) for v in range(V)]
    T = [np.asarray(trans32[v], np.float64) for v in range(V)]
    gf = [1.0] * V
    X = tk.start.copy()
    free, fslot, colv, iterates = columns(used, fixed_row, focal)
    N = len(colv)
    out = dict(quat=np.asarray(quat32, np.float64).copy(), trans=np.asarray(trans32, np.float64).copy(), intr=tk.intr.copy(), points=tk.start.copy(),
               used=used, steps=0, ok=0)
    note = (lambda **kw: trace.append(kw)) if trace is not None else (lambda **kw: None)

    def errs(e):
        with np.errstate(all="ignore"):
            return np.array([float(np.float64(e["E"][v]) / np.float64(e["W"][v])) if used[v] > 0 else 0.0 for v in range(V)])

    kw = dict(free=tuple(free), fslot=fslot, colv=tuple(colv))
    e = evaluate(tk, q, T, gf, X, jac=iters > 0 and iterates, **kw)
    out["reproj"], out["cost"] = np.stack([errs(e), errs(e)], axis=1), np.array([e["F"], e["F"]])
    note(kind="deep", taken=e["deep"], margin=abs(e["minz"]))
    if not (e["deep"] and math.isfinite(e["F"])):
        return out
    out["ok"] = 1
    steps = 0
    for p in range(int(iters)):
        if not iterates:
            break
        note(kind="det", taken=e["passed"], margin=abs(e["ratio"] - DET_FLOOR) / DET_FLOOR)
        if not e["passed"]:
            break
        S, s = reduced(e)
        dc, pivot = bundle.cholesky_solve(S, s)
        note(kind="pivot", taken=dc is not None, margin=abs(pivot - bundle.PIVOT_FLOOR) / bundle.PIVOT_FLOOR, cond=float(np.linalg.cond(S)))
        if dc is None:
            break
        qn, Tn, gn = list(q), list(T), list(gf)
        for k, v in enumerate(free):
            qn[v], Tn[v] = bundle.move_camera(q[v], T[v], dc[6 * k:6 * k + 6])
        for v in range(V):
            if fslot[v] >= 0:
                gn[v] = gf[v] + float(dc[fslot[v]])
        fine = all(np.isfinite(qn[v]).all() and np.isfinite(Tn[v]).all() for v in free) and all(math.isfinite(a) and a > 0.0 for a in gn)
        note(kind="focal", taken=fine, margin=abs(min(gn)))
        if not fine:
            break
        Xn = move_points(tk, X, e, dc)
        e2 = evaluate(tk, qn, Tn, gn, Xn, jac=p + 1 < iters, **kw)
        good = bool(e2["deep"] and e2["F"] <= (1.0 + COST_SLACK) * e["F"])
        note(kind="deep", taken=e2["deep"], margin=abs(e2["minz"]))
        with np.errstate(all="ignore"):
            note(kind="cost", taken=good, margin=abs(e2["F"] / e["F"] - 1.0 - COST_SLACK) / COST_SLACK, F=e2["F"], step=float(np.abs(dc).max()))
        if not good:
            break
        q, T, gf, X, e, steps = qn, Tn, gn, Xn, e2, steps + 1
    out["steps"] = steps
    out["reproj"][:, 1], out["cost"][1] = errs(e), e["F"]
    if steps > 0:
        for v in free:
            out["quat"][v], out["trans"][v] = q[v], T[v]
        for v in range(V):
            if fslot[v] >= 0:
                out["intr"][v, 0], out["intr"][v, 1] = gf[v] * tk.intr[v, 0], gf[v] * tk.intr[v, 1]
        out["points"] = X
    out["N"] = N
    return out


def make_take(start, kp, quat, valid, start_ok, weights, intr, distort, sigma, prior, sl):
    """1. of the rule on the frames sl of a take: its Take"""
    V, J = kp.shape[0], start.shape[1]
    p, k = start[sl].astype(np.float64), kp[:, sl].astype(np.float64)
    w = np.ones(J) if weights is None else np.asarray(weights, np.float64)
    frame = np.isfinite(p).all(axis=(1, 2))
    if start_ok is not None:
        frame &= np.asarray(start_ok)[sl] != 0
    used = np.zeros((V, p.shape[0]), bool)
    for v in range(V):
        if unit(quat[v]) is None:
            continue
        used[v] = frame & np.isfinite(k[v][:, w != 0]).all(axis=(1, 2))
        if valid is not None:
            used[v] &= np.asarray(valid)[v, sl] != 0
    return Take(p, k, used, w, np.asarray(intr, np.float64), distort, sigma, prior)


def calibrate(start, kp, quat, trans, intr, valid=None, take_offset=None, start_ok=None, fixed=None, weights=None, distort=True, focal=True,
              sigma=SIGMA, prior=PRIOR, iters=3, trace=None):
    """The rule on float32 inputs: dict of quat (G, V, 4), trans (G, V, 3), intr (G, V, 9), points (Ftot, J, 3), reproj (G, V, 2), cost (G, 2)
    float64, steps, ok (G) uint8, used (G, V) int32.  What is copied through holds the float32 inputs' values."""
    start, kp = np.asarray(start), np.asarray(kp)
    V, ftot = kp.shape[:2]
    off = bundle.offsets(take_offset, ftot)
    G = len(off) - 1
    quat, trans, intr = (np.asarray(a).reshape(G, V, -1) for a in (quat, trans, intr))
    out = dict(quat=quat.astype(np.float64), trans=trans.astype(np.float64), intr=intr.astype(np.float64), points=start.astype(np.float64),
               reproj=np.zeros((G, V, 2)), cost=np.zeros((G, 2)), steps=np.zeros(G, np.uint8), ok=np.zeros(G, np.uint8), used=np.zeros((G, V), np.int32))
    for g in range(G):
        sl = slice(int(off[g]), int(max(off[g], off[g + 1])))
        tk = make_take(start, kp, quat[g], valid, start_ok, weights, intr[g], distort, sigma, prior, sl)
        res = calibrate_take(tk, quat[g], trans[g], None if fixed is None else np.asarray(fixed).reshape(G, V)[g], focal, iters, trace)
        for k in ("quat", "trans", "intr", "reproj", "cost", "steps", "ok", "used"):
            out[k][g] = res[k]
        out["points"][sl] = res["points"]
    return out


def worst_cond(trace):
    c = [d["cond"] for d in trace if "cond" in d]
    return max(c) if c else 0.0


# ---- a full dense solve of the same normal equations: an independent route to one step ----------------------------------------------------
def jacobian(tk, q, T, gf, X, free, fslot):
    """(r, Jm, layout) of the weighted residual vector sqrt(w_j omega) res and sqrt(prior w_j) (X - start) and its dense Jacobian over
    (camera columns, focal columns, points of the frames of the problem x weighted joints), omega held at its value"""
    colv = [v for v in free for _ in range(6)] + [v for v in range(tk.V) if fslot[v] >= 0]
    N = len(colv)
    frames = np.nonzero(tk.inside)[0]
    joints = [j for j in range(tk.J) if tk.w[j] != 0]
    M = 3 * len(frames) * len(joints)
    rows_r, rows_J, seen = [], [], []
    for a, f in enumerate(frames):
        for b, j in enumerate(joints):
            po = N + 3 * (a * len(joints) + b)
            for v in range(tk.V):
                if not tk.used[v, f]:
                    continue
                R = rotation(q[v])
                intr = np.array(tk.intr[v], np.float64)
                cx, cy = intr[2], intr[3]
                intr[0], intr[1] = gf[v] * intr[0], gf[v] * intr[1]
                P = R.T @ (X[f, j] - T[v])
                du, dv, c = bundle.project_jac(np.array([P[0]]), np.array([P[1]]), np.array([P[2]]), tk.kp[v, f, j, 0], tk.kp[v, f, j, 1], intr, tk.distort)
                du, dv, c = float(du[0]), float(dv[0]), [float(np.asarray(a_).reshape(-1)[0]) for a_ in c]
                e = du * du + dv * dv
                t = 1.0 + e / tk.sigma2
                sw = math.sqrt(tk.w[j] * (1.0 / (t * t)))
                Jpi = np.array([c[:3], c[3:]])
                row = np.zeros((2, N + M))
                row[:, po:po + 3] = Jpi @ R.T
                if v in free:
                    k = list(free).index(v)
                    Px = np.array([[0, -P[2], P[1]], [P[2], 0, -P[0]], [-P[1], P[0], 0]])
                    row[:, 6 * k:6 * k + 3] = -Jpi @ Px
                    row[:, 6 * k + 3:6 * k + 6] = Jpi
                if fslot[v] >= 0:
                    row[:, fslot[v]] = [((du + tk.kp[v, f, j, 0]) - cx) / gf[v], ((dv + tk.kp[v, f, j, 1]) - cy) / gf[v]]
                rows_r += [sw * du, sw * dv]
                rows_J += [sw * row[0], sw * row[1]]
                seen += [True, True]
            sp = math.sqrt(tk.prior * tk.w[j])
            for c3 in range(3):
                row = np.zeros(N + M)
                row[po + c3] = sp
                rows_r.append(sp * (X[f, j, c3] - tk.start[f, j, c3]))
                rows_J.append(row)
                seen.append(False)
    return np.array(rows_r), np.array(rows_J), (N, frames, joints, np.array(seen))


def dense_step(tk, q, T, gf, X, free, fslot):
    """(dc (N), dX (n, J, 3)) of one Gauss-Newton step by a dense solve of the full normal equations"""
    r, Jm, (N, frames, joints, _) = jacobian(tk, q, T, gf, X, free, fslot)
    d = -np.linalg.solve(Jm.T @ Jm, Jm.T @ r)
    dX = np.zeros_like(X)
    for a, f in enumerate(frames):
        for b, j in enumerate(joints):
            po = N + 3 * (a * len(joints) + b)
            dX[f, j] = d[po:po + 3]
    return d[:N], dX


def schur_step(tk, q, T, gf, X, free, fslot, colv):
    """(dc, dX) of the statement's own step"""
    e = evaluate(tk, q, T, gf, X, True, tuple(free), fslot, tuple(colv))
    S, s = reduced(e)
    dc, _ = bundle.cholesky_solve(S, s)
    return dc, move_points(tk, X, e, dc) - X


def residuals(tk, q, T, gf, X):
    """every used observation's (du, dv), frames x weighted joints x used views in a fixed order: what the Jacobians are differenced on"""
    out = []
    for f in np.nonzero(tk.inside)[0]:
        for j in range(tk.J):
            if tk.w[j] == 0:
                continue
            for v in range(tk.V):
                if not tk.used[v, f]:
                    continue
                intr = np.array(tk.intr[v], np.float64)
                intr[0], intr[1] = gf[v] * intr[0], gf[v] * intr[1]
                P = rotation(q[v]).T @ (X[f, j] - T[v])
                du, dv, _ = bundle.project_jac(np.array([P[0]]), np.array([P[1]]), np.array([P[2]]), tk.kp[v, f, j, 0], tk.kp[v, f, j, 1], intr, tk.distort)
                out += [float(du[0]), float(dv[0])]
    return np.array(out)


# ---- the scenes ------------------------------------------------------------------------------------------------------------------------------
FOCAL_OFF = (1.10, 0.90, 1.07, 0.92)                    # the start's focal lengths over the truth's, per view: +-10 %


def scene(V, J, lens, seed, noise=0.002, focal_off=FOCAL_OFF, rad=0.02, metres=0.05, joint_noise=0.03, frame_noise=0.03):
    """A body in smooth motion seen by S11's first V cameras.  Truth: per take a body of J offsets 0.25 N(0, 1) about a root that walks a
    Lissajous path (x, y within +-0.8 m, z in 0.85 .. 0.95 m), every joint swinging by 0.1 m with a period and phase of its own; keypoints = the
    full camera model plus noise N(0, 1).  Start: every view's fx, fy times focal_off[v]; the cameras of views 1.. rotated by rad N(0, 1) per
    component (an axis-angle) and moved by metres N(0, 1) per component (view 0 keeps its extrinsics); the points off by joint_noise N(0, 1) per
    joint (constant in time) plus frame_noise N(0, 1) per frame (all joints alike): 68 mm on average with the defaults.  Returns a dict: the
    float32 inputs start, kp, quat, trans, intr, off and the truth true_points, true_intr, true_quat, true_trans."""
    g = np.random.default_rng(seed)
    ftot, G = int(sum(lens)), len(lens)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    quat, trans, intr = fuse.s11_tables(V, G)
    truth = np.zeros((ftot, J, 3))
    for t in range(G):
        n = int(lens[t])
        s = np.arange(n)[:, None] / 50.0
        body = 0.25 * g.standard_normal((J, 3))
        ph, om = g.uniform(0, 2 * np.pi, (J, 3)), g.uniform(2.0, 6.0, (J, 3))
        root = np.concatenate([0.8 * np.sin(1.3 * s + g.uniform(0, 6)), 0.8 * np.cos(0.9 * s + g.uniform(0, 6)), 0.9 + 0.05 * np.sin(2.1 * s)], axis=1)
        truth[off[t]:off[t + 1]] = root[:, None] + body[None] + 0.1 * np.sin(om[None] * s[:, :, None] + ph[None])
    kp = np.zeros((V, ftot, J, 2), np.float32)
    for t in range(G):
        for v in range(V):
            R = rotation(unit(quat[t, v]))
            for f in range(int(off[t]), int(off[t + 1])):
                kp[v, f] = (fuse.project_view(truth[f], np.zeros(3), R, trans[t, v], intr[t, v], True) + noise * g.standard_normal((J, 2))).astype(np.float32)
    q0, t0, k0 = quat.astype(np.float64), trans.astype(np.float64), intr.astype(np.float64)
    for t in range(G):
        for v in range(V):
            k0[t, v, :2] = k0[t, v, :2] * focal_off[v]
            if v == 0:
                continue
            w = rad * g.standard_normal(3)
            th = np.linalg.norm(w)
            dq = np.concatenate([[np.cos(th / 2)], np.sin(th / 2) * w / th]) if th > 0 else np.array([1.0, 0, 0, 0])
            q0[t, v] = bundle.canonical(bundle.qmul(unit(quat[t, v]), dq))
            t0[t, v] = t0[t, v] + metres * g.standard_normal(3)
    start = truth + joint_noise * np.concatenate([np.broadcast_to(g.standard_normal((1, J, 3)), (int(lens[t]), J, 3)) for t in range(G)]) \
        + frame_noise * g.standard_normal((ftot, 1, 3))
    return dict(start=start.astype(np.float32), kp=kp, quat=q0.astype(np.float32), trans=t0.astype(np.float32), intr=k0.astype(np.float32), off=off,
                true_points=truth, true_intr=intr.astype(np.float64), true_quat=np.stack([[unit(q) for q in row] for row in quat]),
                true_trans=trans.astype(np.float64))


def inputs(sc, **kw):
    """the arguments of calibrate() of a scene"""
    return dict(dict(start=sc["start"], kp=sc["kp"], quat=sc["quat"], trans=sc["trans"], intr=sc["intr"], take_offset=sc["off"]), **kw)


def focal_errors(intr, sc, g=0):
    """per view of take g: |fx / fx_true - 1|"""
    return np.abs(np.asarray(intr, np.float64)[g][:, 0] / sc["true_intr"][g][:, 0] - 1.0)


def point_error(points, sc):
    """the mean distance of the points from the truth, metres"""
    return float(np.linalg.norm(np.asarray(points, np.float64) - sc["true_points"], axis=-1).mean())


RECOVERY = dict(V=4, J=17, lens=(200,), seed=11)        # the issue's scene: 200 frames, 17 joints, four views


@functools.lru_cache(maxsize=None)
def recovery(V=4):
    return scene(V, RECOVERY["J"], list(RECOVERY["lens"]), RECOVERY["seed"])


WEIGHTS = fuse.WEIGHTS


def gap_tables(V, off, seed):
    """(valid (V, Ftot), start_ok (Ftot)) uint8 with about one entry in six cleared"""
    return bundle.gap_tables(V, off, seed)


@functools.lru_cache(maxsize=None)
def cases():
    """(tag, inputs of calibrate(), want, trace) of the device test: takes of 1, 5, 65 and 257 frames, (V, J) = (4, 17), (3, 5), (2, 17), four
    views with one missing, three takes in one call, gaps in valid and start_ok, fixed given and null, weights with zeros, focal 0 and 1, distort
    0 and 1, sigma inf and finite, iters 0, 1, 3 and 8, a fixed-only take with the focal factors free, a take of one view (evaluated only)."""
    out = []

    def add(tag, sc, **kw):
        inp, trace = inputs(sc, **kw), []
        out.append((tag, inp, calibrate(trace=trace, **inp), trace))

    # (five frames of five joints under three cameras leave the reduced system at 2e9: the short takes have 17 joints, the five joints 65 frames)
    for F, V, J, seed in ((1, 4, 17, 400), (5, 2, 17, 402), (65, 3, 5, 404), (257, 4, 17, 406)):
        add(f"F={F} V={V} J={J}", scene(V, J, [F], seed=seed))
    sc = scene(4, 17, [1, 70, 40], seed=410)
    add("three takes", sc)
    for iters in (0, 1, 8):
        add(f"three takes, iters={iters}", sc, iters=iters)
    add("three takes, sigma=inf, pinhole", sc, distort=False, sigma=float("inf"))
    add("three takes, focal held", sc, focal=False)
    valid, start_ok = gap_tables(4, sc["off"], 411)
    valid[2, int(sc["off"][1]):int(sc["off"][2])] = 0                    # take 1: four views with one missing
    add("three takes, gaps in valid and start_ok, view 2 missing in take 1", sc, valid=valid, start_ok=start_ok)
    fixed = np.array([[1, 0, 0, 0], [1, 1, 0, 0], [1, 1, 1, 1]], np.uint8)
    add("three takes, fixed given (take 2: every view fixed, focal free), weights with zeros", sc, fixed=fixed, weights=WEIGHTS)
    add("every view fixed, focal held: evaluated only", sc, fixed=np.ones((3, 4), np.uint8), focal=False)
    one = np.zeros((4, int(sc["off"][-1])), np.uint8)
    one[1] = 1
    add("one view: evaluated only", sc, valid=one)
    return out

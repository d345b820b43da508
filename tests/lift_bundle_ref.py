"""mp_lift_bundle_views' rule (include/manipose_hip.h) stated in numpy float64, the seeded scenes its tests share, and their bounds.

The statement works on the float32 inputs the kernel gets and follows the header step by step.  Per joint it is plain arithmetic in the rule's
order, written once for all frames of a view (numpy elementwise: every frame sees the operations a scalar loop would give it); the sums run over
the views in order, then the joints in order, and a take's sums over the frames in increasing order (numpy.cumsum: a sequential scan).  The
projection and its Jacobian are lift_refine_ref.evaluate's arithmetic restated for arrays - test_lift_bundle_host.py holds the two against each
other.  The statement also returns what the kernel does not: a trace of every decision with its distance from the threshold."""
import functools
import math

import numpy as np

import lift_align_ref as align
import lift_fuse_ref as fuse

MAXITERS = 8                                            # MP_LIFT_BUNDLE_MAXITERS
DET_FLOOR, PIVOT_FLOOR, COST_SLACK, SMALL = 1e-12, 1e-12, 1e-6, 1e-16
STORE_TOL = 2.0 ** -23                                  # the project's bound for a float32 store, times max(1, |x|)
COST_TOL = 1e-9
MARGIN_MIN = 1e-3                                       # every decision of a scene the device is compared on is at least this far from its threshold


def rotation(q):
    """the matrix of a unit quaternion (w, x, y, z), the kernels' expression"""
    w, x, y, z = (float(c) for c in q)
    return np.array([[1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - w * z), 2.0 * (x * z + w * y)],
                     [2.0 * (x * y + w * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - w * x)],
                     [2.0 * (x * z - w * y), 2.0 * (y * z + w * x), 1.0 - 2.0 * (x * x + y * y)]])


def unit(q32):
    """q / |q| in float64 of float32 values, None where |q|^2 is not finite or < 1e-12"""
    w, x, y, z = (float(c) for c in np.asarray(q32, np.float64))
    with np.errstate(all="ignore"):
        n2 = float(np.float64(w) * w + np.float64(x) * x + np.float64(y) * y + np.float64(z) * z)
    if not (math.isfinite(n2) and n2 >= 1e-12):
        return None
    n = math.sqrt(n2)
    return np.array([w / n, x / n, y / n, z / n])


def canonical(q):
    """mp_lift_align_views' sign rule: w >= 0, and if w == 0 the first non-zero component is positive; a zero comes out as +0"""
    return align.canonical(q)


def project_jac(X, Y, Z, ku, kv, intr, distort):
    """step 2 of mp_lift_place_refine at camera-space points (arrays): (du, dv, (c00, c01, c02, c10, c11, c12)), the residual and J_pi"""
    fx, fy, cx, cy, k1, k2, k3, p1, p2 = (float(v) for v in np.asarray(intr, np.float64))
    with np.errstate(all="ignore"):
        qx, qy = X / Z, Y / Z
        xx = np.where(qx < -1.0, -1.0, np.where(qx > 1.0, 1.0, qx))
        yy = np.where(qy < -1.0, -1.0, np.where(qy > 1.0, 1.0, qy))
        px, py, a, b, c, d = xx, yy, 1.0, 0.0, 0.0, 1.0
        if distort:
            r2 = xx * xx + yy * yy
            m = 1.0 + (k1 * r2 + k2 * (r2 * r2) + k3 * (r2 * r2 * r2)) + (p1 * xx + p2 * yy)
            px, py = xx * m + p1 * r2, yy * m + p2 * r2
            dm = k1 + 2.0 * k2 * r2 + 3.0 * k3 * (r2 * r2)
            mx, my = 2.0 * xx * dm + p1, 2.0 * yy * dm + p2
            a, b = m + xx * mx + 2.0 * p1 * xx, xx * my + 2.0 * p1 * yy
            c, d = yy * mx + 2.0 * p2 * xx, m + yy * my + 2.0 * p2 * yy
        du, dv = fx * px + cx - ku, fy * py + cy - kv
        sx = np.where((qx >= -1.0) & (qx <= 1.0), 1.0, 0.0)
        sy = np.where((qy >= -1.0) & (qy <= 1.0), 1.0, 0.0)
        iz = 1.0 / Z
        xz, yz, xq, yq = sx * iz, sy * iz, sx * (-qx / Z), sy * (-qy / Z)
        jac = (fx * (a * xz), fx * (b * yz), fx * (a * xq + b * yq), fy * (c * xz), fy * (d * yz), fy * (c * xq + d * yq))
    return du, dv, jac


def camera_rows(jac, X, Y, Z):
    """the two rows of J_c = J_pi [-[P]x | I], the Jacobian with respect to a camera's (omega, tau), P' = exp([omega]x) P + tau"""
    c00, c01, c02, c10, c11, c12 = jac
    return ((c02 * Y - c01 * Z, c00 * Z - c02 * X, c01 * X - c00 * Y, c00, c01, c02),
            (c12 * Y - c11 * Z, c10 * Z - c12 * X, c11 * X - c10 * Y, c10, c11, c12))


class Take:
    """one take's float32 inputs as float64 arrays: pose (n, J, 3), root (n, 3), kp (V, n, J, 2), used (V, n) bool, w (J), intr (V, 9)"""

    def __init__(self, pose, root, kp, used, w, intr, distort, sigma):
        self.pose, self.root, self.kp, self.used, self.w, self.intr = pose, root, kp, used, w, intr
        self.distort = bool(distort)
        s = np.float64(np.float32(sigma))
        with np.errstate(over="ignore"):
            self.sigma2 = s * s
        self.V, self.n, self.J = kp.shape[0], pose.shape[0], pose.shape[1]
        self.inside = used.any(axis=0)                      # the frames of the problem


def tri(i, j):
    return i * (i + 1) // 2 + j


def evaluate(tk, q, T, r, jac=True, slots=()):
    """3. and the sums of 5. at the state (q[v], T[v], r (n, 3)): dict of F_f (n), F, deep, minz, E (V), W (V) and, with jac, U (n, 6), b (n, 3) and
    per slot Wm (n, 3, 6), Am (n, 21), am (n, 6).  slots: the free views in order."""
    n, J, V = tk.n, tk.J, tk.V
    out = dict(Ff=np.zeros(n), E=np.zeros(V), W=np.zeros(V), deep=True, minz=math.inf, U=np.zeros((n, 6)), b=np.zeros((n, 3)),
               Wm=[np.zeros((n, 3, 6)) for _ in slots], Am=[np.zeros((n, 21)) for _ in slots], am=[np.zeros((n, 6)) for _ in slots])
    Ef, Wf = np.zeros((V, n)), np.zeros((V, n))
    with np.errstate(all="ignore"):
        for v in range(V):
            idx = np.nonzero(tk.used[v])[0]
            if idx.size == 0:
                continue
            R = rotation(q[v])
            ox, oy, oz = r[idx, 0] - T[v][0], r[idx, 1] - T[v][1], r[idx, 2] - T[v][2]
            slot = slots.index(v) if (jac and v in slots) else -1
            for j in range(J):
                wj = float(tk.w[j])
                if wj == 0.0:
                    continue
                wx, wy, wz = tk.pose[idx, j, 0] + ox, tk.pose[idx, j, 1] + oy, tk.pose[idx, j, 2] + oz
                X = R[0, 0] * wx + R[1, 0] * wy + R[2, 0] * wz
                Y = R[0, 1] * wx + R[1, 1] * wy + R[2, 1] * wz
                Z = R[0, 2] * wx + R[1, 2] * wy + R[2, 2] * wz
                if not (Z > 0.0).all():
                    out["deep"] = False
                out["minz"] = min(out["minz"], float(np.nan_to_num(Z / np.sqrt(X * X + Y * Y + Z * Z), nan=-math.inf).min()))
                du, dv, (c00, c01, c02, c10, c11, c12) = project_jac(X, Y, Z, tk.kp[v, idx, j, 0], tk.kp[v, idx, j, 1], tk.intr[v], tk.distort)
                e = du * du + dv * dv
                t = 1.0 + e / tk.sigma2
                Wf[v, idx] += wj
                Ef[v, idx] += wj * np.sqrt(e)
                out["Ff"][idx] += wj * (e / t)
                if not jac:
                    continue
                wt = wj * (1.0 / (t * t))
                j00, j01, j02 = (c00 * R[0, 0] + c01 * R[0, 1] + c02 * R[0, 2], c00 * R[1, 0] + c01 * R[1, 1] + c02 * R[1, 2],
                                 c00 * R[2, 0] + c01 * R[2, 1] + c02 * R[2, 2])
                j10, j11, j12 = (c10 * R[0, 0] + c11 * R[0, 1] + c12 * R[0, 2], c10 * R[1, 0] + c11 * R[1, 1] + c12 * R[1, 2],
                                 c10 * R[2, 0] + c11 * R[2, 1] + c12 * R[2, 2])
                U, b = out["U"], out["b"]
                U[idx, 0] += wt * (j00 * j00 + j10 * j10); U[idx, 1] += wt * (j00 * j01 + j10 * j11); U[idx, 2] += wt * (j00 * j02 + j10 * j12)
                U[idx, 3] += wt * (j01 * j01 + j11 * j11); U[idx, 4] += wt * (j01 * j02 + j11 * j12); U[idx, 5] += wt * (j02 * j02 + j12 * j12)
                b[idx, 0] += wt * (j00 * du + j10 * dv); b[idx, 1] += wt * (j01 * du + j11 * dv); b[idx, 2] += wt * (j02 * du + j12 * dv)
                if slot < 0:
                    continue
                jc0, jc1 = camera_rows((c00, c01, c02, c10, c11, c12), X, Y, Z)
                jr0, jr1 = (j00, j01, j02), (j10, j11, j12)
                for i in range(6):
                    for l in range(i + 1):
                        out["Am"][slot][idx, tri(i, l)] += wt * (jc0[i] * jc0[l] + jc1[i] * jc1[l])
                    out["am"][slot][idx, i] += wt * (jc0[i] * du + jc1[i] * dv)
                    for c in range(3):
                        out["Wm"][slot][idx, c, i] += wt * (jr0[c] * jc0[i] + jr1[c] * jc1[i])
        out["F"] = float(np.cumsum(out["Ff"])[-1]) if n else 0.0
        for v in range(V):
            out["E"][v], out["W"][v] = (float(np.cumsum(Ef[v])[-1]), float(np.cumsum(Wf[v])[-1])) if n else (0.0, 0.0)
    return out


def reduced(tk, e, slots):
    """5.: (S (N, N) lower triangle filled symmetric, s (N), Uinv (n, 6), yb (n, 3), Y per slot (n, 3, 6), the smallest det / (U00 U11 U22) over
    the frames of the problem, whether every U passed)"""
    n, N = tk.n, 6 * len(slots)
    U, b = e["U"], e["b"]
    with np.errstate(all="ignore"):
        U00, U01, U02, U11, U12, U22 = (U[:, k] for k in range(6))
        c00, c01, c02 = U11 * U22 - U12 * U12, U02 * U12 - U01 * U22, U01 * U12 - U02 * U11
        det, scale = U00 * c00 + U01 * c01 + U02 * c02, U00 * U11 * U22
        good = np.isfinite(det) & np.isfinite(scale) & (det > DET_FLOOR * scale)
        inside = tk.inside
        ratio = float((det[inside] / scale[inside]).min()) if inside.any() else math.inf
        if not good[inside].all():
            return None, None, None, None, None, ratio, False
        c11, c12, c22 = U00 * U22 - U02 * U02, U01 * U02 - U00 * U12, U00 * U11 - U01 * U01
        i00, i01, i02, i11, i12, i22 = c00 / det, c01 / det, c02 / det, c11 / det, c12 / det, c22 / det
        for a in (i00, i01, i02, i11, i12, i22):
            a[~inside] = 0.0
        yb = np.stack([(i00 * b[:, 0] + i01 * b[:, 1]) + i02 * b[:, 2], (i01 * b[:, 0] + i11 * b[:, 1]) + i12 * b[:, 2],
                       (i02 * b[:, 0] + i12 * b[:, 1]) + i22 * b[:, 2]], axis=1)
        Ys = []
        Sf, sf = np.zeros((n, N, N)), np.zeros((n, N))
        for k in range(len(slots)):
            Wk = e["Wm"][k]
            Y = np.zeros((n, 3, 6))
            for i in range(6):
                w0, w1, w2 = Wk[:, 0, i], Wk[:, 1, i], Wk[:, 2, i]
                Y[:, 0, i] = (i00 * w0 + i01 * w1) + i02 * w2
                Y[:, 1, i] = (i01 * w0 + i11 * w1) + i12 * w2
                Y[:, 2, i] = (i02 * w0 + i12 * w1) + i22 * w2
                sf[:, 6 * k + i] = e["am"][k][:, i] - ((w0 * yb[:, 0] + w1 * yb[:, 1]) + w2 * yb[:, 2])
            Ys.append(Y)
        for k in range(len(slots)):
            Wk = e["Wm"][k]
            for l in range(k + 1):
                Yl = Ys[l]
                for i in range(6):
                    for c in range(6):
                        prod = (Wk[:, 0, i] * Yl[:, 0, c] + Wk[:, 1, i] * Yl[:, 1, c]) + Wk[:, 2, i] * Yl[:, 2, c]
                        if k != l:
                            Sf[:, 6 * k + i, 6 * l + c] = 0.0 - prod
                        elif c <= i:
                            Sf[:, 6 * k + i, 6 * k + c] = e["Am"][k][:, tri(i, c)] - prod
        S = np.cumsum(Sf, axis=0)[-1] if n else np.zeros((N, N))
        s = np.cumsum(sf, axis=0)[-1] if n else np.zeros(N)
    S = np.tril(S) + np.tril(S, -1).T
    return S, s, (i00, i01, i02, i11, i12, i22), yb, Ys, ratio, True


def cholesky_solve(S, s):
    """-S^-1 s through S = L L^T row by row; (dc or None, the smallest pivot / S_ii met)"""
    N = len(s)
    L, worst = np.zeros((N, N)), math.inf
    with np.errstate(all="ignore"):
        for i in range(N):
            for j in range(i + 1):
                a = float(S[i, j])
                for k in range(j):
                    a -= L[i, k] * L[j, k]
                if i == j:
                    worst = min(worst, a / float(S[i, i]) if S[i, i] != 0 else -math.inf)
                    if not (math.isfinite(a) and a > PIVOT_FLOOR * float(S[i, i])):
                        return None, worst
                    L[i, i] = math.sqrt(a)
                else:
                    L[i, j] = a / L[j, j]
        x = np.zeros(N)
        for i in range(N):
            a = float(s[i])
            for k in range(i):
                a -= L[i, k] * x[k]
            x[i] = a / L[i, i]
        for i in range(N - 1, -1, -1):
            a = float(x[i])
            for k in range(i + 1, N):
                a -= L[k, i] * x[k]
            x[i] = a / L[i, i]
    x = 0.0 - x
    return (x if np.isfinite(x).all() else None), worst


def move_camera(q, T, d):
    """4.: the camera (q unit, T) moved by d = (omega, tau): q * conj(q_w) normalised and canonical, T - R(q') tau"""
    wx, wy, wz = (float(c) for c in d[:3])
    th2 = (wx * wx + wy * wy) + wz * wz
    bw, bs = 1.0, 0.5
    if th2 > SMALL:
        th = math.sqrt(th2)
        bw, bs = math.cos(0.5 * th), math.sin(0.5 * th) / th
    bx, by, bz = 0.0 - bs * wx, 0.0 - bs * wy, 0.0 - bs * wz
    aw, ax, ay, az = (float(c) for c in q)
    p = np.array([((aw * bw - ax * bx) - ay * by) - az * bz, ((aw * bx + ax * bw) + ay * bz) - az * by,
                  ((aw * by - ax * bz) + ay * bw) + az * bx, ((aw * bz + ax * by) - ay * bx) + az * bw])
    p = canonical(p / math.sqrt((p[0] * p[0] + p[1] * p[1]) + (p[2] * p[2] + p[3] * p[3])))
    R = rotation(p)
    tx, ty, tz = (float(c) for c in d[3:6])
    Tn = np.array([T[0] - ((R[0, 0] * tx + R[0, 1] * ty) + R[0, 2] * tz), T[1] - ((R[1, 0] * tx + R[1, 1] * ty) + R[1, 2] * tz),
                   T[2] - ((R[2, 0] * tx + R[2, 1] * ty) + R[2, 2] * tz)])
    return p, Tn


def move_roots(r, yb, Ys, dc):
    """dr_f = -(U^-1 b + sum_k (U^-1 W_k) dc_k), slots in order, columns in order"""
    d = yb.copy()
    with np.errstate(all="ignore"):
        for k, Y in enumerate(Ys):
            for c in range(6):
                d[:, 0] += Y[:, 0, c] * dc[6 * k + c]; d[:, 1] += Y[:, 1, c] * dc[6 * k + c]; d[:, 2] += Y[:, 2, c] * dc[6 * k + c]
        return r - d


def gauge(used_count, fixed_row):
    """2.: (the free views in order, whether the take moves)"""
    V = len(used_count)
    lowest = next((v for v in range(V) if used_count[v] > 0), -1)
    fix = [(fixed_row[v] != 0) if fixed_row is not None else v == lowest for v in range(V)]
    anchored = any(fix[v] and used_count[v] > 0 for v in range(V))
    free = [v for v in range(V) if not fix[v] and used_count[v] > 0]
    return (free, True) if anchored and free else ([], False)


def bundle_take(tk, quat32, trans32, fixed_row, iters, trace=None):
    """one take: dict of quat (V, 4), trans (V, 3), root (n, 3), reproj (V, 2), cost (2), steps, ok, used (V)"""
    V = tk.V
    used = tk.used.sum(axis=1).astype(np.int32)
    q = [unit(quat32[v]) if unit(quat32[v]) is not None else np.array([1.0, 0, 0, 0]) for v in range(V)]
    T = [np.asarray(trans32[v], np.float64) for v in range(V)]
    r = tk.root.copy()
    free, moves = gauge(used, fixed_row)
    out = dict(quat=np.asarray(quat32, np.float64).copy(), trans=np.asarray(trans32, np.float64).copy(), root=tk.root.copy(), used=used, steps=0, ok=0)
    note = (lambda **kw: trace.append(kw)) if trace is not None else (lambda **kw: None)

    def errs(e):
        with np.errstate(all="ignore"):
            return np.array([float(np.float64(e["E"][v]) / np.float64(e["W"][v])) if used[v] > 0 else 0.0 for v in range(V)])

    e = evaluate(tk, q, T, r, jac=iters > 0, slots=free)
    out["reproj"], out["cost"] = np.stack([errs(e), errs(e)], axis=1), np.array([e["F"], e["F"]])
    note(kind="deep", taken=e["deep"], margin=abs(e["minz"]))
    if not (e["deep"] and math.isfinite(e["F"])):
        return out
    out["ok"] = 1
    steps = 0
    for p in range(int(iters)):
        if not moves:
            break
        S, s, _, yb, Ys, ratio, passed = reduced(tk, e, free)
        note(kind="det", taken=passed, margin=abs(ratio - DET_FLOOR) / DET_FLOOR)
        if not passed:
            break
        dc, pivot = cholesky_solve(S, s)
        note(kind="pivot", taken=dc is not None, margin=abs(pivot - PIVOT_FLOOR) / PIVOT_FLOOR, cond=float(np.linalg.cond(S)))
        if dc is None:
            break
        qn, Tn = list(q), list(T)
        for k, v in enumerate(free):
            qn[v], Tn[v] = move_camera(q[v], T[v], dc[6 * k:6 * k + 6])
        if not all(np.isfinite(qn[v]).all() and np.isfinite(Tn[v]).all() for v in free):
            break
        rn = move_roots(r, yb, Ys, dc)
        e2 = evaluate(tk, qn, Tn, rn, jac=p + 1 < iters, slots=free)
        good = bool(e2["deep"] and e2["F"] <= (1.0 + COST_SLACK) * e["F"])
        note(kind="deep", taken=e2["deep"], margin=abs(e2["minz"]))
        with np.errstate(all="ignore"):
            note(kind="cost", taken=good, margin=abs(e2["F"] / e["F"] - 1.0 - COST_SLACK) / COST_SLACK, F=e2["F"], step=float(np.abs(dc).max()))
        if not good:
            break
        q, T, r, e, steps = qn, Tn, rn, e2, steps + 1
    out["steps"] = steps
    out["reproj"][:, 1], out["cost"][1] = errs(e), e["F"]
    if steps > 0:
        for v in free:
            out["quat"][v], out["trans"][v] = q[v], T[v]
        out["root"][tk.inside] = r[tk.inside]
    return out


def offsets(take_offset, ftot):
    return np.array([0, ftot], np.int64) if take_offset is None else np.clip(np.asarray(take_offset, np.int64), 0, ftot)


def make_take(pose, root, kp, quat, valid, root_ok, weights, intr, distort, sigma, sl):
    """1. of the rule on the frames sl of a take: its Take"""
    V, J = kp.shape[0], pose.shape[1]
    p, r, k = pose[sl].astype(np.float64), root[sl].astype(np.float64), kp[:, sl].astype(np.float64)
    w = np.ones(J) if weights is None else np.asarray(weights, np.float64)
    frame = np.isfinite(p).all(axis=(1, 2)) & np.isfinite(r).all(axis=1)
    if root_ok is not None:
        frame &= np.asarray(root_ok)[sl] != 0
    used = np.zeros((V, p.shape[0]), bool)
    for v in range(V):
        if unit(quat[v]) is None:
            continue
        used[v] = frame & np.isfinite(k[v][:, w != 0]).all(axis=(1, 2))
        if valid is not None:
            used[v] &= np.asarray(valid)[v, sl] != 0
    return Take(p, r, k, used, w, np.asarray(intr, np.float64), distort, sigma)


def bundle(pose, root, kp, quat, trans, intr, valid=None, take_offset=None, root_ok=None, fixed=None, weights=None, distort=True,
           sigma=float("inf"), iters=3, trace=None):
    """The rule on float32 inputs: dict of quat (G, V, 4), trans (G, V, 3), root (Ftot, 3), reproj (G, V, 2), cost (G, 2) float64, steps, ok (G)
    uint8, used (G, V) int32.  What is copied through holds the float32 inputs' values."""
    pose, root, kp = np.asarray(pose), np.asarray(root), np.asarray(kp)
    V, ftot = kp.shape[:2]
    off = offsets(take_offset, ftot)
    G = len(off) - 1
    quat, trans, intr = (np.asarray(a).reshape(G, V, -1) for a in (quat, trans, intr))
    out = dict(quat=quat.astype(np.float64), trans=trans.astype(np.float64), root=root.astype(np.float64), reproj=np.zeros((G, V, 2)),
               cost=np.zeros((G, 2)), steps=np.zeros(G, np.uint8), ok=np.zeros(G, np.uint8), used=np.zeros((G, V), np.int32))
    for g in range(G):
        sl = slice(int(off[g]), int(max(off[g], off[g + 1])))
        tk = make_take(pose, root, kp, quat[g], valid, root_ok, weights, intr[g], distort, sigma, sl)
        res = bundle_take(tk, quat[g], trans[g], None if fixed is None else np.asarray(fixed).reshape(G, V)[g], iters, trace)
        out["quat"][g], out["trans"][g], out["root"][sl] = res["quat"], res["trans"], res["root"]
        out["reproj"][g], out["cost"][g], out["steps"][g], out["ok"][g], out["used"][g] = res["reproj"], res["cost"], res["steps"], res["ok"], res["used"]
    return out


def margin(trace):
    """the smallest distance of a decision from its threshold, in units of the threshold's slack: det / (U00 U11 U22) and pivot / S_ii from 1e-12 in
    units of 1e-12, F' / F - 1 from 1e-6 in units of 1e-6, a weighted joint's Z / |P| from 0"""
    m = [d["margin"] for d in trace]
    return min(m) if m else math.inf


def within_store(got, want):
    """every stored float within 2^-23 max(1, |x|) of the statement (a NaN where the statement has none is not within); returns (all within, the
    worst ratio to the bound)"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    with np.errstate(invalid="ignore"):
        ratio = np.where(got == want, 0.0, np.abs(got - want) / (STORE_TOL * np.maximum(1.0, np.abs(want))))      # (an infinite value copied through)
    worst = float(np.nan_to_num(ratio, nan=np.inf).max()) if ratio.size else 0.0
    return worst <= 1.0, worst


# ---- a full dense solve of the same normal equations: an independent route to one step ----------------------------------------------------
def dense_step(tk, q, T, r, free):
    """(dc (6 n), dr (n, 3)) of one Gauss-Newton step by a dense solve of the full system over (cameras, roots of the frames of the problem)"""
    e = evaluate(tk, q, T, r, True, free)
    frames = np.nonzero(tk.inside)[0]
    N, M = 6 * len(free), 3 * len(frames)
    H, g = np.zeros((N + M, N + M)), np.zeros(N + M)
    for k in range(len(free)):
        for i in range(6):
            for l in range(i + 1):
                H[6 * k + i, 6 * k + l] = H[6 * k + l, 6 * k + i] = e["Am"][k][:, tri(i, l)].sum()
        g[6 * k:6 * k + 6] = e["am"][k].sum(axis=0)
    for a, f in enumerate(frames):
        U = e["U"][f]
        H[N + 3 * a:N + 3 * a + 3, N + 3 * a:N + 3 * a + 3] = [[U[0], U[1], U[2]], [U[1], U[3], U[4]], [U[2], U[4], U[5]]]
        g[N + 3 * a:N + 3 * a + 3] = e["b"][f]
        for k in range(len(free)):
            H[N + 3 * a:N + 3 * a + 3, 6 * k:6 * k + 6] = e["Wm"][k][f]
            H[6 * k:6 * k + 6, N + 3 * a:N + 3 * a + 3] = e["Wm"][k][f].T
    d = -np.linalg.solve(H, g)
    dr = np.zeros((tk.n, 3))
    dr[frames] = d[N:].reshape(-1, 3)
    return d[:N], dr


def schur_step(tk, q, T, r, free):
    """(dc, dr) of the statement's own step"""
    e = evaluate(tk, q, T, r, True, free)
    S, s, _, yb, Ys, _, passed = reduced(tk, e, free)
    dc, _ = cholesky_solve(S, s)
    return dc, move_roots(r, yb, Ys, dc) - r


def cost_at(tk, q, T, r):
    return evaluate(tk, q, T, r, jac=False)["F"]


# ---- the alternation the joint step is held against: per-view resection on the fused points <-> the root fit ---------------------------------
def alternate(tk, quat32, trans32, free, rounds=8, inner=3):
    """`rounds` times: every free camera refined alone on the current world points (`inner` Gauss-Newton steps on its 6 parameters), then every
    root refined alone under the new cameras (`inner` steps on its 3).  Returns (q, T, r)."""
    q = [unit(quat32[v]) for v in range(tk.V)]
    T = [np.asarray(trans32[v], np.float64) for v in range(tk.V)]
    r = tk.root.copy()
    for _ in range(rounds):
        for _ in range(inner):
            e = evaluate(tk, q, T, r, True, free)
            for k, v in enumerate(free):
                A = np.zeros((6, 6))
                for i in range(6):
                    for l in range(i + 1):
                        A[i, l] = A[l, i] = e["Am"][k][:, tri(i, l)].sum()
                q[v], T[v] = move_camera(q[v], T[v], -np.linalg.solve(A, e["am"][k].sum(axis=0)))
        for _ in range(inner):
            e = evaluate(tk, q, T, r, True, ())
            for f in np.nonzero(tk.inside)[0]:
                U = e["U"][f]
                r[f] = r[f] - np.linalg.solve(np.array([[U[0], U[1], U[2]], [U[1], U[3], U[4]], [U[2], U[4], U[5]]]), e["b"][f])
    return q, T, r


# ---- the scenes ------------------------------------------------------------------------------------------------------------------------------
def small_rotation(g, deg):
    """a unit quaternion of a rotation by deg about a random axis"""
    axis = g.standard_normal(3)
    axis /= np.linalg.norm(axis)
    h = 0.5 * np.radians(deg)
    return np.concatenate([[np.cos(h)], np.sin(h) * axis])


def qmul(a, b):
    return np.array([a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3], a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                     a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1], a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0]])


def scene(V, J, lens, seed, noise=0.002, deg=0.3, metres=0.15, root_noise=0.05, pose_noise=0.0):
    """lift_fuse_ref.place_scene (poses 0.3 N(0, 1), roots x, y in +-1 m and z in 0.8 .. 1.0 m, keypoints = the full camera model of S11's first V
    cameras plus noise N(0, 1)) with a start that is off: the cameras of views 1.. rotated by `deg` about a random axis and moved by `metres` in a
    random direction (view 0 keeps the truth), the roots by root_noise N(0, 1), the pose by pose_noise N(0, 1).  Returns a dict: the float32
    inputs pose, root, kp, quat, trans, intr, off and the truth true_quat, true_trans, true_root."""
    pose, kp, root, (quat, trans, intr), off = fuse.place_scene(V, J, lens, seed, noise)
    g = np.random.default_rng(seed + 1000)
    G = len(lens)
    q0, t0 = quat.astype(np.float64), trans.astype(np.float64)
    for t in range(G):
        for v in range(1, V):
            d = g.standard_normal(3)
            q0[t, v] = canonical(qmul(unit(quat[t, v]), small_rotation(g, deg)))
            t0[t, v] = t0[t, v] + metres * d / np.linalg.norm(d)
    start = root + root_noise * g.standard_normal(root.shape)
    if pose_noise:
        pose = (pose + pose_noise * g.standard_normal(pose.shape)).astype(np.float32)
        pose[:, 0] = 0
    return dict(pose=pose, root=start.astype(np.float32), kp=kp, quat=q0.astype(np.float32), trans=t0.astype(np.float32), intr=intr, off=off,
                true_quat=np.stack([[unit(q) for q in row] for row in quat]), true_trans=trans.astype(np.float64), true_root=root)


def inputs(sc, **kw):
    """the arguments of bundle() of a scene"""
    return dict(dict(pose=sc["pose"], root=sc["root"], kp=sc["kp"], quat=sc["quat"], trans=sc["trans"], intr=sc["intr"], take_offset=sc["off"]), **kw)


def camera_errors(quat, trans, sc, g=0):
    """per view of take g: (degrees, metres) between cameras and the scene's truth"""
    V = sc["true_quat"].shape[1]
    deg = [align.angle_deg(unit(quat[g][v]), sc["true_quat"][g, v]) for v in range(V)]
    return np.array(deg), np.linalg.norm(np.asarray(trans, np.float64)[g] - sc["true_trans"][g], axis=1)


RECOVERY = dict(V=4, J=17, lens=(60,), seed=7)          # S11's four cameras, 60 frames, start 0.3 degrees / 0.15 m off


# What the statement reaches on the noise-free scene in RECOVERY_STEPS steps, measured in fp64 (degrees, metres of a camera, metres of a root):
# 1.18e-7, 1.47e-8, 1.58e-8 - the float32 rounding of the keypoints, nothing else; the bounds are twice that.  A float32 STORE of the result adds
# its own half ulp: 2^-24 per quaternion component (an angle of at most 4 x 2^-24 rad), 2^-22 per component of a |T| < 8 m, 2^-24 of a |root| < 2 m.
RECOVERY_STEPS = 3
RECOVERY_DEG, RECOVERY_M, RECOVERY_ROOT = 2.4e-7, 3.0e-8, 3.2e-8
STORE_DEG, STORE_M, STORE_ROOT = float(np.degrees(4 * 2.0 ** -24)), float(np.sqrt(3.0) * 2.0 ** -22), 2.0 ** -24


@functools.lru_cache(maxsize=None)
def recovery(noise=0.0):
    return scene(RECOVERY["V"], RECOVERY["J"], list(RECOVERY["lens"]), RECOVERY["seed"], noise=noise)


def refused_scene():
    """one frame seen by two cameras, the second 40 degrees and 1 m off, the root 0.3 m N(0, 1): the first undamped step lowers the cost (248 to
    64), the second would raise it and is not taken"""
    return scene(2, 17, [1], seed=310, deg=40.0, metres=1.0, root_noise=0.3)


WEIGHTS = fuse.WEIGHTS


def gap_tables(V, off, seed):
    """(valid (V, Ftot), root_ok (Ftot)) uint8 with about one entry in six cleared"""
    g = np.random.default_rng(seed)
    return (g.random((V, int(off[-1]))) > 0.16).astype(np.uint8), (g.random(int(off[-1])) > 0.16).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def cases():
    """(tag, inputs of bundle(), want, trace) of the device test: takes of 1, 5, 65, 257 and 600 frames, (V, J) = (4, 17), (3, 5), (2, 17), four
    views with one missing, three takes in one call, gaps in valid and root_ok, fixed given and null, weights with zeros, distort 0 and 1, iters 0,
    1, 3 and 8, sigma inf and finite.  Noisy keypoints: F at the minimum is far above rounding."""
    out = []

    def add(tag, sc, **kw):
        inp, trace = inputs(sc, **kw), []
        out.append((tag, inp, bundle(trace=trace, **inp), trace))

    for n, (F, V, J) in enumerate(((1, 4, 17), (5, 3, 5), (65, 2, 17), (257, 4, 17), (600, 4, 17))):
        add(f"F={F} V={V} J={J}", scene(V, J, [F], seed=200 + n), sigma=0.05)
    sc = scene(4, 17, [1, 70, 40], seed=210)
    add("three takes", sc, sigma=0.05)
    for iters in (0, 1, 8):
        add(f"three takes, iters={iters}", sc, iters=iters, sigma=0.05)
    add("three takes, sigma=inf, pinhole", sc, distort=False)
    add("three takes, sigma=0.004 (two noise scales)", sc, sigma=0.004)
    valid, root_ok = gap_tables(4, sc["off"], 211)
    valid[2, int(sc["off"][1]):int(sc["off"][2])] = 0                    # take 1: four views with one missing
    add("three takes, gaps in valid and root_ok, view 2 missing in take 1", sc, valid=valid, root_ok=root_ok, sigma=0.05)
    fixed = np.array([[1, 0, 0, 0], [1, 1, 0, 0], [0, 0, 0, 1]], np.uint8)
    add("three takes, fixed given, weights with zeros", sc, fixed=fixed, weights=WEIGHTS, sigma=0.05)
    add("257 frames, four views with one missing", scene(4, 17, [257], seed=212), valid=np.repeat(np.array([[1], [1], [0], [1]], np.uint8), 257, axis=1),
        sigma=0.05)
    return out

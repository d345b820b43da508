"""float64 statement of refining placed root trajectories under the full camera model (manipose_amd/lifting.py: place_poses(refine=),
reproject_poses; mp_lift_place_refine), shared by test_lift_refine_host.py and test_gpu_lift_refine.py: the rule of include/manipose_hip.h in
plain Python loops in joint order, nothing else, and the scenes both files use.  Our own code; the linear fit and the camera model are those
of lift_place_ref.py."""
import math

import numpy as np

import lift_place_ref as place

MAXITERS = 16                                           # MP_LIFT_REFINE_MAXITERS
DET_FLOOR, COST_SLACK = 1e-12, 1e-6                     # the two thresholds of the rule


def _clamp1(x):
    return -1.0 if x < -1.0 else (1.0 if x > 1.0 else x)


def _div(a, b):
    """a / b as IEEE has it (Python raises on a zero divisor)"""
    if b != 0.0:
        return a / b
    return float(np.float64(a) / np.float64(b))


def evaluate(pose, kp, intr, w, distort, t, jac=True):
    """One pass over the joints of non-zero weight at the translation t: dict of F, E, W, H (3 x 3 list, symmetric), g (3), deep.  Python floats
    (IEEE: a division by zero gives inf or NaN like the kernel's, not an exception)."""
    fx, fy, cx, cy, k1, k2, k3, p1, p2 = (float(v) for v in np.asarray(intr, np.float64))
    F = E = W = H00 = H01 = H02 = H11 = H12 = H22 = g0 = g1 = g2 = 0.0
    deep = True
    rows_p, rows_u, tx, ty, tz = np.asarray(pose, np.float64).tolist(), np.asarray(kp, np.float64).tolist(), float(t[0]), float(t[1]), float(t[2])
    with np.errstate(all="ignore"):
        for j in range(len(rows_p)):
            wj = float(w[j])
            if wj == 0:
                continue
            X, Y, Z = rows_p[j][0] + tx, rows_p[j][1] + ty, rows_p[j][2] + tz
            if not Z > 0:
                deep = False
            qx, qy = _div(X, Z), _div(Y, Z)
            xx, yy = _clamp1(qx), _clamp1(qy)
            px, py, a, b, c, d = xx, yy, 1.0, 0.0, 0.0, 1.0
            if distort:
                r2 = xx * xx + yy * yy
                m = 1.0 + (k1 * r2 + k2 * (r2 * r2) + k3 * (r2 * r2 * r2)) + (p1 * xx + p2 * yy)
                px, py = xx * m + p1 * r2, yy * m + p2 * r2
                dm = k1 + 2.0 * k2 * r2 + 3.0 * k3 * (r2 * r2)
                mx, my = 2.0 * xx * dm + p1, 2.0 * yy * dm + p2
                a, b = m + xx * mx + 2.0 * p1 * xx, xx * my + 2.0 * p1 * yy
                c, d = yy * mx + 2.0 * p2 * xx, m + yy * my + 2.0 * p2 * yy
            du, dv = fx * px + cx - rows_u[j][0], fy * py + cy - rows_u[j][1]
            rr = du * du + dv * dv
            W += wj
            E += wj * (math.sqrt(rr) if rr >= 0 else float("nan"))
            F += wj * rr
            if not jac:
                continue
            sx, sy = (1.0 if -1.0 <= qx <= 1.0 else 0.0), (1.0 if -1.0 <= qy <= 1.0 else 0.0)
            iz = _div(1.0, Z)
            xz, yz = sx * iz, sy * iz
            xq, yq = sx * _div(-qx, Z), sy * _div(-qy, Z)
            j00, j01, j02 = fx * (a * xz), fx * (b * yz), fx * (a * xq + b * yq)
            j10, j11, j12 = fy * (c * xz), fy * (d * yz), fy * (c * xq + d * yq)
            H00 += wj * (j00 * j00 + j10 * j10); H01 += wj * (j00 * j01 + j10 * j11); H02 += wj * (j00 * j02 + j10 * j12)
            H11 += wj * (j01 * j01 + j11 * j11); H12 += wj * (j01 * j02 + j11 * j12); H22 += wj * (j02 * j02 + j12 * j12)
            g0 += wj * (j00 * du + j10 * dv); g1 += wj * (j01 * du + j11 * dv); g2 += wj * (j02 * du + j12 * dv)
    H, g = [[H00, H01, H02], [H01, H11, H12], [H02, H12, H22]], [g0, g1, g2]
    return dict(F=F, E=E, W=W, H=H, g=g, deep=deep)


def jacobian(point, intr, distort=True):
    """the analytic 2 x 3 Jacobian d pi(P) / dP = d pi(p + t) / dt of the rule at the camera-space point P, through evaluate()'s own arithmetic:
    with the keypoint at pi(P) - (1, 0) the gradient g is the first row, at pi(P) - (0, 1) the second"""
    point = np.asarray(point, np.float64).reshape(1, 3)
    at = place.project(point, intr, distort)[0]
    rows = []
    for r in range(2):
        kp = at.copy()
        kp[r] -= 1.0
        rows.append(np.array(evaluate(point, kp.reshape(1, 2), intr, [1.0], distort, np.zeros(3))["g"]))     # (r = e_r up to one rounding)
    return np.array(rows)


def _finite(*v):
    return all(math.isfinite(x) for x in v)


def step_of(e):
    """(det, H00 H11 H22, d) of one Gauss-Newton step from an evaluation: det by cofactors, d = -adj(H) g / det (None where det is 0 or not finite)"""
    H, g = e["H"], e["g"]
    c00, c01, c02 = H[1][1] * H[2][2] - H[1][2] * H[1][2], H[0][2] * H[1][2] - H[0][1] * H[2][2], H[0][1] * H[1][2] - H[0][2] * H[1][1]
    det, scale = H[0][0] * c00 + H[0][1] * c01 + H[0][2] * c02, H[0][0] * H[1][1] * H[2][2]
    if not _finite(det) or det == 0:
        return det, scale, None
    c11, c12, c22 = H[0][0] * H[2][2] - H[0][2] * H[0][2], H[0][1] * H[0][2] - H[0][0] * H[1][2], H[0][0] * H[1][1] - H[0][1] * H[0][1]
    d = [-(c00 * g[0] + c01 * g[1] + c02 * g[2]) / det, -(c01 * g[0] + c11 * g[1] + c12 * g[2]) / det, -(c02 * g[0] + c12 * g[1] + c22 * g[2]) / det]
    return det, scale, d


def refine_one(pose, kp, intr, weights=None, distort=True, iters=0, start=None, start_ok=1, trace=None):
    """one pose (J, C >= 3), its keypoints (J, 2) -> (t (3,), reproj, ok, steps); start: (3,) float32 values or None (the linear fit).  ``trace``:
    a list that receives one dict per decision (kind, value, threshold, taken) and per evaluation (the sums)."""
    pose, kp = np.asarray(pose, np.float64), np.asarray(kp, np.float64)
    w = np.ones(pose.shape[0]) if weights is None else np.asarray(weights, np.float64)
    if start is None:
        with np.errstate(all="ignore"):
            W, A, B, Q, Sx, Sy, Sc = sums = place.fit_sums(pose, kp, intr, w)
            D = W * Q - A * A - B * B
            if not (W > 0 and np.isfinite(sums).all() and D > 1e-9 * (W * Q)):
                return np.zeros(3), 0.0, 0, 0                             # the degenerate fit
            tz = (W * Sc - A * Sx - B * Sy) / D
            t = np.array([(A * tz - Sx) / W, (B * tz - Sy) / W, tz])     # place_one's t
    else:
        t = np.asarray(start, np.float64)
        if not start_ok or not np.isfinite(t).all() or not sum(float(v) for v in w) > 0:
            return np.asarray(start).copy(), 0.0, 0, 0                    # copied through
    t = [float(v) for v in t]
    e = evaluate(pose, kp, intr, w, distort, t, jac=iters > 0)
    if trace is not None:
        trace.append(dict(kind="eval", **e))
    with np.errstate(all="ignore"):
        if not (e["deep"] and math.isfinite(e["F"])):
            return np.array(t), float(np.float64(e["E"]) / np.float64(e["W"])), 0, 0
        steps = 0
        for _ in range(int(iters)):
            det, scale, d = step_of(e)
            good = _finite(det, scale) and det > DET_FLOOR * scale
            if trace is not None:
                trace.append(dict(kind="det", value=det, threshold=DET_FLOOR * scale, scale=scale, taken=good))
            if not good:
                break
            n = [t[c] + d[c] for c in range(3)]
            if not _finite(*n):
                break
            e2 = evaluate(pose, kp, intr, w, distort, n)
            good = e2["deep"] and e2["F"] <= (1.0 + COST_SLACK) * e["F"]
            if trace is not None:
                trace.append(dict(kind="cost", value=e2["F"], threshold=(1.0 + COST_SLACK) * e["F"], deep=e2["deep"], taken=good,
                                  step=max(abs(v) for v in d)))
            if not good:
                break
            t, e, steps = n, e2, steps + 1
            if trace is not None:
                trace.append(dict(kind="eval", **e))
        return np.array(t), float(np.float64(e["E"]) / np.float64(e["W"])), 1, steps


def refine_all(poses, kp, intr, seq_offset=None, weights=None, distort=True, iters=0, start=None, start_ok=None, trace=None):
    """poses (Ntot, J, C) or (Ntot, inner, J, C), kp (Ntot, J, 2), intr (S, 9), start like traj or None, start_ok like ok or None ->
    traj (Ntot[, inner], 3), reproj (float64; a copied-through start keeps its float32 values), ok, steps (uint8)"""
    poses = np.asarray(poses)
    flat = poses[:, None] if poses.ndim == 3 else poses
    intr = np.asarray(intr).reshape(-1, 9)
    off = [0, flat.shape[0]] if seq_offset is None else [int(v) for v in seq_offset]
    st = None if start is None else np.asarray(start).reshape(flat.shape[:2] + (3,))
    so = None if start_ok is None else np.asarray(start_ok).reshape(flat.shape[:2])
    traj = np.zeros(flat.shape[:2] + (3,))
    err, ok, steps = np.zeros(flat.shape[:2]), np.zeros(flat.shape[:2], np.uint8), np.zeros(flat.shape[:2], np.uint8)
    for s in range(len(off) - 1):
        for g in range(off[s], off[s + 1]):
            for i in range(flat.shape[1]):
                traj[g, i], err[g, i], ok[g, i], steps[g, i] = refine_one(flat[g, i], kp[g], intr[s], weights, distort, iters,
                                                                          None if st is None else st[g, i], 1 if so is None else so[g, i], trace)
    if poses.ndim == 3:
        return traj[:, 0], err[:, 0], ok[:, 0], steps[:, 0]
    return traj, err, ok, steps


def margins(trace):
    """(the smallest relative distance of a cost decision from its threshold, the smallest det / (H00 H11 H22) of a det decision) over a trace; a
    det decision on H = 0 (every projection clamped) compares exact zeros and is left out"""
    cost = [abs(d["value"] - d["threshold"]) / abs(d["threshold"]) for d in trace if d["kind"] == "cost"]
    det = [d["value"] / d["scale"] for d in trace if d["kind"] == "det" and not (d["value"] == 0 and d["scale"] == 0)]      # (H = 0: exactly 0 > 0)
    return (min(cost) if cost else float("inf")), (min(det) if det else float("inf"))


def distorted_scene(lens, inner, ch, intr, seed, noise=0.0):
    """The poses and true translations of lift_place_ref.synthetic_scene(..., noise=0) with keypoints re-made under the FULL camera model:
    kp = float32(project(P0 + t_true, intr[s], True) + noise N(0, 1)), P0 the first inner pose, the noise from default_rng(seed + 1).
    Returns poses, kp, t_true, seq_offset."""
    poses, _, t, off = place.synthetic_scene(lens, inner, ch, intr, seed, noise=0.0)
    g = np.random.default_rng(seed + 1)
    kp = np.zeros((poses.shape[0], 17, 2), np.float32)
    for s in range(len(lens)):
        sl = slice(int(off[s]), int(off[s + 1]))
        P = poses[sl, 0, :, :3].astype(np.float64) + t[sl, None, :].astype(np.float64)
        kp[sl] = (place.project(P, intr[s], True) + noise * g.standard_normal((sl.stop - sl.start, 17, 2))).astype(np.float32)
    return poses, kp, t, off


# ---- the scenes of test_gpu_lift_refine.py, built here so that test_lift_refine_host.py can check their decision margins without a device --------
LENS = [1, 70, 259]                                     # a sequence boundary inside a workgroup of 64 poses, and a tile edge


def s11_intrinsics(n=3):
    from manipose_amd.data.ingest import h36m_cameras
    return np.stack([c["intrinsic"] for c in h36m_cameras()["S11"][:n]]).astype(np.float32)


def fp64_scene(inner, ch):
    """noisy keypoints under the full camera model: the scene of the comparison against the statement"""
    return distorted_scene(LENS, inner, ch, s11_intrinsics(), seed=100 + 10 * inner + ch, noise=0.01)


def recovery_scene():
    """noise-free keypoints under the full camera model: the true translation can be recovered"""
    return distorted_scene(LENS, 1, 3, s11_intrinsics(), seed=7, noise=0.0)


def small_scene():
    """two hypotheses per frame, noisy: weights, the start mode, sequences alone and together"""
    return distorted_scene(LENS, 2, 4, s11_intrinsics(), seed=8, noise=0.01)


CLAMPED, ONE_SPOT, NAN_KP, BEHIND = 1, 2, 4, (6, 1)     # the frames (and the pose) guards_scene() spoils


def guards_scene():
    """8 frames x 2 poses with one camera: (clean poses, clean kp, spoiled poses, spoiled kp, intr).  Frame CLAMPED: keypoints = the pinhole projection
    of the first pose at (8, 8, 5) m, so the linear fit puts every joint at q > 1 in x and y, every projection is clamped and H = 0; frame ONE_SPOT: all
    keypoints coincide, frame NAN_KP: one keypoint is NaN (both: a degenerate fit); pose BEHIND: one joint 40 m behind the others."""
    intr = s11_intrinsics(1)
    poses, kp, _, _ = distorted_scene([8], 2, 3, intr, seed=11, noise=0.01)
    bad_p, bad_k = poses.copy(), kp.copy()
    P = poses[CLAMPED, 0, :, :3].astype(np.float64) + np.array([8.0, 8.0, 5.0])
    bad_k[CLAMPED] = (intr[0, 0:2].astype(np.float64) * (P[:, :2] / P[:, 2:3]) + intr[0, 2:4].astype(np.float64)).astype(np.float32)
    bad_k[ONE_SPOT] = bad_k[ONE_SPOT, 5]
    bad_k[NAN_KP, 9, 1] = np.nan
    bad_p[BEHIND[0], BEHIND[1], 5, 2] = -40.0
    return poses, kp, bad_p, bad_k, intr


def overshoot_start(traj):
    """a start 2.5 m off in x and y: from there some undamped steps land where the cost is several times higher, and are not taken"""
    return (np.asarray(traj, np.float64) + np.array([2.5, 2.5, 0.0])).astype(np.float32)

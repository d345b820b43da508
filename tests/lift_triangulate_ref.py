"""mp_lift_triangulate's rule (include/manipose_hip.h) stated in numpy float64, the seeded scenes its tests share, and their bounds.

The statement works on the float32 inputs the kernel gets and follows the header step by step, ITEM BY ITEM - one (frame, joint) at a time, numpy
float64 scalars in the rule's order of additions (views in order; a sum a + b + c is (a + b) + c, as the kernel's source reads without
contraction).  The rotation, the quaternion test and the projection with its Jacobian are lift_bundle_ref's (rotation, unit, project_jac); the
scenes are lift_fuse_ref.place_scene's.  The statement also returns what the kernel does not: a trace of every decision with its distance from
its threshold - det against 1e-12 H00 H11 H22 for the start ("det0") and for each step ("det"), the smallest Z / |P| of an evaluation against 0
("deep"), F' / F - 1 against the slack 1e-6 ("cost")."""
import functools
import math

import numpy as np

import lift_bundle_ref as bundle
import lift_fuse_ref as fuse

MAXITERS = 16                                           # MP_LIFT_REFINE_MAXITERS
DET_FLOOR, COST_SLACK = 1e-12, 1e-6
STORE_TOL = bundle.STORE_TOL                            # the project's bound for a float32 store, times max(1, |x|)
MARGIN_MIN = bundle.MARGIN_MIN                          # every decision of a scene the device is compared on is at least this far from its threshold
F64 = np.float64


class View:
    """one observation of an item: its view, weight, the view's rotation (3 x 3), translation (3), intrinsics (9), the keypoint"""
    __slots__ = ("v", "w", "R", "T", "intr", "ku", "kv")

    def __init__(self, v, w, R, T, intr, ku, kv):
        self.v, self.w, self.R, self.T, self.intr, self.ku, self.kv = v, F64(w), R, T, intr, F64(ku), F64(kv)


def camera_point(o, X):
    """P = R^T (X - T) in the kernel's order"""
    R = o.R
    wx, wy, wz = X[0] - o.T[0], X[1] - o.T[1], X[2] - o.T[2]
    return (R[0, 0] * wx + R[1, 0] * wy + R[2, 0] * wz, R[0, 1] * wx + R[1, 1] * wy + R[2, 1] * wz, R[0, 2] * wx + R[1, 2] * wy + R[2, 2] * wz)


def residual_jac(o, X, distort):
    """one observation at the world point X: ((du, dv), the 2 x 3 Jacobian J_pi R^T with respect to X, Z, Z / |P|)"""
    Xc, Yc, Zc = camera_point(o, X)
    du, dv, (c00, c01, c02, c10, c11, c12) = bundle.project_jac(Xc, Yc, Zc, o.ku, o.kv, o.intr, distort)
    R = o.R
    rows = ((c00 * R[0, 0] + c01 * R[0, 1] + c02 * R[0, 2], c00 * R[1, 0] + c01 * R[1, 1] + c02 * R[1, 2], c00 * R[2, 0] + c01 * R[2, 1] + c02 * R[2, 2]),
            (c10 * R[0, 0] + c11 * R[0, 1] + c12 * R[0, 2], c10 * R[1, 0] + c11 * R[1, 1] + c12 * R[1, 2], c10 * R[2, 0] + c11 * R[2, 1] + c12 * R[2, 2]))
    with np.errstate(all="ignore"):
        ratio = Zc / np.sqrt(Xc * Xc + Yc * Yc + Zc * Zc)
    return (F64(du), F64(dv)), rows, Zc, float(ratio) if math.isfinite(float(ratio)) else -math.inf


def normal_add(H, g, w, du, dv, r0, r1):
    """lift_geom.h's lift_normal3_add: H (upper triangle: 00 01 02 11 12 22) and g"""
    H[0] += w * (r0[0] * r0[0] + r1[0] * r1[0]); H[1] += w * (r0[0] * r0[1] + r1[0] * r1[1]); H[2] += w * (r0[0] * r0[2] + r1[0] * r1[2])
    H[3] += w * (r0[1] * r0[1] + r1[1] * r1[1]); H[4] += w * (r0[1] * r0[2] + r1[1] * r1[2]); H[5] += w * (r0[2] * r0[2] + r1[2] * r1[2])
    g[0] += w * (r0[0] * du + r1[0] * dv); g[1] += w * (r0[1] * du + r1[1] * dv); g[2] += w * (r0[2] * du + r1[2] * dv)


def solve3(H, g):
    """lift_adj3 and lift_adj3_solve: (det, H00 H11 H22, passed, adj(H) g / det)"""
    H00, H01, H02, H11, H12, H22 = H
    with np.errstate(all="ignore"):
        c00, c01, c02 = H11 * H22 - H12 * H12, H02 * H12 - H01 * H22, H01 * H12 - H02 * H11
        det = H00 * c00 + H01 * c01 + H02 * c02
        scale = H00 * H11 * H22
        c11, c12, c22 = H00 * H22 - H02 * H02, H01 * H02 - H00 * H12, H00 * H11 - H01 * H01
        passed = bool(np.isfinite(det) and np.isfinite(scale) and det > DET_FLOOR * scale)
        x = ((c00 * g[0] + c01 * g[1] + c02 * g[2]) / det, (c01 * g[0] + c11 * g[1] + c12 * g[2]) / det, (c02 * g[0] + c12 * g[1] + c22 * g[2]) / det)
    return det, scale, passed, x


def det_margin(det, scale):
    """the distance of det / (H00 H11 H22) from 1e-12 in units of 1e-12; a scale of exactly 0 decides without rounding"""
    with np.errstate(all="ignore"):
        if not (np.isfinite(det) and np.isfinite(scale)) or scale == 0:
            return math.inf
        return float(abs(det / scale - DET_FLOOR) / DET_FLOOR)


def linear_sums(obs):
    """3.: H (6), h (3) of the linear pinhole triangulation"""
    H, h = [F64(0)] * 6, [F64(0)] * 3
    with np.errstate(all="ignore"):
        for o in obs:
            fx, fy, cx, cy = (F64(c) for c in o.intr[:4])
            R = o.R
            a, b = (o.ku - cx) / fx, (o.kv - cy) / fy
            mx = (R[0, 0] - a * R[0, 2], R[1, 0] - a * R[1, 2], R[2, 0] - a * R[2, 2])
            my = (R[0, 1] - b * R[0, 2], R[1, 1] - b * R[1, 2], R[2, 1] - b * R[2, 2])
            sx = mx[0] * o.T[0] + mx[1] * o.T[1] + mx[2] * o.T[2]
            sy = my[0] * o.T[0] + my[1] * o.T[1] + my[2] * o.T[2]
            normal_add(H, h, o.w, sx, sy, mx, my)
    return H, h


def linear_rows(obs):
    """the stacked equations the linear start solves in the least-squares sense: (A (2 n, 3), b (2 n)), rows scaled by sqrt(w)"""
    A, b = [], []
    for o in obs:
        fx, fy, cx, cy = (float(c) for c in o.intr[:4])
        u, v = (float(o.ku) - cx) / fx, (float(o.kv) - cy) / fy
        for m in (o.R[:, 0] - u * o.R[:, 2], o.R[:, 1] - v * o.R[:, 2]):
            A.append(math.sqrt(float(o.w)) * m)
            b.append(math.sqrt(float(o.w)) * float(m @ o.T))
    return np.array(A), np.array(b)


def evaluate(obs, X, sigma2, prior, X0, pull, distort, jac=True):
    """4. at X: dict of F, E, W, H (6), g (3), deep, minz (the smallest Z / |P|, inf without an observation)"""
    F, E, W = F64(0), F64(0), F64(0)
    H, g = [F64(0)] * 6, [F64(0)] * 3
    deep, minz = True, math.inf
    X = tuple(F64(c) for c in X)
    with np.errstate(all="ignore"):
        for o in obs:
            (du, dv), (r0, r1), Z, ratio = residual_jac(o, X, distort)
            if not Z > 0.0:
                deep = False
            minz = min(minz, ratio)
            e = du * du + dv * dv
            t = 1.0 + e / sigma2
            W += o.w
            E += o.w * np.sqrt(e)
            F += o.w * (e / t)
            if jac:
                normal_add(H, g, o.w * (1.0 / (t * t)), du, dv, r0, r1)
        if pull:
            dx, dy, dz = X[0] - X0[0], X[1] - X0[1], X[2] - X0[2]
            F += prior * ((dx * dx + dy * dy) + dz * dz)
            if jac:
                H[0] += prior; H[3] += prior; H[5] += prior
                g[0] += prior * dx; g[1] += prior * dy; g[2] += prior * dz
    return dict(F=F, E=E, W=W, H=H, g=g, deep=deep, minz=minz)


FAILED = dict(point=(0.0, 0.0, 0.0), err=0.0, ok=0, steps=0)


def triangulate_item(obs, X0, usable, sigma2, prior, distort, iters, note=lambda **kw: None):
    """steps 3 to 6 for one item: obs its observations in view order, X0 the prior point -> dict of point, err, ok, steps"""
    n = len(obs)
    pull = bool(prior > 0 and usable)
    X, tri = None, False
    if n >= 2:
        H, h = linear_sums(obs)
        det, scale, passed, x = solve3(H, h)
        note(kind="det0", taken=passed, margin=det_margin(det, scale))
        if passed and all(np.isfinite(c) for c in x):
            X, tri = x, True
    if X is None:
        if not usable:
            return dict(FAILED)
        X = X0
    jac = iters > 0
    e = evaluate(obs, X, sigma2, prior, X0, pull, distort, jac)
    if n:
        note(kind="deep", taken=e["deep"], margin=abs(e["minz"]))
    if tri and not e["deep"] and usable:
        X, tri = X0, False
        e = evaluate(obs, X, sigma2, prior, X0, pull, distort, jac)
        note(kind="deep", taken=e["deep"], margin=abs(e["minz"]))
    if not (e["deep"] and np.isfinite(e["F"])):
        return dict(FAILED)
    steps = 0
    with np.errstate(all="ignore"):
        for _ in range(int(iters)):
            det, scale, passed, d = solve3(e["H"], e["g"])
            note(kind="det", taken=passed, margin=det_margin(det, scale))
            if not passed:
                break
            cand = (X[0] - d[0], X[1] - d[1], X[2] - d[2])
            if not all(np.isfinite(c) for c in cand):
                break
            e2 = evaluate(obs, cand, sigma2, prior, X0, pull, distort, True)
            good = bool(e2["deep"] and e2["F"] <= (1.0 + COST_SLACK) * e["F"])
            if n:
                note(kind="deep", taken=e2["deep"], margin=abs(e2["minz"]))
            if not (e["F"] == 0 and e2["F"] == 0):                          # (0 <= 0: decided without rounding)
                note(kind="cost", taken=good, margin=float(abs(e2["F"] / e["F"] - 1.0 - COST_SLACK) / COST_SLACK), F=float(e2["F"]))
            if not good:
                break
            X, e, steps = cand, e2, steps + 1
        err = float(e["E"] / e["W"]) if n else 0.0
    return dict(point=tuple(float(c) for c in X), err=err, ok=1 | (2 if tri else 0), steps=steps)


def take_of(raw, ftot, f):
    """(take g of frame f: the last with raw[g] <= f, 0 if none; whether g's clamped range holds f)"""
    G = len(raw) - 1
    g = max([t for t in range(G) if raw[t] <= f], default=0)
    f0 = min(max(raw[g], 0), ftot)
    f1 = min(max(raw[g + 1], f0), ftot)
    return g, f0 <= f < f1


def observations(kp, kp_weight, valid, units, trans, intr, g, f, j):
    """2.: the observations of item (f, j) of take g in view order; units[g][v]: (unit quaternion's matrix or None)"""
    obs = []
    for v in range(kp.shape[0]):
        if units[g][v] is None or (valid is not None and valid[v][f] == 0):
            continue                                                       # an invalid view's data is never looked at
        ku, kv = float(kp[v, f, j, 0]), float(kp[v, f, j, 1])
        w = 1.0 if kp_weight is None else float(kp_weight[v, f, j])
        if not (math.isfinite(ku) and math.isfinite(kv) and math.isfinite(w) and w > 0.0):
            continue
        obs.append(View(v, w, units[g][v], trans[g, v], intr[g, v], ku, kv))
    return obs


def triangulate(pose, root, kp, quat, trans, intr, valid=None, take_offset=None, root_ok=None, kp_weight=None, distort=True, sigma=float("inf"),
                prior=0.0, iters=3, trace=None):
    """The rule on float32 inputs: dict of points (Ftot, J, 3), err (Ftot, J) float64, views, ok, steps (Ftot, J) uint8 and written (Ftot) bool:
    the frames a take holds (the others are zeros here and untouched by the kernel)."""
    pose, root, kp = np.asarray(pose), np.asarray(root), np.asarray(kp)
    V, ftot, J = kp.shape[:3]
    raw = [0, ftot] if take_offset is None else [int(v) for v in take_offset]
    G = len(raw) - 1
    quat, trans, intr = (np.asarray(a).reshape(G, V, -1) for a in (quat, trans, intr))
    trans, intr = trans.astype(np.float64), intr.astype(np.float64)
    units = [[None if bundle.unit(quat[g, v]) is None else bundle.rotation(bundle.unit(quat[g, v])) for v in range(V)] for g in range(G)]
    s = F64(np.float32(sigma))
    with np.errstate(over="ignore"):
        sigma2 = s * s
    pr = F64(np.float32(prior))
    out = dict(points=np.zeros((ftot, J, 3)), err=np.zeros((ftot, J)), views=np.zeros((ftot, J), np.uint8), ok=np.zeros((ftot, J), np.uint8),
               steps=np.zeros((ftot, J), np.uint8), written=np.zeros(ftot, bool))
    for f in range(ftot):
        g, held = take_of(raw, ftot, f)
        if not held:
            continue
        out["written"][f] = True
        for j in range(J):
            with np.errstate(all="ignore"):
                X0 = tuple(F64(pose[f, j, c]) + F64(root[f, c]) for c in range(3))
            usable = bool((root_ok is None or root_ok[f] != 0) and all(np.isfinite(c) for c in X0))
            obs = observations(kp, kp_weight, valid, units, trans, intr, g, f, j)
            note = (lambda f=f, j=j, **kw: trace.append(dict(kw, item=(f, j)))) if trace is not None else (lambda **kw: None)
            res = triangulate_item(obs, X0, usable, sigma2, pr, bool(distort), int(iters), note)
            out["points"][f, j], out["err"][f, j], out["ok"][f, j], out["steps"][f, j] = res["point"], res["err"], res["ok"], res["steps"]
            out["views"][f, j] = sum(1 << o.v for o in obs)
    return out


def margin(trace):
    """the smallest distance of a decision from its threshold, in units of the threshold's slack: det / (H00 H11 H22) from 1e-12 in units of
    1e-12, F' / F - 1 from 1e-6 in units of 1e-6, an observation's Z / |P| from 0"""
    m = [d["margin"] for d in trace]
    return min(m) if m else math.inf


within_store = bundle.within_store


# ---- the scenes ------------------------------------------------------------------------------------------------------------------------------
def scene(V, J, lens, seed, noise=0.002, pose_noise=0.03, root_noise=0.0):
    """lift_fuse_ref.place_scene (poses 0.3 N(0, 1), roots x, y in +-1 m and z in 0.8 .. 1.0 m, keypoints = the full camera model of S11's first V
    cameras plus noise N(0, 1)) with a LIFTED pose that is off: every coordinate of every joint but joint 0 by pose_noise N(0, 1) (0.03: 45 mm mean
    per joint), the root by root_noise N(0, 1).  Returns a dict: the float32 inputs pose, root, kp, quat, trans, intr, off and truth (Ftot, J, 3)."""
    pose, kp, root, (quat, trans, intr), off = fuse.place_scene(V, J, lens, seed, noise)
    g = np.random.default_rng(seed + 2000)
    truth = pose.astype(np.float64) + root[:, None, :]
    lifted = pose + pose_noise * g.standard_normal(pose.shape)
    lifted[:, 0] = 0
    start = root + root_noise * g.standard_normal(root.shape)
    return dict(pose=lifted.astype(np.float32), root=start.astype(np.float32), kp=kp, quat=quat, trans=trans, intr=intr, off=off, truth=truth)


def inputs(sc, **kw):
    """the arguments of triangulate() of a scene"""
    return dict(dict(pose=sc["pose"], root=sc["root"], kp=sc["kp"], quat=sc["quat"], trans=sc["trans"], intr=sc["intr"], take_offset=sc["off"]), **kw)


def errors(points, sc):
    """(Ftot, J) distances in metres between points and the scene's truth"""
    return np.linalg.norm(np.asarray(points, np.float64) - sc["truth"], axis=-1)


def lifted_errors(sc):
    """those of the prior points, the lifted pose plus root"""
    return errors(sc["pose"].astype(np.float64) + sc["root"].astype(np.float64)[:, None, :], sc)


RECOVERY = dict(J=17, lens=(60,), seed=7)               # S11's cameras, 60 frames, 17 joints, the lifted pose 0.03 m N(0, 1) off: 45.1 mm mean


@functools.lru_cache(maxsize=None)
def recovery(V=4, noise=0.0, root_noise=0.0):
    return scene(V, RECOVERY["J"], list(RECOVERY["lens"]), RECOVERY["seed"], noise=noise, root_noise=root_noise)


# What the statement reaches on the committed seeds, measured in fp64 (test_lift_triangulate_host.py prints each figure before it asserts); every
# bound is TWICE the measured value, the project's convention.  A float32 STORE of a coordinate |x| < 8 m adds its own half ulp, 2^-22 per
# coordinate: the device test adds sqrt(3) 2^-22.
# Claim 1, noise-free float32 keypoints, the largest miss of a joint in metres.  4 views: the linear start alone 5.73e-2 (mean 1.09e-2), 1 step
# 5.24e-4 (mean 1.76e-5), 2 steps 7.12e-8 (mean 2.05e-8), 3 steps 7.07e-8 and 5 steps the same: the keypoints' own rounding.  2 views: 2 steps
# 3.59e-7, 3 steps 2.59e-7 (mean 2.75e-8) and 5 steps the same (a few joints stop a step early: at rounding the cost no longer falls).
MEASURED_4V, MEASURED_2V = 7.12e-8, 2.592e-7
RECOVERY_4V, RECOVERY_2V = 2 * MEASURED_4V, 2 * MEASURED_2V
RECOVERY_STEPS_4V, RECOVERY_STEPS_2V = 2, 3
STORE_POINT = float(np.sqrt(3.0) * 2.0 ** -22)
# Claim 2, noise 0.002 (about 1 px), 4 views, 3 steps: the mean error is 5.58e-3 m against the lifted pose's 4.43e-2 m (the claim: below a quarter
# of it).  With noise 0.01: 2.79e-2 m with 4 views, 4.30e-2 m with 2.
MEASURED_NOISY_4V, MEASURED_LIFTED = 5.58e-3, 4.43e-2
# Claim 3, one view, prior 0.01, noise 0.002, 3 steps: the mean error is 2.44e-2 m against the lifted pose's 4.43e-2 m (the claim: below it)
MEASURED_ONE_VIEW = 2.44e-2
ONE_VIEW_PRIOR = 0.01
# Claim 4, the root 0.1 m N(0, 1) off (the prior points 0.175 m off in the mean), 4 views, 2 steps, noise-free, prior 0: the largest miss is
# 7.12e-8 m, claim 1's to the last digit (the claim: claim 1's bound - the start does not depend on X0 where the linear start stands)
MEASURED_ROOT_OFF = 7.12e-8
ROOT_OFF = 0.1


# ---- the constructed items: every rule of the fallbacks ------------------------------------------------------------------------------------------
NO_VIEW, NOTHING, ONE_VIEW, NAN_KP, WEIGHTS, NO_ROOT, BEHIND, PLAIN = range(8)     # the frames constructed() spoils
BEHIND_VIEWS = (0, 1)


def constructed(prior=0.0):
    """scene(4, 5, [8]) with one rule per frame.  NO_VIEW: no valid view, X0 usable; NOTHING: no valid view and root_ok = 0; ONE_VIEW: view 0 alone;
    NAN_KP: view 1's keypoints have a NaN coordinate; WEIGHTS: the weights of views 0, 1, 2 are 0, -1 and NaN; NO_ROOT: root_ok = 0 under four
    views; BEHIND: views 0 and 1 alone, their keypoints the pinhole images of a point 1.5 m BEHIND camera 0 (the linear start finds it); PLAIN:
    untouched.  Returns the arguments of triangulate()."""
    sc = scene(4, 5, [8], seed=420)
    kp, valid, root_ok = sc["kp"].copy(), np.ones((4, 8), np.uint8), np.ones(8, np.uint8)
    w = np.ones((4, 8, 5), np.float32)
    valid[:, NO_VIEW] = 0
    valid[:, NOTHING], root_ok[NOTHING] = 0, 0
    valid[1:, ONE_VIEW] = 0
    kp[1, NAN_KP, :, 0] = np.nan
    w[0, WEIGHTS], w[1, WEIGHTS], w[2, WEIGHTS] = 0.0, -1.0, np.nan
    root_ok[NO_ROOT] = 0
    valid[2:, BEHIND] = 0
    R0 = bundle.rotation(bundle.unit(sc["quat"][0, 0]))
    for j in range(5):
        X = sc["trans"][0, 0].astype(np.float64) - 1.5 * R0[:, 2] + 0.05 * np.array([j, -j, 1.0])
        for v in BEHIND_VIEWS:
            R = bundle.rotation(bundle.unit(sc["quat"][0, v]))
            P = (X - sc["trans"][0, v].astype(np.float64)) @ R
            fx, fy, cx, cy = (float(c) for c in sc["intr"][0, v, :4])
            kp[v, BEHIND, j] = (fx * P[0] / P[2] + cx, fy * P[1] / P[2] + cy)
    return inputs(sc, kp=kp, valid=valid, root_ok=root_ok, kp_weight=w, prior=prior, sigma=0.05)


def twins():
    """two views with IDENTICAL cameras and keypoints: the linear system has rank 2, the start is degenerate and the items start from X0; with
    prior = 0 every step is refused by the 1e-12 rule as well"""
    sc = scene(2, 5, [3], seed=421)
    quat, trans, intr, kp = sc["quat"].copy(), sc["trans"].copy(), sc["intr"].copy(), sc["kp"].copy()
    quat[0, 1], trans[0, 1], intr[0, 1], kp[1] = quat[0, 0], trans[0, 0], intr[0, 0], kp[0]
    return inputs(sc, quat=quat, trans=trans, intr=intr, kp=kp)


def zero_quaternion():
    """view 0 of the take has a zero quaternion: it is no observation anywhere (the Python entry refuses such a camera: through the C entry)"""
    sc = scene(3, 5, [4], seed=422)
    quat = sc["quat"].copy()
    quat[0, 0] = 0
    return inputs(sc, quat=quat, sigma=0.05)


# ---- the device test's cases -----------------------------------------------------------------------------------------------------------------
def gap_tables(V, ftot, seed):
    """(valid (V, Ftot), root_ok (Ftot)) uint8 with about one entry in six cleared"""
    g = np.random.default_rng(seed)
    return (g.random((V, ftot)) > 0.16).astype(np.uint8), (g.random(ftot) > 0.16).astype(np.uint8)


def weight_table(V, ftot, J, seed):
    """kp_weight (V, Ftot, J) float32: about one in five exactly 0, the others fractional in 0.25 .. 1"""
    g = np.random.default_rng(seed)
    w = g.uniform(0.25, 1.0, (V, ftot, J))
    w[g.random((V, ftot, J)) < 0.2] = 0.0
    return w.astype(np.float32)


@functools.lru_cache(maxsize=None)
def cases():
    """(tag, inputs of triangulate(), want, trace) of the device test: takes of 1, 5, 16 and 65 frames at J = 17 (17, 85, 272 and 1105 items: below,
    at and across workgroup boundaries) and one of 257 frames at J = 2; (V, J) = (4, 17), (3, 5), (2, 17), (1, 17); four views with one missing;
    three takes in one call; gaps in valid and root_ok; kp_weight null and with zeros and fractions; distort 0 and 1; iters 0, 1, 3 and 16; sigma
    inf and finite; prior 0 and 0.01.  Noisy keypoints: F at the minimum is far above rounding."""
    out = []

    def add(tag, sc, **kw):
        inp, trace = inputs(sc, **kw), []
        out.append((tag, inp, triangulate(trace=trace, **inp), trace))

    for n, (F, V, J) in enumerate(((1, 4, 17), (5, 4, 17), (16, 2, 17), (65, 4, 17), (257, 4, 2), (7, 3, 5), (6, 1, 17))):
        add(f"F={F} V={V} J={J}", scene(V, J, [F], seed=400 + n), sigma=0.05, prior=0.01 if V == 1 else 0.0)
    sc = scene(4, 17, [1, 9, 6], seed=410)
    ftot = int(sc["off"][-1])
    add("three takes", sc)
    for iters in (0, 1, 16):
        add(f"three takes, iters={iters}", sc, iters=iters, sigma=0.05)
    add("three takes, pinhole, prior 0.01", sc, distort=False, prior=0.01)
    add("three takes, sigma=0.004 (two noise scales)", sc, sigma=0.004)
    valid, root_ok = gap_tables(4, ftot, 411)
    valid[2, int(sc["off"][1]):int(sc["off"][2])] = 0                    # take 1: four views with one missing
    w = weight_table(4, ftot, 17, 412)
    add("three takes, gaps in valid and root_ok, view 2 missing in take 1", sc, valid=valid, root_ok=root_ok, sigma=0.05)
    add("three takes, gaps, weights with zeros and fractions", sc, valid=valid, root_ok=root_ok, kp_weight=w, sigma=0.05)
    add("three takes, gaps, weights, prior 0.01", sc, valid=valid, root_ok=root_ok, kp_weight=w, sigma=0.05, prior=0.01)
    return out

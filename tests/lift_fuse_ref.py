"""float64 statement of fusing the camera views of a take (manipose_amd/lifting.py: fuse_views, place_views; mp_lift_fuse, mp_lift_fuse_place),
shared by test_lift_fuse_host.py and test_gpu_lift_fuse.py: the rules of include/manipose_hip.h in plain numpy and Python loops, nothing else, and
the scenes both files use.  Our own code; a view's projection, Jacobian and per-joint sums are lift_refine_ref.evaluate on the camera-space points
(its H and g are taken into the world with the view's rotation: J_j R^T), the step is lift_refine_ref.step_of."""
import functools
import itertools
import math

import numpy as np

import lift_place_ref as place
import lift_refine_ref as refine

BIG = 1e30
DET_FLOOR, COST_SLACK = refine.DET_FLOOR, refine.COST_SLACK
TAKES = [1, 6, 37]                                      # a take boundary inside a workgroup
# the root's largest miss in metres on the noise-free recovery scene after 0, 1, 2 and 3 steps: what the statement gives ("Fusing the
# views of a take": the last two are the float32 keypoints' rounding), rounded up by a factor of 2
ROOT_MISS = (5.4e-2, 1.3e-4, 3.8e-8, 3.8e-8)


def rotation(q):
    """the matrix of q / |q| (w, x, y, z), or None where |q|^2 is not finite or < 1e-12; q None: the identity"""
    if q is None:
        return np.eye(3)
    q = np.asarray(q, np.float64)
    with np.errstate(all="ignore"):
        n2 = float((q * q).sum())
    if not (math.isfinite(n2) and n2 >= 1e-12):
        return None
    w, x, y, z = q / math.sqrt(n2)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def _take_of(off, f):
    return max(g for g in range(len(off) - 1) if off[g] <= f) if f >= off[0] else 0


def _offsets(take_offset, ftot):
    return [0, ftot] if take_offset is None else [int(v) for v in take_offset]


# ---- mp_lift_fuse ---------------------------------------------------------------------------------------------------------------------------
def fuse_frame(x, rots, sigma, score_weight):
    """x (V, K, J, C) one frame's hypotheses, rots: per view a 3 x 3 matrix, or None for an invalid view (its data is not looked at) ->
    dict(pose (J, 3), choice (V,), cost, spread, ok, gap: second-best E minus best E, inf with one combination)"""
    V, K, J, C = x.shape
    views = [v for v in range(V) if rots[v] is not None]
    n = len(views)
    if n == 0:
        return dict(pose=np.zeros((J, 3)), choice=np.full(V, 255, np.uint8), cost=0.0, spread=0.0, ok=0, gap=math.inf)
    w, u = {}, {}
    with np.errstate(all="ignore"):
        for v in views:
            xv = np.asarray(x[v], np.float64)
            d = xv[:, :, :3] - xv[:, :1, :3]
            w[v] = d @ rots[v].T                                                  # (the identity multiplies by 1 and adds 0: exact)
            s = xv[:, 0, 3] if C == 4 else np.ones(K)
            u[v] = -np.log(np.where(s > 1e-12, s, 1e-12)) if C == 4 else np.zeros(K)
        pair = {}
        for a, b in itertools.combinations(views, 2):
            t = np.zeros((K, K))
            for i in range(K):
                for l in range(K):
                    s = 0.0
                    for e in ((w[a][i] - w[b][l]) ** 2).reshape(-1).tolist():      # joint order, then channel order
                        s += e
                    s /= J
                    t[i, l] = s if math.isfinite(s) else BIG
            pair[a, b] = t
        factor = 1.0 / (2.0 * float(sigma) * float(sigma))
        best, second, choice = None, math.inf, None
        for c in itertools.product(range(K), repeat=n):                            # lexicographic, view 0 most significant
            k = dict(zip(views, c))
            pairs = 0.0
            for a, b in itertools.combinations(views, 2):
                pairs += pair[a, b][k[a], k[b]]
            unary = 0.0
            for v in views:
                unary += u[v][k[v]]
            E = factor * pairs + float(score_weight) * unary
            if best is None or E < best:
                if best is not None:
                    second = min(second, best)
                best, choice = E, k
            else:
                second = min(second, E)
        total = np.zeros((J, 3))
        for v in views:
            total = total + w[v][choice[v]]
        pose = total / n
        dev = 0.0
        for v in views:
            dev += float(((w[v][choice[v]] - pose) ** 2).sum())
        pose[0] = 0.0
        out = np.full(V, 255, np.uint8)
        for v in views:
            out[v] = choice[v]
        return dict(pose=pose, choice=out, cost=best, spread=math.sqrt(dev / (n * J)), ok=0 if best >= BIG else 1, gap=second - best)


def fuse_all(hyps, quat=None, valid=None, take_offset=None, sigma=0.02, score_weight=1.0):
    """hyps (V, Ftot, K, J, C), quat (G, V, 4) or None, valid (V, Ftot) or None -> dict of pose (Ftot, J, 3), choice (Ftot, V), cost, spread, ok, gap"""
    hyps = np.asarray(hyps)
    V, ftot, K, J, C = hyps.shape
    off = _offsets(take_offset, ftot)
    out = dict(pose=np.zeros((ftot, J, 3)), choice=np.zeros((ftot, V), np.uint8), cost=np.zeros(ftot), spread=np.zeros(ftot), ok=np.zeros(ftot, np.uint8),
               gap=np.zeros(ftot))
    for f in range(ftot):
        g = _take_of(off, f)
        rots = []
        for v in range(V):
            R = rotation(None if quat is None else quat[g][v])
            rots.append(R if (valid is None or valid[v][f]) else None)
        r = fuse_frame(hyps[:, f], rots, sigma, score_weight)
        for k in out:
            out[k][f] = r[k]
    return out


# ---- mp_lift_fuse_place ---------------------------------------------------------------------------------------------------------------------
def camera_points(pose, root, R, T):
    """P = R^T (pose_j + r - T): (J, 3) camera-space points"""
    return (np.asarray(pose, np.float64) + np.asarray(root, np.float64) - np.asarray(T, np.float64)) @ R


def project_view(pose, root, R, T, intr, distort=True):
    return place.project(camera_points(pose, root, R, T), intr, distort)


def linear_sums(pose, kps, cams, w):
    """H (3 x 3), h (3), W of the linear pinhole fit; kps: per view (J, 2) or None (invalid), cams: per view (R, T, intr)"""
    H, h, W = np.zeros((3, 3)), np.zeros(3), 0.0
    pose = np.asarray(pose, np.float64)
    with np.errstate(all="ignore"):
        for v, kp in enumerate(kps):
            if kp is None:
                continue
            R, T, intr = cams[v]
            fx, fy, cx, cy = (float(c) for c in np.asarray(intr, np.float64)[:4])
            rx, ry, rz = R[:, 0], R[:, 1], R[:, 2]                                  # the rows of R^T
            for j in range(pose.shape[0]):
                if w[j] == 0:
                    continue
                a, b = (float(kp[j][0]) - cx) / fx, (float(kp[j][1]) - cy) / fy
                mx, my = rx - a * rz, ry - b * rz
                c = np.asarray(T, np.float64) - pose[j]
                W += float(w[j])
                H += float(w[j]) * (np.outer(mx, mx) + np.outer(my, my))
                h += float(w[j]) * (mx * float(mx @ c) + my * float(my @ c))
    return H, h, W


def linear_cost(pose, kps, cams, w, r):
    """the quadratic the linear fit minimises: sum w [(m_x . (pose_j + r - T))^2 + (m_y . (pose_j + r - T))^2]"""
    total = 0.0
    for v, kp in enumerate(kps):
        if kp is None:
            continue
        R, T, intr = cams[v]
        fx, fy, cx, cy = (float(c) for c in np.asarray(intr, np.float64)[:4])
        P = camera_points(pose, r, R, T)
        for j in range(P.shape[0]):
            a, b = (float(kp[j][0]) - cx) / fx, (float(kp[j][1]) - cy) / fy
            total += float(w[j]) * ((P[j, 0] - a * P[j, 2]) ** 2 + (P[j, 1] - b * P[j, 2]) ** 2)
    return total


def _solve(H, h):
    """(det, H00 H11 H22, adj(H) h / det or None) by cofactors"""
    e = dict(H=[[float(v) for v in row] for row in H], g=[-float(v) for v in h])
    return refine.step_of(e)


def evaluate(pose, kps, cams, w, distort, r, jac=True):
    """the sums over the valid views in order, then the joints: dict of F, E, W, H, g, deep, minz (the smallest Z / |P| of a weighted joint) and
    views (per view E_v, W_v)"""
    tot = dict(F=0.0, E=0.0, W=0.0, H=np.zeros((3, 3)), g=np.zeros(3), deep=True, minz=math.inf, views={})
    for v, kp in enumerate(kps):
        if kp is None:
            continue
        R, T, intr = cams[v]
        P = camera_points(pose, r, R, T)
        e = refine.evaluate(P, kp, intr, w, distort, np.zeros(3), jac=jac)
        tot["F"] += e["F"]; tot["E"] += e["E"]; tot["W"] += e["W"]
        tot["H"] = tot["H"] + R @ np.array(e["H"]) @ R.T                            # (J R^T)^T (J R^T)
        tot["g"] = tot["g"] + R @ np.array(e["g"])
        tot["deep"] = tot["deep"] and e["deep"]
        keep = np.asarray(w, np.float64) != 0
        with np.errstate(all="ignore"):
            tot["minz"] = min(tot["minz"], float((P[keep, 2] / np.linalg.norm(P[keep], axis=1)).min()))
        tot["views"][v] = (e["E"], e["W"])
    return tot


def jacobian_view(point, R, T, intr, distort=True):
    """d pi(R^T (p - T)) / dp at the world point p, 2 x 3: the camera-space Jacobian of lift_refine_ref times R^T"""
    P = (np.asarray(point, np.float64) - np.asarray(T, np.float64)) @ R
    return refine.jacobian(P, intr, distort) @ R.T


def place_frame(pose, kps, cams, weights=None, distort=True, iters=3, trace=None):
    """one frame: pose (J, 3), kps per view (J, 2) or None, cams per view (R, T, intr) -> (root (3,), reproj (V,), ok, steps).  trace receives one
    dict per decision: kind in (det0, deep, det, cost), margin = its relative distance from the threshold"""
    V = len(kps)
    pose = np.asarray(pose, np.float64)
    w = np.ones(pose.shape[0]) if weights is None else np.asarray(weights, np.float64)
    zero = (np.zeros(3), np.zeros(V), 0, 0)
    if all(kp is None for kp in kps):
        return zero
    with np.errstate(all="ignore"):
        H, h, W = linear_sums(pose, kps, cams, w)
        det, scale, r = _solve(H, h)
        fine = W > 0 and np.isfinite(H).all() and np.isfinite(h).all() and math.isfinite(W) and math.isfinite(det) and math.isfinite(scale)
        good = bool(fine and det > DET_FLOOR * scale and r is not None and all(math.isfinite(c) for c in r))
        if trace is not None and fine:
            trace.append(dict(kind="det0", taken=good, margin=abs(det / scale - DET_FLOOR) / DET_FLOOR if scale != 0 else 0.0))
        if not good:
            return zero
        e = evaluate(pose, kps, cams, w, distort, r, jac=iters > 0)
        if trace is not None:
            trace.append(dict(kind="deep", taken=e["deep"], margin=abs(e["minz"])))
        steps, ok = 0, 0
        if e["deep"] and math.isfinite(e["F"]):
            ok = 1
            for _ in range(int(iters)):
                det, scale, d = refine.step_of(dict(H=e["H"].tolist(), g=e["g"].tolist()))
                good = math.isfinite(det) and math.isfinite(scale) and det > DET_FLOOR * scale
                if trace is not None:
                    trace.append(dict(kind="det", taken=good, margin=abs(det / scale - DET_FLOOR) / DET_FLOOR if scale != 0 else 0.0))
                if not good:
                    break
                n = [r[c] + d[c] for c in range(3)]
                if not all(math.isfinite(c) for c in n):
                    break
                e2 = evaluate(pose, kps, cams, w, distort, n)
                good = e2["deep"] and e2["F"] <= (1.0 + COST_SLACK) * e["F"]
                if trace is not None:
                    trace.append(dict(kind="deep", taken=e2["deep"], margin=abs(e2["minz"])))
                    trace.append(dict(kind="cost", taken=good, margin=abs(e2["F"] / e["F"] - 1.0 - COST_SLACK) / COST_SLACK, step=max(abs(c) for c in d)))
                if not good:
                    break
                r, e, steps = n, e2, steps + 1
        reproj = np.zeros(V)
        for v, (Ev, Wv) in e["views"].items():
            reproj[v] = float(np.float64(Ev) / np.float64(Wv))
        return np.array(r), reproj, ok, steps


def take_cameras(quat, trans, intr, g, V):
    """per view (R or None, T, intr) of take g from the (G, V, .) tables; quat None: the identity"""
    return [(rotation(None if quat is None else quat[g][v]), np.asarray(trans[g][v], np.float64), np.asarray(intr[g][v], np.float64)) for v in range(V)]


def place_all(pose, kp, quat, trans, intr, valid=None, take_offset=None, weights=None, distort=True, iters=3, trace=None):
    """pose (Ftot, J, 3), kp (V, Ftot, J, 2), tables (G, V, .) -> root (Ftot, 3), reproj (V, Ftot), ok, steps"""
    pose, kp = np.asarray(pose), np.asarray(kp)
    V, ftot = kp.shape[:2]
    off = _offsets(take_offset, ftot)
    root, reproj = np.zeros((ftot, 3)), np.zeros((V, ftot))
    ok, steps = np.zeros(ftot, np.uint8), np.zeros(ftot, np.uint8)
    for f in range(ftot):
        g = _take_of(off, f)
        cams = take_cameras(quat, trans, intr, g, V)
        kps = [kp[v, f] if ((valid is None or valid[v][f]) and cams[v][0] is not None) else None for v in range(V)]
        root[f], reproj[:, f], ok[f], steps[f] = place_frame(pose[f], kps, cams, weights, distort, iters, trace)
    return root, reproj, ok, steps


def margin(trace, kinds=("det0", "deep", "det", "cost")):
    """the smallest relative distance of a decision from its threshold: det / (H00 H11 H22) from 1e-12 in units of 1e-12, a weighted joint's
    Z / |P| from 0, F' / F - 1 from the slack 1e-6 in units of that slack"""
    m = [d["margin"] for d in trace if d["kind"] in kinds]
    return min(m) if m else math.inf


# ---- the scenes of test_gpu_lift_fuse.py, built here so that test_lift_fuse_host.py can check them without a device ---------------------------
def s11_tables(V=4, G=1):
    """(quat (G, V, 4), trans (G, V, 3), intr (G, V, 9)) float32: S11's first V cameras for every take"""
    from manipose_amd.data.ingest import h36m_cameras
    cams = h36m_cameras()["S11"][:V]
    one = [np.stack([np.asarray(c[k], np.float32) for c in cams]) for k in ("orientation", "translation", "intrinsic")]
    return tuple(np.array(np.broadcast_to(t, (G,) + t.shape)) for t in one)                  # (copies: writable)


def fuse_scene(V, K, C, J=17, lens=TAKES, seed=0, with_quat=True):
    """hyps (V, Ftot, K, J, C) float32: per frame one world pose 0.3 N(0, 1), per view rotated into the camera, every hypothesis moved by
    0.05 N(0, 1) per coordinate and every view by an offset of its own (joint 0 is subtracted by the rule); scores uniform in 0.05 .. 1.
    Returns hyps, quat (G, V, 4) or None, take_offset."""
    g = np.random.default_rng(seed)
    ftot, G = int(sum(lens)), len(lens)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    quat = s11_tables(V, G)[0] if with_quat else None
    if quat is not None:
        quat = (quat * g.uniform(0.5, 2.0, (G, V, 1))).astype(np.float32)       # not unit: the rule normalises
    world = 0.3 * g.standard_normal((ftot, J, 3))
    hyps = np.zeros((V, ftot, K, J, C), np.float32)
    for f in range(ftot):
        t = _take_of(off.tolist(), f)
        for v in range(V):
            R = rotation(None if quat is None else quat[t, v])
            cam = world[f] @ R                                                     # R^T p
            hyps[v, f, :, :, :3] = cam + 0.05 * g.standard_normal((K, J, 3)) + g.uniform(-2, 2, (1, 1, 3))
    if C == 4:
        hyps[..., 3] = g.uniform(0.05, 1.0, (V, ftot, K, 1))
    return hyps, quat, off


def valid_table(V, off, seed=0):
    """(V, Ftot) uint8: one view of the whole middle take removed, single frames of single views of the last take removed"""
    g = np.random.default_rng(seed + 77)
    valid = np.ones((V, int(off[-1])), np.uint8)
    valid[V - 1, off[1]:off[2]] = 0
    for f in range(int(off[2]), int(off[3]), 3):
        valid[g.integers(V), f] = 0
    return valid


def place_scene(V, J=17, lens=TAKES, seed=0, noise=0.01):
    """pose (Ftot, J, 3) float32 root-relative in the world, roots x, y in +-1 m, z in 0.8 .. 1.0 m, kp (V, Ftot, J, 2) float32 = the full-model
    projection into S11's cameras plus noise N(0, 1).  Returns pose, kp, root, (quat, trans, intr), take_offset."""
    g = np.random.default_rng(seed)
    ftot, G = int(sum(lens)), len(lens)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    quat, trans, intr = s11_tables(V, G)
    pose = (0.3 * g.standard_normal((ftot, J, 3))).astype(np.float32)
    pose[:, 0] = 0
    root = np.concatenate([g.uniform(-1, 1, (ftot, 2)), g.uniform(0.8, 1.0, (ftot, 1))], axis=1)
    kp = np.zeros((V, ftot, J, 2), np.float32)
    for f in range(ftot):
        t = _take_of(off.tolist(), f)
        for v in range(V):
            kp[v, f] = (project_view(pose[f], root[f], rotation(quat[t, v]), trans[t, v], intr[t, v], True)
                        + noise * g.standard_normal((J, 2))).astype(np.float32)
    return pose, kp, root, (quat, trans, intr), off


WEIGHTS = np.where(np.arange(17) % 5 == 2, 0.0, 0.5 + (np.arange(17) % 3)).astype(np.float32)      # uneven, with zeros
ONE_SPOT, BEHIND, NO_VIEW = 2, 4, 5                     # the frames degenerate_place_scene() spoils


def degenerate_place_scene(V=4):
    """place_scene(V, lens=[8]) with frame ONE_SPOT: all keypoints of all views on one spot; frame BEHIND: a joint 40 m behind camera 0; frame
    NO_VIEW: no valid view.  Returns pose, kp, cams, take_offset, valid."""
    pose, kp, _, cams, off = place_scene(V, lens=[8], seed=21)
    kp[:, ONE_SPOT] = kp[0, ONE_SPOT, 5]
    pose[BEHIND, 5] = (-40.0 * rotation(cams[0][0, 0])[:, 2]).astype(np.float32)
    valid = np.ones((V, 8), np.uint8)
    valid[:, NO_VIEW] = 0
    return pose, kp, cams, off, valid


FUSE_CASES = [(4, 5, 4), (3, 2, 3), (1, 5, 4), (2, 8, 4)]     # (V, K, C)


@functools.lru_cache(maxsize=None)
def fuse_cases():
    """Every comparison scene of mp_lift_fuse and the statement's answer, computed once: list of (tag, hyps, quat, valid, take_offset, want).  Per
    (V, K, C): J = 17 with quaternions and a valid table, J = 17 without either, J = 2 with quaternions, J = 2 without them but with a valid table;
    and (4, 8, 4), all 4096 combinations, on 9 frames alone."""
    cases = []
    for n, (V, K, C) in enumerate(FUSE_CASES):
        for m, (J, with_quat, masked) in enumerate(((17, True, True), (17, False, False), (2, True, False), (2, False, True))):
            hyps, quat, off = fuse_scene(V, K, C, J, seed=10 * n + m, with_quat=with_quat)
            valid = valid_table(V, off, n) if masked else None
            cases.append((f"V={V} K={K} C={C} J={J} quat={int(with_quat)} valid={int(masked)}", hyps, quat, valid, off))
    hyps, quat, off = fuse_scene(4, 8, 4, 17, lens=[9], seed=99)
    cases.append(("V=4 K=8 C=4 J=17 Ftot=9", hyps, quat, None, off))
    return [c + (fuse_all(c[1], c[2], c[3], c[4]),) for c in cases]


@functools.lru_cache(maxsize=None)
def place_cases():
    """Every comparison scene of mp_lift_fuse_place and the statement's answer, computed once: list of (tag, pose, kp, cams, valid, take_offset,
    weights, distort, iters, want, trace): keypoint noise 0.01, iters in {0, 3}, distort in {0, 1}, all views with even weights and a valid table
    with weights that hold zeros."""
    pose, kp, _, cams, off = place_scene(4, seed=5)
    valid = valid_table(4, off, 5)
    cases = []
    for iters in (0, 3):
        for distort in (0, 1):
            for weights, mask in ((None, None), (WEIGHTS, valid)):
                trace = []
                want = place_all(pose, kp, *cams, mask, off, weights, bool(distort), iters, trace)
                cases.append((f"iters={iters} distort={distort} weights={int(weights is not None)} valid={int(mask is not None)}", pose, kp, cams, mask, off,
                              weights, distort, iters, want, trace))
    return cases


def recovery_scene(seed=3, frames=40, K=5, noise=0.0):
    """The scene the feature is for: S11's four cameras, roots x, y in +-1 m, z in 0.8 .. 1.0 m, world poses 0.3 N(0, 1); per view K hypotheses in
    the camera's frame, ONE true to 1 mm (its index drawn per view and frame), the others moved 0.08 N(0, 1) per joint along the camera's depth
    axis plus 5 mm of noise; scores from a Dirichlet draw, in channel 3; keypoints = float32 full-model projections plus noise N(0, 1).
    Returns dict(hyps (4, frames, K, 17, 4), truth (frames, 4), pose (frames, 17, 3) float32, root, kp (4, frames, 17, 2), cams, off)."""
    g = np.random.default_rng(seed)
    V, J = 4, 17
    quat, trans, intr = s11_tables(V, 1)
    pose = (0.3 * g.standard_normal((frames, J, 3))).astype(np.float32)
    pose[:, 0] = 0
    root = np.concatenate([g.uniform(-1, 1, (frames, 2)), g.uniform(0.8, 1.0, (frames, 1))], axis=1).astype(np.float32).astype(np.float64)
    truth = g.integers(K, size=(frames, V))
    hyps = np.zeros((V, frames, K, J, 4), np.float32)
    kp = np.zeros((V, frames, J, 2), np.float32)
    for v in range(V):
        R = rotation(quat[0, v])
        for f in range(frames):
            cam = pose[f].astype(np.float64) @ R
            for k in range(K):
                if k == truth[f, v]:
                    x = cam + 0.001 * g.standard_normal((J, 3))
                else:
                    x = cam + 0.005 * g.standard_normal((J, 3))
                    x[:, 2] += 0.08 * g.standard_normal(J)
                hyps[v, f, k, :, :3] = x
            hyps[v, f, :, :, 3] = g.dirichlet(np.ones(K))[:, None]
            kp[v, f] = (project_view(pose[f], root[f], R, trans[0, v], intr[0, v], True) + noise * g.standard_normal((J, 2))).astype(np.float32)
    return dict(hyps=hyps, truth=truth.astype(np.uint8), pose=pose, root=root, kp=kp, cams=(quat, trans, intr), off=np.array([0, frames], np.int64))

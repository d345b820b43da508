"""numpy float64 statement of placing lifted poses in the scene (manipose_amd/lifting.py: place_poses, to_world; mp_lift_place, mp_lift_world),
shared by test_lift_place_host.py and test_gpu_lift_place.py: the definitions of include/manipose_hip.h, nothing else.  Our own code; the camera
model is the reference's project_to_2d / project_to_2d_linear / qrot restated (tests/golden/place.npz holds the reference's own outputs)."""
import numpy as np

TOL = 2.0 ** -23                                        # per stored number: |x - x64| <= TOL * max(1, |x64|), the final rounding to float32


def within(got, want):
    """the bound every stored float32 is held to against the float64 statement on the same float32 inputs"""
    want = np.asarray(want, np.float64)
    return np.abs(np.asarray(got, np.float64) - want) <= TOL * np.maximum(1.0, np.abs(want))


def worst(got, want):
    want = np.asarray(want, np.float64)
    return float((np.abs(np.asarray(got, np.float64) - want) / np.maximum(1.0, np.abs(want))).max()) / TOL


def project(P, intr, distort=True):
    """pi of include/manipose_hip.h: P (..., 3) camera-space points, intr (9,) -> (..., 2)"""
    P, intr = np.asarray(P, np.float64), np.asarray(intr, np.float64)
    f, c, k, p = intr[0:2], intr[2:4], intr[4:7], intr[7:9]
    with np.errstate(all="ignore"):
        XX = np.clip(P[..., :2] / P[..., 2:3], -1.0, 1.0)
        if not distort:
            return f * XX + c
        r2 = (XX ** 2).sum(-1, keepdims=True)
        radial = 1.0 + (k[0] * r2 + k[1] * r2 ** 2 + k[2] * r2 ** 3)
        tan = (p * XX).sum(-1, keepdims=True)
        return f * (XX * (radial + tan) + p * r2) + c


def fit_sums(pose, kp, intr, w):
    """the seven sums of the normal equations over the joints of non-zero weight, in joint order"""
    fx, fy, cx, cy = (float(v) for v in np.asarray(intr, np.float64)[:4])
    W = A = B = Q = Sx = Sy = Sc = 0.0
    for j in range(pose.shape[0]):
        if w[j] == 0:
            continue
        X, Y, Z = (float(v) for v in pose[j, :3])
        a, b = (float(kp[j, 0]) - cx) / fx, (float(kp[j, 1]) - cy) / fy
        ex, ey = X - a * Z, Y - b * Z
        W += w[j]; A += w[j] * a; B += w[j] * b; Q += w[j] * (a * a + b * b)
        Sx += w[j] * ex; Sy += w[j] * ey; Sc += w[j] * (a * ex + b * ey)
    return W, A, B, Q, Sx, Sy, Sc


def place_one(pose, kp, intr, weights=None, distort=True):
    """one pose (J, C >= 3) and its keypoints (J, 2) -> (t (3,), reproj, ok)"""
    pose, kp = np.asarray(pose, np.float64), np.asarray(kp, np.float64)
    J = pose.shape[0]
    w = np.ones(J) if weights is None else np.asarray(weights, np.float64)
    with np.errstate(all="ignore"):
        W, A, B, Q, Sx, Sy, Sc = sums = fit_sums(pose, kp, intr, w)
        D = W * Q - A * A - B * B
        if not (W > 0 and np.isfinite(sums).all() and D > 1e-9 * (W * Q)):
            return np.zeros(3), 0.0, 0
        tz = (W * Sc - A * Sx - B * Sy) / D
        t = np.array([(A * tz - Sx) / W, (B * tz - Sy) / W, tz])
        keep = w != 0
        Pj = pose[keep, :3] + t
        d = np.sqrt(((project(Pj, intr, distort) - kp[keep]) ** 2).sum(-1))
        err = 0.0
        for wj, dj in zip(w[keep], d):
            err += wj * dj
        return t, err / W, int(bool((Pj[:, 2] > 0).all()))


def place_all(poses, kp, intr, seq_offset=None, weights=None, distort=True):
    """poses (Ntot, J, C) or (Ntot, inner, J, C), kp (Ntot, J, 2), intr (S, 9) -> traj (Ntot[, inner], 3), reproj, ok (uint8) in float64"""
    poses = np.asarray(poses)
    flat = poses[:, None] if poses.ndim == 3 else poses
    intr = np.asarray(intr).reshape(-1, 9)
    off = [0, flat.shape[0]] if seq_offset is None else [int(v) for v in seq_offset]
    traj = np.zeros(flat.shape[:2] + (3,))
    err, ok = np.zeros(flat.shape[:2]), np.zeros(flat.shape[:2], np.uint8)
    for s in range(len(off) - 1):
        for g in range(off[s], off[s + 1]):
            for i in range(flat.shape[1]):
                traj[g, i], err[g, i], ok[g, i] = place_one(flat[g, i], kp[g], intr[s], weights, distort)
    if poses.ndim == 3:
        return traj[:, 0], err[:, 0], ok[:, 0]
    return traj, err, ok


def qrot(q, v):
    """the reference's qrot (data/quaternion.py:6-20): q (4,) = (w, x, y, z), not normalised; v (..., 3)"""
    q, v = np.asarray(q, np.float64), np.asarray(v, np.float64)
    qv = np.broadcast_to(q[1:], v.shape)
    uv = np.cross(qv, v)
    uuv = np.cross(qv, uv)
    return v + 2.0 * (q[0] * uv + uuv)


def world_all(poses, quat, trans=None, traj=None, seq_offset=None):
    """float64 copy of poses (Ntot, J, C) or (Ntot, inner, J, C) with the first three channels p <- qrot(q_s, p + traj) + trans_s"""
    out = np.array(poses, np.float64)
    flat = out[:, None] if out.ndim == 3 else out
    quat = np.asarray(quat, np.float64).reshape(-1, 4)
    off = [0, flat.shape[0]] if seq_offset is None else [int(v) for v in seq_offset]
    for s in range(len(off) - 1):
        p = flat[off[s]:off[s + 1], :, :, :3]
        if traj is not None:
            p = p + np.asarray(traj, np.float64).reshape(flat.shape[:2] + (3,))[off[s]:off[s + 1], :, None, :]
        p = qrot(quat[s], p)
        if trans is not None:
            p = p + np.asarray(trans, np.float64).reshape(-1, 3)[s]
        flat[off[s]:off[s + 1], :, :, :3] = p
    return out


def floor_of(stored, seq_offset=None):
    """(S,) float32: per sequence the minimum z of the STORED float32 poses (Ntot[, inner], J, C)"""
    stored = np.asarray(stored)
    assert stored.dtype == np.float32
    off = [0, stored.shape[0]] if seq_offset is None else [int(v) for v in seq_offset]
    return np.array([stored[off[s]:off[s + 1], ..., 2].min() for s in range(len(off) - 1)], np.float32)


def apply_floor(stored, floor, seq_offset=None):
    """the single float32 subtraction z - floor[s] on a copy of the stored float32 poses"""
    out = np.array(stored, np.float32)
    off = [0, out.shape[0]] if seq_offset is None else [int(v) for v in seq_offset]
    for s in range(len(off) - 1):
        out[off[s]:off[s + 1], ..., 2] = out[off[s]:off[s + 1], ..., 2] - np.float32(floor[s])
    return out


def synthetic_scene(lens, inner, ch, intr, seed, noise=0.01):
    """The construction of the fit tests: poses 0.3 N(0, 1) with the root at 0, true translation x, y in +-1 m and z in 3..7 m, keypoints = the
    pinhole projection of the FIRST inner pose plus noise N(0, 1); everything float32.  intr (S, 9).  Returns poses, kp, t_true, seq_offset."""
    g = np.random.default_rng(seed)
    ntot = int(sum(lens))
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    poses = (0.3 * g.standard_normal((ntot, inner, 17, ch))).astype(np.float32)
    # the further hypotheses of a frame are the first one moved by 0.05 N(0, 1) per coordinate: they share the frame's keypoints, so they have to
    # be poses those keypoints can belong to (unrelated random poses would ask the fit for a depth it cannot have)
    poses[:, 1:, :, :3] = poses[:, :1, :, :3] + (0.05 * g.standard_normal((ntot, inner - 1, 17, 3))).astype(np.float32)
    poses[:, :, 0, :3] = 0
    t = np.concatenate([g.uniform(-1, 1, (ntot, 2)), g.uniform(3, 7, (ntot, 1))], axis=1).astype(np.float32)
    kp = np.zeros((ntot, 17, 2), np.float32)
    for s in range(len(lens)):
        sl = slice(int(off[s]), int(off[s + 1]))
        P = poses[sl, 0, :, :3].astype(np.float64) + t[sl, None, :].astype(np.float64)
        f, c = np.asarray(intr[s], np.float64)[0:2], np.asarray(intr[s], np.float64)[2:4]
        kp[sl] = (f * (P[..., :2] / P[..., 2:3]) + c + noise * g.standard_normal((sl.stop - sl.start, 17, 2))).astype(np.float32)
    return poses, kp, t, off

"""The float64 statement of mp_lift_score (include/manipose_hip.h has the rule), in numpy on the float32 inputs: per sequence and inner index the
counts and sums behind MPJPE, its root mean square, the velocity and acceleration errors, P-MPJPE, per-joint errors and bone-length statistics.
The Procrustes part follows the reference's SVD formulation (oracle/manipose_ref.py: procrustes_align), not the kernel's quaternion form.
Shared by test_lift_score_host.py (which holds it against the oracle's metrics) and test_gpu_lift_score.py; also the inputs of the GPU tests."""
import numpy as np

ROOT_RELATIVE, PROCRUSTES = 1, 2
H36M_PARENTS = (-1, 0, 1, 2, 0, 4, 5, 0, 7, 8, 9, 8, 11, 12, 8, 14, 15)
LENS = (1, 2, 3, 70, 300)                # no pair; one pair, no triple; one triple; longer than a tile; several tiles per share
# (inner, M, C, root_relative) of the GPU test: Procrustes and bones with M = 17 only
GPU_CASES = [(inner, M, C, rr) for inner in (1, 5) for M, C in ((17, 3), (17, 4), (1, 3)) for rr in (False, True)]


def case_id(case):
    return "inner{}-M{}-C{}-{}".format(case[0], case[1], case[2], "rootrel" if case[3] else "abs")


def row_doubles(M):
    return 9 + M + 3 * (M - 1)


def clamp_offsets(off, ntot):
    """[(f0, f1)] of every sequence of an (S + 1) table, clamped as the kernels clamp a device table"""
    out = []
    for s in range(len(off) - 1):
        f0 = min(max(int(off[s]), 0), ntot)
        out.append((f0, min(max(int(off[s + 1]), f0), ntot)))
    return out


def points(x, scale, root_relative):
    """(.., M, C) float32 -> (.., M, 3) float64: scaled, minus joint 0 of the same pose with root_relative"""
    p = np.float64(scale) * x[..., :3].astype(np.float64)
    return p - p[..., :1, :] if root_relative else p


def procrustes_errors(P, G):
    """per-joint errors (M,) after the similarity alignment of P (M, 3) onto G, the reference's SVD form; None: a centred pose is a point"""
    muX, muY = G.mean(0, keepdims=True), P.mean(0, keepdims=True)
    X0, Y0 = G - muX, P - muY
    sx, sy = (X0 ** 2).sum(), (Y0 ** 2).sum()
    if not sx > 0 or not sy > 0:
        return None
    nX, nY = np.sqrt(sx), np.sqrt(sy)
    X0, Y0 = X0 / nX, Y0 / nY
    U, s, Vt = np.linalg.svd(X0.T @ Y0)
    V = Vt.T
    R = V @ U.T
    sign = np.sign(np.linalg.det(R))
    V = V.copy(); s = s.copy()
    V[:, -1] *= sign
    s[-1] *= sign
    R = V @ U.T
    a = s.sum() * nX / nY
    t = muX - a * (muY @ R)
    return np.linalg.norm(a * (P @ R) + t - G, axis=-1)


def horn_gap(P, G):
    """(l1 - l2) / max |l| of the eigenvalues l1 >= l2 >= .. of Horn's 4x4 matrix of the centred poses: what conditions the kernel's eigenvector"""
    X0, Y0 = G - G.mean(0), P - P.mean(0)
    h = Y0.T @ X0
    n = np.array([[h[0, 0] + h[1, 1] + h[2, 2], h[1, 2] - h[2, 1], h[2, 0] - h[0, 2], h[0, 1] - h[1, 0]],
                  [0, h[0, 0] - h[1, 1] - h[2, 2], h[0, 1] + h[1, 0], h[2, 0] + h[0, 2]],
                  [0, 0, -h[0, 0] + h[1, 1] - h[2, 2], h[1, 2] + h[2, 1]],
                  [0, 0, 0, -h[0, 0] - h[1, 1] + h[2, 2]]])
    lam = np.linalg.eigvalsh(n + np.triu(n, 1).T)
    return float((lam[-1] - lam[-2]) / np.abs(lam).max())


def horn_errors(P, G):
    """procrustes_errors by Horn's closed form with numpy's eigensolver (what the kernel does with Jacobi sweeps)"""
    mx, my = G.mean(0), P.mean(0)
    X0, Y0 = G - mx, P - my
    h = Y0.T @ X0
    n = np.array([[h[0, 0] + h[1, 1] + h[2, 2], h[1, 2] - h[2, 1], h[2, 0] - h[0, 2], h[0, 1] - h[1, 0]],
                  [0, h[0, 0] - h[1, 1] - h[2, 2], h[0, 1] + h[1, 0], h[2, 0] + h[0, 2]],
                  [0, 0, -h[0, 0] + h[1, 1] - h[2, 2], h[1, 2] + h[2, 1]],
                  [0, 0, 0, -h[0, 0] - h[1, 1] + h[2, 2]]])
    lam, vec = np.linalg.eigh(n + np.triu(n, 1).T)
    w, x, y, z = vec[:, -1]
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                  [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                  [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
    return np.linalg.norm(lam[-1] / (Y0 ** 2).sum() * (Y0 @ R.T) + mx - G, axis=-1)


def score_rows(pred, gt, off=None, valid=None, parents=None, pred_scale=1.0, gt_scale=1.0, flags=0, frame_fill=-7.0):
    """pred (Ntot, inner, M, C) float32, gt (Ntot, M, 3) float32, off (S + 1) or None (one sequence), valid (Ntot, inner) or None, parents (M) or
    None -> (rows (S, inner, 9 + M + 3 (M - 1)) float64, frame_err (Ntot, inner) float32: -1 for a frame that is not counted, frame_fill for a
    frame that no sequence holds)"""
    ntot, inner, M, _ = pred.shape
    ranges = clamp_offsets([0, ntot] if off is None else off, ntot)
    rr = bool(flags & ROOT_RELATIVE)
    rows = np.zeros((len(ranges), inner, row_doubles(M)))
    frame_err = np.full((ntot, inner), frame_fill, np.float32)
    G = points(gt, gt_scale, rr)
    with np.errstate(invalid="ignore"):
        g_ok = np.isfinite(G).all(axis=(1, 2))
        for i in range(inner):
            P = points(pred[:, i], pred_scale, rr)
            ok = g_ok & np.isfinite(P).all(axis=(1, 2)) & (True if valid is None else valid[:, i] != 0)
            D = P - G
            e = np.sqrt((D ** 2).sum(-1))
            for s, (f0, f1) in enumerate(ranges):
                r = rows[s, i]
                for g in range(f0, f1):
                    if not ok[g]:
                        frame_err[g, i] = -1.0
                        continue
                    frame_err[g, i] = np.float32(e[g].sum() / M)
                    r[0] += 1
                    r[1] += e[g].sum()
                    r[2] += (e[g] ** 2).sum()
                    r[9:9 + M] += e[g]
                    if g - 1 >= f0 and ok[g - 1]:
                        r[3] += 1
                        r[4] += np.linalg.norm((P[g] - P[g - 1]) - (G[g] - G[g - 1]), axis=-1).sum()
                        if g - 2 >= f0 and ok[g - 2]:
                            r[5] += 1
                            r[6] += np.linalg.norm((P[g] - 2 * P[g - 1] + P[g - 2]) - (G[g] - 2 * G[g - 1] + G[g - 2]), axis=-1).sum()
                    if flags & PROCRUSTES:
                        al = procrustes_errors(P[g], G[g])
                        if al is None:
                            r[8] += 1
                        else:
                            r[7] += al.sum()
                    if parents is not None:
                        for b in range(1, M):
                            L = np.linalg.norm(P[g, b] - P[g, parents[b]])
                            LG = np.linalg.norm(G[g, b] - G[g, parents[b]])
                            r[9 + M + 3 * (b - 1):9 + M + 3 * b] += (L, L * L, abs(LG - L))
    return rows, frame_err


def fields(rows, M, procrustes=True):
    """the ratios of score_poses from rows (.., R): a dict; NaN where a count is 0"""
    with np.errstate(invalid="ignore", divide="ignore"):
        n = rows[..., 0]
        ratio = lambda a, b: np.where(b > 0, a / np.where(b > 0, b, 1.0), np.nan)
        out = dict(frames=n, mpjpe=ratio(rows[..., 1], n * M), rmse=np.sqrt(ratio(rows[..., 2], n * M)), mpjve=ratio(rows[..., 4], rows[..., 3] * M),
                   accel=ratio(rows[..., 6], rows[..., 5] * M),
                   p_mpjpe=ratio(rows[..., 7], (n - rows[..., 8]) * M) if procrustes else np.full(n.shape, np.nan),
                   per_joint=ratio(rows[..., 9:9 + M], n[..., None] * np.ones(M)))
        if M > 1:
            b = rows[..., 9 + M:].reshape(*rows.shape[:-1], M - 1, 3)
            cnt = n[..., None] * np.ones(M - 1)
            out["bone_mean"], out["bone_err"] = ratio(b[..., 0], cnt), ratio(b[..., 2], cnt)
            out["bone_std"] = np.sqrt(np.maximum(ratio(b[..., 1], cnt) - out["bone_mean"] ** 2, 0.0))
    return out


# ---- inputs --------------------------------------------------------------------------------------------------------------------------------------
def related_inputs(lens, inner, M, C, seed):
    """"related" poses: gt = 0.3 N(0, 1), pred = 0.9 gt + 0.05 noise (the Procrustes problem is well conditioned: test_lift_score_host.py asserts the
    eigenvalue gap), a random score in channel 3 -> (pred (Ntot, inner, M, C), gt (Ntot, M, 3), off (S + 1) int64)"""
    g = np.random.default_rng(seed)
    ntot = int(sum(lens))
    gt = (0.3 * g.standard_normal((ntot, M, 3))).astype(np.float32)
    pred = np.empty((ntot, inner, M, C), np.float32)
    pred[..., :3] = (0.9 * gt[:, None] + 0.05 * g.standard_normal((ntot, inner, M, 3))).astype(np.float32)
    if C == 4:
        pred[..., 3] = g.random((ntot, inner, M)).astype(np.float32)
    off = np.zeros(len(lens) + 1, np.int64)
    off[1:] = np.cumsum(lens)
    return pred, gt, off


def valid_pattern(off, inner):
    """(Ntot, inner) uint8: in every sequence of at least 60 frames an invalid first and last frame, isolated gaps, a gap of two, and a gap whose
    place depends on the inner index"""
    valid = np.ones((int(off[-1]), inner), np.uint8)
    for f0, f1 in zip(off[:-1], off[1:]):
        if f1 - f0 >= 60:
            for d in (0, 10, 20, 21, 40, int(f1 - f0) - 1):
                valid[f0 + d] = 0
            for i in range(inner):
                valid[f0 + 30 + i, i] = 0
    return valid


def case_inputs(case, seed=5):
    """the inputs of a GPU case: related poses of LENS with a NaN coordinate in two frames of pred and one frame of gt"""
    inner, M, C, rr = case
    pred, gt, off = related_inputs(LENS, inner, M, C, seed + 7 * inner + M + C)
    pred[off[3] + 15, 0, min(3, M - 1), 1] = np.nan
    pred[off[4] + 150, inner - 1, 0, 2] = np.nan                           # (joint 0: root-relative, every joint of the pose is NaN)
    gt[off[4] + 250, min(5, M - 1), 0] = np.nan
    return pred, gt, off


def independence_inputs():
    """(pred, gt, off) of LENS with 5 inner poses, and the same with another last sequence"""
    pred, gt, off = related_inputs(LENS, 5, 17, 4, 31)
    p2, g2, _ = related_inputs(LENS, 5, 17, 4, 32)
    other_p, other_g = pred.copy(), gt.copy()
    other_p[off[-2]:], other_g[off[-2]:] = p2[off[-2]:], g2[off[-2]:]
    return pred, gt, off, other_p, other_g


def similarity_inputs(n=40, seed=51):
    """gt on the grid of multiples of 2^-6 and pred = 2 R gt + t with R a signed permutation (a proper rotation) and t on the grid, per frame: the
    transform is exact in float32, so the aligned error is the rounding of the fp64 alignment alone"""
    g = np.random.default_rng(seed)
    gt = (np.round(0.3 * g.standard_normal((n, 17, 3)) * 64) / 64).astype(np.float32)
    rots = [np.array(r, np.float32) for r in ([[0, -1, 0], [1, 0, 0], [0, 0, 1]], [[1, 0, 0], [0, 0, -1], [0, 1, 0]], [[0, 0, 1], [0, 1, 0], [-1, 0, 0]],
                                              [[0, 1, 0], [0, 0, 1], [1, 0, 0]])]
    pred = np.empty((n, 1, 17, 3), np.float32)
    for f in range(n):
        R = rots[f % 4]
        assert np.linalg.det(R) == 1.0
        t = (np.round(g.standard_normal(3) * 64) / 64).astype(np.float32)
        pred[f, 0] = np.float32(2.0) * (gt[f] @ R.T) + t
    return pred, gt


def constant_bones_inputs(n=24, seed=61):
    """poses whose bones are axis-aligned with lengths on the grid of multiples of 1 / 8, the axis changing from frame to frame, the root moving on the
    grid: every bone has exactly the same length in every frame, and every length, square and sum is exact in fp64 -> (pred, gt, lengths (16))"""
    g = np.random.default_rng(seed)
    lengths = g.integers(1, 5, 16) / 8.0
    axes = np.concatenate([np.eye(3), -np.eye(3)])
    pred = np.zeros((n, 1, 17, 3), np.float32)
    for f in range(n):
        pred[f, 0, 0] = g.integers(-8, 9, 3) / 8.0
        for b in range(1, 17):
            pred[f, 0, b] = pred[f, 0, H36M_PARENTS[b]] + np.float32(lengths[b - 1]) * axes[g.integers(0, 6)].astype(np.float32)
    gt = (0.3 * g.standard_normal((n, 17, 3))).astype(np.float32)
    return pred, gt, lengths


def public_inputs():
    return related_inputs([25, 1, 40], 5, 17, 4, 41)


def procrustes_inputs():
    """(name, pred (Ntot, inner, 17, C), gt) of every input whose slot 7 a GPU test compares with the statement"""
    for case in GPU_CASES:
        if case[1] == 17:
            pred, gt, _ = case_inputs(case)
            yield case_id(case), pred, gt
    pred, gt, _, other_p, other_g = independence_inputs()
    yield "independence", pred, gt
    yield "independence, other last sequence", other_p, other_g
    yield "similarity", *similarity_inputs()
    yield "public", *public_inputs()[:2]

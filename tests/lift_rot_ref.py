"""Joint rotations of lifted poses: the float64 numpy statement of mp_lift_rotations' rule (include/manipose_hip.h), written from the rule and not
from the kernel - world rotations are 3 x 3 matrices here, the kernel carries unit quaternions - with the decoder-convention forward kinematics for
quaternions and for 6-D rotations (the closure: fk(ik(p), measured lengths) == p), the continuity rule, and the scenes the GPU tests run.

Every scene builder prints and asserts its DECISION MARGINS, so that fp64 contraction differences between the kernel and numpy cannot flip a
branch: 1 + rest . u >= 1e-3 on every regular joint, the root frame's |d_b - (d_b . f1) f1| >= 1e-3, the root quaternion's leading component
>= 1e-3, and |dot(c[g], c[g-1])| >= 1e-3 on every consecutive pair of stored quaternions.  The constructed cases (exact_scene) are exact in binary
arithmetic instead: every product and quotient in them is exact or a single correctly rounded operation, so both sides take the same branch and
store the same bits."""
import numpy as np

MARGIN = 1e-3
LENS = (1, 2, 67, 130)          # a single frame, a pair, and the 64-frame chunk boundary with a carry, twice
TOL = 2.0 ** -23                # one unit in the last place of 1.0: both sides round the same real number, known to about 1e-13, to float32

H36M_PARENTS = (-1, 0, 1, 2, 0, 4, 5, 0, 7, 8, 9, 8, 11, 12, 8, 14, 15)
H36M_REST = np.array([(0, 0, 0), (1, 0, 0), (0, -1, 0), (0, -1, 0), (-1, 0, 0), (0, -1, 0), (0, -1, 0), (0, 1, 0), (0, 1, 0), (0, 1, 0), (0, 1, 0),
                      (-1, 0, 0), (-1, 0, 0), (-1, 0, 0), (1, 0, 0), (1, 0, 0), (1, 0, 0)], np.float32)


class Sk:
    """what pose_rotations takes as a skeleton: parents and t_pose_operators (a {joint: direction} table, the root has none)"""

    def __init__(self, parents, rest):
        self.parents = np.asarray(parents)
        self.t_pose_operators = {j: np.asarray(rest[j], np.float32) for j in range(1, len(parents))}


def skeleton(kind):
    """(parents, rest (J, 3) float32): "h36m" (J = 17), "pair" (J = 2, no second reference bone) and "chain" (J = 32, depth 31, T-pose directions
    of any length in any direction)"""
    if kind == "h36m":
        return H36M_PARENTS, H36M_REST.copy()
    if kind == "pair":
        return (-1, 0), np.array([(0, 0, 0), (0.0, 0.6, 0.8)], np.float32)
    if kind == "chain":
        g = np.random.default_rng(32)
        rest = g.uniform(-2.0, 2.0, (32, 3)).astype(np.float32)
        rest[0] = 0
        return (-1,) + tuple(range(31)), rest
    raise ValueError(kind)


def _canon(v):
    """v / |v| with the sign that makes the first non-zero component positive; rows of (..., n)"""
    v = np.asarray(v, np.float64)
    nz = v != 0
    first = np.argmax(nz, axis=-1)
    lead = np.take_along_axis(v, first[..., None], axis=-1)[..., 0]
    n = np.sqrt((v * v).sum(-1))
    return v / np.where(lead < 0, -n, n)[..., None]


def tables(parents, rest):
    """what the entry point derives on the host: unit rest directions, the root's reference children a and b (-1: none), the T-pose frame E (rows
    e1, e2, e3) and every joint's half-turn axis"""
    parents = [int(p) for p in parents]
    J = len(parents)
    r = np.zeros((J, 3))
    r[1:] = np.asarray(rest, np.float64)[1:]
    assert np.isfinite(r).all() and (np.abs(r[1:]).sum(-1) > 0).all()
    r[1:] /= np.sqrt((r[1:] ** 2).sum(-1))[:, None]
    kids = [j for j in range(1, J) if parents[j] == 0]
    a = kids[0]
    b = next((j for j in kids[1:] if np.sqrt((np.cross(r[a], r[j]) ** 2).sum()) > 1e-6), -1)
    E = np.zeros((3, 3))
    E[0] = r[a]
    if b >= 0:
        t = r[b] - (r[b] @ r[a]) * r[a]
        E[1] = t / np.sqrt((t * t).sum())
        E[2] = np.cross(E[0], E[1])
    piax = np.zeros((J, 3))
    for j in range(1, J):
        k = int(np.argmin(np.abs(r[j])))                               # the lowest index on a tie
        piax[j] = _canon(np.eye(3)[k] - r[j, k] * r[j])
    return dict(parents=parents, rest=r, a=a, b=b, E=E, piax=piax, J=J)


def _arc(r, u, pi):
    """(q (N, 4), regular (N,)) of the shortest arc r -> u, rows; a half turn about pi where 1 + r . u < 1e-12"""
    w = 1.0 + (r * u).sum(-1)
    c = np.cross(r, u)
    n = np.sqrt(w * w + (c * c).sum(-1))
    with np.errstate(all="ignore"):
        q = np.concatenate([w[:, None], c], axis=-1) / n[:, None]
    half = w < 1e-12
    q[half] = np.concatenate([np.zeros((int(half.sum()), 1)), np.broadcast_to(pi, (len(w), 3))[half]], axis=-1)
    return q, ~half, w


def matrix(q):
    """(..., 3, 3) rotation matrices of unit quaternions (w, x, y, z)"""
    w, x, y, z = (q[..., i] for i in range(4))
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], -1),
                     np.stack([2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)], -1),
                     np.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1)], -2)


def quat_of(m):
    """unit quaternions of (N, 3, 3) rotation matrices from the largest of 4w^2, 4x^2, 4y^2, 4z^2 (the first on a tie), canonical sign"""
    t = np.stack([1 + m[:, 0, 0] + m[:, 1, 1] + m[:, 2, 2], 1 + m[:, 0, 0] - m[:, 1, 1] - m[:, 2, 2], 1 - m[:, 0, 0] + m[:, 1, 1] - m[:, 2, 2],
                  1 - m[:, 0, 0] - m[:, 1, 1] + m[:, 2, 2]], -1)
    k = np.argmax(t, axis=-1)
    with np.errstate(all="ignore"):
        s = 2.0 * np.sqrt(np.take_along_axis(t, k[:, None], -1)[:, 0])
        a, b, c = (m[:, 2, 1] - m[:, 1, 2]) / s, (m[:, 0, 2] - m[:, 2, 0]) / s, (m[:, 1, 0] - m[:, 0, 1]) / s
        d, e, f = (m[:, 0, 1] + m[:, 1, 0]) / s, (m[:, 0, 2] + m[:, 2, 0]) / s, (m[:, 1, 2] + m[:, 2, 1]) / s
    h = 0.25 * s
    forms = np.stack([np.stack([h, a, b, c], -1), np.stack([a, h, d, e], -1), np.stack([b, d, h, f], -1), np.stack([c, e, f, h], -1)], 1)
    return _canon(forms[np.arange(len(m)), k])


def ik(poses, parents, rest):
    """The rule, steps 1-4, on (..., J, C >= 3) poses: dict of quat (..., J, 4) and rot6d (..., J, 6) float64, ok (...) uint8, and the margins of the
    decisions taken: arc (the least 1 + rest . u over regular joints), frame (the least |d_b - (d_b . f1) f1| over full root frames), lead (the
    least leading component of a full root frame's quaternion)"""
    tb = tables(parents, rest)
    J, par, r = tb["J"], tb["parents"], tb["rest"]
    x = np.asarray(poses)
    lead_shape = x.shape[:-2]
    P = x[..., :3].astype(np.float64).reshape(-1, J, 3)
    N = len(P)
    fin = np.isfinite(P).all(-1)
    bad_pose = ~fin.all(-1)
    ident = np.tile(np.array([1.0, 0, 0, 0]), (N, 1))
    pidx = [0] + par[1:]
    with np.errstate(all="ignore"):
        bone = P - P[:, pidx]
        n = np.sqrt((bone * bone).sum(-1))
        good = fin & fin[:, pidx] & (n > 1e-12)
        good[:, 0] = False
        d = np.where(good[..., None], bone / n[..., None], 0.0)
        a, b = tb["a"], tb["b"]
        da, ga = d[:, a], good[:, a]
        db, gb = (d[:, b], good[:, b]) if b >= 0 else (np.zeros((N, 3)), np.zeros(N, bool))
        t = db - (db * da).sum(-1)[:, None] * da
        tn = np.sqrt((t * t).sum(-1))
        full = ga & gb & (tn > 1e-9)
        f2 = t / tn[:, None]
        f3 = np.cross(da, f2)
        M = da[:, :, None] * tb["E"][0] + f2[:, :, None] * tb["E"][1] + f3[:, :, None] * tb["E"][2]
        M = np.where(full[:, None, None], M, np.eye(3))
        q_full = quat_of(M)
        q_arc, arc_ok, _ = _arc(np.broadcast_to(tb["E"][0], (N, 3)), np.where(ga[:, None], da, tb["E"][0]), tb["piax"][a])
    q = np.tile(ident[:, None], (1, J, 1))
    q[:, 0] = np.where(full[:, None], q_full, np.where(ga[:, None], q_arc, ident))
    regular = np.ones((N, J), bool)
    regular[:, 0] = np.where(full, True, ga & arc_ok & (b < 0))
    Rw = np.zeros((N, J, 3, 3))
    Rw[:, 0] = matrix(q[:, 0])
    arc_pose = np.full(N, np.inf)                                      # per pose: the least 1 + rest . u over its regular joints
    for j in range(1, J):
        Rp = Rw[:, par[j]]
        u = np.einsum("nrc,nr->nc", Rp, d[:, j])                       # Rw[parent]^T d_j
        u = np.where(good[:, j, None], u, r[j])
        qj, reg, w = _arc(np.broadcast_to(r[j], (N, 3)), u, tb["piax"][j])
        q[:, j] = np.where(good[:, j, None], qj, ident)
        regular[:, j] = good[:, j] & reg
        Rw[:, j] = Rp @ matrix(q[:, j])
        arc_pose = np.where(regular[:, j] & ~bad_pose, np.minimum(arc_pose, w), arc_pose)
    q[bad_pose] = ident[0]
    q = q + 0.0                                                        # a zero component is +0
    ok = (regular.all(-1) & ~bad_pose).astype(np.uint8)
    R = matrix(q)
    rot6d = np.concatenate([R[..., :, 0], R[..., :, 1]], axis=-1) + 0.0
    use = full & ~bad_pose
    frame_pose, lead_pose = np.where(use, tn, np.inf), np.where(use, np.abs(q[:, 0, 0]), np.inf)
    return dict(quat=q.reshape(lead_shape + (J, 4)), rot6d=rot6d.reshape(lead_shape + (J, 6)), ok=ok.reshape(lead_shape),
                arc=float(arc_pose.min()), frame=float(frame_pose.min()), lead=float(lead_pose.min()),
                per_pose=np.minimum(np.minimum(arc_pose, frame_pose), lead_pose).reshape(lead_shape))


def measured_lengths(poses, parents):
    """(..., J - 1) float64 bone lengths of every pose"""
    P = np.asarray(poses)[..., :3].astype(np.float64)
    par = [int(p) for p in parents]
    return np.sqrt(((P[..., 1:, :] - P[..., par[1:], :]) ** 2).sum(-1))


def fk(R, lengths, parents, rest, root=None):
    """The decoder's forward kinematics: Rw[0] = R[0], Rw[j] = Rw[parent] R[j], p[j] = p[parent] + Rw[j] (len_j rest_j), rest_j the unit T-pose
    direction; R (..., J, 3, 3) local matrices, lengths (..., J - 1), root (..., 3) or None (0) -> (..., J, 3) float64"""
    tb = tables(parents, rest)
    J, par, r = tb["J"], tb["parents"], tb["rest"]
    R = np.asarray(R, np.float64)
    L = np.broadcast_to(np.asarray(lengths, np.float64), R.shape[:-3] + (J - 1,))
    Rw, p = [R[..., 0, :, :]], [np.zeros(R.shape[:-3] + (3,)) if root is None else np.asarray(root, np.float64)]
    for j in range(1, J):
        Rw.append(Rw[par[j]] @ R[..., j, :, :])
        p.append(p[par[j]] + np.einsum("...rc,...c->...r", Rw[j], L[..., j - 1, None] * r[j]))
    return np.stack(p, axis=-2)


def fk_quat(quat, lengths, parents, rest, root=None):
    return fk(matrix(np.asarray(quat, np.float64)), lengths, parents, rest, root)


def ortho6d(r6):
    """compute_rotation_matrix_from_ortho6d: x = unit(a), z = unit(x x b), y = z x x, columns x | y | z"""
    r6 = np.asarray(r6, np.float64)
    x = r6[..., :3] / np.sqrt((r6[..., :3] ** 2).sum(-1))[..., None]
    z = np.cross(x, r6[..., 3:])
    z = z / np.sqrt((z * z).sum(-1))[..., None]
    return np.stack([x, np.cross(z, x), z], axis=-1)


def fk_rot6d(rot6d, lengths, parents, rest, root=None):
    return fk(ortho6d(rot6d), lengths, parents, rest, root)


def continuity(c32, off=None):
    """Step 5 on stored float32 quaternions c32 (Ntot, inner, J, 4): (the signed float32 quaternions, the flips (Ntot, inner, J) bool, the least
    |dot| of a consecutive pair).  flip[g] = flip[g-1] XOR (dot(c[g], c[g-1]) < 0) is the parity of the votes up to g: a cumulative sum mod 2."""
    c32 = np.asarray(c32, np.float32)
    ntot = c32.shape[0]
    off = [0, ntot] if off is None else [int(v) for v in off]
    flips = np.zeros(c32.shape[:-1], bool)
    least = np.inf
    for s in range(len(off) - 1):
        f0 = min(max(off[s], 0), ntot)
        f1 = min(max(off[s + 1], f0), ntot)
        if f1 - f0 < 2:
            continue
        c = c32[f0:f1].astype(np.float64)
        dots = (c[1:] * c[:-1]).sum(-1)
        least = min(least, float(np.abs(dots).min()))
        flips[f0 + 1:f1] = np.cumsum(dots < 0, axis=0) % 2 == 1
    return np.where(flips[..., None], -c32, c32), flips, least


def rotations(poses, parents, rest, off=None, continuous=True):
    """what mp_lift_rotations stores, as float64 / uint8 arrays, and the margins: (quat, rot6d, ok, flips, margins); quat is the float32-rounded
    canonical quaternion with its continuity sign, widened again"""
    r = ik(poses, parents, rest)
    shape = r["quat"].shape
    c32 = r["quat"].astype(np.float32).reshape((shape[0], -1) + shape[-2:])
    if continuous:
        q32, flips, dot = continuity(c32, off)
    else:
        q32, flips, dot = c32, np.zeros(c32.shape[:-1], bool), np.inf
    return q32.reshape(shape).astype(np.float64), r["rot6d"], r["ok"], flips.reshape(shape[:-1]), dict(arc=r["arc"], frame=r["frame"], lead=r["lead"], dot=dot)


def check_margins(tag, m, need_frame=True):
    print(f"[margins] {tag}: 1 + rest . u >= {m['arc']:.3e}, root frame |t| >= {m['frame']:.3e}, root leading component >= {m['lead']:.3e}, "
          f"|dot| of consecutive stored quaternions >= {m['dot']:.3e} (each needs {MARGIN:g})")
    assert m["arc"] >= MARGIN and m["dot"] >= MARGIN, tag
    assert (m["frame"] >= MARGIN and m["lead"] >= MARGIN) or not need_frame, tag


# ---- scenes ----------------------------------------------------------------------------------------------------------------------------------
def _random_rotations(g, shape, max_angle):
    axis = g.standard_normal(shape + (3,))
    axis /= np.sqrt((axis * axis).sum(-1))[..., None]
    half = 0.5 * g.uniform(0, max_angle, shape)
    return np.concatenate([np.cos(half)[..., None], np.sin(half)[..., None] * axis], axis=-1)


def _draw(g, n, inner, parents, rest):
    """n frames x inner poses by forward kinematics: any root orientation, local rotations up to 150 degrees (with twist: the inverse returns its
    own, twist-free ones), every pose its own bone lengths in 0.1 .. 0.5 and its own root position: float32 (n, inner, J, 3)"""
    J = len(parents)
    q = _random_rotations(g, (n, inner, J), np.deg2rad(150.0))
    q[:, :, 0] = _random_rotations(g, (n, inner), np.pi)
    L = g.uniform(0.1, 0.5, (n, inner, J - 1))
    root = g.uniform(-1.0, 1.0, (n, inner, 3)) + np.array([0, 0, 4.0])
    return fk_quat(q, L, parents, rest, root).astype(np.float32)


def random_scene(kind="h36m", inner=1, C=3, seed=0, lens=LENS):
    """(poses (Ntot, inner, J, C) float32, off (S + 1) int64, parents, rest): random poses, frame by frame unrelated (so consecutive stored
    quaternions lie in either hemisphere: the continuity pass flips about half of them), with every frame whose decisions come nearer than MARGIN
    to a threshold drawn again; channel 3 (C = 4) is a random score.  The margins are printed and asserted."""
    parents, rest = skeleton(kind)
    g = np.random.default_rng(seed)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    ntot = int(off[-1])
    P = _draw(g, ntot, inner, parents, rest)
    for _ in range(50):
        redo = np.zeros(ntot, bool)
        r = ik(P, parents, rest)
        c = r["quat"].astype(np.float32).astype(np.float64)
        redo |= (r["per_pose"] < 2 * MARGIN).any(axis=1) | ~r["ok"].all(axis=1)      # a decision of one of the frame's poses too near its threshold
        for s in range(len(lens)):
            f0, f1 = int(off[s]), int(off[s + 1])
            if f1 - f0 >= 2:
                near = (np.abs((c[f0 + 1:f1] * c[f0:f1 - 1]).sum(-1)) < 2 * MARGIN).any(axis=(1, 2))
                redo[f0 + 1:f1] |= near
        if not redo.any():
            break
        P[redo] = _draw(g, int(redo.sum()), inner, parents, rest)
    assert not redo.any()
    if C == 4:
        P = np.concatenate([P, g.uniform(0, 1, P.shape[:-1] + (1,)).astype(np.float32)], axis=-1)
    return np.ascontiguousarray(P), off, parents, rest


def rigid_h36m_poses(n, seed=5):
    """n random H36M poses on ONE table of bone lengths, float64 (for the fp64 round trip), and the table"""
    g = np.random.default_rng(seed)
    L = g.uniform(0.1, 0.5, 16)
    q = _random_rotations(g, (n, 17), np.deg2rad(150.0))
    q[:, 0] = _random_rotations(g, (n,), np.pi)
    return fk_quat(q, L, H36M_PARENTS, H36M_REST, g.uniform(-1, 1, (n, 3))), L


# (skeleton, inner, C) of the random scenes the GPU tests run and the host tests take the margins of
SCENES = [("h36m", 1, 3), ("h36m", 1, 4), ("h36m", 5, 3), ("h36m", 5, 4), ("pair", 5, 3), ("pair", 1, 4), ("chain", 1, 3), ("chain", 5, 4)]
T_POSE, HALF_TURN, ZERO_BONE, NAN_COORD, COLLINEAR = range(5)


def exact_scene():
    """(poses (5, 1, 17, 3) float32, expected quat (5, 1, 17, 4), rot6d, ok) on the H36M tree, every number a small multiple of a power of two:
    T_POSE: the T-pose with bones of 0.5 (all identities, ok = 1); HALF_TURN: the right knee's bone exactly opposite its T-pose direction under an
    identity parent (q[2] = (0, 1, 0, 0), the ankle following: identity); ZERO_BONE: the left knee on the left hip; NAN_COORD: a NaN in one
    coordinate; COLLINEAR: the spine along the right hip's bone (root: the arc of the hip alone, the identity; the spine's own arc is a quarter
    turn, 1 / sqrt(2) once on both sides; everything above the spine sits on it).  ok = 0 on the last four."""
    tb = tables(H36M_PARENTS, H36M_REST)
    ident = np.zeros((17, 4))
    ident[:, 0] = 1
    base = fk_quat(ident, 0.5, H36M_PARENTS, H36M_REST)
    P = np.tile(base, (5, 1, 1))
    want = np.tile(ident, (5, 1, 1))
    P[HALF_TURN, 2] = P[HALF_TURN, 1] + [0, 0.5, 0]
    P[HALF_TURN, 3] = P[HALF_TURN, 2] + [0, 0.5, 0]
    want[HALF_TURN, 2] = [0, 1, 0, 0]
    P[ZERO_BONE, 5] = P[ZERO_BONE, 4]
    P[ZERO_BONE, 6] = P[ZERO_BONE, 5] + [0, -0.5, 0]
    P[NAN_COORD, 9, 1] = np.nan
    P[COLLINEAR, 7:] = [0.25, 0, 0]
    h = 1.0 / np.sqrt(2.0)
    want[COLLINEAR, 7] = [h, 0, 0, -h]
    poses = P.astype(np.float32)[:, None]
    assert np.array_equal(poses.astype(np.float64)[:, 0][np.isfinite(P)], P[np.isfinite(P)])
    r = ik(poses, H36M_PARENTS, H36M_REST)
    assert np.array_equal(r["quat"][:, 0], want) and r["ok"][:, 0].tolist() == [1, 0, 0, 0, 0]       # the statement on its own constructed cases
    assert np.array_equal(tb["piax"][2], [1, 0, 0])
    return poses, r["quat"], r["rot6d"], r["ok"]


def alternating_scene(n=70):
    """(poses (n, 1, 17, 3) float32, off): the T-pose with bones of 0.5 turned about z by +170 and -170 degrees in turn: 20 degrees apart, but the
    canonical root quaternions (cos 85, 0, 0, +-sin 85) alternate hemisphere, dot = cos 170 < 0 on every pair: every odd frame is flipped."""
    ident = np.zeros((n, 17, 4))
    ident[:, :, 0] = 1
    ang = np.deg2rad(170.0) * np.where(np.arange(n) % 2 == 0, 1.0, -1.0)
    ident[:, 0] = np.stack([np.cos(ang / 2), 0 * ang, 0 * ang, np.sin(ang / 2)], -1)
    P = fk_quat(ident, 0.5, H36M_PARENTS, H36M_REST).astype(np.float32)[:, None]
    return np.ascontiguousarray(P), np.array([0, n], np.int64)

"""Euler channels of a take's joint rotations and their continuity in time: the float64 numpy statement of mp_lift_euler's rule
(include/manipose_hip.h), written from the header's text and not from the kernels - poses are walked by explicit loops, the continuity is a
SEQUENTIAL walk over a track's frames that looks back for its predecessor (the kernel votes in a wave and takes prefix scans) - with an independent
BVH READER written from the format (HIERARCHY and MOTION parsed, R_i R_j R_k composed per node in the listed channel order, the nodes walked to
positions), the scenes and the cases the GPU tests run.

What lets a float32 bound stand: the first pass is a few fp64 operations on float32 inputs, asin and atan2 included, whose library differences of
about 1e-16 are amplified by at most 1 / sqrt(c2); ``euler`` returns the least c2 of a regular joint, the least distance of a canonical angle from
its branch cut, and ``continuity`` the least margins of its two decisions, and test_lift_euler_host.py asserts them on every case."""
import functools

import numpy as np

import lift_retime_ref as rt
import lift_rot_ref as rot

ORDERS = ("XYZ", "XZY", "YXZ", "YZX", "ZXY", "ZYX")
AXES = {"XYZ": (0, 1, 2), "XZY": (0, 2, 1), "YXZ": (1, 0, 2), "YZX": (1, 2, 0), "ZXY": (2, 0, 1), "ZYX": (2, 1, 0)}
DEG = 57.29577951308232         # the double nearest to 180 / pi
LENS = (1, 2, 3, 67, 130)       # a single frame, a pair, a triple, a chunk border inside a sequence, and one past 128 frames
CONTINUOUS = 1


def sign_of(order):
    i, j, _ = AXES[order]
    return 1.0 if (j - i) % 3 == 1 else -1.0


def usable(q):
    """n2 = |q|^2 (summed w, x, y, z) finite and >= 1e-12, rows of (..., 4) float64"""
    with np.errstate(all="ignore"):
        n2 = ((q[..., 0] * q[..., 0] + q[..., 1] * q[..., 1]) + q[..., 2] * q[..., 2]) + q[..., 3] * q[..., 3]
    return np.isfinite(n2) & (n2 >= 1e-12), n2


def axis_matrix(axis, angle):
    """R_axis(angle), angle in radians"""
    c, s = np.cos(angle), np.sin(angle)
    a, b = (axis + 1) % 3, (axis + 2) % 3
    R = np.eye(3)
    R[a, a], R[a, b], R[b, a], R[b, b] = c, -s, s, c
    return R


def compose(order, angles_deg):
    """R_i(al) R_j(be) R_k(ga) of one triple in degrees"""
    i, j, k = AXES[order]
    al, be, ga = (np.deg2rad(float(v)) for v in angles_deg)
    return axis_matrix(i, al) @ axis_matrix(j, be) @ axis_matrix(k, ga)


def angles_of(R, order, m=None):
    """(al, be, ga) in RADIANS of one matrix and whether it is the gimbal case; m collects the margins of a regular joint"""
    i, j, k = AXES[order]
    s = sign_of(order)
    c2 = R[j][k] * R[j][k] + R[k][k] * R[k][k]
    be = np.arcsin(min(max(s * R[i][k], -1.0), 1.0))
    if c2 >= 1e-12:
        al, ga = np.arctan2(-s * R[j][k], R[k][k]), np.arctan2(-s * R[i][j], R[i][i])
        if m is not None:
            m["c2"] = min(m["c2"], float(c2))
            m["cut"] = min(m["cut"], 180.0 - abs(np.rad2deg(al)), 180.0 - abs(np.rad2deg(ga)))
        return (al, be, ga), False
    return (np.arctan2(s * R[k][j], R[j][j]), be, 0.0), True


def qrot_matrix(u, v):
    return rot.matrix(u) @ v


def euler(quat, root, valid, off, basis, shift, scale, order):
    """The FIRST PASS on float32 quat (Ntot, inner, J, 4): dict(angles (Ntot, inner, J, 3) float64 degrees BEFORE the final rounding, pos
    (Ntot, inner, 3) float64 or None, ok (Ntot, inner) uint8, margins).  root (Ntot, inner, 3) float32 or None, valid (Ntot, inner) or None, off
    (S + 1), basis (S, 4) and shift (S, 3) float32 or both None."""
    q = np.asarray(quat, np.float32).astype(np.float64)
    ntot, inner, J = q.shape[:3]
    angles, ok = np.zeros((ntot, inner, J, 3)), np.zeros((ntot, inner), np.uint8)
    pos = None if root is None else np.zeros((ntot, inner, 3))
    m = dict(c2=np.inf, cut=np.inf)
    for g in range(ntot):
        s = rt.seq_of(off, g)
        B, t, basis_ok = np.array([1.0, 0.0, 0.0, 0.0]), np.zeros(3), True
        if basis is not None:
            b = np.asarray(basis, np.float32)[s].astype(np.float64)
            good, n2 = usable(b)
            basis_ok = bool(good)
            if basis_ok:
                B = b / np.sqrt(n2)
            t = np.asarray(shift, np.float32)[s].astype(np.float64)
        for i in range(inner):
            good, n2 = usable(q[g, i])
            if not good.all() or not basis_ok or (valid is not None and valid[g, i] == 0):
                continue
            u = q[g, i] / np.sqrt(n2)[:, None]
            u[0] = rt.qmul(B, u[0])
            M = rot.matrix(u)
            code = 1
            for j in range(J):
                (al, be, ga), gimbal = angles_of(M[j], order, m)
                angles[g, i, j] = (al * DEG + 0.0, be * DEG + 0.0, ga * DEG + 0.0)
                code |= 2 if gimbal else 0
            ok[g, i] = code
            if root is not None:
                pos[g, i] = float(np.float32(scale)) * (qrot_matrix(B, np.asarray(root, np.float32)[g, i].astype(np.float64)) + t) + 0.0
    return dict(angles=angles, pos=pos, ok=ok, margins=m)


# ---- the continuity ----------------------------------------------------------------------------------------------------------------------------
def other(x):
    """T(x): the other Euler solution of the same rotation"""
    return np.array([x[0] + 180.0, 180.0 - x[1], x[2] + 180.0])


def wrap(x):
    return x - 360.0 * np.floor((x + 180.0) / 360.0)


def dist(x, y):
    return (abs(wrap(x[0] - y[0])) + abs(wrap(x[1] - y[1]))) + abs(wrap(x[2] - y[2]))


def frames_of(off, s, ntot):
    f0 = min(max(int(off[s]), 0), ntot)
    return f0, min(max(int(off[s + 1]), f0), ntot)


def continuity(c32, ok, off, m=None):
    """The SECOND PASS on the stored float32 angles c32 (Ntot, inner, J, 3) and ok (Ntot, inner): the float32 array the pass leaves.  A sequential
    walk: every frame with a result looks at the last frame before it that has one, its stored triple, its branch and its turns (the kernel votes
    in a wave and takes prefix scans).  m collects the least |d(c, T(c')) - d(c, c')| of the branch comparison and the least distance of a turn
    count from a tie."""
    c = np.asarray(c32, np.float32)
    out = c.copy()
    ntot, inner, J = c.shape[:3]
    for s in range(len(off) - 1):
        f0, f1 = frames_of(off, s, ntot)
        for i in range(inner):
            for j in range(J):
                prev = None                                               # (c[g'], flip[g'], e[g'], W[g'])
                for g in range(f0, f1):
                    if ok[g, i] == 0:
                        continue
                    x = c[g, i, j].astype(np.float64)
                    if prev is None:
                        flip, e, W = False, x, np.zeros(3)
                    else:
                        pc, pflip, pe, pW = prev
                        d_other, d_same = dist(x, other(pc)), dist(x, pc)
                        flip = pflip != (d_other < d_same)
                        e = other(x) if flip else x
                        turns = (e - pe) / 360.0
                        W = pW - np.rint(turns)
                        if m is not None:
                            m["branch"] = min(m["branch"], abs(d_other - d_same))
                            m["turn"] = min(m["turn"], float(np.abs(np.abs(turns - np.floor(turns)) - 0.5).min()))
                    out[g, i, j] = (e + 360.0 * W).astype(np.float32) + np.float32(0.0)
                    prev = (x, flip, e, W)
    return out


def greedy(c32, ok, off):
    """the same pass as the walk an animator would write: of the two solutions of a frame, the one nearer (by d) to WHAT WAS CHOSEN for the frame
    before, then the multiple of 360 degrees per channel that brings it nearest; float64, before the final rounding.  The header's prefix parity is
    this walk wherever the branch comparison is no tie (d is unchanged when T is applied to both its arguments)."""
    c = np.asarray(c32, np.float32).astype(np.float64)
    out = c.copy()
    ntot, inner, J = c.shape[:3]
    for s in range(len(off) - 1):
        f0, f1 = frames_of(off, s, ntot)
        for i in range(inner):
            for j in range(J):
                chosen, before = None, None                               # the chosen solution of the frame before, without and with its turns
                for g in range(f0, f1):
                    if ok[g, i] == 0:
                        continue
                    x = c[g, i, j]
                    if chosen is None:
                        chosen, before = x, x
                    else:
                        e = other(x) if dist(other(x), chosen) < dist(x, chosen) else x
                        full = e + 360.0 * np.rint((before - e) / 360.0)
                        chosen, before = e, full
                    out[g, i, j] = before
    return out


def solve(quat, root, valid, off, basis, shift, scale, order, flags):
    """both passes: euler's record with ``stored`` (float32, what the device leaves) and, for flags = CONTINUOUS, the margins of the walk"""
    r = euler(quat, root, valid, off, basis, shift, scale, order)
    canon = r["angles"].astype(np.float32) + np.float32(0.0)       # (a -0 the rounding made is +0)
    r["canonical"] = canon
    r["margins"].update(branch=np.inf, turn=np.inf)
    r["stored"] = continuity(canon, r["ok"], off, r["margins"]) if flags & CONTINUOUS else canon
    return r


# ---- an independent BVH reader --------------------------------------------------------------------------------------------------------------------
def read_bvh(path):
    """dict(nodes [name, parent, offset, channels, end], frames M, frame_time, motion (M, channels)) of a BVH file, parsed token by token"""
    tok = open(path).read().split()
    assert tok[0] == "HIERARCHY"
    nodes, stack, p = [], [], 1
    while tok[p] != "MOTION":
        if tok[p] in ("ROOT", "JOINT"):
            nodes.append(dict(name=tok[p + 1], parent=stack[-1] if stack else -1, offset=None, channels=[], end=None))
            cur, p = len(nodes) - 1, p + 2
            assert tok[p] == "{"
            stack.append(cur)
            p += 1
        elif tok[p] == "OFFSET":
            nodes[stack[-1]]["offset"] = [float(v) for v in tok[p + 1:p + 4]]
            p += 4
        elif tok[p] == "CHANNELS":
            n = int(tok[p + 1])
            nodes[stack[-1]]["channels"] = tok[p + 2:p + 2 + n]
            p += 2 + n
        elif tok[p] == "End":
            assert tok[p + 1] == "Site" and tok[p + 2] == "{" and tok[p + 3] == "OFFSET" and tok[p + 7] == "}"
            nodes[stack[-1]]["end"] = [float(v) for v in tok[p + 4:p + 7]]
            p += 8
        else:
            assert tok[p] == "}", tok[p]
            stack.pop()
            p += 1
    assert not stack and tok[p + 1] == "Frames:" and tok[p + 3] == "Frame" and tok[p + 4] == "Time:"
    M, frame_time = int(tok[p + 2]), float(tok[p + 5])
    width = sum(len(n["channels"]) for n in nodes)
    motion = np.array([float(v) for v in tok[p + 6:]]).reshape(M, width)
    return dict(nodes=nodes, frames=M, frame_time=frame_time, motion=motion)


def bvh_positions(parsed):
    """(node positions (M, N, 3), end-site positions (M, N, 3), NaN where a node has none) by walking the hierarchy: a node's world rotation is its
    parent's times the product of its rotation channels in the listed order, its position its parent's plus the parent's rotation of its OFFSET"""
    nodes, motion = parsed["nodes"], parsed["motion"]
    M, N = motion.shape[0], len(nodes)
    P, E = np.zeros((M, N, 3)), np.full((M, N, 3), np.nan)
    for f in range(M):
        col, W = 0, [None] * N
        for k, n in enumerate(nodes):
            R, t = np.eye(3), np.zeros(3)
            for ch in n["channels"]:
                v = motion[f, col]
                col += 1
                if ch.endswith("position"):
                    t["XYZ".index(ch[0])] = v
                else:
                    assert ch.endswith("rotation")
                    R = R @ axis_matrix("XYZ".index(ch[0]), np.deg2rad(v))
            if n["parent"] < 0:
                P[f, k], W[k] = np.asarray(n["offset"]) + t, R
            else:
                P[f, k], W[k] = P[f, n["parent"]] + W[n["parent"]] @ (np.asarray(n["offset"]) + t), W[n["parent"]] @ R
            if n["end"] is not None:
                E[f, k] = P[f, k] + W[k] @ np.asarray(n["end"])
    return P, E


def bvh_joints(parsed, parents):
    """the decoder's J joint positions (M, J, 3) from a bone-centred file: joint 0 is the root node; joint j >= 1 the child end of bone j's node -
    where a child node of it sits, or its End Site.  The file lists the nodes depth first; bone j's node is found by its place in that order."""
    parents = [int(p) for p in parents]
    J = len(parents)
    order, stack = [], [0]                                               # the depth-first order of the bones, children in increasing index
    while stack:
        j = stack.pop()
        order.append(j)
        stack.extend(sorted((k for k in range(1, J) if parents[k] == j), reverse=True))
    at = {j: n for n, j in enumerate(order)}
    P, E = bvh_positions(parsed)
    out = np.zeros((P.shape[0], J, 3))
    out[:, 0] = P[:, 0]
    for j in range(1, J):
        kids = [k for k in range(1, J) if parents[k] == j]
        out[:, j] = P[:, at[kids[0]]] if kids else E[:, at[j]]
        assert parsed["nodes"][at[j]]["parent"] == at[parents[j]]
    return out


# ---- scenes and cases -------------------------------------------------------------------------------------------------------------------------------
def take(kind, inner, lens=LENS, seed=0, holes=True, speed=0.25):
    """A take of big smooth motion: every joint spins about a slowly wobbling axis at up to ``speed`` radians a frame, so that within a sequence
    the canonical angles cross their branch cuts, the middle angle passes +-90 degrees and whole turns pile up.  float32 quat (Ntot, inner, J, 4)
    off the unit sphere (norms 0.5 .. 2), root (Ntot, inner, 3), valid (Ntot, inner) with single holes and a run, or None."""
    parents, rest = rot.skeleton(kind)
    J, ntot = len(parents), sum(lens)
    g = np.random.default_rng(1000 * seed + 10 * J + inner)
    q = np.zeros((ntot, inner, J, 4))
    f0 = 0
    for n in lens:
        t = np.arange(n, dtype=np.float64)[:, None, None]
        axis = g.standard_normal((1, inner, J, 3)) + 0.4 * np.sin(0.05 * t[..., None] + g.uniform(0, 6, (1, inner, J, 3)))
        axis /= np.sqrt((axis * axis).sum(-1))[..., None]
        ang = g.uniform(0, 6, (1, inner, J)) + g.uniform(-speed, speed, (1, inner, J)) * t + 0.5 * np.sin(g.uniform(0.02, 0.1, (1, inner, J)) * t)
        start = rot._random_rotations(g, (1, inner, J), np.pi)
        q[f0:f0 + n] = rt.qmul(np.broadcast_to(start, (n, inner, J, 4)), rt.qexp(ang[..., None] * axis))
        f0 += n
    q = (q * g.uniform(0.5, 2.0, (ntot, inner, J, 1))).astype(np.float32)
    root = (g.uniform(-1, 1, (ntot, inner, 3)) + [0, 0, 1.0]).astype(np.float32)
    valid = None
    if holes:
        valid = (g.uniform(size=(ntot, inner)) > 0.1).astype(np.uint8)
        valid[sum(lens[:3]) + 60:sum(lens[:3]) + 66] = 0                  # a run across the 64-frame chunk border of the fourth sequence
    for a in (q, root) + (() if valid is None else (valid,)):
        a.setflags(write=False)
    return dict(quat=q, root=root, valid=valid, lens=tuple(lens), parents=parents, rest=rest, off=np.concatenate([[0], np.cumsum(lens)]).astype(np.int64))


def transform(S, seed):
    """(basis (S, 4) float32 off the unit sphere, shift (S, 3) float32)"""
    g = np.random.default_rng(77 + seed)
    basis = (rot._random_rotations(g, (S,), np.pi) * g.uniform(0.5, 2.0, (S, 1))).astype(np.float32)
    return basis, g.uniform(-2, 2, (S, 3)).astype(np.float32)


def cases():
    """(id, kind, inner, order, with_basis, with_root, with_valid, scale): all six orders, J 17 / 2 / 32, inner 1 / 5, every optional input on and off"""
    rows = [("h36m", 1, "ZXY", True, True, True, 100.0), ("h36m", 5, "XYZ", True, True, True, 1.0), ("h36m", 5, "ZYX", False, False, False, 1.0),
            ("h36m", 1, "YZX", False, True, False, 100.0), ("pair", 5, "XZY", True, False, True, 1.0), ("pair", 1, "YXZ", False, True, True, 100.0),
            ("chain", 1, "ZXY", True, True, False, 1.0), ("chain", 5, "YXZ", False, False, True, 100.0), ("h36m", 1, "XZY", True, True, True, 1.0),
            ("pair", 5, "ZYX", True, True, False, 100.0), ("chain", 1, "XYZ", False, True, True, 1.0), ("pair", 1, "YZX", True, False, False, 1.0)]
    return [(f"{k}-i{i}-{o}-{'b' if b else 'nob'}-{'r' if r else 'nor'}-{'v' if v else 'nov'}-s{int(sc)}", k, i, o, b, r, v, sc) for k, i, o, b, r, v, sc in rows]


@functools.lru_cache(maxsize=None)
def scene_of(cid):
    """the inputs of a case: (take, basis, shift) - what is switched off is None"""
    _, kind, inner, order, with_basis, with_root, with_valid, scale = next(c for c in cases() if c[0] == cid)
    sc = dict(take(kind, inner, seed=ORDERS.index(order) + 3, holes=with_valid))
    if not with_root:
        sc["root"] = None
    basis, shift = transform(len(LENS), ORDERS.index(order)) if with_basis else (None, None)
    return sc, basis, shift


@functools.lru_cache(maxsize=None)
def solved(cid, flags=CONTINUOUS):
    _, kind, inner, order, with_basis, with_root, with_valid, scale = next(c for c in cases() if c[0] == cid)
    sc, basis, shift = scene_of(cid)
    return solve(sc["quat"], sc["root"], sc["valid"], sc["off"], basis, shift, scale, order, flags)


def exact_scene():
    """Constructed frames whose arithmetic is exact in binary - the matrices of these quaternions hold 0, +-1 alone: exact gimbal poses (the
    permutation matrices of (+-1/2, +-1/2, +-1/2, +-1/2) and quarter-free half turns), half turns about the axes, the identity, a zero quaternion,
    a NaN, and an invalid frame between two frames that flip.  One sequence of J = 2 joints, inner 1: (quat (N, 1, 2, 4), valid (N, 1), off)."""
    h = 0.5
    rows = [(1, 0, 0, 0), (0, 1, 0, 0), (h, h, h, h), (0, 0, 0, 0), (h, -h, h, h), (np.nan, 0, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1), (h, h, -h, h),
            (0, 0, 0, 2), (1, 0, 0, 0), (h, h, h, -h), (0, 3, 0, 0), (-h, h, h, h), (0, 0, 1, 0), (1, 0, 0, 0)]
    N = len(rows)
    q = np.zeros((N, 1, 2, 4), np.float32)
    q[:, 0, 1] = np.array(rows, np.float32)
    q[:, 0, 0] = np.roll(np.array(rows, np.float32), -1, axis=0)           # joint 0: the same poses a frame early ...
    q[2, 0, 0] = q[4, 0, 0] = (1, 0, 0, 0)                                # ... without the bad ones: joint 1 alone decides frames 3 and 5
    valid = np.ones((N, 1), np.uint8)
    valid[7] = 0                                                          # an invalid frame between the half turns about y and about x
    return q, valid, np.array([0, N], np.int64)


# ---- the closure through a file ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def closure_take(n=130, seed=21):
    """One H36M sequence of moderate motion (at most 0.03 radians a frame and joint, so the continuous angles stay within a turn or two: a float32
    angle in degrees is known to half an ulp, 1.5e-5 degrees below 512 and more beyond), with holes, a root and a bone table"""
    sc = dict(take("h36m", 1, (n,), seed=seed, holes=True, speed=0.03))
    sc["bones"] = np.random.default_rng(seed).uniform(0.1, 0.5, 16).astype(np.float32)
    return sc


def named_h36m():
    """a skeleton as bvh_hierarchy takes it: parents, t_pose_operators and joints_names"""
    sk = rot.Sk(rot.H36M_PARENTS, rot.H36M_REST)
    sk.joints_names = ["Hip", "RHip", "RKnee", "RFoot", "LHip", "LKnee", "LFoot", "Spine", "Thorax", "Neck/Nose", "Head", "LShoulder", "LElbow", "LWrist",
                       "RShoulder", "RElbow", "RWrist"]
    return sk


def moved(p, basis, shift, scale):
    """scale (qrot(unit(basis), p) + shift) of float64 points (..., 3); basis (4,) and shift (3,) float32 or None"""
    p = np.asarray(p, np.float64)
    if basis is not None:
        b = np.asarray(basis, np.float32).astype(np.float64)
        p = p @ rot.matrix(b / np.sqrt((b * b).sum())).T + np.asarray(shift, np.float32).astype(np.float64)
    return float(np.float32(scale)) * p


def closure_bound(want, scale):
    """4 x the float32 rounding error of the positions compared against (the largest |float32(p) - p|), floor 1e-7 m x scale: mp_lift_fk's bound"""
    return max(4.0 * float(np.abs(want.astype(np.float32).astype(np.float64) - want).max()), 1e-7 * float(scale))


def row_sources(live):
    """the frame whose row every frame of a written file holds: itself where it has a result, else the last one before it that has one, the first
    one that has one for the leading frames"""
    idx = np.flatnonzero(live)
    src, last = np.zeros(len(live), np.int64), int(idx[0])
    for g in range(len(live)):
        if live[g]:
            last = g
        src[g] = last
    return src


def format_bound(angles32, parents, bones, scale, node_eps=0.0):
    """How far the float32 DEGREES of a file may move a joint, from the number format alone: a stored angle is known to half a float32 ulp, so node
    b's rotation is off by at most eps_b = sum over its three channels of ulp(angle) / 2 in radians (plus ``node_eps``), which moves joint j below
    it by at most eps_b times the length of the tree path from the joint the node sits at to j.  Returns the largest such sum over the frames and
    joints, times ``scale``: (M, J, 3) float32 angles, bone table (J - 1,)."""
    parents = [int(p) for p in parents]
    J = len(parents)
    L = np.asarray(bones, np.float64)
    eps = (np.spacing(np.abs(np.asarray(angles32, np.float32))).astype(np.float64) / 2.0 * np.pi / 180.0).sum(-1) + node_eps      # (M, J)
    worst = 0.0
    for j in range(1, J):
        path, k = [], j
        while k != 0:
            path.append(k)
            k = parents[k]
        path = path[::-1]                                                 # the bones from the root down to j
        below = np.cumsum([L[b - 1] for b in path][::-1])[::-1]           # path length from the joint bone b's node sits at down to j
        moved = eps[:, 0] * below[0] + sum(eps[:, b] * below[n] for n, b in enumerate(path))      # (node 0 and the first bone's node both sit at the root)
        worst = max(worst, float(moved.max()))
    return float(scale) * worst

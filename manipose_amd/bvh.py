"""A lifted take written as a BVH file: host code only; numpy, which the whole package stands on, is its one import outside the standard library.

The hierarchy is BONE-CENTRED, which is what makes the mapping from the decoder's per-bone convention exact.  The decoder's forward kinematics is
Rw[j] = Rw[parent] q[j], p[j] = p[parent] + len_j Rw[j] rest_j: the rotation q[j] belongs to the BONE parent -> j and turns about the PARENT joint.
So every bone j >= 1 gets a node N_j that sits at the parent joint (its OFFSET from N_parent(j) is len_parent(j) rest_parent(j), zero where
parent(j) = 0), carries exactly q[j], and has its child end len_j rest_j away (a leaf bone: its ``End Site``); the root node N_0 carries the root
position and q[0]; the children of joint j hang under N_j.  Then W(N_j) = W(N_parent(j)) q[j] = Rw[j] and every joint comes out where
``pose_from_rotations`` puts it - no approximation and no twist estimate.  Several nodes share a position (the root and its children's bones at
the pelvis), which is valid BVH: importers know such "dummy" joints.  The angles come from ``euler_from_rotations`` (mp_lift_euler).

Not built: a joint-centred hierarchy with renamed joints, a twist estimate, reading BVH, other formats."""
from __future__ import annotations

import re

import numpy as np

ORDERS = ("XYZ", "XZY", "YXZ", "YZX", "ZXY", "ZYX")


def _num(v):
    """a number with 9 significant digits: the float32 nearest to it reads back as itself"""
    return "%.9g" % float(v)


def _rest_rows(skeleton, J):
    ops = getattr(skeleton, "t_pose_operators", None)
    if ops is None:
        raise ValueError("a BVH hierarchy needs the skeleton's t_pose_operators: the T-pose direction of every bone")
    rest = np.zeros((J, 3))
    for j in range(1, J):
        v = ops[j]
        v = np.asarray(v.tolist() if hasattr(v, "tolist") else v, np.float32).astype(np.float64)      # (as the entry points read them: float32)
        n = float(np.sqrt((v * v).sum()))
        if v.shape != (3,) or not np.isfinite(n) or n == 0:
            raise ValueError(f"t_pose_operators[{j}] must be a finite direction that is not zero")
        rest[j] = v / n
    return rest


def bvh_hierarchy(skeleton, bones, scale=1.0):
    """The bone-centred node list of ``skeleton`` (``parents``, ``t_pose_operators``, ``joints_names``) with the bone table ``bones`` (J - 1,), in
    units of ``scale`` (100: centimetres of a table in metres): a list of J dicts, node j the node of bone j (node 0: the root) - ``name``,
    ``parent`` (a node index, -1 for the root), ``joint`` (the joint the node sits at), ``offset`` (3 floats, from the parent node), ``end`` (3
    floats, the leaf bone's End Site, or None) and ``children`` (node indices).  Names: the joint a node sits at names it (``joints_names``, "J<k>"
    where the skeleton has none), with the child joint's name appended after "_" where a joint carries more than one node; whitespace becomes "_";
    ValueError where the names are not unique."""
    parents = [int(p) for p in skeleton.parents]
    J = len(parents)
    if J < 2 or parents[0] != -1 or any(not 0 <= p < j for j, p in enumerate(parents) if j):
        raise ValueError("a BVH hierarchy needs a tree of at least 2 joints: joint 0 the root, parents before their children")
    L = np.asarray(bones.tolist() if hasattr(bones, "tolist") else bones, np.float64)
    if L.shape != (J - 1,) or not np.isfinite(L).all() or (L < 0).any():
        raise ValueError(f"bones must be {J - 1} finite lengths >= 0 (one bone table: a take's), got shape {L.shape}")
    if isinstance(scale, bool) or not isinstance(scale, (int, float, np.integer, np.floating)) or not 0 < float(scale) < float("inf"):
        raise ValueError(f"scale must be a finite number > 0, got {scale!r}")
    rest = _rest_rows(skeleton, J)
    given = list(getattr(skeleton, "joints_names", None) or [""] * J)
    base = [re.sub(r"\s+", "_", str(given[k]).strip()) or f"J{k}" for k in range(J)]
    sits = [0] + [parents[j] for j in range(1, J)]                         # the joint node j sits at
    load = [sum(1 for k in range(J) if sits[k] == p) for p in range(J)]   # nodes a joint carries
    bone = lambda j: float(scale) * L[j - 1] * rest[j]
    nodes = []
    for j in range(J):
        name = base[sits[j]] if j == 0 or load[sits[j]] == 1 else f"{base[sits[j]]}_{base[j]}"
        kids = [k for k in range(1, J) if parents[k] == j]
        offset = np.zeros(3) if j == 0 or parents[j] == 0 else bone(parents[j])
        nodes.append(dict(name=name, parent=-1 if j == 0 else parents[j], joint=sits[j], offset=[float(v) for v in offset],
                          end=None if j == 0 or kids else [float(v) for v in bone(j)], children=kids))
    names = [n["name"] for n in nodes]
    if len(set(names)) != J:
        raise ValueError(f"the BVH node names are not unique: {sorted(n for n in set(names) if names.count(n) > 1)}; give the skeleton unique joints_names")
    return nodes


def _walk(nodes):
    """the nodes in the file's order (depth first, children in increasing index)"""
    order, stack = [], [0]
    while stack:
        j = stack.pop()
        order.append(j)
        stack.extend(reversed(nodes[j]["children"]))
    return order


def write_bvh(path, skeleton, bones, angles, pos, ok, fps, order="ZXY", scale=1.0):
    """Write ``path`` as BVH: HIERARCHY (``bvh_hierarchy(skeleton, bones, scale)``) and MOTION.  ``angles`` (M, J, 3) degrees in channel order and
    ``pos`` (M, 3) (None: the origin) as ``euler_from_rotations(..., order=order, scale=scale)`` returns them, ``ok`` (M,) (None: every frame),
    arrays or host tensors; ``fps`` > 0, ``Frame Time`` is 1 / fps.  The root has the channels Xposition Yposition Zposition and the three
    rotations in ``order``; every other node the three rotations.  Every number is written with 9 significant digits, so its float32 value reads
    back.  A frame with ok = 0 repeats the last frame before it that has a result; leading ones repeat the first frame with a result.  A take
    without such a frame writes no file.  Returns whether the file was written."""
    if not isinstance(order, str) or order not in ORDERS:
        raise ValueError(f"order must be one of {list(ORDERS)}, got {order!r}")
    if isinstance(fps, bool) or not isinstance(fps, (int, float, np.integer, np.floating)) or not 0 < float(fps) < float("inf"):
        raise ValueError(f"fps must be a finite number > 0, got {fps!r}")
    nodes = bvh_hierarchy(skeleton, bones, scale)
    J = len(nodes)
    host = lambda a: np.asarray(a.detach().cpu().numpy() if hasattr(a, "detach") else a)
    A = host(angles)
    if A.ndim != 3 or A.shape[1:] != (J, 3) or A.dtype.kind != "f":
        raise ValueError(f"angles must be (M, {J}, 3) floats, got shape {A.shape} {A.dtype}")
    M = A.shape[0]
    P = np.zeros((M, 3), np.float32) if pos is None else host(pos)
    if P.shape != (M, 3) or P.dtype.kind != "f":
        raise ValueError(f"pos must be ({M}, 3) floats, got shape {P.shape} {P.dtype}")
    K = np.ones(M, np.uint8) if ok is None else host(ok)
    if K.shape != (M,):
        raise ValueError(f"ok must be ({M},), got shape {K.shape}")
    live = np.flatnonzero(K != 0)
    if live.size == 0:
        return False
    src = np.empty(M, np.int64)                                           # the frame whose row a frame writes
    last = int(live[0])
    for g in range(M):
        if K[g] != 0:
            last = g
        src[g] = last
    rot = " ".join(f"{c}rotation" for c in order)
    lines = ["HIERARCHY"]

    def emit(j, depth):
        n, pad = nodes[j], "\t" * depth
        lines.append(f"{pad}{'ROOT' if j == 0 else 'JOINT'} {n['name']}")
        lines.append(pad + "{")
        lines.append(f"{pad}\tOFFSET {' '.join(_num(v) for v in n['offset'])}")
        lines.append(f"{pad}\tCHANNELS 6 Xposition Yposition Zposition {rot}" if j == 0 else f"{pad}\tCHANNELS 3 {rot}")
        for k in n["children"]:
            emit(k, depth + 1)
        if n["end"] is not None:
            lines.extend([f"{pad}\tEnd Site", pad + "\t{", f"{pad}\t\tOFFSET {' '.join(_num(v) for v in n['end'])}", pad + "\t}"])
        lines.append(pad + "}")

    emit(0, 0)
    cols = _walk(nodes)
    lines += ["MOTION", f"Frames: {M}", f"Frame Time: {_num(1.0 / float(fps))}"]
    for g in range(M):
        f = int(src[g])
        lines.append(" ".join([_num(v) for v in P[f]] + [_num(v) for j in cols for v in A[f, j]]))
    with open(path, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    return True

"""numpy float64 statement of rigid lifting (manipose_amd/lifting.py: project_rigid, mp_lift_rigid, mp_bone_length_means), shared by
test_lift_rigid_host.py and test_gpu_lift_rigid.py.  Our own code: the reference has no counterpart."""
import numpy as np

PARENTS = (-1, 0, 1, 2, 0, 4, 5, 0, 7, 8, 9, 8, 11, 12, 8, 14, 15)        # the 17-joint H36M tree (c_parent of csrc/fk_decode.hip)
BONES_LEFT, BONES_RIGHT = (3, 4, 5, 10, 11, 12), (0, 1, 2, 13, 14, 15)      # Skeleton.bones_left / bones_right of that tree


def project(p, L, parents=PARENTS):
    """One pose p (J, 3) with the bone lengths L (J - 1): the root and every bone direction kept, bone j - 1 = (j, parents[j]) of length
    L[j - 1]; a bone of length zero (or non-finite length) takes the direction of its parent's bone, (0, 0, 1) under the root."""
    p = np.asarray(p, np.float64)
    J = p.shape[0]
    q, u = np.zeros((J, 3)), np.zeros((J, 3))
    q[0] = p[0]
    for j in range(1, J):
        d = p[j] - p[parents[j]]
        n = np.sqrt(d @ d)
        if n > 0 and np.isfinite(n):
            u[j] = d / n
        else:
            u[j] = u[parents[j]] if parents[j] != 0 else (0.0, 0.0, 1.0)
        q[j] = q[parents[j]] + float(L[j - 1]) * u[j]
    return q


def project_all(poses, lengths, seq_offset, parents=PARENTS):
    """poses (Ntot, J, 3) or (Ntot, inner, J, C >= 3), lengths (S, J - 1), seq_offset (S + 1): float64 copy with the first three channels of
    every pose projected with the row of its frame's sequence; further channels untouched."""
    out = np.array(poses, np.float64)
    flat = out.reshape(out.shape[0], -1, out.shape[-2], out.shape[-1])
    for s in range(len(seq_offset) - 1):
        for g in range(int(seq_offset[s]), int(seq_offset[s + 1])):
            for i in range(flat.shape[1]):
                flat[g, i, :, :3] = project(flat[g, i, :, :3], lengths[s], parents)
    return out


def bone_lengths(poses, parents=PARENTS):
    """(..., J, C >= 3) -> (..., J - 1) in float64."""
    p = np.asarray(poses, np.float64)[..., :3]
    return np.linalg.norm(p[..., 1:, :] - p[..., list(parents[1:]), :], axis=-1)


def mean_bone_lengths(poses, seq_offset, real=None, parents=PARENTS):
    """(S, J - 1): per sequence the mean over its (first real[s]) frames of the bone lengths of poses (Ntot, J, 3)."""
    bl = bone_lengths(poses, parents)
    rows = []
    for s in range(len(seq_offset) - 1):
        a = int(seq_offset[s])
        b = a + int(real[s]) if real is not None else int(seq_offset[s + 1])
        rows.append(bl[a:b].mean(axis=0))
    return np.stack(rows)


def symmetrise(L):
    L = np.array(L, np.float64)
    m = (L[..., list(BONES_LEFT)] + L[..., list(BONES_RIGHT)]) / 2
    L[..., list(BONES_LEFT)] = m
    L[..., list(BONES_RIGHT)] = m
    return L

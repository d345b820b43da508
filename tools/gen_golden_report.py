"""Generates tests/golden/report.npz by running the reference's own report metrics - ``segments_max_strech_per_bone``,
``segments_max_diff_strech_per_bone`` (metrics/regularizations.py:63-94), ``coordwise_error``, ``jointwise_mse``, ``jointwise_error``
(metrics/mean_joint_errors.py:47-141) and ``mean_velocity_error(axis=1)`` (metrics/losses.py:75-101) - on seeded (prediction, target) pairs
in millimetres, with both call patterns of hpe/main_h36m_lifting.py:934-1089: on the (B, 3, J, L) tensor and on its (1, 3, J, B*L)
reshape.  Also stores ``joints_names`` / ``bones_names`` of the reference's 17-joint H36M skeleton.  Data only.

    python tools/gen_golden_report.py          (where oracle/gen_golden.py finds the reference)

Input sets (B, L) = (3, 5) and (2, 130).  Every bone gets one planted jump - from a frame of the bone's own on, its child joint and the whole subtree below it
are pushed along the bone by 40 mm + 3 mm * bone - so that its largest frame-to-frame difference lies
far above the next one (asserted here: by more than 1 mm in float64) (the poses move by about 1 mm per frame) and the arg-max does not hang on rounding."""
import copy
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import gen_golden  # noqa: E402

PARENTS = (-1, 0, 1, 2, 0, 4, 5, 0, 7, 8, 9, 8, 11, 12, 8, 14, 15)
SETS = ((3, 5), (2, 130))


def subtree(j):
    out = [j]
    for c, p in enumerate(PARENTS):
        if p == j:
            out += subtree(c)
    return out


def make_pair(B, L, seed):
    """A smooth random pose sequence in mm (a base pose plus a slow drift), a target near it, and one planted jump per bone."""
    g = np.random.default_rng(seed)
    base = 250.0 * g.standard_normal((1, 1, 17, 3))
    drift = np.cumsum(1.0 * g.standard_normal((B, L, 17, 3)), axis=1)
    pred = (base + 5.0 * g.standard_normal((B, 1, 17, 3)) + drift).astype(np.float64)
    pred[:, :, 0] = 0.0
    gt = pred + 20.0 * g.standard_normal(pred.shape)
    for k in range(16):
        j, p = k + 1, PARENTS[k + 1]
        b, t = k % B, 1 + (7 * k + 3) % (L - 1)              # the bone is longer from frame t of item b on, in the later items too: ONE
        flat = pred.reshape(B * L, 17, 3)                    # large difference, t-1 -> t, in the windows and in the flattened sequence
        d = flat[b * L + t:, j] - flat[b * L + t:, p]         # (frames, 3)
        push = (40.0 + 3.0 * k) * d / np.linalg.norm(d, axis=-1, keepdims=True)
        for q in subtree(j):
            flat[b * L + t:, q] += push
    # a 1/4 mm grid: exact in float32, and the file stays below 100 KB
    return (np.round(4.0 * pred) / 4.0).astype(np.float32), (np.round(4.0 * gt) / 4.0).astype(np.float32)


def assert_gap(x, what):
    """every bone's largest |difference| stands at least 1 mm above its second largest (float64 from the float32 inputs)"""
    x = x.double()
    for k in range(16):
        d = (x[:, :, k + 1] - x[:, :, PARENTS[k + 1]]).pow(2).sum(1).sqrt().diff(dim=-1).abs().reshape(-1).sort(descending=True)[0]
        assert d[0] - d[1] > 1.0, (what, k, d[:3])


def main():
    ref = gen_golden.import_reference()
    M = ref["M"]
    from mh_so3_hpe.data.h36m_lifting import h36m_skeleton
    sk17 = copy.deepcopy(h36m_skeleton)                      # Human36mDataset(n_joints=17), h36m_lifting.py:649-660
    sk17.remove_joints([4, 5, 9, 10, 11, 16, 20, 21, 22, 23, 24, 28, 29, 30, 31])
    sk17._parents[11] = 8
    sk17._parents[14] = 8
    sk17._compute_metadata()
    assert tuple(int(p) for p in sk17.parents) == PARENTS
    out = {"joints_names": np.array(list(sk17.joints_names)), "bones_names": np.array(list(sk17.bones_names)),
           "bones_left": np.array(sk17.bones_left, dtype=np.int64), "bones_right": np.array(sk17.bones_right, dtype=np.int64),
           "sets": np.array(SETS, dtype=np.int64)}
    sk = ref["sk"]
    for i, (B, L) in enumerate(SETS):
        pred, gt = make_pair(B, L, seed=40 + i)
        p, y = torch.from_numpy(pred), torch.from_numpy(gt)               # (B, L, J, 3) in mm
        gen = p.permute(0, 3, 2, 1)                                      # (B, 3, J, L), main_h36m_lifting.py:935-937
        flat = gen.permute(1, 2, 0, 3).reshape(1, 3, 17, -1)             # (1, 3, J, B*L), :1062-1063
        out[f"pred.{i}"], out[f"gt.{i}"] = pred, gt
        for tag, x in (("win", gen), ("seq", flat)):
            assert_gap(x, (tag, i))
            mn, mx = M.segments_max_strech_per_bone(joints_coords=x, skeleton=sk)
            dv, di = M.segments_max_diff_strech_per_bone(joints_coords=x, skeleton=sk)
            out[f"min_len.{tag}.{i}"], out[f"max_len.{tag}.{i}"] = mn.numpy(), mx.numpy()
            out[f"max_delta.{tag}.{i}"], out[f"max_delta_idx.{tag}.{i}"] = dv.numpy(), di.numpy().astype(np.int64)
        out[f"cw_err.{i}"] = M.coordwise_error(gen.permute(0, 3, 2, 1), y, "average").numpy()
        out[f"cw_sum.{i}"] = M.coordwise_error(gen.permute(0, 3, 2, 1), y, "sum").numpy()
        out[f"mvjpe.{i}"] = np.float32(M.mean_velocity_error(predicted=gen.permute(0, 3, 2, 1), target=y, squared=False, axis=1).item())
        out[f"jw_mse.{i}"] = M.jointwise_mse(gen.permute(0, 3, 2, 1), y, "average").numpy()
        out[f"jw_err.{i}"] = M.jointwise_error(gen.permute(0, 3, 2, 1), y, "average").numpy()
    path = os.path.join(ROOT, "tests", "golden", "report.npz")
    np.savez_compressed(path, **out)
    print("report: ok", os.path.getsize(path), "bytes", {k: out[k].tolist() for k in ("max_delta_idx.win.1", "max_delta_idx.seq.1")})


if __name__ == "__main__":
    main()

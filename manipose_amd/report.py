"""The files of the reference's test pass (hpe/main_h36m_lifting.py:840-1186, hpe/main_3dhp.py:769-988), written from the per-group results
of ``hpe/_entry.py:evaluate(analytics=True)``.  Host only: plain ``csv`` / numpy, no device work and no pandas.

The reference builds every table as a numpy array and writes it with ``pd.DataFrame(value).to_csv(path, header=head, index=False)``
(save_csv_log, main_h36m_lifting.py:54-72); the layout here is that one - a header line, one line per row, "," as the separator, "\\n" line
ends, minimal quoting - so ``pd.read_csv(path, index_col=0)`` reads the files the way the reference's useful_aux_scripts/ do.

H36M (one row per action and a last row "average" of column means): protocol_1_err.csv, seg_symmetry.csv, seg_consistency.csv,
seg_max_strech.csv, seg_max_delta_strech.csv, cw_err.csv, jw_err.csv, all_seg_errs.npy, all_jw_err_var.npy.
3DHP (one row, no row label): seg_symmetry.csv, seg_consistency.csv, cw_err.csv, jw_err.csv.
all_pred_hyps.pkl and the mlflow calls of the reference are not reproduced.
run.hyp_report (no file of the reference: it does this study in follow-up scripts on the pickle): hyp_report.csv, hyp_heads.csv, hyp_joints.csv
from ``HypothesisAccumulator.report()`` (write_hypothesis_report).
run.lift with lift.score (no file of the reference: it never scores a lifted sequence): lift_score.csv, lift_score_joints.csv from the score dicts
of ``lift_sequences(targets=..., return_score=True)`` (write_lift_score_report)."""
from __future__ import annotations

import csv
import os
from typing import Dict, List, Mapping, Optional, Sequence

import numpy as np

# the 17 joints of the reduced H36M skeleton (the reference's h36m_lifting.py names after remove_joints; dataset_3dhp.py uses the same);
# pinned to the reference's by tests/golden/report.npz
H36M_JOINTS_NAMES = ("Hip", "RHip", "RKnee", "RFoot", "LHip", "LKnee", "LFoot", "Spine", "Thorax", "Neck/Nose", "Head", "LShoulder", "LElbow",
                     "LWrist", "RShoulder", "RElbow", "RWrist")
_PARENTS = (-1, 0, 1, 2, 0, 4, 5, 0, 7, 8, 9, 8, 11, 12, 8, 14, 15)
BONES_LEFT, BONES_RIGHT = (3, 4, 5, 10, 11, 12), (0, 1, 2, 13, 14, 15)        # bone index = joint - 1 of joints_left / joints_right

PROTOCOL_HEAD = ("act", "mpjpe", "sag sym", "seg std", "p-mpjpe", "mvjpe", "mse", "err var", "seg err")
PROTOCOL_HEAD_RMCL = ("oracle mpjpe", "pseudo oracle mpjpe")
# column of protocol_1_err.csv -> key of AnalyticsAccumulator.report(); "mpjpe" and the two oracle columns come from evaluate() itself
_PROTOCOL_KEYS = ("mpsse", "mpsce", "p_mpjpe", "mvjpe", "mse", "err_var", "seg_len_err")
SEG_ERR_SAMPLES = 1000              # rows of all_seg_errs.npy per action (main_h36m_lifting.py:998-1004)


def joints_names(skeleton=None) -> List[str]:
    """The skeleton's joint names when it carries any, else the built-in H36M table."""
    names = list(getattr(skeleton, "joints_names", None) or ())
    return names if any(names) else list(H36M_JOINTS_NAMES)


def bones_names(skeleton=None) -> List[str]:
    """"parent->child" of every bone (joint k+1, its parent), as Skeleton.bones_names."""
    names = list(getattr(skeleton, "joints_names", None) or ())
    if any(names):
        return list(skeleton.bones_names)
    return [f"{H36M_JOINTS_NAMES[p]}->{H36M_JOINTS_NAMES[j]}" for j, p in enumerate(_PARENTS) if p >= 0]


def write_csv(path: str, head: Sequence[str], rows: Sequence[Sequence]) -> None:
    """``pd.DataFrame(rows).to_csv(path, header=head, index=False)``: floats as their shortest round-trip text (what numpy's
    ``astype(str)`` and pandas both write for a float64)."""
    def cell(v):
        return v if isinstance(v, str) else repr(float(v))
    with open(path, "w", newline="") as f:
        w = csv.writer(f, lineterminator="\n", quoting=csv.QUOTE_MINIMAL)
        w.writerow(list(head))
        for r in rows:
            if len(r) != len(head):
                raise ValueError(f"{os.path.basename(path)}: a row of {len(r)} cells under a head of {len(head)}")
            w.writerow([cell(v) for v in r])


def seg_symmetry_row(per_pair: Sequence[float], num_bones: int = 16) -> np.ndarray:
    """The six left/right pair values at ``bones_left`` AND ``bones_right`` of a (num_bones,) row, zero elsewhere
    (main_h36m_lifting.py:1017-1022)."""
    row = np.zeros(num_bones)
    row[list(BONES_LEFT)] = np.asarray(per_pair, dtype=np.float64)
    row[list(BONES_RIGHT)] = np.asarray(per_pair, dtype=np.float64)
    return row


def _table(labels, values):
    """Rows [label, *values] plus the last row "average" of column means (errs[-1] = np.mean(errs[:-1], axis=0))."""
    v = np.asarray(values, dtype=np.float64).reshape(len(labels), -1)
    v = np.vstack([v, v.mean(axis=0, keepdims=True)])
    return [[lab, *row.tolist()] for lab, row in zip(list(labels) + ["average"], v)]


def draw_seg_err_rows(n: int, samples: int = SEG_ERR_SAMPLES) -> np.ndarray:
    """The reference's draw of rows of the (n, 16) per-frame bone-length error table: np.random.randint(0, n - 1, 1000) on the global
    numpy generator (main_h36m_lifting.py:998-1004)."""
    return np.random.randint(low=0, high=n - 1, size=samples)


def write_h36m_report(out_dir: str, groups: Mapping[str, Mapping], skeleton=None, rmcl: bool = False) -> List[str]:
    """``groups``: {action: {"mpjpe": .., ["oracle_mpjpe": .., "ps_oracle_mpjpe": ..,] "analytics": AnalyticsAccumulator.report(),
    ["seg_errs": (1000, 16) array]}} in the order of the rows.  Returns the paths written."""
    acts = list(groups)
    if not acts:
        raise ValueError("write_h36m_report: no group to report")
    an = [groups[a]["analytics"] for a in acts]
    jn, bn = joints_names(skeleton), bones_names(skeleton)
    head = list(PROTOCOL_HEAD) + (list(PROTOCOL_HEAD_RMCL) if rmcl else [])
    prot = []
    for a, t in zip(acts, an):
        row = [groups[a]["mpjpe"]] + [t.get(k, float("nan")) for k in _PROTOCOL_KEYS]
        if rmcl:
            row += [groups[a].get("oracle_mpjpe", float("nan")), groups[a].get("ps_oracle_mpjpe", float("nan"))]
        prot.append(row)
    tables = {
        "protocol_1_err": (head, prot),
        "seg_symmetry": (["act", *bn], [seg_symmetry_row(t["mpsse_per_pair"], len(bn)) for t in an]),
        "seg_consistency": (["act", *bn], [t["mpsce_per_bone"] for t in an]),
        "seg_max_strech": (["act", *bn], [t["seg_max_strech"] for t in an]),
        "seg_max_delta_strech": (["act", *bn], [t["seg_max_delta_strech"] for t in an]),
        "cw_err": (["act", "x", "y", "z"], [t["cw_err"] for t in an]),
        "jw_err": (["act", *jn], [t["jointwise_err"] for t in an]),
    }
    paths = []
    for name, (h, values) in tables.items():
        paths.append(os.path.join(out_dir, name + ".csv"))
        write_csv(paths[-1], h, _table(acts, values))
    paths.append(os.path.join(out_dir, "all_jw_err_var.npy"))
    np.save(paths[-1], np.stack([np.asarray(t["jw_err_var"], dtype=np.float64) for t in an], axis=0))
    seg = [np.asarray(groups[a]["seg_errs"]) for a in acts if groups[a].get("seg_errs") is not None]
    if seg:
        paths.append(os.path.join(out_dir, "all_seg_errs.npy"))
        np.save(paths[-1], np.concatenate(seg, axis=0))
    return paths


def write_3dhp_report(out_dir: str, analytics: Mapping, skeleton=None) -> List[str]:
    """The four single-row tables of main_3dhp.py:769-988 (heads without a label column); seg_consistency is the mean over the windows
    of every window's own std there (:870-878), not the flattened sequence's."""
    jn, bn = joints_names(skeleton), bones_names(skeleton)
    tables = {
        "seg_symmetry": (bn, seg_symmetry_row(analytics["mpsse_per_pair"], len(bn)).tolist()),
        "seg_consistency": (bn, analytics["mpsce_per_bone_windows"]),
        "cw_err": (["x", "y", "z"], analytics["cw_err"]),
        "jw_err": (jn, analytics["jointwise_err"]),
    }
    paths = []
    for name, (h, row) in tables.items():
        paths.append(os.path.join(out_dir, name + ".csv"))
        write_csv(paths[-1], h, [list(row)])
    return paths


# column of hyp_report.csv = key of HypothesisAccumulator.report(); the two consistency columns only when every group carries them
HYP_SCALAR_KEYS = ("mpjpe_weighted_ave", "mpjpe_best_score", "mpjpe_oracle", "mpjpe_jbest", "pairwise_distance", "score_of_oracle", "score_max",
                   "top1_agreement")
HYP_CONSISTENCY_KEYS = ("jbest_mpsse", "jbest_mpsce")
HYP_HEAD_TABLES = ("pbest_head_share", "score_head_share", "jbest_head_share", "score_mass_per_head")


def write_hypothesis_report(out_dir: str, groups: Mapping[str, Mapping], skeleton=None, single: bool = False) -> List[str]:
    """``groups``: {action: HypothesisAccumulator.report()} in the order of the rows.  Three tables in the layout of the other report files
    (a label column "act", one row per group and a last row "average" of column means):
      hyp_report.csv   the scalar keys, then top_1 .. top_K (``mpjpe_top_m``);
      hyp_heads.csv    K columns ``<table>_<k>`` for each of pbest_head_share, score_head_share, jbest_head_share, score_mass_per_head;
      hyp_joints.csv   the J-Best error per joint under the joints' names, then the spread per joint under "spread <joint>".
    ``single=True`` (3DHP): the first group only, as single-row tables without the label column.  Returns the paths written."""
    acts = list(groups)
    if not acts:
        raise ValueError("write_hypothesis_report: no group to report")
    reps = [groups[a] for a in acts]
    K = len(reps[0]["mpjpe_top_m"])
    if any(len(r["mpjpe_top_m"]) != K for r in reps):
        raise ValueError("write_hypothesis_report: the groups differ in their number of hypotheses")
    jn = joints_names(skeleton)
    scalars = list(HYP_SCALAR_KEYS) + [k for k in HYP_CONSISTENCY_KEYS if all(k in r for r in reps)]
    tables = {
        "hyp_report": (scalars + [f"top_{m + 1}" for m in range(K)], [[r[k] for k in scalars] + list(r["mpjpe_top_m"]) for r in reps]),
        "hyp_heads": ([f"{t}_{k}" for t in HYP_HEAD_TABLES for k in range(K)], [[v for t in HYP_HEAD_TABLES for v in r[t]] for r in reps]),
        "hyp_joints": (jn + [f"spread {n}" for n in jn], [list(r["jbest_per_joint"]) + list(r["spread_per_joint"]) for r in reps]),
    }
    paths = []
    for name, (h, values) in tables.items():
        paths.append(os.path.join(out_dir, name + ".csv"))
        if single:
            write_csv(paths[-1], h, [list(values[0])])
        else:
            write_csv(paths[-1], ["act", *h], _table(acts, values))
    return paths


LIFT_SCORE_HEAD = ("frames", "mpjpe", "p_mpjpe", "mpjve", "accel", "bone_std", "bone_err")       # then oracle_mpjpe, then traj_ate, traj_frames


def _weighted_rows(labels, values, weights):
    """Rows [label, *values] plus the last row "average": per column the mean weighted by ``weights`` (a column of ``values``' shape or one weight
    per row) over the rows whose value is not NaN; NaN where no such row carries weight."""
    v = np.asarray(values, dtype=np.float64).reshape(len(labels), -1)
    w = np.broadcast_to(np.asarray(weights, dtype=np.float64).reshape(len(labels), -1), v.shape)
    w = np.where(np.isnan(v), 0.0, w)
    tot = w.sum(axis=0)
    avg = np.where(tot > 0, (np.where(w > 0, v, 0.0) * w).sum(axis=0) / np.where(tot > 0, tot, 1.0), np.nan)
    return [[lab, *row.tolist()] for lab, row in zip(list(labels) + ["average"], np.vstack([v, avg[None]]))]


def write_lift_score_report(out_dir: str, scores: Mapping[str, Mapping], skeleton=None, name: str = "lift_score", joints: bool = True) -> List[str]:
    """``scores``: {sequence key: the score dict of ``lift_sequences(targets=..., return_score=True)`` as numbers / numpy arrays, in metres} in the
    order of the rows.  Two tables in the layout of the other report files (a label column "act", one row per key and a last row "average"),
    the errors in millimetres:
      lift_score.csv         frames, mpjpe, p_mpjpe, mpjve, accel, bone_std (the mean over the bones of a bone's standard deviation over the frames),
                             bone_err (the mean over the bones of |target's length - pose's length|); with hypotheses oracle_mpjpe; with a placed
                             trajectory traj_ate and traj_frames.  The "average" row weighs a row by its frames (traj_ate by traj_frames) and sums
                             the two frame columns;
      lift_score_joints.csv  the error per joint under the joints' names, averaged the same way.
    ``name``: the files' stem (run.lift's fused takes go to lift_score_fused.csv); ``joints=False`` leaves the per-joint table out.
    Returns the paths written."""
    keys = list(scores)
    if not keys:
        raise ValueError("write_lift_score_report: no sequence to report")
    recs = [scores[k] for k in keys]
    num = lambda v: float(np.asarray(v, dtype=np.float64).reshape(()))
    mm = lambda v: 1000.0 * num(v)
    mean_mm = lambda v: 1000.0 * float(np.asarray(v, dtype=np.float64).mean())
    frames = [num(r["frames"]) for r in recs]
    head = ["act", *LIFT_SCORE_HEAD]
    cols = [[mm(r["mpjpe"]), mm(r["p_mpjpe"]), mm(r["mpjve"]), mm(r["accel"]), mean_mm(r["bone_std"]), mean_mm(r["bone_err"])] for r in recs]
    weights = [[f] * 6 for f in frames]
    if all("oracle_mpjpe" in r for r in recs):
        head.append("oracle_mpjpe")
        for c, w, r, f in zip(cols, weights, recs, frames):
            c.append(mm(r["oracle_mpjpe"])); w.append(f)
    traj = all("traj" in r for r in recs)
    if traj:
        head += ["traj_ate", "traj_frames"]
        for c, w, r in zip(cols, weights, recs):
            c.append(mm(r["traj"]["ate"])); w.append(num(r["traj"]["frames"]))
    rows = _weighted_rows(keys, cols, weights)
    rows = [[r[0], f, *r[1:]] for r, f in zip(rows, frames + [float(sum(frames))])]
    if traj:
        tf = [num(r["traj"]["frames"]) for r in recs]
        rows = [[*r, f] for r, f in zip(rows, tf + [float(sum(tf))])]
    jn = joints_names(skeleton)
    per_joint = [1000.0 * np.asarray(r["per_joint"], dtype=np.float64).reshape(-1) for r in recs]
    if any(len(v) != len(jn) for v in per_joint):
        raise ValueError(f"write_lift_score_report: per_joint of {len(per_joint[0])} joints under {len(jn)} joint names")
    paths = [os.path.join(out_dir, f"{name}.csv"), os.path.join(out_dir, f"{name}_joints.csv")][:2 if joints else 1]
    write_csv(paths[0], head, rows)
    if joints:
        write_csv(paths[1], ["act", *jn], _weighted_rows(keys, per_joint, frames))
    return paths

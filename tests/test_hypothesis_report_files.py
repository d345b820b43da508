"""manipose_amd/report.py:write_hypothesis_report (host only) from hand-made HypothesisAccumulator.report() dicts - heads, row order, the
"average" row, the K columns - and the run.hyp_report config key, whose default leaves the files of the test pass as they are."""
import csv
import inspect
import os
import sys

import numpy as np
import pytest

from manipose_amd import report

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALARS = ["mpjpe_weighted_ave", "mpjpe_best_score", "mpjpe_oracle", "mpjpe_jbest", "pairwise_distance", "score_of_oracle", "score_max", "top1_agreement"]
HEAD_TABLES = ["pbest_head_share", "score_head_share", "jbest_head_share", "score_mass_per_head"]


def _hyp(seed, K, consistency=True):
    g = np.random.default_rng(seed)
    r = lambda n: g.uniform(0.5, 50.0, n).tolist()
    out = {k: r(1)[0] for k in SCALARS}
    out.update({"mpjpe_top_m": r(K), "jbest_per_joint": r(17), "spread_per_joint": r(17), "oracle_rank_hist": r(K)})
    out.update({t: r(K) for t in HEAD_TABLES})
    if consistency:
        out["jbest_mpsse"], out["jbest_mpsce"] = r(2)
    return out


def _read(path):
    with open(path, newline="") as f:
        return list(csv.reader(f))


def _values(rows):
    return np.array([[float(v) for v in r[1:]] for r in rows[1:]])


@pytest.mark.parametrize("K,consistency", [(5, True), (3, False), (1, True)])
def test_hypothesis_report_files(tmp_path, K, consistency):
    acts = ["walking", "eating", "sittingdown"]                  # row order = the order of the groups, not sorted
    groups = {a: _hyp(i, K, consistency) for i, a in enumerate(acts)}
    written = report.write_hypothesis_report(str(tmp_path), groups)
    assert [os.path.basename(p) for p in written] == ["hyp_report.csv", "hyp_heads.csv", "hyp_joints.csv"] and all(os.path.exists(p) for p in written)
    scal = SCALARS + (["jbest_mpsse", "jbest_mpsce"] if consistency else [])
    rows = _read(tmp_path / "hyp_report.csv")
    assert rows[0] == ["act", *scal, *[f"top_{m}" for m in range(1, K + 1)]]
    assert [r[0] for r in rows[1:]] == acts + ["average"] and all(len(r) == len(rows[0]) for r in rows)
    want = np.array([[groups[a][k] for k in scal] + groups[a]["mpjpe_top_m"] for a in acts])
    got = _values(rows)
    assert np.array_equal(got[:-1], want) and np.array_equal(got[-1], want.mean(axis=0))       # text round-trips the float64 values exactly
    rows = _read(tmp_path / "hyp_heads.csv")
    assert rows[0] == ["act"] + [f"{t}_{k}" for t in HEAD_TABLES for k in range(K)] and len(rows[0]) == 1 + 4 * K
    assert [r[0] for r in rows[1:]] == acts + ["average"]
    want = np.array([[v for t in HEAD_TABLES for v in groups[a][t]] for a in acts])
    got = _values(rows)
    assert np.array_equal(got[:-1], want) and np.array_equal(got[-1], want.mean(axis=0))
    rows = _read(tmp_path / "hyp_joints.csv")
    joints = report.joints_names()
    assert rows[0] == ["act", *joints, *[f"spread {n}" for n in joints]] and rows[0][1:18] == list(report.H36M_JOINTS_NAMES)
    assert [r[0] for r in rows[1:]] == acts + ["average"]
    want = np.array([groups[a]["jbest_per_joint"] + groups[a]["spread_per_joint"] for a in acts])
    got = _values(rows)
    assert np.array_equal(got[:-1], want) and np.array_equal(got[-1], want.mean(axis=0))
    raw = open(tmp_path / "hyp_report.csv").read()
    assert "\r" not in raw and raw.startswith("act,mpjpe_weighted_ave,") and raw.endswith("\n")


def test_single_row_tables_and_refusals(tmp_path):
    """3DHP: one row, no label column (as write_3dhp_report).  No group, or groups of different K, are refused."""
    h = _hyp(4, 5)
    written = report.write_hypothesis_report(str(tmp_path), {"all": h}, single=True)
    assert [os.path.basename(p) for p in written] == ["hyp_report.csv", "hyp_heads.csv", "hyp_joints.csv"]
    rows = _read(tmp_path / "hyp_report.csv")
    assert len(rows) == 2 and rows[0] == SCALARS + ["jbest_mpsse", "jbest_mpsce"] + [f"top_{m}" for m in range(1, 6)]
    assert [float(v) for v in rows[1]] == [h[k] for k in rows[0][:10]] + h["mpjpe_top_m"]
    rows = _read(tmp_path / "hyp_joints.csv")
    assert len(rows) == 2 and rows[0][:17] == report.joints_names() and [float(v) for v in rows[1]] == h["jbest_per_joint"] + h["spread_per_joint"]
    rows = _read(tmp_path / "hyp_heads.csv")
    assert len(rows) == 2 and len(rows[0]) == 20 and [float(v) for v in rows[1][5:10]] == h["score_head_share"]
    with pytest.raises(ValueError):
        report.write_hypothesis_report(str(tmp_path), {})
    with pytest.raises(ValueError):
        report.write_hypothesis_report(str(tmp_path), {"a": _hyp(1, 5), "b": _hyp(2, 3)})


def test_config_key_parses_and_its_default_changes_nothing(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "hpe"))
    import _entry
    assert _entry.load_config([]).run.hyp_report is False
    assert _entry.load_config(["run.hyp_report=true"]).run.hyp_report is True
    assert inspect.signature(_entry.evaluate).parameters["hypotheses"].default is False
    # the file list of the test pass does not know the key: the same nine files
    g = np.random.default_rng(0)
    r = lambda n: g.uniform(0.5, 50.0, n).tolist()
    an = {"mpsse": 1.0, "mpsce": 1.0, "p_mpjpe": 1.0, "mvjpe": 1.0, "mse": 1.0, "err_var": 1.0, "seg_len_err": 1.0, "mpsse_per_pair": r(6),
          "mpsce_per_bone": r(16), "seg_max_strech": r(16), "seg_max_delta_strech": r(16), "cw_err": r(3), "jointwise_err": r(17), "jw_err_var": r(17)}
    written = report.write_h36m_report(str(tmp_path), {"walking": {"mpjpe": 40.0, "analytics": an, "seg_errs": np.zeros((1000, 16))}})
    assert sorted(os.path.basename(p) for p in written) == sorted(
        ["protocol_1_err.csv", "seg_symmetry.csv", "seg_consistency.csv", "seg_max_strech.csv", "seg_max_delta_strech.csv", "cw_err.csv", "jw_err.csv",
         "all_jw_err_var.npy", "all_seg_errs.npy"])
    assert not any(f.startswith("hyp_") for f in os.listdir(tmp_path))

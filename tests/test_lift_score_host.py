"""Scoring a lift, the host side (no GPU): the numpy statement of the rule (lift_score_ref.py) against the oracle's metrics, the condition the GPU
tests' Procrustes inputs must meet (the eigenvalue gap of Horn's matrix), the new entry points of the C ABI in the places that declare them, the
exports, every argument error of score_poses, score_traj and lift_sequences(targets=...) - raised before anything touches a device - the option
checker of the entry point, and the CSV writer."""
import csv
import os
import re
import shlex
import sys

import numpy as np
import pytest
import torch

import lift_score_ref as ref
import manipose_ref as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hpe"))


@pytest.mark.parametrize("root_relative", [False, True])
def test_the_statement_equals_the_oracles_metrics(root_relative):
    """mpjpe_error, mean_velocity_error and p_mpjpe of oracle/manipose_ref.py are pinned to the reference by tests/golden/metrics.npz; both sides
    are float64 numpy / torch on the same numbers: 1e-12 relative."""
    pred, gt, _ = ref.related_inputs([200], 1, 17, 3, 3)
    flags = ref.PROCRUSTES | (ref.ROOT_RELATIVE if root_relative else 0)
    rows, frame_err = ref.score_rows(pred, gt, parents=ref.H36M_PARENTS, flags=flags)
    f = ref.fields(rows, 17)
    P, G = (torch.from_numpy(ref.points(x, 1.0, root_relative)) for x in (pred[:, 0], gt))
    close = lambda a, b: abs(float(a) - float(b)) <= 1e-12 * abs(float(b))
    assert rows[0, 0, 0] == 200 and rows[0, 0, 3] == 199 and rows[0, 0, 5] == 198 and rows[0, 0, 8] == 0
    assert close(f["mpjpe"][0, 0], orc.mpjpe_error(P, G))
    assert close(f["mpjve"][0, 0], orc.mean_velocity_error(P, G, axis=0))
    assert close(f["p_mpjpe"][0, 0], orc.p_mpjpe(P, G))
    assert close(f["accel"][0, 0], torch.norm(torch.diff(P, n=2, dim=0) - torch.diff(G, n=2, dim=0), dim=-1).mean())
    assert close(f["rmse"][0, 0], torch.sqrt(((P - G) ** 2).sum(-1).mean()))
    assert np.allclose(f["per_joint"][0, 0], torch.norm(P - G, dim=-1).mean(0).numpy(), rtol=1e-12, atol=0)
    assert np.allclose(frame_err[:, 0], torch.norm(P - G, dim=-1).mean(1).numpy(), rtol=2.0 ** -23, atol=0)
    par = np.array(ref.H36M_PARENTS[1:])
    L = torch.norm(P[:, 1:] - P[:, par], dim=-1).numpy()
    LG = torch.norm(G[:, 1:] - G[:, par], dim=-1).numpy()
    assert np.allclose(f["bone_mean"][0, 0], L.mean(0), rtol=1e-12) and np.allclose(f["bone_std"][0, 0], L.std(0), rtol=1e-9)
    assert np.allclose(f["bone_err"][0, 0], np.abs(LG - L).mean(0), rtol=1e-12)


def test_the_rules_of_the_statement():
    pred, gt, off = ref.related_inputs([5, 1, 9], 2, 17, 4, 4)
    valid = np.ones((15, 2), np.uint8)
    valid[7, 0] = 0
    pred[9, 1, 4, 2] = np.inf
    gt[12, 0, 0] = np.nan
    rows, fe = ref.score_rows(pred, gt, off, valid, ref.H36M_PARENTS, flags=ref.PROCRUSTES)
    assert rows[:, :, 0].tolist() == [[5, 5], [1, 1], [7, 7]] and rows[:, :, 3].tolist() == [[4, 4], [0, 0], [4, 4]] and rows[:, :, 5].tolist() == [[3, 3], [0, 0], [2, 1]]
    assert fe[7, 0] == -1 and fe[9, 1] == -1 and (fe[12] == -1).all() and (fe[[7, 9], [1, 0]] > 0).all()
    # a sequence gives what it gives alone; a wild table is its clamped form; an empty range is a zero row and leaves its frames alone
    alone = ref.score_rows(pred[6:], gt[6:], None, valid[6:], ref.H36M_PARENTS, flags=ref.PROCRUSTES)
    assert np.array_equal(alone[0][0], rows[2]) and np.array_equal(alone[1], fe[6:])
    wild = ref.score_rows(pred, gt, [-5, 5, 6, 10 ** 12], valid, ref.H36M_PARENTS, flags=ref.PROCRUSTES)
    assert np.array_equal(wild[0], rows) and np.array_equal(wild[1], fe)
    part = ref.score_rows(pred, gt, [6, 6, 15], valid, ref.H36M_PARENTS, flags=ref.PROCRUSTES)
    assert not part[0][0].any() and np.array_equal(part[0][1], rows[2]) and (part[1][:6] == -7).all()
    # the velocity of the channel that is not read, and of a root-relative pose's root, is nothing
    assert np.array_equal(ref.score_rows(pred[..., :3].copy(), gt, off, valid, ref.H36M_PARENTS, flags=ref.PROCRUSTES)[0], rows)
    rel = ref.score_rows(pred, gt, off, valid, None, flags=ref.ROOT_RELATIVE)[0]
    assert not rel[:, :, 9].any() and not rel[:, :, 7:9].any() and not rel[:, :, 9 + 17:].any()
    # all joints on one spot: the alignment skips the frame
    pred[2, 0, :, :3] = 0.25
    assert ref.score_rows(pred, gt, off, valid, None, flags=ref.PROCRUSTES)[0][0, :, 8].tolist() == [1, 0]


def test_the_gpu_tests_procrustes_inputs_are_well_conditioned():
    """A CONDITION on the inputs: the kernel finds the alignment's rotation as the dominant eigenvector of Horn's 4x4 matrix, whose error is about
    2^-52 / (relative gap of the two largest eigenvalues).  Slot 7's bound (1e-9) assumes a gap of at least 0.1; "related" poses keep it, unrelated
    random poses fall to 6e-3 and are not used for slot 7."""
    print()
    for name, pred, gt in ref.procrustes_inputs():
        gaps, worst = [], 0.0
        for g in range(len(gt)):
            G = ref.points(gt[g], 1.0, False)
            for i in range(pred.shape[1]):
                P = ref.points(pred[g, i], 1.0, False)
                if np.isfinite(P).all() and np.isfinite(G).all() and ref.procrustes_errors(P, G) is not None:
                    gaps.append(ref.horn_gap(P, G))
                    if g % 7 == 0:
                        worst = max(worst, float(np.abs(ref.horn_errors(P, G) - ref.procrustes_errors(P, G)).max()))
        print(f"[{name}] {len(gaps)} poses: smallest relative eigenvalue gap {min(gaps):.3f}; Horn's form against the SVD form: {worst:.1e}")
        assert min(gaps) >= 0.1 and worst <= 1e-12
    g = np.random.default_rng(0)                                             # what the condition keeps out
    unrelated = min(ref.horn_gap(0.3 * g.standard_normal((17, 3)), 0.3 * g.standard_normal((17, 3))) for _ in range(2000))
    assert unrelated < 0.05


def test_new_abi_symbols_are_declared_everywhere():
    from manipose_amd import _lib, lifting
    import manipose_amd
    header = open(_lib.HEADER_PATH).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    declared = _lib.declared_symbols()
    names = ("mp_lift_score_row_doubles", "mp_lift_score_scratch_doubles", "mp_lift_score")
    assert all(n in declared and n in _lib._SIGNATURES and f"lib.{n}.argtypes" in doc for n in names)
    proto = re.search(r"int mp_lift_score\((.*?)\);", header, flags=re.S).group(1)
    assert len(proto.split(",")) == len(_lib._SIGNATURES["mp_lift_score"][1]) == 18
    assert _lib._SIGNATURES["mp_lift_score"][1][10] is _lib.f64 and _lib._SIGNATURES["mp_lift_score"][1][11] is _lib.f64
    assert _lib._SIGNATURES["mp_lift_score_scratch_doubles"] == (_lib.i64, [_lib.i32] * 3) and _lib._SIGNATURES["mp_lift_score_row_doubles"] == (_lib.i32, [_lib.i32])
    assert _lib.ABI_VERSION == 8 and int(re.search(r"#define MP_ABI_VERSION (\d+)", header).group(1)) == 8        # purely additive
    shares = int(re.search(r"#define MP_LIFT_SCORE_SHARES (\d+)", header).group(1))
    assert shares == lifting.SCORE_SHARES and shares > 1                    # more than one workgroup per sequence
    assert manipose_amd.score_poses is lifting.score_poses and manipose_amd.score_traj is lifting.score_traj
    assert "score_poses" in lifting.__all__ and "score_traj" in lifting.__all__
    assert lifting._Lifted._fields == ("poses", "hyps", "bones", "place", "path", "score", "rotations")
    assert os.path.exists(os.path.join(ROOT, "manipose_amd", "csrc", "lift_score.hip"))
    if os.path.exists(_lib.LIB_PATH):
        lib = _lib.load()
        assert [lib.mp_lift_score_row_doubles(M) for M in (1, 17, 32, 0, 33)] == [9 + 1, 9 + 17 + 48, 9 + 32 + 93, 0, 0]
        assert lib.mp_lift_score_scratch_doubles(3, 5, 17) == 3 * 5 * shares * 74 and lib.mp_lift_score_scratch_doubles(0, 5, 17) == 0
        assert lib.mp_lift_score(None, 1, 1, 17, 3, None, None, None, 1, None, 1.0, 1.0, 0, None, None, None, 0, None) == 1       # refused on the host
        assert b"null" in lib.mp_last_error()


def _cpu_model(n_hyp=2):
    from manipose_amd import RMCLManifoldMixSTE, h36m_skeleton
    return RMCLManifoldMixSTE(h36m_skeleton(), n_hyp=n_hyp, num_frame=9, embed_dim_rot=32, depth_rot=1, num_heads_rot=4, embed_dim_seg=16, depth_seg=1,
                              num_heads_seg=4)


def test_argument_errors_are_value_errors_before_any_device_work():
    """Every call below is given CPU tensors or a CPU model: had the arguments been accepted, the call would have ended in the RuntimeError that
    refuses them ("no CPU fallback"), which is what the valid calls at the end do."""
    from manipose_amd import h36m_skeleton, lift_sequences, score_poses, score_traj
    p3, p4, t = torch.zeros(6, 17, 3), torch.zeros(6, 5, 17, 4), torch.zeros(6, 17, 3)
    u8 = lambda *shape: torch.ones(*shape, dtype=torch.uint8)
    for args, kw, word in (((p3.double(), t), {}, "poses must be"), ((torch.zeros(6, 17, 4), t), {}, "poses must be"), ((p4.transpose(0, 1), t), {}, "poses must be"),
                           ((torch.zeros(6, 33, 3), torch.zeros(6, 33, 3)), {}, "2..32 expected"),
                           ((p3, torch.zeros(5, 17, 3)), {}, "target must be"), ((p3, t.double()), {}, "target must be"), ((p3, t.numpy()), {}, "target must be"),
                           ((p4, torch.zeros(6, 5, 17, 3)), {}, "target must be"), ((p3, torch.zeros(6, 3, 17).transpose(1, 2)), {}, "target must be"),
                           ((p3, t), dict(valid=u8(6, 1)), "valid must be"), ((p4, t), dict(valid=u8(6)), "valid must be"),
                           ((p4, t), dict(valid=torch.ones(6, 5)), "valid must be"), ((p3, t), dict(valid=np.ones(6, np.uint8)), "valid must be"),
                           ((p3, t), dict(pose_scale=0.0), "finite numbers > 0"), ((p3, t), dict(target_scale=-1.0), "finite numbers > 0"),
                           ((p3, t), dict(pose_scale=float("inf")), "finite numbers > 0"), ((p3, t), dict(target_scale=float("nan")), "finite numbers > 0"),
                           ((p3, t), dict(pose_scale="1"), "finite numbers > 0"), ((p3, t), dict(pose_scale=True), "finite numbers > 0"),
                           ((torch.zeros(6, 2, 3), torch.zeros(6, 2, 3)), {}, "at least 3 joints"),
                           ((torch.zeros(6, 5, 3), torch.zeros(6, 5, 3)), dict(skeleton=h36m_skeleton()), "the skeleton has 17")):
        with pytest.raises(ValueError, match=word):
            score_poses(*args, **kw)
    for args, kw in (((p3, t), {}), ((p4, t), dict(valid=u8(6, 5), root_relative=True, return_frames=True)), ((p3.numpy(), t), {}),
                     ((torch.zeros(6, 2, 3), torch.zeros(6, 2, 3)), dict(procrustes=False))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            score_poses(*args, **kw)
    tr, tt = torch.zeros(6, 3), torch.zeros(6, 3)
    for args, kw, word in (((torch.zeros(6, 4), tt), {}, "traj must be"), ((tr.double(), tt), {}, "traj must be"), ((torch.zeros(6, 2, 2, 3), tt), {}, "traj must be"),
                           ((tr, torch.zeros(5, 3)), {}, "target must be"), ((torch.zeros(6, 4, 3), torch.zeros(6, 4, 3)), {}, "target must be"),
                           ((tr, tt.double()), {}, "target must be"), ((tr, tt), dict(ok=u8(6, 1)), "ok must be"), ((tr, tt), dict(ok=torch.ones(6)), "ok must be"),
                           ((torch.zeros(6, 4, 3), tt), dict(ok=u8(6)), "ok must be")):
        with pytest.raises(ValueError, match=word):
            score_traj(*args, **kw)
    for args, kw in (((tr, tt), {}), ((torch.zeros(6, 4, 3), tt), dict(ok=u8(6, 4))), ((tr.numpy(), tt), {})):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            score_traj(*args, **kw)
    model = _cpu_model()
    seqs = [np.zeros((12, 17, 2), np.float32), np.zeros((20, 17, 2), np.float32)]
    good = [np.zeros((12, 17, 3), np.float32), np.zeros((20, 17, 3), np.float32)]
    for kw, word in ((dict(return_score=True), "pass targets"), (dict(targets=good[:1], return_score=True), "1 arrays for 2 sequences"),
                     (dict(targets=good + good[:1]), "3 arrays for 2 sequences"), (dict(targets=[good[0], good[1][:19]]), "targets\\[1\\] must be \\(20, 17, 3\\)"),
                     (dict(targets=[good[0][:, :16], good[1]]), "targets\\[0\\] must be"), (dict(targets=[good[0], np.zeros((20, 17, 2), np.float32)]), "targets\\[1\\] must be"),
                     (dict(targets=[good[0], good[1].astype(str)]), "targets\\[1\\] must be"), (dict(targets=[good[0], torch.zeros(20, 17)]), "targets\\[1\\] must be"),
                     (dict(targets=good, return_score=True, keep_padding=True), "keep_padding")):
        with pytest.raises(ValueError, match=word):
            lift_sequences(model, seqs, **kw)
    for kw in (dict(targets=good, return_score=True), dict(targets=[torch.from_numpy(g) for g in good], return_score=True, return_hyps=True),
               dict(targets=good), dict(targets=None, return_score=False)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            lift_sequences(model, seqs, **kw)


def test_config_key_the_option_checker_and_the_readme_command():
    from _entry import lift_score_options, load_config, run, synthetic_sequences_2d, synthetic_sequences_3d
    cfg = load_config([])
    assert cfg.lift.score is False and lift_score_options(cfg) is False
    assert lift_score_options(load_config(["run.lift=true", "lift.score=true"])) is True
    assert lift_score_options(load_config(["run.lift=true", "lift.score=false"])) is False
    for argv, word in ((["lift.score=true"], "set run.lift=true"), (["run.lift=true", "lift.score=2"], "true or false"), (["run.lift=true", "lift.score=mm"], "true or false")):
        with pytest.raises(ValueError, match=word):
            lift_score_options(load_config(argv))
        with pytest.raises(ValueError, match=word):                          # ... and before the model is built (a run that got further would need a device)
            run(["run.train=false", "run.test=false"] + argv)
    with pytest.raises(SystemExit):
        load_config(["lift.scor=true"])
    lines = [l for l in open(os.path.join(ROOT, "README.md")).read().splitlines() if l.startswith("python hpe/") and "lift.score=true" in l]
    assert len(lines) == 1
    assert lift_score_options(load_config(shlex.split(lines[0].split("#")[0])[2:])) is True
    # the synthetic targets: the 2-D sequences' keys and lengths, a stream of their own (the 2-D side keeps its bits), the root a few metres away
    cfg = load_config(["data.synthetic_sequences=3", "data.seq_len=27"])
    p2, p3 = synthetic_sequences_2d(cfg, 7), synthetic_sequences_3d(cfg, 7)
    assert list(p2) == list(p3) and all(len(p3[k]) == 1 and p3[k][0].shape == (p2[k][0].shape[0], 17, 3) and p3[k][0].dtype == np.float32 for k in p2)
    g = np.random.default_rng(7)
    assert all(np.array_equal(v[0], np.clip(0.3 * g.standard_normal(v[0].shape), -1, 1).astype(np.float32)) for v in p2.values())
    assert all(np.array_equal(a[0], b[0]) for a, b in zip(p3.values(), synthetic_sequences_3d(cfg, 7).values()))
    assert not np.array_equal(p3["synthetic_000"][0], synthetic_sequences_3d(cfg, 8)["synthetic_000"][0]) and p3["synthetic_000"][0][:, 0, 2].mean() > 3


def test_the_csv_writer(tmp_path):
    from manipose_amd import report
    rec = lambda n, e: dict(frames=np.float64(n), mpjpe=np.float64(e), rmse=np.float64(e), p_mpjpe=np.float64(e / 2), mpjve=np.float64(e / 4), accel=np.float64(e / 8),
                            per_joint=np.full(17, e), bone_mean=np.full(16, 0.3), bone_std=np.linspace(0.0, 0.002, 16), bone_err=np.full(16, e / 10))
    scores = {"a": rec(100, 0.05), "b": rec(300, 0.01), "c": dict(rec(0, np.nan), mpjve=np.float64(np.nan))}
    paths = report.write_lift_score_report(str(tmp_path), scores)
    assert [os.path.basename(p) for p in paths] == ["lift_score.csv", "lift_score_joints.csv"]
    rows = list(csv.reader(open(paths[0])))
    assert rows[0] == ["act", "frames", "mpjpe", "p_mpjpe", "mpjve", "accel", "bone_std", "bone_err"] and [r[0] for r in rows[1:]] == ["a", "b", "c", "average"]
    val = lambda r, c: float(rows[r][rows[0].index(c)])
    assert val(1, "mpjpe") == 50.0 and val(2, "p_mpjpe") == 5.0 and val(1, "mpjve") == 12.5 and val(1, "accel") == 6.25 and val(2, "bone_err") == 1.0
    assert abs(val(1, "bone_std") - 1.0) < 1e-12 and np.isnan(val(3, "mpjpe")) and val(3, "frames") == 0
    assert val(4, "frames") == 400 and abs(val(4, "mpjpe") - (100 * 50 + 300 * 10) / 400) < 1e-9                 # weighted by the frames; the NaN row carries none
    joints = list(csv.reader(open(paths[1])))
    assert joints[0] == ["act", *report.H36M_JOINTS_NAMES] and len(joints) == 5 and float(joints[1][3]) == 50.0 and abs(float(joints[4][17]) - 20.0) < 1e-9
    # with hypotheses and a placed trajectory: three more columns, traj_ate weighted by its own frames
    for k, (o, a, n) in zip(scores, ((0.04, 0.2, 50), (0.005, 0.1, 150), (np.nan, np.nan, 0))):
        scores[k]["oracle_mpjpe"] = np.float64(o)
        scores[k]["traj"] = dict(frames=np.float64(n), ate=np.float64(a), rmse=np.float64(a), velocity=np.float64(a), accel=np.float64(a))
    rows = list(csv.reader(open(report.write_lift_score_report(str(tmp_path), scores)[0])))
    assert rows[0][8:] == ["oracle_mpjpe", "traj_ate", "traj_frames"] and rows[0][:8] == ["act", "frames", "mpjpe", "p_mpjpe", "mpjve", "accel", "bone_std", "bone_err"]
    assert float(rows[1][8]) == 40.0 and float(rows[2][9]) == 100.0 and float(rows[4][10]) == 200 and abs(float(rows[4][9]) - (50 * 200 + 150 * 100) / 200) < 1e-9
    with pytest.raises(ValueError, match="no sequence"):
        report.write_lift_score_report(str(tmp_path), {})

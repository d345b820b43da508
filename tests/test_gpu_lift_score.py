"""Scoring a lift on the device: mp_lift_score against the float64 statement (lift_score_ref.py), determinism and the independence of the
sequences, the exact cases, argument errors, score_poses / score_traj, lift_sequences(targets=...) and run.lift with lift.score.

What is compared and why.  The kernels and the statement work in fp64 on the same float32 inputs and differ by rounding only.  COUNTS (slots 0, 3, 5,
8) are exact.  Every SUM but slot 7 is held to |got - want| <= 1e-10 max(1, |want|): at most 300 * 17 * 3 terms of relative rounding 2^-53 give about
2e-12, so this leaves about 50 times headroom.  SLOT 7 (the aligned error) to 1e-9 max(1, |want|): the kernel's rotation is the dominant eigenvector of
Horn's matrix, whose error is about 2^-52 / gap - at most 1e-14 at the gap of 0.1 that test_lift_score_host.py asserts for every input used here -
and enters the summed norms linearly.  frame_err, a float32, to 2^-23 max(1, |x|), the bound of the other lifting tests, and exactly -1 on a frame that
is not counted.  No bound is measured from the kernel; the worst observed error of each class is printed."""
import csv
import os
import sys

import numpy as np
import pytest
import torch

import lift_score_ref as ref
from lift_fixtures import fixture_model as _model, same as _same, sequences as _sequences

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNT_SLOTS = (0, 3, 5, 8)
FILL = -7.0


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _parents(M):
    import ctypes as C
    return (C.c_int32 * M)(*ref.H36M_PARENTS) if M == 17 else None


def _call(lib, pred, gt, off, valid=None, flags=0, bones=True, pred_scale=1.0, gt_scale=1.0, want_frames=True):
    """mp_lift_score itself on host arrays: (rows (S, inner, R), frame_err (Ntot, inner) prefilled with FILL, or None)"""
    from manipose_amd import _lib
    ntot, inner, M, ch = pred.shape
    d_off = off if torch.is_tensor(off) else _dev(np.asarray(off, np.int64))
    S = int(d_off.numel()) - 1
    R = int(lib.mp_lift_score_row_doubles(M))
    assert R == ref.row_doubles(M)
    rows = torch.full((S, inner, R), FILL, dtype=torch.float64, device="cuda")
    fe = torch.full((ntot, inner), FILL, device="cuda") if want_frames else None
    n = int(lib.mp_lift_score_scratch_doubles(S, inner, M))
    scratch = torch.full((n,), np.nan, dtype=torch.float64, device="cuda")
    d_pred, d_gt, d_valid = _dev(pred), _dev(gt), _dev(valid) if valid is not None else None          # (alive until the call has run)
    _lib.check(lib.mp_lift_score(_lib.ptr(d_pred), ntot, inner, M, ch, _lib.ptr(d_gt), _lib.ptr(d_valid), _lib.ptr(d_off), S, _parents(M) if bones else None, pred_scale, gt_scale, flags, _lib.ptr(rows), _lib.ptr(fe), _lib.ptr(scratch),
                                 n, None), "mp_lift_score")
    torch.cuda.synchronize()
    return rows.cpu().numpy(), fe.cpu().numpy() if want_frames else None


def _errors(rows, want, fe=None, want_fe=None):
    """(counts differ, worst sum error, worst slot-7 error, worst frame_err error), each relative to its max(1, |want|)"""
    rel = np.abs(rows - want) / np.maximum(1.0, np.abs(want))
    sums = [k for k in range(rows.shape[-1]) if k not in COUNT_SLOTS and k != 7]
    frame = 0.0
    if fe is not None:
        assert np.array_equal(fe == -1.0, want_fe == -1.0) and np.array_equal(fe == FILL, want_fe == FILL)
        frame = float((np.abs(fe.astype(np.float64) - want_fe) / np.maximum(1.0, np.abs(want_fe))).max())
    return int((rows[..., COUNT_SLOTS] != want[..., COUNT_SLOTS]).sum()), float(rel[..., sums].max()), float(rel[..., 7].max()), frame


def _holds(rows, want, fe=None, want_fe=None, tag=""):
    counts, sums, aligned, frame = _errors(rows, want, fe, want_fe)
    if tag:
        print(f"\n[score {tag}] counts that differ {counts}; worst sum {sums:.2e} (bound 1e-10), aligned sum {aligned:.2e} (bound 1e-9), "
              f"frame_err {frame:.2e} (bound {2.0 ** -23:.2e})")
    return counts == 0 and sums <= 1e-10 and aligned <= 1e-9 and frame <= 2.0 ** -23


@pytest.mark.parametrize("case", ref.GPU_CASES, ids=ref.case_id)
def test_against_fp64(lib, case):
    inner, M, C, rr = case
    pred, gt, off = ref.case_inputs(case)
    flags = (ref.ROOT_RELATIVE if rr else 0) | (ref.PROCRUSTES if M == 17 else 0)
    parents = ref.H36M_PARENTS if M == 17 else None
    for valid in (None, ref.valid_pattern(off, inner)):
        want, want_fe = ref.score_rows(pred, gt, off, valid, parents, flags=flags, frame_fill=FILL)
        rows, fe = _call(lib, pred, gt, off, valid, flags)
        assert _holds(rows, want, fe, want_fe, f"{ref.case_id(case)} valid={'null' if valid is None else 'pattern'}")
        assert want[3:, :, 0].min() >= 60 and want[:3, :, 5].tolist() == [[0] * inner, [0] * inner, [1] * inner] and want[1, :, 3].tolist() == [1] * inner
        assert (want[:, :, 0].sum(0) < off[-1]).all() and (M != 17 or (want[..., 7] > 0).all())      # the NaN frames are not counted
        again = _call(lib, pred, gt, torch.from_numpy(off).cuda(), valid, flags)
        assert _same(again[0], rows) and _same(again[1], fe)                 # two calls, a host table uploaded and a device table: identical bits
    # scales: the statement with them; and without bones the bone slots are zero, the others keep their bits
    want, want_fe = ref.score_rows(pred, gt, off, None, parents, 1000.0, 0.5, flags, frame_fill=FILL)
    scaled, scaled_fe = _call(lib, pred, gt, off, None, flags, pred_scale=1000.0, gt_scale=0.5)
    assert _holds(scaled, want, scaled_fe, want_fe)
    bare = _call(lib, pred, gt, off, valid, flags, bones=False, want_frames=False)[0]
    assert _same(bare[..., :9 + M], rows[..., :9 + M]) and not bare[..., 9 + M:].any()


def test_sequences_are_independent(lib):
    pred, gt, off, other_p, other_g = ref.independence_inputs()
    flags = ref.PROCRUSTES
    valid = ref.valid_pattern(off, 5)
    rows, fe = _call(lib, pred, gt, off, valid, flags)
    assert _holds(rows, *ref.score_rows(pred, gt, off, valid, ref.H36M_PARENTS, flags=flags, frame_fill=FILL)[:1])
    # the last sequence changes: the sequences before it keep their bits
    r2, f2 = _call(lib, other_p, other_g, off, valid, flags)
    assert _same(r2[:4], rows[:4]) and _same(f2[:off[4]], fe[:off[4]]) and not _same(r2[4], rows[4])
    # a sequence alone gives the bits it has in the call of five
    for s in (3, 4):
        a, b = int(off[s]), int(off[s + 1])
        r1, f1 = _call(lib, np.ascontiguousarray(pred[a:b]), np.ascontiguousarray(gt[a:b]), [0, b - a], np.ascontiguousarray(valid[a:b]), flags)
        assert _same(r1[0], rows[s]) and _same(f1, fe[a:b])
    # a device table with entries outside 0 .. Ntot behaves as its clamped form
    wild = torch.tensor([-5, 1, 3, 6, 76, 10 ** 12], dtype=torch.int64).cuda()
    rw, fw = _call(lib, pred, gt, wild, valid, flags)
    assert _same(rw, rows) and _same(fw, fe)
    # an empty range gives a zero row; frames that no sequence holds are not written
    re_, fe_ = _call(lib, pred, gt, [6, 6, 76], valid, flags)
    assert not re_[0].any() and _same(re_[1], rows[3]) and (fe_[:6] == FILL).all() and (fe_[76:] == FILL).all() and _same(fe_[6:76], fe[6:76])
    want = ref.score_rows(pred, gt, [6, 6, 76], valid, ref.H36M_PARENTS, flags=flags, frame_fill=FILL)
    assert _holds(re_, want[0], fe_, want[1])
    # frame_err may be null
    assert _same(_call(lib, pred, gt, off, valid, flags, want_frames=False)[0], rows)


def test_exact_cases(lib):
    # pred == gt bit for bit: no error, no velocity error, no acceleration error - exactly
    _, gt, off = ref.related_inputs(ref.LENS, 1, 17, 3, 71)
    rows, fe = _call(lib, np.ascontiguousarray(gt[:, None]), gt, off, None, ref.PROCRUSTES)
    assert not rows[..., [1, 2, 4, 6]].any() and not rows[..., 9:9 + 17].any() and not fe.any() and rows[:, 0, 0].tolist() == list(ref.LENS)
    assert (rows[..., 7] <= 1e-12 * rows[..., 0] * 17).all() and not rows[..., 8].any()
    # pred = an exact similarity transform of gt: the aligned error is rounding, the plain error is not
    pred, gt = ref.similarity_inputs()
    rows, _ = _call(lib, pred, gt, [0, len(gt)], None, ref.PROCRUSTES)
    print(f"\n[score similarity] aligned error per joint and frame {rows[0, 0, 7] / (len(gt) * 17):.2e} (bound 1e-9), plain error {rows[0, 0, 1] / (len(gt) * 17):.3f}")
    assert rows[0, 0, 0] == len(gt) and rows[0, 0, 8] == 0 and rows[0, 0, 7] / (len(gt) * 17) < 1e-9 and rows[0, 0, 1] / (len(gt) * 17) > 0.1
    # a pose whose joints all coincide is counted, and skipped by the alignment; so is a target on one spot
    pred, gt, off = ref.related_inputs([12], 2, 17, 4, 72)
    pred[3, 0, :, :3] = 0.25
    pred[7, 1, :, :3] = pred[7, 1, 2, :3]
    gt[9] = gt[9, 4]
    want = ref.score_rows(pred, gt, off, None, ref.H36M_PARENTS, flags=ref.PROCRUSTES)
    rows, _ = _call(lib, pred, gt, off, None, ref.PROCRUSTES)
    assert rows[0, :, 8].tolist() == [2, 2] and rows[0, :, 0].tolist() == [12, 12] and _holds(rows, want[0])
    # constant bone lengths: every bone's standard deviation is exactly 0, its mean the length
    from manipose_amd import score_poses
    pred, gt, lengths = ref.constant_bones_inputs()
    rec = score_poses(_dev(pred[:, 0]), _dev(gt))
    assert not rec.bone_std.cpu().numpy().any() and np.array_equal(rec.bone_mean.cpu().numpy()[0], lengths)
    assert _holds(rec.rows.cpu().numpy()[:, None], ref.score_rows(pred, gt, None, None, ref.H36M_PARENTS, flags=ref.PROCRUSTES)[0])


def test_entry_point_rejects_bad_arguments_before_any_launch(lib):
    import ctypes as C
    ntot, inner, M = 8, 2, 17
    pred = torch.rand(ntot, inner, M, 4, device="cuda") + 0.1
    gt = torch.rand(ntot, M, 3, device="cuda")
    off = torch.tensor([0, 8], dtype=torch.int64, device="cuda")
    R = int(lib.mp_lift_score_row_doubles(M))
    rows = torch.full((1, inner, R), -1.0, dtype=torch.float64, device="cuda")
    fe = torch.full((ntot, inner), -7.0, device="cuda")
    n = int(lib.mp_lift_score_scratch_doubles(1, inner, M))
    scratch = torch.full((n + 1,), -1.0, dtype=torch.float64, device="cuda")
    good = (C.c_int32 * M)(*ref.H36M_PARENTS)
    p = lambda t: None if t is None else t.data_ptr()

    def call(src=pred, tgt=gt, offs=off, dst=rows, scr=scratch, Ntot=ntot, inner=inner, M=M, Cc=4, S=1, par=good, ps=1.0, gs=1.0, flags=3, doubles=n):
        return lib.mp_lift_score(p(src), Ntot, inner, M, Cc, p(tgt), None, p(offs), S, par, ps, gs, flags, p(dst) if not isinstance(dst, int) else dst, p(fe),
                                 scr if isinstance(scr, int) else p(scr), doubles, None)
    broken = lambda j, v: (C.c_int32 * M)(*[v if k == j else q for k, q in enumerate(ref.H36M_PARENTS)])
    bad = [(dict(src=None), "null"), (dict(tgt=None), "null"), (dict(offs=None), "null"), (dict(dst=None), "null"), (dict(scr=None), "null"),
           (dict(Cc=2), "C="), (dict(Cc=5), "C="), (dict(M=0), "M="), (dict(M=33), "M="), (dict(M=-1), "M="), (dict(M=2, par=None), "M >= 3"),
           (dict(Ntot=0), "Ntot="), (dict(Ntot=-4), "Ntot="), (dict(inner=0), "inner="), (dict(S=0), "S="), (dict(S=-1), "S="), (dict(S=9), "S="),
           (dict(flags=4), "flags"), (dict(flags=-1), "flags"),
           (dict(ps=0.0), "scale"), (dict(ps=-1.0), "scale"), (dict(ps=float("inf")), "scale"), (dict(ps=float("nan")), "scale"),
           (dict(gs=0.0), "scale"), (dict(gs=float("nan")), "scale"), (dict(gs=float("inf")), "scale"),
           (dict(par=broken(0, 0)), "parents[0]"), (dict(par=broken(5, 5)), "parents[5]"), (dict(par=broken(3, 7)), "parents[3]"), (dict(par=broken(9, -1)), "parents[9]"),
           (dict(doubles=n - 1), "scratch"), (dict(doubles=0), "scratch"), (dict(scr=scratch.data_ptr() + 4), "aligned"), (dict(dst=rows.data_ptr() + 4), "aligned"),
           (dict(Ntot=2 ** 62), "too many")]
    for kw, word in bad:
        assert call(**kw) == 1 and word in lib.mp_last_error().decode(), (kw, lib.mp_last_error())
    torch.cuda.synchronize()
    assert bool((rows == -1).all()) and bool((fe == -7).all()) and bool((scratch == -1).all())      # nothing ran
    assert call() == 0 and call(par=None, flags=0) == 0                     # the same call with good arguments
    torch.cuda.synchronize()
    assert bool((rows[..., 0] == ntot).all()) and bool((fe > 0).all()) and bool(torch.isfinite(rows).all())


def test_public_functions(lib):
    from manipose_amd import score_poses, score_traj
    from manipose_amd.lifting import PoseScore, TrajScore
    pred, gt, off = ref.public_inputs()
    valid = np.ones((66, 5), np.uint8)
    valid[25] = 0                                                            # the one-frame sequence: nothing is counted in it
    valid[30, 2] = 0
    want_rows, want_fe = ref.score_rows(pred, gt, off, valid, ref.H36M_PARENTS, flags=ref.PROCRUSTES | ref.ROOT_RELATIVE, frame_fill=-1.0)
    want = ref.fields(want_rows, 17)
    close = lambda a, b: np.allclose(a, b, rtol=1e-9, atol=0, equal_nan=True)
    for table in (off, torch.from_numpy(off).cuda()):
        rec = score_poses(_dev(pred), _dev(gt), table, valid=_dev(valid), root_relative=True, return_frames=True)
        assert isinstance(rec, PoseScore) and all(t.is_cuda and t.dtype == torch.float64 for t in rec[:-1]) and rec.frame_err.dtype == torch.float32
        assert [tuple(t.shape) for t in rec] == [(3, 5)] * 6 + [(3, 5, 17)] + [(3, 5, 16)] * 3 + [(3, 5, 74), (66, 5)]
        got = {k: v.cpu().numpy() for k, v in rec._asdict().items()}
        assert _holds(got["rows"], want_rows, got["frame_err"], want_fe) and all(close(got[k], want[k]) for k in want)
        assert np.isnan(got["mpjpe"][1]).all() and np.isnan(got["p_mpjpe"][1]).all() and np.isnan(got["bone_std"][1]).all() and not got["frames"][1].any()
        assert np.isfinite(got["mpjpe"][[0, 2]]).all() and np.isfinite(got["bone_err"][[0, 2]]).all()
    # 3-D poses, one sequence, no alignment, scales: (S,) fields; a sequence of one frame has no velocity
    one = score_poses(_dev(pred[:, 0, :, :3]), _dev(gt), procrustes=False, pose_scale=2.0, target_scale=3.0)
    w1 = ref.score_rows(pred[:, :1], gt, None, None, ref.H36M_PARENTS, 2.0, 3.0, 0)[0][:, 0]
    assert one.frame_err is None and one.mpjpe.shape == (1,) and one.per_joint.shape == (1, 17) and one.rows.shape == (1, 74) and bool(torch.isnan(one.p_mpjpe).all())
    assert _holds(one.rows.cpu().numpy(), w1) and close(one.mpjpe.cpu().numpy(), ref.fields(w1, 17)["mpjpe"])
    single = score_poses(_dev(pred[25:26, 0, :, :3]), _dev(gt[25:26]))
    assert float(single.frames) == 1 and bool(torch.isnan(single.mpjve)) and bool(torch.isnan(single.accel)) and bool(torch.isfinite(single.p_mpjpe))
    # another number of joints: no skeleton, no bone statistics
    p5, g5, _ = ref.related_inputs([9], 1, 5, 3, 42)
    five = score_poses(_dev(p5[:, 0]), _dev(g5), procrustes=False)
    assert five.bone_mean is None and five.bone_std is None and _holds(five.rows.cpu().numpy()[:, None], ref.score_rows(p5, g5)[0])
    # trajectories
    traj, tgt, toff = ref.related_inputs([20, 1, 30], 4, 1, 3, 43)
    ok = np.ones((51, 4), np.uint8)
    ok[[0, 5, 6, 20, 33], [0, 1, 1, 2, 3]] = 0
    traj[40, 1, 0, 1] = np.nan
    wt = ref.score_rows(traj, tgt, toff, ok)[0]
    rec = score_traj(_dev(traj[:, :, 0]), _dev(tgt[:, 0]), ok=_dev(ok), seq_offset=toff)
    assert isinstance(rec, TrajScore) and all(tuple(t.shape) == (3, 4) and t.dtype == torch.float64 and t.is_cuda for t in rec)
    wf = ref.fields(wt, 1, procrustes=False)
    for k, name in (("frames", "frames"), ("mpjpe", "ate"), ("rmse", "rmse"), ("mpjve", "velocity"), ("accel", "accel")):
        assert close(getattr(rec, name).cpu().numpy(), wf[k])
    assert float(rec.frames[1, 2]) == 0 and bool(torch.isnan(rec.ate[1, 2])) and bool(torch.isnan(rec.velocity[1]).all())
    flat = score_traj(_dev(traj[:, 0, 0]), _dev(tgt[:, 0]))
    assert flat.ate.shape == (1,) and close(flat.ate.cpu().numpy(), ref.fields(ref.score_rows(traj[:, :1], tgt)[0][:, 0], 1, False)["mpjpe"])
    with pytest.raises(RuntimeError, match="S=70"):                         # more sequences than frames: the C entry point's refusal
        score_poses(_dev(pred), _dev(gt), np.zeros(71, np.int64))


# ---- end to end: the tiny fp32 fixture models of lift_fixtures.py ------------------------------------------------------------------------------
def _equal(a, b):
    return np.array_equal(a.cpu().numpy(), b.cpu().numpy(), equal_nan=True)


def _zero_root(t):
    t = t.copy()
    t[:, 0] = 0
    return t


def test_lift_sequences_with_targets(lib):
    from manipose_amd import lift_sequences, score_poses, score_traj
    from manipose_amd.data.ingest import h36m_cameras
    from manipose_amd.lifting import SCORE_FIELDS
    model, T, K = _model("rmcl")
    p2, p3 = _sequences((T - 5, 2 * T, 2 * T + 5), 12)
    for t in p3:
        t[:, 0, 2] += np.float32(4.0)                                        # joint 0: the root's position, in front of the camera
    lens = [len(s) for s in p2]
    off = np.concatenate([[0], np.cumsum(lens)])
    gt0 = _dev(np.concatenate([_zero_root(t) for t in p3]))
    kw = dict(stride=T // 2 + 1, batch=2)

    def holds(score, poses, hyps=None):
        rec = score_poses(torch.cat(poses).contiguous(), gt0, off)
        ok = set(score[0]) >= set(SCORE_FIELDS)
        for s in range(3):
            ok = ok and all(_equal(score[s][f], getattr(rec, f)[s]) for f in SCORE_FIELDS) and float(score[s]["frames"]) == lens[s]
        if hyps is not None:
            hrec = score_poses(torch.cat(hyps).contiguous(), gt0, off, return_frames=True)
            for s in range(3):
                ok = ok and all(_equal(score[s]["hyps"][f], getattr(hrec, f)[s]) for f in SCORE_FIELDS) and score[s]["hyps"]["mpjpe"].shape == (K,)
                best = hrec.frame_err[off[s]:off[s + 1]].double().min(dim=1).values.mean()
                ok = ok and abs(float(score[s]["oracle_mpjpe"]) - float(best)) <= 1e-12 * float(best) and float(best) <= float(score[s]["hyps"]["mpjpe"].min())
        return ok

    poses, hyps, score = lift_sequences(model, p2, targets=p3, return_score=True, return_hyps=True, **kw)
    assert len(score) == 3 and all(isinstance(s, dict) and s["mpjpe"].dtype == torch.float64 and s["mpjpe"].is_cuda and s["per_joint"].shape == (17,) for s in score)
    assert holds(score, poses, hyps) and "traj" not in score[0]
    # ... and against the statement
    want = ref.fields(ref.score_rows(torch.cat(poses).cpu().numpy()[:, None], gt0.cpu().numpy(), off, None, ref.H36M_PARENTS, flags=ref.PROCRUSTES)[0][:, 0], 17)
    assert all(np.allclose(torch.stack([s[k] for s in score]).cpu().numpy(), want[k], rtol=1e-9, atol=0) for k in ("mpjpe", "rmse", "mpjve", "accel", "per_joint", "bone_std"))
    print("\n[lift_sequences score] mpjpe per sequence (m):", [round(float(s["mpjpe"]), 4) for s in score], "oracle:", [round(float(s["oracle_mpjpe"]), 4) for s in score])
    # tensors as targets; targets without return_score score nothing; without hypotheses no "hyps"
    dev_targets = lift_sequences(model, p2, targets=[_dev(t) for t in p3], return_score=True, **kw)
    assert "hyps" not in dev_targets[1][0] and all(_equal(a[f], b[f]) for a, b in zip(dev_targets[1], score) for f in SCORE_FIELDS)
    assert isinstance(lift_sequences(model, p2, targets=p3, **kw), list)
    # scale: divided out, every number stays in metres
    scaled = lift_sequences(model, p2, targets=p3, return_score=True, scale=1000.0, **kw)
    assert all(np.allclose(a["mpjpe"].cpu().numpy(), b["mpjpe"].cpu().numpy(), rtol=1e-5) for a, b in zip(scaled[1], score))
    # rigid: the score is that of the re-assembled poses, whose bones do not vary (float32 poses carry about 3e-8 of rounding at these lengths)
    rp, rh, rs = lift_sequences(model, p2, targets=p3, return_score=True, return_hyps=True, rigid=True, **kw)
    assert holds(rs, rp, rh) and all(float(s["bone_std"].max()) < 1e-6 and float(s["hyps"]["bone_std"].max()) < 1e-6 for s in rs)
    assert float(score[0]["bone_std"].max()) > 1e-5
    # a hypothesis path, smoothed: the score is that of the poses that are emitted
    pp, ps = lift_sequences(model, p2, targets=p3, return_score=True, agg="path", tta=False, smooth_poses=2, **kw)
    assert holds(ps, pp) and not _equal(ps[1]["mpjpe"], score[1]["mpjpe"])
    # placed: the trajectory the world frame uses against the targets' joint 0, over the frames whose fit is ok (filled, when smoothed)
    cams = h36m_cameras()["S11"][:3]
    root = _dev(np.concatenate([t[:, 0] for t in p3]))
    for smooth in (0, 3):
        wp, place, ws = lift_sequences(model, p2, targets=p3, return_score=True, cameras=cams, place=True, frame="world", return_place=True, smooth_traj=smooth, **kw)
        traj = torch.cat([d["traj"] for d in place]).contiguous()
        okay = torch.cat([d["filled" if smooth else "ok"] for d in place]).contiguous()
        rec = score_traj(traj, root, ok=okay, seq_offset=off)
        assert all(_equal(ws[s]["traj"][f], getattr(rec, f)[s]) for s in range(3) for f in rec._fields)
        assert all(_equal(ws[s][f], score[s][f]) for s in range(3) for f in SCORE_FIELDS)       # placing moves poses rigidly: scored before it
    # targets=None: not a bit changes
    for extra in (dict(return_hyps=True), dict(rigid=True, return_bones=True, return_hyps=True)):
        a = lift_sequences(model, p2, **extra, **kw)
        b = lift_sequences(model, p2, targets=None, return_score=False, **extra, **kw)
        c = lift_sequences(model, p2, targets=p3, return_score=True, **extra, **kw)
        assert len(c) == len(a) + 1 and all(torch.equal(x, y) for r, q in zip(a, b) for x, y in zip(r, q)) and all(torch.equal(x, y) for r, q in zip(a, c) for x, y in zip(r, q))


def test_score_lift_entry_point(lib, tmp_path, monkeypatch):
    sys.path.insert(0, os.path.join(ROOT, "hpe"))
    from _entry import LIFT_SUFFIXES, load_config, run, synthetic_sequences_3d
    monkeypatch.chdir(tmp_path)
    argv = ["run.train=false", "run.test=false", "run.lift=true", "lift.stride=14", "train.batch_size_test=4", "data.seq_len=27", "model.channels=64",
            "model.layers=2", "model.nheads=4", "model.channels_seg=32", "model.layers_seg=1", "model.nheads_seg=4", "multi_hyp.n_hyp=3",
            "data.synthetic_sequences=3", "model.precision=fp32", "lift.score=true"]
    run(argv)
    out = os.path.join(str(tmp_path), "default")
    z = np.load(os.path.join(out, "lift.npz"))
    keys = [f"synthetic_{i:03d}" for i in range(3)]
    assert sorted(z.files) == keys and not any(f.endswith(LIFT_SUFFIXES) for f in z.files)          # exactly the keys it has without lift.score
    rows = list(csv.reader(open(os.path.join(out, "lift_score.csv"))))
    assert rows[0] == ["act", "frames", "mpjpe", "p_mpjpe", "mpjve", "accel", "bone_std", "bone_err"] and [r[0] for r in rows[1:]] == keys + ["average"]
    targets = synthetic_sequences_3d(load_config(argv), load_config(argv).run.seed)
    total = 0.0
    for i, k in enumerate(keys):
        n = 27 * 4 + 37 * i + 11
        gt = _zero_root(targets[k][0])
        assert z[k].shape == (n, 17, 3) and gt.shape == (n, 17, 3) and float(rows[1 + i][1]) == n
        f = ref.fields(ref.score_rows(z[k][:, None], gt, None, None, ref.H36M_PARENTS, flags=ref.PROCRUSTES)[0][0, 0], 17)
        for col, key in ((2, "mpjpe"), (3, "p_mpjpe"), (4, "mpjve"), (5, "accel")):
            assert abs(float(rows[1 + i][col]) - 1000.0 * float(f[key])) <= 1e-6 * 1000.0 * float(f[key]), (k, key)
        assert abs(float(rows[1 + i][6]) - 1000.0 * float(f["bone_std"].mean())) <= 1e-6 * 1000.0 * float(f["bone_std"].mean())
        total += n * float(rows[1 + i][2])
    frames = sum(27 * 4 + 37 * i + 11 for i in range(3))
    assert float(rows[4][1]) == frames and abs(float(rows[4][2]) - total / frames) <= 1e-9 * total / frames
    joints = list(csv.reader(open(os.path.join(out, "lift_score_joints.csv"))))
    assert len(joints) == 5 and len(joints[0]) == 18 and abs(np.mean([float(v) for v in joints[1][1:]]) - float(rows[1][2])) <= 1e-9 * float(rows[1][2])

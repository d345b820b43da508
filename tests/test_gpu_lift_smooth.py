"""Smoothing lifted sequences in time on the device: mp_lift_smooth against the float64 statement (lift_smooth_ref.py), its bit-exact
properties, exact polynomial reproduction, argument errors, gap filling through place_poses + smooth_traj, lift_sequences(smooth_poses= /
smooth_traj=) for the three architectures, and run.lift.

The bound, everywhere a float32 is compared with float64: |x - x64| <= 2^-23 max(1, |x64|), the project's lifting bound.  The kernel computes
in fp64 between its float32 loads and its one float32 store, so against the float64 statement ON THE SAME float32 INPUTS only the final rounding
(2^-24 relative) remains; the statement itself stays within 1e-3 of the bound's unit of an independent lstsq solve on these very inputs
(test_lift_smooth_host.py).  The bound is not measured from the kernel."""
import os
import sys

import numpy as np
import pytest
import torch

import lift_place_ref as place_ref
import lift_smooth_ref as ref
from lift_fixtures import fixture_model as _model, same as _same, sequences_2d as _sequences

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OFF, NTOT = ref.OFF, ref.NTOT


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _call(lib, x, valid, off, R, deg, taper, want_filled=True):
    """mp_lift_smooth itself on host arrays: (out, filled, the input as the device holds it afterwards)"""
    from manipose_amd import _lib
    d_in, d_out = _dev(x), torch.full(x.shape, -7.0, device="cuda")
    d_valid = _dev(valid) if valid is not None else None
    d_off = off if torch.is_tensor(off) else _dev(np.asarray(off, np.int64))
    d_filled = torch.full(x.shape[:2], 9, dtype=torch.uint8, device="cuda") if want_filled else None
    ntot, inner, M, C = x.shape
    _lib.check(lib.mp_lift_smooth(_lib.ptr(d_in), _lib.ptr(d_out), ntot, inner, M, C, _lib.ptr(d_valid), _lib.ptr(d_off), int(d_off.numel()) - 1, R, deg,
                                  ref.TAPER[taper], _lib.ptr(d_filled), None), "mp_lift_smooth")
    torch.cuda.synchronize()
    return d_out.cpu().numpy(), d_filled.cpu().numpy() if want_filled else None, d_in.cpu().numpy()


@pytest.mark.parametrize("case", ref.GPU_CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_against_fp64(lib, case):
    inner, M, C, R, deg, taper = case
    x, valid = ref.smooth_inputs(inner, M, C, R, deg, ref.case_seed(case))
    want, want_filled = ref.smooth_all(x, valid, OFF, R, deg, taper)
    got, filled, x_after = _call(lib, x, valid, OFF, R, deg, taper)
    assert np.array_equal(filled, want_filled) and (filled == 0).any() and filled.any()
    print(f"\n[smooth {case}] worst error = {ref.worst(got[..., :3], want[..., :3]):.3f} x the bound 2^-23 max(1, |x|); "
          f"{int((filled == 0).sum())} of {filled.size} frames not filled")
    assert ref.within(got[..., :3], want[..., :3]).all()
    assert _same(x_after, x)                                              # the input is unmodified
    if C == 4:
        assert _same(got[..., 3], x[..., 3])                              # the score channel, bit for bit
    assert _same(got[filled == 0], x[filled == 0])                        # no valid tap: the input's bits
    again, filled2, _ = _call(lib, x, valid, torch.from_numpy(OFF).cuda(), R, deg, taper)
    assert _same(again, got) and _same(filled2, filled)                   # two calls, a device table: identical bits


@pytest.mark.parametrize("inner,M,C,R", [(1, 1, 3, 2), (5, 17, 4, 8), (2, 32, 4, 64)])
def test_bit_exact_properties(lib, inner, M, C, R):
    x, valid = ref.smooth_inputs(inner, M, C, R, 2, seed=50 + R)
    got, filled, _ = _call(lib, x, valid, OFF, R, 2, "biweight")
    # sequence s + 1 changes in data and validity: sequence s keeps its bits (and so does every sequence before it)
    x2, valid2 = x.copy(), valid.copy()
    x2[OFF[3]:] = x2[OFF[3]:] * np.float32(-3.0) + np.float32(1.0)
    valid2[OFF[3]:] = 1 - valid2[OFF[3]:]
    other, filled_o, _ = _call(lib, x2, valid2, OFF, R, 2, "biweight")
    assert _same(other[:OFF[3]], got[:OFF[3]]) and _same(filled_o[:OFF[3]], filled[:OFF[3]]) and not _same(other[OFF[3]:], got[OFF[3]:])
    # a device table with entries outside 0 .. Ntot is clamped to the frames the caller vouches for
    wild, filled_w, _ = _call(lib, x, valid, torch.tensor([-5, 1, 3, 73, 10 ** 12], dtype=torch.int64).cuda(), R, 2, "biweight")
    assert _same(wild, got) and _same(filled_w, filled)
    # a valid of all ones equals a null valid; filled may be null
    ones, filled1, _ = _call(lib, x, np.ones_like(valid), OFF, R, 2, "biweight")
    null, filled0, _ = _call(lib, x, None, OFF, R, 2, "biweight")
    assert _same(ones, null) and filled1.all() and filled0.all()
    bare, none, _ = _call(lib, x, valid, OFF, R, 2, "biweight", want_filled=False)
    assert none is None and _same(bare, got)
    # any non-zero byte is valid
    loud, filled_l, _ = _call(lib, x, valid * np.uint8(200), OFF, R, 2, "biweight")
    assert _same(loud, got) and _same(filled_l, filled)
    # the value on an invalid tap is never looked at
    poisoned = x.copy()
    poisoned[valid == 0] = np.nan
    clean, filled_p, _ = _call(lib, poisoned, valid, OFF, R, 2, "biweight")
    keep = filled == 1
    assert _same(filled_p, filled) and _same(clean[keep][..., :3], got[keep][..., :3]) and np.isfinite(clean[keep][..., :3]).all()


@pytest.mark.parametrize("R,taper", [(1, "uniform"), (2, "biweight"), (8, "uniform"), (64, "biweight")])
def test_polynomials_are_reproduced(lib, R, taper):
    """the integer-valued inputs of the host test: wherever the fit has the full degree the device returns the input within the bound"""
    print()
    for deg in (0, 1, 2):
        x = ref.polynomial_inputs(2, 3, 4, deg)
        valid = ref.planted_valid(2, R, deg, seed=5)
        _, want_filled, used = ref.smooth_all(x, valid, OFF, R, deg, taper, return_degree=True)
        got, filled, _ = _call(lib, x, valid, OFF, R, deg, taper)
        full = used == deg
        print(f"[polynomial R={R} deg={deg} {taper}] worst error = {ref.worst(got[full][..., :3], x[full][..., :3]):.3f} x the bound at {int(full.sum())} frames")
        assert full.sum() > 100 and np.array_equal(filled, want_filled) and ref.within(got[full][..., :3], x[full][..., :3]).all()


def test_entry_point_rejects_bad_arguments_before_any_launch(lib):
    x = torch.zeros(8, 2, 17, 3, device="cuda")
    out = torch.full((8, 2, 17, 3), -1.0, device="cuda")
    big = torch.full((2 * 8 * 2 * 17 * 3,), -1.0, device="cuda")
    off = torch.tensor([0, 8], dtype=torch.int64, device="cuda")
    valid = torch.ones(8, 2, dtype=torch.uint8, device="cuda")
    filled = torch.full((8, 2), 7, dtype=torch.uint8, device="cuda")
    p = lambda t: None if t is None else t.data_ptr()

    def call(src=x, dst=out, offs=off, Ntot=8, inner=2, M=17, C=3, S=1, R=2, deg=2, taper=0):
        return lib.mp_lift_smooth(src if isinstance(src, int) else p(src), dst if isinstance(dst, int) else p(dst), Ntot, inner, M, C, p(valid),
                                  p(offs), S, R, deg, taper, p(filled), None)
    n = 8 * 2 * 17 * 3 * 4
    bad = [dict(src=None), dict(dst=None), dict(offs=None),
           dict(dst=x), dict(src=big.data_ptr(), dst=big.data_ptr() + n - 4), dict(src=big.data_ptr() + 4, dst=big.data_ptr()),      # overlapping ranges
           dict(R=0), dict(R=65), dict(R=-1), dict(deg=-1), dict(deg=3), dict(taper=-1), dict(taper=2),
           dict(M=0), dict(M=33), dict(C=2), dict(C=5),
           dict(Ntot=0), dict(Ntot=-3), dict(inner=0), dict(S=0), dict(S=-1), dict(S=9),
           dict(Ntot=2 ** 40, inner=2 ** 10), dict(Ntot=2 ** 62)]
    for kw in bad:
        assert call(**kw) == 1, (kw, lib.mp_last_error())
    torch.cuda.synchronize()
    assert bool((out == -1).all()) and bool((big == -1).all()) and bool((filled == 7).all()) and torch.count_nonzero(x).item() == 0      # nothing ran
    assert call() == 0 and call(src=big.data_ptr(), dst=big.data_ptr() + n) == 0           # the same call with good arguments; adjacent ranges
    torch.cuda.synchronize()
    assert bool((out == 0).all()) and bool((filled == 1).all())


def _smooth_scene(seed, n=120, noise=0.01):
    """synthetic_scene's poses on a SMOOTH true trajectory, noisy keypoints, and a few frames whose keypoints all sit on one spot"""
    intr = np.asarray([c["intrinsic"] for c in _cams(1)], np.float32)
    poses, _, _, _ = place_ref.synthetic_scene([n], 1, 3, intr, seed, noise)
    g = np.random.default_rng(seed + 1)
    f = np.arange(n, dtype=np.float64)
    t_true = np.stack([0.8 * np.sin(f / 25.0), 0.5 * np.cos(f / 31.0), 5.0 + 1.5 * np.sin(f / 40.0 + 1.0)], axis=1).astype(np.float32)
    P = poses[:, 0, :, :3].astype(np.float64) + t_true[:, None, :].astype(np.float64)
    fc, cc = intr[0, 0:2].astype(np.float64), intr[0, 2:4].astype(np.float64)
    kp = (fc * (P[..., :2] / P[..., 2:3]) + cc + noise * g.standard_normal((n, 17, 2))).astype(np.float32)
    holes = [0, 40, 41, 42, 77, n - 1]
    for h in holes:
        kp[h] = kp[h, 3]
    return poses[:, 0], kp, t_true, intr, holes


def _cams(n=3):
    from manipose_amd.data.ingest import h36m_cameras
    return h36m_cameras()["S11"][:n]


def test_gaps_are_filled_through_the_public_functions(lib):
    from manipose_amd import place_poses, smooth_traj
    R = 6
    poses, kp, t_true, intr, holes = _smooth_scene(seed=3)
    traj, reproj, ok = place_poses(_dev(poses), _dev(kp), intr)
    h_traj, h_ok = traj.cpu().numpy(), ok.cpu().numpy()
    assert h_ok.sum() == len(poses) - len(holes) and not h_ok[holes].any() and not h_traj[holes].any()       # ok = 0 and traj = 0 exactly there
    want, want_filled = ref.smooth_all(h_traj[:, None, None, :], h_ok[:, None], None, R, 2, "uniform")
    smoothed, filled = smooth_traj(traj, ok, radius=R)
    assert smoothed.shape == traj.shape and smoothed.dtype == torch.float32 and filled.shape == ok.shape and filled.dtype == torch.uint8
    assert smoothed.data_ptr() != traj.data_ptr() and _same(traj.cpu().numpy(), h_traj)       # a new tensor
    got = smoothed.cpu().numpy()
    assert bool(filled.all()) and want_filled.all() and ref.within(got, want[:, 0, 0]).all()
    t64 = t_true.astype(np.float64)
    miss_filled = np.linalg.norm(got[holes] - t64[holes], axis=1)
    keep = h_ok == 1
    rms_raw = np.sqrt(((h_traj[keep] - t64[keep]) ** 2).sum(-1).mean())
    rms_smooth = np.sqrt(((got[keep] - t64[keep]) ** 2).sum(-1).mean())
    rms_statement = np.sqrt(((want[:, 0, 0][keep] - t64[keep]) ** 2).sum(-1).mean())
    print(f"\n[gap filling R={R}] filled frames: {miss_filled.max():.3f} m from the truth at most ((0, 0, 0): {np.linalg.norm(t64[holes], axis=1).min():.3f} m "
          f"at least); RMS over the ok frames: raw fit {rms_raw:.4f} m, smoothed {rms_smooth:.4f} m (the statement alone {rms_statement:.4f} m)")
    assert (miss_filled < np.linalg.norm(t64[holes], axis=1)).all()       # nearer to the truth than the (0, 0, 0) the fit left
    assert rms_statement < rms_raw and rms_smooth < rms_raw
    # the (Ntot, inner, 3) form, several sequences, a device table: the statement again
    t3 = np.stack([h_traj, h_traj[::-1]], axis=1).copy()
    ok3 = np.stack([h_ok, h_ok[::-1]], axis=1).copy()
    off = np.array([0, 50, 120], np.int64)
    s3, f3 = smooth_traj(_dev(t3), _dev(ok3), torch.from_numpy(off).cuda(), radius=1, degree=1, taper="biweight")
    w3, wf3 = ref.smooth_all(t3[:, :, None, :], ok3, off, 1, 1, "biweight")
    assert s3.shape == (120, 2, 3) and f3.shape == (120, 2) and np.array_equal(f3.cpu().numpy(), wf3) and not wf3.all()       # (frames 40..42 invalid: R = 1 cannot reach 41)
    assert ref.within(s3.cpu().numpy(), w3[:, :, 0]).all() and _same(s3.cpu().numpy()[wf3 == 0], t3[wf3 == 0])
    all_valid, f_all = smooth_traj(_dev(t3), None, off, radius=2)
    assert bool(f_all.all()) and ref.within(all_valid.cpu().numpy(), ref.smooth_all(t3[:, :, None, :], None, off, 2)[0][:, :, 0]).all()


def test_smooth_poses_public_function(lib):
    from manipose_amd import smooth_poses
    g = np.random.default_rng(4)
    x3 = g.standard_normal((NTOT, 17, 3)).astype(np.float32)
    x4 = g.standard_normal((NTOT, 3, 17, 4)).astype(np.float32)
    for x, kw in ((x3, dict(radius=4)), (x4, dict(radius=3, degree=1, taper="biweight"))):
        t = _dev(x)
        r = smooth_poses(t, OFF, **kw)
        assert r.shape == t.shape and r.data_ptr() != t.data_ptr() and _same(t.cpu().numpy(), x)
        want = ref.smooth_all(x.reshape(NTOT, -1, 17, x.shape[-1]), None, OFF, kw["radius"], kw.get("degree", 2), kw.get("taper", "uniform"))[0]
        got = r.cpu().numpy().reshape(want.shape)
        assert ref.within(got[..., :3], want[..., :3]).all()
        if x.shape[-1] == 4:
            assert _same(got[..., 3], x[..., 3])
        assert _same(smooth_poses(_dev(x), torch.from_numpy(OFF).cuda(), **kw).cpu().numpy(), r.cpu().numpy())
    one = smooth_poses(_dev(x3[:9]), radius=2, degree=2)                  # one sequence by default: the classical taps on interior frames
    taps = np.array([-3, 12, 17, 12, -3]) / 35.0
    want = sum(k * x3[2 + t:7 + t].astype(np.float64) for k, t in zip(taps, range(-2, 3)))
    assert ref.within(one.cpu().numpy()[2:7], want).all()


# ---- end to end: the tiny fp32 fixture models of lift_fixtures.py ------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["rmcl", "manifold", "mixste"])
def test_lift_sequences_end_to_end(lib, kind):
    from manipose_amd import camera_table, lift_sequences, project_rigid, smooth_poses, to_world
    model, T, K = _model(kind)
    p2 = _sequences(T)
    lens = [len(s) for s in p2]
    cams = _cams()
    intr, quat, trans = camera_table(cams)
    hyp = kind == "rmcl"
    R = 3
    kw = dict(stride=T // 2 + 1, tta=True, batch=2, return_hyps=hyp)
    plain = lift_sequences(model, p2, **kw)
    off_res = lift_sequences(model, p2, smooth_poses=0, smooth_traj=0, **kw)
    for a, b in zip(plain if hyp else (plain,), off_res if hyp else (off_res,)):
        assert all(torch.equal(x, y) for x, y in zip(a, b))               # the defaults and explicit zeros: not a bit changes
    base, base_h = (plain[0], plain[1]) if hyp else (plain, None)
    # smooth_poses: the public function applied to the plain output, bit for bit; hypotheses too, scores untouched
    res = lift_sequences(model, p2, smooth_poses=R, smooth_taper="biweight", **kw)
    sm, sm_h = (res[0], res[1]) if hyp else (res, None)
    want = [smooth_poses(b.clone(), radius=R, taper="biweight") for b in base]
    assert all(torch.equal(a, b) for a, b in zip(sm, want)) and not any(torch.equal(a, b) for a, b in zip(sm, base))
    if hyp:
        want_h = [smooth_poses(b.clone(), radius=R, taper="biweight") for b in base_h]
        assert all(torch.equal(a, b) for a, b in zip(sm_h, want_h)) and all(torch.equal(a[..., 3], b[..., 3]) for a, b in zip(sm_h, base_h))
    # with rigid: project_rigid of that, with the table the call used
    res = lift_sequences(model, p2, smooth_poses=R, smooth_taper="biweight", rigid=True, lengths="measured", return_bones=True, **kw)
    for s in range(3):
        assert torch.equal(res[0][s], project_rigid(want[s].clone(), res[-1][s]))
        if hyp:
            assert torch.equal(res[1][s], project_rigid(want_h[s].clone(), res[-1][s]))
    # smooth_traj: traj_fit is the un-smoothed run's traj, traj the statement on (traj_fit, ok), the world poses to_world with the smoothed one
    placed = dict(cameras=cams, place=True, return_place=True)
    raw = lift_sequences(model, p2, **placed, **kw)
    res = lift_sequences(model, p2, smooth_traj=R, smooth_degree=1, **placed, **kw)
    assert all(torch.equal(a, b) for a, b in zip(res[0], base))           # place alone leaves the poses where they are
    world = lift_sequences(model, p2, smooth_traj=R, smooth_degree=1, frame="world", **placed, **kw)
    keys = ["traj", "reproj", "ok", "traj_fit", "filled"]
    for s in range(3):
        d, d_raw, d_w = res[-1][s], raw[-1][s], world[-1][s]
        assert sorted(d) == sorted(keys + (["hyps_" + k for k in keys] if hyp else []))
        for pre, inner in (("", ()), ("hyps_", (K,))) if hyp else (("", ()),):
            fit, ok = d[pre + "traj_fit"].cpu().numpy(), d[pre + "ok"].cpu().numpy()
            assert fit.shape == (lens[s],) + inner + (3,) and d[pre + "filled"].shape == (lens[s],) + inner and d[pre + "filled"].dtype == torch.uint8
            assert _same(fit, d_raw[pre + "traj"].cpu().numpy()) and _same(ok, d_raw[pre + "ok"].cpu().numpy())
            assert _same(d[pre + "reproj"].cpu().numpy(), d_raw[pre + "reproj"].cpu().numpy())
            w, wf = ref.smooth_all(fit.reshape(lens[s], -1, 1, 3), ok.reshape(lens[s], -1), None, R, 1, "uniform")
            assert ref.within(d[pre + "traj"].cpu().numpy().reshape(w.shape), w).all() and np.array_equal(d[pre + "filled"].cpu().numpy().reshape(wf.shape), wf)
            assert _same(d_w[pre + "traj"].cpu().numpy(), d[pre + "traj"].cpu().numpy())
        t_s = trans[s]
        assert torch.equal(world[0][s], to_world(base[s].clone(), quat[s], t_s, d["traj"]))
        if hyp:
            assert torch.equal(world[1][s], to_world(base_h[s].clone(), quat[s], t_s, d["hyps_traj"]))
    # both at once, with the floor: runs, and the order of the stages is smooth -> rigid -> place -> smooth -> world
    full = lift_sequences(model, p2, smooth_poses=R, smooth_traj=2, rigid=True, lengths="measured", frame="world", floor=True, **placed, **kw)
    assert all(r[..., 2].min().item() == 0.0 and torch.isfinite(r).all() for r in full[0]) and "floor" in full[-1][0] and "filled" in full[-1][0]


def test_smooth_lift_entry_point(lib, tmp_path, monkeypatch):
    sys.path.insert(0, os.path.join(ROOT, "hpe"))
    from _entry import LIFT_SUFFIXES, run
    monkeypatch.chdir(tmp_path)
    common = ["run.train=false", "run.test=false", "run.lift=true", "lift.stride=14", "train.batch_size_test=4", "data.seq_len=27", "model.channels=64",
              "model.layers=2", "model.nheads=4", "model.channels_seg=32", "model.layers_seg=1", "model.nheads_seg=4", "multi_hyp.n_hyp=3",
              "data.synthetic_sequences=3", "model.precision=fp32", "lift.hyps=true", "lift.place=true"]
    run(common)
    plain = dict(np.load(os.path.join(str(tmp_path), "default", "lift.npz")))
    run(common + ["lift.smooth_poses=4", "lift.smooth_traj=6", "lift.smooth_degree=1", "lift.smooth_taper=biweight"])
    z = np.load(os.path.join(str(tmp_path), "default", "lift.npz"))
    keys = [f"synthetic_{i:03d}" for i in range(3)]
    new = ["__traj_fit", "__filled", "__hyps_traj_fit", "__hyps_filled"]
    assert sorted(z.files) == sorted(list(plain) + [k + s for k in keys for s in new]) and not any(k + s in plain for k in keys for s in new)
    assert all(f == k or f[len(k):] in LIFT_SUFFIXES for f in z.files for k in keys if f.startswith(k))
    for i, k in enumerate(keys):
        n = 27 * 4 + 37 * i + 11
        assert z[k].shape == (n, 17, 3) and z[k + "__hyps"].shape == (n, 3, 17, 4) and z[k + "__traj"].shape == (n, 3)
        assert z[k + "__traj_fit"].shape == (n, 3) and z[k + "__traj_fit"].dtype == np.float32
        assert z[k + "__filled"].shape == (n,) and z[k + "__filled"].dtype == np.uint8
        assert z[k + "__hyps_traj_fit"].shape == (n, 3, 3) and z[k + "__hyps_filled"].shape == (n, 3) and z[k + "__hyps_filled"].dtype == np.uint8
        assert not _same(z[k], plain[k]) and _same(z[k + "__hyps"][..., 3], plain[k + "__hyps"][..., 3])      # smoothed poses, untouched scores
        want = ref.smooth_all(z[k + "__traj_fit"][:, None, None, :], z[k + "__ok"][:, None], None, 6, 1, "biweight")
        assert ref.within(z[k + "__traj"], want[0][:, 0, 0]).all() and np.array_equal(z[k + "__filled"], want[1][:, 0])

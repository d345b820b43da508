"""Refining placed root trajectories under the full camera model on the device: mp_lift_place_refine against the float64 statement of its rule
(lift_refine_ref.py), against mp_lift_place and the recorded bits of both from before they shared a kernel (zero steps: identical bits), the recovery of a known translation that the linear fit misses, weights, the
guards of the iteration, the start mode (reproject_poses, warm starts), sequences alone and together, argument errors, and lift_sequences /
run.lift with place_refine.

The bound, everywhere a float32 is compared with float64: |x - x64| <= 2^-23 max(1, |x64|) (lift_place_ref.TOL).  The kernel computes in fp64 between
its float32 loads and stores and the normal matrix H is well conditioned (det / (H00 H11 H22) >= 1e-3 on these scenes), so against the float64
statement ON THE SAME float32 INPUTS only fp64 noise and the final rounding remain; the bound is not measured from the kernel.  ok and steps are
compared for equality: test_lift_refine_host.py shows every accept / reject decision of these scenes at least 1e-9 relative from its threshold."""
import os
import sys

import numpy as np
import pytest
import torch

import lift_place_ref as place
import lift_refine_ref as ref
from lift_fixtures import fixture_model as _model, same as _same, sequences_2d as _sequences, to_numpy as _np

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NTOT = int(sum(ref.LENS))


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _refine(poses, kp, intr, off=None, weights=None, distort=True, iters=0):
    from manipose_amd import place_poses
    res = place_poses(_dev(poses), _dev(kp), intr, off, weights, distort, refine=iters, return_steps=True)
    torch.cuda.synchronize()
    return [r.cpu().numpy() for r in res]


def _raw(lib, poses, kp, intr, off, iters, start=None, start_ok=None, distort=1):
    """the entry point itself on (Ntot, inner, J, C) poses: (traj, reproj, ok, steps) as numpy"""
    from manipose_amd.lifting import _place_refine
    res = _place_refine(lib, _dev(poses), _dev(kp), _dev(np.asarray(off, np.int64)), len(off) - 1, _dev(intr), None, distort, iters,
                        None if start is None else _dev(start), None if start_ok is None else _dev(start_ok))
    torch.cuda.synchronize()
    return [r.cpu().numpy() for r in res]


def _check(tag, got, want):
    print(f"[{tag}] worst error = {place.worst(got, want):.3f} x the bound 2^-23 max(1, |x|)")
    assert place.within(got, want).all()


def _check_all(tag, got, want):
    _check(tag + ": traj", got[0], want[0])
    _check(tag + ": reproj", got[1], want[1])
    assert np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3]), tag


@pytest.mark.parametrize("iters", [1, 4, 16])
@pytest.mark.parametrize("distort", [True, False])
@pytest.mark.parametrize("inner,ch", [(1, 3), (1, 4), (5, 3), (5, 4)])
def test_refine_against_fp64(lib, inner, ch, distort, iters):
    from manipose_amd import place_poses
    intr = ref.s11_intrinsics()
    poses, kp, t_true, off = ref.fp64_scene(inner, ch)
    given = poses[:, 0] if (inner, ch) == (1, 3) else poses               # the (Ntot, J, 3) form of the public function
    want = ref.refine_all(given, kp, intr, off, None, distort, iters)
    print(f"\n[refine inner={inner} C={ch} distort={int(distort)} iters={iters}] steps taken: {np.bincount(want[3].ravel()).tolist()}, "
          f"mean reprojection error {want[1].mean():.4f}")
    assert want[2].all() and (want[3] == iters).all()                     # the construction is ok = 1 everywhere and never refuses a step
    t = _dev(given)
    got = [r.cpu().numpy() for r in place_poses(t, _dev(kp), intr, off, None, distort, refine=iters, return_steps=True)]
    assert got[0].shape == want[0].shape and got[0].dtype == np.float32 and got[1].shape == want[1].shape and got[1].dtype == np.float32
    assert got[2].shape == want[2].shape and got[2].dtype == np.uint8 and got[3].shape == want[3].shape and got[3].dtype == np.uint8
    _check_all("refine", got, want)
    assert _same(t.cpu().numpy(), given)                                  # poses are read only (the score channel included)
    again = _refine(given, kp, intr, torch.from_numpy(off).cuda(), None, distort, iters)      # a device offset table; and: two calls, identical bits
    assert all(_same(a, b) for a, b in zip(again, got))
    three = place_poses(_dev(given), _dev(kp), intr, off, None, distort, refine=iters)        # without return_steps: the same three tensors
    assert len(three) == 3 and all(_same(a.cpu().numpy(), b) for a, b in zip(three, got))


def _raw_place(lib, poses, kp, intr, off, weights, distort):
    """mp_lift_place itself (no Python launcher calls it any more) on (Ntot, inner, J, C) poses: (traj, reproj, ok) as numpy"""
    from manipose_amd import _lib
    p4, k, o, cam, w = _dev(poses), _dev(kp), _dev(np.asarray(off, np.int64)), _dev(intr), None if weights is None else _dev(weights)
    ntot, inner, J, ch = p4.shape
    traj, reproj = torch.empty(ntot, inner, 3, device="cuda"), torch.empty(ntot, inner, device="cuda")
    ok = torch.empty(ntot, inner, dtype=torch.uint8, device="cuda")
    _lib.check(lib.mp_lift_place(_lib.ptr(p4), ntot, inner, J, ch, _lib.ptr(k), _lib.ptr(o), len(off) - 1, _lib.ptr(cam), _lib.ptr(w), int(distort),
                                 _lib.ptr(traj), _lib.ptr(reproj), _lib.ptr(ok), _lib.stream_ptr()), "mp_lift_place")
    torch.cuda.synchronize()
    return [r.cpu().numpy() for r in (traj, reproj, ok)]


def test_zero_steps_have_the_bits_of_mp_lift_place(lib):
    """mp_lift_place and mp_lift_place_refine are one kernel behind two entry points, so comparing them with each other no longer guards the fit.
    tests/golden/lift_place_bits.npz holds the outputs of the commit BEFORE the two kernels were merged, recorded on gfx950 with this toolchain:
    of its own mp_lift_place kernel on the three scenes below (distort both ways, weights none and uneven), and of mp_lift_place_refine on
    fp64_scene(5, 4) at iters 0, 4 and 16 from the linear fit and at iters 0 from a given start / start_ok.  Both entry points must reproduce
    those bits: a change to the camera model, the degenerate-fit rule or the order of a sum shows here."""
    from manipose_amd import place_poses
    gold = np.load(os.path.join(ROOT, "tests", "golden", "lift_place_bits.npz"))
    intr = ref.s11_intrinsics()
    poses, kp, _, off = ref.fp64_scene(5, 4)
    uneven = np.random.default_rng(9).uniform(0.25, 4.0, 17).astype(np.float32)
    scenes = (("full", poses, kp, intr, off), ("slice", poses[:, 0, :, :3].copy(), kp, intr, off), ("guards",) + ref.guards_scene()[2:] + (None,))
    for name, given, k, cam, o in scenes:
        for distort in (True, False):
            for wname, w in (("none", None), ("uneven", uneven)):
                want = [r.cpu().numpy() for r in place_poses(_dev(given), _dev(k), cam, o, w, distort)]
                got = _refine(given, k, cam, o, w, distort, 0)
                assert all(_same(a, b) for a, b in zip(got[:3], want)) and not got[3].any()
                rec = [gold[f"place_{name}_d{int(distort)}_{wname}_{field}"] for field in ("traj", "reproj", "ok")]
                assert rec[0].dtype == np.float32 and rec[1].dtype == np.float32 and rec[2].dtype == np.uint8
                p4 = given[:, None] if given.ndim == 3 else given
                one = _raw_place(lib, p4, k, cam, [0, len(given)] if o is None else o, w, distort)
                for a, b, r in zip(one, got, rec):                        # mp_lift_place, mp_lift_place_refine at zero steps, the recording
                    assert _same(a, r) and _same(b.reshape(r.shape), r), (name, distort, wname)
    assert not want[2].all() and want[2].any()                            # (the last scene holds degenerate fits and a joint behind the camera)
    fields = ("traj", "reproj", "ok", "steps")
    for iters in (0, 4, 16):                                              # the steps too: the same instructions as before the merge
        got = _raw(lib, poses, kp, intr, off, iters)
        assert all(_same(a, gold[f"refine_i{iters}_{field}"]) for a, field in zip(got, fields)), iters
        assert (got[3] == iters).all()
    start, start_ok = gold["refine_start_in"], gold["refine_start_ok_in"]
    got = _raw(lib, poses, kp, intr, off, 0, start, start_ok)
    assert all(_same(a, gold[f"refine_start_{field}"]) for a, field in zip(got, fields))
    assert not start_ok.all() and not np.isfinite(start).all() and got[2].any() and not got[2].all()      # (skipped poses are in the recording)


def test_recovery_of_a_translation_the_linear_fit_misses(lib):
    from manipose_amd import place_poses
    intr = ref.s11_intrinsics()
    poses, kp, t_true, off = ref.recovery_scene()
    lin = [r.cpu().numpy() for r in place_poses(_dev(poses[:, 0]), _dev(kp), intr, off)]
    traj, err, ok, steps = _refine(poses[:, 0], kp, intr, off, iters=3)
    miss_lin, miss = np.abs(lin[0].astype(np.float64) - t_true).max(), np.abs(traj.astype(np.float64) - t_true).max()
    print(f"\n[recovery] linear fit: max |traj - t_true| = {miss_lin:.3f} m (at least 0.1); 3 steps: {miss:.2e} m (bound 2e-6), max reproj = {err.max():.2e} "
          f"(bound 1e-6)")
    assert lin[2].all() and miss_lin >= 0.1
    assert ok.all() and (steps == 3).all() and miss <= 2e-6 and err.max() <= 1e-6


def test_weights(lib):
    intr = ref.s11_intrinsics()
    poses, kp, _, off = ref.small_scene()
    keep = np.arange(17) % 3 != 0
    zero_some = np.where(keep, 1.0, 0.0).astype(np.float32)
    got = _refine(poses, kp, intr, off, zero_some, iters=4)
    want = ref.refine_all(poses[:, :, keep], kp[:, keep], intr, off, iters=4)      # the statement on the remaining joints alone
    print()
    _check_all("zero weights", got, want)
    poisoned = kp.copy()
    poisoned[:, ~keep] = np.nan                                           # a joint of weight 0 is not looked at
    assert all(_same(a, b) for a, b in zip(_refine(poses, poisoned, intr, off, zero_some, iters=4), got))
    uneven = np.random.default_rng(9).uniform(0.25, 4.0, 17).astype(np.float32)
    got = _refine(poses, kp, intr, off, torch.from_numpy(uneven).cuda(), iters=4)
    _check_all("uneven weights", got, ref.refine_all(poses, kp, intr, off, uneven, iters=4))
    ones = _refine(poses, kp, intr, off, np.ones(17, np.float32), iters=4)
    assert all(_same(a, b) for a, b in zip(ones, _refine(poses, kp, intr, off, iters=4)))      # null weights are all ones


def test_guards_of_the_iteration_leave_the_neighbours_alone(lib):
    from manipose_amd import place_poses
    clean_p, clean_k, bad_p, bad_k, intr = ref.guards_scene()
    clean = _refine(clean_p, clean_k, intr, iters=4)
    got = _refine(bad_p, bad_k, intr, iters=4)
    want = ref.refine_all(bad_p, bad_k, intr, iters=4)
    lin = [r.cpu().numpy() for r in place_poses(_dev(bad_p), _dev(bad_k), intr)]
    print()
    n = ref.CLAMPED                                                       # every projection clamped: H = 0, no step, the linear fit's bits
    assert got[2][n].all() and not got[3][n].any() and _same(got[0][n], lin[0][n]) and _same(got[1][n], lin[1][n]) and want[2][n].all() and not want[3][n].any()
    for n in (ref.ONE_SPOT, ref.NAN_KP):                                  # a degenerate fit: all zeros
        assert not got[2][n].any() and not got[3][n].any() and not want[2][n].any()
        assert _same(got[0][n], np.zeros((2, 3), np.float32)) and _same(got[1][n], np.zeros(2, np.float32))
    g, i = ref.BEHIND                                                     # a joint behind the camera: stored as computed, no step
    assert want[2][g, i] == 0 and got[2][g, i] == 0 and got[3][g, i] == 0 and want[2][g, 1 - i] == 1 and got[2][g, 1 - i] == 1
    assert (bad_p[g, i, :, 2] + want[0][g, i, 2]).min() < 0 and np.isfinite(want[1][g, i]) and (want[0][g, i] != 0).all()
    assert _same(got[0][g, i], lin[0][g, i]) and _same(got[1][g, i], lin[1][g, i])
    _check_all("guards scene", got, want)
    others = np.ones((8, 2), bool)
    others[[ref.CLAMPED, ref.ONE_SPOT, ref.NAN_KP]] = False
    others[g, i] = False
    for a, c in zip(got, clean):                                          # neighbours: the bits of the run without the spoiled poses
        assert _same(a[others], c[others])
    assert got[2][others].all() and (got[3][others] == 4).all()
    none = _refine(clean_p, clean_k, intr, weights=np.zeros(17, np.float32), iters=4)      # no weight at all, in a call of its own
    assert not none[2].any() and not none[3].any() and _same(none[0], np.zeros_like(none[0])) and _same(none[1], np.zeros_like(none[1]))


def test_a_step_that_raises_the_cost_is_not_taken(lib):
    """From a start 2.5 m off, undamped Gauss-Newton overshoots on some poses: the cost at t + d is several times the cost at t (the margins are in
    test_lift_refine_host.py), the step is refused, and t stays the start."""
    intr = ref.s11_intrinsics()
    poses, kp, _, off = ref.small_scene()
    start = ref.overshoot_start(place.place_all(poses, kp, intr, off)[0])
    got = _raw(lib, poses, kp, intr, off, 6, start)
    trace = []
    want = ref.refine_all(poses, kp, intr, off, iters=6, start=start, trace=trace)
    rising = sum(1 for d in trace if d["kind"] == "cost" and not d["taken"] and d["deep"])
    print(f"\n[overshoot] steps taken: {np.bincount(want[3].ravel(), minlength=7).tolist()}; {rising} steps refused for a rising cost alone")
    assert rising > 0 and (want[3] == 0).any() and (want[3] == 6).any()
    _check_all("overshooting start", got, want)
    stay = want[3] == 0
    assert _same(got[0][stay], start[stay]) and got[2][stay].all()        # refused at the first step: the start's bits, ok = 1


def test_start_mode(lib):
    from manipose_amd import reproject_poses
    intr = ref.s11_intrinsics()
    poses, kp, _, off = ref.small_scene()
    four = _refine(poses, kp, intr, off, iters=4)
    print()
    err, ok = (r.cpu().numpy() for r in reproject_poses(_dev(poses), _dev(four[0]), _dev(kp), intr, None, off))
    assert err.shape == (NTOT, 2) and err.dtype == np.float32 and ok.dtype == np.uint8 and ok.all()
    _check("reprojection at the kernel's own traj against its reproj", err, four[1].astype(np.float64))
    _check("... and against the statement", err, ref.refine_all(poses, kp, intr, off, iters=0, start=four[0])[1])
    err3, ok3 = (r.cpu().numpy() for r in reproject_poses(_dev(poses[:, 0, :, :3].copy()), _dev(four[0][:, 0].copy()), _dev(kp), intr, seq_offset=off))
    assert err3.shape == (NTOT,) and _same(err3, err[:, 0]) and _same(ok3, ok[:, 0])          # the (Ntot, J, 3) form
    start, start_ok = four[0].copy(), np.ones((NTOT, 2), np.uint8)
    start_ok[3, 1] = start_ok[100, 0] = 0
    start[7, 0, 1] = np.nan
    start[200, 1, 2] = np.inf
    for iters in (0, 3):
        got = _raw(lib, poses, kp, intr, off, iters, start, start_ok)
        want = ref.refine_all(poses, kp, intr, off, iters=iters, start=start, start_ok=start_ok)
        skipped = np.zeros((NTOT, 2), bool)
        skipped[3, 1] = skipped[100, 0] = skipped[7, 0] = skipped[200, 1] = True
        assert _same(got[0][skipped], start[skipped]) and not got[1][skipped].any() and not got[2][skipped].any() and not got[3][skipped].any()
        assert np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3]) and got[2][~skipped].all()
        assert place.within(got[0][~skipped], want[0][~skipped]).all() and place.within(got[1], want[1]).all()
    via_public = reproject_poses(_dev(poses), _dev(start), _dev(kp), intr, _dev(start_ok), off)
    plain = _raw(lib, poses, kp, intr, off, 0, start, start_ok)
    assert _same(via_public[0].cpu().numpy(), plain[1]) and _same(via_public[1].cpu().numpy(), plain[2])
    warm = _raw(lib, poses, kp, intr, off, 2, four[0])                    # a warm start from the refined traj: it stays where it is
    assert warm[2].all()
    _check("warm start, 2 steps, against the 4-step result", warm[0], four[0].astype(np.float64))
    _check("... its reproj", warm[1], four[1].astype(np.float64))
    _check_all("warm start against the statement", warm, ref.refine_all(poses, kp, intr, off, iters=2, start=four[0]))


def test_sequences_together_equal_sequences_alone(lib):
    intr = ref.s11_intrinsics()
    poses, kp, _, off = ref.small_scene()
    together = _refine(poses, kp, intr, off, iters=4)
    for s in range(3):
        sl = slice(int(off[s]), int(off[s + 1]))
        alone = _refine(poses[sl], kp[sl], intr[s], iters=4)
        assert all(_same(a, b[sl]) for a, b in zip(alone, together))
    wrong = _refine(poses, kp, intr[[1, 2, 0]], off, iters=4)             # (the cameras differ: the table is not idle)
    assert not _same(wrong[0], together[0])


def test_entry_point_rejects_bad_arguments_before_any_launch(lib):
    t = torch.zeros(4, 2, 17, 3, device="cuda")
    kp = torch.zeros(4, 17, 2, device="cuda")
    off = torch.tensor([0, 4], dtype=torch.int64, device="cuda")
    intr = _dev(ref.s11_intrinsics(1))
    traj, err = torch.full((4, 2, 3), -1.0, device="cuda"), torch.full((4, 2), -1.0, device="cuda")
    ok, steps = torch.full((4, 2), 7, dtype=torch.uint8, device="cuda"), torch.full((4, 2), 7, dtype=torch.uint8, device="cuda")
    start, start_ok = torch.zeros(4, 2, 3, device="cuda"), torch.ones(4, 2, dtype=torch.uint8, device="cuda")
    p = lambda x: None if x is None else x.data_ptr()

    def call(poses=t, keys=kp, offs=off, cam=intr, out=traj, e=err, o=ok, n=steps, st=None, so=None, Ntot=4, inner=2, J=17, ch=3, S=1, distort=1, iters=3):
        return lib.mp_lift_place_refine(p(poses), Ntot, inner, J, ch, p(keys), p(offs), S, p(cam), None, distort, p(st), p(so), iters, p(out), p(e), p(o),
                                        p(n), None)
    for kw in (dict(poses=None), dict(keys=None), dict(offs=None), dict(cam=None), dict(out=None), dict(e=None), dict(o=None)):
        assert call(**kw) == 1 and b"null" in lib.mp_last_error()
    for kw, word in ((dict(ch=2), b"C=2"), (dict(ch=5), b"C=5"), (dict(J=1), b"J=1"), (dict(J=33), b"J=33"), (dict(S=0), b"out of range"),
                     (dict(S=5), b"out of range"), (dict(Ntot=0), b"out of range"), (dict(Ntot=-3), b"out of range"), (dict(inner=0), b"out of range"),
                     (dict(Ntot=2 ** 40, inner=2 ** 10), b"too many for one launch"), (dict(distort=2), b"distort=2"), (dict(iters=17), b"iters=17"),
                     (dict(iters=-1), b"iters=-1"), (dict(so=start_ok), b"start_ok without start")):
        assert call(**kw) == 1 and word in lib.mp_last_error(), (kw, lib.mp_last_error())
    torch.cuda.synchronize()
    assert bool((traj == -1).all()) and bool((err == -1).all()) and bool((ok == 7).all()) and bool((steps == 7).all())      # nothing was launched
    assert call() == 0 and call(n=None) == 0 and call(iters=0) == 0 and call(iters=16) == 0                                  # good arguments; steps may be null
    torch.cuda.synchronize()
    assert not bool(ok.any()) and not bool(steps.any()) and bool((traj == 0).all()) and bool((err == 0).all())      # all keypoints on one spot: degenerate
    assert call(st=start, so=start_ok, iters=0) == 0 and call(st=start, iters=2) == 0
    torch.cuda.synchronize()
    assert not bool(ok.any()) and bool((traj == 0).all())                 # the pose sits at the camera's centre: not in front of it
    assert torch.count_nonzero(t).item() == 0


# ---- end to end: the tiny fp32 fixture model of lift_fixtures.py -----------------------------------------------------------------------------
def _cams(n=3):
    from manipose_amd.data.ingest import h36m_cameras
    return h36m_cameras()["S11"][:n]


def test_lift_sequences_end_to_end(lib):
    """place_refine = 3 against the statement applied to the NON-placed output of the same call (which test_gpu_lift.py pins to the oracle and which is
    bit-reproducible); one architecture: the stage does not know which model made the poses."""
    from manipose_amd import camera_table, lift_sequences, reproject_poses
    model, T, K = _model("rmcl")
    p2, cams = _sequences(T), _cams()
    intr = camera_table(cams)[0]
    kw = dict(stride=T // 2 + 1, tta=True, batch=2, return_hyps=True, cameras=cams, place=True, return_place=True)
    base = lift_sequences(model, p2, **kw)
    zero = lift_sequences(model, p2, place_refine=0, **kw)
    assert sorted(base[2][0]) == sorted(zero[2][0]) == sorted(["traj", "reproj", "ok", "hyps_traj", "hyps_reproj", "hyps_ok"])
    for a, b in zip(base[:2], zero[:2]):
        assert all(torch.equal(x, y) for x, y in zip(a, b))               # place_refine at its default: not a bit changes, no dict gains a key
    assert all(torch.equal(a[k], b[k]) for a, b in zip(base[2], zero[2]) for k in a)
    res = lift_sequences(model, p2, place_refine=3, **kw)
    assert all(torch.equal(x, y) for a, b in zip(res[:2], base[:2]) for x, y in zip(a, b))      # the poses stay where they are
    assert all(sorted(d) == sorted(["traj", "reproj", "ok", "steps", "hyps_traj", "hyps_reproj", "hyps_ok", "hyps_steps"]) for d in res[2])
    print()
    for s, d in enumerate(res[2]):
        got = {k: v.cpu().numpy() for k, v in d.items()}
        poses, hyps, k2 = _np(res[0])[s], _np(res[1])[s], p2[s]
        trace = []
        want = ref.refine_all(poses, k2, intr[s:s + 1], iters=3, trace=trace)
        hw = ref.refine_all(hyps, k2, intr[s:s + 1], iters=3, trace=trace)
        print(f"[end to end, sequence {s}] steps taken: {np.bincount(hw[3].ravel(), minlength=4).tolist()}, decision margins (cost, det ratio): {ref.margins(trace)}")
        assert got["steps"].dtype == np.uint8 and got["steps"].shape == (len(poses),) and got["hyps_steps"].shape == (len(poses), K)
        _check_all(f"sequence {s}", [got[k] for k in ("traj", "reproj", "ok", "steps")], want)
        _check_all(f"sequence {s} hypotheses", [got["hyps_" + k] for k in ("traj", "reproj", "ok", "steps")], hw)
    # with smooth_traj: the smoothed refined trajectory, and its reprojection error over the filled frames
    sm = lift_sequences(model, p2, place_refine=3, smooth_traj=3, **kw)
    plain_sm = lift_sequences(model, p2, smooth_traj=3, **kw)
    assert "reproj_smooth" not in plain_sm[2][0] and "steps" not in plain_sm[2][0]
    for s, d in enumerate(sm[2]):
        assert sorted(d) == sorted(pre + k for pre in ("", "hyps_") for k in ("traj", "reproj", "ok", "steps", "traj_fit", "filled", "reproj_smooth"))
        for pre, arr in (("", res[0][s]), ("hyps_", res[1][s])):
            assert torch.equal(d[pre + "traj_fit"], res[2][s][pre + "traj"]) and torch.equal(d[pre + "reproj"], res[2][s][pre + "reproj"])
            err, ok = reproject_poses(arr, d[pre + "traj"].contiguous(), _dev(p2[s]), intr[s], d[pre + "filled"])
            assert d[pre + "reproj_smooth"].shape == d[pre + "filled"].shape and torch.equal(d[pre + "reproj_smooth"], err)
            want = ref.refine_all(arr.cpu().numpy(), p2[s], intr[s:s + 1], iters=0, start=d[pre + "traj"].cpu().numpy(),
                                  start_ok=d[pre + "filled"].cpu().numpy())
            assert place.within(err.cpu().numpy(), want[1]).all() and not bool(err[d[pre + "filled"] == 0].any())       # nothing filled in: 0


def test_place_refine_lift_entry_point(lib, tmp_path, monkeypatch):
    sys.path.insert(0, os.path.join(ROOT, "hpe"))
    from _entry import run
    monkeypatch.chdir(tmp_path)
    common = ["run.train=false", "run.test=false", "run.lift=true", "lift.stride=14", "train.batch_size_test=4", "data.seq_len=27", "model.channels=64",
              "model.layers=2", "model.nheads=4", "model.channels_seg=32", "model.layers_seg=1", "model.nheads_seg=4", "multi_hyp.n_hyp=3",
              "data.synthetic_sequences=2", "model.precision=fp32", "lift.hyps=true", "lift.place=true"]
    keys = [f"synthetic_{i:03d}" for i in range(2)]
    placed = ["", "__hyps", "__traj", "__reproj", "__ok", "__hyps_traj", "__hyps_reproj", "__hyps_ok", "__cam"]
    run(common)                                                           # the key at its default: exactly today's keys
    z0 = np.load(os.path.join(str(tmp_path), "default", "lift.npz"))
    assert sorted(z0.files) == sorted(k + s for k in keys for s in placed)
    z0 = {k: z0[k] for k in z0.files}
    run(common + ["lift.place_refine=3", "lift.smooth_traj=4"])
    z = np.load(os.path.join(str(tmp_path), "default", "lift.npz"))
    more = ["__steps", "__hyps_steps", "__traj_fit", "__filled", "__hyps_traj_fit", "__hyps_filled", "__reproj_smooth", "__hyps_reproj_smooth"]
    assert sorted(z.files) == sorted(k + s for k in keys for s in placed + more)
    for i, k in enumerate(keys):
        n = 27 * 4 + 37 * i + 11
        assert z[k + "__steps"].shape == (n,) and z[k + "__steps"].dtype == np.uint8 and z[k + "__hyps_steps"].shape == (n, 3)
        assert z[k + "__reproj_smooth"].shape == (n,) and z[k + "__hyps_reproj_smooth"].shape == (n, 3) and z[k + "__reproj_smooth"].dtype == np.float32
        assert _same(z[k], z0[k]) and z[k + "__steps"].max() <= 3

"""Placing lifted sequences in the scene on the device: mp_lift_place and mp_lift_world against float64 (lift_place_ref.py) and against the
reference's own outputs (tests/golden/place.npz), the degenerate rule, weights, the floor, determinism, argument errors,
lift_sequences(place= / frame= / floor=) for the three architectures against the statement applied to its own non-placed output, and run.lift.

The bound, everywhere a float32 is compared with float64: |x - x64| <= 2^-23 max(1, |x64|).  The kernels compute in fp64 between their float32
loads and stores, so against the float64 statement ON THE SAME float32 INPUTS only the final rounding (2^-24 relative) remains; the fit's
condition number is below 10^3, which leaves 10^-13 of fp64 noise.  The bound is not measured from the kernels."""
import os
import sys

import numpy as np
import pytest
import torch

import lift_place_ref as ref
from lift_fixtures import fixture_model as _model, same as _same, sequences_2d as _sequences, to_numpy as _np

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENS = [1, 70, 259]                                    # a sequence boundary inside a 256-lane workgroup, and poses that cross one
OFF = np.concatenate([[0], np.cumsum(LENS)]).astype(np.int64)
NTOT = int(OFF[-1])


def _cams(n=3):
    from manipose_amd.data.ingest import h36m_cameras
    return h36m_cameras()["S11"][:n]


def _intr(n=3):
    return np.stack([c["intrinsic"] for c in _cams(n)]).astype(np.float32)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _place(poses, kp, intr, off=None, weights=None, distort=True):
    from manipose_amd import place_poses
    res = place_poses(_dev(poses), _dev(kp), intr, off, weights, distort)
    torch.cuda.synchronize()
    return [r.cpu().numpy() for r in res]


def _check(tag, got, want):
    print(f"[{tag}] worst error = {ref.worst(got, want):.3f} x the bound 2^-23 max(1, |x|)")
    assert ref.within(got, want).all()


@pytest.mark.parametrize("inner,ch", [(1, 3), (1, 4), (5, 3), (5, 4)])
def test_fit_against_fp64(lib, inner, ch):
    intr = _intr()
    poses, kp, t_true, off = ref.synthetic_scene(LENS, inner, ch, intr, seed=100 + 10 * inner + ch)
    public3 = (inner, ch) == (1, 3)                                       # the (Ntot, J, 3) form of the public function
    given = poses[:, 0] if public3 else poses
    print()
    for distort in (True, False):
        want = ref.place_all(given, kp, intr, off, distort=distort)
        depth = (poses[..., 2].astype(np.float64) + np.asarray(want[0]).reshape(NTOT, inner, 3)[..., 2:3]).min()
        print(f"[place inner={inner} C={ch} distort={int(distort)}] minimum depth {depth:.2f} m, mean reprojection error {want[1].mean():.4f}")
        assert want[2].all() and depth > 0                                # the construction is ok = 1 everywhere
        t = _dev(given)
        from manipose_amd import place_poses
        traj, err, ok = (r.cpu().numpy() for r in place_poses(t, _dev(kp), intr, off, None, distort))
        assert traj.shape == want[0].shape and traj.dtype == np.float32 and err.shape == want[1].shape and err.dtype == np.float32
        assert ok.shape == want[2].shape and ok.dtype == np.uint8 and np.array_equal(ok, want[2])
        _check("traj", traj, want[0])
        _check("reproj", err, want[1])
        assert _same(t.cpu().numpy(), given)                              # poses are read only (the score channel included)
        again = _place(given, kp, intr, torch.from_numpy(off).cuda(), None, distort)      # a device offset table; and: two calls, identical bits
        assert _same(again[0], traj) and _same(again[1], err) and _same(again[2], ok)
    assert np.abs(traj.reshape(NTOT, inner, 3)[:, 0] - t_true).max() < 0.5      # (the noisy keypoints still find the true translation roughly)


def test_exact_recovery_without_noise(lib):
    intr = _intr()
    poses, kp, t_true, off = ref.synthetic_scene(LENS, 1, 3, intr, seed=7, noise=0.0)
    traj, err, ok = _place(poses[:, 0], kp, intr, off, distort=False)
    miss = np.abs(traj.astype(np.float64) - t_true).max()
    print(f"\n[recovery] max |traj - t_true| = {miss:.2e} m (bound 2e-6), max reproj = {err.max():.2e} (bound 1e-6)")
    assert ok.all() and miss <= 2e-6 and err.max() <= 1e-6


def test_weights(lib):
    intr = _intr()
    poses, kp, _, off = ref.synthetic_scene(LENS, 5, 4, intr, seed=8)
    keep = np.arange(17) % 3 != 0
    zero_some = np.where(keep, 1.0, 0.0).astype(np.float32)
    got = _place(poses, kp, intr, off, zero_some)
    want = ref.place_all(poses[:, :, keep], kp[:, keep], intr, off)       # the statement on the remaining joints alone
    print()
    _check("zero weights: traj", got[0], want[0])
    _check("zero weights: reproj", got[1], want[1])
    assert np.array_equal(got[2], want[2])
    poisoned = kp.copy()
    poisoned[:, ~keep] = np.nan                                           # a joint of weight 0 is not looked at
    assert all(_same(a, b) for a, b in zip(_place(poses, poisoned, intr, off, zero_some), got))
    uneven = np.random.default_rng(9).uniform(0.25, 4.0, 17).astype(np.float32)
    got = _place(poses, kp, intr, off, torch.from_numpy(uneven).cuda())
    want = ref.place_all(poses, kp, intr, off, uneven)
    _check("uneven weights: traj", got[0], want[0])
    _check("uneven weights: reproj", got[1], want[1])
    assert np.array_equal(got[2], want[2]) and want[2].all()
    ones = _place(poses, kp, intr, off, np.ones(17, np.float32))
    assert all(_same(a, b) for a, b in zip(ones, _place(poses, kp, intr, off)))      # null weights are all ones
    from manipose_amd import place_poses
    with pytest.raises(ValueError, match="non-negative"):
        place_poses(_dev(poses), _dev(kp), intr, off, -uneven)


def test_degenerate_poses_follow_the_rule_and_leave_their_neighbours_alone(lib):
    intr = _intr(1)
    poses, kp, _, _ = ref.synthetic_scene([8], 2, 3, intr, seed=11)
    clean = _place(poses, kp, intr)
    bad_p, bad_k = poses.copy(), kp.copy()
    bad_k[2] = bad_k[2, 5]                                                # all keypoints of frame 2 on one spot
    bad_k[4, 9, 1] = np.nan                                               # a NaN keypoint in frame 4
    bad_p[6, 1, 5, 2] = -40.0                                             # frame 6, second pose: a joint far behind the fitted distance
    got = _place(bad_p, bad_k, intr)
    want = ref.place_all(bad_p, bad_k, intr)
    for n in (2, 4):
        assert not got[2][n].any() and not want[2][n].any()
        assert _same(got[0][n], np.zeros((2, 3), np.float32)) and _same(got[1][n], np.zeros(2, np.float32))
    assert want[2][6, 1] == 0 and got[2][6, 1] == 0 and want[2][6, 0] == 1 and got[2][6, 0] == 1      # the statement finds the joint behind the camera
    assert (bad_p[6, 1, :, 2] + want[0][6, 1, 2]).min() < 0 and np.isfinite(want[1][6, 1]) and (want[0][6, 1] != 0).all()
    assert ref.within(got[0][6, 1], want[0][6, 1]).all() and ref.within(got[1][6, 1], want[1][6, 1])      # stored as computed
    others = np.ones((8, 2), bool)
    others[2] = others[4] = False
    others[6, 1] = False
    for g, c in zip(got, clean):                                          # neighbours: the bits of the run without the degenerate poses
        assert _same(g[others], c[others])
    assert got[2][others].all()
    none = _place(poses, kp, intr, weights=np.zeros(17, np.float32))      # no weight at all, in a call of its own
    assert not none[2].any() and _same(none[0], np.zeros_like(none[0])) and _same(none[1], np.zeros_like(none[1]))


def _world_inputs(inner, ch, seed):
    g = np.random.default_rng(seed)
    poses = g.standard_normal((NTOT, inner, 17, ch)).astype(np.float32)
    traj = g.uniform(-3, 3, (NTOT, inner, 3)).astype(np.float32)
    quat = np.stack([c["orientation"] for c in _cams()]).astype(np.float32)
    quat[2] *= np.float32(1.25)                                           # qrot does not normalise
    trans = np.stack([c["translation"] for c in _cams()]).astype(np.float32)
    return poses, traj, quat, trans


@pytest.mark.parametrize("inner,ch", [(1, 3), (5, 4)])
def test_world_against_fp64(lib, inner, ch):
    from manipose_amd import to_world
    poses, traj, quat, trans = _world_inputs(inner, ch, seed=20 + ch)
    same = to_world(_dev(poses), np.broadcast_to(np.array([1, 0, 0, 0], np.float32), (3, 4)), seq_offset=OFF)
    assert _same(same.cpu().numpy(), poses)                               # identity, no trajectory, no translation: not a bit changes
    public3 = (inner, ch) == (1, 3)
    t = _dev(poses[:, 0] if public3 else poses)
    r = to_world(t, quat, trans, _dev(traj[:, 0] if public3 else traj), OFF)
    assert r is t                                                         # in place
    got = r.cpu().numpy().reshape(poses.shape)
    want = ref.world_all(poses, quat, trans, traj, OFF)
    print()
    _check(f"world inner={inner} C={ch}", got[..., :3], want[..., :3])
    if ch == 4:
        assert _same(got[..., 3], poses[..., 3])                          # the score channel, bit for bit
    rot = to_world(_dev(poses), quat, seq_offset=OFF).cpu().numpy()       # camera_to_world(., R, t = 0)
    _check("rotation only", rot[..., :3], ref.world_all(poses, quat, seq_offset=OFF)[..., :3])
    again = to_world(_dev(poses), quat, trans, _dev(traj), torch.from_numpy(OFF).cuda()).cpu().numpy()
    assert _same(again, got)                                              # two calls: identical bits


@pytest.mark.parametrize("where", ["first", "last"])
def test_floor(lib, where):
    from manipose_amd import to_world
    from manipose_amd.lifting import FLOOR_SHARES
    inner = 5
    poses, traj, quat, trans = _world_inputs(inner, 4, seed=31)
    quat[2] = (1, 0, 0, 0)                                                # sequence 2 keeps its axes, so its lowest point is where it is put:
    traj[OFF[2]:, :, 2] = 0                                               # once in the first, once in the last workgroup's share of the sequence
    trans[2, 2] = 0.5
    n2 = LENS[2] * inner
    share = -(-n2 // FLOOR_SHARES)
    assert n2 > 2 * share                                                 # first and last share are different workgroups
    if where == "first":
        poses[OFF[2], 0, 3, 2] = -9.0
    else:
        poses[OFF[3] - 1, inner - 1, 16, 2] = -9.0
    plain = to_world(_dev(poses), quat, trans, _dev(traj), OFF).cpu().numpy()
    t = _dev(poses)
    r, offsets = to_world(t, quat, trans, _dev(traj), OFF, floor=True)
    assert r is t and tuple(offsets.shape) == (3,) and offsets.dtype == torch.float32
    got, offsets = r.cpu().numpy(), offsets.cpu().numpy()
    want_off = ref.floor_of(plain, OFF)
    assert _same(offsets, want_off) and offsets[2] == np.float32(-8.5)    # the float32 minimum of the floor-off output
    assert _same(got, ref.apply_floor(plain, want_off, OFF))              # z = floor-off z - minimum, one float32 subtraction; x, y, scores untouched
    for s in range(3):
        assert got[OFF[s]:OFF[s + 1], ..., 2].min() == 0.0
    given = to_world(_dev(poses), quat, trans, _dev(traj), OFF, floor=offsets).cpu().numpy()
    assert _same(given, got)                                              # mode 2 with those offsets reproduces mode 1
    given_t = to_world(_dev(poses), quat, trans, _dev(traj), OFF, floor=torch.from_numpy(offsets).cuda()).cpu().numpy()
    r2, off2 = to_world(_dev(poses), quat, trans, _dev(traj), OFF, floor=True)
    assert _same(given_t, got) and _same(r2.cpu().numpy(), got) and _same(off2.cpu().numpy(), offsets)      # two calls: identical bits


def test_the_references_own_outputs(lib, golden_dir):
    from manipose_amd import place_poses, to_world
    z = np.load(os.path.join(golden_dir, "place.npz"))
    X, kp, intr, quat = z["X"].astype(np.float32), z["kp"].astype(np.float32), z["intr"], z["quat"]
    assert np.array_equal(X.astype(np.float64), z["X"]) and np.array_equal(kp.astype(np.float64), z["kp"])       # the file's inputs are float32 values
    off = np.arange(7)
    print()
    for distort, key in ((True, "proj_fit"), (False, "proj_linear_fit")):
        traj, err, ok = (r.cpu().numpy() for r in place_poses(_dev(X), _dev(kp), intr, off, None, distort))
        want_err = np.sqrt(((z[key] - z["kp"][:, None]) ** 2).sum(-1)).mean(-1)       # the reference's projection of the placed points
        _check(f"golden traj distort={int(distort)}", traj, z["t_fit"])
        _check(f"golden reproj distort={int(distort)}", err, want_err)
        assert ok.all()
    assert want_err[4:].min() > 0.1 > want_err[:4].max()                  # frames 4 and 5 sit in the clamp
    world = to_world(_dev(X), quat, seq_offset=off).cpu().numpy()
    _check("golden camera_to_world", world, z["world"])
    floored, offsets = to_world(_dev(X), quat, seq_offset=off, floor=True)
    _check("golden floor offsets", offsets.cpu().numpy(), z["world"][..., 2].min(axis=(1, 2)))
    # float32 z minus float32 minimum, rounded to float32, against the reference's float64 difference: 2^-24 (|z| + |min| + |z - min|) <= 4 2^-24 max |z|
    zmax = np.abs(z["world"][..., 2]).max()
    assert np.abs(floored.cpu().numpy()[..., 2] - z["world_floor"][..., 2]).max() <= 4 * 2.0 ** -24 * zmax
    assert all(floored[n, ..., 2].min().item() == 0.0 for n in range(6))


def test_entry_points_reject_bad_arguments_before_any_launch(lib):
    t = torch.zeros(4, 2, 17, 3, device="cuda")
    kp = torch.zeros(4, 17, 2, device="cuda")
    off = torch.tensor([0, 4], dtype=torch.int64, device="cuda")
    intr = _dev(_intr(1))
    quat = torch.tensor([[0.0, 1.0, 0.0, 0.0]], device="cuda")
    traj, err = torch.full((4, 2, 3), -1.0, device="cuda"), torch.full((4, 2), -1.0, device="cuda")
    ok = torch.full((4, 2), 7, dtype=torch.uint8, device="cuda")
    fl, scratch = torch.full((1,), -1.0, device="cuda"), torch.zeros(16, device="cuda")
    p = lambda x: None if x is None else x.data_ptr()

    def place(poses=t, keys=kp, offs=off, cam=intr, out=traj, e=err, o=ok, Ntot=4, inner=2, J=17, ch=3, S=1, distort=1):
        return lib.mp_lift_place(p(poses), Ntot, inner, J, ch, p(keys), p(offs), S, p(cam), None, distort, p(out), p(e), p(o), None)

    def world(poses=t, offs=off, q=quat, Ntot=4, inner=2, J=17, ch=3, S=1, mode=0, floor=None, scr=None, n=0):
        return lib.mp_lift_world(p(poses), Ntot, inner, J, ch, None, p(offs), S, p(q), None, mode, p(floor), p(scr), n, None)
    for kw in (dict(poses=None), dict(keys=None), dict(offs=None), dict(cam=None), dict(out=None), dict(e=None), dict(o=None)):
        assert place(**kw) == 1 and b"null" in lib.mp_last_error()
    for kw in (dict(poses=None), dict(offs=None), dict(q=None), dict(mode=1, scr=scratch, n=16), dict(mode=2)):
        assert world(**kw) == 1 and b"null" in lib.mp_last_error(), lib.mp_last_error()
    for fn in (place, world):
        for kw, word in ((dict(ch=2), b"C=2"), (dict(ch=5), b"C=5"), (dict(J=1), b"J=1"), (dict(J=33), b"J=33"), (dict(S=0), b"out of range"),
                         (dict(S=5), b"out of range"), (dict(Ntot=0), b"out of range"), (dict(Ntot=-3), b"out of range"), (dict(inner=0), b"out of range"),
                         (dict(Ntot=2 ** 40, inner=2 ** 10), b"too many for one launch")):
            assert fn(**kw) == 1 and word in lib.mp_last_error(), (kw, lib.mp_last_error())
    assert place(distort=2) == 1 and b"distort=2" in lib.mp_last_error()
    assert world(mode=3) == 1 and b"floor_mode=3" in lib.mp_last_error()
    assert world(mode=1, floor=fl, scr=scratch, n=15) == 1 and b"scratch" in lib.mp_last_error()
    assert world(mode=1, floor=fl, scr=None, n=16) == 1 and b"scratch" in lib.mp_last_error()
    torch.cuda.synchronize()
    assert bool((traj == -1).all()) and bool((err == -1).all()) and bool((ok == 7).all()) and bool((fl == -1).all())      # nothing was launched
    assert torch.count_nonzero(t).item() == 0
    assert place() == 0 and world(mode=1, floor=fl, scr=scratch, n=16) == 0       # the same calls with good arguments
    torch.cuda.synchronize()
    assert not bool(ok.any()) and bool((traj == 0).all()) and bool((err == 0).all())      # all keypoints on one spot: degenerate
    assert fl.item() == 0.0 and torch.count_nonzero(t).item() == 0


# ---- end to end: the tiny fp32 fixture models of lift_fixtures.py ------------------------------------------------------------------------------
def _check_placed(tag, info, base, p2, cams, hyps=None):
    """the per-sequence dicts of return_place against the statement applied to the non-placed output `base` (and `hyps`)"""
    from manipose_amd import camera_table
    intr = camera_table(cams)[0]
    for s, (d, b, k) in enumerate(zip(info, base, p2)):
        want = ref.place_all(b, k, intr[s:s + 1])
        got = {key: v.cpu().numpy() for key, v in d.items()}
        assert got["traj"].shape == (len(b), 3) and got["reproj"].shape == (len(b),) and got["ok"].shape == (len(b),) and got["ok"].dtype == np.uint8
        assert ref.within(got["traj"], want[0]).all() and ref.within(got["reproj"], want[1]).all() and np.array_equal(got["ok"], want[2]), tag
        if hyps is not None:
            hw = ref.place_all(hyps[s], k, intr[s:s + 1])
            K = hyps[s].shape[1]
            assert got["hyps_traj"].shape == (len(b), K, 3) and got["hyps_reproj"].shape == (len(b), K) and got["hyps_ok"].dtype == np.uint8
            assert ref.within(got["hyps_traj"], hw[0]).all() and ref.within(got["hyps_reproj"], hw[1]).all() and np.array_equal(got["hyps_ok"], hw[2]), tag
        else:
            assert not any(key.startswith("hyps_") for key in got)


@pytest.mark.parametrize("kind", ["rmcl", "manifold", "mixste"])
def test_lift_sequences_end_to_end(lib, kind):
    """Every placed output is the float64 statement applied to the NON-placed output of the same call (which test_gpu_lift.py pins to the oracle
    and which is bit-reproducible) and to the float32 trajectories the call returned."""
    from manipose_amd import camera_table, lift_sequences
    model, T, K = _model(kind)
    p2 = _sequences(T)
    cams = _cams()
    intr, quat, trans = camera_table(cams)
    hyp = kind == "rmcl"
    for extra in (dict(), dict(scale=1000.0), dict(rigid=True, lengths="measured")):
        kw = dict(stride=T // 2 + 1, tta=True, batch=2, return_hyps=hyp, **extra)
        scale = np.float32(extra.get("scale", 1.0))
        res = lift_sequences(model, p2, **kw)
        base, base_h = (_np(res[0]), _np(res[1])) if hyp else (_np(res), None)
        off_res = lift_sequences(model, p2, place=False, frame="camera", floor=False, cameras=None, **kw)
        for a, b in zip(res if hyp else (res,), off_res if hyp else (off_res,)):
            assert all(torch.equal(x, y) for x, y in zip(a, b))           # the new arguments at their defaults: not a bit changes
        # place alone: the poses stay where they are, the fit is returned
        res = lift_sequences(model, p2, cameras=cams, place=True, return_place=True, **kw)
        assert isinstance(res, tuple) and len(res) == (3 if hyp else 2)
        assert all(_same(a, b) for a, b in zip(_np(res[0]), base))
        _check_placed(f"{kind} {extra} place", res[-1], base, p2, cams, base_h)
        # rotation alone: the reference's prepare_prediction_for_viz before its floor line
        res = lift_sequences(model, p2, cameras=cams, frame="world", **kw)
        rot, rot_h = (_np(res[0]), _np(res[1])) if hyp else (_np(res), None)
        for s in range(3):
            assert ref.within(rot[s], ref.world_all(base[s], quat[s])).all()
            if hyp:
                assert ref.within(rot_h[s][..., :3], ref.world_all(base_h[s], quat[s])[..., :3]).all() and _same(rot_h[s][..., 3], base_h[s][..., 3])
        # everything: place, world frame, floor
        full = lift_sequences(model, p2, cameras=cams, place=True, frame="world", floor=True, return_place=True, **kw)
        nofl = lift_sequences(model, p2, cameras=cams, place=True, frame="world", return_place=True, **kw)
        assert len(full) == (3 if hyp else 2) and sorted(full[-1][0]) == sorted(["traj", "reproj", "ok", "floor"] + (["hyps_traj", "hyps_reproj", "hyps_ok"] if hyp else []))
        _check_placed(f"{kind} {extra} full", full[-1], base, p2, cams, base_h)
        for s in range(3):
            d = {k: v.cpu().numpy() for k, v in full[-1][s].items()}
            t_s = trans[s] * scale                                        # float32: the translation in the poses' unit
            stored = nofl[0][s].cpu().numpy()
            assert ref.within(stored, ref.world_all(base[s], quat[s], t_s, d["traj"])).all()
            fl = ref.floor_of(stored)
            assert d["floor"].shape == () and _same(d["floor"].reshape(1), fl)
            got = full[0][s].cpu().numpy()
            assert _same(got, ref.apply_floor(stored, fl)) and got[..., 2].min() == 0.0
            if hyp:                                                       # the hypotheses stand on the merged poses' floor
                stored_h = nofl[1][s].cpu().numpy()
                want_h = ref.world_all(base_h[s], quat[s], t_s, d["hyps_traj"])
                assert ref.within(stored_h[..., :3], want_h[..., :3]).all() and _same(stored_h[..., 3], base_h[s][..., 3])
                assert _same(full[1][s].cpu().numpy(), ref.apply_floor(stored_h, fl))
    if kind == "rmcl":                                                    # the order poses, hyps, bones, place; floor without place
        res = lift_sequences(model, p2, stride=T, return_hyps=True, rigid=True, return_bones=True, cameras=cams, place=True, return_place=True)
        assert len(res) == 4 and res[1][0].shape[1:] == (K, 17, 4) and res[2][0].shape == (16,) and isinstance(res[3][0], dict)
        res = lift_sequences(model, p2, stride=T, cameras=cams, frame="world", floor=True, return_place=True)
        assert len(res) == 2 and all(sorted(d) == ["floor"] for d in res[1]) and all(r[..., 2].min().item() == 0.0 for r in res[0])


def test_place_lift_entry_point(lib, tmp_path, monkeypatch):
    sys.path.insert(0, os.path.join(ROOT, "hpe"))
    from _entry import run
    from manipose_amd import camera_table
    monkeypatch.chdir(tmp_path)
    common = ["run.train=false", "run.test=false", "run.lift=true", "lift.stride=14", "train.batch_size_test=4", "data.seq_len=27", "model.channels=64",
              "model.layers=2", "model.nheads=4", "model.channels_seg=32", "model.layers_seg=1", "model.nheads_seg=4", "multi_hyp.n_hyp=3",
              "data.synthetic_sequences=5", "model.precision=fp32", "lift.hyps=true"]
    run(common + ["lift.place=true", "lift.frame=world", "lift.floor=true"])
    z = np.load(os.path.join(str(tmp_path), "default", "lift.npz"))
    keys = [f"synthetic_{i:03d}" for i in range(5)]
    suffixes = ["", "__hyps", "__traj", "__reproj", "__ok", "__hyps_traj", "__hyps_reproj", "__hyps_ok", "__floor", "__cam"]
    assert sorted(z.files) == sorted(k + s for k in keys for s in suffixes)
    rows = np.concatenate(camera_table(_cams(4)), axis=1)
    for i, k in enumerate(keys):
        n = 27 * 4 + 37 * i + 11
        assert z[k].shape == (n, 17, 3) and z[k + "__hyps"].shape == (n, 3, 17, 4)
        assert z[k + "__traj"].shape == (n, 3) and z[k + "__reproj"].shape == (n,) and z[k + "__ok"].shape == (n,) and z[k + "__ok"].dtype == np.uint8
        assert z[k + "__hyps_traj"].shape == (n, 3, 3) and z[k + "__hyps_reproj"].shape == (n, 3) and z[k + "__hyps_ok"].shape == (n, 3)
        assert z[k + "__hyps_ok"].dtype == np.uint8 and z[k + "__floor"].shape == () and z[k + "__cam"].shape == (16,)
        assert _same(z[k + "__cam"], rows[i % 4])                         # sequence i: S11's camera i % 4
        assert np.isfinite(z[k]).all() and z[k][..., 2].min() == 0.0      # the merged poses stand on the floor
    run(common)                                                           # the three keys at their defaults: exactly today's keys
    z = np.load(os.path.join(str(tmp_path), "default", "lift.npz"))
    assert sorted(z.files) == sorted(keys + [k + "__hyps" for k in keys])

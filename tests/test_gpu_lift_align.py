"""Aligning a take's views without extrinsics on the device: mp_lift_align_views against the float64 statement of its rule (lift_align_ref.py), the
constructed degenerate takes compared exactly, the invariants (identical bits, a take alone and beside others, inputs untouched), argument errors,
the recovery scene the feature is for, and run.lift with lift.fuse_cameras=estimate end to end.

The bounds against the statement, ON THE SAME float32 INPUTS: used and ok are equal; quat within 2^-23 per component (both canonical); trans, rms
and trans_rms within one float32 ulp of the largest magnitude of the compared array.  The kernel and the statement both work in fp64 and differ in
the order of their sums and in the eigen-solver (Jacobi against LAPACK): relative 1e-15 or so, amplified by the inverse of the relative
eigenvalue gap; what remains is the one rounding to float32.  That holds where the gap is >= 0.1, which every compared row is asserted to be
(test_lift_align_host.py asserts it without a device as well); the bounds are not measured from the kernel.  Measured on an MI355X: quat at most
0.25 x 2^-23, the others at most 0.49 ulp - the one rounding and nothing else."""
import os
import sys

import numpy as np
import pytest
import torch

import lift_align_ref as ref
from lift_fixtures import fixture_model as _model, same as _same

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hpe"))
KEYS = ("quat", "trans", "rms", "trans_rms", "used", "ok")


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _align(poses, valid=None, off=None, traj=None, traj_ok=None, sigma=0.05, iters=5, reference=None):
    from manipose_amd import align_views
    res = align_views(_dev(poses), _dev(valid), off, _dev(traj), _dev(traj_ok), sigma, iters, reference)
    torch.cuda.synchronize()
    return {k: None if r is None else r.cpu().numpy() for k, r in zip(KEYS, res)}


def _compare(tag, got, want, traj):
    assert got["used"].dtype == np.int32 and got["ok"].dtype == np.uint8
    assert np.array_equal(got["used"], want["used"]) and np.array_equal(got["ok"], want["ok"]), (tag, got["ok"], want["ok"], got["used"], want["used"])
    rot = (want["ok"] & 1).astype(bool) & (want["rms"] > 0)
    assert (want["gap"][rot] >= ref.GAP_MIN).all(), tag                   # the bounds are claimed for these rows only
    dq = np.abs(got["quat"].astype(np.float64) - want["quat"]).max()
    print(f"[{tag}] quat off by {dq / ref.QUAT_TOL:.3f} x 2^-23", end="")
    assert ref.close_quat(got["quat"], want["quat"]).all(), tag
    assert (got["quat"][..., 0] >= 0).all()
    for k in ("rms",) + (("trans", "trans_rms") if traj else ()):
        bound = ref.ulp_bound(want[k])
        d = np.abs(got[k].astype(np.float64) - want[k]).max()
        print(f", {k} by {d / bound if bound else 0:.3f} ulp of {np.abs(want[k]).max():.3g}", end="")
        assert d <= bound, (tag, k)
    print()
    if not traj:
        assert got["trans"] is None and got["trans_rms"] is None and not (got["ok"] & 2).any()
    fill = want["ok"] == 0                                                # a degenerate row is the identity, exactly
    assert (got["quat"][fill] == [1, 0, 0, 0]).all() and not got["rms"][fill].any()
    if traj:
        assert not got["trans"][(want["ok"] & 2) == 0].any() and not got["trans_rms"][(want["ok"] & 2) == 0].any()


@pytest.mark.parametrize("n", range(len(ref.cases())))
def test_align_matches_the_statement(n):
    tag, inp, want = ref.cases()[n]
    got = _align(inp["poses"], inp.get("valid"), inp["off"], inp.get("traj"), inp.get("traj_ok"), inp.get("sigma", 0.05), inp.get("iters", 5))
    _compare(tag, got, want, "traj" in inp)


def test_constructed_degenerate_takes():
    fill = lambda r, g, v: (np.array_equal(r["quat"][g, v], [1, 0, 0, 0]) and not r["trans"][g, v].any() and r["rms"][g, v] == 0
                            and r["trans_rms"][g, v] == 0 and r["ok"][g, v] == 0)
    line = np.zeros((2, 6, 4, 3), np.float32)
    line[0, :, 1:, 0], line[1, :, 1:, 1] = [1, 2, 3], [1, 2, 3]           # identical frames, collinear joints: the rotation about the line is free
    zt, ones = np.zeros((2, 6, 3), np.float32), np.ones((2, 6), np.uint8)
    r = _align(line, None, None, zt, ones)
    assert fill(r, 0, 1) and r["used"][0].tolist() == [6, 6] and r["ok"][0, 0] == 1 and np.array_equal(r["quat"][0, 0], [1, 0, 0, 0])
    sc = ref.scene(3, 5, [12], seed=5)
    args = (sc["off"], sc["traj"], sc["traj_ok"])
    valid = np.ones((3, 12), np.uint8)
    valid[0], valid[1, :6], valid[2, 6:] = 0, 0, 0                        # view 0 missing: view 1 is the reference; views 1 and 2 share no valid frame
    r = _align(sc["poses"], valid, *args)
    assert fill(r, 0, 0) and fill(r, 0, 2) and r["used"][0].tolist() == [0, 6, 0] and r["ok"][0].tolist() == [0, 1, 0]
    r = _align(sc["poses"], np.zeros((3, 12), np.uint8), *args)           # no view at all
    assert all(fill(r, 0, v) for v in range(3)) and not r["used"].any()
    tok = sc["traj_ok"].copy()
    tok[2] = 0                                                            # traj_ok nowhere set in view 2
    r = _align(sc["poses"], None, sc["off"], sc["traj"], tok)
    want = ref.align(sc["poses"], None, sc["off"], sc["traj"], tok)
    assert r["ok"][0].tolist() == [1, 3, 1] and not r["trans"][0, 2].any() and r["trans_rms"][0, 2] == 0 and r["rms"][0, 2] > 0
    _compare("traj_ok nowhere set in view 2", r, want, True)
    flat = sc["poses"].copy()
    flat[1] = flat[1][:, :1]                                              # every joint at the root: M = 0
    r = _align(flat, None, *args)
    assert fill(r, 0, 1) and r["used"][0, 1] == 12 and r["ok"][0, 2] == 3
    huge = np.zeros((2, 2, 3, 3), np.float32)                             # every weight 0: (1 + e / sigma^2)^2 overflows
    huge[0, 0, 1:], huge[0, 1, 1:] = [[3e38, 0, 0], [0, 3e38, 0]], [[0, 3e38, 0], [3e38, 0, 0]]
    huge[1, 0, 1:], huge[1, 1, 1:] = [[3e38, 0, 0], [0, 3e38, 0]], [[3e38, 0, 0], [0, -3e38, 0]]
    r = _align(huge, None, None, np.zeros((2, 2, 3), np.float32), np.ones((2, 2), np.uint8), sigma=1e-40, iters=1)
    assert fill(r, 0, 1) and r["used"][0, 1] == 2
    body = np.array([[0, 0, 0], [1, 0, 0], [0, 2, 0], [0, 0, 3], [-2, 0, 0]], np.float32)       # half a turn about y: w = 0 exactly, y positive
    turn = np.stack([np.tile(body, (3, 1, 1)), np.tile(body * np.array([-1, 1, -1], np.float32), (3, 1, 1))])
    r = _align(turn, iters=2)
    assert np.array_equal(r["quat"][0, 1], [0, 0, 1, 0]) and not np.signbit(r["quat"][0, 1]).any() and r["ok"][0, 1] == 1 and r["rms"][0, 1] == 0


def test_invariants():
    from manipose_amd import align_views
    sc = ref.scene(4, 17, [1, 257, 40], seed=111, mirrored=0.3)
    valid = ref.valid_table(4, sc["off"], 112, missing=((1, 0), (2, 2)))
    spoiled = sc["poses"].copy()
    spoiled[valid == 0] = np.nan                                          # an invalid view's frame is never summed
    d = [_dev(a) for a in (spoiled, valid, sc["traj"], sc["traj_ok"])]
    a = align_views(d[0], d[1], sc["off"], d[2], d[3])
    b = align_views(d[0], d[1], sc["off"], d[2], d[3])
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(a, b))                   # identical bits
    assert np.array_equal(d[0].cpu().numpy(), spoiled, equal_nan=True) and _same(d[1].cpu().numpy(), valid) and _same(d[2].cpu().numpy(), sc["traj"])
    clean = _align(sc["poses"], valid, sc["off"], sc["traj"], sc["traj_ok"])
    assert all(_same(clean[k], x.cpu().numpy()) for k, x in zip(KEYS, a))
    for t in range(3):                                                    # a take alone: the bits it has beside the others
        sl = slice(int(sc["off"][t]), int(sc["off"][t + 1]))
        alone = _align(sc["poses"][:, sl], valid[:, sl], None, sc["traj"][:, sl], sc["traj_ok"][:, sl])
        assert all(_same(alone[k][0], clean[k][t]) for k in KEYS)
    blind = _align(sc["poses"], valid, sc["off"], sc["traj"], sc["traj_ok"], sigma=float("inf"), iters=8)
    plain = _align(sc["poses"], valid, sc["off"], sc["traj"], sc["traj_ok"], iters=0)
    assert all(_same(blind[k], plain[k]) for k in KEYS)                   # sigma = inf: every weight is exactly 1


def test_entry_point_rejects_bad_arguments_before_any_launch(lib):
    V, F, J, G = 3, 6, 17, 1
    poses, traj = torch.zeros(V, F, J, 3, device="cuda"), torch.zeros(V, F, 3, device="cuda")
    tok = torch.ones(V, F, dtype=torch.uint8, device="cuda")
    off = torch.tensor([0, F], dtype=torch.int64, device="cuda")
    quat, trans = torch.full((G, V, 4), -1.0, device="cuda"), torch.full((G, V, 3), -1.0, device="cuda")
    rms, trms = torch.full((G, V), -1.0, device="cuda"), torch.full((G, V), -1.0, device="cuda")
    used, ok = torch.full((G, V), 7, dtype=torch.int32, device="cuda"), torch.full((G, V), 7, dtype=torch.uint8, device="cuda")
    p = lambda x: None if x is None else x.data_ptr()

    def call(x=poses, o=off, t=traj, k=tok, q=quat, tr=trans, r=rms, s=trms, u=used, g=ok, v=V, f=F, j=J, ch=3, G=G, sigma=0.05, iters=5):
        return lib.mp_lift_align_views(p(x), v, f, j, ch, None, p(o), G, p(t), p(k), sigma, iters, p(q), p(tr), p(r), p(s), p(u), p(g), None)
    for kw in (dict(x=None), dict(o=None), dict(q=None), dict(r=None), dict(u=None), dict(g=None)):
        assert call(**kw) == 1 and b"null" in lib.mp_last_error()
    for kw, word in ((dict(v=0), b"V=0"), (dict(v=5), b"V=5"), (dict(j=1), b"J=1"), (dict(j=33), b"J=33"), (dict(ch=2), b"C=2"), (dict(ch=5), b"C=5"),
                     (dict(f=0), b"out of range"), (dict(f=-1), b"out of range"), (dict(G=0), b"out of range"), (dict(G=7), b"out of range"),
                     (dict(f=2 ** 31), b"out of range"), (dict(sigma=0.0), b"sigma"), (dict(sigma=-1.0), b"sigma"), (dict(sigma=float("nan")), b"sigma"),
                     (dict(iters=-1), b"iters=-1"), (dict(iters=9), b"iters=9"), (dict(t=None), b"come together"), (dict(k=None), b"come together"),
                     (dict(tr=None), b"trans or trans_rms null"), (dict(s=None), b"trans or trans_rms null")):
        assert call(**kw) == 1 and word in lib.mp_last_error(), (kw, lib.mp_last_error())
    torch.cuda.synchronize()
    for t in (quat, trans, rms, trms):
        assert bool((t == -1).all())                                      # nothing was launched
    assert bool((used == 7).all()) and bool((ok == 7).all())
    assert call(t=None, k=None, tr=None, s=None) == 0                     # good arguments; without traj, trans and trans_rms may be null
    torch.cuda.synchronize()
    assert bool((trans == -1).all()) and bool((trms == -1).all()) and used[0].tolist() == [F] * V and ok[0].tolist() == [1, 0, 0]      # all-zero poses: M = 0
    assert call(sigma=float("inf"), iters=0) == 0
    torch.cuda.synchronize()
    assert bool((trans == 0).all()) and bool((trms == 0).all()) and bool((quat[..., 0] == 1).all())
    from manipose_amd import align_views
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        align_views(poses.cpu())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        align_views(poses, valid=torch.ones(V, F, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        align_views(poses, traj=traj.cpu(), traj_ok=tok)
    with pytest.raises(RuntimeError, match="out of range"):
        align_views(poses, take_offset=list(range(F + 2)))                # more takes than frames: the entry point's own refusal


def test_recovery_scene_on_the_device():
    """the scene of test_lift_align_host.test_recovery_on_the_committed_seed: the device's estimate is the statement's, so the claim is the device's"""
    dirty, clean = ref.recovery()
    angle = lambda r, sc: [ref.angle_deg(r["quat"][0, v], sc["quat"][0, v]) for v in range(1, 4)]
    plain = angle(_align(dirty["poses"], None, dirty["off"], iters=0), dirty)
    got = _align(dirty["poses"], None, dirty["off"], dirty["traj"], dirty["traj_ok"])
    robust, own = angle(got, dirty), angle(_align(clean["poses"], None, clean["off"], iters=0), clean)
    print("plain", np.round(plain, 3), "robust", np.round(robust, 3), "without outliers", np.round(own, 3))
    assert all(r < p for r, p in zip(robust, plain)) and all(r <= 2.0 * c for r, c in zip(robust, own)) and (got["ok"][0] == [1, 3, 3, 3]).all()
    _compare("recovery", got, ref.align(dirty["poses"], None, dirty["off"], dirty["traj"], dirty["traj_ok"]), True)
    cam = np.concatenate([np.ones(9), [0.5, -0.5, 0.5, 0.5], [1.0, 2.0, 3.0]])      # composed with a reference camera on the host
    placed = _align(dirty["poses"], None, dirty["off"], dirty["traj"], dirty["traj_ok"], reference=cam)
    want_q, want_t = ref.compose(got["quat"], got["trans"], got["ok"], [cam[9:13]], [cam[13:16]])
    assert np.abs(placed["quat"] - want_q).max() <= 2.0 ** -23 and np.abs(placed["trans"] - want_t).max() <= ref.ulp_bound(want_t)
    assert all(_same(placed[k], got[k]) for k in ("rms", "trans_rms", "used", "ok"))


# ---- end to end: the tiny fp32 fixture model of lift_fixtures.py -----------------------------------------------------------------------------
def _group(lens=(20, 20, 20, 20, 12, 12, 12), seed=51):
    """one group of 7 sequences: a take of 4 views of 20 frames, then a take of 3 views of 12 frames; S11's cameras as fetch() hands them on"""
    from manipose_amd.data.ingest import h36m_cameras
    s11 = h36m_cameras()["S11"]
    g = np.random.default_rng(seed)
    seqs = [np.clip(0.3 * g.standard_normal((n, 17, 2)), -1, 1).astype(np.float32) for n in lens]
    cams = [np.concatenate([s11[i]["intrinsic"], s11[i]["orientation"], s11[i]["translation"], np.array([i])]) for i in (0, 1, 2, 3, 0, 1, 2)]
    return {"walk": seqs}, {"walk": cams}


@pytest.mark.parametrize("frame", ["camera", "world"])
def test_run_lift_with_estimated_cameras_end_to_end(tmp_path, frame, capsys):
    from _entry import CAMERA_KEYS, lift_sequences_to_file, load_config
    from manipose_amd import align_views, place_poses
    model, T, K = _model("rmcl")
    groups, cams = _group()
    base = ["run.lift=true", "train.tta=false", "train.batch_size_test=2", "lift.hyps=true", "lift.fuse=true"]
    base += ["lift.frame=world", "lift.floor=true"] if frame == "world" else []
    before = lift_sequences_to_file(model, load_config(base), groups, str(tmp_path / "before.npz"), cams)
    named = lift_sequences_to_file(model, load_config(base + ["lift.fuse_cameras=dataset"]), groups, str(tmp_path / "dataset.npz"), cams)
    a, b = np.load(str(tmp_path / "before.npz")), np.load(str(tmp_path / "dataset.npz"))
    assert list(a.keys()) == list(b.keys()) == list(before) == list(named) and all(a[k].dtype == b[k].dtype and _same(a[k], b[k]) for k in a.keys())
    est = lift_sequences_to_file(model, load_config(base + ["lift.fuse_cameras=estimate"]), groups, str(tmp_path / "estimate.npz"), cams)
    new = sorted(set(est) - set(before))
    assert new == sorted(f"walk.fused{t}__cam_{k}" for t in (0, 1) for k in CAMERA_KEYS) and set(before) <= set(est)
    assert all(_same(est[k], v) for k, v in before.items() if ".fused" not in k)          # the views' own outputs do not change
    z = np.load(str(tmp_path / "estimate.npz"))
    assert all(_same(z[k], est[k]) for k in new)
    for t, (n, V) in enumerate(((20, 4), (12, 3))):
        k = f"walk.fused{t}__cam_"
        assert est[k + "quat"].shape == (V, 4) and est[k + "trans"].shape == (V, 3) and est[k + "used"].dtype == np.int32 and est[k + "ok"].dtype == np.uint8
        assert all(est[k + s].shape == (V,) for s in ("rms", "trans_rms", "used", "ok", "err_deg", "err_m"))
        assert est[k + "ok"][0] == 1 and est[k + "used"][0] == n and est[k + "err_deg"][0] < 1e-3 and est[k + "err_m"][0] < 1e-5      # the reference view keeps its camera
        assert est[f"walk.fused{t}"].shape == (n, 17, 3) and np.isfinite(est[f"walk.fused{t}"]).all()
    # the estimate is align_views' on the views' merged poses in their cameras' frames and their own fitted roots (take 0, lift.frame=camera)
    if frame == "camera":
        poses = _dev(np.stack([est[f"walk.{i}"] for i in range(4)]))
        poses = (poses - poses[:, :, :1]).contiguous()
        kp = _dev(np.stack(groups["walk"][:4]))
        intr = np.stack([c[:9] for c in cams["walk"][:4]]).astype(np.float32)
        traj, _, ok = place_poses(poses.reshape(80, 17, 3), kp.reshape(80, 17, 2), intr, [0, 20, 40, 60, 80], refine=3)
        want = align_views(poses, None, None, traj.reshape(4, 20, 3), ok.reshape(4, 20), reference=cams["walk"][0])
        for key, x in zip(CAMERA_KEYS[:6], want):
            assert _same(est["walk.fused0__cam_" + key], x[0].cpu().numpy()), key
    out = capsys.readouterr().out
    for t, V in enumerate((4, 3)):                                        # a view without a rotation is reported and left out
        lost = [v for v in range(V) if not est[f"walk.fused{t}__cam_ok"][v] & 1]
        assert all(f"take {t}, view {v + 4 * t}: its rotation could not be estimated" in out for v in lost)


def test_estimated_cameras_in_synthetic_mode(lib, tmp_path, monkeypatch):
    """run.lift with lift.fuse and lift.fuse_cameras=estimate on synthetic data: every take has one view, which keeps its dataset camera"""
    from _entry import run
    monkeypatch.chdir(tmp_path)
    argv = ["run.train=false", "run.test=false", "run.lift=true", "lift.stride=14", "train.batch_size_test=4", "data.seq_len=27", "model.channels=64",
            "model.layers=2", "model.nheads=4", "model.channels_seg=32", "model.layers_seg=1", "model.nheads_seg=4", "multi_hyp.n_hyp=3",
            "data.synthetic_sequences=2", "model.precision=fp32", "lift.frame=world", "lift.floor=true", "lift.fuse=true"]
    run(argv)
    out = os.path.join(str(tmp_path), "default")
    before = dict(np.load(os.path.join(out, "lift.npz")))
    run(argv + ["lift.fuse_cameras=estimate"])
    z = np.load(os.path.join(out, "lift.npz"))
    assert all(_same(z[k], v) for k, v in before.items() if ".fused" not in k) and set(before) <= set(z.files)
    for name in ("synthetic_000", "synthetic_001"):
        k = f"{name}.fused0__cam_"
        assert z[k + "ok"].tolist() == [1] and z[k + "err_deg"][0] < 1e-3 and z[k + "err_m"][0] < 1e-5 and z[k + "quat"].shape == (1, 4)
        assert np.abs(z[f"{name}.fused0"] - before[f"{name}.fused0"]).max() < 1e-4      # the same camera up to the quaternion's normalisation

"""Fusing the camera views of a take on the device: mp_lift_fuse and mp_lift_fuse_place against the float64 statement of their rules
(lift_fuse_ref.py), the constructed cases compared exactly, the recovery scene the feature is for, the invariants (identical bits, takes alone and
together, inputs untouched, invalid views never read), argument errors, and run.lift with lift.fuse end to end.

The bound, everywhere a float32 is compared with float64: |x - x64| <= 2^-23 max(1, |x64|) (lift_place_ref.TOL).  The kernels compute in fp64 between
their float32 loads and stores and the joint fit is well conditioned (cond(H) about 6 with S11's four cameras), so against the float64 statement ON
THE SAME float32 INPUTS only fp64 noise and the final rounding remain; the bound is not measured from the kernels.  choice, ok and steps are compared
for equality: test_lift_fuse_host.py shows every E gap of these scenes at least 1e-6 (1 + |E|) and every threshold decision at least 1e-3 from its
threshold."""
import os
import sys

import numpy as np
import pytest
import torch

import lift_fuse_ref as ref
import lift_place_ref as place
from lift_fixtures import fixture_model as _model, same as _same

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hpe"))


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _fuse(hyps, quat=None, valid=None, off=None, sigma=0.02, score_weight=1.0):
    from manipose_amd import fuse_views
    res = fuse_views(_dev(hyps), quat, _dev(valid), off, sigma, score_weight)
    torch.cuda.synchronize()
    return dict(zip(("pose", "choice", "cost", "spread", "ok"), (r.cpu().numpy() for r in res)))


def _nested(cams):
    """the (G, V, .) tables as place_views' nested list of 16-number cameras"""
    quat, trans, intr = cams
    return [[np.concatenate([intr[g, v], quat[g, v], trans[g, v]]) for v in range(quat.shape[1])] for g in range(quat.shape[0])]


def _place(pose, kp, cams, valid=None, off=None, weights=None, distort=True, iters=3):
    from manipose_amd import place_views
    res = place_views(_dev(pose), _dev(kp), _nested(cams), _dev(valid), off, weights, distort, iters, return_steps=True)
    torch.cuda.synchronize()
    return [r.cpu().numpy() for r in res]


def _check(tag, got, want):
    print(f"[{tag}] worst error = {place.worst(got, want):.3f} x the bound 2^-23 max(1, |x|)")
    assert place.within(got, want).all(), tag


@pytest.mark.parametrize("n", range(17))
def test_fuse_matches_the_statement(n):
    tag, hyps, quat, valid, off, want = ref.fuse_cases()[n]
    got = _fuse(hyps, quat, valid, off)
    assert np.array_equal(got["choice"], want["choice"]) and np.array_equal(got["ok"], want["ok"]), tag
    for k in ("pose", "cost", "spread"):
        _check(f"{tag}: {k}", got[k], want[k])
    assert not got["pose"][:, 0].any() and not np.signbit(got["pose"][:, 0]).any()                # joint 0 is +0
    if valid is not None:
        assert np.array_equal(got["choice"] == 255, valid.T == 0)


def test_fuse_constructed_cases():
    hyps, quat, off = ref.fuse_scene(4, 5, 4, lens=[8], seed=31)
    clean = _fuse(hyps, quat, None, off)
    twin, first = hyps.copy(), np.zeros(8, np.uint8)
    for f in range(8):                                                    # the winner of view 1 copied bit for bit over its neighbour: the lower index wins
        w = int(clean["choice"][f, 1])
        twin[1, f, (w + 1) % 5] = twin[1, f, w]
        first[f] = min(w, (w + 1) % 5)
    got = _fuse(twin, quat, None, off)
    assert np.array_equal(got["choice"][:, 1], first) and np.array_equal(got["choice"][:, [0, 2, 3]], clean["choice"][:, [0, 2, 3]])
    assert _same(got["cost"], clean["cost"]) and _same(got["pose"], clean["pose"])
    nan = hyps.copy()
    for f in range(8):
        nan[2, f, clean["choice"][f, 2], 5, 1] = np.nan                   # the hypothesis that won in view 2 gets a NaN coordinate
    nan[:, 7, :, 3, 0] = np.nan                                           # frame 7: every hypothesis of every view
    got = _fuse(nan, quat, None, off)
    assert (got["choice"][:7, 2] != clean["choice"][:7, 2]).all() and got["ok"][:7].all() and np.isfinite(got["pose"][:7]).all()
    assert got["ok"][7] == 0 and got["cost"][7] >= 1e30
    valid = np.ones((4, 8), np.uint8)
    valid[:, 4] = 0                                                       # frame 4: no valid view
    got = _fuse(hyps, quat, valid, off)
    assert not got["pose"][4].any() and (got["choice"][4] == 255).all() and got["cost"][4] == 0 and got["spread"][4] == 0 and got["ok"][4] == 0
    assert all(_same(got[k][np.arange(8) != 4], clean[k][np.arange(8) != 4]) for k in clean)
    blind = _fuse(hyps, quat, None, off, sigma=float("inf"))
    assert np.array_equal(blind["choice"], hyps[..., 0, 3].argmax(axis=-1).T)       # sigma = inf: the per-view first arg-max of the score


def test_fuse_ignores_a_view_with_a_zero_quaternion(lib):
    from manipose_amd.lift_views import _fuse as launch
    hyps, quat, off = ref.fuse_scene(4, 5, 4, lens=[3, 5], seed=32)
    dead = quat.copy()
    dead[1, 2] = 0                                                        # view 2 of take 1 (fuse_views refuses this table: the entry point itself)
    valid = np.ones((4, 8), np.uint8)
    valid[2, 3:] = 0
    res = launch(lib, _dev(hyps), None, _dev(off), 2, _dev(dead), 0.02, 1.0)
    want = _fuse(hyps, quat, valid, off)
    assert all(_same(r.cpu().numpy(), want[k]) for r, k in zip(res, ("pose", "choice", "cost", "spread", "ok")))
    assert (want["choice"][3:, 2] == 255).all() and (want["choice"][:3] != 255).all()


@pytest.mark.parametrize("n", range(8))
def test_fuse_place_matches_the_statement(n):
    tag, pose, kp, cams, valid, off, weights, distort, iters, want, _ = ref.place_cases()[n]
    got = _place(pose, kp, cams, valid, off, weights, bool(distort), iters)
    _check(f"{tag}: root", got[0], want[0])
    _check(f"{tag}: reproj", got[1], want[1])
    assert np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3]) and got[2].all(), tag
    if valid is not None:
        assert not got[1][valid == 0].any() and (got[1][valid == 1] > 0).all()


def test_fuse_place_degenerate_frames():
    pose, kp, cams, off, valid = ref.degenerate_place_scene()
    want = ref.place_all(pose, kp, *cams, valid, off, iters=3)
    got = _place(pose, kp, cams, valid, off)
    _check("degenerate scene: root", got[0], want[0])
    _check("degenerate scene: reproj", got[1], want[1])
    assert np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3])
    assert got[2][ref.ONE_SPOT] == 1 and got[3][ref.ONE_SPOT] == 3      # four views: the rays through the four spots still meet in one root
    assert got[2][ref.BEHIND] == 0 and got[3][ref.BEHIND] == 0 and got[0][ref.BEHIND].any()
    assert got[2][ref.NO_VIEW] == 0 and not got[0][ref.NO_VIEW].any() and not got[1][:, ref.NO_VIEW].any() and got[3][ref.NO_VIEW] == 0
    one = np.zeros((4, 8), np.uint8)
    one[0] = 1                                                            # one view alone: all keypoints on one spot is a degenerate fit
    got = _place(pose, kp, cams, one, off)
    assert got[2][ref.ONE_SPOT] == 0 and not got[0][ref.ONE_SPOT].any() and not got[1][:, ref.ONE_SPOT].any() and got[3][ref.ONE_SPOT] == 0


def test_two_small_takes_a_missing_view_and_a_device_offset_table():
    """The smallest shape at which what fuse_views / fuse_views_path and place_views / bundle_views share in front of their launchers can go wrong:
    V = 2, K = 2, J = 3, takes of 1 and 2 frames, view 1 missing in the second take - for place_views said by None in the cameras ALONE
    (valid=None: the mask is made from the cameras), for fuse_views by valid - and the (G + 1) offsets a DEVICE table, so the number of takes is
    read from its size.  Against the float64 statement within the store bound; the decisions' margins are those of the host test."""
    from manipose_amd import place_views
    valid = np.ones((2, 3), np.uint8)
    valid[1, 1:] = 0
    hyps, quat, off = ref.fuse_scene(2, 2, 4, J=3, lens=[1, 2], seed=42)
    want = ref.fuse_all(hyps, quat, valid, off)
    assert (want["gap"] / (1.0 + np.abs(want["cost"]))).min() >= 1e-6
    got = _fuse(hyps, quat, valid, _dev(np.asarray(off, np.int64)))
    assert np.array_equal(got["choice"], want["choice"]) and np.array_equal(got["ok"], want["ok"]) and (got["choice"][1:, 1] == 255).all()
    for k in ("pose", "cost", "spread"):
        _check(f"two small takes: {k}", got[k], want[k])
    pose, kp, _, cams, off = ref.place_scene(2, J=3, lens=[1, 2], seed=42)
    trace = []
    want = ref.place_all(pose, kp, *cams, valid, off, iters=3, trace=trace)
    assert ref.margin(trace) >= 1e-3
    nested = _nested(cams)
    nested[1][1] = None
    got = [r.cpu().numpy() for r in place_views(_dev(pose), _dev(kp), nested, None, _dev(np.asarray(off, np.int64)), None, True, 3, return_steps=True)]
    _check("two small takes: root", got[0], want[0])
    _check("two small takes: reproj", got[1], want[1])
    assert np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3]) and got[2].all() and not got[1][1, 1:].any() and (got[1][0] > 0).all()


def test_one_view_at_the_identity_is_place_poses():
    """V = 1 with no quaternion table and no translation is mp_lift_place_refine's problem: the two kernels agree to the bound"""
    from manipose_amd import place_poses
    from manipose_amd.lift_views import _fuse_place
    from manipose_amd import _lib
    import lift_refine_ref as refine
    poses, kp, _, off = refine.recovery_scene()
    intr = refine.s11_intrinsics()
    pose = np.ascontiguousarray(poses[:, 0, :, :3])
    want = place_poses(_dev(pose), _dev(kp), intr, off, refine=3, return_steps=True)
    got = _fuse_place(_lib.load(), _dev(pose), _dev(kp[None]), None, _dev(off), 3, None, _dev(np.zeros((3, 1, 3), np.float32)), _dev(intr[:, None]), None, True, 3)
    torch.cuda.synchronize()
    _check("one view: root", got[0].cpu().numpy(), want[0].double().cpu().numpy())
    assert torch.equal(got[2], want[2]) and torch.equal(got[3], want[3]) and bool(got[2].all())
    assert (got[1][0] - want[1]).abs().max().item() <= 2.0 ** -23


def test_recovery_scene_on_the_device():
    sc = ref.recovery_scene()
    got = _fuse(sc["hyps"], sc["cams"][0], None, sc["off"])
    assert np.array_equal(got["choice"], sc["truth"]) and got["ok"].all()
    root, reproj, ok, steps = _place(sc["pose"], sc["kp"], sc["cams"], None, sc["off"])
    miss = np.linalg.norm(root - sc["root"], axis=1).max()
    print(f"[recovery] root within {miss:.2e} m of the true one after 3 steps (the host test's bound: {ref.ROOT_MISS[3]:.1e} m; the true roots are float32 numbers)")
    assert ok.all() and (steps == 3).all() and miss <= ref.ROOT_MISS[3]
    fused = _place(got["pose"], sc["kp"], sc["cams"], None, sc["off"])   # the fused pose, true to a millimetre, puts the root within millimetres
    assert fused[2].all() and np.linalg.norm(fused[0] - sc["root"], axis=1).max() <= 5e-3


def test_invariants():
    hyps, quat, off = ref.fuse_scene(4, 5, 4, seed=41)
    valid = ref.valid_table(4, off, 41)
    d_hyps = _dev(hyps)
    from manipose_amd import fuse_views, place_views
    a = fuse_views(d_hyps, quat, _dev(valid), off)
    b = fuse_views(d_hyps, quat, _dev(valid), off)
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and _same(d_hyps.cpu().numpy(), hyps)    # identical bits; the input is unchanged
    spoiled = hyps.copy()
    spoiled[valid == 0] = np.nan                                          # an invalid view's data is never looked at
    c = _fuse(spoiled, quat, valid, off)
    assert all(_same(c[k], x.cpu().numpy()) for k, x in zip(("pose", "choice", "cost", "spread", "ok"), a))
    pose, kp, _, cams, _ = ref.place_scene(4, seed=5)
    spoiled_kp = kp.copy()
    spoiled_kp[valid == 0] = np.nan
    d_pose, d_kp = _dev(pose), _dev(spoiled_kp)
    p = place_views(d_pose, d_kp, _nested(cams), _dev(valid), off, return_steps=True)
    q = place_views(d_pose, d_kp, _nested(cams), _dev(valid), off, return_steps=True)
    clean = _place(pose, kp, cams, valid, off)
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(p, q)) and all(_same(x.cpu().numpy(), y) for x, y in zip(p, clean))
    assert _same(d_pose.cpu().numpy(), pose) and _same(d_kp.cpu().numpy(), spoiled_kp)
    for t in range(3):                                                    # a take alone: the bits it has among the others
        sl = slice(int(off[t]), int(off[t + 1]))
        alone = _fuse(hyps[:, sl], quat[t:t + 1], valid[:, sl], None)
        assert all(_same(alone[k], x[sl].cpu().numpy()) for k, x in zip(("pose", "choice", "cost", "spread", "ok"), a))
        alone = _place(pose[sl], kp[:, sl], tuple(c[t:t + 1] for c in cams), valid[:, sl], None)
        assert _same(alone[0], clean[0][sl]) and _same(alone[1], clean[1][:, sl]) and _same(alone[2], clean[2][sl]) and _same(alone[3], clean[3][sl])


def test_entry_points_reject_bad_arguments_before_any_launch(lib):
    V, F, K, J = 4, 6, 5, 17
    hyps, kp = torch.zeros(V, F, K, J, 4, device="cuda"), torch.zeros(V, F, J, 2, device="cuda")
    off = torch.tensor([0, F], dtype=torch.int64, device="cuda")
    quat, trans, intr = (_dev(t) for t in ref.s11_tables())
    pose, root = torch.full((F, J, 3), -1.0, device="cuda"), torch.full((F, 3), -1.0, device="cuda")
    cost, spread, reproj = torch.full((F,), -1.0, device="cuda"), torch.full((F,), -1.0, device="cuda"), torch.full((V, F), -1.0, device="cuda")
    choice, ok, steps = (torch.full(s, 7, dtype=torch.uint8, device="cuda") for s in ((F, V), (F,), (F,)))
    p = lambda x: None if x is None else x.data_ptr()

    def fuse(h=hyps, o=off, q=quat, out=pose, c=choice, e=cost, s=spread, g=ok, v=V, f=F, k=K, j=J, ch=4, G=1, sigma=0.02, w=1.0):
        return lib.mp_lift_fuse(p(h), v, f, k, j, ch, None, p(o), G, p(q), sigma, w, p(out), p(c), p(e), p(s), p(g), None)
    for kw in (dict(h=None), dict(o=None), dict(out=None), dict(c=None), dict(e=None), dict(s=None), dict(g=None)):
        assert fuse(**kw) == 1 and b"null" in lib.mp_last_error()
    for kw, word in ((dict(v=0), b"V=0"), (dict(v=5), b"V=5"), (dict(k=0), b"K=0"), (dict(k=9), b"K=9"), (dict(j=1), b"J=1"), (dict(j=33), b"J=33"),
                     (dict(ch=2), b"C=2"), (dict(ch=5), b"C=5"), (dict(f=0), b"out of range"), (dict(f=-1), b"out of range"), (dict(G=0), b"out of range"),
                     (dict(G=7), b"out of range"), (dict(sigma=0.0), b"sigma"), (dict(sigma=-1.0), b"sigma"), (dict(sigma=float("nan")), b"sigma"),
                     (dict(w=-1.0), b"score_weight"), (dict(w=float("inf")), b"score_weight"), (dict(w=float("nan")), b"score_weight"),
                     (dict(f=2 ** 40, G=1), b"too many for one launch")):
        assert fuse(**kw) == 1 and word in lib.mp_last_error(), (kw, lib.mp_last_error())

    def put(x=pose, u=kp, o=off, q=quat, t=trans, i=intr, r=root, e=reproj, g=ok, n=steps, v=V, f=F, j=J, G=1, distort=1, iters=3):
        return lib.mp_lift_fuse_place(p(x), p(u), v, f, j, None, p(o), G, p(q), p(t), p(i), None, distort, iters, p(r), p(e), p(g), p(n), None)
    for kw in (dict(x=None), dict(u=None), dict(o=None), dict(t=None), dict(i=None), dict(r=None), dict(e=None), dict(g=None)):
        assert put(**kw) == 1 and b"null" in lib.mp_last_error()
    for kw, word in ((dict(v=0), b"V=0"), (dict(v=5), b"V=5"), (dict(j=1), b"J=1"), (dict(j=33), b"J=33"), (dict(f=0), b"out of range"),
                     (dict(G=0), b"out of range"), (dict(G=7), b"out of range"), (dict(distort=2), b"distort=2"), (dict(iters=17), b"iters=17"),
                     (dict(iters=-1), b"iters=-1"), (dict(f=2 ** 40), b"too many for one launch")):
        assert put(**kw) == 1 and word in lib.mp_last_error(), (kw, lib.mp_last_error())
    torch.cuda.synchronize()
    for t in (pose, root, cost, spread, reproj):
        assert bool((t == -1).all())                                      # nothing was launched
    assert bool((choice == 7).all()) and bool((ok == 7).all()) and bool((steps == 7).all())
    assert fuse() == 0 and fuse(q=None) == 0 and fuse(sigma=float("inf"), w=0.0) == 0                   # good arguments; quat may be null
    torch.cuda.synchronize()
    assert bool((choice == 0).all()) and bool((ok == 1).all()) and bool((pose == 0).all()) and bool((spread == 0).all())      # all hypotheses alike
    assert put(x=torch.zeros(F, J, 3, device="cuda"), n=None) == 0                                      # steps may be null
    torch.cuda.synchronize()
    assert bool((reproj != -1).all()) and bool((root != -1).all()) and bool((ok != 7).all()) and bool((steps == 7).all())
    from manipose_amd import fuse_views, place_views
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fuse_views(hyps.cpu())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fuse_views(hyps, valid=torch.ones(V, F, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        place_views(pose, kp.cpu(), _nested(ref.s11_tables()))
    with pytest.raises(RuntimeError, match="place_views takes device tensors"):
        place_views(pose, kp, _nested(ref.s11_tables()), valid=torch.ones(kp.shape[0], kp.shape[1], dtype=torch.uint8))
    with pytest.raises(ValueError, match="takes"):
        place_views(pose, kp, _nested(ref.s11_tables()), take_offset=[0, 2, F])
    with pytest.raises(RuntimeError, match="out of range"):
        fuse_views(hyps, take_offset=list(range(F + 2)))                  # more takes than frames: the entry point's own refusal


# ---- end to end: the tiny fp32 fixture model of lift_fixtures.py -----------------------------------------------------------------------------
def _group(lens=(20, 20, 20, 20, 12, 12, 12), seed=51):
    """one group of 7 sequences: a take of 4 views of 20 frames, then a take of 3 views of 12 frames; S11's cameras as fetch() hands them on"""
    from manipose_amd.data.ingest import h36m_cameras
    s11 = h36m_cameras()["S11"]
    g = np.random.default_rng(seed)
    seqs = [np.clip(0.3 * g.standard_normal((n, 17, 2)), -1, 1).astype(np.float32) for n in lens]
    cams = [np.concatenate([s11[i]["intrinsic"], s11[i]["orientation"], s11[i]["translation"], np.array([i])]) for i in (0, 1, 2, 3, 0, 1, 2)]
    return {"walk": seqs}, {"walk": cams}


def test_run_lift_fuse_end_to_end(tmp_path):
    from _entry import lift_sequences_to_file, load_config
    from manipose_amd import fuse_views, place_views, to_world
    model, T, K = _model("rmcl")
    groups, cams = _group()
    base = ["run.lift=true", "train.tta=false", "train.batch_size_test=2", "lift.hyps=true"]
    off_file, on_file, plain_file = (str(tmp_path / n) for n in ("off.npz", "on.npz", "plain.npz"))
    plain = lift_sequences_to_file(model, load_config(base), groups, plain_file)
    off = lift_sequences_to_file(model, load_config(base + ["lift.fuse=false"]), groups, off_file, cams)
    a, b = np.load(plain_file), np.load(off_file)                        # lift.fuse off: the file holds what it holds without the key, in the same order
    assert list(a.keys()) == list(b.keys()) == list(plain) and all(a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and _same(a[k], b[k]) for k in a.keys())
    on = lift_sequences_to_file(model, load_config(base + ["lift.fuse=true"]), groups, on_file, cams)
    assert all(_same(on[k], v) for k, v in off.items())                  # what was written before is written as before
    new = sorted(set(on) - set(off))
    suffixes = ("", "__root", "__choice", "__spread", "__cost", "__ok", "__reproj", "__steps", "__views")
    assert new == sorted(f"walk.fused{t}{s}" for t in (0, 1) for s in suffixes)
    hyps = np.zeros((4, 32, K, 17, 4), np.float32)
    kp, valid = np.zeros((4, 32, 17, 2), np.float32), np.ones((4, 32), np.uint8)
    for t, (views, sl) in enumerate((((0, 1, 2, 3), slice(0, 20)), ((4, 5, 6), slice(20, 32)))):
        for v, i in enumerate(views):
            hyps[v, sl], kp[v, sl] = on[f"walk.{i}__hyps"], groups["walk"][i]
    valid[3, 20:] = 0
    quat = np.stack([np.stack([c[9:13] for c in cams["walk"][:4]]), np.stack([c[9:13] for c in cams["walk"][4:]] + [np.array([1.0, 0, 0, 0])])])
    nested = [cams["walk"][:4], cams["walk"][4:] + [None]]
    pose, choice, cost, spread, ok = fuse_views(_dev(hyps), quat, _dev(valid), [0, 20, 32])
    root, reproj, placed, steps = place_views(pose, _dev(kp), nested, _dev(valid), [0, 20, 32], return_steps=True)
    scene = to_world(pose.clone(), np.tile(np.array([1, 0, 0, 0], np.float32), (2, 1)), traj=root, seq_offset=[0, 20, 32])
    for t, (n, V, sl) in enumerate(((20, 4, slice(0, 20)), (12, 3, slice(20, 32)))):
        k = f"walk.fused{t}"
        assert on[k].shape == (n, 17, 3) and on[k + "__root"].shape == (n, 3) and on[k + "__choice"].shape == (n, V) and on[k + "__reproj"].shape == (V, n)
        assert all(on[k + s].shape == (n,) for s in ("__spread", "__cost", "__ok", "__steps"))
        assert on[k + "__views"].tolist() == ([0, 1, 2, 3] if t == 0 else [4, 5, 6])
        assert _same(on[k], scene[sl].cpu().numpy()) and _same(on[k + "__root"], root[sl].cpu().numpy())
        assert _same(on[k + "__choice"], choice[sl, :V].cpu().numpy()) and _same(on[k + "__cost"], cost[sl].cpu().numpy())
        assert _same(on[k + "__spread"], spread[sl].cpu().numpy()) and _same(on[k + "__ok"], (ok[sl] & placed[sl]).cpu().numpy())
        assert _same(on[k + "__reproj"], reproj[:V, sl].cpu().numpy()) and _same(on[k + "__steps"], steps[sl].cpu().numpy())
        assert (on[k + "__choice"] < K).all()
    quiet = lift_sequences_to_file(model, load_config(["run.lift=true", "train.tta=false", "train.batch_size_test=2", "lift.fuse=true"]), groups,
                                   str(tmp_path / "quiet.npz"), cams)
    assert not any("hyps" in k for k in quiet) and all(_same(quiet[k], on[k]) for k in new)       # the fusion reads hypotheses lift.hyps does not write
    uneven, _ = _group((20, 20, 20, 19, 12, 12, 12))
    with pytest.raises(ValueError, match="same frames"):
        lift_sequences_to_file(model, load_config(base + ["lift.fuse=true"]), uneven, str(tmp_path / "bad.npz"), cams)


def test_fuse_entry_point_in_synthetic_mode(lib, tmp_path, monkeypatch, capsys):
    """run.lift with lift.fuse, lift.rigid, lift.frame=world, lift.floor and lift.score on synthetic data: every take has one view, which runs and says so"""
    import csv
    from _entry import run
    monkeypatch.chdir(tmp_path)
    argv = ["run.train=false", "run.test=false", "run.lift=true", "lift.stride=14", "train.batch_size_test=4", "data.seq_len=27", "model.channels=64",
            "model.layers=2", "model.nheads=4", "model.channels_seg=32", "model.layers_seg=1", "model.nheads_seg=4", "multi_hyp.n_hyp=3",
            "data.synthetic_sequences=2", "model.precision=fp32", "lift.score=true", "lift.rigid=true", "lift.frame=world", "lift.floor=true"]
    run(argv)
    out = os.path.join(str(tmp_path), "default")
    before = dict(np.load(os.path.join(out, "lift.npz")))
    head = list(csv.reader(open(os.path.join(out, "lift_score.csv"))))[0]
    run(argv + ["lift.fuse=true"])
    assert "every take has one view" in capsys.readouterr().out
    z = np.load(os.path.join(out, "lift.npz"))
    assert all(_same(z[k], v) for k, v in before.items())                # what was written without lift.fuse is written as before
    assert list(csv.reader(open(os.path.join(out, "lift_score.csv"))))[0] == head
    suffixes = ("", "__root", "__choice", "__spread", "__cost", "__ok", "__reproj", "__steps", "__views", "__floor")
    assert sorted(set(z.files) - set(before)) == sorted(f"synthetic_{i:03d}.fused0{s}" for i in range(2) for s in suffixes)
    for i in range(2):
        k, n = f"synthetic_{i:03d}.fused0", 27 * 4 + 37 * i + 11
        assert z[k].shape == (n, 17, 3) and z[k + "__choice"].shape == (n, 1) and z[k + "__reproj"].shape == (1, n) and z[k + "__views"].tolist() == [0]
        assert (z[k + "__choice"] < 3).all() and not z[k + "__spread"].any()      # one view: the mean of one hypothesis
        assert z[k][..., 2].min() == 0 and z[k + "__floor"].shape == ()         # the take stands on z = 0
        bones = np.linalg.norm(z[k][:, 1:] - z[k][:, [0, 1, 2, 0, 4, 5, 0, 7, 8, 9, 8, 11, 12, 8, 14, 15]], axis=-1)
        assert np.abs(bones - before[f"synthetic_{i:03d}__bones"]).max() <= 1e-5  # lift.rigid: the views' bone table (one view: its own)
    rows = list(csv.reader(open(os.path.join(out, "lift_score_fused.csv"))))
    assert rows[0][:4] == ["act", "frames", "mpjpe", "p_mpjpe"] and rows[0][-2:] == ["traj_ate", "traj_frames"]
    assert [r[0] for r in rows[1:]] == ["synthetic_000.fused0", "synthetic_001.fused0", "average"] and float(rows[1][1]) == 27 * 4 + 11

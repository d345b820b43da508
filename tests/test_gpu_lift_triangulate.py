"""Triangulating a fused take's joints on the device: mp_lift_triangulate against the float64 statement of its rule (lift_triangulate_ref.py), the
constructed items compared exactly, the invariants (identical bits, a take alone and beside others, inputs untouched), argument errors, the
recovery scene the feature is for, and run.lift with lift.fuse_triangulate end to end.

The bounds against the statement, ON THE SAME float32 INPUTS: views, ok and steps are equal; every stored float (points, err) is within
2^-23 max(1, |x|), the project's bound for a float32 store.  The kernel and the statement both work in fp64 with the same operations in the same
order (no contraction, IEEE division and square root), so what remains is the one rounding to float32.  That holds where every decision is away
from its threshold, which test_lift_triangulate_host.py asserts of every compared scene without a device; the bounds are not measured from the
kernel.  No item is excluded from a comparison."""
import os
import sys

import numpy as np
import pytest
import torch

import lift_triangulate_ref as ref
from lift_fixtures import fixture_model as _model, same as _same

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hpe"))
KEYS = ("points", "err", "views", "ok", "steps")
INF = float("inf")


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _cameras(quat, trans, intr):
    """place_views' nested list of the (G, V, .) tables"""
    G, V = quat.shape[:2]
    return [[np.concatenate([intr[g, v], quat[g, v], trans[g, v]]) for v in range(V)] for g in range(G)]


def _tri(pose, root, kp, quat, trans, intr, valid=None, take_offset=None, root_ok=None, kp_weight=None, distort=True, sigma=INF, prior=0.0, iters=3):
    from manipose_amd import triangulate_views
    G = 1 if take_offset is None else len(take_offset) - 1
    quat, trans, intr = (np.asarray(a).reshape(G, kp.shape[0], -1) for a in (quat, trans, intr))
    res = triangulate_views(_dev(pose), _dev(root), _dev(kp), _cameras(quat, trans, intr), _dev(valid), take_offset, _dev(root_ok), _dev(kp_weight),
                            distort, sigma, prior, iters)
    torch.cuda.synchronize()
    return {k: getattr(res, k).cpu().numpy() for k in KEYS}


def _compare(tag, got, want, rows=None):
    rows = slice(None) if rows is None else rows
    assert got["points"].dtype == got["err"].dtype == np.float32 and got["views"].dtype == got["ok"].dtype == got["steps"].dtype == np.uint8
    for k in ("views", "ok", "steps"):
        assert np.array_equal(got[k][rows], want[k][rows]), (tag, k, np.argwhere(got[k][rows] != want[k][rows])[:5])
    worst = {k: ref.within_store(got[k][rows], want[k][rows])[1] for k in ("points", "err")}
    print(f"[{tag}] of 2^-23 max(1, |x|): " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert all(v <= 1.0 for v in worst.values()), (tag, worst)


@pytest.mark.parametrize("n", range(len(ref.cases())))
def test_triangulate_matches_the_statement(n):
    tag, inp, want, _ = ref.cases()[n]
    _compare(tag, _tri(**inp), want)


def _raw(lib, inp, **over):
    """the entry point itself on an inputs dict, the outputs pre-filled: points and err with -1, the bytes with 7"""
    V, F, J = inp["kp"].shape[:3]
    off = np.asarray(inp.get("take_offset", [0, F]), np.int64)
    G = len(off) - 1
    d = {k: _dev(np.ascontiguousarray(inp[k])) for k in ("pose", "root", "kp", "quat", "trans", "intr")}
    d["off"] = _dev(off)
    out = dict(points=torch.full((F, J, 3), -1.0, device="cuda"), err=torch.full((F, J), -1.0, device="cuda"),
               views=torch.full((F, J), 7, dtype=torch.uint8, device="cuda"), ok=torch.full((F, J), 7, dtype=torch.uint8, device="cuda"),
               steps=torch.full((F, J), 7, dtype=torch.uint8, device="cuda"))
    a = dict(pose=d["pose"], root=d["root"], kp=d["kp"], V=V, F=F, J=J, off=d["off"], G=G, quat=d["quat"], trans=d["trans"], intr=d["intr"],
             distort=int(inp.get("distort", True)), sigma=float(inp.get("sigma", INF)), prior=float(inp.get("prior", 0.0)), iters=int(inp.get("iters", 3)),
             **{"o_" + k: v for k, v in out.items()})
    a.update(over)
    p = lambda x: x.data_ptr() if torch.is_tensor(x) else x
    rc = lib.mp_lift_triangulate(p(a["pose"]), p(a["root"]), None, p(a["kp"]), None, a["V"], a["F"], a["J"], None, p(a["off"]), a["G"], p(a["quat"]),
                                 p(a["trans"]), p(a["intr"]), a["distort"], a["sigma"], a["prior"], a["iters"], p(a["o_points"]), p(a["o_err"]),
                                 p(a["o_views"]), p(a["o_ok"]), p(a["o_steps"]), None)
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in out.items()}
    got["rc"] = rc
    return got


def test_constructed_items_are_exact(lib):
    inp = ref.constructed()
    got, want = _tri(**inp), ref.triangulate(**inp)
    _compare("one rule per frame", got, want)
    X0 = (inp["pose"].astype(np.float64) + inp["root"].astype(np.float64)[:, None]).astype(np.float32)
    for f in (ref.NO_VIEW, ref.ONE_VIEW, ref.WEIGHTS, ref.BEHIND):        # the prior point itself: its fp64 sum rounded once, bit for bit
        assert _same(got["points"][f], X0[f]) and (got["steps"][f] == 0).all() and (got["ok"][f] == 1).all()
    f = ref.NOTHING
    assert not got["points"][f].any() and not got["err"][f].any() and not got["ok"][f].any() and not got["steps"][f].any() and not got["views"][f].any()
    assert (got["views"][ref.NAN_KP] == 0b1101).all() and (got["views"][ref.WEIGHTS] == 0b1000).all() and (got["ok"][ref.NO_ROOT] == 3).all()
    assert not got["err"][ref.NO_VIEW].any() and (got["err"][ref.ONE_VIEW] > 0).all()
    pulled = ref.constructed(prior=0.01)
    _compare("one rule per frame, prior 0.01", _tri(**pulled), ref.triangulate(**pulled))
    twins = ref.twins()
    got = _tri(**twins)
    _compare("two views with identical cameras", got, ref.triangulate(**twins))
    assert (got["ok"] == 1).all() and (got["steps"] == 0).all()
    assert _same(got["points"], (twins["pose"].astype(np.float64) + twins["root"].astype(np.float64)[:, None]).astype(np.float32))
    zero = ref.zero_quaternion()                                          # (triangulate_views' cameras refuse a zero quaternion: through the entry point)
    got = _raw(lib, zero)
    assert got["rc"] == 0 and (got["views"] == 0b110).all()
    _compare("a zero quaternion", got, ref.triangulate(**zero))
    sc = ref.scene(2, 5, [6], seed=423)                                   # a frame no take holds is left unwritten
    part = ref.inputs(sc, take_offset=[1, 4])
    got, want = _raw(lib, part), ref.triangulate(**part)
    assert got["rc"] == 0 and want["written"].tolist() == [False, True, True, True, False, False]
    _compare("frames 1 to 3 of 6", got, want, rows=slice(1, 4))
    for f in (0, 4, 5):
        assert (got["points"][f] == -1).all() and (got["err"][f] == -1).all() and (got["views"][f] == 7).all() and (got["ok"][f] == 7).all() and (got["steps"][f] == 7).all()


def test_invariants():
    from manipose_amd import triangulate_views
    sc = ref.scene(4, 17, [1, 9, 6], seed=410)
    ftot = int(sc["off"][-1])
    valid, root_ok = ref.gap_tables(4, ftot, 411)
    w = ref.weight_table(4, ftot, 17, 412)
    spoiled = sc["kp"].copy()
    spoiled[valid == 0] = np.nan                                          # an invalid view's frame is never looked at
    cams = _cameras(sc["quat"], sc["trans"], sc["intr"])
    d = [_dev(a) for a in (sc["pose"], sc["root"], spoiled, valid, root_ok, w)]
    a = triangulate_views(d[0], d[1], d[2], cams, d[3], sc["off"], d[4], d[5], sigma=0.05, prior=0.01)
    b = triangulate_views(d[0], d[1], d[2], cams, d[3], sc["off"], d[4], d[5], sigma=0.05, prior=0.01)
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(a, b))                   # identical bits
    assert _same(d[0].cpu().numpy(), sc["pose"]) and _same(d[1].cpu().numpy(), sc["root"]) and np.array_equal(d[2].cpu().numpy(), spoiled, equal_nan=True)
    assert _same(d[3].cpu().numpy(), valid) and _same(d[4].cpu().numpy(), root_ok) and _same(d[5].cpu().numpy(), w)
    kw = dict(valid=valid, root_ok=root_ok, kp_weight=w, sigma=0.05, prior=0.01)
    clean = _tri(**ref.inputs(sc, **kw))
    assert all(_same(clean[k], getattr(a, k).cpu().numpy()) for k in KEYS)
    for t in range(3):                                                    # a take alone: the bits it has beside the others
        sl = slice(int(sc["off"][t]), int(sc["off"][t + 1]))
        alone = _tri(sc["pose"][sl], sc["root"][sl], sc["kp"][:, sl], sc["quat"][t], sc["trans"][t], sc["intr"][t], valid[:, sl], None, root_ok[sl], w[:, sl],
                     sigma=0.05, prior=0.01)
        assert all(_same(alone[k], clean[k][sl]) for k in KEYS)
    ones = _tri(**ref.inputs(sc, **dict(kw, kp_weight=np.ones_like(w))))  # kp_weight null: every weight 1
    none = _tri(**ref.inputs(sc, **dict(kw, kp_weight=None)))
    assert all(_same(ones[k], none[k]) for k in KEYS)
    missing = cams[1][:2] + [None] + cams[1][3:]                          # a None camera: the view is invalid in every frame of its take
    gone = valid.copy()
    gone[2, int(sc["off"][1]):int(sc["off"][2])] = 0
    res = triangulate_views(d[0], d[1], _dev(sc["kp"]), [cams[0], missing, cams[2]], d[3], sc["off"], d[4], d[5], sigma=0.05, prior=0.01)
    want = _tri(**ref.inputs(sc, **dict(kw, valid=gone)))
    assert all(_same(want[k], getattr(res, k).cpu().numpy()) for k in KEYS)


def test_entry_point_rejects_bad_arguments_before_any_launch(lib):
    sc = ref.scene(3, 5, [6], seed=424)
    inp = ref.inputs(sc)
    none = lambda g: (g["points"] == -1).all() and (g["err"] == -1).all() and (g["views"] == 7).all() and (g["ok"] == 7).all() and (g["steps"] == 7).all()
    for name in ("pose", "root", "kp", "off", "quat", "trans", "intr", "o_points", "o_err", "o_views", "o_ok"):
        got = _raw(lib, inp, **{name: None})
        assert got["rc"] == 1 and b"null" in lib.mp_last_error() and none(got), name
    for kw, word in ((dict(V=0), b"V=0"), (dict(V=5), b"V=5"), (dict(J=1), b"J=1"), (dict(J=33), b"J=33"), (dict(F=0), b"out of range"), (dict(F=-1), b"out of range"),
                     (dict(G=0), b"out of range"), (dict(G=7), b"out of range"), (dict(F=2 ** 36), b"too many"), (dict(distort=2), b"distort=2"),
                     (dict(sigma=0.0), b"sigma"), (dict(sigma=-1.0), b"sigma"), (dict(sigma=float("nan")), b"sigma"), (dict(prior=-1.0), b"prior"),
                     (dict(prior=INF), b"prior"), (dict(prior=float("nan")), b"prior"), (dict(iters=-1), b"iters=-1"), (dict(iters=17), b"iters=17")):
        got = _raw(lib, inp, **kw)
        assert got["rc"] == 1 and word in lib.mp_last_error() and none(got), (kw, lib.mp_last_error())
    good = _raw(lib, inp)
    assert good["rc"] == 0
    _compare("the entry point itself", good, ref.triangulate(**inp))
    nosteps = _raw(lib, inp, o_steps=None)                                # steps may be null
    assert nosteps["rc"] == 0 and (nosteps["steps"] == 7).all() and all(_same(nosteps[k], good[k]) for k in KEYS[:4])
    from manipose_amd import triangulate_views
    cams = _cameras(sc["quat"], sc["trans"], sc["intr"])
    pose, root, kp = (_dev(sc[k]) for k in ("pose", "root", "kp"))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        triangulate_views(pose.cpu(), root, kp, cams)
    with pytest.raises(RuntimeError, match="triangulate_views takes device tensors"):
        triangulate_views(pose, root, kp, cams, kp_weight=torch.ones(3, 6, 5))
    with pytest.raises(ValueError, match="lists 1 takes, take_offset 2"):
        triangulate_views(pose, root, kp, cams, take_offset=[0, 3, 6])


def test_recovery_scene_on_the_device():
    """the scenes of test_lift_triangulate_host.test_recovery_on_the_committed_seeds.  Noise-free, the device is held against the TRUTH, not against
    the statement (F at the minimum is rounding: a decision there is a coin's): the statement's bound and the float32 store's half ulp of a
    coordinate below 8 m, 2^-22, in each of three coordinates.  With noise, against the statement as well."""
    for V, steps, bound in ((4, ref.RECOVERY_STEPS_4V, ref.RECOVERY_4V), (2, ref.RECOVERY_STEPS_2V, ref.RECOVERY_2V)):
        sc = ref.recovery(V, 0.0)
        got = _tri(**ref.inputs(sc, iters=steps))
        worst = ref.errors(got["points"], sc).max()
        print(f"noise-free, {V} views, {steps} steps: max {worst:.3e} m, steps taken {np.bincount(got['steps'].ravel())}")
        assert (got["ok"] == 3).all() and np.abs(sc["truth"]).max() < 8 and worst <= bound + ref.STORE_POINT
    off = ref.recovery(4, 0.0, ref.ROOT_OFF)                              # the root 0.1 m N(0, 1) off: the same points
    got = _tri(**ref.inputs(off, iters=ref.RECOVERY_STEPS_4V))
    assert (got["ok"] == 3).all() and ref.errors(got["points"], off).max() <= ref.RECOVERY_4V + ref.STORE_POINT
    sc = ref.recovery(4, 0.002)
    got = _tri(**ref.inputs(sc))
    mean, lifted = ref.errors(got["points"], sc).mean(), ref.lifted_errors(sc).mean()
    print(f"noise 0.002, 4 views, 3 steps: mean {mean:.5f} m against the lifted pose's {lifted:.5f} m")
    assert mean < 0.25 * lifted
    _compare("recovery, noise 0.002", got, ref.triangulate(**ref.inputs(sc)))


# ---- end to end: the tiny fp32 fixture model of lift_fixtures.py -----------------------------------------------------------------------------
TRI_KEYS = ("__tri", "__tri_err", "__tri_views", "__tri_ok", "__tri_steps")


def _group(lens=(20, 20, 20, 20, 12, 12, 12), seed=51):
    """one group of 7 sequences: a take of 4 views of 20 frames, then a take of 3 views of 12 frames; S11's cameras as fetch() hands them on"""
    from manipose_amd.data.ingest import h36m_cameras
    s11 = h36m_cameras()["S11"]
    g = np.random.default_rng(seed)
    seqs = [np.clip(0.3 * g.standard_normal((n, 17, 2)), -1, 1).astype(np.float32) for n in lens]
    cams = [np.concatenate([s11[i]["intrinsic"], s11[i]["orientation"], s11[i]["translation"], np.array([i])]) for i in (0, 1, 2, 3, 0, 1, 2)]
    return {"walk": seqs}, {"walk": cams}


def _near_fused(tri, fused):
    """a joint that stayed at the prior point is the fused pose plus root: both are float32 roundings (two on the fused side: the sum, then the
    floor's offset) of the same fp64 sum"""
    return np.abs(tri.astype(np.float64) - fused.astype(np.float64)) <= 2.0 ** -22 * np.maximum(1.0, np.abs(fused))


@pytest.mark.parametrize("frame", ["camera", "world"])
def test_run_lift_with_triangulated_joints_end_to_end(tmp_path, frame):
    from _entry import lift_sequences_to_file, load_config
    model, T, K = _model("rmcl")
    groups, cams = _group()
    base = ["run.lift=true", "train.tta=false", "train.batch_size_test=2", "lift.hyps=true", "lift.fuse=true"]
    base += ["lift.frame=world", "lift.floor=true"] if frame == "world" else ["lift.fuse_cameras=estimate", "lift.fuse_bundle=3", "lift.fuse_bundle_sigma=0.5"]
    before = lift_sequences_to_file(model, load_config(base), groups, str(tmp_path / "before.npz"), cams)
    named = lift_sequences_to_file(model, load_config(base + ["lift.fuse_triangulate=false"]), groups, str(tmp_path / "off.npz"), cams)
    a, b = np.load(str(tmp_path / "before.npz")), np.load(str(tmp_path / "off.npz"))
    assert list(a.keys()) == list(b.keys()) == list(before) == list(named) and all(a[k].dtype == b[k].dtype and _same(a[k], b[k]) for k in a.keys())
    assert not any(k.endswith(TRI_KEYS) for k in before)
    on = ["lift.fuse_triangulate=true", "lift.fuse_triangulate_sigma=0.5", "lift.fuse_triangulate_prior=0.01", "lift.fuse_triangulate_steps=2"]
    got = lift_sequences_to_file(model, load_config(base + on), groups, str(tmp_path / "tri.npz"), cams)
    assert sorted(set(got) - set(before)) == sorted(f"walk.fused{t}{k}" for t in (0, 1) for k in TRI_KEYS) and set(before) <= set(got)
    assert all(_same(got[k], v) for k, v in before.items())               # every existing key keeps its bytes
    z = np.load(str(tmp_path / "tri.npz"))
    assert all(_same(z[k], got[k]) for k in got)
    for t, (n, V) in enumerate(((20, 4), (12, 3))):
        k = f"walk.fused{t}"
        tri, ok, views, steps = got[k + "__tri"], got[k + "__tri_ok"], got[k + "__tri_views"], got[k + "__tri_steps"]
        assert tri.shape == (n, 17, 3) and tri.dtype == got[k + "__tri_err"].dtype == np.float32 and got[k + "__tri_err"].shape == (n, 17)
        assert ok.dtype == views.dtype == steps.dtype == np.uint8 and ok.shape == views.shape == steps.shape == (n, 17)
        assert np.isfinite(tri).all() and (views < (1 << V)).all() and (steps <= 2).all() and (ok <= 3).all() and (got[k + "__tri_err"] >= 0).all()
        if frame == "world":                                              # (the dataset's cameras and finite keypoints: every view observes every joint)
            assert (views == (1 << V) - 1).all()
        stayed = (ok == 1) & (steps == 0)
        assert _near_fused(tri, got[k])[stayed].all() and not tri[ok == 0].any()
    plain = lift_sequences_to_file(model, load_config(base + ["lift.fuse_triangulate=true", "lift.fuse_triangulate_steps=0"]), groups, str(tmp_path / "lin.npz"), cams)
    assert all((plain[f"walk.fused{t}__tri_steps"] == 0).all() for t in (0, 1))


def test_triangulated_joints_in_synthetic_mode(lib, tmp_path, monkeypatch):
    """run.lift with lift.fuse_triangulate on synthetic data: every take has one view, so with prior = 0 every joint keeps the fused pose plus
    root; with lift.score the triangulated pose gets lift_score_tri.csv in lift_score_fused.csv's layout"""
    from _entry import run
    monkeypatch.chdir(tmp_path)
    argv = ["run.train=false", "run.test=false", "run.lift=true", "lift.stride=14", "train.batch_size_test=4", "data.seq_len=27", "model.channels=64",
            "model.layers=2", "model.nheads=4", "model.channels_seg=32", "model.layers_seg=1", "model.nheads_seg=4", "multi_hyp.n_hyp=3",
            "data.synthetic_sequences=2", "model.precision=fp32", "lift.frame=world", "lift.floor=true", "lift.fuse=true", "lift.score=true"]
    run(argv)
    out = os.path.join(str(tmp_path), "default")
    before = dict(np.load(os.path.join(out, "lift.npz")))
    fused_csv = open(os.path.join(out, "lift_score_fused.csv")).read()
    assert not os.path.exists(os.path.join(out, "lift_score_tri.csv"))
    run(argv + ["lift.fuse_triangulate=true"])
    z = np.load(os.path.join(out, "lift.npz"))
    assert set(before) <= set(z.files) and all(_same(z[k], v) for k, v in before.items())
    assert open(os.path.join(out, "lift_score_fused.csv")).read() == fused_csv
    tri_csv = open(os.path.join(out, "lift_score_tri.csv")).read().splitlines()
    assert tri_csv[0] == fused_csv.splitlines()[0] and len(tri_csv) == len(fused_csv.splitlines())
    for name in ("synthetic_000", "synthetic_001"):
        k = f"{name}.fused0"
        ok = z[k + "__ok"] != 0
        assert (z[k + "__tri_views"][ok] == 1).all() and (z[k + "__tri_steps"] == 0).all() and (z[k + "__tri_ok"][ok] == 1).all()
        assert _near_fused(z[k + "__tri"], z[k])[ok].all()

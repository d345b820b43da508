"""Fitting one skeleton to a fused take's keypoints on the device: mp_lift_fit_skeleton against the float64 statement of its rule
(lift_skeleton_ref.py), the constructed frames compared exactly, the invariants (identical bits, a take alone and beside others, inputs
untouched, unwritten frames keep their fill), argument errors, the recovery scene the feature is for, and run.lift with lift.fuse_skeleton end
to end.

The bounds against the statement, ON THE SAME float32 INPUTS: ok and steps are equal; every stored float (pose, err) is within
2^-23 max(1, |x|), the project's bound for a float32 store.  The kernel and the statement both work in fp64 with the same operations in the same
order (no contraction, IEEE division and square root), so what remains is the one rounding to float32.  That holds where every decision is away
from its threshold, which test_lift_skeleton_host.py asserts of every compared scene without a device; the bounds are not measured from the
kernel.  No frame is excluded from a comparison."""
import ctypes as C
import os
import sys
import types

import numpy as np
import pytest
import torch

import lift_rot_ref as rot
import lift_skeleton_ref as ref
from lift_fixtures import fixture_model as _model, same as _same

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hpe"))
KEYS = ("pose", "err", "ok", "steps")
INF = float("inf")


def _dev(a):
    return None if a is None else torch.from_numpy(np.array(a, order="C")).cuda()      # (a copy: a broadcast table is not writable)


def _cameras(quat, trans, intr):
    """place_views' nested list of the (G, V, .) tables"""
    G, V = quat.shape[:2]
    return [[np.concatenate([intr[g, v], quat[g, v], trans[g, v]]) for v in range(V)] for g in range(G)]


def _fit(start, kp, quat, trans, intr, lengths, parents=None, valid=None, take_offset=None, start_ok=None, kp_weight=None, distort=True, sigma=INF,
         prior=ref.DEFAULT_PRIOR, iters=ref.DEFAULT_STEPS):
    from manipose_amd import fit_skeleton_views
    G = 1 if take_offset is None else len(take_offset) - 1
    quat, trans, intr = (np.asarray(a).reshape(G, kp.shape[0], -1) for a in (quat, trans, intr))
    sk = types.SimpleNamespace(parents=list(ref.tree(kp.shape[2]) if parents is None else parents))
    res = fit_skeleton_views(_dev(start), _dev(kp), _cameras(quat, trans, intr), np.asarray(lengths), _dev(valid), take_offset, _dev(start_ok),
                             _dev(kp_weight), sk, distort, sigma, prior, iters)
    torch.cuda.synchronize()
    return {k: getattr(res, k).cpu().numpy() for k in KEYS}


def _compare(tag, got, want, rows=None):
    rows = slice(None) if rows is None else rows
    assert got["pose"].dtype == got["err"].dtype == np.float32 and got["ok"].dtype == got["steps"].dtype == np.uint8
    for k in ("ok", "steps"):
        assert np.array_equal(got[k][rows], want[k][rows]), (tag, k, np.argwhere(got[k][rows] != want[k][rows])[:5])
    worst = {k: ref.within_store(got[k][rows], want[k][rows])[1] for k in ("pose", "err")}
    print(f"[{tag}] of 2^-23 max(1, |x|): " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert all(v <= 1.0 for v in worst.values()), (tag, worst)


@pytest.mark.parametrize("n", range(len(ref.cases())))
def test_fit_matches_the_statement(n):
    tag, inp, want, _ = ref.cases()[n]
    _compare(tag, _fit(**inp), want)


def _raw(lib, inp, **over):
    """the entry point itself on an inputs dict, the outputs pre-filled: pose and err with -1, the bytes with 7"""
    V, F, J = inp["kp"].shape[:3]
    off = np.asarray(inp.get("take_offset", [0, F]), np.int64)
    G = len(off) - 1
    d = {k: _dev(np.ascontiguousarray(inp[k])) for k in ("start", "kp", "quat", "trans", "intr")}
    d["lengths"] = _dev(np.ascontiguousarray(np.broadcast_to(np.asarray(inp["lengths"], np.float32), (G, J - 1))))
    d["off"] = _dev(off)
    out = dict(pose=torch.full((F, J, 3), -1.0, device="cuda"), err=torch.full((F, 2), -1.0, device="cuda"),
               ok=torch.full((F,), 7, dtype=torch.uint8, device="cuda"), steps=torch.full((F,), 7, dtype=torch.uint8, device="cuda"))
    a = dict(start=d["start"], kp=d["kp"], V=V, F=F, J=J, off=d["off"], G=G, quat=d["quat"], trans=d["trans"], intr=d["intr"], lengths=d["lengths"],
             parents=(C.c_int32 * J)(*(inp.get("parents") or ref.tree(J))), distort=int(inp.get("distort", True)), sigma=float(inp.get("sigma", INF)),
             prior=float(inp.get("prior", ref.DEFAULT_PRIOR)), iters=int(inp.get("iters", ref.DEFAULT_STEPS)), **{"o_" + k: v for k, v in out.items()})
    a.update(over)
    p = lambda x: x.data_ptr() if torch.is_tensor(x) else x
    rc = lib.mp_lift_fit_skeleton(p(a["start"]), None, p(a["kp"]), None, a["V"], a["F"], a["J"], None, p(a["off"]), a["G"], p(a["quat"]), p(a["trans"]),
                                  p(a["intr"]), p(a["lengths"]), a["parents"], a["distort"], a["sigma"], a["prior"], a["iters"], p(a["o_pose"]),
                                  p(a["o_err"]), p(a["o_ok"]), p(a["o_steps"]), None)
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in out.items()}
    got["rc"] = rc
    return got


def test_constructed_frames_are_exact(lib):
    inp = ref.constructed()
    got, want = _fit(**inp), ref.fit(**inp)
    _compare("one rule per frame", got, want)
    assert got["ok"].tolist() == [1, 1, 0, 0, 3, 2, 3] and got["steps"][ref.NO_OBS] == 0 and got["steps"][ref.PLAIN] == 3
    for f in (ref.NAN_START, ref.NOT_OK, ref.BEHIND):
        assert not got["pose"][f].any() and not got["err"][f].any() and got["steps"][f] == 0
    rigid = ref.rigid(inp["start"], inp["lengths"][0], inp["parents"]).astype(np.float32)
    for f in (ref.NO_OBS,):                                               # no observation, prior 0: the rigid start itself, bit for bit
        assert _same(got["pose"][f], rigid[f]) and not got["err"][f].any()
    zero = _fit(**dict(inp, iters=0))                                     # iters = 0: mp_lift_rigid's rule in fp64, rounded once
    fitted = [ref.ZERO_ROOT_BONE, ref.ZERO_DEEP_BONE, ref.NO_OBS, ref.PLAIN]
    assert _same(zero["pose"][fitted], rigid[fitted]) and not zero["steps"].any()
    pulled = ref.constructed(prior=0.01)
    _compare("one rule per frame, prior 0.01", _fit(**pulled), ref.fit(**pulled))
    bad = ref.bad_lengths()
    got = _fit(**bad)
    _compare("a take whose table has a zero", got, ref.fit(**bad))
    assert not got["ok"][:3].any() and not got["pose"][:3].any() and (got["ok"][3:] == 3).all()
    sc = ref.body_scene(2, 5, [6], seed=623)                              # a frame no take holds is left unwritten
    part = ref.inputs(sc, take_offset=[1, 4])
    got, want = _raw(lib, part), ref.fit(**part)
    assert got["rc"] == 0 and want["written"].tolist() == [False, True, True, True, False, False]
    _compare("frames 1 to 3 of 6", got, want, rows=slice(1, 4))
    for f in (0, 4, 5):
        assert (got["pose"][f] == -1).all() and (got["err"][f] == -1).all() and got["ok"][f] == 7 and got["steps"][f] == 7


def test_invariants():
    from manipose_amd import fit_skeleton_views
    import lift_triangulate_ref as tri
    sc = ref.body_scene(4, 17, [1, 9, 6], seed=610)
    ftot = int(sc["off"][-1])
    valid, start_ok = tri.gap_tables(4, ftot, 615)
    w = tri.weight_table(4, ftot, 17, 612)
    spoiled = sc["kp"].copy()
    spoiled[valid == 0] = np.nan                                          # an invalid view's frame is never looked at
    cams = _cameras(sc["quat"], sc["trans"], sc["intr"])
    d = [_dev(a) for a in (sc["start"], spoiled, valid, start_ok, w)]
    call = lambda: fit_skeleton_views(d[0], d[1], cams, sc["lengths"], d[2], sc["off"], d[3], d[4], sigma=0.05, prior=0.01)
    a, b = call(), call()
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(a, b))                   # identical bits
    assert _same(d[0].cpu().numpy(), sc["start"]) and np.array_equal(d[1].cpu().numpy(), spoiled, equal_nan=True)
    assert _same(d[2].cpu().numpy(), valid) and _same(d[3].cpu().numpy(), start_ok) and _same(d[4].cpu().numpy(), w)
    assert _same(a.lengths.cpu().numpy(), sc["lengths"])
    kw = dict(valid=valid, start_ok=start_ok, kp_weight=w, sigma=0.05, prior=0.01)
    clean = _fit(**ref.inputs(sc, **kw))
    assert all(_same(clean[k], getattr(a, k).cpu().numpy()) for k in KEYS)
    for t in range(3):                                                    # a take alone: the bits it has beside the others
        sl = slice(int(sc["off"][t]), int(sc["off"][t + 1]))
        alone = _fit(sc["start"][sl], sc["kp"][:, sl], sc["quat"][t], sc["trans"][t], sc["intr"][t], sc["lengths"][t], None, valid[:, sl], None,
                     start_ok[sl], w[:, sl], sigma=0.05, prior=0.01)
        assert all(_same(alone[k], clean[k][sl]) for k in KEYS)
    ones = _fit(**ref.inputs(sc, **dict(kw, kp_weight=np.ones_like(w))))  # kp_weight null: every weight 1
    none = _fit(**ref.inputs(sc, **dict(kw, kp_weight=None)))
    assert all(_same(ones[k], none[k]) for k in KEYS)
    # lengths=None: per take and bone the median of the start's bone lengths over the start_ok frames
    res = fit_skeleton_views(d[0], _dev(sc["kp"]), cams, None, d[2], sc["off"], d[3])
    want = np.stack([ref.median_table(sc["start"][int(sc["off"][t]):int(sc["off"][t + 1])][start_ok[int(sc["off"][t]):int(sc["off"][t + 1])] != 0],
                                      sc["parents"]) for t in range(3)])
    assert np.abs(res.lengths.cpu().numpy() - want).max() <= 2.0 ** -23
    given = _fit(**ref.inputs(sc, lengths=res.lengths.cpu().numpy(), valid=valid, start_ok=start_ok))
    assert all(_same(given[k], getattr(res, k).cpu().numpy()) for k in KEYS)


def test_entry_point_rejects_bad_arguments_before_any_launch(lib):
    sc = ref.body_scene(3, 5, [6], seed=624)
    inp = ref.inputs(sc)
    none = lambda g: (g["pose"] == -1).all() and (g["err"] == -1).all() and (g["ok"] == 7).all() and (g["steps"] == 7).all()
    for name in ("start", "kp", "off", "quat", "trans", "intr", "lengths", "parents", "o_pose", "o_err", "o_ok"):
        got = _raw(lib, inp, **{name: None})
        assert got["rc"] == 1 and b"null" in lib.mp_last_error() and none(got), name
    tab = lambda *p: (C.c_int32 * 5)(*p)
    for kw, word in ((dict(V=0), b"V=0"), (dict(V=5), b"V=5"), (dict(J=1), b"J=1"), (dict(J=33), b"J=33"), (dict(F=0), b"out of range"), (dict(F=-1), b"out of range"),
                     (dict(G=0), b"out of range"), (dict(G=7), b"out of range"), (dict(F=2 ** 36), b"too many"), (dict(distort=2), b"distort=2"),
                     (dict(sigma=0.0), b"sigma"), (dict(sigma=-1.0), b"sigma"), (dict(sigma=float("nan")), b"sigma"), (dict(prior=-1.0), b"prior"),
                     (dict(prior=INF), b"prior"), (dict(prior=float("nan")), b"prior"), (dict(iters=-1), b"iters=-1"), (dict(iters=17), b"iters=17"),
                     (dict(parents=tab(0, 0, 1, 2, 0)), b"parents[0]"), (dict(parents=tab(-1, 0, 2, 2, 0)), b"parents[2]"),
                     (dict(parents=tab(-1, 0, 1, -1, 0)), b"parents[3]")):
        got = _raw(lib, inp, **kw)
        assert got["rc"] == 1 and word in lib.mp_last_error() and none(got), (kw, lib.mp_last_error())
    good = _raw(lib, inp)
    assert good["rc"] == 0
    _compare("the entry point itself", good, ref.fit(**inp))
    nosteps = _raw(lib, inp, o_steps=None)                                # steps may be null
    assert nosteps["rc"] == 0 and (nosteps["steps"] == 7).all() and all(_same(nosteps[k], good[k]) for k in KEYS[:3])
    from manipose_amd import fit_skeleton_views
    cams = _cameras(sc["quat"], sc["trans"], sc["intr"])
    start, kp = _dev(sc["start"]), _dev(sc["kp"])
    sk = types.SimpleNamespace(parents=list(sc["parents"]))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fit_skeleton_views(start.cpu(), kp, cams, sc["lengths"], skeleton=sk)
    with pytest.raises(RuntimeError, match="fit_skeleton_views takes device tensors"):
        fit_skeleton_views(start, kp, cams, sc["lengths"], kp_weight=torch.ones(3, 6, 5), skeleton=sk)
    with pytest.raises(ValueError, match="lists 1 takes, take_offset 2"):
        fit_skeleton_views(start, kp, cams, take_offset=[0, 3, 6], skeleton=sk)


def test_recovery_scene_on_the_device():
    """the scenes of test_lift_skeleton_host.test_recovery_on_the_committed_seed, against the statement and against the truth"""
    sc = ref.recovery(4, 0.0)
    got = _fit(**ref.inputs(sc))
    worst = ref.errors(got["pose"], sc).max()
    print(f"noise-free, 4 views, {ref.DEFAULT_STEPS} steps: max {worst:.3e} m, steps taken {np.bincount(got['steps'])}")
    assert (got["ok"] == 3).all() and worst <= ref.RECOVERY_4V + ref.STORE_POINT
    sc = ref.recovery(4, 0.002)
    start = ref.triangulated_start(sc)
    inp = ref.inputs(sc, start=start)
    got = _fit(**inp)
    mean, before = ref.errors(got["pose"], sc).mean(), ref.errors(start, sc).mean()
    again = ref.errors(ref.rigid(start, sc["lengths"][0], sc["parents"]), sc).mean()
    print(f"noise 0.002, 4 views: the fit {mean:.5f} m, the triangulated start {before:.5f} m, re-assembled bone by bone {again:.5f} m")
    assert mean < before and mean < again
    _compare("recovery, noise 0.002", got, ref.fit(**inp))
    bones = ref.bone_lengths(got["pose"], sc["parents"])
    # two float32 stores of coordinates below 8 m (half an ulp, 2^-22, each), three coordinates: sqrt(3) 2^-21, the host test's bound
    assert np.abs(got["pose"]).max() < 8 and np.abs(bones - sc["lengths"][0].astype(np.float64)).max() <= np.sqrt(3.0) * 2.0 ** -21


# ---- end to end: the tiny fp32 fixture model of lift_fixtures.py -----------------------------------------------------------------------------
SKEL_KEYS = ("__skel", "__skel_bones", "__skel_err", "__skel_ok", "__skel_steps", "__skel_quat", "__skel_quat_ok")


def _group(lens=(20, 20, 20, 20, 12, 12, 12), seed=51):
    """one group of 7 sequences: a take of 4 views of 20 frames, then a take of 3 views of 12 frames; S11's cameras as fetch() hands them on"""
    from manipose_amd.data.ingest import h36m_cameras
    s11 = h36m_cameras()["S11"]
    g = np.random.default_rng(seed)
    seqs = [np.clip(0.3 * g.standard_normal((n, 17, 2)), -1, 1).astype(np.float32) for n in lens]
    cams = [np.concatenate([s11[i]["intrinsic"], s11[i]["orientation"], s11[i]["translation"], np.array([i])]) for i in (0, 1, 2, 3, 0, 1, 2)]
    return {"walk": seqs}, {"walk": cams}


def _check_take(z, k, n):
    """the skeleton keys of one fused take: shapes, dtypes, constant bones, and fk(quat, bones) + root reproducing the pose; returns the frames
    with a result (a take none of whose frames could be started from has none, and with the measured table NaN bones: nothing to take a median of)"""
    skel, bones, ok = z[k + "__skel"], z[k + "__skel_bones"], z[k + "__skel_ok"]
    assert skel.shape == (n, 17, 3) and skel.dtype == bones.dtype == z[k + "__skel_err"].dtype == np.float32 and bones.shape == (16,)
    assert z[k + "__skel_err"].shape == (n, 2) and ok.shape == z[k + "__skel_steps"].shape == (n,) and ok.dtype == z[k + "__skel_steps"].dtype == np.uint8
    assert z[k + "__skel_quat"].shape == (n, 17, 4) and z[k + "__skel_quat"].dtype == np.float32 and z[k + "__skel_quat_ok"].dtype == np.uint8
    assert np.isfinite(skel).all() and (ok <= 3).all() and not skel[(ok & 1) == 0].any() and not z[k + "__skel_err"][(ok & 1) == 0].any()
    done = (ok & 1) != 0
    if not done.any():
        assert np.isnan(bones).all() or (bones > 0).all()
        return done
    assert (bones > 0).all()
    scale = max(1.0, float(np.abs(skel).max()))
    got = ref.bone_lengths(skel[done], ref.H36M_PARENTS)
    assert np.abs(got - bones.astype(np.float64)).max() <= 8 * 2.0 ** -23 * scale     # float32 stores of two joints (and of the floor's offset), three coordinates
    qok = z[k + "__skel_quat_ok"][done] != 0
    back = rot.fk_quat(z[k + "__skel_quat"][done][qok], bones.astype(np.float64), rot.H36M_PARENTS, rot.H36M_REST, skel[done][qok][:, 0].astype(np.float64))
    assert qok.any() and np.abs(back - skel[done][qok]).max() <= ROT_TOL
    return done


ROT_TOL = 1e-5               # test_gpu_lift_rot.py's bound for "(root, quat, bones) is the sequence": fk(quat, bones) + root against the emitted pose


@pytest.mark.parametrize("frame", ["camera", "world"])
def test_run_lift_with_a_fitted_skeleton_end_to_end(tmp_path, frame):
    from _entry import lift_sequences_to_file, load_config
    model, T, K = _model("rmcl")
    groups, cams = _group()
    base = ["run.lift=true", "train.tta=false", "train.batch_size_test=2", "lift.hyps=true", "lift.fuse=true", "lift.fuse_triangulate=true", "lift.rotations=true"]
    # world: the dataset's cameras, the bone table measured from the start; camera: estimated and bundle-adjusted cameras, lift.rigid's bone table
    base += ["lift.frame=world", "lift.floor=true"] if frame == "world" else ["lift.fuse_cameras=estimate", "lift.fuse_bundle=3", "lift.fuse_bundle_sigma=0.5", "lift.rigid=true"]
    before = lift_sequences_to_file(model, load_config(base), groups, str(tmp_path / "before.npz"), cams)
    named = lift_sequences_to_file(model, load_config(base + ["lift.fuse_skeleton=false"]), groups, str(tmp_path / "off.npz"), cams)
    assert list(before) == list(named) and all(_same(before[k], named[k]) for k in before) and not any(k.endswith(SKEL_KEYS) for k in before)
    got = lift_sequences_to_file(model, load_config(base + ["lift.fuse_skeleton=true", "lift.fuse_skeleton_sigma=0.5"]), groups, str(tmp_path / "skel.npz"), cams)
    assert sorted(set(got) - set(before)) == sorted(f"walk.fused{t}{k}" for t in (0, 1) for k in SKEL_KEYS) and set(before) <= set(got)
    assert all(_same(got[k], v) for k, v in before.items())               # every existing key keeps its bytes
    z = np.load(str(tmp_path / "skel.npz"))
    assert all(_same(z[k], got[k]) for k in got)
    for t, n in enumerate((20, 12)):
        done = _check_take(got, f"walk.fused{t}", n)
        print(f"[{frame}] take {t}: {int(done.sum())} of {n} frames fitted, steps {np.bincount(got[f'walk.fused{t}__skel_steps'])}")
        if frame == "world":
            assert done.any()
        else:                                                             # the table is the mean of the views' lift.rigid tables
            want = np.mean([got[f"walk.{i}__bones"] for i in got[f"walk.fused{t}__views"]], axis=0)
            assert np.abs(got[f"walk.fused{t}__skel_bones"] - want).max() <= 2.0 ** -23
    plain = lift_sequences_to_file(model, load_config(base + ["lift.fuse_skeleton=true", "lift.fuse_skeleton_steps=0"]), groups, str(tmp_path / "rigid.npz"), cams)
    assert all((plain[f"walk.fused{t}__skel_steps"] == 0).all() for t in (0, 1))


def test_fitted_skeleton_in_synthetic_mode(lib, tmp_path, monkeypatch):
    """run.lift with lift.fuse_skeleton on synthetic data: every take has one view; with lift.score the fitted pose gets lift_score_skel.csv in
    lift_score_fused.csv's layout"""
    from _entry import run
    monkeypatch.chdir(tmp_path)
    argv = ["run.train=false", "run.test=false", "run.lift=true", "lift.stride=14", "train.batch_size_test=4", "data.seq_len=27", "model.channels=64",
            "model.layers=2", "model.nheads=4", "model.channels_seg=32", "model.layers_seg=1", "model.nheads_seg=4", "multi_hyp.n_hyp=3",
            "data.synthetic_sequences=2", "model.precision=fp32", "lift.frame=world", "lift.floor=true", "lift.fuse=true", "lift.score=true",
            "lift.fuse_triangulate=true", "lift.rotations=true"]
    run(argv)
    out = os.path.join(str(tmp_path), "default")
    before = dict(np.load(os.path.join(out, "lift.npz")))
    fused_csv = open(os.path.join(out, "lift_score_fused.csv")).read()
    assert not os.path.exists(os.path.join(out, "lift_score_skel.csv"))
    run(argv + ["lift.fuse_skeleton=true"])
    z = np.load(os.path.join(out, "lift.npz"))
    assert set(before) <= set(z.files) and all(_same(z[k], v) for k, v in before.items())
    assert open(os.path.join(out, "lift_score_fused.csv")).read() == fused_csv
    skel_csv = open(os.path.join(out, "lift_score_skel.csv")).read().splitlines()
    assert skel_csv[0] == fused_csv.splitlines()[0] and len(skel_csv) == len(fused_csv.splitlines())
    for name in ("synthetic_000", "synthetic_001"):
        k = f"{name}.fused0"
        done = _check_take(z, k, z[k].shape[0])
        assert np.array_equal(done, z[k + "__ok"] != 0)

"""Fitting a fused take's skeleton along time on the device: mp_lift_fit_skeleton_smooth against the float64 statement of its rule
(lift_skeleton_smooth_ref.py), smooth = 0 against mp_lift_fit_skeleton on the same buffers, the invariants (identical bits, a take alone and
beside others, inputs untouched, unwritten frames keep their fill), argument errors, the recovery scene the feature is for, and run.lift with
lift.fuse_skeleton_smooth end to end.

The bounds against the statement, ON THE SAME float32 INPUTS: ok, steps and moves are equal; every stored float (pose, err) is within
2^-23 max(1, |x|), the project's bound for a float32 store.  The kernel and the statement both work in fp64 with the same operations in the same
order (no contraction, IEEE division and square root) and the state never leaves fp64 between the visits, so what remains is the one rounding
to float32.  That holds where every decision is away from its threshold, which test_lift_skeleton_smooth_host.py asserts of every compared
scene without a device; the bounds are not measured from the kernel.  No frame is excluded from a comparison."""
import ctypes as C
import os
import sys
import types

import numpy as np
import pytest
import torch

import lift_skeleton_ref as base
import lift_skeleton_smooth_ref as ref
from lift_fixtures import fixture_model as _model, same as _same

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hpe"))
KEYS = ("pose", "err", "ok", "steps", "moves")
INF = float("inf")


def _dev(a):
    return None if a is None else torch.from_numpy(np.array(a, order="C")).cuda()


def _cameras(quat, trans, intr):
    G, V = quat.shape[:2]
    return [[np.concatenate([intr[g, v], quat[g, v], trans[g, v]]) for v in range(V)] for g in range(G)]


def _fit(start, kp, quat, trans, intr, lengths, parents=None, valid=None, take_offset=None, start_ok=None, kp_weight=None, distort=True, sigma=INF,
         prior=base.DEFAULT_PRIOR, iters=base.DEFAULT_STEPS, smooth=ref.DEFAULT_SMOOTH, sweeps=ref.DEFAULT_SWEEPS):
    """fit_skeleton_views; with smooth = 0 it returns mp_lift_fit_skeleton's four outputs, which the statement's smooth = 0 result extends by
    err[:, 2] = err[:, 1] and moves = 0"""
    from manipose_amd import fit_skeleton_views
    G = 1 if take_offset is None else len(take_offset) - 1
    quat, trans, intr = (np.asarray(a).reshape(G, kp.shape[0], -1) for a in (quat, trans, intr))
    sk = types.SimpleNamespace(parents=list(base.tree(kp.shape[2]) if parents is None else parents))
    res = fit_skeleton_views(_dev(start), _dev(kp), _cameras(quat, trans, intr), np.asarray(lengths), _dev(valid), take_offset, _dev(start_ok),
                             _dev(kp_weight), sk, distort, sigma, prior, iters, smooth, sweeps)
    torch.cuda.synchronize()
    got = {k: getattr(res, k).cpu().numpy() for k in KEYS if hasattr(res, k)}
    if "moves" not in got:
        got["err"] = np.concatenate([got["err"], got["err"][:, 1:]], axis=1)
        got["moves"] = np.zeros_like(got["steps"])
    return got


WORST = {"pose": 0.0, "err": 0.0}


def _compare(tag, got, want, rows=None):
    rows = slice(None) if rows is None else rows
    assert got["pose"].dtype == got["err"].dtype == np.float32 and got["ok"].dtype == got["steps"].dtype == got["moves"].dtype == np.uint8
    assert got["err"].shape[1] == 3
    for k in ("ok", "steps", "moves"):
        assert np.array_equal(got[k][rows], want[k][rows]), (tag, k, np.argwhere(got[k][rows] != want[k][rows])[:5])
    worst = {k: ref.within_store(got[k][rows], want[k][rows])[1] for k in ("pose", "err")}
    for k, v in worst.items():
        WORST[k] = max(WORST[k], v)
    print(f"[{tag}] of 2^-23 max(1, |x|): " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()) + f"; moves {np.bincount(got['moves'][rows])}; "
          f"the largest so far: pose {WORST['pose']:.3f}, err {WORST['err']:.3f}")
    assert all(v <= 1.0 for v in worst.values()), (tag, worst)


@pytest.mark.parametrize("n", range(len(ref.cases())))
def test_fit_matches_the_statement(n):
    tag, inp, want, _ = ref.cases()[n]
    _compare(tag, _fit(**inp), want)


def _raw(lib, inp, plain=False, **over):
    """the entry point itself on an inputs dict, the outputs pre-filled: pose and err with -1, the bytes with 7; plain: mp_lift_fit_skeleton on
    uploads of the same inputs, with its (F, 2) err"""
    V, F, J = inp["kp"].shape[:3]
    off = np.asarray(inp.get("take_offset", [0, F]), np.int64)
    G = len(off) - 1
    d = {k: _dev(np.ascontiguousarray(inp[k])) for k in ("start", "kp", "quat", "trans", "intr")}
    d["lengths"] = _dev(np.ascontiguousarray(np.broadcast_to(np.asarray(inp["lengths"], np.float32), (G, J - 1))))
    d["off"] = _dev(off)
    out = dict(pose=torch.full((F, J, 3), -1.0, device="cuda"), err=torch.full((F, 2 if plain else 3), -1.0, device="cuda"),
               **{k: torch.full((F,), 7, dtype=torch.uint8, device="cuda") for k in ("ok", "steps", "moves")})
    need = int(lib.mp_lift_fit_skeleton_smooth_scratch_bytes(F, J))
    scratch = torch.full((max(need // 8, 1) + 1,), float("nan"), dtype=torch.float64, device="cuda")
    a = dict(start=d["start"], start_ok=_dev(inp.get("start_ok")), kp=d["kp"], kp_weight=_dev(inp.get("kp_weight")), V=V, F=F, J=J, valid=_dev(inp.get("valid")),
             off=d["off"], G=G, quat=d["quat"], trans=d["trans"], intr=d["intr"], lengths=d["lengths"], parents=(C.c_int32 * J)(*(inp.get("parents") or base.tree(J))),
             distort=int(inp.get("distort", True)), sigma=float(inp.get("sigma", INF)), prior=float(inp.get("prior", base.DEFAULT_PRIOR)),
             iters=int(inp.get("iters", base.DEFAULT_STEPS)), smooth=float(inp.get("smooth", ref.DEFAULT_SMOOTH)), sweeps=int(inp.get("sweeps", ref.DEFAULT_SWEEPS)),
             scratch=scratch.data_ptr(), scratch_bytes=need, **{"o_" + k: v for k, v in out.items()})
    a.update(over)
    p = lambda x: x.data_ptr() if torch.is_tensor(x) else x
    head = [p(a[k]) for k in ("start", "start_ok", "kp", "kp_weight", "V", "F", "J", "valid", "off", "G", "quat", "trans", "intr", "lengths", "parents", "distort",
                              "sigma", "prior", "iters")]
    if plain:
        rc = lib.mp_lift_fit_skeleton(*head, p(a["o_pose"]), p(a["o_err"]), p(a["o_ok"]), p(a["o_steps"]), None)
    else:
        rc = lib.mp_lift_fit_skeleton_smooth(*head, a["smooth"], a["sweeps"], p(a["o_pose"]), p(a["o_err"]), p(a["o_ok"]), p(a["o_steps"]), p(a["o_moves"]),
                                             a["scratch"], a["scratch_bytes"], None)
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in out.items()}
    got["rc"] = rc
    got["inputs"] = {k: v.cpu().numpy() for k, v in d.items()}
    return got


def test_smooth_zero_and_sweeps_zero_are_the_per_frame_fit_bit_for_bit(lib):
    for tag, inp, want, _ in ref.cases():
        if not ("three takes" in tag or tag.startswith("F=65")):
            continue
        plain = _raw(lib, inp, plain=True)
        assert plain["rc"] == 0
        for over in (dict(smooth=0.0), dict(sweeps=0)):
            got = _raw(lib, inp, **over)
            assert got["rc"] == 0, tag
            assert all(_same(got[k], plain[k]) for k in ("pose", "ok", "steps")) and _same(got["err"][:, :2], plain["err"]), (tag, over)
            assert _same(got["err"][:, 2], got["err"][:, 1]) and not got["moves"].any()
        if inp.get("smooth", ref.DEFAULT_SMOOTH) > 0 and inp.get("sweeps", ref.DEFAULT_SWEEPS) > 0:        # stage A's outputs stay with the sweeps on
            got = _raw(lib, inp)
            assert all(_same(got[k], plain[k]) for k in ("ok", "steps")) and _same(got["err"][:, :2], plain["err"]), tag
            assert got["moves"].any() and not _same(got["pose"], plain["pose"])


def test_invariants(lib):
    tag, inp, want, _ = next(c for c in ref.cases() if "weights with zeros" in c[0])
    spoiled = inp["kp"].copy()
    a, b = _raw(lib, dict(inp, kp=spoiled)), _raw(lib, dict(inp, kp=spoiled))
    assert a["rc"] == b["rc"] == 0 and all(_same(a[k], b[k]) for k in KEYS)                                  # identical bits
    _compare(tag + ", the entry point itself", a, want)
    for k, v in a["inputs"].items():                                      # inputs untouched
        src = np.broadcast_to(np.asarray(inp["lengths"], np.float32), v.shape) if k == "lengths" else np.asarray(inp["take_offset"], np.int64) if k == "off" else inp[k]
        assert np.array_equal(v, np.asarray(src).reshape(v.shape), equal_nan=True), k
    nomoves = _raw(lib, inp, o_moves=None, o_steps=None)                  # steps and moves may be null
    assert nomoves["rc"] == 0 and (nomoves["moves"] == 7).all() and (nomoves["steps"] == 7).all() and all(_same(nomoves[k], a[k]) for k in KEYS[:3])
    off = [int(v) for v in inp["take_offset"]]
    for t in range(len(off) - 1):                                         # a take alone: the bits it has beside the others
        sl = slice(off[t], off[t + 1])
        alone = _fit(inp["start"][sl], inp["kp"][:, sl], inp["quat"][t], inp["trans"][t], inp["intr"][t], inp["lengths"][t], inp["parents"], None, None,
                     inp["start_ok"][sl], inp["kp_weight"][:, sl], sigma=inp["sigma"], sweeps=inp["sweeps"])
        assert all(_same(alone[k], a[k][sl]) for k in KEYS), t
    sc = ref.motion_scene(2, 5, [9], seed=823)                            # a frame no take holds is left unwritten, and no term reaches across it
    part = ref.inputs(sc, take_offset=[1, 8], sweeps=2)
    got, full = _raw(lib, part), ref.fit(**part)
    assert got["rc"] == 0 and full["written"].tolist() == [False] + [True] * 7 + [False]
    _compare("frames 1 to 7 of 9", got, full, rows=slice(1, 8))
    for f in (0, 8):
        assert (got["pose"][f] == -1).all() and (got["err"][f] == -1).all() and got["ok"][f] == got["steps"][f] == got["moves"][f] == 7
    inner = ref.fit(**ref.inputs(dict(sc, start=sc["start"][1:8], kp=sc["kp"][:, 1:8]), take_offset=[0, 7], sweeps=2))
    assert all(np.array_equal(inner[k], full[k][1:8]) for k in KEYS)


def test_entry_point_rejects_bad_arguments_before_any_launch(lib):
    sc = ref.motion_scene(3, 5, [6], seed=824)
    inp = ref.inputs(sc, sweeps=2)
    none = lambda g: (g["pose"] == -1).all() and (g["err"] == -1).all() and all((g[k] == 7).all() for k in ("ok", "steps", "moves"))
    for name in ("start", "kp", "off", "quat", "trans", "intr", "lengths", "parents", "o_pose", "o_err", "o_ok"):
        got = _raw(lib, inp, **{name: None})
        assert got["rc"] == 1 and b"null" in lib.mp_last_error() and none(got), name
    tab = lambda *p: (C.c_int32 * 5)(*p)
    need = int(lib.mp_lift_fit_skeleton_smooth_scratch_bytes(6, 5))
    assert need == 6 * 6 * 5 * 8 and lib.mp_lift_fit_skeleton_smooth_scratch_bytes(0, 5) == 0 and lib.mp_lift_fit_skeleton_smooth_scratch_bytes(6, 33) == 0
    odd = torch.zeros(need // 8 + 2, dtype=torch.float64, device="cuda")
    for kw, word in ((dict(V=0), b"V=0"), (dict(V=5), b"V=5"), (dict(J=1), b"J=1"), (dict(J=33), b"J=33"), (dict(F=0), b"out of range"), (dict(F=-1), b"out of range"),
                     (dict(G=0), b"out of range"), (dict(G=7), b"out of range"), (dict(F=2 ** 36), b"too many"), (dict(distort=2), b"distort=2"),
                     (dict(sigma=0.0), b"sigma"), (dict(sigma=float("nan")), b"sigma"), (dict(prior=-1.0), b"prior"), (dict(prior=INF), b"prior"),
                     (dict(iters=-1), b"iters=-1"), (dict(iters=17), b"iters=17"), (dict(parents=tab(-1, 0, 2, 2, 0)), b"parents[2]"),
                     (dict(smooth=-0.1), b"smooth"), (dict(smooth=INF), b"smooth"), (dict(smooth=float("nan")), b"smooth"),
                     (dict(sweeps=-1), b"sweeps=-1"), (dict(sweeps=65), b"sweeps=65"),
                     (dict(scratch=None), b"scratch"), (dict(scratch=odd.data_ptr() + 4), b"scratch"), (dict(scratch_bytes=need - 8), b"scratch")):
        got = _raw(lib, inp, **kw)
        assert got["rc"] == 1 and word in lib.mp_last_error() and b"mp_lift_fit_skeleton_smooth" in lib.mp_last_error() and none(got), (kw, lib.mp_last_error())
    good = _raw(lib, inp)
    assert good["rc"] == 0
    _compare("the entry point itself", good, ref.fit(**inp))
    most = _raw(lib, inp, sweeps=64, scratch_bytes=need)                  # the largest sweep count, the smallest scratch
    assert most["rc"] == 0
    from manipose_amd import fit_skeleton_views
    cams = _cameras(sc["quat"], sc["trans"], sc["intr"])
    sk = types.SimpleNamespace(parents=list(sc["parents"]))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fit_skeleton_views(_dev(sc["start"]).cpu(), _dev(sc["kp"]), cams, sc["lengths"], skeleton=sk, smooth=0.1)


def test_recovery_scene_on_the_device():
    """the 4-view scene of test_lift_skeleton_smooth_host.test_recovery_on_the_committed_seed, against the statement and against the truth"""
    sc, inp = ref.recovery(4), ref.recovery_inputs(4)
    got, plain = _fit(**inp), _fit(**dict(inp, smooth=0.0))
    _compare("recovery, 4 views", got, ref.fit(**inp))
    mean, before = ref.errors(got["pose"], sc).mean(), ref.errors(plain["pose"], sc).mean()
    sd, sd_before = ref.second_difference(got["pose"]), ref.second_difference(plain["pose"])
    print(f"4 views, noise 0.002: the smoothed fit {mean:.5f} m against the per-frame fit's {before:.5f} m; second difference {sd:.5f} against {sd_before:.5f} m / frame^2")
    assert mean < before and sd < sd_before
    bones = base.bone_lengths(got["pose"], sc["parents"])
    assert np.abs(got["pose"]).max() < 8 and np.abs(bones - sc["lengths"][0].astype(np.float64)).max() <= np.sqrt(3.0) * 2.0 ** -21


# ---- end to end: the tiny fp32 fixture model of lift_fixtures.py -----------------------------------------------------------------------------
def test_run_lift_with_a_smoothed_skeleton_end_to_end(tmp_path):
    from _entry import lift_sequences_to_file, load_config
    from manipose_amd.data.ingest import h36m_cameras
    model, T, K = _model("rmcl")
    s11 = h36m_cameras()["S11"]
    g = np.random.default_rng(51)
    groups = {"walk": [np.clip(0.3 * g.standard_normal((n, 17, 2)), -1, 1).astype(np.float32) for n in (20, 20, 20, 20, 12, 12, 12)]}
    cams = {"walk": [np.concatenate([s11[i]["intrinsic"], s11[i]["orientation"], s11[i]["translation"], np.array([i])]) for i in (0, 1, 2, 3, 0, 1, 2)]}
    base_cfg = ["run.lift=true", "train.tta=false", "train.batch_size_test=2", "lift.hyps=true", "lift.fuse=true", "lift.fuse_triangulate=true", "lift.rotations=true",
                "lift.frame=world", "lift.floor=true", "lift.fuse_skeleton=true", "lift.fuse_skeleton_sigma=0.5"]
    before = lift_sequences_to_file(model, load_config(base_cfg), groups, str(tmp_path / "before.npz"), cams)
    named = lift_sequences_to_file(model, load_config(base_cfg + ["lift.fuse_skeleton_smooth=0.0", "lift.fuse_skeleton_sweeps=8"]), groups, str(tmp_path / "off.npz"), cams)
    assert list(before) == list(named) and all(_same(before[k], named[k]) for k in before)
    assert not any(k.endswith(("__skel_err_smooth", "__skel_moves")) for k in before)
    got = lift_sequences_to_file(model, load_config(base_cfg + ["lift.fuse_skeleton_smooth=0.1"]), groups, str(tmp_path / "smooth.npz"), cams)
    assert sorted(set(got) - set(before)) == sorted(f"walk.fused{t}{k}" for t in (0, 1) for k in ("__skel_err_smooth", "__skel_moves"))
    changed = {k for k in before if not _same(got[k], before[k])}
    assert changed and all(k.endswith(("__skel", "__skel_quat", "__skel_quat_ok")) for k in changed), changed       # nothing else changes
    for t, n in enumerate((20, 12)):
        k = f"walk.fused{t}"
        assert got[k + "__skel_err"].shape == (n, 2) and got[k + "__skel_err_smooth"].shape == (n,) and got[k + "__skel_err_smooth"].dtype == np.float32
        assert got[k + "__skel_moves"].shape == (n,) and got[k + "__skel_moves"].dtype == np.uint8 and got[k + "__skel_moves"].max() <= 8
        done = (got[k + "__skel_ok"] & 1) != 0
        print(f"take {t}: {int(done.sum())} of {n} frames fitted, moves {np.bincount(got[k + '__skel_moves'])}")
        assert done.any() and got[k + "__skel_moves"].any() and not _same(got[k + "__skel"], before[k + "__skel"])
        scale = max(1.0, float(np.abs(got[k + "__skel"]).max()))
        bones = base.bone_lengths(got[k + "__skel"][done], base.H36M_PARENTS)
        assert np.abs(bones - got[k + "__skel_bones"].astype(np.float64)).max() <= 8 * 2.0 ** -23 * scale       # test_gpu_lift_skeleton.py's bound
        assert not got[k + "__skel"][~done].any() and not got[k + "__skel_moves"][~done].any()


def test_smoothed_skeleton_in_synthetic_mode(lib, tmp_path, monkeypatch):
    """run.lift with lift.fuse_skeleton_smooth on synthetic data: every take has one view; lift_score_skel.csv is the smoothed fit's"""
    from _entry import run
    monkeypatch.chdir(tmp_path)
    argv = ["run.train=false", "run.test=false", "run.lift=true", "lift.stride=14", "train.batch_size_test=4", "data.seq_len=27", "model.channels=64",
            "model.layers=2", "model.nheads=4", "model.channels_seg=32", "model.layers_seg=1", "model.nheads_seg=4", "multi_hyp.n_hyp=3",
            "data.synthetic_sequences=2", "model.precision=fp32", "lift.frame=world", "lift.floor=true", "lift.fuse=true", "lift.score=true",
            "lift.fuse_triangulate=true", "lift.rotations=true", "lift.fuse_skeleton=true"]
    run(argv)
    out = os.path.join(str(tmp_path), "default")
    before = dict(np.load(os.path.join(out, "lift.npz")))
    csv = open(os.path.join(out, "lift_score_skel.csv")).read()
    run(argv + ["lift.fuse_skeleton_smooth=0.1", "lift.fuse_skeleton_sweeps=4"])
    z = dict(np.load(os.path.join(out, "lift.npz")))
    assert set(before) < set(z) and all(k.endswith(("__skel_err_smooth", "__skel_moves")) for k in set(z) - set(before))
    after = open(os.path.join(out, "lift_score_skel.csv")).read()
    assert after.splitlines()[0] == csv.splitlines()[0] and len(after.splitlines()) == len(csv.splitlines()) and after != csv
    for name in ("synthetic_000", "synthetic_001"):
        k = f"{name}.fused0"
        n = z[k].shape[0]
        assert z[k + "__skel_err"].shape == (n, 2) and z[k + "__skel_err_smooth"].shape == (n,) and z[k + "__skel_moves"].shape == (n,)
        assert z[k + "__skel_moves"].max() <= 4 and z[k + "__skel_moves"].any() and not _same(z[k + "__skel"], before[k + "__skel"])
        done = (z[k + "__skel_ok"] & 1) != 0
        bones = base.bone_lengths(z[k + "__skel"][done], base.H36M_PARENTS)
        assert np.abs(bones - z[k + "__skel_bones"].astype(np.float64)).max() <= 8 * 2.0 ** -23 * max(1.0, float(np.abs(z[k + "__skel"]).max()))
        assert all(_same(z[q], v) for q, v in before.items() if q.startswith(k) and not q.endswith(("__skel", "__skel_quat", "__skel_quat_ok")))

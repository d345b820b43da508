"""Calibrating a take on its keypoints on the device: mp_lift_calibrate_views against the float64 statement of its rule (lift_calibrate_ref.py),
the invariants (identical bits, a take alone and beside others, inputs untouched), argument errors, and the recovery scene the feature is for.

The bounds against the statement, ON THE SAME float32 INPUTS: steps, ok and used are equal; cost within 1e-9 relative; every stored float (quat,
trans, intr, points, reproj) within 2^-23 max(1, |x|), the project's bound for a float32 store.  The kernel and the statement both work in fp64
and differ in nothing but the library's sine and cosine: relative 1e-16, amplified by the reduced system's condition number, which
test_lift_calibrate_host.py holds at or below 1e8 in every compared scene (with every decision away from its threshold) without a device - far
below the one rounding to float32 that remains.  The bounds are not measured from the kernel.  Measured on an MI355X (synthetic scenes; nothing
here is measured on real data): the worst stored float is 0.497 of its bound (a point; quat 0.248, trans 0.434, intr 0.469, reproj 0.061), the
one rounding and nothing else, and every cost has the statement's bits."""
import numpy as np
import pytest
import torch

import lift_calibrate_ref as ref
from lift_fixtures import same as _same

pytestmark = pytest.mark.gpu

KEYS = ("quat", "trans", "intr", "points", "reproj", "cost", "steps", "ok", "used")


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _cameras(quat, trans, intr):
    G, V = quat.shape[:2]
    return [[np.concatenate([intr[g, v], quat[g, v], trans[g, v]]) for v in range(V)] for g in range(G)]


def _calibrate(start, kp, quat, trans, intr, valid=None, take_offset=None, start_ok=None, fixed=None, weights=None, distort=True, focal=True,
               sigma=ref.SIGMA, prior=ref.PRIOR, iters=3):
    from manipose_amd import calibrate_views
    G = 1 if take_offset is None else len(take_offset) - 1
    quat, trans, intr = (np.asarray(a).reshape(G, kp.shape[0], -1) for a in (quat, trans, intr))
    res = calibrate_views(_dev(start), _dev(kp), _cameras(quat, trans, intr), _dev(valid), take_offset, _dev(start_ok), fixed, weights, distort, focal,
                          sigma, prior, iters)
    torch.cuda.synchronize()
    got = {k: r.cpu().numpy() for k, r in zip(KEYS, res[1:])}
    for g, take in enumerate(res.cameras):                                # the nested cameras are the tables, to be passed on
        for v, cam in enumerate(take):
            assert _same(cam[:9], got["intr"][g, v]) and _same(cam[9:13], got["quat"][g, v]) and _same(cam[13:], got["trans"][g, v])
    return got


def _compare(tag, got, want):
    assert got["used"].dtype == np.int32 and got["ok"].dtype == got["steps"].dtype == np.uint8 and got["cost"].dtype == np.float64
    for k in ("steps", "ok", "used"):
        assert np.array_equal(got[k], want[k]), (tag, k, got[k], want[k])
    dc = np.abs(got["cost"] - want["cost"]) / np.maximum(np.abs(want["cost"]), 1e-300)
    worst = {}
    for k in ("quat", "trans", "intr", "points", "reproj"):
        assert got[k].dtype == np.float32
        _, worst[k] = ref.within_store(got[k], want[k])
    print(f"[{tag}] cost off by {dc.max():.2e} relative; of 2^-23 max(1, |x|): " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert (dc <= ref.COST_TOL).all(), (tag, dc)
    assert all(v <= 1.0 for v in worst.values()), (tag, worst)


@pytest.mark.parametrize("n", range(len(ref.cases())))
def test_calibrate_matches_the_statement(n):
    tag, inp, want, _ = ref.cases()[n]
    got = _calibrate(**inp)
    _compare(tag, got, want)
    for g in range(len(want["steps"])):                                   # what took no step is copied through bit for bit
        if want["steps"][g] == 0:
            sl = slice(int(inp["take_offset"][g]), int(inp["take_offset"][g + 1]))
            assert all(_same(got[k][g], inp[k][g]) for k in ("quat", "trans", "intr")) and _same(got["points"][sl], inp["start"][sl]), (tag, g)
            assert _same(got["reproj"][g][:, 0], got["reproj"][g][:, 1]) and got["cost"][g, 0] == got["cost"][g, 1]


def test_the_cases_cover_what_they_claim():
    by = {tag: (inp, want) for tag, inp, want, _ in ref.cases()}
    assert by["one view: evaluated only"][1]["used"][1].tolist() == [0, 70, 0, 0] and by["one view: evaluated only"][1]["steps"].tolist() == [0, 0, 0]
    inp, want = by["three takes, fixed given (take 2: every view fixed, focal free), weights with zeros"]
    assert want["steps"].tolist() == [3, 3, 3] and np.array_equal(want["quat"][2], inp["quat"][2].astype(np.float64))     # a fixed-only take iterates on
    assert not np.array_equal(want["intr"][2][:, 0], inp["intr"][2][:, 0].astype(np.float64))                             # its focal factors
    assert not np.array_equal(want["intr"][0][0, 0], np.float64(inp["intr"][0][0, 0]))                                    # a fixed view's focal slot moves
    zero = np.asarray(inp["weights"]) == 0
    assert zero.any() and np.array_equal(want["points"][:, zero], inp["start"][:, zero].astype(np.float64))
    inp, want = by["three takes, gaps in valid and start_ok, view 2 missing in take 1"]
    assert want["used"][1, 2] == 0 and (want["used"][1, [0, 1, 3]] > 0).all() and _same(want["quat"][1, 2], inp["quat"][1, 2].astype(np.float64))
    out = inp["start_ok"] == 0
    assert out.any() and np.array_equal(want["points"][out], inp["start"][out].astype(np.float64))
    assert np.array_equal(by["three takes, focal held"][1]["intr"], by["three takes, focal held"][0]["intr"].astype(np.float64))


def test_without_a_camera_update_the_bits_are_the_statements():
    """every view held, the focal factors and the points free: no sine or cosine is on the path, so every operation is an IEEE +, -, x, / or square
    root in the rule's order - the device has the statement's bits: the costs as they are, every stored float the statement's value rounded once.
    That holds the ORDER of every sum (the joints' terms of S and s, the frames) to the rule, which no tolerance can"""
    sc = ref.scene(4, 17, [70, 40], seed=430)
    inp = ref.inputs(sc, fixed=np.ones((2, 4), np.uint8), weights=np.linspace(0.5, 1.5, 17).astype(np.float32))
    got, want = _calibrate(**inp), ref.calibrate(**inp)
    assert want["steps"].tolist() == [3, 3] and got["steps"].tolist() == [3, 3]
    assert _same(got["cost"], want["cost"])
    for k in ("intr", "points", "reproj", "quat", "trans"):
        assert _same(got[k], want[k].astype(np.float32)), k
    assert not _same(got["intr"], inp["intr"]) and not _same(got["points"], inp["start"])


def _raw(lib, inp, **over):
    """the entry point itself on an inputs dict"""
    V, F, J = inp["kp"].shape[:3]
    off = np.asarray(inp.get("take_offset", [0, F]), np.int64)
    G = len(off) - 1
    d = {k: _dev(np.ascontiguousarray(inp[k])) for k in ("start", "kp", "quat", "trans", "intr")}
    d["off"] = _dev(off)
    f32 = lambda *s: torch.full(s, -1.0, device="cuda")
    out = dict(quat=f32(G, V, 4), trans=f32(G, V, 3), intr=f32(G, V, 9), points=f32(F, J, 3), reproj=f32(G, V, 2),
               cost=torch.full((G, 2), -1.0, dtype=torch.float64, device="cuda"), steps=torch.full((G,), 7, dtype=torch.uint8, device="cuda"),
               ok=torch.full((G,), 7, dtype=torch.uint8, device="cuda"), used=torch.full((G, V), 7, dtype=torch.int32, device="cuda"))
    n = int(lib.mp_lift_calibrate_views_scratch_bytes(V, F, J))
    scratch = torch.empty(n // 8 + 1, dtype=torch.float64, device="cuda")
    a = dict(start=d["start"], kp=d["kp"], V=V, F=F, J=J, off=d["off"], G=G, quat=d["quat"], trans=d["trans"], intr=d["intr"], focal=1, distort=1,
             sigma=float(inp.get("sigma", ref.SIGMA)), prior=float(inp.get("prior", ref.PRIOR)), iters=int(inp.get("iters", 3)), scratch=scratch.data_ptr(),
             bytes=n, **{"o_" + k: v for k, v in out.items()})
    a.update(over)
    p = lambda x: x.data_ptr() if torch.is_tensor(x) else x
    rc = lib.mp_lift_calibrate_views(p(a["start"]), None, p(a["kp"]), a["V"], a["F"], a["J"], None, p(a["off"]), a["G"], p(a["quat"]), p(a["trans"]),
                                     p(a["intr"]), None, None, a["focal"], a["distort"], a["sigma"], a["prior"], a["iters"], p(a["o_quat"]), p(a["o_trans"]),
                                     p(a["o_intr"]), p(a["o_points"]), p(a["o_reproj"]), p(a["o_cost"]), p(a["o_steps"]), p(a["o_ok"]), p(a["o_used"]),
                                     a["scratch"], a["bytes"], None)
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in out.items()}
    got["rc"], got["scratch"] = rc, scratch.cpu().numpy()
    return got


def test_the_frames_rows_are_the_statements_bit_for_bit(lib):
    """White box: after a call with iters = 1 the scratch still holds what the frame kernel's first pass wrote, the head of the scratch being the
    frames' rows, entry-major (286 x Ftot doubles: S packed by rows, then s).  Nothing on the way to them is a sine or a cosine, so every frame's
    term of S and s has the statement's bits - which holds the ORDER in which a frame's joints are added to the rule; the reduced system's
    condition number hides a swapped order from every tolerance on the outputs"""
    sc = ref.scene(4, 17, [40], seed=440)
    inp = ref.inputs(sc, iters=1)
    got = _raw(lib, inp)
    assert got["rc"] == 0 and got["steps"][0] == 1
    V, F, J = inp["kp"].shape[:3]
    tk = ref.make_take(inp["start"], inp["kp"], inp["quat"][0], None, None, None, inp["intr"][0], True, ref.SIGMA, ref.PRIOR, slice(0, F))
    free, fslot, colv, iterates = ref.columns(tk.used.sum(axis=1), None, True)
    q, T = [ref.unit(inp["quat"][0, v]) for v in range(V)], [inp["trans"][0, v].astype(np.float64) for v in range(V)]
    e = ref.evaluate(tk, q, T, [1.0] * V, tk.start.copy(), True, tuple(free), fslot, tuple(colv))
    N = len(colv)
    rows = got["scratch"][:286 * F].reshape(286, F)
    assert iterates and N == ref.MAXN and free == [1, 2, 3]
    for r in range(N):
        for c in range(r + 1):
            assert _same(rows[r * (r + 1) // 2 + c], e["Sf"][:, r, c]), (r, c)
        assert _same(rows[253 + r], e["sf"][:, r]), r
    assert np.abs(e["Sf"]).min(axis=0)[np.tril_indices(N)].min() >= 0 and (np.abs(e["Sf"]).max(axis=0)[np.tril_indices(N)] > 0).all()     # (every entry is in use)


def test_invariants():
    from manipose_amd import calibrate_views
    sc = ref.scene(4, 17, [1, 70, 40], seed=410)
    valid, start_ok = ref.gap_tables(4, sc["off"], 411)
    spoiled = sc["kp"].copy()
    spoiled[valid == 0] = np.nan                                          # an invalid view's frame is never looked at
    cams = _cameras(sc["quat"], sc["trans"], sc["intr"])
    d = [_dev(a) for a in (sc["start"], spoiled, valid, start_ok)]
    a = calibrate_views(d[0], d[1], cams, d[2], sc["off"], d[3])
    b = calibrate_views(d[0], d[1], cams, d[2], sc["off"], d[3])
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(a[1:], b[1:]))           # identical bits
    assert _same(d[0].cpu().numpy(), sc["start"]) and np.array_equal(d[1].cpu().numpy(), spoiled, equal_nan=True)
    assert _same(d[2].cpu().numpy(), valid) and _same(d[3].cpu().numpy(), start_ok) and a.steps.tolist() == [3, 3, 3]
    kw = dict(valid=valid, start_ok=start_ok)
    clean = _calibrate(**ref.inputs(sc, **kw))
    assert all(_same(clean[k], x.cpu().numpy()) for k, x in zip(KEYS, a[1:]))
    for t in range(3):                                                    # a take alone: the bits it has beside the others
        sl = slice(int(sc["off"][t]), int(sc["off"][t + 1]))
        alone = _calibrate(sc["start"][sl], sc["kp"][:, sl], sc["quat"][t], sc["trans"][t], sc["intr"][t], valid[:, sl], None, start_ok[sl])
        assert _same(alone["points"], clean["points"][sl]) and all(_same(alone[k][0], clean[k][t]) for k in KEYS if k != "points")
    lowest = [int(np.nonzero(clean["used"][t])[0][0]) for t in range(3)]  # (the gaps may take a take's view 0 away)
    first = _calibrate(**ref.inputs(sc, fixed=np.eye(4, dtype=np.uint8)[lowest], **kw))
    assert all(_same(first[k], clean[k]) for k in KEYS)                   # fixed null: the lowest view with a used frame
    assert all(_same(clean["quat"][t, v], sc["quat"][t, v]) and _same(clean["trans"][t, v], sc["trans"][t, v]) for t, v in enumerate(lowest))


def test_entry_point_rejects_bad_arguments_before_any_launch(lib):
    sc = ref.scene(3, 5, [6], seed=420)
    inp = ref.inputs(sc)
    none = lambda g: all((g[k] == -1).all() for k in ("quat", "trans", "intr", "points", "reproj", "cost")) and (g["steps"] == 7).all() and \
        (g["ok"] == 7).all() and (g["used"] == 7).all()
    for name in ("start", "kp", "off", "quat", "trans", "intr", "o_quat", "o_trans", "o_intr", "o_points", "o_reproj", "o_cost", "o_steps", "o_ok", "o_used"):
        got = _raw(lib, inp, **{name: None})
        assert got["rc"] == 1 and b"null" in lib.mp_last_error() and none(got), name
    for kw, word in ((dict(V=0), b"V=0"), (dict(V=5), b"V=5"), (dict(J=1), b"J=1"), (dict(J=33), b"J=33"), (dict(F=0), b"out of range"), (dict(F=-1), b"out of range"),
                     (dict(G=0), b"out of range"), (dict(G=7), b"out of range"), (dict(F=2 ** 31), b"out of range"), (dict(distort=2), b"distort=2"),
                     (dict(focal=2), b"focal=2"), (dict(focal=-1), b"focal=-1"), (dict(sigma=0.0), b"sigma"), (dict(sigma=-1.0), b"sigma"),
                     (dict(sigma=float("nan")), b"sigma"), (dict(prior=0.0), b"prior"), (dict(prior=-1e-3), b"prior"), (dict(prior=float("nan")), b"prior"),
                     (dict(prior=float("inf")), b"prior"), (dict(iters=-1), b"iters=-1"), (dict(iters=9), b"iters=9"), (dict(scratch=None), b"scratch"),
                     (dict(bytes=8), b"scratch")):
        got = _raw(lib, inp, **kw)
        assert got["rc"] == 1 and word in lib.mp_last_error() and none(got), (kw, lib.mp_last_error())
    n = int(lib.mp_lift_calibrate_views_scratch_bytes(3, 6, 5))
    assert n == 6 * 8 * (286 + 1 + 75 * 5 + 96)
    got = _raw(lib, inp, bytes=n - 1)
    assert got["rc"] == 1 and b"scratch" in lib.mp_last_error() and none(got)
    buf = torch.empty(n // 8 + 1, dtype=torch.float64, device="cuda")
    got = _raw(lib, inp, scratch=buf.data_ptr() + 4)
    assert got["rc"] == 1 and b"misaligned" in lib.mp_last_error() and none(got)
    good = _raw(lib, inp)
    assert good["rc"] == 0
    _compare("the entry point itself", good, ref.calibrate(**inp))
    from manipose_amd import calibrate_views
    cams = _cameras(sc["quat"], sc["trans"], sc["intr"])
    start, kp = _dev(sc["start"]), _dev(sc["kp"])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        calibrate_views(start.cpu(), kp, cams)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        calibrate_views(start, kp, cams, points_ok=torch.ones(6, dtype=torch.uint8))
    with pytest.raises(ValueError, match="prior must be a finite number > 0"):
        calibrate_views(start, kp, cams, prior=0)
    with pytest.raises(ValueError, match="lists 1 takes, take_offset 2"):
        calibrate_views(start, kp, cams, take_offset=[0, 3, 6])


@pytest.mark.parametrize("V", [4, 2])
def test_recovery_scene_on_the_device(V):
    """the scene of test_lift_calibrate_host.test_recovery_on_the_committed_scene through calibrate_views: every view's focal error ends below a
    quarter of its start, the mean point error falls, and the device agrees with the statement"""
    sc = ref.recovery(V)
    got = _calibrate(**ref.inputs(sc))
    e0, e1 = ref.focal_errors(sc["intr"], sc), ref.focal_errors(got["intr"], sc)
    p0, p1 = ref.point_error(sc["start"], sc), ref.point_error(got["points"], sc)
    print(V, "views: focal", e0, "->", e1, "points", p0, "->", p1, "cost", got["cost"])
    assert got["steps"][0] == 3 and (e1 < 0.25 * e0).all() and p1 < p0
    assert _same(got["quat"][0, 0], sc["quat"][0, 0]) and _same(got["trans"][0, 0], sc["trans"][0, 0]) and _same(got["intr"][0][:, 2:], sc["intr"][0][:, 2:])
    _compare(f"recovery, {V} views", got, ref.calibrate(**ref.inputs(sc)))


# ---- end to end: the tiny fp32 fixture model of lift_fixtures.py -----------------------------------------------------------------------------
def _group(lens=(20, 20, 20, 20, 12, 12, 12), seed=51):
    """one group of 7 sequences: a take of 4 views of 20 frames, then a take of 3 views of 12 frames; S11's cameras as fetch() hands them on"""
    from manipose_amd.data.ingest import h36m_cameras
    s11 = h36m_cameras()["S11"]
    g = np.random.default_rng(seed)
    seqs = [np.clip(0.3 * g.standard_normal((n, 17, 2)), -1, 1).astype(np.float32) for n in lens]
    cams = [np.concatenate([s11[i]["intrinsic"], s11[i]["orientation"], s11[i]["translation"], np.array([i])]) for i in (0, 1, 2, 3, 0, 1, 2)]
    return {"walk": seqs}, {"walk": cams}


def _entry():
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "hpe"))
    import _entry
    return _entry


@pytest.mark.parametrize("mode", ["dataset", "bundle", "start_focal"])
def test_run_lift_with_calibrated_takes_end_to_end(tmp_path, mode):
    """run.lift with lift.fuse_calibrate=3: with the dataset's intrinsics (after the closed form, and after lift.fuse_bundle) and with
    lift.fuse_calibrate_start_focal; with the option off lift.npz keeps every byte"""
    from lift_fixtures import fixture_model
    e = _entry()
    model, T, K = fixture_model("rmcl")
    groups, cams = _group()
    base = ["run.lift=true", "train.tta=false", "train.batch_size_test=2", "lift.hyps=true", "lift.fuse=true", "lift.fuse_cameras=estimate",
            "lift.frame=world", "lift.floor=true", "lift.fuse_triangulate=true"]
    base += ["lift.fuse_bundle=2", "lift.fuse_bundle_sigma=0.5"] if mode == "bundle" else []
    base += ["lift.fuse_calibrate_start_focal=2.2"] if mode == "start_focal" else []
    before = e.lift_sequences_to_file(model, e.load_config(base), groups, str(tmp_path / "before.npz"), cams)
    named = e.lift_sequences_to_file(model, e.load_config(base + ["lift.fuse_calibrate=0"]), groups, str(tmp_path / "off.npz"), cams)
    assert open(str(tmp_path / "before.npz"), "rb").read() == open(str(tmp_path / "off.npz"), "rb").read() and list(before) == list(named)
    got = e.lift_sequences_to_file(model, e.load_config(base + ["lift.fuse_calibrate=3", "lift.fuse_calibrate_sigma=0.5"]), groups, str(tmp_path / "cal.npz"), cams)
    suffix = "bundle" if mode == "bundle" else "align"
    added = [f"walk.fused{t}{k}" for t in (0, 1) for k in e.CALIBRATE_KEYS] + \
        [f"walk.fused{t}__cam_{k}_{suffix}" for t in (0, 1) for k in e.CALIBRATE_MOVED]
    assert sorted(set(got) - set(before)) == sorted(added) and set(before) <= set(got)
    assert all(_same(got[k], v) for k, v in before.items() if ".fused" not in k)          # the views' own outputs do not change
    z = np.load(str(tmp_path / "cal.npz"))
    assert all(_same(z[k], got[k]) for k in got)
    s11 = e.synthetic_cameras({"a": [0, 1, 2, 3]})["a"]
    for t, (n, V) in enumerate(((20, 4), (12, 3))):
        k = f"walk.fused{t}"
        for s in e.CALIBRATE_MOVED:                                       # the cameras the calibration started from are kept beside its own
            assert _same(got[f"{k}__cam_{s}_{suffix}"], before[f"{k}__cam_{s}"]) and got[f"{k}__cam_{s}"].shape == before[f"{k}__cam_{s}"].shape
        assert _same(got[k + "__cam_quat"][0], before[k + "__cam_quat"][0]) and _same(got[k + "__cam_trans"][0], before[k + "__cam_trans"][0])      # the first view is held
        assert got[k + "__cal"].shape == (n, 17, 3) and got[k + "__cal"].dtype == np.float32 and np.isfinite(got[k + "__cal"]).all()
        assert got[k + "__cam_intr"].shape == (V, 9) and got[k + "__cam_focal"].shape == (V, 2) and got[k + "__cam_focal_err"].shape == (V,)
        assert got[k + "__cal_reproj"].shape == (V, 2) and got[k + "__cal_cost"].shape == (2,) and got[k + "__cal_cost"].dtype == np.float64
        assert got[k + "__cal_steps"].dtype == got[k + "__cal_ok"].dtype == np.uint8 and got[k + "__cal_used"].shape == (V,) and got[k + "__cal_used"].dtype == np.int32
        assert got[k + "__cal_cost"][1] <= got[k + "__cal_cost"][0] * (1 + 1e-6) and 0 <= got[k + "__cal_steps"] <= 3
        start = np.float32(2.2) if mode == "start_focal" else None
        for v in range(V):
            fx0 = start if start is not None else np.float32(s11[v]["intrinsic"][0])
            assert got[k + "__cam_focal"][v, 0] == fx0 and got[k + "__cam_focal"][v, 1] == got[k + "__cam_intr"][v, 0] > 0
            assert abs(got[k + "__cam_focal_err"][v] - abs(float(got[k + "__cam_intr"][v, 0]) / float(np.float32(s11[v]["intrinsic"][0])) - 1)) < 1e-6
            want = [0] * 7 if start is not None else np.asarray(s11[v]["intrinsic"], np.float32)[2:].tolist()
            assert got[k + "__cam_intr"][v, 2:].tolist() == want              # the centre and the distortion are never touched
        if got[k + "__cal_steps"] == 0:
            assert _same(got[k + "__cam_quat"], before[k + "__cam_quat"]) and _same(got[k + "__cam_focal"][:, 0], got[k + "__cam_focal"][:, 1])
        assert got[k].shape == (n, 17, 3) and got[k + "__root"].shape == (n, 3) and got[k + "__tri"].shape == (n, 17, 3) and np.isfinite(got[k]).all()
    if mode == "start_focal":
        assert all(got[f"walk.{i}__cam"][:9].tolist() == [np.float32(2.2)] * 2 + [0] * 7 for i in range(7))      # what the stages read


def test_calibrated_takes_in_synthetic_mode(lib, tmp_path, monkeypatch):
    """run.lift with lift.fuse_calibrate and lift.score on synthetic data: every take has one view, which decides no focal length - the
    calibration evaluates, nothing moves, and lift_score_cal.csv is written"""
    import os
    e = _entry()
    monkeypatch.chdir(tmp_path)
    argv = ["run.train=false", "run.test=false", "run.lift=true", "lift.stride=14", "train.batch_size_test=4", "data.seq_len=27", "model.channels=64",
            "model.layers=2", "model.nheads=4", "model.channels_seg=32", "model.layers_seg=1", "model.nheads_seg=4", "multi_hyp.n_hyp=3",
            "data.synthetic_sequences=2", "model.precision=fp32", "lift.frame=world", "lift.floor=true", "lift.fuse=true", "lift.fuse_cameras=estimate",
            "lift.hyps=true", "lift.score=true"]
    e.run(argv)
    out = os.path.join(str(tmp_path), "default")
    before = dict(np.load(os.path.join(out, "lift.npz")))
    assert not os.path.exists(os.path.join(out, "lift_score_cal.csv"))
    e.run(argv + ["lift.fuse_calibrate=3"])
    z = np.load(os.path.join(out, "lift.npz"))
    assert set(before) <= set(z.files) and all(_same(z[k], v) for k, v in before.items())
    assert os.path.exists(os.path.join(out, "lift_score_cal.csv"))
    for name in ("synthetic_000", "synthetic_001"):
        k = f"{name}.fused0"
        assert z[k + "__cal_steps"] == 0 and z[k + "__cal_ok"] in (0, 1) and z[k + "__cal_used"].shape == (1,) and _same(z[k + "__cam_quat_align"], z[k + "__cam_quat"])
        assert _same(z[k + "__cam_focal"][:, 0], z[k + "__cam_focal"][:, 1]) and z[k + "__cam_focal_err"].tolist() == [0.0]
        assert z[k + "__cal"].shape == z[k].shape and np.abs(z[k + "__cal"] - z[k]).max() < 1e-5      # copied through: the fused pose at its root, in its frame

"""Bundle-adjusting a take's cameras on the device: mp_lift_bundle_views against the float64 statement of its rule (lift_bundle_ref.py), the
constructed takes compared exactly, the invariants (identical bits, a take alone and beside others, inputs untouched), argument errors, the
recovery scene the feature is for, and run.lift with lift.fuse_bundle end to end.

The bounds against the statement, ON THE SAME float32 INPUTS: steps, ok and used are equal; cost within 1e-9 relative; every stored float (quat,
trans, root, reproj) within 2^-23 max(1, |x|), the project's bound for a float32 store.  The kernel and the statement both work in fp64 and differ
in nothing but the library's sine and cosine: relative 1e-16, amplified by the reduced system's condition number (7e3 to 1e5 in the compared
scenes, which the statement's trace records) - far below the one rounding to float32 that remains.  That holds where every decision is away from its threshold, which
test_lift_bundle_host.py asserts of every compared scene without a device; the bounds are not measured from the kernel.  Measured on an MI355X:
the worst stored float is 0.48 of its bound, the one rounding and nothing else, and every cost has the statement's bits."""
import os
import sys

import numpy as np
import pytest
import torch

import lift_bundle_ref as ref
from lift_fixtures import fixture_model as _model, same as _same

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hpe"))
KEYS = ("quat", "trans", "root", "reproj", "cost", "steps", "ok", "used")


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _cameras(quat, trans, intr):
    """place_views' nested list of the (G, V, .) tables"""
    G, V = quat.shape[:2]
    return [[np.concatenate([intr[g, v], quat[g, v], trans[g, v]]) for v in range(V)] for g in range(G)]


def _bundle(pose, root, kp, quat, trans, intr, valid=None, take_offset=None, root_ok=None, fixed=None, weights=None, distort=True,
            sigma=float("inf"), iters=3):
    from manipose_amd import bundle_views
    G = 1 if take_offset is None else len(take_offset) - 1
    quat, trans, intr = (np.asarray(a).reshape(G, kp.shape[0], -1) for a in (quat, trans, intr))
    res = bundle_views(_dev(pose), _dev(root), _dev(kp), _cameras(quat, trans, intr), _dev(valid), take_offset, _dev(root_ok), fixed, weights, distort,
                       sigma, iters)
    torch.cuda.synchronize()
    got = {k: r.cpu().numpy() for k, r in zip(KEYS, res[1:])}
    for g, take in enumerate(res.cameras):                                # the nested cameras are the tables, to be passed on
        for v, cam in enumerate(take):
            assert np.array_equal(cam[:9], intr[g, v]) and _same(cam[9:13], got["quat"][g, v]) and _same(cam[13:], got["trans"][g, v])
    return got


def _compare(tag, got, want):
    assert got["used"].dtype == np.int32 and got["ok"].dtype == got["steps"].dtype == np.uint8 and got["cost"].dtype == np.float64
    for k in ("steps", "ok", "used"):
        assert np.array_equal(got[k], want[k]), (tag, k, got[k], want[k])
    dc = np.abs(got["cost"] - want["cost"]) / np.maximum(np.abs(want["cost"]), 1e-300)
    worst = {}
    for k in ("quat", "trans", "root", "reproj"):
        assert got[k].dtype == np.float32
        fine, worst[k] = ref.within_store(got[k], want[k])
    print(f"[{tag}] cost off by {dc.max():.2e} relative; of 2^-23 max(1, |x|): " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert (dc <= ref.COST_TOL).all(), (tag, dc)
    assert all(v <= 1.0 for v in worst.values()), (tag, worst)


@pytest.mark.parametrize("n", range(len(ref.cases())))
def test_bundle_matches_the_statement(n):
    tag, inp, want, _ = ref.cases()[n]
    _compare(tag, _bundle(**inp), want)


def _copied(got, inp, g=0):
    return _same(got["quat"][g], inp["quat"][g]) and _same(got["trans"][g], inp["trans"][g])


def test_constructed_takes_are_exact():
    sc = ref.scene(3, 5, [12], seed=31)
    inp = ref.inputs(sc, sigma=0.05)
    nan = dict(inp, kp=inp["kp"].copy())
    nan["kp"][1, :, 2, 0] = np.nan                                        # every frame of view 1 has a NaN keypoint: the view observes nothing
    got, want = _bundle(**nan), ref.bundle(**nan)
    assert got["used"][0].tolist() == [12, 0, 12] and _same(got["quat"][0, 1], inp["quat"][0, 1]) and got["reproj"][0, 1].tolist() == [0, 0] and got["steps"][0] == 3
    _compare("NaN keypoints in view 1", got, want)
    one = dict(inp, kp=inp["kp"].copy(), root=inp["root"].copy())
    one["kp"][:, 4, 1, 1], one["root"][7, 2] = np.nan, np.inf             # frame 4: no view observes it; frame 7: its root is not finite
    got = _bundle(**one)
    assert got["used"][0].tolist() == [10, 10, 10] and _same(got["root"][[4, 7]], one["root"][[4, 7]]) and got["steps"][0] == 3
    _compare("two frames outside the problem", got, ref.bundle(**one))
    behind = dict(inp, pose=inp["pose"].copy())
    behind["pose"][5, 3] = (-40.0 * ref.rotation(ref.unit(inp["quat"][0, 0]))[:, 2]).astype(np.float32)          # a joint 40 m behind camera 0
    got = _bundle(**behind)
    assert got["ok"][0] == 0 and got["steps"][0] == 0 and _copied(got, inp) and _same(got["root"], inp["root"])
    assert _same(got["reproj"][..., 0], got["reproj"][..., 1]) and got["cost"][0, 0] == got["cost"][0, 1]
    free = _bundle(**dict(inp, fixed=np.zeros((1, 3), np.uint8)))         # no fixed view: evaluated only
    assert free["ok"][0] == 1 and free["steps"][0] == 0 and _copied(free, inp) and _same(free["root"], inp["root"]) and free["cost"][0, 0] == free["cost"][0, 1] > 0
    held = _bundle(**dict(inp, fixed=np.ones((1, 3), np.uint8)))          # all views fixed: evaluated only
    assert all(_same(held[k], free[k]) for k in KEYS)
    _compare("all views fixed", held, ref.bundle(**dict(inp, fixed=np.ones((1, 3), np.uint8))))
    zero = dict(inp, quat=inp["quat"].copy())
    zero["quat"][0, 0] = 0                                                # view 0 has a zero quaternion: view 1 is the fixed view (place_views' cameras refuse
    from manipose_amd import _lib                                         # a zero quaternion: through the entry point)
    got = _raw(_lib.load(), zero)
    want = ref.bundle(**zero)
    assert got["used"][0].tolist() == [0, 12, 12] and _same(got["quat"][0, :2], zero["quat"][0, :2]) and _same(got["trans"][0, :2], zero["trans"][0, :2])
    _compare("a zero quaternion", got, want)
    far = ref.inputs(ref.refused_scene(), iters=8)                        # the second step would raise the cost: not taken, the state of the first stays
    got = _bundle(**far)
    assert got["steps"][0] == 1 and got["ok"][0] == 1
    _compare("a refused step", got, ref.bundle(**far))
    assert all(_same(got[k], v) for k, v in _bundle(**dict(far, iters=1)).items())
    off = _bundle(**dict(inp, iters=0))                                   # iters = 0: copied through bit for bit
    assert off["steps"][0] == 0 and off["ok"][0] == 1 and _copied(off, inp) and _same(off["root"], inp["root"])


def _raw(lib, inp, scratch_bytes=None, **over):
    """the entry point itself on an inputs dict"""
    V, F, J = inp["kp"].shape[:3]
    off = np.asarray(inp.get("take_offset", [0, F]), np.int64)
    G = len(off) - 1
    d = {k: _dev(np.ascontiguousarray(inp[k])) for k in ("pose", "root", "kp", "quat", "trans", "intr")}
    d["off"] = _dev(off)
    out = dict(quat=torch.full((G, V, 4), -1.0, device="cuda"), trans=torch.full((G, V, 3), -1.0, device="cuda"), root=torch.full((F, 3), -1.0, device="cuda"),
               reproj=torch.full((G, V, 2), -1.0, device="cuda"), cost=torch.full((G, 2), -1.0, dtype=torch.float64, device="cuda"),
               steps=torch.full((G,), 7, dtype=torch.uint8, device="cuda"), ok=torch.full((G,), 7, dtype=torch.uint8, device="cuda"),
               used=torch.full((G, V), 7, dtype=torch.int32, device="cuda"))
    n = int(lib.mp_lift_bundle_views_scratch_bytes(V, F))
    scratch = torch.empty(n // 8 + 1, dtype=torch.float64, device="cuda")
    a = dict(pose=d["pose"], root=d["root"], kp=d["kp"], V=V, F=F, J=J, off=d["off"], G=G, quat=d["quat"], trans=d["trans"], intr=d["intr"], distort=1,
             sigma=float(inp.get("sigma", float("inf"))), iters=int(inp.get("iters", 3)), scratch=scratch.data_ptr(), bytes=n if scratch_bytes is None else scratch_bytes,
             **{"o_" + k: v for k, v in out.items()})
    a.update(over)
    p = lambda x: x.data_ptr() if torch.is_tensor(x) else x
    rc = lib.mp_lift_bundle_views(p(a["pose"]), p(a["root"]), None, p(a["kp"]), a["V"], a["F"], a["J"], None, p(a["off"]), a["G"], p(a["quat"]), p(a["trans"]),
                                  p(a["intr"]), None, None, a["distort"], a["sigma"], a["iters"], p(a["o_quat"]), p(a["o_trans"]), p(a["o_root"]),
                                  p(a["o_reproj"]), p(a["o_cost"]), p(a["o_steps"]), p(a["o_ok"]), p(a["o_used"]), a["scratch"], a["bytes"], None)
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in out.items()}
    got["rc"] = rc
    return got


def test_invariants():
    from manipose_amd import bundle_views
    sc = ref.scene(4, 17, [1, 70, 40], seed=210)
    valid, root_ok = ref.gap_tables(4, sc["off"], 211)
    spoiled = sc["kp"].copy()
    spoiled[valid == 0] = np.nan                                          # an invalid view's frame is never looked at
    cams = _cameras(sc["quat"], sc["trans"], sc["intr"])
    d = [_dev(a) for a in (sc["pose"], sc["root"], spoiled, valid, root_ok)]
    a = bundle_views(d[0], d[1], d[2], cams, d[3], sc["off"], d[4])
    b = bundle_views(d[0], d[1], d[2], cams, d[3], sc["off"], d[4])
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(a[1:], b[1:]))           # identical bits
    assert _same(d[0].cpu().numpy(), sc["pose"]) and _same(d[1].cpu().numpy(), sc["root"]) and np.array_equal(d[2].cpu().numpy(), spoiled, equal_nan=True)
    assert _same(d[3].cpu().numpy(), valid) and _same(d[4].cpu().numpy(), root_ok) and a.steps.tolist() == [3, 3, 3]
    kw = dict(valid=valid, root_ok=root_ok, sigma=0.05)
    clean = _bundle(**ref.inputs(sc, **kw))
    assert all(_same(clean[k], x.cpu().numpy()) for k, x in zip(KEYS, a[1:]))
    for t in range(3):                                                    # a take alone: the bits it has beside the others
        sl = slice(int(sc["off"][t]), int(sc["off"][t + 1]))
        alone = _bundle(sc["pose"][sl], sc["root"][sl], sc["kp"][:, sl], sc["quat"][t], sc["trans"][t], sc["intr"][t], valid[:, sl], None, root_ok[sl], sigma=0.05)
        assert _same(alone["root"], clean["root"][sl]) and all(_same(alone[k][0], clean[k][t]) for k in KEYS if k != "root")
    first = _bundle(**ref.inputs(sc, fixed=np.array([[1, 0, 0, 0]] * 3, np.uint8), **kw))
    assert all(_same(first[k], clean[k]) for k in KEYS)                   # fixed null: the lowest view with a used frame
    assert all(_same(clean["quat"][t, 0], sc["quat"][t, 0]) and _same(clean["trans"][t, 0], sc["trans"][t, 0]) for t in range(3))


def test_entry_point_rejects_bad_arguments_before_any_launch(lib):
    sc = ref.scene(3, 5, [6], seed=32)
    inp = ref.inputs(sc)
    none = lambda g: (g["quat"] == -1).all() and (g["trans"] == -1).all() and (g["root"] == -1).all() and (g["reproj"] == -1).all() and \
        (g["cost"] == -1).all() and (g["steps"] == 7).all() and (g["ok"] == 7).all() and (g["used"] == 7).all()
    for name in ("pose", "root", "kp", "off", "quat", "trans", "intr", "o_quat", "o_trans", "o_root", "o_reproj", "o_cost", "o_steps", "o_ok", "o_used"):
        got = _raw(lib, inp, **{name: None})
        assert got["rc"] == 1 and b"null" in lib.mp_last_error() and none(got), name
    for kw, word in ((dict(V=0), b"V=0"), (dict(V=5), b"V=5"), (dict(J=1), b"J=1"), (dict(J=33), b"J=33"), (dict(F=0), b"out of range"), (dict(F=-1), b"out of range"),
                     (dict(G=0), b"out of range"), (dict(G=7), b"out of range"), (dict(F=2 ** 31), b"out of range"), (dict(distort=2), b"distort=2"),
                     (dict(sigma=0.0), b"sigma"), (dict(sigma=-1.0), b"sigma"), (dict(sigma=float("nan")), b"sigma"), (dict(iters=-1), b"iters=-1"),
                     (dict(iters=9), b"iters=9"), (dict(scratch=None), b"scratch"), (dict(bytes=8), b"scratch")):
        got = _raw(lib, inp, **kw)
        assert got["rc"] == 1 and word in lib.mp_last_error() and none(got), (kw, lib.mp_last_error())
    n = int(lib.mp_lift_bundle_views_scratch_bytes(3, 6))
    assert n == 6 * 3056 and lib.mp_lift_bundle_views_scratch_bytes(0, 6) == 0 and lib.mp_lift_bundle_views_scratch_bytes(5, 6) == 0 and \
        lib.mp_lift_bundle_views_scratch_bytes(3, 0) == 0
    got = _raw(lib, inp, bytes=n - 1)
    assert got["rc"] == 1 and b"scratch" in lib.mp_last_error() and none(got)
    buf = torch.empty(n // 8 + 1, dtype=torch.float64, device="cuda")
    got = _raw(lib, inp, scratch=buf.data_ptr() + 4)
    assert got["rc"] == 1 and b"misaligned" in lib.mp_last_error() and none(got)
    good = _raw(lib, inp)
    assert good["rc"] == 0
    _compare("the entry point itself", good, ref.bundle(**inp))
    from manipose_amd import bundle_views
    cams = _cameras(sc["quat"], sc["trans"], sc["intr"])
    pose, root, kp = (_dev(sc[k]) for k in ("pose", "root", "kp"))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        bundle_views(pose.cpu(), root, kp, cams)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        bundle_views(pose, root, kp, cams, root_ok=torch.ones(6, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="bundle_views takes device tensors"):
        bundle_views(pose, root, kp, cams, valid=torch.ones(kp.shape[0], 6, dtype=torch.uint8))
    with pytest.raises(ValueError, match="lists 1 takes, take_offset 2"):
        bundle_views(pose, root, kp, cams, take_offset=[0, 3, 6])


def test_recovery_scene_on_the_device():
    """the scenes of test_lift_bundle_host.test_recovery_on_the_committed_seeds.  Noise-free, the device is held against the TRUTH, not against the
    statement (F at the minimum is rounding: a decision there is a coin's); with noise, against the statement as well."""
    sc = ref.recovery(0.0)
    got = _bundle(**ref.inputs(sc, iters=ref.RECOVERY_STEPS))
    deg, m = ref.camera_errors(got["quat"], got["trans"], sc)
    worst = np.abs(got["root"].astype(np.float64) - sc["true_root"]).max()
    print("noise-free: degrees", deg[1:], "metres", m[1:], "roots", worst, "steps", got["steps"])
    assert got["steps"][0] == ref.RECOVERY_STEPS and deg.max() <= ref.RECOVERY_DEG + ref.STORE_DEG and m.max() <= ref.RECOVERY_M + ref.STORE_M
    assert worst <= ref.RECOVERY_ROOT + ref.STORE_ROOT                    # (the statement's bounds and the float32 store's half ulp)
    assert _same(got["quat"][0, 0], sc["quat"][0, 0]) and _same(got["trans"][0, 0], sc["trans"][0, 0])
    sc = ref.recovery(0.002)
    d0, m0 = ref.camera_errors(sc["quat"], sc["trans"], sc)
    got = _bundle(**ref.inputs(sc))
    deg, m = ref.camera_errors(got["quat"], got["trans"], sc)
    print("noise 0.002: degrees", deg[1:], "from", d0[1:], "metres", m[1:], "from", m0[1:])
    assert (deg[1:] < d0[1:]).all() and (m[1:] < m0[1:]).all() and got["steps"][0] == 3
    _compare("recovery, noise 0.002", got, ref.bundle(**ref.inputs(sc)))
    again = _bundle(sc["pose"], got["root"], sc["kp"], got["quat"], got["trans"], sc["intr"])       # passed on: at the minimum nothing moves by much
    assert np.abs(again["root"] - got["root"]).max() < 1e-5 and again["cost"][0, 1] <= again["cost"][0, 0] * (1 + 1e-6)


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
def test_run_lift_with_bundled_cameras_end_to_end(tmp_path, frame):
    from _entry import BUNDLE_KEYS, lift_sequences_to_file, load_config
    model, T, K = _model("rmcl")
    groups, cams = _group()
    base = ["run.lift=true", "train.tta=false", "train.batch_size_test=2", "lift.hyps=true", "lift.fuse=true", "lift.fuse_cameras=estimate"]
    base += ["lift.frame=world", "lift.floor=true"] if frame == "world" else []
    before = lift_sequences_to_file(model, load_config(base), groups, str(tmp_path / "before.npz"), cams)
    named = lift_sequences_to_file(model, load_config(base + ["lift.fuse_bundle=0"]), groups, str(tmp_path / "off.npz"), cams)
    a, b = np.load(str(tmp_path / "before.npz")), np.load(str(tmp_path / "off.npz"))
    assert list(a.keys()) == list(b.keys()) == list(before) == list(named) and all(a[k].dtype == b[k].dtype and _same(a[k], b[k]) for k in a.keys())
    got = lift_sequences_to_file(model, load_config(base + ["lift.fuse_bundle=3", "lift.fuse_bundle_sigma=0.5"]), groups, str(tmp_path / "bundle.npz"), cams)
    new = sorted(set(got) - set(before))
    assert new == sorted(f"walk.fused{t}__cam_{k}" for t in (0, 1) for k in BUNDLE_KEYS) and set(before) <= set(got)
    assert all(_same(got[k], v) for k, v in before.items() if ".fused" not in k)          # the views' own outputs do not change
    z = np.load(str(tmp_path / "bundle.npz"))
    assert all(_same(z[k], got[k]) for k in got)
    for t, (n, V) in enumerate(((20, 4), (12, 3))):
        k = f"walk.fused{t}__cam_"
        for s in ("quat", "trans", "err_deg", "err_m"):                   # the closed form's values are kept beside the refined ones
            assert _same(got[k + s + "_align"], before[k + s]) and got[k + s].shape == before[k + s].shape and got[k + s].dtype == before[k + s].dtype
        assert _same(got[k + "quat"][0], before[k + "quat"][0]) and _same(got[k + "trans"][0], before[k + "trans"][0])          # the first view is fixed
        assert got[k + "bundle_reproj"].shape == (V, 2) and got[k + "bundle_cost"].shape == (2,) and got[k + "bundle_cost"].dtype == np.float64
        assert got[k + "bundle_steps"].dtype == got[k + "bundle_ok"].dtype == np.uint8 and got[k + "bundle_used"].shape == (V,) and got[k + "bundle_used"].dtype == np.int32
        assert got[k + "bundle_cost"][1] <= got[k + "bundle_cost"][0] * (1 + 1e-6) and 0 <= got[k + "bundle_steps"] <= 3
        if got[k + "bundle_steps"] > 0:
            assert np.abs(np.linalg.norm(got[k + "quat"].astype(np.float64), axis=1) - 1).max() < 1e-6 and (got[k + "quat"][:, 0] >= 0).all()
        assert got[f"walk.fused{t}"].shape == (n, 17, 3) and got[f"walk.fused{t}__root"].shape == (n, 3) and got[f"walk.fused{t}__reproj"].shape == (V, n)
        assert np.isfinite(got[f"walk.fused{t}"]).all()


def test_bundled_cameras_in_synthetic_mode(lib, tmp_path, monkeypatch):
    """run.lift with lift.fuse_bundle on synthetic data: every take has one view, which is the fixed one - the bundle evaluates and nothing moves"""
    from _entry import run
    monkeypatch.chdir(tmp_path)
    argv = ["run.train=false", "run.test=false", "run.lift=true", "lift.stride=14", "train.batch_size_test=4", "data.seq_len=27", "model.channels=64",
            "model.layers=2", "model.nheads=4", "model.channels_seg=32", "model.layers_seg=1", "model.nheads_seg=4", "multi_hyp.n_hyp=3",
            "data.synthetic_sequences=2", "model.precision=fp32", "lift.frame=world", "lift.floor=true", "lift.fuse=true", "lift.fuse_cameras=estimate"]
    run(argv)
    out = os.path.join(str(tmp_path), "default")
    before = dict(np.load(os.path.join(out, "lift.npz")))
    run(argv + ["lift.fuse_bundle=3"])
    z = np.load(os.path.join(out, "lift.npz"))
    assert set(before) <= set(z.files) and all(_same(z[k], v) for k, v in before.items())
    for name in ("synthetic_000", "synthetic_001"):
        k = f"{name}.fused0__cam_"
        assert z[k + "bundle_steps"] == 0 and z[k + "bundle_ok"] in (0, 1) and z[k + "bundle_used"].shape == (1,) and _same(z[k + "quat_align"], z[k + "quat"])

"""Pinning a take's feet on the device: mp_lift_footlock against the float64 statement of its rule (lift_footlock_ref.py), constructed scenes compared
exactly, the invariants (identical bits, a sequence alone and beside others, inputs untouched, only knees and ankles differ, bone lengths kept),
argument errors through the ABI and through lock_feet, the recovery scene the feature is for, and run.lift with lift.footlock end to end.

The bound against the statement, ON THE SAME float32 INPUTS (test_lift_footlock_host.py derives it, without a device): run, runs and flags are
EQUAL; out, target and moved are within ONE float32 ulp of max(|want|, L), L the largest |coordinate| of a leg joint in the sequence - the anchors
carry the same bits on both sides (their sums are exact, or a tie is 4 error bounds away), every branch is taken with an asserted margin, what fp64
leaves between the anchors and the stores travels with a measured amplification of at most 24 against an allowed 350 000, and the rounding to
float32 is half an ulp.  Thigh and shank of a re-posed leg stay within 2 ulp of L.  The bounds are derived, not measured from the kernel.
Measured on an MI355X, the worst of the five cases and the three recovery scenes, in these ulps: out 0.000, target 0.000, moved 0.000 - kernel and
statement agree to the bit on these inputs (every compared sum is exact, and both sides follow the header's order) -; thigh and shank 0.837.

The recovery scene (a synthetic walk with known plants, 5 mm of noise, 10 % of the stance frames drifting by 2 mm a frame, seeds 0..2), on the device:
the skate over the unclamped run frames falls from 8.7 .. 9.6 mm a frame to exactly 0 (no frame is reach clamped: every contact pair), the stance
ankle's mean distance from its clean plant from 9.3 .. 9.4 mm to 2.9 .. 3.2 mm, its largest from 42 .. 44 mm to 9 .. 16 mm.  Synthetic walkers;
nothing is measured on real data."""
import os
import sys

import numpy as np
import pytest
import torch

import lift_footlock_ref as ref
from lift_fixtures import same as _same

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hpe"))
KEYS = ("points", "run", "target", "moved", "flags", "runs", "skate", "skate_pairs")
DTYPES = dict(run=np.int32, runs=np.int32, skate_pairs=np.int32, flags=np.uint8)
NAMES = dict(out="points", target="target", moved="moved")


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _ground_of(floor):
    from manipose_amd.lift_ops import Ground
    if floor is None:
        return None
    return Ground(_dev(floor[0]), _dev(floor[1]), None, None, None, None, None, _dev(floor[2]), None, None, None, None)


def _lock(points, contact, off=None, valid=None, floor=None, **kw):
    from manipose_amd import lock_feet
    res = lock_feet(_dev(points), _dev(contact), off, _dev(valid), ground=_ground_of(floor), **kw)
    torch.cuda.synchronize()
    assert res._fields == KEYS
    return {k: r.cpu().numpy() for k, r in zip(KEYS, res)}


def _bones(pts, legs):
    p = pts[..., :3].astype(np.float64)
    return np.stack([np.stack([np.linalg.norm(p[:, k] - p[:, h], axis=1), np.linalg.norm(p[:, a] - p[:, k], axis=1)], 1) for h, k, a in legs], 1)


def _compare(tag, got, want, inp):
    off, legs, pts = inp["off"], inp["opts"]["legs"], inp["points"]
    S, (ntot, nf) = len(off) - 1, want["run"].shape
    shapes = dict(points=pts.shape, run=(ntot, nf), target=(ntot, nf, 3), moved=(ntot, nf), flags=(ntot, nf), runs=(S, nf), skate=(S,), skate_pairs=(S,))
    for k in KEYS:
        assert got[k].shape == shapes[k] and got[k].dtype == DTYPES.get(k, np.float32), (tag, k, got[k].shape, got[k].dtype)
    for k in ("run", "runs", "flags"):
        assert np.array_equal(got[k], want[k]), (tag, k, np.nonzero(got[k] != want[k]))
    assert ref.margins_hold(want["margin"]), (tag, want["margin"])
    worst = {}
    for k in ref.FLOATS:
        g, w = got[NAMES[k]].astype(np.float64), np.asarray(want[k], np.float64)
        if k == "out":
            assert np.array_equal(np.isfinite(g), np.isfinite(w)), tag
            g, w = np.where(np.isfinite(g), g, 0.0)[..., :3], np.where(np.isfinite(w), w, 0.0)[..., :3]
        else:
            assert np.isfinite(g).all(), (tag, k)
        worst[k] = float((np.abs(g - w) / ref.bound(k, want, off)).max())
    posed = want["posed"]
    with np.errstate(invalid="ignore"):                                   # (a leg nobody re-posed may hold the input's NaN)
        change = np.abs(_bones(got["points"], legs) - _bones(pts, legs))
    worst["bones"] = float((change / ref.ulp32(ref.frame_scale(want, off))[:, None, None])[posed].max())
    print(f"[{tag}] off the statement, in float32 ulp of max(|want|, L): " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert max(worst[k] for k in ref.FLOATS) <= 1.0 and worst["bones"] <= 2.0, (tag, worst)
    # only the knees and ankles of re-posed legs differ from the input, by their bits; channel 3 included
    same = got["points"].view(np.uint32) == pts.view(np.uint32)
    touched = np.zeros(pts.shape[:2], bool)
    for k, (h, kn, a) in enumerate(legs):
        touched[:, kn] |= posed[:, k]
        touched[:, a] |= posed[:, k]
    assert same[~touched].all() and (pts.shape[2] == 3 or same[..., 3].all()), tag
    fl = inp["opts"]["floor"]
    sk, pairs = ref.skate(got["points"], inp["contact"], off, [leg[2] for leg in legs], fl, inp["valid"])
    assert np.array_equal(got["skate_pairs"], pairs) and np.allclose(got["skate"], sk, rtol=1e-6, atol=1e-9), (tag, got["skate"], sk)
    return worst


@pytest.mark.parametrize("n", range(len(ref.cases())))
def test_footlock_matches_the_statement(n):
    tag, inp, want = ref.cases()[n]
    o = inp["opts"]
    got = _lock(inp["points"], inp["contact"], inp["off"], inp["valid"], o["floor"], legs=o["legs"], blend=o["blend"], stretch=o["stretch"])
    _compare(tag, got, want, inp)
    held = np.zeros(len(inp["points"]), bool)
    held[int(inp["off"][0]):int(inp["off"][-1])] = True
    for k in ("run", "target", "moved", "flags"):                         # frames that no sequence holds: zeros
        assert not got[k][~held].any(), (tag, k)


def test_constructed_scenes_are_exact():
    zero = lambda a: not any(np.ascontiguousarray(a).tobytes())           # +0 everywhere, by its bits
    pts, c = ref.dyadic_scene(slide=2.0 ** -8)
    none = _lock(pts, np.zeros_like(c))                                   # no contacts: out is points bit for bit
    assert none["points"].tobytes() == pts.tobytes() and zero(none["flags"]) and zero(none["moved"]) and zero(none["run"]) and zero(none["runs"])
    assert _same(none["target"], pts[:, [3, 6]]) and zero(none["skate"]) and zero(none["skate_pairs"])
    got, want = _lock(pts, c), ref.footlock(pts, c)                       # a stance foot sliding by 2^-8 a frame: one ankle for the whole run, skate exactly 0
    assert len({got["points"][f, 3].tobytes() for f in range(4, 20)}) == 1 and got["points"][4, 3].tolist() == [0, 2.0 ** -8 * 11.5, 0]
    assert got["skate"][0] == 0 and zero(got["skate"]) and got["skate_pairs"][0] == 15 and got["runs"].tolist() == [[1, 0]]
    assert _same(got["points"], want["out"]) and _same(got["target"], want["target"].astype(np.float32)) and _same(got["moved"], want["moved"].astype(np.float32))
    assert _same(got["flags"], want["flags"]) and _same(got["run"], want["run"]) and (got["flags"][4:20, 0] == 1).all() and (got["flags"][[0, 1, 2, 3, 20, 21], 0] == 2).all()
    # ankle' is the stored target, not hip + D u formed again: at these anchors 1 + (-1 / D) D is 2^-53 and not 0 in fp64, which would show in z
    for slide, contact, y in ((2.0 ** -7, (12, 22), 68 * 2.0 ** -9), (6 * 2.0 ** -8, (9, 23), 192 * 2.0 ** -9), (6 * 2.0 ** -8, (14, 23), 222 * 2.0 ** -9)):
        D = np.sqrt((0.0 + y * y) + 1.0)
        assert 1.0 + (-1.0 / D) * D != 0.0 and D < 1.1
        pts, c = ref.dyadic_scene(slide=slide, contact=contact)
        got, want = _lock(pts, c), ref.footlock(pts, c)
        pinned = got["points"][contact[0]:contact[1] + 1, 3]
        assert (got["flags"][contact[0]:contact[1] + 1, 0] == 1).all() and zero(pinned[:, [0, 2]]) and (pinned[:, 1] == np.float32(y)).all() and _same(got["points"], want["out"])
    pts, c = ref.straight_leg_scene()                                     # the pole from an axis; a clamp back onto the input
    got, want = _lock(pts, c), ref.footlock(pts, c)
    assert got["flags"][:, 0].tolist() == [17, 5] and _same(got["points"], want["out"]) and _same(got["points"][1], pts[1]) and got["moved"][:, 0].tolist() == [0.125, 0]
    assert got["points"][0, 3].tolist() == [0, 0, 0.125] and got["points"][0, 2, 1] == 0 and got["points"][0, 2, 2] == 0.5625 and got["points"][0, 2, 0] > 0.24
    pts, c = ref.dyadic_scene()
    pts[6, 2] = pts[6, 1]                                                 # a thigh without length: bit 5 alone, zeros, the leg as it was
    got = _lock(pts, c)
    assert got["flags"][6, 0] == 32 and zero(got["target"][6, 0]) and zero(got["moved"][6, 0]) and got["run"][6, 0] == 16 and _same(got["points"], pts)
    pts, c = ref.dyadic_scene()
    pts[2, 3, 2] = -0.125                                                 # a swing foot below the floor
    fl = (np.array([[0, 0, 1]], np.float32), np.array([0.0625], np.float32), np.array([1], np.uint8))
    got, want = _lock(pts, c, floor=fl, blend=1), ref.footlock(pts, c, floor=fl, blend=1)
    assert (got["points"][4:20, 3, 2] == 0.0625).all() and got["flags"][2, 0] == 8 and got["points"][2, 3, 2] == 0.0625 and _same(got["points"], want["out"])
    assert _same(got["flags"], want["flags"])
    off = _lock(pts, c, floor=(fl[0], fl[1], np.array([2], np.uint8)), blend=1)      # bit 0 of ok clear: floor off
    assert (off["flags"][:3, 0] == 0).all() and (off["points"][4:20, 3, 2] == 0).all()


def test_invariants():
    from manipose_amd import lock_feet
    tag, inp, want = ref.cases()[0]
    pts, con, valid, off, fl = inp["points"], inp["contact"], inp["valid"], inp["off"], inp["opts"]["floor"]
    d = [_dev(pts), _dev(con), _dev(valid)]
    g = _ground_of(fl)
    a = lock_feet(d[0], d[1], off, d[2], ground=g)
    b = lock_feet(d[0], d[1], off, d[2], ground=g)
    torch.cuda.synchronize()
    assert all(torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y) for x, y in zip(a, b))
    assert np.array_equal(d[0].cpu().numpy(), pts, equal_nan=True) and _same(d[1].cpu().numpy(), con) and _same(d[2].cpu().numpy(), valid)      # inputs untouched
    full = {k: x.cpu().numpy() for k, x in zip(KEYS, a)}
    filled = pts.copy()                                                   # frames that are not good, and frames no sequence holds, are never read
    filled[valid == 0] = 1.5
    filled[:int(off[0])] = 2.5
    clean = _lock(filled, con, off, valid, fl)
    for k in KEYS[1:]:
        assert _same(clean[k], full[k]), k
    ok = valid != 0
    ok[:int(off[0])] = False
    assert _same(clean["points"][ok], full["points"][ok]) and _same(clean["points"][~ok], filled[~ok])
    for s in range(len(off) - 1):                                         # a sequence alone: the bits it has beside the others
        sl = slice(int(off[s]), int(off[s + 1]))
        if sl.stop == sl.start:
            continue
        alone = _lock(filled[sl], con[sl], None, valid[sl], tuple(t[s:s + 1] for t in fl))
        for k in KEYS:
            assert _same(alone[k], clean[k][s:s + 1] if k in ("runs", "skate", "skate_pairs") else clean[k][sl]), (s, k)


@pytest.mark.parametrize("seed", range(3))
def test_recovery_scene_on_the_device(seed):
    """A synthetic walk with known plants, 5 mm of noise, 10 % of the stance frames drifting by 2 mm a frame.  No threshold beyond: the skate over the
    unclamped run frames is exactly 0, and the stance ankle is no further from its clean plant than the input's.  Measured on an MI355X, seeds
    0, 1, 2: skate 9.117, 9.554, 8.707 mm a frame -> 0; the ankle's mean error 9.37, 9.41, 9.28 mm -> 2.85, 3.11, 3.15 mm, its largest 44.19, 41.52,
    41.97 mm -> 9.33, 13.61, 16.34 mm.  Not real data."""
    from manipose_amd import lock_feet
    from manipose_amd.lift_ops import Ground
    sc = ref.recovery_scene(seed)
    fl = (np.array([[0, 0, 1]], np.float32), np.zeros(1, np.float32), np.ones(1, np.uint8))
    got = _lock(sc["points"], sc["contact"], floor=fl)
    want = ref.footlock(sc["points"], sc["contact"], floor=fl)
    inp = dict(points=sc["points"], contact=sc["contact"], off=np.array([0, 300]), valid=None, opts=dict(legs=ref.H36M_LEGS, floor=fl, blend=5, stretch=1.0))
    _compare(f"recovery {seed}", got, want, inp)
    free = ((got["flags"] & 5) == 1).astype(np.uint8)
    before = ref.skate(sc["points"], sc["contact"], inp["off"], (3, 6), fl)[0][0]
    g = Ground(_dev(fl[0]), _dev(fl[1]), None, None, None, None, None, _dev(fl[2]), None, None, None, None)
    again = lock_feet(_dev(got["points"]), _dev(sc["contact"] * free), ground=g)      # the locked feet, locked again over the unclamped run frames ...
    assert float(again.skate[0]) == 0.0 and int(again.skate_pairs[0]) > 250      # ... they do not slide: exactly 0
    after = ref.skate(got["points"], sc["contact"] * free, inp["off"], (3, 6), fl)
    st = sc["stance"]
    err0 = np.linalg.norm(sc["points"][:, [3, 6]].astype(np.float64) - sc["truth"], axis=2)[st]
    err1 = np.linalg.norm(got["points"][:, [3, 6]].astype(np.float64) - sc["truth"], axis=2)[st]
    print(f"seed {seed}: skate {1000 * before:.3f} -> {1000 * after[0][0]:.3f} mm a frame over {after[1][0]} pairs (all contact pairs: {1000 * got['skate'][0]:.3f}); stance ankle "
          f"off its plant by {1000 * err0.mean():.2f} -> {1000 * err1.mean():.2f} mm (mean), {1000 * err0.max():.2f} -> {1000 * err1.max():.2f} (max); "
          f"{int((got['flags'] & 4 != 0).sum())} reach clamped")
    assert after[0][0] == 0.0 and after[1][0] > 250 and err1.mean() <= err0.mean()


def test_entry_point_rejects_bad_arguments_before_any_launch(lib):
    import ctypes as C
    N, J, S, nf = 40, 17, 2, 2
    pts = torch.zeros(N, J, 3, device="cuda")
    con = torch.ones(N, nf, dtype=torch.uint8, device="cuda")
    off = torch.tensor([0, 25, N], dtype=torch.int64, device="cuda")
    f = lambda *shape: torch.full(shape, -1.0, device="cuda")
    i = lambda *shape, dt=torch.int32: torch.full(shape, 7, dtype=dt, device="cuda")
    outs = dict(out=f(N, J, 3), run=i(N, nf), target=f(N, nf, 3), moved=f(N, nf), flags=i(N, nf, dt=torch.uint8), runs=i(S, nf))
    plane = dict(normal=torch.zeros(S, 3, device="cuda"), offset=torch.zeros(S, device="cuda"), plane_ok=torch.zeros(S, dtype=torch.uint8, device="cuda"))
    p = lambda x: None if x is None else x.data_ptr()

    def call(x=pts, c=con, o=off, n=N, j=J, ch=3, s=S, legs=((1, 2, 3), (4, 5, 6)), nfeet=None, floor=(), blend=5, stretch=1.0, alias=False, **null):
        table = None if legs is None else (C.c_int32 * (3 * len(legs)))(*(q for leg in legs for q in leg))
        return lib.mp_lift_footlock(p(x), n, j, ch, None, p(o), s, p(c), table, (len(legs) if legs is not None else 2) if nfeet is None else nfeet,
                                    *(p(plane[k]) if k in floor else None for k in ("normal", "offset", "plane_ok")), blend, stretch,
                                    *(p(x) if alias and k == "out" else None if k in null else p(t) for k, t in outs.items()), None)
    for kw in (dict(x=None), dict(c=None), dict(o=None), dict(legs=None)) + tuple({k: None} for k in outs):
        assert call(**kw) == 1 and b"null" in lib.mp_last_error(), (kw, lib.mp_last_error())
    nan = float("nan")
    for kw, word in ((dict(j=1), b"J=1"), (dict(j=33), b"J=33"), (dict(ch=2), b"C=2"), (dict(ch=5), b"C=5"), (dict(n=0), b"out of range"), (dict(s=0), b"out of range"),
                     (dict(s=41), b"out of range"), (dict(n=2 ** 30), b"too many"), (dict(alias=True), b"out == points"), (dict(legs=(), nfeet=0), b"nf=0"),
                     (dict(legs=((1, 2, 3),) * 5), b"nf=5"), (dict(legs=((1, 2, 17),)), b"legs[0][2] = 17"), (dict(legs=((1, 2, 3), (-1, 5, 6))), b"legs[1][0] = -1"),
                     (dict(legs=((1, 2, 2),)), b"named twice"), (dict(legs=((1, 2, 3), (4, 5, 3))), b"named twice"), (dict(legs=((1, 2, 3), (1, 5, 6))), b"named twice"),
                     (dict(floor=("normal",)), b"all three or none"), (dict(floor=("normal", "offset")), b"all three or none"), (dict(floor=("plane_ok",)), b"all three or none"),
                     (dict(blend=-1), b"blend=-1"), (dict(blend=33), b"blend=33"), (dict(stretch=0.0), b"stretch"), (dict(stretch=1.5), b"stretch"),
                     (dict(stretch=-1.0), b"stretch"), (dict(stretch=nan), b"stretch")):
        assert call(**kw) == 1 and word in lib.mp_last_error(), (kw, lib.mp_last_error())
    torch.cuda.synchronize()
    assert all(bool((t == (7 if t.dtype in (torch.int32, torch.uint8) else -1)).all()) for t in outs.values())      # nothing was launched
    assert call() == 0 and call(floor=("normal", "offset", "plane_ok"), blend=0, stretch=0.5, legs=((4, 5, 6),)) == 0 and call(blend=32) == 0
    torch.cuda.synchronize()
    # all-zero points: every frame is lockable, the legs have no length: runs of 25 and 15 frames, bit 5 alone
    assert outs["runs"].tolist() == [[1, 1], [1, 1]] and outs["run"][:, 0].tolist() == [25] * 25 + [15] * 15 and bool((outs["flags"] == 32).all())
    assert not outs["out"].any() and not outs["target"].any() and not outs["moved"].any()
    from manipose_amd import lock_feet
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        lock_feet(pts.cpu(), con)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        lock_feet(pts, con.cpu())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        lock_feet(pts, con, valid=torch.ones(N, dtype=torch.uint8))
    with pytest.raises(ValueError, match="joint twice"):
        lock_feet(pts, con, legs=((1, 2, 3), (3, 5, 6)))
    with pytest.raises(ValueError, match="blend"):
        lock_feet(pts, con, blend=33)


# ---- end to end: run.lift in synthetic-data mode ------------------------------------------------------------------------------------------------
COMMON = ["run.train=false", "run.test=false", "run.lift=true", "lift.stride=14", "train.batch_size_test=4", "data.seq_len=27", "model.channels=64",
          "model.layers=2", "model.nheads=4", "model.channels_seg=32", "model.layers_seg=1", "model.nheads_seg=4", "multi_hyp.n_hyp=3",
          "data.synthetic_sequences=2", "model.precision=fp32", "lift.place=true", "lift.ground=estimate", "lift.ground_speed=1000"]      # (a speed every synthetic foot stays under: every valid frame a contact)
NEW = ("__locked", "__lock_flags", "__lock_moved", "__lock_run", "__skate_locked", "__skate_pairs_locked")


def test_run_lift_with_footlock_end_to_end(tmp_path, monkeypatch):
    from _entry import run
    from manipose_amd import estimate_ground, lock_feet
    monkeypatch.chdir(tmp_path)
    run(COMMON + ["run.experiment=before"])
    run(COMMON + ["run.experiment=locked", "lift.footlock=true", "lift.footlock_blend=3"])
    a, z = (np.load(os.path.join(str(tmp_path), d, "lift.npz")) for d in ("before", "locked"))
    keys = [f"synthetic_{i:03d}" for i in range(2)]
    assert sorted(set(z.files) - set(a.files)) == sorted(k + s for k in keys for s in NEW) and set(a.files) <= set(z.files)
    assert all(a[k].dtype == z[k].dtype and a[k].shape == z[k].shape and a[k].tobytes() == z[k].tobytes() for k in a.files)      # every earlier key keeps its bytes
    assert not os.path.exists(os.path.join(str(tmp_path), "before", "lift_footlock.csv"))
    assert open(os.path.join(str(tmp_path), "before", "lift_ground.csv")).read() == open(os.path.join(str(tmp_path), "locked", "lift_ground.csv")).read()
    rows = open(os.path.join(str(tmp_path), "locked", "lift_footlock.csv")).read().splitlines()
    assert rows[0] == "key,frames,runs_r,runs_l,locked,clamped,moved_mean_mm,moved_max_mm,skate_mm,skate_locked_mm" and [r.split(",")[0] for r in rows[1:]] == keys
    for i, k in enumerate(keys):
        n = 27 * 4 + 37 * i + 11
        assert z[k + "__locked"].shape == (n, 17, 3) and z[k + "__locked"].dtype == np.float32
        assert z[k + "__lock_flags"].shape == z[k + "__lock_moved"].shape == z[k + "__lock_run"].shape == (n, 2)
        assert z[k + "__lock_flags"].dtype == np.uint8 and z[k + "__lock_moved"].dtype == np.float32 and z[k + "__lock_run"].dtype == np.int32
        assert z[k + "__skate_locked"].shape == z[k + "__skate_pairs_locked"].shape == () and z[k + "__skate_pairs_locked"].dtype == np.int32
        # the same calls on the file's own arrays: the points as they were emitted
        pts, valid = _dev(z[k] + z[k + "__traj"][:, None]), _dev(z[k + "__ok"])
        g = estimate_ground(pts, None, valid, speed=1000.0)
        assert _same(z[k + "__contact"], g.contact.cpu().numpy())
        want = lock_feet(pts, g.contact, None, valid, ground=g, blend=3)
        assert _same(z[k + "__locked"], want.points.cpu().numpy()) and _same(z[k + "__lock_flags"], want.flags.cpu().numpy())
        assert _same(z[k + "__lock_moved"], want.moved.cpu().numpy()) and _same(z[k + "__lock_run"], want.run.cpu().numpy())
        assert _same(z[k + "__skate_locked"], want.skate[0].cpu().numpy()) and _same(z[k + "__skate_pairs_locked"], want.skate_pairs[0].cpu().numpy())
        assert z[k + "__skate_pairs_locked"] == z[k + "__skate_pairs"] and rows[1 + i].split(",")[1] == str(n)
        assert int(rows[1 + i].split(",")[4]) == int((z[k + "__lock_flags"] & 1 != 0).sum()) == int((z[k + "__lock_run"] > 0).sum())
        assert _same(z[k + "__locked"][z[k + "__lock_flags"].max(axis=1) == 0], (z[k] + z[k + "__traj"][:, None])[z[k + "__lock_flags"].max(axis=1) == 0])

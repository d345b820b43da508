"""Pinning a take's feet, without a device: the float64 statement of mp_lift_footlock's rule (lift_footlock_ref.py) against scenes built by hand, what
it promises (bone lengths kept, anchors on the floor, the ease bounded by the blend), every condition the device bound of test_gpu_lift_footlock.py
stands on, the argument errors and the entry point's option combinations with their messages, and the new ABI entry declared everywhere.

THE DEVICE BOUND, derived here and used there: run, runs and flags are EQUAL, every float is within ONE float32 ulp of max(|want|, L), L the largest
|coordinate| of a leg joint in the sequence.  Kernel and statement read the same float32 numbers and work in fp64.  (1) The anchor is the one value
that is rounded to float32 on the way: both sides round the same fp64 number if their sums agree - they do to the bit where the sum is exact in
every order, which a sum of float32 coordinates of one size is (every compared anchor: the margin `tie` is inf) - or, where they only agree to
(N + 16) u, if the anchor lies at least 4 of those from a rounding tie (asserted).  (2) Every branch of steps C and D is taken with the margin
lift_footlock_ref.py names, asserted for every compared case, so both sides take the same branches.  (3) What remains between the anchors and the
stores is a few dozen fp64 operations, at most 64 u relative on any intermediate value (the header gives their order, a side may still differ in
it), plus N u where a sum is not exact: E = (N + 64) u = 2.2e-14 for N = 130.  The host test MEASURES how far such an error travels.  WHAT IS
DISTURBED IS NOT THE ANCHORS' SUMS THEMSELVES: a sum's error ends at the anchor's rounding to float32, which either swallows it (point 1: the same
float32 on both sides) or turns it into a whole float32 ulp, a jump no amplification figure describes - so the sums are held by the `tie` margin, and
the disturbance goes in behind that rounding, where the fp64 chain starts: every target of step C (the anchor, or the eased ankle) and the lengths l1,
l2, D are disturbed by delta = 1e-9, and the largest change of any output over L, over delta, is the amplification kappa
- 3 to 24 over these cases (the IK is well conditioned where the knee is bent: y / l1 >= 1e-3 is asked, 1.8e-2 is the least).  Asserted:
4 kappa E <= a quarter ulp of 1 (2^-25), the factor 4 because kappa is sampled; kappa could be 350 000.  (4) The one rounding to float32, half an
ulp.  Together under one ulp.  Thigh and shank of a re-posed leg: each end is off its fp64 position by at most sqrt(3) / 2 ulp of L, the fp64
positions keep the lengths to a few u: 2 ulp of L."""
import os
import re
import sys

import numpy as np
import pytest
import torch

import lift_footlock_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hpe"))


def test_the_statement_on_scenes_built_by_hand():
    pts, c = ref.dyadic_scene(slide=2.0 ** -8)                            # contact in frames 4..19, the ankle slides along y
    got = ref.footlock(pts, c, blend=5)
    anchor = np.array([0.0, 2.0 ** -8 * 11.5, 0.0])                       # the mean of 4..19 is 11.5
    assert got["runs"].tolist() == [[1, 0]] and got["run"][:, 0].tolist() == [0] * 4 + [16] * 16 + [0] * 4 and not got["run"][:, 1].any()
    assert (got["out"][4:20, 3] == anchor.astype(np.float32)).all() and (got["target"][4:20, 0] == anchor).all() and (got["flags"][4:20, 0] == 1).all()
    assert np.array_equal(got["moved"][4:20, 0], np.abs(pts[4:20, 3, 1].astype(np.float64) - anchor[1]))
    # the ease: e = anchor - a at the run's border, w = 1 - j / 6 for the j-th frame outside, s(w) = w^2 (3 - 2 w)
    for j in range(1, 5):
        w = 1.0 - j / 6.0
        s = (w * w) * (3.0 - 2.0 * w)
        for f, e in ((4 - j, anchor[1] - 2.0 ** -8 * 4), (19 + j, anchor[1] - 2.0 ** -8 * 19)):
            assert got["flags"][f, 0] == 2 and got["target"][f, 0, 1] == np.float32(pts[f, 3, 1] + s * e), (f, j)
    assert (got["flags"][:, 1] == 0).all() and np.array_equal(got["out"][:, 4:], pts[:, 4:]) and np.array_equal(got["out"][:, :2], pts[:, :2])      # the other leg, the hips
    none = ref.footlock(pts, np.zeros_like(c))
    assert none["out"].tobytes() == pts.tobytes() and not none["flags"].any() and not none["moved"].any() and not none["runs"].any()
    assert np.array_equal(none["target"], pts[:, [3, 6]])                 # a foot nobody pins is sent to where it is
    # B = 0: no ease at all; a gap shorter than the ramp: the two weights sum to 1
    hard = ref.footlock(pts, c, blend=0)
    assert (hard["flags"][:4, 0] == 0).all() and (hard["flags"][20:, 0] == 0).all() and np.array_equal(hard["out"][:4], pts[:4])
    c2 = c.copy()
    c2[10:13, 0] = 0                                                      # runs 4..9 and 13..19, a gap of 3 under B = 5: L = min(6, 13 - 9) = 4
    gap = ref.footlock(pts, c2, blend=5)
    a1, a2 = 2.0 ** -8 * 6.5, 2.0 ** -8 * 16.0
    for f in (10, 11, 12):
        wp, wn = 1.0 - (f - 9) / 4.0, 1.0 - (13 - f) / 4.0
        sp, sn = (wp * wp) * (3.0 - 2.0 * wp), (wn * wn) * (3.0 - 2.0 * wn)
        assert wp + wn == 1.0 and sp + sn == 1.0 and gap["flags"][f, 0] == 2
        assert gap["target"][f, 0, 1] == np.float32((pts[f, 3, 1] + sp * (a1 - 2.0 ** -8 * 9)) + sn * (a2 - 2.0 ** -8 * 13))
    # the straight leg: frame 0 takes its pole from the x axis, frame 1 is clamped back onto where it was
    pts, c = ref.straight_leg_scene()
    st = ref.footlock(pts, c)
    y = np.sqrt(0.25 - 0.4375 ** 2)
    assert st["flags"][:, 0].tolist() == [1 | 16, 1 | 4] and st["run"][:, 0].tolist() == [2, 2]
    assert np.array_equal(st["out"][0, 2], np.array([y, 0, 1 - 0.4375], np.float32)) and np.array_equal(st["out"][0, 3], np.array([0, 0, 0.125], np.float32))
    assert np.array_equal(st["out"][1], pts[1]) and st["moved"][1, 0] == 0 and st["target"][1, 0].tolist() == [0, 0, 0.25] and st["moved"][0, 0] == 0.125
    # a leg without length is left alone, bit 5 alone; a floor under the feet puts the anchor on it and lifts a swing foot onto it
    pts, c = ref.dyadic_scene()
    pts[6, 2] = pts[6, 1]
    zero = ref.footlock(pts, c)
    assert zero["flags"][6, 0] == 32 and not zero["target"][6, 0].any() and zero["run"][6, 0] == 16 and np.array_equal(zero["out"][6], pts[6])
    pts, c = ref.dyadic_scene()
    pts[2, 3, 2] = -0.125                                                 # a swing foot under z = 0, outside the ease of B = 1
    fl = (np.array([[0, 0, 1]], np.float32), np.array([0.0625], np.float32), np.array([1], np.uint8))
    up = ref.footlock(pts, c, floor=fl, blend=1)
    assert (up["out"][4:20, 3, 2] == 0.0625).all() and up["flags"][2, 0] == 8 and up["out"][2, 3, 2] == 0.0625 and up["flags"][0, 0] == 8
    off = ref.footlock(pts, c, floor=(fl[0], fl[1], np.array([2], np.uint8)), blend=1)      # bit 0 clear: the sequence has no floor
    assert (off["flags"][:3, 0] == 0).all() and (off["out"][4:20, 3, 2] == 0).all()


def test_bone_lengths_are_kept_and_anchors_lie_on_the_floor():
    for tag, inp, want in ref.cases():
        pts, legs, off = inp["points"][..., :3].astype(np.float64), inp["opts"]["legs"], inp["off"]
        out = want["out"][..., :3].astype(np.float64)
        L = ref.frame_scale(want, off)
        worst = 0.0
        for k, (hj, kj, aj) in enumerate(legs):
            m = want["posed"][:, k]
            assert m.any(), tag
            for a, b in ((hj, kj), (kj, aj)):
                was, now = np.linalg.norm(pts[m, b] - pts[m, a], axis=1), np.linalg.norm(out[m, b] - out[m, a], axis=1)
                worst = max(worst, float((np.abs(now - was) / ref.ulp32(L[m])).max()))
            assert np.array_equal(want["out"][~m][:, [kj, aj]], inp["points"][~m][:, [kj, aj]], equal_nan=True), tag
        others = [j for j in range(pts.shape[1]) if j not in {j for leg in legs for j in leg[1:]}]
        assert np.array_equal(want["out"][:, others], inp["points"][:, others], equal_nan=True), tag      # only knees and ankles ever differ
        if inp["points"].shape[2] == 4:
            assert np.array_equal(want["out"][..., 3], inp["points"][..., 3], equal_nan=True), tag
        print(f"[{tag}] thigh and shank of {int(want['posed'].sum())} re-posed legs off by at most {worst:.3f} ulp of L")
        assert worst <= 2.0, tag
        fl = inp["opts"]["floor"]
        if fl is not None:
            dist = 0.0
            for s in np.nonzero(fl[2] & 1)[0]:
                sl = slice(int(off[s]), int(off[s + 1]))
                pinned = (want["flags"][sl] & 5) == 1                       # in a run, not reach clamped
                if pinned.any():
                    h = want["target"][sl][pinned] @ fl[0][s].astype(np.float64) - float(fl[1][s])
                    dist = max(dist, float(np.abs(h).max() / ref.ulp32(want["scale"][s])))
            print(f"[{tag}] pinned ankles off the floor by at most {dist:.3f} ulp of L")
            assert 0 < dist <= 1.0, tag                                   # three roundings to float32 along a unit normal: sqrt(3) / 2 ulp of L


def test_the_ease_is_bounded_by_the_blend():
    """Outside runs the correction target - ankle is s(w) e of the neighbouring runs' e = anchor - ankle at their border: never longer than the
    longer e (the weights' s sum to at most 1), and between consecutive frames it changes by at most 1.5 / L of them (s' <= 1.5, w moves by 1 / L)."""
    sc = ref.scene(21, (120,), (([(20, 40), (70, 90)], [(0, 10), (14, 30), (110, 119)]),), lead=0, tail=0)
    for B in (0, 1, 5, 12):
        got = ref.footlock(sc["points"], sc["contact"], sc["off"], blend=B)
        assert not (got["flags"] & 4).any()
        a = sc["points"][:, [3, 6], :3].astype(np.float64)
        c = got["target"] - a
        for k in range(2):
            run = got["run"][:, k] > 0
            border = run & ~(np.roll(run, 1) & np.roll(run, -1))
            emax = np.linalg.norm(c[border, k], axis=1).max()
            outside = np.nonzero(~run)[0]
            assert np.linalg.norm(c[outside, k], axis=1).max() <= emax * (1 + 1e-12)
            far = [f for f in outside if not run[max(f - B, 0):f + B + 1].any()]
            assert len(far) > 0 or B == 12
            assert not c[far, k].any() and not got["flags"][far, k].any()      # further than B frames from every run: untouched
            ends, starts = np.nonzero(run[:-1] & ~run[1:])[0], np.nonzero(~run[:-1] & run[1:])[0] + 1
            Lmin = min([B + 1] + [int(starts[starts > fa].min()) - int(fa) for fa in ends if (starts > fa).any()])
            pairs = [f for f in range(119) if not (run[f] and run[f + 1])]
            step = max(np.linalg.norm(c[f + 1, k] - c[f, k]) for f in pairs)
            assert step <= 2 * 1.5 * emax / Lmin * (1 + 1e-12), (B, k, step, emax, Lmin)
            # the first frame after a run with no run near on the other side: s(1 - 1 / (B + 1)) e exactly
            for f in np.nonzero(run[:-1] & ~run[1:])[0]:
                if not run[f + 1:f + 2 + B + 1].any():
                    w = 1.0 - 1.0 / (B + 1.0)
                    assert np.allclose(c[f + 1, k], (w * w) * (3 - 2 * w) * c[f, k], rtol=0, atol=1e-6), (B, k, f)      # (target is a float32: an ulp of a few metres)


def test_every_condition_the_device_bound_stands_on():
    sizes = set()
    seen = np.zeros(6, int)
    for tag, inp, want in ref.cases():
        mg = want["margin"]
        print(f"[{tag}] margins " + ", ".join(f"{k} {v:.3g}" for k, v in mg.items()))
        assert ref.margins_hold(mg), (tag, mg)
        n_max = int(want["run"].max())
        E = (n_max + 64) * ref.U
        kappa = ref.amplification(inp, want)
        budget = 0.25 * 2.0 ** -23 / (4.0 * E)
        print(f"[{tag}] longest run {n_max}, amplification {kappa:.3g} (allowed {budget:.3g})")
        assert kappa <= budget, tag
        assert np.isfinite(want["target"]).all() and np.isfinite(want["moved"]).all()
        sizes |= set(np.diff(inp["off"]).tolist())
        seen += [int(((want["flags"] >> i) & 1).sum()) for i in range(6)]
    assert {0, 1, 2, 3, 130} <= sizes
    assert (seen[:4] > 50).all(), seen                                    # pinned, eased, reach clamped and lifted (frame, foot)s are all compared in numbers
    tag, inp, want = ref.cases()[0]
    o = inp["off"]
    r = want["run"]
    assert r[o[0], 0] == 1 and r[o[1], 0] == 2 and r[o[2]:o[3], 0].tolist() == [1, 0, 1] and r[o[2]:o[3], 1].tolist() == [0, 1, 0]
    assert (r[o[4] + 60:o[4] + 71, 0] == 11).all() and r[o[4] + 71, 0] == 0 and r[o[4] + 72, 0] == 1 and (r[o[4] + 64:o[4] + 128, 1] == 64).all()
    assert r[o[4] + 63, 1] == 0 and r[o[4] + 128, 1] == 0 and (r[o[4] + 126:o[4] + 130, 0] == 4).all() and (r[o[6]:o[7], 0] == 70).all()
    assert want["runs"][5].tolist() == [3, 4] and r[o[5] + 10, 1] == 0 and r[o[5] + 20, 0] == 0      # the holes and the NaN knee split the runs
    assert not r[:o[0]].any() and not r[o[7]:].any() and len(r) == o[7] + 3


def test_the_recovery_scene_in_the_statement():
    """A synthetic walk with known plants, 5 mm of noise, 10 % of the stance frames drifting: the float64 statement (the device test has the figures)"""
    sc = ref.recovery_scene(0)
    fl = (np.array([[0, 0, 1]], np.float32), np.zeros(1, np.float32), np.ones(1, np.uint8))
    got = ref.footlock(sc["points"], sc["contact"], floor=fl)
    off = np.array([0, 300])
    before, pairs = ref.skate(sc["points"], sc["contact"], off, (3, 6), fl)
    free = (got["flags"] & 5) == 1
    after, _ = ref.skate(got["out"], sc["contact"] * free, off, (3, 6), fl)
    st = sc["stance"]
    err0 = np.linalg.norm(sc["points"][:, [3, 6]].astype(np.float64) - sc["truth"], axis=2)[st]
    err1 = np.linalg.norm(got["out"][:, [3, 6]].astype(np.float64) - sc["truth"], axis=2)[st]
    print(f"skate {1000 * before[0]:.3f} -> {1000 * after[0]:.3f} mm / frame over {pairs[0]} pairs; stance ankle off its plant by {1000 * err0.mean():.2f} -> "
          f"{1000 * err1.mean():.2f} mm (mean), {1000 * err0.max():.2f} -> {1000 * err1.max():.2f} mm (max); {int((got['flags'] & 4 != 0).sum())} clamped")
    assert after[0] == 0.0 and before[0] > 0.005 and err1.mean() <= err0.mean()


def test_argument_errors_are_value_errors_before_any_device_work():
    """The calls are given CPU tensors: had the arguments been accepted, they would have ended in the RuntimeError that refuses them ("no CPU
    fallback"), which is what the valid calls at the end do."""
    from manipose_amd import estimate_ground, lock_feet
    from manipose_amd.lift_ops import Ground
    pts, con, valid = torch.zeros(12, 17, 3), torch.ones(12, 2, dtype=torch.uint8), torch.ones(12, dtype=torch.uint8)
    z = torch.zeros
    g = Ground(z(1, 3), z(1), None, None, None, None, None, z(1, dtype=torch.uint8), None, None, None, None)
    for kw, word in ((dict(points=z(12, 17)), "points must be"), (dict(points=pts.double()), "points must be"), (dict(points=np.zeros((12, 17, 3))), "points must be"),
                     (dict(points=z(12, 1, 3)), "joints"), (dict(points=z(12, 3, 17).transpose(1, 2)), "points must be"), (dict(points=z(0, 17, 3), contact=con[:0]), "no frame"),
                     (dict(contact=None), "contact must be"), (dict(contact=con[:5]), "contact must be"), (dict(contact=con.bool()), "contact must be"),
                     (dict(contact=con[:, :1]), "contact must be"), (dict(valid=valid[:5]), "valid must be"), (dict(valid=valid.bool()), "valid must be"),
                     (dict(seq_offset=[0]), "seq_offset"), (dict(seq_offset=list(range(14))), "seq_offset"), (dict(legs=()), "legs must be"),
                     (dict(legs=((1, 2, 3),) * 5), "legs must be"), (dict(legs=((1, 2),)), "legs must be"), (dict(legs=((1, 2, 17),)), "legs must be"),
                     (dict(legs=((1, 2.0, 3),)), "legs must be"), (dict(legs=3), "sequence of"), (dict(legs=((1, 2, 2), (4, 5, 6))), "joint twice"),
                     (dict(legs=((1, 2, 3), (1, 5, 6))), "joint twice"), (dict(legs=((1, 2, 3), (4, 5, 3))), "joint twice"),
                     (dict(blend=-1), "blend"), (dict(blend=33), "blend"), (dict(blend=5.0), "blend"), (dict(blend=True), "blend"),
                     (dict(stretch=0), "stretch"), (dict(stretch=1.01), "stretch"), (dict(stretch=-0.5), "stretch"), (dict(stretch=float("nan")), "stretch"),
                     (dict(stretch="1"), "stretch"), (dict(stretch=1e-60), "stretch"), (dict(ground=3), "Ground record"), (dict(ground=g._replace(normal=z(2, 3))), "ground.normal"),
                     (dict(ground=g._replace(offset=z(1, 1))), "ground.offset"), (dict(ground=g._replace(ok=z(1))), "ground.ok"), (dict(ground=g._replace(ok=None)), "ground.ok"),
                     (dict(ground=g, seq_offset=[0, 5, 12]), "ground.normal")):
        with pytest.raises(ValueError, match=word):
            lock_feet(**dict(dict(points=pts, contact=con), **kw))
    for kw in (dict(), dict(valid=valid, blend=0, stretch=0.5, ground=g), dict(seq_offset=[0, 5, 12], legs=((4, 5, 6), (1, 2, 3))),
               dict(points=z(12, 5, 4), contact=con[:, :1], legs=((1, 2, 3),), seq_offset=torch.tensor([0, 12]), blend=32)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            lock_feet(**dict(dict(points=pts, contact=con), **kw))
    assert estimate_ground.__defaults__[2] == tuple(leg[2] for leg in lock_feet.__defaults__[2])      # the default legs end in the default feet


def test_config_keys_parse_and_a_footlock_without_the_ground_fails():
    from _entry import FOOTLOCK_DEFAULTS, LIFT_SUFFIXES, lift_footlock_options, load_config, run
    cfg = load_config([])
    assert cfg.lift.footlock is False and lift_footlock_options(cfg) == (False, FOOTLOCK_DEFAULTS) and FOOTLOCK_DEFAULTS == dict(blend=5, stretch=1.0, floor=True)
    placed = ["run.lift=true", "lift.place=true", "lift.ground=estimate", "lift.footlock=true"]
    assert lift_footlock_options(load_config(placed)) == (True, FOOTLOCK_DEFAULTS)
    assert lift_footlock_options(load_config(["run.lift=true", "lift.fuse=true", "lift.ground=estimate", "lift.footlock=true"]))[0] is True
    on, kw = lift_footlock_options(load_config(placed + ["lift.footlock_blend=0", "lift.footlock_stretch=0.9", "lift.footlock_floor=false"]))
    assert on and kw == dict(blend=0, stretch=0.9, floor=False) and type(kw["blend"]) is int
    with pytest.raises(SystemExit):
        load_config(["lift.footlocks=true"])
    off = ["run.lift=true", "lift.place=true", "lift.ground=estimate"]
    for argv, word in ((["run.lift=true", "lift.place=true", "lift.footlock=true"], "set lift.ground=estimate"), (["lift.footlock=true"], "set lift.ground=estimate"),
                       (["run.lift=true", "lift.footlock=true", "lift.ground=estimate"], "lift.fuse=true .* or lift.place=true"),
                       (off + ["lift.footlock=maybe"], "true or false"), (off + ["lift.footlock_blend=3"], "set lift.footlock=true"),
                       (off + ["lift.footlock_stretch=0.9"], "set lift.footlock=true"), (off + ["lift.footlock_floor=false"], "set lift.footlock=true"),
                       (placed + ["lift.footlock_blend=-1"], "0..32"), (placed + ["lift.footlock_blend=33"], "0..32"), (placed + ["lift.footlock_blend=2.5"], "0..32"),
                       (placed + ["lift.footlock_stretch=0"], r"\(0, 1\]"), (placed + ["lift.footlock_stretch=1.5"], r"\(0, 1\]"),
                       (placed + ["lift.footlock_stretch=abc"], r"\(0, 1\]"), (placed + ["lift.footlock_floor=2"], "true or false")):
        with pytest.raises(ValueError, match=word):
            run(["run.train=false", "run.test=false"] + argv)                    # (a run that got further would need a device)
    assert all(s in LIFT_SUFFIXES for s in ("__locked", "__lock_flags", "__lock_moved", "__lock_run", "__skate_locked", "__skate_pairs_locked"))


def test_the_footlock_report(tmp_path):
    from _entry import write_lift_footlock_report
    rows = [dict(key="a.fused0", frames=300, runs_r=4, runs_l=5, locked=331, clamped=2, moved_mean_mm=5.4321, moved_max_mm=25.1, skate_mm=8.8, skate_locked_mm=0.0),
            dict(key="b", frames=5, runs_r=0, runs_l=0, locked=0, clamped=0, moved_mean_mm=0.0, moved_max_mm=0.0, skate_mm=0.0, skate_locked_mm=0.0)]
    text = open(write_lift_footlock_report(str(tmp_path), rows)).read().splitlines()
    assert text[0] == "key,frames,runs_r,runs_l,locked,clamped,moved_mean_mm,moved_max_mm,skate_mm,skate_locked_mm"
    assert text[1] == "a.fused0,300,4,5,331,2,5.4321,25.1,8.8,0" and text[2] == "b,5,0,0,0,0,0,0,0,0" and len(text) == 3


def test_new_abi_symbol_is_declared_everywhere():
    from manipose_amd import _lib, lifting, lift_ops
    import manipose_amd
    header = open(_lib.HEADER_PATH).read()
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "mp_lift_footlock" in _lib.declared_symbols() and len(_lib._SIGNATURES["mp_lift_footlock"][1]) == 22
    assert "lib.mp_lift_footlock.argtypes = [vp, i64, i32, i32, vp, vp, i32, vp, C.POINTER(i32), i32, vp, vp, vp, i32, f32, " in integration
    assert int(re.search(r"#define MP_LIFT_FOOTLOCK_MAXBLEND (\d+)", header).group(1)) == lift_ops.FOOTLOCK_MAXBLEND == 32
    assert manipose_amd.lock_feet is lifting.lock_feet is lift_ops.lock_feet and "lock_feet" in lifting.__all__
    assert lifting.FootLock._fields == ("points", "run", "target", "moved", "flags", "runs", "skate", "skate_pairs")
    source = open(os.path.join(ROOT, "manipose_amd", "csrc", "lift_footlock.hip")).read()
    assert source.index("#pragma clang fp contract(off)") < source.index('#include "lift_geom.h"') and "atomicAdd" not in source
    for name in ("README.md", "DESIGN.md", os.path.join("tools", "README.md")):
        assert "mp_lift_footlock" in open(os.path.join(ROOT, name)).read(), name
    if os.path.exists(_lib.LIB_PATH):
        assert hasattr(_lib.load(), "mp_lift_footlock")

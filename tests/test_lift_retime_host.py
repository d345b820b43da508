"""mp_lift_fk and mp_lift_retime without a device: the properties of the float64 statements of their rules (lift_retime_ref.py), every condition
the device bounds of test_gpu_lift_retime.py stand on, the host side of the bindings (frame counts, argument errors), the config keys of
lift.retime_fps and the new symbols' declarations."""
import os
import re
import sys

import numpy as np
import pytest
import torch

import lift_retime_ref as ref
import lift_rot_ref as rot
import lift_smooth_ref as smooth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hpe"))
PAR, REST = rot.H36M_PARENTS, rot.H36M_REST


def _spin(n, J, axis, omega, phase=0.3):
    """(n, 1, J, 4): joint j turns about ``axis`` at (j + 1) omega radians a frame, from a common start orientation"""
    t = np.arange(n, dtype=np.float64)[:, None]
    ang = phase + (np.arange(J) + 1.0) * omega * t
    q0 = ref.unit(np.array([0.9, 0.1, -0.3, 0.2]))
    return ref.qmul(np.broadcast_to(q0, (n, J, 4)), ref.qexp(ang[..., None] * np.asarray(axis, np.float64)))[:, None]


def _run(q, root=None, valid=None, lens=None, num=1, den=1, start=0.0, R=0, degree=2, taper=0):
    lens = (q.shape[0],) if lens is None else lens
    off, oo, clock = ref.plan(lens, num, den, start)
    return ref.retime(q, root, valid, off, oo, clock, R, degree, taper), oo


def test_fk_is_the_inverse_of_the_rotations_statement():
    P, L = rot.rigid_h36m_poses(40)
    r = rot.ik(P[:, None], PAR, REST)
    # (float64 all the way: the statement takes float32 storage, so its matrices are applied directly)
    back = rot.fk_quat(r["quat"][:, 0], rot.measured_lengths(P, PAR), PAR, REST, P[:, 0])
    assert np.abs(back - P).max() < 5e-15 and r["ok"].all()
    q32 = r["quat"].astype(np.float32)
    mine, ok = ref.fk(q32, rot.measured_lengths(P, PAR)[:, None].astype(np.float32), PAR, REST, P[:, None, 0].astype(np.float32))
    theirs = rot.fk_quat(ref.unit(q32.astype(np.float64)), rot.measured_lengths(P, PAR).astype(np.float32).astype(np.float64)[:, None], PAR, REST,
                         P[:, None, 0].astype(np.float32).astype(np.float64))
    assert np.abs(mine - theirs).max() < 1e-14 and ok.all()             # the two float64 forward kinematics agree on the same float32 inputs
    assert np.abs(mine[:, 0] - P).max() < 2e-6                           # ... and give the poses back to the rounding of what they were given
    per_seq, ok = ref.fk(q32, np.stack([L, 2 * L]).astype(np.float32), PAR, REST, None, [0, 25, 40])
    bones = rot.measured_lengths(per_seq[:, 0], PAR)
    L32 = L.astype(np.float32).astype(np.float64)
    assert np.abs(bones[:25] - L32).max() < 1e-15 and np.abs(bones[25:] - 2 * L32).max() < 1e-15 and not per_seq[:, 0, 0].any()
    bad = q32.copy()
    bad[3, 0, 5] = 0
    bad[4, 0, 0, 1] = np.inf
    out, ok = ref.fk(bad, L[None].astype(np.float32), PAR, REST, P[:, None, 0].astype(np.float32), [0, 40])
    assert ok[:, 0].tolist() == [1, 1, 1, 0, 0] + [1] * 35 and all(np.array_equal(out[k, 0], np.tile(P[k, 0].astype(np.float32), (17, 1))) for k in (3, 4))


def test_identity_clock_and_constant_angular_velocity():
    sc = ref.take("h36m", 2, (5, 9), "single", seed=1)
    got, oo = _run(sc["quat"], sc["root"], sc["valid"], (5, 9))
    assert np.array_equal(got["quat"], sc["quat"].astype(np.float64)) and np.array_equal(got["root"], sc["root"].astype(np.float64))
    assert np.array_equal(got["ok"], sc["valid"]) and (got["taps"] == 1).all() and got["copied"].all() and oo.tolist() == [0, 5, 14]
    axis = ref.unit(np.array([0.3, -0.5, 0.8]))
    n, J = 40, 4
    w = 0.005                                                             # joint 3 turns 0.8 rad over the take: every relative rotation of a window far from pi
    exact = _spin(n, J, axis, w)                                          # float64 input through the float64 statement: the property itself
    for num, den, start in ((3, 5, 0.0), (6, 5, 0.25), (7, 3, 0.0)):
        for degree in (1, 2):
            for R, taper in ((2, 0), (4, 1), (64, 0)):
                off, oo, clock = ref.plan((n,), num, den, start)
                got = _retime64(exact, off, oo, clock, R, degree, taper)
                t = got["time"]
                want = ref.qmul(exact[0, 0][None], ref.qexp(((np.arange(J) + 1.0) * w * t[:, None])[..., None] * axis))
                err = np.abs(np.abs((got["quat"][:, 0] * want).sum(-1)) - 1.0).max()
                assert np.abs(got["quat"][:, 0] - want).max() < 1e-14 and err < 1e-14, (num, den, start, degree, R, taper)


def _retime64(q64, off, oo, clock, R, degree, taper):
    """the statement on float64 input: for the properties that hold in exact arithmetic"""
    return ref.retime(q64, None, None, off, oo, clock, R, degree, taper, storage=np.float64)


def test_two_taps_of_degree_one_are_the_slerp_and_the_root_is_lift_smooths():
    sc = ref.take("h36m", 1, (12,), "none", seed=2)
    valid = np.zeros((12, 1), np.uint8)
    valid[[4, 5]] = 1                                                     # two taps: frames 4 and 5
    for R in (1, 3):
        fit, _ = _run(sc["quat"], sc["root"], valid, (12,), 4, 1, 0.0, R, 1, 0)
        lerp, _ = _run(sc["quat"], sc["root"], valid, (12,), 4, 1, 0.0, 0, 2, 0)
        between = slice(17, 20)                                           # t = 4.25, 4.5, 4.75
        assert (fit["taps"][between] == 2).all() and (lerp["taps"][between] == 2).all()
        assert np.abs(fit["quat"][between] - lerp["quat"][between]).max() < 1e-14 and np.abs(fit["root"][between] - lerp["root"][between]).max() < 1e-14
    # at integer t the root's sum is mp_lift_smooth's: the same taps, weights and normal matrix
    sc = ref.take("h36m", 2, (30, 11), "single", seed=4)
    for R, degree, taper in ((4, 2, "uniform"), (3, 1, "biweight"), (9, 0, "uniform")):
        got, _ = _run(sc["quat"], sc["root"], sc["valid"], (30, 11), 1, 1, 0.0, R, degree, smooth.TAPER[taper])
        want, filled = smooth.smooth_all(sc["root"][:, :, None], sc["valid"], [0, 30, 41], R, degree, taper)
        assert np.array_equal(got["ok"], filled) and np.abs(got["root"] - want[:, :, 0])[filled != 0].max() < 1e-13


def test_bones_stay_on_the_table_where_interpolated_positions_shrink():
    """Two frames of one bone theta apart: the midpoint of the POSITIONS is shorter by 1 - cos(theta / 2), the midpoint on SO(3) is not"""
    par, rest = (-1, 0), np.array([(0, 0, 0), (1.0, 0, 0)], np.float32)
    for deg in (10.0, 20.0):
        th = np.deg2rad(deg)
        q = np.zeros((2, 1, 2, 4))
        q[:, :, :, 0] = 1
        q[1, 0, 1] = [np.cos(th / 2), 0, 0, np.sin(th / 2)]
        off, oo, clock = ref.plan((2,), 2, 1)
        mid = _retime64(q, off, oo, clock, 0, 2, 0)["quat"][1:2]
        L = np.array([[0.45]])
        ends = rot.fk_quat(q[:, 0], L, par, rest)
        on_so3 = rot.fk_quat(mid[:, 0], L, par, rest)
        lin = 0.5 * (ends[0] + ends[1])
        assert abs(np.linalg.norm(on_so3[0, 1]) - 0.45) < 1e-15
        assert abs((0.45 - np.linalg.norm(lin[1])) - 0.45 * (1 - np.cos(th / 2))) < 1e-15
        print(f"\n[{deg:.0f} degrees a frame] a 0.45 m bone at the midpoint: positions {1000 * (0.45 - np.linalg.norm(lin[1])):.2f} mm short, rotations 0")
    sc = ref.take("h36m", 1, (67,), "single", seed=6)
    table = np.random.default_rng(0).uniform(0.1, 0.5, (1, 16)).astype(np.float32)
    for R in (0, 4):
        got, oo = _run(sc["quat"], sc["root"], sc["valid"], (67,), 6, 5, 0.25, R, 2, 1)
        live = (got["ok"][:, 0] & 1) != 0
        p = rot.fk_quat(got["quat"][:, 0], table.astype(np.float64), PAR, REST, got["root"][:, 0])
        assert np.abs(rot.measured_lengths(p[live], PAR) - table).max() < 1e-15 and live.sum() > 40


def test_sign_continuity_and_frame_counts():
    from manipose_amd import lift_args
    for case in ("h36m-i5-single-3by5-s0.0-R4-d2-t1", "h36m-i1-none-6by5-s0.25-R0-d2-t0", "chain-i1-none-2by1-s0.0-R4-d2-t0"):
        sc, (off, oo, clock), want = ref.solved(case)
        q_in = sc["quat"].astype(np.float64)
        f0 = 0
        for s, n in enumerate(sc["lens"]):
            assert ((q_in[f0 + 1:f0 + n] * q_in[f0:f0 + n - 1]).sum(-1) > 0).all()       # the input is sign-continuous ...
            seg, ok = want["quat"][int(oo[s]):int(oo[s + 1])], (want["ok"][int(oo[s]):int(oo[s + 1])] & 1) != 0
            both = ok[1:] & ok[:-1]
            assert ((seg[1:] * seg[:-1]).sum(-1)[both] > 0).all()                         # ... and so is the output, wherever two frames in a row have a result
            f0 += n
    for n in (1, 2, 3, 67, 130):
        for num, den in ref.RATES:
            for start in (0.0, 0.25, 0.5):
                if start > n - 1:
                    with pytest.raises(ValueError, match="past the last frame"):
                        lift_args.retime_plan(None, n, den, num, start)
                    assert ref.frame_count(n, num, den, start) == 0
                    continue
                off, oo, clock, time = lift_args.retime_plan(None, n, den, num, start)
                M = int(oo[1])
                assert M == ref.frame_count(n, num, den, start) == len(time) and clock.tolist() == [[start, float(num), float(den)]]
                assert time[-1] <= n - 1 < start + (M * den) / num and time[0] == start      # the last sample is inside, one more would pass the last frame
                if start == 0:
                    assert M == ((n - 1) * num) // den + 1
    off, oo, clock, time = lift_args.retime_plan([0, 5, 12], 12, 50, 30, [0.0, 1.5])
    assert oo.tolist() == [0, 3, 6] and time.tolist() == [0.0, 50 / 30, 100 / 30, 1.5, 1.5 + 50 / 30, 1.5 + 100 / 30]


def test_the_recovery_scene_in_the_statement():
    """A smooth synthetic motion, rotation noise of 3 degrees a joint, 10 % of the frames invalid, retimed 50 -> 30 with radius 4 (biweight, degree
    2): the fit's mean geodesic error against the true motion at the sampled times is below the noisy input's at its own frames.  The ordering is
    what is asserted; the figures are printed (DESIGN.md section 5 records them)."""
    g = np.random.default_rng(11)
    n, J = 300, 17
    true_q = ref.smooth_tracks(g, n, 1, J, speed=0.03, wobble=0.3)
    noise = ref.qexp(np.deg2rad(3.0) / np.sqrt(3.0) * g.standard_normal((n, 1, J, 3)))
    noisy = ref.qmul(true_q, noise).astype(np.float32)
    valid = (g.uniform(size=(n, 1)) > 0.1).astype(np.uint8)
    off, oo, clock = ref.plan((n,), 30, 50)
    got = ref.retime(noisy, None, valid, off, oo, clock, 4, 2, 1)
    t = got["time"]
    lo = np.floor(t).astype(int)
    hi = np.minimum(lo + 1, n - 1)
    # the truth at fractional times: the short-way slerp of the true frames around t (the motion turns by at most 2.3 degrees a frame and joint)
    al = (t - lo)[:, None, None, None]
    a, b = true_q[lo], true_q[hi]
    m = dict(dot=np.inf, angle=0.0)
    truth = ref.qmul(a, ref.qexp(al * ref.aligned_log(a, b, m)))
    assert (got["ok"] & 1).all()
    fit_err = np.rad2deg(ref.geodesic(got["quat"], truth)).mean()
    in_err = np.rad2deg(ref.geodesic(ref.unit(noisy.astype(np.float64)), true_q))[valid[:, 0] != 0].mean()
    print(f"\n[recovery] mean geodesic error: the noisy input {in_err:.3f} degrees at its {int(valid.sum())} valid frames of {n}, the retimed fit "
          f"(50 -> 30 fps, radius 4, degree 2, biweight) {fit_err:.3f} degrees at {len(t)} sampled times")
    assert fit_err < in_err


def test_every_condition_the_device_bounds_stand_on():
    lens, inners, kinds, rates, starts, radii, degrees, tapers, holes = (set() for _ in range(9))
    worst = dict(dot=np.inf, angle=0.0, window=np.inf)
    for cid, kind, inner, hole, rate, start, R, degree, taper in ref.cases():
        sc, (off, oo, clock), want = ref.solved(cid)
        m = want["margins"]
        worst = dict(dot=min(worst["dot"], m["dot"]), angle=max(worst["angle"], m["angle"]), window=min(worst["window"], m["window"]))
        assert m["dot"] >= 1e-6 and m["angle"] <= np.pi - 1e-3 and m["window"] >= 1e-6, cid
        # t is exact binary arithmetic on both sides; its decisions (floor, nearest tap, bracketing) are either exact ties or far from a tie
        frac = want["time"] - np.floor(want["time"])
        assert ((frac == 0) | ((frac >= 1e-6) & (frac <= 1 - 1e-6))).all() and ((frac == 0.5) | (np.abs(frac - 0.5) >= 1e-6)).all(), cid
        assert sc["lens"] == ref.LENS and np.array_equal(lift_plan(sc["lens"], rate, start), oo)
        made = ~want["copied"]                                            # (a copied frame keeps its bits, off the unit sphere as the scene stores it)
        assert not made.any() or np.abs(np.sqrt((want["quat"][made] ** 2).sum(-1)) - 1).max() < 1e-12
        lens.update(sc["lens"]); inners.add(inner); kinds.add(kind); rates.add(rate); starts.add(start); radii.add(R); degrees.add(degree)
        tapers.add(taper); holes.add(hole)
        if hole == "run" and R <= 4:
            assert (want["ok"] & 1 == 0).any()
        if hole == "none":
            assert (want["ok"] & 1 == 1).all()
        assert (want["ok"] & 2 == 0).all()                                # the host's frame counts never need the clamp
    print(f"\n[margins over the cases] |dot| >= {worst['dot']:.3f}, relative rotation <= {worst['angle']:.3f} rad, | |k - t| - R | >= {worst['window']:.3f} or 0")
    assert lens == set(ref.LENS) and inners == {1, 5} and kinds == {"h36m", "pair", "chain"} and rates == set(ref.RATES) and starts == {0.0, 0.25}
    assert radii == {0, 1, 4, 64} and degrees == {0, 1, 2} and tapers == {0, 1} and holes == {"none", "single", "run"}


def lift_plan(lens, rate, start):
    from manipose_amd import lift_args
    off = np.concatenate([[0], np.cumsum(lens)])
    return lift_args.retime_plan(off, int(off[-1]), rate[1], rate[0], ref.starts(lens, start))[1]


def test_argument_errors_are_value_errors_before_any_device_work():
    """The calls are given CPU tensors: had the arguments been accepted, they would have ended in the RuntimeError that refuses them ("no CPU
    fallback"), which is what the valid calls at the end do."""
    from manipose_amd import pose_from_rotations, retime_rotations, smooth_rotations
    z = torch.zeros
    q, r, v = z(12, 17, 4), z(12, 3), torch.ones(12, dtype=torch.uint8)
    for kw, word in ((dict(quat=z(12, 17)), "quat must be"), (dict(quat=q.double()), "quat must be"), (dict(quat=np.zeros((12, 17, 4))), "quat must be"),
                     (dict(quat=z(12, 1, 4)), "joints"), (dict(quat=z(12, 33, 4)), "joints"), (dict(quat=z(12, 4, 17).transpose(1, 2)), "quat must be"),
                     (dict(quat=z(0, 17, 4)), "no frame"), (dict(root=z(12, 4)), "root must be"), (dict(root=z(11, 3)), "root must be"), (dict(root=r.double()), "root must be"),
                     (dict(valid=v[:5]), "valid must be"), (dict(valid=v.bool()), "valid must be"), (dict(seq_offset=[0]), "seq_offset"),
                     (dict(seq_offset=[0, 13]), "seq_offset"), (dict(seq_offset=[0, 5, 5, 12]), "seq_offset"), (dict(seq_offset=[0.0, 12.0]), "seq_offset"),
                     (dict(fps_in=0), "fps_in"), (dict(fps_in=2.0), "fps_in"), (dict(fps_out=-3), "fps_out"), (dict(fps_out=True), "fps_out"),
                     (dict(start=-0.5), "start"), (dict(start=float("nan")), "start"), (dict(start=[0.0, 1.0]), "start"), (dict(start="0"), "start"),
                     (dict(start=11.5), "past the last frame"), (dict(seq_offset=[0, 3, 12], start=[0.0, 9.0]), "past the last frame"),
                     (dict(radius=-1), "radius"), (dict(radius=65), "radius"), (dict(radius=2.0), "radius"), (dict(degree=3), "degree"), (dict(degree=-1), "degree"),
                     (dict(taper="gauss"), "taper"), (dict(taper=0), "taper")):
        with pytest.raises(ValueError, match=word):
            retime_rotations(**dict(dict(quat=q, root=r, valid=v), **kw))
    with pytest.raises(ValueError, match="radius must be an integer in 1..64"):
        smooth_rotations(q, radius=0)
    for kw in (dict(), dict(fps_in=50, fps_out=30, radius=4, taper="biweight"), dict(quat=z(12, 5, 2, 4), root=None, valid=None, seq_offset=[0, 5, 12], start=[0.0, 0.5]),
               dict(seq_offset=torch.tensor([0, 12]), radius=64, degree=0)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            retime_rotations(**dict(dict(quat=q, root=r, valid=v), **kw))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        smooth_rotations(q, r, v)
    b = np.full(16, 0.5, np.float32)
    for kw, word in ((dict(quat=z(12, 17, 3)), "quat must be"), (dict(quat=z(12, 5, 4)), "default skeleton"), (dict(bones=np.full(15, 0.5)), "bones must be"),
                     (dict(bones=np.full((2, 16), 0.5)), "bones must be"), (dict(bones=-b), "non-negative"), (dict(bones=b * np.nan), "finite"),
                     (dict(bones=z(12, 16).double()), "bones"), (dict(root=z(12, 2)), "root must be"), (dict(seq_offset=[0]), "seq_offset"),
                     (dict(seq_offset=list(range(14))), "seq_offset"), (dict(quat=z(12, 2, 4), skeleton=rot.Sk((-1, 0), np.zeros((2, 3)))), "T-pose direction")):
        with pytest.raises(ValueError, match=word):
            pose_from_rotations(**dict(dict(quat=q, bones=b), **kw))
    for kw in (dict(), dict(root=r, bones=np.full((2, 16), 0.5), seq_offset=[0, 5, 12]), dict(bones=z(12, 16)), dict(quat=z(12, 3, 17, 4), bones=z(12, 3, 16), root=z(12, 3, 3)),
               dict(quat=z(12, 2, 4), bones=[0.5], skeleton=rot.Sk(*rot.skeleton("pair")))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            pose_from_rotations(**dict(dict(quat=q, bones=b), **kw))


def test_config_keys_parse_and_the_refusals_fire():
    from _entry import LIFT_SUFFIXES, RETIME_DEFAULTS, lift_retime_options, load_config, run
    cfg = load_config([])
    assert cfg.lift.retime_fps == 0 and lift_retime_options(cfg) == (False, RETIME_DEFAULTS)
    assert RETIME_DEFAULTS == dict(from_fps=0, radius=0, degree=2, taper="uniform")
    base = ["run.lift=true", "lift.rigid=true", "lift.rotations=true"]
    assert lift_retime_options(load_config(base + ["lift.retime_fps=30"])) == (True, dict(fps_in=50, fps_out=30, radius=0, degree=2, taper="uniform"))
    on, kw = lift_retime_options(load_config(base + ["lift.retime_fps=50", "lift.retime_from_fps=25", "lift.retime_radius=4", "lift.retime_degree=1",
                                                     "lift.retime_taper=biweight"]))
    assert on and kw == dict(fps_in=25, fps_out=50, radius=4, degree=1, taper="biweight") and type(kw["fps_out"]) is int
    with pytest.raises(SystemExit):
        load_config(["lift.retime=30"])
    for argv, word in ((["lift.retime_fps=30", "lift.rigid=true", "lift.rotations=true"], "set run.lift=true"),
                       (["run.lift=true", "lift.rigid=true", "lift.retime_fps=30"], "set lift.rotations=true"),
                       (["run.lift=true", "lift.rotations=true", "lift.retime_fps=30"], "set lift.rigid=true"),
                       (base + ["lift.retime_radius=4"], "set lift.retime_fps"), (base + ["lift.retime_from_fps=25"], "set lift.retime_fps"),
                       (base + ["lift.retime_degree=1"], "set lift.retime_fps"), (base + ["lift.retime_taper=biweight"], "set lift.retime_fps"),
                       (base + ["lift.retime_fps=-1"], "output frame rate"), (base + ["lift.retime_fps=29.97"], "output frame rate"),
                       (base + ["lift.retime_fps=true"], "output frame rate"), (base + ["lift.retime_fps=30", "lift.retime_from_fps=-5"], "input frame rate"),
                       (base + ["lift.retime_fps=30", "lift.retime_radius=65"], "0..64"), (base + ["lift.retime_fps=30", "lift.retime_degree=3"], "0, 1 or 2"),
                       (base + ["lift.retime_fps=30", "lift.retime_taper=gauss"], "uniform or biweight"),
                       (base + ["lift.retime_fps=30", "data.dataset=3dhp"], "set lift.retime_from_fps")):
        with pytest.raises(ValueError, match=word):
            run(["run.train=false", "run.test=false"] + argv)                    # (a run that got further would need a device)
    assert all(s in LIFT_SUFFIXES for s in ("__rt", "__rt_quat", "__rt_root", "__rt_ok", "__rt_taps", "__rt_time", "__rt_fps"))


def test_new_abi_symbols_are_declared_everywhere():
    from manipose_amd import _lib, lifting, lift_ops
    import manipose_amd
    header = open(_lib.HEADER_PATH).read()
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "mp_lift_fk" in _lib.declared_symbols() and len(_lib._SIGNATURES["mp_lift_fk"][1]) == 14
    assert "mp_lift_retime" in _lib.declared_symbols() and len(_lib._SIGNATURES["mp_lift_retime"][1]) == 19
    assert "lib.mp_lift_fk.argtypes = [vp, vp, vp, i64, i32, i32, vp, i32, C.POINTER(i32), C.POINTER(f32), i32, vp, vp, vp]" in integration
    assert "lib.mp_lift_retime.argtypes = [vp, vp, vp, i64, i32, i32, vp, vp, vp, i32, i64, i32, i32, i32, vp, vp, vp, vp, vp]" in integration
    assert int(re.search(r"#define MP_LIFT_FK_POSE_LENGTHS (\d+)", header).group(1)) == lift_ops.FK_POSE_LENGTHS == 1
    for name in ("pose_from_rotations", "retime_rotations", "smooth_rotations"):
        assert getattr(manipose_amd, name) is getattr(lifting, name) is getattr(lift_ops, name) and name in lifting.__all__
    assert lifting.Retimed._fields == ("quat", "root", "ok", "taps", "seq_offset", "time")
    for src in ("lift_fk.hip", "lift_retime.hip"):
        source = open(os.path.join(ROOT, "manipose_amd", "csrc", src)).read()
        assert "atomicAdd" not in source and "__shared__" not in source
    for name in ("README.md", "DESIGN.md", os.path.join("tools", "README.md")):
        text = open(os.path.join(ROOT, name)).read()
        assert "mp_lift_retime" in text and "mp_lift_fk" in text, name
    if os.path.exists(_lib.LIB_PATH):
        lib = _lib.load()
        assert hasattr(lib, "mp_lift_fk") and hasattr(lib, "mp_lift_retime")

"""Standing a take on its floor, without a device: the float64 statement of mp_lift_ground's rule (lift_ground_ref.py) recovers the scenes it is
for, every condition the device bounds of test_gpu_lift_ground.py stand on holds for every compared row, the degenerate scenes come out as the
header says, the argument errors and the entry point's option combinations carry their messages, and the new ABI entry is declared everywhere."""
import os
import re
import sys

import numpy as np
import pytest
import torch

import lift_ground_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hpe"))


def test_the_statement_recovers_a_clean_walker():
    """no noise: the plane through the stance ankles, to the float32 rounding of the coordinates (a few metres: 2.4e-7 m an ulp)"""
    sc = ref.walker(3, 300)
    got = ref.ground(sc["points"])
    rms, angle = ref.recovery_error(sc, got["normal"][0], got["offset"][0])
    print(f"clean walker: plane off by {rms:.2e} m, {angle:.2e} degrees; rms {got['rms'][0]:.2e}, gap {got['gap'][0]:.3f}, skate {got['skate'][0]:.2e}")
    assert got["ok"][0] == 3 and rms < 2e-5 and angle < 5e-3 and got["rms"][0] < 2e-5 and got["skate"][0] == 0      # (the prior's pull: the body leans a little)
    free = ref.ground(sc["points"], prior=0.0)
    rms0, angle0 = ref.recovery_error(sc, free["normal"][0], free["offset"][0])
    print(f"... with prior = 0: {rms0:.2e} m, {angle0:.2e} degrees; rms {free['rms'][0]:.2e}")
    assert free["ok"][0] == 3 and rms0 < 1e-6 and angle0 < 1e-4 and free["rms"][0] < 1e-6
    assert got["used"][0] == got["contact"].sum() > 300 and got["skate_pairs"][0] > 250
    assert not got["contact"][~sc["stance"]].any()                        # no swing frame passes for a contact ...
    inner = sc["stance"][:-4] & sc["stance"][4:] & sc["stance"][2:-2]
    assert got["contact"][2:-2][inner].all()                              # ... and every frame whose +- 2 neighbours stand still is one
    assert not got["contact"][:2].any() and not got["contact"][-2:].any()
    # the returned rotation and shift stand the scene up: the stance ankles at z = foot_height, the thorax above
    up = ref.ground(sc["points"], foot_height=0.08)
    stood = ref.qrot(up["quat"][0], sc["truth"][sc["stance"]]) + up["trans"][0]
    assert np.abs(stood[:, 2] - np.float32(0.08)).max() < 3e-5            # (the prior's pull again; 1.2e-5 m)
    assert (ref.qrot(up["quat"][0], sc["points"][:, 8].astype(np.float64)) + up["trans"][0])[:, 2].min() > 1.0
    assert np.allclose(ref.qrot(up["quat"][0], up["normal"][0]), [0, 0, 1], atol=1e-12) and up["quat"][0, 3] == 0 and up["quat"][0, 0] > 0


@pytest.mark.parametrize("seed", ref.RECOVERY_SEEDS)
def test_the_statement_recovers_the_scene_the_feature_is_for(seed):
    """300 frames, 5 mm of noise, 10 % hover frames: RECOVERY_BOUND is twice the worst of these seeds (lift_ground_ref.py has the figures)"""
    sc = ref.recovery_scene(seed)
    got = ref.ground(sc["points"])
    plain = ref.ground(sc["points"], iters=0)
    rms, angle = ref.recovery_error(sc, got["normal"][0], got["offset"][0])
    rms0, angle0 = ref.recovery_error(sc, plain["normal"][0], plain["offset"][0])
    print(f"seed {seed}: robust {1000 * rms:.3f} mm {angle:.3f} deg; plain squares {1000 * rms0:.3f} mm {angle0:.3f} deg; gap {got['gap'][0]:.3f}")
    assert got["ok"][0] == 3 and rms <= ref.RECOVERY_BOUND["rms_m"] / 2 * 1.001 and angle <= ref.RECOVERY_BOUND["angle_deg"] / 2 * 1.001
    assert rms0 > 3 * rms                                                 # the hover frames pull the plain fit up: the robust weight sheds them
    hover = got["contact"][:, 1].astype(bool) & ~sc["stance"][:, 1]
    assert hover.sum() >= 20 and (got["height"][hover, 1] > 0.1).sum() >= 20      # ... they are contacts, 0.15 m over the plane


def test_every_condition_the_device_bounds_stand_on():
    for tag, inp, want in ref.cases():
        has = (want["ok"] & 1).astype(bool)
        assert want["speed_margin"] >= ref.SPEED_MARGIN, (tag, want["speed_margin"])
        assert has[2:].all() and not has[0], tag                          # the sequences of 64, 257 and 300 frames have a plane, one frame has none
        e = want["eig"]
        assert (e[has, 1] - e[has, 0] >= ref.GAP_MIN * (e[has, 2] - e[has, 0])).all() and (want["gap"][has] >= ref.GAP_MIN).all(), (tag, want["gap"])
        flat = ~has & (want["used"] >= 3)
        assert (e[flat, 1] - e[flat, 0] <= ref.FLAT_MAX * np.maximum(np.abs(e[flat, 0]), np.abs(e[flat, 2]))).all(), tag
        assert (want["side"][has] >= ref.SIDE_MIN).all() and (want["ok"][has] == 3).all(), tag
        kappa = ref.amplification(inp, want)
        budget = 0.25 * 2.0 ** -23 / (4.0 * ref.sum_error(want))
        print(f"[{tag}] used {want['used'].tolist()}, gap {np.round(want['gap'], 4).tolist()}, amplification {kappa:.3g} (allowed {budget:.3g})")
        assert kappa <= budget, tag
        assert np.isfinite(np.concatenate([want[k].ravel() for k in ref.FLOATS])).all()
    lens = np.diff(ref.cases()[0][1]["off"]).tolist()
    assert lens == list(ref.SEQ_LENS) and 1 in lens and 257 in lens and max(lens) == 300
    used = np.array([c[2]["used"] for c in ref.cases()])
    assert (used[:, 0] == 0).all() and (used[:, 3:] > 100).all() and ref.cases()[0][2]["skate_pairs"][4] > 50


def test_degenerate_scenes():
    still = ref.walker(5, 120, still=True)                                # nobody walks: two ankles in place span a line
    none, prior = ref.ground(still["points"], prior=0.0), ref.ground(still["points"])
    assert none["ok"][0] == 0 and none["used"][0] == 2 * 116 and none["normal"][0].tolist() == [0, 0, 1] and none["quat"][0].tolist() == [1, 0, 0, 0]
    assert not none["offset"].any() and not none["rms"].any() and not none["gap"].any() and not none["height"].any() and not none["trans"].any()
    assert none["skate_pairs"][0] == 2 * 115 and none["skate"][0] == 0
    rms, angle = ref.recovery_error(still, prior["normal"][0], prior["offset"][0])
    print(f"stand-still, default prior: {angle:.3f} degrees, {1000 * rms:.3f} mm, gap {prior['gap'][0]:.4f}")
    assert prior["ok"][0] == 3 and angle < 1.5 and rms < 0.005            # the plane perpendicular to the mean body axis, which sways by 1.5 degrees
    noisy = ref.recovery_scene(0, still=True, hover=0.0)                  # with noise the data alone choose a plane through the line at random
    a0 = ref.recovery_error(noisy, *(ref.ground(noisy["points"], prior=0.0)[k][0] for k in ("normal", "offset")))[1]
    a1 = ref.recovery_error(noisy, *(ref.ground(noisy["points"])[k][0] for k in ("normal", "offset")))[1]
    print(f"stand-still, 5 mm of noise: {a1:.3f} degrees with the default prior, {a0:.3f} with prior = 0")
    assert a1 < 0.5 and a0 > 5 * a1
    # no axis (both of its joints are one point): the first non-zero component of the normal is positive, bit 1 clear
    flat = ref.ground(ref.walker(6, 120)["points"][:, [0, 0, 0, 3, 0, 0, 6, 0, 0]], axis=(0, 8))
    assert flat["ok"][0] == 1 and flat["normal"][0][np.nonzero(flat["normal"][0])[0][0]] > 0
    few = ref.ground(ref.walker(7, 5)["points"])                          # one frame with a speed, two feet: two points are no plane
    assert few["ok"][0] == 0 and few["used"][0] <= 2
    gone = ref.ground(still["points"], valid=np.zeros(120, np.uint8))
    assert gone["ok"][0] == 0 and not gone["contact"].any() and gone["used"][0] == 0 and gone["skate_pairs"][0] == 0


def test_constructed_rows_in_the_statement():
    flat = ref.ground(ref.dyadic_scene())
    assert flat["normal"][0].tolist() == [0, 0, 1] and flat["quat"][0].tolist() == [1, 0, 0, 0] and flat["ok"][0] == 3
    assert not flat["offset"].any() and not flat["rms"].any() and not flat["height"].any() and not flat["skate"].any()
    turned = ref.ground(ref.dyadic_scene(flip=True))
    assert turned["normal"][0].tolist() == [0, 0, -1] and turned["quat"][0].tolist() == [0, 1, 0, 0] and turned["ok"][0] == 3
    slide = ref.ground(ref.dyadic_scene(slide=2.0 ** -8), feet=(3,))
    assert slide["skate"][0] == 2.0 ** -8 and slide["skate_pairs"][0] == 48 - 4 - 1 and slide["normal"][0].tolist() == [0, 0, 1]


def test_argument_errors_are_value_errors_before_any_device_work():
    """The calls are given CPU tensors: had the arguments been accepted, they would have ended in the RuntimeError that refuses them ("no CPU
    fallback"), which is what the valid calls at the end do."""
    from manipose_amd import estimate_ground
    pts, valid = torch.zeros(12, 17, 3), torch.ones(12, dtype=torch.uint8)
    for kw, word in ((dict(points=torch.zeros(12, 17)), "points must be"), (dict(points=pts.double()), "points must be"), (dict(points=np.zeros((12, 17, 3))), "points must be"),
                     (dict(points=torch.zeros(12, 17, 2)), "points must be"), (dict(points=torch.zeros(12, 1, 3)), "joints"), (dict(points=torch.zeros(12, 33, 3)), "joints"),
                     (dict(points=torch.zeros(12, 3, 17).transpose(1, 2)), "points must be"), (dict(points=torch.zeros(0, 17, 3)), "no frame"),
                     (dict(valid=valid[:5]), "valid must be"), (dict(valid=valid.bool()), "valid must be"), (dict(seq_offset=[0]), "seq_offset"),
                     (dict(seq_offset=list(range(14))), "seq_offset"), (dict(feet=()), "feet must be"), (dict(feet=(1, 2, 3, 4, 5)), "feet must be"),
                     (dict(feet=(3, 17)), "feet must be"), (dict(feet=(-1,)), "feet must be"), (dict(feet=(3.0, 6)), "feet must be"), (dict(feet=3), "sequences of joint"),
                     (dict(axis=(0, 0)), "axis must be"), (dict(axis=(0, 17)), "axis must be"), (dict(axis=(0,)), "axis must be"), (dict(axis=(0, 8, 9)), "axis must be"),
                     (dict(radius=0), "radius"), (dict(radius=9), "radius"), (dict(radius=2.0), "radius"), (dict(radius=True), "radius"),
                     (dict(iters=-1), "iters"), (dict(iters=9), "iters"), (dict(iters=1.0), "iters"), (dict(speed=0), "speed"), (dict(speed=-0.01), "speed"),
                     (dict(speed=float("inf")), "speed"), (dict(speed=float("nan")), "speed"), (dict(speed=1e-60), "speed"), (dict(speed="a"), "speed"),
                     (dict(sigma=0), "sigma"), (dict(sigma=-1.0), "sigma"), (dict(sigma=float("nan")), "sigma"), (dict(sigma=True), "sigma"),
                     (dict(prior=-0.1), "prior"), (dict(prior=float("inf")), "prior"), (dict(prior=float("nan")), "prior"), (dict(prior=None), "prior"),
                     (dict(foot_height=float("inf")), "foot_height"), (dict(foot_height=float("nan")), "foot_height"), (dict(foot_height="0"), "foot_height")):
        with pytest.raises(ValueError, match=word):
            estimate_ground(**dict(dict(points=pts), **kw))
    for kw in (dict(), dict(valid=valid, sigma=float("inf"), prior=0, iters=0, radius=8, foot_height=-0.1), dict(seq_offset=[0, 5, 12], feet=(3,), axis=(8, 0)),
               dict(points=torch.zeros(12, 5, 4), feet=(3, 4, 1, 2), axis=(0, 1), seq_offset=torch.tensor([0, 12]))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            estimate_ground(**dict(dict(points=pts), **kw))


def test_config_keys_parse_and_a_ground_without_absolute_positions_fails():
    from _entry import GROUND_DEFAULTS, LIFT_SUFFIXES, lift_ground_options, load_config, run
    cfg = load_config([])
    assert cfg.lift.ground == "none" and lift_ground_options(cfg) == (False, GROUND_DEFAULTS)
    assert GROUND_DEFAULTS == dict(speed=0.01, radius=2, sigma=0.03, prior=0.05, iters=5, foot_height=0.0)
    fused, placed = ["run.lift=true", "lift.fuse=true", "lift.ground=estimate"], ["run.lift=true", "lift.place=true", "lift.ground=estimate"]
    assert lift_ground_options(load_config(fused)) == (True, GROUND_DEFAULTS) == lift_ground_options(load_config(placed))
    on, kw = lift_ground_options(load_config(placed + ["lift.ground_speed=0.02", "lift.ground_radius=3", "lift.ground_sigma=.inf", "lift.ground_prior=0",
                                                       "lift.ground_iters=0", "lift.ground_foot_height=0.09"]))
    assert on and kw == dict(speed=0.02, radius=3, sigma=float("inf"), prior=0.0, iters=0, foot_height=0.09) and type(kw["radius"]) is int
    assert lift_ground_options(load_config(["run.lift=true", "lift.place=true", "lift.ground=none"]))[0] is False
    with pytest.raises(SystemExit):
        load_config(["lift.grounds=estimate"])
    off = ["run.lift=true", "lift.place=true"]
    for argv, word in ((off + ["lift.ground=guess"], "none or estimate"), (["run.lift=true", "lift.ground=estimate"], "lift.fuse=true .* or lift.place=true"),
                       (["run.lift=true", "lift.frame=world", "lift.ground=estimate"], "lift.fuse=true .* or lift.place=true"),
                       (["lift.place=true", "lift.ground=estimate"], "set run.lift=true"), (off + ["lift.ground_speed=0.02"], "set lift.ground=estimate"),
                       (off + ["lift.ground_radius=3"], "set lift.ground=estimate"), (off + ["lift.ground_sigma=0.1"], "set lift.ground=estimate"),
                       (off + ["lift.ground_prior=0"], "set lift.ground=estimate"), (off + ["lift.ground_iters=2"], "set lift.ground=estimate"),
                       (off + ["lift.ground_foot_height=0.1"], "set lift.ground=estimate"), (placed + ["lift.ground_radius=0"], "1..8"),
                       (placed + ["lift.ground_radius=9"], "1..8"), (placed + ["lift.ground_radius=1.5"], "1..8"), (placed + ["lift.ground_iters=9"], "0..8"),
                       (placed + ["lift.ground_iters=-1"], "0..8"), (placed + ["lift.ground_speed=0"], "finite and > 0"),
                       (placed + ["lift.ground_speed=.inf"], "finite and > 0"), (placed + ["lift.ground_speed=abc"], "finite and > 0"),
                       (placed + ["lift.ground_sigma=0"], "> 0"), (placed + ["lift.ground_sigma=abc"], "is a number"), (placed + ["lift.ground_prior=-1"], "finite and >= 0"),
                       (placed + ["lift.ground_prior=.inf"], "finite and >= 0"), (placed + ["lift.ground_foot_height=.inf"], "must be finite")):
        with pytest.raises(ValueError, match=word):
            run(["run.train=false", "run.test=false"] + argv)                    # (a run that got further would need a device)
    for s in ("normal", "offset", "quat", "trans", "rms", "gap", "used", "ok", "err_deg", "z"):
        assert "__ground_" + s in LIFT_SUFFIXES
    assert all(s in LIFT_SUFFIXES for s in ("__contact", "__foot_height", "__skate", "__skate_pairs"))


def test_the_ground_report(tmp_path):
    from _entry import write_lift_ground_report
    rows = [dict(key="a.fused0", frames=300, contacts=331, rms_mm=5.4321, gap=0.0251, err_deg=0.0413, z_mm=1.25, skate_mm=8.8, skate_pairs=290),
            dict(key="b", frames=5, contacts=0, rms_mm=0.0, gap=0.0, err_deg=float("nan"), z_mm=float("nan"), skate_mm=0.0, skate_pairs=0)]
    text = open(write_lift_ground_report(str(tmp_path), rows)).read().splitlines()
    assert text[0] == "key,frames,contacts,rms_mm,gap,err_deg,z_mm,skate_mm,skate_pairs"
    assert text[1] == "a.fused0,300,331,5.4321,0.0251,0.0413,1.25,8.8,290" and text[2] == "b,5,0,0,0,nan,nan,0,0" and len(text) == 3


def test_new_abi_symbol_is_declared_everywhere():
    from manipose_amd import _lib, lifting, lift_ops
    import manipose_amd
    header = open(_lib.HEADER_PATH).read()
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "mp_lift_ground" in _lib.declared_symbols() and len(_lib._SIGNATURES["mp_lift_ground"][1]) == 30
    assert "lib.mp_lift_ground.argtypes = [vp, i64, i32, i32, vp, vp, i32, C.POINTER(i32), i32, i32, i32, i32, f32, f32, f32, i32, f32, " in integration
    assert _lib.ABI_VERSION == 8 and int(re.search(r"#define MP_ABI_VERSION (\d+)", header).group(1)) == 8        # purely additive
    for name, value in (("MAXFEET", lift_ops.GROUND_MAXFEET), ("MAXRADIUS", lift_ops.GROUND_MAXRADIUS), ("MAXITERS", lift_ops.GROUND_MAXITERS)):
        assert int(re.search(rf"#define MP_LIFT_GROUND_{name} (\d+)", header).group(1)) == value
    assert manipose_amd.estimate_ground is lifting.estimate_ground is lift_ops.estimate_ground and "estimate_ground" in lifting.__all__
    assert lifting.Ground._fields == ("normal", "offset", "quat", "trans", "rms", "gap", "used", "ok", "contact", "height", "skate", "skate_pairs")
    source = open(os.path.join(ROOT, "manipose_amd", "csrc", "lift_ground.hip")).read()
    assert source.index("#pragma clang fp contract(off)") < source.index('#include "lift_geom.h"') and "atomicAdd" not in source
    for name in ("README.md", "DESIGN.md", os.path.join("tools", "README.md")):
        assert "mp_lift_ground" in open(os.path.join(ROOT, name)).read(), name
    if os.path.exists(_lib.LIB_PATH):
        assert hasattr(_lib.load(), "mp_lift_ground")

"""Synchronising a take's views in time, the parts that need no device: the float64 statement of mp_lift_sync_views' and mp_lift_shift_views'
rules (lift_sync_ref.py) on constructed rows, every condition under which the device test (test_gpu_lift_sync.py) claims its bounds, the
recovery claim on a committed seed, the option checks of hpe/_entry.py and the declarations."""
import os
import re
import sys

import numpy as np
import pytest
import torch

import lift_sync_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hpe"))


def test_the_device_tests_rows_meet_the_conditions_of_their_bounds():
    """lag_int is held to the statement where the best curve value lies at least 1e-9 (relative) below the runner-up, lag where also
    den >= 1e-4 c[d*]: every row of the device test's cases that has a lag is such a row.  The cases cover what the device test says they do."""
    seen_ok, frames, joints, views, lags = set(), set(), set(), set(), set()
    some_inf = all_inf = False
    for tag, inp, want in ref.cases():
        has = (want["ok"] & 1).astype(bool) & (want["used"] > 0)
        assert (want["margin"][has] >= ref.MARGIN_MIN).all(), (tag, want["margin"])
        assert (want["den_ratio"][(want["ok"] & 2).astype(bool)] >= ref.DEN_MIN).all(), (tag, want["den_ratio"])
        seen_ok |= set(want["ok"].ravel().tolist())
        off = inp["off"]
        frames |= {int(b - a) for a, b in zip(off[:-1], off[1:])}
        joints.add(int(inp["poses"].shape[2]))
        views.add(int(inp["poses"].shape[0]))
        lags.add(int(inp.get("max_lag", 32)))
        inf = np.isinf(want["curve"])
        some_inf |= bool(inf.any() and not inf.all())
        all_inf |= any(inf[g, v].all() for g in range(inf.shape[0]) for v in range(inf.shape[1]))
    assert seen_ok == {0, 1, 3} and {1, 255, 256, 257, 600} <= frames and {2, 5, 17} <= joints and {1, 4} <= views and {0, 1, 40, 256} <= lags
    assert some_inf and all_inf
    by_tag = {tag: want for tag, _, want in ref.cases()}
    at, below = by_tag["n(d) exactly min_overlap at |d| = 8"]["curve"][0, 1], by_tag["n(d) one below min_overlap at |d| = 8"]["curve"][0, 1]
    assert np.isfinite(at[[12 - 8, 12 + 8]]).all() and np.isinf(at[[12 - 9, 12 + 9]]).all() and np.isinf(below[[12 - 8, 12 + 8]]).all()
    assert np.isfinite(below[[12 - 7, 12 + 7]]).all() and np.array_equal(at[5:20], below[5:20])
    blind = by_tag["max_lag larger than the take: every lag ineligible"]
    assert blind["ok"][0].tolist() == [1, 0, 0] and np.isinf(blind["curve"][0, 1:]).all() and not blind["lag"].any()


def test_constructed_rows_of_the_statement():
    still = ref.sync(ref.static_pair(), max_lag=8)                        # a body that does not move: the tie rule decides, no parabola
    assert not still["curve"].any() and still["lag_int"][0].tolist() == [0, 0] and not still["lag"].any()
    assert still["ok"][0].tolist() == [1, 1] and not still["contrast"].any() and still["used"][0].tolist() == [40, 40]
    copy = ref.sync(ref.delayed_copy(), max_lag=8, sigma=float("inf"))    # an exact copy delayed by 5 frames
    assert copy["lag_int"][0, 1] == 5 and copy["curve"][0, 1, 8 + 5] == 0 and copy["ok"][0, 1] == 3 and copy["contrast"][0, 1] == 1
    assert abs(copy["lag"][0, 1] - 5) <= 0.5 and (copy["curve"][0, 1, np.arange(17) != 13] > 0).all()
    assert ref.sync(ref.delayed_copy(), max_lag=8)["lag_int"][0, 1] == 5
    border = ref.sync(ref.delayed_copy(), max_lag=5)                      # the minimum at the border of the range: no sub-frame part, bit 1 clear
    assert border["lag_int"][0, 1] == 5 and border["lag"][0, 1] == 5.0 and border["ok"][0, 1] == 1
    for d in (-5, 0, 5):                                                  # the sign of the rule: frame f + lag of view v shows frame f of the reference
        assert ref.sync(ref.delayed_copy(delay=d), max_lag=8)["lag_int"][0, 1] == d
    none = ref.sync(ref.static_pair(), valid=np.zeros((2, 40), np.uint8))
    assert not none["ok"].any() and not none["curve"].any() and not none["used"].any()
    tie = np.array([np.inf, 2.0, 1.0, 3.0, 1.0, 1.0, np.inf])             # lags -3 .. 3: the value, then |d|, then the positive lag
    assert ref.pick(tie, 3)["lag_int"] == 1 and ref.pick(np.array([np.inf, 1.0, 1.0, 3.0, 2.0, 2.0, np.inf]), 3)["lag_int"] == -1
    assert ref.pick(np.array([1.0, 5.0, 1.0]), 1)["lag_int"] == 1 and ref.pick(np.full(3, np.inf), 1)["ok"] == 0
    flat = ref.pick(np.array([2.0, 1.0, 1.0, 1.0, 2.0]), 2)              # den = 0: no parabola
    assert flat["lag_int"] == 0 and flat["lag"] == 0 and flat["ok"] == 1
    steep = ref.pick(np.array([9.0, 1.0, 1.0 + 1e-9, 9.0, 9.0]), 2)       # the vertex is clamped to half a frame
    assert steep["lag_int"] == -1 and steep["ok"] == 3 and -1.0 < steep["lag"] <= -0.5


def test_the_statement_of_shift_views():
    g = np.random.default_rng(4)
    x = g.standard_normal((3, 30, 5, 2)).astype(np.float32)
    off = np.array([0, 12, 30])
    valid = (g.random((3, 30)) > 0.2).astype(np.uint8)
    for mode in ("nearest", "linear"):
        out, vout = ref.shift(x, np.zeros((2, 3)), valid, off, mode)      # lag 0: the identity on data (at the valid frames) and mask
        assert np.array_equal(vout, valid) and np.array_equal(out[valid != 0], x[valid != 0]) and not out[valid == 0].any()
        out, vout = ref.shift(x, np.zeros((2, 3)), None, off, mode)
        assert np.array_equal(out, x) and vout.all()
    lag = np.array([[0, 2, -3], [1, 0, 40]], np.float32)
    a, va = ref.shift(x, lag, valid, off, "nearest")
    b, vb = ref.shift(x, lag, valid, off, "linear")
    assert np.array_equal(a, b) and np.array_equal(va, vb)                # an integer lag in linear is nearest
    assert np.array_equal(a[1, :10], x[1, 2:12] * (valid[1, 2:12, None, None] != 0)) and not va[1, 10:12].any() and not va[2, 12:].any()
    half, vh = ref.shift(x, np.array([[0, 0.5, 0], [0, 0, 0]], np.float32), None, off, "linear")
    assert np.array_equal(half[1, :11], ((0.5 * x[1, :11].astype(np.float64)) + 0.5 * x[1, 1:12].astype(np.float64)).astype(np.float32))
    assert vh[1, :11].all() and not vh[1, 11] and not half[1, 11].any()   # the last frame of the take has no second frame
    near, _ = ref.shift(x, np.array([[0, 0.5, -0.5], [0, 0, 0]], np.float32), None, off, "nearest")
    assert np.array_equal(near[1, :11], x[1, 1:12]) and np.array_equal(near[2, :12], x[2, :12])      # floor(p + 0.5)
    nan, vn = ref.shift(x, np.array([[0, np.nan, 0], [np.inf, 0, 0]], np.float32), None, off, "linear")
    assert not vn[1, :12].any() and not nan[1, :12].any() and vn[1, 12:].all() and not vn[0, 12:].any() and vn[0, :12].all()


def test_recovery_on_the_committed_seed():
    """300 frames, 17 joints, 4 views with true lags of 0, 3, -7.5 and 12.25 frames, noise 0.01 m, 20 % of the frames of views 1..3
    depth-mirrored, 10 % of every view's frames gross outliers (lift_sync_ref.RECOVERY, seed 3).  Measured with the float64 statement, frames
    off the true lag per view 1..3:
      robust (the defaults: max_lag 32, min_overlap 16, sigma 0.05 m)     0.041 0.012 0.000
      plain squares (sigma = inf)                                        0.874 0.614 0.544
      the same motion without noise, mirrored frames and outliers        0.003 0.009 0.034   (the parabola's bias)
    Over the seeds 0 .. 7 the robust estimate ends at most 0.098 frame off, plain squares up to 1.39.  The condition: with the defaults every
    view's lag is within 0.5 frame of the truth - what makes the nearest-frame shift the right one."""
    sc = ref.recovery()
    robust = ref.sync(sc["poses"], None, sc["off"])
    plain = ref.sync(sc["poses"], None, sc["off"], sigma=float("inf"))
    clean = ref.scene(**dict(ref.RECOVERY, lens=list(ref.RECOVERY["lens"]), noise=0.0, mirrored=0.0, outliers=0.0))
    bias = ref.sync(clean["poses"], None, clean["off"])
    err = lambda r: np.abs(r["lag"][0] - sc["lag"])
    print("robust", np.round(err(robust), 3), "plain", np.round(err(plain), 3), "noise-free", np.round(err(bias), 3), "contrast", np.round(robust["contrast"][0], 2))
    assert (err(robust) <= ref.RECOVERY_BOUND).all() and robust["ok"][0].tolist() == [1, 3, 3, 3]
    assert np.array_equal(np.floor(robust["lag"][0] + 0.5), np.floor(sc["lag"] + 0.5)) or (err(robust) < 0.5).all()
    assert err(robust).max() < 0.1 and err(plain).max() > 0.5 and err(bias).max() <= 0.08      # (the figures of the docstring, loosely)
    assert (robust["margin"][0, 1:] >= ref.MARGIN_MIN).all() and (robust["den_ratio"][0, 1:] >= ref.DEN_MIN).all()


def test_new_abi_symbols_are_declared_everywhere():
    from manipose_amd import _lib, lifting
    import manipose_amd
    header = open(_lib.HEADER_PATH).read()
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name, nargs in (("mp_lift_sync_views_scratch_bytes", 3), ("mp_lift_sync_views", 20), ("mp_lift_shift_views", 12)):
        assert name in _lib.declared_symbols() and len(_lib._SIGNATURES[name][1]) == nargs
        assert f"lib.{name}.argtypes" in integration
    assert _lib.ABI_VERSION == 8 and int(re.search(r"#define MP_ABI_VERSION (\d+)", header).group(1)) == 8        # purely additive
    assert int(re.search(r"#define MP_LIFT_SYNC_MAXLAG (\d+)", header).group(1)) == lifting.SYNC_MAXLAG == 256
    assert int(re.search(r"#define MP_LIFT_SHIFT_MAXM (\d+)", header).group(1)) == 2 ** 20
    assert manipose_amd.sync_views is lifting.sync_views and manipose_amd.shift_views is lifting.shift_views
    assert "sync_views" in lifting.__all__ and "shift_views" in lifting.__all__
    assert (lifting.SYNC_MAX_LAG, lifting.SYNC_MIN_OVERLAP, lifting.SYNC_SIGMA) == (32, 16, 0.05)
    assert lifting.ViewSync._fields == ("lag", "lag_int", "curve", "contrast", "used", "ok")
    assert os.path.exists(os.path.join(ROOT, "manipose_amd", "csrc", "lift_sync.hip"))
    for name in ("README.md", "DESIGN.md"):
        assert "mp_lift_sync_views" in open(os.path.join(ROOT, name)).read()
    if os.path.exists(_lib.LIB_PATH):
        assert hasattr(_lib.load(), "mp_lift_sync_views") and hasattr(_lib.load(), "mp_lift_shift_views")
        assert _lib.load().mp_lift_sync_views_scratch_bytes(4, 100, 17) == (4 * 100 * (8 * 16 + 80 + 1) + 7) // 8 * 8
        assert _lib.load().mp_lift_sync_views_scratch_bytes(5, 100, 17) == 0 and _lib.load().mp_lift_sync_views_scratch_bytes(4, 0, 17) == 0


def test_config_keys_parse_and_a_sync_without_the_fusion_fails():
    from _entry import LIFT_SUFFIXES, lift_fuse_sync_options, load_config, run
    cfg = load_config([])
    assert cfg.lift.fuse_sync == "none" and lift_fuse_sync_options(cfg) == (False, 32, 16, 0.05, "linear")
    on = ["run.lift=true", "lift.fuse=true", "lift.fuse_sync=estimate"]
    assert lift_fuse_sync_options(load_config(on)) == (True, 32, 16, 0.05, "linear")
    assert lift_fuse_sync_options(load_config(on + ["lift.fuse_sync_max_lag=0", "lift.fuse_sync_min_overlap=4", "lift.fuse_sync_sigma=0.1",
                                                    "lift.fuse_sync_interp=nearest"])) == (True, 0, 4, 0.1, "nearest")
    assert lift_fuse_sync_options(load_config(["run.lift=true", "lift.fuse=true", "lift.fuse_sync=none"]))[0] is False
    with pytest.raises(SystemExit):
        load_config(["lift.fuse_synch=estimate"])
    fused = ["run.lift=true", "lift.fuse=true"]
    for argv, word in ((fused + ["lift.fuse_sync=guess"], "none or estimate"), (["run.lift=true", "lift.fuse_sync=estimate"], "set lift.fuse=true"),
                       (["lift.fuse_sync=estimate"], "set lift.fuse=true"), (fused + ["lift.fuse_sync_max_lag=8"], "set lift.fuse_sync=estimate"),
                       (fused + ["lift.fuse_sync_min_overlap=8"], "set lift.fuse_sync=estimate"), (fused + ["lift.fuse_sync_sigma=0.1"], "set lift.fuse_sync=estimate"),
                       (fused + ["lift.fuse_sync_interp=nearest"], "set lift.fuse_sync=estimate"), (on + ["lift.fuse_sync_max_lag=257"], "0..256"),
                       (on + ["lift.fuse_sync_max_lag=-1"], "0..256"), (on + ["lift.fuse_sync_max_lag=1.5"], "0..256"), (on + ["lift.fuse_sync_min_overlap=0"], ">= 1"),
                       (on + ["lift.fuse_sync_sigma=0"], "> 0"), (on + ["lift.fuse_sync_sigma=abc"], "is a number"), (on + ["lift.fuse_sync_interp=cubic"], "linear or nearest")):
        with pytest.raises(ValueError, match=word):
            run(["run.train=false", "run.test=false"] + argv)                    # (a run that got further would need a device)
    assert all("__sync_" + s in LIFT_SUFFIXES for s in ("lag", "contrast", "used", "ok", "curve"))


def test_argument_errors_are_value_errors_before_any_device_work():
    """The calls are given CPU tensors: had the arguments been accepted, they would have ended in the RuntimeError that refuses them ("no CPU
    fallback"), which is what the valid calls at the end do."""
    from manipose_amd import shift_views, sync_views
    poses, valid = torch.zeros(3, 6, 17, 3), torch.ones(3, 6, dtype=torch.uint8)
    for kw, word in ((dict(poses=torch.zeros(6, 17, 3)), "poses must be"), (dict(poses=poses.double()), "poses must be"), (dict(poses=torch.zeros(5, 6, 17, 3)), "views"),
                     (dict(poses=torch.zeros(3, 6, 1, 3)), "joints"), (dict(poses=torch.zeros(3, 6, 17, 2)), "poses must be"), (dict(valid=valid[:2]), "valid must be"),
                     (dict(valid=valid.bool()), "valid must be"), (dict(max_lag=-1), "max_lag"), (dict(max_lag=257), "max_lag"), (dict(max_lag=1.5), "max_lag"),
                     (dict(max_lag=True), "max_lag"), (dict(min_overlap=0), "min_overlap"), (dict(min_overlap=2.0), "min_overlap"), (dict(sigma=0), "sigma"),
                     (dict(sigma=-1.0), "sigma"), (dict(sigma=float("nan")), "sigma"), (dict(sigma="a"), "sigma"), (dict(sigma=True), "sigma")):
        with pytest.raises(ValueError, match=word):
            sync_views(**dict(dict(poses=poses), **kw))
    for kw in (dict(), dict(valid=valid, max_lag=0, min_overlap=1, sigma=float("inf")), dict(take_offset=[0, 3, 6], max_lag=256)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            sync_views(poses, **kw)
    x, lag = torch.zeros(3, 6, 5, 2), np.zeros((1, 3), np.float32)
    for kw, word in ((dict(x=torch.zeros(6)), "x must be"), (dict(x=x.double()), "x must be"), (dict(x=torch.zeros(5, 6, 2)), "x must be"),
                     (dict(x=torch.zeros(3, 6, 0)), "floats per frame"), (dict(x=torch.zeros(1, 1, 2 ** 20 + 1)), "floats per frame"), (dict(mode="cubic"), "mode"),
                     (dict(lag=np.zeros((2, 3))), "lag must be"), (dict(lag=np.zeros(4)), "lag must be"), (dict(lag=np.array(["a"] * 3)), "lag must be"),
                     (dict(lag=np.zeros(3), take_offset=[0, 3, 6]), "lag must be"), (dict(valid=valid[:2]), "valid must be")):
        with pytest.raises(ValueError, match=word):
            shift_views(**dict(dict(x=x, lag=lag), **kw))
    for kw in (dict(), dict(lag=np.zeros(3)), dict(lag=torch.zeros(2, 3), take_offset=[0, 3, 6], valid=valid, mode="nearest"), dict(x=torch.zeros(3, 6))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            shift_views(**dict(dict(x=x, lag=lag), **kw))

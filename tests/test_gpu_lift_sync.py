"""Synchronising a take's views in time on the device: mp_lift_sync_views and mp_lift_shift_views against the float64 statement of their rules
(lift_sync_ref.py), constructed rows compared exactly, the invariants (identical bits, a take alone and beside others, inputs untouched, invalid
frames never read), argument errors, the recovery scene the feature is for, and run.lift with lift.fuse_sync end to end.

The bounds against the statement, ON THE SAME float32 INPUTS: used, ok and lag_int are equal; the curve's infinities are equal and a finite value
is within one float32 ulp of max(|want|, floor); lag within one float32 ulp of max(|want|, 1); contrast within one ulp of 1.  The kernel and the
statement both work in fp64 and differ only in the order of their sums: relative 1e-15 or so per sum, 1e-13 at worst over these takes' 600
frames, against 6e-8 for half a float32 ulp; what remains is the one rounding to float32.  lag_int can be held to the statement where the best
value lies at least 1e-9 (relative) below the runner-up, and delta = 0.5 (c- - c+) / den carries the curve's relative error divided by
den / c[d*], asked to be >= 1e-4: 1e-13 / 1e-4 = 1e-9 of a frame, against 1.2e-7 for the ulp of 1.  Every compared row is asserted to meet both
(test_lift_sync_host.py asserts it without a device as well).  The bounds are derived, not measured from the kernel.  Measured on an MI355X:
the curve at most 0.500 ulp, lag 0.483, contrast 0.243 - the one rounding and nothing else.

The floor.  A signal value s = d - m carries an fp64 error of about delta_s = 2^-50 dmax, dmax the take's largest distance: one rounding of the
square root, one of the subtraction, and the mean's, a few units of 2^-53 in either order of summation.  A curve value c is a mean of squared
differences t^2 of such values (the robust factor only shrinks a term), so the two sides differ by at most 2 sqrt(c) (2 delta_s) + (2 delta_s)^2,
relative 4 delta_s / sqrt(c) + ..: below 2^-25, half a float32 ulp's worth, once c >= 2^54 delta_s^2.  With the differences' errors
half correlated that is c >= 2^52 delta_s^2 = 2^-48 dmax^2, the floor; a value below it is cancellation noise - it comes out of terms that
cancel to the last bits - and is held to one float32 ulp OF THE FLOOR, which the bound 2 sqrt(floor) (2 delta_s) = 2^-72 dmax^2 stays under.
In the seeded scenes the smallest curve value is 1e-5 or more against a floor of 1e-14; the rows that are exactly 0 are constructed from dyadic
numbers, on which both sides are exact."""
import os
import sys

import numpy as np
import pytest
import torch

import lift_sync_ref as ref
from lift_fixtures import fixture_model as _model, same as _same

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hpe"))
KEYS = ("lag", "lag_int", "curve", "contrast", "used", "ok")
ULP1 = float(np.spacing(np.float32(1.0)))


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _sync(poses, valid=None, off=None, max_lag=32, min_overlap=16, sigma=0.05):
    from manipose_amd import sync_views
    res = sync_views(_dev(poses), _dev(valid), off, max_lag, min_overlap, sigma)
    torch.cuda.synchronize()
    return {k: r.cpu().numpy() for k, r in zip(KEYS, res)}


def _shift(x, lag, valid=None, off=None, mode="linear"):
    from manipose_amd import shift_views
    out, vout = shift_views(_dev(x), lag, _dev(valid), off, mode)
    torch.cuda.synchronize()
    return out.cpu().numpy(), vout.cpu().numpy()


def _compare(tag, got, want):
    assert got["used"].dtype == got["lag_int"].dtype == np.int32 and got["ok"].dtype == np.uint8
    assert got["lag"].dtype == got["curve"].dtype == got["contrast"].dtype == np.float32 and got["curve"].shape == want["curve"].shape
    assert np.array_equal(got["used"], want["used"]) and np.array_equal(got["ok"], want["ok"]), (tag, got["ok"], want["ok"], got["used"], want["used"])
    has = (want["ok"] & 1).astype(bool) & (want["used"] > 0)
    assert (want["margin"][has] >= ref.MARGIN_MIN).all() and (want["den_ratio"][(want["ok"] & 2).astype(bool)] >= ref.DEN_MIN).all(), tag
    assert np.array_equal(got["lag_int"], want["lag_int"]), (tag, got["lag_int"], want["lag_int"])
    assert np.array_equal(np.isinf(got["curve"]), np.isinf(want["curve"])) and not np.isnan(got["curve"]).any() and not (got["curve"] < 0).any(), tag
    finite = np.isfinite(want["curve"])
    bound = ref.curve_bound(want["curve"], want["dmax"][:, None, None])
    excess = np.abs(np.where(finite, got["curve"].astype(np.float64), 0.0) - np.where(finite, want["curve"], 0.0)) / bound
    d_lag = np.abs(got["lag"].astype(np.float64) - want["lag"]) / ref.ulp32(np.maximum(np.abs(want["lag"]), 1.0))
    d_con = np.abs(got["contrast"].astype(np.float64) - want["contrast"]) / ULP1
    print(f"[{tag}] curve off by {excess.max():.3f} ulp, lag by {d_lag.max():.3f} ulp, contrast by {d_con.max():.3f} ulp of 1")
    assert excess.max() <= 1.0 and d_lag.max() <= 1.0 and d_con.max() <= 1.0, tag
    fill = want["ok"] == 0                                                # a row without a lag: zeros, exactly
    assert not got["lag"][fill].any() and not got["lag_int"][fill].any() and not got["contrast"][fill].any()


@pytest.mark.parametrize("n", range(len(ref.cases())))
def test_sync_matches_the_statement(n):
    tag, inp, want = ref.cases()[n]
    got = _sync(inp["poses"], inp.get("valid"), inp["off"], inp.get("max_lag", 32), inp.get("min_overlap", 16), inp.get("sigma", 0.05))
    _compare(tag, got, want)


def test_constructed_rows():
    still = _sync(ref.static_pair(), max_lag=8)                           # a body that does not move
    assert not still["curve"].any() and not still["lag_int"].any() and not still["lag"].any() and still["ok"][0].tolist() == [1, 1]
    assert not still["contrast"].any() and still["used"][0].tolist() == [40, 40] and not np.signbit(still["lag"]).any()
    far = _sync(ref.static_pair(), max_lag=32)                            # ... and where fewer than 16 frames pair: +inf, by the tie rule still lag 0
    assert np.array_equal(np.isinf(far["curve"][0, 1]), np.abs(np.arange(-32, 33)) > 24) and not far["lag_int"].any() and far["ok"][0, 1] == 1
    copy = _sync(ref.delayed_copy(), max_lag=8, sigma=float("inf"))       # view 1 an exact copy of the reference delayed by 5 frames
    want = ref.sync(ref.delayed_copy(), max_lag=8, sigma=float("inf"))
    assert copy["lag_int"][0, 1] == 5 and copy["curve"][0, 1, 8 + 5] == 0 and copy["ok"][0, 1] == 3 and copy["contrast"][0, 1] == 1
    assert _same(copy["curve"], want["curve"].astype(np.float32)) and _same(copy["lag"], want["lag"].astype(np.float32))      # dyadic: both sides exact
    robust = _sync(ref.delayed_copy(), max_lag=8)
    assert robust["lag_int"][0, 1] == 5 and robust["curve"][0, 1, 13] == 0 and robust["contrast"][0, 1] == 1
    _compare("a delayed copy", robust, ref.sync(ref.delayed_copy(), max_lag=8))
    border = _sync(ref.delayed_copy(), max_lag=5)                         # the minimum at the border: bit 1 clear, no sub-frame part
    assert border["lag_int"][0, 1] == 5 and border["lag"][0, 1] == 5.0 and border["ok"][0, 1] == 1 and border["curve"][0, 1, 10] == 0
    early = _sync(ref.delayed_copy(delay=-5), max_lag=8)
    assert early["lag_int"][0, 1] == -5 and early["curve"][0, 1, 3] == 0
    none = _sync(ref.static_pair(), valid=np.zeros((2, 40), np.uint8))    # no usable frame at all
    assert not none["ok"].any() and not none["curve"].any() and not none["used"].any() and not none["lag"].any()


def _shift_inputs():
    g = np.random.default_rng(4)
    off = np.array([0, 12, 13, 300])
    valid = (g.random((3, 300)) > 0.2).astype(np.uint8)
    lag = np.array([[0, 2, -3], [0.25, 0, -0.5], [1.5, -7.75, 40.125]], np.float32)
    return g, off, valid, lag


@pytest.mark.parametrize("shape", [(), (34,), (5, 17, 4)])
def test_shift_matches_the_statement_bit_for_bit(shape):
    g, off, valid, lag = _shift_inputs()
    x = g.standard_normal((3, 300) + shape).astype(np.float32)
    x[0, 5], x[1, 40] = np.nan, np.inf                                    # (the NaN lies where view 0 is copied: its bits arrive; the infinity is interpolated)
    for mode in ("nearest", "linear"):
        for mask in (valid, None):
            got, want = _shift(x, lag, mask, off, mode), ref.shift(x, lag, mask, off, mode)
            assert got[0].shape == x.shape and _same(got[0], want[0]) and _same(got[1], want[1]), (mode, shape)
        out, vout = _shift(x, np.zeros((3, 3), np.float32), valid, off, mode)          # lag 0: the identity on data and mask
        assert _same(vout, valid) and _same(out[valid != 0], x[valid != 0]) and not out[valid == 0].view(np.uint32).any()
        out, vout = _shift(x, np.zeros((3, 3), np.float32), None, off, mode)
        assert _same(out, x) and vout.all()
    whole = np.round(lag)
    a, b = _shift(x, whole, valid, off, "nearest"), _shift(x, whole, valid, off, "linear")
    assert _same(a[0], b[0]) and _same(a[1], b[1])                        # an integer lag in linear is nearest
    bad = lag.copy()
    bad[2, 1], bad[0, 0] = np.nan, -np.inf                                # a lag that is not finite invalidates the view of that take
    out, vout = _shift(x, bad, valid, off, "linear")
    assert not vout[1, 13:].any() and not out[1, 13:].view(np.uint32).any() and not vout[0, :12].any() and _same(vout[2], ref.shift(x, bad, valid, off)[1][2])
    short, vshort = _shift(x, lag[:2], valid, np.array([0, 12, 13]), "linear")          # frames that no take holds: zeros, invalid
    assert not vshort[:, 13:].any() and not short[:, 13:].view(np.uint32).any() and _same(short[:, :13], ref.shift(x, lag[:2], valid, np.array([0, 12, 13]))[0][:, :13])
    from manipose_amd import shift_views
    d = _dev(x)
    one = shift_views(d[:, :12], torch.from_numpy(lag[0]).cuda(), None, None, "linear")            # (V,) device lags for one take; a view of x made contiguous
    assert _same(one[0].cpu().numpy(), ref.shift(x[:, :12], lag[:1])[0]) and _same(d.cpu().numpy(), x)


def test_invariants():
    from manipose_amd import sync_views
    sc = ref.scene(4, 17, [1, 257, 40], seed=211, true_lag=[0, 2, -4.5, 6.25], mirrored=0.3, outliers=0.1)
    valid = ref.valid_table(4, sc["off"], 212, missing=((1, 0), (2, 2)))
    spoiled = sc["poses"].copy()
    spoiled[valid == 0] = np.nan                                          # a frame marked invalid holds NaN and is never read
    d = [_dev(a) for a in (spoiled, valid)]
    a = sync_views(d[0], d[1], sc["off"])
    b = sync_views(d[0], d[1], sc["off"])
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(a, b))                   # identical bits
    assert np.array_equal(d[0].cpu().numpy(), spoiled, equal_nan=True) and _same(d[1].cpu().numpy(), valid)
    clean = _sync(sc["poses"], valid, sc["off"])
    assert all(_same(clean[k], x.cpu().numpy()) for k, x in zip(KEYS, a))
    for t in range(3):                                                    # a take alone: the bits it has beside the others
        sl = slice(int(sc["off"][t]), int(sc["off"][t + 1]))
        alone = _sync(sc["poses"][:, sl], valid[:, sl])
        assert all(_same(alone[k][0], clean[k][t]) for k in KEYS), t
    g, off, mask, lag = _shift_inputs()
    x = g.standard_normal((3, 300, 6)).astype(np.float32)
    dirty = x.copy()
    dirty[mask == 0] = np.nan
    for mode in ("nearest", "linear"):
        assert all(_same(p, q) for p, q in zip(_shift(dirty, lag, mask, off, mode), _shift(x, lag, mask, off, mode)))


def test_entry_points_reject_bad_arguments_before_any_launch(lib):
    V, F, J, G, L = 3, 40, 17, 1, 4
    poses = torch.zeros(V, F, J, 3, device="cuda")
    off = torch.tensor([0, F], dtype=torch.int64, device="cuda")
    lag, con = torch.full((G, V), -1.0, device="cuda"), torch.full((G, V), -1.0, device="cuda")
    curve = torch.full((G, V, 2 * L + 1), -1.0, device="cuda")
    lag_int, used = torch.full((G, V), 7, dtype=torch.int32, device="cuda"), torch.full((G, V), 7, dtype=torch.int32, device="cuda")
    ok = torch.full((G, V), 7, dtype=torch.uint8, device="cuda")
    need = lib.mp_lift_sync_views_scratch_bytes(V, F, J)
    assert need == (V * F * (8 * (J - 1) + 80 + 1) + 7) // 8 * 8
    scratch = torch.zeros(need // 8 + 1, dtype=torch.float64, device="cuda")
    p = lambda x: None if x is None else x.data_ptr()

    def call(x=poses, o=off, a=lag, i=lag_int, c=curve, k=con, u=used, g=ok, s=scratch, nbytes=need, v=V, f=F, j=J, ch=3, G=G, L=L, overlap=16, sigma=0.05, at=0):
        return lib.mp_lift_sync_views(p(x), v, f, j, ch, None, p(o), G, L, overlap, sigma, p(a), p(i), p(c), p(k), p(u), p(g), None if s is None else p(s) + at,
                                      nbytes, None)
    for kw in (dict(x=None), dict(o=None), dict(a=None), dict(i=None), dict(c=None), dict(k=None), dict(u=None), dict(g=None)):
        assert call(**kw) == 1 and b"null" in lib.mp_last_error()
    for kw, word in ((dict(v=0), b"V=0"), (dict(v=5), b"V=5"), (dict(j=1), b"J=1"), (dict(j=33), b"J=33"), (dict(ch=2), b"C=2"), (dict(ch=5), b"C=5"),
                     (dict(f=0), b"out of range"), (dict(f=-1), b"out of range"), (dict(G=0), b"out of range"), (dict(G=41), b"out of range"),
                     (dict(f=2 ** 31), b"out of range"), (dict(L=-1), b"max_lag=-1"), (dict(L=257), b"max_lag=257"), (dict(overlap=0), b"min_overlap=0"),
                     (dict(sigma=0.0), b"sigma"), (dict(sigma=-1.0), b"sigma"), (dict(sigma=float("nan")), b"sigma"), (dict(s=None), b"scratch"),
                     (dict(nbytes=need - 8), b"scratch"), (dict(at=4), b"scratch")):
        assert call(**kw) == 1 and word in lib.mp_last_error(), (kw, lib.mp_last_error())
    x, out = torch.zeros(V * F * 6 + 8, device="cuda"), torch.full((V * F * 6,), -1.0, device="cuda")
    vout, dlag = torch.full((V, F), 7, dtype=torch.uint8, device="cuda"), torch.zeros(G, V, device="cuda")

    def shift(i=x, o=off, a=dlag, r=out, w=vout, v=V, f=F, m=6, G=G, mode=1, at=0):
        return lib.mp_lift_shift_views(p(i), v, f, m, None, p(o), G, p(a), mode, None if r is None else p(r) + at, p(w), None)
    for kw in (dict(i=None), dict(o=None), dict(a=None), dict(r=None), dict(w=None)):
        assert shift(**kw) == 1 and b"null" in lib.mp_last_error()
    for kw, word in ((dict(v=0), b"V=0"), (dict(v=5), b"V=5"), (dict(m=0), b"M=0"), (dict(m=2 ** 20 + 1), b"M="), (dict(f=0), b"out of range"),
                     (dict(G=0), b"out of range"), (dict(G=41), b"out of range"), (dict(mode=2), b"mode=2"), (dict(mode=-1), b"mode=-1"),
                     (dict(r=x), b"overlap"), (dict(r=x, at=4 * (V * F * 6 - 1)), b"overlap"), (dict(r=x, at=32), b"overlap")):
        assert shift(**kw) == 1 and word in lib.mp_last_error(), (kw, lib.mp_last_error())
    torch.cuda.synchronize()
    for t in (lag, con, curve, out):
        assert bool((t == -1).all())                                      # nothing was launched
    assert all(bool((t == 7).all()) for t in (lag_int, used, ok, vout))
    assert call() == 0 and call(sigma=float("inf"), L=0, c=curve) == 0 and shift() == 0 and shift(i=out, r=x, at=32) == 0
    torch.cuda.synchronize()
    assert used[0].tolist() == [F] * V and ok[0].tolist() == [1, 1, 1] and not lag.any() and bool((vout == 1).all())      # all-zero poses: a curve of zeros
    from manipose_amd import shift_views, sync_views
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        sync_views(poses.cpu())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        sync_views(poses, valid=torch.ones(V, F, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        shift_views(poses.cpu(), np.zeros(V, np.float32))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        shift_views(poses, np.zeros(V, np.float32), valid=torch.ones(V, F, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="out of range"):
        sync_views(poses, take_offset=list(range(F + 2)))                 # more takes than frames: the entry point's own refusal


def test_recovery_scene_on_the_device():
    """the scene of test_lift_sync_host.test_recovery_on_the_committed_seed: with the defaults every view's lag is within 0.5 frame of the truth,
    and align_views' rms on the views shifted by the estimated lags is lower, for every view, than on the unshifted ones.  Measured on an
    MI355X: see DESIGN.md, "Synchronising a take's views in time"."""
    from manipose_amd import align_views, shift_views
    sc = ref.recovery()
    robust, plain = _sync(sc["poses"], None, sc["off"]), _sync(sc["poses"], None, sc["off"], sigma=float("inf"))
    err = lambda r: np.abs(r["lag"][0].astype(np.float64) - sc["lag"])
    print("frames off the truth: robust", np.round(err(robust), 3), "plain", np.round(err(plain), 3), "contrast", np.round(robust["contrast"][0], 2))
    assert (err(robust) <= ref.RECOVERY_BOUND).all() and robust["ok"][0].tolist() == [1, 3, 3, 3]
    _compare("recovery", robust, ref.sync(sc["poses"], None, sc["off"]))
    poses = _dev(sc["poses"])
    before = align_views(poses, None, sc["off"]).rms[0].cpu().numpy()
    for mode in ("linear", "nearest"):
        moved, valid = shift_views(poses, robust["lag"], None, sc["off"], mode)
        after = align_views(moved, valid, sc["off"])
        print(f"align_views rms, views 1..3: unshifted {np.round(before[1:], 4)}, shifted ({mode}) {np.round(after.rms[0, 1:].cpu().numpy(), 4)}")
        assert (after.rms[0, 1:].cpu().numpy() < before[1:]).all() and (after.ok[0].cpu().numpy() & 1).all()


# ---- end to end: the tiny fp32 fixture model of lift_fixtures.py -----------------------------------------------------------------------------
def _group(lens=(20, 20, 20, 20, 12, 12, 12), seed=51):
    """one group of 7 sequences: a take of 4 views of 20 frames, then a take of 3 views of 12 frames; S11's cameras as fetch() hands them on
    (the group of test_gpu_lift_align.py)"""
    from manipose_amd.data.ingest import h36m_cameras
    s11 = h36m_cameras()["S11"]
    g = np.random.default_rng(seed)
    seqs = [np.clip(0.3 * g.standard_normal((n, 17, 2)), -1, 1).astype(np.float32) for n in lens]
    cams = [np.concatenate([s11[i]["intrinsic"], s11[i]["orientation"], s11[i]["translation"], np.array([i])]) for i in (0, 1, 2, 3, 0, 1, 2)]
    return {"walk": seqs}, {"walk": cams}


@pytest.mark.parametrize("cameras", ["dataset", "estimate"])
def test_run_lift_with_synchronised_views_end_to_end(tmp_path, cameras, capsys):
    from _entry import lift_sequences_to_file, load_config
    from manipose_amd import sync_views
    model, T, K = _model("rmcl")
    groups, cams = _group()
    base = ["run.lift=true", "train.tta=false", "train.batch_size_test=2", "lift.hyps=true", "lift.fuse=true", f"lift.fuse_cameras={cameras}"]
    base += ["lift.frame=world", "lift.floor=true"] if cameras == "estimate" else []
    before = lift_sequences_to_file(model, load_config(base), groups, str(tmp_path / "before.npz"), cams)
    off = lift_sequences_to_file(model, load_config(base + ["lift.fuse_sync=none"]), groups, str(tmp_path / "none.npz"), cams)
    a, b = np.load(str(tmp_path / "before.npz")), np.load(str(tmp_path / "none.npz"))
    assert list(a.keys()) == list(b.keys()) == list(before) == list(off) and all(a[k].dtype == b[k].dtype and _same(a[k], b[k]) for k in a.keys())
    assert not any("__sync_" in k for k in a.keys())
    capsys.readouterr()
    on = ["lift.fuse_sync=estimate", "lift.fuse_sync_max_lag=3", "lift.fuse_sync_min_overlap=8"]
    est = lift_sequences_to_file(model, load_config(base + on), groups, str(tmp_path / "estimate.npz"), cams)
    out = capsys.readouterr().out
    new = sorted(set(est) - set(before))
    assert new == sorted(f"walk.fused{t}__sync_{k}" for t in (0, 1) for k in ("lag", "contrast", "used", "ok", "curve")) and set(before) <= set(est)
    assert all(_same(est[k], v) for k, v in before.items() if ".fused" not in k)          # the views' own outputs do not change
    z = np.load(str(tmp_path / "estimate.npz"))
    assert all(_same(z[k], est[k]) for k in new)
    poses, valid = np.zeros((4, 32, 17, 3), np.float32), np.ones((4, 32), np.uint8)       # sync_views on the file's own per-view poses
    for i in range(4):
        poses[i, :20] = est[f"walk.{i}"]
    for i in range(3):
        poses[i, 20:] = est[f"walk.{4 + i}"]
    valid[3, 20:] = 0
    want = sync_views(_dev(poses), _dev(valid), [0, 20, 32], 3, 8, 0.05)
    for t, (n, V) in enumerate(((20, 4), (12, 3))):
        k = f"walk.fused{t}__sync_"
        assert est[k + "lag"].shape == est[k + "contrast"].shape == est[k + "used"].shape == est[k + "ok"].shape == (V,) and est[k + "curve"].shape == (V, 7)
        assert est[k + "lag"].dtype == est[k + "contrast"].dtype == est[k + "curve"].dtype == np.float32
        assert est[k + "used"].dtype == np.int32 and est[k + "ok"].dtype == np.uint8
        for key in ("lag", "contrast", "used", "ok", "curve"):
            assert _same(est[k + key], getattr(want, key)[t, :V].cpu().numpy()), (t, key)
        assert est[k + "ok"][0] == 1 and est[k + "used"].tolist() == [n] * V and est[k + "lag"][0] == 0
        assert est[f"walk.fused{t}"].shape == (n, 17, 3) and np.isfinite(est[f"walk.fused{t}"]).all()
        for v in range(V):                                                # a view that keeps lag 0 is reported
            lost = not est[k + "ok"][v] & 1 or abs(float(est[k + "lag"][v])) == 3      # (the border: lag_int = +-3, no sub-frame part)
            assert (f"lift.fuse_sync [walk]: take {t}, view {v + 4 * t}: its lag could not be estimated" in out) == bool(lost), (t, v, out)
    # the search range 0: every lag is exactly 0, and every fused output is the one of the run without sync, bit for bit
    for interp in ("linear", "nearest"):
        zero = lift_sequences_to_file(model, load_config(base + ["lift.fuse_sync=estimate", "lift.fuse_sync_max_lag=0", f"lift.fuse_sync_interp={interp}"]), groups,
                                      str(tmp_path / "zero.npz"), cams)
        assert all(_same(zero[k], v) for k, v in before.items()) and set(zero) - set(before) == set(new)
        assert all(not zero[f"walk.fused{t}__sync_lag"].any() and zero[f"walk.fused{t}__sync_curve"].shape[1] == 1 for t in (0, 1))

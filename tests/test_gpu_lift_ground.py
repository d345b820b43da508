"""Standing a take on its floor on the device: mp_lift_ground against the float64 statement of its rule (lift_ground_ref.py), constructed rows
compared exactly, the invariants (identical bits, a sequence alone and beside others, inputs untouched, invalid frames never read, to_world with
the returned rotation and shift), argument errors through the ABI, the recovery scene the feature is for, and run.lift with lift.ground end to end.

The bounds against the statement, ON THE SAME float32 INPUTS.  contact, used, ok and skate_pairs are EQUAL: the squared speed of step A is formed
by both sides with the same fp64 operations in the same order (and no compared speed lies within 1e-9, relative, of the threshold); ok's bit 0
is held where a row's gap (a2 - a1) / (a3 - a1) is >= 1e-4 or, for a row without a plane, (a2 - a1) <= 1e-12 max(|a1|, |a3|) against the rule's
1e-9; bit 1 where |n . b| >= 0.1.  Every compared row is asserted to meet these, here and in test_lift_ground_host.py without a device.

A float output is within ONE float32 ulp of max(|want|, its scale), the scale being 1 for the normal, the quaternion and the gap, L - the
largest |coordinate| of a foot in the sequence - for offset, trans, rms and the heights (lengths along the normal: n . x with |x| <= sqrt(3) L),
and the longest step of a contact pair for the skate.  Derivation: kernel and statement both work in fp64 and differ in the order of their sums
and in the eigen-solver (a Jacobi on s I - A against LAPACK on A; both backward stable, an error of a few u |A|, u = 2^-53).  A solve's sums
W, W m and C have N <= 678 terms: each side is off by at most N u times the sum of the absolute terms, which for C's diagonal is the sum
itself and elsewhere at most half the trace, with three roundings per term - in all at most e = 8 N u relative to tr C, 6.0e-13 here.  An
eigenvector moves by the matrix's error over the eigenvalue gap, which is why gap >= 1e-4 is asked: at worst 1e4 e = 6e-9 per solve, a tenth of
an ulp of 1.  The re-weighted solves feed a plane's error into the next solve's weights; instead of a worst-case product of Lipschitz constants
the host test MEASURES the whole chain in the statement: every solve's m, C and the axis are disturbed by delta = 1e-9 (relative to L, tr C, 1),
and the largest change of any output over its scale, over delta, is the amplification kappa - 33 to 86 over these cases.  The host test asserts
4 kappa e <= a quarter ulp of 1 (2^-25) for every case, the factor 4 because kappa is sampled, not maximised; kappa could be 12000.  What remains
is the one rounding to float32, half an ulp: the bound is one ulp.  Exact zeros (rms, heights and skate of the dyadic scenes) are exact on both
sides.  The bounds are derived, not measured from the kernel.  Measured on an MI355X, the worst of the eight cases and
the five recovery scenes, in these ulps: normal 0.247, offset 0.493, quat 0.239, trans 0.493, rms 0.006, gap 0.026, height 0.060, skate 0.242 - the one
rounding to float32 and nothing else.

to_world with the returned quat and trans: mp_lift_world works in fp64 on the float32 quaternion and shift and rounds once.  The quaternion's
components are each within half a float32 ulp of 1, which moves a point at distance sqrt(3) L by at most 4 ulp of L; trans_z, the height it is
compared with, and the result carry one rounding each, 1.5 ulp: a contact foot's z is foot_height + its height within 8 ulp of L, and with
sigma = inf the RMS of z - foot_height over the contact points is `rms` within the same.  Measured: 1.485 and 0.359 ulp of L."""
import os
import sys

import numpy as np
import pytest
import torch

import lift_ground_ref as ref
from lift_fixtures import same as _same

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hpe"))
KEYS = ("normal", "offset", "quat", "trans", "rms", "gap", "used", "ok", "contact", "height", "skate", "skate_pairs")
DTYPES = dict(used=np.int32, skate_pairs=np.int32, ok=np.uint8, contact=np.uint8)


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _ground(points, off=None, valid=None, **kw):
    from manipose_amd import estimate_ground
    res = estimate_ground(_dev(points), off, _dev(valid), **kw)
    torch.cuda.synchronize()
    assert res._fields == KEYS
    return {k: r.cpu().numpy() for k, r in zip(KEYS, res)}


def _compare(tag, got, want, off):
    S, ntot, nf = len(want["ok"]), *want["contact"].shape
    shapes = dict(normal=(S, 3), offset=(S,), quat=(S, 4), trans=(S, 3), rms=(S,), gap=(S,), used=(S,), ok=(S,), contact=(ntot, nf), height=(ntot, nf),
                  skate=(S,), skate_pairs=(S,))
    for k in KEYS:
        assert got[k].shape == shapes[k] and got[k].dtype == DTYPES.get(k, np.float32), (tag, k, got[k].shape, got[k].dtype)
    for k in ("contact", "used", "ok", "skate_pairs"):
        assert np.array_equal(got[k], want[k]), (tag, k, got[k], want[k])
    has = (want["ok"] & 1).astype(bool)
    e = want["eig"]
    assert want["speed_margin"] >= ref.SPEED_MARGIN and (e[has, 1] - e[has, 0] >= ref.GAP_MIN * (e[has, 2] - e[has, 0])).all(), tag
    assert (want["side"][has] >= ref.SIDE_MIN).all(), tag
    worst = {}
    for k in ref.FLOATS:
        assert np.isfinite(got[k]).all(), (tag, k)
        worst[k] = float((np.abs(got[k].astype(np.float64) - want[k]) / ref.bound(k, want, off)).max())
    print(f"[{tag}] off the statement, in float32 ulp of max(|want|, scale): " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert max(worst.values()) <= 1.0, (tag, worst)
    fill = ~has                                                           # a row without a plane: the fill values, exactly
    assert (got["normal"][fill] == [0, 0, 1]).all() and (got["quat"][fill] == [1, 0, 0, 0]).all()
    for k in ("offset", "trans", "rms", "gap"):
        assert not got[k][fill].view(np.uint32).any(), (tag, k)
    for s in np.nonzero(fill)[0]:
        assert not got["height"][int(off[s]):int(off[s + 1])].view(np.uint32).any(), (tag, s)
    assert (got["quat"][:, 3] == 0).all() and (got["quat"][:, 0] >= 0).all() and not got["trans"][:, :2].any()


@pytest.mark.parametrize("n", range(len(ref.cases())))
def test_ground_matches_the_statement(n):
    tag, inp, want = ref.cases()[n]
    _compare(tag, _ground(inp["points"], inp["off"], inp["valid"], **inp["opts"]), want, inp["off"])


def test_constructed_rows():
    zero = lambda a: not np.ascontiguousarray(a).view(np.uint32).any()      # +0 everywhere, by its bits
    flat = _ground(ref.dyadic_scene())                                    # the feet on z = 0, the axis +z
    assert _same(flat["normal"], np.array([[0, 0, 1]], np.float32)) and _same(flat["quat"], np.array([[1, 0, 0, 0]], np.float32)) and flat["ok"][0] == 3
    assert zero(flat["offset"]) and zero(flat["rms"]) and zero(flat["height"]) and zero(flat["skate"]) and zero(flat["trans"])
    assert flat["used"][0] == 44 + 2 * 20 and flat["skate_pairs"][0] == 43 + 2 * 19 and 0 < flat["gap"][0] < 1      # (the second foot takes one step)
    assert np.array_equal(flat["contact"], ref.ground(ref.dyadic_scene())["contact"])
    turned = _ground(ref.dyadic_scene(flip=True))                         # the same scene under an exact half turn about x
    assert _same(turned["normal"], np.array([[0, 0, -1]], np.float32)) and _same(turned["quat"], np.array([[0, 1, 0, 0]], np.float32)) and turned["ok"][0] == 3
    assert not turned["offset"].any() and not turned["rms"].any() and not turned["height"].any() and np.array_equal(turned["contact"], flat["contact"])
    up = _ground(ref.dyadic_scene(), foot_height=0.125)
    assert _same(up["trans"], np.array([[0, 0, 0.125]], np.float32)) and zero(up["height"])
    slide = _ground(ref.dyadic_scene(slide=2.0 ** -8), feet=(3,))         # a stance foot that slides by a dyadic step: that exact skate
    assert slide["skate"][0] == np.float32(2.0 ** -8) and slide["skate_pairs"][0] == 43 and _same(slide["normal"], flat["normal"]) and zero(slide["rms"])
    fast = _ground(ref.dyadic_scene(slide=2.0 ** -6), feet=(3,))          # ... and one that moves faster than the speed: no contact, no plane
    assert not fast["contact"].any() and fast["ok"][0] == 0 and fast["used"][0] == 0 and fast["skate_pairs"][0] == 0 and zero(fast["skate"])
    edge = _ground(ref.dyadic_scene(slide=2.0 ** -7), feet=(3,), speed=2.0 ** -7)      # exactly at the threshold (<=): a contact
    assert edge["contact"][2:-2].all() and edge["skate"][0] == np.float32(2.0 ** -7)
    lone = _ground(ref.dyadic_scene(), prior=0.0, feet=(3,))              # one point, again and again: no plane without a prior, skate reported
    assert lone["ok"][0] == 0 and lone["used"][0] == 44 and lone["skate_pairs"][0] == 43 and zero(lone["skate"]) and _same(lone["normal"], flat["normal"])


def test_invariants():
    from manipose_amd import estimate_ground
    tag, inp, want = ref.cases()[0]
    pts, valid, off = inp["points"], inp["valid"], inp["off"]
    assert valid is not None and (~np.isfinite(pts[valid == 0])).any(axis=(1, 2)).all()      # frames marked invalid hold NaN and are never read ...
    d = [_dev(pts), _dev(valid)]
    a = estimate_ground(d[0], off, d[1], **inp["opts"])
    b = estimate_ground(d[0], off, d[1], **inp["opts"])
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(a, b))                   # identical bits
    assert np.array_equal(d[0].cpu().numpy(), pts, equal_nan=True) and _same(d[1].cpu().numpy(), valid)      # inputs untouched
    filled = pts.copy()
    filled[valid == 0] = 1.5
    clean = _ground(filled, off, valid, **inp["opts"])                    # ... with numbers in their place no output bit changes
    assert all(_same(clean[k], x.cpu().numpy()) for k, x in zip(KEYS, a))
    for s in range(len(off) - 1):                                         # a sequence alone: the bits it has beside the others
        sl = slice(int(off[s]), int(off[s + 1]))
        alone = _ground(pts[sl], None, valid[sl], **inp["opts"])
        for k in KEYS:
            assert _same(alone[k], clean[k][sl] if k in ("contact", "height") else clean[k][s:s + 1]), (s, k)
    short = _ground(pts, off[:4], valid, **inp["opts"])                   # frames that no sequence holds: no contact, height 0
    assert not short["contact"][int(off[3]):].any() and not short["height"][int(off[3]):].view(np.uint32).any()
    assert all(_same(short[k], clean[k][:3]) for k in KEYS if k not in ("contact", "height"))
    assert _same(short["contact"][:int(off[3])], clean["contact"][:int(off[3])]) and _same(short["height"][:int(off[3])], clean["height"][:int(off[3])])


@pytest.mark.parametrize("n", [0, 3])
def test_to_world_stands_the_contact_feet_on_foot_height(n):
    from manipose_amd import to_world
    tag, inp, want = ref.cases()[n]
    o = dict(inp["opts"], foot_height=0.08)
    got = _ground(inp["points"], inp["off"], inp["valid"], **o)
    pts = np.where(np.isfinite(inp["points"][..., :3]), inp["points"][..., :3], np.float32(0)).copy()
    stood = to_world(_dev(pts), got["quat"], translation=got["trans"], seq_offset=inp["off"]).cpu().numpy()
    L = ref.frame_scale(want, inp["off"])
    feet = stood[:, list(o["feet"]), 2].astype(np.float64)
    touch = got["contact"] != 0
    plane = np.repeat((got["ok"] & 1).astype(bool), np.diff(inp["off"]))[:, None] & touch
    off_by = np.abs(feet - np.float32(0.08) - got["height"])[plane] / ref.ulp32(np.broadcast_to(L, feet.shape)[plane])
    print(f"[{tag}] contact feet after to_world: z - foot_height - height off by at most {off_by.max():.3f} ulp of L; {int(plane.sum())} contacts")
    assert plane.sum() > 300 and off_by.max() <= 8.0
    if o["sigma"] == float("inf"):                                        # every weight 1: rms is the RMS of the contact feet's z about foot_height
        for s in np.nonzero(got["ok"] & 1)[0]:
            sl = slice(int(inp["off"][s]), int(inp["off"][s + 1]))
            z = feet[sl][touch[sl]] - np.float32(0.08)
            assert abs(np.sqrt((z * z).mean()) - got["rms"][s]) <= 8.0 * ref.ulp32(want["scale"][s]), s
    assert (stood[:, o["axis"][1], 2][np.repeat((got["ok"] == 3), np.diff(inp["off"])) & (inp["valid"] != 0 if inp["valid"] is not None else True)] > 1.0).all()


@pytest.mark.parametrize("seed", ref.RECOVERY_SEEDS[:5])
def test_recovery_scene_on_the_device(seed):
    """the scene of test_lift_ground_host: 300 frames, 5 mm of noise, 10 % hover frames.  The measure is the RMS distance of the TRUE stance
    positions from the estimated plane and the angle to the true normal; RECOVERY_BOUND comes from the float64 statement on the CPU."""
    sc = ref.recovery_scene(seed)
    got, plain = _ground(sc["points"]), _ground(sc["points"], iters=0)
    rms, angle = ref.recovery_error(sc, got["normal"][0], got["offset"][0])
    rms0, angle0 = ref.recovery_error(sc, plain["normal"][0], plain["offset"][0])
    print(f"seed {seed}: plane off the true stance positions by {1000 * rms:.3f} mm, {angle:.3f} degrees (plain squares {1000 * rms0:.3f} mm, {angle0:.3f}); "
          f"rms {1000 * got['rms'][0]:.2f} mm, gap {got['gap'][0]:.3f}, skate {1000 * got['skate'][0]:.2f} mm / frame over {got['skate_pairs'][0]} pairs")
    assert got["ok"][0] == 3 and rms <= ref.RECOVERY_BOUND["rms_m"] and angle <= ref.RECOVERY_BOUND["angle_deg"] and rms0 > 3 * rms
    _compare(f"recovery {seed}", got, ref.ground(sc["points"]), np.array([0, 300]))


def test_entry_point_rejects_bad_arguments_before_any_launch(lib):
    import ctypes as C
    N, J, S, nf = 40, 17, 2, 2
    pts = torch.zeros(N, J, 3, device="cuda")
    off = torch.tensor([0, 25, N], dtype=torch.int64, device="cuda")
    f = lambda *shape: torch.full(shape, -1.0, device="cuda")
    i = lambda *shape, dt=torch.int32: torch.full(shape, 7, dtype=dt, device="cuda")
    outs = dict(normal=f(S, 3), offset=f(S), quat=f(S, 4), trans=f(S, 3), rms=f(S), gap=f(S), used=i(S), ok=i(S, dt=torch.uint8), contact=i(N, nf, dt=torch.uint8),
                height=f(N, nf), skate=f(S), skate_pairs=i(S))
    p = lambda x: None if x is None else x.data_ptr()

    def call(x=pts, o=off, n=N, j=J, ch=3, s=S, feet=(3, 6), nfeet=None, axis=(0, 8), radius=2, speed=0.01, sigma=0.03, prior=0.05, iters=5, fh=0.0, **null):
        table = None if feet is None else (C.c_int32 * len(feet))(*feet)
        return lib.mp_lift_ground(p(x), n, j, ch, None, p(o), s, table, len(feet) if nfeet is None else nfeet, axis[0], axis[1], radius, speed, sigma, prior,
                                  iters, fh, *(None if k in null else p(t) for k, t in outs.items()), None)
    for kw in (dict(x=None), dict(o=None), dict(feet=None, nfeet=2)) + tuple({k: None} for k in outs):
        assert call(**kw) == 1 and b"null" in lib.mp_last_error(), (kw, lib.mp_last_error())
    inf, nan = float("inf"), float("nan")
    for kw, word in ((dict(j=1), b"J=1"), (dict(j=33), b"J=33"), (dict(ch=2), b"C=2"), (dict(ch=5), b"C=5"), (dict(n=0), b"out of range"), (dict(s=0), b"out of range"),
                     (dict(s=41), b"out of range"), (dict(n=2 ** 30), b"too many"), (dict(feet=(), nfeet=0), b"nf=0"), (dict(feet=(3, 6, 1, 2, 4)), b"nf=5"),
                     (dict(feet=(3, 17)), b"feet[1] = 17"), (dict(feet=(-1, 6)), b"feet[0] = -1"), (dict(axis=(0, 17)), b"axis_to=17"), (dict(axis=(-1, 8)), b"axis_from=-1"),
                     (dict(axis=(8, 8)), b"axis_from == axis_to"), (dict(radius=0), b"radius=0"), (dict(radius=9), b"radius=9"), (dict(iters=-1), b"iters=-1"),
                     (dict(iters=9), b"iters=9"), (dict(speed=0.0), b"speed"), (dict(speed=-1.0), b"speed"), (dict(speed=inf), b"speed"), (dict(speed=nan), b"speed"),
                     (dict(sigma=0.0), b"sigma"), (dict(sigma=-1.0), b"sigma"), (dict(sigma=nan), b"sigma"), (dict(prior=-0.5), b"prior"), (dict(prior=inf), b"prior"),
                     (dict(prior=nan), b"prior"), (dict(fh=inf), b"foot_height"), (dict(fh=nan), b"foot_height")):
        assert call(**kw) == 1 and word in lib.mp_last_error(), (kw, lib.mp_last_error())
    torch.cuda.synchronize()
    assert all(bool((t == (7 if t.dtype in (torch.int32, torch.uint8) else -1)).all()) for t in outs.values())      # nothing was launched
    assert call() == 0 and call(sigma=inf, prior=0.0, iters=0, radius=8, feet=(3,), fh=-1.0) == 0
    torch.cuda.synchronize()
    assert outs["used"].tolist() == [9, 0] and outs["skate_pairs"].tolist() == [8, 0] and not outs["ok"].any() and outs["quat"].tolist() == [[1, 0, 0, 0]] * 2      # all-zero points: one point, no plane
    from manipose_amd import estimate_ground
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        estimate_ground(pts.cpu())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        estimate_ground(pts, valid=torch.ones(N, dtype=torch.uint8))


# ---- end to end: run.lift in synthetic-data mode ------------------------------------------------------------------------------------------------
COMMON = ["run.train=false", "run.test=false", "run.lift=true", "lift.stride=14", "train.batch_size_test=4", "data.seq_len=27", "model.channels=64",
          "model.layers=2", "model.nheads=4", "model.channels_seg=32", "model.layers_seg=1", "model.nheads_seg=4", "multi_hyp.n_hyp=3",
          "data.synthetic_sequences=2", "model.precision=fp32"]
NEW = ("__ground_normal", "__ground_offset", "__ground_quat", "__ground_trans", "__ground_rms", "__ground_gap", "__ground_used", "__ground_ok", "__contact",
       "__foot_height", "__skate", "__skate_pairs", "__ground_err_deg", "__ground_z")


@pytest.mark.parametrize("mode", ["fused", "placed", "placed_world"])
def test_run_lift_with_the_ground_end_to_end(tmp_path, monkeypatch, mode):
    from _entry import run
    from manipose_amd import estimate_ground
    monkeypatch.chdir(tmp_path)
    extra = {"fused": ["lift.frame=world", "lift.floor=true", "lift.fuse=true", "lift.fuse_skeleton=true"], "placed": ["lift.place=true"], "placed_world": ["lift.place=true", "lift.frame=world", "lift.floor=true"]}[mode]
    run(COMMON + extra + ["run.experiment=before"])
    run(COMMON + extra + ["run.experiment=disabled", "lift.ground=none"])
    a, b = (np.load(os.path.join(str(tmp_path), d, "lift.npz")) for d in ("before", "disabled"))
    # the option off: the file of the parent's options - the same keys in the same order, every array's dtype, shape and bytes (the zip's own
    # time stamps aside)
    assert a.files == b.files and all(a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes() for k in a.files)
    assert not any("ground" in k or "__contact" in k or "__skate" in k or "__foot_height" in k for k in a.files)
    assert not os.path.exists(os.path.join(str(tmp_path), "disabled", "lift_ground.csv"))
    assert sorted(os.listdir(os.path.join(str(tmp_path), "before"))) == sorted(os.listdir(os.path.join(str(tmp_path), "disabled")))
    run(COMMON + extra + ["run.experiment=grounded", "lift.ground=estimate", "lift.ground_speed=0.5", "lift.ground_foot_height=0.09"])
    a, z = np.load(os.path.join(str(tmp_path), "before", "lift.npz")), np.load(os.path.join(str(tmp_path), "grounded", "lift.npz"))
    keys = [f"synthetic_{i:03d}" + (".fused0" if mode == "fused" else "") for i in range(2)]
    assert sorted(set(z.files) - set(a.files)) == sorted(k + s for k in keys for s in NEW) and set(a.files) <= set(z.files)
    assert all(a[k].dtype == z[k].dtype and _same(a[k], z[k]) for k in a.files)      # nothing that was emitted before moves
    rows = open(os.path.join(str(tmp_path), "grounded", "lift_ground.csv")).read().splitlines()
    assert rows[0] == "key,frames,contacts,rms_mm,gap,err_deg,z_mm,skate_mm,skate_pairs" and [r.split(",")[0] for r in rows[1:]] == keys
    for i, k in enumerate(keys):
        n = 27 * 4 + 37 * i + 11
        shapes = dict(normal=(3,), offset=(), quat=(4,), trans=(3,), rms=(), gap=(), used=(), ok=(), err_deg=(), z=())
        for s, shape in shapes.items():
            want = np.int32 if s == "used" else np.uint8 if s == "ok" else np.float32
            assert z[f"{k}__ground_{s}"].shape == shape and z[f"{k}__ground_{s}"].dtype == want, s
        assert z[k + "__contact"].shape == z[k + "__foot_height"].shape == (n, 2) and z[k + "__contact"].dtype == np.uint8 and z[k + "__foot_height"].dtype == np.float32
        assert z[k + "__skate"].shape == z[k + "__skate_pairs"].shape == () and z[k + "__skate"].dtype == np.float32 and z[k + "__skate_pairs"].dtype == np.int32
        assert z[k + "__ground_used"] == z[k + "__contact"].sum() and rows[1 + i].split(",")[1:3] == [str(n), str(int(z[k + "__ground_used"]))]
        # the same call on the file's own arrays: the points as they were emitted
        if mode == "fused":
            pts, valid = z[k + "__skel"], z[k + "__skel_ok"] & 1
        else:
            pts, valid = (z[k] if mode == "placed_world" else z[k] + z[k + "__traj"][:, None]), z[k + "__ok"]
        want = estimate_ground(_dev(pts), None, _dev(valid), speed=0.5, foot_height=0.09)
        for s in ("normal", "offset", "quat", "trans", "rms", "gap", "used", "ok"):
            assert _same(z[f"{k}__ground_{s}"], getattr(want, s)[0].cpu().numpy()), (k, s)
        assert _same(z[k + "__contact"], want.contact.cpu().numpy()) and _same(z[k + "__foot_height"], want.height.cpu().numpy())
        assert _same(z[k + "__skate"], want.skate[0].cpu().numpy()) and _same(z[k + "__skate_pairs"], want.skate_pairs[0].cpu().numpy())
        if z[k + "__ground_ok"] & 1:
            cam = z[k + "__cam"] if mode != "fused" else None
            up = np.array([0.0, 0.0, 1.0])
            if mode == "placed":                                          # a camera's frame: its rotation's up, R^T z
                w, x, y, zz = cam[9:13].astype(np.float64) / np.linalg.norm(cam[9:13])
                up = np.array([2 * (x * zz - w * y), 2 * (y * zz + w * x), 1 - 2 * (x * x + y * y)])
            angle = np.degrees(np.arccos(np.clip(z[k + "__ground_normal"].astype(np.float64) @ up, -1, 1)))
            assert abs(angle - z[k + "__ground_err_deg"]) <= 1e-3 and 0 <= z[k + "__ground_err_deg"] <= 180

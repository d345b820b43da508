"""mp_lift_euler on the device against the float64 statement of its rule (lift_euler_ref.py), its exact cases, its invariants, its argument checks,
the closure through a written BVH file, and run.lift with lift.bvh.

The bounds, none measured from the kernels.  Canonical pass: ok equal; every angle (degrees) and every pos coordinate within ONE float32 ulp of
max(|statement|, 1) - fp64 library differences of about 1e-16 are amplified by at most 1 / sqrt(c2) (test_lift_euler_host.py asserts c2 >= 1e-6 on
every case and derives the allowance), which stays orders of magnitude below that ulp.  Continuous pass: the statement's sequential walk applied to
the DEVICE'S OWN canonical output equals the device's continuous output bit for bit (integer decisions on identical float32 inputs), and against
the statement end to end it agrees within the same ulp bound.  Closure: the positions an independent reader gets out of the written file against
pose_from_rotations on the same triple, within 4 x the float32 rounding error of the float64 statement's positions (lift_retime_ref.fk, moved by
basis, shift and scale), floor 1e-7 m x scale - mp_lift_fk's bound.
End to end the files are read back against positions below one metre, where that bound (1.2e-7 m) is smaller than what float32 DEGREES can hold:
an angle below 256 degrees is known to 7.6e-6 degrees, 1.3e-7 radians, a channel, which a lever of a metre turns into 1.3e-7 m.  The bound there
is lift_euler_ref.format_bound - every node's three half ulps times the tree path below it, from the stored angles and the bone table alone - plus
the rounding of the positions compared against (once for the float64 statement, twice for a float32 array of the device); against the emitted
poses, which are not the forward kinematics of the emitted float32 quaternions but what those were measured from, a node gets 2^-23 radians more.
Measured on an MI355X when written: see the docstrings of the tests."""
import os
import sys

import numpy as np
import pytest
import torch

import lift_euler_ref as ref
import lift_retime_ref as rt
import lift_rot_ref as rot
from lift_fixtures import same as _same

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dev(a):
    return None if a is None else torch.from_numpy(np.array(a, order="C")).cuda()      # (a copy: the cached scenes are read-only)


def _np(t):
    return None if t is None else t.cpu().numpy()


def _ulp32(x):
    return np.spacing(np.maximum(np.abs(np.asarray(x, np.float64)), 1.0).astype(np.float32)).astype(np.float64)


def _euler(sc, basis, shift, scale, order, continuous, flat=False, off=None):
    from manipose_amd import euler_from_rotations
    q, r, v = sc["quat"], sc["root"], sc["valid"]
    if flat:
        q, r, v = q[:, 0], None if r is None else r[:, 0], None if v is None else v[:, 0]
    got = euler_from_rotations(_dev(q), _dev(r), _dev(v), sc["off"] if off is None else off, order, continuous, basis, shift, scale)
    torch.cuda.synchronize()
    return got


@pytest.mark.parametrize("case", [c[0] for c in ref.cases()])
def test_euler_against_the_fp64_statement(lib, case):
    """Measured on an MI355X when written, the worst of the twelve cases: canonical angles 0.500 float32 ulp of max(|angle|, 1) (bound 1), pos
    0.500 ulp (bound 1): one rounding of the statement's value; continuous angles against the statement end to end 0.000 ulp (bound 1): the same bits;
    the walk on the device's own canonical angles reproduces the device's continuous angles bit for bit on every case."""
    _, kind, inner, order, with_basis, with_root, with_valid, scale = next(c for c in ref.cases() if c[0] == case)
    sc, basis, shift = ref.scene_of(case)
    want = ref.solved(case)
    flat = inner == 1
    canon = _euler(sc, basis, shift, scale, order, False, flat)
    assert canon.angles.dtype == torch.float32 and canon.ok.dtype == torch.uint8 and (canon.pos is None) == (not with_root)
    assert canon.angles.shape == (sc["quat"][:, 0] if flat else sc["quat"]).shape[:-1] + (3,)
    ok = _np(canon.ok).reshape(want["ok"].shape)
    a = _np(canon.angles).reshape(want["angles"].shape)
    assert np.array_equal(ok, want["ok"])
    ea = float((np.abs(a.astype(np.float64) - want["angles"]) / _ulp32(want["angles"])).max())
    ep = 0.0
    if with_root:
        p = _np(canon.pos).reshape(want["pos"].shape)
        ep = float((np.abs(p.astype(np.float64) - want["pos"]) / _ulp32(want["pos"])).max())
        assert not p[ok == 0].any()
    assert not a[ok == 0].any() and not np.signbit(a[a == 0]).any()       # no result: +0; a computed zero: +0
    cont = _euler(sc, basis, shift, scale, order, True, flat)
    c = _np(cont.angles).reshape(a.shape)
    assert _same(_np(cont.ok), _np(canon.ok)) and (not with_root or _same(_np(cont.pos), _np(canon.pos)))
    walked = ref.continuity(a, ok, sc["off"])
    ec = float((np.abs(c.astype(np.float64) - want["stored"].astype(np.float64)) / _ulp32(want["stored"])).max())
    print(f"\n[{case}] canonical angles {ea:.3f} float32 ulp of max(|angle|, 1) (bound 1), pos {ep:.3f} ulp (bound 1), continuous against the statement "
          f"{ec:.3f} ulp (bound 1); {int((ok == 0).sum())} poses without a result, largest |angle| {float(np.abs(c).max()):.0f} degrees; the walk on the device's "
          f"canonical angles {'equals' if _same(walked, c) else 'DIFFERS FROM'} the device's continuous angles")
    assert ea <= 1.0 and ep <= 1.0
    assert _same(walked, c)
    assert ec <= 1.0


@pytest.mark.parametrize("order", ref.ORDERS)
def test_euler_constructed_cases_bit_for_bit(lib, order):
    """Exact gimbal poses, half turns, a zero quaternion, a NaN, an invalid frame between two flips: arithmetic that is exact in binary"""
    q, valid, off = ref.exact_scene()
    want = ref.solve(q, None, valid, off, None, None, 1.0, order, ref.CONTINUOUS)
    sc = dict(quat=q, root=None, valid=valid, off=off)
    canon, cont = _euler(sc, None, None, 1.0, order, False), _euler(sc, None, None, 1.0, order, True)
    assert np.array_equal(_np(canon.ok), want["ok"]) and np.array_equal(_np(cont.ok), want["ok"])
    assert (want["ok"] == 3).any() and (want["ok"][[3, 5, 7], 0] == 0).all() and int((want["ok"] == 0).sum()) == 3
    assert _same(_np(canon.angles), want["canonical"]) and _same(_np(cont.angles), want["stored"])
    assert float(np.abs(want["stored"]).max()) >= 360.0                   # whole turns pile up over the half turns


@pytest.mark.parametrize("order", ref.ORDERS)
def test_euler_zero_from_the_float32_rounding_is_plus_zero(lib, order):
    """Quaternions (1, 0, +-1e-30, +-1e-30): matrix entries of +-2e-60 give angles of about +-1e-58 degrees, which underflow in the rounding to
    float32; a negative one must not be stored as -0.  Bit for bit against the statement, in both passes."""
    rows = [(1, 0, a, b) for a in (1e-30, -1e-30) for b in (1e-30, -1e-30)] + [(1, a, b, 0) for a in (1e-30, -1e-30) for b in (1e-30, -1e-30)]
    q = np.zeros((len(rows), 1, 2, 4), np.float32)
    q[:, 0, 0], q[:, 0, 1] = np.array(rows, np.float32), np.array(rows[::-1], np.float32)
    root = np.tile(np.array([[-1e-30, 1e-30, 0.0]], np.float32), (len(rows), 1, 1)) * np.float32(1e-10)
    off = np.array([0, len(rows)], np.int64)
    want = ref.solve(q, root, None, off, None, None, 1e-10, order, ref.CONTINUOUS)
    sc = dict(quat=q, root=root, valid=None, off=off)
    for continuous, key in ((False, "canonical"), (True, "stored")):
        got = _euler(sc, None, None, 1e-10, order, continuous)
        a, p = _np(got.angles), _np(got.pos)
        assert _same(a, want[key]) and (a == 0).any() and not np.signbit(a[a == 0]).any()
        assert _same(p, want["pos"].astype(np.float32) + np.float32(0.0)) and not p.any() and not np.signbit(p).any()
    assert (want["angles"] < 0).any() and (want["canonical"][want["angles"] < 0] == 0).any()      # negative values that rounded to zero exist


def _raw(lib, q, r, v, off, S, basis, shift, scale, order, flags, outs):
    p = lambda x: None if x is None else x.data_ptr()
    ntot, inner, J = q.shape[:3]
    return lib.mp_lift_euler(p(q), p(r), p(v), ntot, inner, J, p(off), S, p(basis), p(shift), scale, order, flags, *(p(t) for t in outs), None)


def test_euler_survives_a_seq_offset_it_cannot_trust(lib):
    """seq_offset is device data no host check sees: every frame range is clamped, every sequence index lies in 0 .. S-1.  Outputs sit between guard
    bytes, which must keep their pattern."""
    sc = ref.take("h36m", 5, (40, 60), seed=9)
    q, r, v = _dev(sc["quat"]), _dev(sc["root"]), _dev(sc["valid"])
    ntot, inner, J, S = 100, 5, 17, 2
    basis, shift = (_dev(t) for t in ref.transform(S, 1))
    G = 1024
    fa = torch.full((G + ntot * inner * J * 3 + G,), -7.0, device="cuda")
    fp = torch.full((G + ntot * inner * 3 + G,), -7.0, device="cuda")
    bk = torch.full((G + ntot * inner + G,), 99, dtype=torch.uint8, device="cuda")
    outs = [fa[G:-G], fp[G:-G], bk[G:-G]]
    for off in ([0, 40, 100], [-5, 40, 10 ** 12], [70, 20, 50], [10 ** 15, -10 ** 15, 3], [2 ** 62, -2 ** 62, 2 ** 62], [0, 0, 0], [100, 100, 100]):
        fa.fill_(-7.0)
        fp.fill_(-7.0)
        bk.fill_(99)
        rc = _raw(lib, q, r, v, torch.tensor(off, dtype=torch.int64, device="cuda"), S, basis, shift, 100.0, 4, 1, outs)
        assert rc == 0, lib.mp_last_error()
        torch.cuda.synchronize()
        assert bool((fa[:G] == -7).all()) and bool((fa[-G:] == -7).all()) and bool((fp[:G] == -7).all()) and bool((fp[-G:] == -7).all())
        assert bool((bk[:G] == 99).all()) and bool((bk[-G:] == 99).all())
        assert bool((outs[2] <= 3).all()) and not bool(outs[0][(outs[2] == 0).view(-1, 1).expand(-1, J * 3).reshape(-1)].any())      # every ok byte was written
        if all(b >= a for a, b in zip(off, off[1:])):                      # a table that does not decrease: the rule says what comes out
            want = ref.solve(sc["quat"], sc["root"], sc["valid"], off, _np(basis), _np(shift), 100.0, "ZXY", ref.CONTINUOUS)
            assert np.array_equal(_np(outs[2]).reshape(ntot, inner), want["ok"])
            got = _np(outs[0]).reshape(want["stored"].shape)
            assert float((np.abs(got.astype(np.float64) - want["stored"]) / _ulp32(want["stored"])).max()) <= 1.0


def test_euler_invariants(lib):
    from manipose_amd import euler_from_rotations
    sc = ref.take("h36m", 1, seed=5)
    off = sc["off"]
    basis, shift = ref.transform(len(ref.LENS), 2)
    q, r, v = _dev(sc["quat"][:, 0]), _dev(sc["root"][:, 0]), _dev(sc["valid"][:, 0])
    for order, continuous in (("ZXY", True), ("XYZ", True), ("YZX", False)):
        a = euler_from_rotations(q, r, v, off, order, continuous, basis, shift, 100.0)
        b = euler_from_rotations(q, r, v, torch.from_numpy(off).cuda(), order, continuous, torch.from_numpy(basis), torch.from_numpy(shift), 100.0)
        assert all(_same(_np(x), _np(y)) for x, y in zip(a, b))           # two calls, a device table, tensor tables: identical bits
        f0 = 0
        for s, n in enumerate(ref.LENS):                                  # a sequence alone equals the same sequence among the others
            alone = euler_from_rotations(q[f0:f0 + n].contiguous(), r[f0:f0 + n].contiguous(), v[f0:f0 + n].contiguous(), None, order, continuous, basis[s], shift[s], 100.0)
            assert all(_same(_np(x), _np(y)[f0:f0 + n]) for x, y in zip(alone, a)), (order, s)
            f0 += n
    poisoned = sc["quat"][:, 0].copy()                                    # an invalid frame is transparent, whatever it holds
    poisoned[sc["valid"][:, 0] == 0] = np.nan
    c = euler_from_rotations(_dev(poisoned), r, v, off, "XYZ", True, basis, shift, 100.0)
    a = euler_from_rotations(q, r, v, off, "XYZ", True, basis, shift, 100.0)
    assert all(_same(_np(x), _np(y)) for x, y in zip(a, c))
    plain = euler_from_rotations(q, None, v, off, "XYZ", True, basis, shift, 100.0)
    assert plain.pos is None and _same(_np(plain.angles), _np(a.angles)) and _same(_np(plain.ok), _np(a.ok))
    ident = euler_from_rotations(q, r, v, off, "XYZ", True, np.array([2.0, 0, 0, 0], np.float32), None, 1.0)      # the identity, given or not
    none = euler_from_rotations(q, r, v, off, "XYZ", True, None, None, 1.0)
    assert all(_same(_np(x), _np(y)) for x, y in zip(ident, none))
    dead = euler_from_rotations(q, r, v, off, "XYZ", True, np.zeros(4, np.float32), None, 1.0)                      # an unusable basis: no pose has a result
    assert not bool(dead.ok.any()) and not bool(dead.angles.any()) and not bool(dead.pos.any())


def test_entry_point_rejects_bad_arguments_before_any_launch(lib):
    N, inner, J, S = 12, 2, 17, 2
    q = torch.zeros(N, inner, J, 4, device="cuda")
    q[..., 0] = 1
    r = torch.zeros(N, inner, 3, device="cuda")
    off = torch.tensor([0, 5, N], dtype=torch.int64, device="cuda")
    basis, shift = torch.zeros(S, 4, device="cuda"), torch.zeros(S, 3, device="cuda")
    basis[:, 0] = 1
    outs = dict(angles=torch.full((N, inner, J, 3), -1.0, device="cuda"), pos=torch.full((N, inner, 3), -1.0, device="cuda"),
                ok=torch.full((N, inner), 77, dtype=torch.uint8, device="cuda"))

    for kw in (dict(x=None), dict(o=None), dict(angles=None), dict(ok=None)):
        p = lambda x: None if x is None else x.data_ptr()
        o_ = {k: kw.get(k, v) for k, v in outs.items()}
        rc = lib.mp_lift_euler(p(kw.get("x", q)), p(r), None, N, inner, J, p(kw.get("o", off)), S, p(basis), p(shift), 1.0, 4, 1, *(p(o_[k]) for k in outs), None)
        assert rc == 1 and b"null" in lib.mp_last_error(), (kw, lib.mp_last_error())
    misaligned = torch.zeros(N * inner * J * 4 + 4, device="cuda")[1:-3].view(N, inner, J, 4)
    for kw, word in ((dict(root=None), b"both or neither"), (dict(pos=None), b"both or neither"), (dict(b=None), b"both or neither"), (dict(t=None), b"both or neither"),
                     (dict(order=-1), b"order=-1"), (dict(order=6), b"order=6"), (dict(flags=2), b"flags=2"), (dict(scale=0.0), b"scale="), (dict(scale=-1.0), b"scale="),
                     (dict(scale=float("inf")), b"scale="), (dict(scale=float("nan")), b"scale="), (dict(x=misaligned), b"16-byte aligned"),
                     (dict(pos=r), b"overlaps an input"), (dict(angles=q.view(-1)[:N * inner * J * 3].view(N, inner, J, 3)), b"overlaps an input"),
                     (dict(pos=outs["angles"].view(-1)[:N * inner * 3].view(N, inner, 3)), b"two outputs overlap")):
        p = lambda x: None if x is None else x.data_ptr()
        o_ = {k: kw.get(k, v) for k, v in outs.items()}
        a = dict(x=q, root=r, b=basis, t=shift, scale=1.0, order=4, flags=1)
        a.update({k: v for k, v in kw.items() if k in a})
        rc = lib.mp_lift_euler(p(a["x"]), p(a["root"]), None, N, inner, J, p(off), S, p(a["b"]), p(a["t"]), a["scale"], a["order"], a["flags"], *(p(o_[k]) for k in outs), None)
        assert rc == 1 and word in lib.mp_last_error(), (kw, lib.mp_last_error())
    for (n, i, j, s), word in (((N, inner, 1, S), b"J=1"), ((N, inner, 33, S), b"J=33"), ((0, inner, J, S), b"out of range"), ((N, 0, J, S), b"out of range"),
                               ((N, inner, J, 0), b"out of range"), ((N, inner, J, 13), b"out of range"), ((2 ** 40, 2 ** 10, J, S), b"too many for one launch")):
        p = lambda x: x.data_ptr()
        rc = lib.mp_lift_euler(p(q), p(r), None, n, i, j, p(off), s, p(basis), p(shift), 1.0, 4, 1, *(p(outs[k]) for k in outs), None)
        assert rc == 1 and word in lib.mp_last_error(), ((n, i, j, s), lib.mp_last_error())
    torch.cuda.synchronize()
    assert all(bool((t == (77 if t.dtype == torch.uint8 else -1)).all()) for t in outs.values())      # nothing was launched
    p = lambda x: None if x is None else x.data_ptr()
    assert lib.mp_lift_euler(p(q), p(r), None, N, inner, J, p(off), S, p(basis), p(shift), 1.0, 4, 1, *(p(outs[k]) for k in outs), None) == 0
    assert lib.mp_lift_euler(p(q), None, None, N, inner, J, p(off), S, None, None, 100.0, 0, 0, p(outs["angles"]), None, p(outs["ok"]), None) == 0
    torch.cuda.synchronize()
    assert bool((outs["ok"] == 1).all()) and not bool(outs["angles"].any()) and not bool(outs["pos"].any())
    from manipose_amd import euler_from_rotations
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        euler_from_rotations(q.cpu())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        euler_from_rotations(q, r.cpu())
    with pytest.raises(ValueError, match="order must be"):
        euler_from_rotations(q, order="ZXZ")


@pytest.mark.parametrize("order,continuous,with_basis,scale", [("ZXY", True, True, 100.0), ("XYZ", False, False, 1.0), ("YZX", True, True, 1.0)])
def test_written_file_reads_back_to_the_forward_kinematics(lib, tmp_path, order, continuous, with_basis, scale):
    """Measured on an MI355X when written: see the host test of the same closure (test_lift_euler_host.py) - the device's angles are the
    statement's but for single roundings, and the figures were the same to three digits."""
    from manipose_amd import euler_from_rotations, pose_from_rotations
    from manipose_amd.bvh import write_bvh
    sc = ref.closure_take()
    sk = ref.named_h36m()
    basis, shift = ref.transform(1, 4) if with_basis else (None, None)
    q, r, v = _dev(sc["quat"][:, 0]), _dev(sc["root"][:, 0]), _dev(sc["valid"][:, 0])
    e = euler_from_rotations(q, r, v, None, order, continuous, None if basis is None else basis[0], None if shift is None else shift[0], scale)
    poses, pok = pose_from_rotations(q, sc["bones"], r)
    path = os.path.join(str(tmp_path), "take.bvh")
    assert write_bvh(path, sk, sc["bones"], e.angles, e.pos, e.ok, 50, order, scale)
    got = ref.bvh_joints(ref.read_bvh(path), rot.H36M_PARENTS)
    want = ref.moved(_np(poses).astype(np.float64), None if basis is None else basis[0], None if shift is None else shift[0], scale)
    live = _np(e.ok) != 0
    assert bool(pok.all()) and np.array_equal(live, sc["valid"][:, 0] != 0) and live.sum() > 100
    stated, _ = rt.fk(sc["quat"], sc["bones"][None], rot.H36M_PARENTS, rot.H36M_REST, sc["root"], [0, len(live)])      # float64: its rounding sets the bound
    bound = ref.closure_bound(ref.moved(stated[:, 0], None if basis is None else basis[0], None if shift is None else shift[0], scale)[live], scale)
    err = float(np.abs(got[live] - want[live]).max())
    print(f"\n[closure {order} continuous={continuous} basis={with_basis} scale={scale:g}] |file - pose_from_rotations| = {err:.3e}, bound {bound:.3e} ({err / bound:.3f}); "
          f"largest |angle| {float(e.angles.abs().max()):.0f} degrees")
    assert err <= bound
    src = ref.row_sources(live)
    assert np.array_equal(got, got[src])                                  # a frame without a result repeats the last one before it that has one


# ---- end to end: run.lift in synthetic-data mode ------------------------------------------------------------------------------------------------
COMMON = ["run.train=false", "run.test=false", "run.lift=true", "lift.stride=14", "train.batch_size_test=4", "data.seq_len=27", "model.channels=64",
          "model.layers=2", "model.nheads=4", "model.channels_seg=32", "model.layers_seg=1", "model.nheads_seg=4", "multi_hyp.n_hyp=3",
          "data.synthetic_sequences=2", "model.precision=fp32", "lift.rigid=true", "lift.rotations=true"]
NEW = ("__bvh_euler", "__bvh_pos", "__bvh_ok")


def test_run_lift_with_bvh_end_to_end(tmp_path, monkeypatch):
    sys.path.insert(0, os.path.join(ROOT, "hpe"))
    from _entry import run
    monkeypatch.chdir(tmp_path)
    run(COMMON + ["run.experiment=absent"])
    run(COMMON + ["run.experiment=bvhoff", "lift.bvh=false"])
    run(COMMON + ["run.experiment=plain", "lift.bvh=true", "lift.bvh_up=z", "lift.bvh_scale=1", "lift.bvh_order=XYZ", "lift.bvh_fps=25"])
    run(COMMON + ["run.experiment=rt", "lift.bvh=true", "lift.retime_fps=30", "lift.retime_radius=2"])
    load = lambda d: np.load(os.path.join(str(tmp_path), d, "lift.npz"))
    a, b, z, w = (load(d) for d in ("absent", "bvhoff", "plain", "rt"))
    keys = [f"synthetic_{i:03d}" for i in range(2)]
    assert not any("__bvh" in k for k in a.files) and sorted(a.files) == sorted(b.files)
    assert all(a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes() for k in a.files)         # the key absent and the key false: the same bytes
    assert not os.path.exists(os.path.join(str(tmp_path), "absent", "bvh")) and not os.path.exists(os.path.join(str(tmp_path), "bvhoff", "bvh"))
    assert sorted(set(z.files) - set(a.files)) == sorted(k + s for k in keys for s in NEW)
    assert all(a[k].dtype == z[k].dtype and a[k].tobytes() == z[k].tobytes() for k in a.files)         # every earlier key keeps its bytes
    assert sorted(os.listdir(os.path.join(str(tmp_path), "plain", "bvh"))) == [k + ".bvh" for k in keys] == sorted(os.listdir(os.path.join(str(tmp_path), "rt", "bvh")))
    for k in keys:
        # z up, metres, at the input's rate: the file is the emitted (origin, "__quat", "__bones"), and so the emitted poses
        f = ref.read_bvh(os.path.join(str(tmp_path), "plain", "bvh", k + ".bvh"))
        N = len(z[k])
        assert f["frames"] == N and abs(f["frame_time"] - 1 / 25) < 1e-9 and f["nodes"][0]["channels"][3:] == ["Xrotation", "Yrotation", "Zrotation"]
        assert z[k + "__bvh_euler"].shape == (N, 17, 3) and z[k + "__bvh_pos"].shape == (N, 3) and z[k + "__bvh_ok"].shape == (N,) and z[k + "__bvh_ok"].dtype == np.uint8
        live = z[k + "__bvh_ok"] != 0
        assert np.array_equal(live, z[k + "__quat_ok"] != 0) and live.any()
        got = ref.bvh_joints(f, rot.H36M_PARENTS)
        want = z[k].astype(np.float64)
        back, _ = rt.fk(z[k + "__quat"][:, None], z[k + "__bones"][None], rot.H36M_PARENTS, rot.H36M_REST, None, [0, N])      # float64: its rounding sets the bound
        err, err_fk = float(np.abs(got[live] - want[live]).max()), float(np.abs(got[live] - back[live, 0]).max())
        fmt = ref.format_bound(z[k + "__bvh_euler"][live], rot.H36M_PARENTS, z[k + "__bones"], 1.0)
        emitted = ref.format_bound(z[k + "__bvh_euler"][live], rot.H36M_PARENTS, z[k + "__bones"], 1.0, node_eps=2.0 ** -23)
        rounding = ref.closure_bound(back[live, 0], 1.0)
        print(f"\n[{k} plain] |file - fk of the emitted triple| = {err_fk:.3e} m (float32 degrees allow {fmt:.3e} + {rounding:.3e}), |file - emitted poses| = {err:.3e} m "
              f"(with float32 quaternions {emitted:.3e} + {2 * rounding:.3e})")
        assert err_fk <= fmt + rounding and err <= emitted + 2 * rounding
        # y up, centimetres, retimed to 30 fps: the file is ("__rt_quat", "__bones") and so "__rt", turned (x, y, z) -> (x, z, -y) and scaled
        f = ref.read_bvh(os.path.join(str(tmp_path), "rt", "bvh", k + ".bvh"))
        M = len(w[k + "__rt"])
        assert f["frames"] == M and abs(f["frame_time"] - 1 / 30) < 1e-9 and f["nodes"][0]["channels"][3:] == ["Zrotation", "Xrotation", "Yrotation"]
        live = w[k + "__bvh_ok"] != 0
        assert np.array_equal(live, (w[k + "__rt_ok"] & 1) != 0) and live.any()
        p = w[k + "__rt"].astype(np.float64)
        want = 100.0 * np.stack([p[..., 0], p[..., 2], -p[..., 1]], -1)
        got = ref.bvh_joints(f, rot.H36M_PARENTS)
        back, _ = rt.fk(w[k + "__rt_quat"][:, None], w[k + "__bones"][None], rot.H36M_PARENTS, rot.H36M_REST, None, [0, M])
        rounding = ref.closure_bound(100.0 * np.stack([back[..., 0], back[..., 2], -back[..., 1]], -1)[live, 0], 100.0)
        fmt = ref.format_bound(w[k + "__bvh_euler"][live], rot.H36M_PARENTS, w[k + "__bones"], 100.0)
        err = float(np.abs(got[live] - want[live]).max())
        print(f"[{k} retimed] |file - __rt| = {err:.3e} cm (float32 degrees allow {fmt:.3e} + {2 * rounding:.3e})")
        assert err <= fmt + 2 * rounding

"""mp_lift_fk and mp_lift_retime on the device against the float64 statements of their rules (lift_retime_ref.py), their exact cases, their
invariants, their argument checks, and run.lift with lift.retime_fps.

The bounds, none measured from the kernels.  mp_lift_fk: |poses - statement| <= 4 x the statement's own float32 rounding error (the largest
|float32(p) - p| over the scene), floor 1e-7 m - test_gpu_lift_rot.py's bound for the same closure.  mp_lift_retime: ok and taps equal; every
component of quat_out within 2^-23 of the statement (both sides round the same component of a unit quaternion, known to about 1e-13 given the
margins test_lift_retime_host.py asserts, to float32); root_out within ONE float32 ulp of the statement's value; copied frames bit for bit.  Bones of
the retimed positions: within 2 float32 ulp of the largest |coordinate| of the positions - each end of a bone is rounded once, half an ulp a
coordinate, so the bone vector errs by at most one ulp a coordinate and its length by at most sqrt(3) < 2 (lift_footlock's bone bound).
Measured on an MI355X when written: see the docstrings of the tests."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch

import lift_retime_ref as ref
import lift_rot_ref as rot
from lift_fixtures import same as _same

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLOOR = 1e-7                    # metres: the floor of the forward-kinematics bound
TAPERS = ("uniform", "biweight")


def _dev(a):
    return None if a is None else torch.from_numpy(np.array(a, order="C")).cuda()      # (a copy: the cached scenes are read-only)


def _np(t):
    return None if t is None else t.cpu().numpy()


def _ulp32(x):
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(np.float32)).astype(np.float64)


# ---- mp_lift_fk ------------------------------------------------------------------------------------------------------------------------------
FK_LENS = (1, 2, 67, 130)


@functools.lru_cache(maxsize=None)
def _fk_scene(kind, inner):
    parents, rest = rot.skeleton(kind)
    J = len(parents)
    g = np.random.default_rng(7 + J + inner)
    ntot = sum(FK_LENS)
    q = (rot._random_rotations(g, (ntot, inner, J), np.pi) * g.uniform(0.5, 2.0, (ntot, inner, J, 1))).astype(np.float32)
    root = (g.uniform(-1, 1, (ntot, inner, 3)) + [0, 0, 4.0]).astype(np.float32)
    off = np.concatenate([[0], np.cumsum(FK_LENS)]).astype(np.int64)
    per_seq = g.uniform(0.1, 0.5, (len(FK_LENS), J - 1)).astype(np.float32)
    per_pose = g.uniform(0.1, 0.5, (ntot, inner, J - 1)).astype(np.float32)
    for a in (q, root, per_seq, per_pose):
        a.setflags(write=False)
    return q, root, off, per_seq, per_pose, parents, rest


@pytest.mark.parametrize("kind,inner,per_pose,with_root", [("h36m", 1, False, True), ("h36m", 5, True, False), ("h36m", 5, False, False), ("pair", 5, False, True),
                                                           ("pair", 1, True, True), ("chain", 1, True, False), ("chain", 5, False, True)])
def test_fk_against_the_fp64_statement(lib, kind, inner, per_pose, with_root):
    """Measured on an MI355X when written: 0.250 of the bound on all seven scenes (5.9e-8 .. 2.4e-7 m) - the kernel's float32 is the statement's
    value rounded once, and the bound is four such roundings of the largest coordinate."""
    from manipose_amd import pose_from_rotations
    q, root, off, per_seq, per_pose_len, parents, rest = _fk_scene(kind, inner)
    sk = None if kind == "h36m" else rot.Sk(parents, rest)
    L = per_pose_len if per_pose else per_seq
    want, ok = ref.fk(q, L, parents, rest, root if with_root else None, None if per_pose else off)
    bound = max(4 * float(np.abs(want.astype(np.float32).astype(np.float64) - want).max()), FLOOR)
    flat = inner == 1                                                     # the (Ntot, J, 4) form of the public function
    tq, tr = _dev(q[:, 0] if flat else q), _dev((root[:, 0] if flat else root) if with_root else None)
    tl = _dev(L[:, 0] if flat else L) if per_pose else L
    poses, k = pose_from_rotations(tq, tl, tr, None if per_pose else off, sk)
    assert poses.shape == tq.shape[:-1] + (3,) and poses.dtype == torch.float32 and k.shape == tq.shape[:-2] and k.dtype == torch.uint8
    got = _np(poses).reshape(want.shape)
    err = float(np.abs(got.astype(np.float64) - want).max())
    print(f"\n[fk {kind} inner={inner} per_pose={per_pose} root={with_root}] |poses - statement| = {err:.3e} m, bound {bound:.3e} m ({err / bound:.3f})")
    assert np.array_equal(_np(k).reshape(ok.shape), ok) and ok.all() and err <= bound
    again = pose_from_rotations(tq, _dev(np.asarray(L)) if not per_pose else tl, tr, None if per_pose else torch.from_numpy(off).cuda(), sk)
    assert _same(_np(again[0]), _np(poses)) and _same(_np(again[1]), _np(k))      # a device table, a second call: identical bits
    if not with_root:
        assert not got[..., 0, :].any()


def test_fk_unusable_quaternions_and_closure(lib):
    """Closure measured on an MI355X when written: 1.64e-07 m against a bound of 7.04e-07 m."""
    from manipose_amd import pose_from_rotations, pose_rotations
    q, root, off, per_seq, _, parents, rest = _fk_scene("h36m", 5)
    bad = q.copy()
    bad[3, 1, 9] = 0.0
    bad[70, 4, 0, 2] = np.nan
    bad[71, 0, 16] = 1e-7                                                # |q|^2 = 4e-14 < 1e-12
    poses, ok = (_np(t) for t in pose_from_rotations(_dev(bad), per_seq, _dev(root), off))
    want, wok = ref.fk(bad, per_seq, parents, rest, root, off)
    hit = [(3, 1), (70, 4), (71, 0)]
    assert np.array_equal(ok, wok) and int((ok == 0).sum()) == 3 and all(ok[h] == 0 for h in hit)
    for h in hit:
        assert _same(poses[h], np.tile(root[h], (17, 1)))                 # every joint on the root, bit for bit
    clean, _ = (_np(t) for t in pose_from_rotations(_dev(q), per_seq, _dev(root), off))
    keep = ok != 0
    assert _same(poses[keep], clean[keep])                               # a pose depends on no other pose
    origin = _np(pose_from_rotations(_dev(bad), per_seq, None, off)[0])
    assert all(_same(origin[h], np.zeros((17, 3), np.float32)) for h in hit)
    # the closure on the device: positions -> rotations -> positions, with each pose's own measured lengths
    P, poff, par, prest = rot.random_scene("h36m", 1, 3)
    p = P[:, 0]
    tq, tok = pose_rotations(_dev(p), poff)
    L32 = rot.measured_lengths(p, par).astype(np.float32)
    back = _np(pose_from_rotations(tq, _dev(L32), _dev(p[:, 0].copy()))[0]).astype(np.float64)
    stated_q = rot.rotations(P, par, prest, poff)[0][:, 0]
    stated = float(np.abs(rot.fk_quat(stated_q, rot.measured_lengths(p, par), par, prest, p[:, 0].astype(np.float64)) - p).max())
    bound = max(4 * stated, FLOOR)
    err = float(np.abs(back - p).max())
    print(f"\n[closure] |pose_from_rotations(pose_rotations(p), measured lengths) - p| = {err:.3e} m, bound {bound:.3e} m")
    assert bool(tok.all()) and err <= bound


# ---- mp_lift_retime --------------------------------------------------------------------------------------------------------------------------
def _retime(sc, num, den, start, R, degree, taper, flat=False, **kw):
    from manipose_amd import retime_rotations
    q, r, v = sc["quat"], sc["root"], sc["valid"]
    if flat:
        q, r, v = q[:, 0], r[:, 0], None if v is None else v[:, 0]
    off = np.concatenate([[0], np.cumsum(sc["lens"])]).astype(np.int64)
    got = retime_rotations(_dev(q), _dev(r), _dev(v), kw.get("off", off), den, num, ref.starts(sc["lens"], start), R, degree, TAPERS[taper])
    torch.cuda.synchronize()
    return got


def _against(got, want, shape_q):
    q, r = _np(got.quat).reshape(shape_q), _np(got.root).reshape(want["root"].shape)
    ok, taps = _np(got.ok).reshape(want["ok"].shape), _np(got.taps).reshape(want["taps"].shape)
    assert np.array_equal(ok, want["ok"]) and np.array_equal(taps, want["taps"])
    live = (want["ok"] & 1) != 0
    eq = float(np.abs(q.astype(np.float64) - want["quat"]).max())
    er = float((np.abs(r.astype(np.float64) - want["root"]) / _ulp32(want["root"])).max())
    dead = ~live & ~want["copied"]
    ident = np.zeros(q.shape[2:], np.float32)
    ident[:, 0] = 1
    assert all(_same(x, ident) for x in q[dead]) and not r[dead].any()   # no result: identities and a zero root
    c = want["copied"]
    assert _same(q[c], want["quat"][c].astype(np.float32)) and _same(r[c], want["root"][c].astype(np.float32))
    return eq, er


@pytest.mark.parametrize("case", [c[0] for c in ref.cases()])
def test_retime_against_the_fp64_statement(lib, case):
    """Measured on an MI355X when written, the worst of the twenty cases: |quat_out - statement| = 0.250 x 2^-23 (bound 1; 0 on the identity
    clock), root_out 0.500 float32 ulp (bound 1): one rounding of the statement's value on either."""
    _, kind, inner, holes, (num, den), start, R, degree, taper = next(c for c in ref.cases() if c[0] == case)
    sc, (off, out_off, clock), want = ref.solved(case)
    got = _retime(sc, num, den, start, R, degree, taper, flat=inner == 1)
    assert np.array_equal(_np(got.seq_offset), out_off) and _same(_np(got.time), want["time"])
    assert got.quat.dtype == torch.float32 and got.ok.dtype == torch.uint8 and got.quat.shape[0] == int(out_off[-1])
    eq, er = _against(got, want, want["quat"].shape)
    print(f"\n[{case}] {int(out_off[-1])} output frames, {int((want['ok'] & 1 == 0).sum())} without a result: |quat_out - statement| = {eq / ref.TOL:.3f} x 2^-23 "
          f"(bound 1), root_out {er:.3f} float32 ulp (bound 1)")
    assert eq <= ref.TOL and er <= 1.0
    if holes == "run" and R <= 4:
        assert (want["ok"] & 1 == 0).any()                                # the hole run is longer than the window: frames without a result exist


def test_retime_exact_cases(lib):
    sc = ref.take("h36m", 5, ref.LENS, "single", seed=3)
    q, r, v = sc["quat"], sc["root"], sc["valid"]
    same_clock = _retime(sc, 1, 1, 0.0, 0, 2, 0)                          # the identity clock: the input's bits on every frame, ok = valid
    assert _same(_np(same_clock.quat), q) and _same(_np(same_clock.root), r) and np.array_equal(_np(same_clock.ok), v)
    assert bool((same_clock.taps == 1).all()) and np.array_equal(_np(same_clock.time), np.concatenate([np.arange(n) for n in ref.LENS]).astype(np.float64))
    twice = _retime(sc, 2, 1, 0.0, 0, 2, 0)                               # rate 2 / 1: every even output frame is an input frame
    out_off = _np(twice.seq_offset)
    f0 = 0
    for s, n in enumerate(ref.LENS):
        seg = slice(int(out_off[s]), int(out_off[s + 1]))
        assert out_off[s + 1] - out_off[s] == 2 * n - 1
        assert _same(_np(twice.quat)[seg][::2], q[f0:f0 + n]) and _same(_np(twice.root)[seg][::2], r[f0:f0 + n])
        odd_ok = _np(twice.ok)[seg][1::2]
        assert np.array_equal(odd_ok, v[f0:f0 + n - 1] & v[f0 + 1:f0 + n])       # a midpoint needs both its frames: nothing is filled
        f0 += n
    # a track that alternates hemisphere (frame k stored as (-1)^k q_k) interpolates the short way, in the hemisphere of the frame before
    alt = dict(sc, valid=None)
    sign = np.where(np.arange(q.shape[0]) % 2 == 0, 1.0, -1.0).astype(np.float32)[:, None, None, None]
    alt["quat"] = np.ascontiguousarray(q * sign)
    got = _retime(alt, 2, 1, 0.0, 0, 2, 0)
    plain = _retime(dict(sc, valid=None), 2, 1, 0.0, 0, 2, 0)
    gq, pq = _np(got.quat).astype(np.float64), _np(plain.quat).astype(np.float64)
    off, oo, clock = ref.plan(ref.LENS, 2, 1)
    want = ref.retime(alt["quat"], alt["root"], None, off, oo, clock, 0, 2, 0)
    assert float(np.abs(gq - want["quat"]).max()) <= ref.TOL
    f0 = 0
    for s, n in enumerate(ref.LENS):
        mid = gq[int(oo[s]):int(oo[s + 1])][1::2]
        before = alt["quat"][f0:f0 + n - 1].astype(np.float64)
        assert ((mid * ref.unit(before)).sum(-1) > 0.99).all()           # beside the frame before, on its side of the sphere
        assert (np.abs((mid * pq[int(oo[s]):int(oo[s + 1])][1::2]).sum(-1)) > 1 - 1e-6).all()      # the same rotation as without the flips
        f0 += n


def _raw_call(lib, q, r, v, off, oo, clock, S, mtot, R, degree, taper, outs):
    p = lambda x: None if x is None else x.data_ptr()
    ntot, inner, J = q.shape[:3]
    return lib.mp_lift_retime(p(q), p(r), p(v), ntot, inner, J, p(off), p(oo), p(clock), S, mtot, R, degree, taper, *(p(t) for t in outs), None)


@pytest.mark.parametrize("R", [0, 4])
def test_retime_survives_device_tables_it_cannot_trust(lib, R):
    """clock, seq_offset and out_offset are device data no host check sees: the kernel clamps every index it forms from them.  Outputs sit between
    guard bytes, which must keep their pattern."""
    sc = ref.take("h36m", 5, (40, 60), "single", seed=9)
    q, r, v = _dev(sc["quat"]), _dev(sc["root"]), _dev(sc["valid"])
    ntot, inner, J, mtot, S = 100, 5, 17, 90, 2
    G = 1024
    fq = torch.full((G + mtot * inner * J * 4 + G,), -7.0, device="cuda")
    fr = torch.full((G + mtot * inner * 3 + G,), -7.0, device="cuda")
    bk, bt = (torch.full((G + mtot * inner + G,), 99, dtype=torch.uint8, device="cuda") for _ in range(2))
    outs = [fq[G:-G], fr[G:-G], bk[G:-G], bt[G:-G]]
    nan, inf = float("nan"), float("inf")
    tables = [
        ([0, 40, 100], [0, 30, 90], [[0.0, 0.0, 5.0], [0.0, -3.0, 5.0]]),                                   # num = 0 and < 0: taken as 1
        ([-5, 40, 10 ** 12], [-9, 30, 10 ** 12], [[-4.0, 3.0, 5.0], [1e9, 3.0, 5.0]]),                     # offsets beyond the arrays, start outside
        ([70, 20, 50], [80, 10, 5], [[nan, nan, nan], [inf, 1.0, -inf]]),                                   # decreasing offsets, NaN and inf clocks
        ([10 ** 15, -10 ** 15, 3], [2 ** 62, -2 ** 62, 2 ** 62], [[0.25, 1e300, 1e-300], [0.0, 1e-300, 1e300]]),
    ]
    for off, oo, clock in tables:
        for t in (fq, fr):
            t.fill_(-7.0)
        bk.fill_(99)
        bt.fill_(99)
        rc = _raw_call(lib, q, r, v, torch.tensor(off, dtype=torch.int64, device="cuda"), torch.tensor(oo, dtype=torch.int64, device="cuda"),
                       torch.tensor(clock, dtype=torch.float64, device="cuda"), S, mtot, R, 2, 1, outs)
        assert rc == 0, lib.mp_last_error()
        torch.cuda.synchronize()
        assert bool((fq[:G] == -7).all()) and bool((fq[-G:] == -7).all()) and bool((fr[:G] == -7).all()) and bool((fr[-G:] == -7).all())
        assert bool((bk[:G] == 99).all()) and bool((bk[-G:] == 99).all()) and bool((bt[:G] == 99).all()) and bool((bt[-G:] == 99).all())
        assert bool((outs[2] <= 3).all()) and bool((outs[3] <= 2 * R + 1 if R else outs[3] <= 2).all())     # every output byte was written
        if all(b >= a for a, b in zip(off, off[1:])) and all(b >= a for a, b in zip(oo, oo[1:])):      # tables that do not decrease: the rule says what comes out
            want = ref.retime(sc["quat"], sc["root"], sc["valid"], off, oo, np.array(clock), R, 2, 1, mtot=mtot)
            assert np.array_equal(_np(outs[2]).reshape(mtot, inner), want["ok"]) and np.array_equal(_np(outs[3]).reshape(mtot, inner), want["taps"])
            assert (want["ok"] & 2).any()                                 # frames whose time had to be clamped


def test_retime_invariants(lib):
    """Bones measured on an MI355X when written: at most 0.943 float32 ulp of the largest coordinate (bound 2)."""
    from manipose_amd import pose_from_rotations, retime_rotations, smooth_rotations
    sc = ref.take("h36m", 1, ref.LENS, "single", seed=5)
    off = np.concatenate([[0], np.cumsum(ref.LENS)]).astype(np.int64)
    bones = np.random.default_rng(3).uniform(0.1, 0.5, (len(ref.LENS), 16)).astype(np.float32)
    q, r, v = _dev(sc["quat"][:, 0]), _dev(sc["root"][:, 0]), _dev(sc["valid"][:, 0])
    for num, den, R in ((3, 5, 4), (6, 5, 0), (1, 1, 4)):
        a = retime_rotations(q, r, v, off, den, num, 0.0, R, 2, "biweight")
        b = retime_rotations(q, r, v, torch.from_numpy(off).cuda(), den, num, 0.0, R, 2, "biweight")
        assert all(_same(_np(x), _np(y)) for x, y in zip(a, b))           # two calls, a device table: identical bits
        poses, pok = pose_from_rotations(a.quat, bones, a.root, a.seq_offset)
        p = _np(poses).astype(np.float64)
        live = (_np(a.ok) & 1) != 0
        assert bool(pok.all()) and live.any()
        oo = _np(a.seq_offset)
        worst = 0.0
        for s in range(len(ref.LENS)):
            seg = slice(int(oo[s]), int(oo[s + 1]))
            m = live[seg]
            if m.any():
                scale = _ulp32(np.abs(p[seg][m]).max())
                worst = max(worst, float((np.abs(rot.measured_lengths(p[seg][m], rot.H36M_PARENTS) - bones[s].astype(np.float64)) / scale).max()))
        print(f"\n[bones {num}/{den} R={R}] the retimed positions' bones are off the table by at most {worst:.3f} float32 ulp of the largest coordinate (bound 2)")
        assert worst <= 2.0
        f0 = 0
        for s, n in enumerate(ref.LENS):                                  # a sequence alone equals the same sequence inside the five-sequence call
            alone = retime_rotations(q[f0:f0 + n].contiguous(), r[f0:f0 + n].contiguous(), v[f0:f0 + n].contiguous(), None, den, num, 0.0, R, 2, "biweight")
            seg = slice(int(oo[s]), int(oo[s + 1]))
            assert all(_same(_np(x), _np(y)[seg]) for x, y in zip(alone[:4], a[:4])) and _same(_np(alone.time), _np(a.time)[seg]), s
            f0 += n
    sm = smooth_rotations(q, r, v, off, 4, 2, "biweight")                 # the name for fps_in == fps_out, start 0
    assert all(_same(_np(x), _np(y)) for x, y in zip(sm, a))
    poisoned = sc["quat"][:, 0].copy()                                    # an invalid frame's value never enters the arithmetic
    poisoned[sc["valid"][:, 0] == 0] = np.nan
    c = retime_rotations(_dev(poisoned), r, v, off, 1, 1, 0.0, 4, 2, "biweight")
    assert _same(_np(c.quat), _np(a.quat)) and _same(_np(c.root), _np(a.root))
    no_root = retime_rotations(q, None, v, off, 5, 3, 0.0, 4, 2, "biweight")
    with_root = retime_rotations(q, r, v, off, 5, 3, 0.0, 4, 2, "biweight")
    assert no_root.root is None and _same(_np(no_root.quat), _np(with_root.quat)) and _same(_np(no_root.ok), _np(with_root.ok))


def test_entry_points_reject_bad_arguments_before_any_launch(lib):
    N, M, inner, J, S = 12, 20, 2, 17, 2
    q = torch.zeros(N, inner, J, 4, device="cuda")
    q[..., 0] = 1
    r = torch.zeros(N, inner, 3, device="cuda")
    off = torch.tensor([0, 5, N], dtype=torch.int64, device="cuda")
    oo = torch.tensor([0, 9, M], dtype=torch.int64, device="cuda")
    clock = torch.tensor([[0.0, 2.0, 1.0]] * 2, dtype=torch.float64, device="cuda")
    outs = dict(quat_out=torch.full((M, inner, J, 4), -1.0, device="cuda"), root_out=torch.full((M, inner, 3), -1.0, device="cuda"),
                ok=torch.full((M, inner), 77, dtype=torch.uint8, device="cuda"), taps=torch.full((M, inner), 77, dtype=torch.uint8, device="cuda"))
    p = lambda x: None if x is None else x.data_ptr()

    def call(x=q, root=r, o=off, o2=oo, ck=clock, n=N, i=inner, j=J, s=S, m=M, R=0, deg=2, tp=0, **repl):
        o_ = {k: repl.get(k, t) for k, t in outs.items()}
        return lib.mp_lift_retime(p(x), p(root), None, n, i, j, p(o), p(o2), p(ck), s, m, R, deg, tp, *(p(o_[k]) for k in outs), None)
    for kw in (dict(x=None), dict(o=None), dict(o2=None), dict(ck=None), dict(quat_out=None), dict(ok=None), dict(taps=None)):
        assert call(**kw) == 1 and b"null" in lib.mp_last_error(), (kw, lib.mp_last_error())
    for kw, word in ((dict(root=None), b"both or neither"), (dict(root_out=None), b"both or neither"), (dict(quat_out=q), b"overlaps an input"),
                     (dict(root_out=r), b"overlaps an input"), (dict(taps=outs["ok"]), b"two outputs overlap"), (dict(R=-1), b"radius=-1"), (dict(R=65), b"radius=65"),
                     (dict(deg=3), b"degree=3"), (dict(deg=-1), b"degree=-1"), (dict(tp=2), b"taper=2"), (dict(j=1), b"J=1"), (dict(j=33), b"J=33"),
                     (dict(n=0), b"out of range"), (dict(i=0), b"out of range"), (dict(s=0), b"out of range"), (dict(s=13), b"out of range"), (dict(m=0), b"Mtot=0"),
                     (dict(m=2 ** 40, i=2 ** 10), b"out of range"), (dict(n=2 ** 40, i=2 ** 10), b"too many for one launch")):
        assert call(**kw) == 1 and word in lib.mp_last_error(), (kw, lib.mp_last_error())
    poses, pok = torch.full((N, inner, J, 3), -1.0, device="cuda"), torch.full((N, inner), 77, dtype=torch.uint8, device="cuda")
    L = torch.full((S, J - 1), 0.5, device="cuda")
    par = (C.c_int32 * J)(*rot.H36M_PARENTS)
    rest = (C.c_float * (3 * J))(*rot.H36M_REST.ravel().tolist())
    zero_row = rot.H36M_REST.copy()
    zero_row[4] = 0

    def fk(x=q, root=r, lengths=L, n=N, i=inner, j=J, o=off, s=S, parents=par, dirs=rest, flags=0, out=poses, k=pok):
        return lib.mp_lift_fk(p(x), p(root), p(lengths), n, i, j, p(o), s, parents, dirs, flags, p(out), p(k), None)
    for kw in (dict(x=None), dict(lengths=None), dict(dirs=None), dict(parents=None), dict(out=None), dict(k=None), dict(o=None)):
        assert fk(**kw) == 1 and b"null" in lib.mp_last_error(), (kw, lib.mp_last_error())
    for kw, word in ((dict(flags=2), b"flags=2"), (dict(j=1), b"J=1"), (dict(j=33), b"J=33"), (dict(n=0), b"out of range"), (dict(s=13), b"out of range"),
                     (dict(out=q), b"overlap"), (dict(dirs=(C.c_float * (3 * J))(*zero_row.ravel().tolist())), b"rest[4]"),
                     (dict(parents=(C.c_int32 * J)(*((0,) + rot.H36M_PARENTS[1:]))), b"joint 0 must be the root"), (dict(n=2 ** 40, i=2 ** 10), b"too many")):
        assert fk(**kw) == 1 and word in lib.mp_last_error(), (kw, lib.mp_last_error())
    torch.cuda.synchronize()
    assert all(bool((t == (77 if t.dtype == torch.uint8 else -1)).all()) for t in list(outs.values()) + [poses, pok])      # nothing was launched
    assert call() == 0 and call(root=None, root_out=None, R=64, tp=1) == 0 and fk() == 0 and fk(o=None, flags=1, lengths=torch.full((N, inner, J - 1), 0.5, device="cuda")) == 0
    torch.cuda.synchronize()
    assert bool((outs["ok"] == 1).all()) and bool(pok.all()) and bool((outs["quat_out"][..., 0] == 1).all())
    from manipose_amd import pose_from_rotations, retime_rotations, smooth_rotations
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        retime_rotations(q.cpu())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        retime_rotations(q, r.cpu())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pose_from_rotations(q.cpu(), np.full(16, 0.5, np.float32))
    with pytest.raises(ValueError, match="radius"):
        smooth_rotations(q, radius=0)
    with pytest.raises(ValueError, match="past the last frame"):
        retime_rotations(q, seq_offset=[0, 5, N], start=4.5)


# ---- end to end: run.lift in synthetic-data mode ------------------------------------------------------------------------------------------------
COMMON = ["run.train=false", "run.test=false", "run.lift=true", "lift.stride=14", "train.batch_size_test=4", "data.seq_len=27", "model.channels=64",
          "model.layers=2", "model.nheads=4", "model.channels_seg=32", "model.layers_seg=1", "model.nheads_seg=4", "multi_hyp.n_hyp=3",
          "data.synthetic_sequences=2", "model.precision=fp32", "lift.rigid=true", "lift.rotations=true"]
NEW = ("__rt", "__rt_quat", "__rt_ok", "__rt_taps", "__rt_time", "__rt_fps")


def test_run_lift_with_retime_end_to_end(tmp_path, monkeypatch):
    sys.path.insert(0, os.path.join(ROOT, "hpe"))
    from _entry import run
    from manipose_amd import retime_rotations
    monkeypatch.chdir(tmp_path)
    run(COMMON + ["run.experiment=absent"])
    run(COMMON + ["run.experiment=zero", "lift.retime_fps=0"])
    run(COMMON + ["run.experiment=rt", "lift.retime_fps=30", "lift.retime_radius=2"])
    a, b, z = (np.load(os.path.join(str(tmp_path), d, "lift.npz")) for d in ("absent", "zero", "rt"))
    keys = [f"synthetic_{i:03d}" for i in range(2)]
    assert not any("__rt" in k for k in a.files) and sorted(a.files) == sorted(b.files)
    assert all(a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes() for k in a.files)         # the key absent and the key at 0: the same bytes
    assert sorted(set(z.files) - set(a.files)) == sorted(k + s for k in keys for s in NEW) and set(a.files) <= set(z.files)
    assert all(a[k].dtype == z[k].dtype and a[k].shape == z[k].shape and a[k].tobytes() == z[k].tobytes() for k in a.files)      # every earlier key keeps its bytes
    for i, k in enumerate(keys):
        n = 27 * 4 + 37 * i + 11
        M = ((n - 1) * 30) // 50 + 1
        assert z[k + "__rt"].shape == (M, 17, 3) and z[k + "__rt"].dtype == np.float32 and z[k + "__rt_quat"].shape == (M, 17, 4)
        assert z[k + "__rt_ok"].shape == z[k + "__rt_taps"].shape == z[k + "__rt_time"].shape == (M,) and z[k + "__rt_time"].dtype == np.float64
        assert z[k + "__rt_fps"].tolist() == [50, 30] and z[k + "__rt_fps"].dtype == np.int32 and z[k + "__rt_ok"].dtype == np.uint8
        assert np.array_equal(z[k + "__rt_time"], (np.arange(M, dtype=np.float64) * 50.0) / 30.0) and z[k + "__rt_time"][-1] <= n - 1
        want = retime_rotations(_dev(z[k + "__quat"]), None, _dev(z[k + "__quat_ok"]), None, 50, 30, 0.0, 2, 2, "uniform")
        assert _same(z[k + "__rt_quat"], _np(want.quat)) and _same(z[k + "__rt_ok"], _np(want.ok)) and _same(z[k + "__rt_taps"], _np(want.taps))
        back, ok = ref.fk(z[k + "__rt_quat"][:, None], z[k + "__bones"][None], rot.H36M_PARENTS, rot.H36M_REST, None, [0, M])
        bound = max(4 * float(np.abs(back.astype(np.float32).astype(np.float64) - back).max()), FLOOR)
        assert float(np.abs(z[k + "__rt"].astype(np.float64) - back[:, 0]).max()) <= bound and ok.all()      # fk(__rt_quat, __bones) is __rt
    # the input's own rate with a radius: smoothing in rotation space, the one case lift.score scores (ground truth exists at input frames only)
    run(COMMON + ["run.experiment=sm", "lift.score=true", "lift.retime_fps=50", "lift.retime_radius=3"])
    run(COMMON + ["run.experiment=other", "lift.score=true", "lift.retime_fps=25"])
    rows = open(os.path.join(str(tmp_path), "sm", "lift_score_rt.csv")).read().splitlines()
    assert [r.split(",")[0] for r in rows[1:]] == keys + ["average"] and [int(float(r.split(",")[1])) for r in rows[1:3]] == [27 * 4 + 11, 27 * 4 + 48]
    assert os.path.exists(os.path.join(str(tmp_path), "other", "lift_score.csv")) and not os.path.exists(os.path.join(str(tmp_path), "other", "lift_score_rt.csv"))
    sm = np.load(os.path.join(str(tmp_path), "sm", "lift.npz"))
    assert all(sm[k + "__rt"].shape == sm[k].shape and np.array_equal(sm[k + "__rt_time"], np.arange(len(sm[k]), dtype=np.float64)) for k in keys)

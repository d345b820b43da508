"""Joint rotations of lifted poses on the device: mp_lift_rotations against the float64 statement of its rule (lift_rot_ref.py), the round trip of
its output through fp64 forward kinematics, the closure through the project's own decoder (mp_fk_decode_fwd), its invariants, its argument checks,
and lift_sequences / run.lift with rotations.

The bound wherever a stored float32 is compared with the statement: 2^-23 per component (lift_rot_ref.TOL).  Both sides round the same real number,
a component of a unit quaternion or of a rotation matrix, known to about 1e-13 given the margins test_lift_rot_host.py asserts (every decision at
least 1e-3 from its threshold), to float32: they differ by at most one unit in the last place of 1.0.  ok bytes and continuity signs are compared
for equality, the constructed degenerate cases bit for bit.  No bound here is measured from the kernel."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

import lift_rot_ref as ref
from helpers import load_fixture
from lift_fixtures import fixture_model as _model, same as _same, sequences as _sequences

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAR, REST = ref.H36M_PARENTS, ref.H36M_REST
FLOOR = 1e-7                    # metres: the floor of the round-trip bound


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()                # (a copy: the cached scenes are read-only)


@functools.lru_cache(maxsize=None)
def _scene(kind, inner, ch):
    """a scene and the statement on it, computed once and left unchanged: (poses, off, parents, rest, (quat, rot6d, ok, flips, margins))"""
    P, off, par, rest = ref.random_scene(kind, inner, ch)
    want = ref.rotations(P, par, rest, off)
    for a in (P,) + want[:4]:
        a.setflags(write=False)
    return P, off, par, rest, want


def _run(poses, off=None, sk=None, continuous=True):
    from manipose_amd import pose_rotations
    res = pose_rotations(_dev(poses), off, sk, continuous, return_rot6d=True)
    torch.cuda.synchronize()
    return [r.cpu().numpy() for r in res]


def _worst(got, want):
    return float(np.abs(got.astype(np.float64) - want).max())


def _round_trip(quat, poses, par, rest, lengths=None):
    """max |fk(quat, lengths) - pose| in fp64 (measured lengths by default), root at the pose's own"""
    p = poses[..., :3].astype(np.float64)
    L = ref.measured_lengths(p, par) if lengths is None else lengths
    return float(np.abs(ref.fk_quat(quat.astype(np.float64), L, par, rest, p[..., 0, :]) - p).max())


@pytest.mark.parametrize("kind,inner,ch", ref.SCENES)
def test_kernel_against_the_fp64_statement_and_round_trip(lib, kind, inner, ch):
    """Measured on an MI355X when written: the quaternions have the statement's bits on all eight scenes, rot6d differs by at most 0.25 x 2^-23 (the
    compiler contracts multiply-adds).  Round trip (kernel = the statement's float32 output, metres): H36M 1.8e-7 (inner = 1) and 2.5e-7 (inner = 5),
    J = 2 5.4e-8 and 5.5e-8, the 32-joint chain 8.2e-7 and 9.2e-7: the float32 rounding of the quaternions along the chain, nothing else."""
    P, off, par, rest, (quat, rot6d, ok, flips, m) = _scene(kind, inner, ch)
    sk = None if kind == "h36m" else ref.Sk(par, rest)
    given = P[:, 0] if (inner, ch) == (1, 3) else P                       # the (Ntot, J, 3) form of the public function
    lead = given.shape[:-2]
    t = _dev(given)
    from manipose_amd import pose_rotations
    got = [r.cpu().numpy() for r in pose_rotations(t, off, sk, True, return_rot6d=True)]
    assert _same(t.cpu().numpy(), given)                                  # out of place: the poses (the score channel included) are unchanged
    J = len(par)
    assert got[0].shape == lead + (J, 4) and got[0].dtype == np.float32 and got[1].shape == lead and got[1].dtype == np.uint8
    assert got[2].shape == lead + (J, 6) and got[2].dtype == np.float32
    q, k, r6 = got[0].reshape(quat.shape), got[1].reshape(ok.shape), got[2].reshape(rot6d.shape)
    eq, e6 = _worst(q, quat), _worst(r6, rot6d)
    print(f"\n[{kind} inner={inner} C={ch}] |quat - statement| <= {eq / ref.TOL:.3f}, |rot6d - statement| <= {e6 / ref.TOL:.3f} (x 2^-23, bound 1); "
          f"{int(flips.sum())} of {flips.size} quaternions flipped by the continuity pass")
    assert np.array_equal(k, ok) and ok.all()
    assert eq <= ref.TOL and e6 <= ref.TOL
    plain = _run(given, off, sk, continuous=False)                        # the canonical signs: the continuous result is +- these, bit for bit
    canon = plain[0].reshape(quat.shape)
    assert np.array_equal(q != canon, np.broadcast_to(flips[..., None], q.shape) & (canon != 0)) and _same(np.abs(q), np.abs(canon))
    assert _same(np.where(flips[..., None], -canon, canon), q) and _same(plain[1], got[1]) and _same(plain[2], got[2])
    dev_off = _run(given, torch.from_numpy(off).cuda(), sk)               # a device offset table; and: two calls, identical bits
    assert all(_same(a, b) for a, b in zip(dev_off, got))
    two = pose_rotations(t, off, sk)                                      # without return_rot6d: the same two tensors
    assert len(two) == 2 and _same(two[0].cpu().numpy(), got[0]) and _same(two[1].cpu().numpy(), got[1])
    mine, stated = _round_trip(q, P, par, rest), _round_trip(quat, P, par, rest)
    bound = max(4 * stated, FLOOR)
    print(f"[{kind} inner={inner} C={ch}] round trip fk(quat, measured lengths): kernel {mine:.3e} m, the statement's float32 output {stated:.3e} m, "
          f"bound {bound:.3e} m")
    assert mine <= bound


def test_constructed_cases_are_bit_equal(lib):
    poses, quat, rot6d, ok = ref.exact_scene()
    got = _run(poses, continuous=False)
    assert _same(got[0], quat.astype(np.float32)) and _same(got[2], rot6d.astype(np.float32)) and np.array_equal(got[1], ok)
    assert got[1][:, 0].tolist() == [1, 0, 0, 0, 0]
    assert _same(got[0][ref.HALF_TURN, 0, 2], np.array([0, 1, 0, 0], np.float32))                 # the half turn about the fixed axis
    assert not np.signbit(got[0]).any() or (got[0][np.signbit(got[0])] != 0).all()                 # no negative zero
    cont = _run(poses)                                                    # five unrelated frames as one sequence: signs move, nothing else
    assert _same(np.abs(cont[0]), np.abs(got[0])) and _same(cont[1], got[1]) and _same(cont[2], got[2])
    alt, off = ref.alternating_scene()
    want = ref.rotations(alt, PAR, REST, off)
    a = _run(alt, off)
    canon = _run(alt, off, continuous=False)[0]
    flipped = (a[0] != canon).any(-1)
    assert np.array_equal(flipped[:, 0, 0], np.arange(70) % 2 == 1) and not flipped[:, 0, 1:].any()      # every odd frame, across the 64-frame chunk
    assert _worst(a[0], want[0]) <= ref.TOL and a[1].all()
    d = (a[0][1:, 0, 0].astype(np.float64) * a[0][:-1, 0, 0]).sum(-1)
    assert (d > 0.98).all()                                               # 20 degrees apart, one hemisphere


def test_closure_through_the_decoder(lib):
    """rot6d and per-pose measured lengths fed to mp_fk_decode_fwd give the fixture's poses back, within the tolerance test_gpu_parity.py uses for
    this fixture, with no pose excluded (the two poses with a bone of length 0 included)."""
    from manipose_amd import _lib
    fx = load_fixture("decoder")["poses"]
    assert fx.shape == (21, 17, 3) and fx.dtype == np.float32 and not fx[:, 0].any()
    quat, ok, rot6d = _run(fx, continuous=False)
    lengths = _dev(ref.measured_lengths(fx, PAR).astype(np.float32))
    r6 = _dev(rot6d)
    out = torch.empty(21, 1, 1, 17, 3, device="cuda")
    _lib.check(lib.mp_fk_decode_fwd(r6.data_ptr(), 6, 6, lengths.data_ptr(), out.data_ptr(), 21, 1, 1, torch.cuda.current_stream().cuda_stream))
    got = out.view(21, 17, 3).cpu().numpy()
    print(f"\n[decoder closure] max |fk_decode(rot6d, lengths) - pose| = {np.abs(got - fx).max():.3e} m; ok = 0 on poses {np.nonzero(ok == 0)[0].tolist()}")
    np.testing.assert_allclose(got, fx, rtol=1e-5, atol=2e-6)
    assert np.nonzero(ok == 0)[0].tolist() == [0, 1]


def test_invariants(lib):
    P, off, par, rest, (quat, rot6d, ok, flips, m) = _scene("h36m", 5, 4)
    together = _run(P, off)
    assert all(_same(a, b) for a, b in zip(_run(P, off), together))       # two calls: identical bits
    for s in range(len(off) - 1):                                         # a sequence alone equals the same sequence inside the four-sequence call
        sl = slice(int(off[s]), int(off[s + 1]))
        assert all(_same(a, b[sl]) for a, b in zip(_run(P[sl]), together)), s
    poisoned = P.copy()
    poisoned[..., 3] = np.nan                                             # channel 3 is not read
    assert all(_same(a, b) for a, b in zip(_run(poisoned, off), together))
    one = _run(P)                                                         # (the sequences matter: as ONE sequence the signs differ, nothing else does)
    assert not _same(one[0], together[0]) and _same(np.abs(one[0]), np.abs(together[0])) and _same(one[2], together[2])
    # a device offset table no host check has seen: every sequence's frames are clamped to 0 .. Ntot-1, and a frame no sequence holds keeps its
    # canonical sign
    wild = np.array([-5, 3, 150, 10 ** 12], np.int64)
    got = _run(P, torch.from_numpy(wild).cuda())
    canon = _run(P, continuous=False)[0]
    want = ref.continuity(canon, wild)[0]
    assert _same(got[0], want) and _same(got[1], together[1]) and _same(got[2], together[2])
    gap = np.array([0, 3, 3, 150], np.int64)                              # an empty sequence, and frames 150 .. 199 in no sequence
    got = _run(P, torch.from_numpy(gap).cuda())
    assert _same(got[0], ref.continuity(canon, gap)[0]) and _same(got[0][150:], canon[150:])
    bad = P.copy()
    bad[7, 2, 11, 1] = np.inf                                             # a non-finite coordinate: that pose alone is identities with ok = 0
    got = _run(bad, off, continuous=False)
    assert got[1][7, 2] == 0 and got[1].sum() == got[1].size - 1 and _same(got[0][7, 2], np.tile(np.array([1, 0, 0, 0], np.float32), (17, 1)))
    keep = np.ones(bad.shape[:2], bool)
    keep[7, 2] = False
    assert _same(got[0][keep], canon[keep])


def test_entry_point_rejects_bad_arguments_before_any_launch(lib):
    import ctypes as C
    t = torch.zeros(4, 2, 17, 3, device="cuda")
    off = torch.tensor([0, 4], dtype=torch.int64, device="cuda")
    quat, r6 = torch.full((4, 2, 17, 4), -1.0, device="cuda"), torch.full((4, 2, 17, 6), -1.0, device="cuda")
    ok = torch.full((4, 2), 7, dtype=torch.uint8, device="cuda")
    par = (C.c_int32 * 17)(*PAR)
    rest = (C.c_float * 51)(*REST.ravel().tolist())
    p = lambda x: None if x is None else x.data_ptr()

    def call(poses=t, offs=off, parents=par, dirs=rest, q=quat, r=r6, o=ok, Ntot=4, inner=2, J=17, ch=3, S=1, flags=1):
        return lib.mp_lift_rotations(p(poses), Ntot, inner, J, ch, p(offs), S, parents, dirs, flags, p(q), p(r), p(o), None)
    for kw in (dict(poses=None), dict(offs=None), dict(parents=None), dict(dirs=None), dict(q=None), dict(o=None)):
        assert call(**kw) == 1 and b"null" in lib.mp_last_error()
    late_root = (C.c_int32 * 17)(*((0,) + PAR[1:]))
    forward = (C.c_int32 * 17)(*(PAR[:5] + (6,) + PAR[6:]))
    zero_row, nan_row = REST.copy(), REST.copy()
    zero_row[4] = 0
    nan_row[9, 2] = np.nan
    as_c = lambda a: (C.c_float * 51)(*a.ravel().tolist())
    for kw, word in ((dict(ch=2), b"C=2"), (dict(ch=5), b"C=5"), (dict(J=1), b"J=1"), (dict(J=33), b"J=33"), (dict(S=0), b"out of range"),
                     (dict(S=5), b"out of range"), (dict(Ntot=0), b"out of range"), (dict(inner=0), b"out of range"),
                     (dict(Ntot=2 ** 40, inner=2 ** 10), b"too many for one launch"), (dict(flags=2), b"flags=2"), (dict(flags=-1), b"flags=-1"),
                     (dict(parents=late_root), b"joint 0 must be the root"), (dict(parents=forward), b"parents precede"),
                     (dict(dirs=as_c(zero_row)), b"rest[4]"), (dict(dirs=as_c(nan_row)), b"rest[9]")):
        assert call(**kw) == 1 and word in lib.mp_last_error(), (kw, lib.mp_last_error())
    torch.cuda.synchronize()
    assert bool((quat == -1).all()) and bool((r6 == -1).all()) and bool((ok == 7).all())      # nothing was launched
    assert call() == 0 and call(r=None) == 0 and call(flags=0) == 0                            # good arguments; rot6d may be null
    torch.cuda.synchronize()
    assert not bool(ok.any()) and bool((quat[..., 0] == 1).all()) and bool((quat[..., 1:] == 0).all())      # every joint on one spot: identities, ok = 0
    assert torch.count_nonzero(t).item() == 0


# ---- end to end: the tiny fp32 fixture model of lift_fixtures.py -----------------------------------------------------------------------------
def _tiny_model(kind):
    """(model, T, K): "fixture" - the tiny fp32 RMCL fixture model the other lift GPU tests use (T = 27); "t9" - a seeded T = 9 model of the same
    architecture, so that sequences of 12 and 20 frames hold more than one window"""
    if kind == "fixture":
        return _model("rmcl")
    from manipose_amd import RMCLManifoldMixSTE, h36m_skeleton
    torch.manual_seed(5)
    model = RMCLManifoldMixSTE(h36m_skeleton(), num_frame=9, embed_dim_rot=32, depth_rot=1, num_heads_rot=4, embed_dim_seg=16, depth_seg=1, num_heads_seg=4,
                               n_hyp=2, drop_path_rate=0.0)
    model.precision = "fp32"
    return model.cuda().eval(), 9, 2


@pytest.mark.parametrize("kind", ["t9", "fixture"])
def test_lift_sequences_end_to_end(lib, kind):
    """Two sequences of 12 and 20 frames.  The stage is mp_lift_rotations on the poses as emitted: its output has the bits of pose_rotations on them,
    and fk(quat, bones) gives them back within the bound of the round-trip test (the statement's own float32 output on these poses, x 4)."""
    from manipose_amd import lift_sequences, pose_rotations
    model, T, K = _tiny_model(kind)
    p2 = _sequences((12, 20), 31)[0]
    kw = dict(stride=T // 2 + 1, tta=True, batch=2, return_hyps=True, rigid=True, return_bones=True)
    base = lift_sequences(model, p2, **kw)
    off_ = lift_sequences(model, p2, rotations=False, **kw)
    assert len(base) == len(off_) == 3
    assert all(torch.equal(x, y) for a, b in zip(base, off_) for x, y in zip(a, b))             # the default: not a bit changes, nothing is appended
    res = lift_sequences(model, p2, rotations=True, return_rotations=True, **kw)
    assert len(res) == 4 and all(torch.equal(x, y) for a, b in zip(res[:3], base) for x, y in zip(a, b))      # the poses are not modified
    assert len(lift_sequences(model, p2, rotations=True, **kw)) == 3                                          # computed, not asked for
    print()
    for s, d in enumerate(res[3]):
        assert sorted(d) == ["hyps_ok", "hyps_quat", "ok", "quat"]
        n = p2[s].shape[0]
        poses, hyps, bones = res[0][s].cpu().numpy(), res[1][s].cpu().numpy(), res[2][s].cpu().numpy().astype(np.float64)
        got = {k: v.cpu().numpy() for k, v in d.items()}
        assert got["quat"].shape == (n, 17, 4) and got["ok"].shape == (n,) and got["hyps_quat"].shape == (n, K, 17, 4) and got["hyps_ok"].shape == (n, K)
        assert got["ok"].all() and got["hyps_ok"].all()
        for tag, t, p, q, k in (("poses", res[0][s], poses, got["quat"], got["ok"]), ("hypotheses", res[1][s], hyps, got["hyps_quat"], got["hyps_ok"])):
            alone = pose_rotations(t.contiguous())
            assert _same(alone[0].cpu().numpy(), q) and _same(alone[1].cpu().numpy(), k)
            want = ref.rotations(p if p.ndim == 4 else p[:, None], PAR, REST)
            m = want[4]
            print(f"[lift_sequences {kind}, sequence {s} {tag}] margins of the statement's decisions on the emitted poses: arc {m['arc']:.2e}, frame "
                  f"{m['frame']:.2e}, lead {m['lead']:.2e}, dot {m['dot']:.2e}; |quat - statement| = {_worst(q.reshape(want[0].shape), want[0]) / ref.TOL:.3f} x 2^-23")
            mine, stated = _round_trip(q, p, PAR, REST, bones), _round_trip(want[0].reshape(q.shape), p, PAR, REST, bones)
            bound = max(4 * stated, FLOOR)
            print(f"[lift_sequences {kind}, sequence {s} {tag}] fk(quat, bones) against the emitted poses: kernel {mine:.3e} m, the statement's float32 "
                  f"output {stated:.3e} m, bound {bound:.3e} m")
            assert mine <= bound
    loose = lift_sequences(model, p2, rotations=True, rotations_continuous=False, return_rotations=True, **kw)[3]
    assert all(_same(np.abs(a["quat"].cpu().numpy()), np.abs(b["quat"].cpu().numpy())) for a, b in zip(loose, res[3]))
    assert all(bool((a["quat"][:, :, 0] >= 0).all()) for a in loose)                              # canonical: w >= 0 on every arc, and on these roots


def test_rotations_lift_entry_point(lib, tmp_path, monkeypatch):
    sys.path.insert(0, os.path.join(ROOT, "hpe"))
    from _entry import run
    monkeypatch.chdir(tmp_path)
    common = ["run.train=false", "run.test=false", "run.lift=true", "lift.stride=14", "train.batch_size_test=4", "data.seq_len=27", "model.channels=64",
              "model.layers=2", "model.nheads=4", "model.channels_seg=32", "model.layers_seg=1", "model.nheads_seg=4", "multi_hyp.n_hyp=3",
              "data.synthetic_sequences=2", "model.precision=fp32", "lift.hyps=true", "lift.rigid=true"]
    keys = [f"synthetic_{i:03d}" for i in range(2)]
    before = ["", "__hyps", "__bones"]
    run(common)                                                           # the key at its default: exactly today's keys
    z0 = np.load(os.path.join(str(tmp_path), "default", "lift.npz"))
    assert sorted(z0.files) == sorted(k + s for k in keys for s in before)
    z0 = {k: z0[k] for k in z0.files}
    run(common + ["lift.rotations=true"])
    z = np.load(os.path.join(str(tmp_path), "default", "lift.npz"))
    assert sorted(z.files) == sorted(k + s for k in keys for s in before + ["__quat", "__quat_ok", "__hyps_quat", "__hyps_quat_ok"])
    for i, k in enumerate(keys):
        n = 27 * 4 + 37 * i + 11
        assert z[k + "__quat"].shape == (n, 17, 4) and z[k + "__quat"].dtype == np.float32 and z[k + "__quat_ok"].shape == (n,)
        assert z[k + "__hyps_quat"].shape == (n, 3, 17, 4) and z[k + "__hyps_quat_ok"].shape == (n, 3) and z[k + "__quat_ok"].dtype == np.uint8
        assert all(_same(z[k + s], z0[k + s]) for s in before)
        back = ref.fk_quat(z[k + "__quat"], z[k + "__bones"].astype(np.float64), PAR, REST, z[k][:, 0].astype(np.float64))
        assert np.abs(back - z[k]).max() <= 1e-5 and z[k + "__quat_ok"].all()       # (root, quat, bones) is the sequence

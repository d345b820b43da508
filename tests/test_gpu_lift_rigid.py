"""Rigid lifting on the device: mp_lift_rigid and mp_bone_length_means against float64 (lift_rigid_ref.py), the degenerate-bone rule,
determinism, lift_sequences(rigid=True) for the three architectures against the numpy projection of its own non-rigid output, the three
sources of the bone-length table, and the run.lift entry point."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

import lift_rigid_ref as ref
from lift_fixtures import bits as _bits, fixture_model as _model, sequences_2d as _sequences, to_numpy as _np
from lift_ref import MIRROR, closed_form_tables, cut_windows

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# Bounds, derived and not measured.  A projected joint is the root plus at most 5 bones (the H36M chain depth); each bone costs a handful of
# fp32 roundings (difference, dot product, sqrtf, division, multiply-add) on quantities of about 1 m, ulp 1.2e-7: 5e-6 m for a position, 1e-6 m
# for the length of one bone.  A wrong parent, direction or table row shows at 1e-2 m or more.
POS_TOL, LEN_TOL = 5e-6, 1e-6
LENS = [1, 2, 30, 257]                                                    # a one-frame sequence, one that crosses a 256-lane block
OFF = np.concatenate([[0], np.cumsum(LENS)]).astype(np.int64)
PARENTS_C = (C.c_int32 * 17)(*ref.PARENTS)
BONE_MIRROR = MIRROR[1:] - 1                                              # bone of joint j is read from bone of joint MIRROR[j]


def _random_poses(inner, ch, seed):
    g = np.random.default_rng(seed)
    p = g.standard_normal((int(OFF[-1]), inner, 17, ch)).astype(np.float32)
    short = ref.bone_lengths(p) <= 1e-3
    assert not short.any()                                                # every bone vector longer than 1e-3 m
    L = g.uniform(0.05, 0.6, (len(LENS), 16)).astype(np.float32)
    return p, L


@pytest.mark.parametrize("inner,ch", [(1, 3), (3, 4)])
def test_lift_rigid_kernel_against_fp64(lib, inner, ch):
    from manipose_amd import project_rigid
    p, L = _random_poses(inner, ch, seed=10 * inner + ch)
    want = ref.project_all(p, L, OFF)
    runs = []
    for _ in range(2):
        t = torch.from_numpy(p).cuda()
        t = t[:, 0].contiguous() if (inner, ch) == (1, 3) else t          # the (Ntot, J, 3) form of the public function
        r = project_rigid(t, torch.from_numpy(L).cuda(), OFF)
        assert r is t                                                     # in place
        torch.cuda.synchronize()
        runs.append(r.cpu().numpy().reshape(p.shape))
    got = runs[0]
    err = np.abs(got.astype(np.float64) - want)
    print(f"\n[lift_rigid inner={inner} C={ch}] max |err| = {err.max():.3e} m (bound {POS_TOL:.0e})")
    assert err.max() <= POS_TOL
    bl = ref.bone_lengths(got)                                            # (Ntot, inner, 16) in float64
    rows = np.repeat(L.astype(np.float64), LENS, axis=0)[:, None, :]
    lerr = np.abs(bl - rows).max()
    print(f"[lift_rigid inner={inner} C={ch}] max |bone length - table| = {lerr:.3e} m (bound {LEN_TOL:.0e})")
    assert lerr <= LEN_TOL
    assert np.array_equal(_bits(got[:, :, 0, :3]), _bits(p[:, :, 0, :3]))         # the root, bit for bit
    if ch == 4:
        assert np.array_equal(_bits(got[..., 3]), _bits(p[..., 3]))               # the score channel, bit for bit
    assert np.array_equal(_bits(runs[0]), _bits(runs[1]))                         # two calls: identical bits


def test_lift_rigid_degenerate_bones_follow_the_fallback_rule(lib):
    from manipose_amd import project_rigid
    g = np.random.default_rng(5)
    p = g.standard_normal((5, 17, 3)).astype(np.float32)
    p[1, 7] = p[1, 0]                                  # a bone off the root: up the z axis
    p[2, 5] = p[2, 4]                                  # a bone deeper in a chain: continues 0 -> 4
    p[3, 2] = p[3, 1] = p[3, 0]                        # two in a row from the root: both up the z axis
    p[4, 16] = p[4, 15] = p[4, 14]                     # two in a row at the end of a chain: both continue 8 -> 14
    L = g.uniform(0.05, 0.6, (16,)).astype(np.float32)
    want = ref.project_all(p, L[None], [0, 5])
    got = project_rigid(torch.from_numpy(p).cuda(), L).cpu().numpy()
    assert np.isfinite(got).all()
    assert np.abs(got - want).max() <= POS_TOL
    assert np.abs(ref.bone_lengths(got) - L.astype(np.float64)).max() <= LEN_TOL
    z = np.array([0.0, 0.0, 1.0])
    np.testing.assert_allclose(got[1, 7] - got[1, 0], L[6] * z, rtol=0, atol=LEN_TOL)
    np.testing.assert_allclose(got[3, 1] - got[3, 0], L[0] * z, rtol=0, atol=LEN_TOL)
    np.testing.assert_allclose(got[3, 2] - got[3, 1], L[1] * z, rtol=0, atol=LEN_TOL)
    u4 = (p[2, 4] - p[2, 0]).astype(np.float64)
    np.testing.assert_allclose(got[2, 5] - got[2, 4], L[4] * u4 / np.linalg.norm(u4), rtol=0, atol=2 * LEN_TOL)
    u14 = (p[4, 14] - p[4, 8]).astype(np.float64)
    for j in (15, 16):
        np.testing.assert_allclose(got[4, j] - got[4, j - 1], L[j - 1] * u14 / np.linalg.norm(u14), rtol=0, atol=2 * LEN_TOL)


def test_bone_length_means_against_fp64(lib):
    """fp64 differences, square roots and sums on the device, one rounding to fp32 at the end (2^-24 = 6e-8 relative): within 1e-6 relative."""
    from manipose_amd.lifting import bone_length_means
    p, _ = _random_poses(1, 3, seed=77)
    p = p[:, 0]
    t = torch.from_numpy(p).cuda()
    a = bone_length_means(t, OFF).cpu().numpy()
    b = bone_length_means(t, torch.from_numpy(OFF).cuda()).cpu().numpy()
    want = ref.mean_bone_lengths(p, OFF)
    rel = np.abs(a - want) / want
    print(f"\n[bone_length_means] max relative error = {rel.max():.3e} (bound 1e-6)")
    assert a.shape == (4, 16) and rel.max() <= 1e-6
    assert np.array_equal(_bits(a), _bits(b))                             # two calls: identical bits
    real = np.array([1, 1, 17, 200], np.int64)                            # the frames behind them are padding: they do not contribute
    c = bone_length_means(t, OFF, real_frames=real).cpu().numpy()
    want_c = ref.mean_bone_lengths(p, OFF, real)
    assert (np.abs(c - want_c) / want_c).max() <= 1e-6
    poisoned = p.copy()
    for s in range(4):
        poisoned[OFF[s] + real[s]:OFF[s + 1]] = np.nan
    d = bone_length_means(torch.from_numpy(poisoned).cuda(), OFF, real_frames=real).cpu().numpy()
    assert np.array_equal(_bits(c), _bits(d))
    one = bone_length_means(t[:30].contiguous()).cpu().numpy()            # default: all frames are one sequence
    assert (np.abs(one - ref.mean_bone_lengths(p[:30], [0, 30])) / one).max() <= 1e-6


def test_rigid_entry_points_reject_bad_arguments_before_any_launch(lib):
    t = torch.zeros(4, 17, 3, device="cuda")
    off = torch.tensor([0, 4], dtype=torch.int64, device="cuda")
    L = torch.full((1, 16), 0.3, device="cuda")
    M = torch.full((1, 16), -1.0, device="cuda")

    def rigid(poses=t.data_ptr(), J=17, ch=3, inner=1, S=1, parents=PARENTS_C):
        return lib.mp_lift_rigid(poses, 4, inner, J, ch, off.data_ptr(), S, L.data_ptr(), parents, None)

    def means(poses=t.data_ptr(), J=17, S=1, parents=PARENTS_C):
        return lib.mp_bone_length_means(poses, 4, J, off.data_ptr(), None, S, parents, M.data_ptr(), None)
    child_first = list(ref.PARENTS)
    child_first[3] = 5
    two_roots = list(ref.PARENTS)
    two_roots[4] = -1
    bad_tables = ((C.c_int32 * 17)(*child_first), b"parents precede"), ((C.c_int32 * 17)(*two_roots), b"parents precede"), \
        ((C.c_int32 * 17)(*([0] + list(ref.PARENTS[1:]))), b"root"), (None, b"null parent")
    for fn in (rigid, means):
        for table, word in bad_tables:
            assert fn(parents=table) == 1 and word in lib.mp_last_error(), lib.mp_last_error()
        assert fn(poses=None) == 1 and b"null" in lib.mp_last_error()
        assert fn(S=0) == 1
        assert fn(J=33, parents=(C.c_int32 * 33)(*([-1] + list(range(32))))) == 1 and b"J=33" in lib.mp_last_error()
    assert rigid(ch=5) == 1 and b"C=5" in lib.mp_last_error()
    assert rigid(inner=0) == 1
    torch.cuda.synchronize()
    assert torch.count_nonzero(t).item() == 0 and bool((M == -1).all())   # nothing was launched
    assert means() == 0 and rigid() == 0                                  # the same calls with good arguments
    torch.cuda.synchronize()
    assert bool((M == 0).all())                                           # all joints at the origin: bones of length 0 ...
    want = ref.project_all(np.zeros((4, 17, 3)), np.full((1, 16), np.float32(0.3), np.float64), [0, 4])
    assert np.abs(t.cpu().numpy() - want).max() <= POS_TOL                # ... which all point up the z axis


# ---- end to end: the tiny fp32 fixture models of lift_fixtures.py ------------------------------------------------------------------------------
def _check_projection(got, base, bones, tol=POS_TOL, scale=1.0):
    """every sequence of `got` is the float64 projection of the same sequence of `base` with its row of `bones` (metres) times scale"""
    for g, b, L in zip(got, base, bones):
        want = ref.project_all(b, (np.float64(np.float32(scale)) * L.astype(np.float64))[None], [0, len(b)])
        assert g.shape == b.shape and np.abs(g.astype(np.float64)[..., :3] - want[..., :3]).max() <= tol


@pytest.mark.parametrize("kind", ["rmcl", "manifold", "mixste"])
def test_measured_lengths_end_to_end(lib, kind):
    """The rigid result is the projection of the NON-rigid result of the same call (which test_gpu_lift.py pins to the oracle, and which is
    bit-reproducible) with the float64 mean bone lengths of that result."""
    from manipose_amd import lift_sequences
    model, T, K = _model(kind)
    p2 = _sequences(T)
    for stride in (T, T // 2 + 1):
        kw = dict(stride=stride, tta=True, batch=2)
        base = _np(lift_sequences(model, p2, **kw))
        got, bones = lift_sequences(model, p2, rigid=True, lengths="measured", return_bones=True, **kw)
        got, bones = _np(got), _np(bones)
        for b, L in zip(base, bones):
            want_L = ref.mean_bone_lengths(b, [0, len(b)])[0]
            assert L.shape == (16,) and L.dtype == np.float32 and (np.abs(L - want_L) / want_L).max() <= 1e-6
        _check_projection(got, base, bones)
        for g, L in zip(got, bones):
            assert np.abs(ref.bone_lengths(g) - L.astype(np.float64)).max() <= LEN_TOL
        if kind == "mixste":                                              # its default source
            dflt, dbones = lift_sequences(model, p2, rigid=True, return_bones=True, **kw)
            assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(_np(dflt), got))
            assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(_np(dbones), bones))
    # the padded frames of the last window are projected too and do not count in the mean
    base = _np(lift_sequences(model, p2, tta=True, batch=2, keep_padding=True))
    got, bones = lift_sequences(model, p2, tta=True, batch=2, keep_padding=True, rigid=True, lengths="measured", return_bones=True)
    got, bones = _np(got), _np(bones)
    assert [len(g) for g in got] == [T, 2 * T, 3 * T]
    for b, L, q in zip(base, bones, p2):
        want_L = ref.mean_bone_lengths(b, [0, len(b)], real=[len(q)])[0]
        assert (np.abs(L - want_L) / want_L).max() <= 1e-6
    _check_projection(got, base, bones)


def _model_lengths(model, p2, T, stride, batch):
    """float64 mean over every sequence's windows of (|plain| + |mirrored, left and right swapped back|) / 2, from forwards of the same windows in
    the batches lift_sequences runs (a sequence's windows in forwards of `batch`, the mirrored copies behind the plain ones)."""
    win_seq, win_start = closed_form_tables([len(a) for a in p2], T, stride)
    X = cut_windows(p2, win_seq, win_start, T).astype(np.float32)
    Xf = X[..., MIRROR, :].copy()
    Xf[..., 0] *= -1
    rows = []
    for s in range(len(p2)):
        ws = np.flatnonzero(win_seq == s)
        per_window = []
        for a in range(0, len(ws), batch):
            w = ws[a:a + batch]
            with torch.no_grad():
                model(torch.from_numpy(np.concatenate([X[w], Xf[w]])).cuda())
            lw = np.abs(model._engine.peek(1).view(2 * len(w), 16).cpu().numpy().astype(np.float64))
            per_window.append((lw[:len(w)] + lw[len(w):][:, BONE_MIRROR]) / 2)
        rows.append(np.concatenate(per_window).mean(axis=0))
    return rows


@pytest.mark.parametrize("kind", ["rmcl", "manifold"])
def test_model_lengths_end_to_end(lib, kind):
    from manipose_amd import lift_sequences
    model, T, K = _model(kind)
    p2 = _sequences(T)
    for stride in (T, T // 2 + 1):
        kw = dict(stride=stride, tta=True, batch=2)
        base = _np(lift_sequences(model, p2, **kw))
        got, bones = lift_sequences(model, p2, rigid=True, return_bones=True, **kw)                # "model" is the default of both
        again, bones2 = lift_sequences(model, p2, rigid=True, lengths="model", return_bones=True, **kw)
        assert all(torch.equal(a, b) for a, b in zip(got, again)) and all(torch.equal(a, b) for a, b in zip(bones, bones2))
        got, bones = _np(got), _np(bones)
        want_bones = _model_lengths(model, p2, T, stride, batch=2)
        for L, w in zip(bones, want_bones):                               # fp32: one rounding per window added and two more, at most 6 windows
            assert (np.abs(L - w) / w).max() <= 1e-6
        _check_projection(got, base, bones)
        for g, b in zip(got, base):
            std = ref.bone_lengths(g).std(axis=0)
            assert std.max() <= LEN_TOL
            # the defect this mode removes is present in these inputs: the non-rigid bones change length over time
            assert ref.bone_lengths(b).std(axis=0).max() > 1e-4


def test_hypotheses_symmetry_caller_table_scale_and_the_default(lib):
    from manipose_amd import lift_sequences
    model, T, K = _model("rmcl")
    p2 = _sequences(T)
    kw = dict(stride=T // 2 + 1, tta=True, batch=2)
    plain = lift_sequences(model, p2, **kw)
    off, off_h = lift_sequences(model, p2, rigid=False, return_hyps=True, **kw)
    assert all(torch.equal(a, b) for a, b in zip(plain, off))                                      # rigid=False: nothing changes by a bit
    again, again_h = lift_sequences(model, p2, return_hyps=True, **kw)
    assert all(torch.equal(a, b) for a, b in zip(off, again)) and all(torch.equal(a, b) for a, b in zip(off_h, again_h))
    # every hypothesis of every frame gets the sequence's lengths; the scores are untouched
    got, hyps, bones = lift_sequences(model, p2, rigid=True, return_hyps=True, return_bones=True, **kw)
    for h, h0, L in zip(_np(hyps), _np(off_h), _np(bones)):
        assert h.shape == h0.shape and h.shape[1:] == (K, 17, 4)
        assert np.array_equal(_bits(h[..., 3]), _bits(h0[..., 3]))
        assert np.abs(ref.bone_lengths(h) - L.astype(np.float64)).max() <= LEN_TOL
        assert np.abs(h.astype(np.float64) - ref.project_all(h0, L[None], [0, len(h0)])).max() <= POS_TOL
    # symmetric: the pairs of the table are equal, and so are the output's left and right bones
    for source in ("model", "measured"):
        sym, sbones = lift_sequences(model, p2, rigid=True, lengths=source, symmetric=True, return_bones=True, **kw)
        _, raw = lift_sequences(model, p2, rigid=True, lengths=source, return_bones=True, **kw)
        for g, L, r in zip(_np(sym), _np(sbones), _np(raw)):
            assert np.array_equal(L[list(ref.BONES_LEFT)], L[list(ref.BONES_RIGHT)])
            np.testing.assert_allclose(L, ref.symmetrise(r), rtol=2e-7, atol=0)
            bl = ref.bone_lengths(g)
            assert np.abs(bl[:, list(ref.BONES_LEFT)] - bl[:, list(ref.BONES_RIGHT)]).max() <= LEN_TOL
            assert np.abs(bl - L.astype(np.float64)).max() <= LEN_TOL
    # a caller's (16,) table is used verbatim, and scale multiplies poses and lengths alike (millimetres: the bounds scale with it)
    table = np.random.default_rng(2).uniform(0.05, 0.6, 16).astype(np.float32)
    base_mm = _np(lift_sequences(model, p2, scale=1000.0, **kw))
    got_mm, tb = lift_sequences(model, p2, rigid=True, lengths=table, scale=1000.0, return_bones=True, **kw)
    got_mm, tb = _np(got_mm), _np(tb)
    assert all(np.array_equal(_bits(t), _bits(table)) for t in tb)
    _check_projection(got_mm, base_mm, tb, tol=1000 * POS_TOL, scale=1000.0)
    for g in got_mm:
        assert np.abs(ref.bone_lengths(g) - 1000.0 * table.astype(np.float64)).max() <= 1000 * LEN_TOL
    per_seq = np.stack([table, 2 * table, 0.5 * table])                   # an (S, 16) table: one row per sequence
    got_s, sb = lift_sequences(model, p2, rigid=True, lengths=torch.from_numpy(per_seq), return_bones=True, **kw)
    for g, L, want in zip(_np(got_s), _np(sb), per_seq):
        assert np.array_equal(_bits(L), _bits(want)) and np.abs(ref.bone_lengths(g) - want.astype(np.float64)).max() <= LEN_TOL
    # "measured" in millimetres: the table comes back in metres
    mm, mb = lift_sequences(model, p2, rigid=True, lengths="measured", scale=1000.0, return_bones=True, **kw)
    for g, L, b in zip(_np(mm), _np(mb), base_mm):
        want_L = ref.mean_bone_lengths(b, [0, len(b)])[0] / 1000.0
        assert (np.abs(L - want_L) / want_L).max() <= 1e-6
        assert np.abs(ref.bone_lengths(g) - 1000.0 * L.astype(np.float64)).max() <= 1000 * LEN_TOL


def test_rigid_lift_entry_point(lib, tmp_path, monkeypatch):
    sys.path.insert(0, os.path.join(ROOT, "hpe"))
    from _entry import run
    monkeypatch.chdir(tmp_path)
    run(["run.train=false", "run.test=false", "run.lift=true", "lift.rigid=true", "lift.hyps=true", "lift.stride=14", "train.batch_size_test=4",
         "data.seq_len=27", "model.channels=64", "model.layers=2", "model.nheads=4", "model.channels_seg=32", "model.layers_seg=1",
         "model.nheads_seg=4", "multi_hyp.n_hyp=3", "data.synthetic_sequences=3", "model.precision=fp32"])
    z = np.load(os.path.join(str(tmp_path), "default", "lift.npz"))
    keys = [f"synthetic_{i:03d}" for i in range(3)]
    assert sorted(z.files) == sorted(keys + [k + "__hyps" for k in keys] + [k + "__bones" for k in keys])
    for i, k in enumerate(keys):
        n = 27 * 4 + 37 * i + 11
        assert z[k].shape == (n, 17, 3) and z[k + "__hyps"].shape == (n, 3, 17, 4) and z[k + "__bones"].shape == (16,)
        assert np.isfinite(z[k]).all() and (z[k + "__bones"] > 0).all()
        assert ref.bone_lengths(z[k]).std(axis=0).max() <= LEN_TOL
        assert np.abs(ref.bone_lengths(z[k]) - z[k + "__bones"].astype(np.float64)).max() <= LEN_TOL
        assert np.abs(ref.bone_lengths(z[k + "__hyps"]) - z[k + "__bones"].astype(np.float64)).max() <= LEN_TOL

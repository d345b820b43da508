"""Sequence lifting on the device: mp_lift_merge against fp64 element by element, determinism and independence of the sequences, the
whole of lift_sequences against the CPU oracle applied per window and stitched in numpy (lift_ref.py), lift_action against the
evaluation path, and the run.lift entry point."""
import ctypes as C
import itertools
import os
import sys

import numpy as np
import pytest
import torch

import manipose_ref as orc
from helpers import fixture_state, load_fixture
from lift_fixtures import FIXTURES, fixture_model as _model, sequences as _sequences
from lift_ref import MIRROR, closed_form_tables, covering, cut_windows, oracle_lift, unflip

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24
MIRROR_C = (C.c_int32 * 17)(*MIRROR.tolist())


def _rand_inputs(F, W, K, T, seed, scores=True):
    g = np.random.default_rng(seed)
    poses = g.standard_normal((F * W, K, T, 17, 3)).astype(np.float32)
    sc = None
    if scores:
        z = g.standard_normal((F * W, K, T, 1)) * 2
        e = np.exp(z - z.max(1, keepdims=True))
        sc = (e / e.sum(1, keepdims=True)).astype(np.float32)            # a softmax over K
    return poses, sc


def _half(poses, scores, agg):
    """fp64 p_w (W,T,17,3) of one half, the sum of |terms| behind every element, and the number of products in it."""
    p = poses.astype(np.float64)
    if scores is None:
        return p[:, 0], np.abs(p[:, 0]), 1
    s = scores.astype(np.float64)[..., None]                               # (W,K,T,1,1)
    if agg == "weighted_ave":
        return (p * s).sum(1), np.abs(p * s).sum(1), p.shape[1]
    kb = np.argmax(scores[..., 0], axis=1)                                 # first maximal fp32 score
    sel = np.take_along_axis(p, kb[:, None, :, None, None], axis=1)[:, 0]
    return sel, np.abs(sel), 1


def _want(poses, scores, W, T, tta, win_seq, win_start, lens, agg, blend, scale, cov=None):
    """fp64 result of the merge from the same fp32 inputs, with the derived bound (n + 3) 2^-24 S per element."""
    pw, aw, n1 = _half(poses[:W], scores[:W] if scores is not None else None, agg)
    F = 2 if tta else 1
    if tta:
        p1, a1, _ = _half(poses[W:], scores[W:] if scores is not None else None, agg)
        pw, aw = (pw + unflip(p1)) / 2, (aw + a1[..., MIRROR, :]) / 2
    K = poses.shape[1]
    ph = poses[:W].astype(np.float64).transpose(0, 2, 1, 3, 4)             # (W,T,K,17,3)
    sh = (scores[:W].astype(np.float64) if scores is not None else np.ones((W, K, T, 1))).transpose(0, 2, 1, 3)[..., None, :]
    hw = np.concatenate([ph, np.broadcast_to(sh, ph.shape[:-1] + (1,))], axis=-1)
    sc = np.float64(np.float32(scale))
    hscale = np.array([sc, sc, sc, 1.0])
    out, bnd, hyp, hbnd, nwin = [], [], [], [], []
    g = 0
    for s, n in enumerate(lens):
        for f in range(n):
            ws = cov[g] if cov is not None else covering(win_seq, win_start, s, f, T, blend)
            g += 1
            ts = [f - int(win_start[w]) for w in ws]
            m = len(ws)
            out.append(sum(pw[w, t] for w, t in zip(ws, ts)) / m * sc)
            S = sum(aw[w, t] for w, t in zip(ws, ts)) / m * sc
            bnd.append((m * F * n1 + 3) * U * S)
            hyp.append(sum(hw[w, t] for w, t in zip(ws, ts)) / m * hscale)
            hbnd.append((m + 3) * U * sum(np.abs(hw[w, t]) for w, t in zip(ws, ts)) / m * hscale)
            nwin.append(m)
    return np.stack(out), np.stack(bnd), np.stack(hyp), np.stack(hbnd), np.array(nwin)


def _check(got, got_h, want, bnd, want_h, bnd_h, nwin, K, lens, scale, exact, tag):
    assert got.shape == want.shape == (sum(lens), 17, 3)
    err = np.abs(got.astype(np.float64) - want)
    ratio = float((err / np.maximum(bnd, 1e-300)).max())
    assert np.all(err <= bnd), (tag, ratio)                               # no element excluded
    if got_h is not None:
        assert got_h.shape == want_h.shape == (sum(lens), K, 17, 4)
        eh = np.abs(got_h.astype(np.float64) - want_h)
        assert np.all(eh <= bnd_h), (tag, float((eh / np.maximum(bnd_h, 1e-300)).max()))
    if exact:                                                             # one covering window, best_score, no TTA: the selected hypothesis times scale
        one = nwin == 1
        assert one.any()
        sel = want[one].astype(np.float32) if scale == 1.0 else (want[one] / np.float64(np.float32(scale))).astype(np.float32) * np.float32(scale)
        assert np.array_equal(got[one], sel), tag
    return ratio


def _merge(poses, scores, T, tta, win_seq, win_start, lens, agg, blend, scale, hyps):
    from manipose_amd.lifting import merge_windows
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    o, h = merge_windows(torch.from_numpy(poses).cuda(), torch.from_numpy(scores).cuda() if scores is not None else None, win_seq, win_start, off,
                         T=T, tta=tta, mirror=MIRROR_C, agg=agg, blend=blend, scale=scale, return_hyps=hyps)
    torch.cuda.synchronize()
    return o.cpu().numpy(), (h.cpu().numpy() if hyps else None)


KERNEL_CASES = [(K, T, st) for K in (1, 3, 5, 8) for T in (27, 243) for st in ("T", "half", "one") if not (st == "one" and T == 243)]


@pytest.mark.parametrize("K,T,stride_name", KERNEL_CASES)
def test_lift_merge_kernel_against_fp64(lib, K, T, stride_name):
    """Random hypotheses and softmax scores straight into mp_lift_merge, every element of every output against fp64 within
    (n + 3) 2^-24 S: n products summed into the element (covering windows used x F x K for weighted_ave, x 1 for best_score), S the fp64
    sum of the absolute values of those terms after normalisation.  One covering window + best_score + no TTA: bit-equal."""
    stride = {"T": T, "half": T // 2 + 1, "one": 1}[stride_name]
    lens = [T - 4, T + 1, 2 * T + 5, T] if stride > 1 else [T - 4, T + 1, T + 9]
    win_seq, win_start = closed_form_tables(lens, T, stride)
    W = len(win_seq)
    worst = 0.0
    cov = {b: [covering(win_seq, win_start, s, f, T, b) for s, n in enumerate(lens) for f in range(n)] for b in ("mean", "center")}
    for tta, use_scores in ((False, True), (True, True), (False, False), (True, False)):
        if not use_scores and K > 1:
            continue
        poses, scores = _rand_inputs(2 if tta else 1, W, K, T, seed=1000 * K + T + stride, scores=use_scores)
        for agg, blend in itertools.product(("weighted_ave", "best_score"), ("mean", "center")):
            for hyps in (False, True):
                scale = 1000.0 if hyps else 1.0
                got, got_h = _merge(poses, scores, T, tta, win_seq, win_start, lens, agg, blend, scale, hyps)
                want, bnd, want_h, bnd_h, nwin = _want(poses, scores, W, T, tta, win_seq, win_start, lens, agg, blend, scale, cov[blend])
                worst = max(worst, _check(got, got_h, want, bnd, want_h, bnd_h, nwin, K, lens, scale, exact=agg == "best_score" and not tta,
                                          tag=(tta, agg, blend, hyps)))
    print(f"\n[lift_merge K={K} T={T} stride={stride}] worst |err| / bound = {worst:.3f}")


def test_lift_merge_is_deterministic_and_center_best_returns_input_hypotheses(lib):
    T, K = 27, 5
    lens = [20, 28, 59, 100]
    win_seq, win_start = closed_form_tables(lens, T, T // 2 + 1)
    W = len(win_seq)
    poses, scores = _rand_inputs(2, W, K, T, seed=9)
    a = _merge(poses, scores, T, True, win_seq, win_start, lens, "weighted_ave", "mean", 1.0, True)
    b = _merge(poses, scores, T, True, win_seq, win_start, lens, "weighted_ave", "mean", 1.0, True)
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
    got, _ = _merge(poses[:W], scores[:W], T, False, win_seq, win_start, lens, "best_score", "center", 1.0, False)
    g = 0
    for s, n in enumerate(lens):
        for f in range(n):
            w = covering(win_seq, win_start, s, f, T, "center")[0]
            t = f - int(win_start[w])
            assert any(np.array_equal(got[g], poses[w, k, t]) for k in range(K)), (s, f)      # exactly one input hypothesis
            g += 1


def test_lift_sequences_is_reproducible_and_sequences_do_not_interact(lib):
    from manipose_amd import lift_sequences
    model, T, K = _model("rmcl")
    p2, _ = _sequences([T - 7, 2 * T, 3 * T + 5], seed=4)
    for stride, batch in ((T, 2), (T // 2 + 1, 3)):
        a, ah = lift_sequences(model, p2, stride=stride, batch=batch, return_hyps=True)
        b, bh = lift_sequences(model, p2, stride=stride, batch=batch, return_hyps=True)
        for i in range(3):
            assert a[i].shape == (len(p2[i]), 17, 3) and ah[i].shape == (len(p2[i]), K, 17, 4)
            assert torch.equal(a[i], b[i]) and torch.equal(ah[i], bh[i])                      # two calls: identical bits
            alone, alone_h = lift_sequences(model, [torch.from_numpy(p2[i]).cuda()], stride=stride, batch=batch, return_hyps=True)
            assert torch.equal(a[i], alone[0]) and torch.equal(ah[i], alone_h[0])             # together == alone, bit for bit
    # center + best_score + no TTA: every output frame is one hypothesis of the model, so a window's frames share their bone lengths
    # (the manifold property; tolerance of test_full_size_model_T243_K5_vs_oracle_and_manifold_property: rtol 1e-4, atol 2e-6)
    out = lift_sequences(model, p2, stride=T, tta=False, agg="best_score", blend="center")
    par = torch.tensor(orc.H36M_PARENTS[1:], device="cuda")
    for o in out:
        seg = (o[:, 1:, :] - o[:, par, :]).norm(dim=-1)
        for a0 in range(0, o.shape[0], T):
            blk = seg[a0:a0 + T]
            np.testing.assert_allclose(blk.cpu().numpy(), blk[:1].expand_as(blk).cpu().numpy(), rtol=1e-4, atol=2e-6)
    win_seq, win_start = closed_form_tables([len(a) for a in p2], T, T)
    X = torch.from_numpy(cut_windows(p2, win_seq, win_start, T)).cuda()
    for s in range(3):                                                    # the forward of a sequence's windows, as lift_sequences batches them
        with torch.no_grad():
            poses, _ = model(X[torch.from_numpy(win_seq == s).cuda()].contiguous())
        for f in range(len(p2[s])):
            assert any(torch.equal(out[s][f], poses[f // T, k, f % T]) for k in range(poses.shape[1])), (s, f)


def _oracle_forward(kind, fx):
    st = fixture_state(fx)
    if kind == "rmcl":
        cfg = orc.oracle_cfg(fx["cfg"])
        return lambda x: orc.rmcl_manifold_forward(x, st, cfg)
    if kind == "manifold":
        cfg = orc.oracle_cfg(fx["cfg"])
        return lambda x: (orc.manifold_forward(x, st, cfg)[:, None], None)
    T, C_, depth, heads = [int(v) for v in fx["cfg_mixste"]]
    return lambda x: (orc.mixste_forward(x, st, "", depth, heads)[:, None], None)


@pytest.mark.parametrize("kind", ["rmcl", "manifold", "mixste"])
def test_lift_sequences_end_to_end_vs_oracle(lib, kind):
    """fp32 models on 3 synthetic sequences, TTA on, stride T and T // 2 + 1, against the CPU oracle per window + pose_flip + numpy stitching.
    Bound: the one test_rmcl_model_forward_loss_backward_vs_reference applies to `poses` (tests/test_gpu_parity.py:424: rtol 1e-4, atol 2e-5)."""
    from manipose_amd import lift_sequences
    model, T, _ = _model(kind)
    p2, _ = _sequences([T - 5, 2 * T, 2 * T + 5], seed=12)
    fwd = _oracle_forward(kind, load_fixture(FIXTURES[kind]))
    for stride in (T, T // 2 + 1):
        got = lift_sequences(model, p2, stride=stride, tta=True, batch=2)
        with torch.no_grad():
            want = oracle_lift(fwd, p2, T, stride, tta=True)
        for g, w in zip(got, want):
            assert g.shape == w.shape
            np.testing.assert_allclose(g.cpu().numpy(), w, rtol=1e-4, atol=2e-5)
    if kind == "rmcl":                                                   # the hypotheses too, and best_score / center
        got, got_h = lift_sequences(model, p2, stride=T // 2 + 1, tta=True, agg="best_score", blend="center", return_hyps=True, batch=3)
        with torch.no_grad():
            want, want_h = oracle_lift(fwd, p2, T, T // 2 + 1, tta=True, agg="best_score", blend="center", hyps=True)
        for g, w, gh, wh in zip(got, want, got_h, want_h):
            np.testing.assert_allclose(g.cpu().numpy(), w, rtol=1e-4, atol=2e-5)
            np.testing.assert_allclose(gh.cpu().numpy(), wh, rtol=1e-4, atol=2e-5)


def test_lift_action_agrees_with_the_evaluation_path(lib):
    """lift_action at stride T (padded frames kept) scored by mpjpe_error gives evaluate(..., tta=True)'s mpjpe on the same windows, and
    agg="best_score" its ps_oracle_mpjpe; allowance of test_batched_flip_tta_matches_two_pass_reference_procedure: 1e-3 want + 0.05 mm."""
    sys.path.insert(0, os.path.join(ROOT, "hpe"))
    from _entry import evaluate
    from manipose_amd import lift_action, lift_sequences
    from manipose_amd.hydra_lite import Cfg
    from manipose_amd.metrics import mpjpe_error
    model, T, K = _model("rmcl")
    p2, p3 = _sequences([T - 7, 2 * T, 2 * T + 5], seed=8)
    win_seq, win_start = closed_form_tables([len(a) for a in p2], T, T)
    X = torch.from_numpy(cut_windows(p2, win_seq, win_start, T)).cuda()
    y = torch.from_numpy(cut_windows(p3, win_seq, win_start, T)).cuda()
    want = evaluate(model, X, y, batch=2, tta=True)
    cfg = Cfg.wrap({"train": {"tta": True}})
    pred = lift_action(model, p2, cfg, False)
    assert isinstance(pred, np.ndarray) and pred.shape == (len(win_seq) * T, 17, 3)
    got = 1000.0 * mpjpe_error(torch.from_numpy(pred).cuda(), y.reshape(-1, 17, 3), "average").item()
    assert abs(got - want["mpjpe"]) <= 1e-3 * want["mpjpe"] + 0.05, (got, want)
    hy = lift_action(model, p2, cfg, True)
    assert hy.shape == (len(win_seq) * T, K, 17, 4)
    np.testing.assert_allclose(hy[..., 3].sum(1), 1.0, atol=1e-5)                            # the scores of a frame sum to one
    best = torch.cat(lift_sequences(model, p2, tta=True, agg="best_score", keep_padding=True))
    got_b = 1000.0 * mpjpe_error(best, y.reshape(-1, 17, 3), "average").item()
    assert abs(got_b - want["ps_oracle_mpjpe"]) <= 1e-3 * want["ps_oracle_mpjpe"] + 0.05, (got_b, want)


def test_lift_entry_point_and_argument_errors(lib, tmp_path, monkeypatch):
    sys.path.insert(0, os.path.join(ROOT, "hpe"))
    from _entry import run
    from manipose_amd import lift_sequences
    monkeypatch.chdir(tmp_path)
    run(["run.train=false", "run.test=false", "run.lift=true", "lift.hyps=true", "lift.stride=14", "train.batch_size_test=4", "data.seq_len=27",
         "model.channels=64", "model.layers=2", "model.nheads=4", "model.channels_seg=32", "model.layers_seg=1", "model.nheads_seg=4",
         "multi_hyp.n_hyp=3", "data.synthetic_sequences=3", "model.precision=fp32"])
    z = np.load(os.path.join(str(tmp_path), "default", "lift.npz"))
    assert sorted(z.files) == sorted([f"synthetic_{i:03d}" for i in range(3)] + [f"synthetic_{i:03d}__hyps" for i in range(3)])
    for i in range(3):
        n = 27 * 4 + 37 * i + 11
        assert z[f"synthetic_{i:03d}"].shape == (n, 17, 3) and z[f"synthetic_{i:03d}__hyps"].shape == (n, 3, 17, 4)
        assert np.isfinite(z[f"synthetic_{i:03d}"]).all()
    # CPU input / CPU model: RuntimeError, never a fallback
    model = _model("rmcl")[0]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        lift_sequences(model, [torch.zeros(30, 17, 2)])
    with pytest.raises(ValueError):
        lift_sequences(model, [np.zeros((30, 17, 2), np.float32)], stride=28)
    with pytest.raises(ValueError):
        lift_sequences(model, [np.zeros((30, 17, 2), np.float32)], agg="oracle")
    # argument errors of the C entry point: MP_ERR_ARG with a message, before any launch
    T, K, W = 27, 3, 2
    poses = torch.zeros(W, K, T, 17, 3, device="cuda")
    scores = torch.full((W, K, T, 1), 1.0 / K, device="cuda")
    out = torch.zeros(2 * T, 17, 3, device="cuda")
    seq, start, off = np.zeros(W, np.int32), np.array([0, T], np.int32), np.array([0, 2 * T], np.int64)
    d = [torch.from_numpy(a).cuda() for a in (seq, start, off)]
    i32p, i64p = C.POINTER(C.c_int32), C.POINTER(C.c_int64)

    def call(poses_p=poses.data_ptr(), K_=K, J_=17, agg=0, blend=0, h_start=start, h_off=off):
        return lib.mp_lift_merge(poses_p, scores.data_ptr(), W, K_, T, J_, 0, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), 1,
                                 seq.ctypes.data_as(i32p), h_start.ctypes.data_as(i32p), h_off.ctypes.data_as(i64p), MIRROR_C, agg, blend, 1.0,
                                 out.data_ptr(), None, None)
    assert call() == 0
    for kw, word in ((dict(poses_p=None), b"null"), (dict(K_=0), b"K=0"), (dict(K_=9), b"K=9"), (dict(J_=33), b"J=33"), (dict(agg=2), b"agg"),
                     (dict(blend=-1), b"blend"), (dict(h_off=np.array([0, 2 * T + 1], np.int64)), b"no window covers"),
                     (dict(h_start=np.array([0, T + 1], np.int32)), b"no window covers")):
        assert call(**kw) == 1 and word in lib.mp_last_error(), (kw, lib.mp_last_error())
    assert lib.mp_lift_windows_2d(None, None, 1, None, None, None, None, 1, T, 17, None, None) == 1 and b"null" in lib.mp_last_error()
    torch.cuda.synchronize()

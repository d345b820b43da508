"""mp_hypothesis_stats (manipose_amd/csrc/hypothesis_stats.hip) and what is built on it: hypothesis_stats, the reference-named
calc_jbest_mpjpe / calc_jbest_pose, HypothesisAccumulator, evaluate(hypotheses=True) and the files of run.hyp_report.

The C ABI is held against a float64 numpy restatement computed from the SAME float32 inputs.  Bounds (derived, not tuned), u = 2^-24,
c = the largest |scaled coordinate|, S = the largest per-frame sum of scores:
  * a distance e = ||q - g|| of scaled coordinates (one rounding each, then a handful more): |e - e64| <= d_e = 8 u (c + max e);
  * a pose error E, the sum of 17 distances: 17 d_e;
  * the weighted mean w = sum_k s_k q_k is K products and K - 1 additions of numbers whose magnitudes sum to at most S c, on q_k that
    carry a rounding themselves: |w - w64| <= d_w = (K + 2) u S c per coordinate, sqrt(3) d_w in a norm.  The weighted-average term
    ||w - g|| therefore carries 8 u (c + max ||w - g||) + sqrt(3) d_w;
  * the spread sqrt(sum_k s_k ||q_k - w||^2) is the norm of the 3 K numbers sqrt(s_k) (q_k - w)_i.  A component (q_k - w)_i is off by at
    most delta = u c + d_w + u max|q_k - w| (rounding of q, error of w, the subtraction), the norm by sqrt(3 S) delta; the K squares, sums,
    the products with s_k and the root add (K + 8) u relative: sqrt(3 S) delta + (K + 8) u max spread;
  * a pairwise term 2/(K(K-1)) sum_{k<k'} ||q_k - q_k'||: every distance 8 u (c + max distance), the weights of the P = K(K-1)/2 pairs sum
    to 1, the P additions and the product add (P + 2) u relative;
  * scores and score masses are the inputs themselves: no error in a term;
  * a reduced sum of n terms: n x (the term's bound) + (m + 3) u sum|terms|, m = the number of terms of one block's partial sum.
Counts and indices must EQUAL the float64 ones, for every frame: each case first asserts on the host, in float64, that per frame and
joint the two smallest e[.][j] differ by more than 2 d_e and that ALL pairs of E[k] of a frame differ by more than 2 x 17 d_e (top-m
needs every pair), and that no two scores of a frame are equal.  The data are built to keep those gaps: hypothesis = target + unit
direction x (5 + 3 q + 1.1 r) mm, q a per-(frame, joint) permutation of 0..K-1, r a per-frame one (pose errors then differ by
3 a + 18.7 b mm with b != 0: at least 0.2 mm); scores are positive and normalised over K."""
import ctypes as C
import csv
import os
import re
import sys

import numpy as np
import pytest
import torch

from helpers import fixture_state, load_fixture

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "manipose_amd", "csrc", "hypothesis_stats.hip")) as _f:
    FPB = int(re.search(r"constexpr int HS_FPB = (\d+);", _f.read()).group(1))      # frames per workgroup = terms of one block's partial sum
# the rows of include/manipose_hip.h, mp_hypothesis_stats
F_FRAMES, F_BEST, F_ORACLE, F_JBEST, F_WAVE, F_S_ORACLE, F_S_MAX, F_PAIR, F_TOPM, F_JB_JOINT, F_SPREAD, F_MASS, NF = 0, 1, 2, 3, 4, 5, 6, 7, 8, 16, 33, 50, 58
C_AGREE, C_ORANK, C_PBEST, C_SHEAD, C_JHEAD, NI = 0, 1, 9, 17, 25, 33


def make(B, K, T, seed, unit=0.001):
    """(B, K, T, 17, 3) hypotheses, (B, K, T) scores, (B, T, 17, 3) target, float32; ``unit`` = one millimetre in the data's unit."""
    g = np.random.default_rng(seed)
    gt = 250.0 * g.standard_normal((1, 1, 17, 3)) + 2.0 * np.cumsum(g.standard_normal((B, T, 17, 3)), 1)
    gt[:, :, 0] = 0
    d = g.standard_normal((B, K, T, 17, 3))
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    q = np.argsort(g.random((B, T, 17, K)), -1).transpose(0, 3, 1, 2)      # per (frame, joint) permutation of 0..K-1
    r = np.argsort(g.random((B, T, K)), -1).transpose(0, 2, 1)[..., None]   # per frame permutation
    hyp = gt[:, None] + d * (5.0 + 3.0 * q + 1.1 * r)[..., None]
    s = g.random((B, K, T)) + 0.05
    s /= s.sum(1, keepdims=True)
    return (unit * hyp).astype(np.float32), s.astype(np.float32), (unit * gt).astype(np.float32)


def reference(hyp, s, gt, pose_scale, target_scale, twins=None):
    """float64 restatement of every output with its tolerance.  ``twins`` = (a, b), a < b: hypothesis b is a copy of hypothesis a (the
    gap assertions leave that pair out; the first arg-min settles it)."""
    B, K, T = hyp.shape[:3]
    N = B * T
    q = np.float64(np.float32(pose_scale)) * hyp.astype(np.float64)
    g = np.float64(np.float32(target_scale)) * gt.astype(np.float64)
    s = s.astype(np.float64)
    e = np.sqrt(((q - g[:, None]) ** 2).sum(-1))                             # (B, K, T, 17)
    E = e.sum(-1)                                                            # (B, K, T)
    c = max(np.abs(q).max(), np.abs(g).max())
    d_e = 8 * U * (c + e.max())
    # ---- the gaps that make the indices a matter of the data, not of rounding
    keep = [k for k in range(K) if twins is None or k != twins[1]]
    if len(keep) > 1:
        es = np.sort(e[:, keep], axis=1)
        joint_gap = (es[:, 1] - es[:, 0]).min()
        pose_gap = min(np.abs(E[:, a] - E[:, b]).min() for i, a in enumerate(keep) for b in keep[i + 1:])
        print(f"d_e {d_e:.3e}  smallest joint gap {joint_gap:.3e} (> {2 * d_e:.3e})  smallest pose gap {pose_gap:.3e} (> {34 * d_e:.3e})")
        assert joint_gap > 2 * d_e and pose_gap > 2 * 17 * d_e, "the test data must separate every arg-min from rounding"
    ko, ks, kj = E.argmin(1), s.argmax(1), e.argmin(1)                        # first minimum / maximum; (B, T), (B, T), (B, T, 17)
    order = np.argsort(-s, axis=1, kind="stable")                            # descending, equal scores in the order of their indices
    rank = np.argsort(order, axis=1, kind="stable")                          # place of hypothesis k
    Eord = np.take_along_axis(E, order, axis=1)
    topm = np.minimum.accumulate(Eord, axis=1)                               # (B, K, T): best of the m + 1 best-scored
    pick = lambda a, k: np.take_along_axis(a, k[:, None], axis=1)[:, 0]
    w = (s[..., None, None] * q).sum(1)                                      # (B, T, 17, 3)
    ew = np.sqrt(((w - g) ** 2).sum(-1))
    dev = q - w[:, None]
    spread = np.sqrt((s[..., None] * (dev ** 2).sum(-1)).sum(1))             # (B, T, 17)
    P = K * (K - 1) // 2
    pair = np.zeros((B, T, 17))
    dmax = 0.0
    for a in range(K):
        for b in range(a + 1, K):
            dist = np.sqrt(((q[:, a] - q[:, b]) ** 2).sum(-1))
            pair += dist / P
            dmax = max(dmax, dist.max())
    S = s.sum(1).max()
    d_w = (K + 2) * U * S * c
    d_wave = 8 * U * (c + ew.max()) + np.sqrt(3.0) * d_w
    d_spread = np.sqrt(3.0 * S) * (U * c + d_w + U * np.abs(dev).max()) + (K + 8) * U * spread.max()
    d_pair = 8 * U * (c + dmax) + (P + 2) * U * pair.max()
    m = min(N, FPB)
    fs, tol = np.zeros(NF), np.zeros(NF)

    def put(i, terms, term_bound, per_frame):
        """terms: (frames, ...) per-frame (per_frame joints each) values of slot i, or (frames, n) for n slots from i on"""
        t = terms.reshape(N, -1) if terms.ndim > 1 else terms.reshape(N, 1)
        fs[i:i + t.shape[1]] = t.sum(0)
        tol[i:i + t.shape[1]] = N * per_frame * term_bound + (m * per_frame + 3) * U * np.abs(t).sum(0)

    fs[F_FRAMES] = N
    put(F_BEST, pick(E, ks), 17 * d_e, 1)
    put(F_ORACLE, pick(E, ko), 17 * d_e, 1)
    put(F_JBEST, e.min(1).sum(-1), d_e, 17)
    put(F_WAVE, ew.sum(-1), d_wave, 17)
    put(F_S_ORACLE, pick(s, ko), 0.0, 1)
    put(F_S_MAX, pick(s, ks), 0.0, 1)
    put(F_PAIR, pair.sum(-1), d_pair, 17)
    put(F_TOPM, topm.transpose(0, 2, 1), 17 * d_e, 1)
    put(F_JB_JOINT, e.min(1), d_e, 1)
    put(F_SPREAD, spread, d_spread, 1)
    put(F_MASS, s.transpose(0, 2, 1), 0.0, 1)
    cnt = np.zeros(NI, dtype=np.int64)
    cnt[C_AGREE] = (ko == ks).sum()
    cnt[C_ORANK:C_ORANK + K] = np.bincount(pick(rank, ko).reshape(-1), minlength=K)
    cnt[C_PBEST:C_PBEST + K] = np.bincount(ko.reshape(-1), minlength=K)
    cnt[C_SHEAD:C_SHEAD + K] = np.bincount(ks.reshape(-1), minlength=K)
    cnt[C_JHEAD:C_JHEAD + K] = np.bincount(kj.reshape(-1), minlength=K)
    jpose = np.take_along_axis(hyp, kj[:, None, :, :, None].repeat(3, axis=-1), axis=1)[:, 0]      # the input's float32 values
    return {"sums": fs, "tol": tol, "counts": cnt, "jbest_idx": kj.astype(np.uint8), "jbest_pose": jpose, "ko": ko, "ks": ks}


def call(lib, hyp, s, gt, pose_scale, target_scale, jbest=True):
    """mp_hypothesis_stats through the C ABI -> dict of host arrays (outputs pre-filled with values the kernel never writes)."""
    from manipose_amd import _lib
    B, K, T = hyp.shape[:3]
    h, sc, y = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (hyp, s, gt))
    sums = torch.full((int(lib.mp_hypothesis_stats_row_floats()),), float("nan"), device="cuda")
    counts = torch.full((int(lib.mp_hypothesis_stats_row_counts()),), -7, dtype=torch.int64, device="cuda")
    jp = torch.full((B, T, 17, 3), float("nan"), device="cuda") if jbest else None
    ji = torch.full((B, T, 17), 255, dtype=torch.uint8, device="cuda") if jbest else None
    scratch = torch.empty(int(lib.mp_hypothesis_stats_scratch_floats(B * T)), device="cuda")
    _lib.check(lib.mp_hypothesis_stats(h.data_ptr(), sc.data_ptr(), y.data_ptr(), B, K, T, pose_scale, target_scale, sums.data_ptr(),
                                       counts.data_ptr(), jp.data_ptr() if jbest else None, ji.data_ptr() if jbest else None,
                                       scratch.data_ptr(), scratch.numel(), torch.cuda.current_stream().cuda_stream), "mp_hypothesis_stats")
    torch.cuda.synchronize()
    out = {"sums": sums.cpu().numpy(), "counts": counts.cpu().numpy()}
    if jbest:
        out["jbest_pose"], out["jbest_idx"] = jp.cpu().numpy(), ji.cpu().numpy()
    return out


def check(got, want, K):
    assert got["sums"].shape == (NF,) and got["counts"].shape == (NI,) and got["counts"].dtype == np.int64
    err = np.abs(got["sums"].astype(np.float64) - want["sums"])
    for name, i, n in (("best score", F_BEST, 1), ("oracle", F_ORACLE, 1), ("J-Best", F_JBEST, 1), ("weighted ave", F_WAVE, 1),
                       ("score of oracle", F_S_ORACLE, 1), ("largest score", F_S_MAX, 1), ("pairwise", F_PAIR, 1), ("top-m", F_TOPM, 8),
                       ("J-Best per joint", F_JB_JOINT, 17), ("spread per joint", F_SPREAD, 17), ("score mass", F_MASS, 8)):
        print(f"{name:18s} value {want['sums'][i]:.6e}  largest error {err[i:i + n].max():.3e}  its tolerance {want['tol'][i:i + n][err[i:i + n].argmax()]:.3e}")
    assert got["sums"][F_FRAMES] == want["sums"][F_FRAMES]
    assert (err <= want["tol"]).all(), np.nonzero(err > want["tol"])[0]
    assert (got["sums"][F_TOPM + K:F_TOPM + 8] == 0).all() and (got["sums"][F_MASS + K:F_MASS + 8] == 0).all()
    assert np.array_equal(got["counts"], want["counts"]), (got["counts"], want["counts"])
    # the slot identities: top-1 is the best-scored hypothesis, top-K the oracle - the same bits
    assert got["sums"][F_TOPM].tobytes() == got["sums"][F_BEST].tobytes() and got["sums"][F_TOPM + K - 1].tobytes() == got["sums"][F_ORACLE].tobytes()
    if "jbest_idx" in got:
        assert np.array_equal(got["jbest_idx"], want["jbest_idx"])
        assert got["jbest_pose"].tobytes() == want["jbest_pose"].tobytes()          # the gathered input, bit for bit


CASES = [(1, 1, 1), (2, 2, 7), (2, 5, 27), (3, 8, 43), (1, 2, 515), (1, 5, FPB - 1), (1, 5, FPB), (1, 5, FPB + 1), (1, 5, 2 * FPB + 1),
         (1, 8, 2 * FPB + 1), (1, 5, 600)]


@pytest.mark.parametrize("B,K,T", CASES)
def test_hypothesis_stats_against_float64(lib, B, K, T):
    """Metres in, pose_scale = target_scale = 1000: one frame; K of 1, 2, 5, 8; frame counts around one and two workgroups' worth."""
    hyp, s, gt = make(B, K, T, seed=1000 * B + 10 * T + K)
    assert K == 1 or np.diff(np.sort(s, axis=1), axis=1).min() > 0
    check(call(lib, hyp, s, gt, 1000.0, 1000.0), reference(hyp, s, gt, 1000.0, 1000.0), K)


def test_millimetres_in_with_scale_one_and_without_the_optional_outputs(lib):
    hyp, s, gt = make(2, 5, 27, seed=3, unit=1.0)
    want = reference(hyp, s, gt, 1.0, 1.0)
    check(call(lib, hyp, s, gt, 1.0, 1.0), want, 5)
    check(call(lib, hyp, s, gt, 1.0, 1.0, jbest=False), want, 5)
    # different scales for the two sides: the same poses stored in metres, the target in millimetres
    check(call(lib, (0.001 * hyp.astype(np.float64)).astype(np.float32), s, gt, 1000.0, 1.0, jbest=False),
          reference((0.001 * hyp.astype(np.float64)).astype(np.float32), s, gt, 1000.0, 1.0), 5)


def test_exact_ties_go_to_the_smaller_index(lib):
    """Hypothesis 3 is a copy of hypothesis 1 (the same bits, so the same distances and pose errors): 3 never wins, per joint or per
    pose, and the place of the oracle in the score order is that of hypothesis 1.  Score 4 is a copy of score 2: 2 stands ahead of 4."""
    hyp, s, gt = make(2, 5, 27, seed=21)
    hyp[:, 3] = hyp[:, 1]
    s[:, 4] = s[:, 2]
    want = reference(hyp, s, gt, 1000.0, 1000.0, twins=(1, 3))
    assert (want["ko"] == 1).sum() > 0 and (want["jbest_idx"] == 1).sum() > 0 and (want["ks"] == 2).sum() > 0, "the ties must be at the top somewhere"
    got = call(lib, hyp, s, gt, 1000.0, 1000.0)
    check(got, want, 5)
    assert (got["jbest_idx"] != 3).all() and got["counts"][C_JHEAD + 3] == 0 and got["counts"][C_PBEST + 3] == 0 and got["counts"][C_SHEAD + 4] == 0
    assert got["counts"][C_PBEST + 1] == (want["ko"] == 1).sum() and got["counts"][C_SHEAD + 2] == (want["ks"] == 2).sum()


def test_two_runs_give_identical_bits(lib):
    hyp, s, gt = make(2, 8, 2 * FPB + 5, seed=9)
    a, b = call(lib, hyp, s, gt, 1000.0, 1000.0), call(lib, hyp, s, gt, 1000.0, 1000.0)
    for key in a:
        assert a[key].tobytes() == b[key].tobytes(), key


def test_bad_arguments_are_refused_without_a_launch(lib):
    """K = 9 and a short scratch return MP_ERR_ARG (1); the outputs keep what they held."""
    from manipose_amd.metrics import calc_jbest_mpjpe, hypothesis_stats
    B, T = 2, 5
    h = torch.zeros(B, 9, T, 17, 3, device="cuda")
    s = torch.zeros(B, 9, T, device="cuda")
    y = torch.zeros(B, T, 17, 3, device="cuda")
    sums = torch.full((NF,), -3.0, device="cuda")
    counts = torch.full((NI,), -7, dtype=torch.int64, device="cuda")
    sc = torch.zeros(int(lib.mp_hypothesis_stats_scratch_floats(B * T)), device="cuda")
    args = lambda K, nsc: (h.data_ptr(), s.data_ptr(), y.data_ptr(), B, K, T, 1.0, 1.0, sums.data_ptr(), counts.data_ptr(), None, None, sc.data_ptr(),
                           nsc, None)
    assert lib.mp_hypothesis_stats(*args(9, sc.numel())) == 1 and b"K=9" in lib.mp_last_error()
    assert lib.mp_hypothesis_stats(*args(0, sc.numel())) == 1
    assert lib.mp_hypothesis_stats(*args(8, sc.numel() - 1)) == 1 and b"scratch" in lib.mp_last_error()
    torch.cuda.synchronize()
    assert (sums == -3.0).all() and (counts == -7).all()
    assert lib.mp_hypothesis_stats(*args(8, sc.numel())) == 0
    torch.cuda.synchronize()
    assert sums[F_FRAMES].item() == B * T
    assert int(lib.mp_hypothesis_stats_row_floats()) == NF and int(lib.mp_hypothesis_stats_row_counts()) == NI
    assert int(lib.mp_hypothesis_stats_scratch_floats(FPB + 1)) == 2 * int(lib.mp_hypothesis_stats_scratch_floats(FPB))
    with pytest.raises(RuntimeError):
        hypothesis_stats(h.cpu()[:, :5], s.cpu()[:, :5], y.cpu())            # no CPU fallback
    with pytest.raises(AssertionError):
        hypothesis_stats(h, s, y)                                            # nine hypotheses
    with pytest.raises(RuntimeError):
        calc_jbest_mpjpe(h.cpu()[:, :5], y.cpu())


# ------------------------------------------------------------------------------ the reference's functions, tests/golden/hypotheses.npz
@pytest.fixture(scope="module")
def golden():
    return load_fixture("hypotheses")


def _tiny(name="rmcl_tiny"):
    from manipose_amd import RMCLManifoldMixSTE, h36m_skeleton
    fx = load_fixture(name)
    c = fx["cfg"]
    m = RMCLManifoldMixSTE(h36m_skeleton(), num_frame=c["T"], embed_dim_rot=c["C_rot"], depth_rot=c["depth_rot"], num_heads_rot=c["heads_rot"],
                           embed_dim_seg=c["C_seg"], depth_seg=c["depth_seg"], num_heads_seg=c["heads_seg"], n_hyp=c["n_hyp"], drop_path_rate=0.0)
    m.load_state_dict(fixture_state(fx), strict=True)
    return m.cuda().eval(), c


@pytest.mark.parametrize("i", [0, 1])
def test_reference_named_functions_match_the_reference(lib, golden, i):
    """Both sides are float32 here (the reference ran in torch on the CPU): twice the bounds of the float64 comparison; the J-Best pose
    is a gather of the input and must be the reference's, bit for bit."""
    from manipose_amd.metrics import calc_jbest_mpjpe, calc_jbest_pose, hypothesis_stats
    hyp, s, gt = golden[f"hyp.{i}"], golden[f"scores.{i}"], golden[f"gt.{i}"]
    B, K, L = (int(v) for v in golden["sets"][i])
    assert hyp.shape == (B, K, L, 17, 3)
    want = reference(hyp, s, gt, 1.0, 1.0)
    h, sc, y = (torch.from_numpy(a).cuda() for a in (hyp, s, gt))
    n = B * L * 17
    got = calc_jbest_mpjpe(h, y)
    assert got.shape == () and got.is_cuda
    print("J-Best MPJPE", got.item(), golden[f"jbest_mpjpe.{i}"], "tolerance", 2 * want["tol"][F_JBEST] / n)
    assert abs(got.item() - float(golden[f"jbest_mpjpe.{i}"])) <= 2 * want["tol"][F_JBEST] / n
    pose = calc_jbest_pose(h, y)
    assert pose.shape == (B, L, 17, 3) and pose.cpu().numpy().tobytes() == golden[f"jbest_pose.{i}"].tobytes()
    st = hypothesis_stats(h, sc[..., None], y)                               # scores (B, K, L, 1), as the model returns them
    for key, slot in (("oracle", F_ORACLE), ("best_score", F_BEST), ("weighted_ave", F_WAVE)):
        v = st.sums[slot].item() / n
        print(key, v, golden[f"mpjpe_{key}.{i}"], "tolerance", 2 * want["tol"][slot] / n)
        assert abs(v - float(golden[f"mpjpe_{key}.{i}"])) <= 2 * want["tol"][slot] / n


def test_oracle_slot_is_the_models_oracle_aggregation(lib):
    """mpjpe_error(model.aggregate(mode="oracle")) - two other kernels of this library - against the oracle slot: each side within its
    sum bound of the float64 value."""
    from manipose_amd.metrics import hypothesis_stats, mpjpe_error
    model, _ = _tiny()
    hyp, s, gt = make(2, 5, 27, seed=33, unit=1.0)
    want = reference(hyp, s, gt, 1.0, 1.0)
    h, sc, y = (torch.from_numpy(a).cuda() for a in (hyp, s, gt))
    orac = model.aggregate(h, mode="oracle", ground_truth=y)[1]
    assert orac.cpu().numpy().tobytes() == np.take_along_axis(hyp, want["ko"][:, None, :, None, None], axis=1)[:, 0].tobytes()
    a, b = mpjpe_error(orac, y, "sum").item(), hypothesis_stats(h, sc, y).sums[F_ORACLE].item()
    n = 2 * 27
    other = n * 17 * 8 * U * (np.abs(hyp).max() + 30.0) + (256 * 17 + 3) * U * want["sums"][F_ORACLE]      # mp_mpjpe_sum: partial sums of 256 threads
    print("oracle", a, b, want["sums"][F_ORACLE], "tolerances", other, want["tol"][F_ORACLE])
    assert abs(b - want["sums"][F_ORACLE]) <= want["tol"][F_ORACLE] and abs(a - want["sums"][F_ORACLE]) <= other


def test_accumulator_in_three_pieces_equals_one_call(lib):
    from manipose_amd.metrics import HypothesisAccumulator, hypothesis_stats
    hyp, s, gt = make(5, 5, 27, seed=44)
    want = reference(hyp, s, gt, 1000.0, 1000.0)
    h, sc, y = (torch.from_numpy(a).cuda() for a in (hyp, s, gt))
    whole = hypothesis_stats(h, sc, y, 1000.0, 1000.0)
    acc = HypothesisAccumulator()
    for sl in (slice(0, 2), slice(2, 4), slice(4, 5)):
        acc.add(h[sl], sc[sl], y[sl], pose_scale=1000.0, target_scale=1000.0, consistency=True)
    assert torch.equal(acc.counts, whole.counts) and np.array_equal(acc.counts.cpu().numpy(), want["counts"])
    a, w = acc.sums.cpu().numpy(), whole.sums.double().cpu().numpy()
    assert (np.abs(a - want["sums"]) <= want["tol"]).all() and (np.abs(w - want["sums"]) <= want["tol"]).all()
    acc.all_reduce()                                                          # one process: nothing changes
    r = acc.report()
    N, K = 5 * 27, 5
    assert set(r) == {"mpjpe_weighted_ave", "mpjpe_best_score", "mpjpe_oracle", "mpjpe_jbest", "mpjpe_top_m", "jbest_per_joint", "spread_per_joint",
                      "pairwise_distance", "score_of_oracle", "score_max", "top1_agreement", "oracle_rank_hist", "pbest_head_share",
                      "score_head_share", "jbest_head_share", "score_mass_per_head", "jbest_mpsse", "jbest_mpsce"}
    assert r["mpjpe_oracle"] == a[F_ORACLE] / (N * 17) and r["mpjpe_top_m"] == (a[F_TOPM:F_TOPM + K] / (N * 17)).tolist()
    assert r["mpjpe_top_m"][0] == r["mpjpe_best_score"] and r["mpjpe_top_m"][-1] == r["mpjpe_oracle"] and len(r["jbest_per_joint"]) == 17
    assert r["mpjpe_jbest"] <= r["mpjpe_oracle"] <= r["mpjpe_best_score"] and sorted(r["mpjpe_top_m"], reverse=True) == r["mpjpe_top_m"]
    assert r["top1_agreement"] == want["counts"][C_AGREE] / N and r["oracle_rank_hist"] == (want["counts"][C_ORANK:C_ORANK + K] / N).tolist()
    for key in ("oracle_rank_hist", "pbest_head_share", "score_head_share", "jbest_head_share"):
        assert len(r[key]) == K and abs(sum(r[key]) - 1.0) < 1e-12, key
    assert abs(sum(r["score_mass_per_head"]) - 1.0) < 1e-5                      # normalised float32 scores
    # the J-Best pose through the existing analytics kernel: the same numbers as calling it on the gathered poses
    from manipose_amd.metrics.analytics import AnalyticsAccumulator, pose_analytics
    ref = AnalyticsAccumulator()
    jp = torch.from_numpy(want["jbest_pose"]).cuda()
    for sl in (slice(0, 2), slice(2, 4), slice(4, 5)):
        ref.add(pose_analytics(jp[sl].contiguous(), y[sl].contiguous(), pred_scale=1000.0, gt_scale=1000.0))
    t = ref.report()
    assert r["jbest_mpsse"] == t["mpsse"] and r["jbest_mpsce"] == t["mpsce"] and r["jbest_mpsse"] > 0


# ------------------------------------------------------------------------------ the entry points
def _hpe():
    sys.path.insert(0, os.path.join(ROOT, "hpe"))
    import _entry
    return _entry


def test_evaluate_reports_the_hypotheses_of_the_unflipped_forward(lib):
    """evaluate(hypotheses=True) on rmcl_small (T = 27, K = 5), 5 windows in batches of 2, with flip-TTA on: the new keys are there, equal
    those of an accumulator fed the un-flipped half of the same forward, and the other results do not move."""
    from manipose_amd.metrics import HypothesisAccumulator
    evaluate = _hpe().evaluate
    model, c = _tiny("rmcl_small")
    T, K = c["T"], c["n_hyp"]
    assert (T, K) == (27, 5)
    g = torch.Generator().manual_seed(8)
    X = (0.3 * torch.randn(5, T, 17, 2, generator=g)).clamp(-1, 1).cuda()
    y = 0.3 * torch.randn(5, T, 17, 3, generator=g)
    y[:, :, 0] = 0
    y = y.cuda()
    plain = evaluate(model, X, y, batch=2, tta=True)
    r = evaluate(model, X, y, batch=2, tta=True, hypotheses=True)
    assert "hypotheses" not in plain and {k: v for k, v in r.items() if k != "hypotheses"} == plain
    from manipose_amd.augmentations import pose_flip
    sk = model.decoder.skeleton
    acc, cmax, emax = HypothesisAccumulator(), 0.0, 0.0
    with torch.no_grad():
        for i in range(0, 5, 2):             # evaluate()'s own forward: the flipped copy rides in the same batch; its first half is reported
            xb = X[i:i + 2]
            nb = xb.shape[0]
            poses, scores = model(torch.cat([xb, pose_flip((xb.clone(),), sk)[0]], dim=0))
            acc.add(poses[:nb], scores[:nb], y[i:i + 2], pose_scale=1000.0, target_scale=1000.0, consistency=True)
            cmax = max(cmax, 1000.0 * poses[:nb].abs().max().item(), 1000.0 * y.abs().max().item())
            emax = max(emax, 1000.0 * (poses[:nb] - y[i:i + 2, None]).norm(dim=-1).max().item())
    want = acc.report()
    got = r["hypotheses"]
    assert set(got) == set(want) and len(got["mpjpe_top_m"]) == K
    for k, v in want.items():                     # the same calls on the same bits
        assert got[k] == v, k
    assert got["mpjpe_jbest"] <= got["mpjpe_oracle"] <= got["mpjpe_best_score"]
    # without TTA the three means of evaluate() are these very quantities, from other kernels (mp_aggregate, mp_mpjpe_sum: partial sums of 256
    # terms): each side within its sum bound and the per-term bounds of the module docstring of the float64 value
    r0 = evaluate(model, X, y, batch=2, tta=False, hypotheses=True)
    h0 = r0["hypotheses"]
    term = 8 * U * (cmax + emax) + np.sqrt(3.0) * (K + 2) * U * 1.001 * cmax
    for a, b in ((r0["oracle_mpjpe"], h0["mpjpe_oracle"]), (r0["ps_oracle_mpjpe"], h0["mpjpe_best_score"]), (r0["mpjpe"], h0["mpjpe_weighted_ave"])):
        tol = 2 * term + ((256 + 3) + (FPB * 17 + 3)) * U * b
        print("evaluate", a, "hypotheses", b, "tolerance", tol)
        assert abs(a - b) <= tol
    # a single-hypothesis model has no such table
    from manipose_amd import ManifoldMixSTE, h36m_skeleton
    fx = load_fixture("manifold_k1")
    cm = fx["cfg"]
    m1 = ManifoldMixSTE(h36m_skeleton(), num_frame=cm["T"], embed_dim_rot=cm["C_rot"], depth_rot=cm["depth_rot"], num_heads_rot=cm["heads_rot"],
                        embed_dim_seg=cm["C_seg"], depth_seg=cm["depth_seg"], num_heads_seg=cm["heads_seg"], drop_path_rate=0.0)
    m1.load_state_dict(fixture_state(fx), strict=True)
    g1 = torch.Generator().manual_seed(9)
    X1 = (0.3 * torch.randn(2, cm["T"], 17, 2, generator=g1)).clamp(-1, 1).cuda()
    y1 = (0.3 * torch.randn(2, cm["T"], 17, 3, generator=g1)).cuda()
    assert "hypotheses" not in evaluate(m1.cuda().eval(), X1, y1, batch=2, tta=False, hypotheses=True)


def test_run_hyp_report_writes_the_three_files(lib, tmp_path, monkeypatch):
    """run.test with run.hyp_report=true on the synthetic data path: the three tables beside the report files, with their heads and rows."""
    from manipose_amd import report
    run = _hpe().run
    monkeypatch.chdir(tmp_path)
    run(["run.train=false", "run.test=true", "run.hyp_report=true", "train.batch_size=4", "train.batch_size_test=2", "data.seq_len=27",
         "model.channels=64", "model.layers=2", "model.nheads=4", "model.channels_seg=32", "model.layers_seg=1", "model.nheads_seg=4",
         "multi_hyp.n_hyp=3"])
    d = os.path.join(str(tmp_path), "default")
    K = 3
    joints = report.joints_names()
    heads = {"hyp_report": ["act", *report.HYP_SCALAR_KEYS, *report.HYP_CONSISTENCY_KEYS, "top_1", "top_2", "top_3"],
             "hyp_heads": ["act"] + [f"{t}_{k}" for t in report.HYP_HEAD_TABLES for k in range(K)],
             "hyp_joints": ["act", *joints, *[f"spread {n}" for n in joints]]}
    for name, head in heads.items():
        with open(os.path.join(d, name + ".csv"), newline="") as f:
            rows = list(csv.reader(f))
        assert rows[0] == head, name
        assert [r[0] for r in rows[1:]] == ["synthetic", "average"] and all(len(r) == len(head) for r in rows), name
        vals = np.array([[float(v) for v in r[1:]] for r in rows[1:]])
        assert np.isfinite(vals).all() and np.array_equal(vals[0], vals[1]), name
    assert os.path.exists(os.path.join(d, "protocol_1_err.csv"))

"""mp_bone_extremes (manipose_amd/csrc/bone_extremes.hip) and what is built on it: the reference-named functions
segments_max_strech_per_bone / segments_max_diff_strech_per_bone / coordwise_error, AnalyticsAccumulator.add_extremes, the new keys of
evaluate(analytics=True) and the files run.test writes.

The C ABI is held against a float64 numpy restatement computed from the SAME float32 inputs.  Bounds (derived, not tuned), u = 2^-24:
  * a scaled coordinate carries one rounding, the length a handful more: |len - len64| <= 8 u (max|scaled coordinate| + len);
  * a difference of two lengths: twice that;
  * a coordinate sum: (m + 3) u sum|terms|, m = the number of terms of one block's partial sum (256 frames x 17 joints at most).
The index must EQUAL the float64 arg-max: every case first asserts on the host that the float64 gap between the largest and the
second-largest difference exceeds twice the difference bound for every bone (the data carries planted jumps so that it does)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from helpers import fixture_state, load_fixture

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
PARENTS = (-1, 0, 1, 2, 0, 4, 5, 0, 7, 8, 9, 8, 11, 12, 8, 14, 15)
CHILD = np.arange(1, 17)
PAR = np.array(PARENTS[1:])
SCALE = 1000.0
BLOCK = 256


def subtree(j):
    out = [j]
    for c, p in enumerate(PARENTS):
        if p == j:
            out += subtree(c)
    return out


def plant(x, k, f, amount):
    """Bone k is longer by ``amount`` (input units) from flat frame f on: ONE large difference, between frames f-1 and f."""
    flat = x.reshape(-1, 17, 3)
    d = flat[f:, k + 1] - flat[f:, PARENTS[k + 1]]
    push = amount * d / np.linalg.norm(d, axis=-1, keepdims=True)
    for q in subtree(k + 1):
        flat[f:, q] += push


def make(B, L, seed, plants=None, default=True):
    """(B, L, 17, 3) float32 poses in metres: a base pose, 0.3 mm of per-frame noise, a target 20 mm away; one planted 40 + 3 k mm step
    per bone at a place of its own (when there is a difference to hold it) plus the case's own ``plants`` [(bone, flat frame, metres)]."""
    g = np.random.default_rng(seed)
    x = 0.25 * g.standard_normal((1, 1, 17, 3)) + 0.0003 * g.standard_normal((B, L, 17, 3))
    x[:, :, 0] = 0.0
    y = x + 0.02 * g.standard_normal(x.shape)
    N = B * L
    if default and N > 1:
        for k in range(16):
            plant(x, k, 1 + (7 * k + 3) % (N - 1), 0.040 + 0.003 * k)
    for k, f, a in plants or ():
        plant(x, k, f, a)
    return x.astype(np.float32), y.astype(np.float32)


def lengths64(x32, scale):
    x = np.float64(np.float32(scale)) * x32.astype(np.float64)
    return np.sqrt(((x[..., CHILD, :] - x[..., PAR, :]) ** 2).sum(-1)), np.abs(x).max()


def reference(pred, gt, chain, prev_len=None, frame_base=0, scale=SCALE):
    """float64 restatement: min, max, largest |difference| with its first index and the (largest - second largest) gap, coordinate sums,
    last lengths, and the length bound."""
    B, L = pred.shape[:2]
    ln, cmax = lengths64(pred, scale)                          # (B, L, 16)
    bound = 8 * U * (cmax + ln.max())
    flat = ln.reshape(B * L, 16)
    if chain:
        seq = flat if prev_len is None else np.concatenate([prev_len.astype(np.float64)[None], flat])
        d = np.abs(np.diff(seq, axis=0))
        first = frame_base - (1 if prev_len is not None else 0)  # index of difference 0
    else:
        d = np.abs(np.diff(ln, axis=1)).reshape(-1, 16)
        first = 0
    out = {"min": flat.min(0), "max": flat.max(0), "last": flat[-1], "bound": bound, "n_diff": d.shape[0]}
    if d.shape[0]:
        s = np.sort(d, axis=0)
        out["delta"], out["idx"] = d.max(0), first + d.argmax(0)
        out["gap"] = s[-1] - s[-2] if d.shape[0] > 1 else np.full(16, np.inf)
    if gt is not None:
        e = np.abs(np.float64(np.float32(scale)) * gt.astype(np.float64) - np.float64(np.float32(scale)) * pred.astype(np.float64))
        out["cw"] = e.reshape(-1, 3).sum(0)
    return out


def view(a, layout):
    """Device tensor addressed as (B, L, J, 3): contiguous, or the permuted view of a contiguous (B, 3, J, L) tensor."""
    t = torch.from_numpy(a).cuda()
    return t.contiguous() if layout == "BLJC" else t.permute(0, 3, 2, 1).contiguous().permute(0, 3, 2, 1)


def call(lib, pred, gt=None, chain=0, prev_len=None, frame_base=0, scale=SCALE):
    """mp_bone_extremes through the C ABI on (B, L, J, 3)-shaped device tensors of any strides -> dict of host arrays."""
    from manipose_amd import _lib
    B, L = pred.shape[:2]
    strides = lambda t: (C.c_int64 * 4)(*t.stride())
    f = lambda n: torch.full((n,), float("nan"), device="cuda")
    mn, mx, md, last, cs = f(16), f(16), f(16), f(16), f(3)
    idx = torch.full((16,), -7, dtype=torch.int64, device="cuda")
    scratch = torch.empty(int(lib.mp_bone_extremes_scratch_floats(B * L)), device="cuda")
    _lib.check(lib.mp_bone_extremes(pred.data_ptr(), strides(pred), gt.data_ptr() if gt is not None else None,
                                    strides(gt) if gt is not None else None, B, L, 17, scale, scale, chain,
                                    prev_len.data_ptr() if prev_len is not None else None, frame_base, mn.data_ptr(), mx.data_ptr(),
                                    md.data_ptr(), idx.data_ptr(), cs.data_ptr() if gt is not None else None, last.data_ptr(),
                                    scratch.data_ptr(), scratch.numel(), torch.cuda.current_stream().cuda_stream), "mp_bone_extremes")
    torch.cuda.synchronize()
    return {"min": mn.cpu().numpy(), "max": mx.cpu().numpy(), "delta": md.cpu().numpy(), "idx": idx.cpu().numpy(),
            "last": last.cpu().numpy(), "cw": cs.cpu().numpy()}


def check(got, want, B, L, has_gt):
    b = want["bound"]
    print(f"len bound {b:.3e}  max |min err| {np.abs(got['min'] - want['min']).max():.3e}  max |max err| {np.abs(got['max'] - want['max']).max():.3e}")
    assert np.abs(got["min"] - want["min"]).max() <= b and np.abs(got["max"] - want["max"]).max() <= b
    assert np.abs(got["last"] - want["last"]).max() <= b
    if want["n_diff"] == 0:
        assert (got["idx"] == -1).all() and (got["delta"] == -1).all()
    else:
        print(f"diff bound {2 * b:.3e}  smallest gap {want['gap'].min():.3e}  max |delta err| {np.abs(got['delta'] - want['delta']).max():.3e}")
        assert (want["gap"] > 2 * (2 * b)).all(), "the test data must separate the arg-max from rounding"
        assert np.abs(got["delta"] - want["delta"]).max() <= 2 * b
        assert got["idx"].dtype == np.int64 and (got["idx"] == want["idx"]).all(), (got["idx"], want["idx"])
    if has_gt:
        m = min(B * L, BLOCK) * 17
        tol = (m + 3) * U * want["cw"]
        print(f"coordinate sums {want['cw']}  tol {tol}  err {np.abs(got['cw'] - want['cw'])}")
        assert (np.abs(got["cw"] - want["cw"]) <= tol).all()


@pytest.mark.parametrize("has_gt", [False, True])
@pytest.mark.parametrize("layout", ["BLJC", "BCJL"])
@pytest.mark.parametrize("chain", [0, 1])
@pytest.mark.parametrize("B,L", [(1, 2), (3, 1), (2, 129), (1, 257)])
def test_bone_extremes_against_float64(lib, B, L, chain, layout, has_gt):
    """Smallest shapes at which the kernel can go wrong: one difference; boundary differences only ((3, 1): none at all with chain = 0);
    frames on both sides of the 256-frame block boundary, in one window and in two."""
    pred, gt = make(B, L, seed=B * 1000 + L)
    got = call(lib, view(pred, layout), view(gt, layout) if has_gt else None, chain=chain)
    check(got, reference(pred, gt if has_gt else None, chain), B, L, has_gt)


PLACEMENTS = {                                  # (B, L), the planted largest jump (bone, flat frame, metres), chain
    "inside_a_block": ((1, 257), (5, 77, 0.3), 0),
    "across_the_128_boundary": ((1, 257), (5, 128, 0.3), 0),           # t = 127 -> 128 (a 128-frame block shape would split here)
    "across_the_block_boundary": ((1, 257), (5, 256, 0.3), 0),         # t = 255 -> 256: the frame ahead of block 1 is recomputed
    "across_the_block_boundary_chained": ((2, 129), (5, 256, 0.3), 1),
    "across_a_window_boundary": ((2, 129), (5, 129, 0.3), 1),
}


@pytest.mark.parametrize("case", sorted(PLACEMENTS))
def test_planted_largest_jump_is_found_where_it_is(lib, case):
    (B, L), (k, f, a), chain = PLACEMENTS[case]
    pred, gt = make(B, L, seed=77, plants=[(k, f, a)])
    got = call(lib, view(pred, "BLJC"), None, chain=chain)
    want = reference(pred, None, chain)
    check(got, want, B, L, False)
    assert got["idx"][k] == (f - 1 if chain else (f // L) * (L - 1) + f % L - 1) and abs(got["delta"][k] - SCALE * a) < 5.0      # (the step plus a millimetre of pose noise)
    if case == "across_a_window_boundary":      # the same data without the chain: the window boundary is no difference, the next-largest wins
        got0, want0 = call(lib, view(pred, "BCJL"), None, chain=0), reference(pred, None, 0)
        check(got0, want0, B, L, False)
        assert got0["idx"][k] == want0["idx"][k] != want["idx"][k] and got0["delta"][k] < 0.5 * got["delta"][k]


def test_largest_jump_against_prev_len_and_one_frame_without(lib):
    pred, _ = make(2, 9, seed=5)
    ln, _ = lengths64(pred, SCALE)
    prev = (ln[0, 0] - 100.0).astype(np.float32)               # every bone 100 mm shorter ahead of frame 0
    got = call(lib, view(pred, "BLJC"), None, chain=1, prev_len=torch.from_numpy(prev).cuda(), frame_base=1000)
    want = reference(pred, None, 1, prev_len=prev, frame_base=1000)
    check(got, want, 2, 9, False)
    assert (got["idx"] == 999).all()                            # the difference between frames f-1 and f has index frame_base + f - 1
    got0 = call(lib, view(pred, "BLJC"), None, chain=0, prev_len=torch.from_numpy(prev).cuda(), frame_base=1000)
    check(got0, reference(pred, None, 0), 2, 9, False)          # prev_len belongs to the chain only
    one, _ = make(1, 1, seed=6)
    g1 = call(lib, view(one, "BLJC"), None, chain=1)
    assert (g1["idx"] == -1).all() and (g1["delta"] == -1).all() and (g1["min"] == g1["max"]).all() and (g1["min"] == g1["last"]).all()
    g2 = call(lib, view(one, "BLJC"), None, chain=1, prev_len=torch.from_numpy(prev).cuda(), frame_base=3)
    assert (g2["idx"] == 2).all() and (g2["delta"] > 0).all()


def test_carry_over_two_calls_gives_the_bytes_of_one_call(lib):
    """(4, 9) as two calls of (2, 9) with prev_len / last_len / frame_base against one chained call; bone 3's largest jump sits exactly
    between the two pieces, where only prev_len can see it."""
    pred, gt = make(4, 9, seed=9, plants=[(3, 18, 0.2)])
    whole = call(lib, view(pred, "BLJC"), view(gt, "BLJC"), chain=1)
    check(whole, reference(pred, gt, 1), 4, 9, True)
    a = call(lib, view(pred[:2], "BLJC"), view(gt[:2], "BLJC"), chain=1)
    b = call(lib, view(pred[2:], "BLJC"), view(gt[2:], "BLJC"), chain=1, prev_len=torch.from_numpy(a["last"]).cuda(), frame_base=18)
    newer = b["delta"] > a["delta"]                             # strictly larger: the earlier index keeps a tie
    merged = {"min": np.minimum(a["min"], b["min"]), "max": np.maximum(a["max"], b["max"]), "delta": np.where(newer, b["delta"], a["delta"]),
              "idx": np.where(newer, b["idx"], a["idx"]), "last": b["last"]}
    for key, v in merged.items():
        assert v.tobytes() == whole[key].tobytes(), key
    assert whole["idx"][3] == 17
    cw = a["cw"].astype(np.float64) + b["cw"].astype(np.float64)      # two partial sums rounded apart: within the bound, not the same bytes
    assert (np.abs(cw - whole["cw"]) <= (36 * 17 + 3) * U * cw).all()


def test_ties_go_to_the_first_index_and_runs_are_bit_identical(lib):
    """A constant pose P with another pose Q at frames 10, 20 (same wave), 200 (another wave), 280 (another block): the eight differences
    |len Q - len P| are bit-identical; index 9 must win for every bone."""
    g = np.random.default_rng(3)
    P, Q = (0.25 * g.standard_normal((2, 17, 3))).astype(np.float32)
    x = np.repeat(P[None], 300, axis=0)
    x[[10, 20, 200, 280]] = Q
    x = x[None]                                                  # (1, 300, 17, 3)
    for chain, layout in ((0, "BLJC"), (1, "BCJL")):
        got = call(lib, view(x, layout), None, chain=chain)
        want = reference(x, None, chain)
        assert (got["idx"] == 9).all() and np.abs(got["delta"] - want["delta"]).max() <= 2 * want["bound"]
    pred, gt = make(2, 129, seed=11)
    r1 = call(lib, view(pred, "BCJL"), view(gt, "BCJL"), chain=1)
    r2 = call(lib, view(pred, "BCJL"), view(gt, "BCJL"), chain=1)
    for key in r1:
        assert r1[key].tobytes() == r2[key].tobytes(), key


def test_bad_arguments_are_refused(lib):
    from manipose_amd.metrics import coordwise_error, segments_max_diff_strech_per_bone, segments_max_strech_per_bone
    x = torch.zeros(2, 5, 17, 3, device="cuda")
    st = (C.c_int64 * 4)(*x.stride())
    o = torch.zeros(16, device="cuda")
    oi = torch.zeros(16, dtype=torch.int64, device="cuda")
    sc = torch.zeros(int(lib.mp_bone_extremes_scratch_floats(10)), device="cuda")
    args = lambda J, nsc: (x.data_ptr(), st, None, None, 2, 5, J, 1.0, 1.0, 0, None, 0, o.data_ptr(), o.data_ptr(), o.data_ptr(), oi.data_ptr(),
                           None, o.data_ptr(), sc.data_ptr(), nsc, None)
    assert lib.mp_bone_extremes(*args(16, sc.numel())) != 0 and b"17-joint" in lib.mp_last_error()
    assert lib.mp_bone_extremes(*args(17, sc.numel() - 1)) != 0 and b"scratch" in lib.mp_last_error()
    assert lib.mp_bone_extremes(*args(17, sc.numel())) == 0
    cpu = torch.zeros(2, 3, 17, 5)
    for fn in (lambda: segments_max_strech_per_bone(cpu, None), lambda: segments_max_diff_strech_per_bone(cpu, None),
               lambda: coordwise_error(cpu, cpu, "average"), lambda: coordwise_error(cpu, cpu, "no_agg")):
        with pytest.raises(RuntimeError):
            fn()                                                 # no CPU fallback
    with pytest.raises(IndexError):                              # the reference's torch.max over an empty dimension
        segments_max_diff_strech_per_bone(torch.zeros(2, 3, 17, 1, device="cuda"), None)
    with pytest.raises(ValueError):
        coordwise_error(x, x, "median")


# ------------------------------------------------------------------------------ the reference's functions, tests/golden/report.npz
@pytest.fixture(scope="module")
def golden():
    return load_fixture("report")


@pytest.mark.parametrize("i", [0, 1])
def test_reference_named_functions_match_the_reference(lib, golden, i):
    """Both sides are float32 here: twice the length bound (four times for a difference); indices must be equal."""
    from manipose_amd import h36m_skeleton
    from manipose_amd.metrics import coordwise_error, segments_max_diff_strech_per_bone, segments_max_strech_per_bone
    sk = h36m_skeleton()
    pred, gt = golden[f"pred.{i}"], golden[f"gt.{i}"]
    B, L = pred.shape[:2]
    ln, cmax = lengths64(pred, 1.0)
    b = 2 * 8 * U * (cmax + ln.max())
    p, y = torch.from_numpy(pred).cuda(), torch.from_numpy(gt).cuda()
    gen = p.permute(0, 3, 2, 1)                                               # (B, 3, J, L), no copy
    flat = gen.permute(1, 2, 0, 3).reshape(1, 3, 17, -1)
    for tag, x in (("win", gen), ("seq", flat)):
        mn, mx = segments_max_strech_per_bone(joints_coords=x, skeleton=sk)
        dv, di = segments_max_diff_strech_per_bone(joints_coords=x, skeleton=sk)
        err = [np.abs(a.cpu().numpy() - golden[f"{k}.{tag}.{i}"]).max() for a, k in ((mn, "min_len"), (mx, "max_len"), (dv, "max_delta"))]
        print(tag, "bound", b, "errors", err)
        assert err[0] <= b and err[1] <= b and err[2] <= 2 * b
        assert di.dtype == torch.int64 and (di.cpu().numpy() == golden[f"max_delta_idx.{tag}.{i}"]).all()
    # coordinate errors: both sides add B L 17 float32 terms; (m + 3) u relative for each side
    rel = 2 * (min(B * L, BLOCK) * 17 + 3) * U
    for mode, key in (("average", "cw_err"), ("sum", "cw_sum")):
        got = coordwise_error(p, y, mode).cpu().numpy()
        assert got.shape == (3,) and (np.abs(got - golden[f"{key}.{i}"]) <= rel * golden[f"{key}.{i}"]).all(), (mode, got)
    assert torch.equal(coordwise_error(p, y, "no_agg"), (y - p).abs().reshape(-1, 3))


def test_accumulator_reports_the_reference_quantities(lib, golden):
    """AnalyticsAccumulator fed the (2, 130) set in two pieces: mvjpe, cw_err, jw_err_var and the chained extremes against the reference's
    values on the flattened sequence.  The sums behind them add at most 256 x 17 float32 terms per block: (m + 3) u relative, both sides."""
    from manipose_amd.metrics.analytics import AnalyticsAccumulator, pose_analytics
    pred, gt = golden["pred.1"], golden["gt.1"]
    p, y = torch.from_numpy(pred).cuda(), torch.from_numpy(gt).cuda()
    acc = AnalyticsAccumulator()
    for s in (slice(0, 1), slice(1, 2)):
        acc.add(pose_analytics(p[s].contiguous(), y[s].contiguous()))
        acc.add_extremes(p[s].contiguous(), y[s].contiguous())
    r = acc.report()
    rel = 2 * (BLOCK * 17 + 3) * U
    ln, cmax = lengths64(pred, 1.0)
    b = 2 * 8 * U * (cmax + ln.max())
    assert abs(r["mvjpe"] - golden["mvjpe.1"]) <= rel * golden["mvjpe.1"]
    assert (np.abs(np.array(r["cw_err"]) - golden["cw_err.1"]) <= rel * golden["cw_err.1"]).all()
    want_var = golden["jw_mse.1"].astype(np.float64) - golden["jw_err.1"].astype(np.float64) ** 2
    assert (np.abs(np.array(r["jw_err_var"]) - want_var) <= rel * (golden["jw_mse.1"] + golden["jw_err.1"] ** 2)).all()
    assert np.abs(np.array(r["seg_min_len"]) - golden["min_len.seq.1"]).max() <= b
    assert np.abs(np.array(r["seg_max_len"]) - golden["max_len.seq.1"]).max() <= b
    assert np.abs(np.array(r["seg_max_strech"]) - (golden["max_len.seq.1"] - golden["min_len.seq.1"])).max() <= 2 * b
    assert np.abs(np.array(r["seg_max_delta_strech"]) - golden["max_delta.seq.1"]).max() <= 2 * b
    assert r["seg_max_delta_idx"] == golden["max_delta_idx.seq.1"].tolist()


# ------------------------------------------------------------------------------ the entry points
def _hpe():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "hpe"))
    import _entry
    return _entry


def _tiny():
    from manipose_amd import RMCLManifoldMixSTE, h36m_skeleton
    fx = load_fixture("rmcl_tiny")
    c = fx["cfg"]
    m = RMCLManifoldMixSTE(h36m_skeleton(), num_frame=c["T"], embed_dim_rot=c["C_rot"], depth_rot=c["depth_rot"], num_heads_rot=c["heads_rot"],
                           embed_dim_seg=c["C_seg"], depth_seg=c["depth_seg"], num_heads_seg=c["heads_seg"], n_hyp=c["n_hyp"], drop_path_rate=0.0)
    m.load_state_dict(fixture_state(fx), strict=True)
    return m.cuda().eval(), c["T"]


def test_evaluate_reports_the_extremes_of_the_concatenated_predictions(lib):
    """evaluate(analytics=True) on rmcl_tiny, 5 windows in batches of 2 (2 + 2 + 1): the new keys against numpy on the concatenated
    aggregated predictions in millimetres, flattened to ONE sequence as main_h36m_lifting.py:934-1089 does."""
    evaluate = _hpe().evaluate
    model, T = _tiny()
    g = torch.Generator().manual_seed(8)
    X = (0.3 * torch.randn(5, T, 17, 2, generator=g)).clamp(-1, 1).cuda()
    y = 0.3 * torch.randn(5, T, 17, 3, generator=g)
    y[:, :, 0] = 0
    y = y.cuda()
    r = evaluate(model, X, y, batch=2, tta=False, analytics=True, seg_err_samples=50)
    got = r["analytics"]
    with torch.no_grad():
        preds = []
        for i in range(0, 5, 2):
            poses, scores = model(X[i:i + 2])
            preds.append(model.aggregate(poses, scores, "weighted_ave"))
    pred = torch.cat(preds).cpu().numpy()                                      # metres, float32: the kernel scales by 1000 itself
    gt = y.cpu().numpy()
    want = reference(pred.reshape(1, -1, 17, 3), gt.reshape(1, -1, 17, 3), chain=1)
    b = want["bound"]
    assert np.abs(np.array(got["seg_min_len"]) - want["min"]).max() <= b and np.abs(np.array(got["seg_max_len"]) - want["max"]).max() <= b
    assert np.abs(np.array(got["seg_max_strech"]) - (want["max"] - want["min"])).max() <= 2 * b
    assert np.abs(np.array(got["seg_max_delta_strech"]) - want["delta"]).max() <= 2 * b
    ln, _ = lengths64(pred.reshape(-1, 17, 3), SCALE)
    d = np.abs(np.diff(ln, axis=0))
    for k, i in enumerate(got["seg_max_delta_idx"]):        # an untrained model plants nothing: the index must name a difference that IS the
        assert 0 <= i < d.shape[0] and d[i, k] >= want["delta"][k] - 4 * b      # largest up to rounding, and the arg-max itself where the gap allows
        if want["gap"][k] > 4 * b:
            assert i == want["idx"][k]
    n = pred.shape[0] * T * 17
    rel = (min(2 * T, BLOCK) * 17 + 3) * U
    cw = want["cw"] / n
    assert (np.abs(np.array(got["cw_err"]) - cw) <= rel * cw).all()
    p64, g64 = SCALE * pred.astype(np.float64), SCALE * gt.astype(np.float64)
    v = np.linalg.norm(np.diff(p64, axis=1) - np.diff(g64, axis=1), axis=-1)
    # a velocity term is a difference of differences of four scaled coordinates of size <= c: 4 c u from their roundings and up to 3 c u
    # from the subtractions in each of its three components, sqrt(3) of that in the norm: below 16 c u
    c = max(np.abs(p64).max(), np.abs(g64).max())
    assert abs(got["mvjpe"] - v.mean()) <= rel * v.mean() + 16 * c * U
    e = np.linalg.norm(p64 - g64, axis=-1).reshape(-1, 17)
    var = (e ** 2).mean(0) - e.mean(0) ** 2
    assert (np.abs(np.array(got["jw_err_var"]) - var) <= 2 * rel * ((e ** 2).mean(0) + e.mean(0) ** 2)).all()
    assert r["seg_errs"].shape == (50, 16) and np.isfinite(r["seg_errs"]).all()


def test_run_test_writes_the_report_files(lib, golden, tmp_path, monkeypatch):
    """run.test on the synthetic data path: every file of the reference's H36M test pass, with its head and row labels."""
    run = _hpe().run
    monkeypatch.chdir(tmp_path)
    run(["run.train=false", "run.test=true", "train.batch_size=4", "train.batch_size_test=2", "data.seq_len=27", "model.channels=64",
         "model.layers=2", "model.nheads=4", "model.channels_seg=32", "model.layers_seg=1", "model.nheads_seg=4", "multi_hyp.n_hyp=3"])
    d = os.path.join(str(tmp_path), "default")
    bones, joints = ["act", *golden["bones_names"].tolist()], ["act", *golden["joints_names"].tolist()]
    heads = {"protocol_1_err": ["act", "mpjpe", "sag sym", "seg std", "p-mpjpe", "mvjpe", "mse", "err var", "seg err", "oracle mpjpe",
                                "pseudo oracle mpjpe"],
             "seg_symmetry": bones, "seg_consistency": bones, "seg_max_strech": bones, "seg_max_delta_strech": bones,
             "cw_err": ["act", "x", "y", "z"], "jw_err": joints}
    import csv
    for name, head in heads.items():
        with open(os.path.join(d, name + ".csv"), newline="") as f:
            rows = list(csv.reader(f))
        assert rows[0] == head, name
        assert [r[0] for r in rows[1:]] == ["synthetic", "average"] and all(len(r) == len(head) for r in rows), name
        vals = np.array([[float(v) for v in r[1:]] for r in rows[1:]])
        assert np.isfinite(vals).all() and np.array_equal(vals[0], vals[1]), name       # one group: the average row repeats it
    assert np.load(os.path.join(d, "all_jw_err_var.npy")).shape == (1, 17)
    assert np.load(os.path.join(d, "all_seg_errs.npy")).shape == (1000, 16)

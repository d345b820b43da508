"""Lifting along one hypothesis path on the device: mp_lift_path against the float64 statement (lift_path_ref.py), a sequence longer than two of
the backtrack's chunks, the exact rules (ties, sigma = inf, NaN inputs), independence of the sequences, argument errors, select_path,
lift_sequences(agg="path") and run.lift.

What is compared and why.  The PATH must equal the statement's exactly: test_lift_path_host.py asserts for every input of GPU_CASES that no
alternative path comes within 1e-8 max(1, optimum) of the optimum, and the kernel's fp64 arithmetic differs from numpy's on the same float32 inputs
by rounding only - about N (3 J + 8) 2^-53 relative (the sum of 3 J squares, the scaling, the log, and two additions per frame), 4e-12 at N = 300,
more than 1000 times below that floor.  The COST is held to |cost - optimum| <= 1e-10 max(1, optimum), the same estimate with about 25 times
headroom.  Neither bound is measured from the kernel.  `out` is a copy: bit for bit."""
import os
import re
import sys

import numpy as np
import pytest
import torch

import lift_path_ref as ref
from lift_fixtures import fixture_model as _model, same as _same, sequences_2d as _sequences

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _call(lib, hyps, off, sigma, switch, want_out=True, want_cost=True):
    """mp_lift_path itself on host arrays: (path, out, cost, the input as the device holds it afterwards)"""
    from manipose_amd import _lib
    ntot, K, J, _ = hyps.shape
    d_h = _dev(hyps)
    d_off = off if torch.is_tensor(off) else _dev(np.asarray(off, np.int64))
    S = int(d_off.numel()) - 1
    path = torch.full((ntot,), 99, dtype=torch.uint8, device="cuda")
    out = torch.full((ntot, J, 3), -7.0, device="cuda") if want_out else None
    cost = torch.full((S,), -7.0, dtype=torch.float64, device="cuda") if want_cost else None
    n = int(lib.mp_lift_path_scratch_floats(ntot, K))
    assert n == (ntot * (8 * K * K + 9 * K) + 3) // 4
    scratch = torch.empty(n, dtype=torch.float32, device="cuda")
    _lib.check(lib.mp_lift_path(_lib.ptr(d_h), ntot, K, J, _lib.ptr(d_off), S, float(sigma), float(switch), _lib.ptr(path), _lib.ptr(out), _lib.ptr(cost),
                                _lib.ptr(scratch), n, None), "mp_lift_path")
    torch.cuda.synchronize()
    return path.cpu().numpy(), out.cpu().numpy() if want_out else None, cost.cpu().numpy() if want_cost else None, d_h.cpu().numpy()


def _cost_ok(got, want):
    return bool((np.abs(got - want) <= 1e-10 * np.maximum(1.0, np.abs(want))).all())


def _check(lib, hyps, off, sigma, switch, tag):
    want_path, want_out, want_cost, margin, covered = ref.select_all(hyps, off, sigma, switch)
    path, out, cost, after = _call(lib, hyps, off, sigma, switch)
    worst = float((np.abs(cost - want_cost) / np.maximum(1.0, np.abs(want_cost))).max())
    print(f"\n[path {tag}] {int((path != want_path).sum())} of {len(path)} frames differ from the statement; worst cost error {worst:.2e} (bound 1e-10); "
          f"smallest relative margin {float((margin / np.maximum(1.0, np.abs(want_cost))).min()):.2e}")
    assert covered.all()
    assert np.array_equal(path, want_path)
    assert _cost_ok(cost, want_cost)
    assert _same(out, want_out) and _same(out, hyps[np.arange(len(hyps)), path][:, :, :3])
    assert _same(after, hyps)                                             # the input is unmodified
    return path, out, cost


@pytest.mark.parametrize("case", ref.GPU_CASES, ids=ref.case_id)
def test_against_fp64(lib, case):
    lens, K, J, sigma, switch, _ = case
    hyps, off = ref.case_inputs(case)
    path, out, cost = _check(lib, hyps, off, sigma, switch, ref.case_id(case))
    again = _call(lib, hyps, torch.from_numpy(off).cuda(), sigma, switch)
    assert _same(again[0], path) and _same(again[1], out) and _same(again[2], cost)      # two calls, a device table: identical bits


def test_long_sequence_crosses_the_chunks(lib):
    from manipose_amd import _lib
    chunk = int(re.search(r"#define MP_LIFT_PATH_CHUNK (\d+)", open(_lib.HEADER_PATH).read()).group(1))
    n = 2 * chunk + 3
    hyps, off = ref.path_inputs([n], 8, 4, 11)
    margin = ref.select_all(hyps, off, 0.02, 0.1)[3]
    assert margin[0] >= 1e-8 * max(1.0, ref.select_all(hyps, off, 0.02, 0.1)[2][0])
    path, _, _ = _check(lib, hyps, off, 0.02, 0.1, f"long N={n} K=8")
    assert ref.switches(path, [(0, n)])[0] >= 3                          # a path that says something in every chunk
    assert all(len(set(path[a:b].tolist())) > 1 for a, b in ((0, chunk), (chunk, 2 * chunk)))


def test_exact_rules(lib):
    g = np.random.default_rng(21)
    # all hypotheses identical with equal scores: zeros, with and without a switch cost
    hyps, off = ref.path_inputs([40, 1, 9], 5, 17, 22)
    same = np.ascontiguousarray(np.repeat(hyps[:, :1], 5, axis=1))
    for switch in (0.0, 0.7):
        path, out, _, _ = _call(lib, same, off, 0.02, switch)
        assert not path.any() and _same(out, same[:, 0, :, :3])
    # sigma = inf, no switch cost: the first arg-max of the float32 score per frame, exact ties included
    scores = g.choice(np.array([0.125, 0.25, 0.5, 0.0625], np.float32), size=(50, 5))
    hyps[:, :, :, 3] = scores[:, :, None]
    want = ref.best_score(hyps)
    assert ((scores == scores.max(axis=1, keepdims=True)).sum(axis=1) > 1).sum() >= 10       # many frames hold a tie for the best score
    path, out, cost, _ = _call(lib, hyps, off, np.inf, 0.0)
    assert np.array_equal(path, want) and np.array_equal(path, ref.select_all(hyps, off, np.inf, 0.0)[0])
    assert _cost_ok(cost, ref.select_all(hyps, off, np.inf, 0.0)[2])
    # a NaN coordinate in one hypothesis of a frame, and (separately) a NaN score, are never chosen; everything else is finite
    hyps, off = ref.path_inputs([60, 25], 3, 17, 23)
    bad_xyz = [(5, 0), (30, 2), (59, 1), (60, 1), (84, 0)]
    bad_score = [(0, 2), (17, 1), (70, 0)]
    for f, k in bad_xyz:
        hyps[f, k, 3, 1] = np.nan
    for f, k in bad_score:
        hyps[f, k, :, 3] = np.nan
    want = ref.select_all(hyps, off, 0.02, 0.0)
    assert (want[3] >= 1e-8 * np.maximum(1.0, np.abs(want[2]))).all()
    path, out, cost, _ = _call(lib, hyps, off, 0.02, 0.0)
    assert np.array_equal(path, want[0]) and _cost_ok(cost, want[2]) and _same(out, want[1])
    assert all(path[f] != k for f, k in bad_xyz + bad_score) and np.isfinite(out).all() and np.isfinite(cost).all() and (cost < 1e29).all()


def test_sequences_are_independent(lib):
    hyps, off = ref.path_inputs([30, 1, 44, 20], 5, 17, 31)
    path, out, cost, _ = _call(lib, hyps, off, 0.02, 0.2)
    # sequence s + 1 changes: the sequences before it keep their bits
    other = hyps.copy()
    other[off[2]:, :, :, :3] = other[off[2]:, ::-1, :, :3] * np.float32(1.5)
    other[off[2]:, :, :, 3] = other[off[2]:, ::-1, :, 3]
    p2, o2, c2, _ = _call(lib, other, off, 0.02, 0.2)
    assert _same(p2[:off[2]], path[:off[2]]) and _same(o2[:off[2]], out[:off[2]]) and _same(c2[:2], cost[:2]) and not _same(o2[off[2]:], out[off[2]:])
    # one sequence alone gives the bits it has in the call of four
    p1, o1, c1, _ = _call(lib, np.ascontiguousarray(hyps[off[2]:off[3]]), [0, 44], 0.02, 0.2)
    assert _same(p1, path[off[2]:off[3]]) and _same(o1, out[off[2]:off[3]]) and _same(c1, cost[2:3])
    # a device table with entries outside 0 .. Ntot behaves as its clamped form
    wild = torch.tensor([-5, 30, 31, 75, 10 ** 12], dtype=torch.int64).cuda()
    pw, ow, cw, _ = _call(lib, hyps, wild, 0.02, 0.2)
    assert _same(pw, path) and _same(ow, out) and _same(cw, cost)
    # an empty range costs 0 and writes nothing; frames that no sequence holds are not written
    pe, oe, ce, _ = _call(lib, hyps, [0, 30, 30, 31, 75], 0.02, 0.2)
    assert ce[1] == 0.0 and _same(pe[:75], path[:75]) and _same(oe[:75], out[:75]) and (pe[75:] == 99).all() and (oe[75:] == -7.0).all()
    pp, op, cp, _ = _call(lib, hyps, [31, 75], 0.02, 0.2)
    assert (pp[:31] == 99).all() and (op[:31] == -7.0).all() and _same(pp[31:75], path[31:75]) and _same(op[31:75], out[31:75]) and _same(cp, cost[2:3])
    # out and cost may be null
    pn, on, cn, _ = _call(lib, hyps, off, 0.02, 0.2, want_out=False, want_cost=False)
    assert on is None and cn is None and _same(pn, path)


def test_entry_point_rejects_bad_arguments_before_any_launch(lib):
    ntot, K, J = 8, 3, 17
    hyps = torch.rand(ntot, K, J, 4, device="cuda") + 0.1
    off = torch.tensor([0, 8], dtype=torch.int64, device="cuda")
    path = torch.full((ntot,), 99, dtype=torch.uint8, device="cuda")
    out = torch.full((ntot, J, 3), -1.0, device="cuda")
    cost = torch.full((1,), -1.0, dtype=torch.float64, device="cuda")
    n = int(lib.mp_lift_path_scratch_floats(ntot, 8))
    scratch = torch.full((n + 2,), -1.0, device="cuda")
    p = lambda t: None if t is None else t.data_ptr()

    def call(src=hyps, offs=off, dst=path, scr=scratch, Ntot=ntot, K=K, J=J, S=1, sigma=0.02, switch=0.0, floats=n):
        return lib.mp_lift_path(p(src), Ntot, K, J, p(offs), S, sigma, switch, p(dst), p(out), p(cost), scr if isinstance(scr, int) else p(scr), floats, None)
    bad = [(dict(src=None), "null"), (dict(dst=None), "null"), (dict(offs=None), "null"), (dict(scr=None), "null"),
           (dict(K=0), "K="), (dict(K=9), "K="), (dict(K=-1), "K="), (dict(J=1), "J="), (dict(J=33), "J="),
           (dict(Ntot=0), "Ntot="), (dict(Ntot=-4), "Ntot="), (dict(S=0), "S="), (dict(S=-1), "S="), (dict(S=9), "S="),
           (dict(sigma=0.0), "sigma"), (dict(sigma=-0.02), "sigma"), (dict(sigma=float("nan")), "sigma"),
           (dict(switch=-0.5), "switch_cost"), (dict(switch=float("inf")), "switch_cost"), (dict(switch=float("nan")), "switch_cost"),
           (dict(floats=int(lib.mp_lift_path_scratch_floats(ntot, K)) - 1), "scratch"), (dict(floats=0), "scratch"),
           (dict(scr=scratch.data_ptr() + 4), "scratch"), (dict(Ntot=2 ** 62), "too many")]
    for kw, word in bad:
        assert call(**kw) == 1 and word in lib.mp_last_error().decode(), (kw, lib.mp_last_error())
    torch.cuda.synchronize()
    assert bool((path == 99).all()) and bool((out == -1).all()) and bool((cost == -1).all()) and bool((scratch == -1).all())      # nothing ran
    assert call() == 0 and call(sigma=float("inf")) == 0                 # the same call with good arguments; sigma = inf is allowed
    torch.cuda.synchronize()
    assert bool((path < K).all()) and bool((out != -1).all()) and bool(torch.isfinite(cost).all())


def test_select_path_public_function(lib):
    from manipose_amd import select_path
    hyps, off = ref.path_inputs([25, 1, 40], 5, 17, 41)
    want = ref.select_all(hyps, off, 0.05, 0.3)
    t = _dev(hyps)
    for table in (off, torch.from_numpy(off).cuda()):
        poses, path, cost = select_path(t, table, sigma=0.05, switch_cost=0.3)
        assert poses.shape == (66, 17, 3) and poses.dtype == torch.float32 and path.shape == (66,) and path.dtype == torch.uint8
        assert cost.shape == (3,) and cost.dtype == torch.float64 and poses.is_cuda and path.is_cuda and cost.is_cuda
        assert np.array_equal(path.cpu().numpy(), want[0]) and _same(poses.cpu().numpy(), want[1]) and _cost_ok(cost.cpu().numpy(), want[2])
        assert _same(t.cpu().numpy(), hyps)
    one = select_path(t)                                                  # one sequence, the default sigma, no switch cost
    w1 = ref.select_all(hyps, None, 0.02, 0.0)
    assert one[2].shape == (1,) and np.array_equal(one[1].cpu().numpy(), w1[0]) and _cost_ok(one[2].cpu().numpy(), w1[2])
    with pytest.raises(RuntimeError, match="S=70"):                       # more sequences than frames: the C entry point's refusal
        select_path(t, np.zeros(71, np.int64))


# ---- end to end: the tiny fp32 fixture models of lift_fixtures.py ------------------------------------------------------------------------------
def test_lift_sequences_with_a_path(lib):
    from manipose_amd import lift_sequences, project_rigid, select_path, smooth_poses
    model, T, K = _model("rmcl")
    p2 = _sequences(T)
    lens = [len(s) for s in p2]
    kw = dict(stride=T // 2 + 1, tta=False, batch=2)
    print()
    for sigma, switch in ((2.0, 0.0), (0.05, 0.2)):                       # steps that cost next to nothing (the scores decide), and steps that count
        poses, hyps, chosen = lift_sequences(model, p2, agg="path", path_sigma=sigma, path_switch=switch, return_hyps=True, return_path=True, **kw)
        assert len(poses) == len(hyps) == len(chosen) == 3 and K >= 2
        for s in range(3):
            path, cost = chosen[s]
            assert path.shape == (lens[s],) and path.dtype == torch.uint8 and cost.shape == () and cost.dtype == torch.float64
            h = hyps[s].cpu().numpy()
            assert hyps[s].shape == (lens[s], K, 17, 4) and _same(poses[s].cpu().numpy(), h[np.arange(lens[s]), path.cpu().numpy()][:, :, :3])
            sp, spath, scost = select_path(hyps[s].contiguous(), sigma=sigma, switch_cost=switch)
            assert torch.equal(spath, path) and torch.equal(scost[0], cost) and torch.equal(sp, poses[s])
            print(f"[lift_sequences agg=path sigma={sigma} switch={switch}, sequence {s}] {ref.switches(path.cpu().numpy(), [(0, lens[s])])[0]} switches in {lens[s]} frames, cost {float(cost):.4f}")
    # the hypotheses are those of the other aggregations (the merge is the same), and without return_hyps / return_path only the poses come back
    base = lift_sequences(model, p2, return_hyps=True, **kw)
    assert all(torch.equal(a, b) for a, b in zip(hyps, base[1]))
    bare = lift_sequences(model, p2, agg="path", path_sigma=sigma, path_switch=switch, **kw)
    assert isinstance(bare, list) and all(torch.equal(a, b) for a, b in zip(bare, poses))
    # path_sigma is in metres: scale multiplies poses and sigma alike, and the path stays
    scaled = lift_sequences(model, p2, agg="path", path_sigma=sigma, path_switch=switch, return_hyps=True, return_path=True, scale=1000.0, **kw)
    for s in range(3):
        sp, spath, scost = select_path(scaled[1][s].contiguous(), sigma=sigma * 1000.0, switch_cost=switch)
        assert torch.equal(spath, scaled[2][s][0]) and torch.equal(scost[0], scaled[2][s][1]) and torch.equal(sp, scaled[0][s])
    # the stage order: path -> smooth poses -> rigid, by hand on the selected poses
    res = lift_sequences(model, p2, agg="path", path_sigma=sigma, path_switch=switch, rigid=True, lengths="measured", smooth_poses=2, return_bones=True,
                         return_hyps=True, **kw)
    for s in range(3):
        want = project_rigid(smooth_poses(poses[s].clone(), radius=2), res[2][s])
        assert torch.equal(res[0][s], want) and not torch.equal(res[0][s], poses[s])
        assert torch.equal(res[1][s], project_rigid(smooth_poses(hyps[s].clone(), radius=2), res[2][s]))
    # a model of one hypothesis has no path
    single, T1, _ = _model("manifold")
    with pytest.raises(ValueError, match="this model has 1"):
        lift_sequences(single, _sequences(T1), agg="path", tta=False)
    # the default aggregation: not a bit changes when the path's defaults are spelled out
    for tta in (False, True):
        a = lift_sequences(model, p2, stride=T // 2 + 1, tta=tta, batch=2, return_hyps=True)
        b = lift_sequences(model, p2, stride=T // 2 + 1, tta=tta, batch=2, return_hyps=True, agg="weighted_ave", path_sigma=0.02, path_switch=0.0,
                           return_path=False)
        assert all(torch.equal(x, y) for r, q in zip(a, b) for x, y in zip(r, q))
    assert all(torch.equal(x, y) for x, y in zip(a[0], lift_sequences(model, p2, stride=T // 2 + 1, tta=True, batch=2)))


def test_path_lift_entry_point(lib, tmp_path, monkeypatch):
    sys.path.insert(0, os.path.join(ROOT, "hpe"))
    from _entry import LIFT_SUFFIXES, run
    monkeypatch.chdir(tmp_path)
    run(["run.train=false", "run.test=false", "run.lift=true", "lift.stride=14", "train.batch_size_test=4", "data.seq_len=27", "model.channels=64",
         "model.layers=2", "model.nheads=4", "model.channels_seg=32", "model.layers_seg=1", "model.nheads_seg=4", "multi_hyp.n_hyp=3",
         "data.synthetic_sequences=3", "model.precision=fp32", "lift.hyps=true", "lift.agg=path", "train.tta=false", "lift.path_sigma=0.05",
         "lift.path_switch=0.1"])
    z = np.load(os.path.join(str(tmp_path), "default", "lift.npz"))
    keys = [f"synthetic_{i:03d}" for i in range(3)]
    assert sorted(z.files) == sorted(k + s for k in keys for s in ("", "__hyps", "__path", "__path_cost"))
    assert all(f == k or f[len(k):] in LIFT_SUFFIXES for f in z.files for k in keys if f.startswith(k))
    for i, k in enumerate(keys):
        n = 27 * 4 + 37 * i + 11
        path, h = z[k + "__path"], z[k + "__hyps"]
        assert path.shape == (n,) and path.dtype == np.uint8 and z[k + "__path_cost"].shape == () and z[k + "__path_cost"].dtype == np.float64
        assert h.shape == (n, 3, 17, 4) and _same(z[k], h[np.arange(n), path][:, :, :3])
        want = ref.select_all(h, None, 0.05, 0.1)
        if want[3][0] >= 1e-8 * max(1.0, abs(want[2][0])):                # (an untrained model's hypotheses: compared exactly only where no path ties)
            assert np.array_equal(path, want[0])
        assert _cost_ok(z[k + "__path_cost"][None], want[2])

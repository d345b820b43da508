"""Fusing a take's views along time on the device: mp_lift_fuse_path against the float64 statement of its rule (lift_fuse_path_ref.py), what it
reduces to (mp_lift_fuse without a motion term, mp_lift_path with one view), the mirrored scene the feature is for, the exact rules (NaN, ties,
gaps), the invariants (identical bits, takes alone and together, inputs untouched), argument errors, and run.lift with lift.fuse_path end to end.

choice and ok are compared for equality: test_lift_fuse_path_host.py shows that in every scene compared here the best path leads every path that
differs from it in a valid digit by at least 1e-8 max(1, |cost|), and that no table entry and no frame cost is near 1e30; the kernel and the
statement add the same numbers in the same order (fp64 without contraction), only log may differ by an ulp.  path_cost: 1e-12 relative.  pose, cost
and spread: |x - x64| <= 2^-23 max(1, |x64|), test_gpu_lift_fuse.py's bound for the same quantities (lift_place_ref.TOL).
Chunks: the backtrack walks at most MP_LIFT_FUSE_PATH_CHUNK = 512 frames at a time (lift_fuse_path_ref.CHUNK), fewer where 512 frames of
back-pointers pass the workgroup's LDS (4096 states: 9 frames, so the 12-frame case crosses a chunk as well); the forward pass prefetches one
frame's row at a time.  The long take has 1100 frames: two whole chunks and 76 frames."""
import os
import sys

import numpy as np
import pytest
import torch

import lift_fuse_path_ref as ref
import lift_fuse_ref as fuse_ref
import lift_place_ref as place
from lift_fixtures import same as _same

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hpe"))
KEYS = ("pose", "choice", "cost", "spread", "ok", "path_cost")


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _path(hyps, quat=None, valid=None, off=None, sigma=0.02, score_weight=1.0, path_sigma=0.02, switch_cost=0.0):
    from manipose_amd import fuse_views_path
    res = fuse_views_path(_dev(hyps), quat, _dev(valid), off, sigma, score_weight, path_sigma, switch_cost)
    torch.cuda.synchronize()
    return dict(zip(KEYS, (r.cpu().numpy() for r in res)))


def _check(tag, got, want):
    print(f"[{tag}] worst error = {place.worst(got, want):.3f} x the bound 2^-23 max(1, |x|)")
    assert place.within(got, want).all(), tag


def _compare(tag, got, want, valid=None):
    assert np.array_equal(got["choice"], want["choice"]) and np.array_equal(got["ok"], want["ok"]), tag
    rel = np.abs(got["path_cost"] - want["path_cost"]) / np.maximum(np.abs(want["path_cost"]), 1e-300)
    print(f"[{tag}] path_cost within {rel.max():.2e} relative")
    assert (rel <= 1e-12).all(), tag
    for k in ("pose", "cost", "spread"):
        _check(f"{tag}: {k}", got[k], want[k])
    assert not got["pose"][:, 0].any() and not np.signbit(got["pose"][:, 0]).any()                # joint 0 is +0
    if valid is not None:
        assert np.array_equal(got["choice"] == 255, valid.T == 0)


@pytest.mark.parametrize("n", range(34))
def test_path_matches_the_statement(n):
    """n < 32: (V, K, C) in (4,5,4), (3,2,3), (1,5,4), (2,8,4) on takes of 1, 6 and 37 frames, with and without quat, with and without a valid table,
    at two (path_sigma, switch_cost); 32: (4,8,4), 4096 states, on 12 frames; 33: (2,2,4) on 1100 frames"""
    tag, hyps, quat, valid, off, ps, sw, want = ref.path_cases()[n]
    got = _path(hyps, quat, valid, off, path_sigma=ps, switch_cost=sw)
    assert want["written"].all()
    _compare(tag, got, want, valid)


def test_without_a_motion_term_the_choice_is_fuse_views():
    from manipose_amd import fuse_views
    for n in (0, 3, 9, 30):                                                   # (scenes of the statement test: their per-frame gaps are not zero)
        _, hyps, quat, valid, off, _, _, _ = ref.path_cases()[n]
        got = _path(hyps, quat, valid, off, path_sigma=float("inf"), switch_cost=0.0)
        want = fuse_views(_dev(hyps), quat, _dev(valid), off)
        torch.cuda.synchronize()
        assert np.array_equal(got["choice"], want[1].cpu().numpy()) and np.array_equal(got["ok"], want[4].cpu().numpy())
        _check("pose against fuse_views", got["pose"], want[0].double().cpu().numpy())


def test_one_view_is_select_path():
    """V = 1, no orientation, score_weight = 1, joint 0 exactly 0: mp_lift_path's problem, and its answer byte for byte"""
    from manipose_amd import select_path
    g = np.random.default_rng(7)
    off = np.array([0, 1, 7, 44, 600], np.int64)
    hyps = (0.3 * g.standard_normal((600, 5, 17, 4))).astype(np.float32)
    walk = np.cumsum(0.01 * g.standard_normal((600, 1, 17, 3)), axis=0)
    hyps[..., :3] = (walk + 0.02 * g.standard_normal((600, 5, 17, 3))).astype(np.float32)
    hyps[:, :, 0, :3] = 0
    hyps[..., 3] = g.dirichlet(np.ones(5), 600)[:, :, None]
    for ps, sw in ((0.02, 0.0), (0.05, 0.7)):
        poses, path, cost = select_path(_dev(hyps), off, ps, sw)
        got = _path(hyps[None], None, None, off, path_sigma=ps, switch_cost=sw)
        torch.cuda.synchronize()
        assert _same(got["choice"][:, 0], path.cpu().numpy()) and _same(got["path_cost"], cost.cpu().numpy())
        assert _same(got["pose"], poses.cpu().numpy()) and got["ok"].all()
        assert len(set(path.cpu().numpy().tolist())) > 1


def test_mirrored_scene_on_the_device():
    from manipose_amd import fuse_views
    sc = ref.mirror_scene()
    per_frame = fuse_views(_dev(sc["hyps"]), sc["quat"], None, sc["off"])[1].cpu().numpy()
    wrong = int((per_frame != sc["truth"]).any(axis=1).sum())
    print(f"[mirror] fuse_views is wrong in {wrong} of 60 frames")
    assert wrong >= 20
    for sw in (0.0, 0.5, 2.0):
        got = _path(sc["hyps"], sc["quat"], None, sc["off"], switch_cost=sw)
        assert np.array_equal(got["choice"], sc["truth"]) and got["ok"].all(), sw


def test_exact_rules():
    hyps, quat, off = fuse_ref.fuse_scene(4, 5, 4, lens=[9], seed=131)
    clean = _path(hyps, quat, None, off, path_sigma=0.2)
    nan = hyps.copy()
    f, v = 4, 2
    k = int(clean["choice"][f, v])
    nan[v, f, k, 5, 1] = np.nan                                               # the hypothesis the path went through gets a NaN coordinate
    got = _path(nan, quat, None, off, path_sigma=0.2)
    assert got["choice"][f, v] != k and got["ok"].all() and np.isfinite(got["pose"]).all() and got["path_cost"][0] < 1e29
    want = ref.path_all(nan, quat, None, off, path_sigma=0.2)
    assert want["subs"] > 0 and want["margin"][0] >= 1e-8 * max(1.0, abs(want["path_cost"][0])) and np.array_equal(got["choice"], want["choice"])
    # score ties without a motion term: every view's hypotheses alike in score and the views blind to each other -> the first combination
    tie = hyps.copy()
    tie[..., 3] = 0.5
    got = _path(tie, quat, None, off, sigma=float("inf"), path_sigma=float("inf"))
    assert not got["choice"].any() and got["ok"].all()
    two = hyps.copy()
    two[..., 3] = 0.1
    two[:, :, 2:4, :, 3] = 0.5                                                # hypotheses 2 and 3 tie for the best score: 2 is taken
    got = _path(two, quat, None, off, sigma=float("inf"), path_sigma=float("inf"))
    assert (got["choice"] == 2).all()
    # a view invalid in the middle of the take
    valid = np.ones((4, 9), np.uint8)
    valid[1, 3:6] = 0
    valid[:, 7] = 0                                                           # and a frame without any view
    got = _path(hyps, quat, valid, off, path_sigma=0.2, switch_cost=0.3)
    want = ref.path_all(hyps, quat, valid, off, path_sigma=0.2, switch_cost=0.3)
    assert want["margin"][0] >= 1e-8 * max(1.0, abs(want["path_cost"][0]))
    _compare("gap", got, want, valid)
    assert (got["choice"][3:6, 1] == 255).all() and (got["choice"][7] == 255).all() and got["ok"][7] == 0
    assert not got["pose"][7].any() and got["cost"][7] == 0 and got["spread"][7] == 0
    spoiled = hyps.copy()
    spoiled[valid == 0] = np.nan                                              # an invalid view's data is never looked at
    again = _path(spoiled, quat, valid, off, path_sigma=0.2, switch_cost=0.3)
    assert all(_same(again[k], got[k]) for k in KEYS)


def test_invariants():
    from manipose_amd import fuse_views_path
    hyps, quat, off = fuse_ref.fuse_scene(4, 5, 4, seed=141)
    valid = fuse_ref.valid_table(4, off, 141)
    d_hyps = _dev(hyps)
    a = fuse_views_path(d_hyps, quat, _dev(valid), off, path_sigma=0.2, switch_cost=0.4)
    b = fuse_views_path(d_hyps, quat, _dev(valid), off, path_sigma=0.2, switch_cost=0.4)
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and _same(d_hyps.cpu().numpy(), hyps)    # identical bits; the input is unchanged
    for t in range(3):                                                        # a take alone: the bits it has among the others
        sl = slice(int(off[t]), int(off[t + 1]))
        alone = _path(hyps[:, sl], quat[t:t + 1], valid[:, sl], None, path_sigma=0.2, switch_cost=0.4)
        assert all(_same(alone[k], x[sl].cpu().numpy()) for k, x in zip(KEYS[:5], a))
        assert _same(alone["path_cost"], a[5][t:t + 1].cpu().numpy())
    # a frame that no take holds is not written; an empty take costs 0
    from manipose_amd.lift_views import _fuse_path
    from manipose_amd import _lib
    part = _dev(np.array([0, 6, 6, 30], np.int64))
    res = _fuse_path(_lib.load(), d_hyps, None, part, 3, _dev(np.ascontiguousarray(quat)), 0.02, 1.0, 0.2, 0.4)
    torch.cuda.synchronize()
    assert res[5][1].item() == 0 and res[5][0].item() > 0 and res[5][2].item() > 0
    assert bool((res[1][:30] < 5).all())


def test_entry_point_rejects_bad_arguments_before_any_launch(lib):
    V, F, K, J = 4, 6, 5, 17
    hyps = torch.zeros(V, F, K, J, 4, device="cuda")
    off = torch.tensor([0, F], dtype=torch.int64, device="cuda")
    quat = _dev(fuse_ref.s11_tables()[0])
    pose, cost, spread = torch.full((F, J, 3), -1.0, device="cuda"), torch.full((F,), -1.0, device="cuda"), torch.full((F,), -1.0, device="cuda")
    choice, ok = (torch.full(s, 7, dtype=torch.uint8, device="cuda") for s in ((F, V), (F,)))
    pc = torch.full((1,), -1.0, dtype=torch.float64, device="cuda")
    need = int(lib.mp_lift_fuse_path_scratch_bytes(V, F, K))
    assert need == ref.scratch_bytes(V, F, K) and need % 8 == 0
    for v, f, k in ((1, 7, 1), (2, 1000, 8), (3, 37, 2), (4, 3000, 5), (4, 12, 8)):
        assert int(lib.mp_lift_fuse_path_scratch_bytes(v, f, k)) == ref.scratch_bytes(v, f, k)
    for v, f, k in ((0, 6, 5), (5, 6, 5), (4, 0, 5), (4, 6, 0), (4, 6, 9)):
        assert int(lib.mp_lift_fuse_path_scratch_bytes(v, f, k)) == 0
    scratch = torch.zeros(need // 8 + 1, dtype=torch.float64, device="cuda")
    p = lambda x: None if x is None else x.data_ptr()

    def run(h=hyps, o=off, q=quat, out=pose, c=choice, e=cost, s=spread, g=ok, pcost=pc, sc=scratch.data_ptr(), nb=need, v=V, f=F, k=K, j=J, ch=4,
            G=1, sigma=0.02, w=1.0, ps=0.02, sw=0.0):
        return lib.mp_lift_fuse_path(p(h), v, f, k, j, ch, None, p(o), G, p(q), sigma, w, ps, sw, p(out), p(c), p(e), p(s), p(g), p(pcost), sc, nb, None)
    for kw in (dict(h=None), dict(o=None), dict(out=None), dict(c=None), dict(e=None), dict(s=None), dict(g=None), dict(pcost=None), dict(sc=None)):
        assert run(**kw) == 1 and b"null" in lib.mp_last_error()
    for kw, word in ((dict(v=0), b"V=0"), (dict(v=5), b"V=5"), (dict(k=0), b"K=0"), (dict(k=9), b"K=9"), (dict(j=1), b"J=1"), (dict(j=33), b"J=33"),
                     (dict(ch=2), b"C=2"), (dict(ch=5), b"C=5"), (dict(f=0), b"out of range"), (dict(f=-1), b"out of range"), (dict(G=0), b"out of range"),
                     (dict(G=7), b"out of range"), (dict(sigma=0.0), b"sigma"), (dict(sigma=float("nan")), b"sigma"),
                     (dict(w=-1.0), b"score_weight"), (dict(w=float("inf")), b"score_weight"),
                     (dict(ps=0.0), b"path_sigma"), (dict(ps=-1.0), b"path_sigma"), (dict(ps=float("nan")), b"path_sigma"),
                     (dict(sw=-1.0), b"switch_cost"), (dict(sw=float("inf")), b"switch_cost"), (dict(sw=float("nan")), b"switch_cost"),
                     (dict(f=2 ** 41), b"too many for one launch"), (dict(nb=need - 8), b"scratch too small"), (dict(nb=0), b"scratch too small"),
                     (dict(sc=scratch.data_ptr() + 4), b"8-byte aligned")):
        assert run(**kw) == 1 and word in lib.mp_last_error(), (kw, lib.mp_last_error())
    torch.cuda.synchronize()
    for t in (pose, cost, spread, pc):
        assert bool((t == -1).all())                                          # nothing was launched
    assert bool((choice == 7).all()) and bool((ok == 7).all())
    assert run() == 0 and run(q=None) == 0 and run(sigma=float("inf"), w=0.0, ps=float("inf")) == 0       # good arguments; quat may be null
    torch.cuda.synchronize()
    assert bool((choice == 0).all()) and bool((ok == 1).all()) and bool((pose == 0).all()) and bool((spread == 0).all()) and pc.item() != -1
    from manipose_amd import fuse_views_path
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fuse_views_path(hyps.cpu())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fuse_views_path(hyps, valid=torch.ones(V, F, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="out of range"):
        fuse_views_path(hyps, take_offset=list(range(F + 2)))                 # more takes than frames: the entry point's own refusal


def test_fuse_path_entry_point_in_synthetic_mode(lib, tmp_path, monkeypatch):
    """run.lift with lift.fuse and lift.fuse_path on synthetic data (every take has one view): __path_cost is written and __choice is
    fuse_views_path's on the hypotheses the run wrote; without lift.fuse_path the file has no such key"""
    from _entry import run
    from manipose_amd import fuse_views_path
    monkeypatch.chdir(tmp_path)
    argv = ["run.train=false", "run.test=false", "run.lift=true", "lift.stride=14", "train.batch_size_test=4", "data.seq_len=27", "model.channels=64",
            "model.layers=2", "model.nheads=4", "model.channels_seg=32", "model.layers_seg=1", "model.nheads_seg=4", "multi_hyp.n_hyp=3",
            "data.synthetic_sequences=2", "model.precision=fp32", "lift.hyps=true", "train.tta=false", "lift.fuse=true"]
    out = os.path.join(str(tmp_path), "default", "lift.npz")
    run(argv)
    before = dict(np.load(out))
    assert not any(k.endswith("__path_cost") for k in before)
    run(argv + ["lift.fuse_path=true", "lift.fuse_path_switch=0.25"])
    z = dict(np.load(out))
    assert sorted(set(z) - set(before)) == [f"synthetic_{i:03d}.fused0__path_cost" for i in range(2)]
    for i in range(2):
        k = f"synthetic_{i:03d}"
        assert all(_same(z[f], v) for f, v in before.items() if f.startswith(k) and ".fused" not in f)
        want = fuse_views_path(_dev(z[f"{k}__hyps"][None]), _quat_of(i), None, None, 0.02, 1.0, 0.02, 0.25)
        torch.cuda.synchronize()
        assert _same(z[f"{k}.fused0__choice"], want[1].cpu().numpy())
        assert z[f"{k}.fused0__path_cost"].shape == () and z[f"{k}.fused0__path_cost"] == want[5].cpu().numpy()[0]


def _quat_of(i):
    """synthetic-data mode: sequence i gets camera i % 4 of S11"""
    from manipose_amd.data.ingest import h36m_cameras
    return np.asarray(h36m_cameras()["S11"][i % 4]["orientation"], np.float32)[None]
